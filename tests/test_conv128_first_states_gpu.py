"""bk_conv128_first_states (nets.conv128_first_states): DCNNet's first layer read from packed
states is bitwise bk_conv128_first on bk_observe's planes; rows whose status is not 1 are the
all-zero observation and their bytes are not read; a board's output does not depend on its batch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(7, 2, 5), (14, 2, 3), (20, 4, 3), (20, 3, 2)]


def _observe(states, N, P):
    """bk_observe's planes from the packed states in torch (k_observe, env.hip): plane p < P at
    (r, c) = bit c of word 20 p + r, plane P + q all ones iff q == the to-move word."""
    from blokus_rl_amd.engine import W_TO_MOVE

    B = states.shape[0]
    words = states.view(torch.int32)
    rows = words[:, :20 * P].view(B, P, 20)[:, :, :N]
    cols = torch.arange(N, device=states.device, dtype=torch.int32)
    pieces = ((rows.unsqueeze(-1) >> cols) & 1).float()
    mover = words[:, W_TO_MOVE].view(B, 1) == torch.arange(P, device=states.device).view(1, P)
    return torch.cat([pieces, mover.float().view(B, P, 1, 1).expand(B, P, N, N)], dim=1).contiguous()


def _setup(N, P, B):
    """(planes, states, weights, bias). The engine has 2- and 4-player presets; the kernel also takes
    3 players, whose states here are 4-player boards read as 3 players' (planes 0..2, the mover
    folded into 0..2) and whose planes are _observe's, which is checked against bk_observe where
    the engine exists."""
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import W_TO_MOVE, Engine

    eng = Engine(N, P if P != 3 else 4, 5)
    states = random_boards(eng, B, seed0=100 * N + P, max_plies=30).contiguous()
    if P == 3:
        states.view(torch.int32)[:, W_TO_MOVE] %= 3
    else:
        assert torch.equal(_observe(states, N, P), eng.observe(states))
    g = torch.Generator(device="cuda").manual_seed(N + 7 * P)
    w = torch.randn((128, 2 * P, 3, 3), device="cuda", generator=g) * 0.3
    bias = torch.randn(128, device="cuda", generator=g)
    return _observe(states, N, P), states, w, bias


@pytest.mark.parametrize("N,P,B", CASES)
def test_first_states_is_bitwise_first_on_the_planes(N, P, B):
    from blokus_rl_amd.nets import conv128_first, conv128_first_states

    obs, states, w, bias = _setup(N, P, B)
    assert obs[:, :P].sum() > 0 and obs[:, P:].sum() == B * N * N and tuple(obs.shape) == (B, 2 * P, N, N)
    for relu in (False, True):
        for b in (bias, None):
            ref = conv128_first(obs, w, b, relu)
            y = conv128_first_states(states, None, N, P, w, b, relu)
            assert tuple(y.shape) == (B, N, N, 128) and torch.equal(y, ref), (relu, b is None)
    # the raw-address form (the search's own buffer): B from the status
    ref = conv128_first(obs, w, bias, True)
    ones = torch.ones(B, dtype=torch.int32, device="cuda")
    assert torch.equal(conv128_first_states(states.data_ptr(), ones, N, P, w, bias, True), ref)
    # an empty batch
    y0 = conv128_first_states(states[:0].contiguous(), None, N, P, w, bias, True)
    assert tuple(y0.shape) == (0, N, N, 128)


@pytest.mark.parametrize("N,P,B", CASES)
def test_rows_whose_status_is_not_1_are_the_zero_observation(N, P, B):
    from blokus_rl_amd.nets import conv128_first, conv128_first_states

    obs, states, w, bias = _setup(N, P, B)
    status = torch.ones(B, dtype=torch.int32, device="cuda")
    status[0], status[B - 1] = 0, 2
    dead = status != 1
    full = conv128_first(obs, w, bias, True)
    zero = conv128_first(torch.zeros((1, 2 * P, N, N), device="cuda"), w, bias, True)
    assert torch.equal(zero[0], torch.relu(bias).expand(N, N, 128))
    poisoned = states.clone()
    poisoned[dead] = 0xFF
    for src in (poisoned, poisoned.data_ptr()):
        y = conv128_first_states(src, status, N, P, w, bias, True)
        assert torch.equal(y[dead], zero.expand(int(dead.sum()), N, N, 128))
        assert torch.equal(y[~dead], full[~dead])
    # without a bias and a ReLU the dead rows are exactly zero
    y = conv128_first_states(poisoned, status, N, P, w, None, False)
    assert not y[dead].any()


@pytest.mark.parametrize("N,P,B", CASES)
def test_a_board_does_not_depend_on_its_batch(N, P, B):
    from blokus_rl_amd.nets import conv128_first_states

    _, states, w, bias = _setup(N, P, B)
    y = conv128_first_states(states, None, N, P, w, bias, True)
    for i in range(B):
        alone = conv128_first_states(states[i:i + 1].contiguous(), None, N, P, w, bias, True)
        assert torch.equal(alone[0], y[i]), i
    # a batch that starts at a non-zero row of the buffer
    tail = conv128_first_states(states.data_ptr() + 384, torch.ones(B - 1, dtype=torch.int32, device="cuda"), N, P,
                                w, bias, True)
    assert torch.equal(tail, y[1:])


def test_bad_arguments_are_refused():
    from blokus_rl_amd.engine import EngineError, load_library
    from blokus_rl_amd.nets import conv128_first_states

    _, states, w, bias = _setup(7, 2, 2)
    with pytest.raises(EngineError):
        conv128_first_states(states, None, 8, 2, w, bias)  # board size
    with pytest.raises(ValueError):
        conv128_first_states(states, None, 7, 3, w, bias)  # the weights are 2 players'
    with pytest.raises(ValueError):
        conv128_first_states(states.data_ptr(), None, 7, 2, w, bias)  # an address without a batch size
    lib = load_library()
    assert lib.bk_conv128_first_states(None, None, 0, 7, 2, ctypes.c_void_p(w.data_ptr()), None, 0, None, None) == 0
    assert lib.bk_conv128_first_states(None, None, 0, 7, 5, ctypes.c_void_p(w.data_ptr()), None, 0, None, None) != 0
