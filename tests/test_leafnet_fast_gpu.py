"""k_leafnet_x3 with BK_LN_FAST=1 (the default: binary planes on the two-product stem, the halo
zeroed from per-thread slots, the state words loaded beside status[b], the one-pass stem epilogue,
the value head's stores after its reductions) against BK_LN_FAST=0 (the code without them) in one
process: pf, v and the tower output bitwise equal (torch.equal) for the planes, states and rows
forms. The knob is read per launch. Which stem a planes board took is read from the kernel's path
counters (bk_ln_path_counts), not from timing."""
import contextlib
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

POOL = 65
PLIES = {20: (0, 5, 40), 14: (0, 5, 20)}  # random_boards' max_plies per third of the pool


@contextlib.contextmanager
def _fast(on):
    old = os.environ.get("BK_LN_FAST")
    os.environ["BK_LN_FAST"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["BK_LN_FAST"]
        else:
            os.environ["BK_LN_FAST"] = old


def _path_counts(enable):
    """(binary, full) stems taken by planes workgroups since the last call; then clear, and count on/off."""
    from blokus_rl_amd.engine import load_library

    c = (ctypes.c_uint * 2)()
    assert load_library().bk_ln_path_counts(1 if enable else 0, c) == 0
    return int(c[0]), int(c[1])


@functools.lru_cache(maxsize=None)
def _engine(N):
    from blokus_rl_amd.engine import Engine

    return Engine(N, 4, 5)


@functools.lru_cache(maxsize=None)
def _leaf(N, seed=0, x3_boards=None):
    from blokus_rl_amd.nets import LeafResNet, build_model

    torch.manual_seed(31 + N + 1000 * seed)
    net = build_model("resnet", N, 4, _engine(N).A, num_res_blocks=2).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.1, 0.1)
    kw = {} if x3_boards is None else {"x3_boards": x3_boards}
    leaf = LeafResNet(net, normalize=False, features=True, **kw).eval()
    assert leaf.x3
    return leaf


@functools.lru_cache(maxsize=None)
def _states(N):
    """POOL states: random_boards at max_plies 0, 5 and 40 (N = 14: 20), shuffled by a fixed permutation."""
    from blokus_rl_amd.boards import random_boards

    eng = _engine(N)
    p0, p1, p2 = PLIES[N]
    parts = [random_boards(eng, 5, seed0=1, max_plies=p0), random_boards(eng, 20, seed0=100, max_plies=p1),
             random_boards(eng, POOL - 25, seed0=200, max_plies=p2)]
    perm = torch.randperm(POOL, generator=torch.Generator().manual_seed(N)).to(eng.device)
    return torch.cat(parts)[perm].contiguous()


@functools.lru_cache(maxsize=None)
def _obs(N):
    """bk_observe of the pool, row 1 the all-zero observation (what the search writes for a tree
    without a leaf): every value exactly 0.0f or 1.0f."""
    obs = _engine(N).observe(_states(N)).clone()
    obs[1] = 0.0
    assert obs.shape == (POOL, 8, N, N) and bool(((obs == 0.0) | (obs == 1.0)).all())
    assert not bool(torch.signbit(obs).any())
    zero = (obs.flatten(1) == 0.0).all(dim=1)
    assert int(zero.sum()) == 1
    for q in range(4):  # every mover plane is set on some board
        assert bool((obs[:, 4 + q].flatten(1) == 1.0).all(dim=1).any()), q
    return obs.contiguous()


def _not_binary(obs, kind):
    """obs (one board, [8, N, N]) with one value that is not exactly 0.0f / 1.0f: kinds 0..2 change
    one corner cell of one plane, kind 3 is random float planes of magnitudes 1e-6..1e3."""
    N = obs.shape[-1]
    o = obs.clone()
    if kind == 0:
        o[0, 0, 0] = 0.5
    elif kind == 1:
        o[3, 0, N - 1] = 0.0
        o[3, 0, N - 1] *= -1.0  # -0.0f
        assert bool(torch.signbit(o[3, 0, N - 1]))
    elif kind == 2:
        o[6, N - 1, N - 1] = 2.0
    else:
        g = torch.Generator().manual_seed(5)
        mag = torch.pow(10.0, torch.rand(o.shape, generator=g) * 9.0 - 6.0)
        sign = torch.where(torch.rand(o.shape, generator=g) < 0.5, -1.0, 1.0)
        o = (mag * sign).to(obs.device)
        assert float(o.abs().min()) >= 1e-6 and float(o.abs().max()) <= 1e3
    return o


def _both(run):
    """run() under BK_LN_FAST=1 with the path counters on, then under BK_LN_FAST=0: the outputs
    must be bitwise equal; returns (outputs, (binary, full) workgroups of the FAST launch)."""
    _path_counts(True)
    with _fast(True):
        new = run()
    torch.cuda.synchronize()
    counts = _path_counts(True)
    with _fast(False):
        old = run()
    torch.cuda.synchronize()
    assert _path_counts(False) == (0, 0)  # the other code does not count: it is not the FAST kernel
    for a, b in zip(new, old):
        assert torch.isfinite(b).all()
        assert torch.equal(a, b)
    return new, counts


@pytest.mark.parametrize("N,B", [(20, 1), (20, 3), (20, 65), (14, 1), (14, 5)])
def test_planes_binary_boards_take_the_short_stem(N, B):
    from blokus_rl_amd.nets import leafnet_x3, leafnet_x3_states

    obs, leaf = _obs(N)[:B].contiguous(), _leaf(N)
    new, counts = _both(lambda: leafnet_x3(obs, leaf, want_out=True))
    assert counts == (B, 0)
    # the states form (the same two-product stem from the row words) on the same boards
    live = torch.ones(B, dtype=torch.int32, device=obs.device)
    if B > 1:
        live[1] = 0  # row 1 is the all-zero observation
    st = leafnet_x3_states(_states(N)[:B].contiguous(), live, leaf, want_out=True)
    for a, b in zip(new, st):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,B", [(20, 1), (20, 3), (20, 65), (14, 1), (14, 5)])
def test_planes_other_boards_take_the_full_stem(N, B):
    from blokus_rl_amd.nets import leafnet_x3

    leaf = _leaf(N)
    for first in range(4 if B == 1 else 1):  # B = 1: each kind alone
        obs = torch.stack([_not_binary(_obs(N)[i], (first + i) % 4) for i in range(B)]).contiguous()
        _, counts = _both(lambda: leafnet_x3(obs, leaf, want_out=True))
        assert counts == (0, B), first


@pytest.mark.parametrize("N", [20, 14])
def test_mixed_batch_each_board_as_alone(N):
    from blokus_rl_amd.nets import leafnet_x3

    leaf, B = _leaf(N), 8
    obs = torch.stack([_obs(N)[i] if i % 2 == 0 else _not_binary(_obs(N)[i], i // 2) for i in range(B)]).contiguous()
    (pf, v, out), counts = _both(lambda: leafnet_x3(obs, leaf, want_out=True))
    assert counts == (B // 2, B // 2)
    for i in range(B):
        pf1, v1, out1 = leafnet_x3(obs[i:i + 1].contiguous(), leaf, want_out=True)
        assert torch.equal(pf1, pf[i:i + 1]) and torch.equal(v1, v[i:i + 1]) and torch.equal(out1, out[i:i + 1]), i


def _status(B, dev):
    """Leaf statuses with rows that are not leaves (0, 2, -1) on every third row from row 0 (B = 1: row 0)."""
    status = torch.ones(B, dtype=torch.int32, device=dev)
    third = torch.arange(0, B, 3, device=dev)
    status[third] = torch.tensor([0, 2, -1], dtype=torch.int32, device=dev).repeat(B)[: len(third)]
    return status


@pytest.mark.parametrize("N,B", [(20, 1), (20, 3), (20, 65), (14, 5)])
def test_states_form(N, B):
    """Rows that are not leaves hold 0xFF bytes: FAST loads them (beside status[b]) and drops them."""
    from blokus_rl_amd.nets import leafnet_x3, leafnet_x3_states

    eng, leaf = _engine(N), _leaf(N)
    for status in (_status(B, eng.device), torch.ones(B, dtype=torch.int32, device=eng.device), None):
        states = _states(N)[:B].clone()
        obs = eng.observe(states)
        if status is not None:
            states[status != 1] = 0xFF
            obs[status != 1] = 0.0
        new, _ = _both(lambda: leafnet_x3_states(states, status, leaf, want_out=True))
        with _fast(False):
            ref = leafnet_x3(obs.contiguous(), leaf, want_out=True)
        for a, b in zip(new, ref):
            assert torch.equal(a, b)


@pytest.mark.parametrize("N,B", [(20, 1), (20, 3), (20, 65), (14, 5)])
def test_rows_form(N, B):
    """bk_leafnet_x3_rows over B rows of a shuffled tree table, two nets, trees that are not leaves
    (0xFF state rows): FAST equals the other code, live rows equal the states entry, the rest untouched."""
    from blokus_rl_amd.engine import arena_rows
    from blokus_rl_amd.nets import leafnet_x3_rows, leafnet_x3_states, leafnet_x3_table

    eng = _engine(N)
    dev = eng.device
    nets = [_leaf(N, 0, "all"), _leaf(N, 1, "all")]
    status = _status(B, dev) if B > 1 else torch.ones(1, dtype=torch.int32, device=dev)
    states = _states(N)[:B].clone()
    states[status != 1] = 0xFF
    tree = torch.randperm(B, generator=torch.Generator().manual_seed(B)).to(torch.int32).to(dev)
    net = (torch.arange(B, device=dev) % 2).to(torch.int32)
    sims = torch.full((B,), 5, dtype=torch.int32, device=dev)
    rows = arena_rows(tree, net, sims, B)

    def run():
        pf = torch.full((B, 2 * N * N), -12345.0, dtype=torch.float32, device=dev)
        v = torch.full((B, 4), -12345.0, dtype=torch.float32, device=dev)
        leafnet_x3_rows(leafnet_x3_table(nets, pf, v, states, status), rows, 3, dev)
        return pf, v

    # the sentinel rows are finite and equal in both runs
    (pf, v), _ = _both(run)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    for r in range(B):
        t, k = int(tree[r]), int(net[r])
        if int(status[t]) == 1:
            pf1, v1 = leafnet_x3_states(_states(N)[t:t + 1].contiguous(), ones[:1], nets[k])
            assert torch.equal(pf[t:t + 1], pf1) and torch.equal(v[t:t + 1], v1), (r, t, k)
        else:
            assert bool((pf[t] == -12345.0).all()) and bool((v[t] == -12345.0).all())
