"""k_leafnet_x3<20>'s edge schedule (BK_LN_EDGE=1, the default: four pixel groups that each hold 16
pixels of one board edge skip the K chunks whose 3x3 tap lies wholly in the zero halo) against the
full schedule on the old pixel map (BK_LN_EDGE=0). A skipped chunk adds only a * 0 products, whose
sum is +-0, to an accumulator that is never -0, so every output is bitwise what it was:
torch.equal on the policy features, the values and the tower output (the tower output is written
pixel by pixel through the map, so it also shows every pixel goes back to its own place).

The engine entries are called directly: the knob is read per launch, and no captured graph fixes
it. Dense inputs are non-zero at every pixel, edges and corners included, so a tap skipped wrongly
or a pixel mapped wrongly changes a value."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _leaf(N, nblocks):
    """Dense random weights; every folded bias non-zero (BN statistics and affine drawn at random)."""
    from blokus_rl_amd.nets import LeafResNet, ResNet

    torch.manual_seed(31 * N + nblocks)
    net = ResNet(N, 4, 100, nblocks).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.1, 0.1)
    leaf = LeafResNet(net, normalize=False, features=True).eval()
    assert leaf.x3 and leaf.x3_entry(N) == "classic"
    assert bool((leaf.x3_heads[0] != 0).all()) and bool((leaf.b_tower != 0).all())
    return leaf


def _both(monkeypatch, fn):
    """fn() under BK_LN_EDGE=1 and under BK_LN_EDGE=0."""
    res = []
    for knob in ("1", "0"):
        monkeypatch.setenv("BK_LN_EDGE", knob)
        res.append(fn())
        torch.cuda.synchronize()
    return res


def _assert_same(edge, full):
    for a, b, name in zip(edge, full, ("pf", "v", "xout")):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("nblocks", [1, 2])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_planes_form_is_bitwise_the_full_schedule(monkeypatch, B, nblocks):
    from blokus_rl_amd.nets import leafnet_x3

    leaf = _leaf(20, nblocks)
    g = torch.Generator(device="cuda").manual_seed(100 * B + nblocks)
    obs = torch.randn((B, 8, 20, 20), device="cuda", generator=g)
    obs = torch.where(obs.abs() < 0.05, torch.full_like(obs, 0.05), obs)  # non-zero at every pixel
    assert bool((obs != 0).all())
    edge, full = _both(monkeypatch, lambda: leafnet_x3(obs, leaf, want_out=True))
    _assert_same(edge, full)
    assert bool((full[2] != 0).any(dim=1).all())  # every pixel of the tower output carries a value


@functools.lru_cache(maxsize=None)
def _states():
    """Packed 20x20 states: random playouts, the empty board, and a board whose every border cell
    is occupied (player 0's rows written into the state words: the net reads only the row words
    and the mover)."""
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine

    eng = Engine(20, 4, 5)
    played = random_boards(eng, 7, seed0=3, max_plies=60)
    empty = eng.init_states(1)
    border = eng.init_states(1).clone()
    words = border.view(torch.int32)  # plane p, row r = word 20 p + r
    rows = torch.full((20,), (1 << 19) | 1, dtype=torch.int32)
    rows[0] = rows[19] = (1 << 20) - 1
    words[0, :20] = rows.to(words.device)
    assert torch.equal(eng.observe(border)[0, 0] != 0,
                       torch.nn.functional.pad(torch.zeros(18, 18, device=eng.device), (1, 1, 1, 1), value=1.0) != 0)
    return torch.cat([played, empty, border]).contiguous()


@pytest.mark.parametrize("nblocks", [1, 2])
def test_states_form_is_bitwise_the_full_schedule(monkeypatch, nblocks):
    from blokus_rl_amd.nets import leafnet_x3_states

    leaf, states = _leaf(20, nblocks), _states()
    edge, full = _both(monkeypatch, lambda: leafnet_x3_states(states, None, leaf, want_out=True))
    _assert_same(edge, full)
    # one row that is no leaf (status != 1): evaluated as the all-zero observation in both
    status = torch.ones(states.shape[0], dtype=torch.int32, device=states.device)
    status[2] = 0
    edge, full = _both(monkeypatch, lambda: leafnet_x3_states(states, status, leaf, want_out=True))
    _assert_same(edge, full)
    assert not torch.equal(full[0][2], full[0][1])


def test_knob_changes_nothing_on_14x14(monkeypatch):
    from blokus_rl_amd.nets import leafnet_x3

    leaf = _leaf(14, 1)
    g = torch.Generator(device="cuda").manual_seed(14)
    obs = torch.randn((3, 8, 14, 14), device="cuda", generator=g)
    edge, full = _both(monkeypatch, lambda: leafnet_x3(obs, leaf, want_out=True))
    _assert_same(edge, full)
