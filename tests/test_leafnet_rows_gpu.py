"""bk_leafnet_x3_rows (the leaf net over the arena's rows, a weight set per row) against
bk_leafnet_x3_states / bk_leafnet_x3_np_states on the same states with each net: every live row
bitwise the states entry's row for its net, every other row of pf / vout untouched (a sentinel).
Rows: a shuffled tree_of_row with -1 holes, uninformed seats, budgets above and below `sim`, trees
whose status is not 1."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
SIM = 3


@functools.lru_cache(maxsize=None)
def _engine(N, P):
    from blokus_rl_amd.engine import Engine

    return Engine(N, 4 if P == 3 else P, 5)  # the engine plays 2 or 4 players (3: see _states)


def _leaf3(net):
    """A 3-player net on the np kernel. LeafResNet packs the split-f16 operands only for the stems
    its f32 kernels take (4 or 8 planes); the np kernel itself takes any P <= 4, so pack them here."""
    from blokus_rl_amd.nets import FusedResNet, LeafResNet

    class Leaf3(LeafResNet):
        def __init__(self, net):
            torch.nn.Module.__init__(self)
            self.x3_boards, self.normalize, self.features, self.native, self.x3 = "all", False, True, False, True
            self.f = FusedResNet(net).eval()
            convs = [c for blk in self.f.blocks for c in blk]
            self.register_buffer("b_tower", torch.cat([c.bias.detach().float() for c in convs]).contiguous())
            self._register_x3(convs)

    return Leaf3(net).eval()


@functools.lru_cache(maxsize=None)
def _nets(N, P, blocks=(1, 1, 1)):
    """Three 1-block ResNets with different seeds (non-trivial BN statistics) as LeafResNets."""
    from blokus_rl_amd.nets import LeafResNet, ResNet

    out = []
    for k, nb in enumerate(blocks):
        torch.manual_seed(100 * N + 10 * P + k)
        net = ResNet(N, P, 100, nb).cuda().eval()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.uniform_(-0.2, 0.2)
                    m.running_var.uniform_(0.5, 1.5)
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.1, 0.1)
        leaf = _leaf3(net) if P == 3 else LeafResNet(net, normalize=False, features=True, x3_boards="all").eval()
        assert leaf.takes_states()
        out.append(leaf)
    return out


@functools.lru_cache(maxsize=None)
def _states(N, P, T):
    """T states of random play stopped at plies spread over a game (0 .. most of a game)."""
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import W_TO_MOVE

    eng = _engine(N, P)
    states = random_boards(eng, T, seed0=5, max_plies=3 * P * eng.num_pieces // 4).contiguous()
    if P == 3:  # a 4-player game's boards without colour 3: rows of planes 0..2, movers 0..2
        w = states.view(torch.int32)
        w[:, 3 * 20:4 * 20] = 0
        w[:, W_TO_MOVE] %= 3
        assert set(w[:, W_TO_MOVE].tolist()) == {0, 1, 2}
    return states


@functools.lru_cache(maxsize=None)
def _reference(N, P, T):
    """leafnet_x3_states(states, all ones, model_k) for the three nets, computed once."""
    from blokus_rl_amd.nets import leafnet_x3_states

    ones = torch.ones(T, dtype=torch.int32, device="cuda")
    ref = [leafnet_x3_states(_states(N, P, T), ones, m) for m in _nets(N, P)]
    for pf, v in ref:
        assert torch.isfinite(pf).all() and torch.isfinite(v).all()
    assert not torch.equal(ref[0][0], ref[1][0]) and not torch.equal(ref[1][1], ref[2][1])
    return ref


def _tables(R, T, seed):
    """Row tables over T trees: the kinds cycle with period 8, so R >= 7 holds every kind."""
    rng = np.random.default_rng(seed)
    tree = rng.permutation(T)[:R].astype(np.int32)
    net = (np.arange(R) % 3).astype(np.int32)
    sims = np.full(R, SIM + 2, dtype=np.int32)
    status = np.ones(T, dtype=np.int32)
    kind = np.array(["live"] * R, dtype=object)
    if R >= 5:
        for r in range(R):
            k = r % 8
            if k == 3:
                kind[r] = "dead"
            elif k == 4:
                kind[r] = "uninformed"
            elif k == 5:
                kind[r] = "status"
            elif k == 6:
                kind[r] = "budget"
    for r in range(R):
        if kind[r] == "status":
            status[tree[r]] = (0, 2, -1)[r % 3]
        elif kind[r] == "uninformed":
            net[r] = -1
        elif kind[r] == "budget":
            sims[r] = (SIM, SIM - 1, 0)[r % 3]  # sim >= budget
    tree_dev = tree.copy()
    tree_dev[kind == "dead"] = -1
    return tree, tree_dev, net, sims, status, kind


def _run(N, P, R, T, seed=0):
    from blokus_rl_amd.engine import arena_rows
    from blokus_rl_amd.nets import leafnet_x3_rows, leafnet_x3_table

    nets, ref = _nets(N, P), _reference(N, P, T)
    states = _states(N, P, T)
    tree, tree_dev, net, sims, status, kind = _tables(R, T, seed)
    dev = states.device
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    tabs = (t(tree_dev), t(net), t(sims))
    status_d = t(status)
    pf = torch.full((T, 2 * N * N), SENTINEL, dtype=torch.float32, device=dev)
    v = torch.full((T, P), SENTINEL, dtype=torch.float32, device=dev)
    table = leafnet_x3_table(nets, pf, v, states, status_d)
    leafnet_x3_rows(table, arena_rows(*tabs, T), SIM, dev)
    torch.cuda.synchronize()
    live_trees = set()
    for r in range(R):
        if kind[r] != "live":
            continue
        tr, k = int(tree[r]), int(net[r])
        live_trees.add(tr)
        assert torch.equal(pf[tr], ref[k][0][tr]), (r, tr, k)
        assert torch.equal(v[tr], ref[k][1][tr]), (r, tr, k)
    rest = torch.tensor(sorted(set(range(T)) - live_trees), dtype=torch.long, device=dev)
    assert bool((pf[rest] == SENTINEL).all()) and bool((v[rest] == SENTINEL).all())
    return kind, net


@pytest.mark.parametrize("N,P,R,T", [(20, 4, 37, 148), (14, 4, 5, 12), (7, 2, 37, 74), (20, 3, 37, 111)])
def test_rows_equal_states_entry_per_net(N, P, R, T):
    nets = _nets(N, P)
    assert nets[0].x3_entry(N) == ("classic" if P == 4 and N in (14, 20) else "np")
    kind, net = _run(N, P, R, T)
    if R >= 8:  # the corpus holds a row of every kind, and every net evaluates some live row
        assert {"live", "dead", "uninformed", "status", "budget"} <= set(kind.tolist())
        assert {int(net[r]) for r in range(R) if kind[r] == "live"} == {0, 1, 2}


@pytest.mark.parametrize("N,P", [(20, 4), (7, 2)])
def test_single_row(N, P):
    T = 148 if N == 20 else 74
    for seed in (1, 2):
        _run(N, P, 1, T, seed)


def test_mismatched_net_table_is_einval():
    from blokus_rl_amd.engine import LeafnetArgs, arena_rows, load_library
    from blokus_rl_amd.nets import leafnet_x3_args, leafnet_x3_table

    N, P, T = 20, 4, 148
    nets = _nets(N, P)
    deep = _nets(N, P, blocks=(2, 1, 1))[0]
    states = _states(N, P, T)
    dev = states.device
    status = torch.ones(T, dtype=torch.int32, device=dev)
    pf = torch.full((T, 2 * N * N), SENTINEL, dtype=torch.float32, device=dev)
    v = torch.full((T, P), SENTINEL, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        leafnet_x3_table([nets[0], deep], pf, v, states, status)
    table = (LeafnetArgs * 2)()
    table[0] = leafnet_x3_args(nets[0], pf, v, states=states, status=status)
    table[1] = leafnet_x3_args(deep, pf, v, states=states, status=status)
    assert table[0].nlayers != table[1].nlayers
    tabs = [torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(3)]
    tabs[2] += 5
    lib = load_library()
    rc = lib.bk_leafnet_x3_rows(table, 2, ctypes.byref(arena_rows(*tabs, T)), 0, None)
    assert rc == -1 and b"bk_leafnet_x3_rows" in lib.bk_last_error()
    # a planar-form entry and more nets than the table holds are refused as well
    table[1] = leafnet_x3_args(nets[1], pf, v, obs=torch.zeros((T, 2 * P, N, N), device=dev))
    assert lib.bk_leafnet_x3_rows(table, 2, ctypes.byref(arena_rows(*tabs, T)), 0, None) == -1
    assert lib.bk_leafnet_x3_rows(table, 5, ctypes.byref(arena_rows(*tabs, T)), 0, None) == -1
    torch.cuda.synchronize()
    assert bool((pf == SENTINEL).all()) and bool((v == SENTINEL).all())
