"""Tree-range launches (bk_mcts_select_range, bk_mcts_leaf_step_range) against the whole-batch
entries: two range calls that cover [0, T) leave the trees, counters and leaf outputs of one
whole-batch call, bitwise, and a range call touches no tree outside its range."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _leaf_model(eng, blocks=2, seed=0):
    from blokus_rl_amd.nets import LeafResNet, ResNet

    torch.manual_seed(seed)
    net = ResNet(eng.N, eng.P, eng.A, blocks).cuda().eval()
    return LeafResNet(net, normalize=False, features=True).eval()


def _setup(N, T, sims):
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine

    eng = Engine(N, 4, 5)
    model = _leaf_model(eng)
    roots = random_boards(eng, T, seed0=11, max_plies=24 if N == 20 else 12)
    active = torch.ones(T, dtype=torch.int32, device=eng.device)
    active[T // 3] = 0
    kw = dict(node_cap=sims + 8, child_cap=T * (sims + 8) * 700)
    po = model.f.policy_out
    return (eng, model, roots, active, BatchedMCTS(eng, T, **kw), BatchedMCTS(eng, T, **kw),
            po.weight.detach().contiguous(), po.bias.detach().contiguous())


@pytest.mark.parametrize("N,T", [(20, 12), (14, 7)])
def test_range_calls_match_whole_batch(N, T):
    sims, cut = 6, 5
    eng, model, roots, active, m1, m2, w, b = _setup(N, T, sims)
    _, obs1, _ = m1.select(roots, active, 1.5)
    m2.select_range(0, cut, roots, active, 1.5)
    _, obs2, _ = m2.select_range(cut, T - cut, roots, active, 1.5)
    assert torch.equal(m1.status, m2.status) and torch.equal(obs1, obs2)
    for i in range(sims):
        pf1, v1 = (t.contiguous() for t in model(obs1))
        pf2, v2 = (t.contiguous() for t in model(obs2))
        assert torch.equal(pf1, pf2) and torch.equal(v1, v2)
        last = i == sims - 1
        r = None if last else roots
        m1.leaf_step(pf1, w, b, v1, r, active, 1.5)
        # (the first simulation expands the roots: root_stats needs them in the tree)
        before = m2.root_stats(roots, active) if i > 0 else None
        m2.leaf_step_range(0, cut, pf2, w, b, v2, r, active, 1.5)
        if i > 0:  # only the trees [0, cut) moved
            for x, y in zip(before, m2.root_stats(roots, active)):
                assert torch.equal(x[cut:], y[cut:])
        m2.leaf_step_range(cut, T - cut, pf2, w, b, v2, r, active, 1.5)
        if not last:
            assert torch.equal(m1.status, m2.status) and torch.equal(m1.obs, m2.obs)
            ok = m1.status == 1
            assert torch.equal(m1.leaf_mask[ok], m2.leaf_mask[ok])
            obs1, obs2 = m1.obs, m2.obs
    c1, c2 = m1.check(), m2.check()
    assert c1 == c2 and c1["expanded"] > 0
    for x, y in zip(m1.root_stats(roots, active), m2.root_stats(roots, active)):
        assert torch.equal(x, y)


def test_empty_and_bad_ranges():
    from blokus_rl_amd.engine import _ptr

    T = 7
    eng, model, roots, active, m, _, w, b = _setup(14, T, 2)
    lib = m.lib
    _, obs, _ = m.select(roots, active, 1.5)
    pf, v = (t.contiguous() for t in model(obs))
    m.leaf_step(pf, w, b, v, roots, active, 1.5)  # the roots are in the trees from here on
    pf, v = (t.contiguous() for t in model(m.obs))
    st0, obs0 = m.status.clone(), m.obs.clone()
    before = m.root_stats(roots, active)

    def sel(t0, n):
        return lib.bk_mcts_select_range(m.h, t0, n, _ptr(roots), _ptr(active), 1.5, _ptr(m.status), _ptr(m.obs),
                                        _ptr(m.leaf_mask), m._s())

    def step(t0, n):
        return lib.bk_mcts_leaf_step_range(m.h, t0, n, ctypes.c_void_p(pf.data_ptr()), pf.stride(0), pf.shape[1],
                                           _ptr(w), _ptr(b), _ptr(v), 1, _ptr(roots), _ptr(active), 1.5,
                                           _ptr(m.status), _ptr(m.obs), _ptr(m.leaf_mask), m._s())

    # n = 0: OK, and nothing ran (an empty range at either end or in the middle)
    for t0 in (0, 3, T):
        assert sel(t0, 0) == 0 and step(t0, 0) == 0
    assert torch.equal(m.status, st0) and torch.equal(m.obs, obs0)
    for x, y in zip(before, m.root_stats(roots, active)):
        assert torch.equal(x, y)
    # outside [0, T): an error that names the entry, and still nothing ran
    for t0, n in ((-1, 2), (0, -1), (0, T + 1), (T, 1), (3, T - 2), (2**31 - 1, 2**31 - 1)):
        assert sel(t0, n) == -1 and b"bk_mcts_select_range" in lib.bk_last_error()
        assert step(t0, n) == -1 and b"bk_mcts_leaf_step_range" in lib.bk_last_error()
    for x, y in zip(before, m.root_stats(roots, active)):
        assert torch.equal(x, y)
    assert m.check()["errors"] == 0
