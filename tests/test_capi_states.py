"""The C ABI of the packed-state leaf path: bk_mcts_leaf_step without an observation buffer,
bk_mcts_leaf_states, and bk_leafnet_x3_states' argument checks."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_leaf_step_without_obs_leaves_the_same_leaves():
    """leaf_step(obs=None) writes the same leaf states and statuses as a run with a buffer (only
    the observation rows are skipped), and leaf_states_ptr is the buffer leaf_info copies."""
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import LeafResNet, ResNet, leafnet_x3_states

    T = 4
    eng = Engine(20, 4, 5)
    torch.manual_seed(1)
    model = LeafResNet(ResNet(20, 4, eng.A, 1).cuda().eval(), normalize=False, features=True).eval()
    po = model.f.policy_out
    w, b = po.weight.detach().contiguous(), po.bias.detach().contiguous()
    roots = random_boards(eng, T, seed0=5, max_plies=16)
    active = torch.ones(T, dtype=torch.int32, device=eng.device)
    active[2] = 0
    kw = dict(node_cap=16, child_cap=T * 16 * 700)
    m1, m2 = BatchedMCTS(eng, T, **kw), BatchedMCTS(eng, T, **kw)
    p2 = m2.leaf_states_ptr
    assert p2 != 0 and p2 % 4 == 0 and p2 != m1.leaf_states_ptr
    _, obs1, _ = m1.select(roots, active, 1.5)
    _, obs2, _ = m2.select(roots, active, 1.5)
    for i in range(5):
        pf1, v1 = model(obs1)
        # the second search's net reads its leaf states in place
        pf2, v2 = leafnet_x3_states(m2.leaf_states_ptr, m2.status, model)
        assert torch.equal(pf1, pf2) and torch.equal(v1, v2)
        st1, obs1, _ = m1.leaf_step(pf1, w, b, v1, roots, active, 1.5)
        st2, none, _ = m2.leaf_step(pf2, w, b, v2, roots, active, 1.5, obs=None)
        assert none is None and torch.equal(st1, st2)
        (s1, d1), (s2, d2) = m1.leaf_info(), m2.leaf_info()
        live = st1 == 1
        assert bool(live.any()) and int(st1[2]) == 0
        assert torch.equal(s1[live], s2[live]) and torch.equal(d1, d2)
    assert torch.equal(obs2, m2.obs) and m2.leaf_states_ptr == p2  # untouched since the select; the pointer stays
    assert m1.check() == m2.check()
    for x, y in zip(m1.root_stats(roots, active), m2.root_stats(roots, active)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("P,N,word", [(2, 20, b"P must be 4"), (4, 7, b"N must be 14 or 20"), (4, 21, b"N must be")])
def test_leafnet_x3_states_argument_checks(P, N, word):
    from blokus_rl_amd import engine

    lib = engine.load_library()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    rc = lib.bk_leafnet_x3_states(p, None, 1, N, P, p, p, p, 2, p, p, p, p, p, p, p, p, p, p, p, p, p, p, None, None)
    assert rc == -1 and word in lib.bk_last_error(), lib.bk_last_error()
    # a misaligned states pointer is refused too
    rc = lib.bk_leafnet_x3_states(ctypes.c_void_p(buf.data_ptr() + 2), None, 1, 20, 4, p, p, p, 2, p, p, p, p, p, p, p,
                                  p, p, p, p, p, p, p, None, None)
    assert rc == -1 and b"4-byte aligned" in lib.bk_last_error()
