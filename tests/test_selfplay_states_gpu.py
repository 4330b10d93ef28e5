"""SelfPlay(leaf_input="states"): the leaf net reads the search's packed leaf states and status
(bk_leafnet_x3_states) and the simulation loop writes no observation. The net's outputs equal the
planar path's as float values, so the games must be the same: roots, actions, records, counters."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _same_records(a, b):
    assert len(a._records) == len(b._records) > 0
    for ra, rb in zip(a._records, b._records):
        for i in (0, 3, 4, 5, 6):  # roots, counts, player, game id, acted
            assert torch.equal(ra[i], rb[i]), i
        valid = torch.arange(ra[1].shape[1], device=ra[1].device).unsqueeze(0) < ra[3].clamp(min=0).unsqueeze(1)
        assert torch.equal(torch.where(valid, ra[1], 0), torch.where(valid, rb[1], 0))  # ids
        assert torch.equal(torch.where(valid, ra[2], 0), torch.where(valid, rb[2], 0))  # pi


@pytest.mark.parametrize("use_graph", [True, False])
def test_states_selfplay_plays_the_planes_games(use_graph):
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import ResNet

    eng = Engine(20, 4, 5)
    torch.manual_seed(0)
    net = ResNet(20, 4, eng.A, 2).to(eng.device).eval()
    runs = []
    for mode in ("planes", "states"):
        sp = SelfPlay(eng, net, 8, num_sims=16, seed=3, use_graph=use_graph, leaf_input=mode)
        assert sp.evaluator.sparse and sp.leaf_input == mode
        for _ in range(3):
            sp.play_ply()
        runs.append((sp, sp.check()))
    (a, ca), (b, cb) = runs
    assert ca == cb and ca["expanded"] > 0
    assert torch.equal(a.roots, b.roots) and torch.equal(a.last_action, b.last_action)
    assert bool((a.last_action >= 0).all())
    _same_records(a, b)
    for x, y in zip(a.mcts.root_stats(a.roots), b.mcts.root_stats(b.roots)):
        assert torch.equal(x, y)


def test_states_mode_reads_the_environment(monkeypatch):
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import ResNet

    eng = Engine(20, 4, 5)
    torch.manual_seed(0)
    net = ResNet(20, 4, eng.A, 1).to(eng.device).eval()
    assert SelfPlay(eng, net, 2, num_sims=2, use_graph=False).leaf_input == "planes"
    monkeypatch.setenv("BK_LEAF_INPUT", "states")
    assert SelfPlay(eng, net, 2, num_sims=2, use_graph=False).leaf_input == "states"
    assert SelfPlay(eng, net, 2, num_sims=2, use_graph=False, leaf_input="planes").leaf_input == "planes"
    monkeypatch.setenv("BK_NET_MATH", "f32")  # the f32 kernels take no states
    assert SelfPlay(eng, net, 2, num_sims=2, use_graph=False).leaf_input == "planes"
    monkeypatch.setenv("BK_LEAF_INPUT", "rows")
    with pytest.raises(ValueError):
        SelfPlay(eng, net, 2, num_sims=2, use_graph=False)


def test_states_mode_falls_back_without_a_states_evaluator():
    """DumbNet has no forward to feed: leaf_input="states" reports "planes" and plays the default's ply."""
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import DumbNet

    eng = Engine(7, 2, 5)
    net = DumbNet(7, 2, eng.A).to(eng.device).eval()
    a = SelfPlay(eng, net, 6, num_sims=8, seed=2, cap=256)
    b = SelfPlay(eng, net, 6, num_sims=8, seed=2, cap=256, leaf_input="states")
    assert a.leaf_input == "planes" and b.leaf_input == "planes"
    a.play_ply()
    b.play_ply()
    assert a.check() == b.check()
    assert torch.equal(a.roots, b.roots) and torch.equal(a.last_action, b.last_action)
    _same_records(a, b)
