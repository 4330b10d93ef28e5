"""Self-play with the captured simulations split into staggered tree groups
(SelfPlay(sim_groups=2 | 4), bk_mcts_sims_pipelined) against the one-group schedule: the roots,
root statistics, counters and recorded rows after three plies (three replays of one captured graph)
come out bitwise identical — in both leaf-input modes, with an empty group, uneven groups, a
group whose games are all inactive, the eager multi-stream path and every ring-edge mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

_REF: dict = {}


@pytest.fixture(scope="module")
def eng():
    from blokus_rl_amd.engine import Engine

    return Engine(20, 4, 5)


def _run(eng, games, groups, leaf_input, ring=None, idle=None):
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.nets import ResNet

    torch.manual_seed(0)
    model = ResNet(20, 4, eng.A, num_res_blocks=2).to(eng.device).eval()
    sp = SelfPlay(eng, model, games, num_sims=13, node_cap=256, seed=5, continuous=True, leaf_input=leaf_input,
                  sim_groups=groups, sim_ring=ring, sim_groups_min_games=1)
    assert sp.sim_groups == groups and sp.leaf_input == leaf_input
    if idle is not None:
        sp.active[idle[0]:idle[1]] = 0
    for _ in range(3):
        sp.play_ply()
    _, n, q, p, k = sp.mcts.root_stats(sp.roots, sp.active)  # (an inactive game's root is in no tree)
    out = [sp.roots.clone(), n, q, p, k]
    for roots, ids, pi, counts, player, gid, act in sp._records:
        # the id / pi rows are written up to each game's count only
        valid = torch.arange(ids.shape[1], device=ids.device).unsqueeze(0) < counts.clamp(min=0).unsqueeze(1)
        out += [roots, torch.where(valid, ids, torch.zeros_like(ids)), torch.where(valid, pi, torch.zeros_like(pi)),
                counts, player, gid, act]
    assert len(sp._records) == 3
    return out, sp.mcts.check()


def _ref(eng, games, leaf_input, idle=None):
    """The one-group run, computed once per configuration and shared."""
    key = (games, leaf_input, idle)
    if key not in _REF:
        _REF[key] = _run(eng, games, 1, leaf_input, idle=idle)
    return _REF[key]


def _check(eng, games, groups, leaf_input, ring=None, idle=None):
    ref, cref = _ref(eng, games, leaf_input, idle)
    got, cgot = _run(eng, games, groups, leaf_input, ring=ring, idle=idle)
    assert cgot == cref and cref["expanded"] > 0
    assert len(ref) == len(got)
    for x, y in zip(ref, got):
        assert torch.equal(x, y)


# 6 games in 4 groups: sizes 2, 2, 2, 0 (an empty group); 7 in 4: 2, 2, 2, 1
@pytest.mark.parametrize("leaf_input", ["planes", "states"])
@pytest.mark.parametrize("games,groups", [(6, 2), (6, 4), (7, 4)])
def test_groups_match_one_group(eng, monkeypatch, games, groups, leaf_input):
    monkeypatch.setenv("BK_SIM_GRAPH", "1")
    _check(eng, games, groups, leaf_input)


def test_group_of_inactive_games(eng, monkeypatch):
    """Every game of group 1 ([3, 6)) inactive: `active` is zero over a whole range."""
    monkeypatch.setenv("BK_SIM_GRAPH", "1")
    _check(eng, 6, 2, "planes", idle=(3, 6))


def test_eager_streams_match(eng, monkeypatch):
    """No captured graph: the group chains are enqueued eagerly on the group streams."""
    monkeypatch.setenv("BK_SIM_GRAPH", "1")
    _ref(eng, 6, "planes")  # the shared reference is the captured one-group run
    monkeypatch.setenv("BK_SIM_GRAPH", "0")
    _check(eng, 6, 2, "planes")


# the ring edges off (0), on every simulation (1: the default of two groups) and on a graph's
# first simulation only (2: the default of four groups), each where it is not the default
@pytest.mark.parametrize("games,groups,leaf_input,ring", [(7, 4, "states", 0), (6, 2, "planes", 0),
                                                          (7, 4, "planes", 1), (6, 2, "states", 2)])
def test_ring_edge_modes(eng, monkeypatch, games, groups, leaf_input, ring):
    monkeypatch.setenv("BK_SIM_GRAPH", "1")
    _check(eng, games, groups, leaf_input, ring=ring)


def test_falls_back_to_one_group(eng):
    """Below the games threshold (64 by default), or with more groups than games: one group."""
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.nets import ResNet

    torch.manual_seed(0)
    model = ResNet(20, 4, eng.A, num_res_blocks=1).to(eng.device).eval()
    assert SelfPlay(eng, model, 6, num_sims=2, node_cap=16, sim_groups=2).sim_groups == 1
    assert SelfPlay(eng, model, 3, num_sims=2, node_cap=16, sim_groups=4, sim_groups_min_games=1).sim_groups == 1
    with pytest.raises(ValueError):
        SelfPlay(eng, model, 6, num_sims=2, node_cap=16, sim_groups=3)
