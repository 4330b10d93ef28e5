"""BatchedArena(path="graph"): a ply's simulations as one captured linear graph over the rows
entries and a device-side tail. Uninformed seats: the default path's scores and final states,
exactly. Net seats: whole games against a test-local arena loop built from the per-stage entries
(tests/arena_rows_ref.py), move for move. bk_arena_finish against its NumPy restatement."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _engine(n, p):
    from blokus_rl_amd.engine import Engine

    return Engine(n, p, 5)


@pytest.mark.parametrize("n,p,games,sims", [(7, 2, 4, (12, 7)), (20, 4, 3, (3, 4, 2, 3))])
def test_uninformed_graph_equals_default_path(n, p, games, sims):
    from blokus_rl_amd.alphazero.batched_arena import ArenaSeat, BatchedArena

    eng = _engine(n, p)
    seats = [ArenaSeat(None, s) for s in sims]
    s0, g0, st0 = BatchedArena(eng, seats).play(games, permute=True)
    arena = BatchedArena(eng, seats, path="graph", record_actions=True)
    s1, g1, st1 = arena.play(games, permute=True)
    assert arena.path_used == "graph" and arena.path_reason == ""
    np.testing.assert_array_equal(g0, g1)
    np.testing.assert_array_equal(s0, s1)
    assert torch.equal(st0, st1)
    a = arena.last_actions
    assert a.dtype == np.int32 and a.shape[1] == games and (a[-1] >= 0).any() and (a[0] >= 0).all()
    assert bool(eng.game_ended(st1)[0].all())


def _reference_match(eng, leaves, seat_net_l, sims_l, G, cpuct):
    """The arena loop on the per-stage entries: -> (actions [plies, G], per-game scores, counters)."""
    from arena_rows_ref import PerStage, orders_of, tables_of
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS

    dev, P = eng.device, eng.P
    max_sims = max(sims_l)
    node_cap = max_sims * eng.num_pieces + 1
    T = G * P
    mcts = BatchedMCTS(eng, T, node_cap=node_cap, child_cap=T * node_cap * (256 if eng.N >= 14 else 64))
    ref = PerStage(eng, mcts, leaves, cpuct)
    seat_net, seat_sims = torch.tensor(seat_net_l, device=dev), torch.tensor(sims_l, device=dev)
    orders = orders_of(G, P, True, dev)
    states = eng.init_states(G)
    over = torch.zeros(G, dtype=torch.bool, device=dev)
    final = torch.zeros((G, P), dtype=torch.float64, device=dev)
    acts = []
    while not bool(over.all()):
        tree, net_row, sims_row = tables_of(eng, states, orders, seat_net, seat_sims, over)
        ref.ply(states, tree, net_row, sims_row, max_sims)
        action = ref.move(states, tree)
        acts.append(action.cpu().numpy())
        states, _, status = eng.next_state(states, action)
        assert int(status.max()) == 0
        ended, scores = eng.game_ended(states)
        final = torch.where((ended.bool() & ~over).view(-1, 1), scores, final)
        over |= ended.bool()
    return np.stack(acts), final.cpu().numpy(), mcts.check(), states


@pytest.mark.parametrize("n,p,G,seat_net_l,sims_l", [(7, 2, 4, (0, 1), (6, 4)), (20, 4, 3, (0, 1, -1, 0), (3, 4, 2, 3))])
def test_net_seats_whole_games_equal_per_stage_loop(n, p, G, seat_net_l, sims_l):
    from arena_rows_ref import leaf_net
    from blokus_rl_amd.alphazero.batched_arena import ArenaSeat, BatchedArena

    eng = _engine(n, p)
    pairs = [leaf_net(eng, 30 + k) for k in range(max(seat_net_l) + 1)]
    nets, leaves = [a for a, _ in pairs], [b for _, b in pairs]
    seats = [ArenaSeat(nets[k] if k >= 0 else None, s) for k, s in zip(seat_net_l, sims_l)]
    arena = BatchedArena(eng, seats, cpuct=1.0, path="graph", record_actions=True, x3_boards="all")
    total, per_game, states = arena.play(G, permute=True)
    assert arena.path_used == "graph", arena.path_reason
    acts, final, counters, ref_states = _reference_match(eng, leaves, seat_net_l, sims_l, G, 1.0)
    assert arena.last_actions.shape == acts.shape
    np.testing.assert_array_equal(arena.last_actions, acts)
    np.testing.assert_array_equal(per_game, final)
    assert torch.equal(states, ref_states)
    assert arena.counters == counters
    assert counters["terminal"] >= 1 and counters["errors"] == 0
    assert total.sum() == per_game.sum()


def test_non_resnet_seat_falls_back_to_eager():
    from blokus_rl_amd.alphazero.batched_arena import ArenaSeat, BatchedArena
    from blokus_rl_amd.nets import DCNNet

    eng = _engine(7, 2)
    torch.manual_seed(5)
    net = DCNNet(7, 2, eng.A).to(eng.device).eval()
    seats = [ArenaSeat(net, 4), ArenaSeat(None, 3)]
    s0, g0, st0 = BatchedArena(eng, seats).play(2, permute=True)
    arena = BatchedArena(eng, seats, path="graph")
    s1, g1, st1 = arena.play(2, permute=True)
    assert arena.path_used == "eager" and "DCNNet" in arena.path_reason
    np.testing.assert_array_equal(g0, g1)
    np.testing.assert_array_equal(s0, s1)
    assert torch.equal(st0, st1)


def test_arena_compare_reads_bk_arena(monkeypatch, tmp_path):
    from blokus_rl_amd.alphazero import batched_arena
    from blokus_rl_amd.alphazero.trainer import AlphaZeroTrainer
    from blokus_rl_amd.hparams import AlphaZeroHparams

    monkeypatch.setenv("BK_ARENA", "graph")
    monkeypatch.setenv("BK_X3_BOARDS", "all")
    monkeypatch.chdir(tmp_path)
    seen = []
    play = batched_arena.BatchedArena.play

    def spy(self, *a, **kw):
        out = play(self, *a, **kw)
        seen.append((self.path_used, self.path_reason, out))
        return out

    monkeypatch.setattr(batched_arena.BatchedArena, "play", spy)
    hp = AlphaZeroHparams(board_size=7, number_of_players=2, num_res_blocks=1, num_mcts_sims=4,
                          compare_arena_games=4, permute=True)
    torch.manual_seed(0)
    trainer = AlphaZeroTrainer(hp)
    scores = trainer.arena_compare(None, 4)
    (path, reason, (total, per_game, _)), = seen
    assert path == "graph", reason
    np.testing.assert_array_equal(scores, total)
    assert scores.sum() == per_game.sum() and per_game.shape == (4, 2)


@pytest.mark.parametrize("R", [1, 37, 300])
def test_arena_finish_equals_numpy(R):
    from blokus_rl_amd.alphazero.batched_arena import arena_finish_np
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine as E

    P = 4
    eng = _engine(20, P)
    dev = eng.device
    rng = np.random.default_rng(R)
    base = random_boards(eng, min(R, 16), seed0=9, max_plies=12)
    states = base[torch.from_numpy(rng.integers(0, base.shape[0], R)).to(dev)].contiguous()
    to_move = E.to_move(states).cpu().numpy()
    assert R == 1 or len(set(to_move.tolist())) > 1
    orders = np.stack([rng.permutation(P) for _ in range(R)]).astype(np.int32)
    seat_net = np.array([1, -1, 0, 2], dtype=np.int32)
    seat_sims = np.array([50, 3, 7, 1], dtype=np.int32)
    over = rng.random(R) < 0.25
    final = np.where(over[:, None], rng.choice([-1.0, 1.0, 3.0], (R, P)), 0.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tabs = [torch.full((R,), 77, dtype=torch.int32, device=dev) for _ in range(3)]
    over_d, final_d = t(over.astype(np.uint8)), t(final)
    illegal_d, running_d = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1,), -5, dtype=torch.int32, device=dev)
    illegal = 0
    for step in range(3):  # the in-place tables, over and final carried from call to call
        ended = (rng.random(R) < (0.3, 0.0, 1.0)[step]).astype(np.int32)
        scores = np.where(ended[:, None] != 0, rng.choice([-1.0, 1.0, 3.0], (R, P)), 0.0)
        status = np.zeros(R, dtype=np.int32)
        status[rng.integers(0, R)] = 1 if step == 1 else 0  # counts only on a live row
        want = arena_finish_np(to_move, ended, scores, status, orders, seat_net, seat_sims, over, final, illegal)
        eng.arena_finish(states, t(ended), t(scores), t(status), t(orders), t(seat_net), t(seat_sims), *tabs, over_d,
                         final_d, illegal_d, running_d)
        got = [x.cpu().numpy() for x in tabs] + [over_d.cpu().numpy(), final_d.cpu().numpy(), int(illegal_d), int(running_d)]
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        _, _, _, over, final, illegal, _ = want
        over = over.astype(bool)
    assert bool(over.all()) and int(running_d) == 0
