"""The arena's rows entries (bk_mcts_select_rows, bk_leafnet_x3_rows, bk_mcts_leaf_step_rows,
bk_arena_sims, bk_arena_move) against the existing per-stage entries driven once per net on the
same positions: after every ply of three, with the moves played between them, every tree's
root_stats (ids, N, Q, P) and the counters are equal bitwise, and so are the moves."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (board, players, games, seat -> net index (-1 uninformed), sims per seat)
CASES = {
    "7x7": (7, 2, 5, (0, 1), (5, 3)),
    "20x20": (20, 4, 3, (0, 1, -1, 0), (3, 4, 2, 3)),
}


def run_case(name, mode, plies=3):
    from arena_rows_ref import PerStage, Rows, compare_trees, leaf_net, orders_of, tables_of
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine

    n, p, G, seat_net_l, sims_l = CASES[name]
    eng = Engine(n, p, 5)
    dev = eng.device
    leaves = [leaf_net(eng, 10 + k)[1] for k in range(max(seat_net_l) + 1)]
    seat_net = torch.tensor(seat_net_l, device=dev)
    seat_sims = torch.tensor(sims_l, device=dev)
    max_sims = max(sims_l)
    orders = orders_of(G, p, True, dev)
    T = G * p
    kw = dict(node_cap=max_sims * plies + 8, child_cap=T * (max_sims * plies + 8) * (700 if n == 20 else 96))
    m_ref, m_row = BatchedMCTS(eng, T, **kw), BatchedMCTS(eng, T, **kw)
    ref = PerStage(eng, m_ref, leaves, 1.25)
    row = Rows(eng, m_row, leaves, G, max_sims, 1.25, mode)
    states = random_boards(eng, G, seed0=3, max_plies=2 * p)  # different positions and movers
    over = eng.game_ended(states)[0].bool()
    roots_t = eng.init_states(T)
    seen = torch.zeros(T, dtype=torch.int32, device=dev)
    for _ in range(plies):
        tree, net_row, sims_row = tables_of(eng, states, orders, seat_net, seat_sims, over)
        ref.ply(states, tree, net_row, sims_row, max_sims)
        row.ply(states, tree, net_row, sims_row)
        used = tree[tree >= 0].long()
        roots_t[used] = states[tree >= 0]
        seen[used] = 1
        c = compare_trees(m_ref, m_row, roots_t, seen)
        assert c["errors"] == 0 and c["expanded"] > 0
        a_ref, a_row = ref.move(states, tree), row.move()
        assert torch.equal(a_ref, a_row), (a_ref, a_row)
        assert bool((a_row[tree >= 0] >= 0).all())
        states, _, status = eng.next_state(states, a_row)
        assert int(status.max()) == 0
        over |= eng.game_ended(states)[0].bool()
    c = compare_trees(m_ref, m_row, roots_t, seen)
    # every seat of every game searched its budget once per own ply: the nets' and the
    # uninformed seat's trees all grew
    assert c["expanded"] >= G * min(sims_l)
    return c


@pytest.mark.parametrize("name", ["7x7", "20x20"])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_rows_equal_per_stage(name, mode):
    run_case(name, mode)


def test_rows_equal_per_stage_without_overlap():
    """BK_STEP_OVERLAP=0 (k_leaf_step_rows instead of k_leaf_step_ov_rows), in a fresh process."""
    env = dict(os.environ, BK_STEP_OVERLAP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "20x20", "eager"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "rows ok" in r.stdout


def test_arena_move_dead_row_and_game_without_moves():
    """arena_move == root_policy(T = 0) + argmax: a searched root, a dead row (-1) and a finished
    game whose root was never expanded (-1; both entries flag the missing root)."""
    from arena_rows_ref import PerStage, Rows
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.engine import Engine

    eng = Engine(7, 2, 5)
    dev = eng.device
    G, sims = 3, 6
    T = G * eng.P
    kw = dict(node_cap=32, child_cap=T * 32 * 96)
    m_ref, m_row = BatchedMCTS(eng, T, **kw), BatchedMCTS(eng, T, **kw)
    ref, row = PerStage(eng, m_ref, [], 1.0), Rows(eng, m_row, [], G, sims, 1.0, "sims")
    states = random_boards(eng, G, seed0=21, max_plies=4)
    done = random_boards(eng, 1, seed0=2, max_plies=200)
    assert bool(eng.game_ended(done)[0].all())
    states[2] = done[0]
    i32 = dict(dtype=torch.int32, device=dev)
    tree = torch.tensor([0 * eng.P + 1, -1, 2 * eng.P + 0], **i32)
    net_row = torch.full((G,), -1, **i32)
    sims_row = torch.full((G,), sims, **i32)
    ref.ply(states, tree, net_row, sims_row, sims)
    row.ply(states, tree, net_row, sims_row)
    a_ref, a_row = ref.move(states, tree), row.move()
    assert torch.equal(a_ref, a_row)
    assert int(a_row[0]) >= 0 and a_row[1:].tolist() == [-1, -1]
    c_ref, c_row = m_ref.counters(), m_row.counters()
    assert c_ref == c_row and c_row["errors"] == 16 and c_row["terminal"] == sims


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    run_case(sys.argv[1], sys.argv[2])
    print("rows ok", os.environ.get("BK_STEP_OVERLAP"))
