"""GPU batched MCTS against the CPU MCTSOracle on the board presets the golden vectors do not cover:
14x14 with 4 and 2 players, 2-player 20x20, the 9-piece 20x20 and 5x5.

The procedure is test_mcts_gpu.test_batched_mcts_matches_reference's (stagewise select /
expand_backup, prior_mode 1, the stand-in net prior_value), but the expectations are computed live
by oracle.MCTSOracle, which test_mcts_oracle.py pins to the reference's mcts.py and which knows no
preset. Every simulation: the oracle's outcome (the leaf's board hash, or a terminal board), the
leaf's legal bitmask and the observation planes select() writes (N = 14 and N = 5 take its scalar
row writer). After each of two moves on the reused tree: root ids, N, Q (float64), P,
root_policy at T = 1 and T = 0, the visited children of every oracle node reached from the root,
and the chosen action's next state. All comparisons are equality."""
from collections import defaultdict
from functools import lru_cache

import numpy as np
import pytest
import torch

from mcts_golden_util import prior_value
from oracle.oracle import MCTSOracle, Oracle

pytestmark = pytest.mark.gpu

MOVES = 2
# (preset, root: None = the initial state, else random_board(seed, max_plies), sims, cpuct,
#  the oracle reaches terminal leaves)
CASES = [
    ((14, 4, 5), None, 60, 1, False),
    ((14, 4, 5), (5, 30), 80, 2, False),
    ((14, 2, 5), (3, 24), 80, 1, True),
    ((20, 2, 5), (9, 36), 80, 1, False),
    ((20, 4, 4), (2, 30), 120, 1, False),
    ((5, 2, 5), None, 100, 1, True),
]


def _groups():
    g = defaultdict(list)
    for k, (preset, _, _, cpuct, _) in enumerate(CASES):
        g[(preset, cpuct)].append(k)
    return sorted(g.items())


def _bits_to_ids(words: np.ndarray, A: int) -> np.ndarray:
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:A]
    return np.nonzero(bits)[0]


@lru_cache(maxsize=None)
def _expected(k: int):
    """The oracle's search of case k: per move the root, the outcome of every simulation (the leaf's
    hash, None for a terminal board), the root's statistics and distributions, every node reached
    from the root through visited children, the T = 0 action and the state it leads to."""
    preset, root, sims, cpuct, _ = CASES[k]
    o = Oracle(*preset)
    leaves = []

    def evaluate(s, player):
        leaves.append(o.hash(s))
        ids = o.legal_ids(s, player)
        p, v = prior_value(o.hash(s), len(ids), o.P)
        return ids, p, v.astype(np.float64)

    m = MCTSOracle(o, evaluate)
    s = o.init_state() if root is None else o.random_board(*root)
    moves = []
    for _ in range(MOVES):
        assert o.game_ended(s) is None
        outcomes = []
        for _ in range(sims):
            n_leaves = len(leaves)
            m.simulate(s, cpuct=cpuct)
            outcomes.append(leaves[-1] if len(leaves) > n_leaves else None)
        ids, d1 = m.get_distribution(s, 1)
        _, d0 = m.get_distribution(s, 0)
        node = m.tree[o.hash(s)]
        nodes, seen, frontier = [], set(), [s]
        while frontier:
            nxt = []
            for st in frontier:
                h = o.hash(st)
                if h in seen or h not in m.tree:
                    continue
                seen.add(h)
                nd = m.tree[h]
                nodes.append((st, len(nd["N"]), [[i, n, nd["Q"][i]] for i, n in enumerate(nd["N"]) if n > 0]))
                nxt += [o.next_state(st, a)[0] for a, n in zip(nd["ids"], nd["N"]) if n > 0]
            frontier = nxt
        action = int(ids[int(np.argmax(d0))])
        nxt_root = o.next_state(s, action)[0]
        moves.append({"root": s, "outcomes": outcomes, "ids": ids.tolist(), "N": list(node["N"]),
                      "Q": list(node["Q"]), "P": list(node["P"]), "d1": d1.tolist(), "d0": d0.tolist(),
                      "nodes": nodes, "action": action, "next": nxt_root})
        s = nxt_root
    return moves, m.terminal_hits


@pytest.mark.parametrize("group", _groups(), ids=lambda g: f"{'x'.join(map(str, g[0][0]))}-cpuct{g[0][1]}")
def test_batched_mcts_matches_oracle(group):
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS
    from blokus_rl_amd.engine import Engine

    (preset, cpuct), case_ids = group
    eng, o = Engine(*preset), Oracle(*preset)
    dev = eng.device
    T = len(case_ids)
    expected = [_expected(k) for k in case_ids]
    for k, (_, hits) in zip(case_ids, expected):
        print(f"case {k} {CASES[k][:4]}: oracle terminal hits {hits}")
        if CASES[k][4]:
            assert hits > 0  # the terminal-score backup is exercised
    cases = [mv for mv, _ in expected]
    sims = [CASES[k][2] for k in case_ids]
    m = BatchedMCTS(eng, T, node_cap=4096, child_cap=T * 4096 * (700 if preset[0] >= 14 else 200))
    logp = torch.zeros((T, eng.A), dtype=torch.float32, device=dev)
    vals = torch.zeros((T, eng.P), dtype=torch.float32, device=dev)
    for r in range(MOVES):
        roots = torch.from_numpy(np.stack([c[r]["root"] for c in cases])).to(dev)
        for sim in range(max(sims)):
            act_h = [1 if sim < s else 0 for s in sims]
            status, obs, mask = m.select(roots, torch.tensor(act_h, dtype=torch.int32, device=dev), float(cpuct))
            st_h, obs_h = status.cpu().numpy(), obs.cpu().numpy()
            leaves, _ = m.leaf_info()
            leaves_h = leaves.cpu().numpy()
            mask_h = mask.cpu().numpy().view(np.uint64)
            logp.zero_()
            vals.zero_()
            for t in range(T):
                if not act_h[t]:
                    continue
                want = cases[t][r]["outcomes"][sim]
                assert st_h[t] == (2 if want is None else 1), (r, sim, t)
                if st_h[t] == 1:
                    assert o.hash(leaves_h[t]) == want, (r, sim, t)
                    ids = _bits_to_ids(mask_h[t], eng.A)
                    assert (ids == o.legal_ids(leaves_h[t])).all()
                    assert (obs_h[t] == o.observe(leaves_h[t])).all(), (r, sim, t)
                    p, v = prior_value(want, len(ids), eng.P)
                    logp[t, torch.from_numpy(ids).to(dev)] = torch.from_numpy(p).to(dev)
                    vals[t] = torch.from_numpy(v).to(dev)
            m.expand_backup(logp, vals, prior_mode=1)
        m.check()
        ids, n, q, p, counts = (x.cpu().numpy() for x in m.root_stats(roots, None, cap=2048))
        pid, pi1, pc = (x.cpu().numpy() for x in m.root_policy(roots, None, 1.0))
        _, pi0, _ = (x.cpu().numpy() for x in m.root_policy(roots, None, 0.0))
        for t, c in enumerate(cases):
            mv = c[r]
            K = int(counts[t])
            assert K == len(mv["ids"]) == int(pc[t])
            assert ids[t, :K].tolist() == mv["ids"] and pid[t, :K].tolist() == mv["ids"]
            assert n[t, :K].tolist() == mv["N"]
            assert q[t, :K].tolist() == mv["Q"]
            assert p[t, :K].astype(np.float64).tolist() == mv["P"]
            assert pi1[t, :K].tolist() == mv["d1"]
            assert pi0[t, :K].tolist() == mv["d0"]
            only = torch.zeros(T, dtype=torch.int32, device=dev)
            only[t] = 1
            for state, Kn, visited in mv["nodes"]:
                node_roots = roots.clone()
                node_roots[t] = torch.from_numpy(state).to(dev)
                _, nn_, qq, _, cc = m.root_stats(node_roots, only, cap=2048)
                assert int(cc[t]) == Kn
                nh, qh = nn_[t, :Kn].cpu().numpy(), qq[t, :Kn].cpu().numpy()
                assert [[i, int(nh[i]), float(qh[i])] for i in range(Kn) if nh[i] > 0] == visited
            nxt, nxt_player, status = eng.next_state(roots[t:t + 1].contiguous(),
                                                     torch.tensor([mv["action"]], dtype=torch.int32, device=dev))
            assert int(status[0]) == 0
            assert (nxt[0].cpu().numpy() == mv["next"]).all()
            assert int(nxt_player[0]) == Oracle.to_move(mv["next"])
