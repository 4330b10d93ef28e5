"""GPU batched MCTS against the CPU MCTSOracle on the board presets the golden vectors do not cover:
14x14 with 4 and 2 players, 2-player 20x20, the 9-piece 20x20 and 5x5.

The procedure is test_mcts_gpu.test_batched_mcts_matches_reference's (stagewise select /
expand_backup, prior_mode 1, the stand-in net prior_value), but the expectations are computed live
by oracle.MCTSOracle, which test_mcts_oracle.py pins to the reference's mcts.py and which knows no
preset. Every simulation: the oracle's outcome (the leaf's board hash, or a terminal board), the
leaf's legal bitmask and the observation planes select() writes (N = 14 and N = 5 take its scalar
row writer). After each of two moves on the reused tree: root ids, N, Q (float64), P,
root_policy at T = 1 and T = 0, the visited children of every oracle node reached from the root,
and the chosen action's next state. All comparisons are equality.

Roots named ("bigk", K) are the big-K fixture's states (tests/golden/make_bigk_states.py) with
K = 769, 2049 and 5056 legal moves on 2-player 20x20 and 2374 on 2-player 14x14: above
kSelB * 64 = 768 children select_child takes its two-pass branch (the visit sum, then the scan),
and above kExpandLdsIds = 2048 the expansion compacts the ids straight into the child pool. Their
stand-in net (prior_value_tail) puts the largest prior on the last child, so the first descent
from such a root must pick child K - 1 — a scan that stopped short of the tail picks another —
and the cases assert that a root child of index >= 768 is visited and that a node below the root
with more than 768 children is expanded and descended through."""
from collections import defaultdict
from functools import lru_cache

import numpy as np
import pytest
import torch

import bigk_util
from mcts_golden_util import prior_value
from oracle.oracle import MCTSOracle, Oracle

pytestmark = pytest.mark.gpu

MOVES = 2
BIG = 768  # kSelB * 64
# (preset, root: None = the initial state, ("bigk", K) = the fixture state of that K, else
#  random_board(seed, max_plies), sims, cpuct, the oracle reaches terminal leaves)
CASES = [
    ((14, 4, 5), None, 60, 1, False),
    ((14, 4, 5), (5, 30), 80, 2, False),
    ((14, 2, 5), (3, 24), 80, 1, True),
    ((20, 2, 5), (9, 36), 80, 1, False),
    ((20, 4, 4), (2, 30), 120, 1, False),
    ((5, 2, 5), None, 100, 1, True),
    ((20, 2, 5), ("bigk", 769), 60, 1, False),
    ((20, 2, 5), ("bigk", 2049), 50, 1, False),
    ((20, 2, 5), ("bigk", 5056), 40, 1, False),
    ((14, 2, 5), ("bigk", 2374), 50, 1, False),
]


def _is_bigk(k: int) -> bool:
    return CASES[k][1] is not None and CASES[k][1][0] == "bigk"


def prior_value_tail(h: int, K: int, P: int):
    """prior_value with the largest logit moved to the last child."""
    rng = np.random.default_rng(h & 0x7FFFFFFFFFFFFFFF)
    x = rng.standard_normal(K).astype(np.float32)
    x[K - 1] = x.max() + np.float32(2.0)
    e = np.exp(x - x.max()).astype(np.float32)
    p = (e / e.sum()).astype(np.float32)
    v = rng.uniform(-1.0, 1.0, P).astype(np.float32)
    return p, v


def _prior(k: int):
    return prior_value_tail if _is_bigk(k) else prior_value


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
        p, v = _prior(k)(o.hash(s), len(ids), o.P)
        return ids, p, v.astype(np.float64)

    m = MCTSOracle(o, evaluate)
    if root is None:
        s = o.init_state()
    elif root[0] == "bigk":
        s = bigk_util.state_named(preset, root[1])
    else:
        s = o.random_board(*root)
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
    # the child pool per tree: the presets' usual size, or for fixture roots every expanded node (one
    # a simulation) at twice the largest root's K; the rows read back hold the largest node
    big_k = max([CASES[k][1][1] for k in case_ids if _is_bigk(k)], default=0)
    per_tree = max(4096 * (700 if preset[0] >= 14 else 200), (MOVES * max(sims) + 1) * 2 * big_k)
    cap = 8192 if big_k else 2048
    m = BatchedMCTS(eng, T, node_cap=4096, child_cap=T * per_tree)
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
                    p, v = _prior(case_ids[t])(want, len(ids), eng.P)
                    logp[t, torch.from_numpy(ids).to(dev)] = torch.from_numpy(p).to(dev)
                    vals[t] = torch.from_numpy(v).to(dev)
            m.expand_backup(logp, vals, prior_mode=1)
        m.check()
        ids, n, q, p, counts = (x.cpu().numpy() for x in m.root_stats(roots, None, cap=cap))
        pid, pi1, pc = (x.cpu().numpy() for x in m.root_policy(roots, None, 1.0, cap=cap))
        _, pi0, _ = (x.cpu().numpy() for x in m.root_policy(roots, None, 0.0, cap=cap))
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
            if _is_bigk(case_ids[t]) and r == 0:
                # both passes of select_child's two-pass branch decided something: the scan reached the
                # root's tail, and a node above 768 children below the root was expanded and scanned
                assert K == CASES[case_ids[t]][1][1] and n[t, K - 1] > 0 and n[t, BIG:K].sum() > 0
                below = [(Kn, len(visited)) for _, Kn, visited in mv["nodes"][1:] if Kn > BIG]
                print(f"case {case_ids[t]}: K {K}, visited root children >= {BIG}: {int((n[t, BIG:K] > 0).sum())}, "
                      f"nodes below the root above {BIG} children: {len(below)}, descended through: "
                      f"{sum(1 for _, nv in below if nv)}")
                assert below and any(nv for _, nv in below)
            only = torch.zeros(T, dtype=torch.int32, device=dev)
            only[t] = 1
            for state, Kn, visited in mv["nodes"]:
                node_roots = roots.clone()
                node_roots[t] = torch.from_numpy(state).to(dev)
                _, nn_, qq, _, cc = m.root_stats(node_roots, only, cap=cap)
                assert int(cc[t]) == Kn
                nh, qh = nn_[t, :Kn].cpu().numpy(), qq[t, :Kn].cpu().numpy()
                assert [[i, int(nh[i]), float(qh[i])] for i in range(Kn) if nh[i] > 0] == visited
            nxt, nxt_player, status = eng.next_state(roots[t:t + 1].contiguous(),
                                                     torch.tensor([mv["action"]], dtype=torch.int32, device=dev))
            assert int(status[0]) == 0
            assert (nxt[0].cpu().numpy() == mv["next"]).all()
            assert int(nxt_player[0]) == Oracle.to_move(mv["next"])
