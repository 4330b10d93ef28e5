"""Self-play on the 2-player 7x7 game with x3_boards="all": the leaf net is bk_leafnet_x3_np (one
launch, split-f16), so leaf_input="states" and the pipelined tree groups apply as they do at
20x20. The games must not depend on the input form, the group count or the boards per workgroup,
and the search must replay through the CPU oracle bit for bit."""
import numpy as np
import pytest
import torch

from oracle.oracle import MCTSOracle, Oracle

pytestmark = pytest.mark.gpu


def _setup(blocks=2, seed=0):
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import ResNet

    eng = Engine(7, 2, 5)
    torch.manual_seed(seed)
    return eng, ResNet(7, 2, eng.A, blocks).to(eng.device).eval()


def _same_records(a, b):
    assert len(a._records) == len(b._records) > 0
    for ra, rb in zip(a._records, b._records):
        for i in (0, 3, 4, 5, 6):  # roots, counts, player, game id, acted
            assert torch.equal(ra[i], rb[i]), i
        valid = torch.arange(ra[1].shape[1], device=ra[1].device).unsqueeze(0) < ra[3].clamp(min=0).unsqueeze(1)
        assert torch.equal(torch.where(valid, ra[1], 0), torch.where(valid, rb[1], 0))  # ids
        assert torch.equal(torch.where(valid, ra[2], 0), torch.where(valid, rb[2], 0))  # pi


def _same_games(a, ca, b, cb):
    assert ca == cb and ca["expanded"] > 0
    assert torch.equal(a.roots, b.roots) and torch.equal(a.last_action, b.last_action)
    _same_records(a, b)
    for x, y in zip(a.mcts.root_stats(a.roots), b.mcts.root_stats(b.roots)):
        assert torch.equal(x, y)


def test_knob_is_off_by_default(monkeypatch):
    from blokus_rl_amd.alphazero.selfplay import SelfPlay

    eng, net = _setup()
    kw = dict(num_sims=4, cap=256, use_graph=False, leaf_input="states")
    monkeypatch.delenv("BK_X3_BOARDS", raising=False)
    off = SelfPlay(eng, net, 70, **kw)
    assert not off.evaluator.takes_states and off.sim_groups == 1 and off.leaf_input == "planes"
    assert not off.evaluator.model.x3 and "x3_wstem" not in off.evaluator.model.state_dict()
    on = SelfPlay(eng, net, 70, x3_boards="all", **kw)
    assert on.evaluator.takes_states and on.sim_groups == SelfPlay.SIM_GROUPS_DEFAULT and on.leaf_input == "states"
    monkeypatch.setenv("BK_X3_BOARDS", "all")
    env = SelfPlay(eng, net, 70, **kw)
    assert env.evaluator.takes_states and env.sim_groups == SelfPlay.SIM_GROUPS_DEFAULT
    monkeypatch.setenv("BK_NET_MATH", "f32")  # still wins over the knob
    f32 = SelfPlay(eng, net, 70, **kw)
    assert not f32.evaluator.takes_states and f32.sim_groups == 1
    monkeypatch.setenv("BK_X3_BOARDS", "some")
    with pytest.raises(ValueError):
        SelfPlay(eng, net, 70, **kw)


@pytest.mark.parametrize("use_graph", [True, False])
def test_states_selfplay_plays_the_planes_games(use_graph):
    from blokus_rl_amd.alphazero.selfplay import SelfPlay

    eng, net = _setup()
    runs = []
    for mode in ("planes", "states"):
        sp = SelfPlay(eng, net, 8, num_sims=16, seed=3, cap=256, use_graph=use_graph, leaf_input=mode,
                      x3_boards="all")
        assert sp.evaluator.sparse and sp.leaf_input == mode
        for _ in range(3):
            sp.play_ply()
        runs.append((sp, sp.check()))
    (a, ca), (b, cb) = runs
    assert bool((a.last_action >= 0).all())
    _same_games(a, ca, b, cb)


def test_pipelined_groups_and_workgroup_forms_play_the_same_games(monkeypatch):
    """70 games: four ranges of 18 trees (at least the 64-game threshold, and no multiple of 4, so
    every range has a tail workgroup at four boards per workgroup)."""
    from blokus_rl_amd.alphazero.selfplay import SelfPlay

    eng, net = _setup()
    runs = []
    for groups, pack in ((1, "0"), (4, "1"), (4, "4")):
        monkeypatch.setenv("BK_X3_PACK", pack)
        sp = SelfPlay(eng, net, 70, num_sims=8, seed=5, cap=256, leaf_input="states", sim_groups=groups,
                      x3_boards="all")
        assert sp.leaf_input == "states" and sp.sim_groups == groups
        for _ in range(3):
            sp.play_ply()
        runs.append((sp, sp.check()))
    for sp, c in runs[1:]:
        _same_games(runs[0][0], runs[0][1], sp, c)


T, SIMS = 16, 25


def _dump_forest(sp, eng, o, starts):
    """BFS over every tree t through visited children from each state of starts[t]:
    {tree: {hash: (state, ids, N, Q, P)}} (tests/test_search_parity_gpu.py, at T trees)."""
    trees = [dict() for _ in range(T)]
    frontier = [list(s) for s in starts]
    state_bytes = starts[0][0].shape[0]
    cap = 256
    while any(frontier):
        q = np.zeros((T, state_bytes), dtype=np.uint8)
        act = np.zeros(T, dtype=np.int32)
        cur = [None] * T
        for t in range(T):
            while frontier[t]:
                s = frontier[t].pop()
                h = o.hash(s)
                if h in trees[t] or o.game_ended(s) is not None:
                    continue
                cur[t], q[t], act[t] = s, s, 1
                break
        if not act.any():
            break
        ids, n, qv, p, k = sp.mcts.root_stats(torch.from_numpy(q).to(eng.device),
                                              torch.from_numpy(act).to(eng.device), cap)
        ids, n, qv, p, k = (x.cpu().numpy() for x in (ids, n, qv, p, k))
        for t in range(T):
            if not act[t]:
                continue
            K = int(k[t])
            assert K > 0, f"tree {t}: a visited node is missing from the table"
            s = cur[t]
            trees[t][o.hash(s)] = (s, ids[t, :K].copy(), n[t, :K].astype(np.int64), qv[t, :K].copy(), p[t, :K].copy())
            for i in np.nonzero(n[t, :K])[0]:
                frontier[t].append(o.next_state(s, int(ids[t, i]))[0])
    return trees


def test_search_matches_oracle_replay(monkeypatch):
    """16 trees x 25 simulations of the captured simulation graph on the np leaf net, replayed
    tree by tree through MCTSOracle with the GPU's own leaf evaluations: every expanded node's N
    and Q (float64) and the root pi bit for bit; the stored priors against an fp64 masked softmax.
    The leaves are recomputed in 16-row batches at four boards per workgroup, the search's own
    ran at one: the replay rests on the outputs not depending on either."""
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.nets import net_math

    eng, model = _setup()
    o = Oracle(7, 2, 5)
    monkeypatch.setenv("BK_X3_PACK", "1")
    sp = SelfPlay(eng, model, T, num_sims=SIMS, seed=1, cap=256, x3_boards="all")
    ev = sp.evaluator
    assert ev.sparse and ev.planar and sp._graph_usable() and net_math() == "x3"
    assert ev.model.x3_entry(7) == "np"
    sp.roots = random_boards(eng, T, seed0=21, max_plies=4)
    assert not bool(eng.game_ended(sp.roots)[0].any())
    sp._simulations(SIMS)
    c = sp.check()
    assert c["expanded"] + c["terminal"] == T * SIMS
    roots_h = sp.roots.cpu().numpy()
    rids, rpi, rk = (x.cpu().numpy() for x in sp.mcts.root_policy(sp.roots, sp.active, 1.0))
    trees = _dump_forest(sp, eng, o, [[roots_h[t]] for t in range(T)])
    assert sum(len(tr) for tr in trees) == c["expanded"]

    monkeypatch.setenv("BK_X3_PACK", "4")
    keys = [(t, h) for t in range(T) for h in trees[t]]
    vals, feats = {}, {}
    for i in range(0, len(keys), T):
        chunk = keys[i:i + T]
        st = np.zeros((T, roots_h.shape[1]), dtype=np.uint8)
        for j, (t, h) in enumerate(chunk):
            st[j] = trees[t][h][0]
        pf, v = ev._forward(eng.observe(torch.from_numpy(st).to(eng.device)))
        v, pf = v.cpu().numpy(), pf.cpu().numpy()
        for j, key in enumerate(chunk):
            vals[key], feats[key] = v[j].astype(np.float64), pf[j]

    W = ev.policy_w.cpu().double().numpy()
    b = ev.policy_b.cpu().double().numpy()
    for t, h in keys:
        _, ids, _, _, P = trees[t][h]
        lg = W[ids] @ feats[(t, h)].astype(np.float64) + b[ids]
        e = np.exp(lg - lg.max())
        np.testing.assert_allclose(P, e / e.sum(), rtol=1e-5, atol=1e-7, err_msg=str((t, h)))

    for t in range(T):
        nodes = trees[t]

        def evaluate(s, player, t=t, nodes=nodes):
            h = o.hash(s)
            _, ids, _, _, P = nodes[h]
            assert (ids == o.legal_ids(s, player)).all()
            return ids, P, vals[(t, h)]

        m = MCTSOracle(o, evaluate)
        for _ in range(SIMS):
            m.simulate(roots_h[t], cpuct=sp.cpuct)
        assert set(m.tree) == set(nodes), t
        for h, nd in m.tree.items():
            _, ids, N, Q, _ = nodes[h]
            assert nd["N"] == N.tolist(), (t, h)
            assert nd["Q"] == Q.tolist(), (t, h)
        oids, d = m.get_distribution(roots_h[t], 1.0)
        K = int(rk[t])
        assert (rids[t, :K] == oids).all() and rpi[t, :K].tolist() == d.tolist(), t


def test_predict_with_the_knob_is_fp32_class_of_predict_without(monkeypatch):
    from blokus_rl_amd.boards import random_boards
    from blokus_rl_amd.colossumrl import ColosseumBlokusGameWrapper
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.hparams import AlphaZeroHparams
    from blokus_rl_amd.nets import LeafResNet
    from blokus_rl_amd.neural_network import BlokusNNetWrapper

    hp = AlphaZeroHparams(board_size=7, number_of_players=2, num_res_blocks=2, model_type="resnet")
    game = ColosseumBlokusGameWrapper(hp)
    torch.manual_seed(3)
    nn = BlokusNNetWrapper(game, hp, device=game.device)
    eng = Engine(7, 2, 5)
    states = random_boards(eng, 9, seed0=2, max_plies=8)
    obs = eng.observe(states)
    monkeypatch.delenv("BK_X3_BOARDS", raising=False)
    lp0, v0 = nn.predict_batch(obs)
    lps0, vs0 = nn.predict_states(states)
    assert isinstance(nn._infer, LeafResNet) and not nn._infer.takes_states()
    monkeypatch.setenv("BK_X3_BOARDS", "all")
    nn._infer = None  # the evaluator form is built on first use
    lp1, v1 = nn.predict_batch(obs)
    lps1, vs1 = nn.predict_states(states)
    assert nn._infer.takes_states() and nn._infer.x3_entry(7) == "np"
    assert torch.equal(lps1, lp1) and torch.equal(vs1, v1)
    assert not torch.equal(lp1, lp0)  # another kernel
    for a, b, atol in ((lp1, lp0, 1e-5), (lps1, lps0, 1e-5), (v1, v0, 1e-6), (vs1, vs0, 1e-6)):
        assert torch.allclose(a, b, rtol=1e-5, atol=atol), float((a - b).abs().max())
