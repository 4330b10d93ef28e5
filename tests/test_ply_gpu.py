"""The self-play ply tail (csrc/ply.hip: bk_ply_policy, bk_ply_finish) against its NumPy
restatement (oracle/ply_oracle.py), draw for draw: the random numbers are counter-based, so the
oracle predicts every sampled action, every noise entry and every restart, and nothing here is
statistical (the oracle's own law is pinned in tests/test_ply_oracle.py). Synthetic rows at the
production width (cap = 4096, K across every chunk-size step of the inverse CDF), both Gamma
branches of the noise, the finish kernel across its 1024-game passes, and the production
self-play path end to end at 20x20."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ply_oracle as po

pytestmark = pytest.mark.gpu

A20 = 30433  # action ids of the 20x20 preset fit int16


@pytest.fixture(scope="module")
def eng():
    from blokus_rl_amd.engine import Engine
    return Engine(20, 4, 5)


def _dev(a, eng):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _roots(eng, to_move):
    from blokus_rl_amd.engine import W_TO_MOVE

    roots = eng.init_states(len(to_move))
    roots.view(torch.int32)[:, W_TO_MOVE] = _dev(np.asarray(to_move, dtype=np.int32), eng)
    return roots


def ply_policy_gpu(eng, ids, pi, counts, active, first_ply, cap, weight, alpha, seed, ply, to_move):
    """bk_ply_policy on host arrays -> dict of host arrays; the outputs start from sentinels."""
    from blokus_rl_amd.engine import _check, _ptr

    G = len(counts)
    d = [_dev(np.asarray(ids, dtype=np.int32), eng), _dev(np.asarray(pi, dtype=np.float64), eng),
         _dev(np.asarray(counts, dtype=np.int32), eng), _dev(np.asarray(active, dtype=np.int32), eng),
         _dev(np.asarray(first_ply, dtype=np.uint8), eng)]
    roots = _roots(eng, to_move)
    action = torch.full((G,), -77, dtype=torch.int32, device=eng.device)
    ids16 = torch.full((G, cap), -1, dtype=torch.int16, device=eng.device)
    pi32 = torch.full((G, cap), float("nan"), dtype=torch.float32, device=eng.device)
    act = torch.full((G,), 9, dtype=torch.uint8, device=eng.device)
    player = torch.full((G,), -77, dtype=torch.int32, device=eng.device)
    _check(eng.lib.bk_ply_policy(*[_ptr(t) for t in d], G, cap, float(weight), float(alpha), int(seed), int(ply),
                                 _ptr(roots), _ptr(action), _ptr(ids16), _ptr(pi32), _ptr(act), _ptr(player),
                                 eng._s()))
    torch.cuda.synchronize()
    return dict(action=action.cpu().numpy(), ids16=ids16.cpu().numpy(), pi32=pi32.cpu().numpy(),
                act_mask=act.cpu().numpy(), player=player.cpu().numpy())


def _garbage_ids(rng, counts, cap):
    """Ids in [0, A20) below each row's count, arbitrary words at and beyond it."""
    G = len(counts)
    ids = rng.integers(-2 ** 31, 2 ** 31, size=(G, cap)).astype(np.int32)
    col = np.arange(cap)[None, :]
    return np.where(col < np.maximum(counts, 0)[:, None], rng.integers(0, A20, size=(G, cap)), ids).astype(np.int32)


def _ulps(a, b):
    """Distance in float32 steps between non-negative float32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---------------------------------------------------------------- a. draws without noise
@pytest.fixture(scope="module")
def corpus():
    """The draw corpus (1050 games: 15 K x (64 random + 6 structural rows), NaN / garbage at and
    beyond K) and the oracle's answer per ply, computed once."""
    pi, counts = po.draw_corpus()
    G = len(counts)
    rng = np.random.default_rng(99)
    ids = _garbage_ids(rng, counts, po.CORPUS_CAP)
    to_move = (np.arange(G) * 7 // 3) % 4
    ones, zeros = np.ones(G, dtype=np.int32), np.zeros(G, dtype=np.uint8)
    want = {ply: po.ply_policy(ids, pi, counts, ones, zeros, po.CORPUS_CAP, 0.25, 0.3, po.CORPUS_SEED, ply, to_move)
            for ply in po.CORPUS_PLIES}
    return dict(pi=pi, counts=counts, ids=ids, to_move=to_move, want=want)


@pytest.mark.parametrize("first_ply,weight", [(0, 0.25), (1, 0.0)], ids=["plain", "first-ply-weight0"])
@pytest.mark.parametrize("ply", po.CORPUS_PLIES)
def test_draws_match_oracle(eng, corpus, ply, first_ply, weight):
    """Every K of CORPUS_K (the chunk-size steps 256 -> 257, 512 -> 513, ..., and rows whose last
    thread's chunk holds one entry) x Dirichlet rows, rows with 70% zeros, rows with a zero first
    half, unnormalised rows, and the structural rows (one-hot at 0, K-1, C-1, C, the middle; a
    positive prefix then zeros): records and the sampled action of every game, bit for bit.
    first_ply = 1 with weight 0 runs the noise (alpha 0.3) and must change nothing."""
    c = corpus
    G, cap, counts = len(c["counts"]), po.CORPUS_CAP, c["counts"]
    want = c["want"][ply]
    assert (want["margin"] >= po.MARGIN_MIN).all()  # tests/test_ply_oracle.py: no draw is left out
    got = ply_policy_gpu(eng, c["ids"], c["pi"], counts, np.ones(G), np.full(G, first_ply), cap, weight, 0.3,
                         po.CORPUS_SEED, ply, c["to_move"])
    col = np.arange(cap)[None, :]
    below = col < counts[:, None]
    assert (got["pi32"][below] == c["pi"][below].astype(np.float32)).all()
    assert (got["pi32"][~below] == 0).all()  # NaN beyond K was not read, zeros were written
    assert (got["ids16"] == np.where(below, c["ids"], 0).astype(np.int16)).all()
    assert (got["player"] == c["to_move"]).all()
    assert (got["act_mask"] == 1).all()
    idx = want["index"]
    wrong = np.nonzero(got["action"] != c["ids"][np.arange(G), idx])[0]
    assert len(wrong) == 0, [(int(g), int(counts[g]), int(idx[g])) for g in wrong[:8]]
    assert (got["pi32"][np.arange(G), idx] > 0).all()
    for k in ("pi32", "ids16", "act_mask", "player", "action"):
        assert (got[k] == want[k]).all(), k
    if ply == po.CORPUS_PLIES[0] and first_ply == 0:
        again = ply_policy_gpu(eng, c["ids"], c["pi"], counts, np.ones(G), np.zeros(G), cap, weight, 0.3,
                               po.CORPUS_SEED, ply, c["to_move"])
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), k
        other = ply_policy_gpu(eng, c["ids"], c["pi"], counts, np.ones(G), np.zeros(G), cap, weight, 0.3,
                               po.CORPUS_SEED + 1, ply, c["to_move"])
        assert (other["action"] != got["action"]).any()
        assert other["pi32"].tobytes() == got["pi32"].tobytes()


@pytest.mark.parametrize("K", [257, 1000, 4096])
def test_draw_at_the_ends_of_the_uniform(eng, K):
    """The two draws no seed search reaches, set up by inverting the counter hash, on rows that
    start and end with zeros. u = 1 (target 0) must give the first positive entry. u = 2^-53 puts
    the target one rounding below the total, where the chunk intervals can leave a gap (the scanned
    offsets and the chunk sums round differently once the entries span many binades: the odd
    trials, lognormal over ~28 binades) and the kernel's last-resort search runs: the pick must
    be a positive entry — never one with pi = 0 — with at most rounding left behind it. The bar
    on what is left: a float64 sum of K terms in any order is within K 2^-53 S of the exact S, so
    the target is above S (1 - (K + 1) 2^-53) and a running sum that passes it has an exact value
    above S (1 - (2K + 1) 2^-53); the exact sum behind the pick is therefore at most
    (K + 1) 2^-52 S. On the even trials (entries in [1e-3, 3]: every float64 sum is exact) that
    leaves only the last positive entry."""
    import math

    rng = np.random.default_rng(K)
    cap = 4096
    for trial in range(12):
        r = np.exp(rng.standard_normal(K) * 8.0) if trial % 2 else rng.random(K) * 3.0 + 1e-3
        first, last = K // 4 + trial, K - 1 - K // 4 - trial
        r[:first] = 0.0
        r[last + 1:] = 0.0
        p32 = r.astype(np.float32)
        pi = np.full((1, cap), np.nan)
        pi[0, :K] = r
        counts = np.array([K], dtype=np.int32)
        ids = np.zeros((1, cap), dtype=np.int32)
        ids[0, :K] = rng.permutation(A20)[:K]  # distinct: the action names its position
        ply = 3 + trial
        seed = po.seed_for_draw(2 ** 64 - 1 - trial, ply, 0, po.DRAW_ACTION)
        assert po.draw_index(p32, K, seed, ply, 0)[0] == first
        got = ply_policy_gpu(eng, ids, pi, counts, [1], [0], cap, 0.0, 1.0, seed, ply, [2])
        assert got["action"][0] == ids[0, first], (K, trial)
        seed = po.seed_for_draw(trial, ply, 0, po.DRAW_ACTION)
        got = ply_policy_gpu(eng, ids, pi, counts, [1], [0], cap, 0.0, 1.0, seed, ply, [2])
        at = np.nonzero(ids[0, :K] == got["action"][0])[0]
        assert len(at) == 1 and p32[at[0]] > 0, (K, trial, got["action"][0])
        behind = math.fsum(p32[at[0] + 1:].tolist())
        assert behind <= (K + 1) * 2.0 ** -52 * math.fsum(p32.tolist()), (K, trial, int(at[0]), last)
        if trial % 2 == 0:
            assert at[0] == last == po.draw_index(p32, K, seed, ply, 0)[0]


# ---------------------------------------------------------------- b. rows that take no action
def test_rows_without_action(eng):
    """Inactive games with K > 0 record their pi (no noise, even on a first ply) and take no
    action; counts = 0 and counts < 0 (the root overflowed cap) give an all-zero row."""
    rng = np.random.default_rng(4)
    cap = 512
    counts = np.array([300, 300, 0, 0, -5000, -300, 512, 300, 1, -1, 0, 257], dtype=np.int32)
    active = np.array([0, 0, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0], dtype=np.int32)
    first = np.array([0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1], dtype=np.uint8)
    G = len(counts)
    pi = np.full((G, cap), np.nan)
    for g, K in enumerate(counts):
        if K > 0:
            pi[g, :K] = rng.dirichlet(np.ones(K))
    ids = _garbage_ids(rng, counts, cap)
    to_move = np.arange(G) % 4
    want = po.ply_policy(ids, pi, counts, active, first, cap, 0.25, 0.3, 5, 2, to_move)
    assert (want["margin"] >= po.MARGIN_MIN).all()
    got = ply_policy_gpu(eng, ids, pi, counts, active, first, cap, 0.25, 0.3, 5, 2, to_move)
    quiet = np.array([0, 1, 2, 3, 4, 5, 8, 9, 10, 11])
    assert (got["action"][quiet] == -1).all() and (got["act_mask"][quiet] == 0).all()
    assert (got["act_mask"][[6, 7]] == 1).all() and (got["action"][[6, 7]] >= 0).all()
    for g in (2, 3, 4, 5, 9, 10):
        assert not got["pi32"][g].any() and not got["ids16"][g].any()
    for g in (0, 1, 8, 11, 7):  # inactive, or not a first ply: pi as it came
        K = counts[g]
        assert (got["pi32"][g, :K] == pi[g, :K].astype(np.float32)).all() and not got["pi32"][g, K:].any()
    noisy = 6  # the one active first-ply row: the rule of the noise test
    assert _ulps(got["pi32"][noisy], want["pi32"][noisy]).max() <= 1
    assert (np.delete(got["pi32"], noisy, 0) == np.delete(want["pi32"], noisy, 0)).all()
    i, margin = po.draw_index(got["pi32"][noisy], 512, 5, 2, noisy)
    assert margin >= po.MARGIN_MIN and got["action"][noisy] == ids[noisy, i]
    for k in ("ids16", "act_mask", "player"):
        assert (got[k] == want[k]).all(), k
    assert (np.delete(got["action"], noisy) == np.delete(want["action"], noisy)).all()


# ---------------------------------------------------------------- c. noise
NOISE_K = (1, 2, 257, 1000, 4096)


def _check_noisy_rows(got32, want32, rows, counts, tag):
    """First-ply rows against the oracle's mix: within 1 float32 ulp everywhere and bit-equal in
    at least 99.9% of the entries (device and host log / cos / pow differ by a few float64 ulps,
    which moves a float32 rounding about once in 1e5 entries), none negative."""
    n = bad = 0
    for g in rows:
        K = counts[g]
        d = _ulps(got32[g, :K], want32[g, :K])
        assert d.max() <= 1, (tag, g, K, int(d.max()))
        assert (got32[g, :K] >= 0).all() and not got32[g, K:].any()
        n += K
        bad += int((d != 0).sum())
    print(f"{tag}: {bad} of {n} first-ply pi32 entries differ from the oracle by 1 ulp ({bad / max(n, 1):.2e})")
    assert bad <= 1e-3 * n, (tag, bad, n)
    return bad, n


@pytest.mark.parametrize("weight,alpha", [(0.25, 1.0), (0.25, 0.3), (0.25, 3.0), (1.0, 0.3)])
def test_noise_matches_oracle(eng, weight, alpha):
    """pi = (1 - w) pi + w Dir(alpha) on first plies: the exponential branch (alpha 1),
    Marsaglia-Tsang (3) and its boost (0.3), K from 1 to the full row, every other game a first
    ply. The action is the oracle's draw from the device's own float32 row, exactly."""
    rng = np.random.default_rng(17)
    cap, seed, ply = 4096, 5, 7
    counts = np.repeat(np.array(NOISE_K, dtype=np.int32), 16)
    G = len(counts)
    first = (np.arange(G) % 2).astype(np.uint8)
    pi = np.full((G, cap), np.nan)
    for g, K in enumerate(counts):
        pi[g, :K] = rng.dirichlet(np.ones(K))
    ids = _garbage_ids(rng, counts, cap)
    to_move = np.arange(G) % 4
    want = po.ply_policy(ids, pi, counts, np.ones(G), first, cap, weight, alpha, seed, ply, to_move)
    got = ply_policy_gpu(eng, ids, pi, counts, np.ones(G), first, cap, weight, alpha, seed, ply, to_move)
    for k in ("ids16", "act_mask", "player"):
        assert (got[k] == want[k]).all(), k
    plain = np.nonzero(first == 0)[0]
    assert (got["pi32"][plain] == want["pi32"][plain]).all()
    _check_noisy_rows(got["pi32"], want["pi32"], np.nonzero(first)[0], counts, f"w={weight} alpha={alpha}")
    for g in range(G):
        K = counts[g]
        assert abs(got["pi32"][g, :K].astype(np.float64).sum() - 1.0) < 1e-6, g
        i, margin = po.draw_index(got["pi32"][g], K, seed, ply, g)
        assert margin >= po.MARGIN_MIN, (g, margin)  # a draw this near a boundary: take another seed
        assert got["action"][g] == ids[g, i] and got["pi32"][g, i] > 0, (g, K, i)
    if weight == 1.0:  # pure noise: the rows are the Dirichlet points themselves
        g = int(np.nonzero(first & (counts == 1000))[0][0])
        assert not np.allclose(got["pi32"][g, :1000], pi[g, :1000].astype(np.float32))


# ---------------------------------------------------------------- d. bk_ply_finish
def ply_finish_gpu(eng, G, P, ended, scores, counts, act_mask, game_id, roots, init_state, continuous, num_sims,
                   active, first_ply, z_table, z_known, zcap, next_gid, fin_count, sims_count, cap_overflow):
    from blokus_rl_amd.engine import _check, _ptr

    dev = eng.device
    t = dict(ended=_dev(ended, eng), scores=_dev(scores, eng), counts=_dev(counts, eng), act_mask=_dev(act_mask, eng),
             game_id=_dev(game_id, eng), roots=_dev(roots, eng), active=_dev(active, eng),
             first_ply=_dev(first_ply, eng), z_table=_dev(z_table, eng), z_known=_dev(z_known, eng))
    reset_flags = torch.full((G,), -77, dtype=torch.int32, device=dev)
    game_id_out = torch.full((G,), -77, dtype=torch.int64, device=dev)
    roots_out = torch.full((G, 384), 0xEE, dtype=torch.uint8, device=dev)
    sc = [torch.full((), v, dtype=dt, device=dev) for v, dt in
          ((next_gid, torch.int64), (fin_count, torch.int64), (sims_count, torch.int64), (cap_overflow, torch.int32))]
    _check(eng.lib.bk_ply_finish(G, P, _ptr(t["ended"]), _ptr(t["scores"]), _ptr(t["counts"]), _ptr(t["act_mask"]),
                                 _ptr(t["game_id"]), _ptr(t["roots"]), _ptr(init_state), int(continuous),
                                 int(num_sims), _ptr(t["active"]), _ptr(t["first_ply"]), _ptr(reset_flags),
                                 _ptr(game_id_out), _ptr(roots_out), _ptr(t["z_table"]), _ptr(t["z_known"]),
                                 ctypes.c_int64(zcap), *[_ptr(s) for s in sc], eng._s()))
    torch.cuda.synchronize()
    out = {k: t[k].cpu().numpy() for k in ("active", "first_ply", "z_table", "z_known")}
    out.update(reset_flags=reset_flags.cpu().numpy(), game_id_out=game_id_out.cpu().numpy(),
               roots_out=roots_out.cpu().numpy(), next_gid=int(sc[0]), fin_count=int(sc[1]), sims_count=int(sc[2]),
               cap_overflow=int(sc[3]))
    return out


@pytest.mark.parametrize("continuous", [0, 1])
@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 1024, 1025, 2500])
def test_ply_finish_matches_oracle(eng, G, P, continuous):
    """Everything bk_ply_finish writes, exact, around the wave (64) and pass (1024) boundaries of
    its prefix count: ~30% of the games ended, some of them inactive (not done), random active /
    act_mask / first_ply, game ids with -1 and ids >= zcap (no write), sentinels in the z table,
    counters that start non-zero. Three runs: overflowed roots with the latch at 0 (-> 1), no
    overflow with the latch at 1 (stays 1), no overflow with the latch at 0 (stays 0)."""
    init_state = eng.init_states(1)
    init_h = init_state.cpu().numpy()[0]
    for run, (neg_counts, latch) in enumerate(((True, 0), (False, 1), (False, 0))):
        rng = np.random.default_rng(1000 * G + 10 * P + 3 * continuous + run)
        ended = (rng.random(G) < 0.3).astype(np.int32)
        active = rng.choice(np.array([0, 1, 1, 1, 2], dtype=np.int32), size=G)
        if G > 1:
            ended[:2], active[:2] = (1, 1), (1, 0)  # a done game and an ended inactive one
            ended[-1], active[-1] = 1, 1  # and a done game in the last wave of the last pass
        act_mask = (rng.random(G) < 0.6).astype(np.uint8)
        first_ply = (rng.random(G) < 0.5).astype(np.uint8)
        counts = rng.integers(1, 2000, size=G).astype(np.int32)
        if neg_counts:
            counts[rng.random(G) < 0.1] = -3000
            counts[0], active[0] = -2100, 1
        else:  # counts < 0 only where the game is inactive: no overflow
            counts[(rng.random(G) < 0.1) & (active == 0)] = -3000
        zcap = G + 8
        game_id = rng.permutation(zcap)[:G].astype(np.int64)  # distinct: one writer per z row
        kind = rng.random(G)
        game_id[kind < 0.1] = -1
        big = (kind >= 0.1) & (kind < 0.2)
        game_id[big] = zcap + rng.integers(0, 5, size=int(big.sum()))
        scores = rng.standard_normal((G, P)) * 3
        roots = rng.integers(0, 256, size=(G, 384)).astype(np.uint8)
        z_table = np.full((zcap + 6, P), -7.5, dtype=np.float32)  # rows past zcap: guard the bound
        z_known = np.full(zcap + 6, 2, dtype=np.uint8)
        args = (G, P, ended, scores, counts, act_mask, game_id, roots)
        tail = (continuous, 13, active, first_ply, z_table, z_known, zcap, 1_000_003, 77, 5_000_000_000, latch)
        want = po.ply_finish(*args, init_h, *tail)
        got = ply_finish_gpu(eng, *args, init_state, *tail)
        assert want["cap_overflow"] == (1 if neg_counts or latch else 0)
        for k in ("next_gid", "fin_count", "sims_count", "cap_overflow"):
            assert got[k] == want[k], (run, k, got[k], want[k])
        for k in ("active", "first_ply", "reset_flags", "game_id_out", "roots_out", "z_table", "z_known"):
            bad = np.nonzero((got[k] != want[k]).reshape(G if k not in ("z_table", "z_known") else zcap + 6, -1).any(1))[0]
            assert len(bad) == 0, (run, k, bad[:8].tolist())
        done = (active != 0) & (ended != 0)
        assert want["fin_count"] == 77 + int(done.sum())
        if continuous and done.any():  # new ids: next_gid + rank among the done games in slot order
            assert (got["game_id_out"][done] == 1_000_003 + np.arange(int(done.sum()))).all()
            assert (got["roots_out"][done] == init_h).all()


# ---------------------------------------------------------------- e. the production path
def test_selfplay_actions_match_oracle_20x20():
    """SelfPlay.play_ply at the production shape (20x20, 4 players, cap 2048, alpha 0.3 noise):
    after every ply each game's last_action is the oracle's draw from that ply's recorded pi32 /
    ids16 / counts under (sp._seed, ply index, game), through rows with K > 256 where a thread's
    chunk of the inverse CDF holds several entries; on the first ply the recorded pi32 is the
    oracle's mix of root_policy's pi."""
    from blokus_rl_amd.alphazero.selfplay import SelfPlay
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import DumbNet

    eng = Engine(20, 4, 5)
    G, plies = 16, 20
    torch.manual_seed(0)
    sp = SelfPlay(eng, DumbNet(20, 4, eng.A).to(eng.device).eval(), G, num_sims=6, seed=5, dirichlet_alpha=0.3)
    searched = []
    inner = sp.mcts.root_policy

    def root_policy(*a, **kw):
        out = inner(*a, **kw)
        searched.append(out)
        return out

    sp.mcts.root_policy = root_policy
    kmax = 0
    for ply in range(plies):
        first = sp.first_ply.cpu().numpy().astype(np.uint8)
        active = sp.active.cpu().numpy()
        sp.play_ply()
        _, ids16, pi32, counts, player, _, act = (x.cpu().numpy() for x in sp._records[-1])
        action = sp.last_action.cpu().numpy()
        assert (first == (1 if ply == 0 else 0)).all() and act.all()
        if ply == 0:
            ids, pi, cnt = (x.cpu().numpy() for x in searched[-1])
            want = po.ply_policy(ids, pi, cnt, active, first, sp.cap, sp.weight, sp.alpha, sp._seed, ply, player)
            assert (cnt == counts).all() and (want["ids16"] == ids16).all()
            _check_noisy_rows(pi32, want["pi32"], range(G), counts, "self-play first ply")
        for g in range(G):
            K = int(counts[g])
            i, margin = po.draw_index(pi32[g], K, sp._seed, ply, g)
            assert margin >= po.MARGIN_MIN, (ply, g, margin)  # a draw this near a boundary: take another seed
            assert action[g] == ids16[g, i] and pi32[g, i] > 0, (ply, g, K, i)
        kmax = max(kmax, int(counts.max()))
    sp.check()
    assert kmax > 256, kmax
