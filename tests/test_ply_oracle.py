"""oracle/ply_oracle.py's own law (CPU): the GPU test of the ply tail (tests/test_ply_gpu.py)
compares bk_ply_policy / bk_ply_finish with this restatement draw for draw, so what is checked
here is that the restatement samples what the reference episode samples (trainer.py:108-135:
Dir(alpha) noise, np.random.choice from pi) and that the draws the GPU test uses do not depend on
the order the probabilities are summed in."""
import numpy as np
import pytest
from scipy import stats as st

from oracle import ply_oracle as po
from oracle.vecenv_oracle import mix64 as mix64_int

N = 4096


def test_rng_restatement():
    """The vectorised mix64 is the scalar one; ply_rng is its documented composition; u01 covers
    (0, 1] with 53 bits; unmix64 / seed_for_draw invert them."""
    rng = np.random.default_rng(0)
    xs = rng.integers(0, 1 << 64, size=64, dtype=np.uint64)
    xs[:3] = (0, (1 << 64) - 1, 0x9E3779B97F4A7C15)
    assert po.mix64(xs).tolist() == [mix64_int(int(x)) for x in xs]
    assert [po.unmix64(mix64_int(int(x))) for x in xs] == xs.tolist()
    m = (1 << 64) - 1
    for seed, ply, g, d in ((0, 0, 0, 0), (5, 7, 1049, 0x7FFFFFFF), (m, 123456789012, 65535, 4095 * 128 + 96)):
        want = mix64_int((mix64_int(seed ^ mix64_int(ply)) + (g << 24) + d) & m)
        assert int(po.ply_rng(seed, ply, g, d)) == want
        assert po.seed_for_draw(want, ply, g, d) == seed
    got = po.ply_rng(5, 7, np.arange(4)[:, None], np.arange(3)[None, :])
    assert got.shape == (4, 3) and int(got[2, 1]) == int(po.ply_rng(5, 7, 2, 1))
    assert po.u01(np.array([0, m], dtype=np.uint64)).tolist() == [2.0 ** -53, 1.0]
    assert float(po.u01(np.uint64(1 << 63))) == 0.5 + 2.0 ** -53


@pytest.mark.parametrize("alpha", [0.3, 1.0, 3.0])
def test_gamma_draw_law(alpha):
    """4096 draws against scipy's Gamma(alpha) (Kolmogorov-Smirnov, p > 1e-4): the exponential
    branch, Marsaglia-Tsang, and its u^(1/alpha) boost below 1."""
    x = po.gamma_draw(alpha, seed=5, ply=0, game=3, idx=np.arange(N))
    assert x.shape == (N,) and (x > 0).all() and np.isfinite(x).all()
    assert st.kstest(x, st.gamma(alpha).cdf).pvalue > 1e-4
    # entries own their draw slots: an entry's value does not depend on which others are drawn
    assert (po.gamma_draw(alpha, 5, 0, 3, np.array([77, 5, 4000])) == x[[77, 5, 4000]]).all()
    assert (po.gamma_draw(alpha, 5, 1, 3, np.arange(64)) != x[:64]).all()  # another ply: other draws


def test_dirichlet_noise_law():
    """Dir(0.3) over K = 8 ids, one point per game: on the simplex, coordinate 0 ~ Beta(0.3, 2.1)."""
    K, alpha = 8, 0.3
    pts = np.stack([po.dirichlet_noise(alpha, 5, 0, g, K) for g in range(N)])
    assert (pts >= 0).all() and np.abs(pts.sum(1) - 1).max() < 1e-12
    assert st.kstest(pts[:, 0], st.beta(alpha, alpha * (K - 1)).cdf).pvalue > 1e-4
    assert st.kstest(pts[:, K - 1], st.beta(alpha, alpha * (K - 1)).cdf).pvalue > 1e-4


def test_draw_corpus_margins_and_associations():
    """Every draw of the GPU test's corpus (every K of CORPUS_K, the four row kinds and the
    structural rows, seed 5, plies 0 and 7) lies at least 2^-40 of the total from every CDF
    boundary — rounding of float64 sums moves a boundary by ~2^-50 — so the drawn index cannot
    depend on the association, and the kernel's association (256 chunks, exclusive scan, walk),
    restated in draw_index_chunked, picks the index of the sequential sum on all of them. A
    condition on the corpus, not a tolerance: should a seed ever give a draw under the margin,
    take another seed."""
    pi, counts = po.draw_corpus()
    assert len(counts) == len(po.CORPUS_K) * 70 and sorted(set(counts.tolist())) == sorted(po.CORPUS_K)
    worst = 1.0
    for ply in po.CORPUS_PLIES:
        for g, K in enumerate(counts.tolist()):
            assert np.isnan(pi[g, K:]).all()
            p32 = pi[g, :K].astype(np.float32)
            i, margin = po.draw_index(p32, K, po.CORPUS_SEED, ply, g)
            assert 0 <= i < K and p32[i] > 0
            assert margin >= po.MARGIN_MIN, (ply, g, K, margin)
            assert po.draw_index_chunked(p32, K, po.CORPUS_SEED, ply, g) == i, (ply, g, K)
            worst = min(worst, margin)
    print(f"smallest margin {worst:.3e} (bar {po.MARGIN_MIN:.3e})")


def test_draw_index_by_hand():
    """The inverse CDF on rows small enough to read: zero entries are never drawn, the ends of
    u01 land on the first and last positive entry, the counts of 4096 draws follow p."""
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25, 0.0], dtype=np.float32)
    picks = np.array([po.draw_index(p, 6, 9, 0, g)[0] for g in range(N)])
    assert set(picks.tolist()) == {1, 3, 4}
    obs = np.bincount(picks, minlength=6)[[1, 3, 4]]
    assert st.chisquare(obs, N * np.array([0.25, 0.5, 0.25])).pvalue > 1e-4
    m = (1 << 64) - 1
    lo = po.seed_for_draw(m, 3, 2, po.DRAW_ACTION)  # u = 1: target 0
    hi = po.seed_for_draw(0, 3, 2, po.DRAW_ACTION)  # u = 2^-53: target within an ulp of the total
    assert po.draw_index(p, 6, lo, 3, 2)[0] == 1 and po.draw_index_chunked(p, 6, lo, 3, 2) == 1
    assert po.draw_index(p, 6, hi, 3, 2)[0] == 4 and po.draw_index_chunked(p, 6, hi, 3, 2) == 4
    assert po.draw_index(np.zeros(4, np.float32), 4, 1, 0, 0)[0] == -1


def test_ply_policy_rows():
    """ply_policy's bookkeeping on a hand-made batch: no noise without first_ply or weight,
    inactive and empty rows take no action, rows are cut at their count."""
    rng = np.random.default_rng(2)
    G, cap = 6, 16
    counts = np.array([5, 16, 7, 0, -20, 3], dtype=np.int32)
    active = np.array([1, 1, 0, 1, 1, 1], dtype=np.int32)
    first = np.array([0, 1, 1, 1, 1, 1], dtype=np.uint8)
    ids = rng.integers(0, 30433, size=(G, cap)).astype(np.int32)
    pi = np.full((G, cap), np.nan)
    for g, K in enumerate(counts):
        if K > 0:
            pi[g, :K] = rng.dirichlet(np.ones(K))
    r = po.ply_policy(ids, pi, counts, active, first, cap, 0.25, 0.3, 11, 4, np.arange(G) % 4)
    assert r["act_mask"].tolist() == [1, 1, 0, 0, 0, 1] and r["player"].tolist() == [0, 1, 2, 3, 0, 1]
    assert (r["action"][[2, 3, 4]] == -1).all() and not r["pi32"][[3, 4]].any() and not r["ids16"][[3, 4]].any()
    for g in (0, 2):  # no noise: not a first ply / not active
        assert (r["pi32"][g, :counts[g]] == pi[g, :counts[g]].astype(np.float32)).all()
    for g in (1, 5):
        K = counts[g]
        noise = (r["pi32"][g, :K].astype(np.float64) - 0.75 * pi[g, :K]) / 0.25
        assert np.abs(noise - po.dirichlet_noise(0.3, 11, 4, g, K)).max() < 1e-6
        assert abs(r["pi32"][g, :K].sum() - 1) < 1e-6 and not r["pi32"][g, K:].any()
    for g in (0, 1, 5):
        assert r["action"][g] == ids[g, r["index"][g]] and r["pi32"][g, r["index"][g]] > 0
    assert (r["ids16"][1] == ids[1].astype(np.int16)).all()
    w0 = po.ply_policy(ids, pi, counts, active, first, cap, 0.0, 0.3, 11, 4, np.arange(G) % 4)
    assert (w0["pi32"][1] == pi[1].astype(np.float32)).all()


def test_ply_finish_by_hand():
    """ply_finish on six slots, both modes: ids of restarted games in slot order, guards on the z
    table, the counters and the overflow latch."""
    G, P = 6, 2
    ended = np.array([1, 1, 0, 1, 1, 1], dtype=np.int32)
    active = np.array([1, 0, 1, 1, 1, 1], dtype=np.int32)
    counts = np.array([3, 3, -9, 3, 3, 3], dtype=np.int32)
    act_mask = np.array([1, 0, 0, 1, 1, 0], dtype=np.uint8)
    first = np.array([1, 1, 1, 0, 1, 1], dtype=np.uint8)
    gid = np.array([2, 0, 1, -1, 9, 3], dtype=np.int64)
    scores = np.arange(G * P, dtype=np.float64).reshape(G, P) + 0.5
    roots = np.arange(G * 384, dtype=np.uint8).reshape(G, 384)
    init = np.full(384, 7, dtype=np.uint8)
    z = np.full((4, P), -7.5, dtype=np.float32)
    zk = np.full(4, 2, dtype=np.uint8)
    for cont in (False, True):
        r = po.ply_finish(G, P, ended, scores, counts, act_mask, gid, roots, init, cont, 10, active, first, z, zk, 4,
                          100, 5, 1000, 0)
        assert r["reset_flags"].tolist() == [1, 0, 0, 1, 1, 1]  # slot 1 ended but is inactive: not done
        assert r["z_known"].tolist() == [2, 2, 1, 1] and r["z_table"].tolist() == [[-7.5] * 2] * 2 + [[0.5, 1.5], [10.5, 11.5]]
        assert (r["fin_count"], r["sims_count"], r["cap_overflow"]) == (9, 1030, 1)
        if cont:
            assert r["game_id_out"].tolist() == [100, 0, 1, 101, 102, 103] and r["next_gid"] == 104
            assert r["active"].tolist() == active.tolist() and r["first_ply"].tolist() == [1, 1, 1, 1, 1, 1]
            assert (r["roots_out"][[0, 3, 4, 5]] == 7).all() and (r["roots_out"][[1, 2]] == roots[[1, 2]]).all()
        else:
            assert r["game_id_out"].tolist() == gid.tolist() and r["next_gid"] == 100
            assert r["active"].tolist() == [0, 0, 1, 0, 0, 0] and r["first_ply"].tolist() == [0, 1, 1, 0, 0, 1]
            assert (r["roots_out"] == roots).all()
    r = po.ply_finish(G, P, ended, scores, np.abs(counts), act_mask, gid, roots, init, True, 10, active, first, z, zk,
                      4, 100, 5, 1000, 1)
    assert r["cap_overflow"] == 1  # the latch is never cleared
