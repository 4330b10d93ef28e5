"""Rules, expansion priors and the sparse policy head at child counts random boards never reach.

The roots are the big-K fixture's states (tests/golden/make_bigk_states.py): K = 1 .. 5056 legal
moves, on both sides of every K at which the search kernels change path — 64 (one wave), 768
(select_child's register path), 1024 (kGatherRegs * 64: the softmax's register round, beyond it the
strided tails), 2048 (kExpandLdsIds: ids compacted in LDS; kLeafCap: the sparse head's limit). One
BatchedMCTS holds all states of a preset as the roots of its trees, so a launch covers every K.

The priors are observed through root_stats' P and compared with a float64 masked softmax under a
derived bound (check_priors), not a measured one. Each test prints its largest error / bound ratio.
"""
import contextlib
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import bigk_util
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

PRESETS = [(20, 2, 5), (20, 4, 5), (14, 2, 5), (7, 2, 5)]
LEAF_CAP = 2048  # kLeafCap
U = 2.0 ** -24   # float32 unit roundoff


@lru_cache(maxsize=None)
def _engine(preset):
    from blokus_rl_amd.engine import Engine

    return Engine(*preset)


@lru_cache(maxsize=None)
def _fixture(preset):
    """(K list, states on the host, the oracle's ids per state)."""
    o = Oracle(*preset)
    Ks, st = bigk_util.states_of(preset)
    ids = [o.legal_ids(s) for s in st]
    assert [len(i) for i in ids] == Ks
    return Ks, st, ids


def _mcts(eng, T, per_tree):
    from blokus_rl_amd.alphazero.batched_mcts import BatchedMCTS

    return BatchedMCTS(eng, T, node_cap=16, child_cap=T * per_tree)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_priors(P: np.ndarray, x: np.ndarray, logit_err: float = 0.0) -> float:
    """P (float32) against softmax(x) in float64. With d_i = x_i - max - lse:
        |P_i - Pref_i| <= Pref_i * ((2 |d_i| + 64) * 2^-24 + 2 * logit_err).
    The kernel computes expf((x - max) - lse): the two subtractions round at |x - max| <= |d| and |d|;
    lse = logf(sum) carries the sum's error (<= 32 positive terms a lane plus 6 shuffle adds) and a
    few ulp of logf; expf adds a few ulp. logit_err bounds the absolute error of every x_i the kernel
    computed itself (the sparse head): a softmax moves by at most exp(2 max|dx|) - 1 relative.
    Below Pref = 2^-120 (float32's subnormal edge) only 0 <= P <= 2^-119 is required. Also
    |sum P - 1| <= 2^-20. Returns the largest error / bound ratio."""
    x = x.astype(np.float64)
    P = P.astype(np.float64)
    assert P.shape == x.shape and np.isfinite(P).all()
    z = x - x.max()
    d = z - np.log(np.exp(z).sum())
    ref = np.exp(d)
    tol = ref * ((2.0 * np.abs(d) + 64.0) * U + 2.0 * logit_err)
    big = ref >= 2.0 ** -120
    ratio = float((np.abs(P - ref)[big] / tol[big]).max())
    tiny_ok = bool(((P[~big] >= 0.0) & (P[~big] <= 2.0 ** -119)).all())
    total = abs(float(P.sum()) - 1.0)
    check_priors.last = (ratio, total)
    assert tiny_ok, "a prior below 2^-120 came out above 2^-119 or negative"
    assert ratio <= 1.0, f"prior error / bound = {ratio:.3f}"
    assert total <= 2.0 ** -20, f"|sum P - 1| = {total:.3e}"
    return ratio


# ------------------------------------------------------------------------------------- 2a: rules
@pytest.mark.parametrize("preset", PRESETS, ids=lambda p: "x".join(map(str, p)))
def test_rules_match_oracle_at_big_k(preset):
    eng, o = _engine(preset), Oracle(*preset)
    Ks, st_h, ref_ids = _fixture(preset)
    st = torch.from_numpy(st_h).to(eng.device)
    masks, counts = eng.legal_mask(st)
    ref_masks, ref_counts = o.legal_mask_batch(st_h)
    assert counts.cpu().numpy().tolist() == ref_counts.tolist() == Ks
    assert (masks.cpu().numpy().view(np.uint64) == ref_masks).all()
    # a cap above every K, then per state a cap equal to K and one below it
    cap = max(Ks) + 7
    ids, cnt = eng.legal_ids(st, cap=cap)
    ids_h = ids.cpu().numpy()
    assert cnt.cpu().numpy().tolist() == Ks
    for b, K in enumerate(Ks):
        assert (ids_h[b, :K] == ref_ids[b]).all()
    for b, K in enumerate(Ks):
        for cap in sorted({K, K - 1, (K + 1) // 2} - {0}):
            ids, cnt = eng.legal_ids(st[b:b + 1].contiguous(), cap=cap)
            assert int(cnt[0]) == (K if K <= cap else -K), (K, cap)
            assert (ids[0].cpu().numpy() == ref_ids[b][:cap]).all(), (K, cap)


# --------------------------------------------------------------------- 2c: dense masked softmax
def _dense_patterns(K: int, rng):
    """Child logits, by child index: (1) normal x 3; (2) all equal; (3) the largest only at the last
    child, 100 above the rest (a max that forgot the tail overflows the sum); (4) a spread of 120
    with the top three past index 1024 where K allows, else at the end (most terms underflow)."""
    x1 = (3.0 * rng.standard_normal(K)).astype(np.float32)
    x2 = np.full(K, 0.7, dtype=np.float32)
    x3 = rng.standard_normal(K).astype(np.float32)
    x3[K - 1] = 100.0
    x4 = rng.uniform(-120.0, -40.0, K).astype(np.float32)
    x4[0] = -120.0
    top = [i for i in (K - 1, K - 2, 1024 + (K - 1024) // 2) if 0 <= i < K and (K <= 1024 or i >= 1024)]
    for n, i in enumerate(sorted(set(top))):
        x4[i] = -0.5 * n
    return [x1, x2, x3, x4]


@pytest.mark.parametrize("preset", PRESETS, ids=lambda p: "x".join(map(str, p)))
def test_dense_softmax_priors_match_fp64(preset):
    eng = _engine(preset)
    dev = eng.device
    Ks, st_h, ref_ids = _fixture(preset)
    T, cap = len(Ks), max(Ks)
    roots = torch.from_numpy(st_h).to(dev)
    rng = np.random.default_rng(2024)
    pats = [_dense_patterns(K, rng) for K in Ks]
    vals = torch.zeros((T, eng.P), dtype=torch.float32, device=dev)
    low = sorted(Ks)[len(Ks) // 2] - 1 if T > 1 else 1  # a cap below about half of the K
    for pat in range(4):
        m = _mcts(eng, T, cap + 64)
        # the illegal ids hold large logits: a softmax that is not masked is far off
        logp_h = rng.uniform(20.0, 130.0, (T, eng.A)).astype(np.float32)
        for t in range(T):
            logp_h[t, ref_ids[t]] = pats[t][pat]
        status, _, _ = m.select(roots, None, 1.0)
        assert (status == 1).all()
        m.expand_backup(torch.from_numpy(logp_h).to(dev), vals, prior_mode=0)
        c = m.check()
        assert c["expanded"] == T
        ids, n, q, p, counts = (x.cpu().numpy() for x in m.root_stats(roots, None, cap=cap))
        pid, pi1, pc = (x.cpu().numpy() for x in m.root_policy(roots, None, 1.0, cap=cap))
        _, _, _, _, low_counts = m.root_stats(roots, None, cap=low)
        assert low_counts.cpu().numpy().tolist() == [K if K <= low else -K for K in Ks]
        assert counts.tolist() == Ks == pc.tolist()
        worst = 0.0
        for t, K in enumerate(Ks):
            assert (ids[t, :K] == ref_ids[t]).all() and (pid[t, :K] == ref_ids[t]).all()
            assert not n[t, :K].any() and not q[t, :K].any()
            assert np.allclose(pi1[t, :K], 1.0 / K, rtol=1e-14, atol=0.0)  # no visits yet: uniform
            worst = max(worst, check_priors(p[t, :K], pats[t][pat]))
        print(f"dense softmax {preset} pattern {pat + 1}: largest error / bound = {worst:.4f}")


# ------------------------------------------------------------- 2d: sparse head + softmax vs fp64
def _dot_depth(F: int) -> int:
    """The longest chain of float32 additions a product of a leaf logit passes through.
    F % 4 == 0 (row_dot16): 3 inside its float4's dot; 2 per whole trip of four float4s into the
    lane's partial sum (lane 0 makes the most trips); 1 per remainder float4 (at most 3); 1 joining
    the two partial sums; 4 xor-shuffles over the 16 lanes; 1 for the bias.
    Otherwise (the scalar branch): ceil(F / 64) a lane, wave_sum_f's 6 steps, the bias."""
    if F % 4:
        return -(-F // 64) + 6 + 1
    F4 = F // 4
    trips = max(0, -(-(F4 - 48) // 64))
    rem = max(0, -(-(F4 - 64 * trips) // 16))
    assert rem <= 3
    return 3 + 2 * trips + rem + 1 + 4 + 1


def _head_inputs(eng, T: int, F: int, pad: int, seed: int):
    """feat = relu(normal) with aligned blocks of four zeros, tree 0 all zero and tree 1 all positive
    (|normal| + 0.1: whichever float4 a kernel drops, this tree's logits miss it); leading dimension
    F + pad. W ~ normal * 3 / sqrt(F), bias ~ normal."""
    g = torch.Generator(device=eng.device)
    g.manual_seed(seed)
    dev = eng.device
    store = torch.randn((T, F + pad), generator=g, device=dev).clamp_(min=0.0)
    feat = store[:, :F]
    F4 = F // 4
    if F4:
        zero4 = torch.rand((T, F4), generator=g, device=dev) < 0.3
        feat[:, :4 * F4] *= (~zero4).repeat_interleave(4, dim=1).to(torch.float32)
    feat[0] = 0.0
    if T > 1:
        feat[1] = torch.randn(F, generator=g, device=dev).abs() + 0.1
    W = torch.randn((eng.A, F), generator=g, device=dev) * (3.0 / F ** 0.5)
    bias = torch.randn(eng.A, generator=g, device=dev)
    return feat, W.contiguous(), bias


def _tree_snapshot(m, roots, cap, rows=None, probe=None):
    ctr = m.counters()  # before root_stats, which flags a root that is not in its tree
    if probe is not None:
        probe(m)
    return [x.cpu().numpy() for x in m.root_stats(roots, rows, cap=cap)], ctr


def _run_sparse(eng, roots, T, per_tree, cap, feat, W, bias, vals, form, rows=None, probe=None):
    """The roots' expansion and three more simulations in prior mode 2. form "stages": select,
    leaf_logits, expand_backup; else the fused leaf_step under (BK_STEP_OVERLAP, BK_LEAF_SKIP0).
    Returns the roots' rows (of the trees flagged in rows, default all) after the first expansion
    and after the last, with the counters; probe(m) is called after the first expansion."""
    m = _mcts(eng, T, per_tree)
    env = {} if form == "stages" else {"BK_STEP_OVERLAP": form[0], "BK_LEAF_SKIP0": form[1]}
    with _env(**env):
        status, _, _ = m.select(roots, None, 1.0)
        assert (status == 1).all()
        snaps = []
        for sim in range(4):
            if form == "stages":
                m.leaf_logits(feat, W, bias)
                m.expand_backup(None, vals, prior_mode=2)
                if sim == 0:
                    snaps.append(_tree_snapshot(m, roots, cap, rows, probe))
                m.select(roots, None, 1.0)
            else:
                if sim == 0:  # without the next descent, to read the tree of the first expansion alone
                    m.leaf_step(feat, W, bias, vals)
                    snaps.append(_tree_snapshot(m, roots, cap, rows, probe))
                    m.select(roots, None, 1.0)
                else:
                    m.leaf_step(feat, W, bias, vals, roots=roots)
        snaps.append(_tree_snapshot(m, roots, cap, rows))
    return snaps


FORMS = ["stages", (0, 1), (1, 0), (1, 1)]


def _same(a, b):
    (rows_a, ctr_a), (rows_b, ctr_b) = a, b
    return ctr_a == ctr_b and all(x.tobytes() == y.tobytes() for x, y in zip(rows_a, rows_b))


def _sparse_case(preset, F: int, pad: int, spike: bool = False):
    eng = _engine(preset)
    dev = eng.device
    Ks, st_h, ref_ids = _fixture(preset)
    keep = [t for t, K in enumerate(Ks) if K <= LEAF_CAP]
    Ks, st_h, ref_ids = [Ks[t] for t in keep], st_h[keep], [ref_ids[t] for t in keep]
    T, cap = len(Ks), max(Ks)
    roots = torch.from_numpy(st_h).to(dev)
    feat, W, bias = _head_inputs(eng, T, F, pad, seed=100000 * preset[0] + 10 * F + pad)
    assert feat.stride(0) == F + pad
    if spike:  # every tree's last legal id 100 above the rest: a max that forgot the tail overflows the sum
        bias[torch.from_numpy(np.array([i[-1] for i in ref_ids])).to(dev)] += 100.0
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    vals = torch.rand((T, eng.P), generator=g, device=dev) * 2.0 - 1.0
    runs = [_run_sparse(eng, roots, T, 4 * 6144, cap, feat, W, bias, vals, form) for form in FORMS]
    for form, run in zip(FORMS[1:], runs[1:]):
        # the fused step under BK_STEP_OVERLAP 0 / 1 and BK_LEAF_SKIP0 0 / 1: the stagewise trees, bitwise
        assert _same(run[0], runs[0][0]) and _same(run[1], runs[0][1]), form
    (ids, n, q, p, counts), ctr = runs[0][0]
    assert ctr["expanded"] == T and ctr["errors"] == 0 and counts.tolist() == Ks
    gamma = (_dot_depth(F) + 1) * U
    worst = 0.0
    for t, K in enumerate(Ks):
        assert (ids[t, :K] == ref_ids[t]).all()
        idt = torch.from_numpy(ref_ids[t]).to(dev)
        prod = W[idt].double() * feat[t].double()
        b = bias[idt].double()
        logits = (prod.sum(1) + b).cpu().numpy()
        mag = float((prod.abs().sum(1) + b.abs()).max())
        if t == 0:
            assert mag == float(b.abs().max())  # the all-zero feature row: softmax(bias)
        worst = max(worst, check_priors(p[t, :K], logits, logit_err=0.0 if t == 0 else gamma * mag))
    print(f"sparse head {preset} F {F} ldf {F + pad}{' spike' if spike else ''} (depth {_dot_depth(F)}): largest error / bound = {worst:.4f}")


@pytest.mark.parametrize("F,spike", [(800, False), (64, False), (64, True)])
def test_sparse_head_priors_match_fp64_over_k(F, spike):
    """Every fixture K <= 2048 on 2-player 20x20 at the two feature lengths the nets use; once more
    with the largest logit at each tree's last child (2c's third pattern, through the bias)."""
    _sparse_case((20, 2, 5), F, 0, spike)


@pytest.mark.parametrize("F,pad", [(1, 0), (3, 0), (4, 0), (8, 0), (64, 0), (98, 0), (98, 3), (260, 0), (392, 0),
                                   (392, 3), (800, 0), (1024, 0), (1028, 0), (2048, 0)])
@pytest.mark.parametrize("preset", [(7, 2, 5), (14, 2, 5)], ids=lambda p: "x".join(map(str, p)))
def test_sparse_head_priors_match_fp64_over_f(preset, F, pad):
    """The feature lengths at which leaf_logits_dots and row_dot16 change path: the scalar branch
    (F % 4 != 0: 1, 3, 98 — 7x7's own F); fewer float4s than lanes (4, 8); F4 = 65 and 98, where only
    lane 0 / lanes 0-1 of the 16 have a remainder float4 after their whole trip; F > 960, where the
    fused step's prologue loops over the features; kMaxFeat; and a leading dimension F + 3."""
    _sparse_case(preset, F, pad)


# --------------------------------------------------------------- 2e: a leaf over the sparse cap
@pytest.mark.parametrize("preset,K_over", [((20, 2, 5), 2049), ((20, 2, 5), 5056), ((14, 2, 5), 2374)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"K{v}")
def test_sparse_head_over_the_leaf_cap(preset, K_over):
    """A root with more than kLeafCap = 2048 legal moves in prior mode 2, stagewise and in the fused
    step with overlap 0 and 1: kErrLeafCap is flagged and check() raises, no node is made for that
    tree (expanded = T - 1, its root stays missing), no wave waits for a flag nobody sets (DESIGN §2
    traces the waits), and every other tree is bitwise the tree of a batch without it — after the
    roots' expansion and after three more simulations, in which that tree comes back to the same
    over-cap leaf every time."""
    from blokus_rl_amd.engine import EngineError

    eng = _engine(preset)
    dev = eng.device
    Ks, st_h, _ = _fixture(preset)
    under = [t for t, K in enumerate(Ks) if K <= LEAF_CAP][-3:]
    order = [under[0], Ks.index(K_over)] + under[1:]  # the over-cap tree between the others
    T, F, cap = len(order), 64, LEAF_CAP
    others = [i for i in range(T) if i != 1]
    roots = torch.from_numpy(st_h[order]).to(dev)
    feat, W, bias = _head_inputs(eng, T, F, 0, seed=K_over)
    feat = feat.contiguous()
    feat[0] = feat[1]  # _head_inputs zeroes tree 0's row: give it features
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    vals = torch.rand((T, eng.P), generator=g, device=dev) * 2.0 - 1.0
    rows = torch.ones(T, dtype=torch.int32, device=dev)
    rows[1] = 0

    def probe(m):
        c = m.counters()
        assert c["expanded"] == T - 1 and c["errors"] == 32, c  # kErrLeafCap alone
        with pytest.raises(EngineError):
            m.check()
        counts = m.root_stats(roots, None, cap=cap)[4]
        assert counts.cpu().numpy().tolist() == [Ks[order[0]], -1] + [Ks[t] for t in order[2:]]

    for form in ["stages", (0, 1), (1, 1)]:
        got = _run_sparse(eng, roots, T, 4 * 6144, cap, feat, W, bias, vals, form, rows=rows, probe=probe)
        want = _run_sparse(eng, roots[others].contiguous(), T - 1, 4 * 6144, cap, feat[others].contiguous(), W, bias,
                           vals[others].contiguous(), form)
        assert want[0][1]["errors"] == 0 and want[0][1]["expanded"] == T - 1
        for (rows_got, _), (rows_want, _) in zip(got, want):
            for x, y in zip(rows_got, rows_want):
                assert x[others].tobytes() == y.tobytes(), form
