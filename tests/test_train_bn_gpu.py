"""The learner's batch norm (csrc/trainbn.hip) called directly (train_conv.bn_forward /
bn_backward) on [M, 64, 1, 1] activations, so that M is free, against fp64 torch on the CPU on
the same f32-rounded inputs.

* M = 1, 15, 16, 17 (k_bn_reduce's 16-row pass), 8192 / 8193 (its first grid-stride trip: 512
  workgroups x 16 rows), 32768 / 32769 and 100001 (k_bn_axpb's first and later grid-stride
  trips: 2048 workgroups x 256 float4), with and without the fused ReLU, on inputs 5 + 3 randn,
  randn and the ill-conditioned 100 + 0.1 randn (mean / std = 1e3: an fp32 accumulation of the
  statistics misses the bars there by orders of magnitude).
* Forward: the statistics within one or two f32 roundings of the two-pass fp64 ones, y bitwise
  (x * scale) + shift from the kernel's own f32 statistics, the running statistics.
* Backward: the fp64 formula with the given f32 statistics taken exactly, under the forward's own
  statistics and under made-up ones (mean + std, 0.8 invstd), where the column sums of dx (the conv
  bias gradient, analytically zero under true batch statistics) are far from zero.
* The ReLU mask the backward recomputes is the mask the forward applied (dbeta of dy = 1 is the
  count of positive outputs, exactly).
* ConvBNFunction at 20x20 with B = 83 (M = 33200 > 32768 rows): the autograd wiring of the conv
  bias gradient on the multi-trip path.

Every check prints its largest error / bound ratio (pytest -s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # the eps the kernel receives (a C float)
MOM = 0.1
R_MEAN0, R_VAR0 = 0.25, 1.5
REGIMES = {"5+3n": (5.0, 3.0), "n": (0.0, 1.0), "100+0.1n": (100.0, 0.1)}
WELL = ("5+3n", "n")
# the small M in every regime; each large M in one or two, every regime meeting every code path
CASES = [(M, r) for M in (1, 15, 16, 17) for r in REGIMES] + [
    (8192, "5+3n"), (8193, "n"), (8193, "100+0.1n"), (32768, "100+0.1n"), (32769, "5+3n"), (32769, "n"),
    (100001, "n"), (100001, "100+0.1n")]
IDS = [f"M{M}-{r}" for M, r in CASES]


def _dev(t):
    return t.cuda()


def _ratio(err, bound):
    """Largest err / bound (0 / 0 counts as 0; an error against a zero bound as huge)."""
    return float((err / bound.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=2)
def _inputs(M, regime):
    mu, sd = REGIMES[regime]
    g = torch.Generator().manual_seed(7919 * list(REGIMES).index(regime) + M)
    x = (mu + sd * torch.randn(M, 64, generator=g, dtype=torch.float64)).float()
    gamma = (0.5 + torch.rand(64, generator=g, dtype=torch.float64)).float()
    beta = (0.2 * torch.randn(64, generator=g, dtype=torch.float64)).float()
    xd = x.double()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)  # two-pass
    inv = 1.0 / (var + EPS32).sqrt()
    # dy correlated with x and of non-zero mean: neither backward sum cancels
    dy = (0.3 + torch.randn(M, 64, generator=g, dtype=torch.float64) + 0.5 * (xd - mean) * inv).float()
    return x, gamma, beta, dy, mean, var, inv


def _forward(x, gamma, beta, relu):
    from blokus_rl_amd.alphazero.train_conv import bn_forward

    M = x.shape[0]
    rm, rv = _dev(torch.full((64,), R_MEAN0)), _dev(torch.full((64,), R_VAR0))
    y, stats = bn_forward(_dev(x).view(M, 64, 1, 1), _dev(gamma), _dev(beta), rm, rv, MOM, EPS, relu)
    return y.cpu().reshape(M, 64), stats.cpu(), rm.cpu(), rv.cpu()


def _backward(dy, x, gamma, stats, relu):
    from blokus_rl_amd.alphazero.train_conv import bn_backward

    M = x.shape[0]
    dx, dg, db, ds = bn_backward(_dev(dy).view(M, 64, 1, 1), _dev(x).view(M, 64, 1, 1), _dev(gamma), _dev(stats),
                                 relu, True)
    return dx.cpu().reshape(M, 64), dg.cpu(), db.cpu(), ds.cpu()


def _affine32(x, stats, relu):
    """(x * scale) + shift as two float32 ops from f32 statistics (the library is built with
    -ffp-contract=off: the kernel's value bit for bit), and max(., 0) under relu."""
    z = x * stats[128:192]
    z = z + stats[192:256]
    return torch.where(z > 0, z, torch.zeros_like(z)) if relu else z


@pytest.mark.parametrize("M,regime", CASES, ids=IDS)
def test_bn_forward_matches_fp64(M, regime):
    x, gamma, beta, _, mean, var, inv = _inputs(M, regime)
    g, b = gamma.double(), beta.double()
    for relu in (False, True):
        y, stats, rm, rv = _forward(x, gamma, beta, relu)
        st = stats.double()
        r = {
            "mean": _ratio((st[:64] - mean).abs(), 2.0 ** -23 * x.double().abs().mean(0)),
            "inv": _ratio((st[64:128] - inv).abs(), 2.0 ** -22 * inv),
            "scale": _ratio((st[128:192] - g * inv).abs(), 2.0 ** -22 * (g * inv).abs()),
            "shift": _ratio((st[192:] - (b - mean * g * inv)).abs(), 2.0 ** -22 * (b.abs() + (mean * g * inv).abs())),
        }
        unb = var * M / (M - 1) if M > 1 else var
        for name, got, r0, v in (("rmean", rm, R_MEAN0, mean), ("rvar", rv, R_VAR0, unb)):
            ref = (1 - MOM) * r0 + MOM * v
            r[name] = _ratio((got.double() - ref).abs(), 2.0 ** -21 * (abs((1 - MOM) * r0) + (MOM * v).abs()))
        print(f"bn fwd M={M} {regime} relu={int(relu)}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
        for k, v in r.items():
            assert v <= 1.0, (k, v, relu)
        exp = _affine32(x, stats, relu)
        assert torch.equal(y.view(torch.int32), exp.view(torch.int32)), f"relu={relu}: y is not (x*scale)+shift bitwise"


def _backward_ref(x, dy, gamma, stats, relu):
    """The fp64 batch-norm backward with the f32 statistics taken exactly."""
    M = x.shape[0]
    mask = (_affine32(x, stats, False) > 0).double() if relu else torch.ones(x.shape, dtype=torch.float64)
    xd, g = x.double(), gamma.double()
    mean, inv = stats[:64].double(), stats[64:128].double()
    dym = dy.double() * mask
    sd = dym.sum(0)
    sdx = (dym * (xd - mean)).sum(0)
    k1 = g * inv
    k3 = -g * inv ** 3 * sdx / M
    k2 = -g * inv * sd / M - k3 * mean
    dx = k1 * dym + k3 * xd + k2
    s_e = (k1 * dym).abs() + k3.abs() * (xd.abs() + mean.abs()) + (g * inv * sd / M).abs()
    return {"dx": dx, "dgamma": sdx * inv, "dbeta": sd, "dsum": dx.sum(0), "s_e": s_e,
            "b_dgamma": inv * (dym * (xd - mean)).abs().sum(0), "b_dbeta": dym.abs().sum(0)}


def _made_up_stats(gamma, beta, mean, inv):
    """Statistics that are not the batch's: mean + std, 0.8 invstd, and the scale / shift that go
    with them, rounded to f32. dsum = k3 M (mean - mean') is then far from zero."""
    mean2 = mean + 1.0 / inv
    inv2 = 0.8 * inv
    scale2 = gamma.double() * inv2
    shift2 = beta.double() - mean2 * scale2
    return torch.cat([mean2, inv2, scale2, shift2]).float()


@pytest.mark.parametrize("M,regime", CASES, ids=IDS)
def test_bn_backward_matches_fp64(M, regime):
    x, gamma, beta, dy, mean, _, inv = _inputs(M, regime)
    for relu in (False, True):
        own = _forward(x, gamma, beta, relu)[1]
        for kind, stats in (("own", own), ("made-up", _made_up_stats(gamma, beta, mean, inv))):
            ref = _backward_ref(x, dy, gamma, stats, relu)
            sum_se = ref["s_e"].sum(0)
            if kind == "made-up" and M >= 8192 and regime in WELL:
                # the bias sums are 1000 bars away from zero: a wrong sum cannot hide
                assert bool((ref["dsum"].abs() >= 1e-3 * sum_se).all()), float((ref["dsum"].abs() / sum_se).min())
            dx, dg, db, ds = _backward(dy, x, gamma, stats, relu)
            colsum = dx.double().sum(0)
            r = {
                "dx": _ratio((dx.double() - ref["dx"]).abs(), 1e-6 * ref["s_e"]),
                "dgamma": _ratio((dg.double() - ref["dgamma"]).abs(), 5e-7 * ref["b_dgamma"]),
                "dbeta": _ratio((db.double() - ref["dbeta"]).abs(), 2.0 ** -22 * ref["b_dbeta"]),
                "dsum": _ratio((ds.double() - ref["dsum"]).abs(), 1e-6 * sum_se),
                # the kernel adds exactly the dx it stored, in fp64
                "dsum/stored": _ratio((ds.double() - colsum).abs(),
                                      2.0 ** -23 * colsum.abs() + 1e-12 * dx.double().abs().sum(0)),
            }
            print(f"bn bwd M={M} {regime} relu={int(relu)} {kind}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
            for k, v in r.items():
                assert v <= 1.0, (k, v, relu, kind)


def test_bn_backward_mask_is_the_forwards():
    """dy = 1 under relu with the forward's own statistics: dbeta[c] is the number of rows the
    forward left positive in channel c, exactly (integers below 2^24 in fp64 sums and one f32)."""
    M = 32769
    x, gamma, beta, *_ = _inputs(M, "5+3n")
    y, stats, _, _ = _forward(x, gamma, beta, True)
    _, _, db, _ = _backward(torch.ones(M, 64), x, gamma, stats, True)
    count = (y > 0).sum(0)
    assert 0 < int(count.min()) and int(count.max()) < M  # both sides of the mask in every channel
    assert torch.equal(db.double(), count.double()), (db - count).abs().max()


def test_conv_bn_function_multi_trip_matches_fp64():
    """ConvBNFunction at 20x20 with B = 83 (33200 rows: k_bn_axpb's second grid-stride trip and
    the column sums over it) against the fp64 conv -> batch norm -> ReLU, at the bars of
    test_fused_conv_bn_relu_matches_fp64."""
    from blokus_rl_amd.alphazero.train_conv import ConvBNFunction

    B, relu = 83, True
    g = torch.Generator().manual_seed(19)
    x = torch.randn(B, 64, 20, 20, generator=g, dtype=torch.float64)
    w = torch.randn(64, 64, 3, 3, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(64, generator=g, dtype=torch.float64) * 0.1
    gam = torch.rand(64, generator=g, dtype=torch.float64) + 0.5
    bet = torch.randn(64, generator=g, dtype=torch.float64) * 0.2
    gy = torch.randn(B, 64, 20, 20, generator=g, dtype=torch.float64)
    xr, wr, br, gr, btr = (t.clone().requires_grad_() for t in (x, w, b, gam, bet))
    z = F.conv2d(xr, wr, br, padding=1)
    pre = F.batch_norm(z, torch.zeros(64, dtype=torch.float64), torch.ones(64, dtype=torch.float64), gr, btr,
                       training=True, momentum=0.1, eps=1e-5)
    yr = F.relu(pre)
    # 2.1M pre-activations come within 1e-7 of zero, where the f32 path's rounding decides the ReLU's
    # mask and one flipped element moves every max-norm figure below by far more than its bar. No
    # upstream gradient there (|pre| < 1e-4, above y's bar of ~3e-5; ~200 elements): the mask at the
    # boundary itself is pinned bitwise by test_bn_backward_mask_is_the_forwards.
    edge = pre.detach().abs() < 1e-4
    assert 0 < int(edge.sum()) < 1000
    gy[edge] = 0.0
    yr.backward(gy)
    xd = _dev(x.float()).contiguous(memory_format=torch.channels_last).requires_grad_()
    wd, bd, gd, btd = (_dev(t.float()).requires_grad_() for t in (w, b, gam, bet))
    rm, rv = _dev(torch.zeros(64)), _dev(torch.ones(64))
    y = ConvBNFunction.apply(xd, wd, bd, gd, btd, rm, rv, 0.1, 1e-5, relu)
    y.backward(_dev(gy.float()).contiguous(memory_format=torch.channels_last))
    scale = lambda t: float(t.abs().max())  # noqa: E731
    r = {"y": float((y.detach().double().cpu() - yr.detach()).abs().max()) / (5e-6 * scale(yr.detach()))}
    for name, a, ref in (("dx", xd.grad, xr.grad), ("dW", wd.grad, wr.grad), ("dgamma", gd.grad, gr.grad),
                         ("dbeta", btd.grad, btr.grad)):
        r[name] = float((a.double().cpu() - ref).abs().max()) / (2e-5 * scale(ref))
    r["dcb"] = float(bd.grad.abs().max()) / (1e-6 * float(gy.abs().sum(dim=(0, 2, 3)).max()))
    r["rmean"] = float((rm.double().cpu() - 0.1 * z.detach().mean(dim=(0, 2, 3))).abs().max()) / (
        1e-6 * float(z.detach().abs().max()))
    print("conv-bn B=83: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= 1.0, (k, v)
