"""The learner's sparse policy Linear (csrc/trainfc.hip, train_conv.SparsePolicyLinear) at its edge
shapes, against the dense fp64 Linear followed by the gather at the rows' legal ids, on the same
f32-rounded inputs.

* Widths F = 4 (one lane, one float4 slot), 8, 392 and 1024 (all four slots of every lane: the
  `f < F4` guard at full width); B = 1, 31, 32, 33 (k_splin_dw's bitmap around a word) and 4096
  (the whole bitmap, all four wave quarters, every id held by thousands of rows).
* Rows of K = 0, 1..9 (the pair and the tail of the `j += 8` loops), cap, k = cap + 7 (read as
  cap) and k = -3 (read as 0: the whole xs row zero). ids are distinct within a row; the ids and
  the upstream gradient past a row's K are live values the kernels must not read.
* Element-wise bars, 1e-5 of the sum of the magnitudes that enter each element (fp32's own
  rounding is ~1e-7 of it); dW and db exactly zero at ids no row holds; two runs bitwise equal.
* The refusals (more than 4096 rows in the weight gradient, F not a multiple of 4, F > 1024) raise
  EngineError and write nothing.

Every check prints its largest error / bound ratio (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# B, F, A, cap
SHAPES = [(1, 4, 5, 64), (31, 392, 700, 64), (32, 392, 700, 64), (33, 392, 700, 64), (37, 1024, 300, 128),
          (4096, 8, 64, 64)]


def _dev(t):
    return t.cuda()


def _ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


def _k_rows(B, cap, g):
    """Raw k per row (before the kernels' clamp to [0, cap]): the edge rows first, random after."""
    k = torch.randint(0, cap + 1, (B,), generator=g)
    edge = list(range(10)) + [cap, cap + 7, -3]
    k[: len(edge)] = torch.tensor(edge)
    return k


def _case(B, F, A, cap, seed, k=None):
    g = torch.Generator().manual_seed(seed)
    pf = torch.relu(torch.randn(B, F, generator=g, dtype=torch.float64)).float().double()
    W = (torch.randn(A, F, generator=g, dtype=torch.float64) * 0.03).float().double()
    bias = (torch.randn(A, generator=g, dtype=torch.float64) * 0.1).float().double()
    k = _k_rows(B, cap, g) if k is None else torch.tensor(k)
    assert int(k.clamp(0, cap).max()) <= A  # distinct ids: a row holds at most A
    # every row filled with distinct ids as far as A allows (live ids past K), -1 after; where A
    # leaves room, a random eighth of the ids is in no row at all (zero rows of dW)
    n = min(cap, A)
    pool = torch.randperm(A, generator=g)
    if A - A // 8 >= n:
        pool = pool[: A - A // 8]
    ids = torch.full((B, cap), -1, dtype=torch.int16)
    ids[:, :n] = pool[torch.rand(B, len(pool), generator=g).argsort(1)[:, :n]].to(torch.int16)
    gy = torch.randn(B, cap, generator=g, dtype=torch.float64).float().double()  # live past K too
    return pf, W, bias, ids, k, gy


def _dense(pf, W, bias, ids, valid, gy):
    """The dense Linear + gather at the valid pairs and its gradients, in the inputs' precision."""
    pr, Wr, br = (t.clone().requires_grad_() for t in (pf, W, bias))
    gat = torch.gather(torch.nn.functional.linear(pr, Wr, br), 1, ids.long().clamp(min=0)) * valid
    gat.backward(gy)
    return gat.detach(), pr.grad, Wr.grad, br.grad


def _sparse(pf, W, bias, ids, k, gy):
    from blokus_rl_amd.alphazero.train_conv import SparsePolicyLinear

    pd, Wd, bd = (_dev(t.float()).requires_grad_() for t in (pf, W, bias))
    xs = SparsePolicyLinear.apply(pd, Wd, bd, _dev(ids), _dev(k.to(torch.int32)))
    xs.backward(_dev(gy.float()))
    return xs.detach().cpu(), pd.grad.cpu(), Wd.grad.cpu(), bd.grad.cpu()


def _check_case(tag, pf, W, bias, ids, k, gy):
    cap, A = ids.shape[1], W.shape[0]
    kc = k.clamp(0, cap)  # the kernels' fc_clamp_k
    valid = torch.arange(cap)[None, :] < kc[:, None]
    ref = _dense(pf, W, bias, ids, valid, gy)
    # the bounds: the same sums over magnitudes (xs: |pf|.|W[id]| + |bias|; dpf: sum_j |g||W|;
    # dW: sum_b |g||pf|; db: sum |g|)
    bound = _dense(pf.abs(), W.abs(), bias.abs(), ids, valid, gy.abs())
    outs = [_sparse(pf, W, bias, ids, k, gy) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "two runs differ"
    xs, dpf, dW, db = (t.double() for t in outs[0])
    assert bool((xs[~valid] == 0).all()), "xs past a row's K is not zero"
    r = {n: _ratio((a - e).abs(), 1e-5 * b) for n, a, e, b in zip(("xs", "dpf", "dW", "db"), (xs, dpf, dW, db), ref, bound)}
    print(f"splin {tag}: " + " ".join(f"{n} {v:.4f}" for n, v in r.items()))
    for n, v in r.items():
        assert v <= 1.0, (n, v)
    held = torch.zeros(A, dtype=torch.bool)
    held[ids[valid].long()] = True
    assert bool((dW[~held] == 0).all()) and bool((db[~held] == 0).all())
    return held


@pytest.mark.parametrize("B,F,A,cap", SHAPES, ids=[f"B{s[0]}-F{s[1]}-A{s[2]}-cap{s[3]}" for s in SHAPES])
def test_sparse_policy_linear_edge_shapes(B, F, A, cap):
    if B == 1:  # one row: each edge k that A = 5 distinct ids allow, in turn
        for k in (0, 1, 2, 5, -3):
            _check_case(f"B=1 F={F} k={k}", *_case(B, F, A, cap, 100 + k, k=[k]))
        return
    pf, W, bias, ids, k, gy = _case(B, F, A, cap, B + F)
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, cap, cap + 7, -3} <= set(k.tolist())
    held = _check_case(f"B={B} F={F} A={A} cap={cap}", pf, W, bias, ids, k, gy)
    if B == 4096:  # every id held by thousands of rows, in every quarter of the bitmap
        valid = torch.arange(cap)[None, :] < k.clamp(0, cap)[:, None]
        per_quarter = torch.stack([torch.bincount(ids[q * 1024:(q + 1) * 1024][valid[q * 1024:(q + 1) * 1024]].long(),
                                                  minlength=A) for q in range(4)])
        assert bool(held.all()) and int(per_quarter.min()) >= 256
    else:
        assert int((~held).sum()) > 0  # some ids no row holds: zero rows of dW


def test_sparse_policy_linear_refusals():
    """B > 4096 in the weight gradient, F % 4 != 0 and F > 1024 in the forward: EngineError, and the
    output buffers keep their contents (nothing was launched)."""
    from blokus_rl_amd.engine import EngineError, _check, _ptr, _stream, load_library

    lib = load_library()
    dev = torch.device("cuda")
    st = _stream(dev)
    A, cap = 64, 64
    for F in (6, 1028):
        B = 3
        pf, W, bias = torch.ones(B, F, device=dev), torch.ones(A, F, device=dev), torch.ones(A, device=dev)
        ids = torch.arange(cap, dtype=torch.int16, device=dev).expand(B, cap).contiguous()
        k = torch.full((B,), cap, dtype=torch.int32, device=dev)
        xs = torch.full((B, cap), 7.0, device=dev)
        with pytest.raises(EngineError):
            _check(lib.bk_sparse_linear_fwd(_ptr(pf), B, F, _ptr(W), _ptr(bias), A, _ptr(ids), _ptr(k), cap, _ptr(xs), st))
        torch.cuda.synchronize()
        assert bool((xs == 7.0).all())
    B, F = 4097, 8
    g, pf = torch.ones(B, cap, device=dev), torch.ones(B, F, device=dev)
    start = torch.zeros(A + 1, dtype=torch.int32, device=dev)  # no id held: a launch would write zeros
    pairs = torch.zeros(B * cap, dtype=torch.int32, device=dev)
    dW, db = torch.full((A, F), 7.0, device=dev), torch.full((A,), 7.0, device=dev)
    with pytest.raises(EngineError):
        _check(lib.bk_sparse_linear_dw(_ptr(g), _ptr(pf), B, F, cap, A, _ptr(start), _ptr(pairs), _ptr(dW), _ptr(db), st))
    torch.cuda.synchronize()
    assert bool((dW == 7.0).all()) and bool((db == 7.0).all())
    # and through autograd: the forward runs at 4097 rows, the backward refuses
    from blokus_rl_amd.alphazero.train_conv import SparsePolicyLinear

    pd, Wd, bd = (torch.ones(s, device=dev, requires_grad=True) for s in ((B, F), (A, F), (A,)))
    ids = torch.arange(cap, dtype=torch.int16, device=dev).expand(B, cap).contiguous()
    xs = SparsePolicyLinear.apply(pd, Wd, bd, ids, torch.full((B,), 3, dtype=torch.int32, device=dev))
    with pytest.raises(EngineError):
        xs.sum().backward()
    torch.cuda.synchronize()
