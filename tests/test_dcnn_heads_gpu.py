"""bk_dcnn_heads (nets.DCNNHeads / nets.dcnn_heads): DCNNet's crop, fc1, ReLU, fc2, ReLU, fc4 and
tanh from the fourth convolution's full-frame NHWC output.

Accuracy: the project's fp32-class bar (tests/test_dcnn_leaf_gpu.py): against the same computation
in fp64 on the CPU, the kernel's error is within 4x that of PyTorch's fp32 on the same device, or
2e-6 (features relative to the largest reference magnitude, v absolute)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(7, 2, 5), (7, 2, 17), (14, 2, 3), (20, 4, 2)]


def _dcnn(N, P, A, seed=0):
    from blokus_rl_amd.nets import DCNNet

    torch.manual_seed(seed)
    m = DCNNet(N, P, A, num_channels=128).cuda().eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
    return m


def _heads_torch(f, x, dtype, device):
    """crop, fc1, ReLU, fc2, ReLU, fc4, tanh from the FoldedDCNN's tensors in `dtype` on `device`."""
    c = lambda t: t.detach().to(device=device, dtype=dtype)  # noqa: E731
    N = f.N
    h = c(x)[:, 2:N - 2, 2:N - 2, :].reshape(x.shape[0], -1)
    h = torch.relu(torch.nn.functional.linear(h, c(f.fc1_w), c(f.fc1_b)))
    h = torch.relu(torch.nn.functional.linear(h, c(f.fc2_w), c(f.fc2_b)))
    return h, torch.tanh(torch.nn.functional.linear(h, c(f.fc4_w), c(f.fc4_b)))


@functools.lru_cache(maxsize=None)
def _case(N, P, B):
    """(folded net, heads, activation, fp64 reference) of a case, computed once and left unchanged."""
    from blokus_rl_amd.nets import DCNNHeads, fold_dcnn

    f = fold_dcnn(_dcnn(N, P, 257, seed=N + P))
    g = torch.Generator(device="cuda").manual_seed(5 * N + B)
    x = torch.relu(torch.randn((B, N, N, 128), device="cuda", generator=g)).contiguous()  # as after a ReLU
    return f, DCNNHeads(f), x, _heads_torch(f, x, torch.float64, "cpu")


@pytest.mark.parametrize("N,P,B", CASES)
def test_heads_are_fp32_class(N, P, B):
    from blokus_rl_amd.engine import load_library
    from blokus_rl_amd.nets import dcnn_heads

    f, heads, x, (f_ref, v_ref) = _case(N, P, B)
    assert heads.slices == load_library().bk_dcnn_heads_slices(N) > 0
    feats, v = dcnn_heads(x, heads)
    f32, v32 = _heads_torch(f, x, torch.float32, "cuda")
    torch.cuda.synchronize()
    assert tuple(feats.shape) == (B, 64) and tuple(v.shape) == (B, P)
    assert torch.isfinite(feats).all() and torch.isfinite(v).all() and float(feats.max()) > 0
    scale = float(f_ref.abs().max()) + 1e-30
    for what, e_k, e_32 in (("features", float((feats.double().cpu() - f_ref).abs().max()) / scale,
                             float((f32.double().cpu() - f_ref).abs().max()) / scale),
                            ("v", float((v.double().cpu() - v_ref).abs().max()),
                             float((v32.double().cpu() - v_ref).abs().max()))):
        print(f"N={N} P={P} B={B} {what}: heads {e_k:.3g}  fp32 {e_32:.3g}")
        assert e_k <= max(4 * e_32, 2e-6), (what, e_k, e_32)
    # the same call again on the same workspace
    again = dcnn_heads(x, heads)
    assert torch.equal(again[0], feats) and torch.equal(again[1], v)


@pytest.mark.parametrize("N,P,B", CASES)
def test_only_the_interior_is_read(N, P, B):
    from blokus_rl_amd.nets import dcnn_heads

    _, heads, x, _ = _case(N, P, B)
    feats, v = dcnn_heads(x, heads)
    ring = x.clone()
    ring[:, :2], ring[:, N - 2:], ring[:, :, :2], ring[:, :, N - 2:] = (float("nan"),) * 4
    assert torch.isnan(ring).sum() == B * (N * N - (N - 4) ** 2) * 128
    f2, v2 = dcnn_heads(ring, heads)
    assert torch.equal(f2, feats) and torch.equal(v2, v)


@pytest.mark.parametrize("N,P,B", CASES)
def test_a_board_does_not_depend_on_its_batch(N, P, B):
    from blokus_rl_amd.nets import dcnn_heads

    _, heads, x, _ = _case(N, P, B)
    feats, v = dcnn_heads(x, heads)
    for i in sorted({0, B // 2, B - 1}):  # a board of the first 16-row tile and one of the last
        fa, va = dcnn_heads(x[i:i + 1].contiguous(), heads)
        assert torch.equal(fa[0], feats[i]) and torch.equal(va[0], v[i]), i
    # at another place in another batch
    perm = torch.arange(B - 1, -1, -1, device="cuda")
    fp, vp = dcnn_heads(x[perm].contiguous(), heads)
    assert torch.equal(fp, feats[perm]) and torch.equal(vp, v[perm])


@pytest.mark.parametrize("N,P,B", [(7, 2, 17), (14, 2, 3)])
def test_more_boards_than_one_workgroup_tile(N, P, B):
    """70 boards: more than one workgroup tile (16 boards at 7x7, 64 otherwise), so full tiles (the
    loop without the per-block tests) and a last tile with a single live 16-board block; every
    board equals its value in the small batch."""
    from blokus_rl_amd.nets import dcnn_heads

    _, heads, x, _ = _case(N, P, B)
    idx = torch.arange(70, device="cuda") % B
    feats, v = dcnn_heads(x, heads)
    fb, vb = dcnn_heads(x[idx].contiguous(), heads)
    assert torch.equal(fb, feats[idx]) and torch.equal(vb, v[idx])
    f0, v0 = dcnn_heads(x[:0].contiguous(), heads)
    assert tuple(f0.shape) == (0, 64) and tuple(v0.shape) == (0, P)
