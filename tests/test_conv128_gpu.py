"""bk_conv128_x3 / bk_conv128_first (csrc/conv128.hip, nets.conv128_x3 / conv128_first): DCNNet's
128-channel 3x3 pad-1 convolutions at 14x14 and 20x20 on split-f16 MFMA products (N = 7: the
dispatch to bk_conv7), and the first layer on the planar observation in fp32.

References are fp64 torch on the CPU. The bar is tests/test_ppo_conv_gpu.py's fp32-class one:
elementwise err <= 1e-5 * bound, bound = the same expression on absolute values (the scale of
the sum; fp32's own rounding is ~1e-7 of it). The first layer sums at most 72 products in fp32
(error <= 73 * 2^-24 * bound = 4.4e-6 * bound at worst), so the same bar holds for it."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C = 128
SCALES = [1.0, 1e-6, 1e3, 0.0, 3.7]


@functools.lru_cache(maxsize=None)
def _wb():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    return w.float().double(), b.float().double()  # exact in f32


@functools.lru_cache(maxsize=None)
def _packed():
    from blokus_rl_amd.nets import conv128_pack

    w, b = _wb()
    ws, inv = conv128_pack(w.float().cuda())
    return ws, inv, b.float().cuda()


def _x(N, B, seed, scale=1.0):
    """NCHW fp64 boards; the boards of one batch cycle through the scales 1, 1e-6, 1e3, 0, 3.7 (a
    1e3 board beside a 1e-6 one across the shared halo row of a two-board tile); zero rows inside
    board 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, N, N, generator=g, dtype=torch.float64) * scale
    x = x * torch.tensor([SCALES[b % 5] for b in range(B)], dtype=torch.float64).view(B, 1, 1, 1)
    x[0, :, 2:4, :] = 0.0
    return x.float().double()


def _nhwc(x):
    return x.float().permute(0, 2, 3, 1).contiguous().cuda()


def _bound(x, w, b):
    return F.conv2d(x.abs(), w.abs(), padding=1) + b.abs().view(1, -1, 1, 1)


def _assert_close(got_nhwc, ref, bound, what):
    err = (got_nhwc.double().cpu().permute(0, 3, 1, 2) - ref).abs()
    ratio = float((err / (bound + 1e-300)).max())
    print(f"{what}: max err / bound = {ratio:.3e}")
    assert bool((err <= 1e-5 * bound + 1e-30).all()), f"{what}: max err / bound {ratio:.3e}"


@functools.lru_cache(maxsize=None)
def _case(N, B, scale):
    w, b = _wb()
    x = _x(N, B, 100 * N + B, scale)
    return x, F.conv2d(x, w, b, padding=1), _bound(x, w, b)


# (N, B, input scale): a partial two-board tile at 14x14, one and two tiles at 20x20, the dispatch
# to bk_conv7 at 7x7 (one full tile of 8 boards and a partial one), tiny and huge inputs
@pytest.mark.parametrize("N,B,scale", [(14, 1, 1.0), (14, 3, 1.0), (20, 1, 1.0), (20, 2, 1.0), (7, 9, 1.0),
                                       (14, 3, 1e-3), (20, 2, 1e3)])
def test_conv128_x3_is_fp32_class(N, B, scale):
    from blokus_rl_amd.engine import load_library
    from blokus_rl_amd.nets import conv128_x3

    lib = load_library()
    assert lib.bk_conv128_x3_supported(N) == 1 and lib.bk_conv128_x3_tile_boards(N) == {7: 8, 14: 2, 20: 1}[N]
    x, ref, bound = _case(N, B, scale)
    ws, inv, bd = _packed()
    xd = _nhwc(x)
    y = conv128_x3(xd, ws, inv, bd)
    assert tuple(y.shape) == (B, N, N, C) and y.is_contiguous()
    _assert_close(y, ref, bound, f"N={N} B={B} scale={scale}")
    for bz in range(3, B, 5):  # an all-zero board returns the bias exactly
        assert torch.equal(y[bz], bd.view(1, 1, C).expand(N, N, C)), bz
    assert torch.equal(conv128_x3(xd, ws, inv, bd), y)
    # the fused ReLU, and the result written into a given buffer
    out = torch.full_like(y, float("nan"))
    assert conv128_x3(xd, ws, inv, bd, relu=True, out=out) is out and torch.equal(out, torch.relu(y))
    # without a bias
    y0 = conv128_x3(xd, ws, inv, None)
    bias = _wb()[1].view(1, -1, 1, 1)
    _assert_close(y0, ref - bias, bound - bias.abs(), f"N={N} B={B} no bias")


@pytest.mark.parametrize("N", [14, 20, 7])
def test_a_board_does_not_depend_on_its_batch(N):
    """Every board has its own scale and its own zero halo: the same board alone and at every
    position of a batch (among boards of other magnitudes) gives bitwise equal outputs."""
    from blokus_rl_amd.engine import load_library
    from blokus_rl_amd.nets import conv128_x3

    T = load_library().bk_conv128_x3_tile_boards(N)
    B = 2 * T + 1 if N != 7 else T + 2
    ws, inv, bd = _packed()
    x = _nhwc(_x(N, B, 7 * N))
    probe = _nhwc(_x(N, 2, 11 * N))[1:2]  # a scale-1e-6 board
    alone = conv128_x3(probe.contiguous(), ws, inv, bd)
    assert float(alone.abs().max()) > 0
    for pos in range(B):
        xb = x.clone()
        xb[pos] = probe[0]
        y = conv128_x3(xb, ws, inv, bd)
        assert torch.equal(y[pos], alone[0]), pos


@pytest.mark.parametrize("N", [14, 20])
def test_zero_input_gives_the_bias(N):
    from blokus_rl_amd.nets import conv128_x3

    ws, inv, bd = _packed()
    y = conv128_x3(torch.zeros((3, N, N, C), device="cuda"), ws, inv, bd)
    assert torch.equal(y, bd.view(1, 1, 1, C).expand(3, N, N, C))


@pytest.mark.parametrize("N,cin", [(7, 4), (7, 8), (20, 4), (20, 8), (14, 6)])
def test_first_layer_against_fp64(N, cin):
    from blokus_rl_amd.nets import conv128_first

    g = torch.Generator().manual_seed(N + cin)
    w = (torch.randn(C, cin, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * cin)) ** 0.5).float()
    b = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).float()
    B = 3
    x = (torch.rand((B, cin, N, N), generator=g) < 0.3).float()
    x[1] = torch.randn((cin, N, N), generator=g)  # a dense board between two binary ones
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    bound = F.conv2d(x.double().abs(), w.double().abs(), padding=1) + b.double().abs().view(1, -1, 1, 1)
    y = conv128_first(x.cuda(), w.cuda(), b.cuda())
    assert tuple(y.shape) == (B, N, N, C)
    _assert_close(y, ref, bound, f"first N={N} cin={cin}")
    assert torch.equal(conv128_first(x.cuda(), w.cuda().reshape(C, -1), b.cuda(), relu=True), torch.relu(y))
    y0 = conv128_first(x.cuda(), w.cuda(), None)
    bias = b.double().view(1, -1, 1, 1)
    _assert_close(y0, ref - bias, bound - bias.abs(), f"first N={N} cin={cin} no bias")


def test_empty_batch_and_bad_arguments():
    from blokus_rl_amd.engine import EngineError, load_library
    from blokus_rl_amd.nets import conv128_first, conv128_x3

    lib = load_library()
    ws, inv, bd = _packed()
    for N in (7, 14, 20):
        y = conv128_x3(torch.empty((0, N, N, C), device="cuda"), ws, inv, bd)
        assert tuple(y.shape) == (0, N, N, C)
        y = conv128_first(torch.empty((0, 4, N, N), device="cuda"), torch.zeros((C, 36), device="cuda"), bd)
        assert tuple(y.shape) == (0, N, N, C)
    assert lib.bk_conv128_x3_supported(9) == 0 and lib.bk_conv128_x3_tile_boards(9) == 0
    with pytest.raises(EngineError):
        conv128_x3(torch.zeros((1, 9, 9, C), device="cuda"), ws, inv, bd)
    with pytest.raises(EngineError):
        conv128_first(torch.zeros((1, 2, 7, 7), device="cuda"), torch.zeros((C, 18), device="cuda"), bd)
    torch.cuda.synchronize()
