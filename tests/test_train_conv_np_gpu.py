"""The learner's device path on 7x7 and 14x14 boards (csrc/trainconv_np.hip, opt-in
x3_boards="all" / BK_X3_BOARDS=all): bk_conv_x3_np and bk_conv_x3_np_wgrad against fp64 at the
tolerances of tests/test_train_conv_gpu.py (elementwise 1e-5 of conv(|x|, |w|) + |b|, and no more
than 20x the fp32 convolution's own error), a board's output bitwise independent of its batch,
second trips of the persistent workgroups, the autograd functions, and the Learner on both boards
(dense head at 7x7, F = 98; sparse head at 14x14) and under the default knob."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SCALES = [1.0, 1e-6, 1e3, 0.0, 3.7]


def _lib():
    from blokus_rl_amd.engine import load_library

    return load_library()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _inputs(seed, N, B, device="cpu"):
    """x [B, 64, N, N] f64 with the board magnitudes of SCALES cycling and a zero row block inside
    board 0, w, b (f64)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, 64, N, N, generator=g, dtype=torch.float64, device=device)
    scales = torch.tensor([SCALES[i % 5] for i in range(B)], dtype=torch.float64, device=device).view(B, 1, 1, 1)
    x = x * scales
    x[0, :, 2:4, :] = 0.0  # zero rows inside a board
    w = torch.randn(64, 64, 3, 3, generator=g, dtype=torch.float64, device=device) * (2.0 / 576) ** 0.5
    b = torch.randn(64, generator=g, dtype=torch.float64, device=device) * 0.1
    return x, w, b


def _bound(x, w, b=None):
    y = F.conv2d(x.abs(), w.abs(), padding=1)
    return y + (b.abs().view(1, -1, 1, 1) if b is not None else 0)


def _forward_batch(N):
    from blokus_rl_amd.alphazero.train_conv import conv_x3_np, pack_weight

    T = _lib().bk_conv_x3_np_tile_boards(N)
    B = 2 * T + 3 if N == 7 else 5
    x, w, b = _inputs(2, N, B)
    xd = x.float().cuda().contiguous(memory_format=torch.channels_last)
    ws, inv = pack_weight(w.float().cuda(), False)
    bd = b.float().cuda()
    y = conv_x3_np(xd, ws, inv, bd)
    torch.cuda.synchronize()
    return {"T": T, "B": B, "x": x, "w": w, "b": b, "xd": xd, "ws": ws, "inv": inv, "bd": bd, "y": y}


@pytest.fixture(scope="module")
def batch7():
    return _forward_batch(7)


@pytest.fixture(scope="module")
def batch14():
    return _forward_batch(14)


def _check_forward(d, N):
    # the fp64 reference on the same f32-rounded inputs
    x, w, b = d["x"].float().double(), d["w"].float().double(), d["b"].float().double()
    ref = F.conv2d(x, w, b, padding=1)
    bound = _bound(x, w, b)
    y = d["y"]
    assert y.shape == (d["B"], 64, N, N) and y.is_contiguous(memory_format=torch.channels_last)
    err = (y.double().cpu() - ref).abs()
    r_x3 = float((err / (bound + 1e-30)).max())
    y32 = F.conv2d(d["xd"], d["w"].float().cuda(), d["bd"], padding=1).double().cpu()
    r_32 = float(((y32 - ref).abs() / (bound + 1e-30)).max())
    print(f"N={N} B={d['B']}: max err/bound x3 {r_x3:.3e}, fp32 conv {r_32:.3e}")
    assert bool((err <= 1e-5 * bound + 1e-30).all()), f"max err/bound {r_x3:.3e}"
    assert r_x3 <= max(20 * r_32, 1e-6), (r_x3, r_32)
    # the all-zero boards give the bias exactly
    for i in range(3, d["B"], 5):
        assert torch.equal(y[i].cpu(), d["b"].float().view(64, 1, 1).expand(64, N, N)), i


def test_forward_fp32_class_7(batch7):
    assert batch7["T"] >= 1 and batch7["B"] % batch7["T"] != 0  # the last tile is partial
    _check_forward(batch7, 7)


def test_forward_fp32_class_14(batch14):
    _check_forward(batch14, 14)


def test_board_alone_equals_its_batch_row(batch7):
    """A board's output is bitwise a function of that board and the weights: the first board of a
    tile, a middle one and the last board of the partial tile, each run alone; the batch reversed."""
    from blokus_rl_amd.alphazero.train_conv import conv_x3_np

    d, T, B = batch7, batch7["T"], batch7["B"]
    for i in (T, T + T // 2, B - 1):
        one = conv_x3_np(d["xd"][i:i + 1].contiguous(memory_format=torch.channels_last), d["ws"], d["inv"], d["bd"])
        assert torch.equal(one[0], d["y"][i]), i
    xr = d["xd"].flip(0).contiguous(memory_format=torch.channels_last)
    yr = conv_x3_np(xr, d["ws"], d["inv"], d["bd"])
    assert torch.equal(yr.flip(0), d["y"])


@pytest.mark.parametrize("N", [7, 14])
def test_forward_second_trip(N):
    """More tiles than workgroups: at least one workgroup walks two tiles and the last is partial."""
    from blokus_rl_amd.alphazero.train_conv import conv_x3_np, pack_weight

    T = _lib().bk_conv_x3_np_tile_boards(N)
    B = (_cus() + 1) * T + 3 if N == 7 else _cus() + 44
    x, w, b = _inputs(6, N, B, device="cuda")
    xd = x.float().contiguous(memory_format=torch.channels_last)
    ws, inv = pack_weight(w.float(), False)
    y = conv_x3_np(xd, ws, inv, b.float())
    x, w, b = xd.double(), w.float().double(), b.float().double()
    ref = F.conv2d(x, w, b, padding=1)
    bound = _bound(x, w, b)
    err = (y.double() - ref).abs()
    r_x3 = float((err / (bound + 1e-30)).max())
    r_32 = float(((F.conv2d(xd, w.float(), b.float(), padding=1).double() - ref).abs() / (bound + 1e-30)).max())
    print(f"N={N} B={B}: max err/bound x3 {r_x3:.3e}, fp32 conv {r_32:.3e}")
    assert bool((err <= 1e-5 * bound + 1e-30).all()), f"max err/bound {r_x3:.3e}"
    assert r_x3 <= max(20 * r_32, 1e-6), (r_x3, r_32)
    head = conv_x3_np(xd[:T].contiguous(memory_format=torch.channels_last), ws, inv, b.float())
    assert torch.equal(head, y[:T])


@pytest.mark.parametrize("N", [7, 14])
def test_gradients_through_x3conv2d(N):
    from blokus_rl_amd.alphazero.train_conv import X3Conv2d, train_entry

    assert train_entry(N, 64, "all") == "np" and train_entry(N, 64, "classic") is None
    B = _lib().bk_conv_x3_np_tile_boards(N) + 3
    x, w, b = _inputs(3, N, B)
    x, w, b = x.float().double(), w.float().double(), b.float().double()
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    gy[1] *= 1e-4
    gy = gy.float().double()
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    F.conv2d(xr, wr, br, padding=1).backward(gy)
    conv = torch.nn.Conv2d(64, 64, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(b.float())
    conv.__class__ = X3Conv2d
    conv.x3_boards = "all"
    xd = x.float().cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    y = conv(xd)
    assert y.grad_fn is not None and "ConvX3Function" in type(y.grad_fn).__name__
    y.backward(gy.float().cuda().contiguous(memory_format=torch.channels_last))
    gx_bound = _bound(gy, w.transpose(0, 1).flip(2, 3))
    err = (xd.grad.double().cpu() - xr.grad).abs()
    assert bool((err <= 1e-5 * gx_bound + 1e-30).all()), f"dx max err/bound {(err / (gx_bound + 1e-30)).max():.3e}"
    gw_bound = torch.nn.grad.conv2d_weight(x.abs(), w.shape, gy.abs(), padding=1)
    errw = (conv.weight.grad.double().cpu() - wr.grad).abs()
    assert bool((errw <= 1e-5 * gw_bound + 1e-30).all()), f"dw max err/bound {(errw / (gw_bound + 1e-30)).max():.3e}"
    gb_bound = gy.abs().sum(dim=(0, 2, 3))
    assert bool(((conv.bias.grad.double().cpu() - br.grad).abs() <= 1e-5 * gb_bound + 1e-30).all())
    # under "classic" the same module takes PyTorch's convolution
    conv.x3_boards = "classic"
    assert "ConvX3Function" not in type(conv(xd).grad_fn).__name__


@pytest.mark.parametrize("N", [7, 14])
def test_wgrad_fp32_class(N):
    """bk_conv_x3_np_wgrad with more trips than workgroups and a partial last trip, board magnitudes
    over 1e8 (the workgroup's operand scales drop and its sums are rescaled when a later trip holds
    larger values), all-zero boards; deterministic; one board; no board."""
    from blokus_rl_amd.alphazero.train_conv import conv_x3_np_wgrad

    Tw = _lib().bk_conv_x3_np_wgrad_tile_boards(N)
    B = (_cus() + 1) * Tw + (Tw - 1 if Tw > 1 else 43)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(B, 64, N, N, device="cuda", dtype=torch.float64, generator=g)
    gy = torch.randn(B, 64, N, N, device="cuda", dtype=torch.float64, generator=g)
    sx = torch.logspace(-4, 4, B, device="cuda", dtype=torch.float64)[torch.randperm(B, device="cuda", generator=g)]
    sy = torch.logspace(-4, 4, B, device="cuda", dtype=torch.float64)[torch.randperm(B, device="cuda", generator=g)]
    x *= sx.view(B, 1, 1, 1)
    gy *= sy.view(B, 1, 1, 1)
    x[5] = 0.0
    gy[17] = 0.0
    if N == 14:
        gy[B - 44, :, 7:, :] *= 1e6  # a large lower half after a small upper one
    x32 = x.float().contiguous(memory_format=torch.channels_last)
    gy32 = gy.float().contiguous(memory_format=torch.channels_last)
    dw = conv_x3_np_wgrad(x32, gy32).double()
    xr, gyr = x32.double(), gy32.double()  # the fp64 reference on the same (f32-rounded) inputs
    ref = torch.nn.grad.conv2d_weight(xr, (64, 64, 3, 3), gyr, padding=1)
    bound = torch.nn.grad.conv2d_weight(xr.abs(), (64, 64, 3, 3), gyr.abs(), padding=1)
    ratio = float(((dw - ref).abs() / (bound + 1e-30)).max())
    print(f"N={N} B={B}: wgrad max err / bound = {ratio:.3e}")
    assert ratio <= 1e-5
    assert torch.equal(conv_x3_np_wgrad(x32, gy32), conv_x3_np_wgrad(x32, gy32))
    one = conv_x3_np_wgrad(x32[:1], gy32[:1]).double()
    ref1 = torch.nn.grad.conv2d_weight(xr[:1], (64, 64, 3, 3), gyr[:1], padding=1)
    b1 = torch.nn.grad.conv2d_weight(xr[:1].abs(), (64, 64, 3, 3), gyr[:1].abs(), padding=1)
    assert bool(((one - ref1).abs() <= 1e-5 * b1 + 1e-30).all())
    assert torch.equal(conv_x3_np_wgrad(x32[:0], gy32[:0]), torch.zeros(64, 64, 3, 3, device="cuda"))


@pytest.mark.parametrize("N", [7, 14])
def test_fused_conv_bn_relu_matches_fp64(N):
    """ConvBNFunction on the small boards against the fp64 conv -> BatchNorm2d (-> ReLU), with the
    bars of the 20x20 test."""
    from blokus_rl_amd.alphazero.train_conv import ConvBNFunction

    g = torch.Generator().manual_seed(9)
    for relu in (True, False):
        x = torch.randn(33, 64, N, N, generator=g, dtype=torch.float64)
        w = torch.randn(64, 64, 3, 3, generator=g, dtype=torch.float64) * 0.05
        b = torch.randn(64, generator=g, dtype=torch.float64) * 0.1
        gam = torch.rand(64, generator=g, dtype=torch.float64) + 0.5
        bet = torch.randn(64, generator=g, dtype=torch.float64) * 0.2
        gy = torch.randn(33, 64, N, N, generator=g, dtype=torch.float64)
        xr, wr, br, gr, btr = (t.clone().requires_grad_() for t in (x, w, b, gam, bet))
        z = F.conv2d(xr, wr, br, padding=1)
        yr = F.batch_norm(z, torch.zeros(64, dtype=torch.float64), torch.ones(64, dtype=torch.float64), gr, btr,
                          training=True, momentum=0.1, eps=1e-5)
        if relu:
            yr = F.relu(yr)
        yr.backward(gy)
        xd = x.float().cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
        wd, bd, gd, btd = (t.float().cuda().requires_grad_() for t in (w, b, gam, bet))
        rm, rv = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
        y = ConvBNFunction.apply(xd, wd, bd, gd, btd, rm, rv, 0.1, 1e-5, relu)
        y.backward(gy.float().cuda().contiguous(memory_format=torch.channels_last))
        scale = lambda t: float(t.abs().max())  # noqa: E731
        assert float((y.detach().double().cpu() - yr.detach()).abs().max()) <= 5e-6 * scale(yr.detach())
        for a, r in ((xd.grad, xr.grad), (wd.grad, wr.grad), (gd.grad, gr.grad), (btd.grad, btr.grad)):
            assert float((a.double().cpu() - r).abs().max()) <= 2e-5 * scale(r), (relu, scale(r))
        assert float(bd.grad.abs().max()) <= 1e-6 * float(gy.abs().sum(dim=(0, 2, 3)).max())


def _replay(N, n):
    from blokus_rl_amd.alphazero.learner import DeviceReplay
    from blokus_rl_amd.alphazero.learner_bench import synthetic_replay
    from blokus_rl_amd.engine import Engine

    eng = Engine(N, 2, 5)
    buf, cap, *_ = synthetic_replay(eng, n, seed=7)
    rb = DeviceReplay(eng, cap=cap)
    rb.add_packed(buf, cap)
    return eng, rb


def _bn_fed_bias(k):
    return k in ("conv1.bias", "policy_conv.bias", "value_conv.bias") or (
        k.startswith("res_blocks") and k.endswith(".bias") and k.split(".")[2] in ("0", "3"))


def _count_np(monkeypatch):
    """Counting wrappers around train_conv's two np entry points."""
    from blokus_rl_amd.alphazero import train_conv as tc

    calls = {"conv": 0, "wgrad": 0}
    conv, wgrad = tc.conv_x3_np, tc.conv_x3_np_wgrad

    def conv_w(*a):
        calls["conv"] += 1
        return conv(*a)

    def wgrad_w(*a):
        calls["wgrad"] += 1
        return wgrad(*a)

    monkeypatch.setattr(tc, "conv_x3_np", conv_w)
    monkeypatch.setattr(tc, "conv_x3_np_wgrad", wgrad_w)
    return calls


def test_learner_7x7_matches_fp32(monkeypatch):
    """A 7x7 2-player ResNet under x3_boards="all" (dense head: F = 98) against the fp32 learner:
    one step's gradients parameter by parameter within 5e-4 of each gradient's norm (the biases of
    convs that feed a batch norm aside), four SGD steps' losses within 1e-4 relative; the np kernels
    ran: per step 4 forwards, 4 input gradients and 4 weight gradients (2 blocks)."""
    from blokus_rl_amd.alphazero.learner import Learner, alphazero_loss
    from blokus_rl_amd.alphazero.train_conv import TrainResNet, X3Conv2d, train_entry
    from blokus_rl_amd.nets import ResNet

    calls = _count_np(monkeypatch)
    assert train_entry(7, 64, "all") == "np"
    eng, rb = _replay(7, 512)
    idx = torch.randint(0, 512, (256,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    batch = rb.batch(idx)
    grads = {}
    for dp in (False, True):
        torch.manual_seed(0)
        model = ResNet(7, 2, eng.A, 2).cuda()
        L = Learner(model, batch_size=256, device_path=dp, x3_boards="all")
        assert L.sparse_head is False
        obs = batch["observation"].contiguous(memory_format=torch.channels_last) if dp else batch["observation"]
        model.train()
        p, v = model(obs)
        alphazero_loss(p, v, batch).backward()
        grads[dp] = {k: t.grad.detach().clone() for k, t in model.named_parameters()}
    assert isinstance(model, TrainResNet) and model.x3_boards == "all"
    assert calls == {"conv": 8, "wgrad": 4}
    worst = 0.0
    for k, g32 in grads[False].items():
        if _bn_fed_bias(k):
            continue  # the bias of a conv that feeds a batch norm: zero in exact arithmetic
        d = float((grads[True][k] - g32).norm())
        worst = max(worst, d / (float(g32.norm()) + 1e-30))
        print(f"{k}: |dev - fp32| / |fp32| = {d / (float(g32.norm()) + 1e-30):.3e}")
        assert d <= 5e-4 * float(g32.norm()) + 1e-12, (k, d, float(g32.norm()))
    print(f"worst relative gradient distance {worst:.3e}")

    losses = {}
    for dp in (False, True):
        torch.manual_seed(0)
        model = ResNet(7, 2, eng.A, 2).cuda()
        opt = torch.optim.SGD(model.parameters(), lr=1e-2)
        L = Learner(model, batch_size=256, seed=0, device_path=dp, optimizer=opt, x3_boards="all")
        assert L.device_path == dp and L.sparse_head is False
        assert sum(isinstance(m, X3Conv2d) for m in model.modules()) == (4 if dp else 0)
        gen = torch.Generator(device="cuda").manual_seed(1)
        losses[dp] = [float(L.train_step(rb.batch(torch.randint(0, 512, (256,), device="cuda", generator=gen))))
                      for _ in range(4)]
    print(losses)
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 1e-4 * abs(a), losses
    assert calls == {"conv": 8 + 4 * 8, "wgrad": 4 + 4 * 4}


def test_learner_14x14_sparse_head_matches_dense_head(monkeypatch):
    """A 14x14 2-player ResNet under "all": the sparse policy head (F = 392) against the same
    learner with the dense head (policy_fn wrapped, so it is not policy_loss itself): the loss to
    1e-6 relative, every parameter gradient to 1e-4 of its norm."""
    from blokus_rl_amd.alphazero.learner import Learner, policy_loss
    from blokus_rl_amd.nets import ResNet

    calls = _count_np(monkeypatch)
    eng, rb = _replay(14, 256)
    batch = rb.batch(torch.arange(256, device="cuda"))
    out = {}
    for sparse in (True, False):
        torch.manual_seed(0)
        model = ResNet(14, 2, eng.A, 2).cuda()
        fn = policy_loss if sparse else (lambda *a: policy_loss(*a))
        L = Learner(model, batch_size=256, policy_fn=fn, x3_boards="all",
                    optimizer=torch.optim.SGD(model.parameters(), lr=1e-2))
        assert L.device_path is True and L.sparse_head is sparse
        loss = float(L.train_step(batch))
        out[sparse] = (loss, {n: t.grad.detach().clone() for n, t in model.named_parameters()})
    assert calls["conv"] > 0 and calls["wgrad"] == 8
    assert abs(out[True][0] - out[False][0]) <= 1e-6 * abs(out[False][0]), (out[True][0], out[False][0])
    for n, g0 in out[False][1].items():
        if _bn_fed_bias(n):
            continue
        d = (out[True][1][n] - g0).norm()
        assert float(d) <= 1e-4 * float(g0.norm()) + 1e-12, (n, float(d), float(g0.norm()))


def test_learner_default_knob(monkeypatch):
    """Under the default ("classic") a 7x7 learner on the device path takes a working step with the
    dense head and PyTorch's convolutions; the sparse head is chosen only where trainfc takes it."""
    from blokus_rl_amd.alphazero.learner import Learner
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import ResNet

    monkeypatch.delenv("BK_X3_BOARDS", raising=False)
    calls = _count_np(monkeypatch)
    eng, rb = _replay(7, 256)
    L = Learner(ResNet(7, 2, eng.A, 1).cuda(), batch_size=256)
    assert L.device_path is True and L.sparse_head is False
    loss = L.train_step(rb.batch(torch.arange(256, device="cuda")))
    assert bool(torch.isfinite(loss))
    assert calls == {"conv": 0, "wgrad": 0}
    A20 = Engine(20, 4, 5).A
    assert Learner(ResNet(20, 4, A20, 1).cuda(), batch_size=8192).sparse_head is False
    assert Learner(ResNet(20, 4, A20, 1).cuda(), batch_size=1024).sparse_head is True
