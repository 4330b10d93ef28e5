"""The PPO cnn agent's device ConvBlock (blokus_rl_amd/ppo/device_conv.py, csrc/ppoconv.hip): the
7x7 128-channel convolutions on split-f16 MFMA products, the 1 -> 128 first layer, the dropout's
keep bits, the fused Dropout -> ReLU epilogue and its backward, and the agent / trainer switch.

References are fp64 torch on the CPU. The bar is tests/test_train_conv_gpu.py's fp32-class one:
elementwise err <= 1e-5 * bound, bound = the same expression on absolute values (the scale of
the sum; fp32's own rounding is ~1e-7 of it)."""
import copy
import functools
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, N = 128, 7
SCALES = [1.0, 1e-6, 1e3, 0.0, 3.7]


def _wb(seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    return w, b


def _x(seed, B):
    """Boards of one tile cycle through scales 1, 1e-6, 1e3, 0, 3.7 (a 1e3 board beside a 1e-6 one
    across the shared halo row); zero rows inside board 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, N, N, generator=g, dtype=torch.float64)
    x = x * torch.tensor([SCALES[b % 5] for b in range(B)], dtype=torch.float64).view(B, 1, 1, 1)
    x[0, :, 2:4, :] = 0.0
    return x


def _bound(x, w, b=None):
    y = F.conv2d(x.abs(), w.abs(), padding=1)
    return y + (b.abs().view(1, -1, 1, 1) if b is not None else 0)


def _assert_close(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / (bound + 1e-300)).max())
    print(f"{what}: max err / bound = {ratio:.3e}")
    assert bool((err <= 1e-5 * bound + 1e-30).all()), f"{what}: max err / bound {ratio:.3e}"


@functools.lru_cache(maxsize=None)
def _forward_case(B):
    """(x, w, b, fp64 conv, bound) of the forward test at batch B, computed once."""
    w, b = _wb(2)
    x, w, b = _x(100 + B, B).float().double(), w.float().double(), b.float().double()  # exact in f32
    return x, w, b, F.conv2d(x, w, b, padding=1), _bound(x, w, b)


# ---------------------------------------------------------------- 1. pack
@pytest.mark.parametrize("flip", [False, True])
def test_pack_reproduces_the_weights(flip):
    from blokus_rl_amd.ppo.device_conv import pack_weight, unpack_weight

    w, _ = _wb(1)
    w = w.float()
    w[3] *= 1e-5     # rows of different magnitudes
    w[:, 4] *= 1e-5  # (a row of the flipped / transposed weights)
    w[7, 5] = 0.0    # zero entries
    w[9] = 0.0       # an all-zero row
    w[:, 11] = 0.0   # (and of the flipped weights)
    ref = (w.transpose(0, 1).flip(2, 3) if flip else w).double()
    ref = ref.permute(0, 2, 3, 1).reshape(C, 9, C)  # [o][tap][c]
    ws, inv = pack_weight(w.cuda(), flip)
    hi, lo = unpack_weight(ws)
    rec = (hi.double() + lo.double()).cpu() * inv.double().cpu().view(C, 1, 1)
    rowmax = ref.abs().amax(dim=(1, 2), keepdim=True)
    err = (rec - ref).abs()
    assert bool((err <= 2.0 ** -21 * rowmax).all()), float((err / (rowmax + 1e-300)).max())
    assert float(rec[11 if flip else 9].abs().max()) == 0.0
    # inv is a power of two that brings the row maximum into [2^14, 2^15)
    s = rowmax.view(-1) / inv.double().cpu()
    nz = rowmax.view(-1) > 0
    assert bool(((s[nz] >= 2.0 ** 14) & (s[nz] < 2.0 ** 15)).all())


# ---------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("case", ["1", "T", "T+1", "256T+T+3"])
def test_conv7_forward_fp32_class(case):
    from blokus_rl_amd.ppo.device_conv import conv7, pack_weight, tile_boards

    T = tile_boards()
    B = {"1": 1, "T": T, "T+1": T + 1, "256T+T+3": 256 * T + T + 3}[case]
    x, w, b, ref, bound = _forward_case(B)
    ws, inv = pack_weight(w.float().cuda(), False)
    bd = b.float().cuda()
    y = conv7(x.float().cuda(), ws, inv, bd)  # an NCHW input: conv7 makes it channels_last itself
    assert y.is_contiguous(memory_format=torch.channels_last) and tuple(y.shape) == (B, C, N, N)
    _assert_close(y, ref, bound, f"forward B={B}")
    for bz in range(3, B, 5):  # an all-zero board returns the bias exactly
        assert torch.equal(y[bz].cpu(), b.float().view(C, 1, 1).expand(C, N, N)), bz
        if bz > 40:
            break
    assert torch.equal(conv7(x.float().cuda(), ws, inv, bd), y)


# ---------------------------------------------------------------- 3. fused epilogue
def test_conv7_fused_dropout_relu():
    from blokus_rl_amd.ppo.device_conv import (Conv7Function, DeviceConv2d, conv7, dropout_keep, pack_weight,
                                               tile_boards, unpack_keep)

    B, p = tile_boards() + 1, 0.1
    w, b = _wb(3)
    w, b = w.float().double(), b.float().double()
    x = _x(31, B).float().double()
    key = torch.tensor([12345, -678], dtype=torch.int64, device="cuda")
    keep = dropout_keep(key, B * N * N, p)
    km = unpack_keep(keep).cpu().double().view(B, N, N, C).permute(0, 3, 1, 2)
    ref = F.relu((F.conv2d(x, w, b, padding=1)) * km / (1 - p))
    bound = _bound(x, w, b) * km / (1 - p)
    ws, inv = pack_weight(w.float().cuda(), False)
    xd, bd = x.float().cuda(), b.float().cuda()
    y = conv7(xd, ws, inv, bd, keep, 1.0 / (1.0 - p), True)
    _assert_close(y, ref, bound, "fused dropout + relu")
    assert bool((y.cpu()[km == 0] == 0).all())
    # without a mask and without the ReLU the fused call is the unfused conv, bit for bit
    plain = conv7(xd, ws, inv, bd)
    assert torch.equal(Conv7Function.apply(xd, w.float().cuda(), bd, None, 1.0, False), plain)
    conv = torch.nn.Conv2d(C, C, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(b.float())
    conv.__class__ = DeviceConv2d
    with torch.no_grad():
        assert torch.equal(conv(xd), plain)
    # and the ReLU alone is the ReLU of the unfused result
    assert torch.equal(conv7(xd, ws, inv, bd, None, 1.0, True), torch.relu(plain))


# ---------------------------------------------------------------- 4. gradients
def _grad_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, N, N, generator=g, dtype=torch.float64)
    if B > 1:  # log-spaced 1e-4..1e4, shuffled: a workgroup meets a larger board after a smaller one
        sc = torch.logspace(-4, 4, B, dtype=torch.float64)[torch.randperm(B, generator=g)]
        x = x * sc.view(B, 1, 1, 1)
        x[B // 2, :, 4:, :] *= 1e6  # one board with its lower rows far larger
    gy = torch.randn(B, C, N, N, generator=g, dtype=torch.float64)
    if B > 1:
        gy = gy * torch.logspace(-3, 3, B, dtype=torch.float64)[torch.randperm(B, generator=g)].view(B, 1, 1, 1)
    return x.float().double(), gy.float().double()


def _run_conv7_function(x, w, b, gy, keep, scale):
    from blokus_rl_amd.ppo.device_conv import Conv7Function

    xd = x.float().cuda().requires_grad_()
    wd, bd = w.float().cuda().requires_grad_(), b.float().cuda().requires_grad_()
    y = Conv7Function.apply(xd, wd, bd, keep, scale, True)
    y.backward(gy.float().cuda())
    return y.detach(), xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("B", [1, 300])  # 300 = 256 T' + 44, T' = WGRAD_STEP_BOARDS
def test_conv7_function_gradients_fp32_class(B):
    from blokus_rl_amd.ppo.device_conv import WGRAD_STEP_BOARDS, dropout_keep, unpack_keep

    assert B == 1 or B == 256 * WGRAD_STEP_BOARDS + 44
    p = 0.1
    w, b = _wb(4)
    w, b = w.float().double(), b.float().double()
    x, gy = _grad_inputs(B, 40 + B)
    key = torch.tensor([7, 8], dtype=torch.int64, device="cuda")
    keep = dropout_keep(key, B * N * N, p)
    km = unpack_keep(keep).cpu().double().view(B, N, N, C).permute(0, 3, 1, 2)
    scale = 1.0 / (1.0 - p)
    y, gx, gw, gb = _run_conv7_function(x, w, b, gy, keep, scale)
    # forward against fp64 with the same mask
    z = F.conv2d(x, w, b, padding=1)
    zb = _bound(x, w, b)
    _assert_close(y, F.relu(z * km * scale), zb * km * scale, f"Conv7Function forward B={B}")
    # the ReLU's derivative is taken where the device output is positive; it may differ from the
    # fp64 sign only where z is zero to within the forward bar
    pos = (y.cpu() > 0).double()
    differs = pos != ((z * km) > 0).double()
    assert bool((z.abs()[differs] <= 1e-5 * zb[differs]).all())
    dz = gy * pos * float(torch.tensor(scale, dtype=torch.float32))
    wt = w.transpose(0, 1).flip(2, 3)
    _assert_close(gx, F.conv2d(dz, wt, padding=1), F.conv2d(dz.abs(), wt.abs(), padding=1), f"dx B={B}")
    ref_w = torch.nn.grad.conv2d_weight(x, w.shape, dz, padding=1)
    bound_w = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dz.abs(), padding=1)
    _assert_close(gw, ref_w, bound_w, f"dW B={B}")
    _assert_close(gb, dz.sum(dim=(0, 2, 3)), dz.abs().sum(dim=(0, 2, 3)), f"db B={B}")
    # deterministic: a second run is bitwise equal
    y2, gx2, gw2, gb2 = _run_conv7_function(x, w, b, gy, keep, scale)
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and torch.equal(gw, gw2)


def test_conv7_wgrad_empty_batch_is_zero():
    from blokus_rl_amd.ppo.device_conv import conv7_wgrad

    e = torch.empty((0, C, N, N), device="cuda")
    dw = conv7_wgrad(e, e)
    assert tuple(dw.shape) == (C, C, 3, 3) and float(dw.abs().max()) == 0.0


# ---------------------------------------------------------------- 5. first layer
@pytest.mark.parametrize("B", [1, 300])
def test_first_layer_forward_and_weight_gradient(B):
    from blokus_rl_amd.ppo.device_conv import conv7_first, conv7_first_wgrad

    g = torch.Generator().manual_seed(50 + B)
    x = torch.randint(0, 3, (B, N, N), generator=g).double()
    x = x * torch.tensor([[1.0, 1e-3, 25.0][i % 3] for i in range(B)], dtype=torch.float64).view(B, 1, 1)
    w = (torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64) / 3).float().double()
    b = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).float().double()
    x = x.float().double()
    xd, wd, bd = x.float().cuda(), w.float().cuda(), b.float().cuda()
    y = conv7_first(xd, wd, bd)
    assert y.is_contiguous(memory_format=torch.channels_last) and tuple(y.shape) == (B, C, N, N)
    x4 = x.unsqueeze(1)
    _assert_close(y, F.conv2d(x4, w, b, padding=1), _bound(x4, w, b), f"first layer forward B={B}")
    assert torch.equal(conv7_first(xd, wd, bd, None, 1.0, True), torch.relu(y))
    dz = torch.randn(B, C, N, N, generator=g, dtype=torch.float64).float().double()
    dw = conv7_first_wgrad(xd, dz.float().cuda())
    assert tuple(dw.shape) == (C, 1, 3, 3)
    _assert_close(dw, torch.nn.grad.conv2d_weight(x4, w.shape, dz, padding=1),
                  torch.nn.grad.conv2d_weight(x4.abs(), w.shape, dz.abs(), padding=1), f"first layer dW B={B}")
    assert torch.equal(conv7_first_wgrad(xd, dz.float().cuda()), dw) and torch.equal(conv7_first(xd, wd, bd), y)


# ---------------------------------------------------------------- 6. keep bits
def test_dropout_keep_bits():
    from blokus_rl_amd.ppo.device_conv import dropout_keep, unpack_keep

    npx, p = 4096, 0.1
    key = torch.tensor([2024, 99], dtype=torch.int64, device="cuda")
    keep = dropout_keep(key, npx, p)
    bits = unpack_keep(keep).double()
    frac = float(bits.mean())
    print(f"kept fraction {frac:.5f}")
    assert abs(frac - 0.9) <= 2.1e-3  # 5 sigma over 524,288 bits
    sig_c = (0.09 / npx) ** 0.5
    assert bool(((bits.mean(dim=0) - 0.9).abs() <= 5 * sig_c).all())
    assert torch.equal(dropout_keep(key, npx, p), keep)
    other = dropout_keep(torch.tensor([2024, 100], dtype=torch.int64, device="cuda"), npx, p)
    other0 = dropout_keep(torch.tensor([2025, 99], dtype=torch.int64, device="cuda"), npx, p)
    assert not torch.equal(other, keep) and not torch.equal(other0, keep)
    assert bool((dropout_keep(key, npx, 0.0) == -1).all())  # p = 0: all ones


# ---------------------------------------------------------------- 7. agent
A = 919


def _agent(dropout, seed=0):
    from blokus_rl_amd.ppo.agent import CnnAgent

    torch.manual_seed(seed)
    hp = types.SimpleNamespace(d_model=C, cnn_layers=4, cnn_kernel_size=3, cnn_stride=1, cnn_padding=1,
                               cnn_dropout=dropout, dropout=dropout)
    return CnnAgent((N, N), A, hp)


def _agent_run(agent, obs, rl, rv):
    agent.zero_grad()
    h = agent.features(obs)
    logits, value = agent.actor(h), agent.critic(h)
    ((logits * rl).sum() + (value * rv).sum()).backward()
    out = {"logits": logits.detach(), "value": value.detach()}
    out.update({"grad:" + k: p.grad.detach().clone() for k, p in agent.named_parameters()})
    return out


def _relu_signs(agent, obs):
    """[y > 0] after each (conv, Dropout, ReLU) triple of the agent's ConvBlock (dropout 0), layer
    by layer through the agent's own modules (deterministic: the same values as its forward)."""
    from blokus_rl_amd.ppo.device_conv import Conv7FirstFunction, Conv7Function, DeviceConvBlock

    m, signs = list(agent.conv_block.conv_block), []
    with torch.no_grad():
        h = obs if type(agent.conv_block) is DeviceConvBlock else obs.unsqueeze(1)
        for i in range(0, len(m), 3):
            if type(agent.conv_block) is DeviceConvBlock:
                fn = Conv7FirstFunction if i == 0 else Conv7Function
                h = fn.apply(h, m[i].weight, m[i].bias, None, 1.0, True)
            else:
                h = m[i + 2](m[i + 1](m[i](h)))
            signs.append((h > 0).cpu())
    return signs


def _ref64_run(agent64, obs, rl, rv, signs=None):
    """The fp64 CPU agent's outputs and parameter gradients. The ReLU's derivative jumps at 0, so the
    gradients of a rounded computation are only defined up to the branch taken where a pre-activation
    is zero to within the rounding: with `signs` (a candidate's [y > 0] per layer) the fp64 agent takes
    the candidate's branch at the elements where the two disagree, and every such element must have
    |z| <= 1e-5 * (conv(|h|, |w|) + |b|) in fp64 (the forward bar): elsewhere the branch is fp64's own.
    Returns (results, number of such elements)."""
    agent64.zero_grad()
    m, nflip = list(agent64.conv_block.conv_block), 0
    h = obs.unsqueeze(1)
    for li, i in enumerate(range(0, len(m), 3)):
        z = m[i](h)
        mask = z > 0
        if signs is not None:
            differs = signs[li] != mask
            if bool(differs.any()):
                zb = _bound(h.detach(), m[i].weight.detach(), m[i].bias.detach())
                assert bool((z.detach().abs()[differs] <= 1e-5 * zb[differs]).all()), f"layer {li}: a ReLU branch differs away from 0"
                nflip += int(differs.sum())
                mask = signs[li]
        h = z * mask.double()
    f = h.reshape(h.size(0), -1)
    logits, value = agent64.actor(f), agent64.critic(f)
    ((logits * rl).sum() + (value * rv).sum()).backward()
    out = {"logits": logits.detach(), "value": value.detach()}
    out.update({"grad:" + k: p.grad.detach().clone() for k, p in agent64.named_parameters()})
    return out, nflip


def test_agent_matches_fp64_like_the_fp32_agent():
    """logits, value and every parameter gradient of one backward through the prepared agent against
    the fp64 CPU agent: error <= 4 x the unswapped fp32 agent's error + 1e-6 of the quantity's norm
    (max norm). Among the 1.6 M ReLU inputs of this batch, about one lies within fp32 rounding of 0
    (measured: the device agent and fp64 disagreed on one element of layer 2 with the first seed
    tried, the fp32 agent on none), and one flipped branch moves the upstream gradients by ~1e-3 of
    their norm whichever fp32 implementation computes them; so each candidate's gradients are
    compared with the fp64 agent's at the candidate's branches where (and only where) the
    pre-activation is zero to within the forward bar (_ref64_run)."""
    from blokus_rl_amd.ppo.device_conv import DeviceConvBlock, is_prepared, prepare_agent

    base = _agent(0.0)
    g = torch.Generator().manual_seed(5)
    obs = torch.randint(0, 3, (64, N, N), generator=g).float()
    rl, rv = torch.randn(64, A, generator=g), torch.randn(64, 1, generator=g)
    a64 = copy.deepcopy(base).double().train()
    a32 = copy.deepcopy(base).cuda().train()
    r32 = _agent_run(a32, obs.cuda(), rl.cuda(), rv.cuda())
    dev = copy.deepcopy(base).cuda().train()
    before = {k: v.clone() for k, v in dev.state_dict().items()}
    assert prepare_agent(dev) is dev and is_prepared(dev) and type(dev.conv_block) is DeviceConvBlock
    after = dev.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    rdev = _agent_run(dev, obs.cuda(), rl.cuda(), rv.cuda())
    ref, _ = _ref64_run(a64, obs.double(), rl.double(), rv.double())
    ref32, n32 = _ref64_run(a64, obs.double(), rl.double(), rv.double(), _relu_signs(a32, obs.cuda()))
    refdev, ndev = _ref64_run(a64, obs.double(), rl.double(), rv.double(), _relu_signs(dev, obs.cuda()))
    print(f"ReLU inputs at 0 to within rounding, branch differs from fp64: fp32 agent {n32}, device agent {ndev}")
    assert set(rdev) == set(ref)
    missed = []
    for k, r in ref.items():
        out = not k.startswith("grad:")  # the outputs are continuous: against the plain fp64 run
        e_dev = float((rdev[k].double().cpu() - (r if out else refdev[k])).abs().max())
        e_32 = float((r32[k].double().cpu() - (r if out else ref32[k])).abs().max())
        print(f"{k}: device {e_dev:.3e}  fp32 {e_32:.3e}  |ref| {float(r.abs().max()):.3e}")
        if not e_dev <= 4 * e_32 + 1e-6 * float(r.abs().max()):
            missed.append((k, e_dev, e_32, float(r.abs().max())))
    assert not missed, missed
    # eval mode with dropout 0.1 equals train mode with dropout 0 (no mask either way)
    ev = _agent(0.1)
    ev.load_state_dict(base.state_dict())
    ev = prepare_agent(ev.cuda()).eval()
    with torch.inference_mode():
        h_ev, h_tr = ev.features(obs.cuda()), dev.features(obs.cuda())
        assert torch.equal(h_ev, h_tr)
        assert torch.equal(ev.actor(h_ev), dev.actor(h_tr))
    # the benchmark's call pattern: one conv on an NCHW tensor, differentiated w.r.t. its input
    for agent in (dev, a32):
        conv = agent.conv_block.conv_block[3]
        x = torch.randn((16, C, N, N), device="cuda", requires_grad=True)
        y = conv(x)
        dy = torch.randn_like(y)
        (gx,) = torch.autograd.grad(y, x, dy, retain_graph=True)
        assert gx.shape == x.shape and bool(torch.isfinite(gx).all())


def test_prepare_agent_leaves_other_agents_alone():
    from blokus_rl_amd.ppo.agent import CnnAgent, ConvBlock, MlpAgent
    from blokus_rl_amd.ppo.device_conv import is_prepared, prepare_agent

    hp = types.SimpleNamespace(d_model=64, cnn_layers=4, cnn_kernel_size=3, cnn_stride=1, cnn_padding=1,
                               cnn_dropout=0.1, dropout=0.1)
    a = CnnAgent((N, N), A, hp)
    assert prepare_agent(a) is a and type(a) is CnnAgent and type(a.conv_block) is ConvBlock
    hp.d_model = C
    a = CnnAgent((5, 5), 100, hp)
    assert prepare_agent(a) is a and type(a) is CnnAgent
    hp.cnn_layers = 1
    a = CnnAgent((N, N), A, hp)
    assert prepare_agent(a) is a and type(a) is CnnAgent
    m = MlpAgent((N, N), A, hp)
    assert prepare_agent(m) is m and type(m) is MlpAgent and not is_prepared(m)


# ---------------------------------------------------------------- 8. trainer
def _hp(tmp_path, **kw):
    from blokus_rl_amd.ppo.trainer import PPOHparams

    d = dict(agent_type="cnn", d_model=C, num_envs=64, num_steps=16, dropout=0.1, cnn_dropout=0.1,
             board_size=7, max_piece_cells=4, save_interval=10 ** 9, checkpoint_dir=tmp_path, seed=1)
    d.update(kw)
    return PPOHparams(**d)


def test_trainer_runs_on_the_device_convs(tmp_path, monkeypatch):
    import math

    from blokus_rl_amd.ppo.device_conv import DeviceConvBlock
    from blokus_rl_amd.ppo.trainer import PPOTrainer

    monkeypatch.delenv("BK_PPO_CONV", raising=False)
    tr = PPOTrainer(_hp(tmp_path), device_convs=True)
    assert tr.device_convs and type(tr.agent.conv_block) is DeviceConvBlock
    logs = tr.train(2)
    assert len(logs) == 2
    for log in logs:
        assert all(math.isfinite(float(v)) for k, v in log.items() if k != "explained_variance"), log
    tr._save_checkpoint(2)
    ck = torch.load(tmp_path / "checkpoint_2.pt", map_location="cpu", weights_only=True)
    default = PPOTrainer(_hp(tmp_path))
    assert not default.device_convs and type(default.agent.conv_block) is not DeviceConvBlock
    assert list(ck["agent"]) == list(default.agent.state_dict())
    assert all(ck["agent"][k].shape == v.shape for k, v in default.agent.state_dict().items())
    # the environment knob
    monkeypatch.setenv("BK_PPO_CONV", "x3")
    assert type(PPOTrainer(_hp(tmp_path), device_convs=None).agent.conv_block) is DeviceConvBlock
    monkeypatch.setenv("BK_PPO_CONV", "1")
    assert type(PPOTrainer(_hp(tmp_path)).agent.conv_block) is not DeviceConvBlock
    monkeypatch.delenv("BK_PPO_CONV")
    assert type(PPOTrainer(_hp(tmp_path), device_convs=None).agent.conv_block) is not DeviceConvBlock


@pytest.mark.parametrize("kw", [dict(d_model=64), dict(board_size=5), dict(board_size=5, max_piece_cells=5)])
def test_trainer_falls_back_for_unsupported_agents(tmp_path, monkeypatch, kw):
    """(the rollout's fused draw + step kernel is the 7x7 presets': a 5x5 board takes the trainer's
    torch Categorical path by the trainer's own default)"""
    import math

    from blokus_rl_amd.ppo.agent import CnnAgent, ConvBlock
    from blokus_rl_amd.ppo.trainer import PPOTrainer

    monkeypatch.delenv("BK_PPO_CONV", raising=False)
    tr = PPOTrainer(_hp(tmp_path, **kw), device_convs=True)
    assert tr.device_sampling is (kw.get("board_size", 7) == 7)
    assert not tr.device_convs and type(tr.agent) is CnnAgent and type(tr.agent.conv_block) is ConvBlock
    logs = tr.train(2)
    assert len(logs) == 2 and math.isfinite(float(logs[-1]["loss"]))


def test_trainer_refuses_device_sampling_without_the_kernels(tmp_path):
    from blokus_rl_amd.ppo.trainer import PPOTrainer

    with pytest.raises(ValueError, match="board_size=5, max_piece_cells=4"):
        PPOTrainer(_hp(tmp_path, board_size=5), device_sampling=True)
    assert PPOTrainer(_hp(tmp_path, board_size=5), device_sampling=False).device_sampling is False
    assert PPOTrainer(_hp(tmp_path), device_sampling=False).device_sampling is False
    assert PPOTrainer(_hp(tmp_path)).device_sampling is True
