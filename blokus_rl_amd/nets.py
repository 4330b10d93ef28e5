"""Policy/value nets used as the MCTS leaf evaluator, kept on PyTorch-ROCm (MIOpen convs,
hipBLASLt GEMMs): the north star keeps the repo's existing net. Architectures, forward
semantics and `state_dict` keys follow the reference so its checkpoints load unchanged:

* `ResNet`  — blokus_rl/models/blokus_nnet.py:88-151: conv3x3(2P->64)+BN+ReLU, ONE residual
  around the whole stack of `num_res_blocks` (conv-BN-ReLU-conv-BN) blocks, policy head
  1x1 conv(2)+BN+ReLU+Linear(2*N*N -> A)+log_softmax, value head 1x1 conv(1)+BN+ReLU+
  Linear(N*N -> 64)+ReLU+Linear(64 -> P)+tanh.
* `DCNNet`  — blokus_nnet.py:9-85; as a leaf net optionally `LeafDCNNet` (dcnn_leaf / BK_DCNN_LEAF "x3":
  the convolutions on csrc/conv128.hip, the sparse policy head; "fused": also the heads on
  csrc/dcnnheads.hip and the first layer from packed states).
* `DumbNet` — models/dumbnet.py:6-21: logits 1, value 0 (the "uninformed MCTS" opponent).
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F
from torch import nn


class NativeBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d on PyTorch's own batch-norm kernels instead of MIOpen's (same parameters,
    buffers and state_dict keys; training-mode batch statistics and running-stat updates alike):
    nn.BatchNorm2d.forward's bookkeeping, then aten::native_batch_norm directly (F.batch_norm would
    pick MIOpen; switching the process-wide cudnn flag around it is not thread-safe)."""

    def forward(self, x):
        self._check_input_dim(x)
        factor = 0.0 if self.momentum is None else self.momentum
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
            factor = 1.0 / float(self.num_batches_tracked) if self.momentum is None else self.momentum
        use_batch = self.training or (self.running_mean is None and self.running_var is None)
        track = not self.training or self.track_running_stats
        rm = self.running_mean if track else None
        rv = self.running_var if track else None
        return torch.native_batch_norm(x, self.weight, self.bias, rm, rv, use_batch, factor, self.eps)[0]


def use_native_batchnorm(model: nn.Module) -> nn.Module:
    """Switch every BatchNorm2d of `model` to NativeBatchNorm2d in place."""
    for m in model.modules():
        if type(m) is nn.BatchNorm2d:
            m.__class__ = NativeBatchNorm2d
    return model


class ResNet(nn.Module):
    def __init__(self, board_size: int, num_players: int, action_size: int, num_res_blocks: int = 5,
                 channels: int = 64):
        super().__init__()
        self.board_x = self.board_y = board_size
        self.action_size = action_size
        self.num_players = num_players
        self.input_dim = [2 * num_players, board_size, board_size]
        c = channels
        self.conv1 = nn.Conv2d(2 * num_players, c, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm2d(c)
        self.res_blocks = nn.Sequential(*[
            nn.Sequential(nn.Conv2d(c, c, 3, padding=1), nn.BatchNorm2d(c), nn.ReLU(),
                          nn.Conv2d(c, c, 3, padding=1), nn.BatchNorm2d(c))
            for _ in range(num_res_blocks)
        ])
        n2 = board_size * board_size
        self.policy_conv = nn.Conv2d(c, 2, kernel_size=1)
        self.policy_bn = nn.BatchNorm2d(2)
        self.policy_out = nn.Linear(2 * n2, action_size)
        self.value_conv = nn.Conv2d(c, 1, kernel_size=1)
        self.value_bn = nn.BatchNorm2d(1)
        self.value_fc1 = nn.Linear(n2, 64)
        self.value_fc2 = nn.Linear(64, num_players)

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(x + self.res_blocks(x))
        p = F.relu(self.policy_bn(self.policy_conv(x))).flatten(1)
        p = F.log_softmax(self.policy_out(p), dim=1)
        v = F.relu(self.value_bn(self.value_conv(x))).flatten(1)
        v = torch.tanh(self.value_fc2(F.relu(self.value_fc1(v))))
        return p, v


class DCNNet(nn.Module):
    def __init__(self, board_size: int, num_players: int, action_size: int, num_channels: int = 128,
                 linear_dim: int = 128, dropout: float = 0.3):
        super().__init__()
        n, c, d = board_size, num_channels, linear_dim
        self.num_channels, self.board_x, self.board_y, self.dropout = c, n, n, dropout
        self.conv1 = nn.Conv2d(2 * num_players, c, 3, stride=1, padding=1)
        self.conv2 = nn.Conv2d(c, c, 3, stride=1, padding=1)
        self.conv3 = nn.Conv2d(c, c, 3, stride=1)
        self.conv4 = nn.Conv2d(c, c, 3, stride=1)
        self.bn1, self.bn2, self.bn3, self.bn4 = (nn.BatchNorm2d(c) for _ in range(4))
        self.fc1 = nn.Linear(c * (n - 4) * (n - 4), d)
        self.fc_bn1 = nn.BatchNorm1d(d)
        self.fc2 = nn.Linear(d, d // 2)
        self.fc_bn2 = nn.BatchNorm1d(d // 2)
        self.fc3 = nn.Linear(d // 2, action_size)
        self.fc4 = nn.Linear(d // 2, num_players)

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.relu(self.bn3(self.conv3(x)))
        x = F.relu(self.bn4(self.conv4(x)))
        x = x.reshape(-1, self.num_channels * (self.board_x - 4) * (self.board_y - 4))
        x = F.dropout(F.relu(self.fc_bn1(self.fc1(x))), p=self.dropout, training=self.training)
        x = F.dropout(F.relu(self.fc_bn2(self.fc2(x))), p=self.dropout, training=self.training)
        return F.log_softmax(self.fc3(x), dim=1), torch.tanh(self.fc4(x))


class DumbNet(nn.Module):
    """Uniform prior, zero value. Returns logits of 1 exactly like the reference (not a
    log-softmax); the masked log-softmax downstream makes the prior uniform either way."""

    def __init__(self, board_size: int, num_players: int, action_size: int):
        super().__init__()
        self.p_shape, self.v_shape = action_size, num_players

    def forward(self, x):
        b = x.shape[0]
        return (torch.ones((b, self.p_shape), device=x.device),
                torch.zeros((b, self.v_shape), device=x.device))


def get_model(model_type: str):
    """models/__init__.py:5-11 registry."""
    return {"dumbnet": DumbNet, "dcnnet": DCNNet, "resnet": ResNet}[model_type]


def build_model(model_type: str, board_size: int, num_players: int, action_size: int, **kw) -> nn.Module:
    cls = get_model(model_type)
    if cls is ResNet:
        return ResNet(board_size, num_players, action_size, num_res_blocks=kw.get("num_res_blocks", 5))
    if cls is DCNNet:
        return DCNNet(board_size, num_players, action_size, kw.get("num_channels", 128), kw.get("linear_dim", 128),
                      kw.get("dropout", 0.3))
    return DumbNet(board_size, num_players, action_size)


def _fold_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d) -> nn.Conv2d:
    """conv followed by eval-mode BN -> one conv with scaled weights and shifted bias."""
    fused = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                      bias=True).to(conv.weight.device)
    with torch.no_grad():
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        fused.weight.copy_(conv.weight * scale.view(-1, 1, 1, 1))
        b = conv.bias if conv.bias is not None else torch.zeros_like(bn.running_mean)
        fused.bias.copy_((b - bn.running_mean) * scale + bn.bias)
    return fused


class FusedResNet(nn.Module):
    """Inference form of `ResNet` for the leaf batch: every eval-mode BatchNorm folded into its
    convolution (MIOpen's inference BN costs as much as the convs at batch 256). Same function
    as ResNet.eval() up to float32 rounding."""

    def __init__(self, net: ResNet):
        super().__init__()
        net = net.eval()
        self.stem = _fold_bn(net.conv1, net.bn1)
        self.blocks = nn.ModuleList()
        for blk in net.res_blocks:
            self.blocks.append(nn.ModuleList([_fold_bn(blk[0], blk[1]), _fold_bn(blk[3], blk[4])]))
        self.policy_conv = _fold_bn(net.policy_conv, net.policy_bn)
        self.policy_out = net.policy_out
        self.value_conv = _fold_bn(net.value_conv, net.value_bn)
        self.value_fc1 = net.value_fc1
        self.value_fc2 = net.value_fc2
        self._fc1_t = None

    def value_fc1_wt(self) -> torch.Tensor:
        """value_fc1.weight transposed to [N*N, 64] (bk_resnet_heads' layout), cached."""
        if self._fc1_t is None:
            self._fc1_t = self.value_fc1.weight.detach().float().t().contiguous()
        return self._fc1_t

    def forward(self, x):
        x = F.relu(self.stem(x))
        h = x
        for c1, c2 in self.blocks:
            h = c2(F.relu(c1(h)))
        x = F.relu(x + h)
        p = F.relu(self.policy_conv(x)).flatten(1)
        p = F.log_softmax(self.policy_out(p).float(), dim=1)
        v = F.relu(self.value_conv(x)).flatten(1)
        v = torch.tanh(self.value_fc2(F.relu(self.value_fc1(v)))).float()
        return p, v


def _bias_act(x: torch.Tensor, bias: torch.Tensor, relu: bool, residual: torch.Tensor | None = None):
    """In-place x = act(x + bias (+ residual)) on a channels_last activation (bk_bias_act)."""
    from .engine import _check, _ptr, _stream, load_library

    assert x.is_contiguous(memory_format=torch.channels_last) and x.dtype == torch.float32
    if residual is not None:
        assert residual.is_contiguous(memory_format=torch.channels_last) and residual.shape == x.shape
    _check(load_library().bk_bias_act(ctypes.c_void_p(x.data_ptr()), x.numel(), x.shape[1], _ptr(bias),
                                      None if residual is None else ctypes.c_void_p(residual.data_ptr()),
                                      int(relu), _stream(x.device)))
    return x


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """[64, cin, 3, 3] weights -> bk_conv3x3's operand order: flat [9][cin/4][64 lanes][4 blocks]
    (cin 64: followed by pack_winograd(w) for the Winograd form used at even N),
    element (tap, s, l, j) = w[16j + (l & 15), cin(s, l >> 4), tap // 3, tap % 3] with
    cin(s, g) = 4*VEC*(s // VEC) + VEC*g + s % VEC, VEC = 4 (cin % 16 == 0), 2 (cin 8), 1 (cin 4)."""
    cout, cin = w.shape[0], w.shape[1]
    assert cout == 64 and w.shape[2:] == (3, 3) and cin in (4, 8, 64)
    vec = 4 if cin % 16 == 0 else (2 if cin == 8 else 1)
    dev = w.device
    tap = torch.arange(9, device=dev).view(9, 1, 1, 1)
    s = torch.arange(cin // 4, device=dev).view(1, -1, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 1, 64, 1)
    j = torch.arange(4, device=dev).view(1, 1, 1, 4)
    ci = 4 * vec * (s // vec) + vec * (lane >> 4) + s % vec
    co = 16 * j + (lane & 15)
    out = w.float()[co, ci, tap // 3, tap % 3].contiguous().view(-1)
    if cin != 64:
        return out
    return torch.cat([out, pack_winograd(w)])


_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def pack_winograd(w: torch.Tensor) -> torch.Tensor:
    """[64, 64, 3, 3] -> the Winograd F(2x2,3x3) form's U = G w G^T (computed in fp64, stored f32),
    twice: in k_conv3x3_wino's LDS order (form 1): flat [2 halves h][2 blocks k][16 positions p]
    [16 k-steps s][64 lanes], element = U[32h + 16k + (l & 15), 16 * (l >> 4) + s, p // 4, p % 4];
    then in k_conv3x3_wino2's register order (form 2, below)."""
    assert w.shape == (64, 64, 3, 3)
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    U = torch.einsum("ik,ockl,jl->ocij", G, w.double(), G).reshape(64, 64, 16)  # [cout][cin][p]
    dev = w.device
    h = torch.arange(2, device=dev).view(2, 1, 1, 1, 1)
    k = torch.arange(2, device=dev).view(1, 2, 1, 1, 1)
    pos = torch.arange(16, device=dev).view(1, 1, 16, 1, 1)
    st = torch.arange(16, device=dev).view(1, 1, 1, 16, 1)
    lane = torch.arange(64, device=dev).view(1, 1, 1, 1, 64)
    out = U[32 * h + 16 * k + (lane & 15), 16 * (lane >> 4) + st, pos]
    # form 2 (k_conv3x3_wino2, U in registers): [4 blocks kb][64 q][64 lanes][4 e], i = 4q + e,
    # element = U[16kb + (l & 15), 4 * (i // 16) + (l >> 4), i % 16]
    kb = torch.arange(4, device=dev).view(4, 1, 1, 1)
    q = torch.arange(64, device=dev).view(1, 64, 1, 1)
    l2 = torch.arange(64, device=dev).view(1, 1, 64, 1)
    e = torch.arange(4, device=dev).view(1, 1, 1, 4)
    i = 4 * q + e
    out2 = U[16 * kb + (l2 & 15), 4 * (i // 16) + (l2 >> 4), i % 16]
    return torch.cat([out.float().contiguous().view(-1), out2.float().contiguous().view(-1)])


def conv3x3(x: torch.Tensor, wpacked: torch.Tensor, bias: torch.Tensor, relu: bool,
            residual: torch.Tensor | None = None) -> torch.Tensor:
    """bk_conv3x3: x = planar observation [B, cin, N, N] contiguous (cin 4 / 8) or a 64-channel
    activation in channels_last memory format (NHWC) -> [B, 64, N, N] channels_last."""
    from .engine import _check, _ptr, _stream, load_library

    B, cin, N, _ = x.shape
    assert x.dtype == torch.float32
    if cin == 64:
        assert x.is_contiguous(memory_format=torch.channels_last)
    else:
        assert x.is_contiguous()
    lib = load_library()
    assert wpacked.dtype == torch.float32 and wpacked.numel() == lib.bk_conv3x3_packed_floats(cin)
    y = torch.empty((B, 64, N, N), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if residual is not None:
        assert residual.is_contiguous(memory_format=torch.channels_last) and residual.shape == y.shape
    _check(lib.bk_conv3x3(ctypes.c_void_p(x.data_ptr()), B, N, cin, _ptr(wpacked), _ptr(bias),
                                     None if residual is None else ctypes.c_void_p(residual.data_ptr()), int(relu),
                                     ctypes.c_void_p(y.data_ptr()), _stream(x.device)))
    return y


def pack_tower(weights) -> torch.Tensor:
    """[64, 64, 3, 3] weights of the tower's convs, in order -> bk_resnet_tower's u2all: each
    layer's Winograd U in the form-2 register order (the tail of pack_winograd), concatenated."""
    return torch.cat([pack_winograd(w)[-(4 * 64 * 64 * 4):] for w in weights]).contiguous()


def pack_stem_tower(w: torch.Tensor) -> torch.Tensor:
    """[64, 8, 3, 3] stem weights -> bk_resnet_stem_tower_heads' MFMA order: flat [4 blocks kb]
    [18 k-steps s][64 lanes], element = w[16kb + (l & 15), 4 * (s % 2) + (l >> 4), t // 3, t % 3]
    with tap t = s // 2."""
    assert w.shape == (64, 8, 3, 3)
    dev = w.device
    kb = torch.arange(4, device=dev).view(4, 1, 1)
    st = torch.arange(18, device=dev).view(1, 18, 1)
    lane = torch.arange(64, device=dev).view(1, 1, 64)
    t = st // 2
    return w.float()[16 * kb + (lane & 15), 4 * (st % 2) + (lane >> 4), t // 3, t % 3].contiguous().view(-1)


def pack_x3(w: torch.Tensor, b: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """[64, cin, 3, 3] conv weights (cin 8: the stem, 64: a tower conv) and bias [64] ->
    bk_leafnet_x3's operands: (split weights as uint8 bytes, inverse scales f32 [64], output bound
    f32 [2] = (A, B) with |y| <= A max|x| + B for y = conv(x) + b: A the largest row L1 norm of
    the weights, B the largest |bias|, both rounded up).

    GEMM view: A[o][k] with k = tap * cin + c (tap = 3 ky + kx), K padded to 32-wide chunks (the
    stem's 72 -> 96 with zeros). Row o is scaled by 2^e_o so that its largest magnitude lies in
    [2^14, 2^15), then split hi = f16(x), lo = f16(x - hi); inverse scale 2^-e_o. Fragment order:
    [chunk][wave 4][part hi/lo][lane 64][8 f16], lane l of wave w holding row 16w + l%16, columns
    32 chunk + 8 (l/16) .. +7 (the A operand of v_mfma_f32_16x16x32_f16)."""
    cout, cin = w.shape[0], w.shape[1]
    assert cout == 64 and w.shape[2:] == (3, 3) and cin in (8, 64)
    a = w.detach().to("cpu", torch.float64).permute(0, 2, 3, 1).reshape(64, 9 * cin)  # k = tap * cin + c
    K = (a.shape[1] + 31) // 32 * 32
    a = torch.cat([a, a.new_zeros(64, K - a.shape[1])], dim=1)
    mx = a.abs().amax(dim=1)
    _, e = torch.frexp(mx)
    e = torch.where(mx > 0, 15 - e, torch.zeros_like(e)).to(torch.float64)
    scaled = a * torch.pow(2.0, e).view(64, 1)
    hi = scaled.to(torch.float16)
    lo = (scaled - hi.to(torch.float64)).to(torch.float16)
    parts = torch.stack([hi, lo])                                   # [2][64][K]
    parts = parts.view(2, 4, 16, K // 32, 4, 8)                     # [part][wave][row][chunk][k-group][8]
    packed = parts.permute(3, 1, 0, 4, 2, 5).contiguous()           # [chunk][wave][part][k-group][row][8]
    inv = torch.pow(2.0, -e).to(torch.float32)
    bmax = float(b.detach().abs().max()) if b is not None else 0.0
    bound = torch.tensor([float(a.abs().sum(dim=1).max()) * (1 + 2 ** -16), bmax * (1 + 2 ** -16)],
                         dtype=torch.float32)
    return packed.view(torch.uint8).view(-1).to(w.device), inv.to(w.device).contiguous(), bound.to(w.device)


def pack_x3_stem(w: torch.Tensor, b: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pack_x3 of a stem with fewer than 8 input planes ([64, 2P, 3, 3], P < 4): the input channels
    zero-padded to 8, which is exact (the padded products are +-0) and leaves the row maxima, and
    so the scales and the bound, those of the unpadded weights. bk_leafnet_x3_np's wstem."""
    cin = w.shape[1]
    assert w.shape[0] == 64 and w.shape[2:] == (3, 3) and 0 < cin <= 8
    if cin < 8:
        w = torch.cat([w.detach(), w.detach().new_zeros(64, 8 - cin, 3, 3)], dim=1)
    return pack_x3(w, b)


def x3_boards_mode(arg: str | None = None) -> str:
    """Which board shapes take the one-launch split-f16 leaf net: "classic" (default) = 8 planes
    (4 players) on 14x14 / 20x20, bk_leafnet_x3 only; "all" = also 2 and 3 players and 7x7
    (bk_leafnet_x3_np). arg, else BK_X3_BOARDS."""
    import os

    m = arg if arg is not None else os.environ.get("BK_X3_BOARDS", "classic")
    if m not in ("classic", "all"):
        raise ValueError(f"x3_boards / BK_X3_BOARDS must be classic or all, got {m!r}")
    return m


def x3_pack() -> int:
    """bk_leafnet_x3_np's boards_per_wg: 0 (default) = chosen from the batch size, 1 = one board
    per workgroup, 4 = four (7x7 only); BK_X3_PACK, for tests and A/B runs. The outputs do not
    depend on it (bitwise)."""
    import os

    k = int(os.environ.get("BK_X3_PACK", "0"))
    if k not in (0, 1, 4):
        raise ValueError(f"BK_X3_PACK must be 0, 1 or 4, got {k}")
    return k


def pack_w3(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[64, 64, 3, 3] tower conv weights -> bk_leafnet_w3's operands: the Winograd F(2x2,3x3)
    transform U = G w G^T (fp64), each output channel's row scaled by 2^e_o so that its largest
    |U| lies in [2^14, 2^15), split hi = f16(x), lo = f16(x - hi); and the inverse scales 2^-e_o
    (f32 [64]). Fragment order [pos 16][chunk 2][wave 4][part hi/lo][lane 64][8 f16]: lane
    l = 16 g + r of wave w holds U[16 w + r][32 chunk + 8 g + i][pos], i = 0..7 (the A operand of
    v_mfma_f32_16x16x32_f16 for output channels 16 w.., input channels 32 chunk..)."""
    assert w.shape == (64, 64, 3, 3)
    G = torch.tensor(_WINO_G, dtype=torch.float64)
    U = torch.einsum("ik,ockl,jl->ocij", G, w.detach().to("cpu", torch.float64), G).reshape(64, 64, 16)
    mx = U.abs().amax(dim=(1, 2))
    _, e = torch.frexp(mx)
    e = torch.where(mx > 0, 15 - e, torch.zeros_like(e)).to(torch.float64)
    scaled = U * torch.pow(2.0, e).view(64, 1, 1)
    hi = scaled.to(torch.float16)
    lo = (scaled - hi.to(torch.float64)).to(torch.float16)
    parts = torch.stack([hi, lo]).view(2, 4, 16, 2, 4, 8, 16)      # [part][wave][row][chunk][g][i][pos]
    packed = parts.permute(6, 3, 1, 0, 4, 2, 5).contiguous()       # [pos][chunk][wave][part][g][row][i]
    inv = torch.pow(2.0, -e).to(torch.float32)
    return packed.view(torch.uint8).view(-1).to(w.device), inv.to(w.device).contiguous()


def net_math() -> str:
    """The leaf ResNet's arithmetic on the device: "x3" (default) = bk_leafnet_x3, split-f16 MFMA
    products with f32 accumulation (fp32-class accuracy, tests/test_leafnet_gpu.py); "w3" =
    bk_leafnet_w3, the same products with the residual tower as Winograd F(2x2,3x3) convolutions
    (2.25x fewer products per output); "f32" = the round-1 kernels on the f32 MFMA (BK_NET_MATH)."""
    import os

    m = os.environ.get("BK_NET_MATH", "x3")
    if m not in ("x3", "w3", "f32"):
        raise ValueError(f"BK_NET_MATH must be x3, w3 or f32, got {m!r}")
    return m


def _leafnet_x3_run(model: "LeafResNet", B: int, want_out: bool, **inputs):
    """One bk_leafnet_x3_run call on the B rows of inputs (leafnet_x3_args' obs, or states and
    status) with fresh outputs: (pf, v[, tower output [B, 64, N, N] channels_last])."""
    from .engine import _check, _stream, load_library

    N, dev = model.board_size, model.x3_wstem.device
    pf = torch.empty((B, 2 * N * N), dtype=torch.float32, device=dev)
    v = torch.empty((B, model.f.value_fc2.out_features), dtype=torch.float32, device=dev)
    out = torch.empty((B, 64, N, N), dtype=torch.float32, device=dev,
                      memory_format=torch.channels_last) if want_out else None
    a = leafnet_x3_args(model, pf, v, need_status=False, **inputs)
    optr = None if out is None else ctypes.c_void_p(out.data_ptr())
    _check(load_library().bk_leafnet_x3_run(ctypes.byref(a), 0, B, optr, _stream(dev)))
    return (pf, v, out) if want_out else (pf, v)


def leafnet_x3(obs: torch.Tensor, model: "LeafResNet", want_out: bool = False):
    """bk_leafnet_x3: the planar observation [B, 8, N, N] -> (policy features [B, 2*N*N], values
    [B, P][, tower output [B, 64, N, N] channels_last]) in one launch. A model whose x3 entry for
    N is "np" (LeafResNet.x3_entry: x3_boards "all") takes [B, 2P, N, N] through bk_leafnet_x3_np."""
    return _leafnet_x3_run(model, obs.shape[0], want_out, obs=obs)  # leafnet_x3_args checks obs against the model


def leafnet_x3_states(states, status: torch.Tensor | None, model: "LeafResNet", want_out: bool = False):
    """bk_leafnet_x3_states: packed states [B, 384] uint8 (N = the model's board) -> leafnet_x3's
    outputs on their observation planes, as float values, without the planes. status [B] int32
    (the search's leaf status) or None: rows whose status is not 1 are evaluated as the all-zero
    observation and their state bytes are not interpreted (the classic kernel loads them beside
    the status and drops them: stale rows, but memory of the buffer). states may also be the device address (int)
    of a [B, 384] buffer the caller keeps alive (BatchedMCTS.leaf_states_ptr), with B = len(status)."""
    from .engine import STATE_BYTES

    dev = model.x3_wstem.device
    if isinstance(states, torch.Tensor):
        assert states.dtype == torch.uint8 and states.dim() == 2 and states.shape[1] == STATE_BYTES
        assert states.is_contiguous() and states.device == dev
        B = states.shape[0]
    else:
        assert status is not None, "a raw states pointer needs status for the batch size"
        B = status.shape[0]
    return _leafnet_x3_run(model, B, want_out, states=states, status=status)  # leafnet_x3_args checks status


# bk_leafnet_args' weight fields and the LeafResNet buffers that hold them (x3_head0..8: LeafResNet.x3_heads)
_X3_OPERANDS = (("wstem", "x3_wstem"), ("sstem", "x3_sstem"), ("bstem", "x3_head0"), ("wtower", "x3_wtower"),
                ("stower", "x3_stower"), ("btower", "b_tower"), ("bounds", "x3_bounds")) + tuple(
                    (k, f"x3_head{i + 1}") for i, k in enumerate(("wp", "bp", "wv", "bv", "w1t", "b1", "w2", "b2")))


def leafnet_x3_args(model: "LeafResNet", pf: torch.Tensor, v: torch.Tensor, obs: torch.Tensor | None = None,
                    states=None, status: torch.Tensor | None = None, need_status: bool = True):
    """The operands of leafnet_x3(obs, model) or leafnet_x3_states(states, status, model) as one
    bk_leafnet_args struct (engine.LeafnetArgs) for bk_leafnet_x3_run and bk_mcts_sims_pipelined,
    with pf [B, 2*N*N] and v [B, P] as the outputs. The states form needs a status for the search
    and the net table (need_status); bk_leafnet_x3_run alone also takes None (every row a leaf).
    The struct holds raw addresses: the caller keeps model, obs / states, status, pf and v alive
    while it is in use (a captured graph: as long as the graph)."""
    from .engine import LeafnetArgs, load_library

    assert (obs is None) != (states is None)
    f = model.f
    lib = load_library()
    N, P, nl = model.board_size, f.value_fc2.out_features, 2 * len(f.blocks)
    entry = model.x3_entry(N)
    assert model.x3 and f.stem.in_channels == 2 * P and entry is not None
    assert model.x3_wtower.numel() == nl * lib.bk_leafnet_x3_weight_bytes(64)
    assert model.x3_wstem.numel() == lib.bk_leafnet_x3_weight_bytes(8)
    B = pf.shape[0]
    dev = model.x3_wstem.device
    for t, shape in ((pf, (B, 2 * N * N)), (v, (B, P))):
        assert t.dtype == torch.float32 and t.shape == shape and t.is_contiguous() and t.device == dev
    a = LeafnetArgs()
    if obs is not None:
        assert obs.dtype == torch.float32 and obs.shape == (B, 2 * P, N, N) and obs.is_contiguous() and obs.device == dev
        a.obs = obs.data_ptr()
    else:
        assert status is not None or not need_status
        if status is not None:
            assert status.dtype == torch.int32 and status.shape == (B,)
            assert status.is_contiguous() and status.device == dev
            a.status = status.data_ptr()
        a.states = states.data_ptr() if isinstance(states, torch.Tensor) else int(states)
    a.N, a.P, a.nlayers = N, P, nl
    a.np = x3_pack() + 1 if entry == "np" else 0  # bk_leafnet_x3_np[_states] with boards_per_wg = np - 1
    a.pf, a.vout = pf.data_ptr(), v.data_ptr()
    for field, name in _X3_OPERANDS:
        t = getattr(model, name)
        assert t.is_contiguous() and t.device == dev
        setattr(a, field, t.data_ptr())
    return a


def leafnet_x3_table(models, pf: torch.Tensor, v: torch.Tensor, states, status: torch.Tensor):
    """The net table of bk_leafnet_x3_rows / bk_arena_sims: one bk_leafnet_args per LeafResNet (at
    most engine.ARENA_MAX_NETS), all reading states [T, 384] (a tensor or a device address) with
    status [T] and writing pf [T, 2*N*N] / v [T, P]. The nets must agree in board size, players,
    depth and kernel form; ValueError otherwise. The rows form runs one board per workgroup, so
    the np form's boards_per_wg is pinned to 1. The caller keeps everything alive (see leafnet_x3_args)."""
    from .engine import ARENA_MAX_NETS, LeafnetArgs

    models = list(models)
    if not 0 < len(models) <= ARENA_MAX_NETS:
        raise ValueError(f"the net table holds 1 to {ARENA_MAX_NETS} nets, got {len(models)}")
    for m in models:
        if not (isinstance(m, LeafResNet) and m.takes_states()):
            raise ValueError("the net table takes LeafResNets whose takes_states() holds")
    shape = lambda m: (m.board_size, m.f.value_fc2.out_features, len(m.f.blocks), m.x3_entry(m.board_size))  # noqa: E731
    if any(shape(m) != shape(models[0]) for m in models[1:]):
        raise ValueError(f"the nets differ in (board, players, blocks, kernel form): {[shape(m) for m in models]}")
    table = (LeafnetArgs * len(models))()
    for k, m in enumerate(models):
        a = leafnet_x3_args(m, pf, v, states=states, status=status)
        if a.np:
            a.np = 2  # boards_per_wg = 1
        table[k] = a
    return table


def leafnet_x3_rows(table, rows, sim: int, device=None):
    """bk_leafnet_x3_rows: the leaf net over the arena's rows (engine.arena_rows), each live row
    with the weight set of its net; table from leafnet_x3_table (None or empty: nothing to run)."""
    from .engine import _check, _stream, load_library

    n = 0 if table is None else len(table)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    _check(load_library().bk_leafnet_x3_rows(table, n, ctypes.byref(rows), int(sim), _stream(dev)))


_OBSERVERS: dict = {}


def _observe_states(states: torch.Tensor, N: int, P: int) -> torch.Tensor:
    """bk_observe on states [B, 384] uint8 -> planes [B, 2P, N, N] f32, through an engine context
    kept per (N, P, device) (the planes do not depend on the piece set)."""
    from .engine import Engine

    key = (N, P, states.device)
    eng = _OBSERVERS.get(key)
    if eng is None:
        eng = _OBSERVERS[key] = Engine(N, P, 5, device=states.device)
    return eng.observe(states.contiguous())


def leafnet_w3(obs: torch.Tensor, model: "LeafResNet", want_out: bool = False):
    """bk_leafnet_w3: leafnet_x3's network and outputs with the residual tower as Winograd
    F(2x2,3x3) convolutions on split-f16 products (20x20 boards)."""
    from .engine import _check, _ptr, _stream, load_library

    B, cin, N, _ = obs.shape
    assert cin == 8 and obs.dtype == torch.float32 and obs.is_contiguous()
    f = model.f
    lib = load_library()
    nl = 2 * len(f.blocks)
    assert model.w3_utower.numel() == nl * lib.bk_leafnet_w3_weight_bytes()
    P = f.value_fc2.out_features
    pf = torch.empty((B, 2 * N * N), dtype=torch.float32, device=obs.device)
    v = torch.empty((B, P), dtype=torch.float32, device=obs.device)
    out = torch.empty((B, 64, N, N), dtype=torch.float32, device=obs.device,
                      memory_format=torch.channels_last) if want_out else None
    # the stem output's workspace, kept per model instance, device, batch and stream (a captured graph
    # reuses the pointer; two evaluators or streams never share one)
    cache = model.__dict__.setdefault("_w3_ws", {})
    key = (obs.device, B, N, torch.cuda.current_stream(obs.device).cuda_stream)
    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = torch.empty((B, N * N, 64), dtype=torch.float32, device=obs.device)
    h = model.x3_heads
    _check(lib.bk_leafnet_w3(
        ctypes.c_void_p(obs.data_ptr()), B, N, cin, _ptr(model.x3_wstem), _ptr(model.x3_sstem), _ptr(h[0]), nl,
        _ptr(model.w3_utower), _ptr(model.w3_stower), _ptr(model.b_tower), _ptr(model.x3_bounds),
        *[_ptr(t) for t in h[1:]], P, _ptr(pf), _ptr(v), _ptr(ws),
        None if out is None else ctypes.c_void_p(out.data_ptr()), _stream(obs.device)))
    return (pf, v, out) if want_out else (pf, v)


def tower_enabled() -> bool:
    """BK_TOWER=0 runs the residual tower as one bk_conv3x3 launch per layer instead of the fused
    bk_resnet_tower (same arithmetic; for comparisons)."""
    import os

    return os.environ.get("BK_TOWER", "1") != "0"


def resnet_tower(x: torch.Tensor, u2all: torch.Tensor, biasall: torch.Tensor, nlayers: int) -> torch.Tensor:
    """bk_resnet_tower: x = the stem output [B, 64, N, N] channels_last -> relu(x + tower(x))."""
    from .engine import _check, _ptr, _stream, load_library

    B, C, N, _ = x.shape
    assert C == 64 and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    lib = load_library()
    assert u2all.numel() == nlayers * lib.bk_tower_u_floats() and biasall.numel() == nlayers * 64
    out = torch.empty_like(x, memory_format=torch.channels_last)
    ha = torch.empty_like(x, memory_format=torch.channels_last)
    hb = torch.empty_like(x, memory_format=torch.channels_last)
    _check(lib.bk_resnet_tower(ctypes.c_void_p(x.data_ptr()), B, N, nlayers, _ptr(u2all), _ptr(biasall),
                               ctypes.c_void_p(ha.data_ptr()), ctypes.c_void_p(hb.data_ptr()),
                               ctypes.c_void_p(out.data_ptr()), _stream(x.device)))
    return out


def resnet_tower_heads(x: torch.Tensor, u2all: torch.Tensor, biasall: torch.Tensor, nlayers: int, f: "FusedResNet",
                       want_out: bool = False):
    """bk_resnet_tower_heads: the tower and the heads in one launch, from the stem output x
    [B, 64, N, N] channels_last -> (policy features [B, 2*N*N], values [B, P][, tower output])."""
    from .engine import _check, _ptr, _stream, load_library

    B, C, N, _ = x.shape
    assert C == 64 and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    lib = load_library()
    assert u2all.numel() == nlayers * lib.bk_tower_u_floats() and biasall.numel() == nlayers * 64
    P = f.value_fc2.out_features
    pf = torch.empty((B, 2 * N * N), dtype=torch.float32, device=x.device)
    v = torch.empty((B, P), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x, memory_format=torch.channels_last) if want_out else None
    ha = torch.empty_like(x, memory_format=torch.channels_last)
    hb = torch.empty_like(x, memory_format=torch.channels_last)
    c = lambda t: t.detach().float().contiguous()  # noqa: E731
    wp, wv = c(f.policy_conv.weight.view(2, 64)), c(f.value_conv.weight.view(64))
    _check(lib.bk_resnet_tower_heads(ctypes.c_void_p(x.data_ptr()), B, N, nlayers, _ptr(u2all), _ptr(biasall),
                                     ctypes.c_void_p(ha.data_ptr()), ctypes.c_void_p(hb.data_ptr()),
                                     None if out is None else ctypes.c_void_p(out.data_ptr()), _ptr(wp),
                                     _ptr(c(f.policy_conv.bias)), _ptr(wv), _ptr(c(f.value_conv.bias)),
                                     _ptr(f.value_fc1_wt()), _ptr(c(f.value_fc1.bias)), _ptr(c(f.value_fc2.weight)),
                                     _ptr(c(f.value_fc2.bias)), P, _ptr(pf), _ptr(v), _stream(x.device)))
    return (pf, v, out) if want_out else (pf, v)


def resnet_stem_tower_heads(obs: torch.Tensor, wstem: torch.Tensor, u2all: torch.Tensor, biasall: torch.Tensor,
                            nlayers: int, f: "FusedResNet", want_x0: bool = False):
    """bk_resnet_stem_tower_heads: the planar observation [B, 8, N, N] -> (policy features
    [B, 2*N*N], values [B, P][, the stem output x0]) in one launch: stem conv, tower, heads."""
    from .engine import _check, _ptr, _stream, load_library

    B, cin, N, _ = obs.shape
    assert cin == 8 and obs.dtype == torch.float32 and obs.is_contiguous()
    lib = load_library()
    assert wstem.numel() == lib.bk_stem_tower_u_floats()
    assert u2all.numel() == nlayers * lib.bk_tower_u_floats() and biasall.numel() == nlayers * 64
    P = f.value_fc2.out_features
    pf = torch.empty((B, 2 * N * N), dtype=torch.float32, device=obs.device)
    v = torch.empty((B, P), dtype=torch.float32, device=obs.device)
    x0 = torch.empty((B, 64, N, N), dtype=torch.float32, device=obs.device, memory_format=torch.channels_last)
    ha, hb = torch.empty_like(x0), torch.empty_like(x0)
    c = lambda t: t.detach().float().contiguous()  # noqa: E731
    wp, wv = c(f.policy_conv.weight.view(2, 64)), c(f.value_conv.weight.view(64))
    _check(lib.bk_resnet_stem_tower_heads(
        ctypes.c_void_p(obs.data_ptr()), B, N, cin, _ptr(wstem), _ptr(c(f.stem.bias)), nlayers, _ptr(u2all),
        _ptr(biasall), ctypes.c_void_p(x0.data_ptr()), ctypes.c_void_p(ha.data_ptr()), ctypes.c_void_p(hb.data_ptr()),
        None, _ptr(wp), _ptr(c(f.policy_conv.bias)), _ptr(wv), _ptr(c(f.value_conv.bias)), _ptr(f.value_fc1_wt()),
        _ptr(c(f.value_fc1.bias)), _ptr(c(f.value_fc2.weight)), _ptr(c(f.value_fc2.bias)), P, _ptr(pf), _ptr(v),
        _stream(obs.device)))
    return (pf, v, x0) if want_x0 else (pf, v)


def resnet_heads(x: torch.Tensor, f: "FusedResNet"):
    """bk_resnet_heads: tower output [B, 64, N, N] channels_last -> (policy features [B, 2*N*N] in
    the NCHW flatten order, values [B, P])."""
    from .engine import _check, _ptr, _stream, load_library

    B, C, N, _ = x.shape
    assert C == 64 and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    P = f.value_fc2.out_features
    pf = torch.empty((B, 2 * N * N), dtype=torch.float32, device=x.device)
    v = torch.empty((B, P), dtype=torch.float32, device=x.device)
    c = lambda t: t.detach().float().contiguous()  # noqa: E731
    wp, wv = c(f.policy_conv.weight.view(2, 64)), c(f.value_conv.weight.view(64))
    _check(load_library().bk_resnet_heads(ctypes.c_void_p(x.data_ptr()), B, N * N, _ptr(wp), _ptr(c(f.policy_conv.bias)),
                                          _ptr(wv), _ptr(c(f.value_conv.bias)), _ptr(f.value_fc1_wt()),
                                          _ptr(c(f.value_fc1.bias)), _ptr(c(f.value_fc2.weight)),
                                          _ptr(c(f.value_fc2.bias)), P, _ptr(pf), _ptr(v), _stream(x.device)))
    return pf, v


class LeafResNet(nn.Module):
    """The leaf evaluator's ResNet on the device (fp32): FusedResNet's function with the stem conv +
    bias + ReLU as one bk_conv3x3 launch, the whole residual tower (Winograd fp32 MFMA, NHWC
    activations; + the tower's residual and ReLU) as one bk_resnet_tower launch (board sizes it
    supports; one bk_conv3x3 launch per conv otherwise), both heads' 1x1 convs and the whole value MLP
    in one bk_resnet_heads launch, and the policy Linear in hipBLASLt (or, features=True, left to
    the search's sparse head). Input: the planar observation [B, 2P, N, N]. With normalize=False the policy
    comes back as raw logits (the leaf batch's consumer, k_expand_backup, takes a softmax over the
    legal ids, which a per-row shift does not change), skipping the full-row log-softmax."""

    pipelines = True  # takes_states() comes with a bk_leafnet_args form (leafnet_x3_args / leafnet_x3_table)

    def __init__(self, net: ResNet, normalize: bool = True, features: bool = False, x3_boards: str | None = None):
        super().__init__()
        # "all": the one-launch split-f16 net also for 2- and 3-player stems and 7x7 boards
        # (bk_leafnet_x3_np); "classic" (default): exactly the 8-plane 14x14 / 20x20 form
        self.x3_boards = x3_boards_mode(x3_boards)
        self.f = FusedResNet(net).eval()
        self.normalize = normalize
        self.features = features  # return (policy features [B, 2*N*N], v): the search applies policy_out
        f = self.f
        self.native = f.stem.out_channels == 64 and f.stem.in_channels in (4, 8)
        self.x3 = False
        if self.native:
            self.register_buffer("w_stem", pack_conv3x3(f.stem.weight.detach()))
            for i, (c1, c2) in enumerate(f.blocks):
                self.register_buffer(f"w_{i}_1", pack_conv3x3(c1.weight.detach()))
                self.register_buffer(f"w_{i}_2", pack_conv3x3(c2.weight.detach()))
            if f.stem.in_channels == 8:  # the stem inside the tower launch (bk_resnet_stem_tower_heads)
                self.register_buffer("w_stem_tower", pack_stem_tower(f.stem.weight.detach()))
            if len(f.blocks):  # the fused tower's operands (bk_resnet_tower)
                convs = [c for blk in f.blocks for c in blk]
                self.register_buffer("u_tower", pack_tower([c.weight.detach() for c in convs]))
                self.register_buffer("b_tower", torch.cat([c.bias.detach().float() for c in convs]).contiguous())
            self.x3 = (f.stem.in_channels == 8 or self.x3_boards == "all") and len(f.blocks) > 0
            if self.x3:
                self._register_x3(convs)

    def _register_x3(self, convs):
        """bk_leafnet_x3's operands as buffers: split f16 weights + inverse scales, the heads."""
        f = self.f
        ws, ss, bs = pack_x3_stem(f.stem.weight, f.stem.bias)
        self.register_buffer("x3_wstem", ws)
        self.register_buffer("x3_sstem", ss)
        packs = [pack_x3(c.weight, c.bias) for c in convs]
        self.register_buffer("x3_wtower", torch.cat([p[0] for p in packs]).contiguous())
        self.register_buffer("x3_stower", torch.cat([p[1] for p in packs]).contiguous())
        self.register_buffer("x3_bounds", torch.cat([bs] + [p[2] for p in packs]).contiguous())
        # bk_leafnet_w3's tower operands: split Winograd U + inverse scales
        w3 = [pack_w3(c.weight) for c in convs]
        self.register_buffer("w3_utower", torch.cat([p[0] for p in w3]).contiguous())
        self.register_buffer("w3_stower", torch.cat([p[1] for p in w3]).contiguous())
        c = lambda t: t.detach().float().contiguous().clone()  # noqa: E731
        heads = [c(f.stem.bias), c(f.policy_conv.weight.view(2, 64)), c(f.policy_conv.bias),
                 c(f.value_conv.weight.view(64)), c(f.value_conv.bias), c(f.value_fc1_wt()),
                 c(f.value_fc1.bias), c(f.value_fc2.weight), c(f.value_fc2.bias)]
        # registered buffers, so .to(device) / state_dict see them like the weight packs
        for i, t in enumerate(heads):
            self.register_buffer(f"x3_head{i}", t)

    @property
    def x3_heads(self) -> list[torch.Tensor]:
        """bk_leafnet_x3's head operands (stem bias, policy/value 1x1 convs, value MLP), on the
        module's current device."""
        return [getattr(self, f"x3_head{i}") for i in range(9)]

    @property
    def board_size(self) -> int:
        """N of the net's N x N board (the value MLP reads one feature per cell)."""
        import math

        return math.isqrt(self.f.value_fc1.in_features)

    def x3_entry(self, N: int) -> str | None:
        """The one-launch split-f16 kernel of an N x N board for this net: "classic"
        (bk_leafnet_x3[_states]: 8 planes on 14x14 / 20x20), "np" (bk_leafnet_x3_np[_states], with
        x3_boards "all": the shapes the classic entries refuse) or None (the f32 kernels)."""
        from .engine import load_library

        if not self.x3:
            return None
        lib, cin = load_library(), self.f.stem.in_channels
        if cin == 8 and lib.bk_leafnet_x3_supported(N):
            return "classic"
        if self.x3_boards == "all" and cin % 2 == 0 and lib.bk_leafnet_x3_np_supported(N, cin // 2):
            return "np"
        return None

    @property
    def planar_input(self) -> bool:
        """Whether forward reads the planar observation as the search writes it (the HIP kernels);
        the MIOpen path wants channels_last."""
        return self.native

    def sparse_head(self):
        """The Linear (policy_out) the search's sparse policy head applies to the policy features
        (features=True), or None where the module has no HIP path."""
        return self.f.policy_out if self.native else None

    def takes_states(self) -> bool:
        """Whether forward_states runs bk_leafnet_x3_states (else it observes and calls forward)."""
        return bool(self.x3 and net_math() == "x3" and self.x3_entry(self.board_size) is not None)

    def _policy(self, pf, v):
        """forward's result from the policy features pf and values v: them (features), else the
        policy Linear's logits (normalize: their log-softmax) and v."""
        if self.features:
            return pf, v
        logits = self.f.policy_out(pf)
        return (F.log_softmax(logits, dim=1) if self.normalize else logits), v

    @torch.no_grad()
    def forward_states(self, states: torch.Tensor, status: torch.Tensor | None = None):
        """forward on the observation planes of packed states [B, 384] uint8, without the planes
        where bk_leafnet_x3_states applies (takes_states): the same tuple, equal as float values.
        status [B] int32 or None: rows whose status is not 1 count as the all-zero observation
        (the search's stale leaf rows)."""
        f = self.f
        if self.takes_states():
            return self._policy(*leafnet_x3_states(states, status, self))
        obs = _observe_states(states, self.board_size, f.value_fc2.out_features)
        if status is not None:
            obs = obs * (status == 1).view(-1, 1, 1, 1).to(obs.dtype)
        return self.forward(obs)

    @torch.no_grad()
    def forward(self, x):
        f = self.f
        n = len(f.blocks)
        if self.native:
            # planar observation in (as the search writes it), NHWC activations through the tower
            from .engine import load_library

            math = net_math() if self.x3 else "f32"
            if math == "w3" and f.stem.in_channels == 8 and load_library().bk_leafnet_w3_supported(x.shape[2]):
                # the tower as Winograd convolutions on split-f16 MFMA products (bk_leafnet_w3)
                return self._policy(*leafnet_w3(x.float().contiguous(), self))
            if math in ("x3", "w3") and self.x3_entry(x.shape[2]) is not None:
                # the whole net in one launch on split-f16 MFMA products (bk_leafnet_x3)
                return self._policy(*leafnet_x3(x.float().contiguous(), self))
            fused = n and tower_enabled() and load_library().bk_tower_supported(x.shape[2])
            if fused and f.stem.in_channels == 8:
                # stem conv, tower and heads in one launch (bk_resnet_stem_tower_heads)
                return self._policy(*resnet_stem_tower_heads(x.float().contiguous(), self.w_stem_tower, self.u_tower,
                                                             self.b_tower, 2 * n, f))
            x = conv3x3(x.float().contiguous(), self.w_stem, f.stem.bias, True)
            h = x
            if fused:
                # the tower and the heads in one launch (bk_resnet_tower_heads)
                pf, v = resnet_tower_heads(x, self.u_tower, self.b_tower, 2 * n, f)
            else:
                for i, (c1, c2) in enumerate(f.blocks):
                    h = conv3x3(h, getattr(self, f"w_{i}_1"), c1.bias, True)
                    h = conv3x3(h, getattr(self, f"w_{i}_2"), c2.bias, i + 1 == n, x if i + 1 == n else None)
                if not n:
                    h = torch.relu(x + x)
                pf, v = resnet_heads(h, f)
            return self._policy(pf, v)
        # other widths: MIOpen convolutions (channels_last) with the bk_bias_act epilogue
        x = x.float().contiguous(memory_format=torch.channels_last)
        conv = lambda t, c: F.conv2d(t, c.weight, None, c.stride, c.padding)  # noqa: E731
        x = _bias_act(conv(x, f.stem), f.stem.bias, True)
        h = x
        for i, (c1, c2) in enumerate(f.blocks):
            h = _bias_act(conv(h, c1), c1.bias, True)
            h = _bias_act(conv(h, c2), c2.bias, i + 1 == n, x if i + 1 == n else None)
        x = h if n else F.relu(x + x)
        conv1 = lambda t, c: F.conv2d(t, c.weight, None).contiguous(memory_format=torch.channels_last)  # noqa: E731
        p = _bias_act(conv1(x, f.policy_conv), f.policy_conv.bias, True)
        logits = f.policy_out(p.contiguous().flatten(1))
        v = _bias_act(conv1(x, f.value_conv), f.value_conv.bias, True)
        v = torch.tanh(f.value_fc2(F.relu(f.value_fc1(v.contiguous().flatten(1)))))
        if self.features:
            return p.contiguous().flatten(1), v
        return (F.log_softmax(logits, dim=1) if self.normalize else logits), v


def dcnn_leaf_mode(arg: str | None = None) -> str:
    """How a DCNNet evaluates the leaf batch: "torch" (default) = model.eval() on PyTorch, "x3" =
    LeafDCNNet (the convolutions on the split-f16 MFMA kernels, the sparse policy head), "fused" =
    LeafDCNNet(fused=True): x3 with the heads on bk_dcnn_heads and a packed-state entry
    (bk_conv128_first_states). arg, else BK_DCNN_LEAF."""
    import os

    m = arg if arg is not None else os.environ.get("BK_DCNN_LEAF", "torch")
    if m not in ("torch", "x3", "fused"):
        raise ValueError(f"dcnn_leaf / BK_DCNN_LEAF must be torch, x3 or fused, got {m!r}")
    return m


class FoldedDCNN:
    """DCNNet's eval-mode function as plain tensors (fold_dcnn): conv_w / conv_b, the four
    convolutions with their BatchNorm folded in ([128, cin, 3, 3], [128]); fc1_w with BatchNorm1d
    folded in and its columns reordered from (c, r, col) to (r, col, c) — the NHWC order of the
    cropped fourth activation; fc2_w / fc2_b likewise folded; fc3 (policy) and fc4 (value) as they
    are. N = the board side."""

    def __init__(self, N, conv_w, conv_b, fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b, fc4_w, fc4_b):
        self.N = N
        self.conv_w, self.conv_b = conv_w, conv_b
        self.fc1_w, self.fc1_b, self.fc2_w, self.fc2_b = fc1_w, fc1_b, fc2_w, fc2_b
        self.fc3_w, self.fc3_b, self.fc4_w, self.fc4_b = fc3_w, fc3_b, fc4_w, fc4_b


@torch.no_grad()
def fold_dcnn(model: DCNNet) -> FoldedDCNN:
    """DCNNet -> FoldedDCNN in the model's dtype and on its device (eval-mode BatchNorm: the running
    statistics)."""
    def bn_scale(bn):
        s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return s, bn.bias - bn.running_mean * s

    conv_w, conv_b = [], []
    for conv, bn in ((model.conv1, model.bn1), (model.conv2, model.bn2), (model.conv3, model.bn3),
                     (model.conv4, model.bn4)):
        s, t = bn_scale(bn)
        conv_w.append((conv.weight * s.view(-1, 1, 1, 1)).contiguous())
        conv_b.append((conv.bias * s + t).contiguous())
    N, C, M = model.board_x, model.num_channels, model.board_x - 4
    s, t = bn_scale(model.fc_bn1)
    w1 = model.fc1.weight * s.view(-1, 1)
    w1 = w1.view(-1, C, M, M).permute(0, 2, 3, 1).reshape(w1.shape[0], -1).contiguous()
    b1 = (model.fc1.bias * s + t).contiguous()
    s, t = bn_scale(model.fc_bn2)
    w2 = (model.fc2.weight * s.view(-1, 1)).contiguous()
    b2 = (model.fc2.bias * s + t).contiguous()
    d = lambda p: p.detach().clone()  # noqa: E731
    return FoldedDCNN(N, conv_w, conv_b, w1, b1, w2, b2, d(model.fc3.weight), d(model.fc3.bias),
                      d(model.fc4.weight), d(model.fc4.bias))


def dcnn_fullframe_forward(folded: FoldedDCNN, obs: torch.Tensor, normalize: bool = True, features: bool = False):
    """DCNNet.eval()'s function the way the device path computes it, in pure torch: all four
    convolutions as pad-1 convolutions on the full N x N frame, then the interior [2:N-2, 2:N-2] of
    the fourth output in (r, col, c) order into the folded fc1. Exact, not approximate: the valid
    outputs of conv3 and conv4 read interior positions of their inputs only, so the border ring
    (which differs from the valid form) is never read. Returns (log-probs or, normalize=False, raw
    logits; v), or with features=True (the 64 features after fc2, v)."""
    f, N = folded, folded.N
    x = obs
    for w, b in zip(f.conv_w, f.conv_b):
        x = F.relu(F.conv2d(x, w, b, padding=1))
    x = x[:, :, 2:N - 2, 2:N - 2].permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    x = F.relu(F.linear(x, f.fc1_w, f.fc1_b))
    x = F.relu(F.linear(x, f.fc2_w, f.fc2_b))
    v = torch.tanh(F.linear(x, f.fc4_w, f.fc4_b))
    if features:
        return x, v
    logits = F.linear(x, f.fc3_w, f.fc3_b)
    return (F.log_softmax(logits, dim=1) if normalize else logits), v


def conv128_pack(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[128, 128, 3, 3] f32 device weights -> bk_conv128_x3's operands (bk_conv7_pack: the split
    f16 fragments [bk_conv7_weight_bytes()] uint8 and the inverse row scales [128] f32; they do
    not depend on the board size)."""
    from .engine import _check, _ptr, _stream, load_library

    lib = load_library()
    w = w.detach().float().contiguous()
    if tuple(w.shape) != (128, 128, 3, 3) or not w.is_cuda:
        raise ValueError(f"conv128_pack takes a [128, 128, 3, 3] device tensor, got {tuple(w.shape)}")
    ws = torch.empty(lib.bk_conv7_weight_bytes(), dtype=torch.uint8, device=w.device)
    inv = torch.empty(128, dtype=torch.float32, device=w.device)
    _check(lib.bk_conv7_pack(_ptr(w), 0, _ptr(ws), _ptr(inv), _stream(w.device)))
    return ws, inv


def _nhwc128(t: torch.Tensor, what: str) -> tuple[int, int]:
    if (t.dim() != 4 or t.shape[1] != t.shape[2] or t.shape[3] != 128 or t.dtype != torch.float32 or not t.is_cuda
            or not t.is_contiguous()):
        raise ValueError(f"{what}: a contiguous [B, N, N, 128] f32 device tensor, got {tuple(t.shape)} {t.dtype}")
    return t.shape[0], t.shape[1]


def conv128_x3(x: torch.Tensor, ws: torch.Tensor, inv: torch.Tensor, bias: torch.Tensor | None, relu: bool = False,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """bk_conv128_x3: the 128 -> 128 3x3 pad-1 convolution of an NHWC activation [B, N, N, 128] f32
    (N = 7, 14 or 20) on split-f16 MFMA products, + bias, optional ReLU -> [B, N, N, 128] (into
    `out` when given)."""
    from .engine import _check, _ptr, _stream, load_library

    B, N = _nhwc128(x, "conv128_x3")
    y = torch.empty_like(x) if out is None else out
    if out is not None and (_nhwc128(out, "conv128_x3 out") != (B, N) or out.data_ptr() == x.data_ptr()):
        raise ValueError("conv128_x3: out must be another tensor of x's shape")
    _check(load_library().bk_conv128_x3(_ptr(x), B, N, _ptr(ws), _ptr(inv), _ptr(bias), int(relu), _ptr(y),
                                        _stream(x.device)))
    return y


def conv128_first(obs: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, relu: bool = False,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """bk_conv128_first: the planar observation [B, cin, N, N] f32 (cin = 4, 6 or 8; N = 7, 14 or
    20) through the 3x3 pad-1 convolution w [128, cin, 3, 3] (or flattened [128, cin * 9]) in fp32
    with a fixed summation order, + bias, optional ReLU -> NHWC [B, N, N, 128]."""
    from .engine import _check, _ptr, _stream, load_library

    if obs.dim() != 4 or obs.shape[2] != obs.shape[3] or obs.dtype != torch.float32 or not obs.is_cuda:
        raise ValueError(f"conv128_first: a [B, cin, N, N] f32 device tensor, got {tuple(obs.shape)} {obs.dtype}")
    B, cin, N, _ = obs.shape
    if w.dtype != torch.float32 or w.numel() != 128 * cin * 9 or not w.is_contiguous():
        raise ValueError(f"conv128_first: contiguous f32 weights [128, {cin}, 3, 3], got {tuple(w.shape)} {w.dtype}")
    obs = obs.contiguous()
    y = torch.empty((B, N, N, 128), dtype=torch.float32, device=obs.device) if out is None else out
    if out is not None and _nhwc128(out, "conv128_first out") != (B, N):
        raise ValueError("conv128_first: out must be [B, N, N, 128]")
    _check(load_library().bk_conv128_first(_ptr(obs), B, N, cin, _ptr(w), _ptr(bias), int(relu), _ptr(y),
                                           _stream(obs.device)))
    return y


def conv128_first_states(states, status: torch.Tensor | None, N: int, P: int, w: torch.Tensor,
                         bias: torch.Tensor | None, relu: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """bk_conv128_first_states: conv128_first on the observation planes of packed states [B, 384]
    uint8 (P players on an N x N board; w [128, 2P, 3, 3] or flattened) without the planes, bitwise
    the same -> NHWC [B, N, N, 128]. status [B] int32 or None: rows whose status is not 1 are
    evaluated as the all-zero observation and their state bytes are not read. states may also be
    the device address (int) of a [B, 384] buffer the caller keeps alive
    (BatchedMCTS.leaf_states_ptr), with B = len(status)."""
    from .engine import STATE_BYTES, _check, _ptr, _stream, load_library

    dev = w.device
    if isinstance(states, torch.Tensor):
        if (states.dtype != torch.uint8 or states.dim() != 2 or states.shape[1] != STATE_BYTES
                or not states.is_contiguous() or states.device != dev):
            raise ValueError(f"conv128_first_states: contiguous [B, {STATE_BYTES}] uint8 states on {dev}")
        B, sptr = states.shape[0], ctypes.c_void_p(states.data_ptr())
    else:
        if status is None:
            raise ValueError("conv128_first_states: a raw states address needs status for the batch size")
        B, sptr = status.shape[0], ctypes.c_void_p(int(states))
    if status is not None and (status.dtype != torch.int32 or tuple(status.shape) != (B,) or not status.is_contiguous()
                               or status.device != dev):
        raise ValueError("conv128_first_states: status must be a contiguous [B] int32 tensor on the weights' device")
    if w.dtype != torch.float32 or w.numel() != 128 * 2 * P * 9 or not w.is_contiguous() or not w.is_cuda:
        raise ValueError(f"conv128_first_states: contiguous f32 device weights [128, {2 * P}, 3, 3], "
                         f"got {tuple(w.shape)} {w.dtype}")
    y = torch.empty((B, N, N, 128), dtype=torch.float32, device=dev) if out is None else out
    if out is not None and _nhwc128(out, "conv128_first_states out") != (B, N):
        raise ValueError("conv128_first_states: out must be [B, N, N, 128]")
    _check(load_library().bk_conv128_first_states(sptr, _ptr(status), B, N, P, _ptr(w), _ptr(bias), int(relu),
                                                  _ptr(y), _stream(dev)))
    return y


class DCNNHeads:
    """bk_dcnn_heads' operands from a FoldedDCNN (fp32, on a HIP device): fc1's weights in the
    kernel's fragment order (bk_dcnn_heads_pack), the transposed fc2 / fc4 weights, the biases, and
    the partial-sum workspaces, kept per batch size (allocated at the first call with that batch
    size, so a captured call allocates none)."""

    def __init__(self, f: FoldedDCNN):
        from .engine import _check, _ptr, _stream, load_library

        lib = load_library()
        w1 = f.fc1_w.detach().float().contiguous()
        self.N, self.P = f.N, f.fc4_w.shape[0]
        if not lib.bk_dcnn_heads_supported(self.N) or not w1.is_cuda:
            raise ValueError(f"DCNNHeads: a {self.N}x{self.N} board on {w1.device} (7x7, 14x14 or 20x20 on a HIP device)")
        if tuple(w1.shape) != (128, 128 * (self.N - 4) ** 2) or tuple(f.fc2_w.shape) != (64, 128):
            raise ValueError(f"DCNNHeads: fc1 {tuple(w1.shape)} / fc2 {tuple(f.fc2_w.shape)} are not DCNNet's at 128 channels")
        self.slices = lib.bk_dcnn_heads_slices(self.N)
        self.fc1_packed = torch.empty(lib.bk_dcnn_heads_weight_floats(self.N), dtype=torch.float32, device=w1.device)
        _check(lib.bk_dcnn_heads_pack(_ptr(w1), self.N, _ptr(self.fc1_packed), _stream(w1.device)))
        c = lambda t: t.detach().float().contiguous().clone()  # noqa: E731
        self.fc1_b, self.fc2_wt, self.fc2_b = c(f.fc1_b), c(f.fc2_w.t()), c(f.fc2_b)
        self.fc4_wt, self.fc4_b = c(f.fc4_w.t()), c(f.fc4_b)
        self._ws = {}

    def tensors(self):
        return [self.fc1_packed, self.fc1_b, self.fc2_wt, self.fc2_b, self.fc4_wt, self.fc4_b]

    def workspace(self, B: int, device) -> torch.Tensor:
        key = (B, str(device))
        if key not in self._ws:
            self._ws[key] = torch.empty(max(1, self.slices * B * 128), dtype=torch.float32, device=device)
        return self._ws[key]


def dcnn_heads(x: torch.Tensor, heads: DCNNHeads) -> tuple[torch.Tensor, torch.Tensor]:
    """bk_dcnn_heads: the fourth convolution's full-frame NHWC output [B, N, N, 128] f32 -> (the 64
    features after fc2 [B, 64], v [B, P]): the interior [2:N-2, 2:N-2] read in place, fc1 + ReLU,
    fc2 + ReLU, tanh(fc4). A board's outputs do not depend on its batch (bitwise)."""
    from .engine import _check, _ptr, _stream, load_library

    B, N = _nhwc128(x, "dcnn_heads")
    if N != heads.N or x.device != heads.fc1_packed.device:
        raise ValueError(f"dcnn_heads: a {heads.N}x{heads.N} activation on {heads.fc1_packed.device}, got {N}x{N} on {x.device}")
    feats = torch.empty((B, 64), dtype=torch.float32, device=x.device)
    v = torch.empty((B, heads.P), dtype=torch.float32, device=x.device)
    _check(load_library().bk_dcnn_heads(_ptr(x), B, N, heads.P, *[_ptr(t) for t in heads.tensors()],
                                        _ptr(heads.workspace(B, x.device)), _ptr(feats), _ptr(v), _stream(x.device)))
    return feats, v


class LeafDCNNet(nn.Module):
    """The leaf evaluator's DCNNet on the device (fp32): dcnn_fullframe_forward with conv1 as one
    bk_conv128_first launch on the planar observation [B, 2P, N, N] (as the search writes it) and
    conv2..conv4 as bk_conv128_x3 launches (split-f16 MFMA products, fp32-class) over two NHWC
    activation buffers per batch size (allocated at the first call with that batch size, so a
    captured forward allocates none of them); the crop, fc1, fc2 and fc4 stay on PyTorch (one addmm
    each). features=True returns (the 64 features after fc2, v) and leaves fc3 to the search's
    sparse policy head (sparse_head()); otherwise (log-probs or, normalize=False, raw logits; v).

    It qualifies when the net has 128 channels, 4, 6 or 8 input planes, a 7x7, 14x14 or 20x20 board
    and fp32 parameters on a HIP device. A net that does not keeps the cause in `reason` and
    forward runs model.eval() itself (the same outputs, whatever normalize / features say).

    Without `fused` there is no packed-state entry: takes_states() is False, so self-play feeds it
    observation planes. fused=True (dcnn_leaf / BK_DCNN_LEAF "fused"): the heads run on
    bk_dcnn_heads (dcnn_heads: no crop copy, no addmm; its partial sums in a per-batch-size
    workspace) and forward_states(states, status) runs the first layer on the search's packed states
    (bk_conv128_first_states, bitwise conv128_first on their planes), so takes_states() holds. Either
    way self-play runs a DCNNet's simulations as one chain (`pipelines` is False: the pipelined tree
    groups and the arena's net table are the ResNet's)."""

    pipelines = False  # no bk_leafnet_args form: SelfPlay's pipelined groups / the arena's table are LeafResNet's

    def __init__(self, model: DCNNet, normalize: bool = True, features: bool = False, fused: bool = False):
        super().__init__()
        self.model = model.eval()
        self.normalize = normalize
        self.features = features
        self.fused = bool(fused)
        self.N, self.cin = model.board_x, model.conv1.in_channels
        p = model.conv1.weight
        self.reason = None
        if model.num_channels != 128:
            self.reason = f"{model.num_channels} channels (the split-f16 kernels take 128)"
        elif self.cin not in (4, 6, 8):
            self.reason = f"{self.cin} input planes (4, 6 or 8)"
        elif self.N not in (7, 14, 20):
            self.reason = f"{self.N}x{self.N} board (7x7, 14x14 or 20x20)"
        elif p.dtype != torch.float32:
            self.reason = f"{p.dtype} parameters (float32)"
        elif p.device.type != "cuda":
            self.reason = f"parameters on {p.device.type} (a HIP device)"
        self.native = self.reason is None
        self._act = {}  # batch size -> the two NHWC activation buffers
        if not self.native:
            return
        f = fold_dcnn(model)
        # (2-D / 1-D buffers: a later .to(memory_format=channels_last) leaves their layout alone)
        self.register_buffer("w_first", f.conv_w[0].reshape(128, -1).contiguous())
        for i in range(4):
            self.register_buffer(f"b_conv{i}", f.conv_b[i])
        for i in (1, 2, 3):
            ws, inv = conv128_pack(f.conv_w[i])
            self.register_buffer(f"ws_conv{i}", ws)
            self.register_buffer(f"inv_conv{i}", inv)
        self.register_buffer("fc1_wt", f.fc1_w.t().contiguous())
        self.register_buffer("fc1_b", f.fc1_b)
        self.register_buffer("fc2_wt", f.fc2_w.t().contiguous())
        self.register_buffer("fc2_b", f.fc2_b)
        self.register_buffer("fc4_wt", f.fc4_w.t().contiguous())
        self.register_buffer("fc4_b", f.fc4_b.contiguous())
        self.heads = DCNNHeads(f) if self.fused else None

    @property
    def planar_input(self) -> bool:
        """Whether forward reads the planar observation as the search writes it."""
        return self.native

    def sparse_head(self):
        """The Linear (fc3) the search's sparse policy head applies to the features, or None."""
        return self.model.fc3 if self.native else None

    def takes_states(self) -> bool:
        """Whether forward_states runs bk_conv128_first_states (the native fused form)."""
        return bool(self.native and self.fused)

    @torch.no_grad()
    def forward_states(self, states, status: torch.Tensor | None = None):
        """forward on the observation planes of packed states [B, 384] uint8 (or the device address
        of such a buffer, with B = len(status)), without the planes: the same tuple, bitwise.
        status [B] int32 or None: rows whose status is not 1 count as the all-zero observation."""
        if not self.takes_states():
            if not isinstance(states, torch.Tensor):
                raise ValueError("LeafDCNNet.forward_states: a raw states address needs the fused native form")
            obs = _observe_states(states, self.N, self.cin // 2)
            if status is not None:
                obs = obs * (status == 1).view(-1, 1, 1, 1).to(obs.dtype)
            return self.forward(obs)
        B = states.shape[0] if isinstance(states, torch.Tensor) else status.shape[0]
        src, dst = self._activations(B, self.w_first.device)
        conv128_first_states(states, status, self.N, self.cin // 2, self.w_first, self.b_conv0, True, out=src)
        return self._tail(src, dst)

    def _activations(self, B: int, device):
        key = (B, str(device))
        if key not in self._act:
            self._act[key] = tuple(torch.empty((B, self.N, self.N, 128), dtype=torch.float32, device=device)
                                   for _ in range(2))
        return self._act[key]

    @torch.no_grad()
    def forward(self, x):
        if not self.native:
            return self.model(x)
        N, cin = self.N, self.cin
        if x.dim() != 4 or tuple(x.shape[1:]) != (cin, N, N) or not x.is_cuda:
            raise ValueError(f"LeafDCNNet takes a [B, {cin}, {N}, {N}] device tensor, got {tuple(x.shape)}")
        B = x.shape[0]
        src, dst = self._activations(B, x.device)
        conv128_first(x.float(), self.w_first, self.b_conv0, True, out=src)
        return self._tail(src, dst)

    def _tail(self, src, dst):
        """conv2..conv4 and the heads from the first layer's output in src."""
        N, B = self.N, src.shape[0]
        for i in (1, 2, 3):
            conv128_x3(src, getattr(self, f"ws_conv{i}"), getattr(self, f"inv_conv{i}"), getattr(self, f"b_conv{i}"),
                       True, out=dst)
            src, dst = dst, src
        if self.fused:
            h, v = dcnn_heads(src, self.heads)
        else:
            h = src[:, 2:N - 2, 2:N - 2, :].reshape(B, -1)  # the valid frame, (r, col, c) order
            h = torch.relu(torch.addmm(self.fc1_b, h, self.fc1_wt))
            h = torch.relu(torch.addmm(self.fc2_b, h, self.fc2_wt))
            v = torch.tanh(torch.addmm(self.fc4_b, h, self.fc4_wt))
        if self.features:
            return h, v
        logits = self.model.fc3(h)
        return (F.log_softmax(logits, dim=1) if self.normalize else logits), v


def inference_model(model: nn.Module, normalize: bool = True, dtype: torch.dtype = torch.float32,
                    features: bool = False, x3_boards: str | None = None, dcnn_leaf: str | None = None) -> nn.Module:
    """The leaf evaluator's form of a net: ResNet -> LeafResNet (fp32 HIP kernels) on a HIP
    device, FusedResNet for reduced-precision autocast runs or off the device; DCNNet ->
    LeafDCNNet with dcnn_leaf / BK_DCNN_LEAF "x3" or "fused" (LeafDCNNet(fused=True)) in fp32;
    eval() otherwise.
    normalize=False lets LeafResNet / LeafDCNNet return raw policy logits (see LeafResNet)."""
    if isinstance(model, ResNet):
        dev = next(model.parameters()).device
        if dev.type == "cuda" and dtype == torch.float32:
            return LeafResNet(model, normalize=normalize, features=features, x3_boards=x3_boards).eval()
        return FusedResNet(model).eval()
    mode = dcnn_leaf_mode(dcnn_leaf) if isinstance(model, DCNNet) else "torch"
    if mode != "torch" and dtype == torch.float32:
        return LeafDCNNet(model, normalize=normalize, features=features, fused=mode == "fused").eval()
    return model.eval()
