"""The PPO cnn agent's ConvBlock on the device (csrc/ppoconv.hip), opt-in.

`CnnAgent.conv_block` (agent.py:45-103) is 1 -> 128 followed by 128 -> 128 convolutions, all 3x3
with stride 1 and padding 1 on 7x7 boards, each followed by Dropout and ReLU. PyTorch runs them on
MIOpen's fp32 implicit GEMMs behind NCHW <-> NHWC transposes; here the 128 -> 128 layers run on
the f16 matrix cores at fp32-class accuracy (bk_conv7: split-f16 products, the leaf net's x3
arithmetic; forward, input gradient, weight gradient), the first layer on a plain fp32 kernel that
writes NHWC directly (bk_conv7_first), and each (conv, Dropout, ReLU) triple is one launch: the
dropout's keep bits come packed from bk_dropout_keep and the ReLU is in the conv's epilogue.
Activations stay NHWC ([B, 128, 7, 7] channels_last) from the first layer to the MLP heads, whose
first Linear reads them through its weight columns permuted (no NHWC -> NCHW copy).

`prepare_agent(agent)` switches a qualifying agent in place by class swap: the same modules,
parameters and state_dict keys; anything that does not qualify is left exactly as it is.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from ..engine import _check, _ptr, _stream, load_library
from .agent import MLP, CnnAgent, ConvBlock

C = 128            # channels of the device path (d_model)
N = 7              # board side
PIX = N * N
WGRAD_STEP_BOARDS = 1  # boards per workgroup step of the weight-gradient kernel (k_conv7_x3_wgrad)


def tile_boards() -> int:
    """Boards that share one workgroup tile of bk_conv7."""
    return load_library().bk_conv7_tile_boards()


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """[B, 128, 7, 7] in any memory format -> channels_last (its buffer is the dense NHWC array)."""
    return t.contiguous(memory_format=torch.channels_last)


def _raw(t: torch.Tensor | None):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def pack_weight(weight: torch.Tensor, flip: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """[128, 128, 3, 3] f32 -> (split fragments [bk_conv7_weight_bytes()] uint8, inverse row scales
    [128] f32) of bk_conv7, on the device (flip = the input-gradient conv's weights,
    w[c][o][2-ky][2-kx]). `unpack_weight` documents the fragment order."""
    lib = load_library()
    w = _f32c(weight)
    if tuple(w.shape) != (C, C, 3, 3) or not w.is_cuda:
        raise ValueError(f"pack_weight takes a [128, 128, 3, 3] device tensor, got {tuple(w.shape)}")
    ws = torch.empty(lib.bk_conv7_weight_bytes(), dtype=torch.uint8, device=w.device)
    inv = torch.empty(C, dtype=torch.float32, device=w.device)
    _check(lib.bk_conv7_pack(_ptr(w), int(flip), _ptr(ws), _ptr(inv), _stream(w.device)))
    return ws, inv


def unpack_weight(ws: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The split fragments of `pack_weight` -> (hi, lo), each [128 o][9 tap][128 c] f16: the scaled
    GEMM row o at column k = tap * 128 + c (tap = 3 ky + kx), so (hi + lo) * inv[o] is the weight.
    Fragment order: [chunk 36 = tap * 4 + c // 32][block 8 = o // 16][part 2 = (hi, lo)]
    [k-group 4 = (c // 8) % 4][row 16 = o % 16][8 = c % 8] f16."""
    f = ws.view(torch.float16).reshape(9, 4, 8, 2, 4, 16, 8)  # tap, quarter, block, part, kg, row, el
    f = f.permute(3, 2, 5, 0, 1, 4, 6).reshape(2, C, 9, C)    # part, (block, row), tap, (quarter, kg, el)
    return f[0], f[1]


def conv7(x: torch.Tensor, ws: torch.Tensor, inv: torch.Tensor, bias: torch.Tensor | None,
          keep: torch.Tensor | None = None, keep_scale: float = 1.0, relu: bool = False) -> torch.Tensor:
    """bk_conv7 on a [B, 128, 7, 7] f32 device tensor (any memory format) -> channels_last
    y = conv(x) + bias, * keep bits * keep_scale when keep is given, ReLU when relu."""
    lib = load_library()
    if x.dim() != 4 or tuple(x.shape[1:]) != (C, N, N) or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"conv7 takes a [B, 128, 7, 7] f32 device tensor, got {tuple(x.shape)} {x.dtype}")
    B = x.shape[0]
    x = _nhwc(x)
    y = torch.empty((B, C, N, N), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    b = _f32c(bias) if bias is not None else None
    _check(lib.bk_conv7(_raw(x), B, _ptr(ws), _ptr(inv), _raw(b), _raw(keep), ctypes.c_float(keep_scale), int(relu),
                        _raw(y), _stream(x.device)))
    return y


def conv7_wgrad(x: torch.Tensor, dz: torch.Tensor) -> torch.Tensor:
    """bk_conv7_wgrad: the weight gradient [128, 128, 3, 3] from the conv's input x and the gradient
    dz of its (pre-activation) output, both [B, 128, 7, 7] f32. Deterministic; B = 0 gives zeros."""
    lib = load_library()
    if tuple(x.shape[1:]) != (C, N, N) or x.shape != dz.shape or x.dtype != torch.float32 or dz.dtype != torch.float32:
        raise ValueError("conv7_wgrad takes two [B, 128, 7, 7] f32 tensors")
    B = x.shape[0]
    x, dz = _nhwc(x), _nhwc(dz)
    ws = torch.empty(lib.bk_conv7_wgrad_workspace_floats(B), dtype=torch.float32, device=x.device)
    dw = torch.empty((C, C, 3, 3), dtype=torch.float32, device=x.device)
    _check(lib.bk_conv7_wgrad(_raw(x), _raw(dz), B, _ptr(ws), _ptr(dw), _stream(x.device)))
    return dw


def conv7_first(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, keep: torch.Tensor | None = None,
                keep_scale: float = 1.0, relu: bool = False) -> torch.Tensor:
    """bk_conv7_first: a [B, 7, 7] f32 board -> channels_last [B, 128, 7, 7] (fp32, fixed order)."""
    lib = load_library()
    if x.dim() != 3 or tuple(x.shape[1:]) != (N, N) or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"conv7_first takes a [B, 7, 7] f32 device tensor, got {tuple(x.shape)} {x.dtype}")
    B = x.shape[0]
    x = x.contiguous()
    y = torch.empty((B, C, N, N), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    b = _f32c(bias) if bias is not None else None
    _check(lib.bk_conv7_first(_raw(x), B, _ptr(_f32c(weight)), _raw(b), _raw(keep), ctypes.c_float(keep_scale),
                              int(relu), _raw(y), _stream(x.device)))
    return y


def conv7_first_wgrad(x: torch.Tensor, dz: torch.Tensor) -> torch.Tensor:
    """bk_conv7_first_wgrad: the first layer's weight gradient [128, 1, 3, 3] from the board x
    [B, 7, 7] and dz [B, 128, 7, 7]. Deterministic."""
    lib = load_library()
    B = x.shape[0]
    x, dz = x.contiguous(), _nhwc(dz)
    ws = torch.empty(lib.bk_conv7_wgrad_workspace_floats(B), dtype=torch.float32, device=x.device)
    dw = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=x.device)
    _check(lib.bk_conv7_first_wgrad(_raw(x), _raw(dz), B, _ptr(ws), _ptr(dw), _stream(x.device)))
    return dw


def dropout_keep(key: torch.Tensor, n_pixels: int, p: float) -> torch.Tensor:
    """bk_dropout_keep: packed keep bits [n_pixels, 4] int32 (bit c of a pixel's 128 = channel c
    kept, each with probability 1 - p) from a key of 2 int64 on the device."""
    lib = load_library()
    if key.dtype != torch.int64 or key.numel() != 2 or not key.is_cuda:
        raise ValueError("dropout_keep takes a key of 2 int64 on the device")
    keep = torch.empty((n_pixels, 4), dtype=torch.int32, device=key.device)
    _check(lib.bk_dropout_keep(_ptr(key.contiguous()), n_pixels, ctypes.c_float(p), _ptr(keep), _stream(key.device)))
    return keep


def unpack_keep(keep: torch.Tensor) -> torch.Tensor:
    """[n_pixels, 4] packed keep bits -> [n_pixels, 128] bool."""
    bits = torch.arange(32, device=keep.device, dtype=torch.int32)
    return ((keep.unsqueeze(-1) >> bits) & 1).reshape(keep.shape[0], C).bool()


def act_grad(gy: torch.Tensor, y: torch.Tensor, keep_scale: float) -> torch.Tensor:
    """bk_conv7_act_grad: dz = gy * [y > 0] * keep_scale on two channels_last tensors."""
    lib = load_library()
    gy, y = _nhwc(gy), _nhwc(y)
    dz = torch.empty_like(y, memory_format=torch.channels_last)
    _check(lib.bk_conv7_act_grad(_raw(gy), _raw(y), y.numel(), ctypes.c_float(keep_scale), _raw(dz), _stream(y.device)))
    return dz


def _dz(ctx, gy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The gradient at the conv's pre-activation output from the gradient at the fused output."""
    gy = _nhwc(gy)
    if ctx.relu:
        return act_grad(gy, y, ctx.keep_scale if ctx.masked else 1.0)
    return gy


def _check_epilogue(keep, relu):
    if keep is not None and not relu:
        raise ValueError("a dropout mask without the ReLU is not a device epilogue (its backward reads y > 0)")


class Conv7Function(torch.autograd.Function):
    """y = [relu]([dropout](conv2d(x, weight, bias, padding=1))) for [B, 128, 7, 7] on bk_conv7 (the
    input gradient on the same kernel with flipped weights, the weight gradient on bk_conv7_wgrad,
    the bias gradient the sum of dz); saves x, weight and y (y > 0 implies kept)."""

    @staticmethod
    def forward(ctx, x, weight, bias, keep, keep_scale, relu):
        _check_epilogue(keep, relu)
        x = _nhwc(x)
        ws, inv = pack_weight(weight, flip=False)
        y = conv7(x, ws, inv, bias, keep, float(keep_scale), bool(relu))
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.has_bias, ctx.relu, ctx.masked, ctx.keep_scale = bias is not None, bool(relu), keep is not None, float(keep_scale)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        dz = _dz(ctx, gy, y)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            ws, inv = pack_weight(weight, flip=True)
            gx = conv7(dz, ws, inv, None)
        if ctx.needs_input_grad[1]:
            gw = conv7_wgrad(x, dz)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = dz.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None, None


class Conv7FirstFunction(torch.autograd.Function):
    """The first layer: y = [relu]([dropout](conv2d(x[:, None], weight, bias, padding=1))) for a
    [B, 7, 7] board on bk_conv7_first / bk_conv7_first_wgrad; no input gradient (the board is data)."""

    @staticmethod
    def forward(ctx, x, weight, bias, keep, keep_scale, relu):
        _check_epilogue(keep, relu)
        x = x.contiguous()
        y = conv7_first(x, weight, bias, keep, float(keep_scale), bool(relu))
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.has_bias, ctx.relu, ctx.masked, ctx.keep_scale = bias is not None, bool(relu), keep is not None, float(keep_scale)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        if ctx.needs_input_grad[0]:
            raise RuntimeError("Conv7FirstFunction has no input gradient (the board is not differentiated)")
        x, weight, y = ctx.saved_tensors
        dz = _dz(ctx, gy, y)
        gw = conv7_first_wgrad(x, dz) if ctx.needs_input_grad[1] else None
        gb = dz.sum(dim=(0, 2, 3)) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return None, gw, gb, None, None, None


def _conv_ok(m: nn.Module, cin: int) -> bool:
    return (isinstance(m, nn.Conv2d) and m.in_channels == cin and m.out_channels == C and m.kernel_size == (3, 3)
            and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1
            and m.padding_mode == "zeros")


class DeviceConv2d(nn.Conv2d):
    """nn.Conv2d(128, 128, 3, padding=1) (same parameters and state_dict keys) whose f32 device calls
    on [B, 128, 7, 7] run the unfused device conv (Conv7Function; the input in any memory format,
    the output channels_last); anything else takes nn.Conv2d's own path."""

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and tuple(x.shape[1:]) == (C, N, N)
                and self.weight.is_cuda and self.weight.dtype == torch.float32):
            return Conv7Function.apply(x, self.weight, self.bias, None, 1.0, False)
        return super().forward(x)


class DeviceConvBlock(ConvBlock):
    """ConvBlock (same modules, parameters and state_dict keys) whose forward on a [B, 7, 7] f32
    device batch runs every (conv, Dropout, ReLU) triple as one fused call and returns channels_last
    [B, 128, 7, 7]. In training with p > 0 the keep bits come from bk_dropout_keep under a key drawn
    with torch.randint on the device (torch.manual_seed reproduces a run); otherwise no mask. Works
    under inference_mode. Other inputs take ConvBlock's own forward."""

    def _triples(self):
        m = list(self.conv_block)
        return [(m[i], m[i + 1], m[i + 2]) for i in range(0, len(m), 3)]

    def _device_ok(self, x: torch.Tensor) -> bool:
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and tuple(x.shape[1:]) == (N, N)
                and x.shape[0] > 0 and len(self.conv_block) % 3 == 0 and len(self.conv_block) >= 6):
            return False
        for i, (conv, drop, act) in enumerate(self._triples()):
            if not (_conv_ok(conv, 1 if i == 0 else C) and isinstance(drop, nn.Dropout) and isinstance(act, nn.ReLU)
                    and conv.weight.is_cuda and conv.weight.dtype == torch.float32):
                return False
        return True

    def forward(self, x):
        if not self._device_ok(x):
            return super().forward(x)
        B = x.shape[0]
        h = x
        for i, (conv, drop, _) in enumerate(self._triples()):
            keep, scale = None, 1.0
            if drop.training and drop.p > 0.0:
                key = torch.randint(-2 ** 62, 2 ** 62, (2,), dtype=torch.int64, device=x.device)
                keep = dropout_keep(key, B * PIX, float(drop.p))
                scale = 1.0 / (1.0 - drop.p) if drop.p < 1.0 else 0.0
            fn = Conv7FirstFunction if i == 0 else Conv7Function
            h = fn.apply(h, conv.weight, conv.bias, keep, scale, True)
        return h


def _nhwc_perm(device) -> torch.Tensor:
    """perm[j] for the NHWC-flat index j = p * 128 + c: the (c, h, w)-flat index c * 49 + p."""
    j = torch.arange(C * PIX, device=device)
    return (j % C) * PIX + j // C


class NhwcLinear(nn.Linear):
    """The heads' first nn.Linear(128 * 49, h) (same parameters and keys) reading features flattened
    in (h, w, c) order: its weight columns are permuted by a cached index (differentiable; the
    parameter keeps the reference's (c, h, w) column order)."""

    def forward(self, x):
        perm = self.__dict__.get("_bk_perm")
        if perm is None or perm.device != x.device:
            with torch.inference_mode(False):  # the rollout's first call runs under inference_mode
                perm = _nhwc_perm(x.device)
            self.__dict__["_bk_perm"] = perm
        return F.linear(x, self.weight[:, perm], self.bias)


class DeviceCnnAgent(CnnAgent):
    """CnnAgent (same modules, parameters and state_dict keys) on the device ConvBlock: features()
    are flattened in (h, w, c) order — a view of the channels_last activation, no NHWC -> NCHW copy —
    and the heads' first Linear (NhwcLinear) reads that order."""

    def features(self, x):
        h = self.conv_block(x)
        return h.permute(0, 2, 3, 1).reshape(h.size(0), -1)  # a view when h is channels_last


def _qualifies(agent: nn.Module) -> bool:
    if type(agent) is not CnnAgent or tuple(agent.input_dim) != (N, N) or agent.d_model != C:
        return False
    cb = getattr(agent, "conv_block", None)
    if type(cb) is not ConvBlock or not isinstance(cb.conv_block, nn.Sequential):
        return False
    m = list(cb.conv_block)
    if len(m) < 6 or len(m) % 3:
        return False
    for i in range(0, len(m), 3):
        if not (type(m[i]) is nn.Conv2d and _conv_ok(m[i], 1 if i == 0 else C) and type(m[i + 1]) is nn.Dropout
                and type(m[i + 2]) is nn.ReLU):
            return False
    for head in (agent.actor, agent.critic):
        if not (type(head) is MLP and type(head.net[0]) is nn.Linear and head.net[0].in_features == C * PIX):
            return False
    return True


def is_prepared(agent: nn.Module) -> bool:
    return isinstance(agent, DeviceCnnAgent)


def prepare_agent(agent: nn.Module) -> nn.Module:
    """Switch a qualifying agent to the device ConvBlock IN PLACE and return it: a CnnAgent on 7x7
    boards with d_model = 128, 3x3 / stride 1 / padding 1 convolutions, at least 2 layers. Any other
    agent is returned unchanged (never an error): it keeps PyTorch's path."""
    if not _qualifies(agent):
        return agent
    for i, m in enumerate(agent.conv_block.conv_block):
        if i >= 3 and i % 3 == 0:
            m.__class__ = DeviceConv2d
    agent.conv_block.__class__ = DeviceConvBlock
    agent.actor.net[0].__class__ = NhwcLinear
    agent.critic.net[0].__class__ = NhwcLinear
    agent.__class__ = DeviceCnnAgent
    return agent
