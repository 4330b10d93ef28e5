"""Times the PPO cnn agent's device convolutions (csrc/ppoconv.hip, ppo/device_conv.py) alone, with
stream events: the 128 -> 128 forward, input gradient and weight gradient, the first layer and its
weight gradient, the activation gradient and the keep bits, at B = 65,536 (the bench's minibatch)
and B = 8192 (the rollout's batch), beside PyTorch's NCHW fp32 conv in the same process.

    python tools/ppo_conv_bench.py [--out profiles/ppo_conv_x3.json] [--batches 65536 8192]

Writes one JSON: per batch and kernel {ms, executed TFLOP/s (3 f16 products per fp32 product),
fp32-equivalent TFLOP/s, fraction of the 2.5 PF f16 MFMA peak}. Run one process at a time on the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from blokus_rl_amd.ppo import device_conv as dc  # noqa: E402

F16_PEAK = 2.5e15
C, N = 128, 7


def timed(fn, iters: int, warm: int = 2) -> float:
    """Mean milliseconds of fn() over iters calls, between two events on the current stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def mfma_entry(ms: float, B: int) -> dict:
    flop32 = 2.0 * B * 49 * C * C * 9
    return {"ms": ms, "executed_tflops": 3 * flop32 / (ms * 1e-3) / 1e12, "fp32_equiv_tflops": flop32 / (ms * 1e-3) / 1e12,
            "frac_of_f16_peak": 3 * flop32 / (ms * 1e-3) / F16_PEAK}


def stream_entry(ms: float, nbytes: float) -> dict:
    return {"ms": ms, "bytes": nbytes, "GBps": nbytes / (ms * 1e-3) / 1e9}


def bench_batch(B: int, iters: int) -> dict:
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(B)
    x = torch.randn((B, C, N, N), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    gy = torch.randn((B, C, N, N), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    w = torch.randn((C, C, 3, 3), device=dev, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, device=dev, generator=g) * 0.1
    board = torch.randint(0, 3, (B, N, N), device=dev, generator=g).float()
    w0 = torch.randn((C, 1, 3, 3), device=dev, generator=g) / 3
    key = torch.tensor([1, 2], dtype=torch.int64, device=dev)
    keep = dc.dropout_keep(key, B * 49, 0.1)
    ws, inv = dc.pack_weight(w, False)
    wsf, invf = dc.pack_weight(w, True)
    act = 4.0 * B * 49 * C  # bytes of one activation
    out = {"B": B}
    out["pack"] = {"ms": timed(lambda: dc.pack_weight(w, False), 20)}
    out["fwd"] = mfma_entry(timed(lambda: dc.conv7(x, ws, inv, b), iters), B)
    out["fwd_fused_dropout_relu"] = mfma_entry(timed(lambda: dc.conv7(x, ws, inv, b, keep, 1 / 0.9, True), iters), B)
    out["dgrad"] = mfma_entry(timed(lambda: dc.conv7(gy, wsf, invf, None), iters), B)
    out["wgrad"] = mfma_entry(timed(lambda: dc.conv7_wgrad(x, gy), iters), B)
    out["first"] = stream_entry(timed(lambda: dc.conv7_first(board, w0, b, keep, 1 / 0.9, True), iters), act + 4.0 * B * 49)
    out["first_wgrad"] = stream_entry(timed(lambda: dc.conv7_first_wgrad(board, gy), iters), act + 4.0 * B * 49)
    out["act_grad"] = stream_entry(timed(lambda: dc.act_grad(gy, x, 1 / 0.9), iters), 3 * act)
    out["dropout_keep"] = stream_entry(timed(lambda: dc.dropout_keep(key, B * 49, 0.1), iters), 16.0 * B * 49)
    # PyTorch's fp32 conv on NCHW tensors (MIOpen), the path the agent takes with the knob off
    xn = x.contiguous().requires_grad_(True)
    wn = w.clone().requires_grad_(True)
    gyn = gy.contiguous()
    yn = F.conv2d(xn, wn, b, padding=1)
    flop32 = 2.0 * B * 49 * C * C * 9
    with torch.no_grad():
        ms = timed(lambda: F.conv2d(xn, wn, b, padding=1), iters)
    out["torch_nchw_fwd"] = {"ms": ms, "fp32_tflops": flop32 / (ms * 1e-3) / 1e12}
    ms = timed(lambda: torch.autograd.grad(yn, xn, gyn, retain_graph=True), iters)
    out["torch_nchw_dgrad"] = {"ms": ms, "fp32_tflops": flop32 / (ms * 1e-3) / 1e12}
    ms = timed(lambda: torch.autograd.grad(yn, wn, gyn, retain_graph=True), iters)
    out["torch_nchw_wgrad"] = {"ms": ms, "fp32_tflops": flop32 / (ms * 1e-3) / 1e12}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_conv_x3.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 8192])
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "f16_mfma_peak_pflops": F16_PEAK / 1e15,
           "tile_boards": dc.tile_boards(), "batches": []}
    for B in args.batches:
        r = bench_batch(B, args.iters)
        res["batches"].append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
