"""Times a Learner step on the small boards with the tower convs on PyTorch's fp32 convolutions
(x3_boards="classic", the default) and on csrc/trainconv_np.hip (x3_boards="all"), in one process:
7x7 and 14x14, 2 players, ResNet-5x64, batch 1024 (Adam, the learner's defaults), the two modes in
alternating windows; and the three convolutions of one tower layer alone (forward, input gradient,
weight gradient) as back-to-back calls between two stream events, beside PyTorch's channels_last
fp32 conv on the same tensors.

    python tools/learner_np_bench.py [--out profiles/learner_np_bench.json] [--batch 1024]

Prints one JSON line and writes it to --out. Run one process at a time on the GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from blokus_rl_amd.alphazero import train_conv as tc  # noqa: E402
from blokus_rl_amd.alphazero.learner import DeviceReplay, Learner  # noqa: E402
from blokus_rl_amd.alphazero.learner_bench import synthetic_replay  # noqa: E402
from blokus_rl_amd.engine import Engine, _check, _ptr, _stream, load_library  # noqa: E402
from blokus_rl_amd.nets import ResNet  # noqa: E402


def timed_us(fn, iters: int, warm: int = 5) -> float:
    """Mean microseconds of fn() over iters back-to-back calls, between two events on the stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def bench_kernels(N: int, B: int, iters: int) -> dict:
    """One tower layer's three convolutions alone, outputs preallocated."""
    lib = load_library()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(N)
    x = torch.randn((B, 64, N, N), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    gy = torch.randn((B, 64, N, N), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    w = (torch.randn((64, 64, 3, 3), device=dev, generator=g) * (2.0 / 576) ** 0.5).contiguous(
        memory_format=torch.channels_last)
    b = torch.randn(64, device=dev, generator=g) * 0.1
    ws, inv = tc.pack_weight(w, False)
    wsf, invf = tc.pack_weight(w, True)
    y = torch.empty_like(x)
    work = torch.empty(lib.bk_conv_x3_np_wgrad_workspace_floats(B, N), device=dev)
    dw = torch.empty((64, 64, 3, 3), device=dev)
    st = _stream(dev)
    px, pgy, py = (ctypes.c_void_p(t.data_ptr()) for t in (x, gy, y))

    def fwd():
        _check(lib.bk_conv_x3_np(px, B, N, _ptr(ws), _ptr(inv), _ptr(b), py, st))

    def dgrad():
        _check(lib.bk_conv_x3_np(pgy, B, N, _ptr(wsf), _ptr(invf), None, py, st))

    def wgrad():
        _check(lib.bk_conv_x3_np_wgrad(px, pgy, B, N, _ptr(work), _ptr(dw), st))

    flop32 = 2.0 * B * N * N * 64 * 576
    out = {"fp32_equiv_gflop": flop32 / 1e9,
           "tile_boards": lib.bk_conv_x3_np_tile_boards(N), "wgrad_tile_boards": lib.bk_conv_x3_np_wgrad_tile_boards(N),
           "all": {"pack_us": timed_us(lambda: tc.pack_weight(w, False), iters), "fwd_us": timed_us(fwd, iters),
                   "dgrad_us": timed_us(dgrad, iters), "wgrad_us": timed_us(wgrad, iters)}}
    # PyTorch's fp32 conv on the same channels_last tensors: the classic path's three calls
    xn, wn = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yn = F.conv2d(xn, wn, b, padding=1)
    with torch.no_grad():
        c_fwd = timed_us(lambda: F.conv2d(xn, wn, b, padding=1), iters)
    out["classic"] = {"fwd_us": c_fwd,
                      "dgrad_us": timed_us(lambda: torch.autograd.grad(yn, xn, gy, retain_graph=True), iters),
                      "wgrad_us": timed_us(lambda: torch.autograd.grad(yn, wn, gy, retain_graph=True), iters)}
    return out


def bench_steps(N: int, B: int, steps: int, rounds: int, rows: int) -> dict:
    """Learner.train_step under both modes, `rounds` alternating windows of `steps` steps each."""
    eng = Engine(N, 2, 5)
    buf, cap, *_ = synthetic_replay(eng, rows, seed=N)
    rb = DeviceReplay(eng, cap=cap)
    rb.add_packed(buf, cap)
    gen = torch.Generator(device=eng.device).manual_seed(N)
    batches = [rb.batch(torch.randint(0, rows, (B,), device=eng.device, generator=gen)) for _ in range(4)]
    learners = {}
    for mode in ("classic", "all"):
        torch.manual_seed(0)
        learners[mode] = Learner(ResNet(N, 2, eng.A, 5).to(eng.device), batch_size=B, x3_boards=mode)
        for i in range(8):  # warm-up: code objects, the convolution library's algorithm search
            learners[mode].train_step(batches[i % 4])
    torch.cuda.synchronize()
    ms = {"classic": [], "all": []}
    for _ in range(rounds):
        for mode in ("classic", "all"):
            L = learners[mode]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(steps):
                L.train_step(batches[i % 4])
            e1.record()
            torch.cuda.synchronize()
            ms[mode].append(e0.elapsed_time(e1) / steps)
    out = {}
    for mode in ("classic", "all"):
        L = learners[mode]
        out[mode] = {"step_ms": statistics.median(ms[mode]), "step_ms_windows": ms[mode], "device_path": L.device_path,
                     "sparse_head": L.sparse_head, "samples_per_s": B / (statistics.median(ms[mode]) * 1e-3)}
    out["speedup_all_over_classic"] = out["classic"]["step_ms"] / out["all"]["step_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learner_np_bench.json"))
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--boards", type=int, nargs="+", default=[7, 14])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "players": 2, "net": "ResNet-5x64",
           "steps_per_window": args.steps, "windows": args.rounds, "kernel_iters": args.iters, "boards": {}}
    for N in args.boards:
        res["boards"][str(N)] = {"step": bench_steps(N, args.batch, args.steps, args.rounds, args.rows),
                                 "layer": bench_kernels(N, args.batch, args.iters)}
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
