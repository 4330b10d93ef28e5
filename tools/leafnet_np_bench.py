"""The 7x7 2-player leaf batch and self-play with and without BK_X3_BOARDS=all.

Leaf batch: LeafResNet on B boards [B, 4, 7, 7] for B in 64 .. 4096 with 2 and 5 residual blocks,
three variants, each captured as a graph of 20 batches (so the host's launch cost, ~35 us a call
from Python, is not in the number) and replayed in interleaved rounds with device events after a
warm-up of every variant: "off" (the knob off: one bk_conv3x3 launch per conv + the heads launch,
the f32 MFMA path), "q1" / "q4" (bk_leafnet_x3_np with one / four boards per workgroup). Per
variant: the median over the rounds of the time per batch, and for q1 / q4 the rate at which the
workgroups stream the tower's weight fragments from L2 (144 KB per workgroup and tower conv).

Self-play: SelfPlay(Engine(7, 2, 5), ResNet-2x64) in continuous mode at 256 and 1024 games x 25
simulations, knob off, on, and on with leaf_input="states"; simulations per second over timed
plies, interleaved rounds.

Usage: python tools/leafnet_np_bench.py [--rounds R] [--out FILE] [--quick]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from blokus_rl_amd.alphazero.selfplay import SelfPlay  # noqa: E402
from blokus_rl_amd.engine import Engine  # noqa: E402
from blokus_rl_amd.nets import LeafResNet, ResNet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--quick", action="store_true", help="tiny run: checks the script, measures nothing useful")
opt = ap.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"

N, P = 7, 2
eng = Engine(N, P, 5)

INNER = 20  # batches per captured graph


def capture(fn):
    for _ in range(3):  # first launches load code objects and raise the kernels' LDS limits
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    return g


def timed(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream()
    e0.record(st)
    for _ in range(replays):
        g.replay()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / (replays * INNER) * 1e3  # us per batch


def leaf_table():
    rows = []
    for blocks in (2, 5):
        torch.manual_seed(blocks)
        net = ResNet(N, P, eng.A, blocks).cuda().eval()
        off = LeafResNet(net, normalize=False, features=True, x3_boards="classic").eval()
        on = LeafResNet(net, normalize=False, features=True, x3_boards="all").eval()
        assert off.x3_entry(N) is None and on.x3_entry(N) == "np"
        for B in ((64, 256) if opt.quick else (64, 256, 512, 768, 1024, 4096)):
            obs = (torch.rand((B, 2 * P, N, N), device="cuda") < 0.3).float()

            def run_on(q, obs=obs):
                os.environ["BK_X3_PACK"] = str(q)
                return on(obs)

            variants = {"off": lambda obs=obs: off(obs), "q1": lambda: run_on(1), "q4": lambda: run_on(4)}
            ref = variants["q1"]()
            assert all(torch.equal(a, b) for a, b in zip(variants["q4"](), ref)), "q4 differs from q1"
            replays = 2 if opt.quick else max(10, min(200, 100_000 // B))
            graphs = {k: capture(fn) for k, fn in variants.items()}
            for g in graphs.values():  # warm-up of every variant at this shape
                timed(g, max(2, replays // 4))
            us = {k: [] for k in variants}
            for _ in range(opt.rounds):
                for k, g in graphs.items():
                    us[k].append(timed(g, replays))
            row = {"blocks": blocks, "B": B, "batches_per_window": replays * INNER, "rounds": opt.rounds}
            for k in variants:
                row[f"{k}_us"] = statistics.median(us[k])
                row[f"{k}_us_min_max"] = [min(us[k]), max(us[k])]
            for k, q in (("q1", 1), ("q4", 4)):
                wgs = (B + q - 1) // q
                row[f"{k}_l2_weight_TBps"] = wgs * 2 * blocks * 144 * 1024 / row[f"{k}_us"] / 1e6
            row["speedup_q1_vs_off"] = row["off_us"] / row["q1_us"]
            row["speedup_q4_vs_off"] = row["off_us"] / row["q4_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.environ.pop("BK_X3_PACK", None)
    return rows


def selfplay_table():
    rows = []
    torch.manual_seed(0)
    net = ResNet(N, P, eng.A, 2).cuda().eval()
    plies = 2 if opt.quick else 12
    for games in ((64,) if opt.quick else (256, 1024)):
        sims = 25
        kinds = {"off": dict(), "on": dict(x3_boards="all"), "on_states": dict(x3_boards="all", leaf_input="states")}
        sps = {k: SelfPlay(eng, net, games, num_sims=sims, seed=1, cap=256, continuous=True, **kw)
               for k, kw in kinds.items()}
        for sp in sps.values():  # warm-up: graph capture and the first plies
            for _ in range(3):
                sp.play_ply()
            sp.check()
        rate = {k: [] for k in sps}
        for _ in range(opt.rounds):
            for k, sp in sps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(plies):
                    sp.play_ply()
                torch.cuda.synchronize()
                rate[k].append(games * sims * plies / (time.perf_counter() - t0))
        row = {"games": games, "sims": sims, "plies_per_window": plies, "rounds": opt.rounds}
        for k, sp in sps.items():
            sp.check()
            row[f"{k}_sims_per_s"] = statistics.median(rate[k])
            row[f"{k}_min_max"] = [min(rate[k]), max(rate[k])]
            row[f"{k}_leaf_input"], row[f"{k}_sim_groups"] = sp.leaf_input, sp.sim_groups
        row["speedup_on_vs_off"] = row["on_sims_per_s"] / row["off_sims_per_s"]
        row["speedup_on_states_vs_off"] = row["on_states_sims_per_s"] / row["off_sims_per_s"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


res = {"device": torch.cuda.get_device_name(0), "board": [N, P], "leaf_batch": leaf_table(),
       "selfplay": selfplay_table()}
if opt.out:
    with open(opt.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
