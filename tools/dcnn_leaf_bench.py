"""DCNNet's leaf batch on PyTorch (BK_DCNN_LEAF=torch), on the split-f16 convolutions
(BK_DCNN_LEAF=x3, nets.LeafDCNNet) and with the fused heads and the packed-state first layer
(BK_DCNN_LEAF=fused), at G boards of 20x20 / 4 players and 7x7 / 2 players.

Whole batch: what LeafEvaluator runs per simulation — "torch": DCNNet.eval() on the channels_last
observation, dense logits over all A ids; "x3": LeafDCNNet(features=True) on the planar
observation, the 64 features (fc3 is left to the search's sparse head, which is not part of this
number); "fused": LeafDCNNet(features=True, fused=True) on the same planes (the heads on
bk_dcnn_heads); "fused-states": its forward_states on the packed states and a status of ones
(bk_conv128_first_states: what SelfPlay(leaf_input="states") runs). The boards are seeded random
playouts of 0..60 plies (boards.random_boards) and the planes are their observation. Each variant
is captured as a graph of INNER batches (no host launch cost in the number)
and replayed in interleaved rounds with device events after a warm-up of every variant; the figure
is the median over the rounds of the time per batch.

Stages of the x3 path, each captured and timed alone the same way: the first layer
(k_conv128_first), one 128 -> 128 layer (k_conv128_x3, or k_conv7_x3 at 7x7) with its achieved
MFMA rate (executed products: 3 f16 products per term, 400 columns per tile), the heads on
PyTorch (crop copy, fc1, fc2, fc4), and the fused path's two pieces: the first layer from packed
states (k_conv128_first_states) and the heads kernel (k_dcnn_fc1 + k_dcnn_tail) with its rates
against the work (2 B 128 K1 flop of fc1) and the bytes it has to move (the interior activation,
fc1's weights once, the partial sums out and in). Per-kernel times of the torch path come from a kernel trace of
`--trace torch` / `--trace x3` (a plain loop of eager batches for a profiler to look at; it prints
the event-timed ms per eager batch).

Usage: python tools/dcnn_leaf_bench.py [--games G] [--rounds R] [--out FILE] [--quick]
       python tools/dcnn_leaf_bench.py --trace torch|x3 [--board 20|7]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from blokus_rl_amd.engine import Engine  # noqa: E402
from blokus_rl_amd.boards import random_boards  # noqa: E402
from blokus_rl_amd.nets import (DCNNet, LeafDCNNet, conv128_first, conv128_first_states, conv128_x3,  # noqa: E402
                                dcnn_heads)

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=256)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--quick", action="store_true", help="tiny run: checks the script, measures nothing useful")
ap.add_argument("--trace", choices=["torch", "x3", "fused", "fused-states"], default=None, help="only run eager batches of one variant")
ap.add_argument("--board", type=int, choices=[7, 20], default=20, help="--trace: the board")
opt = ap.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"

INNER = 4 if opt.quick else 10  # batches per captured graph
G = 8 if opt.quick else opt.games


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):  # first launches load code objects, pick algorithms, allocate the buffers
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    return g


def timed_ms(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream()
    e0.record(st)
    for _ in range(replays):
        g.replay()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / (replays * INNER)


def interleaved(graphs: dict, rounds: int, replays: int) -> dict:
    for g in graphs.values():  # warm up every variant
        timed_ms(g, 1)
    ms = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            ms[k].append(timed_ms(g, replays))
    return {k: {"ms_per_batch": statistics.median(v), "min": min(v), "max": max(v), "rounds": len(v)}
            for k, v in ms.items()}


def setup(N, P):
    eng = Engine(N, P, 5)
    torch.manual_seed(0)
    net = DCNNet(N, P, eng.A).cuda().eval()
    states = random_boards(eng, G, seed0=1).contiguous()
    return eng, net, eng.observe(states).contiguous(), states


def board(N, P):
    eng, net, obs, states = setup(N, P)
    leaf = LeafDCNNet(net, normalize=False, features=True).eval()
    fused = LeafDCNNet(net, normalize=False, features=True, fused=True).eval()
    assert leaf.native and fused.native and fused.takes_states(), leaf.reason
    status = torch.ones(G, dtype=torch.int32, device="cuda")
    obs_cl = obs.contiguous(memory_format=torch.channels_last)
    net_cl = net.to(memory_format=torch.channels_last)

    def run_torch():
        with torch.inference_mode():
            return net_cl(obs_cl)

    def run_x3():
        with torch.inference_mode():
            return leaf(obs)

    def run_fused():
        with torch.inference_mode():
            return fused(obs)

    def run_fused_states():
        with torch.inference_mode():
            return fused.forward_states(states, status)

    replays = 1 if opt.quick else (5 if N == 20 else 40)  # a timed window of tenths of a second
    rounds = 2 if opt.quick else opt.rounds
    whole = interleaved({"torch": capture(run_torch), "x3": capture(run_x3), "fused": capture(run_fused),
                         "fused-states": capture(run_fused_states)}, rounds, replays)
    # the x3 path's stages, alone
    a, b = leaf._activations(G, obs.device)

    def heads():
        with torch.inference_mode():
            h = b[:, 2:N - 2, 2:N - 2, :].reshape(G, -1)
            h = torch.relu(torch.addmm(leaf.fc1_b, h, leaf.fc1_wt))
            h = torch.relu(torch.addmm(leaf.fc2_b, h, leaf.fc2_wt))
            return torch.tanh(torch.addmm(leaf.fc4_b, h, leaf.fc4_wt))

    stages = interleaved({
        "conv128_first": capture(lambda: conv128_first(obs, leaf.w_first, leaf.b_conv0, True, out=a)),
        "conv128_x3": capture(lambda: conv128_x3(a, leaf.ws_conv1, leaf.inv_conv1, leaf.b_conv1, True, out=b)),
        "heads_torch": capture(heads),
        "conv128_first_states": capture(lambda: conv128_first_states(states, status, N, P, leaf.w_first, leaf.b_conv0,
                                                                     True, out=a)),
        "heads_fused": capture(lambda: dcnn_heads(b, fused.heads)),
    }, rounds, replays)
    # the heads kernel against its work and its bytes
    K1, S = 128 * (N - 4) ** 2, fused.heads.slices
    h = stages["heads_fused"]
    h["fc1_gflop"] = 2.0 * G * 128 * K1 / 1e9
    h["fc1_tflops"] = 2.0 * G * 128 * K1 / (h["ms_per_batch"] * 1e-3) / 1e12
    h["k_slices"] = S
    h["min_mb"] = (G * K1 + 128 * K1 + 2 * S * G * 128) * 4 / 1e6
    h["min_mb_over_time_tb_s"] = h["min_mb"] / 1e6 / (h["ms_per_batch"] * 1e-3)
    h["over_heads_torch_time"] = h["ms_per_batch"] / stages["heads_torch"]["ms_per_batch"]
    f = stages["conv128_first_states"]
    f["store_mb"] = G * N * N * 128 * 4 / 1e6
    f["over_conv128_first_time"] = f["ms_per_batch"] / stages["conv128_first"]["ms_per_batch"]
    # executed MFMA work of one 128 -> 128 layer: tiles x 400 columns x 128 rows x K 1152 x 3 products
    from blokus_rl_amd.engine import load_library

    T = load_library().bk_conv128_x3_tile_boards(N)
    tiles = (G + T - 1) // T
    flop = 2.0 * tiles * 400 * 128 * 1152 * 3
    c = stages["conv128_x3"]
    c["executed_mfma_gflop"] = flop / 1e9
    c["executed_mfma_tflops"] = flop / (c["ms_per_batch"] * 1e-3) / 1e12
    c["useful_fp32_conv_gflop"] = 2.0 * G * N * N * 128 * 1152 / 1e9
    c["activation_mb"] = 2.0 * G * N * N * 128 * 4 / 1e6
    whole["x3_over_torch_time"] = whole["x3"]["ms_per_batch"] / whole["torch"]["ms_per_batch"]
    whole["fused_over_x3_time"] = whole["fused"]["ms_per_batch"] / whole["x3"]["ms_per_batch"]
    whole["fused_states_over_x3_time"] = whole["fused-states"]["ms_per_batch"] / whole["x3"]["ms_per_batch"]
    return {"board": f"{N}x{N}, {P} players, A = {eng.A}", "games": G, "batches_per_graph": INNER,
            "replays_per_round": replays, "leaf_batch": whole, "x3_stages": stages}


if opt.trace:
    N, P = (20, 4) if opt.board == 20 else (7, 2)
    eng, net, obs, states = setup(N, P)
    if opt.trace == "x3":
        model, x = LeafDCNNet(net, normalize=False, features=True).eval(), obs
    elif opt.trace == "fused":
        model, x = LeafDCNNet(net, normalize=False, features=True, fused=True).eval(), obs
    elif opt.trace == "fused-states":
        model, x = LeafDCNNet(net, normalize=False, features=True, fused=True).eval().forward_states, states
    else:
        model, x = net.to(memory_format=torch.channels_last), obs.contiguous(memory_format=torch.channels_last)
    reps = 4 if opt.quick else 30
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.inference_mode():
        for _ in range(3):
            model(x)
        e0.record()
        for _ in range(reps):
            model(x)
        e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"traced": opt.trace, "board": N, "games": G, "eager_batches": reps,
                      "ms_per_eager_batch": e0.elapsed_time(e1) / reps}))
    sys.exit(0)

res = {"tool": "tools/dcnn_leaf_bench.py", "device": torch.cuda.get_device_name(0),
       "20x20": board(20, 4), "7x7": board(7, 2)}
txt = json.dumps(res, indent=1)
print(txt)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w", encoding="utf-8") as f:
        f.write(txt + "\n")
