"""Times one arena match on the eager path and on the graph path (BatchedArena path="eager" /
"graph"), for two shapes, interleaved so both paths see the same clocks:

  coach  20x20, 4 players, ResNet-5x64: the new net against 3 seats of the old one, 24 games,
         permute, 50 simulations a move (AlphaZeroTrainer.arena_compare's default shape)
  7x7    7x7, 2 players, two ResNet-5x64, x3_boards="all", 64 games, permute, 50 simulations

    python tools/arena_bench.py --rounds 3 --out profiles/arena_graph_bench.json
    python tools/arena_bench.py --shape coach --path graph --rounds 1      # one match, e.g. under a profiler

Each timed match is a whole play() — trees, evaluators and, on the graph path, the capture
included — between device synchronisations. The raw seconds of every round are written out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from blokus_rl_amd.engine import W_PLY  # noqa: E402

SHAPES = {
    "coach": dict(n=20, p=4, games=24, sims=50, blocks=5, x3_boards=None),
    "7x7": dict(n=7, p=2, games=64, sims=50, blocks=5, x3_boards="all"),
}


def make_arena(shape, path, sims=None, games=None):
    from blokus_rl_amd.alphazero.batched_arena import ArenaSeat, BatchedArena
    from blokus_rl_amd.engine import Engine
    from blokus_rl_amd.nets import ResNet

    s = SHAPES[shape]
    eng = Engine(s["n"], s["p"], 5)
    torch.manual_seed(1)
    new = ResNet(s["n"], s["p"], eng.A, s["blocks"]).to(eng.device).eval()
    torch.manual_seed(2)
    old = ResNet(s["n"], s["p"], eng.A, s["blocks"]).to(eng.device).eval()
    k = sims or s["sims"]
    seats = [ArenaSeat(new, k)] + [ArenaSeat(old, k) for _ in range(s["p"] - 1)]
    return BatchedArena(eng, seats, cpuct=1.0, path=path, x3_boards=s["x3_boards"]), games or s["games"]


def one_match(shape, path, sims=None, games=None):
    arena, g = make_arena(shape, path, sims, games)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    total, per_game, states = arena.play(g, permute=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if arena.path_used != path:
        raise SystemExit(f"{shape}: asked for {path}, played {arena.path_used}: {arena.path_reason}")
    plies = int(states.view(torch.int32)[:, W_PLY].max())
    return dt, plies, total.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
    ap.add_argument("--path", choices=["eager", "graph", "both"], default="both")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sims", type=int, default=None)
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = list(SHAPES) if a.shape == "all" else [a.shape]
    paths = ["eager", "graph"] if a.path == "both" else [a.path]
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": {}}
    for sh in shapes:
        r = {p: [] for p in paths}
        info = {}
        for _ in range(a.rounds):  # interleaved: eager, graph, eager, graph, ...
            for p in paths:
                dt, plies, total = one_match(sh, p, a.sims, a.games)
                r[p].append(dt)
                info[p] = {"max_plies": plies, "scores": total}
                print(f"{sh} {p}: {dt:.3f} s ({plies} plies)", flush=True)
        cfg = dict(SHAPES[sh], sims=a.sims or SHAPES[sh]["sims"], games=a.games or SHAPES[sh]["games"])
        entry = {"config": cfg, "seconds": r, "last_match": info}
        if len(paths) == 2:
            entry["median_speedup_graph_vs_eager"] = sorted(r["eager"])[len(r["eager"]) // 2] / sorted(r["graph"])[
                len(r["graph"]) // 2]
        res["shapes"][sh] = entry
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
