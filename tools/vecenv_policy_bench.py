"""Times one PPO rollout step without the agent's forward pass on the big 2-player boards (14x14/5 and
20x20/5, 1024 envs, fixed seeded logits [E, A] f32 resident in HBM), three ways:

  a  the trainer's torch path: Categorical(logits=FilterLegalMoves(logits, mask_words)) sample +
     log_prob, then env.step, launched eagerly (what PPOTrainer does where `policy_kernels` is False);
  b  sample_policy + step_raw (k_vec_policy_wave, k_vec_step), replayed from a HIP graph;
  c  the fused step_policy (k_vec_step<policy>), replayed from a HIP graph
     (b and c on BlokusVectorEnv(policy_draw="all"));
  d  for scale only: step_raw(None), the env step with the in-kernel uniform agent (no logits), from a
     HIP graph — other games than a-c play, so only its order of magnitude compares.

    python tools/vecenv_policy_bench.py [--out profiles/vecenv_policy_all_bench.json]

Every path plays its own env from the same reset; the games run on through the windows (an episode is
12-21 agent steps, so the envs spread over all game phases during the warm-up). The paths take turns
window by window; a window is `--steps` steps between two stream events ending in a synchronise, and
the figure of a path is the median of its windows' per-step times. Run one process at a time on the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from blokus_rl_amd.ppo.agent import FilterLegalMoves  # noqa: E402
from blokus_rl_amd.vector_env import BlokusVectorEnv  # noqa: E402

PER_GRAPH = 10  # steps per captured graph


def clocks_note() -> str:
    """The box's clocks as rocm-smi shows them (read only); the run goes on without them."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30)
        lines = [ln.strip() for ln in r.stdout.splitlines() if "clk" in ln.lower()]
        return "; ".join(lines) if lines else "not available"
    except (OSError, subprocess.SubprocessError):
        return "not available"


def window_ms(fn, calls: int, steps: int) -> float:
    """Milliseconds per step of `calls` fn() calls (steps env steps in all) between two stream events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bench_board(N: int, cells: int, E: int, steps: int, windows: int, warm: int) -> dict:
    envs = {"a": BlokusVectorEnv(E, N, cells), "b": BlokusVectorEnv(E, N, cells, policy_draw="all"),
            "c": BlokusVectorEnv(E, N, cells, policy_draw="all"), "d": BlokusVectorEnv(E, N, cells)}
    dev = envs["a"].device
    A = envs["a"].eng.A
    logits = (torch.randn((E, A), device=dev, generator=torch.Generator(dev).manual_seed(N)) * 2.0).contiguous()
    for env in envs.values():
        env.reset(seed=0)
    filt = FilterLegalMoves()
    torch.manual_seed(0)

    def torch_step():
        env = envs["a"]
        with torch.inference_mode():
            dist = torch.distributions.Categorical(logits=filt(logits, env.mask_words))
            a = dist.sample()
            dist.log_prob(a)
        env.step(a)

    gb, gc, gd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gd):
        for _ in range(PER_GRAPH):
            envs["d"].step_raw(None)
    with torch.cuda.graph(gb):
        for _ in range(PER_GRAPH):
            envs["b"].step_policy(logits, fused=False)
    with torch.cuda.graph(gc):
        for _ in range(PER_GRAPH):
            envs["c"].step_policy(logits)
    reps = max(1, steps // PER_GRAPH)
    run = {"a": lambda: window_ms(torch_step, reps * PER_GRAPH, reps * PER_GRAPH),
           "b": lambda: window_ms(gb.replay, reps, reps * PER_GRAPH),
           "c": lambda: window_ms(gc.replay, reps, reps * PER_GRAPH),
           "d": lambda: window_ms(gd.replay, reps, reps * PER_GRAPH)}
    for _ in range(max(1, warm // (reps * PER_GRAPH))):
        for k in "abcd":
            run[k]()
    # b and c are the same law on the same streams: they must have walked the same games
    same = all(torch.equal(getattr(envs["b"], n), getattr(envs["c"], n)) for n in ("states", "rng", "mask_words"))
    if not same:
        raise RuntimeError("the fused step and the two launches diverged")
    ms = {k: [] for k in "abcd"}
    for _ in range(windows):
        for k in "abcd":  # the paths take turns
            ms[k].append(run[k]())
    med = {k: statistics.median(v) for k, v in ms.items()}
    names = {"a": "torch_filter_categorical_plus_step_eager", "b": "sample_policy_plus_step_raw_graph",
             "c": "fused_step_policy_graph", "d": "uniform_agent_step_raw_graph"}
    out = {"board": f"{N}x{N}/{cells}", "action_ids": A, "envs": E, "steps_per_window": reps * PER_GRAPH,
           "windows": windows, "legal_ids_per_env": {k: float(envs[k].valid_mask().sum()) / E for k in "abcd"}}
    for k in "abcd":
        out[names[k]] = {"ms_per_step_median": med[k], "ms_per_step_min": min(ms[k]), "ms_per_step_max": max(ms[k]),
                         "env_steps_per_s": E / (med[k] * 1e-3), "ms_per_step_windows": ms[k]}
    out["a_over_c"] = med["a"] / med["c"]
    out["b_over_c"] = med["b"] / med["c"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecenv_policy_all_bench.json"))
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2000, help="env steps per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2000, help="env steps per path before the first window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vecenv_policy_bench needs a HIP device")
    res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "clocks_idle_before": clocks_note(),
           "timing": "stream events around a window ending in a synchronise; per-step median over the windows, "
                     "paths alternating window by window",
           "boards": []}
    for N, cells in ((14, 5), (20, 5)):
        r = bench_board(N, cells, args.envs, args.steps, args.windows, args.warmup)
        res["boards"].append(r)
        line = {k: v for k, v in r.items() if not isinstance(v, dict)}
        line.update({k: v["ms_per_step_median"] for k, v in r.items()
                     if isinstance(v, dict) and "ms_per_step_median" in v})
        print(json.dumps(line), flush=True)
    res["clocks_after_last_window"] = clocks_note()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
