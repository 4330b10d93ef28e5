"""Overlap of the leaf steps with the leaf nets in a rocprofv3 kernel trace of
`BK_SIM_GROUPS=K python bench.py --steps S --warmup W` (SelfPlay.sim_groups): the two
kernels' average durations over the timed window, how much of the steps' time lies inside some
net launch's interval, and the window's span against the sum of its launches (equal when the
launches ran one after another). With K groups a ply has K x sims launches of each kernel.
usage: python tools/sim_groups_trace.py <kernel_trace.csv> <out.json> <warmup> <steps> <sims> <groups>"""
import csv
import json
import sys

trace, out = sys.argv[1], sys.argv[2]
W, S, sims, K = (int(v) for v in sys.argv[3:7])
net, step, queues = [], [], set()
with open(trace, newline="") as f:
    for r in csv.DictReader(f):
        name = r["Kernel_Name"]
        iv = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
        if "k_leaf_step_ov" in name:
            step.append(iv)
            queues.add(r.get("Queue_Id"))
        elif "k_leafnet_x3" in name:
            net.append(iv)
            queues.add(r.get("Queue_Id"))
step.sort()
net.sort()
per_ply = K * sims
assert len(step) >= (W + S) * per_ply, (len(step), per_ply)
step = step[-S * per_ply:]  # the timed window: the run's last S plies
t_lo, t_hi = step[0][0], step[-1][1]
net = [iv for iv in net if iv[1] > t_lo and iv[0] < t_hi]
# the part of every step interval covered by the union of the net intervals
covered, j = 0, 0
merged = []
for b, e in net:
    if merged and b <= merged[-1][1]:
        merged[-1][1] = max(merged[-1][1], e)
    else:
        merged.append([b, e])
for b, e in step:
    while j < len(merged) and merged[j][1] <= b:
        j += 1
    i = j
    while i < len(merged) and merged[i][0] < e:
        covered += max(0, min(e, merged[i][1]) - max(b, merged[i][0]))
        i += 1
step_total = sum(e - b for b, e in step)
net_total = sum(e - b for b, e in net)
doc = {"groups": K, "warmup": W, "steps": S, "sims": sims, "window_span_ms": (t_hi - t_lo) / 1e6,
       "k_leaf_step_ov": {"window_dispatches": len(step), "window_avg_us": step_total / len(step) / 1e3},
       "k_leafnet_x3": {"window_dispatches": len(net), "window_avg_us": net_total / len(net) / 1e3},
       "launch_sum_ms": (step_total + net_total) / 1e6,
       "step_time_inside_a_net_fraction": covered / step_total, "queues": sorted(q for q in queues if q is not None)}
json.dump(doc, open(out, "w"), indent=1)
print(json.dumps(doc))
