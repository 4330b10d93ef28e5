"""bench.py's plain run and its --dump-outputs: the plain line carries the headline fields and
nothing that takes a run of its own; the dumped arrays are the last timed ply's outputs, float32,
the same from run to run; the legal workload's dumped mask words restate the bitmasks exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_legal_outputs_words_restate_the_masks():
    import bench

    g = torch.Generator().manual_seed(3)
    masks = torch.randint(-2**63, 2**63 - 1, (40, 7), dtype=torch.int64, generator=g)
    counts = torch.arange(40, dtype=torch.int32)
    out = bench.legal_outputs(masks, counts, rows=16)
    rows = out["mask_rows"].numpy()
    assert len(rows) == 16 and len(set(rows.tolist())) == 16 and (np.diff(rows) > 0).all()
    assert (rows == bench.legal_outputs(masks, counts, rows=16)["mask_rows"].numpy()).all()  # a fixed sample
    w = out["mask_words16"].numpy().astype(np.float32).astype(np.uint64).reshape(16, 7, 4)  # as dump_outputs stores
    back = w[..., 0] | (w[..., 1] << np.uint64(16)) | (w[..., 2] << np.uint64(32)) | (w[..., 3] << np.uint64(48))
    assert (back == masks.numpy().view(np.uint64)[rows]).all()
    assert out["counts"] is counts


def test_dump_outputs_rejected_for_other_workloads():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "dry", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr


def _plain_run(tmp, extra=()):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BK_DIST_BACKEND")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--games", "16", "--sims", "4", "--dump-outputs", str(tmp)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp))}


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    out, a = _plain_run(tmp_path / "a")
    assert out["unit"] == "sims/s" and out["higher_is_better"] is True and out["steps"] == 2 and out["warmup"] == 1
    assert out["metric"].startswith("MCTS sims/sec") and "fp32 net" in out["dtype"]
    # value = the window's simulations over its time; ms_per_step = that time per timed ply
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 * 2 - 16 * 4 * 2) < 1e-6 * 16 * 4 * 2 + 1
    for key in ("roofline", "search_roofline", "tower_roofline", "late_game", "cpu_baseline", "net_math_f32",
                "uninformed_mcts", "legal_move", "ppo_vector_env", "learner", "config1_7x7", "ppo_update"):
        assert key not in out, key
    assert out["stage_ms_per_sim_step"] == {}  # no stage-timed ply
    assert set(a) == {"roots", "ids", "pi", "k", "player", "game_id", "acted", "action", "next_roots"}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["roots"].shape == (16, 384) and a["next_roots"].shape == (16, 384) and a["pi"].shape == a["ids"].shape
    k = a["k"].astype(int)
    assert (a["acted"] == 1).all() and (k > 0).all()  # ply 3 of 16 games: every game moves
    col = np.arange(a["ids"].shape[1])[None]
    assert ((a["ids"] >= 0) == (col < k[:, None])).all() and (a["pi"][col >= k[:, None]] == 0).all()
    assert np.allclose(a["pi"].sum(1), 1.0, atol=1e-5)
    # the sampled action is one of the root's legal ids with visits behind it
    hit = (a["ids"] == a["action"][:, None]) & (a["pi"] > 0)
    assert (hit.sum(1) == 1).all()
    assert (a["roots"] != a["next_roots"]).any(1).all()
    # same arguments, same inputs: a second run writes the same arrays
    _, b = _plain_run(tmp_path / "b")
    for name in a:
        assert np.array_equal(a[name], b[name]), name
