#!/usr/bin/env python3
"""Rates of the rollout with and without waypoint paths (BatchedOSC.set_waypoints -> irlosc_set_waypoints), k13 float64: the two
variants alternate in one process, from the same start states, best of --reps each.
    python tools/waypoint_rates.py [--batch 65536] [--ticks 200] [--reps 3] [--path figure8|gain_test] [--json out.json]
The start states are those of tools/rollout_rates.py (random_state, seed 5), so the figure without paths is that tool's leg (a).
Prints one line per variant and, last, a JSON line with the rates in robot-ticks/s and the arrivals the paths saw."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "examples")]
from headless_loops import THRESHOLD_EE, figure_eight_waypoints, gain_test_waypoints      # noqa: E402
from irl_control_amd import BatchedOSC, _lib, synth                # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--path", choices=("figure8", "gain_test"), default="figure8")
ap.add_argument("--json", default=None)
a = ap.parse_args()
B = a.batch
lay = synth.make_layout("k13")
model = RigidBodyModel.load("dual_ur5")
osc = BatchedOSC(lay, B, dtype=np.float64)
osc.set_model(model)
_, gains, arr = synth.make_batch("k13", B, seed=7)
osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
q, qd = model.random_state(np.random.default_rng(5), B)
qd *= 0.0
osc.set_plant(1e-3, 0.0)
right, left = figure_eight_waypoints() if a.path == "figure8" else gain_test_waypoints()
print(osc.from_q_name, flush=True)
osc.upload_q(q, qd)
osc.set_targets(arr["tgt_pose"])
osc.rollout(8)                                             # warm-up (exchange buffer, lane records)
best = dict(plain=1e30, paths=1e30)
arrivals = 0
u, fl = np.empty((B, lay.n)), np.empty(B, np.uint32)
for _ in range(a.reps):
    for variant in ("plain", "paths"):
        osc.upload_q(q, qd)
        osc.set_targets(arr["tgt_pose"])                   # (clears the paths of the previous leg)
        if variant == "paths":
            osc.set_waypoints([right, left, None], THRESHOLD_EE, loop=True)
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, a.ticks, 0, None, _lib.ptr(u), _lib.ptr(fl)))
        best[variant] = min(best[variant], time.perf_counter() - t0)
        if variant == "paths":
            arrivals = int(osc.waypoint_state()["arrivals"].sum())
osc.close()
out = dict(batch=B, ticks=a.ticks, path=a.path, arrivals=arrivals)
for variant, t in best.items():
    out[f"rollout_{variant}"] = B * a.ticks / t
    print(f"rollout, {variant:5s}: {t / a.ticks * 1e6:8.1f} us per tick, {B * a.ticks / t / 1e6:7.1f} M robot-ticks/s", flush=True)
print(json.dumps(out))
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
