#!/usr/bin/env python3
"""Rates of the rollout with and without joint rows (BatchedOSC.set_joints -> irlosc_set_joints), k12_admit float64 with a sensor feed:
the variants alternate in one process, from the same start states, best of --reps each.
    python tools/joint_rates.py [--batch 65536] [--ticks 200] [--reps 3] [--variants plain,shared,per_robot] [--root DIR] [--json out.json]
"shared": the full 36-row scene set (joints.scene_rows: 24 stops, 10 couplings, 2 ACTION drives, idle without a list) with one table
for the fleet; "per_robot": the same rows with a stiffness per robot, so the table is per robot -- the one extra launch on every timed
tick.  --root DIR times another checkout of the project with this tool (the parent commit, which has no joint rows: --variants plain).
The start states are those of tools/rollout_rates.py (random_state, seed 5, at rest).
Prints one line per variant and, last, a JSON line with the rates in robot-ticks/s and every repetition's microseconds per tick."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--variants", default="plain,shared,per_robot")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None)
a = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(a.root))
from irl_control_amd import BatchedOSC, _lib, synth                # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel              # noqa: E402

B, NS = a.batch, 18
variants = a.variants.split(",")
lay = synth.make_layout("k12_admit")
model = RigidBodyModel.load("dual_ur5")
osc = BatchedOSC(lay, B, dtype=np.float64)
osc.set_model(model)
osc.set_ft_sensors(n_sensor=NS)
_, gains, arr = synth.make_batch("k12_admit", B, seed=7)
osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
q, qd = model.random_state(np.random.default_rng(5), B)
qd *= 0.0
sens = np.random.default_rng(6).normal(0.0, 5.0, size=(B, NS))
osc.set_plant(1e-3, 0.0)
print(osc.from_q_name, flush=True)
osc.upload_q(q, qd)
osc.set_targets(arr["tgt_pose"])
osc.set_sensordata(sens)
osc.rollout(8)                                             # warm-up (exchange buffer, lane records)
rows = {}
if set(variants) - {"plain"}:
    from irl_control_amd import joints                             # noqa: E402
    fixture = os.path.join(HERE, "tests", "golden", "dual_ur5_joints.json")
    rows["shared"] = joints.scene_rows(fixture, 2.0, 0.004, 1.0, 0.002)
    rows["per_robot"] = joints.scene_rows(fixture, np.random.default_rng(8).uniform(1.0, 3.0, B), 0.004, 1.0, 0.002)
times = {v: [] for v in variants}
active = {}
u, fl = np.empty((B, lay.n)), np.empty(B, np.uint32)
for _ in range(a.reps):
    for variant in variants:
        osc.upload_q(q, qd)
        if variant in rows:
            osc.set_joints(rows[variant])
        elif hasattr(osc, "clear_joints"):
            osc.clear_joints()
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, a.ticks, 0, None, _lib.ptr(u), _lib.ptr(fl)))
        times[variant].append(time.perf_counter() - t0)
        if variant in rows:
            active[variant] = float((osc.joint_state()["active_ticks"] > 0).mean())
osc.close()
out = dict(batch=B, ticks=a.ticks, root=os.path.abspath(a.root), rows_that_acted=active)
for variant, ts in times.items():
    t = min(ts)
    out[f"rollout_{variant}"] = B * a.ticks / t
    out[f"us_per_tick_{variant}"] = [x / a.ticks * 1e6 for x in ts]
    print(f"rollout, {variant:9s}: {t / a.ticks * 1e6:8.1f} us per tick (best of {len(ts)}; all: "
          f"{' '.join(f'{x / a.ticks * 1e6:.1f}' for x in ts)}), {B * a.ticks / t / 1e6:7.1f} M robot-ticks/s", flush=True)
print(json.dumps(out))
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
