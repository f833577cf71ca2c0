#!/usr/bin/env python3
"""Rates of the rollout with and without external pushes (BatchedOSC.set_pushes -> irlosc_set_pushes), k12_admit float64 with a
sensor feed: the variants alternate in one process, from the same start states, best of --reps each.
    python tools/push_rates.py [--batch 65536] [--ticks 200] [--reps 3] [--variants plain,pushes] [--root DIR] [--json out.json]
"pushes": one applied-and-sensed push per arm, a wrench per robot (forces N(0, 20 N), torques N(0, 2 N m)), active on every timed
tick -- both extra launches on every tick.  --root DIR times another checkout of the project with this tool (the parent commit, which
has no pushes: --variants plain).  The start states are those of tools/rollout_rates.py (random_state, seed 5).
Prints one line per variant and, last, a JSON line with the rates in robot-ticks/s and the spread of each variant's repetitions."""
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
ap.add_argument("--variants", default="plain,pushes")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None)
a = ap.parse_args()
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
rng = np.random.default_rng(8)
wrench = np.concatenate([rng.normal(0.0, 20.0, (B, 2, 3)), rng.normal(0.0, 2.0, (B, 2, 3))], axis=2)
pushes = [dict(dev="ur5right", window=(0, 1 << 30)), dict(dev="ur5left", window=(0, 1 << 30))]
osc.set_plant(1e-3, 0.0)
print(osc.from_q_name, flush=True)
osc.upload_q(q, qd)
osc.set_targets(arr["tgt_pose"])
osc.set_sensordata(sens)
osc.rollout(8)                                             # warm-up (exchange buffer, lane records)
times = {v: [] for v in variants}
u, fl = np.empty((B, lay.n)), np.empty(B, np.uint32)
for _ in range(a.reps):
    for variant in variants:
        osc.upload_q(q, qd)
        if variant == "pushes":
            osc.set_pushes(pushes, wrench)                 # (tick base 0: every timed tick applies, every one but the first senses)
        elif hasattr(osc, "clear_pushes"):
            osc.clear_pushes()
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, a.ticks, 0, None, _lib.ptr(u), _lib.ptr(fl)))
        times[variant].append(time.perf_counter() - t0)
osc.close()
out = dict(batch=B, ticks=a.ticks, root=os.path.abspath(a.root))
for variant, ts in times.items():
    t = min(ts)
    out[f"rollout_{variant}"] = B * a.ticks / t
    out[f"us_per_tick_{variant}"] = [x / a.ticks * 1e6 for x in ts]
    print(f"rollout, {variant:6s}: {t / a.ticks * 1e6:8.1f} us per tick (best of {len(ts)}; all: "
          f"{' '.join(f'{x / a.ticks * 1e6:.1f}' for x in ts)}), {B * a.ticks / t / 1e6:7.1f} M robot-ticks/s", flush=True)
print(json.dumps(out))
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
