#!/usr/bin/env python3
"""Rates of the closed loop on the GPU (BatchedOSC.rollout -> irlosc_rollout_from_q), float64:
    (a) ticks/s of rollout(--ticks), trace_every = 0 and = 10
    (b) irlosc_step_from_q_device once per call on resident caller buffers in the same process (one step per call, no plant)
    (c) with --host-loop: the host loop of examples/closed_loop_headless.py (dense records + NumPy) on the same fleet size, k13
    python tools/rollout_rates.py [--batch 65536] [--layout k13|k12_admit] [--ticks 200] [--reps 3] [--host-loop] [--json out.json]
Prints one line per leg and, last, a JSON line with every rate in robot-ticks/s (best of --reps).  The plant kernel's own duration:
run this script under `rocprofv3 --kernel-trace --stats -- python tools/rollout_rates.py ...` and read osc_plant_lane_kernel's row."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from irl_control_amd import BatchedOSC, synth                      # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--layout", default="k13")
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-loop", action="store_true")
ap.add_argument("--host-ticks", type=int, default=20)
ap.add_argument("--json", default=None)
a = ap.parse_args()
B, NS = a.batch, 18
feed = a.layout == "k12_admit"
lay = synth.make_layout(a.layout)
model = RigidBodyModel.load("dual_ur5")
rng = np.random.default_rng(5)
osc = BatchedOSC(lay, B, dtype=np.float64)
osc.set_model(model)
_, gains, arr = synth.make_batch(a.layout, B, seed=7)
osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
q, qd = model.random_state(rng, B)
qd *= 0.0
osc.upload_q(q, qd)
osc.set_targets(arr["tgt_pose"])
if feed:
    osc.set_ft_sensors()
    osc.set_sensordata(rng.normal(0.0, 5.0, size=(B, NS)))
osc.set_plant(1e-3, 0.0)
print(osc.from_q_name, flush=True)
out = dict(batch=B, layout=a.layout, ticks=a.ticks)
osc.rollout(8)                                             # warm-up (exchange buffer, lane records)
for every in (0, 10):
    best = 1e30
    for _ in range(a.reps):
        osc.upload_q(q, qd)
        tr = np.empty((-(-a.ticks // every), B, lay.ndev, 7)) if every else None
        u, fl = np.empty((B, lay.n)), np.empty(B, np.uint32)
        from irl_control_amd import _lib
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, a.ticks, every, _lib.ptr(tr), _lib.ptr(u), _lib.ptr(fl)))
        best = min(best, time.perf_counter() - t0)
    out[f"rollout_trace{every}"] = B * a.ticks / best
    print(f"(a) rollout, trace_every={every:2d}: {best / a.ticks * 1e6:8.1f} us per tick, {B * a.ticks / best / 1e6:7.1f} M robot-ticks/s", flush=True)

from conftest import HipBuffers                                    # noqa: E402
hb = HipBuffers()
d_q, d_v, d_t = hb.to_device(q), hb.to_device(qd), hb.to_device(arr["tgt_pose"])
d_s = hb.to_device(rng.normal(0.0, 5.0, size=(B, NS))) if feed else None
d_u, d_f = hb.alloc(B * lay.n * 8), hb.alloc(B * 4)
for _ in range(8):
    osc.step_from_q_device(B, d_q, d_v, d_t, d_u, d_f, d_sensordata=d_s)
osc.sync()
best = 1e30
for _ in range(a.reps):
    t0 = time.perf_counter()
    for _ in range(a.ticks):
        osc.step_from_q_device(B, d_q, d_v, d_t, d_u, d_f, d_sensordata=d_s)
    osc.sync()
    best = min(best, time.perf_counter() - t0)
hb.free()
out["step_from_q_device"] = B * a.ticks / best
print(f"(b) step_from_q_device, one step per call: {best / a.ticks * 1e6:8.1f} us per step, {B * a.ticks / best / 1e6:7.1f} M steps/s", flush=True)
osc.close()

if a.host_loop:
    from test_rollout import ee_poses, host_loop                   # noqa: E402
    tgt = ee_poses(q)
    t0 = time.perf_counter()
    host_loop(q, tgt, a.host_ticks)
    dt = time.perf_counter() - t0
    out["host_loop"] = B * a.host_ticks / dt
    print(f"(c) host loop of closed_loop_headless.py: {dt / a.host_ticks * 1e3:8.2f} ms per tick, {B * a.host_ticks / dt / 1e6:7.3f} M robot-ticks/s", flush=True)
print(json.dumps(out))
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
