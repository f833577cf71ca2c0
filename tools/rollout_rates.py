#!/usr/bin/env python3
"""Rates of the closed loop on the GPU (BatchedOSC.rollout -> irlosc_rollout_from_q), float64:
    (a) ticks/s of rollout(--ticks), trace_every = 0 and = 10
    (b) irlosc_step_from_q_device once per call on resident caller buffers in the same process (one step per call, no plant)
    (c) with --host-loop: the host loop of examples/closed_loop_headless.py (dense records + NumPy) on the same fleet size, k13
    (l) with --log: the episode log (irlosc_rollout_from_q_logged) on the same context, between (a) and (b): see log_legs()
    python tools/rollout_rates.py [--batch 65536] [--layout k13|k12_admit] [--ticks 200] [--reps 3] [--host-loop] [--log] [--json out.json]
Prints one line per leg and, last, a JSON line with every rate in robot-ticks/s (the log legs: us per tick), best of --reps.  A kernel's
own duration: run this script under `rocprofv3 --kernel-trace --stats -- python tools/rollout_rates.py ...` and read its row
(osc_plant_lane_kernel, osc_log_kernel)."""
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
ap.add_argument("--log", action="store_true", help="the episode-log legs (l), between (a) and (b)")
ap.add_argument("--log-ticks1", type=int, default=40, help="ticks of the all-channels, every-tick leg (89 MB of host buffer per tick at 65 536 robots)")
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


def log_legs():
    """(l) the episode log (rollout_logged -> irlosc_rollout_from_q_logged) in this process, on this context:
    EE_POSE alone at every = 10 on the slot as it is -- the EE trace's exact payload, next to leg (a)'s trace_every = 10;
    then the slot ARMED with everything the nine channels need (a sensor feed, force_test's wall on the left arm, the gripper scene's
    joint rows: more kernels per tick, so it gets an unlogged leg of its own): all channels at every = 1 / 10 / 50, a 256-robot subset
    every tick, and the loop callers had before -- rollout(1) with the downloads that yield the same channels -- per tick."""
    from irl_control_amd import _lib, joints, rollout_log

    def timed(ticks, lg, robots, host):
        best = 1e30
        u, fl = np.empty((B, lay.n)), np.empty(B, np.uint32)
        for _ in range(a.reps):
            osc.upload_q(q, qd)
            t0 = time.perf_counter()
            osc._chk(osc.lib.irlosc_rollout_from_q_logged(osc._h, 0, B, ticks, None if lg is None else _lib.C.byref(lg), _lib.ptr(robots),
                                                          _lib.ptr(host), _lib.ptr(u), _lib.ptr(fl)))
            best = min(best, time.perf_counter() - t0)
        return best / ticks * 1e6

    def leg(name, label, ticks, channels, every, robots=None):
        R = B if robots is None else len(robots)
        words = rollout_log.layout(lay.n, lay.ndev, channels, R)[1]
        host = buf[:-(-ticks // every) * words]
        us = timed(ticks, _lib.Log(channels, every, 0 if robots is None else R, 0, 0), robots, host)
        out[name] = us
        print(f"(l) {label}: {us:8.1f} us per tick ({words * 8 / 1e6:.2f} MB per sample, {words * 8 / every / us / 1e3:.2f} GB/s to the host)", flush=True)
        return us

    sub = np.linspace(0, B - 1, min(256, B)).round().astype(np.int32)
    all_words = rollout_log.layout(lay.n, lay.ndev, rollout_log.ALL, B)[1]
    t1 = min(a.ticks, a.log_ticks1)
    buf = np.zeros(max(t1, -(-a.ticks // 10)) * all_words)      # one host buffer for every leg, touched once
    out["log_none"] = timed(a.ticks, None, None, None)
    print(f"(l) the new entry point without a log: {out['log_none']:8.1f} us per tick", flush=True)
    leg("log_ee_every10", "EE_POSE, every = 10", a.ticks, _lib.LOG_EE_POSE, 10)
    leg("log_obs_act_sub256", "qpos qvel ee_pose targets u of 256 robots, every tick", a.ticks, 1 | 2 | 4 | 8 | 32, 1, sub)
    if not feed:
        osc.set_ft_sensors()
        osc.set_sensordata(rng.normal(0.0, 5.0, size=(B, NS)))
    osc.set_walls([dict(dev="ur5left", normal=(0.0, -1.0, 0.0), offset=-0.75, radius=0.1, stiffness=900.0, damping=20.0)])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    osc.set_joints(joints.scene_rows(os.path.join(root, "tests", "golden", "dual_ur5_joints.json"), 2.0, 0.004, 1.0, 0.002,
                                     devices=[d for d in lay.dev_names if d != "base"]))
    out["armed_unlogged"] = timed(a.ticks, None, None, None)
    print(f"(l) armed slot (feed, a wall, joint rows), no log: {out['armed_unlogged']:8.1f} us per tick", flush=True)
    leg("log_all_every1", f"all channels, every tick ({t1} ticks)", t1, rollout_log.ALL, 1)
    leg("log_all_every10", "all channels, every = 10", a.ticks, rollout_log.ALL, 10)
    leg("log_all_every50", "all channels, every = 50", a.ticks, rollout_log.ALL, 50)
    leg("log_all_sub256", "all channels of 256 robots, every tick", a.ticks, rollout_log.ALL, 1, sub)
    n1 = min(a.ticks, 20)
    best = 1e30
    for _ in range(a.reps):
        osc.upload_q(q, qd)
        t0 = time.perf_counter()
        for _ in range(n1):
            osc.download_q(); osc.download_targets()
            osc.rollout(1, trace_every=1)
            osc.wall_state(); osc.joint_state()
        best = min(best, time.perf_counter() - t0)
    out["one_tick_loop"] = best / n1 * 1e6
    print(f"(l) rollout(1) + download_q, download_targets, trace, wall_state, joint_state per tick ({n1} ticks): {best / n1 * 1e6:8.1f} us per tick", flush=True)


if a.log:
    log_legs()

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
