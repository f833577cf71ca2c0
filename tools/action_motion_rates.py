#!/usr/bin/env python3
"""Rates of a rollout whose action list has a MOTION (BatchedOSC.set_action_motion: INTERP moves, seeded target noise) against the same
rollout with the plain list, float64, k13, same process and fleet, the legs alternating:
    python tools/action_motion_rates.py [--batch 65536] [--ticks 200] [--reps 5] [--json out.json]
The list and the fleet are tools/action_list_rates.py's.  Legs:
    list          the plain list: the action kernel as it was
    still         a motion with steps 0 and no noise: the MOTION kernel doing a list's work (the cost of its extra state)
    interp        INTERP on every WP with steps = --ticks: every robot interpolates and every wave stores its target tile on every tick
    interp+noise  the same with noise on every WP (drawn once per robot, on the entry tick)
A leg is rollout(--ticks) from the same start state (state reset by set_action_list / set_action_motion), wall clock around the
library call.  Prints every repetition, then per leg median, best and worst, and a JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from irl_control_amd import BatchedOSC, _lib, synth                # noqa: E402
from irl_control_amd import action_sequence as aseq                # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()
B = a.batch
lay = synth.make_layout("k13")
model = RigidBodyModel.load("dual_ur5")
rng = np.random.default_rng(5)
osc = BatchedOSC(lay, B, dtype=np.float64)
osc.set_model(model)
_, gains, arr = synth.make_batch("k13", B, seed=7)
osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
q, qd = model.random_state(rng, B)
qd *= 0.0
osc.set_plant(1e-3, 0.0)
ia, io = lay.dev_names.index("ur5right"), lay.dev_names.index("ur5left")
A = 4
pose = np.repeat(arr["tgt_pose"][:, ia][:, None], A, axis=1)
desc = dict(n_actions=A, active_dev=ia, passive_dev=io, passive_hold_orientation=1, passive_quat=np.array(aseq.DEFAULT_EE_QUAT),
            kind=np.array([0, 1, 0, 0], np.int32), xyz_from_start=np.array([0, 0, 0, 1], np.int32), grip_ticks=np.array([1, 20, 1, 1], np.int32),
            kp=np.full(A, 6.0), max_error=np.full(A, 0.02), min_speed=np.full(A, 0.1), max_speed=np.full(A, 3.0),
            gripper_force=np.array([0.0, 0.2, 0.0, -0.08]), pose=pose)
N = a.ticks
LEGS = {"list": None, "still": dict(steps=[0, 0, 0, 0]), "interp": dict(steps=[N, 0, N, N]),
        "interp+noise": dict(steps=[N, 0, N, N], noise_std=[0.002, 0.0, 0.002, 0.002], seed=1)}
print(osc.from_q_name, flush=True)


def leg(name):
    osc.upload_q(q, qd)
    osc.set_targets(arr["tgt_pose"])
    osc.set_action_list(desc)
    if LEGS[name] is not None:
        osc.set_action_motion(**LEGS[name])
    u, fl = np.empty((B, lay.n)), np.empty(B, np.uint32)
    t0 = time.perf_counter()
    osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, a.ticks, 0, None, _lib.ptr(u), _lib.ptr(fl)))
    return time.perf_counter() - t0


for name in LEGS:                                          # warm-up (exchange buffer, lane records, the list's and the motion's buffers)
    leg(name)
times = {name: [] for name in LEGS}
for r in range(a.reps):
    for name in LEGS:
        dt = leg(name)
        times[name].append(dt)
        print(f"rep {r} {name:13s}: {dt / a.ticks * 1e6:8.1f} us per tick", flush=True)
st, ms = osc.action_state(), osc.action_motion_state()
out = dict(batch=B, ticks=a.ticks, reps=a.reps, actions_reached=[int(st["action"].min()), int(st["action"].max())],
           steps_reached=[int(ms["step"].min()), int(ms["step"].max())], draws=[int(ms["draws"].min()), int(ms["draws"].max())])
for name in LEGS:
    t = np.array(times[name]) / a.ticks * 1e6
    out[name] = dict(us_per_tick_median=float(np.median(t)), us_per_tick_best=float(t.min()), us_per_tick_worst=float(t.max()),
                     robot_ticks_per_s_median=float(B / np.median(t) * 1e6))
    print(f"{name}: median {np.median(t):.1f} us per tick (best {t.min():.1f}, worst {t.max():.1f}), {B / np.median(t):.1f} M robot-ticks/s")
osc.close()
print(json.dumps(out))
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
