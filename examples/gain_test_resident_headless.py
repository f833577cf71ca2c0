#!/usr/bin/env python3
"""The waypoint demo of gain_test / figure8 (headless_loops.gain_test_loop) on a resident fleet: B robots walk the demo's path and
every tick stays on the GPU -- the targets are cycled there too (BatchedOSC.set_waypoints -> irlosc_set_waypoints).

Per tick and robot, one train of kernels and nothing across PCIe:
    (qpos, qvel) --walk--> M, J, bias, EE pose --OSC step--> u --cycler--> targets of the next tick --plant--> (qpos, qvel)
    cycler: an arm within THRESHOLD_EE of its target moves on to its next waypoint and wraps at the end   (csrc/osc_waypoint.hpp)
The base has no list and keeps its target.  The plant is closed_loop_resident_headless.py's: every joint torque-driven, no contacts,
no joint limits; whether it reaches the demo's waypoints from these start states is reported, not promised.

    python examples/gain_test_resident_headless.py [--robots 4096] [--ticks 4000] [--path gain_test|figure8]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from headless_loops import THRESHOLD_EE, figure_eight_waypoints, gain_test_waypoints      # noqa: E402
from irl_control_amd import BatchedOSC, synth                       # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel               # noqa: E402


def start_states(robots, seed=0):
    """Start configurations: a bent-arm pose of both arms, +- 0.15 rad per robot on the arm joints."""
    rng = np.random.default_rng(seed)
    q = np.zeros((robots, 25))
    q[:, 1:7] = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3]) + rng.uniform(-0.15, 0.15, (robots, 6))
    q[:, 13:19] = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2]) + rng.uniform(-0.15, 0.15, (robots, 6))
    return q


def run(robots=16, ticks=4000, path="gain_test", seed=0, dt=1e-3, damping=0.0, verbose=True):
    right, left = gain_test_waypoints() if path == "gain_test" else figure_eight_waypoints()
    lay = synth.make_layout("k13")                           # devices: ur5right, ur5left, base
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    osc = BatchedOSC(lay, robots, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(dt, damping)
    q = start_states(robots, seed)
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    tgt = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()      # orientations and the base: held where they start
    osc.set_targets(tgt)
    osc.set_waypoints([right, left, None], THRESHOLD_EE, loop=True)
    out = osc.rollout(ticks)
    st = osc.waypoint_state()
    osc.close()
    W = np.array([len(right), len(left)])
    arrivals = st["arrivals"][:, :2].astype(np.int64)
    laps = arrivals // W
    frozen = out["flags_any"] & (64 | 1) != 0                # IRLOSC_FLAG_NONFINITE | IRLOSC_FLAG_M_NOT_PD
    if verbose:
        print(f"{robots} robots, {ticks} ticks of {dt * 1e3:g} ms on the {path} path ({W[0]} / {W[1]} waypoints, threshold {THRESHOLD_EE} m)")
        for d, name in enumerate(("ur5right", "ur5left")):
            a = arrivals[:, d]
            print(f"  {name}: laps min {laps[:, d].min()} median {np.median(laps[:, d]):g} max {laps[:, d].max()}; arrivals min {a.min()} "
                  f"median {np.median(a):g} max {a.max()}; robots that never arrived {int((a == 0).sum())}; last arrival at tick "
                  f"{int(st['last_tick'][:, d].max())} at the latest")
        print(f"  robots frozen by the plant at some tick: {int(frozen.sum())}")
    return dict(arrivals=arrivals, laps=laps, index=st["index"], last_tick=st["last_tick"], q=out["qpos"], flags_any=out["flags_any"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=4000)
    ap.add_argument("--path", choices=("gain_test", "figure8"), default="gain_test")
    a = ap.parse_args()
    run(a.robots, a.ticks, a.path)
