#!/usr/bin/env python3
"""The closed loop of closed_loop_headless.py without the host in it: the same fleet, seeds, start / goal rule and plant, but every
tick stays on the GPU (BatchedOSC.rollout -> irlosc_rollout_from_q).

Per tick and robot (all B robots at once), one train of kernels and nothing across PCIe:
    (qpos, qvel) --walk--> M, J, bias, EE pose in the exchange buffer --OSC step--> u --plant--> (qpos, qvel) of the next tick
    plant: qacc = M^-1 (u - bias - damping qvel); semi-implicit Euler with dt = 1 ms                       (csrc/osc_plant.hpp)
Every joint is torque-driven, no contacts, no joint limits: the plant closed_loop_headless.py integrates in NumPy.  Any fleet size.

    python examples/closed_loop_resident_headless.py [--robots 4096] [--ticks 1500]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irl_control_amd import BatchedOSC, synth                       # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel               # noqa: E402


def scenario(robots, seed=0):
    """-> (q, q_goal): start and goal configurations, drawn exactly as closed_loop_headless.run draws them."""
    rng = np.random.default_rng(seed)
    q = np.zeros((robots, 25))
    q[:, 1:7] = rng.uniform(-1.0, 1.0, (robots, 6)) + np.array([0.0, -0.6, 1.2, 0.0, 0.8, 0.0])
    q[:, 13:19] = rng.uniform(-1.0, 1.0, (robots, 6)) + np.array([0.0, -0.6, 1.2, 0.0, 0.8, 0.0])
    q_goal = q.copy()
    q_goal[:, 1:7] += rng.uniform(-0.35, 0.35, (robots, 6))
    q_goal[:, 13:19] += rng.uniform(-0.35, 0.35, (robots, 6))
    q_goal[:, 0] += rng.uniform(-0.3, 0.3, robots)
    return q, q_goal


def run(robots=16, ticks=1500, seed=0, dt=1e-3, damping=0.0, verbose=True, trace_every=0, start=None, goal=None):
    """`start` / `goal` [robots, 25]: configurations to use instead of scenario(robots, seed)."""
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    model = RigidBodyModel.load("dual_ur5")
    osc = BatchedOSC(lay, robots, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    osc.set_plant(dt, damping)
    q, q_goal = scenario(robots, seed) if start is None else (np.array(start, dtype=np.float64), np.array(goal, dtype=np.float64))
    qd = np.zeros_like(q)

    def ee_pose(qq):
        osc.upload_q(qq, qd * 0.0)
        osc.frontend()
        return osc.download_records(keys=("ee_pose",))["ee_pose"].copy()

    tgt = ee_pose(q_goal)                                    # EE poses at the goal configuration = the targets
    err0 = np.linalg.norm(ee_pose(q)[:, :2, :3] - tgt[:, :2, :3], axis=2)      # the two arms
    osc.upload_q(q, qd)
    osc.set_targets(tgt)
    out = osc.rollout(ticks, trace_every=trace_every)
    # EE poses of the state the rollout left (what the host loop's last tick reports is the state BEFORE its last integration: one
    # tick earlier than this)
    final = np.linalg.norm(ee_pose(out["qpos"])[:, :2, :3] - tgt[:, :2, :3], axis=2)
    hist = None
    if out["ee_trace"] is not None:
        hist = np.linalg.norm(out["ee_trace"][:, :, :2, :3] - tgt[None, :, :2, :3], axis=3).max(axis=(1, 2))
    osc.close()
    if verbose:
        print(f"{robots} robots, {ticks} ticks: EE position error {err0.mean():.3f} m (max {err0.max():.3f}) -> "
              f"{np.nanmean(final):.4f} m (max {np.nanmax(final):.4f})")
    return dict(err0=err0, err=final, hist=hist, q=out["qpos"], qd=out["qvel"], flags_any=out["flags_any"], ee_trace=out["ee_trace"], tgt=tgt)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=1500)
    a = ap.parse_args()
    run(a.robots, a.ticks)
