#!/usr/bin/env python3
"""The push demo of admit_test (headless_loops.admit_test_loop) on a resident fleet: B robots under admittance control hold their
end effectors, a force pushes the left one during a window of ticks, and every tick stays on the GPU -- the push acts on the plant
there and the F/T wrench of the next tick carries its reaction (BatchedOSC.set_pushes -> irlosc_set_pushes).

Per tick and robot, one train of kernels and nothing across PCIe:
    (qpos, qvel) --walk--> M, J, bias, EE pose --feed's wrench - sensed push--> OSC step --> u --bias -= J^T push--> plant --> (qpos, qvel)
Layout k12_admit: both arms under admittance; the left arm carries admit_test's orientation target abg = (0, -pi / 2, 0), positions and
the right arm's orientation are held where they start.  The sensors read zero but for the push (no contact model).  The push is the
demo's 20 N along x on the left arm, per robot drawn around it, in the demo's window (3000 < count < 5000 of a nominal 8 000 ticks)
scaled to the run length.  It acts at the EE body's frame origin (the reference pushes a gripper body below it, at its centre of mass):
the contact-free stand-in of include/irlosc.h, not MuJoCo.  How far the arm yields and whether it comes back is reported, not promised.

    python examples/admit_test_resident_headless.py [--robots 4096] [--ticks 8000]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from irl_control_amd import BatchedOSC, Target, synth               # noqa: E402
from irl_control_amd.pushes import push_window_ticks                # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel               # noqa: E402

DEMO_TICKS, DEMO_WINDOW, DEMO_PUSH = 8000, (3000, 5000), (20.0, 0.0, 0.0, 0.0, 0.0, 0.0)
N_SENSOR = 18


def start_states(robots, seed=0):
    """Start configurations: a bent-arm pose of both arms, +- 0.15 rad per robot on the arm joints."""
    rng = np.random.default_rng(seed)
    q = np.zeros((robots, 25))
    q[:, 1:7] = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3]) + rng.uniform(-0.15, 0.15, (robots, 6))
    q[:, 13:19] = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2]) + rng.uniform(-0.15, 0.15, (robots, 6))
    return q


def window_for(ticks):
    """The demo's window scaled to a run of `ticks` ticks, as 0-based ticks [tick0, tick1)."""
    lo, hi = (int(round(w * ticks / DEMO_TICKS)) for w in DEMO_WINDOW)
    return push_window_ticks((lo, max(hi, lo + 2)))


def run(robots=16, ticks=8000, seed=0, dt=1e-3, damping=0.0, push=True, trace_before=False, verbose=True):
    """-> dict(ee_start, ee_before, ee_window_end, ee_end [B, 2, 7]: the EE poses at the start, at the start of the window's first tick,
    at the start of the first tick behind it and after the last tick; wrench [B, 1, 6]; window; flags_any; q; trace_before: every
    tick's EE poses up to the window, with `trace_before`).  push=False: the same run with the push cleared."""
    lay = synth.make_layout("k12_admit")                     # devices: ur5right, ur5left, both under admittance
    _, gains, _ = synth.make_batch("k12_admit", 1, seed=0)
    osc = BatchedOSC(lay, robots, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_ft_sensors(n_sensor=N_SENSOR)
    osc.set_plant(dt, damping)
    q = start_states(robots, seed)
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    tgt = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()
    t = Target()
    t.set_abg(np.array([0, -1 * np.pi / 2, 0]))              # admit_test.py:66
    tgt[:, 1, 3:] = t.get_quat()
    osc.set_targets(tgt)
    osc.set_sensordata(np.zeros((robots, N_SENSOR)))
    w0, w1 = window_for(ticks)
    rng = np.random.default_rng(seed + 1)
    wrench = np.asarray(DEMO_PUSH) * rng.uniform(0.75, 1.25, (robots, 1, 1))      # per robot, around the demo's 20 N
    osc.set_pushes([dict(dev="ur5left", window=(w0, w1), apply=True, sense=True)], wrench)
    if not push:
        osc.clear_pushes()
    flags = np.zeros(robots, np.uint32)
    pieces = []
    for n, every in ((w0, 1 if trace_before else max(w0, 1)), (w1 - w0, w1 - w0), (ticks - w1, max(ticks - w1, 1))):
        if n < 1:
            pieces.append(None)
            continue
        out = osc.rollout(n, trace_every=every)
        flags |= out["flags_any"]
        pieces.append(out["ee_trace"])
    qpos, qvel = osc.download_q()
    osc.frontend()
    ee_end = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()
    osc.close()
    ee_start = pieces[0][0] if pieces[0] is not None else pieces[1][0]
    ee_before = pieces[1][0]
    ee_window_end = pieces[2][0] if pieces[2] is not None else ee_end
    frozen = flags & (64 | 1) != 0                           # IRLOSC_FLAG_NONFINITE | IRLOSC_FLAG_M_NOT_PD
    if verbose:
        def left(a, b):
            d = np.linalg.norm(a[:, 1, :3] - b[:, 1, :3], axis=1)
            return f"min {d.min():.3g} median {np.median(d):.3g} max {d.max():.3g} m"
        print(f"{robots} robots, {ticks} ticks of {dt * 1e3:g} ms; push on ur5left during ticks [{w0}, {w1}): fx "
              f"{wrench[:, 0, 0].min():.3g} .. {wrench[:, 0, 0].max():.3g} N" + ("" if push else " (cleared)"))
        print(f"  left EE against its start, before the window:   {left(ee_before, ee_start)}")
        print(f"  left EE against before the window, at its end:  {left(ee_window_end, ee_before)}")
        print(f"  left EE against before the window, at the end:  {left(ee_end, ee_before)}")
        print(f"  robots frozen by the plant at some tick: {int(frozen.sum())}")
    return dict(ee_start=ee_start, ee_before=ee_before, ee_window_end=ee_window_end, ee_end=ee_end, wrench=wrench, window=(w0, w1),
                flags_any=flags, q=qpos, qd=qvel, trace_before=pieces[0] if trace_before else None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=8000)
    a = ap.parse_args()
    run(a.robots, a.ticks)
