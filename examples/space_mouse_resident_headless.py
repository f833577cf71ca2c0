#!/usr/bin/env python3
"""The space-mouse teleoperation demo (teleop_loops.space_mouse_loop) on a resident fleet: B robots follow a recorded session -- one
operator's stream for the whole fleet, or a stream per robot -- and every tick stays on the GPU: the stream kernel integrates the tick's
reading into each robot's plate pose and writes the arms' and the base's targets in front of the same tick's OSC step
(BatchedOSC.set_teleop_stream -> irlosc_set_teleop_stream), the contact-free plant advances the coordinates.

Per tick and robot, one train of kernels and nothing across PCIe:
    (qpos, qvel) --walk--> M, J, bias, EE pose;  reading --stream kernel--> plate pose, targets --> OSC step --> u --plant--> (qpos, qvel)
--host-loop runs the per-tick host form instead (teleop.stream_step on the host, set_targets + rollout(1) per tick: one round trip per
control tick), --no-stream the same rollout with the targets held, for the cost of the stream kernel.  How well the arms track is
reported, not promised: the plant has no contacts and the plate may leave the arms' reach.

    python examples/space_mouse_resident_headless.py [--robots 4096] [--ticks 200] [--per-robot] [--host-loop | --no-stream]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from irl_control_amd import BatchedOSC, synth, teleop                # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel               # noqa: E402
import teleop_loops as tl                                           # noqa: E402

AMP = np.array([60.0, 60.0, 40.0, 150.0, 150.0, 250.0])             # teleop_loops.space_mouse_stream


def start_states(robots, seed=0):
    """Start configurations: a bent-arm pose of both arms, +- 0.15 rad per robot on the arm joints."""
    rng = np.random.default_rng(seed)
    q = np.zeros((robots, 25))
    q[:, 1:7] = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3]) + rng.uniform(-0.15, 0.15, (robots, 6))
    q[:, 13:19] = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2]) + rng.uniform(-0.15, 0.15, (robots, 6))
    return q


def fleet_readings(seeds, ticks):
    """[len(seeds), ticks, 6]: teleop_loops.space_mouse_stream(seed, ticks) of every seed, its formula over all ticks at once."""
    t = np.arange(ticks)[:, None]
    out = np.empty((len(seeds), ticks, 6))
    for i, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        ph, fr = rng.uniform(0, 2 * np.pi, 6), rng.uniform(0.02, 0.09, 6)
        out[i] = AMP * np.sin(fr * t + ph)
    return out


def run(robots=16, ticks=200, seed=5, per_robot=False, stream=True, host_loop=False, dt=1e-3, damping=0.0, verbose=True):
    """-> dict(pose [B, 6]: the final plate poses, tgt, ee [B, 3, 7]: targets and EE poses after the last tick, err [B, 2]: the arms'
    position errors, flags_any, q, qd, ms_per_tick: wall clock of the ticks).  per_robot: robot b replays seed + b, else the fleet
    replays `seed`.  stream=False: the targets stay where the first tick of the stream puts them.  host_loop: the per-tick host form."""
    lay = synth.make_layout("k13")                           # devices: ur5right, ur5left, base
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    osc = BatchedOSC(lay, robots, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(dt, damping)
    q = start_states(robots, seed)
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    tgt = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()      # until the first tick: hold the end effectors
    osc.set_targets(tgt)
    osc.rollout(1)                                           # a tick that is not timed: the rollout's buffers are allocated by its first use
    osc.upload_q(q, np.zeros_like(q))
    rig = teleop.space_mouse_rig(lay)
    origin = np.array(teleop.ORIGIN)
    readings = fleet_readings([seed + b for b in range(robots)], ticks) if per_robot else teleop.record_readings(tl.space_mouse_stream(seed, ticks), ticks)
    flags = np.zeros(robots, np.uint32)
    if host_loop or not stream:
        rd = readings if per_robot else readings[None]
        pose = np.tile(origin, (len(rd), 1))
        t0 = time.perf_counter()
        for t in range(ticks if host_loop else 1):
            for b in range(len(rd)):
                pose[b], new = teleop.stream_step(pose[b], rd[b, t], rig)
                rows = slice(b, b + 1) if per_robot else slice(None)
                tgt[rows] = np.where(np.isnan(new), tgt[rows], new)
            osc.set_targets(tgt)
            if host_loop:
                flags |= osc.rollout(1)["flags_any"]
        if not host_loop:
            t0 = time.perf_counter()
            flags |= osc.rollout(ticks)["flags_any"]
        seconds = time.perf_counter() - t0
        pose = np.broadcast_to(pose, (robots, 6)) if not per_robot else pose
    else:
        osc.set_teleop_stream(readings, origin, rig)
        t0 = time.perf_counter()
        flags |= osc.rollout(ticks)["flags_any"]
        seconds = time.perf_counter() - t0
        pose = osc.teleop_state()["pose"]
    tgt_end = osc.download_targets()
    qpos, qvel = osc.download_q()
    osc.frontend()
    ee = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()
    osc.close()
    err = np.linalg.norm(ee[:, :2, :3] - tgt_end[:, :2, :3], axis=2)
    frozen = flags & (64 | 1) != 0                           # IRLOSC_FLAG_NONFINITE | IRLOSC_FLAG_M_NOT_PD
    if verbose:
        how = "the per-tick host loop" if host_loop else "one rollout" + ("" if stream else " with the targets held (no stream)")
        print(f"{robots} robots, {ticks} ticks of {dt * 1e3:g} ms, {'a stream per robot' if per_robot else 'one stream for the fleet'}, {how}: "
              f"{seconds * 1e3 / ticks:.4g} ms per tick")
        print(f"  final plate pose of robot 0 (x y z roll pitch yaw): {np.array2string(np.asarray(pose[0]), precision=4)}")
        for d, name in enumerate(lay.dev_names[:2]):
            e = err[~frozen, d] if (~frozen).any() else err[:, d]
            print(f"  {name}: EE against its target after the last tick: min {e.min():.3g} median {np.median(e):.3g} max {e.max():.3g} m")
        print(f"  robots frozen by the plant at some tick: {int(frozen.sum())}")
    return dict(pose=np.array(pose), tgt=tgt_end, ee=ee, err=err, flags_any=flags, q=qpos, qd=qvel, ms_per_tick=seconds * 1e3 / ticks)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--per-robot", action="store_true", help="robot b replays the session of seed + b")
    ap.add_argument("--host-loop", action="store_true", help="the per-tick host form: stream_step, set_targets, rollout(1)")
    ap.add_argument("--no-stream", action="store_true", help="the same rollout with the targets held: the cost of everything but the stream kernel")
    a = ap.parse_args()
    run(a.robots, a.ticks, a.seed, a.per_robot, stream=not a.no_stream, host_loop=a.host_loop)
