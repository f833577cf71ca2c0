#!/usr/bin/env python3
"""The wall demo of force_test (headless_loops.force_test_loop) on a resident fleet: B robots under admittance control, the left arm
walks the demo's line of waypoints into a wall, and every tick stays on the GPU -- the targets are cycled there
(BatchedOSC.set_waypoints), the wall's force is computed there from the EE position and velocity of the tick, acts on the plant
there, and the F/T wrench of the next tick carries its reaction (BatchedOSC.set_walls -> irlosc_set_walls).

Per tick and robot, one train of kernels and nothing across PCIe:
    (qpos, qvel) --walk--> M, J, bias, EE pose --feed's wrench - wall force of the tick before--> OSC step --> u --cycler--> targets
                 --wall: F = (k depth - c approach speed) n, bias -= J^T F--> plant --> (qpos, qvel)
Layout k12_admit with the osc1 gains: both arms under admittance; force_test_loop's paths -- the right arm one waypoint, the left arm
the ten, threshold 1 cm, looping -- and its orientation target abg = (0, 0, -pi / 2) on the left arm.  The wall is the reference
scene's: the face y = 0.75 of the box x in [-0.5, 0.5], y in [0.75, 0.85], z in [0, 1], as the half-space with the normal (0, -1, 0),
with the geom's solref = "-900 -20" read as a spring of 900 N/m and a damper of 20 N s/m.  The EE is a sphere of --radius around the
EE body's frame origin; the default 0.1 m is a stand-in for the gripper's reach, which nobody has measured.

What this is NOT: it is not MuJoCo's soft constraint (a penalty force, no constraint solver); it has no friction; it has no geometry
beyond a plane (the box's other faces and its extent do not exist); and the contact point is the EE body's frame origin, not a point
on the gripper.  How far this plant yields and whether it settles is reported, not promised.

After every chunk of --log-every ticks the left arm's wall force goes into the CSV the reference writes (x, force_x, force_y, force_z;
here x is the tick count and the force that of robot --csv-robot).

    python examples/force_test_resident_headless.py [--robots 4096] [--ticks 8000] [--log-every 100] [--radius 0.1] [--csv data.csv]
"""
import argparse
import csv
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from irl_control_amd import BatchedOSC, Target, synth, walls        # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel               # noqa: E402

RIGHT_WPS = np.array([[0.3, 0.46432, 0.36243]])                     # headless_loops.force_test_loop
LEFT_WPS = np.array([[-0.3, y, 0.5] for y in (0.46432, 0.5, 0.55, 0.575, 0.6, 0.625, 0.65, 0.675, 0.7, 0.75)])
WALL = dict(dev="ur5left", normal=(0.0, -1.0, 0.0), offset=-0.75, stiffness=900.0, damping=20.0)
N_SENSOR = 18
THRESHOLD = 0.01                                                    # m: force_test_loop's threshold_ee
# joint configurations that put the EEs on their first waypoints (found with the rigid-body oracle)
Q_RIGHT = np.array([-0.069, -0.017, -0.192, 4.603, -1.764, 0.3])
Q_LEFT = np.array([-0.181, -0.186, 0.228, -4.532, -5.541, 0.0])


def start_states(robots, seed=0, spread=0.05):
    """Start configurations: both EEs on their first waypoints, +- `spread` rad per robot on the arm joints, at rest."""
    rng = np.random.default_rng(seed)
    q = np.zeros((robots, 25))
    q[:, 1:7] = Q_RIGHT + rng.uniform(-spread, spread, (robots, 6))
    q[:, 13:19] = Q_LEFT + rng.uniform(-spread, spread, (robots, 6))
    return q


def run(robots=16, ticks=8000, log_every=100, radius=0.1, seed=0, dt=1e-3, damping=0.0, compare=True, csv_path=None, csv_robot=0,
        verbose=True):
    """-> dict(force_log [chunks, B, 3]: the left arm's wall force after every chunk; depth_log [chunks, B]: its deepest penetration so
    far; contact_ticks, first_tick, max_depth [B]: the left arm's wall state at the end; free_depth [B]: the deepest penetration of the
    same run WITHOUT the wall on a second slot (compare=True; every tick's traced EE against the same half-space); index [B]: the left
    arm's waypoint index at the end; csv_rows; flags_any; q)."""
    lay = synth.make_layout("k12_admit")                     # devices: ur5right, ur5left, both under admittance
    _, gains, _ = synth.make_batch("k12_admit", 1, seed=0)   # the osc1 gains: kp 200, kv 50, ko 200
    osc = BatchedOSC(lay, robots, dtype=np.float64, n_slots=2)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_ft_sensors(n_sensor=N_SENSOR)
    osc.set_plant(dt, damping)
    q = start_states(robots, seed)
    wall = dict(WALL, radius=float(radius))
    _, rows = walls.normalise([wall], lay.dev_names, robots)
    slots = (0, 1) if compare else (0,)
    for slot in slots:
        osc.upload_q(q, np.zeros_like(q), slot=slot)
        if slot == 0:
            osc.frontend()
            tgt = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()      # the right arm's orientation: held where it starts
            t = Target()
            t.set_abg(np.array([0, 0, -1 * np.pi / 2]))      # force_test.py
            tgt[:, 1, 3:] = t.get_quat()
        osc.set_targets(tgt, slot=slot)
        osc.set_sensordata(np.zeros((robots, N_SENSOR)), slot=slot)      # the sensors read zero but for the wall
        osc.set_waypoints([RIGHT_WPS, LEFT_WPS], THRESHOLD, loop=True, slot=slot)
    osc.set_walls([wall], slot=0)
    flags = np.zeros(robots, np.uint32)
    free_depth = np.zeros(robots)
    force_log, depth_log, csv_rows = [], [], [["x", "force_x", "force_y", "force_z"]]
    done = 0
    while done < ticks:
        n = min(log_every, ticks - done)
        out = osc.rollout(n, slot=0)
        flags |= out["flags_any"]
        done += n
        st = osc.wall_state(0)
        force_log.append(st["force"][:, 1].copy())
        depth_log.append(st["max_depth"][:, 1].copy())
        csv_rows.append([done] + [float(v) for v in st["force"][csv_robot, 1]])
        if compare:
            tr = osc.rollout(n, trace_every=1, slot=1)["ee_trace"][:, :, 1, :3]      # [n, B, 3]
            g = walls.depth(tr.reshape(-1, 3), rows)[:, 0].reshape(n, robots)
            free_depth = np.maximum(free_depth, np.where(g > 0, g, 0.0).max(axis=0))
    st = osc.wall_state(0)
    index = osc.waypoint_state(0)["index"][:, 1]
    osc.close()
    force_log, depth_log = np.array(force_log), np.array(depth_log)
    if csv_path:
        with open(csv_path, "w", newline="") as f:
            csv.writer(f).writerows(csv_rows)
    frozen = flags & (64 | 1) != 0                           # IRLOSC_FLAG_NONFINITE | IRLOSC_FLAG_M_NOT_PD
    if verbose:
        hit = st["contact_ticks"][:, 1] > 0
        print(f"{robots} robots, {ticks} ticks of {dt * 1e3:g} ms; wall y = 0.75, k = {WALL['stiffness']:g} N/m, c = {WALL['damping']:g} N s/m, "
              f"EE radius {radius:g} m")
        print(f"  robots that touched the wall: {int(hit.sum())}; first touch at tick {st['first_tick'][hit, 1].min() if hit.any() else -1} "
              f"at the earliest; left waypoint index at the end: min {index.min()} median {np.median(index):g} max {index.max()}")
        for i in range(0, len(force_log), max(1, len(force_log) // 10)):
            fy = -force_log[i][:, 1]
            print(f"  tick {min((i + 1) * log_every, ticks):6d}: deepest so far median {np.median(depth_log[i]) * 1e3:7.2f} mm max "
                  f"{depth_log[i].max() * 1e3:7.2f} mm; push of the wall median {np.median(fy):7.2f} N max {fy.max():7.2f} N")
        if compare:
            print(f"  deepest penetration with the wall: median {np.median(st['max_depth'][hit, 1]) * 1e3 if hit.any() else 0:.2f} mm; the "
                  f"same robots without it: median {np.median(free_depth[hit]) * 1e3 if hit.any() else 0:.2f} mm")
        print(f"  robots frozen by the plant at some tick: {int(frozen.sum())}")
    return dict(force_log=force_log, depth_log=depth_log, contact_ticks=st["contact_ticks"][:, 1], first_tick=st["first_tick"][:, 1],
                max_depth=st["max_depth"][:, 1], free_depth=free_depth, index=index, csv_rows=csv_rows, flags_any=flags, q=out["qpos"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=8000)
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--csv", default=None)
    ap.add_argument("--csv-robot", type=int, default=0)
    a = ap.parse_args()
    run(a.robots, a.ticks, a.log_every, a.radius, csv_path=a.csv, csv_robot=a.csv_robot)
