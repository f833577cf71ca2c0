#!/usr/bin/env python3
"""(observation, action) pairs out of a resident fleet: the gain_test fleet of gain_test_resident_headless.py walks its waypoints on
the GPU, and every tick's observations and torques of a handful of its robots come back as an EPISODE LOG
(BatchedOSC.rollout_logged -> irlosc_rollout_from_q_logged, csrc/osc_log.hpp) -- gathered on the GPU behind the tick's OSC step and
drained to the host while the following ticks run, instead of cutting the rollout into one-tick calls with downloads in between.

Per logged tick and robot: qpos, qvel, ee_pose, targets (the observation: the state the controller used and the targets it saw) and u
(the action: the torques it produced).  Written as one .npz: obs_qpos, obs_qvel, obs_ee_pose, obs_targets, act_u [ticks, robots, ...],
with `robots` (their indices in the fleet) and `ticks`.

    python examples/episode_log_resident_headless.py [--robots 4096] [--ticks 400] [--logged 8] [--out episode_log.npz] [--check]

--check replays the same start in one-tick rollouts with downloads around each tick and asserts that the two agree bit for bit.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from gain_test_resident_headless import start_states                 # noqa: E402
from headless_loops import THRESHOLD_EE, gain_test_waypoints         # noqa: E402
from irl_control_amd import BatchedOSC, synth                        # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel                # noqa: E402

CHANNELS = ("qpos", "qvel", "ee_pose", "targets", "u")


def fleet(robots, seed=0, dt=1e-3, damping=0.0):
    """The gain_test fleet at its start: k13, every robot its own bent-arm start, the demo's waypoints on both arms."""
    right, left = gain_test_waypoints()
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    osc = BatchedOSC(lay, robots, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(dt, damping)
    q = start_states(robots, seed)
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    tgt = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()
    osc.upload_q(q, np.zeros_like(q))
    osc.set_targets(tgt)
    osc.set_waypoints([right, left, None], THRESHOLD_EE, loop=True)
    return osc


def logged_robots(robots, logged):
    """`logged` robots spread over the fleet, the first and the last among them."""
    return np.unique(np.linspace(0, robots - 1, min(logged, robots)).round().astype(np.int32))


def run(robots=4096, ticks=400, logged=8, seed=0, verbose=True):
    idx = logged_robots(robots, logged)
    osc = fleet(robots, seed)
    out = osc.rollout_logged(ticks, CHANNELS, every=1, robots=idx)
    osc.close()
    log = out["log"]
    pairs = dict(obs_qpos=log["qpos"], obs_qvel=log["qvel"], obs_ee_pose=log["ee_pose"], obs_targets=log["targets"], act_u=log["u"],
                 robots=idx, ticks=out["log_ticks"])
    if verbose:
        moved = np.abs(log["targets"][1:] - log["targets"][:-1]).max(axis=(2, 3)) > 0
        print(f"{robots} robots, {ticks} ticks; logged robots {idx.tolist()}: {log['u'].shape[0]} (observation, action) pairs each, "
              f"{sum(a.nbytes for a in log.values()) / 1e6:.2f} MB")
        print(f"  waypoint changes seen in the logged targets per robot: {moved.sum(axis=0).tolist()}")
        print(f"  max |u| over the episode per robot: {np.abs(log['u']).max(axis=(0, 2)).round(2).tolist()}")
    return pairs, out


def check(pairs, robots, ticks, seed=0):
    """The same start in one-tick rollouts with downloads around each tick: what callers had before the log.  Bit for bit."""
    idx = pairs["robots"]
    osc = fleet(robots, seed)
    for t in range(ticks):
        q, qd = osc.download_q()
        tgt = osc.download_targets()
        r = osc.rollout(1, trace_every=1)
        for name, got, want in (("qpos", pairs["obs_qpos"][t], q[idx]), ("qvel", pairs["obs_qvel"][t], qd[idx]),
                                ("targets", pairs["obs_targets"][t], tgt[idx]), ("ee_pose", pairs["obs_ee_pose"][t], r["ee_trace"][0][idx]),
                                ("u", pairs["act_u"][t], r["u"][idx])):
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (name, t)
    osc.close()
    print(f"  check: {ticks} one-tick rollouts with downloads agree with the log bit for bit")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=400)
    ap.add_argument("--logged", type=int, default=8)
    ap.add_argument("--out", default="episode_log.npz")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    pairs, _ = run(a.robots, a.ticks, a.logged)
    np.savez(a.out, **pairs)
    print(f"  wrote {a.out}")
    if a.check:
        check(pairs, a.robots, a.ticks)
