#!/usr/bin/env python3
"""The fleet insertion sequence of examples/insertion_fleet_headless.py with the host out of the loop: the same start states, the
same randomly placed action objects and the same SHORT_SEQUENCE, but the WP / GRIP action list runs on the GPU inside
`rollout` (BatchedOSC.set_action_list: csrc/osc_action.hpp between the walk and the OSC step of every tick, the contact-free plant
behind it).  The host asks every `--chunk` ticks whether the fleet is done.

    python examples/insertion_fleet_resident_headless.py [--robots 32] [--chunk 250] [--max-ticks 12000]

The physics differs from the host example's in one respect: the plant kernel integrates every joint with the step's own M and bias
(examples/closed_loop_headless.py), where the host example solves with the M and bias of the dense records; both are contact-free.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from insertion_fleet_headless import SHORT_SEQUENCE, random_objects                   # noqa: E402
from irl_control_amd import BatchedOSC, synth                                         # noqa: E402
from irl_control_amd.action_sequence import load_action_config                        # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel                                 # noqa: E402


def run(robots=32, max_ticks=12000, chunk=250, seed=0, dt=1e-3, verbose=True, sequence=None):
    rng = np.random.default_rng(seed)
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    model = RigidBodyModel.load("dual_ur5")
    cfg = load_action_config("insertion_task.yaml")
    seq = sequence if sequence is not None else SHORT_SEQUENCE
    B = robots
    q = np.zeros((B, 25))
    q[:, 1:7] = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3]) + rng.uniform(-0.15, 0.15, (B, 6))
    q[:, 13:19] = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2]) + rng.uniform(-0.15, 0.15, (B, 6))
    qd = np.zeros_like(q)
    objects = random_objects(rng, lay, model, q, cfg["nist_action_objects"])
    osc = BatchedOSC(lay, B, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    osc.set_plant(dt)
    osc.upload_q(q, qd)
    osc.frontend()
    osc.set_targets(osc.download_records(keys=("ee_pose",))["ee_pose"])      # the runner's start: every arm holds where it is
    osc.set_action_list(seq, objects, active_arm="right", tick_seconds=dt, passive_hold_orientation=True)
    ticks, A = 0, len(seq)
    st = osc.action_state()
    while ticks < max_ticks and not np.all(st["action"] >= A):
        n = min(chunk, max_ticks - ticks)
        out = osc.rollout(n)
        ticks += n
        st = osc.action_state()
    done = st["action"] >= A
    osc.close()
    if verbose:
        ft = st["finished_tick"][done]
        print(f"{B} robots, {A} actions each: {'all finished' if done.all() else f'{int(done.sum())} finished'} after {ticks} ticks on the GPU "
              f"in chunks of {chunk} (finished_tick min {ft.min() if len(ft) else -1}, max {ft.max() if len(ft) else -1}; "
              f"actions reached: min {st['action'].min()}, max {st['action'].max()})")
    return dict(done=done, action=st["action"], finished_tick=st["finished_tick"], ticks=ticks, q=out["qpos"] if ticks else q)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=250)
    ap.add_argument("--max-ticks", type=int, default=12000)
    a = ap.parse_args()
    r = run(a.robots, a.max_ticks, a.chunk)
    sys.exit(0 if r["done"].all() else 1)
