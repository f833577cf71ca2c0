#!/usr/bin/env python3
"""The reference's second action-sequence file, action_sequence_configs/iros2022_task.yaml (a copy: tests/golden/iros2022_task.yaml),
for a fleet on the GPU: its pickup, demo and release sequences as one action list with a MOTION -- the INTERP actions travel to their
goals over `steps` ticks and the `noise: [mean, std]` entries scatter the goals, drawn on the GPU from --seed, the robot's index and
its count of draws (BatchedOSC.set_action_motion; csrc/osc_action.hpp, csrc/osc_rng.hpp).  The reference ships no runner for this
file; the semantics are those of include/irlosc.h.  The file gives a column per device: the active arm's is taken
(action_motion.compile_iros2022), the other arm keeps its pose.  No contact and no objects here: the GRIP actions wait their ticks.

    python examples/iros2022_task_resident_headless.py [--robots 32] [--seed 0] [--arm right] [--episodes 0] [--max-ticks 20000]
                                                        [--config tests/golden/iros2022_task.yaml]

Prints per-robot finish ticks and, per noisy action, the spread of the goals the robots were seen aiming at against the file's std.
With --episodes N every robot runs the list N times from its start state (BatchedOSC.set_episodes); its draws go on counting, so every
episode scatters afresh."""
import argparse
import os
import sys

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from irl_control_amd import BatchedOSC, synth                                         # noqa: E402
from irl_control_amd import action_motion as am                                       # noqa: E402
from irl_control_amd import action_sequence as aseq                                   # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel                                 # noqa: E402

SEQUENCES = ("iros2022_pickup_sequence", "iros2022_demo_sequence", "iros2022_release_sequence")
DEFAULT_CONFIG = os.path.join(ROOT, "tests", "golden", "iros2022_task.yaml")


def compile_task(config_path=DEFAULT_CONFIG, arm="right", seed=0):
    """-> (wp_sequence, motion) of the file's three sequences for the active arm"""
    with open(config_path) as f:
        cfg = yaml.safe_load(f)
    seq, motion = am.compile_action_motion(am.compile_iros2022(cfg, SEQUENCES, arm))
    motion["seed"] = int(seed)
    return seq, motion


def run(robots=32, seed=0, arm="right", episodes=0, max_ticks=20000, chunk=25, config=DEFAULT_CONFIG, dt=1e-3, verbose=True):
    rng = np.random.default_rng(0)                        # the fleet's start states: the same for every --seed, which is the noise's alone
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    model = RigidBodyModel.load("dual_ur5")
    seq, motion = compile_task(config, arm, seed)
    B, A = robots, len(seq)
    q = np.zeros((B, 25))
    q[:, 1:7] = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3]) + rng.uniform(-0.05, 0.05, (B, 6))
    q[:, 13:19] = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2]) + rng.uniform(-0.05, 0.05, (B, 6))
    qd = np.zeros_like(q)
    osc = BatchedOSC(lay, B, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    osc.set_plant(dt)
    osc.upload_q(q, qd)
    osc.frontend()
    osc.set_targets(osc.download_records(keys=("ee_pose",))["ee_pose"])      # every arm holds where it is
    osc.set_action_list(seq, None, active_arm=arm, tick_seconds=dt, passive_hold_orientation=True)
    osc.set_action_motion(motion)
    if episodes:
        osc.set_episodes(q[:, None], qd[:, None], max_episodes=episodes, records=min(16, max(1, episodes)))
    noisy = np.nonzero((motion["noise_std"] > 0) | (motion["noise_mean"] != 0))[0]
    seen = {int(a): {} for a in noisy}                    # action -> {(robot, draw): goal xyz}
    ticks = 0
    st = osc.action_state()
    while ticks < max_ticks:
        if episodes and osc.episode_state()["running"] == 0:
            break
        if not episodes and np.all(st["action"] >= A):
            break
        n = min(chunk, max_ticks - ticks)
        osc.rollout(n)
        ticks += n
        st, ms = osc.action_state(), osc.action_motion_state()
        for b in range(B):
            a = int(st["action"][b])
            if a in seen:
                seen[a][(b, int(ms["draws"][b]))] = ms["goal"][b, :3].copy()
    ms = osc.action_motion_state()
    es = osc.episode_state() if episodes else None
    osc.close()
    done = st["action"] >= A if not episodes else es["count"] >= episodes
    table = aseq.compile_action_list(seq, [{}], 0)["pose"][0]
    spread = {}
    for a, goals in seen.items():
        if goals:
            g = np.array(list(goals.values())) - table[a, :3]
            spread[a] = (len(g), float(g.mean()), float(g.std()))
    if verbose:
        if episodes:
            lens = es["records"][:, :min(episodes, es["records"].shape[1]), 1]
            print(f"{B} robots, {A} actions, {episodes} episodes each: {int(done.sum())} robots through after {ticks} ticks; episode lengths "
                  f"min {lens[lens > 0].min() if (lens > 0).any() else -1}, max {lens.max()}; draws per robot {ms['draws'].min()} .. {ms['draws'].max()}")
        else:
            ft = st["finished_tick"]
            print(f"{B} robots, {A} actions each: {'all finished' if done.all() else f'{int(done.sum())} finished'} after {ticks} ticks on the GPU "
                  f"(actions reached: min {st['action'].min()}, max {st['action'].max()}; draws per robot {ms['draws'].min()} .. {ms['draws'].max()})")
            print("finish ticks per robot:", " ".join(str(int(t)) for t in ft))
        for a, (n, mean, std) in sorted(spread.items()):
            print(f"action {a:2d} ({seq[a].get('name', '')}): {n} goals seen, offset from the file's target mean {mean:+.5f} m, std {std:.5f} m "
                  f"(file: mean {motion['noise_mean'][a]:g}, std {motion['noise_std'][a]:g})")
    return dict(done=done, action=st["action"], finished_tick=st["finished_tick"], ticks=ticks, draws=ms["draws"], spread=spread)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0, help="seed of the target noise")
    ap.add_argument("--arm", default="right", choices=["right", "left"])
    ap.add_argument("--episodes", type=int, default=0, help="episodes per robot (0: the list once, without episodes)")
    ap.add_argument("--max-ticks", type=int, default=20000)
    ap.add_argument("--config", default=DEFAULT_CONFIG)
    a = ap.parse_args()
    r = run(a.robots, a.seed, a.arm, a.episodes, a.max_ticks, config=a.config)
    sys.exit(0 if r["done"].all() else 1)
