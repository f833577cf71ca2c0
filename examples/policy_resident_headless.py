#!/usr/bin/env python3
"""A policy drives a resident fleet: B robots, each with a plate that starts at an origin of its own, are steered to one common goal by a
network evaluated on the GPU per robot and tick (BatchedOSC.set_policy -> irlosc_set_policy, csrc/osc_policy.hpp) -- nothing is recorded
ahead of time and nothing crosses PCIe inside the rollout:
    (qpos, qvel) --walk--> M, J, bias, EE pose;  plate pose --policy kernel--> reading --> plate pose, targets --> OSC step --> u --plant--> (qpos, qvel)

The network is ANALYTIC, no training: a proportional servo, reading = clip(K (goal - plate)), written as a 2-layer ReLU net on the PLATE
observation.  With z_c = K s_c (goal_c - plate_c) -- s_c the sign with which the stream's integration takes reading c: + for x y z roll,
- for pitch and yaw -- the hidden layer holds relu(z_c) and relu(-z_c), the output layer their difference, and the clamp of the policy
bounds the step.  A seventh output, thr - K |goal - plate|_1 over x y z, is positive once the plate is near the goal: the hand closes
there (the ACTION drive of the right arm's gripper motor takes grip_close) and stays open on the way.

It runs with episodes: every `episode_ticks` ticks a robot's plate is put back to its origin and its coordinates to the start, while the
others go on; the outcome counts are printed.  The arms follow as far as the contact-free plant lets them: reported, not promised.

With --std S the servo explores: a Gaussian head of standard deviation S on the six readings (BatchedOSC.set_policy_noise; the grip's
output stays deterministic) is drawn on the GPU per robot and tick from --seed, and the one rollout runs with a log of every tenth
tick's sampled action and log-probability: the fleet's mean logp and the spread of the final plate error are printed.

With --reward the fleet is judged on the GPU as well (BatchedOSC.set_reward, csrc/osc_reward.hpp): per tick minus the distance of the right
hand's TARGET to the point it has once the plate sits on the goal (what the policy steers), minus a tenth of the hand's lag behind that
target and a small cost on the action, accumulated per episode with a discount; a robot whose target stays within --reach metres of the
point for five ticks has reached the GOAL, which ends its episode early.  The mean return of the ended episodes, the rate of episodes that
reached the goal and their mean length are printed.

    python examples/policy_resident_headless.py [--robots 4096] [--episodes 2] [--episode-ticks 300] [--std 0.5 --seed 5] [--reward]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from irl_control_amd import BatchedOSC, _lib, policy, reward as rw, synth, teleop     # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel                   # noqa: E402
import gripper_fleet_resident_headless as grip                          # noqa: E402
from space_mouse_resident_headless import start_states                  # noqa: E402

GOAL = np.array([0.05, 0.45, 0.55, 0.0, 0.0, 0.3])      # x y z roll pitch yaw of the plate
K = 40.0                                                 # 1 / s-like gain on the pose error, in readings per unit
CLIP = 2.0                                               # the largest reading: at most 3 mm (mrad) per tick at the default increment
NEAR = 0.01                                              # m: |goal - plate|_1 over x y z below which the hand closes
SIGN = np.array([1.0, 1.0, 1.0, 1.0, -1.0, -1.0])       # how the integration takes the six readings (include/irlosc.h)


def servo_layers(goal=GOAL, k=K, near=NEAR):
    """The servo as [(W0 [12, 6], b0), (W1 [7, 12], b1)] float32 on the PLATE observation."""
    W0, b0 = np.zeros((12, 6), np.float32), np.zeros(12, np.float32)
    W1, b1 = np.zeros((7, 12), np.float32), np.zeros(7, np.float32)
    for c in range(6):
        for h, s in ((2 * c, 1.0), (2 * c + 1, -1.0)):      # relu(+z_c), relu(-z_c)
            W0[h, c], b0[h] = -s * k * SIGN[c], s * k * SIGN[c] * goal[c]
        W1[c, 2 * c], W1[c, 2 * c + 1] = 1.0, -1.0
    W1[6, :6], b1[6] = -1.0, k * near                       # k near - k |goal - plate|_1 over x y z
    return [(W0, b0), (W1, b1)]


def reach_reward(lay, reach, gamma=0.99, act_cost=1e-3):
    """Steer the right hand's target to a point: r = -|target - point| - 0.1 |EE - target| - act_cost |act|^2; the goal: the target within
    `reach` metres for five ticks.  The point is where the hand's target lies once the plate sits on GOAL (the rig's transform of GOAL)."""
    point = teleop.stream_step(GOAL, np.zeros(6), teleop.space_mouse_rig(lay))[1][0, :3]
    return rw.Reward([rw.dist(rw.target(0), rw.fixed(0), -1.0), rw.dist(rw.ee(0), rw.target(0), -0.1), rw.act_sq(-act_cost)], gamma=gamma, points=point[None],
                     goal_term=0, goal_cmp="<=", goal_value=reach, goal_hold=5)


def run(robots=16, episodes=2, episode_ticks=300, seed=5, dt=1e-3, damping=0.0, verbose=True, std=0.0, reward=False, reach=0.005):
    """-> dict(records [B, episodes, 4], dist [B]: |goal - plate| over x y z when the last episode ended, grip [B], ms_per_tick; with
    std > 0 also logp [S, B]: the log-probabilities of every tenth tick's sampled actions; with reward also returns [B, episodes, 2]:
    (ret, gret) of every ended episode, and goal_rate)"""
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    osc = BatchedOSC(lay, robots, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(dt, damping)
    q = start_states(robots, seed)
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    osc.set_targets(osc.download_records(keys=("ee_pose",))["ee_pose"].copy())      # until the first tick: hold the end effectors
    rng = np.random.default_rng(seed)
    origin = np.tile(teleop.ORIGIN, (robots, 1))
    origin[:, :3] += rng.uniform(-0.08, 0.08, (robots, 3))
    osc.set_policy(servo_layers(), ("plate",), origin, clip=CLIP, grip_dev="ur5right", grip_close=grip.FORCE, grip_open=-grip.FORCE)
    osc.set_joints(grip.scene_rows())
    if reward:      # (the parts, then the reward, then the episodes -- which now also end on the goal)
        osc.set_reward(reach_reward(lay, reach))
    osc.set_episodes(q[:1], max_ticks=episode_ticks, max_episodes=episodes, records=min(max(episodes, 1), 16))
    ticks = episodes * episode_ticks
    t0 = time.perf_counter()
    # the last episode's final tick parks the robot without a reset: its plate is where the servo left it
    logp = None
    if std > 0.0:
        osc.set_policy_noise([std] * 6 + [0.0], seed=seed)
        t0 = time.perf_counter()
        out = osc.rollout_logged(ticks, ("policy_sample",), every=10)
        logp = out["log"]["policy_sample"][:, :, 7]
    else:
        out = osc.rollout(ticks)
    seconds = time.perf_counter() - t0
    st, es = osc.policy_state(), osc.episode_state()
    rs = osc.reward_state() if reward else None
    osc.close()
    dist = np.abs(st["pose"][:, :3] - GOAL[:3]).sum(axis=1)
    outcome = es["records"][:, :min(episodes, 16), 2]
    if verbose:
        print(f"{robots} robots, {episodes} episodes of {episode_ticks} ticks of {dt * 1e3:g} ms under the servo net: {seconds * 1e3 / ticks:.4g} ms per tick")
        for name, bit in (("timeout", _lib.EPISODE_TIMEOUT), ("finished", _lib.EPISODE_FINISHED), ("inserted", _lib.EPISODE_INSERTED)):
            print(f"  episodes with outcome {name}: {int(((outcome & bit) != 0).sum())} of {outcome.size}")
        print(f"  |goal - plate|_1 over x y z at the end: min {dist.min():.3g} median {np.median(dist):.3g} max {dist.max():.3g} m "
              f"(origins up to {np.abs(origin[:, :3] - GOAL[:3]).sum(axis=1).max():.3g} m away)")
        print(f"  hands closing at the end: {int((st['grip'] == grip.FORCE).sum())} of {robots}; robots frozen by the plant at some tick: "
              f"{int((out['flags_any'] & (64 | 1) != 0).sum())}")
        if logp is not None:
            print(f"  Gaussian head, std {std:g} on the six readings, seed {seed}: mean logp of the {logp.size} logged samples {logp.mean():.4f}; final "
                  f"plate error: mean {dist.mean():.3g}, standard deviation {dist.std():.3g} m over the fleet")
    returns = goal_rate = None
    if reward:
        ended = np.arange(min(episodes, 16))[None, :] < es["count"][:, None]      # (an early goal leaves no episode open: all of them ended)
        returns, goal = rs["records"][:, :min(episodes, 16)], (outcome & _lib.EPISODE_GOAL) != 0
        goal_rate = float(goal[ended].mean()) if ended.any() else 0.0
        if verbose:
            print(f"  reward (reach within {reach:g} m for 5 ticks, gamma 0.99): mean return of the {int(ended.sum())} ended episodes {returns[..., 0][ended].mean():.4f} "
                  f"(discounted {returns[..., 1][ended].mean():.4f}); goal rate {goal_rate:.3f}; mean episode length {es['records'][:, :min(episodes, 16), 1][ended].mean():.1f} ticks")
    return dict(returns=returns, goal_rate=goal_rate, records=es["records"], dist=dist, grip=st["grip"], ms_per_tick=seconds * 1e3 / ticks, pose=st["pose"], logp=logp)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--episode-ticks", type=int, default=300)
    ap.add_argument("--seed", type=int, default=5, help="of the start states and origins, and the key of the exploration noise")
    ap.add_argument("--std", type=float, default=0.0, help="> 0: a Gaussian head of this standard deviation on the six readings")
    ap.add_argument("--reward", action="store_true", help="a reach reward with an action cost and a goal, evaluated on the GPU")
    ap.add_argument("--reach", type=float, default=0.005, help="m: the goal's distance of the right hand's target to its point")
    a = ap.parse_args()
    run(a.robots, a.episodes, a.episode_ticks, a.seed, std=a.std, reward=a.reward, reach=a.reach)
