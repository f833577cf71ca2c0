#!/usr/bin/env python3
"""The insertion fleet of examples/insertion_fleet_resident_headless.py, episode after episode without the host in between: every robot
runs SHORT_SEQUENCE on its own action objects, and when its list is through -- or its time limit is up -- the GPU writes the episode's
record, puts the robot back to its start and gives it the next set of object poses (BatchedOSC.set_episodes: csrc/osc_episode.hpp
behind the plant of every tick), while its neighbours go on.  One rollout call runs all the ticks; with --episodes N every robot parks
after N episodes and the call ends by itself once the fleet is through (poll_every).

    python examples/insertion_episodes_resident_headless.py [--robots 32] [--ticks 20000] [--limit 4000] [--variants 3] [--episodes 0]

Prints episodes per second, the FINISHED / TIMEOUT split and the histogram of episode lengths (of the last up to 16 episodes a robot
ended: what the device keeps)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from insertion_fleet_headless import SHORT_SEQUENCE, random_objects                   # noqa: E402
from irl_control_amd import BatchedOSC, _lib, synth                                   # noqa: E402
from irl_control_amd import action_sequence as aseq                                   # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel                                 # noqa: E402


def build(robots=32, variants=3, seed=0, dt=1e-3, distinct=None):
    """-> dict(lay, gains, model, q, qd: one start state per robot; lists: per variant the compiled list (its poses [B, A, 7])).
    distinct: draw this many robots and repeat them to `robots` (a large fleet's objects are placed one robot at a time on the host)."""
    rng = np.random.default_rng(seed)
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    model = RigidBodyModel.load("dual_ur5")
    cfg = aseq.load_action_config("insertion_task.yaml")
    n = robots if distinct is None else min(robots, distinct)
    q = np.zeros((n, 25))
    q[:, 1:7] = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3]) + rng.uniform(-0.15, 0.15, (n, 6))
    q[:, 13:19] = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2]) + rng.uniform(-0.15, 0.15, (n, 6))
    names = list(lay.dev_names)
    lists = []
    for _ in range(variants):
        objects = random_objects(rng, lay, model, q, cfg["nist_action_objects"])
        d = aseq.compile_action_list(SHORT_SEQUENCE, objects, names.index("ur5right"), names.index("ur5left"), dt, True)
        lists.append(dict(d, pose=np.resize(np.asarray(d["pose"], dtype=np.float64), (robots,) + np.shape(d["pose"])[1:])))
    q = np.resize(q, (robots, 25))
    return dict(lay=lay, gains=gains, model=model, q=q, qd=np.zeros_like(q), lists=lists, dt=dt)


def arm(fl, limit, episodes=0, poll_every=0, records=16, with_episodes=True):
    """A context with the fleet on slot 0: start states, targets (every arm holds where it is), the list with variant 0 and -- unless
    with_episodes is off -- the episodes."""
    g, B = fl["gains"], len(fl["q"])
    osc = BatchedOSC(fl["lay"], B, dtype=np.float64)
    osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], g["max_vel"], g["null_kv"])
    osc.set_model(fl["model"])
    osc.set_plant(fl["dt"])
    osc.upload_q(fl["q"], fl["qd"])
    osc.frontend()
    osc.set_targets(osc.download_records(keys=("ee_pose",))["ee_pose"])
    osc.set_action_list(fl["lists"][0])
    if with_episodes:
        osc.set_episodes(fl["q"][:, None], fl["qd"][:, None], max_ticks=limit, max_episodes=episodes, poses=np.stack([d["pose"] for d in fl["lists"]]),
                         records=records, poll_every=poll_every)
    return osc


def run(robots=32, ticks=20000, limit=4000, variants=3, episodes=0, seed=0, verbose=True):
    fl = build(robots, variants, seed)
    osc = arm(fl, limit, episodes, poll_every=64 if episodes else 0)
    t0 = time.perf_counter()
    out = osc.rollout(ticks)
    dt = time.perf_counter() - t0
    st = osc.episode_state()
    osc.close()
    rec = st["records"].reshape(-1, 4)
    rec = rec[rec[:, 1] > 0]
    fin, tmo = int((rec[:, 2] == _lib.EPISODE_FINISHED).sum()), int((rec[:, 2] == _lib.EPISODE_TIMEOUT).sum())
    if verbose:
        print(f"{robots} robots, {out['ticks_run']} ticks in one call ({dt:.2f} s): {int(st['count'].sum())} episodes ended, "
              f"{st['count'].sum() / dt:.1f} episodes/s; {st['running']} robots still running")
        print(f"of the {len(rec)} episodes on record: {fin} FINISHED, {tmo} TIMEOUT (limit {limit} ticks)")
        if len(rec):
            hist, edges = np.histogram(rec[:, 1], bins=8, range=(0, limit))
            for h, lo, hi in zip(hist, edges[:-1], edges[1:]):
                print(f"  {int(lo):6d} .. {int(hi):6d} ticks: {'#' * int(np.ceil(40 * h / max(1, hist.max())))} {h}")
    return dict(count=st["count"], records=st["records"], ticks_run=out["ticks_run"], seconds=dt, finished=fin, timeout=tmo)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=32)
    ap.add_argument("--ticks", type=int, default=20000)
    ap.add_argument("--limit", type=int, default=4000, help="time limit of an episode in ticks")
    ap.add_argument("--variants", type=int, default=3, help="sets of object poses per robot, taken in turn")
    ap.add_argument("--episodes", type=int, default=0, help="episodes per robot (0: no limit, the call runs all its ticks)")
    a = ap.parse_args()
    r = run(a.robots, a.ticks, a.limit, a.variants, a.episodes)
    sys.exit(0 if r["count"].sum() > 0 else 1)
