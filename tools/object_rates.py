#!/usr/bin/env python3
"""Rates of a rollout with action objects (BatchedOSC.set_objects / set_action_refs -> csrc/osc_object.hpp), float64, the insertion fleet
of examples/insertion_episodes_resident_headless.py on k13 (1 024 distinct robots repeated to --batch, no episodes):
    ms per tick of rollout(--ticks) on this build WITHOUT objects and WITH objects -- the male part at the first waypoint's pose, the
    female part at the third's, one gripper on the right arm, one mate, the list's waypoints aiming at them through refs (offset 0,
    grip rotation 1: the same targets) -- and, with --parent-tree PATH (a checkout of the parent commit with its library built: its
    irl_control_amd package is the one the leg imports), of the same rollout without objects on the parent.
The fleet has no joint rows, so its hands stay open and every object stays free: the object kernel's tick is the one of free objects
(EE pose, knuckle, holders, edge detector, the mate's test), not the carry.
Every leg is a child process of its own (a process loads one library), and the legs are INTERLEAVED --rounds times, so that a drift of
the machine shows up as spread inside every leg, not as a difference between legs.
    python tools/object_rates.py [--batch 65536] [--ticks 200] [--rounds 3] [--parent-tree PATH] [--md profiles/object_rates_measured.md]
Prints one line per leg and round, then the table (best, median and spread per leg), and appends it to --md when given."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def child(a):
    """One leg in this process: -> a JSON line."""
    if a.leg == "parent":      # the parent's package and library, imported ahead of the example (which then finds it loaded)
        sys.path.insert(0, os.path.abspath(a.parent_tree))
    import irl_control_amd
    from irl_control_amd import _lib
    assert (a.leg == "parent") == (os.path.abspath(a.parent_tree or "/nowhere") in os.path.abspath(irl_control_amd.__file__)), irl_control_amd.__file__
    import insertion_episodes_resident_headless as ex
    fl = ex.build(a.batch, 1, seed=0, distinct=1024)
    d = fl["lists"][0]
    if a.leg == "objects":      # the same targets, composed on the GPU from the objects' poses
        pose0 = np.ascontiguousarray(d["pose"][:, [0, 2]])
        table = np.array(d["pose"])
        table[:, [0, 2]] = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
        fl = dict(fl, lists=[dict(d, pose=table)])
    osc = ex.arm(fl, 0, with_episodes=False)
    if a.leg == "objects":
        from irl_control_amd import objects as ob
        from irl_control_amd.rigid_body import RigidBodyModel
        names = list(fl["lay"].dev_names)
        kn = RigidBodyModel.load("dual_ur5").joint_names.index("right_outer_knuckle_joint_ur5right")
        osc.set_objects(ob.ObjectSet(radius=[0.03, 0.03], grippers=[ob.Gripper(dev=names.index("ur5right"), joint=kn, q_close=0.3, q_open=0.15)],
                                     mates=[ob.Mate(plug=0, socket=1, tol_xyz=0.03, min_abs_dot=0.99)]), pose0)
        osc.set_action_refs([0, -1, 1, -1], [0, -1, 1, -1])
    B, n = a.batch, fl["lay"].n
    u, fl_any = np.empty((B, n)), np.empty(B, np.uint32)

    def call(ticks):
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, ticks, 0, None, _lib.ptr(u), _lib.ptr(fl_any)))
        return time.perf_counter() - t0

    call(16)                                                # warm-up (exchange buffers, lane records, code objects)
    times = [call(a.ticks) / a.ticks * 1e3 for _ in range(a.reps)]
    osc.close()
    print("RESULT " + json.dumps(dict(leg=a.leg, ms_per_tick=times)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--leg", default=None, help="(internal) run this one leg")
    a = ap.parse_args()
    if a.leg:
        return child(a)
    legs = (["parent"] if a.parent_tree else []) + ["none", "objects"]
    res = {k: [] for k in legs}
    for r in range(a.rounds):
        for leg in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(a.batch), "--ticks", str(a.ticks), "--reps", str(a.reps)] + \
                  (["--parent-tree", a.parent_tree] if a.parent_tree else [])
            p = subprocess.run(cmd, env=dict(os.environ), capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode or not line:
                print(p.stdout[-2000:], p.stderr[-2000:])
                raise SystemExit(f"leg {leg} failed ({p.returncode}): nothing more is started")
            o = json.loads(line[0][7:])
            res[leg] += o["ms_per_tick"]
            print(f"round {r} {leg:8s} " + " ".join(f"{t:.4f}" for t in o["ms_per_tick"]) + " ms per tick", flush=True)
    names = dict(parent="parent commit, no objects", none="this build, no objects", objects="this build, objects and refs")
    lines = [f"| leg ({a.batch} robots, {a.ticks} ticks per call, {a.rounds} rounds x {a.reps} calls, interleaved) | best ms/tick | ticks/s at best | median | "
             "spread (max - min) | spread without the first calls |", "|---|---|---|---|---|---|"]
    for leg in legs:
        t = np.array(res[leg])
        later = np.array([x for i, x in enumerate(res[leg]) if i % a.reps])
        lines.append(f"| {names[leg]} | {t.min():.4f} | {1e3 / t.min():.0f} | {np.median(t):.4f} | {t.max() - t.min():.4f} | {later.max() - later.min():.4f} |")
    print("\n".join(lines))
    if a.md:
        with open(a.md, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
