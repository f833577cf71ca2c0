#!/usr/bin/env python3
"""Rates of a rollout whose carried objects have a weight (BatchedOSC.set_object_loads -> csrc/osc_object_load.hpp), float64, k13,
ms per tick of rollout(--ticks).  Four legs:
    parent       with --parent-tree PATH (a checkout of the parent commit with its library built: its irl_control_amd package is the one
                 the leg imports): the insertion fleet of tools/object_rates.py with objects and refs (1 024 distinct robots repeated to
                 --batch, no joint rows, the hands stay open) -- the parent has no loads
    none         the same fleet on this build, without loads: THE ONE CONDITION is that it agrees with `parent`
    carry        this build's CARRY fleet (examples/insertion_carry_resident_headless.py: joint rows drive the hand, the plug is grasped
                 about 140 ticks in and carried; 1 024 distinct robots repeated to --batch), without loads
    carry_loads  the same fleet, the plug weighing the example's MASS: two more launches per tick (APPLY; SENSE on a slot with a feed --
                 the fleet has a feed of zero sensordata in both CARRY legs, so that SENSE runs)
Every leg is a child process of its own (a process loads one library), and the legs are INTERLEAVED --rounds times, so that a drift of
the machine shows up as spread inside every leg, not as a difference between legs.
    python tools/object_load_rates.py [--batch 65536] [--ticks 200] [--rounds 3] [--parent-tree PATH] [--md profiles/object_load_rates_measured.md]
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
DISTINCT = 1024


def insertion_fleet(a):
    """tools/object_rates.py's leg with objects and refs"""
    import insertion_episodes_resident_headless as ex
    from irl_control_amd import objects as ob
    from irl_control_amd.rigid_body import RigidBodyModel
    fl = ex.build(a.batch, 1, seed=0, distinct=DISTINCT)
    d = fl["lists"][0]
    pose0 = np.ascontiguousarray(d["pose"][:, [0, 2]])
    table = np.array(d["pose"])
    table[:, [0, 2]] = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    fl = dict(fl, lists=[dict(d, pose=table)])
    osc = ex.arm(fl, 0, with_episodes=False)
    names = list(fl["lay"].dev_names)
    kn = RigidBodyModel.load("dual_ur5").joint_names.index("right_outer_knuckle_joint_ur5right")
    osc.set_objects(ob.ObjectSet(radius=[0.03, 0.03], grippers=[ob.Gripper(dev=names.index("ur5right"), joint=kn, q_close=0.3, q_open=0.15)],
                                 mates=[ob.Mate(plug=0, socket=1, tol_xyz=0.03, min_abs_dot=0.99)]), pose0)
    osc.set_action_refs([0, -1, 1, -1], [0, -1, 1, -1])
    return osc, fl["lay"].n


def carry_fleet(a, loads):
    import gripper_fleet_resident_headless as grip
    import insertion_carry_resident_headless as ex
    B = a.batch
    osc = ex.make_ctx(B)
    osc.set_ft_sensors()
    D = min(DISTINCT, B)
    q, near, over = (x[0] for x in ex.carry_states(D, 0))
    start = ex.fk(osc, q)
    sc = ex.carry_scenario(osc.layout, ex.fk(osc, near), ex.fk(osc, over), start)
    rep = lambda x: np.ascontiguousarray(np.tile(x, (-(-B // D),) + (1,) * (x.ndim - 1))[:B])      # noqa: E731
    qB = rep(q)
    osc.upload_q(qB, np.zeros_like(qB))
    osc.set_targets(rep(start))
    osc.set_sensordata(np.zeros((B, 18)))
    osc.set_action_list(dict(sc["desc"], pose=rep(sc["desc"]["pose"])))
    osc.set_joints(grip.scene_rows())
    osc.set_objects(sc["objs"], rep(sc["pose0"]))
    if loads:
        osc.set_object_loads(ex.carry_loads(ex.MASS))
    osc.set_action_refs(sc["refs"]["xyz_obj"], sc["refs"]["quat_obj"])
    return osc, osc.layout.n


def child(a):
    """One leg in this process: -> a JSON line."""
    if a.leg == "parent":      # the parent's package and library, imported ahead of the examples (which then find it loaded)
        sys.path.insert(0, os.path.abspath(a.parent_tree))
    import irl_control_amd
    from irl_control_amd import _lib
    assert (a.leg == "parent") == (os.path.abspath(a.parent_tree or "/nowhere") in os.path.abspath(irl_control_amd.__file__)), irl_control_amd.__file__
    osc, n = insertion_fleet(a) if a.leg in ("parent", "none") else carry_fleet(a, a.leg == "carry_loads")
    B = a.batch
    u, fl_any = np.empty((B, n)), np.empty(B, np.uint32)

    def call(ticks):
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, ticks, 0, None, _lib.ptr(u), _lib.ptr(fl_any)))
        return time.perf_counter() - t0

    call(16)                                                # warm-up (exchange buffers, lane records, code objects)
    times = [call(a.ticks) / a.ticks * 1e3 for _ in range(a.reps)]
    extra = {}
    if a.leg.startswith("carry"):
        extra["holding"] = int((osc.object_state()["holder"][:, 0] >= 0).sum())
    if a.leg == "carry_loads":
        extra["carry_ticks_max"] = int(osc.object_load_state()["carry_ticks"].max())
    osc.close()
    print("RESULT " + json.dumps(dict(leg=a.leg, ms_per_tick=times, **extra)), flush=True)


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
    legs = (["parent"] if a.parent_tree else []) + ["none", "carry", "carry_loads"]
    res = {k: [] for k in legs}
    rows = []
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
            rows.append(f"round {r} {leg:12s} " + " ".join(f"{t:.4f}" for t in o["ms_per_tick"]) + " ms per tick" +
                        "".join(f", {k} {v}" for k, v in o.items() if k not in ("leg", "ms_per_tick")))
            print(rows[-1], flush=True)
    names = dict(parent="parent commit, insertion fleet with objects", none="this build, the same fleet, no loads",
                 carry="this build, CARRY fleet, no loads", carry_loads="this build, CARRY fleet, loads")
    lines = [f"| leg ({a.batch} robots, {a.ticks} ticks per call, {a.rounds} rounds x {a.reps} calls, interleaved) | best ms/tick | ticks/s at best | median | "
             "spread (max - min) | spread without the first calls |", "|---|---|---|---|---|---|"]
    for leg in legs:
        t = np.array(res[leg])
        later = np.array([x for i, x in enumerate(res[leg]) if i % a.reps])
        lines.append(f"| {names[leg]} | {t.min():.4f} | {1e3 / t.min():.0f} | {np.median(t):.4f} | {t.max() - t.min():.4f} | {later.max() - later.min():.4f} |")
    print("\n".join(lines))
    if a.md:
        with open(a.md, "a") as f:
            f.write("\n".join(rows) + "\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
