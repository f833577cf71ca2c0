#!/usr/bin/env python3
"""Rates of a rollout with a reward (BatchedOSC.set_reward -> csrc/osc_reward.hpp), float64, k13, ms per tick of rollout(--ticks), on the
policy fleets of tools/policy_rates.py.  Legs:
    policy_small, policy_big   this build, the two policy fleets WITHOUT a reward
    episodes                   this build, the small fleet with episodes (max_ticks 64, one shared start) and no reward
    parent_policy_small, parent_policy_big, parent_episodes   with --parent-tree PATH (a checkout of the parent commit with its library
                               built): the same three on the parent's package and library.  THE ONE CONDITION: each leg of this build lies
                               inside its parent leg's run-to-run band -- a slot without a reward launches what it launched before, and
                               only the episode kernel differs, by one uniform branch
    reach                      the small fleet + a reach reward: DIST(EE 0, FIXED 0) and ONE           -- against policy_small
    full8_base, full8          the big fleet (feed) with two action objects and a mate, without / with the eight-term list (every kind)
    reach_goal                 the small fleet + the reach reward with a goal (never reached: the tick's cost, not shorter episodes) and
                               episodes                                                                 -- against episodes
A reward's cost is its leg's median minus its base leg's median, set against THE FLOOR: the bytes the reward kernel (and, reach_goal, the
episode kernel's extra loads) moves per robot over --hbm-tbs, the rate a copy reaches on an MI355X in this project's profiles.
Every leg is a child process of its own and the legs are INTERLEAVED --rounds times (tools/policy_rates.py: why).
    python tools/reward_rates.py [--batch 65536] [--ticks 200] [--rounds 3] [--parent-tree PATH] [--md FILE]
Prints the kernel_regs lines of the reward kernels, one line per leg and round, then the table, and appends all of it to --md when given:
the raw material of profiles/reward_rates.md, which quotes it."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
BASE = dict(reach="policy_small", full8="full8_base", reach_goal="episodes")
# bytes per robot and tick.  State: r ret gret disc (load 3, store 4 doubles), steps (4 + 4); a goal adds hold and goal_step (8 + 8).
STATE = 7 * 8 + 8
BYTES = dict(reach=STATE + 3 * 8,                                  # three EE words (the fleet's point comes from the cache)
             # the eight terms: 3 EE + 3 FIXED-side words, target row 21 + 3 object words, 4 + 4 quaternion words (EE, target row shared),
             # act 7 floats, u 25 doubles, wrench row 18 doubles, mated_tick
             full8=STATE + (3 + 3 + 4) * 8 + 21 * 8 + 7 * 4 + 25 * 8 + 18 * 8 + 4,
             reach_goal=STATE + 16 + 3 * 8 + 4)                    # ... and the episode kernel's goal_step load


def parts(leg):
    parent = leg.startswith("parent_")
    return leg[len("parent_"):] if parent else leg, parent


def child(a):
    """One leg in this process: -> a JSON line."""
    name, parent = parts(a.leg)
    if parent:
        sys.path.insert(0, os.path.abspath(a.parent_tree))
    import irl_control_amd
    from irl_control_amd import _lib, policy
    assert parent == (os.path.abspath(a.parent_tree or "/nowhere") in os.path.abspath(irl_control_amd.__file__)), irl_control_amd.__file__
    import policy_rates as pr
    osc, lay, origin = pr.fleet(a)
    B, n = a.batch, lay.n
    big = name in ("policy_big", "full8_base", "full8")
    obs, hidden, n_out = pr.NETS["policy_big" if big else "policy_small"]
    n_in = policy.obs_width(policy.obs_mask(obs), n, lay.ndev)
    rng = np.random.default_rng(1)
    dims = (n_in,) + hidden + (n_out,)
    layers = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), 0.1 * rng.standard_normal(o).astype(np.float32)) for i, o in zip(dims[:-1], dims[1:])]
    if big:
        osc.set_ft_sensors()
        osc.set_sensordata(np.zeros((B, 18)))
    osc.set_policy(layers, obs, origin, clip=60.0, grip_dev=0, grip_close=0.08, grip_open=-0.08)
    q0 = osc.download_q()[0]
    if name in ("full8_base", "full8"):
        from irl_control_amd import objects as ob
        pose0 = np.tile([0.3, 0.4, 0.6, 1.0, 0, 0, 0], (B, 2, 1)).astype(np.float64)
        pose0[:, 1, 0] += 0.5
        osc.set_objects(ob.ObjectSet(radius=[0.05, 0.05], grippers=[ob.Gripper(dev=0, joint=6, q_close=0.3, q_open=0.15)],
                                     mates=[ob.Mate(plug=0, socket=1, tol_xyz=0.01)]), pose0)
    if name in ("reach", "reach_goal", "full8"):
        from irl_control_amd import reward as rw
        pts = np.array([[0.3, 0.4, 0.6]])
        if name == "full8":
            desc = rw.Reward([rw.dist(rw.ee(0), rw.fixed(0), -1.0), rw.dist_sq(rw.target(1), rw.obj(0), 0.3), rw.ori(rw.ee(2), rw.target(2), -0.5), rw.act_sq(-0.01),
                              rw.u_sq(-1e-4), rw.force(0, -0.3), rw.mated(0, 2.0), rw.one(-0.05)], gamma=0.99, points=pts)
        else:
            goal = dict(goal_term=0, goal_value=1e-9, goal_hold=3) if name == "reach_goal" else {}
            desc = rw.Reward([rw.dist(rw.ee(0), rw.fixed(0), -1.0), rw.one(-0.05)], gamma=0.99, points=pts, **goal)
        osc.set_reward(desc)
    if name in ("episodes", "reach_goal"):
        osc.set_episodes(q0[:1], max_ticks=64)
    u, fl_any = np.empty((B, n)), np.empty(B, np.uint32)

    def call(ticks):
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, ticks, 0, None, _lib.ptr(u), _lib.ptr(fl_any)))
        return time.perf_counter() - t0

    call(16)                                                # warm-up (exchange buffers, lane records, code objects)
    times = [call(a.ticks) / a.ticks * 1e3 for _ in range(a.reps)]
    extra = {}
    if name in BASE:
        st = osc.reward_state()
        extra = dict(mean_r=float(np.nanmean(st["r"])), finite=int(np.isfinite(st["ret"]).sum()))
    osc.close()
    print("RESULT " + json.dumps(dict(leg=a.leg, ms_per_tick=times, frozen=int((fl_any & 65 != 0).sum()), **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="TB/s a copy reaches (profiles/NOTES.md); the peak is 8")
    ap.add_argument("--md", default=None)
    ap.add_argument("--legs", default=None, help="comma-separated legs (default: all; the parent legs with --parent-tree)")
    ap.add_argument("--leg", default=None, help="(internal) run this one leg")
    a = ap.parse_args()
    if a.leg:
        return child(a)
    regs = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "reward"], capture_output=True, text=True).stdout.strip()
    print(regs, flush=True)
    mine = ["policy_small", "policy_big", "episodes"]
    legs = a.legs.split(",") if a.legs else [x for m in mine for x in ((["parent_" + m] if a.parent_tree else []) + [m])] + ["reach", "full8_base", "full8", "reach_goal"]
    if any(parts(leg)[1] for leg in legs) and not a.parent_tree:
        raise SystemExit("a parent_* leg needs --parent-tree")
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
            rows.append(f"round {r} {leg:20s} " + " ".join(f"{t:.4f}" for t in o["ms_per_tick"]) + f" ms per tick, frozen {o['frozen']}" +
                        (f", mean r {o['mean_r']:.4g}, finite returns {o['finite']}" if "mean_r" in o else ""))
            print(rows[-1], flush=True)
    lines = [f"| leg ({a.batch} robots, {a.ticks} ticks per call, {a.rounds} rounds x {a.reps} calls, interleaved) | best ms/tick | median | min .. max | "
             "inside the parent's band / cost over its base (medians, us) | floor us (bytes per robot) | cost / floor |", "|---|---|---|---|---|---|---|"]
    for leg in legs:
        t = np.array(res[leg])
        name, parent = parts(leg)
        note = floor = ratio = ""
        if not parent and "parent_" + name in res:
            pt = np.array(res["parent_" + name])
            note = f"parent band {pt.min():.4f} .. {pt.max():.4f}: " + ("inside" if pt.min() <= np.median(t) <= pt.max() else "OUTSIDE") + f" (median {np.median(t) - np.median(pt):+.4f} ms)"
        if name in BASE and BASE[name] in res:
            cost = (np.median(t) - np.median(res[BASE[name]])) * 1e3
            fl = BYTES[name] * a.batch / (a.hbm_tbs * 1e12) * 1e6
            note, floor, ratio = f"{cost:+.1f} over {BASE[name]}", f"{fl:.2f} ({BYTES[name]})", f"{cost / fl:.1f}"
        lines.append(f"| {leg} | {t.min():.4f} | {np.median(t):.4f} | {t.min():.4f} .. {t.max():.4f} | {note} | {floor} | {ratio} |")
    print("\n".join(lines))
    if a.md:
        with open(a.md, "a") as f:
            f.write("```\n" + regs + "\n```\n\n" + "\n".join(rows) + "\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
