#!/usr/bin/env python3
"""Rates of the rollout's episodes (BatchedOSC.set_episodes -> csrc/osc_episode.hpp), float64, the insertion fleet of
examples/insertion_episodes_resident_headless.py on k13:
    ms per tick of rollout(--ticks) on this build WITHOUT episodes, WITH episodes, and with episodes and poll_every = 64 -- and, with
    --parent-tree PATH (a checkout of the parent commit with its library built: its irl_control_amd package is the one the leg imports),
    of the same rollout without episodes on the parent;
    episodes per second and the share of useful ticks (ticks inside a running episode) of one long call with episodes, against the
    same fleet run as one episode per call.
Every leg is a child process of its own (a process loads one library), and the legs are INTERLEAVED --rounds times, so that a drift of
the machine shows up as spread inside every leg, not as a difference between legs.
    python tools/episode_rates.py [--batch 65536] [--ticks 200] [--rounds 3] [--limit 120] [--parent-tree PATH] [--md profiles/episode_rates_measured.md]
Prints one line per leg and round, then the table (best and spread per leg), and appends it to --md when given."""
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
    fl = ex.build(a.batch, 3, seed=0, distinct=1024)
    osc = ex.arm(fl, a.limit, poll_every=64 if a.leg == "episodes_poll" else 0, with_episodes=a.leg.startswith("episodes"))
    B, n = a.batch, fl["lay"].n
    u, fl_any = np.empty((B, n)), np.empty(B, np.uint32)

    def call(ticks):
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, ticks, 0, None, _lib.ptr(u), _lib.ptr(fl_any)))
        return time.perf_counter() - t0

    call(16)                                                # warm-up (exchange buffers, lane records, code objects)
    times = [call(a.ticks) / a.ticks * 1e3 for _ in range(a.reps)]
    out = dict(leg=a.leg, ms_per_tick=times)
    if a.leg == "episodes":                                 # one long call: episodes per second, and what one episode per call wastes
        t = call(a.long_ticks)
        st = osc.episode_state()
        rec = st["records"].reshape(-1, 4)
        rec = rec[rec[:, 1] > 0]
        out.update(episodes=int(st["count"].sum()), seconds=t, episodes_per_s=float(st["count"].sum() / t),
                   finished=int((rec[:, 2] == _lib.EPISODE_FINISHED).sum()), timeout=int((rec[:, 2] == _lib.EPISODE_TIMEOUT).sum()),
                   mean_length=float(rec[:, 1].mean()) if len(rec) else 0.0,
                   # a call per episode runs until its slowest robot is through: every robot's ticks beyond its own length are idle
                   useful_one_episode_per_call=float(rec[:, 1].mean() / rec[:, 1].max()) if len(rec) else 0.0,
                   useful_with_episodes=1.0)                # (no limit on the episodes: every tick of every robot is inside one)
    osc.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--long-ticks", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="time limit of an episode in ticks")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--leg", default=None, help="(internal) run this one leg")
    a = ap.parse_args()
    if a.leg:
        return child(a)
    legs = (["parent"] if a.parent_tree else []) + ["none", "episodes", "episodes_poll"]
    res = {k: [] for k in legs}
    extra = {}
    for r in range(a.rounds):
        for leg in legs:
            env = dict(os.environ)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(a.batch), "--ticks", str(a.ticks), "--reps", str(a.reps),
                   "--limit", str(a.limit), "--long-ticks", str(a.long_ticks)] + (["--parent-tree", a.parent_tree] if a.parent_tree else [])
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode or not line:
                print(p.stdout[-2000:], p.stderr[-2000:])
                raise SystemExit(f"leg {leg} failed ({p.returncode}): nothing more is started")
            o = json.loads(line[0][7:])
            res[leg] += o["ms_per_tick"]
            if leg == "episodes":
                extra = o
            print(f"round {r} {leg:14s} " + " ".join(f"{t:.4f}" for t in o["ms_per_tick"]) + " ms per tick", flush=True)
    names = dict(parent="parent commit, no episodes", none="this build, no episodes", episodes="this build, episodes",
                 episodes_poll="this build, episodes, poll_every = 64")
    lines = [f"| leg ({a.batch} robots, {a.ticks} ticks per call, {a.rounds} rounds x {a.reps} calls, interleaved) | best ms/tick | median | spread (max - min) |", "|---|---|---|---|"]
    for leg in legs:
        t = np.array(res[leg])
        lines.append(f"| {names[leg]} | {t.min():.4f} | {np.median(t):.4f} | {t.max() - t.min():.4f} |")
    if extra:
        lines += ["", f"One call of {a.long_ticks} ticks with episodes (limit {a.limit} ticks): {extra['episodes']} episodes ended in {extra['seconds']:.3f} s = "
                  f"{extra['episodes_per_s']:.0f} episodes/s; on record {extra['finished']} FINISHED, {extra['timeout']} TIMEOUT, mean length "
                  f"{extra['mean_length']:.1f} ticks.  Useful ticks (inside a running episode) / ticks run: {extra['useful_with_episodes']:.2f} with episodes, "
                  f"{extra['useful_one_episode_per_call']:.2f} for the same episodes run one per call (mean length / longest)."]
    print("\n".join(lines))
    if a.md:
        with open(a.md, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
