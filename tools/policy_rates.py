#!/usr/bin/env python3
"""Rates of a rollout under a policy (BatchedOSC.set_policy -> csrc/osc_policy.hpp), float64, k13, ms per tick of rollout(--ticks).  Legs:
    parent_stream  with --parent-tree PATH (a checkout of the parent commit with its library built: its irl_control_amd package is the one
                   the leg imports): the space-mouse fleet of examples/space_mouse_resident_headless.py, one looping stream for the fleet
    stream         the same fleet on this build: THE ONE CONDITION is that it agrees with `parent_stream` -- a slot without a policy pays nothing
    policy_small   this build, the same fleet under a policy on PLATE alone, 6 -> 64 -> 64 -> 6
    policy_big     this build, a policy on every channel the fleet has (qpos qvel ee_pose targets wrench plate = 116 on k13) -> 128 -> 128 -> 7
    parent_policy_small, parent_policy_big   with --parent-tree: the two policy fleets on the parent's package and library
    policy_small_noise, policy_big_noise     this build, the two policy fleets with a Gaussian head (set_policy_noise, every std 0.1): the
                   NOISE form of the kernel.  Reported as the leg's median minus the median of the same fleet without a head, next to
                   THE HEAD'S FLOOR: the --head-valu VALU instructions one draw piece adds to a wave (counted from the kernel's listing: the
                   NOISE = true form minus the NOISE = false form) at 4 cycles each, the fleet's blocks over the chip's SIMDs
    bench_parent, bench   the benchmark's headline (bench.py --gpus 1) in the parent tree and in this one
--legs a,b,... picks the legs (default: parent_stream, stream, policy_small, policy_big -- the legs of profiles/policy_rates.md).
Every leg is a child process of its own (a process loads one library), and the legs are INTERLEAVED --rounds times, so that a drift of
the machine shows up as spread inside every leg, not as a difference between legs.  The policy legs are set against the ARITHMETIC FLOOR
of their network: sum over layers of 4 ceil(out / 16) ceil(in / 4) instructions v_mfma_f32_16x16x4_f32 per 64 robots at 32 cycles each per
SIMD, the waves spread over the chip's SIMDs at --clock-ghz.
    python tools/policy_rates.py [--batch 65536] [--ticks 200] [--rounds 3] [--parent-tree PATH] [--md profiles/policy_rates_measured.md]
Prints the kernel_regs table of the policy kernels, one line per leg and round, then the table, and appends all of it to --md when given."""
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
NETS = {"policy_small": (("plate",), (64, 64), 6), "policy_big": (("qpos", "qvel", "ee_pose", "targets", "wrench", "plate"), (128, 128), 7)}
SIMDS = 256 * 4


def floor_instructions(n_in, hidden, n_out):
    dims = (n_in,) + tuple(hidden) + (n_out,)
    return sum(4 * -(-o // 16) * -(-i // 4) for i, o in zip(dims[:-1], dims[1:]))


def floor_ms(instr, batch, clock_ghz):
    waves = -(-batch // 64)
    return -(-waves // SIMDS) * instr * 32 / (clock_ghz * 1e9) * 1e3


def fleet(a):
    """The space-mouse fleet: -> (osc, layout, origin)"""
    import space_mouse_resident_headless as ex
    from irl_control_amd import BatchedOSC, synth, teleop
    from irl_control_amd.rigid_body import RigidBodyModel
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    osc = BatchedOSC(lay, a.batch, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(1e-3, 0.0)
    D = min(1024, a.batch)
    q = np.ascontiguousarray(np.tile(ex.start_states(D, 5), (-(-a.batch // D), 1))[:a.batch])
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    osc.set_targets(osc.download_records(keys=("ee_pose",))["ee_pose"].copy())
    osc.upload_q(q, np.zeros_like(q))
    return osc, lay, np.array(teleop.ORIGIN)


def parts(leg):
    """leg -> (the fleet: "stream" or a name of NETS, on the parent's build, with a Gaussian head)"""
    parent, noise = leg.startswith("parent_"), leg.endswith("_noise")
    return leg[len("parent_") if parent else 0:len(leg) - (len("_noise") if noise else 0)], parent, noise


def child(a):
    """One leg in this process: -> a JSON line."""
    net, parent, noise = parts(a.leg)
    if parent:      # the parent's package and library, imported ahead of the examples (which then find it loaded)
        sys.path.insert(0, os.path.abspath(a.parent_tree))
    import irl_control_amd
    from irl_control_amd import _lib, teleop
    assert parent == (os.path.abspath(a.parent_tree or "/nowhere") in os.path.abspath(irl_control_amd.__file__)), irl_control_amd.__file__
    import teleop_loops as tl
    osc, lay, origin = fleet(a)
    B, n = a.batch, lay.n
    if net in NETS:
        from irl_control_amd import policy
        obs, hidden, n_out = NETS[net]
        n_in = policy.obs_width(policy.obs_mask(obs), n, lay.ndev)
        rng = np.random.default_rng(1)
        dims = (n_in,) + hidden + (n_out,)
        layers = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), 0.1 * rng.standard_normal(o).astype(np.float32))
                  for i, o in zip(dims[:-1], dims[1:])]
        if "wrench" in obs:
            osc.set_ft_sensors()
            osc.set_sensordata(np.zeros((B, 18)))
        osc.set_policy(layers, obs, origin, clip=60.0, grip_dev=0, grip_close=0.08, grip_open=-0.08)
        if noise:
            osc.set_policy_noise(np.full(n_out, 0.1, np.float32), seed=7)
    else:
        osc.set_teleop_stream(teleop.record_readings(tl.space_mouse_stream(5, 256), 256), origin, loop=True)
    u, fl_any = np.empty((B, n)), np.empty(B, np.uint32)

    def call(ticks):
        t0 = time.perf_counter()
        osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, B, ticks, 0, None, _lib.ptr(u), _lib.ptr(fl_any)))
        return time.perf_counter() - t0

    call(16)                                                # warm-up (exchange buffers, lane records, code objects)
    times = [call(a.ticks) / a.ticks * 1e3 for _ in range(a.reps)]
    osc.close()
    print("RESULT " + json.dumps(dict(leg=a.leg, ms_per_tick=times, frozen=int((fl_any & 65 != 0).sum()))), flush=True)


def bench(tree, steps, warmup):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree, capture_output=True,
                       text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode or not line:
        print(p.stdout[-2000:], p.stderr[-2000:])
        raise SystemExit(f"bench.py in {tree} failed ({p.returncode}): nothing more is started")
    return json.loads(line[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=200, help="0: no benchmark legs")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--md", default=None)
    ap.add_argument("--legs", default=None, help="comma-separated legs (default: the stream and policy legs)")
    ap.add_argument("--head-valu", type=int, default=0, help="VALU instructions the head adds to a wave (from the listing): the head's floor")
    ap.add_argument("--leg", default=None, help="(internal) run this one leg")
    a = ap.parse_args()
    if a.leg:
        return child(a)
    regs = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "policy"], capture_output=True, text=True).stdout.strip()
    print(regs, flush=True)
    legs = a.legs.split(",") if a.legs else (["parent_stream"] if a.parent_tree else []) + ["stream", "policy_small", "policy_big"]
    if any(parts(leg)[1] for leg in legs) and not a.parent_tree:
        raise SystemExit("a parent_* leg needs --parent-tree")
    res = {k: [] for k in legs}
    rows, heads = [], {}
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
            rows.append(f"round {r} {leg:14s} " + " ".join(f"{t:.4f}" for t in o["ms_per_tick"]) + f" ms per tick, frozen {o['frozen']}")
            print(rows[-1], flush=True)
        for name, tree in (("bench_parent", a.parent_tree), ("bench", ROOT)):
            if a.bench_steps and tree:
                o = bench(tree, a.bench_steps, 20)
                heads.setdefault(name, []).append(o)
                rows.append(f"round {r} {name:14s} " + json.dumps(o))
                print(rows[-1], flush=True)
    fleets = dict(stream="stream fleet", policy_small="policy PLATE 6 -> 64 -> 64 -> 6", policy_big="policy every channel 116 -> 128 -> 128 -> 7")
    lines = [f"| leg ({a.batch} robots, {a.ticks} ticks per call, {a.rounds} rounds x {a.reps} calls, interleaved) | best ms/tick | ticks/s at best | median | "
             "spread (max - min) | over the stream fleet / a head: over the same fleet without one (medians) | floor ms (MFMA / a head: its VALU) | cost / floor |",
             "|---|---|---|---|---|---|---|---|"]
    for leg in legs:
        t = np.array(res[leg])
        net, parent, noise = parts(leg)
        cost = floor = ratio = ""
        if noise and net in res:      # the head: over the same fleet without one, against the draw's own floor
            over = np.median(t) - np.median(res[net])
            fm = -(-(-(-a.batch // 64)) // SIMDS) * a.head_valu * 4 / (a.clock_ghz * 1e9) * 1e3
            cost, floor, ratio = f"{over:+.4f}", f"{fm:.4f}" if fm else "", f"{over / fm:.1f}" if fm else ""
        elif net in NETS and not parent and "stream" in res:
            from irl_control_amd import policy, synth
            lay = synth.make_layout("k13")
            obs, hidden, n_out = NETS[net]
            base = np.median(res["stream"])
            fm = floor_ms(floor_instructions(policy.obs_width(policy.obs_mask(obs), lay.n, lay.ndev), hidden, n_out), a.batch, a.clock_ghz)
            cost, floor, ratio = f"{np.median(t) - base:+.4f}", f"{fm:.4f}", f"{(np.median(t) - base) / fm:.1f}"
        name = ("parent commit, " if parent else "this build, ") + fleets[net] + (" + Gaussian head" if noise else "")
        lines.append(f"| {name} | {t.min():.4f} | {1e3 / t.min():.0f} | {np.median(t):.4f} | {t.max() - t.min():.4f} | {cost} | {floor} | {ratio} |")
    print("\n".join(lines))
    if a.md:
        with open(a.md, "a") as f:
            f.write("```\n" + regs + "\n```\n\n" + "\n".join(rows) + "\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
