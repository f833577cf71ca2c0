#!/usr/bin/env python3
"""A fleet that closes its hands on the GPU: B Dual-UR5 robots run a short WP GRIP WP action list inside `rollout`
(BatchedOSC.set_action_list) with the scene's joint rows in force (BatchedOSC.set_joints -> irlosc_set_joints, csrc/osc_joint.hpp):
the range stops of the 24 limited hinges, the ten equality rows that tie each Robotiq finger linkage to its driven knuckle, and the
two gripper motors as ACTION drives -- the GRIP's gripper_force becomes the ctrl of the motor on right_outer_knuckle_joint_<arm>, as
insertion_task.py::send_forces writes it into ctrl[7] / ctrl[14].

Per tick and robot, one train of kernels and nothing across PCIe:
    (qpos, qvel) --walk--> M, J, bias, EE pose --action list--> targets, gripper_force --OSC step--> u
                 --joint rows: tau_j from (q_j, qd_j), bias -= tau--> plant --> (qpos, qvel)
The list: WP to a pose a few centimetres from the start (the FK pose of a nearby configuration), GRIP for --grip-ticks ticks, WP back
to the start position.  A later action with force 0 keeps the grip, as in the reference.

What this is NOT: MuJoCo's soft-constraint solver (the rows are explicit penalties: a spring and a damper per row), friction loss,
fingertip contacts or an object in the hand; the F/T feed does not see these torques.  The penalties are bounded by the explicit
integration: a finger hinge's own inertia is of the order 1e-5 kg m^2, so a stiffness above a few N m / rad diverges at dt = 1 ms
(`stiffness_bound` prints M_jj / dt^2 from the rigid-body oracle).  The values below were chosen with `cpu_loop` -- this scenario in
NumPy: the oracle's M and bias, the oracle's controller, the action list's host restatement, joints.joint_torque and the semi-implicit
Euler of closed_loop_headless.py -- which keeps a closed hand bounded over 2 000 ticks (profiles/joint_rates.md).

    python examples/gripper_fleet_resident_headless.py [--robots 32] [--ticks 600] [--trace-every 50] [--force 0.08]
    python examples/gripper_fleet_resident_headless.py --cpu-loop [--robots 2] [--ticks 600]         # no GPU: the NumPy closed loop
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from irl_control_amd import joints, synth                           # noqa: E402
from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "dual_ur5_joints.json")
# chosen on the CPU (cpu_loop; profiles/joint_rates.md): N m / rad and N m s / rad
LIMIT_K, LIMIT_C, COUPLE_K, COUPLE_C = 2.0, 0.004, 1.0, 0.002
FORCE = 0.08                 # N m on the driven knuckle (gear 1): closes the hand against its upper stop
GRIP_TICKS = 200
# cpu_loop's recorded run (--cpu-loop --record): its parameters, its worst coupling error over 600 ticks and its first ticks, which
# tests/test_joints_host.py repeats -- a change to cpu_loop or to the penalties above shows there, and the record is made again
CPU_RECORD = os.path.join(ROOT, "tests", "golden", "gripper_cpu_loop.json")
Q_RIGHT = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3])          # the insertion fleet's start configurations
Q_LEFT = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2])
WP, GRIP = 0, 1


def start_states(robots, seed=0):
    """-> (q, q_near): the start configurations (arms +- 0.15 rad per joint, hands open, at rest) and, for the first waypoint, the right
    arm moved by up to 0.05 rad per joint"""
    rng = np.random.default_rng(seed)
    q = np.zeros((robots, 25))
    q[:, 1:7] = Q_RIGHT + rng.uniform(-0.15, 0.15, (robots, 6))
    q[:, 13:19] = Q_LEFT + rng.uniform(-0.15, 0.15, (robots, 6))
    near = q.copy()
    near[:, 1:7] += rng.uniform(-0.05, 0.05, (robots, 6))
    return q, near


def scene_rows(drive="action", limit_k=LIMIT_K, limit_c=LIMIT_C, couple_k=COUPLE_K, couple_c=COUPLE_C):
    return joints.scene_rows(FIXTURE, limit_k, limit_c, couple_k, couple_c, drive=drive)


def action_list(robots, ia, io, pose, start, force=FORCE, grip_ticks=GRIP_TICKS):
    """The WP GRIP WP list as the arrays of BatchedOSC.set_action_list / action_sequence.action_list_tick: pose [B, 7] the first
    waypoint of the active arm, start [B, ndev, 7] the EE poses at the start (the last waypoint goes back to the start position)"""
    A = 3
    table = np.zeros((robots, A, 7))
    table[:, :, 3] = 1.0
    table[:, 0], table[:, 2] = pose, start[:, ia]
    return dict(n_actions=A, active_dev=ia, passive_dev=io, passive_hold_orientation=1, passive_quat=np.array([1.0, 0.0, 0.0, 0.0]),
                kind=np.array([WP, GRIP, WP], np.int32), xyz_from_start=np.array([0, 0, 1], np.int32),
                grip_ticks=np.array([1, grip_ticks, 1], np.int32), kp=np.full(A, 2.0), max_error=np.array([0.02, 0.0, 0.05]),
                min_speed=np.full(A, 0.05), max_speed=np.full(A, 1.0), gripper_force=np.array([0.0, force, 0.0]), pose=table)


def hand_rows(desc, names, arm="ur5right"):
    """From the descriptor joints.normalise made of scene_rows(): -> (the arm's driven knuckle hinge, the COUPLE rows of its hand, its
    DRIVE row or None)"""
    kn = names.index(f"right_outer_knuckle_joint_{arm}")
    couple = [r for r in range(len(desc["kind"])) if desc["kind"][r] == joints.COUPLE and names[desc["joint_a"][r]].endswith(arm)]
    drive = [r for r in range(len(desc["kind"])) if desc["kind"][r] == joints.DRIVE and desc["joint_a"][r] == kn]
    return kn, couple, (drive[0] if drive else None)


def cpu_record():
    import json
    with open(CPU_RECORD) as f:
        return json.load(f)


def record_cpu_loop(path, robots=4, ticks=600, head=16):
    """Runs cpu_loop on the oracle-made scenario and writes its parameters, its worst coupling error and its first `head` ticks"""
    import json
    r = cpu_loop(robots, ticks)
    out = dict(robots=robots, ticks=ticks, seed=0, force=FORCE, grip_ticks=GRIP_TICKS, limit_k=LIMIT_K, limit_c=LIMIT_C, couple_k=COUPLE_K,
               couple_c=COUPLE_C, finite=bool(np.all(np.isfinite(r["q"])) and len(r["qd_max"]) == ticks), couple_err_max=float(r["couple_err"].max()), action_end=r["action"][-1].tolist(),
               knuckle_end=r["knuckle"][-1].tolist(), head_knuckle=r["knuckle"][:head].tolist(), head_couple_err=r["couple_err"][:head].tolist())
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def stiffness_bound(dt=1e-3, verbose=True):
    """M_jj / dt^2 of every hinge at the zero configuration, from oracle/rigid_body.py: the stiffness at which an explicit penalty on the
    hinge's own inertia has omega dt = 1 (semi-implicit Euler is unstable from omega dt = 2).  -> dict(name -> N m / rad)"""
    from oracle import rigid_body as rb
    om = rb.Model()
    lay = synth.make_layout("k13")
    M = rb.records(om, lay.as_oracle_dict(), DUAL_UR5_EE, np.zeros(25), np.zeros(25))["M"]
    names = RigidBodyModel.load("dual_ur5").joint_names
    out = {n: float(M[j, j]) / dt ** 2 for j, n in enumerate(names)}
    if verbose:
        fingers = {n: v for n, v in out.items() if "knuckle" in n or "finger" in n}
        lo = min(fingers, key=fingers.get)
        print(f"M_jj / dt^2 at dt = {dt:g} s: finger hinges {min(fingers.values()):.3g} .. {max(fingers.values()):.3g} N m / rad (smallest: {lo}, "
              f"M_jj = {fingers[lo] * dt ** 2:.3g} kg m^2); arm hinges from {min(v for n, v in out.items() if n not in fingers):.3g}")
    return out


def cpu_loop(robots=2, ticks=600, force=FORCE, grip_ticks=GRIP_TICKS, dt=1e-3, damping=0.0, seed=0, verbose=True, scenario=None,
             **penalties):
    """The fleet's scenario in NumPy, no GPU -- the loop the penalties were chosen with: per tick the rigid-body oracle's M, J, bias and
    EE poses, the action list's bookkeeping (action_sequence.action_list_tick: targets, the adaptive velocity limit, gripper_force), the
    OSC oracle's u with the robot's own velocity limit, joints.joint_torque of the scene's rows with their ACTION drives, qacc = M^-1 (u
    - bias - damping qd + tau), semi-implicit Euler.  scenario: dict(q [B, 25], pose [B, 7], start [B, ndev, 7]) as `run` returns it
    (the poses the GPU front end computed); None: the first `robots` start states of `start_states`, the poses from the oracle.
    -> dict(q_log, qd_log [ticks + 1, B, 25]: the coordinates at the start of every tick and after the last; knuckle [ticks, B]: the
    right hand's driven knuckle; couple_err [ticks, B]: the worst |e| of the right hand's couplings; action [ticks, B]; qd_max [ticks]:
    max |qvel| of the finger hinges; bounded: everything finite and the fingers' |qvel| not growing over the last half)."""
    from irl_control_amd import action_sequence as aseq
    from irl_control_amd.layout import pack_gains
    from oracle import osc_oracle
    from oracle import rigid_body as rb
    om = rb.Model()
    lay = synth.make_layout("k13")
    ld = lay.as_oracle_dict()
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    names = RigidBodyModel.load("dual_ur5").joint_names
    ia, io = list(lay.dev_names).index("ur5right"), list(lay.dev_names).index("ur5left")
    ee_of = lambda qq: np.array([rb.records(om, ld, DUAL_UR5_EE, x, np.zeros(25))["ee_pose"] for x in qq])      # noqa: E731
    if scenario is None:
        q, near = start_states(robots, seed)
        scenario = dict(q=q, pose=ee_of(near)[:, ia], start=ee_of(q))
    q = np.array(scenario["q"][:robots], dtype=np.float64)
    robots = len(q)
    alist = action_list(robots, ia, io, scenario["pose"][:robots], scenario["start"][:robots], force, grip_ticks)
    desc, table = joints.normalise(scene_rows(**penalties), names, lay.dev_names, robots)
    kn, hand, _ = hand_rows(desc, names)
    fingers = [j for j, n in enumerate(names) if "knuckle" in n or "finger" in n]
    qd = np.zeros_like(q)
    keys = ("M", "J", "dq", "bias", "ee_pose")
    tgt = np.array(scenario["start"][:robots], dtype=np.float64)
    grec = pack_gains(lay, gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], np.broadcast_to(gains["max_vel"], (robots, lay.ndev, 2)))[0]
    state = aseq.action_list_state(robots)
    ctrl = np.zeros((robots, table.shape[1]))
    knuckle, cerr, qdm, act = np.zeros((ticks, robots)), np.zeros((ticks, robots)), np.zeros(ticks), np.zeros((ticks, robots), np.int32)
    q_log, qd_log = [q.copy()], [qd.copy()]
    for t in range(ticks):
        recs = [rb.records(om, ld, DUAL_UR5_EE, q[b], qd[b]) for b in range(robots)]
        r = {k: np.array([x[k] for x in recs]) for k in keys}
        aseq.action_list_tick(state, r["ee_pose"], tgt, grec, alist, t)
        u = osc_oracle.generate_batch(ld, dict(gains, max_vel=grec[:, :, 9:11].copy()), r["M"], r["J"], r["dq"], r["bias"], r["ee_pose"], tgt)
        tau, ctrl, viol = joints.joint_torque(q, qd, desc, table, ctrl, state["gripper_force"], ia)
        knuckle[t], cerr[t], qdm[t], act[t] = q[:, kn], viol[:, hand].max(axis=1), np.abs(qd[:, fingers]).max(), state["action"]
        qacc = np.linalg.solve(r["M"], (u - r["bias"] - damping * qd + tau)[:, :, None])[:, :, 0]
        qd = qd + dt * qacc
        q = q + dt * qd
        q_log.append(q.copy()); qd_log.append(qd.copy())
        if not np.all(np.isfinite(q)):
            knuckle, cerr, qdm, act = knuckle[:t + 1], cerr[:t + 1], qdm[:t + 1], act[:t + 1]
            break
    half = len(qdm) // 2
    bounded = bool(np.all(np.isfinite(q)) and len(qdm) == ticks and qdm[half:].max() <= max(qdm[:half].max(), 1e-9))
    if verbose:
        print(f"cpu loop: {robots} robots, {len(qdm)} of {ticks} ticks, force {force:g} N m for {grip_ticks} ticks: knuckle {knuckle[0].mean():.3f} -> "
              f"{knuckle[-1].mean():.3f} rad, action index at the end {act[-1].tolist()}, worst coupling error {cerr.max():.5g} rad, finger |qvel| max "
              f"first half {qdm[:half].max():.3g}, second half {qdm[half:].max():.3g} rad/s -> {'bounded' if bounded else 'NOT bounded'}")
    return dict(q_log=np.array(q_log), qd_log=np.array(qd_log), knuckle=knuckle, couple_err=cerr, action=act, qd_max=qdm, bounded=bounded, q=q)


def run(robots=32, ticks=600, trace_every=50, force=FORCE, grip_ticks=GRIP_TICKS, seed=0, dt=1e-3, damping=0.0, verbose=True):
    """-> dict(ticks [S]: the traced ticks; q_log, qd_log [S, B, 25]: the coordinates at the start of those ticks; knuckle [S, B]: the
    active hand's driven knuckle; couple_err [S, B]: the worst coupling error of the active hand at that tick; action [S, B];
    entered_grip [B]: robots whose GRIP was entered; ctrl [B]; max_couple_err [B]: the worst coupling error of the active hand over ALL
    ticks (the rows' max_violation); flags_any; q; scenario: dict(q, pose, start) for cpu_loop)."""
    from irl_control_amd import BatchedOSC
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    model = RigidBodyModel.load("dual_ur5")
    names = model.joint_names
    ia, io = list(lay.dev_names).index("ur5right"), list(lay.dev_names).index("ur5left")
    q, near = start_states(robots, seed)
    qd = np.zeros_like(q)
    osc = BatchedOSC(lay, robots, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    osc.set_plant(dt, damping)
    osc.upload_q(near, qd)
    osc.frontend()
    pose = osc.download_records(keys=("ee_pose",))["ee_pose"][:, ia].copy()      # the first waypoint: reachable by construction
    osc.upload_q(q, qd)
    osc.frontend()
    start = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()
    osc.set_targets(start)
    osc.set_action_list(action_list(robots, ia, io, pose, start, force, grip_ticks))
    rows = scene_rows()
    osc.set_joints(rows)
    d, tab = joints.normalise(rows, names, lay.dev_names, robots)
    kn, hand, r_drive = hand_rows(d, names)
    flags = np.zeros(robots, np.uint32)
    log = dict(ticks=[], q_log=[], qd_log=[], knuckle=[], couple_err=[], action=[])
    done, out = 0, None
    while done < ticks:
        qn, qdn = osc.download_q()
        viol = joints.joint_torque(qn, qdn, d, tab, np.zeros((robots, len(rows))))[2]
        st = osc.action_state()
        log["ticks"].append(done); log["q_log"].append(qn); log["qd_log"].append(qdn)
        log["knuckle"].append(qn[:, kn]); log["couple_err"].append(viol[:, hand].max(axis=1)); log["action"].append(st["action"])
        if verbose:
            print(f"  tick {done:5d}: knuckle median {np.median(qn[:, kn]):7.4f} rad (min {qn[:, kn].min():7.4f}, max {qn[:, kn].max():7.4f}); worst "
                  f"coupling error {viol[:, hand].max():.4g} rad; action index min {st['action'].min()} max {st['action'].max()}")
        n = min(trace_every, ticks - done)
        out = osc.rollout(n)
        flags |= out["flags_any"]
        done += n
    js, st = osc.joint_state(), osc.action_state()
    osc.close()
    entered = js["ctrl"][:, r_drive] != 0.0
    frozen = flags & (64 | 1) != 0                           # IRLOSC_FLAG_NONFINITE | IRLOSC_FLAG_M_NOT_PD
    res = dict({k: np.array(v) for k, v in log.items()}, entered_grip=entered, ctrl=js["ctrl"][:, r_drive], knuckle_end=out["qpos"][:, kn],
               max_couple_err=js["max_violation"][:, hand].max(axis=1), flags_any=flags, q=out["qpos"], qd=out["qvel"], action_end=st["action"],
               scenario=dict(q=q, pose=pose, start=start))
    if verbose:
        print(f"{robots} robots, {ticks} ticks of {dt * 1e3:g} ms, force {force:g} N m for {grip_ticks} ticks; limits k {LIMIT_K:g} c {LIMIT_C:g}, "
              f"couplings k {COUPLE_K:g} c {COUPLE_C:g}")
        print(f"  robots whose GRIP was entered: {int(entered.sum())}; their driven knuckle at the end: median "
              f"{np.median(res['knuckle_end'][entered]) if entered.any() else 0:.4f} rad; worst coupling error of the active hand over all ticks "
              f"{res['max_couple_err'].max():.4g} rad; robots frozen by the plant at some tick: {int(frozen.sum())}")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=None)
    ap.add_argument("--ticks", type=int, default=None)
    ap.add_argument("--trace-every", type=int, default=50)
    ap.add_argument("--force", type=float, default=FORCE)
    ap.add_argument("--grip-ticks", type=int, default=GRIP_TICKS)
    ap.add_argument("--cpu-loop", action="store_true")
    ap.add_argument("--record", default=None, help="with --cpu-loop: write the run's record (tests/golden/gripper_cpu_loop.json)")
    a = ap.parse_args()
    if a.cpu_loop:
        stiffness_bound()
        if a.record:
            record_cpu_loop(a.record, a.robots or 4, a.ticks or 600)
            sys.exit(0)
        r = cpu_loop(a.robots or 2, a.ticks or 600, a.force, a.grip_ticks)
        sys.exit(0 if r["bounded"] else 1)
    run(a.robots or 32, a.ticks or 600, a.trace_every, a.force, a.grip_ticks)
