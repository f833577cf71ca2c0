#!/usr/bin/env python3
"""A fleet that picks its part up, carries it and lets it go in its socket, on the GPU: B Dual-UR5 robots run a WP / GRIP list whose
waypoints aim at ACTION OBJECTS (BatchedOSC.set_objects / set_action_refs: csrc/osc_object.hpp in front of the action kernel of every
tick), the scene's joint rows drive the hand (set_joints), and episodes restart every robot on its next set of object poses
(set_episodes).  An object rides rigidly on the EE once the fingers have closed near it, stays where it is let go, and a plug that is
let go inside its socket's tolerances gives the episode the outcome bit INSERTED.

With --mass M the plug weighs M kg (BatchedOSC.set_object_loads: csrc/osc_object_load.hpp): the hand that holds it feels m g on its
EE body, on the plant and -- a tick later -- in the F/T feed.

What this is NOT: contact.  The weight is quasi-static (no inertial force), nothing collides, falls or slips, the fingers' forces are not
in the feed; a released object hangs where it was let go.

Two lists:
  the demo's (default)   the twelve actions of action_sequence_configs/insertion_task.yaml on the `nist` parts, each placed where the
                         arm can take it (demo_objects), GRIP durations cut to --grip-ticks;
  --carry                CARRY: WP hover -> GRIP close -> WP lift -> WP over the socket -> GRIP open, on poses a few centimetres from
                         the start -- about 1150 ticks an episode; the scenario of tests/test_objects.py.

    python examples/insertion_carry_resident_headless.py [--robots 32] [--episodes 2] [--variants 2] [--carry] [--ticks N] [--mass M]
    python examples/insertion_carry_resident_headless.py --cpu-loop [--robots 2] [--ticks 1300] [--mass M]      # no GPU: CARRY in NumPy

Prints the share of episodes with INSERTED."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from irl_control_amd import joints, object_loads as ol, objects as ob, synth      # noqa: E402
from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel   # noqa: E402
import gripper_fleet_resident_headless as grip                       # noqa: E402

WP, GRIP = 0, 1
ARM = "ur5right"
# CARRY, chosen on the CPU (cpu_loop below; what it printed is in its docstring)
FORCE_CLOSE, FORCE_OPEN = 0.08, -0.08       # N m on the driven knuckle: towards its upper stop / back to its lower one
CLOSE_TICKS, OPEN_TICKS = 330, 400
Q_CLOSE, Q_OPEN = 0.3, 0.15                 # rad of the driven knuckle: closed at and above, open at and below (hysteresis between)
RADIUS = 0.03                               # m around the grip point
A_XYZ = np.array([0.0, 0.0, 0.01])          # the plug in the hovering EE's frame (also the grip point) ...
A_QUAT = np.array([np.cos(0.15), 0.0, 0.0, np.sin(0.15)])
A_FAR = np.array([0.0, 0.0, 0.2])           # ... and where a robot's plug lies that is out of reach
C_XYZ = np.array([0.0, 0.01, 0.0])          # the socket in the EE's frame over it
C_QUAT = np.array([np.cos(0.1), np.sin(0.1), 0.0, 0.0])
TOL_XYZ, MIN_ABS_DOT = 0.06, 0.95
WP_MAX_ERROR = 0.02
OVER_MAX_ERROR = 0.04                       # of the WP over the socket: |xyz error, Euler error|_2, so at most that far off in xyz
KP = 20.0                                   # of the error-adaptive velocity limit: clip(KP err, 0.05, 1) m/s
DAMPING = 0.0                               # N m s / rad, the plant's joint damping
SPREAD = 0.03                               # rad per arm joint around the start configuration: see carry_states
MASS = 0.2                                  # kg of the plug (--mass): chosen on the CPU, see cpu_loop
OVER_ELBOW = 0.2                            # rad of the elbow between the start and the pose over the socket: 9 cm at the EE


def compose(T, A_xyz, A_quat):
    """T o A for poses T [B, 7] (x y z qw qx qy qz) and one transform A, in the object kernel's arithmetic"""
    T = np.asarray(T, dtype=np.float64)
    B = len(T)
    xyz = T[:, :3] + ob.mat_vec(ob.quat2mat(T[:, 3:]), np.broadcast_to(A_xyz, (B, 3)))
    return np.concatenate([xyz, ob.quat_mul(T[:, 3:], np.broadcast_to(A_quat, (B, 4)))], axis=1)


def conj(q):
    return np.asarray(q, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def carry_states(robots, seed=0, variants=1, spread=SPREAD):
    """-> q [V, B, 25] start configurations, near, over [V, B, 25]: the right arm moved by up to 0.005 rad per joint for the hover pose; for
    the pose over the socket its elbow turned by OVER_ELBOW and the other joints moved by up to 0.005 rad.
    The start configurations are the gripper fleet's (grip.Q_RIGHT, Q_LEFT), +- `spread` per arm joint and not that fleet's +- 0.15: how
    the hand hangs decides how its linkage answers the drive of 0.08 N m, and at +- 0.15 rad a robot in a hundred has a hand that swings
    by 0.3 rad about its way to the stop (cpu_loop on robot 0 of 130: a slow mode, 250 ticks a period, which joint damping does not
    remove), lets go on the way and takes the plug again after the opening.  CARRY's thresholds hold for the hands of this spread."""
    out = []
    for v in range(variants):
        rng = np.random.default_rng(1000 + seed + 17 * v)
        q = np.zeros((robots, 25))
        q[:, 1:7] = grip.Q_RIGHT + rng.uniform(-spread, spread, (robots, 6))
        q[:, 13:19] = grip.Q_LEFT + rng.uniform(-spread, spread, (robots, 6))
        near, over = q.copy(), q.copy()
        near[:, 1:7] += rng.uniform(-0.005, 0.005, (robots, 6))
        over[:, 1:7] += rng.uniform(-0.005, 0.005, (robots, 6))
        over[:, 3] += OVER_ELBOW
        out.append((q, near, over))
    return tuple(np.stack(x) for x in zip(*out))


def carry_scenario(lay, ee_near, ee_over, ee_start, far=None, radius=RADIUS, close_ticks=CLOSE_TICKS, open_ticks=OPEN_TICKS):
    """CARRY for B robots from the EE poses [B, ndev, 7] of their near, over and start configurations: the plug lies at T_near o A (A_FAR in
    place of A_XYZ for the robots of `far`: out of the hand's reach), the socket at T_over o C, so the WP that hovers aims at the plug's
    pose + an offset / (x) a grip rotation that lead back to T_near, and the released plug sits at inv(C) o A in the socket's frame for
    every robot -- the mate's seat.
    -> dict(desc: the list with its table of offsets / grip rotations (BatchedOSC.set_action_list), refs, objs: objects.ObjectSet,
            pose0 [B, 2, 7])"""
    names = list(lay.dev_names)
    ia, io = names.index(ARM), (names.index("ur5left") if "ur5left" in names else -1)
    B = len(ee_near)
    far = np.zeros(B, bool) if far is None else np.asarray(far, bool)
    near, over = np.asarray(ee_near, dtype=np.float64)[:, ia], np.asarray(ee_over, dtype=np.float64)[:, ia]
    plug = np.where(far[:, None], compose(near, A_FAR, A_QUAT), compose(near, A_XYZ, A_QUAT))
    sock = compose(over, C_XYZ, C_QUAT)
    A = 5
    table = np.zeros((B, A, 7))
    table[:, :, 3] = 1.0
    table[:, 0, :3], table[:, 0, 3:] = near[:, :3] - plug[:, :3], conj(A_QUAT)          # hover: plug + offset, q_plug (x) conj(q_a)
    table[:, 2] = np.asarray(ee_start, dtype=np.float64)[:, ia]                        # lift: back to the start (xyz_from_start)
    table[:, 3, :3], table[:, 3, 3:] = over[:, :3] - sock[:, :3], conj(C_QUAT)          # over the socket
    desc = dict(n_actions=A, active_dev=ia, passive_dev=io, passive_hold_orientation=1, passive_quat=np.array([1.0, 0.0, 0.0, 0.0]),
                kind=np.array([WP, GRIP, WP, WP, GRIP], np.int32), xyz_from_start=np.array([0, 0, 1, 0, 0], np.int32),
                grip_ticks=np.array([1, close_ticks, 1, 1, open_ticks], np.int32), kp=np.full(A, KP),
                max_error=np.array([WP_MAX_ERROR, 0.0, 0.05, OVER_MAX_ERROR, 0.0]), min_speed=np.full(A, 0.05), max_speed=np.full(A, 1.0),
                gripper_force=np.array([0.0, FORCE_CLOSE, 0.0, 0.0, FORCE_OPEN]), pose=table)
    refs = dict(xyz_obj=np.array([0, -1, -1, 1, -1], np.int32), quat_obj=np.array([0, -1, -1, 1, -1], np.int32))
    jn = RigidBodyModel.load("dual_ur5").joint_names
    seat = compose(np.concatenate([-ob.mat_t_vec(ob.quat2mat(C_QUAT), C_XYZ), conj(C_QUAT)])[None], A_XYZ, A_QUAT)[0]      # inv(C) o A
    objs = ob.ObjectSet(radius=[radius, radius],
                        grippers=[ob.Gripper(dev=ia, joint=jn.index(f"right_outer_knuckle_joint_{ARM}"), q_close=Q_CLOSE, q_open=Q_OPEN, sign=1,
                                             grip_xyz=tuple(A_XYZ))],
                        mates=[ob.Mate(plug=0, socket=1, tol_xyz=TOL_XYZ, min_abs_dot=MIN_ABS_DOT, seat_xyz=tuple(seat[:3]), seat_quat=tuple(seat[3:]))])
    return dict(desc=desc, refs=refs, objs=objs, pose0=np.stack([plug, sock], axis=1))


def live_table(desc, refs, obj_pose):
    """The list's table with every WP that has refs composed on the objects as they are now (objects.ref_target): what the action kernel
    would write if the WP were entered on this tick.  A host loop hands it to action_sequence.action_list_tick tick by tick."""
    table = np.array(desc["pose"], dtype=np.float64)
    for a in range(desc["n_actions"]):
        if desc["kind"][a] == WP and (refs["xyz_obj"][a] >= 0 or refs["quat_obj"][a] >= 0):
            table[:, a] = ob.ref_target(obj_pose, table[:, a], int(refs["xyz_obj"][a]), int(refs["quat_obj"][a]))
    return table


def carry_loads(mass=MASS):
    """CARRY's loads: the plug weighs `mass` kg at its frame origin, the socket nothing (nobody takes it)"""
    return ol.ObjectLoads(mass=[float(mass), 0.0])


def cpu_loop(robots=2, ticks=1300, dt=1e-3, damping=DAMPING, seed=0, verbose=True, far=(), mass=0.0, **kw):
    """CARRY in NumPy, no GPU -- the loop its thresholds, gears and GRIP lengths were chosen with: gripper_fleet_resident_headless.cpu_loop's
    tick (the rigid-body oracle's records, the list's host restatement, the OSC oracle's u, joints.joint_torque, semi-implicit Euler) with
    objects.object_step in front of the list and the list's table composed on the live objects.
    With `mass` > 0 the plug weighs that much (object_loads.load_wrench behind object_step; J^T W of the holder's EE body goes to the
    plant with the joint rows' torques, as csrc/osc_object_load.hpp takes it off the bias).  MASS = 0.2 kg was chosen with this loop
    (2 robots, 1300 ticks): grasp on tick 141 / 144 as without a mass, the arm 0.40 mm lower mid-carry (tick 600), release and mate on tick
    1022 / 1031 (without: 1019 / 1028), the list through on 1131 / 1138 -- CARRY still grasps, carries and mates, inside the band of
    profiles/object_rates.md (grasped by tick 155, let go from tick 994 on).  0.5 kg does too: 1.0 mm, release on 1028 / 1037.
    -> dict(knuckle [T, B], action [T, B], state: the objects' state at the end, obj_log [T, B, 2, 7], ee_log [T, B, 3]: the active
            arm's EE xyz, holder_log [T, B], load_log [T, B, 6])
    Run with the constants above (2 robots, 1300 ticks) it printed: the driven knuckle crosses Q_CLOSE = 0.3 rad 140 ticks into the GRIP
    of 330 ticks and is at its upper stop (0.83 rad) when the arm sets off -- with a GRIP of 170 ticks the hand was still closing then,
    and on the GPU the arm's start pulled the knuckle of 2 robots in 130 back under Q_OPEN: a premature release -- and crosses Q_OPEN =
    0.15 rad 288 / 297 ticks into the opening GRIP of 400; grasp on tick 141, the plug carried 0.092 / 0.089 m, release on tick 1033 /
    1042 and mated on that very tick, the list through on tick 1145."""
    from irl_control_amd import action_sequence as aseq
    from irl_control_amd.layout import pack_gains
    from oracle import osc_oracle
    from oracle import rigid_body as rb
    om = rb.Model()
    lay = synth.make_layout("k13")
    ld = lay.as_oracle_dict()
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    names = RigidBodyModel.load("dual_ur5").joint_names
    ee_of = lambda qq: np.array([rb.records(om, ld, DUAL_UR5_EE, x, np.zeros(25))["ee_pose"] for x in qq])      # noqa: E731
    q0, near, over = (x[0] for x in carry_states(robots, seed))
    start = ee_of(q0)
    isfar = np.zeros(robots, bool)
    isfar[list(far)] = True
    sc = carry_scenario(lay, ee_of(near), ee_of(over), start, far=isfar, **kw)
    desc, refs, objs = sc["desc"], sc["refs"], sc["objs"]
    ia = desc["active_dev"]
    jd, table = joints.normalise(grip.scene_rows(), names, lay.dev_names, robots)
    kn = objs.grippers[0].joint
    q, qd = q0.copy(), np.zeros_like(q0)
    tgt = start.copy()
    grec = pack_gains(lay, gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], np.broadcast_to(gains["max_vel"], (robots, lay.ndev, 2)))[0]
    state, ost = aseq.action_list_state(robots), ob.object_state(sc["pose0"])
    ctrl = np.zeros((robots, table.shape[1]))
    knuckle, act, olog = np.zeros((ticks, robots)), np.zeros((ticks, robots), np.int32), np.zeros((ticks, robots, 2, 7))
    eelog, hlog, wlog = np.zeros((ticks, robots, 3)), np.zeros((ticks, robots), np.int32), np.zeros((ticks, robots, 6))
    loads = carry_loads(mass) if mass else None
    ee_body = om.body_id(DUAL_UR5_EE[ARM])
    keys = ("M", "J", "dq", "bias", "ee_pose")
    for t in range(ticks):
        recs = [rb.records(om, ld, DUAL_UR5_EE, q[b], qd[b]) for b in range(robots)]
        r = {k: np.array([x[k] for x in recs]) for k in keys}
        ob.object_step(ost, objs, r["ee_pose"], q, t)
        aseq.action_list_tick(state, r["ee_pose"], tgt, grec, dict(desc, pose=live_table(desc, refs, ost["pose"])), t)
        u = osc_oracle.generate_batch(ld, dict(gains, max_vel=grec[:, :, 9:11].copy()), r["M"], r["J"], r["dq"], r["bias"], r["ee_pose"], tgt)
        tau, ctrl, _ = joints.joint_torque(q, qd, jd, table, ctrl, state["gripper_force"], ia)
        knuckle[t], act[t], olog[t] = q[:, kn], state["action"], ost["pose"]
        eelog[t], hlog[t] = r["ee_pose"][:, ia, :3], ost["holder"][:, 0]
        if loads is not None:                             # the weight of what the hand holds after this tick's object step, on the plant
            W = ol.load_wrench(loads, objs, r["ee_pose"], ost["pose"], ost["holder"])[:, 0]
            wlog[t] = W
            tau = tau + np.array([np.vstack(rb.body_jacobian(om, recs[b]["kin"], ee_body)).T @ W[b] for b in range(robots)])
        qacc = np.linalg.solve(r["M"], (u - r["bias"] - damping * qd + tau)[:, :, None])[:, :, 0]
        qd = qd + dt * qacc
        q = q + dt * qd
    if verbose:
        for b in range(robots):
            ent = [int(np.argmax(act[:, b] == a)) if (act[:, b] == a).any() else -1 for a in range(desc["n_actions"])]
            cross = lambda thr, t0, up: next((t - t0 for t in range(max(t0, 0), ticks) if (knuckle[t, b] >= thr) == up), -1)      # noqa: E731
            print(f"robot {b}: actions entered on ticks {ent}, through on {int(state['finished_tick'][b])}; knuckle crosses q_close {cross(Q_CLOSE, ent[1], True)} "
                  f"ticks into the closing GRIP, q_open {cross(Q_OPEN, ent[4], False)} into the opening one (max {knuckle[:, b].max():.3f} rad); grasp "
                  f"{ost['grasp_tick'][b, 0]}, release {ost['release_tick'][b, 0]}, mated {ost['mated_tick'][b, 0]}")
    return dict(knuckle=knuckle, action=act, state=ost, obj_log=olog, finished=state["finished_tick"].copy(), ee_log=eelog, holder_log=hlog, load_log=wlog)


def make_ctx(robots, dtype=np.float64, n_slots=1, dt=1e-3, damping=DAMPING):
    from irl_control_amd import BatchedOSC
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    osc = BatchedOSC(lay, robots, dtype=dtype, n_slots=n_slots)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(dt, damping)
    return osc


def fk(osc, q, slot=0):
    """EE poses [B, ndev, 7] of configurations q [B, 25] by the GPU front end"""
    osc.upload_q(q, np.zeros_like(q), slot=slot)
    osc.frontend(slot=slot)
    return osc.download_records(slot=slot, keys=("ee_pose",))["ee_pose"].astype(np.float64)


def summary(st, verbose=True):
    from irl_control_amd import _lib
    rec = st["records"].reshape(-1, 4)
    rec = rec[rec[:, 1] > 0]
    ins = int(((rec[:, 2] & _lib.EPISODE_INSERTED) != 0).sum())
    fin = int(((rec[:, 2] & _lib.EPISODE_FINISHED) != 0).sum())
    share = ins / max(1, len(rec))
    if verbose:
        print(f"{len(rec)} episodes on record: {fin} FINISHED, {len(rec) - fin} TIMEOUT; INSERTED {ins} = {100.0 * share:.1f} %")
        if len(rec):
            print(f"episode lengths {rec[:, 1].min()} .. {rec[:, 1].max()} ticks")
    return dict(episodes=len(rec), inserted=ins, finished=fin, share=share)


def run_carry(robots=32, ticks=3200, episodes=2, variants=2, limit=1500, seed=0, verbose=True, mass=0.0):
    """CARRY with episodes: every robot's episode e starts from start state e mod V on its objects' start poses e mod V (the list's
    table of offsets and grip rotations likewise).  mass > 0: the plug weighs that much (set_object_loads, behind set_objects)."""
    osc = make_ctx(robots)
    lay = osc.layout
    q, near, over = carry_states(robots, seed, variants)
    scs = []
    for v in range(variants):
        start = fk(osc, q[v])
        scs.append(carry_scenario(lay, fk(osc, near[v]), fk(osc, over[v]), start))
    osc.upload_q(q[0], np.zeros_like(q[0]))
    osc.frontend()
    osc.set_targets(fk(osc, q[0]))
    osc.set_action_list(scs[0]["desc"])
    osc.set_joints(grip.scene_rows())
    osc.set_objects(scs[0]["objs"], np.stack([s["pose0"] for s in scs]))
    if mass:
        osc.set_object_loads(carry_loads(mass))
    osc.set_action_refs(scs[0]["refs"]["xyz_obj"], scs[0]["refs"]["quat_obj"])
    osc.set_episodes(np.swapaxes(q, 0, 1), None, max_ticks=limit, max_episodes=episodes, poses=np.stack([s["desc"]["pose"] for s in scs]),
                     records=16, poll_every=64 if episodes else 0)
    out = osc.rollout(ticks)
    st = osc.episode_state()
    osc.close()
    if verbose:
        print(f"CARRY: {robots} robots, {out['ticks_run']} ticks in one call, {int(st['count'].sum())} episodes ended" + (f", the plug weighing {mass} kg" if mass else ""))
    return dict(summary(st, verbose), ticks_run=out["ticks_run"], count=st["count"], records=st["records"])


def demo_objects(rng, osc, q, cfg_objects, spread=0.35):
    """Per robot the two parts of the YAML, placed where the arm can take them, like insertion_fleet_headless.random_objects: a part's
    pose is chosen such that its grip waypoint (the male part: grip_offset; the female part: insert_offset) is the EE pose of a randomly
    perturbed configuration.  Unlike there the offset is taken ALONG THE PART'S OWN AXES (the YAML's parts stand upright, where that is
    the YAML's own world offset): then the hand meets the part at the same point of the EE frame on every robot, which is what one
    grip_xyz and one seat per slot can describe.  -> (objects: per robot {name: {..., "pos", "quat"}}, R [B, 2, 3, 3] the parts' frames)"""
    from irl_control_amd import action_sequence as aseq
    from irl_control_amd.transforms import euler2quat, mat2euler, quat2mat
    ia = list(osc.layout.dev_names).index(ARM)
    B = len(q)
    out, Rs = [dict() for _ in range(B)], np.zeros((B, 2, 3, 3))
    for k, (name, key) in enumerate((("male_object", "grip_offset"), ("female_object", "insert_offset"))):
        qg = q.copy()
        qg[:, 1:7] += rng.uniform(-spread, spread, (B, 6))
        pose = fk(osc, qg)[:, ia]
        E = quat2mat(aseq.grip_quat(cfg_objects[name]))
        for b in range(B):
            o = dict(cfg_objects[name])
            R_obj = quat2mat(pose[b, 3:]) @ E.T                              # R_obj E = R_ee(q_g)
            o["quat"] = euler2quat(*mat2euler(R_obj))
            Rs[b, k] = quat2mat(o["quat"])
            o["pos"] = pose[b, :3] - Rs[b, k] @ np.asarray(o[key], dtype=np.float64)
            out[b][name] = o
    return out, Rs


def run(robots=32, ticks=70000, episodes=2, variants=2, limit=30000, grip_ticks=150, seed=0, verbose=True):
    """The demo's twelve actions on the `nist` parts with refs: the male part is gripped (action 3), carried to the female part and let go
    at its insert offset (action 9), where the mate's seat is: insert_offset - grip_offset in the female part's frame."""
    from irl_control_amd import action_sequence as aseq
    rng = np.random.default_rng(seed)
    osc = make_ctx(robots)
    lay, model = osc.layout, RigidBodyModel.load("dual_ur5")
    names = list(lay.dev_names)
    cfg = aseq.load_action_config("insertion_task.yaml")
    seq = [dict(e, max_error=max(e.get("max_error", 0.0018), 0.012)) if e["action"] == "WP" else dict(e, gripper_duration=grip_ticks * 1e-3)
           for e in cfg["insertion_action_sequence"]]
    q = np.zeros((robots, 25))
    q[:, 1:7] = grip.Q_RIGHT + rng.uniform(-0.15, 0.15, (robots, 6))
    q[:, 13:19] = grip.Q_LEFT + rng.uniform(-0.15, 0.15, (robots, 6))
    compiled = []
    for _ in range(variants):
        objects, Rs = demo_objects(rng, osc, q, cfg["nist_action_objects"])
        d, refs, pose0 = aseq.compile_action_list_refs(seq, objects, names.index(ARM), names.index("ur5left"), 1e-3, True)
        for a in np.nonzero(refs["xyz_obj"] >= 0)[0]:                         # the YAML's offsets along the part's own axes
            d["pose"][:, a, :3] = np.einsum("bij,bj->bi", Rs[:, refs["xyz_obj"][a]], d["pose"][:, a, :3])
        compiled.append((d, refs, pose0))
    d, refs, _ = compiled[0]
    o = cfg["nist_action_objects"]
    g_off = np.asarray(o["male_object"]["grip_offset"], dtype=np.float64)
    seat = np.asarray(o["female_object"]["insert_offset"], dtype=np.float64) - g_off
    grip_xyz = ob.mat_t_vec(ob.quat2mat(aseq.grip_quat(o["male_object"])), -g_off)      # the male part's origin as the gripping EE sees it
    jn = model.joint_names
    objs = ob.ObjectSet(radius=[0.03, 0.03],
                        grippers=[ob.Gripper(dev=names.index(ARM), joint=jn.index(f"right_outer_knuckle_joint_{ARM}"), q_close=Q_CLOSE, q_open=Q_OPEN,
                                             grip_xyz=tuple(grip_xyz))],
                        mates=[ob.Mate(plug=0, socket=1, tol_xyz=0.03, min_abs_dot=0.99, seat_xyz=tuple(seat))])
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    osc.set_targets(osc.download_records(keys=("ee_pose",))["ee_pose"])
    osc.set_action_list(d)
    osc.set_joints(grip.scene_rows())
    osc.set_objects(objs, np.stack([c[2] for c in compiled]))
    osc.set_action_refs(refs["xyz_obj"], refs["quat_obj"])
    osc.set_episodes(q[:, None], None, max_ticks=limit, max_episodes=episodes, poses=np.stack([c[0]["pose"] for c in compiled]), records=16,
                     poll_every=64 if episodes else 0)
    out = osc.rollout(ticks)
    st, os_, act = osc.episode_state(), osc.object_state(), osc.action_state()
    osc.close()
    if verbose:
        print(f"insertion list with refs: {robots} robots, {out['ticks_run']} ticks in one call, {int(st['count'].sum())} episodes ended")
        print(f"robots' last episode: grasped {int((os_['grasp_tick'][:, 0] >= 0).sum())}, released {int((os_['release_tick'][:, 0] >= 0).sum())}, "
              f"mated {int((os_['mated_tick'][:, 0] >= 0).sum())}; action index now {np.bincount(act['action'], minlength=13).tolist()}")
    return dict(summary(st, verbose), ticks_run=out["ticks_run"], count=st["count"], records=st["records"], objects=os_)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=None)
    ap.add_argument("--ticks", type=int, default=None)
    ap.add_argument("--episodes", type=int, default=2, help="episodes per robot (0: no limit, the call runs all its ticks)")
    ap.add_argument("--variants", type=int, default=2, help="sets of object poses per robot, taken in turn")
    ap.add_argument("--limit", type=int, default=None, help="time limit of an episode in ticks")
    ap.add_argument("--grip-ticks", type=int, default=150)
    ap.add_argument("--carry", action="store_true")
    ap.add_argument("--cpu-loop", action="store_true")
    ap.add_argument("--mass", type=float, default=0.0, help=f"kg of the plug (CARRY and --cpu-loop; 0: no loads; chosen on the CPU: {MASS})")
    a = ap.parse_args()
    if a.cpu_loop:
        cpu_loop(a.robots or 2, a.ticks or 1300, mass=a.mass)
        sys.exit(0)
    if a.carry:
        r = run_carry(a.robots or 32, a.ticks or 3200, a.episodes, a.variants, a.limit or 1500, mass=a.mass)
    else:
        r = run(a.robots or 32, a.ticks or 70000, a.episodes, a.variants, a.limit or 30000, a.grip_ticks)
    sys.exit(0 if r["inserted"] > 0 else 1)
