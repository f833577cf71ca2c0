"""Action objects on the host (no GPU): the NumPy mirror irl_control_amd/objects.py on hand-made ticks, the YAML compile helper
action_sequence.compile_action_list_refs, the log mirror's tenth channel and the new ctypes structs against include/irlosc.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from irl_control_amd import _lib, objects as ob, rollout_log
from irl_control_amd import action_sequence as aseq
from irl_control_amd.transforms import euler2quat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KN = 7                        # the hinge the hand-made ticks use as the knuckle
Q_CLOSE, Q_OPEN, RADIUS = 0.3, 0.1, 0.05


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def objset(n_objects=1, mates=(), grip_xyz=(0.0, 0.0, 0.0), sign=1):
    qc, qo = (Q_CLOSE, Q_OPEN) if sign > 0 else (-Q_CLOSE, -Q_OPEN)
    return ob.ObjectSet(radius=[RADIUS] * n_objects, grippers=[ob.Gripper(dev=0, joint=KN, q_close=qc, q_open=qo, sign=sign, grip_xyz=grip_xyz)],
                        mates=list(mates))


def tick(st, objs, ee_pose, knuckle, t):
    """One robot, one device: EE pose [7] and the knuckle angle"""
    q = np.zeros((1, 25))
    q[0, KN] = knuckle
    return ob.object_step(st, objs, np.asarray(ee_pose, dtype=np.float64).reshape(1, 1, 7), q, t)


EE0 = np.concatenate([[0.4, 0.1, 0.3], unit([0.9, 0.1, -0.3, 0.2])])


def test_grasp_only_on_the_rising_edge_and_only_inside_the_radius():
    objs = objset()
    at = np.concatenate([EE0[:3] + [0.0, 0.03, 0.0], [1.0, 0, 0, 0]])[None, None]
    # a hand that is closed from the first tick on (was_closed starts at 0): that IS a rising edge
    st = tick(ob.object_state(at), objs, EE0, 0.5, 0)
    assert st["holder"][0, 0] == 0 and st["grasp_tick"][0, 0] == 0
    # a hand that travels closed and arrives near the object picks nothing up
    st = ob.object_state(at)
    far = EE0.copy()
    far[0] += 1.0
    tick(st, objs, far, 0.5, 0)
    assert st["holder"][0, 0] == -1 and st["was_closed"][0, 0] == 1
    tick(st, objs, EE0, 0.5, 1)
    assert st["holder"][0, 0] == -1
    # open, then closed near it: the edge
    tick(st, objs, EE0, 0.0, 2)
    tick(st, objs, EE0, 0.2, 3)                      # between the thresholds: neither closed nor open
    assert st["holder"][0, 0] == -1 and st["was_closed"][0, 0] == 0
    tick(st, objs, EE0, 0.3, 4)                      # closed is >=
    assert st["holder"][0, 0] == 0 and st["grasp_tick"][0, 0] == 4
    # the radius: squared distances compared, the rim included; a hair outside is outside
    for d, held in ((RADIUS, True), (np.nextafter(RADIUS, 1.0) + 1e-12, False)):
        at = np.array([d, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])[None, None]
        rim = EE0.copy()
        rim[:3] = 0.0                                # the EE at the origin: the distance is d itself
        st = tick(ob.object_state(at), objs, rim, 0.5, 0)
        assert (st["holder"][0, 0] == 0) == held, d
    # the grip point is a point of the EE frame
    g = (0.0, 0.0, 0.2)
    R = ob.quat2mat(EE0[3:])
    at = np.concatenate([EE0[:3] + R @ np.array(g), [1.0, 0, 0, 0]])[None, None]
    assert tick(ob.object_state(at), objset(grip_xyz=g), EE0, 0.5, 0)["holder"][0, 0] == 0
    assert tick(ob.object_state(at), objset(), EE0, 0.5, 0)["holder"][0, 0] == -1
    # sign -1: closed towards negative angles
    at = np.concatenate([EE0[:3], [1.0, 0, 0, 0]])[None, None]
    assert tick(ob.object_state(at), objset(sign=-1), EE0, -0.5, 0)["holder"][0, 0] == 0
    assert tick(ob.object_state(at), objset(sign=-1), EE0, 0.5, 0)["holder"][0, 0] == -1


def test_a_full_hand_takes_no_second_object():
    objs = objset(2)
    at = np.stack([np.concatenate([EE0[:3] + [0.0, 0.01, 0.0], [1.0, 0, 0, 0]]), np.concatenate([EE0[:3] - [0.0, 0.01, 0.0], [1.0, 0, 0, 0]])])[None]
    st = tick(ob.object_state(at), objs, EE0, 0.5, 0)
    assert st["holder"][0].tolist() == [0, -1]       # ascending o: the first one in reach
    tick(st, objs, EE0, 0.0, 1)                      # open: released; not taken again on the tick of its release
    tick(st, objs, EE0, 0.5, 2)
    assert st["holder"][0].tolist() == [0, -1] and st["grasp_tick"][0].tolist() == [2, -1] and st["release_tick"][0].tolist() == [1, -1]


def test_release_at_q_open_with_hysteresis_and_carry():
    """A held object follows T_ee o inv(T_ee0) o T_obj0 (to 1e-15 against float64 matrices), keeps following between the thresholds, and
    stays where it is from the tick the knuckle is at q_open or below."""
    objs = objset()
    qo = unit([0.7, -0.2, 0.1, 0.4])
    at = np.concatenate([EE0[:3] + [0.0, 0.02, -0.01], qo])[None, None]
    st = tick(ob.object_state(at), objs, EE0, 0.5, 0)
    assert st["holder"][0, 0] == 0 and np.array_equal(st["pose"], at)       # the tick of the grasp leaves the pose
    rng = np.random.default_rng(5)
    R0, last = ob.quat2mat(EE0[3:]), None
    for t, kn in enumerate([0.5, 0.31, 0.2, 0.11, np.nextafter(Q_OPEN, 1.0)], start=1):      # never at or below q_open: held throughout
        ee = np.concatenate([rng.uniform(-0.5, 0.5, 3), unit(rng.normal(size=4))])
        tick(st, objs, ee, kn, t)
        assert st["holder"][0, 0] == 0
        R1 = ob.quat2mat(ee[3:])
        want_xyz = ee[:3] + R1 @ R0.T @ (at[0, 0, :3] - EE0[:3])
        want_R = R1 @ R0.T @ ob.quat2mat(qo)
        assert np.abs(st["pose"][0, 0, :3] - want_xyz).max() <= 1e-15
        assert np.abs(ob.quat2mat(st["pose"][0, 0, 3:]) - want_R).max() <= 1e-15
        last = st["pose"].copy()
    tick(st, objs, np.concatenate([[9.0, 9.0, 9.0], unit([1, 2, 3, 4])]), Q_OPEN, 6)      # open is <=
    assert st["holder"][0, 0] == -1 and st["release_tick"][0, 0] == 6 and np.array_equal(st["pose"], last)
    tick(st, objs, EE0, 0.0, 7)
    assert np.array_equal(st["pose"], last) and st["grasp_tick"][0, 0] == 0


def test_a_mate_fires_only_for_a_free_plug_inside_both_tolerances():
    seat_xyz, seat_q = (0.0, 0.0, 0.1), unit([0.9, 0.0, 0.0, 0.4])
    m = ob.Mate(plug=0, socket=1, tol_xyz=0.01, min_abs_dot=0.99, seat_xyz=seat_xyz, seat_quat=tuple(seat_q))
    objs = objset(2, mates=[m])
    sock = np.concatenate([[0.2, -0.1, 0.0], unit([0.8, 0.1, 0.1, -0.5])])
    tgt_xyz = sock[:3] + ob.quat2mat(sock[3:]) @ np.array(seat_xyz)
    tgt_q = ob.quat_mul(sock[3:], seat_q)
    away = EE0.copy()
    away[:3] += 5.0

    def state(plug_xyz, plug_q):
        return ob.object_state(np.stack([np.concatenate([plug_xyz, plug_q]), sock])[None])

    st = tick(state(tgt_xyz + [0.0, 0.009, 0.0], -tgt_q), objs, away, 0.0, 3)              # inside both (the quaternion's sign does not count)
    assert st["mated_tick"][0, 0] == 3
    tick(st, objs, away, 0.0, 4)
    assert st["mated_tick"][0, 0] == 3                                                      # recorded once
    assert tick(state(tgt_xyz + [0.0, 0.011, 0.0], tgt_q), objs, away, 0.0, 0)["mated_tick"][0, 0] == -1      # too far
    turned = ob.quat_mul(tgt_q, np.array([np.cos(0.2), np.sin(0.2), 0.0, 0.0]))            # |dot| = cos 0.2 = 0.980 < 0.99
    assert tick(state(tgt_xyz, turned), objs, away, 0.0, 0)["mated_tick"][0, 0] == -1
    # a held plug does not mate, however well it sits; it does on the tick it is let go
    ee = np.concatenate([tgt_xyz, [1.0, 0, 0, 0]])
    st = tick(state(tgt_xyz, tgt_q), objs, ee, 0.5, 0)
    assert st["holder"][0, 0] == 0 and st["mated_tick"][0, 0] == -1
    tick(st, objs, ee, 0.5, 1)
    assert st["mated_tick"][0, 0] == -1
    tick(st, objs, ee, 0.0, 2)
    assert st["holder"][0, 0] == -1 and st["mated_tick"][0, 0] == 2


def test_nan_is_neither_edge_and_a_nan_pose_keeps_everything():
    objs = objset()
    at = np.concatenate([EE0[:3], [1.0, 0, 0, 0]])[None, None]
    st = tick(ob.object_state(at), objs, EE0, np.nan, 0)
    assert st["holder"][0, 0] == -1 and st["was_closed"][0, 0] == 0                         # not closed
    tick(st, objs, EE0, 0.5, 1)
    moved = EE0.copy()
    moved[0] += 0.3
    tick(st, objs, moved, np.nan, 2)                                                        # not open: still held, and carried
    assert st["holder"][0, 0] == 0 and st["was_closed"][0, 0] == 0 and abs(st["pose"][0, 0, 0] - moved[0]) < 1e-12
    before = {k: v.copy() for k, v in st.items()}
    bad = EE0.copy()
    bad[5] = np.nan
    tick(st, objs, bad, 0.0, 3)                                                             # an EE pose word is NaN: nothing of the robot changes
    assert all(np.array_equal(before[k], st[k]) for k in st)


# ---- the YAML compile helper ------------------------------------------------------------------------------------------------------------
def yaml_objects(rng, cfg_objects, B):
    out = []
    for _ in range(B):
        objs = {}
        for name in ("male_object", "female_object"):
            o = dict(cfg_objects[name])
            o["pos"] = rng.uniform(-0.5, 0.5, 3)
            o["quat"] = euler2quat(0.0, 0.0, rng.uniform(-np.pi, np.pi))
            objs[name] = o
        out.append(objs)
    return out


@pytest.mark.parametrize("which", ["nist_action_objects", "grommet_action_objects"])
def test_the_yaml_list_compiles_into_offsets_grip_rotations_and_refs(which):
    """The table holds the YAML's offsets and the objects' grip rotations, the refs of all twelve actions are right, and composed on the
    objects at rest (objects.ref_target: the kernel's add and product) the table is FleetActionSequenceRunner's static one
    (compile_action_list -> waypoint_target): xyz words bit for bit, quaternions to <= 1e-12 up to sign.
    Measured maximum over 64 robots and both object sets: 2.22e-16 -- an ulp of one Hamilton product of unit quaternions against
    euler2quat(mat2euler(R_obj R_grip)), as the bound's reasoning says."""
    cfg = aseq.load_action_config("insertion_task.yaml")
    seq = cfg["insertion_action_sequence"]
    B = 64
    objects = yaml_objects(np.random.default_rng(11), cfg[which], B)
    static = aseq.compile_action_list(seq, objects, 0, 1)
    d, refs, pose0 = aseq.compile_action_list_refs(seq, objects, 0, 1)
    M, F = 0, 1
    assert refs["xyz_obj"].tolist() == [M, -1, M, -1, M, F, F, -1, F, -1, F, -1]
    assert refs["quat_obj"].tolist() == [M, -1, M, -1, M, M, F, -1, F, -1, F, F]
    offs = {0: ("male_object", "hover_offset"), 2: ("male_object", "grip_offset"), 4: ("male_object", "hover_offset"),
            5: ("female_object", "hover_offset"), 6: ("female_object", "hover_offset"), 8: ("female_object", "insert_offset"),
            10: ("female_object", "hover_offset_lift")}
    for a, (name, key) in offs.items():
        assert np.array_equal(d["pose"][:, a, :3], np.tile(np.asarray(cfg[which][name][key], dtype=np.float64), (B, 1))), a
    for k in ("kind", "xyz_from_start", "grip_ticks", "kp", "max_error", "min_speed", "max_speed", "gripper_force"):
        assert np.array_equal(d[k], static[k]), k
    assert d["xyz_from_start"][11] == 1 and refs["xyz_obj"][11] == -1
    assert pose0.shape == (B, 2, 7)
    for b in range(B):
        assert np.array_equal(pose0[b, M], np.concatenate([objects[b]["male_object"]["pos"], objects[b]["male_object"]["quat"]]))
        assert np.array_equal(pose0[b, F, :3], objects[b]["female_object"]["pos"])
    worst = 0.0
    for a in np.nonzero(d["kind"] == aseq.Action.WP.value)[0]:
        got = ob.ref_target(pose0, d["pose"][:, a], int(refs["xyz_obj"][a]), int(refs["quat_obj"][a]))
        if not d["xyz_from_start"][a]:
            assert np.array_equal(got[:, :3], static["pose"][:, a, :3]), a
        sign = np.sign((got[:, 3:] * static["pose"][:, a, 3:]).sum(axis=1))[:, None]
        worst = max(worst, np.abs(got[:, 3:] * sign - static["pose"][:, a, 3:]).max())
    print(f"\n[{which}] max |q_obj (x) q_grip -+ static quaternion| = {worst:.3g}")
    assert worst <= 1e-12


# ---- the log mirror's tenth channel, the structs ---------------------------------------------------------------------------------------
def test_the_object_pose_channel_in_the_layout_and_its_mirror():
    lib = _lib.load()
    n, ndev, R = 25, 3, 65
    for nobj in (1, 2, 4):
        for channels in (512, 1 | 512, 1023):
            off = np.full(10, -7, dtype=np.int64)
            words = C.c_int64(-7)
            assert lib.irlosc_log_layout_objects(n, ndev, nobj, channels, R, _lib.ptr(off), C.addressof(words)) == 0
            moff, mwords = rollout_log.layout(n, ndev, channels, R, nobj)
            assert np.array_equal(off, moff) and words.value == mwords
            assert off[9] == mwords - R * nobj * 8                                          # the last plane of the sample
    off9, w9 = rollout_log.layout(n, ndev, 511, R)
    off10, w10 = rollout_log.layout(n, ndev, 511, R, nobj=2)
    assert np.array_equal(off9, off10[:9]) and off10[9] == -1 and w9 == w10
    # without objects the bit is unknown, to both; nobj out of range
    off = np.zeros(10, dtype=np.int64)
    words = C.c_int64(0)
    assert lib.irlosc_log_layout_objects(n, ndev, 0, 512, R, _lib.ptr(off), C.addressof(words)) == -1
    assert lib.irlosc_log_layout_objects(n, ndev, 5, 1, R, _lib.ptr(off), C.addressof(words)) == -1
    assert lib.irlosc_log_layout_objects(n, ndev, 0, 511, R, _lib.ptr(off), C.addressof(words)) == 0 and off[9] == -1
    with pytest.raises(ValueError):
        rollout_log.layout(n, ndev, 512, R)
    assert rollout_log.mask(["qpos", "object_pose"]) == 513 and rollout_log.names(513) == ("qpos", "object_pose")
    # split: [S, R, nobj, 8] float64 behind the other planes
    S, nobj = 3, 2
    o, w = rollout_log.layout(n, ndev, 513, R, nobj)
    buf = np.random.default_rng(0).normal(size=(S, w))
    got = rollout_log.split(buf, n, ndev, 513, R, nobj=nobj)
    assert got["object_pose"].shape == (S, R, nobj, 8) and np.array_equal(got["object_pose"].reshape(S, -1), buf[:, o[9]:])


def test_struct_sizes_against_the_header():
    hdr = open(os.path.join(ROOT, "include", "irlosc.h")).read()
    for name, val in (("IRLOSC_MAX_OBJECTS", _lib.MAX_OBJECTS), ("IRLOSC_MAX_GRIPPERS", _lib.MAX_GRIPPERS), ("IRLOSC_MAX_MATES", _lib.MAX_MATES),
                      ("IRLOSC_EPISODE_INSERTED", _lib.EPISODE_INSERTED), ("IRLOSC_MAX_ACTIONS", _lib.MAX_ACTIONS)):
        assert re.search(rf"#define {name}\s+{val}\b", hdr), name
    assert re.search(r"#define IRLOSC_LOG_OBJECT_POSE\s+512u", hdr) and _lib.LOG_OBJECT_POSE == 512
    NO, NG, NM = _lib.MAX_OBJECTS, _lib.MAX_GRIPPERS, _lib.MAX_MATES
    # struct irlosc_objects: 4 + 3 NG + 2 NM int32 (14 words: a multiple of 8 bytes), then doubles
    ints = 4 + 3 * NG + 2 * NM
    assert ints % 2 == 0
    assert C.sizeof(_lib.Objects) == 4 * ints + 8 * (2 * NG + 3 * NG + NO + 3 * NM + 4 * NM + 2 * NM)
    assert C.sizeof(_lib.ActionRefs) == 4 * 2 * _lib.MAX_ACTIONS
    body = hdr[hdr.index("typedef struct irlosc_objects {"):hdr.index("} irlosc_objects;")]
    fields = re.findall(r"^\s*(?:int32_t|double)\s+(\w+)", body, flags=re.M)
    assert fields == [f[0] for f in _lib.Objects._fields_]
    assert ob.ObjectSet(radius=[0.1], grippers=[ob.Gripper(0, 7, 0.3, 0.1)]).to_struct(3).n_variants == 3
    assert (ob.MAX_OBJECTS, ob.MAX_GRIPPERS, ob.MAX_MATES) == (NO, NG, NM)
