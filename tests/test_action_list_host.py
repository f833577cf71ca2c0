"""The WP / GRIP action list on the GPU, the part that needs no GPU: the two exports are declared in include/irlosc.h with
IRLOSC_MAX_ACTIONS and struct irlosc_action_list, fall under the version script's pattern, are bound by _lib.py with a struct of the
header's layout, the ABI version stays 3 (tests/test_abi.py then holds `nm -D` against the header) -- and the NumPy restatement of the
kernel (action_sequence.action_list_tick) is FleetActionSequenceRunner tick for tick, with after_step moved to the next tick's start."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np

from conftest import ROOT
from irl_control_amd import _lib, synth
from irl_control_amd import action_sequence as aseq
from irl_control_amd.layout import pack_gains

NEW = ("irlosc_set_action_list", "irlosc_download_action_state")
CTYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "uint8_t": C.c_uint8}
DIMS = {"IRLOSC_MAX_ACTIONS": _lib.MAX_ACTIONS, "4": 4}


def _header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def test_header_declares_the_action_list_exports():
    h = _header()
    for name in NEW:
        assert re.search(r"IRLOSC_API\s+int\s+" + name + r"\s*\(", h), name
    assert re.search(r"#define\s+IRLOSC_MAX_ACTIONS\s+32\b", h)
    assert _lib.MAX_ACTIONS == 32
    assert re.search(r"#define\s+IRLOSC_ACTION_WP\s+0\b", h) and re.search(r"#define\s+IRLOSC_ACTION_GRIP\s+1\b", h)
    assert (_lib.ACTION_WP, _lib.ACTION_GRIP) == (aseq.Action.WP.value, aseq.Action.GRIP.value) == (0, 1)
    assert re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", h) and _lib.ABI_VERSION == 3      # additive exports: the version stays


def test_version_script_and_binding_list_them():
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), (name, pats)
        assert name in _lib.EXPORTS


def test_action_list_struct_matches_header_layout():
    """The binding's struct field by field against the header's: names, order, element types, array lengths, offsets -- and the size a
    C compiler gives that layout (natural alignment: 4 int32 | 4 double | int32 | 3 x 32 int32 | 4 bytes of padding | 5 x 32 double)."""
    m = re.search(r"typedef struct irlosc_action_list \{(.*?)\} irlosc_action_list;", _header(), flags=re.S)
    assert m, "struct irlosc_action_list"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t|uint32_t|double|uint8_t)\s+(\w+)(?:\[(\w+)\])?;", body)
    assert fields == [("int32_t", "n_actions", ""), ("int32_t", "active_dev", ""), ("int32_t", "passive_dev", ""),
                      ("int32_t", "passive_hold_orientation", ""), ("double", "passive_quat", "4"), ("int32_t", "nb", ""),
                      ("int32_t", "kind", "IRLOSC_MAX_ACTIONS"), ("int32_t", "xyz_from_start", "IRLOSC_MAX_ACTIONS"),
                      ("int32_t", "grip_ticks", "IRLOSC_MAX_ACTIONS"), ("double", "kp", "IRLOSC_MAX_ACTIONS"),
                      ("double", "max_error", "IRLOSC_MAX_ACTIONS"), ("double", "min_speed", "IRLOSC_MAX_ACTIONS"),
                      ("double", "max_speed", "IRLOSC_MAX_ACTIONS"), ("double", "gripper_force", "IRLOSC_MAX_ACTIONS")]
    mirror = type("Mirror", (C.Structure,), {"_fields_": [(n, CTYPES[t] * DIMS[dim] if dim else CTYPES[t]) for t, n, dim in fields]})
    assert [f[0] for f in _lib.ActionList._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.ActionList) == C.sizeof(mirror) == 16 + 32 + 4 + 3 * 128 + 4 + 5 * 256
    for name, _ in mirror._fields_:
        assert getattr(_lib.ActionList, name).offset == getattr(mirror, name).offset, name
        assert getattr(_lib.ActionList, name).size == getattr(mirror, name).size, name


# ---- action_list_tick against FleetActionSequenceRunner on a scripted EE stream ----------------------------------------------------
class StubOSC:
    """What FleetActionSequenceRunner.tick asks of its controller: the EE poses come from a script, the gains and targets it sets
    are kept for the comparison, the step returns nothing of interest."""

    def __init__(self, lay, stream):
        self.layout, self.stream, self.i = lay, stream, 0
        self.max_vel, self.tgt = None, None

    def upload_q(self, q, qd):
        pass

    def frontend(self):
        pass

    def download_records(self, keys=()):
        return {"ee_pose": self.stream[self.i]}

    def set_gains(self, kp, kv, ko, k, d, max_vel, null_kv=0.0):
        self.max_vel = np.array(max_vel)

    def set_targets(self, tgt):
        self.tgt = np.array(tgt)

    def step(self):
        return np.zeros((len(self.stream[0]), self.layout.n))


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def test_action_list_tick_is_the_fleet_runner_with_after_step_shifted_by_one_tick():
    """B = 5 robots, a list WP(object) GRIP(3 ticks) WP(list target) WP(start_pos), a scripted EE stream whose active arm moves a tenth
    of the way to its current target every tick (so every robot reaches every waypoint, at robot-dependent ticks), and one robot whose
    stream holds a NaN from the start.  Host loop: tick(ee[t]) then after_step(ee[t + 1]); restatement: action_list_tick(ee[t], t), whose
    step 1 IS that after_step.  Compared after every tick: action as of after_step, targets, max_vel0, gripper_force, grip_left, err."""
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    B, T = 5, 400
    rng = np.random.default_rng(5)
    ia, io = lay.dev_names.index("ur5right"), lay.dev_names.index("ur5left")
    objects = [{"thing": dict(pos=rng.uniform(-0.3, 0.3, 3), quat=_unit(rng.normal(size=4)), grip_offset=[0.0, 0.01, 0.05], grip_yaw=30.0 * b)}
               for b in range(B)]
    seq = [dict(action="WP", target_xyz="thing", target_abg="thing", offset="grip_offset", max_error=0.02),
           dict(action="GRIP", gripper_force=0.2, gripper_duration=0.003),
           dict(action="WP", target_xyz=[0.1, 0.2, 0.3], target_abg=[10, 20, 30], max_error=0.03, max_speed_xyz=1.0, min_speed_xyz=0.2),
           dict(action="WP", target_xyz="start_pos", max_error=0.05, kp=2.0)]
    for hold in (False, True):
        desc = aseq.compile_action_list(seq, objects, ia, io, tick_seconds=0.001, passive_hold_orientation=hold)
        assert list(desc["kind"]) == [0, 1, 0, 0] and list(desc["xyz_from_start"]) == [0, 0, 0, 1] and desc["grip_ticks"][1] == 3
        assert desc["kp"][0] == 6 and desc["kp"][3] == 2.0 and desc["max_speed"][2] == 1.0 and desc["min_speed"][2] == 0.2
        ee0 = np.concatenate([rng.uniform(-0.5, 0.5, (B, lay.ndev, 3)), _unit(rng.normal(size=(B, lay.ndev, 4)))], axis=2)
        ee0[B - 1, ia, 1] = np.nan                                 # this robot never advances
        stub = StubOSC(lay, [ee0])
        runner = aseq.FleetActionSequenceRunner(stub, gains, objects, seq, active_arm="right", tick_seconds=0.001, passive_hold_orientation=hold)
        state = aseq.action_list_state(B)
        tgt = ee0.copy()                                           # (the runner starts from the EE poses as targets)
        g, _, _ = pack_gains(lay, gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"],
                             np.broadcast_to(gains["max_vel"], (B, lay.ndev, 2)))
        ticks_done = set()
        for t in range(T):
            ee = stub.stream[t]
            prev_action = runner.action.copy()
            aseq.action_list_tick(state, ee, tgt, g, desc, t)
            assert np.array_equal(state["action"], prev_action), t          # step 1 = the after_step the host ran last tick
            stub.i = t
            runner.tick(None, None)
            assert np.array_equal(stub.tgt, tgt, equal_nan=True), t
            assert np.array_equal(runner.entered, state["entered"]) and np.array_equal(runner.grip_left, state["grip_left"]), t
            assert np.array_equal(runner.max_vel0, state["max_vel0"]) and np.array_equal(runner.gripper_force, state["gripper_force"]), t
            assert np.array_equal(runner.err, state["err"], equal_nan=True), t
            moved = runner.max_vel0 > 0
            assert np.array_equal(stub.max_vel[moved, ia, 0], g[moved, ia, 9]) and np.array_equal(stub.max_vel[:, :, 1], g[:, :, 10]), t
            # the next state: the active arm a tenth of the way (pose blended, quaternion renormalised), the passive arm drifts
            nxt = ee.copy()
            nxt[:, ia, :3] += 0.1 * (tgt[:, ia, :3] - ee[:, ia, :3])
            nxt[:, ia, 3:] = _unit(ee[:, ia, 3:] + 0.1 * (_unit(tgt[:, ia, 3:]) * np.sign(np.sum(_unit(tgt[:, ia, 3:]) * ee[:, ia, 3:], axis=1, keepdims=True)) - ee[:, ia, 3:]))
            nxt[:, io, :3] += 1e-4
            stub.stream.append(nxt)
            runner.after_step(nxt)
            ticks_done.update(np.nonzero(runner.done())[0])
        aseq.action_list_tick(state, stub.stream[T], tgt, g, desc, T)
        assert np.array_equal(state["action"], runner.action)
        assert np.all(state["action"][:B - 1] == 4) and state["action"][B - 1] == 0 and state["finished_tick"][B - 1] == -1
        assert len(set(state["finished_tick"][:B - 1])) >= 2 and state["finished_tick"][:B - 1].min() > 0


# ---- robots that a narrower run left out start their list on the first tick that runs them ---------------------------------------
def _closed_stream(state, ee, tgt, gains, desc, ticks, rows, ia):
    """action_list_tick over `ticks` on the first `rows` robots of (state, ee, tgt, gains), the active arm of those robots moving half
    of the way to its target's position after every tick (orientation kept: every pose of the list has the EE's own).  In place."""
    for t in ticks:
        aseq.action_list_tick(state, ee[:rows], tgt, gains, desc, t)
        ee[:rows, ia, :3] += 0.5 * (tgt[:rows, ia, :3] - ee[:rows, ia, :3])


def test_robots_that_start_three_ticks_late_equal_two_restatements_run_apart():
    """B = 6, the list WP GRIP(2) WP WP('start_pos'): robots 0..2 run ticks 0..59, robots 3..5 only ticks 3..59 of the same state (what
    irlosc_rollout_from_q over 3 robots and then over 6 does to a slot).  The late robots' list starts on tick 3: not judged there (their
    targets are the EE poses they start from, which the rule of tick 0 alone would judge as arrived and skip action 0 unentered),
    start_xyz taken there, action 0 entered.  Equal to the two halves run apart -- robots 0..2 for 60 ticks, robots 3..5 for 57 ticks
    from tick 0 -- in every field, targets and gain words, finished_tick of the late half offset by 3."""
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    B, H, T, LATE = 6, 3, 60, 3
    rng = np.random.default_rng(11)
    ia, io = 0, 1
    ee0 = np.concatenate([rng.uniform(-0.5, 0.5, (B, lay.ndev, 3)), _unit(rng.normal(size=(B, lay.ndev, 4)))], axis=2)
    pose = np.zeros((B, 4, 7))
    for a in (0, 2, 3):
        pose[:, a, :3] = ee0[:, ia, :3] + rng.uniform(0.05, 0.3, (B, 3)) * (a + 1)
        pose[:, a, 3:] = ee0[:, ia, 3:]
    desc = dict(n_actions=4, active_dev=ia, passive_dev=io, passive_hold_orientation=1, passive_quat=np.array(aseq.DEFAULT_EE_QUAT),
                kind=np.array([0, 1, 0, 0], np.int32), xyz_from_start=np.array([0, 0, 0, 1], np.int32), grip_ticks=np.array([1, 2, 1, 1], np.int32),
                kp=np.full(4, 2.0), max_error=np.full(4, 0.01), min_speed=np.full(4, 0.05), max_speed=np.full(4, 1.0),
                gripper_force=np.array([0.0, 0.2, 0.1, -0.08]), pose=pose)
    g0 = pack_gains(lay, gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], np.broadcast_to(gains["max_vel"], (B, lay.ndev, 2)))[0]

    def fresh(rows):
        return aseq.action_list_state(len(ee0[rows])), ee0[rows].copy(), ee0[rows].copy(), g0[rows].copy()

    st, ee, tgt, g = fresh(slice(None))
    _closed_stream(st, ee, tgt, g, desc, range(LATE), H, ia)
    assert np.all(st["entered"][H:] == -1) and np.array_equal(tgt[H:], ee0[H:]) and np.array_equal(g[H:], g0[H:])
    _closed_stream(st, ee, tgt, g, desc, range(LATE, T), B, ia)
    for rows, ticks, off in ((slice(0, H), range(T), 0), (slice(H, B), range(T - LATE), LATE)):
        s2, e2, t2, g2 = fresh(rows)
        _closed_stream(s2, e2, t2, g2, dict(desc, pose=pose[rows]), ticks, len(e2), ia)
        assert np.all(s2["action"] == 4) and s2["finished_tick"].min() > 0 and len(set(s2["finished_tick"])) >= 2
        for key in st:
            want = s2[key] + off if key == "finished_tick" else s2[key]
            assert np.array_equal(st[key][rows], want), (key, rows)
        assert np.array_equal(tgt[rows], t2) and np.array_equal(g[rows], g2) and np.array_equal(ee[rows], e2)
    assert np.abs(st["start_xyz"][H:] - ee0[H:, ia, :3]).max() == 0
