"""Joint rows of a rollout (-m gpu): irlosc_set_joints -- range stops, the gripper's equality rows and gripper drives as one torque per
hinge, computed on the device from the tick's coordinates and taken off the bias in front of the plant kernel (csrc/osc_joint.hpp) --
against the CPU oracle, against the NumPy restatement bit for bit, tick by tick and in pieces, against runs without rows, driven by the
action list, next to paths, pushes and walls, and the state rules.

The helpers are those of test_pushes.py / test_rollout.py / test_rollout_layouts.py / test_action_list.py; the torque of a tick is
irl_control_amd/joints.py's (held to a plain loop by tests/test_joints_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import test_action_list as tal
import test_action_list_layouts as tall
import test_pushes as tp
import test_rollout as tr
import test_rollout_layouts as trl
import test_walls as twl
import test_waypoints as tw
from irl_control_amd import _lib, joints as jt, synth
from irl_control_amd.rigid_body import RigidBodyModel

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
DT = 1e-3
ERR_ARG, ERR_STATE = tr.ERR_ARG, tr.ERR_STATE
BAD = tp.BAD
B0 = 130                 # two full walk waves and a ragged one of two lanes
KEYS = tp.KEYS
STATE = ("tau", "max_violation", "active_ticks", "ctrl")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dual_ur5_joints.json")
NAMES = RigidBodyModel.load("dual_ur5").joint_names
FINGERS = [j for j, n in enumerate(NAMES) if "knuckle" in n or "finger" in n]
KNUCKLE = {d: NAMES.index(f"right_outer_knuckle_joint_{d}") for d in ("ur5right", "ur5left")}
# penalties of the multi-tick tests: far below the explicit bound M_jj / dt^2 = 16 N m / rad of an inner-finger hinge (profiles/joint_rates.md)
LK, LC, CK, CC = 2.0, 0.004, 1.0, 0.002
same = tp.same


def same_state(a, b, rows=slice(None)):
    for key in STATE:
        assert np.array_equal(a[key][rows], b[key][rows]), key


def arms_of(lay):
    return [d for d in lay.dev_names if d != "base"]


def scene(lay, lk=LK, lc=LC, ck=CK, cc=CC, **kw):
    """The scene's rows for a layout: ACTION drives for the arms the layout has"""
    return jt.scene_rows(FIXTURE, lk, lc, ck, cc, devices=arms_of(lay), **kw)


class Restated:
    """The per-robot state of the rows, carried by joints.joint_torque"""

    def __init__(self, lay, rows, B):
        self.desc, self.table = jt.normalise(rows, NAMES, lay.dev_names, B)
        R = self.table.shape[1]
        self.st = dict(tau=np.zeros((B, 25)), max_violation=np.zeros((B, R)), active_ticks=np.zeros((B, R), np.int32), ctrl=np.zeros((B, R)))

    def tick(self, q, qd, gripper_force=None, active=None):
        tau, ctrl, viol, on = jt.joint_torque(q, qd, self.desc, self.table, self.st["ctrl"], gripper_force, active, with_active=True)
        mv = self.st["max_violation"]
        with np.errstate(invalid="ignore"):
            mv = np.where(viol > mv, viol, mv)
        self.st = dict(tau=tau, max_violation=mv, active_ticks=self.st["active_ticks"] + on.astype(np.int32), ctrl=ctrl)
        return self.st


# ---- 1. one tick against the oracle ---------------------------------------------------------------------------------------------------
K1, C1 = 2.0, 0.5        # the stops of this test: c large enough that a moderate qd clamps a stop (one tick: stability is not at stake)
USED_ARM = ("joint0_ur5right", "joint4_ur5right", "joint0_ur5left", "joint4_ur5left")      # (hinge 1 differs from states1(): the oracle's cache key)
_S1 = {}


def states1():
    """test_pushes.states1() with the finger hinges and two arm hinges per arm overwritten from a seeded generator: per hinge a
    third of the robots 0.01 .. 0.3 rad below its range, a third inside, a third above; of those outside every fourth leaves so fast that
    the stop is clamped (f < 0).  One state set for every layout (the rows do not depend on the layout's devices, and test_rollout's
    oracle cache holds one set).  -> q, qd, used hinge indices"""
    key = "q"
    if key not in _S1:
        fx = jt.load_fixture(FIXTURE)
        q, qd = (x.copy() for x in tp.states1())
        rng = np.random.default_rng(606)
        used = [j for j, n in enumerate(NAMES) if j in FINGERS or n in USED_ARM]
        for j in used:
            lo, hi = fx["joints"][NAMES[j]]["range"]
            where = rng.permutation(len(q)) % 3
            out = rng.uniform(0.01, 0.3, len(q))
            q[:, j] = np.where(where == 0, lo - out, np.where(where == 2, hi + out, rng.uniform(lo + 1e-3, hi - 1e-3, len(q))))
            clamp = (rng.permutation(len(q)) % 4 == 0) & (where != 1)
            leave = 1.5 * K1 * out / C1 * np.where(where == 0, 1.0, -1.0)
            qd[:, j] = np.where(clamp, leave, qd[:, j])
        _S1[key] = (q, qd, used)
    return _S1[key]


@pytest.mark.parametrize("name", ["k13", "br7"])
def test_one_tick_against_the_oracle(name, monkeypatch):
    """The 256 states of states1() above; the full scene set (k = 2, c = 0.5 on the stops, k = 1, c = 0.002 on the couplings) plus a CONST
    drive per arm with per-robot values.  Asserted on the inputs first, excluding no robot: per LIMIT row on an overwritten hinge at least
    32 robots outside, 32 inside and 4 clamped, min |g| > 1e-6.  Then: tau equals joints.joint_torque on the uploaded coordinates bit for
    bit; qvel_with - qvel_without equals dt M^-1 tau, and qvel / qpos the reference step with tau on the right-hand side, within the bound
    of test_rollout.test_one_tick_against_the_cpu_oracles (its formula, its C_BOUND; M from oracle/rigid_body.py, np.linalg.solve).
    br7: the base is device 0 -- a hinge-index mix-up lands on the wrong hinges."""
    B = tp.B1
    if name == "k13":
        lay, gains, g, model, osc = tr.make_ctx("k13", B, F64, seed=21, n_slots=2)
        assert "fused" in osc.from_q_name
    else:
        lay, gains, g, model, osc = trl.open_ctx(name, B, F64, monkeypatch, seed=21, n_slots=2)
    arms = arms_of(lay)
    qpos, qvel, used = states1()
    rng = np.random.default_rng(17)
    rows = scene(lay, K1, C1) + [dict(kind="drive", joint=f"left_outer_knuckle_joint_{d}", gear=1.5, value=rng.normal(0.0, 0.05, B)) for d in arms]
    desc, table = jt.normalise(rows, NAMES, lay.dev_names, B)
    assert table.shape == (B, 34 + 2 * len(arms), 8)
    for r in np.flatnonzero(desc["kind"] == jt.LIMIT):
        j = int(desc["joint_a"][r])
        if j not in used:
            continue
        g_lo, g_hi = table[:, r, 0] - qpos[:, j], qpos[:, j] - table[:, r, 1]
        f_lo, f_hi = K1 * g_lo - C1 * qvel[:, j], K1 * g_hi + C1 * qvel[:, j]
        outside, clamped = (g_lo > 0) | (g_hi > 0), ((g_lo > 0) & (f_lo < 0)) | ((g_hi > 0) & (f_hi < 0))
        assert outside.sum() >= 32 and (~outside).sum() >= 32 and clamped.sum() >= 4, (NAMES[j], outside.sum(), clamped.sum())
        assert min(np.abs(g_lo).min(), np.abs(g_hi).min()) > 1e-6
    osc.set_plant(DT, 0.0)
    for slot in (0, 1):
        osc.upload_q(qpos, qvel, slot=slot)
        trl.set_targets(osc, g, slot)
    osc.set_joints(rows, slot=0)
    out, plain = osc.rollout(1, slot=0), osc.rollout(1, slot=1)
    st = osc.joint_state(0)
    osc.close()
    assert np.array_equal(out["u"], plain["u"]) and np.array_equal(out["flags_any"], plain["flags_any"]) and not np.any(out["flags_any"] & BAD)
    ref = Restated(lay, rows, B).tick(qpos, qvel)
    same_state(st, ref)
    tau = st["tau"]
    assert np.all(np.count_nonzero(tau[:, used], axis=1) >= 4)
    M, bias = tr.oracle_M_bias(qpos, qvel)
    qv_ref, qp_ref, bv, bp, unit = tp.plant_reference(M, bias, qpos, qvel, out["u"], tau)
    ev = np.abs(out["qvel"] - qv_ref).max(axis=1)
    ep = np.abs(out["qpos"] - qp_ref).max(axis=1)
    dv = DT * np.linalg.solve(M, tau[:, :, None])[:, :, 0]
    ed = np.abs((out["qvel"] - plain["qvel"]) - dv).max(axis=1)
    edp = np.abs((out["qpos"] - plain["qpos"]) - DT * dv).max(axis=1)
    print(f"[joints one tick {name}] worst qvel error / (dt eps cond max|qacc|) = {(ev / (DT * unit)).max():.3g} (bound {tr.C_BOUND:g}); difference "
          f"against dt M^-1 tau: worst error / bound {(ed / bv).max():.3g}; max |tau| {np.abs(tau).max():.3g}, max |dqvel| {np.abs(dv).max():.3g}")
    assert np.all(ev <= bv), (float((ev / bv).max()), int(np.argmax(ev / bv)))
    assert np.all(ep <= bp), (float((ep / bp).max()), int(np.argmax(ep / bp)))
    assert np.all(ed <= bv), (float((ed / bv).max()), int(np.argmax(ed / bv)))
    assert np.all(edp <= bp), (float((edp / bp).max()), int(np.argmax(edp / bp)))
    assert np.all(np.abs(dv).max(axis=1) > bv)      # and the rows acted, on every robot


# ---- 2. tick by tick ----------------------------------------------------------------------------------------------------------------------
CASES = ("k12_admit", "br7", "rlb16", "k13_lane0", "k12_admit_f32")


def mixed_rows(lay, B, per_robot):
    """The scene set plus narrow stops on two arm hinges per arm (random_state draws the arms from [-pi, pi]: about two thirds of the
    robots start outside [-1, 1]), a second stop on one of them (the order of the sum) and a CONST drive per arm"""
    rng = np.random.default_rng(23)
    v = (lambda lo, hi: rng.uniform(lo, hi, B)) if per_robot else (lambda lo, hi: 0.5 * (lo + hi))
    rows = scene(lay)
    for d in arms_of(lay):
        rows += [dict(kind="limit", joint=f"joint1_{d}", lo=v(-1.2, -0.8), hi=v(0.8, 1.2), stiffness=v(30.0, 60.0), damping=v(1.0, 3.0)),
                 dict(kind="limit", joint=f"joint3_{d}", lo=-0.5, hi=1.5, stiffness=20.0, damping=v(0.0, 1.0)),
                 dict(kind="limit", joint=f"joint1_{d}", lo=-2.0, hi=2.0, stiffness=v(5.0, 10.0)),
                 dict(kind="drive", joint=f"left_outer_knuckle_joint_{d}", gear=v(0.5, 1.5), value=v(-0.02, 0.04))]
    return rows


@pytest.mark.parametrize("per_robot", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_T_ticks_equal_T_single_ticks_equal_pieces_and_the_restatement(case, per_robot, monkeypatch):
    """rollout(6) on slot 0, 6 x rollout(1) on slot 1, rollout(2) + rollout(1) + rollout(3) on slot 2: qpos, qvel, u, the OR of the flags
    and the rows' state bit for bit.  Before every single tick the coordinates are downloaded, and joints.joint_torque on them equals the
    tau downloaded after the tick bit for bit; max_violation, active_ticks and ctrl follow the restatement."""
    B, T = B0, 6
    lay, gains, g, model, osc, _, _ = tp.open_case(case, B, monkeypatch, seed=5, n_slots=3)
    tp.start(osc, model, g, B, (0, 1, 2))
    rows = mixed_rows(lay, B, per_robot)
    for slot in (0, 1, 2):
        osc.set_joints(rows, slot=slot)
    ref = Restated(lay, rows, B)
    assert ref.table.shape[0] == (B if per_robot else 1)
    a = osc.rollout(T, slot=0)
    fl = np.zeros(B, np.uint32)
    for t in range(T):
        q, qd = osc.download_q(1)
        b = osc.rollout(1, slot=1)
        fl |= b["flags_any"]
        same_state(osc.joint_state(1), ref.tick(q, qd))
    fc = np.zeros(B, np.uint32)
    for n in (2, 1, 3):
        c = osc.rollout(n, slot=2)
        fc |= c["flags_any"]
    sa, sc = osc.joint_state(0), osc.joint_state(2)
    osc.close()
    assert np.all(np.isfinite(a["qpos"])) and np.all(np.isfinite(a["u"])) and not np.any(a["flags_any"] & BAD)
    same(a, b, ("qpos", "qvel", "u"))
    same(a, c, ("qpos", "qvel", "u"))
    assert np.array_equal(a["flags_any"], fl) and np.array_equal(a["flags_any"], fc)
    same_state(sa, ref.st)
    same_state(sc, ref.st)
    kinds = ref.desc["kind"]
    assert np.all(ref.st["active_ticks"][:, kinds == jt.COUPLE] == T)                  # random fingers: every coupling acts on every tick
    lim = ref.st["active_ticks"][:, kinds == jt.LIMIT]
    assert (lim == T).any() and (lim == 0).any() and np.any((lim > 0) & (lim < T))      # stops held, never touched, and entered or left
    assert np.all(ref.st["max_violation"][:, kinds == jt.DRIVE] == 0.0) and not ref.st["ctrl"][:, kinds != jt.DRIVE].any()


# ---- 3. what a row leaves alone -------------------------------------------------------------------------------------------------------------
def test_rows_that_give_no_torque_change_nothing():
    """Stops nobody reaches, couplings with k = c = 0 and a zero drive: every output of 4 ticks, the EE trace included, is that of a slot
    without rows, bit for bit; tau is zero and nothing was counted."""
    B, T = B0, 4
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    tp.start(osc, model, g, B, (0, 1))
    rows = [dict(r, lo=-100.0, hi=100.0) if r["kind"] == "limit" else r for r in scene(lay, ck=0.0, cc=0.0, drive=0.0)]
    osc.set_joints(rows, slot=0)
    a, b = osc.rollout(T, trace_every=1, slot=0), osc.rollout(T, trace_every=1, slot=1)
    st = osc.joint_state(0)
    osc.close()
    same(a, b, KEYS + ("ee_trace",))
    assert not st["tau"].any() and not st["active_ticks"].any() and not st["ctrl"].any()
    assert st["max_violation"][:, 24:34].min() > 0.0 and not st["max_violation"][:, :24].any()      # |e| is seen all the same


def test_a_robot_outside_its_stop_is_alone():
    """One stop [-3.2, 3.2] on an arm hinge, every robot inside but robot 70 (at 3.5): its wave mates and everybody else equal the slot
    without rows bit for bit over 4 ticks, robot 70 does not."""
    B, T, ODD = B0, 4, 70
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    qpos, qvel, _ = tp.start(osc, model, g, B, (0, 1))
    j = NAMES.index("joint1_ur5left")
    qpos = qpos.copy()
    qpos[ODD, j] = 3.5
    for slot in (0, 1):
        osc.upload_q(qpos, qvel, slot=slot)
    osc.set_joints([dict(kind="limit", joint=j, lo=-3.2, hi=3.2, stiffness=40.0, damping=1.0)], slot=0)
    a, b = osc.rollout(T, trace_every=1, slot=0), osc.rollout(T, trace_every=1, slot=1)
    st = osc.joint_state(0)
    osc.close()
    others = np.arange(B) != ODD
    same(a, b, KEYS, rows=others)
    assert np.array_equal(a["ee_trace"][:, others], b["ee_trace"][:, others])
    assert np.abs(a["qvel"][ODD] - b["qvel"][ODD]).max() > 0.0 and st["active_ticks"][ODD, 0] == T and not st["active_ticks"][others].any()
    assert st["tau"][ODD, j] < 0.0 and not st["tau"][others].any() and np.count_nonzero(st["tau"][ODD]) == 1


def test_a_robot_with_nan_coordinates_is_alone_and_gets_no_torque():
    """The full scene set and the mixed stops, no CONST drive (its torque does not depend on the coordinates); robot 5's coordinates are
    all NaN on slot 0 and finite on slot 1: every other robot is bit-identical over 3 ticks, state included, and robot 5's tau is all
    zero and none of its rows ever acted (no row sees a contact in a NaN)."""
    B, T, ODD = B0, 3, 5
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    qpos, qvel, _ = tp.start(osc, model, g, B, (0, 1))
    bad = qpos.copy()
    bad[ODD] = np.nan
    osc.upload_q(bad, qvel, slot=0)
    rows = [r for r in mixed_rows(lay, B, True) if not (r["kind"] == "drive" and r.get("source", "const") == "const")]
    for slot in (0, 1):
        osc.set_joints(rows, slot=slot)
    a, b = osc.rollout(T, slot=0), osc.rollout(T, slot=1)
    sa, sb = osc.joint_state(0), osc.joint_state(1)
    osc.close()
    others = np.arange(B) != ODD
    same(a, b, KEYS, rows=others)
    same_state(sa, sb, rows=others)
    assert not sa["tau"][ODD].any() and not sa["active_ticks"][ODD].any() and not sa["max_violation"][ODD].any()
    assert a["flags_any"][ODD] & _lib.FLAG_NONFINITE and np.count_nonzero(sb["tau"][ODD]) >= 12


# ---- 4. the ACTION drive --------------------------------------------------------------------------------------------------------------------
FORCES = np.array([0.0, -0.08, 0.0, 0.05])


def grip_scenario(B, **kw):
    """WP GRIP(-0.08) WP(0.0) GRIP(+0.05) with two-tick GRIPs on near poses, 16 ticks (test_action_list_layouts.short_scenario: robots
    stall at different actions, so some never grip)"""
    sc = tall.short_scenario(B, actions=(tall.W, tall.G(2), tall.W, tall.G(2)), late=(), **kw)
    return dict(sc, desc=dict(sc["desc"], gripper_force=FORCES))


def test_the_action_drive_follows_the_list_on_the_tick_a_grip_is_entered():
    """k13, the right arm runs the list.  Slot 0 has the scene set with ACTION drives, slot 1 the same without drives.  Tick by tick:
    ctrl is gripper_force under the hold rule (a non-zero force replaces it, 0.0 keeps the grip), the left hand's ctrl stays 0; tau
    equals the restatement fed with the gripper_force downloaded AFTER the tick, bit for bit, and fed with the one of the tick before it
    does not on a tick that enters a GRIP; on that very tick the driven knuckle's qvel departs from slot 1's, having been equal to it
    until then.  Afterwards the list is cleared: two more ticks keep ctrl."""
    B, T = B0, tall.T
    sc = grip_scenario(B)
    lay = synth.make_layout("k13")
    ia = sc["desc"]["active_dev"]
    assert lay.dev_names[ia] == "ur5right"
    osc = tal.make_ctx(B, n_slots=2)
    for slot in (0, 1):
        tal.fill(osc, sc, slot)
        osc.set_action_list(sc["desc"], slot=slot)
    rows = scene(lay)
    osc.set_joints(rows, slot=0)
    osc.set_joints(scene(lay, drive=None), slot=1)
    ref = Restated(lay, rows, B)
    r_right, r_left = 34, 35
    assert rows[r_right]["dev"] == "ur5right" and rows[r_left]["dev"] == "ur5left"
    kn = KNUCKLE["ur5right"]
    gf_prev = np.zeros(B)
    driven = np.zeros(B, bool)
    late_fails = entered = 0
    for t in range(T):
        q, qd = osc.download_q(0)
        a, b = osc.rollout(1, slot=0), osc.rollout(1, slot=1)
        gf = osc.action_state(0)["gripper_force"]
        st = osc.joint_state(0)
        want = np.where(gf != 0.0, gf, ref.st["ctrl"][:, r_right])
        assert np.array_equal(st["ctrl"][:, r_right], want) and not st["ctrl"][:, r_left].any(), t
        late = jt.joint_torque(q, qd, ref.desc, ref.table, ref.st["ctrl"], gf_prev, ia)[0]
        if np.any(want != ref.st["ctrl"][:, r_right]):      # a tick on which some robot enters a GRIP with a new force
            entered += 1
            late_fails += int(not np.array_equal(late, st["tau"]))
        same_state(st, ref.tick(q, qd, gf, ia))
        now = (want != 0.0) & ~driven                  # robots whose first GRIP was entered on this tick
        if now.any():
            assert np.all(a["qvel"][now, kn] != b["qvel"][now, kn]), t
        still = ~(driven | now)
        same(a, b, ("qpos", "qvel"), rows=still)       # until its drive starts a robot is the robot without drives
        driven |= now
        gf_prev = gf
    assert entered >= 2 and late_fails == entered
    assert 16 <= driven.sum() < B
    assert set(np.unique(ref.st["ctrl"][:, r_right])) == {0.0, -0.08, 0.05}
    assert np.all(np.sign(a["qvel"][driven, kn] - b["qvel"][driven, kn]) != 0)
    assert not np.any(a["flags_any"] & BAD)
    osc.set_action_list(None, slot=0)
    q, qd = osc.download_q(0)
    osc.rollout(1, slot=0)
    same_state(osc.joint_state(0), ref.tick(q, qd))
    osc.rollout(1, slot=0)
    assert np.array_equal(osc.joint_state(0)["ctrl"][:, r_right], ref.st["ctrl"][:, r_right]) and ref.st["ctrl"][:, r_right].any()
    osc.close()


def test_a_list_on_the_other_arm_leaves_the_drive_idle():
    """The list runs on ur5left: the right hand's ACTION drive keeps ctrl = 0 through 16 ticks, the left hand's takes the forces."""
    B, T = B0, tall.T
    lay = synth.make_layout("k13")
    names = list(lay.dev_names)
    sc = grip_scenario(B, active=names.index("ur5left"), passive=names.index("ur5right"))
    osc = tal.make_ctx(B)
    tal.fill(osc, sc, 0)
    osc.set_action_list(sc["desc"])
    osc.set_joints(scene(lay))
    out = osc.rollout(T)
    st, gf = osc.joint_state(), osc.action_state()["gripper_force"]
    osc.close()
    assert not np.any(out["flags_any"] & BAD)
    assert not st["ctrl"][:, 34].any() and not st["active_ticks"][:, 34].any()
    assert st["ctrl"][:, 35].any() and np.array_equal(st["ctrl"][:, 35] != 0.0, st["active_ticks"][:, 35] > 0)
    assert np.all(st["ctrl"][gf != 0.0, 35] == gf[gf != 0.0])


# ---- 5. next to the others ------------------------------------------------------------------------------------------------------------------
def test_rows_next_to_pushes_and_walls_on_the_same_arm():
    """k12_admit with a sensor feed: an applied-and-sensed push, two walls and the mixed rows on the left arm -- rollout(6) equals 6 x
    rollout(1) bit for bit, wall and joint state included, and each of the three acted (against the run that lacks it)."""
    B, T = B0, 6
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=4)
    tp.start(osc, model, g, B, (0, 1, 2, 3))
    d = list(lay.dev_names).index("ur5left")
    ws = twl.median_walls(twl.ee_now(osc, 3), (d,))
    W = tp.wrenches(np.random.default_rng(14), B, 1)
    rows = mixed_rows(lay, B, True)
    for slot in (0, 1, 2):
        osc.set_pushes([dict(dev=d, window=(1, 5))], W, slot=slot)
        osc.set_walls(ws, slot=slot)
        if slot < 2:
            osc.set_joints(rows, slot=slot)
    a = osc.rollout(T, slot=0)
    fl = np.zeros(B, np.uint32)
    for _ in range(T):
        b = osc.rollout(1, slot=1)
        fl |= b["flags_any"]
    no_rows = osc.rollout(T, slot=2)
    twl.same_state(osc.wall_state(0), osc.wall_state(1))
    same_state(osc.joint_state(0), osc.joint_state(1))
    touched = osc.wall_state(0)["contact_ticks"][:, d] > 0
    osc.close()
    same(a, b, ("qpos", "qvel", "u"))
    assert np.array_equal(a["flags_any"], fl) and not np.any(fl & BAD)
    assert np.all(np.abs(a["qvel"] - no_rows["qvel"]).max(axis=1) > 0.0) and touched.sum() >= 32


def test_rows_next_to_waypoint_paths():
    """k13 with paths on both arms and the mixed rows: rollout(8) equals 8 x rollout(1), waypoint and joint state included, and neither
    setter ended the other's state."""
    B, T = B0, 8
    sc = tw.scenario(B, False)
    lay = synth.make_layout("k13")
    osc = tw.make_ctx(B, n_slots=2)
    rows = mixed_rows(lay, B, False)
    for slot in (0, 1):
        tw.fill(osc, sc, slot)
        osc.set_joints(rows, slot=slot)
        osc.set_waypoints(sc["paths"] + [None], tw.THRESHOLD, True, slot=slot)
    a = osc.rollout(T, slot=0)
    for _ in range(T):
        b = osc.rollout(1, slot=1)
    wa, wb = osc.waypoint_state(0), osc.waypoint_state(1)
    same_state(osc.joint_state(0), osc.joint_state(1))
    st = osc.joint_state(0)
    osc.close()
    same(a, b, ("qpos", "qvel", "u"))
    for key in ("index", "arrivals", "last_tick"):
        assert np.array_equal(wa[key], wb[key]), key
    # (the fingers start at 0 and at rest: on tick 0 every coupling has e = 0 and gives nothing; from tick 1 on gravity has moved them)
    assert not np.any(a["flags_any"] & BAD) and np.all(st["active_ticks"][:, 24:34] == T - 1)


# ---- 6. state rules -------------------------------------------------------------------------------------------------------------------------
def make_desc(kind=(0, 1, 2), ja=(2, 8, 9), jb=(0, 7, 0), source=(0, 0, 1), dev=(0, 0, 1), per_robot=0, R=None):
    d = _lib.JointRows()
    d.n_rows, d.per_robot = len(kind) if R is None else R, per_robot
    for r in range(len(kind)):
        d.kind[r], d.joint_a[r], d.joint_b[r], d.source[r], d.dev[r] = kind[r], ja[r], jb[r], source[r], dev[r]
    return d


def good_table(nb=1):
    t = np.zeros((nb, 3, 8))
    t[:, 0, :4] = (-1.0, 1.0, 30.0, 1.0)
    t[:, 1, :6] = (0.0, -1.1, 0.0, 0.0, 1.0, 0.002)
    t[:, 2, :2] = (1.0, 0.0)
    return t


def rc_set(osc, B, desc, t, slot=0):
    return osc.lib.irlosc_set_joints(osc._h, slot, B, None if desc is None else C.byref(desc), None if t is None else _lib.ptr(np.ascontiguousarray(t)))


def rc_get(osc, B, slot=0, R=3):
    tau, mv, at, ct = np.empty((B, 25)), np.empty((B, R)), np.empty((B, R), np.int32), np.empty((B, R))
    return osc.lib.irlosc_download_joint_state(osc._h, slot, B, _lib.ptr(tau), _lib.ptr(mv), _lib.ptr(at), _lib.ptr(ct))


def edited(i, v, row=0, nb=1, robot=0):
    t = good_table(nb)
    t[robot, row, i] = v
    return t


def test_state_rules():
    B = B0
    lay = synth.make_layout("k12_admit")
    _, gains, g = synth.make_batch("k12_admit", B, seed=5)
    model = RigidBodyModel.load("dual_ur5")
    from irl_control_amd import BatchedOSC
    osc = BatchedOSC(lay, B, dtype=F64, n_slots=3)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    assert rc_set(osc, B, make_desc(), good_table()) == ERR_STATE and b"irlosc_set_model" in osc.lib.irlosc_last_error(osc._h)
    osc.set_model(model)
    osc.set_ft_sensors()
    qpos, qvel, sens = tp.start(osc, model, g, B, (0, 1, 2))
    assert rc_get(osc, B) == ERR_STATE and b"no joint rows" in osc.lib.irlosc_last_error(osc._h)
    # rows in force on slots 0 and 1 (the twin that sees no refusal), two ticks run
    for slot in (0, 1):
        assert rc_set(osc, B, make_desc(), good_table(), slot) == 0
        osc._joint_rows[slot] = 3
        osc.rollout(2, slot=slot)
    refusals = [
        (make_desc(R=0), good_table(), b"n_rows"), (make_desc(R=49), good_table(), b"n_rows"),
        (make_desc(per_robot=2), good_table(), b"per_robot"),
        (make_desc(kind=(0, 1, 3)), good_table(), b"kind"), (make_desc(kind=(-1, 1, 2)), good_table(), b"kind"),
        (make_desc(ja=(25, 8, 9)), good_table(), b"joint_a"), (make_desc(ja=(2, 8, -1)), good_table(), b"joint_a"),
        (make_desc(jb=(0, 25, 0)), good_table(), b"joint_b"), (make_desc(jb=(0, 8, 0)), good_table(), b"with itself"),
        (make_desc(source=(0, 0, 2)), good_table(), b"source"), (make_desc(dev=(0, 0, lay.ndev)), good_table(), b"dev"),
        (make_desc(), None, b"NULL"),
        (make_desc(), edited(7, np.nan, row=1), b"not finite"), (make_desc(), edited(1, np.inf, row=2), b"not finite"),
        (make_desc(per_robot=1), edited(0, np.nan, nb=B, robot=B - 1), b"not finite"),
        (make_desc(), edited(0, 1.0), b"lo >= hi"), (make_desc(), edited(1, -2.0), b"lo >= hi"),
        (make_desc(), edited(2, -1.0), b"must be >= 0"), (make_desc(), edited(3, -1.0), b"must be >= 0"),
        (make_desc(), edited(4, -1.0, row=1), b"must be >= 0"), (make_desc(), edited(5, -1.0, row=1), b"must be >= 0"),
        (make_desc(per_robot=1), edited(2, -1.0, nb=B, robot=77), b"must be >= 0"),
    ]
    for desc, t, why in refusals:
        assert rc_set(osc, B, desc, t) == ERR_ARG, why
        assert why in osc.lib.irlosc_last_error(osc._h), (why, osc.lib.irlosc_last_error(osc._h))
    assert rc_set(osc, 0, make_desc(), good_table()) == ERR_ARG and rc_set(osc, B + 1, make_desc(), good_table()) == ERR_ARG
    assert rc_set(osc, B, make_desc(), good_table(), slot=3) == ERR_ARG
    assert rc_get(osc, B + 1) == ERR_ARG
    # ... and the rows in force are whole: state, tick and the next ticks are the twin's
    same_state(osc.joint_state(0), osc.joint_state(1))
    assert np.all(osc.joint_state(0)["active_ticks"][:, 1] == 2)
    # what does not end them: uploads, targets, sensordata, programs, pushes, walls -- the counters go on
    for slot in (0, 1):
        osc.upload_q(qpos, qvel, slot=slot)
        trl.set_targets(osc, g, slot)
        osc.set_sensordata(sens, slot=slot)
    osc.set_pushes([dict(dev=1, window=(50, 60))], tp.wrenches(np.random.default_rng(1), B, 1), slot=0)
    osc.set_walls([dict(dev=1, normal=(0.0, 0.0, 1.0), offset=-50.0, stiffness=10.0)], slot=0)
    osc.set_waypoints([np.array([[0.3, 0.45, 0.5], [0.32, 0.45, 0.5]]), None], 0.01, slot=0)
    trl.set_targets(osc, g, 0)
    osc.clear_pushes(slot=0)
    a, b = osc.rollout(2, slot=0), osc.rollout(2, slot=1)
    same(a, b)
    same_state(osc.joint_state(0), osc.joint_state(1))
    assert np.all(osc.joint_state(0)["active_ticks"][:, 1] == 4)
    osc.clear_walls(slot=0)
    # a successful setter resets state and tick
    assert rc_set(osc, B, make_desc(), good_table()) == 0
    st = osc.joint_state(0)
    assert not st["tau"].any() and not st["active_ticks"].any() and not st["max_violation"].any() and not st["ctrl"].any()
    # a rollout narrower than the rows runs; one wider is refused, and so is a wider download
    osc.upload_q(qpos[:64], qvel[:64], slot=2)
    trl.set_targets(osc, {k: v[:64] if isinstance(v, np.ndarray) and len(v) == B else v for k, v in g.items()}, 2)
    osc.set_sensordata(sens[:64], slot=2)
    assert rc_set(osc, 64, make_desc(), good_table(), slot=2) == 0
    osc._joint_rows[2] = 3
    osc.rollout(1, slot=2)
    osc.upload_q(qpos[:40], qvel[:40], slot=2)
    trl.set_targets(osc, {k: v[:40] if isinstance(v, np.ndarray) and len(v) == B else v for k, v in g.items()}, 2)
    osc.set_sensordata(sens[:40], slot=2)
    narrow = osc.rollout(1, slot=2)
    assert np.all(np.isfinite(narrow["qpos"])) and osc.joint_state(2)["tau"].shape == (40, 25)
    assert np.all(osc.joint_state(2)["active_ticks"][:, 1] == 2)      # (robots 0 .. 39 ran both ticks: the state is the robot's, not the call's)
    tp.start(osc, model, g, B, (2,))
    assert tr._rc_rollout(osc, B, 1, slot=2) == ERR_STATE and b"joint rows cover 64" in osc.lib.irlosc_last_error(osc._h)
    assert rc_get(osc, B, slot=2) == ERR_STATE and b"cover 64" in osc.lib.irlosc_last_error(osc._h)
    # what ends them: the setter with NULL, and set_model (every slot)
    osc.clear_joints(slot=0)
    assert rc_get(osc, B) == ERR_STATE
    assert rc_get(osc, B, slot=1) == 0
    plain = osc.rollout(1, slot=0)                      # (and the slot rolls out without them)
    assert np.all(np.isfinite(plain["qpos"]))
    osc.set_model(model)
    assert rc_get(osc, B, slot=1) == ERR_STATE and rc_get(osc, 64, slot=2) == ERR_STATE
    osc.close()


def test_two_slots_with_different_rows_interleaved():
    """Slot 0 has the mixed rows per robot, slot 1 the scene set with other penalties; rollout(2) calls alternate between them, three
    each.  Each slot equals its solo run of 6 ticks on a context of its own, state included."""
    B, T = B0, 6
    lay = synth.make_layout("k12_admit")
    sets = (mixed_rows(lay, B, True), scene(lay, 1.0, 0.002, 0.5, 0.001, drive=0.03))
    solo = []
    for rows in sets:
        _, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5)
        tp.start(osc, model, g, B, (0,))
        osc.set_joints(rows)
        solo.append((osc.rollout(T), osc.joint_state()))
        osc.close()
    _, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    tp.start(osc, model, g, B, (0, 1))
    for slot, rows in enumerate(sets):
        osc.set_joints(rows, slot=slot)
    fl = [np.zeros(B, np.uint32), np.zeros(B, np.uint32)]
    for _ in range(3):
        outs = [osc.rollout(2, slot=slot) for slot in (0, 1)]
        for slot in (0, 1):
            fl[slot] |= outs[slot]["flags_any"]
    for slot in (0, 1):
        same(outs[slot], solo[slot][0], ("qpos", "qvel", "u"))
        assert np.array_equal(fl[slot], solo[slot][0]["flags_any"])
        same_state(osc.joint_state(slot), solo[slot][1])
    osc.close()
    assert np.abs(solo[0][0]["qvel"] - solo[1][0]["qvel"]).max() > 0.0


# ---- 7. the example -------------------------------------------------------------------------------------------------------------------------
def test_the_example_against_its_numpy_loop_and_closes_the_hands():
    """examples/gripper_fleet_resident_headless.py at B = 130 with the penalties its cpu_loop was run with.
    The first 8 ticks, tick by tick, against cpu_loop on the same scenario (the poses the run computed; robots 0, 1, 64 and 129: a CPU
    tick costs 35 ms per robot): qpos within 1e-9, the tolerance test_rollout.test_trajectory_against_the_host_loop applies to a rollout
    against a host loop (its floor; its spread term is 1e-13 there), and qvel within 1e-9 / dt -- qpos is dt x the sum of the qvel, so
    that is the same allowance on the quantity one integration earlier.  The GPU trajectory is not compared beyond these 8 ticks.
    Then 600 ticks: on every robot whose GRIP was entered the driven knuckle moved in the drive's direction (the force is positive:
    towards the upper stop), no robot is frozen, and the worst coupling error of the active hand over all ticks (the rows'
    max_violation) stays below 2 x the maximum cpu_loop reached over the same 600 ticks (tests/golden/gripper_cpu_loop.json, held to
    cpu_loop by tests/test_joints_host.py; the margin of 2 because the GPU controller's u differs from the NumPy loop's in the last
    bits and the loop amplifies that).
    Measured on an MI355X (printed; profiles/joint_rates.md): first 8 ticks max |dqpos| 2.2e-16 rad, max |dqvel| 6e-14 rad/s; 130 of 130
    robots enter the GRIP, knuckle at the end 0.31 .. 0.84 rad, worst coupling error 0.0591 rad of the 0.0909 allowed."""
    ex = tr._example("gripper_fleet_resident_headless")
    who = [0, 1, 64, 129]
    head = ex.run(robots=B0, ticks=8, trace_every=1, verbose=False)
    sc = {k: v[who] for k, v in head["scenario"].items()}
    cpu = ex.cpu_loop(robots=len(who), ticks=8, verbose=False, scenario=sc)
    gq = np.concatenate([head["q_log"], head["q"][None]])[:, who]
    gqd = np.concatenate([head["qd_log"], head["qd"][None]])[:, who]
    eq, ev = np.abs(gq - cpu["q_log"]).max(axis=(1, 2)), np.abs(gqd - cpu["qd_log"]).max(axis=(1, 2))
    print(f"[gripper example] first 8 ticks against the NumPy loop: max |dqpos| per tick {' '.join(f'{x:.2g}' for x in eq)}; max |dqvel| "
          f"{' '.join(f'{x:.2g}' for x in ev)}; max |qvel| {np.abs(cpu['qd_log']).max():.3g}")
    assert np.array_equal(gq[0], cpu["q_log"][0]) and not np.any(head["flags_any"] & BAD)
    assert eq.max() <= 1e-9 and ev.max() <= 1e-9 / DT, (eq.max(), ev.max())
    assert np.abs(cpu["qd_log"][-1][:, FINGERS]).max() > 1e-3      # and the hands are moving by then: there is something to compare
    r = ex.run(robots=B0, ticks=600, trace_every=100, verbose=False)
    entered = r["entered_grip"]
    rec = ex.cpu_record()
    assert rec["ticks"] == 600 and rec["finite"]
    bound = 2.0 * rec["couple_err_max"]
    print(f"[gripper example] {int(entered.sum())} of {B0} robots entered the GRIP; knuckle at the end {r['knuckle_end'][entered].min():.4f} .. "
          f"{r['knuckle_end'][entered].max():.4f} rad; worst coupling error {r['max_couple_err'].max():.4g} rad (bound {bound:.4g})")
    assert entered.sum() >= B0 // 2 and np.all(r["ctrl"][entered] == ex.FORCE)
    assert np.all(r["knuckle_end"][entered] > 0.0)
    assert not np.any(r["flags_any"] & BAD) and np.all(np.isfinite(r["q"]))
    assert r["max_couple_err"].max() < bound
