"""Joint rows of a rollout, the host side (no GPU): the ctypes mirror of struct irlosc_joint_rows, irl_control_amd/joints.py -- the NumPy
restatement of csrc/osc_joint.hpp against a plain per-robot loop over Python floats, the clamp regimes of a LIMIT, NaN coordinates, the
signs of a COUPLE, the hold rule of an ACTION drive, every refusal of normalise -- and the fixture tests/golden/dual_ur5_joints.json."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from irl_control_amd import _lib, joints as jt
from irl_control_amd.rigid_body import RigidBodyModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dual_ur5_joints.json")
DEVS = ["ur5right", "ur5left"]


def names():
    return RigidBodyModel.load("dual_ur5").joint_names


def test_struct_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "irlosc.h")).read()
    assert f"#define IRLOSC_MAX_JOINT_ROWS {_lib.MAX_JOINT_ROWS}" in hdr and _lib.MAX_JOINT_ROWS == jt.MAX_JOINT_ROWS == 48
    body = re.search(r"typedef struct irlosc_joint_rows \{(.*?)\} irlosc_joint_rows;", hdr, flags=re.S).group(1)
    fields = re.findall(r"int32_t\s+(\w+)(\[IRLOSC_MAX_JOINT_ROWS\])?;", body)
    assert [f for f, _ in fields] == [f for f, _ in _lib.JointRows._fields_]
    assert C.sizeof(_lib.JointRows) == 4 * (2 + 5 * 48)
    for nm, v in (("LIMIT", jt.LIMIT), ("COUPLE", jt.COUPLE), ("DRIVE", jt.DRIVE), ("SRC_CONST", jt.CONST), ("SRC_ACTION", jt.ACTION)):
        assert re.search(rf"#define IRLOSC_JOINT_{nm}\s+{v}\b", hdr), nm
    lib = _lib.load()
    assert hasattr(lib, "irlosc_set_joints") and hasattr(lib, "irlosc_download_joint_state")


def test_the_fixture_holds_the_scene():
    fx = jt.load_fixture(FIXTURE)
    lim = {n: j["range"] for n, j in fx["joints"].items() if j["limited"]}
    assert len(fx["joints"]) == 25 and len(lim) == 24 and "ur_stand_joint" not in lim
    assert list(fx["joints"]) == names()
    for n, r in lim.items():
        if "outer_knuckle" in n:
            assert r == [0.0, 0.8], n
        elif "inner_finger" in n:
            assert r == [-0.8757, 0.8757], n
        elif "inner_knuckle" in n:
            assert r == [0.0, 0.8757], n
        else:
            assert r == [-6.28319, 6.28319], n
    assert len(fx["equality"]) == 10
    for e in fx["equality"]:
        assert e["joint1"] in lim and e["joint2"] in lim and e["qpos0"] == [0.0, 0.0]
        assert e["polycoef"][0] == 0.0 and e["polycoef"][1] in (1.0, -1.1) and e["polycoef"][2:] == [0.0, 0.0, 0.0]
    assert [(m["name"], m["joint"], m["gear"]) for m in fx["gripper_motors"]] == [
        ("gripper_ur5right", "right_outer_knuckle_joint_ur5right", 1.0), ("gripper_ur5left", "right_outer_knuckle_joint_ur5left", 1.0)]


def test_scene_rows_yields_36_rows():
    rows = jt.scene_rows(FIXTURE, 2.0, 0.004, 1.0, 0.002)
    assert [r["kind"] for r in rows] == ["limit"] * 24 + ["couple"] * 10 + ["drive"] * 2
    desc, table = jt.normalise(rows, names(), DEVS, 7)
    assert table.shape == (1, 36, 8) and not desc["per_robot"]
    assert list(desc["dev"][-2:]) == [0, 1] and list(desc["source"][-2:]) == [jt.ACTION] * 2
    assert np.all(table[0, 24:34, 1] == [e["polycoef"][1] for e in jt.load_fixture(FIXTURE)["equality"]])
    assert len(jt.scene_rows(FIXTURE, 2.0, 0.0, 1.0, 0.0, drive=None)) == 34
    const = jt.scene_rows(FIXTURE, 2.0, 0.0, 1.0, 0.0, gear=2.0, drive=-0.08)
    assert const[-1]["source"] == "const" and const[-1]["value"] == -0.08 and const[-1]["gear"] == 2.0


# ---- the restatement against a plain loop over Python floats ----------------------------------------------------------------------------
def plain_loop(q, qd, desc, table, ctrl, gf=None, active=None):
    """The formulas of include/irlosc.h, one robot and one row at a time, on Python floats (IEEE doubles, one rounding per operation)"""
    B, n = q.shape
    R = table.shape[1]
    tau = np.zeros((B, n))
    ctrl = np.array(ctrl, dtype=np.float64)
    viol = np.zeros((B, R))
    fin = lambda x: abs(x) <= 1.7976931348623157e308      # (False for a NaN)
    for b in range(B):
        t = [None] * n

        def add(j, x):
            t[j] = x if t[j] is None else t[j] + x
        for r in range(R):
            row = [float(v) for v in table[b if table.shape[0] > 1 else 0, r]]
            a, bb = int(desc["joint_a"][r]), int(desc["joint_b"][r])
            if desc["kind"][r] == jt.LIMIT:
                lo, hi, k, c = row[:4]
                qa, qda = float(q[b, a]), float(qd[b, a])
                g_lo, g_hi = lo - qa, qa - hi
                f_lo, f_hi = k * g_lo - c * qda, k * g_hi + c * qda
                t_lo = f_lo if (g_lo > 0 and f_lo > 0) else 0.0
                t_hi = f_hi if (g_hi > 0 and f_hi > 0) else 0.0
                add(a, t_lo - t_hi)
                viol[b, r] = g_lo if g_lo > g_hi else g_hi
            elif desc["kind"][r] == jt.COUPLE:
                a0, a1, qa0, qb0, k, c = row[:6]
                e = (float(q[b, a]) - qa0) - (a0 + a1 * (float(q[b, bb]) - qb0))
                de = float(qd[b, a]) - a1 * float(qd[b, bb])
                f = k * e + c * de
                add(a, -f if fin(f) else 0.0)
                add(bb, a1 * f if fin(f) and fin(a1 * f) else 0.0)
                viol[b, r] = abs(e)
            else:
                gear, value = row[:2]
                if desc["source"][r] == jt.CONST:
                    cr = value
                else:
                    cr = float(ctrl[b, r])
                    if gf is not None and int(desc["dev"][r]) == active and float(gf[b]) != 0.0:
                        cr = float(gf[b])
                ctrl[b, r] = cr
                add(a, gear * cr if fin(cr) and fin(gear * cr) else 0.0)
        tau[b] = [0.0 if x is None else x for x in t]
    return tau, ctrl, viol


def straddling_states(rng, B, desc, table, n=25):
    """Random coordinates in which every LIMIT row has robots below, inside and above its range"""
    q, qd = rng.normal(0.0, 1.0, (B, n)), rng.normal(0.0, 2.0, (B, n))
    done = set()
    for r in np.flatnonzero(desc["kind"] == jt.LIMIT):      # (a hinge with two LIMIT rows: the first one's range)
        lo, hi, j = table[0, r, 0], table[0, r, 1], int(desc["joint_a"][r])
        if j not in done:
            q[:, j] = rng.uniform(lo - 0.4 * (hi - lo), hi + 0.4 * (hi - lo), B)
        done.add(j)
    return q, qd


@pytest.mark.parametrize("per_robot", [False, True])
def test_joint_torque_equals_the_plain_loop_bit_for_bit(per_robot):
    B = 200
    rng = np.random.default_rng(5)
    rows = jt.scene_rows(FIXTURE, 2.0, 0.3, 1.0, 0.05)
    rows += [dict(kind="drive", joint="left_outer_knuckle_joint_ur5left", gear=1.5, value=rng.normal(0.0, 0.1, B) if per_robot else 0.07),
             dict(kind="limit", joint="joint1_ur5right", lo=-1.0, hi=0.5, stiffness=50.0, damping=3.0)]      # a second row on a limited hinge
    if per_robot:
        rows[3]["stiffness"] = rng.uniform(1.0, 3.0, B)
        rows[25]["damping"] = rng.uniform(0.0, 0.1, B)
    desc, table = jt.normalise(rows, names(), DEVS, B)
    assert table.shape[0] == (B if per_robot else 1)
    q, qd = straddling_states(rng, B, desc, table)
    for r in np.flatnonzero(desc["kind"] == jt.LIMIT)[:24]:
        j = desc["joint_a"][r]
        assert (q[:, j] < table[0, r, 0]).sum() >= 20 and (q[:, j] > table[0, r, 1]).sum() >= 20
    ctrl0 = np.zeros((B, len(rows)))
    ctrl0[:, 34] = rng.normal(0.0, 0.05, B)      # a held ctrl of the right gripper's ACTION drive
    gf = np.where(rng.random(B) < 0.5, 0.0, rng.normal(0.0, 0.1, B))
    for kw in (dict(), dict(gripper_force=gf, active=0), dict(gripper_force=gf, active=1)):
        tau, ctrl, viol = jt.joint_torque(q, qd, desc, table, ctrl0, **kw)
        pt, pc, pv = plain_loop(q, qd, desc, table, ctrl0, kw.get("gripper_force"), kw.get("active"))
        assert tau.tobytes() == pt.tobytes() and ctrl.tobytes() == pc.tobytes() and viol.tobytes() == pv.tobytes()
        assert np.count_nonzero(tau) > 10 * B
    assert not ctrl0[:, :34].any()      # the input is left alone


def one_limit(q, qd, k=10.0, c=2.0, lo=-0.5, hi=0.25):
    desc, table = jt.normalise([dict(kind="limit", joint=1, lo=lo, hi=hi, stiffness=k, damping=c)], range(3), DEVS, 1)
    tau, _, viol = jt.joint_torque(np.array([[9.0, q, 9.0]]), np.array([[9.0, qd, 9.0]]), desc, table, np.zeros((1, 1)))
    assert tau[0, 0] == 0.0 and tau[0, 2] == 0.0
    return tau[0, 1], viol[0, 0]


def test_the_clamp_regimes_of_a_limit_on_both_sides():
    # outside and pushing back
    assert one_limit(-0.75, 0.0) == (10.0 * 0.25, 0.25)
    assert one_limit(-0.75, 0.5) == (10.0 * 0.25 - 2.0 * 0.5, 0.25)
    assert one_limit(0.5, 0.0) == (-(10.0 * 0.25), 0.25)
    assert one_limit(0.5, -0.5) == (-(10.0 * 0.25 + 2.0 * -0.5), 0.25)
    assert one_limit(0.5, 1.0)[0] == -(2.5 + 2.0)                    # still entering: the damper adds
    # outside but leaving so fast that f < 0: a stop never pulls
    assert one_limit(-0.75, 2.0) == (0.0, 0.25)
    assert one_limit(0.5, -2.0) == (0.0, 0.25)
    # inside: nothing, whatever the speed
    for qd in (0.0, 50.0, -50.0):
        t, v = one_limit(0.0, qd)
        assert t == 0.0 and v == -0.25
    assert one_limit(-0.5, -1.0)[0] == 0.0 and one_limit(0.25, 1.0)[0] == 0.0      # on the stop: g = 0 is no contact


def test_a_nan_coordinate_gives_zero_torque():
    rows = jt.scene_rows(FIXTURE, 2.0, 0.3, 1.0, 0.05, drive=None)
    desc, table = jt.normalise(rows, names(), DEVS, 4)
    q, qd = straddling_states(np.random.default_rng(1), 4, desc, table)
    q[1, :] = np.nan
    qd[2, :] = np.nan
    tau, _, viol = jt.joint_torque(q, qd, desc, table, np.zeros((4, 34)))
    assert np.all(np.isfinite(tau)) and not tau[1].any() and not tau[2].any() and tau[0].any()
    assert tau[3].any()
    assert np.isnan(viol[1]).all()


def test_an_infinite_coordinate_is_outside_its_stop():
    """q = +inf: g_hi = inf > 0, f_hi = inf > 0 -- the formula's answer is an infinite torque, which the plant answers by freezing the robot
    (IRLOSC_FLAG_NONFINITE); only NaN means 'no contact'."""
    t, v = one_limit(math.inf, 0.0)
    assert t == -math.inf and v == math.inf


def test_a_couple_gives_minus_f_and_a1_f():
    desc, table = jt.normalise([dict(kind="couple", joint=2, joint_b=0, a0=0.125, a1=-1.5, qa0=0.25, qb0=-0.5, stiffness=8.0, damping=0.5)],
                               range(3), DEVS, 1)
    assert list(table[0, 0]) == [0.125, -1.5, 0.25, -0.5, 8.0, 0.5, 0.0, 0.0]
    q, qd = np.array([[1.0, 7.0, 2.0]]), np.array([[0.5, 7.0, -1.0]])
    e = (2.0 - 0.25) - (0.125 + -1.5 * (1.0 + 0.5))
    de = -1.0 - -1.5 * 0.5
    f = 8.0 * e + 0.5 * de
    tau, _, viol = jt.joint_torque(q, qd, desc, table, np.zeros((1, 1)))
    assert tau[0, 2] == -f and tau[0, 0] == -1.5 * f and tau[0, 1] == 0.0 and viol[0, 0] == abs(e) and f != 0.0
    q[0, 0] = np.nan
    tau, _, _ = jt.joint_torque(q, qd, desc, table, np.zeros((1, 1)))
    assert not tau.any()


def test_the_hold_rule_of_an_action_drive():
    desc, table = jt.normalise([dict(kind="drive", joint=1, gear=2.0, source="action", dev="ur5left"),
                                dict(kind="drive", joint=2, gear=1.0, source="action", dev="ur5right")], range(3), DEVS, 1)
    q = np.zeros((1, 3))
    ctrl = np.zeros((1, 2))
    want = []
    for gf in (0.0, -0.08, 0.0, 0.05):
        tau, ctrl, _ = jt.joint_torque(q, q, desc, table, ctrl, gripper_force=np.array([gf]), active=1)
        want.append((ctrl[0, 0], tau[0, 1], ctrl[0, 1], tau[0, 2]))
    assert want == [(0.0, 0.0, 0.0, 0.0), (-0.08, -0.16, 0.0, 0.0), (-0.08, -0.16, 0.0, 0.0), (0.05, 0.1, 0.0, 0.0)]
    tau, c2, _ = jt.joint_torque(q, q, desc, table, ctrl)                   # no list: ctrl stays what it was, and keeps driving
    assert c2[0, 0] == 0.05 and tau[0, 1] == 0.1
    tau, c2, _ = jt.joint_torque(q, q, desc, table, ctrl, gripper_force=np.array([0.3]), active=0)      # the other arm's list
    assert c2[0, 0] == 0.05 and c2[0, 1] == 0.3 and tau[0, 2] == 0.3


REFUSED = [
    ([], "1 to 48"),
    ([dict(kind="limit", joint=0, lo=0.0, hi=1.0, stiffness=1.0)] * 49, "1 to 48"),
    ([dict(kind="spring", joint=0)], "unknown kind"),
    ([dict(kind=7, joint=0)], "unknown kind"),
    ([dict(kind="limit", joint=0, lo=0.0, hi=1.0, stiffness=1.0, colour=3)], "unknown keys"),
    ([dict(kind="limit", lo=0.0, hi=1.0, stiffness=1.0)], "joint= is missing"),
    ([dict(kind="limit", joint=3, lo=0.0, hi=1.0, stiffness=1.0)], "out of"),
    ([dict(kind="limit", joint=-1, lo=0.0, hi=1.0, stiffness=1.0)], "out of"),
    ([dict(kind="limit", joint="elbow", lo=0.0, hi=1.0, stiffness=1.0)], "is not one of"),
    ([dict(kind="limit", joint=0, lo=0.0, stiffness=1.0)], "hi= is missing"),
    ([dict(kind="limit", joint=0, lo=0.0, hi=1.0)], "stiffness= is missing"),
    ([dict(kind="limit", joint=0, lo=1.0, hi=1.0, stiffness=1.0)], "lo must be < hi"),
    ([dict(kind="limit", joint=0, lo=[0.0, 0.0, 0.0, 2.0], hi=1.0, stiffness=1.0)], "lo must be < hi"),
    ([dict(kind="limit", joint=0, lo=0.0, hi=1.0, stiffness=-1.0)], "must be >= 0"),
    ([dict(kind="limit", joint=0, lo=0.0, hi=1.0, stiffness=1.0, damping=-0.1)], "must be >= 0"),
    ([dict(kind="limit", joint=0, lo=0.0, hi=np.inf, stiffness=1.0)], "not finite"),
    ([dict(kind="limit", joint=0, lo=np.nan, hi=1.0, stiffness=1.0)], "not finite"),
    ([dict(kind="limit", joint=0, lo=0.0, hi=1.0, stiffness=[1.0, 2.0])], "expected a scalar or shape"),
    ([dict(kind="couple", joint=0, a1=1.0, stiffness=1.0)], "joint_b= is missing"),
    ([dict(kind="couple", joint=0, joint_b=1, stiffness=1.0)], "a1= is missing"),
    ([dict(kind="couple", joint=0, joint_b=0, a1=1.0, stiffness=1.0)], "with itself"),
    ([dict(kind="couple", joint=0, joint_b=5, a1=1.0, stiffness=1.0)], "out of"),
    ([dict(kind="couple", joint=0, joint_b=1, a1=1.0, stiffness=1.0, damping=-1.0)], "must be >= 0"),
    ([dict(kind="couple", joint=0, joint_b=1, a1=np.nan, stiffness=1.0)], "not finite"),
    ([dict(kind="drive", joint=0, source="pedal")], "unknown source"),
    ([dict(kind="drive", joint=0, source="action")], "names its device"),
    ([dict(kind="drive", joint=0, source="action", dev="ur5middle")], "is not one of"),
    ([dict(kind="drive", joint=0, source="action", dev=2)], "out of"),
    ([dict(kind="drive", joint=0, source="action", dev=0, value=1.0)], "takes no value"),
    ([dict(kind="drive", joint=0, source="const", dev=0)], "takes no dev"),
    ([dict(kind="drive", joint=0, value=np.inf)], "not finite"),
]


@pytest.mark.parametrize("rows,why", REFUSED, ids=[f"{i}-{w.replace(' ', '_')}" for i, (_, w) in enumerate(REFUSED)])
def test_normalise_refuses(rows, why):
    with pytest.raises(ValueError, match=why):
        jt.normalise(rows, range(3), DEVS, 4)


def test_normalise_refuses_an_empty_fleet_and_takes_per_robot_values():
    row = dict(kind="limit", joint=0, lo=0.0, hi=1.0, stiffness=1.0)
    with pytest.raises(ValueError, match="B=0"):
        jt.normalise([row], range(3), DEVS, 0)
    desc, table = jt.normalise([row, dict(kind="drive", joint="2", value=np.arange(4.0))], ["0", "1", "2"], DEVS, 4)
    assert desc["per_robot"] and table.shape == (4, 2, 8) and list(table[:, 1, 1]) == [0.0, 1.0, 2.0, 3.0] and np.all(table[:, 0, 1] == 1.0)
    assert list(desc["joint_a"]) == [0, 2]


def test_the_examples_penalties_lie_below_the_explicit_bound():
    """M_jj / dt^2 of the finger hinges from the rigid-body oracle (examples/gripper_fleet_resident_headless.py::stiffness_bound): the
    smallest is 16 N m / rad, and the stiffness the example puts on any one hinge -- its stop plus the couplings that name it, a1^2 k
    on the x side -- stays below it.  And the record the GPU test takes its coupling-error bound from
    (tests/golden/gripper_cpu_loop.json) is the example's cpu_loop with the example's penalties: the same parameters, and its first 16
    ticks repeated here reproduce the recorded knuckle angles and coupling errors (1e-12: the loop is deterministic NumPy; LAPACK builds
    may differ in the last bits) -- whoever changes cpu_loop or the penalties records it again."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gripper_fleet", os.path.join(ROOT, "examples", "gripper_fleet_resident_headless.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    bound = ex.stiffness_bound(verbose=False)
    fingers = {n: v for n, v in bound.items() if "knuckle" in n or "finger" in n}
    assert len(fingers) == 12 and abs(min(fingers.values()) - 16.0) < 0.5 and max(fingers.values()) < 250.0
    desc, table = jt.normalise(ex.scene_rows(), names(), DEVS, 1)
    total = {n: 0.0 for n in names()}
    for r in range(table.shape[1]):
        a, b = names()[desc["joint_a"][r]], names()[desc["joint_b"][r]]
        if desc["kind"][r] == jt.LIMIT:
            total[a] += table[0, r, 2]
        elif desc["kind"][r] == jt.COUPLE:
            total[a] += table[0, r, 4]
            total[b] += table[0, r, 1] ** 2 * table[0, r, 4]
    for n, v in fingers.items():
        assert 0.0 < total[n] < v / 3.0, (n, total[n], v)
    rec = ex.cpu_record()
    assert (rec["force"], rec["grip_ticks"], rec["limit_k"], rec["limit_c"], rec["couple_k"], rec["couple_c"]) == \
        (ex.FORCE, ex.GRIP_TICKS, ex.LIMIT_K, ex.LIMIT_C, ex.COUPLE_K, ex.COUPLE_C)
    assert rec["ticks"] == 600 and rec["finite"] and 0.0 < rec["couple_err_max"] < 0.2
    head = len(rec["head_knuckle"])
    out = ex.cpu_loop(robots=rec["robots"], ticks=head, seed=rec["seed"], verbose=False)
    assert np.all(np.isfinite(out["q"]))
    assert np.abs(out["knuckle"] - np.array(rec["head_knuckle"])).max() <= 1e-12
    assert np.abs(out["couple_err"] - np.array(rec["head_couple_err"])).max() <= 1e-12
    assert np.array(rec["head_couple_err"]).max() > 0.0 and rec["couple_err_max"] >= np.array(rec["head_couple_err"]).max()
