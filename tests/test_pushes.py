"""External pushes of a rollout (-m gpu): irlosc_set_pushes -- wrenches on EE bodies during windows of ticks, applied to the plant in
front of the plant kernel and taken off the sensor feed's wrench a tick later (csrc/osc_push.hpp) -- against the CPU oracles, against
runs without pushes, against itself tick by tick and in pieces, next to a program, the state rules, and the example.

The helpers are those of test_rollout.py / test_rollout_layouts.py / test_fromq_sensor_feed.py; the summed wrenches of a tick are
irl_control_amd/pushes.py's (held by tests/test_pushes_host.py)."""
import ctypes as C

import numpy as np
import pytest

import test_action_list as tal
import test_fromq_sensor_feed as tf
import test_rollout as tr
import test_rollout_layouts as trl
import test_waypoints as tw
from irl_control_amd import BatchedOSC, _lib, pushes as pu, synth
from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
from oracle import osc_oracle
from oracle import rigid_body as rb

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
EPS, NS, DT = tr.EPS, tr.NS, 1e-3
ERR_ARG, ERR_STATE = tr.ERR_ARG, tr.ERR_STATE
BAD = _lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD
B0 = 130                 # two full walk waves and a ragged one of two lanes
KEYS = ("qpos", "qvel", "u", "flags_any")


def wrenches(rng, B, P):
    """[B, P, 6]: forces N(0, 20 N), torques N(0, 2 N m) -- around the demo's 20 N."""
    return np.concatenate([rng.normal(0.0, 20.0, (B, P, 3)), rng.normal(0.0, 2.0, (B, P, 3))], axis=2)


def same(a, b, keys=KEYS, rows=slice(None)):
    for key in keys:
        assert np.array_equal(a[key][rows], b[key][rows]), key


# ---- 1. one tick against the CPU oracles ------------------------------------------------------------------------------------------------
B1 = 256
_REF1 = {}


def states1():
    if "q" not in _REF1:
        q, qd = RigidBodyModel.load("dual_ur5").random_state(np.random.default_rng(4242), B1)
        _REF1["q"] = (q, qd)
    return _REF1["q"]


def ee_jacobians(q, body_names):
    """oracle/rigid_body.py: body_jacobian of each named body at its frame origin, jacp rows then jacr rows -> {name: [B, 6, nj]}"""
    om = rb.Model()
    ids = {nm: om.body_id(nm) for nm in body_names}
    out = {nm: np.zeros((len(q), 6, om.nj)) for nm in body_names}
    for b in range(len(q)):
        kin = rb.kinematics(om, q[b])
        for nm, i in ids.items():
            jp, jr = rb.body_jacobian(om, kin, i)
            out[nm][b, :3], out[nm][b, 3:] = jp, jr
    return out


def jacobians1():
    if "J" not in _REF1:
        _REF1["J"] = ee_jacobians(states1()[0], sorted(set(DUAL_UR5_EE.values())))
    return _REF1["J"]


def plant_reference(M, bias, qpos, qvel, u, gen, dt=DT):
    """qacc = solve(M, u - bias + gen), semi-implicit Euler, and the bounds of test_rollout.test_one_tick_against_the_cpu_oracles
    (its formula, its C_BOUND) -> qv_ref, qp_ref, bv, bp, unit"""
    qacc = np.linalg.solve(M, (u.astype(np.float64) - bias + gen)[:, :, None])[:, :, 0]
    qv = qvel + dt * qacc
    qp = qpos + dt * qv
    unit = EPS * np.linalg.cond(M) * np.abs(qacc).max(axis=1)
    bv = dt * tr.C_BOUND * unit + 4 * EPS * np.abs(qv).max(axis=1)
    bp = dt * bv + 4 * EPS * np.abs(qp).max(axis=1)
    return qv, qp, bv, bp, unit


@pytest.mark.parametrize("name", ["k13", "br7"])
def test_one_tick_with_pushes_against_the_cpu_oracles(name, monkeypatch):
    """256 random states (those of test_one_tick_against_the_cpu_oracles), one push per device active on tick 0, apply only, a wrench per
    robot.  Reference: M, bias from oracle/rigid_body.py, J_d = body_jacobian of the device's EE body at its frame origin, u what the
    rollout returns, qacc_ref = solve(M, u - bias + sum_d J_d^T W_d), Euler in NumPy; the bound is that test's formula with its C_BOUND
    (the push adds one term to a right-hand side whose entries already carry the same rounding allowance).  And the push acts: every
    robot's qvel is further from the same tick without pushes than its bound.  br7: the base is device 0 and the arm device 1 -- a
    device-to-body mix-up lands on the wrong hinges.
    Measured on an MI355X (printed; profiles/push_rates.md): worst qvel error / (dt eps cond max|qacc|) 0.208 (k13) and 0.0198 (br7) of
    the 64 allowed; every robot's qvel moved by at least 1.7e5 x its bound."""
    B = B1
    if name == "k13":
        lay, gains, g, model, osc = tr.make_ctx("k13", B, F64, seed=21, n_slots=2)
        assert "fused" in osc.from_q_name
    else:
        lay, gains, g, model, osc = trl.open_ctx(name, B, F64, monkeypatch, seed=21, n_slots=2)
    qpos, qvel = states1()
    osc.set_plant(DT, 0.0)
    for slot in (0, 1):
        osc.upload_q(qpos, qvel, slot=slot)
        trl.set_targets(osc, g, slot)
    P = lay.ndev
    W = wrenches(np.random.default_rng(11), B, P)
    osc.set_pushes([dict(dev=d, window=(0, 1), apply=True, sense=False) for d in range(P)], W, slot=0)
    out = osc.rollout(1, slot=0)
    plain = osc.rollout(1, slot=1)
    osc.close()
    assert np.array_equal(out["u"], plain["u"]) and np.array_equal(out["flags_any"], plain["flags_any"])      # an applied push is not sensed
    assert not np.any(out["flags_any"] & BAD)
    M, bias = tr.oracle_M_bias(qpos, qvel)
    J = jacobians1()
    gen = sum(np.einsum("bci,bc->bi", J[DUAL_UR5_EE[nm]], W[:, d]) for d, nm in enumerate(lay.dev_names))
    qv_ref, qp_ref, bv, bp, unit = plant_reference(M, bias, qpos, qvel, out["u"], gen)
    ev = np.abs(out["qvel"] - qv_ref).max(axis=1)
    ep = np.abs(out["qpos"] - qp_ref).max(axis=1)
    moved = np.abs(out["qvel"] - plain["qvel"]).max(axis=1)
    print(f"[one tick with pushes {name}] worst qvel error / (dt eps cond max|qacc|) = {(ev / (DT * unit)).max():.3g} (bound {tr.C_BOUND:g}); "
          f"max |dqvel| {ev.max():.3g}, max |dqpos| {ep.max():.3g}; |qvel - qvel without pushes| / bound: min {(moved / bv).min():.3g}")
    assert np.all(ev <= bv), (float((ev / bv).max()), int(np.argmax(ev / bv)))
    assert np.all(ep <= bp), (float((ep / bp).max()), int(np.argmax(ep / bp)))
    assert np.all(moved > bv), int(np.argmin(moved / bv))


# ---- 2. / 3. / 5. untouched ticks and robots; T ticks = T single ticks = pieces; on every layout and both forms ------------------------------
# case: (route of test_rollout_layouts.ROUTES or None, layout, dtype, devices of the pushes, torque only?)
CASES = {
    "k12_admit": (None, "k12_admit", F64, (1, 1), False),
    "br7": ("br7", "br7", F64, (0, 1), False),                        # the base is device 0: device index and EE body differ
    "rlbr10": ("rlbr10", "rlbr10", F64, (0, 3), False),               # blocks 0 and 3 of the right arm share one EE body: they sum
    "k7": ("k7", "k7", F64, (1, 1), True),                            # xyz rows only; a torque still acts: the block's J has six rows
    "rlb16": ("rlb16", "rlb16", F64, (1, 1), False),                  # row16 FROMQ form
    "rlb11_branch_b": ("rlb11_branch_b", "rlb11_branch_b", F64, (2, 2), False),      # target velocities
    "k13_lane0": ("k13_lane0", "k13", F64, (0, 0), False),
    "k12_admit_f32": (None, "k12_admit", F32, (1, 1), False),
    "rlb16_f32": ("rlb16", "rlb16", F32, (0, 0), False),
}


def open_case(case, B, monkeypatch, **kw):
    """A context with the F/T sensors described on the case's layout, the route asserted -> lay, gains, g, model, osc, devs, torque_only"""
    route, cfg, dtype, devs, torque_only = CASES[case]
    if route is not None:
        ctx = trl.open_ctx(route, B, dtype, monkeypatch, feed=True, **kw)
    else:      # k12 + admittance: the (1, 6, 6) tier on its own kernel instantiation
        ctx = tr.make_ctx(cfg, B, dtype, feed=True, **kw)
        osc = ctx[4]
        assert "fused" in osc.from_q_name and "row16" in osc.kernel_name and "_pad" not in osc.kernel_name
        if dtype is F64:
            assert "_rows_1_6_6 " in osc.from_q_name, osc.from_q_name
    return ctx + (devs, torque_only)


def start(osc, model, g, B, slots, damping=0.05):
    qpos, qvel = model.random_state(np.random.default_rng(77), B)
    sens = np.random.default_rng(43).normal(0.0, 5.0, size=(B, NS))
    osc.set_plant(DT, damping)
    for slot in slots:
        osc.upload_q(qpos, qvel, slot=slot)
        trl.set_targets(osc, g, slot)
        osc.set_sensordata(sens, slot=slot)
    return qpos, qvel, sens


def case_wrenches(B, P, torque_only, per_robot=True, seed=12):
    W = wrenches(np.random.default_rng(seed), B if per_robot else 1, P)
    if torque_only:
        W[:, :, :3] = 0.0
    return W if per_robot else W[0]


@pytest.mark.parametrize("case", list(CASES))
def test_untouched_ticks_and_robots_are_bit_identical(case, monkeypatch):
    """Applied-and-sensed pushes with the window [5, 9) on slot 0, none on slot 1, a sensor feed on both.  rollout(5): qpos, qvel, u,
    flags_any and the full EE trace are those of the slot without pushes, bit for bit.  rollout(3) more: the sample at the start of tick
    5 is still identical, the coordinates afterwards differ.  The table is per robot with zero wrenches for robots 64 .. 129: those
    stay bit-identical throughout -- a robot does not see its wave mates' pushes."""
    B = B0
    lay, gains, g, model, osc, devs, torque_only = open_case(case, B, monkeypatch, seed=5, n_slots=2)
    start(osc, model, g, B, (0, 1))
    ds = sorted(set(devs))
    W = case_wrenches(B, len(ds), torque_only)
    W[64:] = 0.0
    osc.set_pushes([dict(dev=d, window=(5, 9)) for d in ds], W, slot=0)
    a, b = osc.rollout(5, trace_every=1, slot=0), osc.rollout(5, trace_every=1, slot=1)
    a2, b2 = osc.rollout(3, trace_every=1, slot=0), osc.rollout(3, trace_every=1, slot=1)
    osc.close()
    same(a, b, KEYS + ("ee_trace",))
    assert not np.any(a2["flags_any"] & BAD) and np.all(np.isfinite(a2["qpos"]))
    assert np.array_equal(a2["ee_trace"][0], b2["ee_trace"][0])
    for key in ("qpos", "qvel"):
        assert np.all(np.abs(a2[key][:64] - b2[key][:64]).max(axis=1) > 0.0), key
    same(a2, b2, KEYS, rows=slice(64, None))
    assert np.array_equal(a2["ee_trace"][:, 64:], b2["ee_trace"][:, 64:])


@pytest.mark.parametrize("per_robot", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_T_ticks_equal_T_single_ticks_equal_pieces(case, per_robot, monkeypatch):
    """rollout(8) on slot 0, 8 x rollout(1) on slot 1, rollout(3) + rollout(5) on slot 2, the same two applied-and-sensed pushes on each:
    windows [2, 4) and [3, 7) on one EE body, so they overlap and straddle the call boundary -- qpos, qvel, u and the OR of the flags
    bit for bit, with a shared table and with one per robot.  This holds "the tick continues across calls"."""
    B, T = B0, 8
    lay, gains, g, model, osc, devs, torque_only = open_case(case, B, monkeypatch, seed=5, n_slots=3)
    qpos, qvel, _ = start(osc, model, g, B, (0, 1, 2))
    W = case_wrenches(B, 2, torque_only, per_robot)
    ps = [dict(dev=devs[0], window=(2, 4)), dict(dev=devs[1], window=(3, 7))]
    for slot in (0, 1, 2):
        osc.set_pushes(ps, W, slot=slot)
    a = osc.rollout(T, slot=0)
    fl = np.zeros(B, np.uint32)
    for _ in range(T):
        b = osc.rollout(1, slot=1)
        fl |= b["flags_any"]
    c3 = osc.rollout(3, slot=2)
    c = osc.rollout(5, slot=2)
    osc.clear_pushes(slot=1)
    osc.upload_q(qpos, qvel, slot=1)
    plain = osc.rollout(T, slot=1)
    osc.close()
    assert np.all(np.isfinite(a["qpos"])) and np.all(np.isfinite(a["u"])) and not np.any(a["flags_any"] & BAD)
    trl.assert_branch_b(case, a["flags_any"])
    same(a, b, ("qpos", "qvel", "u"))
    same(a, c, ("qpos", "qvel", "u"))
    assert np.array_equal(a["flags_any"], fl)
    assert np.array_equal(a["flags_any"], c3["flags_any"] | c["flags_any"])
    assert np.all(np.abs(a["qvel"] - plain["qvel"]).max(axis=1) > 0.0)      # the pushes acted, on every robot


# ---- 4. timing and sign of both halves, tick by tick, against the oracles ----------------------------------------------------------------
def test_timing_and_sign_tick_by_tick_against_the_oracles():
    """k12_admit, float64, a random sensor feed, one applied-and-sensed push on the left arm with the window [2, 4); six single ticks,
    download_q in front of each.  Per tick t: u against oracle/osc_oracle.py on the downloaded state, the oracle's wrench being the feed
    rotated by the site frame of the oracle's own pose minus W^sense(t - 1), at the project's 1e-5 (robots outside the parity domain
    left out as test_fromq_sensor_feed.py leaves them out); the coordinates afterwards against the plant reference of test 1 with
    W^apply(t).  Then the wrong schedules, each on the ticks where it differs from the right one: sensed on tick t instead of t - 1,
    applied a tick late, the sign flipped, force and torque triples swapped -- each must fail the same comparison on at least one robot.
    The magnitude (forces N(0, 20 N), torques N(0, 2 N m) per robot: the demo's 20 N) was chosen on the CPU before any GPU run, from the
    oracles on this test's start states: replacing the push by nothing, by its negative or by its swapped triples moves the oracle's u
    by at least 1.46e3 x the 1e-5 tolerance on every robot (median 2.1e4 x) and the plant reference's qvel by at least 2.55e5 x its
    bound (median 4e6 x); a hundredth of it would still discriminate (14 x and 2.56e3 x).  (profiles/push_rates.md has the figures per
    replacement.)"""
    B, T = B0, 6
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5)
    _, _, sens = start(osc, model, g, B, (0,), damping=0.0)
    Wp = wrenches(np.random.default_rng(9), B, 1)
    ps = [dict(dev="ur5left", window=(2, 4), apply=True, sense=True)]
    osc.set_pushes(ps, Wp)
    ticks = []
    for t in range(T):
        q, qd = osc.download_q()
        ticks.append((q, qd, osc.rollout(1, trace_every=1)))
    osc.close()
    fd = model.ft_desc(lay.dev_names)
    left = DUAL_UR5_EE["ur5left"]
    swap = [3, 4, 5, 0, 1, 2]
    tried = dict(sensed_now=0, applied_late=0, flipped_sense=0, flipped_apply=0, swapped_sense=0, swapped_apply=0)
    for t, (q, qd, out) in enumerate(ticks):
        R, Wfeed = tf.oracle_records_and_wrench(lay, fd, q, qd, sens)
        dom = np.array([tf.in_parity_domain(*osc_oracle.task_inertia(R["J"][b], R["M"][b])[2:]) for b in range(B)])
        assert dom.mean() > 0.9
        J = ee_jacobians(q, [left])[left]

        def u_err(Ws):
            Wx = Wfeed.copy()
            Wx[:, 1] -= Ws
            ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], g["tgt_pose"], Wx)
            return tf.rel_err(out["u"], ref)[dom]

        def x_ok(Wa):
            qv, qp, bv, bp, _ = plant_reference(R["M"], R["bias"], q, qd, out["u"], np.einsum("bci,bc->bi", J, Wa))
            return (np.abs(out["qvel"] - qv).max(axis=1) <= bv) & (np.abs(out["qpos"] - qp).max(axis=1) <= bp)

        S = pu.summed_wrenches(ps, Wp, lay.dev_names, t)
        Ws, Wa = S["sense"][:, 1], S["apply"][:, 1]
        assert S["sense_some"][1] == (t in (3, 4)) and S["apply_some"][1] == (t in (2, 3))
        e = u_err(Ws)
        ok = x_ok(Wa)
        print(f"[tick {t}] sensed {bool(S['sense_some'][1])}, applied {bool(S['apply_some'][1])}: u against the oracle {e.max():.3g}; "
              f"robots within the plant bound {int(ok.sum())}/{B}")
        assert e.max() <= tf.TOL64, (t, float(e.max()))
        assert ok.all(), (t, int(np.argmin(ok)))
        assert not np.any(out["flags_any"] & BAD)
        Wnow = pu.summed_wrenches(ps, Wp, lay.dev_names, t + 1)["sense"][:, 1]       # W^sense(t) in place of W^sense(t - 1)
        Wlate = pu.summed_wrenches(ps, Wp, lay.dev_names, t - 1)["apply"][:, 1] if t else np.zeros_like(Wa)
        if not np.array_equal(Wnow, Ws):
            tried["sensed_now"] += 1
            assert u_err(Wnow).max() > tf.TOL64, t
        if not np.array_equal(Wlate, Wa):
            tried["applied_late"] += 1
            assert not x_ok(Wlate).all(), t
        if Ws.any():
            tried["flipped_sense"] += 1
            tried["swapped_sense"] += 1
            assert u_err(-Ws).max() > tf.TOL64 and u_err(Ws[:, swap]).max() > tf.TOL64, t
        if Wa.any():
            tried["flipped_apply"] += 1
            tried["swapped_apply"] += 1
            assert not x_ok(-Wa).all() and not x_ok(Wa[:, swap]).all(), t
    assert all(n == 2 for n in tried.values()), tried


# ---- 6. with a program -------------------------------------------------------------------------------------------------------------------
def test_pushes_next_to_waypoint_paths():
    """k13 with paths on both arms: a run whose window has not opened yet has the waypoint state (and everything else) of the run
    without pushes; with the window open the run completes with clean flags, and neither setter ended the other's state."""
    B, T = B0, 8
    sc = tw.scenario(B, False)
    osc = tw.make_ctx(B, n_slots=3)
    W = wrenches(np.random.default_rng(13), B, 1)
    for slot, window in ((0, None), (1, (20, 30)), (2, (0, T))):
        tw.fill(osc, sc, slot)
        osc.set_waypoints(sc["paths"] + [None], tw.THRESHOLD, True, slot=slot)
        if window:
            osc.set_pushes([dict(dev="ur5left", window=window)], W, slot=slot)
    outs = [osc.rollout(T, slot=slot) for slot in range(3)]
    sts = [osc.waypoint_state(slot) for slot in range(3)]
    osc.close()
    same(outs[0], outs[1])
    for key in ("index", "arrivals", "last_tick"):
        assert np.array_equal(sts[0][key], sts[1][key]), key
    assert not np.any(outs[2]["flags_any"] & BAD) and np.all(np.isfinite(outs[2]["qpos"]))
    assert np.all(np.abs(outs[2]["qvel"] - outs[0]["qvel"]).max(axis=1) > 0.0)
    assert sts[2]["arrivals"][:, :2].min() >= 1      # (waypoint 0 is where the arms start: the cycler ran on the pushed slot too)


def test_pushes_next_to_an_action_list():
    """k12_admit with a sensor feed, the WP / GRIP list on the right arm and an applied-and-sensed push on it: rollout(8) = 8 x
    rollout(1), bit for bit, action state included -- the order wrench kernel, sense, action kernel."""
    B, T = B0, 8
    sc = tal.scenario(B, cfg="k12_admit")
    osc = tal.make_ctx(B, n_slots=3, cfg="k12_admit", feed=True)
    sens = np.random.default_rng(43).normal(0.0, 5.0, size=(B, NS))
    W = wrenches(np.random.default_rng(14), B, 1)
    for slot in (0, 1, 2):
        tal.fill(osc, sc, slot)
        osc.set_sensordata(sens, slot=slot)
        osc.set_action_list(sc["desc"], slot=slot)
        if slot < 2:
            osc.set_pushes([dict(dev=sc["desc"]["active_dev"], window=(1, 5))], W, slot=slot)
    a = osc.rollout(T, slot=0)
    fl = np.zeros(B, np.uint32)
    for _ in range(T):
        b = osc.rollout(1, slot=1)
        fl |= b["flags_any"]
    plain = osc.rollout(T, slot=2)
    sa, sb = osc.action_state(0), osc.action_state(1)
    osc.close()
    same(a, b, ("qpos", "qvel", "u"))
    assert np.array_equal(a["flags_any"], fl) and not np.any(fl & BAD)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert np.all(np.abs(a["qvel"] - plain["qvel"]).max(axis=1) > 0.0)


# ---- 7. state rules ------------------------------------------------------------------------------------------------------------------------
def make_desc(devs=(1, 1), windows=((2, 4), (3, 7)), apply=(1, 1), sense=(1, 1), nb=1, P=None):
    d = _lib.Pushes()
    d.n_pushes, d.nb = len(devs) if P is None else P, nb
    for p in range(len(devs)):
        d.dev[p], (d.tick0[p], d.tick1[p]), d.apply[p], d.sense[p] = devs[p], windows[p], apply[p], sense[p]
    return d


def rc_set(osc, B, desc, w, slot=0):
    return osc.lib.irlosc_set_pushes(osc._h, slot, B, None if desc is None else C.byref(desc), _lib.ptr(w))


def test_state_rules():
    B = B0
    lay = synth.make_layout("k12_admit")
    _, gains, g = synth.make_batch("k12_admit", B, seed=5)
    model = RigidBodyModel.load("dual_ur5")
    W1 = np.ascontiguousarray(wrenches(np.random.default_rng(15), 1, 2))
    WB = np.ascontiguousarray(wrenches(np.random.default_rng(16), B, 2))
    good = make_desc()
    bare = BatchedOSC(lay, B, dtype=F64)
    bare.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    assert rc_set(bare, B, good, W1) == ERR_STATE                                  # before set_model
    assert "irlosc_set_model" in bare.lib.irlosc_last_error(bare._h).decode()
    assert rc_set(bare, B, None, None) == 0                                        # clearing nothing is no error
    bare.close()

    _, _, _, _, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    _, _, _, _, twin = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    qpos, qvel, sens = start(osc, model, g, B, (0, 1))
    start(twin, model, g, B, (0, 1))

    def reset(o, slots=(0, 1)):
        for slot in slots:
            o.upload_q(qpos, qvel, slot=slot)

    # every refused call leaves the pushes in force, whole, their tick included: the twin never sees one.  The windows stay open through
    # the whole loop and tick 0 runs ahead of it, so every refusal is followed by a tick that both applies and senses
    held = make_desc(windows=((0, 64), (1, 64)))
    assert rc_set(osc, B, held, W1) == 0 and rc_set(twin, B, held, W1) == 0
    same(osc.rollout(1), twin.rollout(1))
    nan, inf = W1.copy(), WB.copy()
    nan[0, 1, 4] = np.nan
    inf[B - 1, 0, 0] = np.inf
    refused = [
        (B, make_desc(devs=(), windows=(), apply=(), sense=(), P=0), W1), (B, make_desc(P=9), W1),      # P outside [1, 8]
        (B, make_desc(devs=(1, 2)), W1), (B, make_desc(devs=(-1, 1)), W1),                              # dev outside [0, ndev)
        (B, make_desc(windows=((2, 2), (3, 7))), W1), (B, make_desc(windows=((-1, 4), (3, 7))), W1),
        (B, make_desc(windows=((2, 4), (7, 3))), W1),                                                   # not 0 <= tick0 < tick1
        (B, make_desc(apply=(2, 1)), W1), (B, make_desc(sense=(1, 3)), W1), (B, make_desc(apply=(1, 0), sense=(1, 0)), W1),
        (B, make_desc(nb=2), W1), (B, make_desc(nb=B - 1), WB), (0, good, W1),                          # nb not 1 or B; B < 1
        (B, good, None), (B, good, nan), (B, make_desc(nb=B), inf),                                     # wrench NULL or not finite
    ]
    for i, (b_, desc, w) in enumerate(refused):
        assert rc_set(osc, b_, desc, w) == ERR_ARG, i
        assert "pushes" in osc.lib.irlosc_last_error(osc._h).decode(), i
        same(osc.rollout(1), twin.rollout(1))
    assert len(refused) + 1 < 64
    plain = twin.rollout(len(refused) + 1, slot=1)
    assert np.abs(osc.download_q()[1] - plain["qvel"]).max() > 0.0                 # (and they were in force)
    assert rc_set(osc, B + 1, good, W1) == ERR_ARG                                 # (check_slot)

    # a rollout over more robots than the pushes cover
    reset(osc)
    assert rc_set(osc, 64, make_desc(nb=64), WB[:64].copy()) == 0
    assert tr._rc_rollout(osc, B) == ERR_STATE and "pushes" in osc.lib.irlosc_last_error(osc._h).decode()
    assert tr._rc_rollout(osc, 64) == 0

    # desc == NULL and set_model clear them
    T = 6
    reset(twin)
    plain = twin.rollout(T, slot=1)
    reset(osc)
    osc.set_pushes([dict(dev=1, window=(0, T))], WB[:, :1])
    osc.clear_pushes()
    same(osc.rollout(T), plain)
    osc.set_pushes([dict(dev=1, window=(0, T))], WB[:, :1])
    osc.set_model(model)
    osc.set_ft_sensors()
    start(osc, model, g, B, (0, 1))
    same(osc.rollout(T), plain)

    # set_targets, set_gains, upload_q and set_sensordata leave them and their tick alone; so does step_q between rollouts
    reset(osc)
    reset(twin)
    for o in (osc, twin):
        assert rc_set(o, B, good, W1) == 0
    osc.rollout(2)
    twin.rollout(2)
    trl.set_targets(osc, g, 0)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload_q(*osc.download_q())
    osc.set_sensordata(sens)
    osc.step_q()
    a, b = osc.rollout(2), twin.rollout(2)
    same(a, b)
    osc.step_q()
    same(osc.rollout(4), twin.rollout(4))
    reset(twin)
    assert np.abs(twin.rollout(8, slot=1)["qvel"] - osc.download_q()[1]).max() > 0.0

    # set_waypoints with real paths leaves them and their tick alone: osc sets its pushes (windows [2, 4) and [3, 7)), runs two ticks
    # and is given paths; the twin runs the two ticks without pushes (none is active on them), is given the same paths and only then
    # the same pushes with their windows two ticks earlier.  Equal from there on only if osc's pushes and their tick survived the call
    reset(osc)
    reset(twin)
    twin.clear_pushes()
    assert rc_set(osc, B, good, W1) == 0
    same(osc.rollout(2), twin.rollout(2))
    paths = [np.array([[0.3, 0.45, 0.5], [0.32, 0.45, 0.5]]), None]
    osc.set_waypoints(paths, 0.01)
    twin.set_waypoints(paths, 0.01)
    assert rc_set(twin, B, make_desc(windows=((0, 2), (1, 5))), W1) == 0
    a, b = osc.rollout(6), twin.rollout(6)
    same(a, b)
    for key, v in osc.waypoint_state().items():
        assert np.array_equal(v, twin.waypoint_state()[key]), key
    twin.upload_q(qpos, qvel, slot=1)                                                # (the same schedule without pushes)
    twin.rollout(2, slot=1)
    twin.set_waypoints(paths, 0.01, slot=1)
    assert np.abs(twin.rollout(6, slot=1)["qvel"] - a["qvel"]).max() > 0.0          # (and they acted behind the call)
    for o in (osc, twin):
        for slot in (0, 1):
            trl.set_targets(o, g, slot)                                              # (the paths end, the targets are the start's again)

    # two slots with different pushes, interleaved
    reset(osc)
    reset(twin)
    other = make_desc(devs=(0,), windows=((1, 5),), apply=(1,), sense=(0,), nb=B)
    WO = np.ascontiguousarray(WB[:, :1])
    assert rc_set(osc, B, good, W1, slot=0) == 0 and rc_set(osc, B, other, WO, slot=1) == 0
    assert rc_set(twin, B, good, W1, slot=0) == 0 and rc_set(twin, B, other, WO, slot=1) == 0
    for _ in range(T):
        a0 = osc.rollout(1, slot=0)
        a1 = osc.rollout(1, slot=1)
    same(a0, twin.rollout(T, slot=0), ("qpos", "qvel", "u"))
    same(a1, twin.rollout(T, slot=1), ("qpos", "qvel", "u"))
    assert np.abs(a0["qvel"] - a1["qvel"]).max() > 0.0
    osc.close()
    twin.close()


# ---- 8. the example ------------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_and_the_push_displaces_the_left_arm():
    """examples/admit_test_resident_headless.py, 130 robots, 64 ticks (the window: ticks [24, 39)): finite, no robot frozen; the EE
    trace before the window is bit-identical to the same run with the push cleared; at the end of the window every robot's left EE is
    displaced -- from where it was before the window, and from where the run without the push has it.  No recovery distance is
    asserted: nobody has measured how this plant settles."""
    mod = tr._example("admit_test_resident_headless")
    r = mod.run(robots=B0, ticks=64, seed=0, trace_before=True, verbose=False)
    r0 = mod.run(robots=B0, ticks=64, seed=0, push=False, trace_before=True, verbose=False)
    assert r["window"] == (24, 39) and r["trace_before"].shape == (24, B0, 2, 7)
    for x in (r, r0):
        assert np.all(np.isfinite(x["q"])) and np.all(np.isfinite(x["qd"])) and np.all(np.isfinite(x["ee_end"]))
        assert not np.any(x["flags_any"] & BAD)
    assert np.array_equal(r["trace_before"], r0["trace_before"]) and np.array_equal(r["ee_before"], r0["ee_before"])
    assert np.all(np.linalg.norm(r["ee_window_end"][:, 1, :3] - r["ee_before"][:, 1, :3], axis=1) > 0.0)
    assert np.all(np.linalg.norm(r["ee_window_end"][:, 1, :3] - r0["ee_window_end"][:, 1, :3], axis=1) > 0.0)
