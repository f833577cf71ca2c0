"""The episode log off k13 and in wide contexts (-m gpu): what tests/test_rollout_log.py holds on k13 (three devices in the order right,
left, base, lane form, max_batch == B), here with everything the log kernel takes as a runtime argument at another value -- ndev, ee0[d],
n_entries, stride, the widths, the LDS tile size and which OSC kernel filled u and flags:

    r6               one device: widths 7 / 6 / 3, nvalid w no multiple of the unroll      lane form, tier (1, 6, 6)
    k12_admit, _f32  two devices with a feed; the float32 records are widened              lane form on the layout's own kernel
    br7              the base is device 0: device index and EE body differ                 lane form, tier (1, 6, 6)
    rlbr10           four devices: ee_pose / targets 28 words wide, more than n = 25;      lane form, tier (1, 6, 6)
                     one EE body behind devices 0 and 3
    rlb16            no lane tier                                                          row16 FROMQ form, KMAX 16
    rlb11_branch_b   target velocities                                                     row16 FROMQ form by the branch-B rule
    k13_lane0        IRLOSC_LANE=0 on the layout the other tests know                      row16 FROMQ form
    k13_wide, _f32   max_batch = 192, everything set and run over B = 130                  lane form; stride = 192
    k13              the layout of test_rollout_log.py, for the parts that file leaves open (wrench, pieces, an action list)

Every case asserts its route from from_q_name / kernel_name (open_rig).  B = 130 (three waves, the last ragged), B = 65 where a CPU oracle
runs per robot, T = 7.  Every slot is armed with all its layout allows (arm): a sensor feed, median walls on the devices test_walls.CASES
names for the layout (a layout it does not name: every arm), test_joints.scene(lay), and waypoint paths with the far threshold of
test_rollout_log.FAR on the layout's arm devices.  Every layout here has an arm and so a feed; what a slot WITHOUT a feed is refused
(the wrench channel, IRLOSC_ERR_STATE) is asserted on a second slot of test 2's contexts.  The reference run asserts its own inputs as
test_rollout_log.chopped does: no robot froze, some robot touched a wall, joint_tau is not all zero, the targets change every tick.

Unless a tolerance is named every comparison is == on bits.  Robots that give up inside a rollout are left out: the module docstring of
tests/test_rollout_layouts.py documents that no such configuration of this model exists.

1. logged = the one-tick loop, per case;  2. tick 0 against references that share no kernel with the log;  3. the wrench against the
oracle;  4. wide = tight;  5. subsets;  6. a two-sample ring;  7. pieces;  8. an action list under the log;  9. a NaN robot on the FROMQ
form.  Measured worst errors of 2 and 3 (printed): profiles/rollout_log_rates.md."""
import hashlib

import numpy as np
import pytest

import test_action_list as tal
import test_action_list_layouts as tall
import test_fromq_sensor_feed as tf
import test_joints as tjn
import test_pushes as tp
import test_rollout as tr
import test_rollout_layouts as trl
import test_rollout_log as tlg
import test_teleop_stream as tts
import test_walls as twl
import test_waypoints as tw
from irl_control_amd import _lib, rollout_log, synth, walls as wl

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
ERR_ARG, ERR_STATE = tr.ERR_ARG, tr.ERR_STATE
BAD = tp.BAD
T = tlg.T
ALL = rollout_log.ALL
FAR = tlg.FAR
WIDE = 192
same_bits, assert_log_is, rc_logged = tlg.same_bits, tlg.assert_log_is, tlg.rc_logged
LOGGED = ("qpos", "qvel", "targets", "u", "flags", "ee_pose", "wall_force", "joint_tau")      # (every channel but the wrench)

# case: route (a key of test_rollout_layouts.ROUTES, else the layout's own lane kernel), layout, dtype, capacity (None: B)
CASES = {
    "r6": dict(route="r6", cfg="r6", dtype=F64),
    "k12_admit": dict(route=None, cfg="k12_admit", dtype=F64),
    "k12_admit_f32": dict(route=None, cfg="k12_admit", dtype=F32),
    "br7": dict(route="br7", cfg="br7", dtype=F64),
    "rlbr10": dict(route="rlbr10", cfg="rlbr10", dtype=F64),
    "rlb16": dict(route="rlb16", cfg="rlb16", dtype=F64),
    "rlb11_branch_b": dict(route="rlb11_branch_b", cfg="rlb11_branch_b", dtype=F64),
    "k13_lane0": dict(route="k13_lane0", cfg="k13", dtype=F64),
    "k13_wide": dict(route=None, cfg="k13", dtype=F64, max_batch=WIDE),
    "k13_wide_f32": dict(route=None, cfg="k13", dtype=F32, max_batch=WIDE),
    "k13": dict(route=None, cfg="k13", dtype=F64),
}
ISSUE_CASES = [c for c in CASES if c != "k13"]
F64_CASES = [c for c in CASES if CASES[c]["dtype"] is F64]


def wall_devices(case):
    """The devices test_walls.CASES names for the case's layout on its route (rlbr10: blocks 0 and 3, of rlbr10 and rlbr10_both); k13 in
    lane form: both arms, as test_rollout_log.arm; a layout that file does not name: every arm."""
    c = CASES[case]
    named = sorted({d for route, cfg, _, devs, _ in twl.CASES.values() if cfg == c["cfg"] and route == c["route"] for d in devs})
    return tuple(named) if named else tuple(d for d, nm in enumerate(synth.make_layout(c["cfg"]).dev_names) if nm != "base")


def assert_own_route(cfg, dtype, fq, kn):
    """k13, k12_admit: the (1, 6, 6) lane tier on the layout's own kernel instantiation (test_action_list_layouts.assert_route); float32
    records: test_pushes.open_case's wording, and where the lane form is reported, that tier."""
    if dtype is F64:
        tall.assert_route(cfg, fq, kn)
    else:
        assert "fused" in fq and "row16" in kn and "_pad" not in kn and ("osc_lane" not in fq or "_rows_1_6_6 " in fq), (fq, kn)


def open_rig(case, B, monkeypatch, n_slots=1, tight=False):
    """A context of the case for B robots (capacity: the case's, or B with `tight`) with the F/T sensors described and the plant of
    test_waypoints.make_ctx, the route asserted.  -> lay, model, osc"""
    c = CASES[case]
    cap = B if tight or not c.get("max_batch") else c["max_batch"]
    if c["route"] is not None:
        lay, _, _, model, osc = trl.open_ctx(c["route"], cap, c["dtype"], monkeypatch, feed=True, n_slots=n_slots)
    else:
        lay, _, _, model, osc = tr.make_ctx(c["cfg"], cap, c["dtype"], feed=True, n_slots=n_slots)
        assert_own_route(c["cfg"], c["dtype"], osc.from_q_name, osc.kernel_name)
    assert osc.max_batch == cap
    osc.set_plant(tw.DT, tw.DAMPING)
    return lay, model, osc


_IN = {}


def inputs(case, B):
    """What a slot of the case is armed with, computed once per (case, B): the start state, targets and paths of test_waypoints.scenario
    on the layout with every arm device listed, target velocities where the layout has them (0.1 x synth.make_batch's, as
    test_action_list_layouts), the feed of test_rollout_log.arm, walls on wall_devices(case) -- per device the planes y = and x = the median
    of the fleet's EE y and x at the start, radius 1 cm: two normals, so that two of a device's three force words are in use (with one, a
    wall on device 1 of three puts its only word where word and device exchanged put it too) -- and the rows of test_joints.scene."""
    if (case, B) in _IN:
        return _IN[(case, B)]
    cfg = CASES[case]["cfg"]
    lay = synth.make_layout(cfg)
    arms = tuple((d, nm) for d, nm in enumerate(lay.dev_names) if nm != "base")
    sc = tw.scenario(B, False, cfg=cfg, listed=arms)
    paths = [None] * lay.ndev
    for i, (d, _) in enumerate(arms):
        paths[d] = sc["paths"][i]
    tgt_vel = 0.1 * synth.make_batch(cfg, B, seed=21)[2]["tgt_vel"] if "branch_b" in cfg else None
    more = np.array(sc["tgt"][::-1][:WIDE - B])      # targets of the robots a wide context holds beyond B (test_action_list_layouts' k13_wide)
    more[:, :, :3] += 0.01
    assert not sc["qd"].any()                        # (the fleet starts at rest: test 2's wall force has no damping term)
    _IN[(case, B)] = dict(q=sc["q"], qd=sc["qd"], tgt=sc["tgt"], tgt_vel=tgt_vel, paths=paths, arms=tuple(d for d, _ in arms),
                          sens=np.random.default_rng(43).normal(0.0, 5.0, size=(B, tr.NS)), rows=tjn.scene(lay), more=more,
                          walls=twl.median_walls(sc["tgt"][:, :, :3], wall_devices(case), r=0.01))
    return _IN[(case, B)]


def arm(osc, slot, case, B, sick=None, program="paths"):
    """Start state, targets, feed, walls, rows and program of the slot, every state and tick count reset.  A context wider than B gets
    targets for all its robots, in front of the coordinates (the slot then holds targets for max_batch robots, and rows B.. are nobody's
    to write).  program: "paths" (the layout's arm devices, threshold FAR), "stream" (a per-robot teleoperation stream), "pushes" (paths
    and a sensed and applied push per arm over ticks [2, 5)), None.  sick: that robot's coordinates are NaN."""
    x = inputs(case, B)
    q = x["q"]
    if sick is not None:
        q = q.copy()
        q[sick] = np.nan
    if osc.max_batch > B:
        assert osc._B[slot] == 0 and x["tgt_vel"] is None
        osc.set_targets(np.concatenate([x["tgt"], x["more"]]), slot=slot)
        osc.upload_q(q, x["qd"], slot=slot)
    else:
        osc.upload_q(q, x["qd"], slot=slot)
        osc.set_targets(x["tgt"], x["tgt_vel"], slot=slot)
    osc.set_sensordata(x["sens"], slot=slot)
    osc.set_walls(x["walls"], slot=slot)
    osc.set_joints(x["rows"], slot=slot)
    if program in ("paths", "pushes"):
        osc.set_waypoints(x["paths"], FAR, True, slot=slot)
    if program == "stream":
        osc.set_teleop_stream(tts.fleet_readings(B, T), tts.ORIGIN, slot=slot)
    if program == "pushes":
        ps = [dict(dev=d, window=(2, 5), apply=True, sense=True) for d in x["arms"]]
        osc.set_pushes(ps, tp.wrenches(np.random.default_rng(9), B, len(ps)), slot=slot)


_CHOPPED, _FULL = {}, {}


def chopped(case, B, monkeypatch):
    """The reference: T x rollout(1, trace_every=1) on the armed slot with downloads around each tick, and what the slot holds
    afterwards.  Once per (case, B); the conditions on its inputs are asserted on it."""
    if (case, B) not in _CHOPPED:
        lay, model, osc = open_rig(case, B, monkeypatch)
        arm(osc, 0, case, B)
        out = dict(qpos=[], qvel=[], targets=[], u=[], flags=[], ee_pose=[], wall_force=[], joint_tau=[])
        for _ in range(T):
            q, qd = osc.download_q()
            out["qpos"].append(q); out["qvel"].append(qd); out["targets"].append(osc.download_targets())
            r = osc.rollout(1, trace_every=1)
            out["u"].append(r["u"]); out["flags"].append(r["flags_any"]); out["ee_pose"].append(r["ee_trace"][0])
            ws = osc.wall_state()
            out["wall_force"].append(ws["force"]); out["joint_tau"].append(osc.joint_state()["tau"])
        osc.close()
        ref = {k: np.array(v) for k, v in out.items()}
        ref["final"] = r
        assert not np.any(ref["flags"] & BAD), "a robot froze in the chopped run"
        assert (ws["contact_ticks"] > 0).any() and ref["wall_force"].any(), "no robot touched its wall within T ticks"
        assert ref["joint_tau"].any()
        assert all((ref["targets"][t + 1] != ref["targets"][t]).any() for t in range(T - 1)), "the targets do not change every tick"
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CHOPPED[(case, B)] = ref
    return _CHOPPED[(case, B)]


def full_log(case, B, ticks, monkeypatch):
    """The all-robots, all-channels, every-tick log of the armed slot with the default ring.  Once per (case, B, ticks)."""
    if (case, B, ticks) not in _FULL:
        lay, model, osc = open_rig(case, B, monkeypatch)
        arm(osc, 0, case, B)
        _FULL[(case, B, ticks)] = osc.rollout_logged(ticks, ALL)
        osc.close()
    return _FULL[(case, B, ticks)]


# ---- 1. logged = the one-tick loop, per case -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("case", ISSUE_CASES)
def test_the_log_equals_the_one_tick_loop_per_case(case, every, monkeypatch):
    """test_rollout_log.test_the_log_equals_the_one_tick_loop with the case as a parameter, B = 130, T = 7, every 1 and 3: per logged tick
    qpos / qvel = download_q before the tick, targets = download_targets before it, u and flags the tick's, ee_pose its trace sample,
    wall_force and joint_tau the states' planes after it; the final u and the OR of the flags.  rlb11_branch_b: more than half the robots
    report FLAG_VEL_BRANCH_B in the logged flags."""
    B = 130
    ref = chopped(case, B, monkeypatch)
    lay, model, osc = open_rig(case, B, monkeypatch)
    arm(osc, 0, case, B)
    r = osc.rollout_logged(T, ALL, every=every)
    osc.close()
    ticks = np.arange(0, T, every)
    assert np.array_equal(r["log_ticks"], ticks) and list(r["log"]) == list(rollout_log.CHANNELS)
    assert_log_is(r["log"], ref, ticks, LOGGED)
    assert r["log"]["wrench"].shape == (len(ticks), B, lay.ndev, 6) and np.all(np.isfinite(r["log"]["wrench"]))
    assert r["log"]["wrench"].dtype == np.dtype(CASES[case]["dtype"]) and r["log"]["wrench"].any()
    assert same_bits(r["u"], ref["u"][-1]) and np.array_equal(r["flags_any"], np.bitwise_or.reduce(ref["flags"], axis=0))
    if "branch_b" in case:
        assert ((r["log"]["flags"] & _lib.FLAG_VEL_BRANCH_B) != 0).any(axis=0).mean() > 0.5


# ---- 2. tick 0 against references that share no kernel with the log --------------------------------------------------------------------
_ORACLE, _TICK0 = {}, {}


def oracle(cfg, q, qd, sens):
    """test_fromq_sensor_feed.oracle_records_and_wrench -> (EE poses [B, ndev, 7] in cfg's device order, world-frame wrench [B, ndev, 6]) of
    the states, once per (layout, states)."""
    key = (cfg, hashlib.sha1(np.ascontiguousarray(q).tobytes() + np.ascontiguousarray(qd).tobytes()).hexdigest())
    if key not in _ORACLE:
        from irl_control_amd.rigid_body import RigidBodyModel
        lay = synth.make_layout(cfg)
        R, W = tf.oracle_records_and_wrench(lay, RigidBodyModel.load("dual_ur5").ft_desc(lay.dev_names), q, qd, sens)
        _ORACLE[key] = (R["ee_pose"], W)
    return _ORACLE[key]


def tick0(case, monkeypatch):
    """B = 65, two slots.  Slot 0 is armed, its targets are downloaded and rollout_logged(T, ALL) runs on it; slot 1 holds the same state,
    those targets (and target velocities) and the feed, no walls, rows or program, and runs step_q; slot 1 again without a feed is
    refused the wrench channel.  Once per case."""
    if case not in _TICK0:
        B = 65
        x = inputs(case, B)
        lay, model, osc = open_rig(case, B, monkeypatch, n_slots=2)
        arm(osc, 0, case, B)
        tgt0 = osc.download_targets(0)
        r = osc.rollout_logged(T, ALL, slot=0)
        osc.upload_q(x["q"], x["qd"], slot=1)
        osc.set_targets(tgt0, x["tgt_vel"], slot=1)
        osc.set_sensordata(x["sens"], slot=1)
        u, fl = osc.step_q(slot=1, return_flags=True)
        osc.set_sensordata(None, slot=1)
        words = rollout_log.layout(lay.n, lay.ndev, ALL, B)[1]
        host = np.zeros((T, words))
        refused = rc_logged(osc, B, T, _lib.Log(_lib.LOG_WRENCH, 1, 0, 0, 0), None, host, slot=1)
        osc.close()
        assert not host.any()
        _TICK0[case] = dict(r=r, tgt0=tgt0, u=u, fl=fl, refused=refused, lay=lay)
    return _TICK0[case]


@pytest.mark.parametrize("case", F64_CASES + ["k12_admit_f32", "k13_wide_f32"])
def test_tick_0_against_references_that_share_no_kernel_with_the_log(case, monkeypatch):
    """B = 65, the sample of tick 0.  qpos and qvel: the uploaded arrays, on bits.  targets: download_targets before the tick (what the
    setters left: set_waypoints wrote waypoint 0), on bits.  ee_pose: oracle/rigid_body.py's EE pose of every device in the layout's device
    order, at the tolerance and comparison test_one_tick_against_the_cpu_oracles_per_layout applies to the EE trace (1e-10 / 2e-6 of the
    robot's largest entry by the context's dtype, as stored); rlbr10: devices 0 and 3 on bits.  u and flags: step_q's on a second slot
    holding the same state, targets and feed, on bits (no wall has acted and nothing is sensed on tick 0).  wall_force: the host restatement
    irl_control_amd/walls.py on the oracle's EE positions, the fleet at rest (v = 0), within test_walls.test_one_tick_force_against_the_
    oracle's bound 1e-10 (k (max|x| + r + |off|) + c max|jacp| sum|qvel|), whose second term is 0 at rest; devices without a wall exactly 0.
    A slot without a feed is refused the wrench channel with IRLOSC_ERR_STATE.
    Measured on an MI355X (printed; profiles/rollout_log_rates.md): ee_pose at most 7.8e-16 of the robot's largest entry on every case and
    dtype (the walk is float64), the wall force at most 2.49e-6 of its bound."""
    B = 65
    dtype = CASES[case]["dtype"]
    x, t0 = inputs(case, B), tick0(case, monkeypatch)
    lay, log = t0["lay"], t0["r"]["log"]
    assert t0["refused"] == ERR_STATE
    assert same_bits(log["qpos"][0], np.ascontiguousarray(x["q"])) and same_bits(log["qvel"][0], np.ascontiguousarray(x["qd"]))
    assert t0["tgt0"].dtype == np.dtype(dtype) and same_bits(log["targets"][0], t0["tgt0"])
    for d in x["arms"]:      # (and waypoint 0 is in, as the context stores it)
        assert same_bits(np.ascontiguousarray(t0["tgt0"][:, d, :3]), np.ascontiguousarray(x["paths"][d][:, 0].astype(dtype)))
    assert same_bits(log["u"][0], t0["u"]) and np.array_equal(log["flags"][0], t0["fl"]) and np.abs(t0["u"]).max() > 0
    ee, _ = oracle(CASES[case]["cfg"], x["q"], x["qd"], x["sens"])
    got = log["ee_pose"][0]
    assert got.shape == ee.shape == (B, lay.ndev, 7)
    scale = np.abs(ee).reshape(B, -1).max(axis=1)[:, None, None] + 1e-300
    ee_err = np.abs(got - ee) / scale
    tol = 1e-10 if dtype is F64 else 2e-6
    if case == "rlbr10":
        assert same_bits(np.ascontiguousarray(got[:, 0]), np.ascontiguousarray(got[:, 3]))
        assert not np.array_equal(got[:, 0], got[:, 1])
    dev, table = wl.normalise(x["walls"], lay.dev_names, B)
    worst = 0.0
    for d in range(lay.ndev):
        F = log["wall_force"][0][:, d]
        if d not in dev:
            assert not F.any(), d
            continue
        rows = twl.rows_of(dev, table, d)
        xo = ee[:, d, :3]
        Fo = wl.contact_force(xo, 0.0, rows)
        bound = 1e-10 * rows[0, 0, 5] * (np.abs(xo).max(axis=1) + rows[0, 0, 4] + np.abs(rows[0, :, 3]).max())
        err = np.abs(F - Fo).max(axis=1)
        worst = max(worst, float((err / bound).max()))
        inside = (wl.depth(xo, rows) > 0).sum(axis=0)      # (per wall: robots in contact on tick 0, and robots that are not)
        assert np.all((inside >= 8) & (inside <= B - 8)) and Fo[:, :2].any(axis=0).all(), (d, inside)
        assert np.all(err <= bound), (d, float((err / bound).max()), int(np.argmax(err / bound)))
    print(f"[tick 0 {case}] ee_pose against the oracle, per device: {' '.join(f'{e:.2g}' for e in ee_err.max(axis=(0, 2)))} (bound {tol:g}); "
          f"wall force: worst error / bound {worst:.3g}")
    assert ee_err.max() <= tol, (float(ee_err.max()), np.unravel_index(np.argmax(ee_err), ee_err.shape))


# ---- 3. the wrench ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F64_CASES)
def test_the_logged_wrench_against_the_oracle(case, monkeypatch):
    """B = 65, float64, every case (each has a feed), k13 itself among them: on ticks 0 (nothing sensed yet) and 3 the logged wrench against
    test_fromq_sensor_feed.oracle_records_and_wrench on the chopped run's coordinates, the force the walls applied on the tick before taken
    off the force words of the devices that have walls (tick_front's SENSE), at that file's TOL64 relative to the robot's largest wrench
    word -- the protocol of test_rollout_log.test_the_wrench_of_a_random_feed_against_the_oracle.  Two ticks: the oracle costs 17 ms per
    robot.  The base has no sensor: its words are exactly 0.
    Measured on an MI355X (printed; profiles/rollout_log_rates.md): at most 1.6e-15 on tick 0 and 1.2e-15 on tick 3."""
    B = 65
    x, ref, t0 = inputs(case, B), chopped(case, B, monkeypatch), tick0(case, monkeypatch)
    lay, log = t0["lay"], t0["r"]["log"]
    walled = sorted({w["dev"] for w in x["walls"]})
    assert log["wrench"].shape == (T, B, lay.ndev, 6)
    for t in (0, 3):
        assert same_bits(log["qpos"][t], ref["qpos"][t]) and same_bits(log["qvel"][t], ref["qvel"][t])
        _, W = oracle(CASES[case]["cfg"], ref["qpos"][t], ref["qvel"][t], x["sens"])
        W = W.copy()
        if t > 0:
            assert ref["wall_force"][t - 1].any()
            for d in walled:
                W[:, d, :3] -= ref["wall_force"][t - 1][:, d]
        for d, nm in enumerate(lay.dev_names):
            if nm == "base":
                assert not log["wrench"][:, :, d].any()
        err = np.abs(log["wrench"][t] - W).reshape(B, -1).max(axis=1) / np.abs(W).reshape(B, -1).max(axis=1)
        print(f"[wrench {case} tick {t}] logged wrench against the oracle: max rel err {err.max():.3g} (bound {tf.TOL64:g})")
        assert err.max() <= tf.TOL64, (t, float(err.max()))


def test_the_float32_wrench_is_the_float64_one_rounded(monkeypatch):
    """k12_admit, B = 65, tick 0: the float32 context's logged wrench within one float32 ulp of the float64 context's cast to float32.  The
    two runs share the state of tick 0 bit for bit (coordinates are float64 on both), and the feed's arithmetic is float64 on both: on
    the fused path csrc/osc_ft.hpp reads the EE quaternion from the walk's float64 exchange block, rotates in double and rounds once on
    the store."""
    a, b = tick0("k12_admit_f32", monkeypatch)["r"]["log"], tick0("k12_admit", monkeypatch)["r"]["log"]
    assert same_bits(a["qpos"][0], b["qpos"][0]) and same_bits(a["qvel"][0], b["qvel"][0])
    got, want = a["wrench"][0], b["wrench"][0].astype(F32)
    assert got.dtype == np.dtype(F32) and np.abs(want).max() > 1.0
    ulp = np.spacing(np.abs(want))
    print(f"[wrench k12_admit_f32 tick 0] max |float32 - (float32)float64| / ulp {(np.abs(got - want) / ulp).max():.3g}")
    assert np.all(np.abs(got - want) <= ulp)


# ---- 4. wide equals tight --------------------------------------------------------------------------------------------------------------
def run_all(case, B, monkeypatch, tight, program):
    """rollout_logged(T, ALL) on the armed slot of a context of the case (tight: of capacity B) -> the result, every state download, and
    the slot's targets of ALL the context's robots afterwards."""
    lay, model, osc = open_rig(case, B, monkeypatch, tight=tight)
    arm(osc, 0, case, B, program=program)
    r = osc.rollout_logged(T, ALL)
    st = dict(walls=osc.wall_state(), joints=osc.joint_state())
    st["program"] = osc.teleop_state() if program == "stream" else osc.waypoint_state()
    if program == "stream":
        st["program"] = dict(pose=st["program"]["pose"], tick=np.array(st["program"]["tick"]))
    tgt = np.empty((osc.max_batch, lay.ndev, 7), dtype=osc.dtype)
    osc._chk(osc.lib.irlosc_download_targets(osc._h, 0, osc.max_batch, _lib.ptr(tgt)))
    osc.close()
    return r, st, tgt


@pytest.mark.parametrize("case,program", [("k13_wide", "paths"), ("k13_wide_f32", "paths"), ("k13_wide", "stream"), ("k13_wide", "pushes")])
def test_a_wide_context_equals_a_tight_one(case, program, monkeypatch):
    """max_batch = 192 against max_batch = 130, everything set and run over B = 130 from the same inputs: the whole log, the final qpos,
    qvel, u and flags_any, and the downloads of wall_state, joint_state and the program's state (waypoint_state; the stream's pose
    [6][stride] and tick), on bits.  The wide slot's targets were given for all 192 robots: rows 130 .. 191 come back untouched, on bits.
    With paths on both dtypes; once with a per-robot teleoperation stream instead of paths; once with paths and a sensed and applied
    push per arm over ticks [2, 5) (pushes have no state download: their table is [wave][P 6][64], and what they did is in qpos, qvel and
    the logged wrench)."""
    B = 130
    x = inputs(case, B)
    (w, ws, wt), (n, ns, nt) = (run_all(case, B, monkeypatch, tight, program) for tight in (False, True))
    assert wt.shape[0] == WIDE and nt.shape[0] == B
    for name in rollout_log.CHANNELS:
        assert same_bits(w["log"][name], n["log"][name]), name
    for key in ("qpos", "qvel", "u", "flags_any"):
        assert same_bits(w[key], n[key]), key
    for part in ws:
        assert list(ws[part]) == list(ns[part])
        for key in ws[part]:
            assert same_bits(np.ascontiguousarray(ws[part][key]), np.ascontiguousarray(ns[part][key])), (part, key)
    assert same_bits(np.ascontiguousarray(wt[:B]), nt) and same_bits(np.ascontiguousarray(wt[B:]), x["more"].astype(CASES[case]["dtype"]))
    # the reference side's inputs: nobody froze, a wall was touched, the rows acted, the program moved the targets
    assert not np.any(n["flags_any"] & BAD) and n["log"]["wall_force"].any() and n["log"]["joint_tau"].any() and n["log"]["wrench"].any()
    assert all((n["log"]["targets"][t + 1] != n["log"]["targets"][t]).any() for t in range(T - 1))
    if program == "pushes":      # (and the pushes acted and were sensed: the same run without them differs in qvel and in the wrench of ticks 3 .. 5)
        plain = full_log(case, B, T, monkeypatch)
        assert np.abs(plain["qvel"] - n["qvel"]).max() > 0 and not np.array_equal(plain["log"]["wrench"][3], n["log"]["wrench"][3])
        assert same_bits(plain["log"]["wrench"][2], n["log"]["wrench"][2])


# ---- 5. subsets off k13 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robots", [[0, 63, 64, 129], [129]])
@pytest.mark.parametrize("case", ["rlbr10", "br7"])
def test_a_subset_is_those_rows_of_the_whole_log_per_case(case, robots, monkeypatch):
    B = 130
    full = full_log(case, B, T, monkeypatch)["log"]
    lay, model, osc = open_rig(case, B, monkeypatch)
    arm(osc, 0, case, B)
    r = osc.rollout_logged(T, ALL, robots=robots)
    osc.close()
    for name in rollout_log.CHANNELS:
        assert r["log"][name].shape[:2] == (T, len(robots)) and same_bits(r["log"][name], np.ascontiguousarray(full[name][:, robots])), name


def test_a_subset_in_a_wide_context_and_indices_beyond_B(monkeypatch):
    """k13_wide, B = 130: the list [0, 64, 129] gives those rows of the whole log; an index at or above B is refused with IRLOSC_ERR_ARG
    although the context has a robot of that number (130, and 191 = max_batch - 1), and leaves the slot as it was."""
    case, B, robots = "k13_wide", 130, [0, 64, 129]
    full = full_log(case, B, T, monkeypatch)["log"]
    lay, model, osc = open_rig(case, B, monkeypatch)
    arm(osc, 0, case, B)
    before = osc.download_q()
    host = np.zeros((T, rollout_log.layout(lay.n, lay.ndev, ALL, 3)[1]))
    for bad in ([0, 64, B], [0, 64, WIDE - 1], [B, B + 1, WIDE - 1]):
        assert rc_logged(osc, B, T, _lib.Log(ALL, 1, 3, 0, 0), bad, host) == ERR_ARG, bad
    assert not host.any() and all(same_bits(a, b) for a, b in zip(before, osc.download_q()))
    r = osc.rollout_logged(T, ALL, robots=robots)
    osc.close()
    for name in rollout_log.CHANNELS:
        assert r["log"][name].shape[:2] == (T, 3) and same_bits(r["log"][name], np.ascontiguousarray(full[name][:, robots])), name


# ---- 6. a two-sample ring off k13 ------------------------------------------------------------------------------------------------------
def test_a_ring_of_two_samples_wraps_on_four_devices(monkeypatch):
    """rlbr10, B = 130, T = 9, every tick, buffer_bytes = exactly two samples of rollout_log.layout(25, 4, ALL, B): nine drains, equal to
    the default ring on bits."""
    case, B, T9 = "rlbr10", 130, 9
    full = full_log(case, B, T9, monkeypatch)
    words = rollout_log.layout(25, 4, ALL, B)[1]
    lay, model, osc = open_rig(case, B, monkeypatch)
    assert (lay.n, lay.ndev) == (25, 4)
    arm(osc, 0, case, B)
    r = osc.rollout_logged(T9, ALL, buffer_bytes=2 * words * 8)
    osc.close()
    for name in rollout_log.CHANNELS:
        assert r["log"][name].shape[0] == T9 and same_bits(r["log"][name], full["log"][name]), name
    tp.same(r, full)


# ---- 7. pieces -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k13", "rlb16"])
def test_two_logged_calls_on_one_slot(case, monkeypatch):
    """rollout_logged(4, ALL, every=3) then rollout_logged(3, ["ee_pose", "wall_force"], every=3, robots=[5, 64]) on one slot, B = 130: the
    cadence counts the CALL's ticks, so the samples are the call ticks {0, 3} and {0} -- rows 0, 3 and 4 of the chopped run; the second
    call's channels and robot list differ from the first's (the ring and the index list are regrown and reused).  The slot's final state
    equals an unlogged rollout(7) on a second slot."""
    B = 130
    ref = chopped(case, B, monkeypatch)
    lay, model, osc = open_rig(case, B, monkeypatch, n_slots=2)
    for slot in (0, 1):
        arm(osc, slot, case, B)
    a = osc.rollout_logged(4, ALL, every=3, slot=0)
    b = osc.rollout_logged(3, ["ee_pose", "wall_force"], every=3, robots=[5, 64], slot=0)
    plain = osc.rollout(T, slot=1)
    states = [(osc.waypoint_state(s), osc.wall_state(s), osc.joint_state(s)) for s in (0, 1)]
    osc.close()
    assert np.array_equal(a["log_ticks"], [0, 3]) and np.array_equal(b["log_ticks"], [0])
    assert_log_is(a["log"], ref, np.array([0, 3]), LOGGED)
    assert sorted(b["log"]) == ["ee_pose", "wall_force"] and b["log"]["ee_pose"].shape == (1, 2, lay.ndev, 7)
    assert_log_is(b["log"], ref, np.array([4]), ("ee_pose", "wall_force"), rows=[5, 64])
    for key in ("qpos", "qvel", "u"):
        assert same_bits(b[key], plain[key]), key
    assert np.array_equal(a["flags_any"] | b["flags_any"], plain["flags_any"])
    assert same_bits(b["u"], ref["u"][-1]) and same_bits(b["qpos"], ref["final"]["qpos"])
    for got, want in zip(*states):
        assert list(got) == list(want)
        for key in want:
            assert same_bits(got[key], want[key]), key


# ---- 8. an action list under the log ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_lists_targets_of_the_tick_are_in_its_sample(dtype):
    """k13, B = 65, the WP / GRIP list of test_action_list.scenario: the list writes in front of the OSC step and nothing moves the targets
    behind it, so the logged targets of tick t = download_targets AFTER the chopped tick t; the logged u and flags are that tick's."""
    B = 65
    sc = tal.scenario(B)
    osc = tal.make_ctx(B, dtype, n_slots=2)
    assert_own_route("k13", dtype, osc.from_q_name, osc.kernel_name)
    for slot in (0, 1):
        tal.fill(osc, sc, slot)
        osc.set_action_list(sc["desc"], slot=slot)
    r = osc.rollout_logged(T, ["targets", "u", "flags"], slot=0)
    tgt, u, fl = [], [], []
    for _ in range(T):
        o = osc.rollout(1, slot=1)
        u.append(o["u"]); fl.append(o["flags_any"])
        tgt.append(osc.download_targets(1))
    acted = osc.action_state(0)["action"]
    osc.close()
    tgt = np.array(tgt)
    assert not np.array_equal(tgt[0], np.asarray(sc["tgt"], dtype=dtype)) and (tgt[-1] != tgt[0]).any() and acted.max() >= 1
    assert not np.any(np.array(fl) & BAD)
    assert same_bits(r["log"]["targets"], tgt) and same_bits(r["log"]["u"], np.array(u)) and np.array_equal(r["log"]["flags"], np.array(fl))


# ---- 9. a NaN robot on the FROMQ form --------------------------------------------------------------------------------------------------
def test_a_robot_with_nan_coordinates_is_alone_in_the_log_on_the_fromq_form(monkeypatch):
    """k13 with IRLOSC_LANE=0, B = 130, robot 96 (16 x 6: the first of its 16-robot block, healthy robots behind it in the block and in
    its wave) has NaN coordinates: every other robot's rows equal the healthy log on bits; the sick robot's qpos repeats bit for bit and
    its flags carry NONFINITE.  A NaN met as data."""
    case, B, sick = "k13_lane0", 130, 96
    full = full_log(case, B, T, monkeypatch)["log"]
    lay, model, osc = open_rig(case, B, monkeypatch)
    arm(osc, 0, case, B, sick=sick)
    r = osc.rollout_logged(T, ALL)
    osc.close()
    others = np.arange(B) != sick
    for name in rollout_log.CHANNELS:
        assert same_bits(np.ascontiguousarray(r["log"][name][:, others]), np.ascontiguousarray(full[name][:, others])), name
    assert (r["flags_any"][sick] & _lib.FLAG_NONFINITE) and not np.any(r["flags_any"][others] & BAD)
    for t in range(T):
        assert np.isnan(r["log"]["qpos"][t, sick]).all() and same_bits(r["log"]["qpos"][t, sick], r["log"]["qpos"][0, sick]), t
