"""The episode log of a rollout (-m gpu): irlosc_rollout_from_q_logged against the path callers had before it -- rollout(1) T times from
the same start with downloads around each tick.  Unless a tolerance is named every comparison is == on bits: widening to double is exact
and both runs execute the same kernels on the same inputs.
Other layouts, the row16 FROMQ form and contexts wider than B: tests/test_rollout_log_layouts.py."""
import ctypes as C

import numpy as np
import pytest

import test_fromq_sensor_feed as tf
import test_joints as tjn
import test_pushes as tp
import test_rollout as tr
import test_rollout_layouts as trl
import test_teleop_stream as tts
import test_walls as twl
import test_waypoints as tw
from irl_control_amd import _lib, pushes as pu, rollout_log

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
ERR_ARG, ERR_STATE = tr.ERR_ARG, tr.ERR_STATE
BAD = tp.BAD
T = 7
ALL = rollout_log.ALL
FAR = 10.0        # m: a waypoint threshold no arm is outside of, so every arm arrives on every tick and the targets change each tick
same_bits = tts.same_bits


# ---- the slot every test but 2 and 3 rolls out: k13 with paths, a feed, a wall per arm and the gripper scene's rows --------------------
def open_rig(B, dtype=F64, n_slots=2):
    osc = tw.make_ctx(B, dtype, n_slots=n_slots)
    osc.set_ft_sensors()
    return osc


def start_of(B, sick=None):
    """(q, qd) of tw.scenario(B, False); `sick`: that robot's coordinates are NaN."""
    sc = tw.scenario(B, False)
    q, qd = sc["q"], sc["qd"]
    if sick is not None:
        q = q.copy()
        q[sick] = np.nan
    return q, qd


def arm(osc, slot, B, sick=None):
    """Start state, targets, feed, walls, rows and paths of the slot, every state and tick count reset.  The walls: per arm the plane y =
    the median of the fleet's EE y at the start, radius 1 cm, so the half of the robots on its far side and those within 1 cm of it touch
    it on tick 0 (a lone robot is its own median: 1 cm deep)."""
    sc = tw.scenario(B, False)
    q, qd = start_of(B, sick)
    osc.upload_q(q, qd, slot=slot)
    osc.set_targets(sc["tgt"], slot=slot)
    osc.set_sensordata(np.random.default_rng(43).normal(0.0, 5.0, size=(B, tr.NS)), slot=slot)
    osc.set_walls(twl.median_walls(sc["tgt"][:, :, :3], (0, 1), r=0.01, normals=(twl.N_Y,)), slot=slot)
    osc.set_joints(tjn.scene(osc.layout), slot=slot)
    osc.set_waypoints(sc["paths"] + [None], FAR, True, slot=slot)


_CHOPPED = {}


def chopped(B, dtype):
    """The reference: T x rollout(1, trace_every=1) on the armed slot with downloads around each tick.  Computed once per (B, dtype)."""
    key = (B, np.dtype(dtype).name)
    if key not in _CHOPPED:
        osc = open_rig(B, dtype, n_slots=1)
        arm(osc, 0, B)
        out = dict(qpos=[], qvel=[], targets=[], u=[], flags=[], ee_pose=[], wall_force=[], joint_tau=[])
        contact = 0
        for _ in range(T):
            q, qd = osc.download_q()
            out["qpos"].append(q); out["qvel"].append(qd); out["targets"].append(osc.download_targets())
            r = osc.rollout(1, trace_every=1)
            out["u"].append(r["u"]); out["flags"].append(r["flags_any"]); out["ee_pose"].append(r["ee_trace"][0])
            ws = osc.wall_state()
            out["wall_force"].append(ws["force"]); out["joint_tau"].append(osc.joint_state()["tau"])
        contact = ws["contact_ticks"]
        osc.close()
        ref = {k: np.array(v) for k, v in out.items()}
        assert not np.any(ref["flags"] & BAD), "a robot froze in the chopped run"
        assert (contact > 0).any() and ref["wall_force"].any(), "no robot touched its wall within T ticks"
        assert ref["joint_tau"].any()
        assert all((ref["targets"][t + 1] != ref["targets"][t]).any() for t in range(T - 1)), "the targets do not change every tick"
        for a in ref.values():
            a.setflags(write=False)
        _CHOPPED[key] = ref
    return _CHOPPED[key]


def assert_log_is(log, ref, ticks, names, rows=slice(None)):
    for name in names:
        want = ref[name][ticks][:, rows]
        assert log[name].dtype == want.dtype and same_bits(log[name], np.ascontiguousarray(want)), name


# ---- 1. logged = chopped ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_log_equals_the_one_tick_loop(dtype, B, every):
    """k13, every channel, B = a lone lane / a full wave / one ragged robot / three waves with a ragged last, T = 7, every 1 and 3 (samples
    at ticks 0, 3, 6: T is no multiple).  Per logged tick: qpos / qvel = download_q before the tick, targets = download_targets before it
    (the cycler moves them behind the log's front launch, every tick), u and flags the tick's, ee_pose its trace sample, wall_force and
    joint_tau the states' planes after it (the back launch)."""
    ref = chopped(B, dtype)
    osc = open_rig(B, dtype, n_slots=1)
    arm(osc, 0, B)
    r = osc.rollout_logged(T, ALL, every=every)
    osc.close()
    ticks = np.arange(0, T, every)
    assert np.array_equal(r["log_ticks"], ticks) and list(r["log"]) == list(rollout_log.CHANNELS)
    assert_log_is(r["log"], ref, ticks, ("qpos", "qvel", "targets", "u", "flags", "ee_pose", "wall_force", "joint_tau"))
    assert r["log"]["wrench"].shape == (len(ticks), B, 3, 6) and np.all(np.isfinite(r["log"]["wrench"]))
    assert same_bits(r["u"], ref["u"][-1]) and np.array_equal(r["flags_any"], np.bitwise_or.reduce(ref["flags"], axis=0))


def test_single_channels_land_where_the_layout_says():
    """Each channel asked for alone (front ones, back ones, and a front + back pair) gives the rows it gives next to all the others."""
    B = 65
    ref = chopped(B, F64)
    osc = open_rig(B, F64, n_slots=1)
    for channels in (["qpos"], ["ee_pose"], ["targets"], ["u"], ["flags"], ["wall_force"], ["joint_tau"], ["qvel", "wall_force"]):
        arm(osc, 0, B)
        r = osc.rollout_logged(T, channels, every=3)
        assert sorted(r["log"]) == sorted(channels)
        assert_log_is(r["log"], ref, np.arange(0, T, 3), channels)
    osc.close()


# ---- 2. targets written in tick_front ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_streams_targets_of_the_tick_are_in_its_sample(dtype):
    """A per-robot teleoperation stream instead of paths, B = 65: the stream writes the targets in front of the OSC step and nothing moves
    them behind it, so targets of tick t = download_targets AFTER the chopped tick t."""
    B = 65
    osc = tts.make_ctx(B, dtype, n_slots=2)
    rd = tts.fleet_readings(B, T)
    for slot in (0, 1):
        tts.fill(osc, B, slot=slot)
        osc.set_teleop_stream(rd, tts.ORIGIN, slot=slot)
    r = osc.rollout_logged(T, ["targets", "u"], slot=0)
    tgt, u = [], []
    for _ in range(T):
        u.append(osc.rollout(1, slot=1)["u"])
        tgt.append(osc.download_targets(1))
    osc.close()
    tgt = np.array(tgt)
    assert all((tgt[t + 1] != tgt[t]).any() for t in range(T - 1))
    assert same_bits(r["log"]["targets"], tgt) and same_bits(r["log"]["u"], np.array(u))


# ---- 3. wrench -----------------------------------------------------------------------------------------------------------------------------
def wrench_ctx(dtype, B):
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, dtype, feed=True, seed=5, n_slots=2)
    tp.start(osc, model, g, B, (0, 1), damping=0.0)
    Wp = tp.wrenches(np.random.default_rng(9), B, 2)
    ps = [dict(dev=d, window=(2, 5), apply=True, sense=True) for d in (0, 1)]
    for slot in (0, 1):
        osc.set_pushes(ps, Wp, slot=slot)
    return lay, model, osc, ps, Wp


@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_wrench_of_a_silent_feed_is_the_sensed_push_negated(dtype):
    """k12 + admittance, B = 65, sensordata zero, one sensed push per arm over ticks [2, 5), no walls: the logged wrench is what
    pushes.summed_wrenches gives the tick to sense, negated and cast to the context dtype (0 - W is exact), and zero on the ticks whose
    step senses nothing (0, 1, 2 and 6: the sensors report a tick late)."""
    B = 65
    lay, model, osc, ps, Wp = wrench_ctx(dtype, B)
    osc.set_sensordata(np.zeros((B, tr.NS)), slot=0)
    r = osc.rollout_logged(T, ["wrench"], slot=0)
    osc.close()
    w = r["log"]["wrench"]
    assert w.dtype == np.dtype(dtype) and w.shape == (T, B, 2, 6)
    for t in range(T):
        S = pu.summed_wrenches(ps, Wp, lay.dev_names, t)
        assert S["sense_some"].all() == (t in (3, 4, 5)) and S["sense_some"].any() == (t in (3, 4, 5))
        assert np.array_equal(w[t], (-S["sense"]).astype(dtype)), t
        if t not in (3, 4, 5):
            assert not w[t].any(), t


def test_the_wrench_of_a_random_feed_against_the_oracle():
    """The same with random sensordata, float64: on ticks 0 (nothing sensed yet), 3 (inside the sensed window) and 6 (behind it) the
    logged wrench against test_fromq_sensor_feed.oracle_records_and_wrench on the chopped run's coordinates minus the sensed push, at that
    file's 1e-5 relative to the robot's largest wrench word (the tolerance it holds the feed to through u).  Three ticks, not seven: the
    oracle costs 17 ms per robot, and the three differ in everything the wrench depends on (state, sensed or not)."""
    B = 65
    lay, model, osc, ps, Wp = wrench_ctx(F64, B)
    sens = np.random.default_rng(43).normal(0.0, 5.0, size=(B, tr.NS))      # (what tp.start fed both slots)
    r = osc.rollout_logged(T, ["wrench", "qpos"], slot=0)
    qs = []
    for _ in range(T):
        qs.append(osc.download_q(1))
        osc.rollout(1, slot=1)
    osc.close()
    fd = model.ft_desc(lay.dev_names)
    for t in (0, 3, 6):
        q, qd = qs[t]
        assert same_bits(r["log"]["qpos"][t], q)
        _, W = tf.oracle_records_and_wrench(lay, fd, q, qd, sens)
        W = W - pu.summed_wrenches(ps, Wp, lay.dev_names, t)["sense"]
        err = np.abs(r["log"]["wrench"][t] - W).reshape(B, -1).max(axis=1) / np.abs(W).reshape(B, -1).max(axis=1)
        print(f"[tick {t}] logged wrench against the oracle: max rel err {err.max():.3g}")
        assert err.max() <= tf.TOL64, (t, float(err.max()))


# ---- 4. subset / 5. ring wrap ------------------------------------------------------------------------------------------------------------------
_FULL = {}


def full_log(B, ticks):
    """The all-robots, all-channels, every-tick log of the armed slot with the default ring.  Computed once per (B, ticks)."""
    if (B, ticks) not in _FULL:
        osc = open_rig(B, F64, n_slots=1)
        arm(osc, 0, B)
        _FULL[(B, ticks)] = osc.rollout_logged(ticks, ALL)
        osc.close()
    return _FULL[(B, ticks)]


@pytest.mark.parametrize("robots", [[0, 63, 64, 129], [129]])
def test_a_subset_is_those_rows_of_the_whole_log(robots):
    B = 130
    full = full_log(B, T)["log"]
    osc = open_rig(B, F64, n_slots=1)
    arm(osc, 0, B)
    r = osc.rollout_logged(T, ALL, robots=robots)
    osc.close()
    for name in rollout_log.CHANNELS:
        assert r["log"][name].shape[:2] == (T, len(robots)) and same_bits(r["log"][name], np.ascontiguousarray(full[name][:, robots])), name


def rc_logged(osc, B, ticks, lg, robots, host, slot=0):
    idx = None if robots is None else np.ascontiguousarray(robots, dtype=np.int32)
    return osc.lib.irlosc_rollout_from_q_logged(osc._h, slot, B, ticks, None if lg is None else C.byref(lg), _lib.ptr(idx), _lib.ptr(host), None, None)


def test_a_ring_of_two_samples_wraps():
    """buffer_bytes = exactly two samples (one per half), T = 9, every tick, B = 130: nine drains, every refill of a half waiting for its
    copy -- equal to the same call with the default ring (one drain).  A ring of one sample is refused."""
    B, T9 = 130, 9
    full = full_log(B, T9)
    words = rollout_log.layout(25, 3, ALL, B)[1]
    osc = open_rig(B, F64, n_slots=1)
    arm(osc, 0, B)
    r = osc.rollout_logged(T9, ALL, buffer_bytes=2 * words * 8)
    q = osc.download_q()
    host = np.zeros((T9, words))
    assert rc_logged(osc, B, T9, _lib.Log(ALL, 1, 0, 0, words * 8), None, host) == ERR_ARG
    assert rc_logged(osc, B, T9, _lib.Log(ALL, 1, 0, 0, 2 * words * 8 - 1), None, host) == ERR_ARG
    assert all(same_bits(a, b) for a, b in zip(q, osc.download_q())) and not host.any()
    osc.close()
    for name in rollout_log.CHANNELS:
        assert same_bits(r["log"][name], full["log"][name]), name
    tp.same(r, full)


# ---- 6. the log only reads -----------------------------------------------------------------------------------------------------------------------
def test_a_logged_rollout_leaves_what_an_unlogged_one_leaves():
    B = 130
    osc = open_rig(B, F64, n_slots=3)
    for slot in (0, 1, 2):
        arm(osc, slot, B)
    a = osc.rollout_logged(T, ALL, every=2, slot=0)
    b = osc.rollout(T, slot=1)
    c = osc.rollout_logged(T, None, slot=2)      # log == NULL through the new entry point
    states = [(osc.waypoint_state(s), osc.wall_state(s), osc.joint_state(s)) for s in (0, 1, 2)]
    osc.close()
    assert c["log"] is None and c["log_ticks"] is None
    for other, st in ((a, states[0]), (c, states[2])):
        tp.same(other, b)
        for got, want in zip(st, states[1]):
            assert list(got) == list(want)
            for key in want:
                assert same_bits(got[key], want[key]), key
    assert not np.any(b["flags_any"] & BAD) and states[1][1]["contact_ticks"].any()


# ---- 7. a sick robot is alone --------------------------------------------------------------------------------------------------------------------
def test_a_robot_with_nan_coordinates_is_alone_in_the_log():
    B, sick = 130, 96      # the middle of the second wave
    full = full_log(B, T)["log"]
    osc = open_rig(B, F64, n_slots=1)
    arm(osc, 0, B, sick=sick)
    r = osc.rollout_logged(T, ALL)
    osc.close()
    others = np.arange(B) != sick
    for name in rollout_log.CHANNELS:
        assert same_bits(np.ascontiguousarray(r["log"][name][:, others]), np.ascontiguousarray(full[name][:, others])), name
    q0 = start_of(B, sick)[0][sick]
    assert np.isnan(q0).all() and (r["flags_any"][sick] & BAD) and not np.any(r["flags_any"][others] & BAD)
    for t in range(T):      # frozen: its coordinates repeat bit for bit
        assert same_bits(r["log"]["qpos"][t, sick], q0), t


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_slot_as_it_was():
    B = 130
    osc = open_rig(B, F64, n_slots=2)
    arm(osc, 0, B)
    sc = tw.scenario(B, False)
    tw.fill(osc, sc, 1)      # slot 1: coordinates and targets, no feed, no walls, no rows
    words = rollout_log.layout(25, 3, ALL, B)[1]
    host = np.zeros((T, words))
    Log = _lib.Log
    before = [osc.download_q(s) for s in (0, 1)]
    ok = [0, 63, 64, 129]
    cases = [
        ("every 0", ERR_ARG, 0, Log(ALL, 0, 0, 0, 0), None, host),
        ("every negative", ERR_ARG, 0, Log(ALL, -1, 0, 0, 0), None, host),
        ("channels 0", ERR_ARG, 0, Log(0, 1, 0, 0, 0), None, host),
        ("an unknown bit", ERR_ARG, 0, Log(ALL | 512, 1, 0, 0, 0), None, host),
        ("reserved", ERR_ARG, 0, Log(ALL, 1, 0, 1, 0), None, host),
        ("robots not ascending", ERR_ARG, 0, Log(ALL, 1, 4, 0, 0), [0, 64, 63, 129], host),
        ("robots repeated", ERR_ARG, 0, Log(ALL, 1, 4, 0, 0), [0, 63, 63, 129], host),
        ("robots out of range", ERR_ARG, 0, Log(ALL, 1, 4, 0, 0), [0, 63, 64, 130], host),
        ("robots negative", ERR_ARG, 0, Log(ALL, 1, 4, 0, 0), [-1, 63, 64, 129], host),
        ("robots with n_robots 0", ERR_ARG, 0, Log(ALL, 1, 0, 0, 0), ok, host),
        ("robots with n_robots above B", ERR_ARG, 0, Log(ALL, 1, B + 1, 0, 0), ok, host),
        ("no robots with n_robots neither 0 nor B", ERR_ARG, 0, Log(ALL, 1, 4, 0, 0), None, host),
        ("log_host NULL", ERR_ARG, 0, Log(ALL, 1, 0, 0, 0), None, None),
        ("wrench without a feed", ERR_STATE, 1, Log(_lib.LOG_WRENCH, 1, 0, 0, 0), None, host),
        ("wall_force without walls", ERR_STATE, 1, Log(_lib.LOG_WALL_FORCE, 1, 0, 0, 0), None, host),
        ("joint_tau without rows", ERR_STATE, 1, Log(_lib.LOG_JOINT_TAU, 1, 0, 0, 0), None, host),
    ]
    for why, want, slot, lg, robots, h in cases:
        assert rc_logged(osc, B, T, lg, robots, h, slot=slot) == want, why
        assert osc.lib.irlosc_last_error(osc._h), why
        for s in (0, 1):
            assert all(same_bits(a, b) for a, b in zip(before[s], osc.download_q(s))), why
    assert not host.any()
    # ... and no tick count moved: the slot still rolls out like one that was never refused anything
    a = osc.rollout_logged(T, ALL, slot=0)
    st = osc.wall_state(0)
    # what the slot without a feed, walls and rows may log, it logs; n_robots = B without a list is the same as 0
    assert rc_logged(osc, B, T, Log(_lib.LOG_QPOS | _lib.LOG_U, 1, B, 0, 0), None, host, slot=1) == 0 and host.any()
    osc.close()
    full = full_log(B, T)
    for name in rollout_log.CHANNELS:
        assert same_bits(a["log"][name], full["log"][name]), name
    assert st["first_tick"].max() < T
