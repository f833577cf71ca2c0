"""The WP / GRIP action list on the GPU (-m gpu): irlosc_set_action_list / irlosc_download_action_state -- the action kernel
(csrc/osc_action.hpp) between the walk and the OSC step of a rollout tick, against its NumPy restatement
(action_sequence.action_list_tick) on one tick, against the host loop tick by tick, against itself in pieces and alone, next to a
robot that holds a NaN, on both forms of the fused step and a one-arm layout, with nothing else moving, and the state rules."""
import ctypes as C
import sys

import numpy as np
import pytest

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from irl_control_amd import BatchedOSC, _lib, synth                  # noqa: E402
from irl_control_amd import action_sequence as aseq                  # noqa: E402
from irl_control_amd.layout import pack_gains                        # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel                # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
F64, F32 = np.float64, np.float32
RIGHT, LEFT = slice(1, 7), slice(13, 19)            # arm joints of the Dual-UR5
Q_RIGHT = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3])
Q_LEFT = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2])
DT, DAMPING = 1e-3, 0.0
WP, GRIP = _lib.ACTION_WP, _lib.ACTION_GRIP

# Chosen on an MI355X so that the conditions asserted on the host loop hold (observed figures: the docstrings of the two host-loop
# tests below; the sweep behind the choice: profiles/action_list_rates.md)
PERTURB = 0.04        # rad, uniform on the six joints of the active arm: a waypoint is the EE pose of start + perturbation
MAX_ERROR = 0.04      # 2-norm of (metres, radians): generous, as the insertion example's
KP = 1.0              # of the adaptive limit: with the arms' gains (kp 200, kv 50) the limit bites where |xyz error| > KP / 4 x err
SPEED_FIXED = 0.02    # m/s, min_speed == max_speed of the fixed-speed scenario: bites where |xyz error| > 5 mm
SPEED_CLIP = (0.01, 3.0)      # the clip range of the other one: under every err in play, so the limit follows err bit by bit
GRIP_TICKS = 3
TICKS = 1500
KINDS = (WP, GRIP, WP, WP)      # the last WP returns to 'start_pos'
# real clip range: 10 x the largest deviation from the host loop measured on an MI355X (max |qpos| 1.25e-13, max |qvel| 1e-12, both on
# the float64 context; the float32 context: 0 and 0), both tighter than the 1e-9 the bound may not exceed
BOUND_QPOS = 1.25e-12
BOUND_QVEL = 1e-11


def base_gains(cfg):
    return synth.make_batch(cfg, 1, seed=0)[1]


def make_ctx(B, dtype=F64, n_slots=1, cfg="k13", max_batch=None, gains=None, feed=False):
    """A context for B robots (max_batch: its capacity, default B) with the layout's base gains (gains: another gains dict, per instance
    then with max_batch rows), the model, the plant and, with feed, the F/T sensors' description."""
    g = base_gains(cfg) if gains is None else gains
    osc = BatchedOSC(synth.make_layout(cfg), B if max_batch is None else max_batch, dtype=dtype, n_slots=n_slots)
    osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], g["max_vel"], g["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    if feed:
        osc.set_ft_sensors()
    osc.set_plant(DT, DAMPING)
    return osc


_PROBE = {}


def ee_start(q, qd, cfg):
    """EE poses [B, ndev, 7] (float64) at the start of a tick from coordinates (q, qd), as the fused walk computes them: the trace of
    one rollout tick on a context of its own (the walk's EE pose is a function of the coordinates alone)."""
    osc = _PROBE.get((cfg, len(q)))
    if osc is None:
        osc = _PROBE[(cfg, len(q))] = make_ctx(len(q), F64, cfg=cfg)
    osc.upload_q(q, qd)
    osc.set_targets(np.tile([0, 0, 0, 1.0, 0, 0, 0], (len(q), osc.layout.ndev, 1)))
    return osc.rollout(1, trace_every=1)["ee_trace"][0].copy()


_SCEN = {}


def start_state(B, rng):
    """(q, qd) [B, 25]: both arms at their start configurations + uniform(-0.15, 0.15) rad per joint, at rest."""
    q = np.zeros((B, 25))
    q[:, RIGHT] = Q_RIGHT + rng.uniform(-0.15, 0.15, (B, 6))
    q[:, LEFT] = Q_LEFT + rng.uniform(-0.15, 0.15, (B, 6))
    return q, np.zeros((B, 25))


def device_roles(cfg, active=None, passive=None):
    """(active, passive) device indices of a list on layout cfg: as given, or by name -- the first ur5right, and the first ur5left where
    the layout has one (else -1: no passive device)."""
    names = list(synth.make_layout(cfg).dev_names)
    ia = names.index("ur5right") if active is None else active
    io = (names.index("ur5left") if "ur5left" in names else -1) if passive is None else passive
    return ia, io


def arm_joints(cfg, dev):
    """The joints of the arm that device `dev` of layout cfg steers."""
    return {"ur5right": RIGHT, "ur5left": LEFT}[synth.make_layout(cfg).dev_names[dev]]


def default_list(fixed_speed=False, max_error=MAX_ERROR):
    """The list WP, GRIP, WP, WP('start_pos') as the arrays of a description."""
    A = len(KINDS)
    lo, hi = (SPEED_FIXED, SPEED_FIXED) if fixed_speed else SPEED_CLIP
    return dict(kind=np.array(KINDS, np.int32), xyz_from_start=np.array([0, 0, 0, 1], np.int32), grip_ticks=np.array([1, GRIP_TICKS, 1, 1], np.int32),
                kp=np.full(A, KP), max_error=np.array([max_error, 0.0, max_error, 1.5 * max_error]), min_speed=np.full(A, lo),
                max_speed=np.array([hi, hi, min(hi, 1.0), hi]), gripper_force=np.array([0.0, 0.2, 0.0, -0.08]))


def scenario(B, cfg="k13", seed=0, fixed_speed=False, perturb=PERTURB, max_error=MAX_ERROR, active=None, passive=None, hold=1,
             passive_quat=None, shared=False, lst=None):
    """-> dict(q, qd, tgt [B, ndev, 7]: the EE poses at the start, desc: the list WP, GRIP, WP, WP('start_pos') with per-robot poses --
    EE poses of the active arm (ur5right) at start + uniform(-perturb, perturb) on its joints).  fixed_speed: min_speed == max_speed on
    every WP.  active, passive: device indices (default: ur5right and ur5left by name); hold, passive_quat: the passive device's
    orientation rule; shared: one pose table for the fleet (robot 0's); lst: another list (the arrays of default_list; its WP poses are
    drawn the same way).  Computed once per key and never written to."""
    key = (B, cfg, seed, fixed_speed, perturb, max_error, active, passive, hold, None if passive_quat is None else tuple(passive_quat), shared,
           None if lst is None else tuple((k, tuple(np.asarray(v).tolist())) for k, v in sorted(lst.items())))
    if key in _SCEN:
        return _SCEN[key]
    rng = np.random.default_rng(2000 + seed)
    ia, io = device_roles(cfg, active, passive)
    arm = arm_joints(cfg, ia)
    q, qd = start_state(B, rng)
    lst = default_list(fixed_speed, max_error) if lst is None else lst
    A = len(lst["kind"])
    pose = np.zeros((B, A, 7))
    pose[:, :, 3] = 1.0
    tgt = ee_start(q, qd, cfg)
    for a in np.nonzero(np.asarray(lst["kind"]) == WP)[0]:
        g = q.copy()
        g[:, arm] += rng.uniform(-perturb, perturb, (B, 6))
        pose[:, a] = ee_start(g, qd, cfg)[:, ia]
    if shared:
        pose = pose[:1].copy()
    desc = dict(n_actions=A, active_dev=ia, passive_dev=io, passive_hold_orientation=int(hold),
                passive_quat=np.array(aseq.DEFAULT_EE_QUAT if passive_quat is None else passive_quat, dtype=F64), pose=pose,
                **{k: np.array(v) for k, v in lst.items()})
    for a in (q, qd, tgt, pose):
        a.setflags(write=False)
    _SCEN[key] = dict(q=q, qd=qd, tgt=tgt, desc=desc, cfg=cfg)
    return _SCEN[key]


def fill(osc, sc, slot=0, rows=slice(None)):
    osc.upload_q(sc["q"][rows], sc["qd"][rows], slot=slot)
    osc.set_targets(sc["tgt"][rows], slot=slot)


def sub_desc(desc, rows):
    return desc if len(desc["pose"]) == 1 else dict(desc, pose=np.ascontiguousarray(desc["pose"][rows]))


def packed_gains(lay, cfg, B, dtype, gains=None):
    """The gain records [B, ndev, 12] as a context of `dtype` stores them: the layout's base gains, or `gains` (per instance: B rows)."""
    g = base_gains(cfg) if gains is None else gains
    return pack_gains(lay, g["kp"], g["kv"], g["ko"], g["k"], g["d"], np.broadcast_to(g["max_vel"], (B, lay.ndev, 2)))[0].astype(dtype)


def host_loop(sc, dtype, T, q=None, gains=None, tgt_vel=None, feed=None):
    """T x (set_gains per instance, set_targets, rollout(1)) on a context of its own, the bookkeeping by action_list_tick on the EE
    poses at the start of every tick, targets and gains kept as the context stores them.  gains: the base gains (default: the
    layout's; per instance: B rows, of which the loop replaces word 9 only); tgt_vel [B, ndev, 6]: target velocities, set with the
    targets on every tick; feed [B, n_sensor]: a constant sensor feed.  -> dict(out: the last tick's rollout result, flags, state,
    tgt, gains, margin: the smallest |err - max_error| over every WP judgement of a robot in the list, entered: per robot the set of
    actions it entered)."""
    cfg, desc = sc["cfg"], sc["desc"]
    q = np.array(sc["q"] if q is None else q)
    qd = np.array(sc["qd"])
    B = len(q)
    osc = make_ctx(B, dtype, cfg=cfg, gains=gains, feed=feed is not None)
    lay, bg = osc.layout, base_gains(cfg) if gains is None else gains
    tgt = np.array(sc["tgt"], dtype=dtype)
    gains = packed_gains(lay, cfg, B, dtype, gains)
    if feed is not None:
        osc.upload_q(q, qd)
        osc.set_sensordata(feed)
    state = aseq.action_list_state(B)
    flags = np.zeros(B, np.uint32)
    margin, entered = np.inf, np.zeros((B, desc["n_actions"]), bool)
    out = None
    for t in range(T):
        ee = ee_start(q, qd, cfg)
        if t > 0:      # the WP judgements of this tick: every robot that is in a WP, on the target the previous tick's step aimed at
            before = state["action"]
            wp = np.nonzero((before < desc["n_actions"]) & (desc["kind"][np.minimum(before, desc["n_actions"] - 1)] == WP))[0]
            margin = min(margin, np.abs(judged_err(ee, tgt, desc)[wp] - desc["max_error"][before[wp]]).min(initial=np.inf))
        aseq.action_list_tick(state, ee, tgt, gains, desc, t)
        live = state["action"] < desc["n_actions"]
        entered[np.nonzero(live)[0], state["action"][live]] = True
        osc.set_gains(bg["kp"], bg["kv"], bg["ko"], bg["k"], bg["d"], gains[:, :, 9:11].astype(F64), bg["null_kv"])
        osc.upload_q(q, qd)
        osc.set_targets(tgt, tgt_vel)
        out = osc.rollout(1)
        flags |= out["flags_any"]
        q, qd = out["qpos"], out["qvel"]
    osc.close()
    return dict(out=out, flags=flags, state=state, tgt=tgt, gains=gains, margin=margin, entered=entered)


def judged_err(ee, tgt, desc):
    """The error step 1 of a tick judges every robot on: |calc_error(ee[active], its target as stored)| (the state's err of a robot that
    then enters a WP is +inf again)."""
    ia = desc["active_dev"]
    return np.linalg.norm(aseq._calc_error_batch(ee[:, ia], tgt[:, ia].astype(F64)), axis=1)


def device_list(sc, dtype, pieces, rows=slice(None), q=None, max_batch=None, gains=None, tgt_vel=None, feed=None, tgt=None, trace=False):
    """One context, the list on slot 0, rollout(p) for p in pieces.  max_batch: the context's capacity (default: the robots run);
    gains: its base gains (default: the layout's); tgt_vel, feed: target velocities and a constant sensor feed on the slot; tgt: the
    slot's targets where they cover MORE robots than the list (given before the coordinates; default: the scenario's, for `rows`);
    trace: every tick's EE poses.  -> dict(out: the last piece's result, outs: every piece's, flags, state, from_q_name, kernel_name,
    trace [ticks, B, ndev, 7] or None)."""
    qq = np.array(sc["q"] if q is None else q)[rows]
    osc = make_ctx(len(qq), dtype, cfg=sc["cfg"], max_batch=max_batch, gains=gains, feed=feed is not None)
    if tgt is not None:
        osc.set_targets(tgt, tgt_vel)
    osc.upload_q(qq, sc["qd"][rows])
    if tgt is None:
        osc.set_targets(sc["tgt"][rows], None if tgt_vel is None else tgt_vel[rows])
    if feed is not None:
        osc.set_sensordata(feed[rows])
    osc.set_action_list(sub_desc(sc["desc"], rows))
    flags = np.zeros(len(qq), np.uint32)
    traces, outs = [], []
    for p in pieces:
        out = osc.rollout(p, trace_every=1 if trace else 0)
        flags |= out["flags_any"]
        traces.append(out["ee_trace"])
        outs.append(out)
    st = osc.action_state()
    names = osc.from_q_name, osc.kernel_name
    osc.close()
    return dict(out=out, outs=outs, flags=flags, state=st, from_q_name=names[0], kernel_name=names[1], trace=np.concatenate(traces) if trace else None)


_RUNS = {}


def runs(B, dtype, fixed_speed, cfg="k13", T=TICKS):
    """(host loop, device list) of one scenario, computed once and shared by the tests that compare them."""
    key = (B, np.dtype(dtype).name, fixed_speed, cfg, T)
    if key not in _RUNS:
        sc = scenario(B, cfg=cfg, fixed_speed=fixed_speed)
        _RUNS[key] = (host_loop(sc, dtype, T), device_list(sc, dtype, (T,)))
    return _RUNS[key]


def assert_host_conditions(host, desc, T):
    A = desc["n_actions"]
    assert np.all(host["state"]["action"] == A), ("not every robot finished within T", np.bincount(host["state"]["action"], minlength=A + 1))
    assert host["entered"].all(), "every robot enters every action"
    ft = host["state"]["finished_tick"]
    assert ft.min() > 0 and ft.max() <= T and (len(ft) == 1 or len(set(ft)) >= 2), ft
    assert host["margin"] >= 1e-9, host["margin"]


def assert_discrete_equal(dev, host, T):
    """The device's state is as of the start of its last tick (T - 1); the host loop's state is the same tick's."""
    for key in ("action", "finished_tick", "grip_left", "gripper_force"):
        assert np.array_equal(dev["state"][key], host["state"][key]), key
    assert np.array_equal(dev["flags"], host["flags"])


# ---- 1. one tick --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [130, 1])
def test_one_and_two_ticks_against_the_numpy_restatement(B):
    """rollout(1) and, on a second slot, rollout(2) with the EE trace: the state after each against action_list_tick on the traced EE
    poses -- discrete fields exact, err within 1e-12 (both sides float64 with a handful of roundings and one atan2 each), max_vel0
    within kp x that; the targets and the gain word through their effect: qpos, qvel and u equal, bit for bit, those of a slot without
    a list that is given the restatement's targets and gains by hand."""
    sc = scenario(B)
    desc = sc["desc"]
    osc = make_ctx(B, F64, n_slots=2)
    lay = osc.layout
    for slot in (0, 1):
        fill(osc, sc, slot)
        osc.set_action_list(desc, slot=slot)
    o1 = osc.rollout(1, trace_every=1, slot=0)
    s1 = osc.action_state(0)
    o2 = osc.rollout(2, trace_every=1, slot=1)
    s2 = osc.action_state(1)
    osc.close()
    state, tgt, gains = aseq.action_list_state(B), np.array(sc["tgt"]), packed_gains(lay, "k13", B, F64)
    aseq.action_list_tick(state, o1["ee_trace"][0], tgt, gains, desc, 0)
    assert np.array_equal(o1["ee_trace"][0], o2["ee_trace"][0])
    for key in ("action", "grip_left", "finished_tick", "gripper_force", "max_vel0"):
        assert np.array_equal(s1[key], state[key]), key
    assert np.all(np.isinf(s1["err"])) and np.all(s1["max_vel0"] == desc["max_speed"][0])
    # the slot's effect on u: one tick by hand with the restatement's targets and gains
    hand = make_ctx(B, F64)
    bg = base_gains("k13")
    hand.set_gains(bg["kp"], bg["kv"], bg["ko"], bg["k"], bg["d"], gains[:, :, 9:11], bg["null_kv"])
    hand.upload_q(sc["q"], sc["qd"])
    hand.set_targets(tgt)
    h1 = hand.rollout(1)
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(o1[key], h1[key]), key
    assert np.abs(h1["u"]).max() > 0 and not np.array_equal(tgt, sc["tgt"])
    aseq.action_list_tick(state, o2["ee_trace"][1], tgt, gains, desc, 1)
    d = np.abs(s2["err"] - state["err"])
    dm = np.abs(s2["max_vel0"] - state["max_vel0"])
    print(f"[one tick B={B}] err {state['err'].min():.3g} .. {state['err'].max():.3g}, max |err_dev - err_numpy| {d.max():.3g}; "
          f"max_vel0 {state['max_vel0'].min():.3g} .. {state['max_vel0'].max():.3g}, max |dev - numpy| {dm.max():.3g}")
    assert np.all(np.isfinite(state["err"])) and d.max() <= 1e-12
    assert dm.max() <= KP * 1e-12                                    # max_vel0 = clip(kp err)
    gains[:, desc["active_dev"], 9] = s2["max_vel0"]                 # (the limit follows err's last bits: the hand-made tick takes the device's)
    hand.set_gains(bg["kp"], bg["kv"], bg["ko"], bg["k"], bg["d"], gains[:, :, 9:11], bg["null_kv"])
    hand.set_targets(tgt)
    h2 = hand.rollout(1)
    hand.close()
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(o2[key], h2[key]), key
    for key in ("action", "grip_left", "finished_tick", "gripper_force"):
        assert np.array_equal(s2[key], state[key]), key


# ---- 2. host loop = device list -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,dtype", [(130, F64), (64, F64), (1, F64), (130, F32)])
def test_host_loop_equals_device_list_bit_for_bit_with_a_fixed_speed(B, dtype):
    """min_speed == max_speed on every WP: the limit does not depend on err's last bits, so T x (set_gains per instance, set_targets,
    rollout(1)) with action_list_tick on the host = one rollout(T) with the list, bit for bit in qpos / qvel / u; action,
    finished_tick, grip_left, gripper_force equal.  Asserted on the host loop: every robot finishes within T, enters every action
    (the 'start_pos' WP included), two robots finish on different ticks, |err - max_error| >= 1e-9 at every WP judgement.
    Observed on the host loop on an MI355X (PERTURB 0.04, MAX_ERROR 0.04, SPEED_FIXED 0.02, T = 1500) -- finished_tick min / median /
    max, closest |err - max_error|:
        B = 130 float64     6 / 238.5 / 605    9.2e-07          B = 64 float64     6 / 205.5 / 619    2.6e-07
        B = 130 float32     6 / 238.5 / 605    9.1e-07          B = 1 float64      357                3.8e-05"""
    host, dev = runs(B, dtype, True)
    desc = scenario(B, fixed_speed=True)["desc"]
    ft = host["state"]["finished_tick"]
    print(f"[host loop fixed B={B} {np.dtype(dtype).name}] finished_tick min {ft.min()} median {np.median(ft):g} max {ft.max()}, "
          f"closest |err - max_error| {host['margin']:.3g}; {dev['from_q_name']}")
    if B > 1:
        assert_host_conditions(host, desc, TICKS)
    else:
        assert host["state"]["action"][0] == desc["n_actions"] and host["entered"].all() and host["margin"] >= 1e-9
    assert_discrete_equal(dev, host, TICKS)
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(dev["out"][key], host["out"][key]), key


@pytest.mark.parametrize("B,dtype", [(130, F64), (130, F32)])
def test_host_loop_equals_device_list_with_the_real_clip_range(B, dtype):
    """A clip range that is a range: min_speed 0.01, max_speed 3.0 (1.0 on action 2), kp 1 (SPEED_CLIP, KP), so max_vel0 = kp err on
    every tick of a WP and the limit follows err, whose last bits differ between the kernel and NumPy (one atan2 each): the
    coordinates may differ at rounding level.  (The demo's own 0.1 .. 3.0 with kp 6 never limits these arms here: with their gains the
    xyz error would have to exceed 1.5 x err.)  Discrete state equal; final qpos / qvel within 10 x the largest deviation measured.
    Measured on an MI355X after T = 1500 ticks, B = 130, device list against host loop:
        float64 context   max |qpos dev - host| 1.25e-13   max |qvel dev - host| 1e-12
        float32 context   0                                0        (the limit is stored as float32: err's last bits do not reach it)
    -> BOUND_QPOS = 1.25e-12, BOUND_QVEL = 1e-11, both under the 1e-9 the bound may not exceed.  Host loop, both contexts:
    finished_tick min 6, median 233, max 598; closest |err - max_error| 1.0e-06."""
    host, dev = runs(B, dtype, False)
    desc = scenario(B, fixed_speed=False)["desc"]
    ft = host["state"]["finished_tick"]
    dq = np.abs(dev["out"]["qpos"] - host["out"]["qpos"]).max()
    dv = np.abs(dev["out"]["qvel"] - host["out"]["qvel"]).max()
    print(f"[host loop clip B={B} {np.dtype(dtype).name}] finished_tick min {ft.min()} median {np.median(ft):g} max {ft.max()}, "
          f"closest |err - max_error| {host['margin']:.3g}; max |qpos dev - host| {dq:.3g}, |qvel| {dv:.3g}")
    assert_host_conditions(host, desc, TICKS)
    assert_discrete_equal(dev, host, TICKS)
    assert dq <= BOUND_QPOS and dv <= BOUND_QVEL


# ---- 3. pieces and fleet-mates ------------------------------------------------------------------------------------------------------
def test_a_rollout_in_pieces_and_a_robot_alone():
    """rollout(T) = rollout(T1) + rollout(T - T1) bit for bit, state included; robot b of B = 130 = the same robot alone (B = 1), for a
    robot of a full wave and one of the ragged wave."""
    B, T, T1 = 130, TICKS, 7
    sc = scenario(B)
    whole = runs(B, F64, False)[1]
    parts = device_list(sc, F64, (T1, T - T1))
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(whole["out"][key], parts["out"][key]), key
    assert np.array_equal(whole["flags"], parts["flags"])
    for key in whole["state"]:
        assert np.array_equal(whole["state"][key], parts["state"][key]), key
    assert whole["state"]["finished_tick"].max() >= T1
    for b in (5, 129):
        solo = device_list(sc, F64, (T,), rows=slice(b, b + 1))
        for key in ("qpos", "qvel", "u"):
            assert np.array_equal(whole["out"][key][b:b + 1], solo["out"][key]), (b, key)
        for key in whole["state"]:
            assert np.array_equal(whole["state"][key][b:b + 1], solo["state"][key]), (b, key)


def test_a_robot_with_nan_never_advances_and_is_alone():
    """A NaN in one robot's qpos (the base hinge and the first hinge of either arm: every EE pose is NaN): it stays in action 0, never
    finishes, and its 63 wave-mates (and everybody else) are bit-equal to the run without it."""
    B, T, bad = 130, 150, 64 + 29
    sc = scenario(B)
    q = sc["q"].copy()
    q[bad, [0, 1, 13]] = np.nan
    clean, out = device_list(sc, F64, (T,)), device_list(sc, F64, (T,), q=q)
    others = np.arange(B) != bad
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(out["out"][key][others], clean["out"][key][others]), key
    assert np.array_equal(out["flags"][others], clean["flags"][others])
    for key in clean["state"]:
        assert np.array_equal(out["state"][key][others], clean["state"][key][others]), key
    assert clean["state"]["action"].max() >= 1
    assert out["state"]["action"][bad] == 0 and out["state"]["finished_tick"][bad] == -1
    assert np.array_equal(out["out"]["qpos"][bad], q[bad], equal_nan=True)


# ---- 4. both forms and another layout -----------------------------------------------------------------------------------------------
def test_host_loop_equals_device_list_behind_the_row16_fromq_form(monkeypatch):
    monkeypatch.setenv("IRLOSC_LANE", "0")
    B, T = 130, TICKS
    sc = scenario(B, fixed_speed=True)
    host, dev = host_loop(sc, F64, T), device_list(sc, F64, (T,))
    assert "osc_lane" not in dev["from_q_name"] and "_fromq (fused" in dev["from_q_name"], dev["from_q_name"]
    assert_host_conditions(host, sc["desc"], T)
    assert_discrete_equal(dev, host, T)
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(dev["out"][key], host["out"][key]), key


def test_host_loop_equals_device_list_on_a_one_arm_layout():
    """r6: one device, the right arm alone: passive_dev = -1, nothing of a passive arm is written."""
    B, T = 130, TICKS
    sc = scenario(B, cfg="r6", fixed_speed=True)
    assert sc["desc"]["passive_dev"] == -1
    host, dev = host_loop(sc, F64, T), device_list(sc, F64, (T,))
    assert_host_conditions(host, sc["desc"], T)
    assert_discrete_equal(dev, host, T)
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(dev["out"][key], host["out"][key]), key


# ---- 5. nothing else moves ----------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    """One context, two slots.  A rollout before set_action_list = a rollout after setting and clearing the list (u, coordinates,
    flags_any).  With a list set on slot 0: slot 1's rollout and step_q on slot 0 give the bits they give without a list, and the
    context's gains are not written (a rollout on slot 1 after the list ran on slot 0 equals the one before)."""
    B, T = 130, 40
    sc = scenario(B)
    osc = make_ctx(B, F64, n_slots=2)
    fill(osc, sc, 0)
    fill(osc, sc, 1)
    before = osc.rollout(T, slot=0)
    other_before = osc.rollout(T, slot=1)
    fill(osc, sc, 0)
    u_before = osc.step_q(slot=0).copy()
    osc.set_action_list(sc["desc"], slot=0)
    osc.set_action_list(None, slot=0)
    after = osc.rollout(T, slot=0)
    for key in ("qpos", "qvel", "u", "flags_any"):
        assert np.array_equal(before[key], after[key]), key
    fill(osc, sc, 0)
    fill(osc, sc, 1)
    osc.set_action_list(sc["desc"], slot=0)
    assert np.array_equal(osc.step_q(slot=0), u_before)              # every other step ignores the list and its gains
    assert np.all(osc.action_state(0)["action"] == 0) and np.all(osc.action_state(0)["max_vel0"] == 0)
    with_list = osc.rollout(T, slot=0)
    assert not np.array_equal(with_list["qpos"], before["qpos"])     # (the list did run)
    other_after = osc.rollout(T, slot=1)
    for key in ("qpos", "qvel", "u", "flags_any"):
        assert np.array_equal(other_before[key], other_after[key]), key
    osc.upload_q(sc["q"], sc["qd"], slot=0)                          # uploads of coordinates leave the list (and its state) alone
    assert osc.action_state(0)["action"].max() >= 0
    osc.close()


# ---- 6. state rules -----------------------------------------------------------------------------------------------------------------
def c_desc(d, **over):
    d = dict(d, **over)
    s = _lib.ActionList()
    s.n_actions, s.active_dev, s.passive_dev = int(d["n_actions"]), int(d["active_dev"]), int(d["passive_dev"])
    s.passive_hold_orientation, s.nb = int(d["passive_hold_orientation"]), int(d.get("nb", len(d["pose"])))
    for i in range(4):
        s.passive_quat[i] = float(d["passive_quat"][i])
    for a in range(min(len(d["kind"]), _lib.MAX_ACTIONS)):
        s.kind[a], s.xyz_from_start[a], s.grip_ticks[a] = int(d["kind"][a]), int(d["xyz_from_start"][a]), int(d["grip_ticks"][a])
        s.kp[a], s.max_error[a], s.min_speed[a], s.max_speed[a] = d["kp"][a], d["max_error"][a], d["min_speed"][a], d["max_speed"][a]
        s.gripper_force[a] = d["gripper_force"][a]
    return s


def test_state_rules():
    B = 70
    sc = scenario(B)
    desc = sc["desc"]
    pose = np.ascontiguousarray(desc["pose"])
    lay = synth.make_layout("k13")
    osc = BatchedOSC(lay, B, dtype=F64)
    lib, h = osc.lib, osc._h
    bg = base_gains("k13")

    def set_al(d=desc, p=pose, n=B, slot=0, **over):
        return lib.irlosc_set_action_list(h, slot, n, C.byref(c_desc(d, **over)), _lib.ptr(p))

    def state_rc():
        return lib.irlosc_download_action_state(h, 0, B, None, None, None, None, None, None)

    def vary(key, a, val):
        v = np.array(desc[key], dtype=np.float64 if desc[key].dtype.kind == "f" else np.int32)
        v[a] = val
        return {key: v}

    # IRLOSC_ERR_STATE: before set_model, set_gains, targets for B; has_max_vel == 0 for the active device; download without a list
    assert set_al() == ERR_STATE and "irlosc_set_model" in lib.irlosc_last_error(h).decode()
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(DT, DAMPING)
    assert set_al() == ERR_STATE and "irlosc_set_gains" in lib.irlosc_last_error(h).decode()
    osc.set_gains(bg["kp"], bg["kv"], bg["ko"], bg["k"], bg["d"], bg["max_vel"], bg["null_kv"])
    osc.upload_q(sc["q"], sc["qd"])
    assert set_al() == ERR_STATE and "irlosc_set_targets" in lib.irlosc_last_error(h).decode()
    assert lib.irlosc_set_targets(h, 0, B - 1, _lib.ptr(np.ascontiguousarray(sc["tgt"][:B - 1])), None) == 0
    assert set_al() == ERR_STATE and state_rc() == ERR_STATE
    osc.set_targets(sc["tgt"])
    g, nk, nb = pack_gains(lay, bg["kp"], bg["kv"], bg["ko"], bg["k"], bg["d"], bg["max_vel"], bg["null_kv"])
    unlimited = g.copy()
    unlimited[:, desc["active_dev"], 11] = 0.0
    assert lib.irlosc_set_gains(h, _lib.ptr(unlimited), _lib.ptr(nk), nb) == 0
    assert set_al() == ERR_STATE and "has_max_vel" in lib.irlosc_last_error(h).decode()
    only_grip = dict(kind=np.array([GRIP] * 4, np.int32), grip_ticks=np.array([2] * 4, np.int32))
    assert set_al(**only_grip) == 0 and state_rc() == 0      # (a list without a WP sets no limit)
    assert lib.irlosc_set_gains(h, _lib.ptr(g), _lib.ptr(nk), nb) == 0
    assert set_al() == 0 and state_rc() == 0
    osc.rollout(10)
    before = osc.action_state()
    assert np.all(np.isfinite(before["err"])) and np.all(before["max_vel0"] > 0)
    # IRLOSC_ERR_ARG, and the list in force stays whole
    nan_pose = pose.copy()
    nan_pose[B - 1, 2, 5] = np.nan
    bad = [dict(n_actions=0), dict(n_actions=33), dict(active_dev=3), dict(active_dev=-1), dict(passive_dev=0), dict(passive_dev=7),
           dict(passive_hold_orientation=2), dict(nb=2), dict(nb=0), dict(passive_quat=np.array([1.0, np.nan, 0, 0])),
           vary("kind", 1, 2), vary("grip_ticks", 1, 0), vary("kp", 0, np.inf), vary("max_error", 2, np.nan), vary("min_speed", 0, 5.0),
           vary("max_speed", 3, np.inf), vary("gripper_force", 1, np.nan), vary("xyz_from_start", 0, 2)]
    for over in bad:
        assert set_al(**over) == ERR_ARG, (over, lib.irlosc_last_error(h).decode())
    assert set_al(p=nan_pose) == ERR_ARG and set_al(p=None) == ERR_ARG and set_al(n=0) == ERR_ARG and set_al(slot=5) == ERR_ARG
    after = osc.action_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a rollout over more robots than the list covers is refused
    assert set_al(n=B - 6, p=np.ascontiguousarray(pose[:B - 6]), nb=B - 6) == 0
    assert lib.irlosc_rollout_from_q(h, 0, B, 1, 0, None, None, None) == ERR_STATE and "action list" in lib.irlosc_last_error(h).decode()
    assert state_rc() == ERR_STATE
    # cleared by a NULL description, set_gains, set_targets, set_waypoints and set_model; a list clears waypoint paths
    assert set_al() == 0 and state_rc() == 0
    assert lib.irlosc_set_action_list(h, 0, B, None, None) == 0 and state_rc() == ERR_STATE
    assert set_al() == 0 and state_rc() == 0
    assert lib.irlosc_set_gains(h, _lib.ptr(g), _lib.ptr(nk), nb) == 0 and state_rc() == ERR_STATE
    assert set_al() == 0 and state_rc() == 0
    osc.set_targets(sc["tgt"])
    assert state_rc() == ERR_STATE
    assert set_al() == 0 and state_rc() == 0
    osc.set_waypoints([sc["tgt"][:, 0, None, :3], None, None], 0.01, True)
    assert state_rc() == ERR_STATE
    assert set_al() == 0 and state_rc() == 0
    assert lib.irlosc_download_waypoint_state(h, 0, B, None, None, None) == ERR_STATE
    # one writer of the targets (the table in include/irlosc.h): what an entry point does not end stays whole.  A list is in force here.
    n = B - 6
    keys = ("action", "grip_left", "err", "max_vel0", "gripper_force", "finished_tick")
    wp = _lib.Waypoints()
    wp.count[0], wp.threshold[0], wp.loop[0], wp.nb = 1, 0.01, 1, B
    wp_tab = np.zeros((B, lay.ndev, 1, 3))
    wp_tab[:, 0, 0] = sc["tgt"][:, 0, :3]                # one waypoint for device 0: its EE position at the start

    def set_wp(tab=wp_tab):
        return lib.irlosc_set_waypoints(h, 0, B, C.byref(wp), _lib.ptr(tab))

    def wp_rc():
        return lib.irlosc_download_waypoint_state(h, 0, B, None, None, None)

    def al_state(m):
        out = dict(action=np.empty(m, np.int32), grip_left=np.empty(m, np.int32), err=np.empty(m), max_vel0=np.empty(m),
                   gripper_force=np.empty(m), finished_tick=np.empty(m, np.int32))
        assert lib.irlosc_download_action_state(h, 0, m, *[_lib.ptr(out[k]) for k in keys]) == 0
        return out

    # ... a NULL paths description ends only paths; a refused irlosc_set_waypoints changes nothing: IRLOSC_ERR_ARG (a NaN waypoint) ...
    assert lib.irlosc_set_waypoints(h, 0, B, None, None) == 0 and state_rc() == 0
    osc.rollout(3)
    before = al_state(B)
    nan_tab = wp_tab.copy()
    nan_tab[B - 1, 0, 0, 1] = np.nan
    assert set_wp(nan_tab) == ERR_ARG
    after = al_state(B)
    assert all(np.array_equal(before[k], after[k]) for k in keys)
    # ... and IRLOSC_ERR_STATE (paths for more robots than the targets cover)
    assert lib.irlosc_set_targets(h, 0, n, _lib.ptr(np.ascontiguousarray(sc["tgt"][:n])), None) == 0
    assert set_al(n=n, p=np.ascontiguousarray(pose[:n]), nb=n) == 0
    assert lib.irlosc_rollout_from_q(h, 0, n, 3, 0, None, None, None) == 0
    before = al_state(n)
    assert set_wp() == ERR_STATE and "irlosc_set_targets" in lib.irlosc_last_error(h).decode()
    after = al_state(n)
    assert all(np.array_equal(before[k], after[k]) for k in keys)
    # paths that replace a list count their ticks from 0 (the list's counter stood at 3) ...
    osc.set_targets(sc["tgt"])
    osc.upload_q(sc["q"], sc["qd"])                      # (the narrower rollout left coordinates of n robots)
    assert set_al() == 0
    osc.rollout(3)
    osc.upload_q(sc["q"], sc["qd"])                      # (back at the start: device 0 arrives on tick 0, and again on tick 1)
    assert set_wp() == 0 and wp_rc() == 0 and state_rc() == ERR_STATE
    osc.rollout(2)
    before = osc.waypoint_state()
    assert before["last_tick"][:, 0].min() >= 0 and before["last_tick"][:, 0].max() <= 1 and np.all(before["last_tick"][:, 1:] == -1)
    # ... and irlosc_set_gains, a NULL list description and a refused irlosc_set_action_list leave them whole
    assert lib.irlosc_set_gains(h, _lib.ptr(g), _lib.ptr(nk), nb) == 0 and wp_rc() == 0
    assert lib.irlosc_set_action_list(h, 0, B, None, None) == 0 and wp_rc() == 0
    assert set_al(n_actions=0) == ERR_ARG and wp_rc() == 0
    after = osc.waypoint_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert set_al() == 0 and state_rc() == 0 and wp_rc() == ERR_STATE
    osc.upload_q(sc["q"], sc["qd"])                      # uploads of coordinates leave the list alone
    assert state_rc() == 0
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    assert state_rc() == ERR_STATE
    osc.close()
