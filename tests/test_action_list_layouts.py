"""The WP / GRIP action list off k13 and off the demo's list (-m gpu): what tests/test_action_list.py holds on one description -- k13, active
device 0, passive device 1, the passive arm keeping its orientation, per-robot tables, WP GRIP WP WP, max_batch == B, broadcast gains --
here with the layout, both device indices, the hold flag and passive_quat, the table's form, the list, the context's capacity, the
base gains, target velocities and a sensor feed as parameters of that file's helpers.

A SHORT SCENARIO, so that every test takes seconds (short_scenario): T = 16 ticks instead of 1500.  A WP pose of a robot is the active
arm's EE pose (the walk's own: ee_start) at its start configuration + s u on the arm's six joints, s = +-1, u uniform in [0.5, 1] x
    NEAR  1e-3 rad:  err 4e-4 .. 4.3e-3, at least 9 x under max_error = 0.04: judged as arrived on the tick after it was entered
    FAR   0.3 rad:   err 0.14 .. 1.15, at least 3.5 x over it: an arm limited to 2 cm/s moves under 1 mm in the ticks of a test
(figures of the CPU oracle's EE poses over 130 robots, k13 either arm and rlbr10).  Robot b STALLS at action (A - (B - 1 - b)) mod (A + 1):
its WP poses before that action are near, that action's is far; a GRIP there runs on and the next WP is far; A: it never stalls -- so
the last robot of the ragged last wave finishes.  Stalling robots alone end in WP actions only, so a third class, LATE, makes GRIP
actions final ones: a late pose lies 0.04 + delta straight along x from the EE position at the start, orientation kept (on a device
without xyz rows: turned by 0.04 + delta about x, position kept), delta from the closed loop's own law -- a velocity-limited arm
covers d_k = dt sum_j v_j, v_{j+1} = v_j + dt kv (k_x v_lim - v_j), in k ticks (limit_vel, oracle/osc_oracle.py; the angle of an
orientation-only device follows theta'' = -ko theta - kv theta') -- at the middle of (d_{k-1}, d_k] for a ladder of k around the ticks that
leave the robot in each GRIP at tick T - 1, two spare rungs either side for what that law leaves out (the other devices, the null
space).  Which rung lands where is not asserted; that every action index is some robot's final one is.

Asserted on the REFERENCE side of every comparison of the standard list (assert_reference_conditions): every action index 0 .. A is the
final action of at least one robot; a finisher sits in the last wave (the ragged one wherever B has one: B = 192 has none); every WP
is entered by some robot; |err - max_error| >= 1e-9 at every WP judgement; and flags_any are equal.  The other lists of part 2 assert
what their docstrings say: a GRIP of one tick is a final action only for a robot that arrives on one given tick, and their ladders
are not built.

1. host loop = device list, bit for bit, per layout and role (CASES);  2. list shapes against the NumPy restatement on the traced EE
poses;  3. two slots interleaved, and a list set again midway;  4. rollouts over fewer robots than the list covers.
Every case asserts its route from from_q_name / kernel_name (assert_route: test_rollout_layouts.ROUTES, and the (1, 6, 6) lane tier
on its own kernel for k13 and k12_admit, as that file's cycler case words it)."""
import numpy as np
import pytest

import test_action_list as tal
import test_rollout_layouts as trl
from irl_control_amd import _lib, synth
from irl_control_amd import action_sequence as aseq

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
WP, GRIP = tal.WP, tal.GRIP
NEAR, FAR = 1e-3, 0.3         # rad on the active arm's joints
MAX_ERROR = 0.04
SPEED_FIXED = tal.SPEED_FIXED
T, PIECES = 16, (5, 11)
QUAT = np.array([0.5, -0.5, 0.5, 0.5])      # a unit quaternion that is not DEFAULT_EE_QUAT and has no zero component
W, WS = ("WP",), ("WP", "start")


def G(n):
    return ("GRIP", n)


STANDARD = (W, G(3), W, G(1), G(2), WS)      # a robot that never stalls finishes on tick 9
# late poses of the standard list: (WP action, ticks k after it was entered on which the arm is to arrive, first robot of the ladder).
# Final action 1 (GRIP(3)) needs WP 0 judged as arrived on tick 13 .. 15; action 3 (GRIP(1)) WP 2 -- entered on tick 4 -- on tick 15,
# k = 11; action 4 (GRIP(2)) WP 2 on tick 13 or 14, k = 9 or 10.
STANDARD_LATE = ((0, range(11, 18), 8), (2, range(7, 14), 70))


def make_list(actions, speed=(SPEED_FIXED, SPEED_FIXED), kp=1.0, max_error=MAX_ERROR):
    """The arrays of a list from ("WP",) / ("WP", "start") / ("GRIP", ticks) entries; gripper_force distinct per action."""
    A = len(actions)
    kind = np.array([WP if a[0] == "WP" else GRIP for a in actions], np.int32)
    return dict(kind=kind, xyz_from_start=np.array([int(a[0] == "WP" and len(a) > 1) for a in actions], np.int32),
                grip_ticks=np.array([a[1] if a[0] == "GRIP" else 1 for a in actions], np.int32), kp=np.full(A, float(kp)),
                max_error=np.where(kind == WP, max_error, 0.0), min_speed=np.full(A, float(speed[0])), max_speed=np.full(A, float(speed[1])),
                gripper_force=np.array([0.05 * (a + 1) * (-1) ** a for a in range(A)]))


def travel(k, kv, kx, vlim, dt=tal.DT):
    """d_0 .. d_k: what a velocity-limited arm covers along one axis in 0 .. k ticks from rest (the module docstring's law)."""
    v, d, out = 0.0, 0.0, [0.0]
    for _ in range(k):
        v += dt * kv * (kx * vlim - v)
        d += dt * v
        out.append(d)
    return np.array(out)


def turned(k, ko, kv, dt=tal.DT):
    """theta_0 .. theta_k over theta_0 of an orientation error left to theta'' = -ko theta - kv theta' from rest."""
    th, w, out = 1.0, 0.0, [1.0]
    for _ in range(k):
        w += dt * (-ko * th - kv * w)
        th += dt * w
        out.append(th)
    return np.array(out)


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


_SHORT = {}


def short_scenario(B, cfg="k13", active=None, passive=None, hold=1, passive_quat=None, actions=STANDARD, late=STANDARD_LATE, shared=None,
                   speed=(SPEED_FIXED, SPEED_FIXED), kp=1.0, max_error=MAX_ERROR, exact_every=0, gains=None, seed=0):
    """-> the dict of test_action_list.scenario (q, qd, tgt: the EE poses at the start, desc, cfg) + stall [B], late: the robots with a
    late pose.  shared: None = a table per robot; else the action at which the ONE table of the fleet is far (-1: nowhere) -- the robots
    then start within 1e-3 rad of one configuration, or the one table would be near for one of them only.  exact_every = n: every n-th
    robot's poses are its EE pose at the start itself (err 0).  gains: per-instance base gains (the late ladder reads the robot's own).
    Computed once per key and never written to."""
    key = (B, cfg, active, passive, hold, None if passive_quat is None else tuple(passive_quat), actions, late, shared, speed, kp, max_error,
           exact_every, gains is not None, seed)
    if key in _SHORT:
        return _SHORT[key]
    rng = np.random.default_rng(3000 + seed)
    lay = synth.make_layout(cfg)
    ia, io = tal.device_roles(cfg, active, passive)
    arm = tal.arm_joints(cfg, ia)
    q, qd = tal.start_state(B, rng)
    if shared is not None:
        for arm_ in (tal.RIGHT, tal.LEFT):
            q[:, arm_] = q[0, arm_] + rng.uniform(-1e-3, 1e-3, (B, 6))
    lst = make_list(actions, speed, kp, max_error)
    A = len(actions)
    wps = np.nonzero(lst["kind"] == WP)[0]
    stall = (A - (B - 1 - np.arange(B))) % (A + 1) if shared is None else np.full(B, A if shared < 0 else shared)
    tgt = tal.ee_start(q, qd, cfg)
    pose = np.zeros((B, A, 7))
    pose[:, :, 3] = 1.0
    for a in wps:
        far = np.array([a == min([w for w in wps if w >= s], default=-1) for s in stall])      # the first WP at or behind the stall
        amp = np.where(far, FAR, NEAR)
        if shared is not None:
            amp[:] = amp[0]
        g = q.copy()
        g[:, arm] += (amp * rng.choice([-1.0, 1.0], B))[:, None] * rng.uniform(0.5, 1.0, (B, 6))
        if shared is not None:
            g[:] = g[0]
        pose[:, a] = tal.ee_start(g, qd, cfg)[:, ia]
        if exact_every:
            pose[::exact_every, a] = tgt[::exact_every, ia]
    bg = tal.base_gains(cfg) if gains is None else gains
    per = lambda x, b: float(np.asarray(x)[b, ia] if np.ndim(x) == 2 else np.asarray(x)[ia])      # noqa: E731
    has_xyz = bool(np.any(lay.ctrlr_dof[ia][:3]))
    late_rows = []
    for a, ks, first in (late if shared is None else ()):
        for i, k in enumerate(ks):
            b = first + i
            if b >= B:
                break
            late_rows.append(b)
            pose[b, wps] = tgt[b, ia]      # its other poses: where it starts (err 0), so that it is where the ladder assumes it
            if has_xyz:
                kx = float(np.asarray(bg["k"])[b, ia, 0] if np.ndim(bg["k"]) == 3 else np.asarray(bg["k"])[ia][0])
                d = travel(k, per(bg["kv"], b), kx, speed[1])
                pose[b, a, 0] += max_error + 0.5 * (d[k - 1] + d[k])
            else:
                r = turned(k, per(bg["ko"], b), per(bg["kv"], b))
                th = max_error / np.sqrt(r[k - 1] * r[k])
                pose[b, a, 3:] = quat_mul(np.array([np.cos(th / 2), np.sin(th / 2), 0.0, 0.0]), tgt[b, ia, 3:])
    if shared is not None:
        pose = pose[:1].copy()
    desc = dict(n_actions=A, active_dev=ia, passive_dev=io, passive_hold_orientation=int(hold),
                passive_quat=np.array(aseq.DEFAULT_EE_QUAT if passive_quat is None else passive_quat, dtype=F64), pose=pose, **lst)
    for x in (q, qd, tgt, pose):
        x.setflags(write=False)
    _SHORT[key] = dict(q=q, qd=qd, tgt=tgt, desc=desc, cfg=cfg, stall=stall, late=np.array(late_rows, int))
    return _SHORT[key]


def assert_route(route, from_q, kernel):
    if route in trl.ROUTES:
        trl.assert_route(route, from_q, kernel)
    else:      # k13, k12_admit: the (1, 6, 6) lane tier on the layout's own kernel instantiation
        assert "fused" in from_q and "osc_lane" in from_q and "_rows_1_6_6 " in from_q and "row16" in kernel and "_pad" not in kernel, (from_q, kernel)


def assert_reference_conditions(ref, sc, coverage=True, finish=True):
    """`ref`: a host_loop result (state, entered, margin).  The module docstring's conditions (coverage: every action index is a final
    one; finish: a finisher in the last wave and every WP entered -- both off only where the one table of a fleet stalls all of it)."""
    desc = sc["desc"]
    A, B = desc["n_actions"], len(sc["q"])
    act = ref["state"]["action"]
    counts = np.bincount(act, minlength=A + 1)
    assert ref["margin"] >= 1e-9, ref["margin"]
    if coverage:
        assert counts.min() > 0, ("an action index is nobody's final action", counts)
    if not finish:
        return counts
    assert np.any(np.nonzero(act == A)[0] // 64 == (B - 1) // 64), "no finisher in the last wave"
    wps = np.nonzero(desc["kind"] == WP)[0]
    assert ref["entered"][:, wps].any(axis=0).all(), ("a WP nobody entered", ref["entered"].sum(axis=0))
    return counts


def assert_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(a[key][rows_a], b[key][rows_b]), key


# ---- 1. host loop = device list, bit for bit, per layout and role -------------------------------------------------------------------
# route: the key of assert_route; the rest: short_scenario's and the helpers' parameters
CASES = {
    "k13_swapped": dict(route="k13", cfg="k13", active=1, passive=0),
    "k13_quat": dict(route="k13", cfg="k13", active=0, passive=1, hold=0, passive_quat=QUAT),
    "k13_base_passive": dict(route="k13", cfg="k13", active=0, passive=2),
    "br7": dict(route="br7", cfg="br7", active=1, passive=0, hold=0, passive_quat="near_base"),
    "rlbr10": dict(route="rlbr10", cfg="rlbr10", B=101, active=3, passive=1, user_targets=True),
    "rlb16_f32": dict(route="rlb16", cfg="rlb16", dtype=F32, B=192, active=0, passive=1),
    "k7": dict(route="k7", cfg="k7", active=0, passive=1),
    "rlb11_branch_b": dict(route="rlb11_branch_b", cfg="rlb11_branch_b", active=1, passive=2, tgt_vel=True),
    "k12_admit_feed": dict(route="k12_admit", cfg="k12_admit", active=0, passive=1, feed=True),
    "k13_shared_near": dict(route="k13", cfg="k13", active=0, passive=1, shared=-1),
    "k13_shared_far_at_2": dict(route="k13", cfg="k13", active=0, passive=1, shared=2),
    "k13_wide": dict(route="k13", cfg="k13", active=0, passive=1, max_batch=192),
    "k13_per_instance": dict(route="k13", cfg="k13", active=0, passive=1, per_instance=True),
    "k13": dict(route="k13", cfg="k13", active=0, passive=1),      # (the standard list on the description of test_action_list.py: part 3's solo run)
}
NS = 18      # the scene's <sensor> block (BatchedOSC.set_ft_sensors)


def case_inputs(name):
    """-> (sc, dtype, kw of host_loop, kw of device_list) of a case."""
    c = CASES[name]
    B, cfg, dtype = c.get("B", 130), c["cfg"], c.get("dtype", F64)
    rng = np.random.default_rng(77)
    gains = synth.make_batch(cfg, B, seed=3, per_instance_gains=True)[1] if c.get("per_instance") else None
    pq = c.get("passive_quat")
    if isinstance(pq, str):      # the base's own orientation turned by 0.01 rad about a skew axis: the stand barely moves, and every word differs
        own = tal.ee_start(tal.start_state(1, np.random.default_rng(0))[0], np.zeros((1, 25)), cfg)[0, c["passive"], 3:]
        ax = np.array([0.36, 0.48, 0.8])
        pq = quat_mul(np.concatenate([[np.cos(0.005)], np.sin(0.005) * ax]), own)
    sc = short_scenario(B, cfg, c["active"], c["passive"], c.get("hold", 1), pq, shared=c.get("shared"), gains=gains)
    hk, dk = dict(gains=gains), dict(gains=gains, max_batch=c.get("max_batch"))
    nd = synth.make_layout(cfg).ndev
    if c.get("user_targets"):      # the devices the list never writes hold values of the user's: 0.1 mm off the EE position, and one word -0.0
        tgt = np.array(sc["tgt"])
        for d in set(range(nd)) - {c["active"], c["passive"]}:
            tgt[:, d, :3] += rng.uniform(-1e-4, 1e-4, (B, 3))
            tgt[:, d, 3:] *= 1.0 + rng.uniform(0.1, 0.5, (B, 1))      # (a target quaternion need not be a unit one: calc_error normalises it)
        tgt[:, 2, 5] = -0.0
        assert np.all(np.signbit(tgt[:, 2, 5])) and not np.array_equal(tgt[:, 0], tgt[:, 3])
        sc = dict(sc, tgt=tgt)
    if c.get("tgt_vel"):
        tv = 0.1 * synth.make_batch(cfg, B, seed=21)[2]["tgt_vel"]
        tv[sc["late"]] = 0.0      # (the ladder's law is branch A's)
        hk["tgt_vel"] = dk["tgt_vel"] = tv.astype(dtype)
    if c.get("feed"):
        sd = np.random.default_rng(43).normal(0.0, 5.0, size=(B, NS))
        sd[sc["late"]] = 0.0      # (the ladder's law knows no wrench)
        hk["feed"] = dk["feed"] = sd
    if c.get("max_batch"):      # the slot's targets cover the context's capacity, the list the scenario's robots
        more = np.array(sc["tgt"][::-1][:c["max_batch"] - B])
        more[:, :, :3] += 0.01
        dk["tgt"] = np.concatenate([sc["tgt"], more])
    return sc, dtype, hk, dk


def standard():
    """The standard list on k13, active 0, passive 1, B = 130: the scenario of parts 2 to 4."""
    return case_inputs("k13")[0]


_HOST, _DEV = {}, {}


def host_run(name):
    if name not in _HOST:
        sc, dtype, hk, dk = case_inputs(name)
        _HOST[name] = tal.host_loop(sc, dtype, T, **hk)
    return _HOST[name]


def dev_run(name, pieces=(T,)):
    if (name, pieces) not in _DEV:
        sc, dtype, hk, dk = case_inputs(name)
        _DEV[(name, pieces)] = tal.device_list(sc, dtype, pieces, **dk)
    return _DEV[(name, pieces)]


@pytest.mark.parametrize("name", [n for n in CASES if n != "k13"])
def test_host_loop_equals_device_list_per_layout_and_role(name):
    """T x (set_gains per instance, set_targets, rollout(1), action_list_tick) = rollout(5) + rollout(11) with the list, with a fixed
    speed (the limit does not follow err's last bits): qpos / qvel / u bit-equal, action / finished_tick / grip_left / gripper_force and
    flags_any equal, the route and the reference-side conditions asserted.  The standard list WP GRIP(3) WP GRIP(1) GRIP(2)
    WP('start_pos'), B = 130 unless stated:
      k13_swapped        active 1 (ur5left), passive 0: both eetab rows swapped
      k13_quat           hold = 0, passive_quat (0.5, -0.5, 0.5, 0.5): the branch that writes the description's quaternion
      k13_base_passive   the passive device is the base (device 2)
      br7                the base first: active 1, passive 0 = the base, hold = 0 with the base's own orientation turned by 0.01 rad (the
                         quaternion of k13_quat would turn the stand by radians within the test and carry every arm off its near poses)
      rlbr10             B = 101, ndev = 4: active 3 (the second ur5right block, orientation rows only: the late poses are turned, not
                         shifted), passive 1; devices 0 and 2 hold targets of the user's, a -0.0 among them, that must come back bit for bit
      rlb16_f32          B = 192 (no ragged wave), float32: the padded row16 FROMQ kernel behind per-robot gains, a float tile
      k7                 the (1, 3, 3) lane tier
      rlb11_branch_b     active 1, passive 2; target velocities on the slot (0.1 x synth.make_batch's): branch B asserted
      k12_admit_feed     a constant sensor feed N(0, 5) on the slot: the wrench kernel between the walk and the action kernel; u differs
                         from the same run without the feed
      k13_shared_*       nb = 1 at B = 130: every robot has the same table, so a stall is the list's, not a robot's -- one run with every
                         pose near (all finish), one with the far pose at action 2 (all end there): 'every action is a final action'
                         cannot hold within one run and is left out; the two runs together cover a finish and a stall
      k13_wide           the device context has max_batch = 192 and targets for 192 robots; upload and list over 130
      k13_per_instance   context gains per instance: the list's copy takes robot b's record, the host loop replaces word 9 only"""
    c = CASES[name]
    sc, dtype, hk, dk = case_inputs(name)
    host, dev = host_run(name), dev_run(name, PIECES)
    assert_route(c["route"], dev["from_q_name"], dev["kernel_name"])
    counts = assert_reference_conditions(host, sc, coverage=c.get("shared") is None, finish=c.get("shared", -1) < 0)
    print(f"[{name}] {dev['from_q_name']}; final actions {counts.tolist()}, finished_tick of finishers "
          f"{sorted(set(host['state']['finished_tick'][host['state']['action'] == sc['desc']['n_actions']].tolist()))}, closest |err - max_error| "
          f"{host['margin']:.3g}")
    if c.get("shared") is not None:
        assert counts[sc["desc"]["n_actions"] if c["shared"] < 0 else c["shared"]] == len(sc["q"])
    if c.get("tgt_vel"):
        trl.assert_branch_b(name, host["flags"])
    if c.get("feed"):      # the feed reaches u: the same run without it differs, on the robots that have a reading
        bare = tal.device_list(sc, dtype, PIECES, **dict(dk, feed=None))
        fed = np.any(hk["feed"] != 0, axis=1)
        assert fed.sum() >= 100 and np.all(np.any(bare["out"]["u"][fed] != dev["out"]["u"][fed], axis=1))
    tal.assert_discrete_equal(dev, host, T)
    assert_bits(dev["out"], host["out"])
    assert np.abs(host["out"]["u"]).max() > 0 and not np.array_equal(host["tgt"], np.asarray(sc["tgt"], dtype=dtype))


# ---- 2. list shapes against the NumPy restatement on the traced EE poses ------------------------------------------------------------
def replay(sc, dev, ticks, gains=None):
    """action_list_tick over the device's own EE trace.  -> state, tgt, gains (as a float64 context stores them), margin, entered,
    regimes: per tick the (robot, kp err) pairs of the robots whose limit was set from a finite err."""
    desc, B = sc["desc"], len(sc["q"])
    lay = synth.make_layout(sc["cfg"])
    state, tgt, g = aseq.action_list_state(B), np.array(sc["tgt"]), tal.packed_gains(lay, sc["cfg"], B, F64, gains)
    margin, entered, finite = np.inf, np.zeros((B, desc["n_actions"]), bool), []
    A = desc["n_actions"]
    for t in range(ticks):
        ee = dev["trace"][t]
        if t > 0:
            before = state["action"]
            wp = np.nonzero((before < A) & (desc["kind"][np.minimum(before, A - 1)] == WP))[0]
            margin = min(margin, np.abs(tal.judged_err(ee, tgt, desc)[wp] - desc["max_error"][before[wp]]).min(initial=np.inf))
        aseq.action_list_tick(state, ee, tgt, g, desc, t)
        live = np.nonzero(state["action"] < A)[0]
        entered[live, state["action"][live]] = True
        inwp = live[(desc["kind"][state["action"][live]] == WP) & np.isfinite(state["err"][live])]
        finite.append((inwp, desc["kp"][state["action"][inwp]] * state["err"][inwp]))
    return dict(state=state, tgt=tgt, gains=g, margin=margin, entered=entered, finite=finite)


def assert_replay(sc, ticks, coverage=False):
    """rollout(ticks - 1) + rollout(1) with the list and the EE trace against the restatement on that trace: discrete state equal, err
    within 1e-12, max_vel0 within kp x 1e-12; the last tick's qpos / qvel / u bit-equal to a slot WITHOUT a list that is given the
    restatement's targets and gains by hand for that tick (the limit: the device's own max_vel0, for its last bits).  -> (dev, rep)"""
    desc, B = sc["desc"], len(sc["q"])
    dev = tal.device_list(sc, F64, (ticks - 1, 1) if ticks > 1 else (1,), trace=True)
    assert_route("k13", dev["from_q_name"], dev["kernel_name"])
    rep = replay(sc, dev, ticks)
    st, ds = rep["state"], dev["state"]
    for key in ("action", "grip_left", "finished_tick", "gripper_force"):
        assert np.array_equal(ds[key], st[key]), key
    both = np.isfinite(st["err"])
    assert np.array_equal(np.isfinite(ds["err"]), both) and np.all(ds["err"][~both] == st["err"][~both])
    assert np.abs(ds["err"][both] - st["err"][both]).max(initial=0.0) <= 1e-12
    assert np.all(np.abs(ds["max_vel0"] - st["max_vel0"]) <= desc["kp"].max() * 1e-12) and np.all((ds["max_vel0"] == 0) == (st["max_vel0"] == 0))
    assert rep["margin"] >= 1e-9, rep["margin"]
    assert rep["entered"][:, desc["kind"] == WP].any(axis=0).all(), ("a WP nobody entered", rep["entered"].sum(axis=0))
    if coverage:
        assert_reference_conditions(rep, sc)
    # the last tick by hand
    ia = desc["active_dev"]
    g = rep["gains"].copy()
    g[:, ia, 9] = np.where(ds["max_vel0"] > 0, ds["max_vel0"], g[:, ia, 9])
    bg = tal.base_gains(sc["cfg"])
    hand = tal.make_ctx(B, F64, cfg=sc["cfg"])
    hand.set_gains(bg["kp"], bg["kv"], bg["ko"], bg["k"], bg["d"], g[:, :, 9:11], bg["null_kv"])
    q, qd = (dev["outs"][-2]["qpos"], dev["outs"][-2]["qvel"]) if ticks > 1 else (sc["q"], sc["qd"])
    hand.upload_q(q, qd)
    hand.set_targets(rep["tgt"])
    h = hand.rollout(1)
    hand.close()
    assert_bits(dev["out"], h)
    assert np.array_equal(dev["out"]["flags_any"], h["flags_any"])
    return dev, rep


def test_a_list_that_starts_with_a_grip_leaves_tick_0_alone():
    """GRIP(2) WP GRIP(1): tick 0 enters a GRIP -- no target is written, no limit, word 9 stays the context's: rollout(1) equals a slot
    without a list bit for bit (flags_any too).  Then 8 ticks against the restatement; GRIP is the last action too: robots finish by
    a count, on tick 4 (asserted: some do, the last robot of the ragged wave among them)."""
    B = 130
    sc = short_scenario(B, actions=(G(2), W, G(1)), late=())
    one = tal.device_list(sc, F64, (1,))
    plain = tal.make_ctx(B, F64)
    tal.fill(plain, sc)
    p = plain.rollout(1)
    plain.close()
    assert_bits(one["out"], p)
    assert np.array_equal(one["flags"], p["flags_any"])
    assert np.all(one["state"]["action"] == 0) and np.all(one["state"]["grip_left"] == 2) and np.all(one["state"]["max_vel0"] == 0)
    dev, rep = assert_replay(sc, 8)
    fin = rep["state"]["finished_tick"]
    assert set(fin[fin >= 0]) == {4} and fin[B - 1] == 4 and np.any(rep["state"]["action"] == 1), np.bincount(rep["state"]["action"])
    assert not np.array_equal(rep["tgt"], sc["tgt"])


@pytest.mark.parametrize("from_start", [0, 1])
def test_a_list_of_one_waypoint(from_start):
    """A = 1, a single WP; then with xyz_from_start on that action 0: the tick-0 path that takes the target's xyz from this tick's EE
    pose itself.  Every other robot stalls (A + 1 = 2 classes); with from_start the far pose is far by its orientation alone."""
    sc = short_scenario(130, actions=((WS if from_start else W),), late=())
    dev, rep = assert_replay(sc, 4)
    act = rep["state"]["action"]
    assert np.bincount(act, minlength=2).min() > 0 and act[129] == 1 and set(rep["state"]["finished_tick"][act == 1]) == {1}
    if from_start:
        assert np.array_equal(rep["tgt"][:, 0, :3], dev["trace"][0][:, 0, :3])


def test_a_list_of_32_actions():
    """A = 32 = IRLOSC_MAX_ACTIONS, the largest by-value argument block: WP (near) and GRIP(1) alternating, T = 48; a robot stalls at its
    action b mod 33 (counted from the last robot), and every robot that never stalls finishes -- on tick 32."""
    sc = short_scenario(130, actions=(W, G(1)) * 16, late=())
    dev, rep = assert_replay(sc, 48)
    st = rep["state"]
    never = sc["stall"] == 32
    assert never.sum() >= 3 and never[129] and np.all(st["action"][never] == 32) and set(st["finished_tick"][never]) == {32}
    assert len(set(st["action"])) >= 17 and rep["entered"][:, ::2].any(axis=0).all()


CLIPS = {"min_bites": ((0.01, 3.0), 1.0), "between": ((1e-5, 3.0), 1.0), "max_bites": ((1e-5, 1e-4), 1.0), "kp_zero": ((0.01, 3.0), 0.0)}


@pytest.mark.parametrize("regime", list(CLIPS))
def test_clip_regimes_of_the_velocity_limit(regime):
    """One WP whose clip range is a range.  The near robots must STAY in the WP for their limit to come from a finite err, so max_error
    is 1e-4 here (near err is about 2e-3) and every third robot's pose is its EE pose at the start itself: those finish on tick 1.  With
    kp = 1: (0.01, 3.0) min_speed bites for the near robots; (1e-5, 3.0) the limit is kp err; (1e-5, 1e-4) max_speed bites; kp = 0: kp err
    is 0 (NaN on the tick the WP is entered, err = +inf: both sides then take max_speed) and min_speed bites.  Each regime is asserted to
    occur on the restatement, for near robots."""
    (lo, hi), kp = CLIPS[regime]
    sc = short_scenario(130, actions=(W,), late=(), speed=(lo, hi), kp=kp, max_error=1e-4, exact_every=3)
    dev, rep = assert_replay(sc, 4)
    rows, v = rep["finite"][-1]
    near = np.isin(rows, np.nonzero(sc["stall"] == 1)[0]) & (rows % 3 != 0)
    assert near.sum() >= 20 and np.all(rep["state"]["action"][::3] == 1) and np.all(rep["state"]["action"][rows[near]] == 0)
    m = rep["state"]["max_vel0"][rows[near]]
    if regime in ("min_bites", "kp_zero"):
        assert np.all(v[near] < lo) and np.all(m == lo) and (kp == 0) == np.all(v[near] == 0)
    elif regime == "between":
        assert np.all((v[near] > lo) & (v[near] < hi)) and np.array_equal(m, v[near]) and len(set(m)) == near.sum()
    else:
        assert np.all(v[near] > hi) and np.all(m == hi)


def test_the_standard_list_against_the_restatement_and_start_pos_in_a_later_call():
    """The standard list, 16 ticks, against the restatement (with the reference-side conditions on it); and rollout(5) + rollout(11) -- the
    'start_pos' WP is entered on tick 8, in the second call, which reloads start_xyz from the state -- equals one rollout(16) bit for bit,
    state included."""
    sc = standard()
    dev, rep = assert_replay(sc, T, coverage=True)
    assert rep["entered"][:, 5].any() and np.all(rep["tgt"][rep["entered"][:, 5], 0, :3] == sc["tgt"][rep["entered"][:, 5], 0, :3])
    whole, parts = dev_run("k13", (T,)), dev_run("k13", PIECES)
    assert_bits(whole["out"], parts["out"])
    assert_bits(whole["out"], dev["out"])
    assert np.array_equal(whole["flags"], parts["flags"])
    for key in whole["state"]:
        assert np.array_equal(whole["state"][key], parts["state"][key]), key


# ---- 3. slots and re-setting --------------------------------------------------------------------------------------------------------
def test_two_slots_with_different_lists_interleaved():
    """One context, two slots: slot 0 the standard list with active 0 / passive 1, slot 1 the list of k13_swapped (active 1 / passive 0,
    other tables); rollout(3) calls alternate between them up to 16 ticks each.  Each slot equals its solo run bit for bit, state
    included."""
    B = 130
    scs = [case_inputs("k13")[0], case_inputs("k13_swapped")[0]]
    osc = tal.make_ctx(B, F64, n_slots=2)
    for slot, sc in enumerate(scs):
        tal.fill(osc, sc, slot)
        osc.set_action_list(sc["desc"], slot=slot)
    flags = [np.zeros(B, np.uint32), np.zeros(B, np.uint32)]
    for p in (3, 3, 3, 3, 3, 1):
        outs = []
        for slot in (0, 1):
            outs.append(osc.rollout(p, slot=slot))
            flags[slot] |= outs[slot]["flags_any"]
    states = [osc.action_state(0), osc.action_state(1)]
    assert_route("k13", osc.from_q_name, osc.kernel_name)
    osc.close()
    for slot, name in enumerate(("k13", "k13_swapped")):
        solo = dev_run(name, (T,))
        assert_bits(outs[slot], solo["out"])
        assert np.array_equal(flags[slot], solo["flags"])
        for key in solo["state"]:
            assert np.array_equal(states[slot][key], solo["state"][key]), (slot, key)
    assert not np.array_equal(outs[0]["qpos"], outs[1]["qpos"])


def test_setting_the_list_again_midway_starts_it_over():
    """rollout(7), then set_action_list again on the same slot: the state is action_list_state's (tick base 0 with it), and a following
    rollout(9) equals a fresh context started from the coordinates the slot then holds (downloaded) and its targets -- which no entry
    point downloads: they are the restatement's on the traced EE poses of the 7 ticks, which a float64 context stores as they are --
    bit for bit, state included: start_xyz is taken again, the tick base is 0 again."""
    B = 130
    sc = standard()
    desc = sc["desc"]
    osc = tal.make_ctx(B, F64)
    tal.fill(osc, sc)
    osc.set_action_list(desc)
    first = osc.rollout(7, trace_every=1)
    mid = osc.action_state()
    rep = replay(sc, dict(trace=first["ee_trace"]), 7)
    for key in ("action", "grip_left", "finished_tick", "gripper_force"):
        assert np.array_equal(mid[key], rep["state"][key]), key
    assert mid["action"].max() >= 3 and rep["margin"] >= 1e-9
    osc.set_action_list(desc)
    reset, init = osc.action_state(), aseq.action_list_state(B)
    for key in reset:
        assert np.array_equal(reset[key], init[key]), key
    q7, qd7 = osc.download_q()
    assert np.array_equal(q7, first["qpos"])
    again = osc.rollout(9)
    st = osc.action_state()
    assert_route("k13", osc.from_q_name, osc.kernel_name)
    osc.close()
    fresh = tal.device_list(dict(sc, q=q7, qd=qd7, tgt=rep["tgt"]), F64, (9,))
    assert_bits(again, fresh["out"])
    assert np.array_equal(again["flags_any"], fresh["flags"])
    for key in st:
        assert np.array_equal(st[key], fresh["state"][key]), key
    assert np.any(st["action"] == 5) and np.any(st["action"] == 0) and not np.array_equal(rep["tgt"], sc["tgt"])      # (tick 8 enters the last WP)


# ---- 4. rollouts narrower than the list ---------------------------------------------------------------------------------------------
def test_a_robot_that_narrower_rollouts_left_out_starts_its_list_on_its_first_tick():
    """The list for 130 robots; irlosc_rollout_from_q over 64 robots for 3 ticks, then over 130 for 13 (a rollout leaves the slot with the
    coordinates of the robots it ran, so the 66 others' are uploaded again in between: uploads leave the list alone).  A robot's list starts on the first
    tick that runs it: robots 64 .. 129 meet theirs on the slot's tick 3 -- not judged there, start_xyz taken, action 0 entered -- and
    equal, bit for bit, a 66-robot context that ran 13 ticks of the same list, the state too, finished_tick offset by 3 (it counts the
    slot's ticks); robots 0 .. 63 equal a 64-robot context after 16 ticks.  Asserted on the two plain contexts: robots of either half
    finish, stall, and enter the 'start_pos' WP (action 5: a start_xyz still (0, 0, 0) would aim it at the origin)."""
    B, H, EARLY = 130, 64, 3
    sc = standard()
    desc = sc["desc"]
    A = desc["n_actions"]
    osc = tal.make_ctx(B, F64)
    tal.fill(osc, sc)
    osc.set_action_list(desc)
    u, fl = np.empty((H, 25)), np.empty(H, np.uint32)
    osc._chk(osc.lib.irlosc_rollout_from_q(osc._h, 0, H, EARLY, 0, None, _lib.ptr(u), _lib.ptr(fl)))
    qh, qdh = np.empty((H, 25)), np.empty((H, 25))      # (the slot keeps coordinates of the 64 robots it ran: the others' go in again)
    osc._chk(osc.lib.irlosc_download_q(osc._h, 0, H, _lib.ptr(qh), _lib.ptr(qdh)))
    osc.upload_q(np.concatenate([qh, sc["q"][H:]]), np.concatenate([qdh, sc["qd"][H:]]))
    out = osc.rollout(T - EARLY)
    st = osc.action_state()
    assert_route("k13", osc.from_q_name, osc.kernel_name)
    osc.close()
    early, late = tal.device_list(sc, F64, (T,), rows=slice(0, H)), tal.device_list(sc, F64, (T - EARLY,), rows=slice(H, B))
    for ref in (early, late):
        a = ref["state"]["action"]
        assert np.any(a == A) and np.any(a < A) and np.any(a == 5) and np.any(ref["state"]["finished_tick"] == 9)
    assert_bits(out, late["out"], slice(H, B))
    assert_bits(out, early["out"], slice(0, H))
    assert np.array_equal(out["flags_any"][H:], late["flags"])
    for key in st:
        assert np.array_equal(st[key][:H], early["state"][key]), key
        want = late["state"][key]
        if key == "finished_tick":
            want = np.where(want >= 0, want + EARLY, -1)
        assert np.array_equal(st[key][H:], want), key
