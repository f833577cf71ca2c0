"""The motion of an action list on the GPU (-m gpu): irlosc_set_action_motion / irlosc_download_action_motion_state -- the action
kernel's MOTION form (csrc/osc_action.hpp, csrc/osc_rng.hpp) held bit for bit to its NumPy mirror (action_motion.action_motion_tick)
at a WP's entry and tick by tick through the log's TARGETS channel, to the plain list where steps = 1 and no noise make it one, to
itself in pieces, under other seeds, behind narrower rollouts and across episodes, to the host loop in closed loop, next to a robot
that holds a NaN, and the setter's rules.

B = 70: a full wave and a ragged one of 6 lanes.  The scenario is tests/test_action_list.py's (EE poses of perturbed joint
configurations as waypoints) with the list WP(noise), INTERP(noise), GRIP, WP('start_pos').

Closed loop against the host loop, measured on an MI355X (B = 70, scenario seed SEED_LOOP = 3, T = 467: the host loop's last finish
+ 2 ticks; finished_tick min 12, median 208, max 465; closest deciding |err - max_error| 1.21e-06):
    float64 context   max |qpos dev - host| 1.98e-14   max |qvel dev - host| 1.84e-13
    float32 context   0                                0        (the limit is stored as float32: err's last bits do not reach it)
-> BOUND_QPOS = 2e-13, BOUND_QVEL = 1.9e-12 (10 x, rounded up), both under the 1e-9 the bound may not exceed.  The seeds tried and
their margins: profiles/action_motion_rates.md."""
import ctypes as C

import numpy as np
import pytest

import test_action_list as tal
from irl_control_amd import _lib, objects as ob, synth
from irl_control_amd import action_motion as am
from irl_control_amd import action_sequence as aseq

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
ERR_ARG, ERR_STATE = tal.ERR_ARG, tal.ERR_STATE
WP, GRIP = tal.WP, tal.GRIP
B = 70
KINDS = (WP, WP, GRIP, WP)               # WP(noise), INTERP(noise), GRIP, WP('start_pos')
NOISE_STD = np.array([0.004, 0.002, 0.0, 0.0])
NOISE_MEAN = np.array([0.0, 0.001, 0.0, 0.0])
N_NOISY = 2
SEED = 2022
CHANNELS = ("qpos", "qvel", "ee_pose", "targets")
# context cases: (layout, dtype, IRLOSC_LANE, max_batch)
CASES = {"k13": ("k13", F64, None, None), "k13_f32": ("k13", F32, None, None), "r6_one_arm": ("r6", F64, None, None),
         "k13_fromq": ("k13", F64, "0", None), "k13_wide": ("k13", F64, None, 200)}
# closed loop (test_closed_loop_equals_the_host_loop): the scenario seed chosen so that the host loop's judgements keep 1e-6 from
# max_error (the search: profiles/action_motion_rates.md), and 10 x the deviation measured on an MI355X, not looser than 1e-9
SEED_LOOP = 3
BOUND_QPOS = 2e-13
BOUND_QVEL = 1.9e-12


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def the_list(max_error=tal.MAX_ERROR):
    A = len(KINDS)
    lo, hi = tal.SPEED_CLIP
    return dict(kind=np.array(KINDS, np.int32), xyz_from_start=np.array([0, 0, 0, 1], np.int32), grip_ticks=np.array([1, 1, tal.GRIP_TICKS, 1], np.int32),
                kp=np.full(A, tal.KP), max_error=np.array([max_error, max_error, 0.0, 1.5 * max_error]), min_speed=np.full(A, lo),
                max_speed=np.full(A, hi), gripper_force=np.array([0.0, 0.0, 0.2, -0.08]))


def scen(cfg="k13", seed=0, shared=False, perturb=tal.PERTURB):
    return tal.scenario(B, cfg=cfg, seed=seed, shared=shared, perturb=perturb, lst=the_list())


def the_motion(steps=(0, 7, 0, 0), seed=SEED, noise=True):
    return am.make_motion(len(KINDS), steps=steps, noise_mean=NOISE_MEAN if noise else None, noise_std=NOISE_STD if noise else None, seed=seed)


def flipped(sc, action):
    """The scenario's list with the goal quaternion of `action` negated for every odd robot: the same rotation, but its dot with the
    arm's orientation -- near the goal's: the waypoints are small perturbations of the start -- is negative."""
    pose = np.array(sc["desc"]["pose"])
    pose[1::2, action, 3:] *= -1.0
    return dict(sc["desc"], pose=pose)


def open_ctx(sc, dtype=F64, desc=None, motion=None, draw0=None, max_batch=None, q=None):
    osc = tal.make_ctx(B, dtype, cfg=sc["cfg"], max_batch=max_batch)
    osc.upload_q(sc["q"] if q is None else q, sc["qd"])
    osc.set_targets(sc["tgt"])
    osc.set_action_list(sc["desc"] if desc is None else desc)
    if motion is not None:
        osc.set_action_motion(motion, draw0=draw0)
    return osc


def run(sc, T, dtype=F64, desc=None, motion=None, draw0=None, max_batch=None, pieces=None, q=None, channels=CHANNELS):
    """One context, the list (and its motion) on slot 0, rollout_logged over `pieces` (default: T in one) -> dict(log: the pieces' logs
    joined, out: the last piece's result, action, motion: the states afterwards, tgt: download_targets)."""
    osc = open_ctx(sc, dtype, desc, motion, draw0, max_batch, q)
    outs = [osc.rollout_logged(p, channels) for p in (pieces or (T,))]
    res = dict(out=outs[-1], log={k: np.concatenate([o["log"][k] for o in outs]) for k in outs[0]["log"]}, action=osc.action_state(),
               motion=osc.action_motion_state() if motion is not None else None, tgt=osc.download_targets(),
               flags=np.bitwise_or.reduce([o["flags_any"] for o in outs]), from_q_name=osc.from_q_name)
    osc.close()
    return res


def replay(sc, desc, motion, ee_log, dtype, draw0=None, refs=None, obj_pose=None):
    """action_motion_tick over logged EE poses [T, B, ndev, 7] -> (targets per tick [T, B, ndev, 7] in dtype, list state, motion state
    per tick)"""
    nb = ee_log.shape[1]
    st = aseq.action_list_state(nb)
    m = dict(motion, state=am.action_motion_state(nb, draw0))
    tgt = np.array(sc["tgt"][:nb], dtype=dtype)
    tgts, mss = [], []
    for t in range(len(ee_log)):
        am.action_motion_tick(st, ee_log[t], tgt, None, desc, t, m, refs=refs, obj_pose=obj_pose)
        tgts.append(tgt.copy())
        mss.append({k: v.copy() for k, v in m["state"].items()})
    return np.array(tgts), st, mss


def assert_motion_state(got, want, rows=slice(None)):
    for k in ("step", "draws", "origin", "goal"):
        assert same_bits(got[k][rows], want[k][rows]), k


# ---- 1. the entry of a noisy WP -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("goal", ["table", "start_pos", "refs"])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_entry_of_a_noisy_wp(dtype, shared, goal):
    """A one-tick rollout of a list whose action 0 is a noisy WP, its goal from a per-robot or a shared table, from 'start_pos' or from
    refs on two objects: download_targets and action_motion_state equal the mirror bit for bit -- the goal in float64 with its noise,
    the target its rounding to the context's dtype, the origin this tick's EE pose, one draw used."""
    sc = scen(shared=shared)
    desc = dict(sc["desc"])
    ia = desc["active_dev"]
    refs = pose0 = None
    if goal == "start_pos":
        desc["xyz_from_start"] = np.array([1, 0, 0, 1], np.int32)
    osc = tal.make_ctx(B, dtype)
    osc.upload_q(sc["q"], sc["qd"])
    osc.set_targets(sc["tgt"])
    if goal == "refs":      # the table's xyz words as offsets on object 0, its quaternion words as a grip rotation on object 1
        rng = np.random.default_rng(11)
        desc["pose"] = np.array(desc["pose"])
        desc["pose"][:, 0, :3] = rng.uniform(-0.05, 0.05, (len(desc["pose"]), 3))
        pose0 = np.zeros((B, 2, 7))
        pose0[:, :, :3] = sc["tgt"][:, ia, None, :3] + rng.uniform(-0.1, 0.1, (B, 2, 3)) + [0.0, 0.0, 0.5]      # out of the hand's reach
        q4 = rng.normal(size=(B, 2, 4))
        pose0[:, :, 3:] = q4 / np.linalg.norm(q4, axis=2, keepdims=True)
        refs = dict(xyz_obj=np.array([0, -1, -1, -1], np.int32), quat_obj=np.array([1, -1, -1, -1], np.int32))
    osc.set_action_list(desc)
    if goal == "refs":
        osc.set_objects(ob.ObjectSet(radius=[0.03, 0.03], grippers=[ob.Gripper(dev=ia, joint=7, q_close=0.3, q_open=0.15)]), pose0)
        osc.set_action_refs(refs["xyz_obj"], refs["quat_obj"])
    motion = the_motion(steps=(0, 7, 0, 0))
    osc.set_action_motion(motion)
    out = osc.rollout(1, trace_every=1)
    got_tgt, got = osc.download_targets(), osc.action_motion_state()
    osc.close()
    tgts, st, mss = replay(sc, desc, motion, out["ee_trace"], dtype, refs=refs, obj_pose=pose0)
    assert same_bits(got_tgt, tgts[0])
    assert_motion_state(got, mss[0])
    assert np.all(got["draws"] == 1) and np.all(got["step"] == 0) and same_bits(got["origin"], out["ee_trace"][0][:, ia])
    assert same_bits(got_tgt[:, ia], got["goal"].astype(dtype))
    # not vacuous: the noise is there, robot by robot, and on xyz alone
    plain, _, _ = replay(sc, desc, the_motion(noise=False), out["ee_trace"], dtype, refs=refs, obj_pose=pose0)
    assert np.all(plain[0][:, ia, :3] != got_tgt[:, ia, :3]) and same_bits(plain[0][:, ia, 3:], got_tgt[:, ia, 3:])
    d = got["goal"][:, :3] - am.normal3(SEED, np.arange(B), 0, 0) * NOISE_STD[0]
    assert len(np.unique(got["goal"][:, 0] - d[:, 0])) == B


# ---- 2. INTERP tick by tick -------------------------------------------------------------------------------------------------------------
T_REPLAY = 500
_TICKS = {}


def tick_run(case):
    """The logged rollout of T_REPLAY ticks of case `case`, INTERPs of 7, 2 and 1 steps, action 0's goal quaternion on the far hemisphere
    for the odd robots; computed once per case."""
    if case not in _TICKS:
        cfg, dtype, lane, max_batch = CASES[case]
        mp = pytest.MonkeyPatch()
        if lane is not None:
            mp.setenv("IRLOSC_LANE", lane)
        try:
            sc = scen(cfg)
            desc = flipped(sc, 0)
            motion = am.make_motion(4, steps=[7, 2, 0, 1], noise_mean=NOISE_MEAN, noise_std=[0.004, 0.002, 0.0, 0.003], seed=SEED)
            _TICKS[case] = dict(run(sc, T_REPLAY, dtype, desc, motion, max_batch=max_batch), sc=sc, desc=desc, mot=motion, dtype=dtype)
        finally:
            mp.undo()
    return _TICKS[case]


@pytest.mark.parametrize("case", list(CASES))
def test_interp_tick_by_tick_through_the_log(case):
    """INTERPs of N = 7, 2 and 1 steps; the mirror, fed only the logged EE poses, reproduces the TARGETS channel of every tick and robot
    bit for bit -- the ticks on which step reaches N and the entries behind them included -- and the states afterwards.  Not vacuous:
    every robot is through the first INTERP and half of them through the list, the odd robots' first goal has a negative dot with their orientation and their
    targets stay on the near hemisphere until the goal itself is written."""
    r = tick_run(case)
    sc, desc, motion, dtype, log = r["sc"], r["desc"], r["mot"], r["dtype"], r["log"]
    ia = desc["active_dev"]
    if case == "k13_fromq":
        assert "osc_lane" not in r["from_q_name"] and "_fromq (fused" in r["from_q_name"], r["from_q_name"]
    tgts, st, mss = replay(sc, desc, motion, log["ee_pose"], dtype)
    assert log["targets"].dtype == dtype
    for t in range(T_REPLAY):
        assert same_bits(log["targets"][t], tgts[t]), (case, t, np.nonzero((log["targets"][t] != tgts[t]).any(axis=(1, 2)))[0])
    assert_motion_state(r["motion"], mss[-1])
    for k in ("action", "grip_left", "finished_tick", "gripper_force"):
        assert np.array_equal(r["action"][k], st[k]), k
    # not vacuous
    assert np.all(r["action"]["action"] >= 1) and (r["action"]["action"] == 4).sum() >= B // 2, np.bincount(r["action"]["action"], minlength=5)
    assert np.all(mss[6]["step"] == 7) and np.all(mss[5]["step"] == 6)
    odd = np.arange(B) % 2 == 1
    q0 = log["ee_pose"][0][:, ia, 3:]
    assert np.all(np.sum(q0 * desc["pose"][:, 0, 3:], axis=1)[odd] < 0) and np.all(np.sum(q0 * desc["pose"][:, 0, 3:], axis=1)[~odd] > 0)
    for t in range(6):
        assert np.all(np.sum(q0 * log["targets"][t][:, ia, 3:].astype(F64), axis=1) > 0)
        assert np.abs(np.linalg.norm(log["targets"][t][:, ia, 3:].astype(F64), axis=1) - 1).max() <= (1e-15 if dtype == F64 else 1e-7)
    assert same_bits(log["targets"][6][:, ia], mss[6]["goal"].astype(dtype))
    assert same_bits(mss[6]["goal"][:, 3:], desc["pose"][:, 0, 3:])      # as composed: the sign is not flipped
    if sc["cfg"] == "r6":
        assert desc["passive_dev"] == -1


# ---- 3. steps = 1 without noise is the list ------------------------------------------------------------------------------------------
def test_steps_1_without_noise_is_the_list_bit_for_bit():
    T = 400
    sc = scen()
    plain = run(sc, T)
    for steps in ([1, 1, 0, 1], [0, 0, 0, 0]):
        moved = run(sc, T, motion=the_motion(steps=steps, noise=False))
        for k in CHANNELS:
            assert same_bits(plain["log"][k], moved["log"][k]), (steps, k)
        for k in ("qpos", "qvel", "u"):
            assert same_bits(plain["out"][k], moved["out"][k]), (steps, k)
        for k in plain["action"]:
            assert same_bits(plain["action"][k], moved["action"][k]), (steps, k)
        assert np.all(moved["motion"]["draws"] == 0)
    assert plain["action"]["action"].max() == 4


# ---- 4. pieces ------------------------------------------------------------------------------------------------------------------------
def test_a_rollout_in_pieces_cut_inside_an_interp():
    T, N = 300, 50
    sc = scen()
    motion = the_motion(steps=(N, N, 0, N))
    whole = run(sc, T, motion=motion)
    parts = run(sc, T, motion=motion, pieces=(20, 1, T - 21))
    assert np.all(replay(sc, sc["desc"], motion, whole["log"]["ee_pose"][:21], F64)[2][20]["step"] == 21)      # the cuts fall inside action 0's INTERP
    for k in CHANNELS:
        assert same_bits(whole["log"][k], parts["log"][k]), k
    for k in ("qpos", "qvel", "u"):
        assert same_bits(whole["out"][k], parts["out"][k]), k
    assert_motion_state(whole["motion"], parts["motion"])
    for k in whole["action"]:
        assert same_bits(whole["action"][k], parts["action"][k]), k
    assert whole["action"]["action"].max() >= 1


# ---- 5. seeds and narrower rollouts ---------------------------------------------------------------------------------------------------
def test_seeds_and_a_rollout_over_fewer_robots():
    T = 60
    sc = scen()
    motion = the_motion()
    a, b = run(sc, T, motion=motion), run(sc, T, motion=motion)
    for k in CHANNELS:
        assert same_bits(a["log"][k], b["log"][k]), k
    assert_motion_state(a["motion"], b["motion"])
    c = run(sc, T, motion=the_motion(seed=SEED + 1))
    ia = sc["desc"]["active_dev"]
    assert np.all(c["log"]["targets"][0][:, ia, :3] != a["log"]["targets"][0][:, ia, :3])      # every noisy target, every word
    assert same_bits(c["log"]["targets"][0][:, ia, 3:], a["log"]["targets"][0][:, ia, 3:])
    # 5 ticks over the first 10 robots, then one over all 70: robots 10 .. 69 enter action 0 on the slot's tick 5 with the draws they
    # get on tick 0 of a rollout over all of them -- the counter holds the slot's index and the robot's own count of draws
    osc = open_ctx(sc, motion=motion)
    assert osc.lib.irlosc_rollout_from_q(osc._h, 0, 10, 5, 0, None, None, None) == 0
    qh, qdh = np.empty((10, 25)), np.empty((10, 25))      # (the slot keeps coordinates of the 10 robots it ran: the others' go in again)
    osc._chk(osc.lib.irlosc_download_q(osc._h, 0, 10, _lib.ptr(qh), _lib.ptr(qdh)))
    osc.upload_q(np.concatenate([qh, sc["q"][10:]]), np.concatenate([qdh, sc["qd"][10:]]))
    osc.rollout(1)
    late = osc.action_motion_state()
    osc.close()
    first = replay(sc, sc["desc"], motion, a["log"]["ee_pose"][:1], F64)[2][0]
    assert same_bits(late["goal"][10:], first["goal"][10:]) and np.all(late["draws"][10:] == 1) and np.all(late["draws"][:10] >= 1)
    assert same_bits(late["origin"][10:], first["origin"][10:])                                # (they have not moved: the same EE poses)


# ---- 6. episodes ----------------------------------------------------------------------------------------------------------------------
def test_a_second_episode_draws_fresh_noise_and_equals_a_fresh_rollout_from_its_draws():
    """max_episodes = 3: a robot's second episode -- ticks start .. start + length of the logged rollout -- equals, bit for bit in
    coordinates and targets, a fresh rollout whose draw0 is the draws its first episode used; its noisy targets differ from the first
    episode's, which started from the same state with the same table."""
    T = 1500
    sc = scen(perturb=0.03)
    motion = the_motion()
    ia = sc["desc"]["active_dev"]
    osc = open_ctx(sc, motion=motion)
    osc.set_episodes(sc["q"][:, None, :], max_episodes=3, records=4)
    ep = osc.rollout_logged(T, CHANNELS)
    es, ms = osc.episode_state(), osc.action_motion_state()
    osc.close()
    assert np.all(es["count"] >= 2), ("every robot ends two episodes within T", np.bincount(es["count"], minlength=4))
    rec = es["records"]
    assert np.all(rec[:, :2, 2] & _lib.EPISODE_FINISHED)
    assert np.array_equal(ms["draws"][es["count"] == 3], np.full((es["count"] == 3).sum(), 3 * N_NOISY))
    fresh = run(sc, int(rec[:, 1, 1].max()), motion=motion, draw0=np.full(B, N_NOISY, np.uint32))
    for b in range(B):
        s0, s1, n1 = int(rec[b, 0, 0]), int(rec[b, 1, 0]), int(rec[b, 1, 1])
        assert s0 == 0 and s1 == int(rec[b, 0, 1])
        for k in ("qpos", "qvel", "targets"):
            assert same_bits(ep["log"][k][s1:s1 + n1, b], fresh["log"][k][:n1, b]), (b, k)
        assert np.all(ep["log"]["targets"][s1, b, ia, :3] != ep["log"]["targets"][0, b, ia, :3])
        assert same_bits(ep["log"]["qpos"][s1, b], ep["log"]["qpos"][0, b])


# ---- 7. closed loop against the host loop ---------------------------------------------------------------------------------------------
def host_loop(sc, motion, dtype, T_max):
    """tests/test_action_list.py's host loop -- per tick set_gains per instance, set_targets, rollout(1) on a context of its own -- with
    action_motion_tick for the bookkeeping, until every robot has finished (+ 2 ticks) or T_max.  -> dict(T, qpos, qvel, state, mstate,
    margin: the smallest |err - max_error| over the judgements that decide -- a robot in a WP that jumps, or in an INTERP that has
    arrived --, trace: per tick every robot's action)."""
    cfg, desc = sc["cfg"], sc["desc"]
    q, qd = np.array(sc["q"]), np.array(sc["qd"])
    osc = tal.make_ctx(B, dtype, cfg=cfg)
    lay, bg = osc.layout, tal.base_gains(cfg)
    tgt = np.array(sc["tgt"], dtype=dtype)
    gains = tal.packed_gains(lay, cfg, B, dtype)
    state = aseq.action_list_state(B)
    m = dict(motion, state=am.action_motion_state(B))
    A, margin, trace, t = desc["n_actions"], np.inf, [], 0
    done_at = None
    while t < T_max and (done_at is None or t < done_at + 2):
        ee = tal.ee_start(q, qd, cfg)
        if t > 0:
            a0 = np.minimum(state["action"], A - 1)
            decides = (state["action"] < A) & (desc["kind"][a0] == WP) & ((motion["steps"][a0] == 0) | (m["state"]["step"] == motion["steps"][a0]))
            w = np.nonzero(decides)[0]
            margin = min(margin, np.abs(tal.judged_err(ee, tgt, desc)[w] - desc["max_error"][a0[w]]).min(initial=np.inf))
        am.action_motion_tick(state, ee, tgt, gains, desc, t, m)
        trace.append(state["action"].copy())
        if done_at is None and np.all(state["action"] == A):
            done_at = t
        osc.set_gains(bg["kp"], bg["kv"], bg["ko"], bg["k"], bg["d"], gains[:, :, 9:11].astype(F64), bg["null_kv"])
        osc.upload_q(q, qd)
        osc.set_targets(tgt)
        out = osc.rollout(1)
        q, qd = out["qpos"], out["qvel"]
        t += 1
    osc.close()
    return dict(T=t, qpos=q, qvel=qd, state=state, mstate=m["state"], margin=margin, trace=np.array(trace), done_at=done_at)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_closed_loop_equals_the_host_loop(dtype):
    """The list WP(noise), INTERP(noise, 7 steps), GRIP, WP('start_pos') for 70 robots: T x (set_gains per instance, set_targets,
    rollout(1)) with action_motion_tick on the host against one rollout(T) with the list and its motion.  Asserted on the host loop:
    every robot finishes within 1500 ticks and no deciding judgement comes within 1e-6 of max_error, for any robot.  Then finish ticks,
    action traces and the motion's state are equal for every robot, and qpos / qvel lie within BOUND_QPOS / BOUND_QVEL: 10 x the
    deviation first measured on an MI355X, never looser than 1e-9 (the limit follows err, whose last bits differ between the kernel
    and NumPy: one atan2 each).
    Measured (the module's docstring; printed by this test before it asserts): float64 max |qpos| 1.98e-14, max |qvel| 1.84e-13 after
    467 ticks, margin 1.21e-06; float32 0 and 0, margin 1.22e-06."""
    sc = scen(seed=SEED_LOOP)
    motion = the_motion()
    host = host_loop(sc, motion, dtype, 1500)
    A = sc["desc"]["n_actions"]
    ft = host["state"]["finished_tick"]
    print(f"\n[closed loop {np.dtype(dtype).name}] host loop: T {host['T']}, finished_tick min {ft.min()} median {np.median(ft):g} max {ft.max()}, "
          f"closest deciding |err - max_error| {host['margin']:.3g}")
    assert np.all(host["state"]["action"] == A), np.bincount(host["state"]["action"], minlength=A + 1)
    assert host["margin"] >= 1e-6, host["margin"]
    T = host["T"]
    dev = run(sc, T, dtype, motion=motion, channels=("targets",))
    dq, dv = np.abs(dev["out"]["qpos"] - host["qpos"]).max(), np.abs(dev["out"]["qvel"] - host["qvel"]).max()
    print(f"[closed loop {np.dtype(dtype).name}] device against host loop after {T} ticks: max |qpos| {dq:.3g}, max |qvel| {dv:.3g}")
    assert np.array_equal(dev["action"]["finished_tick"], ft) and len(set(ft)) >= 2
    for k in ("action", "grip_left", "gripper_force"):
        assert np.array_equal(dev["action"][k], host["state"][k]), k
    # the motion's state: steps, draws and goals (table + noise, 'start_pos': tick 0's EE position) bit for bit; the origin is the EE pose of
    # the tick a WP was entered on, a function of coordinates that differ at rounding level: inside the 1e-9 no bound here exceeds
    for k in ("step", "draws", "goal"):
        assert same_bits(dev["motion"][k], host["mstate"][k]), k
    assert np.abs(dev["motion"]["origin"] - host["mstate"]["origin"]).max() <= 1e-9
    assert np.all(dev["motion"]["draws"] == N_NOISY)
    assert dq <= BOUND_QPOS and dv <= BOUND_QVEL


def test_closed_loop_action_trace_equals_the_host_loops():
    """Per tick and robot the action the host loop is in against the device's, read from a logged rollout cut after every tick would
    cost T calls; instead the device's trace is rebuilt by the mirror from the device's own logged EE poses (test 2 holds that replay to
    the device bit for bit) and held against the host loop's trace."""
    sc = scen(seed=SEED_LOOP)
    motion = the_motion()
    host = host_loop(sc, motion, F64, 1500)
    dev = run(sc, host["T"], F64, motion=motion, channels=("ee_pose", "targets"))
    st = aseq.action_list_state(B)
    m = dict(motion, state=am.action_motion_state(B))
    tgt = np.array(sc["tgt"])
    for t in range(host["T"]):
        am.action_motion_tick(st, dev["log"]["ee_pose"][t], tgt, None, sc["desc"], t, m)
        assert same_bits(dev["log"]["targets"][t], tgt), t
        assert np.array_equal(st["action"], host["trace"][t]), t


# ---- 8. a robot with NaN --------------------------------------------------------------------------------------------------------------
def test_a_robot_with_nan_is_alone():
    T, bad = 150, 64 + 3
    sc = scen()
    motion = the_motion(steps=(5, 7, 0, 0))
    q = sc["q"].copy()
    q[bad, [0, 1, 13]] = np.nan
    clean, out = run(sc, T, motion=motion), run(sc, T, motion=motion, q=q)
    others = np.arange(B) != bad
    for k in CHANNELS:
        assert same_bits(out["log"][k][:, others], clean["log"][k][:, others]), k
    for k in ("qpos", "qvel", "u"):
        assert same_bits(out["out"][k][others], clean["out"][k][others]), k
    assert_motion_state(out["motion"], clean["motion"], others)
    for k in clean["action"]:
        assert same_bits(out["action"][k][others], clean["action"][k][others]), k
    assert clean["action"]["action"].max() >= 1
    assert out["action"]["action"][bad] == 0 and out["motion"]["step"][bad] == 5 and np.all(np.isnan(out["motion"]["origin"][bad]))


# ---- 9. the rules ---------------------------------------------------------------------------------------------------------------------
def test_rules():
    sc = scen()
    motion = the_motion()
    osc = open_ctx(sc)
    lib, h = osc.lib, osc._h

    def c_motion(steps=motion["steps"], mean=NOISE_MEAN, std=NOISE_STD, seed=SEED):
        m = _lib.ActionMotion()
        for a in range(len(steps)):
            m.steps[a], m.noise_mean[a], m.noise_std[a] = int(steps[a]), float(mean[a]), float(std[a])
        m.seed = seed
        return m

    def set_m(slot=0, **kw):
        return lib.irlosc_set_action_motion(h, slot, C.byref(c_motion(**kw)), None)

    def state_rc():
        return lib.irlosc_download_action_motion_state(h, 0, B, None, None, None, None)

    def vary(v, a, val):
        v = np.array(v, dtype=np.float64)
        v[a] = val
        return v

    assert state_rc() == ERR_STATE and "motion" in lib.irlosc_last_error(h).decode()      # a list without a motion
    assert set_m() == 0 and state_rc() == 0
    osc.rollout(12)
    before, tgt_before = osc.action_motion_state(), osc.download_targets()
    assert np.all(before["draws"] >= 1)
    bad = [dict(steps=vary(motion["steps"], 1, -1)), dict(steps=vary(motion["steps"], 0, (1 << 20) + 1)), dict(steps=vary(motion["steps"], 2, 3)),
           dict(mean=vary(NOISE_MEAN, 2, 0.001)), dict(std=vary(NOISE_STD, 2, 0.001)), dict(std=vary(NOISE_STD, 0, -0.001)),
           dict(std=vary(NOISE_STD, 1, np.inf)), dict(std=vary(NOISE_STD, 3, np.nan)), dict(mean=vary(NOISE_MEAN, 0, np.nan)),
           dict(mean=vary(NOISE_MEAN, 3, -np.inf)), dict(mean=vary(NOISE_MEAN, 2, np.nan))]
    for kw in bad:
        assert set_m(**kw) == ERR_ARG, (kw, lib.irlosc_last_error(h).decode())
    assert set_m(slot=5) == ERR_ARG
    assert set_m(steps=vary(motion["steps"], 0, 1 << 20)) == 0 and set_m() == 0            # (the largest steps is fine; and back)
    osc.close()
    # ... the motion in force stays whole behind every refusal: the rollout goes on as one that saw none
    osc = open_ctx(sc, motion=motion)
    osc.rollout(12)
    for kw in bad:
        assert lib.irlosc_set_action_motion(osc._h, 0, C.byref(c_motion(**kw)), None) == ERR_ARG
    assert_motion_state(osc.action_motion_state(), before)
    osc.rollout(30)
    after_refusals = osc.action_motion_state()
    osc.close()
    osc = open_ctx(sc, motion=motion)
    osc.rollout(42)
    assert_motion_state(osc.action_motion_state(), after_refusals)
    # IRLOSC_ERR_STATE on a slot without a list: set_action_list(None) ends list and motion; the motion of another slot stays
    lib, h = osc.lib, osc._h
    osc.set_action_list(None)
    assert lib.irlosc_set_action_motion(h, 0, C.byref(c_motion()), None) == ERR_STATE and "irlosc_set_action_list" in lib.irlosc_last_error(h).decode()
    assert lib.irlosc_download_action_motion_state(h, 0, B, None, None, None, None) == ERR_STATE
    # irlosc_set_action_list ends the motion: the list jumps again
    osc.upload_q(sc["q"], sc["qd"])
    osc.set_targets(sc["tgt"])
    osc.set_action_list(sc["desc"])
    assert lib.irlosc_download_action_motion_state(h, 0, B, None, None, None, None) == ERR_STATE
    plain = osc.rollout_logged(20, ("targets",))["log"]["targets"]
    # motion == NULL clears it, and nothing else: the list in force goes on, jumping
    osc.upload_q(sc["q"], sc["qd"])
    osc.set_targets(sc["tgt"])
    osc.set_action_list(sc["desc"])
    osc.set_action_motion(motion)
    assert lib.irlosc_download_action_motion_state(h, 0, B, None, None, None, None) == 0
    osc.set_action_motion(None)
    assert lib.irlosc_download_action_motion_state(h, 0, B, None, None, None, None) == ERR_STATE
    assert lib.irlosc_download_action_state(h, 0, B, None, None, None, None, None, None) == 0
    cleared = osc.rollout_logged(20, ("targets",))["log"]["targets"]
    assert same_bits(plain, cleared)
    # draw0 is taken
    osc.set_action_motion(motion, draw0=np.arange(B) * 3)
    assert np.array_equal(osc.action_motion_state()["draws"], np.arange(B) * 3) and np.all(osc.action_motion_state()["step"] == 0)
    osc.close()
