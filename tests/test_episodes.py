"""Episodes of a rollout (-m gpu): irlosc_set_episodes / irlosc_download_episode_state and the early exit, against the code that was
there before them.  Every robot's arithmetic is its own lane's, so episode e of robot b must equal, BIT FOR BIT, the first `length` ticks
of a fresh rollout of the entry points without episodes from start e mod S with variant e mod V.  The reference of every test is S x V
fresh logged rollouts, stitched by episodes.stitch along episodes.schedule (lengths from the fresh runs' own finished ticks), compared
with ONE long logged rollout with episodes; records and episode_state() against the schedule.  Fleets stay far below the eigen pass's
lane-form threshold (3000), so both runs take its row16 form.
Each test asserts its preconditions on the reference runs: the lengths differ inside wave 0, both outcomes occur, some robot ends three
episodes, the two robots of the ragged last wave differ."""
import numpy as np
import pytest

import test_action_list as tal
import test_joints as tjn
import test_rollout as tr
import test_teleop_stream as tts
import test_walls as twl
from irl_control_amd import _lib, episodes as ep, synth
from test_action_list_layouts import quat_mul

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
WP, GRIP = tal.WP, tal.GRIP
same_bits = tts.same_bits
B0, BMAX = 130, 192           # waves of 64, 64 and 2; a context whose stride differs from B
S, V = 2, 3                   # they do not divide each other: six (start, variant) pairs in turn
MAX_TICKS, T = 24, 100
RECORDS = 8
MAX_ERROR = 0.04              # of the list's WPs: wide, as the insertion example's
FAR = 0.05                    # m beyond max_error: out of reach of 24 ticks (the limit of 0.04 m/s covers 1 mm in them)
PATH_THR = 4e-4               # m, the paths' threshold
FRONT = ("qpos", "qvel", "ee_pose", "targets", "u", "flags")


# ---- the fleet: two start states and three pose variants per robot -----------------------------------------------------------------------
_FLEET = {}


def fleet(B, kinds=(WP, GRIP, WP), cfg="k13", active=None, passive=None, S=S, V=V):
    """-> dict(q, qd [B, S, 25]; tgt [B, ndev, 7]: the EE poses at start 0, the slot's targets; poses [V, B, A, 7]; desc: the list's
    description with variant 0's poses; cfg, ia, io: the layout and the list's active and passive device (default: k13's, by name); ee:
    the EE poses at start 0).  Start 1 is start 0 with the active arm moved by up to 2e-4 rad, the other arm elsewhere and small joint
    velocities.  A WP's pose is the active EE pose of start 0 moved along x by max_error + delta, delta accumulated over the
    list's WPs: < 0 (within max_error at once), log-uniform in [1e-6, 1e-3] m (the arm has to come that much closer: a few ticks to a
    timeout) or FAR (no chance).  The ragged wave's robots: 128 at once everywhere, 129 FAR in variant 0.
    A list that opens with a GRIP writes no target on its first ticks: there the slot's target of the active arm lies 5 cm beside its EE,
    so that the first OSC steps of an episode run into the velocity limit of the gain record -- word 9, which a reset must take back.
    Every arm of every layout has k13's gains (kp 200, kv 50, k_x 1: synth.make_batch), so the distances hold off k13; an active device
    WITHOUT xyz rows (rlbr10's block 3) gets its WP poses turned about x instead of shifted along it, by max_error + 4 delta: left to
    theta'' = -ko theta - kv theta' the angle shrinks by 1.7e-3 rad in 24 ticks where the limited arm covers 4.2e-4 m
    (test_action_list_layouts.turned / travel).  Start s >= 1 is start 0 perturbed as described, drawn anew per s; V = 0: no variants
    (poses is empty and desc holds variant 0's table)."""
    key = (B, tuple(kinds), cfg, active, passive, S, V)
    if key in _FLEET:
        return _FLEET[key]
    rng = np.random.default_rng(77)
    ia, io = tal.device_roles(cfg, active, passive)
    arm = tal.arm_joints(cfg, ia)
    other = tal.LEFT if arm == tal.RIGHT else tal.RIGHT
    q0, _ = tal.start_state(B, rng)
    q = np.stack([q0] * S, axis=1)
    qd = np.zeros_like(q)
    for s in range(1, S):
        q[:, s, arm] += rng.uniform(-2e-4, 2e-4, (B, 6))
        q[:, s, other] += rng.uniform(-0.1, 0.1, (B, 6))
        qd[:, s, arm] = rng.uniform(-0.01, 0.01, (B, 6))
    ee = tal.ee_start(q[:, 0], qd[:, 0], cfg)
    has_xyz = bool(np.any(synth.make_layout(cfg).ctrlr_dof[ia][:3]))
    tgt = ee.copy()
    if kinds[0] == GRIP:
        tgt[:, ia, 1] += 0.05
    A = len(kinds)
    poses = np.zeros((max(V, 1), B, A, 7))
    poses[..., 3] = 1.0
    for v in range(max(V, 1)):
        u = rng.uniform(size=(B, A))
        delta = np.where(u < 0.25, -0.01, np.where(u < 0.85, 10.0 ** rng.uniform(-6, -3, (B, A)), FAR))
        if B > 129:
            delta[128] = -0.01
            if v == 0:
                delta[129] = FAR
        acc = np.zeros(B)
        for a in range(A):
            if kinds[a] != WP:
                continue
            acc = acc + np.maximum(delta[:, a], 0.0) if a else np.maximum(delta[:, a], 0.0)
            poses[v, :, a] = ee[:, ia]
            if has_xyz:
                poses[v, :, a, 0] += MAX_ERROR + np.where(delta[:, a] < 0, delta[:, a], acc)
            else:
                th = MAX_ERROR + np.where(delta[:, a] < 0, delta[:, a], np.where(acc >= FAR, acc, 4.0 * acc))
                for b in range(B):
                    poses[v, b, a, 3:] = quat_mul(np.array([np.cos(th[b] / 2), np.sin(th[b] / 2), 0.0, 0.0]), ee[b, ia, 3:])
    variant0 = poses[0]
    poses = poses[:V]
    desc = dict(n_actions=A, active_dev=ia, passive_dev=io, passive_hold_orientation=1, passive_quat=np.array([1.0, 0, 0, 0]), pose=variant0,
                kind=np.array(kinds, np.int32), xyz_from_start=np.zeros(A, np.int32), grip_ticks=np.full(A, 2, np.int32), kp=np.full(A, tal.KP),
                max_error=np.full(A, MAX_ERROR), min_speed=np.full(A, tal.SPEED_CLIP[0]), max_speed=np.full(A, tal.SPEED_CLIP[1]),
                gripper_force=np.where(np.array(kinds) == GRIP, 0.2, 0.0))
    for a in (q, qd, tgt, poses, variant0, ee):
        a.setflags(write=False)
    _FLEET[key] = dict(q=q, qd=qd, tgt=tgt, poses=poses, desc=desc, B=B, cfg=cfg, ia=ia, io=io, ee=ee)
    return _FLEET[key]


def sub(fl, rows):
    """The fleet's robots `rows` as a fleet of their own."""
    return dict(fl, q=fl["q"][rows], qd=fl["qd"][rows], tgt=fl["tgt"][rows], ee=fl["ee"][rows], poses=np.ascontiguousarray(fl["poses"][:, rows]),
                desc=dict(fl["desc"], pose=np.ascontiguousarray(fl["desc"]["pose"][rows])), B=len(fl["q"][rows]))


def open_ctx(B, dtype=F64, feed=False, max_batch=BMAX, n_slots=1, cfg="k13", gains=None):
    return tal.make_ctx(B, dtype, n_slots=n_slots, max_batch=max(max_batch, B), feed=feed, cfg=cfg, gains=gains)


def open_for(fl, dtype, feed=False, max_batch=BMAX, n_slots=1):
    """The context of a fleet: its own opener where it brings one (fl["open"](capacity, dtype, feed, n_slots): another layout, with its
    route asserted; per-robot gains), else open_ctx on its layout."""
    cap = max(max_batch, fl["B"])
    if "open" in fl:
        return fl["open"](cap, dtype, feed, n_slots)
    return open_ctx(fl["B"], dtype, feed, cap, n_slots, cfg=fl.get("cfg", "k13"))


def start_of(fl, s):
    """(q, qd) [B, n] of start state s: the fleet's own row, or the one the fleet shares ([S, n] start states)."""
    q, qd = fl["q"], fl["qd"]
    if q.ndim == 2:
        return np.broadcast_to(q[s], (fl["B"], q.shape[1])), np.broadcast_to(qd[s], (fl["B"], q.shape[1]))
    return q[:, s], qd[:, s]


def set_slot_targets(osc, fl, slot=0):
    osc.set_targets(fl["tgt"], fl.get("tgt_vel"), slot=slot)


def arm_extras(osc, fl, extras, slot=0):
    """Feed, walls and joint rows of a case, their state and ticks reset (ahead of the program and the episodes)."""
    B = fl["B"]
    if "walls" in extras:
        osc.set_sensordata(np.random.default_rng(43).normal(0.0, 5.0, size=(B, tr.NS)), slot=slot)
        # per arm the plane x = the median of the fleet's EE x at start 0 shifted to where the moving arm crosses it within a few ticks
        # (a fleet off k13 names its walled devices and their normals)
        osc.set_walls(twl.median_walls(fl.get("wall_x", fl["tgt"])[:, :, :3], fl.get("wall_devs", (0, 1)), r=0.0005,
                                       normals=fl.get("wall_normals", (twl.N_X,))), slot=slot)
    if "joints" in extras:
        osc.set_joints(tjn.scene(osc.layout), slot=slot)


def arm_program(osc, fl, program, variant=0, slot=0):
    if program == "list":
        osc.set_action_list(dict(fl["desc"], pose=np.ascontiguousarray(fl["poses"][variant])) if len(fl["poses"]) else fl["desc"], slot=slot)
    elif program == "paths":
        paths, loop = paths_and_loops(fl)
        osc.set_waypoints(paths, PATH_THR, loop, slot=slot)


def paths_and_loops(fl):
    """The fleet's own (paths, loop flags per device) where it brings them, else paths_of's with every device but the active one looping."""
    if "paths" in fl:
        return fl["paths"], list(fl["loop"])
    return paths_of(fl), [d != fl["ia"] for d in range(fl["tgt"].shape[1])]


def paths_of(fl):
    """Paths for PATHS cases: the right arm (not looping) walks three waypoints along x: the first where it starts, the second the
    threshold + need1 away from there, the third need2 beyond the second -- need1 < 0 (it has arrived when it sets out), log-uniform
    in [1e-7, 2e-5] m (from rest the arm covers about 1.5e-5 m in 24 ticks: a few ticks to a timeout) or FAR; need2 log-uniform in
    [1e-7, 5e-6] m --; the other arm loops over two; the stand keeps its target."""
    ia, io = fl["ia"], fl["io"]
    B = fl["B"]
    rng = np.random.default_rng(78)
    u = rng.uniform(size=B)
    need1 = np.where(u < 0.2, -1e-4, np.where(u < 0.8, 10.0 ** rng.uniform(-7, -4.7, B), FAR))
    need2 = 10.0 ** rng.uniform(-7, -5.3, B)
    ex = np.array([1.0, 0.0, 0.0])
    xa = fl["tgt"][:, ia, :3]
    out = [None] * fl["tgt"].shape[1]
    out[ia] = np.stack([xa, xa + (PATH_THR + need1)[:, None] * ex, xa + (PATH_THR + need1 + need2)[:, None] * ex], axis=1)
    if io >= 0:      # (a layout of one device has no other arm)
        xo = fl["tgt"][:, io, :3]
        out[io] = np.stack([xo, xo + [0.0, 3e-4, 0.0]], axis=1)
    return out


def channels_of(extras):
    return list(FRONT) + (["wrench", "wall_force"] if "walls" in extras else []) + (["joint_tau"] if "joints" in extras else [])


def finish_ticks(osc, program, fl):
    """The tick of a fresh rollout that found each robot done (-1: not yet)."""
    if program == "list":
        return osc.action_state()["finished_tick"]
    if program == "paths":      # every listed device that does not loop is through: the tick of the last of their last arrivals
        paths, loop = paths_and_loops(fl)
        judges = [d for d, p in enumerate(paths) if p is not None and not loop[d]]
        if not judges:
            return np.full(fl["B"], -1)
        st = osc.waypoint_state()
        done = np.all([st["index"][:, d] == np.shape(paths[d])[-2] for d in judges], axis=0)
        return np.where(done, np.max([st["last_tick"][:, d] for d in judges], axis=0), -1)
    return np.full(fl["B"], -1)


_FRESH = {}


def fresh(fl, dtype, program="list", extras=(), ticks=T, max_ticks=MAX_TICKS, key=None, max_batch=BMAX, end_on_finish=True):
    """The reference: S x V fresh logged rollouts of `ticks` ticks WITHOUT episodes -- start s into the coordinates, the targets, the
    case's extras, the program with variant v -- every channel of the case.  -> dict(log: name -> [S, V, ticks, B, ...], lengths,
    outcomes [S, V, B]).  Computed once per key and never written to."""
    key = (key or fl["B"], np.dtype(dtype).name, program, tuple(extras), ticks, max_ticks, end_on_finish)
    if key in _FRESH:
        return _FRESH[key]
    ns = fl["q"].shape[-2]
    nv = max(1, len(fl["poses"])) if program == "list" else 1
    ch = channels_of(extras)
    osc = open_for(fl, dtype, feed="walls" in extras, max_batch=max_batch)
    logs = {n: [] for n in ch}
    fin = np.zeros((ns, nv, fl["B"]), np.int64)
    wps = [[None] * nv for _ in range(ns)]      # (PATHS: the cycler's state behind every fresh run)
    for s in range(ns):
        row = {n: [] for n in ch}
        for v in range(nv):
            osc.upload_q(*start_of(fl, s))
            set_slot_targets(osc, fl)
            arm_extras(osc, fl, extras)
            arm_program(osc, fl, program, v)
            r = osc.rollout_logged(ticks, ch)
            assert r["ticks_run"] == ticks
            fin[s, v] = finish_ticks(osc, program, fl)
            wps[s][v] = osc.waypoint_state() if program == "paths" else None
            for n in ch:
                row[n].append(r["log"][n])
        for n in ch:
            logs[n].append(np.stack(row[n]))
    osc.close()
    log = {n: np.stack(a) for n, a in logs.items()}
    lengths, outcomes = ep.lengths_from_finish(fin, max_ticks, end_on_finish)
    print(f"\n[fresh {key}] episode lengths of wave 0: {sorted(set(lengths[:, :, :64].ravel().tolist()))}; FINISHED {int((outcomes == ep.FINISHED).sum())}, "
          f"TIMEOUT {int((outcomes == ep.TIMEOUT).sum())} of {outcomes.size}")
    assert not np.any(log["flags"].astype(np.uint32) & tal_bad()), "a robot froze in a fresh run"
    for a in list(log.values()) + [lengths, outcomes]:
        a.setflags(write=False)
    _FRESH[key] = dict(log=log, lengths=lengths, outcomes=outcomes, channels=ch, finish=fin, wp_state=wps)
    return _FRESH[key]


def tal_bad():
    return np.uint32(_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD)


def assert_preconditions(ref, sched, B):
    """What makes the comparison worth its name, on the reference runs."""
    ln = ref["lengths"]
    lens0 = {r[1] for b in range(min(B, 64)) for r in sched["records"][b]}
    assert len(lens0) >= 3, f"wave 0 holds the episode lengths {sorted(lens0)} only"
    outs = {r[2] for rec in sched["records"] for r in rec}
    assert outs == {ep.FINISHED, ep.TIMEOUT}, outs
    assert sched["count"].max() >= 3
    assert sched["count"].max() > RECORDS, "no robot's ring of RECORDS entries wrapped"
    if B == B0:
        assert [r[:3] for r in sched["records"][128]] != [r[:3] for r in sched["records"][129]], "the last wave's two robots do not differ"
    assert ln.shape[2] == B


def run_with_episodes(fl, dtype, program, extras, ticks=T, pieces=None, max_episodes=0, poll_every=0, max_ticks=MAX_TICKS, logged=True,
                      end_on_finish=True, max_batch=BMAX, records=RECORDS):
    """One context: extras, program (variant 0), episodes, then the rollout(s).  -> (list of the pieces' results, episode_state, osc closed)."""
    osc = open_for(fl, dtype, feed="walls" in extras, max_batch=max_batch)
    osc.upload_q(*start_of(fl, fl["q"].shape[-2] - 1))      # (NOT start 0, where there is another: set_episodes has to write it)
    set_slot_targets(osc, fl)
    arm_extras(osc, fl, extras)
    arm_program(osc, fl, program, 0)
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=max_ticks, end_on_finish=end_on_finish, max_episodes=max_episodes,
                     poses=fl["poses"] if program == "list" and len(fl["poses"]) else None, records=records, poll_every=poll_every)
    outs = []
    for p in pieces or [ticks]:
        outs.append(osc.rollout_logged(p, channels_of(extras)) if logged else osc.rollout(p))
    st = osc.episode_state()
    more = dict(joint=osc.joint_state() if "joints" in extras else None, wall=osc.wall_state() if "walls" in extras else None)
    osc.close()
    return outs, st, more


def assert_equals_stitched(log, ref, sched, ticks=slice(None), rows=slice(None)):
    want = ep.stitch({n: ref["log"][n][:, :, :, rows] for n in ref["channels"]}, sched)
    for n in ref["channels"]:
        w = np.ascontiguousarray(want[n][ticks])
        assert log[n].dtype == w.dtype and log[n].shape == w.shape, n
        if not same_bits(log[n], w):
            bad = np.argwhere((tts.bits(log[n]) != tts.bits(w)).reshape(w.shape[0], w.shape[1], -1).any(axis=2))
            t, b = bad[0]
            raise AssertionError(f"{n}: {len(bad)} (tick, robot) pairs differ, the first at tick {t}, robot {b} (episode {sched['episode'][t, b]}, "
                                 f"age {sched['age'][t, b]}); max |diff| {np.nanmax(np.abs(log[n].astype(F64) - w.astype(F64))):.3e}")


def assert_state_is(st, sched, ticks, records=RECORDS):
    assert np.array_equal(st["count"], sched["count"])
    assert np.array_equal(st["age"], sched["age_end"])
    assert np.array_equal(st["start_tick"], sched["start_tick"])
    assert np.array_equal(st["records"], ep.ring(sched, records))
    assert st["running"] == int((sched["park_tick"] < 0).sum()) and st["ticks_run"] == ticks


# ---- 1. the list, the paths, no program; walls and joint rows ------------------------------------------------------------------------------
CASES = {
    "list": ("list", ()), "list_f32": ("list", ()), "paths": ("paths", ()), "none": ("none", ()),
    "list_walls": ("list", ("walls",)), "list_joints": ("list", ("joints",)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_episodes_equal_fresh_rollouts(case):
    """B = 130 in a context of 192, S = 2, V = 3, max_ticks 24, 100 ticks: every channel of the long logged rollout with episodes equals
    the stitched fresh rollouts bit for bit; records, count, age and start_tick equal the schedule.  walls: with a sensor feed -- the
    wrench of the first tick of a new episode is the feed's, untouched (it is a fresh rollout's tick 0); joints: the scene's rows with
    their ACTION drives -- ctrl is back at 0 behind a reset (joint_tau of the ticks after it says so; the state's ctrl at the end too)."""
    program, extras = CASES[case]
    dtype = F32 if case.endswith("f32") else F64
    fl = fleet(B0)
    ref = fresh(fl, dtype, program, extras)
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T)
    if program == "none":
        assert (ref["outcomes"] == ep.TIMEOUT).all() and (sched["count"] == T // MAX_TICKS).all()
    else:
        assert_preconditions(ref, sched, B0)
    outs, st, more = run_with_episodes(fl, dtype, program, extras)
    assert outs[0]["ticks_run"] == T and np.array_equal(outs[0]["log_ticks"], np.arange(T))
    assert_equals_stitched(outs[0]["log"], ref, sched)
    assert_state_is(st, sched, T)
    if "walls" in extras:
        assert ref["log"]["wall_force"].any(), "no robot touched a wall in the fresh runs"
        first = np.argwhere(sched["age"][1:] == 0) + [1, 0]      # the first ticks of later episodes
        assert len(first) and all(same_bits(outs[0]["log"]["wrench"][t, b], ref["log"]["wrench"][sched["start"][t, b], sched["variant"][t, b], 0, b])
                                  for t, b in first)
    if "joints" in extras:
        assert ref["log"]["joint_tau"].any()
        fresh_now = sched["age_end"] == 0                        # robots whose last tick ended an episode: every ctrl is 0 again
        assert fresh_now.any() and not more["joint"]["ctrl"][fresh_now].any() and more["joint"]["ctrl"][~fresh_now].any()


def test_a_grip_as_action_0():
    """GRIP WP GRIP: the list's first ticks write no target, so the first OSC steps of a new episode aim at the SNAPSHOT's row -- 5 cm
    beside the EE, far enough for the velocity limit to bite -- and the limit (word 9) they run under is the context's again, not the
    one the last episode's WP left."""
    fl = fleet(B0, kinds=(GRIP, WP, GRIP))
    ref = fresh(fl, F64, "list", (), key="grip0")
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T)
    assert_preconditions(ref, sched, B0)
    outs, st, _ = run_with_episodes(fl, F64, "list", ())
    assert_equals_stitched(outs[0]["log"], ref, sched)
    assert_state_is(st, sched, T)


def test_the_row16_fromq_form(monkeypatch):
    """IRLOSC_LANE=0: the OSC step behind the walk is the row16 FROMQ kernel, in the fresh runs and in the run with episodes."""
    monkeypatch.setenv("IRLOSC_LANE", "0")
    fl = fleet(B0)
    ref = fresh(fl, F64, "list", (), key="lane0")
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T)
    assert_preconditions(ref, sched, B0)
    outs, st, _ = run_with_episodes(fl, F64, "list", ())
    assert_equals_stitched(outs[0]["log"], ref, sched)
    assert_state_is(st, sched, T)


@pytest.mark.parametrize("B", [1, 64])
def test_a_lone_robot_and_a_full_wave(B):
    """B = 1 (robot 3 of the fleet, in a context of exactly one: the shared layouts of every table) and B = 64 (no ragged wave)."""
    fl = sub(fleet(B0), slice(3, 4) if B == 1 else slice(0, 64))
    ref = fresh(fl, F64, "list", (), key=f"sub{B}", max_batch=B)
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T)
    assert sched["count"].max() >= 3
    outs, st, _ = run_with_episodes(fl, F64, "list", (), max_batch=B)
    assert_equals_stitched(outs[0]["log"], ref, sched)
    assert_state_is(st, sched, T)


# ---- 2. rollouts over fewer robots ----------------------------------------------------------------------------------------------------------
def test_a_narrower_rollout_leaves_the_others_ages_standing():
    """30 ticks over all 130, 17 over the first 70 (a ragged second wave), 53 over all: the robots left out neither age nor reset, and
    pick up where they stood."""
    fl = fleet(B0)
    ref = fresh(fl, F64, "list", ())
    ran = np.ones((T, B0), bool)
    ran[30:47, 70:] = False
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T, ran=ran)
    osc = open_ctx(B0)
    osc.upload_q(fl["q"][:, 0], fl["qd"][:, 0])
    osc.set_targets(fl["tgt"])
    arm_program(osc, fl, "list")
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=MAX_TICKS, poses=fl["poses"], records=RECORDS)
    a = osc.rollout_logged(30, list(FRONT))
    age30 = osc.episode_state()["age"]
    osc._B[0] = 70
    b = osc.rollout_logged(17, list(FRONT))
    # (the narrower rollout left the slot coordinates of the 70 robots it ran: the others' go in again as they stood -- uploads leave
    #  the list and the episodes alone)
    osc.upload_q(np.concatenate([b["qpos"], a["qpos"][70:]]), np.concatenate([b["qvel"], a["qvel"][70:]]))
    assert osc._B[0] == B0
    st47 = osc.episode_state()
    c = osc.rollout_logged(53, list(FRONT))
    st = osc.episode_state()
    osc.close()
    assert np.array_equal(st47["age"][70:], age30[70:]) and not np.array_equal(st47["age"][:70], age30[:70])
    assert_equals_stitched(a["log"], ref, sched, ticks=slice(0, 30))
    want = ep.stitch({n: ref["log"][n] for n in ref["channels"]}, sched)
    for n in ref["channels"]:
        assert same_bits(b["log"][n], np.ascontiguousarray(want[n][30:47, :70])), n
    assert_equals_stitched(c["log"], ref, sched, ticks=slice(47, T))
    assert_state_is(st, sched, 53)


# ---- 3. what ends episodes, what is refused ---------------------------------------------------------------------------------------------
def test_a_list_set_again_ends_the_episodes():
    """Episodes, 10 ticks, then the list again (variant 1) and start 1 uploaded: the episodes have ended -- the download says so -- and the
    rollout is the fresh one, beyond max_ticks too."""
    fl = fleet(B0)
    ref = fresh(fl, F64, "list", ())
    osc = open_ctx(B0)
    osc.upload_q(fl["q"][:, 0], fl["qd"][:, 0])
    osc.set_targets(fl["tgt"])
    arm_program(osc, fl, "list")
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=MAX_TICKS, poses=fl["poses"], records=RECORDS)
    osc.rollout(10)
    arm_program(osc, fl, "list", 1)
    with pytest.raises(_lib.IrloscError, match="has no episodes"):
        osc.episode_state()
    osc.upload_q(fl["q"][:, 1], fl["qd"][:, 1])
    osc.set_targets(fl["tgt"])
    arm_program(osc, fl, "list", 1)
    r = osc.rollout_logged(40, list(FRONT))
    osc.close()
    for n in FRONT:
        assert same_bits(r["log"][n], np.ascontiguousarray(ref["log"][n][1, 1, :40])), n


def test_refusals_in_both_orders():
    """Episodes next to a teleoperation stream or pushes: refused whichever comes second, and what was in force stays.  Pose variants on
    a list whose pose table the fleet shares: refused."""
    B = 5
    fl = sub(fleet(B0), slice(0, B))
    osc = open_ctx(B, max_batch=B)
    osc.upload_q(fl["q"][:, 0], fl["qd"][:, 0])
    osc.set_targets(fl["tgt"])
    eps = dict(max_ticks=MAX_TICKS, records=RECORDS)
    rd = tts.fleet_readings(B, 8)
    wr = np.zeros((1, 6))
    push = [dict(dev=0, window=(0, 3), apply=True, sense=False)]
    # a stream, then episodes
    osc.set_teleop_stream(rd, tts.ORIGIN)
    with pytest.raises(_lib.IrloscError, match="-3.*teleoperation stream"):
        osc.set_episodes(fl["q"], fl["qd"], **eps)
    assert osc.teleop_state()["tick"] == 0
    osc.clear_teleop_stream()
    # pushes, then episodes
    osc.set_pushes(push, wr)
    with pytest.raises(_lib.IrloscError, match="-3.*pushes"):
        osc.set_episodes(fl["q"], fl["qd"], **eps)
    osc.clear_pushes()
    # episodes, then either
    osc.set_episodes(fl["q"], fl["qd"], **eps)
    with pytest.raises(_lib.IrloscError, match="-3.*episodes"):
        osc.set_teleop_stream(rd, tts.ORIGIN)
    with pytest.raises(_lib.IrloscError, match="-3.*episodes"):
        osc.set_pushes(push, wr)
    assert osc.episode_state()["count"].tolist() == [0] * B      # (still in force)
    osc.rollout(3)
    assert osc.episode_state()["age"].tolist() == [3] * B
    # variants on a shared table
    osc.set_action_list(dict(fl["desc"], pose=np.ascontiguousarray(fl["desc"]["pose"][:1])))
    with pytest.raises(_lib.IrloscError, match="-3.*shares one"):
        osc.set_episodes(fl["q"], fl["qd"], poses=fl["poses"], **eps)
    with pytest.raises(_lib.IrloscError, match="has no episodes"):      # (the list's setter ended the earlier ones)
        osc.episode_state()
    osc.set_episodes(fl["q"], fl["qd"], **eps)                          # without variants a shared table is fine
    osc.set_action_list(None)
    with pytest.raises(_lib.IrloscError, match="has no episodes"):      # (and clearing the list they were set on ends them)
        osc.episode_state()
    osc.close()


def test_a_slot_whose_episodes_were_cleared_is_a_slot_that_never_had_any():
    fl = fleet(B0)
    ref = fresh(fl, F64, "list", ())
    osc = open_ctx(B0)
    osc.set_targets(fl["tgt"])
    osc.upload_q(fl["q"][:, 1], fl["qd"][:, 1])
    arm_program(osc, fl, "list")
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=MAX_TICKS, poses=fl["poses"], records=RECORDS, poll_every=8, max_episodes=1)
    osc.clear_episodes()
    osc.upload_q(fl["q"][:, 0], fl["qd"][:, 0])      # (set_episodes wrote start 0 and variant 0: the same again, through today's calls)
    arm_program(osc, fl, "list")
    r = osc.rollout_logged(40, list(FRONT))
    osc.close()
    assert r["ticks_run"] == 40
    for n in FRONT:
        assert same_bits(r["log"][n], np.ascontiguousarray(ref["log"][n][0, 0, :40])), n


# ---- 4. the early exit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logged", [True, False])
def test_the_early_exit(logged):
    """max_episodes = 2, poll_every = 8: ticks_run is the formula on the reference lengths; the log is cut to it; parked robots equal
    fresh rollouts that simply ran on; poll_every = 0 runs all ticks."""
    fl = fleet(B0)
    ref = fresh(fl, F64, "list", ())
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T, max_episodes=2)
    assert (sched["park_tick"] >= 0).all() and len(set(sched["park_tick"])) >= 3
    want = ep.ticks_run(sched["park_tick"], T, 8)
    assert 16 < want < T and want % 8 == 0 and want == 8 * (-(-(sched["park_tick"].max() + 1) // 8) + 1)
    outs, st, _ = run_with_episodes(fl, F64, "list", (), max_episodes=2, poll_every=8, logged=logged)
    r = outs[0]
    assert r["ticks_run"] == want == st["ticks_run"] and st["running"] == 0
    cut = ep.schedule(ref["lengths"], ref["outcomes"], want, max_episodes=2)
    if logged:
        assert np.array_equal(r["log_ticks"], np.arange(want))
        assert_equals_stitched(r["log"], ref, cut)
        assert (cut["parked"][-1]).all() and cut["age"][-1].max() > MAX_TICKS      # (the rows of parked robots are fresh ticks beyond the episode)
    else:
        last = ep.stitch({"u": ref["log"]["u"]}, cut)["u"][-1]
        assert same_bits(r["u"], np.ascontiguousarray(last))
    assert np.array_equal(st["count"], np.full(B0, 2)) and np.array_equal(st["records"], ep.ring(cut, RECORDS))
    if logged:
        outs0, st0, _ = run_with_episodes(fl, F64, "list", (), max_episodes=2, poll_every=0)
        assert outs0[0]["ticks_run"] == T and st0["ticks_run"] == T
        assert_equals_stitched(outs0[0]["log"], ref, sched)
