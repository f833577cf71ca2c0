"""Episodes off k13 and on shared tables (-m gpu): what tests/test_episodes.py holds at one value of almost every runtime argument of
osc_episode_kernel -- k13, per-robot tables, shared gains, one slot, RECORDS = 8, poll_every = 8 -- here with ndev, stride, active, A,
wmax, R, S, V, records and the four layout switches (starts_per_robot, list_per_robot, wp_per_robot, gains_per_robot) at other values.

The method is that file's, and so are the helpers (fleet, fresh, run_with_episodes, assert_equals_stitched, assert_state_is,
assert_preconditions, with the layout as a parameter): every robot's arithmetic is its own lane's, so ONE long logged rollout with
episodes equals, BIT FOR BIT on every logged channel, the stitching (episodes.stitch along episodes.schedule) of S x V fresh logged
rollouts through the entry points that were there before episodes, with lengths from the fresh runs' own finished ticks; and
episode_state() equals the schedule.  No comparison in this file has a tolerance.  Preconditions are asserted on the REFERENCE runs of
every case: no robot froze, wave 0 holds three episode lengths, both outcomes occur, some robot's ring wrapped, robots 128 and 129
differ, walls were touched and rows acted where they are armed.  Fresh rollouts run MAX_TICKS ticks where no robot parks (no age beyond
the timeout is ever asked for), T ticks where parked robots run on.  Fleets stay far below the eigen pass's lane-form threshold.

1. per layout;  2. shared tables with B > 1 and per-robot gains;  3. the description's edges;  4. paths with more than one judge;
5. two slots;  6. the early exit off P = 8;  7. the transitions of "one writer of the targets";  8. the eigen pass pinned to its lane
form, in a child process, with flagged robots among the start states."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_action_list as tal
import test_action_list_layouts as tall
import test_episodes as te
import test_rollout as tr
import test_rollout_layouts as trl
import test_rollout_log_layouts as tlgl
import test_walls as twl
from irl_control_amd import _lib, episodes as ep, synth

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
WP, GRIP = tal.WP, tal.GRIP
same_bits = te.same_bits
B0, BMAX, T, MAX_TICKS, RECORDS, PATH_THR, FRONT = te.B0, te.BMAX, te.T, te.MAX_TICKS, te.RECORDS, te.PATH_THR, te.FRONT
BOTH = (twl.N_Y, twl.N_X)      # two normals: two of a device's three force words are in use, so a plane taken for another shows


def check(fl, dtype, program, extras, key, ticks=T, fresh_ticks=MAX_TICKS, max_ticks=MAX_TICKS, pre=True, cap=BMAX, records=RECORDS,
          end_on_finish=True, max_episodes=0):
    """The comparison of test_episodes.test_episodes_equal_fresh_rollouts on a fleet.  -> ref, sched, the run's result, state, more"""
    ref = te.fresh(fl, dtype, program, extras, ticks=fresh_ticks, max_ticks=max_ticks, key=key, max_batch=cap, end_on_finish=end_on_finish)
    sched = ep.schedule(ref["lengths"], ref["outcomes"], ticks, max_episodes=max_episodes)
    if pre:
        te.assert_preconditions(ref, sched, fl["B"])
    if "walls" in extras:
        assert ref["log"]["wall_force"].any(), "no robot touched a wall in the fresh runs"
    if "joints" in extras:
        assert ref["log"]["joint_tau"].any()
    outs, st, more = te.run_with_episodes(fl, dtype, program, extras, ticks=ticks, max_ticks=max_ticks, max_batch=cap, records=records,
                                          end_on_finish=end_on_finish, max_episodes=max_episodes)
    assert outs[0]["ticks_run"] == ticks and np.array_equal(outs[0]["log_ticks"], np.arange(ticks))
    te.assert_equals_stitched(outs[0]["log"], ref, sched)
    te.assert_state_is(st, sched, ticks, records)
    return ref, sched, outs[0], st, more


def first_ticks(sched):
    """(tick, robot) of the first ticks of later episodes."""
    return np.argwhere(sched["age"][1:] == 0) + [1, 0]


# ---- 1. per layout ---------------------------------------------------------------------------------------------------------------------
# route: a key of test_rollout_layouts.ROUTES, else the layout's own lane kernel; active / passive: test_action_list_layouts.CASES'
LAYOUTS = {
    "r6": dict(route="r6", cfg="r6", dtype=F64, roles=None),
    "k12_admit": dict(route=None, cfg="k12_admit", dtype=F64, roles="k12_admit_feed", walls=(0, 1)),
    "k12_admit_f32": dict(route=None, cfg="k12_admit", dtype=F32, roles="k12_admit_feed", walls=(0, 1)),
    "br7": dict(route="br7", cfg="br7", dtype=F64, roles="br7", kinds=(GRIP, WP, GRIP)),
    "rlbr10": dict(route="rlbr10", cfg="rlbr10", dtype=F64, roles="rlbr10", walls=(0, 3)),
    "rlb16": dict(route="rlb16", cfg="rlb16", dtype=F64, roles="rlb16_f32"),
    "rlb11_branch_b": dict(route="rlb11_branch_b", cfg="rlb11_branch_b", dtype=F64, roles="rlb11_branch_b", cap=B0),
    "k13_f32_paths_walls_joints": dict(route=None, cfg="k13", dtype=F32, roles="k13", programs=("paths",)),
}


def opener(name, monkeypatch):
    """-> fl["open"] of a layout case: the context of test_rollout_layouts.open_ctx (its route asserted there) or, for a layout with a
    lane kernel of its own, of test_rollout.make_ctx with test_rollout_log_layouts' route assertion; the plant of test_action_list."""
    c = LAYOUTS[name]

    def open_(cap, dtype, feed, n_slots):
        if c["route"] is not None:
            osc = trl.open_ctx(c["route"], cap, dtype, monkeypatch, feed=feed, n_slots=n_slots)[4]
        else:
            osc = tr.make_ctx(c["cfg"], cap, dtype, feed=feed, n_slots=n_slots)[4]
            tlgl.assert_own_route(c["cfg"], dtype, osc.from_q_name, osc.kernel_name)
        assert osc.max_batch == cap
        osc.set_plant(tal.DT, tal.DAMPING)
        return osc
    return open_


def layout_fleet(name, monkeypatch):
    c = LAYOUTS[name]
    cfg = c["cfg"]
    lay = synth.make_layout(cfg)
    roles = tall.CASES[c["roles"]] if c["roles"] else {}
    fl = te.fleet(B0, kinds=c.get("kinds", (WP, GRIP, WP)), cfg=cfg, active=roles.get("active"), passive=roles.get("passive"))
    walls = c.get("walls") or tlgl.wall_devices(name if name in tlgl.CASES else "k13")
    fl = dict(fl, open=opener(name, monkeypatch), wall_devs=walls, wall_normals=BOTH, wall_x=fl["ee"])
    if "branch_b" in cfg:      # (0.1 x synth.make_batch's, as test_action_list_layouts)
        fl["tgt_vel"] = 0.1 * synth.make_batch(cfg, B0, seed=21)[2]["tgt_vel"]
    # the paths: the first arm with xyz rows walks (paths_of), the other arm loops; rlbr10: block 3 (orientation rows only, the body of
    # block 0) loops over FOUR waypoints within the threshold of each other -- three listed devices, W = 3, 2 and 4
    walker = next(d for d, nm in enumerate(lay.dev_names) if nm == "ur5right" and np.any(lay.ctrlr_dof[d][:3]))
    names = list(lay.dev_names)
    pf = dict(fl, tgt=fl["ee"], ia=walker, io=names.index("ur5left") if "ur5left" in names else -1)
    paths = te.paths_of(pf)
    loop = [d != walker for d in range(lay.ndev)]
    if cfg == "rlbr10":
        x3 = fl["tgt"][:, 3, :3]
        paths[3] = np.stack([x3, x3 + [0.0, 0.0, 2e-4], x3 + [0.0, 2e-4, 0.0], x3 + [0.0, 1e-4, 1e-4]], axis=1)
    fl.update(paths=paths, loop=loop)
    return fl, c["dtype"], c.get("cap", BMAX), c.get("programs", ("list", "paths"))


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_episodes_equal_fresh_rollouts_per_layout(name, monkeypatch):
    """B = 130 (in a context of 192; rlb11_branch_b: of 130), S = 2, V = 3, max_ticks 24, 100 ticks, a LIST program with three variants
    and a PATHS program, each with everything the layout allows: a feed, median walls with two normals on the devices of
    test_rollout_log_layouts.wall_devices (k12_admit: both arms), test_joints.scene(lay).  The route is asserted where the contexts open.
      r6               one device: the row is 7 words, no passive device, the paths on the only device
      k12_admit(_f32)  the wrench enters u: u of the first tick of every later episode is a fresh tick 0's, and some robot that was
                       reset had a wall force on the tick before (asserted on the reference) -- a force left standing would be sensed
      br7              the base is device 0, the active device 1: word 9 at active * GAIN_WORDS + 9 -- the list opens with a GRIP here
                       (GRIP WP GRIP, the slot's target 5 cm beside the EE), as only then a limit left by the last WP reaches a step
      rlbr10           four devices (28 words a row); active 3 has orientation rows only (its poses are turned), passive 1; walls on
                       blocks 0 and 3; paths on three devices with W = 3, 2 and 4
      rlb16            the row16 FROMQ form
      rlb11_branch_b   target velocities on the slot, a tight context: branch B in the logged flags on the first ticks of later
                       episodes (a reset that touched the target velocities would leave branch B or change u)
      k13_f32_paths_walls_joints   float32 records: the paths' (T) conversion and the float32 snapshot under walls and rows"""
    fl, dtype, cap, programs = layout_fleet(name, monkeypatch)
    for program in programs:
        ref, sched, out, st, more = check(fl, dtype, program, ("walls", "joints"), key=(name, program), cap=cap)
        first = first_ticks(sched)
        assert len(first) > B0
        want = ep.stitch({n: ref["log"][n] for n in ("u", "wall_force", "flags")}, sched)
        if "k12_admit" in name:
            for t, b in first:
                assert same_bits(out["log"]["u"][t, b], ref["log"]["u"][sched["start"][t, b], sched["variant"][t, b], 0, b]), (t, b)
            assert sum(bool(want["wall_force"][t - 1, b].any()) for t, b in first) >= 10, "hardly a reset robot had a wall force to be zeroed"
        if "branch_b" in name:
            fb = np.array([want["flags"][t, b] for t, b in first])
            assert ((fb & _lib.FLAG_VEL_BRANCH_B) != 0).mean() > 0.5
            trl.assert_branch_b(name, np.bitwise_or.reduce(out["log"]["flags"], axis=0))
        fresh_now = sched["age_end"] == 0
        assert fresh_now.any() and not more["joint"]["ctrl"][fresh_now].any()


# ---- 2. shared tables with B > 1; per-robot gains ---------------------------------------------------------------------------------------
_CLUSTER = {}


def clustered(rad, kinds=(WP, GRIP, WP)):
    """A k13 fleet of 130 whose robots start within `rad` rad per joint of ONE configuration, so that one table can serve them all: start 1
    is start 0 moved by up to rad / 5 on the active arm with small joint velocities.  Robot 128 starts AT the configuration, 129 lies
    0.05 rad off it (out of reach).  -> fleet()'s dict with per-robot starts and tgt, and centre: the EE poses of the configuration."""
    if (rad, kinds) in _CLUSTER:
        return _CLUSTER[(rad, kinds)]
    B = B0
    rng = np.random.default_rng(79)
    c, _ = tal.start_state(1, rng)
    q0 = np.repeat(c, B, axis=0)
    for arm in (tal.RIGHT, tal.LEFT):
        q0[:, arm] += rng.uniform(-rad, rad, (B, 6))
    q0[128] = c[0]
    q0[129, tal.RIGHT] = c[0, tal.RIGHT] + 0.05
    q = np.stack([q0, q0], axis=1)
    q[:, 1, tal.RIGHT] += rng.uniform(-rad / 5, rad / 5, (B, 6))
    qd = np.zeros_like(q)
    qd[:, 1, tal.RIGHT] = rng.uniform(-0.01, 0.01, (B, 6))
    tgt = tal.ee_start(q[:, 0], qd[:, 0], "k13")
    centre = tal.ee_start(np.repeat(c, B, axis=0), qd[:, 0], "k13")[0]
    base = te.fleet(B0, kinds=kinds)
    for a in (q, qd, tgt, centre):
        a.setflags(write=False)
    _CLUSTER[(rad, kinds)] = dict(base, q=q, qd=qd, tgt=tgt, centre=centre)
    return _CLUSTER[(rad, kinds)]


def one_table(fl, short=2e-4):
    """The fleet with ONE pose table (nb == 1) and no variants: the WPs lie max_error - short and max_error - short + 1e-4 m along x from
    the centre's active EE pose, so a robot's distance follows where in the cluster it starts."""
    desc = fl["desc"]
    pose = np.zeros((1, desc["n_actions"], 7))
    pose[..., 3] = 1.0
    for i, a in enumerate(np.nonzero(desc["kind"] == WP)[0]):
        pose[0, a] = fl["centre"][fl["ia"]]
        pose[0, a, 0] += te.MAX_ERROR - short + 1e-4 * i
    return dict(fl, desc=dict(desc, pose=pose), poses=np.zeros((0,) + fl["poses"].shape[1:]))


def test_shared_starts_with_per_robot_variants():
    """qpos0 [S, n]: every robot starts where robot 128 of the cluster starts; the pose variants are per robot (fleet()'s offsets, taken
    from the shared EE pose), so the lengths differ through the poses."""
    base = te.fleet(B0)
    cl = clustered(1e-3)
    ee = cl["tgt"][128]
    poses = np.array(base["poses"])
    wps = np.nonzero(base["desc"]["kind"] == WP)[0]
    for a in wps:
        off = base["poses"][:, :, a, 0] - base["tgt"][None, :, base["ia"], 0]
        poses[:, :, a] = ee[base["ia"]]
        poses[:, :, a, 0] += off
    fl = dict(base, q=cl["q"][128], qd=cl["qd"][128], tgt=np.ascontiguousarray(np.broadcast_to(ee, base["tgt"].shape)), poses=poses,
              desc=dict(base["desc"], pose=poses[0]))
    assert fl["q"].shape == (te.S, 25)
    check(fl, F64, "list", (), key="shared_starts")


def test_a_shared_pose_table_with_per_robot_starts():
    """nb == 1, V = 0, B = 130: a reset restores the list's state and never writes the one table -- every WP a robot enters in a later
    episode reads it, so a line of it written by anybody's reset shows in the targets of everybody's later episodes (no entry point
    downloads the table; the run against its stitched reference re-derives it WP by WP)."""
    fl = one_table(clustered(1e-3))
    ref, sched, out, st, _ = check(fl, F64, "list", (), key="shared_table")
    assert np.all(st["records"][..., 3] >> 16 == 0)


def test_shared_paths_with_per_robot_starts():
    """One [W, 3] path per device for the fleet (wp_per_robot = 0): the right arm's three waypoints 5e-6 and 7e-6 m beyond the threshold
    from the centre, the left arm looping over two; the robots start within 2e-5 rad of the centre."""
    cl = clustered(2e-5)
    ia, io = cl["ia"], cl["io"]
    xa, xo = cl["centre"][ia, :3], cl["centre"][io, :3]
    paths = [None] * 3
    paths[ia] = np.stack([xa, xa + [PATH_THR + 5e-6, 0.0, 0.0], xa + [PATH_THR + 7e-6, 0.0, 0.0]])
    paths[io] = np.stack([xo, xo + [0.0, 3e-4, 0.0]])
    fl = dict(cl, paths=paths, loop=[False, True, True])
    assert paths[ia].shape == (3, 3)
    check(fl, F64, "paths", (), key="shared_paths")


def test_everything_shared():
    """Shared starts, one pose table, no variants, B = 130: every robot's rows equal robot 0's, in the reference and under test (the
    precondition on distinct lengths does not apply); the run equals the stitched reference."""
    cl = one_table(clustered(1e-3))
    fl = dict(cl, q=cl["q"][128], qd=cl["qd"][128], tgt=np.ascontiguousarray(np.broadcast_to(cl["tgt"][128], cl["tgt"].shape)))
    ref, sched, out, st, _ = check(fl, F64, "list", (), key="all_shared", pre=False)
    assert sched["count"].max() >= 3 and len(set(sched["count"])) == 1
    for n in FRONT:
        for log in (ref["log"][n].reshape((-1,) + ref["log"][n].shape[3:]), out["log"][n]):
            assert all(same_bits(np.ascontiguousarray(log[:, b]), np.ascontiguousarray(log[:, 0])) for b in (1, 63, 64, 128, 129)), n
    assert np.all(st["records"] == st["records"][0])


def test_per_robot_gains():
    """set_gains with a leading axis of max_batch = 192 and a velocity limit per robot in [0.05, 0.15] m/s; the list opens with a GRIP, so
    the first steps of every new episode aim 5 cm beside the EE and run into the robot's OWN limit, taken back from ITS gain record
    (the limit bites where the error exceeds limit / 4: at most 3.75 cm).  Asserted on fresh ticks: u of tick 0 differs for every robot
    from a run with the limits doubled, and robots 0 and 1 have different limits."""
    base = te.fleet(B0, kinds=(GRIP, WP, GRIP))
    rng = np.random.default_rng(80)
    g = tal.base_gains("k13")

    def gains(scale):
        mv = np.broadcast_to(np.asarray(g["max_vel"], F64), (BMAX, 3, 2)).copy()
        mv[:, :2, 0] = scale * limits[:, None]
        return dict(g, max_vel=mv)
    limits = rng.uniform(0.05, 0.15, BMAX)
    assert limits[0] != limits[1]
    fl = dict(base, open=lambda cap, dtype, feed, n_slots: te.open_ctx(B0, dtype, feed, cap, n_slots, gains=gains(1.0)))
    u0 = []
    for scale in (1.0, 2.0):
        osc = te.open_ctx(B0, F64, gains=gains(scale))
        osc.upload_q(*te.start_of(fl, 0))
        osc.set_targets(fl["tgt"])
        u0.append(osc.rollout(1)["u"])
        osc.close()
    assert np.all(np.any(u0[0] != u0[1], axis=1)), "the limit does not bite on tick 0"
    ref, sched, out, st, _ = check(fl, F64, "list", (), key="per_robot_gains")
    assert same_bits(ref["log"]["u"][0, 0, 0], u0[0])


def test_a_lone_robot_in_a_wide_context():
    """B = 1 in a context of 192: the shared layouts of the start states and of the pose table WITH variants (V > 0 next to nb == 1 is
    legal for a lone robot only), at a stride that is not B."""
    fl = te.sub(te.fleet(B0), slice(3, 4))
    ref, sched, out, st, _ = check(fl, F64, "list", (), key="lone_wide", pre=False)
    assert sched["count"].max() >= 3 and len(set(ref["lengths"].ravel())) >= 2


# ---- 3. the description's edges ---------------------------------------------------------------------------------------------------------
def test_end_on_finish_off():
    """end_on_finish = False: every outcome is TIMEOUT, every length max_ticks (lengths_from_finish says so); robots whose list finished
    early hold as finished robots do until the timeout -- the fresh rollouts' rows behind their finished tick."""
    fl = te.fleet(B0)
    ref, sched, out, st, _ = check(fl, F64, "list", (), key="eof0", pre=False, end_on_finish=False)
    assert (ref["lengths"] == MAX_TICKS).all() and (ref["outcomes"] == ep.TIMEOUT).all() and (sched["count"] == T // MAX_TICKS).all()
    early = (ref["finish"] >= 0) & (ref["finish"] < MAX_TICKS - 2)
    assert early.any(axis=(0, 1)).sum() >= 30, "hardly a robot finishes its list ahead of the timeout"
    assert np.all(st["records"][:, :T // MAX_TICKS, 2] == ep.TIMEOUT) and np.all(st["records"][:, :T // MAX_TICKS, 1] == MAX_TICKS)


def test_no_timeout():
    """max_ticks = 0 with end_on_finish: a robot whose variant 0 is out of reach never ends -- count 0, start_tick 0, age T --, the others
    keep finishing (their later episodes may be the ones that never end)."""
    fl = te.fleet(B0)
    ref, sched, out, st, _ = check(fl, F64, "list", (), key="mt0", pre=False, fresh_ticks=T, max_ticks=0)
    never = ref["lengths"][0, 0] == 0
    assert never.sum() >= 10 and never[129] and (~never).sum() >= 30
    assert np.all(st["count"][never] == 0) and np.all(st["start_tick"][never] == 0) and np.all(st["age"][never] == T)
    assert sched["count"].max() > RECORDS and np.all(st["count"][~never] >= 1)
    assert set(st["records"][..., 2].ravel()) == {0, ep.FINISHED}


@pytest.mark.parametrize("records", [1, 16])
def test_rings_of_1_and_16_records(records):
    """records = 1: every robot that ended two episodes has overwritten its entry; records = 16: some robot has wrapped it and some have
    entries never written (zero)."""
    fl = te.fleet(B0)
    ref, sched, out, st, _ = check(fl, F64, "list", (), key=None, records=records)
    assert st["records"].shape == (B0, records, 4)
    assert sched["count"].max() > records
    if records == 16:
        assert (sched["count"] < records).any() and not st["records"][sched["count"] < records, -1].any()


@pytest.mark.parametrize("SV", [(1, 1), (3, 2), (2, 0)])
def test_other_numbers_of_starts_and_variants(SV):
    """(S, V) = (1, 1), (3, 2) and (2, 0: the list's own table stays) on a per-robot list."""
    fl = te.fleet(B0, S=SV[0], V=SV[1])
    assert fl["q"].shape == (B0, SV[0], 25) and len(fl["poses"]) == SV[1]
    ref, sched, out, st, _ = check(fl, F64, "list", (), key=("SV",) + SV)
    assert ref["lengths"].shape == (SV[0], max(SV[1], 1), B0)
    assert set(np.unique(st["records"][..., 3] & 0xFFFF)) == set(range(SV[0])) and set(np.unique(st["records"][..., 3] >> 16)) == set(range(max(SV[1], 1)))


def test_one_episode_per_robot():
    """max_episodes = 1: every robot parks at its first end and no reset ever runs; records and count are right, and the parked rows are
    fresh rollouts that ran on."""
    fl = te.fleet(B0)
    ref, sched, out, st, _ = check(fl, F64, "list", (), key=None, pre=False, ticks=60, fresh_ticks=T, max_episodes=1)
    assert (sched["park_tick"] >= 0).all() and (st["count"] == 1).all() and st["running"] == 0 and len(set(sched["park_tick"])) >= 3
    assert sched["parked"][-1].all() and sched["age"][-1].max() > MAX_TICKS and not st["records"][:, 1:].any()


# ---- 4. paths with more than one judge --------------------------------------------------------------------------------------------------
def judged_paths(kind):
    """fleet(130) with the LEFT arm of start 1 within 2e-5 rad of start 0's instead of 0.1 rad (a path is a robot's, not a start's: an
    arm that judges has to be near its path from every start, or every second episode is a timeout and no ring wraps)."""
    fl = te.fleet(B0)
    ia, io = fl["ia"], fl["io"]
    rng = np.random.default_rng(81)
    q = np.array(fl["q"])
    q[:, 1, tal.LEFT] = q[:, 0, tal.LEFT] + rng.uniform(-2e-5, 2e-5, (B0, 6))
    fl = dict(fl, q=q)
    paths = te.paths_of(fl)
    xo = fl["tgt"][:, io, :3]
    if kind == "both":      # the left arm has to come need beyond the threshold along y: the distribution of paths_of's need1
        u = rng.uniform(size=B0)
        need = np.where(u < 0.2, -1e-4, np.where(u < 0.9, 10.0 ** rng.uniform(-7, -4.7, B0), te.FAR))
        paths[io] = np.stack([xo, xo + (PATH_THR + need)[:, None] * np.array([0.0, 1.0, 0.0])], axis=1)
        loop = [False, False, True]
    elif kind == "all_looping":
        loop = [True, True, True]
    else:                   # one waypoint, not looping: through on its first arrival
        paths[io] = xo[:, None, :].copy()
        loop = [False, False, True]
    return dict(fl, paths=paths, loop=loop)


def test_two_arms_that_do_not_loop():
    """Both arms' paths end: an episode is FINISHED on the tick on which the LATER arm arrives.  Asserted on the fresh runs: where both
    arrive, their ticks differ for most robots."""
    fl = judged_paths("both")
    ref, sched, out, st, _ = check(fl, F64, "paths", (), key="two_judges")
    wp = ref["wp_state"][0][0]
    both = (wp["index"][:, 0] == 3) & (wp["index"][:, 1] == 2)
    assert both.sum() >= 20 and (wp["last_tick"][both, 0] != wp["last_tick"][both, 1]).mean() > 0.5
    later = (wp["last_tick"][both, 1] > wp["last_tick"][both, 0])
    assert later.any() and (~later).any()


def test_only_looping_paths():
    """Every listed device loops: `some` is false, only timeouts occur."""
    fl = judged_paths("all_looping")
    ref, sched, out, st, _ = check(fl, F64, "paths", (), key="all_looping", pre=False)
    assert (ref["outcomes"] == ep.TIMEOUT).all() and (st["count"] == T // MAX_TICKS).all()
    assert (ref["wp_state"][0][0]["arrivals"][:, 0] >= 3).any(), "no robot went round its path"


def test_a_listed_device_with_one_waypoint():
    """The left arm's path is one waypoint and does not loop (W = 1 next to W = 3: wmax is not every device's count)."""
    fl = judged_paths("one")
    check(fl, F64, "paths", (), key="one_waypoint")


# ---- 5. two slots -----------------------------------------------------------------------------------------------------------------------
def calls_run(park_tick, pieces, P):
    """The ticks each of a slot's calls runs (episodes.ticks_run call by call) for robots that park on the slot's ticks park_tick."""
    done, out = 0, []
    for p in pieces:
        rel = np.where(park_tick < 0, 10 ** 9, np.where(park_tick < done, -1, park_tick - done))
        out.append(ep.ticks_run(rel, p, P))
        done += out[-1]
    return out


def test_two_slots_interleaved():
    """n_slots = 2.  Slot 0: paths with episodes, max_ticks 24, records 8.  Slot 1: the list with episodes, max_ticks 17, records 4,
    max_episodes 3, poll_every 8.  Calls 30 (slot 0), 50 (slot 1), 70 (slot 0), 50 (slot 1): each slot equals its own single-slot
    stitched reference and schedule; slot 1's early exit cuts its own calls (per the formula) and never slot 0's."""
    fl = te.fleet(B0)
    r0 = te.fresh(fl, F64, "paths", (), ticks=MAX_TICKS, key="slot0")
    r1 = te.fresh(fl, F64, "list", (), ticks=T, max_ticks=17, key="slot1")
    s0 = ep.schedule(r0["lengths"], r0["outcomes"], T)
    te.assert_preconditions(r0, s0, B0)
    full1 = ep.schedule(r1["lengths"], r1["outcomes"], T, max_episodes=3)
    assert (full1["park_tick"] >= 0).all()
    runs1 = calls_run(full1["park_tick"], (50, 50), 8)
    assert runs1[0] < 50 or runs1[1] < 50
    s1 = ep.schedule(r1["lengths"], r1["outcomes"], sum(runs1), max_episodes=3)
    osc = te.open_for(fl, F64, n_slots=2)
    for slot, program in ((0, "paths"), (1, "list")):
        osc.upload_q(*te.start_of(fl, 1), slot=slot)
        te.set_slot_targets(osc, fl, slot)
        te.arm_program(osc, fl, program, 0, slot=slot)
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=MAX_TICKS, records=8, slot=0)
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=17, poses=fl["poses"], records=4, max_episodes=3, poll_every=8, slot=1)
    a0 = osc.rollout_logged(30, list(FRONT), slot=0)
    a1 = osc.rollout_logged(50, list(FRONT), slot=1)
    b0 = osc.rollout_logged(70, list(FRONT), slot=0)
    b1 = osc.rollout_logged(50, list(FRONT), slot=1)
    st0, st1 = osc.episode_state(0), osc.episode_state(1)
    osc.close()
    assert (a0["ticks_run"], b0["ticks_run"]) == (30, 70) and [a1["ticks_run"], b1["ticks_run"]] == runs1
    te.assert_equals_stitched(a0["log"], r0, s0, ticks=slice(0, 30))
    te.assert_equals_stitched(b0["log"], r0, s0, ticks=slice(30, T))
    te.assert_state_is(st0, s0, 70, 8)
    te.assert_equals_stitched(a1["log"], r1, s1, ticks=slice(0, runs1[0]))
    te.assert_equals_stitched(b1["log"], r1, s1, ticks=slice(runs1[0], sum(runs1)))
    te.assert_state_is(st1, s1, runs1[1], 4)


# ---- 6. the early exit off P = 8 --------------------------------------------------------------------------------------------------------
def armed(fl, **eps):
    """A k13 context with the list and episodes of test_episodes.run_with_episodes, not yet run."""
    osc = te.open_for(fl, F64)
    osc.upload_q(*te.start_of(fl, 1))
    te.set_slot_targets(osc, fl)
    te.arm_program(osc, fl, "list", 0)
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=MAX_TICKS, poses=fl["poses"], records=RECORDS, **eps)
    return osc


def parking():
    """-> the fleet, its fresh T-tick reference (test_episodes' own, shared) and the schedule with max_episodes = 2 over T ticks."""
    fl = te.fleet(B0)
    ref = te.fresh(fl, F64, "list", ())
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T, max_episodes=2)
    assert (sched["park_tick"] >= 0).all() and len(set(sched["park_tick"])) >= 3
    return fl, ref, sched


@pytest.mark.parametrize("P", [7, 1, 128])
def test_the_early_exit_with_other_periods(P):
    """poll_every = 7 (no divisor of 100), 1, and 128 (larger than the call: it runs all its ticks)."""
    fl, ref, sched = parking()
    want = ep.ticks_run(sched["park_tick"], T, P)
    D = int(sched["park_tick"].max())
    assert want == (T if P == 128 else (-(-(D + 1) // P) + 1) * P) and (P == 128 or D + 1 < want < T)
    outs, st, _ = te.run_with_episodes(fl, F64, "list", (), max_episodes=2, poll_every=P)
    r = outs[0]
    assert r["ticks_run"] == want == st["ticks_run"] and st["running"] == 0
    cut = ep.schedule(ref["lengths"], ref["outcomes"], want, max_episodes=2)
    assert np.array_equal(r["log_ticks"], np.arange(want))
    te.assert_equals_stitched(r["log"], ref, cut)
    te.assert_state_is(st, cut, want)


def test_a_second_call_on_a_parked_fleet():
    """After a call that parked every robot, a call of 40 ticks: park_tick = -1 everywhere, so it runs (max(1, 0) + 1) P = 16 ticks, on
    which the robots are fresh rollouts that ran on."""
    fl, ref, sched = parking()
    first = ep.ticks_run(sched["park_tick"], T, 8)
    second = ep.ticks_run(np.full(B0, -1), 40, 8)
    assert second == 16 and first + second <= T
    osc = armed(fl, max_episodes=2, poll_every=8)
    a = osc.rollout_logged(T, list(FRONT))
    b = osc.rollout_logged(40, list(FRONT))
    st = osc.episode_state()
    osc.close()
    assert (a["ticks_run"], b["ticks_run"]) == (first, second)
    cut = ep.schedule(ref["lengths"], ref["outcomes"], first + second, max_episodes=2)
    te.assert_equals_stitched(b["log"], ref, cut, ticks=slice(first, first + second))
    te.assert_state_is(st, cut, second)


def test_a_narrower_call_ends_when_its_own_robots_are_parked():
    """10 ticks over all 130, then a call of 100 over the first 70 with max_episodes = 2, poll_every = 8: it ends by the formula on ITS
    robots' parking ticks; episode_state()'s running still counts those of the 60 left out that are not parked, and their ages stand."""
    fl, ref, full = parking()
    rel = np.where(full["park_tick"][:70] < 10, -1, full["park_tick"][:70] - 10)
    want = ep.ticks_run(rel, T, 8)
    assert want < T - 10
    ran = np.ones((10 + want, B0), bool)
    ran[10:, 70:] = False
    sched = ep.schedule(ref["lengths"], ref["outcomes"], 10 + want, max_episodes=2, ran=ran)
    left = int((sched["park_tick"][70:] < 0).sum())
    assert left >= 30 and (sched["park_tick"][:70] >= 0).all()
    osc = armed(fl, max_episodes=2, poll_every=8)
    a = osc.rollout_logged(10, list(FRONT))
    age10 = osc.episode_state()["age"]
    osc._B[0] = 70
    b = osc.rollout_logged(T, list(FRONT))
    osc._B[0] = B0
    st = osc.episode_state()
    osc.close()
    assert a["ticks_run"] == 10 and b["ticks_run"] == want
    assert st["running"] == left and np.array_equal(st["age"][70:], age10[70:])
    stitched = ep.stitch({n: ref["log"][n] for n in ref["channels"]}, sched)
    for n in ref["channels"]:
        assert same_bits(b["log"][n], np.ascontiguousarray(stitched[n][10:, :70])), n
    te.assert_state_is(st, sched, want)


def test_the_early_exit_cuts_the_trace_and_a_sparse_log():
    """rollout(100, trace_every=3): ee_trace has ceil(ticks_run / 3) samples, the stitched ee_pose of those ticks.  rollout_logged(100,
    every=3, robots = a strictly ascending subset of all three waves): log_ticks and the log are cut to ticks_run."""
    fl, ref, sched = parking()
    want = ep.ticks_run(sched["park_tick"], T, 8)
    stitched = ep.stitch({n: ref["log"][n] for n in ref["channels"]}, ep.schedule(ref["lengths"], ref["outcomes"], want, max_episodes=2))
    ticks = np.arange(0, want, 3)
    osc = armed(fl, max_episodes=2, poll_every=8)
    r = osc.rollout(T, trace_every=3)
    osc.close()
    assert r["ticks_run"] == want and r["ee_trace"].shape[0] == -(-want // 3) == len(ticks)
    assert same_bits(r["ee_trace"], np.ascontiguousarray(stitched["ee_pose"][ticks]))
    robots = [0, 5, 63, 64, 100, 127, 128, 129]
    osc = armed(fl, max_episodes=2, poll_every=8)
    r = osc.rollout_logged(T, list(FRONT), every=3, robots=robots)
    osc.close()
    assert r["ticks_run"] == want and np.array_equal(r["log_ticks"], ticks)
    for n in FRONT:
        assert same_bits(r["log"][n], np.ascontiguousarray(stitched[n][ticks][:, robots])), n


# ---- 7. the transitions of "one writer of the targets" -------------------------------------------------------------------------------------
def test_set_targets_ends_the_episodes():
    fl = te.fleet(B0)
    ref = te.fresh(fl, F64, "list", ())
    osc = armed(fl)
    osc.rollout(10)
    osc.set_targets(fl["tgt"])
    with pytest.raises(_lib.IrloscError, match="has no episodes"):
        osc.episode_state()
    osc.upload_q(*te.start_of(fl, 1))
    te.arm_program(osc, fl, "list", 1)
    r = osc.rollout_logged(40, list(FRONT))
    osc.close()
    assert r["ticks_run"] == 40
    for n in FRONT:
        assert same_bits(r["log"][n], np.ascontiguousarray(ref["log"][n][1, 1, :40])), n


def new_gains(osc):
    """The context's gains with the arms' angular velocity limit at 4 instead of 5 rad/s: new values, so the call is not skipped."""
    g = tal.base_gains("k13")
    mv = np.array(g["max_vel"], F64)
    mv[:2, 1] = 4.0
    osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], mv, g["null_kv"])
    return dict(g, max_vel=mv)


def test_set_gains_ends_a_list_and_its_episodes():
    """set_gains with new values on a slot whose program is a list: the list ends, and the episodes with it; the rollout that follows is
    that of a fresh context with the new gains, the slot's coordinates and targets and no program -- beyond max_ticks too."""
    fl = te.fleet(B0)
    osc = armed(fl)
    osc.rollout(10)
    g = new_gains(osc)
    with pytest.raises(_lib.IrloscError, match="has no episodes"):
        osc.episode_state()
    q, qd = osc.download_q()
    tgt = osc.download_targets()
    r = osc.rollout_logged(40, list(FRONT))
    osc.close()
    plain = te.open_ctx(B0, F64, gains=g)
    plain.upload_q(q, qd)
    plain.set_targets(tgt)
    want = plain.rollout_logged(40, list(FRONT))
    plain.close()
    assert r["ticks_run"] == 40 and not np.any(want["flags_any"] & te.tal_bad())
    for n in FRONT:
        assert same_bits(r["log"][n], want["log"][n]), n


def test_set_gains_leaves_the_episodes_of_paths():
    """set_gains on a slot with paths: the episodes stay.  The new values differ in the arms' angular velocity limit only, which no step
    of these paths reaches (errors of micrometres), so the limit never enters u: 40 + 60 ticks around the call equal the uninterrupted
    stitched reference bit for bit, and count, age and records carry on."""
    fl = te.fleet(B0)
    ref = te.fresh(fl, F64, "paths", (), ticks=MAX_TICKS, key="slot0")
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T)
    te.assert_preconditions(ref, sched, B0)
    osc = te.open_for(fl, F64)
    osc.upload_q(*te.start_of(fl, 1))
    te.set_slot_targets(osc, fl)
    te.arm_program(osc, fl, "paths")
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=MAX_TICKS, records=RECORDS)
    a = osc.rollout_logged(40, list(FRONT))
    new_gains(osc)
    assert np.array_equal(osc.episode_state()["count"], ep.schedule(ref["lengths"], ref["outcomes"], 40)["count"])
    b = osc.rollout_logged(60, list(FRONT))
    st = osc.episode_state()
    osc.close()
    te.assert_equals_stitched(a["log"], ref, sched, ticks=slice(0, 40))
    te.assert_equals_stitched(b["log"], ref, sched, ticks=slice(40, T))
    te.assert_state_is(st, sched, 60)


def test_a_refused_set_episodes_leaves_those_in_force_whole():
    """A context of 192 with targets and a list for 192 robots, coordinates, a feed, walls and episodes for 130.  After 40 ticks
    set_episodes is refused twice -- IRLOSC_ERR_ARG for a NaN in a start state, IRLOSC_ERR_STATE for B = 192, more than the walls cover --
    and 60 more ticks follow: the whole run equals the uninterrupted stitched reference bit for bit, the state the schedule."""
    big = te.fleet(BMAX)
    fl = te.sub(big, slice(0, B0))
    ref = te.fresh(fl, F64, "list", ("walls",), ticks=MAX_TICKS, key="refused")
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T)
    te.assert_preconditions(ref, sched, B0)
    assert ref["log"]["wall_force"].any()
    ch = te.channels_of(("walls",))
    osc = te.open_ctx(BMAX, F64, feed=True)
    osc.upload_q(big["q"][:, 1], big["qd"][:, 1])
    osc.set_targets(big["tgt"])
    te.arm_program(osc, big, "list", 0)
    osc.upload_q(*te.start_of(fl, 1))
    te.arm_extras(osc, fl, ("walls",))
    eps = dict(max_ticks=MAX_TICKS, records=RECORDS)
    osc.set_episodes(fl["q"], fl["qd"], poses=fl["poses"], **eps)
    a = osc.rollout_logged(40, ch)
    bad = np.array(fl["q"])
    bad[77, 1, 3] = np.nan
    with pytest.raises(_lib.IrloscError, match="-1.*not finite"):
        osc.set_episodes(bad, fl["qd"], poses=fl["poses"], **eps)
    osc._B[0] = BMAX
    with pytest.raises(_lib.IrloscError, match="-3.*walls covers 130"):
        osc.set_episodes(big["q"], big["qd"], poses=big["poses"], **eps)
    osc._B[0] = B0
    assert np.array_equal(osc.episode_state()["count"], ep.schedule(ref["lengths"], ref["outcomes"], 40)["count"])
    b = osc.rollout_logged(60, ch)
    st = osc.episode_state()
    osc.close()
    te.assert_equals_stitched(a["log"], ref, sched, ticks=slice(0, 40))
    te.assert_equals_stitched(b["log"], ref, sched, ticks=slice(40, T))
    te.assert_state_is(st, sched, 60)


def test_a_second_set_episodes_starts_over():
    """40 ticks, then targets, list and episodes again: count and age 0, start_tick -1, the ring zero, the tick base 0 -- and 100 ticks
    that equal the stitched reference from its first tick, with start_ticks counted from the second call."""
    fl = te.fleet(B0)
    ref = te.fresh(fl, F64, "list", ())
    sched = ep.schedule(ref["lengths"], ref["outcomes"], T)
    osc = armed(fl)
    osc.rollout(40)
    assert osc.episode_state()["records"].any()
    te.set_slot_targets(osc, fl)
    te.arm_program(osc, fl, "list", 2)
    osc.set_episodes(fl["q"], fl["qd"], max_ticks=MAX_TICKS, poses=fl["poses"], records=RECORDS)
    st = osc.episode_state()
    assert not st["count"].any() and not st["age"].any() and (st["start_tick"] == -1).all() and not st["records"].any() and st["running"] == B0
    r = osc.rollout_logged(T, list(FRONT))
    st = osc.episode_state()
    osc.close()
    te.assert_equals_stitched(r["log"], ref, sched)
    te.assert_state_is(st, sched, T)


# ---- 8. the eigen pass's form under episodes ------------------------------------------------------------------------------------------------
def _eig_child():
    """A robot's bits depend on the form of the eigen pass its step ran, and the form on how many robots of the fleet are flagged on the
    tick -- a number that differs between a run with episodes and a fresh one.  Here the form is pinned (IRLOSC_LANE_EIG_MIN=0: the lane
    form whatever the number) and start 1 of every third robot has its active arm at multiples of pi / 2, where the step takes the eigen
    path: flagged robots come and go with the resets, and the run still equals its fresh rollouts bit for bit."""
    assert os.environ.get("IRLOSC_LANE_EIG_MIN") == "0"
    base = te.fleet(B0)
    rng = np.random.default_rng(82)
    idx = np.arange(2, 128, 3)
    q = np.array(base["q"])
    q[idx, 1, tal.RIGHT] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    fl = dict(base, q=q)
    ref, sched, out, st, _ = check(fl, F64, "list", (), key="eig")
    eig = (ref["log"]["flags"] & _lib.FLAG_EIGEN_PATH) != 0
    per_tick = ((ep.stitch({"flags": ref["log"]["flags"]}, sched)["flags"] & _lib.FLAG_EIGEN_PATH) != 0).sum(axis=1)      # (of the reference)
    assert eig[1].any(), "no fresh run from start 1 takes the eigen path"
    assert eig[1].any(axis=(0, 1)).sum() > eig[0].any(axis=(0, 1)).sum(), "start 1 flags no more robots than start 0"
    assert len(set(per_tick.tolist())) >= 3, "the number of flagged robots hardly changes along the stitched run"
    n0, n1 = (int(eig[s].any(axis=(0, 1)).sum()) for s in (0, 1))
    print(f"[eig child] robots on the eigen path in the fresh runs from start 0 / 1: {n0} / {n1}; flagged robots per tick of the stitched "
          f"run: {int(per_tick.min())} .. {int(per_tick.max())}")


def test_the_eigen_pass_pinned_to_one_form_in_a_child_process():
    """The eigen pass reads its environment once per process: _eig_child runs in a fresh child with IRLOSC_LANE_EIG_MIN=0, one child,
    under its own time limit (the pattern of test_resident_lane_edges)."""
    env = dict(os.environ)
    env.pop("IRLOSC_LANE_EIG_BLOCKS", None)
    env["IRLOSC_LANE_EIG_MIN"] = "0"
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--eig-child"]
    p = subprocess.run(args, env=env, cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=120)
    print(p.stdout[-600:])
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "[eig child]" in p.stdout


if __name__ == "__main__":
    if "--eig-child" in sys.argv:
        _eig_child()
