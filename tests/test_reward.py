"""The reward of a rollout on the GPU (-m gpu): irlosc_set_reward / irlosc_download_reward_state -- the reward kernel (csrc/osc_reward.hpp)
behind the give-up pass of a rollout tick, its log channel and the goal that ends an episode.  Every term kind against the NumPy mirror
(reward.reward_tick) BIT FOR BIT, one logged call against one-tick calls, robots independent of their neighbours, the goal next to
episodes (on a policy slot and with the MATED term), a robot that holds a NaN, and the state rules.

Shapes are tests/test_policy_noise.py's: B = 70 (one full wave and a ragged one of 6 robots) and B = 1; MAXB = 96, so the state planes
have a stride that is not B; float64 and float32 contexts; k13 (three devices) and r6 (one); T <= 12 ticks.  Scenes, nets, start states
and helpers are those of tests/test_policy.py, test_policy_noise.py, test_action_list.py and test_teleop_stream.py, by import."""
import ctypes as C

import numpy as np
import pytest

import test_action_list as tal
import test_joints as tjn
import test_policy as tpo
import test_policy_noise as tpn
from irl_control_amd import _lib, episodes as ep, object_loads as ol, objects as ob, reward as rw
from test_policy import CLIP, GRIP, layers_of, rig_of
from test_teleop_stream import ORIGIN, bits, same_bits, start_state, start_targets

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
F64, F32 = np.float64, np.float32
MAXB = 96
T = 8
GAMMA = 0.9375 + 2.0 ** -20      # not 1, and no power of two: every disc product rounds
_RUNS = {}


def points_of(B, per_robot, P=3):
    """[P, 3] for the fleet or [B, P, 3]: points near the arms' start EE positions, every word irrational enough to round."""
    rng = np.random.default_rng(77)
    base = np.array([0.3, -0.2, 0.6]) + rng.uniform(-0.3, 0.3, (P, 3))
    if not per_robot:
        return base
    return base[None] + np.random.default_rng(78).uniform(-0.1, 0.1, (B, P, 3))


def full_scene(osc, B, slot):
    """tests/test_policy.py's full scene (a zero feed with a sensed push on device 0, joint rows, an object in the right hand, its weight)
    with a MATE on top: the free object 1 is the plug, the carried object 0 the socket, the tolerance the fleet's median distance at the
    start -- so about half the robots are mated on tick 0, and the hand's motion can mate more."""
    q, qd = tpo.scene(osc, B, slot, True)
    ee = tal.ee_start(q, np.array(qd), "k13")
    pose0 = np.stack([ee[:, 0], ee[:, 1] + np.array([0.0, 0.0, 1.0, 0, 0, 0, 0])], axis=1)
    tol = float(np.median(np.linalg.norm(pose0[:, 1, :3] - pose0[:, 0, :3], axis=1)))
    objs = ob.ObjectSet(radius=[0.05, 0.05], grippers=[ob.Gripper(dev=0, joint=tjn.KNUCKLE["ur5right"], q_close=0.3, q_open=0.15)],
                        mates=[ob.Mate(plug=1, socket=0, tol_xyz=tol)])
    osc.set_objects(objs, pose0, slot=slot)
    osc.set_object_loads(ol.ObjectLoads(mass=[0.4, 0.0]), slot=slot)


def set_up(osc, B, slot, cfg, full, head, n_out=7):
    """Scene, the "odd" policy of tests/test_policy.py (qpos | plate -> 20 -> n_out) and, `head`, its Gaussian head."""
    if full:
        full_scene(osc, B, slot)
    else:
        tpo.scene(osc, B, slot, False)
    kw = dict(grip_dev=0, grip_close=GRIP[0], grip_open=GRIP[1]) if n_out == 7 else {}
    osc.set_policy(layers_of(31, (20,), n_out, seed=3), ("qpos", "plate"), ORIGIN, rig=rig_of(cfg), clip=CLIP, slot=slot, **kw)
    if head:
        osc.set_policy_noise(tpn.STD[:n_out], tpn.SEED, None, slot=slot)


def terms_of(full, ndev):
    """Eight terms, every kind and every point kind, weights of mixed sign (full: the scene with feed, objects and a mate); else the six
    kinds a bare policy slot has, over EE, TARGET and FIXED."""
    last = ndev - 1
    if full:
        return [rw.dist(rw.ee(0), rw.fixed(0), -1.25), rw.dist_sq(rw.target(1), rw.obj(0), 0.375), rw.ori(rw.ee(last), rw.target(last), -0.7),
                rw.act_sq(-0.01), rw.u_sq(1e-4), rw.force(0, -0.3), rw.mated(0, 2.5), rw.one(-0.05)]
    return [rw.dist(rw.ee(0), rw.fixed(2), -1.25), rw.dist_sq(rw.ee(last), rw.target(0), 0.375), rw.ori(rw.target(last), rw.ee(0), -0.7),
            rw.act_sq(-0.01), rw.u_sq(1e-4), rw.one(0.05), rw.dist_sq(rw.fixed(0), rw.fixed(1), 0.1)]


def channels_of(full):
    return ("ee_pose", "targets", "u") + (("wrench", "object_pose") if full else ())


def sources(log, osc, slot, full, head):
    """The mirror's inputs of one tick: that tick's log sample, the policy's action and the mates behind it."""
    src = dict(ee_pose=log["ee_pose"], targets=log["targets"], u=log["u"])
    src["act"] = osc.policy_noise_state(slot)["act"] if head else osc.policy_state(slot)["out"]
    if full:
        src.update(wrench=log["wrench"], object_pose=log["object_pose"], mated_tick=osc.object_state(slot)["mated_tick"])
    return src


def run(cfg, B, dtype, full, head, per_robot, goal=True):
    """The run tests a and b share: T x rollout_logged(1) under the policy and the reward, reward_state() behind every tick, and the
    mirror's state beside it."""
    key = (cfg, B, np.dtype(dtype).name, full, head, per_robot, goal)
    if key in _RUNS:
        return _RUNS[key]
    osc = tal.make_ctx(B, dtype, cfg=cfg, max_batch=MAXB, feed=full)
    n_out = 7 if cfg == "k13" else 6
    set_up(osc, B, 0, cfg, full, head, n_out)
    pts = points_of(B, per_robot and B > 1)
    # the goal: the first term (a distance) below a value that the fleet straddles on tick 0, held for two ticks
    desc = rw.Reward(terms_of(full, osc.layout.ndev), gamma=GAMMA, points=pts)
    osc.set_reward(desc)
    first = osc.reward_state()
    if goal:
        probe = osc.rollout_logged(1, ("ee_pose",))["log"]["ee_pose"][0]
        v0 = rw.term_values(rw.Reward(desc.terms[:1], points=pts), ee_pose=probe)[0]
        desc.goal_term, desc.goal_cmp, desc.goal_hold = 0, "<=", 2
        desc.goal_value = float(np.median(v0)) if B > 1 else float(v0[0]) * 1.5
        osc.close()
        osc = tal.make_ctx(B, dtype, cfg=cfg, max_batch=MAXB, feed=full)
        set_up(osc, B, 0, cfg, full, head, n_out)
        osc.set_reward(desc)
    st = rw.reward_state(B)
    rec = dict(dev=[], mir=[], q=[], qd=[], u=[], flags=[], tgt=[], pol=[])
    for _ in range(T):
        r = osc.rollout_logged(1, channels_of(full))
        st = rw.reward_tick(desc, st, **sources({k: v[0] for k, v in r["log"].items()}, osc, 0, full, head))
        rec["dev"].append(osc.reward_state()); rec["mir"].append(st)
        rec["q"].append(r["qpos"]); rec["qd"].append(r["qvel"]); rec["u"].append(r["u"]); rec["flags"].append(r["flags_any"])
        rec["tgt"].append(osc.download_targets()); rec["pol"].append(osc.policy_state())
    osc.close()
    _RUNS[key] = dict(rec=rec, first=first, desc=desc, n_out=n_out)
    return _RUNS[key]


CASES = [("k13", 70, F64, True, True, False), ("k13", 70, F32, True, False, True), ("r6", 70, F32, False, True, True),
         ("k13", 1, F64, False, False, False), ("k13", 70, F64, False, False, True)]


def assert_state(dev, mir, what):
    for k in ("r", "ret", "gret"):
        bad = np.nonzero(bits(dev[k]) != bits(mir[k]))[0]
        assert bad.size == 0, f"{what}: {k} of {len(bad)} robots differs; first robot {bad[0]}: device {dev[k][bad[0]].hex()}, mirror {mir[k][bad[0]].hex()}"
    for k in ("steps", "hold", "goal_step"):
        assert np.array_equal(dev[k], mir[k]), (what, k, dev[k], mir[k])


# ---- a. the kernel against the mirror, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype,full,head,per_robot", CASES)
def test_every_term_and_the_accumulation_equal_the_mirror_bit_for_bit(cfg, B, dtype, full, head, per_robot):
    """r, ret, gret (uint64 views), steps, hold and goal_step of every robot behind every tick == reward.reward_tick on that tick's log
    sample, the policy's action and the mates; the setter left the fresh state."""
    rn = run(cfg, B, dtype, full, head, per_robot)
    f = rn["first"]
    assert not f["r"].any() and not f["ret"].any() and not f["gret"].any() and not f["steps"].any() and not f["hold"].any()
    assert (f["goal_step"] == -1).all() and not f["records"].any() and f["records"].shape == (B, 16, 2)
    kinds = {t[0] for t in rn["desc"].terms}
    assert kinds == (set(range(8)) if full else {rw.DIST, rw.DIST_SQ, rw.ORI, rw.ACT_SQ, rw.U_SQ, rw.ONE})
    for t in range(T):
        assert_state(rn["rec"]["dev"][t], rn["rec"]["mir"][t], f"tick {t}")
        assert (rn["rec"]["dev"][t]["steps"] == t + 1).all()
    v = np.array([m["v"] for m in rn["rec"]["mir"]])      # [T, terms, B]
    assert np.isfinite(v).all() and (v[:, [i for i, t in enumerate(rn["desc"].terms) if t[0] not in (rw.ONE, rw.MATED)]] != 0).any(axis=(0, 2)).all()
    last = rn["rec"]["dev"][-1]
    assert not np.array_equal(bits(last["ret"]), bits(last["gret"]))      # the discount shows
    if B > 1:       # the goal splits the fleet, and hold counts: a robot reaches it on step 2 at the earliest
        gs = last["goal_step"]
        assert (gs >= 2).any() and (gs < 0).any(), gs
    if full:        # the mate and the sensed push show in their terms
        mt = v[:, 6]
        assert (mt == 1).any() and (mt == 0).any() and (v[:, 5] != 0).any()


def test_shared_and_per_robot_points_give_different_rewards():
    a, b = run("k13", 70, F64, False, False, False), run("k13", 70, F64, False, False, True)
    assert (a["rec"]["dev"][0]["r"] != b["rec"]["dev"][0]["r"]).all()
    assert np.asarray(a["desc"].points).ndim == 2 and np.asarray(b["desc"].points).shape == (70, 3, 3)


# ---- b. one logged call equals the one-tick calls; the reward changes nothing else ---------------------------------------------------------
@pytest.mark.parametrize("robots", [[0, 5, 64, 69], None])
def test_the_logs_reward_plane_equals_the_states_behind_one_tick_calls(robots):
    B, full, head = 70, True, True
    rn = run("k13", B, F64, full, head, False)
    rows = slice(None) if robots is None else robots
    osc = tal.make_ctx(B, F64, max_batch=MAXB, feed=True)
    set_up(osc, B, 0, "k13", full, head)
    osc.set_reward(rn["desc"])
    r = osc.rollout_logged(T, ("u", "reward"), robots=robots)
    end = osc.reward_state()
    osc.close()
    plane = r["log"]["reward"]
    assert plane.shape == (T, B if robots is None else 4, 4) and plane.dtype == F64
    for t in range(T):
        d = rn["rec"]["dev"][t]
        assert same_bits(plane[t, :, 0], d["r"][rows]) and same_bits(plane[t, :, 1], d["ret"][rows]), t
        assert np.array_equal(plane[t, :, 2], d["steps"][rows].astype(F64)) and np.array_equal(plane[t, :, 3], (d["goal_step"][rows] >= 0).astype(F64)), t
        assert same_bits(r["log"]["u"][t], rn["rec"]["u"][t][rows]), t
    assert_state(end, rn["rec"]["dev"][-1], "after the logged call")
    assert same_bits(r["qpos"], rn["rec"]["q"][-1]) and same_bits(r["u"], rn["rec"]["u"][-1])


@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_slot_with_a_goalless_reward_rolls_out_like_one_without(dtype):
    """q, qd, u, flags, targets and the policy's state of a slot with a reward (logged, the reward channel included) are bit for bit
    those of the same slot without one."""
    B = 70
    res = []
    for with_reward in (False, True):
        osc = tal.make_ctx(B, dtype, max_batch=MAXB, feed=True)
        set_up(osc, B, 0, "k13", True, True)
        if with_reward:
            osc.set_reward(rw.Reward(terms_of(True, 3), gamma=GAMMA, points=points_of(B, True)))
        out = osc.rollout_logged(T, ("qpos", "u") + (("reward",) if with_reward else ()))
        res.append(tpn.state_of(osc, out) + [out["flags_any"], out["log"]["qpos"], out["log"]["u"]])
        osc.close()
    for k, (x, y) in enumerate(zip(*res)):
        assert same_bits(x, y), k


# ---- c. independence ----------------------------------------------------------------------------------------------------------------------------
def test_a_robots_reward_does_not_depend_on_its_neighbours():
    """The first 6 robots run alone with B = 6 give the bits they give inside B = 70."""
    B, few = 70, 6
    q, qd = start_state(B)
    pts = points_of(B, True)
    res = []
    for nb in (B, few):
        osc = tal.make_ctx(nb, F64, max_batch=MAXB)
        osc.upload_q(np.array(q)[:nb], np.array(qd)[:nb])
        osc.set_targets(start_targets(B, 3)[:nb])
        osc.set_policy(layers_of(31, (20,), 6, seed=3), ("qpos", "plate"), ORIGIN, rig=rig_of("k13"), clip=CLIP)
        osc.set_reward(rw.Reward(terms_of(False, 3), gamma=GAMMA, points=pts[:nb], goal_term=0, goal_value=0.6, goal_hold=2))
        osc.rollout(T)
        res.append(osc.reward_state())
        osc.close()
    for k in ("r", "ret", "gret", "steps", "hold", "goal_step"):
        assert same_bits(res[0][k][:few], res[1][k]), k
    assert res[1]["ret"].all() and len(np.unique(bits(res[1]["ret"]))) == few


# ---- d. the goal and episodes -----------------------------------------------------------------------------------------------------------------
def windowed(v, H):
    """[B]: the smallest value g for which `v <= g` holds on H consecutive ticks of v [T, B]."""
    return np.min([np.max(v[t:t + H], axis=0) for t in range(len(v) - H + 1)], axis=0)


def goal_run(kind, H):
    """-> what test d checks.  kind "policy": a policy slot, the goal a distance of EE 0 to a per-robot point; "mated": no program, two
    free objects that are mated from tick 0 for every other robot, the goal MATED >= a value between 0 and 1."""
    key = ("goal", kind, H)
    if key in _RUNS:
        return _RUNS[key]
    B, TT, MAX_TICKS = 70, 12, 5
    q, qd = start_state(B)
    pts = points_of(B, True)
    ch = ("qpos", "u", "targets", "ee_pose", "reward")

    def scene(osc, slot):
        if kind == "policy":
            tpo.small(osc, B, slot=slot, n_out=6)
            return
        tpo.scene(osc, B, slot, False)
        ee = tal.ee_start(np.array(q), np.array(qd), "k13")
        off = np.where(np.arange(B) % 2 == 0, 0.001, 0.1)
        pose0 = np.stack([ee[:, 0] + np.array([0.0, 0.0, 1.0, 0, 0, 0, 0]), ee[:, 0] + np.array([0.0, 0.0, 1.0, 0, 0, 0, 0])], axis=1)
        pose0[:, 1, 0] += off
        objs = ob.ObjectSet(radius=[0.05, 0.05], grippers=[ob.Gripper(dev=0, joint=tjn.KNUCKLE["ur5right"], q_close=0.3, q_open=0.15)],
                            mates=[ob.Mate(plug=0, socket=1, tol_xyz=0.01)])
        osc.set_objects(objs, pose0, slot=slot)

    terms = [rw.dist(rw.ee(0), rw.fixed(1), -1.0), rw.u_sq(-1e-5), rw.one(0.25)] + ([rw.mated(0, 1.5)] if kind == "mated" else [rw.act_sq(-0.01)])
    gt = 3 if kind == "mated" else 0
    osc = tal.make_ctx(B, F64, n_slots=3, max_batch=MAXB)
    # a first pass without a goal: the goal term's values of a fresh rollout
    scene(osc, 0)
    osc.set_reward(rw.Reward(terms, gamma=GAMMA, points=pts))
    fresh = osc.rollout_logged(TT, ch)["log"]
    if kind == "mated":
        v = np.array([fresh["reward"][t, :, 0] for t in range(TT)])      # (only to size the arrays below)
        mt = osc.object_state()["mated_tick"][:, 0]
        v = np.where((mt >= 0)[None] & (np.arange(TT)[:, None] >= mt[None]), 1.0, 0.0)
        cmp_, value = ">=", 0.5
        reach = -windowed(-v[:MAX_TICKS], H)
        reached = reach >= value
    else:
        v = np.array([rw.term_values(rw.Reward(terms[:1], points=pts), ee_pose=fresh["ee_pose"][t])[0] for t in range(TT)])
        w = np.sort(windowed(v[:MAX_TICKS], H))
        cmp_, value = "<=", float(0.5 * (w[B // 2 - 1] + w[B // 2]))
        assert w[B // 2 - 1] < value < w[B // 2]
        reached = windowed(v[:MAX_TICKS], H) <= value
    assert reached.any() and (~reached).any()
    met = (v >= value) if cmp_ == ">=" else (v <= value)
    goal_step = np.full(B, -1)
    for b in range(B):
        hold = 0
        for t in range(TT):
            hold = hold + 1 if met[t, b] else 0
            if hold >= H:
                goal_step[b] = t + 1
                break
    lengths, outcomes = ep.lengths_from_goal(goal_step, MAX_TICKS)
    if kind == "mated":     # a slot with mates: every mate mated on the ending tick adds INSERTED (include/irlosc.h, "action objects")
        outcomes = np.where(reached, outcomes | _lib.EPISODE_INSERTED, outcomes)
    desc = rw.Reward(terms, gamma=GAMMA, points=pts, goal_term=gt, goal_cmp=cmp_, goal_value=value, goal_hold=H)
    # the run with episodes: one start state per robot, so every episode repeats the fresh rollout
    scene(osc, 1)
    osc.set_reward(desc, slot=1)
    osc.set_episodes(np.array(q)[:, None], max_ticks=MAX_TICKS, records=4, slot=1)
    got = osc.rollout_logged(TT, ch, slot=1)
    es, rs = osc.episode_state(1), osc.reward_state(1)
    # ... and one that parks every robot after its first episode and polls every 2 ticks
    scene(osc, 2)
    osc.set_reward(desc, slot=2)
    osc.set_episodes(np.array(q)[:, None], max_ticks=MAX_TICKS, max_episodes=1, poll_every=2, slot=2)
    parked = osc.rollout_logged(TT, ("reward",), slot=2)
    es2, rs2 = osc.episode_state(2), osc.reward_state(2)
    osc.close()
    _RUNS[key] = dict(B=B, TT=TT, MAX_TICKS=MAX_TICKS, fresh=fresh, got=got, es=es, rs=rs, parked=parked, es2=es2, rs2=rs2, lengths=lengths,
                      outcomes=outcomes, goal_step=goal_step, desc=desc, reached=reached)
    return _RUNS[key]


@pytest.mark.parametrize("kind,H", [("policy", 1), ("policy", 3), ("mated", 1), ("mated", 3)])
def test_a_goal_ends_the_episode_on_its_tick_and_every_episode_is_a_fresh_rollout(kind, H):
    g = goal_run(kind, H)
    B, TT, L, fresh, got = g["B"], g["TT"], g["lengths"], g["fresh"], g["got"]
    assert (L[g["reached"]] < g["MAX_TICKS"]).any()      # episodes -- a policy slot's too -- end before max_ticks
    assert (L[g["reached"]] >= H).all() and (L[~g["reached"]] == g["MAX_TICKS"]).all()
    GOAL, FIN, TMO = _lib.EPISODE_GOAL, _lib.EPISODE_FINISHED, _lib.EPISODE_TIMEOUT
    assert set(np.unique(g["outcomes"])) == {FIN | GOAL | (_lib.EPISODE_INSERTED if kind == "mated" else 0), TMO}
    for b in range(B):
        n = TT // L[b]
        assert g["es"]["count"][b] == n and g["es"]["age"][b] == TT % L[b], b
        st = rw.reward_state(1)
        for t in range(TT):
            age = t % L[b]
            if age == 0:
                st = rw.reward_state(1)
            # every episode repeats the fresh rollout's first L[b] ticks, bit for bit -- the reward's r, ret and steps among them
            for c in ("qpos", "u", "targets", "ee_pose"):
                assert same_bits(got["log"][c][t, b], fresh[c][age, b]), (b, t, c)
            assert same_bits(got["log"]["reward"][t, b, :3], fresh["reward"][age, b, :3]), (b, t)
            ends_goal = g["reached"][b] and age == L[b] - 1
            assert got["log"]["reward"][t, b, 3] == float(ends_goal), (b, t)      # goal_step >= 0 shows on the ending tick alone
            st = rw.accumulate(g["desc"], st, got["log"]["reward"][t, b, :1], np.array([np.nan]))
            if age == L[b] - 1:     # the ending tick: its record, and (ret, gret) == the mirror's accumulation of the logged r
                e = t // L[b]
                if e >= n - 4:
                    rec = g["es"]["records"][b, e % 4]
                    assert tuple(rec[:3]) == (e * L[b], L[b], g["outcomes"][b]), (b, e, rec)
                    assert same_bits(g["rs"]["records"][b, e % 4], np.array([st["ret"][0], st["gret"][0]])), (b, e)
        # behind the call: the running episode's sums (fresh behind a reset on the last tick)
        tail = TT % L[b]
        assert g["rs"]["steps"][b] == tail, b
        if tail == 0:
            assert g["rs"]["ret"][b] == 0 and g["rs"]["gret"][b] == 0 and g["rs"]["r"][b] == 0 and g["rs"]["goal_step"][b] == -1 and g["rs"]["hold"][b] == 0
        else:
            assert same_bits(g["rs"]["ret"][b:b + 1], st["ret"]) and same_bits(g["rs"]["gret"][b:b + 1], st["gret"])
    assert (TT % L == 0).any() and (TT % L != 0).any()      # (robots fresh behind a reset on the last tick, and robots mid-episode)
    assert not g["rs"]["records"][:, 4:].any()      # entries beyond the episodes' `records`: zero


@pytest.mark.parametrize("kind,H", [("policy", 1), ("mated", 3)])
def test_a_fleet_that_reached_its_goal_exits_early_and_parked_robots_go_on_accumulating(kind, H):
    g = goal_run(kind, H)
    L, TT = g["lengths"], g["TT"]
    want = ep.ticks_run(L - 1, TT, 2)
    assert want < TT and g["parked"]["ticks_run"] == want == g["es2"]["ticks_run"] and g["es2"]["running"] == 0
    assert (g["es2"]["count"] == 1).all() and np.array_equal(g["es2"]["records"][:, 0, 1], L) and np.array_equal(g["es2"]["records"][:, 0, 2], g["outcomes"])
    plane = g["parked"]["log"]["reward"]
    assert len(plane) == want
    for b in range(g["B"]):
        assert same_bits(g["rs2"]["records"][b, 0, 0], plane[L[b] - 1, b, 1])          # the record: ret on the ending tick
        assert g["rs2"]["steps"][b] == want and same_bits(g["rs2"]["ret"][b], plane[want - 1, b, 1])      # a parked robot goes on
    assert not g["rs2"]["records"][:, 1:].any()


# ---- e. a robot that holds a NaN --------------------------------------------------------------------------------------------------------------
def test_a_robot_with_a_nan_coordinate_has_a_nan_reward_never_reaches_the_goal_and_leaves_its_neighbours_alone():
    B, sick = 70, 3
    q, qd = start_state(B)
    res = {}
    for nan, with_reward in ((False, True), (True, True), (True, False)):
        qq = np.array(q)
        if nan:
            qq[sick, 2] = np.nan
        osc = tal.make_ctx(B, F64, max_batch=MAXB)
        tpo.small(osc, B, n_out=6)
        osc.upload_q(qq, qd)
        if with_reward:
            osc.set_reward(rw.Reward([rw.dist(rw.ee(0), rw.fixed(0), -1.0), rw.u_sq(1e-4), rw.one(1.0)], gamma=GAMMA, points=points_of(B, False),
                                     goal_term=0, goal_value=1e3))
        out = osc.rollout(T)
        res[(nan, with_reward)] = (osc.reward_state() if with_reward else None, out)
        osc.close()
    (clean, _), (ill, out_ill), (_, out_bare) = res[(False, True)], res[(True, True)], res[(True, False)]
    others = np.arange(B) != sick
    assert np.isnan(ill["r"][sick]) and np.isnan(ill["ret"][sick]) and np.isnan(ill["gret"][sick]) and ill["goal_step"][sick] == -1 and ill["hold"][sick] == 0
    assert ill["steps"][sick] == T and (clean["goal_step"] == 1).all() and np.isfinite(clean["ret"]).all()
    for k in ("r", "ret", "gret", "steps", "hold", "goal_step"):
        assert same_bits(clean[k][others], ill[k][others]), k
    assert np.array_equal(out_ill["flags_any"], out_bare["flags_any"]) and same_bits(out_ill["u"], out_bare["u"]) and same_bits(out_ill["qpos"], out_bare["qpos"])


# ---- f. state rules ------------------------------------------------------------------------------------------------------------------------------
def test_state_rules():
    B = 70
    osc = tal.make_ctx(B, F64, n_slots=2, max_batch=MAXB, feed=True)
    lib, h = osc.lib, osc._h
    pts = points_of(B, False)
    good = rw.Reward(terms_of(True, 3), gamma=GAMMA, points=pts, goal_term=0, goal_value=0.5, goal_hold=2)

    def set_rw(desc=None, points=pts, n=B, slot=0, **edit):
        d = (good if desc is None else desc).desc()
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return lib.irlosc_set_reward(h, slot, n, C.byref(d), _lib.ptr(None if points is None else np.ascontiguousarray(points, dtype=F64)))

    def state_rc(n=B, slot=0):
        return lib.irlosc_download_reward_state(h, slot, n, None, None, None, None, None, None, None)

    def logged(slot, channels, n=B):
        lg = _lib.Log(channels, 1, 0, 0, 0)
        return lib.irlosc_rollout_from_q_logged(h, slot, n, 1, C.byref(lg), None, _lib.ptr(np.zeros((1, B * 256))), None, None)

    # a bare slot (no targets yet): every reward is IRLOSC_ERR_STATE; the NULL description is accepted and does nothing
    assert state_rc() == ERR_STATE and "irlosc_set_reward" in lib.irlosc_last_error(h).decode()
    assert set_rw(rw.Reward([rw.one(1.0)])) == ERR_STATE and lib.irlosc_set_reward(h, 0, B, None, None) == 0
    assert set_rw(slot=5) == ERR_ARG and lib.irlosc_set_reward(None, 0, B, None, None) == ERR_ARG
    # slot 1: targets and coordinates only -- what a term names has to be there (IRLOSC_ERR_STATE, with the reason)
    tpo.scene(osc, B, 1, False)
    for term, word in ((rw.act_sq(1.0), "irlosc_set_policy"), (rw.force(0, 1.0), "irlosc_set_sensordata"), (rw.mated(0, 1.0), "irlosc_set_objects"),
                       (rw.dist(rw.ee(0), rw.obj(0), 1.0), "irlosc_set_objects")):
        assert set_rw(rw.Reward([term]), slot=1) == ERR_STATE and word in lib.irlosc_last_error(h).decode(), term
    assert state_rc(slot=1) == ERR_STATE and logged(1, 4096) == ERR_ARG and logged(1, 1 | 4096) == ERR_ARG      # no reward: an unknown bit
    assert set_rw(rw.Reward([rw.dist(rw.ee(2), rw.target(0), 1.0)]), points=None, slot=1) == 0 and logged(1, 4096) == 0
    # the full scene on slot 0, a reward of 60 robots with a goal; every refusal leaves it in force, whole
    set_up(osc, B, 0, "k13", True, True)
    assert set_rw(n=60) == 0 and state_rc(60) == 0 and state_rc(61) == ERR_STATE
    assert lib.irlosc_rollout_from_q(h, 0, 60, 3, 0, None, None, None) == 0
    assert lib.irlosc_rollout_from_q(h, 0, 61, 1, 0, None, None, None) == ERR_STATE      # the reward covers 60

    def held():
        r, ret, gret = np.empty(60), np.empty(60), np.empty(60)
        steps, hold, gs = np.empty(60, np.int32), np.empty(60, np.int32), np.empty(60, np.int32)
        assert lib.irlosc_download_reward_state(h, 0, 60, *(_lib.ptr(x) for x in (r, ret, gret, steps, hold, gs)), None) == 0
        return r, ret, gret, steps, hold, gs

    was = held()
    assert (was[3] == 3).all() and was[1].all()
    bad = [dict(n_terms=0), dict(n_terms=9), dict(n_points=-1), dict(n_points=9), dict(points_per_robot=2), dict(reserved=(0, 1)), dict(reserved=(1, 1)),
           dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=np.nan), dict(goal_term=8), dict(goal_term=-2), dict(goal_cmp=2), dict(goal_hold=0),
           dict(goal_value=np.inf), dict(goal_value=np.nan), dict(weight=(2, np.nan)), dict(weight=(0, np.inf)), dict(kind=(0, 8)), dict(kind=(0, -1)),
           dict(a_kind=(0, 4)), dict(a_index=(0, 3)), dict(a_index=(0, -1)), dict(b_index=(0, 3)), dict(b_index=(1, 4)), dict(a_index=(5, 3)),
           dict(a_index=(6, 2)), dict(b_kind=(2, _lib.REWARD_FIXED)), dict(a_kind=(3, 1)), dict(b_index=(7, 1)), dict(points=None)]
    for edit in bad:
        kw = dict(edit)
        points = kw.pop("points", pts)
        assert set_rw(points=points, n=60, **kw) == ERR_ARG, (edit, lib.irlosc_last_error(h).decode())
    assert set_rw(points=np.where(np.arange(9).reshape(3, 3) == 4, np.nan, pts), n=60) == ERR_ARG
    assert set_rw(rw.Reward([rw.one(1.0)], goal_term=1), n=60) == ERR_ARG                      # a goal_term outside the terms
    assert set_rw(rw.Reward([rw.one(1.0), rw.one(0.0)]), n=60, n_terms=1, weight=(1, 1.0)) == ERR_ARG      # a term behind n_terms that is not zero
    assert set_rw(n=0) == ERR_ARG and set_rw(n=MAXB + 1) == ERR_ARG
    assert set_rw(rw.Reward([rw.mated(1, 1.0)]), n=60) == ERR_STATE and set_rw(rw.Reward([rw.dist(rw.obj(2), rw.ee(0), 1.0)]), n=60) == ERR_STATE
    # FORCE on a device the feed has no force sensor for (the base of k13 has none): the slot lacks the part
    assert set_rw(rw.Reward([rw.force(2, 1.0)]), n=60) == ERR_STATE and "no force sensor" in lib.irlosc_last_error(h).decode()
    # a context without a model: no reward (and nothing to leave untouched)
    bare = tal.BatchedOSC(osc.layout, MAXB, dtype=F64)
    one = rw.Reward([rw.one(1.0)]).desc()
    assert bare.lib.irlosc_set_reward(bare._h, 0, 4, C.byref(one), None) == ERR_STATE and "irlosc_set_model" in bare.lib.irlosc_last_error(bare._h).decode()
    assert bare.lib.irlosc_download_reward_state(bare._h, 0, 4, None, None, None, None, None, None, None) == ERR_STATE
    bare.close()
    now = held()
    assert all(same_bits(a, b) for a, b in zip(was, now))
    assert lib.irlosc_rollout_from_q(h, 0, 60, 1, 0, None, None, None) == 0 and (held()[3] == 4).all()      # the reward went on, whole
    # the old layout functions refuse bit 4096; only irlosc_log_layout_reward with rewarded == 1 knows it
    off, words = (C.c_int64 * 13)(), C.c_int64(0)
    assert lib.irlosc_log_layout(25, 3, 4096, 4, off, C.byref(words)) == ERR_ARG and lib.irlosc_log_layout_objects(25, 3, 2, 4096, 4, off, C.byref(words)) == ERR_ARG
    assert lib.irlosc_log_layout_policy(25, 3, 2, 7, 1, 4096, 4, off, C.byref(words)) == ERR_ARG
    assert lib.irlosc_log_layout_reward(25, 3, 2, 7, 1, 0, 4096, 4, off, C.byref(words)) == ERR_ARG
    assert lib.irlosc_log_layout_reward(25, 3, 2, 7, 1, 1, 4096 | 1, 4, off, C.byref(words)) == 0 and (off[0], off[12], words.value) == (0, 100, 116)
    # a part that a reward names is ended under it: the rollout is refused with the reason, the reward stays, and comes back with the part
    assert logged(0, 4096, 60) == 0
    osc.set_policy_noise(None)                     # (the head alone: ACT_SQ reads out instead)
    assert lib.irlosc_rollout_from_q(h, 0, 60, 1, 0, None, None, None) == 0
    osc.clear_policy()
    assert lib.irlosc_rollout_from_q(h, 0, 60, 1, 0, None, None, None) == ERR_STATE and "irlosc_set_policy" in lib.irlosc_last_error(h).decode()
    assert state_rc(60) == 0 and (held()[3] == 6).all()
    osc.set_policy(layers_of(31, (20,), 6, seed=3), ("qpos", "plate"), ORIGIN, rig=rig_of("k13"), clip=CLIP)
    osc.set_objects(None, None)
    assert lib.irlosc_rollout_from_q(h, 0, 60, 1, 0, None, None, None) == ERR_STATE and "irlosc_set_objects" in lib.irlosc_last_error(h).decode()
    # success replaces the reward and makes its state fresh; episodes for more robots than the reward covers are refused, and the reverse
    assert set_rw(rw.Reward([rw.u_sq(1.0)]), points=None, n=60) == 0 and not held()[3].any() and (held()[5] == -1).all()
    osc.clear_pushes()                             # (episodes are refused next to pushes)
    with pytest.raises(_lib.IrloscError, match="reward"):
        osc.set_episodes(np.array(start_state(B)[0])[:, None], max_ticks=4)
    assert set_rw(rw.Reward([rw.u_sq(1.0)]), points=None) == 0
    osc.set_episodes(np.array(start_state(B)[0])[:, None], max_ticks=4)
    assert set_rw(rw.Reward([rw.u_sq(1.0)]), points=None, n=60) == ERR_STATE and state_rc(B) == 0
    # episodes that cover fewer robots than a download: the ring is masked per robot -- the covered robots' records count, the others' are zero
    q60 = np.ascontiguousarray(np.array(start_state(B)[0])[:60, None])
    ed = _lib.Episodes(4, 1, 0, 1, 1, 0, 4, 0, 0)
    assert lib.irlosc_set_episodes(h, 0, 60, C.byref(ed), _lib.ptr(q60), _lib.ptr(np.zeros_like(q60)), None) == 0
    assert lib.irlosc_rollout_from_q(h, 0, 60, 4, 0, None, None, None) == 0
    ring = osc.reward_state()["records"]
    assert ring[:60, 0, 0].all() and not ring[:60, 1:].any() and not ring[60:].any()
    # desc == NULL ends the reward, after which bit 4096 is refused; irlosc_set_model ends it too
    assert lib.irlosc_set_reward(h, 0, B, None, None) == 0 and state_rc() == ERR_STATE and logged(0, 4096, 60) == ERR_ARG      # (the episodes cover 60)
    assert state_rc(slot=1) == 0
    osc.set_model(tal.RigidBodyModel.load("dual_ur5"))
    assert state_rc(slot=1) == ERR_STATE
    osc.close()
