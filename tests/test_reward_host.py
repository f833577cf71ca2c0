"""The reward of a rollout, the host side (no GPU): the ABI (struct irlosc_reward, the three exports, the constants), the log layout with
the reward channel (irlosc_log_layout_reward is context-free) against rollout_log.layout, and the NumPy mirror (reward.reward_tick) against
exact rational arithmetic on random data and against a three-term example computed by hand.

BOUNDS, with u = 2^-53 the unit roundoff of float64 and every figure held to 1.01 times its first-order bound (the (1 + u)^k - 1 = k u
(1 + O(k u)) of at most k = 2 N = 400 roundings):
    r     = the chain r = r + w_i v_i over n terms: every addend passes one product and at most n sums   -> (n + 1) u sum |w_i v_i|
    ret   = N sequential sums of the r_t                                                                -> (N - 1) u sum |r_t|
    gret  = sum of disc_t r_t with disc_t = gamma^t from t rounded products: an addend passes t + 1 products and at most N - 1 sums
                                                                                                        -> 2 N u sum |gamma^t r_t|
The references are Fractions of the float64 inputs: exact."""
import ctypes as C
import fnmatch
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from irl_control_amd import _lib, episodes as ep, reward as rw, rollout_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ("irlosc_set_reward", "irlosc_download_reward_state", "irlosc_log_layout_reward")
U = 2.0 ** -53


def header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def c_layout(n, ndev, nobj, n_out, sampled, rewarded, channels, R):
    lib = _lib.load()
    off, words = np.full(13, -7, dtype=np.int64), C.c_int64(-7)
    rc = lib.irlosc_log_layout_reward(n, ndev, nobj, n_out, sampled, rewarded, channels, R, _lib.ptr(off), C.addressof(words))
    return rc, off, words.value


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_exports_and_the_struct_is_272_bytes():
    hdr = header()
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), name
        assert re.search(r"IRLOSC_API int %s\(" % name, hdr), name
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 3 and re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", hdr)
    S = _lib.Reward
    assert C.sizeof(S) == 272
    assert {f: getattr(S, f).offset for f, _ in S._fields_} == dict(n_terms=0, n_points=4, points_per_robot=8, goal_term=12, goal_cmp=16, goal_hold=20,
                                                                     kind=24, a_kind=56, a_index=88, b_kind=120, b_index=152, reserved=184, weight=192,
                                                                     gamma=256, goal_value=264)
    body = re.search(r"typedef struct irlosc_reward \{(.*?)\} irlosc_reward;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    T = "IRLOSC_MAX_REWARD_TERMS"
    assert re.findall(r"(int32_t|double)\s+(\w+)(?:\[(\w+)\])?;", body) == [
        ("int32_t", "n_terms", ""), ("int32_t", "n_points", ""), ("int32_t", "points_per_robot", ""), ("int32_t", "goal_term", ""),
        ("int32_t", "goal_cmp", ""), ("int32_t", "goal_hold", ""), ("int32_t", "kind", T), ("int32_t", "a_kind", T), ("int32_t", "a_index", T),
        ("int32_t", "b_kind", T), ("int32_t", "b_index", T), ("int32_t", "reserved", "2"), ("double", "weight", T), ("double", "gamma", ""),
        ("double", "goal_value", "")]
    for name, value, mine in (("LOG_REWARD", "4096u", _lib.LOG_REWARD), ("EPISODE_GOAL", "8", _lib.EPISODE_GOAL), ("MAX_REWARD_TERMS", "8", _lib.MAX_REWARD_TERMS),
                              ("MAX_REWARD_POINTS", "8", _lib.MAX_REWARD_POINTS)):
        m = re.search(r"#define\s+IRLOSC_%s\s+(\w+)" % name, hdr)
        assert m and m.group(1) == value and int(value.rstrip("u")) == mine, name
    for i, name in enumerate(("EE", "TARGET", "OBJECT", "FIXED")):
        assert re.search(r"#define\s+IRLOSC_REWARD_%s\s+%d\b" % (name, i), hdr) and getattr(_lib, "REWARD_" + name) == i == getattr(rw, name)
    for i, name in enumerate(("DIST_SQ", "DIST", "ORI", "ACT_SQ", "U_SQ", "FORCE", "MATED", "ONE")):
        assert re.search(r"#define\s+IRLOSC_REWARD_%s\s+%d\b" % (name, i), hdr) and getattr(_lib, "REWARD_" + name) == i == getattr(rw, name)
    assert rollout_log.mask("reward") == 4096 and ep.GOAL == 8
    assert rollout_log.CHANNELS == ("qpos", "qvel", "ee_pose", "targets", "wrench", "u", "flags", "wall_force", "joint_tau") and rollout_log.ALL == 511
    # the rules a caller and the mirror need stand in the header
    for words in ("NON-FINITE REWARD IS STORED AS COMPUTED AND SETS NO FLAG", "PARKED robot goes on", "NOT OFFERED", "r_t = R(the state tick t observed"):
        assert words in hdr, words


def test_the_builder_fills_the_struct():
    r = rw.Reward([rw.dist(rw.ee(1), rw.fixed(2), -1.5), rw.ori(rw.obj(3), rw.target(0), 0.25), rw.force(2, 3.0), rw.mated(1, 4.0), rw.one(-1.0)], gamma=0.5,
                  points=np.zeros((5, 3)), goal_term=1, goal_cmp=">=", goal_value=0.75, goal_hold=3)
    d = r.desc()
    assert (d.n_terms, d.n_points, d.points_per_robot, d.goal_term, d.goal_cmp, d.goal_hold) == (5, 5, 0, 1, 1, 3)
    assert (d.gamma, d.goal_value, d.reserved[0], d.reserved[1]) == (0.5, 0.75, 0, 0)
    assert list(d.kind) == [1, 2, 5, 6, 7, 0, 0, 0] and list(d.a_kind) == [0, 2, 0, 0, 0, 0, 0, 0] and list(d.a_index) == [1, 3, 2, 1, 0, 0, 0, 0]
    assert list(d.b_kind) == [3, 1, 0, 0, 0, 0, 0, 0] and list(d.b_index) == [2, 0, 0, 0, 0, 0, 0, 0] and list(d.weight) == [-1.5, 0.25, 3.0, 4.0, -1.0, 0, 0, 0]
    assert rw.Reward([rw.one(1.0)], points=np.zeros((70, 2, 3))).desc().points_per_robot == 1
    with pytest.raises(ValueError):
        rw.Reward([rw.one(1.0)] * 9).desc()
    with pytest.raises(ValueError):
        rw.Reward([rw.one(1.0)], goal_cmp="<").desc()


# ---- the log layout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ndev,nobj,n_out,sampled", [(25, 3, 0, 0, 0), (25, 3, 2, 7, 1), (25, 1, 0, 6, 0)])
@pytest.mark.parametrize("R", [1, 65])
def test_the_layout_with_the_reward_channel_equals_its_numpy_mirror(n, ndev, nobj, n_out, sampled, R):
    width = [n, n, ndev * 7, ndev * 7, ndev * 6, n, 1, ndev * 3, n, nobj * 8, n_out, n_out + 1, 4]
    every = 511 | (512 if nobj else 0) | (1024 if n_out else 0) | (2048 if sampled else 0) | 4096
    for channels in (4096, 1 | 4096, 32 | 64 | 4096, every, ("u", "reward")):
        m = rollout_log.mask(channels)
        rc, off, words = c_layout(n, ndev, nobj, n_out, sampled, 1, m, R)
        assert rc == 0
        moff, mwords = rollout_log.layout(n, ndev, channels, R, nobj, n_out, bool(sampled), True)
        assert len(moff) == 13 and np.array_equal(off, moff) and words == mwords, channels
        at = 0
        for i in range(13):
            if (m >> i) & 1:
                assert off[i] == at
                at += R * width[i]
            else:
                assert off[i] == -1
        assert words == at
    assert rollout_log.names(4096 | 32) == ("u", "reward") and rollout_log.shape("reward", n, ndev) == (4,)
    # without a reward the bit is unknown and the first twelve offsets are irlosc_log_layout_policy's
    lib = _lib.load()
    known = every & ~4096
    rc, off, words = c_layout(n, ndev, nobj, n_out, sampled, 0, known, R)
    off12, words12 = np.full(12, -7, dtype=np.int64), C.c_int64(-7)
    assert lib.irlosc_log_layout_policy(n, ndev, nobj, n_out, sampled, known, R, _lib.ptr(off12), C.addressof(words12)) == 0
    assert rc == 0 and np.array_equal(off[:12], off12) and off[12] == -1 and words == words12.value


def test_layout_refusals_and_the_older_layouts_refuse_the_bit():
    lib = _lib.load()
    off, words = np.zeros(13, dtype=np.int64), C.c_int64(0)
    assert c_layout(25, 3, 0, 0, 0, 0, 4096, 4)[0] == ERR_ARG and c_layout(25, 3, 0, 0, 0, 0, 1 | 4096, 4)[0] == ERR_ARG      # no reward: unknown
    assert c_layout(25, 3, 0, 0, 0, 2, 1, 4)[0] == ERR_ARG and c_layout(25, 3, 0, 0, 0, 1, 8192, 4)[0] == ERR_ARG and c_layout(25, 3, 0, 0, 0, 1, 4096, 0)[0] == ERR_ARG
    assert c_layout(25, 3, 0, 0, 0, 1, 4096 | 1024, 4)[0] == ERR_ARG      # a reward brings no policy channel
    assert lib.irlosc_log_layout(25, 3, 4096, 4, _lib.ptr(off), C.addressof(words)) == ERR_ARG
    assert lib.irlosc_log_layout_objects(25, 3, 2, 4096, 4, _lib.ptr(off), C.addressof(words)) == ERR_ARG
    assert lib.irlosc_log_layout_policy(25, 3, 2, 7, 1, 4096, 4, _lib.ptr(off), C.addressof(words)) == ERR_ARG
    assert lib.irlosc_log_layout_reward(25, 3, 0, 0, 0, 1, 4096, 4, None, C.addressof(words)) == ERR_ARG
    assert lib.irlosc_log_layout_reward(25, 3, 0, 0, 0, 1, 4096, 4, _lib.ptr(off), None) == ERR_ARG
    for args in ((25, 3, 4096, 4), (25, 3, 4096, 4, 2), (25, 3, 4096, 4, 2, 7, True), (25, 3, 8192, 4, 0, 0, False, True)):
        with pytest.raises(ValueError):
            rollout_log.layout(*args)


def test_split_returns_the_reward_channel():
    n, ndev, R, S = 25, 3, 5, 3
    rng = np.random.default_rng(8)
    off, words = rollout_log.layout(n, ndev, ("u", "reward"), R, rewarded=True)
    want = dict(u=rng.normal(size=(S, R, n)), reward=rng.normal(size=(S, R, 4)))
    buf = np.full((S, words), np.nan)
    for i, name in ((5, "u"), (12, "reward")):
        buf[:, off[i]:off[i] + want[name][0].size] = want[name].reshape(S, -1)
    got = rollout_log.split(buf, n, ndev, ("u", "reward"), R, rewarded=True)
    assert list(got) == ["u", "reward"] and all(np.array_equal(got[k], want[k]) for k in want)


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------------
def test_the_mirror_on_a_three_term_example_computed_by_hand():
    """EE 0 at (1, 2, 2) then (0, 3, 4) from the origin: distances 3 and 5; u = (1, 2): U_SQ = 5; weights -0.5, 0.25, 2; gamma 0.5."""
    desc = rw.Reward([rw.dist(rw.ee(0), rw.fixed(0), -0.5), rw.u_sq(0.25), rw.one(2.0)], gamma=0.5, points=np.zeros((1, 3)), goal_term=0, goal_value=4.0, goal_hold=1)
    ee = np.zeros((1, 1, 7))
    ee[0, 0, :3] = (1, 2, 2)
    st = rw.reward_tick(desc, rw.reward_state(1), ee_pose=ee, u=np.array([[1.0, 2.0]], dtype=np.float32))
    assert (st["v"][:, 0] == (3, 5, 1)).all() and st["r"][0] == 1.75 and st["ret"][0] == 1.75 and st["gret"][0] == 1.75 and st["disc"][0] == 0.5
    assert (st["steps"][0], st["hold"][0], st["goal_step"][0]) == (1, 1, 1)
    ee[0, 0, :3] = (0, 3, 4)
    st = rw.reward_tick(desc, st, ee_pose=ee, u=np.array([[1.0, 2.0]], dtype=np.float32))
    assert st["r"][0] == 0.75 and st["ret"][0] == 2.5 and st["gret"][0] == 2.125 and st["disc"][0] == 0.25
    assert (st["steps"][0], st["hold"][0], st["goal_step"][0]) == (2, 0, 1)      # the comparison fails, goal_step stays
    # hold = 2 is never reached by one tick inside; >= with a NaN is false; ORI of a quaternion with itself is 0, with its negative too
    desc2 = rw.Reward(desc.terms, gamma=0.5, points=np.zeros((1, 3)), goal_term=0, goal_value=4.0, goal_hold=2)
    assert rw.reward_tick(desc2, rw.reward_state(1), ee_pose=np.zeros((1, 1, 7)), u=np.zeros((1, 2)))["goal_step"][0] == -1
    nan = np.full((1, 1, 7), np.nan)
    st = rw.reward_tick(rw.Reward(desc.terms, goal_term=0, goal_cmp=">=", goal_value=-1.0, points=np.zeros((1, 3))), rw.reward_state(1), ee_pose=nan, u=np.zeros((1, 2)))
    assert np.isnan(st["r"][0]) and np.isnan(st["ret"][0]) and st["hold"][0] == 0 and st["goal_step"][0] == -1
    q = np.zeros((2, 1, 7))
    q[:, 0, 3:] = (0.5, 0.5, -0.5, 0.5)
    v = rw.term_values(rw.Reward([rw.ori(rw.ee(0), rw.target(0), 1.0)]), ee_pose=q, targets=np.array([1, -1])[:, None, None] * q)
    assert (v == 0).all()
    fresh = rw.reward_state(3)
    assert (fresh["disc"] == 1).all() and (fresh["goal_step"] == -1).all() and not fresh["ret"].any() and fresh["steps"].dtype == np.int32


def test_the_mirrors_sums_against_exact_arithmetic_within_their_rounding_bounds():
    B, N, ndev, n, n_out = 16, 200, 3, 25, 7
    rng = np.random.default_rng(12)
    gamma = 0.97
    terms = [rw.dist(rw.ee(0), rw.fixed(0), -1.25), rw.dist_sq(rw.target(1), rw.obj(0), 0.375), rw.ori(rw.ee(2), rw.target(2), -0.7), rw.act_sq(-0.01),
             rw.u_sq(1e-4), rw.force(0, -0.3), rw.mated(0, 2.5), rw.one(-0.05)]
    desc = rw.Reward(terms, gamma=gamma, points=rng.normal(size=(B, 2, 3)))
    st = rw.reward_state(B)
    rs, worst = [], dict(r=0.0, ret=0.0, gret=0.0)
    for t in range(N):
        st = rw.reward_tick(desc, st, ee_pose=rng.normal(size=(B, ndev, 7)), targets=rng.normal(size=(B, ndev, 7)), u=rng.normal(size=(B, n)) * 30,
                            wrench=rng.normal(size=(B, ndev, 6)), object_pose=rng.normal(size=(B, 1, 8)), act=rng.normal(size=(B, n_out)).astype(np.float32),
                            mated_tick=rng.integers(-1, 2, size=(B, 1)))
        for b in range(B):
            parts = [Fraction(w) * Fraction(float(st["v"][i, b])) for i, (_, _, _, w) in enumerate(terms)]
            err, bound = abs(Fraction(float(st["r"][b])) - sum(parts)), 1.01 * (len(terms) + 1) * U * float(sum(abs(p) for p in parts))
            assert err <= bound, (t, b, float(err), bound)
            worst["r"] = max(worst["r"], float(err) / bound)
        rs.append(st["r"].copy())
    rs = np.array(rs)
    assert (st["steps"] == N).all()
    for b in range(B):
        exact = [Fraction(float(x)) for x in rs[:, b]]
        disc = [Fraction(gamma) ** t * x for t, x in enumerate(exact)]
        for key, ref, bound in (("ret", sum(exact), (N - 1) * U * float(sum(abs(x) for x in exact))), ("gret", sum(disc), 2 * N * U * float(sum(abs(x) for x in disc)))):
            err = abs(Fraction(float(st[key][b])) - ref)
            assert err <= 1.01 * bound, (key, b, float(err), bound)
            worst[key] = max(worst[key], float(err) / (1.01 * bound))
        assert abs(Fraction(float(st["disc"][b])) - Fraction(gamma) ** N) <= 1.01 * N * U * float(Fraction(gamma) ** N)
    print("worst error / bound:", worst)


def test_lengths_from_goal():
    L, O = ep.lengths_from_goal(np.array([-1, 1, 3, 5, 6]), 5)
    assert list(L) == [5, 1, 3, 5, 5] and list(O) == [ep.TIMEOUT, ep.FINISHED | ep.GOAL, ep.FINISHED | ep.GOAL, ep.FINISHED | ep.GOAL, ep.TIMEOUT]
    L, O = ep.lengths_from_goal(np.array([-1, 2, 9]), 5, end_on_finish=False)
    assert list(L) == [5, 5, 5] and list(O) == [ep.TIMEOUT, ep.TIMEOUT | ep.GOAL, ep.TIMEOUT]
