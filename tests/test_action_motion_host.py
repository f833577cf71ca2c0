"""The motion of an action list -- INTERP moves and seeded target noise -- the part that needs no GPU: the exports and the struct of
include/irlosc.h against the binding; Philox4x32-10 against the published known answers; the log, sine and cosine written out for the
device (irl_control_amd/action_motion.py: ln_rn, sincos_turn_rn) against NumPy's; the normals' moments and distribution; the NumPy
mirror of the kernel's MOTION form (action_motion_tick) on a scripted EE stream; and the two compilers on the reference's iros2022 file
(tests/golden/iros2022_task.yaml)."""
import ctypes as C
import os
import re

import numpy as np
import yaml

from conftest import ROOT
from irl_control_amd import _lib
from irl_control_amd import action_motion as am
from irl_control_amd import action_sequence as aseq

NEW = ("irlosc_set_action_motion", "irlosc_download_action_motion_state")
CTYPES = {"int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64}
WP, GRIP = _lib.ACTION_WP, _lib.ACTION_GRIP


def _header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_exports_and_the_binding_lists_them():
    h = _header()
    for name in NEW:
        assert re.search(r"IRLOSC_API\s+int\s+" + name + r"\s*\(", h), name
        assert name in _lib.EXPORTS
    assert re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", h) and _lib.ABI_VERSION == 3      # additive exports: the version stays


def test_action_motion_struct_matches_header_layout():
    m = re.search(r"typedef struct irlosc_action_motion \{(.*?)\} irlosc_action_motion;", _header(), flags=re.S)
    assert m, "struct irlosc_action_motion"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t|double|uint64_t)\s+(\w+)(?:\[(\w+)\])?;", body)
    assert fields == [("int32_t", "steps", "IRLOSC_MAX_ACTIONS"), ("double", "noise_mean", "IRLOSC_MAX_ACTIONS"),
                      ("double", "noise_std", "IRLOSC_MAX_ACTIONS"), ("uint64_t", "seed", "")]
    mirror = type("Mirror", (C.Structure,), {"_fields_": [(n, CTYPES[t] * _lib.MAX_ACTIONS if dim else CTYPES[t]) for t, n, dim in fields]})
    assert [f[0] for f in _lib.ActionMotion._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.ActionMotion) == C.sizeof(mirror) == 128 + 256 + 256 + 8
    for name, _ in mirror._fields_:
        assert getattr(_lib.ActionMotion, name).offset == getattr(mirror, name).offset, name


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The known-answer vectors of Random123's kat_vectors for philox4x32 with 10 rounds: counter, key -> output."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = am.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want, (ctr, key)
    # vectorised: the three at once
    got = am.philox4x32_10(np.array([k[0] for k in kat], dtype=np.uint32), np.array([k[1] for k in kat], dtype=np.uint32))
    assert np.array_equal(got, np.array([k[2] for k in kat], dtype=np.uint32))


def _words(rng, n):
    """uint32 words over the whole range: the ends, the neighbours of every power of two, and n uniform ones."""
    edge = [0, 1, 2, 3, 0xFFFFFFFF, 0xFFFFFFFE]
    for k in range(1, 32):
        edge += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    for k in (29, 30):                                    # ... and of every multiple of an octant
        for m in range(1, 1 << (32 - k)):
            edge += [(m << k) - 1, m << k, (m << k) + 1]
    return np.concatenate([np.array(edge, dtype=np.int64) & 0xFFFFFFFF, rng.integers(0, 1 << 32, n)]).astype(np.uint32)


def test_the_log_written_out_equals_numpys_to_1e_14():
    """ln_rn over its whole input range -- u = (2 w + 1) / 2^33 for every kind of word w, from 2^-33 to 1 - 2^-33 -- against np.log:
    relative error <= 1e-14 (the rounding of a few dozen operations plus a truncation below 1e-17: a sanity bound, not a tuned one)."""
    w = _words(np.random.default_rng(0), 1_000_000).astype(np.float64)
    u = (2.0 * w + 1.0) / 8589934592.0
    assert u.min() == 2.0 ** -33 and u.max() == 1.0 - 2.0 ** -33
    got, want = am.ln_rn(u), np.log(u)
    rel = np.abs(got - want) / np.abs(want)
    print(f"\n[ln_rn] max relative error {rel.max():.3g} over {len(u)} arguments")
    assert np.all(want < 0) and rel.max() <= 1e-14
    # and on arguments other than the generator's: every binade, both sides of sqrt(2)'s split of the mantissa
    x = np.concatenate([np.ldexp(m, e) for e in (-40, -1, 0, 1, 40) for m in (np.linspace(1.0, 2.0, 20001)[:-1],)])
    x = x[x != 1.0]
    assert (np.abs(am.ln_rn(x) - np.log(x)) / np.abs(np.log(x))).max() <= 1e-14
    assert am.ln_rn(np.array([1.0]))[0] == 0.0


def test_the_sine_and_cosine_written_out_equal_numpys_to_1e_14():
    """sincos_turn_rn of 2 pi w / 2^32 over every kind of word w against np.sin / np.cos, relative error <= 1e-14 -- against NumPy's
    functions of the SAME angle in two forms: (a) on the float angle 2 pi w / 2^32 wherever the function is at least 0.1 in size (the
    rounded angle is off by up to 7e-16 rad, which is no relative bound near a zero of the function); (b) everywhere, zeros' neighbours
    included, on the angle reduced to the first octant in exact integer arithmetic, where NumPy's argument carries one rounding.  At
    the multiples of a quarter turn the values are exactly 0 and +-1."""
    w = _words(np.random.default_rng(1), 1_000_000)
    s, c = am.sincos_turn_rn(w)
    theta = w.astype(np.float64) * (2.0 * np.pi / 4294967296.0)
    for got, want in ((s, np.sin(theta)), (c, np.cos(theta))):
        big = np.abs(want) >= 0.1
        assert (np.abs(got - want)[big] / np.abs(want)[big]).max() <= 1e-14
        assert np.abs(got - want).max() <= 1e-14
    wi = w.astype(np.int64)
    octant, r = wi >> 29, wi & ((1 << 29) - 1)
    odd = (octant & 1) == 1
    a = np.where(odd, (1 << 29) - r, r).astype(np.float64) * (2.0 * np.pi / 4294967296.0)      # [0, pi/4]
    sa, ca = np.sin(a), np.cos(a)
    s1, c1 = np.where(odd, ca, sa), np.where(odd, sa, ca)                                       # of the angle inside its quadrant
    quad = octant >> 1
    want_s = np.choose(quad, [s1, c1, -s1, -c1])
    want_c = np.choose(quad, [c1, -s1, -c1, s1])
    for name, got, want in (("sin", s, want_s), ("cos", c, want_c)):
        zero = want == 0.0
        assert np.array_equal(got[zero], want[zero]), name
        rel = np.abs(got - want)[~zero] / np.abs(want)[~zero]
        print(f"\n[sincos_turn_rn] {name}: max relative error {rel.max():.3g} over {len(w)} arguments")
        assert rel.max() <= 1e-14, name
    s4, c4 = am.sincos_turn_rn(np.array([0, 1 << 30, 1 << 31, 3 << 30], dtype=np.uint32))
    assert np.array_equal(s4, [0.0, 1.0, 0.0, -1.0]) and np.array_equal(c4, [1.0, 0.0, -1.0, 0.0])


def test_normal3_is_standard_normal_and_its_draws_are_all_different():
    """1e5 draws (robots 0 .. 99999 of draw 0, action 0) from seed 2022, each of the three components: |mean| < 4 / sqrt(N),
    |var - 1| < 4 sqrt(2 / N), Kolmogorov-Smirnov statistic against scipy.stats.norm < 1.63 / sqrt(N); the components are
    uncorrelated to the same 4 / sqrt(N); draws of different robots, draw indices, actions and seeds are pairwise different; the draw
    is a pure function of its four names."""
    from scipy import stats
    N = 100_000
    z = am.normal3(2022, np.arange(N), 0, 0)
    assert z.shape == (N, 3) and np.all(np.isfinite(z)) and np.abs(z).max() <= np.sqrt(66 * np.log(2.0))
    for c in range(3):
        ks = stats.kstest(z[:, c], stats.norm.cdf).statistic
        print(f"\n[normal3] component {c}: mean {z[:, c].mean():+.4f}, var {z[:, c].var():.4f}, KS {ks:.5f} (bound {1.63 / np.sqrt(N):.5f})")
        assert abs(z[:, c].mean()) < 4 / np.sqrt(N)
        assert abs(z[:, c].var() - 1.0) < 4 * np.sqrt(2.0 / N)
        assert ks < 1.63 / np.sqrt(N)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert abs(np.mean(z[:, i] * z[:, j])) < 4 / np.sqrt(N)
    R = np.arange(50)
    sets = [am.normal3(2022, R[:, None, None], R[None, :20, None], np.arange(8)[None, None, :]).reshape(-1, 3),      # robots x draws x actions
            am.normal3(2023, R, 0, 0)]
    allz = np.concatenate(sets)
    assert len(np.unique(allz.round(15), axis=0)) == len(allz) and len(np.unique(allz[:, 0])) == len(allz)
    assert np.array_equal(am.normal3(2022, 7, 3, 5), am.normal3(2022, R[:, None, None], R[None, :20, None], np.arange(8)[None, None, :])[7, 3, 5])
    assert np.array_equal(am.normal3((1 << 64) + 5, R, 1, 2), am.normal3(5, R, 1, 2))           # the seed is 64 bits
    assert not np.array_equal(am.normal3(1 << 32, R, 1, 2), am.normal3(0, R, 1, 2))             # ... and its high word counts


# ---- the mirror on a scripted EE stream -----------------------------------------------------------------------------------------------
B0, NDEV, IA, IO = 5, 2, 0, 1


def unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def make_desc(kinds, rng, max_error=0.02, flip=()):
    """A list of the given kinds with per-robot poses; `flip`: actions whose goal quaternion gets the sign that makes its dot with the
    start orientation negative."""
    A = len(kinds)
    pose = np.zeros((B0, A, 7))
    pose[:, :, :3] = rng.uniform(-0.3, 0.3, (B0, A, 3))
    pose[:, :, 3:] = unit(np.array([1.0, 0, 0, 0]) + rng.uniform(-0.4, 0.4, (B0, A, 4)))
    for a in flip:
        pose[:, a, 3:] *= -1.0
    return dict(n_actions=A, active_dev=IA, passive_dev=IO, passive_hold_orientation=1, passive_quat=np.array(aseq.DEFAULT_EE_QUAT), pose=pose,
                kind=np.array(kinds, np.int32), xyz_from_start=np.zeros(A, np.int32), grip_ticks=np.full(A, 3, np.int32), kp=np.full(A, 6.0),
                max_error=np.full(A, max_error), min_speed=np.full(A, 0.1), max_speed=np.full(A, 3.0), gripper_force=np.linspace(0.0, 0.3, A))


def drive(desc, T, motion=None, gain=0.5, dtype=np.float64):
    """T ticks of the mirror (action_motion_tick with a motion, else action_list_tick) on an arm whose EE covers `gain` of the way to
    its target per tick -> (targets per tick [T, B, ndev, 7], motion state copies per tick, list state, EE poses per tick)."""
    ee = np.zeros((B0, NDEV, 7))
    ee[:, :, 3] = 1.0
    ee[:, IO, :3] = [0.1, 0.2, 0.3]
    tgt = ee.astype(dtype)
    st = aseq.action_list_state(B0)
    tgts, mss, ees = [], [], []
    for t in range(T):
        ees.append(ee.copy())
        if motion is None:
            aseq.action_list_tick(st, ee, tgt, None, desc, t)
        else:
            am.action_motion_tick(st, ee, tgt, None, desc, t, motion)
            mss.append({k: v.copy() for k, v in motion["state"].items()})
        tgts.append(tgt.copy())
        g = tgt[:, IA].astype(np.float64)
        ee[:, IA, :3] += gain * (g[:, :3] - ee[:, IA, :3])
        sign = np.where(np.sum(ee[:, IA, 3:] * g[:, 3:], axis=1, keepdims=True) < 0, -1.0, 1.0)
        ee[:, IA, 3:] = unit(ee[:, IA, 3:] + gain * (sign * unit(g[:, 3:]) - ee[:, IA, 3:]))
    return np.array(tgts), mss, st, np.array(ees)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_steps_1_without_noise_is_action_list_tick_bit_for_bit():
    kinds = (WP, GRIP, WP, WP)
    for dtype in (np.float64, np.float32):
        desc = make_desc(kinds, np.random.default_rng(3))
        plain, _, st0, _ = drive(desc, 80, dtype=dtype)
        for steps in ([1, 0, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1]):
            moved, _, st1, _ = drive(desc, 80, motion=am.make_motion(4, steps=steps, seed=9), dtype=dtype)
            assert same_bits(plain, moved), steps
            for k in st0:
                assert same_bits(st0[k], st1[k]), (steps, k)
        assert np.all(st0["action"] == 4) and len(set(st0["finished_tick"])) >= 1


def test_an_interp_arrives_on_the_goal_exactly_and_only_then_advances():
    desc = make_desc((WP, WP, GRIP), np.random.default_rng(4), max_error=10.0)      # (so wide that only `step == N` holds an INTERP)
    N = 7
    motion = am.make_motion(3, steps=[N, 0, 0], noise_std=[0.01, 0, 0], seed=1)
    tgts, mss, st, _ = drive(desc, 20, motion=motion)
    for t in range(N):
        assert np.all(mss[t]["step"] == t + 1)
        assert (t == N - 1) == same_bits(tgts[t][:, IA], mss[t]["goal"]), t
    goal = mss[0]["goal"]
    assert not np.array_equal(goal[:, :3], desc["pose"][:, 0, :3]) and same_bits(goal[:, 3:], desc["pose"][:, 0, 3:])      # the noise is on xyz alone
    # the entry tick holds step 1 of N: a seventh of the way from the origin (the EE pose of tick 0)
    assert np.allclose(tgts[0][:, IA, :3], mss[0]["origin"][:, :3] + (goal[:, :3] - mss[0]["origin"][:, :3]) / N, rtol=0, atol=1e-15)
    # judged on tick N (step == N, err <= 10): action 1 is entered there, not before
    assert same_bits(tgts[N - 1][:, IA], goal) and same_bits(tgts[N][:, IA], desc["pose"][:, 1])
    assert np.all(st["action"] == 3)


def test_a_goal_with_a_negative_dot_travels_the_short_arc():
    """Every intermediate quaternion has norm 1 to rounding, the angle to the goal's rotation falls monotonically, and the path stays
    within the angle between the ends (the long way round would pass 180 degrees away from them)."""
    rng = np.random.default_rng(5)
    N = 40
    for _ in range(20):
        qo = unit(rng.normal(size=4))
        axis = unit(rng.normal(size=3))
        ang = rng.uniform(0.2, 2.5)
        dq = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])
        w1, x1, y1, z1 = qo
        w2, x2, y2, z2 = dq
        qg = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                       w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
        qg = -qg if np.dot(qo, qg) > 0 else qg                      # the same rotation, on the far hemisphere
        assert np.dot(qo, qg) < 0
        o, g = np.concatenate([[0, 0, 0], 3.0 * qo]), np.concatenate([[1, 2, 3], 0.5 * qg])      # (ends of any length: both are normalised)
        path = np.array([am.interp_pose(o, g, s, N) for s in range(1, N)])
        assert np.abs(np.linalg.norm(path[:, 3:], axis=1) - 1.0).max() <= 4e-16
        to_goal = 2 * np.arccos(np.clip(np.abs(path[:, 3:] @ unit(qg)), 0, 1))
        from_start = 2 * np.arccos(np.clip(np.abs(path[:, 3:] @ qo), 0, 1))
        assert np.all(np.diff(to_goal) < 0) and np.all(np.diff(from_start) > 0)
        assert to_goal.max() < ang and from_start.max() < ang
        assert np.allclose(path[:, :3], np.outer(np.arange(1, N) / N, [1, 2, 3]), rtol=0, atol=1e-15)


def test_the_tick_travels_the_short_arc_too():
    desc = make_desc((WP, WP), np.random.default_rng(6), max_error=0.05, flip=(0,))
    N = 12
    tgts, mss, st, ees = drive(desc, 60, motion=am.make_motion(2, steps=[N, 2]), gain=0.7)
    assert np.all(np.sum(ees[0][:, IA, 3:] * desc["pose"][:, 0, 3:], axis=1) < 0)
    for t in range(N - 1):
        q = tgts[t][:, IA, 3:]
        assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 4e-16
        assert np.all(np.sum(q * ees[0][:, IA, 3:], axis=1) > 0)       # on the origin's hemisphere all the way
    assert same_bits(tgts[N - 1][:, IA], desc["pose"][:, 0])           # arrives on the goal as given: its sign is not flipped
    assert np.all(st["action"] == 2)


def test_draws_count_noisy_entries_only_and_name_the_noise():
    kinds = (WP, WP, GRIP, WP, WP)
    desc = make_desc(kinds, np.random.default_rng(7))
    mean, std = [0.0, 0.0, 0.0, 0.01, 0.002], [0.003, 0.0, 0.0, 0.0, 0.004]       # actions 0, 3 (a mean alone), 4 are noisy
    motion = am.make_motion(5, steps=[0, 0, 0, 3, 0], noise_mean=mean, noise_std=std, seed=77)
    motion["state"] = am.action_motion_state(B0, draw0=np.arange(B0) * 10)
    tgts, mss, st, _ = drive(desc, 120, motion=motion)
    assert np.all(st["action"] == 5)
    assert np.array_equal(mss[-1]["draws"], np.arange(B0) * 10 + 3) and mss[-1]["draws"].dtype == np.uint32
    assert np.array_equal(mss[0]["draws"], np.arange(B0) * 10 + 1)
    # action 0's goal on tick 0: the table + std z of (seed, robot, draw0, action 0)
    z = am.normal3(77, np.arange(B0), np.arange(B0) * 10, 0)
    assert same_bits(mss[0]["goal"][:, :3], desc["pose"][:, 0, :3] + (0.0 + 0.003 * z))
    assert same_bits(tgts[0][:, IA, :3], mss[0]["goal"][:, :3])
    # another seed: other targets; the same seed: the same
    again, _, _, _ = drive(desc, 120, motion=dict(am.make_motion(5, steps=[0, 0, 0, 3, 0], noise_mean=mean, noise_std=std, seed=77),
                                                  state=am.action_motion_state(B0, draw0=np.arange(B0) * 10)))
    other, _, _, _ = drive(desc, 120, motion=dict(am.make_motion(5, steps=[0, 0, 0, 3, 0], noise_mean=mean, noise_std=std, seed=78),
                                                  state=am.action_motion_state(B0, draw0=np.arange(B0) * 10)))
    assert same_bits(tgts, again) and np.all(other[0][:, IA, :3] != tgts[0][:, IA, :3])


# ---- the compilers on the reference's file --------------------------------------------------------------------------------------------
SEQS = ("iros2022_pickup_sequence", "iros2022_demo_sequence", "iros2022_release_sequence")


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "iros2022_task.yaml")) as f:
        return yaml.safe_load(f)


def test_the_iros2022_file_compiles_to_a_list_and_a_motion():
    cfg = _fixture()
    right = am.compile_iros2022(cfg, SEQS, "right")
    left = am.compile_iros2022(cfg, SEQS, "left")
    assert len(right) == len(left) == 12
    assert [e["action"] for e in right] == ["WP", "GRIP", "WP", "WP", "GRIP", "GRIP", "WP", "INTERP", "WP", "INTERP", "GRIP", "WP"]
    # the active arm's column: devices are [base, ur5left, ur5right]
    assert right[0]["target_xyz"] == [0.625, -0.3, 0.35] and left[0]["target_xyz"] == [0.375, 0.3, 0.35]
    assert right[2]["target_xyz"] == [0.59, -0.16, 0.3] and left[2]["target_xyz"] == [0.33, 0.26, 0.3]          # male_object.hover_offset
    assert right[3]["target_xyz"] == [0.59, -0.16, 0.19] and left[3]["target_xyz"] == [0.33, 0.26, 0.19]        # male_object.grip_offset
    assert right[9]["target_xyz"] == [0.275, 0.59, 0.23] and left[9]["target_xyz"] == [-0.225, 0.61, 0.23]
    assert right[0]["target_quat"] == [0.707, 0.2, -0.707, 0.2] and right[7]["target_quat"] == [0.707, 0.707, -0.707, 0.707]
    assert sum(r.get("target_xyz") != l.get("target_xyz") for r, l in zip(right, left)) == 8                   # every WP / INTERP differs
    seq, motion = am.compile_action_motion(right)
    assert [e["action"] for e in seq] == ["WP", "GRIP", "WP", "WP", "GRIP", "GRIP", "WP", "WP", "WP", "WP", "GRIP", "WP"]
    assert all("steps" not in e and "noise" not in e for e in seq)
    assert motion["steps"].tolist() == [0, 0, 0, 0, 0, 0, 0, 100, 0, 20, 0, 0] and motion["steps"].dtype == np.int32
    assert motion["noise_mean"].tolist() == [0.0] * 12
    assert motion["noise_std"].tolist() == [0, 0, 0, 0, 0, 0, 0.005, 0.001, 0.001, 0.001, 0, 0]                 # (Pre-Grasp's is commented out)
    # ... and on through compile_action_list: the WP defaults apply to an INTERP, target_quat is taken as given
    d = aseq.compile_action_list(seq, [{}], active_dev=2, passive_dev=1)
    assert d["n_actions"] == 12 and d["kind"].tolist() == [0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0]
    assert d["kp"][7] == aseq.DEFAULT_PARAMS[aseq.Action.WP]["kp"] and d["max_error"][7] == 0.2 and d["max_error"][9] == 0.05
    assert d["min_speed"][9] == aseq.DEFAULT_PARAMS[aseq.Action.WP]["min_speed_xyz"]
    assert d["pose"][0, 7].tolist() == [0.275, 0.59, 0.3, 0.707, 0.707, -0.707, 0.707]
    assert d["grip_ticks"].tolist()[4] == 2000 and d["gripper_force"][4] == 0.05
    dl = aseq.compile_action_list(am.compile_action_motion(left)[0], [{}], active_dev=1, passive_dev=2)
    assert not np.array_equal(dl["pose"][:, :, :3], d["pose"][:, :, :3])


def test_the_compiler_refuses_what_the_kernel_cannot_run():
    import pytest
    with pytest.raises(ValueError):
        am.compile_action_motion([dict(action="INTERP", target_xyz=[0, 0, 0])])                    # no steps
    with pytest.raises(ValueError):
        am.compile_action_motion([dict(action="GRIP", noise=[0.0, 0.1])])
    with pytest.raises(ValueError):
        am.compile_action_motion([dict(action="WP", target_xyz=[0, 0, 0], steps=3)])
