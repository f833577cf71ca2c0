"""The resident lane route (irlosc_step / irlosc_step_resident on a slot's compact block, include/irlosc.h irlosc_slot_route) at its
edges: every layout a Dual-UR5 caller can reach, records whose dropped entries are not zero, singular task spaces, both forms of the eigen
pass on the same robots, and the other ways records reach a slot.  The reference is always oracle/osc_oracle.py in float64 on every
robot, with the reference's branch (PINV / TRUNCATED); lane route and row16 route (IRLOSC_RESIDENT_LANE=0) agree within 1e-7, flags
exactly.

Batch-mate contract of the eigen pass: a robot's result does not depend on its batch mates within one form of the pass, but which form
runs depends on how many robots of the step are flagged (>= IRLOSC_LANE_EIG_MIN: one lane per robot, else four robots per wave).
Within one form results are bit-exact; across the two forms they agree to rounding (flags identical)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import oracle_on_all
from irl_control_amd import BatchedOSC, _lib, synth
from oracle import osc_oracle
from test_gpu_parity import in_parity_domain, rel_err
from test_resident_lane import _physical, _rel, _train_equals_single_step, _upload

pytestmark = pytest.mark.gpu

TOL64 = 1e-5
LANE_MIN_B = 4096
EIG_MIN = int(os.environ.get("IRLOSC_LANE_EIG_MIN", "3000"))      # the library's default, or what this process runs with

# The eligibility rule of the resident lane route, stated independently of the library: rows per end-effector body (stand, right arm,
# left arm) fit an instantiation of the lane step, one device per body (the compact block holds one set of entries per body), and no
# target velocities (they keep the row16 kernel, as on the fused path).  Float64 records in an AUTO context, B >= 4096.
BODY = {"base": 0, "ur5right": 1, "ur5left": 2}
LANE_TIERS = ((1, 6, 6), (1, 3, 3))


def lane_tier(cfg):
    names, dof, _, _, _ = synth.LAYOUTS[cfg]
    rows = [0, 0, 0]
    for nm, m in zip(names, dof):
        rows[BODY[nm]] += int(sum(m))
    fits = [t for t, tr in enumerate(LANE_TIERS) if all(r <= c for r, c in zip(rows, tr))]
    return max(fits) if fits else None          # (the smallest tier that holds the layout)


def expected_route(cfg):
    names, _, _, _, fl = synth.LAYOUTS[cfg]
    if fl.get("branch_b") or len(set(names)) != len(names) or lane_tier(cfg) is None:
        return "row16_tree"
    return "lane"


def _tgt_vel(B, nd, rng):
    tv = rng.normal(0.0, 0.3, size=(B, nd, 6))
    tv[::3] = 0.0                                # every third robot stays on branch A
    return tv


def _check_oracle(lay, gains, rec, u, fl, tag):
    """u / flags against the oracle on every robot: <= 1e-5 on the parity domain, PINV / TRUNCATED = the reference's branch (robots
    whose det sits on the 1e-4 cut to 1e-6 relative excepted, as in test_gpu_layouts).  -> (max rel err, parity domain)"""
    ref, dom, pinv, trunc, det = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    assert dom.mean() > 0.5, (tag, dom.mean())
    err = rel_err(u, ref)
    assert err[dom].max() <= TOL64, (tag, float(err[dom].max()))
    assert not np.any(fl[dom] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD)), tag
    clear = dom & (np.abs(np.abs(det) / 1e-4 - 1.0) > 1e-6)
    assert np.array_equal((fl[clear] & _lib.FLAG_PINV_BRANCH) != 0, pinv[clear]), tag
    assert np.array_equal((fl[clear] & _lib.FLAG_TRUNCATED) != 0, trunc[clear]), tag
    return float(err[dom].max()), dom


def _eig_frac(fl):
    return float(np.mean((fl & _lib.FLAG_EIGEN_PATH) != 0))


def _n_flagged(fl):
    return int(np.count_nonzero(fl & _lib.FLAG_EIGEN_PATH))


# ---- 1. every layout: the lane route or the stated fallback ----------------------------------------------------------------------------

def test_the_rule_puts_enough_layouts_on_the_lane_route():
    """(Statement check: the sweep below runs at least eight layouts on the lane route, and every fallback of the rule is among them.)"""
    cfgs = synth.REACHABLE + ["k6", "k13_branch_b"]
    routes = {c: expected_route(c) for c in cfgs}
    assert sum(r == "lane" for r in routes.values()) >= 8, routes
    assert {c for c, r in routes.items() if r != "lane"} == {"rlbr10", "rlb11_branch_b", "brl14", "rlb16", "k13_branch_b"}
    assert lane_tier("k13") == 0 and lane_tier("k6") == 1 and lane_tier("b1") == 1 and lane_tier("rl8") == 0


@pytest.mark.parametrize("cfg", synth.REACHABLE + ["k6", "k13_branch_b"])
def test_every_layout_takes_the_lane_route_or_its_stated_fallback(cfg):
    """Physical states (random joint coordinates, every 10th robot with arm angles at multiples of pi / 2) at B = 4 096 + 37 through the
    front end: slot_route(0) is what the rule above says.  On the lane route: the oracle on every robot, and the row16 route on the same
    records (IRLOSC_RESIDENT_LANE=0) within 1e-7 with identical flags; admittance layouts with a random wrench in the records.  Off it:
    the route name and the oracle bound."""
    B = LANE_MIN_B + 37
    seed = 500 + (synth.REACHABLE + ["k6", "k13_branch_b"]).index(cfg)
    want = expected_route(cfg)
    lay, gains, _, osc, rec = _physical(cfg, B, seed=seed)
    if synth.LAYOUTS[cfg][4].get("branch_b"):
        rec["tgt_vel"] = _tgt_vel(B, lay.ndev, np.random.default_rng(seed))
        osc.set_targets(rec["tgt_pose"], rec["tgt_vel"])
    assert osc.slot_structure(0), cfg
    route = osc.slot_route(0)
    assert route == want, (cfg, route, want)
    u, fl = osc.step(return_flags=True)
    give = int(osc.giveup_counts()[0])
    osc.close()
    err, dom = _check_oracle(lay, gains, rec, u, fl, cfg)
    line = f"{cfg}: route {route}, max rel vs oracle {err:.2e}, eigen path {_eig_frac(fl):.3f}, give-ups {give}"
    if route == "lane":
        _, _, _, r16, rec2 = _physical(cfg, B, seed=seed, lane=False)
        assert np.array_equal(rec2["M"], rec["M"]) and np.array_equal(rec2["J"], rec["J"])
        assert r16.slot_route(0) == "row16_tree"
        u_r, fl_r = r16.step(return_flags=True)
        r16.close()
        d = _rel(u, u_r)
        line += f", lane vs row16 max rel {d[dom].max():.2e}"
        assert np.array_equal(fl, fl_r), cfg
        assert d[dom].max() <= 1e-7, (cfg, float(d[dom].max()))
    print(line)


# ---- 2. the pack's per-row check -------------------------------------------------------------------------------------------------------

def test_a_stray_entry_in_a_row_the_probe_accepts_keeps_the_slot_off_the_lane_route():
    """k13 records (rows: right arm 0-5, left arm 6-11, stand yaw 12).  The structure probe looks at J one column at a time, so a left-arm
    row with an entry at a right-arm joint column (or the stand's yaw row at an arm column) passes it; the pack drops per row every joint
    that cannot move THAT row's body, and its check must keep such records off the lane route.  One robot at a time: robot 0, a robot in
    the middle of a wave, robot B - 1 in the ragged last wave.  The step then equals the row16 route bit for bit and meets the oracle
    computed with the stray entry, which moves that robot's torques by far more than the bound (a dropped entry would be seen)."""
    B = 2 * LANE_MIN_B + 37
    lay, gains, _, osc, rec = _physical("k13", B, seed=41)
    _, _, _, r16, _ = _physical("k13", B, seed=41, lane=False)
    assert osc.slot_route(0) == "lane"
    u_fresh, fl_fresh = osc.step(return_flags=True)              # a fresh context's step on the clean records
    ref0, dom0, _, _, _ = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    J = rec["J"]
    # a column of each arm that moves that arm's end effector (non-zero in its rows): allowed by the column probe
    col_r = 1 + int(np.argmax(np.count_nonzero(J[:, 0:6, 1:13], axis=(0, 1))))
    col_l = 13 + int(np.argmax(np.count_nonzero(J[:, 6:12, 13:25], axis=(0, 1))))
    assert np.all(J[:, 6:12, col_r] == 0) and np.all(J[:, 12, col_l] == 0)
    lay_d = lay.as_oracle_dict()
    for row, col, what in ((8, col_r, "left-arm row, right-arm column"), (12, col_l, "stand yaw row, left-arm column")):
        for b in (0, 29 * 64 + 31, B - 1):
            Jp = J.copy()
            Jp[b, row, col] = 0.3
            r = dict(rec, J=Jp)
            _upload(osc, r)
            _upload(r16, r)
            assert osc.slot_structure(0), (what, b)
            assert osc.slot_route(0) == "row16_tree", (what, b, osc.slot_route(0))
            u, fl = osc.step(return_flags=True)
            u_r, fl_r = r16.step(return_flags=True)
            assert np.array_equal(u, u_r) and np.array_equal(fl, fl_r), (what, b)
            one = {k: v[b:b + 1] for k, v in r.items() if isinstance(v, np.ndarray)}
            ref_b = osc_oracle.generate_batch(lay_d, gains, one["M"], one["J"], one["dq"], one["bias"], one["ee_pose"], one["tgt_pose"])
            assert rel_err(ref_b, ref0[b:b + 1])[0] > 1e-3, (what, b)           # the stray entry matters
            dom_b = in_parity_domain(*osc_oracle.task_inertia(Jp[b], rec["M"][b])[2:])
            ref = ref0.copy()
            ref[b] = ref_b[0]
            dom = dom0.copy()
            dom[b] = dom_b
            err = rel_err(u, ref)
            assert err[dom].max() <= TOL64, (what, b, float(err[dom].max()))
            if dom_b:
                assert err[b] <= TOL64, (what, b, float(err[b]))
            print(f"{what}, robot {b}: route row16_tree, max rel vs oracle {err[dom].max():.2e}, "
                  f"oracle moved by {rel_err(ref_b, ref0[b:b + 1])[0]:.2e}")
    _upload(osc, rec)
    assert osc.slot_route(0) == "lane"
    u, fl = osc.step(return_flags=True)
    assert np.array_equal(u, u_fresh) and np.array_equal(fl, fl_fresh)
    osc.close()
    r16.close()


# ---- 3. singular task spaces on the lane route -----------------------------------------------------------------------------------------

# k13 rows: right arm 0-5, left arm 6-11, stand yaw 12.  "dup": rows of an arm copied into other rows of the same arm (the tree's zero
# pattern and the pack check hold); "zero": whole rows zeroed (the zero-row mask), the stand row first.
SINGULAR = {
    "dup": {1: [(1, 0)], 2: [(1, 0), (2, 0)], 3: [(1, 0), (2, 0), (3, 0)], 5: [(1, 0), (2, 0), (3, 0), (7, 6), (8, 6)]},
    "zero": {1: [12], 2: [12, 0], 3: [12, 0, 6], 5: [12, 0, 1, 6, 7]},
}


def _make_singular(J, bad, case, lost):
    J = J.copy()
    for op in SINGULAR[case][lost]:
        if case == "dup":
            J[bad, op[0]] = J[bad, op[1]]
        else:
            J[bad, op] = 0.0
    return J


@pytest.mark.parametrize("lost", [1, 2, 3, 5])
@pytest.mark.parametrize("case", ["dup", "zero"])
def test_singular_task_spaces_on_the_lane_route(case, lost, monkeypatch):
    """Every third robot of k13 physical records (B = 4 096 + 69) loses `lost` task directions.  The lane route keeps the slot, the
    branch flags are the reference's, the oracle bound holds on every robot, the row16 route agrees (<= 1e-7, flags identical).

    The affected robots are every third one, less those whose clean records already truncate a direction and those with arms at
    multiples of pi / 2 (they would lose more than `lost`: with 3 duplicated rows, 184 of 1 389 robots gave up).  Give-ups follow
    test_row16_rank_deficient_jacobians: more than three lost directions -> every affected robot goes to the generic kernel; up to three
    are deflated in the eigen pass and at most one eighth give up.  Zeroed rows are taken out of
    the factorisation exactly (zero-row mask), as in the padded row16 kernel: they are never deflated and nobody gives up, whatever
    their number.  So the row16 route they are held to is the padded one (IRLOSC_FORCE_PAD=1).  The exact k13 instantiation has no zero-row
    mask: it finds zero rows as null directions in its eigen stage (FLAG_EIGEN_PATH set where the lane step leaves it clear; measured
    1.4e-7 relative from the lane route, which is within 2e-10 of the oracle there), and is held to the same flags otherwise."""
    B = LANE_MIN_B + 69
    lay, gains, _, osc, rec = _physical("k13", B, seed=61)
    _, _, _, r16, _ = _physical("k13", B, seed=61, lane=False)
    if case == "zero":
        monkeypatch.setenv("IRLOSC_FORCE_PAD", "1")           # (read at irlosc_create)
        _, _, _, r16p, _ = _physical("k13", B, seed=61, lane=False)
        monkeypatch.delenv("IRLOSC_FORCE_PAD")
        assert "pad" in r16p.kernel_name
    # every third robot, less those whose clean records already truncate a direction and those with arms at multiples of pi / 2:
    # the affected robots lose exactly `lost` directions
    _, _, _, trunc0, _ = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    bad = np.setdiff1d(np.arange(0, B, 3), np.concatenate([np.flatnonzero(trunc0), np.arange(3, B, 10)]))
    r = dict(rec, J=_make_singular(rec["J"], bad, case, lost))
    _upload(osc, r)
    _upload(r16, r)
    assert osc.slot_route(0) == "lane", osc.slot_route(0)
    u, fl = osc.step(return_flags=True)
    give = int(osc.giveup_counts()[0])
    u_r, fl_r = r16.step(return_flags=True)
    r16.close()
    if case == "zero":
        _upload(r16p, r)
        assert r16p.slot_route(0) == "row16_tree"
        u_p, fl_p = r16p.step(return_flags=True)
        r16p.close()
    osc.close()
    err, dom = _check_oracle(lay, gains, r, u, fl, (case, lost))
    assert np.all(fl[bad] & _lib.FLAG_PINV_BRANCH) and np.all(fl[bad] & _lib.FLAG_TRUNCATED)
    if case == "dup":
        d = _rel(u, u_r)
        assert np.array_equal(fl, fl_r)
    else:
        d = _rel(u, u_p)
        assert np.array_equal(fl, fl_p)
        assert np.array_equal(fl | _lib.FLAG_EIGEN_PATH, fl_r | _lib.FLAG_EIGEN_PATH)
        assert np.array_equal(np.delete(fl, bad), np.delete(fl_r, bad))
        assert _check_oracle(lay, gains, r, u_r, fl_r, (case, lost, "exact row16"))[0] <= TOL64
    print(f"singular {case} lost {lost}: max rel vs oracle {err:.2e}, vs row16{' (padded)' if case == 'zero' else ''} "
          f"{d[dom].max():.2e}, eigen path {_eig_frac(fl):.3f}, give-ups {give} of {len(bad)}")
    assert d[dom].max() <= 1e-7, float(d[dom].max())
    if case == "dup" and lost > 3:
        assert give >= len(bad), give
    else:
        assert give <= len(bad) // 8, give


def test_singular_give_up_lists_inside_trains():
    """Two lane slots of singular records (five and three lost directions on every third robot): every split of a resident train leaves
    what a single step on its last slot leaves, bit for bit, and a train's give-up counts per step equal those of single steps."""
    B = LANE_MIN_B + 69
    _, _, _, osc, rec = _physical("k13", B, seed=62, n_slots=2)
    bad = np.arange(0, B, 3)
    _upload(osc, dict(rec, J=_make_singular(rec["J"], bad, "dup", 5)), slot=0)
    _upload(osc, dict(rec, J=_make_singular(rec["J"], bad, "dup", 3)), slot=1)
    assert [osc.slot_route(s) for s in range(2)] == ["lane", "lane"]
    single = []
    for s in range(2):
        osc.step(slot=s)
        single.append(int(osc.giveup_counts()[0]))
    assert single[0] >= len(bad)
    for first in (0, 1):
        _train_equals_single_step(osc, 2, 9, first, B)
        osc.step_resident(osc.steps_per_launch, first_slot=first)
        counts = osc.giveup_counts()
        assert [int(c) for c in counts[:osc.steps_per_launch]] == [single[(first + i) % 2] for i in range(osc.steps_per_launch)], counts
    osc.close()


# ---- 4. both forms of the eigen pass on the same robots --------------------------------------------------------------------------------

EIG_B = 2 * LANE_MIN_B + 37
EIG_SETTINGS = [("lane", {"IRLOSC_LANE_EIG_MIN": "0"}), ("four_per_wave", {"IRLOSC_LANE_EIG_MIN": "1000000000"}),
                ("lane_capped", {"IRLOSC_LANE_EIG_MIN": "0", "IRLOSC_LANE_EIG_BLOCKS": "64"})]


def _eig_records(cfg, seed):
    """The child's records: slot 0 holds physical records (front end) in which two thirds of the robots are singular (three duplicated
    arm rows; a zeroed row and a duplicated one), slot 1 front-end records of states with every third robot's arms at multiples of
    pi / 2."""
    B = EIG_B
    lay, gains, model, osc, rec = _physical(cfg, B, seed=seed, n_slots=2)
    b = np.arange(B)
    J = _make_singular(rec["J"], b % 3 == 1, "dup", 3)
    J[b % 3 == 2, 0] = 0.0                       # a zero row and a duplicated row (k13 and k12 alike): both on the eigen path
    J[b % 3 == 2, 8] = J[b % 3 == 2, 7]
    rec0 = dict(rec, J=J)
    _upload(osc, rec0, slot=0)
    rng = np.random.default_rng(seed + 1)
    qpos, qvel = model.random_state(rng, B)
    idx = np.arange(0, B, 3)
    qpos[idx, 1:7] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    qpos[idx, 13:19] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    osc.upload_q(qpos, qvel, slot=1)
    osc.frontend(slot=1)
    rec1 = osc.download_records(1)
    rec1["tgt_pose"] = synth.targets_near(rec1["ee_pose"], rng)
    if lay.admittance:
        rec1["wrench"] = np.zeros((B, lay.ndev, 6))     # no F/T reading in slot 1: the wrench term is zero on both of its paths
    osc.set_targets(rec1["tgt_pose"], slot=1)
    return lay, gains, osc, rec0, rec1


def _eig_child(cfg, seed, out, save_records):
    lay, gains, osc, rec0, rec1 = _eig_records(cfg, seed)
    assert osc.slot_route(0) == "lane" and osc.slot_route(1) == "lane", (osc.slot_route(0), osc.slot_route(1))
    res = {}
    res["u0"], res["f0"] = osc.step(slot=0, return_flags=True)
    res["u1"], res["f1"] = osc.step(slot=1, return_flags=True)
    res["uq"], res["fq"] = osc.step_q(slot=1, return_flags=True)      # the fused path runs the same eigen pair
    osc.close()
    if save_records:
        for tag, r in (("r0_", rec0), ("r1_", rec1)):
            res.update({tag + k: v for k, v in r.items() if k not in ("qpos", "qvel")})
    np.savez(out, **res)


@pytest.mark.parametrize("cfg", ["k13", "k12_admit"])
def test_both_eigen_pass_forms_give_the_same_robots_the_same_answer(cfg, tmp_path):
    """The eigen pass reads its environment once per process, so each setting runs in a fresh child process (one at a time, each under
    its own time limit, the test stops at the first that fails): always the lane form, always the four-per-wave form, the lane form
    with its grid capped at 64 blocks (more than 64 x 64 flagged robots: the grid-stride loop wraps).  Same records, on the resident
    lane route and on step_q: identical flags, torques within 1e-9, the capped grid changes no bit, every run meets the oracle."""
    seed = 71 if cfg == "k13" else 72
    runs = {}
    for i, (name, env_extra) in enumerate(EIG_SETTINGS):
        out = str(tmp_path / f"{name}.npz")
        env = dict(os.environ)
        for k in ("IRLOSC_LANE_EIG_MIN", "IRLOSC_LANE_EIG_BLOCKS"):
            env.pop(k, None)
        env.update(env_extra)
        args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
            [os.path.abspath(__file__), "--eig-child", cfg, str(seed), out, "1" if i == 0 else "0"]
        p = subprocess.run(args, env=env, cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        runs[name] = dict(np.load(out))
    base = runs["lane"]
    lay = synth.make_layout(cfg)
    _, gains, _ = synth.make_batch(cfg, 2, seed=1, dtype=np.float64)
    assert _n_flagged(base["f0"]) > 64 * 64, _n_flagged(base["f0"])
    for key in ("0", "1", "q"):
        for name in ("four_per_wave", "lane_capped"):
            assert np.array_equal(runs[name]["f" + key], base["f" + key]), (name, key)
        assert np.array_equal(runs["lane_capped"]["u" + key], base["u" + key]), key          # the block cap changes no bit
        d = _rel(runs["four_per_wave"]["u" + key], base["u" + key])
        print(f"{cfg} step {key}: flagged {_n_flagged(base['f' + key])} of {EIG_B}, lane vs four-per-wave form max rel {d.max():.2e} "
              f"(bit-equal robots {np.mean(np.all(runs['four_per_wave']['u' + key] == base['u' + key], axis=1)):.4f})")
        assert d.max() <= 1e-9, (key, float(d.max()))
    for key, tag in (("0", "r0_"), ("1", "r1_"), ("q", "r1_")):
        rec = {k[len(tag):]: v for k, v in base.items() if k.startswith(tag)}
        for name in runs:
            _check_oracle(lay, gains, rec, runs[name]["u" + key], runs[name]["f" + key], (cfg, name, key))


# ---- 5. other inputs to the route ------------------------------------------------------------------------------------------------------

def test_per_instance_gains_on_the_lane_route():
    """Per-robot gains (kp, kv, ko, k, d and null_kv per robot) on the lane route against the oracle on every robot."""
    B = LANE_MIN_B + 37
    lay, gains0, _, osc, rec = _physical("k13", B, seed=81)
    _, gains, _ = synth.make_batch("k13", B, seed=82, per_instance_gains=True)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    assert osc.slot_route(0) == "lane"
    u, fl = osc.step(return_flags=True)
    osc.close()
    _, dom, _, _, _ = oracle_on_all(lay.as_oracle_dict(), gains0, rec)     # (the domain does not depend on the gains)
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, rec["M"], rec["J"], rec["dq"], rec["bias"], rec["ee_pose"],
                                    rec["tgt_pose"])
    err = rel_err(u, ref)
    assert dom.mean() > 0.9 and err[dom].max() <= TOL64, float(err[dom].max())


def test_a_step_of_fewer_robots_than_the_slot_holds():
    """step_resident(1, B=5000) on a slot that holds 8 192: the first 5 000 robots of the full step -- bit for bit when both steps run
    the same form of the eigen pass, to rounding otherwise.  4 095 robots are below the route's threshold."""
    B = 2 * LANE_MIN_B
    _, _, _, osc, rec = _physical("k13", B, seed=83)
    u, fl = osc.step(return_flags=True)
    assert osc.slot_route(0, 5000) == "lane" and osc.slot_route(0, LANE_MIN_B - 1) == "row16_tree"
    osc.step_resident(1, B=5000)
    u5, fl5 = osc.download(5000)
    osc.close()
    assert np.array_equal(fl5, fl[:5000])
    if (_n_flagged(fl) >= EIG_MIN) == (_n_flagged(fl5) >= EIG_MIN):
        assert np.array_equal(u5, u[:5000])
    else:
        assert _rel(u5, u[:5000]).max() <= 1e-9


def _raw_from_k13_records(rec):
    nv, ns = 25, 18
    B = rec["M"].shape[0]
    d = _lib.RawDesc()
    d.nv, d.n_sensor = nv, ns
    for p_ in range(32):
        d.joint_ids[p_] = p_ if p_ < 25 else 0
        d.dq_src[p_] = p_ if p_ < 25 else -1
    for i in range(4):
        d.ft_force0[i], d.ft_torque0[i] = -1, -1
    jacp, jacr = np.zeros((B, 3, 3, nv)), np.zeros((B, 3, 3, nv))      # k13: ur5right, ur5left, base (yaw = third rotational row)
    jacp[:, 0], jacr[:, 0] = rec["J"][:, 0:3], rec["J"][:, 3:6]
    jacp[:, 1], jacr[:, 1] = rec["J"][:, 6:9], rec["J"][:, 9:12]
    jacr[:, 2, 2] = rec["J"][:, 12]
    arr = dict(qM=rec["M"], qvel=rec["dq"], qfrc_bias=rec["bias"], jacp=jacp, jacr=jacr,
               ee_xpos=np.ascontiguousarray(rec["ee_pose"][:, :, :3]), ee_xquat=np.ascontiguousarray(rec["ee_pose"][:, :, 3:]),
               site_xmat=np.tile(np.eye(3).reshape(9), (B, 3, 1)), sensordata=np.zeros((B, ns)))
    return d, arr


def test_raw_state_upload_takes_the_lane_route():
    """Raw simulator arrays of physical states through irlosc_upload_raw in an AUTO context: probed, packed with the check, on the
    lane route, and the step equals the one on the plainly uploaded records bit for bit."""
    B = LANE_MIN_B + 37
    _, _, _, osc, rec = _physical("k13", B, seed=84)
    u_rec, fl_rec = osc.step(return_flags=True)
    d, arr = _raw_from_k13_records(rec)
    osc.upload_raw(d, **arr)
    osc.set_targets(rec["tgt_pose"])
    assert osc.slot_structure(0) and osc.slot_route(0) == "lane", osc.slot_route(0)
    u, fl = osc.step(return_flags=True)
    osc.close()
    assert np.array_equal(u, u_rec) and np.array_equal(fl, fl_rec)


def test_set_model_on_a_packed_slot():
    """irlosc_set_model drops every compact block: the slot steps on row16_tree until new records arrive, and still meets the oracle."""
    B = LANE_MIN_B + 37
    lay, gains, model, osc, rec = _physical("k13", B, seed=85)
    assert osc.slot_route(0) == "lane"
    u_l = osc.step()
    osc.set_model(model)
    assert osc.slot_route(0) == "row16_tree"
    u, fl = osc.step(return_flags=True)
    _check_oracle(lay, gains, rec, u, fl, "after set_model")
    _upload(osc, rec)
    assert osc.slot_route(0) == "lane"
    assert np.array_equal(osc.step(), u_l)
    osc.close()


@pytest.mark.parametrize("kind", ["float32", "kernel_row16"])
def test_float32_records_and_an_explicit_row16_context_stay_off_the_lane_route(kind):
    """Float32 records (AUTO context) and an explicit KERNEL_ROW16 context never take the lane route at B >= 4 096, whether the
    records come from the front end or from an upload."""
    B = LANE_MIN_B + 5
    dtype, kernel = (np.float32, _lib.KERNEL_AUTO) if kind == "float32" else (np.float64, _lib.KERNEL_ROW16)
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 2, seed=1)
    from irl_control_amd.rigid_body import RigidBodyModel
    model = RigidBodyModel.load("dual_ur5")
    osc = BatchedOSC(lay, B, dtype=dtype, kernel=kernel)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    qpos, qvel = model.random_state(np.random.default_rng(86), B)
    osc.upload_q(qpos, qvel)
    osc.frontend()
    rec = osc.download_records(0)
    rec["tgt_pose"] = synth.targets_near(rec["ee_pose"].astype(np.float64), np.random.default_rng(87))
    osc.set_targets(rec["tgt_pose"])
    assert osc.slot_route(0) in ("row16_tree", "row16"), osc.slot_route(0)      # records of the front end
    _upload(osc, rec)                                                              # uploaded records
    assert osc.slot_route(0) in ("row16_tree", "row16"), osc.slot_route(0)
    u = osc.step()
    osc.close()
    assert np.all(np.isfinite(u))


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--eig-child":
        _eig_child(sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5] == "1")
    else:
        sys.exit("usage: test_resident_lane_edges.py --eig-child CFG SEED OUT.npz SAVE_RECORDS")
