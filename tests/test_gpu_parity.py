"""GPU parity tests proper (-m gpu): the HIP path, called through the C ABI, against
(a) the outputs of the reference itself (golden fixtures) and (b) the oracle on fresh seeded
batches.  Bar from BASELINE.json north_star: torques within 1e-5 relative in fp64.

Relative error per instance = max_j |u_j - ref_j| / max_j |ref_j|.

Parity domain: instances where the reference's own answer is well defined, i.e.
not (|det(Mx_inv)| >= 1e-4 while Mx_inv is numerically singular), and no singular value of Mx_inv
within 1 % of the 1e-5 pinv cut-off when the pinv branch is taken (there LAPACK's and any other
method's 1-ulp differences decide which side of the cut the value falls).
"""
import numpy as np
import pytest

from conftest import (HipBuffers, app_from_e2e, golden_expected_u, golden_gains, golden_names, load_e2e,
                      load_golden, oracle_on_all)
from irl_control_amd import BatchedOSC, OSCLayout, _lib
from oracle import osc_oracle
from irl_control_amd import synth

pytestmark = pytest.mark.gpu
TOL64 = 1e-5


def in_parity_domain(Mx_inv, det):
    s = np.linalg.svd(Mx_inv, compute_uv=False)
    if abs(det) >= 1e-4:
        return s[-1] > 1e-12 * s[0]
    r = s / s[0]
    return not np.any(np.abs(r / 1e-5 - 1.0) < 1e-2)


def run_gpu(lay, gains, g, dtype, kernel=_lib.KERNEL_AUTO):
    B = g["M"].shape[0]
    osc = BatchedOSC(lay, B, dtype=dtype, kernel=kernel)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"],
                  gains["null_kv"])
    u, fl = osc.generate_batched(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"],
                                 g.get("tgt_vel"), g.get("wrench"), return_flags=True)
    name = osc.kernel_name
    osc.close()
    return u.astype(np.float64), fl, name


def rel_err(u, ref):
    m = ~np.isnan(ref)
    d = np.where(m, np.abs(u - np.where(m, ref, 0.0)), 0.0)
    return d.max(axis=1) / np.nanmax(np.abs(ref), axis=1)


@pytest.mark.parametrize("kernel", [_lib.KERNEL_GENERIC, _lib.KERNEL_AUTO])
@pytest.mark.parametrize("name", golden_names())
def test_fp64_matches_reference_outputs(name, kernel):
    g = load_golden(name)
    lay = OSCLayout.from_dict(g["layout"])
    u, fl, kname = run_gpu(lay, golden_gains(g), g, np.float64, kernel)
    exp = golden_expected_u(g)
    dom = np.array([in_parity_domain(a, d) for a, d in zip(g["Mx_inv"], g["det"])])
    assert dom.sum() >= 0.7 * len(dom), "parity domain unexpectedly small"
    err = rel_err(u, exp)
    assert err[dom].max() <= TOL64, (kname, name, err[dom].max())
    assert not np.any(fl[dom] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    # the pinv-branch flag must agree with the reference's det test (osc.py:52)
    assert np.array_equal((fl[dom] & _lib.FLAG_PINV_BRANCH) != 0, np.abs(g["det"][dom]) < 1e-4)
    if name == "k13_branch_b":
        assert np.all(fl & _lib.FLAG_VEL_BRANCH_B)


def test_truncation_regime_is_exercised():
    g = load_golden("k13_pinv_regime")
    lay = OSCLayout.from_dict(g["layout"])
    u, fl, _ = run_gpu(lay, golden_gains(g), g, np.float64)
    s = np.array([np.linalg.svd(a, compute_uv=False) for a in g["Mx_inv"]])
    must_cut = (s[:, -1] < 0.9e-5 * s[:, 0]) & (np.abs(g["det"]) < 1e-4)
    assert must_cut.sum() >= 8
    assert np.all(fl[must_cut] & _lib.FLAG_TRUNCATED)
    no_cut = s[:, -1] > 1.1e-5 * s[:, 0]
    assert not np.any(fl[no_cut] & _lib.FLAG_TRUNCATED)


@pytest.mark.parametrize("cfg", ["k13", "k7", "k12_admit"])
def test_fp64_4096_instances_vs_oracle(cfg):
    """BASELINE config[1]: 4 096 Dual-UR5 instances, fp64, torque parity vs the CPU path."""
    B = 4096
    lay, gains, g = synth.make_batch(cfg, B, seed=1234)
    u, fl, kname = run_gpu(lay, gains, g, np.float64)
    idx = np.arange(0, B, 4)                       # oracle on every 4th instance (~1 ms each)
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, g["M"], g["J"], g["dq"], g["bias"],
                                    g["ee_pose"], g["tgt_pose"], g.get("wrench"), g.get("tgt_vel"), idx=idx)
    dom = []
    for b in idx:
        Mx, Minv, Mxi, det = osc_oracle.task_inertia(g["J"][b], g["M"][b])
        dom.append(in_parity_domain(Mxi, det))
    dom = np.array(dom)
    err = rel_err(u[idx], ref[idx])
    assert dom.mean() > 0.9
    assert err[dom].max() <= TOL64, (kname, err[dom].max())
    assert np.all(np.isfinite(u))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row16_cut_decision_when_power_iteration_is_slow(dtype):
    """Regression (found by running BASELINE config[1] through bench.py): instance 2149 of the 4 096-instance bench batch
    has an eigenvalue of J M^-1 J^T 3.1 % UNDER the pinv cut while lambda_2 / lambda_max = 0.85, so a 24-step power
    iteration is still 6 % short of lambda_max -- the eigenvalue must be cut all the same (osc.py:55).  The whole batch
    against the oracle, every instance, the row16 kernel on float64 and on float32 records."""
    B = 4096
    lay, gains, g = synth.make_batch("k13", B, seed=20241008 + 2000, dtype=dtype)
    g64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in g.items()}
    u, fl, kname = run_gpu(lay, gains, g, dtype, kernel=_lib.KERNEL_ROW16)
    assert "row16" in kname
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, g64["M"], g64["J"], g64["dq"], g64["bias"], g64["ee_pose"],
                                    g64["tgt_pose"])
    err = rel_err(u.astype(np.float64), ref)
    if dtype == np.float64:
        s = np.linalg.svd(osc_oracle.task_inertia(g64["J"][2149], g64["M"][2149])[2], compute_uv=False)
        assert 0.95 < s[-2] / s[0] / 1e-5 < 0.99                  # the case is what the docstring says it is
        assert fl[2149] & 0x8                                      # TRUNCATED
        assert err[2149] <= TOL64, err[2149]
    over = np.nonzero(err > TOL64)[0]
    for b in over:                                                 # anything else over the bar must sit on the cut itself
        Mx, Minv, Mxi, det = osc_oracle.task_inertia(g64["J"][b], g64["M"][b])
        assert not in_parity_domain(Mxi, det), (b, err[b])


@pytest.mark.parametrize("cfg", ["k13", "k7", "k12_admit"])
def test_row16_stress_eigenvalues_all_around_the_cut(cfg):
    """tools/parity_sweep.py --stress in small: 1-3 task rows of J per instance scaled by 10^U(-3.5, -1.5) (picked with
    repetition: down to 1e-10, i.e. singular to working precision), so that nearly every instance truncates and the
    eigenvalues of J M^-1 J^T sit anywhere around the cut.  The row16 kernel against the generic kernel (exact Jacobi
    spectrum) on all of them, disagreements over 1e-5 only where the oracle has a singular value within 1 % of the cut.
    This is what found: rounding-level positive pivots, eigenvectors settled to 1e-5 only, two lambda_max estimates."""
    B = 16384
    lay, gains, g = synth.make_batch(cfg, B, seed=777000 + 131 * 7)
    rng = np.random.default_rng(4242 + 7)
    k = g["J"].shape[1]
    nrows = rng.integers(1, 4, size=B)
    for j in range(3):
        rows = rng.integers(0, k, size=B)
        f = np.where(nrows > j, 10.0 ** rng.uniform(-3.5, -1.5, size=B), 1.0)
        g["J"][np.arange(B), rows, :] *= f[:, None]
    u, fl, kname = run_gpu(lay, gains, g, np.float64, kernel=_lib.KERNEL_ROW16)
    ug, flg, gname = run_gpu(lay, gains, g, np.float64, kernel=1)
    assert "row16" in kname and "generic" in gname
    assert ((fl & 0x8) != 0).mean() > 0.8                                    # nearly everything truncates
    err = rel_err(u, ug)
    for b in np.nonzero(~(err <= TOL64))[0]:
        Mx, Minv, Mxi, det = osc_oracle.task_inertia(g["J"][b], g["M"][b])
        assert not in_parity_domain(Mxi, det), (kname, b, err[b])
    idx = np.arange(0, B, 64)                                                # and the generic kernel against the oracle itself
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"],
                                    g.get("wrench"), g.get("tgt_vel"), idx=idx)
    eo = rel_err(ug[idx], ref[idx])
    for b, e in zip(idx, eo):
        if not e <= TOL64:
            Mx, Minv, Mxi, det = osc_oracle.task_inertia(g["J"][b], g["M"][b])
            assert not in_parity_domain(Mxi, det), (gname, b, e)


def test_per_instance_gains_and_branch_b_batch():
    lay, gains, g = synth.make_batch("k13_branch_b", 512, seed=5, per_instance_gains=True)
    u, fl, _ = run_gpu(lay, gains, g, np.float64)
    idx = np.arange(0, 512, 2)
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, g["M"], g["J"], g["dq"], g["bias"],
                                    g["ee_pose"], g["tgt_pose"], g.get("wrench"), g.get("tgt_vel"), idx=idx)
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(g["J"][b], g["M"][b])[2:]) for b in idx])
    assert rel_err(u[idx], ref[idx])[dom].max() <= TOL64


@pytest.mark.parametrize("name", ["e2e_gain_test", "e2e_admit_test", "e2e_single_arm"])
def test_osc_generate_end_to_end_vs_reference(name):
    """Drop-in check: the build's MujocoApp/Robot/Device/OSC.generate on a FakeSim reproduces the
    reference's (force_idxs, forces) for the gain_test and admit_test call patterns."""
    g = load_e2e(name)
    meta = g["meta"]
    for b in range(g["M"].shape[0]):
        app, robot, osc, targets = app_from_e2e(g, b)
        idxs, forces = osc.generate(targets)
        assert [list(map(int, i)) for i in idxs] == meta["force_idxs"]
        flat = np.concatenate(forces)
        ref = g["forces_flat"][b]
        assert np.max(np.abs(flat - ref)) / np.max(np.abs(ref)) <= TOL64
        for i, f in zip(idxs, forces):         # the caller's loop, examples/gain_test.py:146-147
            app.sim.data.ctrl[i] = f


def test_live_device_mutations_match_reference_phase_by_phase():
    """ps_move_example.py:137-150 / insertion_task.py:294 on the HIP path: one OSC object, the devices' ctrlr_dof_abg and
    max_vel[0] changed between generate() calls exactly as the reference run that minted the fixture changed them; the
    layout is re-keyed (angle block of calc_error off, six rows kept), GPU contexts are reused when a masking recurs."""
    from conftest import live_mutation_phases
    g = load_e2e("e2e_live_mutations")
    meta = g["meta"]
    for b in range(g["qM"].shape[0]):
        osc_obj = None
        for p, app, robot, osc, targets in live_mutation_phases(g, b):
            osc_obj = osc
            idxs, forces = osc.generate(targets)
            assert [list(map(int, i)) for i in idxs] == meta["force_idxs"]
            flat, ref = np.concatenate(forces), g["forces_flat"][b, p]
            assert np.max(np.abs(flat - ref)) / np.max(np.abs(ref)) <= TOL64, (b, p)
        assert len(osc_obj._ctx) == 4 and len(osc_obj._layouts) == 4


def test_empty_batch():
    lay, gains, g = synth.make_batch("k13", 4, seed=7)
    for dtype in (np.float64, np.float32):
        osc = BatchedOSC(lay, 4, dtype=dtype)
        osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
        e = lambda *s: np.zeros(s, dtype=dtype)
        out = osc.generate_batched(e(0, 25, 25), e(0, 13, 25), e(0, 25), e(0, 25), e(0, 3, 7), e(0, 3, 7))
        assert out.shape == (0, 25)
        osc.close()


# ---- the kernels that MEET the bar, at the headline size (BASELINE configs[2] / configs[4]) -----------------------------------
def _full_size_physical(cfg, dtype, seed):
    """65 536 records of physical robot states the way bench.py's default workload makes them: uniformly random joint states
    (every 10th robot with stretched / folded arms: each arm angle a multiple of pi / 2, where J loses rank) -> front end on the
    GPU -> targets scattered around the end effectors it found (+ a random wrench on the admittance layout).
    -> (lay, gains, osc with the records resident in slot 0, host copy of the records incl. tgt_pose / wrench)"""
    from irl_control_amd.rigid_body import RigidBodyModel
    B = 65536
    lay = synth.make_layout(cfg)
    _, gains, _ = synth.make_batch(cfg, 2, seed=1, dtype=dtype)            # the YAML gain set of the layout
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(seed)
    osc = BatchedOSC(lay, B, dtype=dtype, kernel=_lib.KERNEL_AUTO)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    qpos, qvel = model.random_state(rng, B)
    idx = np.arange(3, B, 10)
    qpos[idx, 1:7] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    qpos[idx, 13:19] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    osc.upload_q(qpos, qvel)
    osc.frontend()
    rec = osc.download_records(0)
    rec["tgt_pose"] = synth.targets_near(rec["ee_pose"].astype(np.float64), rng).astype(dtype)
    if lay.admittance:
        rec["wrench"] = rng.normal(0.0, 5.0, size=(B, lay.ndev, 6)).astype(dtype)
        osc.upload(rec["M"], rec["J"], rec["dq"], rec["bias"], rec["ee_pose"], rec["wrench"])      # the wrench only arrives with records
    osc.set_targets(rec["tgt_pose"])
    return lay, gains, osc, rec


@pytest.mark.parametrize("cfg,dtype", [("k13", np.float64), ("k13", np.float32), ("k12_admit", np.float64)],
                         ids=["k13-f64", "k13-mixed", "k12_admit-f64"])
def test_row16_tree_full_size(cfg, dtype):
    """The headline kernel at the headline size (BASELINE configs[2]; configs[4] with the admittance term): osc_row16, fp64
    arithmetic, tree-structured factorisation, on 65 536 dense records of physical robot states -- float64 records, float32 records
    (the mixed path: what KERNEL_AUTO gives float32 storage), k12 + wrench.
    (1) the oracle on EVERY one of the 65 536 instances (~15 % of them go through the in-kernel eigen stage, ~12 % truncate):
        <= 1e-5 in the parity domain, PINV / TRUNCATED flags = the reference's branch;
    (2) size-independent properties on ALL 65 536: u is affine in the bias forces with unit slope (osc.py:191), affine in the
        wrench (osc.py:184-185), and the second half of the batch run alone is bit-identical (sharding changes no bit)."""
    B = 65536
    lay, gains, osc, rec = _full_size_physical(cfg, dtype, seed=20241008 + (5 if lay_admit(cfg) else 3))
    assert "row16" in osc.kernel_name and osc.slot_structure(0), osc.kernel_name
    f64 = dtype == np.float64
    u0, fl0 = osc.step(return_flags=True)
    assert not np.any(fl0 & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD)) and np.all(np.isfinite(u0))
    k13 = lay.k == 13            # (without the base's yaw row far fewer task spaces degenerate: 2 % instead of 15 % reach the eigen stage)
    assert (0.05 if k13 else 0.01) < ((fl0 & _lib.FLAG_EIGEN_PATH) != 0).mean() < 0.5
    assert ((fl0 & _lib.FLAG_TRUNCATED) != 0).mean() > (0.03 if k13 else 0.005)
    up = lambda **kw: osc.upload(*[kw.get(k, rec[k]) for k in ("M", "J", "dq", "bias", "ee_pose")], kw.get("wrench", rec.get("wrench")))
    scale = np.maximum(np.abs(u0).max(axis=1, keepdims=True).astype(np.float64), 1.0)
    rnd = 1e-12 if f64 else 3e-7                       # rounding of the sums (float32 records: u is stored as float32)
    kname = osc.kernel_name
    # (2a) affine in bias, unit slope, on every joint of every instance
    up(bias=rec["bias"] + dtype(3.0))
    assert osc.slot_structure(0)
    u1, fl1 = osc.step(return_flags=True)
    assert np.array_equal(fl1, fl0)
    assert np.all(np.abs((u1.astype(np.float64) - u0) - 3.0) <= rnd * scale + (0 if f64 else 3e-7 * np.abs(rec["bias"]).max()))
    # (2b) affine in the wrench
    if lay.admittance:
        up(wrench=np.zeros_like(rec["wrench"]))
        uw0 = osc.step().astype(np.float64)
        up(wrench=(2.0 * rec["wrench"]).astype(dtype))
        uw2 = osc.step().astype(np.float64)
        d1, d2 = u0 - uw0, uw2 - u0
        sc = np.maximum(np.maximum(np.abs(uw2).max(axis=1), np.abs(uw0).max(axis=1)), 1.0)
        lin = np.abs(d2 - d1).max(axis=1) / sc
        # the solve amplifies the rounding of w by cond(J M^-1 J^T) (<= 1e5 on the kept subspace)
        print(f"wrench linearity: median {np.median(lin):.1e}, p99.9 {np.quantile(lin, 0.999):.1e}, max {lin.max():.1e}")
        assert np.quantile(lin, 0.999) <= 1e-7 and lin.max() <= 1e-4, (float(np.quantile(lin, 0.999)), float(lin.max()))
        assert np.abs(d1).max() > 1.0                     # the wrench really acts
    # (2c) the second half alone: bit-identical
    h = B // 2
    osc.upload(rec["M"][h:], rec["J"][h:], rec["dq"][h:], rec["bias"][h:], rec["ee_pose"][h:], rec["wrench"][h:] if lay.admittance else None)
    osc.set_targets(rec["tgt_pose"][h:])
    assert osc.slot_structure(0)
    uh, fh = osc.step(return_flags=True)
    assert np.array_equal(uh, u0[h:]) and np.array_equal(fh, fl0[h:])
    osc.close()
    # (1) the oracle on EVERY instance (forked over the host cores: ~20 core-seconds)
    idx = np.arange(B)
    ref, dom, pinv, trunc, _ = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    err = rel_err(u0[idx].astype(np.float64), ref)
    fs = fl0[idx]
    n_eig = int(((fs & _lib.FLAG_EIGEN_PATH) != 0).sum())
    print(f"{kname}+tree, {B} physical records: oracle on {len(idx)} instances ({n_eig} through the eigen stage, "
          f"{int(trunc.sum())} truncating, {int((~dom).sum())} outside the parity domain): max rel err in the domain {err[dom].max():.2e}")
    assert len(idx) == B and dom.mean() > 0.97 and n_eig >= (6400 if k13 else 800) and trunc.sum() >= (3200 if k13 else 240)
    assert err[dom].max() <= TOL64, float(err[dom].max())
    assert np.array_equal((fs[dom] & _lib.FLAG_PINV_BRANCH) != 0, pinv[dom])
    assert np.array_equal((fs[dom] & _lib.FLAG_TRUNCATED) != 0, trunc[dom])


def lay_admit(cfg):
    return synth.make_layout(cfg).admittance


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kernel", [(np.float32, _lib.KERNEL_AUTO), (np.float64, _lib.KERNEL_AUTO)])
@pytest.mark.parametrize("iters", [1, 2, 7, 8, 9, 17, 24])
def test_step_resident_trains_equal_single_steps(iters, dtype, kernel):
    """irlosc_step_resident chains several steps (8) per launch on the row16 path (blockIdx.y = step, one give-up pass per train),
    float64 and float32 records; whatever the train split, the
    outputs left behind are bit-for-bit those of a plain single step on the last slot visited (n_slots = 3 distinct
    batches, truncation-heavy data so that the eigen stage has work in every step)."""
    nslots, B = 3, 1024 + 16
    lay = synth.make_layout("k13")
    osc = BatchedOSC(lay, B, dtype=dtype, n_slots=nslots, kernel=kernel)
    assert "row16" in osc.kernel_name      # AUTO: fp64 arithmetic on either record type
    batches = []
    for sl in range(nslots):
        _, gains, g = synth.make_batch("k13", B, seed=100 + sl, dtype=dtype)
        osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g.get("wrench"), slot=sl)
        osc.set_targets(g["tgt_pose"], g.get("tgt_vel"), slot=sl)
        batches.append(g)
        if sl == 0:
            osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    assert 1 <= osc.steps_per_launch <= 16
    first = 1
    osc.step_resident(iters, first_slot=first)
    u_train, f_train = osc.download(B)
    last = (first + iters - 1) % nslots
    osc.step(slot=last)
    u_one, f_one = osc.download(B)
    assert (f_one & _lib.FLAG_EIGEN_PATH).mean() > 0.03          # stage 2 really ran
    assert np.array_equal(u_train, u_one) and np.array_equal(f_train, f_one)
    # and a second resident call right after (pending state fully flushed, sets reused) still agrees
    osc.step_resident(iters, first_slot=last)
    u2, f2 = osc.download(B)
    last2 = (last + iters - 1) % nslots
    osc.step(slot=last2)
    u3, f3 = osc.download(B)
    assert np.array_equal(u2, u3) and np.array_equal(f2, f3)
    osc.close()


def test_give_up_instances_inside_trains():
    """Instances whose task Jacobian loses FIVE ranks exceed what stage 2 deflates (three vectors): they must come out
    of the give-up list -> generic kernel path also when steps are chained in trains, and agree with the generic kernel
    run on its own."""
    B = 2048 + 16
    lay, gains, g = synth.make_batch("k13", B, seed=55, dtype=np.float32)
    bad = np.arange(0, B, 9)
    g["J"][bad, 8:13] = g["J"][bad, 0:5]                       # rows 8..12 duplicate rows 0..4: rank k - 5
    g64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in g.items()}
    ref, fref, _ = run_gpu(lay, gains, g64, np.float64, _lib.KERNEL_GENERIC)       # the same (float32-valued) records, Jacobi in fp64
    osc = BatchedOSC(lay, B, dtype=np.float32, n_slots=2, kernel=_lib.KERNEL_AUTO)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    for sl in range(2):
        osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g.get("wrench"), slot=sl)
        osc.set_targets(g["tgt_pose"], g.get("tgt_vel"), slot=sl)
    assert "row16" in osc.kernel_name
    osc.step_resident(11)
    u, fl = osc.download(B)
    gu = osc.giveup_counts() if hasattr(osc, "giveup_counts") else None
    osc.close()
    assert gu is None or max(gu) >= len(bad), gu            # they really went through the give-up lists
    assert np.all(fl[bad] & _lib.FLAG_TRUNCATED) and np.all(fref[bad] & _lib.FLAG_TRUNCATED)
    assert np.all(np.isfinite(u[bad]))
    d = np.abs(u[bad].astype(np.float64) - ref[bad]).max(axis=1) / np.abs(ref[bad]).max(axis=1)
    assert np.median(d) < 1e-3 and np.quantile(d, 0.9) < 5e-2, (float(np.median(d)), float(d.max()))


def test_row16_give_up_counters_do_not_go_stale_across_uneven_trains():
    """step_resident(12) = a train of 8 and one of 4; the give-up pass of the SHORT train used to zero only four of the
    other bank's eight counters, so the next 8-train appended its give-ups behind the lists of two trains ago and the
    generic kernel recomputed those stale ids with the wrong step's data.  Three slots with DIFFERENT give-up sets (five
    lost ranks: beyond the eigen stage's net), uneven calls, then bit-equality with a plain single step."""
    nslots, B = 3, 512 + 4
    lay = synth.make_layout("k13")
    osc = BatchedOSC(lay, B, dtype=np.float64, n_slots=nslots)
    assert "row16" in osc.kernel_name
    for sl in range(nslots):
        _, gains, g = synth.make_batch("k13", B, seed=300 + sl, dtype=np.float64)
        bad = np.arange(sl, B, 7 + sl)
        g["J"][bad, 8:13] = g["J"][bad, 0:5]
        osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g.get("wrench"), slot=sl)
        osc.set_targets(g["tgt_pose"], g.get("tgt_vel"), slot=sl)
        if sl == 0:
            osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    for rep in range(3):
        osc.step_resident(12, first_slot=0)                      # 8 @ bank 0, 4 @ bank 1
        osc.step_resident(8, first_slot=(1 + rep) % nslots)      # 8 @ bank 0 again: step 7 runs slot (1 + rep + 7) % 3
        u_train, f_train = osc.download(B)
        osc.step(slot=(1 + rep + 7) % nslots)
        u_one, f_one = osc.download(B)
        assert np.array_equal(u_train, u_one) and np.array_equal(f_train, f_one), rep
    osc.close()


def test_a_call_whose_later_train_fails_leaves_the_next_call_exact():
    """A call whose THIRD train meets a slot that was never filled fails with IRLOSC_ERR_STATE after two trains went out, the second on
    the other bank's stream; those trains are still joined into the main stream, and the next valid call and its download are bit for
    bit a single step on the last slot visited.  17 slots, the last one empty: step_resident(24) = slots 0..7, 8..15, then slot 16."""
    nslots, B = 17, 516
    lay = synth.make_layout("k13")
    osc = BatchedOSC(lay, B, dtype=np.float64, n_slots=nslots)
    assert "row16" in osc.kernel_name
    batches = [synth.make_batch("k13", B, seed=400 + i, dtype=np.float64) for i in range(3)]
    _, gains, _ = batches[0]
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    for sl in range(nslots - 1):
        g = batches[sl % 3][2]
        osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g.get("wrench"), slot=sl)
        osc.set_targets(g["tgt_pose"], g.get("tgt_vel"), slot=sl)
    with pytest.raises(_lib.IrloscError, match="error -3: slot 16"):
        osc.step_resident(24, first_slot=0, B=B)
    osc.step_resident(12, first_slot=0)                      # 8 @ bank 0, 4 @ bank 1: step 11 runs slot 11
    u_train, f_train = osc.download(B)
    osc.step(slot=11)
    u_one, f_one = osc.download(B)
    assert np.array_equal(u_train, u_one) and np.array_equal(f_train, f_one)
    osc.close()


def test_time_dominant_kernel_leaves_complete_outputs():
    lay, gains, g = synth.make_batch("k13", 4096, seed=9, dtype=np.float32)
    osc = BatchedOSC(lay, 4096, dtype=np.float32)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    ref = osc.generate_batched(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"], g.get("tgt_vel"), g.get("wrench"))
    ms = osc.time_dominant_kernel(16)
    assert ms > 0
    u, _ = osc.download(4096)
    assert np.array_equal(u, ref)
    osc.close()


def test_fleet_example_matches_per_robot_generate():
    """examples/fleet_batched.py (raw arrays -> GPU assembly -> one batched step -> ctrl) gives every robot the
    actuator forces OSC.generate gives that robot alone (the B = 1 drop-in path), fp64."""
    import importlib.util
    import os
    import irl_control_amd as ic
    from irl_control_amd.fakesim import FakeSim, randomize
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "fleet_batched.py")
    spec = importlib.util.spec_from_file_location("fleet_batched", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 24
    ctrl = mod.run(n_robots=n, ticks=1, seed=3, dtype=np.float64, verbose=False)
    rng = np.random.default_rng(3)                     # the same simulators, one robot at a time through OSC.generate
    for b in range(n):
        sim = randomize(FakeSim(), rng, wrench=True)
        app = ic.MujocoApp("default_xyz_abg.yaml", None, sim=sim)
        rob = app.get_robot("DualUR5")
        cfgs = [("ur5right", app.get_controller_config("osc2")), ("ur5left", app.get_controller_config("osc2")),
                ("base", app.get_controller_config("osc0"))]
        osc = ic.OSC(rob, sim, cfgs, app.get_controller_config("nullspace"))
        targets = {}
        for i, nm in enumerate(["ur5right", "ur5left", "base"]):
            dv = rob.get_device(nm)
            t = ic.Target()
            pose = dv.pack_pose7()
            t.set_all_quat(pose[:3] + 0.1 * np.sin(np.arange(3)), pose[3:])
            targets[nm] = t
        expect = np.zeros_like(sim.data.ctrl)
        for idx, f in zip(*osc.generate(targets)):
            expect[idx] = f
        assert np.max(np.abs(ctrl[b] - expect)) <= 1e-9 * max(1.0, np.abs(expect).max()), b


def test_headless_gain_test_loop_runs():
    """examples/gain_test_headless.py: the reference's tick loop (examples/gain_test.py:98-175) on the build's
    classes with an injected simulator; OSC.generate goes through the C ABI every tick."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "gain_test_headless.py")
    spec = importlib.util.spec_from_file_location("gain_test_headless", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.run(ticks=80, demo="figure8", verbose=False)
    assert out["switches"] >= 2 and np.all(np.isfinite(out["ctrl"])) and np.abs(out["ctrl"]).max() > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfg_file,admittance,names", [
    ("default_xyz_abg.yaml", False, ["ur5right", "ur5left", "base"]),
    ("default_xyz_abg.yaml", True, ["ur5right", "ur5left"]),
])
def test_upload_raw_equals_host_state_assembly(dtype, cfg_file, admittance, names):
    """irlosc_upload_raw (state assembly on the GPU from raw simulator arrays) against the host classes that mirror
    the reference (Robot.get_all_states / Device.get_state, pinned by the end-to-end goldens): same torques.  Scene
    with two free bodies (nv = 37 > n = 25) so that the row / column picking really picks."""
    import irl_control_amd as ic
    from irl_control_amd import raw
    from irl_control_amd.device import DeviceState
    from irl_control_amd.fakesim import FakeModel, FakeSim, dual_ur5_actuated_joints, dual_ur5_tree, randomize
    from irl_control_amd.robot import RobotState
    B = 48
    rng = np.random.default_rng(77)
    sims, robots, apps = [], [], []
    for b in range(B):
        tn, tp, tj = dual_ur5_tree()
        sim = randomize(FakeSim(FakeModel(tn, tp, tj, dual_ur5_actuated_joints(), n_free_bodies=2)), rng, wrench=True)
        app = ic.MujocoApp(cfg_file, None, sim=sim)
        sims.append(sim); apps.append(app); robots.append(app.get_robot("DualUR5"))
    rob = robots[0]
    devs = [rob.get_device(nm) for nm in names]
    lay = OSCLayout.from_devices(devs, rob, use_g=True, admittance=admittance, nullspace=True) if hasattr(OSCLayout, "from_devices") else None
    if lay is None:
        pytest.skip("OSCLayout.from_devices not available")
    # host path: what OSC.generate assembles per robot (osc.py:132-138), stacked into a batch
    M = np.stack([r.get_state(RobotState.M) for r in robots])
    dq = np.stack([r.get_state(RobotState.DQ) for r in robots])
    Jl = []
    for r in robots:
        Js, _ = r.get_state(RobotState.J)
        Jl.append(np.vstack([Js[nm] for nm in names]))
    J = np.stack(Jl)
    bias = np.stack([np.asarray(s.data.qfrc_bias)[r.joint_ids_all] for s, r in zip(sims, robots)])
    ee = np.stack([[r.get_device(nm).pack_pose7() for nm in names] for r in robots])
    wr = np.stack([[r.get_device(nm).pack_wrench6() for nm in names] for r in robots])
    tgt = ee.copy()
    tgt[:, :, :3] += rng.normal(0, 0.2, size=tgt[:, :, :3].shape)
    gains = dict(kp=[200.0] * len(names), kv=[30.0] * len(names), ko=[180.0] * len(names), k=[[1, 1, 1]] * len(names),
                 d=[[0.5, 0.5, 0.5]] * len(names), max_vel=[[0.5, 1.0]] * len(names), null_kv=10.0)
    osc = BatchedOSC(lay, B, dtype=dtype)
    osc.set_gains(**gains)
    osc.upload(M, J, dq, bias, ee, wr)
    osc.set_targets(tgt)
    u_host = osc.step()
    arrs = raw.collect_raw(sims, robots, names, dtype=np.float64)
    osc.upload_raw(raw.raw_desc(rob, names, arrs["sensordata"].shape[1]), **arrs)
    osc.set_targets(tgt)
    u_raw = osc.step()
    osc.close()
    assert np.all(np.isfinite(u_host))
    if admittance:      # the 3 x 3 F/T rotation may round differently from NumPy's matmul in the last bit
        tol = 1e-12 if dtype == np.float64 else 1e-5
        assert np.max(np.abs(u_raw - u_host) / np.abs(u_host).max(axis=1, keepdims=True)) < tol
    else:
        assert np.array_equal(u_raw, u_host)


def test_assemble_device_from_gpu_resident_raw_state():
    """irlosc_assemble_device: raw simulator arrays that already live in HBM (here: hipMalloc'ed buffers) -> resident slot,
    no copies; the following step must equal the host-staged irlosc_upload_raw path bit for bit."""
    import ctypes as C
    hb = HipBuffers()
    B, nv, ns = 256, 37, 18
    lay = synth.make_layout("k13")
    rng = np.random.default_rng(5)
    f = np.float32
    spd = rng.normal(size=(B, nv, nv))
    arr = dict(qM=(spd @ spd.transpose(0, 2, 1) / nv + np.eye(nv)).astype(f), qvel=rng.normal(size=(B, nv)).astype(f),
               qfrc_bias=rng.normal(size=(B, nv)).astype(f), jacp=rng.normal(size=(B, 3, 3, nv)).astype(f),
               jacr=rng.normal(size=(B, 3, 3, nv)).astype(f), ee_xpos=rng.normal(size=(B, 3, 3)).astype(f),
               ee_xquat=rng.normal(size=(B, 3, 4)).astype(f), site_xmat=rng.normal(size=(B, 3, 9)).astype(f),
               sensordata=rng.normal(size=(B, ns)).astype(f))
    d = _lib.RawDesc()
    d.nv, d.n_sensor = nv, ns
    for p_ in range(32):
        d.joint_ids[p_] = p_ + 3 if p_ < 25 else 0           # the robot's dofs sit behind three others
        d.dq_src[p_] = p_ if p_ < 25 else -1
    for i in range(4):
        d.ft_force0[i], d.ft_torque0[i] = (6 * i, 6 * i + 3) if i < 2 else (-1, -1)
    _, gains, g = synth.make_batch("k13", B, seed=2, dtype=f)
    osc = BatchedOSC(lay, B, dtype=f)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload_raw(d, **arr)
    osc.set_targets(g["tgt_pose"])
    u_ref = osc.step()
    dev = {k: hb.to_device(v) for k, v in arr.items()}
    pp = lambda t: t
    # scribble over the slot first so that a no-op would be noticed
    osc.upload(np.zeros((B, 25, 25), f) + np.eye(25, dtype=f), np.zeros((B, 13, 25), f), np.zeros((B, 25), f),
               np.zeros((B, 25), f), g["ee_pose"], None)
    rc = osc.lib.irlosc_assemble_device(osc._h, 0, B, C.byref(d), pp(dev["qM"]), pp(dev["qvel"]), pp(dev["qfrc_bias"]),
                                        pp(dev["jacp"]), pp(dev["jacr"]), pp(dev["ee_xpos"]), pp(dev["ee_xquat"]),
                                        pp(dev["site_xmat"]), pp(dev["sensordata"]), None)
    assert rc == 0, osc.lib.irlosc_last_error(osc._h)
    u_dev = osc.step()
    osc.close()
    hb.free()
    assert np.all(np.isfinite(u_ref)) and np.array_equal(u_dev, u_ref)


def test_step_device_raw_pointers():
    """irlosc_step_device: caller-owned device buffers (hipMalloc'ed here), no copies by the library."""
    hb = HipBuffers()
    B = 512
    lay, gains, g = synth.make_batch("k13", B, seed=8, dtype=np.float32)
    ref, _, _ = run_gpu(lay, gains, g, np.float32)
    osc = BatchedOSC(lay, B, dtype=np.float32)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    dev = {k: hb.to_device(v) for k, v in g.items()}
    u, fl = hb.alloc(B * 25 * 4), hb.to_device(np.zeros(B, np.uint32))
    rc = osc.lib.irlosc_step_device(osc._h, B, dev["M"], dev["J"], dev["dq"], dev["bias"], dev["ee_pose"],
                                    dev["tgt_pose"], None, None, u, fl, None)
    assert rc == 0, osc.lib.irlosc_last_error(osc._h)
    osc.sync()
    assert np.array_equal(hb.to_host(u, (B, 25), np.float32), ref)
    osc.close()
    hb.free()


def test_call_order_and_argument_errors():
    lay, gains, g = synth.make_batch("k13", 32, seed=1, dtype=np.float32)
    osc = BatchedOSC(lay, 32, dtype=np.float32)
    with pytest.raises(_lib.IrloscError, match="upload"):
        osc._B[0] = 32
        osc.step()                                   # step before upload / set_targets / set_gains
    osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"])
    osc.set_targets(g["tgt_pose"])
    with pytest.raises(_lib.IrloscError, match="set_gains"):
        osc.step()
    with pytest.raises(ValueError):
        osc.upload(g["M"][:, :24], g["J"], g["dq"], g["bias"], g["ee_pose"])      # wrong shape
    with pytest.raises(_lib.IrloscError, match="removed in ABI version 3"):
        BatchedOSC(lay, 32, dtype=np.float32, kernel=2)            # the fp32-ARITHMETIC kernel of ABI versions 1-2: gone (it missed 1e-5)
    osc.close()


# ------------------------------------------------------------------------------------------------
# fp64-arithmetic throughput (row16) path: fp64 records, and fp32 records with fp64 arithmetic (mixed)
# ------------------------------------------------------------------------------------------------
def _round32(g):
    return {k: (v.astype(np.float32).astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v)
            for k, v in g.items()}


@pytest.mark.parametrize("name", golden_names())
def test_mixed_path_meets_1e5_on_fp32_rounded_goldens(name):
    """north_star's 1e-5 on float32 RECORDS: the reference-minted fixtures rounded to float32, run through the row16
    kernel (fp32 storage, fp64 arithmetic), against the float64 oracle on the same rounded inputs.  Gate 1e-5 flat
    on the parity domain of the rounded problem (no condition-number allowance).  Every fixture: the layouts beyond the four
    instantiated shapes (target subsets, other row masks, exact zero rows) run the KMAX-padded kernels."""
    g = load_golden(name)
    lay = OSCLayout.from_dict(g["layout"])
    if lay.n != 25:
        pytest.skip("the row16 kernels are instantiated for n = 25")
    g32 = _round32(g)
    u, fl, kname = run_gpu(lay, golden_gains(g), g32, np.float32, _lib.KERNEL_ROW16)
    assert "row16_f32in_f64" in kname
    ref = osc_oracle.generate_batch(g["layout"], golden_gains(g), g32["M"], g32["J"], g32["dq"], g32["bias"],
                                    g32["ee_pose"], g32["tgt_pose"], g32["wrench"], g32["tgt_vel"])
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(g32["J"][b], g32["M"][b])[2:])
                    for b in range(g["M"].shape[0])])
    if name == "k13_gimbal":       # the float32-rounded poses are no longer at gimbal lock; nothing else changes
        assert dom.sum() > 0
    err = rel_err(u, ref)
    assert dom.sum() >= 0.6 * len(dom)
    assert err[dom].max() <= TOL64, (kname, name, float(err[dom].max()))
    assert not np.any(fl[dom] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))


@pytest.mark.parametrize("cfg", ["k13", "k7", "k12_admit"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row16_vs_oracle_flat_1e5(cfg, dtype):
    """1 024 synthetic instances per layout (11 % of them on the truncated-pinv path) on the row16 kernel, float64
    records and float32 records (mixed): every in-domain instance within 1e-5, flags consistent with the reference's
    branch (osc.py:52) and with the singular values it would cut."""
    B = 1024
    lay, gains, g = synth.make_batch(cfg, B, seed=99)
    gin = _round32(g) if dtype == np.float32 else g
    u, fl, kname = run_gpu(lay, gains, gin, dtype, _lib.KERNEL_ROW16)
    assert "row16" in kname
    idx = np.arange(0, B, 2)
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, gin["M"], gin["J"], gin["dq"], gin["bias"],
                                    gin["ee_pose"], gin["tgt_pose"], gin.get("wrench"), gin.get("tgt_vel"), idx=idx)
    dom, small_det, cut = [], [], []
    for b in idx:
        Mx, Minv, Mxi, det = osc_oracle.task_inertia(gin["J"][b], gin["M"][b])
        s = np.linalg.svd(Mxi, compute_uv=False)
        dom.append(in_parity_domain(Mxi, det))
        small_det.append(abs(det) < 1e-4)
        cut.append(abs(det) < 1e-4 and s[-1] <= 1e-5 * s[0])
    dom, small_det, cut = np.array(dom), np.array(small_det), np.array(cut)
    err = rel_err(u[idx], ref[idx])
    assert dom.mean() > 0.9
    assert err[dom].max() <= TOL64, (kname, float(err[dom].max()))
    assert np.array_equal((fl[idx][dom] & _lib.FLAG_PINV_BRANCH) != 0, small_det[dom])
    assert np.array_equal((fl[idx][dom] & _lib.FLAG_TRUNCATED) != 0, cut[dom])
    assert np.all(np.isfinite(u))


@pytest.mark.parametrize("B", [1, 3, 4, 5, 17, 100])
def test_row16_ragged_batches_and_sharding_bit_exact(B):
    """A wave carries four instances: batch sizes around that, and a split at an offset that changes every
    instance's wave-mates.  Each instance must come out bit-identical to what the large batch gives (the eigen path
    freezes an instance at its own convergence, so nothing depends on its neighbours)."""
    lay, gains, g = synth.make_batch("k13", 512, seed=21)
    full, ffull, name = run_gpu(lay, gains, g, np.float64, _lib.KERNEL_ROW16)
    assert "row16" in name and (ffull & _lib.FLAG_EIGEN_PATH).any()
    sub = {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    part, fl, _ = run_gpu(lay, gains, sub, np.float64, _lib.KERNEL_ROW16)
    assert np.array_equal(part, full[:B]) and np.array_equal(fl, ffull[:B])
    off = 257 + B % 3
    tail = {k: (v[off:] if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    ut, ft, _ = run_gpu(lay, gains, tail, np.float64, _lib.KERNEL_ROW16)
    assert np.array_equal(ut, full[off:]) and np.array_equal(ft, ffull[off:])


def _bench_line(extra_args, env_extra, launcher):
    """Run bench.py in a child process, small and quick; -> (parsed JSON line, number of JSON lines on stdout)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["bench.py", "--full", "--steps", "16", "--warmup", "8", "--preroll", "0", "--batch", "2048", "--no-cpu-baseline",
            "--no-secondary", "--no-from-q", "--sustained-steps", "4000"] + extra_args
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(env_extra)
    cmd = [sys.executable] + (launcher or []) + args
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]), len(lines)


def test_bench_two_ranks_self_launched_and_under_a_launcher():
    """SURVEY 8e on the one GPU a test box has: `python bench.py --gpus 2` with no launcher environment starts its two
    workers itself; under `python -m torch.distributed.run` it behaves as before.  Both ranks share device 0
    (IRLOSC_BENCH_DEVICE), so RCCL refuses the duplicate device and every rank switches to the file reduction TOGETHER.
    One JSON line, n_gpus = 2, two checksums, and rank 0's checksum is the one the 1-rank run gives (rank r's data
    depend on r only: sharding changes no bit)."""
    one, n1 = _bench_line(["--gpus", "1"], {}, None)
    assert n1 == 1 and one["n_gpus"] == 1 and len(one["rank_checksums"]) == 1
    own, n2 = _bench_line(["--gpus", "2"], {"IRLOSC_BENCH_DEVICE": "0"}, None)
    assert n2 == 1 and own["n_gpus"] == 2 and len(own["rank_checksums"]) == 2
    assert own["rank_checksums"][0] == one["rank_checksums"][0] and own["rank_checksums"][1] != own["rank_checksums"][0]
    assert own["value"] > 0 and own["config"]["instances_per_gpu"] == 2048
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    tr, n3 = _bench_line(["--gpus", "2"], {"IRLOSC_BENCH_DEVICE": "0"},
                         ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port)])
    assert n3 == 1 and tr["n_gpus"] == 2 and tr["rank_checksums"] == own["rank_checksums"]
    for line in (own, tr):
        assert "RCCL" in line["config"]["sharding"] or "files" in line["config"]["sharding"]


@pytest.mark.parametrize("fail_hand_over", [False, True])
def test_bench_line_with_the_cpu_legs_on_the_physical_workload(fail_hand_over):
    """The default workload's records come out of the GPU, the CPU legs fork before the bench process touches HIP: a child
    process computes slot 0 and hands it over (the parent checks the CRC against its own slot 0).  The line carries the CPU
    baseline and a parity sample of the tree-form kernel against the oracle on those records.  With the hand-over failing
    (IRLOSC_BENCH_FAIL_MINT) the line still comes out: CPU timing on synthetic records, said so, parity in-process."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    if fail_hand_over:
        env["IRLOSC_BENCH_FAIL_MINT"] = "1"
    cmd = [sys.executable, "bench.py", "--full", "--steps", "16", "--warmup", "8", "--preroll", "0", "--batch", "4096", "--cpu-seconds", "0.5",
           "--no-secondary", "--no-from-q", "--sustained-steps", "4000"]
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["config"]["records_from"] == "physical" and line["config"]["kernel"].endswith("+tree")
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["kind"] == "port"
    assert ("SYNTHETIC records" in line["cpu_baseline"]["sample"]) == fail_hand_over
    ps = line["parity_sample"]
    assert ps["n"] >= 512 and ps["n_over_tol_in_parity_domain"] == 0 and ps["max_rel_err"] <= TOL64
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1
    assert line["end_to_end"]["generate_batched"]["value"] > 0


@pytest.mark.parametrize("lost", [1, 2, 3, 5])
def test_row16_rank_deficient_jacobians(lost):
    """Exactly singular task Jacobians (duplicated rows: `lost` zero eigenvalues of J M^-1 J^T): the plain
    factorisation breaks down, the shifted one takes over, up to three null vectors are deflated in the kernel and
    more than three go through the give-up list to the Jacobi kernel.  The reference answer (pinv) is well defined."""
    B = 256
    lay, gains, g = synth.make_batch("k13", B, seed=55)
    bad = np.arange(0, B, 3)
    g["J"][bad, 13 - lost:13] = g["J"][bad, 0:lost]
    u, fl, name = run_gpu(lay, gains, g, np.float64, _lib.KERNEL_ROW16)
    assert "row16" in name
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"],
                                    g["tgt_pose"], g.get("wrench"), g.get("tgt_vel"), idx=bad)
    assert np.all(fl[bad] & _lib.FLAG_TRUNCATED) and np.all(fl[bad] & _lib.FLAG_PINV_BRANCH)
    err = rel_err(u[bad], ref[bad])
    assert err.max() <= TOL64, (lost, float(err.max()))
    # the give-up counter: more than three lost directions go to the generic kernel, up to three stay in the wave
    osc = BatchedOSC(lay, B, dtype=np.float64, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.generate_batched(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"])
    n_give = int(osc.giveup_counts()[0])
    osc.close()
    assert (n_give >= len(bad)) if lost > 3 else (n_give <= len(bad) // 8), (lost, n_give)


def test_rccl_throughput_reduction_single_rank():
    """irlosc_comm_* / irlosc_bench_allreduce on the one GPU of this box: unique id, communicator of world size 1,
    sum / max reduction and checksum all-gather through RCCL (the N > 1 bookkeeping is covered by the gloo test)."""
    from irl_control_amd import sharding
    comm = sharding.RcclComm(0, 1, 0, tag=f"gputest_{__import__('os').getpid()}")
    assert comm.reduce(123.0, 4.5) == (123.0, 4.5)
    assert comm.allgather_u64(0xDEADBEEF12345678) == [0xDEADBEEF12345678]
    assert sharding.reduce_throughput(100.0, 4.0, comm) == (100.0, 4.0, 25.0)
    comm.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tick_equals_upload_targets_step(dtype):
    """irlosc_tick (one call, one sync) gives bit for bit what upload + set_targets + step give."""
    lay, gains, g = synth.make_batch("k12_admit", 37, seed=3, dtype=dtype)
    osc = BatchedOSC(lay, 64, dtype=dtype)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    ref, fref = osc.generate_batched(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"], None, g["wrench"],
                                     return_flags=True)
    u, fl = osc.tick(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"], None, g["wrench"], return_flags=True)
    assert np.array_equal(u, ref) and np.array_equal(fl, fref)
    one = [g[k][:1] for k in ("M", "J", "dq", "bias", "ee_pose", "tgt_pose")]
    u1 = osc.tick(*one, None, g["wrench"][:1])
    assert np.array_equal(u1, osc.generate_batched(*one, None, g["wrench"][:1]))
    osc.close()


# ------------------------------------------------------------------------------------------------
# Caller loops (harness rows): per-tick goldens minted by the reference
# ------------------------------------------------------------------------------------------------
def _load_example(name):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", name + ".py")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_loop_golden(name):
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return {k: z[k] for k in z.files if k != "layout_json"}, json.loads(str(z["layout_json"]))


def test_gain_test_loop_matches_reference_tick_by_tick():
    """examples/gain_test.py:98-175 headless: 160 ticks, the reference's forces of EVERY tick (minted by
    oracle/make_golden.py with the reference's own OSC on the same FakeSim + ToyDynamics) against OSC.generate on the
    HIP path; also the waypoint indices, i.e. the caller-side logic that reads Device state between ticks."""
    g, meta = _load_loop_golden("loop_gain_test")
    mod = _load_example("gain_test_headless")
    rec = mod.run(ticks=meta["ticks"], demo="gain_test", seed=meta["seed"], robot_config=meta["cfg_file"], verbose=False)
    assert rec["idxs"] == meta["idxs"]
    assert np.array_equal(rec["wp"], g["wp"]) and (np.diff(g["wp"], axis=0) != 0).sum() >= 2
    assert np.allclose(rec["err"], g["err"], rtol=0, atol=1e-12)
    err = np.abs(rec["forces"] - g["forces"]).max(axis=1) / np.abs(g["forces"]).max(axis=1)
    assert err.max() <= TOL64, float(err.max())


def test_admit_test_loop_matches_reference_tick_by_tick():
    """examples/admit_test.py:43-80 headless: admittance on, left arm abg = [0, -pi/2, 0], push on the left gripper
    during ticks 40..80 of 120; every tick's forces against the reference's, and the push must be visible in them."""
    g, meta = _load_loop_golden("loop_admit_test")
    mod = _load_example("admit_test_headless")
    rec = mod.run(ticks=meta["ticks"], push_window=tuple(meta["push_window"]), seed=meta["seed"], verbose=False)
    assert rec["idxs"] == meta["idxs"]
    err = np.abs(rec["forces"] - g["forces"]).max(axis=1) / np.abs(g["forces"]).max(axis=1)
    assert err.max() <= TOL64, float(err.max())
    lo, hi = meta["push_window"]
    jump_in = np.abs(g["forces"][lo + 1] - g["forces"][lo]).max()        # first tick that sees the wrench
    jump_before = np.abs(g["forces"][lo] - g["forces"][lo - 1]).max()
    assert jump_in > 2 * jump_before


@pytest.mark.parametrize("demo", ["space_mouse", "ps_move"])
def test_teleoperation_loops_match_the_reference_tick_by_tick(demo):
    """The two teleoperation callers of OSC.generate (examples/space_mouse_example.py:141-143,
    examples/ps_move_example.py:154-159), headless on scripted input streams: the goldens are what the REFERENCE's own loop
    bodies (SpaceMouseDemo.run_demo with the reference's SpaceMouse integrator; PSMoveExample.run with its button poll) wrote
    into sim.data.ctrl tick by tick; here the same streams go through examples/teleop_loops.py and OSC.generate on the HIP
    path.  ps_move: the triggers switch `ctrlr_dof_abg` of live devices (orientation error off, rows kept), released arms
    hold their own position, the gripper position actuators (ctrl 7 / 14) follow circle / triangle."""
    g, meta = _load_loop_golden("loop_" + demo)
    mod = _load_example("teleop_headless")
    rec = mod.run(demo=demo, ticks=meta["ticks"], seed=meta["seed"], rate=meta["rate"], button_every=meta["button_every"], verbose=False)
    assert rec["ctrl"].shape == g["ctrl"].shape
    err = np.abs(rec["ctrl"] - g["ctrl"]).max(axis=1) / np.abs(g["ctrl"]).max(axis=1)
    assert err.max() <= TOL64, (int(np.argmax(err)), float(err.max()))
    if demo == "ps_move":
        eng = rec["engaged"]
        assert (np.diff(eng.astype(int), axis=0) != 0).sum() >= 4              # both arms engaged and released several times
        assert np.array_equal(rec["ctrl"][:, [7, 14]], g["ctrl"][:, [7, 14]])  # gripper set-points: caller-side logic, exact
        assert g["ctrl"][:, 7].max() >= 0.3


# ------------------------------------------------------------------------------------------------
# Rigid-body front end: records from (qpos, qvel) on the GPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["k13", "k7", "k12_admit"])
def test_frontend_records_and_step_from_q(cfg):
    """irlosc_frontend against the float64 rigid-body oracle (itself pinned by physics identities, tests/test_rigid_body.py):
    the torques of step_from_q equal, to 1e-9, those of the OSC step on the oracle's records, and equal the OSC oracle
    on those records to 1e-5 in the parity domain."""
    from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
    from oracle import rigid_body as rb
    B = 64
    lay = synth.make_layout(cfg)
    _, gains, g = synth.make_batch(cfg, B, seed=3)
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(17)
    qpos, qvel = model.random_state(rng, B)
    om = rb.Model()
    recs = [rb.records(om, lay.as_oracle_dict(), DUAL_UR5_EE, qpos[b], qvel[b]) for b in range(B)]
    R = {k: np.array([r[k] for r in recs]) for k in ("M", "J", "dq", "bias", "ee_pose")}
    tgt = R["ee_pose"].copy()
    tgt[:, :, :3] += rng.normal(0.0, 0.2, size=tgt[:, :, :3].shape)
    osc = BatchedOSC(lay, B, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    u_q, fl_q = osc.step_from_q(qpos, qvel, tgt, return_flags=True)
    u_r, fl_r = osc.generate_batched(R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], tgt, return_flags=True)
    osc.close()
    assert np.array_equal(fl_q & 0x4f, fl_r & 0x4f)
    d = np.abs(u_q - u_r).max(axis=1) / np.abs(u_r).max(axis=1)
    assert d.max() <= 1e-9, float(d.max())
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], tgt)
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(R["J"][b], R["M"][b])[2:]) for b in range(B)])
    assert dom.sum() >= B // 2
    assert rel_err(u_q, ref)[dom].max() <= TOL64


def _from_q_setup(cfg, B, dtype, seed, n_slots=1, singular_every=0):
    from irl_control_amd.rigid_body import RigidBodyModel
    lay = synth.make_layout(cfg)
    _, gains, g = synth.make_batch(cfg, B, seed=seed, dtype=dtype)
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(seed + 1000)
    osc = BatchedOSC(lay, B, dtype=dtype, n_slots=n_slots, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    states = []
    for sl in range(n_slots):
        qpos, qvel = model.random_state(rng, B)
        if singular_every:                   # stretched / folded arms: every angle of the two arms a multiple of pi / 2
            idx = np.arange(sl, B, singular_every)
            qpos[idx, 1:7] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
            qpos[idx, 13:19] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
        osc.upload_q(qpos, qvel, slot=sl)
        osc.set_targets(g["tgt_pose"], g.get("tgt_vel"), slot=sl)
        states.append((qpos, qvel))
    return lay, gains, g, model, osc, states


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfg", ["k13", "k7", "k12_admit"])
def test_fused_from_q_equals_the_path_through_dense_records(cfg, dtype, monkeypatch):
    """SURVEY 8 f1, fused form: lane-per-robot walk -> compact exchange buffer -> row16 kernel gathering its operands
    (no dense M / J in HBM) against the same two kernels' arithmetic through dense records (irlosc_frontend +
    irlosc_step).  In float64 the operands are the same numbers, so the torques agree to rounding; with float32 records
    the dense path ROUNDS M / J / bias to float32 on the way while the fused path hands them over in float64, so there the
    comparison is at the float32-records tolerance.  Flags equal.  Singular arm configurations (all arm angles multiples
    of pi / 2) are mixed in: the eigen stage and the give-up hand-over run on both paths."""
    B = 2048 + 37
    lay, gains, g, model, osc, states = _from_q_setup(cfg, B, dtype, seed=5, singular_every=9)
    assert "fused" in osc.from_q_name and "compact" in osc.from_q_name
    u_f, fl_f = osc.step_q(return_flags=True)
    osc.frontend()
    u_d, fl_d = osc.step(return_flags=True)
    osc.close()
    assert np.all(np.isfinite(u_f))
    if cfg != "k7":            # (three translational rows per arm stay well conditioned: no eigen stage there)
        assert (fl_f & _lib.FLAG_EIGEN_PATH).mean() > 0.02
    d = np.abs(u_f.astype(np.float64) - u_d).max(axis=1) / np.abs(u_d).max(axis=1)
    if dtype == np.float64:
        assert np.array_equal(fl_f, fl_d)
        assert d.max() <= 1e-9, float(d.max())
    else:
        same = ((fl_f ^ fl_d) & (_lib.FLAG_PINV_BRANCH | _lib.FLAG_TRUNCATED)) == 0
        assert same.mean() > 0.97
        assert np.median(d) <= 1e-5 and np.quantile(d[same], 0.99) <= 1e-2, (float(np.median(d)), float(np.quantile(d[same], 0.99)))
    monkeypatch.setenv("IRLOSC_FUSED", "0")            # and the library's own switch gives the two-kernel path
    lay, gains, g, model, osc2, _ = _from_q_setup(cfg, B, dtype, seed=5, singular_every=9)
    assert "through dense records" in osc2.from_q_name
    u_2, fl_2 = osc2.step_q(return_flags=True)
    osc2.close()
    assert np.array_equal(u_2, u_d) and np.array_equal(fl_2, fl_d)


def test_fused_from_q_against_the_chained_oracles():
    """The fused path end to end against oracle/rigid_body.py -> oracle/osc_oracle.py on the same (qpos, qvel, targets):
    north_star's 1e-5 in the parity domain."""
    from irl_control_amd.rigid_body import DUAL_UR5_EE
    from oracle import rigid_body as rb
    B = 96
    lay, gains, g, model, osc, states = _from_q_setup("k13", B, np.float64, seed=23, singular_every=0)
    u, fl = osc.step_q(return_flags=True)
    osc.close()
    qpos, qvel = states[0]
    om = rb.Model()
    recs = [rb.records(om, lay.as_oracle_dict(), DUAL_UR5_EE, qpos[b], qvel[b]) for b in range(B)]
    R = {k: np.array([r[k] for r in recs]) for k in ("M", "J", "dq", "bias", "ee_pose")}
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], g["tgt_pose"])
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(R["J"][b], R["M"][b])[2:]) for b in range(B)])
    assert dom.sum() >= B // 2 and rel_err(u, ref)[dom].max() <= TOL64


@pytest.mark.parametrize("cfg", ["k13", "k12_admit", "k7"])
def test_fused_lane_path_full_size_oracle_on_every_robot(cfg):
    """The fused path (lane-per-robot walk -> exchange buffer -> lane-per-robot OSC step -> eigen pass on compact records) at the
    headline size: 65 536 robots from (qpos, qvel), a seventh of them with stretched / folded arms.  The oracle runs on EVERY robot:
    oracle/osc_oracle.generate_batch on the dense records of the same states (GPU front end, itself held to oracle/rigid_body.py at
    1e-10 by test_frontend_records_themselves and chained end to end by the test above): <= 1e-5 in the parity domain, PINV /
    TRUNCATED flags = the reference's branch (osc.py:51-55).  Tiers (1, 6, 6) [k13, k12 + admittance] and (1, 3, 3) [k7]."""
    B = 65536
    lay, gains, g, model, osc, states = _from_q_setup(cfg, B, np.float64, seed=611, singular_every=7)
    if lay.admittance:
        osc.frontend()
        rec0 = osc.download_records(0)
        osc.upload(rec0["M"], rec0["J"], rec0["dq"], rec0["bias"], rec0["ee_pose"], g["wrench"])   # the wrench only arrives with records ...
        osc.upload_q(*states[0])                                                                  # ... and stays with the slot
        osc.set_targets(g["tgt_pose"])
    assert "osc_lane" in osc.from_q_name, osc.from_q_name
    u, fl = osc.step_q(return_flags=True)
    assert np.all(np.isfinite(u)) and not np.any(fl & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    osc.frontend()
    rec = osc.download_records(0)
    osc.close()
    rec["tgt_pose"] = g["tgt_pose"]
    if lay.admittance:
        rec["wrench"] = g["wrench"]
    ref, dom, pinv, trunc, _ = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    err = rel_err(u.astype(np.float64), ref)
    n_eig = int(((fl & _lib.FLAG_EIGEN_PATH) != 0).sum())
    print(f"{osc.from_q_name if False else cfg}: oracle on {B} robots ({n_eig} through the eigen pass, {int(trunc.sum())} truncating, "
          f"{int((~dom).sum())} outside the parity domain): max rel err in the domain {err[dom].max():.2e}")
    assert dom.mean() > 0.97
    if cfg != "k7":
        assert n_eig >= 800 and trunc.sum() >= 240
    assert err[dom].max() <= TOL64, float(err[dom].max())
    assert np.array_equal((fl[dom] & _lib.FLAG_PINV_BRANCH) != 0, pinv[dom])
    assert np.array_equal((fl[dom] & _lib.FLAG_TRUNCATED) != 0, trunc[dom])


def test_structural_walk_equals_the_shape_only_walk(monkeypatch):
    """The fused path's walk exists twice: with the structural constants of the Dual-UR5's MJCF compiled in (TopoDualUr5S: frames not
    rotated against / coincident with their parent's, hinges about coordinate axes through their body's origin, diagonal body-frame
    inertias -- products with those exact zeros and ones left out) and shape-only (any numbers).  irlosc_set_model picks the first
    for the shipped model; IRLOSC_WALK=general forces the second.  Same mathematics: torques agree to rounding, flags exactly."""
    B = 2048 + 11
    lay, gains, g, model, osc, _ = _from_q_setup("k13", B, np.float64, seed=31, singular_every=6)
    assert "compact_dual_ur5_s +" in osc.from_q_name
    u_s, fl_s = osc.step_q(return_flags=True)
    osc.close()
    monkeypatch.setenv("IRLOSC_WALK", "general")
    lay, gains, g, model, osc, _ = _from_q_setup("k13", B, np.float64, seed=31, singular_every=6)
    assert "compact_dual_ur5 +" in osc.from_q_name
    u_g, fl_g = osc.step_q(return_flags=True)
    osc.close()
    assert np.array_equal(fl_s, fl_g)
    d = np.abs(u_s - u_g).max(axis=1) / np.abs(u_g).max(axis=1)
    assert d.max() <= 1e-9, float(d.max())


def test_a_model_without_the_structural_constants_runs_the_shape_only_walk(tmp_path):
    """A robot with the Dual-UR5's tree SHAPE but other numbers where the MJCF has its exact zeros and ones -- a tilted hinge axis, an
    anchor off the body origin, a rotated body frame, a rotated inertial frame, a shifted frame origin -- must not get the walk those
    constants are compiled into: irlosc_set_model falls back to the shape-only instantiation (still the fused path), and the result
    equals the chained oracles on the SAME perturbed model."""
    import copy
    import json
    from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
    from oracle import rigid_body as rb
    base = RigidBodyModel.load("dual_ur5")
    table = copy.deepcopy(base.table)
    bodies = table["bodies"]
    nrm = lambda v: [float(x) for x in (np.asarray(v, float) / np.linalg.norm(v))]
    hinge_bodies = [i for i, b in enumerate(bodies) if b["joint"]]
    bodies[hinge_bodies[3]]["joint"]["axis"] = nrm([1.0, 0.15, -0.1])          # a hinge that is no coordinate axis
    bodies[hinge_bodies[9]]["joint"]["pos"] = [0.01, -0.02, 0.005]             # an anchor off the body origin
    bodies[10]["quat"] = nrm([0.99, 0.05, -0.08, 0.02])                        # ur_EE_ur5right no longer aligned with link6
    bodies[2]["pos"] = [0.0, 0.0, 0.3]                                         # the base's EE frame off the stand's origin
    bodies[5]["iquat"] = nrm([0.9, 0.3, 0.1, -0.2])                            # link2: inertial frame rotated
    bodies[11]["ipos"] = [0.0, 0.003, 0.01]
    path = tmp_path / "dual_ur5_perturbed.json"
    path.write_text(json.dumps(table))
    model = RigidBodyModel.load(str(path))
    B = 96
    lay = synth.make_layout("k13")
    _, gains, g = synth.make_batch("k13", B, seed=5)
    qpos, qvel = model.random_state(np.random.default_rng(6), B)
    osc = BatchedOSC(lay, B, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    assert "compact_dual_ur5 +" in osc.from_q_name and "fused" in osc.from_q_name, osc.from_q_name
    u = osc.step_from_q(qpos, qvel, g["tgt_pose"])
    osc.close()
    om = rb.Model(str(path))
    recs = [rb.records(om, lay.as_oracle_dict(), DUAL_UR5_EE, qpos[b], qvel[b]) for b in range(B)]
    R = {k: np.array([r[k] for r in recs]) for k in ("M", "J", "dq", "bias", "ee_pose")}
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], g["tgt_pose"])
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(R["J"][b], R["M"][b])[2:]) for b in range(B)])
    assert dom.sum() >= B // 2 and rel_err(u, ref)[dom].max() <= TOL64
    # and the shipped model, same states: the structural walk, another answer (the perturbation matters)
    osc = BatchedOSC(lay, B, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(base)
    assert "compact_dual_ur5_s +" in osc.from_q_name
    u0 = osc.step_from_q(qpos, qvel, g["tgt_pose"])
    osc.close()
    assert np.abs(u0 - u).max() > 1e-3


@pytest.mark.parametrize("B", [1, 3, 63, 64, 65, 130, 515])
def test_fused_from_q_ragged_batches_bit_exact(B):
    """A walk wave carries 64 robots, a row16 block 4, and the block -> robots map groups 128 blocks per 8 walk waves: batch
    sizes around all three.  Robot b comes out bit-identical whatever the batch around it."""
    lay, gains, g, model, osc, states = _from_q_setup("k13", 640, np.float64, seed=31, singular_every=5)
    full, ffull = osc.step_q(return_flags=True)
    qpos, qvel = states[0]
    osc.upload_q(qpos[:B], qvel[:B])
    osc.set_targets(g["tgt_pose"][:B])
    part, fpart = osc.step_q(return_flags=True)
    osc.close()
    assert np.array_equal(part, full[:B]) and np.array_equal(fpart, ffull[:B])


@pytest.mark.parametrize("iters", [1, 7, 8, 12, 19])
def test_fused_resident_trains_equal_single_steps(iters):
    """irlosc_step_resident_from_q chains up to 8 steps per launch pair (walk train, OSC train, one give-up pass), each
    step with its own exchange buffer and output set: the outputs left behind are bit for bit those of a single fused
    step on the last slot visited -- also right after an uneven train (the counters of the give-up lists)."""
    nslots, B = 3, 700
    lay, gains, g, model, osc, states = _from_q_setup("k13", B, np.float64, seed=41, n_slots=nslots, singular_every=6)
    for rep in range(2):
        first = (1 + rep) % nslots
        osc.step_resident_from_q(iters, first_slot=first)
        u_t, f_t = osc.download(B)
        u_1, f_1 = osc.step_q(slot=(first + iters - 1) % nslots, return_flags=True)
        assert np.array_equal(u_t, u_1) and np.array_equal(f_t, f_1), rep
    osc.close()


def test_fused_path_turned_on_after_the_coordinates_were_uploaded(monkeypatch):
    """Coordinates uploaded while the fused path was off have no copy in the fused walk's layout yet.  The irlosc_set_model that turns
    the path on lays them out on the main stream before it returns, so the trains of another bank's stream never read a layout still
    being written: 19 steps over three banks, bit for bit a single fused step on the last slot visited."""
    nslots, B, iters = 3, 700, 19
    monkeypatch.setenv("IRLOSC_FUSED", "0")
    lay, gains, g, model, osc, states = _from_q_setup("k13", B, np.float64, seed=43, n_slots=nslots, singular_every=6)
    assert "through dense records" in osc.from_q_name
    monkeypatch.delenv("IRLOSC_FUSED")
    osc.set_model(model)
    assert "fused" in osc.from_q_name
    osc.step_resident_from_q(iters)
    u_t, f_t = osc.download(B)
    u_1, f_1 = osc.step_q(slot=(iters - 1) % nslots, return_flags=True)
    osc.close()
    assert np.array_equal(u_t, u_1) and np.array_equal(f_t, f_1)


@pytest.mark.parametrize("fe", ["lane", "generic"])
@pytest.mark.parametrize("B", [1, 70, 128])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_frontend_records_themselves(fe, B, dtype, monkeypatch):
    """Both front-end kernels (lane-per-instance with the Dual-UR5 tree compiled in; generic wave-per-instance), ragged
    and full waves: every record the front end writes (M, J, dq, bias, ee_pose) against the rigid-body oracle, element
    by element, over a slot that held garbage before (the records are written dense: structural zeros included)."""
    from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
    from oracle import rigid_body as rb
    monkeypatch.setenv("IRLOSC_FRONTEND", fe)
    lay = synth.make_layout("k13")
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(23 + B)
    qpos, qvel = model.random_state(rng, B)
    qpos[0, :] *= 40.0                                    # many turns: the argument reduction of the inline sin / cos
    om = rb.Model()
    recs = [rb.records(om, lay.as_oracle_dict(), DUAL_UR5_EE, qpos[b], qvel[b]) for b in range(B)]
    R = {k: np.array([r[k] for r in recs]) for k in ("M", "J", "dq", "bias", "ee_pose")}
    osc = BatchedOSC(lay, B, dtype=dtype)
    assert osc.frontend_name == ""
    osc.set_model(model)
    assert ("_lane_" in osc.frontend_name) == (fe == "lane") and ("_generic_" in osc.frontend_name) == (fe == "generic")
    junk = {k: rng.normal(size=v.shape) * 7.0 + 3.0 for k, v in R.items()}
    junk["M"] = junk["M"] + junk["M"].transpose(0, 2, 1)
    junk["ee_pose"][:, :, 3:] = [1.0, 0.0, 0.0, 0.0]
    osc.upload(junk["M"], junk["J"], junk["dq"], junk["bias"], junk["ee_pose"])
    osc.upload_q(qpos, qvel)
    osc.frontend()
    got = osc.download_records()
    osc.close()
    tol = 1e-10 if dtype == np.float64 else 2e-6
    for k in ("M", "J", "dq", "bias", "ee_pose"):
        want = R[k]
        scale = np.abs(want).reshape(B, -1).max(axis=1).reshape((B,) + (1,) * (want.ndim - 1)) + 1e-300
        err = np.abs(np.asarray(got[k], dtype=np.float64) - want) / scale
        assert err.max() <= tol, (k, float(err.max()))
    # structural zeros are exact zeros: M[i][j] unless one hinge is above the other, J columns of hinges that do not move the EE
    jb = om.joint_body
    rel = np.array([[om.anc[jb[j], i] or om.anc[jb[i], j] for j in range(om.nj)] for i in range(om.nj)])
    assert np.all(np.asarray(got["M"])[:, ~rel] == 0)
    row = 0
    for name, mask in zip(lay.dev_names, lay.ctrlr_dof):
        moves = om.anc[om.body_id(DUAL_UR5_EE[name])]
        for _ in range(int(np.sum(mask))):
            assert np.all(np.asarray(got["J"])[:, row, ~moves] == 0)
            row += 1


def test_second_tree_through_the_generic_front_end():
    """"Any tree of hinges" on something that is not the Dual-UR5: the single arm of scenes/ur5.xml (models/ur5.json: a chain
    of six on a world-fixed base, one device, k = 6).  It has no compiled shape, so irlosc_set_model picks the wave-per-robot
    front end and the OSC step runs on the generic kernel: records against the rigid-body oracle element by element, torques
    of step_from_q against the OSC oracle on those records."""
    from irl_control_amd.rigid_body import RigidBodyModel
    from oracle import rigid_body as rb
    import os
    B = 70
    model = RigidBodyModel.load("ur5")
    om = rb.Model(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "irl_control_amd", "models", "ur5.json"))
    lay = OSCLayout(n=6, dev_names=["arm"], ctrlr_dof=[[True] * 6], joint_ids=[list(range(6))], j_idx0=[0])
    rng = np.random.default_rng(77)
    qpos, qvel = rng.uniform(-np.pi, np.pi, (B, 6)), rng.normal(0.0, 0.5, (B, 6))
    recs = [rb.records(om, lay.as_oracle_dict(), {"arm": "EE"}, qpos[b], qvel[b]) for b in range(B)]
    R = {k: np.array([r[k] for r in recs]) for k in ("M", "J", "dq", "bias", "ee_pose")}
    gains = dict(kp=[200.0], kv=[50.0], ko=[200.0], k=[[1.0, 2.0, 3.0]], d=[[0.5, 1.0, 1.0]], max_vel=[[1.0, 5.0]], null_kv=10.0)
    tgt = R["ee_pose"].copy()
    tgt[:, :, :3] += rng.normal(0.0, 0.2, size=tgt[:, :, :3].shape)
    for dtype, tol in ((np.float64, 1e-10), (np.float32, 2e-6)):
        osc = BatchedOSC(lay, B, dtype=dtype)
        assert "generic" in osc.kernel_name
        osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
        osc.set_model(model, ee_bodies=["EE"])
        assert "_generic_" in osc.frontend_name and "through dense records" in osc.from_q_name
        u = osc.step_from_q(qpos, qvel, tgt)
        got = osc.download_records()
        osc.close()
        for k in ("M", "J", "dq", "bias", "ee_pose"):
            scale = np.abs(R[k]).reshape(B, -1).max(axis=1).reshape((B,) + (1,) * (R[k].ndim - 1)) + 1e-300
            assert (np.abs(np.asarray(got[k], dtype=np.float64) - R[k]) / scale).max() <= tol, k
        if dtype == np.float64:
            ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], tgt)
            dom = np.array([in_parity_domain(*osc_oracle.task_inertia(R["J"][b], R["M"][b])[2:]) for b in range(B)])
            assert dom.sum() >= B // 2 and rel_err(u.astype(np.float64), ref)[dom].max() <= TOL64


def test_frontend_is_deterministic_and_independent_of_batch_mates():
    """The lane-per-robot front end stages its output through LDS without s_waitcnt between a wave's own writes and
    reads (in-order LDS) and parks its entries in a side buffer shared by all launches of a context: the same robots
    give the same bits launch after launch, in another slot, and whatever else is in the batch."""
    from irl_control_amd.rigid_body import RigidBodyModel
    lay = synth.make_layout("k13")
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(99)
    B = 1000
    qpos, qvel = model.random_state(rng, B)
    osc = BatchedOSC(lay, B, dtype=np.float64, n_slots=2)
    osc.set_model(model)
    assert "_lane_" in osc.frontend_name
    osc.upload_q(qpos, qvel, slot=0)
    osc.frontend(slot=0)
    first = osc.download_records(slot=0)
    for rep in range(20):
        osc.upload_q(qpos[::-1].copy(), qvel[::-1].copy(), slot=1)       # other work through the same side buffer
        osc.frontend(slot=1)
        osc.frontend(slot=0)
        again = osc.download_records(slot=0)
        for k in ("M", "J", "dq", "bias", "ee_pose"):
            assert np.array_equal(first[k], again[k]), (rep, k)
    rev = osc.download_records(slot=1)
    for k in ("M", "J", "dq", "bias", "ee_pose"):
        assert np.array_equal(first[k], rev[k][::-1]), k                   # robot b's records do not depend on its lane or wave
    osc.close()
    small = BatchedOSC(lay, 37, dtype=np.float64)
    small.set_model(model)
    small.upload_q(qpos[500:537], qvel[500:537])
    small.frontend()
    sub = small.download_records()
    small.close()
    for k in ("M", "J", "dq", "bias", "ee_pose"):
        assert np.array_equal(first[k][500:537], sub[k]), k


def test_frontend_needs_a_model_and_coordinates():
    lay, gains, g = synth.make_batch("k13", 8, seed=1)
    osc = BatchedOSC(lay, 8, dtype=np.float64)
    with pytest.raises(_lib.IrloscError, match="irlosc_set_model"):
        osc.upload_q(np.zeros((8, 25)), np.zeros((8, 25)))
    from irl_control_amd.rigid_body import RigidBodyModel
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    with pytest.raises(_lib.IrloscError, match="irlosc_upload_q"):
        osc.frontend()
    osc.close()


def test_a_refused_model_leaves_the_model_in_force_whole():
    """An irlosc_set_model refused with IRLOSC_ERR_ARG -- here ee_body out of range, found after the whole model was validated and
    its tables derived -- changes nothing: the steps from joint coordinates keep their form and name, a slot's records keep their
    route (the resident lane route: its compact block and the pack table stay), the F/T description and the slot's sensor feed stay,
    and a step computes the same bits."""
    import ctypes as C
    from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
    B = 4096
    lay, gains, g = synth.make_batch("k12_admit", B, seed=71)
    model = RigidBodyModel.load("dual_ur5")
    osc = BatchedOSC(lay, B, dtype=np.float64, n_slots=2)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    osc.set_ft_sensors()
    rng = np.random.default_rng(72)
    qpos, qvel = model.random_state(rng, B)
    for sl in range(2):                  # the same robots in both slots; slot 0 with a sensor feed, slot 1 with records
        osc.upload_q(qpos, qvel, slot=sl)
        osc.set_targets(g["tgt_pose"], slot=sl)
    osc.set_sensordata(rng.normal(0.0, 5.0, size=(B, 18)), slot=0)
    osc.frontend(slot=1)

    def observed():
        u, fl = osc.step_q(slot=0, return_flags=True)
        return osc.from_q_name, osc.slot_route(1), u, fl

    name0, route0, u0, fl0 = observed()
    assert "fused" in name0 and route0 == "lane"
    u_plain = osc.step_q(slot=1)
    osc.frontend(slot=1)                 # (the fused step took slot 1's records: here they are again)
    assert not np.array_equal(u_plain, u0)      # slot 0's feed is felt: losing it would show
    st = model.to_struct([DUAL_UR5_EE[d] for d in lay.dev_names])
    st.ee_body[lay.ndev - 1] = model.nb
    assert osc.lib.irlosc_set_model(osc._h, C.byref(st)) == -1      # IRLOSC_ERR_ARG
    assert b"ee_body" in osc.lib.irlosc_last_error(osc._h)
    name1, route1, u1, fl1 = observed()
    osc.close()
    assert name1 == name0 and route1 == route0
    assert np.array_equal(u1, u0) and np.array_equal(fl1, fl0)


def test_step_refuses_more_instances_than_the_slot_holds():
    """state, targets and step sizes are tied together: stepping over more instances than were uploaded (or
    targeted) is IRLOSC_ERR_STATE instead of a silent pass over stale HBM; an asymmetric M is refused on request."""
    lay, gains, g = synth.make_batch("k13", 32, seed=2)
    osc = BatchedOSC(lay, 64, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload(g["M"][:16], g["J"][:16], g["dq"][:16], g["bias"][:16], g["ee_pose"][:16])
    with pytest.raises(ValueError, match="holds 16"):
        osc.set_targets(g["tgt_pose"][:8])
    osc.set_targets(g["tgt_pose"][:16])
    u = np.empty((32, 25)); fl = np.empty(32, dtype=np.uint32)
    rc = osc.lib.irlosc_step(osc._h, 0, 32, _lib.ptr(u), _lib.ptr(fl))
    assert rc == -3 and b"holds state for 16" in osc.lib.irlosc_last_error(osc._h)
    assert osc.lib.irlosc_step(osc._h, 0, 16, _lib.ptr(u), _lib.ptr(fl)) == 0
    Masym = g["M"][:4].copy()
    Masym[2, 3, 7] += 1.0
    with pytest.raises(ValueError, match="instance 2 is not symmetric"):
        osc.upload(Masym, g["J"][:4], g["dq"][:4], g["bias"][:4], g["ee_pose"][:4], check_symmetric=True)
    osc.close()


@pytest.mark.parametrize("dtype,kernel", [(np.float64, _lib.KERNEL_AUTO), (np.float32, _lib.KERNEL_AUTO)])
def test_library_refuses_an_asymmetric_M_on_the_throughput_paths(dtype, kernel):
    """The throughput kernels read row j of M as column j; the reference uses M as given (osc.py:49,151).  Records that
    come from the host are probed ON THE DEVICE (irlosc_upload, irlosc_tick): an asymmetric M is IRLOSC_ERR_ARG naming the
    instance, the slot then holds nothing -- no records, and neither the tree verdict nor the route of the records the refused
    ones overwrote -- and the generic kernel still takes such an M as it is."""
    B = 300
    lay, gains, g = synth.make_batch("k13", B, seed=4, dtype=dtype)
    osc = BatchedOSC(lay, B, dtype=dtype, kernel=kernel)
    assert "generic" not in osc.kernel_name
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"])                     # symmetric: accepted
    Masym = g["M"].copy()
    Masym[257, 3, 7] *= 1.01
    Masym[123, 20, 2] += 0.5
    with pytest.raises(_lib.IrloscError, match=r"M of instance 123 is not symmetric \(2 instance"):
        osc.upload(Masym, g["J"], g["dq"], g["bias"], g["ee_pose"])
    osc.set_targets(g["tgt_pose"])
    with pytest.raises(_lib.IrloscError, match="must precede a step"):                 # the refused upload left the slot empty
        osc.step()
    with pytest.raises(_lib.IrloscError, match="M of instance 123 is not symmetric"):
        osc.tick(Masym, g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"])
    u = osc.tick(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"])      # and the context is still usable
    assert np.all(np.isfinite(u))
    sl = slice(120, 126)                              # small batches are checked on the host, on the caller's array (no kernel)
    with pytest.raises(_lib.IrloscError, match=r"M of instance 3 is not symmetric \(max"):
        osc.tick(Masym[sl], g["J"][sl], g["dq"][sl], g["bias"][sl], g["ee_pose"][sl], g["tgt_pose"][sl])
    with pytest.raises(_lib.IrloscError, match="M of instance 3 is not symmetric"):
        osc.upload(Masym[sl], g["J"][sl], g["dq"][sl], g["bias"][sl], g["ee_pose"][sl])
    u6 = osc.tick(g["M"][sl], g["J"][sl], g["dq"][sl], g["bias"][sl], g["ee_pose"][sl], g["tgt_pose"][sl])
    assert np.array_equal(u6, u[sl])
    assert np.all(np.isfinite(u6))
    # tree-form records (the front end's: synthetic ones do not carry the tree's zeros) accepted with their verdict, then refused ones
    # written over them: the verdict and the route went with the records
    assert not osc.slot_structure(0)
    fe = _from_q_setup("k13", B, dtype, seed=4)[4]
    fe.frontend()
    rec = fe.download_records(0)
    fe.close()
    osc.upload(rec["M"], rec["J"], rec["dq"], rec["bias"], rec["ee_pose"])
    assert osc.slot_structure(0) and osc.slot_route(0) == "row16_tree"
    Mtree = rec["M"].copy()
    Mtree[123, 20, 2] += 0.5
    with pytest.raises(_lib.IrloscError, match="M of instance 123 is not symmetric"):
        osc.upload(Mtree, rec["J"], rec["dq"], rec["bias"], rec["ee_pose"])
    assert not osc.slot_structure(0)
    assert osc.slot_route(0) not in ("row16_tree", "lane")
    with pytest.raises(_lib.IrloscError, match="must precede a step"):
        osc.step()
    osc.close()
    gen = BatchedOSC(lay, B, dtype=dtype, kernel=_lib.KERNEL_GENERIC)
    gen.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    gen.upload(Masym, g["J"], g["dq"], g["bias"], g["ee_pose"])                        # M as given, like the reference
    gen.close()


def test_force_test_loop_matches_reference_tick_by_tick():
    """examples/force_test.py:57-127 headless (osc1 gains, admittance, left arm along a line of waypoints at 1 cm,
    F/T force read back after every step): forces of all 240 ticks, the waypoint indices and the logged sensor force."""
    g, meta = _load_loop_golden("loop_force_test")
    mod = _load_example("force_test_headless")
    rec = mod.run(ticks=meta["ticks"], seed=meta["seed"], verbose=False)
    assert rec["idxs"] == meta["idxs"]
    assert np.array_equal(rec["wp"], g["wp"]) and g["wp"][:, 1].max() >= 2
    assert np.array_equal(rec["ft"], g["ft"])
    err = np.abs(rec["forces"] - g["forces"]).max(axis=1) / np.abs(g["forces"]).max(axis=1)
    assert err.max() <= TOL64, float(err.max())


def test_insertion_action_sequence_matches_reference_tick_by_tick():
    """examples/insertion_task.py:146-318 headless: the eight WP actions of the insertion sequence (object-relative
    waypoints, error-adaptive max_vel) run by ActionSequenceRunner with OSC.generate on the HIP path, against the golden
    the REFERENCE's own InsertionTask methods produced on the same FakeSim: same number of ticks, same velocity limit
    and same ctrl vector on every tick."""
    g, meta = _load_loop_golden("loop_insertion_wp")
    mod = _load_example("insertion_task_headless")
    rec = mod.run(seed=meta["seed"], active_arm=meta["active_arm"], objects=meta["objects"], rate=meta["rate"], verbose=False)
    assert rec["ticks"] == meta["ticks"] == len(g["ctrl"]) and rec["n_actions"] == meta["n_wp"]
    assert np.allclose(rec["max_vel"], g["max_vel"], rtol=1e-9, atol=0)
    err = np.abs(rec["ctrl"] - g["ctrl"]).max(axis=1) / np.abs(g["ctrl"]).max(axis=1)
    assert err.max() <= TOL64, float(err.max())


def test_insertion_sequence_with_grip_actions_matches_reference_tick_by_tick():
    """The WHOLE insertion action list, GRIP entries included (insertion_task.py:190-205).  The reference times a GRIP with a
    wall-clock thread; the golden was minted with that thread replaced by a tick budget of gripper_duration / tick_seconds
    ticks around the reference's own loop body (oracle/make_golden.py), which is what ActionSequenceRunner.grip runs."""
    g, meta = _load_loop_golden("loop_insertion_full")
    assert meta["with_grip"] and meta["n_actions"] == 12
    mod = _load_example("insertion_task_headless")
    rec = mod.run(seed=meta["seed"], active_arm=meta["active_arm"], objects=meta["objects"], rate=meta["rate"], verbose=False,
                  with_grip=True, tick_seconds=meta["tick_seconds"])
    assert rec["ticks"] == meta["ticks"] == len(g["ctrl"]) and rec["n_actions"] == meta["n_actions"]
    assert np.allclose(rec["max_vel"], g["max_vel"], rtol=1e-9, atol=0)
    err = np.abs(rec["ctrl"] - g["ctrl"]).max(axis=1) / np.abs(g["ctrl"]).max(axis=1)
    assert err.max() <= TOL64, float(err.max())
    grip = np.abs(g["ctrl"][:, 7] - (-0.08)) < 1e-15           # the first GRIP's gripper force is on the right gripper's actuator
    assert grip.sum() >= 25


def test_tick_latency_b1_is_bounded():
    """The B = 1 drop-in path costs one library call and one synchronisation per tick (50 us
    median on the row16 kernel); bound it generously so that a regression to several round trips shows."""
    import time
    lay, gains, g = synth.make_batch("k13", 16, seed=1)
    osc = BatchedOSC(lay, 1, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    a = [g[k][:1] for k in ("M", "J", "dq", "bias", "ee_pose", "tgt_pose")]
    for _ in range(50):
        osc.tick(*a)
    t = []
    for _ in range(200):
        t0 = time.perf_counter(); osc.tick(*a); t.append(time.perf_counter() - t0)
    osc.close()
    assert np.median(t) < 250e-6, float(np.median(t))


def test_closed_loop_converges_on_targets():
    """examples/closed_loop_headless.py: 12 robots, the front end as the physics (M, bias read back from HBM, host-side
    integration of M qacc = u - bias), the HIP controller in the loop for 2 000 ticks.  The end effectors must converge
    onto their Cartesian targets: this closes the sign conventions of controller and front end against each other
    (bias compensation, J^T Mx direction, null-space damping), which no open-loop parity test does."""
    mod = _load_example("closed_loop_headless")
    r = mod.run(robots=12, ticks=2000, seed=0, verbose=False)
    assert np.all(np.isfinite(r["q"])) and np.all(np.isfinite(r["err"]))
    worst = r["err"].max(axis=1)                      # per robot: the worse of its two arms
    assert r["err0"].max(axis=1).min() > 0.02         # every robot started away from its targets
    assert (worst < 5e-3).mean() >= 0.75, np.sort(worst)
    assert np.median(worst) < 1e-3


@pytest.mark.gpu
def test_fleet_action_sequence_lockstep_equals_solo_runs():
    """f4 batched over randomised object poses (examples/insertion_fleet_headless.py): every robot of a fleet walks the
    WP / GRIP list to its end, and a robot's torque trajectory inside the fleet is the one it produces alone, bit for
    bit (instances share nothing but the launch)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("insertion_fleet_headless",
                                                  os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                               "examples", "insertion_fleet_headless.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fleet = mod.run(robots=6, max_ticks=14000, verbose=False, sequence=mod.SHORT_SEQUENCE)
    assert fleet["done"].all(), (fleet["action"], fleet["ticks"])
    assert np.isfinite(fleet["u"]).all()
    for b in (0, 4):
        solo = mod.run(robots=6, max_ticks=600, verbose=False, sequence=mod.SHORT_SEQUENCE, only=[b])
        n = solo["u"].shape[0]
        assert n == 600
        assert np.array_equal(solo["u"][:, 0], fleet["u"][:n, b])


# ---- tree-structured factorisation on DENSE records (irlosc_slot_structure) ------------------------------------------------
def _physical_records(cfg, B, dtype, seed, singular_every=7):
    """Dense records of random robot states as the front end writes them (+ the setup's targets and gains)."""
    lay, gains, g, model, osc, states = _from_q_setup(cfg, B, dtype, seed=seed, singular_every=singular_every)
    osc.frontend()
    assert osc.slot_structure(0)                          # the lane kernel's records: tree form by construction
    rec = osc.download_records(0)
    u, fl = osc.step(return_flags=True)
    osc.close()
    if lay.admittance:
        rec["wrench"] = g["wrench"]
    return lay, gains, g, rec, u, fl


def _run_uploaded(lay, gains, g, rec, dtype, n_slots=1):
    B = rec["M"].shape[0]
    osc = BatchedOSC(lay, B, dtype=dtype, n_slots=n_slots, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload(rec["M"], rec["J"], rec["dq"], rec["bias"], rec["ee_pose"], rec.get("wrench"))
    osc.set_targets(g["tgt_pose"][:B], g.get("tgt_vel"))
    st = osc.slot_structure(0)
    u, fl = osc.step(return_flags=True)
    osc.close()
    return st, u, fl


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfg", ["k13", "k7", "k12_admit"])
def test_tree_form_on_dense_records_equals_the_dense_recursion_and_the_oracle(cfg, dtype, monkeypatch):
    """Records of physical robot states carry the zeros of the kinematic tree (what mj_fullM / mj_jacBody leave,
    robot.py:68-72, device.py:115-133).  Uploaded, they are probed and the row16 kernel factors M in the tree-structured
    form; the same records with IRLOSC_TREE=0 go through the dense recursion.  Same flags, torques equal to rounding, both
    within north_star's 1e-5 of the float64 oracle on the same records."""
    B = 1024 + 13
    lay, gains, g, rec, u_fe, fl_fe = _physical_records(cfg, B, dtype, seed=41)
    st_t, u_t, fl_t = _run_uploaded(lay, gains, g, rec, dtype)
    assert st_t                                             # the probe accepted the uploaded records
    if not lay.admittance:                                  # (the front end's slot had no wrench yet)
        assert np.array_equal(u_t, u_fe) and np.array_equal(fl_t, fl_fe)      # same kernel as on the front end's own records
    monkeypatch.setenv("IRLOSC_TREE", "0")
    st_d, u_d, fl_d = _run_uploaded(lay, gains, g, rec, dtype)
    assert not st_d
    d = rel_err(u_t, u_d.astype(np.float64))
    assert np.array_equal(fl_t, fl_d)
    assert d.max() <= (1e-8 if dtype == np.float64 else 5e-7), float(d.max())      # float32 records: the outputs are rounded to float32
    if cfg != "k7":
        assert (fl_t & _lib.FLAG_EIGEN_PATH).mean() > 0.02
    r = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    n = 256
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, r["M"][:n], r["J"][:n], r["dq"][:n], r["bias"][:n], r["ee_pose"][:n],
                                    np.asarray(g["tgt_pose"][:n], dtype=np.float64), r["wrench"][:n] if "wrench" in r else None)
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(r["J"][b], r["M"][b])[2:]) for b in range(n)])
    assert dom.sum() >= n // 2
    assert rel_err(u_t[:n], ref)[dom].max() <= TOL64 and rel_err(u_d[:n], ref)[dom].max() <= TOL64


def test_structure_probe_refuses_what_does_not_carry_the_tree_zeros():
    """irlosc_slot_structure: the verdict is per slot and exact -- one non-zero where the tree has no coupling (between the
    two arms in M; a gripper column of J), a batch under 64 instances, records of unknown origin (synthetic dense M): dense
    recursion, and the answer is the dense recursion's bit for bit."""
    B = 256
    lay, gains, g, rec, _, _ = _physical_records("k13", B, np.float64, seed=43)
    st, u_ok, fl_ok = _run_uploaded(lay, gains, g, rec, np.float64)
    assert st
    bad = {k: v.copy() for k, v in rec.items()}
    bad["M"][5, 3, 20] = bad["M"][5, 20, 3] = 1e-9          # right arm <-> left arm
    st_m, u_m, _ = _run_uploaded(lay, gains, g, bad, np.float64)
    assert not st_m and np.all(np.isfinite(u_m))
    bad = {k: v.copy() for k, v in rec.items()}
    bad["J"][7, 0, 9] = 1e-12                               # a gripper hinge moving an end effector
    st_j, u_j, _ = _run_uploaded(lay, gains, g, bad, np.float64)
    assert not st_j
    small = {k: v[:63] for k, v in rec.items()}
    st_s, u_s, fl_s = _run_uploaded(lay, gains, g, small, np.float64)
    assert not st_s
    assert rel_err(u_s, u_ok[:63]).max() <= 1e-8 and np.array_equal(fl_s, fl_ok[:63])
    _, gains2, a = synth.make_batch("k13", B, seed=3, dtype=np.float64)
    st_x, _, _ = _run_uploaded(lay, gains2, a, a, np.float64)
    assert not st_x


def test_trains_mixing_tree_and_dense_slots_keep_each_slots_own_form():
    """One kernel per launch: a train of irlosc_step_resident whose slots do not all qualify for the tree form is issued as two
    sub-trains (tree kernel for the qualifying steps, dense recursion for the others) -- round 3 dropped the whole train to the
    dense recursion.  Two slots, one of them with synthetic dense records: every slot's result equals its own single step bit
    for bit, whatever the train."""
    B = 512
    lay, gains, g, rec, _, _ = _physical_records("k13", B, np.float64, seed=47)
    _, _, a = synth.make_batch("k13", B, seed=9, dtype=np.float64)
    osc = BatchedOSC(lay, B, dtype=np.float64, n_slots=2, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload(rec["M"], rec["J"], rec["dq"], rec["bias"], rec["ee_pose"], slot=0)
    osc.upload(a["M"], a["J"], a["dq"], a["bias"], a["ee_pose"], slot=1)
    osc.set_targets(g["tgt_pose"][:B], slot=0)
    osc.set_targets(a["tgt_pose"], slot=1)
    assert osc.slot_structure(0) and not osc.slot_structure(1)
    u0_tree, f0 = osc.step(slot=0, return_flags=True)
    u1, f1 = osc.step(slot=1, return_flags=True)
    for iters, last in ((2, 1), (3, 0), (8, 1), (13, 0)):      # trains {0,1}, {0,1,0}, a full train, a full train + a short one
        osc.step_resident(iters, first_slot=0)
        u_last, f_last = osc.download(B)
        assert np.array_equal(u_last, u0_tree if last == 0 else u1) and np.array_equal(f_last, f0 if last == 0 else f1), iters
    osc.close()


def test_raw_state_paths_qualify_for_the_tree_form():
    """Raw simulator arrays of physical states (what mj_fullM / mj_jacBody leave) through the two assembly paths: the
    host-staged irlosc_upload_raw probes by itself; irlosc_assemble_device on device-resident arrays cannot (caller's stream)
    and gets its verdict from irlosc_probe_structure.  Either way the step equals the one on the plainly uploaded records."""
    import ctypes as C
    hb = HipBuffers()
    B = 320
    lay, gains, g, rec, u_rec, fl_rec = _physical_records("k13", B, np.float64, seed=53)
    nv, ns = 25, 18
    d = _lib.RawDesc()
    d.nv, d.n_sensor = nv, ns
    for p_ in range(32):
        d.joint_ids[p_] = p_ if p_ < 25 else 0
        d.dq_src[p_] = p_ if p_ < 25 else -1
    for i in range(4):
        d.ft_force0[i], d.ft_torque0[i] = -1, -1
    # records -> raw: k13 stacks ur5right (6 rows), ur5left (6 rows), base (yaw row = third rotational row)
    jacp, jacr = np.zeros((B, 3, 3, nv)), np.zeros((B, 3, 3, nv))
    jacp[:, 0], jacr[:, 0] = rec["J"][:, 0:3], rec["J"][:, 3:6]
    jacp[:, 1], jacr[:, 1] = rec["J"][:, 6:9], rec["J"][:, 9:12]
    jacr[:, 2, 2] = rec["J"][:, 12]
    arr = dict(qM=rec["M"], qvel=rec["dq"], qfrc_bias=rec["bias"], jacp=jacp, jacr=jacr, ee_xpos=np.ascontiguousarray(rec["ee_pose"][:, :, :3]),
               ee_xquat=np.ascontiguousarray(rec["ee_pose"][:, :, 3:]), site_xmat=np.tile(np.eye(3).reshape(9), (B, 3, 1)),
               sensordata=np.zeros((B, ns)))
    osc = BatchedOSC(lay, B, dtype=np.float64, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload_raw(d, **arr)
    osc.set_targets(g["tgt_pose"])
    assert osc.slot_structure(0)                              # probed by the upload itself
    u_raw, fl_raw = osc.step(return_flags=True)
    assert np.array_equal(u_raw, u_rec) and np.array_equal(fl_raw, fl_rec)
    dev = {k: hb.to_device(v) for k, v in arr.items()}
    pp = lambda t: t
    rc = osc.lib.irlosc_assemble_device(osc._h, 0, B, C.byref(d), pp(dev["qM"]), pp(dev["qvel"]), pp(dev["qfrc_bias"]),
                                        pp(dev["jacp"]), pp(dev["jacr"]), pp(dev["ee_xpos"]), pp(dev["ee_xquat"]),
                                        pp(dev["site_xmat"]), pp(dev["sensordata"]), None)
    assert rc == 0, osc.lib.irlosc_last_error(osc._h)
    assert not osc.slot_structure(0)                          # nobody has looked yet: dense recursion
    u_dense = osc.step()
    assert rel_err(u_dense, u_rec.astype(np.float64)).max() <= 1e-8
    assert osc.probe_structure(0) and osc.slot_structure(0)
    u_dev, fl_dev = osc.step(return_flags=True)
    assert np.array_equal(u_dev, u_rec) and np.array_equal(fl_dev, fl_rec)
    with pytest.raises(_lib.IrloscError):
        osc.probe_structure(0, B + 1)
    osc.close()
    hb.free()


# ---- round 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_in_one_robots_M_is_that_robots_business(dtype):
    """A diverged robot (NaN / Inf in its M) is not "asymmetric": upload and tick accept the batch, that robot is reported through
    its own flags (IRLOSC_FLAG_NONFINITE / M_NOT_PD), and every other robot gets exactly the torques it gets without it -- the
    reference simply propagates that robot's NaN (osc.py:49).  Large batch (device-side probe) and small batch (host check)."""
    B = 300
    lay, gains, g = synth.make_batch("k13", B, seed=14, dtype=dtype)
    osc = BatchedOSC(lay, B, dtype=dtype)
    assert "row16" in osc.kernel_name
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    clean, fclean = osc.generate_batched(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"], return_flags=True)
    M = g["M"].copy()
    M[77, 4, 4] = np.nan
    M[200, 3, 9] = M[200, 9, 3] = np.inf
    M[250, 5, 11] = np.nan                                   # one side only: still not a finite pair
    sick = np.array([77, 200, 250])
    ok = np.setdiff1d(np.arange(B), sick)
    u, fl = osc.generate_batched(M, g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"], return_flags=True)
    assert np.all(fl[sick] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    assert np.array_equal(u[ok], clean[ok]) and np.array_equal(fl[ok], fclean[ok])
    ut, ft = osc.tick(M, g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"], return_flags=True)
    assert np.array_equal(ut[ok], clean[ok]) and np.all(ft[sick] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    sl = slice(70, 90)                                       # 20 robots: the host-side check
    us, fs = osc.tick(M[sl], g["J"][sl], g["dq"][sl], g["bias"][sl], g["ee_pose"][sl], g["tgt_pose"][sl], return_flags=True)
    keep = np.arange(70, 90) != 77
    assert np.array_equal(us[keep], clean[sl][keep]) and (fs[7] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    Masym = M.copy()
    Masym[10, 2, 6] += 0.25                                  # a FINITE asymmetry is still refused
    with pytest.raises(_lib.IrloscError, match="M of instance 10 is not symmetric"):
        osc.upload(Masym, g["J"], g["dq"], g["bias"], g["ee_pose"])
    osc.close()


@pytest.mark.parametrize("where", ["upper", "lower"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_one_sided_nan_in_M_is_flagged(bad, where):
    """M[i][j] non-finite with M[j][i] finite.  The symmetry probe judges finite pairs only, so the batch is accepted;
    the throughput kernels read row j of M as its column j and use EVERY entry of the row for M dq (osc.py:151), so whichever
    triangle holds the bad entry it reaches that robot's torques: NONFINITE (or M_NOT_PD) for that robot, nobody else touched --
    on synthetic dense records (dense recursion) and on physical records (tree form: the entry sits inside the tree's pattern)."""
    B = 256
    lay, gains, g = synth.make_batch("k13", B, seed=15)
    _, _, gp, rec, _, _ = _physical_records("k13", B, np.float64, seed=16, singular_every=0)
    for tag, M, rest, tgt in (("dense", g["M"], g, g["tgt_pose"]), ("tree", rec["M"], rec, gp["tgt_pose"])):
        osc = BatchedOSC(lay, B, dtype=np.float64)
        osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
        clean, fclean = osc.generate_batched(M, rest["J"], rest["dq"], rest["bias"], rest["ee_pose"], tgt, return_flags=True)
        assert osc.slot_structure(0) == (tag == "tree")
        Mb = M.copy()
        i, j = (2, 5) if where == "upper" else (5, 2)          # hinges 2 and 5 of the right arm: a structural non-zero of the tree
        assert Mb[100, i, j] != 0.0
        Mb[100, i, j] = bad
        u, fl = osc.generate_batched(Mb, rest["J"], rest["dq"], rest["bias"], rest["ee_pose"], tgt, return_flags=True)
        assert osc.slot_structure(0) == (tag == "tree")
        osc.close()
        ok = np.arange(B) != 100
        assert fl[100] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD), (tag, hex(int(fl[100])))
        assert not np.all(np.isfinite(u[100]))
        assert np.array_equal(u[ok], clean[ok]) and np.array_equal(fl[ok], fclean[ok])


def test_a_fused_step_leaves_no_records_in_the_slot():
    """irlosc_step_from_q on the fused path writes dense records only for the robots its give-up pass recomputes: afterwards the
    slot holds no records (IRLOSC_ERR_STATE from step / step_resident / download_records, no tree verdict) until the front end
    or an upload fills it again; joint coordinates and targets stay."""
    lay, gains, g, model, osc, states = _from_q_setup("k13", 256, np.float64, seed=77)
    assert "fused" in osc.from_q_name
    osc.frontend()
    assert osc.slot_structure(0)
    u_rec = osc.step()
    osc.download_records(0)
    u_fused = osc.step_q()
    assert rel_err(u_fused, u_rec.astype(np.float64)).max() <= 1e-9
    assert not osc.slot_structure(0)
    with pytest.raises(_lib.IrloscError, match="invalidated"):      # (the text names the fused step as the reason: ADVICE r4)
        osc.step()
    with pytest.raises(_lib.IrloscError, match="invalidated"):
        osc.step_resident(3)
    with pytest.raises(_lib.IrloscError, match="holds state for 0 instances"):
        osc.download_records(0)
    assert np.array_equal(osc.step_q(), u_fused)             # (qpos, qvel) and the targets are still there
    osc.frontend()
    assert osc.slot_structure(0) and np.array_equal(osc.step(), u_rec)
    empty = lambda: osc.lib.irlosc_upload(osc._h, 0, 0, None, None, None, None, None, None)
    assert empty() == 0                                      # an empty batch over records with the verdict: it goes with them
    assert not osc.slot_structure(0) and osc.slot_route(0) == "row16"
    osc.frontend()
    assert osc.slot_structure(0)
    osc.step_q()
    assert empty() == 0                                      # ... and over the slot a fused step left
    assert not osc.slot_structure(0) and osc.slot_route(0) == "row16"
    osc.close()


def test_k6_two_arms_xyz_runs_on_the_row16_kernel():
    """(k, ndev) = (6, 2): both arms, positions only, no base target (robot_configs/default_xyz.yaml:15-16,24-25 driven with the
    two arm targets).  Synthetic dense records and physical records (tree form), float64 and float32 records, against the
    oracle at 1e-5; the fused path from joint coordinates agrees with the path through records."""
    for dtype in (np.float64, np.float32):
        B = 1024
        lay, gains, g = synth.make_batch("k6", B, seed=61, dtype=dtype)
        assert lay.k == 6 and lay.ndev == 2
        u, fl, kname = run_gpu(lay, gains, g, dtype)
        assert "row16" in kname and kname.endswith("k6"), kname
        g64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
        idx = np.arange(0, B, 4)
        ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, g64["M"], g64["J"], g64["dq"], g64["bias"], g64["ee_pose"],
                                        g64["tgt_pose"], None, None, idx=idx)
        dom = np.array([in_parity_domain(*osc_oracle.task_inertia(g64["J"][b], g64["M"][b])[2:]) for b in idx])
        assert dom.mean() > 0.9 and rel_err(u[idx], ref[idx])[dom].max() <= TOL64
    lay, gains, g, rec, u_fe, fl_fe = _physical_records("k6", 512, np.float64, seed=63)
    st, u_t, fl_t = _run_uploaded(lay, gains, g, rec, np.float64)
    assert st and np.array_equal(u_t, u_fe)
    r = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, r["M"], r["J"], r["dq"], r["bias"], r["ee_pose"],
                                    np.asarray(g["tgt_pose"][:512], dtype=np.float64), None)
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(r["J"][b], r["M"][b])[2:]) for b in range(512)])
    assert rel_err(u_t, ref)[dom].max() <= TOL64
    lay, gains, g, model, osc, states = _from_q_setup("k6", 512, np.float64, seed=63, singular_every=7)     # the states of _physical_records
    assert "fused" in osc.from_q_name
    assert rel_err(osc.step_q(), u_fe.astype(np.float64)).max() <= 1e-8
    osc.close()


def test_time_trains_spans_and_periods_are_consistent():
    """irlosc_time_trains: per train an event pair and the kernel's own wall-clock stamps.  Starts increase, a train's in-kernel
    span is positive and no longer than its event pair (which also covers the give-up pass), the period between starts is no
    longer than span + a launch gap, and the outputs left behind are those of a plain step on the last slot visited."""
    nslots, B = 2, 8192
    lay = synth.make_layout("k13")
    osc = BatchedOSC(lay, B, n_slots=nslots)
    for sl in range(nslots):
        _, gains, g = synth.make_batch("k13", B, seed=500 + sl)
        osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], slot=sl)
        osc.set_targets(g["tgt_pose"], slot=sl)
        if sl == 0:
            osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    tt = osc.time_trains(24)
    u_tr, f_tr = osc.download(B)
    spl = osc.steps_per_launch
    last = ((24 + 1) * spl - 1) % nslots                      # one untimed train, then 24: the last step of the last train
    osc.step(slot=last)
    u1, f1 = osc.download(B)
    assert np.array_equal(u_tr, u1) and np.array_equal(f_tr, f1)
    span, per = tt[:, 2] - tt[:, 1], np.diff(tt[:, 1])
    assert tt[0, 1] == 0.0 and np.all(per > 0) and np.all(span > 0)
    assert np.all(span <= tt[:, 0] * 1e3 + 20.0)              # event pair (ms) covers the kernel (+ clock granularity)
    assert np.median(per) <= np.median(span) + 100.0
    assert np.all((tt[:, 3] > 400.0) & (tt[:, 3] < 3000.0))      # sustained shader clock in MHz, seen by a sample wave of each train
    osc.close()


def _bench_run(args, env_extra, timeout=1500, full=True):
    """bench.py in a child process with `args` (+ --full unless full=False) -> (return code, parsed JSON line or None, number of JSON
    lines, stderr)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(env_extra)
    if full:
        args = ["--full"] + list(args)
        if "--sustained-steps" not in args:      # (bench.py's default long leg is ~10 s at the headline batch: the tests ask for a short one)
            args = list(args) + ["--sustained-steps", "8000"]
    p = subprocess.run([sys.executable, "bench.py"] + args, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None), len(lines), p.stderr


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run is the headline alone: the timed steps and one line with metric / value / unit / higher_is_better / dtype /
    ms_per_step, none of the --full legs.  --dump-outputs writes the outputs of the LAST timed step: the same bits from a --full run
    with the same arguments, and (synthetic records, 2 slots, 16 steps: the last step ran on slot 1) the oracle's torques on slot 1's
    inputs."""
    import os
    common = ["--steps", "16", "--warmup", "8", "--preroll", "0", "--batch", "2048", "--slots", "2", "--workload", "synthetic"]
    rc, plain, n, err = _bench_run(common + ["--dump-outputs", str(tmp_path / "plain")], {}, full=False)
    assert rc == 0 and n == 1, err[-2000:]
    assert plain["metric"] == "OSC control steps/sec" and plain["unit"] == "steps/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f64" and plain["steps"] == 16 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert abs(plain["value"] * plain["ms_per_step"] * 1e-3 - 2048) < 1e-6 * 2048        # value = B / (ms_per_step in s)
    assert plain["config"]["full"] is False and plain["config"]["steps_per_launch"] >= 1
    for leg in ("roofline", "sustained", "cpu_baseline", "parity_sample", "secondary", "from_q", "end_to_end", "rank_checksums"):
        assert leg not in plain, leg
    rc, full, n, err = _bench_run(common + ["--dump-outputs", str(tmp_path / "full"), "--sustained-steps", "0", "--no-cpu-baseline",
                                            "--no-secondary", "--no-from-q", "--no-end-to-end"], {})
    assert rc == 0 and n == 1, err[-2000:]
    assert full["config"]["full"] is True and "roofline" in full and "rank_checksums" in full
    got = {d: {f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))} for d in ("plain", "full")}
    assert sorted(got["plain"]) == ["flags", "u"] and got["plain"]["u"].shape == (2048, 25) and got["plain"]["flags"].shape == (2048,)
    assert got["plain"]["u"].dtype == np.float64 and got["plain"]["flags"].dtype == np.float64
    for k in ("u", "flags"):
        assert np.array_equal(got["plain"][k], got["full"][k]), k
    lay, gains, g = synth.make_batch("k13", 2048, seed=20241008 + 2000 + 17 * 1)        # bench.py's synthetic slot 1 of rank 0
    n = 256
    g = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["tgt_pose"],
                                    g.get("wrench"), g.get("tgt_vel"))
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(g["J"][b], g["M"][b])[2:]) for b in range(n)])
    assert dom.sum() > n // 2 and rel_err(got["plain"]["u"][:n], ref)[dom].max() <= TOL64


def test_bench_config3_eight_ranks_dry_run_on_one_device():
    """BASELINE configs[3] = `bench.py --gpus 8 --total-batch 262144` (32 768 instances per rank), dry-run on the ONE GPU of this
    box: eight self-launched ranks share device 0 (IRLOSC_BENCH_DEVICE), RCCL refuses the duplicate device, all ranks switch to
    the file transport together (config.rccl_ranks = 0 says so).  One line, n_gpus = 8, eight checksums -- and each equals the
    checksum of the same slice of ONE process running the whole 262 144 (`--slices 8`): sharding changes no bit."""
    common = ["--steps", "16", "--warmup", "8", "--preroll", "0", "--slots", "2", "--total-batch", "262144", "--no-cpu-baseline",
              "--no-secondary", "--no-from-q", "--no-end-to-end"]
    rc8, eight, n8, err8 = _bench_run(["--gpus", "8"] + common, {"IRLOSC_BENCH_DEVICE": "0"})
    assert rc8 == 0 and n8 == 1, err8[-2000:]
    assert eight["n_gpus"] == 8 and len(eight["rank_checksums"]) == 8 and len(set(eight["rank_checksums"])) == 8
    assert eight["config"]["instances_per_gpu"] == 32768 and "configs[3]" in eight["config"]["workload"]
    assert eight["config"]["rccl_ranks"] == 0 and "files" in eight["config"]["sharding"]
    assert eight["scaling"] == "strong" and eight["value"] > 0 and eight["config"]["kernel"].endswith("+tree")
    rc1, one, n1, err1 = _bench_run(["--gpus", "1", "--slices", "8"] + common, {})
    assert rc1 == 0 and n1 == 1, err1[-2000:]
    assert one["n_gpus"] == 1 and one["config"]["instances_per_gpu"] == 262144 and one["config"]["rccl_ranks"] is None
    assert [r[0] for r in eight["slice_checksums"]] == one["slice_checksums"][0]
    assert eight["rank_checksums"] == [r[0] for r in eight["slice_checksums"]]


def test_bench_require_rccl_refuses_a_silent_downgrade():
    """--require-rccl: two ranks on one device cannot bring RCCL up (duplicate device) -> exit code != 0 and NO line, instead of a
    line whose only trace of the downgrade is config.sharding."""
    rc, line, n, err = _bench_run(["--gpus", "2", "--require-rccl", "--steps", "8", "--warmup", "4", "--preroll", "0", "--batch", "2048",
                                   "--no-cpu-baseline", "--no-secondary", "--no-from-q", "--no-end-to-end"], {"IRLOSC_BENCH_DEVICE": "0"})
    assert rc != 0 and n == 0 and "--require-rccl" in err


def test_bench_multi_rank_line_carries_cpu_baseline_and_parity_sample():
    """N > 1: rank 0 runs the CPU legs (before its RCCL / HIP initialisation, the other ranks wait in the rendezvous) and the line
    carries cpu_baseline + parity_sample like the 1-GPU line does."""
    rc, line, n, err = _bench_run(["--gpus", "2", "--steps", "16", "--warmup", "8", "--preroll", "0", "--batch", "4096", "--cpu-seconds", "0.5",
                                   "--no-secondary", "--no-from-q", "--no-end-to-end"], {"IRLOSC_BENCH_DEVICE": "0"})
    assert rc == 0 and n == 1, err[-2000:]
    assert line["n_gpus"] == 2 and line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1
    ps = line["parity_sample"]
    assert ps["n"] >= 512 and ps["n_over_tol_in_parity_domain"] == 0 and ps["max_rel_err"] <= TOL64


def test_bench_line_end_to_end_and_untraced_roofline():
    """The 1-GPU line: roofline.untraced (per-train kernel spans / periods of THIS run), roofline.committed_profile (what profiles/
    holds, labelled as such) and end_to_end (host arrays every tick: generate_batched, tick at B = 1, upload_raw + step)."""
    rc, line, n, err = _bench_run(["--steps", "64", "--warmup", "8", "--preroll", "0", "--batch", "8192", "--no-cpu-baseline",
                                   "--no-secondary", "--no-from-q"], {})
    assert rc == 0 and n == 1, err[-2000:]
    r = line["roofline"]
    un = r["untraced"]
    assert un["trains"] >= 32 and un["period_us"]["median"] > 0 and un["kernel_span_us"]["median"] > 0
    assert ("frac_rocprof" in r) == ("rocprof_source" in r)      # a committed (not live) number never travels without its label
    # flat scalars for the driver's record (it keeps the scalars of `roofline` / `config`, nested dicts are dropped)
    assert r["untraced_kernel_span_us"] == un["kernel_span_us"]["median"] and r["untraced_period_us"] == un["period_us"]["median"]
    assert 0 < r["frac_from_kernel_span"] < 1 and 500 < r["sclk_mhz"] < 2600
    c = line["config"]
    assert c["sustained_value"] == line["sustained"]["value"] and c["end_to_end_host_arrays_value"] > 0 and c["end_to_end_tick_b1_us"] > 0
    e = line["end_to_end"]
    assert e["generate_batched"]["value"] > 0 and e["generate_batched"]["pcie_GBps"] > 0.5
    assert 5 < e["tick_b1_us"]["median"] < 2000 and e["upload_raw_step"]["value"] > 0
    assert line["data"].startswith("synthetic")
    su = line["sustained"]
    assert su["steps"] == 8000 and su["value"] > 0 and 0.5 < su["value"] / line["value"] < 2.0
    # what the round claims sits inside the first 24 keys of the two dicts the driver's record truncates (bench.CONFIG_FIRST / ROOFLINE_FIRST)
    ck, rk = list(c)[:24], list(r)[:24]
    for must in ("workload", "sustained_value", "parity_n_outside_domain", "end_to_end_host_arrays_value", "end_to_end_pcie_GBps", "rccl_ranks"):
        assert must in ck or must not in c, (must, ck)
    for must in ("frac", "traffic", "untraced_kernel_span_us", "untraced_period_us", "frac_from_period"):
        assert must in rk, (must, rk)
    assert e["generate_batched_float32"]["value"] > e["generate_batched"]["value"]      # half the bytes over the same link


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_from_q_with_target_velocities_and_per_instance_gains(dtype):
    """The round-4 fused path splits the task-space signal: part 1 (calc_error, velocity limit, gains) in the task pass, one lane
    per robot; the damping-branch verdict, the target-velocity term (osc.py:173-181, branch B, needs dx = J dq) and the flags in the
    OSC kernel.  Layout with the base first and non-zero target velocities on two thirds of the robots, PER-INSTANCE gains (the pass
    reads them strided): torques and flags must equal the path through dense records (same arithmetic) -- and the oracle."""
    from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
    B = 777
    lay, gains, g = synth.make_batch("k13_branch_b", B, seed=91, dtype=dtype, per_instance_gains=True)
    assert g["tgt_vel"] is not None and np.ndim(gains["kp"]) == 2
    model = RigidBodyModel.load("dual_ur5")
    qpos, qvel = model.random_state(np.random.default_rng(92), B)
    osc = BatchedOSC(lay, B, dtype=dtype, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model, [DUAL_UR5_EE[d] for d in lay.dev_names])
    assert "fused" in osc.from_q_name
    osc.upload_q(qpos, qvel)
    osc.set_targets(g["tgt_pose"], g["tgt_vel"])
    u_f, fl_f = osc.step_q(return_flags=True)
    osc.frontend()
    u_d, fl_d = osc.step(return_flags=True)
    rec = osc.download_records(0)
    osc.close()
    assert np.array_equal(fl_f, fl_d) and np.all(fl_f[np.arange(B) % 3 != 0] & _lib.FLAG_VEL_BRANCH_B)
    assert not np.any(fl_f[::3] & _lib.FLAG_VEL_BRANCH_B)
    # float32 records: the dense path rounds M / J to float32, the fused path never forms them (float64 exchange buffer) -- the
    # difference is that rounding times the conditioning, not the kernels'
    assert rel_err(u_f.astype(np.float64), u_d.astype(np.float64)).max() <= (1e-9 if dtype == np.float64 else 1e-4)
    if dtype == np.float32:
        u_f = u_d                                          # the oracle below runs on the ROUNDED records: compare like with like
    n = 192
    r = {k: np.asarray(v[:n], dtype=np.float64) for k, v in rec.items()}
    gsub = {k: (np.asarray(v)[:n] if np.ndim(v) >= 1 and np.shape(v)[0] == B else v) for k, v in gains.items()}
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gsub, r["M"], r["J"], r["dq"], r["bias"], r["ee_pose"],
                                    np.asarray(g["tgt_pose"][:n], dtype=np.float64), None, np.asarray(g["tgt_vel"][:n], dtype=np.float64))
    dom = np.array([in_parity_domain(*osc_oracle.task_inertia(r["J"][b], r["M"][b])[2:]) for b in range(n)])
    assert dom.sum() > n // 2 and rel_err(u_f[:n].astype(np.float64), ref)[dom].max() <= TOL64


def _visible_gpus():
    return int(_lib.load().irlosc_device_count())


@pytest.mark.parametrize("world", [2, 8])
def test_rccl_ranks_when_that_many_gpus_are_visible(world):
    """SURVEY.md section 8(e) on hardware: the first box with >= `world` GPUs runs the real thing -- one process per GPU, RCCL over
    xGMI for the barrier / final reduction / checksum all-gather, `--require-rccl` so that a fall-back to the file transport is
    a failure, not a line -- and checks the rank checksums against one process cutting the same total batch into `world` slices.
    Skips with the reason on a smaller box (the builder's boxes have one GPU: RCCL with N > 1 ranks has never executed)."""
    have = _visible_gpus()
    if have < world:
        pytest.skip(f"{have} GPU(s) visible: the {world}-rank RCCL run needs {world}")
    common = ["--steps", "16", "--warmup", "8", "--preroll", "0", "--total-batch", str(4096 * world), "--no-cpu-baseline",
              "--no-secondary", "--no-from-q", "--no-end-to-end"]
    rc, many, n, err = _bench_run(["--gpus", str(world), "--require-rccl"] + common, {})
    assert rc == 0 and n == 1, err[-3000:]
    assert many["n_gpus"] == world and many["config"]["rccl_ranks"] == world and "RCCL" in many["config"]["sharding"].upper()
    assert len(set(many["rank_checksums"])) == world and many["value"] > 0
    rc1, one, n1, err1 = _bench_run(["--gpus", "1", "--slices", str(world)] + common, {})
    assert rc1 == 0 and n1 == 1, err1[-3000:]
    assert [r[0] for r in many["slice_checksums"]] == one["slice_checksums"][0]
    assert many["rank_checksums"] == [r[0] for r in many["slice_checksums"]]
