"""The resident lane route of irlosc_step / irlosc_step_resident: float64 tree-form records of an AUTO context with a model whose
layout has a lane tier are packed once into a compact block, and every step runs the lane-per-robot OSC step on it (include/irlosc.h,
irlosc_slot_route).  Held against the row16 route on the same records (IRLOSC_RESIDENT_LANE=0), the oracle, the fused path from joint
coordinates, its own single steps, and records that change under it."""
import os

import numpy as np
import pytest

from conftest import oracle_on_all
from irl_control_amd import BatchedOSC, _lib, synth

pytestmark = pytest.mark.gpu

TOL64 = 1e-5
LANE_MIN_B = 4096


def _rel(u, ref):
    sc = np.maximum(np.abs(ref).max(axis=1), 1.0)
    return np.abs(u - ref).max(axis=1) / sc


def _physical(cfg, B, seed, n_slots=1, lane=True):
    """An AUTO float64 context with the Dual-UR5 model, records of B physical robot states in slot 0 (front end on the GPU, every
    10th robot with arms at multiples of pi / 2), targets around the end effectors.  -> (lay, gains, model, osc, rec incl. qpos / qvel)"""
    from irl_control_amd.rigid_body import RigidBodyModel
    old = os.environ.get("IRLOSC_RESIDENT_LANE")
    os.environ["IRLOSC_RESIDENT_LANE"] = "1" if lane else "0"      # read at irlosc_create
    try:
        lay = synth.make_layout(cfg)
        osc = BatchedOSC(lay, B, dtype=np.float64, n_slots=n_slots, kernel=_lib.KERNEL_AUTO)
    finally:
        if old is None:
            os.environ.pop("IRLOSC_RESIDENT_LANE")
        else:
            os.environ["IRLOSC_RESIDENT_LANE"] = old
    _, gains, _ = synth.make_batch(cfg, 2, seed=1, dtype=np.float64)
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(seed)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    qpos, qvel = model.random_state(rng, B)
    idx = np.arange(3, B, 10)
    qpos[idx, 1:7] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    qpos[idx, 13:19] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    osc.upload_q(qpos, qvel)
    osc.frontend()
    rec = osc.download_records(0)
    rec["qpos"], rec["qvel"] = qpos, qvel
    rec["tgt_pose"] = synth.targets_near(rec["ee_pose"], rng)
    if lay.admittance:
        rec["wrench"] = rng.normal(0.0, 5.0, size=(B, lay.ndev, 6))
        osc.upload(rec["M"], rec["J"], rec["dq"], rec["bias"], rec["ee_pose"], rec["wrench"])
    osc.set_targets(rec["tgt_pose"])
    return lay, gains, model, osc, rec


def _upload(osc, rec, slot=0, lo=0, hi=None):
    w = rec.get("wrench")
    osc.upload(rec["M"][lo:hi], rec["J"][lo:hi], rec["dq"][lo:hi], rec["bias"][lo:hi], rec["ee_pose"][lo:hi],
               None if w is None else w[lo:hi], slot=slot)
    osc.set_targets(rec["tgt_pose"][lo:hi], slot=slot)


@pytest.mark.parametrize("cfg", ["k13", "k12_admit", "k7"])
def test_lane_route_against_row16_and_the_oracle_full_size(cfg):
    """65 536 physical records: the lane route and the row16 route (IRLOSC_RESIDENT_LANE=0) give the same flags and torques within
    1e-7 in the parity domain; the lane route meets the oracle on every robot (<= 1e-5, PINV / TRUNCATED = the reference's branch)."""
    B = 65536
    lay, gains, _, r16, rec = _physical(cfg, B, seed=777, lane=False)
    assert r16.slot_route(0) == "row16_tree"
    u_r, f_r = r16.step(return_flags=True)
    r16.close()
    _, _, _, osc, rec2 = _physical(cfg, B, seed=777, lane=True)
    assert np.array_equal(rec2["M"], rec["M"]) and np.array_equal(rec2["J"], rec["J"])
    assert osc.slot_route(0) == "lane", osc.slot_route(0)
    assert "row16" in osc.kernel_name and osc.slot_structure(0)       # what the context reports does not change with the route
    u_l, f_l = osc.step(return_flags=True)
    osc.close()
    ref, dom, pinv, trunc, _ = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    d = _rel(u_l, u_r)
    err = _rel(u_l, ref)
    print(f"{cfg}: lane vs row16 max rel {d[dom].max():.2e} (bit-equal robots {np.mean(np.all(u_l == u_r, axis=1)):.3f}); "
          f"lane vs oracle max rel {err[dom].max():.2e}; eigen path {np.mean((f_l & _lib.FLAG_EIGEN_PATH) != 0):.3f}")
    assert np.array_equal(f_l, f_r)
    assert d[dom].max() <= 1e-7, float(d[dom].max())
    assert dom.mean() > 0.97 and err[dom].max() <= TOL64, float(err[dom].max())
    assert np.array_equal((f_l[dom] & _lib.FLAG_PINV_BRANCH) != 0, pinv[dom])
    assert np.array_equal((f_l[dom] & _lib.FLAG_TRUNCATED) != 0, trunc[dom])


def test_front_end_records_routed_against_the_fused_step():
    """The same (qpos, qvel, targets): records of the record-form front end on the lane route against step_q() on the fused path
    (compact walk -> lane kernel).  Both walks park their values in the same order; the torques agree to rounding, flags exactly."""
    B = 8192 + 64
    _, _, _, osc, rec = _physical("k13", B, seed=31)
    assert osc.slot_route(0) == "lane"
    u_l, f_l = osc.step(return_flags=True)
    u_q, f_q = osc.step_q(return_flags=True)
    d = _rel(u_l, u_q)
    print(f"front-end records on the lane route vs the fused step: bit-equal robots {np.mean(np.all(u_l == u_q, axis=1)):.4f}, "
          f"max rel {d.max():.2e}")
    assert np.array_equal(f_l, f_q)
    assert d.max() <= 1e-9, float(d.max())
    osc.close()


def _train_equals_single_step(osc, nslots, iters, first, B):
    osc.step_resident(iters, first_slot=first)
    u_t, f_t = osc.download(B)
    last = (first + iters - 1) % nslots
    u_1, f_1 = osc.step(slot=last, return_flags=True)
    assert np.array_equal(u_t, u_1) and np.array_equal(f_t, f_1), (iters, first, last)


@pytest.mark.parametrize("iters", [1, 7, 8, 9, 17])
def test_resident_trains_over_lane_and_other_slots_equal_single_steps(iters):
    """Two lane slots alone; then four slots -- two on the lane route, synthetic records (no tree verdict), physical records with
    target velocities (row16).  Every train split leaves bit-for-bit what a single step on the last slot gives."""
    B = LANE_MIN_B + 64 + 5
    lay, _, _, osc, rec0 = _physical("k13", B, seed=5, n_slots=2)
    _, _, _, o4, rec1 = _physical("k13", B, seed=6, n_slots=4)
    _upload(osc, rec1, slot=1)
    assert [osc.slot_route(s) for s in range(2)] == ["lane", "lane"]
    _train_equals_single_step(osc, 2, iters, 1, B)
    osc.close()
    _upload(o4, rec0, slot=1)
    _, _, g = synth.make_batch("k13", B, seed=9, dtype=np.float64)
    o4.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g.get("wrench"), slot=2)
    o4.set_targets(g["tgt_pose"], g.get("tgt_vel"), slot=2)
    _upload(o4, rec1, slot=3)
    o4.set_targets(rec1["tgt_pose"], np.full((B, lay.ndev, 6), 0.05), slot=3)
    assert [o4.slot_route(s) for s in range(4)] == ["lane", "lane", "row16", "row16_tree"]
    _train_equals_single_step(o4, 4, iters, 1, B)
    _train_equals_single_step(o4, 4, iters, 3, B)
    o4.close()


def test_ragged_batch_and_a_split_at_an_offset_are_bit_exact():
    """A ragged batch on the lane route, and its tail uploaded alone (a split at an offset that is not a multiple of 64): bit-exact
    per robot.  (Bits hold only within one form of the eigen pass, and the form follows the step's count of flagged robots
    (IRLOSC_LANE_EIG_MIN): both sides must be on the same side of that threshold -- test_resident_lane_edges.py compares the forms.)"""
    B = 2 * LANE_MIN_B + 37
    eig_min = int(os.environ.get("IRLOSC_LANE_EIG_MIN", "3000"))
    _, _, _, osc, rec = _physical("k13", B, seed=11)
    assert osc.slot_route(0) == "lane"
    u, f = osc.step(return_flags=True)
    h = B - LANE_MIN_B - 3
    _upload(osc, rec, lo=h)
    assert osc.slot_route(0) == "lane"
    uh, fh = osc.step(return_flags=True)
    n_all, n_tail = (int(np.count_nonzero(x & _lib.FLAG_EIGEN_PATH)) for x in (f, fh))
    assert (n_all >= eig_min) == (n_tail >= eig_min), (n_all, n_tail, eig_min)
    assert np.array_equal(uh, u[h:]) and np.array_equal(fh, f[h:])
    osc.close()


def test_threshold_boundary():
    """Records of LANE_MIN_B - 1 robots stay on the row16 kernel, LANE_MIN_B robots take the lane route; both agree to rounding."""
    B = LANE_MIN_B
    _, _, _, osc, rec = _physical("k13", B, seed=12)
    assert osc.slot_route(0) == "lane" and osc.slot_route(0, B - 1) == "row16_tree"
    u_l = osc.step()
    _upload(osc, rec, hi=B - 1)
    assert osc.slot_route(0) == "row16_tree"
    u_r = osc.step()
    assert _rel(u_l[:B - 1], u_r).max() <= 1e-7
    osc.close()


def test_stale_blocks_are_never_read():
    """New records in a lane slot: the step follows them.  A fused step from joint coordinates leaves no records (the step fails
    until the front end fills the slot again), and the refilled slot gives what it gave before."""
    B = LANE_MIN_B + 128
    _, _, _, osc, recA = _physical("k13", B, seed=21)
    uA = osc.step()
    _, _, _, o2, recB = _physical("k13", B, seed=22)
    uB_ref = o2.step()
    o2.close()
    _upload(osc, recB)
    assert osc.slot_route(0) == "lane"
    assert np.array_equal(osc.step(), uB_ref)
    # back to A's coordinates: fused step, then no records, then the front end again
    osc.set_targets(recA["tgt_pose"])
    osc.upload_q(recA["qpos"], recA["qvel"])
    osc.step_q()
    assert osc.slot_route(0) != "lane"
    with pytest.raises(_lib.IrloscError):
        osc.step()
    osc.frontend()
    assert osc.slot_route(0) == "lane"
    assert np.array_equal(osc.step(), uA)
    osc.close()
