"""F/T sensor feed of the path from joint coordinates (-m gpu): irlosc_set_ft_sensors / irlosc_set_sensordata.  Every tick the
admittance wrench is the reference's (irl_control/device.py:135-170, osc.py:179-185) -- sensordata slices rotated by the ft_frame_*
site frame -- with the site frame taken from the step's own forward kinematics, on the fused path and through dense records."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, oracle_on_all
from irl_control_amd import BatchedOSC, _lib, synth
from oracle import osc_oracle
from oracle import rigid_body as rb

pytestmark = pytest.mark.gpu
TOL64 = 1e-5
NS = 18


def in_parity_domain(Mx_inv, det):
    s = np.linalg.svd(Mx_inv, compute_uv=False)
    if abs(det) >= 1e-4:
        return s[-1] > 1e-12 * s[0]
    r = s / s[0]
    return not np.any(np.abs(r / 1e-5 - 1.0) < 1e-2)


def rel_err(u, ref):
    return np.abs(u - ref).max(axis=1) / np.abs(ref).max(axis=1)


def setup(cfg, B, dtype, seed, n_slots=1, singular_every=0, sensors=True):
    """Context on the fused path (row16) with the shipped model, resident coordinates and targets in every slot, F/T sensors described."""
    from irl_control_amd.rigid_body import RigidBodyModel
    lay = synth.make_layout(cfg)
    _, gains, g = synth.make_batch(cfg, B, seed=seed, dtype=dtype)
    model = RigidBodyModel.load("dual_ur5")
    rng = np.random.default_rng(seed + 1000)
    osc = BatchedOSC(lay, B, dtype=dtype, n_slots=n_slots, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    if sensors:
        osc.set_ft_sensors()
    states = []
    for sl in range(n_slots):
        qpos, qvel = model.random_state(rng, B)
        if singular_every:                   # stretched / folded arms: every angle of the two arms a multiple of pi / 2
            idx = np.arange(sl, B, singular_every)
            qpos[idx, 1:7] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
            qpos[idx, 13:19] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
        osc.upload_q(qpos, qvel, slot=sl)
        osc.set_targets(g["tgt_pose"], slot=sl)
        states.append((qpos, qvel))
    return lay, gains, g, model, osc, states


def sensordata(rng, B):
    return rng.normal(0.0, 5.0, size=(B, NS))


def oracle_records_and_wrench(lay, fd, qpos, qvel, sens):
    """Records and world-frame wrench of every robot from the oracles alone: R_site = xmat(site body) quat2mat(site quat)."""
    from irl_control_amd.rigid_body import DUAL_UR5_EE
    om = rb.Model()
    B, nd = len(qpos), len(lay.dev_names)
    recs, W = [], np.zeros((B, nd, 6))
    for b in range(B):
        r = rb.records(om, lay.as_oracle_dict(), DUAL_UR5_EE, qpos[b], qvel[b])
        recs.append(r)
        for d in range(nd):
            sb = fd.site_body[d]
            if sb < 0:
                continue
            sq = np.array(fd.site_quat[d][:])
            R = r["kin"]["xmat"][sb] @ rb.quat2mat(sq / np.linalg.norm(sq))
            W[b, d, :3] = R @ sens[b, fd.ft_force0[d]:fd.ft_force0[d] + 3]
            W[b, d, 3:] = R @ sens[b, fd.ft_torque0[d]:fd.ft_torque0[d] + 3]
    R = {k: np.array([r[k] for r in recs]) for k in ("M", "J", "dq", "bias", "ee_pose")}
    return R, W


def check_against_oracle(lay, gains, R, W, tgt, u, fl):
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], tgt, W)
    B = len(u)
    dom = np.zeros(B, bool)
    pinv, trunc = np.zeros(B, bool), np.zeros(B, bool)
    for b in range(B):
        _, _, Mxi, det = osc_oracle.task_inertia(R["J"][b], R["M"][b])
        dom[b] = in_parity_domain(Mxi, det)
        sv = np.linalg.svd(Mxi, compute_uv=False)
        pinv[b] = abs(det) < 1e-4
        trunc[b] = pinv[b] and sv[-1] <= 1e-5 * sv[0]
    assert dom.mean() > 0.9
    err = rel_err(u.astype(np.float64), ref)
    assert err[dom].max() <= TOL64, float(err[dom].max())
    assert np.array_equal((fl[dom] & _lib.FLAG_PINV_BRANCH) != 0, pinv[dom])
    assert np.array_equal((fl[dom] & _lib.FLAG_TRUNCATED) != 0, trunc[dom])
    return ref


def test_sensor_feed_against_the_chained_oracles():
    """k12 + admittance, 2 085 robots (a seventh singular): torques of a fused step with a sensor feed against oracle/rigid_body.py ->
    oracle/osc_oracle.py with the wrench rotated by the oracle's own site frames.  The wrench acts: a zero reading gives other torques."""
    B = 2048 + 37
    lay, gains, g, model, osc, states = setup("k12_admit", B, np.float64, seed=51, singular_every=7)
    assert "osc_lane" in osc.from_q_name
    rng = np.random.default_rng(52)
    sens = sensordata(rng, B)
    osc.set_sensordata(sens)
    u, fl = osc.step_q(return_flags=True)
    osc.set_sensordata(np.zeros((B, NS)))
    u0 = osc.step_q()
    osc.close()
    assert np.all(np.isfinite(u))
    assert np.abs(u - u0).max() > 1.0
    qpos, qvel = states[0]
    R, W = oracle_records_and_wrench(lay, model.ft_desc(lay.dev_names), qpos, qvel, sens)
    check_against_oracle(lay, gains, R, W, g["tgt_pose"], u, fl)


def test_sensor_feed_full_size_oracle_on_every_robot():
    """65 536 robots from (qpos, qvel) with a sensor feed, no record upload: the oracle on every robot's front-end records, the wrench
    computed on the host from the downloaded EE quaternions and R_rel = R(ee)^T R(site) of the oracle at q = 0."""
    from irl_control_amd.rigid_body import DUAL_UR5_EE
    B = 65536
    lay, gains, g, model, osc, states = setup("k12_admit", B, np.float64, seed=611, singular_every=7)
    rng = np.random.default_rng(612)
    sens = sensordata(rng, B)
    osc.set_sensordata(sens)
    u, fl = osc.step_q(return_flags=True)
    assert np.all(np.isfinite(u)) and not np.any(fl & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    osc.frontend()
    rec = osc.download_records(0)
    osc.close()
    om = rb.Model()
    kin0 = rb.kinematics(om, np.zeros(om.nj))
    fd = model.ft_desc(lay.dev_names)
    W = np.zeros((B, lay.ndev, 6))
    for d, name in enumerate(lay.dev_names):
        sq = np.array(fd.site_quat[d][:])
        Rrel = kin0["xmat"][om.body_id(DUAL_UR5_EE[name])].T @ kin0["xmat"][fd.site_body[d]] @ rb.quat2mat(sq / np.linalg.norm(sq))
        q = rec["ee_pose"][:, d, 3:]
        Ree = np.array([rb.quat2mat(x) for x in q])
        Rs = Ree @ Rrel
        W[:, d, :3] = np.einsum("bij,bj->bi", Rs, sens[:, fd.ft_force0[d]:fd.ft_force0[d] + 3])
        W[:, d, 3:] = np.einsum("bij,bj->bi", Rs, sens[:, fd.ft_torque0[d]:fd.ft_torque0[d] + 3])
    rec["tgt_pose"] = g["tgt_pose"]
    rec["wrench"] = W
    ref, dom, pinv, trunc, _ = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    err = rel_err(u, ref)
    assert dom.mean() > 0.97
    assert err[dom].max() <= TOL64, float(err[dom].max())
    assert np.array_equal((fl[dom] & _lib.FLAG_PINV_BRANCH) != 0, pinv[dom])
    assert np.array_equal((fl[dom] & _lib.FLAG_TRUNCATED) != 0, trunc[dom])


def test_per_tick_readings_and_clearing_the_feed():
    """Three consecutive steps on one slot, a new reading each, nothing else uploaded: each matches its own oracle (no stale wrench).
    Clearing the feed brings back exactly the torques of the slot's record wrench."""
    B = 320
    lay, gains, g, model, osc, states = setup("k12_admit", B, np.float64, seed=61)
    qpos, qvel = states[0]
    osc.upload(g["M"], g["J"], g["dq"], g["bias"], g["ee_pose"], g["wrench"])      # a record wrench in the slot ...
    osc.upload_q(qpos, qvel)
    osc.set_targets(g["tgt_pose"])
    u_rec = osc.step_q()                                                            # ... the wrench of this step
    rng = np.random.default_rng(62)
    fd = model.ft_desc(lay.dev_names)
    for tick in range(3):
        sens = sensordata(rng, B)
        osc.set_sensordata(sens)
        u, fl = osc.step_q(return_flags=True)
        R, W = oracle_records_and_wrench(lay, fd, qpos, qvel, sens)
        check_against_oracle(lay, gains, R, W, g["tgt_pose"], u, fl)
        assert np.abs(u - u_rec).max() > 1e-3, tick
    osc.set_sensordata(None)
    u_back = osc.step_q()
    osc.close()
    assert np.array_equal(u_back, u_rec)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_equals_the_path_through_dense_records_with_a_feed(dtype, monkeypatch):
    """The wrench kernel reads the EE quaternion from the exchange buffer on the fused path and from ee_pose records on the path
    through dense records (IRLOSC_FUSED=0): same torques as the existing fused-vs-dense comparison demands, same flags."""
    B = 2048 + 37
    lay, gains, g, model, osc, states = setup("k12_admit", B, dtype, seed=71, singular_every=9)
    sens = sensordata(np.random.default_rng(72), B)
    osc.set_sensordata(sens)
    u_f, fl_f = osc.step_q(return_flags=True)
    osc.close()
    monkeypatch.setenv("IRLOSC_FUSED", "0")
    lay, gains, g, model, osc2, _ = setup("k12_admit", B, dtype, seed=71, singular_every=9)
    assert "through dense records" in osc2.from_q_name
    osc2.set_sensordata(sens)
    u_d, fl_d = osc2.step_q(return_flags=True)
    osc2.close()
    d = np.abs(u_f.astype(np.float64) - u_d).max(axis=1) / np.abs(u_d).max(axis=1)
    if dtype == np.float64:
        assert np.array_equal(fl_f, fl_d)
        assert d.max() <= 1e-9, float(d.max())
    else:
        same = ((fl_f ^ fl_d) & (_lib.FLAG_PINV_BRANCH | _lib.FLAG_TRUNCATED)) == 0
        assert same.mean() > 0.97
        assert np.median(d) <= 1e-5 and np.quantile(d[same], 0.99) <= 1e-2, (float(np.median(d)), float(np.quantile(d[same], 0.99)))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_trains_over_slots_with_and_without_feeds(fused, monkeypatch):
    """irlosc_step_resident_from_q over 4 slots, feeds on slots 0 and 2 only: the outputs left by the last train equal a single step on
    the last slot visited -- one with a feed (11 steps: slot 2) and one without (12 steps: slot 3)."""
    if fused == "0":
        monkeypatch.setenv("IRLOSC_FUSED", "0")
    B, nslots = 700, 4
    lay, gains, g, model, osc, states = setup("k12_admit", B, np.float64, seed=81, n_slots=nslots, singular_every=6)
    rng = np.random.default_rng(82)
    for sl in (0, 2):
        osc.set_sensordata(sensordata(rng, B), slot=sl)
    outs = {}
    for iters in (11, 12):
        osc.step_resident_from_q(iters, first_slot=0)
        u_t, f_t = osc.download(B)
        u_1, f_1 = osc.step_q(slot=(iters - 1) % nslots, return_flags=True)
        assert np.array_equal(u_t, u_1) and np.array_equal(f_t, f_1), iters
        outs[iters] = u_t
    # and the feed is really in those trains: slot 2 without its feed gives other torques
    osc.set_sensordata(None, slot=2)
    u_nofeed = osc.step_q(slot=2)
    osc.close()
    assert np.abs(u_nofeed - outs[11]).max() > 1.0


def test_admittance_off_ignores_the_feed():
    """Without IRLOSC_ADMITTANCE (k13) the reference reads the sensors and does not use them: torques bit-identical with and without a
    feed, on the fused path and through dense records."""
    B = 515
    lay, gains, g, model, osc, states = setup("k13", B, np.float64, seed=91, singular_every=5)
    assert not lay.admittance
    u0, f0 = osc.step_q(return_flags=True)
    osc.set_sensordata(sensordata(np.random.default_rng(92), B))
    u1, f1 = osc.step_q(return_flags=True)
    osc.close()
    assert np.array_equal(u0, u1) and np.array_equal(f0, f1)


def test_validation_of_the_sensor_description_and_feed():
    from irl_control_amd.rigid_body import RigidBodyModel
    B = 64
    lay = synth.make_layout("k12_admit")
    _, gains, g = synth.make_batch("k12_admit", B, seed=3)
    model = RigidBodyModel.load("dual_ur5")
    osc = BatchedOSC(lay, B, dtype=np.float64)
    lib, h = osc.lib, osc._h
    fd = model.ft_desc(lay.dev_names)
    assert lib.irlosc_set_ft_sensors(h, C.byref(fd)) == -3                    # before irlosc_set_model
    assert lib.irlosc_set_sensordata(h, 0, B, _lib.ptr(np.zeros((B, NS)))) == -3     # before irlosc_set_ft_sensors
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    bad = model.ft_desc(lay.dev_names, sites={"ur5left": "gripper_frame_ur5left"})    # a finger hinge between site and EE
    assert lib.irlosc_set_ft_sensors(h, C.byref(bad)) == -1
    assert b"device 1" in lib.irlosc_last_error(h)
    for field, val in (("ft_force0", 16), ("ft_torque0", -2), ("site_body", 99)):
        bad = model.ft_desc(lay.dev_names)
        getattr(bad, field)[0] = val
        assert lib.irlosc_set_ft_sensors(h, C.byref(bad)) == -1, field
        assert b"device 0" in lib.irlosc_last_error(h)
    osc.set_ft_sensors()
    qpos, qvel = model.random_state(np.random.default_rng(4), B)
    osc.upload_q(qpos, qvel)
    osc.set_targets(g["tgt_pose"])
    osc.set_sensordata(np.zeros((B // 2, NS)))                                # a feed of 32 robots, a step over 64
    assert lib.irlosc_step_from_q(h, 0, B, None, None) == -3
    osc.set_sensordata(None)
    osc.step_q()
    # a non-NULL d_sensordata on a context without sensor description
    osc2 = BatchedOSC(lay, B, dtype=np.float64)
    osc2.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc2.set_model(model)
    from conftest import HipBuffers
    hb = HipBuffers()
    try:
        dq, dv = hb.to_device(qpos), hb.to_device(qvel)
        dt, ds = hb.to_device(np.ascontiguousarray(g["tgt_pose"])), hb.to_device(np.zeros((B, NS)))
        du, dfl = hb.alloc(B * lay.n * 8), hb.alloc(B * 4)
        assert osc2.lib.irlosc_step_from_q_device(osc2._h, 0, B, dq, dv, dt, None, ds, du, dfl, None) == -3
        assert osc2.lib.irlosc_step_from_q_device(osc2._h, 0, B, dq, dv, dt, None, None, du, dfl, None) == 0
        hb.to_host(du, (B, lay.n), np.float64)
    finally:
        osc2.close()
        osc.close()
        hb.free()
    # a later irlosc_set_model clears the description
    osc = BatchedOSC(lay, B, dtype=np.float64)
    osc.set_model(model)
    osc.set_ft_sensors()
    osc.set_model(model)
    assert osc.lib.irlosc_set_sensordata(osc._h, 0, B, _lib.ptr(np.zeros((B, NS)))) == -3
    osc.close()


def test_admittance_from_q_example_runs():
    """examples/admittance_from_q_headless.py at small size: finite torques, and the push on the right arm moves its torques."""
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "admittance_from_q_headless.py"), "--robots", "8", "--ticks", "300"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert last, r.stdout[-2000:]
    vals = dict(kv.split("=") for kv in last[-1].split()[1:])
    assert vals["finite"] == "1"
    assert float(vals["push_delta_right"]) > 1.0
    assert float(vals["release_delta_right"]) < float(vals["push_delta_right"])
