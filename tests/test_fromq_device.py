"""irlosc_step_from_q_device (-m gpu): one step from joint coordinates on caller-owned device arrays -- coordinates, targets, F/T
sensordata, outputs -- with a resident slot lending its buffers as scratch.  Bit for bit the host-fed step on the same inputs."""
import ctypes as C

import numpy as np
import pytest

from conftest import HipBuffers
from irl_control_amd import BatchedOSC, _lib, synth

pytestmark = pytest.mark.gpu
NS = 18


def _context(B, dtype, seed):
    from irl_control_amd.rigid_body import RigidBodyModel
    lay = synth.make_layout("k12_admit")
    _, gains, g = synth.make_batch("k12_admit", B, seed=seed, dtype=dtype)
    model = RigidBodyModel.load("dual_ur5")
    osc = BatchedOSC(lay, B, dtype=dtype, n_slots=2, kernel=_lib.KERNEL_ROW16)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    osc.set_ft_sensors()
    return lay, g, model, osc


def _inputs(model, B, dtype, g, rng, singular_every=7):
    qpos, qvel = model.random_state(rng, B)
    idx = np.arange(0, B, singular_every)
    qpos[idx, 1:7] = (np.pi / 2) * rng.integers(-2, 3, size=(len(idx), 6))
    tgt = np.array(g["tgt_pose"], dtype=dtype)          # (a copy: every call perturbs its own)
    tgt[:, :, :3] += rng.normal(0.0, 0.05, size=tgt[:, :, :3].shape).astype(dtype)
    return qpos, qvel, tgt, rng.normal(0.0, 5.0, size=(B, NS))


def _run(B, dtype, with_sens, stream=False, seed=5):
    lay, g, model, osc = _context(B, dtype, seed)
    rng = np.random.default_rng(seed + 1)
    qpos, qvel, tgt, sens = _inputs(model, B, dtype, g, rng)
    # the host-fed step on slot 0
    osc.upload_q(qpos, qvel, slot=0)
    osc.set_targets(tgt, slot=0)
    if with_sens:
        osc.set_sensordata(sens, slot=0)
    u_ref, fl_ref = osc.step_q(slot=0, return_flags=True)
    # slot 1, the scratch slot, holds OTHER coordinates, targets and a feed: nothing of them may reach the device-pointer step
    q2, v2, t2, s2 = _inputs(model, B, dtype, g, rng)
    osc.upload_q(q2, v2, slot=1)
    osc.set_targets(t2[::-1].copy(), slot=1)
    osc.set_sensordata(s2, slot=1)
    hb = HipBuffers()
    hip = hb.hip
    st = C.c_void_p()
    try:
        dq, dv, dt = hb.to_device(qpos), hb.to_device(qvel), hb.to_device(tgt)
        ds = hb.to_device(sens) if with_sens else None
        du, dfl = hb.alloc(B * lay.n * np.dtype(dtype).itemsize), hb.alloc(B * 4)
        if stream:
            hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
            assert hip.hipStreamCreate(C.byref(st)) == 0
        osc.step_from_q_device(B, dq, dv, dt, du, dfl, d_sensordata=ds, slot=1, stream=st if stream else None)
        if stream:
            hip.hipStreamSynchronize.argtypes = [C.c_void_p]
            assert hip.hipStreamSynchronize(st) == 0
        u = hb.to_host(du, (B, lay.n), dtype)
        fl = hb.to_host(dfl, (B,), np.uint32)
        # the scratch slot holds no records and no joint coordinates afterwards
        with pytest.raises(_lib.IrloscError, match="-3"):
            osc.step_q(slot=1)
        with pytest.raises(_lib.IrloscError, match="-3"):
            osc.download_records(slot=1)
        assert osc.lib.irlosc_step(osc._h, 1, B, None, None) == -3
        # ... its targets and feed stay: refilled with the host arrays, slot 1 steps like slot 0 did
        osc.upload_q(qpos, qvel, slot=1)
        osc.set_targets(tgt, slot=1)
        if not with_sens:
            osc.set_sensordata(None, slot=1)
        else:
            osc.set_sensordata(sens, slot=1)
        u_again = osc.step_q(slot=1)
    finally:
        if stream and st.value:
            hip.hipStreamDestroy.argtypes = [C.c_void_p]
            hip.hipStreamDestroy(st)
        hb.free()
        osc.close()
    return u, fl, u_ref, fl_ref, u_again


@pytest.mark.parametrize("with_sens", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", [1000, 65536])
def test_device_step_equals_the_host_fed_step(B, dtype, with_sens):
    u, fl, u_ref, fl_ref, u_again = _run(B, dtype, with_sens)
    assert np.all(np.isfinite(u))
    assert np.array_equal(u, u_ref) and np.array_equal(fl, fl_ref)
    assert np.array_equal(u_again, u_ref)


def test_device_step_on_a_caller_stream():
    u, fl, u_ref, fl_ref, _ = _run(1000, np.float64, True, stream=True, seed=9)
    assert np.array_equal(u, u_ref) and np.array_equal(fl, fl_ref)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_step_through_dense_records(dtype, monkeypatch):
    """IRLOSC_FUSED=0: the device-pointer step runs front end + wrench + step through the scratch slot's dense records."""
    monkeypatch.setenv("IRLOSC_FUSED", "0")
    u, fl, u_ref, fl_ref, _ = _run(1000, dtype, True, seed=13)
    assert np.array_equal(u, u_ref) and np.array_equal(fl, fl_ref)
