"""Closed loops on the GPU (-m gpu): irlosc_set_plant / irlosc_rollout_from_q / irlosc_download_q -- the contact-free plant
(csrc/osc_plant.hpp) behind the fused step from joint coordinates, against the CPU oracles, against itself tick by tick, against the
host loop of examples/closed_loop_headless.py, and the state rules around it.

Run as a script (`python tests/test_rollout.py --host-loop OUT.npz`) it is the child process of the trajectory test: the reference host
loop under whatever IRLOSC_* switches the parent set."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from irl_control_amd import BatchedOSC, _lib, synth                  # noqa: E402
from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel   # noqa: E402
from oracle import osc_oracle                                        # noqa: E402
from oracle import rigid_body as rb                                  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NS = 18
ERR_ARG, ERR_STATE = -1, -3


def actuated_joints():
    with open(os.path.join(ROOT, "irl_control_amd", "models", "dual_ur5.json")) as f:
        m = json.load(f)
    return [m["joint_names"].index(j) for j in m["actuator_joints"]]


def make_ctx(cfg, B, dtype=np.float64, feed=False, seed=0, **kw):
    lay = synth.make_layout(cfg)
    _, gains, g = synth.make_batch(cfg, B, seed=seed, dtype=dtype)
    model = RigidBodyModel.load("dual_ur5")
    osc = BatchedOSC(lay, B, dtype=dtype, **kw)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(model)
    if feed:
        osc.set_ft_sensors()
    return lay, gains, g, model, osc


# ---- 1. one tick against the CPU oracles ------------------------------------------------------------------------------------------
_ORACLE = {}


def _mb_chunk(span, cfg="k13", ee=False):
    """(cfg: the layout whose device order the EE poses follow; M and bias do not depend on it.  ee: return the EE poses as well)"""
    lo, hi = span
    om = rb.Model()
    lay = synth.make_layout(cfg).as_oracle_dict()
    q, qd = _ORACLE["q"], _ORACLE["qd"]
    M, bias = np.zeros((hi - lo, 25, 25)), np.zeros((hi - lo, 25))
    pose = np.zeros((hi - lo, len(lay["dev_names"]), 7))
    for b in range(lo, hi):
        r = rb.records(om, lay, DUAL_UR5_EE, q[b], qd[b])
        M[b - lo], bias[b - lo], pose[b - lo] = r["M"], r["bias"], r["ee_pose"]
    return (lo, M, bias, pose) if ee else (lo, M, bias)


def oracle_M_bias(q, qd):
    """oracle/rigid_body.py -> (M, bias) of every state, over the cores this process may use (computed once per state set)."""
    key = (q.shape[0], float(q[0, 1]))
    if _ORACLE.get("key") == key:
        return _ORACLE["M"], _ORACLE["bias"]
    import multiprocessing as mp
    B = q.shape[0]
    _ORACLE.update(q=q, qd=qd)
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    nw = max(1, min(cores, 16))
    step = max(16, -(-B // (nw * 4)))
    spans = [(lo, min(B, lo + step)) for lo in range(0, B, step)]
    if nw == 1:
        parts = [_mb_chunk(s) for s in spans]
    else:
        with mp.get_context("fork").Pool(nw) as pool:
            parts = pool.map(_mb_chunk, spans)
    M, bias = np.zeros((B, 25, 25)), np.zeros((B, 25))
    for lo, m, b in parts:
        M[lo:lo + len(m)], bias[lo:lo + len(m)] = m, b
    _ORACLE.update(key=key, M=M, bias=bias)
    return M, bias


C_BOUND = 64.0


@pytest.mark.parametrize("cfg,dtype,damping,masked", [
    ("k13", np.float64, 0.0, False), ("k12_admit", np.float64, 0.0, False), ("k13", np.float32, 0.0, False),
    ("k12_admit", np.float32, 0.0, False), ("k13", np.float64, 0.7, False), ("k13", np.float64, 0.0, True)])
def test_one_tick_against_the_cpu_oracles(cfg, dtype, damping, masked):
    """4 096 random states, every robot.  Reference: oracle/rigid_body.py -> M, bias; u = what step_q returns on the same slot state
    (float32 contexts: that float32 u, on both sides); qacc_ref = np.linalg.solve(M, ctrl(u) - bias - damping qvel); Euler in NumPy.

    Bound on qacc, per robot: C eps64 cond_2(M) max|qacc_ref| with C = 64.  Where C comes from: both sides solve M x = rhs with a
    backward-stable factorisation (LAPACK's LU there, the tree's L^T L here), so each x is the exact solution for an M and a rhs
    perturbed relatively by a small multiple of eps64, and the forward error is that multiple times cond_2(M).  The multiples: the
    two M / bias come from two independent float64 evaluations of a 35-body recursion (walk on the GPU, oracle on the CPU), each entry
    a sum over up to 24 bodies through at most 10 frames -- 24 + 10 = 34 roundings worst case, taken as 32 eps relative to |M|; the
    two factorisations and their triangular solves have rows of at most 10 non-zeros (the deepest path of the tree), 3 x 10 eps
    (Higham, Thm 10.4 with the row length in place of n) for both together taken as 32 eps.  Then qvel: dt x that + 4 eps max|qvel|
    (the rounding of the update itself), qpos: dt x the qvel bound + 4 eps max|qpos|.
    Measured on an MI355X (printed by the test; profiles/rollout_rates.md): cond_2(M) of the oracle's M over these 4 096 states
    1.79e5 .. 1.19e6, median 5.11e5; worst qvel error 0.14 (float64 contexts) / 0.28 (float32) in units of dt eps cond max|qacc|."""
    B, dt = 4096, 1e-3
    feed = cfg == "k12_admit"
    lay, gains, g, model, osc = make_ctx(cfg, B, dtype, feed=feed, seed=21)
    assert "fused" in osc.from_q_name
    qpos, qvel = model.random_state(np.random.default_rng(4242), B)
    osc.upload_q(qpos, qvel)
    osc.set_targets(g["tgt_pose"])
    if feed:
        osc.set_sensordata(np.random.default_rng(43).normal(0.0, 5.0, size=(B, NS)))
    u, fl = osc.step_q(return_flags=True)
    act = actuated_joints() if masked else None
    osc.set_plant(dt, damping, act)
    out = osc.rollout(1)
    osc.close()
    assert u.dtype == np.dtype(dtype) and np.array_equal(out["u"], u)
    assert np.array_equal(out["flags_any"], fl)
    assert not np.any(fl & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    M, bias = oracle_M_bias(qpos, qvel)
    ctrl = u.astype(np.float64)
    if masked:
        keep = np.zeros(25, bool)
        keep[act] = True
        ctrl = np.where(keep[None, :], ctrl, 0.0)
    qacc = np.linalg.solve(M, (ctrl - bias - damping * qvel)[:, :, None])[:, :, 0]
    qv_ref = qvel + dt * qacc
    qp_ref = qpos + dt * qv_ref
    cond = np.linalg.cond(M)
    amax = np.abs(qacc).max(axis=1)
    unit = EPS * cond * amax
    ev = np.abs(out["qvel"] - qv_ref).max(axis=1)
    ep = np.abs(out["qpos"] - qp_ref).max(axis=1)
    bv = dt * C_BOUND * unit + 4 * EPS * np.abs(qv_ref).max(axis=1)
    bp = dt * bv + 4 * EPS * np.abs(qp_ref).max(axis=1)
    print(f"[one tick {cfg} {np.dtype(dtype).name} damping={damping} masked={masked}] cond2(M) min {cond.min():.3g} median {np.median(cond):.3g} "
          f"max {cond.max():.3g}; worst qvel error / (dt eps cond max|qacc|) = {(ev / (dt * unit)).max():.3g} (bound {C_BOUND:g}); "
          f"max |dqvel| {ev.max():.3g}, max |dqpos| {ep.max():.3g}, max |qacc| {amax.max():.3g}")
    assert np.all(ev <= bv), (float((ev / bv).max()), int(np.argmax(ev / bv)))
    assert np.all(ep <= bp), (float((ep / bp).max()), int(np.argmax(ep / bp)))


# ---- 2. T ticks equal T single ticks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1000, 65536])
def test_rollout_of_T_ticks_equals_T_single_ticks(B):
    """rollout(24) against 24 x rollout(1) from the same start, bit for bit (coordinates, last torques, OR of the flags); at B = 1 000
    (ragged last wave) also: the first B robots of a rollout on 2 B robots are the rollout on B (a robot does not see its wave mates)."""
    T = 24
    lay, gains, g, model, osc = make_ctx("k13", B, seed=5)
    qpos, qvel = model.random_state(np.random.default_rng(77), B)
    osc.set_plant(1e-3, 0.05)
    osc.upload_q(qpos, qvel)
    osc.set_targets(g["tgt_pose"])
    a = osc.rollout(T)
    osc.upload_q(qpos, qvel)
    fl = np.zeros(B, np.uint32)
    for _ in range(T):
        b = osc.rollout(1)
        fl |= b["flags_any"]
    osc.close()
    assert np.all(np.isfinite(a["qpos"])) and np.abs(a["qpos"] - qpos).max() > 1e-6
    for key in ("qpos", "qvel", "u"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["flags_any"], fl)
    if B > 1000:
        return
    lay, gains, g2, model, big = make_ctx("k13", 2 * B, seed=5)
    q2, v2 = model.random_state(np.random.default_rng(78), 2 * B)
    q2[:B], v2[:B] = qpos, qvel
    t2 = g2["tgt_pose"].copy()
    t2[:B] = g["tgt_pose"]
    big.set_plant(1e-3, 0.05)
    big.upload_q(q2, v2)
    big.set_targets(t2)
    c = big.rollout(T)
    big.close()
    for key in ("qpos", "qvel", "u", "flags_any"):
        assert np.array_equal(a[key], c[key][:B]), key


# ---- the host loop of examples/closed_loop_headless.py on given start states -------------------------------------------------------
def host_loop(q0, tgt, ticks, dt=1e-3, damping=0.0, tile=1, watch=False):
    """The loop of closed_loop_headless.run, line by line, from start states q0 towards targets tgt: upload_q -> frontend ->
    set_targets -> step on dense records, M and bias read back, np.linalg.solve, semi-implicit Euler.  `tile`: the robots repeated
    that many times in the batch (robots are independent; 64 and more make the records eligible for the tree-structured
    factorisation, which IRLOSC_TREE=0 then switches off) -- the first len(q0) are reported.  `watch`: per tick and robot, is the
    state inside the parity domain as conftest._oracle_chunk defines it, and would the reference truncate?"""
    n0 = len(q0)
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 1, seed=0)
    osc = BatchedOSC(lay, n0 * tile, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    q, qd, tg = np.tile(q0, (tile, 1)), np.zeros((n0 * tile, 25)), np.tile(tgt, (tile, 1, 1))
    dom, trunc = np.ones((ticks, n0), bool), np.zeros((ticks, n0), bool)
    for t in range(ticks):
        osc.upload_q(q, qd)
        osc.frontend()
        osc.set_targets(tg)
        u = osc.step()
        rec = osc.download_records()
        if watch:
            for b in range(n0):
                _, _, Mxi, det = osc_oracle.task_inertia(rec["J"][b], rec["M"][b])
                sv = np.linalg.svd(Mxi, compute_uv=False)
                if abs(det) >= 1e-4:
                    dom[t, b] = sv[-1] > 1e-12 * sv[0]
                else:
                    dom[t, b] = not np.any(np.abs(sv / sv[0] / 1e-5 - 1.0) < 1e-2)
                trunc[t, b] = abs(det) < 1e-4 and sv[-1] <= 1e-5 * sv[0]
        qacc = np.linalg.solve(rec["M"], (u - rec["bias"] - damping * qd)[:, :, None])[:, :, 0]
        qd = qd + dt * qacc
        q = q + dt * qd
    ee = rec["ee_pose"][:n0].copy()      # (of the state before the last integration, as the example reports it)
    osc.close()
    return dict(q=q[:n0], qd=qd[:n0], dom=dom, trunc=trunc, ee_last=ee)


def ee_poses(q):
    lay = synth.make_layout("k13")
    osc = BatchedOSC(lay, len(q), dtype=np.float64)
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.upload_q(q, np.zeros_like(q))
    osc.frontend()
    ee = osc.download_records(keys=("ee_pose",))["ee_pose"].copy()
    osc.close()
    return ee


def box_scenario(robots=16, seed=1):      # (seed 0: three robots leave the parity domain within 300 ticks; the cap is two)
    rng = np.random.default_rng(seed)
    q = np.zeros((robots, 25))
    q[:, 1:7] = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3]) + rng.uniform(-0.15, 0.15, (robots, 6))
    q[:, 13:19] = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2]) + rng.uniform(-0.15, 0.15, (robots, 6))
    goal = q.copy()
    goal[:, 1:7] += rng.uniform(-0.1, 0.1, (robots, 6))
    goal[:, 13:19] += rng.uniform(-0.1, 0.1, (robots, 6))
    return q, goal


def test_trajectory_against_the_host_loop():
    """16 robots, 300 ticks, k13, start states in insertion_fleet_headless.py's box, goal = start +- 0.1 on the twelve arm joints.
    Reference: the host loop of closed_loop_headless.py (dense records + NumPy).  Tolerance on q at tick 300: 10 x the spread
    between two REFERENCE loops -- the host loop as is and the host loop with IRLOSC_TREE=0 in a fresh child process, both on the 16
    robots repeated four times (64 records: below that the tree-structured form the switch turns off is never taken and the two
    loops would be one) -- floor 1e-9.  Left out: robots whose reference loop leaves the parity domain of conftest._oracle_chunk at
    some tick or whose TRUNCATED verdict changes between ticks; at most 2 of 16 (seed 1: robots 3 and 12).  Measured on an MI355X: spread
    of the two reference loops 9.7e-15 -> tolerance at its floor, 1e-9; rollout against the host loop 5.1e-15 (profiles/rollout_rates.md)."""
    T = 300
    q0, goal = box_scenario()
    tgt = ee_poses(goal)
    ref = host_loop(q0, tgt, T, tile=4, watch=True)
    import tempfile
    out_npz = os.path.join(tempfile.mkdtemp(prefix="irlosc_rollout_"), "hostloop_tree0.npz")
    env = dict(os.environ, IRLOSC_TREE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-loop", out_npz], capture_output=True, text=True, timeout=1200,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref0 = np.load(out_npz)["q"]
    os.remove(out_npz)
    keep = ref["dom"].all(axis=0) & (ref["trunc"] == ref["trunc"][0]).all(axis=0)
    print(f"[trajectory] robots left out: {np.nonzero(~keep)[0].tolist()}")
    assert (~keep).sum() <= 2, np.nonzero(~keep)[0]
    spread = np.abs(ref["q"] - ref0)[keep].max()
    tol = max(10.0 * spread, 1e-9)
    lay, gains, g, model, osc = make_ctx("k13", 16)
    osc.set_plant(1e-3, 0.0)
    osc.upload_q(q0, np.zeros_like(q0))
    osc.set_targets(tgt)
    out = osc.rollout(T)
    osc.close()
    err = np.abs(out["qpos"] - ref["q"])[keep].max()
    print(f"[trajectory] kept {int(keep.sum())}/16 robots; spread of the two reference loops at tick {T}: {spread:.3g} -> tolerance "
          f"{tol:.3g}; rollout against the host loop: {err:.3g}")
    assert err <= tol, (err, tol)


# ---- 4. convergence --------------------------------------------------------------------------------------------------------------
def _example(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resident_loop_converges_on_targets():
    """examples/closed_loop_resident_headless.py on the 12 robots of test_closed_loop_converges_on_targets, under that test's
    assertions, thresholds unchanged."""
    r = _example("closed_loop_resident_headless").run(robots=12, ticks=2000, seed=0, verbose=False)
    assert np.all(np.isfinite(r["q"])) and np.all(np.isfinite(r["err"]))
    worst = r["err"].max(axis=1)
    assert r["err0"].max(axis=1).min() > 0.02
    assert (worst < 5e-3).mean() >= 0.75, np.sort(worst)
    assert np.median(worst) < 1e-3


def test_resident_loop_on_thousands_of_robots():
    """4 096 robots of closed_loop_headless.py's scenario, 2 000 ticks on the GPU: every robot finite, or frozen and flagged; the
    share of robots under 5 mm is not lower than the share the parent's host loop reaches on the first 256 of the same robots minus
    0.05 (sampling margin of 256 against 4 096); measured on an MI355X: 0.7939 on the GPU, 0.7969 on the host (profiles/rollout_rates.md).  ee_trace with trace_every = 100
    has 20 samples, and download_q + frontend + download_records(("ee_pose",)) reproduces what one more traced tick reports to 1e-12
    (the record-form front end and the fused walk are two kernels: not asserted bit for bit; the test prints whether they are)."""
    B, T = 4096, 2000
    mod = _example("closed_loop_resident_headless")
    q0, goal = mod.scenario(B, seed=0)
    tgt = ee_poses(goal)
    lay, gains, g, model, osc = make_ctx("k13", B)
    osc.set_plant(1e-3, 0.0)
    osc.upload_q(q0, np.zeros_like(q0))
    osc.set_targets(tgt)
    out = osc.rollout(T, trace_every=100)
    assert out["ee_trace"].shape == (20, B, 3, 7)
    qp, qv = osc.download_q()
    assert np.array_equal(qp, out["qpos"]) and np.array_equal(qv, out["qvel"])
    osc.frontend()
    ee = osc.download_records(keys=("ee_pose",))["ee_pose"]
    osc.upload_q(qp, qv)                 # (the front end left the coordinates alone; the targets are the slot's)
    more = osc.rollout(1, trace_every=1)
    osc.close()
    fin = np.isfinite(out["qpos"]).all(axis=1) & np.isfinite(out["qvel"]).all(axis=1)
    flagged = (out["flags_any"] & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD)) != 0
    assert np.all(fin | flagged)
    d = np.abs(more["ee_trace"][0] - ee)[fin]
    print(f"[thousands] traced tick against front end records: max |d ee_pose| = {d.max():.3g} (bit-identical: {bool(d.max() == 0.0)})")
    assert d.max() <= 1e-12
    worst = np.linalg.norm(ee[:, :2, :3] - tgt[:, :2, :3], axis=2).max(axis=1)
    share = float((worst[fin] < 5e-3).sum()) / B
    ref = host_loop(q0[:256], tgt[:256], T)
    worst_ref = np.linalg.norm(ee_poses(ref["q"])[:, :2, :3] - tgt[:256, :2, :3], axis=2).max(axis=1)
    share_ref = float((worst_ref < 5e-3).mean())
    print(f"[thousands] under 5 mm after {T} ticks: {share:.4f} of {B} robots on the GPU ({int((~fin).sum())} not finite, "
          f"{int(flagged.sum())} flagged); host loop on the first 256: {share_ref:.4f}; first 256 on the GPU: {float((worst[:256] < 5e-3).mean()):.4f}")
    assert share >= share_ref - 0.05, (share, share_ref)


# ---- 5. state rules ----------------------------------------------------------------------------------------------------------------
def _rc_rollout(osc, B, ticks=1, slot=0):
    return osc.lib.irlosc_rollout_from_q(osc._h, slot, B, ticks, 0, None, None, None)


def test_state_rules():
    B = 256
    lay = synth.make_layout("k13")
    _, gains, g = synth.make_batch("k13", B, seed=3)
    model = RigidBodyModel.load("dual_ur5")
    osc = BatchedOSC(lay, B, dtype=np.float64)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    pl = _lib.Plant(1e-3, 0.0, (1 << 25) - 1, 0)
    assert osc.lib.irlosc_set_plant(osc._h, C.byref(pl)) == ERR_STATE        # before set_model
    assert _rc_rollout(osc, B) == ERR_STATE
    assert "irlosc_set_model" in osc.lib.irlosc_last_error(osc._h).decode()
    osc.set_model(model)
    qpos, qvel = model.random_state(np.random.default_rng(9), B)
    osc.upload_q(qpos, qvel)
    osc.set_targets(g["tgt_pose"])
    assert _rc_rollout(osc, B) == ERR_STATE                                      # before set_plant
    assert "irlosc_set_plant" in osc.lib.irlosc_last_error(osc._h).decode()
    osc.set_plant(1e-3, 0.1)
    # a bad plant is refused and leaves the old one in force
    for bad in (_lib.Plant(0.0, 0.0, 1, 0), _lib.Plant(float("nan"), 0.0, 1, 0), _lib.Plant(1e-3, -1.0, 1, 0),
                _lib.Plant(1e-3, float("inf"), 1, 0), _lib.Plant(1e-3, 0.0, 1 << 25, 0), _lib.Plant(1e-3, 0.0, 1, 7)):
        assert osc.lib.irlosc_set_plant(osc._h, C.byref(bad)) == ERR_ARG
    a = osc.rollout(3)
    twin = BatchedOSC(lay, B, dtype=np.float64)
    twin.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    twin.set_model(model)
    twin.set_plant(1e-3, 0.1)
    twin.upload_q(qpos, qvel)
    twin.set_targets(g["tgt_pose"])
    assert all(np.array_equal(a[k], v) for k, v in twin.rollout(3).items() if v is not None)
    # after a rollout: no dense records; step_q works and equals a fresh context fed download_q's arrays
    assert osc.lib.irlosc_step(osc._h, 0, B, None, None) == ERR_STATE
    assert osc.lib.irlosc_download_records(osc._h, 0, B, None, None, None, None, None) == ERR_STATE
    qp, qv = osc.download_q()
    u = osc.step_q()
    twin.upload_q(qp, qv)
    assert np.array_equal(u, twin.step_q())
    # set_model clears the plant
    osc.set_model(model)
    assert _rc_rollout(osc, B) == ERR_STATE
    assert "irlosc_set_plant" in osc.lib.irlosc_last_error(osc._h).decode()
    osc.set_plant(1e-3, 0.1)
    # a slot lent to step_from_q_device holds no coordinates: no rollout, no download_q
    from conftest import HipBuffers
    hb = HipBuffers()
    try:
        d_q, d_v, d_t = hb.to_device(qpos), hb.to_device(qvel), hb.to_device(g["tgt_pose"])
        d_u, d_f = hb.alloc(B * 25 * 8), hb.alloc(B * 4)
        osc.step_from_q_device(B, d_q, d_v, d_t, d_u, d_f)
        osc.sync()
        assert _rc_rollout(osc, B) == ERR_STATE
        assert osc.lib.irlosc_download_q(osc._h, 0, B, None, None) == ERR_STATE
    finally:
        hb.free()
    assert _rc_rollout(osc, B + 1) == ERR_ARG and _rc_rollout(twin, B, ticks=0) == ERR_ARG
    osc.close()
    twin.close()


_FUSED_OFF = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
from irl_control_amd import BatchedOSC, synth
from irl_control_amd.rigid_body import RigidBodyModel
lay = synth.make_layout("k13")
_, gains, g = synth.make_batch("k13", 64, seed=3)
model = RigidBodyModel.load("dual_ur5")
osc = BatchedOSC(lay, 64, dtype=np.float64)
osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
osc.set_model(model)
osc.set_plant(1e-3)
qpos, qvel = model.random_state(np.random.default_rng(9), 64)
osc.upload_q(qpos, qvel)
osc.set_targets(g["tgt_pose"])
rc = osc.lib.irlosc_rollout_from_q(osc._h, 0, 64, 1, 0, None, None, None)
print("RESULT", rc, osc.lib.irlosc_last_error(osc._h).decode())
u = osc.step_q()
print("STEPQ", int(np.all(np.isfinite(u))))
"""


def test_no_rollout_without_the_fused_path():
    """IRLOSC_FUSED=0 (fresh child process): irlosc_rollout_from_q answers IRLOSC_ERR_STATE and names the reason; no second form."""
    r = subprocess.run([sys.executable, "-c", _FUSED_OFF.format(root=ROOT)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, IRLOSC_FUSED="0"), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split(" ", 2)
    assert int(res[1]) == ERR_STATE and "IRLOSC_FUSED=0" in res[2], res
    assert "STEPQ 1" in r.stdout


# ---- 6. frozen robots --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "mid_wave", "ragged_last"])
def test_a_robot_with_nan_is_frozen_and_alone(where):
    """A NaN in one robot's qvel (robot 0, one in the middle of a wave, the last robot of a ragged wave): its coordinates come back
    unchanged with NONFINITE in flags_any, every other robot is bit-equal to the run without it.  (A NaN input is data.)"""
    B, T = 1000, 5
    bad = dict(first=0, mid_wave=64 * 3 + 29, ragged_last=B - 1)[where]
    lay, gains, g, model, osc = make_ctx("k13", B, seed=8)
    qpos, qvel = model.random_state(np.random.default_rng(31), B)
    osc.set_plant(1e-3, 0.0)
    osc.upload_q(qpos, qvel)
    osc.set_targets(g["tgt_pose"])
    clean = osc.rollout(T)
    qv = qvel.copy()
    qv[bad, 4] = np.nan
    osc.upload_q(qpos, qv)
    out = osc.rollout(T)
    osc.close()
    others = np.arange(B) != bad
    for key in ("qpos", "qvel", "u", "flags_any"):
        assert np.array_equal(out[key][others], clean[key][others]), key
    assert np.array_equal(out["qpos"][bad], qpos[bad])
    assert np.array_equal(out["qvel"][bad], qv[bad], equal_nan=True)
    assert out["flags_any"][bad] & _lib.FLAG_NONFINITE
    assert not np.any(clean["flags_any"] & _lib.FLAG_NONFINITE)


# ---- 7. nothing else moved ---------------------------------------------------------------------------------------------------------
def test_a_plant_that_never_rolls_out_changes_nothing():
    B = 4096
    res = []
    for with_plant in (False, True):
        lay, gains, g, model, osc = make_ctx("k13", B, seed=12, n_slots=2)
        if with_plant:
            osc.set_plant(1e-3, 0.3, actuated_joints())
        qpos, qvel = model.random_state(np.random.default_rng(55), B)
        for sl in range(2):
            osc.upload_q(qpos, qvel, slot=sl)
            osc.set_targets(g["tgt_pose"], slot=sl)
        names = (osc.from_q_name, osc.kernel_name)
        u, fl = osc.step_q(return_flags=True)
        osc.step_resident_from_q(16)
        u2, fl2 = osc.download()
        res.append((names, u, fl, u2, fl2))
        osc.close()
    assert res[0][0] == res[1][0]
    for x, y in zip(res[0][1:], res[1][1:]):
        assert np.array_equal(x, y)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--host-loop":
        q0_, goal_ = box_scenario()
        np.savez(sys.argv[2], q=host_loop(q0_, ee_poses(goal_), 300, tile=4)["q"])
