#!/usr/bin/env python3
"""Rates of the path from joint coordinates with and without the F/T sensor feed (k12 + admittance by default):
    (a) irlosc_step_resident_from_q, no feed
    (b) the same with a sensor feed on every slot (one osc_ft_wrench launch per train between the walk and the OSC step)
    (c) irlosc_step_from_q_device once per tick on resident caller buffers, HIP events on the caller's stream around the ticks
    (d) the host-fed tick: upload_q + set_targets + set_sensordata + step_from_q + download
    python tools/fromq_feed_rates.py [--batch 65536] [--slots 16] [--steps 128] [--reps 3] [--legs abcd] [--json out.json]
Prints one line per leg and, last, a JSON line with every rate in steps/s (best of --reps)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from irl_control_amd import BatchedOSC, _lib, synth                 # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--slots", type=int, default=16)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layout", default="k12_admit")
ap.add_argument("--legs", default="abcd")
ap.add_argument("--host-ticks", type=int, default=10)
ap.add_argument("--json", default=None)
a = ap.parse_args()
B, NS = a.batch, 18
lay = synth.make_layout(a.layout)
model = RigidBodyModel.load("dual_ur5")
rng = np.random.default_rng(5)
osc = BatchedOSC(lay, B, dtype=np.float64, n_slots=a.slots, kernel=_lib.KERNEL_ROW16)
osc.set_model(model)
osc.set_ft_sensors()
_, gains, arr = synth.make_batch(a.layout, B, seed=7)
osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
states = []
for s in range(a.slots):
    q, qd = model.random_state(rng, B)
    osc.upload_q(q, qd, slot=s)
    osc.set_targets(arr["tgt_pose"], slot=s)
    states.append((q, qd))
sens = rng.normal(0.0, 5.0, size=(B, NS))
print(osc.from_q_name, flush=True)
out = dict(batch=B, slots=a.slots, layout=a.layout, steps=a.steps)


def resident(tag):
    osc.step_resident_from_q(16)                       # warm-up (banks, exchange buffers)
    best = min(osc.step_resident_from_q(a.steps)[1] for _ in range(a.reps))
    out[tag] = B / (best * 1e-3)
    print(f"({tag}) {best * 1e3:8.1f} us per step, {out[tag] / 1e6:7.1f} M steps/s", flush=True)


if "a" in a.legs:
    resident("a_resident_no_feed")
if "b" in a.legs:
    for s in range(a.slots):
        osc.set_sensordata(sens, slot=s)
    resident("b_resident_feed")
if "c" in a.legs:
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [vp]
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamSynchronize.argtypes = [vp]
    hip.hipStreamDestroy.argtypes = [vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    ptrs = []

    def dev(arr_):
        arr_ = np.ascontiguousarray(arr_)
        p = vp()
        assert hip.hipMalloc(C.byref(p), arr_.nbytes) == 0
        assert hip.hipMemcpy(p, arr_.ctypes.data_as(vp), arr_.nbytes, 1) == 0
        ptrs.append(p)
        return p
    q, qd = states[0]
    dq, dv, dt, ds = dev(q), dev(qd), dev(np.ascontiguousarray(arr["tgt_pose"], dtype=np.float64)), dev(sens)
    du, dfl = dev(np.zeros((B, lay.n))), dev(np.zeros(B, np.uint32))
    st, e0, e1 = vp(), vp(), vp()
    assert hip.hipStreamCreate(C.byref(st)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    scratch = a.slots - 1
    for _ in range(4):
        osc.step_from_q_device(B, dq, dv, dt, du, dfl, d_sensordata=ds, slot=scratch, stream=st)
    assert hip.hipStreamSynchronize(st) == 0
    best = None
    for _ in range(a.reps):
        hip.hipEventRecord(e0, st)
        for _ in range(a.steps):
            osc.step_from_q_device(B, dq, dv, dt, du, dfl, d_sensordata=ds, slot=scratch, stream=st)
        hip.hipEventRecord(e1, st)
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), e0, e1)
        best = ms.value / a.steps if best is None else min(best, ms.value / a.steps)
    out["c_device_entry_feed"] = B / (best * 1e-3)
    print(f"(c) {best * 1e3:8.1f} us per step, {out['c_device_entry_feed'] / 1e6:7.1f} M steps/s (one step per call, one stream)", flush=True)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1); hip.hipStreamDestroy(st)
    for p in ptrs:
        hip.hipFree(p)
    osc.upload_q(*states[scratch], slot=scratch)
if "d" in a.legs:
    q, qd = states[0]
    tgt = arr["tgt_pose"]
    osc.step_from_q(q, qd, tgt, sensordata=sens)
    best = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(a.host_ticks):
            osc.step_from_q(q, qd, tgt, sensordata=sens)
        dtk = (time.perf_counter() - t0) / a.host_ticks
        best = dtk if best is None else min(best, dtk)
    out["d_host_fed_tick"] = B / best
    print(f"(d) {best * 1e6:8.1f} us per tick, {out['d_host_fed_tick'] / 1e6:7.1f} M steps/s (PCIe both ways, synchronous)", flush=True)
osc.close()
if "a_resident_no_feed" in out and "b_resident_feed" in out:
    out["b_over_a"] = out["b_resident_feed"] / out["a_resident_no_feed"]
if "a_resident_no_feed" in out and "c_device_entry_feed" in out:
    out["c_over_a"] = out["c_device_entry_feed"] / out["a_resident_no_feed"]
print(json.dumps(out), flush=True)
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
