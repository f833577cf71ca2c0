"""``BatchedOSC``: many independent robot instances per control tick through libirlosc.

This is the batch-of-B form of ``OSC.generate`` (/root/reference/irl_control/osc.py:120-210): the
same inputs the reference assembles per tick (M, stacked J, dq, bias, EE poses, targets, wrench),
with a leading batch axis, in; joint torques ``u_all`` [B, n] out.  All arithmetic happens in the
HIP kernels; this class only owns the context and checks shapes.
"""
import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .layout import OSCLayout, pack_gains


class BatchedOSC:
    def __init__(self, layout: OSCLayout, max_batch: int, dtype=np.float64, hip_device: int = 0,
                 n_slots: int = 1, kernel: int = _lib.KERNEL_AUTO):
        self.lib = _lib.load()
        self.layout = layout
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        self.max_batch, self.n_slots = int(max_batch), int(n_slots)
        code = _lib.F64 if self.dtype == np.float64 else _lib.F32
        cfg = layout.to_cfg(code, self.max_batch, hip_device, self.n_slots, kernel)
        h = C.c_void_p()
        rc = self.lib.irlosc_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise _lib.IrloscError(f"irlosc_create failed ({rc}): "
                                   f"{self.lib.irlosc_last_error(None).decode()}")
        self._h = h
        self._B = [0] * self.n_slots
        self._joint_rows = [0] * self.n_slots      # rows of each slot's set_joints (the width of joint_state's arrays)
        self._episode_records = [1] * self.n_slots      # ring length of each slot's set_episodes (the width of episode_state's records)
        self._objects = [(0, 0)] * self.n_slots      # (objects, mates) of each slot's set_objects (the widths of object_state's arrays)
        self._policy = [None] * self.n_slots      # (n_in, n_out, keep_obs) of each slot's set_policy (the widths of policy_state's arrays)
        self._grippers = [0] * self.n_slots          # ... and its grippers (the width of object_load_state's)
        if kernel == _lib.KERNEL_AUTO and self.max_batch >= 1024 and self.kernel_class == _lib.CLASS_GENERIC:
            import warnings
            warnings.warn(f"layout (n={layout.n}, k={layout.k}, ndev={layout.ndev}) has no throughput kernel: "
                          f"{self.kernel_name} (one wavefront per instance, ~25x slower than osc_row16 at this batch size); "
                          "the row16 kernels take every layout of an n=25 robot (k <= 16, ndev <= 4)", RuntimeWarning, stacklevel=2)

    # -- plumbing ---------------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise _lib.IrloscError(f"libirlosc error {rc}: {self.lib.irlosc_last_error(self._h).decode()}")

    def _arr(self, a, shape, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.shape != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {a.shape}")
        return a

    @staticmethod
    def _check_symmetric(M):
        """The throughput kernels read rows of M as columns (include/irlosc.h): refuse an asymmetric inertia matrix."""
        asym = np.abs(M - np.swapaxes(M, 1, 2)).max(axis=(1, 2))
        scale = np.abs(M).max(axis=(1, 2))
        bad = np.nonzero(asym > 1e-6 * np.maximum(scale, 1e-300))[0]
        if len(bad):
            raise ValueError(f"M of instance {int(bad[0])} is not symmetric (max |M - M^T| = {asym[bad[0]]:.3g})")

    @property
    def kernel_name(self) -> str:
        return self.lib.irlosc_kernel_name(self._h).decode()

    @property
    def kernel_class(self) -> int:
        """_lib.CLASS_GENERIC / CLASS_ROW16 (an instantiation for exactly this layout) / CLASS_ROW16_PADDED (row16 kernel of the
        next tier KMAX >= k, k and ndev at run time) / CLASS_GROUP: irlosc_kernel_class."""
        return int(self.lib.irlosc_kernel_class(self._h))

    @property
    def frontend_name(self) -> str:
        """Kernel `frontend()` launches: the lane-per-robot one when the model has the compiled Dual-UR5 shape, else the generic one."""
        return self.lib.irlosc_frontend_name(self._h).decode()

    def close(self):
        if getattr(self, "_h", None):
            self.lib.irlosc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- API ---------------------------------------------------------------------------------------
    def set_gains(self, kp, kv, ko, k, d, max_vel, null_kv=0.0):
        g, nk, nb = pack_gains(self.layout, kp, kv, ko, k, d, max_vel, null_kv)
        if nb not in (1, self.max_batch):
            raise ValueError(f"per-instance gains need a leading axis of max_batch={self.max_batch}")
        last = getattr(self, "_gains_sent", None)      # a per-tick caller re-sends the same gains: skip the copy then
        if last is not None and last[2] == nb and np.array_equal(last[0], g) and np.array_equal(last[1], nk):
            return
        self._chk(self.lib.irlosc_set_gains(self._h, _lib.ptr(g), _lib.ptr(nk), nb))
        self._gains_sent = (g.copy(), nk.copy(), nb)

    def upload(self, M, J, dq, bias, ee_pose, wrench=None, slot: int = 0, check_symmetric: bool = False):
        """Records of B robots into resident slot `slot`.  On the throughput kernels the library itself refuses an asymmetric M
        (device-side probe, IrloscError); check_symmetric=True additionally checks on the host before anything is copied."""
        L = self.layout
        B = int(np.shape(M)[0])
        M = self._arr(M, (B, L.n, L.n), "M")
        if check_symmetric:
            self._check_symmetric(M)
        J = self._arr(J, (B, L.k, L.n), "J")
        dq = self._arr(dq, (B, L.n), "dq")
        bias = self._arr(bias, (B, L.n), "bias")
        ee = self._arr(ee_pose, (B, L.ndev, 7), "ee_pose")
        wr = self._arr(wrench, (B, L.ndev, 6), "wrench")
        self._chk(self.lib.irlosc_upload(self._h, slot, B, _lib.ptr(M), _lib.ptr(J), _lib.ptr(dq),
                                         _lib.ptr(bias), _lib.ptr(ee), _lib.ptr(wr)))
        self._B[slot] = B

    def upload_raw(self, desc, qM, qvel, qfrc_bias, jacp, jacr, ee_xpos, ee_xquat, site_xmat=None, sensordata=None,
                   slot: int = 0, qm_layout=None):
        """Raw simulator arrays in, state assembly on the GPU (see raw.py / irlosc_upload_raw).  `desc` from
        raw.raw_desc(); arrays batch-major: qM[B,nv,nv], qvel[B,nv], qfrc_bias[B,nv], jacp/jacr[B,ndev,3,nv],
        ee_xpos[B,ndev,3], ee_xquat[B,ndev,4], site_xmat[B,ndev,9], sensordata[B,n_sensor].
        With `qm_layout` (raw.qm_layout(dof_parentid[, dof_Madr])) qM is mjData.qM as MuJoCo holds it, [B, nM]: mj_fullM's expansion
        (robot.py:68-72) then runs on the GPU (irlosc_upload_raw_sparse)."""
        L = self.layout
        B, nv, ns = int(np.shape(qM)[0]), int(desc.nv), int(desc.n_sensor)
        if qm_layout is not None:
            a = [self._arr(qM, (B, int(qm_layout.nM)), "qM (sparse)"), self._arr(qvel, (B, nv), "qvel"), self._arr(qfrc_bias, (B, nv), "qfrc_bias"),
                 self._arr(jacp, (B, L.ndev, 3, nv), "jacp"), self._arr(jacr, (B, L.ndev, 3, nv), "jacr"),
                 self._arr(ee_xpos, (B, L.ndev, 3), "ee_xpos"), self._arr(ee_xquat, (B, L.ndev, 4), "ee_xquat"),
                 self._arr(site_xmat, (B, L.ndev, 9), "site_xmat"), self._arr(sensordata, (B, ns), "sensordata")]
            self._chk(self.lib.irlosc_upload_raw_sparse(self._h, slot, B, C.byref(desc), C.byref(qm_layout), *[_lib.ptr(x) for x in a]))
            self._B[slot] = B
            return
        a = [self._arr(qM, (B, nv, nv), "qM"), self._arr(qvel, (B, nv), "qvel"), self._arr(qfrc_bias, (B, nv), "qfrc_bias"),
             self._arr(jacp, (B, L.ndev, 3, nv), "jacp"), self._arr(jacr, (B, L.ndev, 3, nv), "jacr"),
             self._arr(ee_xpos, (B, L.ndev, 3), "ee_xpos"), self._arr(ee_xquat, (B, L.ndev, 4), "ee_xquat"),
             self._arr(site_xmat, (B, L.ndev, 9), "site_xmat"), self._arr(sensordata, (B, ns), "sensordata")]
        self._chk(self.lib.irlosc_upload_raw(self._h, slot, B, C.byref(desc), *[_lib.ptr(x) for x in a]))
        self._B[slot] = B

    def set_targets(self, tgt_pose, tgt_vel=None, slot: int = 0):
        L = self.layout
        B = int(np.shape(tgt_pose)[0])
        if self._B[slot] and B != self._B[slot]:
            raise ValueError(f"slot {slot} holds {self._B[slot]} instances, targets given for {B}")
        tp = self._arr(tgt_pose, (B, L.ndev, 7), "tgt_pose")
        tv = self._arr(tgt_vel, (B, L.ndev, 6), "tgt_vel")
        self._chk(self.lib.irlosc_set_targets(self._h, slot, B, _lib.ptr(tp), _lib.ptr(tv)))

    def step(self, slot: int = 0, return_flags: bool = False):
        B = self._B[slot]
        u = np.empty((B, self.layout.n), dtype=self.dtype)
        fl = np.empty(B, dtype=np.uint32)
        self._chk(self.lib.irlosc_step(self._h, slot, B, _lib.ptr(u), _lib.ptr(fl)))
        return (u, fl) if return_flags else u

    def step_resident(self, iters: int, first_slot: int = 0, B: Optional[int] = None):
        """-> (ms_total, ms_kernel_avg): `iters` launches on resident data, HIP-event timed."""
        B = self._B[first_slot] if B is None else B
        t, a = C.c_float(), C.c_float()
        self._chk(self.lib.irlosc_step_resident(self._h, first_slot, B, iters, C.byref(t), C.byref(a)))
        return t.value, a.value

    def time_dominant_kernel(self, iters: int, slot: int = 0, B: Optional[int] = None) -> float:
        """Mean duration (ms) of the dominant kernel alone over `iters` launches (roofline support)."""
        B = self._B[slot] if B is None else B
        a = C.c_float()
        self._chk(self.lib.irlosc_time_dominant_kernel(self._h, slot, B, iters, C.byref(a)))
        return a.value

    def time_trains(self, ntrains: int, first_slot: int = 0, B: Optional[int] = None, from_q: bool = False) -> np.ndarray:
        """Untraced timing of `ntrains` consecutive trains (irlosc_time_trains): -> [ntrains, 4] = (HIP event pair of the train in
        ms, start of its first wave, end of its last wave in microseconds of the kernels' own 100 MHz clock since train 0, shader
        clock in MHz seen by a sample wave of the train)."""
        B = self._B[first_slot] if B is None else B
        out = np.zeros((int(ntrains), 4), dtype=np.float64)
        self._chk(self.lib.irlosc_time_trains(self._h, first_slot, B, int(ntrains), 1 if from_q else 0, _lib.ptr(out)))
        return out

    def giveup_counts(self) -> np.ndarray:
        """Instances the steps of the most recent train (a plain step: entry 0) handed to the generic kernel's Jacobi solve
        (irlosc_giveup_counts): same results, but a serial tail -- watch it when task sets can lose more than three directions."""
        out = np.zeros(8, dtype=np.int32)
        self._chk(self.lib.irlosc_giveup_counts(self._h, _lib.ptr(out)))
        return out

    @property
    def steps_per_launch(self) -> int:
        """Steps chained into one launch by step_resident / time_dominant_kernel (1 on the generic path)."""
        n = int(self.lib.irlosc_steps_per_launch(self._h))
        if n < 1:
            raise _lib.IrloscError(f"libirlosc error {n}")
        return n

    def download(self, B: Optional[int] = None):
        B = self._B[0] if B is None else B
        u = np.empty((B, self.layout.n), dtype=self.dtype)
        fl = np.empty(B, dtype=np.uint32)
        self._chk(self.lib.irlosc_download(self._h, B, _lib.ptr(u), _lib.ptr(fl)))
        return u, fl

    # -- rigid-body front end: joint coordinates in, records assembled on the GPU ------------------------------------
    def set_model(self, model, ee_bodies=None):
        """`model`: rigid_body.RigidBodyModel; `ee_bodies`: EE body name per target device (targets order), default the
        Dual-UR5 map."""
        from .rigid_body import DUAL_UR5_EE
        names = ee_bodies if ee_bodies is not None else [DUAL_UR5_EE[d] for d in self.layout.dev_names]
        st = model.to_struct(list(names))
        self._chk(self.lib.irlosc_set_model(self._h, C.byref(st)))
        self._model = model
        self._joint_rows = [0] * self.n_slots      # (irlosc_set_model ends every slot's joint rows)
        self._objects = [(0, 0)] * self.n_slots    # (... and action objects)
        self._grippers = [0] * self.n_slots

    def upload_q(self, qpos, qvel, slot: int = 0):
        B = int(np.shape(qpos)[0])
        qp = np.ascontiguousarray(qpos, dtype=np.float64)
        qv = np.ascontiguousarray(qvel, dtype=np.float64)
        if qp.shape != (B, self.layout.n) or qv.shape != (B, self.layout.n):
            raise ValueError(f"qpos / qvel: expected shape {(B, self.layout.n)}")
        self._chk(self.lib.irlosc_upload_q(self._h, slot, B, _lib.ptr(qp), _lib.ptr(qv)))
        self._B[slot] = B

    def frontend(self, slot: int = 0):
        """(qpos, qvel) of the slot -> its M, J, dq, bias, ee_pose records (on the GPU)."""
        self._chk(self.lib.irlosc_frontend(self._h, slot, self._B[slot]))

    def download_records(self, slot: int = 0, keys=("M", "J", "dq", "bias", "ee_pose")):
        """-> dict of the slot's records as they sit in HBM (uploaded, or assembled by the front end); `keys` picks which
        ones cross PCIe (a per-tick caller that only needs the EE poses asks for ("ee_pose",): 168 B instead of 8.5 KB per robot)."""
        L, B = self.layout, self._B[slot]
        shapes = dict(M=(B, L.n, L.n), J=(B, L.k, L.n), dq=(B, L.n), bias=(B, L.n), ee_pose=(B, L.ndev, 7))
        out = {k: np.empty(shapes[k], self.dtype) for k in keys}
        self._chk(self.lib.irlosc_download_records(self._h, slot, B, *[_lib.ptr(out.get(k)) for k in ("M", "J", "dq", "bias", "ee_pose")]))
        return out

    def slot_structure(self, slot: int = 0) -> bool:
        """True when the records in `slot` carry the zero pattern of the Dual-UR5 tree and the fp64 row16 kernel therefore
        factors M in the tree-structured form (irlosc_slot_structure, include/irlosc.h)."""
        return bool(self.lib.irlosc_slot_structure(self._h, slot))

    def slot_route(self, slot: int = 0, B: Optional[int] = None) -> str:
        """Which kernels a step of B instances (default: the slot's) on `slot` runs (irlosc_slot_route, include/irlosc.h): "lane"
        (the lane-per-robot OSC step on the slot's compact block), "row16_tree", "row16", "generic" or "none"."""
        rc = self.lib.irlosc_slot_route(self._h, slot, 0 if B is None else B)
        return {_lib.ROUTE_GENERIC: "generic", _lib.ROUTE_ROW16: "row16", _lib.ROUTE_ROW16_TREE: "row16_tree",
                _lib.ROUTE_LANE: "lane"}.get(rc, "none")

    def probe_structure(self, slot: int = 0, B: Optional[int] = None) -> bool:
        """Look at the records already in `slot` (irlosc_probe_structure): what assemble_device on a caller's stream cannot
        do for itself.  -> the slot's verdict, as slot_structure() reports it from then on."""
        rc = self.lib.irlosc_probe_structure(self._h, slot, self._B[slot] if B is None else B)
        if rc < 0:
            self._chk(rc)
        return bool(rc)

    @property
    def from_q_name(self) -> str:
        """What step_from_q / step_resident_from_q launch: the fused pair (compact exchange buffer, no dense M / J) when the
        model has the compiled Dual-UR5 shape and the context runs the fp64 row16 kernel, else front end + step."""
        return self.lib.irlosc_from_q_name(self._h).decode()

    def step_q(self, slot: int = 0, return_flags: bool = False):
        """One step from the slot's resident (qpos, qvel) and targets (irlosc_step_from_q)."""
        B = self._B[slot]
        u = np.empty((B, self.layout.n), dtype=self.dtype)
        fl = np.empty(B, dtype=np.uint32)
        self._chk(self.lib.irlosc_step_from_q(self._h, slot, B, _lib.ptr(u), _lib.ptr(fl)))
        return (u, fl) if return_flags else u

    def step_from_q(self, qpos, qvel, tgt_pose, tgt_vel=None, return_flags: bool = False, sensordata=None):
        """One tick from joint coordinates: upload (qpos, qvel) and the targets (and, with `sensordata` [B, n_sensor], the F/T
        readings of this tick: set_sensordata), one step from them, download."""
        self.upload_q(qpos, qvel)
        self.set_targets(tgt_pose, tgt_vel)
        if sensordata is not None:
            self.set_sensordata(sensordata)
        return self.step_q(return_flags=return_flags)

    # -- F/T sensor feed of the steps from joint coordinates (irlosc_set_ft_sensors / irlosc_set_sensordata) ---------------
    def set_ft_sensors(self, sites=None, n_sensor: int = 18):
        """Describe the F/T sensors of the target devices (after set_model; irlosc_set_ft_sensors).  Default: device d's site is
        ft_frame_<name> of the model's `sites` table (the reference's F/T frames) and its sensordata slices those of device._FT_TABLE (as
        raw.raw_desc); `sites` maps a device name to another site.  Devices without an entry have no sensor (zero wrench).  The site's body
        must be welded to the device's EE body (the library checks).  n_sensor = 18: the scene's <sensor> block."""
        model = getattr(self, "_model", None)
        if model is None:
            raise _lib.IrloscError("set_model must precede set_ft_sensors")
        fd = model.ft_desc(self.layout.dev_names, sites, n_sensor)
        self._chk(self.lib.irlosc_set_ft_sensors(self._h, C.byref(fd)))
        self._n_sensor = int(n_sensor)

    def set_sensordata(self, sensordata, slot: int = 0):
        """F/T readings sensordata[B, n_sensor] (float64, MuJoCo's sensordata rows) of slot `slot`: the wrench source of every step from
        joint coordinates on it until the slot gets records again (upload*) or the feed is cleared (sensordata=None)."""
        if sensordata is None:
            self._chk(self.lib.irlosc_set_sensordata(self._h, slot, 0, None))
            return
        ns = getattr(self, "_n_sensor", None)
        if ns is None:
            raise _lib.IrloscError("set_ft_sensors must precede set_sensordata")
        sd = np.ascontiguousarray(sensordata, dtype=np.float64)
        if sd.ndim != 2 or sd.shape[1] != ns:
            raise ValueError(f"sensordata: expected shape (B, {ns}), got {sd.shape}")
        self._chk(self.lib.irlosc_set_sensordata(self._h, slot, int(sd.shape[0]), _lib.ptr(sd)))

    def step_from_q_device(self, B: int, d_qpos: int, d_qvel: int, d_tgt_pose: int, d_u: int, d_flags: int, d_tgt_vel: int = None,
                           d_sensordata: int = None, slot: int = 0, stream: int = None):
        """One step from joint coordinates on caller-owned DEVICE arrays (irlosc_step_from_q_device): integer device addresses
        (e.g. tensor.data_ptr()) of qpos / qvel [B, n] float64, tgt_pose [B, ndev, 7] (and tgt_vel [B, ndev, 6]) in this context's
        dtype, sensordata [B, n_sensor] float64 or None, outputs u [B, n] (context dtype) and flags [B] uint32.  Enqueued on `stream`
        (a hipStream_t address; None = the context's stream), nothing copied, nothing synchronised.  `slot` lends its buffers as
        scratch and holds no records and no joint coordinates afterwards."""
        self._chk(self.lib.irlosc_step_from_q_device(self._h, slot, int(B), d_qpos, d_qvel, d_tgt_pose, d_tgt_vel, d_sensordata,
                                                     d_u, d_flags, stream))

    # -- closed loops on the GPU: a contact-free plant behind the fused step (irlosc_set_plant / irlosc_rollout_from_q) ------------
    def set_plant(self, dt: float, damping: float = 0.0, actuated=None):
        """The plant of `rollout` (after set_model): qacc = M^-1 (u - bias - damping qvel), semi-implicit Euler with step `dt`.
        `actuated`: indices of the joints driven by u (default: all n, as examples/closed_loop_headless.py; the others see u = 0).
        No contacts (but the penalty walls of set_walls); joint limits, the gripper's equality rows and a driven gripper only as
        the penalty rows of set_joints (irlosc_set_joints).  set_model clears it."""
        n = self.layout.n
        idx = list(range(n)) if actuated is None else [int(j) for j in actuated]
        if any(j < 0 or j >= n for j in idx):
            raise ValueError(f"actuated: joint indices must lie in [0, {n})")
        mask = 0
        for j in idx:
            mask |= 1 << j
        pl = _lib.Plant(float(dt), float(damping), mask, 0)
        self._chk(self.lib.irlosc_set_plant(self._h, C.byref(pl)))

    def rollout(self, ticks: int, trace_every: int = 0, slot: int = 0):
        """`ticks` closed-loop ticks on the slot's resident robots without the host in between (irlosc_rollout_from_q): per tick
        the fused step from the slot's coordinates towards its targets, then the plant kernel advances the coordinates.
        -> dict(qpos, qvel: the coordinates afterwards; u: the last tick's torques; flags_any: OR of all ticks' flags;
        ee_trace[ceil(ticks / trace_every), B, ndev, 7]: EE poses at the start of every trace_every-th tick, or None)."""
        L, B = self.layout, self._B[slot]
        ticks, trace_every = int(ticks), int(trace_every)
        u = np.empty((B, L.n), dtype=self.dtype)
        fl = np.empty(B, dtype=np.uint32)
        tr = np.empty((-(-ticks // trace_every), B, L.ndev, 7), dtype=np.float64) if trace_every > 0 and ticks > 0 else None
        self._chk(self.lib.irlosc_rollout_from_q(self._h, slot, B, ticks, trace_every, _lib.ptr(tr), _lib.ptr(u), _lib.ptr(fl)))
        run = self._ticks_run(slot)
        if tr is not None and run < ticks:
            tr = tr[:-(-run // trace_every)]
        qpos, qvel = self.download_q(slot)
        return dict(qpos=qpos, qvel=qvel, u=u, flags_any=fl, ee_trace=tr, ticks_run=run)

    def _log_policy(self, slot: int):
        """(n_out, sampled) of the slot as the library's log sees it: the policy in force (0: none) and whether it has a Gaussian head.
        Asked of the library: other programs' setters, set_targets and set_model end a policy behind this object's back."""
        if self._policy[slot] is None or self.lib.irlosc_download_policy_state(self._h, slot, 0, None, None, None, None, None) != 0:
            return 0, False
        sampled = self.lib.irlosc_download_policy_noise_state(self._h, slot, 0, None, None, None, None) == 0
        return self._policy[slot][1], sampled

    def _log_reward(self, slot: int) -> bool:
        """Whether the slot has a reward as the library's log sees it (set_model ends one behind this object's back)."""
        return self.lib.irlosc_download_reward_state(self._h, slot, 0, None, None, None, None, None, None, None) == 0

    def _ticks_run(self, slot: int) -> int:
        """The ticks the slot's last rollout call ran: fewer than asked where its episodes exited early (set_episodes, poll_every)."""
        run = C.c_int32(0)
        self._chk(self.lib.irlosc_download_episode_state(self._h, slot, 0, None, None, None, None, None, C.byref(run)))
        return int(run.value)

    def rollout_logged(self, ticks: int, channels, every: int = 1, robots=None, slot: int = 0, buffer_bytes: int = 0):
        """`rollout` with an episode log (irlosc_rollout_from_q_logged): on ticks 0, every, 2 every, ... of this call the `channels`
        (names of rollout_log.CHANNELS, or an OR of their bits) of `robots` (strictly ascending indices; None: all B) are gathered on
        the GPU and drained to the host while the following ticks run.  channels=None runs the entry point without a log.
        -> `rollout`'s dict (ee_trace None) plus log: dict of named arrays [S, R, ...] (rollout_log.split) and log_ticks: the S ticks
        they belong to.  `buffer_bytes`: the device ring (0: 256 MiB; else at least two samples)."""
        from . import rollout_log
        L, B = self.layout, self._B[slot]
        ticks = int(ticks)
        u = np.empty((B, L.n), dtype=self.dtype)
        fl = np.empty(B, dtype=np.uint32)
        lg = idx = buf = None
        log, log_ticks = None, None
        if channels is not None:
            m = rollout_log.mask(channels)
            every = int(every)
            if robots is not None:
                idx = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
            R = B if idx is None else len(idx)
            lg = _lib.Log(m & 0xFFFFFFFF, every, 0 if idx is None else R, 0, int(buffer_bytes))
            S = -(-ticks // every) if every > 0 and ticks > 0 else 0
            words = 0
            nobj = self._objects[slot][0]
            n_out, sampled = self._log_policy(slot)
            rewarded = self._log_reward(slot)
            if S and R >= 1 and m and not m & ~rollout_log.known(nobj, n_out, sampled, rewarded):
                words = rollout_log.layout(L.n, L.ndev, m, R, nobj, n_out, sampled, rewarded)[1]
            buf = np.empty((S, words), dtype=np.float64)
        self._chk(self.lib.irlosc_rollout_from_q_logged(self._h, slot, B, ticks, C.byref(lg) if lg is not None else None, _lib.ptr(idx),
                                                        _lib.ptr(buf), _lib.ptr(u), _lib.ptr(fl)))
        run = self._ticks_run(slot)
        if buf is not None:
            log_ticks = np.arange(0, min(ticks, run) if B else ticks, every, dtype=np.int64)      # (an early exit: the rows of the ticks run)
            log = rollout_log.split(buf[:len(log_ticks)], L.n, L.ndev, m, R, dtype=self.dtype, nobj=nobj, n_out=n_out, sampled=sampled, rewarded=rewarded) if B else {}
        qpos, qvel = self.download_q(slot)
        return dict(qpos=qpos, qvel=qvel, u=u, flags_any=fl, ee_trace=None, log=log, log_ticks=log_ticks, ticks_run=run)

    # -- the reward of the rollout (irlosc_set_reward / irlosc_download_reward_state) ---------------------------------------------------
    def set_reward(self, reward, slot: int = 0):
        """A reward for the slot's robots (irlosc_set_reward; "a reward per tick" in include/irlosc.h), evaluated on the GPU on every
        rollout tick behind the OSC step: `reward` is a reward.Reward -- up to 8 weighted terms over the tick's EE poses, targets,
        object poses, fixed points, the policy's action, the torques, the sensed force and the mates -- accumulated per episode plain
        (ret) and discounted (gret; gamma), optionally with a goal: a term's value compared with goal_value for goal_hold ticks in a
        row.  With episodes (set_episodes, end_on_finish) a robot that has reached the goal ends its episode, whose outcome carries
        _lib.EPISODE_GOAL and whose (ret, gret) reward_state keeps.  The log's "reward" channel is [R, 4]: r, ret, steps, goal.  The
        arithmetic is reward.reward_tick's, bit for bit.  After the parts it names (targets, objects, policy, feed), before
        set_episodes; reward=None (or clear_reward) ends it and nothing else."""
        B = self._B[slot]
        if reward is None:
            self._chk(self.lib.irlosc_set_reward(self._h, slot, B, None, None))
            return
        desc = reward.desc()
        pts = None
        if reward.points is not None:
            pts = np.ascontiguousarray(reward.points, dtype=np.float64)
            if pts.ndim == 3 and pts.shape[0] != B:
                raise ValueError(f"points: expected shape (P, 3) or ({B}, P, 3), got {pts.shape}")
        self._chk(self.lib.irlosc_set_reward(self._h, slot, B, C.byref(desc), _lib.ptr(pts)))

    def clear_reward(self, slot: int = 0):
        """Ends the slot's reward (irlosc_set_reward with desc == NULL); everything else is left alone."""
        self.set_reward(None, slot=slot)

    def reward_state(self, slot: int = 0):
        """-> dict(r: the last tick's reward; ret, gret: the running episode's plain and discounted sums; steps, hold, goal_step (-1:
        not reached): [B]; records [B, 16, 2]: (ret, gret) of the robot's ended episodes, entry e mod the episodes' `records` as
        episode_state has them, zero where no episode ended under this reward).  (irlosc_download_reward_state)"""
        B = self._B[slot]
        out = dict(r=np.empty(B), ret=np.empty(B), gret=np.empty(B), steps=np.empty(B, np.int32), hold=np.empty(B, np.int32),
                   goal_step=np.empty(B, np.int32), records=np.empty((B, _lib.MAX_EPISODE_RECORDS, 2)))
        self._chk(self.lib.irlosc_download_reward_state(self._h, slot, B, *(_lib.ptr(out[k]) for k in ("r", "ret", "gret", "steps", "hold", "goal_step", "records"))))
        return out

    # -- episodes of the rollout (irlosc_set_episodes / irlosc_download_episode_state) ------------------------------------------------
    def set_episodes(self, qpos0, qvel0=None, max_ticks: int = 0, end_on_finish: bool = True, max_episodes: int = 0, poses=None,
                     records: int = 4, poll_every: int = 0, slot: int = 0):
        """Episodes for the slot's robots, ended and restarted on the GPU by `rollout` / `rollout_logged`: a robot whose list or
        non-looping paths are through (`end_on_finish`) or that has run `max_ticks` ticks (0: no limit) gets its record written and starts
        over -- coordinates from its next start state, targets from the snapshot taken here, the program's, walls' and joint rows' state
        as their setters leave it -- while its neighbours go on; after `max_episodes` (0: no limit) it parks.  `qpos0`, `qvel0`:
        [S, n] (start states shared by the fleet) or [B, S, n] (per robot; qvel0 None: at rest); episode e starts from state e mod S.
        `poses`: [V, B, A, 7] pose variants of the slot's action list (episode e runs variant e mod V; needs a per-robot pose table), or
        None.  `records`: how many ended episodes per robot episode_state keeps (1 .. 16).  `poll_every` = P > 0: the call ends early,
        at a multiple of P ticks, once every robot is parked (ticks_run in the result; episodes.ticks_run is the formula).  After
        set_model, set_targets and the program; writes start state 0 into the slot's coordinates.  qpos0=None (or clear_episodes) ends
        them.  Refused next to a teleoperation stream or pushes; what else ends them: "one writer of the targets" in include/irlosc.h."""
        B = self._B[slot]
        if qpos0 is None:
            self._chk(self.lib.irlosc_set_episodes(self._h, slot, B, None, None, None, None))
            return
        n = self.layout.n
        q0 = np.ascontiguousarray(qpos0, dtype=np.float64)
        if not (q0.ndim in (2, 3) and q0.shape[-1] == n and q0.shape[-2] >= 1 and (q0.ndim == 2 or q0.shape[0] == B)):
            raise ValueError(f"qpos0: expected shape (S, {n}) or ({B}, S, {n}) with S >= 1, got {q0.shape}")
        v0 = np.zeros_like(q0) if qvel0 is None else np.ascontiguousarray(qvel0, dtype=np.float64)
        if v0.shape != q0.shape:
            raise ValueError(f"qvel0: expected shape {q0.shape}, got {v0.shape}")
        ps = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64)
        if ps is not None and not (ps.ndim == 4 and ps.shape[0] >= 1 and ps.shape[1] == B and ps.shape[3] == 7):
            raise ValueError(f"poses: expected shape (V, {B}, A, 7) with V >= 1, got {ps.shape}")
        desc = _lib.Episodes(int(max_ticks), int(bool(end_on_finish)), int(max_episodes), q0.shape[-2], int(q0.ndim == 3),
                             0 if ps is None else ps.shape[0], int(records), int(poll_every), 0)
        self._chk(self.lib.irlosc_set_episodes(self._h, slot, B, C.byref(desc), _lib.ptr(q0), _lib.ptr(v0), _lib.ptr(ps)))
        self._episode_records[slot] = int(records)

    def clear_episodes(self, slot: int = 0):
        """Ends the slot's episodes (irlosc_set_episodes with desc == NULL); everything else is left alone."""
        self.set_episodes(None, slot=slot)

    def episode_state(self, slot: int = 0):
        """-> dict(count, age, start_tick: [B]; running: robots not parked; records [B, R, 4] int32: start_tick, length, outcome
        (_lib.EPISODE_FINISHED / _TIMEOUT), start index | variant index << 16 of the robot's last R ended episodes, episode e at entry
        e mod R; ticks_run: the ticks the slot's last rollout call ran).  (irlosc_download_episode_state)"""
        B, R = self._B[slot], self._episode_records[slot]
        out = dict(count=np.empty(B, np.int32), age=np.empty(B, np.int32), start_tick=np.empty(B, np.int32))
        rec = np.empty((B, R, 4), dtype=np.int32)
        running, run = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.irlosc_download_episode_state(self._h, slot, B, _lib.ptr(out["count"]), _lib.ptr(out["age"]), _lib.ptr(out["start_tick"]),
                                                         C.byref(running), _lib.ptr(rec), C.byref(run)))
        return dict(out, running=int(running.value), records=rec, ticks_run=int(run.value))

    def download_q(self, slot: int = 0):
        """-> (qpos, qvel) [B, n] float64 of the slot as they sit in HBM: uploaded, or advanced by `rollout` (irlosc_download_q)."""
        B = self._B[slot]
        qpos = np.empty((B, self.layout.n), dtype=np.float64)
        qvel = np.empty((B, self.layout.n), dtype=np.float64)
        self._chk(self.lib.irlosc_download_q(self._h, slot, B, _lib.ptr(qpos), _lib.ptr(qvel)))
        return qpos, qvel

    # -- waypoint paths of the rollout (irlosc_set_waypoints / irlosc_download_waypoint_state) -------------------------------------
    def set_waypoints(self, xyz, threshold, loop=True, slot: int = 0):
        """Paths for the slot's robots, cycled on the GPU by `rollout` as examples/headless_loops.py::gain_test_loop cycles them on the
        host: a device whose EE comes within `threshold` (metres) of its target moves on to its next waypoint, wraps at the end
        (`loop`) or finishes on the last one.  `xyz`: per device (layout order) a [W, 3] array (one path for the fleet), a [B, W, 3]
        array (a path per robot) or None (the device keeps the slot's target); W <= 64.  `threshold`, `loop`: one value or one per
        device.  After set_model and set_targets; writes waypoint 0 into the slot's targets and resets the state.  xyz=None (or all
        None) clears the paths and nothing else.  A slot has one program -- paths, an action list or a teleoperation stream; what else ends them: "one writer of
        the targets" in include/irlosc.h."""
        L, B = self.layout, self._B[slot]
        paths = [None] * L.ndev if xyz is None else [None if p is None else np.asarray(p, dtype=np.float64) for p in xyz]
        if len(paths) != L.ndev:
            raise ValueError(f"xyz: expected one entry per device ({L.ndev}), got {len(paths)}")
        if all(p is None for p in paths):
            self._chk(self.lib.irlosc_set_waypoints(self._h, slot, B, None, None))
            return
        for d, p in enumerate(paths):
            if p is not None and not (p.ndim in (2, 3) and p.shape[-1] == 3 and p.shape[-2] >= 1 and (p.ndim == 2 or p.shape[0] == B)):
                raise ValueError(f"xyz[{d}]: expected shape (W, 3) or ({B}, W, 3) with W >= 1, got {p.shape}")
        nb = B if any(p is not None and p.ndim == 3 for p in paths) else 1
        wmax = max(p.shape[-2] for p in paths if p is not None)
        thr = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (L.ndev,))
        lp = np.broadcast_to(np.asarray(loop, dtype=bool), (L.ndev,))
        desc = _lib.Waypoints()
        desc.nb = nb
        tab = np.zeros((nb, L.ndev, wmax, 3), dtype=np.float64)
        for d, p in enumerate(paths):
            if p is None:
                continue
            desc.count[d], desc.threshold[d], desc.loop[d] = p.shape[-2], float(thr[d]), int(lp[d])
            tab[:, d, :p.shape[-2]] = p
        self._chk(self.lib.irlosc_set_waypoints(self._h, slot, B, C.byref(desc), _lib.ptr(tab)))

    def waypoint_state(self, slot: int = 0):
        """-> dict(index, arrivals, last_tick), each [B, ndev]: where every (robot, device) pair stands in its path (index == W: finished),
        how often it arrived and at which rollout tick since set_waypoints it last did (-1: never).  Devices without a path report
        (-1, 0, -1).  (irlosc_download_waypoint_state)"""
        L, B = self.layout, self._B[slot]
        idx = np.empty((B, L.ndev), dtype=np.int32)
        arr = np.empty((B, L.ndev), dtype=np.uint32)
        last = np.empty((B, L.ndev), dtype=np.int32)
        self._chk(self.lib.irlosc_download_waypoint_state(self._h, slot, B, _lib.ptr(idx), _lib.ptr(arr), _lib.ptr(last)))
        return dict(index=idx, arrivals=arr, last_tick=last)

    # -- the WP / GRIP action list of the rollout (irlosc_set_action_list / irlosc_download_action_state) ---------------------------
    def set_action_list(self, sequence, objects=None, active_arm: str = "right", tick_seconds: float = 0.001,
                        passive_hold_orientation: bool = False, slot: int = 0, passive_arm="auto"):
        """The WP / GRIP list of action_sequence.FleetActionSequenceRunner for the slot's robots, run on the GPU by `rollout`: per
        tick the active arm's error is judged, actions advance, an entered WP writes the slot's targets and the error-adaptive velocity
        limit goes into the slot's own copy of the gains -- no host in between.  `sequence`: the list of action dicts (defaults from
        action_sequence.DEFAULT_PARAMS), or a dict from action_sequence.compile_action_list; `objects`: per robot its action objects
        (one entry: shared by the fleet).  `passive_arm`: "auto" = the other UR5 when the layout has it, None = no passive arm.
        After set_model, set_gains and set_targets; resets the state.  sequence=None clears the list and nothing else.  A slot has one
        program -- a list, waypoint paths or a teleoperation stream; what else ends it: "one writer of the targets" in include/irlosc.h.  gripper_force is state;
        it drives a gripper where the slot has an action drive row on the active arm (set_joints)."""
        from . import action_sequence as aseq
        B = self._B[slot]
        if sequence is None:
            self._chk(self.lib.irlosc_set_action_list(self._h, slot, B, None, None))
            return
        if isinstance(sequence, dict):
            d = sequence
        else:
            names = list(self.layout.dev_names)
            arm = "ur5right" if active_arm == "right" else "ur5left"
            other = "ur5left" if active_arm == "right" else "ur5right"
            if passive_arm == "auto":
                passive_arm = other if other in names else None
            d = aseq.compile_action_list(sequence, objects if objects is not None else [{}], names.index(arm),
                                         names.index(passive_arm) if passive_arm is not None else -1, tick_seconds, passive_hold_orientation)
        A = int(d["n_actions"])
        if not 1 <= A <= _lib.MAX_ACTIONS:
            raise ValueError(f"an action list holds 1 to {_lib.MAX_ACTIONS} actions, got {A}")
        pose = np.ascontiguousarray(d["pose"], dtype=np.float64)
        if pose.ndim != 3 or pose.shape[1:] != (A, 7) or pose.shape[0] not in (1, B):
            raise ValueError(f"pose: expected shape (1 or {B}, {A}, 7), got {pose.shape}")
        desc = _lib.ActionList()
        desc.n_actions, desc.active_dev, desc.passive_dev = A, int(d["active_dev"]), int(d["passive_dev"])
        desc.passive_hold_orientation, desc.nb = int(d["passive_hold_orientation"]), pose.shape[0]
        for i in range(4):
            desc.passive_quat[i] = float(d["passive_quat"][i])
        for a in range(A):
            desc.kind[a], desc.xyz_from_start[a], desc.grip_ticks[a] = int(d["kind"][a]), int(d["xyz_from_start"][a]), int(d["grip_ticks"][a])
            desc.kp[a], desc.max_error[a] = float(d["kp"][a]), float(d["max_error"][a])
            desc.min_speed[a], desc.max_speed[a] = float(d["min_speed"][a]), float(d["max_speed"][a])
            desc.gripper_force[a] = float(d["gripper_force"][a])
        self._chk(self.lib.irlosc_set_action_list(self._h, slot, B, C.byref(desc), _lib.ptr(pose)))

    # -- the motion of the list in force (irlosc_set_action_motion / irlosc_download_action_motion_state) ------------------------------
    def set_action_motion(self, steps, noise_mean=None, noise_std=None, seed: int = 0, draw0=None, slot: int = 0):
        """INTERP moves and seeded target noise for the slot's action list (action_motion.py; "the motion of the list in force" in
        include/irlosc.h): per action `steps` (0: the WP jumps; N >= 1: its target travels from where the arm is to the goal over N
        ticks) and `noise_mean`, `noise_std` (Gaussian scatter on the goal's xyz, drawn on the GPU from `seed`, the robot's index, its
        count of draws and the action -- repeatable, and the same whatever else runs); `steps` may be the motion dict of
        action_motion.compile_action_motion / make_motion (its seed counts unless `seed` is given non-zero).  `draw0`: [B] draws to
        start from (default zeros).  After set_action_list, and after set_action_refs where refs are used; set_action_list ends it.
        steps=None clears the motion and nothing else."""
        if steps is None:
            self._chk(self.lib.irlosc_set_action_motion(self._h, slot, None, None))
            return
        if isinstance(steps, dict):
            noise_mean, noise_std, seed, steps = steps["noise_mean"], steps["noise_std"], seed or steps.get("seed", 0), steps["steps"]
        m = _lib.ActionMotion()
        n = len(steps)
        if n > _lib.MAX_ACTIONS:
            raise ValueError(f"an action list holds up to {_lib.MAX_ACTIONS} actions, got {n} steps")
        for name, v in (("noise_mean", noise_mean), ("noise_std", noise_std)):
            if v is not None and len(v) != n:
                raise ValueError(f"{name}: expected {n} entries like steps, got {len(v)}")
        for a in range(n):
            m.steps[a] = int(steps[a])
            m.noise_mean[a] = 0.0 if noise_mean is None else float(noise_mean[a])
            m.noise_std[a] = 0.0 if noise_std is None else float(noise_std[a])
        m.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        d0 = None
        if draw0 is not None:
            d0 = np.ascontiguousarray(draw0, dtype=np.uint32)
            if d0.shape != (self._B[slot],):
                raise ValueError(f"draw0: expected shape ({self._B[slot]},), got {d0.shape}")
        self._chk(self.lib.irlosc_set_action_motion(self._h, slot, C.byref(m), _lib.ptr(d0)))

    def action_motion_state(self, slot: int = 0):
        """-> dict(step [B] int32, draws [B] uint32, origin [B, 7], goal [B, 7]): the motion's state as of the last tick run -- where
        every robot's INTERP stands, the noise draws it has used, and the float64 goal (noise included) and origin of the WP it entered
        last.  (irlosc_download_action_motion_state)"""
        B = self._B[slot]
        out = dict(step=np.empty(B, np.int32), draws=np.empty(B, np.uint32), origin=np.empty((B, 7)), goal=np.empty((B, 7)))
        self._chk(self.lib.irlosc_download_action_motion_state(self._h, slot, B, *[_lib.ptr(out[k]) for k in ("step", "draws", "origin", "goal")]))
        return out

    # -- action objects of the rollout (irlosc_set_objects / irlosc_set_action_refs / irlosc_download_object_state) ---------------------
    def set_objects(self, objs, pose0=None, slot: int = 0):
        """Kinematic action objects for the slot's robots (objects.ObjectSet): inside `rollout` an object rides rigidly on the EE of a
        gripper whose fingers close near it (the rising edge of `closed`, inside the object's radius), stays where it is let go, and a
        plug that is free inside its socket's tolerances is recorded as mated.  No contact, no fall, no slipping; a weight only with
        set_object_loads.
        `pose0`: [B, nobj, 7] start poses (x y z qw qx qy qz), or [V, B, nobj, 7]: variants that episodes cycle (a reset takes
        variant count mod V).  After set_model and upload_q; resets the objects' state and ends the list's refs.  objs=None clears."""
        B = self._B[slot]
        if objs is None:
            self._chk(self.lib.irlosc_set_objects(self._h, slot, B, None, None))
            self._objects[slot] = (0, 0)
            self._grippers[slot] = 0
            return
        objs.check()
        NO = objs.n_objects
        p0 = np.ascontiguousarray(pose0, dtype=np.float64)
        if p0.ndim == 3:
            p0 = p0[None]
        if p0.ndim != 4 or p0.shape[0] < 1 or p0.shape[1:] != (B, NO, 7):
            raise ValueError(f"pose0: expected shape ({B}, {NO}, 7) or (V, {B}, {NO}, 7) with V >= 1, got {p0.shape}")
        d = objs.to_struct(p0.shape[0])
        self._chk(self.lib.irlosc_set_objects(self._h, slot, B, C.byref(d), _lib.ptr(p0)))
        self._objects[slot] = (NO, len(objs.mates))
        self._grippers[slot] = len(objs.grippers)

    # -- the weight of the action objects (irlosc_set_object_loads / irlosc_download_object_load_state) ---------------------------------
    def set_object_loads(self, loads, slot: int = 0):
        """A weight for the slot's action objects (object_loads.ObjectLoads: per object a mass and a centre of mass, and gravity): inside
        `rollout` a gripper that holds an object feels m g at the object's centre of mass as a wrench on its EE body -- on the plant on
        that tick, behind the pushes and the walls, and in the F/T wrench of the next tick (slots with a sensor feed).  Quasi-static: no
        inertial force, no fall, no collision, no slipping, and the fingers' forces are not in the feed.  After set_objects (which ends the
        loads, as set_model does), in front of set_action_refs and set_episodes; resets the loads' state and tick.  loads=None clears them
        and leaves the objects' state alone."""
        B = self._B[slot]
        if loads is None:
            self._chk(self.lib.irlosc_set_object_loads(self._h, slot, B, None, None))
            return
        NO = self._objects[slot][0]
        if not NO:
            raise _lib.IrloscError("set_objects must precede set_object_loads")
        table = np.ascontiguousarray(loads.table(B, NO))
        d = loads.to_struct(table.shape[0] > 1)      # (a lone robot's table is the shared form)
        self._chk(self.lib.irlosc_set_object_loads(self._h, slot, B, C.byref(d), _lib.ptr(table)))

    def object_load_state(self, slot: int = 0):
        """-> dict(load [B, n_grippers, 6]: the wrench the last tick applied per gripper (fx fy fz tx ty tz, world frame; zeros where it
        holds nothing), carry_ticks [B, n_grippers]: the ticks on which a weight was applied since set_object_loads or the robot's last
        reset).  (irlosc_download_object_load_state)"""
        B, NG = self._B[slot], self._grippers[slot]
        out = dict(load=np.empty((B, NG, 6)), carry_ticks=np.empty((B, NG), np.int32))
        self._chk(self.lib.irlosc_download_object_load_state(self._h, slot, B, _lib.ptr(out["load"]) if NG else None, _lib.ptr(out["carry_ticks"]) if NG else None))
        return out

    def set_action_refs(self, xyz_obj, quat_obj=None, slot: int = 0):
        """The slot's action list aims at its objects: per action the object (index, or -1) whose live xyz a WP's pose words are an
        OFFSET to, and the object whose live quaternion they are a grip rotation on (target = q_obj (x) q_grip), both read when the
        WP is entered.  After set_action_list and set_objects, which both end the refs.  xyz_obj=None clears them."""
        if xyz_obj is None:
            self._chk(self.lib.irlosc_set_action_refs(self._h, slot, None))
            return
        r = _lib.ActionRefs()
        quat_obj = [-1] * len(xyz_obj) if quat_obj is None else quat_obj
        for i in range(_lib.MAX_ACTIONS):
            r.xyz_obj[i] = int(xyz_obj[i]) if i < len(xyz_obj) else -1
            r.quat_obj[i] = int(quat_obj[i]) if i < len(quat_obj) else -1
        self._chk(self.lib.irlosc_set_action_refs(self._h, slot, C.byref(r)))

    def object_state(self, slot: int = 0):
        """-> dict(pose [B, nobj, 7], rel [B, nobj, 7], holder, grasp_tick, release_tick [B, nobj], mated_tick [B, nmates]): the slot's
        action objects as the last tick's object kernel left them (or a reset behind it).  (irlosc_download_object_state)"""
        B = self._B[slot]
        NO, NM = self._objects[slot]
        out = dict(pose=np.empty((B, NO, 7)), holder=np.empty((B, NO), np.int32), rel=np.empty((B, NO, 7)), grasp_tick=np.empty((B, NO), np.int32),
                   release_tick=np.empty((B, NO), np.int32), mated_tick=np.empty((B, NM), np.int32))
        self._chk(self.lib.irlosc_download_object_state(self._h, slot, B, *[_lib.ptr(out[k]) if out[k].size else None for k in
                                                                             ("pose", "holder", "rel", "grasp_tick", "release_tick", "mated_tick")]))
        return out

    def action_state(self, slot: int = 0):
        """-> dict(action, grip_left, err, max_vel0, gripper_force, finished_tick), each [B]: where every robot stands in the slot's
        action list AS OF THE START OF THE LAST TICK RUN (the state the last plant step produced is judged by the next tick);
        action == number of actions: finished, on tick finished_tick (-1 until then).  (irlosc_download_action_state)"""
        B = self._B[slot]
        out = dict(action=np.empty(B, np.int32), grip_left=np.empty(B, np.int32), err=np.empty(B), max_vel0=np.empty(B),
                   gripper_force=np.empty(B), finished_tick=np.empty(B, np.int32))
        self._chk(self.lib.irlosc_download_action_state(self._h, slot, B, *[_lib.ptr(out[k]) for k in
                                                                             ("action", "grip_left", "err", "max_vel0", "gripper_force", "finished_tick")]))
        return out

    # -- the teleoperation stream of the rollout (irlosc_set_teleop_stream / irlosc_download_teleop_state / irlosc_download_targets) ----
    def set_teleop_stream(self, readings, origin, rig=None, increment: float = 0.0015, loop: bool = False, slot: int = 0):
        """A recorded space-mouse session for the slot's robots, replayed on the GPU by `rollout` as examples/teleop_loops.py::
        space_mouse_loop runs it on the host: per tick the reading is integrated into the plate pose (SpaceMouse.update_state) and the
        followers' targets are written in front of the same tick's OSC step.  `readings`: [T, 6] (one stream for the fleet) or
        [B, T, 6] (one per robot), x y z roll pitch yaw rates, T <= 16384; `origin`: [6] or [B, 6], the pose before tick 0; `rig`: one
        teleop.follower per device (default: teleop.space_mouse_rig, the demo's).  `loop`: start over after T ticks, else the stream
        ends there and pose and targets stay.  After set_model and set_targets; resets pose and tick and writes no target (the first
        tick does).  readings=None (or clear_teleop_stream) clears the stream and nothing else.  A slot has one program -- paths, an
        action list or a stream; what else ends it: "one writer of the targets" in include/irlosc.h.  A robot that a narrower rollout
        leaves out keeps its pose and misses those readings.  ps_move has no resident form (teleop.py)."""
        from . import teleop as _t
        B = self._B[slot]
        if readings is None:
            self._chk(self.lib.irlosc_set_teleop_stream(self._h, slot, B, None, None, None))
            return
        rd = np.ascontiguousarray(readings, dtype=np.float64)
        if rd.ndim == 2:
            rd = rd[None]
        if rd.ndim != 3 or rd.shape[2] != 6 or rd.shape[1] < 1 or rd.shape[0] not in (1, B):
            raise ValueError(f"readings: expected shape (T, 6) or ({B}, T, 6) with T >= 1, got {np.shape(readings)}")
        og = np.ascontiguousarray(origin, dtype=np.float64)
        if og.ndim == 1:
            og = og[None]
        if og.ndim != 2 or og.shape[1] != 6 or og.shape[0] not in (1, B):
            raise ValueError(f"origin: expected shape (6,) or ({B}, 6), got {np.shape(origin)}")
        rig = _t.space_mouse_rig(self.layout) if rig is None else list(rig)
        if len(rig) != self.layout.ndev:
            raise ValueError(f"rig: expected one follower per device ({self.layout.ndev}), got {len(rig)}")
        desc = _t.to_struct(rig, rd.shape[1], rd.shape[0], og.shape[0], increment, loop)
        self._chk(self.lib.irlosc_set_teleop_stream(self._h, slot, B, C.byref(desc), _lib.ptr(np.ascontiguousarray(rd)), _lib.ptr(np.ascontiguousarray(og))))

    def clear_teleop_stream(self, slot: int = 0):
        """Ends the slot's stream (irlosc_set_teleop_stream with desc == NULL); targets, paths and a list are left alone."""
        self.set_teleop_stream(None, None, slot=slot)

    def teleop_state(self, slot: int = 0):
        """-> dict(pose [B, 6]: x y z roll pitch yaw of every robot's plate as the last tick that ran it left it (the origin before the
        first), tick: the slot's rollout ticks since set_teleop_stream).  (irlosc_download_teleop_state)"""
        B = self._B[slot]
        pose = np.empty((B, 6), dtype=np.float64)
        tick = C.c_int32(0)
        self._chk(self.lib.irlosc_download_teleop_state(self._h, slot, B, _lib.ptr(pose), C.byref(tick)))
        return dict(pose=pose, tick=int(tick.value))

    # -- the policy of the rollout (irlosc_set_policy / irlosc_download_policy_state) ---------------------------------------------------
    def set_policy(self, layers, obs, origin, rig=None, increment: float = 0.0015, clip: float = 0.0, keep_obs: bool = False,
                   grip_dev=0, grip_close: float = 0.0, grip_open: float = 0.0, slot: int = 0):
        """A policy for the slot's robots, evaluated on the GPU by `rollout`: per tick and robot the network `layers` ([(W [out, in],
        b [out]), ...] float32, ReLU between the layers; policy.from_torch reads them off a torch Sequential) maps the observation --
        the channels of `obs` (names of policy.OBS_BITS or an OR of _lib.OBS_*) in bit order, cast to float32 -- to the tick's
        space-mouse reading (outputs 0 .. 5, clamped to [-clip, clip] where clip > 0), which moves the plate and the followers' targets
        exactly as a stream's reading does (set_teleop_stream: `origin` [6] or [B, 6], `rig`, `increment`), in front of the same tick's
        OSC step.  A seventh output drives the gripper: the ACTION drive rows (set_joints) of device `grip_dev` take `grip_close` where
        it is > 0 and `grip_open` elsewhere.  The arithmetic is policy.mlp's, bit for bit.  `keep_obs`: policy_state also returns the
        observation of the last tick.  After set_model and set_targets (and set_objects, if it observes object_pose); replaces the
        slot's program; layers=None (or clear_policy) clears the policy and nothing else."""
        from . import policy as _p, teleop as _t
        B = self._B[slot]
        if layers is None:
            self._chk(self.lib.irlosc_set_policy(self._h, slot, B, None, None, None))
            self._policy[slot] = None
            return
        layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in layers]
        mask = _p.obs_mask(obs)
        n_in = _p.obs_width(mask, self.layout.n, self.layout.ndev, self._objects[slot][0])
        dims = [n_in] + [W.shape[0] for W, _ in layers]
        for l, (W, b) in enumerate(layers):
            if W.shape != (dims[l + 1], dims[l]) or b.shape != (dims[l + 1],):
                raise ValueError(f"layer {l}: expected W {(dims[l + 1], dims[l])} and b {(dims[l + 1],)}, got {W.shape} and {b.shape}")
        og = np.ascontiguousarray(origin, dtype=np.float64)
        if og.ndim == 1:
            og = og[None]
        if og.ndim != 2 or og.shape[1] != 6 or og.shape[0] not in (1, B):
            raise ValueError(f"origin: expected shape (6,) or ({B}, 6), got {np.shape(origin)}")
        rig = _t.space_mouse_rig(self.layout) if rig is None else list(rig)
        if len(rig) != self.layout.ndev:
            raise ValueError(f"rig: expected one follower per device ({self.layout.ndev}), got {len(rig)}")
        if isinstance(grip_dev, str):
            grip_dev = self.layout.dev_names.index(grip_dev)
        desc = _p.to_struct(layers, mask, rig, og.shape[0], increment, clip, keep_obs, grip_dev, grip_close, grip_open)
        self._chk(self.lib.irlosc_set_policy(self._h, slot, B, C.byref(desc), _lib.ptr(_p.weights(layers)), _lib.ptr(og)))
        self._policy[slot] = (n_in, dims[-1], bool(keep_obs))

    def set_policy_noise(self, std, seed: int = 0, draw0=None, slot: int = 0):
        """A Gaussian head on the slot's policy (irlosc_set_policy_noise; "a stochastic policy head" in include/irlosc.h): the network's
        output becomes the mean, and per tick and robot the action act[c] = out[c] + std[c] eps[c] is drawn on the GPU -- from `seed`,
        the robot's index and its count of draws, so repeatable and the same whatever else runs -- and steers the plate (and the grip)
        in place of out; the robot's log-probability is kept with it (policy_noise_state; the log's policy_sample channel).  `std`:
        [n_out] float32, >= 0, at least one > 0 (0: that output stays deterministic).  `draw0`: [B] draws to start from (default
        zeros).  The arithmetic is policy.sample's, bit for bit.  After set_policy, which ends it; std=None clears the head and
        nothing else."""
        if std is None:
            self._chk(self.lib.irlosc_set_policy_noise(self._h, slot, None, None))
            return
        sd = np.asarray(std, dtype=np.float32).reshape(-1)
        if len(sd) > 8:
            raise ValueError(f"std: expected one entry per output (6 or 7), got {len(sd)}")
        d = _lib.PolicyNoise()
        d.seed, d.n_std, d.reserved = int(seed) & 0xFFFFFFFFFFFFFFFF, len(sd), 0
        for c, v in enumerate(sd):
            d.std[c] = float(v)
        d0 = None
        if draw0 is not None:
            d0 = np.ascontiguousarray(draw0, dtype=np.uint32)
            if d0.shape != (self._B[slot],):
                raise ValueError(f"draw0: expected shape ({self._B[slot]},), got {d0.shape}")
        self._chk(self.lib.irlosc_set_policy_noise(self._h, slot, C.byref(d), _lib.ptr(d0)))

    def policy_noise_state(self, slot: int = 0):
        """-> dict(act [B, n_out] float32: the action the last tick that ran the robot took; logp [B]: its log-probability under the
        head (the density at the unrounded float64 action); draws [B] uint32: the ticks that ran the robot since set_policy_noise, on
        top of draw0; logp_const: C of logp = -sum(eps^2) / 2 - C).  (irlosc_download_policy_noise_state)"""
        B = self._B[slot]
        if self._policy[slot] is None:      # (the library says why)
            self._chk(self.lib.irlosc_download_policy_noise_state(self._h, slot, B, None, None, None, None))
        n_out = self._policy[slot][1]
        act, logp, draws = np.empty((B, n_out), dtype=np.float32), np.empty(B, dtype=np.float64), np.empty(B, dtype=np.uint32)
        const = C.c_double(0.0)
        self._chk(self.lib.irlosc_download_policy_noise_state(self._h, slot, B, _lib.ptr(act), _lib.ptr(logp), _lib.ptr(draws), C.byref(const)))
        return dict(act=act, logp=logp, draws=draws, logp_const=float(const.value))

    def clear_policy(self, slot: int = 0):
        """Ends the slot's policy (irlosc_set_policy with desc == NULL); targets and any other program are left alone."""
        self.set_policy(None, None, None, slot=slot)

    def policy_state(self, slot: int = 0):
        """-> dict(pose [B, 6]: every robot's plate as the last tick that ran it left it (the origin before the first); out [B, n_out]
        float32: the network's output of that tick, before the clamp; grip [B]; obs [B, n_in] float32 (with keep_obs, else None); tick:
        the slot's rollout ticks since set_policy).  (irlosc_download_policy_state)"""
        B = self._B[slot]
        if self._policy[slot] is None:      # (the library says why)
            self._chk(self.lib.irlosc_download_policy_state(self._h, slot, B, None, None, None, None, None))
        n_in, n_out, keep = self._policy[slot]
        pose, out, grip = np.empty((B, 6), dtype=np.float64), np.empty((B, n_out), dtype=np.float32), np.empty(B, dtype=np.float64)
        obs = np.empty((B, n_in), dtype=np.float32) if keep else None
        tick = C.c_int32(0)
        self._chk(self.lib.irlosc_download_policy_state(self._h, slot, B, _lib.ptr(pose), _lib.ptr(out), _lib.ptr(grip), _lib.ptr(obs), C.byref(tick)))
        return dict(pose=pose, out=out, grip=grip, obs=obs, tick=int(tick.value))

    def download_targets(self, slot: int = 0):
        """-> the slot's targets [B, ndev, 7] in the context's dtype as they sit in HBM: given by set_targets, or written by the
        program of its rollouts (irlosc_download_targets)."""
        B = self._B[slot]
        tgt = np.empty((B, self.layout.ndev, 7), dtype=self.dtype)
        self._chk(self.lib.irlosc_download_targets(self._h, slot, B, _lib.ptr(tgt)))
        return tgt

    # -- external pushes of the rollout (irlosc_set_pushes) ---------------------------------------------------------------------------
    def set_pushes(self, pushes, wrench=None, slot: int = 0):
        """External wrenches on EE bodies during windows of the slot's rollout ticks, as examples/headless_loops.py::admit_test_loop
        sets xfrc_applied: `pushes` is a list of dict(dev=name_or_index, window=(tick0, tick1), apply=True, sense=True) -- active on the
        ticks tick0 <= t < tick1 counted since this call (pushes.push_window_ticks maps the reference's window); `apply`: it acts on
        the plant (at the EE body's frame origin), `sense`: the F/T wrench of the next tick carries its reaction (slots with a sensor
        feed).  `wrench`: [P, 6] (one table for the fleet) or [B, P, 6], world frame, fx fy fz tx ty tz.  After set_model.  pushes=None
        (or clear_pushes) ends them and nothing else; they coexist with waypoint paths and an action list."""
        from . import pushes as _p
        B = self._B[slot]
        if pushes is None:
            self._chk(self.lib.irlosc_set_pushes(self._h, slot, B, None, None))
            return
        P = len(pushes)
        if not 1 <= P <= _lib.MAX_PUSHES:
            raise ValueError(f"a slot holds 1 to {_lib.MAX_PUSHES} pushes, got {P}")
        dev, t0, t1, ap, se = _p.normalise(pushes, self.layout.dev_names)
        w = np.ascontiguousarray(wrench, dtype=np.float64)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1:] != (P, 6) or w.shape[0] not in (1, B):
            raise ValueError(f"wrench: expected shape ({P}, 6) or ({B}, {P}, 6), got {np.shape(wrench)}")
        desc = _lib.Pushes()
        desc.n_pushes, desc.nb = P, w.shape[0]
        for p in range(P):
            desc.dev[p], desc.tick0[p], desc.tick1[p] = int(dev[p]), int(t0[p]), int(t1[p])
            desc.apply[p], desc.sense[p] = int(ap[p]), int(se[p])
        self._chk(self.lib.irlosc_set_pushes(self._h, slot, B, C.byref(desc), _lib.ptr(np.ascontiguousarray(w))))

    def clear_pushes(self, slot: int = 0):
        """Ends the slot's pushes (irlosc_set_pushes with desc == NULL); targets, programs and feeds are left alone."""
        self.set_pushes(None, slot=slot)

    # -- compliant walls of the rollout (irlosc_set_walls / irlosc_download_wall_state) ------------------------------------------------
    def set_walls(self, walls, slot: int = 0):
        """Penalty walls on EE bodies inside the slot's rollouts, as the wall of the reference's force_test scene: `walls` is a list of
        dict(dev=name_or_index, normal=(nx, ny, nz), offset= | point=, radius=0, stiffness=, damping=0), values scalars or per-robot
        arrays (walls.normalise).  The EE is a sphere of `radius` around the EE body's frame origin; inside the half-space the force
        stiffness x depth - damping x approach speed acts along the normal, never pulling, and the F/T wrench of the next tick carries
        its reaction (slots with a sensor feed).  After set_model; resets the walls' state and tick.  walls=None (or clear_walls) ends
        them and nothing else; they coexist with waypoint paths, an action list and pushes.  Not MuJoCo's soft constraint: no friction,
        planes only, one contact point."""
        from . import walls as _w
        B = self._B[slot]
        if walls is None:
            self._chk(self.lib.irlosc_set_walls(self._h, slot, B, None, None))
            return
        dev, table = _w.normalise(walls, self.layout.dev_names, B)
        desc = _lib.Walls()
        desc.n_walls, desc.nb = len(dev), table.shape[0]
        for w in range(len(dev)):
            desc.dev[w] = int(dev[w])
        self._chk(self.lib.irlosc_set_walls(self._h, slot, B, C.byref(desc), _lib.ptr(np.ascontiguousarray(table))))

    def clear_walls(self, slot: int = 0):
        """Ends the slot's walls (irlosc_set_walls with desc == NULL); targets, programs, pushes and feeds are left alone."""
        self.set_walls(None, slot=slot)

    def wall_state(self, slot: int = 0):
        """-> dict(force [B, ndev, 3], max_depth [B, ndev], contact_ticks [B, ndev], first_tick [B, ndev]): per robot and device the
        force the last rollout tick applied, the deepest penetration seen since set_walls (0: none), the ticks in contact and the first
        of them (-1: none).  Devices without a wall report (0, 0, 0, -1).  (irlosc_download_wall_state)"""
        L, B = self.layout, self._B[slot]
        force = np.empty((B, L.ndev, 3), dtype=np.float64)
        depth = np.empty((B, L.ndev), dtype=np.float64)
        ticks = np.empty((B, L.ndev), dtype=np.int32)
        first = np.empty((B, L.ndev), dtype=np.int32)
        self._chk(self.lib.irlosc_download_wall_state(self._h, slot, B, _lib.ptr(force), _lib.ptr(depth), _lib.ptr(ticks), _lib.ptr(first)))
        return dict(force=force, max_depth=depth, contact_ticks=ticks, first_tick=first)

    # -- joint rows of the rollout (irlosc_set_joints / irlosc_download_joint_state) --------------------------------------------------
    def set_joints(self, rows, slot: int = 0):
        """Joint-space forces inside the slot's rollouts: `rows` is a list of dicts (joints.normalise; joints.scene_rows builds the
        Dual-UR5 set) -- kind="limit" (a range stop with stiffness and damping on one hinge), kind="couple" (a linear equality row
        between two hinges, as the scene ties a finger linkage to its driven knuckle) or kind="drive" (gear x ctrl on one hinge, ctrl a
        constant or the gripper_force of the slot's action list) -- hinges by name (after set_model) or index, values scalars or
        per-robot arrays.  Every tick the rollout computes one torque per hinge from that hinge's coordinates and hands it to the plant.
        Explicit penalties, not MuJoCo's soft constraints; the F/T feed does not see them.  After set_model; resets the rows' state and
        tick.  rows=None (or clear_joints) ends them and nothing else; they coexist with waypoint paths, an action list, pushes and walls."""
        from . import joints as _j
        B = self._B[slot]
        if rows is None:
            self._chk(self.lib.irlosc_set_joints(self._h, slot, B, None, None))
            self._joint_rows[slot] = 0
            return
        model = getattr(self, "_model", None)
        names = model.joint_names if model is not None else [str(j) for j in range(self.layout.n)]
        d, table = _j.normalise(rows, names, self.layout.dev_names, B)
        desc = _lib.JointRows()
        desc.n_rows, desc.per_robot = table.shape[1], int(d["per_robot"])
        for r in range(table.shape[1]):
            desc.kind[r], desc.joint_a[r], desc.joint_b[r] = int(d["kind"][r]), int(d["joint_a"][r]), int(d["joint_b"][r])
            desc.source[r], desc.dev[r] = int(d["source"][r]), int(d["dev"][r])
        self._chk(self.lib.irlosc_set_joints(self._h, slot, B, C.byref(desc), _lib.ptr(np.ascontiguousarray(table))))
        self._joint_rows[slot] = table.shape[1]

    def clear_joints(self, slot: int = 0):
        """Ends the slot's joint rows (irlosc_set_joints with desc == NULL); targets, programs, pushes, walls and feeds are left alone."""
        self.set_joints(None, slot=slot)

    def joint_state(self, slot: int = 0):
        """-> dict(tau [B, n], max_violation [B, R], active_ticks [B, R], ctrl [B, R]): per robot the torque per hinge the last rollout
        tick applied, and per row the largest violation seen since set_joints (a LIMIT: how far outside its range, a COUPLE: |e|), the
        ticks on which the row contributed and a DRIVE's ctrl.
        (irlosc_download_joint_state)"""
        L, B = self.layout, self._B[slot]
        R = self._joint_rows[slot]
        tau = np.empty((B, L.n), dtype=np.float64)
        viol = np.empty((B, R), dtype=np.float64)
        ticks = np.empty((B, R), dtype=np.int32)
        ctrl = np.empty((B, R), dtype=np.float64)
        self._chk(self.lib.irlosc_download_joint_state(self._h, slot, B, _lib.ptr(tau), _lib.ptr(viol), _lib.ptr(ticks), _lib.ptr(ctrl)))
        return dict(tau=tau, max_violation=viol, active_ticks=ticks, ctrl=ctrl)

    def step_resident_from_q(self, iters: int, first_slot: int = 0, B: Optional[int] = None):
        """-> (ms_total, ms_per_step): `iters` x (front end + step) on resident joint coordinates, HIP-event timed."""
        B = self._B[first_slot] if B is None else B
        t, a = C.c_float(), C.c_float()
        self._chk(self.lib.irlosc_step_resident_from_q(self._h, first_slot, B, iters, C.byref(t), C.byref(a)))
        return t.value, a.value

    def sync(self):
        self._chk(self.lib.irlosc_sync(self._h))

    def device_sync(self):
        """hipDeviceSynchronize on this context's GPU (the bench bracket)."""
        self._chk(self.lib.irlosc_device_sync(self._h))

    def tick(self, M, J, dq, bias, ee_pose, tgt_pose, tgt_vel=None, wrench=None, return_flags: bool = False,
             check_symmetric: bool = False):
        """One control tick for B instances in ONE library call (irlosc_tick): one host-to-device copy, the step, one
        copy back, one synchronisation.  Does not touch the resident slots."""
        L = self.layout
        B = int(np.shape(M)[0])
        M = self._arr(M, (B, L.n, L.n), "M")
        if check_symmetric:
            self._check_symmetric(M)
        J = self._arr(J, (B, L.k, L.n), "J")
        dq = self._arr(dq, (B, L.n), "dq")
        bias = self._arr(bias, (B, L.n), "bias")
        ee = self._arr(ee_pose, (B, L.ndev, 7), "ee_pose")
        wr = self._arr(wrench, (B, L.ndev, 6), "wrench")
        tp = self._arr(tgt_pose, (B, L.ndev, 7), "tgt_pose")
        tv = self._arr(tgt_vel, (B, L.ndev, 6), "tgt_vel")
        u = np.empty((B, L.n), dtype=self.dtype)
        fl = np.empty(B, dtype=np.uint32)
        self._chk(self.lib.irlosc_tick(self._h, B, _lib.ptr(M), _lib.ptr(J), _lib.ptr(dq), _lib.ptr(bias), _lib.ptr(ee),
                                       _lib.ptr(wr), _lib.ptr(tp), _lib.ptr(tv), _lib.ptr(u), _lib.ptr(fl)))
        return (u, fl) if return_flags else u

    def generate_batched(self, M, J, dq, bias, ee_pose, tgt_pose, tgt_vel=None, wrench=None,
                         return_flags: bool = False):
        """One tick for B instances: upload, step, download."""
        self.upload(M, J, dq, bias, ee_pose, wrench)
        self.set_targets(tgt_pose, tgt_vel)
        return self.step(return_flags=return_flags)
