"""The weight of a rollout's action objects on the host (include/irlosc.h: irlosc_set_object_loads; csrc/osc_object_load.hpp): the
descriptor BatchedOSC.set_object_loads takes, and load_wrench, a NumPy mirror of the load kernel's APPLY in the kernel's own operation
order -- every product, sum and difference is one NumPy operation on float64 arrays, so each is rounded on its own as __dmul_rn /
__dadd_rn / __dsub_rn round it, and the mirror repeats the kernel's bits.

What a load is: a held object's weight m g, acting at its centre of mass, felt by the holder's EE body as a wrench at the body's frame
origin -- on the plant on this tick, in the F/T feed on the next.  What it is not: there is no inertial force (m a), a released object
does not fall, nothing collides or slips, and the fingers' forces are not in the feed."""
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from .objects import mat_vec, quat2mat

GRAVITY = (0.0, 0.0, -9.81)


@dataclass
class ObjectLoads:
    """Per object a mass [kg] and a centre of mass in the object's frame [m], and the gravity vector of the world frame.
      mass     [nobj] (shared by the fleet) or [B, nobj] (per robot), >= 0; 0: the object weighs nothing
      com      [nobj, 3] or [B, nobj, 3]; None: the objects' frame origins
      gravity  [3]"""
    mass: Sequence
    com: Sequence = None
    gravity: Sequence[float] = GRAVITY

    def table(self, B: int, nobj: int):
        """-> [nb, nobj, 4] float64 with nb = 1 (mass and com both shared) or B: rows mass, com_x, com_y, com_z -- irlosc_set_object_loads' table"""
        m = np.asarray(self.mass, dtype=np.float64)
        c = np.zeros(m.shape + (3,)) if self.com is None else np.asarray(self.com, dtype=np.float64)
        if m.ndim not in (1, 2) or m.shape[-1] != nobj or (m.ndim == 2 and m.shape[0] != B):
            raise ValueError(f"mass: expected shape ({nobj},) or ({B}, {nobj}), got {m.shape}")
        if c.ndim not in (2, 3) or c.shape[-2:] != (nobj, 3) or (c.ndim == 3 and c.shape[0] != B):
            raise ValueError(f"com: expected shape ({nobj}, 3) or ({B}, {nobj}, 3), got {c.shape}")
        nb = B if (m.ndim == 2 or c.ndim == 3) else 1
        t = np.empty((nb, nobj, 4))
        t[:, :, 0] = m if m.ndim == 2 else m[None]
        t[:, :, 1:] = c if c.ndim == 3 else c[None]
        return t

    def to_struct(self, per_robot: bool):
        """-> struct irlosc_object_loads (_lib.ObjectLoads)"""
        from . import _lib
        d = _lib.ObjectLoads()
        d.per_robot, d.reserved = int(bool(per_robot)), 0
        g = np.asarray(self.gravity, dtype=np.float64).reshape(3)
        for i in range(3):
            d.gravity[i] = float(g[i])
        return d


def load_wrench(loads: ObjectLoads, objs, ee_pose, obj_pose, holder=None):
    """W [B, n_grippers, 6] (fx fy fz tx ty tz, world frame): what the load kernel's APPLY computes on a tick, steps 1 to 3 of
    csrc/osc_object_load.hpp.
      objs      objects.ObjectSet: its grippers name the devices
      ee_pose   [B, ndev, 7] EE poses of the tick (the log's EE_POSE channel)
      obj_pose  [B, nobj, 7] the objects as this tick's object kernel left them, or [B, nobj, 8] with the holder as word 7 (the log's
                OBJECT_POSE channel)
      holder    [B, nobj] int, -1 = free; None: word 7 of obj_pose
    Per gripper g the lowest object it holds counts; none, mass 0 or a word that is not finite: zeros."""
    ee = np.asarray(ee_pose, dtype=np.float64)
    op = np.asarray(obj_pose, dtype=np.float64)
    B, NO = op.shape[:2]
    hold = (op[:, :, 7] if holder is None else np.asarray(holder)).astype(np.int64)
    tab = np.broadcast_to(loads.table(B, NO), (B, NO, 4))
    grav = np.asarray(loads.gravity, dtype=np.float64).reshape(3)
    W = np.zeros((B, len(objs.grippers), 6))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for g, gr in enumerate(objs.grippers):
            found = np.zeros(B, dtype=bool)
            p_ee = ee[:, gr.dev, :3]
            for o in range(NO):
                mine = ~found & (hold[:, o] == g)
                found |= mine
                mass, com = tab[:, o, 0], tab[:, o, 1:]
                c = mat_vec(quat2mat(op[:, o, 3:7]), com)
                p_c = op[:, o, :3] + c
                r = p_c - p_ee
                F = mass[:, None] * grav[None, :]
                T = np.stack([r[:, 1] * F[:, 2] - r[:, 2] * F[:, 1], r[:, 2] * F[:, 0] - r[:, 0] * F[:, 2], r[:, 0] * F[:, 1] - r[:, 1] * F[:, 0]], axis=1)
                Wo = np.concatenate([F, T], axis=1)
                take = mine & (mass != 0.0)
                W[take, g] = Wo[take]
            bad = ~np.isfinite(W[:, g]).all(axis=1)
            W[bad, g] = 0.0
    return W
