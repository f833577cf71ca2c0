"""Action objects of a rollout on the host (include/irlosc.h, "action objects"; csrc/osc_object.hpp): the descriptors that
BatchedOSC.set_objects takes, and object_step, a NumPy mirror of the object kernel in the kernel's own operation order -- every product
and sum is one NumPy operation on float64 arrays, so each is rounded on its own as __dmul_rn / __dadd_rn round it, and the mirror
repeats the kernel's bits.  ref_target is the same for the composition an action list's refs make at a WP's entry (csrc/osc_action.hpp).

What an object is: a pose that rides rigidly on an EE once that arm's fingers have closed near it, stays where it is let go, and can be
recorded as mated with a socket.  By itself it acts on nothing; with loads (object_loads.py) a held object has a weight that the plant
and the F/T feed see.  What it is not: it has no inertial force, collides with nothing and does not fall or slip."""
from dataclasses import dataclass, field
from typing import Dict, List, Sequence

import numpy as np

MAX_OBJECTS, MAX_GRIPPERS, MAX_MATES = 4, 2, 2


@dataclass
class Gripper:
    """A hand that can hold an object: the device whose EE carries it (index in the layout's dev_names), the knuckle hinge whose coordinate
    says closed (sign q >= sign q_close) or open (sign q <= sign q_open), and the point of the EE frame an object must be near."""
    dev: int
    joint: int
    q_close: float
    q_open: float
    sign: int = 1
    grip_xyz: Sequence[float] = (0.0, 0.0, 0.0)


@dataclass
class Mate:
    """Object `plug` counts as inserted when it is free within tol_xyz of the seat (a pose in object `socket`'s frame) and
    |q_plug . q_seat| >= min_abs_dot."""
    plug: int
    socket: int
    tol_xyz: float
    min_abs_dot: float = 0.0
    seat_xyz: Sequence[float] = (0.0, 0.0, 0.0)
    seat_quat: Sequence[float] = (1.0, 0.0, 0.0, 0.0)


@dataclass
class ObjectSet:
    """The action objects of a slot: per object the radius inside which a closing hand takes it, the grippers and the mates."""
    radius: Sequence[float]
    grippers: List[Gripper]
    mates: List[Mate] = field(default_factory=list)

    @property
    def n_objects(self) -> int:
        return len(self.radius)

    def to_struct(self, n_variants: int = 1):
        """-> struct irlosc_objects (_lib.Objects) for `n_variants` sets of start poses"""
        from . import _lib
        d = _lib.Objects()
        d.n_objects, d.n_grippers, d.n_mates, d.n_variants = self.n_objects, len(self.grippers), len(self.mates), int(n_variants)
        for o in range(self.n_objects):
            d.radius[o] = float(self.radius[o])
        for g, gr in enumerate(self.grippers):
            d.dev[g], d.joint[g], d.sign[g], d.q_close[g], d.q_open[g] = int(gr.dev), int(gr.joint), int(gr.sign), float(gr.q_close), float(gr.q_open)
            for i in range(3):
                d.grip_xyz[g][i] = float(gr.grip_xyz[i])
        for m, mt in enumerate(self.mates):
            d.plug[m], d.socket[m], d.tol_xyz[m], d.min_abs_dot[m] = int(mt.plug), int(mt.socket), float(mt.tol_xyz), float(mt.min_abs_dot)
            for i in range(3):
                d.seat_xyz[m][i] = float(mt.seat_xyz[i])
            for i in range(4):
                d.seat_quat[m][i] = float(mt.seat_quat[i])
        return d

    def check(self):
        if not 1 <= self.n_objects <= MAX_OBJECTS or not 1 <= len(self.grippers) <= MAX_GRIPPERS or len(self.mates) > MAX_MATES:
            raise ValueError(f"an object set holds 1..{MAX_OBJECTS} objects, 1..{MAX_GRIPPERS} grippers and up to {MAX_MATES} mates")
        return self


def object_state(pose0) -> Dict:
    """The per-robot state as irlosc_set_objects resets it on start poses pose0 [B, nobj, 7]: free, ticks -1."""
    pose0 = np.array(pose0, dtype=np.float64)
    B, NO = pose0.shape[:2]
    return dict(pose=pose0, rel=np.zeros((B, NO, 7)), holder=np.full((B, NO), -1, np.int32), grasp_tick=np.full((B, NO), -1, np.int32),
                release_tick=np.full((B, NO), -1, np.int32), was_closed=np.zeros((B, MAX_GRIPPERS), np.int32),
                mated_tick=np.full((B, MAX_MATES), -1, np.int32))


# ---- the kernels' helpers (csrc/osc_common.hpp), on arrays [..., 4] / [..., 3]: one NumPy operation per rounded operation -------------
def quat_mul(a, b):
    """a (x) b, the Hamilton product (w x y z), terms left to right: quat_mul_rn."""
    a0, a1, a2, a3 = (a[..., i] for i in range(4))
    b0, b1, b2, b3 = (b[..., i] for i in range(4))
    return np.stack([((a0 * b0 - a1 * b1) - a2 * b2) - a3 * b3,
                     ((a0 * b1 + a1 * b0) + a2 * b3) - a3 * b2,
                     ((a0 * b2 + a2 * b0) + a3 * b1) - a1 * b3,
                     ((a0 * b3 + a3 * b0) + a1 * b2) - a2 * b1], axis=-1)


def quat2mat(q):
    """R(q) [..., 3, 3]: quat2mat_rn (transforms.quat2mat without its Nq < eps branch)."""
    w, x, y, z = (q[..., i] for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        Nq = ((w * w + x * x) + y * y) + z * z
        s = 2.0 / Nq
        X, Y, Z = x * s, y * s, z * s
        wX, wY, wZ = w * X, w * Y, w * Z
        xX, xY, xZ = x * X, x * Y, x * Z
        yY, yZ, zZ = y * Y, y * Z, z * Z
        rows = [[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX], [xZ - wY, yZ + wX, 1.0 - (xX + yY)]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def mat_vec(R, v):
    """R v: each row's three products summed left to right (mat_vec_rn)."""
    return np.stack([(R[..., c, 0] * v[..., 0] + R[..., c, 1] * v[..., 1]) + R[..., c, 2] * v[..., 2] for c in range(3)], axis=-1)


def mat_t_vec(R, v):
    """R^T v (mat_t_vec_rn)."""
    return np.stack([(R[..., 0, c] * v[..., 0] + R[..., 1, c] * v[..., 1]) + R[..., 2, c] * v[..., 2] for c in range(3)], axis=-1)


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def object_step(state: Dict, objs: ObjectSet, ee, q, t: int) -> Dict:
    """One tick of the object kernel in NumPy, in place and in the kernel's order (csrc/osc_object.hpp, steps 0 to 4).
      state  object_state(...), advanced in place
      ee     [B, ndev, 7] EE poses at the start of tick t (the log's EE_POSE channel)
      q      [B, n] joint coordinates at the start of tick t (the log's QPOS channel): the knuckle angles are read from it
      t      the objects' tick"""
    ee = np.asarray(ee, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    B = len(ee)
    NO, G = objs.n_objects, objs.grippers
    pose, rel, holder = state["pose"], state["rel"], state["holder"]
    with np.errstate(invalid="ignore", over="ignore"):
        pe = [ee[:, g.dev, :3] for g in G]
        qe = [ee[:, g.dev, 3:] for g in G]
        R = [quat2mat(x) for x in qe]
        sq = [float(g.sign) * q[:, g.joint] for g in G]
        closed = [s >= float(g.sign) * g.q_close for s, g in zip(sq, G)]
        opened = [s <= float(g.sign) * g.q_open for s, g in zip(sq, G)]
        ok = np.ones(B, dtype=bool)                       # 0. a robot with an EE pose word that is not finite sits the tick out
        for g in G:
            ok &= np.isfinite(ee[:, g.dev]).all(axis=1)
        holds = [np.zeros(B, dtype=bool) for _ in G]
        released = np.zeros((B, NO), dtype=bool)
        for o in range(NO):                               # 1. held objects
            for gi in range(len(G)):
                held = ok & (holder[:B, o] == gi)
                let_go = held & opened[gi]
                carried = held & ~opened[gi]
                holder[:B, o][let_go] = -1
                state["release_tick"][:B, o][let_go] = t
                released[let_go, o] = True
                xyz = pe[gi] + mat_vec(R[gi], rel[:B, o, :3])
                quat = quat_mul(qe[gi], rel[:B, o, 3:])
                pose[:B, o, :3][carried] = xyz[carried]
                pose[:B, o, 3:][carried] = quat[carried]
                holds[gi] |= carried
        for o in range(NO):                               # 2. free objects: the rising edge of a hand near one
            for gi, g in enumerate(G):
                gp = pe[gi] + mat_vec(R[gi], np.broadcast_to(np.asarray(g.grip_xyz, dtype=np.float64), (B, 3)))
                near = _dist2(gp, pose[:B, o, :3]) <= float(objs.radius[o]) * float(objs.radius[o])
                take = ok & (holder[:B, o] < 0) & ~released[:, o] & closed[gi] & (state["was_closed"][:B, gi] == 0) & ~holds[gi] & near
                rx = mat_t_vec(R[gi], pose[:B, o, :3] - pe[gi])
                rq = quat_mul(qe[gi] * np.array([1.0, -1.0, -1.0, -1.0]), pose[:B, o, 3:])
                rel[:B, o, :3][take] = rx[take]
                rel[:B, o, 3:][take] = rq[take]
                holder[:B, o][take] = gi
                state["grasp_tick"][:B, o][take] = t
                holds[gi] |= take
        for gi in range(len(G)):                          # 3. the edge detector
            state["was_closed"][:B, gi][ok] = closed[gi][ok]
        for mi, m in enumerate(objs.mates):               # 4. mates
            ps, qs = pose[:B, m.socket, :3], pose[:B, m.socket, 3:]
            tp = ps + mat_vec(quat2mat(qs), np.broadcast_to(np.asarray(m.seat_xyz, dtype=np.float64), (B, 3)))
            tq = quat_mul(qs, np.broadcast_to(np.asarray(m.seat_quat, dtype=np.float64), (B, 4)))
            qp = pose[:B, m.plug, 3:]
            dot = ((qp[:, 0] * tq[:, 0] + qp[:, 1] * tq[:, 1]) + qp[:, 2] * tq[:, 2]) + qp[:, 3] * tq[:, 3]
            hit = ok & (state["mated_tick"][:B, mi] < 0) & (holder[:B, m.plug] < 0)
            hit &= (_dist2(pose[:B, m.plug, :3], tp) <= float(m.tol_xyz) * float(m.tol_xyz)) & (np.abs(dot) >= float(m.min_abs_dot))
            state["mated_tick"][:B, mi][hit] = t
    return state


def ref_target(obj_pose, table_pose, xyz_obj: int, quat_obj: int):
    """The active arm's target a WP with refs gets at its entry (csrc/osc_action.hpp): obj_pose [B, nobj, 7] the objects of the tick,
    table_pose [B, 7] the list's pose words of the action (offset / grip rotation) -> [B, 7] float64: xyz = object xyz + offset (one add
    per word), quat = q_obj (x) q_grip; a ref of -1 leaves the table's words."""
    out = np.array(table_pose, dtype=np.float64)
    obj_pose = np.asarray(obj_pose, dtype=np.float64)
    if xyz_obj >= 0:
        out[:, :3] = obj_pose[:, xyz_obj, :3] + out[:, :3]
    if quat_obj >= 0:
        out[:, 3:] = quat_mul(obj_pose[:, quat_obj, 3:], np.array(table_pose, dtype=np.float64)[:, 3:])
    return out
