"""Compliant walls of a rollout (BatchedOSC.set_walls, include/irlosc.h: irlosc_set_walls), restated in NumPy: the table the library
takes, and the penalty force of a tick with the rounding order of csrc/osc_wall.hpp -- every product, add and subtract a float64
operation of its own, sums left to right -- so that a host loop can repeat a rollout's wall forces bit for bit."""
import numpy as np

MAX_WALLS = 8
ROW = 8      # nx ny nz off r k c 0


def _per_robot(v, B, shape, what):
    """A scalar / [*shape] value, or one per robot [B, *shape] -> ([B or 1, *shape] float64, per robot?)"""
    a = np.asarray(v, dtype=np.float64)
    if a.shape == shape:
        return a[None], False
    if a.shape == (B,) + shape:
        return a, True
    raise ValueError(f"{what}: expected shape {shape} or {(B,) + shape}, got {a.shape}")


def normalise(walls, dev_names, B):
    """walls: a list of dict(dev=name_or_index, normal=(nx, ny, nz), offset= | point=, radius=0, stiffness=, damping=0) -> (dev [W] int32,
    table [nb, W, 8] float64 with rows nx ny nz off r k c 0; nb = B when any value is given per robot, else 1).  `normal` is a unit
    vector of the world frame (it is not rescaled) and n.x >= offset the free side; `point=` names a point on the wall instead of the
    offset (offset = n.point).  Values are scalars (vectors) or arrays with a leading axis of B robots.  Checked as the library checks."""
    names = list(dev_names)
    W = len(walls)
    if not 1 <= W <= MAX_WALLS:
        raise ValueError(f"a slot holds 1 to {MAX_WALLS} walls, got {W}")
    if B < 1:
        raise ValueError(f"B={B} must be >= 1")
    dev = np.zeros(W, np.int32)
    rows, per = [], False
    for w, d in enumerate(walls):
        unknown = set(d) - {"dev", "normal", "offset", "point", "radius", "stiffness", "damping"}
        if unknown:
            raise ValueError(f"walls[{w}]: unknown keys {sorted(unknown)}")
        dv = d["dev"]
        if isinstance(dv, str):
            if dv not in names:
                raise ValueError(f"walls[{w}]: device {dv!r} is not one of {names}")
            dev[w] = names.index(dv)
        else:
            dev[w] = int(dv)
        if not 0 <= dev[w] < len(names):
            raise ValueError(f"walls[{w}]: device {dv!r} is not one of {names}")
        if ("offset" in d) == ("point" in d):
            raise ValueError(f"walls[{w}]: give offset= or point=, one of them")
        if "stiffness" not in d:
            raise ValueError(f"walls[{w}]: stiffness= is missing")
        n, pn = _per_robot(d["normal"], B, (3,), f"walls[{w}].normal")
        if "offset" in d:
            off, po = _per_robot(d["offset"], B, (), f"walls[{w}].offset")
        else:
            pt, po = _per_robot(d["point"], B, (3,), f"walls[{w}].point")
            nn, pt = np.broadcast_arrays(n, pt)
            off = nn[:, 0] * pt[:, 0] + nn[:, 1] * pt[:, 1] + nn[:, 2] * pt[:, 2]
            po = po or pn
        r, pr = _per_robot(d.get("radius", 0.0), B, (), f"walls[{w}].radius")
        k, pk = _per_robot(d["stiffness"], B, (), f"walls[{w}].stiffness")
        c, pc = _per_robot(d.get("damping", 0.0), B, (), f"walls[{w}].damping")
        for nm, v in (("normal", n), ("offset", off), ("radius", r), ("stiffness", k), ("damping", c)):
            if not np.all(np.isfinite(v)):
                raise ValueError(f"walls[{w}].{nm} holds a value that is not finite")
        if np.any(np.abs((n * n).sum(axis=1) - 1.0) > 1e-12):
            raise ValueError(f"walls[{w}].normal is no unit vector")
        for nm, v in (("radius", r), ("stiffness", k), ("damping", c)):
            if np.any(v < 0.0):
                raise ValueError(f"walls[{w}].{nm} must be >= 0")
        per = per or pn or po or pr or pk or pc
        rows.append((n, off, r, k, c))
    nb = B if per else 1
    table = np.zeros((nb, W, ROW))
    for w, (n, off, r, k, c) in enumerate(rows):
        table[:, w, :3], table[:, w, 3], table[:, w, 4], table[:, w, 5], table[:, w, 6] = n, off, r, k, c
    return dev, table


def depth(x, rows):
    """g = r - ((n0 x0 + n1 x1 + n2 x2) - off) per wall: x [B, 3], rows [B or 1, W, 8] -> [B, W]."""
    x = np.asarray(x, dtype=np.float64)[:, None, :]
    rows = np.asarray(rows, dtype=np.float64)
    nx = (rows[..., 0] * x[..., 0] + rows[..., 1] * x[..., 1]) + rows[..., 2] * x[..., 2]
    return rows[..., 4] - (nx - rows[..., 3])


def contact_force(x, v, rows):
    """The summed force of the walls of one device on its EE (csrc/osc_wall.hpp): x [B, 3] the EE position, v [B, 3] its velocity (or
    0), rows [B or 1, W, 8] the device's walls in ascending w -> F [B, 3].  Per wall g = r - ((n.x) - off), s = n.v, f = k g - c s,
    F_w = f n where g > 0 and f > 0, else 0 (a wall never pulls; a NaN gives no contact); F = F_0 + F_1 + ... left to right."""
    x = np.asarray(x, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), x.shape)[:, None, :]
    g = depth(x, rows)
    with np.errstate(invalid="ignore"):
        s = (rows[..., 0] * v[..., 0] + rows[..., 1] * v[..., 1]) + rows[..., 2] * v[..., 2]
        f = rows[..., 5] * g - rows[..., 6] * s
        on = (g > 0.0) & (f > 0.0)
        Fw = np.where(on[..., None], f[..., None] * rows[..., :3], 0.0)      # [B, W, 3]
    F = Fw[:, 0].copy()
    for w in range(1, Fw.shape[1]):
        F = F + Fw[:, w]
    return F
