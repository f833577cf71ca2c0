"""Joint rows of a rollout (BatchedOSC.set_joints, include/irlosc.h: irlosc_set_joints), restated in NumPy: the descriptor arrays and the
table the library takes, and the torque of a tick with the rounding order of csrc/osc_joint.hpp -- every product, add and subtract a
float64 operation of its own, per hinge the rows' contributions summed in ascending row index, the first taken as it is -- so that a host
loop can repeat a rollout's joint torques bit for bit."""
import json

import numpy as np

MAX_JOINT_ROWS = 48
ROW = 8
LIMIT, COUPLE, DRIVE = 0, 1, 2
CONST, ACTION = 0, 1
_KINDS = {"limit": LIMIT, "couple": COUPLE, "drive": DRIVE}
_SOURCES = {"const": CONST, "action": ACTION}
_KEYS = {LIMIT: {"kind", "joint", "lo", "hi", "stiffness", "damping"},
         COUPLE: {"kind", "joint", "joint_b", "a0", "a1", "qa0", "qb0", "stiffness", "damping"},
         DRIVE: {"kind", "joint", "gear", "value", "source", "dev"}}


def _value(v, B, what):
    """A scalar, or one value per robot [B] -> ([B or 1] float64, per robot?)"""
    a = np.asarray(v, dtype=np.float64)
    if a.shape == ():
        return a[None], False
    if a.shape == (B,):
        return a, True
    raise ValueError(f"{what}: expected a scalar or shape {(B,)}, got {a.shape}")


def _index(v, names, what):
    if isinstance(v, str):
        if v not in names:
            raise ValueError(f"{what}: {v!r} is not one of {list(names)}")
        return list(names).index(v)
    if not 0 <= int(v) < len(names):
        raise ValueError(f"{what}: index {v!r} out of [0, {len(names)})")
    return int(v)


def normalise(rows, joint_names, dev_names, B):
    """rows: a list of dicts, hinges by name or index, values scalars or per-robot arrays [B]:
        dict(kind="limit",  joint=, lo=, hi=, stiffness=, damping=0)
        dict(kind="couple", joint=, joint_b=, a1=, a0=0, qa0=0, qb0=0, stiffness=, damping=0)       joint: MuJoCo's joint1 (the dependent
                                                                                                     y), joint_b: its joint2 (the x)
        dict(kind="drive",  joint=, gear=1, source="const", value=0)  |  dict(kind="drive", joint=, gear=1, source="action", dev=)
    -> (desc, table): desc = dict(kind, joint_a, joint_b, source, dev: int32 [R]; per_robot: bool), table [B or 1, R, 8] float64 with rows
    lo hi k c | a0 a1 qa0 qb0 k c | gear value (zero padded).  Checked as the library checks."""
    jn, dn = list(joint_names), list(dev_names)
    R = len(rows)
    if not 1 <= R <= MAX_JOINT_ROWS:
        raise ValueError(f"a slot holds 1 to {MAX_JOINT_ROWS} joint rows, got {R}")
    if B < 1:
        raise ValueError(f"B={B} must be >= 1")
    desc = {k: np.zeros(R, np.int32) for k in ("kind", "joint_a", "joint_b", "source", "dev")}
    cols, per = [], False
    for r, d in enumerate(rows):
        w = f"joints[{r}]"
        kind = d.get("kind")
        kind = _KINDS.get(kind, kind) if isinstance(kind, str) else kind
        if kind not in (LIMIT, COUPLE, DRIVE):
            raise ValueError(f"{w}: unknown kind {d.get('kind')!r}")
        unknown = set(d) - _KEYS[kind]
        if unknown:
            raise ValueError(f"{w}: unknown keys {sorted(unknown)}")
        if "joint" not in d:
            raise ValueError(f"{w}: joint= is missing")
        desc["kind"][r] = kind
        desc["joint_a"][r] = _index(d["joint"], jn, f"{w}.joint")
        if kind == LIMIT:
            for key in ("lo", "hi", "stiffness"):
                if key not in d:
                    raise ValueError(f"{w}: {key}= is missing")
            vals = [("lo", d["lo"]), ("hi", d["hi"]), ("stiffness", d["stiffness"]), ("damping", d.get("damping", 0.0))]
        elif kind == COUPLE:
            for key in ("joint_b", "a1", "stiffness"):
                if key not in d:
                    raise ValueError(f"{w}: {key}= is missing")
            desc["joint_b"][r] = _index(d["joint_b"], jn, f"{w}.joint_b")
            if desc["joint_b"][r] == desc["joint_a"][r]:
                raise ValueError(f"{w}: couples hinge {d['joint']!r} with itself")
            vals = [("a0", d.get("a0", 0.0)), ("a1", d["a1"]), ("qa0", d.get("qa0", 0.0)), ("qb0", d.get("qb0", 0.0)),
                    ("stiffness", d["stiffness"]), ("damping", d.get("damping", 0.0))]
        else:
            src = d.get("source", "const")
            src = _SOURCES.get(src, src) if isinstance(src, str) else src
            if src not in (CONST, ACTION):
                raise ValueError(f"{w}: unknown source {d.get('source')!r}")
            desc["source"][r] = src
            if src == ACTION:
                if "dev" not in d:
                    raise ValueError(f"{w}: an action drive names its device, dev=")
                if "value" in d:
                    raise ValueError(f"{w}: an action drive takes no value=")
                desc["dev"][r] = _index(d["dev"], dn, f"{w}.dev")
            elif "dev" in d:
                raise ValueError(f"{w}: a const drive takes no dev=")
            vals = [("gear", d.get("gear", 1.0)), ("value", d.get("value", 0.0))]
        col = []
        for nm, v in vals:
            a, p = _value(v, B, f"{w}.{nm}")
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{w}.{nm} holds a value that is not finite")
            if nm in ("stiffness", "damping") and np.any(a < 0.0):
                raise ValueError(f"{w}.{nm} must be >= 0")
            per = per or p
            col.append(a)
        if kind == LIMIT and not np.all(col[0] < col[1]):
            raise ValueError(f"{w}: lo must be < hi")
        cols.append(col)
    desc["per_robot"] = bool(per)
    table = np.zeros((B if per else 1, R, ROW))
    for r, col in enumerate(cols):
        for i, a in enumerate(col):
            table[:, r, i] = a
    return desc, table


def joint_torque(qpos, qvel, desc, table, ctrl, gripper_force=None, active=None, with_active=False):
    """The joint rows' torque of one tick (csrc/osc_joint.hpp): qpos, qvel [B, n] the coordinates at the start of the tick, desc / table as
    normalise returns them, ctrl [B, R] the drives' state before the tick.  gripper_force [B] is the action state's gripper_force AFTER
    this tick's action kernel and active the list's active device index; None: no list in force.
    -> (tau [B, n], ctrl' [B, R], violation [B, R]: max(g_lo, g_hi) of a LIMIT (positive: outside), |e| of a COUPLE, 0 of a DRIVE);
    with_active: and active [B, R] bool, the rows with a non-zero contribution on this tick (what active_ticks counts)."""
    q = np.asarray(qpos, dtype=np.float64)
    qd = np.asarray(qvel, dtype=np.float64)
    B, n = q.shape
    t = np.broadcast_to(np.asarray(table, dtype=np.float64), (B,) + np.shape(table)[1:])
    R = t.shape[1]
    ctrl = np.array(ctrl, dtype=np.float64).reshape(B, R)
    tau = np.zeros((B, n))
    viol = np.zeros((B, R))
    on = np.zeros((B, R), bool)
    seen = np.zeros(n, bool)
    fmax = np.finfo(np.float64).max

    def add(j, x):
        tau[:, j] = tau[:, j] + x if seen[j] else x
        seen[j] = True

    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            a, b, row = int(desc["joint_a"][r]), int(desc["joint_b"][r]), t[:, r]
            if desc["kind"][r] == LIMIT:
                lo, hi, k, c = row[:, 0], row[:, 1], row[:, 2], row[:, 3]
                g_lo, g_hi = lo - q[:, a], q[:, a] - hi
                cqd = c * qd[:, a]
                f_lo, f_hi = k * g_lo - cqd, k * g_hi + cqd
                t_lo = np.where((g_lo > 0.0) & (f_lo > 0.0), f_lo, 0.0)
                t_hi = np.where((g_hi > 0.0) & (f_hi > 0.0), f_hi, 0.0)
                add(a, t_lo - t_hi)
                on[:, r] = (t_lo - t_hi) != 0.0
                viol[:, r] = np.where(g_lo > g_hi, g_lo, g_hi)
            elif desc["kind"][r] == COUPLE:
                a0, a1, qa0, qb0, k, c = (row[:, i] for i in range(6))
                e = (q[:, a] - qa0) - (a0 + a1 * (q[:, b] - qb0))
                de = qd[:, a] - a1 * qd[:, b]
                f = k * e + c * de
                ok = np.abs(f) <= fmax
                p = a1 * f
                add(a, np.where(ok, -f, 0.0))
                add(b, np.where(ok & (np.abs(p) <= fmax), p, 0.0))
                viol[:, r] = np.abs(e)
                on[:, r] = ok & (f != 0.0)
            else:
                gear = row[:, 0]
                if desc["source"][r] == CONST:
                    cr = row[:, 1].copy()
                else:
                    cr = ctrl[:, r].copy()
                    if gripper_force is not None and active is not None and int(desc["dev"][r]) == int(active):
                        gf = np.asarray(gripper_force, dtype=np.float64)
                        cr = np.where(gf != 0.0, gf, cr)
                ctrl[:, r] = cr
                p = gear * cr
                x = np.where((np.abs(cr) <= fmax) & (np.abs(p) <= fmax), p, 0.0)
                add(a, x)
                on[:, r] = x != 0.0
    return (tau, ctrl, viol, on) if with_active else (tau, ctrl, viol)


def load_fixture(path):
    with open(path) as f:
        return json.load(f)


def scene_rows(fixture, limit_k, limit_c, couple_k, couple_c, gear=1.0, drive="action", devices=("ur5right", "ur5left")):
    """The full joint-row set of the scene `fixture` describes (tests/golden/dual_ur5_joints.json, or its path; written by
    tools/parse_mjcf.py --joints): a LIMIT per limited hinge in the fixture's order, a COUPLE per equality row, a DRIVE per gripper motor
    (gear x the fixture's gear).  drive="action": the motors follow the action list of their arm (devices: the layout's devices that
    own a motor, matched by the suffix of the motor's joint name; a motor of none of them gets no drive); a number: CONST drives of
    that value; None: no drives.  Dual-UR5: 24 + 10 + 2 = 36 rows."""
    fx = load_fixture(fixture) if isinstance(fixture, str) else fixture
    rows = []
    for name, j in fx["joints"].items():
        if j["limited"]:
            rows.append(dict(kind="limit", joint=name, lo=j["range"][0], hi=j["range"][1], stiffness=limit_k, damping=limit_c))
    for e in fx["equality"]:
        rows.append(dict(kind="couple", joint=e["joint1"], joint_b=e["joint2"], a0=e["polycoef"][0], a1=e["polycoef"][1],
                         qa0=e["qpos0"][0], qb0=e["qpos0"][1], stiffness=couple_k, damping=couple_c))
    for m in fx["gripper_motors"] if drive is not None else []:
        if drive == "action":
            dev = [d for d in devices if m["joint"].endswith(d)]
            if len(dev) != 1:
                continue
            rows.append(dict(kind="drive", joint=m["joint"], gear=gear * m["gear"], source="action", dev=dev[0]))
        else:
            rows.append(dict(kind="drive", joint=m["joint"], gear=gear * m["gear"], source="const", value=drive))
    return rows
