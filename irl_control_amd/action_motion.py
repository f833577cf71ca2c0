"""The MOTION of an action list: INTERP moves and seeded target noise (include/irlosc.h, "the motion of the list in force";
csrc/osc_action.hpp, csrc/osc_rng.hpp) -- the reference's second action-sequence file, action_sequence_configs/iros2022_task.yaml,
uses `action: INTERP` with `steps: N` and `noise: [mean, std]`, and ships no runner for it, so the semantics are this package's.

Everything here is the NumPy side of the kernel, one NumPy operation per rounded device operation, so that the bits agree:
  philox4x32_10, normal3        the counter-based generator and the Box-Muller triple (ln_rn, sincos_turn_rn: a log, a sine and a cosine
                                written out in add, multiply, divide and square root -- the device's own are not the host's)
  action_motion_state, action_motion_tick
                                the per-robot state and one tick of the kernel's MOTION form (action_sequence.action_list_tick's steps
                                with the motion's rules)
  compile_action_motion         INTERP / noise entries -> a WP sequence and the motion's arrays
  compile_iros2022              the iros2022 file's column-per-device entries -> a sequence in the insertion dialect"""
import copy
from typing import Dict, List

import numpy as np

from . import action_sequence as aseq

MAX_STEPS = 1 << 20
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_SQRT2, _LN2 = 1.4142135623730951, 0.6931471805599453
_K_TURN = 6.283185307179586 / 4294967296.0                    # 2 pi / 2^32
_INV33 = 1.0 / 8589934592.0                                   # 2^-33
_FACT = [1.0]
for _n in range(1, 21):
    _FACT.append(_FACT[-1] * _n)                              # n! up to 20!, each exact in a double


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11; the Random123 constants): counter [..., 4], key [..., 2] uint32 (broadcast
    against each other) -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32)
    c, k = np.broadcast_arrays(c, k[..., [0, 1, 0, 1]])
    c0, c1, c2, c3 = (c[..., i].astype(np.uint64) for i in range(4))
    k0, k1 = k[..., 0].astype(np.uint64), k[..., 1].astype(np.uint64)
    lo32 = np.uint64(0xFFFFFFFF)
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                           # 32 x 32 -> 64 bits
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & lo32, p0 & lo32, n0, n2
        k0, k1 = (k0 + np.uint64(_W0)) & lo32, (k1 + np.uint64(_W1)) & lo32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def ln_rn(x):
    """ln x for positive, finite, normal float64 x: ln_rn of csrc/osc_rng.hpp, bit for bit."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m >= _SQRT2
    m = np.where(big, m * 0.5, m)
    e = e + big
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = np.full(x.shape, 1.0 / 25.0)
    for k in range(23, 0, -2):
        p = p * s2 + 1.0 / float(k)
    return e.astype(np.float64) * _LN2 + (2.0 * s) * p


def sincos_poly_rn(a):
    """(sin a, cos a) for a in [0, pi/4]: the Taylor polynomials of csrc/osc_rng.hpp in Horner form."""
    a = np.asarray(a, dtype=np.float64)
    a2 = a * a
    ps = np.full(a.shape, -1.0 / _FACT[19])
    pc = np.full(a.shape, 1.0 / _FACT[20])
    for k in range(17, 0, -2):
        ps = ps * a2 + (-1.0 if k & 2 else 1.0) / _FACT[k]
    for k in range(18, -1, -2):
        pc = pc * a2 + (-1.0 if k & 2 else 1.0) / _FACT[k]
    return a * ps, pc


def sincos_turn_rn(w):
    """(sin, cos) of 2 pi w / 2^32 for uint32 w: the quadrant from the top two bits, the rest folded onto [0, pi/4] in integers."""
    w = np.asarray(w, dtype=np.uint32).astype(np.int64)
    quad, r = w >> 30, w & 0x3FFFFFFF
    fold = r > 0x20000000
    s, c = sincos_poly_rn(np.where(fold, 0x40000000 - r, r).astype(np.float64) * _K_TURN)
    s, c = np.where(fold, c, s), np.where(fold, s, c)
    return np.choose(quad, [s, c, -s, -c]), np.choose(quad, [c, -s, -c, s])


def normal3(seed: int, robot, draw, action):
    """Three standard normals per robot: Box-Muller on the Philox block of counter (robot, draw, action, 0) under key (seed's low word,
    its high word).  robot, draw, action: uint32, broadcast against each other -> [..., 3] float64 (normal3 of csrc/osc_rng.hpp)."""
    robot, draw, action = np.broadcast_arrays(np.asarray(robot, dtype=np.uint32), np.asarray(draw, dtype=np.uint32), np.asarray(action, dtype=np.uint32))
    ctr = np.stack([robot, draw, action, np.zeros_like(robot)], axis=-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))
    z = np.empty(robot.shape + (3,))
    u0 = (2.0 * w[..., 0].astype(np.float64) + 1.0) * _INV33
    r0 = np.sqrt(-2.0 * ln_rn(u0))
    s, c = sincos_turn_rn(w[..., 1])
    z[..., 0], z[..., 1] = r0 * c, r0 * s
    u1 = (2.0 * w[..., 2].astype(np.float64) + 1.0) * _INV33
    r1 = np.sqrt(-2.0 * ln_rn(u1))
    s, c = sincos_turn_rn(w[..., 3])
    z[..., 2] = r1 * c
    return z


def normal4(seed: int, robot, draw, block, stream):
    """Four standard normals per robot: Box-Muller on both word pairs of the Philox block of counter (robot, draw, block, stream) --
    z0 = r0 cos, z1 = r0 sin, z2 = r1 cos, z3 = r1 sin -> [..., 4] float64 (normal4 of csrc/osc_rng.hpp).  The fourth counter word
    names a stream: normal3 is the first three values of stream 0, a policy's Gaussian head (policy.sample) draws on stream 1."""
    robot, draw, block, stream = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint32) for v in (robot, draw, block, stream)))
    ctr = np.stack([robot, draw, block, stream], axis=-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))
    z = np.empty(robot.shape + (4,))
    for p in (0, 1):
        u = (2.0 * w[..., 2 * p].astype(np.float64) + 1.0) * _INV33
        r = np.sqrt(-2.0 * ln_rn(u))
        s, c = sincos_turn_rn(w[..., 2 * p + 1])
        z[..., 2 * p], z[..., 2 * p + 1] = r * c, r * s
    return z


# ---- the motion as data -------------------------------------------------------------------------------------------------------------
def action_motion_state(B: int, draw0=None) -> Dict:
    """The per-robot state of a motion as irlosc_set_action_motion resets it: step 0, draws = draw0 (default zeros), origin and goal 0."""
    draws = np.zeros(B, np.uint32) if draw0 is None else np.array(draw0, dtype=np.uint32).reshape(B)
    return dict(step=np.zeros(B, np.int32), draws=draws, origin=np.zeros((B, 7)), goal=np.zeros((B, 7)))


def make_motion(A: int, steps=None, noise_mean=None, noise_std=None, seed: int = 0) -> Dict:
    """The motion dict of a list of A actions: steps int32 [A], noise_mean, noise_std float64 [A] (None: zeros), seed."""
    def arr(v, dt):
        a = np.zeros(A, dt) if v is None else np.array(v, dtype=dt).reshape(-1)
        if len(a) != A:
            raise ValueError(f"expected one entry per action ({A}), got {len(a)}")
        return a
    return dict(steps=arr(steps, np.int32), noise_mean=arr(noise_mean, np.float64), noise_std=arr(noise_std, np.float64), seed=int(seed))


def compile_action_motion(sequence: List[Dict]):
    """A sequence that may hold `action: INTERP` entries (with `steps: N`) and `noise: [mean, std]` on WP / INTERP entries ->
    (wp_sequence, motion): the same sequence with every INTERP as a WP (so the WP defaults apply to it) and without the two keys --
    what compile_action_list and set_action_list take -- and make_motion's dict for set_action_motion (seed 0)."""
    A = len(sequence)
    motion = make_motion(A)
    out = []
    for a, entry in enumerate(sequence):
        e = copy.deepcopy(entry)
        steps, noise = e.pop("steps", None), e.pop("noise", None)
        if e["action"] == "INTERP":
            if steps is None or int(steps) < 1:
                raise ValueError(f"action {a}: an INTERP needs steps >= 1, got {steps}")
            e["action"] = "WP"
            motion["steps"][a] = int(steps)
        elif steps is not None:
            raise ValueError(f"action {a}: steps on a {e['action']}")
        if noise is not None:
            if e["action"] != "WP":
                raise ValueError(f"action {a}: noise on a {e['action']}")
            motion["noise_mean"][a], motion["noise_std"][a] = float(noise[0]), float(noise[1])
        out.append(e)
    return out, motion


def compile_iros2022(config: Dict, sequences, active_arm: str = "right") -> List[Dict]:
    """The iros2022 file (action_sequence_configs/iros2022_task.yaml of the reference; a copy: tests/golden/iros2022_task.yaml) gives a
    column per device where the insertion file gives one value: `target_xyz` / `target_quat` are [per device][3 | 4], or name an
    attribute of an action object (`male_object.hover_offset`), itself a column per device.  -> the listed sequences (names of the
    file's keys, in order) as ONE sequence in the insertion dialect, for the active arm: its column of every target (the device order
    is the file's device_config.devices), a named attribute's column taken as written, target_quat taken as given (w x y z, not
    normalised).  The passive arm keeps its pose, as lists do.  INTERP / steps / noise stay: compile_action_motion takes them."""
    devices = list(config["device_config"]["devices"])
    col = devices.index("ur5right" if active_arm == "right" else "ur5left")
    objects = next((v for k, v in config.items() if k.endswith("action_objects")), {})

    def column(v):
        if isinstance(v, str):
            obj, attr = v.split(".")
            v = objects[obj][attr]
        if len(v) == len(devices) and all(isinstance(r, (list, tuple)) for r in v):
            v = v[col]
        return [float(x) for x in v]

    out = []
    for name in sequences:
        for entry in (config[name] if isinstance(name, str) else name):
            e = copy.deepcopy(entry)
            for key in ("target_xyz", "target_quat"):
                if key in e:
                    e[key] = column(e[key])
            out.append(e)
    return out


# ---- one tick of the kernel's MOTION form -------------------------------------------------------------------------------------------
def _norm4(q):
    return np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def interp_pose(origin, goal, step: int, N: int):
    """The target of an INTERP on its tick `step` of N (step < N): xyz_c = origin_c + w (goal_c - origin_c), w = step / N, and the nlerp
    of the two quaternions on the short arc (quat_nlerp_rn of csrc/osc_action.hpp) -> [7] float64."""
    o, g = np.asarray(origin, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    out = np.empty(7)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.float64(step) / np.float64(N)
        out[:3] = o[:3] + w * (g[:3] - o[:3])
        qa, qb = o[3:] / _norm4(o[3:]), g[3:] / _norm4(g[3:])
        dot = ((qa[0] * qb[0] + qa[1] * qb[1]) + qa[2] * qb[2]) + qa[3] * qb[3]
        if dot < 0.0:
            qb = -qb
        r = qa + w * (qb - qa)
        out[3:] = r / _norm4(r)
    return out


def action_motion_tick(state: Dict, ee, tgt, gains, desc: Dict, t: int, motion: Dict, refs: Dict = None, obj_pose=None):
    """One tick of the action kernel's MOTION form in NumPy, in place: action_sequence.action_list_tick's arguments and steps, plus
      motion    make_motion's / compile_action_motion's dict, with motion["state"] = action_motion_state(B) (made on first use)
      refs      dict(xyz_obj, quat_obj) of set_action_refs, with obj_pose [B, nobj, 7] the objects' poses of this tick; or None
    and the rules of include/irlosc.h: a WP's goal is kept in float64, gets its noise, is stored with the origin; an INTERP's target
    travels; an INTERP advances only when it has arrived."""
    from .objects import ref_target
    WP = aseq.Action.WP.value
    A, ia, io = desc["n_actions"], desc["active_dev"], desc["passive_dev"]
    ee = np.asarray(ee, dtype=np.float64)
    B = len(ee)
    st = state
    ms = motion.setdefault("state", action_motion_state(len(st["action"])))
    steps, mean, std, seed = motion["steps"], motion["noise_mean"], motion["noise_std"], motion["seed"]
    first = st["entered"][:B] < 0
    if not first.all():
        live = (st["action"][:B] < A) & ~first
        e = np.linalg.norm(aseq._calc_error_batch(ee[:, ia], np.asarray(tgt[:B, ia], dtype=np.float64)), axis=1)
        for b in np.nonzero(live)[0]:
            a = st["action"][b]
            st["err"][b] = e[b]
            if desc["kind"][a] == WP:
                nxt = st["err"][b] <= desc["max_error"][a] and (steps[a] == 0 or ms["step"][b] == steps[a])
            else:
                st["grip_left"][b] -= 1
                nxt = st["grip_left"][b] <= 0
            if nxt:
                st["action"][b] += 1
                if st["action"][b] == A:
                    st["finished_tick"][b] = t
    st["start_xyz"][:B][first] = ee[first, ia, :3]
    pose = desc["pose"]
    for b in range(B):
        a = st["action"][b]
        if a >= A:
            continue
        wp = desc["kind"][a] == WP
        if st["entered"][b] != a:
            st["entered"][b] = a
            st["gripper_force"][b] = desc["gripper_force"][a]
            if wp:
                if io >= 0:
                    tgt[b, io, :3] = ee[b, io, :3]
                    tgt[b, io, 3:] = ee[b, io, 3:] if desc["passive_hold_orientation"] else desc["passive_quat"]
                g = np.array(pose[b if len(pose) > 1 else 0, a], dtype=np.float64)
                if refs is not None and obj_pose is not None:
                    g = ref_target(np.asarray(obj_pose)[b:b + 1], g[None], int(refs["xyz_obj"][a]), int(refs["quat_obj"][a]))[0]
                if desc["xyz_from_start"][a]:
                    g[:3] = st["start_xyz"][b]
                if std[a] > 0.0 or mean[a] != 0.0:
                    z = normal3(seed, b, ms["draws"][b], a)
                    g[:3] = g[:3] + (np.float64(mean[a]) + np.float64(std[a]) * z)
                    ms["draws"][b] = np.uint32((int(ms["draws"][b]) + 1) & 0xFFFFFFFF)
                ms["goal"][b], ms["origin"][b], ms["step"][b] = g, ee[b, ia], 0
                if steps[a] == 0:
                    tgt[b, ia] = g
                st["err"][b] = np.inf
            else:
                st["grip_left"][b] = desc["grip_ticks"][a]
        if wp and steps[a] >= 1 and ms["step"][b] < steps[a]:
            ms["step"][b] += 1
            tgt[b, ia] = interp_pose(ms["origin"][b], ms["goal"][b], ms["step"][b], steps[a]) if ms["step"][b] < steps[a] else ms["goal"][b]
        if wp:
            with np.errstate(invalid="ignore"):
                st["max_vel0"][b] = max(desc["min_speed"][a], min(desc["max_speed"][a], desc["kp"][a] * st["err"][b]))
            if gains is not None:
                gains[b, ia, 9] = st["max_vel0"][b]
    return state
