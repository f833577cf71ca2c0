"""The NumPy side of a rollout's reward (BatchedOSC.set_reward, csrc/osc_reward.hpp; include/irlosc.h, "a reward per tick"): the term
builder, and a mirror of the reward kernel that repeats its arithmetic operation by operation -- every product, sum, difference and square
root is one float64 NumPy operation, in the kernel's order -- so that the device's r, ret, gret, steps, hold and goal_step are held to it
bit for bit (tests/test_reward.py).

A POINT is (kind, index): ee(d), target(d), obj(o), fixed(p).  A TERM is (kind, a, b, weight) built by dist_sq, dist, ori, act_sq, u_sq,
force, mated, one.  Reward(terms, gamma, points, goal, ...) is the description."""
from dataclasses import dataclass

import numpy as np

from . import _lib

EE, TARGET, OBJECT, FIXED = _lib.REWARD_EE, _lib.REWARD_TARGET, _lib.REWARD_OBJECT, _lib.REWARD_FIXED
DIST_SQ, DIST, ORI, ACT_SQ, U_SQ, FORCE, MATED, ONE = range(8)
_ZERO = (0, 0)


def ee(d: int):
    """The EE pose of device d: the words IRLOSC_LOG_EE_POSE logs."""
    return (EE, int(d))


def target(d: int):
    """The slot's target row of device d as the tick's OSC step read it."""
    return (TARGET, int(d))


def obj(o: int):
    """The pose of action object o as the tick's object kernel left it."""
    return (OBJECT, int(o))


def fixed(p: int):
    """Row p of the reward's points (no orientation)."""
    return (FIXED, int(p))


def dist_sq(a, b, weight: float):
    return (DIST_SQ, a, b, float(weight))


def dist(a, b, weight: float):
    return (DIST, a, b, float(weight))


def ori(a, b, weight: float):
    """1 - |q_a . q_b|: 0 where the two orientations agree."""
    return (ORI, a, b, float(weight))


def act_sq(weight: float):
    """The squared norm of the policy's action of the tick (act of a Gaussian head, else out)."""
    return (ACT_SQ, _ZERO, _ZERO, float(weight))


def u_sq(weight: float):
    """The squared norm of the tick's torques."""
    return (U_SQ, _ZERO, _ZERO, float(weight))


def force(d: int, weight: float):
    """The norm of the force device d's sensor feed read on the tick."""
    return (FORCE, (0, int(d)), _ZERO, float(weight))


def mated(m: int, weight: float):
    """1 while mate m of the slot's action objects is mated."""
    return (MATED, (0, int(m)), _ZERO, float(weight))


def one(weight: float):
    """A constant per tick (a time cost, or an alive bonus)."""
    return (ONE, _ZERO, _ZERO, float(weight))


@dataclass
class Reward:
    """terms: up to 8 built by the functions above; gamma in [0, 1]; points: [P, 3] for the fleet or [B, P, 3] per robot (P <= 8);
    goal_term: the term whose value the goal compares (-1: no goal), goal_cmp "<=" or ">=", goal_value, goal_hold H >= 1 ticks."""
    terms: list
    gamma: float = 1.0
    points: object = None
    goal_term: int = -1
    goal_cmp: str = "<="
    goal_value: float = 0.0
    goal_hold: int = 1

    def n_points(self) -> int:
        return 0 if self.points is None else int(np.asarray(self.points).shape[-2])

    def per_robot(self) -> bool:
        return self.points is not None and np.asarray(self.points).ndim == 3

    def desc(self) -> "_lib.Reward":
        """struct irlosc_reward of this description (ranges are the library's to check)."""
        if len(self.terms) > _lib.MAX_REWARD_TERMS:
            raise ValueError(f"a reward has at most {_lib.MAX_REWARD_TERMS} terms, got {len(self.terms)}")
        if self.goal_cmp not in ("<=", ">="):
            raise ValueError(f"goal_cmp={self.goal_cmp!r} must be '<=' or '>='")
        if self.points is not None and (np.asarray(self.points).ndim not in (2, 3) or np.asarray(self.points).shape[-1] != 3):
            raise ValueError("points: expected [P, 3] or [B, P, 3]")
        d = _lib.Reward()
        d.n_terms, d.n_points, d.points_per_robot = len(self.terms), self.n_points(), int(self.per_robot())
        d.goal_term, d.goal_cmp, d.goal_hold = int(self.goal_term), int(self.goal_cmp == ">="), int(self.goal_hold)
        d.gamma, d.goal_value = float(self.gamma), float(self.goal_value)
        for i, (kind, a, b, w) in enumerate(self.terms):
            d.kind[i], d.a_kind[i], d.a_index[i], d.b_kind[i], d.b_index[i], d.weight[i] = kind, a[0], a[1], b[0], b[1], w
        return d


def reward_state(B: int) -> dict:
    """The fresh per-robot state: what set_reward and a reset of episodes leave."""
    return dict(r=np.zeros(B), ret=np.zeros(B), gret=np.zeros(B), disc=np.ones(B), steps=np.zeros(B, np.int32),
                hold=np.zeros(B, np.int32), goal_step=np.full(B, -1, np.int32))


def _word(kind, index, c, ee_pose, targets, object_pose, points):
    """Word c (0..2 position, 3..6 quaternion w x y z) of a point, [B] float64 (a FIXED point of the fleet: one float64)."""
    if kind == EE:
        return np.asarray(ee_pose, dtype=np.float64)[:, index, c]
    if kind == TARGET:
        return np.asarray(targets)[:, index, c].astype(np.float64)
    if kind == OBJECT:
        return np.asarray(object_pose, dtype=np.float64)[:, index, c]
    p = np.asarray(points, dtype=np.float64)
    return p[:, index, c] if p.ndim == 3 else p[index, c]      # (the fleet's point: a scalar, broadcast)


def _B(*arrays):
    for a in arrays:
        if a is not None:
            return len(a)
    raise ValueError("the mirror needs one per-robot array to know B")


def _sq3(x, y, z):
    s = x * x
    s = s + y * y
    return s + z * z


def term_values(rw: Reward, ee_pose=None, targets=None, u=None, wrench=None, object_pose=None, act=None, mated_tick=None) -> np.ndarray:
    """v[i, b] of every term on one tick.  ee_pose [B, ndev, 7] float64; targets [B, ndev, 7], u [B, n], wrench [B, ndev, 6] in the
    context's dtype (widened exactly here); object_pose [B, nobj, 7+]; act [B, n_out] float32; mated_tick [B, nm] int."""
    B = _B(ee_pose, targets, u, wrench, object_pose, act, mated_tick)
    v = np.empty((len(rw.terms), B), dtype=np.float64)
    src = (ee_pose, targets, object_pose, rw.points)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (kind, a, b, _) in enumerate(rw.terms):
            if kind in (DIST_SQ, DIST):
                d = [_word(a[0], a[1], c, *src) - _word(b[0], b[1], c, *src) for c in range(3)]
                s = _sq3(*d)
                v[i] = np.sqrt(s) if kind == DIST else s
            elif kind == ORI:
                d = _word(a[0], a[1], 3, *src) * _word(b[0], b[1], 3, *src)
                for c in range(4, 7):
                    d = d + _word(a[0], a[1], c, *src) * _word(b[0], b[1], c, *src)
                v[i] = 1.0 - np.abs(d)
            elif kind in (ACT_SQ, U_SQ):
                x = np.asarray(act if kind == ACT_SQ else u).astype(np.float64)
                s = np.zeros(B)
                for c in range(x.shape[1]):
                    s = s + x[:, c] * x[:, c]
                v[i] = s
            elif kind == FORCE:
                w = np.asarray(wrench)[:, a[1], :3].astype(np.float64)
                v[i] = np.sqrt(_sq3(w[:, 0], w[:, 1], w[:, 2]))
            elif kind == MATED:
                v[i] = np.where(np.asarray(mated_tick)[:, a[1]] >= 0, 1.0, 0.0)
            else:
                v[i] = 1.0
    return v


def accumulate(rw: Reward, state: dict, r: np.ndarray, v_goal=None) -> dict:
    """One tick of the accumulation on a tick's reward r [B] (and the goal term's values): -> the new state.  `state` is not modified."""
    st = {k: np.array(x, copy=True) for k, x in state.items()}
    with np.errstate(invalid="ignore", over="ignore"):
        st["r"] = np.array(r, dtype=np.float64)
        st["steps"] = st["steps"] + np.int32(1)
        st["ret"] = st["ret"] + st["r"]
        st["gret"] = st["gret"] + st["disc"] * st["r"]
        st["disc"] = st["disc"] * np.float64(rw.gamma)
        if rw.goal_term >= 0:
            met = (v_goal >= rw.goal_value) if rw.goal_cmp == ">=" else (v_goal <= rw.goal_value)      # (a NaN compares false)
            st["hold"] = np.where(met, st["hold"] + 1, 0).astype(np.int32)
            first = (st["hold"] >= rw.goal_hold) & (st["goal_step"] < 0)
            st["goal_step"] = np.where(first, st["steps"], st["goal_step"]).astype(np.int32)
    return st


def reward_tick(rw: Reward, state: dict, **sources) -> dict:
    """The reward kernel's tick on the host: the terms' values from `sources` (term_values' arguments), r = 0.0; r = r + weight_i v_i,
    then the accumulation and the goal.  -> the new state (with "v": the terms' values [n_terms, B])."""
    v = term_values(rw, **sources)
    r = np.zeros(v.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for i, term in enumerate(rw.terms):
            r = r + np.float64(term[3]) * v[i]
    st = accumulate(rw, {k: x for k, x in state.items() if k != "v"}, r, v[rw.goal_term] if rw.goal_term >= 0 else None)
    st["v"] = v
    return st
