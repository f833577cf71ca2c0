"""Compliant walls of a rollout (-m gpu): irlosc_set_walls -- penalty half-spaces on EE bodies whose force is computed on the device
from the EE position and velocity of the tick's walk, applied to the plant in front of the plant kernel and taken off the sensor
feed's wrench a tick later (csrc/osc_wall.hpp) -- against the CPU oracle, against pushes that carry the same force, against the NumPy
restatement, against runs without walls, against itself tick by tick and in pieces, next to programs and pushes, the state rules, and
the example.

The helpers are those of test_pushes.py / test_rollout.py / test_rollout_layouts.py; the force of a tick is irl_control_amd/walls.py's
(held by tests/test_walls_host.py)."""
import ctypes as C
import time

import numpy as np
import pytest

import test_action_list as tal
import test_pushes as tp
import test_rollout as tr
import test_rollout_layouts as trl
import test_waypoints as tw
from irl_control_amd import BatchedOSC, _lib, synth, walls as wl
from irl_control_amd.rigid_body import DUAL_UR5_EE, RigidBodyModel
from oracle import rigid_body as rb

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
NS, DT = tr.NS, 1e-3
ERR_ARG, ERR_STATE = tr.ERR_ARG, tr.ERR_STATE
BAD = _lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD
B0 = 130                 # two full walk waves and a ragged one of two lanes
KEYS = ("qpos", "qvel", "u", "flags_any")
STATE = ("force", "max_depth", "contact_ticks", "first_tick")
N_Y, N_X = (0.0, -1.0, 0.0), (1.0, 0.0, 0.0)      # the reference wall's normal, and one across it
R1, K1, C1 = 0.05, 900.0, 400.0
same = tp.same


def same_state(a, b, rows=slice(None)):
    for key in STATE:
        assert np.array_equal(a[key][rows], b[key][rows]), key


def rows_of(dev, table, d):
    """The rows of device d's walls, ascending w: [nb, W_d, 8]"""
    return table[:, np.flatnonzero(np.asarray(dev) == d)]


def median_walls(x, devs, r=R1, k=K1, c=C1, normals=(N_Y, N_X)):
    """Per device of `devs` one wall per normal whose offset is the median of n.x over the EE positions x [B, ndev, 3]: about half the
    robots start inside it."""
    out = []
    for d in devs:
        for n in normals:
            out.append(dict(dev=d, normal=n, offset=float(np.median(x[:, d] @ np.array(n))), radius=r, stiffness=k, damping=c))
    return out


def ee_now(osc, slot):
    """The EE positions [B, ndev, 3] the slot's next tick will see: the trace of one tick on a copy of its coordinates in `slot`, which
    is given its coordinates back."""
    q, qd = osc.download_q(slot)
    x = osc.rollout(1, trace_every=1, slot=slot)["ee_trace"][0][:, :, :3].copy()
    osc.upload_q(q, qd, slot=slot)
    return x


# ---- 1. the force against the oracle, one tick -------------------------------------------------------------------------------------------
_REF1 = {}


def oracle1():
    """oracle/rigid_body.py on the 256 states of test_pushes.states1(): EE positions and jacp of every EE body -> {body: (x [B, 3], jacp
    [B, 3, nj])}.  Computed once."""
    if not _REF1:
        q, _ = tp.states1()
        om = rb.Model()
        ids = {nm: om.body_id(nm) for nm in sorted(set(DUAL_UR5_EE.values()))}
        for nm in ids:
            _REF1[nm] = (np.zeros((len(q), 3)), np.zeros((len(q), 3, om.nj)))
        for b in range(len(q)):
            kin = rb.kinematics(om, q[b])
            for nm, i in ids.items():
                _REF1[nm][0][b] = kin["xpos"][i]
                _REF1[nm][1][b] = rb.body_jacobian(om, kin, i)[0]
    return _REF1


def oracle_force(x, jacp, qvel, rows):
    """The formula of the issue in NumPy on the oracle's x and jacp, per wall: -> g, f [B, W], F [B, 3]"""
    v = np.einsum("bci,bi->bc", jacp, qvel)
    n, off, r, k, c = rows[..., :3], rows[..., 3], rows[..., 4], rows[..., 5], rows[..., 6]
    g = r - (np.einsum("bwc,bc->bw", np.broadcast_to(n, (len(x),) + n.shape[1:]), x) - off)
    s = np.einsum("bwc,bc->bw", np.broadcast_to(n, (len(x),) + n.shape[1:]), v)
    f = k * g - c * s
    on = (g > 0) & (f > 0)
    F = (np.where(on, f, 0.0)[..., None] * n).sum(axis=1)
    return g, f, F


@pytest.mark.parametrize("name", ["k13", "br7"])
def test_one_tick_force_against_the_oracle(name, monkeypatch):
    """The 256 states of test_pushes.states1(); per arm two walls, normals (0, -1, 0) and (1, 0, 0), each with `off` the median of n.x
    over the oracle's EE positions; r = 0.05, k = 900, c = 400.  Oracle: x from oracle/rigid_body.py kinematics, jacp from body_jacobian,
    the formula in NumPy.  Asserted on the oracle first, excluding no robot: per arm and wall at least 64 robots in contact, at least 64
    not, at least 8 clamped (g > 0, f < 0); min |g| > 1e-6 and min |k g - c s| > 1e-3.  Then: equal contact sets, clamped robots have
    force exactly 0, n.F >= 0, and |F - F_oracle| <= 1e-10 (k (max|x| + r + |off|) + c max|jacp| sum|qvel|) per robot -- 1e-10 being
    what test_frontend_records_themselves holds the walk's records to, propagated linearly.  br7: the base is device 0 and the arm
    device 1 -- a device-to-body mix-up reads the wrong body's pose.
    Measured on an MI355X (printed; profiles/wall_rates.md): 143 .. 150 robots in contact and 14 .. 19 clamped per arm and wall, min |g|
    4.8e-4, min |f| 0.24 N; max |F - F_oracle| 5.7e-13 N; worst error / bound 2.57e-6 (k13) and 2.14e-6 (br7) of the 1 allowed."""
    B = tp.B1
    if name == "k13":
        lay, gains, g, model, osc = tr.make_ctx("k13", B, F64, seed=21)
        assert "fused" in osc.from_q_name
    else:
        lay, gains, g, model, osc = trl.open_ctx(name, B, F64, monkeypatch, seed=21)
    qpos, qvel = tp.states1()
    ref = oracle1()
    arms = [d for d, nm in enumerate(lay.dev_names) if nm != "base"]
    xo = np.stack([ref[DUAL_UR5_EE[nm]][0] for nm in lay.dev_names], axis=1)      # [B, ndev, 3]
    ws = median_walls(xo, arms)
    dev, table = wl.normalise(ws, lay.dev_names, B)
    osc.set_plant(DT, 0.0)
    osc.upload_q(qpos, qvel)
    trl.set_targets(osc, g, 0)
    osc.set_walls(ws)
    out = osc.rollout(1)
    st = osc.wall_state()
    osc.close()
    assert not np.any(out["flags_any"] & BAD)
    worst = 0.0
    for d in arms:
        x, jacp = ref[DUAL_UR5_EE[lay.dev_names[d]]]
        rows = rows_of(dev, table, d)
        go, fo, Fo = oracle_force(x, jacp, qvel, rows)
        for w in range(rows.shape[1]):
            on, clamped = (go[:, w] > 0) & (fo[:, w] > 0), (go[:, w] > 0) & (fo[:, w] < 0)
            print(f"[one tick {name}] device {d} wall {w}: {int((go[:, w] > 0).sum())} in contact, {int(clamped.sum())} clamped, "
                  f"min |g| {np.abs(go[:, w]).min():.3g}, min |f| {np.abs(fo[:, w]).min():.3g}")
            assert (go[:, w] > 0).sum() >= 64 and (go[:, w] <= 0).sum() >= 64 and clamped.sum() >= 8
            assert np.abs(go[:, w]).min() > 1e-6 and np.abs(fo[:, w]).min() > 1e-3
            c = 1 if w == 0 else 0                    # wall 0 pushes along y, wall 1 along x: the components tell the walls apart
            n_c = rows[0, w, c]
            assert np.array_equal(st["force"][:, d, c] != 0.0, on)                        # the contact sets, exactly
            assert not st["force"][clamped, d, c].any()
            assert np.all(st["force"][:, d, c] * n_c >= 0.0)                              # never pulling
        assert not st["force"][:, d, 2].any()
        bound = 1e-10 * (K1 * (np.abs(x).max(axis=1) + R1 + np.abs(rows[0, :, 3]).max())
                         + C1 * np.abs(jacp).max(axis=(1, 2)) * np.abs(qvel).sum(axis=1))
        err = np.abs(st["force"][:, d] - Fo).max(axis=1)
        worst = max(worst, float((err / bound).max()))
        print(f"[one tick {name}] device {d}: max |F - F_oracle| {err.max():.3g} N, worst error / bound {(err / bound).max():.3g}, max |F| "
              f"{np.abs(Fo).max():.3g} N")
        assert np.all(err <= bound), (d, float((err / bound).max()), int(np.argmax(err / bound)))
        assert np.array_equal(st["contact_ticks"][:, d], (go > 0).any(axis=1).astype(np.int32))
        assert np.array_equal(st["first_tick"][:, d], np.where((go > 0).any(axis=1), 0, -1))
    for d in range(lay.ndev):
        if d not in arms:                             # a device without walls reports (0, 0, 0, -1)
            assert not st["force"][:, d].any() and not st["max_depth"][:, d].any() and not st["contact_ticks"][:, d].any()
            assert np.all(st["first_tick"][:, d] == -1)
    print(f"[one tick {name}] worst ratio {worst:.3g}")


# ---- 2. walls are pushes with the device's own wrench, bit for bit ----------------------------------------------------------------------
# case: (route of test_rollout_layouts.ROUTES or None, layout, dtype, devices that get walls, ticks)
CASES = {
    "k12_admit": (None, "k12_admit", F64, (1,), 6),
    "br7": ("br7", "br7", F64, (1,), 6),                              # the base is device 0: device index and EE body differ
    "rlbr10": ("rlbr10", "rlbr10", F64, (3,), 6),                     # blocks 0 and 3 of the right arm share one EE body
    "rlbr10_both": ("rlbr10", "rlbr10", F64, (0, 3), 4),              # ... and walls on both: the body's bias is updated twice (4 ticks: 8 pushes)
    "rlb16": ("rlb16", "rlb16", F64, (1,), 6),                        # row16 FROMQ form
    "k13_lane0": ("k13_lane0", "k13", F64, (0,), 6),
    "k12_admit_f32": (None, "k12_admit", F32, (1,), 6),
}


def open_case(case, B, monkeypatch, **kw):
    route, cfg, dtype, devs, T = CASES[case]
    if route is not None:
        ctx = trl.open_ctx(route, B, dtype, monkeypatch, feed=True, **kw)
    else:
        ctx = tr.make_ctx(cfg, B, dtype, feed=True, **kw)
        assert "fused" in ctx[4].from_q_name and "row16" in ctx[4].kernel_name
    return ctx + (devs, T)


def wall_pushes(devs, T, first=0):
    """Push (t, d) has the window (t, t + 1), is applied and sensed: the wrench table gives it [F_d(t), 0, 0, 0]"""
    return [dict(dev=d, window=(first + t, first + t + 1), apply=True, sense=True) for t in range(T) for d in devs]


def push_table(forces, devs):
    """forces[t]: [B, ndev, 3] -> [B, T len(devs), 6] in the order of wall_pushes"""
    B = forces[0].shape[0]
    W = np.zeros((B, len(forces) * len(devs), 6))
    for t, F in enumerate(forces):
        for i, d in enumerate(devs):
            W[:, t * len(devs) + i, :3] = F[:, d]
    return W


@pytest.mark.parametrize("case", list(CASES))
def test_walls_are_pushes_with_the_devices_own_wrench(case, monkeypatch):
    """Slot 0 has walls (k = 900, c = 400, offsets the medians of the start positions: half the robots in contact): T single ticks,
    `force` downloaded after each.  Slot 1 has none, starts from the same states, targets and feed, and gets T pushes per walled device:
    push t has the window (t, t + 1), is applied and sensed, and its per-robot wrench is [F_0(t), 0, 0, 0].  After every tick qpos, qvel,
    u, flags_any and the traced EE poses are equal bit for bit.  This pins the sign, the fma order, the J entries and the one-tick delay
    of SENSE to code test_pushes.py holds to both oracles."""
    B = B0
    lay, gains, g, model, osc, devs, T = open_case(case, B, monkeypatch, seed=5, n_slots=2)
    tp.start(osc, model, g, B, (0, 1))
    ws = median_walls(ee_now(osc, 0), devs)
    osc.set_walls(ws, slot=0)
    a, forces = [], []
    for t in range(T):
        a.append(osc.rollout(1, trace_every=1, slot=0))
        forces.append(osc.wall_state(0)["force"])
    osc.set_pushes(wall_pushes(devs, T), push_table(forces, devs), slot=1)
    touched = np.zeros(B, bool)
    for t in range(T):
        b = osc.rollout(1, trace_every=1, slot=1)
        same(a[t], b, KEYS + ("ee_trace",))
        touched |= forces[t].any(axis=(1, 2))
    osc.clear_pushes(slot=1)
    tp.start(osc, model, g, B, (1,))
    plain = osc.rollout(T, slot=1)
    osc.close()
    assert not np.any(a[-1]["flags_any"] & BAD) and np.all(np.isfinite(a[-1]["qpos"]))
    assert 32 <= touched.sum() < B                                                   # robots in contact, and robots that never were
    assert np.all(np.abs(a[-1]["qvel"][touched] - plain["qvel"][touched]).max(axis=1) > 0.0)       # and the walls acted
    same(a[-1], plain, ("qpos", "qvel"), rows=~touched)


# ---- 3. c = 0 is bit-exact on the host ----------------------------------------------------------------------------------------------------
def c0_walls(x, B, per_robot):
    """Two walls on the left arm (the sum order) and one on the right, no damping; per robot: offsets, radii and stiffnesses differ"""
    ws = median_walls(x, (1,), c=0.0) + median_walls(x, (0,), c=0.0, normals=(N_Y,))
    if per_robot:
        rng = np.random.default_rng(31)
        for w in ws:
            w["offset"] = w["offset"] + rng.normal(0.0, 0.05, B)
            w["radius"] = rng.uniform(0.0, 0.1, B)
            w["stiffness"] = rng.uniform(100.0, 1000.0, B)
    return ws


@pytest.mark.parametrize("per_robot", [False, True])
def test_without_damping_the_force_is_the_host_restatement_bit_for_bit(per_robot):
    """k12_admit, c = 0: after every one of 6 single ticks the downloaded force equals walls.contact_force(traced x, 0, rows) bit for
    bit -- a shared and a per-robot table, two walls on one device (both in contact for some robots: the order of the sum) -- and the
    counters are the restatement's on the traced x."""
    B, T = B0, 6
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5)
    tp.start(osc, model, g, B, (0,))
    ws = c0_walls(ee_now(osc, 0), B, per_robot)
    dev, table = wl.normalise(ws, lay.dev_names, B)
    assert table.shape[0] == (B if per_robot else 1)
    osc.set_walls(ws)
    both = 0
    depth = np.zeros((B, 2))
    ticks, first = np.zeros((B, 2), np.int32), np.full((B, 2), -1, np.int32)
    for t in range(T):
        out = osc.rollout(1, trace_every=1)
        st = osc.wall_state()
        for d in (0, 1):
            x = out["ee_trace"][0][:, d, :3]
            rows = rows_of(dev, table, d)
            assert np.array_equal(st["force"][:, d], wl.contact_force(x, 0.0, rows)), (t, d)
            gd = wl.depth(x, rows)
            hit = (gd > 0).any(axis=1)
            depth[:, d] = np.maximum(depth[:, d], np.where(gd > 0, gd, 0.0).max(axis=1))
            ticks[:, d] += hit
            first[:, d] = np.where(hit & (first[:, d] < 0), t, first[:, d])
            if d == 1:
                both += int((gd > 0).all(axis=1).sum())
        assert np.array_equal(st["max_depth"], depth) and np.array_equal(st["contact_ticks"], ticks) and np.array_equal(st["first_tick"], first)
    osc.close()
    assert both >= 16 and (ticks > 0).any(axis=0).all() and (ticks == 0).any(axis=0).all()
    assert not np.any(out["flags_any"] & BAD)


# ---- 4. untouched means untouched ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k12_admit", "k12_admit_f32", "rlb16"])
def test_walls_nobody_reaches_change_nothing(case, monkeypatch):
    """A wall on every walled device of the case that lies 100 m behind every EE: rollout(8) with a sensor feed is bit-identical to the
    slot without walls -- qpos, qvel, u, flags_any and the trace.  (The SENSE launch runs on ticks 1 .. 7 and subtracts a stored +0.0;
    the APPLY launch stores nothing to the bias.)"""
    B, T = B0, 8
    lay, gains, g, model, osc, devs, _ = open_case(case, B, monkeypatch, seed=5, n_slots=2)
    tp.start(osc, model, g, B, (0, 1))
    osc.set_walls([dict(dev=d, normal=N_Y, offset=-100.0, radius=R1, stiffness=K1, damping=C1) for d in range(lay.ndev)], slot=0)
    a, b = osc.rollout(T, trace_every=1, slot=0), osc.rollout(T, trace_every=1, slot=1)
    st = osc.wall_state(0)
    osc.close()
    same(a, b, KEYS + ("ee_trace",))
    assert not st["force"].any() and not st["max_depth"].any() and not st["contact_ticks"].any() and np.all(st["first_tick"] == -1)


def test_a_robot_out_of_reach_does_not_see_its_wave_mates_walls():
    """A per-robot table: robots 0 .. 63 start 2 cm (plus the radius) inside a wall on the left arm, for robots 64 .. 129 it is 100 m
    away.  Those stay bit-identical to the slot without walls throughout; every one of the others is pushed (no damping here: with
    it a robot that starts moving out of the wall fast enough is clamped to no force, which is test 1's subject)."""
    B, T = B0, 8
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    tp.start(osc, model, g, B, (0, 1))
    x = ee_now(osc, 0)
    off = x[:, 1] @ np.array(N_Y) + 0.02
    off[64:] = -100.0
    osc.set_walls([dict(dev="ur5left", normal=N_Y, offset=off, radius=R1, stiffness=K1, damping=0.0)], slot=0)
    a, b = osc.rollout(T, trace_every=1, slot=0), osc.rollout(T, trace_every=1, slot=1)
    st = osc.wall_state(0)
    osc.close()
    same(a, b, KEYS, rows=slice(64, None))
    assert np.array_equal(a["ee_trace"][:, 64:], b["ee_trace"][:, 64:])
    assert np.all(np.abs(a["qvel"][:64] - b["qvel"][:64]).max(axis=1) > 0.0)
    assert np.all(st["first_tick"][:64, 1] == 0) and np.all(st["first_tick"][64:] == -1) and np.all(st["first_tick"][:, 0] == -1)
    assert not np.any(a["flags_any"] & BAD)


# ---- 5. state continuity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_robot", [False, True])
@pytest.mark.parametrize("case", ["k12_admit", "k12_admit_f32", "rlbr10_both", "k13_lane0"])
def test_T_ticks_equal_T_single_ticks_equal_pieces(case, per_robot, monkeypatch):
    """rollout(8) on slot 0, 8 x rollout(1) on slot 1, rollout(3) + rollout(5) on slot 2, the same walls (k = 900, c = 400) on each:
    qpos, qvel, u, the OR of the flags and the walls' state bit for bit -- the stored force crosses the calls of
    irlosc_rollout_from_q.  The counters against the restatement on the single ticks' traced x."""
    B, T = B0, 8
    lay, gains, g, model, osc, devs, _ = open_case(case, B, monkeypatch, seed=5, n_slots=3)
    tp.start(osc, model, g, B, (0, 1, 2))
    ws = median_walls(ee_now(osc, 0), devs)
    if per_robot:
        rng = np.random.default_rng(32)
        for w in ws:
            w["offset"] = w["offset"] + rng.normal(0.0, 0.05, B)
    dev, table = wl.normalise(ws, lay.dev_names, B)
    for slot in (0, 1, 2):
        osc.set_walls(ws, slot=slot)
    a = osc.rollout(T, slot=0)
    fl = np.zeros(B, np.uint32)
    nd = lay.ndev
    depth, ticks, first = np.zeros((B, nd)), np.zeros((B, nd), np.int32), np.full((B, nd), -1, np.int32)
    for t in range(T):
        b = osc.rollout(1, trace_every=1, slot=1)
        fl |= b["flags_any"]
        for d in sorted(set(devs)):
            gd = wl.depth(b["ee_trace"][0][:, d, :3], rows_of(dev, table, d))
            hit = (gd > 0).any(axis=1)
            depth[:, d] = np.maximum(depth[:, d], np.where(gd > 0, gd, 0.0).max(axis=1))
            ticks[:, d] += hit
            first[:, d] = np.where(hit & (first[:, d] < 0), t, first[:, d])
    c3 = osc.rollout(3, slot=2)
    c = osc.rollout(5, slot=2)
    sa, sb, sc = (osc.wall_state(slot) for slot in (0, 1, 2))
    osc.close()
    assert np.all(np.isfinite(a["qpos"])) and np.all(np.isfinite(a["u"])) and not np.any(a["flags_any"] & BAD)
    same(a, b, ("qpos", "qvel", "u"))
    same(a, c, ("qpos", "qvel", "u"))
    assert np.array_equal(a["flags_any"], fl) and np.array_equal(a["flags_any"], c3["flags_any"] | c["flags_any"])
    same_state(sa, sb)
    same_state(sa, sc)
    assert np.array_equal(sb["max_depth"], depth) and np.array_equal(sb["contact_ticks"], ticks) and np.array_equal(sb["first_tick"], first)
    assert (ticks[:, list(devs)] > 0).any() and (ticks[:, list(devs)] == 0).any() and sa["force"].any()


# ---- 6. coexistence -------------------------------------------------------------------------------------------------------------------------
def test_walls_next_to_waypoint_paths():
    """k13 with paths on both arms and a wall on the left arm: rollout(8) = 8 x rollout(1), waypoint state and wall state included, and
    neither setter ended the other's state."""
    B, T = B0, 8
    sc = tw.scenario(B, False)
    osc = tw.make_ctx(B, n_slots=3)
    for slot in (0, 1, 2):
        tw.fill(osc, sc, slot)
    ws = median_walls(ee_now(osc, 2), (1,), r=0.0)      # (the starts lie within centimetres of each other: no radius, half of them inside)
    for slot in (0, 1):
        osc.set_walls(ws, slot=slot)
        osc.set_waypoints(sc["paths"] + [None], tw.THRESHOLD, True, slot=slot)
    osc.set_waypoints(sc["paths"] + [None], tw.THRESHOLD, True, slot=2)
    a = osc.rollout(T, slot=0)
    fl = np.zeros(B, np.uint32)
    for _ in range(T):
        b = osc.rollout(1, slot=1)
        fl |= b["flags_any"]
    plain = osc.rollout(T, slot=2)
    wa, wb = osc.waypoint_state(0), osc.waypoint_state(1)
    sa, sb = osc.wall_state(0), osc.wall_state(1)
    osc.close()
    same(a, b, ("qpos", "qvel", "u"))
    assert np.array_equal(a["flags_any"], fl) and not np.any(fl & BAD)
    for key in wa:
        assert np.array_equal(wa[key], wb[key]), key
    same_state(sa, sb)
    hit = sa["contact_ticks"][:, 1] > 0
    assert 32 <= hit.sum() < B and np.all(np.abs(a["qvel"][hit] - plain["qvel"][hit]).max(axis=1) > 0.0)
    assert wa["arrivals"][:, :2].min() >= 1      # (waypoint 0 is where the arms start: the cycler ran next to the walls)


def test_walls_next_to_an_action_list():
    """k12_admit with a sensor feed, the WP / GRIP list on the right arm and walls on it: rollout(8) = 8 x rollout(1), bit for bit,
    action state and wall state included -- the order wrench kernel, SENSE, action kernel."""
    B, T = B0, 8
    sc = tal.scenario(B, cfg="k12_admit")
    osc = tal.make_ctx(B, n_slots=3, cfg="k12_admit", feed=True)
    sens = np.random.default_rng(43).normal(0.0, 5.0, size=(B, NS))
    for slot in (0, 1, 2):
        tal.fill(osc, sc, slot)
        osc.set_sensordata(sens, slot=slot)
    dv = sc["desc"]["active_dev"]
    dv = lay_index(osc, dv)
    ws = median_walls(ee_now(osc, 2), (dv,), r=0.0)     # (the starts lie within centimetres of each other: no radius, half of them inside)
    for slot in (0, 1, 2):
        osc.set_action_list(sc["desc"], slot=slot)
        if slot < 2:
            osc.set_walls(ws, slot=slot)
    a = osc.rollout(T, slot=0)
    fl = np.zeros(B, np.uint32)
    for _ in range(T):
        b = osc.rollout(1, slot=1)
        fl |= b["flags_any"]
    plain = osc.rollout(T, slot=2)
    aa, ab = osc.action_state(0), osc.action_state(1)
    sa, sb = osc.wall_state(0), osc.wall_state(1)
    osc.close()
    same(a, b, ("qpos", "qvel", "u"))
    assert np.array_equal(a["flags_any"], fl) and not np.any(fl & BAD)
    for key in aa:
        assert np.array_equal(aa[key], ab[key]), key
    same_state(sa, sb)
    hit = sa["contact_ticks"][:, dv] > 0
    assert 32 <= hit.sum() < B and np.all(np.abs(a["qvel"][hit] - plain["qvel"][hit]).max(axis=1) > 0.0)


def lay_index(osc, dv):
    return osc.layout.dev_names.index(dv) if isinstance(dv, str) else int(dv)


def run_walls_and_pushes(wall_dev, push_dev):
    """Slot 0: walls on wall_dev and two applied-and-sensed pushes on push_dev (windows [1, 4) and [2, 6)); slot 1: those two pushes and
    the six wall pushes of test 2 carrying slot 0's forces.  Six single ticks each -> (slot 0's outputs, slot 1's, slot 0's forces)"""
    B, T = B0, 6
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    tp.start(osc, model, g, B, (0, 1))
    two = [dict(dev=push_dev, window=(1, 4)), dict(dev=push_dev, window=(2, 6))]
    Wp = tp.wrenches(np.random.default_rng(17), B, 2)
    osc.set_walls(median_walls(ee_now(osc, 0), (wall_dev,)), slot=0)
    osc.set_pushes(two, Wp, slot=0)
    a, forces = [], []
    for t in range(T):
        a.append(osc.rollout(1, trace_every=1, slot=0))
        forces.append(osc.wall_state(0)["force"])
    osc.set_pushes(two + wall_pushes((wall_dev,), T), np.concatenate([Wp, push_table(forces, (wall_dev,))], axis=1), slot=1)
    b = [osc.rollout(1, trace_every=1, slot=1) for t in range(T)]
    osc.close()
    assert sum(int(F.any(axis=(1, 2)).sum()) for F in forces[1:]) >= 32 and not np.any(a[-1]["flags_any"] & BAD)
    return a, b, forces


def test_walls_next_to_pushes_run_behind_them():
    """k12_admit, pushes on the right arm (device 0), walls on the left (device 1): walls plus two pushes equal, as in test 2, a slot with
    those two pushes plus the six wall pushes, bit for bit after every tick.  Both arms hang on the stand's hinge, whose bias entry
    both launches update: the push kernel takes the devices in ascending order, so the all-pushes slot updates it for device 0 and then
    for device 1 -- pushes, then walls.  (On ONE device the push kernel sums its pushes' wrenches ahead of a single fma chain, which two
    launches cannot repeat bit for bit; that is no order.)  The other way round -- walls on device 0, pushes on device 1 -- the all-pushes
    slot runs walls, then pushes, and the stand hinge's rounding differs on some robot: the order is visible."""
    a, b, _ = run_walls_and_pushes(wall_dev=1, push_dev=0)
    for t in range(len(a)):
        same(a[t], b[t], KEYS + ("ee_trace",))
    a, b, forces = run_walls_and_pushes(wall_dev=0, push_dev=1)
    same(a[0], b[0], KEYS)                                # (tick 0: no push yet)
    both = forces[1].any(axis=(1, 2))                     # robots whose tick 1 has a wall force and a push
    assert both.sum() >= 16 and not np.array_equal(a[-1]["qvel"][:, 0], b[-1]["qvel"][:, 0])
    assert np.abs(a[-1]["qvel"] - b[-1]["qvel"]).max() < 1e-6      # (rounding, nothing else)


# ---- 7. a NaN robot -------------------------------------------------------------------------------------------------------------------------
def test_a_nan_robot_has_no_contact_and_its_wave_mates_do_not_see_it():
    """Robot 5 has NaN in a left-arm joint of qpos: no contact, zero force, frozen by the plant as without walls (its coordinates stay
    what they were); every other robot is bit-identical to the same run without the NaN."""
    B, T = B0, 4
    lay, gains, g, model, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    qpos, qvel, _ = tp.start(osc, model, g, B, (0, 1))
    ws = median_walls(ee_now(osc, 1), (0, 1))
    bad = qpos.copy()
    bad[5, 15] = np.nan
    osc.upload_q(bad, qvel, slot=0)
    for slot in (0, 1):
        osc.set_walls(ws, slot=slot)
    a, b = osc.rollout(T, slot=0), osc.rollout(T, slot=1)
    sa, sb = osc.wall_state(0), osc.wall_state(1)
    osc.close()
    others = np.arange(B) != 5
    same(a, b, KEYS, rows=others)
    same_state(sa, sb, rows=others)
    assert not sa["force"][5, 1].any() and sa["contact_ticks"][5, 1] == 0 and sa["first_tick"][5, 1] == -1 and sa["max_depth"][5, 1] == 0.0
    assert a["flags_any"][5] & _lib.FLAG_NONFINITE
    assert np.array_equal(a["qpos"][5], bad[5], equal_nan=True) and np.array_equal(a["qvel"][5], qvel[5])      # frozen
    assert sb["contact_ticks"][:, 1].max() > 0


# ---- 8. the state rules ---------------------------------------------------------------------------------------------------------------------
def make_desc(devs=(1, 1), nb=1, W=None):
    d = _lib.Walls()
    d.n_walls, d.nb = len(devs) if W is None else W, nb
    for w in range(len(devs)):
        d.dev[w] = devs[w]
    return d


def rc_set(osc, B, desc, table, slot=0):
    return osc.lib.irlosc_set_walls(osc._h, slot, B, None if desc is None else C.byref(desc), _lib.ptr(table))


def rc_get(osc, B, slot=0):
    return osc.lib.irlosc_download_wall_state(osc._h, slot, B, None, None, None, None)


def state_of(osc, n, slot=0):
    """wall_state of the slot's first n robots (BatchedOSC.wall_state asks for all of them)"""
    nd = osc.layout.ndev
    st = dict(force=np.empty((n, nd, 3)), max_depth=np.empty((n, nd)), contact_ticks=np.empty((n, nd), np.int32), first_tick=np.empty((n, nd), np.int32))
    assert osc.lib.irlosc_download_wall_state(osc._h, slot, n, *(_lib.ptr(st[k]) for k in STATE)) == 0
    return st


def test_state_rules():
    B = B0
    lay = synth.make_layout("k12_admit")
    _, gains, g = synth.make_batch("k12_admit", B, seed=5)
    model = RigidBodyModel.load("dual_ur5")
    good = make_desc()
    bare = BatchedOSC(lay, B, dtype=F64)
    bare.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    T1 = np.ascontiguousarray(np.tile([0.0, -1.0, 0.0, -0.3, R1, K1, C1, 0.0], (1, 2, 1)))
    assert rc_set(bare, B, good, T1) == ERR_STATE                                  # before set_model
    assert "irlosc_set_model" in bare.lib.irlosc_last_error(bare._h).decode()
    assert rc_set(bare, B, None, None) == 0                                        # clearing nothing is no error
    assert rc_get(bare, B) == ERR_STATE
    bare.close()

    _, _, _, _, osc = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    _, _, _, _, twin = tr.make_ctx("k12_admit", B, F64, feed=True, seed=5, n_slots=2)
    qpos, qvel, sens = tp.start(osc, model, g, B, (0, 1))
    tp.start(twin, model, g, B, (0, 1))
    x0 = ee_now(osc, 0)
    _, T1 = wl.normalise(median_walls(x0, (1,)), lay.dev_names, B)                 # [1, 2, 8]: half the robots in contact
    TB = np.ascontiguousarray(np.tile(T1, (B, 1, 1)))
    TB[:, :, 3] += np.random.default_rng(33).normal(0.0, 0.05, (B, 2))

    def reset(o, slots=(0, 1)):
        for slot in slots:
            o.upload_q(qpos, qvel, slot=slot)

    def both(n=1, slot=0):
        same(osc.rollout(n, slot=slot), twin.rollout(n, slot=slot))
        same_state(osc.wall_state(slot), twin.wall_state(slot))

    # every refused call leaves the walls in force, whole, their tick and state included: the twin never sees one
    assert rc_set(osc, B, good, T1) == 0 and rc_set(twin, B, good, T1) == 0
    both()

    def broken(i, j, v, per_robot=False):
        t = (TB if per_robot else T1).copy()
        t[-1 if per_robot else 0, i, j] = v
        return t

    refused = [
        (B, make_desc(devs=(), W=0), T1), (B, make_desc(W=9), T1),                                      # W outside [1, 8]
        (B, make_desc(devs=(1, 2)), T1), (B, make_desc(devs=(-1, 1)), T1),                              # dev outside [0, ndev)
        (B, make_desc(nb=2), T1), (B, make_desc(nb=B - 1), TB), (0, good, T1),                          # nb not 1 or B; B < 1
        (B, good, None), (B, good, broken(1, 3, np.nan)), (B, make_desc(nb=B), broken(0, 5, np.inf, True)),      # NULL or not finite
        (B, good, broken(0, 7, np.nan)),                                                                # (the eighth word too)
        (B, good, broken(0, 1, -1.0 - 1e-11)), (B, make_desc(nb=B), broken(1, 0, 1e-5, True)), (B, good, broken(0, 0, 1.0)),      # |n|
        (B, good, broken(0, 4, -1e-9)), (B, good, broken(1, 5, -1.0)), (B, make_desc(nb=B), broken(0, 6, -0.5, True)),            # r, k, c < 0
    ]
    for i, (b_, desc, t) in enumerate(refused):
        assert rc_set(osc, b_, desc, t) == ERR_ARG, i
        assert "walls" in osc.lib.irlosc_last_error(osc._h).decode(), i
        both()
    plain = twin.rollout(len(refused) + 1, slot=1)
    assert np.abs(osc.download_q()[1] - plain["qvel"]).max() > 0.0                 # (and they were in force)
    assert rc_set(osc, B + 1, good, T1) == ERR_ARG                                 # (check_slot)

    # a rollout narrower than the walls runs; one over more robots than they cover is refused, and so is such a download
    reset(osc)
    reset(twin)
    assert rc_set(osc, 64, make_desc(nb=64), TB[:64].copy()) == 0
    assert tr._rc_rollout(osc, B) == ERR_STATE and "walls" in osc.lib.irlosc_last_error(osc._h).decode()
    assert rc_get(osc, B) == ERR_STATE and "walls" in osc.lib.irlosc_last_error(osc._h).decode()
    assert rc_get(osc, 64) == 0 and rc_get(osc, 10) == 0
    assert rc_get(osc, 64, slot=1) == ERR_STATE                                    # a slot without walls
    assert rc_set(twin, B, make_desc(nb=B), TB) == 0
    assert tr._rc_rollout(osc, 64, ticks=2) == 0 and tr._rc_rollout(osc, 10, ticks=2) == 0      # robots 10 .. 63 ran two ticks, the first ten four
    sa = state_of(osc, 64)
    twin.rollout(2)
    same_state(sa, twin.wall_state(), rows=slice(10, 64))      # (their state is that of the last tick that ran them)
    twin.rollout(2)
    same_state(sa, twin.wall_state(), rows=slice(0, 10))

    # desc == NULL and set_model end them
    T = 6
    reset(twin)
    twin.clear_walls()
    plain = twin.rollout(T, slot=1)
    reset(osc)
    assert rc_set(osc, B, good, T1) == 0
    osc.clear_walls()
    assert rc_get(osc, B) == ERR_STATE
    same(osc.rollout(T), plain)
    assert rc_set(osc, B, good, T1) == 0
    osc.set_model(model)
    osc.set_ft_sensors()
    assert rc_get(osc, B) == ERR_STATE
    tp.start(osc, model, g, B, (0, 1))
    same(osc.rollout(T), plain)

    # set_targets, set_gains, upload_q, set_sensordata, set_pushes / clear_pushes and step_q leave them, their state and their tick alone
    reset(osc)
    reset(twin)
    for o in (osc, twin):
        assert rc_set(o, B, good, T1) == 0
    both(2)
    trl.set_targets(osc, g, 0)
    osc.set_gains(gains["kp"], gains["kv"], gains["ko"], gains["k"], gains["d"], gains["max_vel"], gains["null_kv"])
    osc.upload_q(*osc.download_q())
    osc.set_sensordata(sens)
    osc.set_pushes([dict(dev=0, window=(0, 5))], np.ones((1, 6)))
    osc.clear_pushes()
    osc.step_q()
    both(2)
    osc.step_q()
    both(4)
    reset(twin, (1,))
    assert np.abs(twin.rollout(8, slot=1)["qvel"] - osc.download_q()[1]).max() > 0.0

    # set_waypoints leaves them and their tick alone, and clearing the paths too
    reset(osc)
    reset(twin)
    for o in (osc, twin):
        assert rc_set(o, B, good, T1) == 0
    both(2)
    paths = [np.array([[0.3, 0.45, 0.5], [0.32, 0.45, 0.5]]), None]
    osc.set_waypoints(paths, 0.01)
    twin.set_waypoints(paths, 0.01)
    both(3)
    for o in (osc, twin):
        trl.set_targets(o, g, 0)                                                     # (the paths end, the targets are the start's again)
    both(2)
    assert osc.wall_state()["contact_ticks"].max() > 2                               # (counted across the setters)

    # two slots with different walls, interleaved
    reset(osc)
    reset(twin)
    other = make_desc(devs=(0,), nb=B)
    TO = np.ascontiguousarray(np.tile([1.0, 0.0, 0.0, 0.0, R1, K1, 0.0, 0.0], (B, 1, 1)))
    TO[:, 0, 3] = x0[:, 0, 0] + np.random.default_rng(34).normal(0.0, 0.05, B)
    for o in (osc, twin):
        assert rc_set(o, B, good, T1, slot=0) == 0 and rc_set(o, B, other, TO, slot=1) == 0
    for _ in range(T):
        a0 = osc.rollout(1, slot=0)
        a1 = osc.rollout(1, slot=1)
    same(a0, twin.rollout(T, slot=0), ("qpos", "qvel", "u"))
    same(a1, twin.rollout(T, slot=1), ("qpos", "qvel", "u"))
    for slot in (0, 1):
        same_state(osc.wall_state(slot), twin.wall_state(slot))
    assert np.abs(a0["qvel"] - a1["qvel"]).max() > 0.0
    assert osc.wall_state(0)["contact_ticks"][:, 1].any() and osc.wall_state(1)["contact_ticks"][:, 0].any()
    osc.close()
    twin.close()


# ---- 9. the example -------------------------------------------------------------------------------------------------------------------------
def test_the_example_touches_the_wall_and_the_wall_holds_the_arm_back():
    """examples/force_test_resident_headless.py, 64 robots, 600 ticks, EE radius 0.25 m: some robot touches the wall; the force never
    pulls (the wall's normal is (0, -1, 0): force_y <= 0, nothing along x and z); on the robots in contact the left EE's deepest
    penetration is smaller than on a second slot run without the wall.  How far this plant yields and whether it settles is not
    asserted.  The radius: with the osc1 gains and the 1 cm threshold the arm needs 1 920 ticks to the first touch at the example's
    default 0.1 m (profiles/wall_rates.md); at 0.25 m the wall's reach begins between the second and third waypoint and 20 of the 64
    robots are in it from tick 426 on."""
    mod = tr._example("force_test_resident_headless")
    t0 = time.perf_counter()
    r = mod.run(robots=64, ticks=600, log_every=20, radius=0.25, seed=0, verbose=False)
    print(f"[example] {time.perf_counter() - t0:.2f} s; robots in contact {int((r['contact_ticks'] > 0).sum())}/64, max depth with the wall "
          f"{r['max_depth'].max():.4f} m, without {r['free_depth'].max():.4f} m, max |force_y| {np.abs(r['force_log'][:, :, 1]).max():.1f} N")
    assert np.all(np.isfinite(r["q"])) and not np.any(r["flags_any"] & BAD)
    hit = r["contact_ticks"] > 0
    assert hit.any()
    F = r["force_log"]                                   # [chunks, robots, 3]
    assert np.all(F[:, :, 1] <= 0.0) and not F[:, :, 0].any() and not F[:, :, 2].any()
    assert np.all(r["max_depth"][hit] < r["free_depth"][hit])
    assert r["csv_rows"][0] == ["x", "force_x", "force_y", "force_z"] and len(r["csv_rows"]) == 1 + F.shape[0]
