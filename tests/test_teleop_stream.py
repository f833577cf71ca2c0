"""The space-mouse teleoperation stream on the GPU (-m gpu): irlosc_set_teleop_stream / irlosc_download_teleop_state /
irlosc_download_targets -- the stream kernel (csrc/osc_teleop.hpp) in front of the OSC step of a rollout tick, against its NumPy mirror
(teleop.stream_step) tick by tick, against a slot that is handed the same targets by the host, against itself in pieces, shared against
per-robot streams, at its end and across its loop, over a wrap of the yaw, next to a robot that holds a NaN, and the state rules.

Shapes: B = 70 (one full wave and a ragged one of 6 robots) and B = 1; T = 48 readings of space_mouse_stream (seed 5; a robot of its own:
seed 5 + b); float64 and float32 contexts; k13 (three devices: both arms RIGID, the base HEADING) and r6 (one device, tile row 7).

THE BOUND of device against mirror: positions are sums and products rounded alike on both sides -- bit-equal.  Angles, and the target
words derived from them, go through sin / cos / atan2, which HIP states to be within 2 ulp on the device; perturbing every such call of
the mirror by +-2 ulp accumulated to <= 1.1e-14 over 200 ticks, so 1e-12 leaves two orders of magnitude.  A float32 context stores
casts of the same float64 values: within one float32 ulp of the mirror's cast.  The wrap atan2(sin a, cos a) is discontinuous at +-pi:
the tests assert ON THE MIRROR that every angle stays >= 1e-6 from +-pi, so that both sides decide every wrap alike."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

for _p in (ROOT, os.path.join(ROOT, "examples")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from irl_control_amd import BatchedOSC, _lib, synth, teleop      # noqa: E402
from irl_control_amd.rigid_body import RigidBodyModel            # noqa: E402
import teleop_loops as tl                                        # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
F64, F32 = np.float64, np.float32
RIGHT, LEFT = slice(1, 7), slice(13, 19)            # arm joints of the Dual-UR5
Q_RIGHT = np.array([0.3, -0.3, 1.5, 0.3, 1.1, 0.3])
Q_LEFT = np.array([-0.2, -0.8, 1.0, -0.2, 0.6, -0.2])
DT, DAMPING = 1e-3, 0.0
T, SEED = 48, 5
BOUND = 1e-12                                       # float64: angles (mod 2 pi) and target words, device against mirror (above)
WRAP_MARGIN = 1e-6
ORIGIN = np.array(teleop.ORIGIN)


def make_ctx(B, dtype=F64, cfg="k13", n_slots=1, max_batch=None, bare=False):
    """A context for B robots with the layout's base gains, the model and the plant (bare: none of the three)."""
    osc = BatchedOSC(synth.make_layout(cfg), B if max_batch is None else max_batch, dtype=dtype, n_slots=n_slots)
    if not bare:
        g = synth.make_batch(cfg, 1, seed=0)[1]
        osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], g["max_vel"], g["null_kv"])
        osc.set_model(RigidBodyModel.load("dual_ur5"))
        osc.set_plant(DT, DAMPING)
    return osc


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def start_state(B):
    """(q, qd) [B, 25]: both arms at their start configurations + uniform(-0.15, 0.15) rad per joint, at rest.  Never written to."""
    def make():
        rng = np.random.default_rng(4000 + B)
        q = np.zeros((B, 25))
        q[:, RIGHT] = Q_RIGHT + rng.uniform(-0.15, 0.15, (B, 6))
        q[:, LEFT] = Q_LEFT + rng.uniform(-0.15, 0.15, (B, 6))
        qd = np.zeros((B, 25))
        q.setflags(write=False)
        qd.setflags(write=False)
        return q, qd
    return cached(("start", B), make)


def start_targets(B, ndev):
    """Targets [B, ndev, 7] that no tick of a stream produces: every word tells robot and device (what a tick leaves alone shows)."""
    t = np.zeros((B, ndev, 7))
    t[:, :, 0] = 0.125 * (1 + np.arange(ndev))[None, :]
    t[:, :, 1] = 0.25
    t[:, :, 2] = 0.5 + np.arange(B)[:, None] / 1024.0
    t[:, :, 3] = 1.0
    return t


def readings_of(seed, ticks=T):
    return cached(("readings", seed, ticks), lambda: teleop.record_readings(tl.space_mouse_stream(seed, ticks), ticks))


def fleet_readings(B, ticks=T):
    """[B, ticks, 6]: robot b replays the session of seed 5 + b."""
    return np.array([readings_of(SEED + b, ticks) for b in range(B)])


def mirror(origin, readings, rig, tgt0, B):
    """teleop.stream_run per robot -> (poses [T, B, 6], targets [T, B, ndev, 7]); asserts the wrap margin on every angle."""
    origin = np.broadcast_to(np.asarray(origin, dtype=F64), (B, 6))
    readings = np.asarray(readings, dtype=F64)
    readings = np.broadcast_to(readings if readings.ndim == 3 else readings[None], (B,) + readings.shape[-2:])
    runs = [teleop.stream_run(origin[b], readings[b], rig, targets=tgt0[b]) for b in range(B)]
    poses, tgts = np.array([r[0] for r in runs]).transpose(1, 0, 2), np.array([r[1] for r in runs]).transpose(1, 0, 2, 3)
    margin = (np.pi - np.abs(poses[:, :, 3:])).min()
    assert margin >= WRAP_MARGIN, f"the mirror comes within {margin:.3g} rad of +-pi: device and mirror could decide a wrap differently"
    return poses, tgts


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def angle_diff(a, b):
    d = np.asarray(a) - np.asarray(b)
    return np.abs(np.arctan2(np.sin(d), np.cos(d)))


def fill(osc, B, slot=0, tgt=None, tgt_vel=None, sens=None):
    """The start state and the start targets (or `tgt`) of the slot; tgt_vel, sens: its target velocities and its sensor feed's reading."""
    q, qd = start_state(B)
    osc.upload_q(q, qd, slot=slot)
    osc.set_targets(start_targets(B, osc.layout.ndev) if tgt is None else tgt, tgt_vel, slot=slot)
    if sens is not None:
        osc.set_sensordata(sens, slot=slot)


def tick_by_tick(osc, ticks, slot=0):
    """ticks x rollout(1) with state and targets downloaded behind each -> dict of per-tick arrays."""
    out = dict(q=[], qd=[], u=[], flags=[], pose=[], tick=[], tgt=[])
    for _ in range(ticks):
        r = osc.rollout(1, slot=slot)
        st = osc.teleop_state(slot)
        out["q"].append(r["qpos"]); out["qd"].append(r["qvel"]); out["u"].append(r["u"]); out["flags"].append(r["flags_any"])
        out["pose"].append(st["pose"]); out["tick"].append(st["tick"]); out["tgt"].append(osc.download_targets(slot))
    return {k: np.array(v) for k, v in out.items()}


def stepped(cfg, B, dtype, rig=None, name=None, open_ctx=None, **filled):
    """The run the first tests share: per-robot streams (B > 1) of T readings, T x rollout(1), with its mirror.  rig: the followers
    (default: the demo's for the layout); open_ctx: what opens the context (default: make_ctx on cfg), under the cache name `name`;
    filled: what fill() gets beyond the start state and targets."""
    def make():
        osc = make_ctx(B, dtype, cfg=cfg) if open_ctx is None else open_ctx()
        fill(osc, B, **filled)
        rd = fleet_readings(B) if B > 1 else readings_of(SEED)
        followers = teleop.space_mouse_rig(synth.make_layout(cfg)) if rig is None else rig
        osc.set_teleop_stream(rd, ORIGIN, rig=followers)
        first = osc.teleop_state()
        dev = tick_by_tick(osc, T)
        osc.close()
        poses, tgts = mirror(ORIGIN, rd, followers, start_targets(B, len(followers)), B)
        return dict(dev=dev, poses=poses, tgts=tgts, first=first, readings=rd, rig=followers)
    return cached(("stepped", cfg if name is None else name, B, np.dtype(dtype).name), make)


def assert_follows_the_mirror(run, B, dtype, label, ticks=T):
    """The assertions of test 1 on a run of stepped()'s form -> (max angle diff, max target word diff: float64 absolute, float32 in ulp)."""
    dev, poses, tgts = run["dev"], run["poses"], run["tgts"]
    assert run["first"]["tick"] == 0 and same_bits(run["first"]["pose"], np.tile(ORIGIN, (B, 1)))
    assert list(dev["tick"]) == list(range(1, ticks + 1))
    assert same_bits(dev["pose"][:, :, :3], poses[:, :, :3])
    da = angle_diff(dev["pose"][:, :, 3:], poses[:, :, 3:]).max()
    assert np.abs(dev["pose"][:, :, 3:]).max() <= np.pi
    assert dev["tgt"].dtype == dtype
    if dtype == F64:
        dt = np.abs(dev["tgt"] - tgts).max()
        print(f"{label} B={B} float64: device vs mirror over {ticks} ticks: max angle diff {da:.3g}, max target word diff {dt:.3g}")
        assert dt <= BOUND, dt
    else:
        want = tgts.astype(F32)
        dt = (np.abs(dev["tgt"].astype(F64) - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)).max()
        print(f"{label} B={B} float32: device vs mirror over {ticks} ticks: max angle diff {da:.3g}, max target word diff {dt:.3g} float32 ulp")
        assert dt <= 1.0, dt
    assert da <= BOUND, da
    return da, dt


# ---- 1. device against the mirror, tick by tick -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype", [("k13", 70, F64), ("k13", 70, F32), ("k13", 1, F64), ("k13", 1, F32), ("r6", 70, F64), ("r6", 70, F32)])
def test_device_follows_the_mirror_tick_by_tick(cfg, B, dtype):
    """x, y, z bit-equal; angles (mod 2 pi) and float64 target words within 1e-12; float32 target words within one float32 ulp of the
    mirror's cast; the setter wrote no target and left pose = origin, tick = 0.
    Observed on an MI355X over the 48 ticks: angles within 2.22e-15 (B = 70, k13 and r6, both dtypes) and 1.78e-15 (B = 1); float64
    target words within 1.22e-15 (B = 70) and 1.08e-15 (B = 1); float32 target words equal to the mirror's cast (0 ulp)."""
    assert_follows_the_mirror(stepped(cfg, B, dtype), B, dtype, cfg)


# ---- 2. the same tick, nothing else changed ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_slot_fed_the_streams_targets_by_the_host_steps_bit_for_bit_alike(dtype):
    """Slot 0 runs the stream; slot 1 has no program and gets slot 0's targets of tick t by set_targets before its tick t: the stream
    kernel's targets are in place for the OSC step of its own tick, and nothing else of the tick changed."""
    B = 70
    osc = make_ctx(B, dtype, n_slots=2)
    fill(osc, B, slot=0)
    fill(osc, B, slot=1)
    osc.set_teleop_stream(fleet_readings(B), ORIGIN, slot=0)
    for t in range(T):
        a = osc.rollout(1, slot=0)
        osc.set_targets(osc.download_targets(0), slot=1)
        b = osc.rollout(1, slot=1)
        for k in ("qpos", "qvel", "u", "flags_any"):
            assert same_bits(a[k], b[k]), (t, k)
    assert osc.teleop_state(0)["tick"] == T
    osc.close()


# ---- 3. one rollout(T) = T x rollout(1) = 2 x rollout(T / 2) ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype", [("k13", 70, F64), ("k13", 70, F32), ("r6", 70, F64), ("k13", 1, F64)])
def test_pieces_of_a_rollout_add_up(cfg, B, dtype):
    run = stepped(cfg, B, dtype)
    for pieces in ((T,), (T // 2, T // 2)):
        osc = make_ctx(B, dtype, cfg=cfg)
        fill(osc, B)
        osc.set_teleop_stream(run["readings"], ORIGIN)
        for p in pieces:
            out = osc.rollout(p)
        st, tg = osc.teleop_state(), osc.download_targets()
        osc.close()
        assert st["tick"] == T
        assert same_bits(out["qpos"], run["dev"]["q"][-1]) and same_bits(out["qvel"], run["dev"]["qd"][-1]), pieces
        assert same_bits(st["pose"], run["dev"]["pose"][-1]) and same_bits(tg, run["dev"]["tgt"][-1]), pieces


# ---- 4. shared and per-robot streams and origins; narrower rollouts --------------------------------------------------------------------
def test_a_shared_stream_equals_its_row_repeated_and_origins_per_robot_give_poses_per_robot():
    B, n = 70, 64
    rd = readings_of(SEED)
    rng = np.random.default_rng(7)
    origins = ORIGIN + np.concatenate([rng.uniform(-0.1, 0.1, (B, 3)), rng.uniform(-0.3, 0.3, (B, 3))], axis=1)
    res = []
    for readings, origin in ((rd, ORIGIN), (np.tile(rd, (B, 1, 1)), np.tile(ORIGIN, (B, 1))), (rd, origins)):
        osc = make_ctx(B)
        fill(osc, B)
        osc.set_teleop_stream(readings, origin)
        out = osc.rollout(T)
        res.append((out, osc.teleop_state(), osc.download_targets()))
        osc.close()
    (oa, sa, ta), (ob, sb, tb), (oc, sc, tc) = res
    assert same_bits(oa["qpos"], ob["qpos"]) and same_bits(sa["pose"], sb["pose"]) and same_bits(ta, tb)
    rig = teleop.space_mouse_rig(synth.make_layout("k13"))
    poses, tgts = mirror(origins, rd, rig, start_targets(B, 3), B)
    assert len({tuple(p) for p in sc["pose"].round(9)}) == B
    assert same_bits(sc["pose"][:, :3], poses[-1][:, :3]) and angle_diff(sc["pose"][:, 3:], poses[-1][:, 3:]).max() <= BOUND
    assert np.abs(tc - tgts[-1]).max() <= BOUND
    # robots >= n of a narrower rollout keep pose and targets, and miss those readings: the reading index is the slot's tick
    osc = make_ctx(B)
    fill(osc, B)
    osc.set_teleop_stream(rd, origins)
    assert osc.lib.irlosc_rollout_from_q(osc._h, 0, n, 5, 0, None, None, None) == 0
    st, tg = osc.teleop_state(), osc.download_targets()
    assert st["tick"] == 5
    assert same_bits(st["pose"][n:], origins[n:]) and same_bits(tg[n:], start_targets(B, 3)[n:])
    assert same_bits(st["pose"][:n, :3], poses[4][:n, :3]) and np.abs(tg[:n] - tgts[4][:n]).max() <= BOUND
    osc.upload_q(*start_state(B))
    osc.rollout(1)                                       # tick 5 over all B robots: reading 5 for every robot
    st, tg = osc.teleop_state(), osc.download_targets()
    late = [teleop.stream_step(origins[b], rd[5], rig) for b in range(n, B)]
    assert same_bits(st["pose"][n:, :3], np.array([p[:3] for p, _ in late]))
    assert angle_diff(st["pose"][n:, 3:], np.array([p[3:] for p, _ in late])).max() <= BOUND
    assert np.abs(tg[n:, :2] - np.array([t[:2] for _, t in late])).max() <= BOUND
    assert same_bits(st["pose"][:n, :3], poses[5][:n, :3])
    osc.close()


# ---- 5. end and loop -------------------------------------------------------------------------------------------------------------------
def assert_ends_or_loops(osc, B, rig, refill):
    """The body of test 5 on an open context whose slot 0 `refill` puts back to the start: no launch after the last reading while the
    tick counts on; a looped stream reads reading 0 again; a stream of one reading, looped and played once."""
    rd = readings_of(SEED)
    ndev = len(rig)
    two, tgts2 = mirror(ORIGIN, np.concatenate([rd, rd[:3]]), rig, start_targets(B, ndev), B)      # the looped stream, three ticks into its second pass
    refill()
    osc.set_teleop_stream(rd, ORIGIN, rig=rig, loop=False)
    osc.rollout(T)
    end_pose, end_tgt = osc.teleop_state()["pose"], osc.download_targets()
    for extra in range(1, 7):                            # ticks T .. T + 5: no launch, nothing moves, the tick counts
        osc.rollout(1)
        st = osc.teleop_state()
        assert st["tick"] == T + extra and same_bits(st["pose"], end_pose) and same_bits(osc.download_targets(), end_tgt)
    assert same_bits(end_pose[:, :3], two[T - 1][:, :3])
    refill()
    osc.set_teleop_stream(rd, ORIGIN, rig=rig, loop=True)
    osc.rollout(T + 3)                                   # tick T reads reading 0 again
    st, tg = osc.teleop_state(), osc.download_targets()
    assert st["tick"] == T + 3
    assert same_bits(st["pose"][:, :3], two[T + 2][:, :3]) and angle_diff(st["pose"][:, 3:], two[T + 2][:, 3:]).max() <= BOUND
    assert np.abs(tg - tgts2[T + 2]).max() <= BOUND
    # T = 1: one reading, looped three times and played once
    one, tg1 = mirror(ORIGIN, np.tile(rd[:1], (3, 1)), rig, start_targets(B, ndev), B)
    refill()
    osc.set_teleop_stream(rd[:1], ORIGIN, rig=rig, loop=True)
    osc.rollout(3)
    st = osc.teleop_state()
    assert st["tick"] == 3 and same_bits(st["pose"][:, :3], one[2][:, :3]) and np.abs(osc.download_targets() - tg1[2]).max() <= BOUND
    refill()
    osc.set_teleop_stream(rd[:1], ORIGIN, rig=rig, loop=False)
    osc.rollout(3)
    st = osc.teleop_state()
    assert st["tick"] == 3 and same_bits(st["pose"][:, :3], one[0][:, :3]) and np.abs(osc.download_targets() - tg1[0]).max() <= BOUND


@pytest.mark.parametrize("B", [70, 1])
def test_a_stream_ends_or_loops_after_its_last_reading(B):
    osc = make_ctx(B)
    assert_ends_or_loops(osc, B, teleop.space_mouse_rig(synth.make_layout("k13")), lambda: fill(osc, B))
    osc.close()


# ---- 6. a wrap that is decided -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_yaw_that_passes_pi_wraps_on_both_sides(dtype):
    """Origin yaw 3.0; constant readings step it by +0.3 rad per tick (yaw counts DOWN with its reading: -200 x 0.0015) for 3 ticks:
    3.3 - 2 pi, then on.  Device and mirror agree within 1e-12 and land in (-pi, pi]."""
    B = 70
    origin = np.array([0.0, 0.5, 0.5, 0.0, 0.0, 3.0])
    rd = np.tile([0.0, 0.0, 0.0, 0.0, 0.0, -200.0], (3, 1))
    rig = teleop.space_mouse_rig(synth.make_layout("k13"))
    poses, tgts = mirror(origin, rd, rig, start_targets(B, 3), B)
    assert poses[0, 0, 5] < 0 and np.all(np.abs(poses[:, :, 5]) < np.pi) and abs(poses[2, 0, 5] - (3.9 - 2 * np.pi)) < 1e-12
    osc = make_ctx(B, dtype)
    fill(osc, B)
    osc.set_teleop_stream(rd, origin)
    dev = tick_by_tick(osc, 3)
    osc.close()
    assert np.all(dev["pose"][:, :, 5] > -np.pi) and np.all(dev["pose"][:, :, 5] <= np.pi)
    assert np.abs(dev["pose"] - poses).max() <= BOUND        # (not mod 2 pi: the wrap itself is what is compared)
    if dtype == F64:
        assert np.abs(dev["tgt"] - tgts).max() <= BOUND
    else:
        want = tgts.astype(F32)
        assert (np.abs(dev["tgt"].astype(F64) - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)).max() <= 1.0


# ---- 7. state rules ------------------------------------------------------------------------------------------------------------------------
def c_desc(rig, ticks=T, nb=1, nb_origin=1, loop=0, increment=0.0015, **over):
    d = teleop.to_struct(rig, ticks, nb, nb_origin, increment, False)
    d.loop = loop
    for key, (k, i, v) in over.items():
        if i is None:
            getattr(d, key)[k] = v
        else:
            getattr(d, key)[k][i] = v
    return d


def test_state_rules():
    B = 70
    lay = synth.make_layout("k13")
    rig = teleop.space_mouse_rig(lay)
    rd = np.ascontiguousarray(readings_of(SEED))
    og = np.ascontiguousarray(ORIGIN[None])
    q, qd = start_state(B)
    tgt0 = start_targets(B, 3)
    poses, tgts = mirror(ORIGIN, rd, rig, tgt0, B)
    osc = make_ctx(B, bare=True)
    lib, h = osc.lib, osc._h
    g = synth.make_batch("k13", 1, seed=0)[1]

    def set_ts(d=None, r=rd, o=og, n=B, slot=0, **kw):
        return lib.irlosc_set_teleop_stream(h, slot, n, C.byref(c_desc(rig, **kw) if d is None else d), _lib.ptr(r), _lib.ptr(o))

    def state_rc(n=B):
        return lib.irlosc_download_teleop_state(h, 0, n, None, None)

    def follows_mirror(t):
        """The state is the mirror's after tick t (0-based)."""
        st, tg = osc.teleop_state(), osc.download_targets()
        return (st["tick"] == t + 1 and same_bits(st["pose"][:, :3], poses[t][:, :3]) and angle_diff(st["pose"][:, 3:], poses[t][:, 3:]).max() <= BOUND
                and np.abs(tg - tgts[t]).max() <= BOUND)

    # IRLOSC_ERR_STATE: before the model, before the targets, targets for fewer robots; downloads without a stream / targets
    assert set_ts() == ERR_STATE and "irlosc_set_model" in lib.irlosc_last_error(h).decode()
    osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], g["max_vel"], g["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(DT, DAMPING)
    osc.upload_q(q, qd)
    assert set_ts() == ERR_STATE and "irlosc_set_targets" in lib.irlosc_last_error(h).decode()
    buf = np.empty((B, 3, 7))
    assert lib.irlosc_download_targets(h, 0, B, _lib.ptr(buf)) == ERR_STATE
    assert lib.irlosc_set_targets(h, 0, B - 1, _lib.ptr(np.ascontiguousarray(tgt0[:B - 1])), None) == 0
    assert set_ts() == ERR_STATE and state_rc() == ERR_STATE
    assert lib.irlosc_download_targets(h, 0, B, _lib.ptr(buf)) == ERR_STATE and lib.irlosc_download_targets(h, 0, B - 1, _lib.ptr(buf)) == 0
    assert same_bits(buf[:B - 1], tgt0[:B - 1])          # (works without a program)
    assert lib.irlosc_download_targets(h, 0, B - 1, None) == ERR_ARG
    osc.set_targets(tgt0)
    assert set_ts() == 0 and state_rc() == 0
    assert same_bits(osc.download_targets(), tgt0)       # the setter writes no target
    osc.rollout(4)
    assert follows_mirror(3)
    # IRLOSC_ERR_ARG, and the stream in force stays whole
    nan_rd, nan_og = rd.copy(), og.copy()
    nan_rd[T - 1, 4] = np.nan
    nan_og[0, 2] = np.inf
    bad = [dict(ticks=0), dict(ticks=_lib.MAX_STREAM_TICKS + 1), dict(kind=(1, None, 3)), dict(kind=(3, None, teleop.RIGID)), dict(nb=2), dict(nb=0),
           dict(nb_origin=2), dict(nb_origin=0), dict(loop=2), dict(loop=-1), dict(increment=np.nan), dict(increment=np.inf),
           dict(off_xyz=(0, 1, np.nan)), dict(off_quat=(1, 2, np.nan)), dict(off_quat=(0, 0, 1.0 + 1e-9)), dict(off_quat=(1, 3, 0.5)),
           dict(heading_offset=(2, None, np.inf))]
    for over in bad:
        assert set_ts(**over) == ERR_ARG, (over, lib.irlosc_last_error(h).decode())
    none = [teleop.follower()] * 3
    assert lib.irlosc_set_teleop_stream(h, 0, B, C.byref(teleop.to_struct(none, T, 1, 1)), _lib.ptr(rd), _lib.ptr(og)) == ERR_ARG      # all NONE
    assert set_ts(r=nan_rd) == ERR_ARG and set_ts(o=nan_og) == ERR_ARG and set_ts(r=None) == ERR_ARG and set_ts(o=None) == ERR_ARG
    assert set_ts(n=0) == ERR_ARG and set_ts(slot=5) == ERR_ARG and set_ts(n=B + 1) == ERR_ARG
    # (values of a device that does not read them are not judged: a HEADING's offsets, a RIGID's heading_offset)
    osc.rollout(1)
    assert follows_mirror(4)
    # a rollout over more robots than the stream covers is refused
    assert set_ts(n=B - 6) == 0
    assert lib.irlosc_rollout_from_q(h, 0, B, 1, 0, None, None, None) == ERR_STATE and "teleoperation stream" in lib.irlosc_last_error(h).decode()
    assert state_rc() == ERR_STATE and state_rc(B - 6) == 0
    # set_gains leaves it; a NULL description and set_targets end it; it leaves the targets as they are
    osc.upload_q(q, qd)
    assert set_ts() == 0
    osc.rollout(2)
    osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], np.array(g["max_vel"]) * 2.0, g["null_kv"])
    osc.rollout(1)
    assert follows_mirror(2)
    held = osc.download_targets()
    assert lib.irlosc_set_teleop_stream(h, 0, B, None, None, None) == 0 and state_rc() == ERR_STATE
    assert same_bits(osc.download_targets(), held)
    assert set_ts() == 0 and state_rc() == 0
    osc.set_targets(tgt0)
    assert state_rc() == ERR_STATE
    # paths and a list replace a stream, a stream replaces them; their NULL descriptions leave it alone
    wp_rc = lambda: lib.irlosc_download_waypoint_state(h, 0, B, None, None, None)                      # noqa: E731
    al_rc = lambda: lib.irlosc_download_action_state(h, 0, B, None, None, None, None, None, None)      # noqa: E731
    path = [np.array([[0.1, 0.4, 0.5], [0.2, 0.4, 0.5]]), None, None]
    grips = dict(n_actions=1, active_dev=0, passive_dev=1, passive_hold_orientation=1, passive_quat=[1.0, 0, 0, 0], pose=np.zeros((1, 1, 7)),
                 kind=[_lib.ACTION_GRIP], xyz_from_start=[0], grip_ticks=[2], kp=[1.0], max_error=[0.01], min_speed=[0.01], max_speed=[1.0],
                 gripper_force=[0.1])
    assert set_ts() == 0
    osc.set_waypoints(path, 0.01)
    assert state_rc() == ERR_STATE and wp_rc() == 0
    assert set_ts() == 0 and state_rc() == 0 and wp_rc() == ERR_STATE
    osc.set_action_list(grips)
    assert state_rc() == ERR_STATE and al_rc() == 0
    assert set_ts() == 0 and state_rc() == 0 and al_rc() == ERR_STATE
    osc.set_waypoints(None, 0.01)
    osc.set_action_list(None)
    assert state_rc() == 0
    osc.set_targets(tgt0)                                # (the list wrote targets; back to the start for the mirror)
    osc.upload_q(q, qd)
    assert set_ts() == 0
    osc.rollout(1)
    assert follows_mirror(0)
    assert lib.irlosc_set_teleop_stream(h, 0, B, None, None, None) == 0 and wp_rc() == ERR_STATE and al_rc() == ERR_STATE
    osc.set_waypoints(path, 0.01)
    assert lib.irlosc_set_teleop_stream(h, 0, B, None, None, None) == 0 and wp_rc() == 0      # a NULL stream description leaves paths alone
    assert set_ts(ticks=0) == ERR_ARG and wp_rc() == 0                                         # ... and so does a refused one
    assert set_ts() == 0
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    assert state_rc() == ERR_STATE
    osc.close()


def test_a_slot_whose_stream_was_cleared_rolls_out_like_one_that_never_had_one():
    B = 70
    osc = make_ctx(B, n_slots=2)
    fill(osc, B, slot=0)
    osc.set_teleop_stream(readings_of(SEED), ORIGIN, slot=0)
    mid = osc.rollout(3, slot=0)
    osc.clear_teleop_stream(slot=0)
    osc.upload_q(mid["qpos"], mid["qvel"], slot=1)
    osc.set_targets(osc.download_targets(0), slot=1)
    a, b = osc.rollout(5, slot=0), osc.rollout(5, slot=1)
    assert all(same_bits(a[k], b[k]) for k in ("qpos", "qvel", "u", "flags_any"))
    assert same_bits(osc.download_targets(0), osc.download_targets(1))
    osc.close()


# ---- 8. a robot that holds a NaN ------------------------------------------------------------------------------------------------------------
def test_a_robot_with_a_nan_coordinate_leaves_its_neighbours_alone():
    B, sick = 70, 3
    q, qd = start_state(B)
    res = []
    for nan in (False, True):
        qq = np.array(q)
        if nan:
            qq[sick, 2] = np.nan
        osc = make_ctx(B)
        osc.upload_q(qq, qd)
        osc.set_targets(start_targets(B, 3))
        osc.set_teleop_stream(fleet_readings(B), ORIGIN)
        out = osc.rollout(8)
        res.append((out, osc.teleop_state(), osc.download_targets()))
        osc.close()
    (oa, sa, ta), (ob, sb, tb) = res
    others = np.arange(B) != sick
    assert np.isnan(ob["qpos"][sick]).any()
    assert same_bits(oa["qpos"][others], ob["qpos"][others]) and same_bits(oa["qvel"][others], ob["qvel"][others])
    assert same_bits(ta, tb) and same_bits(sa["pose"], sb["pose"])      # the stream reads nothing of the robot's state: it is steered like every other
