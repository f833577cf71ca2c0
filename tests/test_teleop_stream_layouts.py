"""The teleoperation stream off k13 and in front of the FROMQ form (-m gpu): what tests/test_teleop_stream.py holds on k13 and r6 (three
devices RIGID / RIGID / HEADING or one device, the lane form of the fused OSC step, max_batch == B, one slot with a stream), here with
everything osc_teleop_kernel, teleop_args and tick_front take as a runtime argument at another value:

    k12_admit, _f32    two devices, tile row 14, a sensor feed whose wrench admittance reads        lane form on the layout's own kernel
    br7                HEADING on device 0, RIGID on device 1                                       lane form, tier (1, 6, 6)
    rlbr10             four devices, tile row 28: RIGID on 0, 1 and 3 (0 and 3 one arm), HEADING 2   lane form, tier (1, 6, 6)
    rlb16, _f32        no lane tier: task pass + row16 kernel in 16-robot blocks                    row16 FROMQ form, KMAX 16
    rlb11_branch_b     target velocities, which the stream leaves alone; the base first             row16 FROMQ form by the branch-B rule
    k13_lane0          IRLOSC_LANE=0 on the layout the other tests know                             row16 FROMQ form
    k7                 tier (1, 3, 3): the RIGID quaternion words are written though no row reads them
    k13_none           k13 with the rig RIGID / NONE / HEADING: a NONE follower between two live ones
    k13_heading_only   k13 with the rig NONE / NONE / HEADING: no RIGID follower at all
    k13_wide, rlbr10_wide    max_batch = 130 holding 70 robots: the pose planes' stride is not B
    rlb16_feed         rlb16 with the F/T sensors described (the companions of test 10)
    k13                the layout of test_teleop_stream.py, for the two slots of test 8

Every context asserts its route from from_q_name / kernel_name (open_case).  B = 70 (one full walk wave and a ragged one of 6 robots; on the
FROMQ form four full 16-robot blocks and a ragged one of 6) and B = 1; T = 48 readings of space_mouse_stream, robot b on seed 5 + b;
start_state and start_targets are test_teleop_stream's, so every word the stream does not write tells its robot and device.

The bounds are those of tests/test_teleop_stream.py and tests/test_gpu_parity.py, none of them chosen here: bit for bit unless named;
BOUND = 1e-12 on angles (mod 2 pi) and float64 target words, one float32 ulp of the mirror's cast on float32 target words (both derived in
that file's docstring), the wrap margin asserted on the mirror (its smallest distance from +-pi over seeds 5 .. 201 and 48 ticks is 2.6e-5
against WRAP_MARGIN = 1e-6: B stays <= 197 and T = 48 wherever the mirror is compared); TOL64 = 1e-5 relative on the parity domain with
at least 90 % of the robots in it, asserted on the oracle's own numbers.

1. device against the mirror, tick by tick;  2. a slot fed the stream's targets by the host;  3. pieces;  4. the torques of a stream tick
against the float64 oracles;  5. a NaN robot on the FROMQ form;  6. a narrower rollout on the FROMQ form;  7. stride (cases of 1 and 3);
8. two slots, two streams;  9. end and loop on the FROMQ form;  10. companions off k13;  11. the log off k13.
Measured figures, the mutants these tests were run against and the durations: profiles/teleop_stream_layouts.md."""
import numpy as np
import pytest

import test_fromq_sensor_feed as tf
import test_joints as tjn
import test_rollout as tr
import test_teleop_stream as tts
import test_walls as twl
from test_gpu_parity import TOL64, in_parity_domain, rel_err
from test_rollout_layouts import ROUTES, open_ctx
from test_teleop_stream import angle_diff, fleet_readings, mirror, same_bits, start_state, start_targets
from irl_control_amd import _lib, synth, teleop
from irl_control_amd.rigid_body import RigidBodyModel
from oracle import osc_oracle

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
T, SEED, BOUND, ORIGIN = tts.T, tts.SEED, tts.BOUND, tts.ORIGIN
NONE, RIGID, HEADING = teleop.NONE, teleop.RIGID, teleop.HEADING
BAD = _lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD
NS = tr.NS
WIDE = 130

# case: route (a key of test_rollout_layouts.ROUTES; None: the (1, 6, 6) lane tier on the layout's own kernel instantiation), layout, dtype,
# feed (F/T sensors and a reading), tvel (target velocities), kinds (the demo's rig with these kinds; default: the demo's), max_batch
CASES = {
    "k12_admit": dict(route=None, cfg="k12_admit", dtype=F64, feed=True),
    "k12_admit_f32": dict(route=None, cfg="k12_admit", dtype=F32, feed=True),
    "br7": dict(route="br7", cfg="br7", dtype=F64),
    "rlbr10": dict(route="rlbr10", cfg="rlbr10", dtype=F64),
    "rlb16": dict(route="rlb16", cfg="rlb16", dtype=F64),
    "rlb16_f32": dict(route="rlb16", cfg="rlb16", dtype=F32),
    "rlb11_branch_b": dict(route="rlb11_branch_b", cfg="rlb11_branch_b", dtype=F64, tvel=True),
    "k13_lane0": dict(route="k13_lane0", cfg="k13", dtype=F64),
    "k7": dict(route="k7", cfg="k7", dtype=F64),
    "k13_none": dict(route=None, cfg="k13", dtype=F64, kinds=(RIGID, NONE, HEADING)),
    "k13_heading_only": dict(route=None, cfg="k13", dtype=F64, kinds=(NONE, NONE, HEADING)),
    "k13": dict(route=None, cfg="k13", dtype=F64),
    "k13_wide": dict(route=None, cfg="k13", dtype=F64, max_batch=WIDE),
    "rlbr10_wide": dict(route="rlbr10", cfg="rlbr10", dtype=F64, max_batch=WIDE),
    "rlb16_feed": dict(route="rlb16", cfg="rlb16", dtype=F64, feed=True),
}
TABLE = ["k12_admit", "k12_admit_f32", "br7", "rlbr10", "rlb16", "rlb16_f32", "rlb11_branch_b", "k13_lane0", "k7", "k13_none", "k13_heading_only"]
STRIDE = ["k13_wide", "rlbr10_wide"]
FROMQ = [c for c in TABLE if CASES[c]["route"] is not None and (ROUTES[CASES[c]["route"]][2] is None or CASES[c].get("tvel"))]
assert FROMQ == ["rlb16", "rlb16_f32", "rlb11_branch_b", "k13_lane0"]


def layout_of(case):
    return synth.make_layout(CASES[case]["cfg"])


def rig_of(case):
    """The demo's followers for the case's layout, the devices its `kinds` name NONE dropped."""
    rig = teleop.space_mouse_rig(layout_of(case))
    for d, kind in enumerate(CASES[case].get("kinds", ())):
        assert kind in (NONE, rig[d]["kind"])
        if kind == NONE:
            rig[d] = teleop.follower()
    return rig


def open_case(case, B, monkeypatch, n_slots=1):
    """A context of the case that holds B robots (capacity: the case's max_batch, else B) with the plant of test_teleop_stream.make_ctx and,
    where the case has a feed, the F/T sensors described; the route asserted.  -> osc"""
    c = CASES[case]
    cap = c.get("max_batch") or B
    kw = dict(feed=bool(c.get("feed")), n_slots=n_slots)
    if c["route"] is not None:
        osc = open_ctx(c["route"], cap, c["dtype"], monkeypatch, **kw)[4]
    else:
        osc = tr.make_ctx(c["cfg"], cap, c["dtype"], **kw)[4]
        fq, kn = osc.from_q_name, osc.kernel_name
        assert "fused" in fq and "row16" in kn and "_pad" not in kn, (fq, kn)
        if c["dtype"] is F64:
            assert "osc_lane" in fq and "_rows_1_6_6 " in fq, fq
        else:      # (float32 records: the float32 context's own form; where it reports the lane form, that tier)
            assert "osc_lane" not in fq or "_rows_1_6_6 " in fq, fq
    assert osc.max_batch == cap and osc.layout.ndev == layout_of(case).ndev
    osc.set_plant(tts.DT, tts.DAMPING)
    return osc


def extras(case, B):
    """What fill() gives a slot of the case beyond the start state and targets: target velocities (0.1 x synth.make_batch's, which keep
    every third robot on branch A) and the reading of the sensor feed -- the first B rows of the arrays for 70 robots."""
    c = CASES[case]
    out = {}
    if c.get("tvel"):
        out["tgt_vel"] = 0.1 * synth.make_batch(c["cfg"], 70, seed=21)[2]["tgt_vel"][:B]
    if c.get("feed"):
        out["sens"] = np.random.default_rng(43).normal(0.0, 5.0, size=(70, NS))[:B]
    return out


def readings(B):
    return fleet_readings(B) if B > 1 else tts.readings_of(SEED)


def stepped(case, B, monkeypatch):
    """test_teleop_stream.stepped on the case: T x rollout(1) with downloads behind each tick, and the mirror.  Once per (case, B)."""
    c = CASES[case]
    return tts.stepped(c["cfg"], B, c["dtype"], rig=rig_of(case), name="layouts " + case, open_ctx=lambda: open_case(case, B, monkeypatch),
                       **extras(case, B))


def start(osc, case, B, slot=0, stream=True, q=None, **kw):
    """The slot at the start: state (or the coordinates q), start targets, the case's extras and (stream) the per-robot stream."""
    tts.fill(osc, B, slot=slot, **extras(case, B))
    if q is not None:
        osc.upload_q(q, start_state(B)[1], slot=slot)
    if stream:
        osc.set_teleop_stream(readings(B), ORIGIN, rig=rig_of(case), slot=slot, **kw)


# ---- 1. / 7. device against the mirror, tick by tick -----------------------------------------------------------------------------------
def assert_unwritten_words_stay(case, B, tgt):
    """tgt [ticks, B, ndev, 7]: all seven words of a NONE device and the xyz of a HEADING device equal start_targets on every tick, on bits."""
    want = start_targets(B, tgt.shape[2]).astype(tgt.dtype)
    for d, f in enumerate(rig_of(case)):
        words = {NONE: slice(0, 7), HEADING: slice(0, 3)}.get(f["kind"])
        if words is not None:
            for t in range(len(tgt)):
                assert same_bits(np.ascontiguousarray(tgt[t, :, d, words]), np.ascontiguousarray(want[:, d, words])), (d, t)


@pytest.mark.parametrize("B", [70, 1])
@pytest.mark.parametrize("case", TABLE + STRIDE)
def test_device_follows_the_mirror_tick_by_tick_per_case(case, B, monkeypatch):
    """The assertions of test_teleop_stream.test_device_follows_the_mirror_tick_by_tick (x, y, z on bits; angles mod 2 pi and float64 target
    words within 1e-12; float32 target words within one float32 ulp of the mirror's cast; the setter wrote no target), and on every tick
    the words no follower writes are start_targets' on bits.  The wide cases also equal, on bits, the run of the tight context.
    Observed on an MI355X: profiles/teleop_stream_layouts.md."""
    run = stepped(case, B, monkeypatch)
    dtype = CASES[case]["dtype"]
    assert run["dev"]["tgt"].shape == (T, B, layout_of(case).ndev, 7)
    tts.assert_follows_the_mirror(run, B, dtype, case)
    assert_unwritten_words_stay(case, B, run["dev"]["tgt"])
    assert not np.any(run["dev"]["flags"] & BAD)
    if case in STRIDE:
        tight = stepped(case[:-len("_wide")], B, monkeypatch) if case != "k13_wide" else tts.stepped("k13", B, F64)
        for key in ("q", "qd", "u", "flags", "pose", "tgt"):
            assert same_bits(run["dev"][key], tight["dev"][key]), key


# ---- 2. the same tick, nothing else changed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [70, 1])
@pytest.mark.parametrize("case", TABLE)
def test_a_slot_fed_the_streams_targets_by_the_host_steps_bit_for_bit_alike_per_case(case, B, monkeypatch):
    """The protocol of test_teleop_stream's test 2: slot 0 runs the stream; slot 1 has no program and gets slot 0's targets of tick t by
    set_targets before its tick t -- with the same sensor reading and the same target velocities where the case has them: qpos, qvel, u and
    flags_any on bits, every tick.  rlb11_branch_b, B = 70: more than half the robots of slot 1 (the reference run) carry
    FLAG_VEL_BRANCH_B, and slot 0's flags are slot 1's."""
    osc = open_case(case, B, monkeypatch, n_slots=2)
    x = extras(case, B)
    start(osc, case, B, slot=0)
    start(osc, case, B, slot=1, stream=False)
    seen = np.zeros(B, np.uint32)
    for t in range(T):
        a = osc.rollout(1, slot=0)
        osc.set_targets(osc.download_targets(0), x.get("tgt_vel"), slot=1)
        b = osc.rollout(1, slot=1)
        for k in ("qpos", "qvel", "u", "flags_any"):
            assert same_bits(a[k], b[k]), (t, k)
        seen |= b["flags_any"]
    assert osc.teleop_state(0)["tick"] == T
    osc.close()
    assert not np.any(seen & BAD)
    if CASES[case].get("tvel") and B > 1:
        assert ((seen & _lib.FLAG_VEL_BRANCH_B) != 0).mean() > 0.5


# ---- 3. / 7. pieces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [70, 1])
@pytest.mark.parametrize("case", TABLE + STRIDE)
def test_pieces_of_a_rollout_add_up_per_case(case, B, monkeypatch):
    """rollout(48) = 48 x rollout(1) = rollout(5) + rollout(43): qpos, qvel, pose, targets on bits, and the tick."""
    run = stepped(case, B, monkeypatch)
    for pieces in ((T,), (5, T - 5)):
        osc = open_case(case, B, monkeypatch)
        start(osc, case, B)
        for p in pieces:
            out = osc.rollout(p)
        st, tg = osc.teleop_state(), osc.download_targets()
        osc.close()
        assert st["tick"] == T
        assert same_bits(out["qpos"], run["dev"]["q"][-1]) and same_bits(out["qvel"], run["dev"]["qd"][-1]), pieces
        assert same_bits(st["pose"], run["dev"]["pose"][-1]) and same_bits(tg, run["dev"]["tgt"][-1]), pieces


# ---- 4. the torques of a stream tick against the float64 oracles ------------------------------------------------------------------------------
ORACLE_CASES = ["k12_admit", "br7", "rlbr10", "rlb16", "rlb11_branch_b", "k13_lane0"]
_ORACLE = {}


def oracle_at_start(cfg):
    """test_fromq_sensor_feed.oracle_records_and_wrench at start_state(70) -- oracle/rigid_body.py's records in cfg's device order and the
    host restatement of the feed on extras()' reading.  Once per layout."""
    if cfg not in _ORACLE:
        lay = synth.make_layout(cfg)
        q, qd = start_state(70)
        sens = np.random.default_rng(43).normal(0.0, 5.0, size=(70, NS))
        _ORACLE[cfg] = tf.oracle_records_and_wrench(lay, RigidBodyModel.load("dual_ur5").ft_desc(lay.dev_names), q, qd, sens)
    return _ORACLE[cfg]


ORACLE_TICKS = [(case, tick) for case in ORACLE_CASES for tick in (0, T - 1)] + [(case, "eigen") for case in ORACLE_CASES if case in FROMQ]


@pytest.mark.parametrize("case,tick", ORACLE_TICKS)
def test_the_torques_of_a_stream_tick_against_the_oracles(case, tick, monkeypatch):
    """B = 70, ticks 0 and 47 of the tick-by-tick run.  Into the oracle go: the state in front of the tick (tick 0: start_state; tick t: the
    coordinates downloaded behind tick t - 1), the MIRROR's targets of that tick (not the device's), the wrench of the host restatement of
    the feed (oracle site frames; no feed: none) and the slot's target velocities.  oracle/rigid_body.records chained into
    osc_oracle.generate_batch; the tick's u within TOL64 = 1e-5 relative on the parity domain, with at least 90 % of the 70 robots in the
    domain by the oracle's own numbers.
    The give-up pass of the FROMQ form reads "this tick's targets" too, and start_state does not reach it: on an MI355X no robot carries
    FLAG_EIGEN_PATH on tick 0 on any FROMQ case, and on tick 47 none does on rlb11_branch_b (rlb16 and k13_lane0: 20 of 70; printed per
    case and tick).  So every FROMQ case has a third tick, "eigen": the LAST tick of the run on which some robot carries the flag -- asserted
    to exist, with at least one such robot in the parity domain -- held to the oracle like the other two (rlb16, k13_lane0: tick 47 again,
    robots flagged from tick 10 on; rlb11_branch_b: tick 46, one robot on ticks 29 .. 33 and 43 .. 46).
    Observed on an MI355X (printed): profiles/teleop_stream_layouts.md."""
    B = 70
    c = CASES[case]
    lay = layout_of(case)
    run, x = stepped(case, B, monkeypatch), extras(case, B)
    dev = run["dev"]
    want_eigen = tick == "eigen"
    if want_eigen:
        flagged = np.flatnonzero(((dev["flags"] & _lib.FLAG_EIGEN_PATH) != 0).any(axis=1))
        assert len(flagged), "no robot on the eigen path on any tick of the run: the give-up pass was not met"
        tick = int(flagged[-1])
    if tick == 0:
        R, W = oracle_at_start(c["cfg"])
    else:
        R, W = tf.oracle_records_and_wrench(lay, RigidBodyModel.load("dual_ur5").ft_desc(lay.dev_names), dev["q"][tick - 1], dev["qd"][tick - 1],
                                            x.get("sens", np.zeros((B, NS))))
    gains = synth.make_batch(c["cfg"], 1, seed=0)[1]
    ref = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], run["tgts"][tick],
                                    W if c.get("feed") else None, x.get("tgt_vel"))
    inertia = [osc_oracle.task_inertia(R["J"][b], R["M"][b])[2:] for b in range(B)]
    dom = np.array([in_parity_domain(Mxi, det) for Mxi, det in inertia])
    pinv = np.array([abs(det) < 1e-4 for _, det in inertia])
    eig = (dev["flags"][tick] & _lib.FLAG_EIGEN_PATH) != 0
    err = rel_err(dev["u"][tick].astype(F64), ref)
    print(f"[oracle {case} tick {tick}] in the parity domain {int(dom.sum())}/{B}, on the pinv branch {int(pinv.sum())}, on the eigen path "
          f"{int(eig.sum())}; u against the oracle in the domain: max rel err {err[dom].max() if dom.any() else float('nan'):.3g} (bound {TOL64:g})")
    assert dom.mean() >= 0.9, int(dom.sum())
    assert not np.any(dev["flags"][tick] & BAD)
    if want_eigen:
        assert (eig & dom).any(), "no robot on the eigen path in the parity domain"
    assert err[dom].max() <= TOL64, (float(err[dom].max()), int(np.argmax(np.where(dom, err, 0.0))))


# ---- 5. a robot that holds a NaN, on the FROMQ form ---------------------------------------------------------------------------------------------
_CLEAN = {}


def eight_ticks(case, B, monkeypatch, sick=None):
    q = np.array(start_state(B)[0])
    if sick is not None:
        q[sick, 2] = np.nan
    osc = open_case(case, B, monkeypatch)
    start(osc, case, B, q=q)
    out = osc.rollout(8)
    res = (out, osc.teleop_state(), osc.download_targets())
    osc.close()
    return res


@pytest.mark.parametrize("where", ["first", "mid_block", "ragged_last"])
@pytest.mark.parametrize("case", ["rlb16", "k13_lane0"])
def test_a_robot_with_a_nan_coordinate_leaves_its_neighbours_alone_on_the_fromq_form(case, where, monkeypatch):
    """The assertion of test_teleop_stream's test 8 where robots share 16-robot blocks of the row16 FROMQ kernel as well as waves: robot 0,
    robot 37 (healthy robots on either side in its block) or robot 69 (the last of the ragged block) holds a NaN; every other robot's
    coordinates are those of the run without it, on bits, and its own pose and targets are steered like everybody's."""
    B = 70
    sick = dict(first=0, mid_block=37, ragged_last=B - 1)[where]
    if case not in _CLEAN:
        _CLEAN[case] = eight_ticks(case, B, monkeypatch)
    (oa, sa, ta), (ob, sb, tb) = _CLEAN[case], eight_ticks(case, B, monkeypatch, sick)
    others = np.arange(B) != sick
    assert np.isnan(ob["qpos"][sick]).any() and (ob["flags_any"][sick] & BAD) and not np.any(oa["flags_any"] & BAD)
    assert same_bits(oa["qpos"][others], ob["qpos"][others]) and same_bits(oa["qvel"][others], ob["qvel"][others])
    assert same_bits(oa["u"][others], ob["u"][others]) and np.array_equal(oa["flags_any"][others], ob["flags_any"][others])
    assert same_bits(ta, tb) and same_bits(sa["pose"], sb["pose"]) and sa["tick"] == sb["tick"] == 8
    assert not same_bits(ta, start_targets(B, ta.shape[1]))


# ---- 6. a narrower rollout on the FROMQ form ------------------------------------------------------------------------------------------------------
def test_a_narrower_rollout_on_the_fromq_form(monkeypatch):
    """The protocol of the last part of test_teleop_stream's test 4 on rlb16: irlosc_rollout_from_q over n = 40 of the 70 robots, which cuts
    the 16-robot block of robots 32 .. 47, for 5 ticks of a shared stream with origins per robot.  Robots >= 40 keep pose and targets on
    bits, robots < 40 follow the mirror, the tick counts for the slot: a tick over all 70 then gives reading 5 to every robot."""
    case, B, n = "rlb16", 70, 40
    rd = tts.readings_of(SEED)
    rng = np.random.default_rng(7)
    origins = ORIGIN + np.concatenate([rng.uniform(-0.1, 0.1, (B, 3)), rng.uniform(-0.3, 0.3, (B, 3))], axis=1)
    rig = rig_of(case)
    tgt0 = start_targets(B, len(rig))
    poses, tgts = mirror(origins, rd, rig, tgt0, B)
    osc = open_case(case, B, monkeypatch)
    start(osc, case, B, stream=False)
    osc.set_teleop_stream(rd, origins, rig=rig)
    assert osc.lib.irlosc_rollout_from_q(osc._h, 0, n, 5, 0, None, None, None) == 0
    st, tg = osc.teleop_state(), osc.download_targets()
    assert st["tick"] == 5
    assert same_bits(st["pose"][n:], origins[n:]) and same_bits(tg[n:], tgt0[n:])
    assert same_bits(st["pose"][:n, :3], poses[4][:n, :3]) and angle_diff(st["pose"][:n, 3:], poses[4][:n, 3:]).max() <= BOUND
    assert np.abs(tg[:n] - tgts[4][:n]).max() <= BOUND
    osc.upload_q(*start_state(B))
    osc.rollout(1)                                       # tick 5 over all B robots: reading 5 for every robot
    st, tg = osc.teleop_state(), osc.download_targets()
    osc.close()
    late = [teleop.stream_step(origins[b], rd[5], rig) for b in range(n, B)]
    assert st["tick"] == 6
    assert same_bits(st["pose"][n:, :3], np.array([p[:3] for p, _ in late]))
    assert angle_diff(st["pose"][n:, 3:], np.array([p[3:] for p, _ in late])).max() <= BOUND
    want = np.array([np.where(np.isnan(t), tgt0[n + i], t) for i, (_, t) in enumerate(late)])
    assert np.abs(tg[n:] - want).max() <= BOUND
    assert same_bits(st["pose"][:n, :3], poses[5][:n, :3]) and np.abs(tg[:n] - tgts[5][:n]).max() <= BOUND


# ---- 8. two slots, two streams ----------------------------------------------------------------------------------------------------------------------
def swapped_rig():
    """The demo's k13 rig with the two arms' offsets exchanged and the base's heading offset + pi / 2."""
    demo = teleop.space_mouse_rig(synth.make_layout("k13"))
    return [teleop.follower(RIGID, demo[1]["off_xyz"], demo[1]["off_quat"]), teleop.follower(RIGID, demo[0]["off_xyz"], demo[0]["off_quat"]),
            teleop.follower(HEADING, heading_offset=np.pi / 2)]


@pytest.mark.parametrize("first", ["per_robot", "shared"])
def test_two_slots_with_streams_of_their_own(first, monkeypatch):
    """One k13 context, B = 70, two slots with rollouts interleaved 1 : 1 for 12 ticks.  Slot 0: the demo rig at the demo's origin on
    per-robot readings of seeds 5 + b (first = shared: on the one stream of seed 5).  Slot 1: the swapped rig on the one stream of seed 99
    with origins per robot.  Each slot's qpos, qvel, pose and targets equal, on bits, those of a context that ran that slot's stream alone
    in one rollout(12); and the two slots differ from each other."""
    B, ticks = 70, 12
    rng = np.random.default_rng(7)
    origins = ORIGIN + np.concatenate([rng.uniform(-0.1, 0.1, (B, 3)), rng.uniform(-0.3, 0.3, (B, 3))], axis=1)
    demo = teleop.space_mouse_rig(synth.make_layout("k13"))
    streams = [dict(readings=fleet_readings(B) if first == "per_robot" else tts.readings_of(SEED), origin=ORIGIN, rig=demo),
               dict(readings=tts.readings_of(99), origin=origins, rig=swapped_rig())]

    def state_of(osc, out, slot):
        return dict(qpos=out["qpos"], qvel=out["qvel"], pose=osc.teleop_state(slot)["pose"], tgt=osc.download_targets(slot),
                    tick=osc.teleop_state(slot)["tick"])

    alone = []
    for s in streams:
        osc = open_case("k13", B, monkeypatch)
        tts.fill(osc, B)
        osc.set_teleop_stream(**s)
        alone.append(state_of(osc, osc.rollout(ticks), 0))
        osc.close()
    osc = open_case("k13", B, monkeypatch, n_slots=2)
    for slot, s in enumerate(streams):
        tts.fill(osc, B, slot=slot)
        osc.set_teleop_stream(slot=slot, **s)
    for _ in range(ticks):
        outs = [osc.rollout(1, slot=slot) for slot in (0, 1)]
    both = [state_of(osc, outs[slot], slot) for slot in (0, 1)]
    osc.close()
    for slot in (0, 1):
        assert both[slot]["tick"] == alone[slot]["tick"] == ticks
        for key in ("qpos", "qvel", "pose", "tgt"):
            assert same_bits(both[slot][key], alone[slot][key]), (slot, key)
    assert not same_bits(alone[0]["tgt"], alone[1]["tgt"]) and not same_bits(alone[0]["pose"], alone[1]["pose"])


# ---- 9. end and loop on the FROMQ form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [70, 1])
def test_a_stream_ends_or_loops_after_its_last_reading_on_the_fromq_form(B, monkeypatch):
    """test_teleop_stream's test 5 on rlb16: no launch after the last reading while the tick counts on; a looped stream reads reading 0
    again."""
    osc = open_case("rlb16", B, monkeypatch)
    tts.assert_ends_or_loops(osc, B, rig_of("rlb16"), lambda: start(osc, "rlb16", B, stream=False))
    osc.close()


# ---- 10. companions off k13 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k12_admit", "rlb16_feed"])
def test_the_stream_beside_a_feed_walls_and_joint_rows(case, monkeypatch):
    """B = 70, 24 ticks; every slot has the feed's reading, one wall per arm and the joint rows of test_joints.scene.  A wall is the plane
    through the arm's EE position at start_state (oracle/rigid_body.py's) with the normal along -x of the world and test_walls' radius,
    stiffness and damping: the EE sphere is inside it from tick 0.  Slot 0: the stream, rollout(24).  Slot 1: the stream, 24 x rollout(1).
    Slot 2 (the reference): no program, slot 1's targets of the tick by set_targets.  Asserted on slot 2: wall_state reports contact behind
    tick 0 for at least half the robots, and the rows give a torque within the run.  Then slot 1 = slot 2 tick by tick on qpos, qvel, u,
    flags_any and the walls' and rows' state, and slot 0 = slot 1 at the end, all on bits."""
    B, ticks = 70, 24
    lay = layout_of(case)
    ee = oracle_at_start(CASES[case]["cfg"])[0]["ee_pose"]
    arms = [d for d, nm in enumerate(lay.dev_names) if nm != "base"]
    walls = [dict(dev=d, normal=(-1.0, 0.0, 0.0), point=ee[:, d, :3], radius=twl.R1, stiffness=twl.K1, damping=twl.C1) for d in arms]
    rows = tjn.scene(lay)
    osc = open_case(case, B, monkeypatch, n_slots=3)
    x = extras(case, B)
    for slot in (0, 1, 2):
        start(osc, case, B, slot=slot, stream=slot < 2)
        osc.set_walls(walls, slot=slot)
        osc.set_joints(rows, slot=slot)
    whole = osc.rollout(ticks, slot=0)
    tau_seen, touched0 = False, None
    for t in range(ticks):
        a = osc.rollout(1, slot=1)
        osc.set_targets(osc.download_targets(1), x.get("tgt_vel"), slot=2)
        b = osc.rollout(1, slot=2)
        for k in ("qpos", "qvel", "u", "flags_any"):
            assert same_bits(a[k], b[k]), (t, k)
        wa, wb, ja, jb = osc.wall_state(1), osc.wall_state(2), osc.joint_state(1), osc.joint_state(2)
        for got, want in ((wa, wb), (ja, jb)):
            for k in want:
                assert same_bits(got[k], want[k]), (t, k)
        if t == 0:
            touched0 = (wb["contact_ticks"][:, arms] > 0).all(axis=1)
        tau_seen = tau_seen or bool(jb["tau"].any())
        assert not np.any(b["flags_any"] & BAD), t
    print(f"[companions {case}] robots in contact behind tick 0: {int(touched0.sum())}/{B}; largest wall force of the last tick "
          f"{np.abs(wb['force']).max():.3g} N, largest row torque {np.abs(jb['tau']).max():.3g} N m")
    assert touched0.mean() >= 0.5 and wb["force"].any()
    assert tau_seen
    for k in ("qpos", "qvel", "u"):
        assert same_bits(whole[k], a[k]), k
    assert osc.teleop_state(0)["tick"] == osc.teleop_state(1)["tick"] == ticks
    assert same_bits(osc.teleop_state(0)["pose"], osc.teleop_state(1)["pose"]) and same_bits(osc.download_targets(0), osc.download_targets(1))
    for got, want in ((osc.wall_state(0), wa), (osc.joint_state(0), ja)):
        for k in want:
            assert same_bits(got[k], want[k]), k
    osc.close()


# ---- 11. the log off k13 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rlb16", "rlbr10"])
def test_the_logged_targets_of_a_stream_tick_are_that_ticks(case, monkeypatch):
    """B = 70, rollout_logged(24, targets + ee_pose + u + flags, every tick).  The stream writes in front of the OSC step and nothing moves
    the targets behind it, so the TARGETS sample of tick t is download_targets behind tick t of the tick-by-tick run, on bits, and the
    mirror's targets of tick t within BOUND; u and flags are that run's of the tick, on bits.  The EE poses of tick 0 against
    oracle/rigid_body.py's at start_state at the tolerance test_one_tick_against_the_cpu_oracles_per_layout holds the EE trace to (1e-10 of
    the robot's largest entry), those of tick t against the coordinates of the tick-by-tick run through the next sample: the log's
    ee_pose[t] belongs to the state in front of tick t."""
    B, ticks = 70, 24
    run = stepped(case, B, monkeypatch)
    osc = open_case(case, B, monkeypatch)
    start(osc, case, B)
    r = osc.rollout_logged(ticks, ["targets", "ee_pose", "u", "flags"])
    st = osc.teleop_state()
    osc.close()
    log, dev = r["log"], run["dev"]
    assert sorted(log) == ["ee_pose", "flags", "targets", "u"] and np.array_equal(r["log_ticks"], np.arange(ticks)) and st["tick"] == ticks
    assert same_bits(log["targets"], np.ascontiguousarray(dev["tgt"][:ticks]))
    assert np.abs(log["targets"] - run["tgts"][:ticks]).max() <= BOUND
    assert same_bits(log["u"], np.ascontiguousarray(dev["u"][:ticks])) and np.array_equal(log["flags"], dev["flags"][:ticks])
    assert same_bits(r["qpos"], dev["q"][ticks - 1]) and same_bits(st["pose"], dev["pose"][ticks - 1])
    ee = oracle_at_start(CASES[case]["cfg"])[0]["ee_pose"]
    scale = np.abs(ee).reshape(B, -1).max(axis=1)[:, None, None]
    err = np.abs(log["ee_pose"][0] - ee) / scale
    print(f"[log {case}] ee_pose of tick 0 against the oracle: {err.max():.3g} of the robot's largest entry (bound 1e-10)")
    assert err.max() <= 1e-10
    assert all((log["ee_pose"][t + 1] != log["ee_pose"][t]).any() for t in range(ticks - 1))

