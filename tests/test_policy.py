"""A learned policy on the GPU (-m gpu): irlosc_set_policy / irlosc_download_policy_state -- the policy kernel (csrc/osc_policy.hpp) in
front of the OSC step of a rollout tick.  The network's output against its NumPy mirror (policy.mlp) BIT FOR BIT -- which is also the
check that v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain on this hardware --, the observation against the tick's log channels, the
policy against a stream that replays its outputs, in pieces, with zero weights, its grip on the joint rows, next to episodes, next to a
robot that holds a NaN, and the state rules.

Shapes: B = 70 (one full wave and a ragged one of 6 robots) and B = 1; T = 6 ticks; float64 and float32 contexts; k13 (three devices)
and r6 (one).  Helpers, start states and the BOUND of 1e-12 on angles and target words are tests/test_teleop_stream.py's.

NETS.  "one": a single layer on qpos | qvel | ee_pose | targets (92 -> 7 on k13).  "odd": qpos | plate = 31 -> 20 -> 7, no width a
multiple of 4 or 16.  "deep": every channel, 116 + 14 (two objects) = 130 -> 128 -> 128 -> 128 -> 7, on a slot with a sensor feed, a sensed
push, joint rows, an object the right hand carries from tick 0 and its weight.  Weights are N(0, 1 / in), biases N(0, 1): sums of tens of
terms of mixed sign and like size, on which float32 addition is far from associative -- every test that compares against the mirror first
asserts that the mirror summed in DESCENDING order differs from the ascending one on at least half of the outputs it is about to compare.

THE OBSERVATION's targets are the slot's targets in front of the tick's write (include/irlosc.h), so they are compared with the targets
downloaded before the tick -- which for t >= 1 are asserted to be the log's `targets` of tick t - 1; the log's `targets` of tick t itself
hold the policy's write of that tick.  Every other channel is the log's of the same tick."""
import ctypes as C

import numpy as np
import pytest

import test_action_list as tal
import test_joints as tjn
import test_pushes as tp
import test_teleop_stream as tts
from irl_control_amd import _lib, object_loads as ol, objects as ob, policy, synth, teleop
from irl_control_amd.rigid_body import RigidBodyModel
from test_teleop_stream import BOUND, ORIGIN, angle_diff, same_bits, start_state, start_targets

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
F64, F32 = np.float64, np.float32
T = 6
CLIP = 0.5
GRIP = (-0.4, 0.4)                                  # close, open
NETS = {"one": (("qpos", "qvel", "ee_pose", "targets"), ()),
        "odd": (("qpos", "plate"), (20,)),
        "deep": (policy.OBS_BITS, (128, 128, 128))}
CH = ("qpos", "qvel", "ee_pose", "targets", "wrench", "u", "object_pose")
_RUNS = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def layers_of(n_in, hidden, n_out, seed):
    rng = np.random.default_rng(seed)
    dims = (n_in,) + tuple(hidden) + (n_out,)
    return [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), rng.standard_normal(o).astype(F32)) for i, o in zip(dims[:-1], dims[1:])]


def order_shows(obs, layers):
    up, down = policy.mlp(obs, layers), policy.mlp(obs, layers, descending=True)
    frac = (bits(up) != bits(down)).mean()
    assert frac >= 0.5, f"descending and ascending chains agree on {1 - frac:.0%} of the outputs: this data would not tell the orders apart"
    return up


def rig_of(cfg):
    return teleop.space_mouse_rig(synth.make_layout(cfg))


def scene(osc, B, slot, full):
    """The start state and targets of the slot; `full`: on a zero sensor feed with a push on the right arm that is applied and sensed on
    ticks 1 .. 4, the joint rows but for the drives, one object in the right hand (its knuckle starts closed: the rising edge of tick 0 takes the plug lying
    at the grip point) and one out of reach, and the plug's weight."""
    q, qd = start_state(B)
    q = np.array(q)
    if full:
        q[:, tjn.KNUCKLE["ur5right"]] = 0.5
    osc.upload_q(q, qd, slot=slot)
    osc.set_targets(start_targets(B, osc.layout.ndev), slot=slot)
    if not full:
        return q, qd
    osc.set_sensordata(np.zeros((B, 18)), slot=slot)
    osc.set_pushes([dict(dev=0, window=(1, 5))], tp.wrenches(np.random.default_rng(21), B, 1), slot=slot)
    osc.set_joints(tjn.scene(osc.layout, drive=None), slot=slot)      # (stops and couplings; no drive: the stream slot of test c has no grip to feed one)
    ee = tal.ee_start(q, np.array(qd), "k13")
    objs = ob.ObjectSet(radius=[0.05, 0.05], grippers=[ob.Gripper(dev=0, joint=tjn.KNUCKLE["ur5right"], q_close=0.3, q_open=0.15)])
    pose0 = np.stack([ee[:, 0], ee[:, 1] + np.array([0.0, 0.0, 1.0, 0, 0, 0, 0])], axis=1)
    osc.set_objects(objs, pose0, slot=slot)
    osc.set_object_loads(ol.ObjectLoads(mass=[0.4, 0.0]), slot=slot)
    return q, qd


def run(cfg, B, dtype, net):
    """The run tests a, b and c share: slot 0 under the policy, T x rollout_logged(1) with the state downloaded around every tick; then
    slot 1 from the same start under a per-robot stream of the policy's clamped outputs."""
    key = (cfg, B, np.dtype(dtype).name, net)
    if key in _RUNS:
        return _RUNS[key]
    full = net == "deep"
    obs_names, hidden = NETS[net]
    osc = tal.make_ctx(B, dtype, n_slots=2, cfg=cfg, feed=full)
    lay, rig = osc.layout, rig_of(cfg)
    scene(osc, B, 0, full)
    n_in = policy.obs_width(policy.obs_mask(obs_names), lay.n, lay.ndev, 2 if full else 0)
    layers = layers_of(n_in, hidden, 7, seed=n_in)
    osc.set_policy(layers, obs_names, ORIGIN, rig=rig, clip=CLIP, keep_obs=True, grip_dev=0, grip_close=GRIP[0], grip_open=GRIP[1])
    first = osc.policy_state()
    assert same_bits(osc.download_targets(), start_targets(B, lay.ndev).astype(dtype))      # the setter writes no target
    ch = [c for c in CH if (c != "wrench" and c != "object_pose") or full]
    rec = dict(before=[], tgt_before=[], log=[], st=[], tgt=[], q=[], qd=[], u=[], flags=[], holder=[])
    for _ in range(T):
        rec["before"].append(osc.policy_state()["pose"]); rec["tgt_before"].append(osc.download_targets())
        r = osc.rollout_logged(1, ch)
        rec["log"].append({k: v[0] for k, v in r["log"].items()}); rec["st"].append(osc.policy_state()); rec["tgt"].append(osc.download_targets())
        rec["q"].append(r["qpos"]); rec["qd"].append(r["qvel"]); rec["u"].append(r["u"]); rec["flags"].append(r["flags_any"])
        if full:
            rec["holder"].append(osc.object_state()["holder"])
    # the same start under a stream of exactly these readings
    scene(osc, B, 1, full)
    rd = np.stack([policy.clamp(s["out"], CLIP) for s in rec["st"]], axis=1)      # [B, T, 6]
    osc.set_teleop_stream(rd if B > 1 else rd[0], ORIGIN, rig=rig, slot=1)
    stream = dict(pose=[], tgt=[], q=[], qd=[], u=[])
    for _ in range(T):
        r = osc.rollout(1, slot=1)
        stream["pose"].append(osc.teleop_state(1)["pose"]); stream["tgt"].append(osc.download_targets(1))
        stream["q"].append(r["qpos"]); stream["qd"].append(r["qvel"]); stream["u"].append(r["u"])
    osc.close()
    _RUNS[key] = dict(rec=rec, stream=stream, layers=layers, mask=policy.obs_mask(obs_names), first=first, rig=rig, full=full, readings=rd)
    return _RUNS[key]


CASES = [("k13", 70, F64, "one"), ("r6", 70, F32, "odd"), ("k13", 1, F64, "odd"), ("k13", 70, F32, "deep"), ("k13", 70, F64, "deep")]


# ---- a. the kernel against the mirror, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype,net", CASES)
def test_the_networks_output_equals_the_mirror_bit_for_bit(cfg, B, dtype, net):
    """out == policy.mlp(obs) on every robot and tick by uint32 view; the setter left pose = origin, out = 0, grip = 0, tick = 0.
    Observed on an MI355X: equal on every output of every case (the MFMA form is the fmaf chain; no per-lane fallback was built)."""
    rn = run(cfg, B, dtype, net)
    f = rn["first"]
    assert f["tick"] == 0 and same_bits(f["pose"], np.tile(ORIGIN, (B, 1))) and not f["out"].any() and not f["grip"].any()
    obs = np.array([s["obs"] for s in rn["rec"]["st"]])
    out = np.array([s["out"] for s in rn["rec"]["st"]])
    want = order_shows(obs, rn["layers"])
    assert obs.dtype == F32 and out.dtype == F32 and out.shape == (T, B, 7)
    bad = np.argwhere(bits(out) != bits(want))
    assert bad.size == 0, (f"{len(bad)} of {out.size} outputs differ; first (tick, robot, output) = {tuple(bad[0])}: device "
                           f"{float(out[tuple(bad[0])]).hex()}, mirror {float(want[tuple(bad[0])]).hex()}")
    assert [s["tick"] for s in rn["rec"]["st"]] == list(range(1, T + 1))
    assert np.isfinite(out).all() and not np.any(np.array(rn["rec"]["flags"]) & _lib.FLAG_NONFINITE)


# ---- b. the observation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype,net", CASES)
def test_the_kept_observation_is_the_ticks_log_and_the_plate_before_it(cfg, B, dtype, net):
    rn = run(cfg, B, dtype, net)
    rec = rn["rec"]
    for t in range(T):
        ch = dict(rec["log"][t], targets=rec["tgt_before"][t])
        if t:
            assert np.array_equal(rec["tgt_before"][t].astype(F64), rec["log"][t - 1]["targets"].astype(F64))
        want = policy.observe(rn["mask"], ch, rec["before"][t])
        got = rec["st"][t]["obs"]
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (t, np.argwhere(bits(got) != bits(want))[:4])
    if rn["full"]:      # the scene acted: the plug rides in the hand from tick 0, the push shows in the wrench, the objects' poses moved
        assert all((h[:, 0] == 0).all() and (h[:, 1] == -1).all() for h in rec["holder"])
        w = np.array([lg["wrench"] for lg in rec["log"]])
        assert not w[0].any() and w[2][:, 0].any()
        assert not np.array_equal(rec["log"][0]["object_pose"][:, 0], rec["log"][T - 1]["object_pose"][:, 0])


# ---- c. the policy against the stream -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype,net", CASES)
def test_a_stream_of_the_policys_outputs_steps_bit_for_bit_alike_and_both_follow_policy_tick(cfg, B, dtype, net):
    rn = run(cfg, B, dtype, net)
    rec, st = rn["rec"], rn["stream"]
    out = np.array([x["out"] for x in rec["st"]])
    assert np.abs(rn["readings"]).max() == CLIP and (np.abs(out[:, :, :6]) > CLIP).any()      # the clamp acted, and out is what the network gave
    for t in range(T):
        assert same_bits(rec["st"][t]["pose"], st["pose"][t]) and same_bits(rec["tgt"][t], st["tgt"][t]), t
        assert same_bits(rec["q"][t], st["q"][t]) and same_bits(rec["qd"][t], st["qd"][t]) and same_bits(rec["u"][t], st["u"][t]), t
    # pose and targets against policy_tick on the kept observation
    ndev = len(rn["rig"])
    cur = start_targets(B, ndev)
    pose = np.tile(ORIGIN, (B, 1))
    worst = 0.0
    for t in range(T):
        p0, tg0, out0, g0 = policy.policy_tick(pose[0], rec["st"][t]["obs"][0], rn["layers"], rn["rig"], clip=CLIP, grip=GRIP)
        outs = policy.mlp(rec["st"][t]["obs"], rn["layers"])      # (the fleet's outputs in one call; policy_tick is this per robot)
        for b in range(B):
            pose[b], tg = teleop.stream_step(pose[b], policy.clamp(outs[b], CLIP), rn["rig"])
            cur[b] = np.where(np.isnan(tg), cur[b], tg)
        assert same_bits(p0, pose[0]) and np.array_equal(bits(out0), bits(outs[0])) and g0 == rec["st"][t]["grip"][0]
        assert np.array_equal(rec["st"][t]["grip"], np.where(outs[:, 6] > 0, GRIP[0], GRIP[1]))
        dev = rec["st"][t]["pose"]
        assert same_bits(dev[:, :3], pose[:, :3])
        worst = max(worst, angle_diff(dev[:, 3:], pose[:, 3:]).max())
        if dtype == F64:
            worst = max(worst, np.abs(rec["tgt"][t] - cur).max())
        else:
            assert (np.abs(rec["tgt"][t].astype(F64) - cur.astype(F32).astype(F64)) <= np.spacing(np.abs(cur.astype(F32))).astype(F64)).all()
    print(f"{cfg} {net} B={B}: device vs policy_tick over {T} ticks: max diff {worst:.3g}")
    assert worst <= BOUND, worst


# ---- d. pieces add up; a narrower rollout ---------------------------------------------------------------------------------------------------
def small(osc, B, slot=0, n_out=6, clip=CLIP, keep_obs=False, seed=3, **kw):
    """The "odd" policy on slot `slot` from the start state -> its layers"""
    scene(osc, B, slot, False)
    layers = layers_of(31, (20,), n_out, seed)
    osc.set_policy(layers, ("qpos", "plate"), ORIGIN, rig=rig_of("k13"), clip=clip, keep_obs=keep_obs, slot=slot, **kw)
    return layers


def state_of(osc, out, slot=0):
    st = osc.policy_state(slot)
    return [out["qpos"], out["qvel"], out["u"], st["pose"], st["out"], st["grip"], osc.download_targets(slot)]


@pytest.mark.parametrize("dtype", [F64, F32])
def test_pieces_of_a_rollout_add_up_and_a_narrower_rollout_skips_the_rest(dtype):
    B = 70
    res = []
    for pieces in ((8,), (5, 3)):
        osc = tal.make_ctx(B, dtype)
        small(osc, B)
        for p in pieces:
            out = osc.rollout(p)
        assert osc.policy_state()["tick"] == 8
        res.append(state_of(osc, out))
        osc.close()
    assert all(same_bits(a, b) for a, b in zip(*res))
    osc = tal.make_ctx(B, dtype)
    small(osc, B)
    assert osc.lib.irlosc_rollout_from_q(osc._h, 0, 64, 2, 0, None, None, None) == 0
    st, tg = osc.policy_state(), osc.download_targets()
    osc.close()
    assert same_bits(st["pose"][64:], np.tile(ORIGIN, (6, 1))) and not st["out"][64:].any() and st["out"][:64].all()
    assert same_bits(tg[64:], start_targets(B, 3)[64:].astype(dtype)) and not np.array_equal(tg[:64], start_targets(B, 3)[:64].astype(dtype))


# ---- e. zero weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0.25, 0.0])
def test_zero_weights_reproduce_a_constant_stream_of_the_clamped_bias(clip):
    B = 70
    b = np.array([0.5, -0.75, 0.125, -0.25, 0.3, -1.5], dtype=F32)
    osc = tal.make_ctx(B, F64, n_slots=2)
    for slot in (0, 1):
        scene(osc, B, slot, False)
    osc.set_policy([(np.zeros((6, 31), F32), b)], ("qpos", "plate"), ORIGIN, clip=clip, slot=0)
    r = b.astype(F64) if clip == 0.0 else np.clip(b, F32(-clip), F32(clip)).astype(F64)
    assert (np.abs(r).max() == clip) if clip else np.array_equal(r, b.astype(F64))
    osc.set_teleop_stream(np.tile(r, (T, 1)), ORIGIN, slot=1)
    a, s = osc.rollout(T, slot=0), osc.rollout(T, slot=1)
    assert all(same_bits(a[k], s[k]) for k in ("qpos", "qvel", "u", "flags_any"))
    assert same_bits(osc.policy_state(0)["pose"], osc.teleop_state(1)["pose"]) and same_bits(osc.download_targets(0), osc.download_targets(1))
    assert np.array_equal(bits(osc.policy_state(0)["out"]), bits(np.tile(b, (B, 1))))      # out is the network's, before the clamp
    osc.close()


# ---- f. grip -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grip_dev", [0, 1])
def test_the_seventh_output_drives_the_action_rows_of_grip_dev(grip_dev):
    B = 70
    osc = tal.make_ctx(B, F64)
    rows = tjn.scene(osc.layout)
    drives = {r["dev"]: i for i, r in enumerate(rows) if r["kind"] == "drive"}
    assert set(drives) == {"ur5right", "ur5left"}
    scene(osc, B, 0, False)
    W, b = layers_of(31, (), 7, 3)[0]
    W[6], b[6] = 0.0, 0.0
    W[6, 25] = 8.0                                  # output 6 = 8 x the plate's x, which the origins spread over both signs
    og = np.tile(ORIGIN, (B, 1))
    og[:, 0] = (np.arange(B) - 34.5) / 100.0
    osc.set_policy([(W, b)], ("qpos", "plate"), og, rig=rig_of("k13"), clip=CLIP, grip_dev=grip_dev, grip_close=GRIP[0], grip_open=GRIP[1])
    osc.set_joints(rows)
    osc.rollout(3)
    st, js = osc.policy_state(), osc.joint_state()
    osc.close()
    closed = st["out"][:, 6] > 0
    assert closed.any() and (~closed).any()
    want = np.where(closed, GRIP[0], GRIP[1])
    mine, other = (drives["ur5right"], drives["ur5left"]) if grip_dev == 0 else (drives["ur5left"], drives["ur5right"])
    assert np.array_equal(st["grip"], want) and np.array_equal(js["ctrl"][:, mine], want) and not js["ctrl"][:, other].any()


# ---- g. episodes -------------------------------------------------------------------------------------------------------------------------------
def test_every_episode_of_a_policy_slot_is_a_fresh_rollout_and_a_reset_puts_the_plate_back():
    B, L = 70, 3
    q, qd = start_state(B)
    rng = np.random.default_rng(9)
    starts = np.stack([np.array(q), np.array(q) + rng.uniform(-0.05, 0.05, q.shape) * (np.array(q) != 0)], axis=1)      # [B, 2, n]
    og = np.tile(ORIGIN, (B, 1)) + rng.uniform(-0.05, 0.05, (B, 6)) * np.array([1, 1, 1, 0, 0, 0])
    ch = ("qpos", "qvel", "targets", "u")
    osc = tal.make_ctx(B, F64, n_slots=2)
    scene(osc, B, 0, False)
    layers = layers_of(31, (20,), 7, 3)
    kw = dict(rig=rig_of("k13"), clip=CLIP, grip_close=GRIP[0], grip_open=GRIP[1])
    osc.set_policy(layers, ("qpos", "plate"), og, **kw)
    osc.set_episodes(starts, max_ticks=L)
    run3 = osc.rollout_logged(L, ch)
    st = osc.policy_state()
    assert same_bits(st["pose"], og) and not st["out"].any() and not st["grip"].any() and st["tick"] == L      # the reset of tick L - 1
    assert same_bits(run3["qpos"], starts[:, 1])
    run6 = osc.rollout_logged(L, ch)
    es = osc.episode_state()
    assert (es["count"] == 2).all() and (es["records"][:, :2, 1] == L).all() and (es["records"][:, :2, 2] == _lib.EPISODE_TIMEOUT).all()
    for e, got in enumerate((run3, run6)):
        osc.upload_q(starts[:, e], np.zeros_like(q), slot=1)
        osc.set_targets(start_targets(B, 3), slot=1)
        osc.set_policy(layers, ("qpos", "plate"), og, slot=1, **kw)
        fresh = osc.rollout_logged(L, ch, slot=1)
        for c in ch:
            assert same_bits(got["log"][c], fresh["log"][c]), (e, c)
    osc.close()


# ---- h. a robot that holds a NaN ---------------------------------------------------------------------------------------------------------------
def test_a_robot_with_a_nan_coordinate_keeps_its_state_and_leaves_its_neighbours_alone():
    B, sick = 70, 3
    q, qd = start_state(B)
    res = []
    for nan in (False, True):
        qq = np.array(q)
        if nan:
            qq[sick, 2] = np.nan
        osc = tal.make_ctx(B, F64)
        small(osc, B, n_out=7, grip_close=GRIP[0], grip_open=GRIP[1])
        osc.upload_q(qq, qd)
        out = osc.rollout(T)
        res.append((out, osc.policy_state(), osc.download_targets()))
        osc.close()
    (oa, sa, ta), (ob_, sb, tb) = res
    others = np.arange(B) != sick
    assert ob_["flags_any"][sick] & _lib.FLAG_NONFINITE and not np.any(oa["flags_any"] & _lib.FLAG_NONFINITE)
    assert same_bits(sb["pose"][sick], ORIGIN) and same_bits(tb[sick], start_targets(B, 3)[sick]) and sb["grip"][sick] == 0 and not sb["out"][sick].any()
    for x, y in ((oa["qpos"], ob_["qpos"]), (oa["qvel"], ob_["qvel"]), (oa["u"], ob_["u"]), (sa["pose"], sb["pose"]), (sa["out"], sb["out"]),
                 (sa["grip"], sb["grip"]), (ta, tb)):
        assert same_bits(x[others], y[others])
    assert sa["grip"][sick] != 0


# ---- i. state rules ----------------------------------------------------------------------------------------------------------------------------
def test_state_rules():
    B = 70
    lay, rig = synth.make_layout("k13"), rig_of("k13")
    q, qd = start_state(B)
    tgt0 = start_targets(B, 3)
    layers = layers_of(31, (20,), 7, 3)
    w = policy.weights(layers)
    og = np.ascontiguousarray(ORIGIN[None])
    osc = tts.make_ctx(B, bare=True)
    lib, h = osc.lib, osc._h
    g = synth.make_batch("k13", 1, seed=0)[1]

    def desc(layers=layers, obs=("qpos", "plate"), **over):
        d = policy.to_struct(layers, obs, rig, 1, clip=CLIP, grip_dev=0, grip_close=GRIP[0], grip_open=GRIP[1])
        for key, v in over.items():
            if isinstance(v, tuple):
                k, i, x = v
                if i is None:
                    getattr(d, key)[k] = x
                else:
                    getattr(d, key)[k][i] = x
            else:
                setattr(d, key, v)
        return d

    def set_po(d=None, ww=w, o=og, n=B, slot=0, **over):
        return lib.irlosc_set_policy(h, slot, n, C.byref(desc(**over) if d is None else d), _lib.ptr(ww), _lib.ptr(o))

    def state_rc(n=B):
        return lib.irlosc_download_policy_state(h, 0, n, None, None, None, None, None)

    # IRLOSC_ERR_STATE: before the model, before the targets, targets for fewer robots; the download without a policy
    assert set_po() == ERR_STATE and "irlosc_set_model" in lib.irlosc_last_error(h).decode()
    osc.set_gains(g["kp"], g["kv"], g["ko"], g["k"], g["d"], g["max_vel"], g["null_kv"])
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    osc.set_plant(tts.DT, tts.DAMPING)
    osc.upload_q(q, qd)
    assert set_po() == ERR_STATE and "irlosc_set_targets" in lib.irlosc_last_error(h).decode()
    assert lib.irlosc_set_targets(h, 0, B - 1, _lib.ptr(np.ascontiguousarray(tgt0[:B - 1])), None) == 0
    assert set_po() == ERR_STATE and state_rc() == ERR_STATE
    osc.set_targets(tgt0)
    assert set_po(obs=("qpos", "object_pose")) == ERR_STATE and "irlosc_set_objects" in lib.irlosc_last_error(h).decode()
    # a stream is in force; every refused policy leaves it whole
    rd = tts.readings_of(tts.SEED)
    osc.set_teleop_stream(rd, ORIGIN, rig=rig)
    osc.rollout(2)
    nan_w, nan_og = w.copy(), og.copy()
    nan_w[-1] = np.nan
    nan_og[0, 2] = np.inf
    wide = layers_of(31, (129,), 7, 3)
    bad = [dict(obs=0), dict(obs=128 | 1), dict(n_layers=0), dict(n_layers=5), dict(width=(0, None, 0)), dict(width=(0, None, 129)),
           dict(width=(1, None, 4)), dict(n_out=5), dict(n_out=8), dict(keep_obs=2), dict(reserved=1), dict(clip=-0.5), dict(clip=np.nan),
           dict(clip=np.inf), dict(nb_origin=2), dict(nb_origin=0), dict(grip_dev=3), dict(grip_dev=-1), dict(grip_close=0.0), dict(grip_open=np.nan),
           dict(increment=np.nan), dict(kind=(1, None, 3)), dict(kind=(3, None, teleop.RIGID)), dict(off_xyz=(0, 1, np.nan)),
           dict(off_quat=(1, 3, 0.5)), dict(heading_offset=(2, None, np.inf)),
           dict(obs=("qpos", "qvel", "ee_pose", "targets", "wrench", "plate"), layers=layers_of(116, (), 7, 1))]      # (fine by itself ...)
    assert set_po(ww=policy.weights(bad[-1]["layers"]), **bad.pop()) == 0 and state_rc() == 0      # ... n_in = 116 is in range
    osc.set_teleop_stream(rd, ORIGIN, rig=rig)
    osc.rollout(2)
    for over in bad:
        assert set_po(**over) == ERR_ARG, (over, lib.irlosc_last_error(h).decode())
    none = policy.to_struct(layers, ("qpos", "plate"), [teleop.follower()] * 3)
    assert set_po(d=none) == ERR_ARG                                                                # all NONE
    assert set_po(ww=nan_w) == ERR_ARG and set_po(o=nan_og) == ERR_ARG and set_po(ww=None) == ERR_ARG and set_po(o=None) == ERR_ARG
    assert set_po(n=0) == ERR_ARG and set_po(slot=5) == ERR_ARG and set_po(n=B + 1) == ERR_ARG
    assert state_rc() == ERR_STATE
    osc.rollout(1)
    st = osc.teleop_state()
    poses, _ = tts.mirror(ORIGIN, rd, rig, tgt0, B)
    assert st["tick"] == 3 and same_bits(st["pose"][:, :3], poses[2][:, :3])                        # the stream went on, whole
    # a policy replaces a stream; a NULL policy description ends it and nothing else; other programs replace it
    assert set_po() == 0 and state_rc() == 0 and lib.irlosc_download_teleop_state(h, 0, B, None, None) == ERR_STATE
    assert lib.irlosc_download_policy_state(h, 0, B, None, None, None, _lib.ptr(np.empty((B, 31), F32)), None) == ERR_STATE      # keep_obs == 0
    assert same_bits(osc.download_targets(), osc.download_targets())
    assert set_po(n=B - 6) == 0
    assert lib.irlosc_rollout_from_q(h, 0, B, 1, 0, None, None, None) == ERR_STATE and "policy" in lib.irlosc_last_error(h).decode()
    assert state_rc() == ERR_STATE and state_rc(B - 6) == 0
    assert set_po() == 0
    osc.rollout(2)
    held = osc.download_targets()
    assert lib.irlosc_set_teleop_stream(h, 0, B, None, None, None) == 0 and state_rc() == 0         # a NULL stream description leaves it alone
    assert lib.irlosc_set_policy(h, 0, B, None, None, None) == 0 and state_rc() == ERR_STATE
    assert same_bits(osc.download_targets(), held)
    assert set_po() == 0
    osc.set_waypoints([np.array([[0.1, 0.4, 0.5], [0.2, 0.4, 0.5]]), None, None], 0.01)
    assert state_rc() == ERR_STATE and lib.irlosc_download_waypoint_state(h, 0, B, None, None, None) == 0
    assert lib.irlosc_set_policy(h, 0, B, None, None, None) == 0 and lib.irlosc_download_waypoint_state(h, 0, B, None, None, None) == 0
    assert set_po() == 0 and lib.irlosc_download_waypoint_state(h, 0, B, None, None, None) == ERR_STATE
    osc.set_targets(tgt0)
    assert state_rc() == ERR_STATE
    # episodes live next to a policy (and end with it); pushes next to episodes stay refused
    assert set_po() == 0
    osc.set_episodes(np.array(q)[:1], max_ticks=2)
    assert osc.episode_state()["running"] == B
    assert lib.irlosc_set_policy(h, 0, B, None, None, None) == 0
    assert lib.irlosc_download_episode_state(h, 0, B, None, None, None, None, None, None) == ERR_STATE
    assert set_po() == 0
    osc.set_model(RigidBodyModel.load("dual_ur5"))
    assert state_rc() == ERR_STATE
    osc.close()


def test_a_slot_whose_policy_was_cleared_rolls_out_like_one_that_never_had_one():
    B = 70
    osc = tal.make_ctx(B, F64, n_slots=2)
    small(osc, B)
    mid = osc.rollout(3, slot=0)
    osc.clear_policy(slot=0)
    osc.upload_q(mid["qpos"], mid["qvel"], slot=1)
    osc.set_targets(osc.download_targets(0), slot=1)
    a, b = osc.rollout(5, slot=0), osc.rollout(5, slot=1)
    assert all(same_bits(a[k], b[k]) for k in ("qpos", "qvel", "u", "flags_any"))
    assert same_bits(osc.download_targets(0), osc.download_targets(1))
    osc.close()
