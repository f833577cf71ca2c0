"""The Gaussian head of a policy on the GPU (-m gpu): irlosc_set_policy_noise / irlosc_download_policy_noise_state -- the NOISE form of the
policy kernel (csrc/osc_policy.hpp) and the log's policy_out / policy_sample channels.  The sampled action and its log-probability
against their NumPy mirror (policy.sample) BIT FOR BIT, the noisy policy against a stream that replays its actions, robots independent of
their neighbours, in pieces, with the head ended, next to episodes, in the log, next to a robot that holds a NaN, and the state rules.

Shapes are tests/test_policy.py's (its nets, scene, start states and helpers are used as they are): B = 70 (one full wave and a ragged one
of 6 robots) and B = 1; T = 6 ticks; float64 and float32 contexts; k13 (three devices) and r6 (one).  Every context here is WIDER than the
robots it runs (MAXB = 96), so the per-robot state planes have a stride that is not B.  Every std vector has one zero entry; draw0 puts
robots 0 .. 2 in front of the wrap of their draw count at 2^32."""
import ctypes as C

import numpy as np
import pytest

import test_action_list as tal
import test_policy as tpo
import test_teleop_stream as tts
from irl_control_amd import _lib, policy
from test_policy import CLIP, GRIP, T, layers_of, rig_of, scene
from test_teleop_stream import ORIGIN, bits, same_bits, start_state, start_targets

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
F64, F32 = np.float64, np.float32
MAXB = 96
SEED = 0x5EED0123456789AB
STD = np.array([0.3, 0.05, 0.0, 0.2, 0.1, 0.4, 1.0], dtype=F32)      # (output 2 deterministic; the grip's output noisy)
_RUNS = {}


def draw0_of(B):
    return ((2 ** 32 - 3 + np.arange(B, dtype=np.int64) * 1_000_003) % 2 ** 32).astype(np.uint32)


def ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def mirror(out, std, robots, draws, const, seed=SEED):
    return policy.sample(out, std, seed, robots, draws, const)


def run(cfg, B, dtype, net, n_out):
    """The run tests a and b share: slot 0 under the noisy policy, T x rollout(1) with the state downloaded behind every tick; then slot 1
    from the same start under a per-robot stream of the clamped sampled actions."""
    key = (cfg, B, np.dtype(dtype).name, net, n_out)
    if key in _RUNS:
        return _RUNS[key]
    full = net == "deep"
    obs_names, hidden = tpo.NETS[net]
    osc = tal.make_ctx(B, dtype, n_slots=2, cfg=cfg, max_batch=MAXB, feed=full)
    lay, rig = osc.layout, rig_of(cfg)
    scene(osc, B, 0, full)
    n_in = policy.obs_width(policy.obs_mask(obs_names), lay.n, lay.ndev, 2 if full else 0)
    layers = layers_of(n_in, hidden, n_out, seed=n_in)
    osc.set_policy(layers, obs_names, ORIGIN, rig=rig, clip=CLIP, grip_dev=0, grip_close=GRIP[0], grip_open=GRIP[1])
    std, d0 = STD[:n_out], draw0_of(B)
    osc.set_policy_noise(std, SEED, d0)
    first = osc.policy_noise_state()
    rec = dict(st=[], ns=[], tgt=[], q=[], qd=[], u=[], flags=[])
    for _ in range(T):
        r = osc.rollout(1)
        rec["st"].append(osc.policy_state()); rec["ns"].append(osc.policy_noise_state()); rec["tgt"].append(osc.download_targets())
        rec["q"].append(r["qpos"]); rec["qd"].append(r["qvel"]); rec["u"].append(r["u"]); rec["flags"].append(r["flags_any"])
    scene(osc, B, 1, full)
    rd = np.stack([policy.clamp(s["act"], CLIP) for s in rec["ns"]], axis=1)      # [B, T, 6]
    osc.set_teleop_stream(rd if B > 1 else rd[0], ORIGIN, rig=rig, slot=1)
    stream = dict(pose=[], tgt=[], q=[], qd=[], u=[])
    for _ in range(T):
        r = osc.rollout(1, slot=1)
        stream["pose"].append(osc.teleop_state(1)["pose"]); stream["tgt"].append(osc.download_targets(1))
        stream["q"].append(r["qpos"]); stream["qd"].append(r["qvel"]); stream["u"].append(r["u"])
    osc.close()
    _RUNS[key] = dict(rec=rec, stream=stream, first=first, std=std, d0=d0, readings=rd)
    return _RUNS[key]


CASES = [("k13", 70, F64, "odd", 7), ("r6", 70, F32, "odd", 6), ("k13", 1, F64, "odd", 7), ("k13", 70, F32, "deep", 7)]


# ---- a. the kernel against the mirror, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype,net,n_out", CASES)
def test_action_and_logp_equal_the_mirror_bit_for_bit(cfg, B, dtype, net, n_out):
    """act (uint32 view) and logp (uint64 view) of every robot on every tick == policy.sample of the tick's out with the robot's index, its
    draws at the start of the tick and the library's logp_const; draws == draw0 + ticks run (mod 2^32); logp_const within 4 ulp of
    policy.logp_const (two libm logs); the setter left act = 0, logp = 0, draws = draw0."""
    rn = run(cfg, B, dtype, net, n_out)
    f, std, d0 = rn["first"], rn["std"], rn["d0"]
    assert not f["act"].any() and not f["logp"].any() and np.array_equal(f["draws"], d0) and f["act"].shape == (B, n_out)
    const = f["logp_const"]
    assert ulps(const, policy.logp_const(std)) <= 4, (const, policy.logp_const(std))
    assert int(d0[0]) > 2 ** 32 - T and (int(d0[0]) + T) % 2 ** 32 < T      # robot 0 wraps inside the run
    robots = np.arange(B)
    for t in range(T):
        out, ns = rn["rec"]["st"][t]["out"], rn["rec"]["ns"][t]
        draws = (d0.astype(np.int64) + t) % 2 ** 32
        act, logp, eps = mirror(out, std, robots, draws, const)
        bad = np.argwhere(bits(ns["act"]) != bits(act))
        assert bad.size == 0, (f"tick {t}: {len(bad)} of {act.size} actions differ; first (robot, output) = {tuple(bad[0])}: device "
                               f"{float(ns['act'][tuple(bad[0])]).hex()}, mirror {float(act[tuple(bad[0])]).hex()}")
        bad = np.argwhere(bits(ns["logp"]) != bits(logp))
        assert bad.size == 0, f"tick {t}: {len(bad)} of {B} logp differ; first robot {bad[0][0]}: device {ns['logp'][bad[0][0]].hex()}, mirror {logp[bad[0][0]].hex()}"
        assert np.array_equal(ns["draws"], ((draws + 1) % 2 ** 32).astype(np.uint32)) and ns["logp_const"] == const
        on = std > 0
        assert (bits(ns["act"][:, on]) != bits(out[:, on])).all() and np.array_equal(bits(ns["act"][:, ~on]), bits(out[:, ~on]))
        if n_out == 7:
            assert np.array_equal(rn["rec"]["st"][t]["grip"], np.where(ns["act"][:, 6] > 0, GRIP[0], GRIP[1]))
    assert np.isfinite(np.array([s["act"] for s in rn["rec"]["ns"]])).all() and not np.any(np.array(rn["rec"]["flags"]) & _lib.FLAG_NONFINITE)
    if n_out == 7 and B > 1:      # the grip follows act, not out: the two disagree somewhere in the run
        outs, acts = (np.array([s[k][:, 6] for s in rn["rec"][w]]) for w, k in (("st", "out"), ("ns", "act")))
        assert ((outs > 0) != (acts > 0)).any()


# ---- b. the noisy policy against the stream --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,dtype,net,n_out", CASES)
def test_a_stream_of_the_clamped_sampled_actions_steps_bit_for_bit_alike(cfg, B, dtype, net, n_out):
    rn = run(cfg, B, dtype, net, n_out)
    rec, st = rn["rec"], rn["stream"]
    acts = np.array([x["act"] for x in rec["ns"]])
    assert np.abs(rn["readings"]).max() == CLIP and (np.abs(acts[:, :, :6]) > CLIP).any()      # the clamp acted on act
    if B > 1:       # a stream of the means is another one (the single robot's six readings all sit on the clamp, with or without noise)
        assert not np.array_equal(rn["readings"], np.stack([policy.clamp(s["out"], CLIP) for s in rec["st"]], axis=1))
    for t in range(T):
        assert same_bits(rec["st"][t]["pose"], st["pose"][t]) and same_bits(rec["tgt"][t], st["tgt"][t]), t
        assert same_bits(rec["q"][t], st["q"][t]) and same_bits(rec["qd"][t], st["qd"][t]) and same_bits(rec["u"][t], st["u"][t]), t


# ---- helpers of the tests below: the "odd" policy of tests/test_policy.py with a head ---------------------------------------------------------
def noisy(osc, B, slot=0, n_out=7, head=True, draw0="wrap", **kw):
    layers = tpo.small(osc, B, slot=slot, n_out=n_out, grip_close=GRIP[0], grip_open=GRIP[1], **kw)
    if head:
        osc.set_policy_noise(STD[:n_out], SEED, draw0_of(B) if isinstance(draw0, str) else draw0, slot=slot)
    return layers


def state_of(osc, out, slot=0, head=True):
    st = osc.policy_state(slot)
    ns = osc.policy_noise_state(slot) if head else dict(act=st["out"], logp=st["grip"], draws=np.zeros(1, np.uint32))
    return [out["qpos"], out["qvel"], out["u"], st["pose"], st["out"], st["grip"], osc.download_targets(slot), ns["act"], ns["logp"], ns["draws"]]


# ---- c. independence ----------------------------------------------------------------------------------------------------------------------------
def test_a_robots_draws_do_not_depend_on_its_neighbours_and_one_mean_gives_70_actions():
    B = 70
    res = []
    for nb in (B, 64):
        osc = tal.make_ctx(B, F64, max_batch=MAXB)
        noisy(osc, B)
        u, fl = np.empty((nb, 25)), np.empty(nb, np.uint32)
        assert osc.lib.irlosc_rollout_from_q(osc._h, 0, nb, T, 0, None, _lib.ptr(u), _lib.ptr(fl)) == 0
        q, qd = np.zeros((B, 25)), np.zeros((B, 25))      # (the slot holds the coordinates of the nb robots it ran)
        assert osc.lib.irlosc_download_q(osc._h, 0, nb, _lib.ptr(q), _lib.ptr(qd)) == 0
        res.append(state_of(osc, dict(qpos=q, qvel=qd, u=np.concatenate([u, np.zeros((B - nb, 25))]))))
        osc.close()
    full, part = res
    for k, (x, y) in enumerate(zip(full, part)):
        assert same_bits(x[:64], y[:64]), k
    assert not part[7][64:].any() and not part[8][64:].any() and np.array_equal(part[9][64:], draw0_of(B)[64:])      # left out: act, logp, draws stay
    # one start state and one origin for the fleet: tick 0 has one mean and 70 different actions
    q1, qd1 = start_state(1)
    osc = tal.make_ctx(B, F64, max_batch=MAXB)
    noisy(osc, B, draw0=None)
    osc.upload_q(np.tile(q1, (B, 1)), np.tile(qd1, (B, 1)))
    osc.rollout(1)
    st, ns = osc.policy_state(), osc.policy_noise_state()
    osc.close()
    assert (bits(st["out"]) == bits(st["out"][:1])).all() and (ns["draws"] == 1).all()
    for c in np.nonzero(STD > 0)[0]:
        assert len(np.unique(bits(ns["act"][:, c]))) == B, c
    assert len(np.unique(bits(ns["logp"]))) == B


# ---- d. pieces add up; a narrower rollout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_pieces_of_a_rollout_add_up_and_a_narrower_rollout_leaves_the_rest_alone(dtype):
    B = 70
    res = []
    for pieces in ((6,), (4, 2)):
        osc = tal.make_ctx(B, dtype, max_batch=MAXB)
        noisy(osc, B)
        for p in pieces:
            out = osc.rollout(p)
        res.append(state_of(osc, out))
        osc.close()
    assert all(same_bits(a, b) for a, b in zip(*res))
    assert np.array_equal(res[0][9], ((draw0_of(B).astype(np.int64) + 6) % 2 ** 32).astype(np.uint32))
    osc = tal.make_ctx(B, dtype, max_batch=MAXB)
    noisy(osc, B)
    assert osc.lib.irlosc_rollout_from_q(osc._h, 0, 30, 2, 0, None, None, None) == 0
    ns = osc.policy_noise_state()
    osc.close()
    assert not ns["act"][30:].any() and not ns["logp"][30:].any() and np.array_equal(ns["draws"][30:], draw0_of(B)[30:])
    assert ns["act"][:30].all() and ns["logp"][:30].all() and np.array_equal(ns["draws"][:30], ((draw0_of(B)[:30].astype(np.int64) + 2) % 2 ** 32).astype(np.uint32))


# ---- e. ending the head ----------------------------------------------------------------------------------------------------------------------------
def test_a_slot_whose_head_was_ended_rolls_out_like_one_that_never_had_one():
    B = 70
    osc = tal.make_ctx(B, F64, n_slots=3, max_batch=MAXB)
    noisy(osc, B, slot=0, head=False)
    noisy(osc, B, slot=1)
    osc.set_policy_noise(None, slot=1)                                          # noise == NULL: the head ends, the policy stays
    assert osc.lib.irlosc_download_policy_noise_state(osc._h, 1, B, None, None, None, None) == ERR_STATE
    assert osc.lib.irlosc_download_policy_state(osc._h, 1, B, None, None, None, None, None) == 0
    noisy(osc, B, slot=2)
    tpo.small(osc, B, slot=2, n_out=7, grip_close=GRIP[0], grip_open=GRIP[1])   # irlosc_set_policy again ends the head
    assert osc.lib.irlosc_download_policy_noise_state(osc._h, 2, B, None, None, None, None) == ERR_STATE
    never, ended, again = (state_of(osc, osc.rollout(T, slot=s), slot=s, head=False) for s in (0, 1, 2))
    osc.close()
    assert all(same_bits(a, b) for a, b in zip(never, ended)) and all(same_bits(a, b) for a, b in zip(never, again))


# ---- f. episodes -----------------------------------------------------------------------------------------------------------------------------------
def test_episodes_keep_the_draw_count_across_resets_and_a_reset_zeroes_act_and_logp():
    B, L, N = 70, 3, 7
    q, qd = start_state(B)
    ch = ("qpos", "policy_out", "policy_sample")
    osc = tal.make_ctx(B, F64, n_slots=2, max_batch=MAXB)
    for slot in (0, 1):
        noisy(osc, B, slot=slot, draw0=None)
        osc.set_episodes(np.array(q)[:, None], max_ticks=L, slot=slot)
    const = osc.policy_noise_state()["logp_const"]
    lg = osc.rollout_logged(N, ch)["log"]
    short = osc.rollout_logged(L, ch, slot=1)["log"]
    ns, st = osc.policy_noise_state(1), osc.policy_state(1)
    osc.close()
    assert not ns["act"].any() and not ns["logp"].any() and (ns["draws"] == L).all() and not st["out"].any()      # the call ended on a reset tick
    assert lg["policy_out"].dtype == F32 and lg["policy_out"].shape == (N, B, 7) and lg["policy_sample"].shape == (N, B, 8)
    for t in range(N):
        act, logp, _ = mirror(lg["policy_out"][t], STD, np.arange(B), t, const)      # draws count through the resets
        assert np.array_equal(bits(lg["policy_sample"][t, :, :7].astype(F32)), bits(act)), t
        assert np.array_equal(bits(lg["policy_sample"][t, :, 7]), bits(logp)), t
    for k in ch:
        assert same_bits(lg[k][:L], short[k])
    # episode 1 starts where episode 0 started (one start state, the plate back on the origin: the same mean) and explores afresh
    assert same_bits(lg["qpos"][L], lg["qpos"][0]) and same_bits(lg["policy_out"][L], lg["policy_out"][0])
    on = STD > 0
    assert (lg["policy_sample"][L][:, :7][:, on] != lg["policy_sample"][0][:, :7][:, on]).all()
    assert not np.array_equal(lg["qpos"][L + 1], lg["qpos"][1])


# ---- g. the log ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robots", [[0, 5, 64, 69], None])
def test_the_logs_policy_channels_equal_the_states_behind_one_tick_calls(robots):
    B = 70
    rn = run("k13", B, F64, "odd", 7)
    rec = rn["rec"]
    rows = slice(None) if robots is None else robots
    osc = tal.make_ctx(B, F64, max_batch=MAXB)
    scene(osc, B, 0, False)
    osc.set_policy(layers_of(31, (20,), 7, seed=31), tpo.NETS["odd"][0], ORIGIN, rig=rig_of("k13"), clip=CLIP, grip_dev=0, grip_close=GRIP[0], grip_open=GRIP[1])
    osc.set_policy_noise(STD, SEED, draw0_of(B))
    r = osc.rollout_logged(T, ("u", "policy_out", "policy_sample"), every=2, robots=robots)
    ns = osc.policy_noise_state()
    osc.close()
    lg = r["log"]
    assert list(r["log_ticks"]) == [0, 2, 4] and lg["policy_out"].dtype == F32
    for s, t in enumerate((0, 2, 4)):
        assert same_bits(lg["policy_out"][s], rec["st"][t]["out"][rows]), t
        assert same_bits(lg["policy_sample"][s][:, :7].astype(F32), rec["ns"][t]["act"][rows]) and same_bits(lg["policy_sample"][s][:, 7], rec["ns"][t]["logp"][rows]), t
        assert same_bits(lg["u"][s], rec["u"][t][rows]), t
    # the logged rollout is the unlogged one
    assert same_bits(r["qpos"], rec["q"][T - 1]) and same_bits(r["qvel"], rec["qd"][T - 1]) and same_bits(r["u"], rec["u"][T - 1])
    assert same_bits(ns["act"], rec["ns"][T - 1]["act"]) and same_bits(ns["logp"], rec["ns"][T - 1]["logp"])


def test_the_log_refuses_the_policy_channels_a_slot_does_not_have_and_leaves_it_untouched():
    B = 70
    osc = tal.make_ctx(B, F64, n_slots=2, max_batch=MAXB)
    lib, h = osc.lib, osc._h
    noisy(osc, B, slot=0, head=False)
    scene(osc, B, 1, False)                         # slot 1: no policy
    buf = np.zeros((1, B * 64))

    def logged(slot, channels):
        lg = _lib.Log(channels, 1, 0, 0, 0)
        return lib.irlosc_rollout_from_q_logged(h, slot, B, 1, C.byref(lg), None, _lib.ptr(buf), None, None)

    before = (osc.download_q(0), osc.download_q(1), osc.download_targets(0), osc.policy_state(0))
    assert logged(0, 2048) == ERR_ARG and logged(0, 1 | 2048) == ERR_ARG and logged(0, 1024 | 2048) == ERR_ARG      # no head
    assert logged(1, 1024) == ERR_ARG and logged(1, 2048) == ERR_ARG and logged(1, 1 | 1024) == ERR_ARG             # no policy
    assert logged(0, 4096) == ERR_ARG and logged(0, 512) == ERR_ARG and logged(0, 1 | 1 << 31) == ERR_ARG
    with pytest.raises(_lib.IrloscError):
        osc.rollout_logged(1, ("qpos", "policy_sample"))
    after = (osc.download_q(0), osc.download_q(1), osc.download_targets(0), osc.policy_state(0))
    assert all(same_bits(x, y) for a, b in zip(before[:2], after[:2]) for x, y in zip(a, b)) and same_bits(before[2], after[2])
    assert after[3]["tick"] == 0 and same_bits(before[3]["pose"], after[3]["pose"])
    assert logged(0, 1024) == 0 and osc.policy_state(0)["tick"] == 1      # policy_out needs no head
    osc.set_policy_noise(STD, SEED)
    assert logged(0, 1024 | 2048) == 0
    osc.set_policy_noise(None)
    assert logged(0, 2048) == ERR_ARG and osc.policy_state(0)["tick"] == 2
    osc.close()


# ---- h. a robot that holds a NaN ---------------------------------------------------------------------------------------------------------------------
def test_a_robot_with_a_nan_coordinate_keeps_act_and_logp_is_flagged_and_its_draws_advance():
    B, sick = 70, 3
    q, qd = start_state(B)
    res = []
    for nan in (False, True):
        qq = np.array(q)
        if nan:
            qq[sick, 2] = np.nan
        osc = tal.make_ctx(B, F64, max_batch=MAXB)
        noisy(osc, B, draw0=None)
        osc.upload_q(qq, qd)
        out = osc.rollout(T)
        res.append(state_of(osc, out) + [out["flags_any"]])
        osc.close()
    clean, ill = res
    others = np.arange(B) != sick
    assert ill[10][sick] & _lib.FLAG_NONFINITE and not np.any(clean[10] & _lib.FLAG_NONFINITE)
    assert not ill[7][sick].any() and ill[8][sick] == 0 and not ill[4][sick].any() and ill[5][sick] == 0      # act, logp, out, grip kept
    assert same_bits(ill[3][sick], ORIGIN) and same_bits(ill[6][sick], start_targets(B, 3)[sick])
    assert ill[9][sick] == T and (ill[9] == T).all()                                                       # draws count ticks
    assert clean[7][sick].any() and clean[8][sick] != 0
    for k in range(10):
        assert same_bits(clean[k][others], ill[k][others]), k


# ---- i. state rules --------------------------------------------------------------------------------------------------------------------------------
def test_state_rules():
    B = 70
    osc = tal.make_ctx(B, F64, n_slots=2, max_batch=MAXB)
    lib, h = osc.lib, osc._h

    def desc(std=STD, n_std=None, reserved=0, seed=SEED):
        d = _lib.PolicyNoise()
        d.seed, d.n_std, d.reserved = seed, len(std) if n_std is None else n_std, reserved
        for c, v in enumerate(std):
            d.std[c] = v
        return d

    def set_pn(slot=0, d0=None, **kw):
        return lib.irlosc_set_policy_noise(h, slot, C.byref(desc(**kw)), _lib.ptr(d0))

    def state_rc(n=B, slot=0):
        return lib.irlosc_download_policy_noise_state(h, slot, n, None, None, None, None)

    # no policy: IRLOSC_ERR_STATE (under a list, a stream or nothing); the NULL description is accepted and does nothing
    scene(osc, B, 0, False)
    assert set_pn() == ERR_STATE and "irlosc_set_policy" in lib.irlosc_last_error(h).decode() and state_rc() == ERR_STATE
    assert lib.irlosc_set_policy_noise(h, 0, None, None) == 0
    osc.set_teleop_stream(tts.readings_of(tts.SEED), ORIGIN, rig=rig_of("k13"))
    assert set_pn() == ERR_STATE and state_rc() == ERR_STATE
    assert set_pn(slot=5) == ERR_ARG and lib.irlosc_set_policy_noise(None, 0, None, None) == ERR_ARG
    # a policy of 60 robots with a head; every refusal leaves that head in force, whole
    layers = tpo.small(osc, B, n_out=7, grip_close=GRIP[0], grip_open=GRIP[1])
    assert lib.irlosc_set_policy(h, 0, 60, C.byref(policy.to_struct(layers, ("qpos", "plate"), rig_of("k13"), 1, clip=CLIP, grip_close=GRIP[0], grip_open=GRIP[1])),
                                 _lib.ptr(policy.weights(layers)), _lib.ptr(np.ascontiguousarray(ORIGIN[None]))) == 0
    d0 = draw0_of(60)
    assert set_pn(d0=d0) == 0 and state_rc(60) == 0 and state_rc(61) == ERR_STATE and state_rc(B) == ERR_STATE
    assert lib.irlosc_rollout_from_q(h, 0, 60, 2, 0, None, None, None) == 0
    act, logp, draws, const = np.empty((60, 7), F32), np.empty(60), np.empty(60, np.uint32), C.c_double(0)

    def held():
        assert lib.irlosc_download_policy_noise_state(h, 0, 60, _lib.ptr(act), _lib.ptr(logp), _lib.ptr(draws), C.byref(const)) == 0
        return act.copy(), logp.copy(), draws.copy(), const.value

    was = held()
    assert was[0].all() and np.array_equal(was[2], ((d0.astype(np.int64) + 2) % 2 ** 32).astype(np.uint32)) and ulps(was[3], policy.logp_const(STD)) <= 4
    bad = [dict(n_std=6), dict(std=STD[:6]), dict(n_std=8), dict(n_std=0), dict(n_std=-1), dict(reserved=1),
           dict(std=np.where(np.arange(7) == 1, -0.1, STD)), dict(std=np.where(np.arange(7) == 4, np.nan, STD)), dict(std=np.where(np.arange(7) == 6, np.inf, STD)),
           dict(std=np.zeros(7, F32)), dict(std=np.append(STD, F32(0.5)), n_std=7), dict(std=np.append(STD, F32(np.nan)), n_std=7)]
    for over in bad:
        assert set_pn(**over) == ERR_ARG, (over, lib.irlosc_last_error(h).decode())
    assert set_pn(slot=1) == ERR_STATE              # (slot 1 has no policy)
    now = held()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(was[:3], now[:3])) and was[3] == now[3]
    assert lib.irlosc_rollout_from_q(h, 0, 60, 1, 0, None, None, None) == 0
    assert np.array_equal(held()[2], ((d0.astype(np.int64) + 3) % 2 ** 32).astype(np.uint32))      # the head went on, whole
    # success replaces the head and resets its state; draw0 NULL = zeros; any download pointer may be NULL
    assert set_pn(std=np.where(np.arange(7) == 0, 0.0, STD).astype(F32), seed=1) == 0
    fresh = held()
    assert not fresh[0].any() and not fresh[1].any() and not fresh[2].any() and fresh[3] != was[3]
    assert lib.irlosc_download_policy_noise_state(h, 0, 60, None, _lib.ptr(logp), None, None) == 0
    assert lib.irlosc_download_policy_noise_state(h, 0, 0, None, None, None, C.byref(const)) == 0 and const.value == fresh[3]
    # whatever ends the policy ends the head: the NULL policy, another program, irlosc_set_targets, irlosc_set_model
    assert lib.irlosc_set_policy(h, 0, B, None, None, None) == 0 and state_rc(60) == ERR_STATE and set_pn() == ERR_STATE
    for end in (lambda: osc.set_teleop_stream(tts.readings_of(tts.SEED), ORIGIN, rig=rig_of("k13")), lambda: osc.set_targets(start_targets(B, 3)),
                lambda: osc.set_model(tal.RigidBodyModel.load("dual_ur5"))):
        noisy(osc, B)
        assert state_rc() == 0
        end()
        assert state_rc() == ERR_STATE and lib.irlosc_download_policy_state(h, 0, B, None, None, None, None, None) == ERR_STATE
    # a policy of 6 outputs takes a head of 6 and refuses one of 7
    osc.set_plant(tal.DT, tal.DAMPING)
    noisy(osc, B, n_out=6)
    assert state_rc() == 0 and set_pn() == ERR_ARG and set_pn(std=STD[:6]) == 0
    osc.close()
