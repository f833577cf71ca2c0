"""The Gaussian head of a policy, the host side (no GPU): the ABI (struct irlosc_policy_noise, the three exports), action_motion.normal4
against normal3 and against the standard normal's moments, policy.sample against torch.distributions.Normal, its std == 0 selection, and
the log layout with the two policy channels (irlosc_log_layout_policy is context-free) against rollout_log.layout.

BOUNDS.  The moments of N draws of a standard normal: a column mean has standard deviation 1 / sqrt(N), a column variance sqrt(2 / N), a
correlation of two independent columns 1 / sqrt(N); each is held to 4.5 of those (136 figures: a 4.5 sigma miss among them has probability
1e-3 for an ideal generator, and the draws are fixed, so the test does not flicker).  logp against torch in float64: 1e-12 absolute, a
hundred times the 7.1e-15 observed at |logp| <= 8.5 -- a sum of at most 7 + 7 rounded terms of that size."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from irl_control_amd import _lib, action_motion as am, policy, rollout_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ("irlosc_set_policy_noise", "irlosc_download_policy_noise_state", "irlosc_log_layout_policy")
F32 = np.float32


def header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_exports_and_the_struct_is_48_bytes():
    hdr = header()
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), name
        assert re.search(r"IRLOSC_API int %s\(" % name, hdr), name
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 3 and re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", hdr)
    P = _lib.PolicyNoise
    assert C.sizeof(P) == 48
    assert {f: getattr(P, f).offset for f, _ in P._fields_} == dict(seed=0, n_std=8, reserved=12, std=16)
    body = re.search(r"typedef struct irlosc_policy_noise \{(.*?)\} irlosc_policy_noise;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(uint64_t|int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body) == [("uint64_t", "seed", ""), ("int32_t", "n_std", ""),
                                                                                   ("int32_t", "reserved", ""), ("float", "std", "8")]
    for name, bit in (("POLICY_OUT", 1024), ("POLICY_SAMPLE", 2048)):
        m = re.search(r"#define\s+IRLOSC_LOG_%s\s+(\d+)u" % name, hdr)
        assert m and int(m.group(1)) == bit == getattr(_lib, "LOG_" + name) == rollout_log.mask(name.lower())
    assert rollout_log.CHANNELS == ("qpos", "qvel", "ee_pose", "targets", "wrench", "u", "flags", "wall_force", "joint_tau")


# ---- normal4 --------------------------------------------------------------------------------------------------------------------------------
def test_normal4_on_stream_0_holds_normal3_and_stream_1_is_another_block():
    robot = np.arange(4096, dtype=np.uint32)[:, None]
    draw = np.array([0, 1, 77, 2 ** 32 - 1], dtype=np.uint32)[None, :]
    for seed, blk in ((0, 0), (0x123456789ABCDEF0, 3), (2 ** 64 - 1, 11)):
        z3 = am.normal3(seed, robot, draw, blk)
        z0 = am.normal4(seed, robot, draw, blk, 0)
        z1 = am.normal4(seed, robot, draw, blk, 1)
        assert z0.shape == (4096, 4, 4) and np.array_equal(u64(z0[..., :3]), u64(z3))
        assert (u64(z0) != u64(z1)).all()           # every word of the other stream differs
        assert np.isfinite(z0).all() and np.abs(z0).max() <= 6.76


def test_normal4_is_standard_normal():
    N = 200_000
    robot = np.arange(N, dtype=np.uint32)
    cols = np.concatenate([am.normal4(5, robot, d, blk, 1) for d in (0, 1) for blk in (0, 1)], axis=1)      # [N, 16]
    assert cols.shape == (N, 16)
    mean, var = cols.mean(axis=0), cols.var(axis=0)
    corr = np.corrcoef(cols, rowvar=False)
    off = np.abs(corr - np.eye(16)).max()
    print(f"normal4, N = {N}: worst |mean| {np.abs(mean).max():.4f} (bound {4.5 / np.sqrt(N):.4f}), worst |var - 1| {np.abs(var - 1).max():.4f} "
          f"(bound {4.5 * np.sqrt(2 / N):.4f}), worst |corr| {off:.4f} (bound {4.5 / np.sqrt(N):.4f})")
    assert np.abs(mean).max() <= 4.5 / np.sqrt(N)
    assert np.abs(var - 1.0).max() <= 4.5 * np.sqrt(2.0 / N)
    assert off <= 4.5 / np.sqrt(N)
    assert len(np.unique(u64(cols))) == cols.size   # all 3.2 M words distinct


# ---- policy.sample --------------------------------------------------------------------------------------------------------------------------
def test_sample_equals_torch_normal_log_prob():
    import torch
    rng = np.random.default_rng(3)
    B = 4096
    worst = big = 0.0
    for n_out, std in ((7, [0.3, 0.05, 1.5, 0.2, 0.7, 0.01, 2.0]), (6, [0.5, 0.0, 0.25, 1.0, 0.0, 0.125]), (7, [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.4])):
        std = np.array(std, dtype=F32)
        out = rng.standard_normal((B, n_out)).astype(F32)
        const = policy.logp_const(std)
        act, logp, eps = policy.sample(out, std, 11, np.arange(B), 9, const)
        on = std > 0
        m, s, e = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)) for v in (out[:, on], np.broadcast_to(std[on], (B, on.sum())), eps[:, on]))
        want = torch.distributions.Normal(m, s).log_prob(m + s * e).sum(-1).numpy()
        worst, big = max(worst, np.abs(logp - want).max()), max(big, np.abs(want).max())
        assert act.dtype == F32 and logp.dtype == np.float64 and eps.shape == (B, n_out)
        assert np.array_equal(act[:, on].view(np.uint32), (out[:, on].astype(np.float64) + std[on].astype(np.float64) * eps[:, on]).astype(F32).view(np.uint32))
        # the density at the float32 action is another number: the rounding of the cast is visible in it
        again = torch.distributions.Normal(m, s).log_prob(torch.from_numpy(act[:, on].astype(np.float64))).sum(-1).numpy()
        assert np.abs(again - want).max() > 1e-9
    print(f"policy.sample vs torch.distributions.Normal: max |logp diff| {worst:.3g} at |logp| <= {big:.3g}")
    assert worst <= 1e-12


def test_an_output_with_std_0_keeps_the_means_bits_and_adds_nothing_to_logp():
    B = 300
    rng = np.random.default_rng(4)
    out = rng.standard_normal((B, 7)).astype(F32)
    out[::3, 2] = -0.0
    out[1::3, 2] = 0.0
    std = np.array([0.3, 0.0, 0.0, 0.2, 0.0, 0.1, 0.0], dtype=F32)
    act, logp, eps = policy.sample(out, std, 2, np.arange(B), np.arange(B) * 7, policy.logp_const(std))
    off = std == 0
    assert np.array_equal(act[:, off].view(np.uint32), out[:, off].view(np.uint32)) and np.signbit(act[::3, 2]).all() and not np.signbit(act[1::3, 2]).any()
    assert (act[:, ~off] != out[:, ~off]).all() and eps[:, off].all()      # (the deterministic outputs' eps were drawn, and not used)
    s = (eps[:, 0] * eps[:, 0] + eps[:, 3] * eps[:, 3]) + eps[:, 5] * eps[:, 5]
    want = (-0.5 * s) - ((np.log(np.float64(std[0])) + np.log(np.float64(std[3]))) + np.log(np.float64(std[5])) + 1.5 * np.log(2 * np.pi))
    assert np.abs(logp - want).max() <= 1e-12
    assert np.array_equal(u64(logp), u64((-0.5 * s) - policy.logp_const(std)))
    # policy_tick without noise= is what it was; with it the tick steers by the sampled action
    from irl_control_amd import synth, teleop
    rig = teleop.space_mouse_rig(synth.make_layout("k13"))
    layers = [((rng.standard_normal((7, 31)) / 6).astype(F32), rng.standard_normal(7).astype(F32))]
    obs, pose = rng.standard_normal(31).astype(F32), np.array([0.1, 0.4, 0.5, 0.0, 0.0, 0.0])
    plain = policy.policy_tick(pose, obs, layers, rig, clip=0.5, grip=(-1.0, 1.0))
    assert len(plain) == 4
    noisy = policy.policy_tick(pose, obs, layers, rig, clip=0.5, grip=(-1.0, 1.0), noise=dict(std=std, seed=2, robot=5, draw=3, logp_const=0.25))
    a5, l5, _ = policy.sample(plain[2], std, 2, 5, 3, 0.25)
    assert len(noisy) == 6 and np.array_equal(noisy[2].view(np.uint32), plain[2].view(np.uint32)) and np.array_equal(noisy[4].view(np.uint32), a5.view(np.uint32))
    assert noisy[5] == float(l5) and not np.array_equal(noisy[0], plain[0])
    want_pose, _ = teleop.stream_step(pose, policy.clamp(a5, 0.5), rig)
    assert np.array_equal(u64(noisy[0]), u64(want_pose))


# ---- the log layout -------------------------------------------------------------------------------------------------------------------------
def c_layout(n, ndev, nobj, n_out, sampled, channels, R):
    lib = _lib.load()
    off = np.full(12, -7, dtype=np.int64)
    words = C.c_int64(-7)
    rc = lib.irlosc_log_layout_policy(n, ndev, nobj, n_out, sampled, channels, R, _lib.ptr(off), C.addressof(words))
    return rc, off, words.value


@pytest.mark.parametrize("n,ndev,nobj", [(25, 3, 0), (25, 3, 2), (25, 1, 0)])
@pytest.mark.parametrize("n_out", [6, 7])
@pytest.mark.parametrize("R", [1, 65])
def test_the_layout_with_the_policy_channels_equals_its_numpy_mirror(n, ndev, nobj, n_out, R):
    width = [n, n, ndev * 7, ndev * 7, ndev * 6, n, 1, ndev * 3, n, nobj * 8, n_out, n_out + 1]
    every = 511 | (512 if nobj else 0) | 1024 | 2048
    for channels in (1024, 2048, 1024 | 2048, 1 | 32 | 1024 | 2048, every, ("qpos", "policy_out", "policy_sample")):
        m = rollout_log.mask(channels)
        rc, off, words = c_layout(n, ndev, nobj, n_out, 1, m, R)
        assert rc == 0
        moff, mwords = rollout_log.layout(n, ndev, channels, R, nobj, n_out, True)
        assert np.array_equal(off, moff) and words == mwords, channels
        at = 0
        for i in range(12):
            if (m >> i) & 1:
                assert off[i] == at
                at += R * width[i]
            else:
                assert off[i] == -1
        assert words == at
    assert rollout_log.names(1024 | 2048 | 1) == ("qpos", "policy_out", "policy_sample")
    assert rollout_log.shape("policy_out", n, ndev, nobj, n_out) == (n_out,) and rollout_log.shape("policy_sample", n, ndev, nobj, n_out) == (n_out + 1,)
    # without a head bit 2048 is unknown, bit 1024 stays; without a policy both are, and the first ten offsets are irlosc_log_layout_objects'
    rc, off, words = c_layout(n, ndev, nobj, n_out, 0, 1 | 1024, R)
    assert rc == 0 and np.array_equal(off, rollout_log.layout(n, ndev, 1 | 1024, R, nobj, n_out, False)[0]) and words == R * (n + n_out)
    lib = _lib.load()
    known = 511 | (512 if nobj else 0)
    rc, off, words = c_layout(n, ndev, nobj, 0, 0, known, R)
    off10, words10 = np.full(10, -7, dtype=np.int64), C.c_int64(-7)
    assert lib.irlosc_log_layout_objects(n, ndev, nobj, known, R, _lib.ptr(off10), C.addressof(words10)) == 0
    assert rc == 0 and np.array_equal(off[:10], off10) and words == words10.value and (off[10:] == -1).all()
    moff, mwords = rollout_log.layout(n, ndev, known, R, nobj)
    assert np.array_equal(moff, off10[:len(moff)]) and mwords == words


@pytest.mark.parametrize("why,args", [
    ("policy_sample without a head", (25, 3, 0, 7, 0, 2048, 4)), ("policy_sample next to known bits without a head", (25, 3, 0, 7, 0, 1 | 1024 | 2048, 4)),
    ("policy_out without a policy", (25, 3, 0, 0, 0, 1024, 4)), ("policy_sample without a policy", (25, 3, 0, 0, 0, 2048, 4)),
    ("a head without a policy", (25, 3, 0, 0, 1, 2048, 4)), ("object_pose without objects next to a policy", (25, 3, 0, 7, 1, 512, 4)),
    ("bit 12", (25, 3, 2, 7, 1, 4096, 4)), ("bit 31", (25, 3, 2, 7, 1, 1 | 1 << 31, 4)), ("channels 0", (25, 3, 0, 7, 1, 0, 4)),
    ("n_out 5", (25, 3, 0, 5, 0, 1, 4)), ("n_out 8", (25, 3, 0, 8, 1, 1, 4)), ("R 0", (25, 3, 0, 7, 1, 1024, 0))])
def test_layout_refusals(why, args):
    assert c_layout(*args)[0] == ERR_ARG, why
    n, ndev, nobj, n_out, sampled, channels, R = args
    with pytest.raises(ValueError):
        rollout_log.layout(n, ndev, channels, R, nobj, n_out, bool(sampled))


def test_the_older_layouts_still_refuse_the_new_bits_and_null_outputs_are_refused():
    lib = _lib.load()
    off, words = np.zeros(12, dtype=np.int64), C.c_int64(0)
    for bit in (512, 1024, 2048, 1 << 31):
        assert lib.irlosc_log_layout(25, 3, bit, 4, _lib.ptr(off), C.addressof(words)) == ERR_ARG
        with pytest.raises(ValueError):
            rollout_log.layout(25, 3, bit, 4)
    for bit in (1024, 2048):
        assert lib.irlosc_log_layout_objects(25, 3, 2, bit, 4, _lib.ptr(off), C.addressof(words)) == ERR_ARG
        with pytest.raises(ValueError):
            rollout_log.layout(25, 3, bit, 4, 2)
    assert lib.irlosc_log_layout_policy(25, 3, 0, 7, 1, 1024, 4, None, C.addressof(words)) == ERR_ARG
    assert lib.irlosc_log_layout_policy(25, 3, 0, 7, 1, 1024, 4, _lib.ptr(off), None) == ERR_ARG
    assert lib.irlosc_log_layout_policy(25, 3, 0, 7, 2, 1024, 4, _lib.ptr(off), C.addressof(words)) == ERR_ARG


def test_split_returns_the_policy_channels():
    n, ndev, R, S, n_out = 25, 3, 5, 3, 7
    rng = np.random.default_rng(8)
    channels = ("u", "policy_out", "policy_sample")
    off, words = rollout_log.layout(n, ndev, channels, R, 0, n_out, True)
    want = dict(u=rng.normal(size=(S, R, n)), policy_out=rng.normal(size=(S, R, n_out)).astype(F32), policy_sample=rng.normal(size=(S, R, n_out + 1)))
    buf = np.full((S, words), np.nan)
    for i, name in ((5, "u"), (10, "policy_out"), (11, "policy_sample")):
        buf[:, off[i]:off[i] + want[name][0].size] = want[name].reshape(S, -1).astype(np.float64)
    assert not np.isnan(buf).any()
    got = rollout_log.split(buf, n, ndev, channels, R, n_out=n_out, sampled=True)
    assert list(got) == list(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
