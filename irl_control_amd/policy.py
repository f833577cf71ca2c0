"""A learned policy as data: what BatchedOSC.set_policy hands to the GPU (include/irlosc.h, csrc/osc_policy.hpp), and the NumPy mirror of
the kernel's arithmetic -- bit for bit, which is the point: a network evaluated on the device per robot and tick computes the tick's
space-mouse reading, and `mlp` here computes the same 32 bits on the host.

The network is a chain of float32 fused multiply-adds in ascending input order (the f32-input MFMA of gfx950 is such a chain), so the
mirror needs an EXACT float32 fma.  NumPy has none; `fma32` builds one from float64 arithmetic.  Behind the network everything is the
teleoperation stream's (teleop.stream_step): the six outputs are the reading of the tick.
"""
import numpy as np

from . import _lib, teleop

OBS_BITS = ("qpos", "qvel", "ee_pose", "targets", "wrench", "plate", "object_pose")      # bit i of `obs`: _lib.OBS_*
OBS = {name: 1 << i for i, name in enumerate(OBS_BITS)}
F32 = np.float32


def obs_mask(channels):
    """Names of OBS_BITS (or an OR of their bits) -> the OR of their bits."""
    if isinstance(channels, (int, np.integer)):
        return int(channels)
    return int(sum({OBS[c] for c in channels}))


def obs_widths(n, ndev, nobj=0):
    """Words per robot of every channel, in bit order."""
    return (n, n, ndev * 7, ndev * 7, ndev * 6, 6, nobj * 7)


def obs_width(mask, n, ndev, nobj=0):
    """n_in of an observation with the channels of `mask`."""
    return int(sum(w for i, w in enumerate(obs_widths(n, ndev, nobj)) if mask >> i & 1))


def fma32(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, vectorised: libm's fmaf.  a, b, c: float32 (arrays broadcast).  The product of two
    float32 is exact in float64 (48 bits); TwoSum gives the float64 sum s of product and addend and its exact error e; s is then rounded
    TO ODD (where e != 0 and s's last bit is even, s moves one ulp towards the exact value), which makes the final cast to float32 round
    the exact value correctly: 53 bits >= 24 + 2.  float32(float64(a) * b + c) without that step double-rounds: for a = 0x1.00062ep-4,
    b = 0x1.3ec94ep-4, c = 1 it gives 0x1.013ed0p+0 where fmaf gives 0x1.013ed2p+0 (tests/test_policy_host.py)."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        s, e = np.broadcast_arrays(s, e)
        bits = s.copy().view(np.int64)
        fix = np.isfinite(s) & (e != 0.0) & ((bits & 1) == 0)
        away = (e > 0.0) == (s > 0.0)                     # the exact value lies farther from zero than s: the next magnitude up
        bits = np.where(fix, bits + np.where(away, 1, -1), bits)
        return bits.view(np.float64).astype(F32)


def mlp(obs, layers, descending=False):
    """The network on observations obs [..., n_in] (float32) -> out [..., n_out] float32, as the kernel computes it: per layer (W [out,
    in], b [out]) with the inner dimension padded by zeros to a multiple of 4, acc = b[j], then acc = fma32(W[j][i], x[i], acc) for i
    ascending; ReLU (acc > 0 ? acc : 0) behind every layer but the last.  `descending` runs every chain the other way round -- NOT what
    the kernel computes: the tests use it to show that their data tells the two orders apart."""
    x = np.asarray(obs, dtype=F32)
    for li, (W, b) in enumerate(layers):
        W, b = np.asarray(W, dtype=F32), np.asarray(b, dtype=F32)
        o, n = W.shape
        if x.shape[-1] != n:
            raise ValueError(f"layer {li}: expected {n} inputs, got {x.shape[-1]}")
        pad = -n % 4
        Wp = np.concatenate([W, np.zeros((o, pad), F32)], axis=1)
        xp = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), F32)], axis=-1)
        acc = np.broadcast_to(b, x.shape[:-1] + (o,)).astype(F32)
        order = range(n + pad - 1, -1, -1) if descending else range(n + pad)
        for i in order:
            acc = fma32(Wp[:, i], xp[..., i:i + 1], acc)
        x = acc if li == len(layers) - 1 else np.where(acc > 0, acc, F32(0)).astype(F32)
    return x


def clamp(out, clip):
    """The six readings of outputs out [..., n_out] as float64: clamped to [-clip, clip] in float32 where clip > 0, then widened."""
    r = np.asarray(out, dtype=F32)[..., :6]
    clip = F32(clip)
    if clip > 0:
        r = np.where(r < -clip, -clip, np.where(r > clip, clip, r)).astype(F32)
    return r.astype(np.float64)


def observe(mask, channels, plate=None):
    """The observation [B, n_in] float32 the kernel gathers on a tick: the channels of `mask` in bit order, each [B, ...] flattened per
    robot and cast to float32.  `channels`: dict with the log's names (rollout_log: qpos, qvel, ee_pose, targets, wrench, object_pose --
    of which the seven pose words per object are taken, not the holder); `plate` [B, 6]: the plate pose before the tick."""
    mask = obs_mask(mask)
    parts = []
    for i, name in enumerate(OBS_BITS):
        if not mask >> i & 1:
            continue
        a = np.asarray(plate if name == "plate" else channels[name], dtype=np.float64)
        if name == "object_pose":
            a = a[..., :7]
        parts.append(a.reshape(a.shape[0], -1).astype(F32))
    return np.concatenate(parts, axis=1)


_LN_2PI = 1.8378770664093453


def logp_const(std):
    """C of logp = -s / 2 - C for standard deviations std [n_out] (float32): the sum of ln std[c] over the noisy outputs (std[c] > 0),
    c ascending, plus (m / 2) ln 2 pi, m their number -- what irlosc_set_policy_noise computes once (to a few ulp: two libm logs)."""
    sd = np.asarray(std, dtype=F32).astype(np.float64).reshape(-1)
    c, m = 0.0, 0
    for v in sd:
        if v > 0.0:
            c, m = c + float(np.log(v)), m + 1
    return c + (0.5 * m) * _LN_2PI


def sample(out, std, seed, robot, draw, logp_const):
    """The Gaussian head of a policy (include/irlosc.h, "a stochastic policy head"; the NOISE form of csrc/osc_policy.hpp), bit for bit:
    means out [..., n_out] (float32), std [n_out] (float32; 0: that output is deterministic), robot and draw [...] (uint32: the robot's
    index and its count of draws at the start of the tick), logp_const: C (logp_const(std), or the library's) ->
    (act [..., n_out] float32, logp [...] float64, eps [..., n_out] float64).  eps[c] = z[c & 3] of action_motion.normal4(seed, robot,
    draw, c >> 2, stream 1); act[c] = float32(float64(out[c]) + float64(std[c]) * eps[c]) where std[c] > 0, else out[c] itself; logp =
    (-0.5 * s) - C with s the sum of eps[c]^2 over the noisy outputs, c ascending.  eps of a deterministic output is returned as drawn."""
    from .action_motion import normal4
    out = np.asarray(out, dtype=F32)
    sd = np.asarray(std, dtype=F32).reshape(-1)
    n_out = out.shape[-1]
    if len(sd) < n_out:
        raise ValueError(f"std: expected {n_out} entries, got {len(sd)}")
    robot, draw = np.broadcast_arrays(np.asarray(robot, dtype=np.uint32), np.asarray(draw, dtype=np.uint32))
    robot, draw = np.broadcast_to(robot, out.shape[:-1]), np.broadcast_to(draw, out.shape[:-1])
    z = np.concatenate([normal4(seed, robot, draw, blk, 1) for blk in range((n_out + 3) // 4)], axis=-1)      # [..., 4 blocks]
    eps = z[..., :n_out]
    act = out.copy()
    s = np.zeros(out.shape[:-1])
    with np.errstate(over="ignore"):
        for c in range(n_out):
            if sd[c] > 0:
                act[..., c] = (out[..., c].astype(np.float64) + np.float64(sd[c]) * eps[..., c]).astype(F32)
                s = s + eps[..., c] * eps[..., c]
    return act, (-0.5 * s) - np.float64(logp_const), eps


def policy_tick(pose, obs, layers, rig, inc=teleop.INCREMENT, clip=0.0, grip=None, noise=None):
    """One tick of one robot: pose [6] and its observation [n_in] -> (new pose [6], targets [ndev, 7] with NaN where the tick writes
    nothing, out [n_out] float32, grip force or None).  `grip`: (close, open) of a network with a seventh output.
    `noise`: dict(std, seed, robot, draw, logp_const) of a Gaussian head (sample's arguments): the tick then steers and grips by the
    sampled action, and -> (new pose, targets, out, grip, act [n_out] float32, logp)."""
    out = mlp(np.asarray(obs, dtype=F32)[None], layers)[0]
    if noise is None:
        new, tgt = teleop.stream_step(pose, clamp(out, clip), rig, inc)
        g = None if grip is None or len(out) < 7 else float(grip[0] if out[6] > 0 else grip[1])
        return new, tgt, out, g
    act, logp, _ = sample(out, noise["std"], noise["seed"], noise["robot"], noise["draw"], noise["logp_const"])
    new, tgt = teleop.stream_step(pose, clamp(act, clip), rig, inc)
    g = None if grip is None or len(out) < 7 else float(grip[0] if act[6] > 0 else grip[1])
    return new, tgt, out, g, act, float(logp)


def weights(layers):
    """layers -> the one float32 array irlosc_set_policy takes: per layer W [out][in] row-major, then b [out]."""
    return np.concatenate([np.concatenate([np.asarray(W, dtype=F32).reshape(-1), np.asarray(b, dtype=F32).reshape(-1)]) for W, b in layers])


def to_struct(layers, obs, rig, nb_origin=1, increment=teleop.INCREMENT, clip=0.0, keep_obs=False, grip_dev=0, grip_close=0.0, grip_open=0.0):
    """-> _lib.Policy of a network (`layers`: [(W, b), ...]), its observation mask and a rig (one teleop.follower per device)."""
    if not 1 <= len(layers) <= _lib.POLICY_MAX_LAYERS:
        raise ValueError(f"a policy has 1 to {_lib.POLICY_MAX_LAYERS} layers, got {len(layers)}")
    if len(rig) > _lib.MAX_DEV:
        raise ValueError(f"a rig holds at most {_lib.MAX_DEV} followers, got {len(rig)}")
    d = _lib.Policy()
    d.obs, d.n_layers, d.n_out = obs_mask(obs), len(layers), int(np.shape(layers[-1][0])[0])
    for l, (W, _) in enumerate(layers[:-1]):
        d.width[l] = int(np.shape(W)[0])
    d.keep_obs, d.grip_dev, d.nb_origin, d.clip = int(bool(keep_obs)), int(grip_dev), int(nb_origin), float(clip)
    d.grip_close, d.grip_open = float(grip_close), float(grip_open)
    s = teleop.to_struct(rig, 1, 1, nb_origin, increment)
    d.increment = s.increment
    for k in range(_lib.MAX_DEV):
        d.kind[k], d.heading_offset[k] = s.kind[k], s.heading_offset[k]
        for i in range(3):
            d.off_xyz[k][i] = s.off_xyz[k][i]
        for i in range(4):
            d.off_quat[k][i] = s.off_quat[k][i]
    return d


def from_torch(module):
    """A torch.nn.Sequential of Linear / ReLU (Linear first and last, a ReLU between every two) -> layers [(W, b), ...] as float32 arrays
    holding the module's parameters bit for bit."""
    import torch      # only here: nothing else of the package needs it
    mods = list(module)
    layers = []
    for i, m in enumerate(mods):
        want = torch.nn.Linear if i % 2 == 0 else torch.nn.ReLU
        if not isinstance(m, want) or (len(mods) % 2 == 0):
            raise ValueError("from_torch: expected Linear, ReLU, Linear, ..., Linear")
        if isinstance(m, torch.nn.Linear):
            if m.weight.dtype != torch.float32:
                raise ValueError("from_torch: float32 parameters expected")
            b = m.bias.detach().cpu().numpy() if m.bias is not None else np.zeros(m.out_features, F32)
            layers.append((m.weight.detach().cpu().numpy().copy(), np.array(b, dtype=F32)))
    return layers
