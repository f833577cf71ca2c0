"""The episode log of a rollout on the host (include/irlosc.h, "the episode log"): the channel names, a NumPy mirror of
irlosc_log_layout, and split(), which turns the raw buffer of irlosc_rollout_from_q_logged into named arrays."""
import numpy as np

# channel names in bit order: bit i of irlosc_log.channels is CHANNELS[i] (IRLOSC_LOG_QPOS = 1 << 0, ...)
CHANNELS = ("qpos", "qvel", "ee_pose", "targets", "wrench", "u", "flags", "wall_force", "joint_tau")
BITS = {name: 1 << i for i, name in enumerate(CHANNELS)}
ALL = (1 << len(CHANNELS)) - 1
# ... and bit 9, IRLOSC_LOG_OBJECT_POSE, which only a slot with action objects knows (nobj > 0 below): [R, nobj, 8], the seven pose words
# and the holder as a double.  It is no part of CHANNELS / ALL: those are the channels every slot can log.
OBJECT_POSE = "object_pose"
OBJECT_POSE_BIT = 1 << len(CHANNELS)
# ... and bits 10 and 11, IRLOSC_LOG_POLICY_OUT and IRLOSC_LOG_POLICY_SAMPLE, which only a slot with a policy (n_out > 0 below) and one
# whose policy has a Gaussian head (sampled) know: [R, n_out] the network's output (the mean), [R, n_out + 1] the sampled action, then logp.
POLICY_OUT, POLICY_SAMPLE = "policy_out", "policy_sample"
POLICY_OUT_BIT, POLICY_SAMPLE_BIT = 1 << 10, 1 << 11
# ... and bit 12, IRLOSC_LOG_REWARD, which only a slot with a reward (rewarded below) knows: [R, 4] r, ret, steps, goal_step >= 0.
REWARD = "reward"
REWARD_BIT = 1 << 12
_EXTRA = (OBJECT_POSE, POLICY_OUT, POLICY_SAMPLE, REWARD)      # bits 9, 10, 11, 12
MAX_N, MAX_DEV, MAX_OBJECTS = 32, 4, 4


def _channels(nobj: int, n_out: int = 0, rewarded: bool = False) -> tuple:
    """The channel names by bit, up to the last one a slot with nobj action objects, a policy of n_out outputs and (rewarded) a reward can have."""
    if rewarded:
        return CHANNELS + _EXTRA
    if n_out:
        return CHANNELS + (OBJECT_POSE, POLICY_OUT, POLICY_SAMPLE)
    return CHANNELS + (OBJECT_POSE,) if nobj else CHANNELS


def known(nobj: int = 0, n_out: int = 0, sampled: bool = False, rewarded: bool = False) -> int:
    """The OR of the bits a slot with nobj action objects, a policy of n_out outputs (0: none), `sampled`, a Gaussian head and, `rewarded`,
    a reward knows."""
    return (ALL | (OBJECT_POSE_BIT if nobj else 0) | (POLICY_OUT_BIT if n_out else 0) | (POLICY_SAMPLE_BIT if n_out and sampled else 0)
            | (REWARD_BIT if rewarded else 0))


def mask(channels) -> int:
    """An OR of IRLOSC_LOG_* bits from an int or from names ("qpos", ...)."""
    if isinstance(channels, (int, np.integer)):
        return int(channels)
    if isinstance(channels, str):
        channels = [channels]
    m = 0
    for name in channels:
        if name in _EXTRA:
            m |= OBJECT_POSE_BIT << _EXTRA.index(name)
            continue
        if name not in BITS:
            raise ValueError(f"unknown log channel {name!r}: one of {CHANNELS + _EXTRA}")
        m |= BITS[name]
    return m


def names(channels) -> tuple:
    """The names of the channels of a mask, in bit order."""
    m = mask(channels)
    return tuple(name for i, name in enumerate(CHANNELS + _EXTRA) if (m >> i) & 1)


def shape(name: str, n: int, ndev: int, nobj: int = 0, n_out: int = 0) -> tuple:
    """The per-robot shape of a channel: its plane is [R, *shape]."""
    if name == REWARD:
        return (4,)
    if name == OBJECT_POSE:
        return (nobj, 8)
    if name in (POLICY_OUT, POLICY_SAMPLE):
        return (n_out + (name == POLICY_SAMPLE),)
    return {"qpos": (n,), "qvel": (n,), "ee_pose": (ndev, 7), "targets": (ndev, 7), "wrench": (ndev, 6), "u": (n,), "flags": (),
            "wall_force": (ndev, 3), "joint_tau": (n,)}[name]


def layout(n: int, ndev: int, channels, R: int, nobj: int = 0, n_out: int = 0, sampled: bool = False, rewarded: bool = False):
    """-> (offset[9] int64, sample_words) as irlosc_log_layout gives them: where each channel's plane [R][w] starts inside a sample, in
    doubles (-1: not asked for), and the sample's size.  With nobj > 0 (a slot with action objects): offset[10] as
    irlosc_log_layout_objects gives them, the tenth OBJECT_POSE's.  With n_out > 0 (a slot with a policy; `sampled`: with a Gaussian
    head): offset[12] as irlosc_log_layout_policy gives them.  With `rewarded` (a slot with a reward): offset[13] as
    irlosc_log_layout_reward gives them.  Raises ValueError where the library answers IRLOSC_ERR_ARG."""
    m = mask(channels)
    if not 0 <= nobj <= MAX_OBJECTS:
        raise ValueError(f"nobj={nobj} out of range")
    if n_out not in (0, 6, 7):
        raise ValueError(f"n_out={n_out} must be 0, 6 or 7")
    chans = _channels(nobj, n_out, rewarded)
    if m == 0 or m & ~known(nobj, n_out, sampled, rewarded):
        raise ValueError(f"channels=0x{m:x} must be a non-empty OR of the IRLOSC_LOG_* bits")
    if R < 1 or not 1 <= n <= MAX_N or not 1 <= ndev <= MAX_DEV:
        raise ValueError(f"R={R}, n={n}, ndev={ndev} out of range")
    off = np.full(len(chans), -1, dtype=np.int64)
    words = 0
    for i, name in enumerate(chans):
        if (m >> i) & 1:
            off[i] = words
            words += R * int(np.prod(shape(name, n, ndev, nobj, n_out), dtype=np.int64))
    return off, words


def split(buf, n: int, ndev: int, channels, R: int, dtype=np.float64, nobj: int = 0, n_out: int = 0, sampled: bool = False,
          rewarded: bool = False) -> dict:
    """The raw log buffer [S, sample_words] (float64) as named arrays [S, R, ...].  u, targets and wrench come back in `dtype` (the
    context's: the cast undoes the exact widening), flags as uint32, policy_out as float32, everything else float64 (policy_sample: the
    float32 action widened -- .astype(float32) undoes it -- and logp in its last column; reward: r, ret, steps, goal as doubles)."""
    off, words = layout(n, ndev, channels, R, nobj, n_out, sampled, rewarded)
    buf = np.asarray(buf, dtype=np.float64).reshape(-1, words)
    out = {}
    for i, name in enumerate(_channels(nobj, n_out, rewarded)):
        if off[i] < 0:
            continue
        shp = shape(name, n, ndev, nobj, n_out)
        w = int(np.prod(shp, dtype=np.int64))
        a = buf[:, off[i]:off[i] + R * w].reshape((buf.shape[0], R) + shp)
        if name in ("u", "targets", "wrench"):
            a = a.astype(dtype)
        elif name == "flags":
            a = a.astype(np.uint32)
        elif name == POLICY_OUT:
            a = a.astype(np.float32)
        else:
            a = a.copy()
        out[name] = a
    return out
