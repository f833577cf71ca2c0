"""The episode log of a rollout, the host side (no GPU): the ctypes mirror of struct irlosc_log, the exports, irlosc_log_layout (which is
context-free and needs no device) against its NumPy mirror rollout_log.layout, its refusals, and split() on a synthetic buffer."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from irl_control_amd import _lib, rollout_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ("irlosc_log_layout", "irlosc_rollout_from_q_logged")
SINGLE = [1 << i for i in range(9)]


def header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def test_log_struct_matches_header_layout():
    L = _lib.Log
    assert C.sizeof(L) == 4 * 4 + 8 == 24
    assert {f: getattr(L, f).offset for f, _ in L._fields_} == dict(channels=0, every=4, n_robots=8, reserved=12, buffer_bytes=16)
    body = re.search(r"typedef struct irlosc_log \{(.*?)\} irlosc_log;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|int32_t|uint64_t)\s+(\w+);", body)
    assert [f[1] for f in fields] == [f for f, _ in L._fields_]
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64}
    for (ty, name), (_, ct) in zip(fields, L._fields_):
        assert ct is ctype[ty], name


def test_channel_bits_match_the_header():
    hdr = header()
    for i, name in enumerate(rollout_log.CHANNELS):
        m = re.search(r"#define\s+IRLOSC_LOG_%s\s+(\d+)u" % name.upper(), hdr)
        assert m and int(m.group(1)) == 1 << i == rollout_log.BITS[name] == getattr(_lib, "LOG_" + name.upper()), name
    assert rollout_log.ALL == 511 and rollout_log.names(0b100101) == ("qpos", "ee_pose", "u")
    assert rollout_log.mask(["u", "qpos"]) == 33 and rollout_log.mask("flags") == 64 and rollout_log.mask(7) == 7
    with pytest.raises(ValueError):
        rollout_log.mask(["torque"])


def test_exports_and_abi_version():
    hdr = header()
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), name
        assert re.search(r"IRLOSC_API int %s\(" % name, hdr), name
    assert _lib.ABI_VERSION == 3 and re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", hdr)


def c_layout(n, ndev, channels, R):
    lib = _lib.load()
    off = np.full(9, -7, dtype=np.int64)
    words = C.c_int64(-7)
    rc = lib.irlosc_log_layout(n, ndev, channels, R, _lib.ptr(off), C.addressof(words))
    return rc, off, words.value


@pytest.mark.parametrize("n,ndev", [(25, 1), (25, 3), (25, 4)])
@pytest.mark.parametrize("R", [1, 64, 65])
def test_layout_equals_its_numpy_mirror(n, ndev, R):
    width = [n, n, ndev * 7, ndev * 7, ndev * 6, n, 1, ndev * 3, n]
    for channels in SINGLE + [511]:
        rc, off, words = c_layout(n, ndev, channels, R)
        assert rc == 0
        moff, mwords = rollout_log.layout(n, ndev, channels, R)
        assert np.array_equal(off, moff) and words == mwords, channels
        # ... and both are what the header says: planes [R][w] in ascending bit order
        at = 0
        for i in range(9):
            if (channels >> i) & 1:
                assert off[i] == at
                at += R * width[i]
            else:
                assert off[i] == -1
        assert words == at
    if (n, ndev) == (25, 3):
        assert c_layout(n, ndev, 511, R)[2] == 170 * R      # k13: 170 doubles per robot


@pytest.mark.parametrize("why,args", [
    ("channels 0", (25, 3, 0, 4)), ("an unknown bit", (25, 3, 512, 4)), ("an unknown bit next to known ones", (25, 3, 1 | 1 << 31, 4)),
    ("R 0", (25, 3, 1, 0)), ("R negative", (25, 3, 1, -1)), ("n 0", (0, 3, 1, 4)), ("n 33", (33, 3, 1, 4)),
    ("ndev 0", (25, 0, 1, 4)), ("ndev 5", (25, 5, 1, 4))])
def test_layout_refusals(why, args):
    assert c_layout(*args)[0] == ERR_ARG, why
    with pytest.raises(ValueError):
        rollout_log.layout(*args)


def test_layout_refuses_null_outputs():
    lib = _lib.load()
    off = np.zeros(9, dtype=np.int64)
    words = C.c_int64(0)
    assert lib.irlosc_log_layout(25, 3, 1, 4, None, C.addressof(words)) == ERR_ARG
    assert lib.irlosc_log_layout(25, 3, 1, 4, _lib.ptr(off), None) == ERR_ARG


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("channels", [511, 1 | 4 | 32 | 64, 64, 128 | 256])
def test_split_round_trips_a_synthetic_buffer(dtype, channels):
    n, ndev, R, S = 25, 3, 5, 4
    rng = np.random.default_rng(channels)
    want = {}
    for name in rollout_log.names(channels):
        shp = (S, R) + rollout_log.shape(name, n, ndev)
        if name == "flags":
            want[name] = rng.integers(0, 2 ** 32, shp, dtype=np.uint64).astype(np.uint32)
        elif name in ("u", "targets", "wrench"):
            want[name] = rng.normal(size=shp).astype(dtype)
        else:
            want[name] = rng.normal(size=shp)
    off, words = rollout_log.layout(n, ndev, channels, R)
    buf = np.full((S, words), np.nan)
    for i, name in enumerate(rollout_log.CHANNELS):
        if name in want:
            buf[:, off[i]:off[i] + want[name][0].size] = want[name].reshape(S, -1).astype(np.float64)      # (widening: exact)
    assert not np.isnan(buf).any()      # the planes tile the sample
    got = rollout_log.split(buf, n, ndev, channels, R, dtype=dtype)
    assert list(got) == list(want)
    for name in want:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, name
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
    # the flat buffer, as the library fills it, splits alike
    flat = rollout_log.split(buf.reshape(-1), n, ndev, channels, R, dtype=dtype)
    assert all(np.array_equal(flat[k], got[k]) for k in got)
