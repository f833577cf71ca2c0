"""Compliant walls of a rollout, the host side (no GPU): the ctypes mirror of struct irlosc_walls, the exports, every refusal of
walls.normalise and the NumPy restatement of the wall force (irl_control_amd/walls.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from irl_control_amd import _lib, walls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ur5right", "ur5left", "base"]
REF = dict(dev="ur5left", normal=(0.0, -1.0, 0.0), offset=-0.75, radius=0.1, stiffness=900.0, damping=20.0)      # force_test's wall


def test_walls_struct_matches_header_layout():
    # struct irlosc_walls: n_walls, nb (int32), dev[8] (int32)
    W = _lib.Walls
    assert C.sizeof(W) == 4 * 2 + 4 * 8 == 40
    assert {f: getattr(W, f).offset for f, _ in W._fields_} == dict(n_walls=0, nb=4, dev=8)
    hdr = open(os.path.join(ROOT, "include", "irlosc.h")).read()
    assert "#define IRLOSC_MAX_WALLS 8" in hdr and _lib.MAX_WALLS == 8 and walls.MAX_WALLS == 8
    body = re.search(r"typedef struct irlosc_walls \{(.*?)\} irlosc_walls;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|uint8_t)\s+(\w+)(\[IRLOSC_MAX_WALLS\])?;", body)
    assert [f[1] for f in fields] == [f for f, _ in W._fields_]
    ctype = {"int32_t": C.c_int32, "uint8_t": C.c_uint8}
    for (ty, name, arr), (_, ct) in zip(fields, W._fields_):
        assert ct is (ctype[ty] * 8 if arr else ctype[ty]), name


def test_exports_and_abi_version():
    for name in ("irlosc_set_walls", "irlosc_download_wall_state"):
        assert name in _lib.EXPORTS
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    import fnmatch
    for name in ("irlosc_set_walls", "irlosc_download_wall_state"):
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), name
    hdr = open(os.path.join(ROOT, "include", "irlosc.h")).read()
    assert _lib.ABI_VERSION == 3 and re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", hdr)
    for name in ("irlosc_set_walls", "irlosc_download_wall_state"):
        assert re.search(r"IRLOSC_API int %s\(" % name, hdr), name


def test_normalise_builds_the_table():
    dev, tab = walls.normalise([REF, dict(dev=0, normal=(1.0, 0.0, 0.0), point=(0.25, 7.0, -3.0), stiffness=5.0)], NAMES, 4)
    assert dev.tolist() == [1, 0] and tab.shape == (1, 2, 8)
    assert tab[0, 0].tolist() == [0.0, -1.0, 0.0, -0.75, 0.1, 900.0, 20.0, 0.0]
    assert tab[0, 1].tolist() == [1.0, 0.0, 0.0, 0.25, 0.0, 5.0, 0.0, 0.0]
    # any per-robot value makes the whole table per robot
    off = np.linspace(-1.0, 1.0, 4)
    dev, tab = walls.normalise([REF, dict(REF, dev=2, offset=off)], NAMES, 4)
    assert tab.shape == (4, 2, 8) and np.array_equal(tab[:, 1, 3], off) and np.all(tab[:, 0] == tab[0, 0])
    n = np.tile([0.0, 0.6, 0.8], (4, 1))
    _, tab = walls.normalise([dict(dev=0, normal=n, point=(1.0, 1.0, 1.0), stiffness=np.full(4, 2.0))], NAMES, 4)
    assert tab.shape == (4, 1, 8) and np.array_equal(tab[:, 0, 3], np.full(4, (0.0 * 1.0 + 0.6 * 1.0) + 0.8 * 1.0))


BAD = {
    "no walls": [],
    "nine walls": [REF] * 9,
    "unknown device name": [dict(REF, dev="nobody")],
    "device index too large": [dict(REF, dev=3)],
    "device index negative": [dict(REF, dev=-1)],
    "offset and point": [dict(REF, point=(0.0, 0.75, 0.0))],
    "neither offset nor point": [{k: v for k, v in REF.items() if k != "offset"}],
    "no stiffness": [{k: v for k, v in REF.items() if k != "stiffness"}],
    "unknown key": [dict(REF, friction=0.5)],
    "normal of length 2": [dict(REF, normal=(0.0, 1.0))],
    "normal not unit": [dict(REF, normal=(0.0, -1.0, 1e-5))],
    "normal zero": [dict(REF, normal=(0.0, 0.0, 0.0))],
    "normal NaN": [dict(REF, normal=(np.nan, 0.0, 0.0))],
    "offset inf": [dict(REF, offset=np.inf)],
    "radius negative": [dict(REF, radius=-1e-3)],
    "stiffness negative": [dict(REF, stiffness=-1.0)],
    "damping negative": [dict(REF, damping=-1.0)],
    "stiffness NaN": [dict(REF, stiffness=np.nan)],
    "per-robot array of the wrong length": [dict(REF, offset=np.zeros(3))],
    "per-robot value negative for one robot": [dict(REF, radius=np.array([0.1, 0.1, -0.1, 0.1]))],
}


@pytest.mark.parametrize("why", list(BAD))
def test_normalise_refuses(why):
    with pytest.raises(ValueError):
        walls.normalise(BAD[why], NAMES, 4)


def test_normalise_refuses_a_batch_below_one():
    with pytest.raises(ValueError):
        walls.normalise([REF], NAMES, 0)


def _rows(*ws):
    return np.array([[list(n) + [off, r, k, c, 0.0] for n, off, r, k, c in ws]], dtype=np.float64)


def test_contact_force_is_zero_off_contact_and_never_pulls():
    rng = np.random.default_rng(0)
    B = 4000
    x = rng.normal(0.0, 1.0, (B, 3))
    v = rng.normal(0.0, 2.0, (B, 3))
    rows = _rows(((0.0, -1.0, 0.0), -0.75, 0.1, 900.0, 400.0))
    F = walls.contact_force(x, v, rows)
    g = walls.depth(x, rows)[:, 0]
    assert np.array_equal(g, 0.1 - ((0.0 * x[:, 0] + -1.0 * x[:, 1]) + 0.0 * x[:, 2] - -0.75))
    off = g <= 0.0
    assert off.sum() > 100 and (~off).sum() > 100
    assert not F[off].any()                                        # zero off contact
    nF = F @ np.array([0.0, -1.0, 0.0])
    assert np.all(nF >= 0.0)                                       # never pulling
    f = 900.0 * g - 400.0 * (-v[:, 1])
    clamped = (g > 0.0) & (f <= 0.0)
    assert clamped.sum() > 100 and not F[clamped].any()            # the clamp: approaching fast enough backwards, no force
    on = (g > 0.0) & (f > 0.0)
    assert np.array_equal(F[on, 1], f[on] * -1.0) and np.array_equal(nF[on], f[on])


def test_contact_force_repeats_the_written_rounding_order():
    rng = np.random.default_rng(1)
    B = 500
    x, v = rng.normal(0.0, 1.0, (B, 3)), rng.normal(0.0, 1.0, (B, 3))
    n = rng.normal(size=(B, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    off, r, k, c = rng.normal(size=B), rng.uniform(0, 0.2, B), rng.uniform(1, 1000, B), rng.uniform(0, 50, B)
    _, tab = walls.normalise([dict(dev=0, normal=n, offset=off, radius=r, stiffness=k, damping=c)], NAMES, B)
    F = walls.contact_force(x, v, tab)
    want = np.zeros((B, 3))
    for b in range(B):                                             # scalar float64 arithmetic, one operation at a time
        nx = (n[b, 0] * x[b, 0] + n[b, 1] * x[b, 1]) + n[b, 2] * x[b, 2]
        g = r[b] - (nx - off[b])
        s = (n[b, 0] * v[b, 0] + n[b, 1] * v[b, 1]) + n[b, 2] * v[b, 2]
        f = k[b] * g - c[b] * s
        if g > 0 and f > 0:
            want[b] = [f * n[b, 0], f * n[b, 1], f * n[b, 2]]
    assert np.array_equal(F, want) and (want != 0).any(axis=1).sum() > 50
    assert np.array_equal(walls.contact_force(x, 0.0, tab), walls.contact_force(x, np.zeros((B, 3)), tab))


def test_contact_force_sums_the_walls_in_ascending_order():
    rng = np.random.default_rng(2)
    B = 300
    x = rng.normal(0.0, 0.3, (B, 3))
    ws = [((1.0, 0.0, 0.0), 0.1, 0.01, 917.3, 0.0), ((0.6, 0.0, 0.8), 0.2, 0.02, 333.1, 0.0), ((-0.6, 0.0, -0.8), 0.15, 0.0, 1234.5, 0.0)]
    rows = _rows(*ws)
    F = walls.contact_force(x, 0.0, rows)
    one = [walls.contact_force(x, 0.0, rows[:, w:w + 1]) for w in range(3)]
    assert np.array_equal(F, (one[0] + one[1]) + one[2])
    assert (F != one[0] + (one[1] + one[2])).any()                 # three terms: the order is part of the result
    assert all(o.any(axis=1).sum() > B // 2 for o in one)
    # a shared table equals a per-robot table that repeats it
    assert np.array_equal(F, walls.contact_force(x, 0.0, np.tile(rows, (B, 1, 1))))


def test_a_nan_gives_no_contact_and_no_force():
    rows = _rows(((0.0, -1.0, 0.0), -0.75, 0.1, 900.0, 20.0))
    x = np.array([[0.0, 0.8, 0.5], [np.nan, 0.8, 0.5], [0.0, np.nan, 0.5], [0.0, 0.8, 0.5], [0.0, 0.8, 0.5]])
    v = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, np.nan, 0.0], [np.nan, 0.0, 0.0]])
    F = walls.contact_force(x, v, rows)
    assert F[0, 1] < 0.0 and not F[1:].any() and np.all(np.isfinite(F))
    g = walls.depth(x, rows)[:, 0]
    assert not (g[1:3] > 0.0).any() and (g[[0, 3, 4]] > 0.0).all()
