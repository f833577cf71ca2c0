"""External pushes of a rollout, the host side (no GPU): the ctypes mirror of struct irlosc_pushes, the window helper against the
reference loop's own condition, and the NumPy restatement of the two summed wrenches (irl_control_amd/pushes.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from irl_control_amd import _lib, pushes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ur5right", "ur5left", "base"]


def test_pushes_struct_matches_header_layout():
    # struct irlosc_pushes: n_pushes, nb (int32), dev[8], tick0[8], tick1[8] (int32), apply[8], sense[8] (uint8)
    P = _lib.Pushes
    assert C.sizeof(P) == 4 * 2 + 4 * 8 * 3 + 8 * 2 == 120
    want = dict(n_pushes=0, nb=4, dev=8, tick0=40, tick1=72, apply=104, sense=112)
    assert {f: getattr(P, f).offset for f, _ in P._fields_} == want
    hdr = open(os.path.join(ROOT, "include", "irlosc.h")).read()
    assert "#define IRLOSC_MAX_PUSHES 8" in hdr and _lib.MAX_PUSHES == 8
    body = re.search(r"typedef struct irlosc_pushes \{(.*?)\} irlosc_pushes;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|uint8_t)\s+(\w+)(\[IRLOSC_MAX_PUSHES\])?;", body)
    assert [f[1] for f in fields] == [f for f, _ in P._fields_]
    ctype = {"int32_t": C.c_int32, "uint8_t": C.c_uint8}
    for (ty, name, arr), (_, ct) in zip(fields, P._fields_):
        assert ct is (ctype[ty] * 8 if arr else ctype[ty]), name
    assert "irlosc_set_pushes" in _lib.EXPORTS


def _reference_ticks(push_window, ticks):
    """The 0-based ticks on which admit_test_loop's condition holds, by enumerating its 1-based count."""
    out, count = [], 0
    for t in range(ticks):
        count += 1
        if push_window[0] < count < push_window[1]:
            out.append(t)
    return out


@pytest.mark.parametrize("window,ticks", [((3000, 5000), 6000), ((7, 9), 20), ((0, 3), 10)])
def test_window_helper_agrees_with_the_reference_condition(window, ticks):
    t0, t1 = pushes.push_window_ticks(window)
    assert (t0, t1) == (window[0], window[1] - 1)
    assert list(range(t0, t1)) == _reference_ticks(window, ticks)
    if window == (7, 9):
        assert t1 - t0 == 1                      # a window of width 2: one active tick


def test_window_helper_refuses_a_window_without_a_tick():
    assert _reference_ticks((7, 8), 20) == []    # width 1: the reference never pushes
    with pytest.raises(ValueError):
        pushes.push_window_ticks((7, 8))


def _w(rng, B, P):
    return np.concatenate([rng.normal(0, 20.0, (B, P, 3)), rng.normal(0, 2.0, (B, P, 3))], axis=2)


def test_overlapping_pushes_on_one_device_sum_in_ascending_order():
    rng = np.random.default_rng(0)
    B = 5
    ps = [dict(dev="ur5left", window=(2, 6)), dict(dev=1, window=(4, 8)), dict(dev="ur5left", window=(5, 7))]
    w = _w(rng, B, 3)
    for t in range(10):
        r = pushes.summed_wrenches(ps, w, NAMES, t)
        on = [p for p, d in enumerate(ps) if d["window"][0] <= t < d["window"][1]]
        want = np.zeros((B, 6))
        for i, p in enumerate(on):
            want = w[:, p] if i == 0 else want + w[:, p]      # each add rounded on its own, ascending p
        assert np.array_equal(r["apply"][:, 1], want)
        assert list(r["apply_some"]) == [False, bool(on), False]
        assert not r["apply"][:, [0, 2]].any()
    # three terms: the order is part of the result
    r = pushes.summed_wrenches(ps, w, NAMES, 5)
    assert np.array_equal(r["apply"][:, 1], (w[:, 0] + w[:, 1]) + w[:, 2])


def test_disjoint_windows_and_devices():
    rng = np.random.default_rng(1)
    ps = [dict(dev=0, window=(0, 2)), dict(dev=2, window=(3, 4)), dict(dev=0, window=(5, 6))]
    w = _w(rng, 1, 3)[0]
    for t, (d, p) in {0: (0, 0), 1: (0, 0), 3: (2, 1), 5: (0, 2)}.items():
        r = pushes.summed_wrenches(ps, w, NAMES, t, B=4)
        assert r["apply"].shape == (4, 3, 6)
        assert np.array_equal(r["apply"][:, d], np.broadcast_to(w[p], (4, 6)))
        assert r["apply_some"].sum() == 1 and r["apply_some"][d]
    for t in (2, 4, 6, 100):
        r = pushes.summed_wrenches(ps, w, NAMES, t)
        assert not r["apply_some"].any() and not r["apply"].any()


def test_apply_only_and_sense_only_and_the_one_tick_lag():
    rng = np.random.default_rng(2)
    ps = [dict(dev=1, window=(2, 4), apply=True, sense=False), dict(dev=1, window=(2, 4), apply=False, sense=True),
          dict(dev=0, window=(3, 5))]
    w = _w(rng, 3, 3)
    for t in range(8):
        r = pushes.summed_wrenches(ps, w, NAMES, t)
        # applied on the ticks of the window, push 0 and never push 1
        assert np.array_equal(r["apply"][:, 1], w[:, 0] if 2 <= t < 4 else np.zeros((3, 6)))
        # sensed one tick later, push 1 and never push 0
        assert np.array_equal(r["sense"][:, 1], w[:, 1] if 3 <= t < 5 else np.zeros((3, 6)))
        assert r["sense_some"][1] == (3 <= t < 5) and r["apply_some"][1] == (2 <= t < 4)
        # a push with both: W^sense(t - 1) of this tick is W^apply of the tick before
        before = pushes.summed_wrenches(ps, w, NAMES, t - 1)["apply"][:, 0] if t >= 1 else np.zeros((3, 6))
        assert np.array_equal(r["sense"][:, 0], before)
    r0 = pushes.summed_wrenches([dict(dev=0, window=(0, 1))], w[:, :1], NAMES, 0)
    assert r0["apply_some"][0] and not r0["sense_some"].any() and not r0["sense"].any()      # nothing is sensed on tick 0


def test_shared_table_equals_a_per_robot_table_that_repeats_it():
    rng = np.random.default_rng(3)
    ps = [dict(dev=0, window=(0, 3)), dict(dev=0, window=(1, 4), sense=False), dict(dev=2, window=(2, 3), apply=False)]
    w = _w(rng, 1, 3)[0]
    for t in range(6):
        a = pushes.summed_wrenches(ps, w, NAMES, t, B=7)
        b = pushes.summed_wrenches(ps, np.tile(w[None], (7, 1, 1)), NAMES, t)
        for key in a:
            assert np.array_equal(a[key], b[key]), key


def test_descriptions_are_checked():
    for bad in ([dict(dev="nobody", window=(0, 1))], [dict(dev=3, window=(0, 1))], [dict(dev=0, window=(2, 2))],
                [dict(dev=0, window=(-1, 2))], [dict(dev=0, window=(0, 1), apply=False, sense=False)]):
        with pytest.raises(ValueError):
            pushes.normalise(bad, NAMES)
    with pytest.raises(ValueError):
        pushes.summed_wrenches([dict(dev=0, window=(0, 1))], np.zeros((2, 6)), NAMES, 0)
