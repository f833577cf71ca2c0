"""Episodes of a rollout, the part that needs no GPU: the two exports are declared in include/irlosc.h with struct irlosc_episodes, fall
under the version script's pattern, are bound by _lib.py with a struct of the header's layout, the ABI version stays 3 -- and the NumPy
side (irl_control_amd/episodes.py): `schedule` and `stitch` on hand-made lengths, the early-exit formula against a brute-force loop."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from irl_control_amd import _lib, episodes as ep

NEW = ("irlosc_set_episodes", "irlosc_download_episode_state")
FIN, TMO = ep.FINISHED, ep.TIMEOUT


def _header():
    with open(os.path.join(ROOT, "include", "irlosc.h")) as f:
        return f.read()


def test_header_declares_the_episode_exports():
    h = _header()
    for name in NEW:
        assert re.search(r"IRLOSC_API\s+int\s+" + name + r"\s*\(", h), name
    assert re.search(r"#define\s+IRLOSC_EPISODE_FINISHED\s+1\b", h) and re.search(r"#define\s+IRLOSC_EPISODE_TIMEOUT\s+2\b", h)
    assert (_lib.EPISODE_FINISHED, _lib.EPISODE_TIMEOUT) == (FIN, TMO) == (1, 2)
    assert re.search(r"#define\s+IRLOSC_MAX_EPISODE_RECORDS\s+16\b", h) and _lib.MAX_EPISODE_RECORDS == 16
    assert re.search(r"#define\s+IRLOSC_MAX_EPISODE_STARTS\s+4096\b", h) and _lib.MAX_EPISODE_STARTS == 4096
    assert re.search(r"#define\s+IRLOSC_ABI_VERSION\s+3\b", h) and _lib.ABI_VERSION == 3      # additive exports: the version stays


def test_version_script_and_binding_list_them():
    with open(os.path.join(ROOT, "irl_control_amd", "csrc", "irlosc.map")) as f:
        pats = re.search(r"global:(.*?);\s*local:", f.read(), flags=re.S).group(1).replace(";", " ").split()
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), (name, pats)
        assert name in _lib.EXPORTS


def test_episodes_struct_matches_header_layout():
    """The binding's struct field by field against the header's: nine int32, 36 bytes, no padding."""
    m = re.search(r"typedef struct irlosc_episodes \{(.*?)\} irlosc_episodes;", _header(), flags=re.S)
    assert m, "struct irlosc_episodes"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t)\s+(\w+);", body)
    assert [f[1] for f in fields] == ["max_ticks", "end_on_finish", "max_episodes", "n_starts", "starts_per_robot", "n_variants", "records",
                                      "poll_every", "reserved"]
    mirror = type("Mirror", (C.Structure,), {"_fields_": [(n, C.c_int32) for _, n in fields]})
    assert [f[0] for f in _lib.Episodes._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.Episodes) == C.sizeof(mirror) == 36
    for name, _ in mirror._fields_:
        assert getattr(_lib.Episodes, name).offset == getattr(mirror, name).offset, name


# ---- schedule / stitch on hand-made lengths ---------------------------------------------------------------------------------------------
MAXT = 5
# S = 2, V = 3 (they do not divide each other: six episodes until (start, variant) repeats), B = 4.  Robot 0: every episode times out;
# robot 1: mixed lengths; robot 2: finishes ON the timeout tick everywhere; robot 3: one tick per episode.
_FINISH = np.full((2, 3, 4), -1)
_FINISH[:, :, 1] = [[0, 2, 7], [3, 1, -1]]      # (7: done only after the timeout: TIMEOUT)
_FINISH[:, :, 2] = MAXT - 1
_FINISH[:, :, 3] = 0
LENGTHS, OUTCOMES = ep.lengths_from_finish(_FINISH, MAXT)


def test_lengths_from_finish():
    assert np.array_equal(LENGTHS[:, :, 0], np.full((2, 3), MAXT)) and np.all(OUTCOMES[:, :, 0] == TMO)
    assert np.array_equal(LENGTHS[:, :, 1], [[1, 3, MAXT], [4, 2, MAXT]])
    assert np.array_equal(OUTCOMES[:, :, 1], [[FIN, FIN, TMO], [FIN, FIN, TMO]])
    assert np.all(LENGTHS[:, :, 2] == MAXT) and np.all(OUTCOMES[:, :, 2] == FIN)      # a finish on the timeout tick is FINISHED
    ln, oc = ep.lengths_from_finish([3, -1], 0)                                        # no timeout: the unfinished one never ends
    assert list(ln) == [4, 0] and list(oc) == [FIN, TMO]
    ln, oc = ep.lengths_from_finish([3, -1], 6, end_on_finish=False)
    assert list(ln) == [6, 6] and list(oc) == [TMO, TMO]


def brute_schedule(T, max_episodes, ran=None):
    """The rule of include/irlosc.h, robot by robot and tick by tick, written the long way round: (episode, start, variant, age) rows."""
    S, V, B = LENGTHS.shape
    rows = np.zeros((T, B, 4), np.int64)
    count = np.zeros(B, np.int64)
    for b in range(B):
        c, age, over = 0, 0, 0
        for t in range(T):
            parked = max_episodes > 0 and c >= max_episodes
            e = c - 1 if parked else c
            rows[t, b] = (e, e % S, e % V, age + over)
            if ran is not None and not ran[t, b]:
                continue
            if parked:
                over += 1
                continue
            age += 1
            if age == LENGTHS[e % S, e % V, b]:
                c += 1
                if not (max_episodes > 0 and c >= max_episodes):
                    age = 0
        count[b] = c
    return rows, count


@pytest.mark.parametrize("max_episodes", [0, 3])
def test_schedule_follows_the_rule(max_episodes):
    T = 40
    sc = ep.schedule(LENGTHS, OUTCOMES, T, max_episodes)
    rows, count = brute_schedule(T, max_episodes)
    for i, k in enumerate(("episode", "start", "variant", "age")):
        assert np.array_equal(sc[k], rows[:, :, i]), k
    assert np.array_equal(sc["count"], count)
    # robot 0: every episode times out after MAXT ticks, back to back
    assert [r[:3] for r in sc["records"][0]][:3] == [(0, MAXT, TMO), (MAXT, MAXT, TMO), (2 * MAXT, MAXT, TMO)]
    # robot 1 walks (start, variant) = (0,0) (1,1) (0,2) (1,0) (0,1) (1,2): S = 2 and V = 3 do not divide each other
    want = [(0, 1, FIN, 0, 0), (1, 2, FIN, 1, 1), (3, MAXT, TMO, 0, 2), (8, 4, FIN, 1, 0), (12, 3, FIN, 0, 1), (15, MAXT, TMO, 1, 2)]
    assert sc["records"][1][:len(want)][:max_episodes or None] == want[:max_episodes or None]
    assert all(r[2] == FIN and r[1] == MAXT for r in sc["records"][2])      # robot 2: FINISHED on the timeout tick
    if max_episodes:
        assert np.array_equal(sc["count"], [3, 3, 3, 3])
        assert np.array_equal(sc["park_tick"], [3 * MAXT - 1, 7, 3 * MAXT - 1, 2])
        assert not sc["parked"][7, 1] and sc["parked"][8:, 1].all()
        # a parked robot stays in its last episode and its fresh rollout runs on: ages 5, 6, 7, ... behind the TIMEOUT of length 5
        assert np.array_equal(sc["episode"][8:12, 1], [2, 2, 2, 2]) and np.array_equal(sc["age"][8:12, 1], [5, 6, 7, 8])
        assert sc["age_end"][1] == MAXT and sc["start_tick"][1] == 3
    else:
        assert (sc["park_tick"] == -1).all() and not sc["parked"].any()
        assert sc["count"][3] == T and sc["count"][0] == T // MAXT


def test_a_narrower_rollout_leaves_ages_standing():
    T = 12
    ran = np.ones((T, 4), bool)
    ran[2:7, 2:] = False            # ticks 2 .. 6 run robots 0 and 1 only
    sc = ep.schedule(LENGTHS, OUTCOMES, T, 0, ran=ran)
    rows, count = brute_schedule(T, 0, ran)
    assert np.array_equal(sc["age"], rows[:, :, 3]) and np.array_equal(sc["episode"], rows[:, :, 0]) and np.array_equal(sc["count"], count)
    assert np.array_equal(sc["age"][2:8, 2], [2, 2, 2, 2, 2, 2]) and sc["age"][8, 2] == 3
    assert sc["records"][2][0][:2] == (0, MAXT) and sc["records"][2][0][0] == 0      # started on tick 0, ended on tick 9: length counts run ticks
    # robot 3 ends an episode per tick that runs it; the episode that meets the gap starts behind it
    assert [r[0] for r in sc["records"][3]] == [0, 1, 7, 8, 9, 10, 11]


def test_ring_keeps_the_last_records():
    sc = ep.schedule(LENGTHS, OUTCOMES, 40, 0)
    r = ep.ring(sc, 4)
    assert r.shape == (4, 4, 4) and r.dtype == np.int32
    rec = sc["records"][1]
    for e in range(len(rec) - 4, len(rec)):
        st, ln, oc, s, v = rec[e]
        assert tuple(r[1, e % 4]) == (st, ln, oc, s | (v << 16))
    few = ep.ring(ep.schedule(LENGTHS, OUTCOMES, 7, 0), 4)
    assert not few[0, 1:].any() and tuple(few[0, 0]) == (0, MAXT, TMO, 0)


def test_stitch_composes_the_timeline():
    """fresh[s, v, t, b] = a code of (s, v, t, b): the stitched timeline must read, at (tick, robot), the code of the schedule's entry."""
    S, V, B = LENGTHS.shape
    Tf, T = 32, 30
    code = (np.arange(S)[:, None, None, None] * 1000000 + np.arange(V)[None, :, None, None] * 10000 + np.arange(Tf)[None, None, :, None] * 100 +
            np.arange(B)[None, None, None, :]).astype(np.float64)
    fresh = dict(x=code, y=np.stack([code, -code], axis=-1))
    sc = ep.schedule(LENGTHS, OUTCOMES, T, 3)
    out = ep.stitch(fresh, sc)
    assert out["x"].shape == (T, B) and out["y"].shape == (T, B, 2)
    for t in range(T):
        for b in range(B):
            want = sc["start"][t, b] * 1000000 + sc["variant"][t, b] * 10000 + sc["age"][t, b] * 100 + b
            assert out["x"][t, b] == want and tuple(out["y"][t, b]) == (want, -want)
    with pytest.raises(ValueError):      # robot 3 parks on tick 2 and runs on: tick 39 of the call is tick 39 of its fresh rollout
        ep.stitch(dict(x=code), ep.schedule(LENGTHS, OUTCOMES, 40, 3))


def brute_ticks_run(park_tick, ticks, P):
    """The host's loop of the early exit, spelled out: copies after ticks P - 1, 2 P - 1, ...; before tick m P (m >= 2) the copy made
    after tick (m - 1) P - 1 is looked at."""
    if P == 0:
        return ticks
    copies = {}
    t = 0
    while t < ticks:
        if t % P == 0 and t >= 2 * P and copies[t // P - 1] == 0:
            break
        # tick t runs; afterwards the robots with park_tick > t are still running
        if (t + 1) % P == 0:
            copies[(t + 1) // P] = int(np.sum(np.asarray(park_tick) > t))
        t += 1
    return t


def test_early_exit_formula_against_the_loop():
    rng = np.random.default_rng(0)
    for _ in range(400):
        ticks, P, B = int(rng.integers(1, 80)), int(rng.integers(0, 12)), int(rng.integers(1, 5))
        park = rng.integers(-1, 100, B)
        assert ep.ticks_run(park, ticks, P) == brute_ticks_run(park, ticks, P), (park, ticks, P)
    assert ep.ticks_run([13, 40], 100, 8) == 56      # the last robot parks on tick 40: copy 6 (after tick 47) says so, tick 56 is not run
    assert ep.ticks_run([-1], 100, 8) == 16          # all parked before the call: the first copy is looked at before tick 16
    assert ep.ticks_run([7], 100, 8) == 16 and ep.ticks_run([8], 100, 8) == 24
    assert ep.ticks_run([40], 50, 8) == 50 and ep.ticks_run([40], 100, 0) == 100
