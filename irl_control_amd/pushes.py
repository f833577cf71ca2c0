"""External pushes of a rollout (BatchedOSC.set_pushes, include/irlosc.h: irlosc_set_pushes), restated in NumPy: which ticks the
reference's push window covers, and the two summed wrenches a tick sees -- what acts on the plant on tick t and what the F/T sensors
report of tick t - 1 -- with the rounding order of csrc/osc_push.hpp, so that a host loop can repeat a rollout's pushes bit for bit."""
import numpy as np


def push_window_ticks(push_window):
    """The reference pushes while ``push_window[0] < count < push_window[1]`` with ``count`` counting the ticks from 1
    (examples/headless_loops.py::admit_test_loop).  -> the half-open window (tick0, tick1) of 0-based ticks that condition holds on:
    [push_window[0], push_window[1] - 1).  A window that holds no tick is refused."""
    lo, hi = int(push_window[0]), int(push_window[1])
    tick0, tick1 = max(lo, 0), hi - 1
    if tick1 <= tick0:
        raise ValueError(f"push_window={tuple(push_window)} holds no tick")
    return tick0, tick1


def normalise(pushes, dev_names):
    """pushes: a list of dict(dev=name_or_index, window=(tick0, tick1), apply=True, sense=True) -> (dev, tick0, tick1, apply, sense)
    as integer / bool arrays [P], checked as the library checks them."""
    names = list(dev_names)
    P = len(pushes)
    dev, t0, t1 = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    ap, se = np.zeros(P, bool), np.zeros(P, bool)
    for p, d in enumerate(pushes):
        dv = d["dev"]
        dev[p] = names.index(dv) if isinstance(dv, str) else int(dv)
        t0[p], t1[p] = (int(x) for x in d["window"])
        ap[p], se[p] = bool(d.get("apply", True)), bool(d.get("sense", True))
        if not 0 <= dev[p] < len(names):
            raise ValueError(f"pushes[{p}]: device {dv!r} is not one of {names}")
        if not 0 <= t0[p] < t1[p]:
            raise ValueError(f"pushes[{p}]: window {d['window']} must hold 0 <= tick0 < tick1")
        if not (ap[p] or se[p]):
            raise ValueError(f"pushes[{p}]: neither applied nor sensed")
    return dev, t0, t1, ap, se


def _sum(wrench, dev, t0, t1, which, t, ndev):
    """-> (W [B, ndev, 6], non-empty [ndev]): per device the wrenches of the pushes of `which` active on tick t, summed in ascending p --
    the first one taken as it is, every add rounded on its own (float64)."""
    B = wrench.shape[0]
    W = np.zeros((B, ndev, 6))
    some = np.zeros(ndev, bool)
    for p in range(len(dev)):
        if not (which[p] and t0[p] <= t < t1[p]):
            continue
        d = dev[p]
        W[:, d] = W[:, d] + wrench[:, p] if some[d] else wrench[:, p]
        some[d] = True
    return W, some


def summed_wrenches(pushes, wrench, dev_names, t, B=None):
    """What tick `t` (0-based, counted since set_pushes) sees of `pushes` with wrenches `wrench` ([P, 6] shared or [B, P, 6] per robot):
    -> dict(apply [B, ndev, 6], apply_some [ndev], sense [B, ndev, 6], sense_some [ndev]).  `apply` is W^apply(t), what acts on the plant
    on this tick; `sense` is W^sense(t - 1), what the sensors read of the tick before and the OSC step of this tick sees taken off its
    wrench (zero on tick 0).  *_some: the devices whose sum is not empty.  A shared table is broadcast to B robots (default 1)."""
    dev, t0, t1, ap, se = normalise(pushes, dev_names)
    w = np.asarray(wrench, dtype=np.float64)
    if w.ndim == 2:
        w = np.broadcast_to(w[None], (1 if B is None else B,) + w.shape)
    if w.ndim != 3 or w.shape[1:] != (len(dev), 6):
        raise ValueError(f"wrench: expected shape ({len(dev)}, 6) or (B, {len(dev)}, 6), got {np.shape(wrench)}")
    nd = len(list(dev_names))
    Wa, sa = _sum(w, dev, t0, t1, ap, int(t), nd)
    Ws, ss = _sum(w, dev, t0, t1, se, int(t) - 1, nd)
    return dict(apply=Wa, apply_some=sa, sense=Ws, sense_some=ss)
