"""The NumPy side of a rollout's episodes (BatchedOSC.set_episodes, csrc/osc_episode.hpp): which episode, start state and pose variant
every (robot, tick) of a long rollout belongs to, given how long every episode lasts -- and a robot's timeline composed from the logs of
fresh rollouts.  Every robot's arithmetic is its own lane's, so episode e of robot b IS the first `length` ticks of a fresh rollout from
start e mod S with variant e mod V: the device's resets are held to that, bit for bit (tests/test_episodes.py).

Conventions: S start states, V pose variants (0 counts as one: the list's own table), T ticks, B robots.  `lengths[s, v, b]` and
`outcomes[s, v, b]` say how a fresh episode of robot b from start s with variant v ends: after `length` ticks, FINISHED or TIMEOUT."""
import numpy as np

FINISHED, TIMEOUT = 1, 2      # _lib.EPISODE_FINISHED / EPISODE_TIMEOUT
INSERTED, GOAL = 4, 8         # OR-ed into an outcome: every mate mated / the reward's goal reached (_lib.EPISODE_INSERTED / EPISODE_GOAL)


def lengths_from_goal(goal_step, max_ticks, end_on_finish=True):
    """(lengths, outcomes) of fresh episodes on a slot whose reward has a goal, from the reward's goal_step of a fresh rollout (steps
    when the goal was reached, so 1-based; < 0: never, any shape): FINISHED | GOAL after goal_step ticks where that is within max_ticks,
    else TIMEOUT after max_ticks.  Without end_on_finish the goal ends nothing: TIMEOUT after max_ticks, with GOAL where it was reached
    by then.  max_ticks == 0: no timeout, length 0 = the episode never ends."""
    g = np.asarray(goal_step, dtype=np.int64)
    reached = (g >= 1) & ((g <= max_ticks) | (max_ticks == 0))
    done = bool(end_on_finish) & reached
    lengths = np.where(done, g, max_ticks)
    return lengths, (np.where(done, FINISHED, TIMEOUT) | np.where(reached, GOAL, 0)).astype(np.int32)


def lengths_from_finish(finish_tick, max_ticks, end_on_finish=True):
    """(lengths, outcomes) of fresh episodes from the tick that found each robot done (a list's finished_tick, or for paths the tick
    of the last arrival; < 0: never, any shape): FINISHED after finish_tick + 1 ticks where that is within max_ticks (the tick of the
    timeout included), else TIMEOUT after max_ticks; max_ticks == 0: no timeout, length 0 = the episode never ends."""
    f = np.asarray(finish_tick, dtype=np.int64)
    done = bool(end_on_finish) & (f >= 0) & ((f < max_ticks) | (max_ticks == 0))
    lengths = np.where(done, f + 1, max_ticks)
    return lengths, np.where(done, FINISHED, TIMEOUT).astype(np.int32)


def schedule(lengths, outcomes, ticks, max_episodes=0, ran=None):
    """The timetable of `ticks` ticks of a rollout with episodes.  lengths, outcomes: [S, V, B] (a length 0: that episode never ends);
    max_episodes: 0 = no limit; ran [ticks, B] bool: the robots each tick runs (None: all -- a rollout over fewer robots leaves the
    others' episodes standing).
    -> dict of [ticks, B] arrays: episode (the episode the robot is in on that tick; a parked robot stays in its last), start, variant,
       age (ticks the robot has been run in that episode BEFORE this one: the tick of the fresh rollout it repeats; a parked robot's
       goes on counting, as its rollout simply runs on), parked (bool: parked before this tick), run (bool: = ran);
       and per robot: count [B], age_end [B] (the device's age afterwards), start_tick [B] (of the running episode, -1: not run yet),
       park_tick [B] (the tick on which it parked, -1: running), records: list of B lists of (start_tick, length, outcome, start, variant)."""
    L = np.asarray(lengths, dtype=np.int64)
    O = np.asarray(outcomes)
    S, V, B = L.shape
    T = int(ticks)
    ran = np.ones((T, B), bool) if ran is None else np.asarray(ran, bool)
    out = {k: np.zeros((T, B), np.int64) for k in ("episode", "start", "variant", "age")}
    out["parked"] = np.zeros((T, B), bool)
    out["run"] = ran.copy()
    count, age_end = np.zeros(B, np.int64), np.zeros(B, np.int64)
    start_tick, park_tick = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
    records = []
    for b in range(B):
        e, age, st, parked, extra, rec = 0, 0, -1, False, 0, []
        for t in range(T):
            s, v = e % S, e % V
            out["episode"][t, b], out["start"][t, b], out["variant"][t, b] = e, s, v
            out["age"][t, b], out["parked"][t, b] = age + extra, parked
            if not ran[t, b]:
                continue
            if parked:
                extra += 1
                continue
            if age == 0:
                st = t
            age += 1
            if L[s, v, b] > 0 and age == L[s, v, b]:
                rec.append((st, age, int(O[s, v, b]), s, v))
                if max_episodes and e + 1 >= max_episodes:
                    parked, park_tick[b] = True, t
                    count[b] = e + 1
                else:
                    e, age, st = e + 1, 0, -1
        if not parked:
            count[b] = e
        age_end[b], start_tick[b] = age, st
        records.append(rec)
    return dict(out, count=count, age_end=age_end, start_tick=start_tick, park_tick=park_tick, records=records)


def ring(sched, n_records):
    """-> [B, n_records, 4] int32: what episode_state()['records'] holds after the schedule's ticks -- episode e at entry e mod
    n_records, the last n_records of them: start_tick, length, outcome, start | variant << 16; entries never written are zero."""
    B = len(sched["records"])
    out = np.zeros((B, n_records, 4), np.int32)
    for b, rec in enumerate(sched["records"]):
        for e, (st, length, outcome, s, v) in enumerate(rec):
            out[b, e % n_records] = (st, length, outcome, s | (v << 16))
    return out


def stitch(fresh, sched):
    """A rollout with episodes composed from fresh ones.  fresh: dict name -> [S, V, Tf, B, ...], tick by tick what a fresh rollout
    from start s with variant v logs for robot b; sched: `schedule`'s dict.  -> dict name -> [T, B, ...]: entry (t, b) is
    fresh[start, variant, age, b] of the schedule (ticks that do not run the robot: zeros -- mask with sched['run'])."""
    s, v, a, run = sched["start"], sched["variant"], sched["age"], sched["run"]
    T, B = s.shape
    bb = np.broadcast_to(np.arange(B), (T, B))
    out = {}
    for name, f in fresh.items():
        f = np.asarray(f)
        if run.any() and a[run].max() >= f.shape[2]:
            raise ValueError(f"{name}: the fresh rollouts hold {f.shape[2]} ticks, the schedule asks for tick {int(a[run].max())}")
        g = f[s, v, np.minimum(a, f.shape[2] - 1), bb]
        g[~run] = 0
        out[name] = g
    return out


def ticks_run(park_tick, ticks, poll_every):
    """The ticks a call of `ticks` ticks runs with poll_every = P (the formula of include/irlosc.h).  park_tick [B]: the tick OF THE
    CALL on which each of its robots parks -- -1 for one that was parked before the call, any value >= ticks for one that does not
    park within it.  With D = max(park_tick) < ticks: min(ticks, (max(1, ceil((D + 1) / P)) + 1) P); else, or with P == 0: ticks."""
    P, T = int(poll_every), int(ticks)
    D = int(np.max(np.asarray(park_tick))) if len(np.atleast_1d(park_tick)) else -1
    if P == 0 or D >= T:
        return T
    m = max(1, -(-(D + 1) // P))
    return min(T, (m + 1) * P)
