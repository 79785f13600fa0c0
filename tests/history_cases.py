"""What the frame-history tests share (tests/test_history_cpu.py, tests/test_gpu_history.py): the dedicated cases on top of
tests/collect_cases.py, reference states with links, a trace of the links worked out apart from collect_reference, and the
four counts the non-vacuity checks ask for.  Reference states are computed once per case and handed out as they are: no
test changes one."""
import numpy as np

import collect_cases as cc
from tinycarlo_amd import collect as col

TS = (1, 2, 4, 7, 19)
PADS = ("zero", "edge")


def dedicated_cases():
    """six cases in which full, start-cut and lost-predecessor histories and links across call borders all occur"""
    return [cc.Case(400, N, 20, (12, 5, 1), cap, mode, stride, True)
            for (N, cap, stride) in ((70, 400, 1), (63, 300, 2), (300, 1500, 1)) for mode in ("ring", "random")]


def new_state(case, fill=0xFF):
    st = col.reference_state(case.capacity, case.N, (case.F,), cc.COLUMNS, case.next_obs, fill=fill, history=True)
    col.reference_begin(st, case.begin_obs, case.begin_pending)
    return st


_STATES = {}


def _states(case):
    key = (case.id, case.seed)
    if key in _STATES:
        return _STATES[key]
    out, st = [], new_state(case)
    for rows in case.calls:
        col.collect_reference(st, rows, case.stride, case.overflow, case.seed)
        out.append({k: (v.copy() if isinstance(v, np.ndarray) else dict((n, c.copy()) for n, c in v.items()) if isinstance(v, dict) else v)
                    for k, v in st.items()})
    _STATES[key] = out
    return out


def reference(case, upto=None):
    """the reference state with links after the first `upto` calls (all by default); shared, not to be changed"""
    return _states(case)[(len(case.Ks) if upto is None else upto) - 1]


def link_trace(case):
    """prev [capacity] and chain [N] after the case's calls, from Case.trace()'s candidates and the done flags alone: per env
    the previous candidate of the running episode; a slot ends up with the link of the highest ordinal that went to it."""
    cands, _ = case.trace()
    pending = case.begin_pending.astype(bool).copy()
    chain = np.full(case.N, -1, dtype=np.int64)
    holder = {}  # slot -> (ordinal, link)
    for rows, cs in zip(case.calls, cands):
        done = (rows["terminated"] | rows["truncated"]) != 0
        by_row = {(k, n): (o, slot) for k, n, o, slot in cs}
        for k in range(done.shape[0]):
            for n in range(case.N):
                if pending[n]:
                    chain[n] = -1
                elif (k, n) in by_row:
                    o, slot = by_row[(k, n)]
                    if slot >= 0 and (slot not in holder or holder[slot][0] < o):
                        holder[slot] = (o, int(chain[n]))
                    chain[n] = o
                pending[n] = done[k, n]
    prev = np.full(case.capacity, -1, dtype=np.int64)
    for slot, (_, link) in holder.items():
        prev[slot] = link
    return prev, chain


def sample_index(st):
    """every filled slot, then -1, capacity, and an empty slot where there is one"""
    filled = np.nonzero(st["ordinal"] >= 0)[0]
    extra = [-1, len(st["ordinal"])] + [int(s) for s in np.nonzero(st["ordinal"] < 0)[0][:1]]
    return np.concatenate([filled, np.array(extra, dtype=np.int64)]).astype(np.int64)


def call_starts(case):
    """the first ordinal of every call"""
    cands, _ = case.trace()
    return np.cumsum([0] + [len(c) for c in cands])[:-1]


def categories(case, st, T):
    """over the filled slots of reference state `st` (after all calls): histories that are full, cut by an episode start,
    cut by a lost predecessor, and histories with a followed link that crosses a call border"""
    return count_kinds(st, T, case.overflow, case.seed, call_starts(case))


def count_kinds(st, T, overflow, seed, starts):
    """`categories` for any reference state with links; starts: the first ordinal of every call"""
    filled = np.nonzero(st["ordinal"] >= 0)[0]
    h = col.history_reference(st, filled, T, "zero", overflow, seed)
    full = start = lost = crossing = 0
    for b in range(len(filled)):
        v = int(h["valid"][b])
        assert v >= 1
        if v == T:
            full += 1
        elif st["prev"][h["slots"][b, v - 1]] < 0:
            start += 1
        else:
            lost += 1
        o = st["ordinal"][h["slots"][b, :v]]
        assert (np.diff(o) < 0).all()
        call = np.searchsorted(starts, o, side="right")
        crossing += bool((np.diff(call) != 0).any())
    return dict(full=full, start=start, lost=lost, crossing=crossing, samples=len(filled))
