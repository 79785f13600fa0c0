"""Seeded synthetic calls for the sample buffer's tests (tests/test_collect_cpu.py, tests/test_gpu_collect.py): no env, the
rows are made up.  Every frame's bytes encode (call, k, n), and so does every column value, so a frame or a value paired
with the wrong row is visible.  Done flags are random plus forced ones, so that re-spawn rows fall inside calls and envs are
pending across call borders whatever N is."""
import itertools

import numpy as np

from tinycarlo_amd import collect as col

BIG = 1 << 14   # a capacity above everything a case collects (300 envs x 18 rows = 5400 rows at the most)
SMALL = 97
COLUMNS = {"flag": np.uint8, "maneuver": np.int32, "steer": np.float64}  # 1, 4 and 8 bytes
NS, FS = (1, 63, 70, 300), (4, 20, 2560, 12288)
KS = ((12, 5, 1), (5, 12, 1), (1, 12, 5), (12, 1, 5))  # three consecutive calls; every K of {1, 5, 12} in every case
MODES = ("stop", "ring", "random")
BEGIN = 255  # the `call` number of the frames given to begin()


def frames(call, k, n, F):
    """uint8 [..., F] for broadcast (call, k, n): 32-bit word j of a frame is call * 1000003 + k * 10007 + n * 101 + j * 7919"""
    call, k, n = np.broadcast_arrays(np.asarray(call, dtype=np.uint32), np.asarray(k, dtype=np.uint32), np.asarray(n, dtype=np.uint32))
    j = np.arange(F // 4, dtype=np.uint32)
    w = (call[..., None] * np.uint32(1000003) + k[..., None] * np.uint32(10007) + n[..., None] * np.uint32(101) + j * np.uint32(7919))
    return np.ascontiguousarray(w.astype("<u4")).view(np.uint8).reshape(call.shape + (F,))


def make_call(seed, call, K, N, F):
    """the rows of one call: obs, terminated, truncated and the three columns"""
    rng = np.random.default_rng([seed, call])
    kk, nn = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    done = rng.random((K, N)) < 0.1
    done[K - 1, (np.arange(N) + call) % 4 == 0] = True       # pending across the border behind this call
    if K >= 5:
        done[1, (np.arange(N) + call) % 2 == 0] = True       # a re-spawn row at k = 2
    kind = rng.integers(0, 3, (K, N))                        # terminated, truncated or both
    code = call * 100000 + kk * 1000 + nn
    return {"obs": frames(call, kk, nn, F), "terminated": (done & (kind != 1)).astype(np.uint8),
            "truncated": (done & (kind != 0)).astype(np.uint8), "flag": ((call * 7 + kk * 3 + nn) & 0xFF).astype(np.uint8),
            "maneuver": code.astype(np.int32), "steer": code.astype(np.float64) + 0.5}


class Case:
    def __init__(self, seed, N, F, Ks, capacity, overflow, stride, next_obs):
        self.seed, self.N, self.F, self.Ks, self.capacity = seed, N, F, tuple(Ks), capacity
        self.overflow, self.stride, self.next_obs = overflow, stride, next_obs
        self.id = f"N{N}-F{F}-K{'_'.join(map(str, Ks))}-cap{capacity}-{overflow}-s{stride}-{'x1' if next_obs else 'x'}"
        self._calls = None

    @property
    def calls(self):
        if self._calls is None:
            self._calls = [make_call(self.seed, c, K, self.N, self.F) for c, K in enumerate(self.Ks)]
        return self._calls

    @property
    def begin_obs(self):
        return frames(BEGIN, 0, np.arange(self.N), self.F)

    @property
    def begin_pending(self):
        return (np.arange(self.N) % 5 == 3).astype(np.uint8)  # some envs start with a re-spawn row

    def new_state(self, fill=0xFF):
        st = col.reference_state(self.capacity, self.N, (self.F,), COLUMNS, self.next_obs, fill=fill)
        col.reference_begin(st, self.begin_obs, self.begin_pending)
        return st

    def reference(self, upto=None, repeat=1):
        """the reference state after the first `upto` calls (all by default), each applied `repeat` times in a row"""
        st = self.new_state()
        for rows in self.calls[:upto]:
            for _ in range(repeat):
                col.collect_reference(st, rows, self.stride, self.overflow, self.seed)
        return st

    def trace(self):
        """What the rules do with the case, worked out apart from collect_reference (rules 1-3 over the done flags alone):
        per call the (k, n, ordinal, slot) of its candidates, plus the counts the non-vacuity checks ask for."""
        pending, age = self.begin_pending.astype(bool), np.zeros(self.N, dtype=np.int64)
        o, out = 0, []
        stats = dict(respawn_inside=0, pending_border=0, skipped=0, overwritten=0, dropped=0, same_call_clash=0, max_call=0)
        held = set()
        for rows in self.calls:
            done = (rows["terminated"] | rows["truncated"]) != 0
            K = done.shape[0]
            cands, slots_here = [], set()
            stats["pending_border"] += int(pending.sum())
            for k in range(K):
                for n in range(self.N):
                    if pending[n]:
                        age[n] = 0
                        stats["respawn_inside"] += k > 0
                    else:
                        if age[n] % self.stride == 0:
                            slot = o if o < self.capacity else {"stop": -1, "ring": o % self.capacity,
                                                                 "random": int(col.draw_replace_slot(self.seed, o, self.capacity))}[self.overflow]
                            cands.append((k, n, o, slot))
                            stats["dropped"] += slot < 0
                            stats["overwritten"] += slot in held
                            stats["same_call_clash"] += slot in slots_here
                            if slot >= 0:
                                held.add(slot)
                                slots_here.add(slot)
                            o += 1
                        else:
                            stats["skipped"] += 1
                        age[n] += 1
                    pending[n] = done[k, n]
            stats["max_call"] = max(stats["max_call"], len(cands))
            out.append(cands)
        return out, stats


_COMBOS = [(m, c, s, x) for x in (False, True) for s in (1, 2) for c in (SMALL, BIG) for m in MODES]  # 24, the mode fastest
_NF = list(itertools.product(NS, FS))                                                                 # 16


def gpu_cases():
    """48 cases: every (N, F) pair with every mode once, every (mode, capacity, stride, next_obs) combination twice"""
    out = []
    for i in range(48):
        (N, F), (m, c, s, x) = _NF[i % 16], _COMBOS[i % 24]
        out.append(Case(100 + i, N, F, KS[i % 4], c, m, s, x))
    return out


def can_overflow(case):
    """A capacity above everything collected cannot overflow by construction, and one env's 18 rows do not fill 97 slots:
    the overflow conditions are asked of every other case."""
    return case.capacity == SMALL and case.N > 1
