#!/usr/bin/env python3
"""Rate of the device sample buffer (SampleBuffer.collect, tc_collect) at cfg3's shape, beside what a user writes in torch
today and beside a plain copy of the same bytes.  One process, one run, HIP events:

  (a) SampleBuffer.collect of a 128-step packed rollout of 4096 envs (frames of 5 x 64 x 64 / 8 = 2560 bytes), ring mode,
      columns maneuver (int32) and steer (float64), stride 1 and 2;
  (b) the torch formulation of the same call: the candidate mask from the done rows, `nonzero` (a host sync), `index_select`
      of the frames before the steps, `index_copy_` into the buffer, the columns likewise, the carry;
  (c) `copy_` of a tensor of as many bytes as (a) moves frames and columns.

The rows are synthetic (random frame bytes, episodes ending with probability 1/200 per row: the kernels' work does not depend
on what a frame shows).  (a) and (b) start from equal buffers and must leave equal buffers; the timed repeats alternate.
Reported: bytes read + written over the median time of each.  The one condition: (a) is not slower than (b).

    python tools/collect_rate.py [--reps 7] [--out profiles/r11/collect_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tinycarlo_amd import SampleBuffer  # noqa: E402

DEV = "cuda:0"
N, K, SHAPE = 4096, 128, (5, 64, 8)
CAP = 1 << 20  # (holds two stride-1 calls: every candidate of a call is written)


def make_rows(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    done = torch.rand((K, N), device=DEV, generator=g) < 1.0 / 200
    return {"obs": torch.randint(0, 256, (K, N) + SHAPE, dtype=torch.uint8, device=DEV, generator=g),
            "terminated": torch.zeros((K, N), dtype=torch.uint8, device=DEV), "truncated": done.to(torch.uint8),
            "maneuver": torch.randint(0, 4, (K, N), dtype=torch.int32, device=DEV, generator=g),
            "steer": torch.rand((K, N), dtype=torch.float64, device=DEV, generator=g)}


class TorchBuffer:
    """what a user writes today: the same rules with a mask, nonzero, index_select and index_copy_ (ring mode)"""

    def __init__(self, stride):
        self.stride = stride
        F = int(torch.tensor(SHAPE).prod())
        self.obs = torch.zeros((CAP, F), dtype=torch.uint8, device=DEV)
        self.ordinal = torch.full((CAP,), -1, dtype=torch.int64, device=DEV)
        self.env = torch.zeros(CAP, dtype=torch.int32, device=DEV)
        self.maneuver = torch.zeros(CAP, dtype=torch.int32, device=DEV)
        self.steer = torch.zeros(CAP, dtype=torch.float64, device=DEV)
        self.pending = torch.zeros(N, dtype=torch.bool, device=DEV)
        self.age = torch.zeros(N, dtype=torch.int64, device=DEV)
        self.last = torch.zeros((N, F), dtype=torch.uint8, device=DEV)
        self.next_ordinal = 0
        self.rows = torch.arange(K, device=DEV)[:, None]

    def collect(self, r):
        done = (r["terminated"] | r["truncated"]) != 0
        pend = torch.cat([self.pending[None], done[:-1]])                      # the row is a re-spawn row
        spawn_row = torch.where(pend, self.rows, -1).cummax(0).values          # the env's latest re-spawn row so far
        age = torch.where(spawn_row < 0, self.age[None] + self.rows, self.rows - spawn_row - 1)
        mask = ~pend & (age % self.stride == 0)
        sel0 = mask[0].nonzero().squeeze(1)                                    # host sync: candidates of row 0 (frames in `last`)
        sel = mask[1:].reshape(-1).nonzero().squeeze(1)                        # host sync: the rest, row-major = ordinal order
        c0, c = sel0.numel(), sel0.numel() + sel.numel()
        drop = max(0, c - CAP)                                                 # the highest ordinal wins a slot: the first lose
        man, steer = r["maneuver"].view(-1), r["steer"].view(-1)

        def put(idx, first, src, at):
            """candidates `first`, `first` + 1, ... of the call: frames src[idx], columns of the flat rows `at`"""
            skip = min(max(drop - first, 0), idx.numel())
            idx, at = idx[skip:], at[skip:]
            ords = self.next_ordinal + first + skip + torch.arange(idx.numel(), device=DEV)
            slots = ords % CAP
            self.obs.index_copy_(0, slots, src.index_select(0, idx))
            self.maneuver.index_copy_(0, slots, man.index_select(0, at))
            self.steer.index_copy_(0, slots, steer.index_select(0, at))
            self.env.index_copy_(0, slots, (at % N).to(torch.int32))
            self.ordinal.index_copy_(0, slots, ords)
        put(sel0, 0, self.last, sel0)                                          # row 0: the frame before is the carry
        put(sel, c0, r["obs"].view(K * N, -1), sel + N)                        # row k: obs[k - 1][n] is flat row (k - 1) * N + n
        self.next_ordinal += c
        self.last.copy_(r["obs"][-1].view(N, -1))
        self.age = torch.where(pend[-1], 0, age[-1] + 1)
        self.pending = done[-1]
        return c, c0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(stride, reps, rows):
    F = int(torch.tensor(SHAPE).prod())
    a = SampleBuffer(CAP, N, SHAPE, columns={"maneuver": torch.int32, "steer": torch.float64}, stride=stride, overflow="ring",
                     max_rows=K, device=DEV, packed=True)
    b = TorchBuffer(stride)
    first = torch.randint(0, 256, (N,) + SHAPE, dtype=torch.uint8, device=DEV)
    a.begin(first)
    b.last.copy_(first.view(N, -1))
    t = {"collect": [], "torch": [], "copy": []}
    cands = []
    for i in range(2 + reps):  # two warm-up rounds, then the timed ones; (a), (b), (c) in turn
        r = rows[i % len(rows)]
        before = int(a.counters[1])
        ta = timed(lambda: a.collect(r))
        c = int(a.counters[1]) - before
        got = []
        tb = timed(lambda: got.append(b.collect(r)))
        assert got[0][0] == c, (got, c)
        nbytes = c * (F + 4 + 8)  # the frames and columns (a) moves, once
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device=DEV), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        timed(lambda: dst.copy_(src))
        tc = timed(lambda: dst.copy_(src))
        del src, dst
        if i >= 2:
            t["collect"].append(ta)
            t["torch"].append(tb)
            t["copy"].append(tc)
            cands.append(c)
    same = bool(torch.equal(a.obs.view(CAP, -1), b.obs) and torch.equal(a.ordinal, b.ordinal) and torch.equal(a.env, b.env) and
                torch.equal(a.cols["maneuver"], b.maneuver) and torch.equal(a.cols["steer"], b.steer) and
                torch.equal(a.last.view(N, -1), b.last) and torch.equal(a.age.long(), b.age) and torch.equal(a.pending.bool(), b.pending))
    c = statistics.median(cands)
    # read + written: per written candidate its frame, columns, env and ordinal; the done rows; the carry frames
    moved = 2 * c * (F + 4 + 8) + c * (4 + 8) + 2 * K * N + 2 * N * F
    out = {"stride": stride, "candidates_per_call": c, "bytes_read_plus_written": moved, "buffers_equal": same}
    for k, v in t.items():
        ms = statistics.median(v)
        nb = 2 * c * (F + 4 + 8) if k == "copy" else moved
        out[k] = {"ms": round(ms, 4), "GBs": round(nb / ms / 1e6, 1), "spread": round((max(v) - min(v)) / ms, 3), "ms_all": [round(x, 4) for x in v]}
    out["collect_over_torch_time"] = round(out["collect"]["ms"] / out["torch"]["ms"], 4)
    out["collect_share_of_copy_rate"] = round(out["collect"]["GBs"] / out["copy"]["GBs"], 4)
    out["condition_met"] = bool(same and out["collect"]["ms"] <= out["torch"]["ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    rows = [make_rows(s) for s in range(2)]
    res = {"tool": "tools/collect_rate.py", "device": torch.cuda.get_device_name(0), "envs": N, "steps_per_call": K,
           "frame_bytes": int(torch.tensor(SHAPE).prod()), "capacity": CAP, "overflow": "ring", "reps": max(args.reps, 3)}
    for stride in (1, 2):
        res[f"stride{stride}"] = measure(stride, max(args.reps, 3), rows)
        torch.cuda.empty_cache()
    res["condition_met"] = all(res[f"stride{s}"]["condition_met"] for s in (1, 2))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
