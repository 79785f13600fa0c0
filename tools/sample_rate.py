#!/usr/bin/env python3
"""Rate of frame-history samples out of the device sample buffer (SampleBuffer.sample(history=T): tc_history_resolve, then
tc_gather_frames for byte frames or tc_unpack_bits for packed ones) at cfg3's frame, beside the torch formulation of the same
rules.  One process, one run, HIP events:

  (a) buf.sample(idx, torch.float16, history=T) for B = 256 samples, T in {1, 10};
  (b) what a user writes in torch: T - 1 rounds of prev / slot / ordinal indexing for the slot table, then index_select,
      .to(float16), / 255 and a mask for byte frames, or unpack_obs through the table for packed ones.  At T = 1 this is the
      three-op form a buffer without links uses.

The buffer is a ring of 65536 slots filled from three synthetic 16-step calls of 4096 envs (random frame bytes, episodes
ending with probability 1/50 per row), packed frames (5 x 64 x 64 / 8 = 2560 bytes) and byte frames (5 x 64 x 64 = 20480
bytes), without next frames.  (a) and (b) must be equal; the timed repeats alternate.  Reported per form: the median time,
bytes read + written and their rate, and the spread of the repeats.  Nothing is required of the numbers.

    python tools/sample_rate.py [--reps 7] [--out profiles/r14/sample_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tinycarlo_amd import SampleBuffer, unpack_obs  # noqa: E402

DEV = "cuda:0"
N, K, CALLS, CAP, B = 4096, 16, 3, 1 << 16, 256
SHAPES = {"packed": (5, 64, 8), "byte": (5, 64, 64)}
T_MAX = 10


def fill(buf, shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf.begin(torch.randint(0, 256, (N,) + shape, dtype=torch.uint8, device=DEV, generator=g))
    for _ in range(CALLS):
        rows = {"obs": torch.randint(0, 256, (K, N) + shape, dtype=torch.uint8, device=DEV, generator=g),
                "truncated": (torch.rand((K, N), device=DEV, generator=g) < 1.0 / 50).to(torch.uint8)}
        buf.collect(rows)
        del rows
    torch.cuda.synchronize()


def torch_slots(buf, idx, T):
    """the resolve walk of a ring buffer in torch ops: [B, T], -1 behind the end of a history"""
    cur, alive, out = idx, buf.ordinal[idx] >= 0, [idx]
    for _ in range(T - 1):
        p = buf.prev[cur.clamp(min=0)]
        q = torch.where(p < buf.capacity, p, p % buf.capacity).clamp(min=0)
        alive = alive & (p >= 0) & (buf.ordinal[q] == p)
        cur = torch.where(alive, q, -1)
        out.append(cur)
    return torch.stack(out, 1)


def torch_sample(buf, idx, T, dtype):
    slots = torch_slots(buf, idx, T)
    flat = slots.reshape(-1)
    if buf.packed:
        obs = unpack_obs(buf.obs, dtype, index=flat)
    else:
        obs = buf.obs.index_select(0, flat.clamp(min=0)).to(dtype) / 255
        if T > 1:
            obs = obs * (flat >= 0).to(dtype).view(-1, 1, 1, 1)
    return slots, obs.view((len(idx), T) + tuple(obs.shape[1:]))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(kind, reps):
    shape = SHAPES[kind]
    buf = SampleBuffer(CAP, N, shape, stride=1, overflow="ring", max_rows=K, device=DEV, packed=kind == "packed", history=T_MAX)
    fill(buf, shape, 1)
    pixels = 5 * 64 * 64
    res = {"frame_bytes": buf.frame_bytes, "filled": len(buf)}
    g = torch.Generator(device=DEV).manual_seed(2)
    for T in (1, T_MAX):
        t = {"sample": [], "torch": []}
        equal, found = True, []
        for i in range(2 + reps):  # two warm-up rounds, then the timed ones; (a) and (b) in turn, a fresh index per round
            idx = buf.sample_index(B, generator=g)
            got, ref = [], []
            ta = timed(lambda: got.append(buf.sample(idx, torch.float16, history=T)))
            tb = timed(lambda: ref.append(torch_sample(buf, idx, T, torch.float16)))
            s, (slots, obs) = got[0], ref[0]
            equal = equal and bool(torch.equal(s["slots"], slots) and torch.equal(s["obs"].reshape(obs.shape), obs))
            if i >= 2:
                t["sample"].append(ta)
                t["torch"].append(tb)
                found.append(int(s["valid"].sum()))
        n = statistics.median(found)
        moved = n * buf.frame_bytes + B * T * pixels * 2  # frames found, read once; every output frame written once as f16
        out = {"frames_found_of": [n, B * T], "bytes_read_plus_written": moved, "equal": equal}
        for k, v in t.items():
            ms = statistics.median(v)
            out[k] = {"ms": round(ms, 4), "GBs": round(moved / ms / 1e6, 1), "spread": round((max(v) - min(v)) / ms, 3),
                      "ms_all": [round(x, 4) for x in v]}
        out["sample_over_torch_time"] = round(out["sample"]["ms"] / out["torch"]["ms"], 4)
        res[f"T{T}"] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    res = {"tool": "tools/sample_rate.py", "device": torch.cuda.get_device_name(0), "envs": N, "steps_per_call": K, "calls": CALLS,
           "capacity": CAP, "overflow": "ring", "batch": B, "dtype": "float16", "reps": max(args.reps, 3),
           "not_measured": "next frames, pad='edge', stop / random mode, other dtypes and batch sizes, a cold first call"}
    for kind in SHAPES:
        res[kind] = measure(kind, max(args.reps, 3))
        torch.cuda.empty_cache()
    res["all_equal"] = all(res[k][f"T{T}"]["equal"] for k in SHAPES for T in (1, T_MAX))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not res["all_equal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
