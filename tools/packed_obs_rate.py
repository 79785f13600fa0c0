#!/usr/bin/env python3
"""Byte class masks against bit-packed ones (obs_packing="bits"), and the rate of the unpack kernel.

One process, cfg3's and cfg4's shapes of bench.py at 4096 envs.  Per shape two envs, byte and packed, same seed, same
actions (bench.py's distribution), both taken through bench.py's pre-roll so that the timed calls start from its start
state.  Then 64-step step_multi calls with every frame kept, timed byte, packed, byte, packed, ... with a device
synchronise inside every timed window.  Reported per format: env-steps/s, bytes of frames per second, and the spread
(max - min) / median of its own repeats.  The one condition: packed is not slower than byte by more than byte's spread.

Then tc_unpack_bits on a cfg4 rollout (64 steps x 4096 envs), u8 and f16, bytes read + written over device-event time,
beside the fill ceiling of tools/fill_rate.py.

    python tools/packed_obs_rate.py [--rounds 7] [--calls 4] [--out profiles/r07/packed_obs_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import PREROLL_STEPS, WORKLOADS, gen_actions, make_config  # noqa: E402
from tinycarlo_amd import unpack_obs  # noqa: E402
from tinycarlo_amd.vec_env import TinyCarloVecEnv  # noqa: E402

FILL_CEILING_GBS = 6900.0  # tools/fill_rate.py on this GPU: what a pure store stream reaches
K = 64


def make(cfg, n, packing):
    env = TinyCarloVecEnv(cfg, num_envs=n, device="cuda:0", autoreset=True, spawn_queue_len=64, obs_packing=packing)
    env.reset(seed=0)
    roll = env.alloc_rollout(K, keys=("obs", "reward", "terminated", "truncated"))
    env.reserve_steps(K)
    return env, roll


def shape_rates(name, rounds, calls):
    w = WORKLOADS[name]
    cfg, n = make_config(w), w["envs"]
    period = 1024
    cc, man = gen_actions(n, period, seed=0, device="cuda:0")
    envs = {"byte": make(cfg, n, None), "packed": make(cfg, n, "bits")}
    prepared = {f: [e.prepare_step_multi(cc[i:i + K], man[i:i + K], rollout=r) for i in range(0, period, K)]
                for f, (e, r) in envs.items()}
    pos = {f: 0 for f in envs}

    def issue(f, count):
        for _ in range(count):
            prepared[f][pos[f] % len(prepared[f])]()
            pos[f] += 1

    for f, (e, _) in envs.items():  # bench.py's pre-roll: PREROLL_STEPS steps, the spawn queues topped up two thirds in
        issue(f, PREROLL_STEPS * 2 // 3 // K)
        torch.cuda.synchronize()
        e.top_up_spawn_queue()
        issue(f, PREROLL_STEPS // K - PREROLL_STEPS * 2 // 3 // K)
        torch.cuda.synchronize()
        e.top_up_spawn_queue()
    same_state = all(torch.equal(envs["byte"][0].state[k], envs["packed"][0].state[k]) for k in ("x", "y", "theta"))
    times = {f: [] for f in envs}
    for f in envs:  # warm-up of the timed form
        issue(f, calls)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for f in ("byte", "packed"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            issue(f, calls)
            torch.cuda.synchronize()
            times[f].append(time.perf_counter() - t0)
    out = {"envs": n, "steps_per_call": K, "calls_per_repeat": calls, "repeats": rounds, "same_state_after_preroll": bool(same_state)}
    for f, (e, r) in envs.items():
        med = statistics.median(times[f])
        steps = n * K * calls
        out[f] = {"env_steps_per_s": steps / med, "frame_bytes_per_s": steps * e.obs_bytes_per_env / med,
                  "obs_bytes_per_env": e.obs_bytes_per_env, "spread": (max(times[f]) - min(times[f])) / med,
                  "repeat_ms": [round(t * 1e3, 3) for t in times[f]], "kernel": e.launch_info(K)["kernel"]}
    slower = out["byte"]["env_steps_per_s"] / out["packed"]["env_steps_per_s"] - 1.0  # > 0: packed is slower
    out["packed_slower_by"] = slower
    out["condition_met"] = bool(slower <= out["byte"]["spread"])
    packed_roll = envs["packed"][1]["obs"].clone() if name == "cfg4" else None
    for e, _ in envs.values():
        e.close()
    return out, packed_roll


def unpack_rates(packed, reps=10):
    out = {"shape": list(packed.shape), "fill_ceiling_GBs": FILL_CEILING_GBS}
    for dtype, key in ((torch.uint8, "u8"), (torch.float16, "f16")):
        dst = torch.empty(tuple(packed.shape[:-1]) + (packed.shape[-1] * 8,), dtype=dtype, device=packed.device)
        for _ in range(2):
            unpack_obs(packed, dtype, out=dst)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            unpack_obs(packed, dtype, out=dst)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        nbytes = packed.numel() + dst.numel() * dst.element_size()
        out[key] = {"ms": ms, "GBs": nbytes / ms / 1e6, "bytes_read": packed.numel(), "bytes_written": dst.numel() * dst.element_size()}
        del dst
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="repeats per format and shape (>= 5)")
    ap.add_argument("--calls", type=int, default=4, help="64-step calls per repeat")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    res = {"tool": "tools/packed_obs_rate.py", "device": torch.cuda.get_device_name(0)}
    packed_roll = None
    for name in ("cfg3", "cfg4"):
        res[name], pr = shape_rates(name, max(args.rounds, 5), args.calls)
        packed_roll = pr if pr is not None else packed_roll
        torch.cuda.empty_cache()
    res["unpack_cfg4_rollout"] = unpack_rates(packed_roll)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
