#!/usr/bin/env python3
"""Cost of the episode accounting on cfg3 (4096 envs, simple_layout, 64x64 'classes', autoreset): env-steps/s for

    off        no episode buffers installed (the default kernels)
    track      track_episodes(): length / return / statistics kept by the kernels with the episode bit, no limit
    limit      set_time_limit(256) with staggered starts (env i begins at length i * 256 / N): a steady trickle of
               time-limit truncations and re-spawns instead of all envs at once

each in 128-step streamed calls (step_multi with observation rows; track / limit also write the two episode rows) and
in the closed step() loop (tc_step), each with the draw-list statistics of its last frames (a time limit re-spawns cars,
which changes what the cameras see, and so the frame work).

    python tools/bench_episodes.py [--envs 4096] [--calls 4] [--steps 256] [--reps 2]
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from tinycarlo_amd.config import bundled_config  # noqa: E402
from tinycarlo_amd.vec_env import TinyCarloVecEnv  # noqa: E402


def cfg3():
    path = bundled_config("config_simple_layout.yaml")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = [64, 64]
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


def make(case, n):
    env = TinyCarloVecEnv(cfg3(), num_envs=n, device="cuda:0", autoreset=True, spawn_queue_len=64)
    if case == "track":
        env.track_episodes()
    elif case == "limit":
        env.set_time_limit(256)
    env.reset(seed=0)
    if case == "limit":  # staggered starts: not all envs at the limit on the same step
        env.episode_stats["length"].copy_((torch.arange(n, device="cuda:0") * 256 // n).to(torch.int32))
    return env


def actions(n, k, device="cuda:0", seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    cc = torch.stack([torch.rand((k, n), generator=g) * 0.7 + 0.3, torch.rand((k, n), generator=g) * 2 - 1], dim=2)
    man = torch.randint(0, 4, (k, n), generator=g, dtype=torch.int32)
    return cc.to(torch.float32).to(device).contiguous(), man.to(device).contiguous()


def streamed(env, calls, M=128):
    n = env.num_envs
    cc, man = actions(n, M)
    keys = ("obs", "reward", "terminated", "truncated")
    if env.episode_stats is not None:
        keys += ("episode_length", "episode_return")
    roll = env.alloc_rollout(M, keys=keys)
    pc = env.prepare_step_multi(cc, man, roll)
    pc()  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        pc()
    torch.cuda.synchronize()
    return n * M * calls / (time.perf_counter() - t0)


def closed_loop(env, steps):
    n = env.num_envs
    cc, man = actions(n, 64, seed=1)
    for k in range(8):
        env.step_device(cc[k], man[k])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        env.step_device(cc[k % 64], man[k % 64])
    torch.cuda.synchronize()
    return n * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=4, help="128-step streamed calls per measurement")
    ap.add_argument("--steps", type=int, default=256, help="tc_step calls per closed-loop measurement")
    ap.add_argument("--reps", type=int, default=2, help="repetitions, cases interleaved")
    a = ap.parse_args()
    res = {c: {"streamed": [], "closed_loop": []} for c in ("off", "track", "limit")}
    stats = {}
    for _ in range(a.reps):
        for case in res:
            env = make(case, a.envs)
            res[case]["streamed"].append(streamed(env, a.calls))
            stats[case + "_streamed"] = env.draw_list_stats()
            res[case]["closed_loop"].append(closed_loop(env, a.steps))
            stats[case + "_closed_loop"] = env.draw_list_stats()
            if case != "off":
                stats[case + "_episodes_finished"] = int(env.episode_stats["count"].sum())
            env.close()
    out = {"workload": "cfg3", "envs": a.envs, "metric": "env_steps_per_s"}
    for case, r in res.items():
        for mode, v in r.items():
            out[f"{case}_{mode}"] = float(np.median(v))
            out[f"{case}_{mode}_all"] = [round(x) for x in v]
    for mode in ("streamed", "closed_loop"):
        for case in ("track", "limit"):
            out[f"{case}_vs_off_{mode}"] = out[f"{case}_{mode}"] / out[f"off_{mode}"]
    out["draw_list_stats"] = stats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
