#!/usr/bin/env python3
"""Cost of per-env cars on cfg3 (4096 envs, simple_layout, 64x64 'classes', autoreset): env-steps/s for

    shared     the shared car (the default kernels)
    rows       per-env rows set to the config's values (the per-env-car kernels doing the same arithmetic: the pure cost)
    random     per-episode randomisation of all eight columns (every re-spawn draws a new car)

each in 128-step streamed calls (step_multi with observation rows) and in the closed step() loop (tc_step), each with
the draw-list statistics of its last frames (randomised wheelbases change what the camera sees, and so the frame work).

    python tools/bench_car_per_env.py [--envs 4096] [--calls 4] [--steps 256] [--reps 2]
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
    p = env.car_params
    if case == "rows":
        env.set_env_cars(wheelbase=p.wheelbase)
    elif case == "random":
        env.randomize_cars({"wheelbase": (0.8 * p.wheelbase, 1.2 * p.wheelbase),
                            "track_width": (0.8 * p.track_width, 1.2 * p.track_width),
                            "max_velocity": (0.8 * p.max_velocity, 1.2 * p.max_velocity),
                            "max_steering_angle": (0.8 * p.max_steering_angle, 1.2 * p.max_steering_angle),
                            "steering_speed": (0.8 * p.steering_speed, 1.2 * p.steering_speed),
                            "max_acceleration": (0.8 * p.max_acceleration, 1.2 * p.max_acceleration),
                            "max_deceleration": (0.8 * p.max_deceleration, 1.2 * p.max_deceleration),
                            "steering_shift": (-0.02, 0.02)}, seed=1)
    env.reset(seed=0)
    return env


def actions(n, k, device="cuda:0", seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    cc = torch.stack([torch.rand((k, n), generator=g) * 0.7 + 0.3, torch.rand((k, n), generator=g) * 2 - 1], dim=2)
    man = torch.randint(0, 4, (k, n), generator=g, dtype=torch.int32)
    return cc.to(torch.float32).to(device).contiguous(), man.to(device).contiguous()


def streamed(env, calls, M=128):
    n = env.num_envs
    cc, man = actions(n, M)
    roll = env.alloc_rollout(M, keys=("obs", "reward", "terminated", "truncated"))
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
    res = {c: {"streamed": [], "closed_loop": []} for c in ("shared", "rows", "random")}
    stats = {}
    for _ in range(a.reps):
        for case in res:
            env = make(case, a.envs)
            res[case]["streamed"].append(streamed(env, a.calls))
            stats[case + "_streamed"] = env.draw_list_stats()
            res[case]["closed_loop"].append(closed_loop(env, a.steps))
            stats[case + "_closed_loop"] = env.draw_list_stats()
            if case == "random":
                stats["random_episodes_drawn"] = int(env.car_episode.sum())
            env.close()
    out = {"workload": "cfg3", "envs": a.envs, "metric": "env_steps_per_s"}
    for case, r in res.items():
        for mode, v in r.items():
            out[f"{case}_{mode}"] = float(np.median(v))
            out[f"{case}_{mode}_all"] = [round(x) for x in v]
    for mode in ("streamed", "closed_loop"):
        for case in ("rows", "random"):
            out[f"{case}_vs_shared_{mode}"] = out[f"{case}_{mode}"] / out[f"shared_{mode}"]
    out["draw_list_stats"] = stats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
