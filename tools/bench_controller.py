#!/usr/bin/env python3
"""What the built-in controller buys and costs on cfg3 (4096 envs, simple_layout, 64x64 'classes', device spawns, the
wrappers of examples/stanley_batched.py): env-steps/s for

    torch_loop   (a) the closed loop of examples/stanley_batched.py: per step the Stanley law in torch + one tc_step
    drive        (b) set_controller() + drive() in 128-step streamed calls, frames and the label rows into a rollout
    replay       (c) plain step_multi replaying the actions (b) recorded (speed, steer rows), so both draw the same frames

three repetitions, cases interleaved, medians reported, with two ratios: drive / torch_loop (the point of the feature)
and drive / replay (the controller's own cost), and the draw-list statistics of each line's last frames.

    python tools/bench_controller.py [--envs 4096] [--calls 4] [--steps 512] [--reps 3]
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
from tinycarlo_amd.wrapper import CrashTerminationWrapper, CTESparseRewardWrapper, CTETerminationWrapper  # noqa: E402

GAIN, SPEED, M = 4.0, 0.4, 128


def cfg3():
    path = bundled_config("config_simple_layout.yaml")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = [64, 64]
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


def make(n):
    vec = TinyCarloVecEnv(cfg3(), num_envs=n, device="cuda:0", autoreset=True, spawn="device")
    env = CrashTerminationWrapper(CTETerminationWrapper(CTESparseRewardWrapper(vec, 0.01), 0.07, number_of_steps=5))
    env.reset(seed=2)
    return vec


def torch_loop(vec, steps):
    n = vec.num_envs
    max_steer = np.radians(vec.car_params.max_steering_angle)
    cc = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
    cc[:, 0] = SPEED
    man = torch.full((n,), 3, dtype=torch.int32, device="cuda:0")

    def one():
        cte, he = vec.out["cte"], vec.out["heading_error"]
        cc[:, 1] = (he + torch.atan2(GAIN * cte, torch.full_like(cte, SPEED))) / max_steer
        vec.step_device(cc, man)
    for _ in range(8):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    return n * steps / (time.perf_counter() - t0)


def drive(vec, calls):
    """-> (rate, the actions of every call, warm-up included, as step_multi inputs, maneuver rows)"""
    n = vec.num_envs
    vec.set_controller(k=GAIN, speed=SPEED)
    man = torch.full((M, n), 3, dtype=torch.int32, device="cuda:0")
    roll = vec.alloc_rollout(M, keys=("obs", "reward", "terminated", "truncated", "steer"))
    pc = vec.prepare_drive(man, roll)
    pc()  # warm-up
    steer = [roll["steer"].clone()]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        pc()
        steer.append(roll["steer"].clone())  # (a 4 MB device copy per 128-step call: inside the timed region, against (b))
    torch.cuda.synchronize()
    rate = n * M * calls / (time.perf_counter() - t0)
    ccs = [torch.stack([torch.full_like(s, SPEED), s], dim=2).contiguous() for s in steer]
    return rate, ccs, man


def replay(vec, calls, ccs, man):
    """the same env from the same reset, call by call the actions `drive` applied: the same states and frames"""
    n = vec.num_envs
    roll = vec.alloc_rollout(M, keys=("obs", "reward", "terminated", "truncated"))
    pcs = [vec.prepare_step_multi(cc, man, roll) for cc in ccs]
    pcs[0]()  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for pc in pcs[1:]:
        pc()
    torch.cuda.synchronize()
    return n * M * calls / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=4, help="128-step calls per measurement of drive / replay")
    ap.add_argument("--steps", type=int, default=512, help="steps per measurement of the torch loop")
    ap.add_argument("--reps", type=int, default=3, help="repetitions, cases interleaved")
    a = ap.parse_args()
    res = {"torch_loop": [], "drive": [], "replay": []}
    stats, kernels = {}, {}
    for _ in range(a.reps):
        vec = make(a.envs)
        kernels["torch_loop"] = vec.launch_info(1)["kernel"]
        res["torch_loop"].append(torch_loop(vec, a.steps))
        stats["torch_loop"] = vec.draw_list_stats()
        vec.close()
        vec = make(a.envs)
        rate, ccs, man = drive(vec, a.calls)
        kernels["drive"] = vec.launch_info(M)["kernel"]
        res["drive"].append(rate)
        stats["drive"] = vec.draw_list_stats()
        vec.close()
        vec = make(a.envs)
        kernels["replay"] = vec.launch_info(M)["kernel"]
        res["replay"].append(replay(vec, a.calls, ccs, man))
        stats["replay"] = vec.draw_list_stats()
        vec.close()
    out = {"workload": "cfg3 + stanley_batched wrappers", "envs": a.envs, "metric": "env_steps_per_s", "steps_per_call": M,
           "kernels": kernels}
    for case, v in res.items():
        out[case] = float(np.median(v))
        out[case + "_all"] = [round(x) for x in v]
    out["drive_vs_torch_loop"] = out["drive"] / out["torch_loop"]
    out["drive_vs_replay"] = out["drive"] / out["replay"]
    out["draw_list_stats"] = stats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
