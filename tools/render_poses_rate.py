#!/usr/bin/env python3
"""What deferred frames cost (TinyCarloVecEnv.render_rollout / render_poses, tc_render_poses) beside drawing every frame inside
the K-step call, at cfg3's shape (4096 envs, simple_layout, 64x64 classes) and cfg4's (knuffingen, 128x128 classes), K = 128,
the benchmark's actions after the benchmark's pre-roll (bench.py: gen_actions, PREROLL_STEPS).  One process, HIP events, a
warm-up round, then `--reps` rounds (at least 7) in which the forms alternate:

  (A) step_multi with an "obs" rollout                                   today's path, the baseline
  (B) step_multi with x / y / theta rows only + render_rollout of all K x N rows
  (C) (B) with every 2nd, 4th and 8th row (render_rollout(index=...))
  (D) render_poses of 256 random rows of the last call                   the replay-sample case, time per call

Every form steps the same env on from where the one before left it (the state is whatever the actions made it: the
forms see the same distribution of views, not the same frames).  Reported per form: median, min and max milliseconds per
call, and for (A)-(C) the env-steps per second of the median.  Nothing here is a threshold.

    python tools/render_poses_rate.py [--reps 7] [--shapes cfg3,cfg4] [--out profiles/render_poses/rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the benchmark's configs, actions and pre-roll length)
from tinycarlo_amd.vec_env import TinyCarloVecEnv  # noqa: E402

DEV = "cuda:0"
K = 128
STRIDES = (2, 4, 8)
SAMPLE = 256


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(name, reps):
    w = bench.WORKLOADS[name]
    n = w["envs"]
    env = TinyCarloVecEnv(bench.make_config(w), num_envs=n, device=DEV, autoreset=True, spawn_queue_len=64)
    try:
        env.reset(seed=0)
        period = 1024
        cc, man = bench.gen_actions(n, period, 1234, env.device)
        env.reserve_steps(K)
        env.reserve_poses(8192)
        with_obs = env.alloc_rollout(K, keys=("obs", "reward", "terminated", "truncated", "x", "y", "theta"))
        poses = env.alloc_rollout(K, keys=("reward", "terminated", "truncated", "x", "y", "theta"))
        frames = torch.empty_like(with_obs["obs"])
        rows = {s: torch.arange(0, K, s, device=DEV)[:, None].mul(n).add(torch.arange(n, device=DEV)[None, :]).reshape(-1).contiguous()
                for s in STRIDES}
        kept = {s: torch.empty((rows[s].numel(),) + tuple(env._obs_shape), dtype=torch.uint8, device=DEV) for s in STRIDES}
        g = torch.Generator(device=DEV).manual_seed(5)
        sample = torch.randint(0, K * n, (SAMPLE,), device=DEV, generator=g)
        sampled = torch.empty((SAMPLE,) + tuple(env._obs_shape), dtype=torch.uint8, device=DEV)
        t = [0]

        def step(roll):
            i = t[0] % period
            if i + K > period:
                i = 0
            env.step_multi(cc[i:i + K], man[i:i + K], rollout=roll)
            t[0] = i + K

        for done in range(0, bench.PREROLL_STEPS, K):  # the benchmark's pre-roll, without frames
            if done == bench.PREROLL_STEPS * 2 // 3 // K * K:
                env.top_up_spawn_queue()
            step(poses)
        torch.cuda.synchronize()
        env.top_up_spawn_queue()

        def form_b():
            step(poses)
            env.render_rollout(poses, out=frames)

        def form_c(s):
            step(poses)
            env.render_rollout(poses, index=rows[s], out=kept[s])

        forms = {"A_call_with_obs": lambda: step(with_obs), "B_call_plus_all_rows": form_b}
        forms.update({f"C_call_plus_every_{s}th_row": (lambda s=s: form_c(s)) for s in STRIDES})
        forms["D_256_random_rows"] = lambda: env.render_poses(poses["x"], poses["y"], poses["theta"], index=sample, out=sampled)
        ms = {k: [] for k in forms}
        for r in range(1 + reps):  # one warm-up round
            if r % 3 == 2:
                env.top_up_spawn_queue()  # (between the timed calls: host work of a few milliseconds)
            for k, fn in forms.items():
                v = timed(fn)
                if r > 0:
                    ms[k].append(v)
        # the deferred frames of the last (B)-style call against a call that draws them itself is the tests' business; here
        # only that something was drawn
        assert int(frames.max()) == 255 and int(sampled.max()) == 255
        out = {"shape": name, "envs": n, "steps_per_call": K, "reps": reps, "launch": env.launch_info(K)["kernel"],
               "frame_bytes": int(torch.tensor(env._obs_shape).prod()), "reserved_frames": 8192}
        for k, v in ms.items():
            med = statistics.median(v)
            out[k] = {"ms": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3)}
            if not k.startswith("D"):
                out[k]["env_steps_per_s"] = round(K * n / med * 1e3)
        a = out["A_call_with_obs"]["ms"]
        out["B_over_A"] = round(out["B_call_plus_all_rows"]["ms"] / a, 4)
        for s in STRIDES:
            out[f"C{s}_over_A"] = round(out[f"C_call_plus_every_{s}th_row"]["ms"] / a, 4)
        return out
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="cfg3,cfg4")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    lines = []
    for name in args.shapes.split(","):
        res = measure(name, max(args.reps, 7))
        res["tool"] = "tools/render_poses_rate.py"
        res["device"] = torch.cuda.get_device_name(0)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
