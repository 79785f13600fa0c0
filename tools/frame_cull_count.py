#!/usr/bin/env python3
"""Share of the frames the whole-frame cull catches ON THE GPU, from the ablation build's counter (make dev-ablate:
tc_debug_cull_counts; the shipped library has no such counter).  The workload is bench.py's: its config, its actions,
auto-reset, 1024 untimed steps first, then 1024 counted steps in 128-step calls.

    TINYCARLO_HIP_LIB=<ablation build> python tools/frame_cull_count.py [--workload cfg3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--steps", type=int, default=1024)
    a = ap.parse_args()
    from tinycarlo_amd import _native as nat
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    L = nat.lib()
    if not hasattr(L, "tc_debug_cull_counts"):
        sys.exit("frame_cull_count.py: the loaded library is not an ablation build (make -C tinycarlo_amd/csrc dev-ablate)")
    L.tc_debug_cull_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    w = bench.WORKLOADS[a.workload]
    n, M = w["envs"], 128
    dev = torch.device("cuda", 0)
    env = TinyCarloVecEnv(bench.make_config(w), num_envs=n, device=dev, autoreset=True, spawn_queue_len=64)
    env.reset(seed=0)
    cc, man = bench.gen_actions(n, 1024, seed=0, device=dev)
    roll = env.alloc_rollout(M, keys=("obs", "reward", "terminated", "truncated"))
    env.reserve_steps(M)
    for t in range(0, bench.PREROLL_STEPS, M):
        env.step_multi(cc[t:t + M], man[t:t + M], rollout=roll)
    env.top_up_spawn_queue()
    out = (C.c_uint64 * 2)()
    nat.check(L.tc_debug_cull_counts(out, 1), "tc_debug_cull_counts")
    for t in range(0, a.steps, M):
        i = t % 1024
        env.step_multi(cc[i:i + M], man[i:i + M], rollout=roll)
    nat.check(L.tc_debug_cull_counts(out, 1), "tc_debug_cull_counts")
    stats = env.draw_list_stats()
    print(json.dumps({"workload": a.workload, "frames_tested": int(out[0]), "frames_culled": int(out[1]),
                      "culled_share": out[1] / max(1, out[0]), "frames_expected": n * a.steps,
                      "draw_list_stats_last_call": {k: (float(v) if isinstance(v, (int, float)) else str(v)) for k, v in stats.items()}}))
    env.close()


if __name__ == "__main__":
    main()
