#!/usr/bin/env python
"""CPU study of the whole-frame cull (tinycarlo_amd/csrc/tc_cull.h): the oracle under bench.py's action distribution
and auto-reset, 256 envs x 1400 steps, every 8th step from step 700 sampled; per workload and cover the share of frames
the predicate calls empty, the share of the truly empty frames among them, and the number of frames WITH a segment it
calls empty (must be 0).  No GPU.  Writes profiles/r06/frame_cull_shares_cpu.json.

    python tools/frame_cull_study.py [--envs 256] [--steps 1400] [--out profiles/r06/frame_cull_shares_cpu.json]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (WORKLOADS, make_config: the benchmark's own)
import cull_shim  # noqa: E402
import orc  # noqa: E402


def rollout(w, n, steps, first, every):
    """-> (poses [f][3], segments per frame [f]) of the sampled frames"""
    from tinycarlo_amd import gym
    from tinycarlo_amd.camera import Camera
    from tinycarlo_amd.config import CarParams
    from tinycarlo_amd.map import Map
    cfg = bench.make_config(w)
    m = Map(cfg["map"])
    car = CarParams.from_config(1 / cfg["sim"].get("fps", 30), cfg["car"])
    cam = Camera(cfg["camera"])
    orc.set_math_mode(orc.MATH_LIBM)
    o = orc.Oracle(m, car, cam, orc.FMT_CLASSES, n, threads=min(16, os.cpu_count() or 1))
    rngs = [gym.np_random(i)[0] for i in range(n)]
    o.reset([m.sample_spawn_node(r) for r in rngs], flags=orc.F_NO_OBSERVATION)
    o.spawn_queue = np.array([[m.sample_spawn_node(r) for _ in range(64)] for r in rngs], dtype=np.int32)
    rng = np.random.default_rng(0)
    flags = orc.F_AUTORESET | orc.F_NO_OBSERVATION
    poses, nseg = [], []
    man = None
    for t in range(steps):
        if t % 64 == 0:
            man = rng.integers(0, 4, n).astype(np.int32)
        cc = np.stack([rng.uniform(0.3, 1, n), rng.uniform(-1, 1, n)], axis=1)
        o.step(cc, man, flags=flags, with_obs=False)
        if t >= first and (t - first) % every == 0:
            for i in range(n):
                poses.append((o.state["x"][i], o.state["y"][i], o.state["theta"][i]))
                nseg.append(len(o.segments(i)[0]))
    return m, cam, np.array(poses), np.array(nseg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "frame_cull_shares_cpu.json"))
    a = ap.parse_args()
    out = {"_setup": f"oracle (libm), bench.py's actions and auto-reset, {a.envs} envs x {a.steps} steps, every 8th step from "
                     f"step {a.steps // 2} sampled; tools/frame_cull_study.py"}
    with tempfile.TemporaryDirectory() as td:
        shims = {nc: cull_shim.build_shim(td, nc) for nc in (1, 2, 3)}
        for name in ("cfg3", "cfg4"):
            m, cam, poses, nseg = rollout(bench.WORKLOADS[name], a.envs, a.steps, a.steps // 2, 8)
            res = {"frames": int(len(nseg)), "empty_share": float((nseg == 0).mean()), "segments_per_frame": float(nseg.mean()),
                   "variants": []}
            for nc, L in shims.items():
                for cell in (0.01, 0.02, 0.04):
                    c = cull_shim.Cull(L, m, cam, cell=cell)
                    e = c.empty(poses[:, 0], poses[:, 1], poses[:, 2])
                    res["variants"].append({
                        "circles": nc, "cell_m": c.cell, "grid": [c.nx, c.ny], "table_bytes": c.nx * c.ny, "cull_on": int(c.on),
                        "special_nodes": c.n_special, "longest_edge_m": c.lmax,
                        "cover_car_frame_x_y_r": np.round(c.circles, 4).tolist(),
                        "frames_culled_share": float(e.mean()),
                        "empty_frames_culled_share": float(e[nseg == 0].mean()) if (nseg == 0).any() else 0.0,
                        "nonempty_frames_culled": int((e & (nseg > 0)).sum())})
                    print(name, res["variants"][-1], flush=True)
            if not res["variants"][0]["cull_on"]:
                res["why_off"] = ("H1 of tc_cull.h: the map's longest lane-line edge is not shorter than the camera's max_range, or H3 / "
                                  "the special-node limit (grid [0, 0]): the predicate answers 'maybe' for every frame")
            out[name] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
