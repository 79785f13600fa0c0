"""The CPU side of tests/test_gpu_info_rows.py: the oracle's run of a case (spawn nodes, spawn queue and actions drawn
here from a seed, so that no GPU is needed to know what a case will see), computed once per case and shared.
"""
import functools

import numpy as np

import orc
from common import setup
from tinycarlo_amd import terms as T

QLEN = 8  # spawn queue entries per env (the cases are short: no env re-spawns that often)
STATE_F = ("x", "y", "theta", "velocity", "steering", "radius", "front_x", "front_y")


def stack_of(name, layer_names):
    """-> (terms innermost first, env.wrapped).  "laneline": terms that read the distances; "cte" / "cte_short": terms that
    do not (the second ends episodes quickly: re-spawns inside a short call)."""
    if name == "none":
        return [], False
    if name == "laneline":  # (the CTE termination keeps episodes ending, so that the steps differ in kind)
        return [T.laneline_linear_reward(layer_names, {n: 1.0 + i for i, n in enumerate(layer_names)}),
                T.laneline_sparse_reward(layer_names, {layer_names[0]: 0.5, layer_names[-1]: 0.25}),
                T.cte_termination(0.04, 2),
                T.laneline_crossing_termination(layer_names, [layer_names[0], layer_names[1]])], True
    if name == "cte":
        return [T.cte_linear_reward(0.05, 1.0, -1.0), T.cte_sparse_reward(0.02, 2.0), T.cte_termination(0.04, 2)], True
    if name == "cte_short":
        return [T.cte_termination(0.01, 1)], True
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def world(map_name):
    """-> (what tests/test_gpu_parity.make_env takes as its map, Map, CarParams, Camera) at 64x64 class masks.  map_name: a
    bundled map, or "big:<case>" = map 0 of a case of tests/big_maps.py (up to 16 lane-line layers)."""
    if not map_name.startswith("big:"):
        return (map_name,) + tuple(setup(map_name, "r64")[1:])
    import os
    import tempfile

    import big_maps
    from tinycarlo_amd.camera import Camera
    from tinycarlo_amd.config import CarParams
    from tinycarlo_amd.map import Map
    path = os.path.join(tempfile.mkdtemp(prefix="tc_info_rows_"), "map.json")
    cfg = big_maps.case_config(map_name[4:], 0, path)
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["camera"]["resolution"] = [64, 64]
    return cfg, Map(cfg["map"], base_path=path), CarParams.from_config(1 / cfg["sim"].get("fps", 30), cfg["car"]), Camera(cfg["camera"])


def inputs(map_name, n, steps, seed):
    """spawn nodes [n], spawn queue [n, QLEN], car_control [steps, n, 2] float32, maneuver [steps, n] int32"""
    m = world(map_name)[1]
    rng = np.random.default_rng(seed)
    tab = np.asarray(m.spawn_table(), dtype=np.int32)
    nodes = rng.choice(tab, n).astype(np.int32)
    queue = rng.choice(tab, (n, QLEN)).astype(np.int32)
    cc = np.stack([rng.uniform(0.3, 1.0, (steps, n)), rng.uniform(-1.0, 1.0, (steps, n))], axis=2).astype(np.float32)
    man = np.repeat(rng.integers(0, 4, ((steps + 7) // 8, n)), 8, axis=0)[:steps].astype(np.int32)
    return nodes, queue, cc, man


@functools.lru_cache(maxsize=None)
def reference(map_name, n, steps, seed, stack, with_obs=True):
    """The oracle's run: per-step rows (step k of the run) and, per step too, what the env's buffers hold after a call
    that ends with that step.  Read-only for its users, who call it in the oracle's portable math mode (the mode the GPU is
    bit-identical to; a module's fixture sets it)."""
    _, m, car, cam = world(map_name)
    o =orc.Oracle(m, car, cam, orc.FMT_CLASSES, n, threads=8)
    C = o.map.C
    terms, wrapped = stack_of(stack, m.get_laneline_names())
    o.terms = terms
    nodes, queue, cc, man = inputs(map_name, n, steps, seed)
    o.spawn_queue = queue
    flags = orc.F_AUTORESET | (orc.F_WRAPPED if wrapped else 0)
    o.reset(nodes, flags=flags & orc.F_WRAPPED)
    rows = {k: [] for k in ("reward", "terminated", "truncated", "cte", "heading_error", "laneline_distances", "nearest_edge",
                            "lp_len", "fresh", "obs", "state", "needs_reset", "spawn_cursor", "term_counters")}
    for k in range(steps):
        rows["fresh"].append(o.needs_reset.astype(bool).copy())  # re-spawned at this step
        o.step(cc[k].astype(np.float64), man[k], flags=flags, with_obs=with_obs)
        inf = o.info
        rows["reward"].append(inf["reward"].copy())
        rows["cte"].append(inf["cte"].copy())
        rows["heading_error"].append(inf["heading_error"].copy())
        rows["terminated"].append(inf["terminated"].astype(np.uint8))
        rows["truncated"].append(inf["truncated"].astype(np.uint8))
        rows["laneline_distances"].append(inf["dist"][:, :C].copy())
        rows["nearest_edge"].append(inf["nearest_edge"][:, :C].copy())
        rows["lp_len"].append(o.state["lp_len"].copy())
        rows["state"].append(o.state.copy())
        rows["needs_reset"].append(o.needs_reset.copy())
        rows["spawn_cursor"].append(o.spawn_cursor.copy())
        rows["term_counters"].append(o.term_counters.copy())
        if with_obs:
            rows["obs"].append(o.obs.copy())
    out = {k: np.stack(v) for k, v in rows.items() if v}
    for v in out.values():
        v.setflags(write=False)
    return out
