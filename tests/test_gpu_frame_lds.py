"""The frame kernels' own LDS plan and the one-word list entries of the register-held camera path on the GPU: 64 envs and
12-step calls against the oracle (portable math), observations and draw-list lengths at tolerance 0.

(a) simple_layout 64x64 thickness 2, streamed and TC_STREAM=0: the plan of tests/test_frame_lds_cpu.py as the handle
    reports it -- at most 8960 bytes, a head of at least 40 entries, at least 18 workgroups per CU.
(b) the same with TC_SEG_LDS_CAP=3 and =0: every frame with a segment takes the head + refill path of the new layout.
(c) thickness 3: the four-edge outline form, full-size tables.
(d) a map of 160 short edges that all cross one straight line, every car placed so that the camera plane z = 0 lies on
    that line: every edge straddles in clip pass 1 or 2, the packed list is filled to the group's edge count, and a few
    further edges share a target node, so the chain replay runs on packed entries.
(e) knuffingen, component groups at 64x64: the K = 5 / batches-of-16 frame kernel, whose layout and results are unchanged.
(f) single steps on simple_layout as the fused tc_step_kernel and as tc_env_kernel + tc_raster_kernel (TC_FUSE=0): the
    other kernels that run cam_group_regs, with the two-int entries and the layout they always had.
"""
import copy
import json
import math
import os

import numpy as np
import pytest

import big_maps
import frame_lds_shim as fs
import orc
from common import load_cfg
from test_gpu_parity import make_env, make_oracle, push_state

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K = 64, 12


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def actions(seed, slow=False):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.02, 0.12, (K, N)) if slow else rng.uniform(0.3, 1, (K, N))
    cc = np.stack([v, rng.uniform(-1, 1, (K, N))], axis=2).astype(np.float32)
    return cc, rng.integers(0, 4, (K, N)).astype(np.int32)


_refs = {}


def reference(key, env, cc, man, start=None):
    """the oracle's K steps from the env's reset (or from `start`, a state array): frames [K][N][..] and draw-list lengths
    [K][N], computed once per key and left unchanged"""
    if key not in _refs:
        o = make_oracle(env)
        o.reset(env._keep[0].cpu().numpy())
        if start is not None:
            o.state[:] = start
        obs, nseg = [], []
        for k in range(K):
            o.step(cc[k].astype(np.float64), man[k])
            obs.append(o.obs.copy())
            nseg.append([len(o.segments(i)[0]) for i in range(N)])
        obs, nseg = np.stack(obs), np.array(nseg)
        obs.setflags(write=False)
        nseg.setflags(write=False)
        _refs[key] = (obs, nseg)
    return _refs[key]


def check_stats(env, nseg, what):
    """tc_env_draw_list_stats over the call's frames against the oracle's draw-list lengths"""
    st = env.draw_list_stats()
    # (a streamed call: all K steps; a chunked one: the steps of the chunks its scratch ring still holds, the last ones)
    rows = st["frames"] // N
    assert st["frames"] == rows * N and K // 2 <= rows <= K, (what, st)
    nseg = nseg[K - rows:]
    assert st["max_segments"] == int(nseg.max()), (what, st, int(nseg.max()))
    assert st["empty_frame_frac"] == float((nseg == 0).sum()) / nseg.size, (what, st)
    assert st["mean_segments_per_frame"] == float(nseg.sum()) / nseg.size, (what, st)


def run_multi(env, key, cc, man, what, start=None):
    """one K-step call with every frame in a rollout, equal to the oracle"""
    env.reset(seed=21)
    if start is not None:
        push_state(env, start)
    obs, nseg = reference(key, env, cc, man, start)
    roll = env.alloc_rollout(K, keys=("obs", "cte"))
    env.step_multi(torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda(), rollout=roll)
    torch.cuda.synchronize()
    assert env.launch_info(K)["kernel"].endswith("tc_frame_kernel"), (what, env.launch_info(K))
    got = roll["obs"].cpu().numpy().reshape(K, N, -1)
    bad = np.argwhere((got != obs).any(axis=2))
    assert bad.size == 0, (what, "frames differ at (step, env)", bad[:8].tolist(), nseg[tuple(bad[:8].T)].tolist())
    assert got.max() == 255, what
    check_stats(env, nseg, what)
    return nseg


def run_single(env, key, cc, man, what):
    env.reset(seed=21)
    obs, nseg = reference(key, env, cc, man)
    for k in range(K):
        env.step({"car_control": cc[k], "maneuver": man[k]})
        torch.cuda.synchronize()
        got = env.out["obs"].cpu().numpy().reshape(N, -1)
        bad = np.flatnonzero((got != obs[k]).any(axis=1))
        assert bad.size == 0, (what, "step", k, "envs", bad[:8].tolist())
        st = env.draw_list_stats()
        assert (st["frames"], st["max_segments"]) == (N, int(nseg[k].max())), (what, k, st)
        assert st["mean_segments_per_frame"] == float(nseg[k].sum()) / N, (what, k, st)


@pytest.mark.parametrize("stream", ["1", "0"])
def test_a_simple_layout_plan_and_frames(monkeypatch, stream):
    monkeypatch.setenv("TC_STREAM", stream)
    env = make_env("simple_layout", "r64", "classes", N)
    assert env.camera.line_thickness == 2
    info = env.frame_lds_info()
    assert info["lds_bytes"] <= 8960 and info["head_entries"] >= 40 and info["workgroups_per_cu"] >= 18, info
    assert info["bits_offset"] == 5248, info
    cc, man = actions(13)
    nseg = run_multi(env, "simple", cc, man, f"TC_STREAM={stream}")
    assert nseg.max() > 8  # (more than the smallest head holds: what (b) relies on)
    env.close()


@pytest.mark.parametrize("cap", ["3", "0"])
def test_b_head_and_refill_paths(monkeypatch, cap):
    monkeypatch.setenv("TC_SEG_LDS_CAP", cap)
    env = make_env("simple_layout", "r64", "classes", N)
    info = env.frame_lds_info()
    assert info["head_entries"] == 8 and info["lds_bytes"] <= 8960, info  # (the frame kernel's floor of 8 entries)
    cc, man = actions(13)
    run_multi(env, "simple", cc, man, f"TC_SEG_LDS_CAP={cap}")
    env.close()


def test_c_four_edge_form():
    env = make_env("simple_layout", "r64", "classes", N, camera={"line_thickness": 3})
    info = env.frame_lds_info()
    assert info["bits_offset"] == 6784 and info["lds_bytes"] <= 10240, info
    cc, man = actions(13)
    run_multi(env, "simple_t3", cc, man, "thickness 3")
    env.close()


# ---------------------------------------------------------------------------------------------- (d)
N_CROSS = 160


def straddle_map(tmp_path):
    """-> (config, spawn node, start state): a lane path of big_maps' generator, and one lane-line layer of N_CROSS edges across
    the ground line of the camera plane z = 0 of a car spawned at the node (2 i, 2 i + 1 = the ends behind / in front of
    edge i, alternately as e[0]), plus edges that share the behind end of edge 0 (three times a target of pass 1) and of
    edge 1 (twice a target of pass 2)"""
    rng = np.random.default_rng(160)
    mj = big_maps.big_map(rng, [(4, "dashes")])
    cfg = copy.deepcopy(load_cfg("simple_layout")[0])
    path = tmp_path / "straddle.json"
    cfg["map"] = {"json_path": str(path), "pixel_per_meter": 300}
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["camera"].update(resolution=[64, 64], line_thickness=2)

    def write():
        with open(path, "w") as f:
            json.dump(mj, f)

    # the spawn pose, from a map that has the lane path already: the lane lines do not move it
    write()
    from tinycarlo_amd.camera import Camera
    from tinycarlo_amd.config import CarParams
    from tinycarlo_amd.map import Map
    m = Map(cfg["map"])
    cam = Camera(cfg["camera"])
    car = CarParams.from_config(1 / cfg["sim"].get("fps", 30), cfg["car"])
    node = m.sample_spawn_node(np.random.default_rng(5))
    o = orc.Oracle(m, car, cam, orc.FMT_CLASSES, 1)
    o.reset([node])
    row = depth_row(cam, o.state[0])
    a, b, d = row[0], row[1], row[3]           # depth of a ground point: a X + b Y + d (metres); in front: < 0
    nrm = math.hypot(a, b)
    xy = np.array([o.state[0]["x"], o.state[0]["y"]])
    p0 = xy - np.array([a, b]) * ((a * xy[0] + b * xy[1] + d) / (nrm * nrm))  # the point of that line next to the car
    back, tan = np.array([a, b]) / nrm, np.array([-b, a]) / nrm
    nodes, edges = [], []
    for i in range(N_CROSS):
        c = (p0 + tan * ((i - N_CROSS / 2) * 2.2 / 300)) * 300
        nodes.append([int(round(v)) for v in c + back * 45])                          # behind the plane
        nodes.append([int(round(v)) for v in c - back * (30 + (i * 7) % 170)])        # in front of it
        edges.append([2 * i, 2 * i + 1] if i % 2 == 0 else [2 * i + 1, 2 * i])
    edges += [[0, 2 * 2 + 1], [0, 2 * 4 + 1], [2 * 3 + 1, 2 * 1]]
    mj["lanelines"] = {"cross": {"layer_color": [255, 0, 0], "nodes": nodes, "edges": edges}}
    write()
    return cfg, node


def depth_row(cam, st):
    """row 2 of camera.py:62's pose = E @ R(-theta) @ T(-x, -y) for one state"""
    c, s = math.cos(-st["theta"]), math.sin(-st["theta"])
    R = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    T = np.array([[1, 0, 0, -st["x"]], [0, 1, 0, -st["y"]], [0, 0, 1, 0], [0, 0, 0, 1]])
    return (np.asarray(cam.E, dtype=np.float64).reshape(3, 4) @ (R @ T))[2]


def test_d_every_edge_straddles(tmp_path):
    cfg, node = straddle_map(tmp_path)
    env = make_env(cfg, None, None, N)
    assert env.launch_info(K)["kvar"] == 5, env.launch_info(K)
    env.reset(seed=21)
    o = make_oracle(env)
    o.reset(np.full(N, node, dtype=np.int32))
    start = o.state.copy()
    cc, man = actions(7, slow=True)
    # on the CPU: in some sampled frame nearly every edge has one end in front of the camera plane and one behind
    nodes = np.array(env.map.lanelines[0].nodes, dtype=np.float64)
    edges = np.array(env.map.lanelines[0].edges)
    assert len(nodes) == 2 * N_CROSS <= 5 * 64 and N_CROSS < len(edges) <= 5 * 64
    most = 0
    for k in range(K):
        o.step(cc[k].astype(np.float64), man[k], with_obs=False)
        for i in range(0, N, 8):
            r = depth_row(env.camera, o.state[i])
            front = nodes @ r[:2] + r[3] < 0
            most = max(most, int((front[edges[:, 0]] != front[edges[:, 1]]).sum()))
    assert most >= 150, most
    run_multi(env, "straddle", cc, man, "160 straddling edges", start=start)
    env.close()


def test_e_knuffingen_component_groups():
    env = make_env("knuffingen", "r64", "classes", N)
    cfg, path = load_cfg("knuffingen")
    with open(os.path.join(os.path.dirname(path), cfg["map"]["json_path"])) as f:
        plan = big_maps.expected_plan(json.load(f))
    assert plan["kframe"] == 516
    info = env.frame_lds_info()
    shared, head, _ = fs.shared_frame_lds(plan, 64, 64)
    # (not the five-wave kernel: the layout shared with the other kernels, unchanged)
    assert (info["lds_bytes"], info["head_entries"], info["bits_offset"]) == (shared, head, fs.align_up(fs.r_tab_bytes(16), 16)), (info, shared, head)
    cc, man = actions(3)
    run_multi(env, "knuffingen", cc, man, "knuffingen")
    env.close()


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_f_single_step_kernels(monkeypatch, fuse):
    monkeypatch.setenv("TC_FUSE", fuse)
    env = make_env("simple_layout", "r64", "classes", N)
    assert env.launch_info(1)["kernel"] == ("tc_step_kernel" if fuse == "1" else "tc_env_kernel+tc_raster_kernel")
    cc, man = actions(13)
    run_single(env, "simple", cc, man, f"TC_FUSE={fuse}")
    env.close()
