"""The whole-frame cull at the head of the camera stage (tc_cull.h, cam_cull) on the GPU: frames, draw-list statistics
and rollout rows through tc_step, one streamed and one chunked tc_step_multi call against the oracle's, bit for bit, and
bit for bit between TC_FRAME_CULL=1 (default) and 0.

Some envs are parked (zero velocity, zero action: the pose does not move) at poses of the CPU test's sets
(tests/cull_shim.py): far outside the map facing outward, on the ring where the predicate flips and one cell to either
side of it, on the road facing along it, beside the road facing away, and 60 m away, outside the table.  The CPU form of
the predicate says which of them the kernel culls; the kernels carry no counter for it in the shipped build.

knuffingen (component groups, K = 5 / RB = 16) has edges longer than the camera's range: condition H1 of tc_cull.h
switches its cull off, so that case checks that the switch changes nothing there.  Per-env cameras switch the cull off
as well.
"""
import copy

import numpy as np
import pytest

import cull_shim
import orc
from test_gpu_parity import make_env, make_oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 8
KEYS = ("obs", "reward", "terminated", "truncated", "cte")


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cull_shim.build_shim(tmp_path_factory.mktemp("tc_cull_gpu"))


def pinned_poses(cull, m):
    """-> (poses [p][3], first index of the outside poses, their count)"""
    out = cull_shim.outside_poses(cull.nodes, n=4)
    far = np.array([[cull.nodes[:, 0].max() + 60.0, cull.nodes[:, 1].max() + 60.0, 0.7]])
    ring = cull_shim.boundary_poses(cull, n_nodes=2, offsets=(cull.cell, -cull.cell, 0.0))
    road = cull_shim.road_poses(m, n=3)
    away = road.copy()  # beside the road (0.12 m to the left of it), facing away from it
    away[:, 0] += 0.12 * np.cos(road[:, 2] + 0.5 * np.pi)
    away[:, 1] += 0.12 * np.sin(road[:, 2] + 0.5 * np.pi)
    away[:, 2] += 0.5 * np.pi
    return np.concatenate([out, far, ring, road, away]), 0, len(out) + 1


def start(map_name, res_key, n, poses, seed=5, camera=None):
    env = make_env(map_name, res_key, "classes", n, **({} if camera is None else {"camera": camera}))
    o = make_oracle(env)
    env.reset(seed=seed)
    o.reset(env._keep[0].cpu().numpy())
    sd = env.state_dict()
    for i, p in enumerate(poses):
        for k, v in zip(("x", "y", "theta", "velocity", "steering"), (p[0], p[1], p[2], 0.0, 0.0)):
            sd["state"][k][i] = v
            o.state[k][i] = v
    env.load_state_dict(sd)
    return env, o


def actions(n, n_pinned, steps, seed):
    rng = np.random.default_rng(seed)
    cc = np.stack([rng.uniform(0.3, 1, (steps, n)), rng.uniform(-1, 1, (steps, n))], axis=2).astype(np.float32)
    cc[:, :n_pinned, :] = 0.0
    return cc, rng.integers(0, 4, (steps, n)).astype(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run(map_name, res_key, n, poses, stream, got):
    """3 x tc_step, then one K-step call; everything checked against the oracle and appended to got"""
    env, o = start(map_name, res_key, n, poses)
    cc, man = actions(n, len(poses), 3 + K, seed=2)
    for k in range(3):
        env.step({"car_control": cc[k], "maneuver": man[k]})
        o.step(cc[k].astype(np.float64), man[k])
        torch.cuda.synchronize()
        g = env.out["obs"].cpu().numpy().reshape(n, -1)
        bad = np.flatnonzero((g != o.obs).any(axis=1))
        assert bad.size == 0, ("tc_step", map_name, "step", k, "envs", bad[:8])
        got.append(g.copy())
        got.append(np.array(sorted(env.draw_list_stats().items()), dtype=object).astype(str))
    roll = env.alloc_rollout(K, keys=KEYS)
    env.step_multi(torch.from_numpy(cc[3:]).cuda(), torch.from_numpy(man[3:]).cuda(), rollout=roll)
    torch.cuda.synchronize()
    for k in range(K):
        o.step(cc[3 + k].astype(np.float64), man[3 + k])
        assert same_bits(roll["cte"][k].cpu().numpy(), o.info["cte"]), (stream, "cte of step", k)
        assert same_bits(roll["reward"][k].cpu().numpy(), o.info["reward"]), (stream, "reward of step", k)
        assert np.array_equal(roll["terminated"][k].cpu().numpy() != 0, o.info["terminated"] != 0), (stream, "terminated of step", k)
        g = roll["obs"][k].cpu().numpy().reshape(n, -1)
        bad = np.flatnonzero((g != o.obs).any(axis=1))
        assert bad.size == 0, ("tc_step_multi", map_name, stream, "step", k, "envs", bad[:8])
    for key in KEYS:
        got.append(roll[key].cpu().numpy().copy())
    got.append(np.array(sorted(env.draw_list_stats().items()), dtype=object).astype(str))
    for key in ("x", "y", "theta"):
        got.append(env.state[key].cpu().numpy().copy())
    last = roll["obs"][K - 1].cpu().numpy().reshape(n, -1)
    env.close()
    return last, o


@pytest.mark.parametrize("map_name,res_key,n", [("simple_layout", "r64", 64), ("knuffingen", "r128", 16)])
def test_frames_equal_the_oracle_and_the_switch_changes_nothing(map_name, res_key, n, shim, monkeypatch):
    from common import setup
    _, m, _, cam = setup(map_name, res_key)
    cull = cull_shim.Cull(shim, m, cam)
    poses, out0, n_out = pinned_poses(cull, m)
    poses = poses[: n - 2]
    want_culled = cull.empty(poses[:, 0], poses[:, 1], poses[:, 2])
    if map_name == "simple_layout":
        assert cull.on and want_culled[out0:out0 + n_out].all() and not want_culled.all()
        assert len(poses) >= n_out + 6 + 6
    else:
        assert not cull.on and not want_culled.any()  # H1: knuffingen's longest edge is 0.58 m, the camera's range 0.5 m
    results = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("TC_FRAME_CULL", sw)
        got = []
        for stream in ("1", "0"):
            monkeypatch.setenv("TC_STREAM", stream)
            last, o = run(map_name, res_key, n, poses, stream, got)
            # the parked envs stayed where they were put, and the ones the predicate culls drew nothing
            for i, p in enumerate(poses):
                assert (o.state["x"][i], o.state["y"][i], o.state["theta"][i]) == tuple(p), i
            assert not last[:len(poses)][want_culled].any()
            assert last.max() == 255
        results[sw] = got
    assert len(results["1"]) == len(results["0"])
    for a, b in zip(results["1"], results["0"]):
        assert same_bits(a, b) if a.dtype != object and a.dtype.kind != "U" else np.array_equal(a, b)


def test_noise_blob_on_culled_frames(shim, monkeypatch):
    """with noise blobs configured (they black pixels out: a frame without a segment stays empty) the culled frames are
    what the raster stage's own empty-frame path delivers, and the others carry the oracle's noise"""
    from common import setup
    n, C_blobs, R, seed = 64, 3, 20, 11
    _, m, _, cam = setup("simple_layout", "r64")
    cull = cull_shim.Cull(shim, m, cam)
    poses, _, n_out = pinned_poses(cull, m)
    frames = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("TC_FRAME_CULL", sw)
        env, o = start("simple_layout", "r64", n, poses)
        env.set_noise(C_blobs, R, seed=seed)
        cc, man = actions(n, len(poses), 3, seed=4)
        C, (H, W) = env.n_classes, (64, 64)
        got = []
        for step in range(3):
            env.step({"car_control": cc[step], "maneuver": man[step]})
            o.step(cc[step].astype(np.float64), man[step])
            torch.cuda.synchronize()
            want = o.obs.reshape(n, C, H, W).copy()
            for i in range(n):
                orc.noise_classes(want[i], orc.noise_blobs(seed, i, step, C_blobs, C, H, W, R), C_blobs)
            g = env.out["obs"].cpu().numpy().reshape(n, C, H, W)
            assert np.array_equal(g, want), (sw, step)
            assert not np.array_equal(want, o.obs.reshape(n, C, H, W))  # (the noise does change frames)
            got.append(g.copy())
        assert not got[-1][:n_out].any() and got[-1].any()
        frames[sw] = np.stack(got)
        env.close()
    assert same_bits(frames["1"], frames["0"])


def test_camera_change_between_calls_and_per_env_cameras(shim, monkeypatch):
    """tc_env_set_camera to a second parameter set between two K-step calls (the cover follows the camera), then per-env
    cameras (the cull is off: its cover is the shared camera's)"""
    from common import setup
    from tinycarlo_amd.camera import Camera
    n = 64
    _, m, _, cam = setup("simple_layout", "r64")
    cull = cull_shim.Cull(shim, m, cam)
    poses, _, n_out = pinned_poses(cull, m)
    rows = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("TC_FRAME_CULL", sw)
        env, o = start("simple_layout", "r64", n, poses)
        cc, man = actions(n, len(poses), 2 * K + 2, seed=6)
        got = []

        def call(t0):
            roll = env.alloc_rollout(K, keys=("obs", "cte"))
            env.step_multi(torch.from_numpy(cc[t0:t0 + K]).cuda(), torch.from_numpy(man[t0:t0 + K]).cuda(), rollout=roll)
            torch.cuda.synchronize()
            for k in range(K):
                o.step(cc[t0 + k].astype(np.float64), man[t0 + k])
                g = roll["obs"][k].cpu().numpy().reshape(n, -1)
                bad = np.flatnonzero((g != o.obs).any(axis=1))
                assert bad.size == 0, (sw, "call at", t0, "step", k, "envs", bad[:8])
            got.append(roll["obs"].cpu().numpy().copy())

        call(0)
        env.camera.orientation = [35, 3, -20]  # looks down more steeply and to the side: another footprint
        env.camera.fov = 100
        env.camera.update_params()
        o.set_camera(env.camera)
        call(K)
        # per-env cameras: two variants over the batch, one oracle each
        oris, fovs, pick = [[22, 0, 0], [12, -3, 40]], [80, 68], np.arange(n) % 2
        env.set_env_cameras(orientation=[oris[k] for k in pick], fov=[fovs[k] for k in pick])
        oracles = []
        for k in range(2):
            c2 = copy.deepcopy(env.config["camera"])
            c2.update(orientation=oris[k], fov=fovs[k])
            ok = orc.Oracle(env.map, env.car_params, Camera(c2), orc.FMT_CLASSES, n, threads=4)
            ok.state[:] = o.state
            oracles.append(ok)
        for t in range(2 * K, 2 * K + 2):
            env.step({"car_control": cc[t], "maneuver": man[t]})
            torch.cuda.synchronize()
            g = env.out["obs"].cpu().numpy().reshape(n, -1)
            for ok in oracles:
                ok.step(cc[t].astype(np.float64), man[t])
            for i in range(n):
                assert np.array_equal(g[i], oracles[pick[i]].obs[i]), (sw, "per-env cameras", t, i)
            got.append(g.copy())
        rows[sw] = got
        env.close()
    for a, b in zip(rows["1"], rows["0"]):
        assert same_bits(a, b)
