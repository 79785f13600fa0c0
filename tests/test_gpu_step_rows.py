"""The per-step feature rows of a K-step call (tc_step_rows: caller's steering noise in; steer label, maneuver, OU value,
episode length / return and camera index out) at the chunk and segment boundaries of every route a call can take.

The rows are sliced per launch by rows_at() on the host, as the rollout is by rollout_at(): a row family offset wrongly
shows as rows written to (or noise read from) the wrong step.  Reference: a twin env that runs the K steps as K one-step
tc_step_multi calls, each given the [k:k+1] slice of every row array -- no slicing inside the library at all.
Set-up: simple_layout, 64x64 class masks, N = 40 (two workgroups of the grouped kernel, the second partial), K = 6, per-env
cars, a time limit of 3 so that re-spawns fall inside the call, a controller with caller noise, drive randomisation with
maneuvers and OU noise, a camera bank of 3, autoreset with device spawns.  Run on the MI355X box with `pytest -m gpu`."""
import copy
import os

import numpy as np
import pytest

from common import load_cfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K, LIMIT, SEED = 40, 6, 3, 11
ROW_KEYS = ("steer", "maneuver", "steer_noise", "episode_length", "episode_return", "camera")  # + the noise rows going in
KEYS = ("obs", "reward") + ROW_KEYS
LIVE = ("steer_last", "camera_index", "camera_episode", "episode_maneuver", "drive_episode", "ou_state", "ou_draws",
        "env_car_params", "car_episode")


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def make_env(no_observation=False):
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    cfg, path = load_cfg("simple_layout")
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = [64, 64]
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    vec = TinyCarloVecEnv(cfg, num_envs=N, device="cuda:0", autoreset=True, spawn="device")
    p = vec.car_params
    vec.randomize_cars({"max_steering_angle": (0.4 * p.max_steering_angle, 1.2 * p.max_steering_angle)}, seed=SEED)
    vec.set_time_limit(LIMIT)
    vec.set_controller(k=4.0, speed=0.4)
    vec.randomize_drive(maneuvers=(0, 1, 3), ou=dict(theta=0.1, mu=0.0, sigma=0.4, reset=True), seed=SEED + 1)
    vec.randomize_cameras(fov=[80, 90, 105], seed=SEED + 2)
    vec.no_observation = no_observation
    vec.reset(seed=SEED)
    vec.episode_stats["length"].copy_((torch.arange(N, device="cuda:0") % LIMIT).to(torch.int32))  # staggered episodes
    return vec


def caller_noise():
    return torch.from_numpy(np.random.default_rng(SEED).uniform(-0.3, 0.3, (K, N))).cuda()


def final_of(vec, obs):
    torch.cuda.synchronize()
    d = {("state", k): bits(v) for k, v in vec.state.items()}
    d.update({("out", k): bits(v) for k, v in vec.out.items() if obs or k != "obs"})
    d.update({("aux", k): bits(v) for k, v in vec._aux.items() if k != "spawn_queue"})
    d.update({("ep", k): bits(v) for k, v in vec.episode_stats.items()})
    d.update({("live", k): bits(getattr(vec, k)) for k in LIVE if getattr(vec, k) is not None})
    return d


@pytest.fixture(scope="module")
def ref():
    """K one-step tc_step_multi calls, each with the [k:k+1] slice of every row array"""
    vec = make_env()
    roll, noise = vec.alloc_rollout(K, keys=KEYS), caller_noise()
    for k in range(K):
        vec.drive(None, rollout={key: t[k:k + 1] for key, t in roll.items()}, steer_noise=noise[k:k + 1])
    final = final_of(vec, obs=False)  # (the bound observation: untouched by calls with rollout["obs"], not compared)
    rows = {key: bits(t) for key, t in roll.items()}
    vec.close()
    # not vacuous: re-spawns inside the call (staggered starts and a limit of 3: on rows 1, 2, 3 and 5, so in every chunk /
    # segment of two rows, never for all envs at once), and rows that differ from step to step
    respawn = (rows["episode_length"] == 0) & (rows["steer"] == 0)
    assert respawn.any(axis=1)[[1, 2, 3, 5]].all() and not respawn.all(axis=1).any(), respawn.sum(axis=1)
    assert len(np.unique(rows["camera"])) == 3 and (rows["camera"][0] != rows["camera"][-1]).any()
    assert set(np.unique(rows["maneuver"])) == {0, 1, 3} and (rows["maneuver"][0] != rows["maneuver"][-1]).any()
    for key in ("steer", "steer_noise", "episode_length"):
        assert all((rows[key][k] != rows[key][k + 1]).any() for k in range(K - 1)), (key, "rows repeat")
    assert rows["obs"].reshape(K, -1).any(axis=1).all(), "every step draws something"
    return {"rows": rows, "final": final}


ROUTES = {"streamed": ({}, "tc_drive_envg_kernel+tc_frame_kernel", K),
          "segments_of_2": ({"TC_STREAM_SCRATCH_MB": "0.001"}, "tc_drive_envg_kernel+tc_frame_kernel", 2),
          "chunks_of_2": ({"TC_STREAM": "0", "TC_CHUNK": "2"}, "tc_drive_envg_kernel+tc_frame_kernel", 2),
          "no_observation": ({}, "tc_drive_env_kernel", None)}


@pytest.mark.parametrize("route", ROUTES)
def test_rows_at_chunk_and_segment_boundaries(route, ref, monkeypatch):
    env_vars, kernel, per_dispatch = ROUTES[route]
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)  # (the tuning switches are read at tc_env_create)
    obs = route != "no_observation"
    vec = make_env(no_observation=not obs)
    roll = vec.alloc_rollout(K, keys=tuple(k for k in KEYS if obs or k != "obs"))
    vec.drive(None, rollout=roll, steer_noise=caller_noise())
    torch.cuda.synchronize()
    info = vec.launch_info(K)
    assert info["kernel"] == kernel, (route, info)
    if per_dispatch is not None:
        assert info["steps_per_dispatch"] == per_dispatch, (route, info)
    for key, t in roll.items():
        bad = np.flatnonzero((bits(t) != ref["rows"][key]).reshape(K, -1).any(axis=1))
        assert bad.size == 0, (route, key, "rows of steps", bad.tolist())
    final = final_of(vec, obs=False)
    for key, want in ref["final"].items():
        assert np.array_equal(final[key], want), (route, "final", key)
    vec.close()


def test_camera_rows_without_a_bank_are_refused():
    """rows for a feature that is off, the camera bank's (the other three: test_gpu_controller.py, test_gpu_episodes.py,
    test_gpu_drive_randomization.py)"""
    import ctypes as C
    from tinycarlo_amd import _native as nat
    L = nat.lib()
    vec = make_env(no_observation=True)
    vec.randomize_cameras()  # back to the shared camera
    rows = torch.full((K, N), -7, dtype=torch.int32, device="cuda:0")
    sr = nat.StepRows(n_rows=K, camera_out=rows.data_ptr())
    before = final_of(vec, obs=False)
    assert L.tc_step_multi(vec._h, None, nat.F64, None, K, vec._flags(), None, C.byref(sr), vec._stream()) == -1
    assert b"camera rows without a camera bank" in L.tc_last_error()
    after = final_of(vec, obs=False)  # a refused call does nothing
    assert int((rows != -7).sum()) == 0 and all(np.array_equal(after[k], before[k]) for k in before)
    vec.close()
