"""The five-wave frame kernel with the camera's K matrix fetched at the projection and the one-band raster form, on the GPU:
32 envs and 8-step calls against the oracle (portable math), observations and draw-list lengths at tolerance 0.  Extends
tests/test_gpu_frame_lds.py (same map, same comparisons) to what decides where the K matrix comes from and which of the two
kernels runs:

1. shared camera, one band: simple_layout 64x64, thickness 2, streamed and TC_STREAM=0 -- tc_frame_kernel<5, .., 32>, the
   one-band form, K in scalar loads from the argument block.
2. shared camera, several bands: simple_layout 'classes' at 205 rows x 128 columns -- tc_frame_banded.  (64 x 128 is one
   band: a band holds TC_BAND_BYTES = 16384 bytes of bit-planes, 5 layers x 4 words x 4 bytes = 80 per row, 204 rows.  So 205
   rows is the smallest frame of 128 columns with more than one band, and the handle says how many it makes of it.)
   tc_frame_banded stands beside the kernel-variant matrix (tests/test_gpu_variant_matrix.py), so the case runs each of
   its six instantiations: thickness 2 / 1 x class masks / packed class masks / rgb.
3. camera bank: three cameras of clearly different focal lengths (fov 50 / 80 / 120 degrees) and a time limit of 3 steps, so
   the index in entry 12 of the pose rows changes between the rows of one call.
4. per-env cameras: two K matrices (fov 80 / 104) across the envs.
5. recover kernel: the bank of case 3 under TC_STREAM_TEST_SKIP=3 -- tc_frame_recover_kernel draws two or three rows of every
   env in its row loop, with the camera each row came with; a K matrix fetched once in front of that loop would be wrong
   for every env whose recovered rows belong to different episodes.
6. draw list longer than the LDS head: case 1 with TC_SEG_LDS_CAP=3.
"""
import copy
import os

import numpy as np
import pytest

import camera_bank_ref as cbr
import frame_lds_shim as fs
import orc
from common import load_cfg
from test_gpu_parity import make_env, make_oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K = 32, 8
SEED = 21
BANK_FOV = [50, 80, 120]
CAM_SEED = 977
LIMIT = 3
QUEUE_LEN = 8  # (an env re-spawns at most K / LIMIT + 1 times in a call)
MAX_CTE = 10.0  # (of the one termination term the reference carries: never reached -- episodes end by the time limit)


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def actions(seed):
    rng = np.random.default_rng(seed)
    cc = np.stack([rng.uniform(0.3, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2).astype(np.float32)
    return cc, rng.integers(0, 4, (K, N)).astype(np.int32)


def simple_cfg(resolution, fmt="classes", thickness=2):
    cfg, path = load_cfg("simple_layout")
    cfg = copy.deepcopy(cfg)
    cfg["camera"].update(resolution=list(resolution), line_thickness=thickness)
    cfg["sim"]["observation_space_format"] = fmt
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


_refs = {}


def shared(key, make):
    """a reference computed once per key, shared and left unchanged"""
    if key not in _refs:
        val = make()
        for a in val:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[key] = val
    return _refs[key]


def oracle_call(o, nodes, cc, man):
    """K steps of a batch oracle from the reset at `nodes` -> frames [K][N][..], draw-list lengths [K][N]"""
    o.reset(nodes)
    obs, nseg = [], []
    for k in range(K):
        o.step(cc[k].astype(np.float64), man[k])
        obs.append(o.obs.copy())
        nseg.append([len(o.segments(i)[0]) for i in range(N)])
    return np.stack(obs), np.array(nseg)


def check_stats(env, nseg, what):
    """tc_env_draw_list_stats over the call's frames against the reference's draw-list lengths"""
    st = env.draw_list_stats()
    # (a streamed call: all K steps; a chunked one: the steps of the chunks its scratch ring still holds, the last ones)
    rows = st["frames"] // N
    assert st["frames"] == rows * N and K // 2 <= rows <= K, (what, st)
    nseg = nseg[K - rows:]
    assert st["max_segments"] == int(nseg.max()), (what, st, int(nseg.max()))
    assert st["empty_frame_frac"] == float((nseg == 0).sum()) / nseg.size, (what, st)
    assert st["mean_segments_per_frame"] == float(nseg.sum()) / nseg.size, (what, st)


def call_and_compare(env, cc, man, obs, nseg, what, keys=("obs", "cte"), top=255):
    """one K-step call with every frame in a rollout, equal to the reference; -> the rollout"""
    roll = env.alloc_rollout(K, keys=keys)
    env.step_multi(torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda(), rollout=roll)
    torch.cuda.synchronize()
    assert env.launch_info(K)["kernel"].endswith("tc_frame_kernel"), (what, env.launch_info(K))
    got = roll["obs"].cpu().numpy().reshape(K, N, -1)
    bad = np.argwhere((got != obs.reshape(K, N, -1)).any(axis=2))
    assert bad.size == 0, (what, "frames differ at (step, env)", bad[:8].tolist(), nseg[tuple(bad[:8].T)].tolist())
    assert got.max() == 255 if top else got.any(), what
    check_stats(env, nseg, what)
    return roll


def run_shared_camera(env, key, what, packed=False):
    cc, man = actions(13)
    env.reset(seed=SEED)
    nodes = env._keep[0].cpu().numpy()
    obs, nseg = shared(key, lambda: oracle_call(make_oracle(env), nodes, cc, man))
    if packed:  # the packed frame is the packing of the class masks (tinycarlo_amd/packing.py)
        from tinycarlo_amd.packing import pack_bits_reference
        H, W = env.camera.resolution
        obs = pack_bits_reference(obs.reshape(K, N, env.n_classes, H, W)).reshape(K, N, -1)
    # (255: a class mask's set value; packed words and layer colours only have to be there)
    call_and_compare(env, cc, man, obs, nseg, what, top=255 if env.observation_space_format == "classes" and not packed else None)
    return nseg


# ---------------------------------------------------------------------------------------------- 1, 6
@pytest.mark.parametrize("stream", ["1", "0"])
def test_1_shared_camera_one_band(monkeypatch, stream):
    monkeypatch.setenv("TC_STREAM", stream)
    env = make_env("simple_layout", "r64", "classes", N)
    assert env.camera.line_thickness == 2
    info = env.frame_lds_info()
    assert (info["bands"], info["band_rows"]) == (1, 64), info
    nseg = run_shared_camera(env, "r64", f"TC_STREAM={stream}")
    assert nseg.max() > 8  # (more than the smallest head holds: what case 6 relies on)
    env.close()


def test_6_draw_list_longer_than_the_lds_head(monkeypatch):
    monkeypatch.setenv("TC_SEG_LDS_CAP", "3")
    env = make_env("simple_layout", "r64", "classes", N)
    info = env.frame_lds_info()
    assert info["head_entries"] == 8 and info["bands"] == 1, info  # (the frame kernel's floor of 8 entries)
    run_shared_camera(env, "r64", "TC_SEG_LDS_CAP=3")
    env.close()


# ---------------------------------------------------------------------------------------------- 2
H_BANDED, W_BANDED = 205, 128


@pytest.mark.parametrize("fmt", ["classes", "bits", "rgb"])
@pytest.mark.parametrize("thickness", [2, 1])
def test_2_shared_camera_several_bands(thickness, fmt):
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    cfg_fmt = "rgb" if fmt == "rgb" else "classes"
    kw = dict(num_envs=N, device="cuda:0", obs_packing="bits" if fmt == "bits" else None)
    # the arithmetic of the docstring, and the handles' own word: 204 rows are one band, 205 are not
    C_, wpr = 5, W_BANDED // 32
    assert fs.BAND_BYTES // (C_ * wpr * 4) == H_BANDED - 1
    one = TinyCarloVecEnv(simple_cfg([H_BANDED - 1, W_BANDED], cfg_fmt, thickness), **kw)
    assert one.n_classes == C_ and one.frame_lds_info()["bands"] == 1, one.frame_lds_info()
    one.close()
    env = TinyCarloVecEnv(simple_cfg([H_BANDED, W_BANDED], cfg_fmt, thickness), **kw)
    info = env.frame_lds_info()
    assert info["bands"] >= 2 and info["bands"] == -(-H_BANDED // info["band_rows"]), info
    assert env.launch_info(K)["kvar"] == 5, env.launch_info(K)
    run_shared_camera(env, ("banded", thickness, cfg_fmt), f"thickness {thickness} {fmt}: {info['bands']} bands of {info['band_rows']} rows",
                      packed=fmt == "bits")
    env.close()


# ---------------------------------------------------------------------------------------------- 3, 5
def bank_env():
    from tinycarlo_amd import terms as T
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    env = TinyCarloVecEnv(simple_cfg([64, 64]), num_envs=N, device="cuda:0", autoreset=True, spawn="host", spawn_queue_len=QUEUE_LEN)
    env.set_terms([T.cte_termination(MAX_CTE, 1)])
    env.set_time_limit(LIMIT)
    env.randomize_cameras(fov=BANK_FOV, seed=CAM_SEED)
    env.reset(seed=SEED)
    return env


def bank_reference(env, cc, man):
    """tests/camera_bank_ref.py's composed reference on this env's map, spawn nodes and spawn queue -> frames [K][N][..],
    draw-list lengths [K][N], camera index rows [K][N]"""
    from tinycarlo_amd.camera import Camera
    cfg = env.config
    ref = cbr.CameraBankRef(env.map, env.car_params, Camera(copy.deepcopy(cfg["camera"])), orc.FMT_CLASSES,
                            env._keep[0].cpu().numpy(), env._aux["spawn_queue"].cpu().numpy(), MAX_CTE,
                            limit=np.full(N, LIMIT, dtype=np.int64), camera_cfg=cfg["camera"], bank={"fov": BANK_FOV},
                            cam_seed=CAM_SEED)
    ref.reset()
    obs, nseg, cam = [], [], []
    for k in range(K):
        out = ref.step(cc[k].astype(np.float64), man[k])
        obs.append(out["obs"].copy())
        nseg.append([len(o.segments(0)[0]) for o in ref.oracles])
        cam.append(out["camera"].copy())
    return np.stack(obs), np.array(nseg), np.stack(cam)


def run_bank(what):
    env = bank_env()
    assert env.camera_bank_params.shape == (len(BANK_FOV), 7)
    cc, man = actions(17)
    obs, nseg, cam = shared("bank", lambda: bank_reference(env, cc, man))
    # the case tests something: the three K matrices differ, every camera is used, and within the call envs change camera
    Kb = env._cam_bank["K"].cpu().numpy()
    assert len({Kb[i].tobytes() for i in range(len(BANK_FOV))}) == len(BANK_FOV)
    assert set(np.unique(cam)) == set(range(len(BANK_FOV)))
    changed = (cam[1:] != cam[:-1]).any(axis=0)
    assert changed.sum() >= N // 4, ("envs whose camera changes between rows of the call", int(changed.sum()))
    roll = call_and_compare(env, cc, man, obs, nseg, what, keys=("obs", "cte", "camera"))
    assert np.array_equal(roll["camera"].cpu().numpy(), cam), (what, "camera rows")
    env.close()
    return cam, nseg


def test_3_camera_bank():
    run_bank("camera bank")


def test_5_recover_kernel_row_loop(monkeypatch):
    monkeypatch.setenv("TC_STREAM_TEST_SKIP", "3")
    cam, nseg = run_bank("camera bank, TC_STREAM_TEST_SKIP=3")
    # the frames with (row + env) % 3 == 0 were left to tc_frame_recover_kernel: at least two rows of every env, and for some
    # envs rows of different cameras with something to draw in both
    left = (np.arange(K)[:, None] + np.arange(N)[None, :]) % 3 == 0
    assert left.sum(axis=0).min() >= 2
    two_cameras = [i for i in range(N) if len({int(cam[r, i]) for r in range(K) if left[r, i] and nseg[r, i] > 0}) >= 2]
    assert two_cameras, "no env has recovered, non-empty rows of two cameras"


# ---------------------------------------------------------------------------------------------- 4
def test_4_per_env_cameras():
    from tinycarlo_amd.camera import Camera
    env = make_env("simple_layout", "r64", "classes", N)
    fovs = [80, 104]
    pick = (np.arange(N) // 3) % 2  # (runs of three envs: both cameras in every group of eight)
    env.set_env_cameras(fov=[fovs[k] for k in pick])
    Kr = env._env_cams[1].cpu().numpy()
    assert len({Kr[i].tobytes() for i in range(N)}) == 2
    cc, man = actions(19)
    env.reset(seed=SEED)
    nodes = env._keep[0].cpu().numpy()

    def make():
        both = []
        for f in fovs:
            c = copy.deepcopy(env.config["camera"])
            c.update(fov=f)
            both.append(oracle_call(orc.Oracle(env.map, env.car_params, Camera(c), orc.FMT_CLASSES, N, threads=8), nodes, cc, man))
        sel = pick.astype(bool)
        obs = np.where(sel[None, :, None], both[1][0], both[0][0])
        nseg = np.where(sel[None, :], both[1][1], both[0][1])
        assert (both[0][0] != both[1][0]).any()
        return obs, nseg

    obs, nseg = shared("per_env", make)
    call_and_compare(env, cc, man, obs, nseg, "per-env cameras")
    env.close()
