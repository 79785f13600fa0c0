"""The raster stage's item dealing by scan (tc_deal.h, raster_body<.., FORM>) on the GPU: the five-wave frame kernel, its
banded form and its recover kernel against the oracle (portable math) at tolerance 0, 32 envs and 4-step calls.

  two-edge form      simple_layout 64x64, thickness 2 (the benchmark's kernel), streamed and chunked calls
  four-edge form     thickness 3 and 8: two table entries per lane
  several passes     poses and cameras of tests/golden/camera_sweep.* that look along a straight, drawn by render_poses (the
                     same frame kernel): a frame with more than 64 outline chunks AND more than 64 fill rows in one batch of
                     32 segments -- asserted from the oracle's draw list with a lower bound (segments whose quad lies inside
                     the image: no clipping, so an outline edge is as long as the segment and the fill spans its rows) -- and
                     a frame of more than 32 segments, which is a second batch
  head overflow      TC_SEG_LDS_CAP=3: a head of 8 entries, every longer list through the refill path in batches of 8
  banded kernel      205 x 128: tc_frame_banded, the band loop
  recover path       TC_STREAM_TEST_SKIP=3: every third frame is left to tc_frame_recover_kernel
"""
import copy
import json
import os

import numpy as np
import pytest

import orc
from common import GOLDEN, RES, golden, load_cfg
from test_gpu_parity import _oracle_frames, _states_from, make_env, make_oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K = 32, 4
SEED = 33
LCH = 8  # outline steps per chunk (k_common.h)


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def actions():
    rng = np.random.default_rng(29)
    cc = np.stack([rng.uniform(0.3, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2).astype(np.float32)
    return cc, rng.integers(0, 4, (K, N)).astype(np.int32)


_refs = {}


def reference(key, env, cc, man):
    """the oracle's K frames [K][N][..] and draw-list lengths [K][N] from the env's reset: computed once per key, read-only"""
    if key not in _refs:
        o = make_oracle(env)
        o.reset(env._keep[0].cpu().numpy())
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


def run_call(env, key, what):
    cc, man = actions()
    env.reset(seed=SEED)
    obs, nseg = reference(key, env, cc, man)
    roll = env.alloc_rollout(K, keys=("obs", "cte"))
    env.step_multi(torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda(), rollout=roll)
    torch.cuda.synchronize()
    assert env.launch_info(K)["kernel"].endswith("tc_frame_kernel"), (what, env.launch_info(K))
    assert env.launch_info(K)["kvar"] == 5, (what, env.launch_info(K))
    got = roll["obs"].cpu().numpy().reshape(K, N, -1)
    bad = np.argwhere((got != obs.reshape(K, N, -1)).any(axis=2))
    assert bad.size == 0, (what, "frames differ at (step, env)", bad[:8].tolist(), nseg[tuple(bad[:8].T)].tolist())
    assert got.max() == 255, what
    return nseg


def simple_cfg(resolution, thickness):
    cfg, path = load_cfg("simple_layout")
    cfg = copy.deepcopy(cfg)
    cfg["camera"].update(resolution=list(resolution), line_thickness=thickness)
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


# ---------------------------------------------------------------------------------------------- the two forms, both call forms
@pytest.mark.parametrize("stream", ["1", "0"])
def test_two_edge_form(monkeypatch, stream):
    monkeypatch.setenv("TC_STREAM", stream)
    env = make_env("simple_layout", "r64", "classes", N)
    assert env.camera.line_thickness == 2 and env.frame_lds_info()["bands"] == 1
    nseg = run_call(env, "r64", f"thickness 2, TC_STREAM={stream}")
    assert nseg.max() > 8  # (longer than the smallest head: what the head-overflow case relies on)
    env.close()


@pytest.mark.parametrize("stream", ["1", "0"])
@pytest.mark.parametrize("thickness", [3, 8])
def test_four_edge_form(monkeypatch, thickness, stream):
    monkeypatch.setenv("TC_STREAM", stream)
    env = make_env("simple_layout", "r64", "classes", N, camera={"line_thickness": thickness})
    assert env.frame_lds_info()["bands"] == 1
    run_call(env, ("r64", thickness), f"thickness {thickness}, TC_STREAM={stream}")
    env.close()


# ---------------------------------------------------------------------------------------------- refill and recover
def test_head_overflow(monkeypatch):
    monkeypatch.setenv("TC_SEG_LDS_CAP", "3")
    env = make_env("simple_layout", "r64", "classes", N)
    assert env.frame_lds_info()["head_entries"] == 8, env.frame_lds_info()  # (the frame kernel's floor)
    nseg = run_call(env, "r64", "TC_SEG_LDS_CAP=3")
    assert nseg.max() > 16  # (three batches of 8 and more)
    env.close()


def test_recover_path(monkeypatch):
    monkeypatch.setenv("TC_STREAM_TEST_SKIP", "3")
    env = make_env("simple_layout", "r64", "classes", N)
    nseg = run_call(env, "r64", "TC_STREAM_TEST_SKIP=3")
    left = (np.arange(K)[:, None] + np.arange(N)[None, :]) % 3 == 0
    assert (nseg[left] > 0).sum() >= 8  # (frames with something to draw were left to the recover kernel)
    env.close()


@pytest.mark.parametrize("thickness", [2, 3])
def test_banded_kernel(thickness):
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    env = TinyCarloVecEnv(simple_cfg([205, 128], thickness), num_envs=N, device="cuda:0")
    info = env.frame_lds_info()
    assert info["bands"] >= 2, info  # (tc_frame_banded: frame_kernel_of sends every looped K = 5 handle there)
    run_call(env, ("banded", thickness), f"205 x 128, thickness {thickness}: {info['bands']} bands")
    env.close()


# ---------------------------------------------------------------------------------------------- several passes, a second batch
def batch_lower_bounds(seg, H, W):
    """per batch of 32 entries of a draw list: (outline chunks, fill rows) the batch has AT LEAST.  Counted over segments that
    lie 4 px inside the image (ThickLine's quad and its outline then are not clipped): each of the two long outline edges is
    the segment moved by dp, max(|dx|, |dy|) steps up to one of rounding, in chunks of LCH; the fill spans the segment's rows."""
    out = []
    for b in range(0, len(seg), 32):
        s = np.asarray(seg[b:b + 32], dtype=np.int64)
        x0, y0, x1, y1 = s[:, 1], s[:, 2], s[:, 3], s[:, 4]
        ln = np.maximum(np.abs(x1 - x0), np.abs(y1 - y0))
        ok = (np.minimum(x0, x1) >= 4) & (np.maximum(x0, x1) < W - 4) & (np.minimum(y0, y1) >= 4) & (np.maximum(y0, y1) < H - 4) & (ln > 0)
        out.append((int((2 * ((ln[ok] - 1 + LCH) // LCH)).sum()), int(np.abs(y1 - y0)[ok].sum())))
    return out


@pytest.mark.parametrize("pi,res,thickness,want", [(14, [64, 64], 2, "passes"), (14, [128, 160], 3, "passes"), (3, [64, 64], 2, "batches")])
def test_several_passes_and_batches(pi, res, thickness, want):
    with open(os.path.join(GOLDEN, "camera_sweep.json")) as f:
        meta = json.load(f)
    ps = meta["sets"][pi]
    steps = meta["maps"]["simple_layout"]["steps"]
    post = _states_from(golden(meta["maps"]["simple_layout"]["rollout"]), "post_")[steps]
    S = len(steps)
    RES["deal"] = list(res)
    env = make_env("simple_layout", "deal", "classes", S,
                   camera=dict(position=list(ps["position"]), max_range=ps["max_range"], line_thickness=thickness))
    env.camera.orientation = list(ps["orientation"])
    env.camera.fov = ps["fov"]
    env.camera.update_params()
    assert env.frame_lds_info()["bands"] == 1 and env.launch_info(K)["kvar"] == 5
    o = make_oracle(env)
    o.state[:] = post
    _oracle_frames(o)
    segs = [np.asarray(o.segments(i)[0]) for i in range(S)]
    if want == "passes":  # one batch whose outline AND fill take more than one pass of 64 items
        lb = [b for s in segs if len(s) for b in batch_lower_bounds(s, res[0], res[1])]
        assert any(c > 64 and r > 64 for c, r in lb), max(lb, key=min)
    else:
        assert max(len(s) for s in segs) > 32, [len(s) for s in segs]
    x, y, th = (torch.from_numpy(np.ascontiguousarray(post[k], dtype=np.float64)).cuda() for k in ("x", "y", "theta"))
    got = env.render_poses(x, y, th)
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(S, -1)
    bad = np.flatnonzero((got != o.obs).any(axis=1))
    assert bad.size == 0, ("frames differ at poses", bad.tolist(), [len(segs[i]) for i in bad])
    assert got.max() == 255
    env.close()
