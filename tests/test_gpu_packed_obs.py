"""Bit-packed class-mask observations on the GPU (TinyCarloVecEnv(obs_packing="bits"), TC_FMT_CLASSES_BITS) and the device
unpack kernel (tinycarlo_amd.unpack_obs, tc_unpack_bits).

Bar: a packed frame is, byte for byte, pack_bits_reference() of the frame the CPU oracle draws (the oracle has no packed
format), every other rollout row stays bit-identical to the oracle as in test_gpu_bench_shapes, and unpack_obs equals
unpack_bits_reference exactly.  Every buffer the kernels store a frame into is filled with 0xFF first, so a byte a kernel
leaves unwritten shows."""
import numpy as np
import pytest

import orc
from common import load_cfg
from test_gpu_bench_shapes import check_rows_against_oracle, mixed_actions
from test_gpu_parity import assert_same, make_env, make_oracle

from tinycarlo_amd.packing import pack_bits_reference, unpack_bits_reference

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


class FrameRecorder:
    """the oracle, always rendering, keeping a copy of the byte frames [n, C, H, W] of every step"""

    def __init__(self, o, shape):
        self._o, self._shape, self.frames = o, shape, []

    def __getattr__(self, k):
        return getattr(self._o, k)

    def step(self, cc, man, flags=0, with_obs=True):
        self._o.step(cc, man, flags=flags, with_obs=True)
        self.frames.append(self._o.obs.reshape(self._shape).copy())


def byte_shape(env):
    H, W = env.camera.resolution
    return (env.num_envs, env.n_classes, H, W)


def alloc_ff(env, K):
    roll = env.alloc_rollout(K, keys="all")
    roll["obs"].fill_(0xFF)
    return roll


def packed_rollout_case(map_name, n, K, seed, camera=None, want_zero_paths=False):
    """one K-step call of a packed env with autoreset against the oracle -> (env info, packed rollout obs on the host,
    the oracle's byte frames [K, n, C, H, W])"""
    env = make_env(map_name, "r64", "classes", n, autoreset=True, spawn_queue_len=16, obs_packing="bits", camera=dict(camera or {}))
    H, W = env.camera.resolution
    assert env.obs_bytes_per_env == env.n_classes * H * W // 8 and env._obs_shape == (env.n_classes, H, W // 8)
    env.reset(seed=seed)
    o = make_oracle(env, threads=16)
    o.reset(env._keep[0].cpu().numpy())
    o.spawn_queue = env._aux["spawn_queue"].cpu().numpy()
    if want_zero_paths:
        # Cars that start on the road keep some lane line in view for hundreds of steps of these actions (counted on the CPU
        # oracle: not one empty frame in 160 steps), so every fourth env starts 80 m beside the map: its frames are empty
        # until it terminates and is re-spawned, which takes from one step to the whole call.
        sel = np.arange(n) % 4 == 1
        for k in ("x", "front_x"):
            o.state[k][sel] += 80.0
            env.state[k].copy_(torch.from_numpy(np.ascontiguousarray(o.state[k])))
    rec = FrameRecorder(o, byte_shape(env))
    roll = alloc_ff(env, K)
    cc, man = mixed_actions(n, K, seed=seed + 1)
    env.step_multi(cc, man, rollout=roll)
    torch.cuda.synchronize()
    label = f"packed {map_name} {H}x{W}"
    check_rows_against_oracle(env, rec, cc, man, {k: v for k, v in roll.items() if k != "obs"}, orc.F_AUTORESET, label)
    frames = np.stack(rec.frames)
    got = roll["obs"].cpu().numpy()
    want = pack_bits_reference(frames)
    assert got.shape == want.shape == (K, n, env.n_classes, H, W // 8)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).reshape(K, n, -1).any(axis=2))
        raise AssertionError((label, "packed frames differ at (step, env)", bad[:8].tolist(), int((got != want).sum())))
    assert_same(env, o, env.n_classes, check_obs=False, label=label + " bound buffers")
    if want_zero_paths:
        drawn = frames.reshape(K, n, env.n_classes, -1).any(axis=3)  # [K, n, C]: the plane has a pixel
        assert (~drawn.any(axis=2)).any(), (label, "no empty frame in the input: the nseg == 0 path is not tested")
        assert (drawn.any(axis=2) & ~drawn.all(axis=2)).any(), (label, "no frame with an empty plane beside a drawn one")
    info = (env.launch_info(K), env.launch_info(1))
    env.close()
    return info, got, frames


KNUFFINGEN_RES = list(load_cfg("knuffingen")[0]["camera"]["resolution"])

STREAMED_CASES = [
    # wpr 2: the dense case, planes and frames 16-byte aligned
    pytest.param("simple_layout", 256, 12, 3, {"resolution": [64, 64]}, id="simple_layout-64x64"),
    # wpr 5: the LDS planes are not 16-byte aligned (band_rows * 5 words); the K = 9 kernel
    pytest.param("knuffingen", 64, 6, 4, {"resolution": KNUFFINGEN_RES}, id="knuffingen-128x160"),
    # plane = 744 B, frame = 3720 B: destinations that are not 16-byte aligned
    pytest.param("simple_layout", 64, 6, 5, {"resolution": [62, 96]}, id="simple_layout-62x96"),
    # the THICK = false variant
    pytest.param("simple_layout", 64, 6, 6, {"resolution": [64, 64], "line_thickness": 1}, id="simple_layout-64x64-thin"),
]


@pytest.mark.parametrize("map_name,n,K,seed,camera", STREAMED_CASES)
def test_streamed_step_multi(map_name, n, K, seed, camera):
    assert KNUFFINGEN_RES == [128, 160]
    (info_k, _), _, _ = packed_rollout_case(map_name, n, K, seed, camera=camera, want_zero_paths=True)
    assert info_k["kernel"].endswith("+tc_frame_kernel") and not info_k["fused"], info_k


@pytest.mark.parametrize("switch", [{}, {"TC_BAND_BYTES": "2048"}, {"TC_STREAM": "0"}, {"TC_STREAM_TEST_SKIP": "3"}, {"TC_FUSE": "0"},
                                    {"TC_MULTI_SPLIT": "0"}],
                         ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "defaults")
def test_library_switches(switch, monkeypatch):
    for k, v in switch.items():
        monkeypatch.setenv(k, v)
    (info_k, info_1), _, _ = packed_rollout_case("simple_layout", 128, 10, 8, camera={"resolution": [64, 64]})
    assert "tc_step_kernel" not in info_k["kernel"] and not info_k["fused"], info_k
    assert "tc_step_kernel" not in info_1["kernel"] and not info_1["fused"], info_1
    if switch.get("TC_FUSE") == "0":
        assert info_k["kernel"] == "tc_env_kernel+tc_raster_kernel", info_k
    else:
        assert info_k["kernel"] == "tc_envg_kernel+tc_frame_kernel", info_k


def test_single_step_entry_points_on_the_bound_buffer():
    n = 96
    env = make_env("simple_layout", "r64", "classes", n, obs_packing="bits")
    o = make_oracle(env, threads=8)
    shape = byte_shape(env)
    info = env.launch_info(1)
    assert info["kernel"] == "tc_env_kernel+tc_raster_kernel" and not info["fused"], info

    def same_frames(label):
        torch.cuda.synchronize()
        got, want = env.out["obs"].cpu().numpy(), pack_bits_reference(o.obs.reshape(shape))
        assert np.array_equal(got, want), (label, np.flatnonzero((got != want).reshape(n, -1).any(axis=1))[:8])

    env.out["obs"].fill_(0xFF)
    env.reset(seed=12)
    o.reset(env._keep[0].cpu().numpy())
    same_frames("reset")
    rng = np.random.default_rng(3)
    for k in range(5):
        cc = np.stack([rng.uniform(0.3, 1, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
        man = rng.integers(0, 4, n).astype(np.int32)
        env.out["obs"].fill_(0xFF)
        env.step({"car_control": cc, "maneuver": man})
        o.step(cc.astype(np.float64), man)
        assert_same(env, o, env.n_classes, check_obs=False, label=f"step {k}")
        same_frames(f"step {k}")
    # masked reset: the frames of the envs outside the mask are not touched
    mask = rng.integers(0, 2, n).astype(bool)
    mask[:2] = (True, False)
    env.out["obs"].fill_(0xFF)
    env.reset(mask=mask)
    o.reset(env._keep[0].cpu().numpy(), mask=mask.astype(np.uint8))
    torch.cuda.synchronize()
    got, want = env.out["obs"].cpu().numpy(), pack_bits_reference(o.obs.reshape(shape))
    assert np.array_equal(got[mask], want[mask])
    assert (got[~mask] == 0xFF).all()
    # render: the frame of the current state again, every env
    env.out["obs"].fill_(0xFF)
    env.render_current()
    same_frames("render")
    env.close()


def test_byte_env_and_packed_env_agree_under_noise():
    """two envs in one process, same seed, same blob stream: pack(byte frame) == packed frame, single steps and a K-step call"""
    n, K = 64, 8
    a = make_env("simple_layout", "r64", "classes", n, autoreset=True)
    b = make_env("simple_layout", "r64", "classes", n, autoreset=True, obs_packing="bits")
    for e in (a, b):
        e.set_noise(3, 20, 77)
        e.reset(seed=31)
    rng = np.random.default_rng(9)
    for k in range(8):
        cc = np.stack([rng.uniform(0.3, 1, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
        man = rng.integers(0, 4, n).astype(np.int32)
        b.out["obs"].fill_(0xFF)
        a.step({"car_control": cc, "maneuver": man})
        b.step({"car_control": cc, "maneuver": man})
        torch.cuda.synchronize()
        assert np.array_equal(pack_bits_reference(a.out["obs"]), b.out["obs"].cpu().numpy()), ("single step", k)
    ra, rb = a.alloc_rollout(K, keys="all"), alloc_ff(b, K)
    cc, man = mixed_actions(n, K, seed=2)
    a.step_multi(cc, man, rollout=ra)
    b.step_multi(cc, man, rollout=rb)
    torch.cuda.synchronize()
    assert int(ra["obs"].max()) == 255
    assert np.array_equal(pack_bits_reference(ra["obs"]), rb["obs"].cpu().numpy())
    for k in ra:
        if k != "obs":
            x, y = ra[k], rb[k]
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert torch.equal(x, y), k
    # unpack_obs of the packed rollout is the byte env's rollout
    from tinycarlo_amd import unpack_obs
    assert torch.equal(unpack_obs(rb["obs"], torch.uint8), ra["obs"])
    assert torch.equal(b.unpack_obs(rb["obs"], torch.uint8), ra["obs"])
    # the stand-alone noise pass is out of scope for packed frames and says so
    from tinycarlo_amd import _native as nat
    with pytest.raises(nat.NativeError, match="tc_noise"):
        b.apply_noise()
    a.close()
    b.close()


UNPACK_SHAPE = (37, 5, 62, 96 // 8)
DTYPES = [torch.uint8, torch.float16, torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def random_packed():
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, UNPACK_SHAPE, dtype=np.uint8)
    host[3] = 0
    host[4] = 0xFF
    return host, torch.from_numpy(host).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_unpack_obs_on_random_bytes(random_packed, dtype):
    from tinycarlo_amd import unpack_obs
    host, dev = random_packed
    want = unpack_bits_reference(host, 96, dtype)
    got = unpack_obs(dev, dtype)
    torch.cuda.synchronize()
    assert got.dtype == dtype and tuple(got.shape) == (37, 5, 62, 96)
    assert torch.equal(got.cpu(), want)
    # leading axes beyond one: a [K][N] rollout is K * N frames
    got2 = unpack_obs(dev[:36].reshape(4, 9, 5, 62, 12), dtype)
    assert tuple(got2.shape) == (4, 9, 5, 62, 96) and torch.equal(got2.cpu().reshape(36, 5, 62, 96), want[:36])
    # a shuffled index with repeats, into a pre-filled `out`
    idx_h = np.random.default_rng(6).integers(0, 37, 50)
    idx_h[:3] = (7, 7, 36)
    idx = torch.from_numpy(idx_h).cuda()
    out = torch.full((50, 5, 62, 96), 7, dtype=dtype, device="cuda:0")
    r = unpack_obs(dev, dtype, index=idx, out=out)
    assert r is out
    assert torch.equal(out.cpu(), want[torch.from_numpy(idx_h)])
    # an index outside [0, 37) gives a frame of zeros; the frames around it are not disturbed
    idx_bad = torch.tensor([2, 37, -1, 1 << 40, 5], dtype=torch.int64, device="cuda:0")
    out = torch.full((5, 5, 62, 96), 7, dtype=dtype, device="cuda:0")
    unpack_obs(dev, dtype, index=idx_bad, out=out)
    oc = out.cpu()
    assert torch.equal(oc[0], want[2]) and torch.equal(oc[4], want[5])
    assert (oc[1:4].to(torch.float32) == 0).all()
    # nothing asked for
    empty = unpack_obs(dev, dtype, index=torch.empty(0, dtype=torch.int64, device="cuda:0"))
    assert tuple(empty.shape) == (0, 5, 62, 96) and empty.dtype == dtype
    # a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got3 = unpack_obs(dev, dtype, index=idx)
    s.synchronize()
    assert torch.equal(got3.cpu(), want[torch.from_numpy(idx_h)])


def test_unpack_obs_checks_its_arguments(random_packed):
    from tinycarlo_amd import unpack_obs
    _, dev = random_packed
    with pytest.raises(ValueError):
        unpack_obs(dev.cpu())
    with pytest.raises(ValueError):
        unpack_obs(dev.to(torch.int32))
    with pytest.raises(ValueError):
        unpack_obs(dev.transpose(0, 1))
    with pytest.raises(ValueError):
        unpack_obs(dev, torch.float64)
    with pytest.raises(ValueError):
        unpack_obs(dev[..., :10])                  # W = 80: no multiple of 32 (and not contiguous)
    with pytest.raises(ValueError):
        unpack_obs(dev, index=torch.zeros(3, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        unpack_obs(dev, index=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        unpack_obs(dev, out=torch.empty((37, 5, 62, 96), dtype=torch.float16, device="cuda:0"))


def test_packed_call_and_unpack_in_one_graph():
    """a prepared packed 4-step call followed by unpack_obs into a fixed tensor, captured once and replayed with new
    actions; a twin env does the same eagerly"""
    from tinycarlo_amd import unpack_obs
    n, K = 96, 4
    a = make_env("simple_layout", "r64", "classes", n, autoreset=True, obs_packing="bits")
    b = make_env("simple_layout", "r64", "classes", n, autoreset=True, obs_packing="bits")
    a.reset(seed=7)
    b.reset(seed=7)
    cc, man = mixed_actions(n, K, seed=3)
    ra, rb = alloc_ff(a, K), alloc_ff(b, K)
    out_a = torch.full((K, n) + byte_shape(a)[1:], 7, dtype=torch.float16, device="cuda:0")
    call = a.prepare_step_multi(cc, man, ra)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
        unpack_obs(ra["obs"], torch.float16, out=out_a)
    for rep in range(2):
        c2, m2 = mixed_actions(n, K, seed=30 + rep)
        cc.copy_(c2)
        man.copy_(m2)
        g.replay()
        b.step_multi(cc, man, rollout=rb)
        out_b = unpack_obs(rb["obs"], torch.float16)
        torch.cuda.synchronize()
        for k in ra:
            x, y = ra[k], rb[k]
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert torch.equal(x, y), ("replay", rep, k)
        assert torch.equal(out_a, out_b), ("replay", rep)
        assert torch.equal(out_a.cpu(), unpack_bits_reference(rb["obs"], 64, torch.float16)), ("replay", rep)
        assert float(out_a.max()) == 1.0
    a.close()
    b.close()
