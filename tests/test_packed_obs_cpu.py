"""Bit-packed class-mask observations (TC_FMT_CLASSES_BITS), the parts that need no GPU: the layout's executable
definition (tinycarlo_amd/packing.py), the argument checks of tc_unpack_bits and of the env's constructor, the constants,
and the compiler's resource figures of the packed kernels."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import yaml

import common
from tinycarlo_amd.config import bundled_config

torch = pytest.importorskip("torch")

DTYPES = [torch.uint8, torch.float16, torch.bfloat16, torch.float32]


def test_pack_reference_is_numpy_packbits_little():
    from tinycarlo_amd.packing import pack_bits_reference
    rng = np.random.default_rng(0)
    for shape in [(5, 62, 96), (3, 4, 1, 32), (2, 7, 160)]:
        m = rng.integers(0, 2, shape).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)  # any non-zero = set
        want = np.packbits(m != 0, axis=-1, bitorder="little")
        got = pack_bits_reference(m)
        assert got.dtype == np.uint8 and got.shape == shape[:-1] + (shape[-1] // 8,)
        assert np.array_equal(got, want)
        assert np.array_equal(pack_bits_reference(torch.from_numpy(m)), want)


def test_lone_pixel_at_x9_sets_bit_1_of_byte_1():
    from tinycarlo_amd.packing import pack_bits_reference
    m = np.zeros((1, 2, 32), dtype=np.uint8)
    m[0, 1, 9] = 255
    p = pack_bits_reference(m)
    want = np.zeros((1, 2, 4), dtype=np.uint8)
    want[0, 1, 1] = 0b00000010
    assert np.array_equal(p, want)
    # ... and the row's bytes are the little-endian 32-bit word with bit 9 set: the kernels' LDS bit-plane word
    assert p[0, 1].view("<u4")[0] == 1 << 9


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_round_trip(dtype):
    from tinycarlo_amd.packing import pack_bits_reference, unpack_bits_reference
    rng = np.random.default_rng(1)
    m = (rng.integers(0, 2, (3, 5, 6, 64)) * 255).astype(np.uint8)
    u = unpack_bits_reference(pack_bits_reference(m), 64, dtype)
    assert u.dtype == dtype and tuple(u.shape) == m.shape
    if dtype == torch.uint8:
        assert np.array_equal(u.numpy(), m)
    else:
        assert torch.equal(u, (torch.from_numpy(m).to(torch.float32) / 255).to(dtype))  # pre_obs of the consumers
        assert set(u.to(torch.float32).unique().tolist()) == {0.0, 1.0}
    assert np.array_equal(pack_bits_reference(u.to(torch.float32).numpy()), pack_bits_reference(m))


def test_constants_and_header():
    from tinycarlo_amd import _native as nat
    with open(os.path.join(common.ROOT, "include", "tinycarlo_hip.h")) as f:
        h = f.read()
    assert re.search(r"^#define TC_HAS_PACKED_OBS 1$", h, re.M)
    assert re.search(r"^#define TC_FMT_CLASSES_BITS 2$", h, re.M)
    assert nat.FMT_CLASSES_BITS == 2 and nat.HAS_PACKED_OBS == 1
    for name, v in (("TC_F32", nat.F32), ("TC_U8", nat.U8), ("TC_F16", nat.F16), ("TC_BF16", nat.BF16)):
        assert re.search(r"^#define %s %d$" % (name, v), h, re.M), name
    assert "tc_unpack_bits" in nat.EXPORTS and "int tc_unpack_bits(" in h


def test_unpack_bits_refuses_bad_arguments_without_a_gpu():
    """every check of tc_unpack_bits comes before its first HIP call: the pointers below are host memory and are never
    dereferenced"""
    from tinycarlo_amd import _native as nat
    L = nat.lib()
    src = np.zeros(4096, dtype=np.uint8)
    dst = np.zeros(8192 + 16, dtype=np.uint8)
    ps = src.ctypes.data
    pd = (dst.ctypes.data + 15) // 16 * 16
    idx = np.zeros(4, dtype=np.int64).ctypes.data
    good = dict(packed=ps, n_src=4, planes=2, H=4, W=32, index=None, n_out=4, dst=pd, dt=nat.U8)

    def call(**over):
        a = dict(good, **over)
        return L.tc_unpack_bits(a["packed"], a["n_src"], a["planes"], a["H"], a["W"], a["index"], a["n_out"], a["dst"], a["dt"], None)

    bad = [dict(packed=None), dict(dst=None), dict(W=48), dict(W=0), dict(W=-32), dict(H=0), dict(planes=0), dict(planes=-1),
           dict(n_src=0), dict(n_src=-3), dict(dt=nat.F64), dict(dt=5), dict(dt=-1), dict(n_out=-1), dict(n_out=5),
           dict(n_out=-1, index=idx)]
    for over in bad:
        assert call(**over) == -1, over
        assert b"tc_unpack_bits" in L.tc_last_error(), over
    # nothing to do is fine, and launches nothing (no device is needed for it)
    assert call(n_out=0) == 0
    assert call(n_out=0, index=idx) == 0


def _cfg(fmt="classes", res=(64, 64)):
    path = bundled_config("config_simple_layout.yaml")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = list(res)
    cfg["sim"]["observation_space_format"] = fmt
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


def test_constructor_refuses_what_cannot_be_packed(monkeypatch):
    """the three ValueErrors come before any device work"""
    from tinycarlo_amd.vec_env import TinyCarloVecEnv

    def no_device(self):
        raise AssertionError("_setup_device reached")
    monkeypatch.setattr(TinyCarloVecEnv, "_setup_device", no_device)
    with pytest.raises(ValueError, match="classes"):
        TinyCarloVecEnv(_cfg("rgb"), num_envs=2, device="cuda:0", obs_packing="bits")
    with pytest.raises(ValueError, match="multiple of 32"):
        TinyCarloVecEnv(_cfg("classes", (64, 80)), num_envs=2, device="cuda:0", obs_packing="bits")
    with pytest.raises(ValueError, match="rgb_array"):
        TinyCarloVecEnv(_cfg("classes"), num_envs=2, device="cuda:0", obs_packing="bits", render_mode="rgb_array")
    with pytest.raises(ValueError, match="obs_packing"):
        TinyCarloVecEnv(_cfg("classes"), num_envs=2, device="cuda:0", obs_packing="bytes")


def test_packed_env_shapes_follow(monkeypatch):
    from tinycarlo_amd import _native as nat
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    monkeypatch.setattr(TinyCarloVecEnv, "_setup_device", lambda self: None)
    env = TinyCarloVecEnv(_cfg("classes", (62, 96)), num_envs=3, device="cuda:0", obs_packing="bits")
    assert env.obs_packing == "bits" and env._fmt == nat.FMT_CLASSES_BITS
    assert env._obs_shape == (env.n_classes, 62, 12) and env.single_observation_space.shape == env._obs_shape
    assert env._rollout_shapes(4)["obs"][0] == (4, 3, env.n_classes, 62, 12)
    plain = TinyCarloVecEnv(_cfg("classes", (62, 96)), num_envs=3, device="cuda:0")
    assert plain.obs_packing is None and plain._obs_shape == (plain.n_classes, 62, 96)


def test_packed_kernels_do_not_spill():
    seen = common.dev_kernel_resources(("-DTC_DEV_FMTV=2",))  # the dev set with the packed frame / raster kernels
    # tc_frame_kernel<K, THICK, FMT = 2, RB> and tc_raster_kernel<THICK, FMT = 2>
    frame = [n for n in seen if re.match(r"_Z\d+tc_frame_kernelILi\d+ELb[01]ELi2ELi\d+EEv9FrameArgs$", n)]
    raster = [n for n in seen if re.match(r"_Z\d+tc_raster_kernelILb[01]ELi2EEv5RArgs$", n)]
    assert len(frame) == 1 and len(raster) == 1, sorted(seen)
    for n in frame + raster:
        vgpr, spill, scratch = seen[n]
        assert spill == 0 and scratch == 0, (n, seen[n])
        assert vgpr <= 128, (n, vgpr)
    # the packed dev build has no fused step kernel of format 2: that family has no packed variant
    assert not [n for n in seen if re.match(r"_Z\d+tc_(drive_)?step_kernelILi\d+ELb[01]ELi2E", n)], sorted(seen)
    unpack = [n for n in seen if re.match(r"_Z\d+tc_unpack_bits_kernelILi\d+EEv", n)]
    assert len(unpack) == 4, sorted(seen)
    for n in unpack:
        _, spill, scratch = seen[n]
        assert spill == 0 and scratch == 0, (n, seen[n])
