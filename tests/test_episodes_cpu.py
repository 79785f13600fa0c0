"""CPU checks of the episode time limit / statistics API: header, binding and library agree, the argument validation
that needs no device, set_time_limit's input checks, and the compiler's resource figures of the kernels with the episode bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import HIPCC, ROOT, TC_FEAT_CAR, TC_FEAT_EP, assert_one_variant_set, dev_kernel_resources, kernel_variant
from tinycarlo_amd import _native as nat

NEW = ("tc_env_set_episodes",)


def _header():
    return open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()


def test_header_binding_and_library_agree():
    h = _header()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (TC_\w+) (-?\d+)\s", h, re.M)}
    assert d["TC_ABI_VERSION"] == nat.ABI_VERSION == 7
    assert d["TC_HAS_EPISODES"] == nat.HAS_EPISODES == 1
    assert d["TC_S_TIME_LIMIT"] == nat.S_TIME_LIMIT == 32
    others = [v for k, v in d.items() if k.startswith("TC_S_") and k != "TC_S_TIME_LIMIT"]
    assert all(v & 32 == 0 for v in others) and max(others) == 16  # the next free status bit
    L = nat.lib()
    for f in NEW:
        assert f in nat.EXPORTS and re.search(r"\bint " + f + r"\(", h) and hasattr(L, f)
    assert L.tc_abi_version() == 7


def test_struct_size_equals_the_headers_field_count():
    h = _header()
    body = re.search(r"typedef struct \{([^}]*)\} tc_episode_buffers;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for f in body.split(";") if f.strip()]
    assert all("*" in f for f in fields)  # pointers only
    assert len(fields) == len(nat.EpisodeBuffers._fields_) == 8
    assert C.sizeof(nat.EpisodeBuffers) == 8 * len(fields)
    names = [re.search(r"(\w+)\s*$", f).group(1) for f in fields]
    assert names == [n for n, _ in nat.EpisodeBuffers._fields_]
    # the structs out-of-tree callers were compiled against did not grow
    assert C.sizeof(nat.Buffers) == 23 * 8 + 8 and C.sizeof(nat.Rollout) == 15 * 8


def test_argument_validation_needs_no_device():
    L = nat.lib()
    assert L.tc_env_set_episodes(None, None, 0) == -1  # TC_E_INVALID
    assert L.tc_env_set_episodes(None, None, 100) == -1
    b = nat.EpisodeBuffers()  # length / ret missing: refused before the handle is looked at
    assert L.tc_env_set_episodes(None, C.byref(b), 10) == -1
    assert b"length and ret are required" in L.tc_last_error()
    # the episode rows are arguments of the K-step call (tc_step_rows): NULL handle, and a bad n_rows whatever the handle is
    dummy = C.c_void_p(256)  # (never dereferenced: the struct is refused first)

    def multi(n_steps, **kw):
        rows = nat.StepRows(**kw)
        return L.tc_step_multi(None, None, nat.F64, None, n_steps, 0, None, C.byref(rows), None)
    assert multi(1) == -1 and multi(1, n_rows=4, episode_length_out=dummy) == -1
    assert multi(1, n_rows=-1) == -1 and b"n_rows" in L.tc_last_error()
    for member in ("episode_length_out", "episode_return_out"):
        assert multi(1, n_rows=0, **{member: dummy}) == -1 and b"n_rows = 0" in L.tc_last_error()
        assert multi(5, n_rows=4, **{member: dummy}) == -1 and b"rows" in L.tc_last_error()


def _host_env(n=4):
    from oracle_backend import OracleVecEnv
    from tinycarlo_amd.config import bundled_config
    return OracleVecEnv(bundled_config("config_simple_layout.yaml"), num_envs=n)


def test_set_time_limit_rejects_bad_input():
    env = _host_env(4)
    assert env.episode_stats is None
    for bad in (-1, 2.5, "10", True):
        with pytest.raises(ValueError):
            env.set_time_limit(bad)
    for bad in ([1, 2, 3], [1, 2, 3, -4], [1.0, 2.0, 3.0, 4.0], np.ones((2, 2), np.int32)):
        with pytest.raises(ValueError):
            env.set_time_limit(10, per_env=bad)
    import torch
    with pytest.raises(ValueError):
        env.set_time_limit(None, per_env=torch.ones(4))
    with pytest.raises(ValueError):
        env.alloc_rollout(2, keys=("episode_length",))  # needs tracking
    assert env.episode_stats is None  # nothing was switched on by a refused call
    assert "episode_length" not in env.alloc_rollout(2, keys="all")
    env.reset(seed=0)
    _, _, _, _, info = env.step({"car_control": np.zeros((4, 2), np.float32), "maneuver": np.zeros(4, np.int32)})
    assert "episode_length" not in info and "episode_return" not in info  # existing users' key set is unchanged
    assert "episodes" in env.state_dict() and env.state_dict()["episodes"] is None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_episode_kernels_keep_their_registers():
    """the kernels with the episode bit (cfg3's K = 5 variants): no VGPR spill, no scratch, at most 128 VGPRs (4 waves / SIMD)"""
    seen = dev_kernel_resources()
    feat = {n: kernel_variant(n)[1] for n in seen if kernel_variant(n)}
    # every kernel that simulates carries a mask: the twelve below and the four without a feature
    assert len(feat) == 16 and len(feat) == len([n for n in seen if re.search(r"tc_(step|envg|env)_kernel", n)]), sorted(seen)
    ep = [n for n in feat if feat[n] & TC_FEAT_EP]
    # tc_step_kernel<5, .., 2u | 3u>, tc_env_kernel<5, true|false, 2u | 3u>, tc_envg_kernel<2u | 3u>
    assert len(ep) == 8, sorted(seen)
    both = [n for n in ep if feat[n] == TC_FEAT_EP | TC_FEAT_CAR]
    assert len(both) == 4
    assert_one_variant_set(seen, both)
    assert_one_variant_set(seen, [n for n in ep if n not in both])
