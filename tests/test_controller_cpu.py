"""CPU checks of the built-in controller (tc_env_set_controller): header, binding and library agree; the Stanley law of
tinycarlo_amd/csrc/tc_ctrl.h, built alone by the host compiler, against its restatement in Python; and the compiler's
resource figures of the kernels with the controller bit (the tc_drive_* entry points)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from common import HIPCC, ROOT, dev_kernel_resources
from tinycarlo_amd import _native as nat

CSRC = os.path.join(ROOT, "tinycarlo_amd", "csrc")
TC_FEAT_CTRL = 4

SHIM = r"""
#include <stddef.h>
#include "tc_ctrl.h"
#include "../../include/tinycarlo_hip.h"
extern "C" double stanley(double cte, double he, double k, double speed, double msa) { return tc_ctrl_stanley(cte, he, k, speed, msa); }
extern "C" double shim_atan2(double y, double x) { return tc_atan2(y, x); }
extern "C" int controller_sizeof(void) { return (int)sizeof(tc_controller); }
extern "C" int controller_offset(int i) {
  const size_t o[4] = {offsetof(tc_controller, kind), offsetof(tc_controller, k), offsetof(tc_controller, speed),
                       offsetof(tc_controller, steer_last)};
  return (int)o[i];
}
extern "C" int step_rows_sizeof(void) { return (int)sizeof(tc_step_rows); }
extern "C" int step_rows_offset(int i) {
  const size_t o[8] = {offsetof(tc_step_rows, n_rows), offsetof(tc_step_rows, steer_noise_in), offsetof(tc_step_rows, steer_out),
                       offsetof(tc_step_rows, maneuver_out), offsetof(tc_step_rows, ou_noise_out),
                       offsetof(tc_step_rows, episode_length_out), offsetof(tc_step_rows, episode_return_out),
                       offsetof(tc_step_rows, camera_out)};
  return (int)o[i];
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tc_ctrl")
    src, lib = d / "shim.cpp", d / "libtc_ctrl.so"
    src.write_text(SHIM)
    subprocess.check_call(["c++", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.stanley.restype = L.shim_atan2.restype = C.c_double
    L.stanley.argtypes = [C.c_double] * 5
    L.shim_atan2.argtypes = [C.c_double] * 2
    return L


def _header():
    return open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()


def test_header_binding_and_library_agree():
    h = _header()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (TC_\w+) (-?\d+)\s", h, re.M)}
    assert d["TC_ABI_VERSION"] == nat.ABI_VERSION == 7
    assert d["TC_HAS_CONTROLLER"] == nat.HAS_CONTROLLER == 1
    assert d["TC_CTRL_STANLEY"] == nat.CTRL_STANLEY == 1
    assert re.search(r"\bint tc_env_set_controller\(tc_env\* env, const tc_controller\* c\);", h)
    assert "tc_env_set_controller" in nat.EXPORTS
    L = nat.lib()
    assert hasattr(L, "tc_env_set_controller") and L.tc_abi_version() == 7
    assert L.tc_env_set_controller(None, None) == -1  # TC_E_INVALID: refused before any device work
    # without a controller the action stays required
    assert L.tc_step(None, None, nat.F64, None, 0, None) == -1
    assert L.tc_step_multi(None, None, nat.F64, None, 1, 0, None, None, None) == -1


def _header_members(struct):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"[\s*]", "", n) for f in body.split(";") if f.strip()
            for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", f.strip()).split(",")]


def test_struct_mirror_matches_the_header(shim):
    assert C.sizeof(nat.ControllerC) == shim.controller_sizeof() == 32
    for i, (name, _) in enumerate(nat.ControllerC._fields_):
        assert getattr(nat.ControllerC, name).offset == shim.controller_offset(i), name
    assert _header_members("tc_controller") == [n for n, _ in nat.ControllerC._fields_]
    # the structs out-of-tree callers were compiled against did not grow
    assert C.sizeof(nat.Buffers) == 23 * 8 + 8 and C.sizeof(nat.Rollout) == 15 * 8 and C.sizeof(nat.EpisodeBuffers) == 8 * 8


def test_step_rows_mirror_matches_the_header(shim):
    """tc_step_rows, the per-step feature rows of a tc_step_multi call: one n_rows and seven pointers, in / out in the names"""
    assert C.sizeof(nat.StepRows) == shim.step_rows_sizeof() == 8 + 7 * 8
    for i, (name, _) in enumerate(nat.StepRows._fields_):
        assert getattr(nat.StepRows, name).offset == shim.step_rows_offset(i), name
    names = _header_members("tc_step_rows")
    assert names == [n for n, _ in nat.StepRows._fields_]
    assert names[0] == "n_rows" and [n for n in names[1:] if n.endswith("_in")] == ["steer_noise_in"]
    assert all(n.endswith("_out") for n in names[2:])
    h = _header()
    assert re.search(r"const tc_rollout\* rollout, const tc_step_rows\* rows[^,]*, void\* stream\);", h)
    # nothing about rows is left on the handle: no setter struct has a row member, and the episode rows' setter is gone
    for struct in ("tc_controller", "tc_drive_randomization", "tc_camera_bank", "tc_episode_buffers"):
        assert not [n for n in _header_members(struct) if "rows" in n], struct
    assert "episode_rollout" not in h and not [n for n in nat.EXPORTS if "rollout" in n]


def test_stanley_law_bit_for_bit(shim):
    """tc_ctrl_stanley against the formula of the C ABI evaluated operation by operation in Python doubles (tc_atan2 from
    the same header: glibc's atan2 is up to 2 ulp away, so it cannot be the bit-exact restatement), and within 1e-12 of
    the math.atan2 version: 2 ulp of an angle below pi are 9e-16, times 180 / pi / msa <= 5.73 is 5e-15, and the roundings
    of the four outer operations on a value of magnitude <= ~20 add 4 * 2^-53 * 32 = 1.4e-14 at most."""
    rng = np.random.default_rng(20261017)
    n = 10000
    cte, he = rng.uniform(0, 0.3, n), rng.uniform(-math.pi, math.pi, n)
    k, speed, msa = rng.uniform(0.5, 8, n), rng.uniform(0.05, 1, n), rng.uniform(10, 45, n)
    worst = 0.0
    for i in range(n):
        a = (float(cte[i]), float(he[i]), float(k[i]), float(speed[i]), float(msa[i]))
        got = shim.stanley(*a)
        want = (((a[1] + shim.shim_atan2(a[2] * a[0], a[3])) * 180.0) / 3.141592653589793) / a[4]
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (a, got, want)
        libm = (((a[1] + math.atan2(a[2] * a[0], a[3])) * 180.0) / math.pi) / a[4]
        worst = max(worst, abs(got - libm))
    assert worst <= 1e-12, worst
    for kk, sp, m in ((4.0, 0.4, 30.0), (0.5, 1.0, 10.0), (8.0, 0.05, 45.0)):
        z = shim.stanley(0.0, 0.0, kk, sp, m)
        assert z == 0.0 and math.copysign(1.0, z) == 1.0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_controller_kernels_keep_their_registers():
    """the tc_drive_* kernels (cfg3's K = 5 variants): four per mask 4-7 -- the step kernel, the env kernel with and without
    the camera, the grouped kernel -- none spills VGPRs or uses scratch, none has more than 128 VGPRs (4 waves / SIMD); and
    the three existing families keep their sixteen kernels"""
    seen = dev_kernel_resources()
    drive = {}
    for n in seen:
        m = re.match(r"_Z\d+tc_drive_(step|envg|env)_kernelI(?:L\w+E)*Lj(\d+)EEv8StepArgs$", n)
        if m:
            drive[n] = (m.group(1), int(m.group(2)))
    assert len(drive) == 16 and len(drive) == len([n for n in seen if "tc_drive_" in n]), sorted(seen)
    for mask in (4, 5, 6, 7):
        names = [n for n in drive if drive[n][1] == mask]
        assert mask & TC_FEAT_CTRL and sorted(drive[n][0] for n in names) == ["env", "env", "envg", "step"], (mask, names)
        assert sorted(re.search(r"Lb([01])ELj", n).group(1) for n in names if drive[n][0] == "env") == ["0", "1"], names
        for n in names:
            vgpr, spill, scratch = seen[n]
            assert spill == 0 and scratch == 0, (n, "spills VGPRs / uses scratch", seen[n])
            assert vgpr <= 128, (n, "more than 128 VGPRs", vgpr)
    assert len([n for n in seen if re.search(r"tc_(step|envg|env)_kernel", n)]) == 16, sorted(seen)


def test_python_api_rejects_misuse_without_a_controller():
    from oracle_backend import OracleVecEnv
    from tinycarlo_amd.config import bundled_config
    env = OracleVecEnv(bundled_config("config_simple_layout.yaml"), num_envs=4)
    with pytest.raises(ValueError):
        env.alloc_rollout(2, keys=("steer",))  # needs a controller
    assert "steer" not in env.alloc_rollout(2, keys="all")  # existing users' key set is unchanged
    sd = env.state_dict()
    assert "controller" in sd and sd["controller"] is None
