"""CPU checks of the drive randomisation (tc_env_set_drive_randomization): header, binding and library agree; the arithmetic
of tinycarlo_amd/csrc/tc_rng.h / tc_trig.h -- tc_log, tc_normal_at, tc_ou_step, tc_maneuver_index -- built alone by the host
compiler, against its restatement in Python; and the compiler's figures of the kernels that carry it."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from common import HIPCC, ROOT, dev_kernel_resources, kernel_variant
from tinycarlo_amd import _native as nat
from tinycarlo_amd import randomization as R

CSRC = os.path.join(ROOT, "tinycarlo_amd", "csrc")
FIELDS = ("seed", "env_offset", "n_maneuvers", "maneuvers", "maneuver_mode", "ou_reset", "theta", "mu", "sigma", "maneuver",
          "episode", "ou_state", "ou_draws")

SHIM = r"""
#include <stddef.h>
#include "tc_rng.h"
#include "../../include/tinycarlo_hip.h"
extern "C" double shim_log(double x) { return tc_log(x); }
extern "C" double shim_cos(double x) { return tc_cos(x); }
extern "C" double shim_ou(double n, double eps, double theta, double mu, double sigma) { return tc_ou_step(n, eps, theta, mu, sigma); }
extern "C" unsigned long long shim_sm(unsigned long long seed, unsigned long long n) { return tc_splitmix64_at(seed, n); }
extern "C" unsigned int shim_man(unsigned long long seed, unsigned int env, unsigned int ep, unsigned int count) {
  return tc_maneuver_index(seed, env, ep, count);
}
extern "C" void shim_log_n(int n, const double* x, double* out) { for (int i = 0; i < n; i++) out[i] = tc_log(x[i]); }
// draws of one env (stride_env = 0, stride_draw = 1) or draw 0 of many envs (1, 0)
extern "C" void shim_normals(unsigned long long seed, unsigned int env0, unsigned int draw0, unsigned int stride_env,
                             unsigned int stride_draw, int n, double* out) {
  for (int i = 0; i < n; i++) out[i] = tc_normal_at(seed, env0 + stride_env * (unsigned int)i, draw0 + stride_draw * (unsigned int)i);
}
extern "C" int drive_sizeof(void) { return (int)sizeof(tc_drive_randomization); }
extern "C" int drive_offset(int i) {
  const size_t o[13] = {offsetof(tc_drive_randomization, seed), offsetof(tc_drive_randomization, env_offset),
                        offsetof(tc_drive_randomization, n_maneuvers), offsetof(tc_drive_randomization, maneuvers),
                        offsetof(tc_drive_randomization, maneuver_mode), offsetof(tc_drive_randomization, ou_reset),
                        offsetof(tc_drive_randomization, theta), offsetof(tc_drive_randomization, mu),
                        offsetof(tc_drive_randomization, sigma), offsetof(tc_drive_randomization, maneuver),
                        offsetof(tc_drive_randomization, episode), offsetof(tc_drive_randomization, ou_state),
                        offsetof(tc_drive_randomization, ou_draws)};
  return (int)o[i];
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tc_drive")
    src, lib = d / "shim.cpp", d / "libtc_drive.so"
    src.write_text(SHIM)
    subprocess.check_call(["c++", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    dp = C.POINTER(C.c_double)
    L.shim_log.restype = L.shim_cos.restype = L.shim_ou.restype = C.c_double
    L.shim_log.argtypes = L.shim_cos.argtypes = [C.c_double]
    L.shim_ou.argtypes = [C.c_double] * 5
    L.shim_sm.restype = C.c_uint64
    L.shim_sm.argtypes = [C.c_uint64, C.c_uint64]
    L.shim_man.restype = C.c_uint32
    L.shim_man.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    L.shim_log_n.argtypes = [C.c_int, dp, dp]
    L.shim_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, dp]
    L.shim_log_n.restype = L.shim_normals.restype = None
    return L


def normals(shim, seed, env0, draw0, stride_env, stride_draw, n):
    out = np.empty(n, dtype=np.float64)
    shim.shim_normals(seed, env0, draw0, stride_env, stride_draw, n, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def _header():
    return open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()


def test_header_binding_and_library_agree():
    h = _header()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (TC_\w+) (-?\d+)\s", h, re.M)}
    assert d["TC_ABI_VERSION"] == nat.ABI_VERSION == 7
    assert d["TC_HAS_DRIVE_RANDOMIZATION"] == nat.HAS_DRIVE_RANDOMIZATION == 1
    assert (d["TC_MAN_DRAW"], d["TC_MAN_CYCLE"]) == (nat.MAN_DRAW, nat.MAN_CYCLE) == (0, 1)
    assert re.search(r"\bint tc_env_set_drive_randomization\(tc_env\* env, const tc_drive_randomization\* d\);", h)
    assert re.search(r"\bint tc_draw_normals\(uint64_t seed, uint32_t env, uint32_t first_draw, int32_t n, double\* out\);", h)
    assert "tc_env_set_drive_randomization" in nat.EXPORTS and "tc_draw_normals" in nat.EXPORTS
    L = nat.lib()
    assert hasattr(L, "tc_env_set_drive_randomization") and hasattr(L, "tc_draw_normals") and L.tc_abi_version() == 7
    assert L.tc_env_set_drive_randomization(None, None) == -1


def test_struct_mirror_matches_the_header(shim):
    assert C.sizeof(nat.DriveRandomizationC) == shim.drive_sizeof() == 112
    assert tuple(n for n, _ in nat.DriveRandomizationC._fields_) == FIELDS
    for i, name in enumerate(FIELDS):
        assert getattr(nat.DriveRandomizationC, name).offset == shim.drive_offset(i), name
    body = re.search(r"typedef struct \{([^}]*)\} tc_drive_randomization;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\s*]|\[\d+\]", "", n) for f in body.split(";") if f.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", f.strip()).split(",")]
    assert tuple(names) == FIELDS
    # the structs out-of-tree callers were compiled against did not grow
    assert C.sizeof(nat.ControllerC) == 32
    assert C.sizeof(nat.Buffers) == 23 * 8 + 8 and C.sizeof(nat.Rollout) == 15 * 8 and C.sizeof(nat.EpisodeBuffers) == 8 * 8


def test_bad_settings_are_refused_before_any_device_work():
    """every refusal of the header with NULL / host pointers: nothing here may be dereferenced or reach the device"""
    L = nat.lib()
    host = (C.c_int32 * 4)()
    hostd = (C.c_double * 4)()
    ip, dpp = C.addressof(host), C.addressof(hostd)

    def drv(**kw):
        c = nat.DriveRandomizationC()
        c.n_maneuvers, c.maneuver_mode = 2, nat.MAN_DRAW
        c.maneuvers[0], c.maneuvers[1] = 0, 3
        c.theta, c.mu, c.sigma = 0.1, 0.0, 0.4
        c.maneuver, c.episode, c.ou_state, c.ou_draws = ip, ip, dpp, ip
        for k, v in kw.items():
            if k == "maneuvers":
                for i, m in enumerate(v):
                    c.maneuvers[i] = m
            else:
                setattr(c, k, v)
        return c
    bad = [(drv(maneuvers=(0, 4)), b"0..3"), (drv(maneuvers=(-1, 0)), b"0..3"), (drv(n_maneuvers=9), b"0..8"),
           (drv(n_maneuvers=-1), b"0..8"), (drv(maneuver_mode=2), b"maneuver_mode"), (drv(maneuver_mode=-1), b"maneuver_mode"),
           (drv(theta=float("nan")), b"finite"), (drv(mu=float("inf")), b"finite"), (drv(sigma=float("-inf")), b"finite"),
           (drv(maneuver=None), b"maneuver and episode"), (drv(episode=None), b"maneuver and episode"),
           (drv(ou_draws=None), b"ou_draws")]
    for c, why in bad:  # (refused for the struct's own sake, whatever the handle is: the message names the field)
        assert L.tc_env_set_drive_randomization(None, C.byref(c)) == -1
        assert why in L.tc_last_error(), (why, L.tc_last_error())
    # a good struct passes all of that and is refused for the handle: no controller can be installed on no env
    assert L.tc_env_set_drive_randomization(None, C.byref(drv())) == -1
    assert b"no env" in L.tc_last_error()
    assert L.tc_env_set_drive_randomization(None, C.byref(drv(n_maneuvers=0, maneuver=None, episode=None, ou_state=None,
                                                              ou_draws=None))) == -1
    assert b"no env" in L.tc_last_error()
    # the maneuver argument stays required where no device maneuvers can be installed
    assert L.tc_step(None, None, nat.F64, None, 0, None) == -1
    assert L.tc_step_multi(None, None, nat.F64, None, 1, 0, None, None, None) == -1
    # the maneuver / OU rows are the call's (tc_step_rows): a bad struct is refused whatever the handle is, the message says why
    for rows, why in ((nat.StepRows(n_rows=-1), b"negative"), (nat.StepRows(n_rows=0, maneuver_out=ip), b"n_rows = 0"),
                      (nat.StepRows(n_rows=0, ou_noise_out=dpp), b"n_rows = 0")):
        assert L.tc_step_multi(None, None, nat.F64, None, 1, 0, None, C.byref(rows), None) == -1
        assert why in L.tc_last_error(), (why, L.tc_last_error())
    assert L.tc_draw_normals(0, 0, 0, -1, None) == -1 and L.tc_draw_normals(0, 0, 0, 1, None) == -1
    assert L.tc_draw_normals(0, 0, 0, 0, None) == 0


def ulp_diff(a, b):
    """distance in units of the last place of two arrays of finite doubles of the same sign"""
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


def test_log_against_libm(shim):
    """tc_log over (0, 1]: 10^5 log-uniform points down to 2^-53, every power of two 2^-53 .. 2^0.  Bound: 2 ulp -- tc_log
    (the classic reduction + degree-14 polynomial, error < 1 ulp) and glibc's log (< 1 ulp) each stay within 1 ulp of the true
    value, so they are at most 2 ulp apart."""
    rng = np.random.default_rng(20261020)
    x = np.exp2(-53.0 * rng.random(100000))
    x = np.concatenate([x, np.exp2(-np.arange(0, 54, dtype=np.float64))])
    assert x.min() >= 2.0 ** -53 and x.max() == 1.0
    got = np.empty_like(x)
    dp = C.POINTER(C.c_double)
    shim.shim_log_n(len(x), np.ascontiguousarray(x).ctypes.data_as(dp), got.ctypes.data_as(dp))
    want = np.array([math.log(v) for v in x])
    assert np.isfinite(got).all() and (got <= 0).all()
    worst = int(ulp_diff(got[x < 1.0], want[x < 1.0]).max())
    print("tc_log vs math.log: worst", worst, "ulp")
    assert worst <= 2, worst
    z = shim.shim_log(1.0)
    assert z == 0.0 and math.copysign(1.0, z) == 1.0


def normal_py(shim, seed, env, draw):
    """tc_normal_at operation by operation in Python doubles / integers"""
    z = shim.shim_sm(shim.shim_sm(seed, 0x6F75), ((env << 32) | draw) & 0xFFFFFFFFFFFFFFFF)
    a, b = shim.shim_sm(z, 0), shim.shim_sm(z, 1)
    u1 = float((a >> 11) + 1) * 2.0 ** -53
    u2 = float(b >> 11) * 2.0 ** -53
    assert 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
    return math.sqrt(-2.0 * shim.shim_log(u1)) * shim.shim_cos(6.283185307179586 * u2)


def test_splitmix_shim_equals_the_numpy_restatement(shim):
    rng = np.random.default_rng(3)
    for s, n in rng.integers(0, 2 ** 63, (200, 2)):
        assert shim.shim_sm(int(s), int(n)) == int(R.splitmix64_at(np.uint64(s), np.uint64(n)))


def test_normal_bit_for_bit(shim):
    rng = np.random.default_rng(7)
    cases = [(0, 0, 0), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0x7FFFFFFF), (2, 36, 23)]
    cases += [(int(s), int(e), int(d)) for s, e, d in zip(rng.integers(0, 2 ** 63, 3000), rng.integers(0, 2 ** 32, 3000),
                                                           rng.integers(0, 2 ** 31, 3000))]
    for seed, env, draw in cases:
        got = float(normals(shim, seed, env, draw, 0, 0, 1)[0])
        want = normal_py(shim, seed, env, draw)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (seed, env, draw, got, want)


@pytest.mark.parametrize("which", ["one env", "draw 0 of many envs"])
def test_normal_distribution(shim, which):
    """10^6 numbers: |mean| <= 5e-3 (5 standard errors), |var - 1| <= 7.1e-3 (5 * sqrt(2 / n)), |eps| <= sqrt(106 ln 2)"""
    n = 1000000
    x = normals(shim, 2026, 5, 0, 0, 1, n) if which == "one env" else normals(shim, 2026, 0, 0, 1, 0, n)
    assert np.isfinite(x).all()
    mean, var, top = float(x.mean()), float(x.var()), float(np.abs(x).max())
    print(which, "mean", mean, "var", var, "max |eps|", top)
    assert abs(mean) <= 5e-3, mean
    assert abs(var - 1.0) <= 7.1e-3, var
    assert top <= 8.58, top
    assert len(np.unique(x[:10000])) == 10000


def test_first_pairs_are_all_different(shim):
    """the first 10^4 (env, draw) pairs -- 100 envs x 100 draws -- give 10^4 different numbers"""
    x = np.concatenate([normals(shim, 2026, e, 0, 0, 1, 100) for e in range(100)])
    assert len(np.unique(x)) == 10000


def test_library_export_equals_the_shim(shim):
    for seed, env, first in ((0, 0, 0), (2, 36, 1000), (0xDEADBEEFCAFEF00D, 0xFFFFFFFF, 0x7FFFFF00)):
        got = R.draw_normal(seed, env, first, n=300)
        head = min(300, 2 ** 31 - first)  # (the draw counter wraps at 2^31, as ou_draws does)
        want = np.concatenate([normals(shim, seed, env, first, 0, 1, head), normals(shim, seed, env, 0, 0, 1, 300 - head)])
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (seed, env, first)
        assert R.draw_normal(seed, env, first) == want[0]


def test_ou_step_order(shim):
    rng = np.random.default_rng(11)
    for n, eps, th, mu, sg in rng.normal(0, 1, (2000, 5)):
        want = n + (th * (mu - n) + sg * eps)
        assert shim.shim_ou(n, eps, th, mu, sg) == want == float(R.ou_step(n, eps, th, mu, sg))


def test_draw_maneuver(shim):
    rng = np.random.default_rng(13)
    for seed, env, ep, cnt in zip(rng.integers(0, 2 ** 63, 2000), rng.integers(0, 2 ** 32, 2000), rng.integers(0, 2 ** 31, 2000),
                                  rng.integers(1, 9, 2000)):
        cand = list(range(int(cnt)))  # identity candidates: the maneuver IS the index (values 0..7 only here, on the host)
        assert int(R.draw_maneuver(int(seed), int(env), int(ep), cand)) == shim.shim_man(int(seed), int(env), int(ep), int(cnt))
    # cycle mode: train_stanley_il.py's maneuver = (maneuver + 1) % 3 with 2 sent as 3, for env 0
    assert R.draw_maneuver(0, 0, np.arange(7), (0, 1, 3), "cycle").tolist() == [0, 1, 3, 0, 1, 3, 0]
    assert R.draw_maneuver(0, 1, np.arange(4), (0, 1, 3), "cycle").tolist() == [1, 3, 0, 1]
    # what the GPU cases rely on: 37 envs x 3 episodes with candidates (0, 1, 3) reach every candidate in draw mode, and
    # more than half of the envs see two different maneuvers
    m = R.draw_maneuver(2, np.arange(37)[:, None], np.arange(3)[None, :], (0, 1, 3))
    assert m.shape == (37, 3) and set(m.reshape(-1).tolist()) == {0, 1, 3}
    assert sum(len(set(r.tolist())) > 1 for r in m) > 37 // 2
    with pytest.raises(ValueError):
        R.draw_maneuver(0, 0, 0, (0, 1), "shuffle")
    with pytest.raises(ValueError):
        R.draw_maneuver(0, 0, 0, ())


# what DESIGN.md records for the parent commit: (vgpr_count, vgpr_spill_count, scratch bytes) of the sixteen kernels without
# the controller bit in the dev build -- family, mask, camera stage compiled in (tc_env_kernel only)
PARENT_NON_CTRL = {
    ("step", 0, None): 126, ("step", 1, None): 126, ("step", 2, None): 128, ("step", 3, None): 128,
    ("env", 0, "1"): 128, ("env", 1, "1"): 128, ("env", 2, "1"): 128, ("env", 3, "1"): 128,
    ("env", 0, "0"): 128, ("env", 1, "0"): 128, ("env", 2, "0"): 128, ("env", 3, "0"): 128,
    ("envg", 0, None): 125, ("envg", 1, None): 127, ("envg", 2, None): 123, ("envg", 3, None): 125,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_symbols_and_resources():
    """still sixteen tc_drive_* kernels and no further tc_*_kernel family; the feature is a run-time branch of the drive
    kernels, so the sixteen kernels without the controller bit keep the VGPR figures DESIGN.md records for the parent"""
    seen = dev_kernel_resources()
    drive = [n for n in seen if "tc_drive_" in n]
    assert len(drive) == 16, sorted(drive)
    assert all(re.match(r"_Z\d+tc_drive_(step|envg|env)_kernelI", n) for n in drive), sorted(drive)
    for n in drive:
        vgpr, spill, scratch = seen[n]
        assert spill == 0 and scratch == 0 and vgpr <= 128, (n, seen[n])
    got = {}
    for n in seen:
        kv = kernel_variant(n)
        if kv:
            cam = re.search(r"Lb([01])ELj", n).group(1) if kv[0] == "env" else None
            got[(kv[0], kv[1], cam)] = seen[n]
    assert set(got) == set(PARENT_NON_CTRL), sorted(got)
    for key, vgpr in PARENT_NON_CTRL.items():
        assert got[key] == (vgpr, 0, 0), (key, got[key], vgpr)


def test_python_api_rejects_misuse_without_the_feature():
    from oracle_backend import OracleVecEnv
    from tinycarlo_amd.config import bundled_config
    env = OracleVecEnv(bundled_config("config_simple_layout.yaml"), num_envs=4)
    with pytest.raises(ValueError):
        env.randomize_drive(maneuvers=(0, 1, 3))  # needs a controller
    with pytest.raises(ValueError):
        env.set_ou(sigma=0.1)
    for key in ("maneuver", "steer_noise"):
        with pytest.raises(ValueError):
            env.alloc_rollout(2, keys=(key,))
    roll = env.alloc_rollout(2, keys="all")
    assert "maneuver" not in roll and "steer_noise" not in roll  # existing users' key set is unchanged
    assert env.episode_maneuver is None and env.drive_episode is None and env.ou_state is None and env.ou_draws is None
    sd = env.state_dict()
    assert "drive_randomization" in sd and sd["drive_randomization"] is None
    env.randomize_drive()  # off while off: nothing to do
