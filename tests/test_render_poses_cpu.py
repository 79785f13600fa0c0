"""Deferred frames (tc_env_reserve_poses, tc_render_poses) without a GPU: the header and the binding, the refusals that come
before any HIP call, the split of a frame list into launches (tinycarlo_amd/csrc/tc_poses.h, built alone by the host
compiler: the very function the library launches by), and -- on the CPU reference alone -- the premise of the feature: a
frame is a function of (x, y, theta, camera), so the oracle's frame of a zeroed state with only these three set
(tests/render_poses_ref.py) is the frame the run itself drew, for every frame of the variant matrix's and the camera bank's
reference runs.  tests/test_gpu_render_poses.py then holds the library to the same frames."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import camera_bank_ref as cbr
import feature_ref as fr
import orc
import render_poses_ref as rpr
from common import ROOT

LIB = os.path.join(ROOT, "tinycarlo_amd", "libtinycarlo_hip.so")
E_INVALID = -1


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


# ------------------------------------------------------------------ 1. header and binding
def test_header_and_binding_declare_the_two_entry_points():
    from tinycarlo_amd import _native
    hdr = open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()
    assert re.search(r"^#define\s+TC_HAS_RENDER_POSES\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+TC_ABI_VERSION\s+7\s*$", hdr, re.M)
    assert re.search(r"^int\s+tc_env_reserve_poses\s*\(\s*tc_env\s*\*\s*env\s*,\s*int64_t\s+max_frames\s*\)\s*;", hdr, re.M)
    assert re.search(r"^int\s+tc_render_poses\s*\(\s*tc_env\s*\*\s*env\s*,\s*const\s+double\s*\*\s*x\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*const\s+double\s*\*\s*theta\s*,\s*const\s+int32_t\s*\*\s*camera\s*,\s*const\s+int64_t\s*\*\s*index\s*,"
                     r"\s*int64_t\s+n_src\s*,\s*int64_t\s+n_frames\s*,\s*uint8_t\s*\*\s*out\s*,\s*void\s*\*\s*stream\s*\)\s*;", hdr, re.M)
    assert _native.HAS_RENDER_POSES == 1 and _native.ABI_VERSION == 7
    assert "tc_env_reserve_poses" in _native.EXPORTS and "tc_render_poses" in _native.EXPORTS
    L = _native.lib()
    assert hasattr(L, "tc_env_reserve_poses") and hasattr(L, "tc_render_poses")
    assert L.tc_env_reserve_poses(None, 1) == E_INVALID
    assert L.tc_render_poses(None, None, None, None, None, None, 1, 1, None, None) == E_INVALID


def test_render_poses_refuses_bad_arguments_without_a_gpu():
    """every refusal that needs no handle, with host pointers that are never dereferenced and no env: the argument's own fault is
    found first and named (the pattern of test_unpack_bits_refuses_bad_arguments_without_a_gpu)"""
    from tinycarlo_amd import _native
    L = _native.lib()
    buf = np.zeros(64, dtype=np.float64)  # (64-byte aligned or not: only the offsets below matter)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    x, y, th, out, idx, cam = base, base + 8 * 8, base + 16 * 8, base + 32 * 8, base + 24 * 8, base + 28 * 8

    def call(x=x, y=y, th=th, cam=None, idx=None, n_src=4, n=4, out=out):
        rc = L.tc_render_poses(None, x, y, th, cam, idx, n_src, n, out, None)
        return rc, L.tc_last_error().decode()

    for kw, word in (({"x": None}, "required"), ({"y": None}, "required"), ({"th": None}, "required"), ({"out": None}, "required"),
                     ({"n_src": 0}, "n_src"), ({"n_src": -3}, "n_src"), ({"n": -1}, "n_frames"), ({"n": 5}, "n_frames"),
                     ({"out": out + 4}, "aligned"), ({"out": out + 8}, "aligned"), ({"x": x + 4}, "aligned"),
                     ({"idx": idx + 4, "n": 9}, "aligned"), ({"cam": cam + 2}, "aligned")):
        rc, err = call(**kw)
        assert rc == E_INVALID and err.startswith("tc_render_poses:") and word in err, (kw, rc, err)
    # with an index more frames than sources are fine: what is left to refuse is the missing env
    rc, err = call(idx=idx, n=9)
    assert rc == E_INVALID and "no env" in err, (rc, err)
    rc, err = call()
    assert rc == E_INVALID and "no env" in err, (rc, err)
    assert L.tc_env_reserve_poses(None, 0) == E_INVALID and L.tc_env_reserve_poses(None, -5) == E_INVALID


def test_vec_env_methods_exist_and_say_noise_free():
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    for name in ("reserve_poses", "render_poses", "render_rollout"):
        assert callable(getattr(TinyCarloVecEnv, name))
    assert "noise-free" in TinyCarloVecEnv.render_poses.__doc__ and "noise-free" in TinyCarloVecEnv.render_rollout.__doc__
    assert "roll[\"obs\"]" in TinyCarloVecEnv.render_rollout.__doc__


# ------------------------------------------------------------------ 2. the launch split
SPLIT_SHIM = r"""
#include "tc_poses.h"
extern "C" long long shim_group_count(long long n_frames, long long capacity) { return pose_group_count(n_frames, capacity); }
extern "C" void shim_group_at(long long n_frames, long long capacity, long long g, int nt, long long* out) {
  const PoseGroup p = pose_group_at(n_frames, capacity, g, nt);
  out[0] = p.first; out[1] = p.count; out[2] = p.pose_blocks;
}
"""


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    d = tmp_path_factory.mktemp("tc_poses")
    src, lib = d / "shim.cpp", d / "libtc_poses.so"
    src.write_text(SPLIT_SHIM)
    subprocess.check_call(["c++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"),
                           "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.shim_group_count.restype = C.c_longlong
    L.shim_group_count.argtypes = [C.c_longlong, C.c_longlong]
    L.shim_group_at.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.POINTER(C.c_longlong)]
    return L


def test_launch_split_covers_every_frame_exactly_once(split):
    """exhaustive: n_frames 0..300 x capacity 1..70 -- the groups cover every frame once, in order; none exceeds the capacity;
    no slot lies beyond the list; the pose launch has a lane for every frame of its group and no idle workgroup"""
    out = (C.c_longlong * 3)()
    for nt in (256, 64):
        for n in range(0, 301):
            for cap in range(1, 71):
                groups = split.shim_group_count(n, cap)
                assert groups == -(-n // cap), (n, cap, groups)
                nxt = 0
                for g in range(groups):
                    split.shim_group_at(n, cap, g, nt, out)
                    first, count, blocks = out[0], out[1], out[2]
                    assert first == nxt and 1 <= count <= cap and first + count <= n, (n, cap, g, first, count)
                    assert blocks * nt >= count > (blocks - 1) * nt, (n, cap, g, count, blocks)
                    nxt = first + count
                assert nxt == n, (n, cap, nxt)
    assert split.shim_group_count(5, 0) == 0 and split.shim_group_count(-1, 4) == 0
    # the GPU cases' plan: 222 frames through a scratch of 64 are four launches, the last of 30
    assert split.shim_group_count(222, 64) == 4
    split.shim_group_at(222, 64, 3, 256, out)
    assert (out[0], out[1], out[2]) == (192, 30, 1)
    # far beyond 2^31 frames: the first frame of a late group is a 64-bit number
    split.shim_group_at(10 ** 12, 8192, 10 ** 8, 256, out)
    assert (out[0], out[1], out[2]) == (8192 * 10 ** 8, 8192, 32)


# ------------------------------------------------------------------ 3. the premise, on the reference alone
PREMISE = [(5, "classes"), (516, "classes"), (516, "rgb"), (8, "classes"), (9, "classes"), (13, "classes")]


@pytest.mark.parametrize("kcode,fmt", PREMISE)
def test_a_frame_is_a_function_of_the_pose(kcode, fmt):
    """every frame of the run (reset, 4 single steps, the 6-step call: 370 with the re-spawn rows) is the helper's frame of
    the step's x, y, theta alone"""
    run = fr.reference_run(kcode, True, fmt, 0)
    r = rpr.case_renderer(kcode, True, fmt)
    n = nonempty = 0
    for s in run["steps"]:
        x, y, th = (s["state"][k] for k in ("x", "y", "theta"))
        got, nseg = r.frames(x, y, th)
        assert np.array_equal(got, s["obs"]), (kcode, fmt, "frames differ in envs", np.flatnonzero((got != s["obs"]).any(axis=1))[:8])
        assert (nseg[s["obs"].any(axis=1)] > 0).all()
        n += len(got)
        nonempty += int(s["obs"].any(axis=1).sum())
    assert n == 370 and nonempty >= 300, (kcode, fmt, n, nonempty)
    assert any(s["fresh"].any() for s in run["steps"][fr.N_SINGLE + 1:]), "no re-spawn row inside the call"


@pytest.mark.parametrize("kcode", cbr.KCODES)
def test_a_bank_frame_is_a_function_of_the_pose_and_the_camera_row(kcode):
    run = cbr.reference_run(kcode, True, "classes")
    r = rpr.case_renderer(kcode, True, "classes", cameras=run["ref"].cameras)
    for s in run["steps"]:
        got, _ = r.frames(s["state"]["x"], s["state"]["y"], s["state"]["theta"], s["camera"])
        assert np.array_equal(got, s["obs"]), (kcode, "frames differ in envs", np.flatnonzero((got != s["obs"]).any(axis=1))[:8])
    multi = np.stack([s["camera"] for s in run["steps"][cbr.NS:]])
    assert len(np.unique(multi)) >= 3, "fewer than 3 distinct cameras inside the 6-step call"
    # the next camera of the bank draws another frame for some pose of the call (GPU case 3 relies on it)
    s = run["steps"][cbr.NS]
    other, _ = r.frames(s["state"]["x"], s["state"]["y"], s["state"]["theta"], (s["camera"] + 1) % cbr.BANK_COUNT)
    assert (other != s["obs"]).any()


# ------------------------------------------------------------------ 4. the extra poses of the GPU cases
@pytest.mark.parametrize("kcode", (5, 13))
def test_extra_poses_are_what_they_are_named(kcode):
    x, y, th = rpr.extra_poses(kcode)
    assert len(x) == rpr.FAR + rpr.ON_ROAD
    frames, nseg = rpr.case_renderer(kcode, True, "classes").frames(x, y, th)
    assert (nseg[:rpr.FAR] == 0).all() and not frames[:rpr.FAR].any(), "a far-away pose draws something"
    assert (nseg[rpr.FAR:] > 0).all() and frames[rpr.FAR:].any(axis=1).all(), ("an on-road pose draws nothing", nseg[rpr.FAR:])
    assert len(np.unique(frames[rpr.FAR:], axis=0)) >= rpr.ON_ROAD // 2, "the on-road frames barely differ"


def test_some_draw_list_of_the_k5_case_outgrows_a_head_of_eight():
    """GPU case 5 with TC_SEG_LDS_CAP=3 (a head of 8 entries) needs a frame whose list is longer than that"""
    x, y, th = rpr.extra_poses(5)
    _, nseg = rpr.case_renderer(5, True, "classes").frames(x, y, th)
    assert nseg.max() > 8, nseg


# ------------------------------------------------------------------ 5. symbols
def test_the_new_kernel_stands_beside_the_variant_matrix():
    """the pose-row kernel is named without "_kernel": no symbol of the built library that names it matches the pattern by which
    tests/test_variant_matrix_cpu.py counts the tc_*_kernel families, and the source declares it under that name"""
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build)"
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    names = set()
    for flags in (["-D", "--defined-only"], ["--defined-only"]):  # (the dynamic table, and the full one where it was kept)
        out = subprocess.run([nm, *flags, LIB], capture_output=True, text=True).stdout
        names |= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert names, "nm printed no symbol"
    mine = [n for n in names if "pose_rows" in n or "PoseArgs" in n]
    assert not [n for n in mine if re.search(r"tc_\w+_kernel", n)], mine
    src = open(os.path.join(ROOT, "tinycarlo_amd", "csrc", "k_poses.h")).read()
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)
    assert kernels == ["tc_pose_rows"] and not re.match(r"tc_\w+_kernel$", kernels[0])
    assert "template" not in re.sub(r"//.*", "", src), "the pose-row kernel is no template"
