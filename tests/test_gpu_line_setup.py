"""The outline set-up of tc_line.h as the kernels run it -- clipLine on exact-integer doubles, the 32-bit DDA set-up,
ThickLine's quad from int32 parts -- on the GPU, bit for bit against the oracle, which keeps the int64 arithmetic of
drawing.cpp.  tests/test_line_setup_cpu.py compares the two forms of the header on the CPU; here the device's own f64
divide, reciprocal and conversions are in the loop.

Through tc_render_segments (the raster kernel): the segment lists of tests/test_gpu_short_edges.py (borders, corners,
short segments, draw lists of exactly 16, 17, 32 and 33 segments) with a third of every list replaced by
  * magnitudes: one end at or next to +-2^13 or +-2^31 on one axis or both, the other end on screen;
  * double clips: lines that cross the whole frame from outside to outside -- horizontal, vertical, through a corner,
    and steep or shallow ones that leave through two different borders;
at 24x40 and 64x64, thickness 2 (the two long edges) and 3 (all four).
Through the stepped kernels: 64 envs x 8 steps of simple_layout at 64x64 `classes`, as single tc_step calls (the fused
step kernel) and as one streamed tc_step_multi call (the frame kernel), equal to the oracle at tolerance 0.
"""
import ctypes as C

import numpy as np
import pytest

import orc
from test_gpu_parity import make_env, make_oracle
from test_gpu_raster_fuzz import make_env as make_raster_env
from test_gpu_short_edges import CAP, INT_MAX, INT_MIN, N_ENV, short_edge_segments

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def line_setup_segments(rng, H, W, Cn):
    seg, cnt = short_edge_segments(rng, H, W, Cn)
    far = [8191, 8192, 8193, -8191, -8192, -8193, INT_MAX, INT_MAX - 1, INT_MIN, INT_MIN + 1]
    for e in range(N_ENV):
        for k in range(cnt[e]):
            if rng.random() >= 1 / 3:
                continue
            kind = int(rng.integers(0, 6))
            if kind == 0:    # one axis at a large magnitude, the other end on screen
                x0, y0 = int(rng.choice(far)), int(rng.integers(-3, H + 3))
                if rng.random() < 0.5:
                    x0, y0 = int(rng.integers(-3, W + 3)), int(rng.choice(far))
                x1, y1 = int(rng.integers(0, W)), int(rng.integers(0, H))
            elif kind == 1:  # both axes
                x0, y0 = int(rng.choice(far)), int(rng.choice(far))
                x1, y1 = int(rng.integers(0, W)), int(rng.integers(0, H))
            elif kind == 2:  # horizontal / vertical through the whole frame
                L0, L1 = int(rng.choice([1, 3, 100, 5000])), int(rng.choice([1, 3, 100, 5000]))
                if rng.random() < 0.5:
                    y0 = y1 = int(rng.integers(-2, H + 2))
                    x0, x1 = -L0, W - 1 + L1
                else:
                    x0 = x1 = int(rng.integers(-2, W + 2))
                    y0, y1 = -L0, H - 1 + L1
            elif kind == 3:  # through a corner, both ends outside
                cx, cy = (W - 1) * int(rng.integers(0, 2)), (H - 1) * int(rng.integers(0, 2))
                a, b = int(rng.integers(1, 8)) * int(rng.choice([-1, 1])), int(rng.integers(1, 8)) * int(rng.choice([-1, 1]))
                k0, k1 = int(rng.choice([1, 2, 50, 3000])), int(rng.choice([1, 2, 50, 3000]))
                x0, y0, x1, y1 = cx - k0 * a, cy - k0 * b, cx + k1 * a, cy + k1 * b
            elif kind == 4:  # top to bottom, both ends clipped on y (and often on x)
                x0, y0 = int(rng.integers(-W, 2 * W)), -int(rng.integers(1, 4 * H))
                x1, y1 = int(rng.integers(-W, 2 * W)), H + int(rng.integers(0, 4 * H))
            else:            # left to right
                x0, y0 = -int(rng.integers(1, 4 * W)), int(rng.integers(-H, 2 * H))
                x1, y1 = W + int(rng.integers(0, 4 * W)), int(rng.integers(-H, 2 * H))
            if rng.random() < 0.5:
                x0, y0, x1, y1 = x1, y1, x0, y0
            seg[e, k, 1:] = (x0, y0, x1, y1)  # (the layer stays: the list remains grouped by layer)
    return seg, cnt


_ref = {}


def reference(env, seg, cnt, H, W, th):
    """the oracle's frames of this list, computed once per (size, thickness)"""
    key = (H, W, th)
    if key not in _ref:
        omap, ocam = orc.OracleMap(env.map), orc.make_cam(env.camera, orc.FMT_CLASSES)
        ref = np.zeros((N_ENV, env.n_classes * H * W), dtype=np.uint8)
        for e in range(N_ENV):
            s = np.ascontiguousarray(seg[e, :cnt[e]])
            orc.lib().orc_render(omap.h, C.byref(ocam), orc._ip(s) if len(s) else None, int(cnt[e]), orc._bp(ref[e]))
        ref.setflags(write=False)
        _ref[key] = ref
    return _ref[key]


@pytest.mark.parametrize("th", [2, 3])
@pytest.mark.parametrize("H,W", [(24, 40), (64, 64)])
def test_render_segments_bit_exact(H, W, th):
    env = make_raster_env(H, W, "classes", N_ENV, th)
    rng = np.random.default_rng(H * 1000 + W + 7)  # the same list for both thicknesses
    seg, cnt = line_setup_segments(rng, H, W, env.n_classes)
    assert cnt[:6].tolist() == [16, 17, 32, 33, 0, CAP]
    obs = env.render_segments(torch.from_numpy(seg), torch.from_numpy(cnt))
    torch.cuda.synchronize()
    got = obs.cpu().numpy().reshape(N_ENV, -1)
    ref = reference(env, seg, cnt, H, W, th)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, (f"{H}x{W} t={th}: frames differ for envs", bad[:8], cnt[bad[:8]].tolist(),
                           [seg[b, :cnt[b]][:3].tolist() for b in bad[:2]], int((got != ref).sum()))
    assert ref.max() == 255 and got[4].max() == 0
    env.close()


def test_step_and_streamed_step_multi_equal_the_oracle():
    orc.set_math_mode(orc.MATH_PORTABLE)
    try:
        n, K = 64, 8
        rng = np.random.default_rng(13)
        cc = np.stack([rng.uniform(0.3, 1, (K, n)), rng.uniform(-1, 1, (K, n))], axis=2).astype(np.float32)
        man = rng.integers(0, 4, (K, n)).astype(np.int32)

        env = make_env("simple_layout", "r64", "classes", n)  # one streamed tc_step_multi call: the frame kernel
        o = make_oracle(env)
        env.reset(seed=21)
        o.reset(env._keep[0].cpu().numpy())
        roll = env.alloc_rollout(K, keys=("obs", "cte"))
        env.step_multi(torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda(), rollout=roll)
        torch.cuda.synchronize()
        info = env.launch_info(K)  # (after the call: the first streamed call allocates what the form needs)
        assert info["steps_per_dispatch"] == K and info["kernel"].endswith("tc_frame_kernel"), ("not streamed", info)
        seen = 0
        for k in range(K):
            o.step(cc[k].astype(np.float64), man[k])
            assert np.array_equal(roll["cte"][k].cpu().numpy().view(np.int64), o.info["cte"].view(np.int64)), ("cte of step", k)
            g = roll["obs"][k].cpu().numpy().reshape(n, -1)
            bad = np.flatnonzero((g != o.obs).any(axis=1))
            assert bad.size == 0, ("tc_step_multi", "step", k, "envs", bad[:8])
            seen = max(seen, int(g.max()))
        assert seen == 255
        env.close()

        env = make_env("simple_layout", "r64", "classes", n)  # eight single steps: the fused step kernel
        o = make_oracle(env)
        env.reset(seed=21)
        o.reset(env._keep[0].cpu().numpy())
        for k in range(K):
            env.step({"car_control": cc[k], "maneuver": man[k]})
            o.step(cc[k].astype(np.float64), man[k])
            torch.cuda.synchronize()
            g = env.out["obs"].cpu().numpy().reshape(n, -1)
            bad = np.flatnonzero((g != o.obs).any(axis=1))
            assert bad.size == 0, ("tc_step", "step", k, "envs", bad[:8])
        env.close()
    finally:
        orc.set_math_mode(orc.MATH_LIBM)
