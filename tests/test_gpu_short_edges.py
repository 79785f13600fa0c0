"""ThickLine at thickness 2 with only the quad's two long outline edges (tc_line.h, R_F_LONG_EDGES in raster_body) on the
GPU, bit for bit against the oracle, which keeps drawing all four.

Through tc_render_segments (the raster kernel) like tests/test_gpu_raster_fuzz.py, on segment lists made for this change:
end points at -3..+3 px around every border and corner, segments 0-3 px long, coordinates beyond 2^13 and next to
+-2^31, and draw lists of exactly 16, 17, 32 and 33 segments (one pass of the set-up loop / two in the four-edge form,
one raster batch / a second batch of one).  Thickness 2 takes the two-edge form, thickness 3 and TC_SHORT_EDGES=1 the
four-edge form; all three must give the oracle's frames.  Then the frame and step kernels: one 64-env, 6-step
tc_step_multi call and 6 single steps on simple_layout, with the switch at 0 and at 1.

Like the clip-merge test this cannot see WHICH form a kernel took -- both give the same frame by construction
(tests/test_short_edges_cpu.py has the proof); the switch row and the flag are covered by both values running.
"""
import ctypes as C

import numpy as np
import pytest

import orc
from test_gpu_parity import make_env, make_oracle
from test_gpu_raster_fuzz import make_env as make_raster_env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INT_MAX, INT_MIN = 2147483647, -2147483648
N_ENV, CAP = 64, 40
COUNTS = [16, 17, 32, 33, 0, CAP]  # the first envs' draw-list lengths; the rest are random in [25, CAP]


def near_border(rng, n):
    """a pixel coordinate at -3..+3 px from border pixel 0 or n - 1"""
    return int(rng.integers(-3, 4)) + (n - 1) * int(rng.integers(0, 2))


def short_edge_segments(rng, H, W, Cn):
    seg = np.zeros((N_ENV, CAP, 5), dtype=np.int32)
    cnt = rng.integers(25, CAP + 1, N_ENV).astype(np.int32)
    cnt[:len(COUNTS)] = COUNTS
    far = [1 << 13, (1 << 13) + 1, 1 << 14, 1 << 20, INT_MAX, INT_MAX - 1, INT_MAX - 3]
    for e in range(N_ENV):
        for k in range(cnt[e]):
            kind = rng.integers(0, 8)
            if kind <= 2:    # an end point by a border (or a corner: both axes), 0-3 px long
                x0 = near_border(rng, W) if kind != 1 else int(rng.integers(0, W))
                y0 = near_border(rng, H) if kind != 2 else int(rng.integers(0, H))
                x1, y1 = x0 + int(rng.integers(-3, 4)), y0 + int(rng.integers(-3, 4))
            elif kind == 3:  # corner to anywhere on screen
                x0, y0 = near_border(rng, W), near_border(rng, H)
                x1, y1 = int(rng.integers(0, W)), int(rng.integers(0, H))
            elif kind == 4:  # border to border
                x0, y0, x1, y1 = near_border(rng, W), int(rng.integers(-3, H + 3)), int(rng.integers(-3, W + 3)), near_border(rng, H)
            elif kind == 5:  # by a border, the other end at or beyond 2^13 px (edges clipped to the near plane)
                x0, y0 = near_border(rng, W), near_border(rng, H)
                x1 = int(rng.choice(far[:4])) * int(rng.choice([-1, 1])) + int(rng.integers(-2, 3))
                y1 = int(rng.choice(far[:4])) * int(rng.choice([-1, 1])) + int(rng.integers(-2, 3))
            elif kind == 6:  # next to +-2^31
                x0, y0 = (near_border(rng, W), near_border(rng, H)) if rng.random() < 0.7 else (int(rng.choice(far[4:])), INT_MIN + int(rng.integers(0, 4)))
                x1 = int(rng.choice(far[4:])) if rng.random() < 0.5 else INT_MIN + int(rng.integers(0, 4))
                y1 = int(rng.choice(far[4:])) if rng.random() < 0.5 else INT_MIN + int(rng.integers(0, 4))
            else:            # short, anywhere on screen
                x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
                x1, y1 = x0 + int(rng.integers(-3, 4)), y0 + int(rng.integers(-3, 4))
            if rng.random() < 0.5:
                x0, y0, x1, y1 = x1, y1, x0, y0
            seg[e, k] = (rng.integers(0, Cn), x0, y0, x1, y1)
        order = np.argsort(seg[e, :cnt[e], 0], kind="stable")  # a valid list is grouped by layer (renderer.py:41-43)
        seg[e, :cnt[e]] = seg[e, :cnt[e]][order]
    return seg, cnt


_ref = {}


def reference(env, seg, cnt, H, W, th):
    """the oracle's frames of this list: computed once per (size, thickness), shared by the switch's two values"""
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


@pytest.mark.parametrize("switch", ["0", "1"])
@pytest.mark.parametrize("th", [2, 3])
@pytest.mark.parametrize("H,W", [(24, 40), (64, 64)])
def test_render_segments_bit_exact(H, W, th, switch, monkeypatch):
    monkeypatch.setenv("TC_SHORT_EDGES", switch)
    env = make_raster_env(H, W, "classes", N_ENV, th)
    rng = np.random.default_rng(H * 1000 + W)  # the same list for every thickness and switch value
    seg, cnt = short_edge_segments(rng, H, W, env.n_classes)
    assert cnt[:4].tolist() == [16, 17, 32, 33] and 1800 <= int(cnt.sum()) <= 2200
    obs = env.render_segments(torch.from_numpy(seg), torch.from_numpy(cnt))
    torch.cuda.synchronize()
    got = obs.cpu().numpy().reshape(N_ENV, -1)
    ref = reference(env, seg, cnt, H, W, th)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, (f"{H}x{W} t={th} TC_SHORT_EDGES={switch}: frames differ for envs", bad[:8], cnt[bad[:8]].tolist(),
                           [seg[b, :cnt[b]][:3].tolist() for b in bad[:2]], int((got != ref).sum()))
    assert ref.max() == 255 and got[4].max() == 0
    env.close()


@pytest.mark.parametrize("switch", ["0", "1"])
def test_step_and_step_multi_equal_the_oracle(switch, monkeypatch):
    monkeypatch.setenv("TC_SHORT_EDGES", switch)
    orc.set_math_mode(orc.MATH_PORTABLE)
    try:
        n, K = 64, 6
        rng = np.random.default_rng(4)
        cc = np.stack([rng.uniform(0.3, 1, (K, n)), rng.uniform(-1, 1, (K, n))], axis=2).astype(np.float32)
        man = rng.integers(0, 4, (K, n)).astype(np.int32)

        env = make_env("simple_layout", "r64", "classes", n)  # one tc_step_multi call: the frame kernel
        o = make_oracle(env)
        env.reset(seed=9)
        o.reset(env._keep[0].cpu().numpy())
        roll = env.alloc_rollout(K, keys=("obs", "cte"))
        env.step_multi(torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda(), rollout=roll)
        torch.cuda.synchronize()
        seen = 0
        for k in range(K):
            o.step(cc[k].astype(np.float64), man[k])
            assert np.array_equal(roll["cte"][k].cpu().numpy().view(np.int64), o.info["cte"].view(np.int64)), ("cte of step", k)
            g = roll["obs"][k].cpu().numpy().reshape(n, -1)
            bad = np.flatnonzero((g != o.obs).any(axis=1))
            assert bad.size == 0, ("tc_step_multi", switch, "step", k, "envs", bad[:8])
            seen = max(seen, int(g.max()))
        assert seen == 255
        env.close()

        env = make_env("simple_layout", "r64", "classes", n)  # six single steps: the fused step kernel
        o = make_oracle(env)
        env.reset(seed=9)
        o.reset(env._keep[0].cpu().numpy())
        for k in range(K):
            env.step({"car_control": cc[k], "maneuver": man[k]})
            o.step(cc[k].astype(np.float64), man[k])
            torch.cuda.synchronize()
            g = env.out["obs"].cpu().numpy().reshape(n, -1)
            bad = np.flatnonzero((g != o.obs).any(axis=1))
            assert bad.size == 0, ("tc_step", switch, "step", k, "envs", bad[:8])
        env.close()
    finally:
        orc.set_math_mode(orc.MATH_LIBM)
