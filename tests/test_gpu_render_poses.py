"""Deferred frames on the device (tc_render_poses; TinyCarloVecEnv.render_poses / render_rollout) against the call that
produced the poses and against the CPU reference of tests/render_poses_ref.py, byte for byte.

The settings are the kernel-variant matrix's (tests/feature_ref.py): 37 envs, 64x64 frames, the generated maps,
cte_termination(MAX_CTE, 1), host spawns, a reset, 4 single steps and one 6-step call with obs, x, y and theta rows.  With a
scratch of 64 frames the call's 222 frames are four launches, the last of 30 (tests/test_render_poses_cpu.py holds the split,
and the premise that a frame is a function of its pose, without a GPU).

Run on the MI355X box with `pytest -m gpu`."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import camera_bank_ref as cbr
import feature_ref as fr
import orc
import render_poses_ref as rpr
import test_gpu_variant_matrix as vm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, NS, NM = fr.N_ENVS, fr.N_SINGLE, fr.N_MULTI
F = NM * N  # 222 frames
PAD = 0xA5


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


class PoseCell(vm.Cell):
    """the matrix's cell, optionally with the camera bank of tests/camera_bank_ref.py (no ledger: these cases add no kernel variant)"""

    def __init__(self, kcode, thick, fmt, fuse=True, bank=False):
        super().__init__(kcode, thick, fmt, 0, fuse=fuse)
        self.label = f"render_poses kcode {kcode} thick {thick} {fmt}" + (" bank" if bank else "") + ("" if fuse else " TC_FUSE=0")
        self.bank = bank
        if bank:
            self.run = cbr.reference_run(kcode, thick, "rgb" if fmt == "rgb" else "classes")
            self.env.randomize_cameras(seed=cbr.CAM_SEED, **cbr.BANK)

    def note(self, n_steps, mode):
        return self.env.launch_info(n_steps)

    def rollout_call(self, first=NS, steps=NM, keys=("obs", "x", "y", "theta")):
        env = self.env
        roll = env.alloc_rollout(steps, keys=keys + (("camera",) if self.bank else ()))
        roll["obs"].fill_(0xFF)
        env.step_multi(self.cc[first:first + steps].contiguous(), self.man[first:first + steps].contiguous(), rollout=roll)
        return roll

    def whole_run(self):
        self.reset()
        self.single_steps()
        return self.rollout_call()

    def want_rows(self, first=NS, steps=NM):
        return np.stack([self.frames_of(s) for s in self.run["steps"][first:first + steps]])  # [steps, N, bytes]


@functools.lru_cache(maxsize=None)
def helper_frames(kcode, thick, fmt):
    """the helper's frames of the reference run's poses of the 6-step call, [222, bytes], computed once per cell"""
    run = fr.reference_run(kcode, thick, "rgb" if fmt == "rgb" else "classes", 0)
    frames, nseg = rpr.case_renderer(kcode, thick, fmt).frames(*rpr.run_poses(run))
    return frames, nseg


def snapshot(env):
    torch.cuda.synchronize()
    return {**{"state." + k: v.clone() for k, v in env.state.items()}, **{"out." + k: v.clone() for k, v in env.out.items()}}


def assert_untouched(env, snap, label):
    torch.cuda.synchronize()
    now = snapshot(env)
    for k, v in snap.items():
        assert torch.equal(vm.torch.as_tensor(vm.bits(now[k])), vm.torch.as_tensor(vm.bits(v))), (label, "the render changed", k)


def render_all_and_compare(c):
    """case 1's comparison: reserve 64 frames, draw the call's 222 frames into a buffer two frames longer"""
    env = c.env
    roll = c.whole_run()
    snap = snapshot(env)
    env.reserve_poses(64)
    buf = torch.full((F + 2,) + tuple(env._obs_shape), PAD, dtype=torch.uint8, device=env.device)
    got = env.render_rollout(roll, out=buf[:F].view((NM, N) + tuple(env._obs_shape)))
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (NM, N) + tuple(env._obs_shape)
    g = got.cpu().numpy().reshape(NM, N, -1)
    r = roll["obs"].cpu().numpy().reshape(NM, N, -1)
    assert np.array_equal(r, c.want_rows()), (c.label, "the call's own frames are not the reference's")
    bad = np.argwhere((g != r).any(axis=2))
    assert len(bad) == 0, (c.label, "deferred frames differ from the call's own at (row, env)", bad[:8].tolist())
    if not c.bank:
        h, _ = helper_frames(c.kcode, c.thick, c.fmt)
        assert np.array_equal(g.reshape(F, -1), h), (c.label, "deferred frames differ from the helper's")
    assert bool((buf[F:] == PAD).all()), (c.label, "a frame beyond n_frames was written")
    assert g.any(), c.label
    assert_untouched(env, snap, c.label)
    return roll, g


# ------------------------------------------------------------------ 1. against the call itself and the oracle
CASE1 = [(kc, t, f) for kc in (5, 516, 8, 9) for t in (True, False) for f in ("classes", "rgb", "bits")]


@pytest.mark.parametrize("kcode,thick,fmt", CASE1)
def test_rollout_frames_equal_the_call_and_the_helper(kcode, thick, fmt):
    c = PoseCell(kcode, thick, fmt)
    try:
        assert c.env.launch_info(NM)["kernel"].endswith("tc_frame_kernel")
        render_all_and_compare(c)
    finally:
        c.close()


# ------------------------------------------------------------------ 2. index
def case_index():
    rng = np.random.default_rng(20)
    idx = np.concatenate([rng.integers(0, F, 60), np.arange(150, 130, -1), [7, 7, 7, 0, F - 1], [-1, F, 2 ** 40, -2 ** 40, F + 5],
                          rng.integers(0, F, 10)]).astype(np.int64)
    assert len(idx) == 100
    return idx


@pytest.mark.parametrize("fmt", ("classes", "bits"))
def test_index_gathers_repeats_and_clamps(fmt):
    c = PoseCell(5, True, fmt)
    try:
        roll = c.whole_run()
        idx = case_index()
        c.env.reserve_poses(64)  # two launches: 64 + 36
        got = c.env.render_rollout(roll, index=torch.from_numpy(idx).cuda())
        torch.cuda.synchronize()
        h, _ = helper_frames(5, True, fmt)
        assert tuple(got.shape) == (100,) + tuple(c.env._obs_shape)
        assert np.array_equal(got.cpu().numpy().reshape(100, -1), h[np.clip(idx, 0, F - 1)])
        # a 2-d index over the flattened rows, and an empty one
        got2 = c.env.render_poses(roll["x"], roll["y"], roll["theta"], index=torch.from_numpy(idx[:10].reshape(2, 5)).cuda())
        assert np.array_equal(got2.cpu().numpy().reshape(10, -1), h[np.clip(idx[:10], 0, F - 1)])
        none = c.env.render_poses(roll["x"], roll["y"], roll["theta"], index=torch.zeros(0, dtype=torch.int64, device="cuda"))
        assert tuple(none.shape) == (0,) + tuple(c.env._obs_shape)
    finally:
        c.close()


# ------------------------------------------------------------------ 3. cameras, bank
@pytest.mark.parametrize("kcode", cbr.KCODES)
def test_bank_frames_take_the_camera_row(kcode):
    c = PoseCell(kcode, True, "classes", bank=True)
    try:
        roll, g = render_all_and_compare(c)  # (frames from roll["camera"] equal roll["obs"])
        cam = roll["camera"].cpu().numpy()
        assert np.array_equal(cam, np.stack([s["camera"] for s in c.run["steps"][NS:]])) and len(np.unique(cam)) >= 3
        nxt = ((cam + 1) % cbr.BANK_COUNT).astype(np.int32)
        got = c.env.render_poses(roll["x"], roll["y"], roll["theta"], camera=torch.from_numpy(nxt).cuda())
        torch.cuda.synchronize()
        x, y, th = (roll[k].cpu().numpy() for k in ("x", "y", "theta"))
        want, _ = rpr.case_renderer(kcode, True, "classes", cameras=c.run["ref"].cameras).frames(x, y, th, nxt)
        got = got.cpu().numpy().reshape(F, -1)
        assert np.array_equal(got, want), (c.label, "frames of the next camera differ in", np.flatnonzero((got != want).any(axis=1))[:8])
        assert (got != g.reshape(F, -1)).any(), "the next camera draws every frame alike"
        # camera values outside the bank are clamped into it
        wild = nxt.copy().reshape(-1)
        wild[:4] = [-1, cbr.BANK_COUNT, 2 ** 31 - 1, -2 ** 31]
        got = c.env.render_poses(roll["x"], roll["y"], roll["theta"], camera=torch.from_numpy(wild.reshape(NM, N)).cuda())
        want4, _ = rpr.case_renderer(kcode, True, "classes", cameras=c.run["ref"].cameras).frames(
            x.reshape(-1)[:4], y.reshape(-1)[:4], th.reshape(-1)[:4], np.clip(wild[:4].astype(np.int64), 0, cbr.BANK_COUNT - 1))
        assert np.array_equal(got.cpu().numpy().reshape(F, -1)[:4], want4)
        with pytest.raises(ValueError, match="camera"):
            c.env.render_poses(roll["x"], roll["y"], roll["theta"])
        with pytest.raises(ValueError, match="camera"):
            c.env.render_rollout({k: roll[k] for k in ("x", "y", "theta")})
    finally:
        c.close()


# ------------------------------------------------------------------ 4. cameras, per-env and shared
@pytest.mark.parametrize("kcode", (5, 13))
def test_per_env_cameras_row_k_n_takes_env_n(kcode):
    from tinycarlo_amd.camera import Camera
    c = PoseCell(kcode, True, "classes")
    try:
        env = c.env
        pitch = np.array([10.0, 14.0, 19.0])[np.arange(N) % 3]
        fov = np.array([90.0, 110.0, 129.0])[(np.arange(N) // 3) % 3]
        ori = np.tile(np.asarray(env.camera.orientation, dtype=np.float64), (N, 1))
        ori[:, 0] = pitch
        x, y, th = (torch.from_numpy(a).cuda() for a in rpr.run_poses(c.run))
        with pytest.raises(ValueError, match="shared camera"):
            env.render_poses(x, y, th, camera=torch.zeros(F, dtype=torch.int32, device="cuda"))
        env.reserve_poses(64)
        from tinycarlo_amd import _native as nat
        cam0 = torch.zeros(F, dtype=torch.int32, device="cuda")
        out = torch.zeros((F,) + tuple(env._obs_shape), dtype=torch.uint8, device="cuda")
        rc = nat.lib().tc_render_poses(env._h, x.data_ptr(), y.data_ptr(), th.data_ptr(), cam0.data_ptr(), None, F, F, out.data_ptr(), None)
        assert rc == -1 and b"shared camera" in nat.lib().tc_last_error()
        env.reset(seed=fr.case_seed(kcode))  # (a bound, reset handle: the K = 13 path reads the env's other buffers)
        env.set_env_cameras(orientation=ori, fov=fov)
        rc = nat.lib().tc_render_poses(env._h, x.data_ptr(), y.data_ptr(), th.data_ptr(), None, None, F, F, out.data_ptr(), None)
        assert rc == -1 and b"per-env cameras" in nat.lib().tc_last_error()
        got = env.render_rollout({"x": x, "y": y, "theta": th})
        torch.cuda.synchronize()
        cfg = copy.deepcopy(c.env.config["camera"])
        cams = []
        for n in range(N):
            cfg.update(orientation=list(ori[n]), fov=float(fov[n]), position=list(env.camera.position))
            cams.append(Camera(copy.deepcopy(cfg)))
        want, _ = rpr.case_renderer(kcode, True, "classes", cameras=cams).frames(*rpr.run_poses(c.run), np.tile(np.arange(N), NM))
        got = got.cpu().numpy().reshape(F, -1)
        assert np.array_equal(got, want), (c.label, "per-env frames differ in", np.flatnonzero((got != want).any(axis=1))[:8])
        h, _ = helper_frames(kcode, True, "classes")
        assert (want != h).any(), "the per-env cameras draw what the shared camera draws"
    finally:
        c.close()


# ------------------------------------------------------------------ 5. poses no simulator produced
SWITCH5 = {"default": {}, "no_cull": {"TC_FRAME_CULL": "0"}, "head_of_8": {"TC_SEG_LDS_CAP": "3"}}


@pytest.mark.parametrize("switch", SWITCH5)
@pytest.mark.parametrize("fmt", ("classes", "bits"))
def test_poses_no_simulator_produced(switch, fmt, monkeypatch):
    """far outside the map: all zeros, through the cull's verdict in the row (default) and through rows without one
    (TC_FRAME_CULL=0); on a lane line with several headings; draw lists longer than the LDS head (TC_SEG_LDS_CAP=3)"""
    for k, v in SWITCH5[switch].items():
        monkeypatch.setenv(k, v)
    c = PoseCell(5, True, fmt)
    try:
        x, y, th = rpr.extra_poses(5)
        want, nseg = rpr.case_renderer(5, True, fmt).frames(x, y, th)
        if switch == "head_of_8":
            assert c.env.frame_lds_info()["head_entries"] == 8 and nseg.max() > 8
        # (an env that was never reset or stepped: the render needs no state)
        got = c.env.render_poses(*(torch.from_numpy(a).cuda() for a in (x, y, th)))
        torch.cuda.synchronize()
        got = got.cpu().numpy().reshape(len(x), -1)
        assert not got[:rpr.FAR].any(), "a far-away pose drew something"
        assert np.array_equal(got, want), (switch, fmt, "frames differ in poses", np.flatnonzero((got != want).any(axis=1))[:8])
        assert got[rpr.FAR:].any(axis=1).all()
    finally:
        c.close()


# ------------------------------------------------------------------ 6. handles without a frame kernel
CASE6 = [(13, True, "classes", True), (13, False, "rgb", True), (13, True, "bits", True), (5, True, "classes", False), (5, False, "bits", False)]


@pytest.mark.parametrize("kcode,thick,fmt,fuse", CASE6)
def test_handles_without_a_frame_kernel(kcode, thick, fmt, fuse, monkeypatch):
    """K = 13, and K = 5 under TC_FUSE=0: the camera stage of tc_env_kernel in render mode over the gathered poses, rounds of
    N = 37 frames -- case 1's comparison with 222 frames"""
    if not fuse:
        monkeypatch.setenv("TC_FUSE", "0")
    c = PoseCell(kcode, thick, fmt, fuse=fuse)
    try:
        assert not c.env.launch_info(NM)["kernel"].endswith("tc_frame_kernel")
        roll, _ = render_all_and_compare(c)
        stats = c.env.draw_list_stats()  # (still the call's frames: the render drew into a scratch of its own)
        idx = case_index()
        got = c.env.render_rollout(roll, index=torch.from_numpy(idx).cuda())
        want = roll["obs"].cpu().numpy().reshape(F, -1)[np.clip(idx, 0, F - 1)]
        assert np.array_equal(got.cpu().numpy().reshape(100, -1), want)
        assert c.env.draw_list_stats() == stats
    finally:
        c.close()


# ------------------------------------------------------------------ 7. not in the way
@pytest.mark.parametrize("kcode", (5, 13))
def test_a_render_between_two_calls_changes_neither(kcode):
    c = PoseCell(kcode, True, "classes")
    try:
        c.reset()
        c.single_steps()
        keys = ("obs", "x", "y", "theta", "reward", "cte", "terminated", "truncated")
        a = c.rollout_call(NS, 3, keys)
        got = c.env.render_rollout(a)
        b = c.rollout_call(NS + 3, 3, keys)
        torch.cuda.synchronize()
        assert torch.equal(got, a["obs"])
        for first, roll in ((NS, a), (NS + 3, b)):
            assert np.array_equal(roll["obs"].cpu().numpy().reshape(3, N, -1), c.want_rows(first, 3)), (c.label, first)
            for j, s in enumerate(c.run["steps"][first:first + 3]):
                for k in ("x", "y", "theta"):
                    assert np.array_equal(vm.bits(roll[k][j]), vm.bits(s["state"][k])), (c.label, first, j, k)
                for k in ("reward", "cte"):
                    assert np.array_equal(vm.bits(roll[k][j]), vm.bits(s["info"][k])), (c.label, first, j, k)
        c.check(c.run["steps"][-1], "after the second call", obs=False)
    finally:
        c.close()


def test_deferred_frames_are_noise_free():
    c = PoseCell(5, True, "classes")
    try:
        c.reset()
        c.single_steps()
        c.env.set_noise(3, max_radius=12, seed=5)
        roll = c.rollout_call()
        got = c.env.render_rollout(roll)
        torch.cuda.synchronize()
        h, _ = helper_frames(5, True, "classes")
        assert np.array_equal(got.cpu().numpy().reshape(F, -1), h)
        assert (roll["obs"].cpu().numpy().reshape(F, -1) != h).any(), "the call's own frames carry no noise"
    finally:
        c.close()


# ------------------------------------------------------------------ 8. capture
def test_render_poses_captured_into_a_graph():
    from tinycarlo_amd import _native as nat
    c = PoseCell(5, True, "bits")
    try:
        env = c.env
        x0, y0, th0 = rpr.run_poses(c.run)
        x, y, th = (torch.from_numpy(a).cuda() for a in (x0, y0, th0))
        buf = torch.full((F,) + tuple(env._obs_shape), PAD, dtype=torch.uint8, device="cuda")
        # without a reservation the C entry refuses, and says what to call
        rc = nat.lib().tc_render_poses(env._h, x.data_ptr(), y.data_ptr(), th.data_ptr(), None, None, F, F, buf.data_ptr(), None)
        assert rc == -1 and b"tc_env_reserve_poses" in nat.lib().tc_last_error()
        assert nat.lib().tc_render_poses(env._h, x.data_ptr(), y.data_ptr(), th.data_ptr(), None, None, F, 0, buf.data_ptr(), None) == 0
        env.reserve_poses(64)
        env.render_poses(x, y, th, out=buf)  # warm-up: loads the kernels
        torch.cuda.synchronize()
        h, _ = helper_frames(5, True, "bits")
        assert np.array_equal(buf.cpu().numpy().reshape(F, -1), h)
        buf.fill_(PAD)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            env.render_poses(x, y, th, out=buf)
        torch.cuda.synchronize()
        perm = np.random.default_rng(8).permutation(F)
        for a, src in ((x, x0), (y, y0), (th, th0)):
            a.copy_(torch.from_numpy(src.reshape(-1)[perm].reshape(src.shape)))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy().reshape(F, -1), h[perm]), "the replay did not draw the new poses"
    finally:
        c.close()


# ------------------------------------------------------------------ the Python layer's own refusals
def test_python_refusals_come_before_the_library():
    c = PoseCell(5, True, "classes")
    try:
        env = c.env
        x = torch.zeros(6, N, dtype=torch.float64, device="cuda")
        for bad in (dict(x=x.float()), dict(y=x[:3]), dict(theta=x.cpu()), dict(index=torch.zeros(3, dtype=torch.int32, device="cuda")),
                    dict(out=torch.zeros((F,) + tuple(env._obs_shape), dtype=torch.float32, device="cuda")),
                    dict(out=torch.zeros((F + 1,) + tuple(env._obs_shape), dtype=torch.uint8, device="cuda"))):
            kw = dict(x=x, y=x, theta=x)
            kw.update(bad)
            with pytest.raises(ValueError):
                env.render_poses(**kw)
        with pytest.raises(ValueError, match="theta"):
            env.render_rollout({"x": x, "y": x})
        with pytest.raises(ValueError):
            env.reserve_poses(0)
    finally:
        c.close()
