"""The cull verdict in the pose row (entry 13; tc_cull.h, cam_cull_row, frame_pose) and the one-group form of the five-wave
frame kernel, on the GPU: 64 envs, 8-step calls with every frame in a rollout, observations and draw-list lengths against
the oracle (portable math) at tolerance 0.

simple_layout 64x64 is the map whose frames carry verdicts (the only bundled map with a cull table).  Cars start on the road
looking along it and no frame is culled for the first hundred steps, so every case runs behind a pre-roll of PREROLL steps
with bench.py's action distribution (v ~ U(0.3, 1), s ~ U(-1, 1), a maneuver held for 64 steps, auto-reset from a spawn queue),
done by the env itself in 128-step calls without observations and by the oracle beside it; the state behind it is compared
bit for bit.  That both verdicts then occur in the call under test is asserted three ways: from the reference predicate
(tests/cull_shim.py) on the oracle's poses, from the oracle's draw-list lengths, and from the lengths the kernels stored
(seg_n through draw_list_stats: the share of empty frames is the oracle's, and strictly between 0 and 1).

The cases: streamed and TC_STREAM=0 (the row polled lane by lane / read through the scalar cache), TC_FRAME_CULL=0 (no verdict
written or read), TC_STREAM_TEST_SKIP (the recover pass reads the verdict), packed class masks, knuffingen at 128x128
(tc_frame_kernel<5, .., 16>) and the same map with TC_CAM_GROUP=0 (a K = 9 handle) -- knuffingen has no cull table (the
planner's condition H3), so these two run the kernels that read rows with rows that carry no verdict --, a camera bank and
per-env cameras (no verdict either: the cull is off), a prepared call, a call captured into a graph and replayed twice, and
calls of different form on one handle (streamed with every frame / last frame only, whose frame launch reads finished rows /
a single fused step, which evaluates the predicate itself / streamed again).

A K = 5 / batches-of-32 handle with several camera groups cannot be built through the API: a map gets several groups only
when it is too large for K = 8, and then draws with K = 9 or, in component groups, K = 5 with batches of 16.  The path that
sends such a handle to tc_frame_banded is therefore not run here; tests/test_gpu_frame_scalars.py runs tc_frame_banded for
frames of several bands."""
import copy

import numpy as np
import pytest

import cull_shim
import orc
from test_gpu_parity import make_env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K, SEED = 64, 8, 3
PREROLL = 512   # tests/test_cull_row_cpu.py: 24 % of the frames of steps 512..544 are culled (none before step 100)
CALL = 128      # steps per pre-roll call
QUEUE = 64


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cull_shim.build_shim(tmp_path_factory.mktemp("tc_cull_row_gpu"))


def host_actions(steps, seed):
    rng = np.random.default_rng(seed)
    cc = np.stack([rng.uniform(0.3, 1, (steps, N)), rng.uniform(-1, 1, (steps, N))], axis=2).astype(np.float32)
    man = np.repeat(rng.integers(0, 4, ((steps + 63) // 64, N)), 64, axis=0)[:steps].astype(np.int32)
    return np.ascontiguousarray(cc), np.ascontiguousarray(man)


_refs = {}


def reference(key, env, preroll, tail, camera=None):
    """The oracle's run for an env just reset with SEED: `preroll` steps without frames, `tail` steps with.  Computed once
    per key, shared between the cases and left unchanged."""
    nodes, queue = env._keep[0].cpu().numpy(), env._aux["spawn_queue"].cpu().numpy()
    if key in _refs:
        r = _refs[key]
        assert np.array_equal(r["nodes"], nodes) and np.array_equal(r["queue"], queue) and r["tail"] >= tail, key
        return r
    cc, man = host_actions(preroll + tail, seed=SEED + 1)
    fmt = orc.FMT_CLASSES if env.observation_space_format == "classes" else orc.FMT_RGB
    o = orc.Oracle(env.map, env.car_params, env.camera if camera is None else camera, fmt, N, threads=8)
    o.reset(nodes)
    o.spawn_queue = queue.copy()
    for t in range(preroll):
        o.step(cc[t].astype(np.float64), man[t], flags=orc.F_AUTORESET | orc.F_NO_OBSERVATION, with_obs=False)
    state0 = {k: o.state[k].copy() for k in ("x", "y", "theta", "velocity", "steering")}
    obs, nseg, poses = [], [], []
    for t in range(preroll, preroll + tail):
        o.step(cc[t].astype(np.float64), man[t], flags=orc.F_AUTORESET, with_obs=True)
        obs.append(o.obs.copy())
        nseg.append([len(o.segments(i)[0]) for i in range(N)])
        poses.append(np.stack([o.state["x"], o.state["y"], o.state["theta"]], axis=1).copy())
    assert int(o.spawn_cursor.max()) < QUEUE, "the spawn queue wrapped"
    r = {"nodes": nodes, "queue": queue, "cc": cc, "man": man, "state0": state0, "obs": np.stack(obs), "nseg": np.array(nseg),
         "poses": np.stack(poses), "preroll": preroll, "tail": tail}
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _refs[key] = r
    return r


def start(env, key, preroll=PREROLL, tail=2 * K, camera=None):
    """reset, reference, the env's own pre-roll -> (reference, actions on the device)"""
    env.reset(seed=SEED)
    ref = reference(key, env, preroll, tail, camera)
    cc, man = torch.from_numpy(ref["cc"].copy()).cuda(), torch.from_numpy(ref["man"].copy()).cuda()
    if preroll:
        roll = env.alloc_rollout(CALL, keys=("cte",))
        assert preroll % CALL == 0
        for c in range(preroll // CALL):
            env.step_multi(cc[c * CALL:(c + 1) * CALL], man[c * CALL:(c + 1) * CALL], rollout=roll)
        torch.cuda.synchronize()
    for k, v in ref["state0"].items():
        assert np.array_equal(env.state[k].cpu().numpy().view(np.int64), v.view(np.int64)), ("state behind the pre-roll", k)
    return ref, cc, man


def want_frames(env, ref, t0, steps):
    obs = ref["obs"][t0:t0 + steps].reshape(steps, N, -1)
    if env.obs_packing == "bits":  # the packed frame is the packing of the class masks (tinycarlo_amd/packing.py)
        from tinycarlo_amd.packing import pack_bits_reference
        H, W = env.camera.resolution
        obs = pack_bits_reference(ref["obs"][t0:t0 + steps].reshape(steps, N, env.n_classes, H, W)).reshape(steps, N, -1)
    return obs


def check_frames(env, ref, roll, t0, what):
    nseg = ref["nseg"][t0:t0 + K]
    got = roll["obs"].cpu().numpy().reshape(K, N, -1)
    bad = np.argwhere((got != want_frames(env, ref, t0, K)).any(axis=2))
    assert bad.size == 0, (what, "frames differ at (step, env)", bad[:8].tolist(), nseg[tuple(bad[:8].T)].tolist())
    assert got.any(), what
    # draw-list lengths: what the kernels stored in seg_n (a streamed call: all K rows; a chunked one: the rows its ring holds)
    st = env.draw_list_stats()
    rows = st["frames"] // N
    assert st["frames"] == rows * N and K // 2 <= rows <= K, (what, st)
    nseg = nseg[K - rows:]
    assert st["max_segments"] == int(nseg.max()), (what, st, int(nseg.max()))
    assert st["empty_frame_frac"] == float((nseg == 0).sum()) / nseg.size, (what, st)
    assert st["mean_segments_per_frame"] == float(nseg.sum()) / nseg.size, (what, st)
    return st


def call(env, ref, cc, man, t0, what, roll=None):
    """one K-step call on steps t0 .. t0 + K - 1 behind the pre-roll with every frame in a rollout, equal to the reference"""
    p = ref["preroll"]
    roll = env.alloc_rollout(K, keys=("obs", "cte")) if roll is None else roll
    env.step_multi(cc[p + t0:p + t0 + K], man[p + t0:p + t0 + K], rollout=roll)
    torch.cuda.synchronize()
    assert env.launch_info(K)["kernel"].endswith("tc_frame_kernel"), (what, env.launch_info(K))
    return check_frames(env, ref, roll, t0, what)


def both_verdicts(shim, env, ref, t0, st):
    """the call's frames hold culled and drawn ones: by the reference predicate on the oracle's poses, by the oracle's draw
    lists, and by the lengths the kernels stored"""
    cull = cull_shim.Cull(shim, env.map, env.camera)
    assert cull.on
    p = ref["poses"][t0:t0 + K].reshape(-1, 3)
    culled = cull.empty(p[:, 0], p[:, 1], p[:, 2])
    assert 0.1 <= culled.mean() <= 0.9, culled.mean()
    nseg = ref["nseg"][t0:t0 + K].reshape(-1)
    assert not (culled & (nseg > 0)).any()
    assert 0.0 < st["empty_frame_frac"] < 1.0 and st["empty_frame_frac"] >= culled.reshape(K, N)[K - st["frames"] // N:].mean(), st


def simple_env(**kw):
    return make_env("simple_layout", "r64", "classes", N, autoreset=True, spawn_queue_len=QUEUE, **kw)


# ---------------------------------------------------------------------------------------------- the verdict in the row
@pytest.mark.parametrize("stream", ["1", "0"])
def test_streamed_and_chunked(monkeypatch, shim, stream):
    monkeypatch.setenv("TC_STREAM", stream)
    env = simple_env()
    ref, cc, man = start(env, "simple")
    for t0 in (0, K):  # (the second call finds the rows the first one's frame kernel reset)
        st = call(env, ref, cc, man, t0, f"TC_STREAM={stream} call at {t0}")
        both_verdicts(shim, env, ref, t0, st)
    env.close()


def test_cull_switched_off(monkeypatch, shim):
    monkeypatch.setenv("TC_FRAME_CULL", "0")
    env = simple_env()
    ref, cc, man = start(env, "simple")
    st = call(env, ref, cc, man, 0, "TC_FRAME_CULL=0")
    both_verdicts(shim, env, ref, 0, st)  # (the frames are the same ones: only nobody skips the culled ones)
    env.close()


def test_recover_pass_reads_the_verdict(monkeypatch, shim):
    monkeypatch.setenv("TC_STREAM_TEST_SKIP", "3")
    env = simple_env()
    ref, cc, man = start(env, "simple")
    st = call(env, ref, cc, man, 0, "TC_STREAM_TEST_SKIP=3")
    both_verdicts(shim, env, ref, 0, st)
    # the frames with (row + env) % 3 == 0 were left to tc_frame_recover_kernel: culled and drawn ones among them
    left = (np.arange(K)[:, None] + np.arange(N)[None, :]) % 3 == 0
    cull = cull_shim.Cull(shim, env.map, env.camera)
    p = ref["poses"][:K].reshape(-1, 3)
    culled = cull.empty(p[:, 0], p[:, 1], p[:, 2]).reshape(K, N)
    assert culled[left].any() and not culled[left].all()
    st = call(env, ref, cc, man, K, "TC_STREAM_TEST_SKIP=3, second call")
    env.close()


def test_packed_class_masks(shim):
    env = simple_env(obs_packing="bits")
    ref, cc, man = start(env, "simple")
    st = call(env, ref, cc, man, 0, "packed")
    both_verdicts(shim, env, ref, 0, st)
    env.close()


# ---------------------------------------------------------------------------------------------- kernels of the other K
@pytest.mark.parametrize("cam_group,kframe", [(None, "5/16"), ("0", "9")])
def test_knuffingen_128(monkeypatch, shim, cam_group, kframe):
    if cam_group is not None:
        monkeypatch.setenv("TC_CAM_GROUP", cam_group)
    env = make_env("knuffingen", "r128", "classes", N, autoreset=True, spawn_queue_len=QUEUE)
    assert env.launch_info(K)["kvar"] == 9, env.launch_info(K)
    assert not cull_shim.Cull(shim, env.map, env.camera).on  # (no table: the rows carry no verdict)
    ref, cc, man = start(env, "knuffingen", preroll=CALL, tail=K)
    call(env, ref, cc, man, 0, f"knuffingen r128, frame kernel K = {kframe}")
    env.close()


# ---------------------------------------------------------------------------------------------- no verdict in the row
def test_camera_bank():
    """tests/test_gpu_frame_scalars.py's bank case (three cameras, a time limit of 3 steps: the index in entry 12 changes
    between the rows of a call) with entry 13 neither written nor polled"""
    import test_gpu_frame_scalars as fsc
    fsc.run_bank("camera bank, no verdict in the row")


def test_per_env_cameras(shim):
    """per-env camera rows (here the same non-default camera in every row): the cull is off, entry 13 is not written -- on a
    handle whose calls before carried verdicts"""
    from tinycarlo_amd.camera import Camera
    env = simple_env()
    c2 = copy.deepcopy(env.config["camera"])
    c2.update(fov=104)
    env.reset(seed=SEED)
    shared = reference("simple", env, PREROLL, 2 * K)
    ref, cc, man = start(env, "simple_fov104", camera=Camera(c2))
    roll = env.alloc_rollout(K, keys=("obs", "cte"))
    p = ref["preroll"]
    # first a call with the shared camera (verdicts in the rows; the two references differ in the camera alone)
    env.step_multi(cc[p:p + K], man[p:p + K], rollout=roll)
    torch.cuda.synchronize()
    check_frames(env, shared, roll, 0, "shared camera before the per-env rows")
    env.set_env_cameras(fov=[104] * N)
    st = call(env, ref, cc, man, K, "per-env cameras", roll=roll)
    assert 0.0 < st["empty_frame_frac"] < 1.0
    env.close()


# ---------------------------------------------------------------------------------------------- call forms
def test_prepared_call(shim):
    env = simple_env()
    ref, cc, man = start(env, "simple")
    p = ref["preroll"]
    cc_t, man_t = cc[p:p + K].clone(), man[p:p + K].clone()
    roll = env.alloc_rollout(K, keys=("obs", "cte"))
    pc = env.prepare_step_multi(cc_t, man_t, roll)
    for t0 in (0, K):
        cc_t.copy_(cc[p + t0:p + t0 + K])
        man_t.copy_(man[p + t0:p + t0 + K])
        pc()
        torch.cuda.synchronize()
        st = check_frames(env, ref, roll, t0, f"prepared call at {t0}")
        both_verdicts(shim, env, ref, t0, st)
    env.close()


def test_graph_captured_call(shim):
    env = simple_env()
    ref, cc, man = start(env, "simple")
    p = ref["preroll"]
    cc_t, man_t = cc[p:p + K].clone(), man[p:p + K].clone()
    roll = env.alloc_rollout(K, keys=("obs", "cte"))
    env.reserve_steps(K)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_multi(cc_t, man_t, rollout=roll)
    for t0 in (0, K):
        cc_t.copy_(cc[p + t0:p + t0 + K])
        man_t.copy_(man[p + t0:p + t0 + K])
        g.replay()
        torch.cuda.synchronize()
        st = check_frames(env, ref, roll, t0, f"graph replay at {t0}")
        both_verdicts(shim, env, ref, t0, st)
    env.close()


def test_calls_of_different_form_on_one_handle(shim):
    env = simple_env()
    tail = 3 * K + 1
    ref, cc, man = start(env, "simple_long", tail=tail)
    p = ref["preroll"]
    H, W = env.camera.resolution
    st = call(env, ref, cc, man, 0, "streamed, every frame")
    both_verdicts(shim, env, ref, 0, st)
    # only the last frame is wanted: the frame launch runs behind the simulate launch and reads finished rows
    roll = env.alloc_rollout(K, keys=("cte",))
    env.step_multi(cc[p + K:p + 2 * K], man[p + K:p + 2 * K], rollout=roll)
    torch.cuda.synchronize()
    t = 2 * K - 1
    got = env.out["obs"].cpu().numpy().reshape(N, -1)
    bad = np.flatnonzero((got != ref["obs"][t].reshape(N, -1)).any(axis=1))
    assert bad.size == 0, ("last frame only", bad[:8], ref["nseg"][t][bad[:8]])
    assert (ref["nseg"][t] == 0).any() and (ref["nseg"][t] > 0).any()
    # a single step: the fused kernel poses and draws in one wavefront and evaluates the predicate itself
    t = 2 * K
    env.step_device(cc[p + t], man[p + t])
    torch.cuda.synchronize()
    got = env.out["obs"].cpu().numpy().reshape(N, -1)
    bad = np.flatnonzero((got != ref["obs"][t].reshape(N, -1)).any(axis=1))
    assert bad.size == 0, ("single step", bad[:8], ref["nseg"][t][bad[:8]])
    st = call(env, ref, cc, man, 2 * K + 1, "streamed again")
    both_verdicts(shim, env, ref, 2 * K + 1, st)
    env.close()
