"""The built-in Stanley controller (set_controller / drive / drive_step), bit-exact against the existing single-step path.

The reference is never the code under test: a fresh env with the same seeds and settings runs K calls of `step_device`,
and before each the HOST computes that step's action -- `out["cte"]` / `out["heading_error"]` copied to the host, the
command through tinycarlo_amd/csrc/tc_ctrl.h built by the host compiler, with the env's own max_steering_angle from
`env_car_params`, the noise row added, the result uploaded as float64.  Run on the MI355X box with `pytest -m gpu`."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, load_cfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K = 37, 24  # 37: no multiple of the 8 envs per wavefront / 32 per workgroup of the grouped kernel; 24: several chunks
GAIN, SPEED, LIMIT, SEED = 4.0, 0.4, 7, 2
STATE_F = ("x", "y", "theta", "velocity", "steering", "radius", "front_x", "front_y")
OUT_KEYS = ("cte", "heading_error", "reward", "terminated", "truncated", "status", "laneline_distances", "nearest_edge")
EP_KEYS = ("length", "ret", "count", "last_length", "last_return", "length_sum", "return_sum")

SHIM = r"""
#include "tc_ctrl.h"
extern "C" void stanley_n(int n, const double* cte, const double* he, double k, double speed, const double* msa, double* out) {
  for (int i = 0; i < n; i++) out[i] = tc_ctrl_stanley(cte[i], he[i], k, speed, msa[i]);
}
"""


@pytest.fixture(scope="module")
def stanley(tmp_path_factory):
    d = tmp_path_factory.mktemp("tc_ctrl_gpu")
    src, lib = d / "shim.cpp", d / "libtc_ctrl.so"
    src.write_text(SHIM)
    subprocess.check_call(["c++", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"), "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    dp = C.POINTER(C.c_double)
    L.stanley_n.argtypes = [C.c_int, dp, dp, C.c_double, C.c_double, dp, dp]
    L.stanley_n.restype = None

    def f(cte, he, k, speed, msa):
        cte, he, msa = (np.ascontiguousarray(a, dtype=np.float64) for a in (cte, he, msa))
        out = np.empty_like(cte)
        L.stanley_n(len(cte), cte.ctypes.data_as(dp), he.ctypes.data_as(dp), k, speed, msa.ctypes.data_as(dp), out.ctypes.data_as(dp))
        return out
    return f


def cfg_for():
    cfg, path = load_cfg("simple_layout")
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = [64, 64]
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


def make_env(randomize=True, limit=LIMIT, wrappers=True):
    """the settings of examples/stanley_batched.py --randomize --max-episode-steps: device spawns, per-episode cars, the
    three fused wrappers, a time limit with staggered starts"""
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    from tinycarlo_amd.wrapper import CrashTerminationWrapper, CTESparseRewardWrapper, CTETerminationWrapper
    vec = TinyCarloVecEnv(cfg_for(), num_envs=N, device="cuda:0", autoreset=True, spawn="device")
    if randomize:
        p = vec.car_params
        vec.randomize_cars({"max_steering_angle": (0.4 * p.max_steering_angle, 1.2 * p.max_steering_angle),
                            "steering_shift": (-0.01, 0.0)}, seed=SEED)
    env = vec
    if wrappers:
        env = CrashTerminationWrapper(CTETerminationWrapper(CTESparseRewardWrapper(vec, 0.01), 0.07, number_of_steps=5))
    if limit:
        vec.set_time_limit(limit)
    env.reset(seed=SEED)
    if limit:
        vec.episode_stats["length"].copy_((torch.arange(N, device="cuda:0") * limit // N).to(torch.int32))
    return vec


def inputs(steps, seed=11):
    rng = np.random.default_rng(seed)
    man = rng.integers(0, 4, (steps, N)).astype(np.int32)
    g = torch.Generator().manual_seed(seed)
    noise = (0.4 * torch.randn((steps, N), generator=g, dtype=torch.float64)).numpy()
    return man, noise


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def reference_loop(vec, stanley, man, noise, gains):
    """`len(man)` single steps of `vec`; gains[k] = (k, speed) of step k.  Returns the per-step rows (rollout key -> [K, N, ..]),
    the commands before noise (0.0 on the rows of envs the step re-spawned), the actions applied and the re-spawn mask."""
    rows = {k: [] for k in OUT_KEYS + ("obs", "x", "y", "theta", "velocity", "local_path", "lp_len", "episode_length", "episode_return")}
    steer, applied, fresh = [], [], []
    for k in range(len(man)):
        cte, he = vec.out["cte"].cpu().numpy(), vec.out["heading_error"].cpu().numpy()
        msa = (vec.env_car_params[:, 3].cpu().numpy() if vec.env_car_params is not None
               else np.full(N, vec.car_params.max_steering_angle))
        nr = vec._aux["needs_reset"].cpu().numpy().astype(bool)
        cmd = stanley(cte, he, gains[k][0], gains[k][1], msa)
        act = cmd + noise[k] if noise is not None else cmd
        cc = np.stack([np.full(N, gains[k][1]), act], axis=1)
        vec.step_device(torch.from_numpy(cc).cuda(), torch.from_numpy(man[k]).cuda())
        torch.cuda.synchronize()
        steer.append(np.where(nr, 0.0, cmd))
        applied.append(act)
        fresh.append(nr)
        for key in OUT_KEYS + ("obs",):
            rows[key].append(vec.out[key].cpu().numpy().copy())
        for key in ("x", "y", "theta", "velocity", "local_path", "lp_len"):
            rows[key].append(vec.state[key].cpu().numpy().copy())
        if vec.episode_stats is not None:
            rows["episode_length"].append(vec.episode_stats["length"].cpu().numpy().copy())
            rows["episode_return"].append(vec.episode_stats["ret"].cpu().numpy().copy())
    rows = {k: np.stack(v) for k, v in rows.items() if v}
    return rows, np.stack(steer), np.stack(applied), np.stack(fresh)


def final_of(vec):
    torch.cuda.synchronize()
    d = {("state", k): v.cpu().numpy().copy() for k, v in vec.state.items()}
    d.update({("out", k): vec.out[k].cpu().numpy().copy() for k in OUT_KEYS})
    d.update({("aux", k): v.cpu().numpy().copy() for k, v in vec._aux.items() if k != "spawn_queue"})
    d[("terms",)] = vec.term_counters.cpu().numpy().copy()
    if vec.episode_stats is not None:
        d.update({("ep", k): vec.episode_stats[k].cpu().numpy().copy() for k in EP_KEYS})
    if vec.env_car_params is not None:
        d[("car",)] = vec.env_car_params.cpu().numpy().copy()
        d[("car_episode",)] = vec.car_episode.cpu().numpy().copy()
    return d


@pytest.fixture(scope="module")
def ref(stanley):
    """the reference loop of the main setting, run once and shared (read only)"""
    man, noise = inputs(K)
    vec = make_env()
    rows, steer, applied, fresh = reference_loop(vec, stanley, man, noise, [(GAIN, SPEED)] * K)
    fin = final_of(vec)
    obs_last = vec.out["obs"].cpu().numpy().copy()
    vec.close()
    # the run covers what it is meant to cover (else every comparison below could pass vacuously)
    assert fresh[1:-1].any(), "no re-spawn row strictly inside the call"
    assert (np.abs(applied[~fresh]) > 1).any(), "no applied command beyond the steering clip"
    assert (np.abs(steer) > 1e-3).any(), "the controller never steered"
    assert (rows["status"] & 32).any() and fresh.sum() > N, "time limit / re-spawns did not act"
    return {"man": man, "noise": noise, "rows": rows, "steer": steer, "applied": applied, "fresh": fresh, "final": fin,
            "obs_last": obs_last}


def assert_rows(roll, ref, label, upto=None, skip=()):
    torch.cuda.synchronize()
    for k, t in roll.items():
        if k in skip:
            continue
        want = ref["steer"] if k == "steer" else ref["rows"][k]
        got = t.cpu().numpy()
        if upto is not None:
            want, got = want[:upto], got[:upto]
        assert got.shape == want.reshape(got.shape).shape
        assert np.array_equal(bits(got), bits(want.reshape(got.shape))), (label, k)


def assert_final(vec, ref, label):
    got = final_of(vec)
    assert set(got) == set(ref["final"]), label
    for k, v in ref["final"].items():
        assert np.array_equal(bits(got[k]), bits(v)), (label, k)


def drive_env(**kw):
    vec = make_env(**kw)
    vec.set_controller(k=GAIN, speed=SPEED)
    return vec


def run_drive(vec, ref, label, kernel):
    assert vec.launch_info(K)["kernel"] == kernel, vec.launch_info(K)
    roll = vec.alloc_rollout(K, keys="all")
    assert "steer" in roll and "episode_length" in roll and "obs" in roll
    vec.drive(torch.from_numpy(ref["man"]).cuda(), rollout=roll, steer_noise=torch.from_numpy(ref["noise"]).cuda())
    assert_rows(roll, ref, label)
    assert_final(vec, ref, label)
    assert np.array_equal(bits(vec.steer_last), bits(ref["steer"][-1])), (label, "steer_last")
    assert int(roll["obs"].max()) == 255
    return roll


def test_streamed_drive_equals_the_host_loop(ref):
    vec = drive_env()
    run_drive(vec, ref, "streamed", "tc_drive_envg_kernel+tc_frame_kernel")
    assert vec.launch_info(K)["steps_per_dispatch"] == K
    vec.close()


def test_chunked_drive_equals_the_host_loop(ref, monkeypatch):
    monkeypatch.setenv("TC_STREAM", "0")
    vec = drive_env()
    run_drive(vec, ref, "chunked", "tc_drive_envg_kernel+tc_frame_kernel")
    # several chunks (a quarter of the call each); the first goes through tc_drive_env_kernel, the rest through the grouped kernel
    assert 2 <= vec.launch_info(K)["steps_per_dispatch"] < K
    vec.close()


def test_fused_multi_step_drive_equals_the_host_loop(ref, monkeypatch):
    """TC_MULTI_SPLIT=0: the K steps in one launch of the fused step kernel"""
    monkeypatch.setenv("TC_MULTI_SPLIT", "0")
    vec = drive_env()
    run_drive(vec, ref, "fused K-step", "tc_drive_step_kernel")
    vec.close()


@pytest.mark.parametrize("var,kernel", [("TC_ENV_GROUPED", "tc_drive_env_kernel+tc_frame_kernel"),
                                        ("TC_FUSE", "tc_drive_env_kernel+tc_raster_kernel")])
def test_per_env_simulate_kernel_forms_equal_the_host_loop(ref, monkeypatch, var, kernel):
    """TC_ENV_GROUPED=0: every chunk through tc_drive_env_kernel<.., false, ..>, frames by the frame kernel; TC_FUSE=0: the
    camera stage inside tc_drive_env_kernel<.., true, ..> and a raster launch behind it"""
    monkeypatch.setenv(var, "0")
    vec = drive_env()
    run_drive(vec, ref, var + "=0", kernel)
    vec.close()


def test_single_steps_after_a_drive_call_take_none_of_its_rows(ref):
    """drive with noise and label rows, then step_device / step while the controller is on: the step ignores its car_control,
    takes no noise, leaves the earlier call's label rows alone and equals drive_step on a twin"""
    a, b = drive_env(), drive_env()
    man = torch.from_numpy(ref["man"]).cuda()
    rolls = []
    for vec in (a, b):
        roll = vec.alloc_rollout(K, keys=("reward", "steer"))
        vec.drive(man, rollout=roll, steer_noise=torch.from_numpy(ref["noise"]).cuda() + 0.25)
        rolls.append(roll)
    torch.cuda.synchronize()
    assert np.array_equal(bits(rolls[0]["steer"]), bits(rolls[1]["steer"]))
    before = rolls[0]["steer"].clone()
    junk = torch.full((N, 2), 0.7, dtype=torch.float64, device="cuda:0")
    for k in range(3):
        a.step_device(junk, man[k])
        b.drive_step(man[k])
        torch.cuda.synchronize()
        for key in OUT_KEYS + ("obs",):
            assert np.array_equal(bits(a.out[key]), bits(b.out[key])), ("step after drive", k, key)
        assert np.array_equal(bits(a.steer_last), bits(b.steer_last)), ("step after drive", k, "steer_last")
        assert np.array_equal(bits(rolls[0]["steer"]), bits(before)), ("step after drive", k, "label rows written")
    fa, fb = final_of(a), final_of(b)
    for key in fb:
        assert np.array_equal(bits(fa[key]), bits(fb[key])), ("step after drive", key)
    assert (a.steer_last.abs() > 1e-3).any()
    # the C entry point itself: a call prepared with rows changes nothing on the handle, tc_step reads and writes none of them
    a.prepare_drive(man, rolls[0], torch.from_numpy(ref["noise"]).cuda())
    from tinycarlo_amd import _native as nat
    assert nat.lib().tc_step(a._h, None, nat.F64, man[3].data_ptr(), a._flags(), a._stream()) == 0
    b.drive_step(man[3])
    torch.cuda.synchronize()
    assert np.array_equal(bits(rolls[0]["steer"]), bits(before))
    for key in OUT_KEYS + ("obs",):
        assert np.array_equal(bits(a.out[key]), bits(b.out[key])), ("tc_step with rows installed", key)
    # the rows are a call's own: after drive call A (rollout A) and drive call B (rollout B), every tensor of A is bit-unchanged
    noise = torch.from_numpy(ref["noise"]).cuda()
    roll_a, roll_b = (a.alloc_rollout(K, keys=("reward", "cte", "steer")) for _ in range(2))
    a.drive(man, rollout=roll_a, steer_noise=noise)
    torch.cuda.synchronize()
    kept = {key: t.clone() for key, t in roll_a.items()}
    a.drive(man, rollout=roll_b, steer_noise=noise + 0.125)
    a.drive_step(man[0])
    torch.cuda.synchronize()
    for key, t in roll_a.items():
        assert np.array_equal(bits(t), bits(kept[key])), ("rollout of the earlier drive call written by a later one", key)
    assert not np.array_equal(bits(roll_b["steer"]), bits(roll_a["steer"]))  # (B ran on from A's state: its own labels)
    a.close()
    b.close()


def test_no_observation_drive_and_single_drive_steps(ref, stanley):
    """no_observation: one launch of tc_drive_env_kernel<.., false, ..>; drive_step: the fused step kernel, one step per call"""
    vec = drive_env()
    vec.no_observation = True
    assert vec.launch_info(K)["kernel"] == "tc_drive_env_kernel"
    keys = tuple(k for k in vec.alloc_rollout(1, keys="all") if k != "obs")
    roll = vec.alloc_rollout(K, keys=keys)
    vec.drive(torch.from_numpy(ref["man"]).cuda(), rollout=roll, steer_noise=torch.from_numpy(ref["noise"]).cuda())
    assert_rows(roll, ref, "no observation")
    assert_final(vec, ref, "no observation")
    vec.close()
    # drive_step takes no noise: its own reference, ten steps, with the camera (every step's bound outputs compared)
    vec = drive_env()
    assert vec.launch_info(1)["kernel"] == "tc_drive_step_kernel"
    twin = make_env()
    man = torch.from_numpy(ref["man"]).cuda()
    msa_i = 3
    for k in range(10):
        cte, he = twin.out["cte"], twin.out["heading_error"]
        nr = twin._aux["needs_reset"].bool().clone()
        # (the host law through tc_ctrl.h: torch.atan2 is not tc_atan2)
        cmd = torch.from_numpy(stanley(cte.cpu().numpy(), he.cpu().numpy(), GAIN, SPEED,
                                       twin.env_car_params[:, msa_i].cpu().numpy())).cuda()
        cc = torch.stack([torch.full_like(cmd, SPEED), cmd], dim=1).contiguous()
        twin.step_device(cc, man[k])
        vec.drive_step(man[k])
        torch.cuda.synchronize()
        for key in OUT_KEYS + ("obs",):
            assert np.array_equal(bits(vec.out[key]), bits(twin.out[key])), ("drive_step", k, key)
        assert np.array_equal(bits(vec.steer_last), bits(torch.where(nr, torch.zeros_like(cmd), cmd))), ("drive_step", k, "steer_last")
    want = final_of(twin)
    got = final_of(vec)
    for key, v in want.items():
        assert np.array_equal(bits(got[key]), bits(v)), ("drive_step final", key)
    vec.close()
    twin.close()


def test_replay_through_plain_step_multi(ref):
    """the recorded steer + noise rows and the speed, fed to plain step_multi on a fresh env without a controller, reproduce
    the rollout: the feature is tied to the existing K-step path as well"""
    vec = make_env()
    assert vec.launch_info(K)["kernel"] == "tc_envg_kernel+tc_frame_kernel"
    # a re-spawn step ignores its action (and the label row holds 0.0 there): any finite value does
    act = np.where(ref["fresh"], 0.0, ref["steer"]) + ref["noise"]
    assert np.array_equal(bits(act[~ref["fresh"]]), bits(ref["applied"][~ref["fresh"]]))
    cc = np.stack([np.full((K, N), SPEED), act], axis=2)
    roll = vec.alloc_rollout(K, keys="all")
    assert "steer" not in roll
    vec.step_multi(torch.from_numpy(cc).cuda(), torch.from_numpy(ref["man"]).cuda(), rollout=roll)
    assert_rows(roll, ref, "replay")
    assert_final(vec, ref, "replay")
    vec.close()


def test_controller_off_again_and_refusals(ref):
    from tinycarlo_amd import _native as nat
    L = nat.lib()
    a, b = make_env(), make_env()
    a.set_controller(k=GAIN, speed=SPEED)
    a.set_controller(None)
    assert a.steer_last is None and a.launch_info(K)["kernel"] == "tc_envg_kernel+tc_frame_kernel"
    rng = np.random.default_rng(5)
    cc = torch.from_numpy(np.stack([rng.uniform(0.3, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2)).cuda()
    man = torch.from_numpy(ref["man"]).cuda()
    ra, rb = a.alloc_rollout(K, keys="all"), b.alloc_rollout(K, keys="all")
    a.step_multi(cc, man, rollout=ra)
    b.step_multi(cc, man, rollout=rb)
    torch.cuda.synchronize()
    assert set(ra) == set(rb) and "steer" not in ra
    for k in ra:
        assert np.array_equal(bits(ra[k]), bits(rb[k])), k
    fa, fb = final_of(a), final_of(b)
    for k in fb:
        assert np.array_equal(bits(fa[k]), bits(fb[k])), k
    # without a controller the action is required
    assert L.tc_step_multi(a._h, None, nat.F64, man.data_ptr(), K, a._flags(), None, None, a._stream()) == -1
    assert L.tc_step(a._h, None, nat.F64, man.data_ptr(), a._flags(), a._stream()) == -1
    with pytest.raises(RuntimeError):
        a.drive(man)
    with pytest.raises(ValueError):
        a.alloc_rollout(K, keys=("steer",))
    # the setter's refusals
    last = torch.zeros(N, dtype=torch.float64, device="cuda:0")
    rows = torch.zeros((4, N), dtype=torch.float64, device="cuda:0")

    def ctl(kind=nat.CTRL_STANLEY, k=GAIN, speed=SPEED):
        return nat.ControllerC(kind, k, speed, last.data_ptr())

    def multi(n_steps, cc_ptr=None, **kw):  # tc_step_multi with the feature rows kw
        sr = nat.StepRows(**kw)
        return L.tc_step_multi(a._h, cc_ptr, nat.F64, man.data_ptr(), n_steps, a._flags() | nat.F_NO_OBSERVATION, None,
                               C.byref(sr), a._stream())
    for bad in (ctl(kind=2), ctl(kind=0), ctl(k=float("nan")), ctl(k=float("inf")), ctl(speed=float("-inf"))):
        assert L.tc_env_set_controller(a._h, C.byref(bad)) == -1
    assert a.launch_info(1)["kernel"] == "tc_step_kernel"  # a refused call installs nothing
    # rows for a feature that is off: no controller, steer rows
    for kw in ({"steer_out": rows.data_ptr()}, {"steer_noise_in": rows.data_ptr()}):
        assert multi(4, cc.data_ptr(), n_rows=4, **kw) == -1 and b"rows without a controller" in L.tc_last_error()
    assert L.tc_env_set_controller(a._h, C.byref(ctl())) == 0
    # the rows' own refusals: negative n_rows, rows with n_rows = 0, a K-step call longer than n_rows
    assert multi(4, n_rows=-1) == -1 and b"negative" in L.tc_last_error()
    for kw in ({"steer_out": rows.data_ptr()}, {"steer_noise_in": rows.data_ptr()}):
        assert multi(4, n_rows=0, **kw) == -1 and b"n_rows = 0" in L.tc_last_error()
        assert multi(5, n_rows=4, **kw) == -1 and b"rows" in L.tc_last_error()
    assert multi(5) == 0  # no rows: any length
    assert L.tc_step_multi(a._h, None, nat.F64, man.data_ptr(), 5, a._flags() | nat.F_NO_OBSERVATION, None, None, a._stream()) == 0
    with pytest.raises(ValueError):
        a.set_controller(k=float("nan"))
    torch.cuda.synchronize()
    a.close()
    b.close()


def test_graph_captured_drive_sees_new_gains(stanley):
    """a prepare_drive call captured into a HIP graph, replayed twice after set_controller(k=2.0): equals the host loop run
    with the gain each call had (the warm-up call ran with k = 4)"""
    Kg = 8
    man, noise = inputs(3 * Kg, seed=23)
    g_env = drive_env()
    mant = torch.zeros((Kg, N), dtype=torch.int32, device="cuda:0")
    noiset = torch.zeros((Kg, N), dtype=torch.float64, device="cuda:0")
    roll = g_env.alloc_rollout(Kg, keys="all")
    pc = g_env.prepare_drive(mant, roll, noiset)
    twin = make_env()
    rows, steer, _, _ = reference_loop(twin, stanley, man, noise, [(GAIN, SPEED)] * Kg + [(2.0, SPEED)] * (2 * Kg))
    ref_final = final_of(twin)
    twin.close()

    def load(i):
        mant.copy_(torch.from_numpy(man[i * Kg:(i + 1) * Kg]))
        noiset.copy_(torch.from_numpy(noise[i * Kg:(i + 1) * Kg]))

    def check(i):
        torch.cuda.synchronize()
        part = {"rows": {k: v[i * Kg:(i + 1) * Kg] for k, v in rows.items()}, "steer": steer[i * Kg:(i + 1) * Kg]}
        assert_rows(roll, part, ("graph call", i))
    load(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on a side stream, as torch recommends
        pc()
    torch.cuda.current_stream().wait_stream(s)
    check(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc()
    torch.cuda.synchronize()
    g_env.set_controller(k=2.0, speed=SPEED)  # in place: no re-capture
    for i in (1, 2):
        load(i)
        g.replay()
        check(i)
    got = final_of(g_env)
    for k, v in ref_final.items():
        assert np.array_equal(bits(got[k]), bits(v)), ("graph final", k)
    assert (np.abs(steer[Kg:]) > 1e-3).any()
    g_env.close()


def test_state_dict_carries_the_gains():
    a = drive_env(randomize=False, limit=0, wrappers=False)
    a.set_controller(k=2.5, speed=0.3)
    sd = a.state_dict()
    assert sd["controller"] == {"k": 2.5, "speed": 0.3}
    b = make_env(randomize=False, limit=0, wrappers=False)
    b.load_state_dict(sd)
    assert b._ctrl == {"k": 2.5, "speed": 0.3}
    man = torch.zeros((4, N), dtype=torch.int32, device="cuda:0")
    a.drive(man)
    b.drive(man)
    torch.cuda.synchronize()
    for k in a.state:
        assert torch.equal(a.state[k], b.state[k]), k
    assert torch.equal(a.steer_last.view(torch.int64), b.steer_last.view(torch.int64))
    sd["controller"] = None
    b.load_state_dict(sd)
    assert b._ctrl is None and b.launch_info(4)["kernel"].startswith("tc_envg_kernel")
    a.close()
    b.close()
