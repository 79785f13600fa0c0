"""Episode time limit and per-env episode statistics (set_time_limit / track_episodes), bit-exact against the CPU oracle.

The oracle knows nothing of time limits.  The expected run steps an OracleVecEnv one step at a time with autoreset on,
applies the accounting rules of include/tinycarlo_hip.h (tc_env_set_episodes) in numpy after each step, ORs the
time-limit mask into the expected truncated / status and hands it to request_reset(), so that the oracle re-spawns
exactly the envs the device must re-spawn.  Run on the MI355X box with `pytest -m gpu`."""
import copy
import os

import numpy as np
import pytest

import orc
from common import load_cfg
from feature_ref import Ref  # the expected run: an oracle env plus rules 1-3 in numpy

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STATE_F = ("x", "y", "theta", "velocity", "steering", "radius", "front_x", "front_y")
EP_KEYS = ("length", "ret", "count", "last_length", "last_return", "length_sum", "return_sum")
S_NOT_RESET, S_TIME_LIMIT = 8, 32


@pytest.fixture(autouse=True)
def _portable_math():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def cfg_for(map_name="simple_layout", res=(64, 64), fmt="classes"):
    cfg, path = load_cfg(map_name)
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = list(res)
    cfg["sim"]["observation_space_format"] = fmt
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


def make_env(n, **kw):
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    return TinyCarloVecEnv(cfg_for(), num_envs=n, device="cuda:0", **kw)


def make_ref(n, **kw):
    from oracle_backend import OracleVecEnv
    return OracleVecEnv(cfg_for(), num_envs=n, **kw)


def stack_terms():
    """CTELinearRewardWrapper + CTETerminationWrapper(number_of_steps=2), as fused terms"""
    from tinycarlo_amd import terms as T
    return [T.cte_linear_reward(0.02, 1.0, -0.5), T.cte_termination(0.012, 2)]


def actions(K, N, seed, lo=0.5):
    rng = np.random.default_rng(seed)
    cc = np.stack([rng.uniform(lo, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2)
    return cc, rng.integers(0, 4, (K, N)).astype(np.int32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def check_step(env, exp, label, obs=True):
    """everything step() returns, the state and every episode tensor of `env` against the expected step"""
    torch.cuda.synchronize()
    for k in STATE_F + ("lp_len", "local_path", "last_maneuver"):
        assert np.array_equal(bits(env.state[k].cpu().numpy()), bits(exp["state"][k])), (label, k)
    for k in ("cte", "heading_error", "reward", "terminated", "truncated", "status", "laneline_distances", "nearest_edge"):
        assert np.array_equal(bits(env.out[k].cpu().numpy()), bits(exp[k])), (label, k)
    if obs:
        assert np.array_equal(env.out["obs"].cpu().numpy(), exp["obs"]), (label, "obs")
    assert np.array_equal(env._aux["needs_reset"].cpu().numpy(), exp["needs_reset"]), (label, "needs_reset")
    for k in EP_KEYS:
        assert np.array_equal(bits(env.episode_stats[k].cpu().numpy()), bits(exp["ep"][k])), (label, "episode", k)


def closed_loop(N, T, spawn, limit, per_env, terms, stagger, seed, act_seed):
    env, oenv = make_env(N, autoreset=True, spawn=spawn), make_ref(N, autoreset=True, spawn=spawn)
    if terms:
        for e in (env, oenv):
            e.wrapped = True
            e.set_terms(stack_terms())
    lim = np.asarray(per_env if per_env is not None else limit)
    env.set_time_limit(limit, per_env=per_env)
    env.reset(seed=seed)
    length0 = None
    if stagger:
        length0 = (np.arange(N) * 3) % max(int(np.max(lim)), 1)
        env.episode_stats["length"].copy_(torch.from_numpy(length0.astype(np.int32)))
    ref = Ref(oenv, lim, None)
    ref.reset(seed)
    if length0 is not None:
        ref.ep["length"][:] = length0
    cc, man = actions(T, N, act_seed)
    for t in range(T):
        obs, rew, term, trunc, info = env.step({"car_control": cc[t], "maneuver": man[t]})
        exp = ref.step(cc[t], man[t])
        check_step(env, exp, f"step {t}")
        assert np.array_equal(info["episode_length"].cpu().numpy(), exp["ep"]["length"])
        assert np.array_equal(bits(info["episode_return"].cpu().numpy()), bits(exp["ep"]["ret"]))
        assert np.array_equal(trunc.cpu().numpy(), exp["truncated"].astype(bool))
    ref.assert_not_vacuous()
    env.close()
    return ref


def test_closed_loop_base_reward_shared_limit_host_spawn():
    ref = closed_loop(64, 80, "host", 12, None, terms=False, stagger=False, seed=3, act_seed=1)
    assert (ref.ep["last_length"][ref.by_limit & ~ref.by_other] == 12).all()


def test_closed_loop_fused_stack_per_env_limit_device_spawn_staggered():
    N = 64
    per_env = 6 + (np.arange(N) % 5) * 4  # 6 .. 22
    per_env[5] = 0  # no limit for this env
    closed_loop(N, 80, "device", None, per_env, terms=True, stagger=True, seed=5, act_seed=2)


def test_closed_loop_fused_stack_shared_limit_host_spawn_staggered():
    closed_loop(64, 60, "host", 16, None, terms=True, stagger=True, seed=9, act_seed=4)


def _multi_case(N, K, limit, stream_env, oracle_obs=True, seed=7, act_seed=11, min_count=0):
    """one K-step call with rows against K single steps on a twin and against the oracle, row by row"""
    old = os.environ.get("TC_STREAM")
    if stream_env is not None:
        os.environ["TC_STREAM"] = stream_env
    try:
        a, b = make_env(N, autoreset=True), make_env(N, autoreset=True)
    finally:
        if stream_env is not None:
            if old is None:
                del os.environ["TC_STREAM"]
            else:
                os.environ["TC_STREAM"] = old
    oenv = make_ref(N, autoreset=True)
    oenv.no_observation = not oracle_obs
    for e in (a, b, oenv):
        e.wrapped = True
        e.set_terms(stack_terms())
    length0 = ((np.arange(N) * 5) % limit).astype(np.int32)
    for e in (a, b):
        e.set_time_limit(limit)
        e.reset(seed=seed)
        e.episode_stats["length"].copy_(torch.from_numpy(length0))
    ref = Ref(oenv, limit)
    ref.reset(seed)
    ref.ep["length"][:] = length0
    cc, man = actions(K, N, act_seed)
    cct, mant = torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda()
    roll = a.alloc_rollout(K, keys="all")
    assert "episode_length" in roll and "episode_return" in roll
    assert a.launch_info(K)["kernel"] == "tc_envg_kernel+tc_frame_kernel"
    a.step_multi(cct, mant, rollout=roll)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in roll.items()}
    for k in range(K):
        b.step({"car_control": cct[k], "maneuver": mant[k]})
        exp = ref.step(cc[k], man[k])
        check_step(b, exp, f"single step {k}", obs=oracle_obs)
        for key in ("reward", "terminated", "truncated", "status", "cte", "heading_error", "laneline_distances", "nearest_edge"):
            assert np.array_equal(bits(r[key][k]), bits(exp[key])), ("row", k, key)
        assert np.array_equal(r["episode_length"][k], exp["ep"]["length"]), ("row", k)
        assert np.array_equal(bits(r["episode_return"][k]), bits(exp["ep"]["ret"])), ("row", k)
        assert np.array_equal(r["obs"][k], b.out["obs"].cpu().numpy()), ("row", k, "obs")
        info = a.rollout_info(roll, k)
        assert torch.equal(info["episode_length"], roll["episode_length"][k])
    check_step(a, exp, "after the K-step call", obs=False)
    for k in a.state:
        assert torch.equal(a.state[k], b.state[k]), k
    ref.assert_not_vacuous()
    assert ref.ep["count"].max() >= min_count
    a.close()
    b.close()
    return ref


def test_step_multi_rows_small_streamed():
    _multi_case(96, 40, 9, None)


def test_step_multi_rows_small_chunked():
    _multi_case(96, 40, 9, "0")


def test_step_multi_spans_several_limits_in_one_launch():
    ref = _multi_case(64, 48, 5, None, min_count=2)
    assert ref.ep["count"].max() >= 2  # one env ended more than one episode inside the one launch


@pytest.mark.parametrize("stream_env", [None, "0"])
def test_step_multi_rows_cfg3_shape(stream_env):
    _multi_case(4096, 24, 10, stream_env, oracle_obs=False)


def test_no_observation_k_step_call_matches_single_steps():
    """tc_env_kernel (state in LDS across the steps of the launch) against single steps"""
    N, K = 64, 40
    a, b = make_env(N, autoreset=True), make_env(N, autoreset=True)
    for e in (a, b):
        e.no_observation = True
        e.set_time_limit(7)
        e.reset(seed=2)
    cc, man = actions(K, N, 3)
    cct, mant = torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda()
    roll = a.alloc_rollout(K, keys=("reward", "truncated", "status", "episode_length", "episode_return"))
    assert a.launch_info(K)["kernel"] == "tc_env_kernel"
    a.step_multi(cct, mant, rollout=roll)
    for k in range(K):
        b.step({"car_control": cct[k], "maneuver": mant[k]})
        torch.cuda.synchronize()
        assert torch.equal(roll["episode_length"][k], b.episode_stats["length"]), k
        assert torch.equal(roll["episode_return"][k].view(torch.int64), b.episode_stats["ret"].view(torch.int64)), k
        assert torch.equal(roll["truncated"][k], b.out["truncated"]), k
        assert torch.equal(roll["status"][k], b.out["status"]), k
    for k in EP_KEYS:
        assert torch.equal(a.episode_stats[k], b.episode_stats[k]), k
    assert int(a.episode_stats["count"].min()) >= 4 and int((roll["status"] & S_TIME_LIMIT).count_nonzero()) > 0
    a.close()
    b.close()


def test_time_limit_respawns_draw_new_cars():
    from tinycarlo_amd.randomization import car_ranges, draw_car_params
    N, K, seed = 64, 30, 17
    ranges = {"wheelbase": (0.05, 0.08), "max_velocity": (0.5, 1.2), "steering_shift": (-0.05, 0.05)}
    a, b = make_env(N, autoreset=True, spawn="device"), make_env(N, autoreset=True, spawn="device")
    for e in (a, b):
        e.randomize_cars(ranges, seed=seed)
        e.set_time_limit(6)
        e.reset(seed=1)
    lo, hi, mask = car_ranges(a.car_params, ranges)
    cols = [j for j in range(8) if (mask >> j) & 1]  # the drawn columns (the others keep the config's values)
    cc, man = actions(K, N, 8, lo=0.2)
    cct, mant = torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda()
    a.step_multi(cct, mant, rollout=a.alloc_rollout(K, keys=("obs", "truncated", "episode_length")))
    respawns = np.zeros(N, np.int64)
    for k in range(K):
        respawns += b._aux["needs_reset"].cpu().numpy()
        b.step({"car_control": cct[k], "maneuver": mant[k]})
    torch.cuda.synchronize()
    ep = b.car_episode.cpu().numpy()
    assert np.array_equal(ep, 1 + respawns) and respawns.min() >= 4  # every env re-spawned by its limit: K / (6 + 1)
    assert np.array_equal(b.env_car_params.cpu().numpy()[:, cols], draw_car_params(seed, np.arange(N), ep - 1, lo, hi)[:, cols])
    assert torch.equal(a.car_episode, b.car_episode) and torch.equal(a.env_car_params, b.env_car_params)
    for k in EP_KEYS:
        assert torch.equal(a.episode_stats[k], b.episode_stats[k]), k
    a.close()
    b.close()


def test_reset_mask_zeroes_only_the_selected_envs():
    N = 32
    env = make_env(N)
    env.track_episodes()
    env.reset(seed=4)
    cc, man = actions(5, N, 1)
    for t in range(5):
        env.step({"car_control": cc[t], "maneuver": man[t]})
    before = {k: v.clone() for k, v in env.episode_stats.items()}
    assert int(before["length"].min()) == 5 and float(before["ret"].abs().max()) > 0
    mask = np.arange(N) % 3 == 0
    env.reset(mask=mask)
    torch.cuda.synchronize()
    m = torch.from_numpy(mask).cuda()
    assert int(env.episode_stats["length"][m].abs().max()) == 0 and float(env.episode_stats["ret"][m].abs().max()) == 0.0
    for k in EP_KEYS:
        assert torch.equal(env.episode_stats[k][~m], before[k][~m]), k
    for k in ("count", "last_length", "last_return", "length_sum", "return_sum"):
        assert torch.equal(env.episode_stats[k], before[k]), k
    env.close()


def test_without_autoreset_length_keeps_counting_past_the_limit():
    N, T, limit = 32, 12, 5
    env, oenv = make_env(N), make_ref(N)
    env.set_time_limit(limit)
    env.reset(seed=6)
    ref = Ref(oenv, limit)
    ref.reset(6)
    cc, man = actions(T, N, 2)
    for t in range(T):
        env.step({"car_control": cc[t], "maneuver": man[t]})
        exp = ref.step(cc[t], man[t])
        check_step(env, exp, f"step {t}")
        if t + 1 >= limit:
            assert env.out["truncated"].all() and (env.out["status"] & S_TIME_LIMIT).all()
    assert int(env.episode_stats["length"].min()) == T and int(env.episode_stats["count"].min()) >= T - limit + 1
    env.close()


def test_feature_off_after_on_equals_never_on():
    N = 64
    a, b = make_env(N, autoreset=True), make_env(N, autoreset=True)
    a.set_time_limit(4)
    a.reset(seed=8)
    b.reset(seed=8)
    a.track_episodes(False)
    assert a.episode_stats is None
    cc, man = actions(24, N, 5)
    for t in range(12):
        _, _, _, _, info = a.step({"car_control": cc[t], "maneuver": man[t]})
        b.step({"car_control": cc[t], "maneuver": man[t]})
        assert "episode_length" not in info
    cct, mant = torch.from_numpy(cc[12:]).cuda(), torch.from_numpy(man[12:]).cuda()
    ra, rb = a.alloc_rollout(12, keys="all"), b.alloc_rollout(12, keys="all")
    assert "episode_length" not in ra
    a.step_multi(cct, mant, rollout=ra)
    b.step_multi(cct, mant, rollout=rb)
    torch.cuda.synchronize()
    for d in ("state", "out", "_aux"):
        for k, t in getattr(a, d).items():
            assert torch.equal(t, getattr(b, d)[k]), (d, k)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert not (a.out["status"] & S_TIME_LIMIT).any()
    with pytest.raises(ValueError):
        a.alloc_rollout(4, keys=("episode_length",))
    a.close()
    b.close()


def test_graph_captured_call_equals_eager_and_sees_a_new_limit():
    N, K = 64, 16
    g_env, e_env = make_env(N, autoreset=True), make_env(N, autoreset=True)
    for e in (g_env, e_env):
        e.set_time_limit(6)
        e.reset(seed=1)
    cc, man = actions(K, N, 4)
    cct, mant = torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda()
    keys = ("obs", "reward", "terminated", "truncated", "status", "episode_length", "episode_return")
    roll, e_roll = g_env.alloc_rollout(K, keys=keys), e_env.alloc_rollout(K, keys=keys)
    pc = g_env.prepare_step_multi(cct, mant, roll)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pc()  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    e_env.step_multi(cct, mant, rollout=e_roll)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc()
    torch.cuda.synchronize()
    for it in range(3):  # (capturing enqueued nothing: the first replay is call number two of both envs)
        if it == 2:  # a limit changed between replays takes effect without re-capture
            g_env.set_time_limit(3)
            e_env.set_time_limit(3)
        e_env.step_multi(cct, mant, rollout=e_roll)
        g.replay()
        torch.cuda.synchronize()
        for k in roll:
            assert torch.equal(roll[k], e_roll[k]), (it, k)
        for k in EP_KEYS:
            assert torch.equal(g_env.episode_stats[k], e_env.episode_stats[k]), (it, k)
        for k in g_env.state:
            assert torch.equal(g_env.state[k], e_env.state[k]), (it, k)
    assert int(roll["episode_length"][-1].max()) <= 3 and int(roll["episode_length"][:4].max()) > 3
    g_env.close()
    e_env.close()


def test_state_dict_round_trip_mid_episode():
    N = 64
    per_env = 5 + np.arange(N) % 7
    a = make_env(N, autoreset=True)
    a.set_time_limit(None, per_env=per_env)
    a.reset(seed=2)
    cc, man = actions(50, N, 6)
    for t in range(13):
        a.step({"car_control": cc[t], "maneuver": man[t]})
    sd = a.state_dict()
    assert sd["episodes"]["max_episode_steps"] == 0 and np.array_equal(sd["episodes"]["per_env"].numpy(), per_env)
    assert int(sd["episodes"]["stats"]["length"].max()) > 0
    b = make_env(N, autoreset=True)
    b.load_state_dict(sd)
    for t in range(13, 50):
        a.step({"car_control": cc[t], "maneuver": man[t]})
        b.step({"car_control": cc[t], "maneuver": man[t]})
    torch.cuda.synchronize()
    for d in ("state", "out", "_aux", "episode_stats"):
        for k, t_ in getattr(a, d).items():
            assert torch.equal(t_, getattr(b, d)[k]), (d, k)
    old = {k: v for k, v in sd.items() if k != "episodes"}  # a checkpoint from before the feature still loads: off
    b.load_state_dict(old)
    assert b.episode_stats is None
    a.close()
    b.close()


def test_argument_validation_with_a_live_handle():
    import ctypes as C
    from tinycarlo_amd import _native as nat
    env = make_env(8)
    L = nat.lib()
    rows = torch.zeros((4, 8), dtype=torch.int32, device="cuda:0")
    cc = torch.zeros((5, 8, 2), dtype=torch.float32, device="cuda:0")
    man = torch.zeros((5, 8), dtype=torch.int32, device="cuda:0")

    def multi(n_steps, **kw):  # tc_step_multi with the feature rows kw
        sr = nat.StepRows(**kw)
        return L.tc_step_multi(env._h, cc.data_ptr(), nat.F32, man.data_ptr(), n_steps, nat.F_NO_OBSERVATION, None, C.byref(sr), None)
    env.reset(seed=0)
    assert multi(4, n_rows=4, episode_length_out=rows.data_ptr()) == -1  # rows for a feature that is off
    assert b"episode buffers" in L.tc_last_error()
    env.track_episodes()
    assert multi(4, n_rows=-1, episode_length_out=rows.data_ptr()) == -1
    assert multi(4, n_rows=0, episode_length_out=rows.data_ptr()) == -1 and b"n_rows = 0" in L.tc_last_error()
    assert multi(5, n_rows=4, episode_length_out=rows.data_ptr()) == -1 and b"rows" in L.tc_last_error()  # a K-step call longer than n_rows
    torch.cuda.synchronize()
    assert int(rows.abs().sum()) == 0 and int(env.episode_stats["length"].sum()) == 0  # a refused call writes nothing
    assert multi(4, n_rows=4, episode_length_out=rows.data_ptr()) == 0
    assert multi(5) == 0  # no rows: any length
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), np.tile(np.arange(1, 5, dtype=np.int32)[:, None], (1, 8)))
    b = nat.EpisodeBuffers()
    b.length = rows.data_ptr()
    assert L.tc_env_set_episodes(env._h, C.byref(b), 5) == -1  # ret missing
    env.close()


def test_single_env_max_episode_steps():
    from tinycarlo_amd import gym
    import tinycarlo_amd  # noqa: F401  (registers tinycarlo-v2)
    env = gym.make("tinycarlo-v2", config=cfg_for(), max_episode_steps=5)
    for ep in range(2):
        env.reset(seed=ep)
        flags = []
        for t in range(5):
            _, _, terminated, truncated, _ = env.step({"car_control": [0.3, 0.0], "maneuver": 0})
            flags.append((terminated, truncated))
        assert flags == [(False, False)] * 4 + [(False, True)], flags
    env.close()
