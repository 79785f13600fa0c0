"""Per-env car constants (set_env_cars), their per-episode draw on the device (randomize_cars) and live shared-car
constants, bit-exact against the CPU oracle (tests/orc.py).  Run on the MI355X box with `pytest -m gpu`."""
import copy
import dataclasses
import os

import numpy as np
import pytest

import orc
from common import load_cfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STATE_F = ("x", "y", "theta", "velocity", "steering", "radius", "front_x", "front_y")
COLS = ("wheelbase", "track_width", "max_velocity", "max_steering_angle", "steering_speed", "max_acceleration",
        "max_deceleration")


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


def make_env(n, map_name="simple_layout", res=(64, 64), **kw):
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    return TinyCarloVecEnv(cfg_for(map_name, res), num_envs=n, device="cuda:0", **kw)


def params_of_row(p, row):
    return dataclasses.replace(p, **{c: float(row[j]) for j, c in enumerate(COLS)})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_env(env, o, idx, C, obs=True, label=""):
    """env rows `idx` against rows `idx` of oracle batch `o` (state, info, reward, terminated, obs), bit for bit"""
    torch.cuda.synchronize()
    for k in STATE_F:
        assert np.array_equal(bits(env.state[k].cpu().numpy()[idx]), bits(o.state[k][idx])), (label, k)
    assert np.array_equal(env.state["lp_len"].cpu().numpy()[idx], o.state["lp_len"][idx]), label
    for k in ("cte", "heading_error", "reward"):
        assert np.array_equal(bits(env.out[k].cpu().numpy()[idx]), bits(o.info[k][idx])), (label, k)
    assert np.array_equal(env.out["terminated"].cpu().numpy()[idx].astype(bool), o.info["terminated"][idx].astype(bool)), label
    assert np.array_equal(env.out["truncated"].cpu().numpy()[idx].astype(bool), o.info["truncated"][idx].astype(bool)), label
    gd = env.out["laneline_distances"].cpu().numpy()[idx]
    assert np.array_equal(bits(gd), bits(o.info["dist"][idx, :C])), label
    assert np.array_equal(env.out["nearest_edge"].cpu().numpy()[idx], o.info["nearest_edge"][idx, :C]), label
    if obs:
        g = env.out["obs"].cpu().numpy().reshape(env.num_envs, -1)[idx]
        assert np.array_equal(g, o.obs[idx]), label


def variants(p):
    """four cars that differ in every column, shift included (limits stay positive)"""
    out = []
    for k, (f, sh) in enumerate([(0.7, -0.05), (1.0, 0.0), (1.3, 0.03), (1.6, 0.2)]):
        row = [p.wheelbase * f, p.track_width * (2.2 - f), p.max_velocity * f, p.max_steering_angle * (2.1 - f),
               p.steering_speed * (0.5 + f), p.max_acceleration * f * f, p.max_deceleration * (2.4 - f), sh]
        out.append(np.array(row))
    return out


def test_four_car_variants_against_oracles():
    N = 64
    env = make_env(N)
    p = env.car_params
    var = variants(p)
    pick = np.arange(N) % 4
    rows = np.stack([var[k] for k in pick])
    env.set_env_cars(**{c: rows[:, j] for j, c in enumerate(COLS)}, steering_shift=rows[:, 7])
    assert torch.equal(env.env_car_params.cpu(), torch.from_numpy(rows))
    oracles = [orc.Oracle(env.map, params_of_row(p, var[k]), env.camera, orc.FMT_CLASSES, N, threads=4) for k in range(4)]
    env.reset(seed=11)
    nodes = env._keep[0].cpu().numpy()
    for o in oracles:
        o.reset(nodes)
    rng = np.random.default_rng(5)
    for t in range(16):
        cc = np.stack([rng.uniform(-0.3, 1, N), rng.uniform(-1, 1, N)], axis=1)
        man = rng.integers(0, 4, N).astype(np.int32)
        env.step({"car_control": cc, "maneuver": man})
        for k, o in enumerate(oracles):
            ck = cc.copy()
            ck[:, 1] = ck[:, 1] + var[k][7]  # the shift is added before the clip (the oracle clips)
            o.step(ck, man)
        for k in range(4):
            check_env(env, oracles[k], np.flatnonzero(pick == k), env.n_classes, label=f"variant {k} step {t}")
    assert not np.array_equal(oracles[0].state["x"], oracles[3].state["x"])  # the variants really drove apart
    env.close()


def _identity_pair(n, map_name="simple_layout", res=(64, 64)):
    a, b = make_env(n, map_name, res), make_env(n, map_name, res)
    p = a.car_params
    a.set_env_cars(**{c: getattr(p, c) for c in COLS}, steering_shift=0.0)
    return a, b


def _same(a, b, label):
    torch.cuda.synchronize()
    for d in ("state", "out"):
        for k, t in getattr(a, d).items():
            assert torch.equal(t, getattr(b, d)[k]), (label, d, k)


def test_identity_rows_equal_the_shared_car():
    N = 64
    a, b = _identity_pair(N)
    a.reset(seed=3)
    b.reset(seed=3)
    rng = np.random.default_rng(1)
    for t in range(16):
        cc = np.stack([rng.uniform(0, 1, N), rng.uniform(-1, 1, N)], axis=1).astype(np.float32)
        man = rng.integers(0, 4, N).astype(np.int32)
        a.step({"car_control": cc, "maneuver": man})
        b.step({"car_control": cc, "maneuver": man})
        _same(a, b, f"step {t}")
    K = 32
    cc = torch.from_numpy(np.stack([rng.uniform(0, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2).astype(np.float32)).cuda()
    man = torch.from_numpy(rng.integers(0, 4, (K, N)).astype(np.int32)).cuda()
    ra, rb = a.alloc_rollout(K, keys="all"), b.alloc_rollout(K, keys="all")
    assert a.launch_info(K)["kernel"] == "tc_envg_kernel+tc_frame_kernel"
    a.step_multi(cc, man, rollout=ra)
    b.step_multi(cc, man, rollout=rb)
    _same(a, b, "step_multi")
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    a.close()
    b.close()
    # knuffingen 128x128: component-group frames (single steps, a streamed K-step call) and the map's own simulate
    # variant (a K-step call without observations: the one-wavefront-per-env kernel)
    a, b = _identity_pair(32, "knuffingen", (128, 128))
    a.reset(seed=4)
    b.reset(seed=4)
    for t in range(4):
        cc1 = np.stack([rng.uniform(0.3, 1, 32), rng.uniform(-1, 1, 32)], axis=1)
        man1 = rng.integers(0, 4, 32).astype(np.int32)
        a.step({"car_control": cc1, "maneuver": man1})
        b.step({"car_control": cc1, "maneuver": man1})
        _same(a, b, f"knuffingen step {t}")
    K = 24
    cc = torch.from_numpy(np.stack([rng.uniform(0.3, 1, (K, 32)), rng.uniform(-1, 1, (K, 32))], axis=2)).cuda()
    man = torch.from_numpy(rng.integers(0, 4, (K, 32)).astype(np.int32)).cuda()
    ra, rb = a.alloc_rollout(K, keys="all"), b.alloc_rollout(K, keys="all")
    a.step_multi(cc, man, rollout=ra)
    b.step_multi(cc, man, rollout=rb)
    _same(a, b, "knuffingen step_multi")
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert int(ra["obs"].max()) == 255
    for e in (a, b):
        e.no_observation = True
    a.step_multi(cc, man)
    b.step_multi(cc, man)
    _same(a, b, f"knuffingen no-observation step_multi ({a.launch_info(K)})")
    a.close()
    b.close()


@pytest.mark.parametrize("fuse", [True, False])
def test_track_width_terms_per_env(fuse):
    import tinycarlo_amd.wrapper as W
    from tinycarlo_amd import terms as T
    N = 48
    env = make_env(N)
    p = env.car_params
    tws = np.array([p.track_width * 0.6, p.track_width, p.track_width * 1.8])
    pick = np.arange(N) % 3
    env.set_env_cars(track_width=tws[pick])
    names = env.layer_names
    w = W.LanelineSparseRewardWrapper(env, {names[0]: 1.0, names[-1]: -2.0}, fuse=fuse)
    w = W.LanelineLinearRewardWrapper(w, {n: 0.5 for n in names}, fuse=fuse)
    w = W.LanelineCrossingTerminationWrapper(w, [names[0]], fuse=fuse)
    assert bool(w.fused) == fuse
    terms = [T.laneline_sparse_reward(names, {names[0]: 1.0, names[-1]: -2.0}),
             T.laneline_linear_reward(names, {n: 0.5 for n in names}), T.laneline_crossing_termination(names, [names[0]])]
    oracles = []
    for k in range(3):
        o = orc.Oracle(env.map, dataclasses.replace(p, track_width=float(tws[k])), env.camera, orc.FMT_CLASSES, N, threads=4)
        o.terms = terms
        oracles.append(o)
    w.reset(seed=8)
    nodes = env._keep[0].cpu().numpy()
    for o in oracles:
        o.reset(nodes)
    rng = np.random.default_rng(2)
    fired = 0
    for t in range(20):
        cc = np.stack([rng.uniform(0.5, 1, N), rng.uniform(-1, 1, N)], axis=1)
        man = rng.integers(0, 4, N).astype(np.int32)
        _, r, te, _, _ = w.step({"car_control": cc, "maneuver": man})
        for o in oracles:
            o.step(cc, man, flags=orc.F_WRAPPED)
        r, te = r.cpu().numpy(), te.cpu().numpy().astype(bool)
        for k in range(3):
            idx = np.flatnonzero(pick == k)
            assert np.array_equal(bits(r[idx]), bits(oracles[k].info["reward"][idx])), (fuse, t, k)
            assert np.array_equal(te[idx], oracles[k].info["terminated"][idx].astype(bool)), (fuse, t, k)
        fired += int(te.sum())
    assert fired > 0
    env.close()


def _ranges(p):
    return {"wheelbase": (p.wheelbase * 0.7, p.wheelbase * 1.4), "track_width": (p.track_width * 0.8, p.track_width * 1.5),
            "max_velocity": (p.max_velocity * 0.8, p.max_velocity * 1.6),
            "max_steering_angle": (p.max_steering_angle * 0.6, p.max_steering_angle * 1.2),
            "steering_speed": (p.steering_speed * 0.5, p.steering_speed * 3.0),
            "max_acceleration": (p.max_acceleration * 0.5, p.max_acceleration * 2.0),
            "max_deceleration": (p.max_deceleration * 0.5, p.max_deceleration * 1.5), "steering_shift": (-0.08, 0.08)}


def _rand_env(N, seed, env_offset=0, max_cte=None):
    from tinycarlo_amd import terms as T
    env = make_env(N, autoreset=True, spawn="host")
    env.randomize_cars(_ranges(env.car_params), seed=seed, env_offset=env_offset)
    if max_cte is not None:
        env.set_terms([T.cte_termination(max_cte, 1)])
    return env


def test_per_episode_resampling_against_oracles():
    from tinycarlo_amd import terms as T
    from tinycarlo_amd.randomization import draw_car_params
    N, seed = 128, 77
    env = _rand_env(N, seed, max_cte=0.012)
    p = env.car_params
    lo_hi = _ranges(p)
    lo = np.array([lo_hi[c][0] for c in COLS + ("steering_shift",)])
    hi = np.array([lo_hi[c][1] for c in COLS + ("steering_shift",)])
    env.reset(seed=seed)
    episode = np.ones(N, dtype=np.int64)  # reset drew episode 0
    rows = draw_car_params(seed, np.arange(N), 0, lo, hi)
    torch.cuda.synchronize()
    assert np.array_equal(env.env_car_params.cpu().numpy(), rows)
    assert np.array_equal(env.car_episode.cpu().numpy(), episode)
    nodes = env._keep[0].cpu().numpy()
    queue = env._aux["spawn_queue"].cpu().numpy()
    oracles = []
    for i in range(N):
        o = orc.Oracle(env.map, params_of_row(p, rows[i]), env.camera, orc.FMT_CLASSES, 1)
        o.terms = [T.cte_termination(0.012, 1)]
        o.spawn_queue = queue[i:i + 1].copy()
        o.reset(nodes[i:i + 1])
        oracles.append(o)
    rng = np.random.default_rng(9)
    respawns = 0

    def oracle_step(cc, man):
        nonlocal respawns
        for i, o in enumerate(oracles):
            if o.needs_reset[0]:
                rows[i] = draw_car_params(seed, i, episode[i], lo, hi)
                episode[i] += 1
                o.car = orc.make_car(params_of_row(p, rows[i]))
                respawns += 1
            ck = cc[i:i + 1].copy()
            ck[0, 1] += rows[i][7]
            o.step(ck, man[i:i + 1], flags=orc.F_AUTORESET, with_obs=False)

    def check(label, roll=None, k=None):
        for i, o in enumerate(oracles):
            if roll is None:
                st = {f: env.state[f][i].item() for f in ("x", "y", "theta", "velocity")}
                out = {f: env.out[f][i].item() for f in ("cte", "reward")}
                term = bool(env.out["terminated"][i].item())
            else:
                st = {f: roll[f][k, i].item() for f in ("x", "y", "theta", "velocity")}
                out = {f: roll[f][k, i].item() for f in ("cte", "reward")}
                term = bool(roll["terminated"][k, i].item())
            for f, v in st.items():
                assert bits(v) == bits(o.state[f][0]), (label, i, f)
            for f, v in out.items():
                assert bits(v) == bits(o.info[f][0]), (label, i, f)
            assert term == bool(o.info["terminated"][0]), (label, i)

    for t in range(40):
        cc = np.stack([rng.uniform(0.5, 1, N), rng.uniform(-1, 1, N)], axis=1)
        man = rng.integers(0, 4, N).astype(np.int32)
        env.step({"car_control": cc, "maneuver": man})
        oracle_step(cc, man)
        torch.cuda.synchronize()
        ep = env.car_episode.cpu().numpy()
        assert np.array_equal(ep, episode), t
        assert np.array_equal(env.env_car_params.cpu().numpy(), draw_car_params(seed, np.arange(N), ep - 1, lo, hi)), t
        check(f"step {t}")
    K = 24
    cck = np.stack([rng.uniform(0.5, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2)
    mank = rng.integers(0, 4, (K, N)).astype(np.int32)
    roll = env.alloc_rollout(K, keys="all")
    env.step_multi(torch.from_numpy(cck).cuda(), torch.from_numpy(mank).cuda(), rollout=roll)
    torch.cuda.synchronize()
    roll = {k: v.cpu().numpy() for k, v in roll.items()}
    for k in range(K):
        oracle_step(cck[k], mank[k])
        check(f"step_multi row {k}", roll, k)
    ep = env.car_episode.cpu().numpy()
    assert np.array_equal(ep, episode)
    assert np.array_equal(env.env_car_params.cpu().numpy(), draw_car_params(seed, np.arange(N), ep - 1, lo, hi))
    assert respawns >= 64, respawns
    env.close()


def _actions(rng, K, N):
    cc = torch.from_numpy(np.stack([rng.uniform(0.5, 1, (K, N)), rng.uniform(-1, 1, (K, N))], axis=2)).cuda()
    man = torch.from_numpy(rng.integers(0, 4, (K, N)).astype(np.int32)).cuda()
    return cc, man


def test_graph_captured_step_multi_resamples_like_eager():
    N, K = 64, 16
    g_env, e_env = _rand_env(N, 5, max_cte=0.012), _rand_env(N, 5, max_cte=0.012)
    g_env.reset(seed=1)
    rng = np.random.default_rng(4)
    cc, man = _actions(rng, K, N)
    roll = g_env.alloc_rollout(K, keys=("obs", "reward", "terminated", "truncated"))
    pc = g_env.prepare_step_multi(cc, man, roll)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pc()  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc()
    torch.cuda.synchronize()
    e_env.load_state_dict(g_env.state_dict())
    e_roll = e_env.alloc_rollout(K, keys=("obs", "reward", "terminated", "truncated"))
    for it in range(4):
        g.replay()
        e_env.step_multi(cc, man, rollout=e_roll)
        torch.cuda.synchronize()
        _same(g_env, e_env, f"replay {it}")
        for k in roll:
            assert torch.equal(roll[k], e_roll[k]), (it, k)
        assert torch.equal(g_env.env_car_params, e_env.env_car_params), it
        assert torch.equal(g_env.car_episode, e_env.car_episode), it
    assert int(g_env.car_episode.min()) > 1
    g_env.close()
    e_env.close()


def test_checkpoint_mid_run_continues_bit_for_bit():
    N = 64
    a = _rand_env(N, 13, max_cte=0.012)
    a.reset(seed=2)
    rng = np.random.default_rng(6)
    for t in range(20):
        a.step({"car_control": np.stack([rng.uniform(0.5, 1, N), rng.uniform(-1, 1, N)], axis=1),
                "maneuver": rng.integers(0, 4, N).astype(np.int32)})
    sd = a.state_dict()
    assert sd["car_per_env"]["randomization"]["mask"] == 0xFF
    b = make_env(N, autoreset=True, spawn="host")
    from tinycarlo_amd import terms as T
    b.set_terms([T.cte_termination(0.012, 1)])
    b.load_state_dict(sd)
    for t in range(64):
        act = {"car_control": np.stack([rng.uniform(0.5, 1, N), rng.uniform(-1, 1, N)], axis=1),
               "maneuver": rng.integers(0, 4, N).astype(np.int32)}
        a.step(act)
        b.step(act)
        a.top_up_spawn_queue()
        b.top_up_spawn_queue()
    _same(a, b, "after 64 steps")
    assert torch.equal(a.env_car_params, b.env_car_params)
    assert torch.equal(a.car_episode, b.car_episode)
    assert int(a.car_episode.max()) > 1
    a.close()
    b.close()


def test_shards_draw_the_rows_of_one_batch():
    seed = 21
    whole = _rand_env(64, seed, max_cte=0.012)
    parts = [_rand_env(32, seed, env_offset=32 * s, max_cte=0.012) for s in range(2)]
    whole.reset(seed=100)
    for s, e in enumerate(parts):
        e.reset(seed=100 + 32 * s)
    rng = np.random.default_rng(7)
    for t in range(30):
        cc = np.stack([rng.uniform(0.5, 1, 64), rng.uniform(-1, 1, 64)], axis=1)
        man = rng.integers(0, 4, 64).astype(np.int32)
        whole.step({"car_control": cc, "maneuver": man})
        for s, e in enumerate(parts):
            e.step({"car_control": cc[32 * s:32 * s + 32], "maneuver": man[32 * s:32 * s + 32]})
    torch.cuda.synchronize()
    assert torch.equal(whole.env_car_params, torch.cat([e.env_car_params for e in parts]))
    assert torch.equal(whole.car_episode, torch.cat([e.car_episode for e in parts]))
    assert torch.equal(whole.state["x"], torch.cat([e.state["x"] for e in parts]))
    assert int(whole.car_episode.max()) > 1
    for e in [whole] + parts:
        e.close()


def test_live_shared_car_constants():
    from tinycarlo_amd import gym
    env = gym.make("tinycarlo-v2", config=cfg_for())
    u = env.unwrapped
    u.car.max_velocity = 0.05
    assert u.car.max_velocity == 0.05 and u.vec.car_params.max_velocity == 0.05
    o = orc.Oracle(u.map, u.vec.car_params, u.camera, orc.FMT_CLASSES, 1)
    env.reset(seed=4)
    o.reset(u.vec._keep[0].cpu().numpy())
    for t in range(12):
        env.step({"car_control": [1.0, 0.3], "maneuver": 0})
        o.step(np.array([[1.0, 0.3]]), np.array([0], dtype=np.int32))
        assert bits(u.car.velocity) == bits(o.state["velocity"][0]), t
        assert bits(u.car.position[0]) == bits(o.state["x"][0]), t
    assert u.car.velocity <= 0.05
    u.vec.set_env_cars(wheelbase=0.05)
    with pytest.raises(RuntimeError, match="set_env_cars"):
        u.car.max_velocity = 0.1
    assert torch.equal(u.car.wheelbase.cpu(), torch.tensor([0.05], dtype=torch.float64))
    u.vec.set_env_cars()
    u.car.max_velocity = 0.1
    assert u.car.max_velocity == 0.1
    env.close()


def test_stanley_example_with_randomized_cars():
    """examples/stanley_batched.py --randomize: device spawn, per-episode cars, per-env steering normalisation"""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "stanley_batched.py")
    spec = importlib.util.spec_from_file_location("stanley_batched", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.run(num_envs=256, steps=60, randomize=True)
    assert out["car_episodes_drawn"] > 256 and out["episodes_ended"] > 0
