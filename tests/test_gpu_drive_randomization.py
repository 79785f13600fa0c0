"""Drive randomisation (randomize_drive: per-episode maneuvers, Ornstein-Uhlenbeck steering noise), bit-exact against the
existing single-step path.

The method of test_gpu_controller.py: the reference is never the code under test.  A second env with the same seeds and
settings -- no controller, no randomisation -- runs single `step_device` calls, and before each the HOST forms the action:
the Stanley command through tinycarlo_amd/csrc/tc_ctrl.h and the OU value through tinycarlo_amd/csrc/tc_rng.h, both built by
the host compiler, the maneuver through `randomization.draw_maneuver`, the re-spawns read from `needs_reset`.
Shapes: simple_layout, 64x64 classes, N = 37 (no multiple of 8 or 32), K = 24, device spawns, time limit 7 with staggered
starts.  Run on the MI355X box with `pytest -m gpu`.

Where the feature mask has no episode bit (masks 4 and 5) there is no time limit, so the re-spawns come from a source that
needs none: the CTE termination wrapper with a threshold of 1e-6 m and three steps (any driven car is further from the lane
centre than that), its per-env counters staggered over the envs -- episodes of four steps, five or six re-spawns per env in
the call.  Every reference, whatever its mask, is asked for the same conditions before anything is compared with it.
The "a forced maneuver changes the reference" condition is shown once, for the main setting (mask 7, draw mode): every other
case runs on the same map with episodes no longer than its seven steps plus the spawn step, and draws from the same
candidates, so junctions are reached there as they are here."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, load_cfg
from tinycarlo_amd import randomization as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K = 37, 24
GAIN, SPEED, LIMIT, SEED, DSEED = 4.0, 0.4, 7, 2, 77
CAND = (0, 1, 3)
NOLIMIT_STEPS = 3  # masks without the episode bit: action steps per episode, by the CTE termination
# sigma: the issue starts from train_stanley_il.py's 0.4 and lowers it until a quarter of the action rows apply an
# unclipped steering; 0.4 meets it on this set-up (asserted on the reference below), so 0.4 it is
OU = dict(theta=0.1, mu=0.0, sigma=0.4, reset=True)
OUT_KEYS = ("cte", "heading_error", "reward", "terminated", "truncated", "status", "laneline_distances", "nearest_edge")
EP_KEYS = ("length", "ret", "count", "last_length", "last_return", "length_sum", "return_sum")

SHIM = r"""
#include "tc_ctrl.h"
#include "tc_rng.h"
extern "C" void stanley_n(int n, const double* cte, const double* he, double k, double speed, const double* msa, double* out) {
  for (int i = 0; i < n; i++) out[i] = tc_ctrl_stanley(cte[i], he[i], k, speed, msa[i]);
}
extern "C" double normal_at(unsigned long long seed, unsigned int env, unsigned int draw) { return tc_normal_at(seed, env, draw); }
extern "C" double ou_step(double n, double eps, double theta, double mu, double sigma) { return tc_ou_step(n, eps, theta, mu, sigma); }
"""


_HOST = []


@pytest.fixture(scope="module", autouse=True)
def host_shim(tmp_path_factory):
    """tc_ctrl.h and tc_rng.h built by the host compiler, for host()"""
    d = tmp_path_factory.mktemp("tc_drive_gpu")
    src, lib = str(d / "shim.cpp"), str(d / "libtc_drive.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["c++", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"), "-o", lib, src])
    L = C.CDLL(lib)
    dp = C.POINTER(C.c_double)
    L.stanley_n.argtypes = [C.c_int, dp, dp, C.c_double, C.c_double, dp, dp]
    L.stanley_n.restype = None
    L.normal_at.restype = L.ou_step.restype = C.c_double
    L.normal_at.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    L.ou_step.argtypes = [C.c_double] * 5

    def stanley(cte, he, k, speed, msa):
        cte, he, msa = (np.ascontiguousarray(a, dtype=np.float64) for a in (cte, he, msa))
        out = np.empty_like(cte)
        L.stanley_n(len(cte), cte.ctypes.data_as(dp), he.ctypes.data_as(dp), k, speed, msa.ctypes.data_as(dp), out.ctypes.data_as(dp))
        return out
    _HOST[:] = [(stanley, L.normal_at, L.ou_step)]
    yield
    _HOST.clear()


def host():
    return _HOST[0]


def cfg_for(map_name="simple_layout"):
    cfg, path = load_cfg(map_name)
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = [64, 64]
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


def make_env(cars=True, limit=LIMIT, map_name="simple_layout"):
    """device spawns, the three fused wrappers; per-episode cars (mask bit 1) and the time limit with staggered starts (bit 2).
    Without the limit the CTE termination ends every episode after three action steps (see the module docstring)."""
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    from tinycarlo_amd.wrapper import CrashTerminationWrapper, CTESparseRewardWrapper, CTETerminationWrapper
    vec = TinyCarloVecEnv(cfg_for(map_name), num_envs=N, device="cuda:0", autoreset=True, spawn="device")
    if cars:
        p = vec.car_params
        vec.randomize_cars({"max_steering_angle": (0.4 * p.max_steering_angle, 1.2 * p.max_steering_angle),
                            "steering_shift": (-0.01, 0.0)}, seed=SEED)
    cte_term = (0.07, 5) if limit else (1e-6, NOLIMIT_STEPS)
    env = CrashTerminationWrapper(CTETerminationWrapper(CTESparseRewardWrapper(vec, 0.01), cte_term[0], number_of_steps=cte_term[1]))
    if limit:
        vec.set_time_limit(limit)
    env.reset(seed=SEED)
    if limit:
        vec.episode_stats["length"].copy_((torch.arange(N, device="cuda:0") * limit // N).to(torch.int32))
    else:  # staggered: the CTE termination is the second fused term (counter column 1)
        vec.term_counters[:, 1] = (torch.arange(N, device="cuda:0") % NOLIMIT_STEPS).to(torch.int32)
    return vec


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


class HostDrive:
    """the caller's four arrays and the settings, advanced on the host exactly as the header says"""

    def __init__(self, cand=CAND, mode="draw", ou=OU, seed=DSEED, env_offset=0):
        self.cand, self.mode, self.ou, self.seed, self.off = tuple(cand or ()), mode, dict(ou) if ou else None, seed, env_offset
        self.man = np.zeros(N, dtype=np.int32)
        self.episode = np.zeros(N, dtype=np.int32)
        self.state = np.zeros(N, dtype=np.float64)
        self.draws = np.zeros(N, dtype=np.int32)

    def respawn(self, sel):
        for i in np.flatnonzero(sel):
            if self.cand:
                self.man[i] = int(R.draw_maneuver(self.seed, (self.off + int(i)) & 0xFFFFFFFF, int(self.episode[i]), self.cand, self.mode))
                self.episode[i] += 1
            if self.ou and self.ou["reset"]:
                self.state[i] = 0.0

    def act(self, sel):
        """the OU values of the envs that apply an action (0.0 elsewhere)"""
        _, normal_at, ou_step = host()
        n = np.zeros(N, dtype=np.float64)
        if self.ou:
            for i in np.flatnonzero(sel):
                eps = normal_at(self.seed, (self.off + int(i)) & 0xFFFFFFFF, int(self.draws[i]))
                self.draws[i] += 1
                self.state[i] = ou_step(self.state[i], eps, self.ou["theta"], self.ou["mu"], self.ou["sigma"])
                n[i] = self.state[i]
        return n

    def live(self):
        d = {}
        if self.cand:
            d.update(episode_maneuver=self.man.copy(), drive_episode=self.episode.copy())
        if self.ou:
            d.update(ou_state=self.state.copy(), ou_draws=self.draws.copy())
        return d


def reference_loop(vec, hd, steps, man=None, noise=None, force=None, on_step=None):
    """`steps` single steps of `vec` with the action formed on the host; man [steps, N]: the call's maneuver rows (used while hd
    has no candidates); noise: the controller's own noise rows; force: every maneuver replaced by this value (the vacuity
    re-run).  Returns the per-step rows (rollout key -> [steps, N, ..]) and the re-spawn mask."""
    stanley = host()[0]
    rows = {k: [] for k in OUT_KEYS + ("obs", "x", "y", "theta", "velocity", "local_path", "lp_len", "episode_length",
                                       "episode_return", "steer", "maneuver", "steer_noise", "applied")}
    fresh = []
    for k in range(steps):
        cte, he = vec.out["cte"].cpu().numpy(), vec.out["heading_error"].cpu().numpy()
        msa = (vec.env_car_params[:, 3].cpu().numpy() if vec.env_car_params is not None
               else np.full(N, vec.car_params.max_steering_angle))
        nr = vec._aux["needs_reset"].cpu().numpy().astype(bool)
        hd.respawn(nr)
        cmd = stanley(cte, he, GAIN, SPEED, msa)
        n = hd.act(~nr)
        act = cmd + noise[k] if noise is not None else cmd
        act = act + n if hd.ou else act  # (steer + row) + n
        mk = hd.man.copy() if hd.cand else man[k].copy()
        if force is not None:
            mk[:] = force
        cc = np.stack([np.full(N, SPEED), act], axis=1)
        vec.step_device(torch.from_numpy(cc).cuda(), torch.from_numpy(mk).cuda())
        torch.cuda.synchronize()
        fresh.append(nr)
        rows["steer"].append(np.where(nr, 0.0, cmd))
        rows["maneuver"].append(mk)
        rows["steer_noise"].append(np.where(nr, 0.0, n))
        rows["applied"].append(act)
        for key in OUT_KEYS + ("obs",):
            rows[key].append(vec.out[key].cpu().numpy().copy())
        for key in ("x", "y", "theta", "velocity", "local_path", "lp_len"):
            rows[key].append(vec.state[key].cpu().numpy().copy())
        if vec.episode_stats is not None:
            rows["episode_length"].append(vec.episode_stats["length"].cpu().numpy().copy())
            rows["episode_return"].append(vec.episode_stats["ret"].cpu().numpy().copy())
        if on_step:
            on_step(k, hd, rows)
    return {k: np.stack(v) for k, v in rows.items() if v}, np.stack(fresh)


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


def vacuity(rows, fresh, hd, label):
    """the run covers what it is meant to cover (else every comparison could pass vacuously)"""
    action = ~fresh
    if hd.ou:
        assert (rows["steer_noise"][action] != 0.0).all(), (label, "an action row without noise")
        assert (np.abs(rows["applied"][action]) < 1).mean() >= 0.25, (label, "the noise is (nearly) all clipped away")
    assert (fresh.sum(0) >= 2).all(), (label, "an env that did not re-spawn twice inside the call", fresh.sum(0))
    assert len(set(fresh.argmax(0).tolist())) > 1, (label, "every env re-spawns on the same step")
    if hd.cand:
        varied = sum(len(set(rows["maneuver"][:, i].tolist())) >= 2 for i in range(N))
        assert varied > N // 2, (label, "too few envs see two maneuvers", varied)


@functools.lru_cache(maxsize=None)
def ref(mask=7, mode="draw", reset=True, cand=CAND, with_rows=False, ou_on=True, sigma=OU["sigma"], env_offset=0):
    """the reference loop of one setting, run once and shared (read only)"""
    cars, limit = bool(mask & 1), LIMIT if mask & 2 else 0
    rng = np.random.default_rng(11)
    man = rng.integers(0, 4, (K, N)).astype(np.int32)
    g = torch.Generator().manual_seed(11)
    noise = (0.1 * torch.randn((K, N), generator=g, dtype=torch.float64)).numpy() if with_rows else None
    hd = HostDrive(cand=cand, mode=mode, ou=dict(OU, reset=reset, sigma=sigma) if ou_on else None, env_offset=env_offset)
    vec = make_env(cars=cars, limit=limit)
    rows, fresh = reference_loop(vec, hd, K, man=man, noise=noise)
    fin = final_of(vec)
    vec.close()
    vacuity(rows, fresh, hd, ("ref", mask, mode, reset, env_offset))
    return {"rows": rows, "fresh": fresh, "final": fin, "live": hd.live(), "man": man, "noise": noise, "hd": hd, "mask": mask}


def drive_env(mask=7, mode="draw", reset=True, cand=CAND, ou_on=True, sigma=OU["sigma"], env_offset=0):
    vec = make_env(cars=bool(mask & 1), limit=LIMIT if mask & 2 else 0)
    vec.set_controller(k=GAIN, speed=SPEED)
    vec.randomize_drive(maneuvers=cand, mode=mode, ou=dict(OU, reset=reset, sigma=sigma) if ou_on else None, seed=DSEED,
                        env_offset=env_offset)
    return vec


def assert_rows(roll, r, label, lo=0, hi=None):
    torch.cuda.synchronize()
    for k, t in roll.items():
        want = r["rows"][k][lo:hi]
        got = t.cpu().numpy()
        assert np.array_equal(bits(got), bits(want.reshape(got.shape))), (label, k)


def assert_final(vec, r, label):
    got = final_of(vec)
    assert set(got) == set(r["final"]), label
    for k, v in r["final"].items():
        assert np.array_equal(bits(got[k]), bits(v)), (label, k)
    for k, v in r["live"].items():
        assert np.array_equal(bits(getattr(vec, k)), bits(v)), (label, k)


def test_maneuvers_matter_to_the_reference():
    """vacuity of everything below: the reference of the main setting, run again with every maneuver forced to the first
    candidate, ends up somewhere else -- on simple_layout, with the seven-step episodes of the other cases"""
    r = ref()
    hd = HostDrive()
    vec = make_env()
    rows, _ = reference_loop(vec, hd, K, force=CAND[0])
    vec.close()
    assert any(not np.array_equal(bits(rows[k]), bits(r["rows"][k])) for k in ("x", "y", "theta", "local_path")), \
        "seven-step episodes on simple_layout never reach a junction: the maneuver changes nothing"


@pytest.mark.parametrize("mask", [4, 5, 6, 7])
@pytest.mark.parametrize("family", ["streamed", "no_observation", "drive_step"])
def test_drive_with_both_parts_equals_the_host_loop(family, mask):
    """case 1: draw mode and OU with reset through each kernel family, per-episode cars on / off x episodes on / off"""
    r = ref(mask=mask)
    vec = drive_env(mask=mask)
    label = (family, mask)
    if family == "drive_step":
        assert vec.launch_info(1)["kernel"] == "tc_drive_step_kernel"
        for k in range(K):
            vec.drive_step()
            torch.cuda.synchronize()
            for key in OUT_KEYS + ("obs",):
                assert np.array_equal(bits(vec.out[key]), bits(r["rows"][key][k])), (label, k, key)
            assert np.array_equal(bits(vec.steer_last), bits(r["rows"]["steer"][k])), (label, k, "steer_last")
            assert np.array_equal(bits(vec.episode_maneuver), bits(r["rows"]["maneuver"][k])), (label, k, "maneuver")
            act = ~r["fresh"][k]
            assert np.array_equal(bits(vec.ou_state)[act], bits(r["rows"]["steer_noise"][k])[act]), (label, k, "ou_state")
        assert_final(vec, r, label)
        vec.close()
        return
    if family == "no_observation":
        vec.no_observation = True
        assert vec.launch_info(K)["kernel"] == "tc_drive_env_kernel"
        keys = tuple(k for k in vec.alloc_rollout(1, keys="all") if k != "obs")
        roll = vec.alloc_rollout(K, keys=keys)
    else:
        assert vec.launch_info(K)["kernel"] == "tc_drive_envg_kernel+tc_frame_kernel"
        roll = vec.alloc_rollout(K, keys="all")
        assert "obs" in roll
    assert {"steer", "maneuver", "steer_noise"} <= set(roll) and ("episode_length" in roll) == bool(mask & 2)
    vec.drive(None, rollout=roll)
    assert_rows(roll, r, label)
    assert_final(vec, r, label)
    if "obs" in roll:
        assert int(roll["obs"].max()) == 255
    vec.close()


@pytest.mark.parametrize("family", ["streamed", "no_observation"])
def test_ou_without_reset_cycle_mode_and_caller_noise_rows(family):
    """case 2: the OU value carried across episodes, maneuvers in cycle mode, and the controller's own steer_noise rows
    beside the OU noise: (steer + row) + n"""
    r = ref(mode="cycle", reset=False, with_rows=True)
    # (carried across the re-spawns: the OU rows depend on nothing but the draws and the resets, and differ from the main run's)
    assert r["noise"] is not None and not np.array_equal(r["rows"]["steer_noise"], ref()["rows"]["steer_noise"])
    assert (r["rows"]["maneuver"][r["fresh"]][:, None] == np.array(CAND)[None, :]).any(1).all()
    vec = drive_env(mode="cycle", reset=False)
    if family == "no_observation":
        vec.no_observation = True
        assert vec.launch_info(K)["kernel"] == "tc_drive_env_kernel"
    roll = vec.alloc_rollout(K, keys=("reward", "cte", "x", "y", "theta", "steer", "maneuver", "steer_noise", "episode_length") +
                             (() if family == "no_observation" else ("obs",)))
    vec.drive(None, rollout=roll, steer_noise=torch.from_numpy(r["noise"]).cuda())
    assert_rows(roll, r, ("case 2", family))
    assert_final(vec, r, ("case 2", family))
    vec.close()


def test_ou_alone_takes_the_calls_maneuver_rows():
    """OU noise without candidates: the call's own maneuver rows are used, and come back in the "maneuver" rows"""
    r = ref(cand=None)
    vec = drive_env(cand=None)
    assert vec.episode_maneuver is None and vec.ou_state is not None
    with pytest.raises(ValueError):
        vec.drive(None, n_steps=K)
    roll = vec.alloc_rollout(K, keys="all")
    vec.drive(torch.from_numpy(r["man"]).cuda(), rollout=roll)
    assert np.array_equal(roll["maneuver"].cpu().numpy(), r["man"])
    assert_rows(roll, r, "ou alone")
    assert_final(vec, r, "ou alone")
    vec.close()


@pytest.mark.parametrize("mask", [5, 7])
@pytest.mark.parametrize("family", ["streamed", "no_observation", "drive_step"])
def test_env_offset_shifts_the_streams(family, mask):
    """a shard of a larger population: env i draws what env env_offset + i of one batch would (maneuvers and normals), in
    the grouped kernel and in sim_body; offsets whose sum with i crosses 2^32 - 1 wrap as uint32"""
    off = 2 ** 32 - 20 if mask == 5 else 1000003
    r = ref(mask=mask, env_offset=off)
    assert not np.array_equal(r["rows"]["steer_noise"], ref(mask=mask)["rows"]["steer_noise"])
    assert not np.array_equal(r["rows"]["maneuver"], ref(mask=mask)["rows"]["maneuver"])
    vec = drive_env(mask=mask, env_offset=off)
    if family == "drive_step":
        for k in range(K):
            vec.drive_step()
        assert np.array_equal(bits(vec.out["cte"]), bits(r["rows"]["cte"][-1]))
    else:
        vec.no_observation = family == "no_observation"
        roll = vec.alloc_rollout(K, keys=("x", "y", "theta", "cte", "steer", "maneuver", "steer_noise"))
        vec.drive(None, rollout=roll)
        assert_rows(roll, r, ("env_offset", family, mask))
    assert_final(vec, r, ("env_offset", family, mask))
    with pytest.raises(ValueError):
        vec.randomize_drive(maneuvers=CAND, env_offset=2 ** 32)
    with pytest.raises(ValueError):
        vec.randomize_drive(maneuvers=CAND, env_offset=-1)
    vec.close()


@pytest.mark.parametrize("family", ["streamed", "no_observation"])
def test_split_independence(family):
    """case 3: calls of 5 + 19 steps equal the one call of 24 and the 24 single steps (both are the reference's rows)"""
    r = ref()
    vec = drive_env()
    vec.no_observation = family == "no_observation"
    keys = ("reward", "terminated", "truncated", "cte", "x", "y", "theta", "steer", "maneuver", "steer_noise", "episode_length",
            "episode_return") + (() if vec.no_observation else ("obs",))
    lo = 0
    for n in (5, 19):
        roll = vec.alloc_rollout(n, keys=keys)
        vec.drive(None, rollout=roll)
        assert_rows(roll, r, ("split", family, n), lo, lo + n)
        lo += n
    assert_final(vec, r, ("split", family))
    vec.close()


def test_reset_with_a_mask_draws_for_the_selected_envs_only():
    """case 4: tc_reset of some envs: those draw a maneuver, zero their OU value and advance their counter; the others and
    every draw counter stay"""
    vec = drive_env()
    vec.drive(None, n_steps=5)
    torch.cuda.synchronize()
    vec.ou_state.copy_(torch.linspace(0.5, 1.5, N, dtype=torch.float64))  # (an ordinary tensor: writing is allowed)
    man0, ep0 = vec.episode_maneuver.cpu().numpy().copy(), vec.drive_episode.cpu().numpy().copy()
    ou0, dr0 = vec.ou_state.cpu().numpy().copy(), vec.ou_draws.cpu().numpy().copy()
    sel = (np.arange(N) % 3 == 1)
    vec.reset_to(np.asarray(vec.draw_spawn_nodes(), dtype=np.int32), mask=sel)
    torch.cuda.synchronize()
    want = np.where(sel, R.draw_maneuver(DSEED, np.arange(N), ep0, CAND, "draw"), man0)
    assert (want != man0).any(), "the masked reset changes no maneuver"
    assert np.array_equal(vec.episode_maneuver.cpu().numpy(), want)
    assert np.array_equal(vec.drive_episode.cpu().numpy(), ep0 + sel)
    assert np.array_equal(bits(vec.ou_state), bits(np.where(sel, 0.0, ou0)))
    assert np.array_equal(vec.ou_draws.cpu().numpy(), dr0) and (dr0 > 0).all()
    vec.close()


def test_graph_captured_drive_sees_a_new_sigma():
    """case 5: a prepare_drive call captured into a HIP graph and replayed after set_ou(sigma=...): equals the host loop run
    with the sigma each call had, without re-capture"""
    Kg, s2 = 8, 0.15
    hd = HostDrive()
    twin = make_env()
    parts = []
    for i in range(3):
        hd.ou["sigma"] = OU["sigma"] if i == 0 else s2
        rows, fresh = reference_loop(twin, hd, Kg)
        assert fresh.any(0).all() and (rows["steer_noise"][~fresh] != 0).all(), ("graph reference", i)  # (Kg > LIMIT)
        parts.append(rows)
    want = {"final": final_of(twin), "live": hd.live()}
    twin.close()
    g_env = drive_env()
    roll = g_env.alloc_rollout(Kg, keys="all")
    pc = g_env.prepare_drive(None, roll)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on a side stream, as torch recommends
        pc()
    torch.cuda.current_stream().wait_stream(s)
    assert_rows(roll, {"rows": parts[0]}, ("graph call", 0))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc()
    torch.cuda.synchronize()
    g_env.set_ou(sigma=s2)  # in place: no re-capture
    for i in (1, 2):
        g.replay()
        assert_rows(roll, {"rows": parts[i]}, ("graph call", i))
    assert_final(g_env, want, "graph final")
    assert not np.array_equal(parts[1]["steer_noise"], parts[0]["steer_noise"])
    g_env.close()


def test_off_means_off():
    """case 6: after randomize_drive() the results equal a run that never switched it on; with the feature on but sigma = 0,
    mu = 0 and the call's maneuver as the single candidate they equal the plain drive()"""
    man = torch.full((K, N), 3, dtype=torch.int32, device="cuda:0")
    plain = make_env()
    plain.set_controller(k=GAIN, speed=SPEED)
    rp = plain.alloc_rollout(K, keys="all")
    plain.drive(man, rollout=rp)
    fp = final_of(plain)
    plain.close()
    assert "maneuver" not in rp and (rp["steer"].abs() > 1e-3).any()

    off = drive_env()
    off.randomize_drive()
    assert off.episode_maneuver is None and off.ou_state is None
    with pytest.raises(ValueError):
        off.drive(None, n_steps=K)
    with pytest.raises(ValueError):
        off.alloc_rollout(K, keys=("maneuver",))
    ro = off.alloc_rollout(K, keys="all")
    off.drive(man, rollout=ro)
    zero = drive_env(cand=(3,), sigma=0.0)
    zero.episode_maneuver.fill_(3)  # (the episodes under way when the feature came on: theirs is the caller's to set)
    rz = zero.alloc_rollout(K, keys="all")
    zero.drive(None, rollout=rz)
    torch.cuda.synchronize()
    assert set(ro) == set(rp)
    for name, vec, roll in (("off again", off, ro), ("zero noise", zero, rz)):
        for k in rp:
            assert np.array_equal(bits(roll[k]), bits(rp[k])), (name, k)
        got = final_of(vec)
        for k, v in fp.items():
            assert np.array_equal(bits(got[k]), bits(v)), (name, k)
    assert (rz["maneuver"] == 3).all() and (rz["steer_noise"] == 0).all() and int(zero.ou_draws.min()) > 0
    # set_controller(None) drops the randomisation too
    zero.set_controller(None)
    assert zero._drive is None and zero.launch_info(K)["kernel"].startswith("tc_envg_kernel")
    off.close()
    zero.close()


def test_state_dict_carries_settings_and_live_tensors():
    r = ref()
    a = drive_env()
    a.drive(None, n_steps=5)
    sd = a.state_dict()
    assert sd["drive_randomization"]["maneuvers"] == CAND and sd["drive_randomization"]["ou"]["sigma"] == OU["sigma"]
    b = make_env()
    b.load_state_dict(sd)
    roll = b.alloc_rollout(19, keys=("x", "y", "steer", "maneuver", "steer_noise"))
    b.drive(None, rollout=roll)
    assert_rows(roll, r, "state_dict", 5, 24)
    assert_final(b, r, "state_dict")
    a.close()
    b.close()


def test_refusals_with_a_handle():
    """what only a real handle can refuse: no controller installed, and a call longer than the rows it was given"""
    from tinycarlo_amd import _native as nat
    L = nat.lib()
    vec = make_env()
    man_t, ep_t, dr_t = (torch.zeros(N, dtype=torch.int32, device="cuda:0") for _ in range(3))
    ou = torch.zeros(N, dtype=torch.float64, device="cuda:0")
    rows = torch.zeros((4, N), dtype=torch.int32, device="cuda:0")
    nrows = torch.zeros((4, N), dtype=torch.float64, device="cuda:0")

    def drv(**kw):
        c = nat.DriveRandomizationC()
        c.n_maneuvers, c.maneuver_mode = 1, nat.MAN_DRAW
        c.maneuvers[0] = 3
        c.theta, c.mu, c.sigma = 0.1, 0.0, 0.4
        c.maneuver, c.episode, c.ou_state, c.ou_draws = man_t.data_ptr(), ep_t.data_ptr(), ou.data_ptr(), dr_t.data_ptr()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    def multi(n_steps, **kw):  # tc_step_multi with the feature rows kw
        sr = nat.StepRows(**kw)
        return L.tc_step_multi(vec._h, None, nat.F64, None, n_steps, flags, None, C.byref(sr), vec._stream())
    assert L.tc_env_set_drive_randomization(vec._h, C.byref(drv())) == -1 and b"controller" in L.tc_last_error()
    with pytest.raises(ValueError):
        vec.randomize_drive(maneuvers=CAND)
    vec.set_controller(k=GAIN, speed=SPEED)
    flags = vec._flags() | nat.F_NO_OBSERVATION
    # rows for a feature that is off: a controller but no drive randomisation
    for kw in ({"maneuver_out": rows.data_ptr()}, {"ou_noise_out": nrows.data_ptr()}):
        sr = nat.StepRows(n_rows=4, **kw)
        man4 = torch.zeros((4, N), dtype=torch.int32, device="cuda:0")
        assert L.tc_step_multi(vec._h, None, nat.F64, man4.data_ptr(), 4, flags, None, C.byref(sr), vec._stream()) == -1
        assert b"rows without drive randomisation" in L.tc_last_error()
    assert L.tc_env_set_drive_randomization(vec._h, C.byref(drv(maneuver_mode=7))) == -1
    assert vec.launch_info(1)["kernel"] == "tc_drive_step_kernel"
    assert L.tc_env_set_drive_randomization(vec._h, C.byref(drv())) == 0
    for kw in ({"maneuver_out": rows.data_ptr()}, {"ou_noise_out": nrows.data_ptr()}):
        assert multi(5, n_rows=4, **kw) == -1 and b"rows" in L.tc_last_error()  # a K-step call longer than n_rows
        assert multi(4, n_rows=-1, **kw) == -1 and b"negative" in L.tc_last_error()
        assert multi(4, n_rows=0, **kw) == -1 and b"n_rows = 0" in L.tc_last_error()
        assert multi(4, n_rows=4, **kw) == 0
    assert multi(5) == 0  # no rows: any length, and no maneuver argument
    assert L.tc_step_multi(vec._h, None, nat.F64, None, 5, flags, None, None, vec._stream()) == 0
    assert L.tc_step(vec._h, None, nat.F64, None, flags, vec._stream()) == 0
    torch.cuda.synchronize()
    # (the envs under way keep maneuver 0 until they re-spawn, then take the one candidate; some action row carries noise)
    assert set(rows.cpu().numpy().reshape(-1).tolist()) == {0, 3} and (nrows.cpu().numpy() != 0).any()
    assert int(dr_t.min()) > 0 and int(ep_t.max()) > 0
    # OU alone: the maneuver argument is required again
    assert L.tc_env_set_drive_randomization(vec._h, C.byref(drv(n_maneuvers=0))) == 0
    assert L.tc_step_multi(vec._h, None, nat.F64, None, 5, flags, None, None, vec._stream()) == -1
    # a struct with neither part is "off": the maneuver argument is required, as after NULL
    assert L.tc_env_set_drive_randomization(vec._h, C.byref(drv())) == 0
    assert L.tc_env_set_drive_randomization(vec._h, C.byref(drv(n_maneuvers=0, ou_state=None))) == 0
    assert L.tc_step(vec._h, None, nat.F64, None, flags, vec._stream()) == -1
    assert L.tc_env_set_drive_randomization(vec._h, C.byref(drv())) == 0
    assert L.tc_env_set_drive_randomization(vec._h, None) == 0
    assert L.tc_step(vec._h, None, nat.F64, None, flags, vec._stream()) == -1
    torch.cuda.synchronize()
    vec.close()
