"""A composed CPU reference for the simulate kernels' feature masks (per-env cars, episodes, built-in controller).

`FeatureRef` is N single-env `orc.Oracle` objects (portable math) with up to three layers on top, each switched on
independently, each restating one feature of the HIP library on the host:

  cars        per-env car rows drawn with `randomization.draw_car_params(seed, env, episode, lo, hi)`: at reset (episode 0)
              and again at every re-spawn; `steering_shift` is added to the steering input before the clip (the oracle clips)
  episodes    rules 1-3 of tc_env_set_episodes (include/tinycarlo_hip.h) in numpy after each step -- `EpisodeRules`: length,
              return, time-limit truncation, TC_S_TIME_LIMIT, the finished-episode sums, the re-spawn request for the next step
  controller  the action of step k from the reference's OWN cte / heading_error of step k-1, through tc_ctrl_stanley of
              tinycarlo_amd/csrc/tc_ctrl.h built by the host compiler (`stanley_lib`), with the env's own max_steering_angle;
              the command is 0.0 on the step that re-spawns the env; the noise row is added afterwards

Fixed settings: one fused term, cte_termination(max_cte, 1), so that envs end for other reasons than the limit; autoreset
with host spawns (every oracle gets its env's spawn queue).  With every layer off it is the plain batched oracle
(tests/test_variant_matrix_cpu.py holds it to that).

`Ref` is the expected run of tests/test_gpu_episodes.py (an OracleVecEnv plus the same `EpisodeRules`).

The second half describes the cases of the kernel-variant matrix (tests/test_gpu_variant_matrix.py): map, settings and
inputs per (kcode, thick, fmt, feat), the reference run of a case, and the conditions under which a case tests something.
Test infrastructure only: no GPU code, and no answer comes from the library under test."""
import atexit
import copy
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile
import zlib

import numpy as np

import big_maps as bm
import orc
from common import ROOT

STATE_F = ("x", "y", "theta", "velocity", "steering", "radius", "front_x", "front_y")
EP_KEYS = ("length", "ret", "count", "last_length", "last_return", "length_sum", "return_sum")
CAR_COLS = ("wheelbase", "track_width", "max_velocity", "max_steering_angle", "steering_speed", "max_acceleration",
            "max_deceleration")
S_NOT_RESET, S_TIME_LIMIT = 8, 32
FEAT_CAR, FEAT_EP, FEAT_CTRL = 1, 2, 4  # TC_FEAT_* of csrc/k_feat.h

STANLEY_SHIM = r"""
#include "tc_ctrl.h"
extern "C" void stanley_n(int n, const double* cte, const double* he, double k, double speed, const double* msa, double* out) {
  for (int i = 0; i < n; i++) out[i] = tc_ctrl_stanley(cte[i], he[i], k, speed, msa[i]);
}
"""

_stanley = None


def stanley_lib():
    """tc_ctrl_stanley of tc_ctrl.h, built alone by the host compiler (-ffp-contract=off: every operation rounded on its
    own, like the library), once per process -> f(cte[n], he[n], k, speed, msa[n]) -> command[n]"""
    global _stanley
    if _stanley is None:
        d = tempfile.mkdtemp(prefix="tc_ctrl_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src, lib = os.path.join(d, "shim.cpp"), os.path.join(d, "libtc_ctrl.so")
        with open(src, "w") as f:
            f.write(STANLEY_SHIM)
        subprocess.check_call(["c++", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"), "-o", lib, src])
        L = C.CDLL(lib)
        dp = C.POINTER(C.c_double)
        L.stanley_n.argtypes = [C.c_int, dp, dp, C.c_double, C.c_double, dp, dp]
        L.stanley_n.restype = None

        def f(cte, he, k, speed, msa):
            cte, he, msa = (np.ascontiguousarray(a, dtype=np.float64) for a in (cte, he, msa))
            out = np.empty_like(cte)
            L.stanley_n(len(cte), cte.ctypes.data_as(dp), he.ctypes.data_as(dp), float(k), float(speed), msa.ctypes.data_as(dp),
                        out.ctypes.data_as(dp))
            return out
        _stanley = f
    return _stanley


class EpisodeRules:
    """rules 1-3 of tc_env_set_episodes in numpy, applied to one step's outputs after the step"""

    def __init__(self, N, limit, length0=None):
        self.N = N
        self.limit = np.broadcast_to(np.asarray(limit, dtype=np.int64), (N,)).copy()
        self.ep = {"length": np.zeros(N, np.int32), "ret": np.zeros(N, np.float64), "count": np.zeros(N, np.int32),
                   "last_length": np.zeros(N, np.int32), "last_return": np.zeros(N, np.float64),
                   "length_sum": np.zeros(N, np.int64), "return_sum": np.zeros(N, np.float64)}
        if length0 is not None:
            self.ep["length"][:] = length0
        self.respawns = np.zeros(N, np.int64)
        self.by_limit = np.zeros(N, bool)
        self.by_other = np.zeros(N, bool)

    def reset(self, sel):
        self.ep["length"][sel] = 0
        self.ep["ret"][sel] = 0.0

    def step(self, fresh, out):
        """fresh: the envs this step re-spawned; out: the step's status / truncated / reward / terminated arrays --
        truncated and status are replaced by arrays with the time limit in them.  -> the mask of envs truncated by the limit
        (the device re-spawns these on its next step: so must the caller's oracle)"""
        ep = self.ep
        left_alone = (out["status"] & S_NOT_RESET) != 0
        ep["length"][fresh] = 0
        ep["ret"][fresh] = 0.0
        run = ~fresh & ~left_alone
        ep["length"][run] += 1
        tl = run & (self.limit > 0) & (ep["length"] >= self.limit)
        out["truncated"] = out["truncated"] | tl.astype(out["truncated"].dtype)
        out["status"] = out["status"] | (tl.astype(np.int32) * S_TIME_LIMIT)
        for i in np.flatnonzero(run):  # one float64 add per step, in step order
            ep["ret"][i] = ep["ret"][i] + out["reward"][i]
        done = run & ((out["terminated"] | out["truncated"]) != 0)
        ep["last_length"][done] = ep["length"][done]
        ep["last_return"][done] = ep["ret"][done]
        ep["count"][done] += 1
        ep["length_sum"][done] += ep["length"][done]
        for i in np.flatnonzero(done):
            ep["return_sum"][i] = ep["return_sum"][i] + ep["ret"][i]
        self.respawns += fresh
        self.by_limit |= tl
        self.by_other |= done & ~tl
        return tl

    def snapshot(self):
        return {k: v.copy() for k, v in self.ep.items()}


class Ref:
    """the expected run of tests/test_gpu_episodes.py: an oracle env (oracle_backend.OracleVecEnv) plus EpisodeRules"""

    def __init__(self, oenv, limit, length0=None):
        N = oenv.num_envs
        self.o, self.N = oenv, N
        self.rules = r = EpisodeRules(N, limit, length0)
        self.limit, self.ep, self.respawns, self.by_limit, self.by_other = r.limit, r.ep, r.respawns, r.by_limit, r.by_other

    def reset(self, seed, mask=None):
        self.o.reset(seed=seed, mask=mask)
        self.rules.reset(np.ones(self.N, bool) if mask is None else np.asarray(mask).astype(bool))

    def step(self, cc, man):
        import torch
        o = self.o
        fresh = o._aux["needs_reset"].numpy().astype(bool) if o.autoreset else np.zeros(self.N, bool)
        o.step_device(torch.from_numpy(np.ascontiguousarray(cc)), torch.from_numpy(np.ascontiguousarray(man)))
        out = {k: v.numpy().copy() for k, v in o.out.items()}
        tl = self.rules.step(fresh, out)
        o.request_reset(torch.from_numpy(tl))  # the device re-spawns these on its next step: so must the oracle
        out["state"] = {k: v.numpy().copy() for k, v in o.state.items()}
        out["needs_reset"] = o._aux["needs_reset"].numpy().copy()
        out["spawn_cursor"] = o._aux["spawn_cursor"].numpy().copy()
        out["ep"] = self.rules.snapshot()
        return out

    def assert_not_vacuous(self, twice=True):
        assert self.by_limit.any(), "no env was truncated by the limit"
        assert self.by_other.any(), "no env ended by a termination / car truncation before its limit"
        if twice:
            assert self.respawns.max() >= 2, "no env was re-spawned twice"


def params_of_row(p, row):
    import dataclasses
    return dataclasses.replace(p, **{c: float(row[j]) for j, c in enumerate(CAR_COLS)})


class FeatureRef:
    """N single-env oracles and the optional layers (see the head of this file).

    m / car_params / camera: tinycarlo_amd Map / CarParams / Camera; fmt: orc.FMT_*; nodes [N], queue [N, Q]: the spawn nodes
    of the reset and every env's spawn queue; max_cte: of the one fused term.
    cars: None | {"seed", "lo", "hi", "mask"} (randomization.car_ranges); limit: None | [N] per-env time limits (episodes on);
    length0: the staggered starting lengths written after the reset; ctrl: None | {"k", "speed"}.
    reset() and step() return the expected outputs of that call:
      state / info   structured arrays [N] (orc.STATE_DTYPE / orc.INFO_DTYPE; truncated and status with the time limit in them)
      obs [N, bytes], needs_reset, spawn_cursor, fresh (the envs the call re-spawned)
      ep (EP_KEYS -> [N]) | None, car [N, 8] and car_episode [N] | None, steer [N] (before noise) | None"""

    def __init__(self, m, car_params, camera, fmt, nodes, queue, max_cte, cars=None, limit=None, length0=None, ctrl=None):
        from tinycarlo_amd import terms as T
        from tinycarlo_amd.randomization import config_row
        self.N = N = len(nodes)
        self.p, self.C = car_params, len(m.get_laneline_names())
        self.nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        self.cars, self.ctrl = cars, ctrl
        omap = orc.OracleMap(m)
        queue = np.ascontiguousarray(queue, dtype=np.int32)
        self.oracles = []
        for i in range(N):
            o = orc.Oracle(omap, car_params, camera, fmt, 1)
            o.terms = [T.cte_termination(max_cte, 1)]
            o.spawn_queue = queue[i:i + 1].copy()
            self.oracles.append(o)
        self.shared_row = config_row(car_params)
        self.rows = np.tile(self.shared_row, (N, 1)) if cars else None
        self.shift, self.msa = np.zeros(N), np.zeros(N)  # the steering shift and max_steering_angle in force
        self.episode = np.zeros(N, np.int32) if cars else None
        self.rules = EpisodeRules(N, limit) if limit is not None else None
        self.length0 = length0
        self.redrawn = np.zeros(N, np.int64)
        self.last = None

    def _draw(self, i):
        """the row of env i's next episode (the masked columns; the others keep their values), and its episode counter"""
        from tinycarlo_amd.randomization import draw_car_params
        c = self.cars
        self.rows[i] = draw_car_params(c["seed"], i, int(self.episode[i]), c["lo"], c["hi"], c["mask"], base=self.rows[i])
        self.episode[i] += 1
        row = self.rows[i].copy()
        for j in c.get("shared_cols", ()):  # (tests of the tests: these columns act with the shared car's value, shift 0)
            row[j] = self.shared_row[j]
        self.shift[i], self.msa[i] = row[7], row[3]
        self.oracles[i].car = orc.make_car(params_of_row(self.p, row))

    def _collect(self, fresh, steer):
        os_ = self.oracles
        out = {"state": np.concatenate([o.state for o in os_]), "info": np.concatenate([o.info for o in os_]),
               "obs": np.concatenate([o.obs for o in os_]), "fresh": fresh.copy(),
               "spawn_cursor": np.concatenate([o.spawn_cursor for o in os_]), "steer": steer, "ep": None, "car": None,
               "car_episode": None}
        return out

    def _finish(self, out):
        out["needs_reset"] = np.concatenate([o.needs_reset for o in self.oracles])
        if self.rules is not None:
            out["ep"] = self.rules.snapshot()
        if self.cars:
            out["car"], out["car_episode"] = self.rows.copy(), self.episode.copy()
        self.last = out
        return out

    def reset(self):
        for i, o in enumerate(self.oracles):
            if self.cars:
                self._draw(i)
            o.reset(self.nodes[i:i + 1])
        if self.rules is not None:
            self.rules.reset(np.ones(self.N, bool))
            if self.length0 is not None:
                self.rules.ep["length"][:] = self.length0
        return self._finish(self._collect(np.ones(self.N, bool), None))

    def step(self, cc, man, noise=None):
        """cc [N, 2] (ignored with a controller), man [N]; noise [N]: added to the controller's command"""
        N = self.N
        fresh = np.concatenate([o.needs_reset for o in self.oracles]).astype(bool)
        steer = None
        if self.ctrl:
            msa = self.msa if self.cars else np.full(N, self.p.max_steering_angle)
            cmd = stanley_lib()(self.last["info"]["cte"], self.last["info"]["heading_error"], self.ctrl["k"], self.ctrl["speed"], msa)
            act = cmd + noise if noise is not None else cmd
            cc = np.stack([np.full(N, float(self.ctrl["speed"])), act], axis=1)
            steer = np.where(fresh, 0.0, cmd)
        cc = np.ascontiguousarray(cc, dtype=np.float64)
        man = np.ascontiguousarray(man, dtype=np.int32)
        for i, o in enumerate(self.oracles):
            if fresh[i] and self.cars:
                self._draw(i)
                self.redrawn[i] += 1
            ck = cc[i:i + 1].copy()
            if self.cars:
                ck[0, 1] = ck[0, 1] + self.shift[i]  # the shift is added before the clip (the oracle clips)
            o.step(ck, man[i:i + 1], flags=orc.F_AUTORESET)
        out = self._collect(fresh, steer)
        if self.rules is not None:
            inf = out["info"]
            d = {k: inf[k].copy() for k in ("status", "truncated", "reward", "terminated")}
            tl = self.rules.step(fresh, d)
            inf["truncated"], inf["status"] = d["truncated"], d["status"]
            for i in np.flatnonzero(tl):  # the device re-spawns these on its next step
                self.oracles[i].needs_reset[0] = 1
        return self._finish(out)


# ------------------------------------------------------------------------------------------------------------------
# The cases of the kernel-variant matrix: one generated map per K code, the settings of every feature mask, the inputs.
KCODE_CASE = {5: "k5_320_nodes", 8: "k8_512_nodes", 9: "layers_big_component", 516: "components_516_split", 13: "k13_layer_577"}
N_ENVS = 37          # no multiple of the 8 envs per wavefront / the 32 per workgroup of the grouped kernel
RES = [64, 64]
N_SINGLE, N_MULTI = 4, 6
QUEUE_LEN = 8        # spawn queue: more than an env can use up in 10 steps
MAX_CTE = 0.004      # of cte_termination(max_cte, 1): a good part of the envs ends within a few steps of these actions
GAIN, SPEED = 4.0, 0.05  # (a speed within reach of a few steps' acceleration: max_velocity acts)
CAR_SEED = 77
_dir = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="tc_variants_")
        atexit.register(shutil.rmtree, _dir, ignore_errors=True)
    return _dir


def case_cfg(kcode, thick, fmt):
    """config of the K code's map (big_maps.case_config) at 64x64 with the format and line thickness of the matrix cell;
    fmt "bits" is the classes format (the packing is an argument of the env)"""
    name = KCODE_CASE[kcode]
    cfg = bm.case_config(name, 0, os.path.join(_tmp(), f"{name}.json"))
    cfg["sim"]["observation_space_format"] = "rgb" if fmt == "rgb" else "classes"
    cfg["camera"].update(resolution=list(RES), line_thickness=2 if thick else 1)
    return cfg


def case_plan(kcode):
    return bm.case_map(KCODE_CASE[kcode], 0)[1]


def case_seed(kcode):
    return bm.case_seed(KCODE_CASE[kcode], 0)


def car_ranges_of(p):
    """every column drawn, shift included (tests/test_gpu_car_per_env.py: _ranges)"""
    return {"wheelbase": (p.wheelbase * 0.7, p.wheelbase * 1.4), "track_width": (p.track_width * 0.8, p.track_width * 1.5),
            "max_velocity": (p.max_velocity * 0.8, p.max_velocity * 1.6),
            "max_steering_angle": (p.max_steering_angle * 0.6, p.max_steering_angle * 1.2),
            "steering_speed": (p.steering_speed * 0.5, p.steering_speed * 3.0),
            "max_acceleration": (p.max_acceleration * 0.5, p.max_acceleration * 2.0),
            "max_deceleration": (p.max_deceleration * 0.5, p.max_deceleration * 1.5), "steering_shift": (-0.08, 0.08)}


def case_limits(n=N_ENVS):
    """per-env time limits 2 .. 4 and staggered starting lengths (tests/test_gpu_controller.py: make_env), so that some env
    reaches its limit on every step; env 5 has no limit"""
    limit = 2 + np.arange(n) % 3
    length0 = (np.arange(n) * limit // n).astype(np.int32)
    limit[5] = 0
    return limit.astype(np.int64), length0


def case_inputs(kcode, n=N_ENVS, steps=N_SINGLE + N_MULTI):
    """-> car_control [steps, n, 2] f64, maneuver [steps, n] i32, steer noise [steps, n] f64.  An episode here lasts a few
    steps, in which the car gains 0.003 m/s and 1 degree of steering per step at most, so with wild commands alone only the
    two rate limits would ever act.  The commands are therefore a mixture: velocity fast and beyond 1 (max_acceleration
    acts), small (the target is within reach: max_velocity acts) or reverse (max_deceleration); steering wild
    (steering_speed acts) or small (max_steering_angle and the shift act); the controller's noise likewise.
    tests/test_variant_matrix_cpu.py holds every car column to making a difference."""
    rng = np.random.default_rng([zlib.crc32(b"variant-matrix"), int(kcode)])
    shp = (steps, n)
    kind = rng.integers(0, 3, shp)
    v = np.where(kind == 0, rng.uniform(0.6, 1.3, shp), np.where(kind == 1, rng.uniform(0.0, 0.15, shp), rng.uniform(-1.3, -0.05, shp)))
    st = np.where(rng.random(shp) < 0.5, rng.uniform(-1.3, 1.3, shp), rng.uniform(-0.1, 0.1, shp))
    man = rng.integers(0, 4, shp).astype(np.int32)
    noise = np.where(rng.random(shp) < 0.5, 0.5, 0.02) * rng.standard_normal(shp)
    return np.stack([v, st], axis=2), man, noise


@functools.lru_cache(maxsize=None)
def host_spawns(kcode):
    """spawn nodes of reset(seed) and the spawn queue, from the env's host logic alone (OracleVecEnv: no GPU) -- the GPU cases
    hold their env to the same values"""
    from oracle_backend import OracleVecEnv
    oenv = OracleVecEnv(case_cfg(kcode, True, "classes"), num_envs=N_ENVS, autoreset=True, spawn="host", spawn_queue_len=QUEUE_LEN)
    oenv.reset(seed=case_seed(kcode))
    return oenv._keep[0].numpy().copy(), oenv._aux["spawn_queue"].numpy().copy()


def make_reference(kcode, thick, fmt, feat, shared_cols=()):
    """the FeatureRef of a matrix cell (fmt: classes | rgb; packed frames are pack_bits_reference of the classes frames)"""
    from tinycarlo_amd.camera import Camera
    from tinycarlo_amd.config import CarParams
    from tinycarlo_amd.map import Map
    from tinycarlo_amd.randomization import car_ranges
    cfg = case_cfg(kcode, thick, fmt)
    m = Map(cfg["map"])  # (the json_path is absolute)
    p = CarParams.from_config(1 / cfg["sim"].get("fps", 30), cfg["car"])
    cam = Camera(copy.deepcopy(cfg["camera"]))
    nodes, queue = host_spawns(kcode)
    cars = None
    if feat & FEAT_CAR:
        lo, hi, mask = car_ranges(p, car_ranges_of(p))
        cars = {"seed": CAR_SEED, "lo": lo, "hi": hi, "mask": mask, "shared_cols": tuple(shared_cols)}
    limit, length0 = case_limits() if feat & FEAT_EP else (None, None)
    ctrl = {"k": GAIN, "speed": SPEED} if feat & FEAT_CTRL else None
    return FeatureRef(m, p, cam, orc.FMT_RGB if fmt == "rgb" else orc.FMT_CLASSES, nodes, queue, MAX_CTE, cars=cars, limit=limit,
                      length0=length0, ctrl=ctrl)


@functools.lru_cache(maxsize=None)
def reference_run(kcode, thick, fmt, feat, shared_cols=()):
    """the whole run of a cell, computed once and shared (read only): reset, N_SINGLE single steps (no noise: a single step of
    the controller takes none), N_MULTI steps of one call (with the noise rows) -> {"reset": out, "steps": [out] * 10, "ref"}"""
    orc.set_math_mode(orc.MATH_PORTABLE)
    ref = make_reference(kcode, thick, fmt, feat, shared_cols)
    cc, man, noise = case_inputs(kcode)
    run = {"reset": ref.reset(), "steps": [], "ref": ref}
    for t in range(N_SINGLE + N_MULTI):
        run["steps"].append(ref.step(cc[t], man[t], noise[t] if (feat & FEAT_CTRL and t >= N_SINGLE) else None))
    return run


def assert_not_vacuous(run, feat, label=""):
    """the conditions under which a case of the matrix tests what it is named for, on the reference's outputs alone"""
    steps, ref = run["steps"], run["ref"]
    single, multi = steps[:N_SINGLE], steps[N_SINGLE:]
    assert all(s["obs"].any() for s in steps) and run["reset"]["obs"].any(), (label, "a step with every frame empty")
    assert any(s["fresh"].any() for s in single), (label, "no env re-spawned during the single steps")
    assert any(s["fresh"].any() for s in multi[1:]), (label, "no env re-spawned strictly inside the K-step call")
    if feat & FEAT_EP:
        def tl(s):
            return (s["info"]["status"] & S_TIME_LIMIT) != 0
        assert any(tl(s).any() for s in single), (label, "no env truncated by its limit in the single steps")
        assert any(tl(s).any() for s in multi), (label, "no env truncated by its limit inside the K-step call")
        assert ref.rules.by_limit.any() and ref.rules.by_other.any(), (label, "no env ended otherwise than by its limit")
        assert any(((s["info"]["terminated"] != 0) & ~tl(s)).any() for s in steps), label
    else:
        assert not any((s["info"]["status"] & S_TIME_LIMIT).any() for s in steps), label
    if feat & FEAT_CAR:
        car = steps[-1]["car"]
        assert len(np.unique(car, axis=0)) == len(car), (label, "car rows do not differ between envs")
        assert ref.redrawn.sum() >= 1 and int(steps[-1]["car_episode"].max()) >= 2, (label, "no car row was re-drawn")
        assert any(not np.array_equal(a["car"], b["car"]) for a, b in zip(steps, steps[1:])), label
    if feat & FEAT_CTRL:
        for part, name in ((single, "single steps"), (multi, "K-step call")):
            st, fr = np.stack([s["steer"] for s in part]), np.stack([s["fresh"] for s in part])
            live = st[~fr]
            assert (np.abs(live) > 1e-3).any() and len(np.unique(live)) > 2, (label, name, "the controller never steered")
            assert fr.any() and (st[fr] == 0.0).all(), (label, name, "no 0.0 row of a fresh re-spawn")
