"""TinyCarloVecEnv -- N independent tinycarlo envs advancing in lockstep on one MI355X.

Same config schema, action / observation / info semantics as the reference's ``TinyCarloEnv``
(``tinycarlo/env.py:15-147``), batched on a leading ``num_envs`` axis:

* state lives as structure-of-arrays in torch CUDA tensors (``self.state``) that the HIP library
  reads and writes in place through the C ABI (``include/tinycarlo_hip.h``);
* ``step(action)`` enqueues ONE kernel launch (kinematics -> lanepath tracking -> lane-line
  distances -> camera raster) on torch's current stream; observations / rewards / info stay on the
  device unless ``return_numpy=True``;
* spawn nodes are drawn on the host with one ``numpy.random.Generator`` per env, seeded like
  gymnasium seeds ``env.np_random`` (seed + env index), so env ``i`` reproduces the reference env
  reset with ``seed + i``.

No CPU fallback exists: without the compiled library (or a GPU) construction raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as nat
from . import gym
from .config import getenv as gym_getenv
from .camera import Camera
from .config import CarParams, load_config
from .map import Map
from .terms import Term


def _default_device() -> torch.device:
    return torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))


class CarView:
    """``env.unwrapped.car``: the car constants (``car.py:12-19``), live like the reference's ``Car`` attributes, which
    ``Car.step`` reads on every step (``car.py:70-125``).

    Reading a constant gives the shared car's value -- or, while per-env cars are installed (``set_env_cars`` /
    ``randomize_cars``), the env's ``[N]`` column of ``env_car_params`` (a view of the live device rows: the torch-side
    wrappers, ``wrapper/reward.py:20,33``, then broadcast each env's ``track_width``).  Assigning one pushes a new shared
    car to the engine (``tc_env_set_car``) for the steps that follow; with per-env cars installed it raises."""

    CONSTANTS = ("wheelbase", "track_width", "max_velocity", "max_steering_angle", "steering_speed", "max_acceleration",
                 "max_deceleration")

    def __init__(self, p: CarParams, env: Optional["TinyCarloVecEnv"] = None):
        object.__setattr__(self, "_p", p)
        object.__setattr__(self, "_env", env)

    def __getattr__(self, k: str):
        if k.startswith("_"):
            raise AttributeError(k)
        env = self._env
        if env is not None and k in self.CONSTANTS and env._car_rows is not None:
            return env._car_rows[:, nat.CAR_COLUMNS.index(k)]
        p = env.car_params if env is not None else self._p
        return getattr(p, k)

    def __setattr__(self, k: str, v) -> None:
        if k in self.CONSTANTS and self._env is not None:
            self._env._set_shared_car(**{k: v})
        elif k == "T":
            raise AttributeError("car.T is 1 / sim.fps, fixed when the env is created")
        else:
            object.__setattr__(self, k, v)


class LazyInfo(dict):
    """info of a batched step (env.py:83-85): a ``dict`` with the reference's keys.

    The entries the engine writes itself -- ``cte``, ``heading_error``, ``orientation``, ``status`` and the per-layer
    ``laneline_distances`` -- are views of the env's buffers and are in the dict from the start (no device work).
    ``position``, ``local_path``, ``local_path_len`` and ``velocity`` each cost a few small torch kernels and are built
    on first access (``__missing__``); they are listed by ``keys()`` / iteration / ``in`` like the others.  Being a
    real dict it passes gymnasium's ``isinstance(info, dict)`` check and wrappers may add entries.

    Like every tensor the env hands out, the entries show the env's live buffers.  A derived entry that is first read
    AFTER the env has stepped again would silently describe the later step, so that raises instead; ``materialize()``
    returns an independent snapshot (plain dict of clones) for callers that keep infos across steps."""

    DERIVED = ("position", "local_path", "local_path_len", "velocity")
    KEYS = ("cte", "heading_error", "position", "orientation", "laneline_distances", "local_path", "local_path_len",
            "velocity", "status")

    def __init__(self, env):
        st, o = env.state, env.out
        super().__init__(cte=o["cte"], heading_error=o["heading_error"], orientation=st["theta"], status=o["status"],
                         laneline_distances={name: o["laneline_distances"][:, i] for i, name in enumerate(env.layer_names)})
        ep = getattr(env, "_episodes", None)
        if ep is not None:  # track_episodes / set_time_limit: the running episode (views, like the rest)
            dict.__setitem__(self, "episode_length", ep["length"])
            dict.__setitem__(self, "episode_return", ep["ret"])
        self._env = env
        self._serial = env._step_serial
        self._valid = None

    # ---- derived entries
    def _valid_n(self):
        # car.get_info returned real values (car.py:47-51): the local path has its look-ahead edges.  A freshly
        # (re)spawned env has lp_len == 1, and so has one whose tracking stopped early (truncated).  (Not read off
        # nearest_edge[:, 0]: a first lane-line layer without edges would report -1 there for ever.)
        if self._valid is None:
            lp_len = self._env.state["lp_len"]
            valid = lp_len >= 2
            self._valid = (valid, torch.where(valid, lp_len, torch.zeros_like(lp_len)))
        return self._valid

    def __missing__(self, key):
        if key not in self.DERIVED:
            raise KeyError(key)
        e = self._env
        if e._step_serial != self._serial:
            raise RuntimeError(f"info[{key!r}] read after the env stepped again: derived entries are built from the env's "
                               "live buffers; read them before the next step or keep info.materialize()")
        st = e.state
        if key == "position":
            v = torch.stack([st["x"], st["y"]], dim=1)
        elif key == "local_path_len":
            v = self._valid_n()[1]
        elif key == "local_path":
            _, n = self._valid_n()
            idx = st["local_path"][:, 1::2].long().clamp(min=0)
            coords = e._lp_nodes[idx]                              # nodes[edge[1]] per edge (car.py:66)
            keep = (torch.arange(4, device=coords.device)[None, :] < n[:, None])
            v = coords * keep[:, :, None]
        else:  # velocity
            valid, _ = self._valid_n()
            v = torch.where(valid, st["velocity"], torch.zeros_like(st["velocity"]))
        dict.__setitem__(self, key, v)
        return v

    # ---- the derived keys exist as far as any dict protocol can tell
    def _all_keys(self):
        return list(dict.keys(self)) + [k for k in self.DERIVED if not dict.__contains__(self, k)]

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self.DERIVED

    def __iter__(self):
        return iter(self._all_keys())

    def __len__(self):
        return len(self._all_keys())

    def keys(self):
        return self._all_keys()

    def values(self):
        return [self[k] for k in self._all_keys()]

    def items(self):
        return [(k, self[k]) for k in self._all_keys()]

    def get(self, key, default=None):
        return self[key] if key in self else default

    def materialize(self) -> Dict[str, Any]:
        """An independent snapshot: plain dict, every tensor cloned."""
        def cl(v):
            return {k: cl(x) for k, x in v.items()} if isinstance(v, dict) else (v.clone() if isinstance(v, torch.Tensor) else v)
        return {k: cl(self[k]) for k in self._all_keys()}


class TinyCarloVecEnv(gym.Env):
    metadata = {"render_modes": ["rgb_array"]}

    def __init__(self, config: Union[str, Dict[str, Any]], num_envs: Optional[int] = None,
                 device: Union[None, str, torch.device] = None, render_mode: Optional[str] = None,
                 return_numpy: bool = False, autoreset: bool = False, spawn_queue_len: int = 64,
                 spawn: str = "host", obs_packing: Optional[str] = None):
        self.config, self.config_path = load_config(config)
        sim = self.config["sim"]
        self.fps: int = sim.get("fps", 30)
        self.T: float = 1 / self.fps
        self.observation_space_format: str = sim.get("observation_space_format", "rgb")
        if self.observation_space_format not in ("rgb", "classes"):
            raise ValueError("sim.observation_space_format must be 'rgb' or 'classes'")
        self.num_envs = int(num_envs if num_envs is not None else sim.get("num_envs", 1))
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.device = torch.device(device) if device is not None else (
            torch.device(sim["device"]) if "device" in sim else _default_device())
        assert render_mode is None or render_mode in self.metadata["render_modes"]
        self.render_mode = render_mode
        self.return_numpy = return_numpy
        self.autoreset = autoreset
        # where autoreset takes its spawn nodes from: "host" = drawn by the per-env numpy generators into a queue
        # the kernel consumes cyclically (reproduces the reference env reset with seed + i for the first
        # spawn_queue_len re-spawns); "device" = counter-based draw in the kernel (csrc/tc_rng.h), never repeats,
        # no host work, not seed-compatible with the reference's numpy generator
        if spawn not in ("host", "device"):
            raise ValueError("spawn must be 'host' or 'device'")
        self.spawn = spawn
        self._debug_flags = int(os.environ.get("TC_DEBUG_FLAGS", "0"), 0)  # profiling ablations only
        self.wrapped = False          # env.py:56
        self.no_observation = False   # env.py:60

        self.map = Map(self.config["map"], base_path=self.config_path)
        self.car_params = CarParams.from_config(self.T, self.config["car"])
        self.car = CarView(self.car_params, self)
        # per-env cars (set_env_cars / randomize_cars): live [N, 8] f64 rows the kernels read and re-draw, or None
        self._car_rows: Optional[torch.Tensor] = None
        self._car_episode: Optional[torch.Tensor] = None  # [N] int32 episodes drawn per env (randomize_cars)
        self._car_rand: Optional[Dict[str, Any]] = None   # lo, hi, mask, seed, env_offset of randomize_cars
        self.camera = Camera(self.config["camera"], on_update=self._push_camera)
        self.layer_names: List[str] = self.map.get_laneline_names()
        self.n_classes = len(self.layer_names)
        H, W = self.camera.resolution
        self._fmt = nat.FMT_CLASSES if self.observation_space_format == "classes" else nat.FMT_RGB
        # obs_packing="bits": class masks leave the kernels bit-packed, uint8 [C, H, W/8] per env (TC_FMT_CLASSES_BITS,
        # tinycarlo_amd/packing.py); unpack_obs expands them on the device.  An opt-in of the batched env, not a value of
        # sim.observation_space_format: the reference has no such format.
        if obs_packing not in (None, "bits"):
            raise ValueError("obs_packing must be None or 'bits'")
        if obs_packing == "bits":
            if self.observation_space_format != "classes":
                raise ValueError("obs_packing='bits' needs observation_space_format='classes'")
            if W % 32 != 0:
                raise ValueError(f"obs_packing='bits' needs a camera width that is a multiple of 32, not {W}")
            if render_mode == "rgb_array":
                raise ValueError("obs_packing='bits' cannot be combined with render_mode='rgb_array'")
            self._fmt = nat.FMT_CLASSES_BITS
        self.obs_packing = obs_packing

        # spaces (env.py:64-73): per-env spaces; batched tensors carry a leading num_envs axis
        self.single_action_space = gym.spaces.Dict({
            "car_control": gym.spaces.Box(-1, 1, shape=(2,), dtype=np.float32),
            "maneuver": gym.spaces.Discrete(4)})
        obs_shape = ((self.n_classes, H, W // 8) if self._fmt == nat.FMT_CLASSES_BITS else
                     (self.n_classes, H, W) if self._fmt == nat.FMT_CLASSES else (H, W, 3))
        self.single_observation_space = gym.spaces.Box(low=0, high=255, shape=obs_shape, dtype=np.uint8)
        self.action_space = self.single_action_space
        self.observation_space = self.single_observation_space

        self.spawn_queue_len = int(spawn_queue_len)
        self._obs_shape = obs_shape
        # episode time limit / statistics (set_time_limit / track_episodes): the live device tensors, or None = off
        self._episodes: Optional[Dict[str, torch.Tensor]] = None
        self._time_limit = 0                                   # shared max_episode_steps, 0 = none
        self._time_limit_per_env: Optional[torch.Tensor] = None  # [N] int32 device tensor, or None
        # built-in controller (set_controller): its gains, or None = off
        self._ctrl: Optional[Dict[str, float]] = None
        self.steer_last: Optional[torch.Tensor] = None         # [N] f64: the controller's command of the last step
        # drive randomisation (randomize_drive): settings and the four live device tensors, or None = off
        self._drive: Optional[Dict[str, Any]] = None
        # per-episode cameras (randomize_cameras): the bank's device tensors, settings and live index / episode, or None
        self._cam_bank: Optional[Dict[str, Any]] = None
        self._env_cams: Optional[Tuple[torch.Tensor, torch.Tensor]] = None  # static per-env E / K (set_env_cameras)
        self._setup_device()
        self._rngs: List[Optional[np.random.Generator]] = [None] * self.num_envs
        self._was_reset = False
        # torch-side (non-fused) wrappers ask for the mask of envs an autoreset step re-spawned: those did not go
        # through Wrapper.step in the reference's flow (reset() bypasses the wrappers)
        self.track_fresh = False
        self.noise = (0, 0, 0)  # (n_blobs, max_radius, seed) of set_noise
        self.last_fresh: Optional[torch.Tensor] = None
        self._shape_cache: Dict[int, Any] = {}
        self._step_serial = 0      # bumped by every reset / step launch: stale-info detection (LazyInfo)
        self._reserved_steps = 0   # tc_env_reserve_steps: scratch ring of K-step calls that render
        self._reserved_poses = 0   # tc_env_reserve_poses: scratch of deferred frames (render_poses)

    def _setup_device(self) -> None:
        """Creates the native handles and the device tensors the HIP library works on (no CPU path)."""
        if self.device.type != "cuda":
            raise nat.NativeError("tinycarlo_amd runs on an AMD GPU (device 'cuda:N' under ROCm); there is no CPU path")
        if not torch.cuda.is_available():
            raise nat.NativeError("no GPU visible to torch: tinycarlo_amd has no CPU fallback")
        L = nat.lib()
        obs_shape = self._obs_shape
        N, Cn, dev = self.num_envs, self.n_classes, self.device
        with torch.cuda.device(dev):
            self._nmap = nat.NativeMap(self.map)
            h = C.c_void_p()
            cp = nat.make_car_params(self.car_params)
            cam = nat.make_camera_params(self.camera, self._fmt)
            nat.check(L.tc_env_create(self._nmap.handle, C.byref(cp), C.byref(cam), N, C.byref(h)), "tc_env_create")
            self._h = h
            f64 = dict(dtype=torch.float64, device=dev)
            i32 = dict(dtype=torch.int32, device=dev)
            u8 = dict(dtype=torch.uint8, device=dev)
            self.state: Dict[str, torch.Tensor] = {
                "x": torch.zeros(N, **f64), "y": torch.zeros(N, **f64), "theta": torch.zeros(N, **f64),
                "velocity": torch.zeros(N, **f64), "steering": torch.zeros(N, **f64), "radius": torch.zeros(N, **f64),
                "front_x": torch.zeros(N, **f64), "front_y": torch.zeros(N, **f64),
                "local_path": torch.full((N, 8), -1, **i32), "lp_len": torch.zeros(N, **i32),
                "last_maneuver": torch.zeros(N, **i32)}
            self.out: Dict[str, torch.Tensor] = {
                "cte": torch.zeros(N, **f64), "heading_error": torch.zeros(N, **f64), "reward": torch.zeros(N, **f64),
                "terminated": torch.zeros(N, **u8), "truncated": torch.zeros(N, **u8), "status": torch.zeros(N, **i32),
                "laneline_distances": torch.zeros((N, Cn), **f64), "nearest_edge": torch.full((N, Cn), -1, **i32),
                "obs": torch.zeros((N,) + obs_shape, **u8)}
            self._aux: Dict[str, torch.Tensor] = {
                "needs_reset": torch.zeros(N, **u8), "spawn_queue": torch.zeros((N, self.spawn_queue_len), **i32),
                "spawn_cursor": torch.zeros(N, **i32)}
            # steps_true of the consecutive-step termination terms (termination.py:37,59), one per env and slot
            self.term_counters = torch.zeros((N, nat.MAX_TERMS), **i32)
            self.terms: List[Term] = []
            self._lp_nodes = torch.as_tensor(np.asarray(self.map.lanepath.nodes, dtype=np.float64), device=dev)
            b = nat.Buffers()
            for k, t in {**self.state, **self.out, **self._aux}.items():
                setattr(b, k, t.data_ptr())
            b.spawn_queue_len = self.spawn_queue_len
            nat.check(L.tc_env_bind(self._h, C.byref(b)), "tc_env_bind")
        self.obs_bytes_per_env = int(L.tc_env_obs_bytes(self._h))
        self.lds_bytes = int(L.tc_env_lds_bytes(self._h))

    # ------------------------------------------------------------------ helpers
    @property
    def unwrapped(self):
        return self

    def _flags(self) -> int:
        f = 0
        if self.no_observation and self.render_mode is None:  # env.py:78
            f |= nat.F_NO_OBSERVATION
        if self.wrapped:
            f |= nat.F_WRAPPED
        if self.autoreset:
            f |= nat.F_AUTORESET
            if self.spawn == "device":
                f |= nat.F_DEVICE_SPAWN
        return f | self._debug_flags

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _push_camera(self, cam: Camera) -> None:
        cp = nat.make_camera_params(cam, self._fmt)
        nat.check(nat.lib().tc_env_set_camera(self._h, C.byref(cp)), "tc_env_set_camera")

    def set_env_cameras(self, orientation=None, fov=None, position=None) -> None:
        """Per-env camera extrinsics / intrinsics (domain randomisation, train_stanley_il.py:53-57).

        orientation: [N,3] degrees (pitch, roll, yaw), fov: [N] degrees, position: [N,3] metres; any of them may
        be None (keep the shared camera's value).  ``set_env_cameras()`` with no argument returns to the single
        shared camera.  E and K are computed per env on the host with the same code as ``Camera.update_params``.
        Static rows and the per-episode bank of ``randomize_cameras`` exclude each other: this removes a bank."""
        if orientation is None and fov is None and position is None:
            self._push_env_cameras(None, None)
            return
        N = self.num_envs
        ori = np.broadcast_to(np.asarray(self.camera.orientation if orientation is None else orientation, dtype=np.float64), (N, 3))
        fv = np.broadcast_to(np.asarray(self.camera.fov if fov is None else fov, dtype=np.float64), (N,))
        pos = np.broadcast_to(np.asarray(self.camera.position if position is None else position, dtype=np.float64), (N, 3))
        E = np.empty((N, 12), dtype=np.float64)
        K = np.empty((N, 9), dtype=np.float64)
        cache: Dict[Any, Any] = {}
        cfg = dict(self.config["camera"])
        for i in range(N):
            key = (tuple(ori[i]), float(fv[i]), tuple(pos[i]))
            if key not in cache:
                cfg.update(orientation=list(ori[i]), fov=float(fv[i]), position=list(pos[i]))
                c = Camera(cfg)
                cache[key] = (c.E.reshape(-1), c.K.reshape(-1))
            E[i], K[i] = cache[key]
        self._push_env_cameras(E, K)

    def _push_env_cameras(self, E, K) -> None:
        self._cam_bank = None  # (tc_env_set_camera_per_env removes a bank, whatever its arguments)
        if E is None:
            self._env_cams = None
            nat.check(nat.lib().tc_env_set_camera_per_env(self._h, None, None), "tc_env_set_camera_per_env")
            return
        Et = torch.as_tensor(E, dtype=torch.float64).to(self.device).contiguous()
        Kt = torch.as_tensor(K, dtype=torch.float64).to(self.device).contiguous()
        self._env_cams = (Et, Kt)  # keep the device copies alive: the library reads them on every launch
        nat.check(nat.lib().tc_env_set_camera_per_env(self._h, Et.data_ptr(), Kt.data_ptr()), "tc_env_set_camera_per_env")

    # ------------------------------------------------------------------ per-episode cameras from a bank
    CAMERA_ROLLOUT_KEYS = ("camera",)

    def randomize_cameras(self, orientation=None, fov=None, position=None, seed: int = 0, env_offset: int = 0) -> None:
        """Per-episode cameras drawn on the device (the data collection of examples/train_stanley_il.py:53-57: a new
        pitch and fov for every episode).  Each argument is a list of candidate values -- orientation: (pitch, roll, yaw)
        triples in degrees, or a dict ``{"pitch": [...], "roll": [...], "yaw": [...]}`` of per-angle candidates; fov:
        degrees; position: (x, y, z) triples -- and None keeps the shared camera's value.  The bank holds every combination
        (``randomization.camera_bank``; E and K computed on the host with the code of ``Camera.update_params``), and every
        re-spawn of env i (reset, or an autoreset re-spawn inside step / step_multi / drive) draws the index of its next
        episode's camera: ``randomization.draw_camera_index(seed, env_offset + i, camera_episode[i], M)``.  A frame is
        always projected with the camera of the episode it belongs to, however late in a K-step call it is drawn.
        Zeroes the episode counters, so ``reset(seed=...)`` afterwards gives every env its episode-0 camera (until then
        every env uses camera 0).  ``env_offset``: index of env 0 in a larger population (``distributed.shard_range``).
        With no candidate list at all: back to the shared camera.  Removes the static rows of ``set_env_cameras``."""
        from .randomization import camera_bank
        if orientation is None and fov is None and position is None:
            self._set_camera_bank(None)
            return
        if not 0 <= int(env_offset) < 2 ** 32:
            raise ValueError("env_offset must be in [0, 2^32)")
        cfg = dict(self.config["camera"])
        cfg.update(orientation=list(self.camera.orientation), fov=self.camera.fov, position=list(self.camera.position))
        E, K, params = camera_bank(cfg, orientation=orientation, fov=fov, position=position)
        self._set_camera_bank({"E": E, "K": K, "params": params, "seed": int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   "env_offset": int(env_offset)})

    def _set_camera_bank(self, bank: Optional[Dict[str, Any]], index=None, episode=None) -> None:
        with torch.cuda.device(self.device):
            if bank is None:
                if self._cam_bank is not None:
                    nat.check(nat.lib().tc_env_set_camera_bank(self._h, None), "tc_env_set_camera_bank")
                self._cam_bank = None
                return
            E = torch.as_tensor(np.asarray(bank["E"], dtype=np.float64)).to(self.device).contiguous()
            K = torch.as_tensor(np.asarray(bank["K"], dtype=np.float64)).to(self.device).contiguous()
            M = int(E.shape[0])
            if M < 1 or tuple(E.shape) != (M, 12) or tuple(K.shape) != (M, 9):
                raise ValueError(f"camera bank: E must be [M, 12] and K [M, 9], got {tuple(E.shape)} and {tuple(K.shape)}")
            i32 = dict(dtype=torch.int32, device=self.device)
            idx = torch.zeros(self.num_envs, **i32) if index is None else self._to_dev("camera index", index, torch.int32, (self.num_envs,)).clone()
            ep = torch.zeros(self.num_envs, **i32) if episode is None else self._to_dev("camera episode", episode, torch.int32, (self.num_envs,)).clone()
            if index is not None and (int(idx.min()) < 0 or int(idx.max()) >= M):
                raise ValueError(f"camera index outside the bank of {M} cameras")
            self._cam_bank = {"E": E, "K": K, "params": np.array(bank["params"], dtype=np.float64), "seed": int(bank["seed"]),
                              "env_offset": int(bank["env_offset"]), "index": idx, "episode": ep}
            self._env_cams = None  # (the library drops the static rows)
            self._push_camera_bank()

    def _push_camera_bank(self) -> None:
        b = self._cam_bank
        c = nat.CameraBankC(b["E"].data_ptr(), b["K"].data_ptr(), int(b["E"].shape[0]), b["env_offset"], b["seed"],
                            b["index"].data_ptr(), b["episode"].data_ptr())
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_set_camera_bank(self._h, C.byref(c)), "tc_env_set_camera_bank")

    @property
    def camera_index(self) -> Optional[torch.Tensor]:
        """[N] int32 device tensor, live: the camera of the bank each env uses now (None without randomize_cameras)"""
        return None if self._cam_bank is None else self._cam_bank["index"]

    @property
    def camera_episode(self) -> Optional[torch.Tensor]:
        """[N] int32 device counter of the cameras each env has drawn since randomize_cameras (None without it)"""
        return None if self._cam_bank is None else self._cam_bank["episode"]

    @property
    def camera_bank_params(self) -> Optional[np.ndarray]:
        """[M, 7] float64 host table of the bank: pitch, roll, yaw, fov, x, y, z of camera m (None without a bank)"""
        return None if self._cam_bank is None else self._cam_bank["params"]

    # ------------------------------------------------------------------ car constants: shared, per env, per episode
    def _set_shared_car(self, **values) -> None:
        """env.unwrapped.car.<constant> = v: a new shared car for the steps that follow (tc_env_set_car)."""
        if self._car_rows is not None:
            raise RuntimeError("per-env car params are installed: change them with set_env_cars(...) / randomize_cars(...), "
                               "or call set_env_cars() with no argument to return to the shared car first")
        import dataclasses
        for k, v in values.items():
            if getattr(self.car_params, k) is None:
                raise ValueError(f"car.{k} is not set in the config: the engine has no such limit to change")
            v = float(v)
            if not (np.isfinite(v) and v > 0):
                raise ValueError(f"car.{k} must be a positive finite number, got {v}")
            values[k] = v
        p = dataclasses.replace(self.car_params, **values)
        self._push_car(p)
        self.car_params = p

    def _push_car(self, p: CarParams) -> None:
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_set_car(self._h, C.byref(nat.make_car_params(p))), "tc_env_set_car")

    @property
    def env_car_params(self) -> Optional[torch.Tensor]:
        """The live [N, 8] float64 device rows of the per-env cars (columns: ``_native.CAR_COLUMNS``), or None while
        every env runs the shared car.  With ``randomize_cars`` the engine rewrites an env's row at each re-spawn."""
        return self._car_rows

    def set_env_cars(self, wheelbase=None, track_width=None, max_velocity=None, max_steering_angle=None,
                     steering_speed=None, max_acceleration=None, max_deceleration=None, steering_shift=None) -> None:
        """Per-env car constants: each argument a scalar or an [N] sequence / tensor, None = the config's value (shift 0).
        The steering input of env i becomes clip(st + steering_shift[i], -1, 1).  With no argument at all: back to the
        shared car (and no randomisation).  T (fps) stays shared; steering_speed / the acceleration limits only where the
        config has them."""
        from .randomization import car_rows
        vals = dict(wheelbase=wheelbase, track_width=track_width, max_velocity=max_velocity,
                    max_steering_angle=max_steering_angle, steering_speed=steering_speed, max_acceleration=max_acceleration,
                    max_deceleration=max_deceleration, steering_shift=steering_shift)
        if all(v is None for v in vals.values()):
            self._set_car_rows(None)
            return
        self._set_car_rows(torch.as_tensor(car_rows(self.car_params, self.num_envs, vals), dtype=torch.float64))

    def _set_car_rows(self, rows: Optional[torch.Tensor]) -> None:
        with torch.cuda.device(self.device):
            if rows is None:
                nat.check(nat.lib().tc_env_set_car_per_env(self._h, None), "tc_env_set_car_per_env")
                self._car_rows = self._car_episode = self._car_rand = None
                return
            if self._car_rows is None:
                self._car_rows = torch.empty((self.num_envs, nat.CAR_NP), dtype=torch.float64, device=self.device)
            self._car_rows.copy_(rows)
            nat.check(nat.lib().tc_env_set_car_per_env(self._h, self._car_rows.data_ptr()), "tc_env_set_car_per_env")

    def randomize_cars(self, ranges: Optional[Dict[str, Sequence[float]]], seed: int = 0, env_offset: int = 0) -> None:
        """Per-episode car constants drawn on the device: ranges = {name: (lo, hi)} over ``_native.CAR_COLUMNS``.  Every
        re-spawn of env i (reset, or an autoreset re-spawn inside step / step_multi) first draws the named columns of
        its next episode -- ``randomization.draw_car_params(seed, env_offset + i, episode[i], ...)`` -- into its row of
        ``env_car_params``; the other columns keep their values.  Installs per-env rows from the config when there are
        none yet and zeroes the episode counters, so ``reset(seed=...)`` afterwards gives every env its episode-0 draw.
        ``env_offset``: index of env 0 in a larger population (``distributed.shard_range``).  ranges None / {}: no more
        resampling (the rows keep their last values)."""
        from .randomization import car_ranges, config_row
        lo, hi, mask = car_ranges(self.car_params, ranges)
        if not 0 <= int(env_offset) < 2 ** 32:
            raise ValueError("env_offset must be in [0, 2^32)")
        if self._car_rows is None:
            self._set_car_rows(torch.as_tensor(np.tile(config_row(self.car_params), (self.num_envs, 1))))
        with torch.cuda.device(self.device):
            if self._car_episode is None:
                self._car_episode = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            self._car_episode.zero_()
            self._push_car_rand(lo, hi, mask, int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_offset))
        self._car_rand = {"lo": lo, "hi": hi, "mask": mask, "seed": int(seed) & 0xFFFFFFFFFFFFFFFF,
                          "env_offset": int(env_offset)}

    def _push_car_rand(self, lo: np.ndarray, hi: np.ndarray, mask: int, seed: int, env_offset: int) -> None:
        lo_c, hi_c = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        nat.check(nat.lib().tc_env_set_car_randomization(
            self._h, lo_c.ctypes.data_as(C.POINTER(C.c_double)), hi_c.ctypes.data_as(C.POINTER(C.c_double)), mask, seed,
            env_offset, self._car_episode.data_ptr()), "tc_env_set_car_randomization")

    @property
    def car_episode(self) -> Optional[torch.Tensor]:
        """[N] int32 device counter of the episodes each env has drawn since randomize_cars (None without it)."""
        return self._car_episode

    # ------------------------------------------------------------------ episode time limit and statistics
    EPISODE_KEYS = ("length", "ret", "count", "last_length", "last_return", "length_sum", "return_sum")
    EPISODE_ROLLOUT_KEYS = ("episode_length", "episode_return")

    def track_episodes(self, on: bool = True) -> None:
        """Per-env episode statistics kept by the step kernels (tc_env_set_episodes; gymnasium's
        RecordEpisodeStatistics): ``episode_stats`` then holds the live device tensors and ``info`` carries
        ``episode_length`` / ``episode_return``.  ``track_episodes(False)`` switches it off again, time limit included:
        every result is then what it was before.  Turning it on starts from zeroed tensors."""
        if not on:
            if self._episodes is not None:
                with torch.cuda.device(self.device):
                    nat.check(nat.lib().tc_env_set_episodes(self._h, None, 0), "tc_env_set_episodes")
            self._episodes, self._time_limit, self._time_limit_per_env = None, 0, None
            return
        if self._episodes is None:
            N, dev = self.num_envs, self.device
            dts = {"length": torch.int32, "ret": torch.float64, "count": torch.int32, "last_length": torch.int32,
                   "last_return": torch.float64, "length_sum": torch.int64, "return_sum": torch.float64}
            self._episodes = {k: torch.zeros(N, dtype=dts[k], device=dev) for k in self.EPISODE_KEYS}
            self._push_episodes()

    def _push_episodes(self) -> None:
        b = nat.EpisodeBuffers()
        for k in self.EPISODE_KEYS:
            setattr(b, k, self._episodes[k].data_ptr())
        b.limit = self._time_limit_per_env.data_ptr() if self._time_limit_per_env is not None else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_set_episodes(self._h, C.byref(b), int(self._time_limit)), "tc_env_set_episodes")

    def set_time_limit(self, max_episode_steps: Optional[int], per_env=None) -> None:
        """Truncates every episode after ``max_episode_steps`` steps (gymnasium's TimeLimit) inside the step kernels, so
        it also acts between the steps of one ``step_multi`` call: the step that reaches the limit reports
        ``truncated`` with ``TC_S_TIME_LIMIT`` in ``status``, and with autoreset the next step re-spawns the env.
        ``None`` or 0: no shared limit.  ``per_env``: an [N] int tensor / sequence of limits that replaces the shared one
        (entries <= 0: no limit for that env; None: back to the shared limit).  Implies ``track_episodes()``.
        ``episode_stats["length"]`` is an ordinary tensor: write to it to stagger the first episodes, so that the envs
        do not all reach the limit on the same step."""
        lim = 0 if max_episode_steps is None else max_episode_steps
        if isinstance(lim, bool) or not isinstance(lim, (int, np.integer)):
            raise ValueError(f"max_episode_steps must be an int or None, got {max_episode_steps!r}")
        if lim < 0:
            raise ValueError(f"max_episode_steps must not be negative, got {lim}")
        pe = None
        if per_env is not None:
            if isinstance(per_env, torch.Tensor):
                if per_env.is_floating_point() or per_env.dtype == torch.bool:
                    raise ValueError("per_env limits must be integers")
                pe = per_env.detach().to("cpu", torch.int64)
            else:
                a = np.asarray(per_env)
                if a.dtype.kind not in "iu":
                    raise ValueError("per_env limits must be integers")
                pe = torch.from_numpy(a.astype(np.int64))
            if tuple(pe.shape) != (self.num_envs,):
                raise ValueError(f"per_env must have {self.num_envs} entries, got shape {tuple(pe.shape)}")
            if int(pe.min()) < 0 or int(pe.max()) >= 2 ** 31:
                raise ValueError("per_env limits must be in [0, 2^31)")
        self._time_limit = int(lim)
        self._time_limit_per_env = None if pe is None else pe.to(self.device, torch.int32).contiguous()
        if self._episodes is None:
            self.track_episodes(True)
        else:
            self._push_episodes()

    @property
    def episode_stats(self) -> Optional[Dict[str, torch.Tensor]]:
        """The live device tensors of the episode accounting, each [N] (None while it is off): ``length`` / ``ret`` of
        the running episode, ``count`` of finished ones, ``last_length`` / ``last_return`` of the most recent,
        ``length_sum`` / ``return_sum`` over all finished episodes of the env.  Sum them in torch for batch figures."""
        return self._episodes

    # ------------------------------------------------------------------ built-in controller (closed-loop K-step calls)
    CTRL_ROLLOUT_KEYS = ("steer",)

    def set_controller(self, k: Optional[float] = 4.0, speed: float = 0.4) -> None:
        """Installs the Stanley lateral controller of the reference's examples/stanley_control.py:56-57 into the simulate
        kernels (tc_env_set_controller): every step then computes its own action ``(speed, (heading_error + atan2(k * cte,
        speed)) * 180 / pi / max_steering_angle)`` from the env's previous step -- each env with its own
        ``max_steering_angle`` under per-env cars -- so a closed loop runs inside one ``drive`` call.  ``steer_last`` holds
        the command of the last step.  New gains reach a captured HIP graph without re-capture.  ``set_controller(None)``
        switches it off: ``step`` / ``step_multi`` apply their ``car_control`` again (while it is on they ignore it; a
        single step takes no noise and writes no label row, only ``steer_last``)."""
        if k is None:
            if self._ctrl is not None:
                with torch.cuda.device(self.device):
                    nat.check(nat.lib().tc_env_set_controller(self._h, None), "tc_env_set_controller")
            self._ctrl, self.steer_last = None, None
            self._drive = None  # (the library drops the drive randomisation with the controller)
            return
        k, speed = float(k), float(speed)
        if not (np.isfinite(k) and np.isfinite(speed)):
            raise ValueError(f"k and speed must be finite, got {k}, {speed}")
        if self.steer_last is None:
            self.steer_last = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        self._ctrl = {"k": k, "speed": speed}
        self._push_controller()

    def _push_controller(self) -> None:
        c = nat.ControllerC(nat.CTRL_STANLEY, self._ctrl["k"], self._ctrl["speed"], self.steer_last.data_ptr())
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_set_controller(self._h, C.byref(c)), "tc_env_set_controller")

    # ------------------------------------------------------------------ drive randomisation (per-episode maneuver, OU noise)
    DRIVE_ROLLOUT_KEYS = ("maneuver", "steer_noise")
    _MAN_MODES = {"draw": nat.MAN_DRAW, "cycle": nat.MAN_CYCLE}

    def randomize_drive(self, maneuvers: Optional[Sequence[int]] = None, mode: str = "draw", ou: Optional[Dict[str, Any]] = None,
                        seed: int = 0, env_offset: int = 0) -> None:
        """Moves what examples/train_stanley_il.py and examples/train_td3.py do to the action at an episode boundary into the
        simulate kernels (tc_env_set_drive_randomization), so that it follows the episodes of one ``drive`` call:
        ``maneuvers`` -- candidates in {0, 1, 2, 3}, repeats act as weights -- makes the maneuver a per-episode quantity,
        re-drawn (``mode="draw"``: ``randomization.draw_maneuver``) or advanced (``"cycle"``: train_stanley_il.py:105) at every
        re-spawn, and ``drive`` / ``drive_step`` then take ``maneuver=None``; ``ou=dict(theta=0.1, mu=0.0, sigma=0.4,
        reset=False)`` adds Ornstein-Uhlenbeck noise to the applied steering (train_stanley_il.py:66), back to 0 at every
        re-spawn with ``reset=True`` (train_td3.py:177).  Either part may be left out; with neither the feature is off.
        Live tensors: ``episode_maneuver``, ``drive_episode``, ``ou_state``, ``ou_draws``.  Rollout keys ``"maneuver"`` (the
        one in force at each step: the ``Mn`` column) and ``"steer_noise"`` (the OU value applied).  Needs ``set_controller``."""
        if maneuvers is None and ou is None:
            if self._drive is not None:
                with torch.cuda.device(self.device):
                    nat.check(nat.lib().tc_env_set_drive_randomization(self._h, None), "tc_env_set_drive_randomization")
            self._drive = None
            return
        if self._ctrl is None:
            raise ValueError("randomize_drive() needs set_controller() first")
        if not 0 <= int(env_offset) < 2 ** 32:
            raise ValueError("env_offset must be in [0, 2^32)")
        cand = [] if maneuvers is None else [int(m) for m in maneuvers]
        if len(cand) > nat.MAX_MANEUVERS or any(m < 0 or m > 3 for m in cand) or (maneuvers is not None and not cand):
            raise ValueError(f"maneuvers must be 1..{nat.MAX_MANEUVERS} values in 0..3, got {maneuvers!r}")
        if mode not in self._MAN_MODES:
            raise ValueError(f"mode must be 'draw' or 'cycle', got {mode!r}")
        o = None
        if ou is not None:
            unknown = set(ou) - {"theta", "mu", "sigma", "reset"}
            if unknown:
                raise ValueError(f"unknown ou settings {sorted(unknown)}")
            o = {"theta": float(ou.get("theta", 0.1)), "mu": float(ou.get("mu", 0.0)), "sigma": float(ou.get("sigma", 0.4)),
                 "reset": bool(ou.get("reset", False))}
            if not all(np.isfinite(o[k]) for k in ("theta", "mu", "sigma")):
                raise ValueError(f"theta, mu and sigma must be finite, got {ou!r}")
        old = self._drive
        N, dev = self.num_envs, self.device
        keep = lambda k, dt: old[k] if old is not None else torch.zeros(N, dtype=dt, device=dev)  # noqa: E731
        self._drive = {"maneuvers": tuple(cand), "mode": mode, "ou": o, "seed": int(seed) & 0xFFFFFFFFFFFFFFFF,
                       "env_offset": int(env_offset),
                       "maneuver": keep("maneuver", torch.int32), "episode": keep("episode", torch.int32),
                       "ou_state": keep("ou_state", torch.float64), "ou_draws": keep("ou_draws", torch.int32)}
        self._push_drive()

    def set_ou(self, theta: Optional[float] = None, mu: Optional[float] = None, sigma: Optional[float] = None,
               reset: Optional[bool] = None) -> None:
        """New OU settings in place (``sigma``: the annealing of train_td3.py:179); they reach a captured HIP graph without
        re-capture.  The OU state and the draw counters keep their values."""
        if self._drive is None or self._drive["ou"] is None:
            raise ValueError("set_ou() needs randomize_drive(ou=...) first")
        o = dict(self._drive["ou"])
        for k, v in (("theta", theta), ("mu", mu), ("sigma", sigma)):
            if v is not None:
                if not np.isfinite(float(v)):
                    raise ValueError(f"{k} must be finite, got {v}")
                o[k] = float(v)
        if reset is not None:
            o["reset"] = bool(reset)
        self._drive["ou"] = o
        self._push_drive()

    def _push_drive(self) -> None:
        d, c = self._drive, nat.DriveRandomizationC()
        c.seed, c.env_offset, c.n_maneuvers = d["seed"], d["env_offset"], len(d["maneuvers"])
        for i, m in enumerate(d["maneuvers"]):
            c.maneuvers[i] = m
        c.maneuver_mode = self._MAN_MODES[d["mode"]]
        o = d["ou"]
        if o is not None:
            c.theta, c.mu, c.sigma, c.ou_reset = o["theta"], o["mu"], o["sigma"], int(o["reset"])
            c.ou_state, c.ou_draws = d["ou_state"].data_ptr(), d["ou_draws"].data_ptr()
        if d["maneuvers"]:
            c.maneuver, c.episode = d["maneuver"].data_ptr(), d["episode"].data_ptr()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_set_drive_randomization(self._h, C.byref(c)), "tc_env_set_drive_randomization")

    @property
    def _device_maneuvers(self) -> bool:
        return self._drive is not None and len(self._drive["maneuvers"]) > 0

    @property
    def episode_maneuver(self) -> Optional[torch.Tensor]:
        """[N] int32, live: the maneuver in force for each env (randomize_drive with maneuvers), else None"""
        return self._drive["maneuver"] if self._device_maneuvers else None

    @property
    def drive_episode(self) -> Optional[torch.Tensor]:
        """[N] int32, live: maneuvers drawn so far"""
        return self._drive["episode"] if self._device_maneuvers else None

    @property
    def ou_state(self) -> Optional[torch.Tensor]:
        """[N] float64, live and writable: the OU value each env applied last (randomize_drive with ou), else None"""
        return self._drive["ou_state"] if self._drive is not None and self._drive["ou"] is not None else None

    @property
    def ou_draws(self) -> Optional[torch.Tensor]:
        """[N] int32, live: normals consumed so far (never reset)"""
        return self._drive["ou_draws"] if self._drive is not None and self._drive["ou"] is not None else None

    def drive(self, maneuver: Optional[torch.Tensor], rollout: Optional[Dict[str, torch.Tensor]] = None,
              steer_noise: Optional[torch.Tensor] = None, n_steps: Optional[int] = None) -> None:
        """K closed-loop steps in ONE call: ``step_multi`` with every step's action computed on the device by the
        controller of ``set_controller``.  maneuver [K, N] int32; steer_noise [K, N] float64 (optional) is added to the
        command of step k before it is applied (the exploration noise of examples/train_stanley_il.py's data
        collection); ``rollout["steer"]`` (``alloc_rollout(K, keys=(..., "steer"))``) receives the command BEFORE noise,
        the imitation-learning label.  Bit-identical to K ``step_device`` calls with the action computed on the host from
        ``out["cte"]`` / ``out["heading_error"]`` before each.  With ``randomize_drive(maneuvers=...)`` the maneuvers are the
        device's own: ``maneuver`` is None and the number of steps comes from ``n_steps``, the rollout or ``steer_noise``."""
        self.prepare_drive(maneuver, rollout, steer_noise, n_steps)()

    def prepare_drive(self, maneuver: Optional[torch.Tensor], rollout: Optional[Dict[str, torch.Tensor]] = None,
                      steer_noise: Optional[torch.Tensor] = None, n_steps: Optional[int] = None) -> "PreparedStepMulti":
        """`drive` as a checked, reusable call object (see `prepare_step_multi`)."""
        if self._ctrl is None:
            raise RuntimeError("drive() needs set_controller() first")
        if maneuver is None:
            if not self._device_maneuvers:
                raise ValueError("drive(maneuver=None) needs randomize_drive(maneuvers=...) first")
            K = int(n_steps) if n_steps is not None else (int(steer_noise.shape[0]) if steer_noise is not None else
                                                         (int(next(iter(rollout.values())).shape[0]) if rollout else 0))
            if K < 1:
                raise ValueError("drive(maneuver=None) takes its number of steps from n_steps, the rollout or steer_noise")
        else:
            if maneuver.dim() != 2 or int(maneuver.shape[0]) < 1 or int(maneuver.shape[1]) != self.num_envs:
                raise ValueError(f"maneuver must be [K, {self.num_envs}], got {tuple(maneuver.shape)}")
            K = int(maneuver.shape[0])
            if maneuver.device != self.device or maneuver.dtype != torch.int32 or not maneuver.is_contiguous():
                raise ValueError("drive takes a contiguous int32 device tensor as maneuver")
            if n_steps is not None and int(n_steps) != K:
                raise ValueError(f"n_steps = {n_steps} does not fit maneuver rows of {K} steps")
        if steer_noise is not None and (tuple(steer_noise.shape) != (K, self.num_envs) or steer_noise.dtype != torch.float64 or
                                        steer_noise.device != self.device or not steer_noise.is_contiguous()):
            raise ValueError(f"steer_noise must be a contiguous float64 tensor of shape ({K}, {self.num_envs}) on {self.device}")
        r, rows = self._check_rollout(rollout, K)
        if steer_noise is not None:
            rows.steer_noise_in, rows.n_rows = steer_noise.data_ptr(), K
        return PreparedStepMulti(self, None, maneuver, rollout, r, rows, K, steer_noise)

    def drive_step(self, maneuver: Optional[torch.Tensor] = None) -> None:
        """One closed-loop step (tc_step with the controller's action): `step_device` without a car_control."""
        if self._ctrl is None:
            raise RuntimeError("drive_step() needs set_controller() first")
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        if maneuver is None:
            if not self._device_maneuvers:
                raise ValueError("drive_step(maneuver=None) needs randomize_drive(maneuvers=...) first")
        elif (tuple(maneuver.shape) != (self.num_envs,) or maneuver.device != self.device or maneuver.dtype != torch.int32 or
                not maneuver.is_contiguous()):
            raise ValueError(f"drive_step takes a contiguous int32 device tensor of shape ({self.num_envs},) as maneuver")
        self._note_fresh()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_step(self._h, None, nat.F64, maneuver.data_ptr() if maneuver is not None else None,
                                        self._flags(), self._stream()), "tc_step")
        self._keep = (maneuver,)
        self._step_serial += 1

    # ------------------------------------------------------------------ fused reward / termination wrappers
    def set_terms(self, terms: Sequence[Term]) -> None:
        """Installs the wrapper stack `terms` (innermost first) into the step kernel (tc_env_set_terms); the
        counters of the consecutive-step terms are cleared.  An empty list removes all terms."""
        terms = list(terms)
        if len(terms) > nat.MAX_TERMS:
            raise ValueError(f"at most {nat.MAX_TERMS} fused terms")
        arr = nat.make_terms(terms)
        with torch.cuda.device(self.device):
            self.term_counters.zero_()
            nat.check(nat.lib().tc_env_set_terms(self._h, arr, len(terms), self.term_counters.data_ptr()),
                      "tc_env_set_terms")
        self.terms = terms

    def add_term(self, term: Term) -> int:
        """Appends one term (the next wrapper of the stack); returns its slot in `term_counters`."""
        self.set_terms(self.terms + [term])
        return len(self.terms) - 1

    # ------------------------------------------------------------------ NoiseObservationWrapper (wrapper/observation.py)
    def set_noise(self, n_blobs: int, max_radius: int = 100, seed: int = 0) -> None:
        """Blob noise on class-mask observations after every step (tc_env_set_noise); n_blobs = 0 switches it off.
        Blobs are drawn on the device -- the reference's global ``np.random`` stream cannot be reproduced for a batch."""
        if n_blobs and self._fmt not in (nat.FMT_CLASSES, nat.FMT_CLASSES_BITS):
            raise ValueError("observation noise needs observation_space_format='classes' (wrapper/observation.py:7)")
        self._push_noise(int(n_blobs), int(max_radius), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.noise = (int(n_blobs), int(max_radius), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def _push_noise(self, n_blobs: int, max_radius: int, seed: int) -> None:
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_set_noise(self._h, n_blobs, max_radius, seed), "tc_env_set_noise")

    def apply_noise(self, blobs=None) -> torch.Tensor:
        """The noise pass alone on the current observation.  blobs: int32 [N, n_classes * n_blobs, 5] rows
        (x, y, radius, mode, src) to use instead of device-drawn ones (mode 1 = copy from plane src, 0 = erase)."""
        bt = None
        if blobs is not None:
            bt = self._to_dev("blobs", blobs, torch.int32, (self.num_envs, self.n_classes * self.noise[0], 5))
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_noise(self._h, bt.data_ptr() if bt is not None else None, self._stream()), "tc_noise")
        self._keep = (bt,)
        return self.out["obs"]

    @staticmethod
    def unpack_obs(packed: torch.Tensor, dtype: torch.dtype = torch.float32, index: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Bit-packed observations -> [..., C, H, W] of ``dtype`` on the device (tinycarlo_amd.packing.unpack_obs)."""
        from .packing import unpack_obs
        return unpack_obs(packed, dtype=dtype, index=index, out=out)

    def make_sample_buffer(self, capacity: int, columns=("maneuver", "steer"), **kw):
        """A `tinycarlo_amd.SampleBuffer` for this env's K-step calls: num_envs, the frame shape, its packing and the device
        filled in.  columns: names of `[K, N]` rollout keys the env can produce now (a sequence: their rollout dtypes; a
        mapping name -> dtype must agree with them).  Other arguments (next_obs, stride, overflow, seed, max_rows, history) pass
        through; `history=T` keeps a link per slot so that `buf.sample` returns the last T frames of the episode
        (ReplaybufferTemporal's samples).  `buf.begin(obs)` after `reset()`, `buf.collect(rollout)` after each call."""
        from .collect import SampleBuffer
        shapes = self._rollout_shapes(1)
        needs = ((self.EPISODE_ROLLOUT_KEYS, self._episodes, "track_episodes() / set_time_limit()"),
                 (self.CTRL_ROLLOUT_KEYS, self._ctrl, "set_controller()"), (self.CAMERA_ROLLOUT_KEYS, self._cam_bank, "randomize_cameras()"),
                 (self.DRIVE_ROLLOUT_KEYS, self._drive, "randomize_drive()"))
        cols = {}
        for name in columns:
            if name not in shapes or shapes[name][0] != (1, self.num_envs) or name in ("terminated", "truncated"):
                raise ValueError(f"column {name!r} is not a [K, N] rollout key of this env")
            for keys, have, what in needs:
                if name in keys and have is None:
                    raise ValueError(f"column {name!r} needs {what} first")
            if isinstance(columns, dict) and columns[name] != shapes[name][1]:
                raise ValueError(f"column {name!r} is {shapes[name][1]} in this env's rollouts, not {columns[name]}")
            cols[name] = shapes[name][1]
        for k in ("num_envs", "obs_shape", "device", "packed"):
            if k in kw:
                raise ValueError(f"{k} is the env's")
        return SampleBuffer(capacity, self.num_envs, self._obs_shape, columns=cols, device=self.device,
                            packed=self.obs_packing == "bits", **kw)

    def _to_dev(self, key: str, a, dtype: torch.dtype, shape: Tuple[int, ...]) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            t = a
            if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
                t = t.to(device=self.device, dtype=dtype).contiguous()
        else:
            t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device)
        if tuple(t.shape) != shape:
            raise ValueError(f"{key} must have shape {shape}, got {tuple(t.shape)}")
        return t

    def seed_generators(self, seed: Optional[int]) -> None:
        """env i gets gymnasium's np_random(seed + i); seed None only fills generators that do not exist yet."""
        for i in range(self.num_envs):
            if seed is not None:
                self._rngs[i] = gym.np_random(int(seed) + i)[0]
            elif self._rngs[i] is None:
                self._rngs[i] = gym.np_random(None)[0]

    def draw_spawn_nodes(self, mask: Optional[np.ndarray] = None) -> np.ndarray:
        nodes = np.zeros(self.num_envs, dtype=np.int32)
        for i in range(self.num_envs):
            if mask is None or mask[i]:
                nodes[i] = self.map.sample_spawn_node(self._rngs[i])
        return nodes

    def set_spawn_seed(self, seed: int) -> None:
        """(re)starts the device-side spawn stream: uploads the spawn table with `seed`, clears the re-spawn counters"""
        tab = np.ascontiguousarray(self.map.spawn_table(), dtype=np.int32)
        self._push_spawn_table(tab, int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._aux["spawn_cursor"].zero_()
        self.spawn_seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def _push_spawn_table(self, tab: np.ndarray, seed: int) -> None:
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_set_spawn_table(self._h, tab.ctypes.data, int(tab.size), seed),
                      "tc_env_set_spawn_table")

    def refill_spawn_queue(self) -> None:
        """Pre-draws `spawn_queue_len` spawn nodes per env for device-side auto-reset (consumed cyclically)."""
        q = np.zeros((self.num_envs, self.spawn_queue_len), dtype=np.int32)
        for i in range(self.num_envs):
            for j in range(self.spawn_queue_len):
                q[i, j] = self.map.sample_spawn_node(self._rngs[i])
        self._aux["spawn_queue"].copy_(torch.from_numpy(q))
        self._aux["spawn_cursor"].zero_()

    def top_up_spawn_queue(self) -> int:
        """spawn="host": continues every env's seeded spawn stream past the entries the kernel has consumed.

        The queue holds `spawn_queue_len` pre-drawn spawn nodes per env and the kernel reads it cyclically, so an env
        that re-spawned more often than that would replay nodes (flagged TC_S_SPAWN_WRAPPED in `status`).  This keeps
        the entries an env has not used yet, appends as many fresh draws from that env's numpy generator as it has
        used, and clears the cursors -- the sequence of spawn nodes each env sees stays exactly the one the reference
        env seeded `seed + i` would draw, for as long as this is called before any env uses up its queue (call it
        between rollouts: one device->host copy of the cursors, host work only for envs that re-spawned).
        Returns the largest number of entries any env had consumed."""
        if not self.autoreset or self.spawn != "host":
            return 0
        cur = self._aux["spawn_cursor"].cpu().numpy()
        used = int(cur.max()) if cur.size else 0
        if used == 0:
            return 0
        q = self._aux["spawn_queue"].cpu().numpy()
        L_ = self.spawn_queue_len
        for i in np.flatnonzero(cur > 0):
            c = int(min(cur[i], L_))
            fresh = [self.map.sample_spawn_node(self._rngs[i]) for _ in range(c)]
            pos = int(cur[i]) % L_ if cur[i] >= L_ else c      # a wrapped env restarts from what the kernel would read next
            rest = np.concatenate([q[i, pos:], q[i, :pos]])[: L_ - c] if cur[i] >= L_ else q[i, c:]
            q[i] = np.concatenate([rest, np.asarray(fresh, dtype=np.int32)])[:L_]
        self._aux["spawn_queue"].copy_(torch.from_numpy(q))
        self._aux["spawn_cursor"].zero_()
        return used

    # ------------------------------------------------------------------ gym API
    def reset(self, seed: Optional[int] = None, options: Optional[Any] = None, mask=None):
        """env.py:101-113 for every env (or the envs selected by the boolean `mask`)."""
        self.seed_generators(seed)
        mk_np = None if mask is None else np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
        nodes = self.draw_spawn_nodes(mk_np)
        if self.autoreset and (seed is not None or not self._was_reset):
            if self.spawn == "device":
                self.set_spawn_seed(seed if seed is not None else 0)
            else:
                self.refill_spawn_queue()
        self.reset_to(nodes, mk_np)
        return self._obs(), self._info()

    def reset_to(self, spawn_nodes, mask=None) -> None:
        """Reset with explicit spawn nodes (lanepath node ids); device-side only, no RNG involved."""
        nd = self._to_dev("spawn_nodes", spawn_nodes, torch.int32, (self.num_envs,))
        if mask is None:
            mk = None
        elif isinstance(mask, torch.Tensor):  # bool / uint8 tensors (host or device) are taken as they are
            mk = self._to_dev("mask", mask.to(torch.uint8), torch.uint8, (self.num_envs,))
        else:
            mk = self._to_dev("mask", np.asarray(mask, dtype=np.uint8), torch.uint8, (self.num_envs,))
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_reset(self._h, nd.data_ptr(), mk.data_ptr() if mk is not None else None,
                                         self._flags() & ~nat.F_AUTORESET, self._stream()), "tc_reset")
        self._keep = (nd, mk)
        self._was_reset = True
        self._step_serial += 1

    def step(self, action: Dict[str, Any]):
        """env.py:115-147 for every env.  action = {"car_control": [N,2] float32|float64, "maneuver": [N] int}."""
        cc = action["car_control"]
        if isinstance(cc, torch.Tensor):
            dt = torch.float64 if cc.dtype == torch.float64 else torch.float32
        else:
            cc = np.asarray(cc)
            dt = torch.float32 if cc.dtype == np.float32 else torch.float64
        cc_t = self._to_dev("car_control", cc, dt, (self.num_envs, 2))
        mn_t = self._to_dev("maneuver", action["maneuver"], torch.int32, (self.num_envs,))
        dbg = gym_getenv("DEBUG")  # env.py:144 reads the switch on every step
        if dbg:
            t_dbg = time.perf_counter()
            self.profile(1)
        self.step_device(cc_t, mn_t)
        if dbg:
            self._debug_print("step", t_dbg)
        o = self.out
        if self.return_numpy:
            return (self._obs(), o["reward"].cpu().numpy(), o["terminated"].cpu().numpy().astype(bool),
                    o["truncated"].cpu().numpy().astype(bool), self._info())
        # (the engine writes 0 / 1 bytes: reinterpreted as bool in place, no conversion kernel per step)
        return self._obs(), o["reward"], o["terminated"].view(torch.bool), o["truncated"].view(torch.bool), self._info()

    def step_device(self, car_control: torch.Tensor, maneuver: torch.Tensor) -> None:
        """The bare hot path: one launch, nothing returned (results are in self.out / self.state)."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        self._note_fresh()
        dt = nat.F64 if car_control.dtype == torch.float64 else nat.F32
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_step(self._h, car_control.data_ptr(), dt, maneuver.data_ptr(), self._flags(),
                                        self._stream()), "tc_step")
        self._keep = (car_control, maneuver)
        self._step_serial += 1

    def _debug_print(self, what: str, t0: float) -> None:
        """DEBUG=1 (helper.py:4-9; env.py:116-129,144-145 prints `all | obs render | info | car step` from
        time.perf_counter): here the phases are kernels, timed with HIP events on the launch stream (tc_env_profile):
        `simulate` = car.step + get_info (+ camera and raster when the step is one fused kernel), `frames` = camera +
        raster when they run as launches of their own.  Waits for the launch, like the reference's timer does."""
        p = self.profile_read()
        self.profile(0)
        all_ms = (time.perf_counter() - t0) * 1000
        print(f"{what}: all: {all_ms:.2f} ms | kernels: simulate {p['simulate_us'] / 1000:.4f} ms | frames "
              f"{p['raster_us'] / 1000:.4f} ms | {self.num_envs} envs")

    ROLLOUT_KEYS = ("obs", "reward", "terminated", "truncated", "cte", "heading_error")
    # the rest of step()'s info dict (env.py:83-85) and the status bits, per step (ABI 5)
    INFO_ROLLOUT_KEYS = ("status", "x", "y", "theta", "velocity", "laneline_distances", "nearest_edge", "local_path", "lp_len")

    def _rollout_shapes(self, K: int):
        N, Cn = self.num_envs, self.n_classes
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        return {"obs": ((K, N) + self._obs_shape, u8), "reward": ((K, N), f64), "terminated": ((K, N), u8),
                "truncated": ((K, N), u8), "cte": ((K, N), f64), "heading_error": ((K, N), f64),
                "status": ((K, N), i32), "x": ((K, N), f64), "y": ((K, N), f64), "theta": ((K, N), f64),
                "velocity": ((K, N), f64), "laneline_distances": ((K, N, Cn), f64), "nearest_edge": ((K, N, Cn), i32),
                "local_path": ((K, N, 8), i32), "lp_len": ((K, N), i32),
                "episode_length": ((K, N), i32), "episode_return": ((K, N), f64), "steer": ((K, N), f64),
                "camera": ((K, N), i32), "maneuver": ((K, N), i32), "steer_noise": ((K, N), f64)}

    def reserve_steps(self, n_steps: int) -> None:
        """Sizes the library's scratch ring for K-step calls that render observations (tc_env_reserve_steps): done
        once, outside any timed or captured region -- `step_multi` itself never allocates.  `step_multi` calls this on
        first use; call it yourself before capturing a `step_multi` into a HIP graph."""
        if int(n_steps) > self._reserved_steps:
            with torch.cuda.device(self.device):
                nat.check(nat.lib().tc_env_reserve_steps(self._h, int(n_steps)), "tc_env_reserve_steps")
            self._reserved_steps = int(n_steps)

    def alloc_rollout(self, n_steps: int, keys: Sequence[str] = ("obs", "reward", "terminated", "truncated")) -> Dict[str, torch.Tensor]:
        """Device tensors for the per-step outputs of `step_multi`: [n_steps, num_envs, ...] each."""
        K, dev = int(n_steps), self.device
        shapes = self._rollout_shapes(K)
        if keys == "all":  # (the episode rows only while the accounting is on, the controller's while one is installed)
            keys = self.ROLLOUT_KEYS + self.INFO_ROLLOUT_KEYS + (self.EPISODE_ROLLOUT_KEYS if self._episodes is not None else ()) + \
                (self.CTRL_ROLLOUT_KEYS if self._ctrl is not None else ()) + \
                (self.CAMERA_ROLLOUT_KEYS if self._cam_bank is not None else ()) + \
                (self.DRIVE_ROLLOUT_KEYS if self._drive is not None else ())
        for k in keys:
            if k not in shapes:
                raise ValueError(f"unknown rollout key {k!r}; choose from "
                                 f"{self.ROLLOUT_KEYS + self.INFO_ROLLOUT_KEYS + self.EPISODE_ROLLOUT_KEYS + self.CTRL_ROLLOUT_KEYS + self.CAMERA_ROLLOUT_KEYS + self.DRIVE_ROLLOUT_KEYS}")
            if k in self.EPISODE_ROLLOUT_KEYS and self._episodes is None:
                raise ValueError(f"rollout key {k!r} needs track_episodes() / set_time_limit() first")
            if k in self.CTRL_ROLLOUT_KEYS and self._ctrl is None:
                raise ValueError(f"rollout key {k!r} needs set_controller() first")
            if k in self.CAMERA_ROLLOUT_KEYS and self._cam_bank is None:
                raise ValueError(f"rollout key {k!r} needs randomize_cameras() first")
            if k in self.DRIVE_ROLLOUT_KEYS and self._drive is None:
                raise ValueError(f"rollout key {k!r} needs randomize_drive() first")
        return {k: torch.zeros(shapes[k][0], dtype=shapes[k][1], device=dev) for k in keys}

    def rollout_info(self, rollout: Dict[str, torch.Tensor], k: int) -> Dict[str, Any]:
        """info dict of step k of a `step_multi` call (env.py:83-85 per step), built from the rollout's info rows
        (`alloc_rollout(K, keys="all")` or at least INFO_ROLLOUT_KEYS + cte + heading_error): same keys and values as
        `step()`'s info after the k-th of K single steps."""
        lp_len = rollout["lp_len"][k]
        valid = lp_len >= 2
        n = torch.where(valid, lp_len, torch.zeros_like(lp_len))
        idx = rollout["local_path"][k][:, 1::2].long().clamp(min=0)
        coords = self._lp_nodes[idx]
        keep = (torch.arange(4, device=coords.device)[None, :] < n[:, None])
        vel = rollout["velocity"][k]
        ep = {key: rollout[key][k] for key in self.EPISODE_ROLLOUT_KEYS if key in rollout}
        return {**ep, "cte": rollout["cte"][k], "heading_error": rollout["heading_error"][k],
                "position": torch.stack([rollout["x"][k], rollout["y"][k]], dim=1), "orientation": rollout["theta"][k],
                "laneline_distances": {name: rollout["laneline_distances"][k][:, i] for i, name in enumerate(self.layer_names)},
                "local_path": coords * keep[:, :, None], "local_path_len": n,
                "velocity": torch.where(valid, vel, torch.zeros_like(vel)), "status": rollout["status"][k]}

    def step_multi(self, car_control: torch.Tensor, maneuver: torch.Tensor,
                   rollout: Optional[Dict[str, torch.Tensor]] = None) -> None:
        """K steps in ONE launch (tc_step_multi): the caller's `for k: env.step(action[k])` loop of
        env.py:115-147 with the actions known in advance.  car_control [K, N, 2] float32|float64, maneuver [K, N]
        int32, both on the device.  Bit-identical to K calls of `step_device`; self.state / self.out hold step K-1
        afterwards.  `rollout` (from `alloc_rollout`) receives every step's outputs; with rollout["obs"] the
        observations go there and self.out["obs"] is left untouched."""
        self.prepare_step_multi(car_control, maneuver, rollout)()

    def prepare_step_multi(self, car_control: torch.Tensor, maneuver: torch.Tensor,
                           rollout: Optional[Dict[str, torch.Tensor]] = None) -> "PreparedStepMulti":
        """Checks the arguments of a `step_multi` call and sizes the library's scratch for it once, and returns the call
        as an object: `call()` then only enqueues it (one C call on the current stream) -- for loops that step the same
        action / rollout tensors again and again (their CONTENTS may change between calls, the tensors may not), where
        the argument checks of `step_multi` (tens of microseconds of Python) would be paid per call."""
        if car_control.dim() != 3 or tuple(car_control.shape[1:]) != (self.num_envs, 2):
            raise ValueError(f"car_control must be [K, {self.num_envs}, 2], got {tuple(car_control.shape)}")
        K = int(car_control.shape[0])
        if K < 1 or tuple(maneuver.shape) != (K, self.num_envs):
            raise ValueError(f"maneuver must be [{K}, {self.num_envs}], got {tuple(maneuver.shape)}")
        if car_control.device != self.device or maneuver.device != self.device:
            raise ValueError("step_multi takes device tensors")
        if car_control.dtype not in (torch.float32, torch.float64) or maneuver.dtype != torch.int32:
            raise ValueError("car_control must be float32|float64 and maneuver int32")
        if not (car_control.is_contiguous() and maneuver.is_contiguous()):
            raise ValueError("step_multi takes contiguous tensors")
        r, rows = self._check_rollout(rollout, K)
        return PreparedStepMulti(self, car_control, maneuver, rollout, r, rows, K)

    # the rollout keys that are feature rows of the call (tc_step_rows) and no members of tc_rollout: the member, the
    # attribute that is None while the feature is off, and what switches it on
    _STEP_ROWS = {"episode_length": ("episode_length_out", "_episodes", "track_episodes() / set_time_limit()"),
                  "episode_return": ("episode_return_out", "_episodes", "track_episodes() / set_time_limit()"),
                  "steer": ("steer_out", "_ctrl", "set_controller()"),
                  "camera": ("camera_out", "_cam_bank", "randomize_cameras()"),
                  "maneuver": ("maneuver_out", "_drive", "randomize_drive()"),
                  "steer_noise": ("ou_noise_out", "_drive", "randomize_drive()")}  # (the OU value applied, an output)

    def _check_rollout(self, rollout: Optional[Dict[str, torch.Tensor]], K: int) -> Tuple["nat.Rollout", "nat.StepRows"]:
        """the tc_rollout and tc_step_rows of a K-step call from its checked tensors; sizes the library's scratch for the call"""
        r, rows = nat.Rollout(), nat.StepRows()
        if rollout:
            want = self._shape_cache.get(K)
            if want is None:
                want = self._shape_cache[K] = self._rollout_shapes(K)
            for k, t in rollout.items():
                if k not in want:
                    raise ValueError(f"unknown rollout key {k!r}")
                shp, dt_ = want[k]
                if t.dtype != dt_ or tuple(t.shape) != shp or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"rollout[{k!r}] must be a contiguous {dt_} tensor of shape {shp} on {self.device}")
                if k in self._STEP_ROWS:
                    member, feature, switch = self._STEP_ROWS[k]
                    if getattr(self, feature) is None:
                        raise ValueError(f"rollout[{k!r}] needs {switch} first")
                    setattr(rows, member, t.data_ptr())
                    rows.n_rows = K
                    continue
                setattr(r, k, t.data_ptr())
        if K > 1 and not (self.no_observation and self.render_mode is None):
            self.reserve_steps(K)  # (no-op once the scratch covers K: the call itself never allocates)
        return r, rows

    def launch_info(self, n_steps: int = 1) -> Dict[str, Any]:
        """What a call of n_steps steps launches with the current settings (tc_env_launch_info): for benchmark labels."""
        f, kv, spd, name = C.c_int32(), C.c_int32(), C.c_int32(), C.create_string_buffer(64)
        nat.check(nat.lib().tc_env_launch_info(self._h, self._flags(), int(n_steps), C.byref(f), C.byref(kv), C.byref(spd),
                                               name, 64), "tc_env_launch_info")
        return {"fused": bool(f.value), "kvar": kv.value, "kernel": name.value.decode(), "steps_per_dispatch": spd.value}

    def envg_lds_info(self, info_every: bool = False) -> Dict[str, int]:
        """The LDS of a workgroup of the grouped simulate launch of a K-step call (tc_env_envg_lds_info): dynamic and
        static bytes, workgroups per launch, frame workgroups that fit on a CU beside one, and whether the lane-line edge
        records sit in LDS.  info_every: a call with laneline_distances / nearest_edge rows.  No launch."""
        d, s, w, f, m = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_envg_lds_info(self._h, int(bool(info_every)), C.byref(d), C.byref(s), C.byref(w),
                                                     C.byref(f), C.byref(m)), "tc_env_envg_lds_info")
        return {"dynamic_bytes": d.value, "static_bytes": s.value, "workgroups": w.value, "frames_beside": f.value,
                "map_in_lds": m.value}

    def frame_lds_info(self) -> Dict[str, int]:
        """The LDS plan of the handle's frame kernel (tc_env_frame_lds_info): bytes per workgroup, draw-list entries its
        LDS head holds, workgroups per CU as the runtime computes them, offset of the raster bit-planes; and the raster
        bands of a frame (tc_env_frame_bands): their number and rows.  No launch."""
        b, h, w, o = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        nb, br = C.c_int32(), C.c_int32()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_frame_lds_info(self._h, C.byref(b), C.byref(h), C.byref(w), C.byref(o)),
                      "tc_env_frame_lds_info")
            nat.check(nat.lib().tc_env_frame_bands(self._h, C.byref(nb), C.byref(br)), "tc_env_frame_bands")
        return {"lds_bytes": b.value, "head_entries": h.value, "workgroups_per_cu": w.value, "bits_offset": o.value,
                "bands": nb.value, "band_rows": br.value}

    def draw_list_stats(self) -> Dict[str, Any]:
        """What the most recent frames drew (tc_env_draw_list_stats; waits for the device): workload descriptor."""
        m, e, mx, fr = C.c_double(), C.c_double(), C.c_int32(), C.c_int64()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_draw_list_stats(self._h, C.byref(m), C.byref(e), C.byref(mx), C.byref(fr)),
                      "tc_env_draw_list_stats")
        return {"mean_segments_per_frame": m.value, "empty_frame_frac": e.value, "max_segments": mx.value, "frames": fr.value}

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self) -> Dict[str, Any]:
        """Everything needed to continue the batch bit for bit elsewhere or later: car state, last outputs, auto-reset
        bookkeeping, term counters and the host spawn generators (the reference has no env checkpoint; its whole state
        is `car.*`, car.py:25-32).  Tensors are cloned to the host."""
        torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
        cb = self._cam_bank
        # per-episode cameras: the bank, its draw settings, the index in force and the episode counters (only with a bank)
        bank = {} if cb is None else {"camera_bank": {
            "E": cb["E"].detach().cpu().clone(), "K": cb["K"].detach().cpu().clone(), "params": cb["params"].copy(),
            "seed": cb["seed"], "env_offset": cb["env_offset"], "index": cb["index"].detach().cpu().clone(),
            "episode": cb["episode"].detach().cpu().clone()}}
        return {**bank, "num_envs": self.num_envs,
                "state": {k: v.detach().cpu().clone() for k, v in self.state.items()},
                "out": {k: v.detach().cpu().clone() for k, v in self.out.items()},
                "aux": {k: v.detach().cpu().clone() for k, v in self._aux.items()},
                "term_counters": self.term_counters.detach().cpu().clone(),
                "rng": [None if g is None else g.bit_generator.state for g in self._rngs],
                "was_reset": self._was_reset,
                # per-env cars: the rows in force, and the randomisation (ranges, mask, seed, offset, episode counters)
                "car_per_env": None if self._car_rows is None else {
                    "rows": self._car_rows.detach().cpu().clone(),
                    "episode": None if self._car_episode is None else self._car_episode.detach().cpu().clone(),
                    "randomization": None if self._car_rand is None else dict(self._car_rand)},
                # episode accounting: the limits and every tensor of episode_stats
                "episodes": None if self._episodes is None else {
                    "max_episode_steps": int(self._time_limit),
                    "per_env": None if self._time_limit_per_env is None else self._time_limit_per_env.detach().cpu().clone(),
                    "stats": {k: v.detach().cpu().clone() for k, v in self._episodes.items()}},
                # built-in controller: its gains
                "controller": None if self._ctrl is None else dict(self._ctrl),
                # drive randomisation: the settings and the four live tensors
                "drive_randomization": None if self._drive is None else {
                    k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else (dict(v) if isinstance(v, dict) else v))
                    for k, v in self._drive.items()}}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        if int(sd["num_envs"]) != self.num_envs:
            raise ValueError(f"state_dict of {sd['num_envs']} envs, this batch has {self.num_envs}")
        for name, dst in (("state", self.state), ("out", self.out), ("aux", self._aux)):
            for k, v in sd[name].items():
                if tuple(v.shape) != tuple(dst[k].shape):
                    raise ValueError(f"{name}[{k!r}]: shape {tuple(v.shape)} does not fit {tuple(dst[k].shape)} (other config?)")
                dst[k].copy_(v)
        self.term_counters.copy_(sd["term_counters"])
        for i, st in enumerate(sd["rng"]):
            if st is None:
                self._rngs[i] = None
            else:
                g = np.random.Generator(np.random.PCG64())
                g.bit_generator.state = st
                self._rngs[i] = g
        self._was_reset = bool(sd["was_reset"])
        cpe = sd.get("car_per_env")
        if cpe is None:
            if self._car_rows is not None:
                self._set_car_rows(None)
        else:
            rows = cpe["rows"]
            if tuple(rows.shape) != (self.num_envs, nat.CAR_NP):
                raise ValueError(f"car_per_env rows: shape {tuple(rows.shape)} does not fit ({self.num_envs}, {nat.CAR_NP})")
            self._set_car_rows(rows)
            rnd = cpe.get("randomization")
            if rnd is not None:
                self.randomize_cars(None)  # (allocates the counters)
                with torch.cuda.device(self.device):
                    self._car_episode.copy_(cpe["episode"])
                    self._push_car_rand(rnd["lo"], rnd["hi"], rnd["mask"], rnd["seed"], rnd["env_offset"])
                self._car_rand = dict(rnd)
        eps = sd.get("episodes")  # (absent in older checkpoints: off)
        if eps is None:
            if self._episodes is not None:
                self.track_episodes(False)
        else:
            self.set_time_limit(int(eps["max_episode_steps"]), per_env=eps.get("per_env"))
            for k, v in eps["stats"].items():
                self._episodes[k].copy_(v)
        ctl = sd.get("controller")  # (absent in older checkpoints: off)
        if ctl is None:
            self.set_controller(None)
        else:
            self.set_controller(k=ctl["k"], speed=ctl["speed"])
        drv = sd.get("drive_randomization")  # (absent in older checkpoints: off)
        if drv is None or ctl is None:
            self.randomize_drive()
        else:
            ou = drv["ou"]
            self.randomize_drive(maneuvers=drv["maneuvers"] or None, mode=drv["mode"], ou=None if ou is None else dict(ou),
                                 seed=drv["seed"], env_offset=drv["env_offset"])
            for k in ("maneuver", "episode", "ou_state", "ou_draws"):
                self._drive[k].copy_(drv[k])
        bank = sd.get("camera_bank")  # (present only when a bank was installed)
        if bank is None:
            if self._cam_bank is not None:
                self._set_camera_bank(None)
        else:
            self._set_camera_bank({"E": bank["E"].numpy(), "K": bank["K"].numpy(), "params": bank["params"],
                                       "seed": bank["seed"], "env_offset": bank["env_offset"]},
                                      index=bank["index"], episode=bank["episode"])
        self._step_serial += 1

    def request_reset(self, mask: torch.Tensor) -> None:
        """Marks envs for re-spawning at the start of the next autoreset step, in addition to the ones the engine
        flagged itself (terminated | truncated).  Torch-side termination wrappers call this with their result;
        fused terms do it inside the kernel."""
        if self.autoreset:
            self._aux["needs_reset"] |= mask.to(torch.uint8)

    def _note_fresh(self) -> None:
        """before a step: the envs this step is going to re-spawn (only kept when a torch-side wrapper asked)"""
        self.last_fresh = self._aux["needs_reset"].bool() if (self.track_fresh and self.autoreset) else None

    def profile(self, every: int = 1) -> None:
        """Record HIP events around the two kernels of every `every`-th step (ring of the last 64 samples); 0 = off."""
        with torch.cuda.device(self.device):  # the events must belong to the device whose stream records them
            nat.check(nat.lib().tc_env_profile(self._h, int(every)), "tc_env_profile")

    def profile_read(self) -> Dict[str, float]:
        a, b, n = C.c_double(), C.c_double(), C.c_int32()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_env_profile_read(self._h, C.byref(a), C.byref(b), C.byref(n)), "tc_env_profile_read")
        return {"simulate_us": a.value, "raster_us": b.value, "launches": n.value}

    def render_current(self) -> None:
        """Camera.capture_frame of the current state into self.out["obs"], no step (camera.py:52)."""
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_render(self._h, 0, self._stream()), "tc_render")

    def render_segments(self, segments: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
        """Renderer.render_camera_frame_{rgb,classes} (renderer.py:36-51) for caller-provided int32 segment lists:
        segments [N, cap, 5] rows (layer, x0, y0, x1, y1), counts [N].  Returns the observation tensor."""
        seg = self._to_dev("segments", segments, torch.int32, (self.num_envs, segments.shape[1], 5))
        cnt = self._to_dev("counts", counts, torch.int32, (self.num_envs,))
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_render_segments(self._h, seg.data_ptr(), cnt.data_ptr(), int(seg.shape[1]),
                                                   self._stream()), "tc_render_segments")
        self._keep = (seg, cnt)
        return self.out["obs"]

    # ------------------------------------------------------------------ deferred frames
    def reserve_poses(self, max_frames: int) -> None:
        """Sizes the library's scratch of deferred frames (tc_env_reserve_poses) for launches of up to `max_frames` frames; a
        longer list runs as several launches.  `render_poses` calls this with min(M, 8192) on first use when nothing is reserved
        yet; call it yourself before capturing a `render_poses` into a HIP graph -- the call itself never allocates."""
        if int(max_frames) < 1:
            raise ValueError("max_frames must be at least 1")
        if int(max_frames) > self._reserved_poses:
            with torch.cuda.device(self.device):
                nat.check(nat.lib().tc_env_reserve_poses(self._h, int(max_frames)), "tc_env_reserve_poses")
            self._reserved_poses = int(max_frames)

    def render_poses(self, x: torch.Tensor, y: torch.Tensor, theta: torch.Tensor, camera: Optional[torch.Tensor] = None,
                     index: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Observations drawn from stored poses on the device (tc_render_poses) -> uint8 [M, *obs_shape]: frame m is what
        the camera sees from a car at element ``index[m]`` (or m) of the flattened ``x, y, theta`` -- float64 device tensors
        of equal numel and any shape, for instance the x / y / theta rows of a rollout -- bit for bit the frame the call that
        produced the poses drew or would have drawn.  The env's state, `self.out` and every later call are untouched.

        camera: int32, same numel; not allowed with the one shared camera, required with per-env cameras (`set_env_cameras`:
        the env whose camera the frame takes) and with a bank (`randomize_cameras`: the bank index, rollout["camera"]).
        index: int64 over the flattened tensors (the convention of ``unpack_obs(..., index=)``), repeats and any order
        allowed; a value outside [0, numel) is clamped.  out: reused when given.  With ``obs_packing="bits"`` the frames are
        packed [M, C, H, W/8] and feed `unpack_obs`.  The frames are noise-free: the fused noise of `set_noise` is not
        applied (a deferred frame has no place in the blob stream)."""
        ts = {"x": x, "y": y, "theta": theta}
        for k, t in ts.items():
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self.device:
                raise ValueError(f"{k} must be a float64 tensor on {self.device}")
        n_src = int(x.numel())
        if n_src < 1 or int(y.numel()) != n_src or int(theta.numel()) != n_src:
            raise ValueError(f"x, y and theta must have the same, non-zero number of elements, got {int(x.numel())}, {int(y.numel())}, {int(theta.numel())}")
        rows = self._cam_bank is not None or self._env_cams is not None
        if camera is not None and not rows:
            raise ValueError("camera= needs per-env cameras (set_env_cameras) or a bank (randomize_cameras): this env has the one shared camera")
        if camera is None and rows:
            raise ValueError("camera= is required: " + ("the bank index of every pose (rollout['camera'])" if self._cam_bank is not None
                                                         else "the env whose camera every pose takes"))
        if camera is not None and (not isinstance(camera, torch.Tensor) or camera.dtype != torch.int32 or camera.device != self.device
                                   or int(camera.numel()) != n_src):
            raise ValueError(f"camera must be an int32 tensor of {n_src} elements on {self.device}")
        if index is not None and (not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.device != self.device):
            raise ValueError(f"index must be an int64 tensor on {self.device}")
        M = int(index.numel()) if index is not None else n_src
        shape = (M,) + tuple(self._obs_shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != self.device or tuple(out.shape) != shape \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on {self.device}")
        if M == 0:
            return out
        if self._reserved_poses == 0:  # (a scratch somebody reserved is kept: a longer list runs as several launches)
            self.reserve_poses(min(M, 8192))
        x, y, theta = (t.contiguous() for t in (x, y, theta))
        cam = camera.contiguous() if camera is not None else None
        idx = index.contiguous() if index is not None else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().tc_render_poses(self._h, x.data_ptr(), y.data_ptr(), theta.data_ptr(),
                                                cam.data_ptr() if cam is not None else None,
                                                idx.data_ptr() if idx is not None else None, n_src, M, out.data_ptr(),
                                                self._stream()), "tc_render_poses")
        return out

    def render_rollout(self, rollout: Dict[str, torch.Tensor], index: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The frames of a K-step call from its ``x, y, theta`` rows (`render_poses`): row k of a rollout is the state step k
        returned, so ``render_rollout(roll)`` equals ``roll["obs"]`` of the same call when no noise is fused -- the frames
        are noise-free.  With a bank the rollout's ``camera`` rows are required; with per-env cameras row (k, n) is drawn with
        env n's camera.  index=None draws all K x N rows -> [K, N, *obs_shape]; else int64 indices over the flattened
        [K * N] rows -> [M, *obs_shape] (a `drive()` without "obs" plus ``render_rollout(roll, index=kept_rows)`` draws only
        what a learner keeps)."""
        need = ("x", "y", "theta") + (("camera",) if self._cam_bank is not None else ())
        missing = [k for k in need if k not in rollout]
        if missing:
            raise ValueError(f"render_rollout needs the rollout rows {missing} (alloc_rollout(K, keys=(..., {', '.join(repr(k) for k in need)})))")
        x = rollout["x"]
        if x.dim() != 2 or int(x.shape[1]) != self.num_envs:
            raise ValueError(f"rollout['x'] must be [K, {self.num_envs}], got {tuple(x.shape)}")
        K = int(x.shape[0])
        camera = None
        if self._cam_bank is not None:
            camera = rollout["camera"]
        elif self._env_cams is not None:
            camera = torch.arange(self.num_envs, dtype=torch.int32, device=self.device).repeat(K)
        if index is not None:
            return self.render_poses(x, rollout["y"], rollout["theta"], camera=camera, index=index, out=out)
        full = (K, self.num_envs) + tuple(self._obs_shape)
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != full or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {full} on {self.device}")
        flat = None if out is None else out.view((K * self.num_envs,) + tuple(self._obs_shape))
        return self.render_poses(x, rollout["y"], rollout["theta"], camera=camera, out=flat).view(full)

    def render(self):
        """rgb_array of the class-agnostic camera view is only available in 'rgb' observation format."""
        if self.render_mode == "rgb_array" and self._fmt == nat.FMT_RGB:
            return self._obs()
        return None

    def close(self) -> None:
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            nat.lib().tc_env_destroy(self._h)
            self._h = None
            self._nmap.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ outputs
    def _obs(self):
        o = self.out["obs"]
        if self.no_observation and self.render_mode is None:
            o = torch.zeros_like(o)  # env.py:81
        return o.cpu().numpy() if self.return_numpy else o

    def _info(self):
        """Batched version of env.py:83-85 as a mapping whose derived entries are computed on first access.

        `cte`, `heading_error`, `orientation`, `status` and the per-layer `laneline_distances` are the engine's own
        output tensors (views, no work).  `position`, `local_path` ([N,4,2], rows past `local_path_len` are 0),
        `local_path_len` and `velocity` (0 while the info is empty, car.py:47-51) each cost a few small torch kernels,
        so they are built when read: a training loop that only looks at the observation and the reward does not pay
        for them on every step (step() was 147 us against 85 us for the bare launch in round 1).  Like every tensor
        the env hands out they show the env's buffers: read them before the next step (a derived entry first read
        after the next step raises) or keep `info.materialize()`.
        With return_numpy=True everything is materialised at once as host arrays."""
        info = LazyInfo(self)
        if self.return_numpy:
            def cv(v):
                return {k: cv(x) for k, x in v.items()} if isinstance(v, dict) else v.cpu().numpy()
            return {k: cv(info[k]) for k in info}
        return info


class PreparedStepMulti:
    """A checked `step_multi` call (`TinyCarloVecEnv.prepare_step_multi`): calling it enqueues tc_step_multi with the
    tensors it was prepared with, on the stream current at that moment."""

    __slots__ = ("env", "_keep", "_args", "_structs", "K")

    def __init__(self, env, car_control, maneuver, rollout, r, rows, K, steer_noise=None):
        self.env = env
        self.K = K
        # the tensors stay alive as long as the call can be issued (steer_noise: `prepare_drive`'s noise rows, car_control None)
        self._keep = (car_control, maneuver, rollout, steer_noise)
        self._structs = (r, rows)  # the tc_rollout and tc_step_rows _args points to
        dt = nat.F32 if car_control is not None and car_control.dtype == torch.float32 else nat.F64
        self._args = (car_control.data_ptr() if car_control is not None else None, dt,
                      maneuver.data_ptr() if maneuver is not None else None, K,
                      C.byref(r) if rollout else None, C.byref(rows) if rows.n_rows else None)

    def __call__(self) -> None:
        env = self.env
        if not env._was_reset:
            raise RuntimeError("step_multi() before reset()")
        if env._h is None:
            raise RuntimeError("the env was closed")
        env._note_fresh()
        dbg = gym_getenv("DEBUG")
        if dbg:
            t_dbg = time.perf_counter()
            env.profile(1)
        a = self._args
        if a[0] is None and env._ctrl is None:
            raise RuntimeError("a drive() call needs the controller it was prepared with (set_controller)")
        if a[2] is None and not env._device_maneuvers:
            raise RuntimeError("a drive(maneuver=None) call needs the device maneuvers it was prepared with (randomize_drive)")
        with contextlib.nullcontext() if torch.cuda.current_device() == env.device.index else torch.cuda.device(env.device):
            rc = nat.lib().tc_step_multi(env._h, *a[:4], env._flags(), a[4], a[5], env._stream())
        if rc != 0:
            nat.check(rc, "tc_step_multi")
        env._keep = self._keep  # (the launches just enqueued read and write them; the library keeps none of their pointers)
        env._step_serial += 1
        if dbg:
            env._debug_print(f"step_multi[{self.K}]", t_dbg)
