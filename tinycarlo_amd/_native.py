"""ctypes binding of libtinycarlo_hip.so (C ABI: include/tinycarlo_hip.h).

There is NO CPU fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
# torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It must be in the
# process BEFORE libtinycarlo_hip.so is loaded so that the library's DT_NEEDED entry resolves to the same
# runtime: device pointers and streams handed over from torch only mean something inside that runtime.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# TINYCARLO_HIP_LIB: load another build of the same library (tools/phase_clock.py uses the instrumented one)
LIB_PATH = os.environ.get("TINYCARLO_HIP_LIB") or os.path.join(_HERE, "libtinycarlo_hip.so")

ABI_VERSION = 7
# per-env car parameter rows (tc_env_set_car_per_env): column order of TC_CAR_*
CAR_NP = 8
CAR_WHEELBASE, CAR_TRACK_WIDTH, CAR_MAX_VELOCITY, CAR_MAX_STEERING_ANGLE = 0, 1, 2, 3
CAR_STEERING_SPEED, CAR_MAX_ACCELERATION, CAR_MAX_DECELERATION, CAR_STEERING_SHIFT = 4, 5, 6, 7
CAR_COLUMNS = ("wheelbase", "track_width", "max_velocity", "max_steering_angle", "steering_speed", "max_acceleration",
               "max_deceleration", "steering_shift")
MAX_TERMS, MAX_LAYERS = 8, 16
FMT_RGB, FMT_CLASSES = 0, 1
FMT_CLASSES_BITS = 2  # TC_FMT_CLASSES_BITS: bit-packed class masks, uint8 [N][C][H][W/8] (tinycarlo_amd/packing.py)
F32, F64 = 0, 1
U8, F16, BF16 = 2, 3, 4  # with F32: the output dtypes of tc_unpack_bits
HAS_PACKED_OBS = 1  # TC_HAS_PACKED_OBS: additive within ABI 6
F_NO_OBSERVATION, F_WRAPPED, F_AUTORESET, F_DEVICE_SPAWN = 1, 2, 4, 8
S_UTURN_NO_EDGE, S_PICK_EMPTY, S_BAD_SPAWN, S_NOT_RESET, S_SPAWN_WRAPPED = 1, 2, 4, 8, 16
S_TIME_LIMIT = 32  # tc_env_set_episodes: the episode reached its time limit in this step
HAS_EPISODES = 1   # TC_HAS_EPISODES: additive within ABI 6
HAS_CONTROLLER = 1  # TC_HAS_CONTROLLER: likewise
CTRL_STANLEY = 1    # TC_CTRL_STANLEY
HAS_CAMERA_BANK = 1  # TC_HAS_CAMERA_BANK: likewise
HAS_DRIVE_RANDOMIZATION = 1  # TC_HAS_DRIVE_RANDOMIZATION: likewise
MAN_DRAW, MAN_CYCLE = 0, 1   # TC_MAN_*: maneuver_mode of tc_drive_randomization
MAX_MANEUVERS = 8
HAS_COLLECT = 1  # TC_HAS_COLLECT: likewise (tc_collect; its descriptor is mirrored in tinycarlo_amd/collect.py)

HAS_HISTORY = 1  # TC_HAS_HISTORY: likewise (tc_collect_link, tc_history_resolve, tc_gather_frames; tinycarlo_amd/collect.py)
PAD_ZERO, PAD_EDGE = 0, 1  # TC_PAD_*
HAS_RENDER_POSES = 1  # TC_HAS_RENDER_POSES: additive within ABI 7 (tc_env_reserve_poses, tc_render_poses)

EXPORTS = ["tc_abi_version", "tc_last_error", "tc_map_create", "tc_map_destroy", "tc_env_create", "tc_env_destroy",
           "tc_env_bind", "tc_env_set_camera", "tc_env_set_camera_per_env", "tc_env_set_camera_bank", "tc_env_set_car", "tc_env_set_car_per_env",
           "tc_env_set_car_randomization", "tc_env_set_episodes", "tc_env_set_controller", "tc_env_set_drive_randomization", "tc_draw_normals", "tc_env_set_terms", "tc_env_set_spawn_table", "tc_env_set_noise", "tc_noise", "tc_env_obs_bytes", "tc_env_lds_bytes", "tc_env_profile",
           "tc_env_profile_read", "tc_reset", "tc_step", "tc_step_multi", "tc_env_reserve_steps", "tc_env_launch_info", "tc_env_frame_lds_info", "tc_env_envg_lds_info", "tc_env_frame_bands", "tc_env_draw_list_stats", "tc_render",
           "tc_render_segments", "tc_unpack_bits", "tc_collect", "tc_collect_scratch_bytes",
           "tc_collect_link", "tc_history_resolve", "tc_gather_frames", "tc_env_reserve_poses", "tc_render_poses"]

_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


class MapDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("node_count", _ip), ("edge_count", _ip), ("nodes", _dp), ("edges", _ip),
                ("colors", _bp), ("lanepath_node_count", C.c_int32), ("lanepath_edge_count", C.c_int32),
                ("lanepath_nodes", _dp), ("lanepath_edges", _ip)]


class CarParamsC(C.Structure):
    _fields_ = [("T", C.c_double), ("wheelbase", C.c_double), ("track_width", C.c_double), ("max_velocity", C.c_double),
                ("max_steering_angle", C.c_double), ("steering_speed", C.c_double), ("max_acceleration", C.c_double),
                ("max_deceleration", C.c_double), ("has_steering_speed", C.c_int32), ("has_max_acceleration", C.c_int32)]


class CameraParamsC(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("E", C.c_double * 12), ("K", C.c_double * 9),
                ("max_range", C.c_double), ("line_thickness", C.c_int32), ("format", C.c_int32)]


class Buffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("x", "y", "theta", "velocity", "steering", "radius", "front_x", "front_y", "local_path", "lp_len",
                 "last_maneuver", "cte", "heading_error", "reward", "terminated", "truncated", "status",
                 "laneline_distances", "nearest_edge", "obs", "needs_reset", "spawn_queue", "spawn_cursor")] + \
               [("spawn_queue_len", C.c_int32)]


class Rollout(C.Structure):  # tc_rollout: per-step outputs of tc_step_multi, each [K][N] (obs [K][N][obs_bytes]) or NULL
    _fields_ = [(n, C.c_void_p) for n in ("obs", "reward", "terminated", "truncated", "cte", "heading_error", "status",
                                          "x", "y", "theta", "velocity", "laneline_distances", "nearest_edge",
                                          "local_path", "lp_len")]


class EpisodeBuffers(C.Structure):  # tc_episode_buffers: device arrays of N, length and ret required
    _fields_ = [(n, C.c_void_p) for n in ("length", "ret", "count", "last_length", "last_return", "length_sum",
                                          "return_sum", "limit")]


class StepRows(C.Structure):  # tc_step_rows: per-step feature rows of ONE tc_step_multi call, each [n_rows][N] or NULL
    _fields_ = [("n_rows", C.c_int32), ("steer_noise_in", C.c_void_p), ("steer_out", C.c_void_p),
                ("maneuver_out", C.c_void_p), ("ou_noise_out", C.c_void_p), ("episode_length_out", C.c_void_p),
                ("episode_return_out", C.c_void_p), ("camera_out", C.c_void_p)]


class ControllerC(C.Structure):  # tc_controller: gains by value, steer_last a device array [N] or NULL
    _fields_ = [("kind", C.c_int32), ("k", C.c_double), ("speed", C.c_double), ("steer_last", C.c_void_p)]


class DriveRandomizationC(C.Structure):  # tc_drive_randomization: settings by value; device arrays of N
    _fields_ = [("seed", C.c_uint64), ("env_offset", C.c_uint32), ("n_maneuvers", C.c_int32), ("maneuvers", C.c_int32 * 8),
                ("maneuver_mode", C.c_int32), ("ou_reset", C.c_int32), ("theta", C.c_double), ("mu", C.c_double),
                ("sigma", C.c_double), ("maneuver", C.c_void_p), ("episode", C.c_void_p), ("ou_state", C.c_void_p),
                ("ou_draws", C.c_void_p)]


class CameraBankC(C.Structure):  # tc_camera_bank: device pointers; index / episode [N]
    _fields_ = [("E", C.c_void_p), ("K", C.c_void_p), ("count", C.c_int32), ("env_offset", C.c_uint32), ("seed", C.c_uint64),
                ("index", C.c_void_p), ("episode", C.c_void_p)]


class TermC(C.Structure):  # tc_term
    _fields_ = [("kind", C.c_int32), ("number_of_steps", C.c_int32), ("layer_mask", C.c_uint32), ("reserved", C.c_int32),
                ("p", C.c_double * 4), ("per_layer", C.c_double * MAX_LAYERS)]


def make_terms(terms):
    """ctypes array of tc_term from tinycarlo_amd.terms.Term objects"""
    arr = (TermC * max(len(terms), 1))()
    for i, t in enumerate(terms):
        arr[i].kind, arr[i].number_of_steps, arr[i].layer_mask = int(t.kind), int(t.number_of_steps), int(t.layer_mask)
        arr[i].p[:] = [float(v) for v in t.p]
        arr[i].per_layer[:] = [float(v) for v in t.per_layer]
    return arr


class NativeError(RuntimeError):
    pass


_lib = None


def lib():
    """Loads libtinycarlo_hip.so; raises NativeError (never falls back) when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                          f"(or `make -C tinycarlo_amd/csrc`); tinycarlo_amd has no CPU fallback")
    try:
        rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(rt):
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeError(f"cannot load {LIB_PATH}: {e}") from e
    for name in EXPORTS:
        if not hasattr(L, name):
            raise NativeError(f"{LIB_PATH} does not export {name}")
    L.tc_abi_version.restype = C.c_int
    L.tc_last_error.restype = C.c_char_p
    L.tc_map_create.argtypes = [C.POINTER(MapDesc), C.POINTER(C.c_void_p)]
    L.tc_map_destroy.argtypes = [C.c_void_p]
    L.tc_env_create.argtypes = [C.c_void_p, C.POINTER(CarParamsC), C.POINTER(CameraParamsC), C.c_int32,
                                C.POINTER(C.c_void_p)]
    L.tc_env_destroy.argtypes = [C.c_void_p]
    L.tc_env_bind.argtypes = [C.c_void_p, C.POINTER(Buffers)]
    L.tc_env_set_camera.argtypes = [C.c_void_p, C.POINTER(CameraParamsC)]
    L.tc_env_set_camera_per_env.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc_env_set_camera_bank.argtypes = [C.c_void_p, C.POINTER(CameraBankC)]
    L.tc_env_set_car.argtypes = [C.c_void_p, C.POINTER(CarParamsC)]
    L.tc_env_set_car_per_env.argtypes = [C.c_void_p, C.c_void_p]
    L.tc_env_set_car_randomization.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
    L.tc_env_set_episodes.argtypes = [C.c_void_p, C.POINTER(EpisodeBuffers), C.c_int32]
    L.tc_env_set_controller.argtypes = [C.c_void_p, C.POINTER(ControllerC)]
    L.tc_env_set_drive_randomization.argtypes = [C.c_void_p, C.POINTER(DriveRandomizationC)]
    L.tc_draw_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int32, _dp]
    L.tc_env_set_terms.argtypes = [C.c_void_p, C.POINTER(TermC), C.c_int32, C.c_void_p]
    L.tc_env_set_spawn_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64]
    L.tc_env_set_noise.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64]
    L.tc_noise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc_env_obs_bytes.restype = C.c_int64
    L.tc_env_obs_bytes.argtypes = [C.c_void_p]
    L.tc_env_lds_bytes.restype = C.c_int64
    L.tc_env_lds_bytes.argtypes = [C.c_void_p]
    L.tc_env_profile.argtypes = [C.c_void_p, C.c_int32]
    L.tc_env_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.tc_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.tc_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.tc_step_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32,
                                C.POINTER(Rollout), C.POINTER(StepRows), C.c_void_p]
    L.tc_env_reserve_steps.argtypes = [C.c_void_p, C.c_int32]
    L.tc_env_draw_list_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int64)]
    L.tc_env_frame_lds_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
    L.tc_env_envg_lds_info.argtypes = [C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 5
    L.tc_env_frame_bands.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 2
    L.tc_env_launch_info.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    L.tc_render.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.tc_render_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.tc_unpack_bits.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_int32, C.c_void_p]
    L.tc_collect_scratch_bytes.restype = C.c_int64
    L.tc_collect_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    L.tc_collect.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc_collect_link.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc_history_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_void_p, C.c_int64, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tc_gather_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                   C.c_int32, C.c_void_p]
    L.tc_env_reserve_poses.argtypes = [C.c_void_p, C.c_int64]
    L.tc_render_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                  C.c_void_p, C.c_void_p]
    if L.tc_abi_version() != ABI_VERSION:
        raise NativeError(f"ABI mismatch: library {L.tc_abi_version()} vs binding {ABI_VERSION}")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().tc_last_error()
        raise NativeError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def make_car_params(p) -> CarParamsC:
    return CarParamsC(p.T, p.wheelbase, p.track_width, p.max_velocity, p.max_steering_angle,
                      p.steering_speed if p.steering_speed is not None else 0.0,
                      p.max_acceleration if p.max_acceleration is not None else 0.0,
                      p.max_deceleration if p.max_deceleration is not None else 0.0,
                      int(p.steering_speed is not None), int(p.max_acceleration is not None))


def make_camera_params(cam, fmt: int) -> CameraParamsC:
    c = CameraParamsC()
    c.height, c.width = int(cam.resolution[0]), int(cam.resolution[1])
    c.E[:] = list(np.asarray(cam.E, dtype=np.float64).reshape(-1))
    c.K[:] = list(np.asarray(cam.K, dtype=np.float64).reshape(-1))
    c.max_range = float(cam.max_range)
    c.line_thickness = int(cam.line_thickness)
    c.format = fmt
    return c


class NativeMap:
    """Owns a tc_map handle (device copy of the map graphs + orientation tables)."""

    def __init__(self, m):
        f = m.flat()
        self._keep = f
        d = MapDesc(len(f["node_count"]), f["node_count"].ctypes.data_as(_ip), f["edge_count"].ctypes.data_as(_ip),
                    f["nodes"].ctypes.data_as(_dp), f["edges"].ctypes.data_as(_ip), f["colors"].ctypes.data_as(_bp),
                    len(f["lp_nodes"]), len(f["lp_edges"]), f["lp_nodes"].ctypes.data_as(_dp),
                    f["lp_edges"].ctypes.data_as(_ip))
        h = C.c_void_p()
        check(lib().tc_map_create(C.byref(d), C.byref(h)), "tc_map_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            lib().tc_map_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
