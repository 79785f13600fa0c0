"""Per-env car constants and per-episode cameras: the device's draws restated on the host.

The device draws the row of an env's next episode at every re-spawn (``tc_env_set_car_randomization``,
``csrc/tc_rng.h``: ``tc_car_stream`` / ``tc_car_draw``).  ``draw_car_params`` is the same arithmetic in numpy uint64 /
float64, so the constants of any past episode can be recomputed on the host -- and tests use it as the check.

The other two helpers turn the user-facing arguments of ``TinyCarloVecEnv.set_env_cars`` / ``randomize_cars`` into
the library's [N, 8] rows and (lo, hi, mask) tables, with the validation both need (no GPU involved).

Cameras (``TinyCarloVecEnv.randomize_cameras``, ``tc_env_set_camera_bank``): ``camera_bank`` builds the bank -- every
combination of the candidate values, each camera computed by ``Camera`` exactly as ``update_params`` does -- and
``draw_camera_index`` is ``tc_camera_index`` of ``csrc/tc_rng.h``: which camera of the bank an env's episode uses.

Drive randomisation (``TinyCarloVecEnv.randomize_drive``, ``tc_env_set_drive_randomization``): ``draw_maneuver`` is the
maneuver of an env's episode (``tc_maneuver_index``, or the cycle), ``draw_normal`` the env's normal numbers
(``tc_normal_at``, evaluated by the library's host export ``tc_draw_normals``: its logarithm and cosine are the portable
ones of ``csrc/tc_trig.h``, which numpy's are not bit for bit) and ``ou_step`` one step of the Ornstein-Uhlenbeck process.
"""
from __future__ import annotations

import itertools
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

CAR_COLUMNS = ("wheelbase", "track_width", "max_velocity", "max_steering_angle", "steering_speed", "max_acceleration",
               "max_deceleration", "steering_shift")
CAR_NP = len(CAR_COLUMNS)
CAR_STREAM = 0x636172  # "car": the sub-stream of the seed the draws come from (apart from the device spawn stream)
CAM_STREAM = 0x63616D  # "cam": likewise for the camera index of an episode
MAN_STREAM = 0x6D616E  # "man": likewise for the maneuver of an episode
OU_STREAM = 0x6F75      # "ou": likewise for the normal numbers of the steering noise
REP_STREAM = 0x726570   # "rep": likewise for the slot a sample replaces in a full sample buffer (overflow="random")
CAMERA_COLUMNS = ("pitch", "roll", "yaw", "fov", "x", "y", "z")  # columns of a camera bank's parameter table
_GOLDEN, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def splitmix64_at(seed, n):
    """output n of the SplitMix64 sequence started at `seed` (tc_rng.h: tc_splitmix64_at), elementwise on uint64"""
    with np.errstate(over="ignore"):
        z = np.asarray(seed, dtype=np.uint64) + (np.asarray(n, dtype=np.uint64) + np.uint64(1)) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def draw_car_params(seed: int, env_index, episode, lo, hi, mask: int = (1 << CAR_NP) - 1, base=None) -> np.ndarray:
    """The row env `env_index` (global index: env_offset + index in the batch) draws for episode `episode` (its value
    of the episode counter at the re-spawn).  env_index / episode may be arrays (broadcast); returns float64
    [..., 8].  Columns outside `mask` are taken from `base` ([8] or [..., 8]; NaN when not given)."""
    env = np.asarray(env_index, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ep = np.asarray(episode, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    env, ep = np.broadcast_arrays(env, ep)
    s2 = splitmix64_at(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), np.uint64(CAR_STREAM))
    z = splitmix64_at(s2, (env << np.uint64(32)) | ep)
    lo = np.asarray(lo, dtype=np.float64).reshape(CAR_NP)
    hi = np.asarray(hi, dtype=np.float64).reshape(CAR_NP)
    out = np.full(env.shape + (CAR_NP,), np.nan) if base is None else \
        np.array(np.broadcast_to(np.asarray(base, dtype=np.float64), env.shape + (CAR_NP,)))
    for j in range(CAR_NP):
        if (int(mask) >> j) & 1:
            u = (splitmix64_at(z, np.uint64(j)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
            out[..., j] = lo[j] + (hi[j] - lo[j]) * u
    return out


def config_row(p) -> np.ndarray:
    """[8] row of a CarParams (absent optional constants as 0, steering shift 0)"""
    return np.array([p.wheelbase, p.track_width, p.max_velocity, p.max_steering_angle,
                     p.steering_speed if p.steering_speed is not None else 0.0,
                     p.max_acceleration if p.max_acceleration is not None else 0.0,
                     p.max_deceleration if p.max_deceleration is not None else 0.0, 0.0], dtype=np.float64)


def _absent(p) -> set:
    a = set()
    if p.steering_speed is None:
        a.add("steering_speed")
    if p.max_acceleration is None:
        a |= {"max_acceleration", "max_deceleration"}
    return a


def car_rows(p, num_envs: int, values: Dict[str, object]) -> np.ndarray:
    """[num_envs, 8] rows from the config's car `p` and per-column overrides (a scalar or an [num_envs] sequence /
    tensor each; None = the config value, shift 0).  Raises ValueError on unknown names, wrong lengths, non-finite
    values, non-positive constants (the shift may be any finite number) and values for constants the config lacks."""
    rows = np.tile(config_row(p), (num_envs, 1))
    absent = _absent(p)
    for name, v in values.items():
        if name not in CAR_COLUMNS:
            raise ValueError(f"unknown car parameter {name!r}; choose from {CAR_COLUMNS}")
        if v is None:
            continue
        if name in absent:
            raise ValueError(f"car.{name} is not set in the config: the kernel has no such limit to vary")
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        a = np.asarray(v, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != num_envs):
            raise ValueError(f"{name}: expected a scalar or {num_envs} values, got shape {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{name}: values must be finite")
        if name != "steering_shift" and not np.all(a > 0):
            raise ValueError(f"{name}: values must be positive")
        rows[:, CAR_COLUMNS.index(name)] = a
    return rows


def car_ranges(p, ranges: Optional[Dict[str, Sequence[float]]]) -> Tuple[np.ndarray, np.ndarray, int]:
    """(lo[8], hi[8], column mask) of `ranges` = {name: (lo, hi)}; None or {} = no resampling (mask 0)."""
    lo, hi = np.zeros(CAR_NP), np.zeros(CAR_NP)
    mask = 0
    absent = _absent(p)
    for name, r in (ranges or {}).items():
        if name not in CAR_COLUMNS:
            raise ValueError(f"unknown car parameter {name!r}; choose from {CAR_COLUMNS}")
        if name in absent:
            raise ValueError(f"car.{name} is not set in the config: no range can be drawn for it")
        r = np.asarray(r, dtype=np.float64).reshape(-1)
        if r.shape != (2,):
            raise ValueError(f"{name}: a range is (lo, hi), got {r.size} values")
        if not np.all(np.isfinite(r)) or r[0] > r[1]:
            raise ValueError(f"{name}: range must be finite with lo <= hi, got ({r[0]}, {r[1]})")
        if name != "steering_shift" and r[0] <= 0:
            raise ValueError(f"{name}: range must be positive, got ({r[0]}, {r[1]})")
        j = CAR_COLUMNS.index(name)
        lo[j], hi[j] = r
        mask |= 1 << j
    return lo, hi, mask



# ---------------------------------------------------------------------------------------------- camera bank
def draw_camera_index(seed: int, env_index, episode, count: int):
    """The index into a bank of `count` cameras that env `env_index` (global index: env_offset + index in the batch) draws
    for episode `episode` (its value of the camera episode counter at the re-spawn): tc_rng.h's tc_camera_index.
    env_index / episode may be arrays (broadcast; an int32 counter that wrapped gives the draw of its unsigned value);
    returns int64 of the broadcast shape."""
    count = int(count)
    if not 1 <= count <= 2 ** 31:
        raise ValueError(f"count must be in [1, 2^31], got {count}")
    env = np.asarray(env_index, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ep = np.asarray(episode, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    env, ep = np.broadcast_arrays(env, ep)
    s2 = splitmix64_at(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), np.uint64(CAM_STREAM))
    z = splitmix64_at(s2, (env << np.uint64(32)) | ep)
    return (((z >> np.uint64(32)) * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def _values(name: str, v, width: int) -> np.ndarray:
    """candidate values of one camera component as float64 [n, width] (width 1: scalars)"""
    a = np.asarray(list(v) if not hasattr(v, "shape") else v, dtype=np.float64)
    if a.size == 0:
        raise ValueError(f"{name}: the list of candidate values is empty")
    a = a.reshape(-1, 1) if (width == 1 and a.ndim == 1) else a
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{name}: expected a list of " + ("numbers" if width == 1 else f"{width}-vectors") + f", got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: values must be finite")
    return a


def bank_camera_config(camera_cfg: Dict[str, Any], row) -> Dict[str, Any]:
    """the camera config of one row (CAMERA_COLUMNS) of a bank's parameter table"""
    r = [float(x) for x in np.asarray(row, dtype=np.float64).reshape(len(CAMERA_COLUMNS))]
    cfg = dict(camera_cfg)
    cfg.update(orientation=r[0:3], fov=r[3], position=r[4:7])
    return cfg


def camera_bank(camera_cfg: Dict[str, Any], orientation=None, fov=None, position=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(E [M, 12], K [M, 9], params [M, 7]) of the bank made of every combination of the candidate values.

    orientation: a list of (pitch, roll, yaw) triples in degrees, or a dict {"pitch": [...], "roll": [...], "yaw": [...]}
    of per-angle candidates (a missing angle keeps the config's value); fov: a list of degrees; position: a list of
    (x, y, z) triples in metres.  None keeps the config's value.  Rows are ordered orientation-major (pitch, roll, yaw),
    then fov, then position; row m is ``Camera(bank_camera_config(camera_cfg, params[m])).E / .K`` bit for bit.
    Raises ValueError on an empty list, a non-finite value or an unknown angle name."""
    from .camera import Camera
    base = Camera(camera_cfg)
    if isinstance(orientation, dict):
        names = ("pitch", "roll", "yaw")
        for k in orientation:
            if k not in names:
                raise ValueError(f"unknown orientation component {k!r}; choose from {names}")
        comps = [_values(f"orientation[{n!r}]", orientation[n], 1)[:, 0] if orientation.get(n) is not None
                 else np.array([float(base.orientation[i])]) for i, n in enumerate(names)]
        ori = np.array(list(itertools.product(*comps)), dtype=np.float64).reshape(-1, 3)
    elif orientation is None:
        ori = np.array([base.orientation], dtype=np.float64)
    else:
        ori = _values("orientation", orientation, 3)
    fv = np.array([[float(base.fov)]]) if fov is None else _values("fov", fov, 1)
    pos = np.array([base.position], dtype=np.float64) if position is None else _values("position", position, 3)
    if np.any(fv <= 0) or np.any(fv >= 180):
        raise ValueError("fov: values must be in (0, 180) degrees")
    M = ori.shape[0] * fv.shape[0] * pos.shape[0]
    if M > 2 ** 31:
        raise ValueError(f"a bank of {M} cameras is too large")
    params = np.empty((M, len(CAMERA_COLUMNS)), dtype=np.float64)
    E, K = np.empty((M, 12), dtype=np.float64), np.empty((M, 9), dtype=np.float64)
    for m, (o, f, p) in enumerate(itertools.product(ori, fv[:, 0], pos)):
        params[m, 0:3], params[m, 3], params[m, 4:7] = o, f, p
        c = Camera(bank_camera_config(camera_cfg, params[m]))
        E[m], K[m] = c.E.reshape(-1), c.K.reshape(-1)
    return E, K, params


def draw_maneuver(seed: int, env_index, episode, candidates: Sequence[int], mode: str = "draw") -> np.ndarray:
    """The maneuver env `env_index` (global index) takes for episode `episode` (its value of the episode counter at the
    re-spawn) from `candidates` (``tc_env_set_drive_randomization``): ``"draw"`` -- candidate number ``tc_maneuver_index`` of
    ``csrc/tc_rng.h`` -- or ``"cycle"`` -- number (env_index + episode) mod len(candidates), the ``maneuver = (maneuver + 1) % 3``
    of examples/train_stanley_il.py:105.  env_index / episode may be arrays (broadcast); returns int32."""
    cand = np.asarray([int(c) for c in candidates], dtype=np.int32)
    if cand.size < 1:
        raise ValueError("draw_maneuver needs at least one candidate")
    env = np.asarray(env_index, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ep = np.asarray(episode, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    env, ep = np.broadcast_arrays(env, ep)
    if mode == "cycle":
        idx = ((env + ep) & np.uint64(0xFFFFFFFF)) % np.uint64(cand.size)
    elif mode == "draw":
        s2 = splitmix64_at(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), np.uint64(MAN_STREAM))
        z = splitmix64_at(s2, (env << np.uint64(32)) | ep)
        idx = ((z >> np.uint64(32)) * np.uint64(cand.size)) >> np.uint64(32)
    else:
        raise ValueError(f"mode must be 'draw' or 'cycle', got {mode!r}")
    return cand[idx.astype(np.int64)]


def draw_normal(seed: int, env_index: int, draw: int, n: Optional[int] = None):
    """Normal number `draw` of env `env_index` (global index): ``tc_normal_at`` of ``csrc/tc_rng.h``, evaluated on the host by
    the library (``tc_draw_normals``; no device needed).  With `n`: the float64 array of numbers draw .. draw + n - 1."""
    import ctypes as C

    from . import _native as nat
    out = np.empty(1 if n is None else int(n), dtype=np.float64)
    nat.check(nat.lib().tc_draw_normals(int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_index) & 0xFFFFFFFF, int(draw) & 0x7FFFFFFF,
                                        out.size, out.ctypes.data_as(C.POINTER(C.c_double))), "tc_draw_normals")
    return float(out[0]) if n is None else out


def ou_step(n, eps, theta: float, mu: float, sigma: float):
    """``noise += THETA * (MEAN - noise) + SIGMA * randn`` in the expression's order (``tc_ou_step``): float64, no fusing"""
    n, eps = np.float64(n), np.float64(eps)
    return n + (np.float64(theta) * (np.float64(mu) - n) + np.float64(sigma) * eps)


# ---------------------------------------------------------------------------------------------- sample buffer
def draw_replace_slot(seed: int, ordinal, capacity: int):
    """The slot of a full sample buffer of `capacity` slots that the candidate with ordinal `ordinal` replaces
    (``SampleBuffer(overflow="random")``): tc_rng.h's tc_replace_slot -- Replaybuffer.add's np.random.randint(0, size) of the
    reference's examples/rl_utils.py:20 as a counter-based draw.  ordinal may be an array; returns int64 of its shape."""
    capacity = int(capacity)
    if not 1 <= capacity < 2 ** 32:
        raise ValueError(f"capacity must be in [1, 2^32), got {capacity}")
    o = np.asarray(ordinal, dtype=np.int64).astype(np.uint64)
    s2 = splitmix64_at(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), np.uint64(REP_STREAM))
    z = splitmix64_at(s2, o)
    return (((z >> np.uint64(32)) * np.uint64(capacity)) >> np.uint64(32)).astype(np.int64)
