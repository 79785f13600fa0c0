"""Device sample buffer: the (obs, maneuver, steer) samples of K-step calls, collected on the GPU (``tc_collect``).

The reference's training scripts fill a dataset from the env's steps: ``Xn / Mn / Yn`` in examples/train_stanley_il.py:61-77,
100-110 and ``Replaybuffer.add`` in examples/rl_utils.py:13-30.  A K-step call here returns ``[K, N]`` rollout rows; what sits
between the rows and the dataset is defined by ``collect_reference`` below (plain numpy, the executable definition, as
``pack_bits_reference`` is for the packed layout) and carried out on the device by ``SampleBuffer.collect``:

State per env ``n``: ``pending[n]`` (the env's next row is a re-spawn row), ``age[n]`` (action steps of the running episode),
``last[n]`` (the observation the next action is computed from).  Rows are visited ``k`` outer, ``n`` inner:

1. ``pending[n]``: a re-spawn row (the step after ``terminated | truncated`` applied no action): no sample, ``age[n] = 0``.
2. otherwise ``i = age[n]``, ``age[n] = i + 1``; if ``i % stride == 0`` the row is a *candidate*: ``obs = last[n]``,
   ``next_obs = obs[k, n]``, ``env = n`` and every column's value at ``[k, n]`` -- the frame BEFORE a step with that step's
   command (train_stanley_il.py:69-75).
3. ``pending[n] = terminated[k, n] | truncated[k, n]``, ``last[n] = obs[k, n]``.

Candidates take ordinals ``next_ordinal, next_ordinal + 1, ...`` in visiting order.  Ordinal ``o < capacity`` goes to slot
``o``; beyond that ``overflow="stop"`` drops it (the IL script's BUFFER_SIZE), ``"ring"`` takes ``o % capacity``, ``"random"``
``draw_replace_slot(seed, o, capacity)`` (Replaybuffer.add's random slot, counter-based).  A later ordinal overwrites an
earlier one in the same slot; ``ordinal[slot]`` records what a slot holds (-1 = empty).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

from .randomization import draw_replace_slot

OVERFLOW = {"stop": 0, "ring": 1, "random": 2}  # TC_COLLECT_*
MAX_COLUMNS = 8


# ---------------------------------------------------------------------------------------------- the definition
def reference_state(capacity: int, num_envs: int, frame_shape: Sequence[int], columns: Optional[Mapping[str, Any]] = None,
                    next_obs: bool = False, fill: int = 0) -> Dict[str, Any]:
    """An empty buffer for ``collect_reference``: numpy arrays under the names of ``SampleBuffer``'s tensors plus the per-env
    state and the three counters.  columns: name -> numpy dtype.  ``fill``: the byte every destination starts with."""
    cap, N, shape = int(capacity), int(num_envs), tuple(int(v) for v in frame_shape)

    def dest(shp, dt):
        a = np.empty(shp, dtype=dt)
        a.view(np.uint8).fill(fill)
        return a
    return {"obs": dest((cap,) + shape, np.uint8), "next_obs": dest((cap,) + shape, np.uint8) if next_obs else None,
            "ordinal": np.full(cap, -1, dtype=np.int64), "env": dest(cap, np.int32),
            "cols": {k: dest(cap, np.dtype(dt)) for k, dt in (columns or {}).items()},
            "pending": np.zeros(N, dtype=np.uint8), "age": np.zeros(N, dtype=np.int32), "last": np.zeros((N,) + shape, dtype=np.uint8),
            "count": 0, "next_ordinal": 0, "dropped": 0}


def reference_begin(state: Dict[str, Any], obs, pending=None) -> None:
    """``SampleBuffer.begin`` on a reference state"""
    state["last"][...] = np.asarray(obs, dtype=np.uint8).reshape(state["last"].shape)
    state["pending"][...] = 0 if pending is None else (np.asarray(pending).reshape(-1) != 0)
    state["age"][...] = 0


def collect_reference(state: Dict[str, Any], rows: Mapping[str, Any], stride: int = 1, overflow: str = "stop",
                      seed: int = 0) -> Dict[str, Any]:
    """One call's rows into the buffer, in place; returns ``state``.  rows: ``obs`` ``[K, N, ...]`` uint8, optional
    ``terminated`` / ``truncated`` ``[K, N]``, and ``[K, N]`` arrays under the names of ``state["cols"]``."""
    if overflow not in OVERFLOW:
        raise ValueError(f"overflow must be one of {tuple(OVERFLOW)}")
    if int(stride) < 1:
        raise ValueError("stride must be at least 1")
    obs = np.asarray(rows["obs"])
    K, N = int(obs.shape[0]), int(obs.shape[1])
    cap = len(state["ordinal"])
    if N != len(state["pending"]) or obs.dtype != np.uint8 or obs.shape[2:] != state["last"].shape[1:]:
        raise ValueError("rows['obs'] must be uint8 [K, num_envs] + the buffer's frame shape")
    done = np.zeros((K, N), dtype=bool)
    for key in ("terminated", "truncated"):
        if rows.get(key) is not None:
            done |= np.asarray(rows[key]).reshape(K, N) != 0
    cols = {name: np.asarray(rows[name]).reshape(K, N) for name in state["cols"]}
    pending, age, last = state["pending"], state["age"], state["last"]
    for k in range(K):
        for n in range(N):
            if pending[n]:
                age[n] = 0
            else:
                i = int(age[n])
                age[n] = i + 1
                if i % stride == 0:
                    o = state["next_ordinal"]
                    state["next_ordinal"] = o + 1
                    if o < cap:
                        slot = o
                    elif overflow == "ring":
                        slot = o % cap
                    elif overflow == "random":
                        slot = int(draw_replace_slot(seed, o, cap))
                    else:
                        slot = -1
                        state["dropped"] += 1
                    if slot >= 0:
                        state["obs"][slot] = last[n]
                        if state["next_obs"] is not None:
                            state["next_obs"][slot] = obs[k, n]
                        state["env"][slot] = n
                        state["ordinal"][slot] = o
                        for name, c in cols.items():
                            state["cols"][name][slot] = c[k, n]
                        state["count"] = min(cap, o + 1)
            pending[n] = 1 if done[k, n] else 0
            last[n] = obs[k, n]
    return state


# ---------------------------------------------------------------------------------------------- the device path
class _ColumnC(C.Structure):  # tc_collect_column
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("elem_size", C.c_int32), ("reserved", C.c_int32)]


class CollectDescC(C.Structure):  # tc_collect_desc
    _fields_ = [("capacity", C.c_int64), ("num_envs", C.c_int32), ("stride", C.c_int32), ("mode", C.c_int32),
                ("n_columns", C.c_int32), ("seed", C.c_uint64), ("frame_bytes", C.c_int64), ("obs", C.c_void_p),
                ("next_obs", C.c_void_p), ("ordinal", C.c_void_p), ("env", C.c_void_p), ("columns", _ColumnC * MAX_COLUMNS),
                ("pending", C.c_void_p), ("age", C.c_void_p), ("last", C.c_void_p), ("counters", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


class SampleBuffer:
    """A dataset of ``capacity`` samples on the device, filled from the rollout rows of K-step calls by ``tc_collect``.

    ``obs_shape``: the shape of one uint8 frame as the env produces it (packed ``[C, H, W/8]`` with ``packed=True``, byte class
    masks ``[C, H, W]``, rgb ``[H, W, 3]``); its byte count must be a multiple of 4.  ``columns``: name -> torch dtype of 1, 4
    or 8 bytes per element (at most 8), each a ``[K, N]`` row array of the calls.  ``next_obs``: also keep the frame after the
    step (``X1`` of the replay buffer).  ``stride`` / ``overflow`` / ``seed``: see the module's text.  ``max_rows``: the longest
    call ``collect`` accepts (sizes the scratch once; ``collect`` never allocates).

    Live tensors: ``obs``, ``next_obs``, ``ordinal`` (int64, -1 = empty), ``env`` (int32), ``cols[name]``, ``counters`` (int64
    [4]: filled slots, next ordinal, dropped, candidates of the last call) and the per-env carry ``pending`` / ``age`` /
    ``last``.  Only ``len()``, ``dropped`` and ``full`` synchronise."""

    def __init__(self, capacity: int, num_envs: int, obs_shape: Sequence[int], columns: Optional[Mapping[str, Any]] = None,
                 next_obs: bool = False, stride: int = 1, overflow: str = "stop", seed: int = 0, max_rows: int = 128,
                 device: Any = "cuda:0", packed: bool = False):
        import torch
        from . import _native as nat
        self.capacity, self.num_envs, self.obs_shape = int(capacity), int(num_envs), tuple(int(v) for v in obs_shape)
        self.stride, self.overflow, self.seed, self.max_rows = int(stride), str(overflow), int(seed), int(max_rows)
        self.packed = bool(packed)
        self.device = torch.device(device)
        columns = dict(columns or {})
        if overflow not in OVERFLOW:
            raise ValueError(f"overflow must be one of {tuple(OVERFLOW)}, got {overflow!r}")
        if self.capacity < 1 or self.num_envs < 1 or self.max_rows < 1 or self.stride < 1 or not self.obs_shape:
            raise ValueError("capacity, num_envs, max_rows and stride must be positive and obs_shape not empty")
        if overflow == "random" and self.capacity >= 2 ** 32:
            raise ValueError("overflow='random' needs capacity < 2^32")
        self.frame_bytes = int(np.prod(self.obs_shape, dtype=np.int64))
        if self.frame_bytes < 1 or self.frame_bytes % 4:
            raise ValueError(f"a frame of shape {self.obs_shape} has {self.frame_bytes} bytes: need a positive multiple of 4")
        if len(columns) > MAX_COLUMNS:
            raise ValueError(f"at most {MAX_COLUMNS} columns")
        for name, dt in columns.items():
            if not isinstance(dt, torch.dtype) or torch.empty((), dtype=dt).element_size() not in (1, 4, 8):
                raise ValueError(f"column {name!r}: need a torch dtype of 1, 4 or 8 bytes per element, got {dt!r}")
            if name in ("obs", "terminated", "truncated"):
                raise ValueError(f"{name!r} cannot be a column")
        if self.device.type != "cuda":
            raise ValueError("SampleBuffer lives on the GPU (collect_reference is the CPU definition)")
        self._nat = nat
        dev, cap, N = self.device, self.capacity, self.num_envs
        self.obs = torch.zeros((cap,) + self.obs_shape, dtype=torch.uint8, device=dev)
        self.next_obs = torch.zeros((cap,) + self.obs_shape, dtype=torch.uint8, device=dev) if next_obs else None
        self.ordinal = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        self.env = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.cols = {name: torch.zeros(cap, dtype=dt, device=dev) for name, dt in columns.items()}
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)
        self.pending = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.age = torch.zeros(N, dtype=torch.int32, device=dev)
        self.last = torch.zeros((N,) + self.obs_shape, dtype=torch.uint8, device=dev)
        nbytes = int(nat.lib().tc_collect_scratch_bytes(self.max_rows, N))
        self._scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        d = self._desc = CollectDescC()
        d.capacity, d.num_envs, d.stride, d.mode, d.n_columns = cap, N, self.stride, OVERFLOW[overflow], len(columns)
        d.seed, d.frame_bytes = self.seed & 0xFFFFFFFFFFFFFFFF, self.frame_bytes
        d.obs, d.next_obs = self.obs.data_ptr(), (self.next_obs.data_ptr() if next_obs else None)
        d.ordinal, d.env = self.ordinal.data_ptr(), self.env.data_ptr()
        for j, (name, t) in enumerate(self.cols.items()):
            d.columns[j].dst, d.columns[j].elem_size = t.data_ptr(), t.element_size()
        d.pending, d.age, d.last = self.pending.data_ptr(), self.age.data_ptr(), self.last.data_ptr()
        d.counters, d.scratch, d.scratch_bytes = self.counters.data_ptr(), self._scratch.data_ptr(), nbytes

    # ---- filling
    def begin(self, obs, pending=None) -> None:
        """Start of the data: ``obs`` ``[N, ...]`` is the observation the first action is computed from (what ``reset()``
        returned), ``pending`` ``[N]`` marks envs whose next row is a re-spawn row (default: none); ``age = 0``."""
        import torch
        obs = torch.as_tensor(obs, device=self.device)
        if obs.dtype != torch.uint8 or tuple(obs.shape) != tuple(self.last.shape):
            raise ValueError(f"obs must be uint8 of shape {tuple(self.last.shape)}")
        self.last.copy_(obs)
        if pending is None:
            self.pending.zero_()
        else:
            self.pending.copy_((torch.as_tensor(pending, device=self.device).reshape(self.num_envs) != 0).to(torch.uint8))
        self.age.zero_()

    def collect(self, rollout: Mapping[str, Any], columns: Optional[Mapping[str, Any]] = None) -> None:
        """The rows of one K-step call into the buffer, on the current stream: ``rollout["obs"]`` ``[K, N, ...]``, its
        ``terminated`` / ``truncated`` ``[K, N]`` where present, and every column from ``columns`` (name -> ``[K, N]`` tensor)
        or else from the rollout.  Neither allocates nor synchronises; can be captured into a graph."""
        import torch
        obs = rollout["obs"]
        K = int(obs.shape[0])
        if K > self.max_rows:
            raise ValueError(f"a call of {K} rows exceeds max_rows = {self.max_rows}")
        if K < 1 or obs.dtype != torch.uint8 or tuple(obs.shape[1:]) != tuple(self.last.shape) or obs.device != self.device \
                or not obs.is_contiguous():
            raise ValueError(f"rollout['obs'] must be a contiguous uint8 tensor [K, {self.num_envs}] + {self.obs_shape} on {self.device}")
        done = []
        for key in ("terminated", "truncated"):
            t = rollout.get(key)
            if t is not None and (t.dtype not in (torch.uint8, torch.bool) or tuple(t.shape) != (K, self.num_envs)
                                  or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"rollout[{key!r}] must be a contiguous uint8 tensor [{K}, {self.num_envs}] on {self.device}")
            done.append(t.data_ptr() if t is not None else None)
        d = self._desc
        for j, (name, dst) in enumerate(self.cols.items()):
            src = columns[name] if columns is not None and name in columns else rollout.get(name)
            if src is None:
                raise ValueError(f"column {name!r} is neither in `columns` nor in the rollout")
            if src.dtype != dst.dtype or tuple(src.shape) != (K, self.num_envs) or src.device != self.device or not src.is_contiguous():
                raise ValueError(f"column {name!r} must be a contiguous {dst.dtype} tensor [{K}, {self.num_envs}] on {self.device}")
            d.columns[j].src = src.data_ptr()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._nat.check(self._nat.lib().tc_collect(C.byref(d), K, obs.data_ptr(), done[0], done[1], stream), "tc_collect")

    # ---- reading (these three synchronise)
    def __len__(self) -> int:
        return int(self.counters[0])

    @property
    def dropped(self) -> int:
        return int(self.counters[2])

    @property
    def full(self) -> bool:
        return len(self) >= self.capacity

    # ---- sampling
    def sample_index(self, batch: int, generator=None):
        """int64 ``[batch]`` uniform over the filled slots, without a host sync: device uniforms scaled by the device's count
        (an empty buffer gives zeros)."""
        import torch
        u = torch.rand(int(batch), dtype=torch.float64, device=self.device, generator=generator)
        n = self.counters[0]
        return torch.minimum((u * n).to(torch.int64), (n - 1).clamp(min=0))

    def sample(self, index, dtype=None) -> Dict[str, Any]:
        """The samples at ``index`` (int64 ``[B]`` on the device): ``obs`` (and ``next_obs``) as ``dtype`` (default float32)
        -- packed frames through ``unpack_obs`` (0.0 / 1.0, or 0 / 255 for uint8), byte frames as an indexed copy scaled by
        1 / 255 for float dtypes -- plus ``env``, ``ordinal`` and every column at ``index``."""
        import torch
        dtype = torch.float32 if dtype is None else dtype

        def frames(t):
            if self.packed:
                from .packing import unpack_obs
                return unpack_obs(t, dtype, index=index)
            f = t.index_select(0, index)
            return f if dtype == torch.uint8 else f.to(dtype) / 255
        out = {"obs": frames(self.obs), "env": self.env.index_select(0, index), "ordinal": self.ordinal.index_select(0, index)}
        if self.next_obs is not None:
            out["next_obs"] = frames(self.next_obs)
        for name, t in self.cols.items():
            out[name] = t.index_select(0, index)
        return out

    # ---- checkpoints
    _TENSORS = ("obs", "next_obs", "ordinal", "env", "counters", "pending", "age", "last")

    def state_dict(self) -> Dict[str, Any]:
        sd = {k: getattr(self, k).cpu().clone() for k in self._TENSORS if getattr(self, k) is not None}
        sd["cols"] = {k: t.cpu().clone() for k, t in self.cols.items()}
        sd["config"] = {"capacity": self.capacity, "num_envs": self.num_envs, "obs_shape": self.obs_shape, "stride": self.stride,
                        "overflow": self.overflow, "seed": self.seed, "packed": self.packed}
        return sd

    def load_state_dict(self, sd: Mapping[str, Any]) -> None:
        cfg = sd["config"]
        for k in ("capacity", "num_envs", "stride", "overflow", "seed"):
            if cfg[k] != getattr(self, k):
                raise ValueError(f"state_dict was taken from a buffer with {k} = {cfg[k]!r}, this one has {getattr(self, k)!r}")
        if tuple(cfg["obs_shape"]) != self.obs_shape or set(sd["cols"]) != set(self.cols) or ("next_obs" in sd) != (self.next_obs is not None):
            raise ValueError("state_dict does not match this buffer's frames / columns")
        for k in self._TENSORS:
            if getattr(self, k) is not None:
                getattr(self, k).copy_(sd[k])
        for k, t in self.cols.items():
            t.copy_(sd["cols"][k])
