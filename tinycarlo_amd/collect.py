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

Frame histories (``history=T``): a sample of the reference's ``ReplaybufferTemporal`` (examples/rl_utils.py:32-57) is what
the env showed over the last ``SEQ_LEN`` steps of the episode, newest first (``x = feature_vec_queue[1:]``, ``x1 =
feature_vec_queue[:-1]``, examples/train_td3.py:164,175-176,196-198).  The buffer keeps one frame per slot and one link:
per env ``chain[n]``, the ordinal of the env's most recent candidate of the running episode (-1: none), and per slot
``prev[slot]``, the ordinal of the sample that precedes this one in its episode (-1: none).  ``begin()`` and rule 1 set
``chain[n] = -1``; rule 2 takes ``link = chain[n]`` and sets ``chain[n] = o`` whether or not ``o`` is written, and where
``o`` is written to ``slot``, ``prev[slot] = link``.  Steps skipped by ``stride`` do not touch ``chain``: a history is the
env's every ``stride``-th step, as the dataset is.  ``history_reference`` resolves a history: ``slots[b, 0] = index[b]``,
``slots[b, t] = slot(prev[slots[b, t - 1]])`` as long as the link is not -1 (the episode started) and the slot still holds
that ordinal (else the predecessor was dropped or overwritten); ``valid[b]`` entries are found, the rest is -1
(``pad="zero"``: zero frames) or the last slot found (``pad="edge"``).  ``next_obs[b, 0]`` is the slot's next frame and
``next_obs[b, t] = obs[b, t - 1]``.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

from .randomization import draw_replace_slot

OVERFLOW = {"stop": 0, "ring": 1, "random": 2}  # TC_COLLECT_*
PAD = {"zero": 0, "edge": 1}                     # TC_PAD_*
MAX_COLUMNS = 8


# ---------------------------------------------------------------------------------------------- the definition
def reference_state(capacity: int, num_envs: int, frame_shape: Sequence[int], columns: Optional[Mapping[str, Any]] = None,
                    next_obs: bool = False, fill: int = 0, history: bool = False) -> Dict[str, Any]:
    """An empty buffer for ``collect_reference``: numpy arrays under the names of ``SampleBuffer``'s tensors plus the per-env
    state and the three counters.  columns: name -> numpy dtype.  ``fill``: the byte every destination starts with.
    ``history``: also the links ``prev`` (per slot) and ``chain`` (per env), both -1."""
    cap, N, shape = int(capacity), int(num_envs), tuple(int(v) for v in frame_shape)

    def dest(shp, dt):
        a = np.empty(shp, dtype=dt)
        a.view(np.uint8).fill(fill)
        return a
    st = {"obs": dest((cap,) + shape, np.uint8), "next_obs": dest((cap,) + shape, np.uint8) if next_obs else None,
            "ordinal": np.full(cap, -1, dtype=np.int64), "env": dest(cap, np.int32),
            "cols": {k: dest(cap, np.dtype(dt)) for k, dt in (columns or {}).items()},
            "pending": np.zeros(N, dtype=np.uint8), "age": np.zeros(N, dtype=np.int32), "last": np.zeros((N,) + shape, dtype=np.uint8),
            "count": 0, "next_ordinal": 0, "dropped": 0}
    if history:
        st["prev"], st["chain"] = np.full(cap, -1, dtype=np.int64), np.full(N, -1, dtype=np.int64)
    return st


def reference_begin(state: Dict[str, Any], obs, pending=None) -> None:
    """``SampleBuffer.begin`` on a reference state"""
    state["last"][...] = np.asarray(obs, dtype=np.uint8).reshape(state["last"].shape)
    state["pending"][...] = 0 if pending is None else (np.asarray(pending).reshape(-1) != 0)
    state["age"][...] = 0
    if "chain" in state:
        state["chain"][...] = -1


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
    prev, chain = state.get("prev"), state.get("chain")
    for k in range(K):
        for n in range(N):
            if pending[n]:
                age[n] = 0
                if chain is not None:
                    chain[n] = -1
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
                    if chain is not None:
                        link = int(chain[n])
                        chain[n] = o
                    if slot >= 0:
                        state["obs"][slot] = last[n]
                        if state["next_obs"] is not None:
                            state["next_obs"][slot] = obs[k, n]
                        state["env"][slot] = n
                        state["ordinal"][slot] = o
                        if chain is not None:
                            prev[slot] = link
                        for name, c in cols.items():
                            state["cols"][name][slot] = c[k, n]
                        state["count"] = min(cap, o + 1)
            pending[n] = 1 if done[k, n] else 0
            last[n] = obs[k, n]
    return state


def slot_of(o: int, capacity: int, overflow: str, seed: int) -> int:
    """the slot of ordinal ``o`` (``tc_collect_slot``), -1 where the candidate is dropped"""
    if o < capacity:
        return int(o)
    if overflow == "ring":
        return int(o % capacity)
    if overflow == "random":
        return int(draw_replace_slot(seed, o, capacity))
    return -1


def history_reference(state: Dict[str, Any], index, T: int, pad: str = "zero", overflow: str = "stop", seed: int = 0) -> Dict[str, Any]:
    """The histories of length ``T`` of the slots ``index`` (the module's text) on a reference state with links: ``slots``
    int64 ``[B, T]``, ``valid`` int32 ``[B]``, ``obs`` uint8 ``[B, T, ...]`` (raw frames, zeros for -1) and ``next_obs``
    likewise (None without next frames)."""
    if pad not in PAD:
        raise ValueError(f"pad must be one of {tuple(PAD)}")
    if overflow not in OVERFLOW:
        raise ValueError(f"overflow must be one of {tuple(OVERFLOW)}")
    if int(T) < 1:
        raise ValueError("T must be at least 1")
    if "prev" not in state:
        raise ValueError("the state has no links (reference_state(history=True))")
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    B, T, cap = len(index), int(T), len(state["ordinal"])
    slots, valid = np.full((B, T), -1, dtype=np.int64), np.zeros(B, dtype=np.int32)
    for b, s in enumerate(index):
        if s < 0 or s >= cap or state["ordinal"][s] < 0:
            continue
        slots[b, 0], t = s, 1
        while t < T:
            p = int(state["prev"][slots[b, t - 1]])
            if p < 0:
                break
            q = slot_of(p, cap, overflow, seed)
            if q < 0 or state["ordinal"][q] != p:
                break
            slots[b, t] = q
            t += 1
        valid[b] = t
        if pad == "edge":
            slots[b, t:] = slots[b, t - 1]

    def take(frames, table):
        out = frames[np.clip(table, 0, cap - 1)]
        out[table < 0] = 0
        return out
    obs = take(state["obs"], slots)
    nxt = None
    if state["next_obs"] is not None:
        nxt = np.concatenate([take(state["next_obs"], slots[:, :1]), obs[:, :-1]], axis=1)
    return {"slots": slots, "valid": valid, "obs": obs, "next_obs": nxt}


# ---------------------------------------------------------------------------------------------- the device path
class _ColumnC(C.Structure):  # tc_collect_column
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("elem_size", C.c_int32), ("reserved", C.c_int32)]


class CollectDescC(C.Structure):  # tc_collect_desc
    _fields_ = [("capacity", C.c_int64), ("num_envs", C.c_int32), ("stride", C.c_int32), ("mode", C.c_int32),
                ("n_columns", C.c_int32), ("seed", C.c_uint64), ("frame_bytes", C.c_int64), ("obs", C.c_void_p),
                ("next_obs", C.c_void_p), ("ordinal", C.c_void_p), ("env", C.c_void_p), ("columns", _ColumnC * MAX_COLUMNS),
                ("pending", C.c_void_p), ("age", C.c_void_p), ("last", C.c_void_p), ("counters", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


def _gather_dtypes():
    import torch
    from . import _native as nat
    return {torch.uint8: nat.U8, torch.float16: nat.F16, torch.bfloat16: nat.BF16, torch.float32: nat.F32}


class SampleBuffer:
    """A dataset of ``capacity`` samples on the device, filled from the rollout rows of K-step calls by ``tc_collect``.

    ``obs_shape``: the shape of one uint8 frame as the env produces it (packed ``[C, H, W/8]`` with ``packed=True``, byte class
    masks ``[C, H, W]``, rgb ``[H, W, 3]``); its byte count must be a multiple of 4.  ``columns``: name -> torch dtype of 1, 4
    or 8 bytes per element (at most 8), each a ``[K, N]`` row array of the calls.  ``next_obs``: also keep the frame after the
    step (``X1`` of the replay buffer).  ``stride`` / ``overflow`` / ``seed``: see the module's text.  ``max_rows``: the longest
    call ``collect`` accepts (sizes the scratch once; ``collect`` never allocates).  ``history``: T > 1 keeps a link per slot
    (``prev``, and ``chain`` per env: the module's text) so that ``sample`` returns the last T frames of the sample's
    episode; the links travel through ``tc_collect`` as a column, which leaves 7 columns to the caller.  With next
    frames a history needs ``stride = 1`` (``next_obs[b, t] = obs[b, t - 1]`` holds only there).

    Live tensors: ``obs``, ``next_obs``, ``ordinal`` (int64, -1 = empty), ``env`` (int32), ``cols[name]``, ``counters`` (int64
    [4]: filled slots, next ordinal, dropped, candidates of the last call) and the per-env carry ``pending`` / ``age`` /
    ``last``; with a history ``prev`` (int64 per slot) and ``chain`` (int64 per env).  Only ``len()``, ``dropped`` and ``full``
    synchronise."""

    def __init__(self, capacity: int, num_envs: int, obs_shape: Sequence[int], columns: Optional[Mapping[str, Any]] = None,
                 next_obs: bool = False, stride: int = 1, overflow: str = "stop", seed: int = 0, max_rows: int = 128,
                 device: Any = "cuda:0", packed: bool = False, history: int = 1):
        import torch
        from . import _native as nat
        self.capacity, self.num_envs, self.obs_shape = int(capacity), int(num_envs), tuple(int(v) for v in obs_shape)
        self.stride, self.overflow, self.seed, self.max_rows = int(stride), str(overflow), int(seed), int(max_rows)
        self.packed, self.history = bool(packed), int(history)
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
        if self.history < 1:
            raise ValueError("history must be at least 1")
        links = self.history > 1
        if links and next_obs and self.stride > 1:
            raise ValueError("a history of next frames needs stride = 1: next_obs[b, t] = obs[b, t - 1] holds only there")
        if len(columns) > MAX_COLUMNS - links:
            raise ValueError(f"at most {MAX_COLUMNS} columns, {MAX_COLUMNS - 1} with a history (the links are one)")
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
        self.prev = torch.full((cap,), -1, dtype=torch.int64, device=dev) if links else None
        self.chain = torch.full((N,), -1, dtype=torch.int64, device=dev) if links else None
        self._link_rows = torch.zeros((self.max_rows, N), dtype=torch.int64, device=dev) if links else None
        nbytes = int(nat.lib().tc_collect_scratch_bytes(self.max_rows, N))
        self._scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        d = self._desc = CollectDescC()
        d.capacity, d.num_envs, d.stride, d.mode, d.n_columns = cap, N, self.stride, OVERFLOW[overflow], len(columns)
        d.seed, d.frame_bytes = self.seed & 0xFFFFFFFFFFFFFFFF, self.frame_bytes
        d.obs, d.next_obs = self.obs.data_ptr(), (self.next_obs.data_ptr() if next_obs else None)
        d.ordinal, d.env = self.ordinal.data_ptr(), self.env.data_ptr()
        for j, (name, t) in enumerate(self.cols.items()):
            d.columns[j].dst, d.columns[j].elem_size = t.data_ptr(), t.element_size()
        if links:  # the link of a written candidate goes where its columns go
            c = d.columns[len(columns)]
            c.src, c.dst, c.elem_size = self._link_rows.data_ptr(), self.prev.data_ptr(), 8
            d.n_columns = len(columns) + 1
        d.pending, d.age, d.last = self.pending.data_ptr(), self.age.data_ptr(), self.last.data_ptr()
        d.counters, d.scratch, d.scratch_bytes = self.counters.data_ptr(), self._scratch.data_ptr(), nbytes

    # ---- filling
    def begin(self, obs, pending=None) -> None:
        """Start of the data: ``obs`` ``[N, ...]`` is the observation the first action is computed from (what ``reset()``
        returned), ``pending`` ``[N]`` marks envs whose next row is a re-spawn row (default: none); ``age = 0``, ``chain = -1``."""
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
        if self.chain is not None:
            self.chain.fill_(-1)

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
            if self.chain is not None:  # the links of this call's candidates, in front of the call that moves the carry
                self._nat.check(self._nat.lib().tc_collect_link(C.byref(d), K, done[0], done[1], self.chain.data_ptr(),
                                                                self._link_rows.data_ptr(), stream), "tc_collect_link")
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

    def sample(self, index, dtype=None, history=None, pad="zero") -> Dict[str, Any]:
        """The samples at ``index`` (int64 ``[B]`` on the device): ``obs`` (and ``next_obs``) as ``dtype`` (default float32)
        -- packed frames through ``unpack_obs`` (0.0 / 1.0, or 0 / 255 for uint8), byte frames as an indexed copy scaled by
        1 / 255 for float dtypes -- plus ``env``, ``ordinal`` and every column at ``index``.

        On a buffer built with ``history > 1``: ``history`` = t (default: the buffer's T) makes ``obs`` / ``next_obs``
        ``[B, t, ...]`` for t > 1, newest first, and adds ``slots`` int64 ``[B, t]`` and ``valid`` int32 ``[B]`` (the module's
        text; ``pad``: "zero" or "edge").  An index outside the buffer or at an empty slot gives ``valid = 0``, zero frames and
        ``ordinal = -1``.  Columns, ``env`` and ``ordinal`` stay ``[B]``, of the newest entry; a column's history is
        ``buf.cols[name][slots.clamp(min=0)]``.  Byte frames come from ``tc_gather_frames`` in one pass."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        T = self.history if history is None else int(history)
        if pad not in PAD:
            raise ValueError(f"pad must be one of {tuple(PAD)}, got {pad!r}")
        if T < 1:
            raise ValueError("history must be at least 1")
        if self.prev is None:
            if T > 1:
                raise ValueError("this buffer keeps no links: build it with history > 1")
            return self._sample_single(index, dtype)
        nat = self._nat
        if dtype not in _gather_dtypes():
            raise ValueError("dtype must be torch.uint8, float16, bfloat16 or float32")
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or index.device != self.device \
                or not index.is_contiguous():
            raise ValueError(f"index must be a contiguous 1-D int64 tensor on {self.device}")
        B = int(index.shape[0])
        slots = torch.empty((B, T), dtype=torch.int64, device=self.device)
        valid = torch.empty(B, dtype=torch.int32, device=self.device)
        two = self.next_obs is not None and not self.packed and T > 1   # the next-history from its own table
        nslots = torch.empty_like(slots) if two else None
        lead = (B, T) if T > 1 else (B,)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if B:  # (an empty batch has no storage to point at)
                nat.check(nat.lib().tc_history_resolve(self.prev.data_ptr(), self.ordinal.data_ptr(), self.capacity,
                                                       OVERFLOW[self.overflow], self.seed & 0xFFFFFFFFFFFFFFFF, index.data_ptr(), B, T,
                                                       PAD[pad], slots.data_ptr(), nslots.data_ptr() if two else None,
                                                       valid.data_ptr(), stream), "tc_history_resolve")

            def gather(src, src2, table, group):
                out = torch.empty((B * T,) + self.obs_shape, dtype=dtype, device=self.device)
                if B:
                    nat.check(nat.lib().tc_gather_frames(src.data_ptr(), src2.data_ptr() if src2 is not None else None, self.capacity,
                                                         self.frame_bytes, table.data_ptr(), B * T, group, out.data_ptr(),
                                                         _gather_dtypes()[dtype], stream), "tc_gather_frames")
                return out.view(lead + self.obs_shape)
            if self.packed:
                from .packing import unpack_obs
                obs = unpack_obs(self.obs, dtype, index=slots.view(-1))
                obs = obs.view(lead + tuple(obs.shape[1:]))
            else:
                obs = gather(self.obs, None, slots, 1)
            newest = slots[:, 0].clamp(min=0)
            out = {"obs": obs, "env": self.env.index_select(0, newest), "slots": slots, "valid": valid,
                   "ordinal": torch.where(valid > 0, self.ordinal.index_select(0, newest), torch.full_like(newest, -1))}
            if self.next_obs is not None:
                if two:
                    out["next_obs"] = gather(self.obs, self.next_obs, nslots, T)
                elif self.packed:
                    first = unpack_obs(self.next_obs, dtype, index=slots[:, 0].contiguous())
                    out["next_obs"] = first if T == 1 else torch.cat([first.unsqueeze(1), obs[:, :-1]], dim=1)
                else:
                    out["next_obs"] = gather(self.next_obs, None, slots, 1)
        for name, t in self.cols.items():
            out[name] = t.index_select(0, newest)
        return out

    def _sample_single(self, index, dtype) -> Dict[str, Any]:
        import torch

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

    def _tensors(self) -> Tuple[str, ...]:
        return self._TENSORS + (("prev", "chain") if self.prev is not None else ())

    def state_dict(self) -> Dict[str, Any]:
        sd = {k: getattr(self, k).cpu().clone() for k in self._tensors() if getattr(self, k) is not None}
        sd["cols"] = {k: t.cpu().clone() for k, t in self.cols.items()}
        sd["config"] = {"capacity": self.capacity, "num_envs": self.num_envs, "obs_shape": self.obs_shape, "stride": self.stride,
                        "overflow": self.overflow, "seed": self.seed, "packed": self.packed}
        if self.prev is not None:
            sd["config"]["history"] = self.history
        return sd

    def load_state_dict(self, sd: Mapping[str, Any]) -> None:
        cfg = sd["config"]
        for k in ("capacity", "num_envs", "stride", "overflow", "seed"):
            if cfg[k] != getattr(self, k):
                raise ValueError(f"state_dict was taken from a buffer with {k} = {cfg[k]!r}, this one has {getattr(self, k)!r}")
        if tuple(cfg["obs_shape"]) != self.obs_shape or set(sd["cols"]) != set(self.cols) or ("next_obs" in sd) != (self.next_obs is not None):
            raise ValueError("state_dict does not match this buffer's frames / columns")
        if (cfg.get("history", 1) > 1) != (self.prev is not None) or ("prev" in sd) != (self.prev is not None):
            raise ValueError("state_dict and this buffer must both keep history links, or neither")
        for k in self._tensors():
            if getattr(self, k) is not None:
                getattr(self, k).copy_(sd[k])
        for k, t in self.cols.items():
            t.copy_(sd["cols"][k])
