"""Bit-packed class-mask observations (``TC_FMT_CLASSES_BITS``, ``TinyCarloVecEnv(..., obs_packing="bits")``).

Layout: uint8 ``[..., C, H, W/8]``.  Pixel ``(y, x)`` of class ``c`` is bit ``x & 7`` of byte ``x >> 3`` of row ``y`` of
plane ``c``; a set bit stands for 255 in the byte format.  ``W`` is a multiple of 32.

``pack_bits_reference`` / ``unpack_bits_reference`` are plain numpy / torch-CPU and are the executable definition of that
layout; ``unpack_obs`` is the device path (``tc_unpack_bits``: one HIP kernel, no env handle).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native as nat


def pack_bits_reference(mask) -> np.ndarray:
    """Class masks ``[..., W]`` (any non-zero value = set) -> packed uint8 ``[..., W/8]``."""
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    if m.shape[-1] % 8 != 0:
        raise ValueError("the last axis must be a multiple of 8")
    m = (m != 0).reshape(m.shape[:-1] + (m.shape[-1] // 8, 8))
    out = np.zeros(m.shape[:-1], dtype=np.uint8)
    for b in range(8):  # bit b of byte x >> 3 is pixel x = 8 * (x >> 3) + b
        out |= m[..., b].astype(np.uint8) << np.uint8(b)
    return out


def unpack_bits_reference(packed, W: int, dtype=torch.float32) -> torch.Tensor:
    """Packed uint8 ``[..., W/8]`` -> CPU tensor ``[..., W]``: 0 / 255 for ``torch.uint8``, 0.0 / 1.0 for float dtypes."""
    p = packed.detach().cpu().numpy() if isinstance(packed, torch.Tensor) else np.asarray(packed)
    if p.dtype != np.uint8 or p.shape[-1] * 8 != W:
        raise ValueError("packed must be uint8 with a last axis of W / 8")
    bits = (p[..., None] >> np.arange(8, dtype=np.uint8)) & np.uint8(1)   # [..., W/8, 8], bit b at [..., b]
    bits = torch.from_numpy(np.ascontiguousarray(bits.reshape(p.shape[:-1] + (W,))))
    return bits * 255 if dtype == torch.uint8 else bits.to(dtype)


_DTYPES = {torch.uint8: nat.U8, torch.float16: nat.F16, torch.bfloat16: nat.BF16, torch.float32: nat.F32}


def unpack_obs(packed: torch.Tensor, dtype: torch.dtype = torch.float32, index: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Expands packed observations on the device, on the current stream (``tc_unpack_bits``).

    packed: uint8 ``[..., C, H, W/8]``, contiguous, on the GPU (an env's ``out["obs"]``, a rollout's ``obs``, a replay
    buffer).  Returns ``[..., C, H, W]`` of ``dtype`` -- ``torch.uint8`` 0 / 255 (what the byte format holds),
    ``float16`` / ``bfloat16`` / ``float32`` 0.0 / 1.0 (the consumers' ``obs / 255``).  With ``index`` (int64, 1-D, on the
    device) the leading axes are flattened and the result is ``[len(index), C, H, W]``: frame ``j`` is frame ``index[j]``,
    repeats allowed; an index outside the range gives a frame of zeros.  ``out``: a contiguous tensor of the result's
    shape and dtype to write into.  Neither allocates (given ``out``) nor synchronises; can be captured into a graph."""
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or packed.dim() < 3:
        raise ValueError("packed must be a uint8 tensor [..., C, H, W/8]")
    if packed.device.type != "cuda":
        raise ValueError("packed must be on the GPU (unpack_bits_reference is the CPU definition)")
    if not packed.is_contiguous():
        raise ValueError("packed must be contiguous")
    if dtype not in _DTYPES:
        raise ValueError("dtype must be torch.uint8, float16, bfloat16 or float32")
    Cn, H, W8 = (int(v) for v in packed.shape[-3:])
    W = W8 * 8
    if Cn < 1 or H < 1 or W < 1 or W % 32 != 0:
        raise ValueError("packed frames need C, H >= 1 and a width that is a multiple of 32")
    lead = tuple(packed.shape[:-3])
    n_src = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1 or index.device != packed.device or not index.is_contiguous():
            raise ValueError("index must be a contiguous 1-D int64 tensor on packed's device")
        n_out, shape = int(index.shape[0]), (int(index.shape[0]), Cn, H, W)
    else:
        n_out, shape = n_src, lead + (Cn, H, W)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=packed.device)
    elif (tuple(out.shape) != shape or out.dtype != dtype or out.device != packed.device or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on packed's device")
    if n_out == 0:
        return out
    if n_src == 0:
        raise ValueError("packed holds no frame")
    if packed.data_ptr() % 4 or out.data_ptr() % 16:
        raise ValueError("packed must be 4-byte aligned and out 16-byte aligned")
    with torch.cuda.device(packed.device):
        stream = torch.cuda.current_stream(packed.device).cuda_stream
        nat.check(nat.lib().tc_unpack_bits(packed.data_ptr(), n_src, Cn, H, W, index.data_ptr() if index is not None else None,
                                           n_out, out.data_ptr(), _DTYPES[dtype], stream), "tc_unpack_bits")
    return out
