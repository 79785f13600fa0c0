"""Per-env car constants and their per-episode draw, host side (no GPU): the numpy restatement of the device draw
against the oracle's SplitMix64, the argument validation of set_env_cars / randomize_cars, the ABI constants, and the
compiler's resource figures of the per-env-car kernel instantiations."""
import os
import re

import numpy as np
import pytest

import orc
from common import HIPCC, ROOT, TC_FEAT_CAR, assert_one_variant_set, dev_kernel_resources, kernel_variant
from tinycarlo_amd import _native as nat
from tinycarlo_amd.config import CarParams
from tinycarlo_amd.randomization import CAR_COLUMNS, car_ranges, car_rows, config_row, draw_car_params

M64 = (1 << 64) - 1


def _draw_ref(seed, env, episode, lo, hi, mask):
    """the draw rule of include/tinycarlo_hip.h written out with the oracle library's SplitMix64 and python ints"""
    sm = orc.lib().orc_splitmix64_at
    z = sm(sm(seed & M64, 0x636172), ((env & 0xFFFFFFFF) << 32) | (episode & 0xFFFFFFFF))
    row = [float("nan")] * 8
    for j in range(8):
        if (mask >> j) & 1:
            u = float(sm(z, j) >> 11) * 2.0 ** -53
            row[j] = lo[j] + (hi[j] - lo[j]) * u
    return row


def _car(**kw):
    base = dict(T=1 / 30, track_width=0.03, wheelbase=0.08, max_velocity=1.0, max_steering_angle=35.0,
                steering_speed=None, max_acceleration=None, max_deceleration=None)
    base.update(kw)
    return CarParams(**base)


LO = np.array([0.05, 0.02, 0.5, 20.0, 50.0, 0.5, 0.7, -0.05])
HI = np.array([0.11, 0.04, 1.5, 45.0, 150.0, 2.5, 3.0, 0.05])


@pytest.mark.parametrize("seed", [0, 1, 0x636172, 2 ** 63 + 12345, M64])
def test_draw_matches_the_oracle_splitmix(seed):
    envs = [0, 1, 31, 63, 4095, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    eps = [0, 1, 2, 1000, 2 ** 31 - 1, 2 ** 32 - 2, 2 ** 32 - 1]
    for mask in (0xFF, 0b10100101):
        # episode counters are int32 on the device: values near 2^32 arrive as negative int32 and wrap the same way
        got = draw_car_params(seed, np.array(envs)[:, None], np.array(eps, dtype=np.int64)[None, :], LO, HI, mask)
        assert got.shape == (len(envs), len(eps), 8)
        for a, e in enumerate(envs):
            for b, k in enumerate(eps):
                want = _draw_ref(seed, e, k, LO, HI, mask)
                g = got[a, b]
                for j in range(8):
                    if (mask >> j) & 1:
                        assert g[j] == want[j], (seed, e, k, j)
                    else:
                        assert np.isnan(g[j])
        as_i32 = np.array(eps, dtype=np.int64).astype(np.uint32).astype(np.int32)
        assert np.array_equal(draw_car_params(seed, 7, as_i32, LO, HI, mask), draw_car_params(seed, 7, eps, LO, HI, mask),
                              equal_nan=True)


def test_lo_equals_hi_and_u_below_one():
    lo = np.array([0.08, 0.03, 1.0, 35.0, 90.0, 1.0, 2.0, -0.01])
    got = draw_car_params(99, np.arange(512), np.arange(512) * 7, lo, lo)
    assert np.array_equal(got, np.broadcast_to(lo, got.shape))
    u = draw_car_params(3, np.arange(4096), 0, np.zeros(8), np.ones(8))
    assert u.min() >= 0.0 and u.max() < 1.0
    assert 0.45 < u.mean() < 0.55
    base = config_row(_car())
    keep = draw_car_params(3, 5, 2, LO, HI, mask=1 << CAR_COLUMNS.index("steering_shift"), base=base)
    assert np.array_equal(keep[:7], base[:7]) and LO[7] <= keep[7] < HI[7]


def test_streams_differ_per_env_episode_and_seed():
    a = draw_car_params(1, np.arange(64), 0, LO, HI)
    assert len(np.unique(a[:, 0])) == 64
    assert not np.array_equal(a, draw_car_params(1, np.arange(64), 1, LO, HI))
    assert not np.array_equal(a, draw_car_params(2, np.arange(64), 0, LO, HI))
    # sharding: env_offset + index reproduces the rows of one big batch
    assert np.array_equal(a[32:], draw_car_params(1, 32 + np.arange(32), 0, LO, HI))


def test_validation():
    p = _car()
    with pytest.raises(ValueError, match="unknown"):
        car_ranges(p, {"wheelbasee": (0.05, 0.1)})
    with pytest.raises(ValueError, match="lo <= hi"):
        car_ranges(p, {"wheelbase": (0.1, 0.05)})
    with pytest.raises(ValueError, match="not set"):
        car_ranges(p, {"steering_speed": (50, 100)})
    with pytest.raises(ValueError, match="not set"):
        car_ranges(p, {"max_deceleration": (1, 2)})
    with pytest.raises(ValueError, match=r"\(lo, hi\)"):
        car_ranges(p, {"wheelbase": (0.05, 0.08, 0.1)})
    with pytest.raises(ValueError, match="finite"):
        car_ranges(p, {"track_width": (0.01, float("inf"))})
    with pytest.raises(ValueError, match="positive"):
        car_ranges(p, {"max_velocity": (0.0, 1.0)})
    lo, hi, mask = car_ranges(_car(steering_speed=90.0), {"steering_speed": (50, 100), "steering_shift": (-0.02, 0.0)})
    assert mask == (1 << 4) | (1 << 7) and lo[4] == 50 and hi[7] == 0.0
    assert car_ranges(p, None)[2] == 0 and car_ranges(p, {})[2] == 0

    rows = car_rows(p, 4, {"wheelbase": [0.05, 0.06, 0.07, 0.08], "steering_shift": -0.01, "track_width": None})
    assert rows.shape == (4, 8)
    assert np.array_equal(rows[:, 0], [0.05, 0.06, 0.07, 0.08]) and np.all(rows[:, 7] == -0.01)
    assert np.all(rows[:, 1] == 0.03) and np.all(rows[:, 2] == 1.0)
    with pytest.raises(ValueError, match="expected a scalar or 4"):
        car_rows(p, 4, {"wheelbase": [0.05, 0.06, 0.07]})
    with pytest.raises(ValueError, match="positive"):
        car_rows(p, 4, {"max_velocity": [1, 1, 0, 1]})
    with pytest.raises(ValueError, match="finite"):
        car_rows(p, 4, {"steering_shift": float("nan")})
    with pytest.raises(ValueError, match="not set"):
        car_rows(p, 4, {"max_acceleration": 1.0})
    with pytest.raises(ValueError, match="unknown"):
        car_rows(p, 4, {"T": 0.1})


def test_header_constants_match_the_binding():
    h = open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (TC_\w+) (-?\d+)\s", h, re.M)}
    assert d["TC_ABI_VERSION"] == nat.ABI_VERSION == 7
    assert d["TC_CAR_NP"] == nat.CAR_NP == len(nat.CAR_COLUMNS) == 8
    assert nat.CAR_COLUMNS == CAR_COLUMNS
    for j, name in enumerate(CAR_COLUMNS):
        assert d["TC_CAR_" + name.upper()] == j == getattr(nat, "CAR_" + name.upper())
    for f in ("tc_env_set_car", "tc_env_set_car_per_env", "tc_env_set_car_randomization"):
        assert f in nat.EXPORTS and re.search(r"\bint " + f + r"\(", h)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_per_env_car_kernels_keep_their_registers():
    """the kernels with the car bit alone (cfg3's K = 5 variants): no VGPR spill, no scratch, at most 128 VGPRs (4 waves / SIMD)"""
    seen = dev_kernel_resources()
    car = [n for n in seen if (kernel_variant(n) or (None, 0))[1] == TC_FEAT_CAR]
    assert len(car) == 4, sorted(seen)  # tc_step_kernel<5, .., 1u>, tc_env_kernel<5, true|false, 1u>, tc_envg_kernel<1u>
    assert_one_variant_set(seen, car)
