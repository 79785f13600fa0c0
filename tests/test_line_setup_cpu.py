"""The outline set-up the kernels run (tinycarlo_amd/csrc/tc_line.h: r_clip_line_f on exact-integer doubles, the 32-bit
r_line2_setup_f, r_quad_dp / r_outline_edge on int32 parts) against the literal int64 forms of the same header, on the
CPU.  tests/line_setup_shim.py builds the header twice (-DTC_LINE_LITERAL and not) and compares in C; required equal,
exactly: the whole LineP (a, b, step, ecount, ex, ey, xmajor), the clipped end points, the accept / reject bit, and for
the quad its eight vertices and the degenerate bit.

Inputs
  * edges as the kernel makes them: the quad of int32 pixel end points with the raster fuzz test's end-point
    distribution, frames 24x40, 64x64 and 480x640, thickness 1..8, the two long edges and all four;
  * borders: p at -3..+3 px around every border and corner, every integer dp within 1.5 of length 65536 in one octant
    (a different one per frame size), both directions of the edge;
  * magnitudes: pixel coordinates at and next to +-2^31 and +-2^13, one end there and the other on screen, or both there;
  * degenerate shapes: horizontal, vertical, zero-length, through a corner, both ends clipped on one axis.

Non-vacuity: per frame size, the number of cases the LITERAL form alone sends into each branch (the four clip
instances, the role swap of each axis, reject before and between the axes, x-major / y-major, swapped or not) is
printed and must be non-zero.  The literal has no reject behind the x blocks -- they leave both outcodes 0 -- so that
count is printed and must be zero; what is counted there instead is the accept after a clip.
"""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import line_setup_shim as ls
from test_fill_events_cpu import segments as fuzz_segments

SIZES = [(24, 40), (64, 64), (480, 640)]  # H, W
OCTANT = {(24, 40): 0, (64, 64): 3, (480, 640): 5}
INT_MAX, INT_MIN = 2147483647, -2147483648
U_LO, U_HI = 46338, 65539  # the major component of a dp of length 65536 +- 1.5 in one octant
NEEDED = [b for b in ls.BRANCHES if b not in ("reject_after", "degenerate")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return ls.build_shim(tmp_path_factory.mktemp("tc_line_setup"))


def positions(n):
    """pixel coordinates at -3..+3 px from the border pixels 0 and n - 1 of an axis of n pixels, and far from both"""
    return np.array(sorted(set(range(-3, 4)) | set(range(n - 4, n + 3)) | {n // 2}), dtype=np.int32)


def magnitude_segments(H, W):
    """one end at or next to +-2^31 / +-2^13 on one axis or both, the other end on screen or at such a value too"""
    far = [INT_MIN, INT_MIN + 1, INT_MIN + 2, INT_MAX, INT_MAX - 1, INT_MAX - 2, 8191, 8192, 8193, -8191, -8192, -8193]
    on_x, on_y = [0, 1, W // 2, W - 2, W - 1], [0, 1, H // 2, H - 2, H - 1]
    s = []
    for fx in far + on_x:
        for fy in far + on_y:
            if fx in on_x and fy in on_y:
                continue
            for x in on_x:
                for y in on_y:
                    s.append((fx, fy, x, y))
                    s.append((x, y, fx, fy))
            for gx in far[::3]:
                for gy in far[1::3]:
                    s.append((fx, fy, gx, gy))
    return np.array(s, dtype=np.int64).astype(np.int32)


def degenerate_segments(H, W):
    """horizontal, vertical and zero-length segments, lines through each corner, and lines that cross the whole frame
    (both ends clipped on one axis, or on both)"""
    s = []
    far = [1, 3, 7, 100, 5000, 1 << 20]
    for y in list(range(-3, 4)) + list(range(H - 4, H + 3)) + [H // 2]:
        for L in far:
            s += [(-L, y, W - 1 + L, y), (W - 1 + L, y, -L, y), (W // 2, y, W - 1 + L, y), (-L, y, W // 2, y)]
    for x in list(range(-3, 4)) + list(range(W - 4, W + 3)) + [W // 2]:
        for L in far:
            s += [(x, -L, x, H - 1 + L), (x, H - 1 + L, x, -L), (x, H // 2, x, H - 1 + L), (x, -L, x, H // 2)]
    for x in positions(W):
        for y in positions(H):
            s.append((x, y, x, y))
    for cx, cy in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]:
        for a, b in [(1, 1), (1, -1), (2, 1), (1, 2), (3, -1), (-1, 3), (7, 5), (5, -7), (1, 0), (0, 1), (100, 1), (1, 100)]:
            for k in (1, 2, 5, 50, 3000):
                for m in (0, 1, 2, 5, 50, 3000):
                    s += [(cx - k * a, cy - k * b, cx + m * a, cy + m * b), (cx + m * a, cy + m * b, cx - k * a, cy - k * b)]
    rng = np.random.default_rng(H * 7 + W)
    n = 4000
    # through the frame from outside to outside: top to bottom, left to right, and corner to corner
    s += list(zip(rng.integers(-W, 2 * W, n), -rng.integers(1, 4 * H, n), rng.integers(-W, 2 * W, n), H + rng.integers(0, 4 * H, n)))
    s += list(zip(-rng.integers(1, 4 * W, n), rng.integers(-H, 2 * H, n), W + rng.integers(0, 4 * W, n), rng.integers(-H, 2 * H, n)))
    s += list(zip(W + rng.integers(0, 4 * W, n), H + rng.integers(0, 4 * H, n), -rng.integers(1, 4 * W, n), -rng.integers(1, 4 * H, n)))
    return np.array(s, dtype=np.int64).astype(np.int32)


def segment_sets(H, W):
    """name -> list of (thickness, segments)"""
    return {
        "kernel edges": [(th, fuzz_segments(np.random.default_rng(H * 100 + th), 6000, H, W)) for th in range(1, 9)],
        "magnitudes": [(th, magnitude_segments(H, W)) for th in range(1, 9)],
        "degenerate": [(th, degenerate_segments(H, W)) for th in range(1, 9)],
    }


def border_cuts(parts):
    return np.linspace(U_LO, U_HI, parts + 1).astype(np.int64)


def run_borders(shim, H, W, cnt, threads=8):
    px, py = positions(W), positions(H)
    cuts = border_cuts(4 * threads)

    def part(k):
        c = np.zeros(ls.N_CNT, dtype=np.int64)
        return ls.borders(shim, W, H, OCTANT[(H, W)], int(cuts[k]), int(cuts[k + 1]), px, py, c) + (c,)

    with ThreadPoolExecutor(threads) as ex:  # (ctypes releases the GIL for the call)
        parts = list(ex.map(part, range(len(cuts) - 1)))
    for p in parts:
        cnt += p[3]
    return sum(p[0] for p in parts), sum(p[1] for p in parts), next((p[2] for p in parts if p[1]), None)


@pytest.mark.parametrize("H,W", SIZES)
def test_new_forms_equal_the_literal_ones(shim, H, W):
    total = np.zeros(ls.N_CNT, dtype=np.int64)
    for name, sets in segment_sets(H, W).items():
        cnt = np.zeros(ls.N_CNT, dtype=np.int64)
        n = 0
        for th, seg in sets:
            for e_step in (1, 2):  # all four outline edges, and the two long ones of the thickness-2 form
                nbad, first = ls.segments(shim, W, H, th, e_step, seg, cnt)
                assert nbad == 0, (name, H, W, th, e_step, nbad, "first:", first)
                n += len(seg)
        print(f"{H}x{W} {name}: {n} segments;", ", ".join(f"{b} {int(c)}" for b, c in zip(ls.BRANCHES, cnt)))
        total += cnt
    cnt = np.zeros(ls.N_CNT, dtype=np.int64)
    cases, nbad, bad = run_borders(shim, H, W, cnt)
    assert nbad == 0, (H, W, "borders", nbad, "dp, p of the first:", bad)
    assert cases > 2 * 225 * 140_000  # the whole octant of the annulus at 15 x 15 positions, both directions
    print(f"{H}x{W} borders: {cases} edges;", ", ".join(f"{b} {int(c)}" for b, c in zip(ls.BRANCHES, cnt)))
    total += cnt
    print(f"{H}x{W} all: ", ", ".join(f"{b} {int(c)}" for b, c in zip(ls.BRANCHES, total)))
    for b in NEEDED + ["degenerate"]:
        assert total[ls.BRANCHES.index(b)] > 0, (H, W, "the literal form never takes", b)
    assert total[ls.BRANCHES.index("reject_after")] == 0


def test_known_answers(shim):
    """a few cases by hand, so that the comparison is pinned to something outside the header: a zero-length segment is
    degenerate in both forms, and the branch counters see what the case is"""
    cnt = np.zeros(ls.N_CNT, dtype=np.int64)
    assert ls.segments(shim, 64, 64, 2, 1, [(5, 5, 5, 5)], cnt) == (0, None)
    assert cnt[ls.BRANCHES.index("degenerate")] == 1 and cnt.sum() == 1
    cnt[:] = 0
    # a horizontal segment across the whole 64 x 64 frame, thickness 2: the two long edges are clipped at both x borders
    assert ls.segments(shim, 64, 64, 2, 2, [(-10, 30, 80, 30)], cnt) == (0, None)
    got = dict(zip(ls.BRANCHES, cnt.tolist()))
    assert got["x_first"] == 2 and got["x_second"] == 2 and got["y_first"] == 0 and got["x_major"] == 2, got
    assert got["swapped"] == 1 and got["not_swapped"] == 1, got  # v3 -> v0 runs right to left, v1 -> v2 left to right
    cnt[:] = 0
    # far above the frame: both ends carry the same outcode
    assert ls.segments(shim, 64, 64, 3, 1, [(10, -50, 40, -60)], cnt) == (0, None)
    assert cnt[ls.BRANCHES.index("reject_before")] == 4


def test_sanitizer_run(tmp_path):
    """the same shim as a stand-alone program under UBSan (with the float-conversion checks) + ASan, over the same
    inputs: no value reaches an undefined conversion, shift or overflow in either form"""
    exe = ls.build_program(tmp_path)
    path = os.path.join(str(tmp_path), "cases.bin")
    n = 0
    with open(path, "wb") as f:
        for H, W in SIZES:
            for sets in segment_sets(H, W).values():
                for th, seg in sets:
                    for e_step in (1, 2):
                        np.array([0, W, H, th, e_step, len(seg)], dtype=np.int32).tofile(f)
                        np.ascontiguousarray(seg, dtype=np.int32).tofile(f)
                        n += len(seg)
            px, py = positions(W), positions(H)
            np.array([1, W, H, OCTANT[(H, W)], U_LO, U_HI, len(px), len(py)], dtype=np.int32).tofile(f)
            px.tofile(f)
            py.tofile(f)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    cases = int(r.stdout.split()[1])
    assert r.stdout.endswith("mismatches 0\n") and cases > n + 3 * 2 * 225 * 140_000, r.stdout
