"""ThickLine at thickness 2 without its two short outline edges: the proof behind tc_short_edges_skip
(tinycarlo_amd/csrc/tc_line.h), on the CPU, against the literal clipLine / Line2 set-up of the kernels built by the host
compiler (tests/short_edges_shim.py).

ThickLine(p0, p1) fills the quad v0 = p0 + dp, v1 = p0 - dp, v2 = p1 - dp, v3 = p1 + dp: four Line2 outline edges
(v3->v0, v0->v1, v1->v2, v2->v3), the scanline fill, and a round cap at p0 and p1.

LEMMA (thickness 2, frames of at least 8 x 8).  For an integer pixel p and every dp that r_quad can produce, the in-frame
pixels of Line2(p + dp, p - dp) are a subset of
  * the radius-1 cap at p, plus
  * for each end v = p +- dp that lies inside the clip rectangle [0, W << 16) x [0, H << 16): the rounded end point.
The long edge through that v draws exactly that pixel (clipLine does not move an end inside the rectangle, and Line2
draws both end points: one as its step-0 pixel, one as the far end pixel it writes explicitly), and the caps are drawn
for every segment.  Hence ThickLine without v0->v1 and v2->v3 paints the same pixels.

The enumeration: every integer vector dp whose length is within 1.5 units of 65536 (1.2 M vectors; r_quad rounds each
component of a vector of length 65536, so it stays within 0.71; the set is closed under negation, which makes
Line2(p - dp, p + dp), the edge v2->v3, a member too), and p at -3..+3 px from each border on both axes and far from
all of them, at two frame sizes.  A point 3 px outside a border is rejected by the clip; so is everything further out
(both ends carry the same outcode).  At thickness 3 the lemma is false, and the last tests show it: widening the
trigger to 3 fails this file.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cv_lines_py as cv
from short_edges_shim import build_shim, line2

SIZES = [(24, 40), (64, 64)]  # H, W
_ip, _lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("tc_short_edges"))


def cap_mask(thickness):
    """ThickLine's cap at this thickness as a [2 R + 1][2 R + 1] mask, from the independent restatement of Circle()"""
    R = ((thickness << 15) + 32768) >> 16
    m = np.zeros((2 * R + 1, 2 * R + 1), dtype=np.uint8)
    for x, y in cv.circle_fill(64, 64, 32, 32, R):
        m[y - 32 + R, x - 32 + R] = 1
    return R, m


def positions(n):
    """pixel coordinates at -3..+3 px from the border pixels 0 and n - 1 of an axis of n pixels, and far from both"""
    return np.array(sorted(set(range(-3, 4)) | set(range(n - 4, n + 3)) | {n // 2}), dtype=np.int32)


def dp_length(thickness):
    return float((thickness << 15) + (thickness & 1) * 32768)  # ThickLine: (thickness << 15) + odd * XY_ONE / 2


def lemma(shim, W, H, thickness, px, py, x_lo=None, x_hi=None, tol=1.5, threads=None):
    """-> (stats[5], first violation) of the enumeration over dp.x in [x_lo, x_hi) (default: the whole annulus)"""
    R, m = cap_mask(thickness)
    ln = dp_length(thickness)
    lim = int(ln) + 3
    x_lo, x_hi = (-lim if x_lo is None else x_lo), (lim if x_hi is None else x_hi)
    threads = threads or max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
    cuts = np.linspace(x_lo, x_hi, 4 * threads + 1).astype(np.int64)

    def part(k):
        stats, bad = np.zeros(8, dtype=np.int64), np.zeros(6, dtype=np.int64)
        shim.se_lemma(W, H, ln, tol, int(cuts[k]), int(cuts[k + 1]), px.ctypes.data_as(_ip), len(px), py.ctypes.data_as(_ip), len(py),
                      m.ctypes.data_as(C.POINTER(C.c_uint8)), R, stats.ctypes.data_as(_lp), bad.ctypes.data_as(_lp))
        return stats, bad

    with ThreadPoolExecutor(threads) as ex:  # (ctypes releases the GIL for the call)
        parts = list(ex.map(part, range(len(cuts) - 1)))
    stats = sum(p[0] for p in parts)
    bad = next((p[1].tolist() for p in parts if p[0][4]), None)
    return stats[:5].tolist(), bad


def test_trigger(shim):
    assert shim.se_skip(2, 64, 64) == 1 and shim.se_skip(2, 40, 24) == 1 and shim.se_skip(2, 8, 8) == 1
    assert shim.se_skip(2, 7, 64) == 0 and shim.se_skip(2, 64, 7) == 0  # borders of one axis within reach of each other
    for th in (0, 1, 3, 4, 5, 6, 7, 8, 16):
        assert shim.se_skip(th, 64, 64) == 0, th


def test_header_line2_is_the_restatements(shim):
    """the header's clipLine + Line2 set-up draws what tests/cv_lines_py.py's line2 draws (short edges, long edges,
    clipped ones, huge coordinates)"""
    rng = np.random.default_rng(11)
    for H, W in SIZES:
        for k in range(3000):
            if k % 3 == 0:  # a short edge near a border
                p = np.array([rng.choice(positions(W)), rng.choice(positions(H))], dtype=np.int64) << 16
                ang = rng.uniform(0, 2 * np.pi)
                dp = np.rint(65536 * np.array([np.cos(ang), np.sin(ang)])).astype(np.int64)
                a, b = p + dp, p - dp
            elif k % 3 == 1:  # anywhere near the frame
                a = rng.integers(-(W << 16), 2 * (W << 16), 2)
                b = rng.integers(-(H << 16), 2 * (H << 16), 2)
            else:  # one end far away (2^31 px and beyond: 47 bits)
                a = rng.integers(0, min(W, H) << 16, 2)
                b = rng.integers(-(1 << 47), 1 << 47, 2)
            a, b = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
            assert line2(shim, W, H, a, b) == cv.line2(W, H, a, b), (W, H, a, b)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("thickness", [2, 3, 4, 5, 6, 8])
def test_lemma_wherever_the_trigger_holds(shim, thickness, H, W):
    """the exhaustive enumeration, for every thickness tc_short_edges_skip accepts (thickness 2 alone)"""
    if not shim.se_skip(thickness, W, H):
        return  # this thickness keeps its four edges: nothing claimed, nothing to prove
    stats, bad = lemma(shim, W, H, thickness, positions(W), positions(H))
    print(f"{H}x{W} t={thickness}: cases {stats[0]}, clipped away {stats[1]}, drawn with an end outside the rectangle {stats[2]}, "
          f"pixels outside the cap {stats[3]}, violations {stats[4]}")
    assert stats[4] == 0, ("dp, p, pixel of the first violation", bad)
    assert stats[0] > 225 * 1_200_000 and stats[2] > 0 and stats[3] > 0  # the set is the one the docstring names


@pytest.mark.parametrize("H,W", SIZES)
def test_three_px_outside_is_rejected(shim, H, W):
    """an end point 3 px or more outside a border: clipLine rejects the short edge whatever dp is"""
    out_x = np.array([-3, -4, -100, -(1 << 14), W + 2, W + 3, W + 100, 1 << 14], dtype=np.int32)
    out_y = np.array([-3, -4, -100, -(1 << 14), H + 2, H + 3, H + 100, 1 << 14], dtype=np.int32)
    for px, py in ((out_x, positions(H)), (positions(W), out_y), (out_x, out_y)):
        stats, _ = lemma(shim, W, H, 2, px, py, x_lo=-65540, x_hi=65540)
        assert stats[0] > 0 and stats[1] == stats[0], stats


@pytest.mark.parametrize("H,W", SIZES)
def test_long_edges_draw_their_inside_end_points(shim, H, W):
    """Line2(v, w) and Line2(w, v) draw the rounded v whenever v is inside the clip rectangle: w anywhere"""
    rng = np.random.default_rng(5)
    n = 200_000
    v = np.stack([rng.integers(0, W << 16, n), rng.integers(0, H << 16, n)], axis=1)
    v[::4] = np.stack([rng.choice([0, 1, 32767, 32768, (W << 16) - 32769, (W << 16) - 32768, (W << 16) - 1], n // 4),
                       rng.choice([0, 1, 32767, 32768, (H << 16) - 32769, (H << 16) - 32768, (H << 16) - 1], n // 4)], axis=1)
    span = rng.choice([1 << 17, 1 << 20, 1 << 24, 1 << 30, 1 << 47], n)[:, None]
    w = v + (rng.uniform(-1, 1, (n, 2)) * span).astype(np.int64)
    e = np.ascontiguousarray(np.concatenate([v, w], axis=1), dtype=np.int64)
    bad = np.zeros(4, dtype=np.int64)
    assert shim.se_long_edges(W, H, e.ctypes.data_as(_lp), n, bad.ctypes.data_as(_lp)) == 0, bad.tolist()


def thick_line_long_edges_only(W, H, p0, p1, thickness):
    """cv_lines_py.thick_line with FillConvexPoly's outline edges v0->v1 and v2->v3 left out"""
    calls = [0]
    real = cv.line2

    def long_only(W_, H_, a, b):
        calls[0] += 1
        return real(W_, H_, a, b) if calls[0] in (1, 3) else set()  # v3->v0, (v0->v1), v1->v2, (v2->v3)

    cv.line2 = long_only
    try:
        return cv.thick_line(W, H, p0, p1, thickness)
    finally:
        cv.line2 = real


def random_segment(rng, W, H):
    kind = rng.integers(0, 6)
    if kind == 0:  # on screen
        p0, p1 = (rng.integers(0, W), rng.integers(0, H)), (rng.integers(0, W), rng.integers(0, H))
    elif kind == 1:  # within 6 px of the frame
        p0, p1 = (rng.integers(-6, W + 6), rng.integers(-6, H + 6)), (rng.integers(-6, W + 6), rng.integers(-6, H + 6))
    elif kind == 2:  # 1-3 px long, an end point within 3 px of a border
        p0 = (rng.choice(positions(W)), rng.choice(positions(H)))
        p1 = (p0[0] + rng.integers(-3, 4), p0[1] + rng.integers(-3, 4))
    elif kind == 3:  # an end point within 3 px of a border, the other anywhere near
        p0 = (rng.choice(positions(W)), rng.choice(positions(H)))
        p1 = (rng.integers(-200, W + 200), rng.integers(-200, H + 200))
    elif kind == 4:  # within 200 px
        p0, p1 = (rng.integers(-200, W + 200), rng.integers(-200, H + 200)), (rng.integers(-200, W + 200), rng.integers(-200, H + 200))
    else:  # up to +-3000 px
        p0, p1 = (rng.integers(0, W), rng.integers(0, H)), (rng.integers(-3000, 3000), rng.integers(-3000, 3000))
    return (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1]))


@pytest.mark.parametrize("H,W", [(64, 64), (128, 128), (24, 40)])
def test_whole_thick_lines_random(shim, H, W):
    """whole ThickLines, as they are against without the two short Line2 calls, wherever the trigger holds"""
    for thickness in (2, 3, 4):
        if not shim.se_skip(thickness, W, H):
            continue
        rng = np.random.default_rng(1000 * H + W + thickness)
        for _ in range(2500):
            p0, p1 = random_segment(rng, W, H)
            assert cv.thick_line(W, H, p0, p1, thickness) == thick_line_long_edges_only(W, H, p0, p1, thickness), (W, H, p0, p1)


def test_lemma_is_false_at_thickness_3(shim):
    """dp = (-113512, 65537) at p = (-1, 1): the short edge, clipped at the left border, draws (1, 0), outside the
    radius-2 cap at p and no rounded end point -- one of 1.7 M violations of the whole enumeration at thickness 3"""
    H, W = 24, 40
    stats, bad = lemma(shim, W, H, 3, positions(W), positions(H), x_lo=-113513, x_hi=-113511, threads=1)
    assert stats[4] > 0 and bad is not None, stats
    assert not shim.se_skip(3, W, H)


THICKNESS_3_PICTURES = [
    # W, H, p0, p1: ThickLine at thickness 3 loses a pixel without its short edges -- (0, 1), (0, 14), (0, 4), each 2 px
    # from p0 beside the left border, where the clipped short edge reaches further than the cap and the fill
    (40, 24, (1, -1), (-43, -28)),
    (40, 24, (1, 12), (-50, -20)),
    (40, 24, (1, 2), (-21, -11)),
]


def test_thickness_3_needs_its_short_edges():
    assert THICKNESS_3_PICTURES
    for W, H, p0, p1 in THICKNESS_3_PICTURES:
        full, cut = cv.thick_line(W, H, p0, p1, 3), thick_line_long_edges_only(W, H, p0, p1, 3)
        assert cut < full, (W, H, p0, p1)
        assert cv.thick_line(W, H, p0, p1, 2) == thick_line_long_edges_only(W, H, p0, p1, 2)
