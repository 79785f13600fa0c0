"""The fill-walker events of tinycarlo_amd/csrc/tc_fill.h on the CPU: the header is built alone by the host compiler and
its loop-free form (tc_fill_events, what the kernels run) is compared with the literal loop nest
(tc_fill_events_literal, the specification) on every output: np, py[0..np), pv[0..np), wmask, y_first, y_last.

(a) Past its integer prologue the routine is a function of (imin, ty0..ty3, (int)ymax) that only compares those
    integers with each other: every order pattern of the six is enumerated (tc_fill_walk vs tc_fill_walk_literal).
(b) Through the full signature: quads made from end points the way r_quad (tc_device.h) makes them, with the end point
    distribution of tests/test_gpu_raster_fuzz.py, and plain random 64-bit vertices.  The same run checks that the
    literal form IS its prologue followed by tc_fill_walk_literal, which ties (a) to the specification.
(c) The same shim as a stand-alone program under -fsanitize=undefined,address.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import ROOT

INT_MIN = -2147483648

SHIM = r"""
#include "tc_fill.h"
#include <math.h>
#include <stdint.h>
#include <stdio.h>

struct Out {
  int np, py[4], pv[4], wmask, y_first, y_last;
};
static bool same(const Out& a, const Out& b) {
  if (a.np != b.np || a.wmask != b.wmask || a.y_first != b.y_first || a.y_last != b.y_last) return false;
  for (int s = 0; s < a.np; s++)
    if (a.py[s] != b.py[s] || a.pv[s] != b.pv[s]) return false;
  return true;
}
static Out fresh() {
  Out o;
  o.np = -1;
  for (int s = 0; s < 4; s++) o.py[s] = o.pv[s] = -77;
  o.wmask = o.y_first = o.y_last = -77;
  return o;
}

// one call of the post-prologue entry; form 0 = literal, 1 = loop-free.  out[12] = np, py[4], pv[4], wmask, y_first, y_last
extern "C" void walk_one(int form, int imin, const int* ty, int ymaxi, int* out) {
  Out o = fresh();
  o.np = form ? tc_fill_walk(imin, ty[0], ty[1], ty[2], ty[3], ymaxi, 0, o.py, o.pv, o.wmask, o.y_first, o.y_last)
              : tc_fill_walk_literal(imin, ty[0], ty[1], ty[2], ty[3], ymaxi, o.py, o.pv, o.wmask, o.y_first, o.y_last);
  out[0] = o.np;
  for (int s = 0; s < 4; s++) out[1 + s] = o.py[s], out[5 + s] = o.pv[s];
  out[9] = o.wmask, out[10] = o.y_first, out[11] = o.y_last;
}

// (a) every (ty0..ty3) in [0, nv)^4 x imin in 0..3 x ymaxi in [ylo, yhi]: returns the mismatches, *cases = cases run,
// bad[6] = the first mismatching (imin, ty0..ty3, ymaxi); hist[5] counts the cases by np of the literal form
extern "C" long walk_exhaustive(int nv, int ylo, int yhi, long* cases, int* bad, long* hist) {
  long n = 0, nbad = 0;
  for (int t0 = 0; t0 < nv; t0++)
    for (int t1 = 0; t1 < nv; t1++)
      for (int t2 = 0; t2 < nv; t2++)
        for (int t3 = 0; t3 < nv; t3++)
          for (int imin = 0; imin < 4; imin++)
            for (int ym = ylo; ym <= yhi; ym++) {
              Out a = fresh(), b = fresh();
              a.np = tc_fill_walk_literal(imin, t0, t1, t2, t3, ym, a.py, a.pv, a.wmask, a.y_first, a.y_last);
              b.np = tc_fill_walk(imin, t0, t1, t2, t3, ym, 0, b.py, b.pv, b.wmask, b.y_first, b.y_last);
              n++;
              hist[a.np]++;
              if (!same(a, b) && nbad++ == 0) bad[0] = imin, bad[1] = t0, bad[2] = t1, bad[3] = t2, bad[4] = t3, bad[5] = ym;
            }
  *cases = n;
  return nbad;
}

// (b) one quad through the full signature: 0 = all forms agree
static int check_quad(int W, int H, const long long* q, long* stat) {
  Out a = fresh(), b = fresh();
  a.np = tc_fill_events_literal(W, H, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], a.py, a.pv, a.wmask, a.y_first, a.y_last);
  b.np = tc_fill_events(W, H, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], b.py, b.pv, b.wmask, b.y_first, b.y_last);
  int r = same(a, b) ? 0 : 1;
  // the literal form = the prologue, then tc_fill_walk_literal on what the prologue hands over
  int imin, ty0, ty1, ty2, ty3, ymaxi;
  const int off = tc_fill_prologue(W, H, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], imin, ty0, ty1, ty2, ty3, ymaxi);
  Out c = fresh();
  c.np = 0, c.wmask = 0, c.y_first = 0, c.y_last = -1;
  if (!off) c.np = tc_fill_walk_literal(imin, ty0, ty1, ty2, ty3, ymaxi, c.py, c.pv, c.wmask, c.y_first, c.y_last);
  if (!same(a, c)) r |= 2;
  stat[off ? 5 : a.np]++;  // pieces 0..4 of the quads that reach the loop, [5] = off-screen
  if (!off && a.y_last >= a.y_first) stat[6]++;
  return r;
}

// ThickLine's quad as r_quad (tc_device.h) makes it; false when the segment is degenerate
static bool quad_of(int x0, int y0, int x1, int y1, int thickness, long long* q) {
  long long p0x = (long long)x0 * TC_XY_ONE, p0y = (long long)y0 * TC_XY_ONE;
  long long p1x = (long long)x1 * TC_XY_ONE, p1y = (long long)y1 * TC_XY_ONE;
  const double INV_XY_ONE = 1. / TC_XY_ONE;
  double dx = (double)(p0x - p1x) * INV_XY_ONE, dy = (double)(p1y - p0y) * INV_XY_ONE;
  double rr = dx * dx + dy * dy;
  int odd = thickness & 1;
  long long th = (long long)thickness << (TC_XY_SHIFT - 1);
  if (!(tc_fabs(rr) > 2.2204460492503131e-16)) return false;
  rr = ((double)th + odd * TC_XY_ONE * 0.5) / sqrt(rr);
  long long dpx = (long long)rint(dy * rr), dpy = (long long)rint(dx * rr);
  q[0] = p0x + dpx; q[1] = p0x - dpx; q[2] = p1x - dpx; q[3] = p1x + dpx;
  q[4] = p0y + dpy; q[5] = p0y - dpy; q[6] = p1y - dpy; q[7] = p1y + dpy;
  return true;
}

// seg[n][4] = x0, y0, x1, y1.  Returns the mismatching quads; first_bad = index of the first one; stat[7] as above
extern "C" long events_segments(int n, int W, int H, int thickness, const int* seg, long* first_bad, long* stat) {
  long nbad = 0;
  for (int k = 0; k < n; k++) {
    long long q[8];
    if (!quad_of(seg[4 * k], seg[4 * k + 1], seg[4 * k + 2], seg[4 * k + 3], thickness, q)) continue;
    if (check_quad(W, H, q, stat) && nbad++ == 0) *first_bad = k;
  }
  return nbad;
}
// q[n][8] = qx0..qx3, qy0..qy3
extern "C" long events_quads(int n, int W, int H, const long long* q, long* first_bad, long* stat) {
  long nbad = 0;
  for (int k = 0; k < n; k++)
    if (check_quad(W, H, q + 8 * k, stat) && nbad++ == 0) *first_bad = k;
  return nbad;
}

#ifdef TC_FILL_MAIN
// the sanitizer run: the exhaustive domain, then quads from a small generator of its own (end points inside, around and
// far from the frame, INT_MIN, axis-aligned, diagonal, zero length; raw vertices up to +-2^62)
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
static int rint_in(long long lo, long long hi) { return (int)(lo + (long long)(rnd() % (uint64_t)(hi - lo + 1))); }
int main() {
  long cases = 0, hist[5] = {0, 0, 0, 0, 0}, stat[7] = {0, 0, 0, 0, 0, 0, 0}, first = -1;
  int bad[6];
  long nbad = walk_exhaustive(6, -1, 6, &cases, bad, hist);
  const int sizes[3][2] = {{16, 16}, {64, 64}, {480, 640}};
  for (int it = 0; it < 60000; it++) {
    const int H = sizes[it % 3][0], W = sizes[it % 3][1], th = 1 + it / 3 % 8;
    int s[4];
    switch (rnd() % 8) {
      case 0: s[0] = rint_in(0, W - 1), s[1] = rint_in(0, H - 1), s[2] = s[0] + rint_in(-6, 6), s[3] = s[1] + rint_in(-6, 6); break;
      case 1: s[0] = rint_in(-W, 2 * W), s[1] = rint_in(-H, 2 * H), s[2] = rint_in(-W, 2 * W), s[3] = rint_in(-H, 2 * H); break;
      case 2: s[0] = rint_in(0, W - 1), s[1] = rint_in(0, H - 1), s[2] = rint_in(-300000000, 300000000), s[3] = rint_in(-300000000, 300000000); break;
      case 3: for (int j = 0; j < 4; j++) s[j] = rint_in(-2000000000, 2000000000); break;
      case 4: s[0] = rint_in(0, W - 1), s[1] = rint_in(0, H - 1), s[2] = s[3] = INT32_MIN; if (rnd() & 1) s[0] = s[1] = INT32_MIN; break;
      case 5: s[0] = s[2] = rint_in(-2, W + 1), s[1] = s[3] = rint_in(-2, H + 1); break;
      case 6: { const int L = rint_in(1, W > H ? W : H), d = (int)(rnd() % 4);
                s[0] = rint_in(-5, W + 4), s[1] = rint_in(-5, H + 4), s[2] = s[0] + (d != 1) * L, s[3] = s[1] + (d == 3 ? -L : (d != 0) * L); break; }
      default: s[0] = rint_in(0, W - 1), s[1] = -rint_in(0, 5000), s[2] = rint_in(0, W - 1), s[3] = H + rint_in(0, 5000); break;
    }
    nbad += events_segments(1, W, H, th, s, &first, stat);
    long long q[8];
    for (int j = 0; j < 8; j++) q[j] = (long long)rnd() >> (1 + rnd() % 48);
    nbad += events_quads(1, W, H, q, &first, stat);
  }
  printf("cases %ld mismatches %ld\n", cases, nbad);
  return nbad != 0;
}
#endif
"""


def write_shim(d):
    src = os.path.join(str(d), "fill_shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    return src


CXX = ["c++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tc_fill")
    src, lib = write_shim(d), os.path.join(str(d), "libtc_fill.so")
    subprocess.check_call(CXX + ["-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_long)
    L.walk_one.argtypes = [C.c_int, C.c_int, ip, C.c_int, ip]
    L.walk_one.restype = None
    L.walk_exhaustive.argtypes = [C.c_int, C.c_int, C.c_int, lp, ip, lp]
    L.walk_exhaustive.restype = C.c_long
    L.events_segments.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip, lp, lp]
    L.events_segments.restype = C.c_long
    L.events_quads.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), lp, lp]
    L.events_quads.restype = C.c_long
    return L


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_long))


def walk(L, form, imin, ty, ymaxi):
    t, out = np.asarray(ty, dtype=np.int32), np.zeros(12, dtype=np.int32)
    L.walk_one(form, imin, _ip(t), ymaxi, _ip(out))
    n = int(out[0])
    return n, out[1:1 + n].tolist(), out[5:5 + n].tolist(), int(out[9]), int(out[10]), int(out[11])


def test_exhaustive_over_the_order_domain(shim):
    """all (ty0..ty3) in {0..5}^4 x imin in 0..3 x (int)ymax in {-1..6}: 6^4 * 4 * 8 = 41 472 cases, none left out"""
    cases, bad, hist = np.zeros(1, dtype=np.int64), np.zeros(6, dtype=np.int32), np.zeros(5, dtype=np.int64)
    nbad = shim.walk_exhaustive(6, -1, 6, _lp(cases), _ip(bad), _lp(hist))
    assert int(cases[0]) == 6 ** 4 * 4 * 8
    if nbad:
        imin, ty, ym = int(bad[0]), bad[1:5].tolist(), int(bad[5])
        assert walk(shim, 1, imin, ty, ym) == walk(shim, 0, imin, ty, ym), (nbad, "first at imin, ty, ymax =", imin, ty, ym)
    assert nbad == 0
    print("cases by number of pieces 0..4:", hist.tolist())
    # 0, 2, 3 and 4 pieces all occur; 1 cannot (the second walker reaches the first one's vertex within the budget left)
    assert hist[[0, 2, 3, 4]].min() > 0 and hist[1] == 0, hist


def test_known_answers(shim):
    """a few quads by hand, so that the literal copy in the header is pinned to something outside itself"""
    # a diamond: top vertex 0 at row 0, vertices 1 and 3 at row 2, bottom vertex 2 at row 4
    for form in (0, 1):
        assert walk(shim, form, 0, [0, 2, 4, 2], 10) == (4, [0, 0, 2, 2], [0 | 1 << 2, 0 | 3 << 2, 1 | 2 << 2, 3 | 2 << 2], 0b1010, 0, 3)
        # the same cut off by the frame's last row
        assert walk(shim, form, 0, [0, 2, 4, 2], 1) == (2, [0, 0], [0 | 1 << 2, 0 | 3 << 2], 0b10, 0, 1)
        # all four vertices on one row: no piece, no row
        assert walk(shim, form, 0, [3, 3, 3, 3], 10) == (0, [], [], 0, 3, 2)
        # a flat top (vertices 0 and 1 on row 1): walker 0 skips the horizontal edge
        assert walk(shim, form, 0, [1, 1, 5, 5], 10) == (2, [1, 1], [1 | 2 << 2, 0 | 3 << 2], 0b10, 1, 4)
        # first row above the frame
        assert walk(shim, form, 2, [4, 1, -3, 1], 10)[4:] == (0, 3)


def segments(rng, n, H, W):
    """n end point pairs with the distribution of tests/test_gpu_raster_fuzz.py's random_segments, drawn kind by kind"""
    kind = rng.integers(0, 10, n)
    s = np.zeros((n, 4), dtype=np.int64)
    for k in range(10):
        m = np.flatnonzero(kind == k)
        c = len(m)
        if k == 0:      # short, inside
            x0, y0 = rng.integers(0, W, c), rng.integers(0, H, c)
            v = (x0, y0, x0 + rng.integers(-6, 7, c), y0 + rng.integers(-6, 7, c))
        elif k == 1:    # anywhere near the frame: straddles every border
            v = (rng.integers(-W, 2 * W, c), rng.integers(-H, 2 * H, c), rng.integers(-W, 2 * W, c), rng.integers(-H, 2 * H, c))
        elif k == 2:    # one end far away
            v = (rng.integers(0, W, c), rng.integers(0, H, c), rng.integers(-300000000, 300000000, c), rng.integers(-300000000, 300000000, c))
        elif k == 3:    # both ends far away
            v = tuple(rng.integers(-2000000000, 2000000000, c) for _ in range(4))
        elif k == 4:    # np.int32(NaN) / overflow
            x0, y0 = rng.integers(0, W, c), rng.integers(0, H, c)
            both = rng.random(c) < 0.5
            v = (np.where(both, INT_MIN, x0), np.where(both, INT_MIN, y0), np.full(c, INT_MIN), np.full(c, INT_MIN))
        elif k == 5:    # zero length
            x0, y0 = rng.integers(-2, W + 2, c), rng.integers(-2, H + 2, c)
            v = (x0, y0, x0, y0)
        elif k == 6:    # axis aligned / diagonal
            x0, y0 = rng.integers(-5, W + 5, c), rng.integers(-5, H + 5, c)
            L = rng.integers(1, max(W, H), c)
            d = np.array([(1, 0), (0, 1), (1, 1), (1, -1), (-1, 0), (0, -1)])[rng.integers(0, 6, c)]
            v = (x0, y0, x0 + d[:, 0] * L, y0 + d[:, 1] * L)
        elif k == 7:    # hugging a border
            v = (rng.integers(-1, 2, c), rng.integers(-3, H + 3, c), rng.integers(-1, 2, c) + (W - 1) * rng.integers(0, 2, c), rng.integers(-3, H + 3, c))
        elif k == 8:    # steep long line through the frame
            v = (rng.integers(0, W, c), -rng.integers(0, 5000, c), rng.integers(0, W, c), H + rng.integers(0, 5000, c))
        else:           # shallow long line through the frame
            v = (-rng.integers(0, 5000, c), rng.integers(0, H, c), W + rng.integers(0, 5000, c), rng.integers(0, H, c))
        s[m] = np.stack(v, axis=1)
    # hugging the top / bottom border as well (the fuzz test's kind 7 with the axes swapped)
    sw = np.flatnonzero((kind == 7) & (rng.random(n) < 0.5))
    s[sw] = np.stack([rng.integers(-3, W + 3, len(sw)), rng.integers(-1, 2, len(sw)), rng.integers(-3, W + 3, len(sw)),
                      rng.integers(-1, 2, len(sw)) + (H - 1) * rng.integers(0, 2, len(sw))], axis=1)
    return np.ascontiguousarray(s.astype(np.int32))


@pytest.mark.parametrize("H,W", [(16, 16), (64, 64), (480, 640)])
def test_full_signature_on_thick_line_quads(shim, H, W):
    """8 thicknesses x 14 000 segments per frame size (336 000 quads over the three sizes): zero mismatches"""
    stat = np.zeros(7, dtype=np.int64)
    for th in range(1, 9):
        seg = segments(np.random.default_rng(H * 100 + th), 14000, H, W)
        first = np.full(1, -1, dtype=np.int64)
        nbad = shim.events_segments(len(seg), W, H, th, _ip(seg), _lp(first), _lp(stat))
        assert nbad == 0, (H, W, th, nbad, "first:", seg[int(first[0])].tolist())
    print(f"{H}x{W}: quads by pieces 0..4 {stat[:5].tolist()}, off-screen {int(stat[5])}, with fill rows {int(stat[6])}")
    assert stat[2:5].min() > 0 and stat[5] > 0 and stat[6] > 0, stat  # the loop, its early return and real rows are all reached


def test_full_signature_on_random_vertices(shim):
    """plain random 64-bit vertices, no rectangle: magnitudes from a few pixels up to 2^62 (one below the range in which
    the literal form's own `+ delta` would overflow), and small ones around the frame so that the loop is reached"""
    rng = np.random.default_rng(11)
    stat = np.zeros(7, dtype=np.int64)
    for H, W in [(16, 16), (64, 64), (480, 640)]:
        n = 60000
        big = rng.integers(-2 ** 62, 2 ** 62, (n, 8)) >> rng.integers(0, 56, (n, 8))
        near = rng.integers(-2 * max(H, W), 3 * max(H, W), (n, 8)) * 65536 + rng.integers(-65536, 65536, (n, 8))
        mixed = np.where(rng.random((n, 8)) < 0.7, near, big)
        for q in (big, near, mixed):
            q = np.ascontiguousarray(q, dtype=np.int64)
            first = np.full(1, -1, dtype=np.int64)
            nbad = shim.events_quads(n, W, H, q.ctypes.data_as(C.POINTER(C.c_longlong)), _lp(first), _lp(stat))
            assert nbad == 0, (H, W, nbad, "first:", q[int(first[0])].tolist())
    print(f"random vertices: by pieces 0..4 {stat[:5].tolist()}, off-screen {int(stat[5])}, with fill rows {int(stat[6])}")
    assert stat[2:5].min() > 0 and stat[5] > 0, stat


def test_sanitizer_run(tmp_path):
    """the shim as a stand-alone program under UBSan + ASan: out-of-range table slots, signed overflow, bad shifts"""
    src, exe = write_shim(tmp_path), os.path.join(str(tmp_path), "fill_san")
    subprocess.check_call(CXX + ["-g", "-DTC_FILL_MAIN", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.startswith("cases 41472 mismatches 0"), r.stdout
