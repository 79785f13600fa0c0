"""tinycarlo_amd/csrc/tc_line.h (clipLine + Line2's set-up, the literal code of the kernels) built alone by the host
compiler: a shared library for ctypes.  Test infrastructure of tests/test_short_edges_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "tc_line.h"
#include <math.h>
#include <stdint.h>

extern "C" int se_skip(int thickness, int W, int H) { return tc_short_edges_skip(thickness, W, H); }

// pixels of Line2(a, b) inside the frame, in drawing order (far end first); returns their number, -1 = clipped away
static int line2_pixels(int W, int H, long long ax, long long ay, long long bx, long long by, int* out, int max) {
  const LineP L = r_line2_setup(W, H, ax, ay, bx, by);
  if (L.ecount < 0) return -1;
  int n = 0;
  for (int k = -1; k <= L.ecount; k++) {
    int x, y;
    if (k < 0) {
      x = L.ex;
      y = L.ey;
    } else {
      const int mn = (int)(((long long)L.b + (long long)k * L.step) >> TC_XY_SHIFT);
      x = L.xmajor ? L.a + k : mn;
      y = L.xmajor ? mn : L.a + k;
    }
    if (x < 0 || x >= W || y < 0 || y >= H) continue;
    if (n < max) {
      out[2 * n] = x;
      out[2 * n + 1] = y;
    }
    n++;
  }
  return n;
}
extern "C" int se_line2(int W, int H, long long ax, long long ay, long long bx, long long by, int* out, int max) {
  return line2_pixels(W, H, ax, ay, bx, by, out, max);
}

static bool inside(int W, int H, long long x, long long y) {
  return x >= 0 && x < ((long long)W << TC_XY_SHIFT) && y >= 0 && y < ((long long)H << TC_XY_SHIFT);
}

// The lemma of tc_line.h for every integer dp with | |dp| - len | <= tol and dp.x in [x_lo, x_hi), at every position
// (px[i], py[j]): the in-frame pixels of Line2(p + dp, p - dp) lie in the cap (mask [2 R + 1][2 R + 1] around p) or are
// the rounded end point of an end inside the clip rectangle.
// stats: [0] cases, [1] cases clipped away whole, [2] cases with an end outside the rectangle that still draw,
//        [3] pixels outside the cap (covered by a rounded end point), [4] violations;  bad: dpx, dpy, px, py, x, y of the first one
extern "C" void se_lemma(int W, int H, double len, double tol, long long x_lo, long long x_hi, const int* px, int npx,
                         const int* py, int npy, const unsigned char* cap, int R, long long* stats, long long* bad) {
  const double lo2 = (len - tol) * (len - tol), hi2 = (len + tol) * (len + tol);
  const long long ymax = (long long)(len + tol) + 1;
  for (long long dx = x_lo; dx < x_hi; dx++) {
    for (int sgn = 0; sgn < 2; sgn++) {
      const double rem_lo = lo2 - (double)dx * (double)dx, rem_hi = hi2 - (double)dx * (double)dx;
      if (rem_hi < 0) continue;
      long long y0 = rem_lo > 0 ? (long long)sqrt(rem_lo) - 1 : 0, y1 = (long long)sqrt(rem_hi) + 1;
      if (y0 < 0) y0 = 0;
      if (y1 > ymax) y1 = ymax;
      for (long long ady = y0; ady <= y1; ady++) {
        if (sgn && ady == 0) continue;
        const long long dy = sgn ? -ady : ady;
        const double l2 = (double)dx * (double)dx + (double)dy * (double)dy;
        if (l2 < lo2 || l2 > hi2) continue;
        for (int i = 0; i < npx; i++)
          for (int j = 0; j < npy; j++) {
            const long long cx = (long long)px[i] << TC_XY_SHIFT, cy = (long long)py[j] << TC_XY_SHIFT;
            const long long ax = cx + dx, ay = cy + dy, bx = cx - dx, by = cy - dy;
            int pix[2 * 64];
            const int n = line2_pixels(W, H, ax, ay, bx, by, pix, 64);
            stats[0]++;
            if (n < 0) {
              stats[1]++;
              continue;
            }
            const bool ia = inside(W, H, ax, ay), ib = inside(W, H, bx, by);
            if (!ia || !ib) stats[2]++;
            const int rax = (int)((ax + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT), ray = (int)((ay + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT);
            const int rbx = (int)((bx + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT), rby = (int)((by + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT);
            for (int k = 0; k < (n < 64 ? n : 64); k++) {
              const int x = pix[2 * k], y = pix[2 * k + 1], rx = x - px[i], ry = y - py[j];
              if (rx >= -R && rx <= R && ry >= -R && ry <= R && cap[(ry + R) * (2 * R + 1) + rx + R]) continue;
              stats[3]++;
              if (ia && x == rax && y == ray) continue;
              if (ib && x == rbx && y == rby) continue;
              if (stats[4]++ == 0) {
                bad[0] = dx; bad[1] = dy; bad[2] = px[i]; bad[3] = py[j]; bad[4] = x; bad[5] = y;
              }
            }
            if (n > 64 && stats[4]++ == 0) {
              bad[0] = dx; bad[1] = dy; bad[2] = px[i]; bad[3] = py[j]; bad[4] = -1; bad[5] = n;
            }
          }
      }
    }
  }
}

// The long edges: an end v inside the clip rectangle is not moved by the clip, and Line2(v, w) and Line2(w, v) both draw
// its rounded pixel -- as the step-0 pixel or as the far end pixel.  e: [n][4] = vx, vy, wx, wy (16.16); returns failures.
extern "C" int se_long_edges(int W, int H, const long long* e, int n, long long* bad) {
  int fail = 0;
  for (int i = 0; i < n; i++) {
    const long long vx = e[4 * i], vy = e[4 * i + 1], wx = e[4 * i + 2], wy = e[4 * i + 3];
    if (!inside(W, H, vx, vy)) continue;
    const int rx = (int)((vx + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT), ry = (int)((vy + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT);
    for (int dir = 0; dir < 2; dir++) {
      const LineP L = dir ? r_line2_setup(W, H, wx, wy, vx, vy) : r_line2_setup(W, H, vx, vy, wx, wy);
      bool ok = L.ecount >= 0;
      if (ok) {
        const int sx = L.xmajor ? L.a : L.b >> TC_XY_SHIFT, sy = L.xmajor ? L.b >> TC_XY_SHIFT : L.a;  // step 0
        ok = (L.ex == rx && L.ey == ry) || (sx == rx && sy == ry);
      }
      if (!ok && fail++ == 0) {
        bad[0] = vx; bad[1] = vy; bad[2] = wx; bad[3] = wy;
      }
    }
  }
  return fail;
}
"""

FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc")]


def build_shim(d):
    """-> ctypes library of the shim built in directory d"""
    src, lib = os.path.join(str(d), "short_edges_shim.cpp"), os.path.join(str(d), "libtc_short_edges.so")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.check_call(["c++"] + FLAGS + ["-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.se_skip.argtypes = [C.c_int, C.c_int, C.c_int]
    L.se_line2.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, ip, C.c_int]
    L.se_lemma.restype = None
    L.se_lemma.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int64, C.c_int64, ip, C.c_int, ip, C.c_int,
                           C.POINTER(C.c_uint8), C.c_int, lp, lp]
    L.se_long_edges.argtypes = [C.c_int, C.c_int, lp, C.c_int, lp]
    return L


def line2(L, W, H, a, b):
    """set of in-frame pixels of Line2(a, b) by the header's set-up"""
    out = np.zeros((4 * (W + H) + 8, 2), dtype=np.int32)
    n = L.se_line2(W, H, int(a[0]), int(a[1]), int(b[0]), int(b[1]), out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
    assert n <= len(out)
    return set() if n < 0 else {(int(x), int(y)) for x, y in out[:n]}
