"""tinycarlo_amd/csrc/tc_line.h built twice by the host compiler in one translation unit -- namespace lit with
-DTC_LINE_LITERAL (clipLine, Line2's set-up and ThickLine's quad as drawing.cpp has them, in int64) and namespace neu
without (the forms the kernels run: f64 clip, 32-bit set-up) -- and compared case by case in C.  A shared library for
ctypes, and with -DTC_LINE_MAIN a stand-alone program for the sanitizers that reads its cases from a file.
Test infrastructure of tests/test_line_setup_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# counters of ls_* (what the LITERAL form does with a case)
BRANCHES = ["inside", "reject_before", "y_first", "y_second", "reject_between", "x_first", "x_second", "reject_after",
            "accept_clipped", "x_major", "y_major", "swapped", "not_swapped", "y_roles_swapped", "x_roles_swapped", "degenerate"]
N_CNT = len(BRANCHES)

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef TC_LINE_MAIN
#include <thread>
#endif
#include "tc_trig.h"
namespace lit {
#define TC_LINE_LITERAL
#include "tc_line.h"
#undef TC_LINE_LITERAL
}
#undef TC_LINE_H
namespace neu {
#include "tc_line.h"
}

enum { B_INSIDE, B_REJ_BEFORE, B_Y1, B_Y2, B_REJ_BETWEEN, B_X1, B_X2, B_REJ_AFTER, B_ACC_CLIPPED, B_XMAJOR, B_YMAJOR, B_SWAPPED,
       B_NOT_SWAPPED, B_Y_ROLES, B_X_ROLES, B_DEGENERATE, N_CNT };

// The literal r_clip_line again, statement for statement, with a counter in every branch.  check_edge holds it to the
// header's own result, so the counts are the header's.
static bool clip_traced(long long width, long long height, long long& x1, long long& y1, long long& x2, long long& y2, long* cnt) {
  int c1, c2;
  long long right = width - 1, bottom = height - 1;
  c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
  c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
  if ((c1 | c2) == 0) cnt[B_INSIDE]++;
  if ((c1 & c2) != 0) cnt[B_REJ_BEFORE]++;
  if ((c1 & c2) == 0 && (c1 | c2) != 0) {
    const bool n1 = (c1 & 12) != 0, n2 = (c2 & 12) != 0;
    if (n1 || n2) {
      cnt[B_Y1]++;
      const bool sw = !n1;
      if (sw) cnt[B_Y_ROLES]++;
      long long xa = sw ? x2 : x1, ya = sw ? y2 : y1, xb = sw ? x1 : x2, yb = sw ? y1 : y2;
      const int ca = sw ? c2 : c1;
      const long long a = ca < 8 ? 0 : bottom;
      xa += (long long)((double)(a - ya) * (double)(xb - xa) / (double)(yb - ya));
      const int cn = (xa < 0) + (xa > right) * 2;
      if (sw) {
        x2 = xa; y2 = a; c2 = cn;
      } else {
        x1 = xa; y1 = a; c1 = cn;
      }
      if (n1 && n2) {
        cnt[B_Y2]++;
        const long long a2 = c2 < 8 ? 0 : bottom;
        x2 += (long long)((double)(a2 - y2) * (double)(x2 - x1) / (double)(y2 - y1));
        y2 = a2;
        c2 = (x2 < 0) + (x2 > right) * 2;
      }
      if ((c1 & c2) != 0) cnt[B_REJ_BETWEEN]++;
    }
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
      cnt[B_X1]++;
      const bool m1 = c1 != 0, m2 = c2 != 0;
      const bool sw = !m1;
      if (sw) cnt[B_X_ROLES]++;
      long long xa = sw ? x2 : x1, ya = sw ? y2 : y1, xb = sw ? x1 : x2, yb = sw ? y1 : y2;
      const int ca = sw ? c2 : c1;
      const long long a = ca == 1 ? 0 : right;
      ya += (long long)((double)(a - xa) * (double)(yb - ya) / (double)(xb - xa));
      if (sw) {
        x2 = a; y2 = ya; c2 = 0;
      } else {
        x1 = a; y1 = ya; c1 = 0;
      }
      if (m1 && m2) {
        cnt[B_X2]++;
        const long long a2 = c2 == 1 ? 0 : right;
        y2 += (long long)((double)(a2 - x2) * (double)(y2 - y1) / (double)(x2 - x1));
        x2 = a2;
        c2 = 0;
      }
      if ((c1 | c2) != 0) cnt[B_REJ_AFTER]++;  // (the x blocks leave both codes 0: the literal has no reject behind them)
    }
    if ((c1 | c2) == 0) cnt[B_ACC_CLIPPED]++;
  }
  return (c1 | c2) == 0;
}

template <class A, class B>
static bool same_line(const A& a, const B& b) {
  return a.a == b.a && a.b == b.b && a.step == b.step && a.ecount == b.ecount && a.ex == b.ex && a.ey == b.ey && a.xmajor == b.xmajor;
}

// One edge a -> b (16.16, integers below 2^48): the clip alone (accept bit, clipped end points) and the whole LineP, both
// forms.  0 = equal.  bit 0: clip differs, bit 1: LineP differs, bit 2: the traced copy is not the header's literal
static int check_edge(int W, int H, long long ax, long long ay, long long bx, long long by, long* cnt) {
  int r = 0;
  long long l[4] = {ax, ay, bx, by}, t[4] = {ax, ay, bx, by};
  const bool lacc = lit::r_clip_line((long long)W << TC_XY_SHIFT, (long long)H << TC_XY_SHIFT, l[0], l[1], l[2], l[3]);
  const bool tacc = clip_traced((long long)W << TC_XY_SHIFT, (long long)H << TC_XY_SHIFT, t[0], t[1], t[2], t[3], cnt);
  if (tacc != lacc || memcmp(l, t, sizeof l)) r |= 4;
  double d[4] = {(double)ax, (double)ay, (double)bx, (double)by};
  const bool nacc = neu::r_clip_line_f((double)W * 65536.0 - 1.0, (double)H * 65536.0 - 1.0, d[0], d[1], d[2], d[3]);
  if (nacc != lacc) r |= 1;
  for (int k = 0; k < 4; k++)
    if (!(d[k] == (double)l[k]) || d[k] != __builtin_trunc(d[k])) r |= 1;
  const lit::LineP L = lit::r_line2_setup_literal(W, H, ax, ay, bx, by);
  const neu::LineP N = neu::r_line2_setup_f(W, H, (double)ax, (double)ay, (double)bx, (double)by);
  const neu::LineP N2 = neu::r_line2_setup(W, H, ax, ay, bx, by);  // the int64 entry point of the default build
  if (!same_line(L, N) || !same_line(L, N2) || (L.ecount >= 0) != lacc) r |= 2;
  if (lacc) {
    const long long dx = l[2] - l[0], dy = l[3] - l[1];
    const bool xm = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy);
    cnt[xm ? B_XMAJOR : B_YMAJOR]++;
    cnt[(xm ? dx < 0 : dy < 0) ? B_SWAPPED : B_NOT_SWAPPED]++;
    if (xm != (L.xmajor != 0)) r |= 4;
  }
  return r;
}

// One ThickLine segment: the quad (degenerate bit, eight vertices) and its outline edges -- all four, or e_step = 2: the
// two long ones -- from the int32 parts as the kernels form them.  bit 3: quad differs, bit 4: r_outline_edge differs
static int check_segment(int W, int H, int th, const int* s, int e_step, long* cnt) {
  long long q[8], v[8];
  int dpx = 0, dpy = 0, ldx = 0, ldy = 0;
  const bool lok = lit::r_quad_literal(s[0], s[1], s[2], s[3], th, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
  const bool nok = neu::r_quad_dp(s[0], s[1], s[2], s[3], th, dpx, dpy);
  const bool l2ok = lit::r_quad_dp(s[0], s[1], s[2], s[3], th, ldx, ldy);
  if (lok != nok || lok != l2ok) return 8;
  if (!lok) {
    cnt[B_DEGENERATE]++;
    return 0;
  }
  int r = 0;
  neu::r_quad_vertices(s[0], s[1], s[2], s[3], dpx, dpy, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
  if (memcmp(q, v, sizeof q) || ldx != dpx || ldy != dpy) r |= 8;
  for (int e = 0; e < 4; e += e_step) {
    const int p = (e + 3) & 3;  // edge e runs v[e - 1] -> v[e]
    r |= check_edge(W, H, q[p], q[4 + p], q[e], q[4 + e], cnt);
    const lit::LineP L = lit::r_line2_setup_literal(W, H, q[p], q[4 + p], q[e], q[4 + e]);
    const lit::LineP L2 = lit::r_outline_edge(W, H, s[0], s[1], s[2], s[3], dpx, dpy, e);
    const neu::LineP N = neu::r_outline_edge(W, H, s[0], s[1], s[2], s[3], dpx, dpy, e);
    if (!same_line(L, N) || !same_line(L, L2)) r |= 16;
  }
  return r;
}

// seg[n][4] = x0, y0, x1, y1 (pixels).  Returns the number of segments on which the forms differ.
extern "C" long ls_segments(int n, int W, int H, int th, int e_step, const int* seg, long* first_bad, long* cnt) {
  long nbad = 0;
  for (int k = 0; k < n; k++)
    if (check_segment(W, H, th, seg + 4 * k, e_step, cnt) && nbad++ == 0) *first_bad = k;
  return nbad;
}

// Borders: Line2(p + dp, p - dp) and Line2(p - dp, p + dp) for every integer dp with | |dp| - len | <= tol in the octant
// 0 <= dp.y <= dp.x (oct bit 0: x and y change places, bit 1: x negated, bit 2: y negated) with dp.x' in [lo, hi), at every
// p = (px[i], py[j]) pixels.  bad: dpx, dpy, px, py of the first difference
extern "C" long ls_borders(int W, int H, double len, double tol, int oct, long long lo, long long hi, const int* px, int npx,
                           const int* py, int npy, long* cases, long long* bad, long* cnt) {
  long nbad = 0;
  const double lo2 = (len - tol) * (len - tol), hi2 = (len + tol) * (len + tol);
  for (long long u = lo; u < hi; u++)
    for (long long w = 0; w <= u; w++) {
      const double l2 = (double)u * (double)u + (double)w * (double)w;
      if (l2 < lo2) {  // jump to just below the inner circle
        const long long w0 = (long long)sqrt(lo2 - (double)u * (double)u) - 1;
        if (w0 > w) w = w0;
        continue;
      }
      if (l2 > hi2) break;
      long long dx = (oct & 1) ? w : u, dy = (oct & 1) ? u : w;
      if (oct & 2) dx = -dx;
      if (oct & 4) dy = -dy;
      for (int i = 0; i < npx; i++)
        for (int j = 0; j < npy; j++) {
          const long long cx = (long long)px[i] * TC_XY_ONE, cy = (long long)py[j] * TC_XY_ONE;
          const int r = check_edge(W, H, cx + dx, cy + dy, cx - dx, cy - dy, cnt) | check_edge(W, H, cx - dx, cy - dy, cx + dx, cy + dy, cnt);
          *cases += 2;
          if (r && nbad++ == 0) bad[0] = dx, bad[1] = dy, bad[2] = px[i], bad[3] = py[j];
        }
    }
  return nbad;
}

#ifdef TC_LINE_MAIN
// The sanitizer run: the cases of tests/test_line_setup_cpu.py from the file it wrote.  Records of int32:
//   0, W, H, thickness, e_step, n, then n * 4 coordinates       (ls_segments)
//   1, W, H, oct, lo, hi, npx, npy, then npx + npy positions    (ls_borders at length 65536, tolerance 1.5)
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : NULL;
  if (!f) return 2;
  long cnt[N_CNT] = {0}, nbad = 0, cases = 0, first = -1;
  int h[8];
  while (fread(h, sizeof(int), 1, f) == 1) {
    if (h[0] == 0) {
      if (fread(h + 1, sizeof(int), 5, f) != 5) return 3;
      int* seg = (int*)malloc(sizeof(int) * 4 * (size_t)h[5] + 4);
      if (fread(seg, sizeof(int), 4 * (size_t)h[5], f) != 4 * (size_t)h[5]) return 3;
      nbad += ls_segments(h[5], h[1], h[2], h[3], h[4], seg, &first, cnt);
      cases += h[5];
      free(seg);
    } else {
      if (fread(h + 1, sizeof(int), 7, f) != 7) return 3;
      int* p = (int*)malloc(sizeof(int) * (size_t)(h[6] + h[7]) + 4);
      if (fread(p, sizeof(int), (size_t)(h[6] + h[7]), f) != (size_t)(h[6] + h[7])) return 3;
      // (eight slices of the range side by side, each with counters of its own: the enumeration is most of the run)
      enum { NT = 8 };
      long tb[NT] = {0}, tc[NT] = {0}, tcnt[NT][N_CNT] = {{0}};
      long long bad[NT][4];
      std::thread th[NT];
      for (int t = 0; t < NT; t++) {
        const long long lo = h[4] + (long long)(h[5] - h[4]) * t / NT, hi = h[4] + (long long)(h[5] - h[4]) * (t + 1) / NT;
        th[t] = std::thread([=, &tb, &tc, &tcnt, &bad] {
          tb[t] = ls_borders(h[1], h[2], 65536.0, 1.5, h[3], lo, hi, p, h[6], p + h[6], h[7], &tc[t], bad[t], tcnt[t]);
        });
      }
      for (int t = 0; t < NT; t++) {
        th[t].join();
        nbad += tb[t];
        cases += tc[t];
      }
      free(p);
    }
  }
  fclose(f);
  printf("cases %ld mismatches %ld\n", cases, nbad);
  return nbad != 0;
}
#endif
"""

FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc")]
SAN = ["-g", "-pthread", "-DTC_LINE_MAIN", "-fsanitize=undefined,address,float-cast-overflow,float-divide-by-zero", "-fno-sanitize-recover=all"]


def write_src(d):
    src = os.path.join(str(d), "line_setup_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d):
    """-> ctypes library of the shim built in directory d"""
    src, lib = write_src(d), os.path.join(str(d), "libtc_line_setup.so")
    subprocess.check_call(["c++"] + FLAGS + ["-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    ip, lp, llp = C.POINTER(C.c_int32), C.POINTER(C.c_long), C.POINTER(C.c_longlong)
    L.ls_segments.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, lp, lp]
    L.ls_segments.restype = C.c_long
    L.ls_borders.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_longlong, C.c_longlong, ip, C.c_int, ip, C.c_int,
                             lp, llp, lp]
    L.ls_borders.restype = C.c_long
    return L


def build_program(d):
    """-> path of the stand-alone program under UBSan (float conversions included) + ASan"""
    src, exe = write_src(d), os.path.join(str(d), "line_setup_san")
    subprocess.check_call(["c++"] + FLAGS + SAN + ["-o", exe, src])
    return exe


def segments(L, W, H, th, e_step, seg, cnt):
    """-> (mismatches, first mismatching segment or None); adds the literal form's branch counts to cnt"""
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    first = np.full(1, -1, dtype=np.int64)
    nbad = L.ls_segments(len(seg), W, H, th, e_step, seg.ctypes.data_as(C.POINTER(C.c_int32)), first.ctypes.data_as(C.POINTER(C.c_long)),
                         cnt.ctypes.data_as(C.POINTER(C.c_long)))
    return nbad, (seg[int(first[0])].tolist() if nbad else None)


def borders(L, W, H, octant, lo, hi, px, py, cnt):
    """-> (cases, mismatches, first mismatch) of ls_borders over dp's major component in [lo, hi)"""
    cases, bad = np.zeros(1, dtype=np.int64), np.zeros(4, dtype=np.int64)
    ip = C.POINTER(C.c_int32)
    nbad = L.ls_borders(W, H, 65536.0, 1.5, octant, lo, hi, px.ctypes.data_as(ip), len(px), py.ctypes.data_as(ip), len(py),
                        cases.ctypes.data_as(C.POINTER(C.c_long)), bad.ctypes.data_as(C.POINTER(C.c_longlong)),
                        cnt.ctypes.data_as(C.POINTER(C.c_long)))
    return int(cases[0]), nbad, bad.tolist()
