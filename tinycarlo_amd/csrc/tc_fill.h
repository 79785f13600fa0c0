// FillConvexPoly's edge-walker events (drawing.cpp, the scanline loop of a convex quad) in two forms.
//
// The scanline loop is a sequence of "events" (a walker reaches the end row of its polygon edge and picks the next one,
// with a shared budget of npts edges) between which both walkers just add dx per row.  Both forms below run only the
// event part and record every new piece (start row, the two vertex indices of its edge, walker id); row r of walker w is
// then xs + (r - y_start) * dx of its latest piece.  At most 4 pieces: every new piece consumes one of the 4 edges.
//
//   tc_fill_events_literal   the loop nest as drawing.cpp has it: `guard`, two walkers, a scan per walker.  It is the
//                            specification (-DTC_FILL_LITERAL puts it back into the kernels).
//   tc_fill_events           the same function without a data-dependent loop or branch.
//
// Why a second form: the kernels run this with one lane per segment, every lane takes another path through the nest and
// the wavefront pays for the union of the paths.
//
// What makes it possible: past the integer prologue (bounding box, off-screen test, first minimum `imin`) the nest is a
// function of (imin, ty0..ty3, (int)ymax) alone -- tc_fill_walk_literal is that part on its own -- and every candidate
// edge it looks at, hit or miss, takes one unit of the budget of 4.  So the nest is a state machine that makes at most 4
// transitions "the active walker tests its next vertex"; tc_fill_walk makes exactly 4, unrolled, with selects:
//   - the active walker is walker 0 while y >= e_ye0, else walker 1 (the nest's order inside one row);
//   - a miss moves that walker's idx0 along (the nest does so in a local, but a scan only ends with a hit or with the
//     budget, and after the budget nothing reads idx0 again);
//   - when neither walker is active the row advances to min(e_ye0, e_ye1), or the loop is left (`done`) when that is
//     past ymax;
//   - a machine that is not `done` after 4 transitions has an active walker and no budget: the nest's `edges < 0`
//     exit, y_end = y.  (`guard < 8` never binds: every pass of the nest takes from the budget.)
//   - the piece is stored at slot np on every transition and np moves on a hit only, so a miss is overwritten: slots
//     [np, 4) hold leftovers, which no reader looks at.
// tests/test_fill_events_cpu.py compares the two forms on every order pattern of the six integers and on the quads
// r_quad emits.  Plain C++ / HIP like tc_clip.h: the tests build this header with the host compiler.
#ifndef TC_FILL_H
#define TC_FILL_H
#include "tc_trig.h" /* TC_HD */

#ifndef TC_XY_SHIFT
#define TC_XY_SHIFT 16
#define TC_XY_ONE 65536
#endif
#if defined(__clang__)
#define TC_FILL_UNROLL _Pragma("unroll")
#else
#define TC_FILL_UNROLL
#endif

TC_HD int tc_fill_wrap32(long long v) { return (int)(unsigned int)(unsigned long long)v; }

// The four polygon vertices travel as BY-VALUE scalars.  Any aggregate (array or struct behind a
// reference) lets LLVM fold "select of loads" into "load of selected pointer", which pins the
// aggregate in scratch memory -- and scratch write-back shows up as HBM traffic.
TC_HD long long tc_fill_sel4(long long a0, long long a1, long long a2, long long a3, int i) {
  long long r = a0;
  r = i == 1 ? a1 : r;
  r = i == 2 ? a2 : r;
  r = i == 3 ? a3 : r;
  return r;
}
TC_HD int tc_fill_sel4i(int a0, int a1, int a2, int a3, int i) {
  int r = a0;
  r = i == 1 ? a1 : r;
  r = i == 2 ? a2 : r;
  r = i == 3 ? a3 : r;
  return r;
}

//   py/pv: tables [4]; returns number of pieces; wmask bit s = walker of piece s;
//   rows [y_first, y_last] are the ones the fill draws (empty when y_last < y_first).
TC_HD int tc_fill_events_literal(int W, int H, long long qx0, long long qx1, long long qx2, long long qx3,
                                 long long qy0, long long qy1, long long qy2, long long qy3, int* py, int* pv,
                                 int& wmask, int& y_first, int& y_last) {
  // Integer-only part: which polygon edge each walker switches to at which row.  pv[s] = idx0 | idx << 2
  // (xs = vx[idx0], xe = vx[idx], end row = ty[idx]); the slope of piece s is computed by r_fill_slope.
  const int npts = 4, shift = TC_XY_SHIFT;
  const int delta = 1 << shift >> 1;
  wmask = 0;
  y_first = 0;
  y_last = -1;
  int imin = 0;
  long long xmin = qx0, xmax = qx0, ymin = qy0, ymax = qy0;
TC_FILL_UNROLL
  for (int i = 1; i < npts; i++) {
    long long x = tc_fill_sel4(qx0, qx1, qx2, qx3, i), y = tc_fill_sel4(qy0, qy1, qy2, qy3, i);
    if (y < ymin) {
      ymin = y;
      imin = i;
    }
    if (y > ymax) ymax = y;
    if (x > xmax) xmax = x;
    if (x < xmin) xmin = x;
  }
  xmin = (xmin + delta) >> shift;
  xmax = (xmax + delta) >> shift;
  ymin = (ymin + delta) >> shift;
  ymax = (ymax + delta) >> shift;
  if (tc_fill_wrap32(xmax) < 0 || tc_fill_wrap32(ymax) < 0 || tc_fill_wrap32(xmin) >= W || tc_fill_wrap32(ymin) >= H) return 0;
  if (ymax > H - 1) ymax = H - 1;
  const int ty0 = tc_fill_wrap32((qy0 + delta) >> shift), ty1 = tc_fill_wrap32((qy1 + delta) >> shift);
  const int ty2 = tc_fill_wrap32((qy2 + delta) >> shift), ty3 = tc_fill_wrap32((qy3 + delta) >> shift);
  int y = tc_fill_wrap32(ymin);
  int e_idx0 = imin, e_idx1 = imin, e_ye0 = y, e_ye1 = y;
  int edges = npts, np = 0;
  int y_end = (int)ymax + 1;
  for (int guard = 0; guard < 8; guard++) {
TC_FILL_UNROLL
    for (int i = 0; i < 2; i++) {
      const int ye = i ? e_ye1 : e_ye0;
      if (y >= ye) {
        int idx0 = i ? e_idx1 : e_idx0;
        const int di = i ? npts - 1 : 1;
        int idx = idx0 + di;
        if (idx >= npts) idx -= npts;
        for (; edges-- > 0;) {  // (a straight-line 4-candidate version of this scan was tried: 25 % more instructions)
          int ty = idx == 0 ? ty0 : idx == 1 ? ty1 : idx == 2 ? ty2 : ty3;
          if (ty > y) {
            py[np] = y;
            pv[np] = idx0 | (idx << 2);
            wmask |= i << np;
            np++;
            if (i) {
              e_ye1 = ty;
              e_idx1 = idx;
            } else {
              e_ye0 = ty;
              e_idx0 = idx;
            }
            break;
          }
          idx0 = idx;
          idx += di;
          if (idx >= npts) idx -= npts;
        }
      }
    }
    if (edges < 0) {
      y_end = y;
      break;
    }
    int ynext = e_ye0 < e_ye1 ? e_ye0 : e_ye1;
    if (ynext > (int)ymax) break;
    y = ynext;
  }
  y_first = tc_fill_wrap32(ymin) > 0 ? tc_fill_wrap32(ymin) : 0;
  y_last = y_end - 1 < (int)ymax ? y_end - 1 : (int)ymax;
  return np;
}

// The part of tc_fill_events_literal behind its off-screen return, on the values that reach it: the first minimum
// `imin`, the four wrapped vertex rows and ymaxi = (int)ymax after the clip to H - 1.  (`ymin` there is vertex imin's
// row, shifted and wrapped: ty[imin].)  Same statements otherwise.
TC_HD int tc_fill_walk_literal(int imin, int ty0, int ty1, int ty2, int ty3, int ymaxi, int* py, int* pv, int& wmask,
                               int& y_first, int& y_last) {
  const int npts = 4;
  wmask = 0;
  int y = tc_fill_sel4i(ty0, ty1, ty2, ty3, imin);
  const int ymin = y;
  int e_idx0 = imin, e_idx1 = imin, e_ye0 = y, e_ye1 = y;
  int edges = npts, np = 0;
  int y_end = ymaxi + 1;
  for (int guard = 0; guard < 8; guard++) {
TC_FILL_UNROLL
    for (int i = 0; i < 2; i++) {
      const int ye = i ? e_ye1 : e_ye0;
      if (y >= ye) {
        int idx0 = i ? e_idx1 : e_idx0;
        const int di = i ? npts - 1 : 1;
        int idx = idx0 + di;
        if (idx >= npts) idx -= npts;
        for (; edges-- > 0;) {
          int ty = idx == 0 ? ty0 : idx == 1 ? ty1 : idx == 2 ? ty2 : ty3;
          if (ty > y) {
            py[np] = y;
            pv[np] = idx0 | (idx << 2);
            wmask |= i << np;
            np++;
            if (i) {
              e_ye1 = ty;
              e_idx1 = idx;
            } else {
              e_ye0 = ty;
              e_idx0 = idx;
            }
            break;
          }
          idx0 = idx;
          idx += di;
          if (idx >= npts) idx -= npts;
        }
      }
    }
    if (edges < 0) {
      y_end = y;
      break;
    }
    int ynext = e_ye0 < e_ye1 ? e_ye0 : e_ye1;
    if (ynext > ymaxi) break;
    y = ynext;
  }
  y_first = ymin > 0 ? ymin : 0;
  y_last = y_end - 1 < ymaxi ? y_end - 1 : ymaxi;
  return np;
}

// The integer prologue: bounding box, off-screen test, first minimum, the four wrapped rows, the clipped last row.
// Minimum and maximum of four come from one compare per pair plus one each between the pairs (4 compares of 64-bit
// values per axis instead of 6); strict `<` everywhere keeps the FIRST minimum, as the literal scan does.
// Returns 1 when the literal form returns 0 before its loop.
TC_HD int tc_fill_prologue(int W, int H, long long qx0, long long qx1, long long qx2, long long qx3, long long qy0,
                           long long qy1, long long qy2, long long qy3, int& imin, int& ty0, int& ty1, int& ty2,
                           int& ty3, int& ymaxi) {
  const int shift = TC_XY_SHIFT;
  const int delta = 1 << shift >> 1;
  const bool x10 = qx1 < qx0, x32 = qx3 < qx2;
  const long long xlo01 = x10 ? qx1 : qx0, xhi01 = x10 ? qx0 : qx1;
  const long long xlo23 = x32 ? qx3 : qx2, xhi23 = x32 ? qx2 : qx3;
  const long long xmin = xlo23 < xlo01 ? xlo23 : xlo01, xmax = xhi23 > xhi01 ? xhi23 : xhi01;
  const bool y10 = qy1 < qy0, y32 = qy3 < qy2;
  const long long ylo01 = y10 ? qy1 : qy0, yhi01 = y10 ? qy0 : qy1;
  const long long ylo23 = y32 ? qy3 : qy2, yhi23 = y32 ? qy2 : qy3;
  const bool ym = ylo23 < ylo01;
  const long long ymin = ym ? ylo23 : ylo01, ymax = yhi23 > yhi01 ? yhi23 : yhi01;
  imin = ym ? (y32 ? 3 : 2) : (y10 ? 1 : 0);
  const long long ymaxs = (ymax + delta) >> shift;
  const int off = (int)(tc_fill_wrap32((xmax + delta) >> shift) < 0) | (int)(tc_fill_wrap32(ymaxs) < 0) |
                  (int)(tc_fill_wrap32((xmin + delta) >> shift) >= W) | (int)(tc_fill_wrap32((ymin + delta) >> shift) >= H);
  ymaxi = ymaxs > H - 1 ? H - 1 : tc_fill_wrap32(ymaxs);
  ty0 = tc_fill_wrap32((qy0 + delta) >> shift);
  ty1 = tc_fill_wrap32((qy1 + delta) >> shift);
  ty2 = tc_fill_wrap32((qy2 + delta) >> shift);
  ty3 = tc_fill_wrap32((qy3 + delta) >> shift);
  return off;
}

// tc_fill_walk_literal as four unrolled transitions (see the top of the file).  `off`: nothing to walk, the outputs
// are those of the literal form's early return.  Writes py[0..3] / pv[0..3]; entries [np, 4) are leftovers.
TC_HD int tc_fill_walk(int imin, int ty0, int ty1, int ty2, int ty3, int ymaxi, int off, int* py, int* pv, int& wmask,
                       int& y_first, int& y_last) {
  const int ymin = tc_fill_sel4i(ty0, ty1, ty2, ty3, imin);
  int y = ymin, ye0 = ymin, ye1 = ymin, i0 = imin, i1 = imin;
  int np = 0, wm = 0;
  int done = off;  // the scanline loop was left through `ynext > ymax`
TC_FILL_UNROLL
  for (int k = 0; k < 4; k++) {
    const int w = y < ye0;  // the active walker (not done: y >= ye0 or y >= ye1)
    const int idx0 = w ? i1 : i0;
    const int idx = (idx0 + 1 + 2 * w) & 3;
    const int ty = tc_fill_sel4i(ty0, ty1, ty2, ty3, idx);
    const int hit = (ty > y) & (done ^ 1);
    py[np] = y;
    pv[np] = idx0 | (idx << 2);
    wm |= (w & hit) << np;
    np += hit;
    i0 = w ? i0 : idx;
    i1 = w ? idx : i1;
    ye0 = (hit & (w ^ 1)) ? ty : ye0;
    ye1 = (hit & w) ? ty : ye1;
    const int ynext = ye0 < ye1 ? ye0 : ye1;
    const int idle = y < ynext;  // neither walker active: the row loop moves on
    done |= idle & (ynext > ymaxi);
    y = idle ? ynext : y;
  }
  // not done: a walker is active and the budget is spent -- the literal form's `edges < 0`, y_end = y
  const int yl = (int)((unsigned int)y - 1u);
  wmask = wm;
  y_first = off ? 0 : (ymin > 0 ? ymin : 0);
  y_last = off ? -1 : (done || ymaxi < yl ? ymaxi : yl);
  return np;
}

TC_HD int tc_fill_events(int W, int H, long long qx0, long long qx1, long long qx2, long long qx3, long long qy0,
                         long long qy1, long long qy2, long long qy3, int* py, int* pv, int& wmask, int& y_first,
                         int& y_last) {
  int imin, ty0, ty1, ty2, ty3, ymaxi;
  const int off = tc_fill_prologue(W, H, qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3, imin, ty0, ty1, ty2, ty3, ymaxi);
  return tc_fill_walk(imin, ty0, ty1, ty2, ty3, ymaxi, off, py, pv, wmask, y_first, y_last);
}

#endif  // TC_FILL_H
