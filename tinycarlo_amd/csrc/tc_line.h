// Line2's set-up (drawing.cpp: clipLine on 16.16 end points, then the DDA parameters of one polygon-outline edge), and
// which of ThickLine's four outline edges the raster stage has to draw at all.
//
// Plain C++ / HIP like tc_clip.h and tc_fill.h: the tests build this header with the host compiler
// (tests/short_edges_shim.py), the kernels include it through tc_device.h.
//
// THE SHORT OUTLINE EDGES.  ThickLine(p0, p1, thickness) with integer pixel end points fills the quad
//   v0 = p0 + dp, v1 = p0 - dp, v2 = p1 - dp, v3 = p1 + dp        (16.16, |dp| = thickness / 2 px, rounded per component)
// with FillConvexPoly -- the four outline edges v3->v0, v0->v1, v1->v2, v2->v3 drawn with Line2, then the scanline
// fill -- and draws a filled circle of radius (thickness + 1) / 2 at p0 and at p1.  At thickness 2 the edges v0->v1 and
// v2->v3 are 2 px long and centred on an integer pixel, and they add nothing to the picture:
//
//   LEMMA (thickness 2).  The in-frame pixels of Line2(p + dp, p - dp) are a subset of the radius-1 cap at p (the plus
//   shape |dx| + |dy| <= 1) plus, for each end v = p +- dp that lies inside the clip rectangle [0, W << 16) x
//   [0, H << 16), the rounded end point (v + 0.5 px) >> 16.  A long edge has that v as one of ITS end points; clipLine
//   leaves an end inside the rectangle where it is, and Line2 draws both of its (clipped) end points -- one as the
//   step-0 pixel, the other as the far end pixel it writes explicitly.  The caps are drawn for every segment.  So
//   without the two short edges ThickLine paints the same pixels.
//
// tests/test_short_edges_cpu.py proves the lemma by enumeration -- every integer dp within 1.5 units of length 65536
// (a superset of what r_quad rounds to; closed under negation, which covers the edge v2->v3 = Line2(p1 - dp, p1 + dp)),
// p at every distance -3..+3 px from every border on both axes and far away from all of them -- and the statement about
// the long edges on random edges.  Nothing in it depends on the frame size beyond the two borders of an axis not
// interacting (every product and quotient of clipLine is taken on differences from the border being clipped against,
// so the arithmetic is the same at any W, H): frames of at least TC_SHORT_EDGES_MIN_DIM pixels per axis, where a point
// within 3 px of one border is at least 4 px from the other.  At thickness 3 and above the lemma is FALSE (a short edge
// clipped at a border can leave a pixel that neither the cap nor the fill reaches): tc_short_edges_skip says no, and so
// does the test.
#ifndef TC_LINE_H
#define TC_LINE_H
#include "tc_trig.h" /* TC_HD */

#ifndef TC_XY_SHIFT
#define TC_XY_SHIFT 16
#define TC_XY_ONE 65536
#endif

#define TC_SHORT_EDGES_MIN_DIM 8

// 1 = ThickLine at this thickness and frame size needs only its two long outline edges (the lemma above)
TC_HD int tc_short_edges_skip(int thickness, int W, int H) {
  return thickness == 2 && W >= TC_SHORT_EDGES_MIN_DIM && H >= TC_SHORT_EDGES_MIN_DIM;
}

// clipLine(Size2l, Point2l&, Point2l&)
TC_HD bool r_clip_line(long long width, long long height, long long& x1, long long& y1, long long& x2, long long& y2) {
  // clipLine() clips end 1 against the y range, then end 2 (against the already clipped end 1), then the same for x.
  // Under SIMT each of those four blocks (an f64 multiply + divide between int64 conversions) would be executed by
  // the whole wave as soon as one lane needs it.  Here ONE instance per axis serves whichever end needs it -- roles
  // are swapped for lanes where only end 2 does; (a-y2)*(x1-x2)/(y1-y2) equals (a-y2)*(x2-x1)/(y2-y1) bit for bit
  // because IEEE multiplication and division are sign-symmetric -- and a second instance runs only for lanes where
  // both ends need clipping on that axis (rare; skipped by the whole wave otherwise).
  int c1, c2;
  long long right = width - 1, bottom = height - 1;
  if (width <= 0 || height <= 0) return false;
  c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
  c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
  if ((c1 & c2) == 0 && (c1 | c2) != 0) {
    const bool n1 = (c1 & 12) != 0, n2 = (c2 & 12) != 0;
    if (n1 || n2) {
      const bool sw = !n1;  // only end 2 needs it: treat it as "the end to clip"
      long long xa = sw ? x2 : x1, ya = sw ? y2 : y1, xb = sw ? x1 : x2, yb = sw ? y1 : y2;
      const int ca = sw ? c2 : c1;
      const long long a = ca < 8 ? 0 : bottom;
      xa += (long long)((double)(a - ya) * (double)(xb - xa) / (double)(yb - ya));
      const int cn = (xa < 0) + (xa > right) * 2;
      if (sw) {
        x2 = xa;
        y2 = a;
        c2 = cn;
      } else {
        x1 = xa;
        y1 = a;
        c1 = cn;
      }
      if (n1 && n2) {  // both ends: end 2 against the clipped end 1
        const long long a2 = c2 < 8 ? 0 : bottom;
        x2 += (long long)((double)(a2 - y2) * (double)(x2 - x1) / (double)(y2 - y1));
        y2 = a2;
        c2 = (x2 < 0) + (x2 > right) * 2;
      }
    }
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
      const bool m1 = c1 != 0, m2 = c2 != 0;
      const bool sw = !m1;
      long long xa = sw ? x2 : x1, ya = sw ? y2 : y1, xb = sw ? x1 : x2, yb = sw ? y1 : y2;
      const int ca = sw ? c2 : c1;
      const long long a = ca == 1 ? 0 : right;
      ya += (long long)((double)(a - xa) * (double)(yb - ya) / (double)(xb - xa));
      if (sw) {
        x2 = a;
        y2 = ya;
        c2 = 0;
      } else {
        x1 = a;
        y1 = ya;
        c1 = 0;
      }
      if (m1 && m2) {
        const long long a2 = c2 == 1 ? 0 : right;
        y2 += (long long)((double)(a2 - x2) * (double)(y2 - y1) / (double)(x2 - x1));
        x2 = a2;
        c2 = 0;
      }
    }
  }
  return (c1 | c2) == 0;
}

// reciprocal estimate: the hardware's in the kernels; on the host the division (d_sdiv corrects either to the exact quotient)
TC_HD double tc_line_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_rcp(x);
#else
  return 1.0 / x;
#endif
}

// Truncating int64 division n / d (C semantics) for operands below 2^50 (always the case after clipping):
// several times cheaper than the 64-bit integer division sequence.
TC_HD long long d_sdiv(long long n, long long d) {
  long long an = n < 0 ? -n : n, ad = d < 0 ? -d : d;
  if (an < (1LL << 50) && ad < (1LL << 50)) {
    // quotient estimate from a hardware reciprocal (relative error ~2^-50: off by at most one for an < 2^50),
    // made exact by the remainder test -- the result is the true integer quotient, no rounding mode involved.
    // The remainder an - q * ad is taken with ONE fused multiply-add in double precision instead of a 64 x 64-bit
    // integer multiply (four quarter-rate v_mul / v_mad_u64_u32): an, ad and q are integers below 2^53, exact as doubles;
    // the fma forms q * ad exactly and rounds an - q * ad once, and that value is an integer of magnitude <= 2 ad < 2^51,
    // so the rounding is exact too.
    const double dn = (double)an, dd = (double)ad;
    double qd = __builtin_trunc(dn * tc_line_rcp(dd));
    double rd = __builtin_fma(-qd, dd, dn);
    if (rd < 0) {
      qd -= 1.0;
      rd += dd;
    }
    if (rd >= dd) qd += 1.0;
    const long long q = (long long)qd;
    return ((n < 0) != (d < 0)) ? -q : q;
  }
  return n / d;
}

// One polygon-outline edge after clipping, ready for random access by step index k (0..ecount):
//   x-major: pixel (a + k, (b + k*step) >> 16)        y-major: pixel ((b + k*step) >> 16, a + k)
// plus the far end point pixel (ex, ey) that Line2 writes first.
struct LineP {
  int a, b, step;
  int ecount;  // -1: edge invisible
  int ex, ey;
  int xmajor;
};

TC_HD LineP r_line2_setup(int W, int H, long long p1x, long long p1y, long long p2x, long long p2y) {
  LineP L;
  L.a = L.b = L.step = 0;
  L.ecount = -1;
  L.ex = L.ey = -1;
  L.xmajor = 0;
  if (!r_clip_line((long long)W << TC_XY_SHIFT, (long long)H << TC_XY_SHIFT, p1x, p1y, p2x, p2y)) return L;
  long long dx = p2x - p1x, dy = p2y - p1y;
  long long j = dx < 0 ? -1 : 0;
  long long ax = (dx ^ j) - j;
  long long i = dy < 0 ? -1 : 0;
  long long ay = (dy ^ i) - i;
  bool xmajor = ax > ay;
  long long step;
  if (xmajor) {
    dy = (dy ^ j) - j;
    if (j) {
      long long t = p1x; p1x = p2x; p2x = t;
      t = p1y; p1y = p2y; p2y = t;
    }
    step = d_sdiv(dy * TC_XY_ONE, ax | 1);
    L.ecount = (int)((p2x - p1x) >> TC_XY_SHIFT);
  } else {
    dx = (dx ^ i) - i;
    if (i) {
      long long t = p1x; p1x = p2x; p2x = t;
      t = p1y; p1y = p2y; p2y = t;
    }
    step = d_sdiv(dx * TC_XY_ONE, ay | 1);
    L.ecount = (int)((p2y - p1y) >> TC_XY_SHIFT);
  }
  p1x += (TC_XY_ONE >> 1);
  p1y += (TC_XY_ONE >> 1);
  L.ex = (int)((p2x + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT);
  L.ey = (int)((p2y + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT);
  L.xmajor = xmajor;
  L.step = (int)step;
  if (xmajor) {
    L.a = (int)(p1x >> TC_XY_SHIFT);
    L.b = (int)p1y;
  } else {
    L.a = (int)(p1y >> TC_XY_SHIFT);
    L.b = (int)p1x;
  }
  return L;
}

#endif  // TC_LINE_H
