// ThickLine's quad and Line2's set-up (drawing.cpp: clipLine on 16.16 end points, then the DDA parameters of one
// polygon-outline edge), and which of ThickLine's four outline edges the raster stage has to draw at all.
//
// Plain C++ / HIP like tc_clip.h and tc_fill.h: the tests build this header with the host compiler
// (tests/short_edges_shim.py, tests/line_setup_shim.py), the kernels include it through tc_device.h.
//
// Two forms of the set-up live here.  The LITERAL one -- r_clip_line, r_line2_setup_literal, r_quad_literal: int64
// end points as in drawing.cpp -- is the specification.  The kernels run r_clip_line_f, r_line2_setup_f and r_quad_dp:
// end points as exact-integer doubles through the clip, plain 32-bit arithmetic behind it; the argument that they
// compute the same stands at r_clip_line_f, and tests/test_line_setup_cpu.py compares them.  -DTC_LINE_LITERAL
// (make LINE=literal) builds the literal forms back into r_line2_setup, r_quad_dp and r_outline_edge.
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

// clipLine on end points carried as EXACT-INTEGER DOUBLES: the form the kernels run (r_clip_line above is its
// specification, and -DTC_LINE_LITERAL builds it back in).  gfx950 has no 64-bit integer multiply and no int64 <-> f64
// conversion instruction; the literal spends most of its instructions emulating them around four f64 operations.
// Here the end points never leave f64: same blocks, same f64 multiply and divide in the same order (no contraction: the
// header is built with -ffp-contract=off and uses no fma in the clip), and
//   (double)(a - ya)       becomes   a - ya         taken in f64
//   xa += (long long)q     becomes   xa += trunc(q)
//   the outcodes           become    f64 compares.
// right = (W << 16) - 1, bottom = (H << 16) - 1 (W, H >= 1: the literal's empty-rectangle test has nothing to do).
//
// WHY THIS IS THE SAME FUNCTION.  Precondition: every input coordinate is an integer of magnitude below 2^48 -- the
// outline vertices are int32 * 65536 +- dp with |dp| < 2^24 (thickness <= 255), at most 2^47 + 2^24 -- and 0 <= right,
// bottom < 2^31.
//  (1) A block clips an end (xa, ya) that lies outside border a of one axis against the other end (xb, yb), which does
//      not lie outside that border (the outcodes share no bit), so a is between ya and yb: |a - ya| <= |yb - ya| and
//      yb != ya.  With m = a - ya, n = xb - xa, d = yb - ya the block computes q = fl(fl(m * n) / d), and
//      |q| <= fl(fl(|d| |n|) / |d|), which is |n| or a neighbouring double of it: rounding is monotonic, and |n| < 2^50
//      has doubles spaced at most 2^-3 apart around it.  So |trunc(q)| <= |n| with the sign of n (or zero): the clipped
//      coordinate xa + trunc(q) lies between xa and xb.  By induction over the (at most four) blocks every coordinate
//      stays an integer of magnitude below 2^48, every difference below 2^49.
//  (2) Integers below 2^53 are exact as doubles, and so are their sums and differences while those stay below 2^53:
//      a - ya, xb - xa, yb - ya taken in f64 equal the literal's int64 differences converted, and xa + trunc(q) equals
//      the literal's int64 sum.  The multiply and the divide then see the same operands and round the same way.
//  (3) |q| < 2^50 is far inside int64, so (long long)q is trunc(q), exactly.
//  (4) f64 compares of exact integers against 0 and right / bottom give the literal's outcodes.
// After an accepted clip all four coordinates lie in [0, right] x [0, bottom]: each end was inside on an axis or has
// been put on its border, and by (1) the x blocks move y only between two in-range values.
// tests/test_line_setup_cpu.py compares the two forms, with every branch of the literal counted.
TC_HD bool r_clip_line_f(double right, double bottom, double& x1, double& y1, double& x2, double& y2) {
  int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
  int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
  if ((c1 & c2) == 0 && (c1 | c2) != 0) {
    const bool n1 = (c1 & 12) != 0, n2 = (c2 & 12) != 0;
    if (n1 || n2) {
      const bool sw = !n1;
      double xa = sw ? x2 : x1, ya = sw ? y2 : y1, xb = sw ? x1 : x2, yb = sw ? y1 : y2;
      const int ca = sw ? c2 : c1;
      const double a = ca < 8 ? 0.0 : bottom;
      xa += __builtin_trunc((a - ya) * (xb - xa) / (yb - ya));
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
      if (n1 && n2) {
        const double a2 = c2 < 8 ? 0.0 : bottom;
        x2 += __builtin_trunc((a2 - y2) * (x2 - x1) / (y2 - y1));
        y2 = a2;
        c2 = (x2 < 0) + (x2 > right) * 2;
      }
    }
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
      const bool m1 = c1 != 0, m2 = c2 != 0;
      const bool sw = !m1;
      double xa = sw ? x2 : x1, ya = sw ? y2 : y1, xb = sw ? x1 : x2, yb = sw ? y1 : y2;
      const int ca = sw ? c2 : c1;
      const double a = ca == 1 ? 0.0 : right;
      ya += __builtin_trunc((a - xa) * (yb - ya) / (xb - xa));
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
        const double a2 = c2 == 1 ? 0.0 : right;
        y2 += __builtin_trunc((a2 - x2) * (y2 - y1) / (x2 - x1));
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

// Line2's set-up as drawing.cpp has it, on int64 16.16 end points: the specification of r_line2_setup_f below
TC_HD LineP r_line2_setup_literal(int W, int H, long long p1x, long long p1y, long long p2x, long long p2y) {
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


// trunc(n * 65536 / d) for |n| <= d < 2^31, d > 0: d_sdiv's reciprocal path fed from the int32 operands.  dn = |n| * 65536.0
// is exact (below 2^47), the quotient is at most 65536, so an estimate with a relative error below 2^-17 is within one of
// it and the fma remainder (exact, as in d_sdiv) settles which.
TC_HD int r_step32(int n, int d) {
  const int an = n < 0 ? -n : n;
  const double dn = (double)an * (double)TC_XY_ONE, dd = (double)d;
  double qd = __builtin_trunc(dn * tc_line_rcp(dd));
  double rd = __builtin_fma(-qd, dd, dn);
  if (rd < 0) {
    qd -= 1.0;
    rd += dd;
  }
  if (rd >= dd) qd += 1.0;
  const int q = (int)qd;
  return n < 0 ? -q : q;
}

// Line2's set-up on end points carried as exact-integer doubles (|coordinate| < 2^48, see r_clip_line_f): the clip in
// f64, and behind it plain 32-bit arithmetic.  An accepted clip leaves all four coordinates in [0, W << 16) x
// [0, H << 16), and tc_env_create accepts no frame above 16384 x 16384, so they fit int32 with room for the + 32768
// (this form needs W, H < 32768; there is no wider frame to keep the literal form for).  dx, dy, their absolute values,
// ecount and the rounded end points are then the literal's values in 32 bits; dy * 65536 alone does not fit, and the
// step comes from r_step32.
TC_HD LineP r_line2_setup_f(int W, int H, double ax, double ay, double bx, double by) {
  LineP L;
  L.a = L.b = L.step = 0;
  L.ecount = -1;
  L.ex = L.ey = -1;
  L.xmajor = 0;
  if (!r_clip_line_f((double)W * (double)TC_XY_ONE - 1.0, (double)H * (double)TC_XY_ONE - 1.0, ax, ay, bx, by)) return L;
  int p1x = (int)ax, p1y = (int)ay, p2x = (int)bx, p2y = (int)by;
  int dx = p2x - p1x, dy = p2y - p1y;
  const int j = dx < 0 ? -1 : 0;
  const int adx = (dx ^ j) - j;
  const int i = dy < 0 ? -1 : 0;
  const int ady = (dy ^ i) - i;
  const bool xmajor = adx > ady;
  const int sw = xmajor ? j : i;  // the end points change places so that the major axis runs upwards
  if (sw) {
    int t = p1x; p1x = p2x; p2x = t;
    t = p1y; p1y = p2y; p2y = t;
  }
  L.step = r_step32(xmajor ? (dy ^ j) - j : (dx ^ i) - i, (xmajor ? adx : ady) | 1);
  L.ecount = (xmajor ? adx : ady) >> TC_XY_SHIFT;  // (p2 - p1 on the major axis after the swap: its absolute value)
  p1x += (TC_XY_ONE >> 1);
  p1y += (TC_XY_ONE >> 1);
  L.ex = (p2x + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT;
  L.ey = (p2y + (TC_XY_ONE >> 1)) >> TC_XY_SHIFT;
  L.xmajor = xmajor;
  L.a = (xmajor ? p1x : p1y) >> TC_XY_SHIFT;
  L.b = xmajor ? p1y : p1x;
  return L;
}

// Line2's set-up on int64 end points of magnitude below 2^48 (every caller's: see r_clip_line_f)
TC_HD LineP r_line2_setup(int W, int H, long long p1x, long long p1y, long long p2x, long long p2y) {
#ifdef TC_LINE_LITERAL
  return r_line2_setup_literal(W, H, p1x, p1y, p2x, p2y);
#else
  return r_line2_setup_f(W, H, (double)p1x, (double)p1y, (double)p2x, (double)p2y);
#endif
}

// sqrt and round-to-nearest-even to int: the kernels' own calls on the device, libm's on the host
TC_HD double tc_line_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  return sqrt(x);
#else
  return __builtin_sqrt(x);
#endif
}
TC_HD int tc_line_rint(double x) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  return __double2int_rn(x);
#else
  return (int)__builtin_rint(x);
#endif
}

// ThickLine's quad for thickness > 1 as drawing.cpp makes it, int64 16.16 vertices: returns false when the segment is
// degenerate (|r| <= DBL_EPSILON).  The specification of r_quad_dp.
TC_HD bool r_quad_literal(int x0, int y0, int x1, int y1, int thickness, long long& qx0, long long& qx1, long long& qx2,
                          long long& qx3, long long& qy0, long long& qy1, long long& qy2, long long& qy3) {
  long long p0x = (long long)x0 * TC_XY_ONE, p0y = (long long)y0 * TC_XY_ONE;
  long long p1x = (long long)x1 * TC_XY_ONE, p1y = (long long)y1 * TC_XY_ONE;
  const double INV_XY_ONE = 1. / TC_XY_ONE;
  double dx = (double)(p0x - p1x) * INV_XY_ONE, dy = (double)(p1y - p0y) * INV_XY_ONE;
  double rr = dx * dx + dy * dy;
  int odd = thickness & 1;
  long long th = (long long)thickness << (TC_XY_SHIFT - 1);
  if (!(tc_fabs(rr) > 2.2204460492503131e-16)) return false;
  rr = ((double)th + odd * TC_XY_ONE * 0.5) / tc_line_sqrt(rr);
  long long dpx = tc_line_rint(dy * rr), dpy = tc_line_rint(dx * rr);
  qx0 = p0x + dpx; qx1 = p0x - dpx; qx2 = p1x - dpx; qx3 = p1x + dpx;
  qy0 = p0y + dpy; qy1 = p0y - dpy; qy2 = p1y - dpy; qy3 = p1y + dpy;
  return true;
}

// The quad as (pixel end points, dp): v0 = p0 + dp, v1 = p0 - dp, v2 = p1 - dp, v3 = p1 + dp with p = pixel * 65536.
// (double)x0 - (double)x1 is the exact integer x0 - x1 (below 2^32), and so is (double)(p0x - p1x) * 2^-16 -- the int64
// difference is (x0 - x1) * 65536, below 2^48, and the scaling is by a power of two: bit-equal, without the int64 -> f64
// conversion.  |dp| <= thickness * 32768 + 32768 + 1 < 2^24 per component.
TC_HD bool r_quad_dp(int x0, int y0, int x1, int y1, int thickness, int& dpx, int& dpy) {
#ifdef TC_LINE_LITERAL
  long long qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3;
  if (!r_quad_literal(x0, y0, x1, y1, thickness, qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3)) return false;
  dpx = (int)(qx0 - (long long)x0 * TC_XY_ONE);
  dpy = (int)(qy0 - (long long)y0 * TC_XY_ONE);
  return true;
#else
  const double dx = (double)x0 - (double)x1, dy = (double)y1 - (double)y0;
  double rr = dx * dx + dy * dy;
  if (!(tc_fabs(rr) > 2.2204460492503131e-16)) return false;
  rr = (double)((thickness << (TC_XY_SHIFT - 1)) + (thickness & 1) * (TC_XY_ONE >> 1)) / tc_line_sqrt(rr);
  dpx = tc_line_rint(dy * rr);
  dpy = tc_line_rint(dx * rr);
  return true;
#endif
}

// The int64 vertices of (pixel end points, dp), for the fill (tc_fill.h keeps its int64 interface)
TC_HD void r_quad_vertices(int x0, int y0, int x1, int y1, int dpx, int dpy, long long& qx0, long long& qx1, long long& qx2,
                           long long& qx3, long long& qy0, long long& qy1, long long& qy2, long long& qy3) {
  const long long p0x = (long long)x0 * TC_XY_ONE, p0y = (long long)y0 * TC_XY_ONE;
  const long long p1x = (long long)x1 * TC_XY_ONE, p1y = (long long)y1 * TC_XY_ONE;
  qx0 = p0x + dpx; qx1 = p0x - dpx; qx2 = p1x - dpx; qx3 = p1x + dpx;
  qy0 = p0y + dpy; qy1 = p0y - dpy; qy2 = p1y - dpy; qy3 = p1y + dpy;
}

// Outline edge e of the quad (pixel end points, dp), set up for drawing.  FillConvexPoly walks p0 = v[3]; Line2(p0, v[i]);
// p0 = v[i]: edge e runs v[e-1] -> v[e].  The vertices are formed from their int32 parts: as int64 sums for the literal
// set-up, and for the f64 one as (double)pixel * 65536.0 + (double)(+-dp) -- a product below 2^47 and a sum below 2^48 of
// integers, both exact.
TC_HD LineP r_outline_edge(int W, int H, int x0, int y0, int x1, int y1, int dpx, int dpy, int e) {
  const bool a_is_p1 = e == 0 || e == 3, b_is_p1 = e >= 2;
  const bool a_minus = e == 2 || e == 3, b_minus = e == 1 || e == 2;
  const int apx = a_is_p1 ? x1 : x0, apy = a_is_p1 ? y1 : y0, bpx = b_is_p1 ? x1 : x0, bpy = b_is_p1 ? y1 : y0;
  const int adx = a_minus ? -dpx : dpx, ady = a_minus ? -dpy : dpy, bdx = b_minus ? -dpx : dpx, bdy = b_minus ? -dpy : dpy;
#ifdef TC_LINE_LITERAL
  return r_line2_setup_literal(W, H, (long long)apx * TC_XY_ONE + adx, (long long)apy * TC_XY_ONE + ady,
                               (long long)bpx * TC_XY_ONE + bdx, (long long)bpy * TC_XY_ONE + bdy);
#else
  const double one = (double)TC_XY_ONE;
  return r_line2_setup_f(W, H, (double)apx * one + (double)adx, (double)apy * one + (double)ady,
                         (double)bpx * one + (double)bdx, (double)bpy * one + (double)bdy);
#endif
}

#endif  // TC_LINE_H
