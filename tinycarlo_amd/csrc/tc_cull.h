// Whole-frame cull in front of the camera stage: "this frame's draw list is empty" decided from the pose alone.
//
// camera.py:52-97 draws an edge iff one of its ends is in idx = in_frame & idx_front & idx_in_range.  DESIGN.md section 4
// ("Whole-frame cull") proves: under the conditions the planner and the cover function check (H1-H3 below) and the
// per-frame guard G, the final ground position of every node of idx lies within TC_CULL_SLACK of a lane-line EDGE
// SEGMENT of the map and inside the visible ground footprint F of the camera.  So when F, placed at the car's pose,
// keeps more than the slack away from every segment, idx is empty and so is the draw list.
//
//   H1  every lane-line edge is shorter than max_range - 1 mm: no edge joins a node at or behind the camera plane to a
//       node beyond the far plane, so what passes 1 / 2 move (to z = -1e-7) never takes part in passes 3 / 4
//   H2  the camera centre is more than 1e-6 * |frame cone| above the ground: a ground point at depth 1e-7 is never in frame
//   H3  no node with two in-edges has an in-neighbour with two out-edges: there pass 4 moves a node along a line through
//       two points that pass 3 / 4 put ON the far plane, 0 / 0 in exact arithmetic -- rounding noise decides where it lands
//   G   "special" nodes (out-neighbours of a node with >= 2 out-edges, in-neighbours of a node with >= 2 in-edges: the
//       only nodes a second move of one target, or a move along an already moved end, can read) keep
//       |depth + max_range| >= TC_CULL_GUARD in this frame; then those moves have t = 1 + O(1e-5) or t = O(1e-5)
//
// The pieces: (a) tc_cull_plan -- a uniform grid over the segments plus a margin, one saturating uint8 per cell: a lower
// bound, in cells, of the distance from ANY point of the cell to the nearest segment; camera independent.
// (b) tc_cull_cover -- F as a convex polygon in the car's frame from E, K, W, H, max_range, covered by TC_CULL_NC circles
// (F cut into depth slabs, the smallest enclosing circle of each), centres stored in CAMERA coordinates.
// (c) the predicate -- world position of a centre from the 3x4 pose row itself, R^T (c_cam - t), its cell's bound
// against the radius.  "maybe" wherever anything is not guaranteed: NaN, far coordinates, outside the grid with a
// margin below the radius, guard G.
// HIP-free like tc_clip.h / tc_fill.h / tc_plan.h: tests/test_frame_cull_cpu.py builds it with the host compiler.
#ifndef TC_CULL_H
#define TC_CULL_H
#include "tc_trig.h" /* TC_HD */

#ifndef TC_CULL_NC
#define TC_CULL_NC 2  // circles of the cover (profiles/r06/frame_cull_shares_cpu.json: 1, 2, 3 compared)
#endif
#define TC_CULL_MAX_SPECIAL 16
#define TC_CULL_SLACK 1e-4      // metres, times max(1, max_range): see the error budget in DESIGN.md
#define TC_CULL_GUARD 1e-6      // metres of depth: guard G
#define TC_CULL_MAX_COORD 1e4   // |world coordinate of a cover centre| beyond which the answer is "maybe"
#define TC_CULL_MAX_CELLS (1 << 18)

struct TcCullHead {  // the table's header; the cells follow it in the device buffer
  double x0, y0, inv, cell;  // cell (ix, iy) = floor((p - origin) * inv), row-major, nx per row
  double margin;             // the grid reaches this far beyond the segments' bounding box
  double lmax;               // longest lane-line edge (H1)
  int nx, ny;                // 0: no table (H3 fails, too many special nodes, empty or non-finite map): always "maybe"
  int n_special, pad;
  double special[TC_CULL_MAX_SPECIAL][2];
};
#define TC_CULL_HEAD_BYTES 320
static_assert(sizeof(TcCullHead) <= TC_CULL_HEAD_BYTES, "the cells start TC_CULL_HEAD_BYTES into the buffer");

struct TcCullCover {
  int on, pad;               // 0: the cull is off for this camera (H1, H2, a K or E the derivation does not cover)
  double max_range;
  double c[TC_CULL_NC][3];   // circle centres, camera coordinates (E @ [cx, cy, 0, 1])
  double r[TC_CULL_NC];      // radii, slack included
  double car[TC_CULL_NC][2]; // the centres in the car's frame (host / tests only)
};

// ---- (c) the predicate, piece by piece (the kernels run the same pieces with scalar loads in between)
// world ground position of camera-frame point c for the pose row [R | t]
TC_HD void tc_cull_world(const double* pose, const double* c, double* wx, double* wy) {
  const double d0 = c[0] - pose[3], d1 = c[1] - pose[7], d2 = c[2] - pose[11];
  *wx = __builtin_fma(pose[8], d2, __builtin_fma(pose[4], d1, pose[0] * d0));
  *wy = __builtin_fma(pose[9], d2, __builtin_fma(pose[5], d1, pose[1] * d0));
}
#define TC_CULL_CELL_MAYBE (-1)
#define TC_CULL_CELL_CLEAR (-2)
// cell of world point (wx, wy), TC_CULL_CELL_CLEAR: outside the grid, the margin alone keeps radius r free,
// TC_CULL_CELL_MAYBE: no answer (every comparison is written so that a NaN ends here)
TC_HD int tc_cull_cell(const TcCullHead& h, double wx, double wy, double r) {
  if (!(tc_fabs(wx) <= TC_CULL_MAX_COORD && tc_fabs(wy) <= TC_CULL_MAX_COORD) || h.nx <= 0) return TC_CULL_CELL_MAYBE;
  const double fx = (wx - h.x0) * h.inv, fy = (wy - h.y0) * h.inv;
  // outside: more than the margin from every segment -- less the rounding of fx, fy, for which a whole cell is taken off;
  // a point that rounding puts INTO a border cell from just outside is covered by the 1e-9 the planner takes off a cell
  if (!(fx >= 0.0 && fy >= 0.0 && fx < (double)h.nx && fy < (double)h.ny))
    return (r + h.cell <= h.margin) ? TC_CULL_CELL_CLEAR : TC_CULL_CELL_MAYBE;
  return (int)fy * h.nx + (int)fx;
}
TC_HD int tc_cull_free(const TcCullHead& h, int q, double r) { return (double)q * h.cell >= r; }
// guard G: 1 = no special node is within TC_CULL_GUARD of the far plane
TC_HD int tc_cull_guard(const TcCullHead& h, const double* pose, double max_range) {
  int ok = 1;
  for (int i = 0; i < h.n_special && i < TC_CULL_MAX_SPECIAL; i++) {
    const double z = __builtin_fma(pose[9], h.special[i][1], __builtin_fma(pose[8], h.special[i][0], pose[11]));
    ok &= tc_fabs(z + max_range) >= TC_CULL_GUARD;  // (NaN: 0)
  }
  return ok;
}
// the whole predicate: 1 = the frame's draw list is empty, 0 = maybe not
TC_HD int tc_cull_empty(const TcCullHead& h, const unsigned char* cells, const TcCullCover& cv, const double* pose) {
  if (!cv.on || h.nx <= 0) return 0;
  for (int i = 0; i < TC_CULL_NC; i++) {
    double wx, wy;
    tc_cull_world(pose, cv.c[i], &wx, &wy);
    const int cell = tc_cull_cell(h, wx, wy, cv.r[i]);
    if (cell == TC_CULL_CELL_MAYBE) return 0;
    if (cell >= 0 && !tc_cull_free(h, cells[cell], cv.r[i])) return 0;
  }
  return tc_cull_guard(h, pose, cv.max_range);
}

// ---- the verdict as it travels in a pose row (entry TC_CULL_ROW_ENTRY of the row, k_camera.h): the simulate stage evaluates
// the predicate once per (step, env) on the pose it stores, and the frame kernels read the answer instead of evaluating it
// again on 64 lanes.  An 8-byte word like the pose entries, and like them never all ones ("not written yet").  Only the one
// word "culled" skips a frame: whatever else the memory holds decodes as "draw", which is always right.
#define TC_CULL_ROW_ENTRY 13
#define TC_CULL_ROW_DRAW 0ull
#define TC_CULL_ROW_CULLED 1ull
TC_HD unsigned long long tc_cull_row_encode(int empty) { return empty ? TC_CULL_ROW_CULLED : TC_CULL_ROW_DRAW; }
TC_HD int tc_cull_row_decode(unsigned long long w) { return w == TC_CULL_ROW_CULLED; }
// the word a pose-row writer stores for `pose`
TC_HD unsigned long long tc_cull_row_verdict(const TcCullHead& h, const unsigned char* cells, const TcCullCover& cv, const double* pose) {
  return tc_cull_row_encode(tc_cull_empty(h, cells, cv, pose));
}

// ---- (a), (b): host functions
#include <math.h>
#include <vector>

// distance from p to the segment a-b
static inline double tc_cull_seg_dist(double px, double py, double ax, double ay, double bx, double by) {
  const double ex = bx - ax, ey = by - ay, l2 = ex * ex + ey * ey;
  double t = l2 > 0 ? ((px - ax) * ex + (py - ay) * ey) / l2 : 0.0;
  t = t < 0 ? 0 : (t > 1 ? 1 : t);
  const double dx = px - (ax + t * ex), dy = py - (ay + t * ey);
  return sqrt(dx * dx + dy * dy);
}

// (a) nodes: [n_nodes][2]; edges: [n_edges][2] global node ids (all layers; no layer shares a node with another).
// out: TC_CULL_HEAD_BYTES of header + nx * ny cells, padded to a multiple of 4 bytes.
static inline void tc_cull_plan(const double* nodes, int n_nodes, const int* edges, int n_edges, double cell, double margin,
                                std::vector<unsigned char>& out) {
  TcCullHead h;
  memset(&h, 0, sizeof(h));
  h.margin = margin;
  auto finish = [&](const std::vector<unsigned char>& cells) {
    out.assign(TC_CULL_HEAD_BYTES + (cells.size() + 3) / 4 * 4, 0);
    memcpy(out.data(), &h, sizeof(h));
    if (!cells.empty()) memcpy(out.data() + TC_CULL_HEAD_BYTES, cells.data(), cells.size());
  };
  const std::vector<unsigned char> none;
  if (n_nodes < 1 || n_edges < 1 || !(cell > 0) || !(margin > 0)) return finish(none);
  std::vector<int> outd(n_nodes, 0), ind(n_nodes, 0);
  double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  for (int e = 0; e < n_edges; e++) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || b < 0 || a >= n_nodes || b >= n_nodes) return finish(none);
    outd[a]++;
    ind[b]++;
    for (int k = 0; k < 2; k++)
      for (int n : {a, b}) {
        const double v = nodes[2 * n + k];
        if (!(tc_fabs(v) <= 0.5 * TC_CULL_MAX_COORD)) return finish(none);  // (NaN too)
        lo[k] = v < lo[k] ? v : lo[k];
        hi[k] = v > hi[k] ? v : hi[k];
      }
    const double ex = nodes[2 * a] - nodes[2 * b], ey = nodes[2 * a + 1] - nodes[2 * b + 1];
    const double len = sqrt(ex * ex + ey * ey);
    h.lmax = len > h.lmax ? len : h.lmax;
  }
  // H3 and the special nodes of guard G
  std::vector<char> special(n_nodes, 0);
  for (int e = 0; e < n_edges; e++) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (ind[b] >= 2 && outd[a] >= 2) return finish(none);  // H3
    if (outd[a] >= 2) special[b] = 1;
    if (ind[b] >= 2) special[a] = 1;
  }
  for (int n = 0; n < n_nodes; n++)
    if (special[n]) {
      if (h.n_special == TC_CULL_MAX_SPECIAL) {
        h.n_special = 0;
        return finish(none);
      }
      h.special[h.n_special][0] = nodes[2 * n];
      h.special[h.n_special][1] = nodes[2 * n + 1];
      h.n_special++;
    }
  // the grid: bounding box + margin, the cell grown until the count fits
  const double wx = hi[0] - lo[0] + 2 * margin, wy = hi[1] - lo[1] + 2 * margin;
  while ((ceil(wx / cell) + 1) * (ceil(wy / cell) + 1) > (double)TC_CULL_MAX_CELLS) cell *= 1.25;
  const int nx = (int)ceil(wx / cell) + 1, ny = (int)ceil(wy / cell) + 1;
  h.x0 = lo[0] - margin;
  h.y0 = lo[1] - margin;
  h.cell = cell;
  h.inv = 1.0 / cell;
  // distance from each cell centre to the nearest segment, as far as it matters: beyond `cap` every cell is as good
  const double cap = margin + 2 * cell;
  std::vector<double> d((size_t)nx * ny, cap);
  for (int e = 0; e < n_edges; e++) {
    const double ax = nodes[2 * edges[2 * e]], ay = nodes[2 * edges[2 * e] + 1];
    const double bx = nodes[2 * edges[2 * e + 1]], by = nodes[2 * edges[2 * e + 1] + 1];
    const int ix0 = (int)floor(((ax < bx ? ax : bx) - cap - h.x0) * h.inv) - 1, ix1 = (int)floor(((ax > bx ? ax : bx) + cap - h.x0) * h.inv) + 1;
    const int iy0 = (int)floor(((ay < by ? ay : by) - cap - h.y0) * h.inv) - 1, iy1 = (int)floor(((ay > by ? ay : by) + cap - h.y0) * h.inv) + 1;
    for (int iy = iy0 < 0 ? 0 : iy0; iy <= iy1 && iy < ny; iy++)
      for (int ix = ix0 < 0 ? 0 : ix0; ix <= ix1 && ix < nx; ix++) {
        const double v = tc_cull_seg_dist(h.x0 + (ix + 0.5) * cell, h.y0 + (iy + 0.5) * cell, ax, ay, bx, by);
        double& s = d[(size_t)iy * nx + ix];
        s = v < s ? v : s;
      }
  }
  // any point of the cell is at most half a diagonal from the centre; 1e-9 * extent for the arithmetic above and the
  // predicate's own (coordinates below 1e4: errors below 1e-11)
  const double loss = 0.70710678118654757 * cell * (1 + 1e-9) + 1e-9 * (1.0 + wx + wy);
  std::vector<unsigned char> cells((size_t)nx * ny);
  for (size_t i = 0; i < cells.size(); i++) {
    const double q = floor((d[i] - loss) / cell);
    cells[i] = (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
  }
  h.nx = nx;
  h.ny = ny;
  finish(cells);
}

// convex polygon (x, y pairs) clipped to a * x + b * y + c >= 0
static inline void tc_cull_clip(std::vector<double>& poly, double a, double b, double c) {
  std::vector<double> o;
  const size_t n = poly.size() / 2;
  for (size_t i = 0; i < n; i++) {
    const double x0 = poly[2 * i], y0 = poly[2 * i + 1], x1 = poly[2 * ((i + 1) % n)], y1 = poly[2 * ((i + 1) % n) + 1];
    const double g0 = a * x0 + b * y0 + c, g1 = a * x1 + b * y1 + c;
    if (g0 >= 0) {
      o.push_back(x0);
      o.push_back(y0);
    }
    if ((g0 >= 0) != (g1 >= 0)) {
      const double t = g0 / (g0 - g1);
      o.push_back(x0 + t * (x1 - x0));
      o.push_back(y0 + t * (y1 - y0));
    }
  }
  poly.swap(o);
}

// smallest circle around the points (a handful: every pair and triple is tried); radius < 0: no points
static inline void tc_cull_enclose(const std::vector<double>& p, double* cx, double* cy, double* r) {
  const int n = (int)(p.size() / 2);
  *cx = *cy = 0;
  *r = -1;
  if (n == 0) return;
  double best = INFINITY;
  auto all_in = [&](double x, double y, double rr) {
    for (int i = 0; i < n; i++)
      if (hypot(p[2 * i] - x, p[2 * i + 1] - y) > rr * (1 + 1e-9) + 1e-12) return false;
    return true;
  };
  auto take = [&](double x, double y, double rr) {
    if (rr < best && all_in(x, y, rr)) {
      best = rr;
      *cx = x;
      *cy = y;
    }
  };
  take(p[0], p[1], 0.0);
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) {
      take(0.5 * (p[2 * i] + p[2 * j]), 0.5 * (p[2 * i + 1] + p[2 * j + 1]), 0.5 * hypot(p[2 * i] - p[2 * j], p[2 * i + 1] - p[2 * j + 1]));
      for (int k = j + 1; k < n; k++) {
        const double ax = p[2 * i], ay = p[2 * i + 1], bx = p[2 * j] - ax, by = p[2 * j + 1] - ay, qx = p[2 * k] - ax, qy = p[2 * k + 1] - ay;
        const double dd = 2 * (bx * qy - by * qx);
        if (dd == 0) continue;
        const double ux = (qy * (bx * bx + by * by) - by * (qx * qx + qy * qy)) / dd, uy = (bx * (qx * qx + qy * qy) - qx * (bx * bx + by * by)) / dd;
        take(ax + ux, ay + uy, hypot(ux, uy));
      }
    }
  if (best == INFINITY) {  // (degenerate input: the bounding circle around the first point)
    best = 0;
    for (int i = 0; i < n; i++) best = fmax(best, hypot(p[2 * i] - p[0], p[2 * i + 1] - p[1]));
    *cx = p[0];
    *cy = p[1];
  }
  *r = best;
}

// F in the car's frame: ground points p with camera coordinates P = E [p, 0, 1], -max_range <= P.z <= 0 and the pixel
// (K P) / (K P).z inside [0, W] x [0, H] (closed: a superset of camera.py:90's strict test).  Empty vector: not covered.
static inline std::vector<double> tc_cull_footprint(const double* E, const double* K, int W, int H, double max_range) {
  std::vector<double> poly;
  if (!(K[6] == 0 && K[7] == 0 && K[8] > 0) || !(max_range > 0) || !(max_range < 1e3)) return poly;
  double R[9] = {E[0], E[1], E[2], E[4], E[5], E[6], E[8], E[9], E[10]};
  for (int i = 0; i < 3; i++)  // R^T (c - t) is the inverse only of a rigid E
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += R[3 * i + k] * R[3 * j + k];
      if (!(fabs(s - (i == j ? 1.0 : 0.0)) <= 1e-9)) return poly;
    }
  for (int i = 0; i < 12; i++)
    if (!(fabs(E[i]) < 1e3)) return poly;
  // every constraint g(p) = a * px + b * py + c >= 0, from rows of E (P = A p + t) and K
  auto row = [&](const double* k3, double* g) {  // k3 . P as a function of p
    g[0] = k3[0] * E[0] + k3[1] * E[4] + k3[2] * E[8];
    g[1] = k3[0] * E[1] + k3[1] * E[5] + k3[2] * E[9];
    g[2] = k3[0] * E[3] + k3[1] * E[7] + k3[2] * E[11];
  };
  const double ez[3] = {0, 0, 1};
  double z[3], h0[3], h1[3], h2[3];
  row(ez, z);
  row(K, h0);
  row(K + 3, h1);
  row(K + 6, h2);
  const double B = 1e3 * (max_range + 1.0);
  poly = {-B, -B, B, -B, B, B, -B, B};
  tc_cull_clip(poly, -z[0], -z[1], -z[2]);                                   // z <= 0
  tc_cull_clip(poly, z[0], z[1], z[2] + max_range);                          // z >= -max_range
  tc_cull_clip(poly, -h0[0], -h0[1], -h0[2]);                                // u >= 0 (h2 < 0: h0 <= 0)
  tc_cull_clip(poly, h0[0] - W * h2[0], h0[1] - W * h2[1], h0[2] - W * h2[2]);  // u <= W: h0 >= W h2
  tc_cull_clip(poly, -h1[0], -h1[1], -h1[2]);
  tc_cull_clip(poly, h1[0] - H * h2[0], h1[1] - H * h2[1], h1[2] - H * h2[2]);
  for (size_t i = 0; i < poly.size(); i++)
    if (!(fabs(poly[i]) < 0.5 * B)) {  // unbounded within anything a table could serve
      poly.clear();
      break;
    }
  return poly;
}

// (b) the cover of F for this camera and this table (H1 reads the table's longest edge)
static inline void tc_cull_cover(const double* E, const double* K, int W, int H, double max_range, const TcCullHead& h, TcCullCover* cv) {
  memset(cv, 0, sizeof(*cv));
  cv->max_range = max_range;
  std::vector<double> F = tc_cull_footprint(E, K, W, H, max_range);
  if (F.size() < 6 || h.nx <= 0) return;
  if (!(h.lmax <= max_range - 1e-3)) return;  // H1
  // H2: the camera centre C = -R^T t, its height over the ground |C.z|, against the frame cone at depth 1e-7
  const double cz = -(E[2] * E[3] + E[6] * E[7] + E[10] * E[11]);
  const double ax = fmax(fabs(K[2]), fabs(W - K[2])) / fabs(K[0]), ay = fmax(fabs(K[5]), fabs(H - K[5])) / fabs(K[4]);
  if (!(fabs(cz) > 1e-6 * sqrt(1 + ax * ax + ay * ay))) return;
  const double zr[3] = {E[8], E[9], E[11]};
  double zlo = INFINITY, zhi = -INFINITY;
  for (size_t i = 0; i < F.size() / 2; i++) {
    const double zz = zr[0] * F[2 * i] + zr[1] * F[2 * i + 1] + zr[2];
    zlo = fmin(zlo, zz);
    zhi = fmax(zhi, zz);
  }
  const double slack = TC_CULL_SLACK * fmax(1.0, max_range);
  for (int i = 0; i < TC_CULL_NC; i++) {
    // slab i of the depth range; equal AREA would suit a trapezoid better than equal depth: the far slabs are the wide
    // ones, so the cuts sit at the square roots
    const double f0 = sqrt((double)i / TC_CULL_NC), f1 = sqrt((double)(i + 1) / TC_CULL_NC);
    const double z0 = zhi + (zlo - zhi) * f1, z1 = zhi + (zlo - zhi) * f0;  // z0 <= z <= z1 (depths are negative)
    std::vector<double> s = F;
    if (i + 1 < TC_CULL_NC) tc_cull_clip(s, zr[0], zr[1], zr[2] - z0);
    if (i > 0) tc_cull_clip(s, -zr[0], -zr[1], -(zr[2] - z1));
    double cx, cy, r;
    tc_cull_enclose(s, &cx, &cy, &r);
    if (r < 0) {  // an empty slab (a degenerate F): a point of F, radius 0
      cx = F[0];
      cy = F[1];
      r = 0;
    }
    cv->car[i][0] = cx;
    cv->car[i][1] = cy;
    for (int k = 0; k < 3; k++) cv->c[i][k] = E[4 * k] * cx + E[4 * k + 1] * cy + E[4 * k + 3];
    cv->r[i] = r * (1 + 1e-9) + slack;
  }
  cv->on = 1;
}
#endif  // TC_CULL_H
