"""tinycarlo_amd/csrc/tc_cull.h built alone by the host compiler: a shared library for ctypes (build_shim) and, from the
same source, a stand-alone program with its own main() for sanitizer builds (build_program).  Test infrastructure, also
used by tools/frame_cull_study.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "tc_cull.h"
#include <stdio.h>
#include <stdlib.h>

struct Cull {
  std::vector<unsigned char> tab;
  TcCullHead h;
  TcCullCover cv;
  std::vector<double> F;
};
static void matmul(const double* A, const double* B, double* Cm, int n, int k, int p) {  // numpy's dgemm association
  for (int i = 0; i < n; i++)
    for (int j = 0; j < p; j++) {
      double acc = 0.0;
      for (int t = 0; t < k; t++) acc = __builtin_fma(A[i * k + t], B[t * p + j], acc);
      Cm[i * p + j] = acc;
    }
}
extern "C" void* cull_create(const double* nodes, int n_nodes, const int* edges, int n_edges, double cell, double margin) {
  Cull* c = new Cull;
  tc_cull_plan(nodes, n_nodes, edges, n_edges, cell, margin, c->tab);
  memcpy(&c->h, c->tab.data(), sizeof(c->h));
  memset(&c->cv, 0, sizeof(c->cv));
  return c;
}
extern "C" void cull_free(void* p) { delete (Cull*)p; }
// out: x0, y0, inv, cell, margin, lmax, nx, ny, n_special
extern "C" void cull_head(void* p, double* out) {
  const TcCullHead& h = ((Cull*)p)->h;
  const double v[9] = {h.x0, h.y0, h.inv, h.cell, h.margin, h.lmax, (double)h.nx, (double)h.ny, (double)h.n_special};
  memcpy(out, v, sizeof(v));
}
extern "C" const unsigned char* cull_cells(void* p) { return ((Cull*)p)->tab.data() + TC_CULL_HEAD_BYTES; }
extern "C" int cull_nc() { return TC_CULL_NC; }
// circles: [NC][3] = centre in the car's frame, radius; poly: up to 16 vertices of F; returns on | n_vertices << 8
extern "C" int cull_set_camera(void* p, const double* E, const double* K, int W, int H, double max_range, double* circles,
                               double* poly, double* Estore) {
  Cull* c = (Cull*)p;
  tc_cull_cover(E, K, W, H, max_range, c->h, &c->cv);
  c->F = tc_cull_footprint(E, K, W, H, max_range);
  for (int i = 0; i < TC_CULL_NC; i++) {
    circles[3 * i] = c->cv.car[i][0];
    circles[3 * i + 1] = c->cv.car[i][1];
    circles[3 * i + 2] = c->cv.r[i];
  }
  const int nv = (int)(c->F.size() / 2) < 16 ? (int)(c->F.size() / 2) : 16;
  for (int i = 0; i < 2 * nv; i++) poly[i] = c->F[i];
  memcpy(Estore, E, 12 * sizeof(double));
  return c->cv.on | nv << 8;
}
static int empty_at(const Cull* c, const double* E, double x, double y, double cth, double sth) {
  double R[16] = {cth, -sth, 0, 0, sth, cth, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double Tm[16] = {1, 0, 0, -x, 0, 1, 0, -y, 0, 0, 1, 0, 0, 0, 0, 1};
  double car3d[16], pose[12];
  matmul(R, Tm, car3d, 4, 4, 4);
  matmul(E, car3d, pose, 3, 4, 4);
  return tc_cull_empty(c->h, c->tab.data() + TC_CULL_HEAD_BYTES, c->cv, pose);
}
// poses: [n][4] = x, y, cos(-theta), sin(-theta) (camera.py:61 / car.py's 3d transformation)
extern "C" void cull_empty_batch(void* p, const double* E, int n, const double* poses, unsigned char* out) {
  for (int i = 0; i < n; i++) out[i] = (unsigned char)empty_at((Cull*)p, E, poses[4 * i], poses[4 * i + 1], poses[4 * i + 2], poses[4 * i + 3]);
}

#ifdef CULL_MAIN
// stand-alone form: argv[1] is a file of doubles -- n_nodes, n_edges, cell, margin, E[12], K[9], W, H, max_range, n_poses,
// nodes[2 n_nodes], edges[2 n_edges], then per pose x, y, c, s, "the oracle's draw list is not empty".  Exit status 1 if a
// pose with a segment is called empty; prints the count of culled poses.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> d;
  double buf[1024];
  size_t got;
  while ((got = fread(buf, sizeof(double), 1024, f)) > 0) d.insert(d.end(), buf, buf + got);
  fclose(f);
  if (d.size() < 29) return 2;
  const int n_nodes = (int)d[0], n_edges = (int)d[1], W = (int)d[25], H = (int)d[26], n_poses = (int)d[28];
  if (d.size() != (size_t)29 + 2 * n_nodes + 2 * n_edges + 5 * n_poses) return 2;
  const double* nodes = d.data() + 29;
  std::vector<int> edges(2 * n_edges);
  for (int i = 0; i < 2 * n_edges; i++) edges[i] = (int)nodes[2 * n_nodes + i];
  Cull* c = (Cull*)cull_create(nodes, n_nodes, edges.data(), n_edges, d[2], d[3]);
  double circles[3 * TC_CULL_NC], poly[32], Es[12];
  cull_set_camera(c, d.data() + 4, d.data() + 16, W, H, d[27], circles, poly, Es);
  const double* ps = nodes + 2 * n_nodes + 2 * n_edges;
  int culled = 0, wrong = 0;
  for (int i = 0; i < n_poses; i++) {
    const int e = empty_at(c, Es, ps[5 * i], ps[5 * i + 1], ps[5 * i + 2], ps[5 * i + 3]);
    culled += e;
    wrong += e && ps[5 * i + 4] != 0;
  }
  cull_free(c);
  printf("culled %d of %d, wrong %d\n", culled, n_poses, wrong);
  return wrong ? 1 : 0;
}
#endif
"""

FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc")]


def _write_src(d):
    src = os.path.join(str(d), "cull_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d, nc=None):
    """-> ctypes library of the shim built in directory d (nc: TC_CULL_NC override, else the header's own)"""
    src = _write_src(d)
    lib = os.path.join(str(d), "libtc_cull%s.so" % ("" if nc is None else "_nc%d" % nc))
    subprocess.check_call(["c++"] + FLAGS + ([] if nc is None else ["-DTC_CULL_NC=%d" % nc]) + ["-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.cull_create.restype = C.c_void_p
    L.cull_create.argtypes = [dp, C.c_int, ip, C.c_int, C.c_double, C.c_double]
    L.cull_free.argtypes = [C.c_void_p]
    L.cull_head.argtypes = [C.c_void_p, dp]
    L.cull_cells.restype = C.POINTER(C.c_uint8)
    L.cull_cells.argtypes = [C.c_void_p]
    L.cull_set_camera.argtypes = [C.c_void_p, dp, dp, C.c_int, C.c_int, C.c_double, dp, dp, dp]
    L.cull_empty_batch.argtypes = [C.c_void_p, dp, C.c_int, dp, C.POINTER(C.c_uint8)]
    return L


def build_program(d, sanitize=True):
    """-> path of the stand-alone program (its own main), with -fsanitize=address,undefined unless told otherwise"""
    src = _write_src(d)
    exe = os.path.join(str(d), "cull_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["c++"] + FLAGS + san + ["-DCULL_MAIN", "-o", exe, src])
    return exe


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def graph_of(m):
    """(nodes [n][2] f64, edges [e][2] i32 with global node ids) of a tinycarlo_amd.map.Map's lane-line layers"""
    f = m.flat()
    node_off = np.concatenate([[0], np.cumsum(f["node_count"])]).astype(np.int64)
    nodes = np.ascontiguousarray(f["nodes"], dtype=np.float64).reshape(-1, 2)
    edges = np.ascontiguousarray(np.asarray(f["edges"]).reshape(-1, 2) + np.repeat(node_off[:-1], f["edge_count"])[:, None], dtype=np.int32)
    return nodes, edges


class Cull:
    """The planner's table for one map, the cover of one camera, and the predicate."""

    CELL, MARGIN = 0.02, 1.0  # what tc_env_create passes

    def __init__(self, L, m, camera=None, cell=CELL, margin=MARGIN):
        self.L = L
        self.nodes, self.edges = graph_of(m)
        self.cell_arg, self.margin_arg = cell, margin
        self.h = L.cull_create(_dp(self.nodes), len(self.nodes), self.edges.ctypes.data_as(C.POINTER(C.c_int32)), len(self.edges),
                               cell, margin)
        hd = np.zeros(9)
        L.cull_head(self.h, _dp(hd))
        self.x0, self.y0, self.inv, self.cell, self.margin, self.lmax = hd[:6]
        self.nx, self.ny, self.n_special = int(hd[6]), int(hd[7]), int(hd[8])
        self.nc = L.cull_nc()
        self.on = 0
        if camera is not None:
            self.set_camera(camera)

    def __del__(self):
        try:
            self.L.cull_free(self.h)
        except Exception:
            pass

    def cells(self):
        return np.ctypeslib.as_array(self.L.cull_cells(self.h), shape=(self.ny, self.nx)).copy() if self.nx else np.zeros((0, 0), np.uint8)

    def set_camera(self, cam):
        self.set_camera_raw(np.asarray(cam.E, dtype=np.float64), np.asarray(cam.K, dtype=np.float64), int(cam.resolution[1]),
                            int(cam.resolution[0]), float(cam.max_range))

    def set_camera_raw(self, E, K, W, H, max_range):
        self.E = np.ascontiguousarray(E, dtype=np.float64).reshape(12)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        circles, poly, es = np.zeros(3 * self.nc), np.zeros(32), np.zeros(12)
        r = self.L.cull_set_camera(self.h, _dp(self.E), _dp(K), W, H, max_range, _dp(circles), _dp(poly), _dp(es))
        self.on = r & 1
        self.circles = circles.reshape(-1, 3)
        self.poly = poly[:2 * (r >> 8)].reshape(-1, 2)

    def empty(self, x, y, theta):
        """the predicate at poses (arrays or scalars) -> bool array"""
        x, y, theta = np.broadcast_arrays(np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64)),
                                          np.atleast_1d(np.asarray(theta, dtype=np.float64)))
        p = np.ascontiguousarray(np.stack([x, y, np.cos(-theta), np.sin(-theta)], axis=1))
        out = np.zeros(len(p), dtype=np.uint8)
        self.L.cull_empty_batch(self.h, _dp(self.E), len(p), _dp(p), out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out.astype(bool)

    def program_input(self, K, W, H, max_range, poses, nonempty):
        """the stand-alone program's input file as an array of doubles; poses [n][3] = x, y, theta"""
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        head = np.concatenate([[len(self.nodes), len(self.edges), self.cell_arg, self.margin_arg], self.E,
                               np.asarray(K, dtype=np.float64).reshape(9), [W, H, max_range, len(poses)]])
        ps = np.stack([poses[:, 0], poses[:, 1], np.cos(-poses[:, 2]), np.sin(-poses[:, 2]),
                       np.asarray(nonempty, dtype=np.float64)], axis=1)
        return np.concatenate([head, self.nodes.reshape(-1), self.edges.reshape(-1).astype(np.float64), ps.reshape(-1)])


# ---- pose sets shared by tests/test_frame_cull_cpu.py and tests/test_gpu_frame_cull.py: rows of (x, y, theta)
def outside_poses(nodes, dist=2.5, n=12):
    """parked more than 2 m outside the lane lines' bounding box, facing outward"""
    lo, hi = nodes.min(0), nodes.max(0)
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    out = []
    for k in range(n):
        a = 2 * np.pi * (k + 0.25) / n
        d = np.array([np.cos(a), np.sin(a)])
        s = min((half[0] + dist) / max(abs(d[0]), 1e-12), (half[1] + dist) / max(abs(d[1]), 1e-12))  # onto the box grown by dist
        p = c + d * s * 1.05
        out.append((p[0], p[1], a))
    return np.array(out)


def road_poses(m, n=12):
    """parked on lane-path nodes, facing along an out-edge"""
    f = m.flat()
    lp, le = np.asarray(f["lp_nodes"], dtype=np.float64).reshape(-1, 2), np.asarray(f["lp_edges"]).reshape(-1, 2)
    out = []
    for e in le[:: max(1, len(le) // n)][:n]:
        d = lp[e[1]] - lp[e[0]]
        out.append((lp[e[0]][0], lp[e[0]][1], np.arctan2(d[1], d[0])))
    return np.array(out)


def boundary_poses(cull, n_nodes=8, seed=5, offsets=None):
    """Around sampled lane-line nodes, on the ring where the predicate flips: the car backs away from the node along its
    heading (facing the node), along the opposite heading (facing away) and sideways (tangential) until the predicate
    says "empty" (bisection to 1e-12), then the poses at that distance, +- one cell and +- 1e-9."""
    rng = np.random.default_rng(seed)
    offsets = (0.0, cull.cell, -cull.cell, 1e-9, -1e-9) if offsets is None else offsets
    out = []
    for i in rng.choice(len(cull.nodes), min(n_nodes, len(cull.nodes)), replace=False):
        p = cull.nodes[i]
        for kind in range(3):
            a = rng.uniform(-np.pi, np.pi)  # direction from the node to the car
            th = (a + np.pi, a, a + 0.5 * np.pi)[kind]  # facing the node, away from it, tangential
            d = np.array([np.cos(a), np.sin(a)])
            lo, hi = 0.0, 4.0
            if not cull.empty(*(p + hi * d), th)[0] or cull.empty(*(p + lo * d), th)[0]:
                continue  # (the cull is off, or already empty on the node: no ring)
            while hi - lo > 1e-12:
                mid = 0.5 * (lo + hi)
                if cull.empty(*(p + mid * d), th)[0]:
                    hi = mid
                else:
                    lo = mid
            for o in offsets:
                q = p + (hi + o) * d
                out.append((q[0], q[1], th))
    return np.array(out).reshape(-1, 3)


def grid_poses(cull):
    """on cell corners (+- 1 ulp), on the grid's outer border, outside it and 60 m away"""
    if not cull.nx:
        return np.zeros((0, 3))
    out = []
    x1, y1 = cull.x0 + cull.nx * cull.cell, cull.y0 + cull.ny * cull.cell
    for (ix, iy) in ((cull.nx // 2, cull.ny // 2), (cull.nx // 3, cull.ny // 2), (1, 1), (cull.nx - 1, cull.ny - 1)):
        x, y = cull.x0 + ix * cull.cell, cull.y0 + iy * cull.cell
        for xx in (x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)):
            for yy in (y, np.nextafter(y, -np.inf), np.nextafter(y, np.inf)):
                out.append((xx, yy, 0.3))
    for th in (0.0, 1.0, 2.5, -2.0):
        out += [(cull.x0, cull.y0, th), (x1, y1, th), (cull.x0, 0.5 * (cull.y0 + y1), th), (0.5 * (cull.x0 + x1), y1, th),
                (np.nextafter(cull.x0, -np.inf), cull.y0, th), (x1 + 0.3, y1 + 0.3, th), (cull.x0 - 0.5, cull.y0 - 0.5, th),
                (cull.x0 - 60.0, cull.y0, th), (x1 + 60.0, y1 + 60.0, th)]
    return np.array(out)
