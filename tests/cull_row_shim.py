"""The cull verdict of a pose row (tc_cull_row_encode / tc_cull_row_decode / tc_cull_row_verdict of
tinycarlo_amd/csrc/tc_cull.h) built by the host compiler: tests/cull_shim.py's source with the row helpers behind it, as a
shared library for ctypes (build_shim) and as a stand-alone program with its own main() for sanitizer builds
(build_program).  Test infrastructure of tests/test_cull_row_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import cull_shim

SRC = cull_shim.SRC + r"""
// ---- the verdict word of a pose row
static void pose_at(const double* E, double x, double y, double cth, double sth, double* pose) {
  double R[16] = {cth, -sth, 0, 0, sth, cth, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double Tm[16] = {1, 0, 0, -x, 0, 1, 0, -y, 0, 0, 1, 0, 0, 0, 0, 1};
  double car3d[16];
  matmul(R, Tm, car3d, 4, 4, 4);
  matmul(E, car3d, pose, 3, 4, 4);
}
extern "C" unsigned long long row_encode(int empty) { return tc_cull_row_encode(empty); }
extern "C" int row_decode(unsigned long long w) { return tc_cull_row_decode(w); }
extern "C" int row_entry() { return TC_CULL_ROW_ENTRY; }
// poses: [n][4] = x, y, cos(-theta), sin(-theta); out: the word a pose-row writer stores for each
extern "C" void row_verdict_batch(void* p, const double* E, int n, const double* poses, unsigned long long* out) {
  const Cull* c = (const Cull*)p;
  for (int i = 0; i < n; i++) {
    double pose[12];
    pose_at(E, poses[4 * i], poses[4 * i + 1], poses[4 * i + 2], poses[4 * i + 3], pose);
    out[i] = tc_cull_row_verdict(c->h, c->tab.data() + TC_CULL_HEAD_BYTES, c->cv, pose);
  }
}

#ifdef ROW_MAIN
// stand-alone form: the input file of cull_shim's program.  Every pose's word is one of the two verdicts, never "not written
// yet" (all ones), decodes to tc_cull_empty of that pose, and no pose with a segment decodes as culled.  Also the codec on
// words no writer stores: only the word "culled" skips a frame.  Exit status 1 on any miss; prints the counts.
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
  std::vector<double> p4(4 * (size_t)n_poses);
  for (int i = 0; i < n_poses; i++)
    for (int k = 0; k < 4; k++) p4[4 * i + k] = ps[5 * i + k];
  std::vector<unsigned long long> w(n_poses);
  row_verdict_batch(c, Es, n_poses, p4.data(), w.data());
  int culled = 0, wrong = 0;
  for (int i = 0; i < n_poses; i++) {
    const int e = empty_at(c, Es, ps[5 * i], ps[5 * i + 1], ps[5 * i + 2], ps[5 * i + 3]);
    wrong += w[i] == ~0ull || (w[i] != TC_CULL_ROW_DRAW && w[i] != TC_CULL_ROW_CULLED);
    wrong += tc_cull_row_decode(w[i]) != e;
    wrong += tc_cull_row_decode(w[i]) && ps[5 * i + 4] != 0;
    culled += tc_cull_row_decode(w[i]);
  }
  const unsigned long long odd[6] = {~0ull, 2ull, 1ull << 32, 0x8000000000000001ull, 0x3ff0000000000000ull, 0x7ff8000000000000ull};
  for (int i = 0; i < 6; i++) wrong += tc_cull_row_decode(odd[i]) != 0;
  wrong += tc_cull_row_decode(tc_cull_row_encode(1)) != 1 || tc_cull_row_decode(tc_cull_row_encode(0)) != 0;
  cull_free(c);
  printf("culled %d of %d, wrong %d\n", culled, n_poses, wrong);
  return wrong ? 1 : 0;
}
#endif
"""


def _write_src(d):
    src = os.path.join(str(d), "cull_row_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d):
    """-> ctypes library: cull_shim's functions (usable through cull_shim.Cull) and the row helpers"""
    src = _write_src(d)
    lib = os.path.join(str(d), "libtc_cull_row.so")
    subprocess.check_call(["c++"] + cull_shim.FLAGS + ["-shared", "-fPIC", "-o", lib, src])
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
    L.row_encode.restype = C.c_uint64
    L.row_encode.argtypes = [C.c_int]
    L.row_decode.argtypes = [C.c_uint64]
    L.row_verdict_batch.argtypes = [C.c_void_p, dp, C.c_int, dp, C.POINTER(C.c_uint64)]
    return L


def build_program(d, sanitize=True):
    """-> path of the stand-alone program (its own main), with -fsanitize=address,undefined unless told otherwise"""
    src = _write_src(d)
    exe = os.path.join(str(d), "cull_row_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["c++"] + cull_shim.FLAGS + san + ["-DROW_MAIN", "-o", exe, src])
    return exe


def verdicts(L, cull, x, y, theta):
    """the words a pose-row writer stores for poses (arrays) of cull_shim.Cull `cull` (built on this library) -> uint64 array"""
    p = np.ascontiguousarray(np.stack([x, y, np.cos(-theta), np.sin(-theta)], axis=1), dtype=np.float64)
    out = np.zeros(len(p), dtype=np.uint64)
    L.row_verdict_batch(cull.h, cull.E.ctypes.data_as(C.POINTER(C.c_double)), len(p), p.ctypes.data_as(C.POINTER(C.c_double)),
                        out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return out
