"""plan_frame_lds of tinycarlo_amd/csrc/tc_plan.h and the one-word list entries of tc_pack.h, built alone by the host
compiler: as a ctypes library for tests/test_frame_lds_cpu.py, and as a stand-alone program (its own main) that walks
the packing exhaustively and a grid of plans under -fsanitize=address,undefined.  Test infrastructure only.

`shared_frame_lds` restates, from plan_cam_lds (through the shim of tests/big_maps.py) and the R_* macros of k_common.h,
what layout_lds and grow_lds_for_draw_lists give a frame workgroup -- the bytes the frame plan may never exceed."""
import ctypes as C
import os
import subprocess

import numpy as np

import big_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 64
LIVE_BYTES = 416     # TC_LIVE_BYTES
LDS_STEP = 1280      # a CU grants LDS in steps of this many bytes
CU_LDS = 160 * 1024
ENTRY = 20           # bytes of a draw-list entry
BAND_BYTES = 16384   # default of TC_BAND_BYTES
PACK_IDS = 1024      # TC_PACK_IDS
FIELDS = ("off_p", "off_flg", "off_list", "off_cnt", "cam_total", "list_bytes", "counters", "r_off_tab", "r_off_bits", "r_total",
          "head_off", "head_cap", "total")

SRC = r"""
#include "tc_plan.h"
#include "tc_pack.h"
#include <cstdio>
#include <vector>
// in: cap_n, cap_e, total_nodes, windowed, rb, sh, band_bytes, live, seg_lds, seg_lds_limit, limit, reserve; out: 13 ints
extern "C" void frame_lds(const int* in, int* out) {
  const FrameLds f = plan_frame_lds(in[0], in[1], in[2], in[3] != 0, in[4], in[5], in[6], in[7], in[8] != 0, in[9], in[10], in[11]);
  const int v[13] = {f.off_p, f.off_flg, f.off_list, f.off_cnt, f.cam_total, f.list_bytes, f.counters ? 1 : 0, f.r_off_tab,
                     f.r_off_bits, f.r_total, f.head_off, f.head_cap, f.total};
  for (int i = 0; i < 13; i++) out[i] = v[i];
}
extern "C" int pack(int e, int t, int o) { return tc_pack(e, t, o); }
extern "C" int pack_edge(int w) { return tc_pack_edge(w); }
extern "C" int pack_target(int w) { return tc_pack_target(w); }
extern "C" int pack_other(int w) { return tc_pack_other(w); }
extern "C" int pack_list_bytes(int cap_n, int cap_e) { return tc_pack_list_bytes(cap_n, cap_e); }
extern "C" int pack_ids() { return TC_PACK_IDS; }
extern "C" int pack_fits(int k) { return TC_PACK_FITS(k) ? 1 : 0; }
// every (edge, target, other) below n: round trip, non-negative, and word order = edge order for entries of one target
extern "C" long long pack_walk(int n) {
  long long bad = 0;
  for (int e = 0; e < n; e++)
    for (int t = 0; t < n; t++)
      for (int o = 0; o < n; o++) {
        const int w = tc_pack(e, t, o);
        bad += !(w >= 0 && tc_pack_edge(w) == e && tc_pack_target(w) == t && tc_pack_other(w) == o);
      }
  for (int e = 0; e + 1 < n; e++)  // the extremes of `other` on both sides: the edge id alone decides
    bad += !(tc_pack(e, 0, n - 1) < tc_pack(e + 1, 0, 0)) + !(tc_pack(e, n - 1, n - 1) < tc_pack(e + 1, n - 1, 0));
  return bad;
}
#ifdef FRAME_LDS_MAIN
int main() {
  long long bad = pack_walk(13 * 64);
  // a list of entries written and read back through a buffer of exactly tc_pack_list_bytes
  for (int cap_n = 1; cap_n <= 832; cap_n += 37)
    for (int cap_e = 0; cap_e <= 832; cap_e += 41) {
      std::vector<unsigned char> buf((size_t)tc_pack_list_bytes(cap_n, cap_e));
      int* list = (int*)buf.data();
      unsigned short* cand = (unsigned short*)buf.data();
      for (int j = 0; j < cap_e; j++) list[j] = tc_pack(j, (j * 7) % cap_n, (j * 11) % cap_n);
      for (int j = 0; j < cap_e; j++) bad += tc_pack_edge(list[j]) != j;
      for (int j = 0; j < cap_n; j++) cand[j] = (unsigned short)j;
      for (int j = 0; j < cap_n; j++) bad += cand[j] != j;
      for (int w = 0; w < 2; w++)
        for (int sh = 1; sh <= 2; sh++)
          for (int rb = 16; rb <= 32; rb += 16) {
            const FrameLds f = plan_frame_lds(cap_n, cap_e, cap_n + 5, w != 0, rb, sh, 2560, 416, true, 1 << 30, 0, 0);
            bad += f.total < f.head_off + 20 * f.head_cap || f.head_off < f.cam_total || f.head_off < f.r_total || f.head_cap < 8;
          }
    }
  printf("bad %lld\n", bad);
  return bad != 0;
}
#endif
"""
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc")]


def _write_src(d):
    src = os.path.join(str(d), "frame_lds_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d):
    lib = os.path.join(str(d), "libtc_frame_lds.so")
    subprocess.check_call(["c++"] + FLAGS + ["-shared", "-fPIC", "-o", lib, _write_src(d)])
    L = C.CDLL(lib)
    L.pack_walk.restype = C.c_longlong
    return L


def build_program(d, sanitize=True):
    """-> path of the stand-alone program (its own main), with -fsanitize=address,undefined unless told otherwise"""
    exe = os.path.join(str(d), "frame_lds_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["c++"] + FLAGS + san + ["-DFRAME_LDS_MAIN", "-o", exe, _write_src(d)])
    return exe


def frame_lds(L, cap_n, cap_e, total_nodes, windowed, rb, sh, band_bytes, live=LIVE_BYTES, seg_lds=True, seg_lds_limit=1 << 30,
              limit=0, reserve=0):
    a = np.array([cap_n, cap_e, total_nodes, int(windowed), rb, sh, band_bytes, live, int(seg_lds), seg_lds_limit, limit, reserve],
                 dtype=np.int32)
    out = np.zeros(len(FIELDS), dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    L.frame_lds(a.ctypes.data_as(ip), out.ctypes.data_as(ip))
    return dict(zip(FIELDS, (int(v) for v in out)))


def align_up(v, a):
    return (v + a - 1) // a * a


def r_tab_bytes(rb):
    """R_TAB_BYTES_OF(RB) of k_common.h: the raster tables at their full size"""
    return (rb * 4 * 5 + rb * 4 + 5 * rb + 8 * rb) * 4 + 2 * 4 * rb * 8


def frame_rb(kframe):
    """segments per raster batch of the frame kernel variant (RB_OF_K; 516 = K 5 with batches of 16)"""
    return 16 if kframe == 516 or kframe >= 8 else 32


def shared_frame_lds(plan, H, W):
    """What layout_lds and grow_lds_for_draw_lists give a frame workgroup of a handle with this plan (big_maps.expected_plan)
    at resolution H x W with the default switches -> (bytes, head entries, band_rows)"""
    C_ = plan["n_layers"]
    cam = plan["lds"]["total"]
    rb_k = 32 if plan["kvar"] in (5, 13) else 16
    off_bits_k = align_up(r_tab_bytes(rb_k), 16)
    row_bytes = C_ * ((W + 31) // 32) * 4
    band_rows = min(max(BAND_BYTES // row_bytes, 1), H)
    if -(-H // band_rows) > 1:
        fit = (cam - off_bits_k) // row_bytes
        if 8 <= fit < band_rows:
            band_rows = fit
    r_lds_k = off_bits_k + align_up(band_rows * row_bytes, 16)
    off_live = align_up(max(cam, r_lds_k), 16)
    total = off_live + LIVE_BYTES
    w = max(CU_LDS // total, 1)
    grown = max(min(CU_LDS // w // LDS_STEP * LDS_STEP, total + 4096), total)
    return grown, (grown - off_live) // ENTRY, band_rows


def handle_frame_lds(L, plan, H, W, thickness, **kw):
    """the frame plan of a handle with this map plan and camera, as plan_frame (tinycarlo_hip.hip) makes it: the planner's
    for the K = 5 kernel with batches of 32 (`lean`), the layout shared with the other kernels for every other frame kernel
    (default switches only)"""
    limit, head, band_rows = shared_frame_lds(plan, H, W)
    kf = 5 if plan["kframe"] == 516 else plan["kframe"]
    n0, e0 = plan["n0"], plan["e0"]
    windowed = any(n0[g + 1] - n0[g] > kf * NT or e0[g + 1] - e0[g] > kf * NT for g in range(plan["n_groups"]))
    sh = 1 if thickness == 2 and W >= 8 and H >= 8 and kw.pop("short_edges_skip", True) else 2
    band_bytes = band_rows * plan["n_layers"] * ((W + 31) // 32) * 4
    if not (kf == 5 and frame_rb(plan["kframe"]) == 32):
        L0 = plan["lds"]
        # the bit-planes where this frame kernel puts them, behind full-size tables of its own batch size; the head where
        # layout_lds put the parked state (off_live), behind the tables of the handle's fused kernels (never smaller)
        rb_k = 32 if plan["kvar"] in (5, 13) else 16
        bits = align_up(r_tab_bytes(frame_rb(plan["kframe"])), 16)
        f = dict(off_p=L0["off_p"], off_flg=L0["off_flg"], off_list=L0["off_list"], off_cnt=L0["off_cnt"], cam_total=L0["total"],
                 list_bytes=L0["off_cnt"] - L0["off_list"], counters=1, r_off_tab=0, r_off_bits=bits, r_total=bits + align_up(band_bytes, 16),
                 head_cap=head, total=limit)
        f["head_off"] = align_up(max(L0["total"], align_up(r_tab_bytes(rb_k), 16) + align_up(band_bytes, 16)), 16)
        f.update(windowed=windowed, sh=2, limit=limit, band_bytes=band_bytes, lean=False)
        return f
    f = frame_lds(L, plan["cap_n"], plan["cap_e"], plan["total_nodes"], windowed, frame_rb(plan["kframe"]), sh, band_bytes, limit=limit, **kw)
    f.update(windowed=windowed, sh=sh, limit=limit, band_bytes=band_bytes, lean=True)
    return f
