"""plan_envg_lds of tinycarlo_amd/csrc/tc_plan.h (the LDS of a workgroup of the grouped simulate launch), built alone by the
host compiler: as a ctypes library for tests/test_envg_lds_cpu.py, and as a stand-alone program (its own main) that walks a
grid of plans under -fsanitize=address,undefined.  Test infrastructure only.

`launch_request` restates in Python what the launch asks for (launch_envg of tinycarlo_hip.hip and the kernel's reading of
it in k_envg.h): the tests compare the planner with it, not with itself."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_STEP = 1280      # a CU grants LDS in steps of this many bytes
CU_LDS = 160 * 1024
EDGE_BYTES = 48      # end points (4 doubles) + two orientations of a lane-line edge
LP_NODE_BYTES = 96   # sizeof(LpNode), tc_device.h
MAX_TERMS = 8        # TC_MAX_TERMS
ENVS_PER_WG = 32     # TC_ENVG_NT / TC_EL
MAP_CAP, FAT_CAP = 40 * 1024, 56 * 1024  # above these a table stays in global memory
FIELDS = ("map_lds", "fat_lds", "fat_off", "grp_off", "grp_stride", "cnt_off", "dynamic", "static_bytes", "granted", "workgroups",
          "frames_beside")

SRC = r"""
#include "tc_plan.h"
#include <cstdio>
#include <cstring>
#include <vector>
// in: total_edges, lpN, lp_node_bytes, C, max_terms, N, groups, info_every, map_switch, static_bytes, frame_lds, pad
extern "C" void envg_lds(const int* in, int* out) {
  const EnvgLds p = plan_envg_lds(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7] != 0, in[8] != 0, in[9], in[10], in[11]);
  const int v[11] = {p.map_lds, p.fat_lds, p.fat_off, p.grp_off, p.grp_stride, p.cnt_off, p.dynamic, p.static_bytes, p.granted,
                     p.workgroups, p.frames_beside};
  for (int i = 0; i < 11; i++) out[i] = v[i];
}
extern "C" int envg_static(int groups, int ep, int ctrl) { return envg_static_lds(groups, ep != 0, ctrl != 0); }
#ifdef ENVG_LDS_MAIN
// a grid of plans, each laid out in a buffer of exactly `dynamic` bytes and written as the kernel writes it: the edge
// records, the fat node records, every env's distances and counters -- every region inside the buffer, none overlapping
int main() {
  long long bad = 0;
  for (int edges = 0; edges <= 900; edges += 75)
    for (int lpN = 1; lpN <= 640; lpN += 71)
      for (int C = 1; C <= 16; C += 5)
        for (int mt = 4; mt <= 8; mt += 4)
          for (int flags = 0; flags < 4; flags++)
            for (int groups = 32; groups <= 64; groups += 32) {
              const EnvgLds p = plan_envg_lds(edges, lpN, 96, C, mt, 4096 + 1, groups, (flags & 1) != 0, (flags & 2) != 0, 128, 8960, 0);
              std::vector<unsigned char> buf((size_t)p.dynamic, 0);
              auto mark = [&](long long off, long long n) {
                for (long long i = 0; i < n; i++) {
                  if (off + i >= (long long)buf.size()) {
                    bad++;
                    return;
                  }
                  bad += buf[(size_t)(off + i)] != 0;
                  buf[(size_t)(off + i)] = 1;
                }
              };
              if (p.map_lds) mark(0, (long long)edges * 48);
              if (p.fat_lds) mark(p.fat_off, (long long)lpN * 96);
              for (int g = 0; g < groups; g++) {
                mark(p.grp_off + (long long)g * p.grp_stride, (long long)C * 8);
                mark(p.grp_off + (long long)g * p.grp_stride + p.cnt_off, mt * 4);
              }
              bad += p.fat_off % 16 != 0 || p.grp_off % 16 != 0 || p.grp_stride % 8 != 0 || p.cnt_off % 8 != 0;
              bad += p.granted % TC_LDS_STEP != 0 || p.granted < p.dynamic + 128 || p.workgroups != (4097 + groups - 1) / groups;
              bad += p.map_lds && !(flags & 1);
            }
  printf("bad %lld\n", bad);
  return bad != 0;
}
#endif
"""
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc")]


def _write_src(d):
    src = os.path.join(str(d), "envg_lds_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d):
    lib = os.path.join(str(d), "libtc_envg_lds.so")
    subprocess.check_call(["c++"] + FLAGS + ["-shared", "-fPIC", "-o", lib, _write_src(d)])
    return C.CDLL(lib)


def build_program(d, sanitize=True):
    """-> path of the stand-alone program (its own main), with -fsanitize=address,undefined unless told otherwise"""
    exe = os.path.join(str(d), "envg_lds_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["c++"] + FLAGS + san + ["-DENVG_LDS_MAIN", "-o", exe, _write_src(d)])
    return exe


def envg_lds(L, total_edges, lpN, C_, N, info_every, map_switch=True, static_bytes=0, frame_lds=0, pad=0,
             groups=ENVS_PER_WG):
    a = np.array([total_edges, lpN, LP_NODE_BYTES, C_, MAX_TERMS, N, groups, int(info_every), int(map_switch), static_bytes,
                  frame_lds, pad], dtype=np.int32)
    out = np.zeros(len(FIELDS), dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    L.envg_lds(a.ctypes.data_as(ip), out.ctypes.data_as(ip))
    return dict(zip(FIELDS, (int(v) for v in out)))


def align_up(v, a):
    return (v + a - 1) // a * a


def static_lds(ep=False, ctrl=False, groups=ENVS_PER_WG):
    """the static LDS of the kernel, from its declarations in k_envg.h: g_cam_idx (int per env); with the episode
    accounting g_ep_len (int) and g_ep_ret (double); with the controller g_drv_man, g_drv_draws (int) and g_drv_ou (double)"""
    return groups * 4 + (groups * 12 if ep else 0) + (groups * 16 if ctrl else 0)


def launch_request(total_edges, lpN, C_, info_every, map_switch=True, groups=ENVS_PER_WG):
    """dynamic LDS bytes the launch asks for, and whether the edge records are part of it: the records only when every step
    reads them and they are at most 40 KB; the fat lanepath nodes when at most 56 KB; then, 16-byte aligned, per env C doubles
    and TC_MAX_TERMS ints; the whole rounded up to 16 bytes"""
    map_bytes = align_up(total_edges * EDGE_BYTES, 16)
    fat_bytes = lpN * LP_NODE_BYTES
    map_lds = map_switch and info_every and map_bytes <= MAP_CAP
    fat_lds = map_switch and fat_bytes <= FAT_CAP
    off = (map_bytes if map_lds else 0) + (fat_bytes if fat_lds else 0)
    off = align_up(off, 16) + groups * (C_ * 8 + MAX_TERMS * 4)
    return align_up(off, 16), bool(map_lds), bool(fat_lds)
