"""The clip-pass pair test of tinycarlo_amd/csrc/tc_clip.h on the CPU: the header is built alone by the host compiler
into a camera stage that runs a pair of clip passes as ONE pass over the concatenated list wherever tc_clip_pair_test
says "merge" and in the literal two-pass form otherwise.  Its draw list (integer pixels and the f64 coordinates behind
them) must equal the oracle's orc_capture_segments bit for bit -- the merged pass has no tolerance.

The whole map is one group with global node ids, the way the frame kernel holds a bundled map; `per_layer` runs the
same code layer by layer (camera.py's own loop), where fewer pairs have both lists.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
from common import FUZZ_MAPS, ROOT, setup

MAPS = ["simple_layout", "knuffingen", "stress_graph"] + FUZZ_MAPS

SHIM = r"""
#include "tc_clip.h"
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

static void matmul(const double* A, const double* B, double* Cm, int n, int k, int p) {  // numpy's dgemm association
  for (int i = 0; i < n; i++)
    for (int j = 0; j < p; j++) {
      double acc = 0.0;
      for (int t = 0; t < k; t++) acc = __builtin_fma(A[i * k + t], B[t * p + j], acc);
      Cm[i * p + j] = acc;
    }
}
// camera.py:112-122, stored into P[t]
static void move_to_plane(double* P, int o, int t, double tz) {
  const double d0 = P[3 * o] - P[3 * t], d1 = P[3 * o + 1] - P[3 * t + 1], d2 = P[3 * o + 2] - P[3 * t + 2];
  if (d2 == 0) {
    P[3 * t] = P[3 * t + 1] = P[3 * t + 2] = NAN;
    return;
  }
  const double tt = (tz - P[3 * t + 2]) / d2;
  const double a = P[3 * t] + tt * d0, b = P[3 * t + 1] + tt * d1, c = P[3 * t + 2] + tt * d2;
  P[3 * t] = a;
  P[3 * t + 1] = b;
  P[3 * t + 2] = c;
}
// one literal pass: list first, then the moves in list order
static void literal_pass(double* P, const int* E, int ne, unsigned char* flg, int bit, int which, double tz, int* list) {
  int n = 0;
  for (int e = 0; e < ne; e++)
    if (tc_clip_sel(flg[E[2 * e]], flg[E[2 * e + 1]], bit) == which) list[n++] = e;
  for (int i = 0; i < n; i++) {
    const int a = E[2 * list[i]], b = E[2 * list[i] + 1];
    const int t = which == 1 ? a : b, o = which == 1 ? b : a;
    move_to_plane(P, o, t, tz);
    flg[t] |= (unsigned char)bit;
  }
}
static int32_t np_int32(double v) {
  if (!(v > -2147483649.0 && v < 2147483648.0)) return INT32_MIN;
  return (int32_t)v;
}

// stats[2 * pair + 0] = TC_CLIP_* of the pair test, stats[2 * pair + 1] = n1 | n2 << 16; summed over the groups in cnt[]:
// cnt[4 * pair + 0..3] = groups with the pair empty / one list only / both and merged / both and refused
extern "C" int clip_capture(int Cn, const int* node_off, const int* edge_off, const double* nodes, const int* edges_g,
                            const double* Ecam, const double* Kcam, int W, int H, double max_range, double x, double y,
                            double cth, double sth, int merge, int per_layer, int32_t* seg_i, double* seg_f, int max,
                            int* cnt) {
  double R[16] = {cth, -sth, 0, 0, sth, cth, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double Tm[16] = {1, 0, 0, -x, 0, 1, 0, -y, 0, 0, 1, 0, 0, 0, 0, 1};
  double car3d[16], pose[12];
  matmul(R, Tm, car3d, 4, 4, 4);
  matmul(Ecam, car3d, pose, 3, 4, 4);
  int count = 0;
  const int ngrp = per_layer ? Cn : 1;
  for (int g = 0; g < ngrp; g++) {
    const int l0 = per_layer ? g : 0, l1 = per_layer ? g + 1 : Cn;
    const int n0 = node_off[l0], nn = node_off[l1] - n0, e0 = edge_off[l0], ne = edge_off[l1] - e0;
    std::vector<double> P(3 * nn + 3), pp(2 * nn + 2);
    std::vector<unsigned char> flg(nn + 1), vis(nn + 1);
    std::vector<int> E(2 * ne + 2), list(2 * ne + 2);
    for (int e = 0; e < 2 * ne; e++) E[e] = edges_g[2 * e0 + e] - n0;
    for (int i = 0; i < nn; i++) {
      double h[4] = {nodes[2 * (n0 + i)], nodes[2 * (n0 + i) + 1], 0.0, 1.0};
      matmul(pose, h, &P[3 * i], 3, 4, 1);
      flg[i] = P[3 * i + 2] < 0 ? 1 : 0;  // camera.py:70
    }
    for (int pair = 0; pair < 2; pair++) {
      const int bit = pair ? 2 : 1, mark = pair ? TC_CLIP_MARK1 : TC_CLIP_MARK0;
      const double tz = pair ? -max_range : -0.0000001;
      if (pair)
        for (int i = 0; i < nn; i++) flg[i] |= P[3 * i + 2] > -max_range ? 2 : 0;  // camera.py:80, mutated depths
      int n1, n2;
      const int r = tc_clip_pair_test(E.data(), ne, flg.data(), bit, mark, list.data(), &n1, &n2);
      const int both = (r & 3) == 3;
      cnt[4 * pair + ((r & 3) == 0 ? 0 : !both ? 1 : (r & TC_CLIP_MERGE) ? 2 : 3)]++;
      if (merge && (r & TC_CLIP_MERGE)) {
        for (int i = 0; i < n1 + n2; i++) {
          move_to_plane(P.data(), list[2 * i + 1], list[2 * i], tz);
          flg[list[2 * i]] |= (unsigned char)bit;
        }
      } else {
        literal_pass(P.data(), E.data(), ne, flg.data(), bit, 1, tz, list.data());
        literal_pass(P.data(), E.data(), ne, flg.data(), bit, 2, tz, list.data());
      }
    }
    for (int i = 0; i < nn; i++) {  // camera.py:133-142, 90-93
      double h[3];
      matmul(Kcam, &P[3 * i], h, 3, 3, 1);
      pp[2 * i] = h[0] / h[2];
      pp[2 * i + 1] = h[1] / h[2];
      vis[i] = (pp[2 * i] > 0) && (pp[2 * i] < W) && (pp[2 * i + 1] > 0) && (pp[2 * i + 1] < H) && (flg[i] & 3) == 3;
    }
    for (int e = 0; e < ne; e++) {  // camera.py:95
      const int a = E[2 * e], b = E[2 * e + 1];
      if (!(vis[a] || vis[b])) continue;
      if (count < max) {
        int layer = l0;
        for (int c = l0 + 1; c < l1; c++) layer += (e0 + e) >= edge_off[c];
        int32_t* o = seg_i + 5 * count;
        o[0] = layer;
        o[1] = np_int32(pp[2 * a]);
        o[2] = np_int32(pp[2 * a + 1]);
        o[3] = np_int32(pp[2 * b]);
        o[4] = np_int32(pp[2 * b + 1]);
        double* f = seg_f + 4 * count;
        f[0] = pp[2 * a];
        f[1] = pp[2 * a + 1];
        f[2] = pp[2 * b];
        f[3] = pp[2 * b + 1];
      }
      count++;
    }
  }
  return count;
}

// the pair test alone on a hand-made graph: flags in, TC_CLIP_* out
extern "C" int pair_test(const int* edges, int ne, unsigned char* flg, int bit, int mark) {
  std::vector<int> list(2 * ne + 2);
  int n1, n2;
  return tc_clip_pair_test(edges, ne, flg, bit, mark, list.data(), &n1, &n2);
}
"""

FIRST, SECOND, MERGE = 1, 2, 4  # TC_CLIP_*
# Two of the random maps cannot give both answers, whatever the pose (the graphs are in tests/golden/fuzz200x.json):
# fuzz2001 is one node with a self-loop -- no edge ever straddles a plane;
NEVER_BOTH_LISTS = {"fuzz2001"}
# fuzz2002 is the chain 0 -> 1 -> 2 -> 3 with nodes 1 and 2 at the same point (always on the same side of a plane) and
# the edge (0, 1) listed twice, plus self-loops: the only second-list / first-list edge beside (2, 3) is the doubled
# (0, 1), two moves of one target -- every pair with both lists is a chain inside one list, which is refused.
NEVER_MERGEABLE = {"fuzz2002"}


def build_shim(d):
    src, lib = os.path.join(str(d), "clip_shim.cpp"), os.path.join(str(d), "libtc_clip.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"), "-o", lib, src])
    L = C.CDLL(lib)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.clip_capture.argtypes = [C.c_int, ip, ip, dp, ip, dp, dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                               C.c_double, C.c_double, C.c_int, C.c_int, ip, dp, C.c_int, ip]
    L.pair_test.argtypes = [ip, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int]
    return L


class ClipStage:
    """The shim's camera stage on one map / camera, and the oracle's beside it."""

    def __init__(self, L, map_name, res_key="r64"):
        self.L = L
        _, m, car, cam = setup(map_name, res_key)
        self.m = m
        f = m.flat()
        self.Cn = len(f["node_count"])
        self.node_off = np.concatenate([[0], np.cumsum(f["node_count"])]).astype(np.int32)
        self.edge_off = np.concatenate([[0], np.cumsum(f["edge_count"])]).astype(np.int32)
        self.nodes = np.ascontiguousarray(f["nodes"], dtype=np.float64)
        self.edges_g = np.ascontiguousarray(f["edges"] + np.repeat(self.node_off[:-1], f["edge_count"])[:, None], dtype=np.int32)
        self.E = np.ascontiguousarray(np.asarray(cam.E, dtype=np.float64).reshape(-1))
        self.K = np.ascontiguousarray(np.asarray(cam.K, dtype=np.float64).reshape(-1))
        self.H, self.W = int(cam.resolution[0]), int(cam.resolution[1])
        self.max_range = float(cam.max_range)
        self.oracle = orc.Oracle(m, car, cam, orc.FMT_CLASSES, 1)
        cap = int(self.edge_off[-1]) + 1
        self.seg_i, self.seg_f = np.zeros((cap, 5), dtype=np.int32), np.zeros((cap, 4), dtype=np.float64)

    def capture(self, x, y, theta, merge=1, per_layer=0, mode=orc.MATH_PORTABLE):
        """-> (seg_i, seg_f, cnt[8]) of the shim at this pose"""
        cnt = np.zeros(8, dtype=np.int32)
        cth, sth = orc.lib().orc_trig(1, -theta, 0.0, mode), orc.lib().orc_trig(0, -theta, 0.0, mode)
        n = self.L.clip_capture(self.Cn, orc._ip(self.node_off), orc._ip(self.edge_off), orc._dp(self.nodes),
                                orc._ip(self.edges_g), orc._dp(self.E), orc._dp(self.K), self.W, self.H, self.max_range,
                                x, y, cth, sth, merge, per_layer, orc._ip(self.seg_i), orc._dp(self.seg_f),
                                len(self.seg_i), orc._ip(cnt))
        assert n <= len(self.seg_i)
        return self.seg_i[:n].copy(), self.seg_f[:n].copy(), cnt

    def reference(self, x, y, theta, mode=orc.MATH_PORTABLE):
        orc.set_math_mode(mode)
        st = self.oracle.state
        st["x"][0], st["y"][0], st["theta"][0] = x, y, theta
        return self.oracle.segments(0, cap=len(self.seg_i))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("tc_clip"))


def poses(stage, n, seed):
    """n poses: on the lane-line nodes with a random heading (edges straddle z = 0 right under the camera and
    z = -max_range half a metre ahead), the same pushed back along the heading by max_range and by half of it (the node
    sits on / inside the far plane), and uniform over the map's bounding box."""
    rng = np.random.default_rng(seed)
    lo, hi = stage.nodes.min(0), stage.nodes.max(0)
    out = []
    for k in range(n):
        th = rng.uniform(-np.pi, np.pi)
        if k % 4 == 3:
            p = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo))
        else:
            back = (0.0, stage.max_range, 0.5 * stage.max_range)[k % 4]
            p = stage.nodes[rng.integers(len(stage.nodes))] - back * np.array([np.cos(th), np.sin(th)])
            p = p + rng.normal(0, 0.02 * stage.max_range, 2)
        out.append((float(p[0]), float(p[1]), float(th)))
    return out


@pytest.mark.parametrize("map_name", MAPS)
def test_merged_pass_equals_the_oracle(shim, map_name):
    stage = ClipStage(shim, map_name)
    total = np.zeros(8, dtype=np.int64)
    n_poses = 160 if map_name == "knuffingen" else 400
    for per_layer in (0, 1):
        for (x, y, th) in poses(stage, n_poses, seed=7 + per_layer):
            si, sf, cnt = stage.capture(x, y, th, merge=1, per_layer=per_layer)
            ri, rf = stage.reference(x, y, th)
            assert si.shape == ri.shape and np.array_equal(si, ri), (map_name, per_layer, x, y, th)
            assert sf.tobytes() == rf.tobytes(), (map_name, per_layer, x, y, th)  # NaNs included: bit for bit
            total += cnt
    print(map_name, "pairs 1+2 / 3+4: empty, one list, merged, refused:", total[:4].tolist(), total[4:].tolist())
    # the poses reach both answers of the pair test on every map whose graph allows both
    if map_name in NEVER_BOTH_LISTS:
        assert total[1] + total[2] + total[3] + total[5] + total[6] + total[7] == 0, total
    elif map_name in NEVER_MERGEABLE:
        assert total[2] + total[6] == 0 and total[3] + total[7] > 0, total
    else:
        assert total[2] + total[6] > 0, total
        assert total[3] + total[7] > 0, total


def test_literal_form_equals_the_oracle(shim):
    """merge = 0: the shim's own four passes are the reference's (so a failure above is the merged pass's)"""
    stage = ClipStage(shim, "stress_graph")
    for (x, y, th) in poses(stage, 100, seed=3):
        si, sf, _ = stage.capture(x, y, th, merge=0)
        ri, rf = stage.reference(x, y, th)
        assert np.array_equal(si, ri) and sf.tobytes() == rf.tobytes()


def _pair(shim, edges, flg, bit=1, mark=32):
    e = np.ascontiguousarray(edges, dtype=np.int32)
    f = np.ascontiguousarray(flg, dtype=np.uint8)
    return shim.pair_test(orc._ip(e), len(e), f.ctypes.data_as(C.POINTER(C.c_uint8)), bit, mark)


@pytest.mark.parametrize("bit,mark", [(1, 32), (2, 64)])
def test_hand_made_chains(shim, bit, mark):
    """3-node chains, flags = membership before the pair (in / out of the set).

    Condition (b) has no configuration of its own: an end that stays is in the set and a target is not, so a chain in
    which pass 1 moves or adds a node that pass 2 reads is either a shared target (a) or an edge that pass 1 hands to
    pass 2 (c) -- tc_clip.h's header gives the argument.  The "(b)" case below is therefore the "(c)" chain with its
    edges in another order; it is kept because it is the reading of the chain that the condition names."""
    IN, OUT = bit, 0
    # mergeable: 0 out <- 1 in (first list, target 0), 1 in -> 2 out (second list, target 2)
    assert _pair(shim, [[0, 1], [1, 2]], [OUT, IN, OUT], bit, mark) == FIRST | SECOND | MERGE
    # (a) node 1 is the target of both passes: (1, 0) has e[0] out, e[1] in; (2, 1) has e[0] in, e[1] out
    assert _pair(shim, [[1, 0], [2, 1]], [IN, OUT, IN], bit, mark) == FIRST | SECOND
    # (b) pass 2 reads node 1 -- as the end that stays of (1, 2) once it is in the set -- and pass 1 moves it:
    #     (1, 0) puts node 1 into the set, then (1, 2) moves node 2 along the MOVED node 1; a second-list edge
    #     elsewhere, (3, 4), makes both lists non-empty before the pair
    assert _pair(shim, [[1, 0], [1, 2], [3, 4]], [IN, OUT, OUT, IN, OUT], bit, mark) == FIRST | SECOND
    # (c) the same edge (1, 2) seen as "pass 1 adds an edge to pass 2's list", with the second list's own edge sharing
    #     no node with the chain
    assert _pair(shim, [[3, 4], [1, 0], [1, 2]], [IN, OUT, OUT, IN, OUT], bit, mark) == FIRST | SECOND
    # (c) does not fire when the far end is a first-list target too: both end up in the set
    assert _pair(shim, [[1, 0], [1, 2], [2, 0], [3, 4]], [IN, OUT, OUT, IN, OUT], bit, mark) == FIRST | SECOND | MERGE
    # a chain inside ONE list (node 1 the target of two first-list edges): order matters there, refused
    assert _pair(shim, [[1, 0], [1, 2], [3, 4]], [IN, OUT, IN, IN, OUT], bit, mark) == FIRST | SECOND
    # one list empty / both empty: nothing to merge
    assert _pair(shim, [[0, 1], [1, 2]], [OUT, IN, IN], bit, mark) == FIRST
    assert _pair(shim, [[0, 1], [1, 2]], [IN, IN, OUT], bit, mark) == SECOND
    assert _pair(shim, [[0, 1], [1, 2]], [IN, IN, IN], bit, mark) == 0
