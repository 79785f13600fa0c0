// tinycarlo_hip.hip -- libtinycarlo_hip.so: kernels + C ABI (include/tinycarlo_hip.h).
//
// Build (csrc/Makefile): hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared
//
// What the kernel stages share lives in device-only headers included below in a fixed order
// (k_*.h; the tc_*.h beside them are plain arithmetic that the tests also build with the host compiler):
//   k_probe.h    timing / marker probes and the ablation switches (in no shipped kernel)
//   k_common.h   LDS layout, the env's LiveLds record, KArgs / MultiArgs, wavefront helpers
//   k_feat.h     reward / termination terms, per-env cars, camera bank, episodes, controller (the FEAT template mask)
//   k_collect.h  the sample buffer's kernels (tc_collect: scan, rank, claim, copy; tc_collect_link); no env handle, no template
//   k_history.h  frame histories out of the sample buffer (tc_history_resolve; tc_gather_frames, a template compiled in part 0)
// The kernel stages follow in this file, each with its own argument block (RArgs, StepArgs, FrameArgs, NArgs), then the
// host side (from `// Host side: C ABI` down):
//   camera       phase C  transform -> 4 clip passes -> project -> visibility -> draw list (camera.py:52-110)
//   simulate     phase A  kinematics + lanepath tracking + CTE/heading   (car.py:70-148, 46-53)
//                phase B  nearest lane-line edge per layer + distance    (layer.py:33-44, car.py:55-64)
//                tc_env_kernel<K, CAM, FEAT>: one 64-lane wavefront (= one workgroup) per env;
//                tc_envg_kernel<FEAT>: the same two phases for K-step calls, 8 lanes per env
//   raster       tc_raster_kernel<..>: cv2.polylines of the draw list into LDS bit-planes (renderer.py:36-51), expanded to
//                uint8 and stored with 16-byte-per-lane coalesced stores (zeros included: a class-mask frame is written
//                exactly once)
//   frame        tc_frame_kernel<..>: camera + raster of one (step, env) frame per workgroup, from the pose the simulate
//                launch left; tc_step_kernel<..>: simulate + camera + raster of an env in one launch
//   noise        tc_noise_kernel: NoiseObservationWrapper over a finished observation
//   others       tc_order_kernel, tc_gate_kernel, tc_unpack_bits_kernel
//   tables       the instantiation lists of the parts (TC_PART) and the *_kernel_of tables
// Which of these kernels a call launches -- one fused tc_step_kernel, or a simulate launch with tc_frame_kernel behind or
// beside it, or a simulate launch with the camera stage and tc_raster_kernel behind it -- is plan_call()'s choice (tc_plan.h).
//
// TC_PART: the default library is this file compiled as six translation units side by side (Makefile), because one
// compiler process over every kernel takes ~25 minutes: part 0 = the host code and every kernel but those of the other
// parts, parts 1 / 3 = the tc_drive_step_kernel family (class masks / rgb), parts 4 / 5 = the tc_step_kernel family (class
// masks / rgb), part 2 = the packed-observation kernels (TC_FMT_CLASSES_BITS frame / recover / raster variants,
// tc_unpack_bits_kernel).  Parts 1-5 hold explicit instantiations only; part 0 declares them
// `extern template`, so its kernel tables (step_kernel_of, ...) take the addresses without compiling the bodies.  Every
// kernel is compiled from the same text with the same flags as in a one-unit build (TC_PART undefined: make dev, make
// timing).  The lists of instantiations are TC_INST_* below and follow Kcodes / Thicks / Fmts / FrameFmts / DriveFeats.
// (TC_PLAIN_KERNEL, which keeps the kernels that are no templates in part 0, is defined in k_common.h.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tinycarlo_hip.h"
#include "tc_device.h"
#include "tc_rng.h"
#include "tc_ctrl.h"
#include "tc_clip.h"
#include "tc_cull.h"

#include "k_probe.h"
#include "k_common.h"
#include "k_feat.h"
#include "k_collect.h"
#include "k_history.h"

// ---------------------------------------------------------------------------------------------
// Per-lane register cache of the map: lane `tid` keeps nodes / edges (w*K + k)*64 + tid, k < K, of window w.
// Maps up to 64*K nodes and edges (all bundled ones with K = 5 or 13) are a single window that is loaded once at
// kernel start -- behind the latency of phase A -- and then serves every pass of phases B and C; larger maps
// reload window by window inside each pass.
template <int K>
struct MapCache {
  double2 nd[K];
  int2 ed[K];
};

// slot k of lane tid <-> node (edge) base + k*64 + tid, valid below `end`
template <int K>
__device__ inline void cache_nodes(MapCache<K>& c, const DevMap& m, int base, int end, int tid) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int i = base + k * TC_NT + tid;
    c.nd[k] = i < end ? m.nodes[i] : make_double2(0.0, 0.0);
  }
}
template <int K>
__device__ inline void cache_nodes_from(MapCache<K>& c, const double2* nodes, int base, int end, int tid) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int i = base + k * TC_NT + tid;
    c.nd[k] = i < end ? nodes[i] : make_double2(0.0, 0.0);
  }
}
template <int K>
__device__ inline void cache_edges_from(MapCache<K>& c, const int2* edges_g, int base, int end, int nbase, int tid) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int e = base + k * TC_NT + tid;
    int2 ed = e < end ? edges_g[e] : make_int2(nbase, nbase);
    c.ed[k] = make_int2(ed.x - nbase, ed.y - nbase);
  }
}
// node ids are stored relative to `nbase` (the first node of the camera group; 0 for whole-map use)
template <int K>
__device__ inline void cache_edges(MapCache<K>& c, const DevMap& m, int base, int end, int nbase, int tid) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int e = base + k * TC_NT + tid;
    int2 ed = e < end ? m.edges_g[e] : make_int2(nbase, nbase);
    c.ed[k] = make_int2(ed.x - nbase, ed.y - nbase);
  }
}

// camera.py:70-86: one of the four fix-up loops.  `bit` selects the membership flag (1 = idx_front,
// 2 = idx_in_range).  The reference builds the edge list first and then mutates nodes in list
// (= edge) order; updates of different target nodes are independent (a target is never read as
// the "other" end within one pass), so each target node's chain is replayed in ascending edge
// index by the lane that owns the chain's first edge.  List entries carry (edge, target | other << 16)
// so the chain loops touch LDS only.
// Works on one camera group: edges ge0 .. ge0+ne-1 (ids below are relative to ge0), node ids relative to gn0.
// camera.py:112-122 __point_on_line_at_z(p0 = P[o], p1 = P[t], tz), stored into P[t]
__device__ __forceinline__ void cam_move_to_plane(double* Px, double* Py, double* Pz, int o, int t, double tz) {
  double d0 = Px[o] - Px[t], d1 = Py[o] - Py[t], d2 = Pz[o] - Pz[t];
  if (d2 == 0) {
    double qn = __longlong_as_double(0x7ff8000000000000LL);
    Px[t] = qn;
    Py[t] = qn;
    Pz[t] = qn;
  } else {
    double tt = (tz - Pz[t]) / d2;
    double aa = Px[t] + tt * d0, bb = Py[t] + tt * d1, cc = Pz[t] + tt * d2;
    Px[t] = aa;
    Py[t] = bb;
    Pz[t] = cc;
  }
}

// The exact replay of one fix-up pass from its list of n straddling edges (edge id, target | other << 16): every target
// node's chain of moves in ascending edge index, run by the lane that holds the chain's first edge.  range_too: the
// target's idx_in_range bit is refreshed from its new depth (camera.py:80 reads the depths passes 1-2 left behind).
__device__ inline void cam_chain_replay(double* Px, double* Py, double* Pz, unsigned char* flg, int bit, double tz,
                                        const int* list, int n, double max_range, bool range_too, int tid) {
  for (int k = tid; k < n; k += TC_NT) {
    const int e = list[2 * k];
    const int t = list[2 * k + 1] & 0xffff;
    bool first = true;
    for (int j = 0; j < n; j++)
      if ((list[2 * j + 1] & 0xffff) == t && list[2 * j] < e) first = false;
    if (!first) continue;
    int cur = e, o = (unsigned)list[2 * k + 1] >> 16;  // the end that stays
    for (int guard = 0; guard < n; guard++) {
      cam_move_to_plane(Px, Py, Pz, o, t, tz);
      int nxt = 0x7fffffff, no = 0;
      for (int j = 0; j < n; j++) {
        const int ej = list[2 * j], pj = list[2 * j + 1];
        if ((pj & 0xffff) == t && ej > cur && ej < nxt) {
          nxt = ej;
          no = (unsigned)pj >> 16;
        }
      }
      if (nxt == 0x7fffffff) break;
      cur = nxt;
      o = no;
    }
    unsigned int f = flg[t] | (unsigned)bit;
    if (range_too) f = (f & ~2u) | (Pz[t] > -max_range ? 2u : 0u);
    flg[t] = (unsigned char)f;
  }
}

__device__ inline int2 cam_project(const double* K, double X, double Y, double Z, double& u, double& v);

// Phase C of one camera group whose nodes and edges sit in the wavefront's registers (one window: every bundled map).
// camera.py:52-110 reads the whole node / edge arrays in each of its steps; here the flags of an edge's two ends are
// carried in a register per edge slot (`ff`) and refreshed only after a pass that moved something, so a fix-up pass in
// which no edge straddles the plane -- or only a handful, the usual case -- costs a few compares per slot instead of a
// round of LDS traffic, and the straddling edges are compacted (ballot + mbcnt, no atomics) so that the move code runs
// ONCE per pass, on the low lanes, instead of once per register slot.
//   idx_in_range (camera.py:80) is evaluated on the depths left by passes 1-2: it is set here from the transformed depth
// and refreshed for exactly the nodes those passes move -- the same values, without a pass over all nodes.
// Appends the group's visible edges to the draw list at segg[5 * nseg ...] and advances nseg (wave-uniform).
template <int K>
__device__ __forceinline__ void cam_group_regs(const KArgs& a, const MapCache<K>& mc, const double* pose, const double* Kc,
                                               const int l0, const int l1, const int ge0, const int nn, const int ne,
                                               double* Px, double* Py, double* Pz, unsigned char* flg, int* list,
                                               int* segg, LdsIntPtr seg_lds, int& nseg, unsigned int& my_layers, const int env,
                                               const int tid) {
  const DevMap& m = a.m;
  const DevCam& cam = a.cam;
  const double max_range = cam.max_range;
#pragma unroll
  for (int k = 0; k < K; k++) {  // camera.py:124-131, 70, 80
    const int i = k * TC_NT + tid;
    if (i < nn) {
      double h[4] = {mc.nd[k].x, mc.nd[k].y, 0.0, 1.0};
      double p[3];
      d_matmul<3, 4, 1>(pose, h, p);
      Px[i] = p[0];
      Py[i] = p[1];
      Pz[i] = p[2];
      flg[i] = (unsigned char)((p[2] < 0 ? 1 : 0) | (p[2] > -max_range ? 2 : 0));
    }
  }
  lds_sync();
  TSTAMP(4);
  int ff[K];  // flags of the two ends of edge slot k: flg[ed.x] | flg[ed.y] << 8 (0 for an empty slot)
#pragma unroll
  for (int k = 0; k < K; k++) ff[k] = k * TC_NT + tid < ne ? (int)flg[mc.ed[k].x] | ((int)flg[mc.ed[k].y] << 8) : 0;
  // camera.py:71-74, 75-77 (plane z = -1e-7, flag idx_front), then 81-83, 84-86 (plane z = -max_range, flag
  // idx_in_range): one copy of the pass, looped.  Where tc_clip.h allows it -- both lists of a pair non-empty, every
  // target of the two lists its own node, no edge that the first pass would add to the second's list -- the pair runs
  // as ONE pass over the concatenated list (one compaction, one LDS round trip, one batch of divisions, one flag
  // refresh); otherwise the first list alone is used, it sits at the head of the concatenated one, and the second
  // pass follows in its literal form from the refreshed flags.
  const bool merge_on = a.clip_merge != 0;
#pragma nounroll
  for (int pass = 0; pass < 4 && !DBG_ON(a.dbg, DBG_SKIP_CLIP); pass++) {
    const int bit = pass < 2 ? 1 : 2, mark = pass < 2 ? TC_CLIP_MARK0 : TC_CLIP_MARK1;
    const double tz = pass < 2 ? -0.0000001 : -max_range;
    int s1 = 0, s2 = 0;  // bit k: slot k is in the pair's first (target e[0]) / second (target e[1]) list, flags as they stand
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int w = tc_clip_sel(ff[k] & 0xff, ff[k] >> 8, bit);
      s1 |= w == 1 ? 1 << k : 0;
      s2 |= w == 2 ? 1 << k : 0;
    }
    const bool any1 = __ballot(s1 != 0) != 0, any2 = __ballot(s2 != 0) != 0;
    if (!(pass & 1) && !any1) {  // nothing for the first pass: the flags stand, s2 is the second pass's list
      TSTAMP(17 + pass);  // (a pass that does not run still leaves its stamp: phase_clock.py reads all of 17-19 per frame)
      pass++;
    }
    bool merged = !(pass & 1) && merge_on && any2;  // (wave-uniform, like every decision below)
    if (pass & 1) {
      if (!any2) {
        if (pass < 3) TSTAMP(17 + pass);
        continue;
      }
      s1 = 0;
    } else if (!merged) {
      s2 = 0;
    }
    int n = 0, n1 = 0;
#pragma nounroll
    for (int h = 0; h < 2; h++) {  // the first list's entries, then the second's
      const int sm = h ? s2 : s1;
      if (__ballot(sm != 0) == 0) continue;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const bool s_k = (sm >> k) & 1;
        const unsigned long long mk = __ballot(s_k);
        if (s_k) {
          const int j = n + wave_rank(mk);
          const int t = h ? mc.ed[k].y : mc.ed[k].x, o = h ? mc.ed[k].x : mc.ed[k].y;
          list[2 * j] = k * TC_NT + tid;
          list[2 * j + 1] = t | (o << 16);
          // "target of the first list" for the test below (lanes sharing the node write the same byte)
          if (merged && h == 0) flg[t] = (unsigned char)((ff[k] & 0xff) | mark);
        }
        n += __popcll(mk);
      }
      if (h == 0) n1 = n;
    }
    lds_sync();
    if (merged) {  // condition (c) of tc_clip.h: an edge the first pass would hand to the second
      bool joins = false;
#pragma unroll
      for (int k = 0; k < K; k++)
        if (k * TC_NT + tid < ne && !(ff[k] & bit) && !((ff[k] >> 8) & bit))
          joins |= tc_clip_joins_second(flg[mc.ed[k].x], flg[mc.ed[k].y], bit, mark) != 0;
      if (__ballot(joins) != 0) {
        merged = false;
        n = n1;
      }
    }
    // the usual case: every straddling edge has a target node of its own -> one move each, order irrelevant
    bool dup;
    int mine;
    for (;;) {
      dup = n > TC_NT;
      mine = 0;
      if (n <= TC_NT) {
        // lane j < n takes list entry j; the target nodes are compared lane against lane through v_readlane (the loop
        // over the list in LDS was one dependent LDS round trip per entry, four passes per frame)
        mine = tid < n ? list[2 * tid + 1] : -1;
        const int my_t = mine & 0xffff;
        for (int j = 0; j < n; j++) {
          const int tj = __builtin_amdgcn_readlane(my_t, j);
          dup |= tid < n && j != tid && tj == my_t;
        }
      }
      dup = __ballot(dup) != 0;
      if (!merged || !dup) break;
      merged = false;  // a target shared between the lists or inside one: the first list alone, the literal way
      n = n1;
    }
    if (!dup) {
      if (tid < n) {
        const int t = mine & 0xffff, o = (unsigned)mine >> 16;
        cam_move_to_plane(Px, Py, Pz, o, t, tz);
        unsigned int f = flg[t] | (unsigned)bit;
        if (pass < 2) f = (f & ~2u) | (Pz[t] > -max_range ? 2u : 0u);
        flg[t] = (unsigned char)f;
      }
    } else {
      cam_chain_replay(Px, Py, Pz, flg, bit, tz, list, n, max_range, pass < 2, tid);
    }
    lds_sync();
#pragma unroll
    for (int k = 0; k < K; k++) ff[k] = k * TC_NT + tid < ne ? (int)flg[mc.ed[k].x] | ((int)flg[mc.ed[k].y] << 8) : 0;
    if (pass < 3) TSTAMP(17 + pass);
    if (merged) {  // both passes of the pair are done: the second one's interval reads as empty
      pass++;
      if (pass < 3) TSTAMP(17 + pass);
    }
  }
  TSTAMP(5);
  // Only nodes in front AND in range can be "visible" (camera.py:92-93), and an edge is drawn when one of its ends is
  // (camera.py:95) -- with the pixel coordinates of BOTH ends.  So the nodes worth projecting (two f64 divisions each)
  // are the ends of edges that have an end in front and in range: mark them, compact them, project them in one
  // lane-parallel pass.
  int cand = 0;  // bit k: edge slot k has an end in front and in range
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int fa = ff[k] & 0xff, fb = ff[k] >> 8;
    if ((fa & 3) == 3 || (fb & 3) == 3) {  // (lanes sharing a node write the same value: nothing else changes here)
      cand |= 1 << k;
      flg[mc.ed[k].x] = (unsigned char)(fa | 16);
      flg[mc.ed[k].y] = (unsigned char)(fb | 16);
    }
  }
  lds_sync();
  int ncand = 0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int i = k * TC_NT + tid;
    const bool c = i < nn && (flg[i] & 16);
    const unsigned long long mk = __ballot(c);
    if (c) list[ncand + wave_rank(mk)] = i;
    ncand += __popcll(mk);
  }
  lds_sync();
  for (int k = tid; k < ncand; k += TC_NT) {  // camera.py:133-142, 90
    const int i = list[k];
    double u, v;
    int2 q = cam_project(Kc, Px[i], Py[i], Pz[i], u, v);
    const bool vis = (u > 0) && (u < cam.W) && (v > 0) && (v < cam.H) && (flg[i] & 3) == 3;
    ((int2*)Px)[i] = q;  // renderer.py:43,50 np.int32(...)
    if (vis) flg[i] |= 4;
  }
  lds_sync();
  TSTAMP(6);
  // camera.py:95: the edges with a visible end, compacted first (edge id, end nodes) so that the code that emits a
  // segment runs once over a dense list instead of once per register slot with a few lanes active in each
  int ndraw = 0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    bool draw = false;
    if ((cand >> k) & 1) draw = ((flg[mc.ed[k].x] | flg[mc.ed[k].y]) & 4) != 0;  // a visible end
    const unsigned long long mk = __ballot(draw);
    if (draw) {
      const int j = ndraw + wave_rank(mk);
      list[2 * j] = k * TC_NT + tid;
      list[2 * j + 1] = mc.ed[k].x | (mc.ed[k].y << 16);
    }
    ndraw += __popcll(mk);
  }
  lds_sync();
  for (int j = tid; j < ndraw; j += TC_NT) {  // both ends were marked above and hold pixel coordinates
    const int e = list[2 * j], xy = list[2 * j + 1];
    const int2 pa = ((int2*)Px)[xy & 0xffff], pb = ((int2*)Px)[(unsigned)xy >> 16];
    int layer = l0;
    for (int c = l0 + 1; c < l1; c++) layer += (ge0 + e) >= m.edge_off[c];
    my_layers |= 1u << layer;
    const int js = nseg + j;  // < seg_cap == total edge count
    if (js < a.seg_lds_cap) {  // the raster stage of this wavefront reads it back from LDS: no store -> load round trip
      const LdsIntPtr o = seg_lds + 5 * js;
      o[0] = layer;
      o[1] = pa.x;
      o[2] = pa.y;
      o[3] = pb.x;
      o[4] = pb.y;
    } else {
      int* o = segg + 5 * js;
      o[0] = layer;
      o[1] = pa.x;
      o[2] = pa.y;
      o[3] = pb.x;
      o[4] = pb.y;
    }
  }
  nseg += ndraw;
  lds_sync();  // the next group reuses the node buffer
}

template <int K>
__device__ inline void cam_fixup_pass(MapCache<K>& mc, const DevMap& m, bool reload, int ge0, int ne, int gn0, int nwin,
                                      double* Px, double* Py, double* Pz, unsigned char* flg, int bit, bool target_e0,
                                      double tz, int* list, int* cnt, int tid) {
  // *cnt was zeroed (and a barrier passed) before the call
  if (!reload) {
    // The group's edges sit in this wavefront's registers (one window).  Typical frame: a handful of edges straddle
    // the plane, each with a target node of its own.  Then no list is needed at all: the lane holding a straddling
    // edge moves that edge's target itself.  Only when two straddling edges share a target does the order of
    // camera.py's loop matter -- detected by every selecting lane writing its edge id into claim[target] and reading
    // it back (one wavefront: LDS operations complete in program order) -- and then the exact list replay below runs.
    int sel = 0;  // bit k: slot k of this lane straddles the plane in the direction of this pass
    int* claim = list;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int e = k * TC_NT + tid;
      if (e < ne) {
        const int2 ed = mc.ed[k];
        const bool fa = flg[ed.x] & bit, fb = flg[ed.y] & bit;
        if (target_e0 ? (!fa && fb) : (fa && !fb)) {
          sel |= 1 << k;
          claim[target_e0 ? ed.x : ed.y] = e;
        }
      }
    }
    if (__ballot(sel != 0) == 0) return;  // nothing straddles: flags, nodes, list and counter untouched
    bool dup = false;
#pragma unroll
    for (int k = 0; k < K; k++)
      if ((sel >> k) & 1) dup |= claim[target_e0 ? mc.ed[k].x : mc.ed[k].y] != k * TC_NT + tid;
    if (__ballot(dup) == 0) {
#pragma unroll
      for (int k = 0; k < K; k++)
        if ((sel >> k) & 1) {
          const int t = target_e0 ? mc.ed[k].x : mc.ed[k].y, o = target_e0 ? mc.ed[k].y : mc.ed[k].x;
          cam_move_to_plane(Px, Py, Pz, o, t, tz);
          flg[t] |= (unsigned char)bit;  // targets are distinct: no two lanes touch the same byte
        }
      __syncthreads();
      return;
    }
    __syncthreads();  // claim[] aliases the list the exact path is about to build
  }
  for (int w = 0; w < nwin; w++) {
    if (reload) cache_edges(mc, m, ge0 + w * K * TC_NT, ge0 + ne, gn0, tid);
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int e = (w * K + k) * TC_NT + tid;
      if (e < ne) {
        const int2 ed = mc.ed[k];
        const bool fa = flg[ed.x] & bit, fb = flg[ed.y] & bit;
        const bool sel = target_e0 ? (!fa && fb) : (fa && !fb);
        if (sel) {
          const int j = atomicAdd(cnt, 1);
          list[2 * j] = e;
          list[2 * j + 1] = target_e0 ? (ed.x | (ed.y << 16)) : (ed.y | (ed.x << 16));
        }
      }
    }
  }
  __syncthreads();
  cam_chain_replay(Px, Py, Pz, flg, bit, tz, list, *cnt, 0.0, false, tid);
  __syncthreads();
}

// A spawn node must exist and have an out-edge (map.py:62-64 re-draws otherwise; the host RNG mirror
// does that).  Anything else would index out of bounds, so it is replaced and flagged.
__device__ inline int checked_spawn(const DevMap& m, int node, int& status) {
  if ((unsigned)node < (unsigned)m.lpN && m.lp_fat[node].nnext > 0) return node;
  status |= TC_S_BAD_SPAWN;
  return m.first_spawnable;
}

// camera.py:133-142 for one node + the np.int32 cast of renderer.py:43,50
__device__ inline int2 cam_project(const double* K, double X, double Y, double Z, double& u, double& v) {
  double P3[3] = {X, Y, Z};
  double h[3];
  d_matmul<3, 3, 1>(K, P3, h);
  u = h[0] / h[2];
  v = h[1] / h[2];
  return make_int2(d_np_int32(u), d_np_int32(v));
}

// Caller's buffers -> LiveLds, one item per lane (one vector-memory round trip for the ~30 scalars of an env).
__device__ __forceinline__ void live_in(const KArgs& a, unsigned char* smem, int env, int mode, unsigned int flags,
                                        const int tid = threadIdx.x) {
  const tc_buffers& b = a.b;
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid < 8) {
    const double* p = b.x;
    p = tid == 1 ? b.y : p;
    p = tid == 2 ? b.theta : p;
    p = tid == 3 ? b.velocity : p;
    p = tid == 4 ? b.steering : p;
    p = tid == 5 ? b.radius : p;
    p = tid == 6 ? b.front_x : p;
    p = tid == 7 ? b.front_y : p;
    lv->d[tid] = p[env];
  } else if (tid < 16) {
    lv->lp[tid - 8] = b.local_path[env * 8 + (tid - 8)];
  } else if (tid == 16) {
    lv->lp_len = b.lp_len[env];
  } else if (tid == 17) {
    lv->last_maneuver = b.last_maneuver[env];
  } else if (tid == 18) {
    lv->needs_reset = (mode == MODE_STEP && (flags & TC_F_AUTORESET)) ? b.needs_reset[env] : 0;
  } else if (tid == 19) {
    const int c = (mode == MODE_STEP && (flags & TC_F_AUTORESET)) ? b.spawn_cursor[env] : 0;
    lv->cursor = c;
    lv->cursor0 = c;
  } else if (tid < 28) {
    const int t = tid - 20;
    lv->cnt[t] = (a.n_terms > 0 && a.term_counters) ? a.term_counters[(size_t)env * TC_MAX_TERMS + t] : 0;
  } else if (tid == 28) {
    lv->d[8] = 0;
    lv->d[9] = 0;
    lv->have_trig = 0;
  }
  lds_sync();
}

// LiveLds -> caller's buffers after the last step of the launch (not for MODE_RENDER, which changes nothing).
__device__ __forceinline__ void live_out(const KArgs& a, unsigned char* smem, int env, const int tid = threadIdx.x) {
  const tc_buffers& b = a.b;
  const LiveLds* lv = (const LiveLds*)(smem + a.lds.off_live);
  const int C = a.m.C;
  lds_sync();
  if (tid < 8) {
    double* p = b.x;
    p = tid == 1 ? b.y : p;
    p = tid == 2 ? b.theta : p;
    p = tid == 3 ? b.velocity : p;
    p = tid == 4 ? b.steering : p;
    p = tid == 5 ? b.radius : p;
    p = tid == 6 ? b.front_x : p;
    p = tid == 7 ? b.front_y : p;
    p[env] = lv->d[tid];
  } else if (tid < 16) {
    b.local_path[env * 8 + (tid - 8)] = lv->lp[tid - 8];
  } else if (tid == 16) {
    b.lp_len[env] = lv->lp_len;
  } else if (tid == 17) {
    b.last_maneuver[env] = lv->last_maneuver;
  } else if (tid == 18) {
    if (b.needs_reset) b.needs_reset[env] = (unsigned char)lv->needs_reset;
  } else if (tid == 19) {
    if (lv->cursor != lv->cursor0) b.spawn_cursor[env] = lv->cursor;
  } else if (tid < 28) {
    const int t = tid - 20;
    if (a.term_counters && t < a.n_terms) a.term_counters[(size_t)env * TC_MAX_TERMS + t] = lv->cnt[t];
  } else if (tid == 28) {
    b.cte[env] = lv->cte;
  } else if (tid == 29) {
    b.heading_error[env] = lv->he;
  } else if (tid == 30) {
    b.reward[env] = lv->reward;
  } else if (tid == 31) {
    b.terminated[env] = (unsigned char)lv->terminated;
  } else if (tid == 32) {
    b.truncated[env] = (unsigned char)lv->trunc;
  } else if (tid == 33) {
    b.status[env] = lv->status;
  } else if (tid < 34 + TC_MAX_LAYERS - 4) {  // lanes 34..45: layers 0..11
    const int l = tid - 34;
    if (l < C) {
      b.laneline_distances[(size_t)env * C + l] = lv->dist[l];
      b.nearest_edge[(size_t)env * C + l] = lv->ne[l];
    }
  } else if (tid < 50) {  // lanes 46..49: layers 12..15
    const int l = tid - 34;
    if (l < C) {
      b.laneline_distances[(size_t)env * C + l] = lv->dist[l];
      b.nearest_edge[(size_t)env * C + l] = lv->ne[l];
    }
  }
}

// The running episode of an env: caller's buffers -> LiveLds before live_in (whose barrier covers it), and back after
// live_out, by one lane that live_in / live_out leave idle.
__device__ __forceinline__ void ep_in(const KArgs& a, const EpArgs& ep, unsigned char* smem, int env, const int tid = threadIdx.x) {
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid == 50) {
    lv->ep_len = ep.length[env];
    lv->ep_ret = ep.ret[env];
  }
}
// What the env reported after the step before this launch: caller's buffers -> LiveLds, likewise before live_in (the
// TC_FEAT_CTRL kernels only: no other kernel reads the two before it has written them).
__device__ __forceinline__ void ctrl_in(const KArgs& a, unsigned char* smem, int env, const int tid = threadIdx.x) {
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid == 51) lv->cte = a.b.cte[env];
  if (tid == 52) lv->he = a.b.heading_error[env];
}
// The env's camera of the bank: caller's buffer -> LiveLds, likewise before live_in (only while a bank is installed).
__device__ __forceinline__ void cam_in(const KArgs& a, const CamBank& cb, unsigned char* smem, int env, const int tid = threadIdx.x) {
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid == 53) lv->cam_idx = cam_clamp(cb, cb.index[env]);
}
__device__ __forceinline__ void ep_out(const KArgs& a, const EpArgs& ep, unsigned char* smem, int env, const int tid = threadIdx.x) {
  const LiveLds* lv = (const LiveLds*)(smem + a.lds.off_live);
  if (tid == 50) {
    ep.length[env] = lv->ep_len;
    ep.ret[env] = lv->ep_ret;
  }
}

#ifndef TC_MIN_WAVES
#define TC_MIN_WAVES 4
#endif
// Stage 1 (simulate) for one env by one wavefront.  Returns false when nothing is to be rasterised for this env.
// always inlined: out of line, `a` would be a pointer into private memory and the whole kernel-argument struct
// (~1 KB) would be copied to scratch by every lane (the inliner's cost threshold is close: measured 47.9 k vs 47.6 k)
// One step of one env: reads and rewrites the env's LiveLds record; the caller's buffers are only touched by live_in /
// live_out (and the per-step rollout rows of `roll`).
// what the camera needs of an env's state: rear-axle position and cos / sin of MINUS the heading (car.py:159-165)
struct FramePose {
  double x, y, cth, sth;
};

// PER: the env's car constants come from its row of cr.rows (per-env cars, tc_env_set_car_per_env), else a.car.
// EP: episode length / return / time limit (tc_env_set_episodes); the running pair lives in LiveLds (ep_len, ep_ret).
// CTRL: the action comes from the built-in controller (tc_env_set_controller), computed from the cte / he the record holds
// from the step before; car_control is not read.
// need_b (wave-uniform): this step computes the lane-line distances -- the launch's last step, and every step when the
// call's plan says someone reads them (TC_FI_INFO_EVERY).  need_win: the map window is fetched into `mc` behind phase A: for
// phase B, and for the camera stage where the same wavefront runs one behind this step.
template <int K, unsigned FEAT = 0>
__device__ __forceinline__ void sim_body(const KArgs& a, unsigned char* smem, int env, int mode,
                                const void* car_control, int cdtype,
                                const int* maneuver, const int* spawn_nodes, const unsigned char* mask,
                                unsigned int flags, const RollStep& roll, const int tid, MapCache<K>& mc, FramePose& fp,
                                int& cam_row, const bool need_b, const bool need_win, const CarRows& cr = CarRows(),
                                const EpArgs& ep = EpArgs(),
                                const CtrlArgs& ct = CtrlArgs(), const CamBank& cb = CamBank(),
                                const DriveArgs& dr = DriveArgs()) {
  constexpr bool PER = (FEAT & TC_FEAT_CAR) != 0, EP = (FEAT & TC_FEAT_EP) != 0, CTRL = (FEAT & TC_FEAT_CTRL) != 0;

  TSTAMP(0);
  TSTAMP_REAL(30);
  const DevMap& m = a.m;
  const tc_buffers& b = a.b;
  // map windows of 64*K nodes / edges; one window (the usual case) is fetched now and kept in registers
  const int nwin_n = (m.total_nodes + TC_NT * K - 1) / (TC_NT * K), nwin_e = (m.total_edges + TC_NT * K - 1) / (TC_NT * K);
  const bool single = a.n_grp == 1 && !a.cam_nodes && a.grp_layer[0] == 0 && a.grp_layer[1] == m.C && nwin_n <= 1 && nwin_e <= 1;
  double* dn = (double*)(smem + a.lds.off_p);  // phase B: one double per lane-line node (aliases the camera's node buffer)

  // ---- state: all lanes read the same LDS words (broadcast)
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  // (readfirstlane: the values are wave-uniform, and the compiler has to KNOW it -- read straight from LDS they count
  // as divergent, every branch of the scalar phases below becomes an exec-mask region and the kernel triples in size)
  CarState s;
  s.x = uni_d(lv->d[0]);
  s.y = uni_d(lv->d[1]);
  s.theta = uni_d(lv->d[2]);
  s.velocity = uni_d(lv->d[3]);
  s.steering = uni_d(lv->d[4]);
  s.radius = uni_d(lv->d[5]);
  s.front_x = uni_d(lv->d[6]);
  s.front_y = uni_d(lv->d[7]);
  s.cth = uni_d(lv->d[8]);
  s.sth = uni_d(lv->d[9]);
#pragma unroll
  for (int i = 0; i < 8; i++) s.lp[i] = uni_i(lv->lp[i]);
  s.lp_len = uni_i(lv->lp_len);
  s.last_maneuver = uni_i(lv->last_maneuver);
  bool have_trig = uni_i(lv->have_trig) != 0;  // s.cth / s.sth hold cos / sin of the current heading
  const int nr = uni_i(lv->needs_reset);
  int cursor = uni_i(lv->cursor);
  int my_cnt = tid < TC_MAX_TERMS ? lv->cnt[tid] : 0;  // lane t: steps_true of term slot t
  int ep_len = EP ? uni_i(lv->ep_len) : 0;
  // which camera row this step's frame uses: the env's own (shared camera: unused), or its index into the bank
  const bool bank = (flags & TC_FI_CAM_BANK) != 0;
  cam_row = bank ? uni_i(lv->cam_idx) : env;

  int status = 0, trunc = 0;
  PathInfo pinfo;
  pinfo.ax = pinfo.ay = pinfo.bx = pinfo.by = pinfo.ori = 0;
  pinfo.valid = 0;
  bool fresh = false;  // env was (re)spawned in this launch: info is empty (car.py:47-51)
  const double* crow = PER ? cr.rows + (size_t)env * TC_CAR_NP : nullptr;
  double ctrl_steer = 0.0;  // CTRL: this step's command before noise (0 when no action is applied)
  // CTRL, drive randomisation: the maneuver in force and the OU value applied (0 when no action is applied), for the rows
  const bool drv_man = CTRL && (flags & TC_FI_DRIVE_MAN) != 0, drv_ou = CTRL && (flags & TC_FI_DRIVE_OU) != 0;
  int drive_m = 0;
  double drive_n = 0.0;
  // a re-spawn: the next episode's maneuver, and the OU value back to 0 when asked for (lane 0 stores; see DriveArgs)
  auto drive_respawn = [&]() {
    if (drv_man) {
      drive_m = drive_respawn_man<true>(dr, env, tid == 0, uni_i(dr.maneuver[env]));
      if (tid == 0) dr.maneuver[env] = drive_m;
    }
    if (drv_ou && drive_ou_reset(dr) && tid == 0) dr.ou_state[env] = 0.0;
  };
  if (mode == MODE_RESET) {
    if (PER) car_respawn<true>(cr, env, true);
    if (bank) cam_row = cam_respawn<true>(cb, env, tid == 0);
    if (CTRL) drive_respawn();
    d_reset(m, PER ? car_of<true>(a.car, crow) : a.car, s, checked_spawn(m, spawn_nodes[env], status));
    fresh = true;
    have_trig = true;
  } else if (mode == MODE_STEP) {
    if ((flags & TC_F_AUTORESET) && nr) {
      const int cur = cursor;
      int node;
      if ((flags & TC_F_DEVICE_SPAWN) && a.spawn_n > 0) {
        node = a.spawn_tab[tc_spawn_index(a.spawn_seed, (uint32_t)env, (uint32_t)cur, (uint32_t)a.spawn_n)];
      } else {
        if ((unsigned)cur >= (unsigned)b.spawn_queue_len) status |= TC_S_SPAWN_WRAPPED;  // replaying the queue
        node = b.spawn_queue[(size_t)env * b.spawn_queue_len + ((unsigned)cur % (unsigned)b.spawn_queue_len)];
      }
      if (PER) car_respawn<true>(cr, env, true);
      if (bank) cam_row = cam_respawn<true>(cb, env, tid == 0);
      if (CTRL) {
        drive_respawn();
        if (!drv_man && dr.man_rows) drive_m = maneuver[env];
      }
      d_reset(m, PER ? car_of<true>(a.car, crow) : a.car, s, checked_spawn(m, node, status));
      fresh = true;
      have_trig = true;
      cursor = cur + 1;
    } else if ((unsigned)s.lp[0] >= (unsigned)m.lpN || (unsigned)s.lp[1] >= (unsigned)m.lpN) {
      status |= TC_S_NOT_RESET;  // stepping an env that was never reset: no valid lanepath edge to index with
      trunc = 1;
      if (CTRL && dr.man_rows) drive_m = drv_man ? uni_i(dr.maneuver[env]) : maneuver[env];
    } else {
      double v, st;
      if (CTRL) {  // (every input is wave-uniform; double arithmetic has no scalar form, so the lanes all compute it)
        ctrl_steer = ctrl_command(ct, uni_d(lv->cte), uni_d(lv->he),
                                  PER ? car_ld<true>(crow, TC_CAR_MAX_STEERING_ANGLE) : a.car.max_steering_angle, v);
        st = ct.noise ? ctrl_steer + uni_d(ct.noise[roll.row0 + env]) : ctrl_steer;
        if (drv_ou) {  // (steer + row) + n
          const int draws = uni_i(dr.ou_draws[env]);
          drive_n = drive_ou(dr, env, uni_d(dr.ou_state[env]), draws);
          st = st + drive_n;
          if (tid == 0) {
            dr.ou_state[env] = drive_n;
            dr.ou_draws[env] = (draws + 1) & 0x7fffffff;
          }
        }
      } else if (cdtype == TC_F32) {
        v = (double)((const float*)car_control)[2 * env];
        st = (double)((const float*)car_control)[2 * env + 1];
      } else {
        v = ((const double*)car_control)[2 * env];
        st = ((const double*)car_control)[2 * env + 1];
      }
      v = d_np_clip(v, -1.0, 1.0);  // env.py:118
      // per-env steering shift: added before the clip (examples/train_td3.py:146-148)
      st = d_np_clip(PER ? st + car_ld<true>(crow, TC_CAR_STEERING_SHIFT) : st, -1.0, 1.0);
      const int man = drv_man ? uni_i(dr.maneuver[env]) : maneuver[env];
      if (CTRL) drive_m = man;
      d_car_kinematics(PER ? car_of<true>(a.car, crow) : a.car, s, v, st, have_trig);
      TSTAMP(23);
      const FatGlobal fg = {m.lp_fat, m.lp_nodes};
      trunc = d_find_local_path(m, fg, s, man, status, pinfo, tid);
      have_trig = true;
    }
  }

  TSTAMP(1);
  if (mode != MODE_RENDER) {
    // ---- write the state back + scalar info (lane 0)
    const bool have_info = !fresh && s.lp_len >= 2;
    double cte = 0, he = 0;
    if (have_info && !pinfo.valid) {  // path kept from an earlier step (truncated before it was rebuilt)
      double2 n1 = m.lp_nodes[s.lp[2]], n2 = m.lp_nodes[s.lp[3]];
      pinfo.ax = n1.x;
      pinfo.ay = n1.y;
      pinfo.bx = n2.x;
      pinfo.by = n2.y;
      pinfo.ori = d_lp_edge_ori(m, s.lp[2], s.lp[3]);
    }
    if (have_info) {  // car.py:52-53 (nodes and orientation of local_path[1] were captured while tracking)
      cte = d_distance_to_edge(pinfo.ax, pinfo.ay, pinfo.bx, pinfo.by, s.front_x, s.front_y);
      he = d_clip_angle(pinfo.ori - s.theta);
    }
    double reward = 0;
    int terminated = 0;
    if (!(flags & TC_F_WRAPPED) && !fresh) {  // env.py:93,99
      const double tw = PER ? car_ld<true>(crow, TC_CAR_TRACK_WIDTH) : a.car.track_width;
      double r = (-1 / tw) * cte + 1;
      reward = (0 > r) ? 0 : r;
      terminated = cte > (tw * 10);
    }
    const bool late = a.n_terms > 0;  // reward / terminated depend on phase B: written after it
    if (EP) ep_count<true>(ep, env, fresh, ep_len, trunc, status);  // (the time limit: before trunc / status are stored)
    if (tid == 0) {
      lv->d[0] = s.x;
      lv->d[1] = s.y;
      lv->d[2] = s.theta;
      lv->d[3] = s.velocity;
      lv->d[4] = s.steering;
      lv->d[5] = s.radius;
      lv->d[6] = s.front_x;
      lv->d[7] = s.front_y;
      lv->d[8] = s.cth;
      lv->d[9] = s.sth;
      lv->lp_len = s.lp_len;
      lv->last_maneuver = s.last_maneuver;
      lv->have_trig = have_trig ? 1 : 0;
      lv->cursor = cursor;
      lv->cte = cte;
      lv->he = he;
      lv->trunc = trunc;
      lv->status = status;
      if (roll.cte) roll.cte[roll.row0 + env] = cte;
      if (roll.heading_error) roll.heading_error[roll.row0 + env] = he;
      if (roll.truncated) roll.truncated[roll.row0 + env] = (unsigned char)trunc;
      if (roll.status) roll.status[roll.row0 + env] = status;
      if (roll.x) roll.x[roll.row0 + env] = s.x;
      if (roll.y) roll.y[roll.row0 + env] = s.y;
      if (roll.theta) roll.theta[roll.row0 + env] = s.theta;
      if (roll.velocity) roll.velocity[roll.row0 + env] = s.velocity;
      if (roll.lp_len) roll.lp_len[roll.row0 + env] = s.lp_len;
      if (CTRL && mode == MODE_STEP) {
        ctrl_store(ct, env, roll.row0 + env, ctrl_steer);
        drive_store(dr, roll.row0 + env, drive_m, drive_n);
      }
      if (EP) lv->ep_len = ep_len;
      if (bank) {
        if (fresh) lv->cam_idx = cam_row;
        if (cb.rows && mode == MODE_STEP) cb.rows[roll.row0 + env] = cam_row;
      }
      if (!late) {
        lv->reward = reward;
        lv->terminated = terminated;
        lv->needs_reset = (flags & TC_F_AUTORESET) ? (terminated || trunc) : 0;
        if (roll.reward) roll.reward[roll.row0 + env] = reward;
        if (roll.terminated) roll.terminated[roll.row0 + env] = (unsigned char)terminated;
        if (EP) ep_close(ep, env, roll.row0 + env, fresh, status, ep_len, lv->ep_ret, reward, terminated | trunc);
      }
    }
    if (tid < 8) {  // register-resident select (a runtime-indexed s.lp[tid] would live in scratch)
      int v = s.lp[0];
#pragma unroll
      for (int i = 1; i < 8; i++) v = tid == i ? s.lp[i] : v;
      lv->lp[tid] = v;
      if (roll.lp) roll.lp[(roll.row0 + env) * 8 + tid] = v;
    }

    TSTAMP(2);
    // The map window is fetched here, behind phase A, and not at the top of the step: across the scalar phase its 30
    // registers per lane were what pushed the fused kernel over 128 VGPRs (the allocator answered by spilling the node
    // half to scratch and reloading it here).  The lines are L1 / L2 resident after the first step of a launch.
    if (single && need_win) {  // (the camera stage behind this one finds the window loaded)
      cache_nodes(mc, m, 0, m.total_nodes, tid);
      cache_edges(mc, m, 0, m.total_edges, 0, tid);
    }
    // ---- phase B: lane-line distances (car.py:55-64)
    const int C = m.C;
    double dist_l = 0;  // lane l < C: distance to lane-line layer l (0 while the info is empty, car.py:47-51)
    // Without need_b neither branch runs: nobody reads this step's distances (see envg_kernel_body) -- no rollout rows for
    // them, no term that looks at dist_l -- and lv->dist / lv->ne keep an earlier step's values until the launch's last
    // step, which always comes through here, rewrites them for live_out.  (The condition sits in the two branches, not in
    // a third one in front of them: that form moved the fused kernels' VGPR counts, which the tests hold to the recorded ones.)
    if (need_b && have_info && !DBG_ON(flags, DBG_SKIP_DIST)) {
      int my_e = -1;
      const int cell = uni_i(d_grid_cell(m, s.x, s.y));  // (every lane holds the same state)
      if (cell >= 0) {
        // layer.py:43 over the cell's candidate edges (DevMap: every edge that can be the first minimum for a point of
        // the cell, all layers, ascending): one lane per candidate, two distances straight from the edge record
        const int o0 = m.cand_off[cell * C], o1 = m.cand_off[cell * C + C];
        TSTAMP(14);
        for (int l0 = 0; l0 < C; l0 += TC_AG) {
          double bd[TC_AG];
          int best[TC_AG], lo[TC_AG], hi[TC_AG];
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            bd[g] = 0;
            best[g] = -1;
            lo[g] = l0 + g < C ? m.edge_off[l0 + g] : 0x7fffffff;
            hi[g] = l0 + g < C ? m.edge_off[l0 + g + 1] : 0x7fffffff;
          }
          const int e_lo = m.edge_off[l0], e_hi = m.edge_off[l0 + TC_AG < C ? l0 + TC_AG : C];
          for (int i = o0 + tid; i < o1; i += TC_NT) {
            const int e = m.cand_idx[i];
            if (e >= e_lo && e < e_hi) {
              const double4 q = m.edge_xy[e];
              const double d = tc_fabs(d_dist(s.x, s.y, q.x, q.y) + d_dist(s.x, s.y, q.z, q.w));
#pragma unroll
              for (int g = 0; g < TC_AG; g++) {
                const bool take = e >= lo[g] && e < hi[g] && (best[g] < 0 || d < bd[g]);
                bd[g] = take ? d : bd[g];
                best[g] = take ? e - lo[g] : best[g];
              }
            }
          }
          wave_argmin_group(bd, best);
#pragma unroll
          for (int g = 0; g < TC_AG; g++)
            if (tid == l0 + g) my_e = best[g];
        }
      } else {
      for (int w = 0; w < nwin_n; w++) {
        if (!single) cache_nodes(mc, m, w * K * TC_NT, m.total_nodes, tid);
#pragma unroll
        for (int k = 0; k < K; k++) {
          const int i = (w * K + k) * TC_NT + tid;
          if (i < m.total_nodes) dn[i] = d_dist(s.x, s.y, mc.nd[k].x, mc.nd[k].y);
        }
      }
      lds_sync();
      TSTAMP(14);
      // layer.py:43 for every layer: each lane scans its edges once (ascending index) and keeps one partial per layer
      // of the current group of TC_AG layers; the group's reductions then run together (wave_argmin_group).  A layer's
      // edges are contiguous, so edge e belongs to group layer g iff edge_off[l0 + g] <= e < edge_off[l0 + g + 1].
      for (int l0 = 0; l0 < C; l0 += TC_AG) {
        double bd[TC_AG];
        int best[TC_AG], lo[TC_AG], hi[TC_AG];
#pragma unroll
        for (int g = 0; g < TC_AG; g++) {
          bd[g] = 0;
          best[g] = -1;
          lo[g] = l0 + g < C ? m.edge_off[l0 + g] : 0x7fffffff;
          hi[g] = l0 + g < C ? m.edge_off[l0 + g + 1] : 0x7fffffff;
        }
        const int e_lo = m.edge_off[l0], e_hi = m.edge_off[l0 + TC_AG < C ? l0 + TC_AG : C];
        for (int w = 0; w < nwin_e; w++) {
          const int w0 = w * K * TC_NT;
          if (w0 >= e_hi || w0 + K * TC_NT <= e_lo) continue;  // no edge of this layer group in the window
          if (!single) cache_edges(mc, m, w0, m.total_edges, 0, tid);
#pragma unroll
          for (int k = 0; k < K; k++) {
            const int e = (w * K + k) * TC_NT + tid;
            if (e >= e_lo && e < e_hi) {
              const double d = tc_fabs(dn[mc.ed[k].x] + dn[mc.ed[k].y]);
#pragma unroll
              for (int g = 0; g < TC_AG; g++) {
                const bool take = e >= lo[g] && e < hi[g] && (best[g] < 0 || d < bd[g]);
                bd[g] = take ? d : bd[g];
                best[g] = take ? e - lo[g] : best[g];
              }
            }
          }
        }
        wave_argmin_group(bd, best);
#pragma unroll
        for (int g = 0; g < TC_AG; g++)
          if (tid == l0 + g) my_e = best[g];
      }
      }
      TSTAMP(15);
      if (tid < C) {
        const int l = tid;
        if (my_e >= 0) {
          const int ge = m.edge_off[l] + my_e;
          int2 ed = m.edges_g[ge];
          double2 n0 = m.nodes[ed.x], n1 = m.nodes[ed.y];
          // layer.py:126-142 by the sign of two dot products; the literal atan2 form only for the lanes (if any) whose
          // angle is within 1e-6 rad of the pi/2 threshold
          bool certain;
          bool inb = d_within_bounds_filter(n0.x, n0.y, n1.x, n1.y, s.x, s.y, certain);
          if (!certain) inb = d_within_bounds(n0.x, n0.y, n1.x, n1.y, m.ori_fwd[ge], m.ori_rev[ge], s.x, s.y);
          if (inb) {
            dist_l = tc_fabs(d_distance_to_edge(n0.x, n0.y, n1.x, n1.y, s.x, s.y));
          } else {
            double da = d_dist(s.x, s.y, n0.x, n0.y);
            double db = d_dist(s.front_x, s.front_y, n1.x, n1.y);  // FRONT axle for n1 (car.py:64)
            dist_l = db < da ? db : da;
          }
        }
        lv->dist[l] = dist_l;
        lv->ne[l] = my_e;
        if (roll.dist) roll.dist[(roll.row0 + env) * C + l] = dist_l;
        if (roll.ne) roll.ne[(roll.row0 + env) * C + l] = my_e;
      }
      TSTAMP(16);
      lds_sync();  // dn aliases the camera's node buffer
    } else if (need_b && tid < C) {
      lv->dist[tid] = 0;
      lv->ne[tid] = -1;
      if (roll.dist) roll.dist[(roll.row0 + env) * C + tid] = 0;
      if (roll.ne) roll.ne[(roll.row0 + env) * C + tid] = -1;
    }
    if (late) {
      // a re-spawned env did not go through Wrapper.step (the reference's reset() bypasses the wrappers)
      if (!fresh) {
        d_apply_terms(a.terms, a.n_terms, my_cnt, PER ? car_ld<true>(crow, TC_CAR_TRACK_WIDTH) : a.car.track_width, tid, C,
                      cte, have_info ? s.velocity : 0.0, dist_l, reward, terminated);
        if (tid < TC_MAX_TERMS) lv->cnt[tid] = my_cnt;
      }
      if (tid == 0) {
        lv->reward = reward;
        lv->terminated = terminated;
        lv->needs_reset = (flags & TC_F_AUTORESET) ? (terminated || trunc) : 0;
        if (roll.reward) roll.reward[roll.row0 + env] = reward;
        if (roll.terminated) roll.terminated[roll.row0 + env] = (unsigned char)terminated;
        if (EP) ep_close(ep, env, roll.row0 + env, fresh, status, ep_len, lv->ep_ret, reward, terminated | trunc);
      }
    }
  }

  TSTAMP(3);
  TSTAMP_REAL(29);
  // what the camera stage needs.  car.py:159-165 takes cos(-theta), sin(-theta): tc_cos is exactly even and tc_sin
  // exactly odd (their kernels are built from x*x and x*y terms only), so the values of the front-axle update are
  // reused bit for bit.
  fp.x = s.x;
  fp.y = s.y;
  if (have_trig) {
    fp.cth = s.cth;
    fp.sth = -s.sth;
  } else {
    fp.cth = tc_cos(-s.theta);
    fp.sth = tc_sin(-s.theta);
  }
}

// Phase C, the camera (camera.py:52-110) of one frame: transform -> 4 clip passes -> project -> visibility -> draw list
// (row `seg_row` of the per-env lists).  Depends on the env's state only through `fp`, so a frame can be produced by the
// wavefront that simulated the step or by any other one later.  mc_loaded: `mc` already holds the whole map's window
// (the simulate stage of the same wavefront loaded it).
// camera.py:62 `pose = E @ car3d` of one frame: the 3x4 matrix every node of the map is transformed with.  It depends on
// the env's state only through fp (and on the env's camera): the simulate stage computes it once per (step, env) and
// hands it over in the pose row, so the 64 lanes of a frame wavefront do not each redo the two matrix products.
#define TC_POSE_ROW 16  // doubles per (step, env) pose row: the 12 entries, padded to 128 bytes
// "not written yet" in a pose row of a streamed call (a NaN no arithmetic produces: all ones); and the marker a frame
// workgroup that gave up waiting leaves in place of its draw-list length
#define TC_POSE_EMPTY 0xFFFFFFFFFFFFFFFFull
#define TC_FRAME_SKIPPED (-2)
__device__ __forceinline__ void cam_pose12(const KArgs& a, int cam_row, const FramePose& fp, double* pose) {
  // this env's camera (camera.py:23-24,48-50): shared, or row cam_row of the camera rows (its own after
  // tc_env_set_camera_per_env, its episode's of the bank after tc_env_set_camera_bank)
  double Ec[12];
  if (a.cam_E) {
#pragma unroll
    for (int i = 0; i < 12; i++) Ec[i] = a.cam_E[(size_t)cam_row * 12 + i];
  } else {
    const __attribute__((address_space(4))) double* ee = (const __attribute__((address_space(4))) double*)(unsigned long long)a.cam.E;
#pragma unroll
    for (int i = 0; i < 12; i++) Ec[i] = ee[i];
  }
  const double cth = fp.cth, sth = fp.sth;
  double R[16] = {cth, -sth, 0, 0, sth, cth, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double Tm[16] = {1, 0, 0, -fp.x, 0, 1, 0, -fp.y, 0, 0, 1, 0, 0, 0, 0, 1};
  double car3d[16];
  d_matmul<4, 4, 4>(R, Tm, car3d);
  d_matmul<3, 4, 4>(Ec, car3d, pose);  // camera.py:62
}

// The whole-frame cull of tc_cull.h at the head of the camera stage: true = this pose's draw list is empty.  Wave-uniform
// (the pose is in scalar registers); the header fields, the cells and the special nodes come through scalar loads, and
// every cell word is fetched before the first is looked at.
#ifdef TC_ABLATE
__device__ unsigned long long tc_cull_counts[2];  // frames that ran the test, frames it culled (lane 0 counts)
#endif
__device__ __forceinline__ bool cam_cull(const KArgs& a, const double* pose) {
  typedef const __attribute__((address_space(4))) double* DConst;
  typedef const __attribute__((address_space(4))) int* IConst;
  typedef const __attribute__((address_space(4))) unsigned int* UConst;
  static_assert(offsetof(TcCullHead, margin) == 32 && offsetof(TcCullHead, nx) == 48 && offsetof(TcCullHead, n_special) == 56 &&
                    offsetof(TcCullHead, special) == 64 && TC_CULL_HEAD_BYTES % 4 == 0,
                "the fields are read by offset below");
  const DConst hd = (DConst)(unsigned long long)a.cull_tab;
  const IConst hi = (IConst)(unsigned long long)a.cull_tab;
  TcCullHead h;
  h.x0 = hd[0];
  h.y0 = hd[1];
  h.inv = hd[2];
  h.cell = hd[3];
  h.margin = hd[4];
  h.nx = hi[12];
  h.ny = hi[13];
  h.n_special = hi[14];
  int cell[TC_CULL_NC];
  unsigned int word[TC_CULL_NC];
#pragma unroll
  for (int i = 0; i < TC_CULL_NC; i++) {
    double wx, wy;
    tc_cull_world(pose, a.cull.c[i], &wx, &wy);
    cell[i] = uni_i(tc_cull_cell(h, wx, wy, a.cull.r[i]));
    // (a cell index is below nx * ny, and the buffer is padded to whole words: see tc_cull_plan)
    word[i] = ((UConst)(unsigned long long)a.cull_tab)[(TC_CULL_HEAD_BYTES + (cell[i] > 0 ? cell[i] : 0)) >> 2];
  }
  bool empty = true;
#pragma unroll
  for (int i = 0; i < TC_CULL_NC; i++) {
    const int q = (int)((word[i] >> (8 * (cell[i] & 3))) & 255u);
    empty = empty && (cell[i] == TC_CULL_CELL_CLEAR || (cell[i] >= 0 && tc_cull_free(h, q, a.cull.r[i])));
  }
  if (empty) {  // guard G, only for a frame that would be culled
    const double mr = a.cull.max_range;
    for (int i = 0; i < h.n_special; i++) {
      const double z = __builtin_fma(pose[9], hd[9 + 2 * i], __builtin_fma(pose[8], hd[8 + 2 * i], pose[11]));
      empty = empty && tc_fabs(z + mr) >= TC_CULL_GUARD;
    }
  }
#ifdef TC_ABLATE
  if (threadIdx.x == 0) {
    atomicAdd(&tc_cull_counts[0], 1ull);
    if (empty) atomicAdd(&tc_cull_counts[1], 1ull);
  }
#endif
  return empty;
}

template <int K>
__device__ __forceinline__ void cam_body(const KArgs& a, unsigned char* smem, int env, int cam_row, const double* pose_in, MapCache<K>& mc,
                                         const bool mc_loaded, const int tid, const int seg_row, int& nseg_out,
                                         unsigned int& used_out, const bool store_n = true) {
  unsigned int my_layers = 0;  // layers this lane put a segment into the draw list for
  const DevMap& m = a.m;
  const int nwin_n = (m.total_nodes + TC_NT * K - 1) / (TC_NT * K), nwin_e = (m.total_edges + TC_NT * K - 1) / (TC_NT * K);
  const bool single = a.n_grp == 1 && !a.cam_nodes && a.grp_layer[0] == 0 && a.grp_layer[1] == m.C && nwin_n <= 1 && nwin_e <= 1;
  // the 12 entries are the same in every lane: kept in scalar registers through the node loop (24 VGPRs less)
  double pose[12];
#pragma unroll
  for (int i = 0; i < 12; i++) pose[i] = uni_d(pose_in[i]);
  // Whole-frame cull: a pose whose visible ground footprint keeps clear of every lane-line segment has an empty draw
  // list (tc_cull.h) -- the stage ends here with what it delivers for an empty list: length 0, no
  // layer, the length stored where it is stored otherwise, nothing written to the overflow list.
  if (a.frame_cull && cam_cull(a, pose)) {
    nseg_out = 0;
    used_out = 0;
    if (store_n && tid == 0) a.seg_n[(size_t)seg_row * a.N + env] = 0;
    return;
  }
  if (single && !mc_loaded) {
    cache_nodes(mc, m, 0, m.total_nodes, tid);
    cache_edges(mc, m, 0, m.total_edges, 0, tid);
  }
  double* Px = (double*)(smem + a.lds.off_p);
  double* Py = Px + a.cap_nodes;
  double* Pz = Py + a.cap_nodes;
  unsigned char* flg = smem + a.lds.off_flg;
  int* list = (int*)(smem + a.lds.off_list);
  int* cnt = (int*)(smem + a.lds.off_cnt);
  const DevCam& cam = a.cam;
  double Kc[9];
  if (a.cam_K) {  // (a branch, not a select of pointers: the shared camera's K then comes in scalar loads)
#pragma unroll
    for (int i = 0; i < 9; i++) Kc[i] = a.cam_K[(size_t)cam_row * 9 + i];  // (the row that came with the pose, not the env's latest)
  } else {
    const __attribute__((address_space(4))) double* kk = (const __attribute__((address_space(4))) double*)(unsigned long long)cam.K;
#pragma unroll
    for (int i = 0; i < 9; i++) Kc[i] = kk[i];  // (explicitly the kernarg segment: cannot be merged with the other branch)
  }
  // The lane-line layers of a camera group are processed together: node ids are made global (edges_g) and then
  // relative to the group, so each of the passes below is ONE loop over the group's nodes / edges instead of one
  // per layer (the layers never share nodes, so camera.py's per-layer loop and this are the same computation).
  // Small maps are a single group; larger ones are split by the host so that the node buffer (and with it the
  // number of workgroups a CU can hold) is sized by the largest group instead of the whole map.
  // counters: cnt[0..3] fix-up passes, cnt[4] projection candidates, cnt[5] draw list
  int* seg_cnt = cnt + 5;
  const size_t seg_slot = (size_t)seg_row * a.N + env;
  int* segg = a.seg_g + seg_slot * a.seg_cap * 5;  // [seg_cap][5]: layer, x0, y0, x1, y1
  int nseg = 0;  // draw-list length so far (wave-uniform)
  for (int g = 0; g < a.n_grp; g++) {
    const int l0 = a.grp_l0[g], l1 = a.grp_l1[g];
    const int gn0 = a.grp_n0[g], ge0 = a.grp_e0[g];
    const int nn = a.grp_n0[g + 1] - gn0, ne = a.grp_e0[g + 1] - ge0;
    const int nwn = (nn + TC_NT * K - 1) / (TC_NT * K), nwe = (ne + TC_NT * K - 1) / (TC_NT * K);
    const bool one = nwn <= 1 && nwe <= 1;  // the group fits the register cache: loaded once, serves every pass
    const bool reload = !one;
    if (one && !single) {
      if (a.cam_nodes) {  // (component groups: always `one`, tc_env_create sees to it)
        cache_nodes_from(mc, a.cam_nodes, gn0, gn0 + nn, tid);
        cache_edges_from(mc, a.cam_edges_g, ge0, ge0 + ne, gn0, tid);
      } else {
        cache_nodes(mc, m, gn0, gn0 + nn, tid);
        cache_edges(mc, m, ge0, ge0 + ne, gn0, tid);
      }
    }
    if (one) {
      cam_group_regs<K>(a, mc, pose, Kc, l0, l1, ge0, nn, ne, Px, Py, Pz, flg, list, segg, (LdsIntPtr)(smem + a.seg_lds_off), nseg,
                        my_layers, env, tid);
      continue;
    }
    // a group larger than the register window: window by window, lists and counters in LDS.  No bundled map gets here;
    // tests/test_gpu_big_map_fuzz.py does with k13_by_edges (two edge windows over one node window), k13_9_layers_2970
    // (four node windows) and TC_GROUPS=0 on layers_cap_576; tests/test_gpu_parity.py with knuffingen three times over
    if (tid < 5) cnt[tid] = 0;
    if (tid == 5) cnt[5] = nseg;
    for (int w = 0; w < nwn; w++) {  // camera.py:124-131
      if (reload) cache_nodes(mc, m, gn0 + w * K * TC_NT, gn0 + nn, tid);
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int i = (w * K + k) * TC_NT + tid;
        if (i < nn) {
          double h[4] = {mc.nd[k].x, mc.nd[k].y, 0.0, 1.0};
          double p[3];
          d_matmul<3, 4, 1>(pose, h, p);
          Px[i] = p[0];
          Py[i] = p[1];
          Pz[i] = p[2];
          flg[i] = p[2] < 0 ? 1 : 0;  // camera.py:70
        }
      }
    }
    __syncthreads();
    TSTAMP(4);
    // camera.py:71-74, 75-77 (plane z = -1e-7, flag idx_front), then 81-83, 84-86 (plane z = -max_range, flag
    // idx_in_range): ONE inlined copy of the pass, looped -- four copies were ~4 k instructions of the kernel
#pragma nounroll
    for (int pass = 0; pass < 4 && !DBG_ON(a.dbg, DBG_SKIP_CLIP); pass++) {
      if (pass == 2) {
        for (int i = tid; i < nn; i += TC_NT)
          if (Pz[i] > -cam.max_range) flg[i] |= 2;  // camera.py:80, on the mutated depths
        __syncthreads();
      }
      cam_fixup_pass(mc, m, reload, ge0, ne, gn0, nwe, Px, Py, Pz, flg, pass < 2 ? 1 : 2, (pass & 1) == 0,
                     pass < 2 ? -0.0000001 : -cam.max_range, list, cnt + pass, tid);
      if (pass < 3) TSTAMP(17 + pass);
    }
    TSTAMP(5);
    // Only nodes in front AND in range can be "visible" (camera.py:92-93), and an edge is drawn when one of its ends is
    // (camera.py:95) -- with the pixel coordinates of BOTH ends.  So the nodes worth projecting (two f64 divisions each)
    // are the ends of edges that have an end in front and in range: mark them, compact them, project them in one
    // lane-parallel pass.  (Projecting the far ends inside the draw-list loop instead made the whole wavefront run the
    // projection code in every edge slot in which a single lane needed it.)
    for (int w = 0; w < nwe; w++) {
      if (reload) cache_edges(mc, m, ge0 + w * K * TC_NT, ge0 + ne, gn0, tid);
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int e = (w * K + k) * TC_NT + tid;
        if (e < ne) {
          const int2 ed = mc.ed[k];
          const int fa = flg[ed.x], fb = flg[ed.y];
          if ((fa & 3) == 3 || (fb & 3) == 3) {  // (lanes sharing a node write the same value: nothing else changes here)
            flg[ed.x] = (unsigned char)(fa | 16);
            flg[ed.y] = (unsigned char)(fb | 16);
          }
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < nn; i += TC_NT)
      if (flg[i] & 16) list[atomicAdd(cnt + 4, 1)] = i;
    __syncthreads();
    const int ncand = cnt[4];
    for (int k = tid; k < ncand; k += TC_NT) {  // camera.py:133-142, 90
      const int i = list[k];
      double u, v;
      int2 q = cam_project(Kc, Px[i], Py[i], Pz[i], u, v);
      const bool vis = (u > 0) && (u < cam.W) && (v > 0) && (v < cam.H) && (flg[i] & 3) == 3;
      ((int2*)Px)[i] = q;  // renderer.py:43,50 np.int32(...)
      if (vis) flg[i] |= 4;
    }
    __syncthreads();
    TSTAMP(6);
    for (int w = 0; w < nwe; w++) {  // camera.py:95
      if (reload) cache_edges(mc, m, ge0 + w * K * TC_NT, ge0 + ne, gn0, tid);
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int e = (w * K + k) * TC_NT + tid;
        if (e < ne) {
          const int2 ed = mc.ed[k];
          if ((flg[ed.x] | flg[ed.y]) & 4) {  // a visible end: both ends were marked above and hold pixel coordinates
            const int2 pa = ((int2*)Px)[ed.x], pb = ((int2*)Px)[ed.y];
            int layer = l0;
            for (int c = l0 + 1; c < l1; c++) layer += (ge0 + e) >= m.edge_off[c];
            my_layers |= 1u << layer;
            int j = atomicAdd(seg_cnt, 1);
            int* o = segg + 5 * j;  // j < seg_cap == total edge count
            o[0] = layer;
            o[1] = pa.x;
            o[2] = pa.y;
            o[3] = pb.x;
            o[4] = pb.y;
          }
        }
      }
    }
    __syncthreads();  // the next group reuses the node buffer and the counters
    nseg = uni_i(*seg_cnt);
    __syncthreads();
  }
  TSTAMP(7);
  nseg_out = nseg;
  // The list length goes to memory for a raster launch of its own.  When the SAME wavefront rasterises the frame it gets
  // the length in a register, and must not have this store in flight: the raster stage's first s_waitcnt vmcnt(0) (the
  // compiler guards the registers of its draw-list loads with one) would sit out the store's whole round trip behind
  // the other wavefronts' frame stores -- measured with the phase clock: 12.9 k of a frame's 83 k clocks.  Those kernels
  // store the length for tc_env_draw_list_stats after their last frame store instead.
  if (store_n && tid == 0) a.seg_n[seg_slot] = nseg_out;
  used_out = 0;
  for (int c = 0; c < m.C; c++)
    if (__ballot((my_layers >> c) & 1u)) used_out |= 1u << c;
}

// ---------------------------------------------------------------------------------------------
// Kernel 2: renderer.py:36-51 -- cv2.polylines of every segment into LDS bit-planes, then the frame is
// written to HBM once with 16-byte stores.  One wavefront per env; small argument block, small LDS.
struct RCam {
  int H, W, wpr, band_rows, n_bands, thickness, format;
  int cap_r;                  // round-cap radius of ThickLine: (thickness*32768 + 32768) >> 16
  unsigned char cap_hw[32];   // half width of the cap per |row offset| (midpoint circle of drawing.cpp)
  unsigned int cap_hw4;       // cap_hw[0..3] packed, for radii <= 3 (thickness <= 6): a scalar, where indexing the table
                              // is a vector load from the kernarg segment per cap row (three dependent ~1 us loads per frame)
};
struct RArgs {
  int N, C;
  int env0;
  RCam cam;
  unsigned char colors[16][3];
  const int* seg_g;  // [N][seg_cap][5]
  const int* seg_n;  // [N]
  int seg_cap;
  unsigned char* obs;
  const unsigned char* mask;  // reset mask (NULL = all envs)
  int off_tab, off_bits;
  unsigned int flags;
  // raster launches over several steps' frames (grid.y = frames rows): row blockIdx.y reads draw list / pose row
  // seg_row0 + blockIdx.y of the library's scratch ring, writes its frame obs_row_stride bytes behind the previous
  // row's, and is step noise_row0 + blockIdx.y of the call (position in the blob stream)
  int seg_row0;
  int noise_row0;
  long long obs_row_stride;
  // NoiseObservationWrapper fused into the raster stage (class masks only): blobs per plane (0 = off), radius bound,
  // the per-radius span table and the blob stream (position of frame row 0 = *noise_step)
  int noise_blobs, noise_max_radius;
  const unsigned char* noise_hw;
  unsigned long long noise_seed;
  const unsigned int* noise_step;
  int seg_lds_off, seg_lds_cap;  // see KArgs
  unsigned int colors_packed[16];  // colors[c] as r | g << 8 | b << 16: read with scalar loads (uniform class index)
};

#ifndef TC_RASTER_WAVES
#define TC_RASTER_WAVES 4
#endif
// LDSONLY (tc_frame_kernel): the stage reads draw-list entries from LDS only, and its common path contains no vector load
// at all.  That matters beyond the loads themselves: vector memory operations retire in issue order, and the compiler
// guards a load that MAY have been issued (the k >= seg_lds_cap branch of seg_get) with s_waitcnt vmcnt(0) at the join --
// which, executed by a wavefront that took the LDS branch, waits for nothing but the wavefront's own earlier STORES: the
// zero planes stored at the head of the stage, the previous band's pixels.  Without the branch the stores drain behind
// the raster work (cfg5: band b's 38 KB land while band b+1 is rasterised).
//   A frame whose list outgrew the LDS head (nseg_in > a.seg_lds_cap: the caller has then put the WHOLE list into the
// global array, head included) is rasterised batch by batch all the same: each batch of RB entries is first copied from
// the global list to the start of the LDS region -- loads and their wait inside a branch the common path never enters.
// Flow control of a banded frame's stores (cfg5: 19 bands of 38 KB): before a band's stores are issued, the stores of the
// band before it must have landed.  With no wait at all a wavefront runs up to 63 store instructions ahead and the chip
// as a whole writes SLOWER (cfg5, stores only: 2.81 ms per dispatch against 2.62); with the wait at the head of the band
// (where the compiler used to put one) the raster work of band b+1 cannot overlap the stores of band b (3.36 ms -> see
// DESIGN.md 6); here the raster work overlaps and at most one band is in flight.
#ifndef TC_BAND_VMCNT
#define TC_BAND_VMCNT 0
#endif
#define TC_BAND_THROTTLE() asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TC_BAND_VMCNT) : "memory")
// Bytes of one env's observation: the one place that spells them out (raster_body's `out`, the fused kernel's step stride,
// tc_env_obs_bytes).  TC_FMT_CLASSES_BITS needs W % 32 == 0 (fill_camera): a row is W / 8 bytes.
__host__ __device__ __forceinline__ size_t tc_obs_bytes_of(int fmt, int C, int H, int W) {
  return fmt == TC_FMT_CLASSES_BITS ? (size_t)C * H * (size_t)(W >> 3) : (size_t)H * W * (fmt == TC_FMT_CLASSES ? C : 3);
}
// the two class-mask formats: identical up to the store phase
#define TC_FMT_IS_CLASSES(fmt) ((fmt) == TC_FMT_CLASSES || (fmt) == TC_FMT_CLASSES_BITS)
// TC_FMT_CLASSES_BITS stores.  A packed row is the row's LDS words byte for byte (both little-endian), and rows follow each
// other without padding on both sides, so rows y0..y1 of a plane are ONE run of nw 32-bit words: lane-consecutive 16-byte
// stores when source and destination are both 16-byte aligned (wave-uniform; a frame is C*H*W/8 bytes and a plane H*W/8,
// neither need be a multiple of 16, and with odd wpr nor need the LDS plane offset), 4-byte stores otherwise.  The odd
// words behind the last whole 16 bytes go out as 4-byte stores: no byte of the run is left unwritten.
__device__ __forceinline__ void packed_zero_words(unsigned char* dst, const int nw, const int tid) {
  if ((((unsigned long long)dst) & 15ull) == 0) {
    const int n4 = nw >> 2;
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (int q = tid; q < n4; q += TC_NT) ((uint4*)dst)[q] = z;
    for (int i = (n4 << 2) + tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = 0u;
  } else {
    for (int i = tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = 0u;
  }
}
// src_word0: index of the run's first word in the bit-plane region, whose start is 16-byte aligned
__device__ __forceinline__ void packed_copy_words(unsigned char* dst, const unsigned int* src, const int src_word0, const int nw,
                                                  const int tid) {
  if ((((unsigned long long)dst) & 15ull) == 0 && (src_word0 & 3) == 0) {
    const int n4 = nw >> 2;
    for (int q = tid; q < n4; q += TC_NT) ((uint4*)dst)[q] = ((const uint4*)src)[q];
    for (int i = (n4 << 2) + tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = src[i];
  } else {
    for (int i = tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = src[i];
  }
}
template <bool THICK, int FMT, bool LDSONLY = false, int RB = RB_MAX>
__device__ __forceinline__ void raster_body(const RArgs& a0, unsigned char* smem, int env, unsigned char* obs_base,
                                            const int tid, const size_t seg_slot0, const int nseg_in,
                                            const unsigned int used_in, const int frame_row) {
  const RArgs& a = a0;
  const RCam& cam = a.cam;
  unsigned int* bits = (unsigned int*)(smem + R_OFF_BITS_OF(RB));
  const int* segg = a.seg_g + (seg_slot0 + env) * a.seg_cap * 5;
  // draw-list entry k: from LDS when the camera stage of this wavefront left it there (tc_frame_kernel), else global
  const LdsIntPtr seg_lds = (LdsIntPtr)(smem + a.seg_lds_off);
  const int seg_lds_cap = a.seg_lds_cap;
  struct SegV {
    int v[5];
    __device__ __forceinline__ int operator[](int i) const { return v[i]; }
  };
  // LDSONLY: entry k sits at LDS slot k - lds_base (lds_base = 0, or the first entry of the batch just copied in)
  int lds_base = 0;
  const bool refill = LDSONLY && nseg_in > seg_lds_cap;  // (wave-uniform)
  const int rb_step = (refill && seg_lds_cap < RB) ? seg_lds_cap : RB;  // batch size (the LDS region holds >= 8 entries: tc_env_create)
  auto seg_refill = [&](int base, int nb) {  // global entries [base, base + nb) -> LDS slots [0, nb); nb <= rb_step <= seg_lds_cap
    lds_sync();  // the batch before has been read
    for (int i = threadIdx.x; i < 5 * nb; i += TC_NT) seg_lds[i] = segg[5 * base + i];
    lds_base = base;
    lds_sync();
  };
  auto seg_get = [&](int k) {
    SegV r;
    if (LDSONLY) {
#pragma unroll
      for (int i = 0; i < 5; i++) r.v[i] = seg_lds[5 * (k - lds_base) + i];
    } else if (k < seg_lds_cap) {
#pragma unroll
      for (int i = 0; i < 5; i++) r.v[i] = seg_lds[5 * k + i];
    } else {
#pragma unroll
      for (int i = 0; i < 5; i++) r.v[i] = segg[5 * k + i];
    }
    return r;
  };
  auto seg_layer = [&](int k) { return LDSONLY ? seg_lds[5 * (k - lds_base)] : k < seg_lds_cap ? seg_lds[5 * k] : segg[5 * k]; };
  // draw-list length and the layers that have a segment in this frame (wave-uniform): handed over in registers by the
  // camera stage of the same wavefront, or read back when this is a launch of its own (nseg_in < 0)
  int nseg = nseg_in;
  unsigned int used_layers = used_in;
  TSTAMP(8);
  if (!LDSONLY && nseg_in < 0) {
    nseg = a.seg_n[seg_slot0 + env];
    used_layers = 0;
    for (int k = tid; k < nseg; k += TC_NT) used_layers |= 1u << segg[5 * k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) used_layers |= __shfl_xor(used_layers, off);
  }

  const int H = cam.H, W = cam.W, wpr = cam.wpr, C = a.C;
  constexpr bool CLS = TC_FMT_IS_CLASSES(FMT), BITS = FMT == TC_FMT_CLASSES_BITS;
  unsigned char* out = obs_base + (size_t)env * tc_obs_bytes_of(FMT, C, H, W);
  int* lt = (int*)(smem + R_OFF_TAB);     // [RB*4][5] outline-edge parameters
  int* lc = lt + RB * 4 * 5;              // [RB*4] chunks per outline edge, then exclusive prefix
  int* fl = lc + RB * 4;                  // [RB] first fill row of the segment in this band
  int* fc = fl + RB;                      // [RB] fill rows, then exclusive prefix
  int* fm = fc + RB;                      // [RB] pieces | walker mask << 8 | quad valid << 16
  int* fd = fm + RB;                      // [RB][2] ThickLine's (dp.x, dp.y)
  int* fpy = fd + 2 * RB;                 // [RB][4] fill pieces: start row
  int* fpv = fpy + 4 * RB;                // [RB][4] fill pieces: polygon vertices idx0 | idx << 2
  long long* fpx = (long long*)(fpv + 4 * RB);  // [RB][4] x at the start row (16.16)
  long long* fpd = fpx + 4 * RB;          // [RB][4] dx per row
  // Class masks, one band: the planes of layers that have no segment in this frame are all zeros (unless noise blobs are
  // going to copy into them) and are stored NOW, at the head of the stage -- their 16-byte stores drain while the used
  // planes are rasterised instead of queueing behind each other at the end of the wavefront's life (the store phase
  // is 15 % of the kernel's time for 9 % of its instructions).  A frame with no segment at all (37-57 % of the
  // benchmark's frames once cars have wandered off the road) is done here: no planes to clear, no tables, no expansion.
  unsigned int early_zero = 0;
  if (CLS && cam.n_bands == 1 && (W & 15) == 0 && a.noise_blobs == 0 && !DBG_ON(a.flags, DBG_SKIP_STORE)) {
    const int per_plane = H * (W >> 4);
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < C; c++) {
      if ((used_layers >> c) & 1u) continue;
      if (BITS) {  // the plane's H * wpr words
        packed_zero_words(out + (size_t)c * H * wpr * 4, H * wpr, tid);
        continue;
      }
      uint4* po = (uint4*)(out + (size_t)c * H * W);
      for (int q = tid; q < per_plane; q += TC_NT) po[q] = zero4;
    }
    early_zero = ~used_layers;
    if (nseg == 0) {
      TSTAMP(9);
      TSTAMP(10);
      TSTAMP(11);
      TSTAMP(12);
      TSTAMP(13);
      TSTAMP_REAL(31);
      return;
    }
  }
  for (int band = 0; band < cam.n_bands; band++) {
    const int y0 = band * cam.band_rows;
    const int y1 = (y0 + cam.band_rows < H) ? y0 + cam.band_rows : H;
    const int rows = y1 - y0;
    const int nwords = C * cam.band_rows * wpr;
    if (cam.n_bands > 1 && (W & 15) == 0) {
      // A frame taller than one LDS band (cfg5: 480 x 640 in 19 bands): most bands see no lane line at all.  Such a band
      // is all zeros whatever the format (and whatever the noise blobs copy or erase), so it is written as a plain
      // stream of 16-byte zero stores: no bit-planes to clear, nothing to scan, and no wait for the zeros to land before
      // pixel stores that never come.
      bool touched = refill;  // (a list that is not in LDS as a whole is not worth a pass of its own)
      const long long mg = (long long)cam.thickness + 2;  // ThickLine paints within thickness / 2 + 1 rows of the segment
      for (int k0 = 0; k0 < nseg && !touched; k0 += TC_NT) {
        bool t = false;
        if (k0 + tid < nseg) {
          const SegV sg = seg_get(k0 + tid);
          const long long ya = sg[2], yb = sg[4];
          t = (ya < yb ? yb : ya) + mg >= y0 && (ya < yb ? ya : yb) - mg < y1;
        }
        touched = __ballot(t) != 0;
      }
      if (!touched && DBG_ON(a.flags, DBG_SKIP_STORE)) continue;
      if (!touched) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        TC_BAND_THROTTLE();
        if (BITS) {
          for (int c = 0; c < C; c++) packed_zero_words(out + ((size_t)c * H + y0) * wpr * 4, rows * wpr, tid);
        } else if (CLS) {
          const int per_plane = rows * (W >> 4);
          for (int c = 0; c < C; c++) {
            uint4* dst = (uint4*)(out + ((size_t)c * H + y0) * W);
            for (int q = tid; q < per_plane; q += TC_NT) dst[q] = z;
          }
        } else {
          const int n16 = rows * W * 3 / 16;
          uint4* dst = (uint4*)(out + (size_t)y0 * W * 3);
          for (int q = tid; q < n16; q += TC_NT) dst[q] = z;
        }
        continue;
      }
    }
    {  // (R_OFF_BITS_OF(RB) is a multiple of 16: whole 16-byte writes, then the odd words)
      const int n4 = nwords >> 2;
      for (int i = tid; i < n4; i += TC_NT) ((uint4*)bits)[i] = make_uint4(0, 0, 0, 0);
      for (int i = (n4 << 2) + tid; i < nwords; i += TC_NT) bits[i] = 0;
    }
    lds_sync();
    TSTAMP(9);
#ifdef TC_TIMING_LDS
    TSTAMP(26);  // back to back with probe 9: what a probe costs
#endif
    Ras r;
    r.W = W;
    r.H = H;
    r.wpr = wpr;
    r.y0 = y0;
    r.y1 = y1;
    const int plane = cam.band_rows * wpr;
    if (DBG_ON(a.flags, DBG_SKIP_RASTER)) {
    } else if (!THICK) {
      for (int base = 0; base < nseg; base += refill ? rb_step : nseg) {
        const int nb = refill ? (nseg - base < rb_step ? nseg - base : rb_step) : nseg;
        if (refill) seg_refill(base, nb);
        for (int k = base + tid; k < base + nb; k += TC_NT) {
          const SegV sg = seg_get(k);
          r.bits = bits + sg[0] * plane;
          r_line_bresenham(r, sg[1], sg[2], sg[3], sg[4]);  // ThickLine with thickness <= 1 is a plain Line()
        }
      }
    } else {
      // ThickLine = FillConvexPoly(quad) [4 Line2 outline edges + scanline fill] + 2 round caps.
      // Segments are taken RB at a time; their pixel work is cut into small uniform items that are dealt
      // to the 64 lanes through prefix sums, so one long line does not serialise the wave.
      for (int base = 0; base < nseg; base += rb_step) {
        // (the loops usually run once: arguments are re-read inside them instead of being hoisted in front and held --
        // or spilled -- across the whole stage)
        const RArgs& a = kernarg_again(a0);
        const RCam& cam = a.cam;
        const int nb = nseg - base < rb_step ? nseg - base : rb_step;
        if (refill) seg_refill(base, nb);
#ifdef TC_TIMING_LDS
        if (cam.n_bands >= 0) TSTAMP(27);  // first value of the re-read argument block has arrived
#endif
        if (cam.n_bands > 1) {
          // Frames taller than one LDS band run this loop once per band (cfg5: 19 bands).  A batch none of whose
          // segments can reach the band's rows is skipped whole -- set-up, prefix sums, pixel loops: most bands of a
          // 480 x 640 frame see no lane line at all and are then a pure zero-store stream.
          bool t = false;
          if (tid < nb) {
            const SegV sg = seg_get(base + tid);
            const long long ya = sg[2], yb = sg[4], mg = (long long)cam.thickness + 2;
            t = (ya < yb ? yb : ya) + mg >= y0 && (ya < yb ? ya : yb) - mg < y1;
          }
          if (__ballot(t) == 0) continue;
        }
#ifdef TC_TIMING_LDS
        if (cam.thickness > 0) TSTAMP(24);  // (depends on a kernel argument re-read above: the scalar loads have returned)
#endif
        if (tid < RB) {  // per segment: ThickLine's dp, fill walker pieces, fill rows of this band
          int nrow = 0, lo = 0, np = 0, wm = 0, dpx = 0, dpy = 0, okq = 0;
#ifdef TC_TIMING_LDS
          TSTAMP(25);
#endif
          if (tid < nb) {
            const SegV sg = seg_get(base + tid);
            long long qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3;
            TSTAMP(20);
            // Frames taller than one LDS band are rasterised band by band, and every band runs this set-up again.  A
            // segment whose rows cannot reach the band is dropped before any of it: ThickLine paints within
            // thickness / 2 + 1 rows of the segment (quad corners p +- dp with |dp| <= thickness / 2 + 1 px, cap radius
            // (thickness + 1) / 2), and `thickness + 2` rows are allowed here.  On cfg5 (12 bands) a segment survives
            // this in 1-3 bands instead of 12.
            bool touch = true;
            if (cam.n_bands > 1) {
              const long long ya = sg[2], yb = sg[4], mg = (long long)cam.thickness + 2;
              const long long ymin = (ya < yb ? ya : yb) - mg, ymax = (ya < yb ? yb : ya) + mg;
              touch = ymax >= y0 && ymin < y1;
            }
            if (touch && !DBG_ON(a.flags, DBG_SKIP_QUAD) && r_quad_dp(sg[1], sg[2], sg[3], sg[4], cam.thickness, dpx, dpy)) {
              TSTAMP(21);
              okq = 1;
              r_quad_vertices(sg[1], sg[2], sg[3], sg[4], dpx, dpy, qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3);
              int hi = -1;
              if (!DBG_ON(a.flags, DBG_SKIP_EVENTS))
              np = r_fill_events(W, H, qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3, fpy + 4 * tid, fpv + 4 * tid, wm, lo,
                                 hi);
              TSTAMP(22);
              if (lo < y0) lo = y0;
              if (hi > y1 - 1) hi = y1 - 1;
              if (np > 0 && hi >= lo) nrow = hi - lo + 1;
            }
          }
          fl[tid] = lo;
          fc[tid] = nrow;
          fm[tid] = np | (wm << 8) | (okq << 16);
          fd[2 * tid] = dpx;
          fd[2 * tid + 1] = dpy;
        }
        lds_sync();
        TSTAMP(10);
        MARK("outline setup");
        // Outline edges: clip + DDA parameters.  Four per segment (FillConvexPoly's), or -- R_F_LONG_EDGES: thickness 2, see
        // tc_line.h -- only the two long ones v3->v0 and v1->v2, whose items then sit two per segment at the front of the
        // tables: a batch of up to 32 segments is ONE pass of this loop instead of two.  Entries past the items keep a chunk
        // count of 0 either way.  The fill pieces ride along: one per edge lane in the four-edge form, pieces i and i + 2
        // on the segment's lane i = 0, 1 in the two-edge form (the second evaluation is skipped by the whole wavefront when
        // no segment has more than two pieces).
        // (everything the two forms differ in hangs on one scalar: items per segment = 1 << sh)
        const int sh = (a.flags & R_F_LONG_EDGES) ? 1 : 2;
        for (int t = tid; t < RB * 4; t += TC_NT) {
          int nchunk = 0;
          const int j = t >> sh;
          if (t < (nb << sh) && ((fm[j] >> 16) & 1)) {
            const int s0 = t & ((1 << sh) - 1), e = s0 << (2 - sh);  // item of the segment; its edge: 0 2, or 0 1 2 3
            const SegV sg = seg_get(base + j);
            // the quad travels as (pixel end points, dp): the fill pieces and the outline edge each form the vertices
            // they need from the int32 parts (r_fill_slope, r_outline_edge)
            const int dpx = fd[2 * j], dpy = fd[2 * j + 1];
            const int np = fm[j] & 0xff;
            // fill pieces of this lane (x at the start row and slope): piece s0, and s0 + 2 in the two-edge form -- one
            // instance of the code, a loop the wavefront leaves together
#pragma nounroll
            for (int h = 0; h < (8 >> sh) && !DBG_ON(a.flags, DBG_SKIP_SLOPE); h += 2) {
              const bool want = s0 + h < np;
              if (h != 0 && __ballot(want) == 0) break;
              if (want) {
                const int s = 4 * j + s0 + h;
                long long xs, dxs;
                r_fill_slope(sg[1], sg[2], sg[3], sg[4], dpx, dpy, fpy[s], fpv[s], xs, dxs);
                fpx[s] = xs;
                fpd[s] = dxs;
              }
            }
            LineP L;
            L.ecount = -1;
            if (!DBG_ON(a.flags, DBG_SKIP_LINESETUP)) L = r_outline_edge(W, H, sg[1], sg[2], sg[3], sg[4], dpx, dpy, e);
            if (L.ecount >= 0) {
              r.bits = bits + sg[0] * plane;
              r_put(r, L.ex, L.ey);
              int* o = lt + 5 * t;
              o[0] = L.a;
              o[1] = L.b;
              o[2] = L.step;
              o[3] = L.ecount | (L.xmajor << 30);
              o[4] = sg[0];
              nchunk = (L.ecount + LCH) / LCH;
            }
          }
          lc[t] = nchunk;
        }
        lds_sync();
        MARK("prefix sums");
        int tot_l, tot_f;
        {  // exclusive prefix sums (RB*4 = 2 entries per lane, or 1 when RB = 16; RB entries on the low lanes)
          static_assert(RB * 4 == 2 * TC_NT || RB * 4 == TC_NT, "outline-edge chunk counts: one or two per lane");
          constexpr bool TWO = RB * 4 == 2 * TC_NT;
          int v0 = TWO ? lc[2 * tid] : lc[tid], v1 = TWO ? lc[2 * tid + 1] : 0;
          int inc = wave_incl_scan(v0 + v1, tid);
          tot_l = __builtin_amdgcn_readlane(inc, TC_NT - 1);
          int f = tid < RB ? fc[tid] : 0;
          int finc = wave_incl_scan(f, tid);
          tot_f = __builtin_amdgcn_readlane(finc, TC_NT - 1);
          if (TWO) {
            lc[2 * tid] = inc - v0 - v1;  // each lane rewrites only the entries it read
            lc[2 * tid + 1] = inc - v1;
          } else {
            lc[tid] = inc - v0;
          }
          if (tid < RB) fc[tid] = finc - f;
        }
        lds_sync();
        TSTAMP(11);
        for (int c = tid; c < tot_l && !DBG_ON(a.flags, DBG_SKIP_R2); c += TC_NT) {  // outline pixels, LCH steps per chunk
          int lo = 0, hi = RB * 4;
          while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (lc[mid] <= c) lo = mid; else hi = mid;
          }
          const int* o = lt + 5 * lo;
          const int ecount = o[3] & 0xffff, xmajor = (o[3] >> 30) & 1;
          const int k0 = (c - lc[lo]) * LCH;
          const int k1 = k0 + LCH - 1 < ecount ? k0 + LCH - 1 : ecount;
          r.bits = bits + o[4] * plane;
          r_line2_pixels(r, o[0], o[1], o[2], xmajor, k0, k1);
        }
        MARK("fill rows");
        for (int c = tid; c < tot_f && !DBG_ON(a.flags, DBG_SKIP_R3); c += TC_NT) {  // scanline fill, one row per item
          int lo = 0, hi = RB;
          while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (fc[mid] <= c) lo = mid; else hi = mid;
          }
          const int row = fl[lo] + (c - fc[lo]);
          const int mm = fm[lo];
          r.bits = bits + seg_layer(base + lo) * plane;
          r_fill_row(r, row, mm & 0xff, (mm >> 8) & 0xff, fpy + 4 * lo, fpx + 4 * lo, fpd + 4 * lo);
        }
        MARK("caps");
        for (int t = tid; t < nb * 2 && !DBG_ON(a.flags, DBG_SKIP_R4); t += TC_NT) {  // round caps (flags = 3: both ends)
          const int k = base + (t >> 1);
          const SegV sg = seg_get(k);
          r.bits = bits + sg[0] * plane;
          const int cx = (t & 1) ? sg[3] : sg[1], cy = (t & 1) ? sg[4] : sg[2];
          if (cam.n_bands > 1 && ((long long)cy + cam.cap_r < y0 || (long long)cy - cam.cap_r >= y1)) continue;  // cap outside the band
          if (cam.cap_r < 32)
            r_cap(r, cx, cy, cam.cap_r, cam.cap_hw, cam.cap_hw4);
          else
            r_circle_fill(r, cx, cy, cam.cap_r);
        }
        lds_sync();
      }
    }
    lds_sync();
    if (CLS && a.noise_blobs > 0) {
      // NoiseObservationWrapper (wrapper/observation.py:15-27) on the bit-planes, before they are expanded: the frame
      // never makes the extra round trip through HBM a pass of its own costs (71 us per step on cfg3 in round 1).
      // Every operation of the reference is per pixel -- plane c |= plane src & circle, or plane c &= ~circle, blob
      // after blob, plane after plane -- so one lane owns one (row, 32-pixel word) of ALL planes and replays the whole
      // blob sequence on it: no lane ever reads a word another lane writes, no barrier between blobs.  Plane c's word
      // lives in a register while its n_blobs are applied; planes < c are read back noised, planes > c as rasterised,
      // exactly the sequential order.  A filled cv2.circle with its centre inside the image is, row by row, the span
      // centre +- hw[radius][|row - cy|] clipped to the image (see tc_noise_kernel).
      const int nbl = a.noise_blobs, nb = C * nbl, mr = a.noise_max_radius;
      int* bp = (int*)(smem + R_OFF_TAB);                 // [nb][2] (x | y << 16), (r | mode << 12 | src << 16): the
      unsigned char* bh = (unsigned char*)(bp + 2 * nb);  // raster tables are dead here;  [nb][rows] half widths
      const bool staged = nb * 8 + nb * rows <= R_TAB_BYTES_OF(RB);
      const unsigned int nstep = *a.noise_step + (unsigned int)frame_row;
      for (int k = tid; k < nb; k += TC_NT) {
        const tc_blob bl = tc_noise_blob(a.noise_seed, (uint32_t)env, nstep, (uint32_t)k, W, H, mr, C);
        bp[2 * k] = bl.x | (bl.y << 16);
        bp[2 * k + 1] = bl.r | (bl.mode << 12) | (bl.src << 16);
      }
      lds_sync();
      if (staged) {  // half width of every (blob, row of this band): one table byte each, fetched with the loads in flight
        for (int row = tid; row < rows; row += TC_NT) {
#pragma unroll 5
          for (int k = 0; k < nb; k++) {
            const int by = bp[2 * k] >> 16, rr = bp[2 * k + 1] & 0xfff;
            int t = y0 + row - by;
            t = t < 0 ? -t : t;
            bh[k * rows + row] = t <= rr ? a.noise_hw[rr * mr + t] : (unsigned char)0;
          }
        }
        lds_sync();
      }
      const int items = rows * wpr;
      for (int it = tid; it < items; it += TC_NT) {
        const int row = it / wpr, w = it - row * wpr;
        const int yy = y0 + row, x_lo = w << 5;
        for (int c = 0; c < C; c++) {
          unsigned int cur = bits[(c * cam.band_rows + row) * wpr + w];
          for (int j = 0; j < nbl; j++) {
            const int k = c * nbl + j;
            const int p0 = bp[2 * k], p1 = bp[2 * k + 1];
            const int bx = p0 & 0xffff, by = p0 >> 16, rr = p1 & 0xfff, src = p1 >> 16;
            int t = yy - by;
            t = t < 0 ? -t : t;
            if (t <= rr) {
              const int hwv = staged ? (int)bh[k * rows + row] : (int)a.noise_hw[rr * mr + t];
              int xl = bx - hwv, xr = bx + hwv;
              xl = xl < 0 ? 0 : xl;
              xr = xr > W - 1 ? W - 1 : xr;
              const int b0 = xl > x_lo ? xl - x_lo : 0, b1 = xr < x_lo + 31 ? xr - x_lo : 31;
              if (b1 >= b0) {
                const unsigned int mask = (0xffffffffu >> (31 - b1)) & (0xffffffffu << b0);
                if ((p1 >> 12) & 1) {  // observation.py:22-24
                  const unsigned int sw = src == c ? cur : bits[(src * cam.band_rows + row) * wpr + w];
                  cur |= sw & mask;
                } else {
                  cur &= ~mask;  // observation.py:26
                }
              }
            }
          }
          bits[(c * cam.band_rows + row) * wpr + w] = cur;
        }
      }
      lds_sync();
      used_layers = C >= 32 ? 0xffffffffu : ((1u << C) - 1u);  // a copy may have filled a plane that had no segment
    }
    TSTAMP(12);
    const RArgs& a = kernarg_again(a0);
    const RCam& cam = a.cam;
    if (cam.n_bands > 1) TC_BAND_THROTTLE();
    if (DBG_ON(a.flags, DBG_SKIP_STORE)) {
    } else if (BITS) {
      // packed class masks: the store phase is a copy of the band's rows, plane by plane (planes of layers without a
      // segment: zeros, unless they went out at the head of the stage)
      for (int c = 0; c < C; c++) {
        if ((early_zero >> c) & 1u) continue;
        unsigned char* po = out + ((size_t)c * H + y0) * wpr * 4;
        const int w0 = c * cam.band_rows * wpr;
        if ((used_layers >> c) & 1u)
          packed_copy_words(po, bits + w0, w0, rows * wpr, tid);
        else
          packed_zero_words(po, rows * wpr, tid);
      }
    } else if (CLS) {
      if ((W & 15) == 0) {
        // 16 pixels -> one 16-byte store per lane, consecutive lanes on consecutive addresses
        // (two 16-byte stores per lane at a 32-byte lane stride were tried: 2x slower, half-line writes)
        const int g = W >> 4;  // 16-pixel groups per row
        const int per_plane = rows * g;
        const bool dense = (W & 31) == 0;  // then 16-bit half h of plane word q>>1 is group q
        const uint4 zero4 = make_uint4(0, 0, 0, 0);
        for (int c = 0; c < C; c++) {
          const unsigned int* pl = bits + c * cam.band_rows * wpr;
          unsigned char* po = out + ((size_t)c * H + y0) * W;
          if ((early_zero >> c) & 1u) continue;  // stored as zeros at the head of the stage
          if (!((used_layers >> c) & 1u)) {  // no segment of this layer in the frame: the plane is all zeros
            for (int q = tid; q < per_plane; q += TC_NT) *(uint4*)(po + (size_t)q * 16) = zero4;
            continue;
          }
          if (dense) {
            // four groups per lane and round: the four plane words are fetched together, so the wavefront waits for the
            // LDS once per round instead of once per store (the phase is a chain of read -> expand -> store; measured
            // with the stores switched off it is 15 % of the kernel's time for 9 % of its instructions)
            for (int q0 = tid; q0 < per_plane; q0 += 4 * TC_NT) {
              unsigned int w4[4];
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int q = q0 + j * TC_NT;
                w4[j] = q < per_plane ? pl[q >> 1] : 0u;
              }
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int q = q0 + j * TC_NT;
                const unsigned int b16 = (w4[j] >> ((q & 1) << 4)) & 0xffffu;
                uint4 o = zero4;
                if (__ballot(b16 != 0)) {  // wave-uniform: skip the bit spreading when all 64 groups are empty
                  o.x = spread4(b16 & 15u);
                  o.y = spread4((b16 >> 4) & 15u);
                  o.z = spread4((b16 >> 8) & 15u);
                  o.w = spread4(b16 >> 12);
                }
                if (q < per_plane) *(uint4*)(po + (size_t)q * 16) = o;  // rows of a plane are contiguous: group q sits at byte 16 q
              }
            }
            continue;
          }
          for (int q = tid; q < per_plane; q += TC_NT) {
            const int yy = q / g;
            const int xx = (q - yy * g) << 4;
            const unsigned int b16 = (pl[yy * wpr + (xx >> 5)] >> (xx & 31)) & 0xffffu;
            uint4 o = zero4;
            if (__ballot(b16 != 0)) {
              o.x = spread4(b16 & 15u);
              o.y = spread4((b16 >> 4) & 15u);
              o.z = spread4((b16 >> 8) & 15u);
              o.w = spread4(b16 >> 12);
            }
            *(uint4*)(po + (size_t)q * 16) = o;
          }
        }
      } else {
        const int per_plane = rows * W;
        const int total = C * per_plane;
        for (int q = tid; q < total; q += TC_NT) {
          int c = q / per_plane, p = q - c * per_plane;
          int yy = p / W, xx = p - yy * W;
          unsigned int word = bits[(c * cam.band_rows + yy) * wpr + (xx >> 5)];
          out[((size_t)c * H + y0 + yy) * W + xx] = ((word >> (xx & 31)) & 1u) ? 255 : 0;
        }
      }
    } else {
      // rgb: painter's order (renderer.py:41-43): the highest layer covering a pixel wins
      if ((W & 15) == 0) {
        // this band's rows as zeros first, then only the pixels that have a bit set in some plane.  The byte stores
        // follow the zero stores of the same wavefront to the same addresses in program order, and the memory system
        // keeps stores of one wavefront to one address in that order (the compiler relies on the same guarantee: it
        // never waits between two stores that may alias) -- no wait for the zeros to land: that wait was a full store
        // round trip per band, the largest single item of a touched band (cfg5 ablation, profiles/r03).
        // (Zeroing the whole frame before the first band was measured: 16 % slower)
        {
          const int n16 = rows * W * 3 / 16;
          uint4* dst = (uint4*)(out + (size_t)y0 * W * 3);
          const uint4 z = make_uint4(0, 0, 0, 0);
          for (int q = tid; q < n16; q += TC_NT) dst[q] = z;
        }
        // Class by class, highest first; a class paints the pixels it covers that no higher class covers.  The colour of a
        // class is then ONE value for the whole wavefront, fetched with a scalar load.  (Looked up per pixel --
        // colors[top][k] with `top` differing between lanes -- it was a vector load from the kernarg segment, and vector
        // memory operations retire in order: the wavefront sat out the round trip of this band's zero stores at every
        // such load, which is why raster and store time of cfg5 added up instead of overlapping -- ablation)
        const int nw = rows * wpr;
        const int pstride = cam.band_rows * wpr;
        const __attribute__((address_space(4))) unsigned int* pk =
            (const __attribute__((address_space(4))) unsigned int*)(unsigned long long)&a.colors_packed[0];
        for (int c = C - 1; c >= 0; c--) {
          const unsigned int col = pk[c];
          const unsigned char c0 = (unsigned char)col, c1 = (unsigned char)(col >> 8), c2 = (unsigned char)(col >> 16);
          for (int q = tid; q < nw; q += TC_NT) {
            unsigned int mine = bits[c * pstride + q];
            if (mine == 0) continue;
            for (int h = c + 1; h < C; h++) mine &= ~bits[h * pstride + q];
            const int yy = q / wpr, xw = (q - yy * wpr) << 5;
            unsigned char* row = out + ((size_t)(y0 + yy) * W + xw) * 3;
            while (mine) {
              const int bpos = __ffs(mine) - 1;
              mine &= mine - 1;
              unsigned char* o = row + bpos * 3;
              o[0] = c0;
              o[1] = c1;
              o[2] = c2;
            }
          }
        }
      } else if ((W & 3) == 0) {
        const int total = rows * W / 4;
        for (int g = tid; g < total; g += TC_NT) {
          int pix = g * 4;
          int yy = pix / W, xx = pix - yy * W;
          unsigned int top4 = 0;  // per pixel: 1 + index of the highest layer set, 4 pixels in 4 bytes
          for (int c = 0; c < C; c++) {
            unsigned int word = bits[(c * cam.band_rows + yy) * wpr + (xx >> 5)];
            unsigned int m4 = spread4((word >> (xx & 31)) & 15u);  // 0xFF where the layer covers the pixel
            top4 = (top4 & ~m4) | (m4 & (0x01010101u * (unsigned)(c + 1)));
          }
          unsigned char px[12];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            int top = (int)((top4 >> (8 * k)) & 255u) - 1;
            px[3 * k] = top >= 0 ? a.colors[top][0] : 0;
            px[3 * k + 1] = top >= 0 ? a.colors[top][1] : 0;
            px[3 * k + 2] = top >= 0 ? a.colors[top][2] : 0;
          }
          unsigned int* o = (unsigned int*)(out + ((size_t)(y0 + yy) * W + xx) * 3);
          o[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((unsigned)px[3] << 24);
          o[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((unsigned)px[7] << 24);
          o[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((unsigned)px[11] << 24);
        }
      } else {
        const int total = rows * W;
        for (int p = tid; p < total; p += TC_NT) {
          int yy = p / W, xx = p - yy * W;
          int top = -1;
          for (int c = 0; c < C; c++) {
            unsigned int word = bits[(c * cam.band_rows + yy) * wpr + (xx >> 5)];
            if ((word >> (xx & 31)) & 1u) top = c;
          }
          unsigned char* o = out + ((size_t)(y0 + yy) * W + xx) * 3;
          o[0] = top >= 0 ? a.colors[top][0] : 0;
          o[1] = top >= 0 ? a.colors[top][1] : 0;
          o[2] = top >= 0 ? a.colors[top][2] : 0;
        }
      }
    }
    lds_sync();
  }
  TSTAMP(13);
  TSTAMP_REAL(31);
}

template <bool THICK, int FMT>
__global__ __launch_bounds__(TC_NT, TC_RASTER_WAVES) void tc_raster_kernel(RArgs a_unused) {
  extern __shared__ __align__(16) unsigned char smem[];
  // raster_body re-reads its arguments through kernarg_again(): it must be handed the block in the kernarg segment
  // itself, not a by-value copy the compiler is free to keep in registers or scratch
  const RArgs& a = *(const RArgs*)(const __attribute__((address_space(4))) RArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const int env = a.env0 + blockIdx.x;
  if (env >= a.N) return;
  if (a.mask && !a.mask[env]) return;
  // one workgroup per (frame row, env): with more frames than resident workgroups the dispatcher hands the next frame
  // to whichever slot frees up first, so light and heavy frames balance out across the chip
  const size_t slot0 = (size_t)(a.seg_row0 + blockIdx.y) * a.N;
  raster_body<THICK, FMT>(a, smem, env, a.obs + (size_t)blockIdx.y * a.obs_row_stride, threadIdx.x, slot0, -1, 0u, a.noise_row0 + (int)blockIdx.y);
}

// ---------------------------------------------------------------------------------------------
// NoiseObservationWrapper (wrapper/observation.py:15-27) as a pass over a finished class-mask observation.
// Every operation of the reference is per pixel -- obs[c] |= obs[src] & circle, or obs[c] &= ~circle -- so rows are
// independent: the frame is taken through LDS as bit-planes band by band (same layout as the rasteriser), the blobs
// are applied to the band in order, and the band is written back.  A filled cv2.circle whose centre lies inside the
// image is, row by row, the span centre +- hw[radius][|row - cy|] clipped to the image (Circle() of drawing.cpp paints
// symmetric spans and its bounding-box tests never reject a row when the centre is inside); hw is tabulated on the
// host by running that midpoint algorithm once per radius.
struct NArgs {
  int N, C, H, W, wpr, band_rows, n_bands;
  unsigned char* obs;
  const int* blobs;  // [N][C * n_blobs][5] or NULL: drawn here (tc_rng.h)
  int n_blobs, max_radius;
  const unsigned char* hw;  // [max_radius][max_radius]: half width of row offset t of the circle of radius r
  unsigned long long seed;
  const unsigned int* step;  // device counter of noise passes so far (advanced by tc_noise_tick on the same stream:
                             // a kernel argument would be frozen into a captured HIP graph and replay the same blobs)
  unsigned int inv_cpr;  // 2^32 / (W / 16) + 1, for fdiv by the 16-pixel chunks per row
};

TC_PLAIN_KERNEL __global__ void tc_noise_tick(unsigned int* step, unsigned int n) { *step += n; }

// q / d for q < 2^31 with inv = 2^32 / d + 1 (host): one multiply-high and a fix-up instead of a ~30-instruction
// runtime division (as first written this kernel spent most of its ~12 k instructions per wavefront dividing indices)
__device__ __forceinline__ int fdiv(int q, int d, unsigned int inv) {
  int e = (int)__umulhi((unsigned int)q, inv);
  e -= (e * d > q);
  e += ((e + 1) * d <= q);
  return e;
}

// LDS: bit-planes of one band | blob rows [nb][5] | per blob the span-table row of its radius [nb][max_radius]
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_NT) void tc_noise_kernel(NArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int env = blockIdx.x, tid = threadIdx.x;
  if (env >= a.N) return;
  const int C = a.C, H = a.H, W = a.W, wpr = a.wpr;
  const int nb = C * a.n_blobs;
  unsigned int* bits = (unsigned int*)smem;
  int* lb = (int*)(smem + (size_t)C * a.band_rows * wpr * 4);
  unsigned char* lhw = (unsigned char*)(lb + nb * 5);
  unsigned char* out = a.obs + (size_t)env * ((size_t)C * H * W);

  // All blobs of this env at once, one per lane: the draws (or the caller's rows) and, behind them, each blob's row of
  // the span table, so that the blob loop touches nothing but LDS.
  for (int k = tid; k < nb; k += TC_NT) {
    tc_blob bl;
    if (a.blobs) {
      const int* p = a.blobs + ((size_t)env * nb + k) * 5;
      bl.x = p[0];
      bl.y = p[1];
      bl.r = p[2];
      bl.mode = p[3];
      bl.src = p[4];
    } else {
      bl = tc_noise_blob(a.seed, (uint32_t)env, *a.step, (uint32_t)k, W, H, a.max_radius, C);
    }
    // caller-provided lists are not trusted with LDS indices: an invalid row becomes a blob that touches nothing.
    // src only matters on the copy branch: erase blobs carry src = -1 in the reference's draw order (nothing is drawn
    // for them, observation.py:25-26) and must stay erasers.
    const bool ok = bl.r >= 1 && bl.r < a.max_radius && (unsigned)bl.x < (unsigned)W && (unsigned)bl.y < (unsigned)H &&
                    (bl.mode == 0 || (unsigned)bl.src < (unsigned)C);
    lb[5 * k] = bl.x;
    lb[5 * k + 1] = bl.y;
    lb[5 * k + 2] = ok ? bl.r : -1;
    lb[5 * k + 3] = bl.mode;
    lb[5 * k + 4] = (ok && bl.mode != 0) ? bl.src : 0;
  }
  __syncthreads();
  for (int k = 0; k < nb; k++) {  // row k of lhw = row r_k of the table, entries 0 .. r_k
    const int r = lb[5 * k + 2];
    for (int t = tid; t <= r; t += TC_NT) lhw[k * a.max_radius + t] = a.hw[r * a.max_radius + t];
  }

  // this lane's place in a pass over (row, 32-bit word) and over (row, 16-pixel chunk): fixed for the whole kernel
  const int lw = wpr <= TC_NT ? wpr : TC_NT;           // words of a row handled side by side
  const int w_lane = tid % lw, r_lane = tid / lw, r_step = TC_NT / lw;
  const bool w16 = (W & 15) == 0;                      // rows are whole 16-byte chunks: one lane per chunk, coalesced
  const int cpr = W >> 4;
  for (int band = 0; band < a.n_bands; band++) {
    const int y0 = band * a.band_rows;
    const int rows = (y0 + a.band_rows < H ? y0 + a.band_rows : H) - y0;
    if (w16) {  // bytes (0 / 255) -> bits, 16 pixels per lane
      const int per_plane = rows * cpr;
      for (int c = 0; c < C; c++) {
        const unsigned char* pl = out + ((size_t)c * H + y0) * W;  // the band's rows of a plane are contiguous
        for (int q = tid; q < per_plane; q += TC_NT) {
          const int row = fdiv(q, cpr, a.inv_cpr), ch = q - row * cpr;
          const uint4 v = *(const uint4*)(pl + (size_t)q * 16);
          const unsigned int h = ((((v.x & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) |
                                 (((((v.y & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) << 4) |
                                 (((((v.z & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) << 8) |
                                 (((((v.w & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) << 12);
          ((unsigned short*)bits)[((c * a.band_rows + row) * wpr) * 2 + ch] = (unsigned short)h;
        }
      }
    } else {
      for (int c = 0; c < C; c++)
        for (int row = r_lane; row < rows; row += r_step)
          for (int w = w_lane; w < wpr; w += lw) {
            const unsigned char* src = out + ((size_t)c * H + y0 + row) * W + w * 32;
            unsigned int word = 0;
            for (int j = 0; j < 32 && w * 32 + j < W; j++) word |= (src[j] ? 1u : 0u) << j;
            bits[(c * a.band_rows + row) * wpr + w] = word;
          }
    }
    __syncthreads();
    int c = 0, left = a.n_blobs;  // plane of blob k = k / n_blobs, kept by counting
    for (int k = 0; k < nb; k++) {  // wrapper/observation.py:16-26, blob after blob
      const int bx = lb[5 * k], by = lb[5 * k + 1], br = lb[5 * k + 2], mode = lb[5 * k + 3], bsrc = lb[5 * k + 4];
      const int ylo = by - br > y0 ? by - br : y0;
      const int yhi = br >= 1 ? (by + br < y0 + rows - 1 ? by + br : y0 + rows - 1) : ylo - 1;
      const unsigned char* hwk = lhw + k * a.max_radius;
      for (int row = ylo + r_lane; row <= yhi; row += r_step) {
        const int t = row > by ? row - by : by - row;
        const int hw = hwk[t];
        int xl = bx - hw, xr = bx + hw;
        xl = xl < 0 ? 0 : xl;
        xr = xr > W - 1 ? W - 1 : xr;
        for (int w = w_lane; w < wpr; w += lw) {
          const int b0 = xl > w * 32 ? xl - w * 32 : 0, b1 = xr < w * 32 + 31 ? xr - w * 32 : 31;
          if (b1 < b0) continue;
          const unsigned int mask = (b1 - b0 == 31) ? 0xffffffffu : (((1u << (b1 - b0 + 1)) - 1u) << b0);
          const int ic = (c * a.band_rows + row - y0) * wpr + w;
          if (mode)
            bits[ic] |= bits[(bsrc * a.band_rows + row - y0) * wpr + w] & mask;  // observation.py:22-24
          else
            bits[ic] &= ~mask;  // observation.py:26
        }
      }
      __syncthreads();  // the next blob may read what this one wrote
      if (--left == 0) {
        c++;
        left = a.n_blobs;
      }
    }
    if (w16) {  // bits -> bytes, one 16-byte store per lane
      const int per_plane = rows * cpr;
      for (int cc = 0; cc < C; cc++) {
        unsigned char* pl = out + ((size_t)cc * H + y0) * W;
        for (int q = tid; q < per_plane; q += TC_NT) {
          const int row = fdiv(q, cpr, a.inv_cpr), ch = q - row * cpr;
          const unsigned int h = ((const unsigned short*)bits)[((cc * a.band_rows + row) * wpr) * 2 + ch];
          uint4 o;
          o.x = spread4(h & 15u);
          o.y = spread4((h >> 4) & 15u);
          o.z = spread4((h >> 8) & 15u);
          o.w = spread4((h >> 12) & 15u);
          *(uint4*)(pl + (size_t)q * 16) = o;
        }
      }
    } else {
      for (int cc = 0; cc < C; cc++)
        for (int row = r_lane; row < rows; row += r_step)
          for (int w = w_lane; w < wpr; w += lw) {
            unsigned char* dst = out + ((size_t)cc * H + y0 + row) * W + w * 32;
            const unsigned int word = bits[(cc * a.band_rows + row) * wpr + w];
            for (int j = 0; j < 32 && w * 32 + j < W; j++) dst[j] = (word >> j) & 1u ? 255 : 0;
          }
    }
    __syncthreads();
  }
}

// Everything a launch is given, as ONE kernel parameter (so that it sits at offset 0 of the kernarg segment).
struct StepArgs {
  KArgs a;
  RArgs r;
  MultiArgs ma;
  int mode, cdtype;
  unsigned int flags;
  const void* car_control;
  const int* maneuver;
  const int* spawn_nodes;
  const unsigned char* mask;
  const int* env_order;  // tc_step_kernel: workgroup w works on env env_order[w] (a permutation of 0..N-1), or NULL = env w
  CarRows cr;            // per-env cars: read by the TC_FEAT_CAR kernels only (last, so every other member keeps its offset)
  EpArgs ep;             // episodes: read by the TC_FEAT_EP kernels only (behind it, for the same reason)
  CtrlArgs ct;           // built-in controller: read by the TC_FEAT_CTRL kernels only (likewise)
  CamBank cb;            // camera bank: index NULL = none (likewise behind the others)
  DriveArgs dr;          // drive randomisation: read by the TC_FEAT_CTRL kernels only, behind TC_FI_DRIVE_* of flags (likewise)
};

// The launch arguments, read through a pointer the optimiser cannot see through.  Inside the step loop of tc_step_multi
// every argument (and every address computed from one) is loop invariant; LLVM hoists all of them out of the loop and
// keeps them alive across the whole ~20 k-instruction body -- measured: 817 SGPRs spilled into VGPR lanes, which in turn
// pushed 223 VGPRs to scratch.  Re-deriving the pointer per step (an empty asm the compiler must assume changes it)
// makes each use reload its argument with a scalar load from the constant address space where it needs it, exactly as
// in a single-step kernel.
// The lane id, likewise: everything computed from it (lane predicates, LDS addresses) is loop invariant too and was
// hoisted and then spilled (-mllvm -disable-machine-licm in the Makefile does the same for the constants the instruction
// selector materialises).
__device__ __forceinline__ int step_lane() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}
typedef const __attribute__((address_space(4))) StepArgs* StepArgsConst;
__device__ __forceinline__ const StepArgs& step_args() {
  unsigned long long p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const StepArgs*)(StepArgsConst)p;
}

__device__ __forceinline__ bool wants_frame(const StepArgs& sa) {
  return !(sa.flags & (TC_F_NO_OBSERVATION | DBG_SKIP_CAMERA)) && (sa.a.b.obs != nullptr || sa.ma.roll.obs != nullptr);
}

// Simulate stage alone: the steps' state recurrence (phases A + B) with the env's state parked in LDS between steps.
// What becomes of the frames is the launch's choice: nothing (no observation), the camera stage here and a raster
// launch behind (cam_here; maps of the K = 13 variant, TC_FUSE=0), or -- the K-step default -- only the poses, from which
// tc_frame_kernel produces every (step, env) frame as a workgroup of its own.
template <int K, bool CAM, unsigned FEAT>
__device__ __forceinline__ void env_kernel_body() {
  constexpr bool EP = (FEAT & TC_FEAT_EP) != 0, CTRL = (FEAT & TC_FEAT_CTRL) != 0;
  extern __shared__ __align__(16) unsigned char smem[];
  // Touching v127 makes the kernel descriptor ask for 128 VGPRs, i.e. caps the SIMD at the 4 wavefronts the launch
  // needs (N = 4096 one-wavefront workgroups = 4 per SIMD).  The camera-less variant uses 74 registers and would fit 6,
  // and the dispatcher does fill SIMDs that unevenly: measured, wavefronts on the crowded SIMDs took 54 k clocks per
  // step against 27 k on the sparse ones, and a K-step launch lasts as long as its slowest wavefront (580 us, median
  // wavefront 420 us).  (amdgpu_waves_per_eu(4, 4) next to __launch_bounds__ did not raise the allocation.)
  asm volatile("v_mov_b32 v127, 0" ::: "v127");
  const StepArgs& s0 = step_args();
  const int env = s0.a.env0 + blockIdx.x;
  if (env >= s0.a.N) return;
  if (s0.mode == MODE_RESET && s0.mask && !s0.mask[env]) return;  // whole workgroup skips
  if (EP) ep_in(s0.a, s0.ep, smem, env);
  if (CTRL) ctrl_in(s0.a, smem, env);
  if (s0.flags & TC_FI_CAM_BANK) cam_in(s0.a, s0.cb, smem, env);
  live_in(s0.a, smem, env, s0.mode, s0.flags);
  const int nsteps = s0.ma.nsteps;
  long long t_prev = 0;
#ifdef TC_TIMING
  t_prev = clock64();
#endif
  (void)t_prev;
  // The 4 wavefronts of a SIMD compete for its vector issue slots, and at equal priority the arbiter favours the OLDEST
  // one: measured over a 30-step launch, a step took the oldest wavefront 27 k clocks and the youngest 54 k, so the
  // launch lasted 550 us while the median wavefront was done after 420.  Rotating the priority with the step index
  // (each wavefront is on top every 4th step) lets the four progress at the same average rate and finish together.
  const int wave_slot = (int)(__builtin_amdgcn_s_getreg(63492) & 15u);  // HW_REG_HW_ID.wave_id: distinct on a SIMD
  for (int k = 0; k < nsteps; k++) {
    TSTAMP_LOOP(k, nsteps, t_prev);
    switch ((k + wave_slot) & 3) {  // (s_setprio takes an immediate)
      case 0: __builtin_amdgcn_s_setprio(0); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      default: __builtin_amdgcn_s_setprio(3); break;
    }
    const StepArgs& sa = step_args();  // re-read per step: see step_args()
    const size_t esz = sa.cdtype == TC_F32 ? 4 : 8;
    const size_t row0 = (size_t)k * sa.a.N;
    const int seg_row = sa.ma.seg_rows > 1 ? k : 0;
    const int tid = step_lane();
    MapCache<K> mc = {};  // (initialised: a path that leaves it unset would otherwise make it a loop-carried value -- 30
                          // registers per lane held across the whole step body, raster stage included)
    FramePose fp;
    int cam_row;
    const bool need_b = k == nsteps - 1 || (sa.flags & TC_FI_INFO_EVERY) != 0;
    sim_body<K, FEAT>(sa.a, smem, env, sa.mode, (const char*)sa.car_control + row0 * 2 * esz, sa.cdtype, sa.maneuver + row0,
                         sa.spawn_nodes, sa.mask, sa.flags, roll_at(sa.ma.roll, row0, sa.a.m.C), tid, mc, fp, cam_row, need_b,
                         need_b || (CAM && sa.ma.cam_here), sa.cr, sa.ep, sa.ct, sa.cb, sa.dr);
    if (sa.ma.pose_rows) {
      double pose[12];
      cam_pose12(sa.a, cam_row, fp, pose);
      if (tid == 0) {
        double2* o = (double2*)(step_args().ma.pose_rows + (row0 + env) * TC_POSE_ROW);
#pragma unroll
        for (int i = 0; i < 6; i++) o[i] = make_double2(pose[2 * i], pose[2 * i + 1]);
        if (sa.flags & TC_FI_CAM_BANK) ((long long*)o)[12] = cam_row;  // (the bank index of this (step, env): see CamBank)
      }
    }
    if (CAM && sa.ma.cam_here) {
      if (wants_frame(sa)) {
        int nseg;
        unsigned int used;
        double pose[12];
        cam_pose12(sa.a, cam_row, fp, pose);
        cam_body<K>(sa.a, smem, env, cam_row, pose, mc, sa.mode != MODE_RENDER, tid, seg_row, nseg, used);  // (tc_render skips phase B's fetch)
      }
      else if (tid == 0)
        step_args().a.seg_n[(size_t)seg_row * sa.a.N + env] = 0;
    }
    lds_sync();  // the next step reads the LiveLds record this one wrote
  }
  TSTAMP_END(t_prev);
  const StepArgs& s1 = step_args();
  if (s1.mode != MODE_RENDER) {
    live_out(s1.a, smem, env);
    if (EP) ep_out(s1.a, s1.ep, smem, env);
  }
}
template <int K, bool CAM, unsigned FEAT>
__global__ __launch_bounds__(TC_NT, (K <= 5 ? TC_MIN_WAVES : K <= 9 ? 3 : 2)) void tc_env_kernel(StepArgs sa_unused) {
  env_kernel_body<K, CAM, FEAT>();
}
// the same body with the built-in controller compiled in (FEAT has TC_FEAT_CTRL: masks 4-7)
template <int K, bool CAM, unsigned FEAT>
__global__ __launch_bounds__(TC_NT, (K <= 5 ? TC_MIN_WAVES : K <= 9 ? 3 : 2)) void tc_drive_env_kernel(StepArgs sa_unused) {
  static_assert((FEAT & TC_FEAT_CTRL) != 0, "the controller's entry point");
  env_kernel_body<K, CAM, FEAT>();
}

// ---------------------------------------------------------------------------------------------
// Grouped simulate kernel for K-step calls: TC_EL lanes per env, 64 / TC_EL envs per wavefront.
// Phases A and B of a step are ~900 + ~900 wave-instructions in the one-wavefront-per-env kernel above, and A is scalar
// work that all 64 lanes repeat.  The chip is bound by vector issue (counters: the frame kernel keeps the VALUs 96 %
// busy, the per-env simulate kernel 71 %), so what a step COSTS is its instruction count.  Here an instruction of phase
// A serves 64 / TC_EL envs at once (control flow may differ between envs: plain SIMT divergence), and phase B gives each
// lane of a group every TC_EL-th edge of a layer -- two distances per edge straight from the map (L1-resident), no
// staging of node distances, an xor butterfly over the group for the argmin -- with the per-layer tail evaluated by
// every lane of the group, so nothing has to be passed around afterwards.  State lives in registers for the whole
// launch.  Per env-step: ~2 300 wave-instructions / 8 envs instead of ~1 700 / 1 env.
// The price is latency (a group of 8 lanes walks 33 edges per layer pass one after the other), which nobody waits for:
// the kernel leaves most of the chip's issue slots free for the frame kernel of the previous call.
#define TC_EL 8
#ifndef TC_ENVG_NT
#define TC_ENVG_NT 256  // threads per workgroup: 4 wavefronts = 32 envs share one LDS copy of the edge records
#endif
#ifndef TC_ENVG_PRIO
#define TC_ENVG_PRIO 3
#endif
struct GroupLds {  // per env of the wavefront: what the reward / termination terms read and count
  double dist[TC_MAX_LAYERS];
  int cnt[TC_MAX_TERMS];
};

// Where the edge records are read from matters when the kernel runs beside the frame kernel: a frame wavefront ends
// with ~20 KB of 16-byte stores, and a global load of this kernel issued on the same CU queues behind those bursts in
// the CU's vector-memory pipeline (measured: 22 us per step alone, 35 us beside the frame kernel, 23 us beside a frame
// kernel with its stores switched off).  The edge scan is ~33 loads per lane and step: from LDS it neither waits for
// the stores nor pays an L2 round trip per batch of loads.
typedef const __attribute__((address_space(3))) double* LdsDouble;
template <unsigned FEAT>
__device__ __forceinline__ void envg_kernel_body() {
  constexpr bool PER = (FEAT & TC_FEAT_CAR) != 0, EP = (FEAT & TC_FEAT_EP) != 0, CTRL = (FEAT & TC_FEAT_CTRL) != 0;
  __shared__ GroupLds glds[TC_ENVG_NT / TC_EL];
  extern __shared__ __align__(16) unsigned char gsm[];
  // Highest issue priority: when this kernel shares the chip with the frame kernel of the previous chunk it is the
  // critical path (a serial chain per step, few instructions), and the frame wavefronts would otherwise crowd it out
  // of the vector issue slots by sheer number (measured: 36 us per step beside them, 21 us alone).
  __builtin_amdgcn_s_setprio(TC_ENVG_PRIO);
  const StepArgs& s0 = step_args();
  const int lane = threadIdx.x, sub = lane & (TC_EL - 1), grp = lane / TC_EL;
  if (s0.ma.resident && lane == 0) __hip_atomic_fetch_add(s0.ma.resident, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int N = s0.a.N;
  int env = s0.a.env0 + blockIdx.x * (TC_ENVG_NT / TC_EL) + grp;
  const bool map_lds = s0.ma.map_lds != 0;
  const LdsDouble l_exy = (LdsDouble)gsm;  // [total_edges][4]: n0.x, n0.y, n1.x, n1.y
  const LdsDouble l_ofw = (LdsDouble)(gsm + (size_t)s0.a.m.total_edges * 32);
  const LdsDouble l_orv = l_ofw + s0.a.m.total_edges;
  const bool fat_lds = s0.ma.fat_lds != 0;
  const size_t fat_off = map_lds ? ((size_t)s0.a.m.total_edges * 48 + 15) / 16 * 16 : 0;
  const FatLds fl = {(const __attribute__((address_space(3))) int*)(gsm + fat_off)};
  if (fat_lds) {  // the table word by word, consecutive lanes on consecutive words (once per launch)
    const int* src = (const int*)s0.a.m.lp_fat;
    __attribute__((address_space(3))) int* dst = (__attribute__((address_space(3))) int*)(gsm + fat_off);
    const int nw = s0.a.m.lpN * (int)(sizeof(LpNode) / 4);
    for (int i = lane; i < nw; i += TC_ENVG_NT) dst[i] = src[i];
    static_assert(sizeof(LpNode) % 16 == 0, "fat node records keep 16-byte alignment in LDS");
  }
  if (map_lds) {
    const DevMap& m0 = s0.a.m;
    __attribute__((address_space(3))) double* w4 = (__attribute__((address_space(3))) double*)gsm;
    __attribute__((address_space(3))) double* wd = w4 + (size_t)m0.total_edges * 4;
    for (int i = lane; i < m0.total_edges; i += TC_ENVG_NT) {
      const double4 q = m0.edge_xy[i];
      w4[4 * i] = q.x;
      w4[4 * i + 1] = q.y;
      w4[4 * i + 2] = q.z;
      w4[4 * i + 3] = q.w;
      wd[i] = m0.ori_fwd[i];
      wd[m0.total_edges + i] = m0.ori_rev[i];
    }
  }
  if (map_lds || fat_lds) __syncthreads();
  const bool live = env < N;  // groups past the last env compute on a copy of it and store nothing
  env = live ? env : N - 1;
  GroupLds& gl = glds[grp];
  CarState s;
  int nr = 0, cursor = 0, cursor0 = 0;
  bool have_trig = false;
  {
    const tc_buffers& b = s0.a.b;
    s.x = b.x[env];
    s.y = b.y[env];
    s.theta = b.theta[env];
    s.velocity = b.velocity[env];
    s.steering = b.steering[env];
    s.radius = b.radius[env];
    s.front_x = b.front_x[env];
    s.front_y = b.front_y[env];
    s.cth = s.sth = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s.lp[i] = b.local_path[env * 8 + i];
    s.lp_len = b.lp_len[env];
    s.last_maneuver = b.last_maneuver[env];
    if (s0.flags & TC_F_AUTORESET) {
      nr = b.needs_reset[env];
      cursor = cursor0 = b.spawn_cursor[env];
    }
    if (sub < TC_MAX_TERMS) gl.cnt[sub] = (s0.a.n_terms > 0 && s0.a.term_counters) ? s0.a.term_counters[(size_t)env * TC_MAX_TERMS + sub] : 0;
    static_assert(TC_EL >= TC_MAX_TERMS, "one lane per term counter");
  }
  // the running episode (EP) waits in LDS between its two uses per step (three registers per lane across the whole step
  // took the kernel from 125 to 129 VGPRs): the length is read and rewritten by every lane of the group with the same
  // value (the time limit decides `truncated`, which all of them branch on), the return by the lane that stores the
  // env's outputs
  __shared__ int g_ep_len[EP ? TC_ENVG_NT / TC_EL : 1];
  __shared__ double g_ep_ret[EP ? TC_ENVG_NT / TC_EL : 1];
  if (EP) {
    g_ep_len[grp] = s0.ep.length[env];
    if (sub == 0) g_ep_ret[grp] = s0.ep.ret[env];
  }
  // the env's camera of the bank (tc_env_set_camera_bank), in LDS for the same reason; every lane of the group writes the
  // same value, and only lanes of this wavefront read it (LDS operations of a wavefront complete in order)
  __shared__ int g_cam_idx[TC_ENVG_NT / TC_EL];
  if (s0.flags & TC_FI_CAM_BANK) g_cam_idx[grp] = cam_clamp(s0.cb, s0.cb.index[env]);
  // drive randomisation (tc_env_set_drive_randomization): the env's maneuver, OU value and draw counter, in LDS like the
  // two above (every lane of the group computes and writes the same values) and back to the caller's arrays once per launch
  __shared__ int g_drv_man[CTRL ? TC_ENVG_NT / TC_EL : 1], g_drv_draws[CTRL ? TC_ENVG_NT / TC_EL : 1];
  __shared__ double g_drv_ou[CTRL ? TC_ENVG_NT / TC_EL : 1];
  if (CTRL && (s0.flags & TC_FI_DRIVE_MAN)) g_drv_man[grp] = s0.dr.maneuver[env];
  if (CTRL && (s0.flags & TC_FI_DRIVE_OU)) {
    g_drv_ou[grp] = s0.dr.ou_state[env];
    g_drv_draws[grp] = s0.dr.ou_draws[env];
  }
  double cte = 0, he = 0, reward = 0;
  if (CTRL) {  // what the env reported after the step before this launch: the controller's input at the first step
    cte = s0.a.b.cte[env];
    he = s0.a.b.heading_error[env];
  }
  int terminated = 0, trunc = 0, status = 0;
  const int nsteps = s0.ma.nsteps;
  // The action of step k+1 is fetched at the top of step k.  Vector-memory operations retire in issue order, so a load
  // issued at the top of a step would come back behind the rollout / pose-row stores of the step before -- each a round
  // trip through a memory pipeline the frame kernel keeps full of 16-byte stores.  Issued a whole step early, the load
  // has long returned when it is used, and the stores behind it are not waited for (raw bits are kept: converting at
  // once would be a wait).
  double2 act_d = make_double2(0.0, 0.0);
  float2 act_f = make_float2(0.f, 0.f);
  int act_m = 0;
  auto fetch_action = [&](int kk) {
    const StepArgs& sq = step_args();
    const size_t r = (size_t)kk * sq.a.N + env;
    if (CTRL) {  // the command is computed where it is applied: only the noise value (act_d.y) travels
      if (sq.ct.noise) act_d.y = sq.ct.noise[r];
    } else if (sq.cdtype == TC_F32)
      act_f = ((const float2*)sq.car_control)[r];
    else
      act_d = ((const double2*)sq.car_control)[r];
    if (!(CTRL && (sq.flags & TC_FI_DRIVE_MAN))) act_m = sq.maneuver[r];  // (device maneuvers: nothing to fetch)
  };
  fetch_action(0);
  for (int k = 0; k < nsteps; k++) {
    const StepArgs& sa = step_args();  // re-read per step: see step_args()
    const KArgs& a = sa.a;
    const DevMap& m = a.m;
    const tc_buffers& b = a.b;
    const unsigned int flags = sa.flags;
    const size_t row0 = (size_t)k * a.N;
    const RollStep roll = roll_at(sa.ma.roll, row0, a.m.C);
    status = 0;
    trunc = 0;
    // this step's action (fetched a step ago), and the next step's on its way (the last step re-reads its own row)
    const double2 cur_d = act_d;
    const float2 cur_f = act_f;
    const int cur_m = act_m;
    fetch_action(k + 1 < nsteps ? k + 1 : k);
    TSTAMP(24);
    PathInfo pinfo;
    pinfo.ax = pinfo.ay = pinfo.bx = pinfo.by = pinfo.ori = 0;
    pinfo.valid = 0;
    bool fresh = false, track = false;
    int track_man = 0;
    double ctrl_steer = 0.0;  // CTRL: this step's command before noise (0 when no action is applied)
    if ((flags & TC_F_AUTORESET) && nr) {
      const int cur = cursor;
      int node;
      if ((flags & TC_F_DEVICE_SPAWN) && a.spawn_n > 0) {
        node = a.spawn_tab[tc_spawn_index(a.spawn_seed, (uint32_t)env, (uint32_t)cur, (uint32_t)a.spawn_n)];
      } else {
        if ((unsigned)cur >= (unsigned)b.spawn_queue_len) status |= TC_S_SPAWN_WRAPPED;
        node = b.spawn_queue[(size_t)env * b.spawn_queue_len + ((unsigned)cur % (unsigned)b.spawn_queue_len)];
      }
      if (PER) car_respawn<false>(sa.cr, env, live && sub == 0);  // (one lane of the group writes the row and counter)
      if (flags & TC_FI_CAM_BANK) g_cam_idx[grp] = cam_respawn<false>(sa.cb, env, live && sub == 0);
      if (CTRL && (flags & TC_FI_DRIVE_MAN)) g_drv_man[grp] = drive_respawn_man<false>(sa.dr, env, live && sub == 0, g_drv_man[grp]);
      if (CTRL && (flags & TC_FI_DRIVE_OU) && drive_ou_reset(sa.dr)) g_drv_ou[grp] = 0.0;
      d_reset(m, PER ? car_of<false>(a.car, sa.cr.rows + (size_t)env * TC_CAR_NP) : a.car, s, checked_spawn(m, node, status));
      fresh = true;
      have_trig = true;
      cursor = cur + 1;
    } else if ((unsigned)s.lp[0] >= (unsigned)m.lpN || (unsigned)s.lp[1] >= (unsigned)m.lpN) {
      status |= TC_S_NOT_RESET;
      trunc = 1;
    } else {
      double v, st;
      const double* crow = PER ? sa.cr.rows + (size_t)env * TC_CAR_NP : nullptr;
      if (CTRL) {  // cte / he still hold what the step before left (0 / 0 behind a re-spawn)
        ctrl_steer = ctrl_command(sa.ct, cte, he, PER ? car_ld<false>(crow, TC_CAR_MAX_STEERING_ANGLE) : a.car.max_steering_angle, v);
        st = sa.ct.noise ? ctrl_steer + cur_d.y : ctrl_steer;
        if (flags & TC_FI_DRIVE_OU) {  // (steer + row) + n
          const int draws = g_drv_draws[grp];
          const double n = drive_ou(sa.dr, env, g_drv_ou[grp], draws);
          st = st + n;
          g_drv_ou[grp] = n;
          g_drv_draws[grp] = (draws + 1) & 0x7fffffff;
        }
      } else if (sa.cdtype == TC_F32) {
        v = (double)cur_f.x;
        st = (double)cur_f.y;
      } else {
        v = cur_d.x;
        st = cur_d.y;
      }
      v = d_np_clip(v, -1.0, 1.0);  // env.py:118
      st = d_np_clip(PER ? st + car_ld<false>(crow, TC_CAR_STEERING_SHIFT) : st, -1.0, 1.0);  // (train_td3.py:146-148)
      const int man = CTRL && (flags & TC_FI_DRIVE_MAN) ? g_drv_man[grp] : cur_m;
      TSTAMP(25);
      d_car_kinematics(PER ? car_of<false>(a.car, crow) : a.car, s, v, st, have_trig);
      TSTAMP(26);
      have_trig = true;
      track = true;
      track_man = man;
    }
    // ---- this step's pose row, as early as the pose is final (nothing below moves the car): in a streamed call the frame
    // workgroups of this (step, env) are waiting for it, and what follows -- lanepath tracking, distances, reward, rollout
    // rows -- is most of the step
    const bool bank = (flags & TC_FI_CAM_BANK) != 0;
    const int cam_row = bank ? g_cam_idx[grp] : (live ? env : 0);  // camera row of this step's frame (see CamBank)
    if (bank && sa.cb.rows && live && sub == 0) sa.cb.rows[row0 + env] = cam_row;
    if (sa.ma.pose_rows) {
      // car.py:159-165 takes cos(-theta), sin(-theta): tc_cos is exactly even and tc_sin exactly odd, so the values of
      // the front-axle update are reused bit for bit (as in sim_body)
      FramePose fp;
      fp.x = s.x;
      fp.y = s.y;
      fp.cth = have_trig ? s.cth : tc_cos(-s.theta);
      fp.sth = have_trig ? -s.sth : tc_sin(-s.theta);
      double pose[12];
      cam_pose12(sa.a, cam_row, fp, pose);
      if (live && sub == 0) {
        if (sa.ma.resident) {
          // streamed call: the frame workgroup of this (step, env) may already be polling the row.  Each entry is one
          // 8-byte device-scope store (sc1: written through to where every XCD sees it) and validates itself -- the
          // reader waits until none of the twelve holds TC_POSE_EMPTY any more -- so the stores need no order among
          // themselves and this wavefront waits for none of them.
          unsigned long long* o = (unsigned long long*)(sa.ma.pose_rows + (row0 + env) * TC_POSE_ROW);
#pragma unroll
          for (int i = 0; i < 12; i++)
            __hip_atomic_store(o + i, (unsigned long long)__double_as_longlong(pose[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          // with a bank, a thirteenth entry of the same kind: the index this (step, env) was posed with (never all ones)
          if (bank) __hip_atomic_store(o + 12, (unsigned long long)(unsigned int)cam_row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          double2* o = (double2*)(sa.ma.pose_rows + (row0 + env) * TC_POSE_ROW);
#pragma unroll
          for (int i = 0; i < 6; i++) o[i] = make_double2(pose[2 * i], pose[2 * i + 1]);
          if (bank) ((long long*)o)[12] = cam_row;
        }
      }
    }
    if (track) {  // car.py:127-148 (the env went through the kinematic update above)
      if (fat_lds) {
        trunc = d_find_local_path<TC_EL>(m, fl, s, track_man, status, pinfo, sub);
      } else {
        const FatGlobal fg = {m.lp_fat, m.lp_nodes};
        trunc = d_find_local_path<TC_EL>(m, fg, s, track_man, status, pinfo, sub);
      }
    }
    TSTAMP(27);
    // ---- info (car.py:46-53), default reward / termination (env.py:93,99)
    const bool have_info = !fresh && s.lp_len >= 2;
    cte = 0;
    he = 0;
    if (have_info && !pinfo.valid) {  // path kept from an earlier step (truncated before it was rebuilt)
      double2 n1 = m.lp_nodes[s.lp[2]], n2 = m.lp_nodes[s.lp[3]];
      pinfo.ax = n1.x;
      pinfo.ay = n1.y;
      pinfo.bx = n2.x;
      pinfo.by = n2.y;
      pinfo.ori = d_lp_edge_ori(m, s.lp[2], s.lp[3]);
    }
    if (have_info) {
      cte = d_distance_to_edge(pinfo.ax, pinfo.ay, pinfo.bx, pinfo.by, s.front_x, s.front_y);
      he = d_clip_angle(pinfo.ori - s.theta);
    }
    reward = 0;
    terminated = 0;
    if (!(flags & TC_F_WRAPPED) && !fresh) {
      const double tw = PER ? car_ld<false>(sa.cr.rows + (size_t)env * TC_CAR_NP, TC_CAR_TRACK_WIDTH) : a.car.track_width;
      double r = (-1 / tw) * cte + 1;
      reward = (0 > r) ? 0 : r;
      terminated = cte > (tw * 10);
    }
    // ---- phase B: nearest lane-line edge and distance per layer (car.py:55-64, layer.py:33-44,126-164)
    const int C = m.C;
    // On demand: the phase carries nothing to the next step, and what it computes leaves the launch through the rollout's
    // rows, the terms below and -- of the last step -- the env's buffers.  The plan (CallPlan::info_every) says whether any
    // step but the last has a reader; without one those steps skip the phase, the grid lookup included.  roll.dist / roll.ne
    // are NULL then (they are what sets the bit), and gl.dist keeps the values of an earlier step or launch: no term of
    // the stack reads it (that would have set the bit too).  need_b is wave-uniform: a scalar branch round the phase.
    const bool last = k == nsteps - 1;
    const bool need_b = last || (flags & TC_FI_INFO_EVERY) != 0;
    TSTAMP(0);
    static_assert(TC_EL == 8 && TC_AG <= TC_EL, "group8_argmin_multi, one lane per layer of a block");
    if (need_b) {
      const int cell = have_info ? d_grid_cell(m, s.x, s.y) : -1;
      if (have_info) {
        // The cell's candidate edges (DevMap: every edge that can be the first minimum for a point of the cell, layer by
        // layer, ascending -- a handful per layer), a block of TC_AG layers at a time.  Memory first, arithmetic after: the
        // block's list offsets are fetched together, then each lane's first candidate of every layer together (two load
        // latencies for the whole block, whatever the vector-memory pipeline's queue looks like beside the frame kernel),
        // then the layers are scanned one after the other from the LDS edge records; lane g of the group finally evaluates
        // layer g's tail, so the bounds test and the distance run once per block, not once per layer.
        //   A car outside the grid (cell < 0) runs the SAME code with the identity list -- every edge of the layer -- so a
        // wavefront with one such env executes longer loops, not a second copy of the phase.
        const bool far = cell < 0;
        for (int lb = 0; lb < C; lb += TC_AG) {
          double bd[TC_AG];
          int best[TC_AG], lo[TC_AG], off[TC_AG + 1], e0[TC_AG];
#pragma unroll
          for (int g = 0; g <= TC_AG; g++) {
            const int lg = lb + g < C ? lb + g : C;
            off[g] = far ? m.edge_off[lg] : m.cand_off[cell * C + lg];
          }
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            lo[g] = lb + g < C ? m.edge_off[lb + g] : 0;
            e0[g] = off[g] + sub < off[g + 1] ? (far ? off[g] + sub : m.cand_idx[off[g] + sub]) : -1;
          }
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            double bdg = 0;
            int bg = -1, e = e0[g];
            for (int i = off[g] + sub; i < off[g + 1]; i += TC_EL) {
              double4 q;
              if (map_lds)
                q = make_double4(l_exy[4 * e], l_exy[4 * e + 1], l_exy[4 * e + 2], l_exy[4 * e + 3]);
              else
                q = m.edge_xy[e];
              const double d = tc_fabs(d_dist(s.x, s.y, q.x, q.y) + d_dist(s.x, s.y, q.z, q.w));
              if (bg < 0 || d < bdg) {
                bg = e - lo[g];
                bdg = d;
              }
              if (i + TC_EL < off[g + 1]) e = far ? i + TC_EL : m.cand_idx[i + TC_EL];
            }
            bd[g] = bdg;
            best[g] = bg;
          }
          if (lb == 0) TSTAMP(16);
          group8_argmin_multi(bd, best);
          if (lb == 0) TSTAMP(1);
          int ne = -1, eo = 0;
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            ne = sub == g ? best[g] : ne;
            eo = sub == g ? lo[g] : eo;
          }
          const int l = lb + sub;
          if (sub < TC_AG && l < C) {  // lane g: layer lb + g
            double dist_l = 0;
            if (ne >= 0) {
              const int ge = eo + ne;
              double4 q;
              double o_fw, o_rv;
              if (map_lds) {
                q = make_double4(l_exy[4 * ge], l_exy[4 * ge + 1], l_exy[4 * ge + 2], l_exy[4 * ge + 3]);
                o_fw = l_ofw[ge];
                o_rv = l_orv[ge];
              } else {
                q = m.edge_xy[ge];
                o_fw = m.ori_fwd[ge];
                o_rv = m.ori_rev[ge];
              }
              const double2 n0 = make_double2(q.x, q.y), n1 = make_double2(q.z, q.w);
              bool certain;
              bool inb = d_within_bounds_filter(n0.x, n0.y, n1.x, n1.y, s.x, s.y, certain);
              if (!certain) inb = d_within_bounds(n0.x, n0.y, n1.x, n1.y, o_fw, o_rv, s.x, s.y);
              if (inb) {
                dist_l = tc_fabs(d_distance_to_edge(n0.x, n0.y, n1.x, n1.y, s.x, s.y));
              } else {
                const double da = d_dist(s.x, s.y, n0.x, n0.y);
                const double db = d_dist(s.front_x, s.front_y, n1.x, n1.y);  // FRONT axle for n1 (car.py:64)
                dist_l = db < da ? db : da;
              }
            }
            gl.dist[l] = dist_l;
            if (live) {
              if (roll.dist) roll.dist[(roll.row0 + env) * C + l] = dist_l;
              if (roll.ne) roll.ne[(roll.row0 + env) * C + l] = ne;
            }
            if (last && live) {
              b.laneline_distances[(size_t)env * C + l] = dist_l;
              b.nearest_edge[(size_t)env * C + l] = ne;
            }
          }
          if (lb == 0) TSTAMP(2);
        }
      } else {
        for (int l = sub; l < C; l += TC_EL) {  // no info this step (car.py:47-51): zero distances, no nearest edge
          gl.dist[l] = 0;
          if (live) {
            if (roll.dist) roll.dist[(roll.row0 + env) * C + l] = 0;
            if (roll.ne) roll.ne[(roll.row0 + env) * C + l] = -1;
          }
          if (last && live) {
            b.laneline_distances[(size_t)env * C + l] = 0;
            b.nearest_edge[(size_t)env * C + l] = -1;
          }
        }
      }
    }
    TSTAMP(14);
    // ---- reward / termination wrappers (a re-spawned env did not go through Wrapper.step)
    if (a.n_terms > 0 && !fresh)
      d_apply_terms_mem(a.terms, a.n_terms, gl.cnt,
                        PER ? car_ld<false>(sa.cr.rows + (size_t)env * TC_CAR_NP, TC_CAR_TRACK_WIDTH) : a.car.track_width, C,
                        cte, have_info ? s.velocity : 0.0, gl.dist, reward, terminated);
    int ep_len = 0;
    if (EP) {
      ep_len = g_ep_len[grp];
      ep_count<false>(sa.ep, env, fresh, ep_len, trunc, status);
      g_ep_len[grp] = ep_len;
    }
    nr = (flags & TC_F_AUTORESET) ? (terminated || trunc) : 0;
    // ---- this step's rollout rows and pose row
    if (live && sub == 0) {
      if (EP) ep_close(sa.ep, env, row0 + env, fresh, status, ep_len, g_ep_ret[grp], reward, terminated | trunc);
      if (CTRL) {
        ctrl_store(sa.ct, env, row0 + env, ctrl_steer);
        drive_store(sa.dr, row0 + env, (flags & TC_FI_DRIVE_MAN) ? g_drv_man[grp] : cur_m,
                    track && (flags & TC_FI_DRIVE_OU) ? g_drv_ou[grp] : 0.0);
      }
      if (roll.cte) roll.cte[roll.row0 + env] = cte;
      if (roll.heading_error) roll.heading_error[roll.row0 + env] = he;
      if (roll.truncated) roll.truncated[roll.row0 + env] = (unsigned char)trunc;
      if (roll.reward) roll.reward[roll.row0 + env] = reward;
      if (roll.terminated) roll.terminated[roll.row0 + env] = (unsigned char)terminated;
      if (roll.status) roll.status[roll.row0 + env] = status;
      if (roll.x) roll.x[roll.row0 + env] = s.x;
      if (roll.y) roll.y[roll.row0 + env] = s.y;
      if (roll.theta) roll.theta[roll.row0 + env] = s.theta;
      if (roll.velocity) roll.velocity[roll.row0 + env] = s.velocity;
      if (roll.lp_len) roll.lp_len[roll.row0 + env] = s.lp_len;
      if (roll.lp) {
        int4* o = (int4*)(roll.lp + (roll.row0 + env) * 8);
        o[0] = make_int4(s.lp[0], s.lp[1], s.lp[2], s.lp[3]);
        o[1] = make_int4(s.lp[4], s.lp[5], s.lp[6], s.lp[7]);
      }
    }
    TSTAMP(15);
  }
  // ---- state and the last step's outputs back to the caller's buffers
  const StepArgs& s1 = step_args();
  const tc_buffers& b = s1.a.b;
  if (live && sub == 0) {
    b.x[env] = s.x;
    b.y[env] = s.y;
    b.theta[env] = s.theta;
    b.velocity[env] = s.velocity;
    b.steering[env] = s.steering;
    b.radius[env] = s.radius;
    b.front_x[env] = s.front_x;
    b.front_y[env] = s.front_y;
#pragma unroll
    for (int i = 0; i < 8; i++) b.local_path[env * 8 + i] = s.lp[i];
    b.lp_len[env] = s.lp_len;
    b.last_maneuver[env] = s.last_maneuver;
    b.cte[env] = cte;
    b.heading_error[env] = he;
    b.reward[env] = reward;
    b.terminated[env] = (unsigned char)terminated;
    b.truncated[env] = (unsigned char)trunc;
    b.status[env] = status;
    if (b.needs_reset) b.needs_reset[env] = (unsigned char)nr;
    if (cursor != cursor0) b.spawn_cursor[env] = cursor;
    if (EP) {
      s1.ep.length[env] = g_ep_len[grp];
      s1.ep.ret[env] = g_ep_ret[grp];
    }
    if (CTRL && (s1.flags & TC_FI_DRIVE_MAN)) s1.dr.maneuver[env] = g_drv_man[grp];
    if (CTRL && (s1.flags & TC_FI_DRIVE_OU)) {
      s1.dr.ou_state[env] = g_drv_ou[grp];
      s1.dr.ou_draws[env] = g_drv_draws[grp];
    }
  }
  if (live && s1.a.term_counters && sub < s1.a.n_terms) s1.a.term_counters[(size_t)env * TC_MAX_TERMS + sub] = gl.cnt[sub];
}
// (Launch bounds: with the episode accounting 4 wavefronts per SIMD are asked for -- left to itself the allocator takes
// 129 / 131 VGPRs there, whatever the episode state is kept in; held to the 128 of the other variants it spills nothing.
// 0 = nothing asked for, as for the variants without it.)
template <unsigned FEAT>
__global__ __launch_bounds__(TC_ENVG_NT, ((FEAT & TC_FEAT_EP) ? 4 : 0)) void tc_envg_kernel(StepArgs sa_unused) {
  envg_kernel_body<FEAT>();
}
// the same body with the built-in controller compiled in (FEAT has TC_FEAT_CTRL: masks 4-7).  4 wavefronts per SIMD are
// asked for in every mask: with the drive randomisation's normal (tc_log, sqrt, tc_cos beside the whole car state in
// registers) the allocator left to itself takes 128 / 130 VGPRs in masks 4 / 5; held to 128 it spills nothing.
template <unsigned FEAT>
__global__ __launch_bounds__(TC_ENVG_NT, 4) void tc_drive_envg_kernel(StepArgs sa_unused) {
  static_assert((FEAT & TC_FEAT_CTRL) != 0, "the controller's entry point");
  envg_kernel_body<FEAT>();
}

// One (step, env) frame per workgroup: camera stage from the pose the simulate launch left, then the raster stage.
// Frames do not depend on each other, a launch has steps x N of them -- many more than the chip holds at once -- and
// their cost varies 8-fold with what is in view, so the dispatcher's hand-out of the next frame to the next free slot is
// what balances the load (a wavefront that keeps an env for the whole launch inherits that env's view instead).
struct FrameArgs {
  KArgs a;
  RArgs r;
  const double* pose_rows;  // [rows][N][TC_POSE_ROW]
  const int* order;         // workgroup x of every grid row draws env order[x] (heaviest frames first: see launch()), or NULL
  // Streamed call (launch()): this kernel runs BESIDE the simulate launch that produces its pose rows.
  int gate;                 // 0: the rows are complete (written by an earlier launch); 1: wait for the row (bounded: gate_ticks);
                            // 2: tc_frame_recover_kernel, behind the simulate launch: draws what a gate-1 workgroup gave up on
  int bank;                 // cameras in a.cam_E / a.cam_K when they are a bank (tc_env_set_camera_bank): entry 12 of a pose row
                            // then holds the frame's index into it; 0: no bank (the camera row is the env).  (Beside `gate`:
                            // the two are read together)
  int recover_rows;         // gate 2: rows of the call
  unsigned int* abort_word; // gate 1: set by the first workgroup whose wait ran out; the others then give up at once
  unsigned int* resident;   // gate 2: workgroup 0 clears this and abort_word for the next call
  long long gate_ticks;     // gate 1: how long a workgroup waits for its row, in 100 MHz ticks
  int gate_test;            // tests only: gate-1 workgroups with (row + env) % gate_test == 0 give up without waiting
};
// The argument block is read through a pointer the compiler cannot see through, once per stage: the stage's values are
// then loaded (s_load from the kernarg segment) where they are used instead of all being fetched at kernel entry and
// kept in -- or spilled from -- scalar registers across both stages.
typedef const __attribute__((address_space(4))) FrameArgs* FrameArgsConst;
__device__ __forceinline__ const FrameArgs& frame_args() {
  unsigned long long p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const FrameArgs*)(FrameArgsConst)p;
}
// The pose row of frame (slot0 + env).  In a streamed call (fa.gate) the row may not exist yet: lanes 0..11 read one entry
// each with device-scope loads (sc1: neither this CU's caches nor this XCD's L2 may answer with an older copy; the scalar
// cache is out of the question) until none holds TC_POSE_EMPTY; the values then move to scalar registers.  Rows are
// dispatched in step order and the simulate launch is resident before the frame kernel starts (tc_gate_kernel), so the
// wait ends -- but nothing relies on that: a wait that outlasts gate_ticks marks the frame skipped, tells the others and
// returns false, and tc_frame_recover_kernel, behind the simulate launch, draws the frame.  `wait` false: the row is known
// to be there (gate 2, or read before by this workgroup) -- one read.
// cam_row: the frame's row of the camera rows -- the env, or with a bank the index the simulate stage left in entry 12,
// polled and validated like the other twelve (kept inside the bank whatever the memory holds).
__device__ __forceinline__ bool frame_pose(const size_t slot0, const int env, const int row, const bool wait, double* pose, int& cam_row) {
  const FrameArgs& fa = frame_args();
  const int tid = threadIdx.x;
  const int gate = fa.gate, bank = fa.bank;
  const int np = bank ? 13 : 12;
  cam_row = env;
  if (gate) {
    unsigned long long* prow = (unsigned long long*)(fa.pose_rows + (slot0 + env) * TC_POSE_ROW);
    unsigned long long v = 0;
    bool give_up = wait && fa.gate == 1 && fa.gate_test > 0 && (row + env) % fa.gate_test == 0;
    long long t0 = 0;
    while (!give_up) {
      v = tid < np ? __hip_atomic_load(prow + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
      if (__ballot(v == TC_POSE_EMPTY) == 0 || fa.gate == 2 || !wait) break;
      const long long now = wall_clock64();
      if (t0 == 0) t0 = now;
      if (now - t0 > fa.gate_ticks || __hip_atomic_load(fa.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)
        give_up = true;
      else
        __builtin_amdgcn_s_sleep(8);
    }
    if (give_up) {
      if (tid == 0) {
        if (t0 != 0) __hip_atomic_store(fa.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (not the test's skips)
        fa.a.seg_n[slot0 + env] = TC_FRAME_SKIPPED;
      }
      return false;
    }
    const unsigned int vlo = (unsigned int)v, vhi = (unsigned int)(v >> 32);
#pragma unroll
    for (int i = 0; i < 12; i++) {
      const unsigned long long q = (unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)vlo, i) |
                                   ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)vhi, i) << 32);
      pose[i] = __longlong_as_double((long long)q);
    }
    if (bank) {
      const unsigned int idx = (unsigned int)__builtin_amdgcn_readlane((int)vlo, 12);
      cam_row = (int)(idx < (unsigned int)bank ? idx : (unsigned int)bank - 1u);
    }
  } else {
    // written by an earlier launch, complete and visible before this kernel started: one address for the whole wavefront,
    // read through the scalar cache
    const __attribute__((address_space(4))) double* pr =
        (const __attribute__((address_space(4))) double*)(unsigned long long)(fa.pose_rows + (slot0 + env) * TC_POSE_ROW);
#pragma unroll
    for (int i = 0; i < 12; i++) pose[i] = pr[i];
    if (bank) {
      const unsigned int idx = ((const __attribute__((address_space(4))) unsigned int*)(unsigned long long)pr)[24];
      cam_row = (int)(idx < (unsigned int)bank ? idx : (unsigned int)bank - 1u);
    }
  }
  return true;
}

// One frame: `rowy` is the frame's row in the launch (its step), `env` its env.
// HOT (tc_frame_kernel): the raster stage in its LDS-only form (see raster_body); !HOT (the recover kernel): the generic form.
template <int K, bool THICK, int FMT, bool HOT, int RBT>
__device__ __forceinline__ void frame_one(unsigned char* smem, const int env, const int rowy) {
  const int tid = threadIdx.x;
  int nseg;
  unsigned int used;
  {
    const FrameArgs& fa = frame_args();
    const int row = fa.r.seg_row0 + rowy;
    const size_t slot0 = (size_t)row * fa.a.N;
    double pose[12];
    int cam_row;
    if (!frame_pose(slot0, env, row, true, pose, cam_row)) return;
    MapCache<K> mc;
    TSTAMP_CLEAR();
    TSTAMP(3);
    TSTAMP_REAL(30);
    cam_body<K>(fa.a, smem, env, cam_row, pose, mc, false, tid, row, nseg, used, false);
  }
  const FrameArgs& fr = frame_args();
  const size_t slot0 = (size_t)(fr.r.seg_row0 + rowy) * fr.a.N;
  if (__builtin_expect(nseg > fr.a.seg_lds_cap, 0)) {  // (wave-uniform; cfg3: more than 56 segments)
    if (HOT) {
      // the list outgrew the LDS head: its tail is in the global array already, the head follows, and the raster stage
      // takes the whole list from there batch by batch
      lds_sync();
      const LdsIntPtr sl = (LdsIntPtr)(smem + fr.a.seg_lds_off);
      int* sg = fr.a.seg_g + (slot0 + env) * fr.a.seg_cap * 5;
      for (int i = tid; i < 5 * fr.a.seg_lds_cap; i += TC_NT) sg[i] = sl[i];
    }
    __syncthreads();  // draw-list entries that went through global memory are visible to this wavefront (vmcnt(0) + barrier)
  } else {
    lds_sync();
  }
  raster_body<THICK, FMT, HOT, RBT>(fr.r, smem, env, fr.r.obs + (size_t)rowy * fr.r.obs_row_stride, tid, slot0, nseg, used,
                                           fr.r.noise_row0 + rowy);
  {
    const FrameArgs& fe = frame_args();
    const size_t slot = (size_t)(fe.r.seg_row0 + rowy) * fe.a.N + env;
    if (tid == 0) fe.a.seg_n[slot] = nseg;  // workload statistics, the next dispatch's order, "drawn" for the recover pass
    // a streamed call's row goes back to "not written yet" for the next call (which starts behind this kernel)
    if (fe.gate && tid < (fe.bank ? 13 : 12))
      __hip_atomic_store((unsigned long long*)(fe.pose_rows + slot * TC_POSE_ROW) + tid, TC_POSE_EMPTY, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  TSTAMP_DUMP(env);
}

// K: slots of the camera stage's register cache per lane (a camera group has at most 64 K nodes / edges); RBT: segments per
// raster batch.  K = 5 with RBT = 16 is the variant of maps whose camera groups are packs of connected components (knuffingen:
// the map needs K = 9 as a whole or layer by layer, its component groups fit K = 5).
template <int K, bool THICK, int FMT, int RBT = RB_OF_K(K)>
__global__ __launch_bounds__(TC_NT, (K <= 5 ? 4 : K <= 9 ? 3 : 2)) void tc_frame_kernel(FrameArgs fa_unused) {
  extern __shared__ __align__(16) unsigned char smem[];
  const FrameArgs& fa = frame_args();
  if ((int)blockIdx.x >= fa.a.N) return;
  const int env = fa.order ? uni_i(((const __attribute__((address_space(4))) int*)(unsigned long long)fa.order)[blockIdx.x])
                           : fa.a.env0 + (int)blockIdx.x;
  frame_one<K, THICK, FMT, true, RBT>(smem, env, (int)blockIdx.y);
}

// The pass behind a streamed call's simulate launch: one workgroup per env looks through the call's rows for frames a
// gated workgroup gave up on (TC_FRAME_SKIPPED; normally none: one strided read per row block and out) and draws them
// itself, one after the other, with gate = 2 (the row is there: read once, no waiting) and the generic form of both
// stages.  Workgroup 0 resets the call's two words.
// Never on the hot path, so what the step loop around a ~10 k-instruction body costs in registers does not matter.
template <int K, bool THICK, int FMT, int RBT = RB_OF_K(K)>
__global__ __launch_bounds__(TC_NT) void tc_frame_recover_kernel(FrameArgs fa_unused) {
  extern __shared__ __align__(16) unsigned char smem[];
  const FrameArgs& fa = frame_args();
  const int env = (int)blockIdx.x, tid = threadIdx.x;
  if (env >= fa.a.N) return;
  if (fa.gate && env == 0 && tid == 0) {
    __hip_atomic_store(fa.abort_word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(fa.resident, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int rows = fa.recover_rows;
  bool any = false;  // (TC_FRAME_SKIPPED: the only negative length)
  for (int r = tid; r < rows; r += TC_NT) any |= ((const volatile int*)fa.a.seg_n)[(size_t)(fa.r.seg_row0 + r) * fa.a.N + env] < 0;
  if (__ballot(any) == 0) return;
  for (int r = 0; r < rows; r++) {
    const FrameArgs& fb = frame_args();
    if (uni_i(((const volatile int*)fb.a.seg_n)[(size_t)(fb.r.seg_row0 + r) * fb.a.N + env]) >= 0) continue;
    frame_one<K, THICK, FMT, false, RBT>(smem, env, r);
    __syncthreads();  // the next frame reuses the LDS
  }
}

// All stages in one launch: the same wavefront simulates its env, runs the camera and rasterises the frame.  The form
// of tc_step / tc_reset / tc_render (one step: nothing to balance, and one kernel boundary less), and of tc_step_multi
// under TC_MULTI_SPLIT=0.
template <int K, bool THICK, int FMT, int RBT, unsigned FEAT>
__device__ __forceinline__ void step_kernel_body() {
  constexpr bool EP = (FEAT & TC_FEAT_EP) != 0, CTRL = (FEAT & TC_FEAT_CTRL) != 0;
  extern __shared__ __align__(16) unsigned char smem[];
  const StepArgs& s0 = step_args();
  if ((int)blockIdx.x >= s0.a.N) return;
  // which env this workgroup works on: see tc_order_kernel (a scalar load: one address for the whole wavefront)
  const int env = s0.env_order ? uni_i(((const __attribute__((address_space(4))) int*)(unsigned long long)s0.env_order)[blockIdx.x])
                               : s0.a.env0 + (int)blockIdx.x;
  if (s0.mode == MODE_RESET && s0.mask && !s0.mask[env]) return;  // whole workgroup skips
  if (EP) ep_in(s0.a, s0.ep, smem, env);
  if (CTRL) ctrl_in(s0.a, smem, env);
  if (s0.flags & TC_FI_CAM_BANK) cam_in(s0.a, s0.cb, smem, env);
  live_in(s0.a, smem, env, s0.mode, s0.flags);
  const int nsteps = s0.ma.nsteps;
  long long t_prev = 0;
#ifdef TC_TIMING
  t_prev = clock64();
#endif
  (void)t_prev;
  for (int k = 0; k < nsteps; k++) {
    TSTAMP_LOOP(k, nsteps, t_prev);
    const StepArgs& sa = step_args();  // re-read per step: see step_args()
    const size_t esz = sa.cdtype == TC_F32 ? 4 : 8;
    const size_t row0 = (size_t)k * sa.a.N;
    const int tid = step_lane();
    MapCache<K> mc = {};  // (initialised: a path that leaves it unset would otherwise make it a loop-carried value -- 30
                          // registers per lane held across the whole step body, raster stage included)
    FramePose fp;
    int cam_row;  // (the bank index stays in a register: the same wavefront draws the frame)
    // (the map window is fetched every step: the camera stage below finds it loaded)
    sim_body<K, FEAT>(sa.a, smem, env, sa.mode, (const char*)sa.car_control + row0 * 2 * esz, sa.cdtype, sa.maneuver + row0,
                         sa.spawn_nodes, sa.mask, sa.flags, roll_at(sa.ma.roll, row0, sa.a.m.C), tid, mc, fp, cam_row,
                         k == nsteps - 1 || (sa.flags & TC_FI_INFO_EVERY) != 0, true, sa.cr, sa.ep, sa.ct, sa.cb, sa.dr);
    if (wants_frame(sa)) {
      int nseg;
      unsigned int used;
      double pose[12];
      cam_pose12(sa.a, cam_row, fp, pose);
      cam_body<K>(sa.a, smem, env, cam_row, pose, mc, sa.mode != MODE_RENDER, tid, 0, nseg, used, false);  // (tc_render skips phase B's fetch)
      if (nseg > sa.a.seg_lds_cap)
        __syncthreads();  // draw-list entries that went through global memory are visible to this wavefront (vmcnt(0) + barrier)
      else
        lds_sync();
      const StepArgs& sb = step_args();
      const size_t obs_step = sb.ma.roll.obs ? (size_t)sb.a.N * tc_obs_bytes_of(FMT, sb.r.C, sb.r.cam.H, sb.r.cam.W) : 0;
      unsigned char* obs_base = sb.ma.roll.obs ? sb.ma.roll.obs : sb.r.obs;
      raster_body<THICK, FMT, false, RBT>(sb.r, smem, env, obs_base + (size_t)k * obs_step, tid, 0, nseg, used, k);
      if (tid == 0) step_args().a.seg_n[env] = nseg;  // workload statistics only
    } else {
      lds_sync();  // the next step reads the LiveLds record this one wrote
    }
  }
  TSTAMP_END(t_prev);
  const StepArgs& s1 = step_args();
  if (s1.mode != MODE_RENDER) {
    live_out(s1.a, smem, env);
    if (EP) ep_out(s1.a, s1.ep, smem, env);
  }
}
template <int K, bool THICK, int FMT, int RBT, unsigned FEAT>
__global__ __launch_bounds__(TC_NT, (K <= 5 ? 4 : K <= 9 ? 3 : 2)) void tc_step_kernel(StepArgs sa_unused) {
  step_kernel_body<K, THICK, FMT, RBT, FEAT>();
}
// the same body with the built-in controller compiled in (FEAT has TC_FEAT_CTRL: masks 4-7)
template <int K, bool THICK, int FMT, int RBT, unsigned FEAT>
__global__ __launch_bounds__(TC_NT, (K <= 5 ? 4 : K <= 9 ? 3 : 2)) void tc_drive_step_kernel(StepArgs sa_unused) {
  static_assert((FEAT & TC_FEAT_CTRL) != 0, "the controller's entry point");
  step_kernel_body<K, THICK, FMT, RBT, FEAT>();
}

// ---------------------------------------------------------------------------------------------
// Which env each workgroup of a single-step launch works on.  One tc_step is N one-wavefront workgroups, exactly one
// resident round on the chip, so it lasts as long as its busiest SIMD -- and the hardware puts workgroups w, w + G,
// w + 2G, ... (G = number of SIMDs: 1024) on the SAME SIMD, whichever SIMD that is in a given launch (measured,
// tools/hw_map.py: every SIMD holds env ids that differ by exactly 1024; sum of the four wavefront lives per SIMD:
// busiest / mean = 1.4-1.6, because an env's frame costs between ~10 k and ~130 k clocks and keeps its kind of view for
// many steps).  The cost of a frame is known well enough from the frame before it (its draw-list length; the wavefront's
// measured life as the key was tried and is worse than no re-deal at all: it carries the contention of the previous deal), so the envs are
// sorted by that and dealt to the G groups in serpentine order -- heaviest with lightest -- and workgroup w takes env
// order[w].  Any permutation gives the same results (envs are independent); only the launch time changes.
// One workgroup: counting sort of the N lengths (descending), then rank r -> workgroup (r / G) * G + (r / G even ? r % G :
// G - 1 - r % G).
#define TC_ORDER_NT 1024
#define TC_ORDER_BINS 256
// (the keys are read ONCE, into LDS: the lengths may belong to a frame row another stream is about to redraw, and a key
// that changed between the counting and the placing pass would break the permutation)
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_ORDER_NT) void tc_order_kernel(const int* cost, int N, int G, int* order) {
  __shared__ int hist[TC_ORDER_BINS], cursor[TC_ORDER_BINS];
  extern __shared__ unsigned char okeys[];  // [N]
  const int t = threadIdx.x;
  for (int b = t; b < TC_ORDER_BINS; b += TC_ORDER_NT) hist[b] = 0;
  __syncthreads();
  for (int i = t; i < N; i += TC_ORDER_NT) {
    int c = cost[i];
    c = c < 0 ? 0 : (c > TC_ORDER_BINS - 1 ? TC_ORDER_BINS - 1 : c);
    okeys[i] = (unsigned char)(TC_ORDER_BINS - 1 - c);  // bin 0 = the heaviest
    atomicAdd(&hist[TC_ORDER_BINS - 1 - c], 1);
  }
  __syncthreads();
  {  // exclusive prefix sum over the bins: a DPP scan inside each of the first four wavefronts, their totals through LDS
    __shared__ int wtot[TC_ORDER_BINS / TC_NT];
    static_assert(TC_ORDER_BINS % TC_NT == 0 && TC_ORDER_BINS <= TC_ORDER_NT, "one thread per bin, whole wavefronts");
    int v = 0, inc = 0;
    if (t < TC_ORDER_BINS) {
      v = hist[t];
      inc = wave_incl_scan(v, t & (TC_NT - 1));
      if ((t & (TC_NT - 1)) == TC_NT - 1) wtot[t / TC_NT] = inc;
    }
    __syncthreads();
    if (t < TC_ORDER_BINS) {
      int base = 0;
      for (int w = 0; w < t / TC_NT; w++) base += wtot[w];
      cursor[t] = base + inc - v;
    }
  }
  __syncthreads();
  for (int i = t; i < N; i += TC_ORDER_NT) {
    const int r = atomicAdd(&cursor[okeys[i]], 1);  // rank among the envs, heaviest first
    const int row = r / G, j = r - row * G;
    order[row * G + ((row & 1) ? G - 1 - j : j)] = i;
  }
}

// Streamed call: holds the frame stream until every workgroup of the simulate launch on the caller's stream has started
// (they count themselves into *resident).  One wavefront, so it cannot keep them off the chip itself; the frame
// kernel behind it in stream order then finds its producers resident whatever it fills the chip with.  Bounded: after
// `ticks` (100 MHz) it lets the frame kernel go regardless, whose workgroups have a bound of their own.
TC_PLAIN_KERNEL __global__ __launch_bounds__(64) void tc_gate_kernel(const unsigned int* resident, unsigned int want, long long ticks) {
  const long long t0 = wall_clock64();
  while (__hip_atomic_load(resident, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want && wall_clock64() - t0 < ticks)
    __builtin_amdgcn_s_sleep(2);
}

// ---------------------------------------------------------------------------------------------
// The instantiations of parts 1-5 (see TC_PART), D = `template` where they are compiled, `extern template` in part 0.
// (K, RB) pairs: StepKRb / FrameKRb of the codes 516, 5, 8, 9.
#define TC_INST_STEP(D, KERN, C, K, RB, T, F)                         \
  D __global__ void KERN<K, T, F, RB, C>(StepArgs);                     \
  D __global__ void KERN<K, T, F, RB, (C) | TC_FEAT_CAR>(StepArgs);     \
  D __global__ void KERN<K, T, F, RB, (C) | TC_FEAT_EP>(StepArgs);      \
  D __global__ void KERN<K, T, F, RB, (C) | TC_FEAT_ALL>(StepArgs);
#define TC_INST_STEP_T(D, KERN, C, K, RB, F) TC_INST_STEP(D, KERN, C, K, RB, true, F) TC_INST_STEP(D, KERN, C, K, RB, false, F)
#define TC_INST_STEP_F(D, KERN, C, F)                                                             \
  TC_INST_STEP_T(D, KERN, C, 5, 16, F) TC_INST_STEP_T(D, KERN, C, 5, RB_OF_K(5), F)                 \
  TC_INST_STEP_T(D, KERN, C, 8, RB_OF_K(8), F) TC_INST_STEP_T(D, KERN, C, 9, RB_OF_K(9), F)
#define TC_INST_PART1(D) TC_INST_STEP_F(D, tc_drive_step_kernel, TC_FEAT_CTRL, TC_FMT_CLASSES)
#define TC_INST_PART3(D) TC_INST_STEP_F(D, tc_drive_step_kernel, TC_FEAT_CTRL, TC_FMT_RGB)
#define TC_INST_PART4(D) TC_INST_STEP_F(D, tc_step_kernel, 0u, TC_FMT_CLASSES)
#define TC_INST_PART5(D) TC_INST_STEP_F(D, tc_step_kernel, 0u, TC_FMT_RGB)
#define TC_INST_PFRAME2(D, K, RB, T)                                                        \
  D __global__ void tc_frame_kernel<K, T, TC_FMT_CLASSES_BITS, RB>(FrameArgs);                \
  D __global__ void tc_frame_recover_kernel<K, T, TC_FMT_CLASSES_BITS, RB>(FrameArgs);
#define TC_INST_PFRAME(D, K, RB) TC_INST_PFRAME2(D, K, RB, true) TC_INST_PFRAME2(D, K, RB, false)
#define TC_INST_PART2(D)                                                                                                  \
  TC_INST_PFRAME(D, 5, 16) TC_INST_PFRAME(D, 5, RB_OF_K(5)) TC_INST_PFRAME(D, 8, RB_OF_K(8)) TC_INST_PFRAME(D, 9, RB_OF_K(9)) \
  D __global__ void tc_raster_kernel<true, TC_FMT_CLASSES_BITS>(RArgs);                                                     \
  D __global__ void tc_raster_kernel<false, TC_FMT_CLASSES_BITS>(RArgs);
#define TC_INST_UNPACK(D)                                                                                                          \
  D __global__ void tc_unpack_bits_kernel<TC_U8>(const unsigned int*, long long, long long, const long long*, long long, uint4*);   \
  D __global__ void tc_unpack_bits_kernel<TC_F16>(const unsigned int*, long long, long long, const long long*, long long, uint4*);  \
  D __global__ void tc_unpack_bits_kernel<TC_BF16>(const unsigned int*, long long, long long, const long long*, long long, uint4*); \
  D __global__ void tc_unpack_bits_kernel<TC_F32>(const unsigned int*, long long, long long, const long long*, long long, uint4*);
#if defined(TC_PART) && TC_PART == 0
TC_INST_PART1(extern template)
TC_INST_PART2(extern template)
TC_INST_PART3(extern template)
TC_INST_PART4(extern template)
TC_INST_PART5(extern template)
#endif

#if !defined(TC_PART) || TC_PART == 0
// ---------------------------------------------------------------------------------------------
// From run-time choices to a kernel: lift(f, Among<T, ..>{v}, ..) calls f with one std::integral_constant per choice --
// the value of the list that v equals, the LAST of the list when it equals none -- so f can use them as template arguments.
template <class T, T V, T... Vs>
struct Among {
  T v;
};
template <class F>
static auto lift(F&& f) {
  return f();
}
template <class F, class T, T V, T... Vs, class... More>
static auto lift(F&& f, Among<T, V, Vs...> c, More... more) {
  auto with = [&](auto... rest) { return f(std::integral_constant<T, V>{}, rest...); };
  if constexpr (sizeof...(Vs) == 0)
    return lift(with, more...);
  else
    return c.v == V ? lift(with, more...) : lift(f, Among<T, Vs...>{c.v}, more...);
}

// The variants compiled, per template parameter.  Kcode names a (K, RB) pair of tc_step_kernel / tc_frame_kernel: K itself
// with the batch size that goes with it, or 516 = K 5 with batches of 16 (tc_env::kframe).
// TC_DEV_FAST (make dev): only the K = 5 / thick / classes variants are instantiated -- a compile of seconds instead of
// minutes for kernel work on cfg3 (make dev DEVK=9 DEVFMT=TC_FMT_RGB: the variants of cfg5; DEVK=9 alone: cfg4) -- and
// every request maps to them (one-element lists).  Never shipped: the default build has no such macro.
using Feats = Among<unsigned, 0u, TC_FEAT_CAR, TC_FEAT_EP, TC_FEAT_ALL>;
// the masks of the tc_drive_* entry points (the built-in controller alone, with per-env cars, with episodes, with both)
using DriveFeats = Among<unsigned, TC_FEAT_CTRL, TC_FEAT_CTRL | TC_FEAT_CAR, TC_FEAT_CTRL | TC_FEAT_EP, TC_FEAT_CTRL | TC_FEAT_ALL>;
using Bools = Among<bool, true, false>;
#ifdef TC_DEV_FAST
#ifndef TC_DEV_KV
#define TC_DEV_KV 5
#endif
#ifndef TC_DEV_FMTV
#define TC_DEV_FMTV TC_FMT_CLASSES
#endif
#ifndef TC_DEV_SK   // K / batch size of the one fused step kernel variant compiled (cfg4, cfg5: 5 and 16, like TC_DEV_FK / TC_DEV_FRB)
#define TC_DEV_SK TC_DEV_KV
#endif
#ifndef TC_DEV_SRB
#define TC_DEV_SRB RB_OF_K(TC_DEV_SK)
#endif
#ifndef TC_DEV_FK   // K / batch size of the one frame kernel variant compiled (cfg4, cfg5: DEVFK=5 DEVFRB=16)
#define TC_DEV_FK TC_DEV_KV
#endif
#ifndef TC_DEV_FRB
#define TC_DEV_FRB RB_OF_K(TC_DEV_FK)
#endif
using Kvars = Among<int, TC_DEV_KV>;
using Kcodes = Among<int, 0>;
using Thicks = Among<bool, true>;
// (the fused step kernels have no packed variant: a packed dev build compiles their byte class-mask form, which a packed env never launches)
using Fmts = Among<int, (TC_DEV_FMTV == TC_FMT_CLASSES_BITS ? TC_FMT_CLASSES : TC_DEV_FMTV)>;
using FrameFmts = Among<int, TC_DEV_FMTV>;
template <int> struct StepKRb { static constexpr int K = TC_DEV_SK, RB = TC_DEV_SRB; };
template <int> struct FrameKRb { static constexpr int K = TC_DEV_FK, RB = TC_DEV_FRB; };
#else
using Kvars = Among<int, 5, 8, 9, 13>;
using Kcodes = Among<int, 516, 5, 8, 9>;
using Thicks = Bools;
using Fmts = Among<int, TC_FMT_CLASSES, TC_FMT_RGB>;
// tc_frame_kernel, tc_frame_recover_kernel and tc_raster_kernel also exist for packed class masks (TC_FMT_CLASSES_BITS); the
// fused tc_step_kernel / tc_drive_step_kernel family -- the bulk of the build -- does not: plan_call() never sends a packed
// env there
using FrameFmts = Among<int, TC_FMT_CLASSES, TC_FMT_CLASSES_BITS, TC_FMT_RGB>;
template <int CODE> struct StepKRb { static constexpr int K = CODE == 516 ? 5 : CODE, RB = CODE == 516 ? 16 : RB_OF_K(CODE); };
template <int CODE> using FrameKRb = StepKRb<CODE>;
#endif

typedef void (*step_kern_t)(StepArgs);
typedef void (*frame_kern_t)(FrameArgs);
typedef void (*raster_kern_t)(RArgs);
// all stages in one launch
static step_kern_t step_kernel_of(int kcode, bool thick, int fmt, unsigned feat) {
  if (feat & TC_FEAT_CTRL)
    return lift([](auto kc, auto t, auto f, auto ft) -> step_kern_t { return tc_drive_step_kernel<StepKRb<kc>::K, t, f, StepKRb<kc>::RB, ft>; },
                Kcodes{kcode}, Thicks{thick}, Fmts{fmt}, DriveFeats{feat});
  return lift([](auto kc, auto t, auto f, auto ft) -> step_kern_t { return tc_step_kernel<StepKRb<kc>::K, t, f, StepKRb<kc>::RB, ft>; },
              Kcodes{kcode}, Thicks{thick}, Fmts{fmt}, Feats{feat});
}
// simulate stage alone, by register-cache variant, with or without the camera stage compiled in (without: fewer
// registers, half the code)
static step_kern_t env_kernel_of(int kv, bool cam, unsigned feat) {
  if (feat & TC_FEAT_CTRL)
    return lift([](auto k, auto c, auto ft) -> step_kern_t { return tc_drive_env_kernel<k, c, ft>; }, Kvars{kv}, Bools{cam}, DriveFeats{feat});
  return lift([](auto k, auto c, auto ft) -> step_kern_t { return tc_env_kernel<k, c, ft>; }, Kvars{kv}, Bools{cam}, Feats{feat});
}
static step_kern_t envg_kernel_of(unsigned feat) {
  if (feat & TC_FEAT_CTRL) return lift([](auto ft) -> step_kern_t { return tc_drive_envg_kernel<ft>; }, DriveFeats{feat});
  return lift([](auto ft) -> step_kern_t { return tc_envg_kernel<ft>; }, Feats{feat});
}
// recover: tc_frame_recover_kernel, the pass behind a streamed call's frame launch
static frame_kern_t frame_kernel_of(int kcode, bool thick, int fmt, bool recover) {
  return lift(
      [](auto kc, auto t, auto f, auto rec) -> frame_kern_t {
        if constexpr (rec) return tc_frame_recover_kernel<FrameKRb<kc>::K, t, f, FrameKRb<kc>::RB>;
        else return tc_frame_kernel<FrameKRb<kc>::K, t, f, FrameKRb<kc>::RB>;
      },
      Kcodes{kcode}, Thicks{thick}, FrameFmts{fmt}, Bools{recover});
}
static raster_kern_t raster_kernel_of(bool thick, int fmt) {
  return lift([](auto t, auto f) -> raster_kern_t { return tc_raster_kernel<t, f>; }, Thicks{thick}, FrameFmts{fmt});
}

#endif  // part 0: the kernel tables

// ---------------------------------------------------------------------------------------------
// tc_unpack_bits: packed class masks (TC_FMT_CLASSES_BITS) -> [n_out][planes][H][W] of u8 0/255 or f16 / bf16 / f32 0.0/1.0,
// optionally gathered through an index (the replay-buffer sample).  Bandwidth only: 1 bit read, 1-4 bytes written per pixel.
// W % 32 == 0, so a frame is one run of 32-bit words on the packed side (pixel p of the frame is bit p & 31 of word p >> 5)
// and one run of pixels on the other: a lane owns the P = 16 / 8 / 4 pixels of ONE 16-byte store, consecutive lanes store to
// consecutive addresses, and the 2 / 4 / 8 lanes that share a packed word read it with one address (a wavefront reads
// 128 / 64 / 32 consecutive bytes per round, once).  Workgroup (x, y) strides over the 256-store chunks of a frame and over
// the output frames, so one launch covers any n_out; the frame's source index is one scalar load per frame.
// An index outside [0, n_src) reads nothing and stores zeros.
template <int DT>
__global__ __launch_bounds__(256) void tc_unpack_bits_kernel(const unsigned int* __restrict__ src, const long long n_src,
                                                             const long long frame_words, const long long* __restrict__ index,
                                                             const long long n_out, uint4* __restrict__ dst) {
  constexpr int P = DT == TC_U8 ? 16 : DT == TC_F32 ? 4 : 8;  // pixels of one 16-byte store
  constexpr unsigned int ONE16 = DT == TC_F16 ? 0x3C00u : 0x3F80u;  // 1.0 as f16 / bf16
  const long long items = frame_words * (32 / P);              // 16-byte stores per frame
  for (long long j = blockIdx.y; j < n_out; j += gridDim.y) {
    const long long f = index ? index[j] : j;
    const bool inside = f >= 0 && f < n_src;  // (workgroup-uniform)
    const unsigned int* sf = src + (inside ? f : 0) * frame_words;
    uint4* df = dst + j * items;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
      const long long p0 = it * P;
      unsigned int b = 0;
      if (inside) b = (sf[p0 >> 5] >> (unsigned)(p0 & 31)) & ((1u << P) - 1u);
      uint4 o;
      if (DT == TC_U8) {
        o.x = spread4(b & 15u);
        o.y = spread4((b >> 4) & 15u);
        o.z = spread4((b >> 8) & 15u);
        o.w = spread4(b >> 12);
      } else if (DT == TC_F32) {
        o.x = (b & 1u) ? 0x3F800000u : 0u;
        o.y = (b & 2u) ? 0x3F800000u : 0u;
        o.z = (b & 4u) ? 0x3F800000u : 0u;
        o.w = (b & 8u) ? 0x3F800000u : 0u;
      } else {
        o.x = ((b & 1u) ? ONE16 : 0u) | ((b & 2u) ? ONE16 << 16 : 0u);
        o.y = ((b & 4u) ? ONE16 : 0u) | ((b & 8u) ? ONE16 << 16 : 0u);
        o.z = ((b & 16u) ? ONE16 : 0u) | ((b & 32u) ? ONE16 << 16 : 0u);
        o.w = ((b & 64u) ? ONE16 : 0u) | ((b & 128u) ? ONE16 << 16 : 0u);
      }
      df[it] = o;
    }
  }
}

#if defined(TC_PART) && TC_PART == 1
TC_INST_PART1(template)
#elif defined(TC_PART) && TC_PART == 2
TC_INST_PART2(template)
TC_INST_UNPACK(template)
#elif defined(TC_PART) && TC_PART == 3
TC_INST_PART3(template)
#elif defined(TC_PART) && TC_PART == 4
TC_INST_PART4(template)
#elif defined(TC_PART) && TC_PART == 5
TC_INST_PART5(template)
#elif defined(TC_PART)
TC_INST_UNPACK(extern template)
#endif

#if !defined(TC_PART) || TC_PART == 0
// =============================================================================================
// Host side: C ABI
// =============================================================================================
#include <assert.h>

#include <algorithm>
#include <memory>
#include <utility>

#include "tc_plan.h"

static thread_local std::string g_err;
static void set_err(const std::string& s) { g_err = s; }
extern "C" const char* tc_last_error(void) { return g_err.c_str(); }
extern "C" int tc_abi_version(void) { return TC_ABI_VERSION; }

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      set_err(std::string(#expr) + ": " + hipGetErrorString(_e));                        \
      return TC_E_HIP;                                                                   \
    }                                                                                    \
  } while (0)

// ---------------------------------------------------------------------------------------------
// Every switch the library reads from the environment, parsed once per tc_env_create / tc_map_create by read_tuning()
// -- the only place that looks at the environment.  INTEGRATION.md calls the shipped ones result-neutral.
struct Tuning {
  int fuse, env_grouped, envg_map_lds, first_per_env, stream, groups, seg_lds, frame_order, cand_grid, clip_merge, frame_cull, short_edges, info_every;  // on / off
  // tc_step_multi with observations, split form (default; 0 selects the fused K-step kernel): ONE
  // simulate launch loops over the K steps and leaves K draw lists per env, ONE raster launch of K x N workgroups
  // draws them.  Why: a frame costs between ~10 k clocks (nothing in view) and ~80 k (60 segments) to rasterise and an
  // env keeps its kind of view for many steps, so in the fused K-step kernel the launch lasts as long as its heaviest
  // env (measured on cfg3: 70.9 us per step against a mean of 41 us per wavefront-step).  Frames are independent of
  // each other, and K x N workgroups are many more than the chip holds at once, so the dispatcher balances them.
  int multi_split;
  int chunk;          // K-step calls with a rollout: steps per chunk
  int pipe;           // 1: the frame launches of a chunk run on an internal stream beside the next chunk's simulate launch
  int frame_streams;  // short K-step calls: frame launches of consecutive chunks alternate between two streams
  long long gate_ticks;  // bound of a frame workgroup's wait in a streamed call (100 MHz ticks)
  int gate_test;         // m > 0 (tests): frames with (row + env) % m == 0 are left to the gate-2 pass
  int band_bytes;     // LDS budget of one band's bit-planes
  bool band_fixed;    // ... given by the caller: the band is not shrunk to the camera stage's LDS afterwards
  int cam_group;      // nodes / edges per component group of the camera's copy of the map
  int seg_lds_limit;  // at most so many segments of a frame's draw list stay in LDS
  int order_every;    // the env order of single steps is refreshed every n-th tc_step, 0 = no such order
  double scratch_bytes;  // budget of the scratch of streamed K-step calls
  bool print_lds = false;             // development builds only (TC_ABLATE)
  int lds_pad = 0, step_lds_pad = 0;  // development builds only (TC_EXPERIMENT)
};

static Tuning read_tuning() {
  static_assert(5 * TC_NT == 320, "default of TC_CAM_GROUP below");
  static const struct {
    const char *name, *dflt, *what;
  } table[] = {
      {"TC_FUSE", "1", "0: a single step is a simulate launch and a raster launch instead of one tc_step_kernel"},
      {"TC_MULTI_SPLIT", "1", "0: K steps with frames loop inside the fused tc_step_kernel"},
      {"TC_ENV_GROUPED", "1", "0: K-step calls simulate with one wavefront per env (tc_env_kernel), not tc_envg_kernel"},
      {"TC_ENVG_MAP_LDS", "1", "0: tc_envg_kernel reads the edge and lanepath records from global memory, never LDS"},
      {"TC_CHUNK", "16", "steps per chunk of a chunked K-step call; <= 0: 16, and the chunks are not pipelined"},
      {"TC_FIRST_CHUNK_PER_ENV", "1", "0: the first chunk of a pipelined call is simulated by tc_envg_kernel too"},
      {"TC_FRAME_STREAMS", "2", "1: the frame launches of short chunks stay on one internal stream"},
      {"TC_STREAM", "1", "0: K-step calls run chunked instead of streamed"},
      {"TC_STREAM_WAIT_US", "5000", "patience of a frame workgroup of a streamed call, microseconds"},
      {"TC_STREAM_TEST_SKIP", "0", "m > 0 (tests): every m-th gated frame workgroup gives up at once"},
      {"TC_STREAM_SCRATCH_MB", "16384", "budget of a streamed call's scratch; longer calls run as segments"},
      {"TC_BAND_BYTES", "16384", "LDS bytes of one raster band's bit-planes (>= 1024); set: no later shrink"},
      {"TC_GROUPS", "1", "0: no camera groups, big maps take the K = 13 windowed path"},
      {"TC_CAM_GROUP", "320", "nodes / edges per component group; outside [64, 576]: groups of whole layers"},
      {"TC_SEG_LDS", "1", "0: draw lists go through global memory only"},
      {"TC_SEG_LDS_CAP", "-1", "n >= 0: at most n segments of a draw list stay in LDS"},
      {"TC_FRAME_ORDER", "1", "0: frame workgroups in env order instead of heaviest first"},
      {"TC_STEP_ORDER", "8", "single steps re-deal the envs to workgroups every n-th tc_step; <= 0: never"},
      {"TC_CAND_GRID", "1", "0: nearest-edge queries scan every edge instead of the candidate grid"},
      {"TC_CLIP_MERGE", "1", "0: the camera stage always runs its four clip passes one by one"},
      {"TC_FRAME_CULL", "1", "0: the camera stage never culls a whole frame from its pose (tc_cull.h)"},
      {"TC_SHORT_EDGES", "0", "1: thickness 2 draws the quad's two short outline edges too (tc_line.h)"},
      {"TC_INFO_EVERY_STEP", "0", "1: every step computes the lane-line distances, also where nothing reads them (tc_plan.h)"},
#ifdef TC_ABLATE
      {"TC_PRINT_LDS", "", "set: tc_env_create prints its LDS layout"},
#endif
#ifdef TC_EXPERIMENT
      {"TC_LDS_PAD", "0", "unused LDS bytes per frame workgroup (occupancy experiments)"},
      {"TC_STEP_LDS_PAD", "0", "unused LDS bytes per tc_step_kernel workgroup"},
#endif
  };
  // the switch's text, or its default; *set: whether the environment has it
  auto sw = [&](const char* name, bool* set = nullptr) -> const char* {
    for (const auto& row : table)
      if (!strcmp(row.name, name)) {
        const char* v = getenv(row.name);
        if (set) *set = v != nullptr;
        return v ? v : row.dflt;
      }
    assert(!"read_tuning: a switch that is not in the table");
    return "";
  };
  auto on = [&](const char* name) { return atoi(sw(name)) != 0 ? 1 : 0; };
  auto positive = [&](const char* name) { return atoi(sw(name)) > 0 ? atoi(sw(name)) : 0; };
  Tuning t;
  t.fuse = on("TC_FUSE");
  t.multi_split = on("TC_MULTI_SPLIT");
  t.env_grouped = on("TC_ENV_GROUPED");
  t.envg_map_lds = on("TC_ENVG_MAP_LDS");
  t.first_per_env = on("TC_FIRST_CHUNK_PER_ENV");
  t.stream = on("TC_STREAM");
  t.groups = on("TC_GROUPS");
  t.seg_lds = on("TC_SEG_LDS");
  t.frame_order = on("TC_FRAME_ORDER");
  t.cand_grid = on("TC_CAND_GRID");
  t.clip_merge = on("TC_CLIP_MERGE");
  t.frame_cull = on("TC_FRAME_CULL");
  t.short_edges = on("TC_SHORT_EDGES");
  t.info_every = on("TC_INFO_EVERY_STEP");
  t.pipe = positive("TC_CHUNK") > 0;
  t.chunk = t.pipe ? positive("TC_CHUNK") : 16;
  t.frame_streams = atoi(sw("TC_FRAME_STREAMS")) == 1 ? 1 : 2;
  t.gate_ticks = (long long)(atof(sw("TC_STREAM_WAIT_US")) * 100.0);
  t.gate_test = positive("TC_STREAM_TEST_SKIP");
  t.scratch_bytes = atof(sw("TC_STREAM_SCRATCH_MB")) * 1048576.0;
  t.band_bytes = atoi(sw("TC_BAND_BYTES", &t.band_fixed));
  if (t.band_bytes < 1024) t.band_bytes = 16384;
  t.cam_group = atoi(sw("TC_CAM_GROUP"));
  t.seg_lds_limit = atoi(sw("TC_SEG_LDS_CAP")) >= 0 ? atoi(sw("TC_SEG_LDS_CAP")) : 1 << 30;
  t.order_every = positive("TC_STEP_ORDER");
#ifdef TC_ABLATE
  (void)sw("TC_PRINT_LDS", &t.print_lds);
#endif
#ifdef TC_EXPERIMENT
  t.lds_pad = atoi(sw("TC_LDS_PAD"));
  t.step_lds_pad = atoi(sw("TC_STEP_LDS_PAD"));
#endif
  return t;
}

// ---------------------------------------------------------------------------------------------
// Move-only owners of a HIP resource: it is released when its owner goes or is assigned another.
template <class H, hipError_t (*Release)(H)>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
  Owned& operator=(Owned&& o) noexcept {  // (what this held goes with `o`)
    std::swap(h, o.h);
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (h) (void)Release(h);
    h = nullptr;
  }
  operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
template <class T>
struct DevPtr {  // device memory of `count` T
  Owned<void*, hipFree> mem;
  operator T*() const { return (T*)mem.h; }
  hipError_t alloc(size_t count) {
    mem.reset();
    return hipMalloc(&mem.h, count * sizeof(T));
  }
};

// Scratch of K-step calls, `rows` steps of it: what the simulate launch leaves per (step, env) for the frame launch
struct ScratchRows {
  DevPtr<int> seg_g;    // [..rows][N][seg_cap][5] draw lists
  DevPtr<int> seg_n;    // [..rows][N] their lengths
  DevPtr<double> pose;  // [..rows][N][TC_POSE_ROW]
  int rows = 0;
};

struct tc_map {
  DevMap d{};
  std::vector<DevPtr<char>> allocs;
  int device = 0;
  std::vector<double2> h_nodes;   // host copies of d.nodes / d.edges_g (tc_env_create groups the camera's copy by them)
  std::vector<int2> h_edges_g;
};

struct tc_env {
  explicit tc_env(const Tuning& t) : tune(t) {}
  const Tuning tune;
  const tc_map* map = nullptr;
  KArgs k{};
  // owners of what k points to: k.seg_g / k.seg_n, k.terms, k.spawn_tab, k.cam_nodes / k.cam_edges_g (the camera's copy of
  // the map, grouped by connected components, or NULL)
  DevPtr<int> seg_g, seg_n;
  DevPtr<tc_term> terms;
  DevPtr<int> spawn_tab;
  DevPtr<double2> cam_nodes;
  DevPtr<int2> cam_edges;
  DevPtr<unsigned char> cull_tab;  // k.cull_tab: the whole-frame cull's table (tc_cull.h), or NULL
  TcCullHead cull_head{};          // its header (tc_cull_cover reads it when the camera changes)
  CarRows cr{};          // per-env cars (tc_env_set_car_per_env / tc_env_set_car_randomization); rows NULL = shared car
  DevPtr<CarDrawTab> car_tab;  // device copy of the randomisation ranges (updated in place), or NULL
  EpArgs ep{};           // episodes (tc_env_set_episodes / tc_env_set_episode_rollout); length NULL = feature off
  DevPtr<int> ep_tab;    // device word holding max_episode_steps (updated in place), or NULL
  int ep_rows = 0;       // rows of ep.len_rows / ep.ret_rows
  CtrlArgs ct{};         // built-in controller (tc_env_set_controller); tab NULL = off
  DevPtr<CtrlTab> ctrl_tab;  // device copy of the gains (updated in place), or NULL
  CtrlTab ctrl_host{};   // what ctrl_tab holds
  int ctrl_rows = 0;     // rows of ct.noise / ct.rows
  DriveArgs dr{};        // drive randomisation (tc_env_set_drive_randomization); tab NULL = off
  DevPtr<DriveTab> drive_tab;  // device copy of the settings (updated in place), or NULL
  DriveTab drive_host{};  // what drive_tab holds
  int drive_rows = 0;    // rows of dr.man_rows / dr.noise_rows
  unsigned drive_flags = 0;  // TC_FI_DRIVE_* of every launch while it is on
  bool terms_read_dist = false;  // an installed term reads lane-line distances (term_reads_distances; tc_env_set_terms)
  CamBank cb{};          // camera bank (tc_env_set_camera_bank); index NULL = off.  k.cam_E / k.cam_K then point to the bank
  DevPtr<CamDrawTab> cam_tab;  // device copy of the draw settings (updated in place), or NULL
  CamDrawTab cam_host{};       // what cam_tab holds
  int cam_count = 0;     // cameras in the bank (0 = off)
  int cam_rows = 0;      // rows of cb.rows
  bool bound = false;
  int64_t obs_bytes = 0;
  int r_off_tab = 0, r_off_bits = 0, r_lds = 0;
  Stream frame_stream, frame_stream2;
  Event sim_ev, frames_ev, frames_ev2;
  Event slot_ev[TC_RING_SLOTS];  // frames of the chunk that last used ring slot s are done
  Event call_ev;                 // end of the last K-step call on its stream
  hipStream_t last_stream = nullptr;  // stream of that call
  bool have_call = false;
  // where the draw-list lengths of the most recent frames are (tc_env_draw_list_stats): up to TC_RING_SLOTS (first ring
  // row, rows) pairs of the last K-step call, or the per-env list of the last single step (draw_n < 0)
  int draw_rows[TC_RING_SLOTS][2] = {};
  int draw_n = 0;
  const int* draw_base = nullptr;  // the [rows][N] array the pairs index: the ring's, or the streamed call's
  // Streamed K-step calls (tune.stream = 0: chunked): ONE simulate launch for all steps of the call and ONE frame launch
  // beside it whose workgroups wait for their pose row -- see launch_streamed().  Scratch for streamed.rows steps
  // (tc_env_reserve_steps), every pose entry TC_POSE_EMPTY between calls; longer calls run as segments of that many steps.
  ScratchRows streamed;
  DevPtr<unsigned int> st_words;  // [0] simulate workgroups resident, [1] "a frame workgroup gave up waiting"
  Event start_ev;
  // scratch ring of chunked K-step calls (tc_env_reserve_steps): TC_RING_SLOTS chunks of ring.rows steps
  ScratchRows ring;
  int step_lds = 0;  // tc_step_kernel: LDS bytes per workgroup (lds.total grown like frame_lds)
  // heaviest-first order of the frame workgroups of a K-step call (tune.frame_order = 0: env order), one buffer per frame stream
  DevPtr<int> frame_order[2];               // [N] each
  const int* cost_row[2] = {};              // draw-list lengths of the last frame row launched on that stream (library scratch), or NULL
  bool frame_order_valid[2] = {};           // the buffer holds a permutation (a sort has run on it)
  // cost-aware env order of single-step launches (tc_order_kernel): refreshed every tune.order_every-th tc_step
  DevPtr<int> env_order;  // [N], a permutation (identity until the first refresh); NULL = off (order_every 0, N % G != 0)
  int order_g = 0;        // G = SIMDs of the device
  int order_calls = 0;
  int frame_lds = 0, seg_lds_off = 0, seg_lds_cap = 0;  // tc_frame_kernel: LDS bytes per workgroup, draw-list region (see KArgs)
  int kvar = 0;    // register-cache slots of the simulate stage: 5, 8 (whole map in one window), 9 (camera layer groups), 13
  int kframe = 0;  // tc_frame_kernel variant: kvar, or 516 (K = 5, batches of 16) when every component group fits 320 nodes / edges
  int frame_seg_cap = 0;  // tc_frame_kernel's own capacity: seg_lds_cap, but never below 8 (its raster stage reads the list from LDS only)
  // optional per-kernel timing: a ring of (start, mid, end) HIP events recorded on the caller's stream
  int prof = 0;    // 0 = off, n = record every n-th tc_step
  int prof_n = 0;  // launches recorded so far
  int prof_calls = 0;
  int prof_piped[TC_PROF_RING] = {};
  hipEvent_t ev[4][TC_PROF_RING] = {};  // start, simulate done, all done, first frame launch (pipelined calls)
  // NoiseObservationWrapper: blobs per plane (0 = off), radius bound, the per-radius span table, launch counter
  int noise_blobs = 0, noise_max_radius = 0;
  DevPtr<unsigned char> noise_hw;
  unsigned long long noise_seed = 0;
  DevPtr<unsigned int> noise_step;  // device counter
};

template <typename T>
static int upload(tc_map* m, const std::vector<T>& h, const T** out) {
  DevPtr<char> p;
  HIP_TRY(p.alloc((h.size() ? h.size() : 1) * sizeof(T)));
  *out = (const T*)(char*)p;
  m->allocs.push_back(std::move(p));
  if (h.size()) HIP_TRY(hipMemcpy((void*)*out, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return TC_OK;
}

extern "C" int tc_map_destroy(tc_map* m) {
  delete m;
  return TC_OK;
}

extern "C" int tc_map_create(const tc_map_desc* desc, tc_map** out) {
  if (!desc || !out) return TC_E_INVALID;
  *out = nullptr;
  const int C = desc->n_layers;
  {
    long long tn = 0;
    for (int l = 0; l < C && l < TC_MAX_LAYERS; l++) tn += desc->node_count[l];
    if (tn > 65535) {
      set_err("tc_map_create: at most 65535 lane-line nodes (node ids are packed in 16 bits in the clip lists)");
      return TC_E_INVALID;
    }
  }
  if (C < 1 || C > TC_MAX_LAYERS || desc->lanepath_node_count < 1 || desc->lanepath_edge_count < 0) {
    set_err("tc_map_create: need 1..16 lane-line layers and a non-empty lanepath");
    return TC_E_INVALID;
  }
  std::unique_ptr<tc_map> owner(new tc_map());
  tc_map* m = owner.get();
  DevMap& d = m->d;
  d.C = C;
  for (int l = 0; l < C; l++) {
    if (desc->node_count[l] < 0 || desc->edge_count[l] < 0) return TC_E_INVALID;
    d.node_off[l + 1] = d.node_off[l] + desc->node_count[l];
    d.edge_off[l + 1] = d.edge_off[l] + desc->edge_count[l];
    if (desc->node_count[l] > d.max_nodes) d.max_nodes = desc->node_count[l];
    if (desc->edge_count[l] > d.max_edges) d.max_edges = desc->edge_count[l];
    memcpy(d.colors[l], desc->colors + 3 * l, 3);
  }
  d.total_nodes = d.node_off[C];
  d.total_edges = d.edge_off[C];
  const int TN = d.total_nodes, TE = d.total_edges;
  // validate indices: the kernels index LDS/global with them
  for (int l = 0; l < C; l++)
    for (int e = d.edge_off[l]; e < d.edge_off[l + 1]; e++)
      for (int k = 0; k < 2; k++) {
        int v = desc->edges[2 * e + k];
        if (v < 0 || v >= desc->node_count[l]) {
          set_err("tc_map_create: lane-line edge references a node outside its layer");
          return TC_E_INVALID;
        }
      }
  const int lpN = desc->lanepath_node_count, lpE = desc->lanepath_edge_count;
  for (int e = 0; e < lpE; e++)
    for (int k = 0; k < 2; k++) {
      int v = desc->lanepath_edges[2 * e + k];
      if (v < 0 || v >= lpN) {
        set_err("tc_map_create: lanepath edge references a missing node");
        return TC_E_INVALID;
      }
    }
  std::vector<double2> nodes(TN), lpn(lpN);
  std::vector<int2> edges(TE), lpe(lpE), edges_g(TE);
  std::vector<int> edge_layer(TE);
  std::vector<double> of(TE), orv(TE), lpo(lpE), nori(lpE), pori(lpE);
  std::vector<double4> exy(TE);
  std::vector<int> noff(lpN + 1, 0), poff(lpN + 1, 0), nnode(lpE), pnode(lpE);
  for (int i = 0; i < TN; i++) nodes[i] = make_double2(desc->nodes[2 * i], desc->nodes[2 * i + 1]);
  for (int l = 0; l < C; l++)
    for (int e = d.edge_off[l]; e < d.edge_off[l + 1]; e++) {
      edges[e] = make_int2(desc->edges[2 * e], desc->edges[2 * e + 1]);
      edges_g[e] = make_int2(d.node_off[l] + edges[e].x, d.node_off[l] + edges[e].y);
      edge_layer[e] = l;
      double2 a = nodes[d.node_off[l] + edges[e].x], b = nodes[d.node_off[l] + edges[e].y];
      double evx = b.x - a.x, evy = b.y - a.y;
      // static halves of layer.py:140-141, evaluated with the host libm like the reference does
      of[e] = atan2(evy, evx);
      orv[e] = atan2(-evy, -evx);
      exy[e] = make_double4(a.x, a.y, b.x, b.y);
    }
  for (int i = 0; i < lpN; i++) lpn[i] = make_double2(desc->lanepath_nodes[2 * i], desc->lanepath_nodes[2 * i + 1]);
  for (int e = 0; e < lpE; e++) {
    lpe[e] = make_int2(desc->lanepath_edges[2 * e], desc->lanepath_edges[2 * e + 1]);
    double2 a = lpn[lpe[e].x], b = lpn[lpe[e].y];
    lpo[e] = atan2(b.y - a.y, b.x - a.x);  // layer.py:179-181
    noff[lpe[e].x + 1]++;
    poff[lpe[e].y + 1]++;
  }
  for (int i = 0; i < lpN; i++) {
    noff[i + 1] += noff[i];
    poff[i + 1] += poff[i];
  }
  {  // get_next_nodes / get_prev_nodes (layer.py:183-185) as CSR, edge-list order preserved
    std::vector<int> nf(lpN, 0), pf(lpN, 0);
    for (int e = 0; e < lpE; e++) {
      int a = lpe[e].x, b = lpe[e].y;
      int s = noff[a] + nf[a]++;
      nnode[s] = b;
      nori[s] = atan2(lpn[b].y - lpn[a].y, lpn[b].x - lpn[a].x);  // layer.py:122 seen from a
      int p = poff[b] + pf[b]++;
      pnode[p] = a;
      pori[p] = atan2(lpn[a].y - lpn[b].y, lpn[a].x - lpn[b].x);  // layer.py:122 seen from b
    }
  }
  std::vector<LpNode> fat(lpN);
  for (int i = 0; i < lpN; i++) {
    LpNode& F = fat[i];
    memset(&F, 0, sizeof(F));
    F.x = lpn[i].x;
    F.y = lpn[i].y;
    F.nnext = noff[i + 1] - noff[i];
    F.nprev = poff[i + 1] - poff[i];
    for (int k = 0; k < 3; k++) {
      F.next[k] = k < F.nnext ? nnode[noff[i] + k] : -1;
      F.next_ori[k] = k < F.nnext ? nori[noff[i] + k] : 0.0;
      F.prev[k] = k < F.nprev ? pnode[poff[i] + k] : -1;
      F.prev_ori[k] = k < F.nprev ? pori[poff[i] + k] : 0.0;
    }
  }
  d.lpN = lpN;
  d.lpE = lpE;
  d.first_spawnable = -1;
  for (int i = 0; i < lpN && d.first_spawnable < 0; i++)
    if (noff[i + 1] > noff[i]) d.first_spawnable = i;
  if (d.first_spawnable < 0) {
    set_err("tc_map_create: lanepath has no edge, nothing can spawn");
    return TC_E_INVALID;
  }
  // ---- candidate grid (see DevMap): cells of >= 4 cm, at most ~64 k of them, over the lane lines + 4 m
  std::vector<int> coff(1, 0), cidx;
  {
    bool finite = TN > 0 && TE > 0;
    double bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
    for (int i = 0; i < TN && finite; i++) {
      const double x = nodes[i].x, y = nodes[i].y;
      if (!(fabs(x) < 1e12) || !(fabs(y) < 1e12)) finite = false;
      if (i == 0 || x < bx0) bx0 = x;
      if (i == 0 || x > bx1) bx1 = x;
      if (i == 0 || y < by0) by0 = y;
      if (i == 0 || y > by1) by1 = y;
    }
    finite = finite && read_tuning().cand_grid;
    std::vector<double> f(d.max_edges > 0 ? d.max_edges : 1);
    // appends the lists of an nx x ny grid of `cell`-sized cells with origin (x0, y0); returns the id of its first cell
    auto add_level = [&](double x0, double y0, double cell, int nx, int ny) {
      const int base = (int)((coff.size() - 1) / C);
      const double r = 0.5 * sqrt(2.0) * cell * 1.001 + 1e-12;
      coff.resize(coff.size() + (size_t)nx * ny * C, 0);
      for (int iy = 0; iy < ny; iy++)
        for (int ix = 0; ix < nx; ix++) {
          const double cx = x0 + (ix + 0.5) * cell, cy = y0 + (iy + 0.5) * cell;
          for (int l = 0; l < C; l++) {
            const int e0 = d.edge_off[l], e1 = d.edge_off[l + 1];
            double fmin = 0;
            for (int e = e0; e < e1; e++) {
              const double4 q = exy[e];
              const double a0 = q.x - cx, a1 = q.y - cy, b0 = q.z - cx, b1 = q.w - cy;
              f[e - e0] = sqrt(a0 * a0 + a1 * a1) + sqrt(b0 * b0 + b1 * b1);
              if (e == e0 || f[e - e0] < fmin) fmin = f[e - e0];
            }
            const double thr = fmin + 4.0 * r + 1e-9 * (1.0 + fmin);
            for (int e = e0; e < e1; e++)
              if (f[e - e0] <= thr) cidx.push_back(e);
            coff[((size_t)base + (size_t)iy * nx + ix) * C + l + 1] = (int)cidx.size();
          }
          if (cidx.size() > (size_t)48 << 20) return -1;  // a map on which the lists do not thin out (192 MB of ids): no grid
        }
      return base;
    };
    if (finite) {
      const double margin = 4.0, x0 = bx0 - margin, y0 = by0 - margin, x1 = bx1 + margin, y1 = by1 + margin;
      double cell = sqrt((x1 - x0) * (y1 - y0) / 65536.0);
      if (cell < 0.04) cell = 0.04;
      const int nx = (int)ceil((x1 - x0) / cell), ny = (int)ceil((y1 - y0) / cell);
      if (nx >= 1 && ny >= 1 && (long long)nx * ny <= 200000 && add_level(x0, y0, cell, nx, ny) >= 0) {
        d.grid_nx = nx;
        d.grid_ny = ny;
        d.grid_x0 = x0;
        d.grid_y0 = y0;
        d.grid_inv = 1.0 / cell;
      }
    }
    if (d.grid_nx == 0) {  // no grid (or abandoned): the kernels take the identity lists
      coff.assign(1, 0);
      cidx.clear();
    }
    if (cidx.empty()) cidx.push_back(0);
  }
  int rc = TC_OK;
  HIP_TRY(hipGetDevice(&m->device));
#define UP(vec, field)                                             \
  if (rc == TC_OK) rc = upload(m, vec, &d.field);
  UP(fat, lp_fat) UP(nodes, nodes) UP(edges, edges) UP(edges_g, edges_g) UP(edge_layer, edge_layer) UP(of, ori_fwd) UP(orv, ori_rev) UP(exy, edge_xy) UP(lpn, lp_nodes) UP(lpe, lp_edges)
  UP(lpo, lp_ori) UP(noff, next_off) UP(nnode, next_node) UP(nori, next_ori) UP(poff, prev_off)
  UP(pnode, prev_node) UP(pori, prev_ori) UP(coff, cand_off) UP(cidx, cand_idx)
#undef UP
  m->h_nodes = nodes;
  m->h_edges_g = edges_g;
  if (rc != TC_OK) return rc;
  *out = owner.release();
  return TC_OK;
}

// the constants tc_env_set_car may change (T and the presence flags are fixed at tc_env_create)
static void fill_car_constants(DevCar& c, const tc_car_params* car) {
  c.wheelbase = car->wheelbase;
  c.track_width = car->track_width;
  c.max_velocity = car->max_velocity;
  c.max_steering_angle = car->max_steering_angle;
  c.steering_speed = car->steering_speed;
  c.max_acceleration = car->max_acceleration;
  c.max_deceleration = car->max_deceleration;
}

static int fill_camera(tc_env* e, const tc_camera_params* cam) {
  if (cam->height < 1 || cam->width < 1 || cam->height > 16384 || cam->width > 16384 || cam->line_thickness < 1 ||
      cam->line_thickness > 255 || !(cam->max_range > 0) ||
      (cam->format != TC_FMT_RGB && !TC_FMT_IS_CLASSES(cam->format))) {
    set_err("camera: need height,width,line_thickness >= 1, max_range > 0, format rgb|classes|classes_bits");
    return TC_E_INVALID;
  }
  if (cam->format == TC_FMT_CLASSES_BITS && cam->width % 32 != 0) {
    set_err("camera: TC_FMT_CLASSES_BITS needs a width that is a multiple of 32 (a packed row is the row's 32-bit words)");
    return TC_E_INVALID;
  }
  DevCam& c = e->k.cam;
  c.H = cam->height;
  c.W = cam->width;
  memcpy(c.E, cam->E, sizeof(c.E));
  memcpy(c.K, cam->K, sizeof(c.K));
  c.max_range = cam->max_range;
  c.thickness = cam->line_thickness;
  c.format = cam->format;
  c.wpr = (c.W + 31) / 32;
  return TC_OK;
}

// ---- tc_env_create, step by step (in the order they are called)

static int create_streams_and_events(tc_env* e) {
  bool ok = hipStreamCreateWithFlags(&e->frame_stream.h, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&e->frame_stream2.h, hipStreamNonBlocking) == hipSuccess;
  for (Event* ev : {&e->frames_ev2, &e->sim_ev, &e->start_ev, &e->frames_ev, &e->call_ev, &e->slot_ev[0], &e->slot_ev[1], &e->slot_ev[2]})
    ok = ok && hipEventCreateWithFlags(&ev->h, hipEventDisableTiming) == hipSuccess;
  static_assert(TC_RING_SLOTS == 3, "slot events are listed one by one above");
  if (!ok) {
    set_err("tc_env_create: cannot create the internal frame streams / events");
    return TC_E_HIP;
  }
  return TC_OK;
}

// bit-plane band: keep one band's planes within a budget so several envs share a CU's 160 KiB LDS
static void set_band_rows(tc_env* e, int band_rows) {
  DevCam& dc = e->k.cam;
  if (band_rows < 1) band_rows = 1;
  if (band_rows > dc.H) band_rows = dc.H;
  dc.band_rows = band_rows;
  dc.n_bands = (dc.H + band_rows - 1) / band_rows;
}

// Camera groups of whole layers (tc_plan.h), or the whole map as one group: sets kvar and the group bounds; returns
// the nodes / edges of the largest group through cap_n / cap_e.
static void plan_layers(tc_env* e, int* cap_n, int* cap_e) {
  const DevMap& m = e->k.m;
  const int big = m.total_nodes > m.total_edges ? m.total_nodes : m.total_edges;
  *cap_n = m.total_nodes;
  *cap_e = m.total_edges;
  e->k.n_grp = 1;
  e->k.grp_layer[0] = 0;
  e->k.grp_layer[1] = m.C;
  e->kvar = big <= 5 * TC_NT ? 5 : big <= 8 * TC_NT ? 8 : 13;
  if (big > 8 * TC_NT && e->tune.groups) {
    const LayerGroups p = plan_layer_groups(m.node_off, m.edge_off, m.C, 9 * TC_NT, TC_MAX_GROUPS);
    if (p.ok) {
      e->k.n_grp = (int)p.layer.size() - 1;
      std::copy(p.layer.begin(), p.layer.end(), e->k.grp_layer);
      *cap_n = p.cap_n;
      *cap_e = p.cap_e;
      e->kvar = 9;
    }
  }
  for (int g = 0; g <= e->k.n_grp; g++) {
    e->k.grp_n0[g] = m.node_off[e->k.grp_layer[g]];
    e->k.grp_e0[g] = m.edge_off[e->k.grp_layer[g]];
  }
  for (int g = 0; g < e->k.n_grp; g++) {
    e->k.grp_l0[g] = e->k.grp_layer[g];
    e->k.grp_l1[g] = e->k.grp_layer[g + 1];
  }
}

// The camera's copy of the map with the nodes renumbered by `p`, on the device; false (nothing kept) when that fails.
static bool upload_camera_copy(tc_env* e, const ComponentGroups& p) {
  const tc_map* map = e->map;
  std::vector<double2> cn((size_t)p.n0.back());
  std::vector<int2> ce(map->h_edges_g.size());
  for (size_t i = 0; i < map->h_nodes.size(); i++)
    if (p.new_id[i] >= 0) cn[p.new_id[i]] = map->h_nodes[i];
  for (size_t ed = 0; ed < ce.size(); ed++) ce[ed] = make_int2(p.new_id[map->h_edges_g[ed].x], p.new_id[map->h_edges_g[ed].y]);
  DevPtr<double2> dn;
  DevPtr<int2> de;
  if (dn.alloc(cn.size()) != hipSuccess || de.alloc(ce.size()) != hipSuccess ||
      hipMemcpy(dn, cn.data(), cn.size() * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(de, ce.data(), ce.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess)
    return false;
  e->cam_nodes = std::move(dn);
  e->cam_edges = std::move(de);
  e->k.cam_nodes = e->cam_nodes;
  e->k.cam_edges_g = e->cam_edges;
  return true;
}

// Camera groups of connected components (tc_plan.h) in place of the layer groups, where the plan succeeds
static void plan_components(tc_env* e, int* cap_n, int* cap_e) {
  const DevMap& m = e->k.m;
  const tc_map* map = e->map;
  const int T = e->tune.cam_group;
  if (e->k.n_grp < 2 || e->kvar != 9 || (int)map->h_nodes.size() != m.total_nodes || (int)map->h_edges_g.size() != m.total_edges ||
      T < TC_NT || T > 9 * TC_NT)
    return;
  static_assert(sizeof(int2) == 2 * sizeof(int), "edges are read as pairs of int");
  const ComponentGroups p = plan_component_groups(m.edge_off, m.C, (const int*)map->h_edges_g.data(), m.total_nodes, T, TC_MAX_GROUPS);
  if (!p.ok || !upload_camera_copy(e, p)) return;
  e->k.n_grp = (int)p.l0.size();
  std::copy(p.n0.begin(), p.n0.end(), e->k.grp_n0);
  std::copy(p.e0.begin(), p.e0.end(), e->k.grp_e0);
  std::copy(p.l0.begin(), p.l0.end(), e->k.grp_l0);
  std::copy(p.l1.begin(), p.l1.end(), e->k.grp_l1);
  *cap_n = p.cap_n;
  *cap_e = p.cap_e;
}

// LDS of a workgroup: the camera stage's buffers (tc_plan.h), the raster stage's tables and band, the parked env state
static void layout_lds(tc_env* e, int cap_n, int cap_e) {
  const DevMap& m = e->k.m;
  DevCam& dc = e->k.cam;
  LdsLayout& L = e->k.lds;
  e->kframe = e->kvar;
  if (e->k.cam_nodes && cap_n <= 5 * TC_NT && cap_e <= 5 * TC_NT) e->kframe = 516;
  e->k.cap_nodes = cap_n > 0 ? cap_n : 1;
  plan_cam_lds(L, cap_n, cap_e, m.total_nodes);
  // raster kernel: tables + bit-planes of one band
  // A frame taller than one band: the workgroup's LDS is the larger of the two stages' needs, and how many workgroups a
  // CU holds decides the rate of the big frames (cfg5: 6 per CU at 23.2 KB, 9 at 17.4 KB: 3.10 -> 3.82 M env-steps/s).
  // So the band shrinks until the raster stage needs no more than the camera stage does anyway -- not further: more
  // bands only repeat the per-band set-up (measured: 8 KB and 6 KB bands are slower again).
  // (tables of the batch size the fused / frame kernels of this variant are compiled with; tc_raster_kernel: RB_MAX)
  const int row_bytes = m.C * dc.wpr * 4;
  const int r_off_bits_k = e->kvar == 13 ? R_OFF_BITS_OF(RB_MAX) : (e->kvar >= 8 ? R_OFF_BITS_OF(RB_OF_K(8)) : R_OFF_BITS_OF(RB_OF_K(5)));
  if (dc.n_bands > 1 && !e->tune.band_fixed) {
    const int fit = (L.total - r_off_bits_k) / row_bytes;
    if (fit >= 8 && fit < dc.band_rows) set_band_rows(e, fit);
  }
  e->r_off_tab = R_OFF_TAB;
  e->r_off_bits = R_OFF_BITS_OF(RB_MAX);
  e->r_lds = e->r_off_bits + align_up(dc.band_rows * row_bytes, 16);
  // the env's parked state (tc_step_multi) sits behind whichever stage needs more, so that neither aliases it
  const int r_lds_k = r_off_bits_k + align_up(dc.band_rows * row_bytes, 16);
  L.off_live = align_up(L.total > r_lds_k ? L.total : r_lds_k, 16);
  L.total = L.off_live + TC_LIVE_BYTES;
}

// tc_frame_kernel keeps no env state in LDS, so the bytes behind both stages' buffers -- the LiveLds slot and whatever
// the workgroup can grow without costing the CU a workgroup (160 KB / workgroups per CU, in 1280-byte steps) --
// hold the head of the frame's draw list: the raster stage reads what the camera stage of the same wavefront just
// wrote without a round trip through global memory (cfg3: 44 of a frame's ~20-30 segments).
static void grow_lds_for_draw_lists(tc_env* e) {
  const LdsLayout& L = e->k.lds;
  const int cu_lds = 160 * 1024;
  const int w = cu_lds / L.total > 0 ? cu_lds / L.total : 1;
  int grown = cu_lds / w / 1280 * 1280;
  if (grown > L.total + 4096) grown = L.total + 4096;  // (200 segments are plenty)
  if (grown < L.total) grown = L.total;
#ifdef TC_TIMING_LDS
  if (grown - 256 >= L.total) grown -= 256;  // the stamp buffer (static LDS) comes out of the draw-list head: same workgroups per CU
#endif
  e->frame_lds = e->step_lds = grown;
  e->seg_lds_off = L.off_live;
  e->seg_lds_cap = (grown - L.off_live) / 20;
  if (!e->tune.seg_lds) {
    e->seg_lds_cap = 0;
    e->frame_lds = e->step_lds = L.total;
  }
  // tune.seg_lds_limit (tests): a small n makes every frame take the mixed LDS + global list that otherwise only frames
  // with more than ~44 segments reach
  if (e->seg_lds_cap > e->tune.seg_lds_limit) e->seg_lds_cap = e->tune.seg_lds_limit;
  // tc_frame_kernel reads draw lists from LDS only (longer ones batch by batch through it): it keeps a region of at least
  // 8 entries whatever the switches above say (they still rule tc_step_kernel, which has the generic form)
  e->frame_seg_cap = e->seg_lds_cap;
  if (e->frame_seg_cap < 8) {
    e->frame_seg_cap = 8;
    if (e->frame_lds < e->seg_lds_off + 8 * 20) e->frame_lds = e->seg_lds_off + 8 * 20;
  }
#ifdef TC_ABLATE
  if (e->tune.print_lds)
    fprintf(stderr, "tc_env_create: lds.total %d off_live %d frame_lds %d seg_lds_cap %d r_lds %d band_rows %d n_bands %d\n", (int)L.total,
            (int)L.off_live, e->frame_lds, e->seg_lds_cap, e->r_lds, e->k.cam.band_rows, e->k.cam.n_bands);
#endif
#ifdef TC_EXPERIMENT
  // occupancy experiments (make dev-exp, never shipped): unused LDS bytes per frame workgroup -> fewer workgroups per CU
  e->frame_lds += e->tune.lds_pad;
  e->step_lds += e->tune.step_lds_pad;
#endif
}

static int raise_lds_limits(const tc_env* e) {
  const DevMap& m = e->k.m;
  const int total = e->k.lds.total;
  int rc = TC_OK;
  // lets `kernel` be launched with `bytes` of dynamic LDS (beyond the runtime's default limit); after a refusal no more are tried
  auto raise = [&rc](const void* kernel, int bytes, const char* family) {
    const hipError_t he = rc == TC_OK ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) : hipSuccess;
    if (he == hipSuccess) return;
    (void)hipGetLastError();
    set_err(std::string("tc_env_create: cannot raise the dynamic LDS limit of ") + family + " to " + std::to_string(bytes) +
            " bytes: " + hipGetErrorString(he));
    rc = TC_E_HIP;
  };
  int lds = total > e->r_lds ? total : e->r_lds;
  if (e->frame_lds > lds) lds = e->frame_lds;
  if (lds > 48 * 1024)  // every tc_step_kernel and tc_frame_kernel variant
    for (int kcode : {516, 5, 8, 9})
      for (int t = 0; t < 2; t++)
        for (int fmt : {TC_FMT_CLASSES, TC_FMT_CLASSES_BITS, TC_FMT_RGB}) {
          for (unsigned feat = 0; feat <= (TC_FEAT_CTRL | TC_FEAT_ALL) && fmt != TC_FMT_CLASSES_BITS; feat++)
            raise((const void*)step_kernel_of(kcode, t, fmt, feat), lds, (feat & TC_FEAT_CTRL) ? "tc_drive_step_kernel" : "tc_step_kernel");
          raise((const void*)frame_kernel_of(kcode, t, fmt, false), lds, "tc_frame_kernel");
        }
  // tc_envg_kernel's LDS copies of the map (edge records + fat lanepath nodes, see launch_envg()) can exceed the 48 KB default
  const size_t envg_lds = ((size_t)m.total_edges * 48 + 15) / 16 * 16 + (size_t)m.lpN * sizeof(LpNode);
  if (envg_lds > 40 * 1024)
    for (unsigned feat = 0; feat <= (TC_FEAT_CTRL | TC_FEAT_ALL); feat++)
      raise((const void*)envg_kernel_of(feat), (int)(envg_lds < 150 * 1024 ? envg_lds : 150 * 1024),
            (feat & TC_FEAT_CTRL) ? "tc_drive_envg_kernel" : "tc_envg_kernel");
  if (e->r_lds > 48 * 1024)
    for (int t = 0; t < 2; t++)
      for (int fmt : {TC_FMT_CLASSES, TC_FMT_CLASSES_BITS, TC_FMT_RGB}) raise((const void*)raster_kernel_of(t, fmt), e->r_lds, "tc_raster_kernel");
  if (total > 48 * 1024) {
    static const int kvs[4] = {5, 8, 9, 13};
    for (int i = 0; i < 64; i++)  // every tc_env_kernel / tc_drive_env_kernel variant
      raise((const void*)env_kernel_of(kvs[i & 3], (i & 4) == 0, (unsigned)i >> 3), total, (i >> 5) ? "tc_drive_env_kernel" : "tc_env_kernel");
  }
  return rc;
}

// the draw list of the current frame, per env (single steps)
static int alloc_draw_lists(tc_env* e) {
  const size_t N = (size_t)e->k.N;
  e->k.seg_cap = e->k.m.total_edges > 0 ? e->k.m.total_edges : 1;
  hipError_t he = e->seg_g.alloc(N * e->k.seg_cap * 5);
  if (he == hipSuccess) he = e->seg_n.alloc(N);
  if (he == hipSuccess) he = hipMemset(e->seg_n, 0, N * sizeof(int));
  if (he != hipSuccess) {
    set_err(std::string("hipMalloc(draw list): ") + hipGetErrorString(he));
    return TC_E_NOMEM;
  }
  e->k.seg_g = e->seg_g;
  e->k.seg_n = e->seg_n;
  return TC_OK;
}

// The orders workgroups are dealt in; each is optional (an allocation that fails leaves it off).
static void alloc_orders(tc_env* e) {
  const int N = e->k.N;
  // heaviest-first order of the frame workgroups of a K-step call, one buffer per frame stream
  if (e->tune.frame_order && N <= 60000) {
    DevPtr<int> f0, f1;
    if (f0.alloc((size_t)N) == hipSuccess && f1.alloc((size_t)N) == hipSuccess) {
      e->frame_order[0] = std::move(f0);
      e->frame_order[1] = std::move(f1);
    } else {
      (void)hipGetLastError();
    }
  }
  // cost-aware env order of single-step launches (tc_order_kernel): when the N workgroups are whole rows of G = SIMDs
  // of the device and all resident at once (N / G <= 4 wavefronts per SIMD)
  hipDeviceProp_t prop;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) e->order_g = prop.multiProcessorCount * 4;
  if (e->tune.order_every > 0 && e->order_g > 0 && N % e->order_g == 0 && N / e->order_g <= 4 && N / e->order_g >= 2) {
    std::vector<int> ident((size_t)N);
    for (int i = 0; i < N; i++) ident[(size_t)i] = i;
    DevPtr<int> o;
    if (o.alloc((size_t)N) == hipSuccess && hipMemcpy(o, ident.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice) == hipSuccess)
      e->env_order = std::move(o);
    else
      (void)hipGetLastError();
  }
}

// The whole-frame cull's table (tc_cull.h): built from the host copy of the lane-line graph, uploaded once; the cover of
// the camera follows in cover_cull().  Cells of 2 cm, 1 m of margin (a cover circle of the bundled cameras has 0.3-0.45 m).
static void cover_cull(tc_env* e) {
  tc_cull_cover(e->k.cam.E, e->k.cam.K, e->k.cam.W, e->k.cam.H, e->k.cam.max_range, e->cull_head, &e->k.cull);
  e->k.frame_cull = e->tune.frame_cull && e->k.cull_tab && e->k.cull.on && !e->k.cam_E;
}
static int plan_cull(tc_env* e) {
  const tc_map* map = e->map;
  std::vector<unsigned char> tab;
  tc_cull_plan(map->h_nodes.empty() ? nullptr : &map->h_nodes[0].x, (int)map->h_nodes.size(),
               map->h_edges_g.empty() ? nullptr : &map->h_edges_g[0].x, (int)map->h_edges_g.size(), 0.02, 1.0, tab);
  memcpy(&e->cull_head, tab.data(), sizeof(e->cull_head));
  if (e->cull_head.nx > 0) {
    HIP_TRY(e->cull_tab.alloc(tab.size()));
    HIP_TRY(hipMemcpy(e->cull_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    e->k.cull_tab = e->cull_tab;
  }
  cover_cull(e);
  return TC_OK;
}

extern "C" int tc_env_create(const tc_map* map, const tc_car_params* car, const tc_camera_params* cam,
                             int32_t num_envs, tc_env** out) {
  if (!map || !car || !cam || !out || num_envs < 1) return TC_E_INVALID;
  *out = nullptr;
  std::unique_ptr<tc_env> e(new tc_env(read_tuning()));
  e->map = map;
  int rc = create_streams_and_events(e.get());
  if (rc != TC_OK) return rc;
  e->k.m = map->d;
  e->k.N = num_envs;
  e->k.clip_merge = e->tune.clip_merge;
  e->k.car.T = car->T;
  e->k.car.has_steering_speed = car->has_steering_speed;
  e->k.car.has_max_acceleration = car->has_max_acceleration;
  fill_car_constants(e->k.car, car);
  rc = fill_camera(e.get(), cam);
  if (rc != TC_OK) return rc;
  rc = plan_cull(e.get());
  if (rc != TC_OK) return rc;
  const DevCam& dc = e->k.cam;
  const DevMap& m = map->d;
  set_band_rows(e.get(), e->tune.band_bytes / (m.C * dc.wpr * 4));
  int cap_n = 0, cap_e = 0;  // nodes / edges of the largest camera group
  plan_layers(e.get(), &cap_n, &cap_e);
  plan_components(e.get(), &cap_n, &cap_e);
  layout_lds(e.get(), cap_n, cap_e);
  grow_lds_for_draw_lists(e.get());
  if (e->k.lds.total > 160 * 1024 || e->r_lds > 160 * 1024) {
    set_err("tc_env_create: map too large for one workgroup's LDS");
    return TC_E_LDS;
  }
  rc = raise_lds_limits(e.get());
  if (rc != TC_OK) return rc;
  e->obs_bytes = (int64_t)tc_obs_bytes_of(dc.format, m.C, dc.H, dc.W);
  rc = alloc_draw_lists(e.get());
  if (rc != TC_OK) return rc;
  alloc_orders(e.get());
  *out = e.release();
  return TC_OK;
}

extern "C" int tc_env_profile(tc_env* e, int32_t enable) {
  if (!e) return TC_E_INVALID;
  if (enable && !e->ev[0][0]) {
    for (int k = 0; k < 4; k++)
      for (int i = 0; i < TC_PROF_RING; i++) HIP_TRY(hipEventCreate(&e->ev[k][i]));
  }
  e->prof = enable > 0 ? enable : 0;
  e->prof_n = 0;
  e->prof_calls = 0;
  return TC_OK;
}

extern "C" int tc_env_profile_read(tc_env* e, double* sim_us, double* raster_us, int32_t* launches) {
  if (!e || !sim_us || !raster_us || !launches) return TC_E_INVALID;
  int n = e->prof_n < TC_PROF_RING ? e->prof_n : TC_PROF_RING;
  double a = 0, b = 0;
  for (int i = 0; i < n; i++) {
    float t0 = 0, t1 = 0;
    HIP_TRY(hipEventSynchronize(e->ev[2][i]));
    HIP_TRY(hipEventElapsedTime(&t0, e->ev[0][i], e->ev[1][i]));
    // pipelined K-step call: the frame launches run beside the simulate launches, from their own start event
    HIP_TRY(hipEventElapsedTime(&t1, e->prof_piped[i] ? e->ev[3][i] : e->ev[1][i], e->ev[2][i]));
    a += t0;
    b += t1;
  }
  *launches = n;
  *sim_us = n ? a / n * 1e3 : 0;
  *raster_us = n ? b / n * 1e3 : 0;
  return TC_OK;
}

extern "C" int tc_env_destroy(tc_env* e) {
  if (!e) return TC_OK;
  if (e->ev[0][0])
    for (int k = 0; k < 4; k++)
      for (int i = 0; i < TC_PROF_RING; i++) (void)hipEventDestroy(e->ev[k][i]);
  delete e;
  return TC_OK;
}

extern "C" int64_t tc_env_obs_bytes(const tc_env* e) { return e ? e->obs_bytes : TC_E_INVALID; }
extern "C" int64_t tc_env_lds_bytes(const tc_env* e) { return e ? (e->k.lds.total > e->r_lds ? e->k.lds.total : e->r_lds) : TC_E_INVALID; }

extern "C" int tc_env_bind(tc_env* e, const tc_buffers* b) {
  if (!e || !b) return TC_E_INVALID;
  if (!b->x || !b->y || !b->theta || !b->velocity || !b->steering || !b->radius || !b->front_x || !b->front_y ||
      !b->local_path || !b->lp_len || !b->last_maneuver || !b->cte || !b->heading_error || !b->reward ||
      !b->terminated || !b->truncated || !b->status || !b->laneline_distances || !b->nearest_edge) {
    set_err("tc_env_bind: a required buffer pointer is NULL");
    return TC_E_INVALID;
  }
  if (b->needs_reset && (!b->spawn_queue || !b->spawn_cursor || b->spawn_queue_len < 1)) {
    set_err("tc_env_bind: needs_reset given without spawn_queue/spawn_cursor/spawn_queue_len");
    return TC_E_INVALID;
  }
  e->k.b = *b;
  e->bound = true;
  return TC_OK;
}

static bool car_ok(const tc_car_params* c) {
  const double v[7] = {c->wheelbase, c->track_width, c->max_velocity, c->max_steering_angle, c->steering_speed,
                       c->max_acceleration, c->max_deceleration};
  for (int i = 0; i < 7; i++)
    if (!isfinite(v[i])) return false;
  return true;
}

extern "C" int tc_env_set_car(tc_env* e, const tc_car_params* car) {
  if (!e || !car) return TC_E_INVALID;
  if (car->T != e->k.car.T || car->has_steering_speed != e->k.car.has_steering_speed ||
      car->has_max_acceleration != e->k.car.has_max_acceleration || !car_ok(car)) {
    set_err("tc_env_set_car: T and the presence flags are fixed at tc_env_create, and every constant must be finite");
    return TC_E_INVALID;
  }
  fill_car_constants(e->k.car, car);
  return TC_OK;
}

extern "C" int tc_env_set_car_per_env(tc_env* e, double* params) {
  if (!e) return TC_E_INVALID;
  e->cr.rows = params;
  if (!params) {  // back to the shared car: nothing left to randomise
    e->cr.tab = nullptr;
    e->cr.episode = nullptr;
  }
  return TC_OK;
}

extern "C" int tc_env_set_car_randomization(tc_env* e, const double* lo, const double* hi, uint32_t column_mask,
                                            uint64_t seed, uint32_t env_offset, int32_t* episode) {
  if (!e) return TC_E_INVALID;
  if (!e->cr.rows) {
    set_err("tc_env_set_car_randomization: no per-env car params installed (tc_env_set_car_per_env)");
    return TC_E_INVALID;
  }
  if (column_mask >> TC_CAR_NP) {
    set_err("tc_env_set_car_randomization: column mask has bits beyond TC_CAR_NP");
    return TC_E_INVALID;
  }
  const uint32_t absent = (e->k.car.has_steering_speed ? 0u : 1u << TC_CAR_STEERING_SPEED) |
                          (e->k.car.has_max_acceleration ? 0u : (1u << TC_CAR_MAX_ACCELERATION) | (1u << TC_CAR_MAX_DECELERATION));
  if (column_mask & absent) {
    set_err("tc_env_set_car_randomization: a range for a column the car does not have (steering_speed / max_acceleration)");
    return TC_E_INVALID;
  }
  if (column_mask && (!lo || !hi || !episode)) return TC_E_INVALID;
  CarDrawTab t;
  memset(&t, 0, sizeof(t));
  for (int j = 0; j < TC_CAR_NP; j++) {
    if (!((column_mask >> j) & 1u)) continue;
    if (!isfinite(lo[j]) || !isfinite(hi[j]) || lo[j] > hi[j]) {
      set_err("tc_env_set_car_randomization: every range must be finite with lo <= hi");
      return TC_E_INVALID;
    }
    t.lo[j] = lo[j];
    t.hi[j] = hi[j];
  }
  t.seed = seed;
  t.mask = column_mask;
  t.env_offset = env_offset;
  if (!e->car_tab) HIP_TRY(e->car_tab.alloc(1));
  // (in place: a graph captured earlier keeps reading this table; the copy waits for launches that may still read it)
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(e->car_tab, &t, sizeof(t), hipMemcpyHostToDevice));
  e->cr.tab = e->car_tab;
  e->cr.episode = column_mask ? episode : e->cr.episode;
  return TC_OK;
}

extern "C" int tc_env_set_episodes(tc_env* e, const tc_episode_buffers* bufs, int32_t max_episode_steps) {
  if (bufs && (!bufs->length || !bufs->ret)) {
    set_err("tc_env_set_episodes: length and ret are required");
    return TC_E_INVALID;
  }
  if (!e) return TC_E_INVALID;
  if (!bufs) {  // feature off: the per-step rows go with it
    const int* tab = e->ep_tab;
    memset(&e->ep, 0, sizeof(e->ep));
    e->ep.shared = tab;
    e->ep_rows = 0;
    return TC_OK;
  }
  if (!e->ep_tab) HIP_TRY(e->ep_tab.alloc(1));
  // (in place: a graph captured earlier keeps reading this word; the copy waits for launches that may still read it)
  const int lim = max_episode_steps > 0 ? max_episode_steps : 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(e->ep_tab, &lim, sizeof(lim), hipMemcpyHostToDevice));
  e->ep.length = bufs->length;
  e->ep.ret = bufs->ret;
  e->ep.count = bufs->count;
  e->ep.last_length = bufs->last_length;
  e->ep.last_return = bufs->last_return;
  e->ep.length_sum = (long long*)bufs->length_sum;
  e->ep.return_sum = bufs->return_sum;
  e->ep.limit = bufs->limit;
  e->ep.shared = e->ep_tab;
  return TC_OK;
}

extern "C" int tc_env_set_episode_rollout(tc_env* e, int32_t* length_rows, double* return_rows, int32_t n_rows) {
  if (n_rows < 0) {
    set_err("tc_env_set_episode_rollout: n_rows must not be negative");
    return TC_E_INVALID;
  }
  if (!e) return TC_E_INVALID;
  const bool any = length_rows || return_rows;
  if (any && !e->ep.length) {
    set_err("tc_env_set_episode_rollout: no episode buffers installed (tc_env_set_episodes)");
    return TC_E_INVALID;
  }
  if (any && n_rows < 1) {
    set_err("tc_env_set_episode_rollout: rows given with n_rows = 0");
    return TC_E_INVALID;
  }
  e->ep.len_rows = length_rows;
  e->ep.ret_rows = return_rows;
  e->ep_rows = any ? n_rows : 0;
  return TC_OK;
}

extern "C" int tc_env_set_controller(tc_env* e, const tc_controller* c) {
  if (!e) return TC_E_INVALID;
  if (!c) {  // feature off (the table stays for a graph captured earlier); the drive randomisation goes with it
    memset(&e->ct, 0, sizeof(e->ct));
    e->ctrl_rows = 0;
    memset(&e->dr, 0, sizeof(e->dr));
    e->drive_rows = 0;
    e->drive_flags = 0;
    return TC_OK;
  }
  if (c->kind != TC_CTRL_STANLEY) {
    set_err("tc_env_set_controller: unknown controller kind");
    return TC_E_INVALID;
  }
  if (!isfinite(c->k) || !isfinite(c->speed)) {
    set_err("tc_env_set_controller: k and speed must be finite");
    return TC_E_INVALID;
  }
  if (c->n_rows < 0) {
    set_err("tc_env_set_controller: n_rows must not be negative");
    return TC_E_INVALID;
  }
  if ((c->steer_noise || c->steer_rows) && c->n_rows < 1) {
    set_err("tc_env_set_controller: rows given with n_rows = 0");
    return TC_E_INVALID;
  }
  const bool fresh_tab = !e->ctrl_tab;
  if (fresh_tab) HIP_TRY(e->ctrl_tab.alloc(1));
  const CtrlTab want = {c->k, c->speed};
  if (fresh_tab || memcmp(&want, &e->ctrl_host, sizeof(want)) != 0) {  // (bitwise: -0.0 is another speed than 0.0 to atan2)
    // (in place: a graph captured earlier keeps reading this table; the copy waits for launches that may still read it.
    // A call that only changes the row pointers -- kernel arguments -- has nothing to wait for.)
    const CtrlTab t = want;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(e->ctrl_tab, &t, sizeof(t), hipMemcpyHostToDevice));
    e->ctrl_host = t;
  }
  e->ct.tab = e->ctrl_tab;
  e->ct.noise = c->steer_noise;
  e->ct.rows = c->steer_rows;
  e->ct.last = c->steer_last;
  e->ctrl_rows = (c->steer_noise || c->steer_rows) ? c->n_rows : 0;
  return TC_OK;
}

extern "C" int tc_env_set_drive_randomization(tc_env* e, const tc_drive_randomization* d) {
  if (!d) {  // feature off (the table stays for a graph captured earlier)
    if (!e) return TC_E_INVALID;
    memset(&e->dr, 0, sizeof(e->dr));
    e->drive_rows = 0;
    e->drive_flags = 0;
    return TC_OK;
  }
  // (the settings first: a bad struct is refused whatever the handle is)
  if (d->n_maneuvers < 0 || d->n_maneuvers > TC_MAX_MANEUVERS) {
    set_err("tc_env_set_drive_randomization: n_maneuvers must be in 0..8");
    return TC_E_INVALID;
  }
  for (int i = 0; i < d->n_maneuvers; i++)
    if (d->maneuvers[i] < 0 || d->maneuvers[i] > 3) {
      set_err("tc_env_set_drive_randomization: every maneuver must be in 0..3");
      return TC_E_INVALID;
    }
  if (d->maneuver_mode != TC_MAN_DRAW && d->maneuver_mode != TC_MAN_CYCLE) {
    set_err("tc_env_set_drive_randomization: unknown maneuver_mode");
    return TC_E_INVALID;
  }
  if (!isfinite(d->theta) || !isfinite(d->mu) || !isfinite(d->sigma)) {
    set_err("tc_env_set_drive_randomization: theta, mu and sigma must be finite");
    return TC_E_INVALID;
  }
  if (d->n_maneuvers > 0 && (!d->maneuver || !d->episode)) {
    set_err("tc_env_set_drive_randomization: candidates need the maneuver and episode arrays (n_maneuvers > 0)");
    return TC_E_INVALID;
  }
  if (d->ou_state && !d->ou_draws) {
    set_err("tc_env_set_drive_randomization: ou_state needs ou_draws");
    return TC_E_INVALID;
  }
  if (d->n_rows < 0) {
    set_err("tc_env_set_drive_randomization: n_rows must not be negative");
    return TC_E_INVALID;
  }
  if ((d->maneuver_rows || d->noise_rows) && d->n_rows < 1) {
    set_err("tc_env_set_drive_randomization: rows given with n_rows = 0");
    return TC_E_INVALID;
  }
  if (!e) {
    set_err("tc_env_set_drive_randomization: no env");
    return TC_E_INVALID;
  }
  if (!e->ct.tab) {
    set_err("tc_env_set_drive_randomization: no controller installed (tc_env_set_controller)");
    return TC_E_INVALID;
  }
  if (d->n_maneuvers == 0 && !d->ou_state) {  // neither part: off (no launch takes a drive entry point for nothing)
    memset(&e->dr, 0, sizeof(e->dr));
    e->drive_rows = 0;
    e->drive_flags = 0;
    return TC_OK;
  }
  DriveTab want;
  memset(&want, 0, sizeof(want));
  want.seed = d->seed;
  want.theta = d->theta;
  want.mu = d->mu;
  want.sigma = d->sigma;
  want.env_offset = d->env_offset;
  want.n_man = d->n_maneuvers;
  want.mode = d->maneuver_mode;
  want.ou_reset = d->ou_reset != 0;
  for (int i = 0; i < d->n_maneuvers; i++) want.man[i] = d->maneuvers[i];
  const bool fresh_tab = !e->drive_tab;
  if (fresh_tab) HIP_TRY(e->drive_tab.alloc(1));
  if (fresh_tab || memcmp(&want, &e->drive_host, sizeof(want)) != 0) {
    // (in place: a graph captured earlier keeps reading this table; the copy waits for launches that may still read it.
    // A call that only changes the pointers -- kernel arguments -- has nothing to wait for.)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(e->drive_tab, &want, sizeof(want), hipMemcpyHostToDevice));
    e->drive_host = want;
  }
  e->dr.tab = e->drive_tab;
  e->dr.maneuver = d->n_maneuvers > 0 ? d->maneuver : nullptr;
  e->dr.episode = d->n_maneuvers > 0 ? d->episode : nullptr;
  e->dr.ou_state = d->ou_state;
  e->dr.ou_draws = d->ou_state ? d->ou_draws : nullptr;
  e->dr.man_rows = d->maneuver_rows;
  e->dr.noise_rows = d->noise_rows;
  e->drive_rows = (d->maneuver_rows || d->noise_rows) ? d->n_rows : 0;
  e->drive_flags = (d->n_maneuvers > 0 ? TC_FI_DRIVE_MAN : 0u) | (d->ou_state ? TC_FI_DRIVE_OU : 0u);
  return TC_OK;
}

extern "C" int tc_draw_normals(uint64_t seed, uint32_t env, uint32_t first_draw, int32_t n, double* out) {
  if (n < 0 || (n > 0 && !out)) return TC_E_INVALID;
  for (int32_t i = 0; i < n; i++) out[i] = tc_normal_at(seed, env, (first_draw + (uint32_t)i) & 0x7fffffffu);
  return TC_OK;
}

extern "C" int tc_env_set_camera_per_env(tc_env* e, const double* E, const double* K) {
  if (!e || ((E == nullptr) != (K == nullptr))) return TC_E_INVALID;
  e->k.cam_E = E;
  e->k.cam_K = K;
  memset(&e->cb, 0, sizeof(e->cb));  // (static rows and a bank exclude each other: installing one removes the other)
  e->cam_count = e->cam_rows = 0;
  cover_cull(e);  // (per-env cameras: the cull is off, its cover is the shared camera's)
  return TC_OK;
}

extern "C" int tc_env_set_camera_bank(tc_env* e, const tc_camera_bank* b) {
  if (!e) return TC_E_INVALID;
  if (!b) {  // bank off: back to the shared camera (the table stays for a graph captured earlier)
    if (e->cb.index) e->k.cam_E = e->k.cam_K = nullptr;
    memset(&e->cb, 0, sizeof(e->cb));
    e->cam_count = e->cam_rows = 0;
    cover_cull(e);
    return TC_OK;
  }
  if (!b->E || !b->K || !b->index || !b->episode || b->count < 1) {
    set_err("tc_env_set_camera_bank: E, K, index and episode are required, and count must be at least 1");
    return TC_E_INVALID;
  }
  if (b->n_rows < 0 || (b->index_rows && b->n_rows < 1)) {
    set_err("tc_env_set_camera_bank: index_rows need n_rows >= 1 (and n_rows must not be negative)");
    return TC_E_INVALID;
  }
  const CamDrawTab t = {b->seed, (unsigned int)b->count, b->env_offset};
  const bool fresh_tab = !e->cam_tab;
  if (fresh_tab) HIP_TRY(e->cam_tab.alloc(1));
  if (fresh_tab || memcmp(&t, &e->cam_host, sizeof(t)) != 0) {
    // (in place: a graph captured earlier keeps reading this table; the copy waits for launches that may still read it.
    // A call that only changes pointers -- kernel arguments -- has nothing to wait for.)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(e->cam_tab, &t, sizeof(t), hipMemcpyHostToDevice));
    e->cam_host = t;
  }
  e->k.cam_E = b->E;
  e->k.cam_K = b->K;
  e->cb.index = b->index;
  e->cb.episode = b->episode;
  e->cb.tab = e->cam_tab;
  e->cb.rows = b->index_rows;
  e->cam_count = b->count;
  e->cam_rows = b->index_rows ? b->n_rows : 0;
  cover_cull(e);  // (a bank: the cull is off, as with per-env cameras)
  return TC_OK;
}

#ifdef TC_ABLATE
// ablation build only: frames that ran the whole-frame cull's test and frames it culled since the last reset
extern "C" int tc_debug_cull_counts(unsigned long long* out, int reset) {
  HIP_TRY(hipDeviceSynchronize());
  if (out) HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(tc_cull_counts), 2 * sizeof(unsigned long long)));
  const unsigned long long zero[2] = {0, 0};
  if (reset) HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(tc_cull_counts), zero, sizeof(zero)));
  return TC_OK;
}
#endif

static int noise_lds_bytes(const tc_env* e) {  // bit-planes of a band + blob rows + one span-table row per blob
  const int nb = e->k.m.C * e->noise_blobs;
  return e->k.m.C * e->k.cam.band_rows * e->k.cam.wpr * 4 + nb * 5 * 4 + align_up(nb * e->noise_max_radius, 16);
}

#ifdef TC_TIMING
// timing build only: a [n_envs][32] buffer of shader-clock stamps (see TSTAMP); read() copies it to the host
// The buffer must cover every env of every launch made while it is installed: install it BEFORE the first launch of an
// env handle and remove it (n_envs = 0) before using a larger one -- a stale smaller buffer is an out-of-bounds write.
static long long* g_tstamp = nullptr;
static int g_tstamp_n = 0;
extern "C" int tc_debug_tstamp_alloc(int n_envs) {
  HIP_TRY(hipDeviceSynchronize());
  long long* none = nullptr;
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(tc_tstamp), &none, sizeof(none)));
  if (g_tstamp) HIP_TRY(hipFree(g_tstamp));
  g_tstamp = nullptr;
  g_tstamp_n = 0;
  if (n_envs <= 0) return TC_OK;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, (size_t)n_envs * 32 * sizeof(long long)));
  HIP_TRY(hipMemset(p, 0, (size_t)n_envs * 32 * sizeof(long long)));
  g_tstamp = (long long*)p;
  g_tstamp_n = n_envs;
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(tc_tstamp), &g_tstamp, sizeof(g_tstamp)));
  return TC_OK;
}
// copies the stamps of the last launch to the host and zeroes them (a probe a wavefront skipped then reads 0)
extern "C" int tc_debug_tstamp_read(long long* out, int n_envs) {
  if (!g_tstamp || n_envs != g_tstamp_n) return TC_E_INVALID;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, g_tstamp, (size_t)n_envs * 32 * sizeof(long long), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(g_tstamp, 0, (size_t)n_envs * 32 * sizeof(long long)));
  return TC_OK;
}
#endif

extern "C" int tc_env_set_noise(tc_env* e, int32_t n_blobs, int32_t max_radius, uint64_t seed) {
  if (!e || n_blobs < 0) return TC_E_INVALID;
  if (n_blobs == 0) {
    e->noise_blobs = 0;
    return TC_OK;
  }
  if (!TC_FMT_IS_CLASSES(e->k.cam.format)) {
    set_err("tc_env_set_noise: only class-mask observations (wrapper/observation.py:7)");
    return TC_E_INVALID;
  }
  if (max_radius < 2 || max_radius > 256) {
    set_err("tc_env_set_noise: max_radius must be in [2, 256] (numpy's randint(1, max_radius) needs >= 2)");
    return TC_E_INVALID;
  }
  // Circle(center, radius, fill) of drawing.cpp run once per radius on the host: per-row half widths
  std::vector<unsigned char> hw((size_t)max_radius * max_radius, 0);
  for (int radius = 1; radius < max_radius; radius++) {
    unsigned char* row = hw.data() + (size_t)radius * max_radius;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
      if (row[dy] < dx) row[dy] = (unsigned char)dx;
      if (row[dx] < dy) row[dx] = (unsigned char)dy;
      dy++;
      err += plus;
      plus += 2;
      int mask2 = (err <= 0) - 1;
      err -= minus & mask2;
      dx += mask2;
      minus -= mask2 & 2;
    }
  }
  HIP_TRY(hipDeviceSynchronize());  // launches in flight still read the old table
  HIP_TRY(e->noise_hw.alloc(hw.size()));  // (lets the old one go first)
  HIP_TRY(hipMemcpy(e->noise_hw, hw.data(), hw.size(), hipMemcpyHostToDevice));
  e->noise_blobs = n_blobs;
  e->noise_max_radius = max_radius;
  e->noise_seed = seed;
  if (!e->noise_step) HIP_TRY(e->noise_step.alloc(1));
  HIP_TRY(hipMemset(e->noise_step, 0, sizeof(unsigned int)));
  const int lds = noise_lds_bytes(e);
  if (lds > 160 * 1024) {
    set_err("tc_env_set_noise: blob tables do not fit one workgroup's LDS");
    e->noise_blobs = 0;
    return TC_E_LDS;
  }
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)tc_noise_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  return TC_OK;
}

static int launch_noise(tc_env* e, const int32_t* blobs, void* stream, uint8_t* obs = nullptr) {
  NArgs n;
  memset(&n, 0, sizeof(n));
  const DevCam& c = e->k.cam;
  n.N = e->k.N;
  n.C = e->k.m.C;
  n.H = c.H;
  n.W = c.W;
  n.wpr = c.wpr;
  n.band_rows = c.band_rows;
  n.n_bands = c.n_bands;
  n.obs = obs ? obs : e->k.b.obs;
  n.blobs = blobs;
  n.n_blobs = e->noise_blobs;
  n.max_radius = e->noise_max_radius;
  n.hw = e->noise_hw;
  n.seed = e->noise_seed;
  n.step = e->noise_step;
  n.inv_cpr = (c.W >> 4) > 0 ? (unsigned int)((1ull << 32) / (unsigned)(c.W >> 4) + 1ull) : 0u;
  hipLaunchKernelGGL(tc_noise_kernel, dim3(n.N), dim3(TC_NT), noise_lds_bytes(e), (hipStream_t)stream, n);
  HIP_TRY(hipGetLastError());
  if (!blobs) {  // device-drawn blobs consumed one position of the stream
    hipLaunchKernelGGL(tc_noise_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, e->noise_step, 1u);
    HIP_TRY(hipGetLastError());
  }
  return TC_OK;
}

extern "C" int tc_noise(tc_env* e, const int32_t* blobs, void* stream) {
  if (!e) return TC_E_INVALID;
  if (!e->bound || !e->k.b.obs) {
    set_err("tc_noise: no observation buffer bound");
    return TC_E_UNBOUND;
  }
  if (e->noise_blobs < 1) {
    set_err("tc_noise: call tc_env_set_noise first");
    return TC_E_INVALID;
  }
  if (e->k.cam.format == TC_FMT_CLASSES_BITS) {
    set_err("tc_noise: the stand-alone pass reads byte class masks; a packed env gets its noise inside the raster stage");
    return TC_E_INVALID;
  }
  return launch_noise(e, blobs, stream);
}

extern "C" int tc_env_set_spawn_table(tc_env* e, const int32_t* nodes, int32_t n, uint64_t seed) {
  if (!e || n < 0 || (n > 0 && !nodes)) {
    set_err("tc_env_set_spawn_table: need n >= 0 and a node array");
    return TC_E_INVALID;
  }
  for (int i = 0; i < n; i++)
    if (nodes[i] < 0 || nodes[i] >= e->k.m.lpN) {
      set_err("tc_env_set_spawn_table: node id out of range");
      return TC_E_INVALID;
    }
  HIP_TRY(hipDeviceSynchronize());  // launches in flight still read the old table
  e->spawn_tab.mem.reset();
  e->k.spawn_tab = nullptr;
  e->k.spawn_n = 0;
  if (n > 0) {
    HIP_TRY(e->spawn_tab.alloc((size_t)n));
    HIP_TRY(hipMemcpy(e->spawn_tab, nodes, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    e->k.spawn_tab = e->spawn_tab;
    e->k.spawn_n = n;
  }
  e->k.spawn_seed = seed;
  return TC_OK;
}

extern "C" int tc_env_set_terms(tc_env* e, const tc_term* terms, int32_t n_terms, int32_t* counters) {
  if (!e || n_terms < 0 || n_terms > TC_MAX_TERMS || (n_terms > 0 && !terms)) {
    set_err("tc_env_set_terms: n_terms must be 0..TC_MAX_TERMS with a term array");
    return TC_E_INVALID;
  }
  const int C = e->k.m.C;
  const uint32_t all = C >= 32 ? 0xffffffffu : ((1u << C) - 1u);
  for (int t = 0; t < n_terms; t++) {
    const tc_term& T = terms[t];
    if (T.kind < TC_T_LANELINE_SPARSE_REWARD || T.kind > TC_T_CRASH_TERMINATION) {
      set_err("tc_env_set_terms: unknown term kind");
      return TC_E_INVALID;
    }
    if (T.layer_mask & ~all) {
      set_err("tc_env_set_terms: layer_mask names a layer the map does not have");
      return TC_E_INVALID;
    }
    if ((T.kind == TC_T_CTE_TERMINATION || T.kind == TC_T_CRASH_TERMINATION) && !counters) {
      set_err("tc_env_set_terms: consecutive-step terms need the counters buffer");
      return TC_E_INVALID;
    }
  }
  HIP_TRY(hipDeviceSynchronize());  // launches in flight still read the old table
  if (!e->terms) {
    HIP_TRY(e->terms.alloc(TC_MAX_TERMS));
    e->k.terms = e->terms;
  }
  if (n_terms > 0) HIP_TRY(hipMemcpy(e->terms, terms, sizeof(tc_term) * n_terms, hipMemcpyHostToDevice));
  e->k.n_terms = n_terms;
  e->k.term_counters = counters;
  e->terms_read_dist = false;  // (once here, not per call: plan_of)
  for (int t = 0; t < n_terms; t++) e->terms_read_dist = e->terms_read_dist || term_reads_distances(terms[t].kind);
  return TC_OK;
}

extern "C" int tc_env_set_camera(tc_env* e, const tc_camera_params* cam) {
  if (!e || !cam) return TC_E_INVALID;
  if (cam->height != e->k.cam.H || cam->width != e->k.cam.W || cam->format != e->k.cam.format) {
    set_err("tc_env_set_camera: resolution and format are fixed at tc_env_create");
    return TC_E_INVALID;
  }
  int band_rows = e->k.cam.band_rows, n_bands = e->k.cam.n_bands;
  int rc = fill_camera(e, cam);
  e->k.cam.band_rows = band_rows;
  e->k.cam.n_bands = n_bands;
  if (rc == TC_OK) cover_cull(e);  // (the cover travels by value with the launch arguments: no table to replace, no wait)
  return rc;
}

static RArgs make_rargs(tc_env* e, const int* seg_g, const int* seg_n, int seg_cap, const uint8_t* mask, uint32_t flags,
                        int env0, uint8_t* obs = nullptr, bool with_noise = false) {
  RArgs r;
  memset(&r, 0, sizeof(r));
  r.N = e->k.N;
  r.env0 = env0;
  r.C = e->k.m.C;
  const DevCam& c = e->k.cam;
  r.cam.H = c.H; r.cam.W = c.W; r.cam.wpr = c.wpr; r.cam.band_rows = c.band_rows; r.cam.n_bands = c.n_bands;
  r.cam.thickness = c.thickness; r.cam.format = c.format;
  {  // Circle(center, radius, fill) of drawing.cpp run once on the host: per-row half widths
    int radius = (int)((((long long)c.thickness << 15) + 32768) >> 16);
    r.cam.cap_r = radius;
    if (radius < 32) {
      int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
      while (dx >= dy) {
        if (r.cam.cap_hw[dy] < dx) r.cam.cap_hw[dy] = (unsigned char)dx;
        if (r.cam.cap_hw[dx] < dy) r.cam.cap_hw[dx] = (unsigned char)dy;
        dy++;
        err += plus;
        plus += 2;
        int mask2 = (err <= 0) - 1;
        err -= minus & mask2;
        dx += mask2;
        minus -= mask2 & 2;
      }
    }
  }
  r.cam.cap_hw4 = r.cam.cap_hw[0] | (r.cam.cap_hw[1] << 8) | (r.cam.cap_hw[2] << 16) | ((unsigned)r.cam.cap_hw[3] << 24);
  memcpy(r.colors, e->k.m.colors, sizeof(r.colors));
  for (int c = 0; c < 16; c++) r.colors_packed[c] = r.colors[c][0] | (r.colors[c][1] << 8) | ((unsigned)r.colors[c][2] << 16);
  r.seg_g = seg_g;
  r.seg_n = seg_n;
  r.seg_cap = seg_cap;
  r.obs = obs ? obs : e->k.b.obs;
  r.mask = mask;
  r.off_tab = e->r_off_tab;
  r.off_bits = e->r_off_bits;
  r.flags = flags & ~R_F_LONG_EDGES;
  if (!e->tune.short_edges && tc_short_edges_skip(c.thickness, c.W, c.H)) r.flags |= R_F_LONG_EDGES;
  r.seg_row0 = 0;
  r.noise_row0 = 0;
  r.obs_row_stride = 0;
  if (with_noise && e->noise_blobs > 0 && TC_FMT_IS_CLASSES(c.format)) {
    r.noise_blobs = e->noise_blobs;
    r.noise_max_radius = e->noise_max_radius;
    r.noise_hw = e->noise_hw;
    r.noise_seed = e->noise_seed;
    r.noise_step = e->noise_step;
  }
  return r;
}

static int check_stamp_buffer(const tc_env* e) {
#ifdef TC_TIMING
  if (g_tstamp && e->k.N > g_tstamp_n) {
    set_err("timing build: the installed stamp buffer is smaller than this env batch");
    return TC_E_INVALID;
  }
#endif
  return TC_OK;
}

static int launch_raster(tc_env* e, const int* seg_g, const int* seg_n, int seg_cap, const uint8_t* mask, uint32_t flags,
                         void* stream, int env0 = 0, int count = -1, uint8_t* obs = nullptr, bool with_noise = false) {
  int rc = check_stamp_buffer(e);
  if (rc != TC_OK) return rc;
  RArgs r = make_rargs(e, seg_g, seg_n, seg_cap, mask, flags, env0, obs, with_noise);
  if (count < 0) count = e->k.N;
  hipLaunchKernelGGL(raster_kernel_of(r.cam.thickness > 1, r.cam.format), dim3(count), dim3(TC_NT), e->r_lds, (hipStream_t)stream, r);
  HIP_TRY(hipGetLastError());
  return TC_OK;
}

static int noise_advance(tc_env* e, int mode, bool rendered, int nsteps, void* stream) {
  // the fused noise consumed one position of the blob stream per step of this launch
  if (rendered && mode == MODE_STEP && e->noise_blobs > 0 && TC_FMT_IS_CLASSES(e->k.cam.format)) {
    hipLaunchKernelGGL(tc_noise_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, e->noise_step, (unsigned int)nsteps);
    HIP_TRY(hipGetLastError());
  }
  return TC_OK;
}

// What plan_call (tc_plan.h) reads, filled from the handle and the call: for launch(), which dispatches on the plan, and for
// tc_env_launch_info, which reports it.  obs: there is a tensor to draw into (the bound one or the rollout's); all: every
// step's frame is wanted (a rollout with observations), else only the last one survives.
static CallPlan plan_of(const tc_env* e, uint32_t flags, int nsteps, bool obs, bool all, const tc_rollout* roll = nullptr) {
  const Tuning& t = e->tune;
  CallInputs in;
  in.fuse = t.fuse; in.multi_split = t.multi_split; in.env_grouped = t.env_grouped; in.pipe = t.pipe; in.stream = t.stream; in.chunk = t.chunk;
  in.kvar = e->kvar;
  in.packed = e->k.cam.format == TC_FMT_CLASSES_BITS;
  in.ring_rows = e->ring.rows; in.streamed_rows = e->streamed.rows; in.st_words = e->st_words != nullptr;
  in.flags = flags; in.no_frame_flags = TC_F_NO_OBSERVATION | DBG_SKIP_CAMERA;
  in.nsteps = nsteps; in.obs = obs; in.all = all;
  in.info_rows = roll && (roll->laneline_distances || roll->nearest_edge);
  in.info_terms = e->terms_read_dist;
  in.info_every = t.info_every;
  return plan_call(in);
}

#define TC_STREAM_MAX_ROWS 128
// Makes `s` hold `slots` x `rows` rows of N envs.  Nothing to do when it has that many rows; else the old arrays go
// (once the launches that may still use them are done) and new ones come, their contents left to the caller: *grown.
static int reserve_rows(tc_env* e, ScratchRows& s, int slots, int rows, const char* what, bool* grown) {
  *grown = false;
  if (s.rows >= rows) return TC_OK;
  HIP_TRY(hipDeviceSynchronize());
  s = ScratchRows();
  e->cost_row[0] = e->cost_row[1] = nullptr;
  const size_t R = (size_t)slots * rows * e->k.N;
  hipError_t he = s.seg_g.alloc(R * e->k.seg_cap * 5);
  if (he == hipSuccess) he = s.seg_n.alloc(R);
  if (he == hipSuccess) he = s.pose.alloc(R * TC_POSE_ROW);
  if (he != hipSuccess) {
    s = ScratchRows();
    set_err(std::string("hipMalloc(") + what + "): " + hipGetErrorString(he));
    return TC_E_NOMEM;
  }
  s.rows = rows;
  *grown = true;
  return TC_OK;
}

// scratch of streamed calls: rows for min(max_call_steps, TC_STREAM_MAX_ROWS) steps
static int reserve_stream(tc_env* e, int max_call_steps) {
  int rows = max_call_steps < TC_STREAM_MAX_ROWS ? max_call_steps : TC_STREAM_MAX_ROWS;
  // the scratch of a row is N x (pose row + draw-list length + room for a whole draw list: 20 B x lane-line edges of the
  // map -- knuffingen: 15 KB per frame); with many envs on a big map the rows are cut so that it stays within a budget
  // (tune.scratch_bytes, default 16 GiB), and a longer call runs as more, shorter segments
  const double per_row = (double)e->k.N * ((double)e->k.seg_cap * 5 * sizeof(int) + sizeof(int) + TC_POSE_ROW * sizeof(double));
  const double fit = e->tune.scratch_bytes / per_row;
  if (fit < (double)rows) rows = (int)fit;
  if (rows < 2) rows = 2;
  bool grown;
  int rc = reserve_rows(e, e->streamed, 1, rows, "scratch of streamed K-step calls", &grown);
  if (rc != TC_OK || grown) e->draw_n = 0;  // (the rows the draw-list statistics pointed into are gone)
  if (rc != TC_OK || !grown) return rc;
  const size_t R = (size_t)rows * e->k.N;
  hipError_t he = hipSuccess;
  if (!e->st_words) {
    he = e->st_words.alloc(64);
    if (he == hipSuccess) he = hipMemset(e->st_words, 0, 256);
  }
  if (he == hipSuccess) he = hipMemset(e->streamed.pose, 0xFF, R * TC_POSE_ROW * sizeof(double));  // every entry TC_POSE_EMPTY
  if (he == hipSuccess) he = hipMemset(e->streamed.seg_n, 0, R * sizeof(int));
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he != hipSuccess) {
    e->streamed = ScratchRows();
    set_err(std::string("hipMalloc(scratch of streamed K-step calls): ") + hipGetErrorString(he));
    return TC_E_NOMEM;
  }
  return TC_OK;
}

extern "C" int tc_env_reserve_steps(tc_env* e, int32_t max_call_steps) {
  if (!e || max_call_steps < 1) return TC_E_INVALID;
  if (e->tune.stream && e->tune.env_grouped && e->tune.pipe) {
    int rc = reserve_stream(e, max_call_steps);
    if (rc != TC_OK) return rc;
  }
  int rows = max_call_steps < e->tune.chunk ? max_call_steps : e->tune.chunk;
  if (rows < 2) rows = 2;  // (a pipelined call never uses chunks of fewer than 2 steps)
  bool grown;
  return reserve_rows(e, e->ring, TC_RING_SLOTS, rows, "scratch ring of K-step calls", &grown);
}

// a rollout from [step][env] row r0 on
static tc_rollout rollout_at(const tc_rollout& r, size_t r0, size_t obs_bytes, size_t C) {
  auto at = [r0](auto* p, size_t per_row) { return p ? p + r0 * per_row : p; };
  tc_rollout q;
  q.obs = at(r.obs, obs_bytes);
  q.reward = at(r.reward, 1);
  q.terminated = at(r.terminated, 1);
  q.truncated = at(r.truncated, 1);
  q.cte = at(r.cte, 1);
  q.heading_error = at(r.heading_error, 1);
  q.status = at(r.status, 1);
  q.x = at(r.x, 1);
  q.y = at(r.y, 1);
  q.theta = at(r.theta, 1);
  q.velocity = at(r.velocity, 1);
  q.laneline_distances = at(r.laneline_distances, C);
  q.nearest_edge = at(r.nearest_edge, C);
  q.local_path = at(r.local_path, 8);
  q.lp_len = at(r.lp_len, 1);
  return q;
}

// One call of launch(): its arguments and what every route needs of them.
struct Call {
  int mode;
  const void* cc;
  int cdtype;
  const int32_t *man, *spawn;
  const uint8_t* mask;
  uint32_t flags;
  hipStream_t main;  // the caller's stream
  int nsteps;
  const tc_rollout* roll;
  bool ep_rows;
  // per-env cars (tc_env_set_car_per_env) and episodes (tc_env_set_episodes): the instantiations of the simulate stages
  // with those bits, the same launches otherwise
  unsigned feat;
  bool all;  // with a rollout every step's frame is wanted; else only the last survives
  bool thick;
  int fmt;
  CallPlan plan;
  bool prof;  // the call is recorded in slot `slot` of the profile ring
  int slot;
};

// What a simulate launch is given of the CALL, for the launch whose first step is step c0 of it: the handle's arguments
// and feature rows, mode / dtype / flags, and the control, maneuver, rollout and episode rows from [step][env] row c0 * N
// on.  What belongs to the path is left to the caller: ma.nsteps and the members of ma behind it, the scratch a.seg_g /
// a.seg_n point to, r, env_order.
static StepArgs step_args_at(const tc_env* e, const Call& c, int c0) {
  const size_t r0 = (size_t)c0 * e->k.N;
  const bool ep_rows = c.ep_rows;
  StepArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.a = e->k;
  sa.a.env0 = 0;
  sa.cr = e->cr;
  sa.ep = e->ep;  // (the per-step rows belong to K-step calls only)
  sa.ep.len_rows = ep_rows && e->ep.len_rows ? e->ep.len_rows + r0 : nullptr;
  sa.ep.ret_rows = ep_rows && e->ep.ret_rows ? e->ep.ret_rows + r0 : nullptr;
  sa.ct = e->ct;  // (the per-step rows belong to K-step calls only, like the episode rows: tc_step reads and writes none)
  sa.ct.noise = ep_rows && e->ct.noise ? e->ct.noise + r0 : nullptr;
  sa.ct.rows = ep_rows && e->ct.rows ? e->ct.rows + r0 : nullptr;
  sa.cb = e->cb;  // (the index rows likewise)
  sa.cb.rows = ep_rows && e->cb.index && e->cb.rows ? e->cb.rows + r0 : nullptr;
  if (c.roll) sa.ma.roll = rollout_at(*c.roll, r0, (size_t)e->obs_bytes, (size_t)e->k.m.C);
  sa.mode = c.mode;
  sa.cdtype = c.cdtype;
  sa.dr = e->dr;  // (the rows likewise)
  sa.dr.man_rows = ep_rows && e->dr.man_rows ? e->dr.man_rows + r0 : nullptr;
  sa.dr.noise_rows = ep_rows && e->dr.noise_rows ? e->dr.noise_rows + r0 : nullptr;
  sa.flags = (c.flags & ~(TC_FI_CAM_BANK | TC_FI_DRIVE | TC_FI_INFO_EVERY)) | (e->cb.index ? TC_FI_CAM_BANK : 0u) |
             (e->dr.tab ? e->drive_flags : 0u) | (c.plan.info_every ? TC_FI_INFO_EVERY : 0u);
  sa.car_control = c.cc ? (const char*)c.cc + r0 * 2 * (c.cdtype == TC_F32 ? 4 : 8) : nullptr;  // (NULL: a controller acts)
  sa.maneuver = c.man ? c.man + r0 : nullptr;  // (NULL: the maneuvers are the device's, tc_env_set_drive_randomization)
  sa.spawn_nodes = c.spawn;
  sa.mask = c.mask;
  return sa;
}

// The argument block of a frame launch over scratch rows: of the streamed form (gated: see launch_streamed()) or of the ring.
// `gate` and `order` are the launch's own.
static FrameArgs frame_args_of(const tc_env* e, uint32_t flags, const RArgs& r, bool streamed) {
  FrameArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.a = e->k;
  fa.a.dbg = flags;
  fa.a.env0 = 0;
  const ScratchRows& s = streamed ? e->streamed : e->ring;
  fa.a.seg_g = s.seg_g;
  fa.a.seg_n = s.seg_n;
  fa.r = r;
  fa.pose_rows = s.pose;
  fa.a.seg_lds_off = fa.r.seg_lds_off = e->seg_lds_off;
  fa.a.seg_lds_cap = fa.r.seg_lds_cap = e->frame_seg_cap;
  if (streamed) {
    fa.abort_word = e->st_words + 1;
    fa.resident = e->st_words;
    fa.gate_ticks = e->tune.gate_ticks;
    fa.gate_test = e->tune.gate_test;
  }
  fa.bank = e->cb.index ? e->cam_count : 0;
  return fa;
}

// The grouped simulate launch (tc_envg_kernel: 32 envs per workgroup) of the steps `sa` describes.
static unsigned int envg_grid(int N) { return (unsigned int)((N + TC_ENVG_NT / TC_EL - 1) / (TC_ENVG_NT / TC_EL)); }
static int launch_envg(const tc_env* e, unsigned feat, StepArgs& sa, hipStream_t stream) {
  // LDS copies of the lane-line edge records (48 B per edge) and of the lanepath's fat node records (96 B per node):
  // simple_layout 12.4 + 17.5 KB, knuffingen 34.6 + 40.2 KB per workgroup of 32 envs (a CU holds one or two such
  // workgroups: 128 of them cover 4096 envs)
  const size_t map_bytes = ((size_t)e->k.m.total_edges * 48 + 15) / 16 * 16, fat_bytes = (size_t)e->k.m.lpN * sizeof(LpNode);
  sa.ma.map_lds = (e->tune.envg_map_lds && map_bytes <= 40 * 1024) ? 1 : 0;
  sa.ma.fat_lds = (e->tune.envg_map_lds && fat_bytes <= 56 * 1024) ? 1 : 0;
  hipLaunchKernelGGL(envg_kernel_of(feat), dim3(envg_grid(e->k.N)), dim3(TC_ENVG_NT),
                     (sa.ma.map_lds ? map_bytes : 0) + (sa.ma.fat_lds ? fat_bytes : 0), stream, sa);
  HIP_TRY(hipGetLastError());
  return TC_OK;
}

// Heaviest frames first on frame stream fsi (0: frame_stream, also the caller's stream of a call that is not piped; 1:
// frame_stream2).  With `sort` the permutation is rewritten on `fs` from the draw-list lengths of the last frame row
// launched on that stream, when there are a buffer and such a row.  *order: what goes into FrameArgs -- the buffer once a
// sort has run on it, else NULL (env order).
static int frame_order_of(tc_env* e, int fsi, hipStream_t fs, bool sort, const int** order) {
  const int N = e->k.N;
  if (sort && e->frame_order[fsi] && e->cost_row[fsi]) {
    hipLaunchKernelGGL(tc_order_kernel, dim3(1), dim3(TC_ORDER_NT), (size_t)(N + 15) / 16 * 16, fs, e->cost_row[fsi], N, N, e->frame_order[fsi]);
    HIP_TRY(hipGetLastError());
    e->frame_order_valid[fsi] = true;
  }
  *order = e->frame_order[fsi] && e->frame_order_valid[fsi] ? (const int*)e->frame_order[fsi] : nullptr;
  return TC_OK;
}

// Streamed form (default when every step's frame is wanted).  The chunked pipeline of launch_chunked pays for its structure: the
// first chunk's simulate launch overlaps with nothing, and every frame dispatch ends in a tail with the chip half empty
// -- a quarter of a 20-step call.  Here the whole call (or a segment of st_rows steps) is ONE simulate launch on the
// caller's stream and ONE frame launch of steps x N workgroups on the internal stream that starts right away, beside
// it: a frame workgroup polls its pose row until the simulate launch has written it (device-scope loads; every entry
// validates itself, tc_frame_kernel).  Only the first step is exposed, and there is one tail per call.
//   frame stream: [order kernel] [tc_gate_kernel: until the simulate workgroups are resident] [tc_frame_kernel, gate 1]
//                 (wait: simulate launch done) [tc_frame_recover_kernel: whatever a gate-1 workgroup gave up on]
// Every wait on the device is bounded (gate_ticks), and what a bound cuts short the recover pass completes: the
// result never depends on how the two launches were scheduled.
static int launch_streamed(tc_env* e, const Call& c) {
  const int N = e->k.N, nsteps = c.nsteps;
  const hipStream_t main = c.main, fs = e->frame_stream;
  e->draw_n = 0;
  e->draw_base = e->streamed.seg_n;
  int si = 0;
  for (int c0 = 0, cn = 0; c0 < nsteps; c0 += cn, si++) {
    cn = nsteps - c0 < c.plan.steps ? nsteps - c0 : c.plan.steps;
    // a later segment reuses the scratch rows: the frames of the one before must be drawn (and its rows cleared)
    if (si > 0) HIP_TRY(hipStreamWaitEvent(main, e->slot_ev[0], 0));
    HIP_TRY(hipEventRecord(e->start_ev, main));
    StepArgs sa = step_args_at(e, c, c0);
    sa.a.seg_g = e->streamed.seg_g;
    sa.a.seg_n = e->streamed.seg_n;
    sa.ma.nsteps = cn;
    sa.ma.seg_rows = cn > 1 ? cn : 2;
    sa.ma.pose_rows = e->streamed.pose;
    sa.ma.resident = e->st_words;
    int rc = launch_envg(e, c.feat, sa, main);
    if (rc != TC_OK) return rc;
    if (c.prof && c0 + cn >= nsteps) HIP_TRY(hipEventRecord(e->ev[1][c.slot], main));
    HIP_TRY(hipEventRecord(e->sim_ev, main));
    // ---- the frame stream
    HIP_TRY(hipStreamWaitEvent(fs, e->start_ev, 0));
    // heaviest frames first, by the last row of the call before (see the chunked form below).  Behind the wait: the
    // call before may have drawn on the CALLER's stream (a call that keeps only its last frame runs its frame kernel
    // there, reading this very permutation, behind the simulate launch that wrote the costs), so the sort that rewrites
    // the permutation in place is ordered behind everything the caller's stream did before this call -- and it belongs
    // to the capture when the call is captured into a graph.  start_ev is recorded ahead of the simulate launch, so the
    // sort still runs while that launch starts
    const int* order;
    rc = frame_order_of(e, 0, fs, true, &order);
    if (rc != TC_OK) return rc;
    RArgs r = make_rargs(e, e->streamed.seg_g, e->streamed.seg_n, e->k.seg_cap, nullptr, c.flags, 0, sa.ma.roll.obs, c.mode == MODE_STEP);
    r.seg_row0 = 0;
    r.noise_row0 = c0;
    r.obs_row_stride = (long long)N * (long long)e->obs_bytes;
    FrameArgs fa = frame_args_of(e, c.flags, r, true);
    fa.order = order;
    // (ten times the patience of a frame workgroup: one idle wavefront costs nothing, and when another env's frame
    // launch has the chip -- two handles stepping on one GPU -- the simulate workgroups only get on as that launch drains)
    hipLaunchKernelGGL(tc_gate_kernel, dim3(1), dim3(64), 0, fs, (const unsigned int*)e->st_words, envg_grid(N), 10 * e->tune.gate_ticks);
    HIP_TRY(hipGetLastError());
    if (c.prof && si == 0) HIP_TRY(hipEventRecord(e->ev[3][c.slot], fs));
    fa.gate = 1;
    hipLaunchKernelGGL(frame_kernel_of(e->kframe, c.thick, c.fmt, false), dim3(N, cn), dim3(TC_NT), e->frame_lds, fs, fa);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamWaitEvent(fs, e->sim_ev, 0));
    fa.gate = 2;
    fa.recover_rows = cn;
    fa.order = nullptr;
    hipLaunchKernelGGL(frame_kernel_of(e->kframe, c.thick, c.fmt, true), dim3(N), dim3(TC_NT), e->frame_lds, fs, fa);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->slot_ev[0], fs));
    if (e->frame_order[0]) e->cost_row[0] = e->streamed.seg_n + (size_t)(cn - 1) * N;
    const int keep = cn < 3 * 16 ? cn : 3 * 16;  // the statistics cover the same span as a chunked call's ring
    e->draw_rows[0][0] = cn - keep;
    e->draw_rows[0][1] = keep;
    e->draw_n = 1;
  }
  // join the frame stream back; the end-of-frames probe then sits on the caller's stream behind the join
  HIP_TRY(hipEventRecord(e->frames_ev, fs));
  HIP_TRY(hipStreamWaitEvent(main, e->frames_ev, 0));
  return TC_OK;
}

// K steps, split form: per chunk ONE simulate launch over its steps and ONE launch over the frames wanted.  The pose
// rows / draw lists of a chunk live in slot (chunk index mod TC_RING_SLOTS) of the scratch ring.
static int launch_chunked(tc_env* e, const Call& c) {
  const int N = e->k.N, nsteps = c.nsteps;
  const hipStream_t main = c.main;
  const bool frames = c.plan.frames, all = c.all;
  // Pipelining inside the call.  The steps are issued in chunks: the simulate launch of chunk c+1 runs on the caller's
  // stream while the frames of chunk c are produced on an internal stream (joined back before the call's work ends
  // on the caller's stream, so the caller still sees everything complete in stream order).  The two kernels suit
  // each other: the frame kernel is bound by vector issue, the grouped simulate kernel by latency (512 wavefronts
  // for 4096 envs), so the second hides in the first's shadow instead of adding its 21 us per step.
  // (Measured and dropped, DESIGN.md section 4: chunk sizes ramping up 1, 2, 4, ...; a short or half first chunk; other
  // divisors than 4 for short calls.)
  const bool piped = c.plan.piped;
  const int chunk = c.plan.steps;
  hipStream_t fs = piped ? (hipStream_t)e->frame_stream : main;
  // Short calls (chunks of fewer than 8 steps): a frame launch of 5 x N workgroups spends a good part of its life
  // ramping up and draining (5 rows: 34.6 us per row alone, 16 rows: 30.8), and a 20-step call is four of them.  There
  // the frame launches of consecutive chunks go to two streams alternately -- each still behind its own chunk's
  // simulate launch -- so that chunk c+1's workgroups fill the slots chunk c's tail leaves empty (cfg3: 8-step call
  // 66.2 -> 58.3 us per step, 20-step call 46.9 -> 44.0; with chunks of 10 steps it costs 7 %, so longer calls keep one
  // stream and their frame launches follow one another, as a kernel trace of the default command shows them).
  const bool two_fs = piped && e->tune.frame_streams == 2 && chunk < 8;
  bool first_frames = true;
  bool used_fs[2] = {false, false};
  e->draw_n = 0;
  e->draw_base = e->ring.seg_n;
  int ci = 0;
  for (int c0 = 0, cn = 0; c0 < nsteps; c0 += cn, ci++) {
    cn = nsteps - c0 < chunk ? nsteps - c0 : chunk;
    const int rslot = ci % TC_RING_SLOTS;
    const size_t rb = (size_t)rslot * e->ring.rows;   // first row of this chunk in the scratch ring
    // the frames that read this ring slot TC_RING_SLOTS chunks ago must be done before it is rewritten
    if (piped && ci >= TC_RING_SLOTS) HIP_TRY(hipStreamWaitEvent(main, e->slot_ev[rslot], 0));
    StepArgs sa = step_args_at(e, c, c0);
    sa.a.seg_g = e->ring.seg_g + rb * N * e->k.seg_cap * 5;
    sa.a.seg_n = e->ring.seg_n + rb * N;
    sa.ma.nsteps = cn;
    sa.ma.seg_rows = cn > 1 ? cn : 2;  // (> 1: row k of the chunk's lists; a one-step chunk still writes row 0 of them)
    sa.ma.cam_here = frames ? 0 : 1;
    sa.ma.pose_rows = frames ? e->ring.pose + rb * N * TC_POSE_ROW : nullptr;
    // The first chunk's simulate launch overlaps with nothing, so it should be SHORT rather than cheap: it goes through
    // the one-wavefront-per-env kernel (4096 wavefronts, bound by throughput: ~15 us per step) instead of the grouped
    // one (512 wavefronts, a latency chain: 13-23 us per step).  20-step call 48.4 -> 47.2 us per step, 128-step calls
    // 38.2 -> 37.6.  Both kernels read and leave the env's state in the caller's buffers, bit for bit the same.
    if (c.plan.grouped && !(e->tune.first_per_env && c0 == 0 && piped && nsteps > chunk)) {  // (a one-chunk call: grouped)
      int rc = launch_envg(e, c.feat, sa, main);
      if (rc != TC_OK) return rc;
    } else {
      hipLaunchKernelGGL(env_kernel_of(e->kvar, !frames, c.feat), dim3(N), dim3(TC_NT), e->k.lds.total, main, sa);
      HIP_TRY(hipGetLastError());
    }
    const bool last_chunk = c0 + cn >= nsteps;
    if (c.prof && last_chunk) HIP_TRY(hipEventRecord(e->ev[1][c.slot], main));
    if (!all && !last_chunk) continue;  // only the last step's frame is wanted
    if (two_fs) fs = (ci & 1) ? e->frame_stream2 : e->frame_stream;
    const int fsi = fs == e->frame_stream2 ? 1 : 0;
    if (piped) {
      HIP_TRY(hipEventRecord(e->sim_ev, main));
      HIP_TRY(hipStreamWaitEvent(fs, e->sim_ev, 0));
      used_fs[fsi] = true;
    }
    if (c.prof && first_frames && piped) HIP_TRY(hipEventRecord(e->ev[3][c.slot], fs));
    first_frames = false;
    RArgs r = make_rargs(e, e->ring.seg_g, e->ring.seg_n, e->k.seg_cap, nullptr, c.flags, 0, all ? sa.ma.roll.obs : nullptr, c.mode == MODE_STEP);
    // scratch row of the first frame drawn / its step index in the call (position in the blob stream)
    r.seg_row0 = (int)rb + (all ? 0 : cn - 1);
    r.noise_row0 = all ? c0 : nsteps - 1;
    r.obs_row_stride = all ? (long long)N * (long long)e->obs_bytes : 0;
    const int rows = all ? cn : 1;  // (<= ring_rows <= 16: one grid)
    if (frames) {
      FrameArgs fa = frame_args_of(e, c.flags, r, false);
      // Heaviest frames first.  A dispatch ends with a tail -- the chip half empty while the last workgroups finish, ~36 us
      // of a 16-step dispatch, a fifth of a 5-step one -- and the dispatcher hands workgroups out in index order, so the
      // envs are sorted by the draw-list lengths of the last frame row drawn on this stream (tc_order_kernel with one
      // group: plain descending order): the last workgroups to start are then the cheap, mostly empty frames.
      // (a re-sort costs ~5 us of the frame stream -- kernel + launch -- so short dispatches, whose tails already overlap on
      // two streams, re-sort only once per call and otherwise keep the stream's last order)
      int rc = frame_order_of(e, fsi, fs, rows >= 8 || ci < 2, &fa.order);
      if (rc != TC_OK) return rc;
      hipLaunchKernelGGL(frame_kernel_of(e->kframe, c.thick, c.fmt, false), dim3(N, rows), dim3(TC_NT), e->frame_lds, fs, fa);
      if (e->frame_order[fsi]) e->cost_row[fsi] = e->ring.seg_n + ((size_t)r.seg_row0 + (size_t)rows - 1) * N;
    } else {
      hipLaunchKernelGGL(raster_kernel_of(c.thick, c.fmt), dim3(N, rows), dim3(TC_NT), e->r_lds, fs, r);
    }
    HIP_TRY(hipGetLastError());
    if (piped) HIP_TRY(hipEventRecord(e->slot_ev[rslot], fs));
    {  // (the ring keeps the last TC_RING_SLOTS chunks: remember where their draw-list lengths are)
      const int w = e->draw_n < TC_RING_SLOTS ? e->draw_n++ : (memmove(e->draw_rows[0], e->draw_rows[1], sizeof(int) * 2 * (TC_RING_SLOTS - 1)), TC_RING_SLOTS - 1);
      e->draw_rows[w][0] = r.seg_row0;
      e->draw_rows[w][1] = rows;
    }
  }
  // join the frame stream(s) back; the end-of-frames probe then sits on the caller's stream behind the join
  if (used_fs[0]) {
    HIP_TRY(hipEventRecord(e->frames_ev, e->frame_stream));
    HIP_TRY(hipStreamWaitEvent(main, e->frames_ev, 0));
  }
  if (used_fs[1]) {
    HIP_TRY(hipEventRecord(e->frames_ev2, e->frame_stream2));
    HIP_TRY(hipStreamWaitEvent(main, e->frames_ev2, 0));
  }
  return TC_OK;
}

// one launch: simulate + raster by the same wavefront
static int launch_fused(tc_env* e, const Call& c) {
  const int N = e->k.N;
  StepArgs sa = step_args_at(e, c, 0);
  sa.ma.nsteps = c.nsteps;
  // (component groups that fit the K = 5 register cache: the K = 5 kernel with 16-segment batches, as for the frame kernel --
  // its simulate stage then walks the map's lane-line nodes in windows of 320 instead of 576)
  assert(c.fmt != TC_FMT_CLASSES_BITS);  // (plan_call)
  step_kern_t fk = step_kernel_of(e->kframe == 516 ? 516 : e->kvar, c.thick, c.fmt, c.feat);
  sa.r = make_rargs(e, e->k.seg_g, e->k.seg_n, e->k.seg_cap, nullptr, c.flags, 0, nullptr, c.mode == MODE_STEP);
  // covers both stages and the parked state; behind it, up to the size that costs the CU no workgroup, the head of the
  // frame's draw list (see tc_env_create)
  const int lds = e->step_lds;
  sa.a.seg_lds_off = sa.r.seg_lds_off = e->k.lds.total;
  sa.a.seg_lds_cap = sa.r.seg_lds_cap = e->seg_lds_cap ? (e->step_lds - e->k.lds.total) / 20 : 0;
  if (sa.a.seg_lds_cap > e->tune.seg_lds_limit) sa.a.seg_lds_cap = sa.r.seg_lds_cap = e->tune.seg_lds_limit;
  if (e->env_order && c.nsteps == 1) {
    // every order_every-th step the envs are re-dealt to the workgroups by the draw-list lengths of the step before
    // (tc_order_kernel: a 1-workgroup launch of a few microseconds on the caller's stream)
    if (c.mode == MODE_STEP && e->order_calls++ % e->tune.order_every == 0 && e->order_calls > 1) {
      hipLaunchKernelGGL(tc_order_kernel, dim3(1), dim3(TC_ORDER_NT), (size_t)(N + 15) / 16 * 16, c.main, (const int*)e->k.seg_n, N, e->order_g, e->env_order);
      HIP_TRY(hipGetLastError());
    }
    sa.env_order = e->env_order;
  }
  hipLaunchKernelGGL(fk, dim3(N), dim3(TC_NT), lds, c.main, sa);
  HIP_TRY(hipGetLastError());
  e->draw_n = -1;
  // one kernel: its whole duration is reported as the first interval, the second is empty
  if (c.prof) HIP_TRY(hipEventRecord(e->ev[1][c.slot], c.main));
  return TC_OK;
}

// one tc_env_kernel launch, and a tc_raster_kernel launch behind it when frames are drawn
static int launch_two(tc_env* e, const Call& c) {
  const int N = e->k.N;
  const bool do_raster = c.plan.do_raster;
  StepArgs sa = step_args_at(e, c, 0);
  sa.ma.nsteps = c.nsteps;
  sa.ma.cam_here = do_raster ? 1 : 0;
  // (K steps without observations run on the one-wavefront-per-env kernel: with nothing to share the chip with, its
  // shorter serial chain wins -- cfg2: 16.5 us per step against 20.7 for the grouped kernel)
  hipLaunchKernelGGL(env_kernel_of(e->kvar, do_raster, c.feat), dim3(N), dim3(TC_NT), e->k.lds.total, c.main, sa);
  HIP_TRY(hipGetLastError());
  if (c.prof) HIP_TRY(hipEventRecord(e->ev[1][c.slot], c.main));
  if (do_raster) {
    int rc = launch_raster(e, e->k.seg_g, e->k.seg_n, e->k.seg_cap, c.mode == MODE_RESET ? c.mask : nullptr, c.flags, c.main, 0, N,
                           c.roll ? c.roll->obs : nullptr, c.mode == MODE_STEP);
    if (rc != TC_OK) return rc;
    e->draw_n = -1;
  }
  return TC_OK;
}

static int launch(tc_env* e, int mode, const void* cc, int cdtype, const int32_t* man, const int32_t* spawn,
                  const uint8_t* mask, uint32_t flags, void* stream, int nsteps = 1, const tc_rollout* roll = nullptr,
                  bool ep_rows = false) {
  if (!e) return TC_E_INVALID;
  if (!e->bound) {
    set_err("tc_env_bind has not been called");
    return TC_E_UNBOUND;
  }
  if ((flags & TC_F_AUTORESET) && !e->k.b.needs_reset) {
    set_err("TC_F_AUTORESET needs needs_reset/spawn_queue/spawn_cursor buffers");
    return TC_E_INVALID;
  }
  if ((flags & TC_F_DEVICE_SPAWN) && e->k.spawn_n < 1) {
    set_err("TC_F_DEVICE_SPAWN needs a table (tc_env_set_spawn_table)");
    return TC_E_INVALID;
  }
  int rc = check_stamp_buffer(e);
  if (rc != TC_OK) return rc;
  const unsigned feat = (e->cr.rows ? TC_FEAT_CAR : 0u) | (e->ep.length && mode != MODE_RENDER ? TC_FEAT_EP : 0u) |
                        (e->ct.tab && (mode == MODE_STEP || (mode == MODE_RESET && e->dr.tab)) ? TC_FEAT_CTRL : 0u);
  // (the controller: the tc_drive_* entry points; a tc_reset takes them too while the drive randomisation is on: the
  // re-spawn draws the episode's maneuver)
  Call c;  // (filled by name: the order of the fields is free to change)
  c.mode = mode; c.cc = cc; c.cdtype = cdtype; c.man = man; c.spawn = spawn; c.mask = mask; c.flags = flags;
  c.main = (hipStream_t)stream; c.nsteps = nsteps; c.roll = roll; c.ep_rows = ep_rows; c.feat = feat;
  c.all = roll && roll->obs;
  c.thick = e->k.cam.thickness > 1; c.fmt = e->k.cam.format;
  c.plan = plan_of(e, flags, nsteps, e->k.b.obs || c.all, c.all, roll);
  c.prof = e->prof > 0 && mode == MODE_STEP && (e->prof_calls++ % e->prof) == 0;
  c.slot = e->prof_n % TC_PROF_RING;
  if (c.plan.split && e->ring.rows < 1) {
    set_err("tc_step_multi with observations needs the scratch ring: call tc_env_reserve_steps(env, n) once before "
            "(tc_step_multi itself never allocates)");
    return TC_E_INVALID;
  }
  // ---- begin
  if (c.prof) HIP_TRY(hipEventRecord(e->ev[0][c.slot], c.main));
  // one stream at a time per handle: a K-step call on another stream than the previous K-step call waits for that call.
  // A K-step call that is not split (no observations, one fused launch, two launches) keeps the promise of the split form:
  // on another stream than the handle's previous K-step call it waits for that call, and it is the next call's predecessor
  if (nsteps > 1 && e->have_call && e->last_stream != c.main) HIP_TRY(hipStreamWaitEvent(c.main, e->call_ev, 0));
  rc = c.plan.streamed ? launch_streamed(e, c) : c.plan.split ? launch_chunked(e, c) : c.plan.fused ? launch_fused(e, c) : launch_two(e, c);
  if (rc != TC_OK) return rc;
  // ---- end
  if (c.prof) {
    HIP_TRY(hipEventRecord(e->ev[2][c.slot], c.main));
    e->prof_piped[c.slot] = c.plan.piped ? 1 : 0;  // (every route: a slot reused by another form must not keep the old flag)
    e->prof_n++;
  }
  rc = noise_advance(e, mode, c.plan.do_raster, nsteps, stream);
  if (rc != TC_OK || nsteps < 2) return rc;
  HIP_TRY(hipEventRecord(e->call_ev, c.main));
  e->last_stream = c.main;
  e->have_call = true;
  return TC_OK;
}

extern "C" int tc_reset(tc_env* e, const int32_t* spawn_nodes, const uint8_t* mask, uint32_t flags, void* stream) {
  if (!spawn_nodes) return TC_E_INVALID;
  return launch(e, MODE_RESET, nullptr, TC_F32, nullptr, spawn_nodes, mask, flags, stream);
}

extern "C" int tc_step(tc_env* e, const void* car_control, int32_t control_dtype, const int32_t* maneuver,
                       uint32_t flags, void* stream) {
  if (control_dtype != TC_F32 && control_dtype != TC_F64) return TC_E_INVALID;
  if (!maneuver && !(e && e->dr.tab && (e->drive_flags & TC_FI_DRIVE_MAN))) return TC_E_INVALID;  // (device maneuvers replace it)
  if (!car_control && !(e && e->ct.tab)) return TC_E_INVALID;  // (a built-in controller replaces the action)
  return launch(e, MODE_STEP, car_control, control_dtype, maneuver, nullptr, nullptr, flags, stream);
}

extern "C" int tc_step_multi(tc_env* e, const void* car_control, int32_t control_dtype, const int32_t* maneuver,
                             int32_t n_steps, uint32_t flags, const tc_rollout* rollout, void* stream) {
  if (!e || (control_dtype != TC_F32 && control_dtype != TC_F64) || n_steps < 1) return TC_E_INVALID;
  if (!maneuver && !(e->dr.tab && (e->drive_flags & TC_FI_DRIVE_MAN))) return TC_E_INVALID;  // (device maneuvers replace it)
  if (!car_control && !e->ct.tab) return TC_E_INVALID;  // (a built-in controller replaces the action)
  // (not left to launch(): the row checks below would answer first for an unbound handle whose rows are too short)
  if (!e->bound) {
    set_err("tc_env_bind has not been called");
    return TC_E_UNBOUND;
  }
  if (e->ct.tab && (e->ct.noise || e->ct.rows) && n_steps > e->ctrl_rows) {
    set_err("tc_step_multi: more steps than the controller's rows hold (tc_env_set_controller)");
    return TC_E_INVALID;
  }
  if (e->dr.tab && (e->dr.man_rows || e->dr.noise_rows) && n_steps > e->drive_rows) {
    set_err("tc_step_multi: more steps than the drive randomisation's rows hold (tc_env_set_drive_randomization)");
    return TC_E_INVALID;
  }
  if (e->cb.index && e->cb.rows && n_steps > e->cam_rows) {
    set_err("tc_step_multi: more steps than the camera index rows hold (tc_env_set_camera_bank)");
    return TC_E_INVALID;
  }
  if ((e->ep.len_rows || e->ep.ret_rows) && n_steps > e->ep_rows) {
    set_err("tc_step_multi: more steps than the episode rows hold (tc_env_set_episode_rollout)");
    return TC_E_INVALID;
  }
  return launch(e, MODE_STEP, car_control, control_dtype, maneuver, nullptr, nullptr, flags, stream, n_steps, rollout, true);
}

// Workload descriptor for benchmark lines: what the most recent frames actually drew.  Waits for the device and copies
// the draw-list lengths (one int per frame) to the host: of the last single step's N frames, or of the frames of the
// last (up to TC_RING_SLOTS) chunks of the last K-step call.
extern "C" int tc_env_draw_list_stats(tc_env* e, double* mean_segments, double* empty_frac, int32_t* max_segments,
                                      int64_t* frames) {
  if (!e || !mean_segments || !empty_frac || !max_segments || !frames) return TC_E_INVALID;
  *mean_segments = *empty_frac = 0;
  *max_segments = 0;
  *frames = 0;
  if (e->draw_n == 0) return TC_OK;
  HIP_TRY(hipDeviceSynchronize());
  const int N = e->k.N;
  std::vector<int> h;
  long long tot = 0, empty = 0, cnt = 0;
  int mx = 0;
  auto take = [&](const int* dev, size_t n) -> int {
    h.resize(n);
    HIP_TRY(hipMemcpy(h.data(), dev, n * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
      tot += h[i];
      empty += h[i] == 0;
      mx = h[i] > mx ? h[i] : mx;
    }
    cnt += (long long)n;
    return TC_OK;
  };
  if (e->draw_n < 0) {
    int rc = take(e->k.seg_n, (size_t)N);
    if (rc != TC_OK) return rc;
  } else {
    for (int i = 0; i < e->draw_n; i++) {
      int rc = take(e->draw_base + (size_t)e->draw_rows[i][0] * N, (size_t)e->draw_rows[i][1] * N);
      if (rc != TC_OK) return rc;
    }
  }
  *frames = cnt;
  *mean_segments = cnt ? (double)tot / (double)cnt : 0.0;
  *empty_frac = cnt ? (double)empty / (double)cnt : 0.0;
  *max_segments = mx;
  return TC_OK;
}

extern "C" int tc_env_launch_info(const tc_env* e, uint32_t flags, int32_t n_steps, int32_t* fused, int32_t* kvar,
                                  int32_t* steps_per_dispatch, char* name, int32_t name_cap) {
  if (!e) return TC_E_INVALID;
  const CallPlan p = plan_of(e, flags, n_steps, e->k.b.obs != nullptr, true);  // (every frame wanted)
  if (fused) *fused = p.fused ? 1 : 0;
  if (kvar) *kvar = (p.fused && e->kframe == 516) ? 5 : e->kvar;  // (the fused kernel of a map with component groups: K = 5)
  if (steps_per_dispatch) *steps_per_dispatch = p.steps;
  const bool drive = e->ct.tab != nullptr;  // (a controller is installed: the tc_drive_* entry points)
  if (name && name_cap > 0)
    snprintf(name, (size_t)name_cap, "%s",
             p.fused ? (drive ? "tc_drive_step_kernel" : "tc_step_kernel")
             : p.grouped ? (drive ? "tc_drive_envg_kernel+tc_frame_kernel" : "tc_envg_kernel+tc_frame_kernel")
             : p.frames  ? (drive ? "tc_drive_env_kernel+tc_frame_kernel" : "tc_env_kernel+tc_frame_kernel")
             : p.do_raster ? (drive ? "tc_drive_env_kernel+tc_raster_kernel" : "tc_env_kernel+tc_raster_kernel")
                           : (drive ? "tc_drive_env_kernel" : "tc_env_kernel"));
  return TC_OK;
}

extern "C" int tc_render_segments(tc_env* e, const int32_t* segments, const int32_t* counts, int32_t capacity,
                                  void* stream) {
  if (!e || !segments || !counts || capacity < 1) return TC_E_INVALID;
  if (!e->bound || !e->k.b.obs) {
    set_err("tc_render_segments needs bound buffers with an observation tensor");
    return TC_E_UNBOUND;
  }
  return launch_raster(e, segments, counts, capacity, nullptr, 0, stream);
}

extern "C" int tc_render(tc_env* e, uint32_t flags, void* stream) {
  return launch(e, MODE_RENDER, nullptr, TC_F32, nullptr, nullptr, nullptr, flags & ~TC_F_NO_OBSERVATION, stream);
}

extern "C" int tc_unpack_bits(const uint8_t* packed, int64_t n_src_frames, int32_t planes, int32_t H, int32_t W,
                              const int64_t* index, int64_t n_out, void* dst, int32_t dst_dtype, void* stream) {
  // (every check comes before the first HIP call: a bad argument is reported on a machine without a device too)
  if (!packed || !dst || n_src_frames < 1 || planes < 1 || H < 1 || W < 1 || W % 32 != 0 || n_out < 0 ||
      (!index && n_out > n_src_frames) ||
      (dst_dtype != TC_U8 && dst_dtype != TC_F16 && dst_dtype != TC_BF16 && dst_dtype != TC_F32)) {
    set_err("tc_unpack_bits: need packed and dst, positive sizes, W % 32 == 0, dst_dtype TC_U8|TC_F16|TC_BF16|TC_F32, "
            "n_out >= 0, and n_out <= n_src_frames without an index");
    return TC_E_INVALID;
  }
  if (((uintptr_t)packed & 3u) || ((uintptr_t)dst & 15u)) {
    set_err("tc_unpack_bits: packed must be 4-byte aligned and dst 16-byte aligned");
    return TC_E_INVALID;
  }
  if (n_out == 0) return TC_OK;
  const long long frame_words = (long long)planes * H * (W / 32);
  const int per_word = dst_dtype == TC_U8 ? 2 : dst_dtype == TC_F32 ? 8 : 4;  // 16-byte stores per packed word
  const long long chunks = (frame_words * per_word + 255) / 256;
  // enough workgroups to fill the device several times over, each with several stores in flight per lane
  const unsigned int gx = (unsigned int)(chunks < 64 ? chunks : (chunks + 3) / 4 < 64 ? 64 : (chunks + 3) / 4 < 1024 ? (chunks + 3) / 4 : 1024);
  const long long want_y = (32768 + gx - 1) / gx;
  const unsigned int gy = (unsigned int)(n_out < want_y ? n_out : want_y);
  const dim3 grid(gx, gy), block(256);
  const unsigned int* src = (const unsigned int*)packed;
  const long long* idx = (const long long*)index;
  hipStream_t st = (hipStream_t)stream;
  switch (dst_dtype) {
    case TC_U8: hipLaunchKernelGGL(tc_unpack_bits_kernel<TC_U8>, grid, block, 0, st, src, (long long)n_src_frames, frame_words, idx, (long long)n_out, (uint4*)dst); break;
    case TC_F16: hipLaunchKernelGGL(tc_unpack_bits_kernel<TC_F16>, grid, block, 0, st, src, (long long)n_src_frames, frame_words, idx, (long long)n_out, (uint4*)dst); break;
    case TC_BF16: hipLaunchKernelGGL(tc_unpack_bits_kernel<TC_BF16>, grid, block, 0, st, src, (long long)n_src_frames, frame_words, idx, (long long)n_out, (uint4*)dst); break;
    default: hipLaunchKernelGGL(tc_unpack_bits_kernel<TC_F32>, grid, block, 0, st, src, (long long)n_src_frames, frame_words, idx, (long long)n_out, (uint4*)dst); break;
  }
  HIP_TRY(hipGetLastError());
  return TC_OK;
}

extern "C" int64_t tc_collect_scratch_bytes(int32_t n_rows, int32_t num_envs) { return tc_collect_scratch_size(n_rows, num_envs); }

extern "C" int tc_collect(const tc_collect_desc* d, int32_t n_rows, const uint8_t* obs_rows, const uint8_t* terminated,
                          const uint8_t* truncated, void* stream) {
  // (every check comes before the first HIP call: a bad argument is reported on a machine without a device too)
  auto bad = [](const char* what) {
    set_err(std::string("tc_collect: ") + what);
    return TC_E_INVALID;
  };
  auto mis = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
  if (!d) return bad("NULL descriptor");
  if (!obs_rows || !d->obs || !d->ordinal || !d->env || !d->pending || !d->age || !d->last || !d->counters || !d->scratch)
    return bad("obs_rows, obs, ordinal, env, pending, age, last, counters and scratch are required");
  if (n_rows < 1 || d->capacity < 1 || d->num_envs < 1 || d->frame_bytes < 1) return bad("n_rows, capacity, num_envs and frame_bytes must be positive");
  // (tc_collect_copy runs one wavefront per (row, env): 2^26 pairs would be a grid of 2^32 threads, which a launch refuses --
  // and by then the scan and rank launches would have moved the carry and the counters)
  if ((int64_t)n_rows * d->num_envs >= (1ll << 26)) return bad("n_rows * num_envs must be below 2^26");
  if (d->stride < 1) return bad("stride must be at least 1");
  if (d->frame_bytes % 4 != 0) return bad("frame_bytes must be a multiple of 4");
  if (d->mode != TC_COLLECT_STOP && d->mode != TC_COLLECT_RING && d->mode != TC_COLLECT_RANDOM) return bad("unknown mode");
  if (d->mode == TC_COLLECT_RANDOM && d->capacity >= (1ll << 32)) return bad("TC_COLLECT_RANDOM needs capacity < 2^32");
  if (d->n_columns < 0 || d->n_columns > TC_COLLECT_MAX_COLUMNS) return bad("at most TC_COLLECT_MAX_COLUMNS columns");
  for (int j = 0; j < d->n_columns; j++) {
    const tc_collect_column& c = d->columns[j];
    if (c.elem_size != 1 && c.elem_size != 4 && c.elem_size != 8) return bad("a column's element size must be 1, 4 or 8");
    if (!c.src || !c.dst) return bad("a column needs src and dst");
    if (mis(c.src, (uintptr_t)c.elem_size) || mis(c.dst, (uintptr_t)c.elem_size)) return bad("a column's src and dst must be aligned to its element size");
  }
  if (mis(obs_rows, 4) || mis(d->obs, 4) || mis(d->last, 4) || (d->next_obs && mis(d->next_obs, 4))) return bad("frames must be 4-byte aligned");
  if (mis(d->ordinal, 8) || mis(d->counters, 8) || mis(d->env, 4) || mis(d->age, 4) || mis(d->scratch, 16))
    return bad("ordinal and counters must be 8-byte, env and age 4-byte, scratch 16-byte aligned");
  if (d->scratch_bytes < tc_collect_scratch_size(n_rows, d->num_envs)) return bad("scratch is too small (tc_collect_scratch_bytes)");
  CollectArgs a;
  a.d = *d;
  a.rows = n_rows;
  a.waves = (int)tc_collect_waves(d->num_envs);
  a.vec16 = d->frame_bytes % 16 == 0 && !mis(obs_rows, 16) && !mis(d->obs, 16) && !mis(d->last, 16) && !(d->next_obs && mis(d->next_obs, 16));
  a.obs_rows = obs_rows;
  a.terminated = terminated;
  a.truncated = truncated;
  const size_t cells = (size_t)n_rows * a.waves;
  a.head = (long long*)d->scratch;
  a.mask = (unsigned long long*)((char*)d->scratch + 16);
  a.base = (int*)((char*)d->scratch + 16 + cells * 8);
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(TC_COLLECT_NT);
  const long long pairs = (long long)n_rows * d->num_envs;
  hipLaunchKernelGGL(tc_collect_scan, dim3((unsigned)((d->num_envs + TC_COLLECT_NT - 1) / TC_COLLECT_NT)), block, 0, st, a);
  hipLaunchKernelGGL(tc_collect_rank, dim3(1), block, 0, st, a);
  if (d->mode == TC_COLLECT_RANDOM)
    hipLaunchKernelGGL(tc_collect_claim, dim3((unsigned)((pairs + TC_COLLECT_NT - 1) / TC_COLLECT_NT)), block, 0, st, a);
  hipLaunchKernelGGL(tc_collect_copy, dim3((unsigned)((pairs + TC_COLLECT_NT / 64 - 1) / (TC_COLLECT_NT / 64))), block, 0, st, a);  // one wavefront per (row, env)
  HIP_TRY(hipGetLastError());
  return TC_OK;
}

extern "C" int tc_collect_link(const tc_collect_desc* d, int32_t n_rows, const uint8_t* terminated, const uint8_t* truncated,
                               int64_t* chain, int64_t* link_rows, void* stream) {
  // (every check comes before the first HIP call; the fields tc_collect alone uses are its business)
  auto bad = [](const char* what) {
    set_err(std::string("tc_collect_link: ") + what);
    return TC_E_INVALID;
  };
  auto mis = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
  if (!d) return bad("NULL descriptor");
  if (!d->pending || !d->age || !d->counters || !d->scratch || !chain || !link_rows)
    return bad("pending, age, counters, scratch, chain and link_rows are required");
  if (n_rows < 1 || d->capacity < 1 || d->num_envs < 1) return bad("n_rows, capacity and num_envs must be positive");
  if ((int64_t)n_rows * d->num_envs >= (1ll << 26)) return bad("n_rows * num_envs must be below 2^26");
  if (d->stride < 1) return bad("stride must be at least 1");
  if (mis(d->counters, 8) || mis(d->age, 4) || mis(d->scratch, 16) || mis(chain, 8) || mis(link_rows, 8))
    return bad("counters, chain and link_rows must be 8-byte, age 4-byte, scratch 16-byte aligned");
  if (d->scratch_bytes < tc_collect_scratch_size(n_rows, d->num_envs)) return bad("scratch is too small (tc_collect_scratch_bytes)");
  CollectArgs a;
  a.d = *d;
  a.rows = n_rows;
  a.waves = (int)tc_collect_waves(d->num_envs);
  a.vec16 = 0;
  a.obs_rows = nullptr;
  a.terminated = terminated;
  a.truncated = truncated;
  const size_t cells = (size_t)n_rows * a.waves;
  a.head = (long long*)d->scratch;
  a.mask = (unsigned long long*)((char*)d->scratch + 16);
  a.base = (int*)((char*)d->scratch + 16 + cells * 8);
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(TC_COLLECT_NT), envs((unsigned)((d->num_envs + TC_COLLECT_NT - 1) / TC_COLLECT_NT));
  hipLaunchKernelGGL(tc_collect_link_scan, envs, block, 0, st, a);
  hipLaunchKernelGGL(tc_collect_link_rank, dim3(1), block, 0, st, a);
  hipLaunchKernelGGL(tc_collect_link_walk, envs, block, 0, st, a, (long long*)chain, (long long*)link_rows);
  HIP_TRY(hipGetLastError());
  return TC_OK;
}

extern "C" int tc_history_resolve(const int64_t* prev, const int64_t* ordinal, int64_t capacity, int32_t mode, uint64_t seed,
                                  const int64_t* index, int64_t n_index, int32_t T, int32_t pad, int64_t* slots,
                                  int64_t* next_slots, int32_t* valid, void* stream) {
  auto bad = [](const char* what) {
    set_err(std::string("tc_history_resolve: ") + what);
    return TC_E_INVALID;
  };
  auto mis = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
  if (!prev || !ordinal || !index || !slots || !valid) return bad("prev, ordinal, index, slots and valid are required");
  if (capacity < 1 || T < 1 || n_index < 0) return bad("capacity and T must be positive, n_index not negative");
  if (n_index >= (1ll << 31) * TC_HISTORY_NT) return bad("n_index is too large for one launch");
  if (mode != TC_COLLECT_STOP && mode != TC_COLLECT_RING && mode != TC_COLLECT_RANDOM) return bad("unknown mode");
  if (mode == TC_COLLECT_RANDOM && capacity >= (1ll << 32)) return bad("TC_COLLECT_RANDOM needs capacity < 2^32");
  if (pad != TC_PAD_ZERO && pad != TC_PAD_EDGE) return bad("pad must be TC_PAD_ZERO or TC_PAD_EDGE");
  if (mis(prev, 8) || mis(ordinal, 8) || mis(index, 8) || mis(slots, 8) || mis(next_slots, 8) || mis(valid, 4))
    return bad("prev, ordinal, index, slots and next_slots must be 8-byte, valid 4-byte aligned");
  if (n_index == 0) return TC_OK;
  ResolveArgs a;
  a.prev = (const long long*)prev;
  a.ordinal = (const long long*)ordinal;
  a.capacity = capacity;
  a.mode = mode;
  a.T = T;
  a.pad = pad;
  a.seed = seed;
  a.index = (const long long*)index;
  a.n_index = n_index;
  a.slots = (long long*)slots;
  a.next_slots = (long long*)next_slots;
  a.valid = valid;
  hipLaunchKernelGGL(tc_history_resolve_walk, dim3((unsigned)((n_index + TC_HISTORY_NT - 1) / TC_HISTORY_NT)), dim3(TC_HISTORY_NT), 0,
                     (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return TC_OK;
}

template <int DT>
static void launch_gather(bool wide, dim3 grid, hipStream_t st, const uint8_t* src, const uint8_t* src2, int64_t n_src, int64_t F,
                          const int64_t* index, int64_t n_out, int64_t group, void* dst) {
  constexpr int V = DT == TC_U8 ? 16 : DT == TC_F32 ? 4 : 8;  // source bytes of one 16-byte store
  if (wide)
    hipLaunchKernelGGL((tc_gather_frames_k<DT, V>), grid, dim3(TC_HISTORY_NT), 0, st, src, src2, (long long)n_src, (long long)F,
                       (const long long*)index, (long long)n_out, (long long)group, (unsigned char*)dst);
  else
    hipLaunchKernelGGL((tc_gather_frames_k<DT, 4>), grid, dim3(TC_HISTORY_NT), 0, st, src, src2, (long long)n_src, (long long)F,
                       (const long long*)index, (long long)n_out, (long long)group, (unsigned char*)dst);
}

extern "C" int tc_gather_frames(const uint8_t* src, const uint8_t* src2, int64_t n_src_frames, int64_t frame_bytes,
                                const int64_t* index, int64_t n_out, int64_t group, void* dst, int32_t dst_dtype, void* stream) {
  auto bad = [](const char* what) {
    set_err(std::string("tc_gather_frames: ") + what);
    return TC_E_INVALID;
  };
  auto mis = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
  if (!src || !index || !dst) return bad("src, index and dst are required");
  if (n_src_frames < 1 || frame_bytes < 1 || n_out < 0) return bad("n_src_frames and frame_bytes must be positive, n_out not negative");
  if (frame_bytes % 4 != 0) return bad("frame_bytes must be a multiple of 4");
  if (src2 && group < 1) return bad("group must be at least 1 with a second source");
  if (dst_dtype != TC_U8 && dst_dtype != TC_F16 && dst_dtype != TC_BF16 && dst_dtype != TC_F32)
    return bad("dst_dtype must be TC_U8, TC_F16, TC_BF16 or TC_F32");
  if (mis(src, 4) || mis(src2, 4) || mis(index, 8) || mis(dst, 16)) return bad("src and src2 must be 4-byte, index 8-byte, dst 16-byte aligned");
  if (n_out == 0) return TC_OK;
  const int V = dst_dtype == TC_U8 ? 16 : dst_dtype == TC_F32 ? 4 : 8;
  const bool wide = frame_bytes % V == 0 && !mis(src, (uintptr_t)V) && !mis(src2, (uintptr_t)V);
  const long long chunks = (frame_bytes / (wide ? V : 4) + TC_HISTORY_NT - 1) / TC_HISTORY_NT;
  // (as tc_unpack_bits: enough workgroups to fill the device several times over, several stores in flight per lane)
  const unsigned int gx = (unsigned int)(chunks < 64 ? chunks : (chunks + 3) / 4 < 64 ? 64 : (chunks + 3) / 4 < 1024 ? (chunks + 3) / 4 : 1024);
  const long long want_y = (32768 + gx - 1) / gx;
  const dim3 grid(gx, (unsigned int)(n_out < want_y ? n_out : want_y));
  hipStream_t st = (hipStream_t)stream;
  switch (dst_dtype) {
    case TC_U8: launch_gather<TC_U8>(wide, grid, st, src, src2, n_src_frames, frame_bytes, index, n_out, group, dst); break;
    case TC_F16: launch_gather<TC_F16>(wide, grid, st, src, src2, n_src_frames, frame_bytes, index, n_out, group, dst); break;
    case TC_BF16: launch_gather<TC_BF16>(wide, grid, st, src, src2, n_src_frames, frame_bytes, index, n_out, group, dst); break;
    default: launch_gather<TC_F32>(wide, grid, st, src, src2, n_src_frames, frame_bytes, index, n_out, group, dst); break;
  }
  HIP_TRY(hipGetLastError());
  return TC_OK;
}
#endif  // part 0: the host side
