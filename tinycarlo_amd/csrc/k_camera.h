// k_camera.h -- the camera stage, phase C of a frame (camera.py:52-110): transform -> 4 clip passes -> project ->
// visibility -> draw list.  Holds the per-lane register cache of the map (MapCache, cache_*) that the simulate stage's
// phase B shares, the fix-up passes (cam_move_to_plane, cam_chain_replay, cam_group_regs for a group held in registers,
// cam_fixup_pass for windowed groups; rules of the merged passes: tc_clip.h), cam_project (camera.py:133-142), what a
// frame needs of an env (FramePose, the pose row and its markers, cam_pose12 = camera.py:62), the whole-frame cull
// (cam_cull, and cam_cull_row for the pose-row writers of the simulate kernels; tc_cull.h) and the stage itself,
// cam_body.  Defines no kernel: tc_env_kernel<.., CAM = true> (k_env.h), tc_frame_kernel and tc_step_kernel (k_frame.h) run it.  Includes k_common.h and the plain-arithmetic tc_clip.h,
// tc_cull.h, tc_device.h.
#ifndef K_CAMERA_H
#define K_CAMERA_H

#include "k_common.h"
#include "tc_clip.h"
#include "tc_cull.h"
#include "tc_pack.h"
#include "tc_device.h"

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

// The same replay over the one-word entries of tc_pack.h (cam_group_regs' lists): the word compares as its edge id.
__device__ inline void cam_chain_replay_packed(double* Px, double* Py, double* Pz, unsigned char* flg, int bit, double tz,
                                               const int* list, int n, double max_range, bool range_too, int tid) {
  for (int k = tid; k < n; k += TC_NT) {
    const int w = list[k];
    const int t = tc_pack_target(w);
    bool first = true;
    for (int j = 0; j < n; j++)
      if (tc_pack_target(list[j]) == t && list[j] < w) first = false;
    if (!first) continue;
    int cur = w;
    for (int guard = 0; guard < n; guard++) {
      cam_move_to_plane(Px, Py, Pz, tc_pack_other(cur), t, tz);
      int nxt = 0x7fffffff;
      for (int j = 0; j < n; j++) {
        const int wj = list[j];
        if (tc_pack_target(wj) == t && wj > cur && wj < nxt) nxt = wj;
      }
      if (nxt == 0x7fffffff) break;
      cur = nxt;
    }
    unsigned int f = flg[t] | (unsigned)bit;
    if (range_too) f = (f & ~2u) | (Pz[t] > -max_range ? 2u : 0u);
    flg[t] = (unsigned char)f;
  }
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

// The nine entries of a frame's K matrix (camera.py:48-50) as wave-uniform values in scalar registers: the shared camera's in
// scalar loads from the kernel-argument segment, or row cam_row of the camera rows -- vector loads made uniform: the row is the
// same for the whole wavefront, but the rows are device memory that tc_env_set_camera_per_env / tc_env_set_camera_bank rewrite
// between calls, and nothing shows that no such copy is ever in flight beside a frame launch, which a read through the
// scalar cache would need.  Called with the argument block passed through kernarg_again(), so the loads stay at the call.
__device__ __forceinline__ void cam_load_K(const KArgs& a, const int cam_row, double* Kc) {
  if (a.cam_K) {  // (a branch, not a select of pointers: the shared camera's K then comes in scalar loads)
#pragma unroll
    for (int i = 0; i < 9; i++) Kc[i] = uni_d(a.cam_K[(size_t)cam_row * 9 + i]);  // (the row that came with the pose, not the env's latest)
  } else {
    const __attribute__((address_space(4))) double* kk = (const __attribute__((address_space(4))) double*)(unsigned long long)a.cam.K;
#pragma unroll
    for (int i = 0; i < 9; i++) Kc[i] = kk[i];  // (explicitly the kernarg segment: cannot be merged with the other branch)
  }
}

// Phase C of one camera group whose nodes and edges sit in the wavefront's registers (one window: every bundled map).
// camera.py:52-110 reads the whole node / edge arrays in each of its steps; here the flags of an edge's two ends are
// carried in a register per edge slot (`ff`) and refreshed only after a pass that moved something, so a fix-up pass in
// which no edge straddles the plane -- or only a handful, the usual case -- costs a few compares per slot instead of a
// round of LDS traffic, and the straddling edges are compacted (ballot + mbcnt, no atomics) so that the move code runs
// ONCE per pass, on the low lanes, instead of once per register slot.
//   idx_in_range (camera.py:80) is evaluated on the depths left by passes 1-2: it is set here from the transformed depth
// and refreshed for exactly the nodes those passes move -- the same values, without a pass over all nodes.
// Appends the group's visible edges to the draw list at segg[5 * nseg ...] and advances nseg (wave-uniform).
// PACKED: the lists hold the one-word entries of tc_pack.h (and 16-bit projection candidates) instead of two ints per entry
// (edge id; target | other << 16): half the list region.  The form of the kernel whose LDS plan is sized for it -- the
// five-wave frame kernel (plan_frame(), tinycarlo_hip.hip); every other kernel keeps the two-int entries, with which its
// register count is what it was.
template <int K, bool PACKED = false>
__device__ __forceinline__ void cam_group_regs(const KArgs& a, const MapCache<K>& mc, const double* pose, const double* Kc,
                                               const int cam_row, const int l0, const int l1, const int ge0, const int nn, const int ne,
                                               double* Px, double* Py, double* Pz, unsigned char* flg, int* list,
                                               int* segg, LdsIntPtr seg_lds, int& nseg, unsigned int& my_layers, const int env,
                                               const int tid) {
  static_assert(!PACKED || TC_PACK_FITS(K), "a group's edge and node ids must fit the one-word list entries of tc_pack.h");
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
          if constexpr (PACKED) {
            list[j] = tc_pack(k * TC_NT + tid, t, o);
          } else {
            list[2 * j] = k * TC_NT + tid;
            list[2 * j + 1] = t | (o << 16);
          }
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
        mine = tid < n ? (PACKED ? list[tid] : list[2 * tid + 1]) : -1;
        const int my_t = PACKED ? tc_pack_target(mine) : mine & 0xffff;
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
        const int t = PACKED ? tc_pack_target(mine) : mine & 0xffff, o = PACKED ? tc_pack_other(mine) : (int)((unsigned)mine >> 16);
        cam_move_to_plane(Px, Py, Pz, o, t, tz);
        unsigned int f = flg[t] | (unsigned)bit;
        if (pass < 2) f = (f & ~2u) | (Pz[t] > -max_range ? 2u : 0u);
        flg[t] = (unsigned char)f;
      }
    } else {
      if constexpr (PACKED)
        cam_chain_replay_packed(Px, Py, Pz, flg, bit, tz, list, n, max_range, pass < 2, tid);
      else
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
  unsigned short* cand_list = (unsigned short*)list;  // PACKED: node ids, 16 bits each
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int i = k * TC_NT + tid;
    const bool c = i < nn && (flg[i] & 16);
    const unsigned long long mk = __ballot(c);
    if (c) {
      if constexpr (PACKED)
        cand_list[ncand + wave_rank(mk)] = (unsigned short)i;
      else
        list[ncand + wave_rank(mk)] = i;
    }
    ncand += __popcll(mk);
  }
  lds_sync();
  double Kl[9];  // PACKED: the camera's K matrix, fetched here, where it is used, and not held across the clip passes (see cam_body)
  if constexpr (PACKED) cam_load_K(kernarg_again(a), cam_row, Kl);
  const double* Kp = PACKED ? Kl : Kc;
  for (int k = tid; k < ncand; k += TC_NT) {  // camera.py:133-142, 90
    const int i = PACKED ? (int)cand_list[k] : list[k];
    double u, v;
    int2 q = cam_project(Kp, Px[i], Py[i], Pz[i], u, v);
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
      if constexpr (PACKED) {
        list[j] = tc_pack(k * TC_NT + tid, mc.ed[k].x, mc.ed[k].y);
      } else {
        list[2 * j] = k * TC_NT + tid;
        list[2 * j + 1] = mc.ed[k].x | (mc.ed[k].y << 16);
      }
    }
    ndraw += __popcll(mk);
  }
  lds_sync();
  for (int j = tid; j < ndraw; j += TC_NT) {  // both ends were marked above and hold pixel coordinates
    const int w = PACKED ? list[j] : list[2 * j + 1], e = PACKED ? tc_pack_edge(w) : list[2 * j];
    const int2 pa = ((int2*)Px)[PACKED ? tc_pack_target(w) : w & 0xffff], pb = ((int2*)Px)[PACKED ? tc_pack_other(w) : (int)((unsigned)w >> 16)];
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

// what the camera needs of an env's state: rear-axle position and cos / sin of MINUS the heading (car.py:159-165)
struct FramePose {
  double x, y, cth, sth;
};

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
// (entry 12 is the camera bank's index, entry TC_CULL_ROW_ENTRY = 13 the whole-frame cull's verdict, tc_cull.h: written, polled and
// reset like the twelve pose entries when the call's rows carry them, and like them never all ones)
static_assert(TC_CULL_ROW_DRAW != TC_POSE_EMPTY && TC_CULL_ROW_CULLED != TC_POSE_EMPTY && TC_CULL_ROW_ENTRY == 13 && TC_CULL_ROW_ENTRY < TC_POSE_ROW,
              "a verdict is never read as 'not written yet'");
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
// the table's header fields the predicate reads, through scalar loads (one address for every lane)
__device__ __forceinline__ void cam_cull_head(const KArgs& a, TcCullHead& h) {
  typedef const __attribute__((address_space(4))) double* DConst;
  typedef const __attribute__((address_space(4))) int* IConst;
  static_assert(offsetof(TcCullHead, margin) == 32 && offsetof(TcCullHead, nx) == 48 && offsetof(TcCullHead, n_special) == 56 &&
                    offsetof(TcCullHead, special) == 64 && TC_CULL_HEAD_BYTES % 4 == 0,
                "the fields are read by offset below");
  const DConst hd = (DConst)(unsigned long long)a.cull_tab;
  const IConst hi = (IConst)(unsigned long long)a.cull_tab;
  h.x0 = hd[0];
  h.y0 = hd[1];
  h.inv = hd[2];
  h.cell = hd[3];
  h.margin = hd[4];
  h.nx = hi[12];
  h.ny = hi[13];
  h.n_special = hi[14];
}
__device__ __forceinline__ bool cam_cull(const KArgs& a, const double* pose) {
  typedef const __attribute__((address_space(4))) double* DConst;
  typedef const __attribute__((address_space(4))) unsigned int* UConst;
  const DConst hd = (DConst)(unsigned long long)a.cull_tab;
  TcCullHead h;
  cam_cull_head(a, h);
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

// The same predicate where the pose differs from lane to lane: the pose-row writers of the simulate kernels (k_envg.h holds an
// env per group of lanes, k_env.h one per wavefront), which evaluate it once per (step, env) on the very pose they store and
// leave the answer in entry TC_CULL_ROW_ENTRY of the row (tc_cull.h), so that no frame wavefront evaluates it again.  The same
// pieces of tc_cull.h in the same order: header and special nodes through scalar loads, a cell's byte through a vector load.
// Only called when a.cull_rows is set (then a.frame_cull is, and the table exists).
__device__ __forceinline__ unsigned long long cam_cull_row(const KArgs& a, const double* pose) {
  typedef const __attribute__((address_space(4))) double* DConst;
  const DConst hd = (DConst)(unsigned long long)a.cull_tab;
  TcCullHead h;
  cam_cull_head(a, h);
  bool empty = true;
#pragma unroll
  for (int i = 0; i < TC_CULL_NC; i++) {
    double wx, wy;
    tc_cull_world(pose, a.cull.c[i], &wx, &wy);
    const int cell = tc_cull_cell(h, wx, wy, a.cull.r[i]);
    // (a cell index is below nx * ny; the byte of cell 0 stands in for "no cell" and is not looked at)
    const int q = (int)a.cull_tab[TC_CULL_HEAD_BYTES + (cell > 0 ? cell : 0)];
    empty = empty && (cell == TC_CULL_CELL_CLEAR || (cell >= 0 && tc_cull_free(h, q, a.cull.r[i])));
  }
  if (empty) {  // guard G, only for a frame that would be culled
    const double mr = a.cull.max_range;
    for (int i = 0; i < h.n_special; i++) {
      const double z = __builtin_fma(pose[9], hd[9 + 2 * i], __builtin_fma(pose[8], hd[8 + 2 * i], pose[11]));
      empty = empty && tc_fabs(z + mr) >= TC_CULL_GUARD;
    }
  }
  return tc_cull_row_encode(empty);
}

// LEAN: the form of the five-wave frame kernel -- the camera's K matrix in scalar registers (see below) and the one-word list
// entries of cam_group_regs<K, PACKED>
// ROW: the frame's pose came in a pose row, and with it the cull's verdict (`row_culled`, wave-uniform: what the simulate stage
// left in entry TC_CULL_ROW_ENTRY, false when the call's rows carry none): the form of the frame, banded and recover kernels,
// which never evaluate the predicate themselves.  !ROW: the pose was computed by this wavefront (the fused step kernels,
// tc_env_kernel<.., CAM>): cam_cull here.
// ONE_GROUP: the handle's camera groups are one group (KArgs::n_grp == 1) that fits the register cache -- cam_group_regs once,
// no group loop whose invariants would have to be kept "because the loop could run again".  The form of tc_frame_kernel<5, .., 32>
// alone (frame_kernel_of sends every other handle of that K to tc_frame_banded).
template <int K, bool LEAN = false, bool ROW = false, bool ONE_GROUP = false>
__device__ __forceinline__ void cam_body(const KArgs& a, unsigned char* smem, int env, int cam_row, const double* pose_in, MapCache<K>& mc,
                                         const bool mc_loaded, const int tid, const int seg_row, int& nseg_out,
                                         unsigned int& used_out, const bool store_n = true, const bool row_culled = false) {
  // Whole-frame cull: a pose whose visible ground footprint keeps clear of every lane-line segment has an empty draw
  // list (tc_cull.h) -- the stage ends here with what it delivers for an empty list: length 0, no
  // layer, the length stored where it is stored otherwise, nothing written to the overflow list.
#ifdef TC_ABLATE
  if (ROW && a.cull_rows && threadIdx.x == 0) {  // (the counts of cam_cull, for the frames whose verdict came in the row)
    atomicAdd(&tc_cull_counts[0], 1ull);
    if (row_culled) atomicAdd(&tc_cull_counts[1], 1ull);
  }
#endif
  if (ROW && row_culled) {  // (the pose was not even fetched: frame_pose)
    nseg_out = 0;
    used_out = 0;
    if (store_n && tid == 0) a.seg_n[(size_t)seg_row * a.N + env] = 0;
    return;
  }
  unsigned int my_layers = 0;  // layers this lane put a segment into the draw list for
  const DevMap& m = a.m;
  const int nwin_n = (m.total_nodes + TC_NT * K - 1) / (TC_NT * K), nwin_e = (m.total_edges + TC_NT * K - 1) / (TC_NT * K);
  const bool single = a.n_grp == 1 && !a.cam_nodes && a.grp_layer[0] == 0 && a.grp_layer[1] == m.C && nwin_n <= 1 && nwin_e <= 1;
  // the 12 entries are the same in every lane: kept in scalar registers through the node loop (24 VGPRs less)
  double pose[12];
#pragma unroll
  for (int i = 0; i < 12; i++) pose[i] = uni_d(pose_in[i]);
  if (!ROW && a.frame_cull && cam_cull(a, pose)) {
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
  // (LEAN: wave-uniform like the pose, and in scalar registers like it: as vector values the nine entries are 18 VGPRs held
  // from here across the clip passes to the projection -- the registers the frame kernel's five-wave bound lacks -- and as
  // scalar values fetched here they were 18 SGPRs spilled to vector lanes across the same span.  So that form fetches them
  // at the projection: cam_load_K.  The kernels that simulate in the same wavefront sit at their SGPR limit already and keep
  // the vector form, fetched here.)
  double Kc[9];
  if constexpr (LEAN) {
    // (fetched where the projection needs them: in cam_group_regs, and below for a windowed group)
  } else if (a.cam_K) {  // (a branch, not a select of pointers: the shared camera's K then comes in scalar loads)
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
  if constexpr (ONE_GROUP) {
    // group 0 is all there is, and it sits in the register cache (the host checks both: frame_kernel_of's `looped`)
    const int gn0 = a.grp_n0[0], ge0 = a.grp_e0[0];
    const int nn = a.grp_n0[1] - gn0, ne = a.grp_e0[1] - ge0;
    if (!single) {
      if (a.cam_nodes) {
        cache_nodes_from(mc, a.cam_nodes, gn0, gn0 + nn, tid);
        cache_edges_from(mc, a.cam_edges_g, ge0, ge0 + ne, gn0, tid);
      } else {
        cache_nodes(mc, m, gn0, gn0 + nn, tid);
        cache_edges(mc, m, ge0, ge0 + ne, gn0, tid);
      }
    }
    cam_group_regs<K, LEAN>(a, mc, pose, Kc, cam_row, a.grp_l0[0], a.grp_l1[0], ge0, nn, ne, Px, Py, Pz, flg, list, segg,
                            (LdsIntPtr)(smem + a.seg_lds_off), nseg, my_layers, env, tid);
  } else
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
      cam_group_regs<K, LEAN>(a, mc, pose, Kc, cam_row, l0, l1, ge0, nn, ne, Px, Py, Pz, flg, list, segg, (LdsIntPtr)(smem + a.seg_lds_off), nseg,
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
    if constexpr (LEAN) cam_load_K(kernarg_again(a), cam_row, Kc);
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

#endif  // K_CAMERA_H
