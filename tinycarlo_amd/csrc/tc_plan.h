// Host-only planners: of tc_env_create, how the camera stage's work is cut into groups and where its buffers sit in
// LDS; of a call, which route it takes through launch() (plan_call, at the end).  Pure arithmetic on host values -- no
// HIP header, no device call -- so the host compiler builds it alone (tests/test_plan_cpu.py does).  The limits that
// belong to the kernels (group count, register-cache sizes) come in as arguments.
#pragma once
#include <vector>

#include "../../include/tinycarlo_hip.h" /* TC_T_* */

static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// Camera layer groups.  Up to 512 nodes / edges the whole map is one group held in the K = 5 / 8 register cache.
// Beyond that the layers are packed greedily, in order, into groups no larger than the largest single layer:
// the LDS node buffer shrinks from the whole map to that layer (knuffingen: 827 -> 517 nodes, 26.6 -> 17.4 KB per
// env, 6 -> 8 workgroups per CU) and a K = 9 cache (576 slots) covers a group.  Maps whose largest layer exceeds
// `max_cap` (576) nodes or edges, or that would need more than `max_groups` groups or fewer than two, stay one group
// on the K = 13 windowed path: ok is false and nothing else is set.
struct LayerGroups {
  bool ok = false;
  std::vector<int> layer;  // group g = layers layer[g] .. layer[g + 1] - 1
  int cap_n = 0, cap_e = 0;  // nodes / edges of the largest group
};
static inline LayerGroups plan_layer_groups(const int* node_off, const int* edge_off, int C, int max_cap, int max_groups) {
  LayerGroups p;
  int cap = 0;
  for (int l = 0; l < C; l++) {
    int nl = node_off[l + 1] - node_off[l], el = edge_off[l + 1] - edge_off[l];
    cap = nl > cap ? nl : cap;
    cap = el > cap ? el : cap;
  }
  if (cap > max_cap) return p;
  std::vector<int> lay(1, 0);
  for (int l = 0; l < C;) {
    if ((int)lay.size() - 1 == max_groups) return p;
    int first = l;
    while (l < C && node_off[l + 1] - node_off[first] <= cap && edge_off[l + 1] - edge_off[first] <= cap) l++;
    lay.push_back(l);  // l > first: a single layer always fits `cap`
  }
  const int ng = (int)lay.size() - 1;
  if (ng < 2) return p;
  for (int g = 0; g < ng; g++) {
    int nl = node_off[lay[g + 1]] - node_off[lay[g]], el = edge_off[lay[g + 1]] - edge_off[lay[g]];
    p.cap_n = nl > p.cap_n ? nl : p.cap_n;
    p.cap_e = el > p.cap_e ? el : p.cap_e;
  }
  p.layer = lay;
  p.ok = true;
  return p;
}

// Component groups.  The layer scheme leaves the LDS node buffer at the size of the largest LAYER (knuffingen: 517 of
// 827 nodes, 12.4 KB of a workgroup's 17.4 KB), and that buffer is what decides how many frame workgroups a CU holds
// (9).  A layer is not the unit of independence, though: camera.py's fix-up passes move a node along its own edges
// only, so every connected component of the lane-line graph (a dash of a dashed line is one) can be processed on its
// own.  The camera stage therefore works from a copy of the map in which the components of each layer stand side by
// side -- nodes renumbered, every layer's edges still contiguous and in their original relative order (the replay of a
// fix-up chain follows edge order, and a chain never leaves its component) -- packed greedily into groups of at most
// T nodes / edges (TC_CAM_GROUP, default 320: the buffer shrinks to 7.7 KB).  Nodes without an edge are never drawn and
// are left out.  ok is false when a component is larger than T, the groups are more than `max_groups`, or a group's
// edges are not one index range: the caller keeps the layer scheme.
struct ComponentGroups {
  bool ok = false;
  std::vector<int> new_id;    // [n_nodes]: a node's id in the camera copy, -1 for a node without an edge
  std::vector<int> n0, e0;    // group g = nodes n0[g] .. n0[g + 1] - 1 (new ids) and edges e0[g] .. e0[g + 1] - 1
  std::vector<int> l0, l1;    // ... whose layers are l0[g] .. l1[g] - 1
  int cap_n = 0, cap_e = 0;   // nodes / edges of the largest group
};
// edges: n_edges = edge_off[C] pairs of global node ids, layer by layer
static inline ComponentGroups plan_component_groups(const int* edge_off, int C, const int* edges, int n_nodes, int T,
                                                    int max_groups) {
  ComponentGroups p;
  const int TN = n_nodes, TE = edge_off[C];
  std::vector<int> parent(TN);
  for (int i = 0; i < TN; i++) parent[i] = i;
  auto find = [&](int x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  for (int ed = 0; ed < TE; ed++) {
    const int a0 = find(edges[2 * ed]), b0 = find(edges[2 * ed + 1]);
    if (a0 != b0) parent[b0 > a0 ? b0 : a0] = b0 > a0 ? a0 : b0;
  }
  // components in order of their first edge (edges are layer by layer, so components are too)
  std::vector<int> comp_of_root(TN, -1), comp_first_edge, comp_nn, comp_ne;
  std::vector<int> edge_comp(TE);
  for (int ed = 0; ed < TE; ed++) {
    const int r = find(edges[2 * ed]);
    if (comp_of_root[r] < 0) {
      comp_of_root[r] = (int)comp_first_edge.size();
      comp_first_edge.push_back(ed);
      comp_nn.push_back(0);
      comp_ne.push_back(0);
    }
    edge_comp[ed] = comp_of_root[r];
    comp_ne[edge_comp[ed]]++;
  }
  std::vector<int> node_comp(TN, -1);
  for (int i = 0; i < TN; i++) {
    const int c = comp_of_root[find(i)];
    node_comp[i] = c;  // -1: a node without an edge
    if (c >= 0) comp_nn[c]++;
  }
  const int NC = (int)comp_first_edge.size();
  if (NC == 0) return p;
  for (int c = 0; c < NC; c++)
    if (comp_nn[c] > T || comp_ne[c] > T) return p;
  std::vector<int> grp_first_comp(1, 0);
  for (int c = 0, gn = 0, ge = 0; c < NC; c++) {
    if (gn + comp_nn[c] > T || ge + comp_ne[c] > T) {
      grp_first_comp.push_back(c);
      gn = ge = 0;
    }
    gn += comp_nn[c];
    ge += comp_ne[c];
  }
  grp_first_comp.push_back(NC);
  const int NG = (int)grp_first_comp.size() - 1;
  if (NG > max_groups) return p;
  // New node ids: components in order, nodes of a component in their old order.  The edges are NOT moved (inside a
  // layer the edges of two components may interleave -- two dashes drawn alternately -- and the replay of a fix-up
  // chain needs every layer's edges in their old relative order): an edge keeps its index and only its node ids
  // change.  A group's edges are then the index range from its first component's first edge to its last component's
  // last edge, which must hold no edge of another group's components and start where the group before ends.
  p.new_id.assign(TN, -1);
  std::vector<int> comp_n0(NC + 1, 0);
  for (int c = 0; c < NC; c++) comp_n0[c + 1] = comp_n0[c] + comp_nn[c];
  std::vector<int> fill(comp_n0.begin(), comp_n0.end() - 1);
  for (int i = 0; i < TN; i++)
    if (node_comp[i] >= 0) p.new_id[i] = fill[node_comp[i]]++;
  std::vector<int> comp_last_edge(NC, -1);
  for (int ed = 0; ed < TE; ed++) comp_last_edge[edge_comp[ed]] = ed;
  p.e0.assign(NG + 1, TE);
  p.n0.assign(NG + 1, comp_n0[NC]);
  int next_e = 0;  // where a group's edges must start: right behind the group before
  for (int g = 0; g < NG; g++) {
    const int c0 = grp_first_comp[g], c1 = grp_first_comp[g + 1];
    int lo = TE, hi = -1, ne = 0;
    for (int c = c0; c < c1; c++) {
      lo = comp_first_edge[c] < lo ? comp_first_edge[c] : lo;
      hi = comp_last_edge[c] > hi ? comp_last_edge[c] : hi;
      ne += comp_ne[c];
    }
    if (lo != next_e) return p;
    for (int ed = lo; ed <= hi; ed++)
      if (edge_comp[ed] < c0 || edge_comp[ed] >= c1) return p;
    next_e = lo + ne;
    p.e0[g] = lo;
    p.n0[g] = comp_n0[c0];
  }
  p.l0.assign(NG, 0);
  p.l1.assign(NG, 0);
  for (int g = 0; g < NG; g++) {
    const int nl = p.n0[g + 1] - p.n0[g], el = p.e0[g + 1] - p.e0[g];
    p.cap_n = nl > p.cap_n ? nl : p.cap_n;
    p.cap_e = el > p.cap_e ? el : p.cap_e;
    int la = 0, lb = 0;
    while (la + 1 < C && p.e0[g] >= edge_off[la + 1]) la++;
    while (lb + 1 < C && p.e0[g + 1] - 1 >= edge_off[lb + 1]) lb++;
    p.l0[g] = la;
    p.l1[g] = lb + 1;
  }
  p.ok = true;
  return p;
}

// LDS of the camera stage, per workgroup: the node buffer, the node flags, the fix-up edge list / projection candidate
// list and the counters, for camera groups of at most cap_n nodes and cap_e edges on a map of total_nodes nodes.
// Sets off_p, off_flg, off_list, off_cnt and total of L (the kernels' LdsLayout).
template <class Layout>
static inline void plan_cam_lds(Layout& L, int cap_n, int cap_e, int total_nodes) {
  const int cap_nodes = cap_n > 0 ? cap_n : 1;
  int off = 0;
  L.off_p = off;  // node buffer: 3 doubles per node of the largest camera group; phase B aliases it with one
                  // double per lane-line node of the whole map
  int pbytes = 3 * cap_nodes * 8;
  if (total_nodes * 8 > pbytes) pbytes = total_nodes * 8;
  off += align_up(pbytes, 16);
  L.off_flg = off;
  off += align_up(cap_nodes, 16);
  L.off_list = off;  // fix-up edge list / projection candidate list
  off += align_up((2 * cap_e > cap_n ? 2 * cap_e : cap_n) * 4 + 16, 16);
  L.off_cnt = off;
  off += 64;
  L.total = off;
}

// LDS of a tc_frame_kernel / tc_frame_recover_kernel workgroup.  These kernels keep no env state in LDS and run the
// camera stage and the raster stage one after the other, so a workgroup needs the larger of the two stages plus the head
// of the frame's draw list, which both stages see -- and how many workgroups a CU holds follows from that sum in steps of
// 1280 bytes.  Where plan_cam_lds and the full-size raster tables are sized for every path a kernel may take, this plan
// is sized for the paths THIS handle takes:
//   - camera groups held in registers (`windowed` false) use the one-word list entries of tc_pack.h and keep their counts
//     in registers: the list region is tc_pack_list_bytes, and there is no counter block (off_cnt then names the list
//     region: nothing reads it).  A windowed group keeps the two-int entries and the 64-byte block of plan_cam_lds.
//   - the outline table `lt` holds rb << sh items: sh = 1 when the handle draws with the two long outline edges
//     (R_F_LONG_EDGES), 2 otherwise (the layout of k_common.h's R_OFF_LC_OF / R_OFF_BITS_SH, repeated here in plain
//     arithmetic; the host source asserts that the two agree).
// The head sits behind whichever stage is larger and takes what is left up to the next 1280-byte step (at least `live`
// bytes, the slot the fused kernels park the env in: the head never gets smaller than it would be without any growth),
// at most 4096 bytes more, and the whole never exceeds `limit`, the bytes the layout shared with the other kernels
// gives a frame workgroup (0: no limit).  seg_lds / seg_lds_limit: the switches TC_SEG_LDS / TC_SEG_LDS_CAP; the frame
// kernels read draw lists from LDS only, so the head holds 8 entries whatever they say.  reserve: bytes of static LDS
// the build adds to every workgroup (the stamp buffer of the timing builds), taken out of the growth.
struct FrameLds {
  int off_p = 0, off_flg = 0, off_list = 0, off_cnt = 0;  // camera stage
  int cam_total = 0;
  int list_bytes = 0;
  bool counters = false;
  int r_off_tab = 0, r_off_bits = 0;  // raster stage
  int r_total = 0;
  int head_off = 0, head_cap = 0;  // draw-list head: head_cap entries of 20 bytes
  int total = 0;                   // dynamic LDS of the launch
};
#define TC_LDS_STEP 1280
#define TC_SEG_ENTRY_BYTES 20
static inline FrameLds plan_frame_lds(int cap_n, int cap_e, int total_nodes, bool windowed, int rb, int sh, int band_bytes,
                                      int live, bool seg_lds, int seg_lds_limit, int limit, int reserve) {
  FrameLds f;
  const int cap_nodes = cap_n > 0 ? cap_n : 1;
  int off = 0;
  f.off_p = off;
  int pbytes = 3 * cap_nodes * 8;
  if (total_nodes * 8 > pbytes) pbytes = total_nodes * 8;
  off += align_up(pbytes, 16);
  f.off_flg = off;
  off += align_up(cap_nodes, 16);
  f.off_list = off;
  f.list_bytes = windowed ? (2 * cap_e > cap_n ? 2 * cap_e : cap_n) * 4 + 16 : (4 * cap_e > 2 * cap_n ? 4 * cap_e : 2 * cap_n) + 16;
  f.list_bytes = align_up(f.list_bytes, 16);
  off += f.list_bytes;
  f.counters = windowed;
  f.off_cnt = windowed ? off : f.off_list;
  if (windowed) off += 64;
  f.cam_total = off;
  f.r_off_tab = 0;
  f.r_off_bits = align_up(rb * 116 + (rb << sh) * (4 + 5 * 4), 16);
  f.r_total = f.r_off_bits + align_up(band_bytes, 16);
  f.head_off = align_up(f.cam_total > f.r_total ? f.cam_total : f.r_total, 16);
  const int want = f.head_off + live;
  int grown = align_up(want + reserve, TC_LDS_STEP) - reserve;
  if (grown > want + 4096) grown = want + 4096;
  if (limit > 0 && grown > limit) grown = limit;
  if (grown < want) grown = want;
  f.total = grown;
  f.head_cap = (grown - f.head_off) / TC_SEG_ENTRY_BYTES;
  if (!seg_lds) {
    f.head_cap = 0;
    f.total = want;
  }
  if (f.head_cap > seg_lds_limit) f.head_cap = seg_lds_limit;
  if (f.head_cap < 8) {
    f.head_cap = 8;
    if (f.total < f.head_off + 8 * TC_SEG_ENTRY_BYTES) f.total = f.head_off + 8 * TC_SEG_ENTRY_BYTES;
  }
  return f;
}

// LDS of a tc_envg_kernel / tc_drive_envg_kernel workgroup.  The simulate launch of a streamed call runs BESIDE the frame
// dispatch for most of the call, one workgroup on a CU, and what it holds there the frame workgroups cannot have: every
// TC_LDS_STEP * 7 = 8960 bytes (cfg3) is one frame workgroup fewer on that CU while the launch lasts.  So the launch asks
// for what THIS call reads:
//   - the lane-line edge records (48 bytes per edge; phase B's edge scan) only when every step runs phase B
//     (`info_every`, CallPlan::info_every).  Otherwise phase B runs in the launch's last step alone and reads the records
//     from global memory: a copy held for 128 steps and read in one is not worth its bytes.
//   - the lanepath's fat node records (`lp_node_bytes` each; the tracking of every step), as before.
//   - per env of the workgroup (`groups` of them), one double per lane-line layer of THIS map (the distances the terms
//     read), not TC_MAX_LAYERS of them, and the terms' `max_terms` counters.
// `map_switch`: TC_ENVG_MAP_LDS (0: neither table in LDS).  `static_bytes`: the kernel's own static LDS (the per-env words
// of the features compiled in: envg_static_lds).  `pad`: unused bytes (experiment builds).  `frame_lds`: the dynamic LDS of
// a frame workgroup of the handle (0: the handle has no frame kernel), for frames_beside.
#define TC_CU_LDS (160 * 1024)
struct EnvgLds {
  int map_lds = 0, fat_lds = 0;  // MultiArgs::map_lds / fat_lds
  int fat_off = 0;               // the fat node records: behind the edge records, or at 0 without them
  int grp_off = 0, grp_stride = 0, cnt_off = 0;  // env g's block at grp_off + g * grp_stride: distances, counters at cnt_off
  int dynamic = 0;               // dynamic LDS of the launch
  int static_bytes = 0;
  int granted = 0;               // dynamic + static as a CU grants it: whole steps of TC_LDS_STEP
  int workgroups = 0;            // of the launch
  int frames_beside = 0;         // frame workgroups that fit on a CU beside one simulate workgroup
};
// static LDS of the kernel: the camera-bank index of every env, the running episode (EP) and the drive randomisation's
// maneuver / draw counter / OU value (CTRL) -- per env where the feature is compiled in, nothing otherwise (the host
// source reports the compiler's own figure, tc_env_envg_lds_info; this restates it for the CPU tests)
static inline int envg_static_lds(int groups, bool ep, bool ctrl) {
  return groups * 4 + (ep ? groups * (4 + 8) : 0) + (ctrl ? groups * (4 + 4 + 8) : 0);
}
static inline EnvgLds plan_envg_lds(int total_edges, int lpN, int lp_node_bytes, int C, int max_terms, int N,
                                    int groups, bool info_every, bool map_switch, int static_bytes, int frame_lds, int pad) {
  EnvgLds p;
  const long long map_bytes = align_up(total_edges * 48, 16), fat_bytes = (long long)lpN * lp_node_bytes;
  p.map_lds = (map_switch && info_every && map_bytes <= 40 * 1024) ? 1 : 0;
  p.fat_lds = (map_switch && fat_bytes <= 56 * 1024) ? 1 : 0;
  int off = 0;
  if (p.map_lds) off += (int)map_bytes;
  p.fat_off = off;
  if (p.fat_lds) off += (int)fat_bytes;
  off = align_up(off, 16);
  p.grp_off = off;
  p.cnt_off = C * 8;
  p.grp_stride = C * 8 + align_up(max_terms * 4, 8);
  off += groups * p.grp_stride;
  p.dynamic = align_up(off, 16) + pad;
  p.static_bytes = static_bytes;
  p.granted = align_up(p.dynamic + p.static_bytes, TC_LDS_STEP);
  p.workgroups = (N + groups - 1) / groups;
  const int frame_granted = align_up(frame_lds, TC_LDS_STEP);
  p.frames_beside = frame_granted > 0 && p.granted < TC_CU_LDS ? (TC_CU_LDS - p.granted) / frame_granted : 0;
  return p;
}

// Which way a call of nsteps steps goes through launch() on a handle: decided here for launch(), which dispatches on
// it, and for tc_env_launch_info, which reports it.  What the decision reads of the handle and of the call comes in as
// plain values (the host side fills them in one place, plan_of()).
struct CallInputs {
  // the switches, in this order: TC_FUSE, TC_MULTI_SPLIT, TC_ENV_GROUPED, TC_CHUNK > 0 (pipe), TC_STREAM, and the value
  // of TC_CHUNK (chunk)
  int fuse, multi_split, env_grouped, pipe, stream, chunk;
  int kvar;            // register-cache slots of the handle's simulate stage: 5, 8, 9, 13
  bool packed;         // the observation format is the packed class masks (TC_FMT_CLASSES_BITS)
  int ring_rows;       // steps a slot of the scratch ring of chunked calls holds (0: no ring)
  int streamed_rows;   // steps the scratch of streamed calls holds (0: none)
  bool st_words;       // the two device words of a streamed call exist
  unsigned flags;      // the call's flags ...
  unsigned no_frame_flags;  // ... and the bits of them that leave the frames out (they belong to the kernels' header)
  int nsteps;
  bool obs;            // there is a tensor to draw into (the bound one or the rollout's)
  bool all;            // every step's frame is wanted (a rollout with observations), else only the last one survives
  // who reads the lane-line distances ("phase B" of the simulate kernels) of a step that is not a launch's last:
  bool info_rows = false;   // the call's rollout has laneline_distances or nearest_edge rows
  bool info_terms = false;  // an installed term does (term_reads_distances; kept on the handle by tc_env_set_terms)
  int info_every = 0;       // the switch TC_INFO_EVERY_STEP
};
struct CallPlan {
  bool do_raster;  // frames are drawn at all
  bool fused;      // one tc_step_kernel launch: simulate + raster by the same wavefront
  bool split;      // K steps with frames: per chunk ONE simulate launch over its steps and ONE launch over the frames
                   // wanted (neither: one tc_env_kernel launch, and a tc_raster_kernel launch behind it when frames are
                   // drawn)
  bool frames;     // split: camera + raster per frame (tc_frame_kernel); else camera in the simulate launch (the
                   // register-hungry K = 13 stage, TC_FUSE=0) and a raster launch
  bool grouped;    // frames: the simulate launches are the grouped kernel (tc_envg_kernel), else one wavefront per env
  bool piped;      // split: the frames of a chunk are produced on an internal stream, beside the next simulate launch
  bool streamed;   // piped: the whole call (or st_rows steps of it) is one simulate launch and one gated frame launch
  int steps;       // steps per simulate / frame dispatch
  bool info_every; // every step of every simulate launch of the call computes the lane-line distances; else only a
                   // launch's last step does (the env's laneline_distances / nearest_edge buffers hold that step's)
};
// The reward / termination terms that read a step's lane-line distances (d_apply_terms): the three lane-line kinds.
static inline bool term_reads_distances(int kind) {
  return kind == TC_T_LANELINE_SPARSE_REWARD || kind == TC_T_LANELINE_LINEAR_REWARD || kind == TC_T_LANELINE_CROSSING_TERMINATION;
}
static inline CallPlan plan_call(const CallInputs& in) {
  CallPlan p;
  // (the register-hungry K = 13 simulate stage spills when fused, so it stays two launches)
  const bool can_frames = in.fuse && in.kvar != 13;
  // packed class masks have tc_frame_kernel and tc_raster_kernel variants only: a single step is the two-launch form,
  // K steps are always split (TC_MULTI_SPLIT=0 is ignored)
  const bool can_fuse = can_frames && !in.packed;
  p.do_raster = !(in.flags & in.no_frame_flags) && in.obs;
  p.split = p.do_raster && in.nsteps > 1 && (in.multi_split || !can_fuse);
  p.fused = p.do_raster && can_fuse && !p.split;
  p.frames = p.split && can_frames;
  p.grouped = p.frames && in.env_grouped;
  p.piped = p.grouped && in.pipe && in.all;
  p.streamed = p.piped && in.stream && in.streamed_rows >= 2 && in.st_words;
  // Phase B carries nothing from step to step, and its results leave a launch three ways only: the rollout's rows, the
  // terms of the step, and -- of the launch's last step -- the env's buffers.  One bit for the whole call: every launch it is
  // split into (chunks, 128-step segments) is given the same.
  p.info_every = in.info_rows || in.info_terms || in.info_every != 0;
  p.steps = in.nsteps;
  if (p.streamed) {
    if (p.steps > in.streamed_rows) p.steps = in.streamed_rows;
  } else if (!p.fused) {
    // a chunk of a pipelined call: TC_CHUNK (16) steps, or a quarter of the call when that is less, so that a short
    // call (the 20 steps of a smoke benchmark) still has several chunks in flight; never more than a ring slot holds.
    // Calls that are not pipelined run in chunks as large as the ring allows.
    if (p.piped) {
      const int q = (in.nsteps + 3) / 4;
      p.steps = in.chunk < q ? in.chunk : (q < 2 ? 2 : q);
    }
    if (in.ring_rows > 0 && p.steps > in.ring_rows) p.steps = in.ring_rows;
  }
  return p;
}
