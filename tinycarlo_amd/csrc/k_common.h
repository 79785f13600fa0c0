// k_common.h -- what every kernel stage shares: the TC_PART split of the build (TC_PLAIN_KERNEL), the launch modes, the LDS
// layout and the env's LiveLds record, the kernel-argument blocks KArgs / MultiArgs / RollStep, and the wavefront helpers
// (lds_sync, kernarg_again, d_readlane, uni_i / uni_d, wave_rank, wave_incl_scan, wave_incl_max, spread4).  Defines no kernel; the state
// it lays out is car.py's and env.py's per-env state.
#ifndef K_COMMON_H
#define K_COMMON_H

#include <hip/hip_runtime.h>

#include "../../include/tinycarlo_hip.h"
#include "k_probe.h"
#include "tc_cull.h"
#include "tc_device.h"

// (TC_PART: see the head of tinycarlo_hip.hip)
#if defined(TC_PART) && defined(TC_DEV_FAST)
#error "the development builds are one translation unit"
#endif
#if defined(TC_PART) && TC_PART > 0
#define TC_PLAIN_KERNEL static  // (kernels that are no templates live in part 0)
#else
#define TC_PLAIN_KERNEL
#endif

#define TC_PROF_RING 64
#define TC_RING_SLOTS 3  // chunks of a K-step call whose pose rows / draw lists exist at once (tc_env_reserve_steps)
#define MODE_STEP 0
#define MODE_RESET 1
#define MODE_RENDER 2

// Every workgroup of the stage kernels is ONE wavefront, and the LDS executes a wavefront's operations in program order:
// between phases that hand data from lane to lane through LDS nothing has to be waited for except the LDS queue itself
// (and the compiler kept from moving memory operations across).  __syncthreads() would also drain the vector-memory
// counter -- the frame's stores still in flight at the end of a band, the next batch's draw-list loads.
// The same goes for the simulate stage: a wait for vmcnt there would sit out the round trip of the step's rollout-row /
// pose-row stores (vector-memory operations retire in issue order).
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// A reference into the kernel-argument segment, passed through an empty asm: the compiler can no longer tell that two
// reads go to the same block, so values loaded behind this point are not merged with (and kept alive from) earlier
// loads, nor hoisted out of the loop the call sits in -- they are s_load'ed where they are used.
template <class T>
__device__ __forceinline__ const T& kernarg_again(const T& r) {
  unsigned long long p = (unsigned long long)&r;
  asm volatile("" : "+s"(p));
  return *(const T*)(const __attribute__((address_space(4))) T*)p;
}

// Segments rasterised per batch: 32 (64 * 106 bytes of tables per workgroup), or 16 in the kernels of the big-map
// variants (K >= 8: knuffingen), where the tables' 6.6 KB are what decides how many workgroups a CU holds.
#define RB_MAX 32
#define RB_OF_K(K) ((K) >= 8 ? 16 : 32)
// raster-stage LDS layout (compile-time: folds into instruction offsets and frees SGPRs)
#define R_OFF_TAB 0
#define R_TAB_BYTES_OF(RB) (((RB) * 4 * 5 + (RB) * 4 + 5 * (RB) + 8 * (RB)) * 4 + 2 * 4 * (RB) * 8)
#define R_OFF_BITS_OF(RB) ((R_TAB_BYTES_OF(RB) + 15) / 16 * 16)
// The tables of the five-wave frame kernel (raster_body<.., FORM>), which is launched with an LDS plan of the handle's outline
// form (plan_frame_lds, tc_plan.h): those of fixed size first (116 bytes per segment), then the two with an entry per outline
// item, the chunk counts `lc` (4 bytes) and the outline-edge parameters `lt` (20 bytes).  A batch has RB << sh items: sh = 2,
// the four edges of FillConvexPoly's quad, or sh = 1, the two long ones (R_F_LONG_EDGES); the bit-planes follow at
// RArgs::off_bits = R_OFF_BITS_SH(RB, sh).  Every other kernel keeps room for RB * 4 items and the layout above.
#define R_OFF_LC_OF(RB) ((RB) * 116)
#define R_TAB_BYTES_SH(RB, sh) (R_OFF_LC_OF(RB) + ((RB) << (sh)) * (4 + 5 * 4))
#define R_OFF_BITS_SH(RB, sh) ((R_TAB_BYTES_SH(RB, sh) + 15) / 16 * 16)
static_assert(R_TAB_BYTES_SH(32, 2) == R_TAB_BYTES_OF(32) && R_TAB_BYTES_SH(16, 2) == R_TAB_BYTES_OF(16), "the four-edge form is the full size");
#define LCH 8        // outline steps per chunk

#define TC_MAX_GROUPS 8
struct LdsLayout {
  int off_p, off_flg, off_list, off_cnt;
  int total;
  int off_live;  // tc_step_multi: the env's state between two steps (beyond both stages' buffers, never aliased)
};

// The env's state and step outputs live in this LDS record for the whole launch: live_in() fills it from the caller's
// buffers, every step reads and rewrites it (one wavefront, program order), live_out() stores it back.  The step body
// therefore has ONE form whether it is the only step of a launch (tc_step) or one of many (tc_step_multi), and the
// raster stage keeps none of it in registers.
struct LiveLds {
  double d[10];  // x, y, theta, velocity, steering, radius, front_x, front_y, cos(theta), sin(theta)
  double cte, he, reward;
  double dist[TC_MAX_LAYERS];
  int lp[8];
  int lp_len, last_maneuver;
  int have_trig;    // d[8], d[9] hold cos / sin of d[2] (set by every update of the front axle)
  int needs_reset;  // TC_F_AUTORESET: re-spawn at the start of the next step
  int cursor;       // spawn_cursor: re-spawns of this env so far
  int cursor0;      // its value in the caller's buffer (stored back only when it changed)
  int trunc, status, terminated;
  int ep_len;  // running episode's length (tc_env_set_episodes; touched by the TC_FEAT_EP kernels only)
  int cam_idx;  // the env's camera of the bank (tc_env_set_camera_bank; touched only while one is installed)
  int pad;
  int cnt[TC_MAX_TERMS];  // steps_true of the consecutive-step terms
  int ne[TC_MAX_LAYERS];
  double ep_ret;  // running episode's return (likewise)
};
#define TC_LIVE_BYTES 416
static_assert(sizeof(LiveLds) <= TC_LIVE_BYTES, "LiveLds must fit its LDS slot");

// per-step rollout outputs of tc_step_multi, already advanced to the current step (each [N] or NULL)
struct RollStep {
  double *reward, *cte, *heading_error;
  unsigned char *terminated, *truncated;
  int* status;
  double *x, *y, *theta, *velocity;
  double* dist;  // [N][C]
  int* ne;       // [N][C]
  int* lp;       // [N][8]
  int* lp_len;
  size_t row0;   // first row of the step in the [K][N] arrays above (k * N)
};

struct KArgs {
  DevMap m;
  DevCar car;
  DevCam cam;
  tc_buffers b;
  LdsLayout lds;
  int N;
  int env0;    // first env of this launch (a step may be issued as several sub-batches)
  // optional camera rows (NULL: cam.E / cam.K for every env): one per env ([N][12] / [N][9], tc_env_set_camera_per_env: row
  // = env), or a bank of cameras ([count][12] / [count][9], tc_env_set_camera_bank: row = the index that travels with the
  // (step, env), see CamBank)
  const double* cam_E;
  const double* cam_K;
  int* seg_g;  // [N][seg_cap][5] draw list of the current frame (library owned)
  int* seg_n;  // [N]
  int seg_cap;
  const tc_term* terms;  // device table [TC_MAX_TERMS] (library owned); reward / termination wrappers
  int n_terms;
  int* term_counters;    // [N][TC_MAX_TERMS] (caller owned)
  // camera layer groups: phase C handles lane-line layers grp_layer[g] .. grp_layer[g+1]-1 together (camera.py's
  // per-layer loop makes the layers independent); the LDS node buffer holds cap_nodes nodes, the largest group
  // Group g = nodes grp_n0[g] .. grp_n0[g+1]-1 and edges grp_e0[g] .. grp_e0[g+1]-1, whose layers are grp_l0[g] ..
  // grp_l1[g]-1.  Either whole layers of the map's own arrays (cam_nodes == NULL), or -- maps that need groups -- whole
  // CONNECTED COMPONENTS of the lane-line graph in the env's camera copy of the map (cam_nodes / cam_edges_g: the same
  // nodes and edges, every layer's edges still contiguous and in their original relative order, components side by
  // side): camera.py moves a node only along its own edges, so components are as independent as layers are, and a
  // group no longer has to hold the largest layer (knuffingen: 517 nodes) -- see tc_env_create.
  int n_grp;
  int grp_layer[TC_MAX_GROUPS + 1];
  int grp_n0[TC_MAX_GROUPS + 1], grp_e0[TC_MAX_GROUPS + 1];
  int grp_l0[TC_MAX_GROUPS], grp_l1[TC_MAX_GROUPS];
  const double2* cam_nodes;
  const int2* cam_edges_g;
  int cap_nodes;
  const int* spawn_tab;  // TC_F_DEVICE_SPAWN: spawnable candidate nodes (library owned), spawn_n > 0 entries
  int spawn_n;
  unsigned long long spawn_seed;
  unsigned int dbg;  // DBG_* ablation switches for the camera stage of tc_frame_kernel (0 in every other launch)
  // tc_frame_kernel: the first seg_lds_cap entries of the frame's draw list stay in LDS (byte offset seg_lds_off of the
  // workgroup's block, behind both stages' buffers) instead of going through global memory; 0 in every other launch
  int seg_lds_off, seg_lds_cap;
  int clip_merge;  // TC_CLIP_MERGE: 1 = a pair of clip passes runs as one pass where tc_clip.h allows it, 0 = always four
  // Whole-frame cull (tc_cull.h).  frame_cull: TC_FRAME_CULL, and the map has a table, and the shared camera a cover (never
  // with per-env cameras: the cover is the shared camera's); cull_tab: header + cells (library owned, camera independent)
  int frame_cull;
  // cull_rows: the pose rows of a call carry the verdict (entry TC_CULL_ROW_ENTRY, tc_cull.h): the simulate launch that writes
  // a row evaluates the predicate on the pose it stores, and the frame kernels that draw from rows read the answer there.  Set
  // where frame_cull is (cover_cull()): every frame launch draws from rows its own call's simulate launch wrote, so the two
  // are on together -- and with a camera bank or per-env cameras both are off, entry 13 neither written nor polled.  0: the
  // frame kernels draw every frame; the kernels that pose and draw in one wavefront go by frame_cull alone.
  int cull_rows;
  const unsigned char* cull_tab;
  TcCullCover cull;
};

// value of lane `l` (wave-uniform index): v_readlane instead of a shuffle through the LDS crossbar
__device__ __forceinline__ double d_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// wave-uniform value as something the compiler knows to be uniform (first active lane's copy, held in SGPRs)
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni_d(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

typedef __attribute__((address_space(3))) int* LdsIntPtr;  // (explicitly LDS: a select between it and a global pointer
                                                            // cannot be folded into one flat access)

// rank of this lane among the set bits of a wave ballot
__device__ __forceinline__ int wave_rank(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ inline unsigned int spread4(unsigned int x) {  // x < 16: 4 bits -> 4 bytes of 0x00/0xFF
  const unsigned int m = (x * 0x00204081u) & 0x01010101u;  // 24-bit multiply: full rate
  return (m << 8) - m;                                     // * 255 without v_mul_lo_u32
}

// Inclusive prefix sum over the 64 lanes with DPP moves (register to register): Hillis-Steele inside each row of 16
// (row_shr 1, 2, 4, 8, zeros shifted in), then lane 15 of a row added to the next row and lane 31 to the upper half
// (row_bcast 15 / 31) -- instead of six ds_bpermute round trips through the LDS crossbar.  All 64 lanes must be active.
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
  (void)lane;
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2 and 3
  return v;
}

// Inclusive prefix MAXIMUM of non-negative values, the same DPP moves.  The maximum is taken unsigned: 0 -- what is shifted in,
// and what a row outside the row mask receives -- is then the identity, as it is of +, and every step is one v_max_u32_dpp.
// tc_deal.h's scan.
__device__ __forceinline__ int wave_incl_max(int x) {
  unsigned int v = (unsigned int)x;
  auto mx = [](unsigned int a, unsigned int b) { return a > b ? a : b; };
  v = mx(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));   // row_shr:1
  v = mx(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));   // row_shr:2
  v = mx(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));   // row_shr:4
  v = mx(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));   // row_shr:8
  v = mx(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1 and 3
  v = mx(v, (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2 and 3
  return (int)v;
}

// Step k of a launch reads row k of the action arrays and writes row k of the rollout arrays ([nsteps][N] each).
struct MultiArgs {
  int nsteps;
  int seg_rows;  // > 1: step k writes its draw list to row k of seg_g / seg_n ([seg_rows][N] lists) for a raster launch
                 // over all (step, env) frames behind this kernel; 1: row 0 every step (same wavefront rasterises it)
  int cam_here;  // tc_env_kernel: 1 = the camera stage (draw list) runs in this kernel, 0 = not (no observation wanted,
                 // or tc_frame_kernel produces the frames from pose_rows)
  double* pose_rows;  // [nsteps][N][TC_POSE_ROW] camera.py:62 pose matrix of every (step, env) for tc_frame_kernel, or NULL
  unsigned int* resident;  // streamed call (see launch()): every workgroup counts itself in here when it starts, and the
                           // pose rows are written with device-scope stores (a frame kernel that runs BESIDE this launch
                           // polls them); NULL otherwise
  int map_lds;        // tc_envg_kernel: 1 = the lane-line edge records (end points + orientations, 48 bytes per edge) are
                      // copied into the workgroup's LDS at kernel start and phase B reads them from there
  int fat_lds;        // tc_envg_kernel: 1 = the lanepath's fat node records (96 bytes per node) sit in LDS too, behind the
                      // edge records (or at offset 0 without them), and lanepath tracking reads them there
  int grp_off, grp_stride, cnt_off;  // tc_envg_kernel: the per-env block of distances and term counters in dynamic LDS
                                     // (GroupLds, k_envg.h): env g of the workgroup at grp_off + g * grp_stride, its
                                     // counters cnt_off bytes in (plan_envg_lds, tc_plan.h)
  tc_rollout roll;
};
// (base pointers and the row: the address of a row is formed where it is stored, under its null test -- forming all 15 row
// pointers at the top of every step was ~60 scalar instructions per step of every wavefront, 4 % of cfg2)
__device__ __forceinline__ RollStep roll_at(const tc_rollout& r, size_t row0, int C) {
  RollStep q;
  q.reward = r.reward;
  q.cte = r.cte;
  q.heading_error = r.heading_error;
  q.terminated = r.terminated;
  q.truncated = r.truncated;
  q.status = r.status;
  q.x = r.x;
  q.y = r.y;
  q.theta = r.theta;
  q.velocity = r.velocity;
  q.dist = r.laneline_distances;
  q.ne = r.nearest_edge;
  q.lp = r.local_path;
  q.lp_len = r.lp_len;
  q.row0 = row0;
  return q;
}

#endif  // K_COMMON_H
