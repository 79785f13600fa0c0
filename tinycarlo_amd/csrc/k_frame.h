// k_frame.h -- the kernels that draw frames with the camera and raster stages in one workgroup (camera.py:52-110,
// renderer.py:36-51):
//   tc_frame_kernel<K, THICK, FMT, RBT>    camera + raster of one (step, env) frame per workgroup, from the pose row the
//                                          simulate launch left (FrameArgs, frame_args(), frame_pose, frame_one);
//                                          tc_frame_recover_kernel draws what a gated workgroup of a streamed call gave up on;
//                                          tc_frame_banded is the K = 5 / batches-of-32 kernel for frames of several bands
//   tc_step_kernel<K, THICK, FMT, RBT, FEAT>  simulate + camera + raster of an env in one launch (step_kernel_body over
//                                          StepArgs of k_env.h); tc_drive_step_kernel is the TC_FEAT_CTRL entry point
// Includes k_camera.h, k_raster.h, k_sim.h and k_env.h.
#ifndef K_FRAME_H
#define K_FRAME_H

#include "k_camera.h"
#include "k_env.h"
#include "k_raster.h"
#include "k_sim.h"

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
// culled: the whole-frame cull's verdict on this pose, which the simulate stage left in entry TC_CULL_ROW_ENTRY when the call's
// rows carry it (KArgs::cull_rows; tc_cull.h) -- polled and validated like the others, by lane 13.  A culled frame returns
// without its pose: `pose` is then not set, and nothing moves to scalar registers.
__device__ __forceinline__ bool frame_pose(const size_t slot0, const int env, const int row, const bool wait, double* pose, int& cam_row,
                                           bool& culled) {
  const FrameArgs& fa = frame_args();
  const int tid = threadIdx.x;
  const int gate = fa.gate, bank = fa.bank;
  const bool verdict = fa.a.cull_rows != 0;
  cam_row = env;
  culled = false;
  if (gate) {
    unsigned long long* prow = (unsigned long long*)(fa.pose_rows + (slot0 + env) * TC_POSE_ROW);
    unsigned long long v = 0;
    bool give_up = wait && fa.gate == 1 && fa.gate_test > 0 && (row + env) % fa.gate_test == 0;
    long long t0 = 0;
    while (!give_up) {
      v = (tid < 12 || (tid == 12 && bank) || (tid == TC_CULL_ROW_ENTRY && verdict))
              ? __hip_atomic_load(prow + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
              : 0ull;
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
    static_assert(TC_CULL_ROW_ENTRY > 12 && TC_CULL_ROW_ENTRY < TC_POSE_ROW && TC_CULL_ROW_ENTRY < TC_NT, "a lane and a row entry of its own");
    if (__ballot(tid == TC_CULL_ROW_ENTRY && tc_cull_row_decode(v)) != 0) {  // (lane 13 holds 0 when the rows carry no verdict)
      culled = true;
      return true;
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
    if (verdict && tc_cull_row_decode(((const __attribute__((address_space(4))) unsigned long long*)(unsigned long long)pr)[TC_CULL_ROW_ENTRY])) {
      culled = true;
      return true;
    }
#pragma unroll
    for (int i = 0; i < 12; i++) pose[i] = pr[i];
    if (bank) {
      const unsigned int idx = ((const __attribute__((address_space(4))) unsigned int*)(unsigned long long)pr)[24];
      cam_row = (int)(idx < (unsigned int)bank ? idx : (unsigned int)bank - 1u);
    }
  }
  return true;
}

// Waves per SIMD the frame kernel is compiled for.  The K = 5 kernel with batches of 32 (simple_layout and the other
// small maps) is held to 96 VGPRs, five wavefronts per SIMD: its LDS plan (plan_frame_lds) leaves room for 18 workgroups
// per CU, and with four per SIMD the register file would stop at 16.
#ifndef TC_FRAME_WAVES_K5
#define TC_FRAME_WAVES_K5 5
#endif
#define TC_FRAME_WAVES(K, RBT) ((K) <= 5 ? ((RBT) == 32 ? TC_FRAME_WAVES_K5 : 4) : (K) <= 9 ? 3 : 2)
// ... and that kernel alone runs the forms that go with the plan: cam_body<K, LEAN> (one-word list entries, the camera's K
// matrix in scalar registers) and raster_body<.., FORM> (outline tables sized by the form).  Every other instantiation, and the
// recover kernel of every handle but that one's, is the code it was.
#define TC_FRAME_LEAN(K, RBT) ((K) <= 5 && (RBT) == 32)
// One frame: `rowy` is the frame's row in the launch (its step), `env` its env.
// HOT (tc_frame_kernel): the raster stage in its LDS-only form (see raster_body); !HOT (the recover kernel): the generic form.
// ONE: the handle's frames are one raster band and its camera groups one group in the register cache (raster_body's form without
// the band loop, cam_body's without the group loop).
template <int K, bool THICK, int FMT, bool HOT, int RBT, bool ONE = false>
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
    bool culled;
    if (!frame_pose(slot0, env, row, true, pose, cam_row, culled)) return;
    MapCache<K> mc;
    TSTAMP_CLEAR();
    TSTAMP(3);
    TSTAMP_REAL(30);
    cam_body<K, TC_FRAME_LEAN(K, RBT), true, ONE>(fa.a, smem, env, cam_row, pose, mc, false, tid, row, nseg, used, false, culled);
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
  raster_body<THICK, FMT, HOT, RBT, TC_FRAME_LEAN(K, RBT), ONE>(fr.r, smem, env, fr.r.obs + (size_t)rowy * fr.r.obs_row_stride, tid, slot0, nseg, used,
                                           fr.r.noise_row0 + rowy);
  {
    const FrameArgs& fe = frame_args();
    const size_t slot = (size_t)(fe.r.seg_row0 + rowy) * fe.a.N + env;
    if (tid == 0) fe.a.seg_n[slot] = nseg;  // workload statistics, the next dispatch's order, "drawn" for the recover pass
    // a streamed call's row goes back to "not written yet" for the next call (which starts behind this kernel)
    // (entry 12 with a bank, the cull's verdict in entry 13 when the rows carry it: what frame_pose polls)
    if (fe.gate && (tid < 12 || (tid == 12 && fe.bank) || (tid == TC_CULL_ROW_ENTRY && fe.a.cull_rows)))
      __hip_atomic_store((unsigned long long*)(fe.pose_rows + slot * TC_POSE_ROW) + tid, TC_POSE_EMPTY, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  TSTAMP_DUMP(env);
}

// K: slots of the camera stage's register cache per lane (a camera group has at most 64 K nodes / edges); RBT: segments per
// raster batch.  K = 5 with RBT = 16 is the variant of maps whose camera groups are packs of connected components (knuffingen:
// the map needs K = 9 as a whole or layer by layer, its component groups fit K = 5).
template <int K, bool THICK, int FMT, int RBT = RB_OF_K(K)>
__global__ __launch_bounds__(TC_NT, TC_FRAME_WAVES(K, RBT)) void tc_frame_kernel(FrameArgs fa_unused) {
  extern __shared__ __align__(16) unsigned char smem[];
  const FrameArgs& fa = frame_args();
  if ((int)blockIdx.x >= fa.a.N) return;
  const int env = fa.order ? uni_i(((const __attribute__((address_space(4))) int*)(unsigned long long)fa.order)[blockIdx.x])
                           : fa.a.env0 + (int)blockIdx.x;
  // (the five-wave kernel draws one-band frames of one camera group only: frame_kernel_of sends every other handle to tc_frame_banded)
  frame_one<K, THICK, FMT, true, RBT, TC_FRAME_LEAN(K, RBT)>(smem, env, (int)blockIdx.y);
}

// The five-wave kernel for a handle whose frames are taller than one raster band (RCam::n_bands > 1; no benchmark config: a small
// map at a large resolution) or whose camera groups are not one group in the register cache (KArgs::n_grp != 1: no handle of
// this K and batch size today): the same stages with the band loop and the group loop.  tc_frame_kernel<5, .., 32> itself is the one-band form,
// straight-line code -- the loop's invariants, set up in front of a loop that runs once, were 68 of its spilled scalar
// registers ("Scalar spills, round 17").  Exists for TC_FRAME_LEAN (K, RBT) only: every other frame kernel
// has the band loop in tc_frame_kernel, as it always had.  (Named without "_kernel": the kernel-variant matrix of the tests keeps
// a ledger of the tc_*_kernel symbols by family; this one stands beside that matrix and has its cases in
// tests/test_gpu_frame_scalars.py, one per instantiation.)
template <int K, bool THICK, int FMT, int RBT = RB_OF_K(K)>
__global__ __launch_bounds__(TC_NT, TC_FRAME_WAVES(K, RBT)) void tc_frame_banded(FrameArgs fa_unused) {
  static_assert(TC_FRAME_LEAN(K, RBT), "only the five-wave kernel has a one-band form to stand beside");
  extern __shared__ __align__(16) unsigned char smem[];
  const FrameArgs& fa = frame_args();
  if ((int)blockIdx.x >= fa.a.N) return;
  const int env = fa.order ? uni_i(((const __attribute__((address_space(4))) int*)(unsigned long long)fa.order)[blockIdx.x])
                           : fa.a.env0 + (int)blockIdx.x;
  frame_one<K, THICK, FMT, true, RBT, false>(smem, env, (int)blockIdx.y);
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

#endif  // K_FRAME_H
