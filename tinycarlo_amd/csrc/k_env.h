// k_env.h -- the per-env simulate kernels: one 64-lane wavefront (= one workgroup) per env runs sim_body (k_sim.h: car.py,
// layer.py) for every step of the launch, with the camera stage (k_camera.h) behind each step when CAM.  Holds StepArgs,
// the one argument block of every kernel that simulates (it embeds RArgs, hence k_raster.h), with the step_lane() /
// step_args() / wants_frame() idiom that the grouped and the fused kernels (k_envg.h, k_frame.h) share, then
// env_kernel_body<K, CAM, FEAT>, tc_env_kernel and tc_drive_env_kernel (the TC_FEAT_CTRL entry point).  Includes k_sim.h
// (and through it k_camera.h, k_feat.h) and k_raster.h.
#ifndef K_ENV_H
#define K_ENV_H

#include "k_camera.h"
#include "k_raster.h"
#include "k_sim.h"

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

#ifndef TC_MIN_WAVES
#define TC_MIN_WAVES 4
#endif
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
        // the whole-frame cull's verdict on this pose, for the frame kernel that draws from the row (KArgs::cull_rows)
        if (sa.a.cull_rows) ((unsigned long long*)o)[TC_CULL_ROW_ENTRY] = cam_cull_row(step_args().a, pose);
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

#endif  // K_ENV_H
