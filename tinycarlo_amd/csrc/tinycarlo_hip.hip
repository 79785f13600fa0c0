// tinycarlo_hip.hip -- libtinycarlo_hip.so: the kernel tables + C ABI (include/tinycarlo_hip.h).
//
// Build (csrc/Makefile): hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared
//
// Every kernel lives in a device-only header included below in a fixed order, each stage with its own argument block
// (k_*.h; the tc_*.h beside them are plain arithmetic that the tests also build with the host compiler):
//   k_probe.h    timing / marker probes and the ablation switches (in no shipped kernel)
//   k_common.h   LDS layout, the env's LiveLds record, KArgs / MultiArgs, wavefront helpers
//   k_feat.h     reward / termination terms, per-env cars, camera bank, episodes, controller (the FEAT template mask)
//   k_collect.h  the sample buffer's kernels (tc_collect: scan, rank, claim, copy; tc_collect_link); no env handle, no template
//   k_history.h  frame histories out of the sample buffer (tc_history_resolve; tc_gather_frames, a template compiled in part 0)
//   k_camera.h   phase C: transform -> 4 clip passes -> project -> visibility -> draw list; MapCache, FramePose, the pose row
//   k_sim.h      phases A + B of one env by one wavefront: sim_body, live_in / live_out and the other LiveLds movers
//   k_raster.h   RArgs, raster_body, tc_raster_kernel<..>: cv2.polylines of the draw list into LDS bit-planes, then the stores
//   k_noise.h    NArgs, tc_noise_kernel: NoiseObservationWrapper over a finished observation
//   k_env.h      StepArgs, tc_env_kernel<K, CAM, FEAT> / tc_drive_env_kernel: one 64-lane wavefront (= one workgroup) per env
//   k_envg.h     tc_envg_kernel<FEAT> / tc_drive_envg_kernel: the same two phases for K-step calls, 8 lanes per env
//   k_frame.h    FrameArgs, tc_frame_kernel<..> (+ recover): camera + raster of one (step, env) frame per workgroup, from the
//                pose the simulate launch left; tc_step_kernel<..> / tc_drive_step_kernel: simulate + camera + raster of an env
//   k_misc.h     tc_order_kernel, tc_gate_kernel, tc_unpack_bits_kernel
//   k_poses.h    PoseArgs, tc_pose_rows: stored poses -> pose rows, for frames drawn later (tc_render_poses)
// This file holds no device code.  It holds what needs every kernel at once -- the instantiation lists of the parts (TC_INST_*,
// TC_PART) and the tables from run-time choices to a kernel (the *_kernel_of functions) -- and then the host side (from
// `// Host side: C ABI` down).
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
#include "k_camera.h"
#include "k_sim.h"
#include "k_raster.h"
#include "k_noise.h"
#include "k_env.h"
#include "k_envg.h"
#include "k_frame.h"
#include "k_misc.h"
#include "k_poses.h"

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
  D __global__ void tc_frame_banded<5, true, TC_FMT_CLASSES_BITS, RB_OF_K(5)>(FrameArgs);                            \
  D __global__ void tc_frame_banded<5, false, TC_FMT_CLASSES_BITS, RB_OF_K(5)>(FrameArgs);                           \
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
// looped: the handle's frames need one of the loops (frame_looped()): more than one raster band, or camera groups that are not
// one group in the register cache.  The five-wave kernel (TC_FRAME_LEAN) is the one-band, one-group form and has
// tc_frame_banded, with both loops, beside it; every other frame kernel, and every recover kernel, has both loops itself
static frame_kern_t frame_kernel_of(int kcode, bool thick, int fmt, bool recover, bool looped) {
  return lift(
      [](auto kc, auto t, auto f, auto rec, auto bd) -> frame_kern_t {
        constexpr int K = FrameKRb<kc>::K, RB = FrameKRb<kc>::RB;
        if constexpr (rec) return tc_frame_recover_kernel<K, t, f, RB>;
        else if constexpr (bd && TC_FRAME_LEAN(K, RB)) return tc_frame_banded<K, t, f, RB>;
        else return tc_frame_kernel<K, t, f, RB>;
      },
      Kcodes{kcode}, Thicks{thick}, FrameFmts{fmt}, Bools{recover}, Bools{looped});
}
// K and batch size of the kernel frame_kernel_of picks for a code: what the host plans that kernel's LDS from
static int frame_k_of(int kcode) {
  return lift([](auto kc) -> int { return FrameKRb<kc>::K; }, Kcodes{kcode});
}
static int frame_rb_of(int kcode) {
  return lift([](auto kc) -> int { return FrameKRb<kc>::RB; }, Kcodes{kcode});
}
static raster_kern_t raster_kernel_of(bool thick, int fmt) {
  return lift([](auto t, auto f) -> raster_kern_t { return tc_raster_kernel<t, f>; }, Thicks{thick}, FrameFmts{fmt});
}

#endif  // part 0: the kernel tables

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
#include "tc_poses.h"

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
  int lds_pad = 0, step_lds_pad = 0, envg_lds_pad = 0;  // development builds only (TC_EXPERIMENT)
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
      {"TC_ENVG_LDS_PAD", "0", "unused LDS bytes per tc_envg_kernel workgroup (what a simulate workgroup costs the frames beside it)"},
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
  t.envg_lds_pad = atoi(sw("TC_ENVG_LDS_PAD"));
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
  // The features' kernel arguments as the handle holds them: the per-step row members of ep, ct, dr and cb stay NULL here,
  // they are a call's (tc_step_rows: step_args_at() fills them)
  EpArgs ep{};           // episodes (tc_env_set_episodes); length NULL = feature off
  DevPtr<int> ep_tab;    // device word holding max_episode_steps (updated in place), or NULL
  CtrlArgs ct{};         // built-in controller (tc_env_set_controller); tab NULL = off
  DevPtr<CtrlTab> ctrl_tab;  // device copy of the gains (updated in place), or NULL
  CtrlTab ctrl_host{};   // what ctrl_tab holds
  DriveArgs dr{};        // drive randomisation (tc_env_set_drive_randomization); tab NULL = off
  DevPtr<DriveTab> drive_tab;  // device copy of the settings (updated in place), or NULL
  DriveTab drive_host{};  // what drive_tab holds
  unsigned drive_flags = 0;  // TC_FI_DRIVE_* of every launch while it is on
  bool terms_read_dist = false;  // an installed term reads lane-line distances (term_reads_distances; tc_env_set_terms)
  CamBank cb{};          // camera bank (tc_env_set_camera_bank); index NULL = off.  k.cam_E / k.cam_K then point to the bank
  DevPtr<CamDrawTab> cam_tab;  // device copy of the draw settings (updated in place), or NULL
  CamDrawTab cam_host{};       // what cam_tab holds
  int cam_count = 0;     // cameras in the bank (0 = off)
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
  // Deferred frames (tc_render_poses; tc_env_reserve_poses): a scratch of its own for poses_cap frames per launch group --
  // pose rows, draw-list lengths, overflow room -- so that a render between two K-step calls leaves theirs alone.  Handles
  // without a frame kernel draw rounds of N frames instead: draw lists of N frames and the gathered poses as plain arrays.
  ScratchRows poses;       // (rows: unused)
  long long poses_cap = 0;  // frames per launch group; 0 = not reserved
  DevPtr<double> poses_xyt;  // [3][N] gathered x, y, theta of a round (handles without a frame kernel), else NULL
  DevPtr<int> poses_cam;     // [N] gathered camera rows of a round
  DevPtr<CamDrawTab> poses_cam_tab;  // count = N: the clamp of the gathered rows of per-env cameras
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
  // tc_frame_kernel / tc_frame_recover_kernel: their own LDS plan (plan_frame_lds, tc_plan.h), remade when the camera's
  // outline form changes (tc_env_set_camera).  frame_lds = fl.total (+ the experiments' padding); shared_frame_lds: what
  // the layout shared with the other kernels would give a frame workgroup, the plan's upper limit
  FrameLds fl;
  int plan_cap_n = 0, plan_cap_e = 0;  // nodes / edges of the largest camera group, as planned at tc_env_create
  int shared_frame_lds = 0, shared_seg_cap = 0;  // (and the head capacity that goes with them)
  int r_off_bits_k = 0;  // bit-plane offset of the fused kernels of this handle's variant (full-size tables of their batch size)
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
  e->r_off_bits_k = r_off_bits_k;
  e->plan_cap_n = cap_n;
  e->plan_cap_e = cap_e;
  e->r_lds = e->r_off_bits + align_up(dc.band_rows * row_bytes, 16);
  // the env's parked state (tc_step_multi) sits behind whichever stage needs more, so that neither aliases it
  const int r_lds_k = r_off_bits_k + align_up(dc.band_rows * row_bytes, 16);
  L.off_live = align_up(L.total > r_lds_k ? L.total : r_lds_k, 16);
  L.total = L.off_live + TC_LIVE_BYTES;
}

// items per segment of the outline tables, as a shift: 1 = the two long edges (R_F_LONG_EDGES), 2 = all four
static int outline_shift(const tc_env* e) {
  const DevCam& c = e->k.cam;
  return (!e->tune.short_edges && tc_short_edges_skip(c.thickness, c.W, c.H)) ? 1 : 2;
}
static_assert(R_OFF_BITS_SH(32, 1) == 32 * 116 + 64 * 24 && R_OFF_TAB == 0 && TC_LDS_STEP == 1280 && TC_SEG_ENTRY_BYTES == 20,
              "plan_frame_lds spells the raster tables out in plain arithmetic");

// The LDS of the frame kernels' launches.  The K = 5 kernel with batches of 32 -- compiled for five waves, with the one-word list
// entries and the form-sized raster tables (TC_FRAME_LEAN, k_frame.h) -- gets a plan of its own (plan_frame_lds), never larger
// than what grow_lds_for_draw_lists gave (cfg3: 8960 bytes instead of 10240, 18 workgroups per CU instead of 16).  Every
// other frame kernel is the code it was and keeps the layout it shares with the other kernels.
static void plan_frame(tc_env* e) {
  const DevMap& m = e->k.m;
  const DevCam& dc = e->k.cam;
  const LdsLayout& L = e->k.lds;
  const int kf = frame_k_of(e->kframe), rb = frame_rb_of(e->kframe);
  FrameLds f;
  if (TC_FRAME_LEAN(kf, rb)) {
    bool windowed = false;  // a camera group larger than the register cache (cam_body's `one` is false; never at K = 5 today)
    for (int g = 0; g < e->k.n_grp; g++)
      windowed = windowed || e->k.grp_n0[g + 1] - e->k.grp_n0[g] > kf * TC_NT || e->k.grp_e0[g + 1] - e->k.grp_e0[g] > kf * TC_NT;
    int reserve = 0;
#ifdef TC_TIMING_LDS
    reserve = 256;  // the stamp buffer (static LDS) comes out of the draw-list head: same workgroups per CU
#endif
    f = plan_frame_lds(e->plan_cap_n, e->plan_cap_e, m.total_nodes, windowed, rb, outline_shift(e), dc.band_rows * m.C * dc.wpr * 4,
                       TC_LIVE_BYTES, e->tune.seg_lds != 0, e->tune.seg_lds_limit, e->shared_frame_lds, reserve);
  } else {
    f.off_p = L.off_p, f.off_flg = L.off_flg, f.off_list = L.off_list, f.off_cnt = L.off_cnt;
    f.cam_total = L.off_cnt + 64;
    f.list_bytes = L.off_cnt - L.off_list;
    f.counters = true;
    // (where this frame kernel puts its bit-planes: behind full-size tables of its own batch size, which for a handle whose
    // fused kernels run larger batches is below the r_off_bits_k the shared layout was sized with)
    f.r_off_tab = R_OFF_TAB, f.r_off_bits = R_OFF_BITS_OF(rb);
    f.r_total = f.r_off_bits + align_up(dc.band_rows * m.C * dc.wpr * 4, 16);
    f.head_off = e->seg_lds_off;
    f.head_cap = e->shared_seg_cap;
    f.total = e->shared_frame_lds;
  }
  e->fl = f;
  e->frame_lds = f.total;
  e->frame_seg_cap = f.head_cap;
#ifdef TC_ABLATE
  if (e->tune.print_lds)
    fprintf(stderr, "tc_env_create: frame plan: camera %d raster %d (bits at %d) head at %d, %d entries, total %d (shared layout: %d)\n",
            e->fl.cam_total, e->fl.r_total, e->fl.r_off_bits, e->fl.head_off, e->fl.head_cap, e->fl.total, e->shared_frame_lds);
#endif
#ifdef TC_EXPERIMENT
  // occupancy experiments (make dev-exp, never shipped): unused LDS bytes per frame workgroup -> fewer workgroups per CU
  e->frame_lds += e->tune.lds_pad;
#endif
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
  e->shared_frame_lds = e->frame_lds;
  e->shared_seg_cap = e->frame_seg_cap;
  plan_frame(e);
#ifdef TC_EXPERIMENT
  e->step_lds += e->tune.step_lds_pad;  // (occupancy experiments: see plan_frame)
#endif
}

// The LDS of a workgroup of the grouped simulate launch (launch_envg(); plan_envg_lds, tc_plan.h), for a call whose every step runs phase B
// (`info_every`) or whose launches do so in their last step only: for launch_envg(), which asks for it, for
// raise_lds_limits() and for tc_env_envg_lds_info, which reports it.  static_bytes: of the kernel variant, 0 = not asked.
static EnvgLds envg_lds_of(const tc_env* e, bool info_every, int static_bytes) {
  int pad = 0;
#ifdef TC_EXPERIMENT
  pad = e->tune.envg_lds_pad;  // (occupancy experiments: see plan_frame)
#endif
  return plan_envg_lds(e->k.m.total_edges, e->k.m.lpN, (int)sizeof(LpNode), e->k.m.C, TC_MAX_TERMS, e->k.N,
                       TC_ENVG_NT / TC_EL, info_every, e->tune.envg_map_lds != 0, static_bytes, e->kvar != 13 ? e->frame_lds : 0, pad);
}

static int raise_lds_limits(const tc_env* e) {
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
          for (int looped = 0; looped < 2; looped++)  // (the same kernel twice where there is no looped one)
            raise((const void*)frame_kernel_of(kcode, t, fmt, false, looped), lds, "tc_frame_kernel");
        }
  // tc_envg_kernel's LDS copies of the map (edge records + fat lanepath nodes, see launch_envg()) can exceed the 48 KB default
  // (the larger form: every step reads the edge records)
  const size_t envg_lds = (size_t)envg_lds_of(e, true, 0).dynamic;
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
  // the verdict travels in the pose rows (KArgs::cull_rows): every frame launch reads rows that a simulate launch of the same
  // call wrote with this very block, so whenever the cull is on the rows carry it
  e->k.cull_rows = e->k.frame_cull;
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
  if (!bufs) {  // feature off
    const int* tab = e->ep_tab;
    memset(&e->ep, 0, sizeof(e->ep));
    e->ep.shared = tab;
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

extern "C" int tc_env_set_controller(tc_env* e, const tc_controller* c) {
  if (!e) return TC_E_INVALID;
  if (!c) {  // feature off (the table stays for a graph captured earlier); the drive randomisation goes with it
    memset(&e->ct, 0, sizeof(e->ct));
    memset(&e->dr, 0, sizeof(e->dr));
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
  const bool fresh_tab = !e->ctrl_tab;
  if (fresh_tab) HIP_TRY(e->ctrl_tab.alloc(1));
  const CtrlTab want = {c->k, c->speed};
  if (fresh_tab || memcmp(&want, &e->ctrl_host, sizeof(want)) != 0) {  // (bitwise: -0.0 is another speed than 0.0 to atan2)
    // (in place: a graph captured earlier keeps reading this table; the copy waits for launches that may still read it.
    // A call that leaves the gains as they are has nothing to wait for.)
    const CtrlTab t = want;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(e->ctrl_tab, &t, sizeof(t), hipMemcpyHostToDevice));
    e->ctrl_host = t;
  }
  e->ct.tab = e->ctrl_tab;
  e->ct.last = c->steer_last;
  return TC_OK;
}

extern "C" int tc_env_set_drive_randomization(tc_env* e, const tc_drive_randomization* d) {
  if (!d) {  // feature off (the table stays for a graph captured earlier)
    if (!e) return TC_E_INVALID;
    memset(&e->dr, 0, sizeof(e->dr));
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
    // A call that leaves the settings as they are has nothing to wait for.)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(e->drive_tab, &want, sizeof(want), hipMemcpyHostToDevice));
    e->drive_host = want;
  }
  e->dr.tab = e->drive_tab;
  e->dr.maneuver = d->n_maneuvers > 0 ? d->maneuver : nullptr;
  e->dr.episode = d->n_maneuvers > 0 ? d->episode : nullptr;
  e->dr.ou_state = d->ou_state;
  e->dr.ou_draws = d->ou_state ? d->ou_draws : nullptr;
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
  e->cam_count = 0;
  cover_cull(e);  // (per-env cameras: the cull is off, its cover is the shared camera's)
  return TC_OK;
}

extern "C" int tc_env_set_camera_bank(tc_env* e, const tc_camera_bank* b) {
  if (!e) return TC_E_INVALID;
  if (!b) {  // bank off: back to the shared camera (the table stays for a graph captured earlier)
    if (e->cb.index) e->k.cam_E = e->k.cam_K = nullptr;
    memset(&e->cb, 0, sizeof(e->cb));
    e->cam_count = 0;
    cover_cull(e);
    return TC_OK;
  }
  if (!b->E || !b->K || !b->index || !b->episode || b->count < 1) {
    set_err("tc_env_set_camera_bank: E, K, index and episode are required, and count must be at least 1");
    return TC_E_INVALID;
  }
  const CamDrawTab t = {b->seed, (unsigned int)b->count, b->env_offset};
  const bool fresh_tab = !e->cam_tab;
  if (fresh_tab) HIP_TRY(e->cam_tab.alloc(1));
  if (fresh_tab || memcmp(&t, &e->cam_host, sizeof(t)) != 0) {
    // (in place: a graph captured earlier keeps reading this table; the copy waits for launches that may still read it.
    // A call that leaves seed, count and env_offset as they are has nothing to wait for.)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(e->cam_tab, &t, sizeof(t), hipMemcpyHostToDevice));
    e->cam_host = t;
  }
  e->k.cam_E = b->E;
  e->k.cam_K = b->K;
  e->cb.index = b->index;
  e->cb.episode = b->episode;
  e->cb.tab = e->cam_tab;
  e->cam_count = b->count;
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
  if (rc == TC_OK) plan_frame(e);  // (a new thickness may change the outline form, and with it the raster tables' size)
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
  if (outline_shift(e) == 1) r.flags |= R_F_LONG_EDGES;
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

// a call's feature rows from [step][env] row r0 on
static tc_step_rows rows_at(const tc_step_rows& r, size_t r0) {
  auto at = [r0](auto* p) { return p ? p + r0 : p; };
  tc_step_rows q;
  q.n_rows = r.n_rows;  // (of the whole call: checked by tc_step_multi, not read again)
  q.steer_noise_in = at(r.steer_noise_in);
  q.steer_out = at(r.steer_out);
  q.maneuver_out = at(r.maneuver_out);
  q.ou_noise_out = at(r.ou_noise_out);
  q.episode_length_out = at(r.episode_length_out);
  q.episode_return_out = at(r.episode_return_out);
  q.camera_out = at(r.camera_out);
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
  const tc_step_rows* rows;  // the features' per-step rows (tc_step_multi), or NULL
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
// and features, mode / dtype / flags, and the control, maneuver, rollout and feature rows from [step][env] row c0 * N
// on.  What belongs to the path is left to the caller: ma.nsteps and the members of ma behind it, the scratch a.seg_g /
// a.seg_n point to, r, env_order.
static StepArgs step_args_at(const tc_env* e, const Call& c, int c0) {
  const size_t r0 = (size_t)c0 * e->k.N;
  const tc_step_rows fr = c.rows ? rows_at(*c.rows, r0) : tc_step_rows{};  // (tc_step, tc_reset: no rows)
  StepArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.a = e->k;
  sa.a.env0 = 0;
  sa.cr = e->cr;
  sa.ep = e->ep;
  sa.ep.len_rows = fr.episode_length_out;
  sa.ep.ret_rows = fr.episode_return_out;
  sa.ct = e->ct;
  sa.ct.noise = fr.steer_noise_in;
  sa.ct.rows = fr.steer_out;
  sa.cb = e->cb;
  sa.cb.rows = fr.camera_out;
  if (c.roll) sa.ma.roll = rollout_at(*c.roll, r0, (size_t)e->obs_bytes, (size_t)e->k.m.C);
  sa.mode = c.mode;
  sa.cdtype = c.cdtype;
  sa.dr = e->dr;
  sa.dr.man_rows = fr.maneuver_out;
  sa.dr.noise_rows = fr.ou_noise_out;
  sa.flags = (c.flags & ~(TC_FI_CAM_BANK | TC_FI_DRIVE | TC_FI_INFO_EVERY)) | (e->cb.index ? TC_FI_CAM_BANK : 0u) |
             (e->dr.tab ? e->drive_flags : 0u) | (c.plan.info_every ? TC_FI_INFO_EVERY : 0u);
  sa.car_control = c.cc ? (const char*)c.cc + r0 * 2 * (c.cdtype == TC_F32 ? 4 : 8) : nullptr;  // (NULL: a controller acts)
  sa.maneuver = c.man ? c.man + r0 : nullptr;  // (NULL: the maneuvers are the device's, tc_env_set_drive_randomization)
  sa.spawn_nodes = c.spawn;
  sa.mask = c.mask;
  return sa;
}

// frame_kernel_of's `looped`: a handle whose frames are taller than one raster band, or whose camera groups are not one group
// that sits in the register cache (no handle of the five-wave kernel today: a map of several groups gets K = 9 or K = 5 with
// batches of 16), draws with the kernels that keep the band loop and the group loop
static bool frame_looped(const tc_env* e) {
  const int kf = frame_k_of(e->kframe);
  return e->k.cam.n_bands > 1 || e->k.n_grp != 1 || e->k.grp_n0[1] - e->k.grp_n0[0] > kf * TC_NT || e->k.grp_e0[1] - e->k.grp_e0[0] > kf * TC_NT;
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
  // the frame kernels' own LDS plan: camera regions, raster tables of the handle's outline form, the draw-list head
  fa.a.lds.off_p = e->fl.off_p;
  fa.a.lds.off_flg = e->fl.off_flg;
  fa.a.lds.off_list = e->fl.off_list;
  fa.a.lds.off_cnt = e->fl.off_cnt;
  fa.a.lds.total = e->fl.total;
  fa.a.lds.off_live = e->fl.head_off;
  fa.r.off_tab = e->fl.r_off_tab;
  fa.r.off_bits = e->fl.r_off_bits;
  fa.a.seg_lds_off = fa.r.seg_lds_off = e->fl.head_off;
  fa.a.seg_lds_cap = fa.r.seg_lds_cap = e->fl.head_cap;
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
  // The lanepath's fat node records (96 B per node) always; the lane-line edge records (48 B per edge) only when every
  // step reads them; the per-env distances and counters behind them.  simple_layout: 17.5 KB + 2.3 KB, with the edge
  // records 12.4 KB more; knuffingen 40.2 KB (+ 34.6 KB).  128 such workgroups cover 4096 envs, one to a CU.
  const EnvgLds p = envg_lds_of(e, (sa.flags & TC_FI_INFO_EVERY) != 0, 0);
  sa.ma.map_lds = p.map_lds;
  sa.ma.fat_lds = p.fat_lds;
  sa.ma.grp_off = p.grp_off;
  sa.ma.grp_stride = p.grp_stride;
  sa.ma.cnt_off = p.cnt_off;
  hipLaunchKernelGGL(envg_kernel_of(feat), dim3(envg_grid(e->k.N)), dim3(TC_ENVG_NT), (size_t)p.dynamic, stream, sa);
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
    hipLaunchKernelGGL(frame_kernel_of(e->kframe, c.thick, c.fmt, false, frame_looped(e)), dim3(N, cn), dim3(TC_NT), e->frame_lds, fs, fa);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamWaitEvent(fs, e->sim_ev, 0));
    fa.gate = 2;
    fa.recover_rows = cn;
    fa.order = nullptr;
    hipLaunchKernelGGL(frame_kernel_of(e->kframe, c.thick, c.fmt, true, frame_looped(e)), dim3(N), dim3(TC_NT), e->frame_lds, fs, fa);
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
      hipLaunchKernelGGL(frame_kernel_of(e->kframe, c.thick, c.fmt, false, frame_looped(e)), dim3(N, rows), dim3(TC_NT), e->frame_lds, fs, fa);
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
                  const tc_step_rows* rows = nullptr) {
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
  c.main = (hipStream_t)stream; c.nsteps = nsteps; c.roll = roll; c.rows = rows; c.feat = feat;
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

// Why a call of n_steps steps cannot take these feature rows, or NULL when it can.  The struct's own faults come first:
// they are refused whatever the handle is.
static const char* rows_refusal(const tc_env* e, const tc_step_rows& r, int n_steps) {
  const bool steer = r.steer_noise_in || r.steer_out, drive = r.maneuver_out || r.ou_noise_out;
  const bool episode = r.episode_length_out || r.episode_return_out, any = steer || drive || episode || r.camera_out;
  if (r.n_rows < 0) return "the rows' n_rows must not be negative";
  if (any && r.n_rows < 1) return "rows given with n_rows = 0";
  if (any && n_steps > r.n_rows) return "more steps than the call's rows hold (tc_step_rows.n_rows)";
  if (!e) return nullptr;
  if (steer && !e->ct.tab) return "steer rows without a controller (tc_env_set_controller)";
  if (drive && !e->dr.tab) return "maneuver / OU noise rows without drive randomisation (tc_env_set_drive_randomization)";
  if (episode && !e->ep.length) return "episode rows without episode buffers (tc_env_set_episodes)";
  if (r.camera_out && !e->cb.index) return "camera rows without a camera bank (tc_env_set_camera_bank)";
  return nullptr;
}

extern "C" int tc_step_multi(tc_env* e, const void* car_control, int32_t control_dtype, const int32_t* maneuver,
                             int32_t n_steps, uint32_t flags, const tc_rollout* rollout, const tc_step_rows* rows,
                             void* stream) {
  if (const char* why = rows ? rows_refusal(e, *rows, n_steps) : nullptr) {
    set_err(std::string("tc_step_multi: ") + why);
    return TC_E_INVALID;
  }
  if (!e || (control_dtype != TC_F32 && control_dtype != TC_F64) || n_steps < 1) return TC_E_INVALID;
  if (!maneuver && !(e->dr.tab && (e->drive_flags & TC_FI_DRIVE_MAN))) return TC_E_INVALID;  // (device maneuvers replace it)
  if (!car_control && !e->ct.tab) return TC_E_INVALID;  // (a built-in controller replaces the action)
  return launch(e, MODE_STEP, car_control, control_dtype, maneuver, nullptr, nullptr, flags, stream, n_steps, rollout, rows);
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

extern "C" int tc_env_frame_lds_info(const tc_env* e, int32_t* lds_bytes, int32_t* head_entries, int32_t* workgroups_per_cu,
                                     int32_t* bits_offset) {
  if (!e) return TC_E_INVALID;
  if (lds_bytes) *lds_bytes = e->frame_lds;
  if (head_entries) *head_entries = e->fl.head_cap;
  if (bits_offset) *bits_offset = e->fl.r_off_bits;
  if (workgroups_per_cu) {
    *workgroups_per_cu = 0;
    if (e->kvar != 13) {  // (K = 13 handles have no frame kernel: plan_call)
      const DevCam& c = e->k.cam;
      int n = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)frame_kernel_of(e->kframe, c.thickness > 1, c.format, false, frame_looped(e)), TC_NT,
                                                           (size_t)e->frame_lds));
      *workgroups_per_cu = n;
    }
  }
  return TC_OK;
}

extern "C" int tc_env_envg_lds_info(const tc_env* e, int32_t info_every, int32_t* dynamic_bytes, int32_t* static_bytes,
                                    int32_t* workgroups, int32_t* frames_beside, int32_t* map_in_lds) {
  if (!e) return TC_E_INVALID;
  // the variant a K-step call of the handle as it stands would launch (launch(): the features installed)
  const unsigned feat = (e->cr.rows ? TC_FEAT_CAR : 0u) | (e->ep.length ? TC_FEAT_EP : 0u) | (e->ct.tab ? TC_FEAT_CTRL : 0u);
  hipFuncAttributes fa;
  HIP_TRY(hipFuncGetAttributes(&fa, (const void*)envg_kernel_of(feat)));
  const EnvgLds p = envg_lds_of(e, info_every != 0 || e->terms_read_dist || e->tune.info_every, (int)fa.sharedSizeBytes);
  if (dynamic_bytes) *dynamic_bytes = p.dynamic;
  if (static_bytes) *static_bytes = p.static_bytes;
  if (workgroups) *workgroups = p.workgroups;
  if (frames_beside) *frames_beside = p.frames_beside;
  if (map_in_lds) *map_in_lds = p.map_lds;
  return TC_OK;
}

extern "C" int tc_env_frame_bands(const tc_env* e, int32_t* n_bands, int32_t* band_rows) {
  if (!e) return TC_E_INVALID;
  if (n_bands) *n_bands = e->k.cam.n_bands;
  if (band_rows) *band_rows = e->k.cam.band_rows;
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

// ---------------------------------------------------------------------------------------------
// Deferred frames: observations drawn from stored poses (k_poses.h, tc_poses.h; DESIGN.md "Deferred frames").

// a handle whose K-step calls draw with a frame kernel (plan_call's can_frames); the others draw deferred frames the way
// tc_render draws theirs: the camera stage inside tc_env_kernel, tc_raster_kernel behind it
static bool has_frame_kernel(const tc_env* e) { return e->tune.fuse && e->kvar != 13; }

extern "C" int tc_env_reserve_poses(tc_env* e, int64_t max_frames) {
  if (!e || max_frames < 1) {
    set_err("tc_env_reserve_poses: need an env and max_frames >= 1");
    return TC_E_INVALID;
  }
  const bool frames = has_frame_kernel(e);
  const size_t N = (size_t)e->k.N;
  // per frame: a pose row (128 B), a draw-list length and room for a draw list (20 B x lane-line edges of the map), within
  // the budget of the streamed calls' scratch (tune.scratch_bytes); handles without a frame kernel: rounds of N frames
  const double per_frame = (double)e->k.seg_cap * 5 * sizeof(int) + sizeof(int) + TC_POSE_ROW * sizeof(double);
  long long cap = max_frames < TC_POSES_MAX_CAPACITY ? (long long)max_frames : TC_POSES_MAX_CAPACITY;
  if ((double)cap * per_frame > e->tune.scratch_bytes) cap = (long long)(e->tune.scratch_bytes / per_frame);
  if (cap < 1) cap = 1;
  if (!frames) cap = (long long)N;
  if (e->poses_cap >= cap) return TC_OK;
  HIP_TRY(hipDeviceSynchronize());  // an earlier render may still use the old arrays
  e->poses = ScratchRows();
  e->poses_cap = 0;
  ScratchRows s;
  DevPtr<double> xyt;
  DevPtr<int> cam;
  DevPtr<CamDrawTab> tab;
  hipError_t he = s.seg_g.alloc((size_t)cap * e->k.seg_cap * 5);
  if (he == hipSuccess) he = s.seg_n.alloc((size_t)cap);
  if (he == hipSuccess) he = hipMemset(s.seg_n, 0, (size_t)cap * sizeof(int));
  if (he == hipSuccess && frames) he = s.pose.alloc((size_t)cap * TC_POSE_ROW);
  if (he == hipSuccess && !frames) he = xyt.alloc(3 * N);
  if (he == hipSuccess && !frames) he = cam.alloc(N);
  if (he == hipSuccess && !frames) he = tab.alloc(1);
  if (he == hipSuccess && !frames) {
    const CamDrawTab t = {0ull, (unsigned int)N, 0u};
    he = hipMemcpy(tab, &t, sizeof(t), hipMemcpyHostToDevice);
  }
  if (he != hipSuccess) {
    (void)hipGetLastError();
    set_err(std::string("hipMalloc(scratch of deferred frames): ") + hipGetErrorString(he));
    return TC_E_NOMEM;
  }
  e->poses = std::move(s);
  if (!frames) {
    e->poses_xyt = std::move(xyt);
    e->poses_cam = std::move(cam);
    e->poses_cam_tab = std::move(tab);
  }
  e->poses_cap = cap;
  return TC_OK;
}

// one launch group on a handle with a frame kernel: the pose rows, then one frame workgroup per row
static int launch_pose_frames(tc_env* e, PoseArgs& pa, const PoseGroup& g, int cam_rows, uint8_t* out, hipStream_t st) {
  pa.first = g.first;
  pa.n = g.count;
  pa.rows = e->poses.pose;
  hipLaunchKernelGGL(tc_pose_rows, dim3((unsigned)g.pose_blocks), dim3(TC_POSES_NT), 0, st, pa);
  HIP_TRY(hipGetLastError());
  const DevCam& c = e->k.cam;
  RArgs r = make_rargs(e, e->poses.seg_g, e->poses.seg_n, e->k.seg_cap, nullptr, 0, 0, out + (size_t)g.first * (size_t)e->obs_bytes, false);
  r.N = g.count;
  FrameArgs fa = frame_args_of(e, 0, r, false);
  // one grid row as wide as the group: slot m of the scratch is workgroup m, and no workgroup stands for a frame beyond the list
  fa.a.N = g.count;
  fa.a.seg_g = e->poses.seg_g;
  fa.a.seg_n = e->poses.seg_n;
  fa.pose_rows = e->poses.pose;
  fa.gate = 0;
  fa.order = nullptr;
  fa.bank = cam_rows;  // (per-env cameras too: the row comes from entry 12, not from the slot)
  hipLaunchKernelGGL(frame_kernel_of(e->kframe, c.thickness > 1, c.format, false, frame_looped(e)), dim3((unsigned)g.count), dim3(TC_NT),
                     e->frame_lds, st, fa);
  HIP_TRY(hipGetLastError());
  return TC_OK;
}

// one round on a handle without a frame kernel, the form tc_render has there: the poses gathered into plain arrays, a copy of
// the launch arguments whose x / y / theta (and camera index) are those arrays, tc_env_kernel<K, CAM> in MODE_RENDER over the
// round's slots and tc_raster_kernel behind it, both into the scratch's draw lists
static int launch_pose_round(tc_env* e, PoseArgs& pa, const PoseGroup& g, int cam_rows, uint8_t* out, hipStream_t st) {
  const size_t N = (size_t)e->k.N;
  pa.first = g.first;
  pa.n = g.count;
  pa.rows = nullptr;
  pa.gx = e->poses_xyt;
  pa.gy = e->poses_xyt + N;
  pa.gth = e->poses_xyt + 2 * N;
  pa.gcam = e->poses_cam;
  hipLaunchKernelGGL(tc_pose_rows, dim3((unsigned)g.pose_blocks), dim3(TC_POSES_NT), 0, st, pa);
  HIP_TRY(hipGetLastError());
  uint8_t* obs = out + (size_t)g.first * (size_t)e->obs_bytes;
  StepArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.a = e->k;
  sa.a.env0 = 0;
  sa.a.b.x = pa.gx;
  sa.a.b.y = pa.gy;
  sa.a.b.theta = pa.gth;
  sa.a.b.obs = obs;
  sa.a.seg_g = e->poses.seg_g;
  sa.a.seg_n = e->poses.seg_n;
  sa.mode = MODE_RENDER;
  sa.cdtype = TC_F32;
  if (cam_rows > 0) {  // the slot's camera row is the gathered one: a bank's index, or the env of per-env cameras
    sa.flags = TC_FI_CAM_BANK;
    sa.cb.index = pa.gcam;
    sa.cb.tab = e->cb.index ? (const CamDrawTab*)e->cam_tab : (const CamDrawTab*)e->poses_cam_tab;
  }
  sa.ma.nsteps = 1;
  sa.ma.cam_here = 1;
  hipLaunchKernelGGL(env_kernel_of(e->kvar, true, 0u), dim3((unsigned)g.count), dim3(TC_NT), e->k.lds.total, st, sa);
  HIP_TRY(hipGetLastError());
  return launch_raster(e, e->poses.seg_g, e->poses.seg_n, e->k.seg_cap, nullptr, 0, st, 0, g.count, obs, false);
}

extern "C" int tc_render_poses(tc_env* e, const double* x, const double* y, const double* theta, const int32_t* camera,
                               const int64_t* index, int64_t n_src, int64_t n_frames, uint8_t* out, void* stream) {
  // (every check comes before the first HIP call, and those of the arguments alone before the handle is looked at: a bad
  // argument is reported on a machine without a device too)
  auto bad = [](const char* what) {
    set_err(std::string("tc_render_poses: ") + what);
    return TC_E_INVALID;
  };
  auto mis = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
  if (!x || !y || !theta || !out) return bad("x, y, theta and out are required");
  if (n_src < 1) return bad("n_src must be at least 1");
  if (n_frames < 0) return bad("n_frames must not be negative");
  if (!index && n_frames > n_src) return bad("without an index n_frames must not exceed n_src");
  if (mis(out, 16)) return bad("out must be 16-byte aligned, like the obs rows of a rollout");
  if (mis(x, 8) || mis(y, 8) || mis(theta, 8) || mis(index, 8) || mis(camera, 4)) return bad("x, y, theta and index must be 8-byte, camera 4-byte aligned");
  if (!e) return bad("no env");
  const int cam_rows = e->cb.index ? e->cam_count : (e->k.cam_E ? e->k.N : 0);
  if (cam_rows == 0 && camera) return bad("camera given on a handle with the one shared camera");
  if (cam_rows > 0 && !camera)
    return bad(e->cb.index ? "a handle with a camera bank needs camera (the bank index of every pose)"
                           : "a handle with per-env cameras needs camera (the env whose camera every pose takes)");
  if (n_frames == 0) return TC_OK;
  if (e->poses_cap < 1)
    return bad("needs its scratch: call tc_env_reserve_poses(env, max_frames) once before (the call itself never allocates)");
  const bool frames = has_frame_kernel(e);
  if (!frames && !e->bound) {
    set_err("tc_render_poses: a handle without a frame kernel draws with the simulate kernel's camera stage, which reads the bound buffers: tc_env_bind first");
    return TC_E_UNBOUND;
  }
  int rc = check_stamp_buffer(e);
  if (rc != TC_OK) return rc;
#ifdef TC_TIMING
  // (a frame workgroup stamps the row of its slot, and a group has up to poses_cap slots)
  if (g_tstamp && frames && e->poses_cap > g_tstamp_n) return bad("timing build: the installed stamp buffer is smaller than a launch group");
#endif
  const hipStream_t st = (hipStream_t)stream;
  // (the groups of a render reuse the scratch in stream order; renders on different streams are the caller's to order)
  PoseArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.a = e->k;
  pa.x = x;
  pa.y = y;
  pa.theta = theta;
  pa.camera = camera;
  pa.index = (const long long*)index;
  pa.n_src = n_src;
  pa.cam_rows = cam_rows;
  const long long groups = pose_group_count(n_frames, e->poses_cap);
  for (long long gi = 0; gi < groups; gi++) {
    const PoseGroup g = pose_group_at(n_frames, e->poses_cap, gi, TC_POSES_NT);
    rc = frames ? launch_pose_frames(e, pa, g, cam_rows, out, st) : launch_pose_round(e, pa, g, cam_rows, out, st);
    if (rc != TC_OK) return rc;
  }
  return TC_OK;
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
