// k_probe.h -- the probes every stage carries and no shipped kernel contains: TSTAMP* / TSTAMP_DUMP (shader-clock stamps of
// the timing builds, tools/phase_clock.py), MARK (section marks of tools/kernel_stats.py --sections) and the DBG_* ablation
// switches with DBG_ON (make dev-ablate).  Defines no kernel and mirrors nothing of the reference.
#ifndef K_PROBE_H
#define K_PROBE_H

#include <hip/hip_runtime.h>

// Timing build only (make timing -> libtinycarlo_hip_timing.so, used by tools/phase_clock.py): every wavefront stores
// the shader clock at its phase boundaries.  The shipped library is compiled without TC_TIMING and contains none of it.
#if defined(TC_TIMING) && defined(TC_TIMING_LOOP)
// variant of the timing build (make dev-timing-loop): no phase probes, only the period of every step of a K-step launch
// (slot k = clocks from the top of step k-1 to the top of step k, k < 32; slot 0 = launch entry -> top of step 0)
__device__ long long* tc_tstamp = nullptr;
#define TSTAMP(i) \
  do {            \
  } while (0)
#define TSTAMP_REAL(i) \
  do {                 \
  } while (0)
#define TSTAMP_LOOP(k, nsteps, tprev)                                                      \
  do {                                                                                     \
    long long _t = clock64();                                                              \
    long long* _tp = tc_tstamp;                                                            \
    if (_tp && threadIdx.x == 0 && (k) < 31) _tp[(size_t)env * 32 + (k)] = _t - (tprev);  \
    (tprev) = _t;                                                                          \
  } while (0)
#define TSTAMP_END(tprev)                                                                  \
  do {                                                                                     \
    long long* _tp = tc_tstamp;                                                            \
    if (_tp && threadIdx.x == 0) {                                                         \
      _tp[(size_t)env * 32 + 31] = clock64() - (tprev);                                    \
      _tp[(size_t)env * 32 + 30] = (long long)(unsigned)__builtin_amdgcn_s_getreg(63492) | /* HW_REG_HW_ID */ \
                                   ((long long)(unsigned)__builtin_amdgcn_s_getreg(63508) << 32); /* XCC_ID */ \
    }                                                                                      \
  } while (0)
#elif defined(TC_TIMING) && defined(TC_TIMING_LDS)
// Variant for the frame / step kernels (make dev-timing-lds): the stamps go to 256 bytes of LDS -- no vector-memory
// operation, nothing drained -- and one lane copies them out when the frame is done.  A stamp written with a global store
// (the variant below) puts that store's round trip into the NEXT s_waitcnt vmcnt(0) of the wavefront, i.e. the probes
// themselves create the longest "phase" of a wavefront that otherwise has no store in flight; this variant shows the
// latencies the shipped kernel has.  (s_memtime returns through the scalar-memory counter, so a stamp still waits for the
// LDS queue: almost every probe sits behind an lds_sync anyway.)
__device__ long long* tc_tstamp = nullptr;  // [N][32]
__shared__ long long tc_ts_lds[32];
#define TSTAMP(i)                                              \
  do {                                                         \
    if (threadIdx.x == 0) tc_ts_lds[(i)] = clock64();          \
  } while (0)
#define TSTAMP_REAL(i)                                         \
  do {                                                         \
    if (threadIdx.x == 0) tc_ts_lds[(i)] = wall_clock64();     \
  } while (0)
#define TSTAMP_LOOP(k, nsteps, tprev) \
  do {                                \
  } while (0)
#define TSTAMP_END(tprev) \
  do {                    \
  } while (0)
#define TSTAMP_DUMP(env_)                                                                  \
  do {                                                                                     \
    long long* _tp = tc_tstamp;                                                            \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                     \
    if (_tp && threadIdx.x < 32) _tp[(size_t)(env_) * 32 + threadIdx.x] = tc_ts_lds[threadIdx.x]; \
  } while (0)
#define TSTAMP_CLEAR()                                         \
  do {                                                         \
    if (threadIdx.x < 32) tc_ts_lds[threadIdx.x] = 0;          \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         \
  } while (0)
#elif defined(TC_TIMING)
__device__ long long* tc_tstamp = nullptr;  // [N][32]
// (outstanding memory operations are drained first, so a phase is charged with the latencies it started)
#define TSTAMP(i)                                                                          \
  do {                                                                                     \
    long long* _tp = tc_tstamp;                                                            \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                            \
    if (_tp && threadIdx.x == 0) _tp[(size_t)env * 32 + (i)] = clock64();                  \
  } while (0)
// the constant 100 MHz counter next to the shader clock: (stamp 13 - stamp 0) / (stamp 31 - stamp 30) x 100 MHz is the
// clock the chip actually holds while the kernel runs
// loop period of the step loop: slot 28 = clocks from the top of the previous step to the top of the last one
#define TSTAMP_LOOP(k, nsteps, tprev)                                                      \
  do {                                                                                     \
    long long _t = clock64();                                                              \
    long long* _tp = tc_tstamp;                                                            \
    if (_tp && threadIdx.x == 0 && (k) == (nsteps)-1 && (k) > 0) _tp[(size_t)env * 32 + 28] = _t - (tprev); \
    (tprev) = _t;                                                                          \
  } while (0)
#define TSTAMP_REAL(i)                                                                     \
  do {                                                                                     \
    long long* _tp = tc_tstamp;                                                            \
    if (_tp && threadIdx.x == 0) _tp[(size_t)env * 32 + (i)] = wall_clock64();            \
  } while (0)
#define TSTAMP_END(tprev) \
  do {                    \
  } while (0)
#elif defined(TC_MARKERS)
// tools/kernel_stats.py --sections: the probes become assembler comments, so that the static instruction mix between two
// probes can be read off the compiler's output (no code is emitted for them)
#define TC_STR2(x) #x
#define TC_STR(x) TC_STR2(x)
#define TSTAMP(i) asm volatile("; @@TS " TC_STR(i) ::: "memory")
#define TSTAMP_REAL(i) \
  do {                 \
  } while (0)
#define TSTAMP_LOOP(k, nsteps, tprev) \
  do {                                \
  } while (0)
#define TSTAMP_END(tprev) \
  do {                    \
  } while (0)
#else
#define TSTAMP(i) \
  do {            \
  } while (0)
#define TSTAMP_REAL(i) \
  do {                 \
  } while (0)
#define TSTAMP_LOOP(k, nsteps, tprev) \
  do {                                \
  } while (0)
#define TSTAMP_END(tprev) \
  do {                    \
  } while (0)
#endif
#ifndef TSTAMP_DUMP
#define TSTAMP_DUMP(env_) \
  do {                    \
  } while (0)
#define TSTAMP_CLEAR() \
  do {                 \
  } while (0)
#endif
// finer section marks for tools/kernel_stats.py --sections (nothing in any other build)
#ifdef TC_MARKERS
#define MARK(name) asm volatile("; @@MK " name ::: "memory")
#else
#define MARK(name) \
  do {             \
  } while (0)
#endif

// ablation switches for profiling (not part of the ABI contract; results are wrong when set)
#define DBG_SKIP_RASTER 0x100u
#define DBG_SKIP_STORE 0x200u
#define DBG_SKIP_CAMERA 0x400u
#define DBG_SKIP_DIST 0x800u
#define DBG_SKIP_R2 0x1000u
#define DBG_SKIP_R3 0x2000u
#define DBG_SKIP_R4 0x4000u
#define DBG_SKIP_EVENTS 0x10000u
#define DBG_SKIP_LINESETUP 0x20000u
#define DBG_SKIP_SLOPE 0x40000u
#define DBG_SKIP_QUAD 0x80000u
#define DBG_SKIP_CLIP 0x100000u
#define DBG_SKIP_DRAWLIST 0x200000u
// not an ablation switch: set by make_rargs in RArgs.flags when ThickLine needs only its two long outline edges
// (tc_short_edges_skip of tc_line.h holds for the camera and TC_SHORT_EDGES is 0); never part of a caller's flags
#define R_F_LONG_EDGES 0x40000000u
// the kernels test them only in the ablation build (make dev-ablate): in the shipped library every test folds to false,
// so the switches cost no scalar registers there (they were ~25 live conditions at the head of the raster stage)
#ifdef TC_ABLATE
#define DBG_ON(word, f) (((word) & (f)) != 0)
#else
#define DBG_ON(word, f) false
#endif

#endif  // K_PROBE_H
