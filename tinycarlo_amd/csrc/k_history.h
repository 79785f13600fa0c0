// k_history.h -- reading frame histories out of the sample buffer (rules: tc_collect.h, definition: history_reference of
// tinycarlo_amd/collect.py; the links themselves are written by tc_collect_link / tc_collect of k_collect.h):
//   tc_history_resolve  one thread per sample walks its chain (tc_history_walk: T - 1 dependent 8-byte loads of prev and
//                       ordinal, nothing beside the frames) and leaves the slot table [B][T], optionally the table of
//                       the next-history, and the number of entries found
//   tc_gather_frames    byte frames by index into u8 / f16 / bf16 / f32, tc_unpack_bits_kernel's layout with bytes instead
//                       of bits: a lane owns ONE store and gets its V source bytes with one load, consecutive lanes store
//                       to consecutive addresses; workgroup (x, y) strides over the 256-store chunks of a frame and over
//                       the output frames; the frame's source index is one workgroup-uniform load per frame.  V = 16 / 8 /
//                       4 source bytes make a 16-byte store of u8 / f16, bf16 / f32; V = 4 is the path of frames whose size
//                       or base is no multiple of that (a 4 / 8 / 16-byte store).
// Only plain vector loads and stores.
#ifndef K_HISTORY_H
#define K_HISTORY_H

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "../../include/tinycarlo_hip.h"
#include "k_common.h"
#include "tc_collect.h"

#define TC_HISTORY_NT 256

struct ResolveArgs {
  const long long* prev;
  const long long* ordinal;
  long long capacity;
  int mode;
  int T;
  int pad;
  unsigned long long seed;
  const long long* index;
  long long n_index;
  long long* slots;       // [n_index][T]
  long long* next_slots;  // likewise, or NULL
  int* valid;             // [n_index]
};

TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_HISTORY_NT) void tc_history_resolve_walk(ResolveArgs a) {
  const long long b = (long long)blockIdx.x * TC_HISTORY_NT + threadIdx.x;
  if (b >= a.n_index) return;
  long long* row = a.slots + b * a.T;
  a.valid[b] = tc_history_walk((const int64_t*)a.prev, (const int64_t*)a.ordinal, a.mode, (uint64_t)a.seed, a.capacity, a.index[b],
                               a.T, a.pad == TC_PAD_EDGE, (int64_t*)row);
  if (a.next_slots) {  // (this thread's own stores, read back in program order)
    long long* nx = a.next_slots + b * a.T;
    nx[0] = row[0];
    for (int t = 1; t < a.T; t++) nx[t] = row[t - 1];
  }
}

// byte v -> v / 255 in the dtype, as torch's device kernel divides by a scalar: the float product with the float
// reciprocal (1.0f / 255.0f, rounded once), then one rounding to nearest-even.  (The IEEE quotient float(v) / 255.0f is
// another float for some v; sample() has always returned torch's.)
template <int DT>
__device__ __forceinline__ unsigned int gather_value(unsigned int v) {
  const float q = __fmul_rn((float)v, 1.0f / 255.0f);
  if (DT == TC_F32) return __float_as_uint(q);
  if (DT == TC_F16) return (unsigned int)__half_as_ushort(__float2half_rn(q));
  const unsigned int u = __float_as_uint(q);  // bf16 (q is finite)
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// the 4 bytes of w -> 4 elements of DT, into o[0 .. E-1] 32-bit words (E = 1 / 2 / 4)
template <int DT>
__device__ __forceinline__ void gather_word(unsigned int w, unsigned int* o) {
  if (DT == TC_U8) {
    o[0] = w;
  } else if (DT == TC_F32) {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = gather_value<DT>((w >> (8 * i)) & 255u);
  } else {
    o[0] = gather_value<DT>(w & 255u) | (gather_value<DT>((w >> 8) & 255u) << 16);
    o[1] = gather_value<DT>((w >> 16) & 255u) | (gather_value<DT>(w >> 24) << 16);
  }
}

template <int W>
struct alignas(W * 4) GatherWords {
  unsigned int w[W];
};

// V: source bytes per lane (a multiple of 4); a lane stores V elements of DT
template <int DT, int V>
__global__ __launch_bounds__(TC_HISTORY_NT) void tc_gather_frames_k(const unsigned char* src, const unsigned char* src2,
                                                                   const long long n_src, const long long frame_bytes,
                                                                   const long long* __restrict__ index, const long long n_out,
                                                                   const long long group, unsigned char* __restrict__ dst) {
  constexpr int E = DT == TC_U8 ? 1 : DT == TC_F32 ? 4 : 2;  // bytes of an element
  typedef GatherWords<V / 4> In;
  typedef GatherWords<V / 4 * E> Out;
  const long long items = frame_bytes / V;
  for (long long j = blockIdx.y; j < n_out; j += gridDim.y) {
    const long long f = index[j];
    const bool inside = f >= 0 && f < n_src;  // (workgroup-uniform)
    const unsigned char* from = src2 && j % group == 0 ? src2 : src;
    const In* sf = (const In*)(from + (inside ? f : 0) * frame_bytes);
    Out* df = (Out*)(dst + j * frame_bytes * E);
    for (long long it = (long long)blockIdx.x * TC_HISTORY_NT + threadIdx.x; it < items; it += (long long)gridDim.x * TC_HISTORY_NT) {
      In in;
#pragma unroll
      for (int i = 0; i < V / 4; i++) in.w[i] = 0;
      if (inside) in = sf[it];
      Out out;
#pragma unroll
      for (int i = 0; i < V / 4; i++) gather_word<DT>(in.w[i], &out.w[i * E]);
      df[it] = out;
    }
  }
}

#endif  // K_HISTORY_H
