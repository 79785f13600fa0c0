// k_misc.h -- the small kernels beside the stages, none of which restates a line of the reference:
//   tc_order_kernel        which env each workgroup of a single-step launch works on (heaviest frames first)
//   tc_gate_kernel         streamed call: holds the frame stream until the simulate launch is resident
//   tc_unpack_bits_kernel  packed class masks (TC_FMT_CLASSES_BITS) -> u8 / f16 / bf16 / f32, optionally gathered
// Includes k_common.h (TC_PLAIN_KERNEL, wave_incl_scan, spread4).
#ifndef K_MISC_H
#define K_MISC_H

#include "k_common.h"

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

#endif  // K_MISC_H
