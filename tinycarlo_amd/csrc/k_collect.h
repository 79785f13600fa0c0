// k_collect.h -- the kernels of the sample buffer (tc_collect; rules: tc_collect.h, definition: tinycarlo_amd/collect.py).
// A call is three launches on one stream (four in random mode), no template among them:
//   tc_collect_scan   one thread per env walks the call's rows (the state machine of rules 1-3 is sequential along k, the
//                     loads of the done rows coalesced along n); every (row, wavefront) leaves its 64 candidate flags as
//                     one ballot mask and their number
//   tc_collect_rank   one workgroup: exclusive prefix sum over the [rows][wavefronts] counts in row-major order = the rank
//                     of each wavefront's first candidate; then the counter block moves on (tc_collect_advance)
//   tc_collect_claim  random mode only: atomicMax(ordinal[slot(o)], o) for every candidate
//   tc_collect_link_* frame histories only, a pass of three launches IN FRONT of the call (tc_collect_link_scan and _rank: the
//                     scan and the rank again without moving the carry or the counters; then one thread per env links
//                     each candidate to its env's previous one); its link_rows travel through tc_collect_copy as a column
//   tc_collect_copy   one wavefront per (row, env): a candidate that is written (tc_collect_writes) moves its frame(s) with
//                     up to four 16-byte loads per lane in flight before the stores, its columns, env and ordinal.  The
//                     wavefront of (row 0, env n) reads last[n] for its sample and then stores obs[rows - 1][n] over it --
//                     the same lanes touch the same bytes in program order, which orders the call's only read-then-write
//                     of a carry array.
// Only plain vector stores and atomics.
#ifndef K_COLLECT_H
#define K_COLLECT_H

#include <hip/hip_runtime.h>

#include "../../include/tinycarlo_hip.h"
#include "k_common.h"
#include "tc_collect.h"

#define TC_COLLECT_NT 256  // threads per workgroup of every launch here (4 wavefronts)

struct CollectArgs {
  tc_collect_desc d;
  int rows;
  int waves;  // wavefronts of 64 envs per row
  int vec16;  // frames move as 16-byte words (else 4-byte)
  const unsigned char* obs_rows;
  const unsigned char* terminated;
  const unsigned char* truncated;
  long long* head;            // scratch: [0] = next_ordinal before the call, [1] = candidates of the call
  unsigned long long* mask;   // scratch: [rows][waves]
  int* base;                  // scratch: [rows][waves] counts, then exclusive ranks
};

// (COMMIT: the carry moves on; without it the pass only looks: the link pass in front of tc_collect)
template <bool COMMIT>
__device__ __forceinline__ void collect_scan(const CollectArgs& a) {
  const int n = (int)(blockIdx.x * TC_COLLECT_NT + threadIdx.x);
  const int N = a.d.num_envs;
  const bool live = n < N;  // (lanes beyond N stay in the loop: the ballot below is over whole wavefronts)
  const int w = n >> 6;
  unsigned char pending = live ? a.d.pending[n] : 0;
  int age = live ? a.d.age[n] : 0;
  for (int k = 0; k < a.rows; k++) {
    int cand = 0;
    if (live) {
      const size_t at = (size_t)k * N + n;
      const int done = (a.terminated ? a.terminated[at] : 0) | (a.truncated ? a.truncated[at] : 0);
      cand = tc_collect_env_step(&pending, &age, a.d.stride, done);
    }
    const unsigned long long m = __ballot(cand);
    if ((threadIdx.x & 63) == 0 && w < a.waves) {
      a.mask[(size_t)k * a.waves + w] = m;
      a.base[(size_t)k * a.waves + w] = __popcll(m);
    }
  }
  if (COMMIT && live) {
    a.d.pending[n] = pending;
    a.d.age[n] = age;
  }
}
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_COLLECT_NT) void tc_collect_scan(CollectArgs a) { collect_scan<true>(a); }
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_COLLECT_NT) void tc_collect_link_scan(CollectArgs a) { collect_scan<false>(a); }

template <bool COMMIT>
__device__ __forceinline__ void collect_rank(const CollectArgs& a) {
  __shared__ long long part[TC_COLLECT_NT];
  const int t = threadIdx.x;
  const long long cells = (long long)a.rows * a.waves;
  const long long per = (cells + TC_COLLECT_NT - 1) / TC_COLLECT_NT;
  const long long i0 = t * per < cells ? t * per : cells, i1 = i0 + per < cells ? i0 + per : cells;
  long long s = 0;
  for (long long i = i0; i < i1; i++) s += a.base[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < TC_COLLECT_NT; off <<= 1) {  // inclusive scan of the threads' sums
    const long long v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long long run = part[t] - s;
  for (long long i = i0; i < i1; i++) {
    const int c = a.base[i];
    a.base[i] = (int)run;
    run += c;
  }
  if (t == TC_COLLECT_NT - 1) {
    const long long c = part[t];
    a.head[0] = a.d.counters[TC_COLLECT_NEXT];
    a.head[1] = c;
    if (!COMMIT) return;
    long long ctr[4] = {a.d.counters[0], a.d.counters[1], a.d.counters[2], a.d.counters[3]};
    tc_collect_advance(a.d.mode, c, a.d.capacity, (int64_t*)ctr);
    for (int j = 0; j < 4; j++) a.d.counters[j] = ctr[j];
  }
}
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_COLLECT_NT) void tc_collect_rank(CollectArgs a) { collect_rank<true>(a); }
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_COLLECT_NT) void tc_collect_link_rank(CollectArgs a) { collect_rank<false>(a); }

// ordinal of candidate (k, n), or -1 where the row is no candidate
__device__ __forceinline__ long long collect_ordinal(const CollectArgs& a, int k, int n) {
  const size_t cell = (size_t)k * a.waves + (n >> 6);
  const unsigned long long m = a.mask[cell];
  const int bit = n & 63;
  if (!((m >> bit) & 1ull)) return -1;
  return a.head[0] + a.base[cell] + __popcll(m & ((1ull << bit) - 1ull));
}

// The link pass (tc_collect_link, frame histories): behind tc_collect_link_scan / _rank, which leave the masks, the ranks and
// head[0] of the call that tc_collect is about to make without moving the carry or the counters.  One thread per env walks
// the rows (tc_collect_chain_step beside the state machine of rules 1-3; loads and stores coalesced along n): a candidate's
// link goes to link_rows[k][n], every other entry becomes -1, the carry chain[n] moves on.
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_COLLECT_NT) void tc_collect_link_walk(CollectArgs a, long long* chain, long long* link_rows) {
  const int n = (int)(blockIdx.x * TC_COLLECT_NT + threadIdx.x);
  const int N = a.d.num_envs;
  if (n >= N) return;
  unsigned char pending = a.d.pending[n];
  int age = a.d.age[n];
  int64_t c = chain[n];
  for (int k = 0; k < a.rows; k++) {
    const size_t at = (size_t)k * N + n;
    const int done = (a.terminated ? a.terminated[at] : 0) | (a.truncated ? a.truncated[at] : 0);
    const int respawn = pending != 0;
    const int cand = tc_collect_env_step(&pending, &age, a.d.stride, done);
    const long long o = cand ? collect_ordinal(a, k, n) : -1;
    link_rows[at] = tc_collect_chain_step(&c, respawn, cand, o);
  }
  chain[n] = c;
}

TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_COLLECT_NT) void tc_collect_claim(CollectArgs a) {
  const long long p = (long long)blockIdx.x * TC_COLLECT_NT + threadIdx.x;
  if (p >= (long long)a.rows * a.d.num_envs) return;
  const int k = (int)(p / a.d.num_envs), n = (int)(p - (long long)k * a.d.num_envs);
  const long long o = collect_ordinal(a, k, n);
  if (o < 0) return;
  const long long slot = tc_collect_slot(a.d.mode, a.d.seed, o, a.d.capacity);
  if (slot >= 0) atomicMax((long long*)&a.d.ordinal[slot], o);
}

// one frame, by the 64 lanes of a wavefront (src and dst may be the same array at different frames; never __restrict__:
// the carry copy below relies on program order between a load and a later store of the same bytes)
template <class T>
__device__ __forceinline__ void collect_move(const unsigned char* src, unsigned char* dst, long long bytes, int lane) {
  const T* s = (const T*)src;
  T* d = (T*)dst;
  const long long items = bytes / (long long)sizeof(T);
  for (long long i = lane; i < items; i += 256) {
    const bool b1 = i + 64 < items, b2 = i + 128 < items, b3 = i + 192 < items;
    T v0 = s[i], v1, v2, v3;
    if (b1) v1 = s[i + 64];
    if (b2) v2 = s[i + 128];
    if (b3) v3 = s[i + 192];
    d[i] = v0;
    if (b1) d[i + 64] = v1;
    if (b2) d[i + 128] = v2;
    if (b3) d[i + 192] = v3;
  }
}
__device__ __forceinline__ void collect_frame(const CollectArgs& a, const unsigned char* src, unsigned char* dst, int lane) {
  if (a.vec16) collect_move<uint4>(src, dst, a.d.frame_bytes, lane);
  else collect_move<unsigned int>(src, dst, a.d.frame_bytes, lane);
}

TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_COLLECT_NT) void tc_collect_copy(CollectArgs a) {
  const int lane = threadIdx.x & 63;
  const long long p = uni_i((int)(((long long)blockIdx.x * TC_COLLECT_NT + threadIdx.x) >> 6));  // (rows * envs < 2^26)
  const int N = a.d.num_envs;
  if (p >= (long long)a.rows * N) return;
  const int k = (int)(p / N), n = (int)(p - (long long)k * N);
  const long long F = a.d.frame_bytes;
  const long long o = collect_ordinal(a, k, n);
  if (o >= 0) {
    const long long slot = tc_collect_slot(a.d.mode, a.d.seed, o, a.d.capacity);
    long long claimed = o;
    if (a.d.mode == TC_COLLECT_RANDOM && slot >= 0) claimed = a.d.ordinal[slot];
    if (slot >= 0 && tc_collect_writes(a.d.mode, o, a.head[0], a.head[1], a.d.capacity, claimed)) {
      const unsigned char* before = k == 0 ? a.d.last + (size_t)n * F : a.obs_rows + ((size_t)(k - 1) * N + n) * F;
      collect_frame(a, before, a.d.obs + (size_t)slot * F, lane);
      if (a.d.next_obs) collect_frame(a, a.obs_rows + ((size_t)k * N + n) * F, a.d.next_obs + (size_t)slot * F, lane);
      const size_t at = (size_t)k * N + n;
#pragma unroll
      for (int j = 0; j < TC_COLLECT_MAX_COLUMNS; j++) {  // lane j moves column j (constant indices: the block stays in SGPRs)
        if (j < a.d.n_columns && lane == j) {
          const tc_collect_column& c = a.d.columns[j];
          if (c.elem_size == 1) ((unsigned char*)c.dst)[slot] = ((const unsigned char*)c.src)[at];
          else if (c.elem_size == 4) ((unsigned int*)c.dst)[slot] = ((const unsigned int*)c.src)[at];
          else ((unsigned long long*)c.dst)[slot] = ((const unsigned long long*)c.src)[at];
        }
      }
      if (lane == 0) {
        a.d.env[slot] = n;
        a.d.ordinal[slot] = o;  // (random mode: already there)
      }
    }
  }
  // the carry: behind this wavefront's own read of last[n]
  if (k == 0) collect_frame(a, a.obs_rows + ((size_t)(a.rows - 1) * N + n) * F, a.d.last + (size_t)n * F, lane);
}

#endif  // K_COLLECT_H
