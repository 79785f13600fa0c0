// k_noise.h -- NoiseObservationWrapper (wrapper/observation.py:15-27) as a pass over a finished class-mask observation:
// the argument block NArgs, tc_noise_tick (the device counter of passes), fdiv and tc_noise_kernel.  (The same blobs
// fused into the raster stage are raster_body's, k_raster.h.)  Includes k_common.h and tc_rng.h (the blob draws).
#ifndef K_NOISE_H
#define K_NOISE_H

#include "k_common.h"
#include "tc_rng.h"

// ---------------------------------------------------------------------------------------------
// NoiseObservationWrapper (wrapper/observation.py:15-27) as a pass over a finished class-mask observation.
// Every operation of the reference is per pixel -- obs[c] |= obs[src] & circle, or obs[c] &= ~circle -- so rows are
// independent: the frame is taken through LDS as bit-planes band by band (same layout as the rasteriser), the blobs
// are applied to the band in order, and the band is written back.  A filled cv2.circle whose centre lies inside the
// image is, row by row, the span centre +- hw[radius][|row - cy|] clipped to the image (Circle() of drawing.cpp paints
// symmetric spans and its bounding-box tests never reject a row when the centre is inside); hw is tabulated on the
// host by running that midpoint algorithm once per radius.
struct NArgs {
  int N, C, H, W, wpr, band_rows, n_bands;
  unsigned char* obs;
  const int* blobs;  // [N][C * n_blobs][5] or NULL: drawn here (tc_rng.h)
  int n_blobs, max_radius;
  const unsigned char* hw;  // [max_radius][max_radius]: half width of row offset t of the circle of radius r
  unsigned long long seed;
  const unsigned int* step;  // device counter of noise passes so far (advanced by tc_noise_tick on the same stream:
                             // a kernel argument would be frozen into a captured HIP graph and replay the same blobs)
  unsigned int inv_cpr;  // 2^32 / (W / 16) + 1, for fdiv by the 16-pixel chunks per row
};

TC_PLAIN_KERNEL __global__ void tc_noise_tick(unsigned int* step, unsigned int n) { *step += n; }

// q / d for q < 2^31 with inv = 2^32 / d + 1 (host): one multiply-high and a fix-up instead of a ~30-instruction
// runtime division (as first written this kernel spent most of its ~12 k instructions per wavefront dividing indices)
__device__ __forceinline__ int fdiv(int q, int d, unsigned int inv) {
  int e = (int)__umulhi((unsigned int)q, inv);
  e -= (e * d > q);
  e += ((e + 1) * d <= q);
  return e;
}

// LDS: bit-planes of one band | blob rows [nb][5] | per blob the span-table row of its radius [nb][max_radius]
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_NT) void tc_noise_kernel(NArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int env = blockIdx.x, tid = threadIdx.x;
  if (env >= a.N) return;
  const int C = a.C, H = a.H, W = a.W, wpr = a.wpr;
  const int nb = C * a.n_blobs;
  unsigned int* bits = (unsigned int*)smem;
  int* lb = (int*)(smem + (size_t)C * a.band_rows * wpr * 4);
  unsigned char* lhw = (unsigned char*)(lb + nb * 5);
  unsigned char* out = a.obs + (size_t)env * ((size_t)C * H * W);

  // All blobs of this env at once, one per lane: the draws (or the caller's rows) and, behind them, each blob's row of
  // the span table, so that the blob loop touches nothing but LDS.
  for (int k = tid; k < nb; k += TC_NT) {
    tc_blob bl;
    if (a.blobs) {
      const int* p = a.blobs + ((size_t)env * nb + k) * 5;
      bl.x = p[0];
      bl.y = p[1];
      bl.r = p[2];
      bl.mode = p[3];
      bl.src = p[4];
    } else {
      bl = tc_noise_blob(a.seed, (uint32_t)env, *a.step, (uint32_t)k, W, H, a.max_radius, C);
    }
    // caller-provided lists are not trusted with LDS indices: an invalid row becomes a blob that touches nothing.
    // src only matters on the copy branch: erase blobs carry src = -1 in the reference's draw order (nothing is drawn
    // for them, observation.py:25-26) and must stay erasers.
    const bool ok = bl.r >= 1 && bl.r < a.max_radius && (unsigned)bl.x < (unsigned)W && (unsigned)bl.y < (unsigned)H &&
                    (bl.mode == 0 || (unsigned)bl.src < (unsigned)C);
    lb[5 * k] = bl.x;
    lb[5 * k + 1] = bl.y;
    lb[5 * k + 2] = ok ? bl.r : -1;
    lb[5 * k + 3] = bl.mode;
    lb[5 * k + 4] = (ok && bl.mode != 0) ? bl.src : 0;
  }
  __syncthreads();
  for (int k = 0; k < nb; k++) {  // row k of lhw = row r_k of the table, entries 0 .. r_k
    const int r = lb[5 * k + 2];
    for (int t = tid; t <= r; t += TC_NT) lhw[k * a.max_radius + t] = a.hw[r * a.max_radius + t];
  }

  // this lane's place in a pass over (row, 32-bit word) and over (row, 16-pixel chunk): fixed for the whole kernel
  const int lw = wpr <= TC_NT ? wpr : TC_NT;           // words of a row handled side by side
  const int w_lane = tid % lw, r_lane = tid / lw, r_step = TC_NT / lw;
  const bool w16 = (W & 15) == 0;                      // rows are whole 16-byte chunks: one lane per chunk, coalesced
  const int cpr = W >> 4;
  for (int band = 0; band < a.n_bands; band++) {
    const int y0 = band * a.band_rows;
    const int rows = (y0 + a.band_rows < H ? y0 + a.band_rows : H) - y0;
    if (w16) {  // bytes (0 / 255) -> bits, 16 pixels per lane
      const int per_plane = rows * cpr;
      for (int c = 0; c < C; c++) {
        const unsigned char* pl = out + ((size_t)c * H + y0) * W;  // the band's rows of a plane are contiguous
        for (int q = tid; q < per_plane; q += TC_NT) {
          const int row = fdiv(q, cpr, a.inv_cpr), ch = q - row * cpr;
          const uint4 v = *(const uint4*)(pl + (size_t)q * 16);
          const unsigned int h = ((((v.x & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) |
                                 (((((v.y & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) << 4) |
                                 (((((v.z & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) << 8) |
                                 (((((v.w & 0x01010101u) * 0x10204080u) >> 28) & 0xfu) << 12);
          ((unsigned short*)bits)[((c * a.band_rows + row) * wpr) * 2 + ch] = (unsigned short)h;
        }
      }
    } else {
      for (int c = 0; c < C; c++)
        for (int row = r_lane; row < rows; row += r_step)
          for (int w = w_lane; w < wpr; w += lw) {
            const unsigned char* src = out + ((size_t)c * H + y0 + row) * W + w * 32;
            unsigned int word = 0;
            for (int j = 0; j < 32 && w * 32 + j < W; j++) word |= (src[j] ? 1u : 0u) << j;
            bits[(c * a.band_rows + row) * wpr + w] = word;
          }
    }
    __syncthreads();
    int c = 0, left = a.n_blobs;  // plane of blob k = k / n_blobs, kept by counting
    for (int k = 0; k < nb; k++) {  // wrapper/observation.py:16-26, blob after blob
      const int bx = lb[5 * k], by = lb[5 * k + 1], br = lb[5 * k + 2], mode = lb[5 * k + 3], bsrc = lb[5 * k + 4];
      const int ylo = by - br > y0 ? by - br : y0;
      const int yhi = br >= 1 ? (by + br < y0 + rows - 1 ? by + br : y0 + rows - 1) : ylo - 1;
      const unsigned char* hwk = lhw + k * a.max_radius;
      for (int row = ylo + r_lane; row <= yhi; row += r_step) {
        const int t = row > by ? row - by : by - row;
        const int hw = hwk[t];
        int xl = bx - hw, xr = bx + hw;
        xl = xl < 0 ? 0 : xl;
        xr = xr > W - 1 ? W - 1 : xr;
        for (int w = w_lane; w < wpr; w += lw) {
          const int b0 = xl > w * 32 ? xl - w * 32 : 0, b1 = xr < w * 32 + 31 ? xr - w * 32 : 31;
          if (b1 < b0) continue;
          const unsigned int mask = (b1 - b0 == 31) ? 0xffffffffu : (((1u << (b1 - b0 + 1)) - 1u) << b0);
          const int ic = (c * a.band_rows + row - y0) * wpr + w;
          if (mode)
            bits[ic] |= bits[(bsrc * a.band_rows + row - y0) * wpr + w] & mask;  // observation.py:22-24
          else
            bits[ic] &= ~mask;  // observation.py:26
        }
      }
      __syncthreads();  // the next blob may read what this one wrote
      if (--left == 0) {
        c++;
        left = a.n_blobs;
      }
    }
    if (w16) {  // bits -> bytes, one 16-byte store per lane
      const int per_plane = rows * cpr;
      for (int cc = 0; cc < C; cc++) {
        unsigned char* pl = out + ((size_t)cc * H + y0) * W;
        for (int q = tid; q < per_plane; q += TC_NT) {
          const int row = fdiv(q, cpr, a.inv_cpr), ch = q - row * cpr;
          const unsigned int h = ((const unsigned short*)bits)[((cc * a.band_rows + row) * wpr) * 2 + ch];
          uint4 o;
          o.x = spread4(h & 15u);
          o.y = spread4((h >> 4) & 15u);
          o.z = spread4((h >> 8) & 15u);
          o.w = spread4((h >> 12) & 15u);
          *(uint4*)(pl + (size_t)q * 16) = o;
        }
      }
    } else {
      for (int cc = 0; cc < C; cc++)
        for (int row = r_lane; row < rows; row += r_step)
          for (int w = w_lane; w < wpr; w += lw) {
            unsigned char* dst = out + ((size_t)cc * H + y0 + row) * W + w * 32;
            const unsigned int word = bits[(cc * a.band_rows + row) * wpr + w];
            for (int j = 0; j < 32 && w * 32 + j < W; j++) dst[j] = (word >> j) & 1u ? 255 : 0;
          }
    }
    __syncthreads();
  }
}

#endif  // K_NOISE_H
