// k_raster.h -- the raster stage (renderer.py:36-51): cv2.polylines of a frame's draw list into LDS bit-planes (the line
// and fill walkers of tc_line.h / tc_fill.h, through tc_device.h), expanded to uint8 and stored with 16-byte-per-lane
// coalesced stores (zeros included: a class-mask frame is written exactly once), or stored as the packed words themselves
// (TC_FMT_CLASSES_BITS).  Holds the stage's argument block (RCam, RArgs), its tunables (TC_RASTER_WAVES, TC_BAND_VMCNT),
// tc_obs_bytes_of, TC_FMT_IS_CLASSES, the packed-word stores, raster_body<THICK, FMT, LDSONLY, RB> and the kernel of the
// stage alone, tc_raster_kernel<THICK, FMT>; tc_frame_kernel and tc_step_kernel (k_frame.h) run raster_body behind the
// camera stage.  Includes k_common.h, tc_deal.h (how the FORM kernels deal pixel items to lanes), tc_device.h and tc_rng.h
// (the noise blobs fused into the stage).
#ifndef K_RASTER_H
#define K_RASTER_H

#include "k_common.h"
#include "tc_deal.h"
#include "tc_device.h"
#include "tc_rng.h"

// ---------------------------------------------------------------------------------------------
// Kernel 2: renderer.py:36-51 -- cv2.polylines of every segment into LDS bit-planes, then the frame is
// written to HBM once with 16-byte stores.  One wavefront per env; small argument block, small LDS.
struct RCam {
  int H, W, wpr, band_rows, n_bands, thickness, format;
  int cap_r;                  // round-cap radius of ThickLine: (thickness*32768 + 32768) >> 16
  unsigned char cap_hw[32];   // half width of the cap per |row offset| (midpoint circle of drawing.cpp)
  unsigned int cap_hw4;       // cap_hw[0..3] packed, for radii <= 3 (thickness <= 6): a scalar, where indexing the table
                              // is a vector load from the kernarg segment per cap row (three dependent ~1 us loads per frame)
};
struct RArgs {
  int N, C;
  int env0;
  RCam cam;
  unsigned char colors[16][3];
  const int* seg_g;  // [N][seg_cap][5]
  const int* seg_n;  // [N]
  int seg_cap;
  unsigned char* obs;
  const unsigned char* mask;  // reset mask (NULL = all envs)
  int off_tab, off_bits;
  unsigned int flags;
  // raster launches over several steps' frames (grid.y = frames rows): row blockIdx.y reads draw list / pose row
  // seg_row0 + blockIdx.y of the library's scratch ring, writes its frame obs_row_stride bytes behind the previous
  // row's, and is step noise_row0 + blockIdx.y of the call (position in the blob stream)
  int seg_row0;
  int noise_row0;
  long long obs_row_stride;
  // NoiseObservationWrapper fused into the raster stage (class masks only): blobs per plane (0 = off), radius bound,
  // the per-radius span table and the blob stream (position of frame row 0 = *noise_step)
  int noise_blobs, noise_max_radius;
  const unsigned char* noise_hw;
  unsigned long long noise_seed;
  const unsigned int* noise_step;
  int seg_lds_off, seg_lds_cap;  // see KArgs
  unsigned int colors_packed[16];  // colors[c] as r | g << 8 | b << 16: read with scalar loads (uniform class index)
};

#ifndef TC_RASTER_WAVES
#define TC_RASTER_WAVES 4
#endif
// LDSONLY (tc_frame_kernel): the stage reads draw-list entries from LDS only, and its common path contains no vector load
// at all.  That matters beyond the loads themselves: vector memory operations retire in issue order, and the compiler
// guards a load that MAY have been issued (the k >= seg_lds_cap branch of seg_get) with s_waitcnt vmcnt(0) at the join --
// which, executed by a wavefront that took the LDS branch, waits for nothing but the wavefront's own earlier STORES: the
// zero planes stored at the head of the stage, the previous band's pixels.  Without the branch the stores drain behind
// the raster work (cfg5: band b's 38 KB land while band b+1 is rasterised).
//   A frame whose list outgrew the LDS head (nseg_in > a.seg_lds_cap: the caller has then put the WHOLE list into the
// global array, head included) is rasterised batch by batch all the same: each batch of RB entries is first copied from
// the global list to the start of the LDS region -- loads and their wait inside a branch the common path never enters.
// Flow control of a banded frame's stores (cfg5: 19 bands of 38 KB): before a band's stores are issued, the stores of the
// band before it must have landed.  With no wait at all a wavefront runs up to 63 store instructions ahead and the chip
// as a whole writes SLOWER (cfg5, stores only: 2.81 ms per dispatch against 2.62); with the wait at the head of the band
// (where the compiler used to put one) the raster work of band b+1 cannot overlap the stores of band b (3.36 ms -> see
// DESIGN.md 6); here the raster work overlaps and at most one band is in flight.
#ifndef TC_BAND_VMCNT
#define TC_BAND_VMCNT 0
#endif
#define TC_BAND_THROTTLE() asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TC_BAND_VMCNT) : "memory")
// Bytes of one env's observation: the one place that spells them out (raster_body's `out`, the fused kernel's step stride,
// tc_env_obs_bytes).  TC_FMT_CLASSES_BITS needs W % 32 == 0 (fill_camera): a row is W / 8 bytes.
__host__ __device__ __forceinline__ size_t tc_obs_bytes_of(int fmt, int C, int H, int W) {
  return fmt == TC_FMT_CLASSES_BITS ? (size_t)C * H * (size_t)(W >> 3) : (size_t)H * W * (fmt == TC_FMT_CLASSES ? C : 3);
}
// the two class-mask formats: identical up to the store phase
#define TC_FMT_IS_CLASSES(fmt) ((fmt) == TC_FMT_CLASSES || (fmt) == TC_FMT_CLASSES_BITS)
// TC_FMT_CLASSES_BITS stores.  A packed row is the row's LDS words byte for byte (both little-endian), and rows follow each
// other without padding on both sides, so rows y0..y1 of a plane are ONE run of nw 32-bit words: lane-consecutive 16-byte
// stores when source and destination are both 16-byte aligned (wave-uniform; a frame is C*H*W/8 bytes and a plane H*W/8,
// neither need be a multiple of 16, and with odd wpr nor need the LDS plane offset), 4-byte stores otherwise.  The odd
// words behind the last whole 16 bytes go out as 4-byte stores: no byte of the run is left unwritten.
__device__ __forceinline__ void packed_zero_words(unsigned char* dst, const int nw, const int tid) {
  if ((((unsigned long long)dst) & 15ull) == 0) {
    const int n4 = nw >> 2;
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (int q = tid; q < n4; q += TC_NT) ((uint4*)dst)[q] = z;
    for (int i = (n4 << 2) + tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = 0u;
  } else {
    for (int i = tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = 0u;
  }
}
// src_word0: index of the run's first word in the bit-plane region, whose start is 16-byte aligned
__device__ __forceinline__ void packed_copy_words(unsigned char* dst, const unsigned int* src, const int src_word0, const int nw,
                                                  const int tid) {
  if ((((unsigned long long)dst) & 15ull) == 0 && (src_word0 & 3) == 0) {
    const int n4 = nw >> 2;
    for (int q = tid; q < n4; q += TC_NT) ((uint4*)dst)[q] = ((const uint4*)src)[q];
    for (int i = (n4 << 2) + tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = src[i];
  } else {
    for (int i = tid; i < nw; i += TC_NT) ((unsigned int*)dst)[i] = src[i];
  }
}
// FORM (the five-wave frame kernel, whose LDS plan is sized for it: plan_frame_lds): the outline tables hold the RB << sh items
// of the handle's outline form -- sh = 2, the four edges of FillConvexPoly's quad, or 1, the two long ones (R_F_LONG_EDGES) --
// and the bit-planes follow at RArgs::off_bits; the pixel loops deal their items by scan (tc_deal.h) and the layers ride in
// lt[..][3] and fm.  Otherwise the tables have their full size at compile-time offsets and the loops search the prefix tables.
// ONE_BAND: the frame is known to be a single band (RCam::n_bands == 1, the caller's promise) -- the stage is then straight-line
// code: no band loop, whose invariants the compiler would otherwise set up -- and spill -- in front of a loop that runs once.
template <bool THICK, int FMT, bool LDSONLY = false, int RB = RB_MAX, bool FORM = false, bool ONE_BAND = false>
__device__ __forceinline__ void raster_body(const RArgs& a0, unsigned char* smem, int env, unsigned char* obs_base,
                                            const int tid, const size_t seg_slot0, const int nseg_in,
                                            const unsigned int used_in, const int frame_row) {
  const RArgs& a = a0;
  const RCam& cam = a.cam;
  auto n_bands_of = [](const RCam& c) { return ONE_BAND ? 1 : c.n_bands; };  // (a constant under ONE_BAND: every test on it folds)
  // (FORM: behind tables sized by the outline form, where the host's plan says: R_OFF_BITS_SH(RB, sh))
  unsigned int* bits = (unsigned int*)(smem + (FORM ? a.off_bits : R_OFF_BITS_OF(RB)));
  const int* segg = a.seg_g + (seg_slot0 + env) * a.seg_cap * 5;
  // draw-list entry k: from LDS when the camera stage of this wavefront left it there (tc_frame_kernel), else global
  const LdsIntPtr seg_lds = (LdsIntPtr)(smem + a.seg_lds_off);
  const int seg_lds_cap = a.seg_lds_cap;
  struct SegV {
    int v[5];
    __device__ __forceinline__ int operator[](int i) const { return v[i]; }
  };
  // LDSONLY: entry k sits at LDS slot k - lds_base (lds_base = 0, or the first entry of the batch just copied in)
  int lds_base = 0;
  const bool refill = LDSONLY && nseg_in > seg_lds_cap;  // (wave-uniform)
  const int rb_step = (refill && seg_lds_cap < RB) ? seg_lds_cap : RB;  // batch size (the LDS region holds >= 8 entries: tc_env_create)
  auto seg_refill = [&](int base, int nb) {  // global entries [base, base + nb) -> LDS slots [0, nb); nb <= rb_step <= seg_lds_cap
    lds_sync();  // the batch before has been read
    for (int i = threadIdx.x; i < 5 * nb; i += TC_NT) seg_lds[i] = segg[5 * base + i];
    lds_base = base;
    lds_sync();
  };
  auto seg_get = [&](int k) {
    SegV r;
    if (LDSONLY) {
#pragma unroll
      for (int i = 0; i < 5; i++) r.v[i] = seg_lds[5 * (k - lds_base) + i];
    } else if (k < seg_lds_cap) {
#pragma unroll
      for (int i = 0; i < 5; i++) r.v[i] = seg_lds[5 * k + i];
    } else {
#pragma unroll
      for (int i = 0; i < 5; i++) r.v[i] = segg[5 * k + i];
    }
    return r;
  };
  auto seg_layer = [&](int k) { return LDSONLY ? seg_lds[5 * (k - lds_base)] : k < seg_lds_cap ? seg_lds[5 * k] : segg[5 * k]; };
  // draw-list length and the layers that have a segment in this frame (wave-uniform): handed over in registers by the
  // camera stage of the same wavefront, or read back when this is a launch of its own (nseg_in < 0)
  int nseg = nseg_in;
  unsigned int used_layers = used_in;
  TSTAMP(8);
  if (!LDSONLY && nseg_in < 0) {
    nseg = a.seg_n[seg_slot0 + env];
    used_layers = 0;
    for (int k = tid; k < nseg; k += TC_NT) used_layers |= 1u << segg[5 * k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) used_layers |= __shfl_xor(used_layers, off);
  }

  int H = cam.H, W = cam.W, wpr = cam.wpr, C = a.C;  // (not const: the banded FORM kernel fetches them again per band)
  constexpr bool CLS = TC_FMT_IS_CLASSES(FMT), BITS = FMT == TC_FMT_CLASSES_BITS;
  unsigned char* out = obs_base + (size_t)env * tc_obs_bytes_of(FMT, C, H, W);
  // Every kernel but FORM ones: lt and lc in front, with room for RB * 4 items, then the tables of fixed size -- all at
  // compile-time offsets.  FORM: the tables of fixed size (116 bytes per segment) in front, then lc and lt for the RB << sh
  // items of the handle's outline form (placed in the batch loop below, where sh is read).
  int* lt0 = (int*)(smem + R_OFF_TAB);    // [RB*4][5] outline-edge parameters
  int* lc0 = lt0 + RB * 4 * 5;            // [RB*4] chunks per outline edge, then exclusive prefix
  int* fl = FORM ? (int*)(smem + R_OFF_TAB) : lc0 + RB * 4;  // [RB] first fill row of the segment in this band
  int* fc = fl + RB;                      // [RB] fill rows, then exclusive prefix
  int* fm = fc + RB;                      // [RB] pieces | walker mask << 8 | quad valid << 16 (FORM: | layer << 17)
  int* fd = fm + RB;                      // [RB][2] ThickLine's (dp.x, dp.y)
  int* fpy = fd + 2 * RB;                 // [RB][4] fill pieces: start row
  int* fpv = fpy + 4 * RB;                // [RB][4] fill pieces: polygon vertices idx0 | idx << 2
  long long* fpx = (long long*)(fpv + 4 * RB);  // [RB][4] x at the start row (16.16)
  long long* fpd = fpx + 4 * RB;          // [RB][4] dx per row
  static_assert(R_OFF_LC_OF(RB) == 13 * RB * 4 + 2 * 4 * RB * 8 && (13 * RB * 4) % 8 == 0, "FORM: lc starts where the fixed tables end");
  // Class masks, one band: the planes of layers that have no segment in this frame are all zeros (unless noise blobs are
  // going to copy into them) and are stored NOW, at the head of the stage -- their 16-byte stores drain while the used
  // planes are rasterised instead of queueing behind each other at the end of the wavefront's life (the store phase
  // is 15 % of the kernel's time for 9 % of its instructions).  A frame with no segment at all (37-57 % of the
  // benchmark's frames once cars have wandered off the road) is done here: no planes to clear, no tables, no expansion.
  unsigned int early_zero = 0;
  if (CLS && n_bands_of(cam) == 1 && (W & 15) == 0 && a.noise_blobs == 0 && !DBG_ON(a.flags, DBG_SKIP_STORE)) {
    const int per_plane = H * (W >> 4);
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < C; c++) {
      if ((used_layers >> c) & 1u) continue;
      if (BITS) {  // the plane's H * wpr words
        packed_zero_words(out + (size_t)c * H * wpr * 4, H * wpr, tid);
        continue;
      }
      uint4* po = (uint4*)(out + (size_t)c * H * W);
      for (int q = tid; q < per_plane; q += TC_NT) po[q] = zero4;
    }
    early_zero = ~used_layers;
    if (nseg == 0) {
      TSTAMP(9);
      TSTAMP(10);
      TSTAMP(11);
      TSTAMP(12);
      TSTAMP(13);
      TSTAMP_REAL(31);
      return;
    }
  }
  for (int band = 0; band < n_bands_of(cam); band++) {
    // (FORM with a band loop -- tc_frame_banded: every band fetches the arguments it needs again; as loop invariants
    // they were fetched in front of the loop and spilled across it)
    if constexpr (FORM && !ONE_BAND) {
      const RArgs& ab = kernarg_again(a0);
      H = ab.cam.H, W = ab.cam.W, wpr = ab.cam.wpr, C = ab.C;
    }
    const int y0 = band * cam.band_rows;
    const int y1 = (y0 + cam.band_rows < H) ? y0 + cam.band_rows : H;
    const int rows = y1 - y0;
    const int nwords = C * cam.band_rows * wpr;
    if (n_bands_of(cam) > 1 && (W & 15) == 0) {
      // A frame taller than one LDS band (cfg5: 480 x 640 in 19 bands): most bands see no lane line at all.  Such a band
      // is all zeros whatever the format (and whatever the noise blobs copy or erase), so it is written as a plain
      // stream of 16-byte zero stores: no bit-planes to clear, nothing to scan, and no wait for the zeros to land before
      // pixel stores that never come.
      bool touched = refill;  // (a list that is not in LDS as a whole is not worth a pass of its own)
      const long long mg = (long long)cam.thickness + 2;  // ThickLine paints within thickness / 2 + 1 rows of the segment
      for (int k0 = 0; k0 < nseg && !touched; k0 += TC_NT) {
        bool t = false;
        if (k0 + tid < nseg) {
          const SegV sg = seg_get(k0 + tid);
          const long long ya = sg[2], yb = sg[4];
          t = (ya < yb ? yb : ya) + mg >= y0 && (ya < yb ? ya : yb) - mg < y1;
        }
        touched = __ballot(t) != 0;
      }
      if (!touched && DBG_ON(a.flags, DBG_SKIP_STORE)) continue;
      if (!touched) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        TC_BAND_THROTTLE();
        if (BITS) {
          for (int c = 0; c < C; c++) packed_zero_words(out + ((size_t)c * H + y0) * wpr * 4, rows * wpr, tid);
        } else if (CLS) {
          const int per_plane = rows * (W >> 4);
          for (int c = 0; c < C; c++) {
            uint4* dst = (uint4*)(out + ((size_t)c * H + y0) * W);
            for (int q = tid; q < per_plane; q += TC_NT) dst[q] = z;
          }
        } else {
          const int n16 = rows * W * 3 / 16;
          uint4* dst = (uint4*)(out + (size_t)y0 * W * 3);
          for (int q = tid; q < n16; q += TC_NT) dst[q] = z;
        }
        continue;
      }
    }
    {  // (the bit-planes' offset is a multiple of 16: whole 16-byte writes, then the odd words)
      const int n4 = nwords >> 2;
      for (int i = tid; i < n4; i += TC_NT) ((uint4*)bits)[i] = make_uint4(0, 0, 0, 0);
      for (int i = (n4 << 2) + tid; i < nwords; i += TC_NT) bits[i] = 0;
    }
    lds_sync();
    TSTAMP(9);
#ifdef TC_TIMING_LDS
    TSTAMP(26);  // back to back with probe 9: what a probe costs
#endif
    Ras r;
    r.W = W;
    r.H = H;
    r.wpr = wpr;
    r.y0 = y0;
    r.y1 = y1;
    const int plane = cam.band_rows * wpr;
    if (DBG_ON(a.flags, DBG_SKIP_RASTER)) {
    } else if (!THICK) {
      for (int base = 0; base < nseg; base += refill ? rb_step : nseg) {
        const int nb = refill ? (nseg - base < rb_step ? nseg - base : rb_step) : nseg;
        if (refill) seg_refill(base, nb);
        for (int k = base + tid; k < base + nb; k += TC_NT) {
          const SegV sg = seg_get(k);
          r.bits = bits + sg[0] * plane;
          r_line_bresenham(r, sg[1], sg[2], sg[3], sg[4]);  // ThickLine with thickness <= 1 is a plain Line()
        }
      }
    } else {
      // ThickLine = FillConvexPoly(quad) [4 Line2 outline edges + scanline fill] + 2 round caps.
      // Segments are taken RB at a time; their pixel work is cut into small uniform items that are dealt
      // to the 64 lanes through prefix sums, so one long line does not serialise the wave.
      for (int base = 0; base < nseg; base += rb_step) {
        // (the loops usually run once: arguments are re-read inside them instead of being hoisted in front and held --
        // or spilled -- across the whole stage)
        const RArgs& a = kernarg_again(a0);
        const RCam& cam = a.cam;
        const int nb = nseg - base < rb_step ? nseg - base : rb_step;
        if (refill) seg_refill(base, nb);
#ifdef TC_TIMING_LDS
        if (cam.n_bands >= 0) TSTAMP(27);  // first value of the re-read argument block has arrived
#endif
        if (n_bands_of(cam) > 1) {
          // Frames taller than one LDS band run this loop once per band (cfg5: 19 bands).  A batch none of whose
          // segments can reach the band's rows is skipped whole -- set-up, prefix sums, pixel loops: most bands of a
          // 480 x 640 frame see no lane line at all and are then a pure zero-store stream.
          bool t = false;
          if (tid < nb) {
            const SegV sg = seg_get(base + tid);
            const long long ya = sg[2], yb = sg[4], mg = (long long)cam.thickness + 2;
            t = (ya < yb ? yb : ya) + mg >= y0 && (ya < yb ? ya : yb) - mg < y1;
          }
          if (__ballot(t) == 0) continue;
        }
#ifdef TC_TIMING_LDS
        if (cam.thickness > 0) TSTAMP(24);  // (depends on a kernel argument re-read above: the scalar loads have returned)
#endif
        if (tid < RB) {  // per segment: ThickLine's dp, fill walker pieces, fill rows of this band
          int nrow = 0, lo = 0, np = 0, wm = 0, dpx = 0, dpy = 0, okq = 0, layer = 0;
#ifdef TC_TIMING_LDS
          TSTAMP(25);
#endif
          if (tid < nb) {
            const SegV sg = seg_get(base + tid);
            layer = sg[0];
            long long qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3;
            TSTAMP(20);
            // Frames taller than one LDS band are rasterised band by band, and every band runs this set-up again.  A
            // segment whose rows cannot reach the band is dropped before any of it: ThickLine paints within
            // thickness / 2 + 1 rows of the segment (quad corners p +- dp with |dp| <= thickness / 2 + 1 px, cap radius
            // (thickness + 1) / 2), and `thickness + 2` rows are allowed here.  On cfg5 (12 bands) a segment survives
            // this in 1-3 bands instead of 12.
            bool touch = true;
            if (n_bands_of(cam) > 1) {
              const long long ya = sg[2], yb = sg[4], mg = (long long)cam.thickness + 2;
              const long long ymin = (ya < yb ? ya : yb) - mg, ymax = (ya < yb ? yb : ya) + mg;
              touch = ymax >= y0 && ymin < y1;
            }
            if (touch && !DBG_ON(a.flags, DBG_SKIP_QUAD) && r_quad_dp(sg[1], sg[2], sg[3], sg[4], cam.thickness, dpx, dpy)) {
              TSTAMP(21);
              okq = 1;
              r_quad_vertices(sg[1], sg[2], sg[3], sg[4], dpx, dpy, qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3);
              int hi = -1;
              if (!DBG_ON(a.flags, DBG_SKIP_EVENTS))
              np = r_fill_events(W, H, qx0, qx1, qx2, qx3, qy0, qy1, qy2, qy3, fpy + 4 * tid, fpv + 4 * tid, wm, lo,
                                 hi);
              TSTAMP(22);
              if (lo < y0) lo = y0;
              if (hi > y1 - 1) hi = y1 - 1;
              if (np > 0 && hi >= lo) nrow = hi - lo + 1;
            }
          }
          fl[tid] = lo;
          fc[tid] = nrow;
          // (FORM: the segment's layer rides in bits 17..21, so a fill row does not read the draw list for it)
          fm[tid] = np | (wm << 8) | (okq << 16) | (FORM ? layer << 17 : 0);
          fd[2 * tid] = dpx;
          fd[2 * tid + 1] = dpy;
        }
        lds_sync();
        TSTAMP(10);
        MARK("outline setup");
        // Outline edges: clip + DDA parameters.  Four per segment (FillConvexPoly's), or -- R_F_LONG_EDGES: thickness 2, see
        // tc_line.h -- only the two long ones v3->v0 and v1->v2, whose items then sit two per segment at the front of the
        // tables: a batch of up to 32 segments is ONE pass of this loop instead of two.  Entries past the items keep a chunk
        // count of 0 either way.  The fill pieces ride along: one per edge lane in the four-edge form, pieces i and i + 2
        // on the segment's lane i = 0, 1 in the two-edge form (the second evaluation is skipped by the whole wavefront when
        // no segment has more than two pieces).
        // (everything the two forms differ in hangs on one scalar: items per segment = 1 << sh)
        const int sh = (a.flags & R_F_LONG_EDGES) ? 1 : 2;
        const int n_items = FORM ? RB << sh : RB * 4;  // entries of lc and lt that exist
        int* lc = FORM ? (int*)(fpd + 4 * RB) : lc0;   // [items] chunks per outline edge, then exclusive prefix
        int* lt = FORM ? lc + n_items : lt0;           // [items][5] outline-edge parameters
        for (int t = tid; t < n_items; t += TC_NT) {
          int nchunk = 0;
          const int j = t >> sh;
          if (t < (nb << sh) && ((fm[j] >> 16) & 1)) {
            const int s0 = t & ((1 << sh) - 1), e = s0 << (2 - sh);  // item of the segment; its edge: 0 2, or 0 1 2 3
            const SegV sg = seg_get(base + j);
            // the quad travels as (pixel end points, dp): the fill pieces and the outline edge each form the vertices
            // they need from the int32 parts (r_fill_slope, r_outline_edge)
            const int dpx = fd[2 * j], dpy = fd[2 * j + 1];
            const int np = fm[j] & 0xff;
            // fill pieces of this lane (x at the start row and slope): piece s0, and s0 + 2 in the two-edge form -- one
            // instance of the code, a loop the wavefront leaves together
#pragma nounroll
            for (int h = 0; h < (8 >> sh) && !DBG_ON(a.flags, DBG_SKIP_SLOPE); h += 2) {
              const bool want = s0 + h < np;
              if (h != 0 && __ballot(want) == 0) break;
              if (want) {
                const int s = 4 * j + s0 + h;
                long long xs, dxs;
                r_fill_slope(sg[1], sg[2], sg[3], sg[4], dpx, dpy, fpy[s], fpv[s], xs, dxs);
                fpx[s] = xs;
                fpd[s] = dxs;
              }
            }
            LineP L;
            L.ecount = -1;
            if (!DBG_ON(a.flags, DBG_SKIP_LINESETUP)) L = r_outline_edge(W, H, sg[1], sg[2], sg[3], sg[4], dpx, dpy, e);
            if (L.ecount >= 0) {
              r.bits = bits + sg[0] * plane;
              r_put(r, L.ex, L.ey);
              int* o = lt + 5 * t;
              o[0] = L.a;
              o[1] = L.b;
              o[2] = L.step;
              if constexpr (FORM) {  // the layer in bits 16..20 (ecount has 16 bits); the stride stays 5 words
                o[3] = L.ecount | (sg[0] << 16) | (L.xmajor << 30);
              } else {
                o[3] = L.ecount | (L.xmajor << 30);
                o[4] = sg[0];
              }
              nchunk = (L.ecount + LCH) / LCH;
            }
          }
          lc[t] = nchunk;
        }
        lds_sync();
        MARK("prefix sums");
        int tot_l, tot_f;
        int dl_p0 = 0, dl_n0 = 0, dl_p1 = 0, dl_n1 = 0, dl_t0 = 0, df_p = 0, df_n = 0;  // FORM: (prefix, count) of this lane's entries
        {  // exclusive prefix sums (RB*4 = 2 entries per lane, or 1 when RB = 16; RB entries on the low lanes)
          static_assert(RB * 4 == 2 * TC_NT || RB * 4 == TC_NT, "outline-edge chunk counts: one or two per lane");
          constexpr bool TWO = RB * 4 == 2 * TC_NT;
          // (FORM, two-edge form: half the items, one entry per lane -- or none: wave-uniform)
          const bool two = TWO && !(FORM && sh == 1);
          const bool mine = !FORM || tid < n_items;  // (without FORM every lane has its entry: RB * 4 >= TC_NT)
          int v0 = two ? lc[2 * tid] : (mine ? lc[tid] : 0), v1 = two ? lc[2 * tid + 1] : 0;
          int inc = wave_incl_scan(v0 + v1, tid);
          tot_l = __builtin_amdgcn_readlane(inc, TC_NT - 1);
          int f = tid < RB ? fc[tid] : 0;
          int finc = wave_incl_scan(f, tid);
          tot_f = __builtin_amdgcn_readlane(finc, TC_NT - 1);
          if constexpr (FORM) {
            // the pixel loops deal by scan (tc_deal.h): prefix and count stay in the registers the scan left them in, and
            // neither table is read again -- lc keeps the chunk counts and becomes the dealing's scratch, fc keeps the rows
            dl_t0 = two ? 2 * tid : tid;
            dl_p0 = inc - v0 - v1, dl_n0 = v0, dl_p1 = inc - v1, dl_n1 = v1;
            df_p = finc - f, df_n = f;
          } else {
            if (two) {
              lc[2 * tid] = inc - v0 - v1;  // each lane rewrites only the entries it read
              lc[2 * tid + 1] = inc - v1;
            } else if (mine) {
              lc[tid] = inc - v0;
            }
            if (tid < RB) fc[tid] = finc - f;
          }
        }
        lds_sync();
        TSTAMP(11);
        if constexpr (FORM) {
          static_assert(!FORM || (RB == 32 && RB * 4 <= TC_DEAL_IDS && TC_NT == TC_DEAL_LANES), "lc holds >= 64 words and a marker names every entry");
          // One pass: zero the 64 slots (the head of lc, dead: see above), the entries that start in the window drop their
          // markers, every lane picks its slot up and the max-scan spreads each marker over the items behind it.
          auto deal = [&](const int c0, const int carry, const int p0, const int n0, const int t0, const int p1, const int n1) {
            lc[tid] = 0;
            if (tc_deal_starts(p0, n0, c0)) lc[p0 - c0] = tc_deal_word(p0, t0);
            if (tc_deal_starts(p1, n1, c0)) lc[p1 - c0] = tc_deal_word(p1, t0 + 1);
            lds_sync();
            const int w = wave_incl_max(lc[tid]);
            return w > carry ? w : carry;
          };
          int carry = 0;
          for (int c0 = 0; c0 < tot_l && !DBG_ON(a.flags, DBG_SKIP_R2); c0 += TC_NT) {  // outline pixels, LCH steps per chunk
            const int w = deal(c0, carry, dl_p0, dl_n0, dl_t0, dl_p1, dl_n1);
            carry = __builtin_amdgcn_readlane(w, TC_NT - 1);
            const int c = c0 + tid;
            if (c < tot_l) {
              const int* o = lt + 5 * tc_deal_owner(w);
              const int o3 = o[3];
              const int ecount = o3 & 0xffff, xmajor = (o3 >> 30) & 1;
              const int k0 = tc_deal_offset(w, c) * LCH;
              const int k1 = k0 + LCH - 1 < ecount ? k0 + LCH - 1 : ecount;
              r.bits = bits + ((o3 >> 16) & 31) * plane;  // (the layer rides in the word: see the set-up)
              r_line2_pixels(r, o[0], o[1], o[2], xmajor, k0, k1);
            }
          }
          MARK("fill rows");
          carry = 0;
          for (int c0 = 0; c0 < tot_f && !DBG_ON(a.flags, DBG_SKIP_R3); c0 += TC_NT) {  // scanline fill, one row per item
            const int w = deal(c0, carry, df_p, df_n, tid, 0, 0);
            carry = __builtin_amdgcn_readlane(w, TC_NT - 1);
            const int c = c0 + tid;
            if (c < tot_f) {
              const int lo = tc_deal_owner(w);
              const int row = fl[lo] + tc_deal_offset(w, c);
              const int mm = fm[lo];
              r.bits = bits + ((mm >> 17) & 31) * plane;  // (likewise)
              r_fill_row(r, row, mm & 0xff, (mm >> 8) & 0xff, fpy + 4 * lo, fpx + 4 * lo, fpd + 4 * lo);
            }
          }
        } else {  // every other kernel: the binary search through the prefix tables (tc_deal_search's form)
          for (int c = tid; c < tot_l && !DBG_ON(a.flags, DBG_SKIP_R2); c += TC_NT) {  // outline pixels, LCH steps per chunk
            int lo = 0, hi = n_items;
            while (hi - lo > 1) {
              int mid = (lo + hi) >> 1;
              if (lc[mid] <= c) lo = mid; else hi = mid;
            }
            const int* o = lt + 5 * lo;
            const int ecount = o[3] & 0xffff, xmajor = (o[3] >> 30) & 1;
            const int k0 = (c - lc[lo]) * LCH;
            const int k1 = k0 + LCH - 1 < ecount ? k0 + LCH - 1 : ecount;
            r.bits = bits + o[4] * plane;
            r_line2_pixels(r, o[0], o[1], o[2], xmajor, k0, k1);
          }
          MARK("fill rows");
          for (int c = tid; c < tot_f && !DBG_ON(a.flags, DBG_SKIP_R3); c += TC_NT) {  // scanline fill, one row per item
            int lo = 0, hi = RB;
            while (hi - lo > 1) {
              int mid = (lo + hi) >> 1;
              if (fc[mid] <= c) lo = mid; else hi = mid;
            }
            const int row = fl[lo] + (c - fc[lo]);
            const int mm = fm[lo];
            r.bits = bits + seg_layer(base + lo) * plane;
            r_fill_row(r, row, mm & 0xff, (mm >> 8) & 0xff, fpy + 4 * lo, fpx + 4 * lo, fpd + 4 * lo);
          }
        }
        MARK("caps");
        for (int t = tid; t < nb * 2 && !DBG_ON(a.flags, DBG_SKIP_R4); t += TC_NT) {  // round caps (flags = 3: both ends)
          const int k = base + (t >> 1);
          const SegV sg = seg_get(k);
          r.bits = bits + sg[0] * plane;
          const int cx = (t & 1) ? sg[3] : sg[1], cy = (t & 1) ? sg[4] : sg[2];
          if (n_bands_of(cam) > 1 && ((long long)cy + cam.cap_r < y0 || (long long)cy - cam.cap_r >= y1)) continue;  // cap outside the band
          if (cam.cap_r < 32)
            r_cap(r, cx, cy, cam.cap_r, cam.cap_hw, cam.cap_hw4);
          else
            r_circle_fill(r, cx, cy, cam.cap_r);
        }
        lds_sync();
      }
    }
    lds_sync();
    if (CLS && a.noise_blobs > 0) {
      // NoiseObservationWrapper (wrapper/observation.py:15-27) on the bit-planes, before they are expanded: the frame
      // never makes the extra round trip through HBM a pass of its own costs (71 us per step on cfg3 in round 1).
      // Every operation of the reference is per pixel -- plane c |= plane src & circle, or plane c &= ~circle, blob
      // after blob, plane after plane -- so one lane owns one (row, 32-pixel word) of ALL planes and replays the whole
      // blob sequence on it: no lane ever reads a word another lane writes, no barrier between blobs.  Plane c's word
      // lives in a register while its n_blobs are applied; planes < c are read back noised, planes > c as rasterised,
      // exactly the sequential order.  A filled cv2.circle with its centre inside the image is, row by row, the span
      // centre +- hw[radius][|row - cy|] clipped to the image (see tc_noise_kernel).
      const int nbl = a.noise_blobs, nb = C * nbl, mr = a.noise_max_radius;
      int* bp = (int*)(smem + R_OFF_TAB);                 // [nb][2] (x | y << 16), (r | mode << 12 | src << 16): the
      unsigned char* bh = (unsigned char*)(bp + 2 * nb);  // raster tables are dead here;  [nb][rows] half widths
      const bool staged = nb * 8 + nb * rows <= (FORM ? a.off_bits : R_OFF_BITS_OF(RB)) - R_OFF_TAB;
      const unsigned int nstep = *a.noise_step + (unsigned int)frame_row;
      for (int k = tid; k < nb; k += TC_NT) {
        const tc_blob bl = tc_noise_blob(a.noise_seed, (uint32_t)env, nstep, (uint32_t)k, W, H, mr, C);
        bp[2 * k] = bl.x | (bl.y << 16);
        bp[2 * k + 1] = bl.r | (bl.mode << 12) | (bl.src << 16);
      }
      lds_sync();
      if (staged) {  // half width of every (blob, row of this band): one table byte each, fetched with the loads in flight
        for (int row = tid; row < rows; row += TC_NT) {
#pragma unroll 5
          for (int k = 0; k < nb; k++) {
            const int by = bp[2 * k] >> 16, rr = bp[2 * k + 1] & 0xfff;
            int t = y0 + row - by;
            t = t < 0 ? -t : t;
            bh[k * rows + row] = t <= rr ? a.noise_hw[rr * mr + t] : (unsigned char)0;
          }
        }
        lds_sync();
      }
      const int items = rows * wpr;
      for (int it = tid; it < items; it += TC_NT) {
        const int row = it / wpr, w = it - row * wpr;
        const int yy = y0 + row, x_lo = w << 5;
        for (int c = 0; c < C; c++) {
          unsigned int cur = bits[(c * cam.band_rows + row) * wpr + w];
          for (int j = 0; j < nbl; j++) {
            const int k = c * nbl + j;
            const int p0 = bp[2 * k], p1 = bp[2 * k + 1];
            const int bx = p0 & 0xffff, by = p0 >> 16, rr = p1 & 0xfff, src = p1 >> 16;
            int t = yy - by;
            t = t < 0 ? -t : t;
            if (t <= rr) {
              const int hwv = staged ? (int)bh[k * rows + row] : (int)a.noise_hw[rr * mr + t];
              int xl = bx - hwv, xr = bx + hwv;
              xl = xl < 0 ? 0 : xl;
              xr = xr > W - 1 ? W - 1 : xr;
              const int b0 = xl > x_lo ? xl - x_lo : 0, b1 = xr < x_lo + 31 ? xr - x_lo : 31;
              if (b1 >= b0) {
                const unsigned int mask = (0xffffffffu >> (31 - b1)) & (0xffffffffu << b0);
                if ((p1 >> 12) & 1) {  // observation.py:22-24
                  const unsigned int sw = src == c ? cur : bits[(src * cam.band_rows + row) * wpr + w];
                  cur |= sw & mask;
                } else {
                  cur &= ~mask;  // observation.py:26
                }
              }
            }
          }
          bits[(c * cam.band_rows + row) * wpr + w] = cur;
        }
      }
      lds_sync();
      used_layers = C >= 32 ? 0xffffffffu : ((1u << C) - 1u);  // a copy may have filled a plane that had no segment
    }
    TSTAMP(12);
    const RArgs& a = kernarg_again(a0);
    const RCam& cam = a.cam;
    if (n_bands_of(cam) > 1) TC_BAND_THROTTLE();
    if (DBG_ON(a.flags, DBG_SKIP_STORE)) {
    } else if (BITS) {
      // packed class masks: the store phase is a copy of the band's rows, plane by plane (planes of layers without a
      // segment: zeros, unless they went out at the head of the stage)
      for (int c = 0; c < C; c++) {
        if ((early_zero >> c) & 1u) continue;
        unsigned char* po = out + ((size_t)c * H + y0) * wpr * 4;
        const int w0 = c * cam.band_rows * wpr;
        if ((used_layers >> c) & 1u)
          packed_copy_words(po, bits + w0, w0, rows * wpr, tid);
        else
          packed_zero_words(po, rows * wpr, tid);
      }
    } else if (CLS) {
      if ((W & 15) == 0) {
        // 16 pixels -> one 16-byte store per lane, consecutive lanes on consecutive addresses
        // (two 16-byte stores per lane at a 32-byte lane stride were tried: 2x slower, half-line writes)
        const int g = W >> 4;  // 16-pixel groups per row
        const int per_plane = rows * g;
        const bool dense = (W & 31) == 0;  // then 16-bit half h of plane word q>>1 is group q
        const uint4 zero4 = make_uint4(0, 0, 0, 0);
        for (int c = 0; c < C; c++) {
          const unsigned int* pl = bits + c * cam.band_rows * wpr;
          unsigned char* po = out + ((size_t)c * H + y0) * W;
          if ((early_zero >> c) & 1u) continue;  // stored as zeros at the head of the stage
          if (!((used_layers >> c) & 1u)) {  // no segment of this layer in the frame: the plane is all zeros
            for (int q = tid; q < per_plane; q += TC_NT) *(uint4*)(po + (size_t)q * 16) = zero4;
            continue;
          }
          if (dense) {
            // four groups per lane and round: the four plane words are fetched together, so the wavefront waits for the
            // LDS once per round instead of once per store (the phase is a chain of read -> expand -> store; measured
            // with the stores switched off it is 15 % of the kernel's time for 9 % of its instructions)
            for (int q0 = tid; q0 < per_plane; q0 += 4 * TC_NT) {
              unsigned int w4[4];
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int q = q0 + j * TC_NT;
                w4[j] = q < per_plane ? pl[q >> 1] : 0u;
              }
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int q = q0 + j * TC_NT;
                const unsigned int b16 = (w4[j] >> ((q & 1) << 4)) & 0xffffu;
                uint4 o = zero4;
                if (__ballot(b16 != 0)) {  // wave-uniform: skip the bit spreading when all 64 groups are empty
                  o.x = spread4(b16 & 15u);
                  o.y = spread4((b16 >> 4) & 15u);
                  o.z = spread4((b16 >> 8) & 15u);
                  o.w = spread4(b16 >> 12);
                }
                if (q < per_plane) *(uint4*)(po + (size_t)q * 16) = o;  // rows of a plane are contiguous: group q sits at byte 16 q
              }
            }
            continue;
          }
          for (int q = tid; q < per_plane; q += TC_NT) {
            const int yy = q / g;
            const int xx = (q - yy * g) << 4;
            const unsigned int b16 = (pl[yy * wpr + (xx >> 5)] >> (xx & 31)) & 0xffffu;
            uint4 o = zero4;
            if (__ballot(b16 != 0)) {
              o.x = spread4(b16 & 15u);
              o.y = spread4((b16 >> 4) & 15u);
              o.z = spread4((b16 >> 8) & 15u);
              o.w = spread4(b16 >> 12);
            }
            *(uint4*)(po + (size_t)q * 16) = o;
          }
        }
      } else {
        const int per_plane = rows * W;
        const int total = C * per_plane;
        for (int q = tid; q < total; q += TC_NT) {
          int c = q / per_plane, p = q - c * per_plane;
          int yy = p / W, xx = p - yy * W;
          unsigned int word = bits[(c * cam.band_rows + yy) * wpr + (xx >> 5)];
          out[((size_t)c * H + y0 + yy) * W + xx] = ((word >> (xx & 31)) & 1u) ? 255 : 0;
        }
      }
    } else {
      // rgb: painter's order (renderer.py:41-43): the highest layer covering a pixel wins
      if ((W & 15) == 0) {
        // this band's rows as zeros first, then only the pixels that have a bit set in some plane.  The byte stores
        // follow the zero stores of the same wavefront to the same addresses in program order, and the memory system
        // keeps stores of one wavefront to one address in that order (the compiler relies on the same guarantee: it
        // never waits between two stores that may alias) -- no wait for the zeros to land: that wait was a full store
        // round trip per band, the largest single item of a touched band (cfg5 ablation, profiles/r03).
        // (Zeroing the whole frame before the first band was measured: 16 % slower)
        {
          const int n16 = rows * W * 3 / 16;
          uint4* dst = (uint4*)(out + (size_t)y0 * W * 3);
          const uint4 z = make_uint4(0, 0, 0, 0);
          for (int q = tid; q < n16; q += TC_NT) dst[q] = z;
        }
        // Class by class, highest first; a class paints the pixels it covers that no higher class covers.  The colour of a
        // class is then ONE value for the whole wavefront, fetched with a scalar load.  (Looked up per pixel --
        // colors[top][k] with `top` differing between lanes -- it was a vector load from the kernarg segment, and vector
        // memory operations retire in order: the wavefront sat out the round trip of this band's zero stores at every
        // such load, which is why raster and store time of cfg5 added up instead of overlapping -- ablation)
        const int nw = rows * wpr;
        const int pstride = cam.band_rows * wpr;
        const __attribute__((address_space(4))) unsigned int* pk =
            (const __attribute__((address_space(4))) unsigned int*)(unsigned long long)&a.colors_packed[0];
        for (int c = C - 1; c >= 0; c--) {
          const unsigned int col = pk[c];
          const unsigned char c0 = (unsigned char)col, c1 = (unsigned char)(col >> 8), c2 = (unsigned char)(col >> 16);
          for (int q = tid; q < nw; q += TC_NT) {
            unsigned int mine = bits[c * pstride + q];
            if (mine == 0) continue;
            for (int h = c + 1; h < C; h++) mine &= ~bits[h * pstride + q];
            const int yy = q / wpr, xw = (q - yy * wpr) << 5;
            unsigned char* row = out + ((size_t)(y0 + yy) * W + xw) * 3;
            while (mine) {
              const int bpos = __ffs(mine) - 1;
              mine &= mine - 1;
              unsigned char* o = row + bpos * 3;
              o[0] = c0;
              o[1] = c1;
              o[2] = c2;
            }
          }
        }
      } else if ((W & 3) == 0) {
        const int total = rows * W / 4;
        for (int g = tid; g < total; g += TC_NT) {
          int pix = g * 4;
          int yy = pix / W, xx = pix - yy * W;
          unsigned int top4 = 0;  // per pixel: 1 + index of the highest layer set, 4 pixels in 4 bytes
          for (int c = 0; c < C; c++) {
            unsigned int word = bits[(c * cam.band_rows + yy) * wpr + (xx >> 5)];
            unsigned int m4 = spread4((word >> (xx & 31)) & 15u);  // 0xFF where the layer covers the pixel
            top4 = (top4 & ~m4) | (m4 & (0x01010101u * (unsigned)(c + 1)));
          }
          unsigned char px[12];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            int top = (int)((top4 >> (8 * k)) & 255u) - 1;
            px[3 * k] = top >= 0 ? a.colors[top][0] : 0;
            px[3 * k + 1] = top >= 0 ? a.colors[top][1] : 0;
            px[3 * k + 2] = top >= 0 ? a.colors[top][2] : 0;
          }
          unsigned int* o = (unsigned int*)(out + ((size_t)(y0 + yy) * W + xx) * 3);
          o[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((unsigned)px[3] << 24);
          o[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((unsigned)px[7] << 24);
          o[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((unsigned)px[11] << 24);
        }
      } else {
        const int total = rows * W;
        for (int p = tid; p < total; p += TC_NT) {
          int yy = p / W, xx = p - yy * W;
          int top = -1;
          for (int c = 0; c < C; c++) {
            unsigned int word = bits[(c * cam.band_rows + yy) * wpr + (xx >> 5)];
            if ((word >> (xx & 31)) & 1u) top = c;
          }
          unsigned char* o = out + ((size_t)(y0 + yy) * W + xx) * 3;
          o[0] = top >= 0 ? a.colors[top][0] : 0;
          o[1] = top >= 0 ? a.colors[top][1] : 0;
          o[2] = top >= 0 ? a.colors[top][2] : 0;
        }
      }
    }
    lds_sync();
  }
  TSTAMP(13);
  TSTAMP_REAL(31);
}

template <bool THICK, int FMT>
__global__ __launch_bounds__(TC_NT, TC_RASTER_WAVES) void tc_raster_kernel(RArgs a_unused) {
  extern __shared__ __align__(16) unsigned char smem[];
  // raster_body re-reads its arguments through kernarg_again(): it must be handed the block in the kernarg segment
  // itself, not a by-value copy the compiler is free to keep in registers or scratch
  const RArgs& a = *(const RArgs*)(const __attribute__((address_space(4))) RArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const int env = a.env0 + blockIdx.x;
  if (env >= a.N) return;
  if (a.mask && !a.mask[env]) return;
  // one workgroup per (frame row, env): with more frames than resident workgroups the dispatcher hands the next frame
  // to whichever slot frees up first, so light and heavy frames balance out across the chip
  const size_t slot0 = (size_t)(a.seg_row0 + blockIdx.y) * a.N;
  raster_body<THICK, FMT>(a, smem, env, a.obs + (size_t)blockIdx.y * a.obs_row_stride, threadIdx.x, slot0, -1, 0u, a.noise_row0 + (int)blockIdx.y);
}

#endif  // K_RASTER_H
