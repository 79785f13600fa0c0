// Dealing the raster stage's pixel items to the 64 lanes (raster_body, k_raster.h).
//
// A batch's pixel work is a table of entries (outline edges, or segments' fill rows), entry t holding cnt[t] items; with the
// exclusive prefix pre[t] the items of the batch are numbered 0 .. total-1 and item c belongs to
//
//     the last entry t with pre[t] <= c            (among entries of equal prefix that is the one that HAS items)
//
// at offset c - pre[t].  A pass hands items c0 .. c0+63 to lanes 0 .. 63.  Two forms of finding the owner:
//
//   tc_deal_search   the binary search through the table of prefixes, once per lane and pass.  It is the specification, and
//                    what every kernel but the five-wave frame kernels runs.
//   the scan form    no table is read.  Every entry with items whose first item falls into the pass's window
//                    (tc_deal_starts) drops ONE marker word, tc_deal_word(pre, t) = pre << 7 | t, into slot pre - c0 of a
//                    64-word scratch that was zeroed; lane L picks up slot L, and an inclusive MAX-scan over the lanes
//                    (tc_deal_scan64: the order of combination of the kernels' DPP scan) followed by a max with the carry
//                    -- the word lane 63 ended the previous pass with, 0 in front of the first -- leaves every lane with the
//                    marker of the last entry that starts at or before its item: owner tc_deal_owner(w), offset
//                    tc_deal_offset(w, c).  Markers of one batch are ordered as their prefixes are (entries with items have
//                    distinct prefixes, and the prefix sits on top of the word), so the maximum IS the latest start.  The
//                    all-zero word is both "no marker" and the marker of entry 0 at prefix 0, which is what an item in
//                    front of every other marker belongs to.  A window into which no entry starts is carried across.
//
// Limits: entries < 128 (TC_DEAL_IDS), total items < 2^24 (the word stays a non-negative int).
// tests/test_deal_cpu.py runs the scan form, 64 emulated lanes, against the search.  Plain C / HIP like tc_fill.h and
// tc_pack.h: the tests build this header with the host compiler.
#ifndef TC_DEAL_H
#define TC_DEAL_H
#include "tc_trig.h" /* TC_HD */

#define TC_DEAL_BITS 7
#define TC_DEAL_IDS (1 << TC_DEAL_BITS)  // entries a marker can name
#define TC_DEAL_LANES 64

TC_HD int tc_deal_word(int pre, int t) { return (pre << TC_DEAL_BITS) | t; }
TC_HD int tc_deal_owner(int w) { return w & (TC_DEAL_IDS - 1); }
TC_HD int tc_deal_offset(int w, int c) { return c - (int)((unsigned)w >> TC_DEAL_BITS); }
// does entry (pre, cnt) drop its marker in the pass of items c0 .. c0+63?  (its slot is then pre - c0)
TC_HD int tc_deal_starts(int pre, int cnt, int c0) { return cnt != 0 && (unsigned)(pre - c0) < (unsigned)TC_DEAL_LANES; }

// the specification: owner of item c by binary search through the n exclusive prefixes (n >= 1, pre[0] == 0 <= c)
TC_HD int tc_deal_search(const int* pre, int n, int c) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

// Inclusive max-scan of 64 non-negative words in the combination order of the kernels' DPP scan (wave_incl_scan /
// wave_incl_max, k_common.h): shifts by 1, 2, 4, 8 inside each row of 16 with zeros shifted in, then lane 15 of a row into
// the whole next row (rows 1 and 3), then lane 31 into rows 2 and 3.  Host emulation for the tests; the kernels run the
// DPP form.
TC_HD void tc_deal_scan64(int* w) {
  int s[TC_DEAL_LANES];
  for (int d = 1; d < 16; d <<= 1) {
    for (int l = 0; l < TC_DEAL_LANES; l++) s[l] = (l & 15) >= d ? w[l - d] : 0;
    for (int l = 0; l < TC_DEAL_LANES; l++) w[l] = w[l] > s[l] ? w[l] : s[l];
  }
  for (int l = 0; l < TC_DEAL_LANES; l++) s[l] = ((l >> 4) & 1) ? w[(l & ~15) - 1] : 0;
  for (int l = 0; l < TC_DEAL_LANES; l++) w[l] = w[l] > s[l] ? w[l] : s[l];
  for (int l = 0; l < TC_DEAL_LANES; l++) s[l] = l >= 32 ? w[31] : 0;
  for (int l = 0; l < TC_DEAL_LANES; l++) w[l] = w[l] > s[l] ? w[l] : s[l];
}

// One pass of the scan form over a table of n entries (host emulation of the 64 lanes): words[L] = the marker lane L ends
// with for item c0 + L; returns the carry into the next pass.  `scratch` are the 64 slots.
TC_HD int tc_deal_pass(const int* pre, const int* cnt, int n, int c0, int carry, int* scratch, int* words) {
  for (int l = 0; l < TC_DEAL_LANES; l++) scratch[l] = 0;
  for (int t = 0; t < n; t++)
    if (tc_deal_starts(pre[t], cnt[t], c0)) scratch[pre[t] - c0] = tc_deal_word(pre[t], t);
  for (int l = 0; l < TC_DEAL_LANES; l++) words[l] = scratch[l];
  tc_deal_scan64(words);
  for (int l = 0; l < TC_DEAL_LANES; l++) words[l] = words[l] > carry ? words[l] : carry;
  return words[TC_DEAL_LANES - 1];
}

#endif  // TC_DEAL_H
