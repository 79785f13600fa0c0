// The camera stage's clip passes (camera.py:70-86) as pairs: when passes 1+2 (plane z = -1e-7, set idx_front) or passes
// 3+4 (plane z = -max_range, set idx_in_range) may run as ONE pass with the reference's result, bit for bit.
//
// A pass freezes its edge list from the membership set as it stands when the pass starts, then moves, in list order,
// the end outside the set onto the plane along the edge and adds it to the set.  The first pass of a pair takes the
// edges with e[0] outside and e[1] inside (target e[0]), the second the edges with e[0] inside and e[1] outside
// (target e[1]).  With S the set before the pair, L1 / L2 the two lists computed from S, T1 / T2 their targets:
//
//   (a) no node is a target of both passes;
//   (b) no node pass 2 reads (as the end that stays, or as a target) is moved or added by pass 1;
//   (c) pass 1 adds no edge to pass 2's list by putting a node into the set.
//
// The ends that stay are members of S in both lists and targets never are, so a move of either list reads only its own
// target and a node no pass of the pair writes: (b) reduces to (a).  (c) fails exactly for an edge (a, b) with a in T1
// and b neither in S nor in T1 -- after pass 1 it reads "e[0] inside, e[1] outside".  Under (a) and (c) the list pass 2
// freezes equals L2, and when in addition every target of L1 ++ L2 is distinct the moves are independent of each
// other: any order, and so one pass over the concatenated list, leaves what the two passes leave.  A target shared
// inside ONE list makes the order of that list's moves matter; the pair is then refused as well and the two passes run
// in their literal form (which replays such chains in edge order).
//
// The kernels evaluate this with ballots over the edge slots of a wavefront (cam_group_regs, k_camera.h); the
// scalar form below is the definition, and what tests/test_clip_merge_cpu.py proves against the oracle.
// Plain C / HIP like tc_trig.h and tc_rng.h: the tests build this header with the host compiler.
#ifndef TC_CLIP_H
#define TC_CLIP_H
#include "tc_trig.h" /* TC_HD */

// node flag byte of the camera stage: 1 idx_front, 2 idx_in_range, 4 visible, 16 projection candidate, and one bit
// per pair for "target of the pair's first list" (left set: every reader masks)
#define TC_CLIP_MARK0 32
#define TC_CLIP_MARK1 64

// which list of the pair on membership bit `bit` an edge with end flags fa, fb belongs to:
// 1 = first (e[0] outside, e[1] inside), 2 = second (e[0] inside, e[1] outside), 0 = neither
TC_HD int tc_clip_sel(int fa, int fb, int bit) {
  const int ia = (fa & bit) != 0, ib = (fb & bit) != 0;
  return (!ia && ib) ? 1 : ((ia && !ib) ? 2 : 0);
}

// (c) for one edge, once the targets of the first list carry `mark`: 1 = this edge would join the second list
TC_HD int tc_clip_joins_second(int fa, int fb, int bit, int mark) {
  return !(fa & bit) && !(fb & bit) && (fa & mark) && !(fb & mark);
}

#define TC_CLIP_FIRST 1   // the pair's first list is not empty
#define TC_CLIP_SECOND 2  // the pair's second list (computed from the flags before the pair) is not empty
#define TC_CLIP_MERGE 4   // both are, and the pair may run as one pass

// The pair test on a whole edge list (ne edges, node ids in edges[2 * e], edges[2 * e + 1]; flg: one byte per node).
// list: room for 2 * ne ints; receives (target, other end) of L1 ++ L2, *n1 / *n2 their lengths.  Sets `mark` on T1.
TC_HD int tc_clip_pair_test(const int* edges, int ne, unsigned char* flg, int bit, int mark, int* list, int* n1, int* n2) {
  int n = 0;
  for (int which = 1; which <= 2; which++) {
    for (int e = 0; e < ne; e++) {
      const int a = edges[2 * e], b = edges[2 * e + 1];
      if (tc_clip_sel(flg[a], flg[b], bit) != which) continue;
      list[2 * n] = which == 1 ? a : b;
      list[2 * n + 1] = which == 1 ? b : a;
      n++;
    }
    if (which == 1) *n1 = n;
  }
  *n2 = n - *n1;
  int r = (*n1 ? TC_CLIP_FIRST : 0) | (*n2 ? TC_CLIP_SECOND : 0);
  if (r != (TC_CLIP_FIRST | TC_CLIP_SECOND)) return r;
  for (int i = 0; i < *n1; i++) flg[list[2 * i]] |= (unsigned char)mark;
  for (int i = 0; i < n; i++)  // (a), and a chain inside one list
    for (int j = 0; j < i; j++)
      if (list[2 * i] == list[2 * j]) return r;
  for (int e = 0; e < ne; e++)  // (c)
    if (tc_clip_joins_second(flg[edges[2 * e]], flg[edges[2 * e + 1]], bit, mark)) return r;
  return r | TC_CLIP_MERGE;
}

#endif  // TC_CLIP_H
