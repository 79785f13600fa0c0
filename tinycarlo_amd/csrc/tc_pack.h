// One-word list entries of the camera stage's register-held path (cam_group_regs, k_camera.h).
//
// A fix-up list entry and a draw-compaction entry name an edge slot of the group and the edge's two end nodes, all three
// relative to the group and so below K * 64 (K: register-cache slots per lane, at most 13: 832).  Ten bits each make one
// 32-bit word where the windowed path keeps two ints (edge id; target | other << 16):
//
//     bits 20..29  edge id        bits 10..19  the other end (the one that stays)        bits 0..9  the target node
//
// The edge id sits on top, so two entries compare as their edge ids do (edge ids of one list are distinct): the chain
// replay, which follows a target's moves in ascending edge id, may compare whole words.  Bits 30 and 31 stay clear: an
// entry is a non-negative int, and -1 is free to mean "no entry".
// Projection candidates are node ids alone and travel as 16-bit values.
// Plain C / HIP like tc_clip.h: the tests build this header with the host compiler.
#ifndef TC_PACK_H
#define TC_PACK_H
#include "tc_trig.h" /* TC_HD */

#define TC_PACK_BITS 10
#define TC_PACK_IDS (1 << TC_PACK_BITS)  // ids an entry can name: every K with K * 64 <= this may use the format
#define TC_PACK_MASK (TC_PACK_IDS - 1)
#define TC_PACK_FITS(K) ((K) * 64 <= TC_PACK_IDS)

TC_HD int tc_pack(int edge, int target, int other) { return (edge << (2 * TC_PACK_BITS)) | (other << TC_PACK_BITS) | target; }
TC_HD int tc_pack_edge(int w) { return (int)((unsigned)w >> (2 * TC_PACK_BITS)); }
TC_HD int tc_pack_target(int w) { return w & TC_PACK_MASK; }
TC_HD int tc_pack_other(int w) { return (w >> TC_PACK_BITS) & TC_PACK_MASK; }

// bytes of the list region for camera groups of at most cap_n nodes and cap_e edges: the packed edge list or the 16-bit
// candidate list, whichever is larger (the same 16 bytes of slack the two-int form has)
TC_HD int tc_pack_list_bytes(int cap_n, int cap_e) { return (4 * cap_e > 2 * cap_n ? 4 * cap_e : 2 * cap_n) + 16; }

#endif  // TC_PACK_H
