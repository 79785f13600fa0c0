// tc_collect.h -- the rules of the sample buffer (tc_collect, include/tinycarlo_hip.h): which rows of a K-step call are
// samples, which slot a sample goes to, and which samples of a call are written at all.  The executable definition is
// tinycarlo_amd/collect.py (collect_reference); this header restates it for the kernels of k_collect.h and for the CPU tests,
// which build it alone with the host compiler (tests/collect_shim.py) and run whole calls sequentially through it.
//
// What is restated: the pairing of examples/train_stanley_il.py:69-75 (the frame BEFORE a step with that step's command),
// its `i % SKIP_STEPS == 0` per episode (:70), the stop at BUFFER_SIZE (:100-110) and Replaybuffer.add of
// examples/rl_utils.py:19-22 (overwrite a random slot once full), plus a plain ring.
// HIP-free, TC_HD like tc_rng.h.
#ifndef TC_COLLECT_H
#define TC_COLLECT_H
#include <stdint.h>

#include "../../include/tinycarlo_hip.h" /* TC_COLLECT_* */
#include "tc_rng.h"                      /* TC_HD, tc_replace_slot */

// One row of one env (rules 1-3): `done` = terminated | truncated of the row.  Returns 1 when the row is a candidate.
// A pending env's row is the re-spawn row: no action was applied, no sample; the episode's step count starts over.
TC_HD int tc_collect_env_step(uint8_t* pending, int32_t* age, int32_t stride, int done) {
  int cand = 0;
  if (*pending) {
    *age = 0;
  } else {
    const int32_t i = *age;
    *age = i + 1;
    cand = (i % stride) == 0;
  }
  *pending = done ? 1 : 0;
  return cand;
}

// Slot of ordinal o (>= 0), or -1 where the candidate is dropped.
TC_HD int64_t tc_collect_slot(int mode, uint64_t seed, int64_t o, int64_t cap) {
  if (o < cap) return o;
  if (mode == TC_COLLECT_RING) return o % cap;
  if (mode == TC_COLLECT_RANDOM) return (int64_t)tc_replace_slot(seed, (uint64_t)o, (uint32_t)cap);
  return -1;
}

// Does ordinal o of a call that started at next_ordinal = o0 and has c candidates get written?  Where several candidates
// of a call share a slot the highest ordinal wins:
//   stop    every kept candidate has a slot of its own;
//   ring    the last `cap` ordinals of the call have distinct slots and beat every earlier one;
//   random  decided by the slots themselves: pass 1 raises ordinal[slot] to the highest claimant (ordinals only grow, so
//           what earlier calls left there is lower), and the candidate writes iff it finds its own ordinal (`claimed`).
TC_HD int tc_collect_writes(int mode, int64_t o, int64_t o0, int64_t c, int64_t cap, int64_t claimed) {
  if (mode == TC_COLLECT_STOP) return o < cap;
  if (mode == TC_COLLECT_RING) return o >= o0 + c - cap;
  return claimed == o;
}

// The counter block after a call with c candidates.
TC_HD void tc_collect_advance(int mode, int64_t c, int64_t cap, int64_t* counters) {
  const int64_t o0 = counters[TC_COLLECT_NEXT], o1 = o0 + c;
  if (mode == TC_COLLECT_STOP) counters[TC_COLLECT_DROPPED] += (o1 > cap ? o1 - cap : 0) - (o0 > cap ? o0 - cap : 0);
  counters[TC_COLLECT_COUNT] = o1 < cap ? o1 : cap;
  counters[TC_COLLECT_NEXT] = o1;
  counters[TC_COLLECT_LAST_CALL] = c;
}

// Scratch of a call of `rows` rows over `n_envs` envs: a 16-byte head (o0 and c of the call), then per (row, wavefront of 64
// envs) the 64 candidate flags as one 64-bit mask and the rank of the wavefront's first candidate within the call.
TC_HD int64_t tc_collect_waves(int32_t n_envs) { return ((int64_t)n_envs + 63) / 64; }
TC_HD int64_t tc_collect_scratch_size(int32_t rows, int32_t n_envs) {
  if (rows < 1 || n_envs < 1) return 0;
  const int64_t cells = (int64_t)rows * tc_collect_waves(n_envs);
  return 16 + cells * 8 + (cells * 4 + 15) / 16 * 16;
}

// ---- frame histories (TC_HAS_HISTORY): a link per slot to the sample that precedes it in its episode, so that a sample
// of ReplaybufferTemporal (examples/rl_utils.py:32-57: what the env showed over the last SEQ_LEN steps, newest first,
// examples/train_td3.py:164,175-176) is gathered from single-frame slots.  chain[n] = ordinal of env n's most recent
// candidate of the running episode (-1: none), prev[slot] = ordinal of the sample before the slot's (-1: the episode
// started there).  Definition: collect_reference / history_reference of tinycarlo_amd/collect.py.

// One row of one env, beside tc_collect_env_step: `respawn` = the env was pending BEFORE the row (rule 1), `cand` = the row
// is a candidate with ordinal o (rule 2).  Returns the candidate's link (what prev[slot] becomes if o is written); the chain
// moves on whether or not o is written.  A row skipped by the stride touches nothing.
TC_HD int64_t tc_collect_chain_step(int64_t* chain, int respawn, int cand, int64_t o) {
  if (respawn) {
    *chain = -1;
    return -1;
  }
  if (!cand) return -1;
  const int64_t link = *chain;
  *chain = o;
  return link;
}

// The history of slot s, newest first, into slots[0 .. T-1]; returns the number of entries found (0: s is outside the
// buffer or empty).  The walk stops where the episode started (prev < 0) or where the predecessor was dropped or
// overwritten (its slot holds another ordinal); ordinals strictly decrease along a chain.  The rest is -1, or with
// pad_edge the last slot found.
TC_HD int32_t tc_history_walk(const int64_t* prev, const int64_t* ordinal, int mode, uint64_t seed, int64_t cap, int64_t s,
                              int32_t T, int pad_edge, int64_t* slots) {
  int32_t valid = 0;
  if (s >= 0 && s < cap && ordinal[s] >= 0) {
    slots[0] = s;
    valid = 1;
    while (valid < T) {
      const int64_t p = prev[s];
      if (p < 0) break;
      const int64_t q = tc_collect_slot(mode, seed, p, cap);
      if (q < 0 || ordinal[q] != p) break;
      slots[valid++] = s = q;
    }
  }
  const int64_t fill = pad_edge && valid > 0 ? s : -1;
  for (int32_t t = valid; t < T; t++) slots[t] = fill;
  return valid;
}
#endif
