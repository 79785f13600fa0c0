// Counter-based spawn sampling for device-side auto-reset ("throughput mode").
//
// Not a restatement of anything in the reference -- its resets draw from the env's numpy PCG64 generator
// (map.py:61), which stays available as the seed-parity mode (host-drawn spawn_queue).  Here the k-th re-spawn of env
// e takes output number n = (e << 32 | k) of the SplitMix64 sequence started at `seed` (Steele, Lea, Flood 2014:
// z = seed + (n+1)*0x9E3779B97F4A7C15, then the two xor-shift-multiply rounds), i.e. random access into one
// stream, no per-env generator state besides the reset counter that already exists (spawn_cursor).
// The table holds the candidates of map.py:61 that have an out-edge (duplicates kept), so a uniform draw from it has
// the distribution of the reference's draw-again-on-sinks loop (map.py:62-64).
// Plain C / HIP like tc_trig.h: the CPU test oracle includes this header too (the package never includes the oracle).
#ifndef TC_RNG_H
#define TC_RNG_H
#include <math.h> /* sqrt */
#include <stdint.h>

#include "tc_trig.h" /* TC_HD, tc_log, tc_cos */

TC_HD uint64_t tc_splitmix64_at(uint64_t seed, uint64_t n) {
  uint64_t z = seed + (n + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// index into a table of `count` (> 0) entries for re-spawn number `cursor` of env `env`:
// high 32 bits scaled by count (Lemire's multiply-shift; bias <= count / 2^32)
TC_HD uint32_t tc_spawn_index(uint64_t seed, uint32_t env, uint32_t cursor, uint32_t count) {
  uint64_t z = tc_splitmix64_at(seed, ((uint64_t)env << 32) | cursor);
  return (uint32_t)(((z >> 32) * (uint64_t)count) >> 32);
}

// Per-episode car parameters (tc_env_set_car_randomization).  Episode `episode` of env `env` (global index: the
// caller's env_offset + the env's index in the batch) draws column j of its row as lo_j + (hi_j - lo_j) * u_j with
// u_j = the top 53 bits of output j of the sub-stream SplitMix64(s')[env << 32 | episode], s' = SplitMix64(seed)[0x636172]
// ("car": a stream of its own, apart from the spawn stream of the same seed).  u_j is in [0, 1), so lo == hi gives lo.
// Two roundings (the product, then the sum): the library and the oracle are built with -ffp-contract=off.
TC_HD uint64_t tc_car_stream(uint64_t seed, uint32_t env, uint32_t episode) {
  return tc_splitmix64_at(tc_splitmix64_at(seed, 0x636172ull), ((uint64_t)env << 32) | episode);
}
TC_HD double tc_car_draw(uint64_t z, int j, double lo, double hi) {
  const double u = (double)(tc_splitmix64_at(z, (uint64_t)j) >> 11) * 0x1p-53;
  return lo + (hi - lo) * u;
}

// Per-episode camera from a bank of `count` (> 0) cameras (tc_env_set_camera_bank).  Episode `episode` of env `env` (global
// index, as for the cars) takes the camera whose index is the high 32 bits of output (env << 32 | episode) of the sub-stream
// s' = SplitMix64(seed)[0x63616D] ("cam": apart from the car and spawn streams of the same seed), scaled by count as in
// tc_spawn_index.  count == 1 gives 0.
TC_HD uint32_t tc_camera_index(uint64_t seed, uint32_t env, uint32_t episode, uint32_t count) {
  const uint64_t z = tc_splitmix64_at(tc_splitmix64_at(seed, 0x63616Dull), ((uint64_t)env << 32) | episode);
  return (uint32_t)(((z >> 32) * (uint64_t)count) >> 32);
}

// Drive randomisation (tc_env_set_drive_randomization): the maneuver of an episode and the Ornstein-Uhlenbeck steering noise
// of examples/train_stanley_il.py:66,105 and examples/train_td3.py:143,178, each on a sub-stream of its own.
// Episode `episode` of env `env` (global index) takes candidate number tc_maneuver_index of `count` (> 0): the high 32 bits of
// output (env << 32 | episode) of s' = SplitMix64(seed)[0x6D616E] ("man"), scaled by count as in tc_camera_index.
TC_HD uint32_t tc_maneuver_index(uint64_t seed, uint32_t env, uint32_t episode, uint32_t count) {
  const uint64_t z = tc_splitmix64_at(tc_splitmix64_at(seed, 0x6D616Eull), ((uint64_t)env << 32) | episode);
  return (uint32_t)(((z >> 32) * (uint64_t)count) >> 32);
}
// Standard normal number `draw` of env `env`: Box-Muller over outputs 0 and 1 of SplitMix64(z),
// z = SplitMix64(SplitMix64(seed)[0x6F75])[env << 32 | draw] ("ou").  u1 = ((a >> 11) + 1) * 2^-53 lies in (0, 1], so the
// logarithm is finite and <= 0; u2 = (b >> 11) * 2^-53 in [0, 1).  |result| <= sqrt(106 ln 2) = 8.58, never NaN or infinite.
// tc_log / tc_cos are the portable ones of tc_trig.h, sqrt the correctly rounded IEEE one on both sides, every operation
// rounded on its own (-ffp-contract=off): host and device agree bit for bit.
TC_HD double tc_normal_at(uint64_t seed, uint32_t env, uint32_t draw) {
  const uint64_t z = tc_splitmix64_at(tc_splitmix64_at(seed, 0x6F75ull), ((uint64_t)env << 32) | draw);
  const uint64_t a = tc_splitmix64_at(z, 0), b = tc_splitmix64_at(z, 1);
  const double u1 = (double)((a >> 11) + 1) * 0x1p-53;
  const double u2 = (double)(b >> 11) * 0x1p-53;
  return sqrt(-2.0 * tc_log(u1)) * tc_cos(6.283185307179586 * u2);
}
// noise += THETA * (MEAN - noise) + SIGMA * randn, in the Python expression's order
TC_HD double tc_ou_step(double n, double eps, double theta, double mu, double sigma) {
  return n + (theta * (mu - n) + sigma * eps);
}

// Sample buffer (tc_collect, tc_collect.h), overflow mode "random": the candidate with ordinal `o` (>= capacity) replaces slot
// tc_replace_slot of `capacity` (0 < capacity < 2^32) -- the np.random.randint(0, size) of examples/rl_utils.py:20 as a
// counter-based draw: the high 32 bits of output `o` of s' = SplitMix64(seed)[0x726570] ("rep"), scaled by capacity as in
// tc_camera_index.
TC_HD uint32_t tc_replace_slot(uint64_t seed, uint64_t o, uint32_t capacity) {
  const uint64_t z = tc_splitmix64_at(tc_splitmix64_at(seed, 0x726570ull), o);
  return (uint32_t)(((z >> 32) * (uint64_t)capacity) >> 32);
}

// One blob of NoiseObservationWrapper (wrapper/observation.py:18-20): centre (x, y) inside the frame, radius in
// [1, max_radius), mode 1 = "copy in" with probability 0.3 (else erase), src = the plane copied from.  Blob k of
// (env, step) takes two outputs of the sub-stream SplitMix64(seed)[env << 32 | step].  The reference draws these
// from the global numpy generator; this is the device-side stand-in with the same distributions (src and mode from
// 8 and 24 bits).
typedef struct {
  int32_t x, y, r, mode, src;
} tc_blob;

TC_HD tc_blob tc_noise_blob(uint64_t seed, uint32_t env, uint32_t step, uint32_t k, int W, int H, int max_radius,
                            int C) {
  const uint64_t base = tc_splitmix64_at(seed, ((uint64_t)env << 32) | step);
  const uint64_t a = tc_splitmix64_at(base, 2ull * k), b = tc_splitmix64_at(base, 2ull * k + 1);
  tc_blob o;
  o.x = (int32_t)(((a >> 32) * (uint64_t)W) >> 32);
  o.y = (int32_t)(((a & 0xffffffffull) * (uint64_t)H) >> 32);
  o.r = 1 + (int32_t)(((b >> 32) * (uint64_t)(max_radius - 1)) >> 32);
  o.mode = ((b >> 8) & 0xffffffull) < 5033165ull ? 1 : 0; /* 0.3 * 2^24 */
  o.src = (int32_t)(((b & 0xffull) * (uint64_t)C) >> 8);
  return o;
}
#endif
