// k_feat.h -- the per-env feature blocks of the simulate stages: reward / termination terms (tinycarlo/wrapper/*.py, the
// epilogue of a step), the TC_FEAT_* template mask, per-env car rows, the camera bank, episodes, the built-in controller
// (tc_ctrl.h) and the drive randomisation behind it.  Defines no kernel: sim_body (k_sim.h) and the grouped kernel (k_envg.h)
// compile these in by mask.
#ifndef K_FEAT_H
#define K_FEAT_H

#include "k_common.h"
#include "tc_ctrl.h"
#include "tc_rng.h"

// ---------------------------------------------------------------------------------------------
// Reward / termination wrappers (tinycarlo/wrapper/*.py) as an epilogue of the step.  Every lane runs the same
// scalar code; dist_l is lane l's laneline distance (lanes >= C hold 0) and is broadcast layer by layer so that
// the additions happen in the dict order of info["laneline_distances"] (env.py:85, reward.py:20,40).
__device__ inline double d_linear_reward(double x, double max_x, double max_reward, double min_reward) {
  double y = (-max_reward / max_x) * tc_fabs(x) + max_reward;  // utils.py:33
  if (max_reward > 0) return (min_reward > y) ? min_reward : y;  // python max(y, min_reward)
  return (min_reward < y) ? min_reward : y;                      // python min(y, min_reward)
}

// ---------------------------------------------------------------------------------------------
// Per-env features of the simulate stages: ONE template parameter (FEAT, a mask of these bits) of sim_body and of the
// three kernels that simulate -- tc_step_kernel<.., FEAT>, tc_env_kernel<.., FEAT>, tc_envg_kernel<FEAT>; a kernel trace
// shows the mask as a number (tc_envg_kernel<3u>: both).  launch() sets the bits of a call (`feat`).
//   bit              compiles in                                                           reads
//   TC_FEAT_CAR (1)  car constants from the env's row, re-drawn at every re-spawn          StepArgs::cr
//   TC_FEAT_EP  (2)  episode length / return / time limit and the finished-episode sums    StepArgs::ep
//   TC_FEAT_CTRL (4) the action computed on the device by the built-in controller           StepArgs::ct
// A kernel without a bit contains none of that feature's code and compiles as if the feature did not exist.
// The masks with TC_FEAT_CTRL are instantiations of three entry points of their own over the same bodies --
// tc_drive_step_kernel, tc_drive_env_kernel, tc_drive_envg_kernel (masks 4-7) -- so the twelve-plus-four kernels of masks
// 0-3 keep their names and their number, and a kernel trace tells a closed-loop call from an open-loop one by name.
enum : unsigned { TC_FEAT_CAR = 1, TC_FEAT_EP = 2, TC_FEAT_ALL = TC_FEAT_CAR | TC_FEAT_EP, TC_FEAT_CTRL = 4 };

// ---------------------------------------------------------------------------------------------
// Per-env car constants (tc_env_set_car_per_env): row [env][TC_CAR_NP] of a caller-owned device buffer replaces the
// shared car's wheelbase, track width and limits; T and the two presence flags stay shared.  Only the TC_FEAT_CAR kernels
// (the PER instantiations of the simulate stages, chosen at launch) read it: the shared-car kernels compile as before.
// With tc_env_set_car_randomization, every re-spawn draws the masked columns of the env's next episode first
// (tc_car_stream / tc_car_draw, tc_rng.h) and writes them back to the row, so the row always holds the constants in force.
struct CarDrawTab {  // library owned, updated in place by tc_env_set_car_randomization (a captured graph sees new ranges)
  double lo[TC_CAR_NP], hi[TC_CAR_NP];
  unsigned long long seed;
  unsigned int mask, env_offset;  // mask 0: no resampling
};
struct CarRows {
  double* rows;           // [N][TC_CAR_NP] (caller owned)
  const CarDrawTab* tab;  // NULL: no resampling
  int* episode;           // [N] episodes drawn so far (caller owned)
};
typedef const __attribute__((address_space(4))) CarDrawTab* CarDrawTabConst;  // never written by a kernel: scalar loads

// a constant of the env's row, read where it is used (UNI: the env is wave-uniform, the value goes to SGPRs)
template <bool UNI>
__device__ __forceinline__ double car_ld(const double* row, int j) {
  return UNI ? uni_d(row[j]) : row[j];
}
// the env's car: shared T and presence flags, the rest from its row (unused loads are dropped by the compiler)
template <bool UNI>
__device__ __forceinline__ DevCar car_of(const DevCar& shared, const double* row) {
  DevCar c = shared;
  c.wheelbase = car_ld<UNI>(row, TC_CAR_WHEELBASE);
  c.track_width = car_ld<UNI>(row, TC_CAR_TRACK_WIDTH);
  c.max_velocity = car_ld<UNI>(row, TC_CAR_MAX_VELOCITY);
  c.max_steering_angle = car_ld<UNI>(row, TC_CAR_MAX_STEERING_ANGLE);
  c.steering_speed = car_ld<UNI>(row, TC_CAR_STEERING_SPEED);
  c.max_acceleration = car_ld<UNI>(row, TC_CAR_MAX_ACCELERATION);
  c.max_deceleration = car_ld<UNI>(row, TC_CAR_MAX_DECELERATION);
  return c;
}
// A re-spawn of env `env` (before d_reset): the masked columns of its next episode's row, and the episode counter.  The
// writer stores them; every lane that reads the row later is of the same wavefront (stores and loads in program order).
template <bool UNI>
__device__ __forceinline__ void car_respawn(const CarRows& cr, int env, bool writer) {
  if (!cr.tab) return;
  const CarDrawTabConst t = (CarDrawTabConst)(unsigned long long)cr.tab;
  const unsigned int mask = t->mask;
  if (mask == 0) return;
  const int ep = UNI ? uni_i(cr.episode[env]) : cr.episode[env];
  const uint64_t z = tc_car_stream(t->seed, (uint32_t)(t->env_offset + (unsigned int)env), (uint32_t)ep);
  double* row = cr.rows + (size_t)env * TC_CAR_NP;
#pragma unroll
  for (int j = 0; j < TC_CAR_NP; j++)
    if ((mask >> j) & 1u) {
      const double v = tc_car_draw(z, j, t->lo[j], t->hi[j]);
      if (writer) row[j] = v;
    }
  if (writer) cr.episode[env] = ep + 1;
}

// ---------------------------------------------------------------------------------------------
// Camera bank (tc_env_set_camera_bank): KArgs::cam_E / cam_K hold `count` cameras, each env an index into them that every
// re-spawn re-draws (tc_camera_index, tc_rng.h).  E is consumed where the pose row is formed, K later by the frame stage --
// in a K-step call possibly after the env has re-spawned again -- so the index in force at a step travels with that
// (step, env): entry 12 of its pose row (or a register, where the same wavefront draws the frame).  A run-time branch on
// TC_FI_CAM_BANK in every simulate kernel (no instantiation of its own, as cam_E is); the frame kernels branch on FrameArgs::bank.
// Set by the library in StepArgs::flags of every launch while a bank is installed: the kernels branch on this bit of a word
// they hold anyway instead of fetching a pointer of their argument block per step to test it (never taken from the caller).
#define TC_FI_CAM_BANK 0x80000000u
// Likewise set by the library, from the call's plan (CallPlan::info_every, tc_plan.h): every step of the launch computes
// the lane-line distances (phase B of the simulate stages).  Clear, only the launch's last step does: nothing reads another
// step's -- no rollout rows for them, no term that looks at distances -- and the env's buffers take the last step's.
#define TC_FI_INFO_EVERY 0x08000000u
struct CamDrawTab {  // library owned, updated in place by tc_env_set_camera_bank (a captured graph sees new settings)
  unsigned long long seed;
  unsigned int count, env_offset;
};
struct CamBank {
  int* index;             // [N] the camera each env uses now (caller owned); NULL: no bank (TC_FI_CAM_BANK clear)
  int* rows;              // [K][N] the index in force at each step of a K-step call, first row of this launch; or NULL
  int* episode;           // [N] cameras drawn so far (caller owned)
  const CamDrawTab* tab;
};
typedef const __attribute__((address_space(4))) CamDrawTab* CamDrawTabConst;  // never written by a kernel: scalar loads
// an index as read from memory, kept inside the bank whatever the caller's buffer holds
__device__ __forceinline__ int cam_clamp(const CamBank& cb, int idx) {
  const unsigned int last = ((CamDrawTabConst)(unsigned long long)cb.tab)->count - 1u;
  return (int)((unsigned int)idx < last ? (unsigned int)idx : last);
}
// A re-spawn of env `env`: the camera of its next episode.  The writer stores index and counter (as car_respawn does).
template <bool UNI>
__device__ __forceinline__ int cam_respawn(const CamBank& cb, int env, bool writer) {
  const CamDrawTabConst t = (CamDrawTabConst)(unsigned long long)cb.tab;
  const int ep = UNI ? uni_i(cb.episode[env]) : cb.episode[env];
  const int idx = (int)tc_camera_index(t->seed, (uint32_t)(t->env_offset + (unsigned int)env), (uint32_t)ep, t->count);
  if (writer) {
    cb.index[env] = idx;
    cb.episode[env] = ep + 1;
  }
  return idx;
}

// ---------------------------------------------------------------------------------------------
// Episode time limit and per-env episode statistics (tc_env_set_episodes).  Only the TC_FEAT_EP kernels (the EP instantiations
// of the simulate stages, chosen at launch) touch any of this: every other kernel compiles as before.  Per env and step:
//   re-spawned in this step (tc_reset, autoreset)  length = 0, ret = 0.0, nothing else
//   TC_S_NOT_RESET                                 left alone
//   else  length += 1; limit > 0 && length >= limit: truncated = 1, status |= TC_S_TIME_LIMIT   (ep_count, every lane)
//         ret = ret + reward, with the step's FINAL reward: one double add per step, in step order
//         terminated | truncated: last_* = (length, ret), count += 1, *_sum += (length, ret)   (ep_close, one lane)
// length / ret stay on chip across the steps of a launch (LiveLds, or registers in the grouped kernel) and go back to the
// caller's buffers once; the finished-episode statistics are rare and go straight to memory.
struct EpArgs {
  int* length;           // [N] caller owned, as are the next seven
  double* ret;
  int* count;            // (count .. return_sum: each may be NULL)
  int* last_length;
  double* last_return;
  long long* length_sum;
  double* return_sum;
  const int* limit;      // [N] per-env limit, or NULL: *shared
  const int* shared;     // library owned, updated in place by tc_env_set_episodes (a captured graph sees a new limit)
  int* len_rows;         // [K][N] rows of a K-step call (tc_step_rows.episode_*_out), first row of this launch; or NULL
  double* ret_rows;
};
typedef const __attribute__((address_space(4))) int* EpIntConst;  // never written by a kernel: scalar load
// first half, before truncated / status are stored: the length, and the time limit (gymnasium TimeLimit: whatever
// `terminated` turns out to be).  Every lane that works on the env runs it, so truncated stays uniform among them.
template <bool UNI>
__device__ __forceinline__ void ep_count(const EpArgs& ep, int env, bool fresh, int& len, int& trunc, int& status) {
  if (fresh) {
    len = 0;
    return;
  }
  if (status & TC_S_NOT_RESET) return;
  len += 1;
  const int lim = ep.limit ? (UNI ? uni_i(ep.limit[env]) : ep.limit[env]) : *(EpIntConst)(unsigned long long)ep.shared;
  if (lim > 0 && len >= lim) {
    trunc = 1;
    status |= TC_S_TIME_LIMIT;
  }
}
// second half, by the one lane that stores the env's outputs, once reward / terminated are final; row: (step, env) of
// the launch's per-step rows
__device__ __forceinline__ void ep_close(const EpArgs& ep, int env, size_t row, bool fresh, int status, int len, double& ret,
                                         double reward, int done) {
  if (fresh) {
    ret = 0.0;
  } else if (!(status & TC_S_NOT_RESET)) {
    ret = ret + reward;
    if (done) {
      if (ep.last_length) ep.last_length[env] = len;
      if (ep.last_return) ep.last_return[env] = ret;
      if (ep.count) ep.count[env] += 1;
      if (ep.length_sum) ep.length_sum[env] += (long long)len;
      if (ep.return_sum) ep.return_sum[env] = ep.return_sum[env] + ret;
    }
  }
  if (ep.len_rows) ep.len_rows[row] = len;
  if (ep.ret_rows) ep.ret_rows[row] = ret;
}

// ---------------------------------------------------------------------------------------------
// Built-in controller (tc_env_set_controller, tc_ctrl.h).  Only the TC_FEAT_CTRL kernels (the tc_drive_* entry points,
// chosen at launch) touch any of this: every other kernel compiles as before.  Per env and step the action is
//   (speed, tc_ctrl_stanley(cte, he, k, speed, max_steering_angle) + noise[k][env])
// with cte / he as the env reported them after its previous step (the bound buffers at the first step of a launch, 0 / 0
// after a re-spawn), max_steering_angle the env's own (its car row under TC_FEAT_CAR), and car_control is never read.
// The command before noise goes to rows[k][env] / last[env]; a step that applies no action (re-spawn, TC_S_NOT_RESET)
// stores 0.0 there.
struct CtrlTab {  // library owned, updated in place by tc_env_set_controller (a captured graph sees new gains)
  double k, speed;
};
struct CtrlArgs {
  const CtrlTab* tab;
  const double* noise;  // [K][N] from the first step of this launch on, or NULL
  double* rows;         // likewise, out
  double* last;         // [N] out, or NULL
};
typedef const __attribute__((address_space(4))) CtrlTab* CtrlTabConst;  // never written by a kernel: scalar loads
// the steering command of one env (before noise), and the velocity command
__device__ __forceinline__ double ctrl_command(const CtrlArgs& ct, double cte, double he, double msa, double& speed) {
  const CtrlTabConst t = (CtrlTabConst)(unsigned long long)ct.tab;
  speed = t->speed;
  return tc_ctrl_stanley(cte, he, t->k, speed, msa);
}
// by the one lane that stores the env's outputs; row: (step, env) of the launch's per-step rows
__device__ __forceinline__ void ctrl_store(const CtrlArgs& ct, int env, size_t row, double steer) {
  if (ct.rows) ct.rows[row] = steer;
  if (ct.last) ct.last[env] = steer;
}

// ---------------------------------------------------------------------------------------------
// Drive randomisation (tc_env_set_drive_randomization): the maneuver as a per-episode quantity and Ornstein-Uhlenbeck
// steering noise, both following the episode inside a call.  Lives in the TC_FEAT_CTRL kernels only, behind two bits the
// library sets in StepArgs::flags of every launch while the part is installed (run-time branches, as for TC_FI_CAM_BANK:
// no instantiation of its own; never taken from the caller):
//   TC_FI_DRIVE_MAN  candidates are installed: the maneuver of an action step is maneuver[env], re-drawn at every re-spawn
//                    (tc_maneuver_index, or the cycle), and the call's maneuver rows are not read
//   TC_FI_DRIVE_OU   ou_state is installed: every action step consumes one normal (tc_normal_at, evaluated right here: one
//                    tc_log, one sqrt and one tc_cos next to the controller's tc_atan2 and the kinematics' tc_sin / tc_cos,
//                    where few registers are live) and adds the new OU value behind the controller's own noise row
// The grouped kernel keeps the three per-env values in a per-group LDS word across the steps of a launch and stores them
// once; the per-env kernels read and write the caller's arrays where the step needs them (by the lane that stores the env's
// outputs, read back by lanes of the same wavefront, as the car rows are): the LiveLds record has one spare int (`pad`) and
// the three values need 16 bytes; 12 more would move TC_LIVE_BYTES, which the LDS budget of every kernel is laid out around.
#define TC_FI_DRIVE_MAN 0x20000000u
#define TC_FI_DRIVE_OU 0x10000000u
#define TC_FI_DRIVE (TC_FI_DRIVE_MAN | TC_FI_DRIVE_OU)
#define TC_MAX_MANEUVERS 8
struct DriveTab {  // library owned, updated in place by tc_env_set_drive_randomization (a captured graph sees new settings)
  unsigned long long seed;
  double theta, mu, sigma;
  unsigned int env_offset;
  int n_man, mode, ou_reset;
  int man[TC_MAX_MANEUVERS];
};
struct DriveArgs {
  const DriveTab* tab;  // NULL: off
  int* maneuver;        // [N] the maneuver in force (caller owned, as are the next three)
  int* episode;         // [N] episodes drawn so far
  double* ou_state;     // [N] or NULL
  int* ou_draws;        // [N] normals consumed so far
  int* man_rows;        // [K][N] from the first step of this launch on, out, or NULL
  double* noise_rows;   // likewise
};
typedef const __attribute__((address_space(4))) DriveTab* DriveTabConst;  // never written by a kernel: scalar loads
// the maneuver of episode `ep` of env `env` (n candidates, n > 0)
__device__ __forceinline__ int drive_pick(const DriveTabConst t, int n, int env, int ep) {
  const unsigned int g = t->env_offset + (unsigned int)env;
  const unsigned int i = t->mode == TC_MAN_CYCLE ? (g + (unsigned int)ep) % (unsigned int)n
                                                 : tc_maneuver_index(t->seed, g, (uint32_t)ep, (uint32_t)n);
  return t->man[i < TC_MAX_MANEUVERS ? i : 0];
}
// A re-spawn of env `env` (TC_FI_DRIVE_MAN): the maneuver of its next episode; the writer stores the counter.  `held` is
// returned while the table holds no candidate.
template <bool UNI>
__device__ __forceinline__ int drive_respawn_man(const DriveArgs& dr, int env, bool writer, int held) {
  const DriveTabConst t = (DriveTabConst)(unsigned long long)dr.tab;
  const int n = t->n_man;
  if (n <= 0) return held;
  const int ep = UNI ? uni_i(dr.episode[env]) : dr.episode[env];
  const int m = drive_pick(t, n < TC_MAX_MANEUVERS ? n : TC_MAX_MANEUVERS, env, ep);
  if (writer) dr.episode[env] = ep + 1;
  return m;
}
// An action step of env `env` (TC_FI_DRIVE_OU): normal number `draws` of the env moves its OU value `ou`
__device__ __forceinline__ double drive_ou(const DriveArgs& dr, int env, double ou, int draws) {
  const DriveTabConst t = (DriveTabConst)(unsigned long long)dr.tab;
  const double eps = tc_normal_at(t->seed, (uint32_t)(t->env_offset + (unsigned int)env), (uint32_t)draws);
  return tc_ou_step(ou, eps, t->theta, t->mu, t->sigma);
}
__device__ __forceinline__ bool drive_ou_reset(const DriveArgs& dr) {
  return ((DriveTabConst)(unsigned long long)dr.tab)->ou_reset != 0;
}
// by the one lane that stores the env's outputs; row: (step, env) of the launch's per-step rows
__device__ __forceinline__ void drive_store(const DriveArgs& dr, size_t row, int man, double noise) {
  if (dr.man_rows) dr.man_rows[row] = man;
  if (dr.noise_rows) dr.noise_rows[row] = noise;
}

// (scalars by value: a reference to the kernel-argument struct would force a copy of it into scratch)
// my_cnt: lane t < TC_MAX_TERMS holds steps_true of term slot t (loaded at kernel start, stored by the caller)
__device__ __forceinline__ void d_apply_terms(const tc_term* terms, int n_terms, int& my_cnt, double tw, int tid, int C,
                                              double cte, double vel, double dist_l, double& reward, int& terminated) {
  const double half = tw / 2;
  for (int t = 0; t < n_terms; t++) {
    const tc_term* T = terms + t;
    const int kind = T->kind;
    const unsigned mask = T->layer_mask;
    if (kind == TC_T_LANELINE_SPARSE_REWARD) {  // reward.py:20-21, utils.py:15-19
      double local = 0.0;
      for (int l = 0; l < C; l++) {
        const double d = d_readlane(dist_l, l);
        if (((mask >> l) & 1u) && d < half) local += T->per_layer[l];
      }
      reward = reward + local;
    } else if (kind == TC_T_LANELINE_LINEAR_REWARD) {  // reward.py:40-41
      for (int l = 0; l < C; l++) {
        const double d = d_readlane(dist_l, l);
        reward = reward + d_linear_reward(d, tw, T->per_layer[l], 0.0);
      }
    } else if (kind == TC_T_CTE_SPARSE_REWARD) {  // reward.py:60
      double local = 0.0;
      if (tc_fabs(cte) <= T->p[0]) local += T->p[1];
      reward = reward + local;
    } else if (kind == TC_T_CTE_LINEAR_REWARD) {  // reward.py:83
      reward = reward + d_linear_reward(cte, T->p[0], T->p[1], T->p[2]);
    } else if (kind == TC_T_LANELINE_CROSSING_TERMINATION) {  // termination.py:19-21
      for (int l = 0; l < C; l++) {
        const double d = d_readlane(dist_l, l);
        if (((mask >> l) & 1u) && d <= half) terminated = 1;
      }
    } else if (kind == TC_T_CTE_TERMINATION || kind == TC_T_CRASH_TERMINATION) {  // termination.py:39-47,61-69
      const bool cond = kind == TC_T_CTE_TERMINATION ? (tc_fabs(cte) > T->p[0]) : (tc_fabs(vel) < T->p[0]);
      int c = __builtin_amdgcn_readlane(my_cnt, t);
      if (cond) {
        c += 1;
        if (c >= T->number_of_steps) {
          terminated = 1;
          c = 0;
        }
      } else {
        c = 0;
      }
      if (tid == t) my_cnt = c;
    }
  }
}

// The same stack for the grouped simulate kernel, where every lane of an env's group runs it: distances and counters
// of the env sit in a small LDS record (all lanes of the group read and write the same words with the same values).
__device__ __forceinline__ void d_apply_terms_mem(const tc_term* terms, int n_terms, int* cnt, double tw, int C, double cte,
                                                  double vel, const double* dist, double& reward, int& terminated) {
  const double half = tw / 2;
  for (int t = 0; t < n_terms; t++) {
    const tc_term* T = terms + t;
    const int kind = T->kind;
    const unsigned mask = T->layer_mask;
    if (kind == TC_T_LANELINE_SPARSE_REWARD) {  // reward.py:20-21, utils.py:15-19
      double local = 0.0;
      for (int l = 0; l < C; l++)
        if (((mask >> l) & 1u) && dist[l] < half) local += T->per_layer[l];
      reward = reward + local;
    } else if (kind == TC_T_LANELINE_LINEAR_REWARD) {  // reward.py:40-41
      for (int l = 0; l < C; l++) reward = reward + d_linear_reward(dist[l], tw, T->per_layer[l], 0.0);
    } else if (kind == TC_T_CTE_SPARSE_REWARD) {  // reward.py:60
      double local = 0.0;
      if (tc_fabs(cte) <= T->p[0]) local += T->p[1];
      reward = reward + local;
    } else if (kind == TC_T_CTE_LINEAR_REWARD) {  // reward.py:83
      reward = reward + d_linear_reward(cte, T->p[0], T->p[1], T->p[2]);
    } else if (kind == TC_T_LANELINE_CROSSING_TERMINATION) {  // termination.py:19-21
      for (int l = 0; l < C; l++)
        if (((mask >> l) & 1u) && dist[l] <= half) terminated = 1;
    } else if (kind == TC_T_CTE_TERMINATION || kind == TC_T_CRASH_TERMINATION) {  // termination.py:39-47,61-69
      const bool cond = kind == TC_T_CTE_TERMINATION ? (tc_fabs(cte) > T->p[0]) : (tc_fabs(vel) < T->p[0]);
      int c = cnt[t];
      if (cond) {
        c += 1;
        if (c >= T->number_of_steps) {
          terminated = 1;
          c = 0;
        }
      } else {
        c = 0;
      }
      cnt[t] = c;
    }
  }
}

#endif  // K_FEAT_H
