// k_envg.h -- the grouped simulate kernels for K-step calls: the two phases of k_sim.h (car.py:70-148, 46-53;
// layer.py:33-44, car.py:55-64) restated for TC_EL = 8 lanes per env, 64 / TC_EL envs per wavefront, state in registers
// for the whole launch, the lanepath records in LDS and -- when every step reads them -- the edge records too.  Holds TC_EL, the tunables TC_ENVG_NT / TC_ENVG_PRIO, GroupLds,
// envg_kernel_body<FEAT>, tc_envg_kernel and tc_drive_envg_kernel (the TC_FEAT_CTRL entry point).  Leaves poses, never
// frames: tc_frame_kernel (k_frame.h) draws them.  Includes k_env.h (StepArgs and its idiom; through it k_sim.h, k_feat.h).
#ifndef K_ENVG_H
#define K_ENVG_H

#include "k_env.h"

// ---------------------------------------------------------------------------------------------
// Grouped simulate kernel for K-step calls: TC_EL lanes per env, 64 / TC_EL envs per wavefront.
// Phases A and B of a step are ~900 + ~900 wave-instructions in the one-wavefront-per-env kernel above, and A is scalar
// work that all 64 lanes repeat.  The chip is bound by vector issue (counters: the frame kernel keeps the VALUs 96 %
// busy, the per-env simulate kernel 71 %), so what a step COSTS is its instruction count.  Here an instruction of phase
// A serves 64 / TC_EL envs at once (control flow may differ between envs: plain SIMT divergence), and phase B gives each
// lane of a group every TC_EL-th edge of a layer -- two distances per edge straight from the map (L1-resident), no
// staging of node distances, an xor butterfly over the group for the argmin -- with the per-layer tail evaluated by
// every lane of the group, so nothing has to be passed around afterwards.  State lives in registers for the whole
// launch.  Per env-step: ~2 300 wave-instructions / 8 envs instead of ~1 700 / 1 env.
// The price is latency (a group of 8 lanes walks 33 edges per layer pass one after the other), which nobody waits for:
// the kernel leaves most of the chip's issue slots free for the frame kernel of the previous call.
#define TC_EL 8
#ifndef TC_ENVG_NT
#define TC_ENVG_NT 256  // threads per workgroup: 4 wavefronts = 32 envs share one LDS copy of the edge records
#endif
#ifndef TC_ENVG_PRIO
#define TC_ENVG_PRIO 3
#endif
// Per env of the workgroup, what the reward / termination terms read and count: one distance per lane-line layer of the
// map and the TC_MAX_TERMS counters.  The block sits in the launch's dynamic LDS, behind the map
// records, sized by plan_envg_lds (tc_plan.h) for the map -- as a static array of TC_MAX_LAYERS doubles and TC_MAX_TERMS
// ints per env it was 5 KB, most of which a five-layer map never touched.
struct GroupLds {
  double* dist;  // [C]
  int* cnt;      // [TC_MAX_TERMS]
};

// Where the edge records are read from matters when the kernel runs beside the frame kernel: a frame wavefront ends
// with ~20 KB of 16-byte stores, and a global load of this kernel issued on the same CU queues behind those bursts in
// the CU's vector-memory pipeline (measured: 22 us per step alone, 35 us beside the frame kernel, 23 us beside a frame
// kernel with its stores switched off).  The edge scan is ~33 loads per lane and step: from LDS it neither waits for
// the stores nor pays an L2 round trip per batch of loads.
//   That holds for a launch whose every step scans (TC_FI_INFO_EVERY).  A launch that scans in its last step only reads
// the records from global memory (ma.map_lds = 0, plan_envg_lds): the workgroup sits on a CU beside the frame workgroups
// for the whole launch, and 12 KB held for 128 steps to be read in one are LDS those cannot have.
typedef const __attribute__((address_space(3))) double* LdsDouble;
template <unsigned FEAT>
__device__ __forceinline__ void envg_kernel_body() {
  constexpr bool PER = (FEAT & TC_FEAT_CAR) != 0, EP = (FEAT & TC_FEAT_EP) != 0, CTRL = (FEAT & TC_FEAT_CTRL) != 0;
  extern __shared__ __align__(16) unsigned char gsm[];
  // Highest issue priority: when this kernel shares the chip with the frame kernel of the previous chunk it is the
  // critical path (a serial chain per step, few instructions), and the frame wavefronts would otherwise crowd it out
  // of the vector issue slots by sheer number (measured: 36 us per step beside them, 21 us alone).
  __builtin_amdgcn_s_setprio(TC_ENVG_PRIO);
  const StepArgs& s0 = step_args();
  const int lane = threadIdx.x, sub = lane & (TC_EL - 1), grp = lane / TC_EL;
  if (s0.ma.resident && lane == 0) __hip_atomic_fetch_add(s0.ma.resident, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int N = s0.a.N;
  int env = s0.a.env0 + blockIdx.x * (TC_ENVG_NT / TC_EL) + grp;
  const bool map_lds = s0.ma.map_lds != 0;
  const LdsDouble l_exy = (LdsDouble)gsm;  // [total_edges][4]: n0.x, n0.y, n1.x, n1.y
  const LdsDouble l_ofw = (LdsDouble)(gsm + (size_t)s0.a.m.total_edges * 32);
  const LdsDouble l_orv = l_ofw + s0.a.m.total_edges;
  const bool fat_lds = s0.ma.fat_lds != 0;
  const size_t fat_off = map_lds ? ((size_t)s0.a.m.total_edges * 48 + 15) / 16 * 16 : 0;
  const FatLds fl = {(const __attribute__((address_space(3))) int*)(gsm + fat_off)};
  if (fat_lds) {  // the table word by word, consecutive lanes on consecutive words (once per launch)
    const int* src = (const int*)s0.a.m.lp_fat;
    __attribute__((address_space(3))) int* dst = (__attribute__((address_space(3))) int*)(gsm + fat_off);
    const int nw = s0.a.m.lpN * (int)(sizeof(LpNode) / 4);
    for (int i = lane; i < nw; i += TC_ENVG_NT) dst[i] = src[i];
    static_assert(sizeof(LpNode) % 16 == 0, "fat node records keep 16-byte alignment in LDS");
  }
  if (map_lds) {
    const DevMap& m0 = s0.a.m;
    __attribute__((address_space(3))) double* w4 = (__attribute__((address_space(3))) double*)gsm;
    __attribute__((address_space(3))) double* wd = w4 + (size_t)m0.total_edges * 4;
    for (int i = lane; i < m0.total_edges; i += TC_ENVG_NT) {
      const double4 q = m0.edge_xy[i];
      w4[4 * i] = q.x;
      w4[4 * i + 1] = q.y;
      w4[4 * i + 2] = q.z;
      w4[4 * i + 3] = q.w;
      wd[i] = m0.ori_fwd[i];
      wd[m0.total_edges + i] = m0.ori_rev[i];
    }
  }
  if (map_lds || fat_lds) __syncthreads();
  const bool live = env < N;  // groups past the last env compute on a copy of it and store nothing
  env = live ? env : N - 1;
  GroupLds gl;
  gl.dist = (double*)(gsm + s0.ma.grp_off + grp * s0.ma.grp_stride);
  gl.cnt = (int*)(gsm + s0.ma.grp_off + grp * s0.ma.grp_stride + s0.ma.cnt_off);
  CarState s;
  int nr = 0, cursor = 0, cursor0 = 0;
  bool have_trig = false;
  {
    const tc_buffers& b = s0.a.b;
    s.x = b.x[env];
    s.y = b.y[env];
    s.theta = b.theta[env];
    s.velocity = b.velocity[env];
    s.steering = b.steering[env];
    s.radius = b.radius[env];
    s.front_x = b.front_x[env];
    s.front_y = b.front_y[env];
    s.cth = s.sth = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s.lp[i] = b.local_path[env * 8 + i];
    s.lp_len = b.lp_len[env];
    s.last_maneuver = b.last_maneuver[env];
    if (s0.flags & TC_F_AUTORESET) {
      nr = b.needs_reset[env];
      cursor = cursor0 = b.spawn_cursor[env];
    }
    // (without terms the counters are never read; the variants with the episode accounting set them all the same, as they
    // always did: leaving the store out moves their register allocation off the recorded 123 / 125 VGPRs)
    if (sub < TC_MAX_TERMS && (EP || s0.a.n_terms > 0))
      gl.cnt[sub] = (s0.a.n_terms > 0 && s0.a.term_counters) ? s0.a.term_counters[(size_t)env * TC_MAX_TERMS + sub] : 0;
    static_assert(TC_EL >= TC_MAX_TERMS, "one lane per term counter");
  }
  // the running episode (EP) waits in LDS between its two uses per step (three registers per lane across the whole step
  // took the kernel from 125 to 129 VGPRs): the length is read and rewritten by every lane of the group with the same
  // value (the time limit decides `truncated`, which all of them branch on), the return by the lane that stores the
  // env's outputs
  __shared__ int g_ep_len[EP ? TC_ENVG_NT / TC_EL : 1];
  __shared__ double g_ep_ret[EP ? TC_ENVG_NT / TC_EL : 1];
  if (EP) {
    g_ep_len[grp] = s0.ep.length[env];
    if (sub == 0) g_ep_ret[grp] = s0.ep.ret[env];
  }
  // the env's camera of the bank (tc_env_set_camera_bank), in LDS for the same reason; every lane of the group writes the
  // same value, and only lanes of this wavefront read it (LDS operations of a wavefront complete in order)
  __shared__ int g_cam_idx[TC_ENVG_NT / TC_EL];
  if (s0.flags & TC_FI_CAM_BANK) g_cam_idx[grp] = cam_clamp(s0.cb, s0.cb.index[env]);
  // drive randomisation (tc_env_set_drive_randomization): the env's maneuver, OU value and draw counter, in LDS like the
  // two above (every lane of the group computes and writes the same values) and back to the caller's arrays once per launch
  __shared__ int g_drv_man[CTRL ? TC_ENVG_NT / TC_EL : 1], g_drv_draws[CTRL ? TC_ENVG_NT / TC_EL : 1];
  __shared__ double g_drv_ou[CTRL ? TC_ENVG_NT / TC_EL : 1];
  if (CTRL && (s0.flags & TC_FI_DRIVE_MAN)) g_drv_man[grp] = s0.dr.maneuver[env];
  if (CTRL && (s0.flags & TC_FI_DRIVE_OU)) {
    g_drv_ou[grp] = s0.dr.ou_state[env];
    g_drv_draws[grp] = s0.dr.ou_draws[env];
  }
  double cte = 0, he = 0, reward = 0;
  if (CTRL) {  // what the env reported after the step before this launch: the controller's input at the first step
    cte = s0.a.b.cte[env];
    he = s0.a.b.heading_error[env];
  }
  int terminated = 0, trunc = 0, status = 0;
  const int nsteps = s0.ma.nsteps;
  // The action of step k+1 is fetched at the top of step k.  Vector-memory operations retire in issue order, so a load
  // issued at the top of a step would come back behind the rollout / pose-row stores of the step before -- each a round
  // trip through a memory pipeline the frame kernel keeps full of 16-byte stores.  Issued a whole step early, the load
  // has long returned when it is used, and the stores behind it are not waited for (raw bits are kept: converting at
  // once would be a wait).
  double2 act_d = make_double2(0.0, 0.0);
  float2 act_f = make_float2(0.f, 0.f);
  int act_m = 0;
  auto fetch_action = [&](int kk) {
    const StepArgs& sq = step_args();
    const size_t r = (size_t)kk * sq.a.N + env;
    if (CTRL) {  // the command is computed where it is applied: only the noise value (act_d.y) travels
      if (sq.ct.noise) act_d.y = sq.ct.noise[r];
    } else if (sq.cdtype == TC_F32)
      act_f = ((const float2*)sq.car_control)[r];
    else
      act_d = ((const double2*)sq.car_control)[r];
    if (!(CTRL && (sq.flags & TC_FI_DRIVE_MAN))) act_m = sq.maneuver[r];  // (device maneuvers: nothing to fetch)
  };
  fetch_action(0);
  for (int k = 0; k < nsteps; k++) {
    const StepArgs& sa = step_args();  // re-read per step: see step_args()
    const KArgs& a = sa.a;
    const DevMap& m = a.m;
    const tc_buffers& b = a.b;
    const unsigned int flags = sa.flags;
    const size_t row0 = (size_t)k * a.N;
    const RollStep roll = roll_at(sa.ma.roll, row0, a.m.C);
    status = 0;
    trunc = 0;
    // this step's action (fetched a step ago), and the next step's on its way (the last step re-reads its own row)
    const double2 cur_d = act_d;
    const float2 cur_f = act_f;
    const int cur_m = act_m;
    fetch_action(k + 1 < nsteps ? k + 1 : k);
    TSTAMP(24);
    PathInfo pinfo;
    pinfo.ax = pinfo.ay = pinfo.bx = pinfo.by = pinfo.ori = 0;
    pinfo.valid = 0;
    bool fresh = false, track = false;
    int track_man = 0;
    double ctrl_steer = 0.0;  // CTRL: this step's command before noise (0 when no action is applied)
    if ((flags & TC_F_AUTORESET) && nr) {
      const int cur = cursor;
      int node;
      if ((flags & TC_F_DEVICE_SPAWN) && a.spawn_n > 0) {
        node = a.spawn_tab[tc_spawn_index(a.spawn_seed, (uint32_t)env, (uint32_t)cur, (uint32_t)a.spawn_n)];
      } else {
        if ((unsigned)cur >= (unsigned)b.spawn_queue_len) status |= TC_S_SPAWN_WRAPPED;
        node = b.spawn_queue[(size_t)env * b.spawn_queue_len + ((unsigned)cur % (unsigned)b.spawn_queue_len)];
      }
      if (PER) car_respawn<false>(sa.cr, env, live && sub == 0);  // (one lane of the group writes the row and counter)
      if (flags & TC_FI_CAM_BANK) g_cam_idx[grp] = cam_respawn<false>(sa.cb, env, live && sub == 0);
      if (CTRL && (flags & TC_FI_DRIVE_MAN)) g_drv_man[grp] = drive_respawn_man<false>(sa.dr, env, live && sub == 0, g_drv_man[grp]);
      if (CTRL && (flags & TC_FI_DRIVE_OU) && drive_ou_reset(sa.dr)) g_drv_ou[grp] = 0.0;
      d_reset(m, PER ? car_of<false>(a.car, sa.cr.rows + (size_t)env * TC_CAR_NP) : a.car, s, checked_spawn(m, node, status));
      fresh = true;
      have_trig = true;
      cursor = cur + 1;
    } else if ((unsigned)s.lp[0] >= (unsigned)m.lpN || (unsigned)s.lp[1] >= (unsigned)m.lpN) {
      status |= TC_S_NOT_RESET;
      trunc = 1;
    } else {
      double v, st;
      const double* crow = PER ? sa.cr.rows + (size_t)env * TC_CAR_NP : nullptr;
      if (CTRL) {  // cte / he still hold what the step before left (0 / 0 behind a re-spawn)
        ctrl_steer = ctrl_command(sa.ct, cte, he, PER ? car_ld<false>(crow, TC_CAR_MAX_STEERING_ANGLE) : a.car.max_steering_angle, v);
        st = sa.ct.noise ? ctrl_steer + cur_d.y : ctrl_steer;
        if (flags & TC_FI_DRIVE_OU) {  // (steer + row) + n
          const int draws = g_drv_draws[grp];
          const double n = drive_ou(sa.dr, env, g_drv_ou[grp], draws);
          st = st + n;
          g_drv_ou[grp] = n;
          g_drv_draws[grp] = (draws + 1) & 0x7fffffff;
        }
      } else if (sa.cdtype == TC_F32) {
        v = (double)cur_f.x;
        st = (double)cur_f.y;
      } else {
        v = cur_d.x;
        st = cur_d.y;
      }
      v = d_np_clip(v, -1.0, 1.0);  // env.py:118
      st = d_np_clip(PER ? st + car_ld<false>(crow, TC_CAR_STEERING_SHIFT) : st, -1.0, 1.0);  // (train_td3.py:146-148)
      const int man = CTRL && (flags & TC_FI_DRIVE_MAN) ? g_drv_man[grp] : cur_m;
      TSTAMP(25);
      d_car_kinematics(PER ? car_of<false>(a.car, crow) : a.car, s, v, st, have_trig);
      TSTAMP(26);
      have_trig = true;
      track = true;
      track_man = man;
    }
    // ---- this step's pose row, as early as the pose is final (nothing below moves the car): in a streamed call the frame
    // workgroups of this (step, env) are waiting for it, and what follows -- lanepath tracking, distances, reward, rollout
    // rows -- is most of the step
    const bool bank = (flags & TC_FI_CAM_BANK) != 0;
    const int cam_row = bank ? g_cam_idx[grp] : (live ? env : 0);  // camera row of this step's frame (see CamBank)
    if (bank && sa.cb.rows && live && sub == 0) sa.cb.rows[row0 + env] = cam_row;
    if (sa.ma.pose_rows) {
      // car.py:159-165 takes cos(-theta), sin(-theta): tc_cos is exactly even and tc_sin exactly odd, so the values of
      // the front-axle update are reused bit for bit (as in sim_body)
      FramePose fp;
      fp.x = s.x;
      fp.y = s.y;
      fp.cth = have_trig ? s.cth : tc_cos(-s.theta);
      fp.sth = have_trig ? -s.sth : tc_sin(-s.theta);
      double pose[12];
      cam_pose12(sa.a, cam_row, fp, pose);
      if (live && sub == 0) {
        if (sa.ma.resident) {
          // streamed call: the frame workgroup of this (step, env) may already be polling the row.  Each entry is one
          // 8-byte device-scope store (sc1: written through to where every XCD sees it) and validates itself -- the
          // reader waits until none of the twelve holds TC_POSE_EMPTY any more -- so the stores need no order among
          // themselves and this wavefront waits for none of them.
          unsigned long long* o = (unsigned long long*)(sa.ma.pose_rows + (row0 + env) * TC_POSE_ROW);
#pragma unroll
          for (int i = 0; i < 12; i++)
            __hip_atomic_store(o + i, (unsigned long long)__double_as_longlong(pose[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          // with a bank, a thirteenth entry of the same kind: the index this (step, env) was posed with (never all ones)
          if (bank) __hip_atomic_store(o + 12, (unsigned long long)(unsigned int)cam_row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          // and the whole-frame cull's verdict on this very pose (cam_cull_row; KArgs::cull_rows), evaluated behind the twelve
          // stores and stored last: the frame workgroup, which waits for it like for the others, then neither fetches the
          // table nor runs the predicate -- here it is one evaluation per (step, env), eight envs to the wavefront
          if (sa.a.cull_rows)
            __hip_atomic_store(o + TC_CULL_ROW_ENTRY, cam_cull_row(sa.a, pose), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          double2* o = (double2*)(sa.ma.pose_rows + (row0 + env) * TC_POSE_ROW);
#pragma unroll
          for (int i = 0; i < 6; i++) o[i] = make_double2(pose[2 * i], pose[2 * i + 1]);
          if (bank) ((long long*)o)[12] = cam_row;
          if (sa.a.cull_rows) ((unsigned long long*)o)[TC_CULL_ROW_ENTRY] = cam_cull_row(sa.a, pose);
        }
      }
    }
    if (track) {  // car.py:127-148 (the env went through the kinematic update above)
      if (fat_lds) {
        trunc = d_find_local_path<TC_EL>(m, fl, s, track_man, status, pinfo, sub);
      } else {
        const FatGlobal fg = {m.lp_fat, m.lp_nodes};
        trunc = d_find_local_path<TC_EL>(m, fg, s, track_man, status, pinfo, sub);
      }
    }
    TSTAMP(27);
    // ---- info (car.py:46-53), default reward / termination (env.py:93,99)
    const bool have_info = !fresh && s.lp_len >= 2;
    cte = 0;
    he = 0;
    if (have_info && !pinfo.valid) {  // path kept from an earlier step (truncated before it was rebuilt)
      double2 n1 = m.lp_nodes[s.lp[2]], n2 = m.lp_nodes[s.lp[3]];
      pinfo.ax = n1.x;
      pinfo.ay = n1.y;
      pinfo.bx = n2.x;
      pinfo.by = n2.y;
      pinfo.ori = d_lp_edge_ori(m, s.lp[2], s.lp[3]);
    }
    if (have_info) {
      cte = d_distance_to_edge(pinfo.ax, pinfo.ay, pinfo.bx, pinfo.by, s.front_x, s.front_y);
      he = d_clip_angle(pinfo.ori - s.theta);
    }
    reward = 0;
    terminated = 0;
    if (!(flags & TC_F_WRAPPED) && !fresh) {
      const double tw = PER ? car_ld<false>(sa.cr.rows + (size_t)env * TC_CAR_NP, TC_CAR_TRACK_WIDTH) : a.car.track_width;
      double r = (-1 / tw) * cte + 1;
      reward = (0 > r) ? 0 : r;
      terminated = cte > (tw * 10);
    }
    // ---- phase B: nearest lane-line edge and distance per layer (car.py:55-64, layer.py:33-44,126-164)
    const int C = m.C;
    // On demand: the phase carries nothing to the next step, and what it computes leaves the launch through the rollout's
    // rows, the terms below and -- of the last step -- the env's buffers.  The plan (CallPlan::info_every) says whether any
    // step but the last has a reader; without one those steps skip the phase, the grid lookup included.  roll.dist / roll.ne
    // are NULL then (they are what sets the bit), and gl.dist keeps the values of an earlier step or launch: no term of
    // the stack reads it (that would have set the bit too).  need_b is wave-uniform: a scalar branch round the phase.
    const bool last = k == nsteps - 1;
    const bool need_b = last || (flags & TC_FI_INFO_EVERY) != 0;
    TSTAMP(0);
    static_assert(TC_EL == 8 && TC_AG <= TC_EL, "group8_argmin_multi, one lane per layer of a block");
    if (need_b) {
      const int cell = have_info ? d_grid_cell(m, s.x, s.y) : -1;
      if (have_info) {
        // The cell's candidate edges (DevMap: every edge that can be the first minimum for a point of the cell, layer by
        // layer, ascending -- a handful per layer), a block of TC_AG layers at a time.  Memory first, arithmetic after: the
        // block's list offsets are fetched together, then each lane's first candidate of every layer together (two load
        // latencies for the whole block, whatever the vector-memory pipeline's queue looks like beside the frame kernel),
        // then the layers are scanned one after the other from the LDS edge records; lane g of the group finally evaluates
        // layer g's tail, so the bounds test and the distance run once per block, not once per layer.
        //   A car outside the grid (cell < 0) runs the SAME code with the identity list -- every edge of the layer -- so a
        // wavefront with one such env executes longer loops, not a second copy of the phase.
        const bool far = cell < 0;
        for (int lb = 0; lb < C; lb += TC_AG) {
          double bd[TC_AG];
          int best[TC_AG], lo[TC_AG], off[TC_AG + 1], e0[TC_AG];
#pragma unroll
          for (int g = 0; g <= TC_AG; g++) {
            const int lg = lb + g < C ? lb + g : C;
            off[g] = far ? m.edge_off[lg] : m.cand_off[cell * C + lg];
          }
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            lo[g] = lb + g < C ? m.edge_off[lb + g] : 0;
            e0[g] = off[g] + sub < off[g + 1] ? (far ? off[g] + sub : m.cand_idx[off[g] + sub]) : -1;
          }
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            double bdg = 0;
            int bg = -1, e = e0[g];
            for (int i = off[g] + sub; i < off[g + 1]; i += TC_EL) {
              double4 q;
              if (map_lds)
                q = make_double4(l_exy[4 * e], l_exy[4 * e + 1], l_exy[4 * e + 2], l_exy[4 * e + 3]);
              else
                q = m.edge_xy[e];
              const double d = tc_fabs(d_dist(s.x, s.y, q.x, q.y) + d_dist(s.x, s.y, q.z, q.w));
              if (bg < 0 || d < bdg) {
                bg = e - lo[g];
                bdg = d;
              }
              if (i + TC_EL < off[g + 1]) e = far ? i + TC_EL : m.cand_idx[i + TC_EL];
            }
            bd[g] = bdg;
            best[g] = bg;
          }
          if (lb == 0) TSTAMP(16);
          group8_argmin_multi(bd, best);
          if (lb == 0) TSTAMP(1);
          int ne = -1, eo = 0;
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            ne = sub == g ? best[g] : ne;
            eo = sub == g ? lo[g] : eo;
          }
          const int l = lb + sub;
          if (sub < TC_AG && l < C) {  // lane g: layer lb + g
            double dist_l = 0;
            if (ne >= 0) {
              const int ge = eo + ne;
              double4 q;
              double o_fw, o_rv;
              if (map_lds) {
                q = make_double4(l_exy[4 * ge], l_exy[4 * ge + 1], l_exy[4 * ge + 2], l_exy[4 * ge + 3]);
                o_fw = l_ofw[ge];
                o_rv = l_orv[ge];
              } else {
                q = m.edge_xy[ge];
                o_fw = m.ori_fwd[ge];
                o_rv = m.ori_rev[ge];
              }
              const double2 n0 = make_double2(q.x, q.y), n1 = make_double2(q.z, q.w);
              bool certain;
              bool inb = d_within_bounds_filter(n0.x, n0.y, n1.x, n1.y, s.x, s.y, certain);
              if (!certain) inb = d_within_bounds(n0.x, n0.y, n1.x, n1.y, o_fw, o_rv, s.x, s.y);
              if (inb) {
                dist_l = tc_fabs(d_distance_to_edge(n0.x, n0.y, n1.x, n1.y, s.x, s.y));
              } else {
                const double da = d_dist(s.x, s.y, n0.x, n0.y);
                const double db = d_dist(s.front_x, s.front_y, n1.x, n1.y);  // FRONT axle for n1 (car.py:64)
                dist_l = db < da ? db : da;
              }
            }
            gl.dist[l] = dist_l;
            if (live) {
              if (roll.dist) roll.dist[(roll.row0 + env) * C + l] = dist_l;
              if (roll.ne) roll.ne[(roll.row0 + env) * C + l] = ne;
            }
            if (last && live) {
              b.laneline_distances[(size_t)env * C + l] = dist_l;
              b.nearest_edge[(size_t)env * C + l] = ne;
            }
          }
          if (lb == 0) TSTAMP(2);
        }
      } else {
        for (int l = sub; l < C; l += TC_EL) {  // no info this step (car.py:47-51): zero distances, no nearest edge
          gl.dist[l] = 0;
          if (live) {
            if (roll.dist) roll.dist[(roll.row0 + env) * C + l] = 0;
            if (roll.ne) roll.ne[(roll.row0 + env) * C + l] = -1;
          }
          if (last && live) {
            b.laneline_distances[(size_t)env * C + l] = 0;
            b.nearest_edge[(size_t)env * C + l] = -1;
          }
        }
      }
    }
    TSTAMP(14);
    // ---- reward / termination wrappers (a re-spawned env did not go through Wrapper.step)
    if (a.n_terms > 0 && !fresh)
      d_apply_terms_mem(a.terms, a.n_terms, gl.cnt,
                        PER ? car_ld<false>(sa.cr.rows + (size_t)env * TC_CAR_NP, TC_CAR_TRACK_WIDTH) : a.car.track_width, C,
                        cte, have_info ? s.velocity : 0.0, gl.dist, reward, terminated);
    int ep_len = 0;
    if (EP) {
      ep_len = g_ep_len[grp];
      ep_count<false>(sa.ep, env, fresh, ep_len, trunc, status);
      g_ep_len[grp] = ep_len;
    }
    nr = (flags & TC_F_AUTORESET) ? (terminated || trunc) : 0;
    // ---- this step's rollout rows and pose row
    if (live && sub == 0) {
      if (EP) ep_close(sa.ep, env, row0 + env, fresh, status, ep_len, g_ep_ret[grp], reward, terminated | trunc);
      if (CTRL) {
        ctrl_store(sa.ct, env, row0 + env, ctrl_steer);
        drive_store(sa.dr, row0 + env, (flags & TC_FI_DRIVE_MAN) ? g_drv_man[grp] : cur_m,
                    track && (flags & TC_FI_DRIVE_OU) ? g_drv_ou[grp] : 0.0);
      }
      if (roll.cte) roll.cte[roll.row0 + env] = cte;
      if (roll.heading_error) roll.heading_error[roll.row0 + env] = he;
      if (roll.truncated) roll.truncated[roll.row0 + env] = (unsigned char)trunc;
      if (roll.reward) roll.reward[roll.row0 + env] = reward;
      if (roll.terminated) roll.terminated[roll.row0 + env] = (unsigned char)terminated;
      if (roll.status) roll.status[roll.row0 + env] = status;
      if (roll.x) roll.x[roll.row0 + env] = s.x;
      if (roll.y) roll.y[roll.row0 + env] = s.y;
      if (roll.theta) roll.theta[roll.row0 + env] = s.theta;
      if (roll.velocity) roll.velocity[roll.row0 + env] = s.velocity;
      if (roll.lp_len) roll.lp_len[roll.row0 + env] = s.lp_len;
      if (roll.lp) {
        int4* o = (int4*)(roll.lp + (roll.row0 + env) * 8);
        o[0] = make_int4(s.lp[0], s.lp[1], s.lp[2], s.lp[3]);
        o[1] = make_int4(s.lp[4], s.lp[5], s.lp[6], s.lp[7]);
      }
    }
    TSTAMP(15);
  }
  // ---- state and the last step's outputs back to the caller's buffers
  const StepArgs& s1 = step_args();
  const tc_buffers& b = s1.a.b;
  if (live && sub == 0) {
    b.x[env] = s.x;
    b.y[env] = s.y;
    b.theta[env] = s.theta;
    b.velocity[env] = s.velocity;
    b.steering[env] = s.steering;
    b.radius[env] = s.radius;
    b.front_x[env] = s.front_x;
    b.front_y[env] = s.front_y;
#pragma unroll
    for (int i = 0; i < 8; i++) b.local_path[env * 8 + i] = s.lp[i];
    b.lp_len[env] = s.lp_len;
    b.last_maneuver[env] = s.last_maneuver;
    b.cte[env] = cte;
    b.heading_error[env] = he;
    b.reward[env] = reward;
    b.terminated[env] = (unsigned char)terminated;
    b.truncated[env] = (unsigned char)trunc;
    b.status[env] = status;
    if (b.needs_reset) b.needs_reset[env] = (unsigned char)nr;
    if (cursor != cursor0) b.spawn_cursor[env] = cursor;
    if (EP) {
      s1.ep.length[env] = g_ep_len[grp];
      s1.ep.ret[env] = g_ep_ret[grp];
    }
    if (CTRL && (s1.flags & TC_FI_DRIVE_MAN)) s1.dr.maneuver[env] = g_drv_man[grp];
    if (CTRL && (s1.flags & TC_FI_DRIVE_OU)) {
      s1.dr.ou_state[env] = g_drv_ou[grp];
      s1.dr.ou_draws[env] = g_drv_draws[grp];
    }
  }
  if (live && s1.a.term_counters && sub < s1.a.n_terms) s1.a.term_counters[(size_t)env * TC_MAX_TERMS + sub] = gl.cnt[sub];
}
// (Launch bounds: with the episode accounting 4 wavefronts per SIMD are asked for -- left to itself the allocator takes
// 129 / 131 VGPRs there, whatever the episode state is kept in; held to the 128 of the other variants it spills nothing.
// 0 = nothing asked for, as for the variants without it.)
template <unsigned FEAT>
__global__ __launch_bounds__(TC_ENVG_NT, ((FEAT & TC_FEAT_EP) ? 4 : 0)) void tc_envg_kernel(StepArgs sa_unused) {
  envg_kernel_body<FEAT>();
}
// the same body with the built-in controller compiled in (FEAT has TC_FEAT_CTRL: masks 4-7).  4 wavefronts per SIMD are
// asked for in every mask: with the drive randomisation's normal (tc_log, sqrt, tc_cos beside the whole car state in
// registers) the allocator left to itself takes 128 / 130 VGPRs in masks 4 / 5; held to 128 it spills nothing.
template <unsigned FEAT>
__global__ __launch_bounds__(TC_ENVG_NT, 4) void tc_drive_envg_kernel(StepArgs sa_unused) {
  static_assert((FEAT & TC_FEAT_CTRL) != 0, "the controller's entry point");
  envg_kernel_body<FEAT>();
}

#endif  // K_ENVG_H
