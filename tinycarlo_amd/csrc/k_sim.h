// k_sim.h -- the simulate stage of one env by one 64-lane wavefront:
//   phase A  kinematics + lanepath tracking + CTE / heading              (car.py:70-148, 46-53)
//   phase B  nearest lane-line edge per layer + distance                 (layer.py:33-44, car.py:55-64)
// sim_body<K, FEAT> is one step: it reads and rewrites the env's LiveLds record (k_common.h) and leaves the frame's
// FramePose; live_in / live_out, ep_in / ep_out, ctrl_in and cam_in move that record between the caller's buffers and LDS
// around a launch's steps; checked_spawn guards a re-spawn node.  The features of k_feat.h are compiled in by the FEAT
// mask.  Defines no kernel: tc_env_kernel (k_env.h) and tc_step_kernel (k_frame.h) run it; the grouped kernel (k_envg.h)
// restates the two phases for 8 lanes per env.  Includes k_feat.h, and k_camera.h for MapCache and FramePose only, which
// sim_body takes by reference.
#ifndef K_SIM_H
#define K_SIM_H

#include "k_camera.h"
#include "k_feat.h"
#include "tc_device.h"
#include "tc_rng.h"

// A spawn node must exist and have an out-edge (map.py:62-64 re-draws otherwise; the host RNG mirror
// does that).  Anything else would index out of bounds, so it is replaced and flagged.
__device__ inline int checked_spawn(const DevMap& m, int node, int& status) {
  if ((unsigned)node < (unsigned)m.lpN && m.lp_fat[node].nnext > 0) return node;
  status |= TC_S_BAD_SPAWN;
  return m.first_spawnable;
}

// Caller's buffers -> LiveLds, one item per lane (one vector-memory round trip for the ~30 scalars of an env).
__device__ __forceinline__ void live_in(const KArgs& a, unsigned char* smem, int env, int mode, unsigned int flags,
                                        const int tid = threadIdx.x) {
  const tc_buffers& b = a.b;
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid < 8) {
    const double* p = b.x;
    p = tid == 1 ? b.y : p;
    p = tid == 2 ? b.theta : p;
    p = tid == 3 ? b.velocity : p;
    p = tid == 4 ? b.steering : p;
    p = tid == 5 ? b.radius : p;
    p = tid == 6 ? b.front_x : p;
    p = tid == 7 ? b.front_y : p;
    lv->d[tid] = p[env];
  } else if (tid < 16) {
    lv->lp[tid - 8] = b.local_path[env * 8 + (tid - 8)];
  } else if (tid == 16) {
    lv->lp_len = b.lp_len[env];
  } else if (tid == 17) {
    lv->last_maneuver = b.last_maneuver[env];
  } else if (tid == 18) {
    lv->needs_reset = (mode == MODE_STEP && (flags & TC_F_AUTORESET)) ? b.needs_reset[env] : 0;
  } else if (tid == 19) {
    const int c = (mode == MODE_STEP && (flags & TC_F_AUTORESET)) ? b.spawn_cursor[env] : 0;
    lv->cursor = c;
    lv->cursor0 = c;
  } else if (tid < 28) {
    const int t = tid - 20;
    lv->cnt[t] = (a.n_terms > 0 && a.term_counters) ? a.term_counters[(size_t)env * TC_MAX_TERMS + t] : 0;
  } else if (tid == 28) {
    lv->d[8] = 0;
    lv->d[9] = 0;
    lv->have_trig = 0;
  }
  lds_sync();
}

// LiveLds -> caller's buffers after the last step of the launch (not for MODE_RENDER, which changes nothing).
__device__ __forceinline__ void live_out(const KArgs& a, unsigned char* smem, int env, const int tid = threadIdx.x) {
  const tc_buffers& b = a.b;
  const LiveLds* lv = (const LiveLds*)(smem + a.lds.off_live);
  const int C = a.m.C;
  lds_sync();
  if (tid < 8) {
    double* p = b.x;
    p = tid == 1 ? b.y : p;
    p = tid == 2 ? b.theta : p;
    p = tid == 3 ? b.velocity : p;
    p = tid == 4 ? b.steering : p;
    p = tid == 5 ? b.radius : p;
    p = tid == 6 ? b.front_x : p;
    p = tid == 7 ? b.front_y : p;
    p[env] = lv->d[tid];
  } else if (tid < 16) {
    b.local_path[env * 8 + (tid - 8)] = lv->lp[tid - 8];
  } else if (tid == 16) {
    b.lp_len[env] = lv->lp_len;
  } else if (tid == 17) {
    b.last_maneuver[env] = lv->last_maneuver;
  } else if (tid == 18) {
    if (b.needs_reset) b.needs_reset[env] = (unsigned char)lv->needs_reset;
  } else if (tid == 19) {
    if (lv->cursor != lv->cursor0) b.spawn_cursor[env] = lv->cursor;
  } else if (tid < 28) {
    const int t = tid - 20;
    if (a.term_counters && t < a.n_terms) a.term_counters[(size_t)env * TC_MAX_TERMS + t] = lv->cnt[t];
  } else if (tid == 28) {
    b.cte[env] = lv->cte;
  } else if (tid == 29) {
    b.heading_error[env] = lv->he;
  } else if (tid == 30) {
    b.reward[env] = lv->reward;
  } else if (tid == 31) {
    b.terminated[env] = (unsigned char)lv->terminated;
  } else if (tid == 32) {
    b.truncated[env] = (unsigned char)lv->trunc;
  } else if (tid == 33) {
    b.status[env] = lv->status;
  } else if (tid < 34 + TC_MAX_LAYERS - 4) {  // lanes 34..45: layers 0..11
    const int l = tid - 34;
    if (l < C) {
      b.laneline_distances[(size_t)env * C + l] = lv->dist[l];
      b.nearest_edge[(size_t)env * C + l] = lv->ne[l];
    }
  } else if (tid < 50) {  // lanes 46..49: layers 12..15
    const int l = tid - 34;
    if (l < C) {
      b.laneline_distances[(size_t)env * C + l] = lv->dist[l];
      b.nearest_edge[(size_t)env * C + l] = lv->ne[l];
    }
  }
}

// The running episode of an env: caller's buffers -> LiveLds before live_in (whose barrier covers it), and back after
// live_out, by one lane that live_in / live_out leave idle.
__device__ __forceinline__ void ep_in(const KArgs& a, const EpArgs& ep, unsigned char* smem, int env, const int tid = threadIdx.x) {
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid == 50) {
    lv->ep_len = ep.length[env];
    lv->ep_ret = ep.ret[env];
  }
}
// What the env reported after the step before this launch: caller's buffers -> LiveLds, likewise before live_in (the
// TC_FEAT_CTRL kernels only: no other kernel reads the two before it has written them).
__device__ __forceinline__ void ctrl_in(const KArgs& a, unsigned char* smem, int env, const int tid = threadIdx.x) {
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid == 51) lv->cte = a.b.cte[env];
  if (tid == 52) lv->he = a.b.heading_error[env];
}
// The env's camera of the bank: caller's buffer -> LiveLds, likewise before live_in (only while a bank is installed).
__device__ __forceinline__ void cam_in(const KArgs& a, const CamBank& cb, unsigned char* smem, int env, const int tid = threadIdx.x) {
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  if (tid == 53) lv->cam_idx = cam_clamp(cb, cb.index[env]);
}
__device__ __forceinline__ void ep_out(const KArgs& a, const EpArgs& ep, unsigned char* smem, int env, const int tid = threadIdx.x) {
  const LiveLds* lv = (const LiveLds*)(smem + a.lds.off_live);
  if (tid == 50) {
    ep.length[env] = lv->ep_len;
    ep.ret[env] = lv->ep_ret;
  }
}

// Stage 1 (simulate) for one env by one wavefront.  Returns false when nothing is to be rasterised for this env.
// always inlined: out of line, `a` would be a pointer into private memory and the whole kernel-argument struct
// (~1 KB) would be copied to scratch by every lane (the inliner's cost threshold is close: measured 47.9 k vs 47.6 k)
// One step of one env: reads and rewrites the env's LiveLds record; the caller's buffers are only touched by live_in /
// live_out (and the per-step rollout rows of `roll`).
// PER: the env's car constants come from its row of cr.rows (per-env cars, tc_env_set_car_per_env), else a.car.
// EP: episode length / return / time limit (tc_env_set_episodes); the running pair lives in LiveLds (ep_len, ep_ret).
// CTRL: the action comes from the built-in controller (tc_env_set_controller), computed from the cte / he the record holds
// from the step before; car_control is not read.
// need_b (wave-uniform): this step computes the lane-line distances -- the launch's last step, and every step when the
// call's plan says someone reads them (TC_FI_INFO_EVERY).  need_win: the map window is fetched into `mc` behind phase A: for
// phase B, and for the camera stage where the same wavefront runs one behind this step.
template <int K, unsigned FEAT = 0>
__device__ __forceinline__ void sim_body(const KArgs& a, unsigned char* smem, int env, int mode,
                                const void* car_control, int cdtype,
                                const int* maneuver, const int* spawn_nodes, const unsigned char* mask,
                                unsigned int flags, const RollStep& roll, const int tid, MapCache<K>& mc, FramePose& fp,
                                int& cam_row, const bool need_b, const bool need_win, const CarRows& cr = CarRows(),
                                const EpArgs& ep = EpArgs(),
                                const CtrlArgs& ct = CtrlArgs(), const CamBank& cb = CamBank(),
                                const DriveArgs& dr = DriveArgs()) {
  constexpr bool PER = (FEAT & TC_FEAT_CAR) != 0, EP = (FEAT & TC_FEAT_EP) != 0, CTRL = (FEAT & TC_FEAT_CTRL) != 0;

  TSTAMP(0);
  TSTAMP_REAL(30);
  const DevMap& m = a.m;
  const tc_buffers& b = a.b;
  // map windows of 64*K nodes / edges; one window (the usual case) is fetched now and kept in registers
  const int nwin_n = (m.total_nodes + TC_NT * K - 1) / (TC_NT * K), nwin_e = (m.total_edges + TC_NT * K - 1) / (TC_NT * K);
  const bool single = a.n_grp == 1 && !a.cam_nodes && a.grp_layer[0] == 0 && a.grp_layer[1] == m.C && nwin_n <= 1 && nwin_e <= 1;
  double* dn = (double*)(smem + a.lds.off_p);  // phase B: one double per lane-line node (aliases the camera's node buffer)

  // ---- state: all lanes read the same LDS words (broadcast)
  LiveLds* lv = (LiveLds*)(smem + a.lds.off_live);
  // (readfirstlane: the values are wave-uniform, and the compiler has to KNOW it -- read straight from LDS they count
  // as divergent, every branch of the scalar phases below becomes an exec-mask region and the kernel triples in size)
  CarState s;
  s.x = uni_d(lv->d[0]);
  s.y = uni_d(lv->d[1]);
  s.theta = uni_d(lv->d[2]);
  s.velocity = uni_d(lv->d[3]);
  s.steering = uni_d(lv->d[4]);
  s.radius = uni_d(lv->d[5]);
  s.front_x = uni_d(lv->d[6]);
  s.front_y = uni_d(lv->d[7]);
  s.cth = uni_d(lv->d[8]);
  s.sth = uni_d(lv->d[9]);
#pragma unroll
  for (int i = 0; i < 8; i++) s.lp[i] = uni_i(lv->lp[i]);
  s.lp_len = uni_i(lv->lp_len);
  s.last_maneuver = uni_i(lv->last_maneuver);
  bool have_trig = uni_i(lv->have_trig) != 0;  // s.cth / s.sth hold cos / sin of the current heading
  const int nr = uni_i(lv->needs_reset);
  int cursor = uni_i(lv->cursor);
  int my_cnt = tid < TC_MAX_TERMS ? lv->cnt[tid] : 0;  // lane t: steps_true of term slot t
  int ep_len = EP ? uni_i(lv->ep_len) : 0;
  // which camera row this step's frame uses: the env's own (shared camera: unused), or its index into the bank
  const bool bank = (flags & TC_FI_CAM_BANK) != 0;
  cam_row = bank ? uni_i(lv->cam_idx) : env;

  int status = 0, trunc = 0;
  PathInfo pinfo;
  pinfo.ax = pinfo.ay = pinfo.bx = pinfo.by = pinfo.ori = 0;
  pinfo.valid = 0;
  bool fresh = false;  // env was (re)spawned in this launch: info is empty (car.py:47-51)
  const double* crow = PER ? cr.rows + (size_t)env * TC_CAR_NP : nullptr;
  double ctrl_steer = 0.0;  // CTRL: this step's command before noise (0 when no action is applied)
  // CTRL, drive randomisation: the maneuver in force and the OU value applied (0 when no action is applied), for the rows
  const bool drv_man = CTRL && (flags & TC_FI_DRIVE_MAN) != 0, drv_ou = CTRL && (flags & TC_FI_DRIVE_OU) != 0;
  int drive_m = 0;
  double drive_n = 0.0;
  // a re-spawn: the next episode's maneuver, and the OU value back to 0 when asked for (lane 0 stores; see DriveArgs)
  auto drive_respawn = [&]() {
    if (drv_man) {
      drive_m = drive_respawn_man<true>(dr, env, tid == 0, uni_i(dr.maneuver[env]));
      if (tid == 0) dr.maneuver[env] = drive_m;
    }
    if (drv_ou && drive_ou_reset(dr) && tid == 0) dr.ou_state[env] = 0.0;
  };
  if (mode == MODE_RESET) {
    if (PER) car_respawn<true>(cr, env, true);
    if (bank) cam_row = cam_respawn<true>(cb, env, tid == 0);
    if (CTRL) drive_respawn();
    d_reset(m, PER ? car_of<true>(a.car, crow) : a.car, s, checked_spawn(m, spawn_nodes[env], status));
    fresh = true;
    have_trig = true;
  } else if (mode == MODE_STEP) {
    if ((flags & TC_F_AUTORESET) && nr) {
      const int cur = cursor;
      int node;
      if ((flags & TC_F_DEVICE_SPAWN) && a.spawn_n > 0) {
        node = a.spawn_tab[tc_spawn_index(a.spawn_seed, (uint32_t)env, (uint32_t)cur, (uint32_t)a.spawn_n)];
      } else {
        if ((unsigned)cur >= (unsigned)b.spawn_queue_len) status |= TC_S_SPAWN_WRAPPED;  // replaying the queue
        node = b.spawn_queue[(size_t)env * b.spawn_queue_len + ((unsigned)cur % (unsigned)b.spawn_queue_len)];
      }
      if (PER) car_respawn<true>(cr, env, true);
      if (bank) cam_row = cam_respawn<true>(cb, env, tid == 0);
      if (CTRL) {
        drive_respawn();
        if (!drv_man && dr.man_rows) drive_m = maneuver[env];
      }
      d_reset(m, PER ? car_of<true>(a.car, crow) : a.car, s, checked_spawn(m, node, status));
      fresh = true;
      have_trig = true;
      cursor = cur + 1;
    } else if ((unsigned)s.lp[0] >= (unsigned)m.lpN || (unsigned)s.lp[1] >= (unsigned)m.lpN) {
      status |= TC_S_NOT_RESET;  // stepping an env that was never reset: no valid lanepath edge to index with
      trunc = 1;
      if (CTRL && dr.man_rows) drive_m = drv_man ? uni_i(dr.maneuver[env]) : maneuver[env];
    } else {
      double v, st;
      if (CTRL) {  // (every input is wave-uniform; double arithmetic has no scalar form, so the lanes all compute it)
        ctrl_steer = ctrl_command(ct, uni_d(lv->cte), uni_d(lv->he),
                                  PER ? car_ld<true>(crow, TC_CAR_MAX_STEERING_ANGLE) : a.car.max_steering_angle, v);
        st = ct.noise ? ctrl_steer + uni_d(ct.noise[roll.row0 + env]) : ctrl_steer;
        if (drv_ou) {  // (steer + row) + n
          const int draws = uni_i(dr.ou_draws[env]);
          drive_n = drive_ou(dr, env, uni_d(dr.ou_state[env]), draws);
          st = st + drive_n;
          if (tid == 0) {
            dr.ou_state[env] = drive_n;
            dr.ou_draws[env] = (draws + 1) & 0x7fffffff;
          }
        }
      } else if (cdtype == TC_F32) {
        v = (double)((const float*)car_control)[2 * env];
        st = (double)((const float*)car_control)[2 * env + 1];
      } else {
        v = ((const double*)car_control)[2 * env];
        st = ((const double*)car_control)[2 * env + 1];
      }
      v = d_np_clip(v, -1.0, 1.0);  // env.py:118
      // per-env steering shift: added before the clip (examples/train_td3.py:146-148)
      st = d_np_clip(PER ? st + car_ld<true>(crow, TC_CAR_STEERING_SHIFT) : st, -1.0, 1.0);
      const int man = drv_man ? uni_i(dr.maneuver[env]) : maneuver[env];
      if (CTRL) drive_m = man;
      d_car_kinematics(PER ? car_of<true>(a.car, crow) : a.car, s, v, st, have_trig);
      TSTAMP(23);
      const FatGlobal fg = {m.lp_fat, m.lp_nodes};
      trunc = d_find_local_path(m, fg, s, man, status, pinfo, tid);
      have_trig = true;
    }
  }

  TSTAMP(1);
  if (mode != MODE_RENDER) {
    // ---- write the state back + scalar info (lane 0)
    const bool have_info = !fresh && s.lp_len >= 2;
    double cte = 0, he = 0;
    if (have_info && !pinfo.valid) {  // path kept from an earlier step (truncated before it was rebuilt)
      double2 n1 = m.lp_nodes[s.lp[2]], n2 = m.lp_nodes[s.lp[3]];
      pinfo.ax = n1.x;
      pinfo.ay = n1.y;
      pinfo.bx = n2.x;
      pinfo.by = n2.y;
      pinfo.ori = d_lp_edge_ori(m, s.lp[2], s.lp[3]);
    }
    if (have_info) {  // car.py:52-53 (nodes and orientation of local_path[1] were captured while tracking)
      cte = d_distance_to_edge(pinfo.ax, pinfo.ay, pinfo.bx, pinfo.by, s.front_x, s.front_y);
      he = d_clip_angle(pinfo.ori - s.theta);
    }
    double reward = 0;
    int terminated = 0;
    if (!(flags & TC_F_WRAPPED) && !fresh) {  // env.py:93,99
      const double tw = PER ? car_ld<true>(crow, TC_CAR_TRACK_WIDTH) : a.car.track_width;
      double r = (-1 / tw) * cte + 1;
      reward = (0 > r) ? 0 : r;
      terminated = cte > (tw * 10);
    }
    const bool late = a.n_terms > 0;  // reward / terminated depend on phase B: written after it
    if (EP) ep_count<true>(ep, env, fresh, ep_len, trunc, status);  // (the time limit: before trunc / status are stored)
    if (tid == 0) {
      lv->d[0] = s.x;
      lv->d[1] = s.y;
      lv->d[2] = s.theta;
      lv->d[3] = s.velocity;
      lv->d[4] = s.steering;
      lv->d[5] = s.radius;
      lv->d[6] = s.front_x;
      lv->d[7] = s.front_y;
      lv->d[8] = s.cth;
      lv->d[9] = s.sth;
      lv->lp_len = s.lp_len;
      lv->last_maneuver = s.last_maneuver;
      lv->have_trig = have_trig ? 1 : 0;
      lv->cursor = cursor;
      lv->cte = cte;
      lv->he = he;
      lv->trunc = trunc;
      lv->status = status;
      if (roll.cte) roll.cte[roll.row0 + env] = cte;
      if (roll.heading_error) roll.heading_error[roll.row0 + env] = he;
      if (roll.truncated) roll.truncated[roll.row0 + env] = (unsigned char)trunc;
      if (roll.status) roll.status[roll.row0 + env] = status;
      if (roll.x) roll.x[roll.row0 + env] = s.x;
      if (roll.y) roll.y[roll.row0 + env] = s.y;
      if (roll.theta) roll.theta[roll.row0 + env] = s.theta;
      if (roll.velocity) roll.velocity[roll.row0 + env] = s.velocity;
      if (roll.lp_len) roll.lp_len[roll.row0 + env] = s.lp_len;
      if (CTRL && mode == MODE_STEP) {
        ctrl_store(ct, env, roll.row0 + env, ctrl_steer);
        drive_store(dr, roll.row0 + env, drive_m, drive_n);
      }
      if (EP) lv->ep_len = ep_len;
      if (bank) {
        if (fresh) lv->cam_idx = cam_row;
        if (cb.rows && mode == MODE_STEP) cb.rows[roll.row0 + env] = cam_row;
      }
      if (!late) {
        lv->reward = reward;
        lv->terminated = terminated;
        lv->needs_reset = (flags & TC_F_AUTORESET) ? (terminated || trunc) : 0;
        if (roll.reward) roll.reward[roll.row0 + env] = reward;
        if (roll.terminated) roll.terminated[roll.row0 + env] = (unsigned char)terminated;
        if (EP) ep_close(ep, env, roll.row0 + env, fresh, status, ep_len, lv->ep_ret, reward, terminated | trunc);
      }
    }
    if (tid < 8) {  // register-resident select (a runtime-indexed s.lp[tid] would live in scratch)
      int v = s.lp[0];
#pragma unroll
      for (int i = 1; i < 8; i++) v = tid == i ? s.lp[i] : v;
      lv->lp[tid] = v;
      if (roll.lp) roll.lp[(roll.row0 + env) * 8 + tid] = v;
    }

    TSTAMP(2);
    // The map window is fetched here, behind phase A, and not at the top of the step: across the scalar phase its 30
    // registers per lane were what pushed the fused kernel over 128 VGPRs (the allocator answered by spilling the node
    // half to scratch and reloading it here).  The lines are L1 / L2 resident after the first step of a launch.
    if (single && need_win) {  // (the camera stage behind this one finds the window loaded)
      cache_nodes(mc, m, 0, m.total_nodes, tid);
      cache_edges(mc, m, 0, m.total_edges, 0, tid);
    }
    // ---- phase B: lane-line distances (car.py:55-64)
    const int C = m.C;
    double dist_l = 0;  // lane l < C: distance to lane-line layer l (0 while the info is empty, car.py:47-51)
    // Without need_b neither branch runs: nobody reads this step's distances (see envg_kernel_body) -- no rollout rows for
    // them, no term that looks at dist_l -- and lv->dist / lv->ne keep an earlier step's values until the launch's last
    // step, which always comes through here, rewrites them for live_out.  (The condition sits in the two branches, not in
    // a third one in front of them: that form moved the fused kernels' VGPR counts, which the tests hold to the recorded ones.)
    if (need_b && have_info && !DBG_ON(flags, DBG_SKIP_DIST)) {
      int my_e = -1;
      const int cell = uni_i(d_grid_cell(m, s.x, s.y));  // (every lane holds the same state)
      if (cell >= 0) {
        // layer.py:43 over the cell's candidate edges (DevMap: every edge that can be the first minimum for a point of
        // the cell, all layers, ascending): one lane per candidate, two distances straight from the edge record
        const int o0 = m.cand_off[cell * C], o1 = m.cand_off[cell * C + C];
        TSTAMP(14);
        for (int l0 = 0; l0 < C; l0 += TC_AG) {
          double bd[TC_AG];
          int best[TC_AG], lo[TC_AG], hi[TC_AG];
#pragma unroll
          for (int g = 0; g < TC_AG; g++) {
            bd[g] = 0;
            best[g] = -1;
            lo[g] = l0 + g < C ? m.edge_off[l0 + g] : 0x7fffffff;
            hi[g] = l0 + g < C ? m.edge_off[l0 + g + 1] : 0x7fffffff;
          }
          const int e_lo = m.edge_off[l0], e_hi = m.edge_off[l0 + TC_AG < C ? l0 + TC_AG : C];
          for (int i = o0 + tid; i < o1; i += TC_NT) {
            const int e = m.cand_idx[i];
            if (e >= e_lo && e < e_hi) {
              const double4 q = m.edge_xy[e];
              const double d = tc_fabs(d_dist(s.x, s.y, q.x, q.y) + d_dist(s.x, s.y, q.z, q.w));
#pragma unroll
              for (int g = 0; g < TC_AG; g++) {
                const bool take = e >= lo[g] && e < hi[g] && (best[g] < 0 || d < bd[g]);
                bd[g] = take ? d : bd[g];
                best[g] = take ? e - lo[g] : best[g];
              }
            }
          }
          wave_argmin_group(bd, best);
#pragma unroll
          for (int g = 0; g < TC_AG; g++)
            if (tid == l0 + g) my_e = best[g];
        }
      } else {
      for (int w = 0; w < nwin_n; w++) {
        if (!single) cache_nodes(mc, m, w * K * TC_NT, m.total_nodes, tid);
#pragma unroll
        for (int k = 0; k < K; k++) {
          const int i = (w * K + k) * TC_NT + tid;
          if (i < m.total_nodes) dn[i] = d_dist(s.x, s.y, mc.nd[k].x, mc.nd[k].y);
        }
      }
      lds_sync();
      TSTAMP(14);
      // layer.py:43 for every layer: each lane scans its edges once (ascending index) and keeps one partial per layer
      // of the current group of TC_AG layers; the group's reductions then run together (wave_argmin_group).  A layer's
      // edges are contiguous, so edge e belongs to group layer g iff edge_off[l0 + g] <= e < edge_off[l0 + g + 1].
      for (int l0 = 0; l0 < C; l0 += TC_AG) {
        double bd[TC_AG];
        int best[TC_AG], lo[TC_AG], hi[TC_AG];
#pragma unroll
        for (int g = 0; g < TC_AG; g++) {
          bd[g] = 0;
          best[g] = -1;
          lo[g] = l0 + g < C ? m.edge_off[l0 + g] : 0x7fffffff;
          hi[g] = l0 + g < C ? m.edge_off[l0 + g + 1] : 0x7fffffff;
        }
        const int e_lo = m.edge_off[l0], e_hi = m.edge_off[l0 + TC_AG < C ? l0 + TC_AG : C];
        for (int w = 0; w < nwin_e; w++) {
          const int w0 = w * K * TC_NT;
          if (w0 >= e_hi || w0 + K * TC_NT <= e_lo) continue;  // no edge of this layer group in the window
          if (!single) cache_edges(mc, m, w0, m.total_edges, 0, tid);
#pragma unroll
          for (int k = 0; k < K; k++) {
            const int e = (w * K + k) * TC_NT + tid;
            if (e >= e_lo && e < e_hi) {
              const double d = tc_fabs(dn[mc.ed[k].x] + dn[mc.ed[k].y]);
#pragma unroll
              for (int g = 0; g < TC_AG; g++) {
                const bool take = e >= lo[g] && e < hi[g] && (best[g] < 0 || d < bd[g]);
                bd[g] = take ? d : bd[g];
                best[g] = take ? e - lo[g] : best[g];
              }
            }
          }
        }
        wave_argmin_group(bd, best);
#pragma unroll
        for (int g = 0; g < TC_AG; g++)
          if (tid == l0 + g) my_e = best[g];
      }
      }
      TSTAMP(15);
      if (tid < C) {
        const int l = tid;
        if (my_e >= 0) {
          const int ge = m.edge_off[l] + my_e;
          int2 ed = m.edges_g[ge];
          double2 n0 = m.nodes[ed.x], n1 = m.nodes[ed.y];
          // layer.py:126-142 by the sign of two dot products; the literal atan2 form only for the lanes (if any) whose
          // angle is within 1e-6 rad of the pi/2 threshold
          bool certain;
          bool inb = d_within_bounds_filter(n0.x, n0.y, n1.x, n1.y, s.x, s.y, certain);
          if (!certain) inb = d_within_bounds(n0.x, n0.y, n1.x, n1.y, m.ori_fwd[ge], m.ori_rev[ge], s.x, s.y);
          if (inb) {
            dist_l = tc_fabs(d_distance_to_edge(n0.x, n0.y, n1.x, n1.y, s.x, s.y));
          } else {
            double da = d_dist(s.x, s.y, n0.x, n0.y);
            double db = d_dist(s.front_x, s.front_y, n1.x, n1.y);  // FRONT axle for n1 (car.py:64)
            dist_l = db < da ? db : da;
          }
        }
        lv->dist[l] = dist_l;
        lv->ne[l] = my_e;
        if (roll.dist) roll.dist[(roll.row0 + env) * C + l] = dist_l;
        if (roll.ne) roll.ne[(roll.row0 + env) * C + l] = my_e;
      }
      TSTAMP(16);
      lds_sync();  // dn aliases the camera's node buffer
    } else if (need_b && tid < C) {
      lv->dist[tid] = 0;
      lv->ne[tid] = -1;
      if (roll.dist) roll.dist[(roll.row0 + env) * C + tid] = 0;
      if (roll.ne) roll.ne[(roll.row0 + env) * C + tid] = -1;
    }
    if (late) {
      // a re-spawned env did not go through Wrapper.step (the reference's reset() bypasses the wrappers)
      if (!fresh) {
        d_apply_terms(a.terms, a.n_terms, my_cnt, PER ? car_ld<true>(crow, TC_CAR_TRACK_WIDTH) : a.car.track_width, tid, C,
                      cte, have_info ? s.velocity : 0.0, dist_l, reward, terminated);
        if (tid < TC_MAX_TERMS) lv->cnt[tid] = my_cnt;
      }
      if (tid == 0) {
        lv->reward = reward;
        lv->terminated = terminated;
        lv->needs_reset = (flags & TC_F_AUTORESET) ? (terminated || trunc) : 0;
        if (roll.reward) roll.reward[roll.row0 + env] = reward;
        if (roll.terminated) roll.terminated[roll.row0 + env] = (unsigned char)terminated;
        if (EP) ep_close(ep, env, roll.row0 + env, fresh, status, ep_len, lv->ep_ret, reward, terminated | trunc);
      }
    }
  }

  TSTAMP(3);
  TSTAMP_REAL(29);
  // what the camera stage needs.  car.py:159-165 takes cos(-theta), sin(-theta): tc_cos is exactly even and tc_sin
  // exactly odd (their kernels are built from x*x and x*y terms only), so the values of the front-axle update are
  // reused bit for bit.
  fp.x = s.x;
  fp.y = s.y;
  if (have_trig) {
    fp.cth = s.cth;
    fp.sth = -s.sth;
  } else {
    fp.cth = tc_cos(-s.theta);
    fp.sth = tc_sin(-s.theta);
  }
}

#endif  // K_SIM_H
