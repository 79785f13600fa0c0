/* tinycarlo_hip.h -- C ABI of libtinycarlo_hip.so: batched tinycarlo step()/reset() on one MI355X.
 *
 * The reference (emrullahArkun/tinycarlo) is pure Python and has no FFI; its only seam is the
 * gymnasium API of tinycarlo/env.py.  This header is what a Python `TinyCarloEnv` binds through
 * ctypes to move the per-step hot path onto the GPU (binding shown in INTEGRATION.md):
 *
 *   reference interface replaced                                  entry point here
 *   ------------------------------------------------------------  -------------------------
 *   Map.__init__ / __change_scale      tinycarlo/map.py:9-37       tc_map_create
 *   Car.__init__, Camera.__init__      car.py:10-19, camera.py:12-24  tc_env_create
 *   Camera.update_params               camera.py:48-50             tc_env_set_camera
 *   TinyCarloEnv.reset                 env.py:101-113              tc_reset
 *     (Car.reset car.py:34-44, Map.sample_spawn map.py:51-69 with the node index drawn by the host RNG)
 *   TinyCarloEnv.step                  env.py:115-147              tc_step
 *     (Car.step car.py:70-125, Car.find_local_path 127-148, Layer.* layer.py:33-187,
 *      Camera.capture_frame camera.py:52-110, Renderer.render_camera_frame_{rgb,classes}
 *      renderer.py:36-51, Car.get_info car.py:46-68, default reward/termination env.py:87-99)
 *
 * Conventions
 *   - N independent envs live as structure-of-arrays in device memory OWNED BY THE CALLER
 *     (e.g. torch tensors); the library stores the pointers given to tc_env_bind and never frees them.
 *   - every pointer inside tc_buffers, and the action pointers of tc_step / tc_reset, are DEVICE
 *     pointers on the device that was current at tc_map_create time.
 *   - kernels are enqueued on the hipStream_t passed as `stream` (void*, NULL = default stream) and complete in
 *     stream order; tc_reset / tc_step / tc_step_multi / tc_render* / tc_noise neither allocate nor synchronise
 *     (they can be captured into a HIP graph).  The calls that DO wait for the device: tc_map_create,
 *     tc_env_create, tc_env_reserve_steps (when it has to re-allocate), tc_env_set_terms, tc_env_set_noise,
 *     tc_env_set_spawn_table, tc_env_profile_read and the destroy calls.
 *   - one host thread per env handle at a time, and ONE STREAM AT A TIME per handle: the library-owned scratch of a
 *     handle (draw lists, pose rows) is reused by consecutive calls, which is safe because they follow each other in
 *     stream order.  A K-step call issued on a different stream than the handle's previous K-step call is ordered
 *     behind it by the library (an event wait); for every other combination of streams the caller orders them.
 *   - every function returns 0 on success or a negative TC_E_* code; nothing throws.
 *   - arithmetic is IEEE double like the reference (python floats / numpy float64); pixel
 *     coordinates are int32, observations uint8.
 */
#ifndef TINYCARLO_HIP_H
#define TINYCARLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 7: the per-step rows of the per-episode features are arguments of the K-step call (tc_step_rows, a parameter of
 * tc_step_multi) and no longer installed on the handle: the episode-rollout setter and the row members of tc_controller,
 * tc_drive_randomization and tc_camera_bank are gone.
 * ABI 6: per-env car constants and their per-episode draw (tc_env_set_car, tc_env_set_car_per_env,
 * tc_env_set_car_randomization, TC_CAR_*) */
#define TC_ABI_VERSION 7
/* Additive within ABI 6 (new entry points only, no struct changed): tc_env_set_episodes, TC_S_TIME_LIMIT.  Callers that
 * must run against an older ABI-6 library test for this macro / the symbols. */
#define TC_HAS_EPISODES 1
/* Likewise additive within ABI 6: tc_env_set_controller, tc_controller, TC_CTRL_STANLEY. */
#define TC_HAS_CONTROLLER 1
/* Likewise additive within ABI 6: TC_FMT_CLASSES_BITS, tc_unpack_bits, TC_U8 / TC_F16 / TC_BF16. */
#define TC_HAS_PACKED_OBS 1
/* Likewise additive within ABI 6: tc_env_set_camera_bank, tc_camera_bank. */
#define TC_HAS_CAMERA_BANK 1
/* Likewise additive within ABI 6: tc_env_set_drive_randomization, tc_drive_randomization, TC_MAN_*, tc_draw_normals. */
#define TC_HAS_DRIVE_RANDOMIZATION 1
/* Likewise additive within ABI 6: tc_collect, tc_collect_scratch_bytes, tc_collect_desc, TC_COLLECT_*. */
#define TC_HAS_COLLECT 1
/* Likewise additive within ABI 6: tc_collect_link, tc_history_resolve, tc_gather_frames, TC_PAD_*. */
#define TC_HAS_HISTORY 1
/* Additive within ABI 7: tc_env_reserve_poses, tc_render_poses (deferred frames). */
#define TC_HAS_RENDER_POSES 1
#define TC_MAX_LAYERS 16

/* error codes */
#define TC_OK 0
#define TC_E_INVALID (-1)  /* bad argument / inconsistent sizes */
#define TC_E_HIP (-2)      /* a HIP runtime call failed (tc_last_error() has the text) */
#define TC_E_NOMEM (-3)
#define TC_E_UNBOUND (-4)  /* tc_step/tc_reset before tc_env_bind */
#define TC_E_LDS (-5)      /* map/camera too large for the 160 KiB LDS budget of one workgroup */

/* observation formats (sim.observation_space_format, env.py:42,67-72) */
#define TC_FMT_RGB 0     /* uint8 [N][H][W][3] */
#define TC_FMT_CLASSES 1 /* uint8 [N][C][H][W], values 0/255 */
/* Bit-packed class masks: uint8 [N][C][H][W/8].  Pixel (y, x) of class c is bit x & 7 of byte x >> 3 of row y of plane c; a
 * set bit stands for 255 -- np.packbits(mask != 0, axis=-1, bitorder="little") of the TC_FMT_CLASSES frame, one eighth of its
 * bytes.  All planes of an env are contiguous (a frame is C*H*W/8 bytes, see tc_env_obs_bytes).  An opt-in of the batched
 * env, not a value of sim.observation_space_format: the reference has no such format.
 *   - W % 32 != 0 with this format is TC_E_INVALID from tc_env_create and tc_env_set_camera.
 *   - tc_env_set_noise works as for TC_FMT_CLASSES (the blobs are applied to the bit-planes before the store, same stream).
 *   - the stand-alone tc_noise pass reads byte masks: on a packed env it returns TC_E_INVALID (out of scope).
 *   - what is launched: tc_frame_kernel, tc_frame_recover_kernel and tc_raster_kernel exist for this format, the fused
 *     tc_step_kernel / tc_drive_step_kernel do not.  tc_step / tc_reset / tc_render therefore take the two-launch form
 *     (tc_env_kernel + tc_raster_kernel, what TC_FUSE=0 selects for the byte formats), K-step calls the streamed or chunked
 *     frame-kernel forms, and TC_MULTI_SPLIT=0 is ignored.  tc_env_launch_info reports it.
 *   - tc_unpack_bits expands packed frames on the device. */
#define TC_FMT_CLASSES_BITS 2

/* dtypes: TC_F32 / TC_F64 are the action dtypes of tc_step; TC_U8, TC_F16, TC_BF16 and TC_F32 the output dtypes of
 * tc_unpack_bits */
#define TC_F32 0
#define TC_F64 1
#define TC_U8 2
#define TC_F16 3
#define TC_BF16 4

/* step / reset flags */
#define TC_F_NO_OBSERVATION 1u /* env.no_observation (env.py:60,78-81): obs left untouched, no camera work */
#define TC_F_WRAPPED 2u        /* env.wrapped (env.py:56,137-138): reward = 0, terminated = false */
#define TC_F_AUTORESET 4u      /* envs whose needs_reset flag is set are re-spawned from spawn_queue at the
                                  start of the step (their action is ignored, reward 0, info empty) and the
                                  flag is set again from terminated|truncated at the end of the step */

#define TC_F_DEVICE_SPAWN 8u    /* with TC_F_AUTORESET: re-spawn nodes are drawn on the device from the table of
                                  tc_env_set_spawn_table (counter-based, tinycarlo_amd/csrc/tc_rng.h) instead of
                                  being read from spawn_queue; spawn_cursor[i] counts env i's re-spawns */

/* per-env status bits (tc_buffers.status), situations where the reference raises a Python exception */
#define TC_S_UTURN_NO_EDGE 1 /* U-turn found no lanepath edge within +-30 deg (TypeError at car.py:143): truncated */
#define TC_S_PICK_EMPTY 2    /* neighbour list made only of self-loops (ValueError at layer.py:123): truncated */
#define TC_S_BAD_SPAWN 4     /* spawn node out of range or without out-edge: first spawnable node used instead */
#define TC_S_NOT_RESET 8     /* tc_step on an env that was never reset: truncated, state untouched */
#define TC_S_SPAWN_WRAPPED 16 /* TC_F_AUTORESET without TC_F_DEVICE_SPAWN: this re-spawn read spawn_queue past its end
                                 (cursor >= spawn_queue_len, the queue is consumed cyclically): from here on the env
                                 replays spawn nodes it already used -- refill the queue and clear spawn_cursor */
#define TC_S_TIME_LIMIT 32   /* tc_env_set_episodes: the episode reached its time limit in this step: truncated */

/* Reward / termination terms: the wrappers of tinycarlo/wrapper/reward.py and termination.py, evaluated in the
 * epilogue of the step kernel in the order given (= the order the wrappers are stacked, innermost first; reward
 * additions are floating point, so the order is part of the result). */
#define TC_MAX_TERMS 8
#define TC_T_LANELINE_SPARSE_REWARD 1       /* reward.py:5-23   per_layer = sparse_rewards[name], layer_mask = names present */
#define TC_T_LANELINE_LINEAR_REWARD 2       /* reward.py:25-42  per_layer = max_rewards[name] (every layer) */
#define TC_T_CTE_SPARSE_REWARD 3            /* reward.py:44-62  p = {min_cte, sparse_reward} */
#define TC_T_CTE_LINEAR_REWARD 4            /* reward.py:64-84  p = {min_cte, max_reward, min_reward} */
#define TC_T_LANELINE_CROSSING_TERMINATION 5 /* termination.py:4-22   layer_mask = lanelines */
#define TC_T_CTE_TERMINATION 6              /* termination.py:24-48  p = {max_cte}, number_of_steps */
#define TC_T_CRASH_TERMINATION 7            /* termination.py:50-70  p = {velocity threshold}, number_of_steps */

typedef struct {
  int32_t kind;            /* TC_T_* */
  int32_t number_of_steps; /* consecutive-step terms */
  uint32_t layer_mask;     /* bit l = lane-line layer l takes part */
  int32_t reserved;
  double p[4];
  double per_layer[TC_MAX_LAYERS];
} tc_term;

typedef struct tc_map tc_map;
typedef struct tc_env tc_env;

/* Host-side description of a map, coordinates already in metres (map.py:28-37).
 * Lane-line layers are concatenated in JSON key order (map.py:23); edge node ids are layer-local. */
typedef struct {
  int32_t n_layers;
  const int32_t* node_count; /* [n_layers] */
  const int32_t* edge_count; /* [n_layers] */
  const double* nodes;       /* [sum node_count][2] */
  const int32_t* edges;      /* [sum edge_count][2] */
  const uint8_t* colors;     /* [n_layers][3], written to channels 0,1,2 as given (renderer.py:43) */
  int32_t lanepath_node_count;
  int32_t lanepath_edge_count;
  const double* lanepath_nodes;  /* [lanepath_node_count][2] */
  const int32_t* lanepath_edges; /* [lanepath_edge_count][2] */
} tc_map_desc;

/* car.py:10-19 */
typedef struct {
  double T; /* 1/fps, env.py:40-41 */
  double wheelbase, track_width, max_velocity, max_steering_angle;
  double steering_speed;                  /* used when has_steering_speed */
  double max_acceleration, max_deceleration; /* used when has_max_acceleration */
  int32_t has_steering_speed, has_max_acceleration;
} tc_car_params;

/* Per-env car constants (tc_env_set_car_per_env): one row of TC_CAR_NP doubles per env, columns below.  T (1/fps) and
 * the presence flags has_steering_speed / has_max_acceleration stay shared; a column whose presence flag is 0 is
 * ignored.  The steering input of env i becomes np.clip(st + row[i][TC_CAR_STEERING_SHIFT], -1, 1) (the shift is added
 * before the clamp, examples/train_td3.py:146-148).  Wheelbase: kinematics, front axle and re-spawn pose; track width:
 * the base reward / termination (env.py:93,99) and the fused terms; the rest: the kinematic update (car.py:70-125). */
#define TC_CAR_NP 8
#define TC_CAR_WHEELBASE 0
#define TC_CAR_TRACK_WIDTH 1
#define TC_CAR_MAX_VELOCITY 2
#define TC_CAR_MAX_STEERING_ANGLE 3
#define TC_CAR_STEERING_SPEED 4
#define TC_CAR_MAX_ACCELERATION 5
#define TC_CAR_MAX_DECELERATION 6
#define TC_CAR_STEERING_SHIFT 7

/* camera.py:12-24; E and K are computed on the host exactly as camera.py:145-178 does */
typedef struct {
  int32_t height, width;
  double E[12]; /* 3x4 row major */
  double K[9];  /* 3x3 row major */
  double max_range;
  int32_t line_thickness;
  int32_t format; /* TC_FMT_* */
} tc_camera_params;

/* Device buffers, all [N] unless noted.  State is in/out, the rest is written by tc_step/tc_reset. */
typedef struct {
  /* --- car state (car.py:25-32) */
  double *x, *y, *theta;  /* rear-axle position (m), heading (rad) */
  double *velocity;       /* m/s */
  double *steering;       /* deg */
  double *radius;         /* m, 0 when driving straight */
  double *front_x, *front_y;
  int32_t* local_path;    /* [N][8]: up to 4 lanepath edges (n0,n1), -1 padded */
  int32_t* lp_len;        /* 1 after reset, 1..4 after a step */
  int32_t* last_maneuver;
  /* --- per-step outputs (env.py:83-85,136-147) */
  double *cte, *heading_error, *reward;
  uint8_t *terminated, *truncated;
  int32_t* status;             /* TC_S_* bits */
  double* laneline_distances;  /* [N][n_layers] */
  int32_t* nearest_edge;       /* [N][n_layers] layer-local edge index of Layer.get_nearest_edge(rear), -1 if info empty */
  uint8_t* obs;                /* [N][C][H][W], [N][H][W][3] or [N][C][H][W/8]; may be NULL if every call passes TC_F_NO_OBSERVATION */
  /* --- auto-reset (TC_F_AUTORESET) */
  uint8_t* needs_reset;        /* [N] */
  const int32_t* spawn_queue;  /* [N][spawn_queue_len] spawnable lanepath node ids drawn by the host RNG */
  int32_t* spawn_cursor;       /* [N] */
  int32_t spawn_queue_len;
} tc_buffers;

int tc_abi_version(void);
const char* tc_last_error(void);

int tc_map_create(const tc_map_desc* desc, tc_map** out);
int tc_map_destroy(tc_map* map);

int tc_env_create(const tc_map* map, const tc_car_params* car, const tc_camera_params* cam, int32_t num_envs,
                  tc_env** out);
int tc_env_destroy(tc_env* env);
int tc_env_bind(tc_env* env, const tc_buffers* buffers);
/* New E/K (and range / thickness) for all envs; takes effect for launches enqueued afterwards. */
int tc_env_set_camera(tc_env* env, const tc_camera_params* cam);
/* Per-env cameras (domain randomisation: examples/train_stanley_il.py:53-57 changes camera.orientation / fov and
 * calls update_params() once per episode; batched, that is one E and K per env).  E: device double [N][12],
 * K: device double [N][9], caller owned and read by every launch until replaced; (NULL, NULL) returns to the shared
 * camera of tc_env_create / tc_env_set_camera.  Resolution, max_range, thickness and format stay shared.  Removes a
 * camera bank (tc_env_set_camera_bank), whatever the arguments. */
int tc_env_set_camera_per_env(tc_env* env, const double* E, const double* K);
/* Per-EPISODE cameras from a bank (the data collection of examples/train_stanley_il.py:53-57 -- a new pitch and fov, then
 * update_params() and reset(), for every episode -- without leaving a K-step call at each termination).  The bank is `count`
 * cameras computed on the host like the shared one (so no trigonometry on the device); env i uses camera index[i], and every
 * re-spawn of env i by the library (tc_reset of an env the mask selects, or a TC_F_AUTORESET re-spawn in either spawn mode
 * and in every kernel form), before the new pose is set, draws its next one:
 *   z        = SplitMix64(SplitMix64(seed)[0x63616D])[(env_offset + i) << 32 | episode[i]]
 *   index[i] = ((z >> 32) * count) >> 32
 *   episode[i] += 1
 * (tinycarlo_amd/csrc/tc_rng.h: tc_camera_index; a stream of its own, and a counter apart from the cars').
 * The index in force when a step was simulated travels WITH that (step, env) to wherever its frame is drawn -- in a streamed,
 * chunked or recovered K-step call that is possibly after the env has re-spawned again -- so a frame is always projected with
 * the E and K of the episode it belongs to.  tc_step_rows.camera_out[k][i] receives the index in force at step k of a
 * tc_step_multi call.
 * Everything else is as with per-env cameras: resolution, max_range, thickness and format stay shared, draw-list capacity and
 * plan hold for arbitrary E / K, and the whole-frame cull is off while a bank is installed.  A bank and the static rows of
 * tc_env_set_camera_per_env exclude each other: installing one removes the other.  bank = NULL returns to the shared camera.
 * seed, count and env_offset sit in a library-owned device table updated in place (a captured graph sees new settings
 * without re-capture; a call that changes them waits for the device, one that leaves them as they are does not); the
 * pointers are kernel arguments of the launches enqueued afterwards.  An index found outside [0, count) in `index` is read
 * as count - 1; nothing is read out of bounds.
 * TC_E_INVALID: a NULL E, K, index or episode, count < 1. */
typedef struct {
  const double* E;     /* device [count][12] */
  const double* K;     /* device [count][9] */
  int32_t count;       /* cameras in the bank */
  uint32_t env_offset; /* index of env 0 in a larger population (shards draw what one batch would) */
  uint64_t seed;
  int32_t* index;      /* device [N], in/out, caller owned: the camera each env uses */
  int32_t* episode;    /* device [N], in/out, caller owned: cameras drawn so far */
} tc_camera_bank;
int tc_env_set_camera_bank(tc_env* env, const tc_camera_bank* bank); /* NULL = off */
/* New shared car (Car constants assigned at run time: the reference's Car.step reads them on every step, car.py:70-125).
 * Takes effect for launches enqueued afterwards; T must stay the value of tc_env_create. */
int tc_env_set_car(tc_env* env, const tc_car_params* car);
/* Per-env cars.  params: device double [N][TC_CAR_NP], caller owned, read (and, with tc_env_set_car_randomization,
 * written) by every launch until replaced; NULL returns to the shared car and drops the randomisation.  The kernels
 * that read it are separate instantiations chosen at launch: the shared-car kernels are unchanged. */
int tc_env_set_car_per_env(tc_env* env, double* params);
/* Per-episode randomisation of the per-env cars.  On every re-spawn of env i by the library (tc_reset of an env the
 * mask selects, or a TC_F_AUTORESET re-spawn in either spawn mode), before the new pose is set:
 *   z = SplitMix64(SplitMix64(seed)[0x636172])[(env_offset + i) << 32 | episode[i]]
 *   params[i][j] = lo[j] + (hi[j] - lo[j]) * ((SplitMix64(z)[j] >> 11) * 2^-53)   for every column j in column_mask
 *   episode[i] += 1
 * (tinycarlo_amd/csrc/tc_rng.h: tc_car_stream, tc_car_draw).  Columns outside the mask keep their values; lo == hi gives
 * exactly lo.  lo, hi: HOST arrays of TC_CAR_NP, copied into a library-owned device table that is updated in place (a
 * captured graph sees new ranges, mask and seed without re-capture; the call waits for the device).  episode: device
 * int32 [N], caller owned.  env_offset: index of env 0 in a larger population (shards of a multi-GPU run draw the rows
 * one batch would).  column_mask = 0 stops resampling.  TC_E_INVALID without per-env params, with lo > hi, a non-finite
 * bound, a mask bit >= TC_CAR_NP or a bit for a column whose presence flag is 0. */
int tc_env_set_car_randomization(tc_env* env, const double* lo, const double* hi, uint32_t column_mask, uint64_t seed,
                                 uint32_t env_offset, int32_t* episode);
/* Episode time limit and per-env episode statistics, kept by the step kernels (gymnasium's TimeLimit and
 * RecordEpisodeStatistics; `for ep_step in range(MAX_STEPS)` / `ep_rew += rew` of examples/train_td3.py:181,199).
 * All members are DEVICE arrays of N, caller owned, read and written by every tc_reset / tc_step / tc_step_multi until
 * replaced.  length and ret are required, the others may be NULL.  bufs = NULL switches the feature off; without it nothing changes, and the kernels that do the accounting are separate instantiations
 * chosen at launch (the TC_FEAT_EP bit of their feature mask): the others are untouched.
 * Per env i; limit_i = limit[i] when limit is given, else max_episode_steps; a value <= 0 means no limit:
 *   1. (re)spawned by tc_reset (mask) or by a TC_F_AUTORESET re-spawn at the start of a step: length = 0, ret = 0.0.  The
 *      re-spawn step itself counts nothing; count, last_* and *_sum are not touched.
 *   2. any other step of an env that has been reset: length += 1; if limit_i > 0 and length >= limit_i: truncated = 1,
 *      status |= TC_S_TIME_LIMIT, whatever `terminated` is.  Then ret = ret + reward with the step's final reward (after
 *      the fused terms): one double add per step, in step order.
 *   3. if terminated | truncated after that: last_length = length, last_return = ret, count += 1, length_sum += length,
 *      return_sum += ret.  length and ret keep their values until the re-spawn (without TC_F_AUTORESET they go on counting).
 *   4. a time-limit truncation is an ordinary truncation: under TC_F_AUTORESET it sets needs_reset, and the next step --
 *      of the same K-step launch too -- re-spawns the env (spawn queue entry / device draw, new car with randomisation).
 *   5. envs with TC_S_NOT_RESET are left alone.
 * length is an ordinary in/out array: writing to it between calls staggers the episodes.
 * max_episode_steps sits in a library-owned device word updated in place (a captured graph sees a new value without
 * re-capture; the call waits for the device). */
typedef struct {
  int32_t* length;      /* [N] running episode: steps so far */
  double* ret;          /* [N] running episode: sum of rewards so far */
  int32_t* count;       /* [N] episodes finished */
  int32_t* last_length; /* [N] most recent finished episode */
  double* last_return;
  int64_t* length_sum;  /* [N] over all finished episodes of env i */
  double* return_sum;
  const int32_t* limit; /* [N] per-env limit, or NULL */
} tc_episode_buffers;
int tc_env_set_episodes(tc_env* env, const tc_episode_buffers* bufs, int32_t max_episode_steps);
/* Per step of a tc_step_multi call: tc_step_rows.episode_length_out[k][i] / episode_return_out[k][i] hold env i's length /
 * ret after step k (the episode's totals on a row where it ended, 0 / 0.0 on a re-spawn row). */
/* Built-in controller: the action of every step is computed by the simulate kernels from what the env reported after its
 * previous step, so a closed control loop -- the `while: step(controller(info))` of examples/stanley_control.py:50-60 and
 * of the data collection of examples/train_stanley_il.py -- runs inside ONE tc_step_multi call.  With a controller
 * installed, per env i and step k of a call:
 *   - car_control of tc_step / tc_step_multi is ignored and may be NULL; maneuver rows are read as before.
 *   - steer = (((he + atan2(k * cte, speed)) * 180.0) / 3.141592653589793) / max_steering_angle, in this operation order
 *     (tinycarlo_amd/csrc/tc_ctrl.h: tc_ctrl_stanley; stanley_control.py:56-57).  cte / he are what the env reported
 *     after its previous step: the bound cte / heading_error buffers at the first step of a call, 0 / 0 after a reset or
 *     re-spawn -- exactly what a host loop reads between two tc_step calls.  max_steering_angle is the env's own: its
 *     per-env car row when rows are installed (tc_env_set_car_per_env), else the shared car's.
 *   - the applied action is (speed, steer + steer_noise_in[k][i]) with a call's noise rows (tc_step_rows), else
 *     (speed, steer); from there the existing path: velocity clip, steering shift, steering clip, kinematics.
 *   - steer (BEFORE noise: the imitation-learning label, train_stanley_il.py:73) goes to the call's steer_out[k][i]
 *     (tc_step_rows) and to steer_last[i].  A step that applies no action -- a TC_F_AUTORESET re-spawn, whose action is
 *     ignored as ever, or an env with TC_S_NOT_RESET, which is left alone -- stores 0.0 there.
 *   - a tc_step has no rows: its command goes to steer_last only.
 * k and speed sit in a library-owned device table updated in place (a captured graph sees new gains without re-capture;
 * a call that changes them waits for the device, one that leaves them as they are does not).  The kernels that run the
 * controller are entry points of their own chosen at launch (tc_drive_step_kernel, tc_drive_env_kernel,
 * tc_drive_envg_kernel: the TC_FEAT_CTRL bit of the feature mask); without a controller nothing changes.  c = NULL
 * switches it off.
 * TC_E_INVALID: an unknown kind, non-finite k or speed. */
#define TC_CTRL_STANLEY 1
typedef struct {
  int32_t kind;       /* TC_CTRL_STANLEY */
  double k, speed;    /* gain; velocity command in [-1,1] units, also atan2's second argument (stanley_control.py:56) */
  double* steer_last; /* device [N] or NULL, out: the command BEFORE noise of the most recent step (the IL label, train_stanley_il.py:73) */
} tc_controller;
int tc_env_set_controller(tc_env* env, const tc_controller* c); /* NULL = off; drops the drive randomisation too */
/* Drive randomisation: what examples/train_stanley_il.py and examples/train_td3.py do to the action at an episode boundary,
 * inside a call, where only the kernel knows where an episode ends.  Two parts, each optional, both need a controller:
 *   maneuvers (n_maneuvers > 0): the maneuver is a per-episode quantity (train_stanley_il.py:105, train_td3.py:178) kept in
 *     maneuver[i]; entries of `maneuvers` are in {0, 1, 2, 3}, repeats act as weights.
 *   OU noise (ou_state != NULL): noise += THETA * (MEAN - noise) + SIGMA * randn (train_stanley_il.py:66, train_td3.py:143)
 *     kept in ou_state[i], reset to 0 at every episode start when ou_reset != 0 (train_td3.py:177), else carried across.
 * Per env i:
 *   - a re-spawn by the library (tc_reset of an env the mask selects, or a TC_F_AUTORESET re-spawn in either spawn mode and in
 *     every kernel form): with n_maneuvers > 0, e = episode[i] and
 *       TC_MAN_DRAW   maneuver[i] = maneuvers[((z >> 32) * n_maneuvers) >> 32],
 *                     z = SplitMix64(SplitMix64(seed)[0x6D616E])[(env_offset + i) << 32 | e]
 *       TC_MAN_CYCLE  maneuver[i] = maneuvers[(env_offset + i + e) % n_maneuvers]
 *     then episode[i] += 1; with ou_reset != 0, ou_state[i] = 0.0.  The re-spawn step applies no action: it consumes no
 *     normal, stores 0.0 in the call's ou_noise_out row and the NEW episode's maneuver in its maneuver_out row (tc_step_rows).
 *   - a step that applies an action: the maneuver is maneuver[i] when n_maneuvers > 0 (the `maneuver` argument of tc_step /
 *     tc_step_multi is then ignored and may be NULL), else the call's maneuver row as ever.  With OU noise:
 *       eps = normal number ou_draws[i] of env (env_offset + i) of the seed; ou_draws[i] = (ou_draws[i] + 1) mod 2^31
 *       n   = ou_state[i] + (theta * (mu - ou_state[i]) + sigma * eps); ou_state[i] = n
 *     (tinycarlo_amd/csrc/tc_rng.h: tc_normal_at -- Box-Muller on a sub-stream of its own -- and tc_ou_step) and the applied
 *     steering is steer + n, or (steer + steer_noise_in[k][i]) + n when the call has noise rows.  steer_out / steer_last
 *     keep the command before any noise; ou_noise_out[k][i] = n, maneuver_out[k][i] = the maneuver used.
 *   - envs with TC_S_NOT_RESET are left alone: no draw, noise row 0.0.
 * All state lives in the caller's arrays between calls, so a K-step call is bit-identical to K tc_step calls and to any
 * split of the K steps.
 * seed, env_offset, candidates, mode, theta, mu, sigma and ou_reset sit in a library-owned device table updated in place (a
 * captured graph sees new values without re-capture; a call that changes them waits for the device, one that leaves them as
 * they are does not); the pointers are
 * kernel arguments of the launches enqueued afterwards, and so is which of the two parts is on.  Runs in the tc_drive_*
 * entry points behind a run-time branch; while it is on, tc_reset takes them too.  d = NULL switches it off, and so does a
 * struct with neither part (n_maneuvers = 0 and ou_state = NULL).
 * TC_E_INVALID, before any device work: no controller installed, a maneuver outside 0..3, n_maneuvers outside 0..8, an
 * unknown mode, a non-finite theta / mu / sigma, n_maneuvers > 0 with a NULL maneuver or episode, ou_state without ou_draws. */
#define TC_MAN_DRAW 0
#define TC_MAN_CYCLE 1
typedef struct {
  uint64_t seed;
  uint32_t env_offset;    /* index of env 0 in a larger population (shards draw what one batch would) */
  int32_t n_maneuvers;    /* 0..8; 0: the call's maneuver rows as ever */
  int32_t maneuvers[8];   /* candidates, each 0, 1, 2 or 3 */
  int32_t maneuver_mode;  /* TC_MAN_DRAW or TC_MAN_CYCLE */
  int32_t ou_reset;       /* != 0: ou_state = 0.0 at every re-spawn */
  double theta, mu, sigma;
  int32_t* maneuver;      /* device [N], in/out, caller owned: the maneuver in force */
  int32_t* episode;       /* device [N], in/out: episodes drawn so far */
  double* ou_state;       /* device [N], in/out, or NULL: no OU noise */
  int32_t* ou_draws;      /* device [N], in/out: normals consumed so far (never reset; wraps at 2^31) */
} tc_drive_randomization;
int tc_env_set_drive_randomization(tc_env* env, const tc_drive_randomization* d); /* NULL = off */
/* Normal number first_draw + j (mod 2^31) of env `env` (tc_normal_at of tc_rng.h) for j < n into out[j], on the host (no
 * device needed): what a restatement of the OU process in another language calls. */
int tc_draw_normals(uint64_t seed, uint32_t env, uint32_t first_draw, int32_t n, double* out);
/* Installs n_terms (0..TC_MAX_TERMS) reward / termination terms; they apply to every tc_step enqueued afterwards
 * (the call waits for earlier launches).  Each term starts from the reward / terminated value left by the one
 * before it, the first from the base values of env.py:136-138 (0 / false under TC_F_WRAPPED, which the reference
 * wrappers always set).  counters: device int32 [N][TC_MAX_TERMS], caller owned, zero-initialised: steps_true of
 * the consecutive-step terms (termination.py:37,59), one per env and term slot; like the reference's attribute it
 * is NOT cleared when an env is reset.  May be NULL when no such term is installed.  Envs re-spawned by
 * TC_F_AUTORESET in a step skip the terms for that step (the reference's reset() does not pass through
 * Wrapper.step): reward 0, terminated 0, counters untouched.  n_terms = 0 removes all terms. */
int tc_env_set_terms(tc_env* env, const tc_term* terms, int32_t n_terms, int32_t* counters);
/* Device-side spawn sampling (TC_F_DEVICE_SPAWN).  nodes: HOST array of n > 0 lanepath node ids, copied by the call:
 * the candidates of Map.sample_spawn (map.py:61: spawn_points, or 0..len(nodes)-2) that have an out-edge, duplicates
 * kept -- a uniform draw from it is distributed like the reference's draw-again-on-sinks loop (map.py:62-64).
 * Re-spawn number k of env i uses SplitMix64 output (i << 32 | k) of the stream `seed`.  Not seed-compatible with
 * the reference's numpy generator; the host-drawn spawn_queue remains the seed-parity mode.  n = 0 removes the table. */
int tc_env_set_spawn_table(tc_env* env, const int32_t* nodes, int32_t n, uint64_t seed);
/* NoiseObservationWrapper (wrapper/observation.py:5-33) for class-mask observations: per class plane n_blobs blobs,
 * each a filled circle (centre inside the frame, radius in [1, max_radius)) that either erases the plane inside the
 * circle or ORs in the circle-masked content of a random plane, applied in order.  With n_blobs > 0 every tc_step /
 * tc_step_multi that renders an observation applies the blobs inside the raster stage, on the frame's bit-planes in
 * LDS before they are expanded to bytes (no extra pass over the observation in HBM), blobs drawn on the device
 * (tinycarlo_amd/csrc/tc_rng.h; the reference draws from the global numpy generator, which cannot be reproduced
 * for a batch).  Every rendered step consumes one position of the blob stream; the position is a counter in device
 * memory advanced on the stream behind the launch, so a call captured into a HIP graph draws new blobs on every
 * replay.  tc_reset / tc_render frames carry no noise (the reference's reset() does not pass through the wrapper's
 * step()).  n_blobs = 0 switches the noise off.  Needs TC_FMT_CLASSES or TC_FMT_CLASSES_BITS and max_radius in [2, 256]. */
int tc_env_set_noise(tc_env* env, int32_t n_blobs, int32_t max_radius, uint64_t seed);
/* The noise pass alone, on the currently bound observation.  blobs: device int32 [N][n_layers * n_blobs][5] rows
 * (x, y, radius, mode, src) -- blob k belongs to plane k / n_blobs, mode 1 = copy from plane src, 0 = erase -- or
 * NULL to draw them on the device as tc_step does.  Byte class masks only: TC_E_INVALID on a TC_FMT_CLASSES_BITS env. */
int tc_noise(tc_env* env, const int32_t* blobs, void* stream);
/* bytes of one env's observation: C*H*W (classes), H*W*3 (rgb), C*H*W/8 (packed classes) */
int64_t tc_env_obs_bytes(const tc_env* env);
/* dynamic LDS bytes one workgroup of the step kernel uses (for occupancy reporting) */
int64_t tc_env_lds_bytes(const tc_env* env);

/* Per-kernel timing for benchmarks: with enable = n > 0 every n-th tc_step records HIP events on the caller's
 * stream around its two kernels ("simulate": kinematics + tracking + distances + camera geometry; "raster":
 * cv2.polylines + observation store) into a ring of the last 64 launches.  tc_env_profile_read waits for
 * those launches and returns their mean durations in microseconds.  When a step is issued as ONE fused kernel
 * (the default unless a lane-line layer has more than 576 nodes / edges; env var TC_FUSE=0 forces two launches), simulate_us is
 * the duration of that kernel and raster_us is ~0. */
int tc_env_profile(tc_env* env, int32_t enable);
int tc_env_profile_read(tc_env* env, double* simulate_us, double* raster_us, int32_t* launches);

/* env.py:101-113 for the envs selected by mask (NULL = all): pose from spawn_nodes[i], zeroed info,
 * observation rendered unless TC_F_NO_OBSERVATION. */
int tc_reset(tc_env* env, const int32_t* spawn_nodes, const uint8_t* mask, uint32_t flags, void* stream);

/* env.py:115-147 for all envs.  car_control: [N][2] (velocity, steering in [-1,1], clipped like env.py:118),
 * dtype TC_F32 or TC_F64; maneuver: [N] in {0,1,2,3}.
 * One launch (tc_step_kernel: a wavefront simulates its env, runs the camera and rasterises the frame).  Which env a
 * workgroup works on is the library's choice -- envs are independent, any assignment gives the same results: when N is
 * 2-4 rows of one workgroup per SIMD of the device, the envs are re-dealt every TC_STEP_ORDER-th call (default 8; a
 * one-workgroup tc_order_kernel launch in front of the step) so that frames with long and short draw lists share a
 * SIMD (workgroups w, w + #SIMDs, ... land on the same SIMD). */
int tc_step(tc_env* env, const void* car_control, int32_t control_dtype, const int32_t* maneuver, uint32_t flags,
            void* stream);

/* K steps in ONE call: the caller's `for k in range(K): env.step(action[k])` loop (env.py:115-147 called K times,
 * e.g. examples/stanley_control.py:50-60 with the actions known in advance: action repeat, open-loop rollouts,
 * scripted policies).  Envs are independent, so no grid-wide synchronisation exists between steps.
 *   car_control: [K][N][2], maneuver: [K][N] (step k uses row k).
 *   Results are bit-identical to K calls of tc_step with the same flags: the bound buffers (tc_env_bind) hold the
 *   state and the outputs of step K-1 afterwards (status included: the TC_S_* bits of step K-1 only -- the per-step
 *   bits are in rollout->status); TC_F_AUTORESET re-spawns and fused terms (tc_env_set_terms) act per step exactly
 *   as there.
 *   rollout (may be NULL): per-step copies of everything env.step() returns (env.py:83-85,131-147), each member
 *   [K][N] (shapes below) or NULL.  With rollout->obs the observation of step k goes to rollout->obs[k] and the
 *   bound obs buffer is left untouched; without it every step stores its observation into the bound buffer (which
 *   ends up holding the last).
 * What is launched (tc_env_launch_info reports it):
 *   - no observation wanted: ONE launch of tc_env_kernel, one wavefront per env looping over the K steps with the
 *     env's state parked in LDS.
 *   - observations into rollout->obs (every step's frame wanted), STREAMED -- the default: per call (per segment of
 *     128 steps of a longer call) ONE simulate launch on the caller's stream -- tc_envg_kernel: 8 lanes per env, 8 envs
 *     per wavefront, state in registers, looping over the steps and leaving one 128-byte pose row (camera.py:62) per
 *     (step, env) -- and, on an internal stream, ONE frame launch that starts at once and runs BESIDE it --
 *     tc_frame_kernel: one workgroup per (step, env), camera stage + raster stage + the observation store; a workgroup
 *     first polls its pose row with device-scope loads until the simulate launch has written it (each of the twelve
 *     entries validates itself: a row is "not written yet" while any entry holds an all-ones NaN, and the frame
 *     workgroup puts that pattern back when it is done).  Only the call's first step is exposed, and the chip drains
 *     once per call instead of once per chunk.  Around the two launches, on the internal stream: tc_order_kernel
 *     (heaviest frames first, see TC_FRAME_ORDER), tc_gate_kernel, one wavefront that holds the frame launch back until
 *     every simulate workgroup has started, so the frame workgroups can fill the chip without keeping their producers
 *     off it, and, behind the simulate launch, tc_frame_recover_kernel.  EVERY wait on the device is bounded
 *     (TC_STREAM_WAIT_US, default 5000): a frame workgroup whose wait runs out marks its frame skipped, tells the others
 *     to stop waiting and leaves, and the recover kernel -- one workgroup per env, normally one look at the call's
 *     rows and out -- draws the skipped frames from the then complete rows.  The result therefore never depends on
 *     how the two launches were scheduled, only the time does.  The internal stream is joined back into the caller's
 *     before the call's work there ends, so everything completes in stream order.
 *   - the same, CHUNKED (TC_STREAM=0, and the form of calls without rollout->obs, where only the last step's frame
 *     is drawn): the steps are issued in chunks of at most 16 steps (a quarter of the call if that is less).  Per
 *     chunk a simulate launch (tc_envg_kernel; the first chunk of a multi-chunk call goes through tc_env_kernel: short
 *     rather than cheap, nothing overlaps it) and a frame launch (tc_frame_kernel, pose rows complete: no polling)
 *     on an internal stream behind it, so chunk c+1 is simulated while chunk c is drawn.  Calls whose chunks are
 *     shorter than 8 steps alternate their frame launches between two internal streams.
 *   - maps whose largest lane-line layer exceeds 576 nodes / edges (K = 13 variant) and TC_FUSE=0: the camera stage
 *     runs inside the simulate launch and tc_raster_kernel draws the frames.
 * The pose rows and draw lists in flight live in library-owned scratch sized by tc_env_reserve_steps, which must have
 * been called once before the first K-step call that renders (n_steps > 1 with an observation): tc_step_multi itself
 * never allocates and never waits for the device; without the scratch it returns TC_E_INVALID.
 * Env vars (all result-neutral, read at tc_env_create): TC_STREAM=0 chunked form; TC_STREAM_WAIT_US=t bound of a frame
 * workgroup's wait; TC_STREAM_SCRATCH_MB=m budget of the streamed form's scratch (default 16384: the rows of a segment
 * are cut to fit, tc_env_reserve_steps); TC_STREAM_TEST_SKIP=m (tests) frames with (step + env) % m == 0 are left to the recover kernel;
 * TC_CHUNK=n steps per chunk (0: chunks follow each other on the caller's stream, no overlap, no streaming),
 * TC_ENV_GROUPED=0 one wavefront per env in every simulate launch (no overlap, no streaming),
 * TC_FIRST_CHUNK_PER_ENV=0, TC_FRAME_STREAMS=1 (chunked form), TC_ENVG_MAP_LDS=0, TC_MULTI_SPLIT=0 a single fused launch
 * in which the same wavefront simulates its env and rasterises each of its frames, TC_SEG_LDS=0 / TC_SEG_LDS_CAP=n draw
 * lists through global memory only / beyond the first n segments, TC_FRAME_ORDER=0 frame workgroups in env order (default:
 * the envs whose last frame had the longest draw list first, so that a dispatch ends with its cheapest frames),
 * TC_STEP_ORDER=n (tc_step: the envs are re-dealt to the workgroups every n-th step so that heavy and light frames share
 * a SIMD, default 8; 0 = workgroup w works on env w).
 * The env's laneline_distances / nearest_edge buffers hold the call's last step; per-step values come from the rollout's
 * rows (TC_INFO_EVERY_STEP=1: every step computes them, also where neither rows nor a lane-line term read them). */
typedef struct {
  uint8_t* obs;          /* [K][N][tc_env_obs_bytes] */
  double* reward;        /* [K][N] */
  uint8_t* terminated;   /* [K][N] */
  uint8_t* truncated;    /* [K][N] */
  double* cte;           /* [K][N] */
  double* heading_error; /* [K][N] */
  /* --- ABI 5: the rest of env.step()'s info dict (env.py:83-85) and the status bits, per step */
  int32_t* status;             /* [K][N] TC_S_* bits raised in step k */
  double *x, *y, *theta;       /* [K][N] info["position"], info["orientation"] (state after step k) */
  double* velocity;            /* [K][N] car velocity after step k (info["velocity"] is this, or 0 while lp_len < 2) */
  double* laneline_distances;  /* [K][N][n_layers] */
  int32_t* nearest_edge;       /* [K][N][n_layers] */
  int32_t* local_path;         /* [K][N][8] */
  int32_t* lp_len;             /* [K][N] */
} tc_rollout;
/* The per-step rows of a call's per-episode features: like the members of tc_rollout they are arguments of ONE tc_step_multi
 * call, [n_rows][N] on the device, caller owned, each may be NULL, and step k of the call reads / writes row k.  n_rows is
 * the one capacity of all of them.  The library keeps none of the pointers beyond the launches the call enqueues; tc_step
 * and tc_reset have no rows.  `_in` is read, `_out` is written.  tc_step_multi returns TC_E_INVALID, before any device work
 * and without allocating or waiting: for n_rows < 0, a pointer set with n_rows < 1, n_steps > n_rows while a pointer is set,
 * steer_noise_in / steer_out without a controller, maneuver_out / ou_noise_out without drive randomisation,
 * episode_*_out without episode buffers, camera_out without a camera bank. */
typedef struct {
  int32_t n_rows;
  const double* steer_noise_in; /* tc_env_set_controller: added to the command of step k */
  double* steer_out;            /* the command BEFORE any noise (the IL label, train_stanley_il.py:73) */
  int32_t* maneuver_out;        /* tc_env_set_drive_randomization: the maneuver in force */
  double* ou_noise_out;         /* the OU value applied */
  int32_t* episode_length_out;  /* tc_env_set_episodes: length / ret after the step */
  double* episode_return_out;
  int32_t* camera_out;          /* tc_env_set_camera_bank: the camera index in force */
} tc_step_rows;
int tc_step_multi(tc_env* env, const void* car_control, int32_t control_dtype, const int32_t* maneuver, int32_t n_steps,
                  uint32_t flags, const tc_rollout* rollout, const tc_step_rows* rows /* may be NULL */, void* stream);

/* Sizes the scratch of K-step calls that render observations, for calls of up to max_call_steps steps: per (step, env)
 * a pose row (128 B), a draw-list length and room for a draw list (20 B x lane-line edges of the map; only a frame's
 * overflow beyond the LDS-resident head travels through it).  Streamed form: min(max_call_steps, 128) steps x N envs, fewer when that would exceed TC_STREAM_SCRATCH_MB (16 GiB)
 * (cfg3: 22 MB per step); chunked form: a ring of TC_RING_SLOTS (3) chunks of min(max_call_steps, 16 or TC_CHUNK) steps.
 * A call of ANY n_steps then runs in segments / chunks that fit.  Re-allocating waits for the device first (an earlier
 * launch may still use the old arrays); a request the current scratch already covers returns at once.
 * max_call_steps < 1 is TC_E_INVALID. */
int tc_env_reserve_steps(tc_env* env, int32_t max_call_steps);

/* What the library launches for a call of n_steps steps (1 = tc_step) with the current settings -- for benchmark
 * labels, not for control flow: fused = 1 when simulate + raster run as one kernel; kvar = register-cache variant of
 * the simulate stage (5, 8, 9, 13); steps_per_dispatch = steps one kernel dispatch of the call covers when every
 * step's frame goes to a rollout (the whole call when it is streamed, else a chunk: see tc_step_multi); name receives the
 * kernel symbols ("tc_step_kernel", "tc_envg_kernel+tc_frame_kernel", "tc_env_kernel+tc_raster_kernel", "tc_env_kernel";
 * with a controller installed the tc_drive_* entry points: "tc_drive_step_kernel", "tc_drive_envg_kernel+tc_frame_kernel", ...),
 * at most name_cap bytes including the terminator. */
int tc_env_launch_info(const tc_env* env, uint32_t flags, int32_t n_steps, int32_t* fused, int32_t* kvar,
                       int32_t* steps_per_dispatch, char* name, int32_t name_cap);

/* The LDS plan of the handle's frame kernel (tc_frame_kernel: one workgroup per (step, env) frame of a K-step call), for
 * benchmark labels and tests: lds_bytes = dynamic LDS per workgroup; head_entries = draw-list entries that stay in LDS
 * between the camera and the raster stage (longer lists take the overflow path through the global array);
 * workgroups_per_cu = what the runtime computes for that kernel and that LDS size
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor: registers and LDS together; nothing is launched); bits_offset = where
 * that kernel's raster stage puts its bit-planes: behind the tables of the handle's outline form (the K = 5 kernel with
 * batches of 32) or behind full-size tables of the kernel's own batch size.  Any pointer may be NULL.  Handles
 * whose K-step calls never run the frame kernel (kvar 13) report the plan all the same, with workgroups_per_cu = 0. */
int tc_env_frame_lds_info(const tc_env* env, int32_t* lds_bytes, int32_t* head_entries, int32_t* workgroups_per_cu,
                          int32_t* bits_offset);

/* The LDS of a workgroup of the grouped simulate launch of a K-step call (tc_envg_kernel / tc_drive_envg_kernel, the variant
 * of the features installed on the handle), which in a streamed call shares its CU with the frame workgroups for most of
 * the call.  info_every != 0: a call whose every step computes the lane-line distances (a rollout with laneline_distances /
 * nearest_edge rows; an installed lane-line term or TC_INFO_EVERY_STEP=1 make every call such a call) -- the launch then
 * holds the lane-line edge records in LDS (map_in_lds = 1) where the map allows it; otherwise only a launch's last step
 * reads them, from global memory.  dynamic_bytes = what the launch asks for, static_bytes = the kernel's own,
 * workgroups = of a launch over the handle's envs, frames_beside = frame workgroups (tc_env_frame_lds_info's lds_bytes,
 * granted in steps of 1280 bytes) that fit a CU's 160 KB beside one simulate workgroup; 0 for handles without a frame
 * kernel.  The figures are the launch's own plan; nothing is launched.  Any pointer may be NULL. */
int tc_env_envg_lds_info(const tc_env* env, int32_t info_every, int32_t* dynamic_bytes, int32_t* static_bytes,
                         int32_t* workgroups, int32_t* frames_beside, int32_t* map_in_lds);

/* The raster bands of the handle's frames: a frame whose bit-planes do not fit the LDS budget of one band (TC_BAND_BYTES) is
 * rasterised in n_bands bands of band_rows rows (the last one shorter).  n_bands == 1 is every bundled config at the
 * benchmark resolutions up to 128 x 128; the K = 5 frame kernel with batches of 32 then runs its one-band form, and
 * tc_frame_banded otherwise.  Either pointer may be NULL. */
int tc_env_frame_bands(const tc_env* env, int32_t* n_bands, int32_t* band_rows);

/* Workload descriptor for benchmark lines -- what the most recent frames drew: mean / max length of the frames' draw
 * lists (segments handed to cv2.polylines, camera.py:95-106) and the fraction of frames with none, over the N frames of
 * the last tc_step or, of the last tc_step_multi call, the frames of its last (up to 48) steps.  Waits for the device. */
int tc_env_draw_list_stats(tc_env* env, double* mean_segments, double* empty_frac, int32_t* max_segments, int64_t* frames);

/* Renderer.render_camera_frame_{rgb,classes} alone (renderer.py:36-51): rasterise caller-provided segment lists
 * into the bound observation tensor.  segments: device int32 [N][capacity][5] rows of (layer, x0, y0, x1, y1) --
 * the np.int32 end points handed to cv2.polylines; counts: device int32 [N], each <= capacity. */
int tc_render_segments(tc_env* env, const int32_t* segments, const int32_t* counts, int32_t capacity, void* stream);

/* Re-render the observation of the current state without stepping (Camera.capture_frame, camera.py:52). */
int tc_render(tc_env* env, uint32_t flags, void* stream);

/* Deferred frames: observations drawn from STORED poses, without the simulate stage and without touching the env.  A frame
 * depends on the env's state only through (x, y, theta) and the camera, so the x / y / theta rows of a rollout (28 bytes per
 * step with a camera index) are enough to draw any step's frame later -- only the rows a learner keeps, a replay sample, a
 * handful of envs of a long call -- bit for bit what the call that produced the poses drew or would have drawn.
 *
 * tc_render_poses draws n_frames frames with the handle's own camera settings (resolution, format, thickness, max_range,
 * packing); output frame m is at out + m * tc_env_obs_bytes and is what Camera.capture_frame (camera.py:52) gives for a car
 * at element j = index ? index[m] : m of the arrays.  x, y, theta and camera are device arrays of n_src elements -- for
 * instance the [K][N] rows of a tc_rollout --, index a device int64 array of n_frames elements (repeats and any order
 * allowed) or NULL, then n_frames <= n_src.  An index outside [0, n_src) is clamped into it and a camera value into the
 * camera rows: nothing is read or written out of bounds whatever the integers hold.
 *   camera: NULL on a handle with the one shared camera; required on a handle with per-env cameras
 *     (tc_env_set_camera_per_env), where it is the env whose camera the frame takes; required on a handle with a camera bank
 *     (tc_env_set_camera_bank), where it is the bank index: the camera_out rows of the call that produced the poses.
 *   noise: the fused observation noise of tc_env_set_noise is NOT applied -- a deferred frame has no place in the blob stream.
 * Everything is enqueued on `stream`, in stream order, into a scratch of the call's own: the bound obs tensor, the env's
 * state, the noise counter, the profile ring, the scratch of K-step calls and what tc_env_draw_list_stats reports are not
 * touched (also on handles without a frame kernel, whose frames are drawn by the simulate kernel's camera stage in its render
 * mode with tc_raster_kernel behind it, in rounds of N frames -- those handles must be bound), and every later call on the
 * handle gives bit for bit what it would have given without the render.  Renders on one handle share that scratch: the caller
 * keeps them in one stream's order (one stream, or its own events).  After tc_env_reserve_poses the call neither allocates nor synchronises and can be
 * captured into a HIP graph; without a reservation it returns TC_E_INVALID (tc_last_error names tc_env_reserve_poses), the rule
 * tc_step_multi has for tc_env_reserve_steps.  n_frames == 0 is TC_OK without a launch.
 * TC_E_INVALID before any HIP call: NULL env / x / y / theta / out, n_src < 1, n_frames < 0, index == NULL with
 * n_frames > n_src, camera given on a shared-camera handle or missing on the other two kinds, a misaligned pointer (out: 16
 * bytes, as the obs rows of a rollout; x, y, theta, index: 8; camera: 4).
 *
 * tc_env_reserve_poses sizes that scratch for launches of up to max_frames frames; a longer list runs as several launches
 * one after the other.  Per frame: a pose row (128 B), a draw-list length (4 B) and room for a draw list (20 B x lane-line
 * edges of the map; only a frame's overflow beyond the LDS-resident head travels through it) -- simple_layout 5.4 KB,
 * knuffingen 15 KB --, cut to the budget TC_STREAM_SCRATCH_MB.  Handles without a frame kernel keep N draw lists and N
 * gathered poses whatever max_frames is.  Waits for the device only when it has to re-allocate; a request the scratch already
 * covers returns at once.  max_frames < 1 is TC_E_INVALID. */
int tc_env_reserve_poses(tc_env* env, int64_t max_frames);
int tc_render_poses(tc_env* env, const double* x, const double* y, const double* theta, const int32_t* camera,
                    const int64_t* index, int64_t n_src, int64_t n_frames, uint8_t* out, void* stream);

/* Expands bit-packed class masks (TC_FMT_CLASSES_BITS) on the device; needs no env handle.  A "frame" is planes*H*W/8 packed
 * bytes -- the rows of a [K][N] rollout are simply K*N frames.  dst: [n_out][planes][H][W] of dst_dtype: TC_U8 gives 0 / 255,
 * bit-identical to what TC_FMT_CLASSES would have written; TC_F16, TC_BF16 and TC_F32 give 0.0 / 1.0, which is the consumers'
 * pre_obs(obs) = obs / 255 (examples/benchmark_tinycar_net.py:20: 255 / 255 is exactly 1.0 in each of them).
 *   index = NULL: output frame j is source frame j (n_out <= n_src_frames).
 *   else: device int64 [n_out]; output frame j is source frame index[j] -- a replay-buffer sample (examples/rl_utils.py),
 *     repeats allowed, any order.  An index outside [0, n_src_frames) yields a frame of zeros; nothing is read out of bounds.
 * packed, index and dst are device pointers; packed must be 4-byte and dst 16-byte aligned.  One launch on `stream`; neither
 * allocates nor synchronises and can be captured into a HIP graph.  n_out = 0 is TC_OK without a launch.
 * TC_E_INVALID, before any HIP call: NULL packed or dst, W % 32 != 0, a non-positive size, an unknown dtype, n_out < 0,
 * index == NULL with n_out > n_src_frames, a misaligned pointer. */
int tc_unpack_bits(const uint8_t* packed, int64_t n_src_frames, int32_t planes, int32_t H, int32_t W, const int64_t* index,
                   int64_t n_out, void* dst, int32_t dst_dtype, void* stream);

/* Sample buffer: turns the [K][N] rows of one K-step call into dataset samples on the device -- the Xn / Mn / Yn fill of
 * examples/train_stanley_il.py:61-77,100-110 and Replaybuffer.add of examples/rl_utils.py:13-30.  Needs no env handle.
 * The executable definition is collect_reference of tinycarlo_amd/collect.py; tinycarlo_amd/csrc/tc_collect.h holds the rules.
 *
 * Per env n the caller keeps pending[n] (u8: the env's next row is a re-spawn row), age[n] (i32: action steps of the
 * running episode) and last[n] (one frame: the observation the next action is computed from).  Rows are visited k outer,
 * n inner:
 *   1. pending[n]: a re-spawn row (TC_F_AUTORESET applied no action): no sample, age[n] = 0.
 *   2. else i = age[n]++; if i % stride == 0 the row is a candidate: obs = last[n], next_obs = obs_rows[k][n], env = n and
 *      every column's value of (k, n).
 *   3. pending[n] = terminated[k][n] | truncated[k][n] (either may be NULL), last[n] = obs_rows[k][n].
 * Candidates take ordinals counters[TC_COLLECT_NEXT], +1, ... in visiting order.  Ordinal o < capacity goes to slot o; beyond
 * that TC_COLLECT_STOP drops it (and counts it), TC_COLLECT_RING takes slot o % capacity, TC_COLLECT_RANDOM the counter-based
 * draw of tc_rng.h (sub-stream "rep" of `seed`, ordinal o).  Where candidates of one call share a slot the highest ordinal
 * wins, as in a sequential loop; ordinal[slot] records what a slot holds (-1 = empty; the caller initialises it).
 *
 * A frame is frame_bytes opaque bytes (packed bits, byte class masks, rgb), frame_bytes % 4 == 0; copies move 16 bytes per
 * lane when frame_bytes % 16 == 0 and obs, next_obs, last and obs_rows are 16-byte aligned, 4 bytes otherwise.
 * Every pointer is a device pointer.  counters: int64[4] = filled slots, next ordinal, dropped, candidates of the last call.
 * scratch: at least tc_collect_scratch_bytes bytes for (n_rows, num_envs), 16-byte aligned, contents free between calls.
 * Neither allocates nor synchronises: everything is enqueued on `stream` in order, every counter lives on the device, and
 * the call can be captured into a HIP graph (a replay advances the buffer like a fresh call over the rows' contents).
 * TC_E_INVALID with tc_last_error() text, before any HIP call: a NULL required pointer, a non-positive size, stride < 1,
 * frame_bytes % 4 != 0, a misaligned pointer, an element size not in {1, 4, 8}, more than TC_COLLECT_MAX_COLUMNS columns, an
 * unknown mode, capacity >= 2^32 with TC_COLLECT_RANDOM, n_rows * num_envs >= 2^26 (the copy launch
 * runs one wavefront per (row, env)), a scratch that is too small. */
#define TC_COLLECT_STOP 0
#define TC_COLLECT_RING 1
#define TC_COLLECT_RANDOM 2
#define TC_COLLECT_MAX_COLUMNS 8
#define TC_COLLECT_COUNT 0     /* indices into the counter block */
#define TC_COLLECT_NEXT 1
#define TC_COLLECT_DROPPED 2
#define TC_COLLECT_LAST_CALL 3
typedef struct {
  const void* src;   /* [n_rows][num_envs] elements of this call */
  void* dst;         /* [capacity] elements */
  int32_t elem_size; /* 1, 4 or 8 bytes; src and dst aligned to it */
  int32_t reserved;
} tc_collect_column;
typedef struct {
  int64_t capacity;
  int32_t num_envs;
  int32_t stride;
  int32_t mode; /* TC_COLLECT_* */
  int32_t n_columns;
  uint64_t seed;
  int64_t frame_bytes;
  uint8_t* obs;      /* [capacity][frame_bytes] */
  uint8_t* next_obs; /* likewise, or NULL */
  int64_t* ordinal;  /* [capacity] */
  int32_t* env;      /* [capacity] */
  tc_collect_column columns[TC_COLLECT_MAX_COLUMNS];
  uint8_t* pending; /* [num_envs] */
  int32_t* age;     /* [num_envs] */
  uint8_t* last;    /* [num_envs][frame_bytes] */
  int64_t* counters;
  void* scratch;
  int64_t scratch_bytes;
} tc_collect_desc;
int64_t tc_collect_scratch_bytes(int32_t n_rows, int32_t num_envs);
int tc_collect(const tc_collect_desc* desc, int32_t n_rows, const uint8_t* obs_rows, const uint8_t* terminated,
               const uint8_t* truncated, void* stream);

/* Frame histories over the sample buffer (TC_HAS_HISTORY): a sample of ReplaybufferTemporal (examples/rl_utils.py:32-57) is
 * what the env showed over the last T steps of the episode, newest first (examples/train_td3.py:164,175-176).  The buffer
 * keeps one frame per slot plus one link: prev[slot] = ordinal of the sample that precedes the slot's in its episode (-1:
 * none), and per env chain[n] = ordinal of the env's most recent candidate of the running episode (-1: none; the caller
 * sets chain to -1 where it sets age to 0).  Rules: tc_collect.h (tc_collect_chain_step, tc_history_walk); definition:
 * collect_reference / history_reference of tinycarlo_amd/collect.py.
 *
 * tc_collect_link: call it BEFORE tc_collect, on the same stream, with the same descriptor, n_rows and done rows.  It reads
 * pending, age and counters[TC_COLLECT_NEXT] without changing them, repeats the scan and the rank into desc->scratch (which
 * tc_collect overwrites afterwards) and then, one thread per env, walks the rows: a re-spawn row sets chain[n] = -1, a
 * candidate with ordinal o gets link_rows[k][n] = chain[n] and sets chain[n] = o, written or not; every other entry of
 * link_rows becomes -1.  Hand link_rows to tc_collect as an 8-byte column whose dst is prev: prev[slot] is then written
 * under exactly the condition under which the slot's frame, env and ordinal are, so a buffer with links has at most
 * TC_COLLECT_MAX_COLUMNS - 1 columns of its own.  desc->columns is not looked at here.  chain: device int64 [num_envs];
 * link_rows: device int64 [n_rows][num_envs].  Three launches; neither allocates nor synchronises; can be captured.
 * TC_E_INVALID before any HIP call: what tc_collect refuses about the fields used here, a NULL or misaligned chain / link_rows. */
int tc_collect_link(const tc_collect_desc* desc, int32_t n_rows, const uint8_t* terminated, const uint8_t* truncated,
                    int64_t* chain, int64_t* link_rows, void* stream);

/* The histories of n_index slots: slots[b][0] = index[b], slots[b][t] = the slot of the sample t steps before it, as far
 * as the links lead: the walk stops where the episode started (prev < 0) or where the predecessor was dropped or
 * overwritten (the slot of ordinal prev is -1 or holds another ordinal).  valid[b] = entries found; the rest is -1
 * (TC_PAD_ZERO) or the last slot found (TC_PAD_EDGE).  An index outside [0, capacity) or an empty slot gives valid = 0 and
 * -1 throughout.  next_slots (or NULL): [b][0] = slots[b][0], [b][t] = slots[b][t-1] -- with tc_gather_frames' second
 * source the next-history x1 = queue[:-1] against x = queue[1:].  mode, seed, capacity: the buffer's.  index, slots,
 * next_slots: device int64 [n_index], [n_index][T]; valid: device int32 [n_index].  One launch, one thread per sample.
 * TC_E_INVALID before any HIP call: a NULL or misaligned pointer, capacity < 1, T < 1, n_index < 0, an unknown mode or pad,
 * capacity >= 2^32 with TC_COLLECT_RANDOM.  n_index = 0 is TC_OK without a launch. */
#define TC_PAD_ZERO 0
#define TC_PAD_EDGE 1
int tc_history_resolve(const int64_t* prev, const int64_t* ordinal, int64_t capacity, int32_t mode, uint64_t seed,
                       const int64_t* index, int64_t n_index, int32_t T, int32_t pad, int64_t* slots, int64_t* next_slots,
                       int32_t* valid, void* stream);

/* Byte frames gathered by index into the dtype the consumer wants: dst [n_out][frame_bytes] elements of dst_dtype, output
 * frame j = frame index[j] of src -- or of src2, where src2 is given and j % group == 0.  TC_U8 copies; TC_F16, TC_BF16 and
 * TC_F32 give float(v) * (1.0f / 255.0f) rounded once to the dtype: what torch's device kernel computes for
 * frames.to(dtype) / 255 (a division by a scalar is a product with the float reciprocal there), bit for bit.
 * An index outside [0, n_src_frames) yields zeros and reads nothing.  Each lane owns one 16-byte store and takes its 16 /
 * 8 / 4 source bytes with one load when frame_bytes and src (src2) are multiples of that; otherwise lanes move 4 source
 * bytes each (frame_bytes % 4 == 0, src 4-byte aligned).  dst is 16-byte aligned.  One launch; neither allocates nor
 * synchronises; can be captured.  TC_E_INVALID before any HIP call: NULL src, index or dst, non-positive n_src_frames or
 * frame_bytes, frame_bytes % 4 != 0, n_out < 0, group < 1 with src2, an unknown dtype, a misaligned pointer. */
int tc_gather_frames(const uint8_t* src, const uint8_t* src2, int64_t n_src_frames, int64_t frame_bytes, const int64_t* index,
                     int64_t n_out, int64_t group, void* dst, int32_t dst_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TINYCARLO_HIP_H */
