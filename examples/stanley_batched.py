#!/usr/bin/env python3
"""The Stanley lateral controller of the reference's examples/stanley_control.py (k = 4, speed 0.4, steer =
(heading_error + atan2(k * cte, speed)) in units of max_steering_angle), for N cars at once and entirely on the GPU: the
controller reads cte / heading_error from the env's device tensors and writes the action tensor, the reference's
wrappers (CTE sparse reward, CTE and crash termination) run inside the step kernel, finished envs re-spawn on the device.

    python examples/stanley_batched.py [--envs 4096] [--steps 600] [--maneuver 3] [--randomize] [--max-episode-steps N] [--fused K [--packed] [--randomize-cameras] [--explore] [--collect CAP]]

--randomize: every episode of every env drives its own car, drawn on the device at the re-spawn (wheelbase, track width,
speed and steering limits within +-20 %), plus the steering shift of the reference's TD3 study (examples/train_td3.py:37,
146-147: STEERING_SHIFT = -0.01, here drawn per episode from [-0.01, 0]); the controller normalises its steering by each
env's own max_steering_angle, read from the live per-env rows (vec.env_car_params).

--max-episode-steps N: a controller that drives this well never ends an episode, so nothing would ever re-spawn (or draw
a new car).  The time limit truncates every episode after N steps inside the step kernel (starts staggered over the
envs); the episodes finished and their mean length / return are read from vec.episode_stats afterwards.

--fused K: the same run with the controller inside the simulate kernels (vec.set_controller): `drive` calls of K steps
each, one launch sequence per K steps instead of one per step plus the torch glue; the per-step rewards, cte and episode
ends come back in the call's rollout rows.  The default stays the torch loop below.

--packed (with --fused K): class-mask frames leave the kernels bit-packed (obs_packing="bits": uint8 [C, H, W/8], an eighth
of the bytes), and a sample of each call's rows is expanded on the device to float16 0.0 / 1.0 -- what a consumer that
trains on a batch of the rollout does (tinycarlo_amd.unpack_obs).

--randomize-cameras (with --fused K): every episode of every env looks through its own camera, as the data collection of the
reference's examples/train_stanley_il.py:53-57 does -- an integer pitch from [10, 20) and an integer fov from [90, 130),
here a bank of the 400 combinations from which each re-spawn draws on the device (vec.randomize_cameras); the index each
frame was drawn with comes back in the rollout's "camera" rows (vec.camera_bank_params[index]: pitch, roll, yaw, fov, position).
With --max-episode-steps, so that episodes end, this is that data collection entirely on the device.

--explore (with --fused K): the rest of that data collection (vec.randomize_drive) -- the maneuver is a per-episode quantity that
cycles through (0, 1, 3) at every re-spawn (train_stanley_il.py:105), and Ornstein-Uhlenbeck noise (theta 0.1, sigma 0.4,
carried across episodes, train_stanley_il.py:66) is added to the applied steering; the maneuver in force at each step comes
back in the rollout's "maneuver" rows (the Mn column), and the share of each among the collected frames is printed.

--collect CAP (with --fused K): the script's dataset itself (train_stanley_il.py:61-77, 100-110) -- a device sample buffer of CAP
samples (vec.make_sample_buffer) takes every call's rows: the frame before a step with that step's steering command and
maneuver, every SKIP_STEPS = 2nd action step of an episode, until the buffer is full (overflow="stop").  The maneuver column
exists only with --explore (without it the maneuver is the one constant of --maneuver and no rollout rows carry it: the buffer
then holds obs and steer).  Samples kept and dropped and, with --explore, the maneuver shares among the samples are printed.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tinycarlo_amd import TinyCarloVecEnv  # noqa: E402
from tinycarlo_amd.config import bundled_config  # noqa: E402
from tinycarlo_amd.wrapper import CrashTerminationWrapper, CTESparseRewardWrapper, CTETerminationWrapper  # noqa: E402


def run(num_envs=4096, steps=600, maneuver=3, k=4.0, speed=0.4, device="cuda:0", seed=2, randomize=False,
        max_episode_steps=None, fused=0, packed=False, randomize_cameras=False, explore=False, collect=0):
    config = bundled_config("config_simple_layout.yaml")
    if packed:  # packing is for class masks: the bundled config with that format
        if not fused:
            raise ValueError("--packed goes with --fused K (the frames of a rollout)")
        import yaml
        with open(config) as f:
            cfg = yaml.safe_load(f)
        cfg["sim"]["observation_space_format"] = "classes"
        cfg["map"]["json_path"] = os.path.join(os.path.dirname(config), cfg["map"]["json_path"])
        config = cfg
    vec = TinyCarloVecEnv(config, num_envs=num_envs, device=device, autoreset=True, spawn="device",
                          obs_packing="bits" if packed else None)
    if randomize:
        p = vec.car_params
        vec.randomize_cars({name: (0.8 * getattr(p, name), 1.2 * getattr(p, name))
                            for name in ("wheelbase", "track_width", "max_velocity", "max_steering_angle")}
                           | {"steering_shift": (-0.01, 0.0)}, seed=seed)
    if explore and not fused:
        raise ValueError("--explore goes with --fused K (the device's maneuvers and noise belong to the built-in controller)")
    if collect and not fused:
        raise ValueError("--collect goes with --fused K (the samples are taken from the rows of a call)")
    if randomize_cameras:
        if not fused:
            raise ValueError("--randomize-cameras goes with --fused K (the camera of a frame comes back in the rollout rows)")
        vec.randomize_cameras(orientation={"pitch": range(10, 20)}, fov=range(90, 130), seed=seed)
    env = CrashTerminationWrapper(CTETerminationWrapper(CTESparseRewardWrapper(vec, 0.01), 0.07, number_of_steps=5))
    if max_episode_steps:
        vec.set_time_limit(max_episode_steps)
    obs, info = env.reset(seed=seed)
    if max_episode_steps:  # staggered first episodes: the envs do not all reach the limit on the same step
        vec.episode_stats["length"].copy_((torch.arange(num_envs, device=device) * max_episode_steps // num_envs).to(torch.int32))
    max_steer = math.radians(vec.car_params.max_steering_angle)
    cc = torch.zeros((num_envs, 2), dtype=torch.float64, device=device)
    cc[:, 0] = speed
    man = torch.full((num_envs,), maneuver, dtype=torch.int32, device=device)
    ret = torch.zeros(num_envs, dtype=torch.float64, device=device)
    cte_abs = torch.zeros((), dtype=torch.float64, device=device)
    ended = torch.zeros((), dtype=torch.int64, device=device)
    if fused:
        vec.set_controller(k=k, speed=speed)
        if explore:  # the settings of train_stanley_il.py: maneuvers (0, 1, 3) in turn, OU noise that is never reset
            vec.randomize_drive(maneuvers=(0, 1, 3), mode="cycle", ou=dict(theta=0.1, mu=0.0, sigma=0.4, reset=False), seed=seed)
            # (the episodes under way were spawned before the feature came on: give them the maneuver episode 0 would have drawn)
            from tinycarlo_amd.randomization import draw_maneuver
            vec.episode_maneuver.copy_(torch.from_numpy(draw_maneuver(seed, range(num_envs), 0, (0, 1, 3), "cycle")))
            vec.drive_episode.fill_(1)
            man_frames = torch.zeros(4, dtype=torch.int64, device=device)
        calls = [min(fused, steps - s0) for s0 in range(0, steps, fused)]
        prepared = {}
        for n in set(calls):  # (a shorter last call has rows of its own)
            roll = vec.alloc_rollout(n, keys=("obs", "reward", "terminated", "truncated", "cte") + (("camera",) if randomize_cameras else ()) +
                                     (("maneuver",) if explore else ()) + (("steer",) if collect else ()))
            prepared[n] = (vec.prepare_drive(None if explore else man.expand(n, num_envs).contiguous(), roll), roll)
        if collect:  # the script's dataset: SKIP_STEPS = 2, stop at BUFFER_SIZE (without --explore the maneuver is one constant: no column)
            buf = vec.make_sample_buffer(collect, columns=("maneuver", "steer") if explore else ("steer",), stride=2, overflow="stop",
                                         max_rows=max(calls))
            buf.begin(vec.out["obs"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if fused:
        for n in calls:
            call, roll = prepared[n]
            call()                                                    # n closed-loop steps, frames into roll["obs"]
            if collect:
                buf.collect(roll)                                     # (obs before the step, maneuver, steer) samples, on the device
            ret += roll["reward"].sum(0)
            cte_abs += roll["cte"].abs().mean(1).sum()
            ended += (roll["terminated"] | roll["truncated"]).sum()
            if explore:
                man_frames += torch.bincount(roll["maneuver"].reshape(-1), minlength=4)[:4]
            if packed:  # a batch for the network: 256 random (step, env) rows of this call, float16 0.0 / 1.0
                batch_idx = torch.randint(0, n * num_envs, (256,), device=device)
                batch = vec.unpack_obs(roll["obs"], torch.float16, index=batch_idx)
    else:
        for _ in range(steps):
            cte, he = vec.out["cte"], vec.out["heading_error"]      # of the previous step, already on the device
            if randomize:  # this episode's car of every env (the rows change at each re-spawn)
                max_steer = torch.deg2rad(vec.env_car_params[:, 3])
            cc[:, 1] = (he + torch.atan2(k * cte, torch.full_like(cte, speed))) / max_steer
            vec.step_device(cc, man)                                  # one kernel: physics, tracking, camera, wrappers
            ret += vec.out["reward"]
            cte_abs += vec.out["cte"].abs().mean()
            ended += (vec.out["terminated"] | vec.out["truncated"]).sum()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"envs": num_envs, "steps": steps, "env_steps_per_s": num_envs * steps / dt,
           "mean_abs_cte_m": float(cte_abs) / steps, "episodes_ended": int(ended),
           "mean_reward_per_step": float(ret.mean()) / steps, "obs_shape": tuple(vec.out["obs"].shape)}
    if fused:
        out["steps_per_call"] = fused
    if packed:
        out["batch"] = (tuple(batch.shape), str(batch.dtype))
    if randomize:
        out["car_episodes_drawn"] = int(vec.car_episode.sum())
    if randomize_cameras:
        out.update(cameras_in_bank=len(vec.camera_bank_params), camera_episodes_drawn=int(vec.camera_episode.sum()),
                   cameras_in_last_call=int(roll["camera"].unique().numel()))
    if explore:
        tot = max(int(man_frames.sum()), 1)
        out.update(maneuver_share={m: round(int(man_frames[m]) / tot, 4) for m in range(4) if int(man_frames[m])},
                   maneuver_episodes_drawn=int(vec.drive_episode.sum()), normals_consumed=int(vec.ou_draws.sum()))
    if collect:
        kept = len(buf)
        out.update(samples_kept=kept, samples_dropped=buf.dropped, sample_buffer_full=buf.full)
        if explore and kept:
            share = torch.bincount(buf.cols["maneuver"][:kept].long(), minlength=4)[:4]
            out["sample_maneuver_share"] = {m: round(int(share[m]) / kept, 4) for m in range(4) if int(share[m])}
    if max_episode_steps:
        es = vec.episode_stats
        n_ep = int(es["count"].sum())
        out.update(episodes_finished=n_ep, mean_episode_length=float(es["length_sum"].sum()) / max(n_ep, 1),
                   mean_episode_return=float(es["return_sum"].sum()) / max(n_ep, 1))
    vec.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--maneuver", type=int, default=3)
    ap.add_argument("--randomize", action="store_true", help="per-episode car constants and steering shift")
    ap.add_argument("--max-episode-steps", type=int, default=None, help="time limit per episode (kept by the step kernel)")
    ap.add_argument("--fused", type=int, default=0, metavar="K", help="built-in controller: drive() calls of K steps")
    ap.add_argument("--packed", action="store_true", help="with --fused: bit-packed class-mask frames, unpacked in batches")
    ap.add_argument("--randomize-cameras", action="store_true", help="with --fused: per-episode pitch / fov from a 400-camera bank")
    ap.add_argument("--explore", action="store_true", help="with --fused: per-episode maneuvers (0, 1, 3) in turn and OU steering noise")
    ap.add_argument("--collect", type=int, default=0, metavar="CAP", help="with --fused: a device sample buffer of CAP (obs, maneuver, steer) samples")
    a = ap.parse_args()
    print(run(a.envs, a.steps, a.maneuver, randomize=a.randomize, max_episode_steps=a.max_episode_steps, fused=a.fused,
              packed=a.packed, randomize_cameras=a.randomize_cameras, explore=a.explore, collect=a.collect))
