#!/usr/bin/env python3
"""Cost of the camera images (k_render through QuadrupedVecEnv.render_tensor -> qs_render): HIP events around back-to-back renders for the
kernel time, wall time for the end-to-end calls.  Three shapes: one 1440 x 1080 frame (plus QuadrupedGymEnv.render() end to end, which
includes the copy of the frame to the host), 64 x 320 x 240, and 4096 x 64 x 64 (a vision learner's batch).

    python tools/time_render.py [--out FILE]       # prints one JSON line; --out also writes it to FILE (profiles/render_cost.json)
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "quadruped-springs_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

KW = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, enable_action_filter=True, noise=False, seed=1)


def kernel_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def batch(n, w, h, reps):
    from qs_amd.vec_env import QuadrupedVecEnv
    v = QuadrupedVecEnv(num_envs=n, auto_reset=False, **KW)
    v.reset_tensor()
    act = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (n, v.action_dim)).astype(np.float32)).cuda()
    for _ in range(20):              # robots in the air, legs moving: the images hold robots and shadows
        v.step_tensor(act)
    fn = lambda: v.render_tensor(width=w, height=h)  # noqa: E731
    ms = kernel_ms(fn, reps)
    r = dict(images=n, width=w, height=h, kernel_ms=round(ms, 4), rays_per_s=round(n * w * h / (ms * 1e-3)), wall_ms_render_tensor=round(wall_ms(fn, reps), 4))
    fn_d = lambda: v.render_tensor(width=w, height=h, depth=True, segmentation=True)  # noqa: E731
    r["kernel_ms_with_depth_and_segmentation"] = round(kernel_ms(fn_d, reps), 4)
    v.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    from qs_amd import lib
    from qs_amd.env.quadruped_gym_env import QuadrupedGymEnv
    res = dict(device=torch.cuda.get_device_name(0), library=lib.load().qs_version().decode())
    res["frame_1440x1080"] = batch(1, 1440, 1080, 50)
    env = QuadrupedGymEnv(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, seed=1, noise=False)
    env.reset()
    res["frame_1440x1080"]["wall_ms_gym_env_render"] = round(wall_ms(env.render, 20), 3)
    env.close()
    res["batch_64x320x240"] = batch(64, 320, 240, 20)
    res["batch_4096x64x64"] = batch(4096, 64, 64, 20)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
