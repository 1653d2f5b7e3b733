#!/usr/bin/env python3
"""Roll a few environments of the jump-in-place task and write what the camera saw: one animated GIF per environment (PIL), or, without
PIL, one .npy of frames [T, H, W, 3] per environment.

    python examples/render_rollout.py [--envs 4] [--steps 60] [--camera CLASSIC] [--size 480 360] [--out render_out]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "quadruped-springs_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from qs_amd.render import CAMERA_MODES  # noqa: E402
from qs_amd.vec_env import QuadrupedVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--camera", default="CLASSIC", choices=sorted(CAMERA_MODES))
    ap.add_argument("--size", type=int, nargs=2, default=(480, 360), metavar=("W", "H"))
    ap.add_argument("--out", default="render_out")
    a = ap.parse_args()
    env = QuadrupedVecEnv(num_envs=a.envs, task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True,
                          enable_action_filter=True, auto_reset=False, seed=0, noise=False)
    env.reset_tensor()
    w, h = a.size
    rng = np.random.default_rng(0)
    frames = torch.empty((a.steps, a.envs, h, w, 3), dtype=torch.uint8, device=env.device)
    for k in range(a.steps):
        # a crude jump: crouch, then push off with all legs, then hold the landing pose
        phase = k % 40
        base = -1.0 if phase < 15 else (1.0 if phase < 22 else 0.0)
        act = np.clip(base + 0.1 * rng.normal(size=(a.envs, env.action_dim)), -1, 1).astype(np.float32)
        env.step_tensor(torch.from_numpy(act).to(env.device))
        rgb, _, _ = env.render_tensor(camera=a.camera, width=w, height=h)   # stays on the device
        frames[k].copy_(rgb)
    frames = frames.cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for e in range(a.envs):
        if Image is not None:
            imgs = [Image.fromarray(frames[k, e]) for k in range(a.steps)]
            path = os.path.join(a.out, f"env{e}.gif")
            imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=int(1000 * env.cfg.dt * env.cfg.action_repeat), loop=0)
        else:
            path = os.path.join(a.out, f"env{e}.npy")
            np.save(path, frames[:, e])
        print(path)
    env.close()


if __name__ == "__main__":
    main()
