#!/usr/bin/env python3
"""What step_tensor(active=) costs and saves at the launch: HIP events around back-to-back steps of N standing robots under the zero action,
median and spread of the repeats, in one process, the cases alternating:
  - no mask (qs_step), and a mask of ones (the mask read is all that is added);
  - a mask of zeros: every wave leaves before the tile load (the settle lanes' workgroups and the solo waves' are still launched; the
    handle is one without auto-reset, as DeviceARS uses it, so the settle lanes have no work: with work a settle wave takes as long as
    an environments' wave whatever the mask says);
  - every other wave frozen, and every other environment frozen (no wave can leave early: frozen quads step the parked record).

    python tools/time_active_mask.py [--n 8192] [--out profiles/active_mask_launch.md]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch  # noqa: E402

from qs_amd import QuadrupedVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    env = QuadrupedVecEnv(num_envs=n, device=0, auto_reset=False, reset_lookahead=2, task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC",
                          action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                          env_randomizer_mode="GROUND_RANDOMIZER")
    env.reset_tensor()
    dev = env.device
    act = torch.zeros((n, env.action_dim), device=dev)
    idx = torch.arange(n, device=dev)
    masks = {"no mask": None, "mask of ones": torch.ones(n, dtype=torch.uint8, device=dev), "mask of zeros (all frozen)": torch.zeros(n, dtype=torch.uint8, device=dev),
             "every other wave frozen": ((idx // 16) % 2 == 0).to(torch.uint8), "every other environment frozen": (idx % 2 == 0).to(torch.uint8)}
    us = {k: [] for k in masks}
    for _ in range(50):
        env.step_tensor(act)
    for rep in range(args.repeats + 1):
        for name, m in masks.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                env.step_tensor(act, active=m)
            b.record()
            b.synchronize()
            if rep:                                   # (the first round warms every case up)
                us[name].append(a.elapsed_time(b) * 1e3 / args.steps)
    rare = env.counter("limit_path_substeps")
    lines = [f"`python tools/time_active_mask.py --n {n}`: {n} standing robots under the zero action (auto_reset=False, reset_lookahead=2: a parked record, settle lanes without work; "
             f"{rare} many-rows wave-substeps in the whole run), {args.steps} back-to-back steps between two HIP events, {args.repeats} alternating repeats; "
             "median (min - max) us per step.", "", "| case | us per step |", "|---|---|"]
    for name, v in us.items():
        lines.append(f"| {name} | {statistics.median(v):.1f} ({min(v):.1f} - {max(v):.1f}) |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    env.close()


if __name__ == "__main__":
    main()
