#!/usr/bin/env python3
"""Predictive sampling on JUMPING_IN_PLACE with device forks: M real robots, C candidates each, all in one handle of M x (1 + C) environments.
Per control step: ONE fork copies every real robot into its C candidates; H step_tensor calls roll the candidates out under action
sequences sampled around the previous plan (candidate 0 runs the plan itself); the real robots, which stepped along, go back to where
they were (a masked restore of a masked snapshot); then the first action of each robot's best candidate is the one step the real robot
takes, and the rest of that sequence is the next plan.  Prints the real robots' mean return (the rewards of their first episode, plus the task's end-of-episode reward for
the state they are in if it has not ended: get_info("reward_end")) against the same loop with C = 1 (no
sampling: the plan is never improved).  Nothing leaves the GPU inside a control step.
--freeze-done: a candidate whose episode has ended is not rolled out to the horizon (step_tensor(active=)); the scores ignore it from
there on anyway, so the result printed is the same.

    python examples/mpc.py [--robots 64] [--candidates 63] [--horizon 12] [--steps 150] [--sigma 0.5] [--freeze-done]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch

from qs_amd import QuadrupedVecEnv


def run(M, C, H, steps, sigma, seed, freeze_done=False):
    n = M * (1 + C)
    env = QuadrupedVecEnv(num_envs=n, device=0, auto_reset=True, task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC",
                          action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                          env_randomizer_mode="GROUND_RANDOMIZER", noise=False, seed=seed)
    dev, d = env.device, env.action_dim
    gen = torch.Generator(device=dev).manual_seed(seed)
    # environments [0, M) are the real robots; candidate c of robot m is environment M + m * C + c
    real = torch.arange(M, device=dev)
    src_of = torch.cat([torch.full((M,), -1, device=dev), real.repeat_interleave(C)]).to(torch.int32)
    real_mask = torch.zeros(n, dtype=torch.bool, device=dev)
    real_mask[:M] = True
    env.reset_tensor()
    keep = env.snapshot(indices=real_mask)
    plan = torch.zeros((M, H, d), device=dev)
    actions = torch.zeros((n, d), device=dev)
    ret = torch.zeros(M, device=dev)
    alive = torch.ones(M, dtype=torch.bool, device=dev)
    active = torch.ones(n, dtype=torch.bool, device=dev)           # --freeze-done: the real robots, and the candidates still in their episode
    for _ in range(steps):
        env.fork(src_of=src_of)
        env.snapshot(indices=real_mask, out=keep)
        seq = plan[:, None] + sigma * torch.randn((M, C, H, d), generator=gen, device=dev)
        seq[:, 0] = plan                                            # candidate 0: the plan as it stands
        seq = seq.clamp_(-1.0, 1.0).view(M * C, H, d)
        score = torch.zeros(M * C, device=dev)
        running = torch.ones(M * C, dtype=torch.bool, device=dev)
        for h in range(H):
            actions[M:] = seq[:, h]
            if freeze_done:
                active[M:] = running
                _, rew, done, _ = env.step_tensor(actions, active=active)
            else:
                _, rew, done, _ = env.step_tensor(actions)
            score += rew[M:] * running
            running &= ~done[M:].bool()
        # the task pays at the end of the episode: a candidate still in its episode at the horizon is worth what the task would pay there
        score += env.get_info("reward_end")[M:, 0] * running
        best = score.view(M, C).argmax(dim=1)
        chosen = seq.view(M, C, H, d)[real, best]                   # [M, H, d]
        env.restore(keep, indices=real_mask)                        # the real robots stepped along: back to where they were
        actions[:M] = chosen[:, 0]
        _, rew, done, _ = env.step_tensor(actions)
        ret += rew[:M] * alive
        alive &= ~done[:M].bool()
        plan = torch.cat([chosen[:, 1:], chosen[:, -1:]], dim=1)    # shifted by one step, the last action held
    ret += env.get_info("reward_end")[:M, 0] * alive            # robots still in their episode: what the task would pay them now
    out = ret.mean().item(), int(alive.sum().item())
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=63)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--freeze-done", action="store_true", help="stop rolling out a candidate once its episode has ended")
    a = ap.parse_args()
    for C in (a.candidates, 1):
        r, up = run(a.robots, C, a.horizon, a.steps, a.sigma, a.seed, a.freeze_done)
        print(f"C = {C:3d} candidates x H = {a.horizon}: mean return of the {a.robots} real robots over their first episode (at most {a.steps} steps) "
              f"{r:8.3f}, {up} of them still in it")


if __name__ == "__main__":
    main()
