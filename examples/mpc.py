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

--device-planner: the same loop with qs_amd.DeviceMPC, the planner's bookkeeping in HIP (one small launch per horizon step instead of six or
seven torch launches; ties go to the lower candidate, so a run is reproducible from its seed); --method mppi [--temperature T] takes the mean
of the candidates under the weights exp((score - max) / T) instead of the best one.

    python examples/mpc.py [--robots 64] [--candidates 63] [--horizon 12] [--steps 150] [--sigma 0.5] [--freeze-done]
                           [--device-planner [--method {best,mppi}] [--temperature 1.0]]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch

from qs_amd import QuadrupedVecEnv


def make_env(M, C, seed):
    return QuadrupedVecEnv(num_envs=M * (1 + C), device=0, auto_reset=True, task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC",
                           action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                           env_randomizer_mode="GROUND_RANDOMIZER", noise=False, seed=seed)


class TorchPlanner:
    """the torch loop: the state of the planner and of the real robots' returns, and one control step of it"""

    def __init__(self, env, M, C, H, sigma, seed, freeze_done=False):
        self.env, self.M, self.C, self.H, self.sigma, self.freeze_done = env, M, C, H, sigma, freeze_done
        n = M * (1 + C)
        dev, d = env.device, env.action_dim
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        # environments [0, M) are the real robots; candidate c of robot m is environment M + m * C + c
        self.real = torch.arange(M, device=dev)
        self.src_of = torch.cat([torch.full((M,), -1, device=dev), self.real.repeat_interleave(C)]).to(torch.int32)
        self.real_mask = torch.zeros(n, dtype=torch.bool, device=dev)
        self.real_mask[:M] = True
        env.reset_tensor()
        self.keep = env.snapshot(indices=self.real_mask)
        self.plan = torch.zeros((M, H, d), device=dev)
        self.actions = torch.zeros((n, d), device=dev)
        self.ret = torch.zeros(M, device=dev)
        self.alive = torch.ones(M, dtype=torch.bool, device=dev)
        self.active = torch.ones(n, dtype=torch.bool, device=dev)      # --freeze-done: the real robots, and the candidates still in their episode

    def step(self):
        env, M, C, H, sigma, gen, freeze_done = self.env, self.M, self.C, self.H, self.sigma, self.gen, self.freeze_done
        real, real_mask, keep, plan, actions, active = self.real, self.real_mask, self.keep, self.plan, self.actions, self.active
        dev, d = env.device, env.action_dim
        env.fork(src_of=self.src_of)
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
        self.ret += rew[:M] * self.alive
        self.alive &= ~done[:M].bool()
        self.plan = torch.cat([chosen[:, 1:], chosen[:, -1:]], dim=1)    # shifted by one step, the last action held


class DevicePlanner:
    """the same loop with qs_amd.DeviceMPC (--device-planner): the planner's bookkeeping in HIP, one small launch per horizon step"""

    def __init__(self, env, M, C, H, sigma, seed, freeze_done=False, method="best", temperature=1.0):
        from qs_amd import DeviceMPC
        self.env, self.M = env, M
        env.reset_tensor()
        self.mpc = DeviceMPC(env, M, C, H, sigma=sigma, method=method, temperature=temperature, freeze_done=freeze_done, seed=seed)
        self.ret = torch.zeros(M, device=env.device)
        self.alive = torch.ones(M, dtype=torch.bool, device=env.device)

    def step(self):
        _, rew, done, _ = self.mpc.step()
        self.ret += rew * self.alive
        self.alive &= ~done.bool()


def run(M, C, H, steps, sigma, seed, freeze_done=False, device_planner=False, method="best", temperature=1.0):
    env = make_env(M, C, seed)
    if device_planner:
        loop = DevicePlanner(env, M, C, H, sigma, seed, freeze_done, method, temperature)
    else:
        loop = TorchPlanner(env, M, C, H, sigma, seed, freeze_done)
    for _ in range(steps):
        loop.step()
    ret, alive = loop.ret, loop.alive
    ret += env.get_info("reward_end")[:M, 0] * alive            # robots still in their episode: what the task would pay them now
    out = ret.mean().item(), int(alive.sum().item())
    if device_planner:
        loop.mpc.close()
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
    ap.add_argument("--device-planner", action="store_true", help="plan with qs_amd.DeviceMPC (HIP) instead of the torch loop")
    ap.add_argument("--method", choices=("best", "mppi"), default="best", help="with --device-planner: the best candidate, or MPPI's weighted mean")
    ap.add_argument("--temperature", type=float, default=1.0, help="with --method mppi: the weights are exp((score - max) / temperature)")
    a = ap.parse_args()
    if a.method != "best" and not a.device_planner:
        ap.error("--method mppi needs --device-planner (the torch loop is best-of-C)")
    for C in (a.candidates, 1):
        r, up = run(a.robots, C, a.horizon, a.steps, a.sigma, a.seed, a.freeze_done, a.device_planner, a.method, a.temperature)
        print(f"C = {C:3d} candidates x H = {a.horizon}: mean return of the {a.robots} real robots over their first episode (at most {a.steps} steps) "
              f"{r:8.3f}, {up} of them still in it")


if __name__ == "__main__":
    main()
