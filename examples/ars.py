#!/usr/bin/env python3
"""Augmented Random Search (the reference's first training step, sb3_contrib ARS) with every candidate of an iteration evaluated in ONE
rollout: 8192 environments = 64 directions x 2 signs x 64 episodes, each block of 64 environments driven by its own perturbed parameter
vector through DevicePolicy (one HIP launch per step for all 128 policies).  Nothing leaves the GPU inside an iteration.

    python examples/ars.py [--iterations 12] [--n-delta 64] [--episodes 64] [--horizon 300]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch

from qs_amd import DevicePolicy, DeviceVecNormalize, QuadrupedVecEnv
from qs_amd.policy import ars_population, ars_update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--n-delta", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=64, help="episodes (environments) per candidate")
    ap.add_argument("--horizon", type=int, default=300, help="steps after which an iteration's rollout stops")
    ap.add_argument("--n-top", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=0.05)       # sb3_contrib: delta_std
    ap.add_argument("--step-size", type=float, default=0.02)   # sb3_contrib: learning_rate
    args = ap.parse_args()
    P, n = 2 * args.n_delta, 2 * args.n_delta * args.episodes
    venv = QuadrupedVecEnv(num_envs=n, device=0, auto_reset=False, task_env="JUMPING_IN_PLACE", observation_space_mode="ARS_BASIC",
                           action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                           env_randomizer_mode="GROUND_RANDOMIZER")
    env = DeviceVecNormalize(venv, training=True, norm_reward=False)
    policy = DevicePolicy(env.obs_dim, env.action_dim, net_arch=(), activation="none", bias=False, num_envs=n, n_policies=P)   # ARS "LinearPolicy"
    torch.manual_seed(0)
    theta = torch.zeros(policy.n_params, device="cuda")
    for it in range(args.iterations):
        deltas = torch.randn(args.n_delta, policy.n_params, device="cuda")
        policy.set_params(ars_population(theta, deltas, args.sigma))        # [P, n_params]: + first, - second
        obs = env.reset_tensor()
        ret = torch.zeros(n, device="cuda")
        alive = torch.ones(n, dtype=torch.bool, device="cuda")
        for _ in range(args.horizon):
            obs, rew, done, trunc = env.step_tensor(policy.act(obs))
            ret += env.old_reward * alive                                   # the raw reward, until the environment's episode ends
            alive &= ~done.bool()
            if not bool(alive.any()):                                       # (the iteration's only host synchronisation)
                break
        per_policy = ret.view(P, args.episodes).mean(1)                     # the per-block episode return
        r_plus, r_minus = per_policy[:args.n_delta], per_policy[args.n_delta:]
        theta = ars_update(theta, deltas, r_plus, r_minus, args.step_size, args.n_top)
        print(f"iteration {it:2d}: mean return {per_policy.mean().item():8.3f}   best candidate {per_policy.max().item():8.3f}")
    policy.close()
    env.close()


if __name__ == "__main__":
    main()
