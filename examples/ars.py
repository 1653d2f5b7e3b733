#!/usr/bin/env python3
"""Augmented Random Search (the reference's first training step, sb3_contrib ARS) with every candidate of an iteration evaluated in ONE
rollout: 8192 environments = 64 directions x 2 signs x 64 episodes, each block of 64 environments driven by its own perturbed parameter
vector through DevicePolicy (one HIP launch per step for all 128 policies).  DeviceARS keeps an iteration's bookkeeping on the GPU as well:
the candidates, the episode accounting (one small launch per step, the host looks at the alive counter every 16 steps) and the update.
--host-loop runs the loop this example had before DeviceARS (torch accumulation, a host wait per step, torch's argsort / std / matmul), for
comparison; tools/time_ars.py times the two against each other.

--freeze-done: environments whose episode has ended are no longer stepped (DeviceARS(freeze_done=True), step_tensor(active=)); under this
example's DeviceVecNormalize(training=True) the statistics then see living robots only, so the numbers printed differ from a run without it.

    python examples/ars.py [--iterations 12] [--n-delta 64] [--episodes 64] [--horizon 300] [--host-loop] [--freeze-done]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch

from qs_amd import DeviceARS, DevicePolicy, DeviceVecNormalize, QuadrupedVecEnv
from qs_amd.policy import ars_population, ars_update


def make(n_delta, episodes):
    P, n = 2 * n_delta, 2 * n_delta * episodes
    venv = QuadrupedVecEnv(num_envs=n, device=0, auto_reset=False, task_env="JUMPING_IN_PLACE", observation_space_mode="ARS_BASIC",
                           action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                           env_randomizer_mode="GROUND_RANDOMIZER")
    env = DeviceVecNormalize(venv, training=True, norm_reward=False)
    policy = DevicePolicy(env.obs_dim, env.action_dim, net_arch=(), activation="none", bias=False, num_envs=n, n_policies=P)   # ARS "LinearPolicy"
    return env, policy


def host_iteration(env, policy, theta, deltas, n_delta, episodes, horizon, sigma, step_size, n_top):
    """one iteration as this example ran it before DeviceARS -> (the new theta, the per-candidate mean returns, the steps it took)"""
    n = env.num_envs
    policy.set_params(ars_population(theta, deltas, sigma))             # [P, n_params]: + first, - second
    obs = env.reset_tensor()
    ret = torch.zeros(n, device="cuda")
    alive = torch.ones(n, dtype=torch.bool, device="cuda")
    steps = 0
    for _ in range(horizon):
        obs, rew, done, trunc = env.step_tensor(policy.act(obs))
        ret += env.old_reward * alive                                   # the raw reward, until the environment's episode ends
        alive &= ~done.bool()
        steps += 1
        if not bool(alive.any()):                                       # (a host synchronisation per step)
            break
    per_policy = ret.view(2 * n_delta, episodes).mean(1)                # the per-block episode return
    r_plus, r_minus = per_policy[:n_delta], per_policy[n_delta:]
    return ars_update(theta, deltas, r_plus, r_minus, step_size, n_top), per_policy, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--n-delta", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=64, help="episodes (environments) per candidate")
    ap.add_argument("--horizon", type=int, default=300, help="steps after which an iteration's rollout stops")
    ap.add_argument("--n-top", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=0.05)       # sb3_contrib: delta_std
    ap.add_argument("--step-size", type=float, default=0.02)   # sb3_contrib: learning_rate
    ap.add_argument("--host-loop", action="store_true", help="the torch bookkeeping with a host wait per step, as before DeviceARS")
    ap.add_argument("--freeze-done", action="store_true", help="stop stepping an environment once its episode has ended")
    args = ap.parse_args()
    if args.host_loop and args.freeze_done:
        ap.error("--freeze-done belongs to DeviceARS, not to --host-loop")
    env, policy = make(args.n_delta, args.episodes)
    if args.host_loop:
        torch.manual_seed(0)
        theta = torch.zeros(policy.n_params, device="cuda")
        for it in range(args.iterations):
            deltas = torch.randn(args.n_delta, policy.n_params, device="cuda")
            theta, per_policy, _ = host_iteration(env, policy, theta, deltas, args.n_delta, args.episodes, args.horizon, args.sigma, args.step_size, args.n_top)
            print(f"iteration {it:2d}: mean return {per_policy.mean().item():8.3f}   best candidate {per_policy.max().item():8.3f}")
    else:
        # (a candidate's return is the SUM over its block: the step's scale is 1 / (n_top std) of those sums, so the learning rate that
        # matches the host loop's block means is step_size itself -- the update is invariant to a common factor of the returns)
        ars = DeviceARS(env, policy, n_delta=args.n_delta, n_top=args.n_top, learning_rate=args.step_size, delta_std=args.sigma, horizon=args.horizon, seed=0,
                        freeze_done=args.freeze_done)
        for it in range(args.iterations):
            per_policy = ars.train_iteration() / args.episodes
            print(f"iteration {it:2d}: mean return {per_policy.mean().item():8.3f}   best candidate {per_policy.max().item():8.3f}")
        ars.close()
    policy.close()
    env.close()


if __name__ == "__main__":
    main()
