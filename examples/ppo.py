#!/usr/bin/env python3
"""PPO (the reference's second training step, SB3 PPO on the *_PPO tasks) with the rollout collected on the device: 8192 environments,
per collected step ONE launch for actor and critic (DeviceActorCritic) that also fills the rollout buffer's rows, GAE in one launch, the
update (SB3's PPO.train) in torch on the same parameter memory, or with --update device in HIP as well (gradient by index from the rollout
arrays, clip and Adam in place).  Nothing leaves the GPU inside an iteration but the printed line.

    python examples/ppo.py [--iterations 10] [--envs 8192] [--n-steps 64] [--update device]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch

from qs_amd import DeviceActorCritic, DevicePPO, DeviceVecNormalize, QuadrupedVecEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--n-steps", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--learning-rate", type=float, default=3e-4)
    ap.add_argument("--update", choices=("torch", "device"), default="torch")
    args = ap.parse_args()
    venv = QuadrupedVecEnv(num_envs=args.envs, device=0, auto_reset=True, task_env="JUMPING_IN_PLACE_PPO", observation_space_mode="PPO_BASIC",
                           action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                           env_randomizer_mode="GROUND_RANDOMIZER")
    env = DeviceVecNormalize(venv, training=True)
    torch.manual_seed(0)
    policy = DeviceActorCritic(env.obs_dim, env.action_dim, net_arch=(64, 64), activation="tanh", num_envs=args.envs)
    algo = DevicePPO(env, policy, n_steps=args.n_steps, batch_size=args.batch_size, n_epochs=args.epochs, learning_rate=args.learning_rate, seed=0, update=args.update)
    algo.learn(args.iterations * args.n_steps * args.envs)
    algo.close()
    policy.close()
    env.close()


if __name__ == "__main__":
    main()
