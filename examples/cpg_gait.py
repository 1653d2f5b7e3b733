#!/usr/bin/env python3
"""Hopf-oscillator gaits (quadruped_spring/hopf_network.py) on many robots at once.

    python examples/cpg_gait.py [--gait TROT] [--envs 1024] [--seconds 4] [--on-rack]

--on-rack hangs the robots at 1 m (hopf_network.py:185, "useful for debugging!"): the legs swing the gait in the air, and the script
prints how far the bases strayed from the anchor and the rack's mean vertical force instead of the walking figures.

The reference's driver (hopf_network.py:183-289) ticks four coupled oscillators on the host, maps them to foot positions, runs
inverse kinematics and a joint PD and sends torques to ONE PyBullet robot.  Here the oscillators, the foot trajectory, the inverse
kinematics and the PD run inside the step kernel (action_space_mode="CPG"): an action is the five gait parameters
(omega_swing, omega_stance, mu, step length, body height) scaled to [-1, 1], so a policy can steer the gait of every robot."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import numpy as np
import torch

from qs_amd import QuadrupedVecEnv
from qs_amd.config import CPG_HI, CPG_LO

GAITS = {"TROT": (16.0, 4.0), "WALK": (24.0, 25.0), "PACE": (20.0, 20.0), "BOUND": (10.0, 40.0)}   # omega_swing, omega_stance in units of pi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gait", default="TROT", choices=sorted(GAITS))
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--driver-gains", action="store_true", help="joint PD gains of the reference's driver (kp 150 / 70 / 70, kd 2 / 0.5 / 0.5) instead of the config's")
    ap.add_argument("--on-rack", action="store_true", help="hang the trunks at 1 m and swing the gait in the air (gait debugging)")
    args = ap.parse_args()
    env = QuadrupedVecEnv(num_envs=args.envs, auto_reset=False, task_env="NO_TASK", observation_space_mode="ENCODER", action_space_mode="CPG",
                          cpg_gait=args.gait, enable_springs=False, env_randomizer_mode="GROUND_RANDOMIZER", seed=0, on_rack=args.on_rack)
    ws, wst = GAITS[args.gait]
    want = np.array([ws * np.pi, wst * np.pi, 1.0, 0.05, 0.25])          # hopf_network.py:36-45: mu = 1, 5 cm steps, 25 cm body height
    lo, hi = np.array(CPG_LO), np.array(CPG_HI)
    a = torch.as_tensor(np.tile(2 * (want - lo) / (hi - lo) - 1, (args.envs, 1)), dtype=torch.float32, device=env.device)
    env.reset_tensor()
    if args.driver_gains:     # hopf_network.py:233-235
        env.set_params("kp", np.tile([150.0, 70.0, 70.0], (args.envs, 1)).astype(np.float32))
        env.set_params("kd", np.tile([2.0, 0.5, 0.5], (args.envs, 1)).astype(np.float32))
    x0 = env.get_state()[:, 0].clone()
    steps = int(args.seconds / 0.01)
    for _ in range(steps):
        env.step_tensor(a)
    st = env.get_state()
    if args.on_rack:
        rack = env.get_info("rack")
        print(f"{args.gait} on the rack: {args.envs} robots, {args.seconds:.1f} s: base {float((st[:, 2] - 1.0).abs().max()):.4f} m from the "
              f"anchor at most, rack force z {float(rack[:, 3].mean()):.1f} N on average")
        env.close()
        return
    up = 1 - 2 * (st[:, 3] ** 2 + st[:, 4] ** 2)                          # R22: cosine of the tilt
    walked = (st[:, 0] - x0).cpu().numpy()
    ok = ((up > 0.85) & (st[:, 2] > 0.15)).cpu().numpy()
    print(f"{args.gait}: {args.envs} robots, {args.seconds:.1f} s: upright {ok.mean():.1%}, forward speed of the upright ones "
          f"{walked[ok].mean() / args.seconds:.3f} +- {walked[ok].std() / args.seconds:.3f} m/s, body height {float(st[:, 2][torch.as_tensor(ok)].mean()):.3f} m")
    env.close()


if __name__ == "__main__":
    main()
