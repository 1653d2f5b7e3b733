"""Cost of external pushes (QuadrupedVecEnv.apply_external_force) per step launch at N = 8192, on the benchmark's environment: no push, a
50 N world-frame lateral push on every environment for one env step, the same push on one environment in 64.  Each case on a fresh
handle, the push set again before every step (as a learner that shoves every step would); prints one JSON line, and writes it to --out.
The time per launch is the step kernel's batch timing (qs_enable_timing), which also spans the small kernels of apply_external_force
between two steps; --case runs one case only, for a rocprofv3 --kernel-trace --stats run that gives the step kernel's own duration."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped-springs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--case", default="", choices=["", "none", "all", "one_in_64"])
    a = ap.parse_args()
    import torch
    from qs_amd.vec_env import QuadrupedVecEnv
    kw = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, enable_action_filter=True,
              env_randomizer_mode="GROUND_RANDOMIZER", seed=1, noise=False)
    n = a.n
    res = {"n": n, "steps": a.steps}
    cases = (a.case,) if a.case else ("none", "all", "one_in_64")
    for case in cases:
        v = QuadrupedVecEnv(num_envs=n, **kw)
        v.reset_tensor()
        rng = np.random.default_rng(0)
        acts = [torch.as_tensor(rng.uniform(-1, 1, (n, v.action_dim)).astype(np.float32), device=v.device) for _ in range(16)]
        F = torch.zeros((n, 3), device=v.device)
        F[:, 1] = 50.0
        steps = torch.full((n,), v.cfg.action_repeat, dtype=torch.int32, device=v.device)
        if case == "one_in_64":
            steps[torch.arange(n, device=v.device) % 64 != 0] = 0
        for k in range(a.warmup + a.steps):
            if k == a.warmup:
                v.enable_timing(True)
            if case != "none":
                v.apply_external_force(F, substeps=steps, frame="world")
            v.step_tensor(acts[k % 16])
        res[case + "_us"] = 1000.0 * v.last_step_kernel_ms()
        res[case + "_pending_after"] = float(v.get_info("external_wrench")[:, 6].max().item())
        v.close()
        del v
        torch.cuda.synchronize()
    if not a.case:
        res["all_vs_none"] = res["all_us"] / res["none_us"] - 1.0
        res["one_in_64_vs_none"] = res["one_in_64_us"] / res["none_us"] - 1.0
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
