"""Cost of the rack (on_rack=True) per step launch, on the benchmark's environment: the same handle without a rack, with every robot hung,
and with every robot released after the reset (the rack kernels with no hung robot).  N = 1, 1024 and 8192 by default; each case on a fresh
handle, --repeats times, interleaved; the time per launch is the step kernel's batch timing (qs_enable_timing): mean and min / max of the
repeats.  The cases do different work besides the rows (robots on the floor that fall under random actions, hung ones that touch nothing,
released ones that drop 1 m and land), so the ratios are those of the workloads, not the price of the six rows alone.  Prints one JSON
line, and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped-springs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1, 1024, 8192])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from qs_amd.vec_env import QuadrupedVecEnv
    kw = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, enable_action_filter=True,
              env_randomizer_mode="GROUND_RANDOMIZER", seed=1, noise=False, auto_reset=False)
    res = {"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "cases": {}}
    for n in a.n:
        times = {c: [] for c in ("no_rack", "hung", "released")}
        for _ in range(a.repeats):                 # (the cases interleaved, each on a fresh handle)
            for case in times:
                v = QuadrupedVecEnv(num_envs=n, on_rack=case != "no_rack", **kw)
                v.reset_tensor()
                if case == "released":
                    v.set_rack(False)
                rng = np.random.default_rng(0)
                acts = [torch.as_tensor(rng.uniform(-1, 1, (n, v.action_dim)).astype(np.float32), device=v.device) for _ in range(16)]
                for k in range(a.warmup + a.steps):
                    if k == a.warmup:
                        v.enable_timing(True)
                    v.step_tensor(acts[k % 16])
                times[case].append(1000.0 * v.last_step_kernel_ms())
                v.close()
                del v
                torch.cuda.synchronize()
        row = {}
        for case, ts in times.items():
            row[case + "_us"] = float(np.mean(ts))
            row[case + "_us_min_max"] = [float(np.min(ts)), float(np.max(ts))]
        row["hung_vs_no_rack"] = row["hung_us"] / row["no_rack_us"]
        row["released_vs_no_rack"] = row["released_us"] / row["no_rack_us"]
        res["cases"][str(n)] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
