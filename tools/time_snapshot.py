"""Cost of device snapshots on the benchmark's environment: qs_snapshot, qs_restore, qs_fork from one source to all others and qs_fork under
a permutation, next to a torch device-to-device copy_ of the same number of bytes (the yardstick: it moves the same bytes with no logic)
and one step launch of a twin handle.  N = 1, 1024 and 8192 by default; per case the time of --launches back-to-back calls between two
events on the stream, divided by their number, --repeats times with the cases interleaved: mean and min / max of the repeats.  The
entries are called through the C ABI with their arguments prepared (as a control loop that reuses its tensors would), so at N = 1 the
figures are what a launch costs, not what the bytes cost.  A fork is two launches (gather, scatter).  Prints one JSON line, and writes it
to --out (profiles/snapshot_cost.json)."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped-springs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1, 1024, 8192])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from qs_amd import lib as _lib
    from qs_amd.handle import ptr
    from qs_amd.vec_env import QuadrupedVecEnv
    kw = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, enable_action_filter=True,
              env_randomizer_mode="GROUND_RANDOMIZER", seed=1, noise=False, auto_reset=True)
    res = {"launches": a.launches, "repeats": a.repeats, "cases": {}}
    for n in a.n:
        v = QuadrupedVecEnv(num_envs=n, **kw)
        v.reset_tensor()
        rng = np.random.default_rng(0)
        acts = [torch.as_tensor(rng.uniform(-1, 1, (n, v.action_dim)).astype(np.float32), device=v.device) for _ in range(16)]
        for k in range(50):
            v.step_tensor(acts[k % 16])
        # the step launch is timed on a twin handle that is never restored: a restore re-seats the look-ahead windows, and the settle lanes
        # then work the N x K states off inside the following step launches
        w = QuadrupedVecEnv(num_envs=n, **kw)
        w.reset_tensor()
        for k in range(50):
            w.step_tensor(acts[k % 16])
        snap = v.snapshot()
        rows, twin = snap.rows, torch.empty_like(snap.rows)
        one = torch.zeros(n, dtype=torch.int32, device=v.device)
        perm = torch.as_tensor(rng.permutation(n).astype(np.int32), device=v.device)
        v._stream()
        turn = itertools.count()
        h, L, p = v.h, v.lib, ptr
        cases = dict(snapshot=lambda: L.qs_snapshot(h, None, p(rows)), restore=lambda: L.qs_restore(h, None, p(rows)),
                     fork_one_to_all=lambda: L.qs_fork(h, p(one)), fork_permutation=lambda: L.qs_fork(h, p(perm)),
                     copy_same_bytes=lambda: twin.copy_(rows), step=lambda: w.step_tensor(acts[next(turn) % 16]))
        times = {c: [] for c in cases}
        for c in cases:                             # (first calls: the fork's staging rows, the allocator)
            cases[c]()
        for _ in range(a.repeats):
            for c, call in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _k in range(a.launches):
                    call()
                e1.record()
                torch.cuda.synchronize()
                times[c].append(1000.0 * e0.elapsed_time(e1) / a.launches)
        v.counter("resets")                         # (raises if a fork was refused)
        row = {"row_bytes": int(snap.row_floats) * 4, "bytes": int(snap.bytes)}
        for c, ts in times.items():
            row[c + "_us"] = float(np.mean(ts))
            row[c + "_us_min_max"] = [float(np.min(ts)), float(np.max(ts))]
        res["cases"][str(n)] = row
        v.close(); w.close()
        del v, w
        torch.cuda.synchronize()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
