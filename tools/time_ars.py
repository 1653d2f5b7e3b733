#!/usr/bin/env python3
"""What an ARS iteration costs with DeviceARS against the host loop examples/ars.py had before it (--host-loop): the two ALTERNATE in one
process on the same environments, the same policy handle and the same directions; wall-clock time around a whole iteration with the device
drained at its end (the host waits are what is compared), median and spread over the repeats.  Next to it the per-launch time of
k_ars_account and of finish (returns + select + apply), HIP events around back-to-back enqueues, median of 5 repeats.

    python tools/time_ars.py [--out profiles/ars_iteration.md] [--repeats 7]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch  # noqa: E402

from qs_amd import DeviceARS  # noqa: E402


def example():
    spec = importlib.util.spec_from_file_location("ars_example", os.path.join(REPO, "examples", "ars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, iters, warmup=20, repeats=5):
    """microseconds per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out)


def spread(x):
    return f"{statistics.median(x):.2f} ({min(x):.2f} - {max(x):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-delta", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=300)
    ap.add_argument("--n-top", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    ex = example()
    env, policy = ex.make(args.n_delta, args.episodes)
    n = env.num_envs
    ars = DeviceARS(env, policy, n_delta=args.n_delta, n_top=args.n_top, learning_rate=0.02, delta_std=0.05, horizon=args.horizon, seed=0)
    theta_host = torch.zeros(policy.n_params, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    rows = {"DeviceARS": [], "host loop": []}
    for it in range(args.warmup + args.repeats):
        deltas = torch.randn(args.n_delta, policy.n_params, device="cuda", generator=gen)
        for name in (("DeviceARS", "host loop") if it % 2 == 0 else ("host loop", "DeviceARS")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "DeviceARS":
                ars.perturb(deltas)
                ars.rollout()
                ars.finish()
                steps = ars.last_rollout_steps
            else:
                theta_host, _, steps = ex.host_iteration(env, policy, theta_host, deltas, args.n_delta, args.episodes, args.horizon, 0.05, 0.02, args.n_top)
                policy.set_params(ars.candidates)                       # (the handle reads DeviceARS's tensor again)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if it >= args.warmup:
                rows[name].append((ms, steps))
    # what both loops share: the reset of all environments at the start of an iteration
    ms_reset = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.reset_tensor()
        torch.cuda.synchronize()
        ms_reset.append((time.perf_counter() - t0) * 1e3)
    # the launches on their own
    rew, done = torch.rand(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    ars.begin()
    us_account = timed(lambda: ars.account(rew, done), 1000)
    ars.perturb(deltas)
    us_finish = timed(ars.finish, 200)
    us_perturb = timed(lambda: ars.perturb(deltas), 200)

    def host_bookkeeping():
        ret, alive = host_bookkeeping.ret, host_bookkeeping.alive
        ret += rew * alive
        alive &= ~done.bool()
    host_bookkeeping.ret, host_bookkeeping.alive = torch.zeros(n, device="cuda"), torch.ones(n, dtype=torch.bool, device="cuda")
    us_host_step = timed(host_bookkeeping, 1000)
    lines = [f"`python tools/time_ars.py`: N = {n} environments = {args.n_delta} directions x 2 signs x {args.episodes} episodes, linear policy "
             f"({policy.n_params} parameters), horizon {args.horizon}, n_top {args.n_top}; {args.repeats} alternating repeats after {args.warmup} warm-up "
             "iterations; median (min - max).", "",
             "| loop | ms per iteration | rollout steps per iteration | us per rollout step |", "|---|---|---|---|"]
    for name, r in rows.items():
        lines.append(f"| {name} | {spread([ms for ms, _ in r])} | {spread([float(s) for _, s in r])} | {spread([ms * 1e3 / s for ms, s in r])} |")
    dev, host = statistics.median(ms for ms, _ in rows["DeviceARS"]), statistics.median(ms for ms, _ in rows["host loop"])
    lines += ["", f"DeviceARS / host loop, median ms per iteration: {dev / host:.3f}.  Both include the reset of all environments at the start of the "
              f"iteration: {spread(ms_reset)} ms.", "",
              "| launch | us (stream kept busy, median of 5) |", "|---|---|",
              f"| k_ars_account (one per environment step) | {us_account:.1f} |",
              f"| the host loop's four torch launches per step, without its wait | {us_host_step:.1f} |",
              f"| finish = k_ars_returns + k_ars_select + k_ars_apply | {us_finish:.1f} |",
              f"| k_ars_perturb | {us_perturb:.1f} |"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    ars.close()
    policy.close()
    env.close()


if __name__ == "__main__":
    main()
