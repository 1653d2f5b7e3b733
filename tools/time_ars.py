#!/usr/bin/env python3
"""What an ARS iteration costs with DeviceARS, with DeviceARS(freeze_done=True) -- environments whose episode has ended are no longer
stepped (step_tensor(active=)) -- and with the host loop examples/ars.py had before (--host-loop): the three ALTERNATE in one
process on the same environments, the same policy handle and the same directions; wall-clock time around a whole iteration with the device
drained at its end (the host waits are what is compared), median and spread over the repeats; per loop also the environments stepped per
rollout step and the many-rows wave-substeps (counter limit_path_substeps) of an iteration.  Next to it the per-launch time of
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
    ars_f = DeviceARS(env, policy, n_delta=args.n_delta, n_top=args.n_top, learning_rate=0.02, delta_std=0.05, horizon=args.horizon, seed=0, freeze_done=True)
    learners = {"DeviceARS": ars, "DeviceARS, freeze_done": ars_f}
    sim = env.venv if hasattr(env, "venv") else env
    theta_host = torch.zeros(policy.n_params, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    rows = {"DeviceARS": [], "DeviceARS, freeze_done": [], "host loop": []}
    order = list(rows)
    for it in range(args.warmup + args.repeats):
        deltas = torch.randn(args.n_delta, policy.n_params, device="cuda", generator=gen)
        for name in order[it % 3:] + order[:it % 3]:
            rare0 = sim.counter("limit_path_substeps")                   # (waits for the device: outside the timed part)
            if name != "host loop":
                policy.set_params(learners[name].candidates)            # (the handle reads this learner's tensor)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name != "host loop":
                learner = learners[name]
                learner.perturb(deltas)
                learner.rollout()
                learner.finish()
                steps = learner.last_rollout_steps
            else:
                theta_host, _, steps = ex.host_iteration(env, policy, theta_host, deltas, args.n_delta, args.episodes, args.horizon, 0.05, 0.02, args.n_top)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            # environments stepped per rollout step: all of them, or (freeze_done) those alive = the sum of the episode lengths / steps
            stepped = int(learners[name].get("steps").item()) / steps if name == "DeviceARS, freeze_done" else float(n)
            if it >= args.warmup:
                rows[name].append((ms, steps, stepped, sim.counter("limit_path_substeps") - rare0))
    # The direct measurement: the same candidates with and without freezing.  Statistics held (training=False) and both learners on one theta:
    # what differs is who is stepped (and the episode's randomizer draws, new at every reset); rollout() alone, alternating.
    same = {"DeviceARS": [], "DeviceARS, freeze_done": []}
    was_training = getattr(env, "training", None)
    if was_training is not None:
        env.training = False
    ars_f.theta.copy_(ars.theta)
    for it in range(args.warmup + args.repeats):
        deltas = torch.randn(args.n_delta, policy.n_params, device="cuda", generator=gen)
        names = list(same)
        for name in (names if it % 2 == 0 else names[::-1]):
            learner = learners[name]
            policy.set_params(learner.candidates)
            learner.perturb(deltas)
            rare0 = sim.counter("limit_path_substeps")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            learner.rollout()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            alive_steps = int(learner.get("steps").item())
            if it >= args.warmup:
                same[name].append((ms, learner.last_rollout_steps, alive_steps / learner.last_rollout_steps, sim.counter("limit_path_substeps") - rare0))
    if was_training is not None:
        env.training = was_training
    policy.set_params(ars.candidates)
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
             "| loop | ms per iteration | rollout steps per iteration | us per rollout step | environments stepped per rollout step | "
             "limit_path_substeps per iteration |", "|---|---|---|---|---|---|"]
    for name, r in rows.items():
        lines.append(f"| {name} | {spread([x[0] for x in r])} | {spread([float(x[1]) for x in r])} | {spread([x[0] * 1e3 / x[1] for x in r])} | "
                     f"{spread([x[2] for x in r])} | {spread([float(x[3]) for x in r])} |")
    med = {name: statistics.median(x[0] for x in r) for name, r in rows.items()}
    dev, host, frz = med["DeviceARS"], med["host loop"], med["DeviceARS, freeze_done"]
    lo, hi = min(x[0] for x in rows["DeviceARS"]), max(x[0] for x in rows["DeviceARS"])
    flo, fhi = min(x[0] for x in rows["DeviceARS, freeze_done"]), max(x[0] for x in rows["DeviceARS, freeze_done"])
    apart = fhi < lo or flo > hi
    lines += ["", f"DeviceARS / host loop, median ms per iteration: {dev / host:.3f}.  All include the reset of all environments at the start of the "
              f"iteration: {spread(ms_reset)} ms.", "",
              f"freeze_done / DeviceARS, median ms per iteration: {frz / dev:.3f}; the two loops' min - max ranges "
              f"({flo:.2f} - {fhi:.2f} against {lo:.2f} - {hi:.2f} ms) " + ("do not overlap." if apart else "OVERLAP: the difference is inside the spread of the two.") +
              "  (The environment is a DeviceVecNormalize in training mode, so the frozen loop's statistics see living robots only and its "
              "policies, episodes and counts are its own: the comparison is of cost, not of results.)", "",
              "The same candidates with and without freezing (statistics held with training=False, one theta for both learners, the same directions; "
              "the ground randomizer draws anew at every reset, so the episodes are alike, not the same bits; rollout() alone, alternating):", "",
              "| loop | ms per rollout | us per rollout step | environments alive per rollout step | limit_path_substeps per rollout |", "|---|---|---|---|---|"]
    for name, r in same.items():
        lines.append(f"| {name} | {spread([x[0] for x in r])} | {spread([x[0] * 1e3 / x[1] for x in r])} | {spread([x[2] for x in r])} | "
                     f"{spread([float(x[3]) for x in r])} |")
    a_lo, a_hi = min(x[0] for x in same["DeviceARS"]), max(x[0] for x in same["DeviceARS"])
    f_lo, f_hi = min(x[0] for x in same["DeviceARS, freeze_done"]), max(x[0] for x in same["DeviceARS, freeze_done"])
    ratio = statistics.median(x[0] for x in same["DeviceARS, freeze_done"]) / statistics.median(x[0] for x in same["DeviceARS"])
    lines += ["", f"freeze_done / DeviceARS on the same candidates, median ms: {ratio:.3f}; ranges {f_lo:.2f} - {f_hi:.2f} against {a_lo:.2f} - {a_hi:.2f} ms: " +
              ("they do not overlap." if f_hi < a_lo or f_lo > a_hi else "they OVERLAP."), "",
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
    ars_f.close()
    policy.close()
    env.close()


if __name__ == "__main__":
    main()
