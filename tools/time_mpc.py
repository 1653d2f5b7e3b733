#!/usr/bin/env python3
"""What a control step of sampling MPC costs with the torch loop of examples/mpc.py (imported, not copied: TorchPlanner) and with DeviceMPC,
each with and without freeze_done, DeviceMPC under both methods: six loops, each on an environment of its own with the same seed, ALTERNATING
in one process after a warm-up of every one.  HIP events around a window of whole control steps (the real robots' step and the example's
return accounting included, the same in every loop); the window of a loop is sized from its warm-up to hold at least a second of work;
median and range over the repeats.  Two tables: at the example's sigma the robots of each loop are where that loop's plans have taken them, so
the loops do not step the same states; at sigma = 0 every robot stands and the loops differ by their launches alone.  Results are held by
tests/test_gpu_mpc.py, not here.

    python tools/time_mpc.py [--out profiles/mpc_planner.md] [--repeats 5]"""
import argparse
import importlib.util
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch  # noqa: E402

LAUNCHES = """Launches, counted from the code (examples/mpc.py's TorchPlanner.step, qs_amd/mpc.py's DeviceMPC.step; H = horizon).  The real robots' one
step and the example's return accounting (five torch launches) are the same in every loop and are not counted.

| | torch loop | torch loop, freeze_done | DeviceMPC | DeviceMPC, freeze_done |
|---|---|---|---|---|
| per horizon step, next to the step launch | 6: the strided copy into actions[M:], multiply, add, cast, not, and | 7: and the mask copy | 1: k_mpc_feed | 1: k_mpc_feed (writes the mask too) |
| per control step, outside the horizon loop | 20: fork 2, snapshot 1, randn 1, multiply 1, add 1, candidate-0 copy 1, clamp 1, zeros 1, ones 1, reward_end getter 1, multiply 1, add 1, argmax 1, gather 1, restore 2, action copy 1, cat 1 | 20 | 11: fork 2, snapshot 1, randn 1, k_mpc_sample 1, reward_end getter 1, k_mpc_feed(H) 1, k_mpc_finish 1, restore 2, k_mpc_set_plan 1 | 8: no snapshot, no restore |
| per control step at H = 12, step launches included | 20 + 12 x 7 = 104 | 20 + 12 x 8 = 116 | 11 + 12 x 2 = 35 | 8 + 12 x 2 = 32 |"""


def example():
    spec = importlib.util.spec_from_file_location("mpc_example", os.path.join(REPO, "examples", "mpc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def window(loop, k):
    """milliseconds per control step over k control steps, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        loop.step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def spread(x):
    return f"{statistics.median(x):.3f} ({min(x):.3f} - {max(x):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=63)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--sigmas", type=float, nargs="+", default=[0.5, 0.0], help="one table per value; 0 keeps every loop on the same (standing) states")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.1, help="the least work a window holds")
    a = ap.parse_args()
    ex = example()
    M, C, H = a.robots, a.candidates, a.horizon
    n = M * (1 + C)
    lines = [f"`python tools/time_mpc.py`: {M} robots x {C} candidates = {n} environments, horizon {H}, JUMPING_IN_PLACE; {a.repeats} alternating windows per "
             f"loop after a warm-up of every loop, each window at least {a.seconds} s of work; HIP events around whole control steps; median (min - max)."]
    for sigma in a.sigmas:
        loops = {}
        for freeze in (False, True):
            tail = ", freeze_done" if freeze else ""
            loops["torch loop" + tail] = ex.TorchPlanner(ex.make_env(M, C, 0), M, C, H, sigma, 0, freeze)
            for method in ("best", "mppi"):
                loops[f"DeviceMPC {method}" + tail] = ex.DevicePlanner(ex.make_env(M, C, 0), M, C, H, sigma, 0, freeze, method, a.temperature)
        names = list(loops)
        # warm-up of every loop, and the size of its window
        size = {}
        for name in names:
            window(loops[name], 20)
            size[name] = max(20, int(a.seconds / (window(loops[name], 50) * 1e-3)) + 1)
        rows = {name: [] for name in names}
        for it in range(a.repeats):
            for name in names[it % len(names):] + names[:it % len(names)]:
                rows[name].append(window(loops[name], size[name]))
        what = ("sigma = 0: every candidate is the plan and the plan stays zero, so the robots stand and EVERY loop steps the same states -- the loops differ "
                "by their launches alone" if sigma == 0 else
                f"sigma = {sigma}: the robots of each loop are where that loop's plans have taken them (jumping, landing, lying on the floor, which is the "
                "slow many-rows contact path), so the loops do not step the same states")
        lines += ["", f"**{what}.**", "", "| loop | ms per control step | control steps per window | us per horizon step (ms / (H + 1)) |", "|---|---|---|---|"]
        for name in names:
            lines.append(f"| {name} | {spread(rows[name])} | {size[name]} | {spread([x * 1e3 / (H + 1) for x in rows[name]])} |")
        lines.append("")
        for freeze in (False, True):
            tail = ", freeze_done" if freeze else ""
            base = rows["torch loop" + tail]
            for method in ("best", "mppi"):
                dev = rows[f"DeviceMPC {method}" + tail]
                apart = max(dev) < min(base) or min(dev) > max(base)
                lines.append(f"DeviceMPC {method}{tail} / torch loop{tail}, median ms per control step: {statistics.median(dev) / statistics.median(base):.3f}; the ranges "
                             f"({min(dev):.3f} - {max(dev):.3f} against {min(base):.3f} - {max(base):.3f} ms) " +
                             ("do not overlap." if apart else "OVERLAP: the difference is inside the spread of the two."))
        for loop in loops.values():
            if hasattr(loop, "mpc"):
                loop.mpc.close()
            loop.env.close()
    lines += ["", LAUNCHES]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
