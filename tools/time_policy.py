#!/usr/bin/env python3
"""What one policy forward pass costs on the stream: DevicePolicy.act (one HIP launch) against the same torch.nn.Sequential + clamp eager,
the same under torch.cuda.graph, and -- with one parameter row per block of environments -- against a torch bmm formulation; the step
kernel's own time next to them for scale.  HIP events around 1000 enqueues after 50 warm-up, the stream kept busy (no synchronisation
inside the timed region), median of 5 repeats.

    python tools/time_policy.py [--out profiles/policy_launch.md]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch  # noqa: E402

from qs_amd import DevicePolicy, QuadrupedVecEnv  # noqa: E402


def timed(fn, iters=1000, warmup=50, repeats=5):
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


def sequential(obs_dim, arch, action_dim, bias=True):
    nn = torch.nn
    layers, d = [], obs_dim
    for w in arch:
        layers += [nn.Linear(d, w, bias=bias), nn.Tanh()]
        d = w
    layers.append(nn.Linear(d, action_dim, bias=bias))
    return nn.Sequential(*layers).cuda()


def graphed(fn):
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g.replay
    except Exception as e:  # noqa: BLE001
        print("torch.cuda.graph did not capture:", e, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    with torch.no_grad():
        for n in (8192, 65536):
            for name, arch, bias in (("linear 28->6 (no bias)", (), False), ("28-64-64-6 tanh", (64, 64), True)):
                net = sequential(28, arch, 6, bias)
                obs = torch.randn(n, 28, device="cuda")
                pol = DevicePolicy.from_module(net, num_envs=n)
                eager = lambda: net(obs).clamp_(-1.0, 1.0)  # noqa: E731
                g = graphed(eager)
                rows.append((n, 1, name, timed(lambda: pol.act(obs)), timed(eager), timed(g) if g else None))
                assert (pol.act(obs) - eager()).abs().max().item() < 1e-5
                pol.close()
        # one parameter row per block of 64 environments (ARS candidates): the kernel against gather-free bmm
        n, P = 8192, 128
        for name, arch in (("linear 28->6 (no bias)", ()), ("28-64-64-6 tanh", (64, 64))):
            bias = bool(arch)
            pol = DevicePolicy(28, 6, net_arch=arch, activation="tanh" if arch else "none", bias=bias, num_envs=n, n_policies=P)
            theta = torch.randn(P, pol.n_params, device="cuda") * 0.1
            pol.set_params(theta)
            obs = torch.randn(n, 28, device="cuda")
            dims, off, Ws, bs = [28] + list(arch) + [6], 0, [], []
            for i in range(len(dims) - 1):
                o, k = dims[i + 1], dims[i]
                Ws.append(theta[:, off:off + o * k].reshape(P, o, k).transpose(1, 2).contiguous()); off += o * k
                if bias:
                    bs.append(theta[:, off:off + o].reshape(P, 1, o).contiguous()); off += o

            def bmm():
                h = obs.view(P, n // P, 28)
                for i, W in enumerate(Ws):
                    h = torch.baddbmm(bs[i], h, W) if bias else torch.bmm(h, W)
                    if i < len(Ws) - 1:
                        h = torch.tanh(h)
                return h.clamp_(-1.0, 1.0).view(n, 6)
            assert (pol.act(obs) - bmm()).abs().max().item() < 1e-4
            g = graphed(bmm)
            rows.append((n, P, name, timed(lambda: pol.act(obs)), timed(bmm), timed(g) if g else None))
            pol.close()
    step = {}
    for n in (8192, 65536):
        env = QuadrupedVecEnv(num_envs=n, device=0, auto_reset=True, task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True,
                              enable_action_filter=True, env_randomizer_mode="GROUND_RANDOMIZER")
        env.enable_timing(True)
        env.reset_tensor()
        a = torch.zeros(n, env.action_dim, device="cuda")
        ms = []
        for _ in range(60):
            env.step_tensor(a)
            ms.append(env.last_step_kernel_ms())
        step[n] = statistics.median(ms[10:]) * 1e3
        env.close()
    lines = ["| N | policies | network | DevicePolicy.act (us) | torch eager (us) | torch.cuda.graph (us) | step kernel (us) |", "|---|---|---|---|---|---|---|"]
    f = lambda x: "n/a" if x is None else f"{x:.1f}"  # noqa: E731
    for n, P, name, a, b, c in rows:
        lines.append(f"| {n} | {P} | {name} | {f(a)} | {f(b) + (' (bmm)' if P > 1 else '')} | {f(c)} | {f(step.get(n))} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
