#!/usr/bin/env python3
"""What PPO collection costs on the stream (profiles/ppo_collect.md).  Same process, warm, HIP events around many enqueues with the
stream kept busy, median and spread (min .. max) of the repeats:
(a) per collected step at N = 8192, 28-64-64-6 tanh: qs_ac_collect (one launch) against the assembly it replaces -- two DevicePolicy.act
    launches (clipped action + log-prob, value) and the torch copies of observation, action, value and log-prob into [T, N, ...] storage;
(b) k_gae at T = 128 against the torch loop of the same recurrence on the device;
(c) one DevicePPO iteration with examples/ppo.py's defaults, split into collect, GAE and train();
    with --update: train() in both modes in ONE process at the same defaults, the per-minibatch time of each kernel of the device update,
    and the device's gradient against float64 under tests/ppo_train_ref.py's yardstick (profiles/ppo_update.md, profiles/ppo_update_parity.json);
(d) with --learn K: the return per iteration of K iterations of examples/ppo.py's configuration.

    python tools/time_ppo.py [--out profiles/ppo_collect.md] [--learn 10]
    python tools/time_ppo.py --update [--out profiles/ppo_update.md] [--parity profiles/ppo_update_parity.json]"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quadruped-springs_amd"))

import torch  # noqa: E402

from qs_amd import DeviceActorCritic, DevicePolicy, DevicePPO, DeviceRolloutBuffer, DeviceVecNormalize, QuadrupedVecEnv, lib  # noqa: E402


def timed(fn, iters=500, warmup=50, repeats=7):
    """microseconds per call: (median, min, max) over the repeats"""
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
    return statistics.median(out), min(out), max(out)


def fmt(x):
    return f"{x[0]:.1f} ({x[1]:.1f} .. {x[2]:.1f})"


def collect_step(n=8192, T=8):
    ac = DeviceActorCritic(28, 6, num_envs=n)
    pol = DevicePolicy(28, 6, num_envs=n)
    val = DevicePolicy(28, 1, num_envs=n, clip=None)
    pol.set_params(ac.actor_params); val.set_params(ac.critic_params)
    obs, eps, log_std = torch.randn(n, 28, device="cuda"), torch.randn(n, 6, device="cuda"), ac.log_std.detach()
    buf = DeviceRolloutBuffer(T, n, 28, 6)
    state = {"t": 0}

    def fused():
        t = state["t"] = (state["t"] + 1) % T
        ac.collect(obs, eps, buf.observations[t], buf.actions[t], buf.values[t], buf.log_probs[t])

    def assembled():
        t = state["t"] = (state["t"] + 1) % T
        a, mean, lp = pol.act(obs, eps, log_std, want_mean=True, want_log_prob=True)
        v = val.act(obs, want_mean=True)[1]
        buf.observations[t].copy_(obs)
        torch.addcmul(mean, log_std.exp(), eps, out=buf.actions[t])          # the unclipped sample SB3 stores
        buf.values[t].copy_(v[:, 0])
        buf.log_probs[t].copy_(lp)
    # alternate the two so that both see the same machine
    rows = [("qs_ac_collect (one launch)", timed(fused)), ("two DevicePolicy.act + torch copies", timed(assembled)),
            ("qs_ac_collect (one launch), again", timed(fused)), ("two DevicePolicy.act + torch copies, again", timed(assembled))]
    for p in (ac, pol, val):
        p.close()
    return rows


def gae_step(T=128, n=8192):
    buf = DeviceRolloutBuffer(T, n, 1, 1)
    buf.rewards.normal_(); buf.values.normal_()
    buf.episode_starts.copy_((torch.rand(T, n, device="cuda") < 0.05).float())
    lv, ld = torch.randn(n, device="cuda"), (torch.rand(n, device="cuda") < 0.3).to(torch.uint8)
    adv = torch.zeros_like(buf.rewards)

    def loop():
        gae = torch.zeros(n, device="cuda")
        for t in reversed(range(T)):
            nnt = 1.0 - (ld.float() if t == T - 1 else buf.episode_starts[t + 1])
            nv = lv if t == T - 1 else buf.values[t + 1]
            delta = buf.rewards[t] + buf.gamma * nv * nnt - buf.values[t]
            gae = delta + buf.gamma * buf.gae_lambda * nnt * gae
            adv[t] = gae
        return adv + buf.values
    return [("k_gae, T = 128, N = 8192", timed(lambda: buf.compute_returns_and_advantage(lv, ld), iters=200)),
            ("torch loop of the same recurrence", timed(loop, iters=5, warmup=2, repeats=5))]


def make_algo(envs=8192, n_steps=64, batch_size=65536, epochs=10, update="torch"):
    venv = QuadrupedVecEnv(num_envs=envs, device=0, auto_reset=True, task_env="JUMPING_IN_PLACE_PPO", observation_space_mode="PPO_BASIC",
                           action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                           env_randomizer_mode="GROUND_RANDOMIZER")
    env = DeviceVecNormalize(venv, training=True)
    torch.manual_seed(0)
    policy = DeviceActorCritic(env.obs_dim, env.action_dim, num_envs=envs)
    return DevicePPO(env, policy, n_steps=n_steps, batch_size=batch_size, n_epochs=epochs, seed=0, update=update)


def iteration_split(repeats=3):
    algo = make_algo()
    out = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        algo.collect_rollouts()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        algo.buffer.compute_returns_and_advantage(algo._last_values, algo._last_done)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        algo.train()
        torch.cuda.synchronize(); t3 = time.perf_counter()
        out.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    out = out[1:]                                                                   # the first iteration warms everything up
    med = lambda k: (statistics.median(x[k] for x in out), min(x[k] for x in out), max(x[k] for x in out))  # noqa: E731
    algo.policy.close(); algo.env.close()
    return [("collect_rollouts (64 steps x 8192 environments, with its GAE)", med(0)), ("k_gae alone, again", med(1)), ("train() (10 epochs x 8 minibatches of 65536)", med(2))]


def update_split(repeats=5):
    """train() in both modes on the SAME collected rollout, alternating so that both see the same machine; then the device update's kernels"""
    algos = {u: make_algo(update=u) for u in ("torch", "device")}
    for a in algos.values():
        a.collect_rollouts()
    times = {u: [] for u in algos}
    for _ in range(repeats + 1):
        for u, a in algos.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            a.train()
            torch.cuda.synchronize()
            times[u].append((time.perf_counter() - t0) * 1e3)
    rows = [(f'train() with update="{u}" (10 epochs x 8 minibatches of 65536)', (statistics.median(x[1:]), min(x[1:]), max(x[1:]))) for u, x in times.items()]
    a = algos["device"]
    total = a.n_steps * a.policy.num_envs
    idx = torch.randperm(total, device="cuda")[:a.batch_size].contiguous()
    a.grad_minibatch(idx)                                                     # (the hyper-parameters and the stream are set)
    h, hy, l = a.hp, a._hy, a.lib
    import ctypes as C
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    buf = a.buffer
    saved = [x.clone() for x in (a.policy.actor_params, a.policy.critic_params, a.policy.log_std.data, a.exp_avg, a.exp_avg_sq)]

    def grad():
        l.qs_ppo_grad(h, p(buf.observations), p(buf.actions), p(buf.log_probs), p(buf.advantages), p(buf.returns), total, p(idx), idx.numel(), C.byref(hy), p(a.grad), p(a._stats))

    def adam():
        l.qs_ppo_adam(h, p(a.grad), C.byref(hy), 1, p(a._stats))
    per = [("qs_ppo_grad, one minibatch of 65536 (k_adv_moments + k_ppo_grad + k_ppo_reduce)", timed(grad, iters=50, warmup=5)),
           ("qs_ppo_adam, one step (k_ppo_adam)", timed(adam, iters=50, warmup=5))]
    hy.normalize_advantage = 0
    per.append(("qs_ppo_grad without the normalisation (k_ppo_grad + k_ppo_reduce)", timed(grad, iters=50, warmup=5)))
    hy.normalize_advantage = 1
    with torch.no_grad():
        for x, y in zip((a.policy.actor_params, a.policy.critic_params, a.policy.log_std.data, a.exp_avg, a.exp_avg_sq), saved):
            x.copy_(y)
    for a in algos.values():
        a.close(); a.policy.close(); a.env.close()
    return rows, per


def update_parity(path):
    """the device's gradient against float64 and against the host twin under tests/ppo_train_ref.py's yardstick at the tests' shapes -> the
    record, per case: the device against float64, the twin against float64, the device against the twin (the tests print the same figures;
    this recorder keeps them)"""
    import json
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ppo_train_ref as T
    rec = {}
    for net in sorted(T.NETS):
        for B in T.BATCHES:
            pol, data, idx = T.case(net, B)
            algo = T.learner(pol, data, 1, B + 7, update="device", batch_size=B, clip_range=T.HYPER["clip_range"], ent_coef=T.HYPER["ent_coef"], vf_coef=T.HYPER["vf_coef"])
            algo.grad_minibatch(torch.as_tensor(idx, device="cuda"))
            g, st = algo.grad.cpu().numpy(), algo._read_stats()
            g_twin, st_twin, _, flags_twin = T.twin_grad(pol, data, idx, T.HYPER)
            flags = flags_twin if round(st["clip_fraction"] * B) == round(st_twin["clip_fraction"] * B) else None
            name = f"{net} B={B}"
            rec[name] = dict(device=T.yardstick("device " + name, pol, data, idx, T.HYPER, g, flags)[0], twin=T.yardstick("twin " + name, pol, data, idx, T.HYPER, g_twin, flags_twin)[0],
                             device_against_twin=T.yardstick("device against the twin " + name, pol, data, idx, T.HYPER, g, flags, g_other=g_twin)[0])
            algo.close(); algo.policy.close()
    if path:
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--learn", type=int, default=0)
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--parity", default=None)
    args = ap.parse_args()
    if args.update:
        rows, per = update_split()
        lines = [f"library: `{lib.load().qs_version().decode()}`", "", "train() in milliseconds, the entries in microseconds per call: median (min .. max) of the repeats; one process, the",
                 "two modes alternating on the same collected rollout (N = 8192, T = 64, 28-64-64-6 tanh)", "", "| what | time |", "|---|---|"]
        lines += [f"| {name} | {fmt(x)} ms |" for name, x in rows] + [f"| {name} | {fmt(x)} us |" for name, x in per]
        rec = update_parity(args.parity)
        lines += ["", "the gradient under tests/ppo_train_ref.py's yardstick: r_peer; the worst elementwise ratio of the device against float64, of the host twin against",
                  "float64 and of the device against the twin; the actor's and the critic's normwise error of the device (of the peer); undecided samples, and how",
                  "many of them were granted slack (0 where the evaluation's own branches were given to float64)", "",
                  "| case | r_peer | device | twin | device / twin | actor (peer) | critic (peer) | undecided | granted |", "|---|---|---|---|---|---|---|---|---|"]
        for k, v in rec.items():
            d = v["device"]
            lines.append(f"| {k} | {d['r_peer']:.3f} | {d['worst']:.3f} | {v['twin']['worst']:.3f} | {v['device_against_twin']['worst']:.3f} | {d['norm']['actor']:.2e} ({d['norm_peer']['actor']:.2e}) | "
                         f"{d['norm']['critic']:.2e} ({d['norm_peer']['critic']:.2e}) | {d['undecided']} | {d['slack_samples']} |")
        text = "\n".join(lines)
        print(text)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        return
    lines = [f"library: `{lib.load().qs_version().decode()}`", "", "(a), (b) in microseconds per call, (c) in milliseconds: median (min .. max) of the repeats", "",
             "| what | time |", "|---|---|"]
    for name, x in collect_step() + gae_step():
        lines.append(f"| {name} | {fmt(x)} us |")
    for name, x in iteration_split():
        lines.append(f"| {name} | {fmt(x)} ms |")
    if args.learn:
        algo = make_algo()
        log = []
        algo.learn(args.learn * algo.n_steps * algo.policy.num_envs, log=log.append)
        lines += ["", "```"] + log + ["```"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
