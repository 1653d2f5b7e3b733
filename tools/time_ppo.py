#!/usr/bin/env python3
"""What PPO collection costs on the stream (profiles/ppo_collect.md).  Same process, warm, HIP events around many enqueues with the
stream kept busy, median and spread (min .. max) of the repeats:
(a) per collected step at N = 8192, 28-64-64-6 tanh: qs_ac_collect (one launch) against the assembly it replaces -- two DevicePolicy.act
    launches (clipped action + log-prob, value) and the torch copies of observation, action, value and log-prob into [T, N, ...] storage;
(b) k_gae at T = 128 against the torch loop of the same recurrence on the device;
(c) one DevicePPO iteration with examples/ppo.py's defaults, split into collect, GAE and train();
(d) with --learn K: the return per iteration of K iterations of examples/ppo.py's configuration.

    python tools/time_ppo.py [--out profiles/ppo_collect.md] [--learn 10]"""
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


def make_algo(envs=8192, n_steps=64, batch_size=65536, epochs=10):
    venv = QuadrupedVecEnv(num_envs=envs, device=0, auto_reset=True, task_env="JUMPING_IN_PLACE_PPO", observation_space_mode="PPO_BASIC",
                           action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True, enable_action_filter=True,
                           env_randomizer_mode="GROUND_RANDOMIZER")
    env = DeviceVecNormalize(venv, training=True)
    torch.manual_seed(0)
    policy = DeviceActorCritic(env.obs_dim, env.action_dim, num_envs=envs)
    return DevicePPO(env, policy, n_steps=n_steps, batch_size=batch_size, n_epochs=epochs, seed=0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--learn", type=int, default=0)
    args = ap.parse_args()
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
