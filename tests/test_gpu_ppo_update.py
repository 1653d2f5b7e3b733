"""The PPO update on the device (qs_ppo_*, csrc/qs_ppo_train.hip; DevicePPO(update="device")) against float64 autograd and the host twin
under tests/ppo_train_ref.py's yardstick, at the shapes of tests/test_ppo_update_cpu.py; clip + Adam in place on the DeviceActorCritic's own
memory; train() in both modes against a float64 loop; stream order; learn()."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_train_ref as T  # noqa: E402
from emu import emu_ppo_train as E  # noqa: E402
from test_gpu_round2 import vec_env  # noqa: E402
from test_ppo_update_cpu import descs, twin_grad  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = 12345.5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).view(np.int32)


def guarded(torch, n):
    """-> (whole, view): a float32 tensor with 64 canaries either side of the n entries the view covers"""
    whole = torch.full((n + 128,), CANARY, device="cuda")
    return whole, whole[64:64 + n]


def intact(whole, n):
    w = whole.cpu().numpy()
    return bool((w[:64] == CANARY).all() and (w[64 + n:] == CANARY).all())


@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("net", sorted(T.NETS))
def test_the_gradient_under_the_yardstick_and_against_the_host_twin(torch_cuda, net, B):
    torch = torch_cuda
    import qs_amd.lib as lib
    pol, data, idx = T.case(net, B)
    hy = dict(T.HYPER, max_grad_norm=0.5)
    algo = T.learner(pol, data, 1, B + 7, update="device", batch_size=B, clip_range=hy["clip_range"], ent_coef=hy["ent_coef"], vf_coef=hy["vf_coef"])
    n = algo.grad.numel()
    g_whole, algo.grad = guarded(torch, n)
    s_whole, algo._stats = guarded(torch, len(lib.PPO_STATS))
    ix = torch.as_tensor(idx, device="cuda")
    algo.grad_minibatch(ix)
    g1, s1 = algo.grad.clone(), algo._stats.clone()
    algo.grad_minibatch(ix)
    torch.cuda.synchronize()
    assert intact(g_whole, n) and intact(s_whole, len(lib.PPO_STATS)), "a canary next to grad_out / stats_out was overwritten"
    assert np.array_equal(bits(g1), bits(algo.grad)) and np.array_equal(bits(s1), bits(algo._stats)), "two calls gave different bits"
    g = algo.grad.cpu().numpy()
    st = algo._read_stats()
    _, st64 = T.autograd(pol, data, idx, T.HYPER, torch.float64)
    _, st_peer = T.autograd(pol, data, idx, T.HYPER, torch.float32)
    g_twin, st_twin, _ = twin_grad(pol, data, idx, T.HYPER)
    # the device's branch decisions are the twin's when both count the same clipped samples; held against the twin first, with nothing granted
    # then, so a decision that differs all the same shows as an error of a whole sample.  Otherwise: not known, the clip-edge samples' policy terms
    flags = E.grad.last_flags if round(st["clip_fraction"] * B) == round(st_twin["clip_fraction"] * B) else None
    T.yardstick(f"device against the twin {net} B={B}", pol, data, idx, T.HYPER, g, flags, g_other=g_twin)
    _, ref = T.yardstick(f"device {net} B={B}", pol, data, idx, T.HYPER, g, flags)
    T.hold_stats(f"device {net} B={B}", st, ref, st_peer, st64, B)
    algo.close(); algo.policy.close()


def test_indices_out_of_range_are_refused_not_read(torch_cuda):
    torch = torch_cuda
    n_steps, num_envs = 3, 100
    total = n_steps * num_envs
    pol = T.make_policy(T.NETS["tanh-28-64x64-6"], 3)
    data = T.make_data(pol, total, 3)
    hyper = dict(T.HYPER, normalize_advantage=False)
    good = np.random.default_rng(3).permutation(total)[:60].astype(np.int64)
    idx = good.copy()
    bad = {4: -1, 17: total, 33: 2 ** 40, 59: -2 ** 62}
    for k, v in bad.items():
        idx[k] = v
    valid = np.array([k for k in range(idx.size) if k not in bad])
    algo = T.learner(pol, data, n_steps, num_envs, update="device", batch_size=idx.size, clip_range=hyper["clip_range"], ent_coef=hyper["ent_coef"],
                   vf_coef=hyper["vf_coef"], normalize_advantage=False)
    algo.grad_minibatch(torch.as_tensor(idx, device="cuda"))
    torch.cuda.synchronize()
    g_bad = algo.grad.clone()
    with pytest.raises(RuntimeError, match="refused 4 samples"):
        algo._read_stats()
    count = C.c_uint64(99)
    assert algo.lib.qs_ppo_refusals(algo.hp, C.byref(count)) == 0 and count.value == 0          # (the read cleared the counter)
    # a refusal in an EARLIER minibatch is reported at the next read as well
    algo.grad_minibatch(torch.as_tensor(idx, device="cuda"))
    algo.grad_minibatch(torch.as_tensor(good, device="cuda"))
    assert float(algo._stats.cpu()[6]) == 0.0
    with pytest.raises(RuntimeError, match="refused 4 samples"):
        algo._read_stats()
    algo._read_stats()
    algo.grad_minibatch(torch.as_tensor(idx, device="cuda"))
    assert algo.lib.qs_ppo_refusals(algo.hp, C.byref(count)) == 0 and count.value == 4
    assert np.array_equal(bits(algo.grad), bits(g_bad))
    # the other samples' gradient: the float64 restatement over them, with B = 60 the divisor
    ref = T.restate(pol, data, idx[valid], hyper, batch=idx.size)
    scale = valid.size / idx.size

    def auto(dtype):
        g, _ = T.autograd(pol, data, idx[valid], dict(hyper, ent_coef=hyper["ent_coef"] / scale), dtype)
        return g * scale
    g64 = auto(torch.float64)
    assert np.max(np.abs(g64 - ref["g"])) <= 1e-9
    peer = T.measure(auto(torch.float32), ref, g64)
    assert not ref["undecided"].any()
    T.hold("refused", algo.grad.cpu().numpy(), ref, peer, g64)
    # with the normalisation on as well: no fault, the same count
    algo.normalize_advantage = True
    algo.grad_minibatch(torch.as_tensor(idx, device="cuda"))
    assert float(algo._stats.cpu()[6]) == 4.0 and bool(torch.isfinite(algo.grad).all())
    assert algo.lib.qs_ppo_refusals(algo.hp, C.byref(count)) == 0 and count.value == 4
    algo.close(); algo.policy.close()


@pytest.mark.parametrize("max_grad_norm", [0.1, 1e4])
def test_adam_in_place_on_the_policys_memory(torch_cuda, max_grad_norm):
    torch = torch_cuda
    B = 100
    pol, data, idx = T.case("tanh-28-64x64-6", B)
    algo = T.learner(pol, data, 1, B + 7, update="device", batch_size=B, max_grad_norm=max_grad_norm, learning_rate=1e-2)
    dev = algo.policy
    ptrs = (dev.actor_params.data_ptr(), dev.critic_params.data_ptr(), dev.log_std.data_ptr(), dev.actor[0].weight.data_ptr())
    flat = lambda: torch.cat([dev.actor_params, dev.critic_params, dev.log_std.detach()]).cpu().numpy()  # noqa: E731
    n, o, a = dev.num_envs, dev.obs_dim, dev.action_dim
    obs, eps = torch.as_tensor(data["observations"], device="cuda"), torch.randn(n, a, device="cuda")
    rows = [torch.zeros(n, o, device="cuda"), torch.zeros(n, a, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    a0 = dev.collect(obs, eps, *rows).clone()
    ix = torch.as_tensor(idx, device="cuda")
    hy = E.hyper(max_grad_norm=max_grad_norm, lr=1e-2)
    for step in (1, 2, 3):
        p0, m0, v0 = flat(), algo.exp_avg.cpu().numpy(), algo.exp_avg_sq.cpu().numpy()
        algo.grad_minibatch(ix)
        g = algo.grad.cpu().numpy()
        algo.adam_minibatch()
        p1, m1, v1 = flat(), algo.exp_avg.cpu().numpy(), algo.exp_avg_sq.cpu().numpy()
        norm = algo._read_stats()["grad_norm"]
        assert (norm > max_grad_norm) == (max_grad_norm == 0.1), norm
        tp, tm, tv, tnorm = E.adam(p0, m0, v0, g, hy, step)
        p64, m64, v64, norm64, bound, dm, dv = T.adam64(p0, m0, v0, g, step, lr=1e-2, max_grad_norm=max_grad_norm)
        assert abs(norm - norm64) <= 300 * T.U * norm64 and abs(norm - tnorm) <= 4 * T.U * norm64
        assert np.all(np.abs(p1 - p64) <= bound), float(np.max(np.abs(p1 - p64) / bound))
        assert np.all(np.abs(p1 - tp.astype(np.float64)) <= 2 * bound)
        assert np.all(np.abs(m1 - m64) <= dm) and np.all(np.abs(v1 - v64) <= dv)
    assert ptrs == (dev.actor_params.data_ptr(), dev.critic_params.data_ptr(), dev.log_std.data_ptr(), dev.actor[0].weight.data_ptr())
    a1 = dev.collect(obs, eps, *rows)
    assert not torch.equal(a1, a0)
    with torch.no_grad():
        want = (dev.actor(obs) + dev.log_std.exp() * eps).clamp(-1.0, 1.0)
    assert torch.allclose(a1, want, atol=1e-5)
    algo.close(); dev.close()


def float64_loop(torch, pol, data, minibatches, kw):
    """PPO.train's steps in float64 on the CPU over the given minibatches -> flat parameters [actor | critic | log_std]"""
    from qs_amd.ppo import ppo_loss
    c = T.copy_of(pol, torch.float64)
    opt = torch.optim.Adam(c.parameters(), lr=kw["learning_rate"], eps=1e-5)
    d = {k: torch.as_tensor(v).double() for k, v in data.items()}
    for idx in minibatches:
        values, log_prob, entropy = c.evaluate_actions(d["observations"][idx], d["actions"][idx])
        loss, _ = ppo_loss(values, log_prob, entropy, values.detach(), d["old_log_prob"][idx], d["advantages"][idx], d["returns"][idx], 0.2, None, 0.0, 0.5, True)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(c.parameters(), 0.5)
        opt.step()
    return torch.cat([p.detach().reshape(-1) for p in c.parameters()]).numpy()


@pytest.mark.parametrize("batch_size, n_epochs", [(1024, 3), (256, 2)])
def test_train_in_both_modes_against_a_float64_loop(torch_cuda, batch_size, n_epochs):
    torch = torch_cuda
    n_steps, num_envs = 8, 128
    total = n_steps * num_envs
    pol = T.make_policy(T.NETS["tanh-28-64x64-6"], 5)
    data = T.make_data(pol, total, 5)
    kw = dict(batch_size=batch_size, n_epochs=n_epochs, learning_rate=1e-3, seed=7)
    algos = {u: T.learner(pol, data, n_steps, num_envs, update=u, **kw) for u in ("device", "torch")}
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    minibatches = []
    for _ in range(n_epochs):
        perm = torch.randperm(total, device="cuda", generator=gen).cpu()
        minibatches += [perm[s:s + batch_size] for s in range(0, total, batch_size)]
    infos = {u: a.train() for u, a in algos.items()}
    assert list(infos["device"]) == list(infos["torch"]) and infos["device"]["n_epochs_run"] == infos["torch"]["n_epochs_run"] == n_epochs
    p64 = float64_loop(torch, pol, data, minibatches, kw)
    flat = lambda a: torch.cat([a.policy.actor_params, a.policy.critic_params, a.policy.log_std.detach()]).cpu().numpy().astype(np.float64)  # noqa: E731
    na, nc = pol.actor_params.numel(), pol.critic_params.numel()
    nets = dict(actor=np.r_[0:na, na + nc:na + nc + pol.action_dim], critic=np.r_[na:na + nc])
    for k, ix in nets.items():
        d_dev, d_torch = np.max(np.abs(flat(algos["device"]) - p64)[ix]), np.max(np.abs(flat(algos["torch"]) - p64)[ix])
        print(f"train bs={batch_size} {k}: device {d_dev:.3e}  torch {d_torch:.3e} from the float64 loop")
        assert d_dev <= T.FACTOR * d_torch and d_torch <= T.FACTOR * d_dev, (k, d_dev, d_torch)
        assert np.max(np.abs(p64 - flat(algos["torch"]))[ix]) < 1e-2 and np.max(np.abs(p64[ix] - np.concatenate([pol.actor_params.detach().numpy(), pol.critic_params.detach().numpy(), pol.log_std.detach().numpy()])[ix])) > 1e-4
    for k in ("policy_loss", "value_loss", "approx_kl", "clip_fraction", "grad_norm"):
        assert abs(infos["device"][k] - infos["torch"][k]) <= 1e-3 * (1.0 + abs(infos["torch"][k])), (k, infos)
    for a in algos.values():
        a.close(); a.policy.close()


def test_target_kl_stops_both_modes_in_the_same_epoch(torch_cuda):
    """old_log_prob is the policy's own log-prob, so approx_kl starts at 0 and grows with every step: with the whole buffer as the minibatch
    and learning_rate 3e-3 it is 0.0019 before the second step and 0.0073 before the third (torch, CPU).  target_kl = 0.003 (the stop is at
    1.5 x) lets two real Adam steps through and skips the third, in both modes; at 1e-4 one step goes through."""
    torch = torch_cuda
    pol = T.make_policy(T.NETS["tanh-28-64x64-6"], 5)
    data = T.make_data(pol, 1024, 5)
    with torch.no_grad():
        c = T.copy_of(pol, torch.float64)
        data["old_log_prob"] = c.evaluate_actions(torch.as_tensor(data["observations"]).double(), torch.as_tensor(data["actions"]).double())[1].numpy().astype(np.float32)
    for target_kl, epochs in ((0.003, 2), (1e-4, 1)):
        out, params = {}, {}
        for u in ("device", "torch"):
            a = T.learner(pol, data, 8, 128, update=u, batch_size=1024, n_epochs=6, learning_rate=3e-3, seed=7, target_kl=target_kl)
            out[u] = a.train()
            params[u] = torch.cat([a.policy.actor_params, a.policy.critic_params, a.policy.log_std.detach()]).cpu().numpy()
            if u == "device":
                assert a.adam_step == epochs
            a.close(); a.policy.close()
        print(target_kl, out)
        assert out["device"]["n_epochs_run"] == out["torch"]["n_epochs_run"] == epochs and list(out["device"]) == list(out["torch"])
        assert np.isnan(out["device"]["grad_norm"]) and np.isnan(out["torch"]["grad_norm"])
        assert abs(out["device"]["approx_kl"] - out["torch"]["approx_kl"]) <= 1e-3 * out["torch"]["approx_kl"] + 1e-7
        assert np.max(np.abs(params["device"] - params["torch"])) <= 1e-5
        assert (np.max(np.abs(params["device"] - np.concatenate([pol.actor_params.detach().numpy(), pol.critic_params.detach().numpy(), pol.log_std.detach().numpy()]))) > 1e-3) == (epochs > 0)


def test_train_behind_a_rollout_on_a_side_stream_needs_no_synchronisation(torch_cuda):
    torch = torch_cuda
    from qs_amd import DeviceActorCritic, DevicePPO

    def run(stream):
        env = vec_env(256, auto_reset=True)
        torch.manual_seed(4)
        ac = DeviceActorCritic(env.obs_dim, env.action_dim, num_envs=256)
        algo = DevicePPO(env, ac, n_steps=4, batch_size=512, n_epochs=2, seed=4, update="device")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            algo.collect_rollouts()
            algo.train()                                   # enqueued behind the rollout, nothing waited for in between
            out = torch.cat([ac.actor_params, ac.critic_params, ac.log_std.detach(), algo.grad]).clone()
        torch.cuda.synchronize()
        algo.close(); ac.close(); env.close()
        return out
    assert np.array_equal(bits(run(torch.cuda.Stream())), bits(run(torch.cuda.current_stream())))


def test_three_iterations_of_learn_with_the_device_update(torch_cuda):
    torch = torch_cuda
    from qs_amd import DeviceActorCritic, DevicePPO, DeviceVecNormalize
    env = DeviceVecNormalize(vec_env(256, auto_reset=True, env_randomizer_mode="GROUND_RANDOMIZER"), training=True)
    torch.manual_seed(2)
    ac = DeviceActorCritic(env.obs_dim, env.action_dim, num_envs=256)
    before = [ac.actor_params.clone(), ac.critic_params.clone(), ac.log_std.detach().clone()]
    algo = DevicePPO(env, ac, n_steps=16, batch_size=1024, n_epochs=2, seed=2, update="device")
    lines = []
    algo.learn(3 * 16 * 256, log=lines.append)
    print("\n".join(lines))
    assert len(lines) == 3 and algo.num_timesteps == 3 * 16 * 256 and algo.adam_step == 3 * 2 * 4
    for now, was in zip((ac.actor_params, ac.critic_params, ac.log_std.detach()), before):
        assert bool(torch.isfinite(now).all()) and not torch.equal(now, was)
    algo.close(); ac.close(); env.close()
