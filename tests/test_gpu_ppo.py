"""PPO collection on the device (k_actor_critic, k_gae through qs_ac_* / qs_gae and qs_amd.ppo): bitwise against two DevicePolicy objects and
against the host build of csrc/qs_ppo.h, rows and masks, a rollout over a real environment against the same rollout assembled from the
existing parts, the parameter views, stream order, one short learn()."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402
import ppo_ref  # noqa: E402
from emu import emu_ppo  # noqa: E402
from test_gpu_round2 import vec_env  # noqa: E402
from test_policy_cpu import desc_of, ppo_state_dict  # noqa: E402
from test_ppo_cpu import NO_CLIP, pair  # noqa: E402

pytestmark = pytest.mark.gpu

# The rollout test's environments, picked on the CPU oracle (64 environments, 40 steps, settle_steps 100, action_repeat 300: an episode's
# 10 s are 34 steps).  No single configuration tried there gave both kinds of episode end inside 40 steps -- the jumping tasks end every
# episode within a few steps of 300 substeps (64 of 64 environments terminated before step 5, none truncated), the task-free environment
# never terminates (64 of 64 truncated at step 33) -- so the rollout is run on one of each.
ROLLOUT_ENVS = {"truncations": dict(task_env="NO_TASK", enable_action_filter=False, action_repeat=300, settle_steps=100, seed=3),
                "terminations": dict(task_env="JUMPING_IN_PLACE", action_repeat=300, settle_steps=100, seed=3)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def bits(x):
    x = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "cpu") else x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def actor_critic(torch, n, obs_dim, action_dim, arch, vf_arch, activation, pa, pc, log_std):
    from qs_amd import DeviceActorCritic
    ac = DeviceActorCritic(obs_dim, action_dim, net_arch=arch, vf_arch=vf_arch, activation=activation, num_envs=n)
    with torch.no_grad():
        ac.actor_params.copy_(torch.as_tensor(pa.reshape(-1)))
        ac.critic_params.copy_(torch.as_tensor(pc.reshape(-1)))
        ac.log_std.copy_(torch.as_tensor(log_std))
    return ac


# ---- k_gae
@pytest.mark.parametrize("T, N", [(1, 1), (7, 100), (128, 8192)])
def test_gae_equals_the_host_build_bit_for_bit(torch_cuda, T, N):
    torch = torch_cuda
    from qs_amd import DeviceRolloutBuffer
    rng = np.random.default_rng([T, N])
    r, v, es, lv, ld = ppo_ref.gae_data(rng, T, N)
    buf = DeviceRolloutBuffer(T, N, 3, 2, gamma=0.99, gae_lambda=0.95)
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    buf.rewards.copy_(dev(r)); buf.values.copy_(dev(v)); buf.episode_starts.copy_(dev(es))
    buf.compute_returns_and_advantage(dev(lv), dev(ld))
    adv, ret = emu_ppo.gae(r, v, es, lv, ld, 0.99, 0.95)
    assert np.array_equal(bits(buf.advantages), bits(adv)) and np.array_equal(bits(buf.returns), bits(ret))
    buf.compute_returns_and_advantage(dev(lv), dev(ld.astype(bool)))          # bool flags are the same bytes
    assert np.array_equal(bits(buf.advantages), bits(adv))


# ---- qs_ac_collect
@pytest.mark.parametrize("activation, arch, vf_arch, obs_dim, action_dim, n", [("tanh", (64, 64), (64, 64), 28, 6, 8192), ("tanh", (64, 64), (64, 64), 28, 6, 100),
                                                                              ("relu", (33, 7), (16,), 30, 5, 21), ("none", (), (), 28, 12, 40),
                                                                              ("relu", (256, 200), (64,), 64, 4, 50)])
def test_collect_equals_two_device_policies_and_the_host_build(torch_cuda, activation, arch, vf_arch, obs_dim, action_dim, n):
    torch = torch_cuda
    from qs_amd import DevicePolicy
    rng = np.random.default_rng([obs_dim, action_dim, n])
    ka, kc, da, dc = pair(obs_dim, action_dim, arch, vf_arch, activation, n)
    pa, pc = R.make_params(rng, obs_dim, action_dim, arch, True, 1, 3.0), R.make_params(rng, obs_dim, 1, vf_arch, True, 1, 3.0)
    obs, eps = R.make_obs(rng, n, obs_dim), rng.standard_normal((n, action_dim)).astype(np.float32)
    log_std = rng.uniform(-1.5, 0.3, action_dim).astype(np.float32)
    ac = actor_critic(torch, n, obs_dim, action_dim, arch, vf_arch, activation, pa, pc, log_std)
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    T, t_row, canary = 3, 1, 12345.0
    rows = [torch.full((T, n, obs_dim), canary, device="cuda"), torch.full((T, n, action_dim), canary, device="cuda"), torch.full((T, n), canary, device="cuda"),
            torch.full((T, n), canary, device="cuda")]
    d_obs, d_eps = dev(obs), dev(eps)
    env_act = ac.collect(d_obs, d_eps, *[x[t_row] for x in rows])
    # the rows land in row t and nowhere else
    for x in rows:
        assert bool((x[0] == canary).all()) and bool((x[2] == canary).all()) and not bool((x[1] == canary).any())
    # two DevicePolicy objects with the same parameters
    pol = DevicePolicy(obs_dim, action_dim, net_arch=arch, activation=activation, num_envs=n)
    raw = DevicePolicy(obs_dim, action_dim, net_arch=arch, activation=activation, num_envs=n, clip=None)
    val = DevicePolicy(obs_dim, 1, net_arch=vf_arch, activation=activation, num_envs=n, clip=None)
    pol.set_params(pa); raw.set_params(pa); val.set_params(pc)
    d_ls = dev(log_std)
    a_clip, _, lp = pol.act(d_obs, d_eps, d_ls, want_log_prob=True)
    assert np.array_equal(bits(env_act), bits(a_clip)) and np.array_equal(bits(rows[3][t_row]), bits(lp))
    assert np.array_equal(bits(rows[1][t_row]), bits(raw.act(d_obs, d_eps, d_ls)))
    assert np.array_equal(bits(rows[2][t_row]), bits(val.act(d_obs, want_mean=True)[1][:, 0]))
    assert np.array_equal(bits(rows[0][t_row]), bits(obs))
    assert np.array_equal(bits(ac.predict_values(d_obs)), bits(rows[2][t_row]))
    # the host build
    e_env, e_act, e_val, e_lp = emu_ppo.collect(da, dc, pa, pc, obs, eps, log_std)
    assert np.array_equal(bits(rows[3][t_row]), bits(e_lp))
    if activation != "tanh":
        assert np.array_equal(bits(rows[2][t_row]), bits(e_val))
        if activation == "none":          # (expf in the sample is the platform's: only the mean is compared bitwise otherwise)
            assert np.allclose(rows[1][t_row].cpu().numpy(), e_act, rtol=1e-6, atol=1e-6)
    else:
        c = R.tanh_c()
        v64, v_bound = R.forward(pc, obs, obs_dim, 1, vf_arch, activation, False, True, 1, c)
        m64, m_bound = R.forward(pa, obs, obs_dim, action_dim, arch, activation, False, True, 1, c)
        assert np.all(np.abs(rows[2][t_row].cpu().numpy() - v64[:, 0]) <= v_bound[:, 0])
        std = np.exp(log_std.astype(np.float64))
        a64 = m64 + std * eps.astype(np.float64)
        assert np.all(np.abs(rows[1][t_row].cpu().numpy() - a64) <= m_bound + 6 * R.U * std * np.abs(eps) + R.U * np.abs(a64))
    for p in (pol, raw, val, ac):
        p.close()


# ---- the masked critic
def test_values_and_bootstrap_honour_the_mask(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(21)
    n = 1000
    ka, kc, da, dc = pair(28, 6, (64, 64), (64, 64), "relu", n)
    pa, pc = R.make_params(rng, 28, 6, (64, 64), True, 1, 3.0), R.make_params(rng, 28, 1, (64, 64), True, 1, 3.0)
    ac = actor_critic(torch, n, 28, 6, (64, 64), (64, 64), "relu", pa, pc, np.zeros(6, np.float32))
    obs, rew = R.make_obs(rng, n, 28), rng.standard_normal(n).astype(np.float32)
    mask = (rng.random(n) < 0.05).astype(np.uint8)
    mask[16:64] = 0                                              # whole tiles without a masked environment
    mask[999] = 1                                                # the last, partial tile
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    out = torch.full((n,), 7.0, device="cuda")
    ac.predict_values(dev(obs), mask=dev(mask), out=out)
    assert np.array_equal(bits(out), bits(emu_ppo.values(dc, pc, obs, mask=mask, out=np.full(n, 7.0, np.float32))))
    d_rew = dev(rew)
    ac.bootstrap(dev(obs), dev(mask), 0.99, d_rew)
    assert np.array_equal(bits(d_rew), bits(emu_ppo.bootstrap(dc, pc, obs, mask, np.float32(0.99), rew)))
    assert bool((d_rew.cpu() != torch.as_tensor(rew)).any())
    # an all-zero mask writes nothing
    zero = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out.fill_(7.0)
    d_rew = dev(rew)
    ac.predict_values(dev(obs), mask=zero, out=out)
    ac.bootstrap(dev(obs), zero, 0.99, d_rew)
    assert bool((out == 7.0).all()) and np.array_equal(bits(d_rew), bits(rew))
    ac.close()


# ---- a rollout over a real environment
@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("ends", sorted(ROLLOUT_ENVS))
def test_collect_rollouts_equals_the_rollout_assembled_from_existing_parts(torch_cuda, ends, normalised):
    torch = torch_cuda
    from qs_amd import DeviceActorCritic, DevicePolicy, DevicePPO, DeviceVecNormalize
    N, T, gamma = 64, 40, 0.99

    def make_env():
        env = vec_env(N, auto_reset=True, **ROLLOUT_ENVS[ends])
        return DeviceVecNormalize(env, training=True) if normalised else env
    env = make_env()
    torch.manual_seed(5)
    ac = DeviceActorCritic(env.obs_dim, env.action_dim, num_envs=N, log_std_init=-0.5)
    with torch.no_grad():
        ac.critic[-1].bias.fill_(2.0)                            # values that a bootstrap visibly adds
    algo = DevicePPO(env, ac, n_steps=T, gamma=gamma, seed=11)
    algo.collect_rollouts()
    buf = algo.buffer

    # the same rollout, step by step, from two DevicePolicy objects, step_tensor and torch arithmetic
    env2 = make_env()
    A = env2.action_dim
    pol = DevicePolicy(env2.obs_dim, A, num_envs=N)
    raw = DevicePolicy(env2.obs_dim, A, num_envs=N, clip=None)
    val = DevicePolicy(env2.obs_dim, 1, num_envs=N, clip=None)
    pol.set_params(ac.actor_params.clone()); raw.set_params(ac.actor_params.clone()); val.set_params(ac.critic_params.clone())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    eps = torch.randn((T, N, A), dtype=torch.float32, device="cuda", generator=gen)
    log_std = ac.log_std.detach().clone()
    obs = env2.reset_tensor()
    starts = torch.ones(N, device="cuda")
    n_trunc = n_term = 0
    f64 = torch.float64
    for t in range(T):
        a_clip, _, lp = pol.act(obs, eps[t], log_std, want_log_prob=True)
        want = dict(observations=obs.clone(), actions=raw.act(obs, eps[t], log_std).clone(), log_probs=lp.clone(),
                    values=val.act(obs, want_mean=True)[1][:, 0].clone(), episode_starts=starts.clone())
        if normalised:
            term = torch.zeros((N, env2.obs_dim), device="cuda")
            obs, rew, done, trunc = env2.step_tensor(a_clip, terminal_obs=term)
        else:
            obs, rew, done, trunc = env2.step_tensor(a_clip)
            term = env2.get_info("terminal_obs")
        v_term = val.act(term, want_mean=True)[1][:, 0]
        # fmaf(gamma, v, r): the float32 product is exact in float64, the sum rounds once to float32
        boot = (float(np.float32(gamma)) * v_term.to(f64) + rew.to(f64)).to(torch.float32)
        want["rewards"] = torch.where(trunc.bool(), boot, rew)
        for name, w in want.items():
            assert np.array_equal(bits(getattr(buf, name)[t]), bits(w)), (name, t)
        n_trunc += int(trunc.sum()); n_term += int((done.bool() & ~trunc.bool()).sum())
        starts = done.to(torch.float32)
    assert (n_trunc if ends == "truncations" else n_term) > 0, (n_trunc, n_term)
    last_v = val.act(obs, want_mean=True)[1][:, 0]
    adv, ret = emu_ppo.gae(buf.rewards.cpu().numpy(), buf.values.cpu().numpy(), buf.episode_starts.cpu().numpy(), last_v.cpu().numpy(), done.cpu().numpy(), gamma, 0.95)
    assert np.array_equal(bits(buf.advantages), bits(adv)) and np.array_equal(bits(buf.returns), bits(ret))
    # the printed statistic: the raw returns of the episodes that ended, against a host loop
    ret_sum, count = algo.episode_stats()
    raw_rew, dones = algo._raw_rewards.cpu().numpy().astype(np.float64), np.concatenate([buf.episode_starts[1:].cpu().numpy(), done.cpu().numpy()[None]], 0) > 0
    run, total, k = np.zeros(N), 0.0, 0
    for t in range(T):
        run += raw_rew[t]
        total += run[dones[t]].sum(); k += int(dones[t].sum()); run[dones[t]] = 0.0
    assert int(count) == k == n_trunc + n_term and abs(float(ret_sum) - total) <= 1e-3 * max(1.0, abs(total))
    for p in (pol, raw, val, ac):
        p.close()
    env.close(); env2.close()


# ---- the parameter views on the device
def test_an_optimiser_step_changes_the_next_collect_without_set_params(torch_cuda):
    torch = torch_cuda
    from qs_amd import DeviceActorCritic
    torch.manual_seed(1)
    n = 128
    ac = DeviceActorCritic(28, 6, num_envs=n)
    vec = torch.nn.utils.parameters_to_vector
    assert torch.equal(vec(ac.actor.parameters()), ac.actor_params) and ac.actor[0].weight.data_ptr() == ac.actor_params.data_ptr()
    obs, eps = torch.randn(n, 28, device="cuda"), torch.randn(n, 6, device="cuda")
    rows = [torch.zeros(n, 28, device="cuda"), torch.zeros(n, 6, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    a0, v0 = ac.collect(obs, eps, *rows).clone(), rows[2].clone()
    assert torch.equal(ac.collect(obs, eps, *rows), a0)
    opt = torch.optim.Adam(ac.parameters(), lr=1e-2, eps=1e-5)
    values, log_prob, _ = ac.evaluate_actions(obs, rows[1].clone())
    assert torch.allclose(values, v0, atol=1e-4) and torch.allclose(log_prob, rows[3], atol=1e-3)
    (values.sum() - log_prob.sum()).backward()
    opt.step()
    a1 = ac.collect(obs, eps, *rows)
    assert not torch.equal(a1, a0) and not torch.equal(rows[2], v0)
    # what the kernel computed is the stepped torch module's forward
    with torch.no_grad():
        want = (ac.actor(obs) + ac.log_std.exp() * eps).clamp(-1.0, 1.0)
    assert torch.allclose(a1, want, atol=1e-5)
    ac.close()


# ---- stream order
def test_collect_behind_the_step_on_a_side_stream_needs_no_synchronisation(torch_cuda):
    torch = torch_cuda
    from qs_amd import DeviceActorCritic
    rng = np.random.default_rng(12)
    n = 512
    env = vec_env(n)
    ac = DeviceActorCritic.from_state_dict(ppo_state_dict(rng, env.obs_dim, env.action_dim), num_envs=n)
    env.reset_tensor()
    a0 = torch.as_tensor(rng.uniform(-1, 1, (n, env.action_dim)).astype(np.float32), device="cuda")
    eps = torch.randn(n, env.action_dim, device="cuda")
    mk = lambda: [torch.zeros(n, env.obs_dim, device="cuda"), torch.zeros(n, env.action_dim, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]  # noqa: E731
    rows, rows2 = mk(), mk()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        obs = env.step_tensor(a0)[0]
        act = ac.collect(obs, eps, *rows).clone()                # enqueued behind the step, nothing waited for
        obs_h = obs.clone()
    torch.cuda.synchronize()
    assert np.array_equal(bits(ac.collect(obs_h, eps, *rows2)), bits(act))
    for x, y in zip(rows, rows2):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(rows[0]), bits(obs_h))
    ac.close(); env.close()


# ---- the whole loop
def test_three_iterations_of_learn_leave_finite_parameters(torch_cuda):
    torch = torch_cuda
    from qs_amd import DeviceActorCritic, DevicePPO, DeviceVecNormalize
    env = DeviceVecNormalize(vec_env(256, auto_reset=True, env_randomizer_mode="GROUND_RANDOMIZER"), training=True)
    torch.manual_seed(2)
    ac = DeviceActorCritic(env.obs_dim, env.action_dim, num_envs=256)
    before = ac.actor_params.clone()
    algo = DevicePPO(env, ac, n_steps=16, batch_size=1024, n_epochs=2, seed=2)
    lines = []
    algo.learn(3 * 16 * 256, log=lines.append)
    print("\n".join(lines))
    assert len(lines) == 3 and algo.num_timesteps == 3 * 16 * 256
    assert bool(torch.isfinite(ac.actor_params).all()) and bool(torch.isfinite(ac.critic_params).all()) and bool(torch.isfinite(ac.log_std).all())
    assert not torch.equal(ac.actor_params, before)
    ac.close(); env.close()
