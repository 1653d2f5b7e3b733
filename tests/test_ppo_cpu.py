"""PPO collection without a GPU: the host build of csrc/qs_ppo.h (tests/emu/qs_emu_ppo.cpp) -- GAE against float64 under the
bound derived in tests/ppo_ref.py, the actor-critic against two policies of the host build of csrc/qs_policy.h, the bootstrap --, the
parameter views of DeviceActorCritic, ppo_loss against numpy, and train() on a fabricated buffer."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import policy_ref as R  # noqa: E402
import ppo_ref  # noqa: E402
from emu import emu_policy, emu_ppo  # noqa: E402
from test_policy_cpu import desc_of, ppo_state_dict  # noqa: E402

NO_CLIP = (-3.0e38, 3.0e38)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def pair(obs_dim=28, action_dim=6, net_arch=(64, 64), vf_arch=(64, 64), activation="tanh", n=40):
    """(actor kw, critic kw, actor desc, critic desc) of a PPO MlpPolicy with separate trunks"""
    ka = dict(obs_dim=obs_dim, action_dim=action_dim, net_arch=net_arch, activation=activation, squash_output=False, bias=True, n_policies=1)
    kc = dict(ka, action_dim=1, net_arch=vf_arch)
    return ka, kc, desc_of(ka, n), desc_of(kc, n, NO_CLIP)


# ---- 1. the package
def test_the_package_exports_the_ppo_classes():
    import qs_amd
    from qs_amd import ppo
    for name in ("DeviceActorCritic", "DeviceRolloutBuffer", "DevicePPO", "ppo_loss"):
        assert getattr(qs_amd, name) is getattr(ppo, name)


@pytest.mark.parametrize("who, change, word", [("actor", dict(n_policies=2), "n_policies"), ("critic", dict(n_envs=48), "n_envs"), ("critic", dict(obs_dim=27), "obs_dim"),
                                               ("critic", dict(action_dim=2), "action_dim"), ("critic", dict(squash_output=1), "squash"),
                                               ("critic", dict(clip_lo=-1.0), "finite clips"), ("critic", dict(clip_hi=1.0), "finite clips")])
def test_pairs_qs_ac_create_refuses_with_their_reason(who, change, word):
    _, _, da, dc = pair()
    for k, v in change.items():
        setattr(da if who == "actor" else dc, k, v)
    with pytest.raises(ValueError, match=word):
        emu_ppo.check(da, dc)
    emu_ppo.check(*pair()[2:])


# ---- 2. GAE of the host build
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("T, N", [(1, 5), (16, 33), (128, 64)])
def test_gae_against_float64_under_the_derived_bound(T, N, lam):
    rng = np.random.default_rng([T, N, int(lam * 100)])
    data = ppo_ref.gae_data(rng, T, N)
    assert T == 1 or (data[2].any() and data[4].any() and not data[4].all())
    adv, ret = emu_ppo.gae(*data, 0.99, lam)
    adv64, ret64, adv_bound, ret_bound = ppo_ref.gae(*data, 0.99, lam)
    ra, rr = np.max(np.abs(adv - adv64) / adv_bound), np.max(np.abs(ret - ret64) / ret_bound)
    print(f"T = {T}, N = {N}, lambda = {lam}: max err / bound = {ra:.3g} (advantages), {rr:.3g} (returns); largest bound {adv_bound.max():.3g}")
    assert ra <= 1.0 and rr <= 1.0, (ra, rr)
    assert adv_bound.max() < 1e-4 * max(1.0, np.abs(adv64).max())      # (the bound says something)


def test_gae_restarts_at_episode_starts_and_at_last_done():
    """an episode start at t + 1 cuts step t off from everything later: advantage[t] = reward[t] - value[t]"""
    rng = np.random.default_rng(3)
    r, v, es, lv, ld = ppo_ref.gae_data(rng, 12, 8, p_start=0.3)
    adv, ret = emu_ppo.gae(r, v, es, lv, ld, 0.99, 0.95)
    cut = np.concatenate([es[1:], ld[None].astype(np.float32)], 0) > 0
    assert cut.any()
    assert np.array_equal(bits(adv[cut]), bits((r - v)[cut]))
    assert np.array_equal(bits(ret), bits(adv + v))


def test_gae_on_exactly_representable_inputs_is_bit_for_bit():
    rng = np.random.default_rng(4)
    T, N = 8, 50
    r, v = rng.integers(-4, 5, (T, N)).astype(np.float32), rng.integers(-4, 5, (T, N)).astype(np.float32)
    es, lv, ld = (rng.random((T, N)) < 0.2).astype(np.float32), rng.integers(-4, 5, N).astype(np.float32), (rng.random(N) < 0.3).astype(np.uint8)
    adv, ret = emu_ppo.gae(r, v, es, lv, ld, 0.5, 0.5)
    adv64, ret64, _, _ = ppo_ref.gae(r, v, es, lv, ld, 0.5, 0.5)
    assert np.array_equal(adv64.astype(np.float32).astype(np.float64), adv64)       # (float32 holds the exact results)
    assert np.array_equal(bits(adv), bits(adv64.astype(np.float32))) and np.array_equal(bits(ret), bits(ret64.astype(np.float32)))


# ---- 3. the actor-critic of the host build
@pytest.mark.parametrize("activation, arch, vf_arch, obs_dim, action_dim, n", [("tanh", (64, 64), (64, 64), 28, 6, 40), ("relu", (33, 7), (16,), 30, 5, 21),
                                                                              ("none", (), (), 28, 12, 16), ("tanh", (256, 200), (64,), 64, 4, 17)])
def test_collect_equals_two_policies_bit_for_bit(activation, arch, vf_arch, obs_dim, action_dim, n):
    rng = np.random.default_rng([obs_dim, action_dim, n])
    ka, kc, da, dc = pair(obs_dim, action_dim, arch, vf_arch, activation, n)
    pa = R.make_params(rng, obs_dim, action_dim, arch, True, 1, 3.0)
    pc = R.make_params(rng, obs_dim, 1, vf_arch, True, 1, 3.0)
    obs, eps = R.make_obs(rng, n, obs_dim), rng.standard_normal((n, action_dim)).astype(np.float32)
    log_std = rng.uniform(-1.5, 0.3, action_dim).astype(np.float32)
    env_act, act, val, lp = emu_ppo.collect(da, dc, pa, pc, obs, eps, log_std)
    clipped, mean, want_lp = emu_policy.act(da, pa, obs, eps, log_std)
    unclipped = emu_policy.act(desc_of(ka, n, NO_CLIP), pa, obs, eps, log_std)[0]
    value = emu_policy.act(dc, pc, obs)[1]
    assert np.array_equal(bits(env_act), bits(clipped)) and np.array_equal(bits(act), bits(unclipped))
    assert np.array_equal(bits(lp), bits(want_lp)) and np.array_equal(bits(val), bits(value[:, 0]))
    assert np.any(act != env_act) and np.all(np.abs(env_act) <= 1.0)
    assert np.array_equal(bits(emu_ppo.values(dc, pc, obs)), bits(val))


# ---- 4. the bootstrap
def test_bootstrap_changes_only_truncated_rows_by_the_stated_fmaf():
    rng = np.random.default_rng(6)
    n = 50
    _, kc, _, dc = pair(n=n)
    pc = R.make_params(rng, 28, 1, (64, 64), True, 1, 3.0)
    term, rew = R.make_obs(rng, n, 28), rng.standard_normal(n).astype(np.float32)
    trunc = (rng.random(n) < 0.3).astype(np.uint8)
    gamma = np.float32(0.99)
    got = emu_ppo.bootstrap(dc, pc, term, trunc, gamma, rew)
    v = emu_ppo.values(dc, pc, term)
    on = trunc > 0
    assert on.any() and not on.all()
    assert np.array_equal(bits(got[~on]), bits(rew[~on]))
    # the product of two float32 is exact in float64; its sum with a float32 rounds once more, to float32: fmaf
    want = (np.float64(gamma) * v.astype(np.float64) + rew.astype(np.float64)).astype(np.float32)
    assert np.array_equal(bits(got[on]), bits(want[on]))
    masked = emu_ppo.values(dc, pc, term, mask=trunc, out=np.full(n, 7.0, np.float32))
    assert np.array_equal(bits(masked[on]), bits(v[on])) and np.all(masked[~on] == 7.0)
    assert np.array_equal(emu_ppo.bootstrap(dc, pc, term, np.zeros(n, np.uint8), gamma, rew), rew)


# ---- 5. DeviceActorCritic's parameter views (torch on the host: no GPU is needed to build the torch side)
def test_parameter_views_round_trip_and_follow_an_optimiser_step():
    import torch
    from qs_amd import DeviceActorCritic
    torch.manual_seed(0)
    ac = DeviceActorCritic(28, 6, num_envs=32, device="cpu")
    assert ac.h is None
    vec = torch.nn.utils.parameters_to_vector
    assert torch.equal(vec(ac.actor.parameters()), ac.actor_params) and torch.equal(vec(ac.critic.parameters()), ac.critic_params)
    assert ac.actor_params.numel() == 28 * 64 + 64 + 64 * 64 + 64 + 64 * 6 + 6 and ac.critic_params.numel() == 28 * 64 + 64 + 64 * 64 + 64 + 64 + 1
    for p in list(ac.actor.parameters()) + list(ac.critic.parameters()):
        assert p.untyped_storage().data_ptr() in (ac.actor_params.untyped_storage().data_ptr(), ac.critic_params.untyped_storage().data_ptr())
    # SB3's initialisation: orthogonal trunks with gain sqrt(2), a small action head, zero biases
    w0 = ac.actor[0].weight.detach()
    assert torch.allclose(w0.T @ w0, 2.0 * torch.eye(28), atol=1e-4) and float(ac.actor[-1].weight.detach().abs().max()) < 0.05 and float(ac.actor[0].bias.detach().abs().max()) == 0.0
    # state dict <-> flat tensors, under SB3's names
    sd = ppo_state_dict(np.random.default_rng(1))
    ac.load_state_dict(sd)
    spec_pi, spec_vf = (__import__("qs_amd.policy", fromlist=["x"]).spec_from_state_dict(sd, "ppo", "tanh", head) for head in ("policy", "value"))
    assert np.array_equal(ac.actor_params.numpy(), spec_pi["params"]) and np.array_equal(ac.critic_params.numpy(), spec_vf["params"])
    assert torch.equal(ac.log_std.detach(), sd["log_std"])
    out = ac.state_dict()
    assert sorted(out) == sorted(sd)
    for k in sd:
        assert torch.equal(out[k], torch.as_tensor(sd[k])), k
    again = DeviceActorCritic.from_state_dict(out, num_envs=8, device="cpu")
    assert torch.equal(again.actor_params, ac.actor_params) and torch.equal(again.critic_params, ac.critic_params)
    # an in-place optimiser step is a change of the flat tensors
    before_a, before_c = ac.actor_params.clone(), ac.critic_params.clone()
    opt = torch.optim.Adam(ac.parameters(), lr=1e-2, eps=1e-5)
    obs, actions = torch.randn(16, 28), torch.randn(16, 6)
    values, log_prob, entropy = ac.evaluate_actions(obs, actions)
    (values.sum() + log_prob.sum()).backward()
    opt.step()
    assert not torch.equal(ac.actor_params, before_a) and not torch.equal(ac.critic_params, before_c)
    assert torch.equal(vec(ac.actor.parameters()), ac.actor_params) and torch.equal(vec(ac.critic.parameters()), ac.critic_params)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ac.predict(np.zeros((32, 28), np.float32))


def test_evaluate_actions_is_the_host_build_of_the_kernel():
    """values and log-prob of the torch side against csrc/qs_ppo.h for the same parameters (float32 against float32: a loose bound)"""
    import torch
    from qs_amd import DeviceActorCritic
    rng = np.random.default_rng(8)
    n = 24
    ac = DeviceActorCritic(28, 6, num_envs=n, device="cpu")
    ac.load_state_dict(ppo_state_dict(rng))
    _, _, da, dc = pair(n=n)
    obs, eps = R.make_obs(rng, n, 28), rng.standard_normal((n, 6)).astype(np.float32)
    log_std = ac.log_std.detach().numpy()
    _, act, val, lp = emu_ppo.collect(da, dc, ac.actor_params.numpy(), ac.critic_params.numpy(), obs, eps, log_std)
    values, log_prob, entropy = ac.evaluate_actions(torch.as_tensor(obs), torch.as_tensor(act))
    assert np.allclose(values.detach().numpy(), val, atol=1e-4) and np.allclose(log_prob.detach().numpy(), lp, atol=1e-3)
    assert np.allclose(entropy.detach().numpy(), (0.5 + 0.5 * np.log(2 * np.pi) + log_std).sum(), atol=1e-5)


# ---- 6. ppo_loss against SB3's formulas in numpy
@pytest.mark.parametrize("clip_range_vf", [None, 0.3])
@pytest.mark.parametrize("with_entropy", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
def test_ppo_loss_against_numpy(clip_range_vf, with_entropy, normalize):
    import torch
    from qs_amd import ppo_loss
    rng = np.random.default_rng(9)
    B = 64
    old_lp = rng.normal(-5.0, 1.0, B)
    lp = old_lp + rng.normal(0.0, 0.25, B)                      # ratios on both sides of [0.8, 1.2]
    adv, old_v = rng.standard_normal(B), rng.standard_normal(B)
    v, ret, ent = old_v + rng.normal(0.0, 0.5, B), rng.standard_normal(B), rng.uniform(1.0, 3.0, B)
    ratio = np.exp(lp - old_lp)
    clipped = (np.abs(ratio - 1.0) > 0.2)
    assert clipped.any() and not clipped.all()                                  # both branches of the policy loss ...
    assert (np.abs(v - old_v) > 0.3).any() and (np.abs(v - old_v) < 0.3).any()  # ... and of the value clip
    tt = lambda x: torch.as_tensor(x, dtype=torch.float64)  # noqa: E731
    loss, info = ppo_loss(tt(v), tt(lp), tt(ent) if with_entropy else None, tt(old_v), tt(old_lp), tt(adv), tt(ret), 0.2, clip_range_vf, 0.01, 0.5, normalize)
    want = ppo_ref.ppo_loss(v, lp, ent if with_entropy else None, old_v, old_lp, adv, ret, 0.2, clip_range_vf, 0.01, 0.5, normalize)
    got = (loss, info["policy_loss"], info["value_loss"], info["entropy_loss"], info["approx_kl"], info["clip_fraction"])
    for name, g, w in zip(("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction"), got, want):
        assert abs(float(g) - float(w)) <= 1e-12 * max(1.0, abs(float(w))), (name, float(g), float(w))
    assert float(info["clip_fraction"]) == clipped.mean()


# ---- 7. train() on a fabricated buffer
def fabricated(n_epochs, target_kl=None, seed=0):
    import torch
    from qs_amd import DeviceActorCritic, DevicePPO
    torch.manual_seed(seed)
    T, N = 8, 32
    ac = DeviceActorCritic(28, 6, num_envs=N, device="cpu")
    algo = DevicePPO(None, ac, n_steps=T, batch_size=64, n_epochs=n_epochs, learning_rate=3e-3, target_kl=target_kl, normalize_advantage=False, seed=seed)
    buf = algo.buffer
    buf.observations.copy_(torch.randn(T, N, 28))
    with torch.no_grad():
        mean = ac.actor(buf.observations)
        buf.actions.copy_(mean + torch.randn(T, N, 6))
        values, log_prob, _ = ac.evaluate_actions(buf.observations, buf.actions)
    buf.values.copy_(values.view(T, N))
    buf.log_probs.copy_(log_prob)
    buf.advantages.copy_(torch.where(buf.actions[..., 0] > 0, 1.0, -1.0))
    buf.returns.copy_(buf.values)
    return ac, algo


def test_train_moves_the_mean_towards_the_rewarded_actions():
    import torch
    ac, algo = fabricated(n_epochs=1)
    first = []
    for _ in range(6):
        with torch.no_grad():
            first.append(float(ac.actor(algo.buffer.observations)[..., 0].mean()))
        info = algo.train()
        assert np.isfinite(info["approx_kl"]) and info["n_epochs_run"] == 1
    print("mean first action component per epoch:", first)
    assert all(b > a for a, b in zip(first, first[1:])), first


def test_a_tiny_target_kl_stops_the_epoch_loop_early():
    _, algo = fabricated(n_epochs=10, target_kl=1e-9)
    info = algo.train()
    assert info["n_epochs_run"] < 10 and np.isfinite(info["approx_kl"]) and info["approx_kl"] > 1.5e-9


def test_minibatches_cover_the_buffer_once():
    import torch
    _, algo = fabricated(n_epochs=1)
    buf = algo.buffer
    buf.returns.copy_(torch.arange(8 * 32, dtype=torch.float32).view(8, 32))
    seen = torch.cat([mb["returns"] for mb in buf.get(100, generator=algo.generator)])
    assert seen.numel() == 256 and torch.equal(seen.sort().values, torch.arange(256, dtype=torch.float32)) and not torch.equal(seen, seen.sort().values)
    with pytest.raises(RuntimeError, match="no CPU path"):
        buf.compute_returns_and_advantage(torch.zeros(32), torch.zeros(32, dtype=torch.uint8))
