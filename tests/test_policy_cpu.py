"""Policy inference without a GPU: the host build of csrc/qs_policy.h (tests/emu/qs_emu_policy.cpp) against the float64
reference and its derived error bound (tests/policy_ref.py), per-policy blocks, the Gaussian path, reading torch / SB3 objects, ARS plumbing."""
import ctypes as C
import os
import sys
import zipfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import policy_ref as R  # noqa: E402
from emu import emu_policy  # noqa: E402
from qs_amd import policy as P  # noqa: E402
from qs_amd.lib import QsPolicyDesc  # noqa: E402


def desc_of(kw, n_envs, clip=(-1.0, 1.0)):
    arch = tuple(kw["net_arch"])
    return QsPolicyDesc(n_envs, kw["n_policies"], kw["obs_dim"], kw["action_dim"], len(arch), (C.c_int32 * 4)(*arch), P.ACTIVATIONS[kw["activation"]],
                        int(kw["squash_output"]), int(kw["bias"]), clip[0], clip[1])


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ---- 1. descriptors the host build refuses
@pytest.mark.parametrize("change, word", [(dict(net_arch=(257,)), "hidden[0]"), (dict(n_policies=3), "n_policies"), (dict(obs_dim=65), "obs_dim"),
                                          (dict(action_dim=0), "action_dim"), (dict(activation_code=7), "activation")])
def test_bad_descriptors_are_refused_with_their_reason(change, word):
    kw = dict(obs_dim=28, action_dim=6, net_arch=(64, 64), activation="tanh", squash_output=False, bias=True, n_policies=1)
    code = change.pop("activation_code", None)
    kw.update(change)
    d = desc_of(kw, 64)
    if code is not None:
        d.activation = code
    with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
        emu_policy.param_count(d)


def test_five_hidden_layers_are_refused():
    d5 = desc_of(dict(obs_dim=28, action_dim=6, net_arch=(8,), activation="tanh", squash_output=False, bias=True, n_policies=1), 64)
    d5.n_hidden = 5
    with pytest.raises(ValueError, match="n_hidden"):
        emu_policy.param_count(d5)


# The LDS layout of a launch of k_policy / k_actor_critic as csrc/qs_policy.h sizes it: (obs_dim, net_arch, action_dim, critic's net_arch or None
# for k_policy, N, policies) -> act_stride, w_floats, wide, waves, LDS bytes, LDS bytes of a one-wave launch (None: not stated).
# 48-256-4 is the smallest net with a k-chunked layer (272 x 48 = 13 056 floats, above 12 288).
LAYOUTS = [
    ((28, (64, 64), 6, None, 8192, 1), (68, 5120, 0, 2, 29184, None)),
    ((28, (64, 64), 6, None, 16400, 1), (68, 5120, 0, 4, 37888, None)),
    ((28, (64, 64), 6, None, 8192, 128), (68, 5120, 0, 2, 29184, None)),
    ((28, (64, 64), 6, None, 40, 2), (68, 5120, 0, 1, 24832, None)),
    ((28, (), 6, None, 64, 1), (68, 448, 0, None, None, None)),
    ((30, (33, 7), 5, None, 64, 1), (68, 1536, 0, None, None, None)),
    ((64, (256, 200, 256), 12, None, 64, 1), (260, 12288, 1, None, None, None)),
    ((48, (256,), 4, None, 16400, 1), (260, 12288, 1, 4, 115712, None)),
    ((48, (256,), 4, None, 100, 1), (260, 12288, 1, 1, 65792, None)),
    ((28, (64, 64), 6, (64, 64), 8192, 1), (68, 5120, 0, 2, 37888, 29184)),
    ((28, (64, 64), 6, (64, 64), 16400, 1), (68, 5120, 0, 4, 55296, 29184)),
    ((48, (256,), 4, (64,), 16400, 1), (260, 12288, 1, 2, 115712, 82432)),     # (4 waves would need 182 272 B, above the 160 KB of a compute unit)
]


def test_param_count_is_parameters_to_vector():
    import torch
    net = torch.nn.Sequential(torch.nn.Linear(28, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 6))
    kw = dict(obs_dim=28, action_dim=6, net_arch=(64, 64), activation="tanh", squash_output=False, bias=True, n_policies=1)
    n = torch.nn.utils.parameters_to_vector(net.parameters()).numel()
    assert emu_policy.param_count(desc_of(kw, 16)) == n == P.param_count(28, 6, (64, 64)) == 28 * 64 + 64 + 64 * 64 + 64 + 64 * 6 + 6
    assert emu_policy.param_count(desc_of(dict(kw, net_arch=(), bias=False), 16)) == 28 * 6
    # ... and the LDS image the same descriptors are given
    for (obs_dim, arch, action_dim, vf_arch, n, n_pol), want in LAYOUTS:
        ka = dict(kw, obs_dim=obs_dim, action_dim=action_dim, net_arch=arch, n_policies=n_pol)
        critic = None if vf_arch is None else desc_of(dict(ka, action_dim=1, net_arch=vf_arch), n)
        got = emu_policy.layout(desc_of(ka, n), critic)
        assert all(w is None or g == w for g, w in zip(got, want)), (obs_dim, arch, action_dim, vf_arch, n, n_pol, got, want)


# ---- 2. the host emulation against float64, under the derived bound
def worst_ratio(net_name, scale, run):
    """max over the cases of max |run(...) - float64| / bound (the clamp is 1-Lipschitz: the mean's bound holds for the action)"""
    c = R.tanh_c()
    worst, worst_tag = 0.0, None
    for tag, kw, params, obs in R.cases(net_name, scale):
        mean64, bound = R.forward(params, obs, kw["obs_dim"], kw["action_dim"], kw["net_arch"], kw["activation"], kw["squash_output"], kw["bias"], kw["n_policies"], c)
        act = run(kw, params, obs)
        ratio = float(np.max(np.abs(act.astype(np.float64) - np.clip(mean64, -1.0, 1.0)) / bound))
        if ratio > worst:
            worst, worst_tag = ratio, tag
    return worst, worst_tag


def test_host_tanhf_error_is_what_the_record_says():
    """the bound's c rests on this measurement: a libm whose tanhf is worse than the record knows must not pass silently"""
    x = R.tanh_points()
    m = R.max_ulp_error(x, emu_policy.tanh(x))
    print("host tanhf max error: %.3f ulp" % m)
    R.record("tanhf_max_ulp_error_seen", "host_emulation", m)
    assert 2.0 * m <= R.tanh_c(), (m, R.tanh_c())


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("net_name", sorted(R.NETS))
def test_emulation_against_float64_under_the_bound(net_name, scale):
    ratio, tag = worst_ratio(net_name, scale, lambda kw, params, obs: emu_policy.act(desc_of(kw, obs.shape[0]), params, obs)[0])
    print(f"{net_name} x{scale:g}: max err / bound = {ratio:.3g} at {tag}")
    R.record("emulation_max_err_over_bound", f"{net_name}-x{scale:g}", ratio)
    assert ratio <= 1.0, (ratio, tag)


def test_the_bound_is_not_vacuous():
    """some case must come within three orders of magnitude of its bound"""
    best = max(worst_ratio(n, 1.0, lambda kw, params, obs: emu_policy.act(desc_of(kw, obs.shape[0]), params, obs)[0])[0] for n in ("ars_linear", "tanh64x64"))
    assert best >= 1e-3, best


# ---- 3. the bound has teeth
@pytest.mark.parametrize("net_name", ["ars_linear", "relu16"])
def test_one_weight_off_by_1e_4_breaks_the_bound(net_name):
    """The same comparison with one weight of the last layer moved by 1e-4 must fail.  It does where the bound is sharp (5e-6 for the
    linear policy, 2e-5 behind 16 relu units).  Behind two tanh layers of 64 the worst-case propagation |W| e has grown the bound to about
    1e-4 itself (the same change reaches 0.88 of it), behind four layers of 256 far beyond: there the bound holds, and says little."""
    def run(kw, params, obs):
        off = params.copy()
        off[:, P.param_count(kw["obs_dim"], kw["action_dim"], kw["net_arch"], kw["bias"]) - 2 * kw["action_dim"]] += 1e-4   # a weight of the last layer
        return emu_policy.act(desc_of(kw, obs.shape[0]), off, obs)[0]
    ratio, _ = worst_ratio(net_name, 1.0, run)
    assert ratio > 1.0, ratio


# ---- 4. per-policy blocks, independence of the other environments
def test_each_block_runs_its_own_policy_and_no_environment_sees_another():
    rng = np.random.default_rng(4)
    kw = dict(obs_dim=28, action_dim=6, net_arch=(64, 64), activation="tanh", squash_output=False, bias=True, n_policies=4)
    n = 4 * 24
    params, obs = R.make_params(rng, 28, 6, (64, 64), True, 4), R.make_obs(rng, n, 28)
    act4 = emu_policy.act(desc_of(kw, n), params, obs)[0]
    for p in range(4):
        one = emu_policy.act(desc_of(dict(kw, n_policies=1), n), params[p:p + 1], obs)[0]
        assert np.array_equal(bits(one[p * 24:(p + 1) * 24]), bits(act4[p * 24:(p + 1) * 24]))
    i = 37
    perm = rng.permutation(n)
    perm = np.concatenate([perm[perm != i][:i], [i], perm[perm != i][i:]])      # everyone else moves, i stays
    assert perm[i] == i and not np.array_equal(perm, np.arange(n))
    same_policy = emu_policy.act(desc_of(dict(kw, n_policies=1), n), params[1:2], obs[perm])[0]
    assert np.array_equal(bits(same_policy[i]), bits(act4[i]))                  # (environment 37 is in block 1)


# ---- 5. the Gaussian path
def test_sample_and_log_prob_against_torch_distributions():
    """Tolerances (reasoned, u = 2^-24): the action is mean + exp(log_std) * eps with expf good to 3 ulp (6 u relative; OpenCL's bound for
    exp, glibc's is under 1) and one rounding of the fmaf: bound(mean) + 6 u std |eps| + u |a|.  log_prob is a sum of A terms
    -eps^2 / 2 - log_std - log(2 pi) / 2, each two roundings: gamma_(A + 2) sum |term| with the three parts' magnitudes added."""
    import torch
    rng = np.random.default_rng(5)
    kw = dict(obs_dim=28, action_dim=6, net_arch=(64, 64), activation="tanh", squash_output=False, bias=True, n_policies=2)
    n = 64
    params, obs = R.make_params(rng, 28, 6, (64, 64), True, 2, 3.0), R.make_obs(rng, n, 28)
    eps = rng.standard_normal((n, 6)).astype(np.float32)
    log_std = rng.uniform(-1.5, 0.3, 6).astype(np.float32)
    act, mean, lp = emu_policy.act(desc_of(kw, n), params, obs, eps, log_std)
    mean64, bound = R.forward(params, obs, 28, 6, (64, 64), "tanh", False, True, 2, R.tanh_c())
    assert np.all(np.abs(mean - mean64) <= bound)
    std = np.exp(log_std.astype(np.float64))
    a64 = mean64 + std * eps.astype(np.float64)
    dist = torch.distributions.Normal(torch.as_tensor(mean64), torch.as_tensor(std))
    lp64 = dist.log_prob(torch.as_tensor(a64)).sum(-1).numpy()
    tol_a = bound + 6 * R.U * std * np.abs(eps) + R.U * np.abs(a64)
    assert np.all(np.abs(act - np.clip(a64, -1.0, 1.0)) <= tol_a)
    assert np.any(np.abs(a64) > 1.0) and np.all(np.abs(act) <= 1.0)              # the clamp bites, on the actions ...
    assert np.array_equal(mean, emu_policy.act(desc_of(kw, n), params, obs)[1])  # ... only: the mean is the deterministic one, unclipped
    tol_lp = R.gamma(6 + 2) * (0.5 * eps.astype(np.float64) ** 2 + np.abs(log_std) + 0.9189385).sum(-1)
    assert np.all(np.abs(lp - lp64) <= tol_lp), np.max(np.abs(lp - lp64) / tol_lp)


# ---- 6. reading torch and SB3 objects
def ppo_state_dict(rng, obs_dim=28, action_dim=6, width=64):
    import torch
    t = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    sd = {"log_std": t(action_dim)}
    for trunk in ("policy_net", "value_net"):
        sd.update({f"mlp_extractor.{trunk}.0.weight": t(width, obs_dim), f"mlp_extractor.{trunk}.0.bias": t(width),
                   f"mlp_extractor.{trunk}.2.weight": t(width, width), f"mlp_extractor.{trunk}.2.bias": t(width)})
    sd.update({"action_net.weight": t(action_dim, width), "action_net.bias": t(action_dim), "value_net.weight": t(1, width), "value_net.bias": t(1)})
    return sd


def test_spec_from_module_keeps_parameters_to_vector_order():
    import torch
    nn = torch.nn
    net = nn.Sequential(nn.Linear(28, 64), nn.Tanh(), nn.Linear(64, 32), nn.Tanh(), nn.Linear(32, 6))
    s = P.spec_from_module(net)
    assert (s["obs_dim"], s["action_dim"], s["net_arch"], s["activation"], s["squash_output"], s["bias"]) == (28, 6, (64, 32), "tanh", False, True)
    assert np.array_equal(s["params"], torch.nn.utils.parameters_to_vector(net.parameters()).detach().numpy())
    obs = R.make_obs(np.random.default_rng(6), 16, 28)
    kw = dict(s, n_policies=1)
    act = emu_policy.act(desc_of(kw, 16, clip=(-3e38, 3e38)), s["params"][None], obs)[0]
    assert np.allclose(act, net(torch.as_tensor(obs)).detach().numpy(), atol=1e-5)
    lin = P.spec_from_module(nn.Sequential(nn.Linear(28, 6, bias=False)))
    assert (lin["net_arch"], lin["activation"], lin["bias"], lin["params"].size) == ((), "none", False, 168)
    sq = P.spec_from_module(nn.Sequential(nn.Linear(28, 16), nn.ReLU(), nn.Linear(16, 6), nn.Tanh()))
    assert (sq["activation"], sq["squash_output"]) == ("relu", True)
    with pytest.raises(ValueError, match="Sigmoid"):
        P.spec_from_module(nn.Sequential(nn.Linear(28, 6), nn.Sigmoid()))
    with pytest.raises(ValueError, match="one activation"):
        P.spec_from_module(nn.Sequential(nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 2)))


def test_spec_from_state_dict_ppo_ars_and_their_errors():
    rng = np.random.default_rng(7)
    sd = ppo_state_dict(rng)
    s = P.spec_from_state_dict(sd, "ppo")
    want = np.concatenate([sd[k].numpy().ravel() for k in ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
                                                            "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias")])
    assert np.array_equal(s["params"], want) and s["net_arch"] == (64, 64) and np.array_equal(s["log_std"], sd["log_std"].numpy())
    v = P.spec_from_state_dict(sd, "ppo", head="value")
    assert v["action_dim"] == 1 and v["log_std"] is None and np.array_equal(v["params"][-65:-1], sd["value_net.weight"].numpy().ravel())
    broken = dict(sd); del broken["action_net.bias"]
    with pytest.raises(KeyError) as ei:
        P.spec_from_state_dict(broken, "ppo")
    assert "action_net.bias" in str(ei.value) and "mlp_extractor.policy_net.0.weight" in str(ei.value)      # the missing key, and the ones found
    wrong = dict(sd, **{"mlp_extractor.policy_net.2.weight": sd["mlp_extractor.policy_net.2.weight"][:, :32]})
    with pytest.raises(ValueError, match="layer 1"):
        P.spec_from_state_dict(wrong, "ppo")
    with pytest.raises(ValueError, match="log_std"):
        P.spec_from_state_dict(dict(sd, log_std=sd["log_std"][:3]), "ppo")
    import torch
    lin = {"action_net.weight": torch.as_tensor(rng.standard_normal((6, 28)).astype(np.float32))}
    a = P.spec_from_state_dict(lin, "ars", activation="none")
    assert a["bias"] is False and a["net_arch"] == () and np.array_equal(a["params"], lin["action_net.weight"].numpy().ravel())
    mlp = {"action_net.0.weight": torch.zeros(16, 28), "action_net.0.bias": torch.ones(16), "action_net.2.weight": torch.zeros(6, 16), "action_net.2.bias": torch.ones(6)}
    m = P.spec_from_state_dict(mlp, "ars", activation="relu")
    assert m["net_arch"] == (16,) and m["bias"] and m["params"].size == 28 * 16 + 16 + 16 * 6 + 6
    with pytest.raises(KeyError, match="action_net.0.weight"):
        P.spec_from_state_dict({"something.weight": torch.zeros(2, 2)}, "ars")
    with pytest.raises(ValueError, match="algo"):
        P.spec_from_state_dict(sd, "sac")


def test_state_dict_from_an_sb3_style_zip(tmp_path):
    import io
    import torch
    sd = ppo_state_dict(np.random.default_rng(8))
    buf = io.BytesIO()
    torch.save(sd, buf)
    path = tmp_path / "model.zip"
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", "{}")
        z.writestr("policy.pth", buf.getvalue())
    back = P.state_dict_from_zip(path)
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert np.array_equal(P.spec_from_state_dict(back)["params"], P.spec_from_state_dict(sd)["params"])
    with zipfile.ZipFile(tmp_path / "empty.zip", "w") as z:
        z.writestr("data", "{}")
    with pytest.raises(KeyError, match="policy.pth"):
        P.state_dict_from_zip(tmp_path / "empty.zip")


# ---- 7. ARS plumbing
def test_ars_population_and_update_against_numpy():
    import torch
    rng = np.random.default_rng(9)
    n_delta, n_params, n_top, sigma, lr = 8, 30, 3, 0.05, 0.02
    theta, deltas = rng.standard_normal(n_params), rng.standard_normal((n_delta, n_params))
    rp, rm = rng.standard_normal(n_delta), rng.standard_normal(n_delta)
    pop = P.ars_population(torch.as_tensor(theta), torch.as_tensor(deltas), sigma).numpy()
    assert pop.shape == (2 * n_delta, n_params)
    assert np.allclose(pop[:n_delta], theta + sigma * deltas) and np.allclose(pop[n_delta:], theta - sigma * deltas)
    # sb3_contrib ARS._do_one_update, restated
    top = np.argsort(-np.maximum(rp, rm))[:n_top]
    std = np.concatenate([rp[top], rm[top]]).std(ddof=1)
    want = theta + lr / (n_top * std + 1e-6) * ((rp[top] - rm[top]) @ deltas[top])
    got = P.ars_update(torch.as_tensor(theta), torch.as_tensor(deltas), torch.as_tensor(rp), torch.as_tensor(rm), lr, n_top).numpy()
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
