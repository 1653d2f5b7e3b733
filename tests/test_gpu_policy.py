"""Policy inference on the device (k_policy through qs_policy_act / DevicePolicy): bitwise against the host build of csrc/qs_policy.h where no
tanh is involved, under the derived bound of tests/policy_ref.py where one is, per-policy blocks at N = 8192, a closed loop with the
environment, stream order, the SB3-style surface.  (The kernel has no tap for pre-activations, so the tanh networks are not compared
bitwise layer by layer; their linear parts are the same code as the bitwise cases'.)"""
import ctypes as C
import os
import sys
import zipfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402
from emu import emu_policy  # noqa: E402
from test_gpu_round2 import vec_env  # noqa: E402
from test_policy_cpu import desc_of, ppo_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def bits(x):
    x = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def device_policy(kw, n, params, **more):
    from qs_amd import DevicePolicy
    pol = DevicePolicy(kw["obs_dim"], kw["action_dim"], net_arch=kw["net_arch"], activation=kw["activation"], squash_output=kw["squash_output"],
                       bias=kw["bias"], num_envs=n, n_policies=kw["n_policies"], **more)
    pol.set_params(params)
    return pol


def device_act(torch, kw, params, obs):
    pol = device_policy(kw, obs.shape[0], params)
    out = pol.act(torch.as_tensor(obs, device="cuda")).cpu().numpy()
    pol.close()
    return out


# ---- 8. against the host emulation (bitwise) and against float64 (bound)
def test_device_tanhf_error_is_what_the_record_says(torch_cuda):
    """tanhf of the device over the 10^6 points, through the public interface: a 1 -> 1 linear policy with weight 1 and squash_output"""
    torch = torch_cuda
    x = R.tanh_points()
    kw = dict(obs_dim=1, action_dim=1, net_arch=(), activation="none", squash_output=True, bias=False, n_policies=1)
    pol = device_policy(kw, x.size, np.ones((1, 1), np.float32), clip=None)
    y = pol.act(torch.as_tensor(x.reshape(-1, 1), device="cuda")).cpu().numpy().reshape(-1)
    pol.close()
    m = R.max_ulp_error(x, y)
    print("device tanhf max error: %.3f ulp" % m)
    R.record("tanhf_max_ulp_error_seen", "device", m)
    assert 2.0 * m <= R.tanh_c(), (m, R.tanh_c())


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("net_name", ["ars_linear", "relu16"])
def test_device_equals_the_emulation_bit_for_bit(torch_cuda, net_name, scale):
    for tag, kw, params, obs in R.cases(net_name, scale):
        want = emu_policy.act(desc_of(kw, obs.shape[0]), params, obs)[0]
        got = device_act(torch_cuda, kw, params, obs)
        assert np.array_equal(bits(got), bits(want)), (tag, np.argwhere(bits(got) != bits(want))[:8].tolist(), float(np.abs(got - want).max()))


def test_widths_and_observations_that_are_no_multiple_of_four_bit_for_bit(torch_cuda):
    """obs_dim 30, widths 33 and 7 (relu), action_dim 5: the zero products that fill an MFMA step's four k are the emulation's too"""
    rng = np.random.default_rng(80)
    kw = dict(obs_dim=30, action_dim=5, net_arch=(33, 7), activation="relu", squash_output=False, bias=True, n_policies=2)
    params, obs = R.make_params(rng, 30, 5, (33, 7), True, 2, 3.0), R.make_obs(rng, 2 * 21, 30)
    want = emu_policy.act(desc_of(kw, 42), params, obs)[0]
    got = device_act(torch_cuda, kw, params, obs)
    assert np.array_equal(bits(got), bits(want))
    wide = dict(obs_dim=64, action_dim=12, net_arch=(256, 200, 256), activation="relu", squash_output=False, bias=True, n_policies=1)   # layers in k-chunks
    params, obs = R.make_params(rng, 64, 12, (256, 200, 256), True, 1), R.make_obs(rng, 100, 64)
    assert np.array_equal(bits(device_act(torch_cuda, wide, params, obs)), bits(emu_policy.act(desc_of(wide, 100), params, obs)[0]))


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("net_name", ["tanh64x64", "tanh256x4"])
def test_device_tanh_networks_against_float64_under_the_bound(torch_cuda, net_name, scale):
    from test_policy_cpu import worst_ratio
    ratio, tag = worst_ratio(net_name, scale, lambda kw, params, obs: device_act(torch_cuda, kw, params, obs))
    print(f"{net_name} x{scale:g}: device max err / bound = {ratio:.3g} at {tag}")
    R.record("device_max_err_over_bound", f"{net_name}-x{scale:g}", ratio)
    assert ratio <= 1.0, (ratio, tag)


def test_gaussian_path_on_the_device(torch_cuda):
    """test_policy_cpu.test_sample_and_log_prob_against_torch_distributions on the device, with its tolerances; log_prob has no
    transcendental in it and equals the emulation's bit for bit"""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    kw = dict(obs_dim=28, action_dim=6, net_arch=(64, 64), activation="tanh", squash_output=False, bias=True, n_policies=2)
    n = 64
    params, obs = R.make_params(rng, 28, 6, (64, 64), True, 2, 3.0), R.make_obs(rng, n, 28)
    eps = rng.standard_normal((n, 6)).astype(np.float32)
    log_std = rng.uniform(-1.5, 0.3, 6).astype(np.float32)
    pol = device_policy(kw, n, params)
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    act, mean, lp = [x.cpu().numpy() for x in pol.act(dev(obs), eps=dev(eps), log_std=dev(log_std), want_mean=True, want_log_prob=True)]
    pol.close()
    mean64, bound = R.forward(params, obs, 28, 6, (64, 64), "tanh", False, True, 2, R.tanh_c())
    std = np.exp(log_std.astype(np.float64))
    a64 = mean64 + std * eps.astype(np.float64)
    assert np.all(np.abs(mean - mean64) <= bound)
    assert np.all(np.abs(act - np.clip(a64, -1.0, 1.0)) <= bound + 6 * R.U * std * np.abs(eps) + R.U * np.abs(a64))
    assert np.array_equal(bits(lp), bits(emu_policy.act(desc_of(kw, n), params, obs, eps, log_std)[2]))
    lp64 = torch.distributions.Normal(torch.as_tensor(mean64), torch.as_tensor(std)).log_prob(torch.as_tensor(a64)).sum(-1).numpy()
    assert np.all(np.abs(lp - lp64) <= R.gamma(8) * (0.5 * eps.astype(np.float64) ** 2 + np.abs(log_std) + 0.9189385).sum(-1))


# ---- 9. per-policy blocks on the device
@pytest.mark.parametrize("n, n_pol", [(8192, 128), (8200, 1), (8200, 8), (40, 2)])
def test_blocks_and_independence_on_the_device(torch_cuda, n, n_pol):
    torch = torch_cuda
    rng = np.random.default_rng(n + n_pol)
    kw = dict(obs_dim=28, action_dim=6, net_arch=(64, 64), activation="relu", squash_output=False, bias=True, n_policies=n_pol)
    n_per = n // n_pol
    params, obs = R.make_params(rng, 28, 6, (64, 64), True, n_pol, 2.0), R.make_obs(rng, n, 28)
    got = device_act(torch, kw, params, obs)
    assert np.array_equal(bits(got), bits(emu_policy.act(desc_of(kw, n), params, obs)[0]))
    for p in sorted({0, n_pol // 2, n_pol - 1}):        # block p alone, as a shared policy over all environments
        one = device_act(torch, dict(kw, n_policies=1), params[p:p + 1], obs)
        assert np.array_equal(bits(one[p * n_per:(p + 1) * n_per]), bits(got[p * n_per:(p + 1) * n_per])), p
    i = n_per * (n_pol - 1) + n_per // 2                  # an environment of the last block: everyone else's observation moves
    perm = rng.permutation(n)
    perm = np.concatenate([perm[perm != i][:i], [i], perm[perm != i][i:]])
    moved = device_act(torch, dict(kw, n_policies=1), params[n_pol - 1:], obs[perm])
    assert np.array_equal(bits(moved[i]), bits(got[i]))


# ---- 10. a closed loop with the environment
def test_closed_loop_with_the_environment(torch_cuda):
    """50 steps of 256 environments under DeviceVecNormalize driven by DevicePolicy.act.  At every step the torch Sequential the policy was
    made from sees the SAME observation tensor; both are held against float64 (DevicePolicy under the bound; torch's distance is recorded)."""
    torch = torch_cuda
    from qs_amd import DevicePolicy, DeviceVecNormalize
    nn = torch.nn
    torch.manual_seed(10)
    env = DeviceVecNormalize(vec_env(256, auto_reset=True), training=True)
    net = nn.Sequential(nn.Linear(env.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, env.action_dim)).cuda()
    pol = DevicePolicy.from_module(net, num_envs=256)
    theta = torch.nn.utils.parameters_to_vector(net.parameters()).detach()
    assert torch.equal(pol.get_params()[0], theta)
    obs = env.reset_tensor()
    worst, worst_torch = 0.0, 0.0
    for _ in range(50):
        act = pol.act(obs)
        with torch.no_grad():
            ref32 = net(obs).clamp(-1.0, 1.0)
        mean64, bound = R.forward(theta.cpu().numpy()[None], obs.cpu().numpy(), env.obs_dim, env.action_dim, (64, 64), "tanh", False, True, 1, R.tanh_c())
        a64 = np.clip(mean64, -1.0, 1.0)
        worst = max(worst, float(np.max(np.abs(act.cpu().numpy() - a64) / bound)))
        worst_torch = max(worst_torch, float(np.max(np.abs(ref32.cpu().numpy() - a64) / bound)))
        obs, rew, done, trunc = env.step_tensor(act)
    print(f"closed loop: DevicePolicy max err / bound = {worst:.3g}, torch fp32 forward = {worst_torch:.3g}")
    R.record("closed_loop_max_err_over_bound", "device_policy", worst)
    R.record("closed_loop_max_err_over_bound", "torch_fp32", worst_torch)
    pol.close(); env.close()
    assert worst <= 1.0, worst


# ---- 11. stream order
def test_act_behind_the_step_on_a_side_stream_needs_no_synchronisation(torch_cuda):
    """act, and a second DevicePolicy (the value head) on the same observations, enqueued right behind step_tensor on a side stream give
    the bits of the same calls made after a full synchronisation"""
    torch = torch_cuda
    from qs_amd import DevicePolicy
    rng = np.random.default_rng(12)
    env = vec_env(512)
    sd = ppo_state_dict(rng, env.obs_dim, env.action_dim)
    sd["value_net.bias"] = sd["value_net.bias"] + 20.0      # (values well outside the action Box)
    pol = DevicePolicy.from_state_dict(sd, "ppo", num_envs=512)
    val = DevicePolicy.from_state_dict(sd, "ppo", num_envs=512, head="value")
    assert val.action_dim == 1 and val.clip[1] > 1e30
    env.reset_tensor()
    a0 = torch.as_tensor(rng.uniform(-1, 1, (512, env.action_dim)).astype(np.float32), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        obs = env.step_tensor(a0)[0]
        act = pol.act(obs).clone()                           # enqueued behind the step, nothing waited for
        value = val.act(obs, want_mean=True)[1].clone()
        obs_h = obs.clone()
    torch.cuda.synchronize()
    assert np.array_equal(bits(pol.act(obs_h)), bits(act))
    assert np.array_equal(bits(val.act(obs_h, want_mean=True)[1]), bits(value))
    a, m, _ = val.act(obs_h, want_mean=True)                 # the value head is not clipped to the action Box
    assert torch.equal(a, m) and float(m.abs().min()) > 1.0
    pol.close(); val.close(); env.close()


# ---- 12. the SB3-style surface
def test_predict_load_and_argument_checks(torch_cuda, tmp_path):
    import io
    torch = torch_cuda
    from qs_amd import DevicePolicy
    rng = np.random.default_rng(13)
    sd = ppo_state_dict(rng)
    buf = io.BytesIO()
    torch.save(sd, buf)
    with zipfile.ZipFile(tmp_path / "model.zip", "w") as z:
        z.writestr("policy.pth", buf.getvalue())
    pol = DevicePolicy.load(tmp_path / "model.zip", num_envs=48)
    assert (pol.obs_dim, pol.action_dim, pol.net_arch, pol.n_params) == (28, 6, (64, 64), 28 * 64 + 64 + 64 * 64 + 64 + 64 * 6 + 6)
    assert torch.equal(pol.log_std.cpu(), sd["log_std"])
    obs = R.make_obs(rng, 48, 28)
    a_np, state = pol.predict(obs, deterministic=True)
    assert state is None and isinstance(a_np, np.ndarray) and a_np.dtype == np.float32
    assert np.array_equal(bits(a_np), bits(pol.act(torch.as_tensor(obs, device="cuda"))))
    a_t, _ = pol.predict(torch.as_tensor(obs, device="cuda"))
    assert torch.is_tensor(a_t) and np.array_equal(bits(a_t), bits(a_np))
    noisy, _ = pol.predict(obs, deterministic=False)
    assert not np.array_equal(noisy, a_np) and np.all(np.abs(noisy) <= 1.0)
    with pytest.raises(ValueError, match="obs has shape"):
        pol.act(torch.zeros((47, 28), device="cuda"))
    with pytest.raises(TypeError, match="obs must be float32"):
        pol.act(torch.zeros((48, 28), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="eps has shape"):
        pol.act(torch.zeros((48, 28), device="cuda"), eps=torch.zeros((48, 5), device="cuda"))
    with pytest.raises(ValueError, match="obs is on"):
        pol.act(torch.zeros((48, 28)))
    with pytest.raises(ValueError, match="params has shape"):
        pol.set_params(np.zeros(7, np.float32))
    pol.close()
    with pytest.raises(RuntimeError, match="hidden\\[0\\]"):
        DevicePolicy(28, 6, net_arch=(300,), num_envs=16)
    with pytest.raises(RuntimeError, match="n_policies"):
        DevicePolicy(28, 6, num_envs=16, n_policies=3)
    # an ARS population: [2 n_delta, n_params] built on the device and used in place
    from qs_amd.policy import ars_population
    lin = DevicePolicy(28, 6, net_arch=(), activation="none", bias=False, num_envs=64, n_policies=8)
    theta = torch.as_tensor(rng.standard_normal(lin.n_params).astype(np.float32), device="cuda")
    deltas = torch.as_tensor(rng.standard_normal((4, lin.n_params)).astype(np.float32), device="cuda")
    pop = ars_population(theta, deltas, 0.05)
    lin.set_params(pop)
    assert lin.get_params().data_ptr() == pop.data_ptr()
    obs64 = R.make_obs(rng, 64, 28)
    kw = dict(obs_dim=28, action_dim=6, net_arch=(), activation="none", squash_output=False, bias=False, n_policies=8)
    assert np.array_equal(bits(lin.act(torch.as_tensor(obs64, device="cuda"))), bits(emu_policy.act(desc_of(kw, 64), pop.cpu().numpy(), obs64)[0]))
    lin.close()
