"""DeviceARS on the GPU (csrc/qs_ars.hip): every kernel bit for bit against the host twin (tests/emu/qs_emu_ars.cpp) over the shapes of
tests/ars_ref.py -- m in {1, 3, 64, 65, 130}, n_delta in {1, 2, 5, 64, 65, 1024}, n_top in {1, middle, n_delta}, n_params in {1, 168, 255,
256, 257, 6406} -- on fabricated rewards and dones; std and step within the derived bounds of the float64 restatement (the measured ratios
are printed and, where QS_RECORD_DIR names a directory, appended to its ars_parity.jsonl); repeatability; independence of check_every; a
real rollout against today's torch accumulation; the refusals."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import ars_ref as A  # noqa: E402
from emu import emu_ars as E  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


class Params:
    """what DeviceARS uses of a policy, for the kernels' shapes alone (n_params = 1, 2048 candidates): no network behind it"""

    def __init__(self, torch, num_envs, n_policies, n_params):
        self.num_envs, self.n_policies, self.n_params, self.device = num_envs, n_policies, n_params, torch.device("cuda", 0)
        self._params = None

    def set_params(self, p):
        self._params = p

    def get_params(self):
        return self._params


def learner(torch, m, n_delta, n_top, n_params, **kw):
    from qs_amd import DeviceARS
    return DeviceARS(None, Params(torch, 2 * n_delta * m, 2 * n_delta, n_params), n_delta=n_delta, n_top=n_top, **kw)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def host(t):
    return t.cpu().numpy().copy()


def record(rec):
    """one line per case into $QS_RECORD_DIR/ars_parity.jsonl (what profiles/ars_parity.json is assembled from); nothing without the variable"""
    out = os.environ.get("QS_RECORD_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ars_parity.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def inputs(n_delta, n_params, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n_params) * 0.3).astype(np.float32), rng.standard_normal((n_delta, n_params)).astype(np.float32)


@pytest.mark.parametrize("m, n_delta, n_top, n_params", A.SHAPES)
def test_kernels_against_the_twin(torch_cuda, m, n_delta, n_top, n_params):
    t = torch_cuda
    N, epe = 2 * n_delta * m, 1 + (m % 2)
    theta, delta = inputs(n_delta, n_params, n_delta * 7 + m)
    ars = learner(t, m, n_delta, n_top, n_params, episodes_per_env=epe, alive_bonus_offset=0.25)
    ars.theta.copy_(t.from_numpy(theta))
    d_dev = t.from_numpy(delta).cuda()
    # perturb: into the tensor the policy was given
    cand = ars.perturb(d_dev)
    assert cand.data_ptr() == ars.policy.get_params().data_ptr()
    assert np.array_equal(bits(host(cand)), bits(E.perturb(theta, delta, 0.05)))
    # account: after every step of a 12-step sequence
    rew, done = A.sequence(N, 12, seed=m)
    r_dev, d_done = t.from_numpy(rew).cuda(), t.from_numpy(done).cuda()
    twin = E.Accounts(N, epe)
    ars.begin()
    assert ars.alive() == N and host(ars.get("alive")).all() and not host(ars.get("len")).any()
    for k in range(12):
        ars.account(r_dev[k], d_done[k])
        twin.account(rew[k], done[k])
        assert np.array_equal(bits(host(ars.get("ret"))), bits(twin.ret)), k
        assert np.array_equal(host(ars.get("len")), twin.len) and np.array_equal(host(ars.get("episodes")), twin.episodes), k
        assert np.array_equal(host(ars.get("alive")), twin.alive), k
        assert int(ars.get("n_alive").item()) == twin.n_alive == ars.alive(), k
    # the candidates' returns and the step sum
    R = host(ars.candidate_returns())
    R_twin, steps_twin = twin.returns(n_delta, 0.25)
    assert np.array_equal(bits(R), bits(R_twin)) and int(ars.get("steps").item()) == steps_twin
    # finish: idx and w equal, theta equal to the twin's apply fed the device's step, std and step within the derived bounds
    ars.finish()
    idx, w, (std, step) = host(ars.get("idx")), host(ars.get("w")), host(ars.get("stats"))
    assert int(ars.get("steps").item()) == steps_twin and np.array_equal(bits(host(ars.get("returns"))), bits(R_twin))
    i_twin, w_twin, std_twin, step_twin = E.select(R_twin, n_top, 0.02)
    assert np.array_equal(idx, i_twin) and np.array_equal(bits(w), bits(w_twin))
    assert np.array_equal(bits(host(ars.theta)), bits(E.apply(theta, delta, idx, w, step)))
    s = A.select(R_twin, n_top, 0.02)
    r_std, r_step = abs(float(std) - s["std"]) / s["e_std"], abs(float(step) - s["step"]) / s["e_step"]
    rec = dict(m=m, n_delta=n_delta, n_top=n_top, n_params=n_params, std_ratio_to_bound=r_std, step_ratio_to_bound=r_step,
               std_bits_equal_host=bool(bits(std) == bits(std_twin)), step_bits_equal_host=bool(bits(step) == bits(step_twin)))
    print("ars parity:", json.dumps(rec))
    record(rec)
    assert r_std <= 1.0 and r_step <= 1.0, rec
    ars.close()


@pytest.mark.parametrize("n_delta, n_top", [(5, 2), (64, 16), (65, 33), (1024, 300), (1024, 1023)])
def test_tie_cases_and_two_finishes(torch_cuda, n_delta, n_top):
    """integer returns with ties through the cut (every environment carries its candidate's return: m = 1): idx and w as the twin's; a
    second finish on the same inputs gives the same bits"""
    t = torch_cuda
    n_params = 257
    R = A.tied_returns(n_delta, n_top, seed=n_delta)
    theta, delta = inputs(n_delta, n_params, n_delta)
    ars = learner(t, 1, n_delta, n_top, n_params)
    d_dev = t.from_numpy(delta).cuda()
    ars.begin()
    ars.account(t.from_numpy(R).cuda(), t.ones(2 * n_delta, dtype=t.uint8, device="cuda"))
    assert ars.alive() == 0
    out = []
    for _ in range(2):
        ars.theta.copy_(t.from_numpy(theta))
        ars.finish(d_dev)
        out.append([host(ars.get(k)) for k in ("returns", "idx", "w", "stats")] + [host(ars.theta)])
    assert np.array_equal(out[0][0], R)
    i_twin, w_twin, _, _ = E.select(R, n_top, 0.02)
    assert np.array_equal(out[0][1], i_twin) and np.array_equal(bits(out[0][2]), bits(w_twin))
    score = np.maximum(R[:n_delta], R[n_delta:])
    assert out[0][1].tolist() == sorted(range(n_delta), key=lambda k: (-score[k], k))[:n_top]
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(bits(out[0][4]), bits(E.apply(theta, delta, out[0][1], out[0][2], out[0][3][1])))
    ars.close()


# (JUMPING_IN_PLACE_PPO: the jumping-in-place task with a reward in every step; JUMPING_IN_PLACE pays at the episode's end alone, past this horizon)
KW = dict(task_env="JUMPING_IN_PLACE_PPO", observation_space_mode="ARS_BASIC", action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True,
          enable_action_filter=True, env_randomizer_mode="GROUND_RANDOMIZER", seed=5)


def real(torch, n_delta=2, m=4, auto_reset=False, **kw):
    from qs_amd import DeviceARS, DevicePolicy, DeviceVecNormalize, QuadrupedVecEnv
    n = 2 * n_delta * m
    env = DeviceVecNormalize(QuadrupedVecEnv(num_envs=n, device=0, auto_reset=auto_reset, **KW), training=True, norm_reward=False)
    pol = DevicePolicy(env.obs_dim, env.action_dim, net_arch=(), activation="none", bias=False, num_envs=n, n_policies=2 * n_delta)
    return env, pol, DeviceARS(env, pol, n_delta=n_delta, **kw)


def close(*things):
    for x in things:
        x.close()


class Tape:
    """a fabricated environment: step t hands out row t of prepared rewards and dones"""

    def __init__(self, torch, rew, done):
        self.rew, self.done, self.num_envs, self.t = torch.from_numpy(rew).cuda(), torch.from_numpy(done).cuda(), rew.shape[1], 0
        self.obs = torch.zeros((self.num_envs, 1), device="cuda")

    def reset_tensor(self):
        self.t = 0
        return self.obs

    def step_tensor(self, actions):
        self.t += 1
        return self.obs, self.rew[self.t - 1], self.done[self.t - 1], None


def test_check_every_does_not_change_the_result(torch_cuda):
    """every environment is dead after step 10 and the rewards go on for 40: looking at the counter every step stops the rollout there,
    never looking runs to the horizon, and the accounts, the returns and theta are the same bits"""
    t = torch_cuda
    m, n_delta, n_params = 3, 5, 168
    rew, done = A.sequence(2 * n_delta * m, 40, seed=9)
    done[9] = 1
    _, delta = inputs(n_delta, n_params, 9)
    got = []
    for every in (1, 1000):
        pol = Params(t, 2 * n_delta * m, 2 * n_delta, n_params)
        pol.act = lambda obs: obs
        from qs_amd import DeviceARS
        ars = DeviceARS(Tape(t, rew, done), pol, n_delta=n_delta, n_top=2, horizon=40, check_every=every)
        ars.perturb(t.from_numpy(delta).cuda())
        R = host(ars.rollout())
        ars.finish()
        got.append((host(ars.get("ret")), host(ars.get("len")), R, host(ars.theta), ars.last_rollout_steps))
        ars.close()
    for a, b in zip(got[0][:4], got[1][:4]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert (got[0][4], got[1][4]) == (10, 40) and got[0][1].max() == 10 and np.abs(got[0][3]).max() > 0


def test_rollout_against_the_torch_accumulation(torch_cuda):
    """two iterations on a real environment, linear policy, n_delta = 2, m = 4, horizon 20: a second, identically seeded environment driven by
    the SAME candidate tensor with examples/ars.py's torch accumulation gives the per-environment returns and lengths bit for bit"""
    t = torch_cuda
    from qs_amd import DevicePolicy, DeviceVecNormalize, QuadrupedVecEnv
    env, pol, ars = real(t, horizon=20, check_every=16, seed=1)
    n = env.num_envs
    env2 = DeviceVecNormalize(QuadrupedVecEnv(num_envs=n, device=0, auto_reset=False, **KW), training=True, norm_reward=False)
    pol2 = DevicePolicy(env2.obs_dim, env2.action_dim, net_arch=(), activation="none", bias=False, num_envs=n, n_policies=4)
    pol2.set_params(ars.candidates)
    for it in range(2):
        ars.perturb(ars.sample_delta())
        returns = host(ars.rollout())
        ret_dev, len_dev = host(ars.get("ret")), host(ars.get("len"))
        obs = env2.reset_tensor()
        ret = t.zeros(n, device="cuda")
        length = t.zeros(n, dtype=t.int32, device="cuda")
        alive = t.ones(n, dtype=t.bool, device="cuda")
        for _ in range(ars.last_rollout_steps):
            obs, rew, done, trunc = env2.step_tensor(pol2.act(obs))
            ret += env2.old_reward * alive
            length += alive
            alive &= ~done.bool()
        assert np.array_equal(bits(ret_dev), bits(host(ret))), it
        assert np.array_equal(len_dev, host(length)), it
        assert int(ars.get("steps").item()) == int(len_dev.sum())
        R_twin, _ = E.returns(ret_dev, len_dev, 2, 0.0)
        assert np.array_equal(bits(returns), bits(R_twin))
        ars.finish()
    assert np.abs(ret_dev).max() > 0 and len_dev.min() >= 1
    close(ars, pol2, env2)
    # learn: theta moves and stays finite, the timesteps are the device's sum, the state dict is what layers_from_state_dict reads
    lines = []
    ars2_env, ars2_pol, ars2 = real(t, horizon=20, seed=1)
    ars2.learn(20 * n + 1, log=lines.append)
    theta = host(ars2.theta)
    assert np.isfinite(theta).all() and np.abs(theta).max() > 0 and ars2.num_timesteps > 0 and len(lines) == ars2.iteration >= 2
    from qs_amd.policy import flatten_layers, layers_from_state_dict
    layers, _ = layers_from_state_dict(ars2.state_dict(), algo="ars")
    assert np.array_equal(flatten_layers(layers, bias=False), theta)
    one = ars2.to_policy(3)
    assert one.n_policies == 1 and np.array_equal(host(one.get_params())[0], theta)
    close(one, ars2, ars2_pol, ars2_env, pol, env)


def test_refusals(torch_cuda):
    t = torch_cuda
    from qs_amd import DeviceARS
    with pytest.raises(ValueError, match="num_envs"):
        DeviceARS(None, Params(t, 31, 10, 168), n_delta=5)                 # N not divisible by P
    with pytest.raises(ValueError, match="n_top"):
        learner(t, 3, 5, 6, 168)
    with pytest.raises(ValueError, match="n_delta"):
        DeviceARS(None, Params(t, 2050, 2050, 1), n_delta=1025)
    with pytest.raises(ValueError, match="n_policies"):
        DeviceARS(None, Params(t, 30, 5, 168), n_delta=5)
    env, pol, ars = real(t)                                                 # auto_reset=False
    with pytest.raises(ValueError, match="episodes_per_env"):
        DeviceARS(env, pol, n_delta=2, episodes_per_env=2)
    close(ars, pol, env)
    ars = learner(t, 3, 5, 2, 168)
    good_r, good_d = t.zeros(30, device="cuda"), t.zeros(30, dtype=t.uint8, device="cuda")
    for name, r, d in (("raw_reward", good_r.double(), good_d), ("raw_reward", good_r.cpu(), good_d), ("raw_reward", t.zeros(31, device="cuda"), good_d),
                       ("done", good_r, good_d.bool()), ("done", good_r, good_d.cpu()), ("done", good_r, good_d[:29])):
        with pytest.raises(ValueError, match=name):
            ars.account(r, d)
    for bad in (t.zeros((5, 167), device="cuda"), t.zeros((5, 168), device="cuda", dtype=t.float64), t.zeros((5, 168)), t.zeros((168, 5), device="cuda").T):
        with pytest.raises(ValueError, match="delta"):
            ars.perturb(bad)
    ars.close()
    env, pol, ars = real(t, auto_reset=True, episodes_per_env=2, horizon=3)   # with auto-reset it is taken
    ars.train_iteration()
    close(ars, pol, env)
