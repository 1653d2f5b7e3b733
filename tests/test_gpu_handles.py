"""What qs_amd.handle.DeviceHandle owns, for each of the seven handle classes at its smallest legal shape: the stream hand-off (a call under
a fresh non-default stream gives the bits it gives on the default stream) and the lifecycle (close() twice, the second a no-op; dropping an
unclosed object frees its handle and nothing else)."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, OBS, ACT, ARCH, N_DELTA, T = 16, 5, 3, (8,), 2, 2
M, CAND, HOR = 1, 3, 2
ENV_KW = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True,
              enable_action_filter=True, env_randomizer_mode="GROUND_RANDOMIZER", noise=False, seed=3, auto_reset=True, reset_lookahead=0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def randn(t, *shape, seed=0):
    return t.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()


class Params:
    """what DeviceARS uses of a policy (tests/test_gpu_ars.py)"""

    def __init__(self, t):
        self.num_envs, self.n_policies, self.n_params, self.device, self._params = N, 2 * N_DELTA, 7, t.device("cuda", 0), None

    def set_params(self, p):
        self._params = p


# every maker -> (the object, call() -> the tensors one call of it leaves behind, what else to close at the end); call() is a pure function
# of the object's state as the maker leaves it, or puts that state back first
def make_env(t):
    from qs_amd import QuadrupedVecEnv
    env = QuadrupedVecEnv(num_envs=N, device=0, **ENV_KW)
    env.reset_tensor()
    snap, zero = env.snapshot(), t.zeros((N, env.action_dim), device="cuda")

    def call(first=[True]):
        if not first[0]:
            env.restore(snap)
            t.cuda.synchronize()
        first[0] = False
        return env.step_tensor(zero)
    return env, call, ()


def make_norm(t):
    from qs_amd import DeviceVecNormalize, QuadrupedVecEnv
    env = QuadrupedVecEnv(num_envs=N, device=0, **ENV_KW)
    w = DeviceVecNormalize(env, training=False)
    w.set_stats(np.full(env.obs_dim, 0.25), np.full(env.obs_dim, 2.0), 100.0, 0.5, 3.0, 100.0)
    w.reset_tensor()
    snap, zero = w.snapshot(), t.zeros((N, env.action_dim), device="cuda")

    def call(first=[True]):
        if not first[0]:
            w.restore(snap)
            t.cuda.synchronize()
        first[0] = False
        return w.step_tensor(zero) + (w.old_obs, w.old_reward)
    return w, call, (env,)


def make_policy(t):
    from qs_amd import DevicePolicy
    pol = DevicePolicy(OBS, ACT, net_arch=ARCH, num_envs=N)
    pol.set_params(0.3 * randn(t, pol.n_params, seed=1))
    obs, eps = randn(t, N, OBS, seed=2), randn(t, N, ACT, seed=3)
    return pol, lambda: pol.act(obs, eps=eps, want_mean=True, want_log_prob=True), ()


def make_ac(t):
    from qs_amd import DeviceActorCritic
    ac = DeviceActorCritic(OBS, ACT, net_arch=ARCH, num_envs=N)
    obs, eps = randn(t, N, OBS, seed=2), randn(t, N, ACT, seed=3)
    rows = (t.zeros((N, OBS), device="cuda"), t.zeros((N, ACT), device="cuda"), t.zeros(N, device="cuda"), t.zeros(N, device="cuda"))
    return ac, lambda: (ac.collect(obs, eps, *rows),) + rows, ()


def make_ppo(t):
    from qs_amd import DeviceActorCritic, DevicePPO
    ac = DeviceActorCritic(OBS, ACT, net_arch=ARCH, num_envs=N)
    algo = DevicePPO(None, ac, n_steps=T, batch_size=T * N, update="device")
    buf = algo.buffer
    for k, name in enumerate(("observations", "actions", "log_probs", "advantages", "returns")):
        getattr(buf, name).copy_(randn(t, *getattr(buf, name).shape, seed=10 + k))
    idx = t.arange(T * N, device="cuda").flip(0).contiguous()

    def call():
        algo.grad_minibatch(idx)
        return algo.grad, algo._stats
    return algo, call, (ac,)


def make_ars(t):
    from qs_amd import DeviceARS
    ars = DeviceARS(None, Params(t), n_delta=N_DELTA, zero_policy=True)
    ars.theta.copy_(randn(t, ars.n_params, seed=4))
    delta = randn(t, N_DELTA, ars.n_params, seed=5)
    return ars, lambda: (ars.perturb(delta),), ()


def make_mpc(t):
    from qs_amd import DeviceMPC
    mpc = DeviceMPC(None, M, CAND, HOR, action_dim=ACT)
    eps = randn(t, HOR, M * CAND, ACT, seed=6)

    def call():
        mpc.sample(eps)
        return mpc.get("seq"), mpc.get("score"), mpc.get("running")
    return mpc, call, ()


MAKERS = dict(QuadrupedVecEnv=make_env, DeviceVecNormalize=make_norm, DevicePolicy=make_policy, DeviceActorCritic=make_ac, DevicePPO=make_ppo,
              DeviceARS=make_ars, DeviceMPC=make_mpc)


def handle_of(obj):
    return obj.hp if type(obj).__name__ == "DevicePPO" else obj.h


@pytest.mark.parametrize("name", list(MAKERS))
def test_stream_hand_off_and_lifecycle(torch_cuda, name):
    t = torch_cuda
    from qs_amd.handle import DeviceHandle
    obj, call, others = MAKERS[name](t)
    assert isinstance(obj, DeviceHandle) or isinstance(obj._update, DeviceHandle)
    assert handle_of(obj)
    first = call()
    want = [x.clone() for x in first]
    for x in first:                                  # (reused output buffers: what the second call leaves in them is its own work)
        x.zero_()
    t.cuda.synchronize()
    s = t.cuda.Stream()
    with t.cuda.stream(s):
        got = [x.clone() for x in call()]
    s.synchronize()
    assert len(got) == len(want) and len(want) >= 1
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), (name, k)
    assert any(bool(a.any()) for a in want), "the call left zeros only: the comparison shows nothing"
    t.cuda.synchronize()
    obj.close()
    assert not handle_of(obj)
    obj.close()                                      # a no-op
    assert not handle_of(obj)
    for o in others:
        o.close()
    # an unclosed one is dropped: its handle goes, and what it wraps stays usable
    obj, call, others = MAKERS[name](t)
    call()
    t.cuda.synchronize()
    del obj, call
    gc.collect()
    if name == "DeviceVecNormalize":
        env = others[0]
        assert env.h and env.get_state().shape == (N, 37)
    t.cuda.synchronize()
    for o in others:
        o.close()
