"""Solo waves (qs_solo_waves): a robot about to put a link on the floor steps in a workgroup of its own, next to copies of the
parked record.  Every output is bit for bit what the handle gives with solo waves off; only who computes it changes."""
import numpy as np
import pytest

from test_gpu_round2 import RAW, fallen_states, vec_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def A(x):
    return x.cpu().numpy().copy()


def fallen_half(v, seed, lo=0.16, hi=0.3):
    """the handle's reset state with every other robot thrown on the floor, just above it: they land within the first steps"""
    rng = np.random.default_rng(seed)
    s = A(v.get_state())
    lying = np.arange(len(s)) % 2 == 1
    s[lying] = fallen_states(s[lying], rng)
    s[lying, 2] = rng.uniform(lo, hi, size=lying.sum())
    return s.astype(np.float32)


def test_on_off_overflow_and_reach(torch_cuda):
    """Three handles from one state under the same torques: solo waves off; every robot at risk with room for 8 (the solo path and the
    overflow back into the home waves both run); the default reach with room for everybody."""
    torch = torch_cuda
    n = 32
    hs = [vec_env(n, reset_lookahead=2, solo_waves=0, **RAW),
          vec_env(n, reset_lookahead=2, solo_waves=8, solo_reach=1e3, **RAW),
          vec_env(n, reset_lookahead=2, solo_waves=32, **RAW)]
    for v in hs:
        v.reset()
    s = fallen_half(hs[0], 31)
    for v in hs:
        v.set_state(s)
    rng = np.random.default_rng(32)
    for t in range(40):
        tau = torch.as_tensor(rng.uniform(-4, 4, size=(n, 12)).astype(np.float32), device=hs[0].device)
        outs = []
        for v in hs:
            obs, rew, done, _ = v.step_tensor(tau)
            outs.append((A(v.get_state()), A(obs), A(rew), A(done), A(v.get_info("foot_force"))))
        for k in (1, 2):
            for name, a, b in zip(("state", "obs", "reward", "done", "foot_force"), outs[0], outs[k]):
                assert np.array_equal(a, b), f"handle {k}, step {t}: {name}"
    assert hs[0].counter("limit_path_substeps") > 100 and hs[0].counter("solo_path_substeps") == 0
    for v in hs[1:]:
        assert v.counter("solo_path_substeps") > 0
    print("solo share of the many-rows wave-substeps:", [v.counter("solo_path_substeps") / v.counter("limit_path_substeps") for v in hs[1:]])
    for v in hs:
        v.close()


@pytest.mark.parametrize("n", [32, 17])
def test_headline_configuration(torch_cuda, n):
    """The benchmark's configuration in small: auto-reset with look-ahead states under random actions, 300 steps, on against off.  The
    robots that fall are reset inside solo waves."""
    torch = torch_cuda
    kw = dict(env_randomizer_mode="GROUND_RANDOMIZER", auto_reset=True, reset_lookahead=4, seed=3, body_contacts=True)
    off, on = vec_env(n, solo_waves=0, **kw), vec_env(n, solo_waves=32, **kw)
    off.reset_tensor(); on.reset_tensor()
    gen = torch.Generator(device=off.device).manual_seed(5)
    acts = torch.rand((300, n, off.action_dim), generator=gen, device=off.device) * 2 - 1
    for t in range(300):
        a = [A(x) for x in off.step_tensor(acts[t])] + [A(off.get_info("terminal_obs"))]
        b = [A(x) for x in on.step_tensor(acts[t])] + [A(on.get_info("terminal_obs"))]
        for name, x, y in zip(("obs", "reward", "done", "truncated", "terminal_obs"), a, b):
            assert np.array_equal(x, y), f"step {t}: {name}"
    assert on.counter("resets") == off.counter("resets") > n
    assert on.counter("solo_path_substeps") > 0 and off.counter("solo_path_substeps") == 0
    print("solo share:", on.counter("solo_path_substeps") / on.counter("limit_path_substeps"), "resets:", on.counter("resets") - n)
    off.close(); on.close()


@pytest.mark.parametrize("space", [dict(), dict(action_space_mode="CPG")], ids=["default", "cpg"])
def test_parked_quads_never_vote(torch_cuda, space):
    """All standing under the zero action, everybody "at risk": every environment steps in a solo wave beside fifteen parked records, every
    home wave steps sixteen parked records -- and no wave takes a rare path."""
    torch = torch_cuda
    n = 16
    kw = dict(reset_lookahead=2, body_contacts=True, **space)
    off, on = vec_env(n, solo_waves=0, **kw), vec_env(n, solo_waves=16, solo_reach=1e3, **kw)
    off.reset_tensor(); on.reset_tensor()
    a = torch.zeros((n, off.action_dim), device=off.device)
    for t in range(50):
        x = [A(y) for y in off.step_tensor(a)] + [A(off.get_state())]
        z = [A(y) for y in on.step_tensor(a)] + [A(on.get_state())]
        for name, p, q in zip(("obs", "reward", "done", "truncated", "state"), x, z):
            assert np.array_equal(p, q), f"step {t}: {name}"
    assert on.counter("limit_path_substeps") == 0 and off.counter("limit_path_substeps") == 0
    off.close(); on.close()


def test_one_environment(torch_cuda):
    """N = 1: the fifteen tail quads of the wave step the parked record, not copies of the fallen robot -- one many-rows solve per substep
    at the most -- and the robot does what it does as environment 0 of a full handle."""
    torch = torch_cuda
    one, many = vec_env(1, reset_lookahead=2, **RAW), vec_env(32, reset_lookahead=2, solo_waves=0, **RAW)
    one.reset(); many.reset()
    s = fallen_half(many, 41)
    s[0] = s[1]                                   # environment 0 lies on the floor
    many.set_state(s); one.set_state(s[:1])
    rng = np.random.default_rng(42)
    rare0, steps = one.counter("limit_path_substeps"), 30
    for t in range(steps):
        tau = torch.as_tensor(rng.uniform(-4, 4, size=(32, 12)).astype(np.float32), device=one.device)
        one.step_tensor(tau[:1].contiguous()); many.step_tensor(tau)
        assert np.array_equal(A(one.get_state())[0], A(many.get_state())[0]), f"step {t}"
    rare = one.counter("limit_path_substeps") - rare0
    assert 0 < rare <= steps * one.cfg.action_repeat, rare
    one.close(); many.close()
