"""A hand-over late in a long env step on the GPU: action_repeat = 300 (time_step 0.001, one solver iteration), a robot on its side dropped
so that its first body contact comes ~270 substeps into the first step.  The step kernel hands its wave over to the full build at a substep
index beyond 255 (qs_env.h, Env::step); the wave's other 15 environments must not notice, and the dropped robot follows the oracle.
tests/test_emu_hand_over.py holds the same hand-over bit for bit against the full build on the host."""
import numpy as np
import pytest

from test_gpu_round2 import fallen_states, vec_env

pytestmark = pytest.mark.gpu

ON_ITS_SIDE = [0.6631, 0.0, 0.0, 0.7485]   # roll ~1.45 rad
DROP_Z = 0.52                              # first body contact at substep ~274 of the first step (qse_step_build: resume)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


@pytest.mark.parametrize("step_kernel", ["1", "2"])
def test_late_hand_over_leaves_wave_mates_alone(torch_cuda, monkeypatch, step_kernel):
    """Environment k of wave 0 (with the dropped robot) against its twin k + 16 of wave 1 (same state, same actions, no such neighbour),
    bitwise, step after step, with each step kernel forced (QS_STEP_VARIANT is read by qs_create); the first step's many-rows substeps
    show that the wave handed over late, not at k mod 256; every robot against the float32 oracle at the fallen-robot tolerances of
    test_gpu_round2.py::test_fallen_robots_parity."""
    from oracle.qso import Oracle
    monkeypatch.setenv("QS_STEP_VARIANT", step_kernel)
    n, odd = 32, 5
    v = vec_env(n, time_step=0.001, action_repeat=300, enable_action_filter=False)
    assert v.cfg.action_repeat == 300 and v.cfg.solver_iters == 1
    o = Oracle(v.cfg, "f32")
    o.reset(); v.reset()
    rng = np.random.default_rng(11)
    s = o.get_state()
    s[16:] = s[:16]
    s[odd] = fallen_states(s[odd:odd + 1], rng)[0]
    s[odd, 2] = DROP_Z; s[odd, 3:7] = ON_ITS_SIDE
    twins = np.array([k for k in range(16) if k != odd])
    hold = np.array(v.cfg.settle_action[:v.cfg.action_dim], np.float32)     # the standing robots hold their pose: no rare path of theirs
    for t in range(6):
        st = s if t == 0 else o.get_state()
        o.set_state(st); v.set_state(st.astype(np.float32))
        a = np.tile(hold + 0.1 * rng.uniform(-1, 1, size=(16, len(hold))), (2, 1)).astype(np.float32)
        rare0 = v.counter("limit_path_substeps")
        obs = v.step(a)[0]
        o.step(a)
        rare = v.counter("limit_path_substeps") - rare0
        if t == 0:   # wave 0 went on in the full build from substep ~274: at most the last 44 substeps took the many-rows solve
            assert 0 < rare <= 300 - 256, rare
        sv, so = v.get_state().cpu().numpy(), o.get_state()
        obs = obs.cpu().numpy() if hasattr(obs, "cpu") else obs
        assert np.array_equal(sv[twins], sv[twins + 16]), f"step {t}"
        assert np.array_equal(obs[twins], obs[twins + 16]), f"step {t}"
        ff = v.get_info("foot_force").cpu().numpy()
        assert np.array_equal(ff[twins], ff[twins + 16]), f"step {t}"
        np.testing.assert_allclose(sv[:, :7], so[:, :7], atol=5e-5, err_msg=f"pose step {t}")
        np.testing.assert_allclose(sv[:, 7:13], so[:, 7:13], atol=2e-2, err_msg=f"base velocity step {t}")
        np.testing.assert_allclose(sv[:, 13:25], so[:, 13:25], atol=2e-4, err_msg=f"q step {t}")
        np.testing.assert_allclose(sv[:, 25:], so[:, 25:], atol=1e-1, err_msg=f"qd step {t}")
    assert sv[odd, 2] < 0.2                   # it did land
    v.close()
