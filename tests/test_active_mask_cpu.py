"""step_tensor(active=) without a device: where the mask stands in the two prototypes, the float64 restatement of the masked VecNormalize
(tests/active_ref.py) is the unmasked one under a full mask, and the argument errors that are raised before anything is launched."""
import os
import re

import numpy as np
import pytest

from active_ref import MaskedVecNormalizeRef

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_mask_is_the_third_and_the_fifth_argument():
    """of qs_step_masked and of qs_norm_step_masked, a const uint8_t* in both (every argument's kind against the binding: test_abi_cpu.py)"""
    header = open(os.path.join(REPO, "include", "qs_amd.h")).read()
    bare = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "qs_step_masked(qs_handle* h, const float* actions, const uint8_t* active ," in bare
    assert "qs_norm_step_masked(qs_norm* h, float* obs , float* rew , const uint8_t* done , const uint8_t* active ," in bare


def test_a_full_mask_is_no_mask_in_the_reference():
    rng = np.random.default_rng(0)
    n, o = 40, 7
    a, b = MaskedVecNormalizeRef(n, o), MaskedVecNormalizeRef(n, o)
    for t in range(6):
        obs, rew, done = rng.normal(size=(n, o)).astype(np.float32), rng.normal(size=n).astype(np.float32), rng.random(n) < 0.2
        xa, xb = a.step(obs, rew, done), b.step(obs, rew, done, active=np.ones(n, np.uint8))
        assert np.array_equal(xa[0], xb[0]) and np.array_equal(xa[1], xb[1])
        assert np.array_equal(a.returns, b.returns)
    for k, v in a.stats().items():
        assert np.array_equal(v, b.stats()[k]), k
    # ... and an empty one changes nothing; a partial one counts its rows
    before = {k: np.copy(v) for k, v in b.stats().items()}
    ret = b.returns.copy()
    b.step(obs, rew, np.ones(n, bool), active=np.zeros(n, bool))
    assert all(np.array_equal(before[k], v) for k, v in b.stats().items()) and np.array_equal(ret, b.returns)
    on = np.arange(n) % 3 == 0
    b.step(obs, rew, np.ones(n, bool), active=on)
    assert b.stats()["obs_count"] == before["obs_count"] + on.sum() and np.array_equal(b.returns[~on], ret[~on]) and not b.returns[on].any()


def test_the_mask_is_checked_before_any_launch():
    import torch
    from qs_amd.vec_env import active_mask
    ok = active_mask(torch.ones(5, dtype=torch.bool), 5, "cpu")
    assert ok.dtype == torch.uint8 and ok.tolist() == [1] * 5
    assert active_mask(torch.zeros(5, dtype=torch.uint8), 5, "cpu").dtype == torch.uint8
    strided = active_mask(torch.ones(10, dtype=torch.uint8)[::2], 5, "cpu")
    assert strided.is_contiguous()
    for bad, word in ((torch.ones(4, dtype=torch.bool), "shape"), (torch.ones((5, 1), dtype=torch.bool), "shape"), (torch.ones(5), "bool or uint8"),
                      (torch.ones(5, dtype=torch.int32), "bool or uint8"), (np.ones(5, np.uint8), "torch tensor"),
                      (torch.ones(5, dtype=torch.bool, device="meta"), "is on")):
        with pytest.raises(ValueError, match="active.*" + word):
            active_mask(bad, 5, "cpu")


def test_step_tensor_signatures():
    """(the keyword does not exist before this feature)"""
    import inspect
    from qs_amd import DeviceARS, DeviceVecNormalize, QuadrupedVecEnv
    from qs_amd.sharded import ShardedVecEnv
    assert inspect.signature(QuadrupedVecEnv.step_tensor).parameters["active"].default is None
    assert list(inspect.signature(DeviceVecNormalize.step_tensor).parameters)[1:] == ["actions", "terminal_obs", "active"]
    assert inspect.signature(DeviceARS.__init__).parameters["freeze_done"].default is False
    sharded = ShardedVecEnv.__new__(ShardedVecEnv)     # (no process group: the refusal comes before anything is touched)
    with pytest.raises(NotImplementedError, match="fused row"):
        sharded.step_tensor(None, active=np.ones(1))


def test_device_ars_refuses_freeze_done_on_an_environment_without_the_keyword():
    import torch
    from qs_amd import DeviceARS

    class Policy:
        n_policies, num_envs, n_params, device = 4, 8, 3, torch.device("cpu")

    class Plain:
        num_envs = 8

        def step_tensor(self, actions):
            raise AssertionError("never stepped")

    class Masked(Plain):
        def step_tensor(self, actions, active=None):
            raise AssertionError("never stepped")

    with pytest.raises(ValueError, match="freeze_done=True needs an environment whose step_tensor takes active="):
        DeviceARS(Plain(), Policy(), n_delta=2, freeze_done=True)
    # with the keyword (or without the flag) the constructor gets as far as the device check
    for env, flag in ((Masked(), True), (Plain(), False)):
        with pytest.raises(ValueError, match="no CPU path"):
            DeviceARS(env, Policy(), n_delta=2, freeze_done=flag)
