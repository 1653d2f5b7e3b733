"""qs_amd/handle.py without a device: the argument check every handle shares (its five refusals, in order, with class and text), the one
"who is meant" -> uint8 mask converter against masks built by hand, and the three questions the learners ask of an environment."""
import ctypes as C

import numpy as np
import pytest
import torch

from qs_amd import handle as H

CPU = torch.device("cpu")


def test_ptr():
    x = torch.zeros(3)
    assert H.ptr(None) is None
    assert isinstance(H.ptr(x), C.c_void_p) and H.ptr(x).value == x.data_ptr()


def test_tensor_arg_refuses_in_order_and_returns_the_pointer():
    good = torch.zeros((4, 3))
    p = H.tensor_arg("obs", good, (4, 3), torch.float32, CPU, "learner")
    assert isinstance(p, C.c_void_p) and p.value == good.data_ptr()
    # every bad argument below also has every later fault: the message is the first one's
    wrong = torch.zeros((3, 5), dtype=torch.float64, device="meta")[:, ::2]
    assert not wrong.is_contiguous()
    cases = ((np.zeros((3, 5)), "obs must be a torch tensor, got ndarray"),
             (wrong, "obs must be float32, got torch.float64"),
             (wrong.float(), "obs is on meta, this learner on cpu"),
             (torch.zeros((3, 5))[:, ::2], r"obs has shape \(3, 3\), expected \(4, 3\)"),
             (torch.zeros((4, 6))[:, ::2], "obs must be contiguous"))
    for kind in (ValueError, TypeError):
        for k, (bad, text) in enumerate(cases):
            with pytest.raises(kind if k < 2 else ValueError, match=text) as e:
                H.tensor_arg("obs", bad, (4, 3), torch.float32, CPU, "learner", kind_error=kind)
            assert type(e.value) is (kind if k < 2 else ValueError)
    with pytest.raises(ValueError, match="done must be uint8, got torch.bool"):
        H.tensor_arg("done", torch.zeros(4, dtype=torch.bool), (4,), torch.uint8, CPU, "planner")
    with pytest.raises(ValueError, match="this planner on cpu"):
        H.tensor_arg("done", torch.zeros(4, dtype=torch.uint8, device="meta"), (4,), torch.uint8, CPU, "planner")


N = 5
BY_HAND = torch.tensor([0, 1, 0, 1, 1], dtype=torch.uint8)      # environments 1, 3 and 4


@pytest.mark.parametrize("who", [BY_HAND.bool(), BY_HAND.clone(), torch.tensor([4, 1, 3]), torch.tensor([[1, 3], [4, 4]]), [3, 1, 4], (1, 3, 4), np.array([1, 4, 3]),
                                 np.array([1, 3, 4], np.int32), torch.tensor([1, 3, 4], dtype=torch.int32)],
                         ids=["bool", "uint8", "int64", "int64-2d", "list", "tuple", "numpy", "numpy-int32", "int32"])
def test_env_mask_against_a_mask_built_by_hand(who):
    m = H.env_mask(who, N, CPU)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (N,) and m.is_contiguous() and m.device == CPU
    assert torch.equal(m, BY_HAND)


def test_env_mask_edges():
    assert H.env_mask(None, N, CPU) is None
    assert H.env_mask(None, N, "cpu") is None
    for one in (3, np.int64(3), torch.tensor(3), [3], np.array(3)):
        assert H.env_mask(one, N, CPU).tolist() == [0, 0, 0, 1, 0], one
    assert H.env_mask([], N, CPU).tolist() == [0] * N and H.env_mask([2, 2], N, "cpu").tolist() == [0, 0, 1, 0, 0]
    # a mask is used as it is: the same memory where it is contiguous uint8, a view of the same memory where it is bool
    u8, b = BY_HAND.clone(), BY_HAND.bool()
    assert H.env_mask(u8, N, CPU).data_ptr() == u8.data_ptr() and H.env_mask(b, N, CPU).data_ptr() == b.data_ptr()
    strided = torch.stack([BY_HAND, 1 - BY_HAND], 1)[:, 0]
    assert not strided.is_contiguous()
    m = H.env_mask(strided, N, CPU)
    assert m.is_contiguous() and torch.equal(m, BY_HAND)
    assert torch.equal(H.env_mask(strided.bool(), N, CPU), BY_HAND)
    # (ids in a tensor on the handle's device -- here the CPU -- are not looked at on the host: not among these)
    for bad in ([0, N], [-1], N, np.array([1, 7]), np.int64(-2)):
        with pytest.raises(ValueError, match=rf"environment ids must lie in \[0, {N}\)"):
            H.env_mask(bad, N, CPU)
    for bad in (torch.ones(N - 1, dtype=torch.bool), torch.ones((N, 1), dtype=torch.uint8), torch.ones(N + 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"a mask must have shape \(5,\)"):
            H.env_mask(bad, N, CPU)


def test_to_device_nowait_on_the_host():
    a = np.arange(6, dtype=np.int32).reshape(2, 3)[:, ::2]
    t = H.to_device_nowait(a, CPU)
    assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == [[0, 2], [3, 5]]


class Env:
    auto_reset = False

    def step_tensor(self, actions, active=None):
        raise AssertionError("never stepped")


class Wrapper:
    def __init__(self, venv):
        self.venv, self.old_reward = venv, "raw"

    def step_tensor(self, actions, terminal_obs=None):
        raise AssertionError("never stepped")


class Neither:
    pass


def test_what_the_learners_ask_of_an_environment():
    env, nothing = Env(), Neither()
    wrapped = Wrapper(env)
    assert H.takes_active(env) is True and H.takes_active(wrapped) is False and H.takes_active(nothing) is False
    assert H.auto_reset_of(env) is False and H.auto_reset_of(wrapped) is False and H.auto_reset_of(nothing) is None
    cfg = Neither()
    cfg.auto_reset = 1
    nothing.cfg = cfg
    assert H.auto_reset_of(nothing) is True and H.auto_reset_of(Wrapper(nothing)) is True
    assert H.raw_reward_of(env, "rew") == "rew" and H.raw_reward_of(wrapped, "rew") == "raw" and H.raw_reward_of(Neither(), "rew") == "rew"
    assert H.raw_reward_of(None, "rew") == "rew"                     # (a learner without an environment never steps; the rule still answers)


def test_close_is_idempotent_and_leaves_a_wrapped_handle_alone():
    """the lifecycle of DeviceHandle on a stand-in library: one destroy per handle, none for a handle the object merely forwards to"""
    gone = []

    class Lib:
        def qs_fake_destroy(self, h):
            gone.append(h.value)

    class Owner(H.DeviceHandle):
        _prefix = "qs_fake"

        def __init__(self, value):
            self.lib, self.h = Lib(), C.c_void_p(value)

    class Forwarder(H.DeviceHandle):
        _prefix = "qs_fake"

        def __init__(self, inner):
            self.lib, self.inner = Lib(), inner

        def __getattr__(self, name):
            return getattr(self.inner, name)

    a = Owner(7)
    a.close()
    a.close()
    assert gone == [7] and not a.h
    del a
    b = Owner(9)
    f = Forwarder(b)
    assert f.h.value == 9
    f.close()
    del f
    assert gone == [7]
    del b
    assert gone == [7, 9]
    half_built = Owner.__new__(Owner)           # a constructor that raised before the handle existed
    half_built.close()
    del half_built
    assert gone == [7, 9]
