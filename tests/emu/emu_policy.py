"""ctypes driver for the TEST-ONLY host build of policy inference (tests/emu/qs_emu_policy.cpp over csrc/qs_policy.h)."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO_POLICY = os.path.join(_HERE, "libqs_emu_policy.so")
_lib = None


def build_policy():
    return _compile(_SO_POLICY, os.path.join(_HERE, "qs_emu_policy.cpp"))


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_policy())
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def param_count(desc):
    """parameters per policy of a qs_amd.lib.QsPolicyDesc; raises ValueError with the library's reason for a bad one"""
    err = C.create_string_buffer(256)
    n = _load().qsepol_param_count(C.byref(desc), err, 256)
    if n < 0:
        raise ValueError(err.value.decode())
    return n


def act(desc, params, obs, eps=None, log_std=None):
    """params [P, n_params], obs [N, obs_dim], eps [N, A] / log_std [A] or None -> actions [N, A], mean [N, A], log_prob [N] (None without eps)"""
    n, a = desc.n_envs, desc.action_dim
    par = np.ascontiguousarray(params, np.float32).reshape(desc.n_policies, param_count(desc))
    ob = np.ascontiguousarray(obs, np.float32).reshape(n, desc.obs_dim)
    ep = None if eps is None else np.ascontiguousarray(eps, np.float32).reshape(n, a)
    ls = None if log_std is None else np.ascontiguousarray(log_std, np.float32).reshape(a)
    actions, mean = np.zeros((n, a), np.float32), np.zeros((n, a), np.float32)
    lp = None if ep is None else np.zeros(n, np.float32)
    rc = _load().qsepol_act(C.byref(desc), _p(par), _p(ob), _p(ep), _p(ls), _p(actions), _p(mean), _p(lp))
    assert rc == 0, rc
    return actions, mean, lp


def layout(desc, critic=None):
    """(act_stride, w_floats, wide, waves, LDS bytes, LDS bytes of a one-wave launch) of k_policy for `desc`, of k_actor_critic with a critic"""
    out = (C.c_int * 6)()
    rc = _load().qsepol_layout(C.byref(desc), None if critic is None else C.byref(critic), 1 if critic is None else 2, out)
    assert rc == 0, rc
    return tuple(out)


def tanh(x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    _load().qsepol_tanh(_p(x), x.size, _p(y))
    return y
