"""ctypes driver for the TEST-ONLY host build of PPO collection (tests/emu/qs_emu_ppo.cpp over csrc/qs_ppo.h)."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO_PPO = os.path.join(_HERE, "libqs_emu_ppo.so")
_lib = None


def build_ppo():
    return _compile(_SO_PPO, os.path.join(_HERE, "qs_emu_ppo.cpp"))


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_ppo())
        _lib.qseppo_values.argtypes = [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_void_p]
        _lib.qseppo_gae.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        _lib.qseppo_gae.restype = None
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a, shape):
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def check(actor_desc, critic_desc):
    """raises ValueError with the reason qs_ac_create gives for a pair of descriptors it refuses"""
    err = C.create_string_buffer(512)
    if _load().qseppo_check(C.byref(actor_desc), C.byref(critic_desc), err, 512):
        raise ValueError(err.value.decode())


def collect(actor_desc, critic_desc, actor_params, critic_params, obs, eps, log_std):
    """-> env_actions [N, A] (clipped), actions [N, A] (unclipped), values [N], log_probs [N]"""
    n, a, o = actor_desc.n_envs, actor_desc.action_dim, actor_desc.obs_dim
    pa, pc = _f(actor_params, -1), _f(critic_params, -1)
    ob, ep, ls = _f(obs, (n, o)), _f(eps, (n, a)), _f(log_std, a)
    env_act, act, val, lp = np.zeros((n, a), np.float32), np.zeros((n, a), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    rc = _load().qseppo_collect(C.byref(actor_desc), C.byref(critic_desc), _p(pa), _p(pc), _p(ob), _p(ep), _p(ls), _p(env_act), _p(act), _p(val), _p(lp))
    assert rc == 0, rc
    return env_act, act, val, lp


def values(critic_desc, critic_params, obs, mask=None, out=None):
    """V(obs) where mask (all without one); the other entries of `out` (zeros if not given) are left as they are"""
    n = critic_desc.n_envs
    pc, ob = _f(critic_params, -1), _f(obs, (n, critic_desc.obs_dim))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(n)
    v = np.zeros(n, np.float32) if out is None else _f(out, n).copy()
    assert _load().qseppo_values(C.byref(critic_desc), _p(pc), _p(ob), _p(m), 0.0, None, _p(v)) == 0
    return v


def bootstrap(critic_desc, critic_params, terminal_obs, truncated, gamma, rewards):
    """-> a copy of rewards with fmaf(gamma, V(terminal_obs), reward) where truncated"""
    n = critic_desc.n_envs
    pc, ob = _f(critic_params, -1), _f(terminal_obs, (n, critic_desc.obs_dim))
    m = np.ascontiguousarray(truncated, np.uint8).reshape(n)
    r = _f(rewards, n).copy()
    assert _load().qseppo_values(C.byref(critic_desc), _p(pc), _p(ob), _p(m), float(gamma), _p(r), None) == 0
    return r


def gae(rewards, values_, episode_starts, last_values, last_dones, gamma, lam):
    """arrays [T, N] -> advantages, returns [T, N]"""
    r = np.ascontiguousarray(rewards, np.float32)
    T, N = r.shape
    v, es = _f(values_, (T, N)), _f(episode_starts, (T, N))
    lv, ld = _f(last_values, N), np.ascontiguousarray(last_dones, np.uint8).reshape(N)
    adv, ret = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    _load().qseppo_gae(_p(r), _p(v), _p(es), _p(lv), _p(ld), T, N, float(gamma), float(lam), _p(adv), _p(ret))
    return adv, ret
