"""ctypes driver for the TEST-ONLY host build of the PPO update (tests/emu/qs_emu_ppo_train.cpp over csrc/qs_ppo_train.h)."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO = os.path.join(_HERE, "libqs_emu_ppo_train.so")
_lib = None


class Hyper(C.Structure):
    """qs_ppo_hyper (include/qs_amd.h); qs_amd.lib.QsPpoHyper is the same layout"""
    _fields_ = [("clip_range", C.c_float), ("ent_coef", C.c_float), ("vf_coef", C.c_float), ("max_grad_norm", C.c_float),
                ("normalize_advantage", C.c_int32), ("reserved", C.c_int32),
                ("lr", C.c_double), ("beta_one", C.c_double), ("beta_two", C.c_double), ("adam_eps", C.c_double)]


def hyper(clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True, lr=3e-4, betas=(0.9, 0.999), eps=1e-5):
    return Hyper(clip_range, ent_coef, vf_coef, 3.0e38 if max_grad_norm is None else max_grad_norm, int(bool(normalize_advantage)), 0, lr, betas[0], betas[1], eps)


def build():
    return _compile(_SO, os.path.join(_HERE, "qs_emu_ppo_train.cpp"))


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp, ll = C.c_void_p, C.c_longlong
        _lib.qsept_moments.argtypes = [vp, ll, vp, C.c_int, vp, vp]
        _lib.qsept_moments.restype = None
        _lib.qsept_grad.argtypes = [vp] * 10 + [ll, vp, C.c_int, C.POINTER(Hyper), vp, vp, vp]
        _lib.qsept_adam.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(Hyper), C.c_int]
        _lib.qsept_adam.restype = C.c_float
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, shape):
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def check(actor_desc, critic_desc):
    """raises ValueError with the reason qs_ppo_create gives for a pair of descriptors it refuses"""
    err = C.create_string_buffer(512)
    if _load().qsept_check(C.byref(actor_desc), C.byref(critic_desc), err, 512):
        raise ValueError(err.value.decode())


def layout(actor_desc, critic_desc):
    """dict(n_actor, n_critic, n_total, parts, waves, lds_bytes) of the device update for this pair"""
    out = (C.c_longlong * 6)()
    assert _load().qsept_layout(C.byref(actor_desc), C.byref(critic_desc), out) == 0
    return dict(zip(("n_actor", "n_critic", "n_total", "parts", "waves", "lds_bytes"), (int(x) for x in out)))


def moments(adv, idx):
    a, i = _f(adv, -1), np.ascontiguousarray(idx, np.int64)
    m, s = np.zeros(1, np.float32), np.zeros(1, np.float32)
    _load().qsept_moments(_p(a), a.size, _p(i), i.size, _p(m), _p(s))
    return m[0], s[0]


def grad(actor_desc, critic_desc, actor_params, critic_params, log_std, obs, actions, old_log_prob, adv, returns, idx, hy):
    """-> (grad [n_total] float32, stats [8] float32, refused); the per-sample flags [B] uint8, bit 0 = the unclipped branch carried the sample's
    gradient, bit 1 = the sample counted as clipped, are left in grad.last_flags"""
    o, a = actor_desc.obs_dim, actor_desc.action_dim
    pa, pc, ls = _f(actor_params, -1), _f(critic_params, -1), _f(log_std, a)
    ob = _f(obs, (-1, o))
    total = ob.shape[0]
    ac, ol, ad, re = _f(actions, (total, a)), _f(old_log_prob, total), _f(adv, total), _f(returns, total)
    ix = np.ascontiguousarray(idx, np.int64)
    g, st, fl = np.zeros(pa.size + pc.size + a, np.float32), np.zeros(8, np.float32), np.zeros(ix.size, np.uint8)
    rc = _load().qsept_grad(C.byref(actor_desc), C.byref(critic_desc), _p(pa), _p(pc), _p(ls), _p(ob), _p(ac), _p(ol), _p(ad), _p(re), total, _p(ix), ix.size,
                            C.byref(hy), _p(g), _p(st), _p(fl))
    assert rc >= 0, rc
    grad.last_flags = fl
    return g, st, rc


def adam(p, m, v, g, hy, step):
    """-> (p, m, v copies after the step, the norm before clipping)"""
    p, m, v, g = (_f(x, -1).copy() for x in (p, m, v, g))
    norm = _load().qsept_adam(_p(p), _p(m), _p(v), _p(g), p.size, C.byref(hy), int(step))
    return p, m, v, float(norm)
