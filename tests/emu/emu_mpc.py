"""ctypes driver for the TEST-ONLY host build of the sampling planner (tests/emu/qs_emu_mpc.cpp over csrc/qs_mpc.h)."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO = os.path.join(_HERE, "libqs_emu_mpc.so")
_lib = None
METHOD = dict(best=0, mppi=1)


def build():
    return _compile(_SO, os.path.join(_HERE, "qs_emu_mpc.cpp"))


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        _lib.qsem_check.argtypes = [i32, i32, i32, i32, C.c_char_p, i32]
        _lib.qsem_check_sigma.argtypes = [f32, C.c_char_p, i32]
        _lib.qsem_check_lambda.argtypes = [f32, C.c_char_p, i32]
        _lib.qsem_exp_nonpos.argtypes = [vp, i32, vp]
        _lib.qsem_exp_nonpos.restype = None
        _lib.qsem_sample.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, vp, vp]
        _lib.qsem_sample.restype = None
        _lib.qsem_feed.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp]
        _lib.qsem_feed.restype = None
        _lib.qsem_finish.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]
        _lib.qsem_finish.restype = None
        _lib.qsem_set_plan.argtypes = [vp, vp, vp, i32, i32, i32]
        _lib.qsem_set_plan.restype = None
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a, shape=-1):
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def check(n_robots, n_candidates, horizon, action_dim):
    """raises ValueError with the reason qs_mpc_create gives for a shape it refuses"""
    err = C.create_string_buffer(512)
    if _load().qsem_check(n_robots, n_candidates, horizon, action_dim, err, 512):
        raise ValueError(err.value.decode())


def check_sigma(sigma):
    err = C.create_string_buffer(512)
    if _load().qsem_check_sigma(float(sigma), err, 512):
        raise ValueError(err.value.decode())


def check_lambda(lam):
    err = C.create_string_buffer(512)
    if _load().qsem_check_lambda(float(lam), err, 512):
        raise ValueError(err.value.decode())


def exp_nonpos(x):
    x = _f(x)
    out = np.empty_like(x)
    _load().qsem_exp_nonpos(_p(x), x.size, _p(out))
    return out


class Planner:
    """the handle's arrays on the host: plan [M, H, d], seq [H, M C, d], score and running [M C], best and best_score [M], actions [N, d],
    active [N]"""

    def __init__(self, M, C_, H, d):
        check(M, C_, H, d)
        self.M, self.C, self.H, self.d, self.N = M, C_, H, d, M * (1 + C_)
        MC = M * C_
        self.plan, self.seq = np.zeros((M, H, d), np.float32), np.zeros((H, MC, d), np.float32)
        self.score, self.running = np.zeros(MC, np.float32), np.zeros(MC, np.uint8)
        self.best, self.best_score = np.zeros(M, np.int32), np.zeros(M, np.float32)
        self.actions, self.active = np.zeros((self.N, d), np.float32), np.ones(self.N, np.uint8)

    def set_plan(self, plan=None, mask=None):
        src = None if plan is None else _f(plan, (self.M, self.H, self.d))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.M)
        _load().qsem_set_plan(_p(self.plan), _p(src), _p(m), self.M, self.H, self.d)

    def sample(self, eps, sigma):
        e = _f(eps, (self.H, self.M * self.C, self.d))
        _load().qsem_sample(_p(self.plan), _p(e), self.M, self.C, self.H, self.d, float(sigma), _p(self.seq), _p(self.score), _p(self.running))

    def feed(self, h, reward=None, done=None, reward_end=None, mask=True):
        """reward float32 [N] and done [N] for h >= 1, reward_end [N, k] at h == H; mask: whether `active` is written"""
        r = None if reward is None else _f(reward, self.N)
        dn = None if done is None else np.ascontiguousarray(done, np.uint8).reshape(self.N)
        re_, stride = None, 0
        if reward_end is not None:
            re_ = np.ascontiguousarray(reward_end, np.float32).reshape(self.N, -1)
            stride = re_.shape[1]
        assert h == 0 or (r is not None and dn is not None)
        assert h < self.H or re_ is not None
        _load().qsem_feed(int(h), _p(self.seq), _p(self.score), _p(self.running), self.M, self.C, self.H, self.d, _p(r), _p(dn), _p(re_), stride,
                          _p(self.actions), _p(self.active) if mask else None)

    def finish(self, method="best", lam=1.0):
        _load().qsem_finish(_p(self.seq), _p(self.score), self.M, self.C, self.H, self.d, METHOD[method], float(lam), _p(self.plan), _p(self.actions),
                            _p(self.best), _p(self.best_score))
