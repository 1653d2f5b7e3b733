"""ctypes driver for the TEST-ONLY host build of ARS's bookkeeping (tests/emu/qs_emu_ars.cpp over csrc/qs_ars.h)."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO = os.path.join(_HERE, "libqs_emu_ars.so")
_lib = None


def build():
    return _compile(_SO, os.path.join(_HERE, "qs_emu_ars.cpp"))


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        _lib.qsea_check.argtypes = [i32, i32, i32, i32, C.c_char_p, i32]
        _lib.qsea_perturb.argtypes = [vp, vp, i32, i32, f32, vp]
        _lib.qsea_perturb.restype = None
        _lib.qsea_begin.argtypes = [vp, vp, vp, vp, i32, vp]
        _lib.qsea_begin.restype = None
        _lib.qsea_account.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp]
        _lib.qsea_account.restype = None
        _lib.qsea_returns.argtypes = [vp, vp, i32, i32, f32, vp]
        _lib.qsea_returns.restype = C.c_longlong
        _lib.qsea_select.argtypes = [vp, i32, i32, f32, vp, vp, vp]
        _lib.qsea_select.restype = None
        _lib.qsea_apply.argtypes = [vp, vp, i32, vp, vp, i32, f32]
        _lib.qsea_apply.restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, shape=-1):
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def check(n_envs, n_delta, n_params, episodes_per_env=1):
    """raises ValueError with the reason qs_ars_create gives for a shape it refuses"""
    err = C.create_string_buffer(512)
    if _load().qsea_check(n_envs, n_delta, n_params, episodes_per_env, err, 512):
        raise ValueError(err.value.decode())


def perturb(theta, delta, sigma):
    """-> candidates [2 n_delta, n_params]"""
    d = _f(delta, (len(delta), -1))
    th = _f(theta)
    assert th.size == d.shape[1]
    cand = np.zeros((2 * d.shape[0], d.shape[1]), np.float32)
    _load().qsea_perturb(_p(th), _p(d), d.shape[0], d.shape[1], float(sigma), _p(cand))
    return cand


class Accounts:
    """the per-environment accounts of a rollout: begin() at construction, account(raw, done) per step"""

    def __init__(self, n_envs, episodes_per_env=1):
        self.n, self.epe = int(n_envs), int(episodes_per_env)
        self.ret, self.len, self.episodes = np.empty(self.n, np.float32), np.empty(self.n, np.int32), np.empty(self.n, np.int32)
        self.alive, self._n_alive = np.empty(self.n, np.uint8), np.zeros(1, np.int32)
        _load().qsea_begin(_p(self.ret), _p(self.len), _p(self.episodes), _p(self.alive), self.n, _p(self._n_alive))

    @property
    def n_alive(self):
        return int(self._n_alive[0])

    def account(self, raw_reward, done):
        r, d = _f(raw_reward), np.ascontiguousarray(done, np.uint8).reshape(-1)
        assert r.size == d.size == self.n
        _load().qsea_account(_p(self.ret), _p(self.len), _p(self.episodes), _p(self.alive), _p(r), _p(d), self.n, self.epe, _p(self._n_alive))

    def returns(self, n_delta, alive_bonus_offset=0.0):
        return returns(self.ret, self.len, n_delta, alive_bonus_offset)


def returns(ret, length, n_delta, alive_bonus_offset=0.0):
    """-> (R [2 n_delta] float32, the sum of all lengths)"""
    r, l = _f(ret), np.ascontiguousarray(length, np.int32).reshape(-1)
    assert r.size == l.size and r.size % (2 * n_delta) == 0
    R = np.zeros(2 * n_delta, np.float32)
    steps = _load().qsea_returns(_p(r), _p(l), r.size, int(n_delta), float(alive_bonus_offset), _p(R))
    return R, int(steps)


def select(R, n_top, lr):
    """-> (idx [n_top] int32, w [n_top] float32, std, step)"""
    R = _f(R)
    n_delta = R.size // 2
    assert 1 <= n_top <= n_delta <= 1024
    idx, w, st = np.zeros(n_top, np.int32), np.zeros(n_top, np.float32), np.zeros(2, np.float32)
    _load().qsea_select(_p(R), n_delta, int(n_top), float(lr), _p(idx), _p(w), _p(st))
    return idx, w, st[0], st[1]


def apply(theta, delta, idx, w, step):
    """-> the new theta (a copy)"""
    d = _f(delta, (len(delta), -1))
    th, ix, ww = _f(theta).copy(), np.ascontiguousarray(idx, np.int32), _f(w)
    assert th.size == d.shape[1] and ix.size == ww.size
    _load().qsea_apply(_p(th), _p(d), d.shape[1], _p(ix), _p(ww), ix.size, float(np.float32(step)))
    return th
