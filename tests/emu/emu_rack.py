"""ctypes driver for the TEST-ONLY emulation of a handle with a rack (tests/emu/qs_emu_rack.cpp), on a handle of emu.Emu."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO_RACK = os.path.join(_HERE, "libqs_emu_rack.so")
# INIT_RACK_POSITION, INIT_ORIENTATION of the robot config (go1/configs_go1_*.py)
ANCHOR = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], np.float32)


def build_rack():
    """the RACK builds of Env (~60 s of g++ the first time), only on demand"""
    return _compile(_SO_RACK, os.path.join(_HERE, "qs_emu_rack.cpp"))


_lib = None


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_rack())
    return _lib


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _anchor(anchor):
    a = np.ascontiguousarray(ANCHOR if anchor is None else anchor, np.float32)
    assert a.shape == (7,)
    return a


def _mask(mask):
    return None if mask is None else np.ascontiguousarray(mask, np.uint8)


def reset_rack(emu, mask=None, anchor=None):
    """reset on the rack (spawn at the anchor, settle hung) of the masked environments; returns the observations"""
    a, m = _anchor(anchor), _mask(mask)
    assert _load().qser_reset(emu.h, _p(a), _p(m)) == 0
    return emu.get_obs()


def reset_to_rack(emu, states, mask=None, anchor=None):
    a, m = _anchor(anchor), _mask(mask)
    s = np.ascontiguousarray(states, np.float32)
    assert _load().qser_reset_to(emu.h, _p(a), _p(m), _p(s)) == 0
    return emu.get_obs()


def set_rack(emu, hung, mask=None):
    m = _mask(mask)
    assert _load().qser_set_rack(emu.h, _p(m), int(bool(hung))) == 0


def step_rack(emu, actions, variant=0, anchor=None):
    """One env step of `emu` with a rack.  variant 0 = the full build, 1 / 2 = k_step_rack's / k_step_dense_rack's common-path build and
    hand-over.  Returns obs, rew, done, truncated, resume."""
    n = emu.n
    a = np.ascontiguousarray(actions, np.float32).reshape(n, emu.d)
    obs = np.zeros((n, emu.o), np.float32)
    rew = np.zeros(n, np.float32)
    done = np.zeros(n, np.uint8)
    trunc = np.zeros(n, np.uint8)
    resume = np.zeros(n, np.int32)
    rc = _load().qser_step(emu.h, _p(_anchor(anchor)), _p(a), int(variant), _p(obs), _p(rew), _p(done), _p(trunc), _p(resume))
    assert rc == 0, rc
    return obs, rew, done.astype(bool), trunc.astype(bool), resume


def rack_info(emu, anchor=None):
    """[N, 8]: hung, force 3, torque 3, |base origin - anchor| (QS_INFO_RACK)"""
    out = np.zeros((emu.n, 8), np.float32)
    assert _load().qser_info(emu.h, _p(_anchor(anchor)), _p(out)) == 0
    return out


class RackCapture:
    """`with RackCapture(max_sets) as cap:` records the inputs of the RACK builds' many-rows solves while steps run; afterwards cap.rows /
    env / warm / pay (the rack's rows in the payload positions; has_pay False where a solve had none) as emu.rare_solve() takes them"""

    def __init__(self, max_sets=4096):
        self.max_sets = max_sets

    def __enter__(self):
        self.rec = _load().qser_rare_capture(int(self.max_sets))
        return self

    def __exit__(self, *exc):
        lib = _load()
        n = lib.qser_rare_captured(None)
        buf = np.zeros((n, self.rec), np.float32)
        lib.qser_rare_captured(buf.ctypes.data_as(C.c_void_p))
        lib.qser_rare_capture(0)
        self.rows = buf[:, :768].reshape(n, 4, 12, 16)
        self.env, self.warm = buf[:, 768:770], buf[:, 770:774]
        self.pay, self.has_pay = buf[:, 774:833], buf[:, 833] > 0.5
        return False
