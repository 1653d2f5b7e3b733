"""ctypes driver for the TEST-ONLY emulation of steps with external pushes (tests/emu/qs_emu_push.cpp), on a handle of emu.Emu."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO_PUSH = os.path.join(_HERE, "libqs_emu_push.so")


def build_push():
    """the full and the common-path builds of Env::step with push rows (~60 s of g++ the first time), only on demand"""
    return _compile(_SO_PUSH, os.path.join(_HERE, "qs_emu_push.cpp"))


_lib = None


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_push())
    return _lib


def step_push(emu, actions, push, variant=0):
    """One env step of `emu` (an emu.Emu) with push rows push [N, 8] (force 3, torque 3, remaining substeps, frame), which it counts down
    in place as the kernel does.  variant 0 = the full build, 1 / 2 = k_step's / k_step_dense's common-path build and hand-over.
    Returns obs, rew, done, truncated, resume."""
    n = emu.n
    a = np.ascontiguousarray(actions, np.float32).reshape(n, emu.d)
    assert push.dtype == np.float32 and push.shape == (n, 8) and push.flags.c_contiguous
    obs = np.zeros((n, emu.o), np.float32)
    rew = np.zeros(n, np.float32)
    done = np.zeros(n, np.uint8)
    trunc = np.zeros(n, np.uint8)
    resume = np.zeros(n, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _load().qsep_step(emu.h, p(a), p(push), int(variant), p(obs), p(rew), p(done), p(trunc), p(resume))
    assert rc == 0, rc
    return obs, rew, done.astype(bool), trunc.astype(bool), resume


def push_rows(n, force=(0, 0, 0), torque=(0, 0, 0), substeps=0, frame=2):
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = force
    r[:, 3:6] = torque
    r[:, 6] = substeps
    r[:, 7] = frame
    return r
