"""ctypes driver for the TEST-ONLY probe of ONE physics substep on the GPU (tests/hip/substep_probe.hip): Sim<LaneDev, CONE, HOT, SOFT>::substep
between Env::load_state / load_par and Env::store_state, compiled into a small kernel with the product's hipcc options
(quadruped-springs_amd/build.py: hipcc_flags).

This is the substep's SOURCE in a small kernel, not the code inlined into k_step / k_step_dense: what the register allocator makes of it
there is not what runs here.  The end-to-end parity tests (tests/test_gpu_parity.py, test_gpu_round2.py) and tools/gate.sh stay the check
for the step kernels' own machine code."""
import ctypes as C
import os

import numpy as np

from rare_probe import build_probe

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "substep_probe.hip")
_SO = os.path.join(_HERE, "libsubstep_probe.so")

PUSH_FLOATS = 8
BUILDS = {"full": 0, "hot": 1, "hot_soft": 2}   # Sim<.., HOT = false>; the common-path build; the common-path build with the payload block's rows
ERR_ARGS = -1


def build():
    """libsubstep_probe.so next to this file (rare_probe.build_probe: on first use, and again when a header, the probe or the options change)"""
    return build_probe(_SRC, _SO)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.qsp_substep.restype = C.c_int
    return _lib


def rec_floats():
    return int(lib().qsp_substep_rec_floats())


def substep(cfg, recs, tau, push=None, build="full"):
    """One launch, a wave per 16 records.  recs [n, QS_REC], tau [n, 12], push [n, 8] or None; n a multiple of 16; the friction model is
    cfg.friction_cone's.  Returns (rc, records after the substep [n, QS_REC], substep's return value [n], counters [32]); rc 0, a HIP error
    code, or ERR_ARGS for a shape or a build the probe does not hold (the outputs then stay NaN / -1)."""
    recs, tau = np.ascontiguousarray(recs, np.float32), np.ascontiguousarray(tau, np.float32)
    n = recs.shape[0]
    push = None if push is None else np.ascontiguousarray(push, np.float32)
    out, ret = np.full(recs.shape, np.nan, np.float32), np.full(n, -1, np.int32)
    counters = np.zeros(int(lib().qsp_substep_counters()), np.uint64)
    if recs.ndim != 2 or recs.shape[1] != rec_floats() or tau.shape != (n, 12) or (push is not None and push.shape != (n, PUSH_FLOATS)):
        return ERR_ARGS, out, ret, counters
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib().qsp_substep(C.byref(cfg), n, BUILDS[build], p(recs), p(tau), p(push), p(out), p(ret), p(counters))
    return rc, out, ret, counters
