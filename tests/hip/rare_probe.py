"""ctypes driver for the TEST-ONLY probe of the many-rows contact solve on the GPU (tests/hip/rare_probe.hip): RareSolver<LaneDev, CONE>
compiled into a small kernel with the product's hipcc options (quadruped-springs_amd/build.py: hipcc_flags)."""
import ctypes as C
import glob
import importlib.util
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(os.path.dirname(_HERE))
_SRC = os.path.join(_HERE, "rare_probe.hip")
_SO = os.path.join(_HERE, "librare_probe.so")
_BUILD_PY = os.path.join(_REPO, "quadruped-springs_amd", "build.py")

ROW_FLOATS, PAY_FLOATS = 16, 59
CORES = {"default": 0, "0_4": 1, "0_6": 2, "18_12": 3}      # RareSolver::solve<CORE>: 0 picks by shape, the others force core<NAX, NBX>
ERR_SHAPE = -2                                              # a forced <0, 4> / <0, 6> refused a row set it cannot hold


def _deps(src):
    return [src, _BUILD_PY, os.path.join(_REPO, "include", "qs_amd.h")] + \
        sorted(glob.glob(os.path.join(_REPO, "quadruped-springs_amd", "csrc", "*.h")))


def _build_mod():
    spec = importlib.util.spec_from_file_location("qs_build_flags", _BUILD_PY)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_probe(src, so):
    """hipcc --offload-arch=gfx950 with build.py's options: the probe `src` into the library `so`, when a header, the probe or the options
    are newer (cross-compiles without a GPU)"""
    if os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in _deps(src)):
        return so
    b = _build_mod()
    tmp = "%s.%d.tmp" % (so, os.getpid())   # (renamed into place: a concurrent loader never sees half a library)
    cmd = lambda form: [b.hipcc()] + b.hipcc_flags(form) + ["-I" + os.path.join(_REPO, "include"), "-o", tmp, src]
    r = subprocess.run(cmd(os.environ.get("QS_MFMA_VGPR_FORM", "1") != "0"), stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        if "Rewrite AGPR-Copy-MFMA" not in r.stderr:   # (the back-end crash build.py also works round)
            raise subprocess.CalledProcessError(r.returncode, r.args)
        subprocess.check_call(cmd(False))
    os.replace(tmp, so)
    return so


def build():
    """librare_probe.so next to this file"""
    return build_probe(_SRC, _SO)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.qsp_rare_solve.restype = C.c_int
    return _lib


def solve(cfg, rows, env, warm, pay=None, core="default"):
    """One launch, a wave per 16 row sets.  rows [n, 4, 12, 16] (per leg, its twelve Rows), env [n, 2] (mu, mine), warm [n, 4] (the feet's
    warm start), pay [n, 59] or None; n a multiple of 16.  Returns (rc, lam12 [n, 4, 12], plam [n, 6]); rc 0 or a HIP error code, or
    ERR_SHAPE for a forced instantiation that cannot hold one of the row sets."""
    rows, env, warm = (np.ascontiguousarray(x, np.float32) for x in (rows, env, warm))
    n = rows.shape[0]
    assert rows.shape == (n, 4, 12, ROW_FLOATS) and env.shape == (n, 2) and warm.shape == (n, 4) and n % 16 == 0
    pay = None if pay is None else np.ascontiguousarray(pay, np.float32).reshape(n, PAY_FLOATS)
    lam12, plam = np.zeros((n, 4, 12), np.float32), np.zeros((n, 6), np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib().qsp_rare_solve(C.byref(cfg), n, CORES[core], p(rows), p(env), p(warm), p(pay), p(lam12), p(plam))
    return rc, lam12, plam
