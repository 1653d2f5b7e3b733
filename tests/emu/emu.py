"""ctypes driver for the TEST-ONLY host emulation of the kernel arithmetic (tests/emu/qs_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libqs_emu.so")
_SO_HOT = os.path.join(_HERE, "libqs_emu_hot.so")
import glob
# every header under csrc/ counts (round 4's hand-kept list lacked qs_rare.h: an edit of the many-rows solver left a stale emulation behind)
_HDR = sorted(glob.glob(os.path.join(_REPO, "quadruped-springs_amd", "csrc", "*.h"))) + \
       [os.path.join(_REPO, "include", "qs_amd.h"), os.path.join(_HERE, "qs_emu.h")]
_SRC = [os.path.join(_HERE, "qs_emu.cpp")] + _HDR


def _compile(so, src):
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in [src] + _HDR):
        tmp = "%s.%d.tmp" % (so, os.getpid())   # (renamed into place: a concurrent loader never sees half a library)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off",
                               "-I" + os.path.join(_REPO, "include"), "-o", tmp, src])
        os.replace(tmp, so)
    return so


def build():
    return _compile(_SO, _SRC[0])


def build_hot():
    """the step kernels' common-path builds and their hand-over (qs_emu_hot.cpp): ~50 s of g++, so only on demand"""
    return _compile(_SO_HOT, os.path.join(_HERE, "qs_emu_hot.cpp"))


class Emu:
    def __init__(self, cfg):
        self.lib = C.CDLL(build())
        self.lib.qse_create.restype = C.c_void_p
        self.lib.qse_records.restype = C.POINTER(C.c_float)
        self.cfg = cfg
        self.n, self.d, self.o = cfg.n_envs, cfg.action_dim, cfg.obs_dim
        self.h = C.c_void_p(self.lib.qse_create(C.byref(cfg)))
        self.rec_size = self.lib.qse_rec_size()

    def _p(self, a):
        return a.ctypes.data_as(C.c_void_p)

    def field(self, name):
        return self.lib.qse_field(name.encode())

    def records(self):
        return np.ctypeslib.as_array(self.lib.qse_records(self.h), shape=(self.n, self.rec_size))

    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.lib.qse_reset(self.h, None if m is None else self._p(m))
        return self.get_obs()

    def get_obs(self):
        obs = np.zeros((self.n, self.o), np.float32)
        self.lib.qse_get_obs(self.h, self._p(obs))
        return obs

    def get_term_obs(self):
        obs = np.zeros((self.n, self.o), np.float32)
        self.lib.qse_get_term_obs(self.h, self._p(obs))
        return obs

    def step(self, actions):
        a = np.ascontiguousarray(actions, np.float32).reshape(self.n, self.d)
        obs = np.zeros((self.n, self.o), np.float32)
        rew = np.zeros(self.n, np.float32)
        done = np.zeros(self.n, np.uint8)
        trunc = np.zeros(self.n, np.uint8)
        self.lib.qse_step(self.h, self._p(a), self._p(obs), self._p(rew), self._p(done), self._p(trunc))
        return obs, rew, done.astype(bool), trunc.astype(bool)

    def _hot(self):
        if getattr(self, "_hot_lib", None) is None:
            self._hot_lib = C.CDLL(build_hot())
        return self._hot_lib

    def step_hot(self, actions, variant):
        """step() through the builds step kernel `variant` launches (1 = k_step, 2 = k_step_dense, as QS_STEP_VARIANT): the common-path
        build, then the full build from the substep where it handed over.  resume: per environment -1 (not handed over) or the substep,
        with resume_at_boundary() added for a hand-over between two substeps."""
        a = np.ascontiguousarray(actions, np.float32).reshape(self.n, self.d)
        obs = np.zeros((self.n, self.o), np.float32)
        rew = np.zeros(self.n, np.float32)
        done = np.zeros(self.n, np.uint8)
        trunc = np.zeros(self.n, np.uint8)
        resume = np.zeros(self.n, np.int32)
        rc = self._hot().qse_step_hot(self.h, self._p(a), self._p(obs), self._p(rew), self._p(done), self._p(trunc), int(variant), self._p(resume))
        assert rc == 0, rc
        return obs, rew, done.astype(bool), trunc.astype(bool), resume

    def resume_at_boundary(self):
        return int(self._hot().qse_resume_at_boundary())

    def settle_slice(self, settle_n, spawn=False, variant=0):
        """one slice of a reset's settle as a settle lane runs it: `spawn` first draws the next episode's parameters and spawn state;
        variant 0 = the full build, 1 / 2 = the step kernels' builds with their hand-over.  Returns resume as step_hot does."""
        resume = np.zeros(self.n, np.int32)
        rc = self._hot().qse_settle_slice(self.h, int(settle_n), int(bool(spawn)), int(variant), self._p(resume))
        assert rc == 0, rc
        return resume

    def set_trace(self, env):
        self._trace = np.zeros((self.cfg.action_repeat, 70), np.float32)
        self.lib.qse_set_trace(self.h, int(env), self._p(self._trace))
        return self._trace

    def get_state(self):
        s = np.zeros((self.n, 37), np.float32)
        self.lib.qse_get_state(self.h, self._p(s))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, np.float32).reshape(self.n, 37)
        self.lib.qse_set_state(self.h, self._p(s))

    def phys_step(self, env, tau):
        t = np.ascontiguousarray(tau, np.float32)
        self.lib.qse_phys_step(self.h, env, self._p(t))

    def obb_overlap(self, ca, Ra, ha, cb, Rb, hb):
        a = [np.ascontiguousarray(x, np.float32) for x in (ca, Ra, ha, cb, Rb, hb)]
        return bool(self.lib.qse_obb_overlap(*[self._p(x) for x in a]))

    def get(self, name, dim):
        f = self.field(name)
        return self.records()[:, f:f + dim].copy()

    def block(self):
        """the payload block as its own body (payload="soft"): rows as in Oracle.block()"""
        return self.get("R_BLOCK", 20)

    def set_mu(self, mu):
        self.records()[:, self.field("R_PARAMS")] = mu

    def reset_to(self, states, mask=None):
        st = np.ascontiguousarray(states, np.float32).reshape(self.n, 37)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.lib.qse_reset_to(self.h, None if m is None else self._p(m), self._p(st))
        return self.get_obs()

    def set_demo(self, rows):
        r = np.ascontiguousarray(rows, np.float32).reshape(-1, self.d + 38)
        self.lib.qse_set_demo(self.h, self._p(r), int(r.shape[0]))

    def set_demo_counter(self, values, mask=None):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values, np.int32), (self.n,)))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.lib.qse_set_demo_counter(self.h, None if m is None else self._p(m), self._p(v))


def rare_solve(cfg, rows, env, warm, pay=None):
    """the emulation twin of the many-rows solve (RareSolver<LaneEmu, cfg.friction_cone>, qs_rare.h) on row sets in the layout of
    tests/hip/probe.py: rows [n, 4, 12, 16], env [n, 2] (mu, mine), warm [n, 4], pay [n, 59] or None -> lam12 [n, 4, 12], plam [n, 6]"""
    lib = C.CDLL(build())
    rows, env, warm = (np.ascontiguousarray(x, np.float32) for x in (rows, env, warm))
    n = rows.shape[0]
    assert rows.shape == (n, 4, 12, 16) and env.shape == (n, 2) and warm.shape == (n, 4)
    pay = None if pay is None else np.ascontiguousarray(pay, np.float32).reshape(n, 59)
    lam12, plam = np.zeros((n, 4, 12), np.float32), np.zeros((n, 6), np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.qse_rare_solve(C.byref(cfg), n, p(rows), p(env), p(warm), p(pay), p(lam12), p(plam))
    assert rc == 0, rc
    return lam12, plam


class RareCapture:
    """`with RareCapture(max_sets) as cap:` records the inputs of the emulation's many-rows solves (qse_rare_capture) while steps run;
    afterwards cap.rows / env / warm / pay (None where a solve had no payload rows) as rare_solve() takes them"""

    def __init__(self, max_sets=4096):
        self.max_sets = max_sets

    def __enter__(self):
        self.lib = C.CDLL(build())
        self.rec = self.lib.qse_rare_capture(int(self.max_sets))
        return self

    def __exit__(self, *exc):
        n = self.lib.qse_rare_captured(None)
        buf = np.zeros((n, self.rec), np.float32)
        self.lib.qse_rare_captured(buf.ctypes.data_as(C.c_void_p))
        self.lib.qse_rare_capture(0)
        self.rows = buf[:, :768].reshape(n, 4, 12, 16)
        self.env, self.warm = buf[:, 768:770], buf[:, 770:774]
        self.pay, self.has_pay = buf[:, 774:833], buf[:, 833] > 0.5
        return False
