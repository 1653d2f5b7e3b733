"""ctypes driver for the TEST-ONLY host emulation of the kernel arithmetic: tests/emu/qs_emu.cpp (the handle, the plain full builds) and
tests/emu/qs_emu_step.cpp (the builds of the step kernels with their hand-over, pushes, the rack)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libqs_emu.so")
_SO_STEP = os.path.join(_HERE, "libqs_emu_step.so")
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


def build_step():
    """every build the step kernels run, with the hand-over (qs_emu_step.cpp): minutes of g++, so only on demand"""
    return _compile(_SO_STEP, os.path.join(_HERE, "qs_emu_step.cpp"))


_step_lib = None


def step_lib():
    global _step_lib
    if _step_lib is None:
        _step_lib = C.CDLL(build_step())
    return _step_lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mask(mask):
    return None if mask is None else np.ascontiguousarray(mask, np.uint8)


class Emu:
    def __init__(self, cfg, rack=None):
        """rack: None = a plain handle; True or an anchor (position 3, quaternion xyzw 4) = a handle with a rack, as qs_create_ex's"""
        self.lib = C.CDLL(build())
        self.lib.qse_create.restype = C.c_void_p
        self.lib.qse_records.restype = C.POINTER(C.c_float)
        self.cfg = cfg
        self.n, self.d, self.o = cfg.n_envs, cfg.action_dim, cfg.obs_dim
        self.h = C.c_void_p(self.lib.qse_create(C.byref(cfg)))
        self.rec_size = self.lib.qse_rec_size()
        if rack is not None:
            self.set_rack_anchor(True, None if rack is True else rack)

    def on_rack(self):
        return bool(self.lib.qse_rack(self.h, -1, None))

    def set_rack_anchor(self, on, anchor=None):
        """the handle runs the RACK builds (on) or the plain ones; anchor None keeps the handle's (at first the reference's, ANCHOR).
        Emu.step / reset / reset_to hold the plain builds only and refuse a rack handle; step_build and the *_rack functions run either."""
        a = None if anchor is None else np.ascontiguousarray(anchor, np.float32)
        assert a is None or a.shape == (7,)
        assert self.lib.qse_rack(self.h, int(bool(on)), _p(a)) >= 0

    def field(self, name):
        return self.lib.qse_field(name.encode())

    def records(self):
        return np.ctypeslib.as_array(self.lib.qse_records(self.h), shape=(self.n, self.rec_size))

    def reset(self, mask=None):
        assert self.lib.qse_reset(self.h, _p(_mask(mask))) == 0
        return self.get_obs()

    def get_obs(self):
        obs = np.zeros((self.n, self.o), np.float32)
        self.lib.qse_get_obs(self.h, _p(obs))
        return obs

    def get_term_obs(self):
        obs = np.zeros((self.n, self.o), np.float32)
        self.lib.qse_get_term_obs(self.h, _p(obs))
        return obs

    def _step(self, call, actions=None):
        """allocates a step's outputs and makes the call: call(actions, obs, rew, done, trunc, resume) -> rc"""
        a = None if actions is None else np.ascontiguousarray(actions, np.float32).reshape(self.n, self.d)
        obs = np.zeros((self.n, self.o), np.float32)
        rew = np.zeros(self.n, np.float32)
        done = np.zeros(self.n, np.uint8)
        trunc = np.zeros(self.n, np.uint8)
        resume = np.zeros(self.n, np.int32)
        rc = call(*[_p(x) for x in (a, obs, rew, done, trunc, resume)])
        assert rc == 0, rc
        return obs, rew, done.astype(bool), trunc.astype(bool), resume

    def step(self, actions):
        return self._step(lambda *p: self.lib.qse_step(self.h, *p[:5]), actions)[:4]

    def step_build(self, actions, variant, push=None, settle_n=0, spawn=False):
        """step() through the builds step kernel `variant` launches (1 = k_step, 2 = k_step_dense, as QS_STEP_VARIANT): the common-path
        build, then the full build from the substep where it handed over; 0 = the full build alone.  push: rows [N, 8] (push_rows), counted
        down in place as the kernel does.  resume: per environment -1 (not handed over) or the substep, with resume_at_boundary() added
        for a hand-over between two substeps."""
        assert push is None or (push.dtype == np.float32 and push.shape == (self.n, 8) and push.flags.c_contiguous)
        return self._step(lambda a, obs, rew, done, trunc, resume: step_lib().qse_step_build(
            self.h, int(variant), a, _p(push), int(settle_n), int(bool(spawn)), obs, rew, done, trunc, resume), actions)

    step_hot = step_build

    def resume_at_boundary(self):
        return int(self.lib.qse_resume_at_boundary())

    def settle_slice(self, settle_n, spawn=False, variant=0):
        """one slice of a reset's settle as a settle lane runs it: `spawn` first draws the next episode's parameters and spawn state;
        variant 0 = the full build, 1 / 2 = the step kernels' builds with their hand-over.  Returns resume as step_build does."""
        assert settle_n > 0
        return self.step_build(None, variant, settle_n=settle_n, spawn=spawn)[4]

    def set_trace(self, env):
        self._trace = np.zeros((self.cfg.action_repeat, 70), np.float32)
        self.lib.qse_set_trace(self.h, int(env), _p(self._trace))
        return self._trace

    def get_state(self):
        s = np.zeros((self.n, 37), np.float32)
        self.lib.qse_get_state(self.h, _p(s))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, np.float32).reshape(self.n, 37)
        self.lib.qse_set_state(self.h, _p(s))

    def phys_step(self, env, tau):
        t = np.ascontiguousarray(tau, np.float32)
        self.lib.qse_phys_step(self.h, env, _p(t))

    def obb_overlap(self, ca, Ra, ha, cb, Rb, hb):
        a = [np.ascontiguousarray(x, np.float32) for x in (ca, Ra, ha, cb, Rb, hb)]
        return bool(self.lib.qse_obb_overlap(*[_p(x) for x in a]))

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
        assert self.lib.qse_reset_to(self.h, _p(_mask(mask)), _p(st)) == 0
        return self.get_obs()

    def set_demo(self, rows):
        r = np.ascontiguousarray(rows, np.float32).reshape(-1, self.d + 38)
        self.lib.qse_set_demo(self.h, _p(r), int(r.shape[0]))

    def set_demo_counter(self, values, mask=None):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values, np.int32), (self.n,)))
        self.lib.qse_set_demo_counter(self.h, _p(_mask(mask)), _p(v))


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


_SO_SUBSTEP = os.path.join(_HERE, "libqs_emu_substep.so")
SUBSTEP_BUILDS = {"full": 0, "hot": 1, "hot_soft": 2}
_substep_lib = None


def build_substep():
    """one substep of every build tests/hip/substep_probe.hip holds (qs_emu_substep.cpp): a library of its own, on demand"""
    return _compile(_SO_SUBSTEP, os.path.join(_HERE, "qs_emu_substep.cpp"))


def substep(cfg, recs, tau, push=None, build="full"):
    """the emulation twin of tests/hip/substep_probe.py's substep(): recs [n, QS_REC], tau [n, 12], push [n, 8] or None -> (records after
    the substep, substep's return value [n]); each environment decides its own give-up"""
    global _substep_lib
    if _substep_lib is None:
        _substep_lib = C.CDLL(build_substep())
    out, tau = np.array(recs, np.float32, order="C"), np.ascontiguousarray(tau, np.float32)
    n = out.shape[0]
    push = None if push is None else np.ascontiguousarray(push, np.float32)
    assert tau.shape == (n, 12) and (push is None or push.shape == (n, 8))
    ret = np.full(n, -1, np.int32)
    rc = _substep_lib.qse_substep(C.byref(cfg), n, SUBSTEP_BUILDS[build], _p(out), _p(tau), _p(push), _p(ret))
    assert rc == 0, rc
    return out, ret


def build_stride(cfg, rack):
    """qs::Build::of(cfg, rack) as launch_step uses it: (rec_stride, step_lds_bytes), and the layout's QS_REC_END, QS_INFO_END"""
    out = [C.c_int() for _ in range(3)]
    stride = C.CDLL(build()).qse_build_stride(C.byref(cfg), int(bool(rack)), *[C.byref(v) for v in out])
    return (stride,) + tuple(v.value for v in out)


class RareCapture:
    """`with RareCapture(max_sets) as cap:` records the inputs of the many-rows solves of one emulation library (qse_rare_capture; `lib`:
    default the plain full builds' of Emu.step, step_lib() for step_build's) while steps run; afterwards cap.rows / env / warm / pay (a
    RACK build: the rack's rows in the payload positions; has_pay False where a solve had none) as rare_solve() takes them"""

    def __init__(self, max_sets=4096, lib=None):
        self.max_sets, self.lib = max_sets, lib

    def __enter__(self):
        self.lib = self.lib or C.CDLL(build())
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


# ---- external pushes (qs_set_external_wrench)
def step_push(emu, actions, push, variant=0):
    return emu.step_build(actions, variant, push=push)


def push_rows(n, force=(0, 0, 0), torque=(0, 0, 0), substeps=0, frame=2):
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = force
    r[:, 3:6] = torque
    r[:, 6] = substeps
    r[:, 7] = frame
    return r


# ---- a handle with a rack (qs_create_ex with qs_rack::on = 1).  Rack and anchor are state of the handle (Emu(cfg, rack=...),
# Emu.set_rack_anchor); resetting or stepping "on the rack" below switches a plain handle over, and `anchor=` sets the handle's anchor
# before the call (None: keeps it).
# INIT_RACK_POSITION, INIT_ORIENTATION of the robot config (go1/configs_go1_*.py): a new handle's anchor
ANCHOR = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], np.float32)


def reset_rack(emu, mask=None, anchor=None):
    """reset on the rack (spawn at the anchor, settle hung) of the masked environments; returns the observations"""
    emu.set_rack_anchor(True, anchor)
    assert step_lib().qse_reset_build(emu.h, _p(_mask(mask)), None) == 0
    return emu.get_obs()


def reset_to_rack(emu, states, mask=None, anchor=None):
    emu.set_rack_anchor(True, anchor)
    s = np.ascontiguousarray(states, np.float32).reshape(emu.n, 37)
    assert step_lib().qse_reset_build(emu.h, _p(_mask(mask)), _p(s)) == 0
    return emu.get_obs()


def set_rack(emu, hung, mask=None):
    assert emu.lib.qse_set_rack(emu.h, _p(_mask(mask)), int(bool(hung))) == 0


def step_rack(emu, actions, variant=0, anchor=None):
    """One env step of `emu` with a rack.  variant 0 = the full build, 1 / 2 = k_step_rack's / k_step_dense_rack's common-path build and
    hand-over.  Returns obs, rew, done, truncated, resume."""
    emu.set_rack_anchor(True, anchor)
    return emu.step_build(actions, variant)


def rack_info(emu, anchor=None):
    """[N, 8]: hung, force 3, torque 3, |base origin - anchor| (QS_INFO_RACK); a query: the handle's builds stay what they are"""
    if anchor is not None:
        emu.set_rack_anchor(emu.on_rack(), anchor)
    out = np.zeros((emu.n, 8), np.float32)
    assert emu.lib.qse_rack_info(emu.h, _p(out)) == 0
    return out


def RackCapture(max_sets=4096):
    """RareCapture of the step kernels' builds (the RACK ones among them)"""
    return RareCapture(max_sets, step_lib())
