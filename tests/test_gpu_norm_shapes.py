"""k_norm_moments / k_norm_finish (csrc/qs_norm.hip) through the C ABI on fabricated arrays against the float64 reference of tests/norm_ref.py
(itself judged against np.longdouble in tests/test_norm_ref_cpu.py): every width on both sides of the 32-column chunk edges up to the
maximum of 255, every size at which the merge of the blocks' moments takes another path, every (training, norm_obs, norm_reward), in place
and through out_*, and masks over more than one block -- block 0 empty, an empty middle block, uncounted pivots, one row, no row, random
rows, and a mask of ones against qs_norm_step bit for bit.  Per case one reset, six training steps and two evaluation steps; every step
is compared on the normalised observations and terminal observations, rewards, raw copies, the six statistics and the per-environment
returns.  The tolerances are those of test_gpu_parity.py::test_vec_normalize_kernels_against_torch_float64 (norm_ref.py); each case prints
its largest ratio to each bound and, where QS_RECORD_DIR names a directory, appends them to its norm_parity.jsonl.

Before the merge pivot was taken from the first block that counted a row (it was block 0's mean, 0 when a mask emptied block 0), the masked
cases missed the variance bound; the figures are in profiles/norm_parity.md."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import norm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BOUNDS = ("outputs", "mean", "var", "ret_moments", "returns")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def record(rec):
    """one line per case into $QS_RECORD_DIR/norm_parity.jsonl (what profiles/norm_parity.json is assembled from); nothing without the variable"""
    out = os.environ.get("QS_RECORD_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "norm_parity.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64, 1: np.uint8}[x.dtype.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Handle:
    """a qs_norm handle on device 0 and the device arrays of its calls"""

    def __init__(self, t, n, o):
        from qs_amd import lib as L
        self.t, self.L, self.lib, self.n, self.o = t, L, L.load(), n, o
        self.h = C.c_void_p()
        L.check(self.lib.qs_norm_create(n, o, R.CLIP_OBS, R.CLIP_REW, R.GAMMA, R.EPS, 0, C.byref(self.h)))

    def dev(self, x):
        return self.t.from_numpy(np.ascontiguousarray(x)).cuda()

    @staticmethod
    def p(x):
        return C.c_void_p(x.data_ptr())

    def stats(self):
        mean, var = np.zeros(self.o), np.zeros(self.o)
        c = [C.c_double() for _ in range(4)]
        self.L.check(self.lib.qs_norm_get_stats(self.h, mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), *[C.byref(x) for x in c]))
        return dict(obs_mean=mean, obs_var=var, obs_count=c[0].value, ret_mean=c[1].value, ret_var=c[2].value, ret_count=c[3].value)

    def set_stats(self, s):
        m, v = np.ascontiguousarray(s["obs_mean"], np.float64), np.ascontiguousarray(s["obs_var"], np.float64)
        self.L.check(self.lib.qs_norm_set_stats(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), float(s["obs_count"]), float(s["ret_mean"]),
                                                float(s["ret_var"]), float(s["ret_count"])))

    def returns(self):
        r = self.t.empty(self.n, dtype=self.t.float64, device="cuda")
        self.L.check(self.lib.qs_norm_get_returns(self.h, self.p(r)))
        self.t.cuda.synchronize()
        return r.cpu().numpy()

    def set_returns(self, r):
        d = self.dev(np.asarray(r, np.float64))
        self.L.check(self.lib.qs_norm_set_returns(self.h, self.p(d)))
        self.t.cuda.synchronize()

    def reset(self, obs, training, norm_obs):
        d = self.dev(obs)
        self.L.check(self.lib.qs_norm_reset(self.h, self.p(d), int(training), int(norm_obs)))
        return dict(obs=d.cpu().numpy())

    def step(self, s, training, norm_obs, norm_reward, through_out=False):
        """one step on copies of s's arrays -> what the device left: obs, rew, term, raw_obs, raw_rew.  through_out: qs_norm_step_io with out_obs /
        out_rew / out_done (the inputs must stay raw, the flags are copied); an active mask: qs_norm_step_masked; else qs_norm_step."""
        t, p = self.t, self.p
        obs, rew, term, done = self.dev(s["obs"]), self.dev(s["rew"]), self.dev(s["term"]), self.dev(s["done"])
        raw_obs, raw_rew = t.full_like(obs, 7.0), t.full_like(rew, 7.0)
        if s["active"] is not None:
            act = self.dev(s["active"])
            self.L.check(self.lib.qs_norm_step_masked(self.h, p(obs), p(rew), p(done), p(act), p(term), int(training), int(norm_obs), int(norm_reward),
                                                      p(raw_obs), p(raw_rew)))
            out_obs, out_rew = obs, rew
        elif through_out:
            out_obs, out_rew, out_done = t.full_like(obs, 9.0), t.full_like(rew, 9.0), t.full_like(done, 9)
            v = lambda x: x.data_ptr()
            io = self.L.NormIO(obs=v(obs), rew=v(rew), done=v(done), term_obs=v(term), raw_obs=v(raw_obs), raw_rew=v(raw_rew), out_obs=v(out_obs), out_rew=v(out_rew),
                               out_done=v(out_done))
            self.L.check(self.lib.qs_norm_step_io(self.h, C.byref(io), int(training), int(norm_obs), int(norm_reward)))
            assert same_bits(obs.cpu().numpy(), s["obs"]) and same_bits(rew.cpu().numpy(), s["rew"]), "qs_norm_step_io with out_*: the inputs did not stay raw"
            assert np.array_equal(out_done.cpu().numpy(), s["done"])
        else:
            self.L.check(self.lib.qs_norm_step(self.h, p(obs), p(rew), p(done), p(term), int(training), int(norm_obs), int(norm_reward), p(raw_obs), p(raw_rew)))
            out_obs, out_rew = obs, rew
        assert np.array_equal(done.cpu().numpy(), s["done"])
        return dict(obs=out_obs.cpu().numpy(), rew=out_rew.cpu().numpy(), term=term.cpu().numpy(), raw_obs=raw_obs.cpu().numpy(), raw_rew=raw_rew.cpu().numpy())

    def close(self):
        self.lib.qs_norm_destroy(self.h)
        self.h = None


class Ratios:
    """|device - reference| / bound per bound of norm_ref.py: the largest of every step (step -1: the reset), and of the case with the step it
    came from.  Where a bound is zero -- the variance of a constant column has only a relative bound -- the device must give the reference's
    value itself; what does not is counted in `exact_misses`."""

    def __init__(self):
        self.worst = {k: (0.0, None) for k in BOUNDS}
        self.by_step = {k: {} for k in BOUNDS}
        self.exact_misses = 0

    def add(self, name, k, diff, bound):
        diff, bound = np.atleast_1d(np.asarray(diff, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
        self.exact_misses += int(((bound <= 0) & (diff != 0)).sum())
        r = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), 0.0)
        r = float(np.max(r)) if r.size else 0.0
        if not r <= self.by_step[name].get(k, 0.0):
            self.by_step[name][k] = r
        if not r <= self.worst[name][0]:
            self.worst[name] = (r, k)

    def outputs(self, k, got, exp):
        for key in ("obs", "term", "rew"):
            if exp.get(key) is not None:
                e = np.asarray(exp[key], np.float64)
                assert np.isfinite(got[key]).all(), (k, key)
                self.add("outputs", k, np.abs(got[key] - e), R.OUT_TOL + R.OUT_TOL * np.abs(e))

    def stats(self, k, s, r):
        self.add("mean", k, np.abs(s["obs_mean"] - r["obs_mean"]), R.MEAN_REL * np.abs(r["obs_mean"]) + R.MEAN_STD * np.sqrt(r["obs_var"]))
        self.add("var", k, np.abs(s["obs_var"] - r["obs_var"]), R.VAR_RTOL * np.abs(r["obs_var"]))
        for key in ("ret_mean", "ret_var"):
            self.add("ret_moments", k, abs(s[key] - r[key]), R.MOM_RTOL * abs(r[key]) + R.MOM_ATOL)
        assert s["obs_count"] == r["obs_count"] and s["ret_count"] == r["ret_count"], (k, s["obs_count"], r["obs_count"], s["ret_count"], r["ret_count"])

    def returns(self, k, got, ref):
        self.add("returns", k, np.abs(got - ref), R.MOM_RTOL * np.abs(ref) + R.MOM_ATOL)

    def report(self, **case):
        rec = dict(case, **{name + "_ratio_to_bound": self.worst[name][0] for name in BOUNDS}, **{name + "_worst_step": self.worst[name][1] for name in BOUNDS},
                   exact_misses=self.exact_misses, var_ratio_by_step={str(k): v for k, v in sorted(self.by_step["var"].items())})
        print("norm parity:", json.dumps(rec))
        record(rec)
        assert self.exact_misses == 0, rec
        for name in BOUNDS:
            assert self.worst[name][0] <= 1.0, rec


def run_case(t, n, o, flags=(1, 1, 1), masked=False):
    training, norm_obs, norm_reward = flags
    dev, ratios = Handle(t, n, o), Ratios()
    state = {}

    def on_step(k, ref, s, exp):
        if k < 0:     # the reset, on RunningMeanStd's prior; then the settled statistics and the returns of the case, read back bit for bit
            got = dev.reset(s["obs"], training, norm_obs)
            assert not dev.returns().any()
            if not norm_obs:
                assert same_bits(got["obs"], s["obs"])
            ratios.outputs(k, got, exp)
            ratios.stats(k, dev.stats(), ref.stats())
            mean, var, rm, rv = R.settled(o, (n, o) == R.OFFSET_REWARDS)
            want = dict(obs_mean=mean, obs_var=var, obs_count=float(n), ret_mean=rm, ret_var=rv, ret_count=float(n))
            dev.set_stats(want)
            dev.set_returns(R.initial_returns(n, o))
            have = dev.stats()
            assert all(same_bits(np.asarray(have[key], np.float64), np.asarray(want[key], np.float64)) for key in want)
            assert same_bits(dev.returns(), R.initial_returns(n, o))
            state.update(stats=have, returns=dev.returns())
            return
        train = s["training"] and training
        name = R.MASKS[k] if s["active"] is not None else None
        if name == "ones":     # a second handle in the same state, fed the same arrays through qs_norm_step
            twin = Handle(t, n, o)
            twin.set_stats(state["stats"]); twin.set_returns(state["returns"])
            unmasked = dict(s, active=None)
            want = twin.step(unmasked, train, norm_obs, norm_reward)
        got = dev.step(s, train, norm_obs, norm_reward, through_out=k % 2 == 1)
        stats, returns = dev.stats(), dev.returns()
        assert same_bits(got["raw_obs"], s["obs"]) and same_bits(got["raw_rew"], s["rew"]), f"step {k}: raw copies"
        if not norm_obs:
            assert same_bits(got["obs"], s["obs"]) and same_bits(got["term"], s["term"]), f"step {k}: norm_obs = 0 changed the observations"
            assert same_bits(stats["obs_mean"], state["stats"]["obs_mean"]) and same_bits(stats["obs_var"], state["stats"]["obs_var"]), f"step {k}"
            assert stats["obs_count"] == state["stats"]["obs_count"] == float(n), f"step {k}: norm_obs = 0 moved the observations' count"
        if not norm_reward:
            assert same_bits(got["rew"], s["rew"]), f"step {k}: norm_reward = 0 changed the rewards"
        if train:
            assert stats["ret_count"] == state["stats"]["ret_count"] + (n if s["active"] is None else int(s["active"].sum()))
            if s["active"] is None or s["active"].any():
                assert stats["ret_mean"] != state["stats"]["ret_mean"] and stats["ret_var"] != state["stats"]["ret_var"], f"step {k}: the returns' statistics stood still"
        else:
            assert all(same_bits(np.asarray(stats[key]), np.asarray(state["stats"][key])) for key in stats), f"step {k}: an evaluation step moved the statistics"
        if s["active"] is not None:
            off = s["active"] == 0
            assert same_bits(returns[off], state["returns"][off]), f"step {k} ({name}): the return of an uncounted row advanced or was cleared"
            if name == "none":
                assert all(same_bits(np.asarray(stats[key]), np.asarray(state["stats"][key])) for key in stats), "a step without a counted row moved the statistics"
                assert same_bits(returns, state["returns"])
            if name == "ones":
                for key in got:
                    assert same_bits(got[key], want[key]), f"mask of ones against qs_norm_step: {key}"
                ts = twin.stats()
                assert all(same_bits(np.asarray(stats[key]), np.asarray(ts[key])) for key in stats), "mask of ones against qs_norm_step: statistics"
                assert same_bits(returns, twin.returns())
                twin.close()
        ratios.outputs(k, got, exp)
        ratios.stats(k, stats, ref.stats())
        ratios.returns(k, returns, ref.returns)
        state.update(stats=stats, returns=returns)

    R.run_reference(n, o, flags=flags, masked=masked, on_step=on_step)
    dev.close()
    return ratios


@pytest.mark.parametrize("n, o", R.SHAPES)
def test_shapes(torch_cuda, n, o):
    rows, parts = R.layout(n)
    run_case(torch_cuda, n, o).report(test="shapes", n=n, o=o, rows_per_block=rows, n_parts=parts, chunks=(o + 32) // 32)


@pytest.mark.parametrize("flags", R.FLAGS, ids=lambda f: "training%d-norm_obs%d-norm_reward%d" % f)
@pytest.mark.parametrize("n, o", R.FLAG_SHAPES)
def test_flags(torch_cuda, n, o, flags):
    run_case(torch_cuda, n, o, flags=flags).report(test="flags", n=n, o=o, training=flags[0], norm_obs=flags[1], norm_reward=flags[2])


@pytest.mark.parametrize("n, o", R.MASK_SHAPES)
def test_masks(torch_cuda, n, o):
    """MASKS of norm_ref.py, one per training step.  The worst step of each bound is printed with the ratio: steps 0 .. 5 are the masks in
    their order."""
    rows, parts = R.layout(n)
    run_case(torch_cuda, n, o, masked=True).report(test="masks", n=n, o=o, rows_per_block=rows, n_parts=parts, masks=list(R.MASKS))


@pytest.mark.parametrize("n, o, out, word", [(64, 0, True, "obs_dim 0"), (64, 256, True, "obs_dim 256"), (0, 33, True, "n_envs 0"), (64, 33, False, "bad argument")])
def test_create_refuses(torch_cuda, n, o, out, word):
    from qs_amd import lib as L
    lib = L.load()
    h = C.c_void_p()
    rc = lib.qs_norm_create(n, o, R.CLIP_OBS, R.CLIP_REW, R.GAMMA, R.EPS, 0, C.byref(h) if out else None)
    assert rc != 0 and not h.value
    reason = lib.qs_last_error().decode()
    assert "bad argument" in reason and word in reason, reason


def test_contact_bundle_environment(torch_cuda):
    """DeviceVecNormalize(training=True) over PPO_BASIC_CONTACT (32 columns: the returns column alone in the second chunk), n = 100 (two
    blocks): 20 steps of step_tensor against VecNormalizeRef with float64 moments at the bounds of test_gpu_parity.py::test_device_vec_normalize,
    then 5 steps with rows [0, 64) -- all of block 0 -- frozen against MaskedVecNormalizeRef."""
    t = torch_cuda
    from active_ref import MaskedVecNormalizeRef
    from qs_amd import DeviceVecNormalize
    from test_gpu_round2 import vec_env
    n = 100
    env = DeviceVecNormalize(vec_env(n, task_env="JUMPING_FORWARD", observation_space_mode="PPO_BASIC_CONTACT", action_space_mode="DEFAULT",
                                     env_randomizer_mode="GROUND_RANDOMIZER", auto_reset=True, reset_lookahead=2, seed=5), training=True)
    assert env.obs_dim == 32
    ref = MaskedVecNormalizeRef(n, env.obs_dim, training=True)     # (moments_dtype = np.float64; without a mask it is VecNormalizeRef.step)
    A = lambda x: x.cpu().numpy().copy()
    obs = env.reset_tensor()
    np.testing.assert_allclose(A(obs), ref.reset(A(env.old_obs)), atol=2e-5)
    rng = np.random.default_rng(9)
    frozen = np.zeros(n, bool); frozen[:64] = True
    term = t.zeros((n, env.obs_dim), dtype=t.float32, device=env.device)
    n_done = 0
    for k in range(25):
        on = None if k < 20 else ~frozen
        act = t.as_tensor(rng.uniform(-1, 1, size=(n, env.action_dim)).astype(np.float32), device=env.device)
        obs, rew, done, _ = env.step_tensor(act, terminal_obs=term, active=None if on is None else t.as_tensor(on, device=env.device))
        term_raw = A(env.venv.get_info("terminal_obs"))
        o_ref, r_ref, t_ref = ref.step(A(env.old_obs), A(env.old_reward).astype(np.float64), A(done), term_raw, active=on)
        np.testing.assert_allclose(A(obs), o_ref, atol=2e-5, err_msg=f"obs step {k}")
        np.testing.assert_allclose(A(rew), r_ref, atol=2e-5, rtol=1e-5, err_msg=f"reward step {k}")
        ended = A(done).astype(bool)
        np.testing.assert_allclose(A(term)[ended], t_ref[ended], atol=2e-5, err_msg=f"terminal observations step {k}")
        s, r = env.get_stats(), ref.stats()
        np.testing.assert_allclose(s["obs_mean"], r["obs_mean"], rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
        np.testing.assert_allclose(s["obs_var"], r["obs_var"], rtol=1e-5, err_msg=f"step {k}")
        np.testing.assert_allclose([s["obs_count"], s["ret_mean"], s["ret_var"], s["ret_count"]], [r["obs_count"], r["ret_mean"], r["ret_var"], r["ret_count"]],
                                   rtol=1e-5, err_msg=f"step {k}")
        assert s["obs_count"] == r["obs_count"] and s["ret_count"] == r["ret_count"]
        np.testing.assert_allclose(A(env._returns()), ref.returns, rtol=1e-5, atol=1e-7, err_msg=f"returns step {k}")
        n_done += int(ended.sum())
    assert abs(s["obs_count"] - (1e-4 + 21 * n + 5 * 36)) < 1e-6
    print("contact bundle: episodes ended", n_done)
    env.close()
