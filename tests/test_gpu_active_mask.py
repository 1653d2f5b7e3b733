"""step_tensor(active=) (qs_step_masked): a frozen environment is stepped by nobody -- its whole record, its push and its last
observation stay what they are --, every active environment gets the bits it gets without a mask, a frozen robot on the floor puts no
wave on a rare path, and a thawed environment goes on as if the frozen steps had not been.  DeviceVecNormalize and DeviceARS on top."""
import numpy as np
import pytest

from test_gpu_round2 import RAW, fallen_states, vec_env

pytestmark = pytest.mark.gpu

NAMES = ("state", "obs", "reward", "done", "truncated", "foot_force")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def A(x):
    return x.cpu().numpy().copy()


def fallen_half(v, seed, lo=0.16, hi=0.3):
    """the handle's reset state with every other robot thrown on the floor, just above it (tests/test_gpu_solo_waves.py)"""
    rng = np.random.default_rng(seed)
    s = A(v.get_state())
    lying = np.arange(len(s)) % 2 == 1
    s[lying] = fallen_states(s[lying], rng)
    s[lying, 2] = rng.uniform(lo, hi, size=lying.sum())
    return s.astype(np.float32)


def outputs(v, out):
    obs, rew, done, trunc = out
    return A(v.get_state()), A(obs), A(rew), A(done), A(trunc), A(v.get_info("foot_force"))


def same(a, b, rows, what):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x[rows], y[rows]), f"{what}: {name}"


def twins_under_a_mask(t, n, active, steps, seed, pushes=(), release=None, **kw):
    """Handles A (no mask) and B (`active`, a bool [n]) from one state, half the robots on the floor, under the same random torques: B's active
    environments give A's bits at every step; B's frozen ones keep their whole snapshot row (record, push, last and terminal observation),
    return their last observation, reward 0 and no flag.  pushes: frozen environments with a push pending."""
    a, b = vec_env(n, **kw), vec_env(n, **kw)
    a.reset(); b.reset()
    if release is not None:
        a.set_rack(False, indices=release); b.set_rack(False, indices=release)
    s = fallen_half(a, seed)
    a.set_state(s); b.set_state(s)
    rng = np.random.default_rng(seed + 1)
    on = np.asarray(active, bool)
    frozen = np.nonzero(~on)[0]
    mask = t.as_tensor(on, device=b.device)
    for v in (a, b):     # (both: the active environments of a wave with a pushed mate must not notice either)
        for e in pushes:
            v.apply_external_force([30.0, -20.0, 10.0], torque=[1.0, 2.0, -1.0], substeps=25, indices=[int(e)])
    for e in pushes:
        assert not on[e]
    before = A(b.snapshot().rows)
    push0 = A(b.get_info("external_wrench"))
    last = A(b._obs)[frozen]     # (the handle's last observation: the reset's -- set_state leaves it)
    for k in range(steps):
        tau = t.as_tensor(rng.uniform(-4, 4, size=(n, 12)).astype(np.float32), device=a.device)
        xa = outputs(a, a.step_tensor(tau))
        xb = outputs(b, b.step_tensor(tau, active=mask if k % 2 else mask.to(t.uint8)))     # (bool and uint8 masks alike)
        same(xa, xb, on, f"step {k}, active environments")
        assert np.array_equal(xb[1][frozen], last), f"step {k}: a frozen environment's row of obs is not its last observation"
        assert not xb[2][frozen].any() and not xb[3][frozen].any() and not xb[4][frozen].any(), f"step {k}: reward / done / truncated of a frozen environment"
    after = A(b.snapshot().rows)
    assert np.array_equal(before[frozen].view(np.int32), after[frozen].view(np.int32)), "a frozen environment's snapshot row changed"
    assert not np.array_equal(before[on], after[on])
    push1 = A(b.get_info("external_wrench"))
    assert np.array_equal(push0[frozen], push1[frozen])
    for e in pushes:
        assert push1[e, 6] == 25.0, "a frozen environment's push counted down"
    return a, b


def mask40():
    on = np.ones(40, bool)
    on[16:32] = False              # all of wave 1
    on[0:16:3] = False             # every third environment of wave 0
    on[[33, 39]] = False           # two of the tail's eight
    return on


@pytest.mark.parametrize("step_kernel", ["1", "2"], ids=["k_step", "k_step_dense"])
@pytest.mark.parametrize("solo", [dict(solo_waves=0), dict(solo_waves=32, solo_reach=1e3)], ids=["home", "solo"])
def test_active_do_not_notice_and_frozen_do_not_move(torch_cuda, monkeypatch, step_kernel, solo):
    """1. and 2.: N = 40 (two full waves, a tail of 8), the whole of wave 1, every third of wave 0 and two of the tail frozen for 40 steps,
    half the robots on the floor; pushes pending on a frozen environment of a mixed wave and on one of the all-frozen wave."""
    monkeypatch.setenv("QS_STEP_VARIANT", step_kernel)
    a, b = twins_under_a_mask(torch_cuda, 40, mask40(), 40, 51, pushes=(3, 20), reset_lookahead=2, **solo, **RAW)
    assert a.counter("limit_path_substeps") > 100
    if solo["solo_waves"] and step_kernel == "1":
        assert a.counter("solo_path_substeps") > 0 and b.counter("solo_path_substeps") > 0
    a.close(); b.close()


def test_the_last_observation_is_returned(torch_cuda):
    """2., the observation row: a frozen environment's row of obs is its row of the step before, bit for bit"""
    t = torch_cuda
    n = 20
    v = vec_env(n, auto_reset=True, reset_lookahead=2, noise=True)
    v.reset_tensor()
    gen = t.Generator(device=v.device).manual_seed(1)
    for _ in range(3):
        prev = A(v.step_tensor(t.rand((n, v.action_dim), generator=gen, device=v.device) * 2 - 1)[0])
    on = np.arange(n) % 2 == 0
    obs = A(v.step_tensor(t.rand((n, v.action_dim), generator=gen, device=v.device) * 2 - 1, active=t.as_tensor(on, device=v.device))[0])
    assert np.array_equal(obs[~on], prev[~on]) and not np.array_equal(obs[on], prev[on])
    v.close()


def test_thaw(torch_cuda):
    """3. N = 17, noise and the ground randomizer on, auto-reset with look-ahead states, everybody flagged for a solo wave in every step
    (solo_reach = 1e3).  S is frozen for steps 10..24; from step 25 on its environments give what the unmasked twin gave 15 steps earlier
    under the same actions, resets and terminal observations included; a push set while frozen starts to count at the thaw.  S is taken
    from the twin's run, which comes first: environments whose episode ends after the step the thaw corresponds to."""
    t = torch_cuda
    n, T, lo, hi = 17, 240, 10, 25
    lag = hi - lo
    kw = dict(env_randomizer_mode="GROUND_RANDOMIZER", auto_reset=True, reset_lookahead=4, seed=3, body_contacts=True, noise=True, solo_waves=32,
              solo_reach=1e3)
    a, b = vec_env(n, **kw), vec_env(n, **kw)
    a.reset_tensor(); b.reset_tensor()
    gen = t.Generator(device=a.device).manual_seed(7)
    acts = t.rand((T, n, a.action_dim), generator=gen, device=a.device) * 2 - 1
    names = ("obs", "reward", "done", "truncated", "terminal_obs")
    push = dict(force=[40.0, 25.0, 0.0], substeps=3 * a.cfg.action_repeat, indices=[5])
    pushed = 5

    def record(v, out):
        return [A(x) for x in out] + [A(v.get_info("terminal_obs"))]

    ra = []
    for k in range(T):
        if k == lo:
            a.apply_external_force(**push)              # the twin: at the step the thaw corresponds to
        ra.append(record(a, a.step_tensor(acts[k])))
    ends = np.stack([r[2] for r in ra[lo + 3:T - lag]]).any(0)
    ends[pushed] = False
    assert ends.any(), "no episode of the twin ends after step 12: the run shows nothing about resets after the thaw"
    S = np.concatenate([[pushed], np.nonzero(ends)[0][:4]])
    in_s = np.zeros(n, bool); in_s[S] = True
    done_after_thaw = 0
    for k in range(T):
        frozen_now = lo <= k < hi
        if k == lo + 7:
            b.apply_external_force(**push)              # while frozen
        act = acts[k].clone()
        if k >= hi:
            act[S] = acts[k - lag][S]
        mask = t.as_tensor(~in_s, device=b.device) if frozen_now else None
        rb = record(b, b.step_tensor(act, active=mask))
        for name, x, y in zip(names, ra[k], rb):
            assert np.array_equal(x[~in_s], y[~in_s]), f"step {k}: {name} of the environments that were never frozen"
        if k < lo:
            for name, x, y in zip(names, ra[k], rb):
                assert np.array_equal(x[S], y[S]), f"step {k}: {name} before the freeze"
        if k >= hi:
            for name, x, y in zip(names, ra[k - lag], rb):
                assert np.array_equal(x[S], y[S]), f"step {k}: {name} of the thawed environments against the twin's step {k - lag}"
            done_after_thaw += int(rb[2][S].sum())
        if k == hi - 1:
            assert A(b.get_info("external_wrench"))[pushed, 6] == 3 * a.cfg.action_repeat
    assert done_after_thaw > 0, "no thawed environment was reset: the run shows nothing about resets after the thaw"
    assert a.counter("resets") > n
    a.close(); b.close()


def test_frozen_quads_never_vote(torch_cuda):
    """4. N = 32: every odd robot is thrown on the floor and lands for 10 steps, then exactly those are frozen.  Over the next 30 steps no
    wave of the masked handle takes the many-rows path, in a home wave or in a solo wave, while the unmasked twin's keep taking it; the
    standing robots (held by a joint PD computed here from their own state) match the twin bit for bit."""
    t = torch_cuda
    n = 32
    kw = dict(reset_lookahead=2, solo_waves=32, **RAW)
    a, b = vec_env(n, **kw), vec_env(n, **kw)
    a.reset(); b.reset()
    q0 = A(a.get_state())[:, 13:25].copy()
    s = fallen_half(a, 61)
    a.set_state(s); b.set_state(s)
    odd = np.arange(n) % 2 == 1
    mask = t.as_tensor(~odd, device=b.device)

    def torques(v):
        x = A(v.get_state())
        tau = 60.0 * (q0 - x[:, 13:25]) - 1.5 * x[:, 25:37]
        tau[odd] = 0.0
        return t.as_tensor(np.clip(tau, -20, 20).astype(np.float32), device=v.device)

    for k in range(10):
        tau = torques(a)
        xa, xb = outputs(a, a.step_tensor(tau)), outputs(b, b.step_tensor(tau))
        same(xa, xb, slice(None), f"landing step {k}")
    rare_a, rare_b = [v.counter("limit_path_substeps") for v in (a, b)]
    solo_a, solo_b = [v.counter("solo_path_substeps") for v in (a, b)]
    assert rare_a == rare_b > 0
    for k in range(30):
        tau = torques(a)
        xa, xb = outputs(a, a.step_tensor(tau)), outputs(b, b.step_tensor(tau, active=mask))
        same(xa, xb, ~odd, f"step {k}, the standing robots")
    print("many-rows wave-substeps over 30 steps: unmasked", a.counter("limit_path_substeps") - rare_a, "(solo", a.counter("solo_path_substeps") - solo_a,
          ") masked", b.counter("limit_path_substeps") - rare_b, "(solo", b.counter("solo_path_substeps") - solo_b, ")")
    assert b.counter("limit_path_substeps") == rare_b and b.counter("solo_path_substeps") == solo_b
    assert a.counter("limit_path_substeps") - rare_a > 0 and a.counter("solo_path_substeps") - solo_a > 0
    a.close(); b.close()


def test_all_none_and_one(torch_cuda):
    """5. a mask of ones is no mask; a mask of zeros changes nothing in the handle over 5 steps (snapshot rows and counters), and the next
    unmasked step is the twin's next step; N = 1 frozen, then thawed."""
    t = torch_cuda
    n = 24
    kw = dict(env_randomizer_mode="GROUND_RANDOMIZER", auto_reset=True, reset_lookahead=2, seed=2, noise=True)
    a, b = vec_env(n, **kw), vec_env(n, **kw)
    a.reset_tensor(); b.reset_tensor()
    gen = t.Generator(device=a.device).manual_seed(3)
    acts = t.rand((60, n, a.action_dim), generator=gen, device=a.device) * 2 - 1
    ones, zeros = t.ones(n, dtype=t.bool, device=a.device), t.zeros(n, dtype=t.uint8, device=a.device)
    for k in range(50):
        same(outputs(a, a.step_tensor(acts[k])), outputs(b, b.step_tensor(acts[k], active=ones)), slice(None), f"step {k}, mask of ones")
    assert a.counter("resets") == b.counter("resets") >= n
    last = A(b.step_tensor(acts[50], active=ones)[0])
    a.step_tensor(acts[50])
    rows = A(b.snapshot().rows)
    for k in range(5):
        obs, rew, done, trunc = b.step_tensor(acts[51 + k], active=zeros)
        assert np.array_equal(A(obs), last) and not A(rew).any() and not A(done).any() and not A(trunc).any()
    assert np.array_equal(rows.view(np.int32), A(b.snapshot().rows).view(np.int32))
    for name in ("resets", "limit_path_substeps", "solo_path_substeps", "lookahead_served", "reset_stalls"):
        assert a.counter(name) == b.counter(name), name
    same(outputs(a, a.step_tensor(acts[56])), outputs(b, b.step_tensor(acts[56])), slice(None), "the step after five frozen ones")
    a.close(); b.close()
    one, two = vec_env(1, **kw), vec_env(1, **kw)
    one.reset_tensor(); two.reset_tensor()
    off = t.zeros(1, dtype=t.bool, device=one.device)
    hist = []
    for k in range(30):
        hist.append(outputs(one, one.step_tensor(acts[k, :1].contiguous())))
    for k in range(34):
        if 3 <= k < 7:
            row = A(two.snapshot().rows)
            two.step_tensor(acts[k, :1].contiguous(), active=off)
            assert np.array_equal(row.view(np.int32), A(two.snapshot().rows).view(np.int32))
        else:
            j = k if k < 3 else k - 4
            same(hist[j], outputs(two, two.step_tensor(acts[j, :1].contiguous())), slice(None), f"N = 1, step {k}")
    one.close(); two.close()


@pytest.mark.parametrize("build", ["rack", "lookahead0"])
def test_other_builds(torch_cuda, build):
    """6. N = 24, 20 steps: a handle with a rack and half its robots released; a handle without look-ahead states and so without a parked
    record, whose frozen quads step a private copy of their own record (correct, not faster)."""
    n = 24
    on = np.ones(n, bool)
    on[0:16:3] = False
    on[[17, 23]] = False
    if build == "rack":
        kw = dict(on_rack=True, reset_lookahead=2, body_contacts=True, release=list(range(0, n, 2)), **RAW)
    else:
        kw = dict(reset_lookahead=0, **RAW)
    a, b = twins_under_a_mask(torch_cuda, n, on, 20, 71, **kw)
    a.close(); b.close()


def test_soft_payload_is_refused(torch_cuda):
    t = torch_cuda
    v = vec_env(16, payload="soft", env_randomizer_mode="MASS_RANDOMIZER", seed=3)
    v.reset_tensor()
    a = t.zeros((16, v.action_dim), device=v.device)
    v.step_tensor(a)
    with pytest.raises(RuntimeError, match="active mask is not supported with payload_soft"):
        v.step_tensor(a, active=t.ones(16, dtype=t.bool, device=v.device))
    v.step_tensor(a)
    v.close()


def test_argument_errors(torch_cuda):
    t = torch_cuda
    v = vec_env(16)
    v.reset_tensor()
    a = t.zeros((16, v.action_dim), device=v.device)
    before = A(v.get_state())
    for bad, word in ((t.ones(15, dtype=t.bool, device=v.device), "shape"), (t.ones(16, device=v.device), "bool or uint8"), (t.ones(16, dtype=t.bool), "is on")):
        with pytest.raises(ValueError, match="active.*" + word):
            v.step_tensor(a, active=bad)
    assert np.array_equal(before, A(v.get_state())), "a refused mask launched a step"
    v.close()


# ------------------------------------------------------------------ DeviceVecNormalize
def test_vec_normalize_masked(torch_cuda):
    """7. N = 40, 12 training steps under a mask that changes every step (one step with a single active row, one with none): the statistics
    and the per-environment returns against the float64 restatement (tests/active_ref.py), at the bounds of
    test_gpu_parity.py::test_device_vec_normalize; then a mask of ones against qs_norm_step, bit for bit."""
    t = torch_cuda
    from active_ref import MaskedVecNormalizeRef
    from qs_amd import DeviceVecNormalize
    n = 40
    kw = dict(env_randomizer_mode="GROUND_RANDOMIZER", auto_reset=True, reset_lookahead=2, seed=5)
    env = DeviceVecNormalize(vec_env(n, **kw), training=True)
    ref = MaskedVecNormalizeRef(n, env.obs_dim, training=True)
    env.reset_tensor()
    ref.reset(A(env.old_obs))
    rng = np.random.default_rng(8)
    for k in range(12):
        on = rng.random(n) < 0.6
        if k == 4:
            on[:] = False; on[13] = True
        if k == 7:
            on[:] = False
        act = t.as_tensor(rng.uniform(-1, 1, size=(n, env.action_dim)).astype(np.float32), device=env.device)
        obs, rew, done, _ = env.step_tensor(act, active=t.as_tensor(on, device=env.device))
        o_ref, r_ref, _ = ref.step(A(env.old_obs), A(env.old_reward), A(done), active=on)
        np.testing.assert_allclose(A(obs), o_ref, atol=2e-5, err_msg=f"obs step {k}")
        np.testing.assert_allclose(A(rew), r_ref, atol=2e-5, rtol=1e-5, err_msg=f"reward step {k}")
        s, r = env.get_stats(), ref.stats()
        np.testing.assert_allclose(s["obs_mean"], r["obs_mean"], rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
        np.testing.assert_allclose(s["obs_var"], r["obs_var"], rtol=1e-5, err_msg=f"step {k}")
        np.testing.assert_allclose([s["obs_count"], s["ret_mean"], s["ret_var"], s["ret_count"]], [r["obs_count"], r["ret_mean"], r["ret_var"], r["ret_count"]],
                                   rtol=1e-5, err_msg=f"step {k}")
        assert s["obs_count"] == r["obs_count"] and s["ret_count"] == r["ret_count"]
        np.testing.assert_allclose(A(env._returns()), ref.returns, rtol=1e-5, atol=1e-7, err_msg=f"returns step {k}")
    env.venv.close()
    # a mask of ones: the statistics of qs_norm_step, bit for bit
    a, b = DeviceVecNormalize(vec_env(n, **kw), training=True), DeviceVecNormalize(vec_env(n, **kw), training=True)
    a.reset_tensor(); b.reset_tensor()
    ones = t.ones(n, dtype=t.uint8, device=a.device)
    for k in range(8):
        act = t.as_tensor(rng.uniform(-1, 1, size=(n, a.action_dim)).astype(np.float32), device=a.device)
        xa, xb = a.step_tensor(act), b.step_tensor(act, active=ones)
        for name, x, y in zip(("obs", "reward", "done"), xa, xb):
            assert np.array_equal(A(x), A(y)), f"step {k}: {name}"
    sa, sb = a.get_stats(), b.get_stats()
    for key in sa:
        assert np.array_equal(np.asarray(sa[key]), np.asarray(sb[key])), key
    assert np.array_equal(A(a._returns()), A(b._returns()))
    a.venv.close(); b.venv.close()


# ------------------------------------------------------------------ DeviceARS
def test_ars_freeze_done(torch_cuda):
    """8. one train_iteration() of DeviceARS on an un-normalised environment (N = 64, n_delta = 4, horizon 60, check_every 7) with
    freeze_done=True against False from the same seed: accounts, returns, selection and theta bit for bit, and fewer many-rows
    wave-substeps."""
    t = torch_cuda
    from qs_amd import DeviceARS, DevicePolicy
    got = []
    for freeze in (False, True):
        env = vec_env(64, env_randomizer_mode="GROUND_RANDOMIZER", reset_lookahead=2, seed=4, body_contacts=True)
        pol = DevicePolicy(env.obs_dim, env.action_dim, net_arch=(), activation="none", bias=False, num_envs=64, n_policies=8)
        ars = DeviceARS(env, pol, n_delta=4, n_top=2, horizon=60, check_every=7, seed=11, delta_std=0.5, freeze_done=freeze)
        rare0 = env.counter("limit_path_substeps")
        R = A(ars.train_iteration())
        got.append(dict(ret=A(ars.get("ret")), len=A(ars.get("len")), returns=R, idx=A(ars.get("idx")), w=A(ars.get("w")), theta=A(ars.theta),
                        rare=env.counter("limit_path_substeps") - rare0, steps=ars.last_rollout_steps))
        ars.close(); env.close()
    off, on = got
    for key in ("ret", "len", "returns", "idx", "w", "theta"):
        assert np.array_equal(off[key].view(np.int32), on[key].view(np.int32)), key
    print("many-rows wave-substeps:", off["rare"], "->", on["rare"], "; episode lengths", off["len"].min(), "..", off["len"].max(), "; steps", off["steps"], on["steps"])
    assert off["len"].min() < off["steps"], "no episode ended before the rollout did: freezing had nothing to freeze"
    assert np.abs(off["theta"]).max() > 0
    assert on["rare"] < off["rare"]
