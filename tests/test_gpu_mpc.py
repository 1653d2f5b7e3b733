"""DeviceMPC on the GPU (csrc/qs_mpc.hip): every kernel bit for bit against the host twin (tests/emu/qs_emu_mpc.cpp) over the shapes of
tests/mpc_ref.py on fabricated rewards and dones; MPPI's plans within the derived bounds of the float64 restatement (the measured ratios are
printed and, where QS_RECORD_DIR names a directory, appended to its mpc_parity.jsonl); repeatability; a real planner against a host-driven
one; freeze_done against snapshot and restore; a single candidate; the refusals.
The last shape is (2, 3, 170, 6): 170 is the 1024-element limit rounded down to a whole horizon at six actions.  A horizon of 171 is 1026
elements, which one workgroup cannot hold with a lane per element; test_the_shape_above_the_limit_is_refused holds that it is refused."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import mpc_ref as A  # noqa: E402
from emu import emu_mpc as E  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def host(t):
    return t.cpu().numpy().copy()


def record(rec):
    """one line per case into $QS_RECORD_DIR/mpc_parity.jsonl (what profiles/mpc_parity.json is assembled from); nothing without the variable"""
    out = os.environ.get("QS_RECORD_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "mpc_parity.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def planner(M, C, H, d, **kw):
    from qs_amd import DeviceMPC
    return DeviceMPC(None, M, C, H, action_dim=d, **kw)


@pytest.mark.parametrize("M, C, H, d", A.SHAPES)
def test_kernels_against_the_twin(torch_cuda, M, C, H, d):
    t = torch_cuda
    seed, lam = M * 31 + C, 0.7
    plan, eps = A.inputs(M, C, H, d, seed)
    rew, done, end = A.sequence(M, C, H, seed)
    dev, twin = planner(M, C, H, d, freeze_done=True, temperature=lam), E.Planner(M, C, H, d)
    dev.set_plan(t.from_numpy(plan).cuda())
    twin.set_plan(plan)
    assert np.array_equal(bits(host(dev.get("plan"))), bits(twin.plan))
    # sample
    dev.sample(t.from_numpy(eps).cuda())
    twin.sample(eps, 0.5)
    seq = host(dev.get("seq"))
    assert np.array_equal(bits(seq), bits(twin.seq))
    assert not host(dev.get("score")).any() and host(dev.get("running")).all()
    # every feed: score, running, the action slab and the mask
    r_dev, d_dev, e_dev = t.from_numpy(rew).cuda(), t.from_numpy(done).cuda(), t.from_numpy(end).cuda()
    for h in range(H + 1):
        dev.feed(h, r_dev[h - 1] if h else None, d_dev[h - 1] if h else None, e_dev if h == H else None)
        twin.feed(h, rew[h - 1] if h else None, done[h - 1] if h else None, end if h == H else None)
        assert np.array_equal(bits(host(dev.get("score"))), bits(twin.score)), h
        assert np.array_equal(host(dev.get("running")), twin.running), h
        assert np.array_equal(bits(host(dev.actions)), bits(twin.actions)), h
        assert np.array_equal(host(dev.active), twin.active), h
    assert np.isfinite(twin.score).all()
    # finish under both methods (it reads the sequences and the scores, which it leaves as they are)
    for method in ("best", "mppi"):
        dev.method = method
        dev.finish()
        twin.finish(method, lam)
        assert np.array_equal(host(dev.get("best")), twin.best), method
        assert np.array_equal(bits(host(dev.get("best_score"))), bits(twin.best_score)), method
        assert np.array_equal(bits(host(dev.actions)), bits(twin.actions)), method
        assert np.array_equal(bits(host(dev.get("plan"))), bits(twin.plan)), method
    c64, b_c = A.mppi(twin.score, twin.seq, C, lam)
    act64, plan64 = A.shift(c64)
    b_act, b_plan = A.shift(b_c)
    rec = dict(M=M, C=C, H=H, d=d, temperature=lam, actions_ratio_to_bound=A.ratio(host(dev.actions)[:M], act64, b_act),
               plan_ratio_to_bound=A.ratio(host(dev.get("plan")), plan64, b_plan), largest_bound=float(np.max(b_c)), bits_equal_host=True)
    print("mpc parity:", json.dumps(rec))
    record(rec)
    assert rec["actions_ratio_to_bound"] <= 1.0 and rec["plan_ratio_to_bound"] <= 1.0, rec
    dev.close()


def test_the_shape_above_the_limit_is_refused(torch_cuda):
    with pytest.raises((ValueError, RuntimeError), match="horizon \\* action_dim"):
        planner(*A.SHAPE_ABOVE)


def test_non_finite_scores_and_ties_on_the_device(torch_cuda):
    t = torch_cuda
    nan, inf = np.nan, np.inf
    scores = np.array([[nan, 1.0, inf, 0.5, -inf], [nan, inf, -inf, nan, inf], [7.0, -3.0, 7.0, 7.0, -5.0]], np.float32)
    M, C, H, d = 3, 5, 2, 6
    plan, eps = A.inputs(M, C, H, d, 2)
    N = M * (1 + C)
    rew = np.zeros((H, N), np.float32)
    rew[0, M:] = scores.reshape(-1)
    done, end = np.zeros((H, N), np.uint8), np.zeros((N, 1), np.float32)
    for method in ("best", "mppi"):
        dev, twin = planner(M, C, H, d, method=method, temperature=0.5), E.Planner(M, C, H, d)
        dev.set_plan(t.from_numpy(plan).cuda())
        twin.set_plan(plan)
        dev.sample(t.from_numpy(eps).cuda())
        twin.sample(eps, 0.5)
        for h in range(H + 1):
            dev.feed(h, t.from_numpy(rew[h - 1]).cuda() if h else None, t.from_numpy(done[h - 1]).cuda() if h else None, t.from_numpy(end).cuda() if h == H else None)
            twin.feed(h, rew[h - 1] if h else None, done[h - 1] if h else None, end if h == H else None, mask=False)
        dev.finish()
        twin.finish(method, 0.5)
        assert host(dev.get("best")).tolist() == twin.best.tolist() == [1, 0, 0], method
        assert np.array_equal(bits(host(dev.get("best_score"))), bits(twin.best_score))
        assert np.array_equal(bits(host(dev.get("plan"))), bits(twin.plan)) and np.array_equal(bits(host(dev.actions)), bits(twin.actions)), method
        assert np.isfinite(host(dev.get("plan"))).all() and np.isfinite(host(dev.actions)).all()
        assert host(dev.active).all(), "a planner without freeze_done wrote the mask"
        dev.close()


def test_the_same_seed_gives_the_same_bits(torch_cuda):
    t = torch_cuda
    M, C, H, d = 3, 70, 4, 6
    rew, done, end = A.sequence(M, C, H, 4)
    r_dev, d_dev, e_dev = t.from_numpy(rew).cuda(), t.from_numpy(done).cuda(), t.from_numpy(end).cuda()
    out = []
    for _ in range(2):
        dev = planner(M, C, H, d, method="mppi", temperature=0.3, seed=11)
        got = []
        for _ in range(3):                                      # three control steps: the plan feeds the next sample
            dev.sample(dev.sample_eps())
            for h in range(H + 1):
                dev.feed(h, r_dev[h - 1] if h else None, d_dev[h - 1] if h else None, e_dev if h == H else None)
            dev.finish()
            got += [host(dev.get("seq")), host(dev.get("score")), host(dev.get("plan")), host(dev.actions)]
        out.append(got)
        dev.close()
    for a, b in zip(*out):
        assert np.array_equal(bits(a), bits(b))
    assert np.abs(out[0][-2]).max() > 0


KW = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", action_space_mode="SYMMETRIC", motor_control_mode="PD", enable_springs=True,
          enable_action_filter=True, env_randomizer_mode="GROUND_RANDOMIZER", noise=False, seed=3, auto_reset=True)
M_, C_, H_ = 3, 5, 3


def make_env():
    from qs_amd import QuadrupedVecEnv
    env = QuadrupedVecEnv(num_envs=M_ * (1 + C_), device=0, **KW)
    env.reset_tensor()
    return env


@pytest.mark.parametrize("method", ["best", "mppi"])
def test_a_real_planner_against_the_host_driven_one(torch_cuda, method):
    """four control steps: DeviceMPC.step() on one handle; on a second, identically seeded handle the twin plans, with every step's rewards and
    dones copied to the host.  The real robots' states and the plans are the same bits after every control step."""
    t = torch_cuda
    from qs_amd import DeviceMPC
    M, C, H, lam = M_, C_, H_, 0.4
    env, env2 = make_env(), make_env()
    mpc = DeviceMPC(env, M, C, H, sigma=0.5, method=method, temperature=lam, seed=7)
    d, n = mpc.d, mpc.num_envs
    twin = E.Planner(M, C, H, d)
    gen = t.Generator(device="cuda").manual_seed(7)
    keep, moved = None, False
    for k in range(4):
        obs, rew, done, trunc = mpc.step()
        assert obs.shape[0] == rew.shape[0] == done.shape[0] == M
        # the host-driven control step
        env2.fork(src_of=mpc.src_of)
        keep = env2.snapshot(indices=mpc.real_mask, out=keep)
        twin.sample(host(t.randn((H, M * C, d), generator=gen, device="cuda")), 0.5)
        r = dn = None
        for h in range(H):
            twin.feed(h, r, dn, mask=False)
            _, r, dn, _ = env2.step_tensor(t.from_numpy(twin.actions).cuda())
            r, dn = host(r), host(dn)
        twin.feed(H, r, dn, host(env2.get_info("reward_end")), mask=False)
        assert np.array_equal(bits(host(mpc.get("score"))), bits(twin.score)), k
        assert np.array_equal(bits(host(mpc.get("seq"))), bits(twin.seq)), k
        twin.finish(method, lam)
        env2.restore(keep, indices=mpc.real_mask)
        _, _, dn, _ = env2.step_tensor(t.from_numpy(twin.actions).cuda())
        twin.set_plan(None, mask=host(dn)[:M])
        assert np.array_equal(host(mpc.get("best")), twin.best), k
        assert np.array_equal(bits(host(mpc.get("plan"))), bits(twin.plan)), k
        assert np.array_equal(bits(host(env.get_state())[:M]), bits(host(env2.get_state())[:M])), k
        moved = moved or bool(np.abs(twin.plan).max() > 0)
    assert moved, "the plan never left zero: the comparison shows nothing"
    mpc.close()
    env.close()
    env2.close()


@pytest.mark.parametrize("method", ["best", "mppi"])
def test_freeze_done_gives_the_bits_of_snapshot_and_restore(torch_cuda, method):
    from qs_amd import DeviceMPC
    envs = [make_env(), make_env()]
    mpcs = [DeviceMPC(env, M_, C_, H_, method=method, temperature=0.4, seed=9, freeze_done=f) for env, f in zip(envs, (False, True))]
    for k in range(4):
        rows = [m.step() for m in mpcs]
        for a, b in zip(*rows):
            assert np.array_equal(host(a).view(np.int32) if a.dtype.is_floating_point else host(a), host(b).view(np.int32) if b.dtype.is_floating_point else host(b)), k
        for what in ("score", "plan", "seq", "best"):
            assert np.array_equal(host(mpcs[0].get(what)).view(np.int32), host(mpcs[1].get(what)).view(np.int32)), (k, what)
        assert np.array_equal(bits(host(envs[0].get_state())[:M_]), bits(host(envs[1].get_state())[:M_])), k
    assert mpcs[1]._keep is None and mpcs[0]._keep is not None          # no snapshot was taken under freeze_done
    act = host(mpcs[1].active)
    assert not act[:M_].any()
    for m in mpcs:
        m.close()
    for e in envs:
        e.close()


@pytest.mark.parametrize("method", ["best", "mppi"])
def test_a_single_candidate_takes_the_plan_and_shifts_it(torch_cuda, method):
    t = torch_cuda
    M, C, H, d = 2, 1, 3, 6
    plan, _ = A.inputs(M, C, H, d, 8)
    rew, done, end = A.sequence(M, C, H, 8)
    dev = planner(M, C, H, d, method=method, temperature=0.2)
    dev.set_plan(t.from_numpy(plan).cuda())
    dev.sample(dev.sample_eps())
    for h in range(H + 1):
        dev.feed(h, t.from_numpy(rew[h - 1]).cuda() if h else None, t.from_numpy(done[h - 1]).cuda() if h else None, t.from_numpy(end).cuda() if h == H else None)
    dev.finish()
    act, nxt = A.shift(plan)
    assert np.array_equal(bits(host(dev.actions)[:M]), bits(act)) and np.array_equal(bits(host(dev.get("plan"))), bits(nxt))
    assert not host(dev.get("best")).any()
    dev.reset_plan([1])
    got = host(dev.get("plan"))
    assert np.array_equal(bits(got[0]), bits(nxt[0])) and not got[1].any()
    dev.close()


class NoMask:
    """an environment whose step_tensor has no active="""

    def __init__(self, env):
        self.env, self.num_envs, self.action_dim, self.device = env, env.num_envs, env.action_dim, env.device

    def step_tensor(self, actions):
        return self.env.step_tensor(actions)


def test_refusals(torch_cuda):
    t = torch_cuda
    from qs_amd import DeviceMPC
    env = make_env()
    with pytest.raises(ValueError, match="num_envs"):
        DeviceMPC(env, M_, C_ + 1, H_)
    with pytest.raises(ValueError, match="active="):
        DeviceMPC(NoMask(env), M_, C_, H_, freeze_done=True)
    DeviceMPC(NoMask(env), M_, C_, H_).close()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            DeviceMPC(env, M_, C_, H_, method="mppi", temperature=bad)
    with pytest.raises(ValueError, match="method"):
        DeviceMPC(env, M_, C_, H_, method="cem")
    with pytest.raises(ValueError, match="n_candidates"):
        DeviceMPC(None, 1, 4097, 1, action_dim=6)
    mpc = DeviceMPC(env, M_, C_, H_)
    d = mpc.d
    for bad in (t.zeros((M_ * C_, H_, d), device="cuda"), t.zeros((H_, M_ * C_, d), device="cuda", dtype=t.float64), t.zeros((H_, M_ * C_, d)),
                t.zeros((H_, d, M_ * C_), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="eps"):
            mpc.sample(bad)
    n = mpc.num_envs
    with pytest.raises(ValueError, match="reward"):
        mpc.feed(1, t.zeros(n - 1, device="cuda"), t.zeros(n, dtype=t.uint8, device="cuda"))
    with pytest.raises(ValueError, match="done"):
        mpc.feed(1, t.zeros(n, device="cuda"), t.zeros(n, dtype=t.bool, device="cuda"))
    with pytest.raises(ValueError, match="reward_end"):
        mpc.feed(H_, t.zeros(n, device="cuda"), t.zeros(n, dtype=t.uint8, device="cuda"), None)
    with pytest.raises(ValueError, match="horizon"):
        mpc.feed(H_ + 1)
    mpc.close()
    env.close()
