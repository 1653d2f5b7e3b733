"""The sampling planner on the device, its CPU side: the binding's limits and methods, and the TEST-ONLY host twin of the kernels
(tests/emu/qs_emu_mpc.cpp over csrc/qs_mpc.h) against the float64 restatement and the derived bounds of tests/mpc_ref.py, on the tie rule, the
non-finite rule, hand-written accounting sequences, exp_nonpos against float64 exp, and the independence of a robot from the others."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import mpc_ref as A  # noqa: E402
from emu import emu_mpc as E  # noqa: E402


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def test_the_limits_the_getters_and_the_methods_of_the_binding():
    from qs_amd import mpc
    assert mpc.MAX_CANDIDATES == 4096 and mpc.MAX_ELEMENTS == 1024 and len(mpc.GET) == 6
    header = open(os.path.join(REPO, "include", "qs_amd.h")).read()
    for name, value in re.findall(r"QS_MPC_(BEST|MPPI) = (\d+)", header):
        assert mpc.METHOD[name.lower()] == E.METHOD[name.lower()] == int(value), name
    assert len(mpc.METHOD) == 2


def test_device_mpc_is_exported():
    import qs_amd
    assert qs_amd.DeviceMPC.__name__ == "DeviceMPC"
    for name in ("plan", "step", "reset_plan", "get", "close", "sample", "feed", "finish"):
        assert callable(getattr(qs_amd.DeviceMPC, name)), name


@pytest.mark.parametrize("args, word", [((3, 5, 3, 6), None), ((1, 4096, 1, 6), None), ((2, 3, 170, 6), None), (A.SHAPE_ABOVE, "horizon \\* action_dim"),
                                        ((0, 5, 3, 6), "n_robots"), ((3, 0, 3, 6), "n_candidates"), ((3, 5, 0, 6), "horizon"), ((3, 5, 3, 0), "action_dim"),
                                        ((1, 4097, 1, 6), "above 4096"), ((1, 1, 1025, 1), "above 1024"), ((2 ** 30, 1, 1, 1), "31 bits"),
                                        ((2 ** 20, 4096, 1, 1), "31 bits"), ((2 ** 21, 1, 1024, 1), "31 bits")])
def test_shapes_the_create_entry_refuses(args, word):
    if word is None:
        E.check(*args)
    else:
        with pytest.raises(ValueError, match=word):
            E.check(*args)


def test_values_the_calls_refuse():
    E.check_sigma(0.5)
    E.check_sigma(0.0)
    E.check_lambda(1e-3)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            E.check_sigma(bad)
        with pytest.raises(ValueError, match="lambda"):
            E.check_lambda(bad)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="lambda"):
            E.check_lambda(bad)


# ---- exp_nonpos
def grid():
    """dense over [-104, 0]: every multiple of 2^-9, every float32 next to a multiple of ln 2 / 2 (where k changes), the cut and its neighbours"""
    x = [-np.arange(0, 104 * 512 + 1, dtype=np.float64) / 512.0]
    edges = -(np.arange(0, 301) * (np.log(2.0) / 2.0)).astype(np.float32)
    x += [edges, np.nextafter(edges, np.float32(-200)), np.nextafter(edges, np.float32(1))]
    cut = np.float32(A.EXP_CUT)
    x += [np.array([cut, np.nextafter(cut, np.float32(-200)), np.nextafter(cut, np.float32(0)), -104.0, -1e-30, -1e-45, 0.0])]
    x = np.unique(np.concatenate([np.asarray(a, np.float32) for a in x]))
    return x[(x <= 0) & (x >= -104)][::-1].copy()                    # descending from 0


def test_exp_nonpos_is_within_its_derived_bound():
    x = grid()
    got = E.exp_nonpos(x)
    ref = np.exp(x.astype(np.float64))
    r = A.ratio(got, ref, A.exp_bound(x))
    above = x >= A.EXP_CUT
    r_above = A.ratio(got[above], ref[above], A.exp_bound(x[above]))          # (below the cut the error is the bound itself: ratio 1)
    print("exp_nonpos: REL = %.3e (%.2f u) from %s; measured / derived = %.3f above the cut, over %d points" %
          (A.EXP_REL, A.EXP_REL / A.U, A.EXP_TERMS, r_above, int(above.sum())))
    assert r <= 1.0 and r_above < 1.0
    assert A.EXP_REL < 8 * A.U, "the derivation went wrong: a degree-7 polynomial on |r| <= ln 2 / 2 is a few u"
    assert bits(E.exp_nonpos(np.zeros(1)))[0] == bits(np.float32(1.0))
    assert np.all(np.diff(got.astype(np.float64)) <= 0.0), "not monotone over the grid"
    assert np.all(got[x < A.EXP_CUT] == 0.0) and np.all(got[x >= A.EXP_CUT] >= np.float32(2.0 ** -126))
    assert bits(E.exp_nonpos(np.array([-np.inf], np.float32)))[0] == 0


def test_the_first_reduction_step_is_exact():
    """mpc_ref's derivation takes fmaf(k, -LN2_HI, x) as exact: in float64 the product and the difference are exact, and the difference is a float32"""
    x = grid()
    x = x[x >= A.EXP_CUT]
    k = np.rint((x * np.float32(A.K["LOG2E"])).astype(np.float32)).astype(np.float64)
    r1 = x.astype(np.float64) - k * A.K["LN2_HI"]
    assert np.array_equal(r1, r1.astype(np.float32).astype(np.float64))
    assert np.abs(k).max() <= np.ceil(abs(A.EXP_CUT) / np.log(2.0)) + 1
    r = r1 - k * A.K["LN2_LO"]
    assert np.abs(r).max() <= A.EXP_TERMS["R"]


# ---- the twin against float64
def run_twin(M, C, H, d, seed, method, lam=0.7, sigma=0.5, mask=True):
    plan, eps = A.inputs(M, C, H, d, seed)
    rew, done, end = A.sequence(M, C, H, seed)
    p = E.Planner(M, C, H, d)
    p.set_plan(plan)
    p.sample(eps, sigma)
    steps = []
    for h in range(H + 1):
        p.feed(h, rew[h - 1] if h else None, done[h - 1] if h else None, end if h == H else None, mask=mask)
        steps.append((p.score.copy(), p.running.copy(), p.actions.copy(), p.active.copy()))
    seq = p.seq.copy()
    p.finish(method, lam)
    return p, plan, eps, rew, done, end, seq, steps


@pytest.mark.parametrize("M, C, H, d", A.SHAPES)
def test_twin_against_float64(M, C, H, d):
    seed = M * 31 + C
    p, plan, eps, rew, done, end, seq, steps = run_twin(M, C, H, d, seed, "best")
    MC = M * C
    # sample: within one fmaf rounding; candidate 0 is the plan
    seq64, b_seq = A.sample(plan, eps, 0.5, C)
    assert seq.shape == (H, MC, d) and A.ratio(seq, seq64, b_seq) <= 1.0
    assert np.abs(seq).max() <= 1.0
    # feed: flags equal, scores within gamma_H sum |r|, the slab and the mask
    ref = A.scores(rew, done, end, M)
    assert not steps[0][0].any() and steps[0][1].all()
    for h in range(H + 1):
        score, running, actions, active = steps[h]
        if h >= 1:
            r = ref[h - 1]
            assert np.array_equal(running.astype(bool), r["running"]), h
            if h < H:
                # (before the last feed the reference has not added reward_end either)
                assert A.ratio(score, r["score"], r["bound"]) <= 1.0, h
        assert np.array_equal(active[M:], running) and not active[:M].any(), h
        if h < H:
            assert np.array_equal(bits(actions[M:]), bits(seq[h])), h
        assert not actions[:M].any()
    final = ref[-1]
    assert A.ratio(steps[H][0], final["score"], final["bound"]) <= 1.0
    assert np.isfinite(steps[H][0]).all(), "the second column of reward_end was read"
    # best: exact where the float64 scores are separated -- and the fabricated ones are, everywhere
    sep = A.separated(final["score"], final["bound"], C)
    assert sep.all(), "a fabricated case is not separated: it would be skipped"
    b64, _ = A.best(final["score"], C)
    assert np.array_equal(p.best, b64)
    b32, s32 = A.best(steps[H][0], C)
    assert np.array_equal(p.best, b32) and np.array_equal(bits(p.best_score), bits(s32.astype(np.float32)))
    chosen = seq.reshape(H, M, C, d)[:, np.arange(M), p.best].transpose(1, 0, 2)
    act, nxt = A.shift(chosen)
    assert np.array_equal(bits(p.actions[:M]), bits(act)) and np.array_equal(bits(p.plan), bits(nxt))
    # mppi: within the derived bound, at a sharp and at a flat temperature
    for lam in (0.05, 0.7, 30.0):
        q, *_ = run_twin(M, C, H, d, seed, "mppi", lam=lam)
        c64, b_c = A.mppi(steps[H][0], seq, C, lam)
        act64, plan64 = A.shift(c64)
        b_act, b_plan = A.shift(b_c)
        r_a, r_p = A.ratio(q.actions[:M], act64, b_act), A.ratio(q.plan, plan64, b_plan)
        assert r_a <= 1.0 and r_p <= 1.0, (lam, r_a, r_p)
        assert np.array_equal(q.best, p.best) and np.abs(q.plan).max() <= 1.0
        if C > 1:
            assert np.abs(b_c).max() < 1e-3, "the bound says nothing"


def test_a_robot_is_a_function_of_its_block_alone():
    """the tiled inputs give the same bits: robot m's result does not depend on where its block lies or on the other robots"""
    C, H, d = 130, 3, 6
    plan, eps = A.inputs(1, C, H, d, 5)
    rew, done, end = A.sequence(1, C, H, 5)
    for method in ("best", "mppi"):
        out = []
        for M in (1, 4):
            p = E.Planner(M, C, H, d)
            p.set_plan(np.tile(plan, (M, 1, 1)))
            p.sample(np.tile(eps, (1, M, 1)), 0.5)
            tile = lambda a: np.concatenate([np.repeat(a[..., :1], M, -1), np.tile(a[..., 1:], M)], -1)      # [.., N]: reals first, then the blocks
            for h in range(H + 1):
                p.feed(h, tile(rew[h - 1]) if h else None, tile(done[h - 1]) if h else None, tile(end.T).T if h == H else None)
            p.finish(method, 0.7)
            out.append(p)
        one, many = out
        for m in range(4):
            assert np.array_equal(bits(many.plan[m]), bits(one.plan[0])) and np.array_equal(bits(many.actions[m]), bits(one.actions[0])), (method, m)
            assert many.best[m] == one.best[0] and bits(many.best_score[m]) == bits(one.best_score[0])
        assert np.array_equal(bits(many.score.reshape(4, C)), bits(np.tile(one.score, (4, 1))))


def test_candidate_zero_is_the_plan_bit_for_bit():
    M, C, H, d = 2, 5, 3, 6
    plan, eps = A.inputs(M, C, H, d, 1)
    plan[0, 0, :4] = [1.0, -1.0, -0.0, np.nextafter(np.float32(1.0), np.float32(0))]
    p = E.Planner(M, C, H, d)
    p.set_plan(plan)
    p.sample(eps, 0.5)
    zero = p.seq.reshape(H, M, C, d)[:, :, 0].transpose(1, 0, 2)
    assert np.array_equal(bits(zero), bits(plan))
    # sigma = 0: every candidate is the plan
    p.sample(eps, 0.0)
    assert np.array_equal(p.seq.reshape(H, M, C, d), np.broadcast_to(plan.transpose(1, 0, 2)[:, :, None], (H, M, C, d)))


def planner_with_scores(score, H=2, d=3, seed=0):
    """a planner whose candidates carry `score` [M, C] (handed over as reward_end of a one-step rollout would not do: feed them as step rewards)"""
    score = np.asarray(score, np.float32)
    M, C = score.shape
    plan, eps = A.inputs(M, C, H, d, seed)
    p = E.Planner(M, C, H, d)
    p.set_plan(plan)
    p.sample(eps, 0.5)
    N = M * (1 + C)
    rew, done = np.zeros(N, np.float32), np.zeros(N, np.uint8)
    rew[M:] = score.reshape(-1)
    for h in range(H + 1):
        p.feed(h, rew if h == 1 else np.zeros(N, np.float32), done if h else None, np.zeros((N, 1), np.float32) if h == H else None)
    assert np.array_equal(bits(p.score), bits(score.reshape(-1) + np.float32(0.0)))
    return p


def test_tie_rule_lower_index_first():
    p = planner_with_scores([[1, 7, 7, 3, 7], [2, 2, 2, 2, 2], [0.5, -1, 0.25, 0.5, 0.5]])
    seq = p.seq.copy().reshape(p.H, p.M, p.C, p.d)
    p.finish("best")
    assert p.best.tolist() == [1, 0, 0] and p.best_score.tolist() == [7.0, 2.0, 0.5]
    for m, b in enumerate(p.best):
        assert np.array_equal(bits(p.actions[m]), bits(seq[0, m, b])) and np.array_equal(bits(p.plan[m, 0]), bits(seq[1, m, b]))
    assert A.best(p.score, p.C)[0].tolist() == [1, 0, 0]
    # equal scores everywhere under mppi: every weight is 1, the plain mean (in the stated chain's order)
    q = planner_with_scores([[1, 7, 7, 3, 7], [2, 2, 2, 2, 2], [0.5, -1, 0.25, 0.5, 0.5]])
    q.finish("mppi", 0.3)
    assert q.best.tolist() == [1, 0, 0]
    acc = np.zeros((p.H, p.d), np.float32)
    for c in range(p.C):
        acc = (acc.astype(np.float64) + seq[:, 1, c].astype(np.float64)).astype(np.float32)       # fmaf(1, x, acc): one rounding of the exact sum
    mean = np.clip(acc / np.float32(p.C), -1, 1).astype(np.float32)
    assert np.array_equal(bits(q.actions[1]), bits(mean[0])) and np.array_equal(bits(q.plan[1, 0]), bits(mean[1]))


def test_non_finite_scores_never_win():
    nan, inf = np.nan, np.inf
    scores = [[nan, 1.0, inf, 0.5, -inf], [nan, inf, -inf, nan, inf], [inf, -3.0, nan, -3.0, -5.0]]
    for method in ("best", "mppi"):
        p = planner_with_scores(scores)
        seq = p.seq.copy().reshape(p.H, p.M, p.C, p.d)
        p.finish(method, 0.5)
        assert p.best.tolist() == [1, 0, 1], method
        assert p.best_score[0] == 1.0 and p.best_score[1] == -np.inf and p.best_score[2] == -3.0
        assert np.isfinite(p.plan).all() and np.isfinite(p.actions).all(), method
        # all non-finite: candidate 0, the plan as it stood
        assert np.array_equal(bits(p.actions[1]), bits(seq[0, 1, 0])) and np.array_equal(bits(p.plan[1, 0]), bits(seq[1, 1, 0])), method
        if method == "mppi":
            # robot 0: the weights of the three non-finite candidates are 0, so the mean is over candidates 1 and 3
            c64, bound = A.mppi(p.score, p.seq, p.C, 0.5)
            assert A.ratio(p.actions[:p.M], c64[:, 0], bound[:, 0]) <= 1.0
            w = np.array([0.0, 1.0, 0.0, np.exp(-1.0), 0.0])
            want = np.einsum("c,cd->d", w, seq[0, 0].astype(np.float64)) / w.sum()
            assert np.abs(p.actions[0] - np.clip(want, -1, 1)).max() < 1e-5
    assert A.best(np.asarray(scores, np.float32).reshape(-1), 5)[0].tolist() == [1, 0, 1]


def test_accounting_sequences():
    # M = 1, C = 4, H = 3.  candidate 0: done at step 0; 1: done at the last step (no reward_end); 2: never done (gets reward_end);
    # 3: done at step 1, rewards keep arriving and are ignored, and so is a second done
    M, C, H, d = 1, 4, 3, 2
    rew = np.array([[9, 1.0, 0.5, 2.0, 1.0], [9, 10.0, 0.25, 3.0, 1.0], [9, 100.0, 0.125, 4.0, 1000.0]], np.float32)
    done = np.array([[1, 1, 0, 0, 0], [1, 0, 0, 0, 1], [1, 1, 1, 0, 1]], np.uint8)
    end = np.array([[77, 77], [64, 77], [32, 77], [16, 77], [8, 77]], np.float32)
    p = E.Planner(M, C, H, d)
    p.sample(np.zeros((H, C, d), np.float32), 0.5)
    assert p.running.tolist() == [1, 1, 1, 1] and not p.score.any()
    want_running = [[1, 1, 1, 1], [0, 1, 1, 1], [0, 1, 1, 0], [0, 0, 1, 0]]
    want_score = [[0, 0, 0, 0], [1.0, 0.5, 2.0, 1.0], [1.0, 0.75, 5.0, 2.0], [1.0, 0.875, 9.0 + 16.0, 2.0]]
    for h in range(H + 1):
        p.feed(h, rew[h - 1] if h else None, done[h - 1] if h else None, end if h == H else None)
        assert p.running.tolist() == want_running[h] and p.score.tolist() == want_score[h], h
        assert p.active.tolist() == [0] + want_running[h], h
    ref = A.scores(rew, done, end, M)
    assert ref[-1]["score"].tolist() == want_score[-1] and ref[-1]["running"].tolist() == [bool(x) for x in want_running[-1]]
    # without a mask nothing is written to it
    q = E.Planner(M, C, H, d)
    q.sample(np.zeros((H, C, d), np.float32), 0.5)
    q.feed(0, mask=False)
    q.feed(1, rew[0], done[0], mask=False)
    assert q.active.tolist() == [1] * 5 and q.running.tolist() == want_running[1]


def test_set_plan_rows():
    p = E.Planner(3, 2, 2, 2)
    plan = np.arange(12, dtype=np.float32).reshape(3, 2, 2) / 16
    p.set_plan(plan)
    assert np.array_equal(p.plan, plan)
    p.set_plan(None, mask=[0, 1, 0])
    assert np.array_equal(p.plan[[0, 2]], plan[[0, 2]]) and not p.plan[1].any()
    p.set_plan(None)
    assert not p.plan.any()
