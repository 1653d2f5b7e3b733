"""ARS's bookkeeping on the device, its CPU side: the binding's limit, and the TEST-ONLY host twin of the kernels
(tests/emu/qs_emu_ars.cpp over csrc/qs_ars.h) against the float64 restatement and the derived bounds of tests/ars_ref.py, against
policy.ars_update in float64, on the tie rule and on hand-written accounting sequences."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ars_ref as A  # noqa: E402
from emu import emu_ars as E  # noqa: E402


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def test_the_limit_and_the_getters_of_the_binding():
    from qs_amd import ars
    assert ars.MAX_DELTA == 1024 and len(ars.GET) == 10


def test_device_ars_is_exported():
    import qs_amd
    assert qs_amd.DeviceARS.__name__ == "DeviceARS"
    for name in ("_do_one_update", "evaluate_candidates", "rollout", "train_iteration", "learn", "to_policy", "state_dict", "close"):
        assert callable(getattr(qs_amd.DeviceARS, name)), name


@pytest.mark.parametrize("args, word", [((30, 5, 168, 1), None), ((31, 5, 168, 1), "multiple"), ((2050, 1025, 1, 1), "above 1024"), ((0, 1, 1, 1), "multiple"),
                                        ((2, 1, 0, 1), "n_params"), ((2, 1, 1, 0), "episodes_per_env"), ((2, 0, 1, 1), "n_delta")])
def test_shapes_the_create_entry_refuses(args, word):
    if word is None:
        E.check(*args)
    else:
        with pytest.raises(ValueError, match=word):
            E.check(*args)


@pytest.mark.parametrize("m, n_delta, n_top, n_params", A.SHAPES)
def test_twin_against_float64(m, n_delta, n_top, n_params):
    rng = np.random.default_rng(n_delta * 7 + m)
    theta = (rng.standard_normal(n_params) * 0.3).astype(np.float32)
    delta = rng.standard_normal((n_delta, n_params)).astype(np.float32)
    # perturb
    cand = E.perturb(theta, delta, 0.05)
    ref, bound = A.perturb(theta, delta, 0.05)
    assert cand.shape == (2 * n_delta, n_params) and A.ratio(cand, ref, bound) <= 1.0
    # account: integers equal after every step, ret within gamma_T sum |r|
    N, epe = 2 * n_delta * m, 1 + (m % 2)
    rew, done = A.sequence(N, 12, seed=m)
    acc, ref_steps = E.Accounts(N, epe), A.account(rew, done, epe)
    for t in range(12):
        acc.account(rew[t], done[t])
        r = ref_steps[t]
        assert np.array_equal(acc.len, r["len"]) and np.array_equal(acc.episodes, r["episodes"]) and np.array_equal(acc.alive.astype(bool), r["alive"]), t
        assert acc.n_alive == r["n_alive"], t
        assert A.ratio(acc.ret, r["ret"], r["bound"]) <= 1.0, t
    assert 0 < ref_steps[-1]["n_alive"] < N or N <= 2
    # returns (the twin's float32 accounts are the inputs)
    R, steps = acc.returns(n_delta, 0.25)
    R64, steps64, bR = A.returns(acc.ret, acc.len, n_delta, 0.25)
    assert steps == steps64 == int(acc.len.sum()) and A.ratio(R, R64, bR) <= 1.0
    # select: exact idx and w (the float32 returns are the inputs), std and step within the derived bounds
    idx, w, std, step = E.select(R, n_top, 0.02)
    s = A.select(R, n_top, 0.02)
    assert np.array_equal(idx, s["idx"])
    assert np.array_equal(bits(w), bits(s["w"].astype(np.float32)))
    assert abs(float(std) - s["std"]) <= s["e_std"] and abs(float(step) - s["step"]) <= s["e_step"], (std, s)
    # apply
    new = E.apply(theta, delta, idx, w, step)
    new64, bT = A.apply(theta, delta, s["idx"], s["w"], s["step"], s["e_step"])
    assert A.ratio(new, new64, bT) <= 1.0
    assert np.isfinite(new).all() and (new != theta).any()


def test_returns_are_a_function_of_the_block_alone():
    """candidate p's sum does not depend on where its block lies or on the other candidates"""
    rng = np.random.default_rng(3)
    m = 130
    ret, length = rng.standard_normal(m).astype(np.float32) * 50, rng.integers(1, 300, m).astype(np.int32)
    one, _ = E.returns(np.tile(ret, 2), np.tile(length, 2), 1, 0.5)
    many, steps = E.returns(np.tile(ret, 10), np.tile(length, 10), 5, 0.5)
    assert len(set(bits(many).tolist())) == 1 and bits(many)[0] == bits(one)[0] and steps == 10 * int(length.sum())
    # the stated order, spelled out: lane c takes c, c + 64, ...; then the lanes ascending
    term = np.float32(0.5) * length.astype(np.float64) + ret.astype(np.float64)      # (fmaf: one rounding of the exact value)
    term = term.astype(np.float32)
    lanes = np.zeros(64, np.float32)
    for e in range(m):
        lanes[e % 64] = np.float32(lanes[e % 64] + term[e])
    tot = np.float32(0.0)
    for c in range(64):
        tot = np.float32(tot + lanes[c])
    assert bits(tot) == bits(one)[0]


@pytest.mark.parametrize("n_delta, n_top", [(5, 2), (64, 16), (65, 65), (1024, 300)])
def test_twin_against_torch_ars_update(n_delta, n_top):
    """policy.ars_update in float64 on the twin's returns: the same kept set (no ties here) and the same theta within the derived bound"""
    import torch
    from qs_amd.policy import ars_update
    rng = np.random.default_rng(n_delta)
    n_params = 168
    theta = (rng.standard_normal(n_params) * 0.3).astype(np.float32)
    delta = rng.standard_normal((n_delta, n_params)).astype(np.float32)
    R = (rng.permutation(2 * n_delta) * 1.5 + rng.random(2 * n_delta)).astype(np.float32) - n_delta        # no two equal
    assert len(np.unique(R)) == 2 * n_delta
    idx, w, std, step = E.select(R, n_top, 0.02)
    new = E.apply(theta, delta, idx, w, step)
    t64 = lambda x: torch.as_tensor(np.asarray(x, np.float64))
    rp, rm = t64(R[:n_delta]), t64(R[n_delta:])
    top = torch.argsort(torch.maximum(rp, rm), descending=True)[:n_top]
    assert set(top.tolist()) == set(idx.tolist()) and top.tolist() == idx.tolist()
    new_t = ars_update(t64(theta), t64(delta), rp, rm, float(np.float32(0.02)), n_top).numpy()
    s = A.select(R, n_top, 0.02)
    new64, bT = A.apply(theta, delta, s["idx"], s["w"], s["step"], s["e_step"])
    assert np.max(np.abs(new_t - new64)) <= 1e-9 * max(1.0, np.max(np.abs(new64))), "the float64 restatement and torch's float64 ars_update disagree"
    assert A.ratio(new, new_t, bT * (1.0 + 1e-6) + 1e-12) <= 1.0
    assert abs(float(std) - float(torch.cat([rp[top], rm[top]]).std())) <= s["e_std"] * (1.0 + 1e-6) + 1e-12


def test_tie_rule_lower_index_first():
    """integer-valued returns with duplicated scores on both sides of the cut: rank = #{j: score_j > score_k, or equal and j < k}"""
    rp = np.array([5, 7, 7, 3, 7, 1], np.float32)
    rm = np.array([2, 1, 7, 7, 0, 7], np.float32)
    R = np.concatenate([rp, rm])              # scores 5 7 7 7 7 7: the order is 1 2 3 4 5 0
    for n_top, want in ((1, [1]), (3, [1, 2, 3]), (5, [1, 2, 3, 4, 5]), (6, [1, 2, 3, 4, 5, 0])):
        idx, w, std, step = E.select(R, n_top, 0.02)
        assert idx.tolist() == want, (n_top, idx.tolist())
        assert w.tolist() == (rp - rm)[want].tolist()
        s = A.select(R, n_top, 0.02)
        assert s["idx"].tolist() == want
    # all equal: the identity order, std 0, a finite step and a zero update
    idx, w, std, step = E.select(np.full(8, 3.0, np.float32), 4, 0.02)
    assert idx.tolist() == [0, 1, 2, 3] and not w.any() and std == 0.0 and step == np.float32(0.02) / np.float32(1e-6)
    # the generated tie cases of the GPU test hold the same rule in both precisions
    for n_delta, n_top in ((5, 2), (64, 16), (65, 33), (1024, 300)):
        R = A.tied_returns(n_delta, n_top, seed=n_delta)
        score = np.maximum(R[:n_delta], R[n_delta:])
        assert len(np.unique(score)) < n_delta
        idx, w, _, _ = E.select(R, n_top, 0.02)
        s = A.select(R, n_top, 0.02)
        assert np.array_equal(idx, s["idx"]) and np.array_equal(w, s["w"].astype(np.float32))
        order = sorted(range(n_delta), key=lambda k: (-score[k], k))
        assert idx.tolist() == order[:n_top]
        assert score[order[n_top - 1]] == score[order[n_top]], "the cut does not pass through a tie"


def test_accounting_sequences():
    # environment: 0 ends at step 1; 1 never ends; 2 ends at step 2 and gets another `done` at step 4 when it is dead; 3 ends at step 3
    rew = np.array([[1.0, 0.5, 2.0, 1.0], [10.0, 0.25, 3.0, 1.0], [100.0, 0.125, 4.0, 1.0], [1000.0, 1.0, 5.0, 1.0], [1e4, 1.0, 6.0, 1.0]], np.float32)
    done = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 1, 0], [0, 0, 0, 0]], np.uint8)
    acc = E.Accounts(4, 1)
    assert acc.n_alive == 4 and acc.alive.tolist() == [1, 1, 1, 1] and not acc.ret.any() and not acc.len.any()
    want_alive = [[0, 1, 1, 1], [0, 1, 0, 1], [0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]]
    for t in range(5):
        acc.account(rew[t], done[t])
        assert acc.alive.tolist() == want_alive[t] and acc.n_alive == sum(want_alive[t]), t
    assert acc.ret.tolist() == [1.0, 2.875, 5.0, 3.0] and acc.len.tolist() == [1, 5, 2, 3] and acc.episodes.tolist() == [1, 0, 1, 1]
    # episodes_per_env = 2: the same flags; 0 ends twice (steps 1 and 4), 2 ends twice (steps 2 and 4), 3 ends once and stays alive
    acc = E.Accounts(4, 2)
    want_alive = [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 1, 0, 1], [0, 1, 0, 1]]
    for t in range(5):
        acc.account(rew[t], done[t])
        assert acc.alive.tolist() == want_alive[t] and acc.n_alive == sum(want_alive[t]), t
    assert acc.ret.tolist() == [1111.0, 2.875, 14.0, 5.0] and acc.len.tolist() == [4, 5, 4, 5] and acc.episodes.tolist() == [2, 0, 2, 1]
    R, steps = acc.returns(1, 0.0)
    assert R.tolist() == [1113.875, 19.0] and steps == 18
    R, _ = acc.returns(1, -0.5)               # alive_bonus_offset: per step
    assert R.tolist() == [1113.875 - 4.5, 19.0 - 4.5]
