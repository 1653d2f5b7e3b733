"""The small cores of the many-rows contact solve (core<0, 4> and core<0, 6>, qs_rare.h) sweep all four or six contact points of their
instantiation, whatever the solve's count: a padded row reads the dummy LDS record, and its all-zero row data must make its impulse and every
change it passes on exactly zero.  Here every count from 0 to 6 goes through the probe kernel (tests/hip/rare_probe.hip), once with clean
inputs and once with NaN in every row slot that a leg does not use while another leg of the environment does: the solver writes such rows
to the dummy record, which the padded rows then read.  Both runs, and the large core<18, 12> (which keeps a branch per row), must give the
same bits; the pyramid also matches the host twin bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip"))
import rare_probe  # noqa: E402
import rare_rows as R  # noqa: E402
from emu import emu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def config(model, thr, iters):
    from qs_amd.config import build_config
    cfg, _ = build_config(n_envs=16, friction_model=model, solver_residual_threshold=thr)
    cfg.solver_iters = iters
    return cfg


def bits(x):
    return (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)


def sets_0_to_6(seed):
    """32 row sets without region-A rows, contact points 0 .. 6 in turn (near-duplicate points in every other wave)"""
    rng = np.random.default_rng(seed)
    return [R.shape_set(rng, 0, k % 7, near_dup=bool(k // 16)) for k in range(32)]


def with_garbage(rows):
    """NaN in every field but `act` of the row slots a leg leaves empty while another leg of the same environment fills them (the solver
    writes those to the dummy record)"""
    rows = rows.copy()
    act = rows[:, :, :, 14] > 0.5                  # [n, leg, row]
    act[:, :, 1:9:3] = act[:, :, 0:9:3]; act[:, :, 2:9:3] = act[:, :, 0:9:3]   # a contact point's friction rows go with its normal
    used = act.any(1, keepdims=True)
    junk = used & ~act
    rows[..., :14][junk] = np.nan
    rows[..., 15][junk] = np.nan
    rows[..., 14][junk] = 0.0
    return rows, int(junk.sum())


@pytest.mark.parametrize("iters", [1, 3, 30])
@pytest.mark.parametrize("thr", [0.0, 1e-7])
@pytest.mark.parametrize("model", ["cone", "pyramid"])
def test_padded_rows_are_exact_zeros(torch_cuda, model, thr, iters):
    cfg = config(model, thr, iters)
    rows, env, warm, pay = R.stack(sets_0_to_6(50))
    mA, mB = R.counts(rows, pay)
    assert (mA == 0).all() and sorted(set(mB.tolist())) == list(range(7))
    dirty, n_junk = with_garbage(rows)
    assert n_junk > 0
    runs = {}
    for name, rr, core in (("clean", rows, "default"), ("dirty", dirty, "default"), ("dirty_6", dirty, "0_6"),
                           ("clean_big", rows, "18_12"), ("dirty_big", dirty, "18_12")):
        rc, lam, plam = rare_probe.solve(cfg, rr, env, warm, pay, core=core)
        assert rc == 0, (name, rc)
        assert np.isfinite(lam).all() and np.isfinite(plam).all(), name
        runs[name] = lam
    for name, lam in runs.items():
        bad = np.nonzero((bits(lam) != bits(runs["clean"])).any((1, 2)))[0]
        assert len(bad) == 0, f"{name}: differs from the clean run for sets {bad.tolist()} (contact points {mB[bad].tolist()})"
    dead = rows[:, :, :, 14] <= 0.5
    dead[:, :, 1:9:3] = dead[:, :, 0:9:3]; dead[:, :, 2:9:3] = dead[:, :, 0:9:3]
    assert not runs["dirty"][dead].any()
    if model == "pyramid":
        tl, _ = emu.rare_solve(cfg, rows, env, warm, pay)
        assert (bits(runs["clean"]) == bits(tl)).all()
