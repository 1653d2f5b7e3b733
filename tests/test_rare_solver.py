"""The many-rows contact solve on the host: the float64 PGS of tests/rare_ref.py against exact LCP solutions and its own complementarity
conditions, the emulation twin (RareSolver<LaneEmu>, qs_rare.h) against it on synthetic and captured row sets, and the GPU probe of the
device solver (tests/hip/rare_probe.hip) builds for gfx950.  tests/test_gpu_rare_solver.py runs the probe."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip"))
import rare_ref  # noqa: E402
import rare_rows as R  # noqa: E402
from emu import emu  # noqa: E402
from qs_amd.config import build_config  # noqa: E402

MB = [0, 1, 4, 5, 6, 7, 11, 12]
MA = [0, 1, 2, 6, 11, 12, 17, 18]
# twin against ref64, per set and relative to max(1, |lambda|): TW_ATOL per sweep plus TW_K x the set's own float32 sensitivity (how far
# the float32 run of the reference lies from the float64 one) -- many-contact sets do not converge in 300 sweeps (friction makes PGS cycle)
# and amplify rounding; a wrong row shows from the first sweep (<= 7e-7 there)
TW_ATOL, TW_K = 2e-6, 16.0


def config(model, thr, iters):
    cfg, _ = build_config(n_envs=16, friction_model=model, solver_residual_threshold=thr)
    cfg.solver_iters = iters
    return cfg


def lcp_exact(M, b):
    """the solution of  M x - b >= 0, x >= 0, x (M x - b) = 0  by enumeration of the active sets (M positive definite: it is unique)"""
    n = len(b)
    for S in itertools.chain.from_iterable(itertools.combinations(range(n), k) for k in range(n + 1)):
        S = list(S)
        x = np.zeros(n)
        if S:
            x[S] = np.linalg.solve(M[np.ix_(S, S)], b[S])
        if (x >= -1e-12).all() and (M @ x - b >= -1e-10).all():
            return x
    raise AssertionError("no active set solves the LCP")


@pytest.mark.parametrize("n_pts", [1, 2, 3])
def test_reference_solves_frictionless_lcp_exactly(n_pts):
    """mu = 0 and 1-3 contact points: the fixed point of the reference's sweeps is the LCP of the normals, M = the Delassus matrix with
    1 / dinv on its diagonal, b = rhs / dinv"""
    rng = np.random.default_rng(n_pts)
    cfg = config("pyramid", 0.0, 3000)
    for trial in range(20):
        legs = rng.choice(4, size=n_pts, replace=True)
        points = [tuple(sorted(set(int(c) for c, L in zip(rng.permutation(3), legs) if L == K))) for K in range(4)]
        if sum(len(p) for p in points) != n_pts:
            points = [tuple(range(int((legs == K).sum()))) for K in range(4)]
        rows, env, warm, pay = R.synthetic(rng, points=points, separating=0.4)
        env[0] = 0.0
        rows, env, warm = rows[None], env[None], warm[None]
        for model in ("pyramid", "cone"):
            lam12, _, _, _ = rare_ref.solve(cfg, rows, env, warm, None, cone=model == "cone")
            w, a, b, rhs, dinv, diag, live, grp = rare_ref.unpack(rows, env, None)
            idx = [p for p in range(rare_ref.NRM0, rare_ref.FRI0) if live[0, p]]
            assert len(idx) == n_pts
            G = -rare_ref.delassus(w, a, b, dinv, live, grp)[0] / np.where(dinv[0] > 0, dinv[0], 1.0)[None, :]
            M = G[np.ix_(idx, idx)] + np.diag(1.0 / dinv[0, idx])
            x = lcp_exact(M, rhs[0, idx] / dinv[0, idx])
            got = np.array([lam12[0, rare_ref.POS[p][0], rare_ref.POS[p][1]] for p in idx])
            np.testing.assert_allclose(got, x, rtol=1e-7, atol=1e-10 * max(1.0, np.abs(x).max()), err_msg=f"trial {trial} {model}")
            assert not lam12[0][:, [1, 2, 4, 5, 7, 8]].any()          # mu = 0: no friction impulse


@pytest.mark.parametrize("model", ["pyramid", "cone"])
def test_reference_complementarity_and_friction_bounds(model):
    """many sweeps on generated sets of up to 4 contact points, 2 limit rows and the payload: every unilateral row is at the clamp of its own
    candidate (lambda >= 0, and lambda = candidate where lambda > 0), friction within mu x its normal impulse (pyramid: each row, where that
    is positive; cone: the pair)"""
    rng = np.random.default_rng(7)
    sets = [R.shape_set(rng, int(rng.choice([0, 1, 2, 6])), int(rng.integers(1, 5)), separating=0.3) for _ in range(64)]
    rows, env, warm, pay = R.stack(sets)
    cfg = config(model, 0.0, 4000)
    lam12, plam, sweeps, resid = rare_ref.solve(cfg, rows, env, warm, pay)
    conv = resid[:, -1] < 1e-10
    assert conv.mean() > 0.8, conv.mean()
    w, a, b, rhs, dinv, diag, live, grp = rare_ref.unpack(rows, env, pay)
    A = rare_ref.delassus(w, a, b, dinv, live, grp)
    lam = np.zeros((len(sets), rare_ref.N))
    for p, (L, r) in enumerate(rare_ref.POS):
        lam[:, p] = plam[:, r] if L == 4 else lam12[:, L, r]
    cand = rhs + np.einsum("njp,nj->np", A, lam)
    scale = np.maximum(1.0, np.abs(lam).max(1))[:, None]
    uni = np.zeros(rare_ref.N, bool); uni[:rare_ref.PAY0] = True; uni[rare_ref.NRM0:rare_ref.FRI0] = True
    m = conv[:, None] & live & uni[None]
    assert (lam[m] >= 0).all()
    assert (np.abs(lam - np.maximum(cand, 0.0))[m] <= 1e-8 * np.broadcast_to(scale, lam.shape)[m]).all()
    mu = env[:, 0].astype(np.float64)
    for f in range(rare_ref.FRI0, rare_ref.N, 2):
        L, r = rare_ref.POS[f]
        ln = lam[:, rare_ref.NRM0 + 3 * L + (r - 1) // 3]
        ok = conv & live[:, f]
        if model == "cone":
            assert (np.hypot(lam[ok, f], lam[ok, f + 1]) <= mu[ok] * ln[ok] * (1 + 1e-9) + 1e-12).all()
        else:
            ok &= ln > 0           # (while the normal impulse is not positive the pair is left alone: Bullet's rule)
            assert (np.abs(lam[ok, f:f + 2]) <= (mu[ok] * ln[ok])[:, None] * (1 + 1e-9) + 1e-12).all()


def twin_vs_ref(cfg, rows, env, warm, pay, label):
    tl, tp = emu.rare_solve(cfg, rows, env, warm, pay)
    rl, rp, sweeps, resid = rare_ref.solve(cfg, rows, env, warm, pay)
    r32, p32, _, _ = rare_ref.solve(cfg, rows, env, warm, pay, dtype=np.float32)
    scale = np.maximum(1.0, np.maximum(np.abs(rl).max((1, 2)), np.abs(rp).max(1)))
    dist = lambda l, p: np.maximum(np.abs(l - rl).max((1, 2)), np.abs(p - rp).max(1)) / scale
    d, d32 = dist(tl, tp), dist(r32, p32)
    thr = cfg.solver_residual_threshold
    clear = ~(np.abs(resid - np.sqrt(thr)) <= 0.01 * np.sqrt(thr)).any(1) if thr > 0 else np.ones(len(rows), bool)
    bound = TW_ATOL * max(1, cfg.solver_iters) + TW_K * d32
    bad = np.nonzero(clear & (d > bound))[0]
    assert len(bad) == 0, f"{label}: twin - ref64 {d[bad[:8]].tolist()} beyond {bound[bad[:8]].tolist()} for sets {bad[:8].tolist()}"
    return clear


@pytest.mark.parametrize("thr", [0.0, 1e-7])
@pytest.mark.parametrize("model", ["pyramid", "cone"])
def test_twin_matches_reference_on_boundary_shapes(model, thr):
    rng = np.random.default_rng(11)
    sets = [R.shape_set(rng, mA, mB, near_dup=nd) for nd in (False, True) for mA in MA for mB in MB]
    sets += [R.synthetic(rng), R.empty()]
    rows, env, warm, pay = R.stack(sets)
    for iters in (0, 1, 2, 3, 30, 300):
        clear = twin_vs_ref(config(model, thr, iters), rows, env, warm, pay, f"{model} thr {thr} iters {iters}")
        assert clear.sum() > len(sets) // 2


@pytest.mark.parametrize("kind", ["thrown", "stop", "payload"])
@pytest.mark.parametrize("model", ["pyramid", "cone"])
def test_twin_matches_reference_on_captured_rows(model, kind):
    """row sets the emulation's own steps produced (thrown robots, joints at their stops, the soft payload)"""
    cfg, rows, env, warm, pay = R.captured(kind, model, 1e-7)
    assert len(rows) >= 64
    mA, mB = R.counts(rows, pay)
    assert {"thrown": mB.max() >= 2, "stop": (mA > 0).sum() >= 16, "payload": pay is not None and (mA >= 6).all()}[kind]
    for iters in (1, 3, 30):
        cfg.solver_iters = iters
        twin_vs_ref(cfg, rows, env, warm, pay, f"{kind} {model} iters {iters}")


def test_probe_builds_for_gfx950():
    """the probe of the device solver cross-compiles with the product's options and exports its entry point"""
    import rare_probe
    so = rare_probe.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "qsp_rare_solve" in syms
    with open(so, "rb") as f:
        assert b"gfx950" in f.read()
