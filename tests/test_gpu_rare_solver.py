"""The device many-rows contact solve (RareSolver<LaneDev, CONE>, qs_rare.h) on its own: row sets handed to a probe kernel
(tests/hip/rare_probe.hip) and its impulses compared with the host emulation twin (RareSolver<LaneEmu>) and the float64 PGS of
tests/rare_ref.py.

The probe compiles the solver's source with the product's hipcc options into a small kernel.  It does not test the machine code inlined
into k_step / k_step_dense, which allocates registers differently: the end-to-end parity tests (test_gpu_parity.py, test_gpu_round2.py)
and tools/gate.sh still cover that.

Bounds:
  * pyramid: the device equals the twin bit for bit (same operation order, explicit fmaf, v_med3 = min / max for finite values);
    +0 and -0 count as equal.
  * cone: v_rsq_f32 is not 1 / sqrtf, so per environment |device - ref64| <= CONE_ATOL x scale + CONE_K x |twin - ref64|, scale =
    max(1, |lambda|) of the set.  Thresholded runs are held to ref64 only on sets whose exit sweep is unambiguous (no sweep's residual
    within 1 % of the threshold).
  * the three instantiations of core<> agree bit for bit wherever each can hold the shape; results depend only on the environment's own rows.
The distances are recorded as rare_solver.jsonl by record_jsonl (test_gpu_parity.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip"))
import rare_probe  # noqa: E402
import rare_ref  # noqa: E402
import rare_rows as R  # noqa: E402
from emu import emu  # noqa: E402
from test_gpu_parity import record_jsonl  # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = ["cone", "pyramid"]
THRESHOLDS = [0.0, 1e-7]
ITERS = [0, 1, 2, 3, 30, 300]
MB = [0, 1, 4, 5, 6, 7, 11, 12]
MA = [0, 1, 2, 6, 11, 12, 17, 18]
CONE_ATOL, CONE_K = 5e-5, 20.0   # recorded: |dev - ref64| / (|twin - ref64| + 2e-6) at most 0.24 up to 3 sweeps, 2.7 at 30, 13.3 at 300


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def config(model, thr, iters):
    from qs_amd.config import build_config
    cfg, _ = build_config(n_envs=16, friction_model=model, solver_residual_threshold=thr)
    cfg.solver_iters = iters     # (what int(300 / action_repeat) gives for action_repeat 1000, 300, 150, 100, 10, 1)
    return cfg


def bits(x):
    """float32 bit patterns with -0 as +0"""
    return (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)


def shape_sets():
    """every (mA, mB) of the boundary lists, twice (the second time with near-duplicate contact points): 128 sets, 8 full waves"""
    rng = np.random.default_rng(20)
    return [R.shape_set(rng, mA, mB, near_dup=nd) for nd in (False, True) for mA in MA for mB in MB]


def edge_waves():
    """wave 0: one busy environment in slot 0, the others with rows but no `mine`; wave 1: the same in slot 15; wave 2: `mine` without live
    rows in every other slot, busy environments between them"""
    rng = np.random.default_rng(21)
    busy = R.shape_set(rng, 12, 7)
    idle = [R.shape_set(rng, 2, 5) for _ in range(16)]
    for s in idle:
        s[1][1] = 0.0
    none = R.synthetic(rng)                    # mine, no rows
    w0 = [busy] + idle[1:]
    w1 = idle[:15] + [busy]
    w2 = [none if k % 2 == 0 else R.shape_set(rng, MA[k // 2 % 8], MB[(k // 2 + 3) % 8]) for k in range(16)]
    return w0 + w1 + w2


def run_all(sets, model, thr, iters, core="default"):
    cfg = config(model, thr, iters)
    rows, env, warm, pay = R.stack(sets)
    rc, lam, plam = rare_probe.solve(cfg, rows, env, warm, pay, core=core)
    assert rc == 0, f"probe returned {rc}"
    return cfg, (rows, env, warm, pay), lam, plam


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("model", MODELS)
def test_device_against_twin_and_float64(torch_cuda, model, thr, iters):
    sets = shape_sets() + edge_waves()
    cfg, (rows, env, warm, pay), lam, plam = run_all(sets, model, thr, iters)
    assert np.isfinite(lam).all() and np.isfinite(plam).all()
    tl, tp = emu.rare_solve(cfg, rows, env, warm, pay)
    rl, rp, sweeps, resid = rare_ref.solve(cfg, rows, env, warm, pay)
    mine = env[:, 1] > 0.5
    # lanes without `mine` and rows that do not exist return 0
    mA, mB = R.counts(rows, pay)
    assert not lam[~mine].any() and not plam[~mine].any()
    no_pay = np.ones(len(sets), bool) if pay is None else pay[:, R.PAY_ACT] <= 0.5
    assert not plam[no_pay].any()
    dead = rows[:, :, :, 14] <= 0.5
    dead[:, :, 1:9:3] = dead[:, :, 0:9:3]; dead[:, :, 2:9:3] = dead[:, :, 0:9:3]
    assert not lam[dead].any()
    scale = np.maximum(1.0, np.maximum(np.abs(rl).max((1, 2)), np.abs(rp).max(1)))
    d_dev = np.maximum(np.abs(lam - rl).max((1, 2)), np.abs(plam - rp).max(1)) / scale
    d_twin = np.maximum(np.abs(tl - rl).max((1, 2)), np.abs(tp - rp).max(1)) / scale
    thr_s = np.sqrt(thr)
    clear = ~(np.abs(resid - thr_s) <= 0.01 * thr_s).any(1) if thr > 0 else np.ones(len(sets), bool)
    early = (sweeps < iters) & (mA + mB > 0)
    record_jsonl("rare_solver", dict(test="device_vs_ref", model=model, thr=thr, iters=iters, n=int(mine.sum()),
                                     dev_max=float(d_dev.max()), dev_med=float(np.median(d_dev)), twin_max=float(d_twin.max()),
                                     twin_med=float(np.median(d_twin)), dev_twin_max=float(np.abs(lam - tl).max()),
                                     ratio_q=[float(x) for x in np.quantile(d_dev[mine] / (d_twin[mine] + CONE_ATOL), [0.5, 0.9, 0.99, 1.0])],
                                     excess_max=float((d_dev - CONE_K * d_twin).max()),
                                     clear=int(clear.sum()), early_exit=int(early.sum()), bitwise_twin=bool((bits(lam) == bits(tl)).all())))
    if thr > 0 and iters >= 30:
        assert early.any(), "no thresholded set left its sweeps early"
        assert (clear & early).any(), "no thresholded set with an unambiguous exit sweep"
    if model == "pyramid":
        bad = np.nonzero((bits(lam) != bits(tl)).any((1, 2)) | (bits(plam) != bits(tp)).any(1))[0]
        assert len(bad) == 0, f"pyramid: device != twin bitwise for sets {bad[:10].tolist()} (shapes {[(int(mA[i]), int(mB[i])) for i in bad[:10]]})"
    else:
        bound = CONE_ATOL + CONE_K * d_twin
        bad = np.nonzero(clear & (d_dev > bound))[0]
        assert len(bad) == 0, f"cone: |device - ref64| beyond {CONE_ATOL} + {CONE_K} |twin - ref64| for sets {bad[:10].tolist()}: " \
            f"{d_dev[bad[:10]].tolist()} vs {bound[bad[:10]].tolist()} (shapes {[(int(mA[i]), int(mB[i])) for i in bad[:10]]})"


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("model", MODELS)
def test_instantiations_agree_bitwise(torch_cuda, model, thr):
    """core<0, 4>, <0, 6> and <18, 12>, forced, give the same bits wherever each can hold the shape; the default choice is the forced one"""
    rng = np.random.default_rng(30)
    small4 = [R.shape_set(rng, 0, mB, near_dup=bool(k & 1)) for k in range(16) for mB in [[0, 1, 2, 3, 4][k % 5]]]
    small6 = [R.shape_set(rng, 0, [5, 6][k % 2], near_dup=bool(k & 2)) for k in range(16)]
    big = [R.shape_set(rng, MA[k % 8], MB[(k * 3) % 8]) for k in range(16)]
    for iters in (1, 2, 30, 300):
        r4 = {c: run_all(small4, model, thr, iters, c)[2:] for c in ("default", "0_4", "0_6", "18_12")}
        r6 = {c: run_all(small6, model, thr, iters, c)[2:] for c in ("default", "0_6", "18_12")}
        rb = {c: run_all(big, model, thr, iters, c)[2:] for c in ("default", "18_12")}
        for res in (r4, r6, rb):
            for c, (lam, plam) in res.items():
                assert (bits(lam) == bits(res["default"][0])).all() and (bits(plam) == bits(res["default"][1])).all(), (iters, c)
    cfg = config(model, thr, 30)
    rows, env, warm, pay = R.stack(small6)
    assert rare_probe.solve(cfg, rows, env, warm, pay, core="0_4")[0] == rare_probe.ERR_SHAPE
    rows, env, warm, pay = R.stack(big)
    assert rare_probe.solve(cfg, rows, env, warm, pay, core="0_6")[0] == rare_probe.ERR_SHAPE


@pytest.mark.parametrize("model", MODELS)
def test_result_depends_on_own_rows_only(torch_cuda, model):
    """each set of a full wave, alone in slot 0 / slot 15 of an otherwise idle wave (neighbours with rows but no `mine`) or among 15 busy
    neighbours: the same bits"""
    rng = np.random.default_rng(40)
    sets = [R.shape_set(rng, MA[k % 8], MB[(k * 5 + 1) % 8], near_dup=bool(k & 4)) for k in range(16)]
    idle = []
    for _ in range(15):
        s = R.shape_set(rng, 11, 12)
        s[1][1] = 0.0
        idle.append(s)
    for iters in (2, 300):
        full = run_all(sets, model, 1e-7, iters)
        mixed = run_all(sets[::-1], model, 1e-7, iters)
        for k in range(16):
            for slot, wave in ((0, [sets[k]] + idle), (15, idle + [sets[k]])):
                _, _, lam, plam = run_all(wave, model, 1e-7, iters)
                assert (bits(lam[slot]) == bits(full[2][k])).all() and (bits(plam[slot]) == bits(full[3][k])).all(), (iters, k, slot)
                assert not lam[np.arange(16) != slot].any()
            assert (bits(mixed[2][15 - k]) == bits(full[2][k])).all(), (iters, k)


@pytest.mark.parametrize("model", MODELS)
def test_device_on_captured_rows(torch_cuda, model):
    """row sets the host emulation's own steps produced (thrown robots, joints at their stops, the soft payload), thresholded as the default
    configuration is: pyramid bitwise against the twin, cone within the bound against ref64"""
    for kind in ("thrown", "stop", "payload"):
        cfg, rows, env, warm, pay = R.captured(kind, model, 1e-7, max_sets=128)
        for iters in (3, 30):
            cfg.solver_iters = iters
            rc, lam, plam = rare_probe.solve(cfg, rows, env, warm, pay)
            assert rc == 0, rc
            tl, tp = emu.rare_solve(cfg, rows, env, warm, pay)
            if model == "pyramid":
                assert (bits(lam) == bits(tl)).all() and (bits(plam) == bits(tp)).all(), (kind, iters)
                continue
            rl, rp, _, resid = rare_ref.solve(cfg, rows, env, warm, pay)
            scale = np.maximum(1.0, np.maximum(np.abs(rl).max((1, 2)), np.abs(rp).max(1)))
            d_dev = np.maximum(np.abs(lam - rl).max((1, 2)), np.abs(plam - rp).max(1)) / scale
            d_twin = np.maximum(np.abs(tl - rl).max((1, 2)), np.abs(tp - rp).max(1)) / scale
            clear = ~(np.abs(resid - np.sqrt(1e-7)) <= 0.01 * np.sqrt(1e-7)).any(1)
            record_jsonl("rare_solver", dict(test="captured", kind=kind, iters=iters, dev_max=float(d_dev.max()), twin_max=float(d_twin.max())))
            assert not (clear & (d_dev > CONE_ATOL + CONE_K * d_twin)).any(), (kind, iters)
