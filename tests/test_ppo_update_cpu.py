"""The PPO update without a GPU: the size of qs_ppo_hyper, DevicePPO(update="device") and what it refuses, the host twin of csrc/qs_ppo_train.h
(tests/emu/qs_emu_ppo_train.cpp) under tests/ppo_train_ref.py's yardstick -- gradient, statistics, the part reduction and the sample order,
the tie rule, clip and Adam -- and the stand-alone sanitizer driver."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import ppo_train_ref as T  # noqa: E402
from emu import emu_ppo_train as E  # noqa: E402

NO_CLIP = (-3.0e38, 3.0e38)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


descs = T.descs


def twin_grad(pol, data, idx, hyper):
    """the host twin on data[idx] -> (grad, stats as a dict, refused); the per-sample flags stay in E.grad.last_flags"""
    return T.twin_grad(pol, data, idx, hyper)[:3]


# ---- 1. the C ABI and the Python surface
def test_the_hyper_struct_has_the_size_of_the_host_builds():
    import ctypes as C
    from qs_amd import lib
    assert C.sizeof(lib.QsPpoHyper) == C.sizeof(E.Hyper) == 56 and len(lib.PPO_STATS) == 8


def test_device_ppo_takes_update_device():
    """(fails with TypeError before the update existed)"""
    from qs_amd import DeviceActorCritic, DevicePPO
    pol = DeviceActorCritic(28, 6, num_envs=8, device="cpu")
    algo = DevicePPO(None, pol, n_steps=4, update="device")
    n = pol.actor_params.numel() + pol.critic_params.numel() + 6
    assert algo.update == "device" and algo.exp_avg.shape == algo.exp_avg_sq.shape == algo.grad.shape == (n,) and algo.adam_step == 0
    assert DevicePPO(None, pol, n_steps=4).update == "torch"
    with pytest.raises(ValueError, match="neither"):
        DevicePPO(None, pol, n_steps=4, update="hip")
    with pytest.raises(RuntimeError, match="GPU"):
        algo.train()


@pytest.mark.parametrize("kw, ppo_kw, word", [(dict(net_arch=(65, 64)), {}, "exceed 64"), (dict(net_arch=(64, 64), vf_arch=(32, 32, 32)), {}, "3 hidden layers"),
                                              ({}, dict(clip_range_vf=0.2), "clip_range_vf"), ({}, dict(learning_rate=lambda f: 3e-4 * f), "constants")])
def test_what_the_device_update_refuses_with_its_reason(kw, ppo_kw, word):
    from qs_amd import DeviceActorCritic, DevicePPO
    pol = DeviceActorCritic(28, 6, num_envs=8, device="cpu", **kw)
    with pytest.raises(ValueError, match=word):
        DevicePPO(None, pol, n_steps=4, update="device", **ppo_kw)
    if not ppo_kw.get("learning_rate"):
        DevicePPO(None, pol, n_steps=4, update="torch", **ppo_kw)          # widths up to 256, four hidden layers and clip_range_vf keep working


@pytest.mark.parametrize("who, change, word", [("actor", dict(hidden=(65, 64)), "wider than 64"), ("critic", dict(n_hidden=3, hidden=(8, 8, 8)), "3 hidden layers"),
                                               ("actor", dict(has_bias=0), "biases"), ("actor", dict(action_dim=65), "action_dim")])
def test_what_qs_ppo_create_refuses_with_its_reason(who, change, word):
    import ctypes as C
    pol = T.make_policy(T.NETS["tanh-28-64x64-6"], 0)
    da, dc = descs(pol)
    E.check(da, dc)
    d = da if who == "actor" else dc
    for k, v in change.items():
        setattr(d, k, (C.c_int32 * 4)(*v) if k == "hidden" else v)
    with pytest.raises(ValueError, match=word):
        E.check(da, dc)


def test_the_layout_fits_a_compute_unit_and_the_parts_are_the_references():
    for name, net in T.NETS.items():
        lay = E.layout(*descs(T.make_policy(net, 0)))
        print(name, lay)
        assert lay["parts"] == T.PARTS and lay["waves"] >= 1 and lay["lds_bytes"] <= 160 * 1024


# ---- 2. the host twin under the yardstick
@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("net", sorted(T.NETS))
def test_the_twins_gradient_and_statistics_under_the_yardstick(net, B):
    """float64 takes the twin's own branch on a clip-edge undecided sample (the twin reports its decisions per sample) and the peer's own on
    the peer's side, so no clip-edge sample is granted anything; B = 32849 has parts with two and three full tiles"""
    import torch
    pol, data, idx = T.case(net, B)
    plain = T.restate(pol, data, idx, T.HYPER)
    g64, st64 = T.autograd(pol, data, idx, T.HYPER, torch.float64)
    assert T.measure(plain["g"], plain, g64)[0] < 1e-3, "the float64 restatement and float64 autograd disagree"
    if B >= 100:
        clipped = np.abs(plain["ratio"] - 1.0) > T.HYPER["clip_range"]
        assert 0.05 <= clipped.mean() <= 0.5 and (clipped & (plain["adv"] > 0)).any() and (clipped & (plain["adv"] < 0)).any()
    _, st_peer = T.autograd(pol, data, idx, T.HYPER, torch.float32)
    g, st, refused = twin_grad(pol, data, idx, T.HYPER)
    flags = E.grad.last_flags
    assert refused == 0 and st["refused"] == 0.0
    g2, st2, _ = twin_grad(pol, data, idx, T.HYPER)
    assert np.array_equal(bits(g), bits(g2)) and st == st2
    _, ref = T.yardstick(f"twin {net} B={B}", pol, data, idx, T.HYPER, g, flags)
    T.hold_stats(f"twin {net} B={B}", st, ref, st_peer, st64, B)


# ---- 3. the part reduction and the sample order
@pytest.mark.parametrize("B", [100, 1000])
def test_the_order_of_the_indices_moves_the_result_by_rounding_only(B):
    import torch
    net = "tanh-28-64x64-6"
    pol, data, idx = T.case(net, B)
    ref = T.restate(pol, data, idx, T.HYPER)
    g64, _ = T.autograd(pol, data, idx, T.HYPER, torch.float64)
    g = twin_grad(pol, data, idx, T.HYPER)[0]
    shuffled = idx[np.random.default_rng(B).permutation(B)]
    g64_s, _ = T.autograd(pol, data, shuffled, T.HYPER, torch.float64)
    assert np.max(np.abs(g64_s - g64) / (T.U * ref["S"])) < 1e-6            # float64's own rounding, nine digits below float32's
    g_s = twin_grad(pol, data, shuffled, T.HYPER)[0]
    assert not np.array_equal(bits(g_s), bits(g))                           # (the order is part of the float32 result ...)
    T.yardstick(f"twin, shuffled indices B={B}", pol, data, shuffled, T.HYPER, g_s, E.grad.last_flags)   # (... and every order is under the yardstick)


def test_advantage_moments_of_the_twin():
    rng = np.random.default_rng(0)
    for B in (2, 17, 1000, 5000):
        adv = (2.0 * rng.standard_normal(B + 3) + 0.3).astype(np.float32)
        idx = rng.permutation(B + 3)[:B]
        mean, sd = E.moments(adv, idx)
        a = adv[idx].astype(np.float64)
        # B plain adds / fmafs along a chain of at most B / 1024 + 16 + 64 links: gamma of that length on sum |.|
        k = B // 1024 + 1 + 16 + 64 + 2
        assert abs(mean - a.mean()) <= T.R.gamma(k) * np.abs(a).mean() + T.U * abs(a.mean())
        assert abs(sd - a.std(ddof=1)) <= (T.R.gamma(k + 4) + 4 * T.R.gamma(k) * np.abs(a).mean() / a.std(ddof=1)) * a.std(ddof=1)


# ---- 4. the tie rule
def test_the_tie_rule_is_torchs():
    """dlp = (u1 <= u2) ? -u1 / B : 0 against autograd through torch.min and torch.clamp on this build of torch: inside the range (ties, edges
    included), outside with either sign of A, and A = 0 outside"""
    import torch
    c = 0.2
    lo, hi = float(np.float32(1.0) - np.float32(c)), float(np.float32(1.0) + np.float32(c))
    r0 = torch.tensor([lo, hi, 1.0, 0.9, 1.1, 0.5, 0.5, 1.5, 1.5, 0.5, 1.5, np.nextafter(np.float32(lo), np.float32(0)), np.nextafter(np.float32(hi), np.float32(2))], dtype=torch.float32)
    A = torch.tensor([1.0, 1.0, -2.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 0.0, 0.0, 1.0, -1.0], dtype=torch.float32)
    lr = r0.log().clone().requires_grad_(True)
    r = lr.exp()
    (-torch.min(A * r, A * torch.clamp(r, lo, hi))).sum().backward()
    rn, An = r.detach().numpy(), A.numpy()
    u1, u2 = An * rn, An * np.clip(rn, np.float32(lo), np.float32(hi))
    want = np.where(u1 <= u2, -u1, 0.0)
    assert np.array_equal(lr.grad.numpy(), want.astype(np.float32)), (lr.grad.numpy(), want)
    # and the twin: one sample per row of the table above, B = 1 each (no normalisation), the gradient of log_std's first entry has dlp's sign
    pol = T.make_policy(T.NETS["none-28-12"], 1)
    data = T.make_data(pol, 13, 1)
    for s in range(13):
        d = dict(data)
        lp = float(T.restate(pol, data, np.array([s]), dict(T.HYPER, normalize_advantage=False))["ratio"][0])
        d["advantages"] = data["advantages"].copy(); d["advantages"][s] = An[s]
        d["old_log_prob"] = data["old_log_prob"].copy()
        d["old_log_prob"][s] = np.float32(np.log(lp) + data["old_log_prob"][s].astype(np.float64) - np.log(rn[s].astype(np.float64)))
        hyper = dict(T.HYPER, normalize_advantage=False)
        g = twin_grad(pol, d, np.array([s]), hyper)[0]
        ref = T.restate(pol, d, np.array([s]), hyper)
        if ref["undecided"].any():
            continue                                                        # (the rows at the edges: either side is right in float32)
        assert np.allclose(g, ref["g"], rtol=1e-3, atol=1e-6), s


# ---- 5. clip and Adam
def adam_inputs(n=12345, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((0.3 * rng.standard_normal(n)).astype(np.float32), (1e-2 * rng.standard_normal(n)).astype(np.float32), (1e-4 * rng.random(n)).astype(np.float32),
            (scale * 1e-2 * rng.standard_normal(n)).astype(np.float32))


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("scale, binding", [(1.0, True), (0.01, False)])
def test_the_twins_adam_against_the_float64_formula_under_the_counted_roundings(scale, binding, t):
    p, m, v, g = adam_inputs(scale=scale)
    if t == 1:
        m, v = np.zeros_like(m), np.zeros_like(v)
    g[:7] = 0.0
    p1, m1, v1, norm = E.adam(p, m, v, g, E.hyper(), t)
    p64, m64, v64, norm64, bound, dm, dv = T.adam64(p, m, v, g, t)
    assert (norm64 > 0.5) == binding
    assert abs(norm - norm64) <= (0.5 * T.R.gamma(T.NORM_BLOCK + 49) + 2 * T.U) * norm64
    worst = float(np.max(np.abs(p1 - p64) / bound))
    print(f"adam t={t} binding={binding}: worst |p - p64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert np.all(np.abs(m1 - m64) <= dm) and np.all(np.abs(v1 - v64) <= dv)


@pytest.mark.parametrize("scale", [1.0, 0.01])
def test_three_steps_of_the_twins_adam_against_torchs(scale):
    import torch
    p, m, v, _ = adam_inputs(scale=scale)
    grads = [adam_inputs(seed=k + 1, scale=scale)[3] for k in range(3)]
    out = {}
    for dtype in (torch.float32, torch.float64):
        w = torch.nn.Parameter(torch.as_tensor(p).to(dtype))
        opt = torch.optim.Adam([w], lr=3e-4, eps=1e-5)
        for g in grads:
            w.grad = torch.as_tensor(g).to(dtype)
            torch.nn.utils.clip_grad_norm_([w], 0.5)
            opt.step()
        out[dtype] = w.detach().double().numpy()
    pt, mt, vt = p, np.zeros_like(m), np.zeros_like(v)
    for k, g in enumerate(grads):
        pt, mt, vt, _ = E.adam(pt, mt, vt, g, E.hyper(), k + 1)
    d_twin, d_torch = np.max(np.abs(pt - out[torch.float64])), np.max(np.abs(out[torch.float32] - out[torch.float64]))
    print(f"three steps: twin {d_twin:.3e}, torch float32 {d_torch:.3e} from torch float64")
    assert d_twin <= T.FACTOR * d_torch


# ---- 6. the stand-alone sanitizer driver
def test_the_sanitizer_driver_runs_clean(tmp_path):
    exe = str(tmp_path / "drv_ppo_train")
    subprocess.check_call(["g++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17",
                           "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"), "-o", exe, os.path.join(HERE, "sanitize", "drv_ppo_train.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    clean = r.returncode == 0 and r.stdout.startswith("ok") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert clean, (r.stdout[-300:], r.stderr[-2000:])
