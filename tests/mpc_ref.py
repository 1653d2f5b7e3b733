"""Float64 restatement of the sampling planner on the device (csrc/qs_mpc.h, steps 1-4) and the bounds a float32 evaluation in the header's order
is held to (TEST INFRASTRUCTURE; shared by tests/test_mpc_cpu.py and tests/test_gpu_mpc.py).

Every bound counts the roundings of the header's sequence with u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1).  The inputs of each step are float32 numbers and enter the float64 restatement exactly.  No constant is
measured; the constants of exp_nonpos are READ from the header, and their distances from log2 e, ln 2 and 1 / i! are computed here.
  sample    one fmaf per element, then a clamp (monotone, non-expansive):   |d seq| <= u |plan + sigma eps|;  candidate 0 is the plan: EQUAL
  feed      at most H + 1 terms (H rewards and reward_end) added to 0 in step order; the first addition is exact:
                                                                            |d score| <= gamma_H sum |r|  over the terms that were added;  running: EQUAL
  best      comparisons of float32 numbers: EQUAL to the float64 choice wherever the two largest float64 scores of a robot lie further apart
            than their two bounds together
  exp_nonpos(x), EXP_CUT <= x <= 0:
            t = fl(x LOG2E):  |t - x log2 e| <= |x| (|LOG2E - log2 e| + LOG2E u) = e_t   (taken at |x| = |EXP_CUT|)
            k = rint(t):      |x log2 e - k| <= 1/2 + e_t, so r* = x - k ln 2 has |r*| <= ln 2 (1/2 + e_t)
            r1 = fmaf(k, -LN2_HI, x) is exact (k LN2_HI has at most 16 significant bits; the difference is a multiple of ulp(x) no larger than
            |x|: test_mpc_cpu.py checks it on its grid);  r = fmaf(k, -LN2_LO, r1): one rounding, and the constants' own error:
                              |r - r*| <= |k| |ln 2 - (LN2_HI + LN2_LO)| + u (|r*| + that) = e_r,  |k| <= K_MAX = ceil(|EXP_CUT| log2 e) + 1
            with R = ln 2 (1/2 + e_t) + e_r >= |r|:
              truncation of the Taylor polynomial of degree 7 (Lagrange):   R^8 / 8! e^R
              the coefficients' rounding:                                   sum_i |c_i - 1 / i!| R^i
              Horner in 7 fmafs: the term c_i r^i passes through min(i, 6) + 1 roundings:   sum_i gamma_(min(i, 6) + 1) c_i R^i
            their sum, relative to exp(r) >= e^-R, is rel_poly;  exp(r) against exp(r*) is a factor e^(e_r);  ldexpf is exact (the result is a
            normal number: exp(EXP_CUT) (1 - REL) > 2^-126, asserted below):      REL = (1 + rel_poly) e^(e_r) - 1
            x < EXP_CUT: the result is 0 and the error is exp(x) itself.
  mppi      per robot, from the float32 scores s_c and sequences:  x_c = (s_c - s_max) / lambda: a subtraction and a division (C_DIV u):
              e_x = |x| ((1 + u) (1 + C_DIV u) - 1);   e_w = e^x (e^(e_x) (1 + REL) - 1), or e^(x + e_x) where x - e_x < EXP_CUT (0 or the value)
              Z: ceil(C / 64) + min(C, 64) additions:      e_Z = sum e_w + gamma_depth sum (w + e_w)
              A = chain of C fmafs of w_c seq_c:           e_A = sum e_w |seq_c| + gamma_C sum (w_c + e_w) |seq_c|
              q = A / Z:  e_q = (e_A + |q| e_Z) / (Z - e_Z), then one division: + C_DIV u (|q| + e_q);  the clamp is non-expansive.
            C_DIV = 2: the float32 division is documented as within 1 ulp = 2 u on the device (correctly rounded on the host and, as the library
            is built, on the device).
"""
import math
import os
import re

import numpy as np

U = 2.0 ** -24
C_DIV = 2.0
# (M, C, H, d): the smallest shapes at which the kernels can go wrong
SHAPES = [(1, 1, 1, 6),        # a single candidate, which is the plan
          (3, 5, 3, 6),        # a partial wave everywhere, M C d not a multiple of 64
          (2, 64, 2, 12),      # one full lane pass, the 12-wide action space
          (2, 70, 4, 6),       # lanes that take two candidates
          (5, 130, 2, 6),      # more than two candidates per lane
          (1, 4096, 1, 6),     # the LDS limit
          (2, 3, 170, 6)]      # H d = 1020: the 1024 limit rounded down to a whole horizon (sixteen waves of elements, the last one partial)
# the horizon above it: 171 * 6 = 1026 elements do not fit one workgroup and are refused (both tests hold that)
SHAPE_ABOVE = (2, 3, 171, 6)


def _header_constants():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadruped-springs_amd", "csrc", "qs_mpc.h")
    text = open(path).read()
    out = {}
    for name in ("LOG2E", "LN2_HI", "LN2_LO", "EXP_CUT", "EXP_C2", "EXP_C3", "EXP_C4", "EXP_C5", "EXP_C6", "EXP_C7"):
        m = re.search(r"constexpr float " + name + r" = (-?[0-9.e+-]+)f;", text)
        assert m, name
        out[name] = float(np.float32(float(m.group(1))))      # the float32 number the compiler makes of the literal
    return out


K = _header_constants()
EXP_CUT = K["EXP_CUT"]
COEF = [1.0, 1.0] + [K[f"EXP_C{i}"] for i in range(2, 8)]


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(x):
    return np.asarray(x, np.float64)


def _derive_exp_bound():
    log2e, ln2 = 1.0 / math.log(2.0), math.log(2.0)
    e_t = abs(EXP_CUT) * (abs(K["LOG2E"] - log2e) + K["LOG2E"] * U)
    r_star = ln2 * (0.5 + e_t)
    k_max = math.ceil(abs(EXP_CUT) * log2e) + 1
    e_c = k_max * abs(ln2 - (K["LN2_HI"] + K["LN2_LO"]))
    e_r = e_c + U * (r_star + e_c)
    R = r_star + e_r
    trunc = R ** 8 / math.factorial(8) * math.exp(R)
    coef = sum(abs(COEF[i] - 1.0 / math.factorial(i)) * R ** i for i in range(8))
    horner = sum(gamma(min(i, 6) + 1) * COEF[i] * R ** i for i in range(8))
    rel_poly = (trunc + coef + horner) * math.exp(R)
    rel = (1.0 + rel_poly) * math.exp(e_r) - 1.0
    assert math.exp(EXP_CUT) * (1.0 - rel) > 2.0 ** -126, "a result above the cut could be subnormal: ldexpf would round"
    return rel, dict(e_t=e_t, R=R, e_r=e_r, truncation=trunc, coefficients=coef, horner=horner, rel_poly=rel_poly)


EXP_REL, EXP_TERMS = _derive_exp_bound()
EXP_REL_F64 = 4.0 * 2.0 ** -53         # numpy's float64 exp, the yardstick itself


def exp_bound(x):
    """|exp_nonpos(x) - exp(x)| for float32 x <= 0: REL exp(x) above the cut, exp(x) (the result is 0) below it"""
    x = f64(x)
    e = np.exp(x)
    return np.where(x < EXP_CUT, e, (EXP_REL + EXP_REL_F64) * e)


def sample(plan, eps, sigma, C):
    """plan [M, H, d], eps [H, M C, d] float32 -> (seq [H, M C, d] float64, bound)"""
    p, e, s = f64(plan), f64(eps), float(np.float32(sigma))
    M, H, d = p.shape
    base = np.repeat(p.transpose(1, 0, 2), C, axis=1)                 # [H, M C, d]: candidate i's plan row
    raw = base + s * e
    seq, bound = np.clip(raw, -1.0, 1.0), U * np.abs(raw)
    first = np.arange(M) * C
    seq[:, first], bound[:, first] = base[:, first], 0.0
    return seq, bound


def scores(rewards, dones, reward_end, M):
    """rewards [H, N] float32, dones [H, N], reward_end [N, k] -> per feed h = 1 .. H a dict(score float64 [M C], running bool [M C], bound)"""
    r, dn, re_ = f64(rewards)[:, M:], np.asarray(dones).astype(bool)[:, M:], f64(reward_end)[M:, 0]
    H = r.shape[0]
    score, mag, running = np.zeros(r.shape[1]), np.zeros(r.shape[1]), np.ones(r.shape[1], bool)
    out = []
    for h in range(H):
        score = np.where(running, score + r[h], score)
        mag = np.where(running, mag + np.abs(r[h]), mag)
        running = running & ~dn[h]
        if h == H - 1:
            score = np.where(running, score + re_, score)
            mag = np.where(running, mag + np.abs(re_), mag)
        out.append(dict(score=score.copy(), running=running.copy(), bound=gamma(H) * mag))
    return out


def key(score):
    """a score that is not finite counts as -inf"""
    s = f64(score).copy()
    s[~np.isfinite(s)] = -np.inf
    return s


def best(score, C):
    """score [M C] -> (best [M] by the stated rule (the lowest index among the maxima; 0 where no score is finite), s_max [M])"""
    s = key(score).reshape(-1, C)
    b = np.argmax(s, axis=1)                          # numpy's argmax is the first maximum
    return b, s[np.arange(len(b)), b]


def separated(score, bound, C):
    """per robot: whether its two largest float64 scores lie further apart than their bounds together (C = 1: nothing to confuse)"""
    s, e = key(score).reshape(-1, C), np.broadcast_to(f64(bound), np.shape(score)).reshape(-1, C)
    if C == 1:
        return np.ones(len(s), bool)
    order = np.argsort(-s, axis=1, kind="stable")
    rows = np.arange(len(s))
    a, b = order[:, 0], order[:, 1]
    return s[rows, a] - s[rows, b] > e[rows, a] + e[rows, b]


def shift(chosen):
    """chosen [M, H, d] -> (actions [M, d], plan [M, H, d]): the rest of the sequence, the last action held"""
    return chosen[:, 0], np.concatenate([chosen[:, 1:], chosen[:, -1:]], axis=1)


def mppi(score, seq, C, lam):
    """score [M C] float32, seq [H, M C, d] float32 -> (chosen [M, H, d] float64, bound)"""
    s, q = key(score).reshape(-1, C), f64(seq)
    H, MC, d = q.shape
    M = MC // C
    q = q.reshape(H, M, C, d)
    lam = float(np.float32(lam))
    chosen, bound = np.zeros((M, H, d)), np.zeros((M, H, d))
    depth = -(-C // 64) + min(C, 64)
    for m in range(M):
        s_max = s[m].max()
        if not np.isfinite(s_max):
            chosen[m] = q[:, m, 0]
            continue
        with np.errstate(invalid="ignore"):
            x = np.where(np.isfinite(s[m]), (s[m] - s_max) / lam, -np.inf)
        ax = np.where(np.isfinite(x), np.abs(x), 0.0)
        e_x = ax * ((1.0 + U) * (1.0 + C_DIV * U) - 1.0)
        w = np.exp(x)
        rel = EXP_REL + EXP_REL_F64
        with np.errstate(invalid="ignore", over="ignore"):
            e_w = np.where(np.isfinite(x), np.where(x - e_x < EXP_CUT, np.exp(x + e_x), w * (np.exp(e_x) * (1.0 + rel) - 1.0)), 0.0)
        Z = w.sum()
        e_Z = e_w.sum() + gamma(depth) * (w + e_w).sum()
        assert e_Z < Z
        A = np.einsum("c,hcd->hd", w, q[:, m])
        absq = np.abs(q[:, m])
        e_A = np.einsum("c,hcd->hd", e_w, absq) + gamma(C) * np.einsum("c,hcd->hd", w + e_w, absq)
        val = A / Z
        e_q = (e_A + np.abs(val) * e_Z) / (Z - e_Z)
        chosen[m] = np.clip(val, -1.0, 1.0)
        bound[m] = e_q + C_DIV * U * (np.abs(val) + e_q)
    return chosen, bound


def sequence(M, C, H, seed=0, p_done=0.15):
    """fabricated rewards [H, N] float32 (both signs, magnitudes over three decades), dones [H, N] uint8 and reward_end [N, 2] float32 (the
    second column is never to be read); candidate 0 of robot 0 never ends and the last candidate ends at step 0"""
    rng = np.random.default_rng(seed)
    N = M * (1 + C)
    rew = (rng.standard_normal((H, N)) * 10.0 ** rng.uniform(-2, 1, (H, N))).astype(np.float32)
    done = (rng.random((H, N)) < p_done).astype(np.uint8)
    done[:, M] = 0
    done[0, -1] = 1
    end = np.stack([rng.standard_normal(N) * 5.0, np.full(N, np.nan)], axis=1).astype(np.float32)
    return rew, done, end


def inputs(M, C, H, d, seed=0):
    """a plan [M, H, d] with entries at and beyond the clamp edges, and eps [H, M C, d]"""
    rng = np.random.default_rng(seed + 1000)
    plan = rng.uniform(-1.0, 1.0, (M, H, d)).astype(np.float32)
    flat = plan.reshape(-1)
    flat[0] = 1.0
    if flat.size > 1:
        flat[1] = -1.0
    eps = rng.standard_normal((H, M * C, d)).astype(np.float32)
    return plan, eps


def ratio(got, ref, bound):
    """the largest |got - ref| / bound (0 / 0 counts as 0)"""
    d = np.abs(f64(got) - f64(ref))
    b = np.broadcast_to(f64(bound), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / b)
    return float(np.max(r)) if r.size else 0.0
