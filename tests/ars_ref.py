"""Float64 restatement of ARS's bookkeeping on the device (csrc/qs_ars.h, steps 1-6) and the bounds a float32 evaluation in the header's order
is held to (TEST INFRASTRUCTURE; shared by tests/test_ars_cpu.py and tests/test_gpu_ars.py).

Every bound counts the roundings of the header's sequence with u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1: a chain of n additions or fused multiply-adds is within gamma_n x the sum of the absolute terms).  The
inputs of each step are float32 numbers and enter the float64 restatement exactly.  No constant is measured.
  perturb   one fmaf per element:                                    |d cand|  <= u |theta +- sigma delta|
  account   T plain additions in step order:                         |d ret|   <= gamma_T sum_t |r_t|  over the steps the environment was alive; len, episodes, alive, n_alive are integers: equal
  returns   term_e = fmaf(bonus, len_e, ret_e): one rounding; lane chain of ceil(m / 64) additions, then at most 64 lane sums:
                                                                     |d R_p|   <= gamma_(ceil(m / 64) + min(m, 64) + 1) sum_e |term_e|
  select    score, rank, idx are comparisons of float32 numbers: EQUAL.  w_r = R+ - R-: one rounding of the exact difference, so EQUAL to the
            float64 difference rounded to float32.  With n = 2b values v and S = sum |v_i|:
              mean:  n - 1 additions, one division             e_mean = gamma_n S / n
              d_i = v_i - mean: one subtraction                e_d_i  = e_mean + u (|d_i| + e_mean)
              ss:    n fmafs on the rounded d                  e_ss   = gamma_n sum (|d_i| + e_d_i)^2 + sum e_d_i (2 |d_i| + e_d_i)
              q = ss / (n - 1): one division                   e_q    = e_ss / (n - 1) + C u q
              std = sqrtf(q):  |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|)
                                                               e_std  = min(e_q / sqrt q, sqrt e_q) + C u (std + that)
              den = fmaf(b, std, 1e-6f): one rounding          e_den  = b e_std + u den
              step = lr / den                                  e_step = lr e_den / (den (den - e_den)) + C u step
            C = 2: sqrtf and the float32 division are documented as within 1 ulp = 2 u on the device (HIP's math tables; both are
            correctly rounded on the host, and are on the device as the library is built -- the tests record which, they do not rely on it).
  apply     g_i: b fmafs                                             e_g_i     = gamma_b sum_r |w_r delta[idx_r][i]|
            theta_i' = fmaf(step, g_i, theta_i): one rounding        |d theta_i'| <= e_step (|g_i| + e_g_i) + step e_g_i + u (|theta_i'| + those)
"""
import numpy as np

U = 2.0 ** -24
C_LIBM = 2.0          # sqrtf and division: within 1 ulp = 2 u
EPS_DEN = float(np.float32(1e-6))
# (m, n_delta, n_top, n_params): every value of tests/test_gpu_ars.py's lists at least once
SHAPES = [(1, 1, 1, 1), (3, 5, 2, 168), (64, 2, 1, 255), (65, 5, 5, 256), (130, 2, 2, 257), (3, 64, 16, 6406), (1, 65, 33, 168), (1, 1024, 1, 1),
          (1, 1024, 300, 257), (3, 1024, 1024, 6406)]


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(x):
    return np.asarray(x, np.float64)


def perturb(theta, delta, sigma):
    """-> (cand [2 n_delta, n_params] float64, bound)"""
    th, d, s = f64(theta), f64(delta), float(np.float32(sigma))
    cand = np.concatenate([th + s * d, th - s * d], 0)
    return cand, U * np.abs(cand)


def account(rewards, dones, episodes_per_env=1):
    """rewards [T, N] float32, dones [T, N] -> per step t a dict(ret float64 [N], len, episodes, alive, n_alive, bound [N]) AFTER step t"""
    r, d = f64(rewards), np.asarray(dones).astype(bool)
    T, N = r.shape
    ret, mag = np.zeros(N), np.zeros(N)
    length, episodes, alive = np.zeros(N, np.int64), np.zeros(N, np.int64), np.ones(N, bool)
    out = []
    for t in range(T):
        ret = np.where(alive, ret + r[t], ret)
        mag = np.where(alive, mag + np.abs(r[t]), mag)
        length = length + alive
        episodes = episodes + (alive & d[t])
        alive = alive & ~(d[t] & (episodes >= episodes_per_env))
        out.append(dict(ret=ret.copy(), len=length.copy(), episodes=episodes.copy(), alive=alive.copy(), n_alive=int(alive.sum()),
                        bound=gamma(np.maximum(length, 1)) * mag))
    return out


def returns(ret, length, n_delta, alive_bonus_offset=0.0):
    """ret [N] float32, len [N] -> (R [2 n_delta] float64, the sum of all lengths, bound [2 n_delta])"""
    P = 2 * int(n_delta)
    term = float(np.float32(alive_bonus_offset)) * f64(length) + f64(ret)
    m = term.size // P
    term = term.reshape(P, m)
    depth = -(-m // 64) + min(m, 64) + 1
    return term.sum(1), int(np.asarray(length, np.int64).sum()), gamma(depth) * np.abs(term).sum(1)


def select(R, n_top, lr):
    """R [2 n_delta] float32 -> dict(idx, w (float64), std, step, e_std, e_step): the stated ranking (ties: lower index first)"""
    R = f64(R)
    n_delta, b = R.size // 2, int(n_top)
    rp, rm = R[:n_delta], R[n_delta:]
    score = np.maximum(rp, rm)
    k = np.arange(n_delta)
    rank = ((score[None, :] > score[:, None]) | ((score[None, :] == score[:, None]) & (k[None, :] < k[:, None]))).sum(1)
    idx = np.empty(b, np.int64)
    keep = rank < b
    idx[rank[keep]] = k[keep]
    v = np.concatenate([rp[idx], rm[idx]])
    n = 2 * b
    S = np.abs(v).sum()
    mean = v.sum() / n
    d = v - mean
    q = (d * d).sum() / (n - 1)
    std = np.sqrt(q)
    lr = float(np.float32(lr))
    den = b * std + EPS_DEN
    step = lr / den
    e_mean = gamma(n) * S / n
    e_d = e_mean + U * (np.abs(d) + e_mean)
    e_ss = gamma(n) * ((np.abs(d) + e_d) ** 2).sum() + (e_d * (2.0 * np.abs(d) + e_d)).sum()
    e_q = e_ss / (n - 1) + C_LIBM * U * q
    e_sqrt = min(e_q / np.sqrt(q), np.sqrt(e_q)) if q > 0.0 else np.sqrt(e_q)
    e_std = e_sqrt + C_LIBM * U * (std + e_sqrt)
    e_den = b * e_std + U * (den + b * e_std)
    e_step = lr * e_den / (den * (den - e_den)) + C_LIBM * U * step if e_den < den else np.inf
    return dict(idx=idx, w=rp[idx] - rm[idx], std=std, step=step, e_std=e_std, e_step=e_step)


def apply(theta, delta, idx, w, step, e_step=0.0):
    """-> (theta' float64, bound); w and step in float64 (step with its bound e_step), delta and theta float32 inputs"""
    th, rows, w = f64(theta), f64(delta)[np.asarray(idx, np.int64)], f64(w)
    g = w @ rows
    e_g = gamma(len(w)) * (np.abs(w) @ np.abs(rows))
    new = th + step * g
    e = e_step * (np.abs(g) + e_g) + abs(step) * e_g
    return new, e + U * (np.abs(new) + e)


def sequence(n_envs, steps=12, seed=0, p_done=0.15):
    """fabricated rewards [T, N] float32 (both signs, magnitudes over three decades) and dones [T, N] uint8; environment 0 never ends and
    environment N - 1 ends at step 1"""
    rng = np.random.default_rng(seed)
    rew = (rng.standard_normal((steps, n_envs)) * 10.0 ** rng.uniform(-2, 1, (steps, n_envs))).astype(np.float32)
    done = (rng.random((steps, n_envs)) < p_done).astype(np.uint8)
    done[:, 0] = 0
    done[0, -1] = 1
    return rew, done


def tied_returns(n_delta, n_top, seed=0):
    """R [2 n_delta] float32, integer-valued, with duplicated scores on both sides of the n_top cut (n_delta >= 3) and no two directions equal
    in both returns' order otherwise"""
    rng = np.random.default_rng(seed)
    rp = rng.permutation(n_delta).astype(np.float32) * 2.0 + 10.0
    rm = rp - rng.integers(1, 9, n_delta).astype(np.float32)
    if n_delta >= 3:
        order = np.argsort(-np.maximum(rp, rm), kind="stable")
        cut = min(max(n_top, 1), n_delta - 1)
        a, b = order[cut - 1], order[cut]                       # the last kept and the first dropped direction: make them tie
        rp[b] = rp[a]
        if cut >= 2:
            rm[order[cut - 2]] = rp[a]                           # and a third whose score comes from its minus side: max(rp, rm) ties as well
            rp[order[cut - 2]] = rp[a] - 3.0
    return np.concatenate([rp, rm]).astype(np.float32)


def ratio(got, ref, bound):
    """the largest |got - ref| / bound (0 / 0 counts as 0)"""
    d = np.abs(f64(got) - f64(ref))
    b = np.broadcast_to(f64(bound), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / b)
    return float(np.max(r)) if r.size else 0.0
