"""Plain impulse-space PGS for the many-rows contact solve, written from the contract in qs_rare.h's header comment and RarePos (not from
either C++ version of it), vectorised over environments, in float64 by default.

Row sets come in the layout of tests/hip/rare_probe.hip: rows [n, 4, 12, 16] (per leg K its twelve Rows: contact point c at 3 c (normal),
3 c + 1, 3 c + 2 (friction), joint limits at 9 + j; a Row is jq 3, u 3, w 6, rhs, dinv, act, diag), env [n, 2] (mu, mine), warm [n, 4],
pay [n, 59] (w 36, rhs 6, dinv 6, diag 6, rB 3, mI, act) or None.

The 54 positions in sweep order: 0..11 joint limits (3 K + j), 12..17 payload rows, 18..29 normals (18 + 3 K + c), 30..53 friction pairs
(30 + 6 K + 2 c + t).  A row's group is its leg, 4 for the payload rows; A'[j][p] = -dinv_p (w_j . w_p + [grp_j = grp_p] a_j . b_p), no self
term, a = jq and b = u for the legs' rows."""
import numpy as np

N, PAY0, NRM0, FRI0 = 54, 12, 18, 30
BIG = 1e10


def positions():
    """(leg, row) of each position; leg 4 / row k for the payload rows"""
    out = []
    for p in range(N):
        if p < PAY0:
            out.append((p // 3, 9 + p % 3))
        elif p < NRM0:
            out.append((4, p - PAY0))
        elif p < FRI0:
            q = p - NRM0
            out.append((q // 3, 3 * (q % 3)))
        else:
            q = p - FRI0
            out.append((q // 6, 3 * ((q % 6) // 2) + 1 + q % 2))
    return out


POS = positions()


def pay_jacobian(rB):
    """[n, 6, 3]: the payload rows' a (the block's angular Jacobian: -(rB x e_k) for k < 3, -e_k - 3 after)"""
    n = rB.shape[0]
    a = np.zeros((n, 6, 3), rB.dtype)
    rx, ry, rz = rB[:, 0], rB[:, 1], rB[:, 2]
    a[:, 0, 1], a[:, 0, 2] = -rz, ry
    a[:, 1, 0], a[:, 1, 2] = rz, -rx
    a[:, 2, 0], a[:, 2, 1] = -ry, rx
    a[:, 3, 0] = a[:, 4, 1] = a[:, 5, 2] = -1.0
    return a


def unpack(rows, env, pay, dtype=np.float64):
    """per position: w [n, 54, 6], a, b [n, 54, 3], rhs, dinv, diag [n, 54], live [n, 54], grp [54]"""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    w, a, b = np.zeros((n, N, 6), dtype), np.zeros((n, N, 3), dtype), np.zeros((n, N, 3), dtype)
    rhs, dinv, diag = np.zeros((n, N), dtype), np.zeros((n, N), dtype), np.zeros((n, N), dtype)
    live = np.zeros((n, N), bool)
    grp = np.array([L for L, _ in POS])
    for p, (L, r) in enumerate(POS):
        if L == 4:
            continue
        q = rows[:, L, r]
        w[:, p], a[:, p], b[:, p] = q[:, 6:12], q[:, 0:3], q[:, 3:6]
        rhs[:, p], dinv[:, p], diag[:, p] = q[:, 12], q[:, 13], q[:, 15]
        # a friction row exists with its contact point: it carries the normal's act (the normal of row 3 c + 1 + t is row 3 c)
        act = rows[:, L, 3 * (r // 3), 14] if r < 9 else q[:, 14]
        live[:, p] = act > 0.5
    if pay is not None:
        pay = np.asarray(pay, np.float32)
        ja = pay_jacobian(pay[:, 54:57].astype(dtype))
        for k in range(6):
            p = PAY0 + k
            w[:, p] = pay[:, 6 * k:6 * k + 6]
            a[:, p] = ja[:, k]
            b[:, p] = ja[:, k] * pay[:, 57:58].astype(dtype)
            rhs[:, p], dinv[:, p], diag[:, p] = pay[:, 36 + k], pay[:, 42 + k], pay[:, 48 + k]
            live[:, p] = pay[:, 58] > 0.5
    mine = np.asarray(env)[:, 1] > 0.5
    live &= mine[:, None]
    return w, a, b, rhs, dinv, diag, live, grp


def delassus(w, a, b, dinv, live, grp):
    """A' [n, j, p] as in the module docstring (zero for rows that do not exist and on the diagonal)"""
    same = grp[:, None] == grp[None, :]
    A = np.einsum("nji,npi->njp", w, w) + same[None] * np.einsum("nji,npi->njp", a, b)
    A = -dinv[:, None, :] * A
    A = A * (live[:, :, None] & live[:, None, :])
    A[:, np.arange(N), np.arange(N)] = 0.0
    return A


def solve(cfg, rows, env, warm, pay=None, dtype=np.float64, iters=None, threshold=None, cone=None):
    """-> lam12 [n, 4, 12], plam [n, 6], sweeps [n] (how many ran), resid [n, iters] (each sweep's largest |dlam x diag| over the live rows;
    NaN after the exit).  cfg gives solver_iters, solver_residual_threshold, dt and friction_cone unless overridden."""
    iters = cfg.solver_iters if iters is None else iters
    threshold = cfg.solver_residual_threshold if threshold is None else threshold
    cone = bool(cfg.friction_cone) if cone is None else cone
    w, a, b, rhs, dinv, diag, live, grp = unpack(rows, env, pay, dtype)
    n = w.shape[0]
    A = delassus(w, a, b, dinv, live, grp)
    mu = np.asarray(env, dtype)[:, 0]
    bound = dtype(500.0) * dtype(cfg.dt)
    lam = np.zeros((n, N), dtype)
    for K in range(4):
        p = NRM0 + 3 * K
        lam[:, p] = np.where(live[:, p], np.asarray(warm, dtype)[:, K], 0.0)
    lo = np.zeros(N, dtype); hi = np.full(N, BIG, dtype)
    lo[PAY0:NRM0], hi[PAY0:NRM0] = -bound, bound
    any_live = live.any(0)
    running = np.ones(n, bool)
    sweeps = np.zeros(n, np.int64)
    resid = np.full((n, iters), np.nan)
    thr = np.sqrt(threshold)

    def cand(p):
        return rhs[:, p] + np.einsum("nj,nj->n", A[:, :, p], lam)

    def put(p, v, m):
        lam[:, p] = np.where(m & live[:, p], v, lam[:, p])

    for it in range(iters):
        if not running.any():
            break
        lam_in = lam.copy()
        region_a = range(NRM0) if it & 1 else range(NRM0 - 1, -1, -1)
        for p in list(region_a) + list(range(NRM0, FRI0)):
            if any_live[p]:
                put(p, np.clip(cand(p), lo[p], hi[p]), running)
        for f in range(FRI0, N, 2):
            if not any_live[f]:
                continue
            L, r = POS[f]
            ln = lam[:, NRM0 + 3 * L + (r - 1) // 3]
            lim = mu * ln
            if cone:
                ca, cb = cand(f), cand(f + 1)
                r2 = np.sqrt(ca * ca + cb * cb)
                sc = np.where(r2 > lim, lim / np.where(r2 > 0, r2, 1.0), 1.0)
                put(f, ca * sc, running); put(f + 1, cb * sc, running)
            else:
                m = running & (ln > 0)
                put(f, np.clip(cand(f), -lim, lim), m)
                put(f + 1, np.clip(cand(f + 1), -lim, lim), m)
        r_it = np.where(live, np.abs((lam - lam_in) * diag), 0.0).max(1)
        resid[running, it] = r_it[running]
        sweeps += running
        if threshold > 0:
            running &= r_it > thr
    lam12 = np.zeros((n, 4, 12), dtype)
    for p, (L, r) in enumerate(POS):
        if L < 4:
            lam12[:, L, r] = lam[:, p]
    return lam12, lam[:, PAY0:NRM0].copy(), sweeps, resid
