"""Row sets for the many-rows contact solve (tests/test_rare_solver.py, tests/test_gpu_rare_solver.py), in the layout of
tests/hip/rare_probe.hip (see tests/rare_ref.py).

Synthetic sets are physically consistent: per leg an SPD 3 x 3 joint-space compliance K with u = K jq, the base side w = S (jb - B u) with
jb = (r x d, d) for a contact direction d at point r (0 for a limit row), diag = jq . u + |w|^2 and dinv = 1 / diag in float32 (as the
step computes them), friction rows carrying their normal's act.  The Delassus matrix is then a Gram matrix plus per-leg SPD blocks."""
import numpy as np

ROW = 16
PAY_W, PAY_RHS, PAY_DINV, PAY_DIAG, PAY_RB, PAY_MI, PAY_ACT = 0, 36, 42, 48, 54, 57, 58


def _spd(rng, n, scale):
    m = rng.normal(size=(n, n))
    return scale * (m @ m.T / n + 0.2 * np.eye(n))


def _put(rows, L, r, jq, u, w, rhs, act):
    f = np.float32
    q = rows[L, r]
    q[0:3], q[3:6], q[6:12] = jq, u, w
    jq32, u32, w32 = jq.astype(f), u.astype(f), w.astype(f)
    diag = f(jq32[0] * u32[0]) + f(jq32[1] * u32[1]) + f(jq32[2] * u32[2])
    for i in range(6):
        diag = f(diag + f(w32[i] * w32[i]))
    dinv = f(1.0) / max(diag, f(1e-30))
    q[12], q[13], q[14], q[15] = f(rhs) * dinv * f(act), dinv, act, diag


def synthetic(rng, limits=((), (), (), ()), points=((), (), (), ()), payload=False, near_dup=False, separating=0.25, mine=True):
    """One row set.  limits[K]: joints of leg K at their stop; points[K]: which contact points c (0 = the foot) of leg K touch;
    near_dup: the contact points of a leg are corners of one box 1e-3 apart (near-parallel rows); separating: the probability of a
    normal row with a negative rhs (its impulse ends at 0).  Returns (rows [4, 12, 16], env [2], warm [4], pay [59] or None)."""
    rows = np.zeros((4, 12, ROW), np.float32)
    S = _spd(rng, 6, 1.5)
    for K in range(4):
        Kc = _spd(rng, 3, 8.0)
        Bc = rng.normal(scale=0.3, size=(6, 3))
        axes = rng.normal(size=(3, 3)); axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        joints = rng.normal(scale=0.1, size=(3, 3))
        base = rng.normal(scale=0.2, size=3)
        for j in limits[K]:
            jq = np.zeros(3); jq[j] = rng.choice([-1.0, 1.0])
            u = Kc @ jq
            _put(rows, K, 9 + j, jq, u, S @ (-Bc @ u), rng.uniform(-0.2, 1.0), 1.0)
        for c in points[K]:
            r = base + (1e-3 * rng.choice([-1.0, 1.0], size=3) if near_dup else rng.normal(scale=0.1, size=3))
            nrm = np.array([0.0, 0.0, 1.0]) + (rng.normal(scale=1e-3, size=3) if near_dup else rng.normal(scale=0.2, size=3))
            nrm /= np.linalg.norm(nrm)
            t1 = np.cross(nrm, [1.0, 0.0, 0.0]); t1 /= np.linalg.norm(t1)
            t2 = np.cross(nrm, t1)
            for t, (d, rhs) in enumerate([(nrm, rng.uniform(-1.0, -0.1) if rng.random() < separating else rng.uniform(0.05, 1.0)),
                                          (t1, rng.normal(scale=0.5)), (t2, rng.normal(scale=0.5))]):
                jq = np.array([np.dot(np.cross(axes[i], r - joints[i]), d) for i in range(3)])
                u = Kc @ jq
                jb = np.concatenate([np.cross(r, d), d])
                _put(rows, K, 3 * c + t, jq, u, S @ (jb - Bc @ u), rhs, 1.0)
    pay = None
    if payload:
        pay = np.zeros(59, np.float32)
        pay[PAY_RB:PAY_RB + 3] = rng.normal(scale=0.1, size=3)
        pay[PAY_MI] = rng.uniform(20.0, 200.0)
        pay[PAY_ACT] = 1.0
        from rare_ref import pay_jacobian
        ja = pay_jacobian(pay[None, PAY_RB:PAY_RB + 3].astype(np.float64))[0]
        for k in range(6):
            w = (S @ rng.normal(scale=0.5, size=6)).astype(np.float32)
            pay[6 * k:6 * k + 6] = w
            diag = np.float32(np.dot(w.astype(np.float64), w) + pay[PAY_MI] * np.dot(ja[k], ja[k]))
            pay[PAY_DIAG + k] = diag
            pay[PAY_DINV + k] = np.float32(1.0) / diag
            pay[PAY_RHS + k] = np.float32(rng.normal(scale=0.3)) * pay[PAY_DINV + k]
    warm = np.array([rng.uniform(0.0, 0.3) * rows[K, 0, 13] if rows[K, 0, 14] > 0.5 else 0.0 for K in range(4)], np.float32)
    env = np.array([rng.uniform(0.3, 1.0), 1.0 if mine else 0.0], np.float32)
    return rows, env, warm, pay


def spread(rng, n, k, cap=3):
    """n items over k legs (at most cap each), at random"""
    out = [0] * k
    for _ in range(n):
        out[int(rng.choice([i for i in range(k) if out[i] < cap]))] += 1
    return out


def shape_set(rng, mA, mB, near_dup=False, separating=0.25):
    """a row set with mA region-A rows (limit rows, + 6 payload rows when mA >= 6 and it is 6 or 17 / 18 -- see below) and mB contact points.
    mA: 0, 1, 2, 11, 12 limit rows; 6 = payload only; 17 = 11 limits + payload; 18 = 12 limits + payload."""
    payload = mA in (6, 17, 18)
    n_lim = mA - 6 if payload else mA
    lim_per = spread(rng, n_lim, 4)
    pts_per = spread(rng, mB, 4)
    limits = [tuple(sorted(rng.choice(3, size=m, replace=False))) for m in lim_per]
    points = [tuple(sorted(rng.choice(3, size=m, replace=False))) for m in pts_per]
    return synthetic(rng, limits, points, payload, near_dup=near_dup, separating=separating)


def stack(sets):
    """list of row sets -> (rows [n, 4, 12, 16], env [n, 2], warm [n, 4], pay [n, 59] or None); sets without payload rows get act 0"""
    rows = np.stack([s[0] for s in sets]); env = np.stack([s[1] for s in sets]); warm = np.stack([s[2] for s in sets])
    if all(s[3] is None for s in sets):
        return rows, env, warm, None
    pay = np.stack([s[3] if s[3] is not None else np.zeros(59, np.float32) for s in sets])
    return rows, env, warm, pay


def empty():
    """no rows, mine unset"""
    return np.zeros((4, 12, ROW), np.float32), np.zeros(2, np.float32), np.zeros(4, np.float32), None


def counts(rows, pay):
    """(mA, mB) of each set"""
    mA = (rows[:, :, 9:12, 14] > 0.5).sum((1, 2)) + (0 if pay is None else 6 * (pay[:, PAY_ACT] > 0.5))
    mB = (rows[:, :, 0:9:3, 14] > 0.5).sum((1, 2))
    return mA, mB


def captured(kind, model="pyramid", thr=0.0, max_sets=256):
    """row sets captured from the host emulation's many-rows solves (emu.RareCapture) while it steps: "thrown" -- robots dropped on trunk,
    hips and thighs; "stop" -- the same robots with calves, hips and thighs driven into their joint stops; "payload" -- payload="soft" robots thrown
    on their side.  Returns (cfg, rows, env, warm, pay)."""
    from emu.emu import Emu, RareCapture
    from qs_amd.config import build_config
    kw = dict(n_envs=16, noise=False, isRLGymInterface=False, motor_control_mode="TORQUE", task_env="NO_TASK", observation_space_mode="ENCODER",
              enable_action_filter=False, enable_springs=False, friction_model=model, solver_residual_threshold=thr, settle_steps=50)
    if kind == "payload":
        kw.update(payload="soft", env_randomizer_mode="MASS_RANDOMIZER", seed=3)
    else:
        kw.update(env_randomizer_mode="NONE")
    cfg, _ = build_config(**kw)
    e = Emu(cfg)
    e.reset()
    rng = np.random.default_rng({"thrown": 1, "stop": 2, "payload": 3}[kind])
    s = e.get_state()
    from scipy.spatial.transform import Rotation as Rot
    s[:, :3] = [0.0, 0.0, 0.22]
    s[:, 3:7] = Rot.from_euler("xyz", np.stack([rng.choice([1.45, -1.45, 3.0, 0.7], 16), rng.uniform(-0.5, 0.5, 16), np.zeros(16)], 1)).as_quat()
    s[:, 7:] = 0.0
    s[:, 9] = -1.0                                   # thrown at the floor
    s[:, 13:25] = np.tile([0.0, 1.2, -2.4], 4)
    e.set_state(s)
    with RareCapture(max_sets) as cap:
        for i in range(6):
            tau = 2.0 * rng.normal(size=(16, 12)).astype(np.float32)
            if kind == "stop":
                tau[:, 2::3] = -30.0
                if i >= 3:
                    tau[:, 0::3] = np.array([-20.0, 20.0, -20.0, 20.0], np.float32); tau[:, 1::3] = -20.0
            e.step(tau)
    n = (len(cap.rows) // 16) * 16
    pay = cap.pay[:n] if cap.has_pay[:n].any() else None
    return cfg, cap.rows[:n], cap.env[:n], cap.warm[:n], pay
