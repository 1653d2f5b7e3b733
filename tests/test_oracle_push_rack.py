"""Known answers for the oracle's restatement of external pushes (qso_set_external_wrench) and of the rack (qso_create_ex / qso_set_rack):
momentum and angular-momentum balances in free flight, the push's velocity change against the independent CRBA mass matrix, force and
moment balances of a robot standing under a push, hanging from the rack and hanging with its feet on the floor, the rack's one-substep
answer against a float64 PGS, the push's duration across env steps, and a release and re-hang.  Analytic: no GPU, no emulation.  The
emulation and the kernels are held to this oracle (test_emu_push.py, test_emu_rack.py, test_gpu_push.py, test_gpu_rack.py)."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle.qso import Oracle
from qs_amd.config import build_config
from test_emu_push import C_TRUNK, RAW, base_velocities
from test_emu_rack import ANCHORS, airborne_near_anchor, pgs, rack_jacobian

DT = 0.001
G = 9.8
ANCHOR = ANCHORS["identity"]
PHYS = dict(action_repeat=1, self_collision=False, body_contacts=False, noise=False, env_randomizer_mode="NONE", **RAW)


def tumbling(dt, seed):
    """one robot in the air, gravity off, spinning at up to 8 rad/s with moving legs; the constant joint torques of the run"""
    cfg, _ = build_config(n_envs=1, time_step=dt, **PHYS)
    o = Oracle(cfg)
    o.set_gravity(0.0)
    rng = np.random.default_rng(seed)
    s = o.get_state()
    s[:, :3] = [0.0, 0.0, 1.0]
    s[:, 3:7] = Rotation.random(1, random_state=seed).as_quat()
    s[:, 7:10] = rng.uniform(-0.5, 0.5, 3)
    s[:, 10:13] = rng.uniform(-1, 1, 3) * 8.0
    s[:, 13:25] = np.tile([0.0, 0.8, -1.6], 4)
    s[:, 25:37] = rng.uniform(-2, 2, 12)
    o.set_state(s)
    return o, rng.uniform(-2, 2, 12)


def momentum_defect(dt, n, frame, F, T, seed):
    """`n` substeps of `dt` under the push: (measured change of p, L) - (sum over the substeps of dt F_k, dt (r_k x F_k + tau_k)) with the
    trunk's inertial origin r_k and the orientation R_k taken from the state each substep starts from; the largest rate met
    (|base angular velocity| + fastest joint), the largest |p| and |L|, the expected changes"""
    o, tau = tumbling(dt, seed)
    o.set_external_wrench(np.concatenate([F, T]), n, frame)
    e0 = o.energy(0)
    dp, dL, rate, pmax, lmax = np.zeros(3), np.zeros(3), 0.0, 0.0, 0.0
    for _ in range(n):
        st = o.get_state()[0]
        R = Rotation.from_quat(st[3:7]).as_matrix()
        Fw, Tw = (F, T) if frame == "world" else (R @ F, R @ T)
        dp += dt * Fw
        dL += dt * (np.cross(st[:3] + R @ C_TRUNK, Fw) + Tw)
        rate = max(rate, np.linalg.norm(st[10:13]) + np.abs(st[25:37]).max())
        e = o.energy(0)
        pmax, lmax = max(pmax, np.linalg.norm(e["p"])), max(lmax, np.linalg.norm(e["L"]))
        o.phys_step(0, tau)
    e1 = o.energy(0)
    assert o.get_info(14)[0, 6] == 0
    o.close()
    return (e1["p"] - e0["p"]) - dp, (e1["L"] - e0["L"]) - dL, rate, pmax + np.linalg.norm(dp), lmax + np.linalg.norm(dL), dp, dL


F_PUSH, T_PUSH = np.array([40.0, -25.0, 60.0]), np.array([3.0, -2.0, 1.5])


@pytest.mark.parametrize("frame", ["world", "link"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_push_in_free_flight_balances_momentum(seed, frame):
    """Gravity off, tumbling robot, constant joint torques, F and tau for 40 substeps: Delta p = sum dt F_k, Delta L (about the world origin)
    = sum dt (r_k x F_k + tau_k); world frame: F_k = F (so Delta p = 40 dt F exactly), link frame: F_k = R_k F.

    The step is semi-implicit Euler: the velocities change by dt x the accelerations of the configuration the substep starts from (the
    balance holds exactly there: p and L are linear in the velocities), then the configuration moves on with the velocities held, which
    changes p and L by second-order terms that add up to a defect of FIRST order in dt.  So: (1) the defect of the run is within
    dt x rate x (|p| + |Delta p|) -- rate = the fastest turning met, |base angular velocity| + fastest joint: the configuration turns by
    dt x rate per substep, and so does what it carries; (2) the same time span in substeps of dt / 2 halves the defect (ratio within
    0.4 .. 0.6); (3) Richardson's 2 defect(dt / 2) - defect(dt), which cancels the first order, is within (dt x rate)^2 x (|p| + |Delta p|):
    this is the test's tolerance, measured at 1e-5 .. 7e-5 of |Delta p| here.  Link frame: the world-frame expectation 40 dt F lies at
    least 50 x that tolerance away (measured: 2.4 .. 3.3 N s against 2e-3 .. 4e-3), so the case tells the frames apart."""
    n = 40
    a = momentum_defect(DT, n, frame, F_PUSH, T_PUSH, seed)
    b = momentum_defect(DT / 2, 2 * n, frame, F_PUSH, T_PUSH, seed)
    rate = max(a[2], b[2])
    for name, ea, eb, scale in (("p", a[0], b[0], max(a[3], b[3])), ("L", a[1], b[1], max(a[4], b[4]))):
        first, second = DT * rate * scale, (DT * rate) ** 2 * scale
        print(f"{frame} seed {seed} {name}: defect(dt) {np.abs(ea).max():.3e} defect(dt/2) {np.abs(eb).max():.3e} extrapolated "
              f"{np.abs(2 * eb - ea).max():.3e}; rate {rate:.1f} rad/s, bounds {first:.3e} {second:.3e}")
        assert np.abs(ea).max() <= first, (name, ea, first)
        big = np.abs(ea) > 0.1 * np.abs(ea).max()
        assert big.any() and np.all((eb[big] / ea[big] > 0.4) & (eb[big] / ea[big] < 0.6)), (name, ea, eb)
        assert np.abs(2 * eb - ea).max() <= second, (name, 2 * eb - ea, second)
    if frame == "world":
        np.testing.assert_allclose(a[5], n * DT * F_PUSH, rtol=0, atol=1e-13)
    else:
        second = (DT * rate) ** 2 * max(a[3], b[3])
        assert np.abs(a[5] - n * DT * F_PUSH).max() >= 50 * second, (a[5], n * DT * F_PUSH, second)


@pytest.mark.parametrize("frame", ["world", "link"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_push_against_the_crba_mass_matrix(seed, frame):
    """one substep, no contact, joint torques and velocities: v(push) - v(no push) = dt H^-1 [c x F_b + tau_b ; F_b ; 0] with H from the
    independent CRBA (the oracle's step is ABA with the wrench as a spatial force on body 0).  float64 and a linear relation: 1e-9 of
    the largest entry.  The expectation without the lever arm c x F_b must miss by at least 1e4 x that."""
    cases = [((40.0, -25.0, 60.0), (0, 0, 0)), ((0, 0, 0), (3.0, -2.0, 1.5)), ((-30.0, 50.0, 10.0), (1.0, 2.0, -1.0))]
    n = len(cases)
    cfg, _ = build_config(n_envs=n, time_step=DT, **PHYS)
    rng = np.random.default_rng(seed)
    a, b = Oracle(cfg), Oracle(cfg)
    s = a.get_state()
    s[:, :3] = [0.0, 0.0, 1.0]
    s[:, 3:7] = Rotation.random(n, random_state=seed).as_quat()
    s[:, 7:13] = rng.uniform(-0.5, 0.5, (n, 6))
    s[:, 13:25] = np.tile([0.0, 0.8, -1.6], 4)
    s[:, 25:37] = rng.uniform(-0.5, 0.5, (n, 12))
    a.set_state(s); b.set_state(s)
    a.set_external_wrench(np.array([np.concatenate(c) for c in cases]), 1, frame)
    for i in range(n):
        tau = rng.uniform(-3, 3, 12)
        a.phys_step(i, tau); b.phys_step(i, tau)
    _, R0 = base_velocities(s)
    sa, sb = a.get_state(), b.get_state()
    dv = np.concatenate([np.einsum("nji,nj->ni", R0, sa[:, 10:13] - sb[:, 10:13]), np.einsum("nji,nj->ni", R0, sa[:, 7:10] - sb[:, 7:10]),
                         sa[:, 25:37] - sb[:, 25:37]], 1)
    b.set_state(s)
    for i, (F, T) in enumerate(cases):
        F, T = np.asarray(F, np.float64), np.asarray(T, np.float64)
        Fb, Tb = (R0[i].T @ F, R0[i].T @ T) if frame == "world" else (F, T)
        H, _ = b.crba_rnea(i)
        want = DT * np.linalg.solve(H, np.concatenate([np.cross(C_TRUNK, Fb) + Tb, Fb, np.zeros(12)]))
        tol = 1e-9 * np.abs(want).max()
        assert np.abs(dv[i] - want).max() < tol, (i, np.abs(dv[i] - want).max(), tol)
        if np.any(F):
            no_lever = DT * np.linalg.solve(H, np.concatenate([Tb, Fb, np.zeros(12)]))
            assert np.abs(dv[i] - no_lever).max() > 1e4 * tol, (i, np.abs(dv[i] - no_lever).max(), tol)


STAND = dict(task_env="NO_TASK", observation_space_mode="ENCODER", isRLGymInterface=False, motor_control_mode="PD", noise=False,
             env_randomizer_mode="NONE", enable_action_filter=False)


def test_push_on_a_standing_robot_loads_the_feet():
    """Standing under PD (springs on), then a constant world push (0, 0, -30 N) for 300 substeps.  Over every substep the feet, gravity
    and the push change the momentum: sum of foot forces = m g + F_z + Delta p_z / dt (floor normal = z; exact but for the second-order
    terms of the configuration update, which vanish with the velocities: asserted to 1e-3 m g = 0.4 % of the push, before, during and
    after it).  The step load leaves the robot bouncing on its sprung legs (1.7 Hz, lightly damped: +-5.6 N after 0.2 s), so the plain
    rise of the load is taken between means over 200 substeps: F_z to 10 % (measured 3 %); once the push has run out the load goes back."""
    fz = 30.0
    cfg, _ = build_config(n_envs=1, time_step=DT, action_repeat=1, **STAND)
    o = Oracle(cfg)
    o.reset()
    act = np.asarray(cfg.settle_cmd, np.float32)[None, :cfg.action_dim]
    mg = o.crba_rnea(0)[0][3, 3] * G
    feet = []
    for k in range(900):
        if k == 300:
            o.set_external_wrench([0, 0, -fz, 0, 0, 0], 300, "world")
        p0 = o.energy(0)["p"][2]
        o.step(act)
        rate = (o.energy(0)["p"][2] - p0) / DT
        feet.append(o.get_info(0).sum())
        push = fz if 300 <= k < 600 else 0.0
        assert abs(feet[-1] - (mg + push + rate)) < 1e-3 * mg, (k, feet[-1], mg + push + rate)
        assert o.get_info(14)[0, 6] == (599 - k if 300 <= k < 600 else 0)
    feet = np.array(feet)
    before, during, after = feet[100:300].mean(), feet[400:600].mean(), feet[700:900].mean()
    np.testing.assert_allclose(before, mg, rtol=0.01)
    np.testing.assert_allclose(during - before, fz, rtol=0.10)
    np.testing.assert_allclose(after, before, atol=0.10 * fz)


@pytest.mark.parametrize("repeat", [10, 4])
def test_push_duration_across_env_steps(repeat):
    """a push of 25 substeps: the remaining count after each env step reads max(0, 25 - substeps run); the trajectory is that of pushes
    re-issued before every step for the substeps that fall into it, bit for bit; a reset in between cancels it"""
    n = 3
    cfg, _ = build_config(n_envs=n, time_step=DT, action_repeat=repeat, settle_steps=300, **STAND)
    a, b, c = Oracle(cfg), Oracle(cfg), Oracle(cfg)
    for o in (a, b, c):
        o.reset()
    rng = np.random.default_rng(repeat)
    w = np.concatenate([rng.uniform(-150, 150, (n, 3)), rng.uniform(-8, 8, (n, 3))], 1)
    a.set_external_wrench(w, 25, "world")
    steps = 25 // repeat + 3
    for t in range(steps):
        left = max(0, 25 - t * repeat)
        np.testing.assert_array_equal(a.get_info(14)[:, 6], left)
        np.testing.assert_array_equal(a.get_info(14)[:, :6], w)
        assert np.all(a.get_info(14)[:, 7] == 2)
        b.set_external_wrench(w, min(left, repeat), "world")
        act = (np.asarray(cfg.settle_cmd)[None, :] + rng.uniform(-0.1, 0.1, (n, 12))).astype(np.float32)
        ra, rb = a.step(act), b.step(act)
        np.testing.assert_array_equal(a.get_state(), b.get_state())
        np.testing.assert_array_equal(ra[0], rb[0])
        if t == 0:
            c.step(act)
            assert np.abs(c.get_state() - a.get_state()).max() > 1e-4      # (the push does act)
    assert np.all(a.get_info(14)[:, 6] == 0)
    # a reset cancels: set_state keeps it
    a.set_external_wrench(w, 25, "link")
    a.step(act)
    a.set_state(a.get_state())
    assert np.all(a.get_info(14)[:, 6] == 25 - repeat) and np.all(a.get_info(14)[:, 7] == 1)
    m = np.array([1, 0, 1], np.uint8)
    a.reset(m); c.reset()
    assert a.get_info(14)[:, 6].tolist() == [0, 25 - repeat, 0]
    a.reset_to(a.get_state(), np.array([0, 1, 0], np.uint8))
    assert np.all(a.get_info(14)[:, 6] == 0)
    a.reset(); a.step(act); c.step(act)
    np.testing.assert_array_equal(a.get_state(), c.get_state())
    # a settle never sees a push, and does not count it down: a push set before nothing but resets... is cancelled by them; refused rows
    a.set_external_wrench(w, 7, "world")
    bad = w.copy(); bad[1, 2] = np.nan
    with pytest.raises(RuntimeError, match="environment 1"):
        a.set_external_wrench(bad, 3, "link")
    assert a.get_info(14)[:, 6].tolist() == [3, 7, 3] and a.get_info(14)[:, 7].tolist() == [1, 2, 1]
    with pytest.raises(RuntimeError, match="environment 0"):
        a.set_external_wrench(w, np.array([-1, 2, 2], np.int32), "world")
    assert a.get_info(14)[:, 6].tolist() == [3, 2, 2]
    with pytest.raises(RuntimeError, match="frame"):
        a.set_external_wrench(w, 1, 3)
    a.set_external_wrench(w, 0, "world")
    assert np.all(a.get_info(14)[:, 6] == 0)


@pytest.mark.parametrize("auto_reset", [True, False])
def test_the_end_of_the_episode_cancels_the_push(auto_reset):
    """the step in which the episode ends leaves no push behind, whether it resets the environment itself (auto_reset) or leaves that to
    the caller; the neighbour's push counts on"""
    cfg, _ = build_config(n_envs=2, time_step=DT, settle_steps=100, task_env="JUMPING_IN_PLACE", noise=False, env_randomizer_mode="NONE", auto_reset=auto_reset)
    o = Oracle(cfg)
    o.reset()
    o.set_external_wrench([[0, 500.0, 0, 80.0, 0, 0], [0, 0, 1.0, 0, 0, 0]], np.array([100000, 100000], np.int32), "world")     # throws env 0 over
    for t in range(200):
        _, _, done, _ = o.step(np.zeros((2, cfg.action_dim), np.float32))
        if done[0]:
            break
    assert done[0] and not done[1], t
    assert o.get_info(14)[:, 6].tolist() == [0, 100000 - (t + 1) * cfg.action_repeat]
    assert (o.get_info(7)[0, 0] == 0) == auto_reset


# ---------------------------------------------------------------------------------------------------------------- the rack
def rack_cfg(n, **kw):
    return build_config(n_envs=n, noise=False, task_env="NO_TASK", on_rack=True, **{"env_randomizer_mode": "NONE", **kw})


def test_rack_refusals():
    cfg, meta = rack_cfg(1)
    for bad in ([0, 0, 1, 0, 0, 0, 0], [0, 0, 1, np.nan, 0, 0, 1], [np.inf, 0, 1, 0, 0, 0, 1]):
        with pytest.raises(RuntimeError, match="anchor"):
            Oracle(cfg, rack=bad)
    soft, _ = build_config(n_envs=1, payload="soft", env_randomizer_mode="MASS_RANDOMIZER")
    with pytest.raises(RuntimeError, match="payload_soft"):
        Oracle(soft, rack=True)
    plain = Oracle(cfg)
    with pytest.raises(RuntimeError, match="no rack"):
        plain.set_rack(False)
    with pytest.raises(RuntimeError, match="no rack"):
        plain.get_info(15)
    o = Oracle(cfg, rack=[0.5, 0, 1, 0, 0, 3.0, 4.0])       # normalised
    o.reset()
    np.testing.assert_allclose(o.get_state()[0, 3:7], [0, 0, 0.6, 0.8], atol=1e-3)
    np.testing.assert_allclose(o.get_state()[0, :3], [0.5, 0, 1], atol=2e-3)


@pytest.mark.parametrize("randomizer", ["NONE", "MASS_RANDOMIZER"])
def test_static_hang_after_a_reset(randomizer):
    """after a reset on the rack: the base within 2 mm of the anchor and 0.5 degrees of level, the rack carrying m g, gravity's moment about
    the pivot balanced, no foot on the floor (the oracle twin of test_emu_rack.py::test_static_hang_after_a_reset)"""
    n = 4
    cfg, meta = rack_cfg(n, env_randomizer_mode=randomizer)
    o = Oracle(cfg, rack=meta["rack"])
    o.reset()
    s, info = o.get_state(), o.get_info(15)
    assert np.all(info[:, 0] == 1.0)
    assert np.all(np.linalg.norm(s[:, :3] - ANCHOR[:3], axis=1) < 2e-3) and np.all(info[:, 7] < 2e-3)
    np.testing.assert_allclose(info[:, 7], np.linalg.norm(s[:, :3] - ANCHOR[:3], axis=1), atol=1e-12)
    assert np.all(np.degrees(Rotation.from_quat(s[:, 3:7]).magnitude()) < 0.5)
    assert np.all(o.get_info(1) == 0.0)
    for i in range(n):
        e = o.energy(i)
        m = o.crba_rnea(i)[0][3, 3]
        np.testing.assert_allclose(info[i, 3], m * G, rtol=1e-3)
        assert np.abs(info[i, 1:3]).max() < 1e-3 * m * G
        moment = np.cross(e["com"] - s[i, :3], [0.0, 0.0, -m * G])
        np.testing.assert_allclose(info[i, 4:7], -moment, atol=1e-3 * m * G * 0.05)     # (levers of a few centimetres)


def test_low_anchor_shares_the_weight_with_the_feet():
    """the anchor 4 mm below the settled standing height: the four feet bear on the floor while the rack holds the base down and in
    place.  At rest the external forces balance -- rack + feet (normal and friction) + gravity = 0 -- and so do their moments about the
    pivot, to 1e-3 of m g (x the 0.3 m the feet lie from the pivot for the moments)."""
    n = 2
    cfg, _ = build_config(n_envs=n, noise=False, task_env="NO_TASK", env_randomizer_mode="NONE")
    o = Oracle(cfg)
    o.reset()
    stand = o.get_state()[0, :7].copy()
    anchor = stand.copy(); anchor[2] -= 0.004; anchor[3:] = [0, 0, 0, 1]
    r = Oracle(cfg, rack=anchor)
    r.reset()
    s, info, feet = r.get_state(), r.get_info(15), r.foot_wrench()
    assert np.all(r.get_info(1) == 1.0) and np.all(info[:, 0] == 1.0)
    assert np.abs(s[:, 7:13]).max() < 1e-4 and np.abs(s[:, 25:37]).max() < 1e-3      # at rest
    for i in range(n):
        m = r.crba_rnea(i)[0][3, 3]
        total = info[i, 1:4] + feet[i, :, :3].sum(0) + [0, 0, -m * G]
        assert np.abs(total).max() < 1e-3 * m * G, total
        assert feet[i, :, 2].min() > 1.0 and abs(info[i, 3]) > 1.0, (feet[i], info[i])      # both carry load
        np.testing.assert_allclose(feet[i, :, 2], r.get_info(0)[i])
        pivot = s[i, :3]
        mom = info[i, 4:7] + np.cross(feet[i, :, 3:] - pivot, feet[i, :, :3]).sum(0) + np.cross(r.energy(i)["com"] - pivot, [0, 0, -m * G])
        assert np.abs(mom).max() < 1e-3 * m * G * 0.3, mom


@pytest.mark.parametrize("anchor", sorted(ANCHORS))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_substep_rack_answer(seed, anchor):
    """no contact: the rack changes v by H^-1 J^T lambda, lambda = a float64 PGS of the six rows (pivot rows along the world axes, rows on
    the rotation vector of q_base q_anchor^-1, ERP joint_erp, bound 500 N x dt), H from the independent CRBA; the reported reaction is
    lambda / dt.  The oracle twin of test_emu_rack.py::test_one_substep_known_answer, in float64: 1e-9."""
    pos_err = [1e-4, 3e-4, 1e-3, 0.02, 0.05, 0.0]
    ang_err = [1e-4, 1e-3, 3e-3, 0.05, 0.1, 0.2]
    n = len(pos_err)
    cfg, _ = build_config(n_envs=n, time_step=DT, solver_residual_threshold=0.0, **PHYS)
    anc = ANCHORS[anchor]
    s, plain = airborne_near_anchor(cfg, seed, pos_err, ang_err, anc)
    s = s.astype(np.float64)
    s[:, 3:7] /= np.linalg.norm(s[:, 3:7], axis=1, keepdims=True)
    o = Oracle(cfg, rack=anc)
    o.set_state(s); plain.set_state(s)
    tau = np.random.default_rng(seed).uniform(-3, 3, (n, 12))
    for i in range(n):
        o.phys_step(i, tau[i]); plain.phys_step(i, tau[i])
    _, R0 = base_velocities(s)
    sa, sb = o.get_state(), plain.get_state()
    vstar = np.concatenate([np.einsum("nji,nj->ni", R0, sb[:, 10:13]), np.einsum("nji,nj->ni", R0, sb[:, 7:10]), sb[:, 25:37]], 1)
    info = o.get_info(15)
    plain.set_state(s)
    bound, binds, unclamped = 500.0 * DT, 0, 0
    qn = anc[3:].astype(np.float64) / np.linalg.norm(anc[3:].astype(np.float64))
    for i in range(n):
        H, _ = plain.crba_rnea(i)
        J = rack_jacobian(R0[i])
        A = J @ np.linalg.solve(H, J.T)
        q = (Rotation.from_quat(s[i, 3:7]) * Rotation.from_quat(qn).inv()).as_quat()
        err = np.concatenate([s[i, :3] - anc[:3].astype(np.float64), (2.0 if q[3] >= 0 else -2.0) * q[:3]])
        lam = pgs(A, -err * (cfg.joint_erp / DT) - J @ vstar[i], cfg.solver_iters, bound)
        binds += int(np.any(np.abs(lam) >= bound * (1 - 1e-12)))
        fin = vstar[i] + np.linalg.solve(H, J.T @ lam)
        # the substep clamps every velocity component to +-vel_cap behind the solve (world frame for the base): so does the expectation
        cap = cfg.vel_cap
        want = np.concatenate([np.clip(R0[i] @ fin[0:3], -cap, cap), np.clip(R0[i] @ fin[3:6], -cap, cap), np.clip(fin[6:], -cap, cap)])
        have = np.concatenate([sa[i, 10:13], sa[i, 7:10], sa[i, 25:37]])
        assert np.abs(have - want).max() < 1e-9 * max(1.0, np.abs(want).max()), (i, np.abs(have - want).max())
        unclamped += int(np.abs(fin).max() < 0.99 * cap)
        np.testing.assert_allclose(info[i, 1:7], lam / DT, rtol=0, atol=1e-9 * max(1.0, np.abs(lam / DT).max()))
        assert np.abs(info[i, 1:7]).max() <= 500.0 * (1 + 1e-12)
    assert binds >= 2, "the cases with large pose errors should hit the impulse bound"
    assert unclamped >= 4


def test_release_and_rehang():
    """a released robot falls freely for 0.2 s (0.196 m, 1.96 m/s) while its neighbour hangs; hung again it is pulled back with every
    reaction component within 500 N, and ends at rest at the anchor; a reset hangs a released robot again"""
    n = 2
    cfg, meta = rack_cfg(n)
    o = Oracle(cfg, rack=meta["rack"])
    o.reset()
    act = np.zeros((n, cfg.action_dim), np.float32)
    z0, p0 = o.get_state()[0, 2], o.energy(0)["p"][2]
    m = o.crba_rnea(0)[0][3, 3]
    o.set_rack(False, np.array([1, 0], np.uint8))
    for _ in range(20):
        o.step(act)
    s, info = o.get_state(), o.get_info(15)
    assert abs(s[1, 2] - 1.0) < 2e-3
    t = 0.2
    # free fall: the momentum goes down by m g t (the velocity update is exact in it); the base follows the centre of mass but for what
    # the PD-held legs move against it (a part in a thousand), and the position sums dt v: g / 2 t (t + dt)
    np.testing.assert_allclose(o.energy(0)["p"][2] - p0, -m * G * t, rtol=1e-4)
    np.testing.assert_allclose(s[0, 9], -G * t, rtol=1e-3)
    np.testing.assert_allclose(s[0, 2] - z0, -0.5 * G * t * (t + DT), rtol=2e-3)
    assert info[0, 0] == 0.0 and np.all(info[0, 1:7] == 0.0) and info[1, 0] == 1.0
    o.set_rack(True, np.array([1, 0], np.uint8))
    gap, binding = [o.get_info(15)[0, 7]], 0
    for k in range(150):
        o.step(act)
        info = o.get_info(15)
        assert info[0, 0] == 1.0 and np.abs(info[0, 1:7]).max() <= 500.0 * (1 + 1e-12), (k, info[0])
        binding += int(np.abs(info[0, 1:7]).max() >= 500.0 * (1 - 1e-3))
        gap.append(info[0, 7])
    gap = np.array(gap)
    assert binding >= 3, binding
    assert gap[:60].min() < 0.25 * gap[0] and gap[-20:].max() < 2e-3, gap
    assert np.abs(o.get_info(15)[0, 1:7]).max() < 500.0 * (1 - 1e-3)
    s = o.get_state()
    assert np.degrees(Rotation.from_quat(s[0, 3:7]).magnitude()) < 0.5 and np.abs(s[0, 7:13]).max() < 1e-2
    o.set_rack(False)
    o.step(act)
    o.reset(np.array([0, 1], np.uint8))
    assert o.get_info(15)[:, 0].tolist() == [0.0, 1.0]


def test_snapshot_carries_push_and_rack():
    """qso_snapshot / qso_restore (the yardstick's what_if restores and re-steps): push rows, hung flags and the last reaction"""
    n = 2
    cfg, meta = rack_cfg(n)
    o = Oracle(cfg, rack=meta["rack"])
    o.reset()
    act = np.zeros((n, cfg.action_dim), np.float32)
    o.set_external_wrench([10.0, 0, 0, 0, 1.0, 0], 25, "link")
    o.set_rack(False, np.array([0, 1], np.uint8))
    o.step(act)
    snap = o.snapshot()
    keep = (o.get_info(14).copy(), o.get_info(15).copy())
    o.step(act)
    after = o.get_state().copy()
    o.set_external_wrench(np.zeros(6), 0); o.set_rack(True)
    o.restore(snap)
    np.testing.assert_array_equal(o.get_info(14), keep[0]); np.testing.assert_array_equal(o.get_info(15), keep[1])
    o.step(act)
    np.testing.assert_array_equal(o.get_state(), after)
