"""The rack (on_rack=True: qs_create_ex with a qs_rack) in the host emulation (tests/emu/qs_emu_step.cpp): the velocity change of one substep
against a float64 PGS of the six rows through the oracle's mass matrix, the reported reaction, the common-path build's hand-over to the full
build bit for bit with a joint at its stop, the many-rows solve's rack rows against tests/rare_ref.py, a static hang after a reset, a
release and a re-hang, the bindings' refusals, and the schedules of push_rack_cases.py -- hung under PD, hung on a low anchor with the
feet on the floor, released and hung again while falling, joints at their stops -- against the float64 oracle under the yardstick, the
rack's reaction included (the CPU twins of test_gpu_rack.py).  No GPU."""

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle.qso import Oracle
from qs_amd.config import build_config
from emu.emu import Emu
from emu.emu_rack import ANCHOR, rack_info, reset_rack, set_rack, step_rack
from test_emu_hand_over import assert_bitwise
from test_emu_push import base_velocities

RAW = dict(task_env="NO_TASK", observation_space_mode="ENCODER", enable_action_filter=False, isRLGymInterface=False, motor_control_mode="TORQUE")
DT = 0.001
G = 9.8   # (build_config: cfg.gravity, pybullet.setGravity(0, 0, -9.8))


def rack_jacobian(R):
    """[6, 18]: the rack's rows in the oracle's generalized velocity (base angular, base linear -- both in the base frame --, joints): pivot
    rows e_k . (R v_b), rotation rows e_k . (R w_b)"""
    J = np.zeros((6, 18))
    for k in range(3):
        J[k, 3:6] = R[k, :]
        J[3 + k, 0:3] = R[k, :]
    return J


def pgs(A, b, iters, bound):
    """float64 PGS of the six rows as the solvers sweep them (qs_core.h solve_and_integrate, PAY): backwards on even sweeps, forwards on
    odd ones, each impulse clamped to +-bound; every sweep is run (solver_residual_threshold = 0)"""
    lam = np.zeros(6)
    for it in range(iters):
        for p in (range(6) if it & 1 else range(5, -1, -1)):
            lam[p] = np.clip(lam[p] + (b[p] - A[p] @ lam) / A[p, p], -bound, bound)
    return lam


# the reference's anchor, and one displaced and turned (qs_create_ex takes any position and orientation)
ANCHORS = {"identity": ANCHOR, "tilted": np.concatenate([[0.3, -0.2, 1.2], Rotation.from_rotvec([0.25, -0.4, 0.9]).as_quat()]).astype(np.float32)}


def airborne_near_anchor(cfg, seed, pos_err, ang_err, anchor=ANCHOR):
    """states whose base origin lies pos_err from the anchor and whose frame is turned by ang_err (world axis) from the anchor's"""
    rng = np.random.default_rng(seed)
    o = Oracle(cfg)
    s = o.get_state()
    n = cfg.n_envs
    s[:, :3] = anchor[:3] + rng.normal(size=(n, 3)) * np.asarray(pos_err)[:, None]
    s[:, 3:7] = (Rotation.from_rotvec(rng.normal(size=(n, 3)) * np.asarray(ang_err)[:, None]) * Rotation.from_quat(anchor[3:])).as_quat()
    s[:, 7:13] = rng.uniform(-0.3, 0.3, (n, 6))
    s[:, 13:25] = np.tile([0.0, 0.8, -1.6], 4) + rng.uniform(-0.2, 0.2, (n, 12))
    s[:, 25:37] = rng.uniform(-0.5, 0.5, (n, 12))
    return s.astype(np.float32), o


@pytest.mark.parametrize("anchor", sorted(ANCHORS))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_substep_known_answer(seed, anchor):
    """action_repeat = 1, no contact: the rack changes v by H^-1 J^T lambda, lambda = the six rows' PGS; the reported force and torque are
    lambda / dt.  Small pose errors leave the impulse bound (500 N x dt) alone, large ones make it bind."""
    pos_err = [1e-4, 3e-4, 1e-3, 0.02, 0.05, 0.0]
    ang_err = [1e-4, 1e-3, 3e-3, 0.05, 0.1, 0.2]
    n = len(pos_err)
    cfg, _ = build_config(n_envs=n, time_step=DT, action_repeat=1, self_collision=False, body_contacts=False, noise=False,
                          env_randomizer_mode="NONE", solver_residual_threshold=0.0, **RAW)
    anc = ANCHORS[anchor]
    s, o = airborne_near_anchor(cfg, seed, pos_err, ang_err, anc)
    o.set_state(s.astype(np.float64))
    act = np.zeros((n, cfg.action_dim), np.float32)
    a, b = Emu(cfg), Emu(cfg)
    a.set_state(s); b.set_state(s)
    set_rack(a, True); set_rack(b, False)
    step_rack(a, act, 0, anchor=anc)
    step_rack(b, act, 0, anchor=anc)
    _, R0 = base_velocities(s)
    sa, sb = a.get_state().astype(np.float64), b.get_state().astype(np.float64)
    dv = np.concatenate([np.einsum("nji,nj->ni", R0, sa[:, 10:13] - sb[:, 10:13]), np.einsum("nji,nj->ni", R0, sa[:, 7:10] - sb[:, 7:10]),
                         sa[:, 25:37] - sb[:, 25:37]], 1)
    vstar = np.concatenate([np.einsum("nji,nj->ni", R0, sb[:, 10:13]), np.einsum("nji,nj->ni", R0, sb[:, 7:10]), sb[:, 25:37]], 1)
    info = rack_info(a, anchor=anc)
    bound = 500.0 * DT
    binds = 0
    for i in range(n):
        H, _ = o.crba_rnea(i)
        J = rack_jacobian(R0[i])
        A = J @ np.linalg.solve(H, J.T)
        q = (Rotation.from_quat(s[i, 3:7].astype(np.float64)) * Rotation.from_quat(anc[3:].astype(np.float64)).inv()).as_quat()
        perr = s[i, :3].astype(np.float64) - anc[:3]
        aerr = (2.0 if q[3] >= 0 else -2.0) * q[:3]       # rotation vector of q_base q_anchor^-1, small angle
        err = np.concatenate([perr, aerr])
        rhs = -err * (cfg.joint_erp / DT) - J @ vstar[i]
        lam = pgs(A, rhs, cfg.solver_iters, bound)
        binds += int(np.any(np.abs(lam) >= bound * (1 - 1e-9)))
        want = np.linalg.solve(H, J.T @ lam)
        # the substep clamps every velocity component to +-vel_cap behind the solve (world frame for the base): so does the expectation
        cap = cfg.vel_cap
        fin = vstar[i] + want
        exp_w, exp_v = np.clip(R0[i] @ fin[0:3], -cap, cap), np.clip(R0[i] @ fin[3:6], -cap, cap)
        exp = np.concatenate([exp_w, exp_v, np.clip(fin[6:], -cap, cap)])
        got = np.concatenate([sa[i, 10:13], sa[i, 7:10], sa[i, 25:37]])
        scale = max(1.0, np.abs(want).max())
        assert np.abs(got - exp).max() < 2e-5 * scale, (i, np.abs(got - exp).max(), got, exp)
        if np.abs(fin).max() < 0.99 * cap:
            assert np.abs(dv[i] - want).max() < 2e-5 * scale, (i, np.abs(dv[i] - want).max(), dv[i], want)
        assert info[i, 0] == 1.0
        np.testing.assert_allclose(info[i, 1:7], lam / DT, rtol=2e-3, atol=2e-3 * max(1.0, np.abs(lam / DT).max()))
    assert binds >= 2, "the cases with large pose errors should hit the impulse bound"
    assert np.all(rack_info(b, anchor=anc)[:, 1:7] == 0.0) and np.all(rack_info(b, anchor=anc)[:, 0] == 0.0)


def _stop_run(cfg, variant, steps=14):
    """hung robots whose calves are driven into their stops (raw torques), released and hung again on the way: the full build against the
    builds of the step kernels, bit for bit"""
    n = cfg.n_envs
    full, hot = Emu(cfg), Emu(cfg)
    reset_rack(full); reset_rack(hot)
    assert_bitwise(full.records(), hot.records(), "records after the reset")
    rng = np.random.default_rng(variant)
    handed = []
    for t in range(steps):
        act = rng.uniform(-1, 1, (n, cfg.action_dim)).astype(np.float32) * 0.3
        act[: n // 2, 2::3] = -30.0 if t % 8 < 4 else 30.0       # (N m) calves against their stops, one way then the other
        if t == 5:
            m = np.arange(n) % 3 == 0
            set_rack(full, False, m); set_rack(hot, False, m)
        if t == 10:
            set_rack(full, True); set_rack(hot, True)
        rf = step_rack(full, act, 0)
        rh = step_rack(hot, act, variant)
        for name, x, y in zip(("obs", "reward", "done", "truncated"), rf[:4], rh[:4]):
            assert_bitwise(x, y, f"{name}, step {t}")
        assert_bitwise(full.records(), hot.records(), f"records, step {t}")
        handed.append(rh[4])
    return np.concatenate(handed)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("friction", ["cone", "pyramid"])
def test_hand_over_with_a_joint_at_its_stop_is_the_full_build(variant, friction):
    """k_step_rack / k_step_dense_rack: the common-path build with the rack's rows (cone) or without them (pyramid: a hung wave hands over at
    once), and its hand-over to the full build's many-rows solve when a joint reaches its stop, equal the full build alone bit for bit"""
    cfg, _ = build_config(n_envs=6, time_step=DT, action_repeat=10, settle_steps=300, noise=False, body_contacts=True, friction_model=friction,
                          env_randomizer_mode="GROUND_RANDOMIZER", **RAW)
    cfg.tau_max[:] = [40.0, 40.0, 40.0]
    handed = _stop_run(cfg, variant)
    assert np.any(handed >= 0), "no step handed over: the joint stops were not reached"
    if friction == "cone":
        assert np.any(handed < 0), "every step handed over: the common-path build never solved the rack's rows"


@pytest.mark.parametrize("friction", ["cone", "pyramid"])
def test_many_rows_solve_of_the_rack_rows(friction):
    """the row sets the RACK builds hand the many-rows solve while hung robots hold joints at their stops: the rack's rows sit in the payload
    positions as rack_rows builds them (1 / mass = 1 / inertia = 0, no lever, 1 / diag of |w|^2, act 1), and the emulation twin of the
    solve agrees with tests/rare_ref.py's float64 PGS on them"""
    from emu.emu_rack import RackCapture
    from test_rare_solver import twin_vs_ref
    cfg, _ = build_config(n_envs=6, time_step=DT, action_repeat=10, settle_steps=300, noise=False, body_contacts=True, friction_model=friction,
                          env_randomizer_mode="GROUND_RANDOMIZER", **RAW)
    cfg.tau_max[:] = [40.0, 40.0, 40.0]
    with RackCapture(512) as cap:
        _stop_run(cfg, 1, steps=14)
    sel = np.nonzero(cap.has_pay)[0]
    assert len(sel) >= 16, len(sel)
    pay = cap.pay[sel]
    assert np.all(pay[:, 54:58] == 0.0) and np.all(pay[:, 58] == 1.0)          # rB, 1 / inertia; act
    w = pay[:, :36].reshape(-1, 6, 6).astype(np.float64)
    np.testing.assert_allclose(pay[:, 48:54], (w ** 2).sum(2), rtol=1e-5)
    assert np.all(cap.rows[sel][:, :, 9:12, 14].sum((1, 2)) > 0)               # joint-limit rows beside them
    for iters in (1, 3, 30):
        cfg.solver_iters = iters
        twin_vs_ref(cfg, cap.rows[sel], cap.env[sel], cap.warm[sel], pay, f"rack rows {friction} iters {iters}")


@pytest.mark.parametrize("randomizer", ["NONE", "MASS_RANDOMIZER"])
def test_static_hang_after_a_reset(randomizer):
    """after a reset on the rack (2500 settle substeps hung): the base within 2 mm of the anchor, the trunk within 0.5 degrees of level, the
    rack carrying the whole weight (URDF masses plus the payload block: the mass randomizer keeps the total) and balancing gravity's moment
    about the pivot, no foot on the floor"""
    n = 4
    cfg, _ = build_config(n_envs=n, noise=False, task_env="NO_TASK", env_randomizer_mode=randomizer, on_rack=True)
    e = Emu(cfg)
    reset_rack(e)
    s = e.get_state().astype(np.float64)
    info = rack_info(e).astype(np.float64)
    assert np.all(info[:, 0] == 1.0)
    assert np.all(np.linalg.norm(s[:, :3] - ANCHOR[:3], axis=1) < 2e-3), s[:, :3]
    tilt = np.degrees(Rotation.from_quat(s[:, 3:7]).magnitude())
    assert np.all(tilt < 0.5), tilt
    assert np.all(info[:, 7] < 2e-3)
    assert np.all(e.records()[:, e.field("R_FOOT_CONTACT"):e.field("R_FOOT_CONTACT") + 4] == 0.0)
    o = Oracle(cfg)
    o.set_state(s)
    for i in range(n):
        H, _ = o.crba_rnea(i)
        m = H[3, 3]
        np.testing.assert_allclose(info[i, 3], m * G, rtol=1e-3)
        assert np.abs(info[i, 1:3]).max() < 1e-3 * m * G
        if randomizer == "NONE":   # (the oracle's masses are the URDF's: the centre of mass is the same only without the randomizer)
            com = o.energy(i)["com"]
            moment = np.cross(com - ANCHOR[:3], [0.0, 0.0, -m * G])   # gravity's moment about the pivot
            np.testing.assert_allclose(info[i, 4:7], -moment, atol=2e-3)


def test_released_robot_falls_and_rehung_robot_is_pulled_back():
    """a released robot falls freely while its neighbour still hangs; hung again 0.2 m below the anchor and moving down at 2 m/s, the rack
    pulls it back -- every reported force and torque component within the 500 N x dt bound -- and holds it at the anchor"""
    n = 2
    cfg, _ = build_config(n_envs=n, noise=False, task_env="NO_TASK", on_rack=True, env_randomizer_mode="NONE")
    e = Emu(cfg)
    reset_rack(e)
    act = np.zeros((n, cfg.action_dim), np.float32)
    set_rack(e, False, np.array([1, 0], np.uint8))
    for _ in range(20):
        step_rack(e, act, 1)
    s = e.get_state()
    assert abs(s[1, 2] - 1.0) < 2e-3, s[:, 2]                      # env 1 still hangs
    assert 0.75 < s[0, 2] < 0.85 and s[0, 9] < -1.5, s[0]           # env 0 has fallen freely for 0.2 s (0.2 m, 2 m/s)
    info = rack_info(e)
    assert info[0, 0] == 0.0 and np.all(info[0, 1:7] == 0.0) and info[1, 0] == 1.0
    set_rack(e, True, np.array([1, 0], np.uint8))
    gap = [rack_info(e)[0, 7]]
    for k in range(150):
        step_rack(e, act, 1)
        info = rack_info(e)
        assert info[0, 0] == 1.0
        assert np.abs(info[0, 1:7]).max() <= 500.0 * (1 + 1e-5), (k, info[0])
        gap.append(info[0, 7])
    gap = np.array(gap)
    # (still moving down at first, then pulled up at the bound and past the anchor a few times -- the ERP target is far beyond what the
    # bound allows -- until the error is small enough for the rows to act within it)
    assert gap[:60].min() < 0.25 * gap[0], gap[:60]
    assert gap[-1] < 2e-3 and gap[-20:].max() < 2e-3, gap[-20:]
    assert np.abs(rack_info(e)[0, 1:7]).max() < 500.0                # back at rest: the bound no longer binds
    assert np.degrees(Rotation.from_quat(e.get_state()[0, 3:7].astype(np.float64)).magnitude()) < 0.5


RACK_TWINS = ["hung_cone", "hung_pyramid", "low_anchor", "low_anchor_sweeps3", "rehang", "stops"]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("case", RACK_TWINS)
def test_rack_against_the_oracle(case, variant):
    """push_rack_cases.RACK_CASES through yardstick.resynced_parity with the emulation as the device: state, observation, reward, torques,
    foot forces and the rack's reaction (force: 0.5 N + 2 %; torque: yardstick.RACK_FIELDS) strictly where the step map is smooth, under
    the spread rule where the rack's bound binds in either oracle build or a link is on the ground; hung flags equal before and after
    every step; the coverage the case exists for.  The full build and both hand-over variants."""
    import push_rack_cases as P
    from test_emu_push import emu_device
    P.check(P.run(case, P.RACK_CASES, emu_device(variant)), f"test_emu_rack[{case}-{variant}]", "emulation")


@pytest.mark.parametrize("case", RACK_TWINS)
def test_float32_oracle_meets_the_rack_schedules(case):
    import push_rack_cases as P
    P.check(P.run(case, P.RACK_CASES, P.OracleDevice), f"test_emu_rack[{case}-oracle32]", "oracle32")


def test_rack_torque_floor_is_the_measured_one():
    """yardstick.RACK_FIELDS' floor for the reaction's torque is FACTOR x the 99th percentile of |oracle32 - oracle64| over the smooth hung
    rows of the rack schedules, as written next to it: measured again here, it lies within a factor 1.5 of the recorded figure"""
    import push_rack_cases as P
    import yardstick as Y
    pool = []
    for case in RACK_TWINS:
        pool += P.run(case, P.RACK_CASES, P.OracleDevice)["rack_own_smooth"]["rack_torque"]
    p50, p90, p99 = Y.percentiles(pool)
    print("rack torque |oracle32 - oracle64| over", len(pool), "smooth rows: p50 / p90 / p99", p50, p90, p99)
    assert len(pool) >= 1000
    assert Y.RACK_TORQUE_OWN["p99"] / 1.5 <= p99 <= Y.RACK_TORQUE_OWN["p99"] * 1.5, (p99, Y.RACK_TORQUE_OWN)
    assert Y.RACK_FIELDS["rack_torque"] == (3, Y.FACTOR * Y.RACK_TORQUE_OWN["p99"])


# ---- bindings (no device needed)
def test_on_rack_refusals():
    cfg, meta = build_config(n_envs=1, on_rack=True)
    assert meta["rack"]["on"] and list(meta["rack"]["pos"]) == [0, 0, 1] and list(meta["rack"]["quat"]) == [0, 0, 0, 1]
    assert not build_config(n_envs=1)[1]["rack"]["on"]
    with pytest.raises(NotImplementedError, match="payload"):
        build_config(n_envs=1, on_rack=True, payload="soft")
    with pytest.raises(NotImplementedError, match="render"):
        build_config(n_envs=1, render=True)
    with pytest.raises(NotImplementedError, match="render") as ei:
        build_config(n_envs=1, render=True, on_rack=True)
    assert "on_rack" not in str(ei.value)


def test_gym_env_robot_reports_the_rack_position():
    from qs_amd.env.quadruped_gym_env import _RobotView
    from qs_amd import go1_config

    class _E:
        _robot_config = go1_config.make_config(False)
        _on_rack = True
    assert _RobotView(_E())._GetDefaultInitPosition() == [0, 0, 1]
    _E._on_rack = False
    assert _RobotView(_E())._GetDefaultInitPosition() == [0, 0, 0.32]
