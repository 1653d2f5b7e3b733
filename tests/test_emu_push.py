"""External pushes on the trunk (qs_set_external_wrench) in the host emulation (tests/emu/qs_emu_step.cpp): the velocity change of one
substep against the float64 mass matrix of the oracle, the common-path build's hand-over under a push against the full build bit for bit,
a zero-duration push against the push-free step, the bindings' refusals, and the schedules of push_rack_cases.py -- pushed on the ground
under PD, toppled, a duration that crosses six env steps -- against the float64 oracle under the yardstick (the CPU twins of
test_gpu_push.py).  No GPU."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle.qso import Oracle
from qs_amd.config import build_config
from emu.emu import Emu
from emu.emu_push import push_rows, step_push
from test_emu_hand_over import assert_bitwise

RAW = dict(task_env="NO_TASK", observation_space_mode="ENCODER", enable_action_filter=False, isRLGymInterface=False, motor_control_mode="TORQUE")
C_TRUNK = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "urdf_tables.npz"))["com"][1]   # trunk's inertial origin
DT = 0.001
# |measured - expected| of the known-answer cases below stays under 2e-6 (float32 state of magnitude ~1 differenced against float64
# H^-1 Q); what dropping the lever arm c x F changes in the same cases is at least 50 x this (asserted per case)
TOL = 5e-6


def base_velocities(s):
    """[N, 18]: angular and linear velocity of the base in the base frame, joint velocities (the oracle's generalized velocity)"""
    R = Rotation.from_quat(s[:, 3:7].astype(np.float64)).as_matrix()
    w = np.einsum("nji,nj->ni", R, s[:, 10:13].astype(np.float64))
    v = np.einsum("nji,nj->ni", R, s[:, 7:10].astype(np.float64))
    return np.concatenate([w, v, s[:, 25:37].astype(np.float64)], 1), R


def airborne_state(cfg, seed):
    rng = np.random.default_rng(seed)
    o = Oracle(cfg)
    s = o.get_state()
    s[:, :3] = [0.0, 0.0, 1.0]
    s[:, 3:7] = Rotation.random(cfg.n_envs, random_state=seed).as_quat()
    s[:, 7:13] = rng.uniform(-0.5, 0.5, (cfg.n_envs, 6))
    s[:, 13:25] = np.tile([0.0, 0.8, -1.6], 4)
    s[:, 25:37] = rng.uniform(-0.5, 0.5, (cfg.n_envs, 12))
    return s, o


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("frame", ["world", "link"])
def test_one_substep_known_answer(seed, frame):
    """action_repeat = 1, robot 1 m up in the air: the push changes v by dt H(q0)^-1 [c x F_b + tau_b ; F_b ; 0]"""
    cases = [((40.0, -25.0, 60.0), (0, 0, 0)), ((0, 0, 0), (3.0, -2.0, 1.5)), ((-30.0, 50.0, 10.0), (1.0, 2.0, -1.0))]
    n = len(cases)
    cfg, _ = build_config(n_envs=n, time_step=DT, action_repeat=1, self_collision=False, body_contacts=False, noise=False,
                          env_randomizer_mode="NONE", **RAW)
    s, o = airborne_state(cfg, seed)
    o.set_state(s)
    act = np.zeros((n, cfg.action_dim), np.float32)
    a, b = Emu(cfg), Emu(cfg)
    a.set_state(s.astype(np.float32)); b.set_state(s.astype(np.float32))
    fr = 2 if frame == "world" else 1
    push = push_rows(n, substeps=1, frame=fr)
    for i, (F, T) in enumerate(cases):
        push[i, 0:3], push[i, 3:6] = F, T
    step_push(a, act, push, 0)
    step_push(b, act, push_rows(n), 0)
    v0, R0 = base_velocities(s.astype(np.float32))
    va, _ = base_velocities(a.get_state())
    vb, _ = base_velocities(b.get_state())
    # the substep integrates in the frame of R0: both runs rotate their new world velocities back with the same R0
    sa, sb = a.get_state().astype(np.float64), b.get_state().astype(np.float64)
    dv = np.concatenate([np.einsum("nji,nj->ni", R0, sa[:, 10:13] - sb[:, 10:13]), np.einsum("nji,nj->ni", R0, sa[:, 7:10] - sb[:, 7:10]),
                         sa[:, 25:37] - sb[:, 25:37]], 1)
    for i, (F, T) in enumerate(cases):
        F, T = np.asarray(F, np.float64), np.asarray(T, np.float64)
        Fb, Tb = (R0[i].T @ F, R0[i].T @ T) if frame == "world" else (F, T)
        H, _ = o.crba_rnea(i)
        Q = np.concatenate([np.cross(C_TRUNK, Fb) + Tb, Fb, np.zeros(12)])
        want = DT * np.linalg.solve(H, Q)
        err = np.abs(dv[i] - want).max()
        assert err < TOL, (i, err, dv[i], want)
        if np.any(F):
            lever = DT * np.linalg.solve(H, np.concatenate([np.cross(C_TRUNK, Fb), np.zeros(15)]))
            assert np.abs(lever).max() > 50 * TOL, (i, np.abs(lever).max())


def standing(cfg, seed=0):
    a, b = Emu(cfg), Emu(cfg)
    a.reset(); b.reset()
    assert_bitwise(a.records(), b.records(), "records after reset")
    return a, b


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("case", ["topple", "ends_mid_step", "beyond_step"])
def test_hand_over_under_push_is_the_full_build(case, variant):
    """the common-path build plus the full build's resume equals the full build alone, bit for bit, with pushes in flight"""
    n = 6
    cfg, _ = build_config(n_envs=n, time_step=DT, action_repeat=10, settle_steps=300, noise=False, body_contacts=True,
                          env_randomizer_mode="GROUND_RANDOMIZER", **RAW)
    full, hot = standing(cfg)
    rng = np.random.default_rng(variant)
    if case == "topple":       # lateral shoves hard enough to throw a standing robot onto its side within a few steps
        push = push_rows(n, substeps=60, frame=2)
        side = rng.choice([-1.0, 1.0], n)
        push[:, 1] = side * rng.uniform(300.0, 600.0, n)
        push[:, 3] = -side * rng.uniform(60.0, 90.0, n)     # (the roll a shove at the trunk's height gives, sped up)
        push[0, 6] = 0.0       # a wave-mate without a push
    elif case == "ends_mid_step":
        push = push_rows(n, substeps=5, frame=1)
        push[:, 0:3] = rng.uniform(-150, 150, (n, 3)); push[:, 3:6] = rng.uniform(-5, 5, (n, 3))
    else:
        push = push_rows(n, substeps=25, frame=2)
        push[:, 0:3] = rng.uniform(-200, 200, (n, 3)); push[:, 3:6] = rng.uniform(-8, 8, (n, 3))
    pf, ph = push.copy(), push.copy()
    act = np.zeros((n, cfg.action_dim), np.float32)
    handed = []
    for t in range(12):
        rf = step_push(full, act, pf, 0)
        rh = step_push(hot, act, ph, variant)
        for name, x, y in zip(("obs", "reward", "done", "truncated"), rf[:4], rh[:4]):
            assert_bitwise(x, y, f"{name}, step {t}")
        assert_bitwise(full.records(), hot.records(), f"records, step {t}")
        assert_bitwise(pf, ph, f"push rows, step {t}")
        handed.append(rh[4])
    handed = np.concatenate(handed)
    if case == "topple":
        assert (handed >= 0).any(), "no hand-over: the pushes threw nobody down"
        R = Rotation.from_quat(full.get_state()[1:, 3:7]).as_matrix()
        assert (R[:, 2, 2] < 0.5).any(), "no robot lies on its side"
    if case == "ends_mid_step":
        assert (pf[:, 6] == 0).all()
    if case == "beyond_step":
        assert (pf[:, 6] == 0).all() and np.isin(handed, -1).any()


def test_push_counts_down_and_zero_push_is_the_plain_step():
    n = 4
    cfg, _ = build_config(n_envs=n, time_step=DT, action_repeat=10, settle_steps=300, noise=False, **RAW)
    a, b = standing(cfg)
    act = np.random.default_rng(0).uniform(-1, 1, (n, cfg.action_dim)).astype(np.float32)
    zero = push_rows(n, force=(500.0, 0, 0), substeps=0)       # a cancelled push: its force never acts
    for t in range(3):
        ra = step_push(a, act, zero, 0)
        rb = b.step(act)
        for name, x, y in zip(("obs", "reward", "done", "truncated"), ra[:4], rb):
            assert_bitwise(x, y, f"{name}, step {t}")
        assert_bitwise(a.records(), b.records(), f"records, step {t}")
    p = push_rows(n, force=(0, 0, 30.0), substeps=25)
    left = []
    for _ in range(3):
        step_push(a, act, p, 0)
        left.append(p[:, 6].copy())
    assert np.array_equal(np.stack(left), np.array([[15] * n, [5] * n, [0] * n], np.float32))


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_push_acts_on_exactly_its_substeps(variant):
    """action_repeat = 2, airborne, one env step: pushes of 0, 1 and 2 substeps give three different results, 2 and 3 substeps the same
    (both cover the step); 3 substeps over two steps equal 2, then 1 issued before the second step (the gate k < remaining, every build)"""
    n = 3
    cfg, _ = build_config(n_envs=n, time_step=DT, action_repeat=2, self_collision=False, body_contacts=False, noise=False,
                          env_randomizer_mode="NONE", **RAW)
    s, _ = airborne_state(cfg, 11)
    F = np.array([[40.0, -25.0, 60.0], [0, 0, -30.0], [-30.0, 50.0, 10.0]], np.float32)
    T = np.array([[0, 0, 0], [3.0, -2.0, 1.5], [1.0, 2.0, -1.0]], np.float32)
    act = np.zeros((n, cfg.action_dim), np.float32)

    def row(k):
        p = push_rows(n, substeps=k, frame=1)
        p[:, 0:3], p[:, 3:6] = F, T
        return p
    emus, rows = [], []
    for k in range(4):
        e = Emu(cfg)
        e.set_state(s.astype(np.float32))
        rows.append(row(k))
        step_push(e, act, rows[-1], variant)
        emus.append(e)
    st = [e.get_state() for e in emus]
    for i in range(3):
        for j in range(i + 1, 3):
            assert (st[i] != st[j]).any(axis=1).all(), f"pushes of {i} and {j} substeps gave the same result"
    assert_bitwise(emus[2].records(), emus[3].records(), "pushes of 2 and 3 substeps over a step of 2")
    assert [int(r[0, 6]) for r in rows] == [0, 0, 0, 1]
    step_push(emus[3], act, rows[3], variant)
    step_push(emus[2], act, row(1), variant)
    assert_bitwise(emus[2].records(), emus[3].records(), "3 substeps at once vs 2 + 1")


def emu_device(variant):
    """make_device of push_rack_cases.run: the emulation through the builds of step kernel `variant` (0 = the full build alone)"""
    import yardstick as Y

    def make(cfg, meta):
        rk = meta["rack"]
        dev = Y.EmuDevice(Emu(cfg, rack=np.concatenate([rk["pos"], rk["quat"]]) if rk["on"] else None), variant)
        dev.reset(np.ones(cfg.n_envs, np.uint8))
        return dev
    return make


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("case", ["ground_cone", "ground_pyramid", "topple", "repeat4"])
def test_pushes_against_the_oracle(case, variant):
    """push_rack_cases.PUSH_CASES through yardstick.resynced_parity with the emulation as the device: every step from the oracle's state,
    strict (pose 5e-6, base velocity 5e-4, q 2e-5, qd 5e-3) where the step map is smooth, tolerance + 5 x |oracle32 - oracle64| where a
    non-foot link touched the ground; the remaining-substeps column equal on both oracle builds and the emulation before and after every
    step; the coverage the case exists for.  The full build and both hand-over variants."""
    import push_rack_cases as P
    P.check(P.run(case, P.PUSH_CASES, emu_device(variant)), f"test_emu_push[{case}-{variant}]", "emulation")


@pytest.mark.parametrize("case", ["ground_cone", "ground_pyramid", "topple", "repeat4"])
def test_float32_oracle_meets_the_push_schedules(case):
    """the oracle's own float32 build as the device: inside the same bounds, and the coverage counts are met by the oracles alone"""
    import push_rack_cases as P
    P.check(P.run(case, P.PUSH_CASES, P.OracleDevice), f"test_emu_push[{case}-oracle32]", "oracle32")


class _Stub:
    """the attributes apply_external_force validates against, without a device"""

    def __init__(self, n=4):
        import torch
        from qs_amd.vec_env import QuadrupedVecEnv
        self.torch, self.num_envs, self.device = torch, n, torch.device("cpu")
        self.cfg, _ = build_config(n_envs=n, **RAW)
        self._stream = lambda: None
        self.apply = QuadrupedVecEnv.apply_external_force.__get__(self)
        self._indices = QuadrupedVecEnv._indices.__get__(self)


@pytest.mark.parametrize("kw, msg", [
    (dict(force=np.zeros((4, 2))), "force must have shape"),
    (dict(force=np.zeros((3, 3))), "force must have shape"),
    (dict(force=np.zeros(3), torque=np.zeros(4)), "torque must have shape"),
    (dict(force=[np.nan, 0, 0]), "force must be finite"),
    (dict(force=np.zeros(3), torque=[0, np.inf, 0]), "torque must be finite"),
    (dict(force=np.zeros(3), frame="base"), "frame must be one of"),
    (dict(force=np.zeros(3), substeps=-1), "substeps must be a non-negative integer"),
    (dict(force=np.zeros(3), substeps=2.5), "substeps must be a non-negative integer"),
    (dict(force=np.zeros(3), substeps=np.ones(3, np.int32)), "substeps must be a scalar or have shape"),
])
def test_bindings_refuse_bad_pushes(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _Stub().apply(**kw)
