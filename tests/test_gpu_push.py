"""External pushes on the trunk (qs_set_external_wrench, QuadrupedVecEnv.apply_external_force) on the device: the velocity change of
one substep against the float64 mass matrix, the duration counted across env steps, independence of environments without a push,
both step kernels, resets, the host / fused paths and the single-environment drop-in; and the schedules of push_rack_cases.py -- pushed on
the ground under PD with springs and the filter, toppled by a push, a duration that crosses six env steps -- held to the float64 oracle
under the yardstick (tests/yardstick.py resynced_parity)."""
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from test_gpu_round2 import RAW, vec_env

pytestmark = pytest.mark.gpu
C_TRUNK = np.load(os.path.join(os.path.dirname(__file__), "golden", "urdf_tables.npz"))["com"][1]
DT = 0.001


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def bits(x):
    x = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b, what):
    assert np.array_equal(bits(a), bits(b)), f"{what}: {np.argwhere(bits(a) != bits(b))[:8].tolist()}"


def airborne(n, seed):
    rng = np.random.default_rng(seed)
    from oracle.qso import Oracle
    cfg_env = vec_env(n, time_step=DT, action_repeat=1, self_collision=False, body_contacts=False, **RAW)
    o = Oracle(cfg_env.cfg)
    s = o.get_state()
    s[:, :3] = [0.0, 0.0, 1.0]
    s[:, 3:7] = Rotation.random(n, random_state=seed).as_quat()
    s[:, 7:13] = rng.uniform(-0.5, 0.5, (n, 6))
    s[:, 13:25] = np.tile([0.0, 0.8, -1.6], 4)
    s[:, 25:37] = rng.uniform(-0.5, 0.5, (n, 12))
    return cfg_env, o, s


@pytest.mark.parametrize("frame", ["world", "link"])
def test_device_one_substep_known_answer(torch_cuda, frame):
    F = np.array([[40.0, -25.0, 60.0], [0, 0, 0], [-30.0, 50.0, 10.0]], np.float32)
    T = np.array([[0, 0, 0], [3.0, -2.0, 1.5], [1.0, 2.0, -1.0]], np.float32)
    a, o, s = airborne(3, 7)
    b = vec_env(3, time_step=DT, action_repeat=1, self_collision=False, body_contacts=False, **RAW)
    o.set_state(s)
    for v in (a, b):
        v.reset_tensor(); v.set_state(s.astype(np.float32))
    act = torch_cuda.zeros((3, a.action_dim), device=a.device)
    a.apply_external_force(F, T, substeps=1, frame=frame)
    a.step_tensor(act); b.step_tensor(act)
    R0 = Rotation.from_quat(s[:, 3:7].astype(np.float32).astype(np.float64)).as_matrix()
    sa, sb = a.get_state().cpu().numpy().astype(np.float64), b.get_state().cpu().numpy().astype(np.float64)
    dv = np.concatenate([np.einsum("nji,nj->ni", R0, sa[:, 10:13] - sb[:, 10:13]), np.einsum("nji,nj->ni", R0, sa[:, 7:10] - sb[:, 7:10]),
                         sa[:, 25:37] - sb[:, 25:37]], 1)
    for i in range(3):
        Fb, Tb = (R0[i].T @ F[i], R0[i].T @ T[i]) if frame == "world" else (F[i].astype(np.float64), T[i].astype(np.float64))
        H, _ = o.crba_rnea(i)
        want = DT * np.linalg.solve(H, np.concatenate([np.cross(C_TRUNK, Fb) + Tb, Fb, np.zeros(12)]))
        assert np.abs(dv[i] - want).max() < 5e-6, (i, dv[i], want)


def test_duration_across_steps(torch_cuda):
    """25 substeps with action_repeat = 10: remaining 15, 5, 0; the same as pushes of 10, 10, 5 issued per step; the impulse F 25 dt"""
    t = torch_cuda
    a, o, s = airborne(2, 3)
    kw = dict(time_step=DT, action_repeat=10, self_collision=False, body_contacts=False, **RAW)
    a = vec_env(2, **kw); b = vec_env(2, **kw); c = vec_env(2, **kw)
    for v in (a, b, c):
        v.reset_tensor(); v.set_state(s.astype(np.float32))
    F = np.array([[30.0, -20.0, 50.0], [-60.0, 10.0, 0.0]], np.float32)
    act = t.zeros((2, a.action_dim), device=a.device)
    a.apply_external_force(F, substeps=25, frame="world")
    left = []
    for k in (10, 10, 5):
        b.apply_external_force(F, substeps=k, frame="world")
        a.step_tensor(act); b.step_tensor(act); c.step_tensor(act)
        left.append(a.get_info("external_wrench")[:, 6].cpu().numpy())
        same(a.get_state(), b.get_state(), "state, 25 substeps at once vs 10 + 10 + 5")
    assert np.array_equal(np.stack(left), [[15, 15], [5, 5], [0, 0]])
    info = a.get_info("external_wrench").cpu().numpy()
    assert np.array_equal(info[:, :3], F) and (info[:, 7] == 2).all()

    def momentum(v):
        st = v.get_state().cpu().numpy().astype(np.float64)
        o.set_state(st)
        out = []
        for i in range(2):
            H, _ = o.crba_rnea(i)
            R = Rotation.from_quat(st[i, 3:7]).as_matrix()
            vb = np.concatenate([R.T @ st[i, 10:13], R.T @ st[i, 7:10], st[i, 25:37]])
            out.append(R @ (H @ vb)[3:6])
        return np.array(out)
    dp = momentum(a) - momentum(c)
    np.testing.assert_allclose(dp, F.astype(np.float64) * 25 * DT, rtol=1e-2, atol=2e-3)   # (float32 velocities of ~1 m/s times 12 kg: ~1e-5)


def topple_push(n, wave_env):
    F = np.zeros((n, 3), np.float32); T = np.zeros((n, 3), np.float32)
    F[wave_env, 1] = 300.0; F[wave_env, 2] = -600.0; T[wave_env, 0] = -100.0   # sideways and down: a body link reaches the ground
    return F, T


@pytest.mark.parametrize("step_kernel", ["1", "2"])
def test_no_push_invariance_and_wave_mates(torch_cuda, monkeypatch, step_kernel):
    monkeypatch.setenv("QS_STEP_VARIANT", step_kernel)
    t = torch_cuda
    n = 32
    kw = dict(body_contacts=True, env_randomizer_mode="GROUND_RANDOMIZER")
    never, zero, pushed = vec_env(n, **kw), vec_env(n, **kw), vec_env(n, **kw)
    for v in (never, zero, pushed):
        v.reset_tensor()
    rng = np.random.default_rng(0)
    zero.apply_external_force(np.full(3, 300.0, np.float32), substeps=0)
    F, T = topple_push(n, 3)
    F[20], T[20] = [0, 0, 80.0], [0, 0, 0]
    mask = np.zeros(n, bool); mask[[3, 20]] = True
    pushed.apply_external_force(F, T, substeps=np.where(mask, 100, 0).astype(np.int32))
    fell = False
    for k in range(20):
        act = t.as_tensor(rng.uniform(-1, 1, (n, never.action_dim)).astype(np.float32), device=never.device)
        r0 = [x.clone() for x in never.step_tensor(act)]
        r1 = [x.clone() for x in zero.step_tensor(act)]
        r2 = [x.clone() for x in pushed.step_tensor(act)]
        for name, x, y, z in zip(("obs", "rew", "done", "trunc"), r0, r1, r2):
            same(x, y, f"{name}: never pushed vs zero push, step {k}")
            same(x[~mask], z[~mask], f"{name}: wave-mates of pushed environments, step {k}")
        same(never.get_state(), zero.get_state(), f"state, step {k}")
        same(never.get_state()[~mask], pushed.get_state()[~mask], f"wave-mates' state, step {k}")
        fell = fell or bool(pushed.get_info("n_invalid")[3, 0] > 0)
    assert fell, "the pushed robot never touched the ground with its body: its wave never took the full build"
    assert not np.array_equal(bits(never.get_state()[3]), bits(pushed.get_state()[3]))


def test_both_step_kernels_agree_under_pushes(torch_cuda, monkeypatch):
    t = torch_cuda
    n = 32
    out = []
    for variant in ("1", "2"):
        monkeypatch.setenv("QS_STEP_VARIANT", variant)
        v = vec_env(n, body_contacts=True, env_randomizer_mode="GROUND_RANDOMIZER", auto_reset=True, reset_lookahead=0)
        v.reset_tensor()
        rng = np.random.default_rng(5)
        res = []
        for k in range(10):
            if k % 3 == 0:
                v.apply_external_force(rng.uniform(-400, 400, (n, 3)).astype(np.float32), rng.uniform(-40, 40, (n, 3)).astype(np.float32),
                                       substeps=rng.integers(0, 30, n).astype(np.int32), frame="world" if k % 2 else "link")
            act = t.as_tensor(rng.uniform(-1, 1, (n, v.action_dim)).astype(np.float32), device=v.device)
            res.append([x.clone() for x in v.step_tensor(act)] + [v.get_state(), v.get_info("external_wrench")])
        out.append(res)
    for k, (x, y) in enumerate(zip(*out)):
        for i, (p, q) in enumerate(zip(x, y)):
            same(p, q, f"k_step vs k_step_dense, step {k}, output {i}")


def test_reset_cancels_and_next_episode_is_push_free(torch_cuda):
    t = torch_cuda
    n = 16
    kw = dict(auto_reset=True, reset_lookahead=4, env_randomizer_mode="GROUND_RANDOMIZER")
    a, b = vec_env(n, **kw), vec_env(n, **kw)
    a.reset_tensor(); b.reset_tensor()
    F, T = topple_push(n, 2)
    a.apply_external_force(F, T, substeps=np.where(np.arange(n) == 2, 100000, 0).astype(np.int32))
    act = t.zeros((n, a.action_dim), device=a.device)
    for k in range(200):
        _, _, done, _ = a.step_tensor(act)
        if bool(done[2]):
            break
    assert bool(done[2]), "the pushed robot never fell"
    assert a.get_info("external_wrench")[2, 6].item() == 0.0
    # the push-free handle's environment 2 starts its next episode by a reset of its own: keyed by (seed, environment, episode)
    m = np.zeros(n, np.uint8); m[2] = 1
    b.reset_tensor(mask=m)
    same(a.get_state()[2], b.get_state()[2], "next episode's start state")
    same(a.get_info("params")[2], b.get_info("params")[2], "next episode's parameters")
    a.apply_external_force(np.full(3, 50.0, np.float32), substeps=40)
    a.reset_tensor(mask=m)
    assert a.get_info("external_wrench")[2, 6].item() == 0.0 and a.get_info("external_wrench")[0, 6].item() == 40.0


def test_host_and_fused_paths_take_the_push(torch_cuda):
    t = torch_cuda
    n = 16
    kw = dict(body_contacts=True, auto_reset=True, reset_lookahead=0)
    vs = [vec_env(n, **kw) for _ in range(3)]
    for v in vs:
        v.reset_tensor()
    rng = np.random.default_rng(2)
    F = rng.uniform(-300, 300, (n, 3)).astype(np.float32)
    for k in range(4):
        if k in (0, 2):
            for v in vs:
                v.apply_external_force(F if k == 0 else t.as_tensor(F, device=v.device), substeps=15, frame="link" if k else "world")
        a = rng.uniform(-1, 1, (n, vs[0].action_dim)).astype(np.float32)
        at = t.as_tensor(a, device=vs[0].device)
        obs, rew, done, trunc = [x.clone() for x in vs[0].step_tensor(at)]
        o1, r1, d1, _ = vs[1].step(a)
        fused = t.empty((n, vs[2].obs_dim + 2), dtype=t.float32, device=vs[2].device)
        vs[2].step_fused(at, fused)
        same(obs[~done.bool()], o1[~d1], f"obs, host path, step {k}")
        same(rew, r1, f"reward, host path, step {k}")
        same(obs, fused[:, :-2], f"obs, fused, step {k}")
        same(rew, fused[:, -2], f"reward, fused, step {k}")
        same(vs[0].get_state(), vs[1].get_state(), f"state, host path, step {k}")
        same(vs[0].get_state(), vs[2].get_state(), f"state, fused, step {k}")


def test_drop_in_robot_apply_external_force(torch_cuda):
    from qs_amd.env.quadruped_gym_env import QuadrupedGymEnv
    kw = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, noise=False)
    env, ref, plain = QuadrupedGymEnv(**kw), QuadrupedGymEnv(**kw), QuadrupedGymEnv(**kw)
    for e in (env, ref, plain):
        e.reset()
    same(env._vec.get_state(), ref._vec.get_state(), "start")
    f = [120.0, -80.0, 40.0]
    a = np.full(env._vec.action_dim, 0.2, np.float32)
    env.robot.apply_external_force(f)
    ref._vec.apply_external_force(np.asarray(f, np.float32), substeps=1, frame="link")
    info = env._vec.get_info("external_wrench")[0].cpu().numpy()
    assert np.array_equal(info, np.array(f + [0, 0, 0, 1, 1], np.float32)), info
    for e in (env, ref, plain):
        e.step(a)
    same(env._vec.get_state(), ref._vec.get_state(), "drop-in vs batched link-frame one-substep push")
    assert env._vec.get_info("external_wrench")[0, 6].item() == 0.0
    assert not np.array_equal(bits(env._vec.get_state()), bits(plain._vec.get_state()))
    # exactly one substep: the drop-in differs from a push of 2 substeps within this env step (the gate k < remaining)
    longer = QuadrupedGymEnv(**kw)
    longer.reset()
    longer._vec.apply_external_force(np.asarray(f, np.float32), substeps=2, frame="link")
    longer.step(a)
    assert not np.array_equal(bits(env._vec.get_state()), bits(longer._vec.get_state()))
    for e in (env, ref):
        e.step(a)
    same(env._vec.get_state(), ref._vec.get_state(), "second step")


def test_pushing_every_step_never_waits_for_the_device(torch_cuda):
    """device tensors with the default duration, and numpy / list inputs with indices, under torch's sync debug mode "error": no call
    of apply_external_force synchronises the host with the device"""
    t = torch_cuda
    n = 64
    v = vec_env(n)
    v.reset_tensor()
    act = t.zeros((n, v.action_dim), device=v.device)
    F = t.zeros((n, 3), device=v.device)
    F[:, 1] = 50.0
    rng = np.random.default_rng(0)
    hostF = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    t.cuda.synchronize()
    t.cuda.set_sync_debug_mode("error")
    try:
        for k in range(6):
            v.apply_external_force(F)                                                    # device tensor, substeps=None
            v.step_tensor(act)
            v.apply_external_force(hostF, torque=[0.0, 0.0, 1.0], substeps=7, frame="link", indices=[1, 5, 9])   # host data
            v.apply_external_force(F, substeps=t.full((n,), 3, dtype=t.int32, device=v.device), indices=t.arange(4, device=v.device))
            v.step_tensor(act)
    finally:
        t.cuda.set_sync_debug_mode("default")
    info = v.get_info("external_wrench").cpu().numpy()
    np.testing.assert_array_equal(info[5, :3], hostF[5])
    assert info[5, 5] == 1.0 and info[5, 7] == 1.0 and info[0, 7] == 2.0


def test_refused_device_rows_are_reported(torch_cuda):
    t = torch_cuda
    n = 16
    v = vec_env(n)
    v.reset_tensor()
    v.apply_external_force(np.full(3, 20.0, np.float32), substeps=40)
    v.stats()                                  # nothing refused so far
    F = t.zeros((n, 3), device=v.device)
    F[2, 0] = float("nan")
    v.apply_external_force(F, substeps=5)      # a device tensor is not inspected on the host: the kernel refuses the row
    with pytest.raises(RuntimeError, match="refused the row of environment 2"):
        v.stats()
    v.stats()                                  # reported once
    info = v.get_info("external_wrench").cpu().numpy()
    assert info[2, 6] == 40.0 and info[2, 0] == 20.0, "the refused environment keeps its earlier push"
    assert info[3, 6] == 5.0 and info[3, 0] == 0.0
    k = t.full((n,), 4, dtype=t.int32, device=v.device)
    k[7] = -1
    v.apply_external_force(F.nan_to_num(), substeps=k)
    with pytest.raises(RuntimeError, match="refused the row of environment 7"):
        v.counter(0)


def vec_device(cfg, meta):
    """make_device of push_rack_cases.run: a device handle for the case's configuration (from_config takes meta["rack"]), reset"""
    import yardstick as Y
    from qs_amd.vec_env import QuadrupedVecEnv
    v = QuadrupedVecEnv.from_config(cfg, meta)
    v.reset()
    return Y.VecEnvDevice(v)


@pytest.mark.parametrize("case, step_kernel", [("ground_cone", "1"), ("ground_cone", "2"), ("ground_pyramid", None), ("topple", None), ("repeat4", None)])
def test_pushes_against_the_oracle(torch_cuda, monkeypatch, case, step_kernel):
    """push_rack_cases.PUSH_CASES on the device (n = 16, one wave), every step from the oracle's state: strict (pose 5e-6, base velocity
    5e-4, q 2e-5, qd 5e-3; torques, foot forces, observation, reward) where the step map is smooth, tolerance + 5 x |oracle32 - oracle64|
    where a non-foot link touched the ground, the impact rows' 90th and 99th percentile within tolerance + 2 x the float32 oracle's own;
    the remaining-substeps column equal on both oracle builds and the device before and after every step.
    ground_*: default task, a push of +-150 N / +-8 N m every 3rd step for 0, 1, 5 or 25 substeps, world and link frame in turn (at least
    100 compared env-steps with a push active and a foot in contact), cone under either step kernel, pyramid.  topple: 300 - 600 N
    sideways with a roll torque for 60 substeps on half of the environments (at least 30 impact rows).  repeat4: action_repeat = 4,
    time_step = 0.0025, pushes of 25 substeps.  The CPU twins are tests/test_emu_push.py::test_pushes_against_the_oracle."""
    import push_rack_cases as P
    if step_kernel:
        monkeypatch.setenv("QS_STEP_VARIANT", step_kernel)
    P.check(P.run(case, P.PUSH_CASES, vec_device), f"test_gpu_push[{case}-{step_kernel}]")
