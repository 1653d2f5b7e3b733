"""The step kernels' hand-over on the host (tests/emu/qs_emu_step.cpp): the common-path build of Env::step that k_step / k_step_dense run
first, and the full build's step<true>(..., resume) that goes on from the substep where it gave up, against the full build's step from
the same records -- bit for bit (qs_env.h, Env::step).  Mid-substep hand-overs (a vote of substep k gave up) and boundary ones (substep
k - 1 predicted the rare path: RESUME_AT_BOUNDARY), the CONE / SOFT / LEAN builds launch_step launches, hand-overs late in a long step, and
the settle lanes' slices."""
import numpy as np
import pytest

from qs_amd.config import build_config
from emu.emu import Emu

RAW = dict(task_env="NO_TASK", observation_space_mode="ENCODER", enable_action_filter=False, isRLGymInterface=False, motor_control_mode="TORQUE")
CALF_BEYOND_STOP = -2.76    # FR calf beyond its lower stop (-2.7227): the limit row is there from the first substep


def fallen_states(s, rng, z=None):
    """robots on their side, back, front, hips: the attitudes of tests/test_gpu_round2.py::fallen_states"""
    from scipy.spatial.transform import Rotation as Rot
    n = len(s)
    s = s.copy()
    s[:, :3] = 0.0
    s[:, 2] = rng.uniform(0.16, 0.3, n) if z is None else z
    eul = np.stack([rng.choice([0.0, 1.45, -1.45, 3.0, 0.7], n), rng.uniform(-0.5, 0.5, n), np.zeros(n)], 1)
    s[:, 3:7] = Rot.from_euler("xyz", eul).as_quat()
    s[:, 7:] = 0
    s[:, 13:25] = np.tile([0.0, 1.2, -2.4], 4)
    return s


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def assert_bitwise(a, b, what):
    assert np.array_equal(bits(a), bits(b)), f"{what}: {np.argwhere(bits(a) != bits(b))[:8].tolist()}"


class Pair:
    """the same configuration twice: `full` steps with the full build (qse_step), `hot` with the step kernel's builds (qse_step_build)"""

    def __init__(self, cfg, meta=None, trace_env=None):
        self.cfg = cfg
        self.full, self.hot = Emu(cfg), Emu(cfg)
        if meta is not None and meta.get("demo") is not None:
            self.full.set_demo(meta["demo"]); self.hot.set_demo(meta["demo"])
        self.full.reset(); self.hot.reset()
        self.tr = None if trace_env is None else (self.full.set_trace(trace_env), self.hot.set_trace(trace_env))
        self.resumes = []

    def set_state(self, s):
        self.full.set_state(s); self.hot.set_state(s)
        assert_bitwise(self.full.records(), self.hot.records(), "records before the step")

    def step(self, act, variant, t=0):
        rf = self.full.step(act)
        rh = self.hot.step_hot(act, variant)
        for name, x, y in zip(("obs", "reward", "done", "truncated"), rf, rh[:4]):
            assert_bitwise(x, y, f"{name}, step {t}")
        assert_bitwise(self.full.records(), self.hot.records(), f"records, step {t}")
        if self.cfg.auto_reset:
            assert_bitwise(self.full.get_term_obs(), self.hot.get_term_obs(), f"terminal observations, step {t}")
        if self.tr is not None:
            assert_bitwise(self.tr[0], self.tr[1], f"trace rows, step {t}")
        self.resumes.append(rh[4].copy())
        return rh

    def kinds(self):
        """(substeps of the mid-substep hand-overs, substeps of the boundary ones) over the run"""
        r = np.concatenate(self.resumes)
        flag = self.hot.resume_at_boundary()
        r = r[r >= 0]
        at = (r & flag) != 0
        return r[~at], r[at] & (flag - 1)


def throw(pair, rng, lying_every=2):
    """half the robots thrown over, one robot with a joint beyond its stop, the others standing with their joints nudged"""
    s = pair.full.get_state()
    n = len(s)
    s[:, 13:25] += rng.uniform(-0.1, 0.1, size=(n, 12)).astype(np.float32)
    lying = np.arange(n) % lying_every == 1
    s[lying] = fallen_states(s[lying], rng)
    s[0, 13 + 2] = CALF_BEYOND_STOP
    pair.set_state(s.astype(np.float32))


def actions(cfg, rng):
    if not cfg.rl_interface:
        return (4.0 * rng.normal(size=(cfg.n_envs, cfg.action_dim))).astype(np.float32)
    return rng.uniform(-1, 1, size=(cfg.n_envs, cfg.action_dim)).astype(np.float32)


def run(kw, variant, steps=12, n=8, seed=0):
    rng = np.random.default_rng(seed)
    if kw.get("task_env", "").endswith("_DEMO"):
        d = {"CPG": 5, "DEFAULT": 12, "SYMMETRIC": 6, "SYMMETRIC_NO_HIP": 4}[kw.get("action_space_mode", "SYMMETRIC")]
        kw = dict(kw, demo=rng.uniform(-1, 1, size=(40, d + 38)).astype(np.float32))
    cfg, meta = build_config(n_envs=n, **kw)
    p = Pair(cfg, meta, trace_env=1)
    throw(p, rng)
    for t in range(steps):
        p.step(actions(cfg, rng), variant, t)
    assert any((r >= 0).any() for r in p.resumes), "no step was handed over: the test proves nothing"
    return p


BASE = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, enable_action_filter=True, settle_steps=200,
            noise=True, auto_reset=True)
CASES = {
    "cone_k_step": (dict(BASE), 1),
    "cone_dense_cartesian12_resid0": (dict(BASE, action_space_mode="DEFAULT", motor_control_mode="CARTESIAN_PD", solver_residual_threshold=0.0), 2),
    "pyramid_nohip4_auto_contacts": (dict(BASE, task_env="JUMPING_FORWARD", action_space_mode="SYMMETRIC_NO_HIP", friction_model="pyramid",
                                          body_contacts="auto"), 1),
    "pyramid_dense_torque": (dict(RAW, friction_model="pyramid", body_contacts="auto", settle_steps=200), 2),
    "cone_soft_k_step": (dict(BASE, payload="soft", env_randomizer_mode="MASS_RANDOMIZER"), 1),
    "cone_soft_dense": (dict(BASE, payload="soft", solver_residual_threshold=0.0), 2),
    "cpg": (dict(BASE, action_space_mode="CPG"), 1),
    "cpg_dense": (dict(BASE, action_space_mode="CPG"), 2),
    "landing": (dict(BASE, wrapper="LANDING"), 1),
    "go_to_rest_dense": (dict(BASE, wrapper="GO_TO_REST", friction_model="pyramid"), 2),
    "demo": (dict(BASE, task_env="JUMPING_IN_PLACE_DEMO"), 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_hand_over_gives_the_full_build_bit_for_bit(case):
    kw, variant = CASES[case]
    p = run(kw, variant, seed=len(case))
    mid, at = p.kinds()
    assert len(mid) > 0, "no mid-substep hand-over"
    if case.startswith("cone_k_step") or case.startswith("cpg"):
        assert len(at) > 0, "no boundary hand-over (for CPG: the resume_ticked branch never ran)"


@pytest.mark.parametrize("variant", [1, 2])
def test_pyramid_with_the_soft_payload_hands_over_at_substep_0(variant):
    """the pyramid has no common-path build with the block's rows: every step of such a handle goes on in the full build from substep 0"""
    p = run(dict(BASE, payload="soft", friction_model="pyramid"), variant, steps=6, seed=3)
    assert all((r == 0).all() for r in p.resumes), p.resumes


WRAPPERS = [None, "LANDING", "GO_TO_REST", "LANDING2", "LANDING_BACKFLIP", "LANDING_BACKFLIP2", "LANDING_CONTINUOUS"]


def draw(rng):
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    kw = dict(task_env=pick(["JUMPING_IN_PLACE", "JUMPING_FORWARD", "NO_TASK", "BACKFLIP", "CONTINUOUS_JUMPING_FORWARD"]),
              observation_space_mode=pick(["PPO_BASIC", "ENCODER", "ARS_BASIC"]), action_space_mode=pick(["DEFAULT", "SYMMETRIC", "SYMMETRIC_NO_HIP", "CPG"]),
              motor_control_mode=pick(["PD", "CARTESIAN_PD", "TORQUE"]), wrapper=pick(WRAPPERS), friction_model=pick(["cone", "pyramid"]),
              solver_residual_threshold=pick([0.0, 1e-7]), body_contacts=pick([True, "auto"]), enable_springs=bool(rng.integers(2)),
              enable_action_filter=bool(rng.integers(2)), payload=pick(["weld", "soft"]), env_randomizer_mode=pick(["NONE", "GROUND_RANDOMIZER", "MASS_RANDOMIZER"]),
              noise=bool(rng.integers(2)), auto_reset=bool(rng.integers(2)), seed=int(rng.integers(1000)), settle_steps=150)
    if kw["motor_control_mode"] == "TORQUE":
        kw.update(isRLGymInterface=False, action_space_mode="DEFAULT", wrapper=None)
    if kw["action_space_mode"] == "CPG":
        kw.update(wrapper=None)
    if rng.integers(3) == 0:
        kw.update(time_step=0.002, action_repeat=5)
    return kw, int(rng.integers(1, 3))


@pytest.mark.parametrize("seed", list(range(4)))
def test_random_configurations_hand_over_bit_for_bit(seed):
    rng = np.random.default_rng(100 + seed)
    ran = 0
    while ran < 3:
        kw, variant = draw(rng)
        try:
            build_config(n_envs=1, **kw)
        except (ValueError, KeyError):          # combinations the reference refuses
            continue
        ran += 1
        run(kw, variant, steps=8, seed=int(rng.integers(1 << 30)))


LATE = {"cone": (dict(), 1), "pyramid": (dict(friction_model="pyramid"), 1), "cone_dense": (dict(), 2),
        "cone_soft": (dict(payload="soft", env_randomizer_mode="MASS_RANDOMIZER"), 1)}


@pytest.mark.parametrize("action_repeat", [255, 256, 300])
@pytest.mark.parametrize("case", list(LATE))
def test_late_hand_over(case, action_repeat):
    """A long env step (time_step 0.001, action_repeat up to 300, the reference's int(300 / action_repeat) solver iterations): robots on
    their side dropped from heights at which their first body contact comes 237 - 294 substeps into the first step, so the hand-over comes
    at a substep index beyond 255 where the step is long enough."""
    extra, variant = LATE[case]
    cfg, _ = build_config(n_envs=8, time_step=0.001, action_repeat=action_repeat, settle_steps=200, noise=False,
                          **{**RAW, "body_contacts": True, "env_randomizer_mode": "NONE", **extra})
    assert cfg.solver_iters == int(300 / action_repeat)
    p = Pair(cfg, trace_env=5)
    rng = np.random.default_rng(action_repeat)
    s = p.full.get_state()
    drop = np.arange(8) % 2 == 1
    s[drop] = fallen_states(s[drop], rng, z=np.array([0.45, 0.5, 0.55, 0.6]))
    s[drop, 3:7] = [0.6631, 0.0, 0.0, 0.7485]     # all on their side (roll ~1.45 rad)
    p.set_state(s.astype(np.float32))
    for t in range(3):
        p.step(np.zeros((8, 12), np.float32), variant, t)
    mid, at = p.kinds()
    ks = np.concatenate([mid, at])
    assert (ks >= 0).all() and (ks < action_repeat).all(), ks
    if action_repeat > 256:
        assert (ks >= 256).any(), f"no hand-over beyond substep 255: {sorted(ks)}"
    else:
        assert (ks >= 200).any(), f"no late hand-over: {sorted(ks)}"


@pytest.mark.parametrize("case", ["cone", "pyramid_dense", "cone_soft_dense", "pyramid_soft"])
def test_settle_slices_hand_over_bit_for_bit(case):
    """A reset's settle in the slices the settle lanes run (settle_steps = 253 with action_repeat 10: 25 slices of 10 substeps and a last
    one of 3), the first one with the spawn, from spawns that need the rare path (robots thrown over, a joint beyond its stop)."""
    kw = dict(BASE, settle_steps=253, auto_reset=False)
    variant = 2 if case.endswith("dense") else 1
    if "pyramid" in case:
        kw["friction_model"] = "pyramid"
    if "soft" in case:
        kw.update(payload="soft", env_randomizer_mode="MASS_RANDOMIZER")
    cfg, _ = build_config(n_envs=8, **kw)
    p = Pair(cfg)
    rng = np.random.default_rng(7)
    rep = cfg.action_repeat
    epoch = (cfg.settle_steps + rep - 1) // rep
    slices = [rep] * (epoch - 1) + [cfg.settle_steps - rep * (epoch - 1)]
    assert slices[-1] == 3
    resumes = []
    for i, n_sub in enumerate(slices):
        p.full.settle_slice(n_sub, spawn=i == 0, variant=0)
        r = p.hot.settle_slice(n_sub, spawn=i == 0, variant=variant)
        resumes.append(r)
        assert_bitwise(p.full.records(), p.hot.records(), f"records, slice {i} of {n_sub} substeps")
        if i == 0:          # the spawn is in place: now throw the robots over (both handles alike)
            throw(p, rng)
    r = np.concatenate(resumes)
    assert (r >= 0).sum() > len(slices), "the settle was hardly handed over: the test proves little"
    if case == "pyramid_soft":
        assert (r == 0).all()
    else:
        assert ((r >= 0) & ((r & p.hot.resume_at_boundary()) == 0)).any()


@pytest.mark.parametrize("rack", [False, True])
@pytest.mark.parametrize("payload", ["weld", "soft"])
def test_launch_sizes_the_tile_as_the_kernel_strides_it(rack, payload):
    """step_body spells the record stride of its LDS tile out (going through qs::Build changes the step kernels' register allocation);
    launch_step sizes the LDS by qs::Build::step_lds_bytes.  The two statements agree for every (rack, payload_soft), and the kernel's
    line is still the one this test restates."""
    import os
    from emu.emu import build_stride
    if rack and payload == "soft":
        cfg, _ = build_config(n_envs=16, payload="weld", **RAW)     # (qs_create_ex refuses the pair; the rule is total all the same)
        cfg.payload_soft = 1
    else:
        cfg, _ = build_config(n_envs=16, payload=payload, **RAW)
    assert bool(cfg.payload_soft) == (payload == "soft")
    stride, lds_bytes, rec_end, info_end = build_stride(cfg, rack)
    src = open(os.path.join(os.path.dirname(__file__), "..", "quadruped-springs_amd", "csrc", "qs_hip.hip")).read()
    assert "const int ls = (RACK || cfg.payload_soft) ? (int)QS_REC_END : (int)QS_INFO_END;" in src
    assert "s_obs = s_dyn + QS_ENVS_PER_WAVE * ls;" in src and "s_act = s_obs + QS_ENVS_PER_WAVE * QS_MAX_OBS;" in src
    assert stride == (rec_end if (rack or cfg.payload_soft) else info_end) and info_end < rec_end
    max_obs = 64    # QS_MAX_OBS (include/qs_amd.h); the action rows: 12 floats
    assert lds_bytes == 16 * (stride + max_obs + 12) * 4
