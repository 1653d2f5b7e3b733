"""CPU-side checks of the product: the C-ABI library builds, loads and exports every symbol include/qs_amd.h declares
(no compute calls without a GPU), the host registries mirror the reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from qs_amd import config as qcfg
from qs_amd.config import build_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from qs_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("qs_build", os.path.join(REPO, "quadruped-springs_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    header = open(os.path.join(REPO, "include", "qs_amd.h")).read()
    declared = set(re.findall(r"\b(qs_[a-z_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    l = lib.load()
    for name in declared:
        assert hasattr(l, name), f"{name} declared in include/qs_amd.h but not exported"
    assert set(lib.EXPORTS) == declared
    for name, restype, argtypes in lib.SIGNATURES:   # load() binds every row as the table states it (the table against the header: test_abi_cpu.py)
        assert getattr(l, name).restype is restype and tuple(getattr(l, name).argtypes) == argtypes, name


def test_the_library_says_which_sources_it_was_built_from():
    """build.py compiles the fingerprint of the source tree into the library (-DQS_SOURCE_SHA), qs_version() returns it: a profile, a
    bench line and the parity gate's record (profiles/validated_libraries.jsonl) name the binary by what it was compiled from."""
    import importlib.util
    from qs_amd import lib
    spec = importlib.util.spec_from_file_location("qs_build", os.path.join(REPO, "quadruped-springs_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    assert lib.source_sha() == b.source_fingerprint()


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from qs_amd.vec_env import QuadrupedVecEnv
    with pytest.raises(RuntimeError, match="no CPU path"):
        QuadrupedVecEnv(num_envs=2)
    from qs_amd import lib
    cfg, _ = build_config(n_envs=2)
    h = C.c_void_p()
    assert lib.load().qs_create(C.byref(cfg), 0, C.byref(h)) != 0   # the C ABI refuses as well
    assert b"no HIP device" in lib.load().qs_last_error() or b"failed" in lib.load().qs_last_error()


@pytest.mark.parametrize("field,value,needle", [
    ("action_repeat", 0, b"action_repeat must be between 1 and"),
    ("action_repeat", -3, b"action_repeat must be between 1 and"),
    ("action_repeat", 1 << 30, b"action_repeat must be between 1 and"),
    ("settle_steps", -1, b"settle_steps must be between 0 and"),
    ("settle_steps", 1 << 30, b"settle_steps must be between 0 and"),
    ("settle_steps", 0, b"needs settle_steps > 0"),
])
def test_create_refuses_substep_counts_the_step_cannot_run(field, value, needle):
    """qs_create validates the config before it looks for a device: a step's substep index travels with a flag bit above it through the
    hand-over to the full build (Env::RESUME_AT_BOUNDARY = 1 << 30), and the settle lanes' schedule divides by action_repeat and by the
    slices of a settle -- counts outside what that allows are refused with their own message, on any machine."""
    from qs_amd import lib
    cfg, _ = build_config(n_envs=2)
    cfg.reset_lookahead = 16
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.load().qs_create(C.byref(cfg), 0, C.byref(h)) != 0
    assert needle in lib.load().qs_last_error(), lib.load().qs_last_error()
    cfg, _ = build_config(n_envs=2)       # without look-ahead resets a reset settles inside the step: settle_steps = 0 is fine there
    cfg.settle_steps, cfg.reset_lookahead = 0, 0
    assert lib.load().qs_create(C.byref(cfg), 0, C.byref(h)) == 0 or b"settle_steps" not in lib.load().qs_last_error()
    if h.value:
        lib.load().qs_destroy(h)


def test_registries_and_errors_mirror_the_reference():
    cfg, meta = build_config(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True)
    assert cfg.action_dim == 6 and cfg.obs_dim == 28 and cfg.solver_iters == 30 and cfg.settle_steps == 2500
    assert cfg.max_sim_steps == 10000   # sim_time > 10 s first holds at step 10001 (gym_env.py:245)
    assert meta["layout"]["keys"] == ["Encoder", "JointVelocity", "Pitch", "Height", "Base Linear Velocity z direction", "is landing"]
    with pytest.raises(ValueError):
        build_config(motor_control_mode="TORQUE")            # gym_env.py:167-168
    with pytest.raises(KeyError):
        build_config(observation_space_mode="ARS_HEIGHT")    # the reference's broken gym default (quadruped_spring/__init__.py:9)
    with pytest.raises(ValueError):
        build_config(task_env="JUMPING_IN_PLACE_DEMO", demo=np.zeros((5, 7)))   # rows of a demonstration are action_dim + 38 wide
    c4, m4 = build_config(task_env="JUMPING_IN_PLACE_DEMO", demo=np.zeros((5, 44)))
    assert c4.task == 13 and m4["demo"].shape == (5, 44) and m4["demo"].dtype == np.float32
    c2, _ = build_config(time_step=0.002, action_repeat=5, enable_springs=True)
    assert c2.solver_iters == 60 and c2.max_sim_steps == 5000
    # BACKFLIP widens two joint limits in place (motor_interface.py:17-22)
    c3, m3 = build_config(task_env="BACKFLIP", observation_space_mode="PPO_BACKFLIP", enable_springs=True)
    assert abs(c3.cmd_hi[7] - np.pi / 2) < 1e-6 and abs(c3.cmd_hi[10] - np.pi / 2) < 1e-6 and abs(c3.cmd_hi[1] - (np.pi / 4 + 0.5)) < 1e-6
    assert m3["layout"]["high"][7] == pytest.approx(np.pi / 2)


def test_symmetric_action_kat_from_survey():
    """symmetric action [0.3,-0.5,0.9,-1,1,0.1] -> command."""
    from oracle.qso import Oracle
    cfg, _ = build_config(enable_springs=True, task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC")
    cmd = Oracle(cfg).action_to_command([0.3, -0.5, 0.9, -1, 1, 0.1])
    np.testing.assert_allclose(cmd, [0.06, 0.535398, -1.0275, -0.06, 0.535398, -1.0275, -0.2, 1.285398, -1.6475, 0.2, 1.285398, -1.6475], atol=1e-6)


def test_unknown_keywords_are_refused():
    """The reference's constructor raises TypeError for a keyword it does not know (quadruped_gym_env.py:52-70); so does build_config --
    a typo must not silently run another simulation.  Its rendering / curriculum keywords are accepted and unused."""
    import pytest
    from qs_amd.config import build_config
    with pytest.raises(TypeError):
        build_config(n_envs=1, enable_spring=True)          # (enable_springs)
    with pytest.raises(TypeError):
        build_config(n_envs=1, reset_lookahead=4)           # (a QuadrupedVecEnv keyword, not a configuration field)
    cfg, _ = build_config(n_envs=1, camera_mode="CLASSIC", curriculum_level=0.3, verbose=1, on_rack=False, render=False)
    assert cfg.n_envs == 1
    with pytest.raises(NotImplementedError):
        build_config(n_envs=1, render=True)


def test_robot_view_getters_follow_the_reference_formulas():
    """The getters of quadruped.py that need no simulation step -- orientation matrix, body-frame angular velocity (quadruped.py:141-175),
    the springs' real stiffness / damping under the unilateral gating (springs.py:28-74), URDF masses (go1.urdf: 12.01301 kg), the
    payload block's offset -- on a stand-in for the device handle: plain formulas, checked against scipy's rotation and by hand."""
    import math
    from types import SimpleNamespace

    import torch
    from scipy.spatial.transform import Rotation

    from qs_amd.env.quadruped_gym_env import _RobotView
    from qs_amd.go1_config import make_config

    rng = np.random.default_rng(0)
    quat = Rotation.random(random_state=1).as_quat()          # xyzw, as PyBullet
    state = np.zeros(37); state[0:3] = [0.1, -0.2, 0.31]; state[3:7] = quat; state[10:13] = [0.3, -1.1, 0.7]
    q = np.tile([0.0, math.pi / 4, -math.pi / 2 + 0.3], 4) + np.array([0.1, 0.1, 0.1, 0.1, -0.1, -0.1, -0.1, 0.1, 0.1, -0.1, -0.1, -0.1])
    state[13:25] = q
    params = np.zeros(24); params[1:4] = [20, 20, 30]; params[4:7] = 0.3; params[7:10] = [0.0, math.pi / 4, -math.pi / 2 + 0.3]
    params[20] = 1.5; params[21:24] = [0.05, -0.02, 0.1]

    class Vec:
        cfg = SimpleNamespace(payload_soft=0)
        def get_state(self): return torch.tensor(state[None])
        def get_info(self, which): assert which == "params"; return torch.tensor(params[None])

    env = SimpleNamespace(_vec=Vec(), _replay_row=None, _robot_config=make_config(True), _enable_springs=True)
    r = _RobotView(env)
    R = Rotation.from_quat(quat).as_matrix()
    np.testing.assert_allclose(r.GetBaseOrientationMatrix(), R, atol=1e-12)
    np.testing.assert_allclose(r.GetTrueBaseRollPitchYawRate(), R.T @ state[10:13], atol=1e-12)
    assert r.getHeight() == 0.31
    k, b, rest = r.get_spring_real_stiffness_and_damping()
    # FR (right): hip 0.1 > rest -> off, thigh above rest -> on, calf above rest -> off; FL (left): hip 0.1 > rest -> on, thigh below -> off, calf below -> on
    np.testing.assert_allclose(k[:6], [0, 20, 0, 20, 0, 30]); np.testing.assert_allclose(b[:6], [0, 0.3, 0, 0.3, 0, 0.3])
    # RR (right): hip -0.1 -> on, thigh above -> on, calf above -> off; RL (left): hip -0.1 < rest -> off, thigh below -> off, calf below -> on
    np.testing.assert_allclose(k[6:], [20, 20, 0, 0, 0, 30]); np.testing.assert_allclose(rest, np.tile(params[7:10], 4))
    assert abs(sum(r.GetTotalMassFromURDF()) - 12.01301) < 1e-9 and len(r.GetTotalMassFromURDF()) == 19     # base + 18 links
    assert r.GetBaseMassFromURDF() == [5.204] and len(r.GetLegMassesFromURDF()) == 12 and r.GetFootMassesFromURDF() == [0.06] * 4
    assert r.get_offset_mass_value() == 1.5
    np.testing.assert_allclose(r.get_offset_mass_position(), R @ params[21:24], atol=1e-12)
    env._enable_springs = False
    assert not r.get_spring_real_stiffness_and_damping()[0].any()


def _load_build_module():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("qs_build_under_test", os.path.join(repo, "quadruped-springs_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, repo


def test_touching_any_source_makes_the_build_recompile(tmp_path):
    """build.py decides by modification times whether libqs_hip.so is current.  Round 4 kept the list of sources by hand and qs_rare.h was
    not on it: every file under csrc/, every public header and every quoted #include of the .hip files must count."""
    b, repo = _load_build_module()
    deps = b.deps()
    csrc = os.path.join(repo, "quadruped-springs_amd", "csrc")
    for f in os.listdir(csrc):
        assert os.path.join(csrc, f) in deps, f
    for f in os.listdir(os.path.join(repo, "include")):
        assert os.path.join(repo, "include", f) in deps, f
    names = {os.path.basename(d) for d in deps}
    for d in deps:
        if d.endswith((".hip", ".h")):
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(d).read(), re.M):
                assert os.path.basename(inc) in names, (d, inc)
    out = tmp_path / "lib.so"
    out.write_bytes(b"x")
    newest = max(os.path.getmtime(d) for d in deps)
    os.utime(out, (newest + 1, newest + 1))
    assert not b.needs_build(str(out))
    for d in deps:                      # a library older than ANY one of them is stale
        t = os.path.getmtime(d) - 1
        os.utime(out, (t, t))
        assert b.needs_build(str(out)), d
    assert b.needs_build(str(tmp_path / "missing.so"))
    assert len(b.fingerprint(str(out))) == 64


def test_the_build_does_not_pass_split_spill_mode():
    """Round 5: the first library with the many-rows solver's core<0, 4> came out of `-mllvm -split-spill-mode=size` miscompiled (caught by the
    GPU parity gates); the option is out of the build and must not come back as a flag (the comment that says why may name it)."""
    b, repo = _load_build_module()
    text = open(os.path.join(repo, "quadruped-springs_amd", "build.py")).read()
    assert '"-split-spill-mode' not in text and "'-split-spill-mode" not in text
    assert "split-spill-mode" not in os.environ.get("QS_HIPCC_EXTRA", "")
    # round 6: its partner -greedy-regclass-priority-trumps-globalness=1 went too (+0.5 % / -0.4 % on the two headline figures: noise)
    assert '"-greedy-regclass-priority' not in text and "'-greedy-regclass-priority" not in text


def test_gate_record_reads_a_gate_run(tmp_path, capsys):
    """tools/gate_record.py (the verdict of tools/gate.sh): accepted only if both pytest runs passed, every fuzz mode ran with 0 deviated, the
    soak said ok and the library reports the tree's source fingerprint; the JSON line carries library_sha256 / source_sha256."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("gate_record", os.path.join(REPO, "tools", "gate_record.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    out = tmp_path / "run"
    os.makedirs(out)
    for f in ("pytest_default.log", "pytest_dense.log"):
        (out / f).write_text("....\n153 passed, 237 deselected in 350.00s (0:05:50)\nRCCL version : 2.26.6\nLibrccl path : /x/librccl.so\n")   # (the banner of the one-rank RCCL test comes last)
    for k in ("plain", "fallen", "lookahead", "fallen_dense"):
        (out / f"fuzz_{k}.log").write_text("case 0 ...\n250 configurations ran, 0 deviated\n")
    (out / "soak.log").write_text("step 300000: 63 M env-steps/s\nok\n")
    assert g.main(str(out), "quick", jsonl_dir=str(tmp_path)) == 0
    rec = json.loads(open(tmp_path / "validated_libraries.jsonl").read().splitlines()[-1])
    assert rec["accepted"] and rec["deviated"] == 0 and len(rec["library_sha256"]) == 64 and rec["source_sha256"] == rec["tree_sha256"]
    (out / "fuzz_fallen.log").write_text("250 configurations ran, 3 deviated\n")
    assert g.main(str(out), "quick", jsonl_dir=str(tmp_path)) == 1
    assert not json.loads(open(tmp_path / "validated_libraries.jsonl").read().splitlines()[-1])["accepted"]
    capsys.readouterr()


def test_design_md_stays_a_design():
    """DESIGN.md is the CURRENT design -- at most 400 lines, prose within 160 columns (a table row is one line by
    definition) -- and the history lives in EXPERIMENTS.md, which it points to."""
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    lines = text.split("\n")
    assert len(lines) <= 400, len(lines)
    long = [(i + 1, len(l)) for i, l in enumerate(lines) if len(l) > 160 and not l.startswith("|")]
    assert not long, long
    assert "EXPERIMENTS.md" in text and os.path.exists(os.path.join(REPO, "EXPERIMENTS.md"))
    for section in ("## 1.", "## 2.", "## 3.", "## 4.", "### 4a.", "## 5.", "## 6.", "## 7.", "## 8.", "## 9.", "## 10."):
        assert section in text, section
