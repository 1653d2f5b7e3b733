"""Camera images without a GPU: the float64 numpy reference (tests/render_ref.py) against the oracle's kinematics and known answers, the
host build of csrc/qs_render.h (tests/emu/qs_emu_render.cpp) against the reference, and the Python surface (qs_camera layout, argument
checks, tile_images, camera_mode)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_ref as R  # noqa: E402
from emu import emu_render  # noqa: E402
from oracle.qso import Oracle  # noqa: E402
from qs_amd.config import build_config  # noqa: E402
from qs_amd.lib import QsCamera  # noqa: E402
from qs_amd.render import CAMERA_MODES, Camera, check_request, tile_images  # noqa: E402

W, H = 160, 120
RAW = dict(task_env="NO_TASK", observation_space_mode="CARTESIAN_NO_IMU", enable_action_filter=False, isRLGymInterface=False,
           motor_control_mode="TORQUE", env_randomizer_mode="NONE", noise=False)


def params_with_payload(mass=1.5, offset=(0.05, -0.02, 0.09)):
    p = np.zeros(24, np.float32)
    p[20] = mass
    p[21:24] = offset
    return p


@pytest.fixture(scope="module")
def states():
    """standing (settled), mid-air, fallen on its side and on its back (settled by the oracle), random joint angles"""
    cfg, _ = build_config(n_envs=1, **RAW)
    o = Oracle(cfg)
    o.reset()
    stand = o.get_state()[0].copy()
    out = [("standing", stand)]
    air = stand.copy()
    air[2] += 0.5
    out.append(("mid-air", air))
    rng = np.random.default_rng(3)
    for name, rot in (("side", Rotation.from_euler("x", 90, degrees=True)), ("back", Rotation.from_euler("x", 180, degrees=True))):
        s = stand.copy()[None]
        s[0, 2] = 0.35
        s[0, 3:7] = rot.as_quat()
        s[0, 7:13] = 0.0
        s[0, 25:37] = 0.0
        o.set_state(s)
        for _ in range(60):
            o.step(np.zeros((1, 12), np.float32))
        out.append((name, o.get_state()[0].copy()))
    for k in range(8):
        s = stand.copy()
        s[0:2] = rng.uniform(-2, 2, 2)
        s[2] = rng.uniform(0.15, 0.9)
        s[3:7] = Rotation.random(random_state=k).as_quat() if k % 2 else Rotation.from_euler("z", rng.uniform(-3, 3)).as_quat()
        s[13:25] = rng.uniform(-1.5, 1.5, 12)
        out.append((f"random{k}", s))
    return [(n, np.asarray(s, np.float32)) for n, s in out]


def cam_c(mode, draw_payload=True, **over):
    c = Camera.from_mode(mode)
    for k, v in over.items():
        setattr(c, k, v)
    c.draw_payload = draw_payload
    return c.to_c()


def test_reference_feet_match_the_oracle():
    """the reference's foot-sphere centres, relative to the hip joints in the base frame, against the oracle's feet positions (its sensor
    takes the link lengths of the robot config, whose hip offset is 0.0847 where go1.urdf's thigh joint sits 0.08 out: the URDF's here)"""
    cfg, _ = build_config(n_envs=1, **RAW)
    assert abs(cfg.leg_len[1] - 0.213) < 1e-6 and abs(cfg.leg_len[2] - 0.213) < 1e-6
    cfg.leg_len[0] = R.THIGH_Y
    o = Oracle(cfg)
    o.reset()
    rng = np.random.default_rng(0)
    for step in range(6):
        obs = o.get_obs()[0]
        st = o.get_state()[0]
        for leg in range(4):
            (ph, _), _, _, foot = R.leg_frames(leg, st[13 + 3 * leg: 16 + 3 * leg])
            np.testing.assert_allclose(foot - ph, obs[3 * leg: 3 * leg + 3], atol=1e-6, rtol=0)
        o.step(rng.uniform(-5, 5, (1, 12)).astype(np.float32))


def test_emulation_matches_reference(states):
    """every state under all three camera modes, and with a payload block, at 160 x 120"""
    par = params_with_payload()
    for name, s in states:
        for mode in CAMERA_MODES:
            for p in (None, par):
                rgb, depth, seg = emu_render.render(s[None], cam_c(mode), W, H, None if p is None else p[None])
                ref = R.render(s, mode, W, H, params=p)
                msg = R.compare(ref, rgb[0], depth[0], seg[0])
                assert msg is None, f"{name} {mode} payload={p is not None}: {msg}"


def test_emulation_scene_matches_reference(states):
    for name, s in states[:6]:
        par = params_with_payload()
        tab, bounds = emu_render.scene(s, par)
        prims = R.scene(s, par)
        assert len(prims) == 22
        for k, (typ, pid, Rw, c, e) in enumerate(prims):
            kind = int(tab[k, 15])
            row = k if k == 0 else (21 if pid == 18 else None)
            if row is None:
                continue
            assert kind & 15 == typ and kind >> 4 == pid
            np.testing.assert_allclose(tab[k, 9:12], c, atol=1e-5)
            np.testing.assert_allclose(tab[k, 0:9].reshape(3, 3), Rw, atol=1e-5)
        # every reference primitive appears in the table
        cs = tab[:, 9:12]
        for typ, pid, Rw, c, e in prims:
            k = int(np.argmin(np.linalg.norm(cs - c, axis=1) + 10 * (tab[:, 15].astype(int) >> 4 != pid)))
            np.testing.assert_allclose(cs[k], c, atol=1e-5)
            assert np.linalg.norm(cs[k] - s[:3]) <= bounds[k] + 1e-6


def test_classic_centre_ray_goes_through_the_base(states):
    s = states[0][1]
    cam = R.camera("CLASSIC", s[:3], W, H)
    d = R.rays(cam, np.array([W / 2 - 0.5]), np.array([H / 2 - 0.5]))[0]
    to_base = s[:3] - cam["eye"]
    assert np.linalg.norm(np.cross(d, to_base)) / np.linalg.norm(d) < 1e-9
    for img in (R.render(s, "CLASSIC", W, H)[2], emu_render.render(s[None], cam_c("CLASSIC"), W, H)[2][0]):
        assert img[H // 2, W // 2] == 1


def test_floor_depth_is_the_plane_intersection(states):
    s = states[1][1]
    _, depth, seg = emu_render.render(s[None], cam_c("BACKFLIP"), W, H)
    cam = R.camera("BACKFLIP", s[:3], W, H)
    for col, row in ((5, H - 3), (W - 4, H - 10), (W // 2, H - 1), (20, H - 30)):
        assert seg[0, row, col] == 0
        d = R.rays(cam, np.array([col]), np.array([row]))[0]
        t = -cam["eye"][2] / d[2]     # d has unit depth along the view axis
        assert abs(depth[0, row, col] - t) <= 1e-5 * t


def test_foot_centroid_sits_at_its_projection(states):
    """legs straight down, seen from below: every foot sphere lies in front of its calf, and its pixels' centroid is its projected centre"""
    s = states[0][1].copy()
    s[0:3] = [0.0, 0.0, 1.0]
    s[3:7] = [0, 0, 0, 1]
    s[13:25] = 0.0
    big_w, big_h = 640, 480
    mode = (0.9, 0.0, 89.0, 60.0, None)
    c = QsCamera()
    c.distance, c.yaw_deg, c.pitch_deg, c.fov_deg, c.near_clip, c.far_clip, c.follow_base, c.draw_payload = 0.9, 0.0, 89.0, 60.0, 0.1, 100.0, 1, 1
    ref = R.render(s, mode, big_w, big_h)
    _, _, seg = emu_render.render(s[None], c, big_w, big_h)
    cam = R.camera(mode, s[:3], big_w, big_h)
    for leg in range(4):
        fid = 2 + 4 * leg + 3
        _, _, _, foot = R.leg_frames(leg, s[13 + 3 * leg: 16 + 3 * leg])
        u, v = R.project(cam, s[:3] + foot)
        for img in (ref[2], seg[0]):
            rr, cc = np.nonzero(img == fid)
            assert rr.size > 100
            assert abs(cc.mean() + 0.5 - u) < 1.0 and abs(rr.mean() + 0.5 - v) < 1.0, (leg, cc.mean() + 0.5, u, rr.mean() + 0.5, v)


def test_shadow_lands_where_the_light_puts_it(states):
    s = states[0][1].copy()
    s[2] += 0.5
    s[3:7] = [0, 0, 0, 1]
    mode = (3.0, 0.0, -60.0, 60.0, None)   # from above and behind, so that the shadow is in view
    cam = R.camera(mode, s[:3], W, H)
    L = R.LIGHT
    centre = s[:3] - L * (s[2] / L[2])     # the trunk centre's shadow on the floor
    u, v = R.project(cam, centre)
    col, row = int(u), int(v)
    c = QsCamera()
    c.distance, c.yaw_deg, c.pitch_deg, c.fov_deg, c.near_clip, c.far_clip, c.follow_base, c.draw_payload = 3.0, 0.0, -60.0, 60.0, 0.1, 100.0, 1, 1
    rgb, _, seg = emu_render.render(s[None], c, W, H)
    ref = R.render(s, mode, W, H)
    assert ref[2][row, col] == 0 and seg[0, row, col] == 0 and ref[3][row, col], "the floor under the light ray through the trunk is shadowed"
    # shadowed floor is ambient-lit: darker than the same checker square's lit neighbours
    lit = R.render(s * np.r_[1, 1, 0, np.ones(34)].astype(np.float32) + np.r_[0, 0, -5.0, np.zeros(34)].astype(np.float32), mode, W, H)
    assert int(rgb[0, row, col].sum()) < int(lit[0][row, col].sum())


def test_camera_formula_yaw_pitch_zero():
    """yaw = pitch = 0: the eye sits at target - (0, distance, 0), looking along +y, up +z (pins the reading of Bullet's view matrix)"""
    target = np.array([0.3, -0.2, 0.4])
    cam = R.camera((2.0, 0.0, 0.0, 60.0, tuple(target)), np.zeros(3), W, H)
    np.testing.assert_allclose(cam["eye"], target - [0, 2.0, 0], atol=1e-12)
    np.testing.assert_allclose(cam["fwd"], [0, 1, 0], atol=1e-12)
    np.testing.assert_allclose(cam["right"], [1, 0, 0], atol=1e-12)
    # the host build, robot out of sight: the floor depth at the bottom centre pixel is that of the reference's ray from that eye
    st = np.zeros(37, np.float32)
    st[2] = -50.0   # robot far below the floor: only floor and sky
    st[6] = 1.0
    c = QsCamera()
    c.target[0], c.target[1], c.target[2] = target
    c.distance, c.yaw_deg, c.pitch_deg, c.fov_deg, c.near_clip, c.far_clip, c.follow_base, c.draw_payload = 2.0, 0.0, 0.0, 60.0, 0.1, 100.0, 0, 1
    _, depth, seg = emu_render.render(st[None], c, W, H)
    row, col = H - 1, W // 2
    d = R.rays(cam, np.array([col]), np.array([row]))[0]
    assert seg[0, row, col] == 0
    assert abs(depth[0, row, col] - (-target[2] / d[2])) < 1e-5
    assert np.all(seg[0, : H // 2] == -1), "the horizon is at the image centre for pitch 0"


def test_bindings_refuse_bad_requests():
    with pytest.raises(KeyError):
        Camera.from_mode("SIDEWAYS")
    for w, h in ((0, 10), (10, 0), (8193, 10), (10, 9000), (10.5, 10)):
        with pytest.raises(ValueError):
            check_request(1, w, h)
    with pytest.raises(ValueError, match="render_indices or render_size"):
        check_request(8192, 1440, 1080, "render_indices or render_size")
    check_request(172, 1440, 1080)          # 172 frames of 1440 x 1080: 1.070e9 bytes, just under 1 GiB
    with pytest.raises(ValueError):
        check_request(173, 1440, 1080)
    from qs_amd.render import as_camera
    with pytest.raises(TypeError):
        as_camera(3)


def test_c_abi_refuses_bad_arguments():
    """qs_render_states checks its arguments before it touches the device (this runs without one)"""
    from qs_amd import lib
    L = lib.load()
    good = Camera.from_mode("CLASSIC").to_c()
    buf = C.c_void_p(8)   # never dereferenced: the checks come first

    def call(m=1, cam=good, w=16, h=16, rgba=buf, states=buf):
        return L.qs_render_states(states, None, m, C.byref(cam) if cam is not None else None, w, h, rgba, None, None, None)

    assert call(m=-1) < 0 and b"negative" in L.qs_last_error()
    assert call(w=0) < 0 and call(h=8193) < 0
    assert call(rgba=None) < 0 and b"rgba" in L.qs_last_error()
    for fov in (0.0, 180.0, -5.0):
        c = Camera.from_mode("CLASSIC")
        c.fov = fov
        assert call(cam=c.to_c()) < 0 and b"fov" in L.qs_last_error()
    c = Camera.from_mode("CLASSIC")
    c.near = 0.0
    assert call(cam=c.to_c()) < 0
    assert call(cam=None) < 0
    assert call(m=0) == 0                   # nothing to draw
    assert L.qs_render(None, None, 1, C.byref(good), 16, 16, buf, None, None) < 0


def test_tile_images_matches_sb3_layout():
    imgs = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    out = tile_images(imgs)
    rows, cols = 3, 2                       # ceil(sqrt(5)) rows, ceil(5 / 3) columns
    assert out.shape == (rows * 2, cols * 3, 3)
    for i in range(rows * cols):
        r, c = divmod(i, cols)
        tile = out[r * 2:(r + 1) * 2, c * 3:(c + 1) * 3]
        np.testing.assert_array_equal(tile, imgs[i] if i < 5 else 0)
    assert tile_images(imgs[:1]).shape == (2, 3, 3)
    assert tile_images(np.zeros((4, 2, 3, 3), np.uint8)).shape == (4, 6, 3)


def test_unknown_camera_mode_constructs_then_raises_at_render(monkeypatch):
    """QuadrupedGymEnv accepts any camera_mode (as the reference's constructor does); render() raises KeyError, as utils/camera.py does"""
    from qs_amd.env import quadruped_gym_env as G

    class FakeVec:
        meta = dict(robot_config=None, layout=dict(keys=[], dims=[]), settle_action=np.zeros(6), init_pose=None, landing_action=None)
        action_dim = 6
        action_space = observation_space = None

        def __init__(self, **kw):
            pass

        def render_tensor(self, **kw):
            raise AssertionError("must fail before it renders")

    monkeypatch.setattr(G, "QuadrupedVecEnv", FakeVec)
    env = G.QuadrupedGymEnv(camera_mode="NO_SUCH_MODE")
    with pytest.raises(KeyError):
        env.render()
    assert env.render(mode="human").size == 0
    assert G.QuadrupedGymEnv(camera_mode="BACKFLIP")._camera_mode == "BACKFLIP"
    assert math.isclose(CAMERA_MODES["BACKFLIP"]["fov"], 80.0)
