"""Camera images on the device (k_render through qs_render / qs_render_states, QuadrupedVecEnv.render_tensor / get_images / render,
QuadrupedGymEnv.render): against the float64 numpy reference and the host build of csrc/qs_render.h, the handle path against the state-row
path, independence of the batch, no effect on the simulation, the drop-in surface, sub-step frames and the absence of host synchronisation."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402
from emu import emu_render  # noqa: E402
from test_gpu_round2 import vec_env  # noqa: E402

pytestmark = pytest.mark.gpu


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


def thrown_and_fallen(n, seed=0):
    """settled standing states, thrown robots (random attitude and height, random joints) and robots lying on the floor"""
    from oracle.qso import Oracle
    from qs_amd.config import build_config
    cfg, _ = build_config(n_envs=1, env_randomizer_mode="NONE", noise=False)
    o = Oracle(cfg)
    o.reset()
    stand = o.get_state()[0]
    rng = np.random.default_rng(seed)
    out = np.tile(stand, (n, 1))
    for i in range(n):
        kind = i % 4
        out[i, 0:2] = rng.uniform(-3, 3, 2)
        if kind == 1:      # thrown
            out[i, 2] = rng.uniform(0.3, 1.5)
            out[i, 3:7] = Rotation.random(random_state=seed + i).as_quat()
            out[i, 13:25] = rng.uniform(-2, 2, 12)
        elif kind == 2:    # fallen on its side or back
            out[i, 2] = 0.09 if i % 8 == 2 else 0.13
            out[i, 3:7] = Rotation.from_euler("xz", [90 if i % 8 == 2 else 180, rng.uniform(-180, 180)], degrees=True).as_quat()
        elif kind == 3:    # random joint angles, mid-air
            out[i, 2] = rng.uniform(0.4, 0.8)
            out[i, 3:7] = Rotation.from_euler("z", rng.uniform(-180, 180), degrees=True).as_quat()
            out[i, 13:25] = rng.uniform(-1.5, 1.5, 12)
    return out.astype(np.float32)


def payload_params(n, seed=1):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 24), np.float32)
    p[::2, 20] = 1.0
    p[:, 21:24] = rng.uniform(-0.08, 0.08, (n, 3))
    return p


def test_render_states_matches_reference_and_emulation(torch_cuda):
    from qs_amd.render import Camera, render_states
    t = torch_cuda
    n, W, H = 64, 320, 240
    st, par = thrown_and_fallen(n), payload_params(n)
    for mode in ("CLASSIC", "BACKFLIP", "CONTINUOUS_JUMPING_FORWARD"):
        rgb, depth, seg = render_states(t.from_numpy(st).cuda(), t.from_numpy(par).cuda(), camera=mode, width=W, height=H, depth=True,
                                        segmentation=True)
        rgb, depth, seg = rgb.cpu().numpy(), depth.cpu().numpy(), seg.cpu().numpy()
        assert rgb.shape == (n, H, W, 3) and rgb.dtype == np.uint8
        ergb, edepth, eseg = emu_render.render(st, Camera.from_mode(mode).to_c(), W, H, par)
        for i in range(n):
            if i % 8 == 0:   # (the float64 reference takes half a second per image: every eighth state of each mode)
                ref = R.render(st[i], mode, W, H, params=par[i])
                msg = R.compare(ref, rgb[i], depth[i], seg[i])
                assert msg is None, f"{mode} state {i} against the reference: {msg}"
            # against the host build (the same arithmetic up to the device code's FMA contraction); shadow and checker edges: where the
            # host build's brightness jumps
            lum = ergb[i].astype(np.int32).sum(-1)
            jump = np.zeros((H, W), np.int32)
            jump[:, 1:] |= np.abs(np.diff(lum, axis=1)) > 30
            jump[1:, :] |= np.abs(np.diff(lum, axis=0)) > 30
            msg = R.compare((ergb[i], edepth[i], eseg[i], jump.astype(bool), np.zeros((H, W), int)), rgb[i], depth[i], seg[i])
            assert msg is None, f"{mode} state {i} against the emulation: {msg}"


def test_handle_render_equals_state_rows(torch_cuda):
    t = torch_cuda
    v = vec_env(48, env_randomizer_mode="MASS_RANDOMIZER")
    v.reset_tensor()
    act = t.zeros((48, v.action_dim), device=v.device)
    for _ in range(5):
        v.step_tensor(act)
    from qs_amd.render import render_states
    for mode in ("CLASSIC", "BACKFLIP"):
        a = v.render_tensor(camera=mode, width=200, height=150, depth=True, segmentation=True)
        b = render_states(v.get_state(), v.get_info("params"), camera=mode, width=200, height=150, depth=True, segmentation=True)
        for x, y, what in zip(a, b, ("rgb", "depth", "seg")):
            same(x, y, f"{mode} {what}")
    assert (v.get_info("params")[:, 20] > 0).any(), "the mass randomizer put a payload on some robots"
    assert (b[2] == 18).any()


def test_one_environment_alone_equals_it_in_a_batch(torch_cuda):
    t = torch_cuda
    n = 257
    v = vec_env(n)
    v.reset_tensor()
    st = t.from_numpy(thrown_and_fallen(n, seed=5)).to(v.device)
    v.set_state(st)
    batch = v.render_tensor(width=96, height=64, depth=True, segmentation=True)
    for k in (0, 100, 256):
        alone = v.render_tensor(indices=[k], width=96, height=64, depth=True, segmentation=True)
        for x, y, what in zip(alone, batch, ("rgb", "depth", "seg")):
            same(x[0], y[k], f"env {k} {what}")
    again = v.render_tensor(width=96, height=64, depth=True, segmentation=True)
    for x, y, what in zip(again, batch, ("rgb", "depth", "seg")):
        same(x, y, f"second render {what}")


def test_rendering_does_not_touch_the_simulation(torch_cuda):
    t = torch_cuda
    n = 64
    a, b = vec_env(n, seed=3), vec_env(n, seed=3)
    a.reset_tensor(), b.reset_tensor()
    rng = np.random.default_rng(2)
    for _ in range(50):
        act = t.from_numpy(rng.uniform(-1, 1, (n, a.action_dim)).astype(np.float32)).to(a.device)
        oa, ra, da, _ = a.step_tensor(act)
        ob, rb, db, _ = b.step_tensor(act)
        b.render_tensor(width=64, height=48, depth=True, segmentation=True)
        same(oa, ob, "obs"), same(ra, rb, "rew"), same(da, db, "done")
    same(a.get_state(), b.get_state(), "state")
    b.stats()   # nothing refused


def test_out_of_range_device_id_draws_sky_and_is_reported(torch_cuda):
    t = torch_cuda
    v = vec_env(16)
    v.reset_tensor()
    ids = t.tensor([3, 16, 5], dtype=t.int32, device=v.device)
    rgb, _, seg = v.render_tensor(indices=ids, width=32, height=32, segmentation=True)
    assert (seg[1] == -2).all() and not (seg[0] == -2).any()
    with pytest.raises(RuntimeError, match="position 1 of env_ids"):
        v.stats()
    v.stats()     # reported once
    with pytest.raises(ValueError, match="environment ids"):
        v.render_tensor(indices=[0, 16])


def gym_env(**kw):
    from qs_amd.env.quadruped_gym_env import QuadrupedGymEnv
    return QuadrupedGymEnv(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, seed=4, noise=False, **kw)


def test_gym_env_render_follows_the_robot(torch_cuda):
    env = gym_env()
    env.reset()
    f0 = env.render()
    assert f0.shape == (1080, 1440, 3) and f0.dtype == np.uint8
    a = np.ones(env.action_dim)
    for _ in range(15):
        env.step(a)
    f1 = env.render()
    assert np.abs(f1.astype(int) - f0.astype(int)).sum() > 0
    assert env.render(mode="human").size == 0
    env.close()


def test_backflip_camera_keeps_the_floor_still(torch_cuda):
    from qs_amd.render import render_states
    env = gym_env(camera_mode="BACKFLIP")
    env.reset()
    f0 = env.render()
    s0 = env._vec.get_state()
    for _ in range(15):
        env.step(np.ones(env.action_dim))
    f1 = env.render()
    s1 = env._vec.get_state()
    seg0 = render_states(s0, camera="BACKFLIP", segmentation=True)[2][0].cpu().numpy()
    seg1 = render_states(s1, camera="BACKFLIP", segmentation=True)[2][0].cpu().numpy()
    away = s0.clone()
    away[:, 2] = -50.0                   # the floor alone (robot far below it)
    bare = render_states(away, camera="BACKFLIP")[0][0].cpu().numpy()
    floor = (seg0 == 0) & (seg1 == 0)
    differ = floor & np.any(f0 != f1, -1)
    # a floor pixel that changed lies in a shadow in one of the two frames (darker than the bare floor there)
    shadowed = np.any(f0 != bare, -1) | np.any(f1 != bare, -1)
    assert not np.any(differ & ~shadowed)
    assert differ.sum() < 0.1 * floor.sum() and floor.sum() > 100000
    env.close()


def test_get_images_render_and_the_guard(torch_cuda):
    v = vec_env(5)
    v.reset_tensor()
    v.set_attr("render_size", (64, 48))
    imgs = v.get_images()
    assert len(imgs) == 5 and all(i.shape == (48, 64, 3) and i.dtype == np.uint8 and i.flags.c_contiguous for i in imgs)
    assert v.render().shape == (3 * 48, 2 * 64, 3)
    v.set_attr("render_indices", [1, 3])
    assert len(v.get_images()) == 2 and v.render().shape == (2 * 48, 1 * 64, 3)
    np.testing.assert_array_equal(v.get_images()[1], imgs[3])
    v.set_attr("camera_mode", "BACKFLIP")
    assert not np.array_equal(v.get_images()[0], imgs[1])
    with pytest.raises(NotImplementedError):
        v.render(mode="human")
    big = vec_env(8192)
    with pytest.raises(ValueError, match="render_indices or render_size"):
        big.render_tensor()
    # the wrappers forward
    from qs_amd.vec_normalize import DeviceVecNormalize
    w = DeviceVecNormalize(v)
    assert len(w.get_images()) == 2 and w.render().shape == (2 * 48, 64, 3)


def test_sub_step_frames_equal_the_trace_rows(torch_cuda):
    from qs_amd.render import render_states
    t = torch_cuda
    env = gym_env()
    env.reset()
    env._vec.render_size = (160, 120)
    frames = []
    env.set_sub_step_callback(lambda: frames.append(env.render()))
    env.step(np.ones(env.action_dim))
    rows = env._vec.get_trace(as_dict=False)
    assert len(frames) == rows.shape[0] == 10
    st = t.from_numpy(rows[:, 1:38].astype(np.float32)).to(env._vec.device)
    par = env._vec.get_info("params").expand(10, 24).contiguous()
    ref = render_states(st, par, camera="CLASSIC", width=160, height=120)[0].cpu().numpy()
    for k in range(10):
        np.testing.assert_array_equal(frames[k], ref[k])
    assert not np.array_equal(frames[0], frames[-1])
    env.close()


def test_render_tensor_never_waits_for_the_device(torch_cuda):
    t = torch_cuda
    n = 64
    v = vec_env(n)
    v.reset_tensor()
    act = t.zeros((n, v.action_dim), device=v.device)
    ids = t.arange(0, n, 2, dtype=t.int32, device=v.device)
    t.cuda.synchronize()
    t.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(4):
            v.step_tensor(act)
            v.render_tensor(width=64, height=48, depth=True, segmentation=True)
            v.render_tensor(indices=[1, 5, 9], camera="BACKFLIP", width=32, height=32)
            v.render_tensor(indices=ids, width=32, height=32)
    finally:
        t.cuda.set_sync_debug_mode("default")
    v.stats()
