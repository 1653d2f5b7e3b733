"""Camera images of the robot (the reference's utils/camera.py:14-117 behind QuadrupedGymEnv.render(mode="rgb_array")), ray cast on the device
by k_render (csrc/qs_render.hip).  What a frame shows, the camera convention and the segmentation ids: include/qs_amd.h (qs_render)."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import lib as _lib
from .handle import ptr as _ptr

# utils/camera.py:14-20, 86-117: distance, yaw, pitch (degrees), vertical fov (degrees); target None = the base position (the camera follows
# the robot), else a fixed world point
CAMERA_MODES = {
    "CLASSIC": dict(distance=1.3, yaw=20.0, pitch=-20.0, fov=60.0, target=None),
    "BACKFLIP": dict(distance=1.3, yaw=0.0, pitch=-6.0, fov=80.0, target=(-0.55, 0.0, 0.6)),
    "CONTINUOUS_JUMPING_FORWARD": dict(distance=1.3, yaw=10.0, pitch=-8.0, fov=80.0, target=None),
}
DEFAULT_SIZE = (1440, 1080)   # (width, height), camera.py:26-27
MAX_RGBA_BYTES = 1 << 30      # one request's RGBA buffer
SEG_BAD_ENV, SEG_SKY, SEG_GROUND, SEG_TRUNK, SEG_PAYLOAD = -2, -1, 0, 1, 18


def seg_leg(leg, part):
    """segmentation id of leg `leg` (q order) and part 0 hip, 1 thigh (box and shoulder cylinder), 2 calf, 3 foot"""
    return 2 + 4 * leg + part


@dataclass
class Camera:
    """A camera as Bullet's computeViewMatrixFromYawPitchRoll / computeProjectionMatrixFOV take it (utils/camera.py:38-49).
    follow_base: the target is the base position + `target`."""
    target: tuple = (0.0, 0.0, 0.0)
    distance: float = 1.3
    yaw: float = 20.0
    pitch: float = -20.0
    fov: float = 60.0
    near: float = 0.1
    far: float = 100.0
    follow_base: bool = True
    draw_payload: bool = True

    @classmethod
    def from_mode(cls, mode):
        """one of CAMERA_MODES; KeyError for any other name"""
        m = CAMERA_MODES[mode]
        t = m["target"]
        return cls(target=(0.0, 0.0, 0.0) if t is None else tuple(float(x) for x in t), distance=m["distance"], yaw=m["yaw"], pitch=m["pitch"],
                   fov=m["fov"], follow_base=t is None)

    def to_c(self):
        c = _lib.QsCamera()
        for i in range(3):
            c.target[i] = float(self.target[i])
        c.distance, c.yaw_deg, c.pitch_deg, c.fov_deg = float(self.distance), float(self.yaw), float(self.pitch), float(self.fov)
        c.near_clip, c.far_clip = float(self.near), float(self.far)
        c.follow_base, c.draw_payload = int(bool(self.follow_base)), int(bool(self.draw_payload))
        return c


def as_camera(camera):
    """a mode name, a Camera"""
    if isinstance(camera, Camera):
        return camera
    if isinstance(camera, str):
        return Camera.from_mode(camera)
    raise TypeError(f"camera must be a mode name {sorted(CAMERA_MODES)} or a Camera, got {camera!r}")


def check_request(m, width, height, what="the request"):
    """image size and the 1 GiB bound of one request's RGBA buffer; ValueError naming `what`"""
    if not (isinstance(width, (int, np.integer)) and isinstance(height, (int, np.integer))) or not (1 <= width <= 8192 and 1 <= height <= 8192):
        raise ValueError(f"image size {width} x {height}: width and height must be integers in [1, 8192]")
    if m * width * height * 4 > MAX_RGBA_BYTES:
        raise ValueError(f"{m} images of {width} x {height} need {m * width * height * 4 / 1e9:.1f} GB of RGBA, more than the "
                         f"{MAX_RGBA_BYTES >> 30} GiB one render may take: reduce {what}")


def alloc(torch, m, width, height, device, depth, segmentation):
    """the output buffers: RGBA packed as int32 [m, H, W] (viewed as uint8 [m, H, W, 4]), float32 depth and int32 segmentation or None"""
    rgba = torch.empty((m, height, width), dtype=torch.int32, device=device)
    d = torch.empty((m, height, width), dtype=torch.float32, device=device) if depth else None
    s = torch.empty((m, height, width), dtype=torch.int32, device=device) if segmentation else None
    return rgba, d, s


def rgb_view(rgba):
    """uint8 [m, H, W, 3] view of the packed RGBA buffer (R in the low byte)"""
    import torch
    return rgba.view(torch.uint8).view(*rgba.shape, 4)[..., :3]


def render_states(states, params=None, camera="CLASSIC", width=DEFAULT_SIZE[0], height=DEFAULT_SIZE[1], depth=False, segmentation=False,
                  stream=None):
    """Images of any state rows (qs_render_states): states [m, 37] float32 on the device (qs_get_state layout: a recorded rollout, trace
    rows[:, 1:38], ...), params [m, 24] (QS_INFO_PARAMS layout; the payload block is drawn at r_payload) or None.  Returns (rgb uint8
    [m, H, W, 3], a view of the RGBA buffer; depth float32 [m, H, W] or None; segmentation int32 [m, H, W] or None), device tensors, on
    `stream` (default: torch's current stream of the states' device); nothing waits for the device."""
    import torch
    if not isinstance(states, torch.Tensor) or states.device.type != "cuda":
        raise TypeError("states must be a tensor on the device")
    if states.dim() != 2 or states.shape[1] != 37 or states.dtype != torch.float32:
        raise ValueError(f"states must be float32 [m, 37], got {states.dtype} {tuple(states.shape)}")
    m = states.shape[0]
    if params is not None:
        if not isinstance(params, torch.Tensor) or params.device != states.device or params.dtype != torch.float32 or tuple(params.shape) != (m, 24):
            raise ValueError(f"params must be float32 [{m}, 24] on the states' device")
        params = params.contiguous()
    cam = as_camera(camera)
    check_request(m, width, height, "the number of states or the image size")
    states = states.contiguous()
    rgba, d, s = alloc(torch, m, int(width), int(height), states.device, depth, segmentation)
    if stream is None:
        stream = torch.cuda.current_stream(states.device)
    cs = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    c = cam.to_c()
    _lib.check(_lib.load().qs_render_states(_ptr(states), _ptr(params), m, C.byref(c), int(width), int(height), _ptr(rgba), _ptr(d), _ptr(s),
                                            C.c_void_p(cs)))
    return rgb_view(rgba), d, s


def tile_images(imgs):
    """SB3's tile_images (common/vec_env/base_vec_env.py): n images [H, W, C] on a grid of ceil(sqrt(n)) rows and ceil(n / rows) columns,
    row-major, padded with black images."""
    imgs = np.asarray(imgs)
    n, h, w, c = imgs.shape
    rows = int(math.ceil(math.sqrt(n)))
    cols = int(math.ceil(n / rows))
    grid = np.zeros((rows * cols, h, w, c), imgs.dtype)
    grid[:n] = imgs
    return grid.reshape(rows, cols, h, w, c).transpose(0, 2, 1, 3, 4).reshape(rows * h, cols * w, c)
