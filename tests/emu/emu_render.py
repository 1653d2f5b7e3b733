"""ctypes driver for the TEST-ONLY host build of the camera images (tests/emu/qs_emu_render.cpp over csrc/qs_render.h)."""
import ctypes as C
import os

import numpy as np

from .emu import _HERE, _compile

_SO_RENDER = os.path.join(_HERE, "libqs_emu_render.so")
_lib = None


def build_render():
    return _compile(_SO_RENDER, os.path.join(_HERE, "qs_emu_render.cpp"))


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_render())
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def render(states, cam, width, height, params=None, blocks=None):
    """states [m, 37], params [m, 24] or None, blocks [m, 7] or None, cam a qs_amd.lib.QsCamera.  Returns rgb uint8 [m, H, W, 3],
    depth [m, H, W], seg int32 [m, H, W]."""
    st = np.ascontiguousarray(states, np.float32).reshape(-1, 37)
    m = st.shape[0]
    par = None if params is None else np.ascontiguousarray(params, np.float32).reshape(m, 24)
    blk = None if blocks is None else np.ascontiguousarray(blocks, np.float32).reshape(m, 7)
    rgba = np.zeros((m, height, width), np.uint32)
    depth = np.zeros((m, height, width), np.float32)
    seg = np.zeros((m, height, width), np.int32)
    rc = _load().qser_render(_p(st), _p(par), _p(blk), m, C.byref(cam), width, height, _p(rgba), _p(depth), _p(seg))
    assert rc == 0
    return rgba.view(np.uint8).reshape(m, height, width, 4)[..., :3], depth, seg


def scene(state, params=None, block=None, draw_payload=True):
    """the primitive table [22, 16] (R 9, centre 3, extents 3, kind) and the bounds [22] of one state"""
    st = np.ascontiguousarray(state, np.float32)
    par = None if params is None else np.ascontiguousarray(params, np.float32)
    blk = None if block is None else np.ascontiguousarray(block, np.float32)
    out = np.zeros((22, 16), np.float32)
    b = np.zeros(22, np.float32)
    _load().qser_scene(_p(st), _p(par), _p(blk), int(draw_payload), _p(out), _p(b))
    return out, b
