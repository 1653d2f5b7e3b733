"""TEST-ONLY float64 numpy ray caster of the camera images (qs_render), written from the description in include/qs_amd.h and
INTEGRATION.md "Rendering" with kinematics of its own: the independent reference of tests/test_render_cpu.py and test_gpu_render.py.

The numbers below are go1.urdf's collision geometry and the picture's constants, written down again on purpose (a shared header would make
the reference agree with the kernel by construction)."""
import math

import numpy as np

# go1.urdf: hip joints, thigh offset, link lengths, collision primitives
HIP_X, HIP_Y, THIGH_Y, LEG_Z = 0.1881, 0.04675, 0.08, -0.213
TRUNK_HALF = (0.1881, 0.04675, 0.057)
HIP_R, HIP_HALF = 0.046, 0.02
SHOULDER_R, SHOULDER_HALF = 0.041, 0.016
THIGH_HALF, CALF_HALF, LINK_BOX_Z = (0.017, 0.01225, 0.1065), (0.008, 0.008, 0.1065), -0.1065
FOOT_R, PAYLOAD_HALF = 0.02, 0.05
# the picture
LIGHT = np.array([0.3, 0.2, 0.932737905])
AMBIENT, DIFFUSE, SHADOW_EPS = 0.35, 0.65, 1e-4
SKY = (0.62, 0.76, 0.92)
GROUND = ((0.62, 0.62, 0.62), (0.42, 0.42, 0.42))
TRUNK_RGB, PAYLOAD_RGB = (0.85, 0.55, 0.15), (0.70, 0.15, 0.15)
PART_RGB = ((0.25, 0.30, 0.38), (0.75, 0.76, 0.80), (0.35, 0.40, 0.48), (0.10, 0.10, 0.10))
BOX, CYL, SPHERE = 1, 2, 3
CAMERA_MODES = {   # utils/camera.py: distance, yaw, pitch, fov, fixed target or None (follow the base)
    "CLASSIC": (1.3, 20.0, -20.0, 60.0, None),
    "BACKFLIP": (1.3, 0.0, -6.0, 80.0, (-0.55, 0.0, 0.6)),
    "CONTINUOUS_JUMPING_FORWARD": (1.3, 10.0, -8.0, 80.0, None),
}


def quat_matrix(q):
    x, y, z, w = (float(v) for v in q)
    n = x * x + y * y + z * z + w * w
    x, y, z, w = (v / math.sqrt(n) for v in (x, y, z, w))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rx(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def ry(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def leg_frames(leg, q):
    """base-frame origins and rotations of hip, thigh and calf of leg `leg` (FR, FL, RR, RL), and the foot centre"""
    fx = 1.0 if leg < 2 else -1.0
    sy = -1.0 if leg % 2 == 0 else 1.0
    p_hip = np.array([fx * HIP_X, sy * HIP_Y, 0.0])
    R_hip = rx(q[0])
    p_thigh = p_hip + R_hip @ np.array([0.0, sy * THIGH_Y, 0.0])
    R_thigh = R_hip @ ry(q[1])
    p_calf = p_thigh + R_thigh @ np.array([0.0, 0.0, LEG_Z])
    R_calf = R_thigh @ ry(q[2])
    foot = p_calf + R_calf @ np.array([0.0, 0.0, LEG_Z])
    return (p_hip, R_hip), (p_thigh, R_thigh), (p_calf, R_calf), foot


def scene(state, params=None, block=None, draw_payload=True):
    """primitives (type, id, R world-from-local, centre, extents) of one state row [37]"""
    st = np.asarray(state, np.float64)
    pos, Rb = st[0:3], quat_matrix(st[3:7])
    local = [(BOX, 1, np.eye(3), np.zeros(3), TRUNK_HALF)]
    for leg in range(4):
        (ph, Rh), (pt, Rt), (pc, Rc), foot = leg_frames(leg, st[13 + 3 * leg: 16 + 3 * leg])
        base = 2 + 4 * leg
        local += [(CYL, base, Rh, ph, (HIP_R, HIP_HALF, 0)), (CYL, base + 1, Rt, pt, (SHOULDER_R, SHOULDER_HALF, 0)),
                  (BOX, base + 1, Rt, pt + Rt @ [0, 0, LINK_BOX_Z], THIGH_HALF), (BOX, base + 2, Rc, pc + Rc @ [0, 0, LINK_BOX_Z], CALF_HALF),
                  (SPHERE, base + 3, Rc, foot, (FOOT_R, 0, 0))]
    prims = [(t, i, Rb @ R, pos + Rb @ c, np.asarray(e, np.float64)) for t, i, R, c, e in local]
    if draw_payload and params is not None and params[20] > 0:
        if block is None:
            prims.append((BOX, 18, Rb, pos + Rb @ np.asarray(params[21:24], np.float64), np.full(3, PAYLOAD_HALF)))
        else:
            prims.append((BOX, 18, quat_matrix(block[3:7]), np.asarray(block[0:3], np.float64), np.full(3, PAYLOAD_HALF)))
    return prims


def camera(mode_or_tuple, base_pos, width, height, near=0.1, far=100.0):
    """eye, forward, right, up (unit) and the image-plane half extents at unit depth"""
    dist, yaw, pitch, fov, target = CAMERA_MODES[mode_or_tuple] if isinstance(mode_or_tuple, str) else mode_or_tuple
    tgt = np.asarray(base_pos, np.float64) if target is None else np.asarray(target, np.float64)
    R = rz(math.radians(yaw)) @ rx(math.radians(pitch))
    eye = tgt + R @ np.array([0.0, -dist, 0.0])
    up = R @ np.array([0.0, 0.0, 1.0])
    fwd = (tgt - eye) / np.linalg.norm(tgt - eye)
    right = np.cross(fwd, up)
    th = math.tan(math.radians(fov) / 2)
    return dict(eye=eye, fwd=fwd, right=right / np.linalg.norm(right), up=up, th=th, aspect=width / height, near=near, far=far, w=width, h=height)


def rays(cam, cols, rows):
    """directions through image points (col, row) (pixel centres at + 0.5), scaled to unit depth along the view axis"""
    u = 2 * (np.asarray(cols, np.float64) + 0.5) / cam["w"] - 1
    v = 1 - 2 * (np.asarray(rows, np.float64) + 0.5) / cam["h"]
    return cam["fwd"] + (u * cam["th"] * cam["aspect"])[..., None] * cam["right"] + (v * cam["th"])[..., None] * cam["up"]


def project(cam, p):
    """image coordinates (col, row) of world point p (continuous: pixel (c, r) covers [c, c + 1) x [r, r + 1))"""
    q = np.asarray(p, np.float64) - cam["eye"]
    z = q @ cam["fwd"]
    u = (q @ cam["right"]) / (z * cam["th"] * cam["aspect"])
    v = (q @ cam["up"]) / (z * cam["th"])
    return (u + 1) * cam["w"] / 2, (1 - v) * cam["h"] / 2


def _entry(prim, o, d, tmin):
    """entry parameter (inf if none at t >= tmin) and world normal of rays o + t d into one primitive"""
    typ, _, R, c, e = prim
    ol, dl = (o - c) @ R, d @ R
    n = len(d)
    t = np.full(n, np.inf)
    nl = np.zeros((n, 3))
    if typ == BOX:
        ds = np.where(np.abs(dl) > 1e-12, dl, np.where(dl < 0, -1e-12, 1e-12))
        a, b = (-e - ol) / ds, (e - ol) / ds
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        ax = np.argmax(lo, axis=1)
        t0, t1 = lo.max(axis=1), hi.min(axis=1)
        ok = (t0 <= t1) & (t0 >= tmin)
        t[ok] = t0[ok]
        nl[np.arange(n), ax] = np.where(ds[np.arange(n), ax] < 0, 1.0, -1.0)
    elif typ == CYL:
        r, h = e[0], e[1]
        A = dl[:, 0] ** 2 + dl[:, 2] ** 2
        B = ol[:, 0] * dl[:, 0] + ol[:, 2] * dl[:, 2]
        Cc = ol[:, 0] ** 2 + ol[:, 2] ** 2 - r * r
        disc = B * B - A * Cc
        with np.errstate(invalid="ignore", divide="ignore"):
            ts = (-B - np.sqrt(np.maximum(disc, 0))) / np.where(A > 1e-12, A, 1.0)
        ys = ol[:, 1] + ts * dl[:, 1]
        side = (A > 1e-12) & (disc >= 0) & (ts >= tmin) & (np.abs(ys) <= h)
        t[side] = ts[side]
        nside = np.stack([(ol[:, 0] + ts * dl[:, 0]) / r, np.zeros(n), (ol[:, 2] + ts * dl[:, 2]) / r], 1)
        nl[side] = nside[side]
        dy = np.where(np.abs(dl[:, 1]) > 1e-12, dl[:, 1], np.where(dl[:, 1] < 0, -1e-12, 1e-12))
        cy = np.where(dy > 0, -h, h)
        tc = (cy - ol[:, 1]) / dy
        xc, zc = ol[:, 0] + tc * dl[:, 0], ol[:, 2] + tc * dl[:, 2]
        cap = (tc >= tmin) & (xc * xc + zc * zc <= r * r) & (tc < t)
        t[cap] = tc[cap]
        nl[cap] = np.stack([np.zeros(n), np.where(dy > 0, -1.0, 1.0), np.zeros(n)], 1)[cap]
    else:
        r = e[0]
        A = (dl * dl).sum(1)
        B = (ol * dl).sum(1)
        Cc = (ol * ol).sum(1) - r * r
        disc = B * B - A * Cc
        ts = (-B - np.sqrt(np.maximum(disc, 0))) / A
        ok = (disc >= 0) & (ts >= tmin)
        t[ok] = ts[ok]
        nl[ok] = ((ol + ts[:, None] * dl) / r)[ok]
    return t, nl @ R.T


def render(state, cam_spec="CLASSIC", width=160, height=120, params=None, block=None, draw_payload=True, near=0.1, far=100.0):
    """rgb uint8 [H, W, 3], depth [H, W], seg int32 [H, W], shadowed bool [H, W], checker parity int [H, W] (-1 off the floor)"""
    prims = scene(state, params, block, draw_payload)
    cam = camera(cam_spec, np.asarray(state, np.float64)[0:3], width, height, near, far)
    rows, cols = np.mgrid[0:height, 0:width]
    d = rays(cam, cols.ravel(), rows.ravel())
    n = len(d)
    o = np.broadcast_to(cam["eye"], (n, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = np.where(np.abs(d[:, 2]) > 1e-12, -cam["eye"][2] / d[:, 2], np.inf)
    tg = np.where(tg >= near, tg, np.inf)
    best, seg, nrm = tg.copy(), np.where(np.isfinite(tg), 0, -1), np.tile([0.0, 0.0, 1.0], (n, 1))
    for p in prims:
        t, nw = _entry(p, o, d, near)
        closer = t < best
        best[closer], seg[closer], nrm[closer] = t[closer], p[1], nw[closer]
    sky = ~np.isfinite(best) | (best > far)
    seg[sky] = -1
    depth = np.where(sky, far, best)
    hitp = o + depth[:, None] * d
    lam = np.maximum(nrm @ LIGHT, 0.0)
    want = ~sky & (lam > 0)
    shadow = np.zeros(n, bool)
    so = hitp + SHADOW_EPS * nrm
    L = np.broadcast_to(LIGHT, (n, 3))
    for p in prims:
        t, _ = _entry(p, so, L, 0.0)
        shadow |= want & np.isfinite(t)
    col = np.zeros((n, 3))
    parity = np.full(n, -1)
    fl = seg == 0
    parity[fl] = (np.floor(hitp[fl, 0]).astype(np.int64) + np.floor(hitp[fl, 1]).astype(np.int64)) & 1
    col[fl] = np.asarray(GROUND)[parity[fl]]
    col[seg == 1] = TRUNK_RGB
    col[seg == 18] = PAYLOAD_RGB
    legs = (seg >= 2) & (seg < 18)
    col[legs] = np.asarray(PART_RGB)[(seg[legs] - 2) % 4]
    lit = AMBIENT + np.where(shadow, 0.0, DIFFUSE * lam)
    c = col * lit[:, None]
    c[sky] = SKY
    rgb = np.floor(np.clip(c, 0, 1) * 255 + 0.5).astype(np.uint8)
    return (rgb.reshape(height, width, 3), depth.reshape(height, width), seg.reshape(height, width).astype(np.int32),
            shadow.reshape(height, width), parity.reshape(height, width))


def edge_mask(a):
    """pixels whose 3 x 3 neighbourhood holds more than one value of `a`"""
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    m = np.zeros(a.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m |= p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != a
    return m


def compare(ref, rgb, depth, seg, max_boundary=0.005):
    """the pass criteria: segmentation equal except at the reference's segment boundaries (those <= max_boundary of the pixels); where it
    agrees, depth within 1e-4 relative and RGB within 1, except next to a shadow or checker edge.  Returns a message or None."""
    rrgb, rdepth, rseg, rshadow, rpar = ref
    bad = rseg != seg
    boundary = edge_mask(rseg)
    if np.any(bad & ~boundary):
        return f"segmentation differs off the boundaries at {np.argwhere(bad & ~boundary)[:5].tolist()}"
    if bad.mean() > max_boundary:
        return f"segmentation differs on {bad.mean():.4%} of the pixels"
    ok = ~bad
    rel = np.abs(depth - rdepth) / np.maximum(np.abs(rdepth), 1e-9)
    if np.any(ok & (rel > 1e-4)):
        return f"depth off by {rel[ok].max():.2e} relative at {np.argwhere(ok & (rel > 1e-4))[:5].tolist()}"
    soft = edge_mask(rshadow.astype(np.int8)) | edge_mask(rpar)
    diff = np.abs(rgb.astype(np.int32) - rrgb.astype(np.int32)).max(-1)
    if np.any(ok & ~soft & (diff > 1)):
        return f"rgb off by {diff[ok & ~soft].max()} at {np.argwhere(ok & ~soft & (diff > 1))[:5].tolist()}"
    return None
