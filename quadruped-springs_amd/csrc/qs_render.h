// qs_render.h -- ray-cast camera images of the robot's collision primitives and the ground (qs_render, qs_render_states).
//
// Plain scalar C++ (no lane intrinsics): k_render (qs_render.hip) runs it with one pixel per thread, and the host emulation of the tests
// (tests/emu/qs_emu_render.cpp) builds it unchanged with g++.
//
// Scene of one environment: the collision primitives of go1.urdf posed by a state row (qs_get_state layout: position, quaternion xyzw, ...,
// joint angles in q order), the payload block, the plane z = 0 (checkerboard of 1 m squares) and a constant sky.  One directional light,
// Lambert shading plus ambient, hard shadows cast by the robot.  Camera: Bullet's computeViewMatrixFromYawPitchRoll(target, distance, yaw,
// pitch, roll = 0, upAxisIndex = 2) and computeProjectionMatrixFOV(fov, W / H, near, far), as the reference's utils/camera.py:38-49 calls
// them, read as: R = Rz(yaw) Rx(pitch), eye = target + R (0, -distance, 0), up = R (0, 0, 1), looking from the eye at the target, fov
// vertical.  A ray's parameter t is its depth along the view axis, so the near / far planes are plain bounds on t.
#pragma once
#include "qs_core.h"

namespace qs {
namespace rnd {

// ------------------------------------------------------------------ every constant of the picture
constexpr int MAX_PRIM = 22;            // trunk, 4 x (hip, shoulder, thigh, calf, foot), payload block
constexpr int TILE = 16;                // k_render: a workgroup renders a TILE x TILE block of one image
enum { PRIM_NONE = 0, PRIM_BOX = 1, PRIM_CYL = 2 /* axis: local y */, PRIM_SPHERE = 3 };
// segmentation ids: sky, ground, trunk, 2 + 4 leg + part (0 hip, 1 thigh box and shoulder, 2 calf, 3 foot), payload; an environment id out
// of range (qs_render) draws sky with id SEG_BAD_ENV
enum { SEG_BAD_ENV = -2, SEG_SKY = -1, SEG_GROUND = 0, SEG_TRUNK = 1, SEG_LEG = 2, SEG_PAYLOAD = 18 };
constexpr float LIGHT[3] = {0.3f, 0.2f, 0.932737905f};   // unit vector towards the light
constexpr float AMBIENT = 0.35f, DIFFUSE = 0.65f;        // colour x (AMBIENT + DIFFUSE max(0, n . LIGHT)); shadowed: colour x AMBIENT
constexpr float SHADOW_EPS = 1e-4f;                     // a shadow ray starts at p + SHADOW_EPS n
constexpr float SKY[3] = {0.62f, 0.76f, 0.92f};
constexpr float GROUND[2][3] = {{0.62f, 0.62f, 0.62f}, {0.42f, 0.42f, 0.42f}};  // checker squares with floor(x) + floor(y) even / odd
constexpr float CHECKER = 1.0f;                         // m
constexpr float TRUNK_RGB[3] = {0.85f, 0.55f, 0.15f};
constexpr float PART_RGB[4][3] = {{0.25f, 0.30f, 0.38f}, {0.75f, 0.76f, 0.80f}, {0.35f, 0.40f, 0.48f}, {0.10f, 0.10f, 0.10f}};  // hip, thigh, calf, foot
constexpr float PAYLOAD_RGB[3] = {0.70f, 0.15f, 0.15f};
constexpr float BOUND_PAD = 1e-3f;                      // m added to the robot's bounding sphere (the skip must never drop a hit)
constexpr float DIR_TINY = 1e-12f;                      // direction components closer to 0 count as this (no infinities: -ffinite-math-only)

struct F3 { float x, y, z; };
QS_FN F3 f3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
QS_FN F3 add(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
QS_FN F3 sub(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
QS_FN F3 scl(F3 a, float s) { return f3(a.x * s, a.y * s, a.z * s); }
QS_FN float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
QS_FN F3 cross3(F3 a, F3 b) { return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// A primitive: world-from-local rotation R (row-major; column j = local axis j in world coordinates), centre c, extents e (box: half extents;
// cylinder: radius, half length, -; sphere: radius, -, -), kind = type | segmentation id << 4.  64 bytes.
struct Prim { float R[9]; float c[3]; float e[3]; int kind; };

QS_FN void mat_mul(const float* A, const float* B, float* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
QS_FN F3 mat_vec(const float* A, F3 v) {
    return f3(A[0] * v.x + A[1] * v.y + A[2] * v.z, A[3] * v.x + A[4] * v.y + A[5] * v.z, A[6] * v.x + A[7] * v.y + A[8] * v.z);
}
QS_FN void quat_mat(float x, float y, float z, float w, float* R) {   // xyzw, need not be of unit length
    const float s = 2.0f / (x * x + y * y + z * z + w * w);
    const float xs = x * s, ys = y * s, zs = z * s;
    const float wx = w * xs, wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
    R[0] = 1.0f - (yy + zz); R[1] = xy - wz; R[2] = xz + wy;
    R[3] = xy + wz; R[4] = 1.0f - (xx + zz); R[5] = yz - wx;
    R[6] = xz - wy; R[7] = yz + wx; R[8] = 1.0f - (xx + yy);
}
QS_FN void rot_x(float a, float* R) { float s, c; qsincos(a, s, c); R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = c; R[5] = -s; R[6] = 0; R[7] = s; R[8] = c; }
QS_FN void rot_xy(float a, float b, float* R) {   // Rx(a) Ry(b): hip about x, then thigh / calf about y
    float sa, ca, sb, cb; qsincos(a, sa, ca); qsincos(b, sb, cb);
    R[0] = cb; R[1] = 0; R[2] = sb;
    R[3] = sa * sb; R[4] = ca; R[5] = -sa * cb;
    R[6] = -ca * sb; R[7] = sa; R[8] = ca * cb;
}

// What a scene is built from: a state row [37] (qs_get_state layout), the parameter row [24] or null (no payload), the payload block's
// pose (position 3, quaternion 4; cfg.payload_soft) or null (the block sits at r_pay in the base frame).
struct SceneSrc { const float* st; const float* par; const float* blk; int draw_payload; };

// Primitive k (0 .. MAX_PRIM - 1) of the scene, with the radius of a sphere about the base position that holds it (0 for PRIM_NONE).
//   k = 0 trunk; k = 1 + 5 leg + part, part 0 hip housing, 1 thigh-shoulder cylinder, 2 thigh box, 3 calf box, 4 foot; k = 21 payload.
// Legs in q order (FR, FL, RR, RL), frames as the step kernels build them (qs_core.h Sim::substep: hip joint at (fx HIP_X, sy HIP_Y, 0)
// about x, thigh frame THIGH_Y further along the hip's y, calf frame LEG_Z down the thigh's z, foot LEG_Z down the calf's z).
QS_FN void build_prim(const SceneSrc& src, int k, Prim& P, float& bound) {
    using namespace go1;
    const float* st = src.st;
    float Rb[9]; quat_mat(st[3], st[4], st[5], st[6], Rb);
    const F3 pos = f3(st[0], st[1], st[2]);
    float Rl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    F3 cl = f3(0, 0, 0);
    int type = PRIM_NONE, id = SEG_SKY;
    P.e[0] = P.e[1] = P.e[2] = 0.0f;
    if (k == 0) {
        type = PRIM_BOX; id = SEG_TRUNK;
        P.e[0] = TRUNK_HALF[0]; P.e[1] = TRUNK_HALF[1]; P.e[2] = TRUNK_HALF[2];
    } else if (k < 21) {
        const int leg = (k - 1) / 5, part = (k - 1) % 5;
        const float fx = leg < 2 ? 1.0f : -1.0f, sy = (leg & 1) ? 1.0f : -1.0f;
        const float q0 = st[13 + 3 * leg], q1 = st[14 + 3 * leg], q2 = st[15 + 3 * leg];
        const F3 p1 = f3(fx * HIP_X, sy * HIP_Y, 0.0f);
        if (part == 0) {
            rot_x(q0, Rl); cl = p1;
            type = PRIM_CYL; id = SEG_LEG + 4 * leg; P.e[0] = HIP_CYL_R; P.e[1] = HIP_CYL_HALF_LEN;
        } else {
            float R1[9]; rot_x(q0, R1);
            const F3 p2 = add(p1, scl(f3(R1[1], R1[4], R1[7]), sy * THIGH_Y));
            rot_xy(q0, q1, Rl);
            if (part == 1) {
                cl = p2; type = PRIM_CYL; id = SEG_LEG + 4 * leg + 1; P.e[0] = SHOULDER_CYL_R; P.e[1] = SHOULDER_CYL_HALF_LEN;
            } else if (part == 2) {
                cl = add(p2, scl(f3(Rl[2], Rl[5], Rl[8]), LINK_BOX_Z));
                type = PRIM_BOX; id = SEG_LEG + 4 * leg + 1; P.e[0] = THIGH_HALF[0]; P.e[1] = THIGH_HALF[1]; P.e[2] = THIGH_HALF[2];
            } else {
                const F3 p3 = add(p2, scl(f3(Rl[2], Rl[5], Rl[8]), LEG_Z));
                rot_xy(q0, q1 + q2, Rl);
                const F3 z3 = f3(Rl[2], Rl[5], Rl[8]);
                if (part == 3) {
                    cl = add(p3, scl(z3, LINK_BOX_Z));
                    type = PRIM_BOX; id = SEG_LEG + 4 * leg + 2; P.e[0] = CALF_HALF[0]; P.e[1] = CALF_HALF[1]; P.e[2] = CALF_HALF[2];
                } else {
                    cl = add(p3, scl(z3, LEG_Z));
                    type = PRIM_SPHERE; id = SEG_LEG + 4 * leg + 3; P.e[0] = FOOT_R;
                }
            }
        }
    } else if (src.draw_payload && src.par && src.par[P_M_PAY] > 0.0f) {
        type = PRIM_BOX; id = SEG_PAYLOAD;
        P.e[0] = P.e[1] = P.e[2] = PAYLOAD_HALF;
        if (src.blk == nullptr) cl = f3(src.par[P_R_PAY], src.par[P_R_PAY + 1], src.par[P_R_PAY + 2]);
    }
    if (k == 21 && type != PRIM_NONE && src.blk != nullptr) {   // the block's own pose (world)
        quat_mat(src.blk[3], src.blk[4], src.blk[5], src.blk[6], P.R);
        P.c[0] = src.blk[0]; P.c[1] = src.blk[1]; P.c[2] = src.blk[2];
    } else {
        mat_mul(Rb, Rl, P.R);
        const F3 c = add(pos, mat_vec(Rb, cl));
        P.c[0] = c.x; P.c[1] = c.y; P.c[2] = c.z;
    }
    P.kind = type | (id << 4);
    float ext = 0.0f;
    if (type == PRIM_BOX) ext = qsqrt(P.e[0] * P.e[0] + P.e[1] * P.e[1] + P.e[2] * P.e[2]);
    else if (type == PRIM_CYL) ext = qsqrt(P.e[0] * P.e[0] + P.e[1] * P.e[1]);
    else if (type == PRIM_SPHERE) ext = P.e[0];
    const F3 off = sub(f3(P.c[0], P.c[1], P.c[2]), pos);
    bound = type == PRIM_NONE ? 0.0f : qsqrt(dot3(off, off)) + ext;
}
QS_FN int prim_type(const Prim& P) { return P.kind & 15; }
QS_FN int prim_id(const Prim& P) { return P.kind >> 4; }

// ------------------------------------------------------------------ camera
// What every pixel of every image shares, worked out once on the host: the image's basis scaled so that the ray of the pixel with
// normalised coordinates (u, v) in [-1, 1]^2 is d = fwd + u rx + v uy (t = depth along the view axis), and the eye relative to the target.
struct CamSetup {
    float target[3];     // world; with follow: added to the base position
    float eye_off[3];    // R (0, -distance, 0)
    float fwd[3], rx[3], uy[3];
    float near_clip, far_clip;
    float inv_w, inv_h;  // 2 / W, 2 / H
    int32_t follow, draw_payload, width, height;
};
QS_FN CamSetup camera_setup(const qs_camera& cam, int width, int height) {
    const float deg = 3.14159265358979f / 180.0f;
    float sy_, cy, sp, cp; qsincos(cam.yaw_deg * deg, sy_, cy); qsincos(cam.pitch_deg * deg, sp, cp);
    // R = Rz(yaw) Rx(pitch); columns: R e_x (right), R e_y (forward), R e_z (up)
    const F3 ex = f3(cy, sy_, 0.0f), ey = f3(-sy_ * cp, cy * cp, sp), ez = f3(sy_ * sp, -cy * sp, cp);
    const float th = tanf(0.5f * cam.fov_deg * deg), aspect = (float)width / (float)height;
    CamSetup c;
    for (int i = 0; i < 3; i++) c.target[i] = cam.target[i];
    c.eye_off[0] = -cam.distance * ey.x; c.eye_off[1] = -cam.distance * ey.y; c.eye_off[2] = -cam.distance * ey.z;
    c.fwd[0] = ey.x; c.fwd[1] = ey.y; c.fwd[2] = ey.z;
    c.rx[0] = ex.x * th * aspect; c.rx[1] = ex.y * th * aspect; c.rx[2] = ex.z * th * aspect;
    c.uy[0] = ez.x * th; c.uy[1] = ez.y * th; c.uy[2] = ez.z * th;
    c.near_clip = cam.near_clip; c.far_clip = cam.far_clip;
    c.inv_w = 2.0f / (float)width; c.inv_h = 2.0f / (float)height;
    c.follow = cam.follow_base; c.draw_payload = cam.draw_payload; c.width = width; c.height = height;
    return c;
}
QS_FN F3 eye_of(const CamSetup& c, const float* base_pos) {
    F3 t = f3(c.target[0], c.target[1], c.target[2]);
    if (c.follow) t = add(t, f3(base_pos[0], base_pos[1], base_pos[2]));
    return add(t, f3(c.eye_off[0], c.eye_off[1], c.eye_off[2]));
}
// ray of pixel (col, row) through its centre, row 0 at the top
QS_FN F3 pixel_dir(const CamSetup& c, int col, int row) {
    const float u = ((float)col + 0.5f) * c.inv_w - 1.0f, v = 1.0f - ((float)row + 0.5f) * c.inv_h;
    return f3(c.fwd[0] + u * c.rx[0] + v * c.uy[0], c.fwd[1] + u * c.rx[1] + v * c.uy[1], c.fwd[2] + u * c.rx[2] + v * c.uy[2]);
}

// ------------------------------------------------------------------ ray tests: the entry point of the ray into the solid, if it lies at
// t >= tmin (a solid the ray starts inside, or enters before tmin, is not hit).  t and the outward normal (local frame) on a hit.
QS_FN float safe_dir(float d) { return qabs(d) > DIR_TINY ? d : (d < 0.0f ? -DIR_TINY : DIR_TINY); }

QS_FN bool hit_box(F3 o, F3 d, const float* e, float tmin, float& t, F3& n) {
    const float ov[3] = {o.x, o.y, o.z}, dv[3] = {safe_dir(d.x), safe_dir(d.y), safe_dir(d.z)};
    float t0 = -3.0e38f, t1 = 3.0e38f; int ax = 0;
    for (int j = 0; j < 3; j++) {
        const float inv = 1.0f / dv[j];
        const float a = (-e[j] - ov[j]) * inv, b = (e[j] - ov[j]) * inv;
        const float lo = qmin(a, b), hi = qmax(a, b);
        if (lo > t0) { t0 = lo; ax = j; }
        t1 = qmin(t1, hi);
    }
    if (!(t0 <= t1 && t0 >= tmin)) return false;
    t = t0;
    const float s = dv[ax] < 0.0f ? 1.0f : -1.0f;
    n = f3(ax == 0 ? s : 0.0f, ax == 1 ? s : 0.0f, ax == 2 ? s : 0.0f);
    return true;
}
QS_FN bool hit_cyl(F3 o, F3 d, float r, float h, float tmin, float& t, F3& n) {   // axis: local y
    bool hit = false;
    const float a = d.x * d.x + d.z * d.z;
    if (a > DIR_TINY) {   // (quadratic about the ray's closest point to the axis: b^2 - a c loses the digits of a grazing ray)
        const float tc = -(o.x * d.x + o.z * d.z) / a, qx = o.x + tc * d.x, qz = o.z + tc * d.z;
        const float disc = r * r - (qx * qx + qz * qz);
        const float ts = tc - qsqrt(qmax(disc, 0.0f) / a);
        const float y = o.y + ts * d.y;
        if (disc >= 0.0f && ts >= tmin && qabs(y) <= h) { t = ts; n = f3((o.x + ts * d.x) / r, 0.0f, (o.z + ts * d.z) / r); hit = true; }
    }
    const float dy = safe_dir(d.y), cy = dy > 0.0f ? -h : h;   // the cap that faces the ray
    const float tc = (cy - o.y) / dy;
    const float x = o.x + tc * d.x, z = o.z + tc * d.z;
    if (tc >= tmin && x * x + z * z <= r * r && (!hit || tc < t)) { t = tc; n = f3(0.0f, dy > 0.0f ? -1.0f : 1.0f, 0.0f); hit = true; }
    return hit;
}
QS_FN bool hit_sphere(F3 o, F3 d, float r, float tmin, float& t, F3& n) {
    const float a = dot3(d, d), tc = -dot3(o, d) / a;   // (about the ray's closest point to the centre, as for the cylinder)
    const F3 q = add(o, scl(d, tc));
    const float disc = r * r - dot3(q, q);
    if (disc < 0.0f) return false;
    const float ts = tc - qsqrt(disc / a);
    if (ts < tmin) return false;
    t = ts; n = scl(add(o, scl(d, ts)), 1.0f / r);
    return true;
}
// primitive P in world coordinates: the ray moves into its frame, the normal comes back
QS_FN bool hit_prim(const Prim& P, F3 o, F3 d, float tmin, float& t, F3& n) {
    const int type = prim_type(P);
    if (type == PRIM_NONE) return false;
    const F3 r = sub(o, f3(P.c[0], P.c[1], P.c[2]));
    const float* R = P.R;
    const F3 ol = f3(R[0] * r.x + R[3] * r.y + R[6] * r.z, R[1] * r.x + R[4] * r.y + R[7] * r.z, R[2] * r.x + R[5] * r.y + R[8] * r.z);
    const F3 dl = f3(R[0] * d.x + R[3] * d.y + R[6] * d.z, R[1] * d.x + R[4] * d.y + R[7] * d.z, R[2] * d.x + R[5] * d.y + R[8] * d.z);
    F3 nl;
    bool h;
    if (type == PRIM_BOX) h = hit_box(ol, dl, P.e, tmin, t, nl);
    else if (type == PRIM_CYL) h = hit_cyl(ol, dl, P.e[0], P.e[1], tmin, t, nl);
    else h = hit_sphere(ol, dl, P.e[0], tmin, t, nl);
    if (h) n = mat_vec(R, nl);
    return h;
}
// does the line o + t d come within radius r of the centre c (conservative test for skipping the primitive loop)
QS_FN bool near_sphere(F3 o, F3 d, F3 c, float r) {
    const F3 w = sub(c, o);
    const F3 x = cross3(w, d);
    return dot3(x, x) <= r * r * dot3(d, d);
}

// nearest primitive the ray enters at t >= tmin and before `tbest`: updates tbest, n, id
QS_FN void trace_prims(const Prim* P, F3 o, F3 d, float tmin, float& tbest, F3& n, int& id) {
    for (int k = 0; k < MAX_PRIM; k++) {
        float t; F3 nk;
        if (hit_prim(P[k], o, d, tmin, t, nk) && t < tbest) { tbest = t; n = nk; id = prim_id(P[k]); }
    }
}
QS_FN bool occluded(const Prim* P, F3 o, F3 d) {
    for (int k = 0; k < MAX_PRIM; k++) {
        float t; F3 nk;
        if (hit_prim(P[k], o, d, 0.0f, t, nk)) return true;
    }
    return false;
}

QS_FN uint32_t pack_rgb(float r, float g, float b) {
    const uint32_t R = (uint32_t)qfloor(qmin(qmax(r, 0.0f), 1.0f) * 255.0f + 0.5f);
    const uint32_t G = (uint32_t)qfloor(qmin(qmax(g, 0.0f), 1.0f) * 255.0f + 0.5f);
    const uint32_t B = (uint32_t)qfloor(qmin(qmax(b, 0.0f), 1.0f) * 255.0f + 0.5f);
    return R | (G << 8) | (B << 16) | 0xff000000u;
}
QS_FN void seg_rgb(int id, float& r, float& g, float& b) {
    const float* c = id == SEG_TRUNK ? TRUNK_RGB : id == SEG_PAYLOAD ? PAYLOAD_RGB : PART_RGB[(id - SEG_LEG) & 3];
    r = c[0]; g = c[1]; b = c[2];
}

struct Pixel { uint32_t rgba; float depth; int seg; };
QS_FN Pixel sky_pixel(const CamSetup& c, int seg) { Pixel px; px.rgba = pack_rgb(SKY[0], SKY[1], SKY[2]); px.depth = c.far_clip; px.seg = seg; return px; }

// Primary hit of a pixel: nearest robot primitive (when `robot`: the caller found the ray near the robot) or the ground, within [near, far].
struct Hit { float t; F3 n; int id; };
QS_FN Hit primary_hit(const Prim* P, const CamSetup& c, F3 eye, F3 d, bool robot) {
    Hit hit; hit.t = 3.0e38f; hit.n = f3(0.0f, 0.0f, 1.0f); hit.id = SEG_SKY;
    if (qabs(d.z) > DIR_TINY) {
        const float tg = -eye.z / d.z;
        if (tg >= c.near_clip) { hit.t = tg; hit.id = SEG_GROUND; }
    }
    if (robot) trace_prims(P, eye, d, c.near_clip, hit.t, hit.n, hit.id);
    if (hit.t > c.far_clip) { hit.id = SEG_SKY; hit.t = c.far_clip; }
    return hit;
}
// the hit's shade: Lambert term (0 where the surface faces away from the light, no shadow ray needed there)
QS_FN float lambert(const Hit& h) { return qmax(dot3(h.n, f3(LIGHT[0], LIGHT[1], LIGHT[2])), 0.0f); }
QS_FN F3 shadow_origin(F3 eye, F3 d, const Hit& h) { return add(add(eye, scl(d, h.t)), scl(h.n, SHADOW_EPS)); }
QS_FN Pixel shade(F3 eye, F3 d, const Hit& h, const CamSetup& c, bool shadowed) {
    if (h.id == SEG_SKY) return sky_pixel(c, SEG_SKY);
    float r, g, b;
    if (h.id == SEG_GROUND) {
        const float x = eye.x + h.t * d.x, y = eye.y + h.t * d.y;
        const int par = ((int)qfloor(x * (1.0f / CHECKER)) + (int)qfloor(y * (1.0f / CHECKER))) & 1;
        r = GROUND[par][0]; g = GROUND[par][1]; b = GROUND[par][2];
    } else {
        seg_rgb(h.id, r, g, b);
    }
    const float lit = AMBIENT + (shadowed ? 0.0f : DIFFUSE * lambert(h));
    Pixel px; px.rgba = pack_rgb(r * lit, g * lit, b * lit); px.depth = h.t; px.seg = h.id;
    return px;
}

// One pixel without a bounding-sphere skip (the host emulation; k_render makes the same decisions per wave).
QS_FN Pixel render_pixel(const Prim* P, F3 bc, float br, const CamSetup& c, F3 eye, int col, int row) {
    const F3 d = pixel_dir(c, col, row);
    const Hit h = primary_hit(P, c, eye, d, near_sphere(eye, d, bc, br));
    bool sh = false;
    if (h.id != SEG_SKY && lambert(h) > 0.0f) {
        const F3 o = shadow_origin(eye, d, h), L = f3(LIGHT[0], LIGHT[1], LIGHT[2]);
        if (near_sphere(o, L, bc, br)) sh = occluded(P, o, L);
    }
    return shade(eye, d, h, c, sh);
}

}  // namespace rnd
}  // namespace qs
