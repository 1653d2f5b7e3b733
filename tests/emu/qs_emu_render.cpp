// qs_emu_render.cpp -- TEST-ONLY host build of the camera images (quadruped-springs_amd/csrc/qs_render.h): the scene build, the rays and
// the shading k_render runs, one pixel at a time, with the skip decided per pixel instead of per wave (which changes no pixel).
#include <vector>
#include "../../quadruped-springs_amd/csrc/qs_render.h"

using namespace qs::rnd;

extern "C" {
// states [m][37], params [m][24] or null, blocks [m][7] (payload block position and quaternion) or null; outputs [m][H][W]
int qser_render(const float* states, const float* params, const float* blocks, int m, const qs_camera* cam, int width, int height, uint32_t* rgba,
                float* depth, int32_t* seg) {
    const CamSetup cs = camera_setup(*cam, width, height);
    for (int i = 0; i < m; i++) {
        SceneSrc ss;
        ss.st = states + (size_t)i * QS_STATE_DIM;
        ss.par = params ? params + (size_t)i * QS_PARAM_DIM : nullptr;
        ss.blk = blocks ? blocks + (size_t)i * 7 : nullptr;
        ss.draw_payload = cam->draw_payload;
        Prim P[MAX_PRIM]; float br = 0.0f;
        for (int k = 0; k < MAX_PRIM; k++) { float b; build_prim(ss, k, P[k], b); br = qmax(br, b); }
        br += BOUND_PAD;
        const F3 bc = f3(ss.st[0], ss.st[1], ss.st[2]), eye = eye_of(cs, ss.st);
        for (int r = 0; r < height; r++)
            for (int c = 0; c < width; c++) {
                const Pixel px = render_pixel(P, bc, br, cs, eye, c, r);
                const size_t o = ((size_t)i * height + r) * width + c;
                rgba[o] = px.rgba;
                if (depth) depth[o] = px.depth;
                if (seg) seg[o] = px.seg;
            }
    }
    return 0;
}
// the primitive table of one scene: [22][16] floats (R 9, centre 3, extents 3, kind as a float), and the bounds [22]
void qser_scene(const float* state, const float* params, const float* block, int draw_payload, float* out, float* bounds) {
    SceneSrc ss; ss.st = state; ss.par = params; ss.blk = block; ss.draw_payload = draw_payload;
    for (int k = 0; k < MAX_PRIM; k++) {
        Prim p; build_prim(ss, k, p, bounds[k]);
        for (int j = 0; j < 9; j++) out[k * 16 + j] = p.R[j];
        for (int j = 0; j < 3; j++) { out[k * 16 + 9 + j] = p.c[j]; out[k * 16 + 12 + j] = p.e[j]; }
        out[k * 16 + 15] = (float)p.kind;
    }
}
}
