// qs_render.hip -- k_render and the C ABI of camera images (qs_render, qs_render_states; include/qs_amd.h).
//
// One workgroup of 256 threads renders a 16 x 16 block of one environment's image (grid: blocks of the image x environments); a wave is
// four image rows of 16 pixels.  The first 22 lanes pose the environment's primitives into LDS (22 x 64 B), then every thread casts the
// ray of its pixel (qs_render.h).  Most pixels see only floor and sky: a lane tests its primary ray and then its shadow ray against the
// robot's bounding sphere, and the wave runs the primitive loop only when some lane's ray comes near it (the branch is wave-uniform; a lane
// whose ray misses the sphere finds no primitive in the loop either, so the skip decides the cost, never the picture).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "qs_render.h"
#include "qs_host.h"

namespace {
using namespace qs::rnd;

// where environment e's rows are: the handle's records (state at R_POS, parameters at R_PARAMS, block at R_BLOCK) or caller arrays
struct RenderSrc {
    const float* st; long long st_stride;
    const float* par; long long par_stride;   // or null
    const float* blk; long long blk_stride;   // or null
    const int32_t* ids; int n_envs;           // qs_render: env_ids; qs_render_states: null (the image's own row)
    unsigned long long* refused;
};

__global__ __launch_bounds__(TILE * TILE) void k_render(RenderSrc src, CamSetup cam, int tiles_x, int m0, uint32_t* __restrict__ rgba,
                                                         float* __restrict__ depth, int32_t* __restrict__ seg) {
    __shared__ Prim sp[MAX_PRIM];
    __shared__ float sbound[MAX_PRIM];
    const int tid = threadIdx.x;
    const int img = m0 + blockIdx.y;
    const int col = (blockIdx.x % tiles_x) * TILE + (tid & (TILE - 1)), row = (blockIdx.x / tiles_x) * TILE + tid / TILE;
    const bool inside = col < cam.width && row < cam.height;
    const size_t pix = ((size_t)img * cam.height + (inside ? row : 0)) * cam.width + (inside ? col : 0);
    int env = img;
    if (src.ids) {
        env = src.ids[img];
        if (env < 0 || env >= src.n_envs) {   // (the same for the whole workgroup)
            if (tid == 0) atomicCAS(src.refused, 0ull, (unsigned long long)img + 1ull);
            if (inside) {
                const Pixel px = sky_pixel(cam, SEG_BAD_ENV);
                rgba[pix] = px.rgba;
                if (depth) depth[pix] = px.depth;
                if (seg) seg[pix] = px.seg;
            }
            return;
        }
    }
    const float* st = src.st + (size_t)env * src.st_stride;
    if (tid < MAX_PRIM) {
        SceneSrc ss;
        ss.st = st; ss.draw_payload = cam.draw_payload;
        ss.par = src.par ? src.par + (size_t)env * src.par_stride : nullptr;
        ss.blk = src.blk ? src.blk + (size_t)env * src.blk_stride : nullptr;
        Prim p; float b;
        build_prim(ss, tid, p, b);
        sp[tid] = p; sbound[tid] = b;
    }
    __syncthreads();
    float br = 0.0f;
    for (int k = 0; k < MAX_PRIM; k++) br = qmax(br, sbound[k]);
    br += BOUND_PAD;
    const F3 bc = f3(st[0], st[1], st[2]);
    const F3 eye = eye_of(cam, st);
    const F3 d = pixel_dir(cam, col, row);
    const Hit h = primary_hit(sp, cam, eye, d, __any(near_sphere(eye, d, bc, br)));
    const bool want = h.id != SEG_SKY && lambert(h) > 0.0f;
    const F3 o = shadow_origin(eye, d, h), L = f3(LIGHT[0], LIGHT[1], LIGHT[2]);
    bool sh = false;
    if (__any(want && near_sphere(o, L, bc, br))) sh = want && occluded(sp, o, L);
    if (!inside) return;
    const Pixel px = shade(eye, d, h, cam, sh);
    rgba[pix] = px.rgba;
    if (depth) depth[pix] = px.depth;
    if (seg) seg[pix] = px.seg;
}

int check_args(int m, const qs_camera* cam, int width, int height, const uint32_t* rgba) {
    if (m < 0) QS_FAIL(-1, "m = %d must not be negative", m);
    if (!cam) QS_FAIL(-1, "null camera");
    if (width < 1 || width > 8192 || height < 1 || height > 8192) QS_FAIL(-1, "image size %d x %d outside [1, 8192]", width, height);
    if (!rgba) QS_FAIL(-1, "null rgba");
    if (!(cam->fov_deg > 0.0f && cam->fov_deg < 180.0f)) QS_FAIL(-1, "fov_deg = %g outside (0, 180)", (double)cam->fov_deg);
    if (!(cam->near_clip > 0.0f && cam->near_clip < cam->far_clip)) QS_FAIL(-1, "need 0 < near_clip < far_clip (got %g, %g)", (double)cam->near_clip, (double)cam->far_clip);
    return 0;
}

// launches over chunks of images: gridDim.y <= 65535, and a grid's work-items fit 32 bits
int launch(const RenderSrc& src, const qs_camera* cam, int m, int width, int height, uint32_t* rgba, float* depth, int32_t* seg, hipStream_t stream) {
    const CamSetup cs = camera_setup(*cam, width, height);
    const int tx = (width + TILE - 1) / TILE, ty = (height + TILE - 1) / TILE;
    const long long tiles = (long long)tx * ty;
    long long per = (0x7fffffffLL / (tiles * TILE * TILE));
    if (per > 65535) per = 65535;
    for (int m0 = 0; m0 < m; m0 += (int)per) {
        const int n = (int)(m - m0 < per ? m - m0 : per);
        hipLaunchKernelGGL(k_render, dim3((unsigned)tiles, n), dim3(TILE * TILE), 0, stream, src, cs, tx, m0, rgba, depth, seg);
        QS_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int qs_render(qs_handle* h, const int32_t* env_ids, int m, const qs_camera* cam, int width, int height, uint32_t* rgba, float* depth, int32_t* seg) {
    if (!h) QS_FAIL(-1, "null handle");
    if (int rc = check_args(m, cam, width, height, rgba)) return rc;
    if (m > 0 && !env_ids) QS_FAIL(-1, "null env_ids");
    if (m == 0) return 0;
    QsRenderView v;
    qs_render_view(h, &v);
    DeviceGuard guard(v.device);
    RenderSrc src;
    src.st = v.rec + R_POS; src.st_stride = QS_REC;
    src.par = v.rec + R_PARAMS; src.par_stride = QS_REC;
    src.blk = v.payload_soft ? v.rec + R_BLOCK : nullptr; src.blk_stride = QS_REC;
    src.ids = env_ids; src.n_envs = v.n_envs; src.refused = v.refused;
    return launch(src, cam, m, width, height, rgba, depth, seg, v.stream);
}

int qs_render_states(const float* states, const float* params, int m, const qs_camera* cam, int width, int height, uint32_t* rgba, float* depth,
                     int32_t* seg, void* stream) {
    if (int rc = check_args(m, cam, width, height, rgba)) return rc;
    if (m > 0 && !states) QS_FAIL(-1, "null states");
    if (m == 0) return 0;
    RenderSrc src;
    src.st = states; src.st_stride = QS_STATE_DIM;
    src.par = params; src.par_stride = QS_PARAM_DIM;
    src.blk = nullptr; src.blk_stride = 0;
    src.ids = nullptr; src.n_envs = m; src.refused = nullptr;
    return launch(src, cam, m, width, height, rgba, depth, seg, (hipStream_t)stream);
}

}  // extern "C"
