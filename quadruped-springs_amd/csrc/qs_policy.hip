// qs_policy.hip -- k_policy and the C ABI of policy inference (qs_policy_*; include/qs_amd.h): model.predict(obs) of load_model.py:132
// for every environment in ONE launch, with one parameter row per block of environments (ARS's candidates).
//
// A wave takes 16 consecutive environments of one policy; a workgroup is 1, 2 or 4 such waves of the SAME policy and shares that
// policy's weights.  Layer by layer: the workgroup stages the layer's weights k-major into LDS ([k][out_pad]; layers over 48 KB in
// k-chunks, the accumulators stay in registers across chunks), then every wave runs D[out][env] += W[out][k] h[k][env] on
// v_mfma_f32_16x16x4_f32 with one accumulator tile per 16 outputs (up to 16 independent tiles, which covers the instruction's dependent
// latency).  A = the weights (lane l: output 16 t + (l & 15), k = l >> 4), B = the wave's activations (lane l: k = l >> 4, environment
// l & 15) from the wave's own LDS rows [env][k]; the result has the environment on the lane and four consecutive outputs in the
// registers, so it goes back to those rows as one 16-byte store per tile.  Nothing intermediate touches global memory.  Environments
// past the end of a policy's block are masked lanes (zero observation, no store): tiles never straddle two policies.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "qs_policy.h"
#include "qs_host.h"

using namespace qs::pol;

namespace {
struct PolicyArgs {
    const float* obs; const float* params; const float* eps; const float* log_std;
    float* actions; float* mean_out; float* log_prob;
    int n_per, tiles_per_policy, wg_per_policy, act_stride, w_floats;
};
}  // namespace

struct qs_policy {
    qs_policy_desc desc;
    Net net;
    int device, n_per, tiles_per_policy, waves, wg_per_policy, act_stride, w_floats;
    size_t lds_bytes;
    void (*kernel)(Net, PolicyArgs);   // k_policy<4> or k_policy<16>, chosen at create
    hipStream_t stream;
    const float* params;      // the caller's [n_policies][n_params] (kept, not copied)
};

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// a wave's LDS rows are written by some of its lanes and read by others: LDS serves one wave's accesses in order, the compiler must keep them so
#define QP_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// NT: accumulator tiles a layer may need (4: every width <= 64; 16: widths up to 256)
template <int NT>
__global__ __launch_bounds__(256) void k_policy(Net net, PolicyArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ f32x4 qp_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const int e = lane & 15, g = lane >> 4;
    const int p = blockIdx.x / a.wg_per_policy, tile = (blockIdx.x - p * a.wg_per_policy) * n_waves + wave;
    const bool tile_on = tile < a.tiles_per_policy;                       // (wave-uniform)
    const int S = a.act_stride;
    float* const sw = (float*)qp_lds;
    float* const sa = sw + a.w_floats + (size_t)wave * TILE * S;          // this wave's activations [16][S]
    const int row0 = tile * TILE;                                         // first environment of the tile inside the policy's block
    const int rows = tile_on ? min(TILE, a.n_per - row0) : 0;
    const size_t env0 = (size_t)p * a.n_per + row0;
    const float* const par = a.params + (size_t)p * net.n_params;

    // observations: the tile's rows are contiguous in memory
    {
        const int od = net.obs_dim, od4 = round_up(od, 4);
        const float* src = a.obs + env0 * od;
        for (int i = lane; i < rows * od; i += 64) { const int r = i / od; sa[r * S + (i - r * od)] = src[i]; }
        for (int i = lane; i < TILE * od4; i += 64) { const int r = i / od4, k = i - r * od4; if (r >= rows || k >= od) sa[r * S + k] = 0.0f; }
    }
    QP_WAVE_SYNC();

    for (int l = 0; l < net.n_layers; l++) {
        const int in = net.in[l], out = net.out[l], in4 = round_up(in, 4), nt = (out + TILE - 1) / TILE, op = out_pad(out);
        int kc = (a.w_floats / op) & ~3;
        if (kc > in4) kc = in4;
        const float* const W = par + net.w_off[l];
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (t < nt && net.has_bias) {
#pragma unroll
                for (int r = 0; r < 4; r++) { const int o = TILE * t + 4 * g + r; acc[t][r] = o < out ? par[net.b_off[l] + o] : 0.0f; }
            }
        }
        for (int k0 = 0; k0 < in4; k0 += kc) {
            const int kn = min(kc, in4 - k0);
            __syncthreads();                                             // every wave is done with the previous image
            for (int i = tid; i < nt * TILE * kn; i += blockDim.x) {    // k fastest: rows of W are read along k
                const int o = i / kn, k = i - o * kn;
                sw[k * op + o] = (o < out && k0 + k < in) ? W[(size_t)o * in + k0 + k] : 0.0f;
            }
            __syncthreads();
            if (tile_on) {
                for (int s = 0; s < kn; s += 4) {
                    const float b = sa[e * S + k0 + s + g];
                    const float* const wk = sw + (s + g) * op + e;
#pragma unroll
                    for (int t = 0; t < NT; t++)
                        if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[TILE * t], b, acc[t], 0, 0, 0);
                }
            }
        }
        const bool last = l == net.n_layers - 1;
        const int kind = last ? (net.squash ? (int)QS_POLICY_ACT_TANH : (int)QS_POLICY_ACT_NONE) : net.activation;
        // outputs past `out` are act(0) = 0: the zero k of the next layer's last MFMA step
#pragma unroll
        for (int t = 0; t < NT; t++)
            if (t < nt) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; r++) v[r] = activate(acc[t][r], kind);
                *(f32x4*)(sa + e * S + TILE * t + 4 * g) = v;
            }
        QP_WAVE_SYNC();
    }

    if (e < rows) {
        const int A = net.action_dim;
        const size_t env = env0 + e;
        const float* const eps_row = a.eps ? a.eps + env * A : nullptr;
        for (int j = g; j < A; j += 4)
            epilogue_elem(net, sa[e * S + j], eps_row, a.log_std, j, a.actions + env * A, a.mean_out ? a.mean_out + env * A : nullptr);
        if (a.log_prob && g == 0) a.log_prob[env] = log_prob_row(net, eps_row, a.log_std);
    }
#endif
}

}  // namespace

extern "C" {

int qs_policy_create(const qs_policy_desc* d, int device, qs_policy** out) {
    if (!d || !out) QS_FAIL(-1, "null argument");
    Net net;
    if (net_from_desc(*d, net, qs_g_err, sizeof(qs_g_err))) return -1;
    qs_policy* h;
    if (int rc = qs_new_handle(out, device, &h)) return rc;
    h->desc = *d; h->net = net;
    h->n_per = d->n_envs / d->n_policies;
    h->tiles_per_policy = (h->n_per + TILE - 1) / TILE;
    const Net* nets[1] = {&h->net};
    int wide;
    layout_sizes(nets, 1, h->act_stride, h->w_floats, wide);
    h->waves = waves_per_workgroup(h->tiles_per_policy, d->n_policies, h->w_floats, 1, h->act_stride);
    h->wg_per_policy = (h->tiles_per_policy + h->waves - 1) / h->waves;
    h->lds_bytes = lds_bytes(h->w_floats, h->waves, 1, h->act_stride);
    h->kernel = wide ? k_policy<16> : k_policy<4>;
    QS_ON_DEVICE(h);
    hipError_t e = hipFuncSetAttribute((const void*)h->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes);
    if (e != hipSuccess) { snprintf(qs_g_err, sizeof(qs_g_err), "hipFuncSetAttribute(%zu bytes of LDS) failed: %s", h->lds_bytes, hipGetErrorString(e)); delete h; return -2; }
    *out = h;
    return 0;
}

void qs_policy_destroy(qs_policy* h) { qs_delete_handle(h, [](qs_policy*) {}); }   // (no device memory of its own)

int qs_policy_set_stream(qs_policy* h, void* s) { return qs_set_stream_of(h, s); }

int qs_policy_param_count(const qs_policy* h) { if (!h) QS_FAIL(-1, "null handle"); return h->net.n_params; }

int qs_policy_set_params(qs_policy* h, const float* dev_params) {
    if (!h || !dev_params) QS_FAIL(-1, "null argument");
    h->params = dev_params;
    return 0;
}

int qs_policy_act(qs_policy* h, const float* obs, const float* eps, const float* log_std, float* actions, float* mean_out, float* log_prob) {
    if (!h || !obs || !actions) QS_FAIL(-1, "null argument (handle, obs and actions are required)");
    if (!h->params) QS_FAIL(-1, "qs_policy_act before qs_policy_set_params");
    if (eps && !log_std) QS_FAIL(-1, "eps given without log_std");
    if (log_prob && !eps) QS_FAIL(-1, "log_prob asked for without eps");
    QS_ON_DEVICE(h);
    PolicyArgs a;
    a.obs = obs; a.params = h->params; a.eps = eps; a.log_std = log_std; a.actions = actions; a.mean_out = mean_out; a.log_prob = log_prob;
    a.n_per = h->n_per; a.tiles_per_policy = h->tiles_per_policy; a.wg_per_policy = h->wg_per_policy; a.act_stride = h->act_stride; a.w_floats = h->w_floats;
    const dim3 grid((unsigned)(h->desc.n_policies * h->wg_per_policy)), block(64 * h->waves);
    hipLaunchKernelGGL(h->kernel, grid, block, h->lds_bytes, h->stream, h->net, a);
    QS_LAUNCHED();
    return 0;
}

}  // extern "C"
