// qs_ars.hip -- k_ars_perturb, k_ars_begin, k_ars_account, k_ars_returns, k_ars_select, k_ars_apply and the C ABI of ARS's bookkeeping on the
// device (qs_ars_*; include/qs_amd.h): the candidates of an iteration, the episode accounting of its rollout without a host wait per step,
// the candidates' returns, the choice of the best directions and the parameter step.  The arithmetic and its order are csrc/qs_ars.h; every
// kernel here is that header's functions, one lane per element, and nothing else.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "qs_amd.h"
#include "qs_ars.h"
#include "qs_host.h"

namespace ar = qs::ars;

struct qs_ars {
    int n_envs, n_delta, n_params, episodes_per_env, m, device;
    hipStream_t stream;
    float* ret; int* len; int* episodes; uint8_t* alive;   // [n_envs]
    int* n_alive; unsigned long long* steps;               // device counters
    float* R;                                              // [2 n_delta]: the candidates' returns, + first
    int* idx; float* w; float* stats;                      // [n_delta], [n_delta], [2] = std, step
};

namespace {

constexpr int BLOCK = 256;

__global__ __launch_bounds__(BLOCK) void k_ars_perturb(const float* __restrict__ theta, const float* __restrict__ delta, int n_delta, int n_params, float sigma,
                                                       float* __restrict__ cand) {
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x, total = (long long)n_delta * n_params;
    if (at >= total) return;
    const float t = theta[at % n_params], d = delta[at];
    cand[at] = ar::perturb(t, d, sigma);
    cand[total + at] = ar::perturb(t, d, -sigma);
}

__global__ __launch_bounds__(BLOCK) void k_ars_begin(float* __restrict__ ret, int* __restrict__ len, int* __restrict__ episodes, uint8_t* __restrict__ alive, int n_envs,
                                                     int* __restrict__ n_alive, unsigned long long* __restrict__ steps) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e < n_envs) { ret[e] = 0.0f; len[e] = 0; episodes[e] = 0; alive[e] = 1; }
    if (e == 0) { *n_alive = n_envs; *steps = 0ULL; }
}

__global__ __launch_bounds__(BLOCK) void k_ars_account(float* __restrict__ ret, int* __restrict__ len, int* __restrict__ episodes, uint8_t* __restrict__ alive,
                                                       const float* __restrict__ raw_reward, const uint8_t* __restrict__ done, int n_envs, int episodes_per_env,
                                                       int* __restrict__ n_alive) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    int died = 0;
    if (e < n_envs && alive[e]) {                                          // (a dead environment is neither read further nor written)
        float r = ret[e];
        int l = len[e], ep = episodes[e];
        uint8_t a = 1;
        died = ar::account(r, l, ep, a, raw_reward[e], done[e], episodes_per_env);
        ret[e] = r; len[e] = l; episodes[e] = ep;
        if (died) alive[e] = 0;
    }
    const unsigned long long gone = __builtin_amdgcn_ballot_w64(died != 0);   // (every lane of the wave gets here)
    if ((threadIdx.x & (ar::WAVE - 1)) == 0 && gone) atomicSub(n_alive, (int)__builtin_popcountll(gone));
}

// one wave per candidate
__global__ __launch_bounds__(ar::WAVE) void k_ars_returns(const float* __restrict__ ret, const int* __restrict__ len, int m, float alive_bonus_offset,
                                                          float* __restrict__ R, unsigned long long* __restrict__ steps) {
    __shared__ float lanes[ar::WAVE];
    __shared__ long long lane_steps[ar::WAVE];
    const int p = blockIdx.x, c = threadIdx.x;
    long long s;
    lanes[c] = ar::lane_return(ret + (size_t)p * m, len + (size_t)p * m, m, c, alive_bonus_offset, s);
    lane_steps[c] = s;
    __syncthreads();
    if (c == 0) {
        R[p] = ar::sum_lanes(lanes);
        long long tot = 0;
        for (int k = 0; k < ar::WAVE; k++) tot += lane_steps[k];
        atomicAdd(steps, (unsigned long long)tot);
    }
}

// one workgroup of at least n_delta lanes
__global__ __launch_bounds__(ar::MAX_DELTA) void k_ars_select(const float* __restrict__ R, int n_delta, int b, float lr, int* __restrict__ idx, float* __restrict__ w,
                                                              float* __restrict__ stats) {
    __shared__ float score[ar::MAX_DELTA], v[2 * ar::MAX_DELTA];
    const int k = threadIdx.x;
    if (k < n_delta) score[k] = ar::score_of(R, n_delta, k);
    __syncthreads();
    if (k < n_delta) {
        const int r = ar::rank_of(score, n_delta, k);
        if (r < b) { idx[r] = k; w[r] = R[k] - R[n_delta + k]; v[r] = R[k]; v[b + r] = R[n_delta + k]; }
    }
    __syncthreads();
    if (k == 0) {
        float st[2];
        ar::select_stats(v, b, lr, st);
        stats[0] = st[0]; stats[1] = st[1];
    }
}

__global__ __launch_bounds__(BLOCK) void k_ars_apply(float* __restrict__ theta, const float* __restrict__ delta, int n_params, const int* __restrict__ idx,
                                                     const float* __restrict__ w, int b, const float* __restrict__ stats) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_params) theta[i] = ar::apply(theta[i], delta, n_params, i, idx, w, b, stats[1]);
}

int launch_returns(qs_ars* h, float alive_bonus_offset) {
    QS_HIP(hipMemsetAsync(h->steps, 0, sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_ars_returns, dim3((unsigned)(2 * h->n_delta)), dim3(ar::WAVE), 0, h->stream, (const float*)h->ret, (const int*)h->len, h->m, alive_bonus_offset,
                       h->R, h->steps);
    QS_LAUNCHED();
    return 0;
}

void free_all(qs_ars* h) {
    hipFree(h->ret); hipFree(h->len); hipFree(h->episodes); hipFree(h->alive); hipFree(h->n_alive); hipFree(h->steps);
    hipFree(h->R); hipFree(h->idx); hipFree(h->w); hipFree(h->stats);
}

}  // namespace

extern "C" {

int qs_ars_create(int n_envs, int n_delta, int n_params, int episodes_per_env, int device, qs_ars** out) {
    if (ar::check_shape(n_envs, n_delta, n_params, episodes_per_env, qs_g_err, sizeof(qs_g_err))) return -1;
    qs_ars* h;
    if (int rc = qs_new_handle(out, device, &h)) return rc;
    h->n_envs = n_envs; h->n_delta = n_delta; h->n_params = n_params; h->episodes_per_env = episodes_per_env;
    h->m = ar::block_of(n_envs, n_delta);
    QS_ON_DEVICE(h);
    const size_t N = (size_t)n_envs, D = (size_t)n_delta;
    ZeroedAlloc zeroed;
    zeroed(&h->ret, N); zeroed(&h->len, N); zeroed(&h->episodes, N); zeroed(&h->alive, N); zeroed(&h->n_alive, 1); zeroed(&h->steps, 1);
    zeroed(&h->R, 2 * D); zeroed(&h->idx, D); zeroed(&h->w, D); zeroed(&h->stats, 2);
    if (zeroed.failed("qs_ars_create: %d environments, %d directions", n_envs, n_delta)) { qs_ars_destroy(h); return -2; }
    *out = h;
    return 0;
}

void qs_ars_destroy(qs_ars* h) { qs_delete_handle(h, free_all); }

int qs_ars_set_stream(qs_ars* h, void* s) { return qs_set_stream_of(h, s); }

int qs_ars_perturb(qs_ars* h, const float* theta, const float* delta, float sigma, float* candidates) {
    if (!h || !theta || !delta || !candidates) QS_FAIL(-1, "null argument");
    QS_ON_DEVICE(h);
    hipLaunchKernelGGL(k_ars_perturb, dim3(qs_blocks((long long)h->n_delta * h->n_params, BLOCK)), dim3(BLOCK), 0, h->stream, theta, delta, h->n_delta, h->n_params, sigma,
                       candidates);
    QS_LAUNCHED();
    return 0;
}

int qs_ars_begin(qs_ars* h) {
    if (!h) QS_FAIL(-1, "null handle");
    QS_ON_DEVICE(h);
    hipLaunchKernelGGL(k_ars_begin, dim3(qs_blocks(h->n_envs, BLOCK)), dim3(BLOCK), 0, h->stream, h->ret, h->len, h->episodes, h->alive, h->n_envs, h->n_alive, h->steps);
    QS_LAUNCHED();
    return 0;
}

int qs_ars_account(qs_ars* h, const float* raw_reward, const uint8_t* done) {
    if (!h || !raw_reward || !done) QS_FAIL(-1, "null argument");
    QS_ON_DEVICE(h);
    hipLaunchKernelGGL(k_ars_account, dim3(qs_blocks(h->n_envs, BLOCK)), dim3(BLOCK), 0, h->stream, h->ret, h->len, h->episodes, h->alive, raw_reward, done, h->n_envs,
                       h->episodes_per_env, h->n_alive);
    QS_LAUNCHED();
    return 0;
}

int qs_ars_alive(qs_ars* h, int* out) {
    if (!h || !out) QS_FAIL(-1, "null argument");
    QS_ON_DEVICE(h);
    QS_HIP(hipMemcpyAsync(out, h->n_alive, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    QS_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int qs_ars_returns(qs_ars* h, float alive_bonus_offset) {
    if (!h) QS_FAIL(-1, "null handle");
    QS_ON_DEVICE(h);
    return launch_returns(h, alive_bonus_offset);
}

int qs_ars_finish(qs_ars* h, float* theta, const float* delta, int n_top, float learning_rate, float alive_bonus_offset) {
    if (!h || !theta || !delta) QS_FAIL(-1, "null argument");
    if (n_top < 1 || n_top > h->n_delta) QS_FAIL(-1, "qs_ars_finish: n_top = %d outside [1, n_delta = %d]", n_top, h->n_delta);
    QS_ON_DEVICE(h);
    if (int rc = launch_returns(h, alive_bonus_offset)) return rc;
    hipLaunchKernelGGL(k_ars_select, dim3(1), dim3((unsigned)((h->n_delta + ar::WAVE - 1) / ar::WAVE * ar::WAVE)), 0, h->stream, (const float*)h->R, h->n_delta, n_top,
                       learning_rate, h->idx, h->w, h->stats);
    QS_LAUNCHED();
    hipLaunchKernelGGL(k_ars_apply, dim3(qs_blocks(h->n_params, BLOCK)), dim3(BLOCK), 0, h->stream, theta, delta, h->n_params, (const int*)h->idx, (const float*)h->w, n_top,
                       (const float*)h->stats);
    QS_LAUNCHED();
    return 0;
}

int qs_ars_get(qs_ars* h, int what, void* dev_out) {
    if (!h || !dev_out) QS_FAIL(-1, "null argument");
    const size_t N = (size_t)h->n_envs, D = (size_t)h->n_delta;
    QsSpan s;
    switch (what) {
        case QS_ARS_GET_RET: s = {h->ret, N * sizeof(float)}; break;
        case QS_ARS_GET_LEN: s = {h->len, N * sizeof(int)}; break;
        case QS_ARS_GET_EPISODES: s = {h->episodes, N * sizeof(int)}; break;
        case QS_ARS_GET_ALIVE: s = {h->alive, N}; break;
        case QS_ARS_GET_N_ALIVE: s = {h->n_alive, sizeof(int)}; break;
        case QS_ARS_GET_STEPS: s = {h->steps, sizeof(unsigned long long)}; break;
        case QS_ARS_GET_RETURNS: s = {h->R, 2 * D * sizeof(float)}; break;
        case QS_ARS_GET_IDX: s = {h->idx, D * sizeof(int)}; break;
        case QS_ARS_GET_W: s = {h->w, D * sizeof(float)}; break;
        case QS_ARS_GET_STATS: s = {h->stats, 2 * sizeof(float)}; break;
        default: QS_FAIL(-1, "qs_ars_get: what = %d is no QS_ARS_GET_*", what);
    }
    return qs_copy_out(h, s, dev_out);
}

}  // extern "C"
