// qs_mpc.hip -- k_mpc_sample, k_mpc_feed, k_mpc_finish, k_mpc_set_plan and the C ABI of the sampling planner on the device (qs_mpc_*;
// include/qs_amd.h): the candidates' action sequences around the plan, the slab of actions and the scores of every horizon step in one
// launch next to the step kernel, and the choice of the next plan (best of C, or MPPI's weighted mean) with one workgroup per robot.  The
// arithmetic and its order are csrc/qs_mpc.h; every kernel here is that header's functions and nothing else.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "qs_amd.h"
#include "qs_mpc.h"
#include "qs_host.h"

namespace mp = qs::mpc;

struct qs_mpc {
    int M, C, H, d, device;
    hipStream_t stream;
    float* plan;        // [M][H][d]
    float* seq;         // [H][M C][d]
    float* score;       // [M C]
    uint8_t* running;   // [M C]
    int* best;          // [M]
    float* best_score;  // [M]
};

namespace {

constexpr int BLOCK = 256;

// one lane per (h, i, j); total = H M C d < 2^31
__global__ __launch_bounds__(BLOCK) void k_mpc_sample(const float* __restrict__ plan, const float* __restrict__ eps, int MC, int C, int H, int d, float sigma,
                                                      float* __restrict__ seq, float* __restrict__ score, uint8_t* __restrict__ running) {
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x, total = (long long)H * MC * d;
    if (at >= total) return;
    const int j = (int)(at % d);
    const long long hi = at / d;
    const int i = (int)(hi % MC), h = (int)(hi / MC);
    const int m = i / C, c = i - m * C;
    seq[at] = mp::sample(plan[((size_t)m * H + h) * d + j], eps[at], sigma, c);
    if (at < MC) { score[at] = 0.0f; running[at] = 1; }                    // (H d >= 1: the first MC lanes exist)
}

// one lane per element of the action slab: M C d lanes, of which the first M C account a candidate each and the first M <= M C clear a real
// robot's flag.  reward and done are read for step >= 1, reward_end at step == H, active may be null.
__global__ __launch_bounds__(BLOCK) void k_mpc_feed(int step, const float* __restrict__ seq, float* __restrict__ score, uint8_t* __restrict__ running, int M, int MC,
                                                    int H, int d, const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                    const float* __restrict__ reward_end, int stride, float* __restrict__ actions, uint8_t* __restrict__ active) {
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x, slab = (long long)MC * d;
    if (at < MC) {
        const int i = (int)at;
        uint8_t run = running[i];
        if (step >= 1) {
            float s = score[i];
            const bool last = step == H;
            mp::account(s, run, reward[M + i], done[M + i], last, last ? reward_end[(size_t)(M + i) * stride] : 0.0f);
            score[i] = s;
            running[i] = run;
        }
        if (active) active[M + i] = run;
    }
    if (active && at < M) active[at] = 0;
    if (step < H && at < slab) actions[(size_t)M * d + at] = seq[(size_t)step * slab + at];
}

// one workgroup per robot, blockDim.x = H d rounded up to whole waves (<= MAX_ELEMENTS)
__global__ __launch_bounds__(mp::MAX_ELEMENTS) void k_mpc_finish(const float* __restrict__ seq, const float* __restrict__ score, int MC, int C, int H, int d, int method,
                                                                 float lambda, float* __restrict__ plan, float* __restrict__ actions, int* __restrict__ best,
                                                                 float* __restrict__ best_score) {
    __shared__ float w[mp::MAX_CANDIDATES];
    __shared__ float red_s[mp::MAX_ELEMENTS];
    __shared__ int red_c[mp::MAX_ELEMENTS];
    __shared__ uint8_t red_ok[mp::MAX_ELEMENTS];
    __shared__ float lanes[mp::WAVE];
    const int m = blockIdx.x, tid = threadIdx.x, B = blockDim.x;
    const float* sc = score + (size_t)m * C;
    // the best candidate: every lane's share, then a tree over the lanes (a total order: the winner does not depend on the tree)
    {
        bool ok; float s; int c;
        mp::best_of(sc, C, tid, B, ok, s, c);
        red_ok[tid] = ok; red_s[tid] = s; red_c[tid] = c;
    }
    __syncthreads();
    int span = 1;
    while (span < B) span <<= 1;
    for (int half = span >> 1; half >= 1; half >>= 1) {
        if (tid < half && tid + half < B) {
            const int o = tid + half;
            if (mp::ahead(red_ok[o], red_s[o], red_c[o], red_ok[tid], red_s[tid], red_c[tid])) { red_ok[tid] = red_ok[o]; red_s[tid] = red_s[o]; red_c[tid] = red_c[o]; }
        }
        __syncthreads();
    }
    const bool ok = red_ok[0];
    const float s_max = red_s[0];                          // (0 where no score is finite: read by nobody then)
    const int b = ok ? red_c[0] : 0;
    if (tid == 0) {
        best[m] = b;
        if (ok) best_score[m] = s_max; else mp::store_bits(best_score + m, mp::MINUS_INF_BITS);
    }
    const bool mean = method == mp::METHOD_MPPI && ok;      // (uniform over the workgroup: the barriers below are reached by all or none)
    float Z = 0.0f;
    if (mean) {
        for (int c = tid; c < C; c += B) w[c] = mp::weight(sc + c, s_max, lambda);
        __syncthreads();
        if (tid < mp::WAVE) lanes[tid] = mp::lane_sum(w, C, tid);
        __syncthreads();
        Z = mp::sum_lanes(lanes);
    }
    if (tid >= H * d) return;
    const int h = tid / d, j = tid - h * d;
    const float* e = seq + ((size_t)h * MC + (size_t)m * C) * d + j;
    const float v = mean ? mp::mppi_element(w, e, C, d, Z) : e[(size_t)b * d];
    if (h == 0) actions[(size_t)m * d + j] = v;
    if (h >= 1) plan[((size_t)m * H + h - 1) * d + j] = v;
    if (h == H - 1) plan[((size_t)m * H + h) * d + j] = v;
}

// one lane per element of plan
__global__ __launch_bounds__(BLOCK) void k_mpc_set_plan(float* __restrict__ plan, const float* __restrict__ src, const uint8_t* __restrict__ mask, int M, int Hd) {
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (at >= (long long)M * Hd) return;
    if (mask && !mask[at / Hd]) return;
    plan[at] = src ? src[at] : 0.0f;
}

void free_all(qs_mpc* h) {
    hipFree(h->plan); hipFree(h->seq); hipFree(h->score); hipFree(h->running); hipFree(h->best); hipFree(h->best_score);
}

}  // namespace

extern "C" {

int qs_mpc_create(int n_robots, int n_candidates, int horizon, int action_dim, int device, qs_mpc** out) {
    if (mp::check_shape(n_robots, n_candidates, horizon, action_dim, qs_g_err, sizeof(qs_g_err))) return -1;
    qs_mpc* h;
    if (int rc = qs_new_handle(out, device, &h)) return rc;
    h->M = n_robots; h->C = n_candidates; h->H = horizon; h->d = action_dim;
    QS_ON_DEVICE(h);
    const size_t M = (size_t)n_robots, MC = M * n_candidates, Hd = (size_t)horizon * action_dim;
    ZeroedAlloc zeroed;                                                        // (the first plan is zero)
    zeroed(&h->plan, M * Hd); zeroed(&h->seq, MC * Hd); zeroed(&h->score, MC); zeroed(&h->running, MC); zeroed(&h->best, M); zeroed(&h->best_score, M);
    if (zeroed.failed("qs_mpc_create: %d robots x %d candidates x horizon %d", n_robots, n_candidates, horizon)) { qs_mpc_destroy(h); return -2; }
    *out = h;
    return 0;
}

void qs_mpc_destroy(qs_mpc* h) { qs_delete_handle(h, free_all); }

int qs_mpc_set_stream(qs_mpc* h, void* s) { return qs_set_stream_of(h, s); }

int qs_mpc_sample(qs_mpc* h, const float* eps, float sigma) {
    if (!h || !eps) QS_FAIL(-1, "null argument");
    if (mp::check_sigma(sigma, qs_g_err, sizeof(qs_g_err))) return -1;
    QS_ON_DEVICE(h);
    const int MC = h->M * h->C;
    hipLaunchKernelGGL(k_mpc_sample, dim3(qs_blocks((long long)h->H * MC * h->d, BLOCK)), dim3(BLOCK), 0, h->stream, (const float*)h->plan, eps, MC, h->C, h->H, h->d, sigma,
                       h->seq, h->score, h->running);
    QS_LAUNCHED();
    return 0;
}

int qs_mpc_feed(qs_mpc* h, int step, const float* reward, const uint8_t* done, const float* reward_end, int reward_end_stride, float* actions, uint8_t* active) {
    if (!h || !actions) QS_FAIL(-1, "null argument");
    if (step < 0 || step > h->H) QS_FAIL(-1, "qs_mpc_feed: step = %d outside [0, horizon = %d]", step, h->H);
    if (step >= 1 && (!reward || !done)) QS_FAIL(-1, "qs_mpc_feed: step = %d accounts the step before it and needs reward and done", step);
    if (step == h->H && (!reward_end || reward_end_stride < 1)) QS_FAIL(-1, "qs_mpc_feed: step = horizon needs reward_end and a positive row stride");
    QS_ON_DEVICE(h);
    const int MC = h->M * h->C;
    hipLaunchKernelGGL(k_mpc_feed, dim3(qs_blocks((long long)MC * h->d, BLOCK)), dim3(BLOCK), 0, h->stream, step, (const float*)h->seq, h->score, h->running, h->M, MC, h->H,
                       h->d, reward, done, reward_end, reward_end_stride, actions, active);
    QS_LAUNCHED();
    return 0;
}

int qs_mpc_finish(qs_mpc* h, int method, float lambda, float* actions) {
    if (!h || !actions) QS_FAIL(-1, "null argument");
    if (method != QS_MPC_BEST && method != QS_MPC_MPPI) QS_FAIL(-1, "qs_mpc_finish: method = %d is no QS_MPC_BEST / QS_MPC_MPPI", method);
    if (method == QS_MPC_MPPI && mp::check_lambda(lambda, qs_g_err, sizeof(qs_g_err))) return -1;
    QS_ON_DEVICE(h);
    const unsigned lanes = (unsigned)((h->H * h->d + mp::WAVE - 1) / mp::WAVE * mp::WAVE);
    hipLaunchKernelGGL(k_mpc_finish, dim3((unsigned)h->M), dim3(lanes), 0, h->stream, (const float*)h->seq, (const float*)h->score, h->M * h->C, h->C, h->H, h->d, method,
                       lambda, h->plan, actions, h->best, h->best_score);
    QS_LAUNCHED();
    return 0;
}

int qs_mpc_set_plan(qs_mpc* h, const float* plan, const uint8_t* mask) {
    if (!h) QS_FAIL(-1, "null handle");
    QS_ON_DEVICE(h);
    const int Hd = h->H * h->d;
    hipLaunchKernelGGL(k_mpc_set_plan, dim3(qs_blocks((long long)h->M * Hd, BLOCK)), dim3(BLOCK), 0, h->stream, h->plan, plan, mask, h->M, Hd);
    QS_LAUNCHED();
    return 0;
}

int qs_mpc_get(qs_mpc* h, int what, void* dev_out) {
    if (!h || !dev_out) QS_FAIL(-1, "null argument");
    const size_t M = (size_t)h->M, MC = M * h->C, Hd = (size_t)h->H * h->d;
    QsSpan s;
    switch (what) {
        case QS_MPC_GET_PLAN: s = {h->plan, M * Hd * sizeof(float)}; break;
        case QS_MPC_GET_SEQ: s = {h->seq, MC * Hd * sizeof(float)}; break;
        case QS_MPC_GET_SCORE: s = {h->score, MC * sizeof(float)}; break;
        case QS_MPC_GET_RUNNING: s = {h->running, MC}; break;
        case QS_MPC_GET_BEST: s = {h->best, M * sizeof(int)}; break;
        case QS_MPC_GET_BEST_SCORE: s = {h->best_score, M * sizeof(float)}; break;
        default: QS_FAIL(-1, "qs_mpc_get: what = %d is no QS_MPC_GET_*", what);
    }
    return qs_copy_out(h, s, dev_out);
}

}  // extern "C"
