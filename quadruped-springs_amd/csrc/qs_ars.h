// qs_ars.h -- the bookkeeping of one iteration of sb3_contrib's ARS (Augmented Random Search: ARS.evaluate_candidates' episode accounting and
// ARS._do_one_update), shared by k_ars_perturb / k_ars_begin / k_ars_account / k_ars_returns / k_ars_select / k_ars_apply (qs_ars.hip) and
// their TEST-ONLY host build (tests/emu/qs_emu_ars.cpp, tests/sanitize/drv_ars.cpp).  sb3_contrib 1.5 as remembered: the package was not
// available to check against.
//
// Numerical contract: float32 throughout.  N = P m environments, P = 2 n_delta candidates; candidate p owns the environments
// [p m, (p + 1) m) (DevicePolicy's block rule); the + candidates come first, the - candidates second (policy.ars_population's order).
//   1. perturb (one lane per (k, i)):  cand[k][i] = fmaf(sigma, delta[k][i], theta[i]);  cand[n_delta + k][i] = fmaf(-sigma, delta[k][i], theta[i])
//   2. begin:  ret = 0, len = 0, episodes = 0, alive = 1 per environment; the counters n_alive = N and steps = 0
//   3. account (one launch per environment step, one lane per environment): an alive environment does ret = ret + raw_reward (a plain add, in
//      step order) and len += 1; where done, episodes += 1 and alive = 0 once episodes == episodes_per_env.  A dead environment changes
//      nothing.  A wave in which lanes died subtracts their number from n_alive with one integer atomic.
//   4. returns (one wave per candidate):  R_p = sum_e fmaf(alive_bonus_offset, (float)len_e, ret_e)  over the block: lane c adds the block's
//      environments c, c + 64, ... in ascending order from 0 (plain adds); the 64 lane sums are then added in ascending lane order from 0.
//      A pure function of m.  The same pass sums len as integers into `steps` (an integer atomic per candidate: exact in any order).
//   5. select (one workgroup, n_delta <= MAX_DELTA, b = n_top):  score_k = fmaxf(R+_k, R-_k);
//      rank_k = #{j : score_j > score_k, or score_j == score_k and j < k};  direction k with rank_k < b is kept at position rank_k.
//      (torch.argsort leaves the order of ties unspecified; lower index first is THIS PROJECT'S rule.)
//      v = R+ in position order, then R- in position order (torch.cat's order), 2b values:
//      mean = (ascending sum of v) / 2b;  ss = ascending chain fmaf(d, d, ss) of d = v - mean;  std = sqrtf(ss / (2b - 1));
//      step = lr / fmaf((float)b, std, 1e-6f);  w_r = R+_r - R-_r.   (b = 1, R+ == R-: std = 0, step = lr / 1e-6f and w = 0; no division by zero.)
//   6. apply (one lane per parameter):  g_i = chain over positions r ascending from 0 of fmaf(w_r, delta[idx_r][i], g);  theta_i = fmaf(step, g_i, theta_i)
// No floating-point atomics, no wave waits on another, nothing depends on the grid or on timing.  sqrtf and the division are the
// platform's (correctly rounded on the host and, as the kernels are built, on the device; tests/ars_ref.py bounds them all the same).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define QA_HD __host__ __device__ inline
#else
#define QA_HD inline
#endif

namespace qs {
namespace ars {

constexpr int WAVE = 64;           // lanes of k_ars_returns' wave = chains of a candidate's sum
constexpr int MAX_DELTA = 1024;    // directions k_ars_select's one workgroup takes

QA_HD int block_of(int n_envs, int n_delta) { return n_envs / (2 * n_delta); }

// what qs_ars_create takes; returns 0 or writes why not into err
inline int check_shape(int n_envs, int n_delta, int n_params, int episodes_per_env, char* err, size_t err_size) {
#define QA_BAD(...) do { snprintf(err, err_size, __VA_ARGS__); return -1; } while (0)
    if (n_delta < 1) QA_BAD("qs_ars_create: n_delta = %d must be positive", n_delta);
    if (n_delta > MAX_DELTA) QA_BAD("qs_ars_create: n_delta = %d is above %d (the selection is one workgroup)", n_delta, MAX_DELTA);
    if (n_params < 1) QA_BAD("qs_ars_create: n_params = %d must be positive", n_params);
    if ((long long)n_delta * n_params > 0x7fffffffLL) QA_BAD("qs_ars_create: n_delta * n_params = %lld does not fit 31 bits", (long long)n_delta * n_params);
    if (n_envs < 1 || n_envs % (2 * n_delta)) QA_BAD("qs_ars_create: n_envs = %d is not a positive multiple of 2 * n_delta = %d candidates", n_envs, 2 * n_delta);
    if (episodes_per_env < 1) QA_BAD("qs_ars_create: episodes_per_env = %d must be positive", episodes_per_env);
#undef QA_BAD
    return 0;
}

// 1. called with sigma for the first n_delta candidates, with -sigma for the second
QA_HD float perturb(float theta, float delta, float sigma) { return fmaf(sigma, delta, theta); }

// 3. one environment's step; returns 1 if the environment died in it
QA_HD int account(float& ret, int& len, int& episodes, uint8_t& alive, float raw_reward, uint8_t done, int episodes_per_env) {
    if (!alive) return 0;
    ret = ret + raw_reward;
    len += 1;
    if (!done) return 0;
    episodes += 1;
    if (episodes < episodes_per_env) return 0;
    alive = 0;
    return 1;
}

// 4. lane c's share of candidate p's sum: the block's environments c, c + WAVE, ... ascending; steps receives their lengths' sum
QA_HD float lane_return(const float* ret, const int* len, int m, int c, float alive_bonus_offset, long long& steps) {
    float acc = 0.0f;
    steps = 0;
    for (int e = c; e < m; e += WAVE) {
        acc = acc + fmaf(alive_bonus_offset, (float)len[e], ret[e]);
        steps += len[e];
    }
    return acc;
}
QA_HD float sum_lanes(const float* lane_sums) {
    float tot = 0.0f;
    for (int c = 0; c < WAVE; c++) tot = tot + lane_sums[c];
    return tot;
}

// 5. R [2 n_delta]: R+ first, R- second
QA_HD float score_of(const float* R, int n_delta, int k) { return fmaxf(R[k], R[n_delta + k]); }
QA_HD int rank_of(const float* score, int n_delta, int k) {
    const float s = score[k];
    int rank = 0;
    for (int j = 0; j < n_delta; j++) rank += (score[j] > s || (score[j] == s && j < k)) ? 1 : 0;
    return rank;
}
// v [2b] in position order (R+ then R-) -> out[0] = std, out[1] = step
QA_HD void select_stats(const float* v, int b, float lr, float* out) {
    const int n = 2 * b;
    float sum = 0.0f;
    for (int i = 0; i < n; i++) sum = sum + v[i];
    const float mean = sum / (float)n;
    float ss = 0.0f;
    for (int i = 0; i < n; i++) { const float d = v[i] - mean; ss = fmaf(d, d, ss); }
    const float sd = sqrtf(ss / (float)(n - 1));
    out[0] = sd;
    out[1] = lr / fmaf((float)b, sd, 1e-6f);
}

// 6. parameter i
QA_HD float apply(float theta, const float* delta, int n_params, int i, const int* idx, const float* w, int b, float step) {
    float g = 0.0f;
    for (int r = 0; r < b; r++) g = fmaf(w[r], delta[(size_t)idx[r] * n_params + i], g);
    return fmaf(step, g, theta);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: every kernel as plain loops over its lanes
inline void perturb_host(const float* theta, const float* delta, int n_delta, int n_params, float sigma, float* cand) {
    for (int k = 0; k < n_delta; k++)
        for (int i = 0; i < n_params; i++) {
            const float d = delta[(size_t)k * n_params + i];
            cand[(size_t)k * n_params + i] = perturb(theta[i], d, sigma);
            cand[(size_t)(n_delta + k) * n_params + i] = perturb(theta[i], d, -sigma);
        }
}
inline void begin_host(float* ret, int* len, int* episodes, uint8_t* alive, int n_envs, int* n_alive) {
    for (int e = 0; e < n_envs; e++) { ret[e] = 0.0f; len[e] = 0; episodes[e] = 0; alive[e] = 1; }
    *n_alive = n_envs;
}
inline void account_host(float* ret, int* len, int* episodes, uint8_t* alive, const float* raw_reward, const uint8_t* done, int n_envs, int episodes_per_env,
                         int* n_alive) {
    for (int e = 0; e < n_envs; e++) *n_alive -= account(ret[e], len[e], episodes[e], alive[e], raw_reward[e], done[e], episodes_per_env);
}
// R [2 n_delta]; returns the sum of all lengths
inline long long returns_host(const float* ret, const int* len, int n_envs, int n_delta, float alive_bonus_offset, float* R) {
    const int m = block_of(n_envs, n_delta);
    long long steps = 0;
    for (int p = 0; p < 2 * n_delta; p++) {
        float lanes[WAVE];
        for (int c = 0; c < WAVE; c++) {
            long long s;
            lanes[c] = lane_return(ret + (size_t)p * m, len + (size_t)p * m, m, c, alive_bonus_offset, s);
            steps += s;
        }
        R[p] = sum_lanes(lanes);
    }
    return steps;
}
// idx [b], w [b], stats [2] = std, step; scratch-free for n_delta <= MAX_DELTA
inline void select_host(const float* R, int n_delta, int b, float lr, int* idx, float* w, float* stats) {
    static thread_local float score[MAX_DELTA], v[2 * MAX_DELTA];
    for (int k = 0; k < n_delta; k++) score[k] = score_of(R, n_delta, k);
    for (int k = 0; k < n_delta; k++) {
        const int r = rank_of(score, n_delta, k);
        if (r < b) { idx[r] = k; w[r] = R[k] - R[n_delta + k]; v[r] = R[k]; v[b + r] = R[n_delta + k]; }
    }
    select_stats(v, b, lr, stats);
}
inline void apply_host(float* theta, const float* delta, int n_params, const int* idx, const float* w, int b, float step) {
    for (int i = 0; i < n_params; i++) theta[i] = apply(theta[i], delta, n_params, i, idx, w, b, step);
}
#endif

}  // namespace ars
}  // namespace qs
