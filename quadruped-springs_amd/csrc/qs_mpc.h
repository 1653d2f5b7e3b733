// qs_mpc.h -- the planner side of sampling MPC (predictive sampling and MPPI, examples/mpc.py): the candidates' action sequences, their scores over
// a rollout and the choice of the next plan, shared by k_mpc_sample / k_mpc_feed / k_mpc_finish / k_mpc_set_plan (qs_mpc.hip) and their
// TEST-ONLY host build (tests/emu/qs_emu_mpc.cpp, tests/sanitize/drv_mpc.cpp).
//
// Layout: M real robots are the environments [0, M); candidate c of robot m is environment M + m C + c, so N = M (1 + C); i = m C + c indexes
// candidates; H is the horizon, d the action dimension.  plan [M][H][d]; seq and eps [H][M C][d] (step h of every candidate is one contiguous
// slab, the one that goes into actions[M:]); score [M C]; running uint8 [M C]; best int32 [M]; best_score [M].  float32 throughout.
//
// Numerical contract:
//   1. sample (one lane per (h, i, j)):  c >= 1: seq[h][i][j] = clamp(fmaf(sigma, eps[h][i][j], plan[m][h][j]), -1, 1);  c == 0: seq[h][i][j] =
//      plan[m][h][j] as it stands, not clamped (candidate 0 is the plan, bit for bit);  score[i] = 0, running[i] = 1.
//   2. feed(h), h = 0 .. H (one launch per horizon step, one lane per element):  for h >= 1 candidate i accounts step h - 1: if running[i] then
//      score[i] = score[i] + reward[M + i] (a plain add, in step order); then running[i] &= !done[M + i].  For h < H, actions[M:] = seq[h].  For
//      h == H a candidate still running adds reward_end[(M + i) stride] (what the task would pay where it stands).  With a mask:
//      active[M + i] = running[i] (as just updated), active[m] = 0.
//   3. finish (one workgroup per robot):  a score that is not finite counts as -inf.  s_max = the maximum over c, best = the LOWEST c that has
//      it (torch.argmax leaves ties unspecified on the device; lower index first is THIS PROJECT'S rule).  No finite score at all: best = 0,
//      s_max = -inf, and under either method the result is candidate 0.
//        best:  chosen = seq[:, m C + best, :]
//        mppi:  w_c = exp_nonpos((s_c - s_max) / lambda), 0 for a -inf score (the division is the platform's, correctly rounded);
//               Z = sum of the w_c: lane l adds the candidates l, l + 64, ... ascending (plain adds), then the 64 lane sums are added
//               ascending from lane 0 (qs_ars.h's order);  chosen[h][j] = clamp(a / Z, -1, 1), a = chain over c ascending from 0 of
//               fmaf(w_c, seq[h][m C + c][j], a), one lane per element.
//      Then actions[m] = chosen[0];  plan[m][h] = chosen[h + 1] for h < H - 1, plan[m][H - 1] = chosen[H - 1] (the last action held).
//   4. exp_nonpos(x), x <= 0:  0 for x < EXP_CUT = -87 (below it exp leaves float32's normal range: every result is 0 or a normal number and the
//      scaling by 2^k is exact);  otherwise k = rintf(x * LOG2E), r = fmaf(k, -LN2_LO, fmaf(k, -LN2_HI, x)) (the inner one is exact: LN2_HI has 9
//      significant bits, |k| < 2^7),  p = Horner chain of 7 fmaf over the Taylor coefficients 1 / i! up to i = 7,  result = ldexpf(p, k).
//      rintf, fmaf and ldexpf are exact or correctly rounded on host and device alike: the same bits on both.  exp_nonpos(0) == 1.
//      Its distance from exp is derived in tests/mpc_ref.py.
//   5. check_shape refuses M, C, H, d < 1, C > MAX_CANDIDATES, H d > MAX_ELEMENTS and products beyond 31 bits; check_sigma a non-finite sigma;
//      check_lambda a lambda that is not a positive finite number.
// No floating-point atomics, no wave waits on another, nothing depends on the grid or on timing.
// The library is built with -ffinite-math-only: isfinite() is a constant there, and so is any test of a float PARAMETER's bits (the compiler
// marks float parameters and results as never NaN or infinite and folds the test).  So a score's finiteness is read from its 32 bits as
// loaded from memory, before they are ever a float; -inf is stored as bits; and the two checks of a float argument are kept from the optimiser.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIPCC__)
#define QM_HD __host__ __device__ inline
#else
#define QM_HD inline
#endif

namespace qs {
namespace mpc {

constexpr int WAVE = 64;               // chains of a robot's weight sum
constexpr int MAX_CANDIDATES = 4096;   // per robot: the weights of one robot lie in one workgroup's LDS
constexpr int MAX_ELEMENTS = 1024;     // H d: one lane of k_mpc_finish's workgroup per element of a sequence
enum { METHOD_BEST = 0, METHOD_MPPI = 1 };

constexpr float LOG2E = 1.44269502e+00f;
constexpr float LN2_HI = 0.693359375f;          // 355 / 512
constexpr float LN2_LO = -2.12194440e-4f;       // ln 2 - LN2_HI, rounded
constexpr float EXP_CUT = -87.0f;
// 1 / i!, i = 2 .. 7, each rounded to float32 (1 / 0! and 1 / 1! are 1); tests/mpc_ref.py reads these lines
constexpr float EXP_C2 = 0.5f;
constexpr float EXP_C3 = 1.66666672e-01f;
constexpr float EXP_C4 = 4.16666679e-02f;
constexpr float EXP_C5 = 8.33333377e-03f;
constexpr float EXP_C6 = 1.38888892e-03f;
constexpr float EXP_C7 = 1.98412701e-04f;

#if defined(__clang__)
#define QM_UNOPTIMISED __attribute__((optnone, noinline))
#else
#define QM_UNOPTIMISED
#endif

constexpr uint32_t MINUS_INF_BITS = 0xff800000u;
QM_HD uint32_t load_bits(const float* p) { uint32_t b; memcpy(&b, p, sizeof(b)); return b; }
QM_HD void store_bits(float* p, uint32_t b) { memcpy(p, &b, sizeof(b)); }
QM_HD float from_bits(uint32_t b) { float x; memcpy(&x, &b, sizeof(x)); return x; }
QM_HD bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

// what qs_mpc_create takes; returns 0 or writes why not into err
inline int check_shape(int n_robots, int n_candidates, int horizon, int action_dim, char* err, size_t err_size) {
#define QM_BAD(...) do { snprintf(err, err_size, __VA_ARGS__); return -1; } while (0)
    if (n_robots < 1) QM_BAD("qs_mpc_create: n_robots = %d must be positive", n_robots);
    if (n_candidates < 1) QM_BAD("qs_mpc_create: n_candidates = %d must be positive", n_candidates);
    if (n_candidates > MAX_CANDIDATES) QM_BAD("qs_mpc_create: n_candidates = %d is above %d (a robot's weights lie in one workgroup's LDS)", n_candidates, MAX_CANDIDATES);
    if (horizon < 1) QM_BAD("qs_mpc_create: horizon = %d must be positive", horizon);
    if (action_dim < 1) QM_BAD("qs_mpc_create: action_dim = %d must be positive", action_dim);
    if ((long long)horizon * action_dim > MAX_ELEMENTS)
        QM_BAD("qs_mpc_create: horizon * action_dim = %lld is above %d (one lane per element of a sequence)", (long long)horizon * action_dim, MAX_ELEMENTS);
    const long long n_envs = (long long)n_robots * (1 + (long long)n_candidates);
    if (n_envs > 0x7fffffffLL) QM_BAD("qs_mpc_create: n_robots * (1 + n_candidates) = %lld does not fit 31 bits", n_envs);
    const long long total = (long long)n_robots * n_candidates * horizon * action_dim;     // (each factor < 2^31 and H d <= 1024: no overflow of the product)
    if (total > 0x7fffffffLL) QM_BAD("qs_mpc_create: n_robots * n_candidates * horizon * action_dim = %lld does not fit 31 bits", total);
    return 0;
}
QM_UNOPTIMISED inline int check_sigma(float sigma, char* err, size_t err_size) {
    if (!finite_bits(load_bits(&sigma))) QM_BAD("qs_mpc_sample: sigma must be finite");
    return 0;
}
QM_UNOPTIMISED inline int check_lambda(float lambda, char* err, size_t err_size) {
    const uint32_t b = load_bits(&lambda);
    // (positive and finite, read from the bits: sign clear, exponent below all-ones, not zero)
    if ((b >> 31) || !finite_bits(b) || !(b << 1)) QM_BAD("qs_mpc_finish: lambda must be a positive finite number");
    return 0;
}
#undef QM_BAD

QM_HD float clamp_unit(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }

// 1. candidate c's element
QM_HD float sample(float plan, float eps, float sigma, int c) { return c == 0 ? plan : clamp_unit(fmaf(sigma, eps, plan)); }

// 2. one candidate's accounting in feed(h >= 1); reward_end is read at h == H alone
QM_HD void account(float& score, uint8_t& running, float reward, uint8_t done, bool last, float reward_end) {
    if (running) score = score + reward;
    running = (uint8_t)(running && !done);
    if (last && running) score = score + reward_end;
}

// 4.
QM_HD float exp_nonpos(float x) {
    if (x < EXP_CUT) return 0.0f;
    const float k = rintf(x * LOG2E);
    const float r = fmaf(k, -LN2_LO, fmaf(k, -LN2_HI, x));
    float p = fmaf(EXP_C7, r, EXP_C6);
    p = fmaf(p, r, EXP_C5);
    p = fmaf(p, r, EXP_C4);
    p = fmaf(p, r, EXP_C3);
    p = fmaf(p, r, EXP_C2);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return ldexpf(p, (int)k);
}

// 3. the order of candidates: a is ahead of b.  (ok, s, c) = (the score is finite, the score, the index)
QM_HD bool ahead(bool ok_a, float s_a, int c_a, bool ok_b, float s_b, int c_b) {
    if (ok_a != ok_b) return ok_a;
    if (!ok_a) return c_a < c_b;
    return s_a > s_b || (s_a == s_b && c_a < c_b);
}
// the best of the candidates first, first + stride, ... below C: a total order, so any split of the range gives the same winner.
// (s is 0 where ok is not set: a score that is not finite never becomes a float)
QM_HD void best_of(const float* score, int C, int first, int stride, bool& ok, float& s, int& c) {
    ok = false; s = 0.0f; c = 0x7fffffff;
    for (int k = first; k < C; k += stride) {
        const uint32_t bk = load_bits(score + k);
        const bool okk = finite_bits(bk);
        const float sk = okk ? from_bits(bk) : 0.0f;
        if (ahead(okk, sk, k, ok, s, c)) { ok = okk; s = sk; c = k; }
    }
}
// candidate's weight from where its score lies; s_max is finite
QM_HD float weight(const float* score, float s_max, float lambda) {
    const uint32_t b = load_bits(score);
    return finite_bits(b) ? exp_nonpos((from_bits(b) - s_max) / lambda) : 0.0f;
}
QM_HD float lane_sum(const float* w, int C, int lane) {
    float acc = 0.0f;
    for (int c = lane; c < C; c += WAVE) acc = acc + w[c];
    return acc;
}
QM_HD float sum_lanes(const float* lane_sums) {
    float tot = 0.0f;
    for (int l = 0; l < WAVE; l++) tot = tot + lane_sums[l];
    return tot;
}
// one element of the weighted mean: seq points at candidate 0's element, candidate c's lies c * d floats on
QM_HD float mppi_element(const float* w, const float* seq, int C, int d, float Z) {
    float a = 0.0f;
    for (int c = 0; c < C; c++) a = fmaf(w[c], seq[(size_t)c * d], a);
    return clamp_unit(a / Z);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: every kernel as plain loops over its lanes
inline void sample_host(const float* plan, const float* eps, int M, int C, int H, int d, float sigma, float* seq, float* score, uint8_t* running) {
    const size_t MC = (size_t)M * C;
    for (int h = 0; h < H; h++)
        for (size_t i = 0; i < MC; i++)
            for (int j = 0; j < d; j++) {
                const size_t at = ((size_t)h * MC + i) * d + j;
                seq[at] = sample(plan[((i / C) * H + h) * d + j], eps[at], sigma, (int)(i % C));
            }
    for (size_t i = 0; i < MC; i++) { score[i] = 0.0f; running[i] = 1; }
}
// reward, done [N] (read for step >= 1), reward_end [N][stride] (read at step == H), actions [N][d] (written for step < H), active [N] or null
inline void feed_host(int step, const float* seq, float* score, uint8_t* running, int M, int C, int H, int d, const float* reward, const uint8_t* done,
                      const float* reward_end, int stride, float* actions, uint8_t* active) {
    const size_t MC = (size_t)M * C;
    for (size_t i = 0; i < MC; i++) {
        if (step >= 1) account(score[i], running[i], reward[M + i], done[M + i], step == H, step == H ? reward_end[(M + i) * stride] : 0.0f);
        if (active) active[M + i] = running[i];
    }
    if (active) for (int m = 0; m < M; m++) active[m] = 0;
    if (step < H) for (size_t t = 0; t < MC * d; t++) actions[(size_t)M * d + t] = seq[(size_t)step * MC * d + t];
}
// plan [M][H][d] and actions [N][d] are written; best [M], best_score [M]
inline void finish_host(const float* seq, const float* score, int M, int C, int H, int d, int method, float lambda, float* plan, float* actions, int* best,
                        float* best_score) {
    const size_t MC = (size_t)M * C;
    static thread_local float w[MAX_CANDIDATES];
    for (int m = 0; m < M; m++) {
        const float* sc = score + (size_t)m * C;
        bool ok; float s_max; int b;
        best_of(sc, C, 0, 1, ok, s_max, b);
        if (!ok) b = 0;
        best[m] = b;
        if (ok) best_score[m] = s_max; else store_bits(best_score + m, MINUS_INF_BITS);
        float Z = 0.0f;
        if (method == METHOD_MPPI && ok) {
            for (int c = 0; c < C; c++) w[c] = weight(sc + c, s_max, lambda);
            float lanes[WAVE];
            for (int l = 0; l < WAVE; l++) lanes[l] = lane_sum(w, C, l);
            Z = sum_lanes(lanes);
        }
        for (int h = 0; h < H; h++)
            for (int j = 0; j < d; j++) {
                const float* e = seq + ((size_t)h * MC + (size_t)m * C) * d + j;
                const float v = (method == METHOD_MPPI && ok) ? mppi_element(w, e, C, d, Z) : e[(size_t)b * d];
                if (h == 0) actions[(size_t)m * d + j] = v;
                if (h >= 1) plan[((size_t)m * H + h - 1) * d + j] = v;
                if (h == H - 1) plan[((size_t)m * H + h) * d + j] = v;
            }
    }
}
// rows of robots with mask[m] (null: all) = src's (null: zeros)
inline void set_plan_host(float* plan, const float* src, const uint8_t* mask, int M, int H, int d) {
    for (int m = 0; m < M; m++)
        if (!mask || mask[m])
            for (int e = 0; e < H * d; e++) plan[(size_t)m * H * d + e] = src ? src[(size_t)m * H * d + e] : 0.0f;
}
#endif

}  // namespace mpc
}  // namespace qs
