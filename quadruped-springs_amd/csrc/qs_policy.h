// qs_policy.h -- the arithmetic of a policy network's forward pass (model.predict of load_model.py:132; SB3 BasePolicy.predict for a PPO
// MlpPolicy, sb3_contrib's ARS policies), shared by k_policy (qs_policy.hip) and its TEST-ONLY host build (tests/emu/qs_emu_policy.cpp).
//
// Numerical contract: float32, and every pre-activation is ONE chain of fused multiply-adds in ascending k that starts from the bias
// (or from 0):   acc = b;  acc = fmaf(W[o][k], h[k], acc)  for k = 0, 1, ..., in - 1,   then zero products up to the next multiple of 4
// (they leave acc as it is; a chain that arrives at -0 leaves as +0).  v_mfma_f32_16x16x4_f32 computes exactly that chain, four k per
// instruction, so the kernel's tiles, this header's host loop and a lane-per-environment VALU build give the same bits, and an
// environment's result never depends on which environments share its wave.  tanhf / expf are the platform's: those differ in the last
// bits between the device and the host (tests bound them instead of comparing bits).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/qs_amd.h"

#if defined(__HIPCC__)
#define QP_HD __host__ __device__ inline
#else
#define QP_HD inline
#endif

namespace qs {
namespace pol {

constexpr int MAX_OBS = 64, MAX_WIDTH = 256, MAX_LAYERS = QS_POLICY_MAX_HIDDEN + 1;
constexpr int TILE = 16;                       // environments of one MFMA tile
constexpr int W_LDS_FLOATS = 12288;            // at most 48 KB of a layer's weights in LDS at a time (wider layers: k-chunks)
constexpr size_t LDS_MAX_BYTES = 160 * 1024;   // of a gfx950 compute unit

// the layers of one policy and where they lie in its parameter row (torch.nn.utils.parameters_to_vector order: per layer weight
// [out][in] row-major, then bias [out])
struct Net {
    int n_layers, obs_dim, action_dim, n_params, activation, squash, has_bias;
    int in[MAX_LAYERS], out[MAX_LAYERS], w_off[MAX_LAYERS], b_off[MAX_LAYERS];
    float lo, hi;
};

QP_HD int round_up(int x, int m) { return (x + m - 1) / m * m; }
// a layer's k-major LDS image [k][out_pad]: the four k of an MFMA step must fall into four different quarters of the 64 banks
QP_HD int out_pad(int out) { const int op = round_up(out, TILE); return op % 32 == 16 ? op : op + 16; }

// The sizes of a launch's LDS layout (k_policy, qs_policy.hip; k_actor_critic, qs_ppo.hip), as the host fixes them for the networks that pass
// through one weight image:
// act_stride = floats of a wave's row [env][k], w_floats = floats of the weight image, wide = some layer needs more than 4 tiles.
inline void layout_sizes(const Net* const* nets, int n_nets, int& act_stride, int& w_floats, int& wide) {
    int widest = 0, w_need = 0;
    wide = 0;
    for (int i = 0; i < n_nets; i++) {
        const Net& net = *nets[i];
        if (round_up(net.obs_dim, 4) > widest) widest = round_up(net.obs_dim, 4);
        for (int l = 0; l < net.n_layers; l++) {
            const int nt = (net.out[l] + TILE - 1) / TILE, need = out_pad(net.out[l]) * round_up(net.in[l], 4);
            if (nt * TILE > widest) widest = nt * TILE;
            if (need > w_need) w_need = need;
            if (nt > 4) wide = 1;
        }
    }
    act_stride = round_up(widest, 64) + 4;        // (stride % 64 == 4: the 16 environments x 4 k of an MFMA step cover the 64 banks once)
    w_floats = w_need < W_LDS_FLOATS ? round_up(w_need, 4) : W_LDS_FLOATS;
}
// row_sets: sets of rows [16][act_stride] per wave (k_policy: 1, the activations; k_actor_critic: 2, the observations as well)
inline size_t lds_bytes(int w_floats, int waves, int row_sets, int act_stride) {
    return ((size_t)w_floats + (size_t)waves * row_sets * TILE * act_stride) * sizeof(float);
}
// waves of a workgroup: as many as share a weight image (the tiles of one group: a policy's block), fewer while that leaves compute units
// without a workgroup or the compute unit's LDS too small
inline int waves_per_workgroup(int tiles_per_group, int groups, int w_floats, int row_sets, int act_stride) {
    int waves = 4;
    while (waves > 1 && (waves / 2 >= tiles_per_group || (long long)groups * ((tiles_per_group + waves - 1) / waves) < 256 ||
                         lds_bytes(w_floats, waves, row_sets, act_stride) > LDS_MAX_BYTES))
        waves /= 2;
    return waves;
}

// fills `net`; returns 0 or writes why not into err
inline int net_from_desc(const qs_policy_desc& d, Net& net, char* err, size_t err_size) {
#define QP_BAD(...) do { snprintf(err, err_size, __VA_ARGS__); return -1; } while (0)
    if (d.n_envs <= 0) QP_BAD("qs_policy_desc: n_envs = %d must be positive", d.n_envs);
    if (d.n_policies <= 0 || d.n_envs % d.n_policies != 0) QP_BAD("qs_policy_desc: n_policies = %d must be positive and divide n_envs = %d", d.n_policies, d.n_envs);
    if (d.obs_dim <= 0 || d.obs_dim > MAX_OBS) QP_BAD("qs_policy_desc: obs_dim = %d outside [1, %d]", d.obs_dim, MAX_OBS);
    if (d.action_dim <= 0 || d.action_dim > MAX_WIDTH) QP_BAD("qs_policy_desc: action_dim = %d outside [1, %d]", d.action_dim, MAX_WIDTH);
    if (d.n_hidden < 0 || d.n_hidden > QS_POLICY_MAX_HIDDEN) QP_BAD("qs_policy_desc: n_hidden = %d outside [0, %d]", d.n_hidden, QS_POLICY_MAX_HIDDEN);
    for (int l = 0; l < d.n_hidden; l++)
        if (d.hidden[l] <= 0 || d.hidden[l] > MAX_WIDTH) QP_BAD("qs_policy_desc: hidden[%d] = %d outside [1, %d]", l, d.hidden[l], MAX_WIDTH);
    if (d.activation < QS_POLICY_ACT_NONE || d.activation > QS_POLICY_ACT_RELU) QP_BAD("qs_policy_desc: activation = %d is none of QS_POLICY_ACT_*", d.activation);
    if (!(d.clip_lo <= d.clip_hi)) QP_BAD("qs_policy_desc: clip_lo = %g above clip_hi = %g", (double)d.clip_lo, (double)d.clip_hi);
#undef QP_BAD
    net.n_layers = d.n_hidden + 1; net.obs_dim = d.obs_dim; net.action_dim = d.action_dim;
    net.activation = d.activation; net.squash = d.squash_output ? 1 : 0; net.has_bias = d.has_bias ? 1 : 0;
    net.lo = d.clip_lo; net.hi = d.clip_hi;
    int off = 0, in = d.obs_dim;
    for (int l = 0; l < MAX_LAYERS; l++) { net.in[l] = net.out[l] = net.w_off[l] = net.b_off[l] = 0; }
    for (int l = 0; l < net.n_layers; l++) {
        const int out = l < d.n_hidden ? d.hidden[l] : d.action_dim;
        net.in[l] = in; net.out[l] = out;
        net.w_off[l] = off; off += out * in;
        net.b_off[l] = off; if (net.has_bias) off += out;
        in = out;
    }
    net.n_params = off;
    return 0;
}

QP_HD float activate(float x, int kind) {
    if (kind == QS_POLICY_ACT_TANH) return tanhf(x);
    if (kind == QS_POLICY_ACT_RELU) return fmaxf(x, 0.0f);
    return x;
}
// DiagGaussianDistribution: a = mean + exp(log_std) * eps
QP_HD float gauss_action(float mean, float log_std, float eps) { return fmaf(expf(log_std), eps, mean); }
// one dimension of Normal(mean, exp(log_std)).log_prob(mean + exp(log_std) * eps) = -eps^2 / 2 - log_std - log(2 pi) / 2
QP_HD float log_prob_term(float eps, float log_std) { return fmaf(-0.5f * eps, eps, -log_std) - 0.918938533204672742f; }
QP_HD float clampf(float a, float lo, float hi) { return fminf(fmaxf(a, lo), hi); }

// What one environment's row of outputs is once the last layer's values `mean` [action_dim] are known (the kernel runs this with the
// dimensions spread over four lanes; log_prob is summed in ascending j by one of them).
QP_HD void epilogue_elem(const Net& net, float mean, const float* eps_row, const float* log_std, int j, float* act_row, float* mean_row) {
    const float a = eps_row ? gauss_action(mean, log_std[j], eps_row[j]) : mean;
    act_row[j] = clampf(a, net.lo, net.hi);
    if (mean_row) mean_row[j] = mean;
}
QP_HD float log_prob_row(const Net& net, const float* eps_row, const float* log_std) {
    float lp = 0.0f;
    for (int j = 0; j < net.action_dim; j++) lp += log_prob_term(eps_row[j], log_std[j]);
    return lp;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The chain of one output, as the header's first comment states it.
inline float dot_chain(const float* w_row, float bias, const float* h, int in) {
    float acc = bias;
    for (int k = 0; k < in; k++) acc = fmaf(w_row[k], h[k], acc);
    for (int k = in; k < round_up(in, 4); k++) acc = fmaf(0.0f, 0.0f, acc);
    return acc;
}
// One environment on the host: params = its policy's row [n_params]; eps / log_std / mean_row / log_prob may be null.
inline void forward_env(const Net& net, const float* params, const float* obs, const float* eps_row, const float* log_std, float* act_row,
                        float* mean_row, float* log_prob) {
    float h[2][MAX_WIDTH];
    for (int k = 0; k < net.obs_dim; k++) h[0][k] = obs[k];
    int cur = 0;
    for (int l = 0; l < net.n_layers; l++) {
        const bool last = l == net.n_layers - 1;
        const int kind = last ? (net.squash ? (int)QS_POLICY_ACT_TANH : (int)QS_POLICY_ACT_NONE) : net.activation;
        for (int o = 0; o < net.out[l]; o++)
            h[cur ^ 1][o] = activate(dot_chain(params + net.w_off[l] + (size_t)o * net.in[l], net.has_bias ? params[net.b_off[l] + o] : 0.0f, h[cur], net.in[l]), kind);
        cur ^= 1;
    }
    for (int j = 0; j < net.action_dim; j++) epilogue_elem(net, h[cur][j], eps_row, log_std, j, act_row, mean_row);
    if (log_prob) *log_prob = log_prob_row(net, eps_row, log_std);
}
#endif

}  // namespace pol
}  // namespace qs
