// qs_ppo_train.h -- the arithmetic of one minibatch of SB3's PPO.train (evaluate_actions, the clipped loss, loss.backward, clip_grad_norm_,
// Adam.step), shared by k_adv_moments / k_ppo_grad / k_ppo_reduce / k_ppo_adam (qs_ppo_train.hip) and their TEST-ONLY host build
// (tests/emu/qs_emu_ppo_train.cpp, tests/sanitize/drv_ppo_train.cpp).
//
// Numerical contract: float32 (one accumulator of the statistics excepted, below).  A minibatch is B samples taken BY INDEX from the flat rollout arrays [total, ...]; sample s is
// row indices[s].  An index outside [0, total) is never read: its sample is a MASKED row (zero activations, zero delta, no statistics),
// it is counted as refused, and B stays the divisor.
//   Forward: qs_policy.h's chain, unchanged (one fmaf chain per pre-activation in ascending k from the bias):
//       mean = actor(obs),  value = critic(obs)[0]
//       z_j = (action_j - mean_j) * inv_std_j,  inv_std_j = expf(-log_std_j)
//       log_prob = sum_j log_prob_term(z_j, log_std_j) = sum_j (fmaf(-0.5 z_j, z_j, -log_std_j) - log(2 pi) / 2)     ascending j from 0
//   Advantage normalisation (skipped when B == 1 or normalize_advantage is off), in a pass of its own (adv_moments):
//       A = (adv - mean_B) / (std_B + 1e-8f),   std_B = sqrtf(sum (adv - mean_B)^2 / (B - 1)),  mean_B = sum adv / B
//       each sum: chain c of MOM_CHAINS takes the samples c, c + MOM_CHAINS, ... in ascending order (plain adds for the mean,
//       fmaf(d, d, acc) for the squares); 16 consecutive chains are added in ascending order, then those 64 sums in ascending order.
//   Ratio, loss terms and the loss gradient of a sample (policy_terms, value_grad), fB = (float)B:
//       lr = log_prob - old_log_prob,  r = expf(lr),  u1 = A r,  u2 = A clamp(r, 1 - c, 1 + c)
//       policy term = -fminf(u1, u2);  kl term = (r - 1) - lr;  clipped = fabsf(r - 1) > c;  value term = (return - value)^2
//       dlp = d loss / d log_prob = (u1 <= u2) ? -u1 / fB : 0
//           The tie rule is torch's: min's backward gives each side half at u1 == u2, clamp's backward passes inside [1 - c, 1 + c],
//           edges included.  Inside, r == clamp(r) so u1 == u2 and the halves add up to the whole; outside, u1 == u2 only for A == 0, where
//           the half is 0 as well: `u1 <= u2` is torch's gradient for every finite input.
//       d loss / d mean_j = (dlp * z_j) * inv_std_j;     log_std term of the sample = dlp * fmaf(z_j, z_j, -1)
//       d loss / d value  = ((2 vf_coef) * (value - return)) / fB
//   Backward through the layers, per sample (delta_top as above; h_l the stored post-activations, h_-1 = obs):
//       dW_l[o][i] = fmaf(delta_l[o], h_(l-1)[i], dW_l[o][i]);   db_l[o] += delta_l[o]
//       delta_(l-1)[i] = chain(o ascending from 0: fmaf(W_l[o][i], delta_l[o], acc)) * act'(h_(l-1)[i])
//       act' = fmaf(-h, h, 1) for tanh, (h > 0) for relu, 1 for none
//   Summation order: a pure function of B and the constants below, never of the device, the grid or timing; no floating-point atomics.
//       Sample s belongs to tile s / 16; tile t belongs to part t % PARTS; a part goes through its tiles in ascending order and
//       through a tile's samples in ascending order, every sum starting from 0: weights by the fmaf above (one chain over all of the
//       part's samples, which is what v_mfma_f32_16x16x4_f32 computes four samples at a time), biases, log_std terms and statistics by
//       plain adds.  Then the parts 0 .. min(PARTS, tiles) - 1 are added in ascending order, starting from 0 (reduce_parts).
//       d loss / d log_std_j = (sum of the samples' terms) - ent_coef.
//   Statistics (SB3's names; finish_stats).  A part's sums are float32; the parts' sums of a statistic are added in ascending order in ONE
//       float64 accumulator and rounded to float32 once (a thousand float32 additions of like-signed terms would cost the value loss ten
//       unit roundoffs; the gradient's sums have both signs and stay float32).  policy_loss = sum / fB, value_loss = sum / fB, approx_kl = sum / fB, clip_fraction = count / fB,
//       entropy_loss = -sum_j (log_std_j + (0.5 + 0.5 log 2 pi))  ascending j (the same for every sample),
//       loss = fmaf(vf_coef, value_loss, fmaf(ent_coef, entropy_loss, policy_loss)).
//   Gradient norm over actor, critic and log_std together (the flat gradient [n_actor | n_critic | action_dim]): blocks of NORM_BLOCK
//       consecutive entries, each fmaf(g, g, acc) in ascending order from 0; the blocks' sums added in ascending order; sqrtf.
//   Clip and Adam (torch's clip_grad_norm_ and Adam without weight decay or amsgrad; adam_consts, adam_elem), step t = 1, 2, ...:
//       coef = fminf(1, max_grad_norm / (norm + 1e-6f));   gc = g * coef
//       m = fmaf(b1, m, (1 - b1) * gc);   v = fmaf(b2, v, ((1 - b2) * gc) * gc)
//       p = p - (step_size * m) / (sqrtf(v) / bc2_sqrt + eps)
//       b1, 1 - b1, b2, 1 - b2, eps, step_size = lr / (1 - b1^t) and bc2_sqrt = sqrt(1 - b2^t) are computed in double (as torch computes
//       them in Python) and rounded to float32 once.
// expf / tanhf / sqrtf are the platform's: the device and the host differ in the last bits (tests bound them, tests/ppo_train_ref.py).
#pragma once
#include "qs_ppo.h"
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace qs {
namespace train {

using pol::Net;
using pol::TILE;

constexpr int PARTS = 1024;          // parts a minibatch's tiles are dealt to (a wave of k_ppo_grad is a part)
constexpr int MOM_CHAINS = 1024;     // chains of the advantage moments (a lane of k_adv_moments is a chain)
constexpr int NORM_BLOCK = 256;      // entries of the flat gradient per partial sum of squares
constexpr int MAX_WIDTH = 64, MAX_HIDDEN = 2, MAX_LAYERS = MAX_HIDDEN + 1;
constexpr int S = 68;                // floats of a wave's LDS row [sample][k] (S % 64 == 4, as qs_policy.h's act_stride)
constexpr int ROW_SETS = 5;          // observations, two hidden layers, the output / its delta, the epilogue's terms
enum { PS_POLICY = 0, PS_KL = 1, PS_CLIP = 2, PS_VALUE = 3, PS_REFUSED = 4, PART_STATS_USED = 5, PART_STATS = 8 };   // a part's statistics, after its gradient
constexpr float ENTROPY_CONST = 1.4189385332046727f;   // 0.5 + 0.5 log(2 pi)

QP_HD int tiles_of(int B) { return (B + TILE - 1) / TILE; }
QP_HD int parts_used(int B) { const int t = tiles_of(B); return t < PARTS ? t : PARTS; }
QP_HD int total_params(const Net& a, const Net& c) { return a.n_params + c.n_params + a.action_dim; }
QP_HD int part_stride(int n_total) { return pol::round_up(n_total, 4) + PART_STATS; }
QP_HD int norm_blocks(int n_total) { return (n_total + NORM_BLOCK - 1) / NORM_BLOCK; }

// One network's weights in LDS: per layer the k-major image [k][out_pad(out)] the forward pass reads (qs_policy.h's), and for every layer
// but the first the row-major image [o][out_pad(in)] the backward product delta W reads (the four o of an MFMA step in four bank quarters).
struct Image { int fw_off[MAX_LAYERS], rw_off[MAX_LAYERS], floats; };
inline Image image_of(const Net& net) {
    Image im;
    int off = 0;
    for (int l = 0; l < MAX_LAYERS; l++) im.fw_off[l] = im.rw_off[l] = 0;
    for (int l = 0; l < net.n_layers; l++) { im.fw_off[l] = off; off += pol::round_up(net.in[l], 4) * pol::out_pad(net.out[l]); }
    for (int l = 1; l < net.n_layers; l++) { im.rw_off[l] = off; off += pol::round_up(net.out[l], 4) * pol::out_pad(net.in[l]); }
    im.floats = pol::round_up(off, 4);
    return im;
}
inline size_t lds_bytes(int image_floats, int waves) { return ((size_t)image_floats + (size_t)waves * ROW_SETS * TILE * S) * sizeof(float); }
// waves of a workgroup of k_ppo_grad: 4, fewer while the compute unit's LDS is too small; 0 = even one wave does not fit
inline int waves_of(int image_floats) {
    int waves = 4;
    while (waves > 0 && lds_bytes(image_floats, waves) > pol::LDS_MAX_BYTES) waves /= 2;
    return waves;
}

// what the update supports of what qs_ac_create takes; fills the nets; returns 0 or writes why not into err
inline int check_train(const qs_policy_desc& a, const qs_policy_desc& c, Net& na, Net& nc, char* err, size_t err_size) {
#define QT_BAD(...) do { snprintf(err, err_size, __VA_ARGS__); return -1; } while (0)
    if (pol::net_from_desc(a, na, err, err_size) || pol::net_from_desc(c, nc, err, err_size) || ppo::check_pair(a, c, err, err_size)) return -1;
    const qs_policy_desc* both[2] = {&a, &c};
    for (int n = 0; n < 2; n++) {
        const qs_policy_desc& d = *both[n];
        const char* who = n ? "critic" : "actor";
        if (d.n_hidden > MAX_HIDDEN) QT_BAD("qs_ppo_create: the %s has %d hidden layers, the device update takes at most %d", who, d.n_hidden, MAX_HIDDEN);
        for (int l = 0; l < d.n_hidden; l++)
            if (d.hidden[l] > MAX_WIDTH) QT_BAD("qs_ppo_create: the %s's hidden[%d] = %d is wider than %d (a layer's weight-gradient tiles stay in registers)", who, l, d.hidden[l], MAX_WIDTH);
        if (d.action_dim > MAX_WIDTH) QT_BAD("qs_ppo_create: the %s's action_dim = %d is above %d", who, d.action_dim, MAX_WIDTH);
        if (!d.has_bias) QT_BAD("qs_ppo_create: the %s has no biases (SB3's MlpPolicy has them on every layer)", who);
        if (d.squash_output) QT_BAD("qs_ppo_create: the %s has squash_output set: the update is the diagonal Gaussian's", who);
    }
#undef QT_BAD
    return 0;
}

QP_HD float adv_norm(float adv, float mean, float std, int on) { return on ? (adv - mean) / (std + 1e-8f) : adv; }
QP_HD float z_of(float action, float mean, float inv_std) { return (action - mean) * inv_std; }
struct PolTerms { float dlp, pol, kl, clip, on; };   // on: 1 where the unclipped branch carries the gradient
QP_HD PolTerms policy_terms(float log_prob, float old_log_prob, float A, float c, float fB) {
    const float lr = log_prob - old_log_prob, r = expf(lr);
    const float u1 = A * r, u2 = A * pol::clampf(r, 1.0f - c, 1.0f + c);
    PolTerms t;
    t.on = u1 <= u2 ? 1.0f : 0.0f;
    t.dlp = u1 <= u2 ? -u1 / fB : 0.0f;
    t.pol = -fminf(u1, u2);
    t.kl = (r - 1.0f) - lr;
    t.clip = fabsf(r - 1.0f) > c ? 1.0f : 0.0f;
    return t;
}
QP_HD float mean_grad(float dlp, float z, float inv_std) { const float t = dlp * z; return t * inv_std; }
QP_HD float log_std_term(float dlp, float z) { return dlp * fmaf(z, z, -1.0f); }
QP_HD float value_grad(float value, float ret, float vf_coef, float fB) { const float d = value - ret; return ((2.0f * vf_coef) * d) / fB; }
QP_HD float value_term(float value, float ret) { const float d = ret - value; return d * d; }
QP_HD float dact(float h, int kind) {
    if (kind == QS_POLICY_ACT_TANH) return fmaf(-h, h, 1.0f);
    if (kind == QS_POLICY_ACT_RELU) return h > 0.0f ? 1.0f : 0.0f;
    return 1.0f;
}
QP_HD float entropy_of(const float* log_std, int A) {
    float e = 0.0f;
    for (int j = 0; j < A; j++) e += log_std[j] + ENTROPY_CONST;
    return e;
}
// sums[PART_STATS] (the parts added up) -> stats[QS_PPO_N_STATS]; grad_norm is the Adam call's
QP_HD void finish_stats(const float* sums, float entropy, float ent_coef, float vf_coef, int B, float* stats) {
    const float fB = (float)B;
    stats[QS_PPO_STAT_POLICY_LOSS] = sums[PS_POLICY] / fB;
    stats[QS_PPO_STAT_VALUE_LOSS] = sums[PS_VALUE] / fB;
    stats[QS_PPO_STAT_ENTROPY_LOSS] = -entropy;
    stats[QS_PPO_STAT_APPROX_KL] = sums[PS_KL] / fB;
    stats[QS_PPO_STAT_CLIP_FRACTION] = sums[PS_CLIP] / fB;
    stats[QS_PPO_STAT_GRAD_NORM] = 0.0f;
    stats[QS_PPO_STAT_REFUSED] = sums[PS_REFUSED];
    stats[QS_PPO_STAT_LOSS] = fmaf(vf_coef, stats[QS_PPO_STAT_VALUE_LOSS], fmaf(ent_coef, -entropy, stats[QS_PPO_STAT_POLICY_LOSS]));
}

struct AdamConsts { float b1, omb1, b2, omb2, eps, step_size, bc2_sqrt, max_norm; };
inline AdamConsts adam_consts(const qs_ppo_hyper& hy, int step) {
    AdamConsts k;
    k.b1 = (float)hy.beta_one; k.omb1 = (float)(1.0 - hy.beta_one); k.b2 = (float)hy.beta_two; k.omb2 = (float)(1.0 - hy.beta_two);
    k.eps = (float)hy.adam_eps;
    k.step_size = (float)(hy.lr / (1.0 - pow(hy.beta_one, (double)step)));
    k.bc2_sqrt = (float)sqrt(1.0 - pow(hy.beta_two, (double)step));
    k.max_norm = hy.max_grad_norm;
    return k;
}
QP_HD float clip_coef(float norm, float max_norm) { return fminf(1.0f, max_norm / (norm + 1e-6f)); }
QP_HD void adam_elem(float g, float coef, const AdamConsts& k, float& p, float& m, float& v) {
    const float gc = g * coef;
    m = fmaf(k.b1, m, k.omb1 * gc);
    v = fmaf(k.b2, v, (k.omb2 * gc) * gc);
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    const float q = (k.step_size * m) / denom;
    p = p - q;
}

#if !defined(__HIP_DEVICE_COMPILE__)
inline bool index_ok(long long i, long long total) { return i >= 0 && i < total; }

// mean and unbiased std of the indexed advantages in the stated order; masked samples add nothing
inline void adv_moments_host(const float* adv, long long total, const long long* idx, int B, float* mean_out, float* std_out) {
    float mean = 0.0f, sd = 0.0f;
    for (int pass = 0; pass < 2; pass++) {
        float groups[MOM_CHAINS / 16];
        for (int gr = 0; gr < MOM_CHAINS / 16; gr++) {
            float gs = 0.0f;
            for (int c = 16 * gr; c < 16 * gr + 16; c++) {
                float acc = 0.0f;
                for (int s = c; s < B; s += MOM_CHAINS) {
                    if (!index_ok(idx[s], total)) continue;
                    const float a = adv[idx[s]];
                    if (pass == 0) acc += a;
                    else { const float d = a - mean; acc = fmaf(d, d, acc); }
                }
                gs += acc;
            }
            groups[gr] = gs;
        }
        float tot = 0.0f;
        for (int gr = 0; gr < MOM_CHAINS / 16; gr++) tot += groups[gr];
        if (pass == 0) mean = tot / (float)B;
        else sd = B > 1 ? sqrtf(tot / (float)(B - 1)) : 0.0f;
    }
    *mean_out = mean; *std_out = sd;
}

// forward of one sample with every layer's post-activation kept: h[0] = obs, h[l + 1] = layer l's output
inline void forward_keep(const Net& net, const float* par, const float* obs, float h[MAX_LAYERS + 1][MAX_WIDTH]) {
    for (int k = 0; k < net.obs_dim; k++) h[0][k] = obs[k];
    for (int l = 0; l < net.n_layers; l++) {
        const int kind = l == net.n_layers - 1 ? (int)QS_POLICY_ACT_NONE : net.activation;
        for (int o = 0; o < net.out[l]; o++)
            h[l + 1][o] = pol::activate(pol::dot_chain(par + net.w_off[l] + (size_t)o * net.in[l], par[net.b_off[l] + o], h[l], net.in[l]), kind);
    }
}
// backward of one sample into a part's row `acc` [n_params]: delta = d loss / d (the last layer's output)
inline void backward_sample(const Net& net, const float* par, const float h[MAX_LAYERS + 1][MAX_WIDTH], const float* delta_top, float* acc) {
    float d[MAX_WIDTH], dp[MAX_WIDTH];
    for (int o = 0; o < net.out[net.n_layers - 1]; o++) d[o] = delta_top[o];
    for (int l = net.n_layers - 1; l >= 0; l--) {
        const int in = net.in[l], out = net.out[l];
        for (int o = 0; o < out; o++) {
            float* row = acc + net.w_off[l] + (size_t)o * in;
            for (int i = 0; i < in; i++) row[i] = fmaf(d[o], h[l][i], row[i]);
            acc[net.b_off[l] + o] += d[o];
        }
        if (l == 0) break;
        const float* W = par + net.w_off[l];
        for (int i = 0; i < in; i++) {
            float a = 0.0f;
            for (int o = 0; o < out; o++) a = fmaf(W[(size_t)o * in + i], d[o], a);
            dp[i] = a * dact(h[l][i], net.activation);
        }
        for (int i = 0; i < in; i++) d[i] = dp[i];
    }
}

// One minibatch gradient with its statistics: grad [n_actor + n_critic + A], stats [QS_PPO_N_STATS]; returns the refused samples.
// flags [B] (tests): per sample, bit 0 = the unclipped branch carried the gradient (u1 <= u2), bit 1 = counted as clipped.
inline int grad_host(const Net& na, const Net& nc, const float* pa, const float* pc, const float* log_std, const float* obs, const float* actions,
                     const float* old_log_prob, const float* adv, const float* returns, long long total, const long long* idx, int B,
                     const qs_ppo_hyper& hy, float* grad, float* stats, unsigned char* flags = nullptr) {
    const int A = na.action_dim, n_total = total_params(na, nc), off_c = na.n_params, off_ls = na.n_params + nc.n_params;
    const int norm_on = hy.normalize_advantage && B > 1;
    const float fB = (float)B;
    float mean_b = 0.0f, std_b = 0.0f;
    if (norm_on) adv_moments_host(adv, total, idx, B, &mean_b, &std_b);
    float inv_std[MAX_WIDTH];
    for (int j = 0; j < A; j++) inv_std[j] = expf(-log_std[j]);
    std::vector<float> part((size_t)n_total + PART_STATS);
    double sums64[PART_STATS];
    float sums[PART_STATS];
    for (int i = 0; i < n_total; i++) grad[i] = 0.0f;
    for (int i = 0; i < PART_STATS; i++) sums64[i] = 0.0;
    const int n_tiles = tiles_of(B), used = parts_used(B);
    for (int p = 0; p < used; p++) {
        for (size_t i = 0; i < part.size(); i++) part[i] = 0.0f;
        float* st = part.data() + n_total;
        for (int tile = p; tile < n_tiles; tile += PARTS) {
            for (int s = tile * TILE; s < tile * TILE + TILE && s < B; s++) {
                const long long at = idx[s];
                if (!index_ok(at, total)) { st[PS_REFUSED] += 1.0f; if (flags) flags[s] = 0; continue; }
                float h[MAX_LAYERS + 1][MAX_WIDTH], delta[MAX_WIDTH], z[MAX_WIDTH];
                // the actor
                forward_keep(na, pa, obs + (size_t)at * na.obs_dim, h);
                const float* mean = h[na.n_layers];
                float lp = 0.0f;
                for (int j = 0; j < A; j++) { z[j] = z_of(actions[(size_t)at * A + j], mean[j], inv_std[j]); lp += pol::log_prob_term(z[j], log_std[j]); }
                const PolTerms t = policy_terms(lp, old_log_prob[at], adv_norm(adv[at], mean_b, std_b, norm_on), hy.clip_range, fB);
                if (flags) flags[s] = (unsigned char)((t.on != 0.0f ? 1 : 0) | (t.clip != 0.0f ? 2 : 0));
                for (int j = 0; j < A; j++) { delta[j] = mean_grad(t.dlp, z[j], inv_std[j]); part[off_ls + j] += log_std_term(t.dlp, z[j]); }
                backward_sample(na, pa, h, delta, part.data());
                st[PS_POLICY] += t.pol; st[PS_KL] += t.kl; st[PS_CLIP] += t.clip;
                // the critic
                forward_keep(nc, pc, obs + (size_t)at * nc.obs_dim, h);
                const float value = h[nc.n_layers][0];
                delta[0] = value_grad(value, returns[at], hy.vf_coef, fB);
                backward_sample(nc, pc, h, delta, part.data() + off_c);
                st[PS_VALUE] += value_term(value, returns[at]);
            }
        }
        for (int i = 0; i < n_total; i++) grad[i] += part[i];      // reduce_parts: ascending parts, from 0
        for (int i = 0; i < PART_STATS; i++) sums64[i] += (double)st[i];
    }
    for (int i = 0; i < PART_STATS; i++) sums[i] = (float)sums64[i];
    for (int j = 0; j < A; j++) grad[off_ls + j] -= hy.ent_coef;
    finish_stats(sums, entropy_of(log_std, A), hy.ent_coef, hy.vf_coef, B, stats);
    return (int)sums[PS_REFUSED];
}

inline float grad_norm_host(const float* grad, int n_total) {
    float tot = 0.0f;
    for (int b = 0; b < norm_blocks(n_total); b++) {
        float acc = 0.0f;
        for (int i = b * NORM_BLOCK; i < (b + 1) * NORM_BLOCK && i < n_total; i++) acc = fmaf(grad[i], grad[i], acc);
        tot += acc;
    }
    return sqrtf(tot);
}
// clip_grad_norm_ and Adam.step on the flat arrays [n] (parameters, moments, gradient); returns the norm before clipping
inline float adam_host(float* p, float* m, float* v, const float* grad, int n, const qs_ppo_hyper& hy, int step) {
    const float norm = grad_norm_host(grad, n);
    const AdamConsts k = adam_consts(hy, step);
    const float coef = clip_coef(norm, k.max_norm);
    for (int i = 0; i < n; i++) adam_elem(grad[i], coef, k, p[i], m[i], v[i]);
    return norm;
}
#endif

}  // namespace train
}  // namespace qs
