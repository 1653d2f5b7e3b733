// qs_ppo_train.hip -- k_adv_moments, k_ppo_grad, k_ppo_reduce, k_ppo_adam and the C ABI of the PPO update on the device (qs_ppo_*;
// include/qs_amd.h): one minibatch of SB3's PPO.train -- evaluate_actions, the clipped loss, loss.backward, clip_grad_norm_, Adam.step --
// without a gather, autograd or a host round trip.  The arithmetic and its summation order are csrc/qs_ppo_train.h.
//
// k_ppo_grad: a wave is a PART (qs_ppo_train.h): it goes through the part's tiles of 16 samples, first all of them for the actor, then all
// of them for the critic, and keeps the network's weight-gradient tiles in registers the whole time (one v_mfma_f32_16x16x4_f32 accumulator
// per 16 outputs x 16 inputs of every layer).  A workgroup is 4 (2, 1) waves that share the network's weights in LDS, staged ONCE per
// network in two images: k-major for the forward pass (k_policy's), row-major for the backward product.  Per tile the wave
//   gathers the 16 rows by index into its LDS rows [sample][k] (an index out of range, or a row past B: zeros, every layer masked to 0),
//   runs the forward as k_policy does and keeps every layer's activations in its rows,
//   turns the last layer's rows into d loss / d output in place (the loss epilogue),
//   and walks back: dW_l += delta_l^T h_(l-1) is an MFMA with k = sample (A = delta's rows, B = h's rows, four samples per instruction, so
//   the accumulator is ONE fmaf chain over the part's samples in ascending order); delta_(l-1) = (delta_l W_l) . act'(h_(l-1)) is an MFMA
//   with k = output index over the row-major image, written over h_(l-1) in place once dW_l has read it.
// Biases, log_std terms and statistics are summed by the lanes over the tile's rows in ascending order.  A part's sums go to its row of the
// handle's [PARTS][stride] buffer; k_ppo_reduce adds the rows in ascending order.  Nothing is atomic, nothing depends on the grid.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "qs_ppo_train.h"
#include "qs_host.h"

using namespace qs::pol;
namespace tr = qs::train;

namespace {
struct GradArgs {
    const float* obs; const float* actions; const float* old_log_prob; const float* adv; const float* returns;
    const float* actor_params; const float* critic_params; const float* log_std;
    const long long* idx;
    const float* moments;         // [2]: mean and std of the indexed advantages (read when norm_on)
    float* parts;                 // [PARTS][stride]
    long long total;
    int B, stride, image_floats, norm_on;
    float clip_range, vf_coef;
    tr::Image ia, ic;
};
}  // namespace

struct qs_ppo {
    Net actor, critic;
    tr::Image ia, ic;
    int device, max_batch, n_total, stride, waves, image_floats;
    size_t lds_bytes;
    hipStream_t stream;
    float* pa; float* pc; float* log_std; float* m; float* v;   // the caller's arrays (kept, not copied)
    float* parts; float* moments; float* sumsq;                 // owned: [PARTS][stride], [2], [norm_blocks]
    unsigned long long* refused;                                // owned device counter
};

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int S = tr::S, ML = tr::MAX_LAYERS, NT = 4;   // NT: tiles of 16 across a width of at most 64
// a wave's LDS rows are written by some of its lanes and read by others: LDS serves one wave's accesses in order, the compiler must keep them so
#define QT_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

__global__ __launch_bounds__(1024) void k_adv_moments(const float* __restrict__ adv, const long long* __restrict__ idx, long long total, int B, float* __restrict__ out) {
    __shared__ float sc[tr::MOM_CHAINS], sg[tr::MOM_CHAINS / 16], sm;
    const int c = threadIdx.x;
    float mean = 0.0f;
    for (int pass = 0; pass < 2; pass++) {
        float acc = 0.0f;
        for (int s = c; s < B; s += tr::MOM_CHAINS) {
            const long long i = idx[s];
            if (i < 0 || i >= total) continue;
            const float a = adv[i];
            if (pass == 0) acc += a;
            else { const float d = a - mean; acc = fmaf(d, d, acc); }
        }
        sc[c] = acc;
        __syncthreads();
        if (c < tr::MOM_CHAINS / 16) {
            float gs = 0.0f;
            for (int k = 0; k < 16; k++) gs += sc[16 * c + k];
            sg[c] = gs;
        }
        __syncthreads();
        if (c == 0) {
            float tot = 0.0f;
            for (int k = 0; k < tr::MOM_CHAINS / 16; k++) tot += sg[k];
            if (pass == 0) sm = tot / (float)B;
            else { out[0] = mean; out[1] = B > 1 ? sqrtf(tot / (float)(B - 1)) : 0.0f; }
        }
        __syncthreads();
        mean = sm;
    }
}

// One network over all the tiles of the wave's part.  Every wave of the workgroup calls it (the images are staged by all of them).
template <bool ACTOR>
__device__ __forceinline__ void net_phase(const Net& net, const tr::Image& im, const float* __restrict__ par, const GradArgs& a, float* sw, float* rows,
                                          float* prow, int row_off, int ls_off, int part, bool part_on) {
    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, g = lane >> 4;
    const int L = net.n_layers, act = net.activation;
    float* const sx = rows;
    float* const sh0 = rows + TILE * S;
    float* const sh1 = rows + 2 * TILE * S;
    float* const so = rows + 3 * TILE * S;
    float* const st = rows + 4 * TILE * S;

    for (int l = 0; l < L; l++) {
        const int in = net.in[l], out = net.out[l], in4 = round_up(in, 4), op = out_pad(out);
        const float* const W = par + net.w_off[l];
        for (int i = tid; i < in4 * op; i += blockDim.x) {
            const int k = i / op, o = i - k * op;
            sw[im.fw_off[l] + i] = (o < out && k < in) ? W[(size_t)o * in + k] : 0.0f;
        }
        if (l > 0) {
            const int out4 = round_up(out, 4), ip = out_pad(in);
            for (int i = tid; i < out4 * ip; i += blockDim.x) {
                const int o = i / ip, k = i - o * ip;
                sw[im.rw_off[l] + i] = (o < out && k < in) ? W[(size_t)o * in + k] : 0.0f;
            }
        }
    }
    __syncthreads();
    if (!part_on) return;                                                  // (wave-uniform; no workgroup barrier below)

    f32x4 G[ML][NT][NT];
    float db[ML], dls = 0.0f, stat = 0.0f;
    int refused = 0;
#pragma unroll
    for (int l = 0; l < ML; l++) {
        db[l] = 0.0f;
#pragma unroll
        for (int to = 0; to < NT; to++)
#pragma unroll
            for (int ti = 0; ti < NT; ti++) G[l][to][ti] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const float fB = (float)a.B;
    const float mean_b = a.norm_on ? a.moments[0] : 0.0f, std_b = a.norm_on ? a.moments[1] : 0.0f;
    const int n_tiles = tr::tiles_of(a.B), A = net.action_dim, od = net.obs_dim, od16 = round_up(od, TILE);

    for (int tile = part; tile < n_tiles; tile += tr::PARTS) {
        const int s_at = tile * TILE + e;
        const bool in_batch = s_at < a.B;
        const long long at = in_batch ? a.idx[s_at] : -1;
        const bool valid = in_batch && at >= 0 && at < a.total;
        if (ACTOR) refused += __builtin_popcountll(__builtin_amdgcn_ballot_w64(in_batch && !valid && g == 0));

        for (int k = g; k < od16; k += 4) sx[e * S + k] = (valid && k < od) ? a.obs[(size_t)at * od + k] : 0.0f;
        QT_WAVE_SYNC();

        // forward: every layer's activations stay in the rows (layer 0 -> sh0, layer 1 -> sh1, the last -> so)
#pragma unroll
        for (int l = 0; l < ML; l++) {
            if (l < L) {
                const bool last = l == L - 1;
                const int in4 = round_up(net.in[l], 4), out = net.out[l], nt = (out + TILE - 1) / TILE, op = out_pad(out);
                const float* const hin = l == 0 ? sx : (l == 1 ? sh0 : sh1);
                float* const hout = last ? so : (l == 0 ? sh0 : sh1);
                f32x4 acc[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (t < nt) {
#pragma unroll
                        for (int r = 0; r < 4; r++) { const int o = TILE * t + 4 * g + r; acc[t][r] = o < out ? par[net.b_off[l] + o] : 0.0f; }
                    }
                }
                for (int s = 0; s < in4; s += 4) {
                    const float b = hin[e * S + s + g];
                    const float* const wk = sw + im.fw_off[l] + (s + g) * op + e;
#pragma unroll
                    for (int t = 0; t < NT; t++)
                        if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[TILE * t], b, acc[t], 0, 0, 0);
                }
                const int kind = last ? (int)QS_POLICY_ACT_NONE : act;
#pragma unroll
                for (int t = 0; t < NT; t++)
                    if (t < nt) {
                        f32x4 v;
#pragma unroll
                        for (int r = 0; r < 4; r++) v[r] = valid ? activate(acc[t][r], kind) : 0.0f;
                        *(f32x4*)(hout + e * S + TILE * t + 4 * g) = v;
                    }
                QT_WAVE_SYNC();
            }
        }

        // the loss epilogue: so becomes d loss / d output; st receives the log_std terms (columns < 64) and the statistics (columns 64 ..)
        if (ACTOR) {
            for (int j = g; j < A; j += 4) {
                const float ls = a.log_std[j], z = tr::z_of(valid ? a.actions[(size_t)at * A + j] : 0.0f, so[e * S + j], expf(-ls));
                st[e * S + j] = log_prob_term(z, ls);
            }
            QT_WAVE_SYNC();
            float lp = 0.0f;
            for (int j = 0; j < A; j++) lp += st[e * S + j];
            QT_WAVE_SYNC();
            tr::PolTerms t = {0.0f, 0.0f, 0.0f, 0.0f};
            if (valid) t = tr::policy_terms(lp, a.old_log_prob[at], tr::adv_norm(a.adv[at], mean_b, std_b, a.norm_on), a.clip_range, fB);
            for (int j = g; j < tr::MAX_WIDTH; j += 4) {
                float term = 0.0f;
                if (j < A) {
                    const float ls = a.log_std[j], inv = expf(-ls), z = tr::z_of(valid ? a.actions[(size_t)at * A + j] : 0.0f, so[e * S + j], inv);
                    so[e * S + j] = valid ? tr::mean_grad(t.dlp, z, inv) : 0.0f;
                    term = valid ? tr::log_std_term(t.dlp, z) : 0.0f;
                }
                st[e * S + j] = term;
            }
            st[e * S + 64 + g] = g == 0 ? t.pol : (g == 1 ? t.kl : (g == 2 ? t.clip : 0.0f));
        } else {
            const float value = so[e * S];
            QT_WAVE_SYNC();
            const float ret = valid ? a.returns[at] : 0.0f;
            if (g == 0) so[e * S] = valid ? tr::value_grad(value, ret, a.vf_coef, fB) : 0.0f;
            st[e * S + 64 + g] = (g == 0 && valid) ? tr::value_term(value, ret) : 0.0f;
        }
        QT_WAVE_SYNC();
        if (ACTOR) {
            for (int s = 0; s < TILE; s++) dls += st[s * S + lane];
        }
        if (lane < 4) {
            for (int s = 0; s < TILE; s++) stat += st[s * S + 64 + lane];
        }

        // backward: layer l's delta is where its activations were (the last layer's in so), h_(l-1) below it
#pragma unroll
        for (int l = ML - 1; l >= 0; l--) {
            if (l < L) {
                const int in = net.in[l], out = net.out[l], nto = (out + TILE - 1) / TILE, nti = (in + TILE - 1) / TILE;
                const float* const D = l == L - 1 ? so : (l == 0 ? sh0 : sh1);
                float* const Hp = l == 0 ? sx : (l == 1 ? sh0 : sh1);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float av[NT], bv[NT];
#pragma unroll
                    for (int t = 0; t < NT; t++) {
                        av[t] = t < nto ? D[(4 * q + g) * S + TILE * t + e] : 0.0f;
                        bv[t] = t < nti ? Hp[(4 * q + g) * S + TILE * t + e] : 0.0f;
                    }
#pragma unroll
                    for (int to = 0; to < NT; to++)
#pragma unroll
                        for (int ti = 0; ti < NT; ti++)
                            if (to < nto && ti < nti) G[l][to][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[to], bv[ti], G[l][to][ti], 0, 0, 0);
                }
                if (lane < out) {
                    for (int s = 0; s < TILE; s++) db[l] += D[s * S + lane];
                }
                if (l > 0) {
                    const int out4 = round_up(out, 4), ip = out_pad(in);
                    f32x4 acc[NT];
#pragma unroll
                    for (int t = 0; t < NT; t++) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    for (int s = 0; s < out4; s += 4) {
                        const float b = D[e * S + s + g];
                        const float* const wk = sw + im.rw_off[l] + (s + g) * ip + e;
#pragma unroll
                        for (int t = 0; t < NT; t++)
                            if (t < nti) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[TILE * t], b, acc[t], 0, 0, 0);
                    }
#pragma unroll
                    for (int t = 0; t < NT; t++)
                        if (t < nti) {
                            float* const at_h = Hp + e * S + TILE * t + 4 * g;
                            const f32x4 hv = *(const f32x4*)at_h;
                            f32x4 v;
#pragma unroll
                            for (int r = 0; r < 4; r++) v[r] = acc[t][r] * tr::dact(hv[r], act);
                            *(f32x4*)at_h = v;
                        }
                    QT_WAVE_SYNC();
                }
            }
        }
        QT_WAVE_SYNC();                                                    // the rows are free for the next tile
    }

    // the part's sums -> its row: [actor | critic | log_std | pad | statistics]
    float* const base = prow + row_off;
#pragma unroll
    for (int l = 0; l < ML; l++) {
        if (l < L) {
            const int in = net.in[l], out = net.out[l], nto = (out + TILE - 1) / TILE, nti = (in + TILE - 1) / TILE;
#pragma unroll
            for (int to = 0; to < NT; to++)
#pragma unroll
                for (int ti = 0; ti < NT; ti++)
                    if (to < nto && ti < nti) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int o = TILE * to + 4 * g + r, i = TILE * ti + e;
                            if (o < out && i < in) base[net.w_off[l] + o * in + i] = G[l][to][ti][r];
                        }
                    }
            if (lane < out) base[net.b_off[l] + lane] = db[l];
        }
    }
    float* const ps = prow + a.stride - tr::PART_STATS;
    if (ACTOR) {
        if (lane < A) prow[ls_off + lane] = dls;
        if (lane == 0) { ps[tr::PS_POLICY] = stat; ps[tr::PS_REFUSED] = (float)refused; }
        if (lane == 1) ps[tr::PS_KL] = stat;
        if (lane == 2) ps[tr::PS_CLIP] = stat;
    } else if (lane == 0) ps[tr::PS_VALUE] = stat;
}

__global__ __launch_bounds__(256) void k_ppo_grad(Net actor, Net critic, GradArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ f32x4 qt_lds[];
    const int wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int part = blockIdx.x * n_waves + wave;
    const bool part_on = part < tr::parts_used(a.B);                       // (wave-uniform)
    float* const sw = (float*)qt_lds;
    float* const rows = sw + a.image_floats + (size_t)wave * tr::ROW_SETS * TILE * S;
    float* const prow = a.parts + (size_t)(part_on ? part : 0) * a.stride;
    net_phase<true>(actor, a.ia, a.actor_params, a, sw, rows, prow, 0, actor.n_params + critic.n_params, part, part_on);
    __syncthreads();                                                       // every wave is done with the actor's images
    net_phase<false>(critic, a.ic, a.critic_params, a, sw, rows, prow, actor.n_params, 0, part, part_on);
#endif
}

// grad[i] = the parts' rows added in ascending order (log_std: - ent_coef); a block's sum of squares; block 0 finishes the statistics
__global__ __launch_bounds__(256) void k_ppo_reduce(const float* __restrict__ parts, int stride, int n_total, int off_ls, int A, int B,
                                                    const float* __restrict__ log_std, float ent_coef, float vf_coef, float* __restrict__ grad,
                                                    float* __restrict__ sumsq, float* __restrict__ stats, unsigned long long* __restrict__ refused) {
    __shared__ float sq[tr::NORM_BLOCK], sums[tr::PART_STATS];
    if (threadIdx.x >= tr::PART_STATS_USED && threadIdx.x < tr::PART_STATS) sums[threadIdx.x] = 0.0f;
    const int tid = threadIdx.x, i = blockIdx.x * tr::NORM_BLOCK + tid, used = tr::parts_used(B);
    float acc = 0.0f;
    if (i < n_total) {
        for (int p = 0; p < used; p++) acc += parts[(size_t)p * stride + i];
        if (i >= off_ls) acc -= ent_coef;
        grad[i] = acc;
    }
    sq[tid] = acc;
    if (blockIdx.x == 0 && tid < tr::PART_STATS_USED) {
        double s = 0.0;                                                    // (the statistics' one float64 accumulator, qs_ppo_train.h)
        for (int p = 0; p < used; p++) s += (double)parts[(size_t)p * stride + stride - tr::PART_STATS + tid];
        sums[tid] = (float)s;
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
        for (int k = 0; k < tr::NORM_BLOCK; k++) s = fmaf(sq[k], sq[k], s);
        sumsq[blockIdx.x] = s;
        if (blockIdx.x == 0) {
            float local[QS_PPO_N_STATS];
            tr::finish_stats(sums, tr::entropy_of(log_std, A), ent_coef, vf_coef, B, local);
            for (int k = 0; k < QS_PPO_N_STATS; k++) stats[k] = local[k];
            *refused += (unsigned long long)sums[tr::PS_REFUSED];
        }
    }
}

// one workgroup: the norm from the blocks' sums of squares, then clip and Adam in place
__global__ __launch_bounds__(1024) void k_ppo_adam(const float* __restrict__ grad, const float* __restrict__ sumsq, int n_blocks, int n_actor, int n_critic,
                                                   int n_total, tr::AdamConsts k, float* __restrict__ pa, float* __restrict__ pc, float* __restrict__ log_std,
                                                   float* __restrict__ m, float* __restrict__ v, float* __restrict__ stats) {
    __shared__ float s_coef;
    if (threadIdx.x == 0) {
        float tot = 0.0f;
        for (int b = 0; b < n_blocks; b++) tot += sumsq[b];
        const float norm = sqrtf(tot);
        stats[QS_PPO_STAT_GRAD_NORM] = norm;
        s_coef = tr::clip_coef(norm, k.max_norm);
    }
    __syncthreads();
    const float coef = s_coef;
    for (int i = threadIdx.x; i < n_total; i += blockDim.x) {
        float* const p = i < n_actor ? pa + i : (i < n_actor + n_critic ? pc + (i - n_actor) : log_std + (i - n_actor - n_critic));
        float pv = *p, mv = m[i], vv = v[i];
        tr::adam_elem(grad[i], coef, k, pv, mv, vv);
        *p = pv; m[i] = mv; v[i] = vv;
    }
}

}  // namespace

extern "C" {

int qs_ppo_create(const qs_policy_desc* actor, const qs_policy_desc* critic, int max_batch, int device, qs_ppo** out) {
    if (!actor || !critic || !out) QS_FAIL(-1, "null argument");
    Net na, nc;
    if (tr::check_train(*actor, *critic, na, nc, qs_g_err, sizeof(qs_g_err))) return -1;
    if (max_batch <= 0) QS_FAIL(-1, "qs_ppo_create: max_batch = %d must be positive", max_batch);
    const tr::Image ia = tr::image_of(na), ic = tr::image_of(nc);
    const int image_floats = ia.floats > ic.floats ? ia.floats : ic.floats, waves = tr::waves_of(image_floats);
    if (waves == 0)
        QS_FAIL(-1, "qs_ppo_create: the weight images (%d floats) and one wave's rows need %zu bytes of LDS, a compute unit has %zu", image_floats,
                tr::lds_bytes(image_floats, 1), LDS_MAX_BYTES);
    qs_ppo* h;
    if (int rc = qs_new_handle(out, device, &h)) return rc;
    h->actor = na; h->critic = nc; h->ia = ia; h->ic = ic; h->max_batch = max_batch;
    h->n_total = tr::total_params(na, nc); h->stride = tr::part_stride(h->n_total);
    h->waves = waves; h->image_floats = image_floats; h->lds_bytes = tr::lds_bytes(image_floats, waves);
    QS_ON_DEVICE(h);
    ZeroedAlloc zeroed;
    zeroed.e = hipFuncSetAttribute((const void*)k_ppo_grad, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes);
    const size_t parts_floats = (size_t)tr::PARTS * h->stride;                     // (a row's pad and spare statistics are never written)
    zeroed(&h->parts, parts_floats); zeroed(&h->moments, 2); zeroed(&h->sumsq, (size_t)tr::norm_blocks(h->n_total)); zeroed(&h->refused, 1);
    if (zeroed.failed("qs_ppo_create: %zu bytes of LDS, %zu bytes of part rows", h->lds_bytes, parts_floats * sizeof(float))) { qs_ppo_destroy(h); return -2; }
    *out = h;
    return 0;
}

void qs_ppo_destroy(qs_ppo* h) {
    qs_delete_handle(h, [](qs_ppo* h) { hipFree(h->parts); hipFree(h->moments); hipFree(h->sumsq); hipFree(h->refused); });
}

int qs_ppo_set_stream(qs_ppo* h, void* s) { return qs_set_stream_of(h, s); }

int qs_ppo_bind(qs_ppo* h, float* actor_params, float* critic_params, float* log_std, float* exp_avg, float* exp_avg_sq) {
    if (!h || !actor_params || !critic_params || !log_std || !exp_avg || !exp_avg_sq) QS_FAIL(-1, "null argument");
    h->pa = actor_params; h->pc = critic_params; h->log_std = log_std; h->m = exp_avg; h->v = exp_avg_sq;
    return 0;
}

int qs_ppo_grad(qs_ppo* h, const float* observations, const float* actions, const float* old_log_prob, const float* advantages, const float* returns,
                long long total, const long long* indices, int batch, const qs_ppo_hyper* hyper, float* grad_out, float* stats_out) {
    if (!h || !observations || !actions || !old_log_prob || !advantages || !returns || !indices || !hyper || !grad_out || !stats_out) QS_FAIL(-1, "null argument");
    if (!h->pa) QS_FAIL(-1, "qs_ppo_grad before qs_ppo_bind");
    if (batch <= 0 || batch > h->max_batch) QS_FAIL(-1, "qs_ppo_grad: batch = %d outside [1, max_batch = %d]", batch, h->max_batch);
    if (total <= 0) QS_FAIL(-1, "qs_ppo_grad: total = %lld must be positive", total);
    QS_ON_DEVICE(h);
    GradArgs a;
    memset(&a, 0, sizeof(a));
    a.obs = observations; a.actions = actions; a.old_log_prob = old_log_prob; a.adv = advantages; a.returns = returns;
    a.actor_params = h->pa; a.critic_params = h->pc; a.log_std = h->log_std; a.idx = indices; a.moments = h->moments; a.parts = h->parts;
    a.total = total; a.B = batch; a.stride = h->stride; a.image_floats = h->image_floats;
    a.norm_on = hyper->normalize_advantage && batch > 1;
    a.clip_range = hyper->clip_range; a.vf_coef = hyper->vf_coef; a.ia = h->ia; a.ic = h->ic;
    if (a.norm_on) {
        hipLaunchKernelGGL(k_adv_moments, dim3(1), dim3(tr::MOM_CHAINS), 0, h->stream, advantages, indices, total, batch, h->moments);
        QS_LAUNCHED();
    }
    const int used = tr::parts_used(batch);
    hipLaunchKernelGGL(k_ppo_grad, dim3((unsigned)((used + h->waves - 1) / h->waves)), dim3(64 * h->waves), h->lds_bytes, h->stream, h->actor, h->critic, a);
    QS_LAUNCHED();
    hipLaunchKernelGGL(k_ppo_reduce, dim3((unsigned)tr::norm_blocks(h->n_total)), dim3(tr::NORM_BLOCK), 0, h->stream, (const float*)h->parts, h->stride, h->n_total,
                       h->actor.n_params + h->critic.n_params, h->actor.action_dim, batch, (const float*)h->log_std, hyper->ent_coef, hyper->vf_coef, grad_out,
                       h->sumsq, stats_out, h->refused);
    QS_LAUNCHED();
    return 0;
}

int qs_ppo_adam(qs_ppo* h, const float* grad, const qs_ppo_hyper* hyper, int step, float* stats_inout) {
    if (!h || !grad || !hyper || !stats_inout) QS_FAIL(-1, "null argument");
    if (!h->pa) QS_FAIL(-1, "qs_ppo_adam before qs_ppo_bind");
    if (step <= 0) QS_FAIL(-1, "qs_ppo_adam: step = %d must be 1, 2, ...", step);
    QS_ON_DEVICE(h);
    hipLaunchKernelGGL(k_ppo_adam, dim3(1), dim3(1024), 0, h->stream, grad, (const float*)h->sumsq, tr::norm_blocks(h->n_total), h->actor.n_params,
                       h->critic.n_params, h->n_total, tr::adam_consts(*hyper, step), h->pa, h->pc, h->log_std, h->m, h->v, stats_inout);
    QS_LAUNCHED();
    return 0;
}

int qs_ppo_refusals(qs_ppo* h, unsigned long long* out) {
    if (!h || !out) QS_FAIL(-1, "null argument");
    QS_ON_DEVICE(h);
    QS_HIP(hipMemcpyAsync(out, h->refused, sizeof(*out), hipMemcpyDeviceToHost, h->stream));
    QS_HIP(hipMemsetAsync(h->refused, 0, sizeof(*out), h->stream));
    QS_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
