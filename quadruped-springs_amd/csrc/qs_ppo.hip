// qs_ppo.hip -- k_actor_critic, k_gae and the C ABI of on-device PPO collection (qs_ac_*, qs_gae; include/qs_amd.h): what SB3's
// OnPolicyAlgorithm.collect_rollouts does per step (policy.forward, RolloutBuffer.add, the time-limit bootstrap) and
// RolloutBuffer.compute_returns_and_advantage, without a host round trip.  The arithmetic is csrc/qs_ppo.h.
//
// k_actor_critic: a wave takes 16 consecutive environments, a workgroup is 1, 2 or 4 such waves and shares the weight image, as in k_policy
// (qs_policy.hip), whose tile layout this is: A = the weights from the k-major LDS image, B = the wave's activations from its LDS rows
// [env][k], one accumulator tile per 16 outputs, the result back to the rows as one 16-byte store per tile.  Each wave has TWO sets of
// rows: `sx` holds the tile's observations, read from global memory once (and written on to row t of the rollout from the same
// registers), `sa` the activations.  A network's first layer reads sx and writes sa, its later layers work on sa in place, so the
// observations are still there when the second network starts.  The actor runs first, its epilogue writes the clipped action for the
// environment step and the unclipped action and the log-prob into row t; then the critic runs on the same rows and writes the value.
// One weight image is in LDS at a time (the layers of both networks pass through the same region, at most 48 KB).
//
// The critic-only build of the same body computes V(obs) for the environments a uint8 mask names (all without a mask) and either
// stores it (the last values of a rollout) or adds gamma * V to a reward in place (the time-limit bootstrap).  A masked launch has
// one wave per workgroup; a wave whose tile has no masked environment leaves at a ballot before it stages anything.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "qs_ppo.h"
#include "qs_host.h"

using namespace qs::pol;
namespace ppo = qs::ppo;

namespace {
struct AcArgs {
    const float* obs; const float* actor_params; const float* critic_params; const float* eps; const float* log_std;
    float* env_actions; float* obs_row; float* action_row; float* value_row; float* log_prob_row;   // collect
    const uint8_t* mask; float* values_out; float* rewards; float gamma;                            // critic only
    int n, tiles, act_stride, w_floats;
};
typedef void (*AcKernel)(Net, Net, AcArgs);
}  // namespace

struct qs_ac {
    qs_policy_desc actor_desc, critic_desc;
    Net actor, critic;
    int device, n, tiles, waves, act_stride, w_floats;
    size_t lds_bytes, lds_bytes_one;   // of a launch with `waves` waves / with one wave (masked)
    AcKernel k_collect, k_critic;      // k_actor_critic<4 or 16, true / false>, chosen at create
    hipStream_t stream;
    const float* actor_params;         // the caller's arrays (kept, not copied)
    const float* critic_params;
};

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// a wave's LDS rows are written by some of its lanes and read by others: LDS serves one wave's accesses in order, the compiler must keep them so
#define QA_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// One network over the wave's tile: observations in sx [16][S], activations (and at the end the outputs) in sa [16][S].  Every wave of the
// workgroup calls it (the weight image is staged by all of them, between two workgroup barriers); a wave without a tile skips the MFMAs.
template <int NT>
__device__ __forceinline__ void net_forward(const Net& net, const float* par, float* sw, int w_floats, const float* sx, float* sa, int S, bool tile_on) {
    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, g = lane >> 4;
    for (int l = 0; l < net.n_layers; l++) {
        const int in = net.in[l], out = net.out[l], in4 = round_up(in, 4), nt = (out + TILE - 1) / TILE, op = out_pad(out);
        int kc = (w_floats / op) & ~3;
        if (kc > in4) kc = in4;
        const float* const W = par + net.w_off[l];
        const float* const h = l == 0 ? sx : sa;
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
                    const float b = h[e * S + k0 + s + g];
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
        QA_WAVE_SYNC();
    }
}

// NT: accumulator tiles a layer may need (4: every width <= 64; 16: widths up to 256).  ACTOR: the collected step (actor, then critic);
// otherwise the critic alone, under the mask.
template <int NT, bool ACTOR>
__global__ __launch_bounds__(256) void k_actor_critic(Net actor, Net critic, AcArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ f32x4 qa_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const int e = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x * n_waves + wave;
    const bool tile_on = tile < a.tiles;                                  // (wave-uniform)
    const int S = a.act_stride;
    float* const sw = (float*)qa_lds;
    float* const sx = sw + a.w_floats + (size_t)wave * 2 * TILE * S;      // this wave's observations [16][S]
    float* const sa = sx + TILE * S;                                      // and activations [16][S]
    const int row0 = tile * TILE;
    const int rows = tile_on ? min(TILE, a.n - row0) : 0;
    const size_t env = (size_t)row0 + e;

    bool want = e < rows && g == 0;                                       // the lane that writes environment e's value
    if (!ACTOR && a.mask) {
        want = want && a.mask[env] != 0;
        if (n_waves == 1 && __builtin_amdgcn_ballot_w64(want) == 0) return;   // (a masked launch: the wave is the workgroup)
    }

    // observations: the tile's rows are contiguous in memory; read once, kept in sx for both networks
    {
        const int od = actor.obs_dim, od4 = round_up(od, 4);
        const size_t base = (size_t)row0 * od;
        for (int i = lane; i < rows * od; i += 64) {
            const int r = i / od;
            const float v = a.obs[base + i];
            sx[r * S + (i - r * od)] = v;
            if (ACTOR) a.obs_row[base + i] = v;
        }
        for (int i = lane; i < TILE * od4; i += 64) { const int r = i / od4, k = i - r * od4; if (r >= rows || k >= od) sx[r * S + k] = 0.0f; }
    }
    QA_WAVE_SYNC();

    if (ACTOR) {
        net_forward<NT>(actor, a.actor_params, sw, a.w_floats, sx, sa, S, tile_on);
        if (e < rows) {
            const int A = actor.action_dim;
            const float* const eps_row = a.eps + env * A;
            for (int j = g; j < A; j += 4) ppo::collect_elem(actor, sa[e * S + j], eps_row, a.log_std, j, a.env_actions + env * A, a.action_row + env * A);
            if (g == 0) a.log_prob_row[env] = log_prob_row(actor, eps_row, a.log_std);
        }
        QA_WAVE_SYNC();                                                   // the means are read before the critic writes the rows
    }
    net_forward<NT>(critic, a.critic_params, sw, a.w_floats, sx, sa, S, tile_on);
    if (want) {
        const float v = sa[e * S];
        if (ACTOR) a.value_row[env] = v;
        else if (a.rewards) a.rewards[env] = ppo::bootstrap_reward(a.gamma, v, a.rewards[env]);
        else a.values_out[env] = v;
    }
#endif
}

// one lane per environment walks t = T-1 ... 0; arrays [T][N], so a wave's loads and stores of one t are consecutive
__global__ __launch_bounds__(256) void k_gae(const float* __restrict__ rewards, const float* __restrict__ values, const float* __restrict__ episode_starts,
                                             const float* __restrict__ last_values, const uint8_t* __restrict__ last_dones, int T, int N, float gamma,
                                             float lambda, float* __restrict__ advantages, float* __restrict__ returns) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float gl = gamma * lambda;
    float gae = 0.0f, nv = last_values[i], nnt = 1.0f - (last_dones[i] ? 1.0f : 0.0f);
    size_t at = (size_t)(T - 1) * N + i;
    float r = rewards[at], v = values[at], es = episode_starts[at];
    for (int t = T - 1; t >= 0; t--) {
        float r1 = 0.0f, v1 = 0.0f, es1 = 0.0f;
        if (t > 0) { r1 = rewards[at - N]; v1 = values[at - N]; es1 = episode_starts[at - N]; }   // step t-1's loads, ahead of step t's chain
        float ret;
        ppo::gae_step(gamma, gl, r, v, nv, nnt, gae, ret);
        advantages[at] = gae; returns[at] = ret;
        nv = v; nnt = 1.0f - es;
        r = r1; v = v1; es = es1;
        if (t > 0) at -= N;
    }
}

int launch(qs_ac* h, AcKernel kernel, const AcArgs& a, bool one_wave) {
    const int waves = one_wave ? 1 : h->waves;
    const size_t lds = one_wave ? h->lds_bytes_one : h->lds_bytes;
    const dim3 grid((unsigned)((h->tiles + waves - 1) / waves)), block(64 * waves);
    hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, h->actor, h->critic, a);
    QS_LAUNCHED();
    return 0;
}

AcArgs base_args(const qs_ac* h, const float* obs) {
    AcArgs a;
    memset(&a, 0, sizeof(a));
    a.obs = obs; a.actor_params = h->actor_params; a.critic_params = h->critic_params;
    a.n = h->n; a.tiles = h->tiles; a.act_stride = h->act_stride; a.w_floats = h->w_floats;
    return a;
}

}  // namespace

extern "C" {

int qs_ac_create(const qs_policy_desc* actor, const qs_policy_desc* critic, int device, qs_ac** out) {
    if (!actor || !critic || !out) QS_FAIL(-1, "null argument");
    Net na, nc;
    if (net_from_desc(*actor, na, qs_g_err, sizeof(qs_g_err))) return -1;
    if (net_from_desc(*critic, nc, qs_g_err, sizeof(qs_g_err))) return -1;
    if (ppo::check_pair(*actor, *critic, qs_g_err, sizeof(qs_g_err))) return -1;
    qs_ac* h;
    if (int rc = qs_new_handle(out, device, &h)) return rc;
    h->actor_desc = *actor; h->critic_desc = *critic; h->actor = na; h->critic = nc;
    h->n = actor->n_envs;
    h->tiles = (h->n + TILE - 1) / TILE;
    const Net* nets[2] = {&h->actor, &h->critic};
    int wide;
    layout_sizes(nets, 2, h->act_stride, h->w_floats, wide);
    h->waves = waves_per_workgroup(h->tiles, 1, h->w_floats, 2, h->act_stride);
    h->lds_bytes = lds_bytes(h->w_floats, h->waves, 2, h->act_stride); h->lds_bytes_one = lds_bytes(h->w_floats, 1, 2, h->act_stride);
    h->k_collect = wide ? k_actor_critic<16, true> : k_actor_critic<4, true>;
    h->k_critic = wide ? k_actor_critic<16, false> : k_actor_critic<4, false>;
    QS_ON_DEVICE(h);
    const int lds = (int)h->lds_bytes;            // (the largest launch; a one-wave launch needs less)
    hipError_t e = hipFuncSetAttribute((const void*)h->k_collect, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)h->k_critic, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) { snprintf(qs_g_err, sizeof(qs_g_err), "hipFuncSetAttribute(%zu bytes of LDS) failed: %s", h->lds_bytes, hipGetErrorString(e)); delete h; return -2; }
    *out = h;
    return 0;
}

void qs_ac_destroy(qs_ac* h) { qs_delete_handle(h, [](qs_ac*) {}); }   // (no device memory of its own)

int qs_ac_set_stream(qs_ac* h, void* s) { return qs_set_stream_of(h, s); }

int qs_ac_set_params(qs_ac* h, const float* actor_params, const float* critic_params) {
    if (!h || !actor_params || !critic_params) QS_FAIL(-1, "null argument");
    h->actor_params = actor_params; h->critic_params = critic_params;
    return 0;
}

int qs_ac_collect(qs_ac* h, const float* obs, const float* eps, const float* log_std, float* env_actions, float* obs_row, float* action_row,
                  float* value_row, float* log_prob_row) {
    if (!h || !obs || !eps || !log_std || !env_actions || !obs_row || !action_row || !value_row || !log_prob_row)
        QS_FAIL(-1, "null argument (qs_ac_collect needs every pointer; eps is required: a collected step is a sample)");
    if (!h->actor_params) QS_FAIL(-1, "qs_ac_collect before qs_ac_set_params");
    QS_ON_DEVICE(h);
    AcArgs a = base_args(h, obs);
    a.eps = eps; a.log_std = log_std; a.env_actions = env_actions; a.obs_row = obs_row; a.action_row = action_row; a.value_row = value_row;
    a.log_prob_row = log_prob_row;
    return launch(h, h->k_collect, a, false);
}

int qs_ac_values(qs_ac* h, const float* obs, const uint8_t* mask, float* values_out) {
    if (!h || !obs || !values_out) QS_FAIL(-1, "null argument (handle, obs and values_out are required)");
    if (!h->critic_params) QS_FAIL(-1, "qs_ac_values before qs_ac_set_params");
    QS_ON_DEVICE(h);
    AcArgs a = base_args(h, obs);
    a.mask = mask; a.values_out = values_out;
    return launch(h, h->k_critic, a, mask != nullptr);
}

int qs_ac_bootstrap(qs_ac* h, const float* terminal_obs, const uint8_t* truncated, float gamma, float* rewards_inout) {
    if (!h || !terminal_obs || !truncated || !rewards_inout) QS_FAIL(-1, "null argument");
    if (!h->critic_params) QS_FAIL(-1, "qs_ac_bootstrap before qs_ac_set_params");
    QS_ON_DEVICE(h);
    AcArgs a = base_args(h, terminal_obs);
    a.mask = truncated; a.rewards = rewards_inout; a.gamma = gamma;
    return launch(h, h->k_critic, a, true);
}

int qs_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values, const uint8_t* last_dones, int T, int N,
           float gamma, float lambda, float* advantages, float* returns, void* hip_stream) {
    if (!rewards || !values || !episode_starts || !last_values || !last_dones || !advantages || !returns) QS_FAIL(-1, "null argument");
    if (T <= 0 || N <= 0) QS_FAIL(-1, "qs_gae: T = %d and N = %d must be positive", T, N);
    hipLaunchKernelGGL(k_gae, dim3(qs_blocks(N, 256)), dim3(256), 0, (hipStream_t)hip_stream, rewards, values, episode_starts, last_values,
                       last_dones, T, N, gamma, lambda, advantages, returns);
    QS_LAUNCHED();
    return 0;
}

}  // extern "C"
