// qs_ppo.h -- the arithmetic of on-device PPO collection (SB3 OnPolicyAlgorithm.collect_rollouts and RolloutBuffer.compute_returns_and_advantage),
// shared by k_actor_critic / k_gae (qs_ppo.hip) and their TEST-ONLY host build (tests/emu/qs_emu_ppo.cpp).
//
// Numerical contract: float32 throughout.
//   Actor and critic are two separate networks (SB3 MlpPolicy's net_arch = dict(pi=[..], vf=[..])), each qs_policy.h's chain unchanged: the
//   critic is a Net with action_dim 1, no squash and no clip.  For one environment
//       mean       = actor(obs)                                    forward_env / the MFMA tiles: one fmaf chain per pre-activation
//       action     = fmaf(expf(log_std[j]), eps[j], mean[j])       gauss_action: what the rollout stores (SB3 stores the unclipped action)
//       env_action = clamp(action, lo, hi)                         epilogue_elem: what the environment steps with
//       log_prob   = log_prob_row(eps, log_std)                    summed in ascending j
//       value      = critic(obs)[0]
//   so action, value and log-prob are the bits two qs_policy handles give for the same parameters.
//   Time-limit bootstrap (collect_rollouts: rewards[i] += gamma * V(terminal_obs[i]) where TimeLimit.truncated): ONE fmaf,
//       reward = fmaf(gamma, V(terminal_obs), reward)              for truncated environments; the others are not touched.
//   GAE, per environment, ONE sequence walking t = T-1 ... 0 with gae = 0 before the first step:
//       nnt   = 1 - (t == T-1 ? last_done : episode_start[t+1])
//       nv    =      t == T-1 ? last_value : value[t+1]
//       delta = fmaf(gamma * nnt, nv, reward[t]) - value[t]
//       gae   = fmaf(gamma * lambda * nnt, gae, delta)             gamma * lambda is rounded once; nnt is 0 or 1
//       advantage[t] = gae;   return[t] = gae + value[t]
//   There is no transcendental in it: the kernel and the host build agree bit for bit.
#pragma once
#include "qs_policy.h"

namespace qs {
namespace ppo {

using pol::Net;

// a critic is a Net that returns its last layer's single output as it is; writes why not into err
inline int check_pair(const qs_policy_desc& a, const qs_policy_desc& c, char* err, size_t err_size) {
#define QPPO_BAD(...) do { snprintf(err, err_size, __VA_ARGS__); return -1; } while (0)
    if (a.n_policies != 1 || c.n_policies != 1) QPPO_BAD("qs_ac_create: n_policies = %d (actor) / %d (critic): PPO collection takes one policy for all environments", a.n_policies, c.n_policies);
    if (a.n_envs != c.n_envs) QPPO_BAD("qs_ac_create: actor n_envs = %d, critic n_envs = %d", a.n_envs, c.n_envs);
    if (a.obs_dim != c.obs_dim) QPPO_BAD("qs_ac_create: actor obs_dim = %d, critic obs_dim = %d", a.obs_dim, c.obs_dim);
    if (c.action_dim != 1) QPPO_BAD("qs_ac_create: the critic's action_dim = %d must be 1 (the value)", c.action_dim);
    if (c.squash_output) QPPO_BAD("qs_ac_create: the critic has squash_output set: a value is not squashed");
    if (c.clip_lo > -3.0e38f || c.clip_hi < 3.0e38f) QPPO_BAD("qs_ac_create: the critic has finite clips [%g, %g]: a value is not clipped (-3e38 / 3e38)", (double)c.clip_lo, (double)c.clip_hi);
#undef QPPO_BAD
    return 0;
}

// one action dimension of a collected step, its mean known: the stored (unclipped) sample and the clipped one the environment reads
QP_HD void collect_elem(const Net& actor, float mean, const float* eps_row, const float* log_std, int j, float* env_act_row, float* action_row) {
    action_row[j] = pol::gauss_action(mean, log_std[j], eps_row[j]);
    pol::epilogue_elem(actor, mean, eps_row, log_std, j, env_act_row, nullptr);
}

QP_HD float bootstrap_reward(float gamma, float terminal_value, float reward) { return fmaf(gamma, terminal_value, reward); }

// one step of the backward walk; next_non_terminal is 0 or 1
QP_HD void gae_step(float gamma, float gamma_lambda, float reward, float value, float next_value, float next_non_terminal, float& gae, float& ret) {
    const float delta = fmaf(gamma * next_non_terminal, next_value, reward) - value;
    gae = fmaf(gamma_lambda * next_non_terminal, gae, delta);
    ret = gae + value;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One environment's walk on the host; the arrays are [T][N], `i` the environment.
inline void gae_env(const float* rewards, const float* values, const float* episode_starts, float last_value, uint8_t last_done, int T, int N, int i,
                    float gamma, float lambda, float* advantages, float* returns) {
    const float gl = gamma * lambda;
    float gae = 0.0f, nv = last_value, nnt = 1.0f - (last_done ? 1.0f : 0.0f);
    for (int t = T - 1; t >= 0; t--) {
        const size_t at = (size_t)t * N + i;
        float ret;
        gae_step(gamma, gl, rewards[at], values[at], nv, nnt, gae, ret);
        advantages[at] = gae; returns[at] = ret;
        nv = values[at]; nnt = 1.0f - episode_starts[at];
    }
}
// One environment's collected step on the host (both parameter rows are one policy's).
inline void collect_env(const Net& actor, const Net& critic, const float* pa, const float* pc, const float* obs, const float* eps_row, const float* log_std,
                        float* env_act_row, float* action_row, float* value, float* log_prob) {
    float mean[pol::MAX_WIDTH], clipped[pol::MAX_WIDTH], v, vc;
    pol::forward_env(actor, pa, obs, nullptr, nullptr, clipped, mean, nullptr);
    for (int j = 0; j < actor.action_dim; j++) collect_elem(actor, mean[j], eps_row, log_std, j, env_act_row, action_row);
    *log_prob = pol::log_prob_row(actor, eps_row, log_std);
    pol::forward_env(critic, pc, obs, nullptr, nullptr, &vc, &v, nullptr);
    *value = v;
}
inline float value_env(const Net& critic, const float* pc, const float* obs) {
    float v, vc;
    pol::forward_env(critic, pc, obs, nullptr, nullptr, &vc, &v, nullptr);
    return v;
}
#endif

}  // namespace ppo
}  // namespace qs
