// qs_emu_ppo_train.cpp -- TEST-ONLY host build of the PPO update (quadruped-springs_amd/csrc/qs_ppo_train.h): what k_adv_moments, k_ppo_grad,
// k_ppo_reduce and k_ppo_adam compute, as plain loops in the header's stated order.  expf / tanhf / sqrtf are this platform's libm.
#include <stddef.h>
#include "../../quadruped-springs_amd/csrc/qs_ppo_train.h"

using namespace qs::pol;
namespace train = qs::train;

extern "C" {
// 0, or -1 with the reason qs_ppo_create would give in err
int qsept_check(const qs_policy_desc* da, const qs_policy_desc* dc, char* err, int err_size) {
    Net na, nc;
    return train::check_train(*da, *dc, na, nc, err, (size_t)err_size);
}
// out[0..5] = n_actor, n_critic, n_total, PARTS, waves of a workgroup (0: does not fit), LDS bytes of that workgroup
int qsept_layout(const qs_policy_desc* da, const qs_policy_desc* dc, long long* out) {
    Net na, nc;
    char err[512];
    if (train::check_train(*da, *dc, na, nc, err, sizeof(err))) return -1;
    const train::Image ia = train::image_of(na), ic = train::image_of(nc);
    const int floats = ia.floats > ic.floats ? ia.floats : ic.floats, waves = train::waves_of(floats);
    out[0] = na.n_params; out[1] = nc.n_params; out[2] = train::total_params(na, nc); out[3] = train::PARTS; out[4] = waves;
    out[5] = (long long)train::lds_bytes(floats, waves ? waves : 1);
    return 0;
}
void qsept_moments(const float* adv, long long total, const long long* idx, int B, float* mean, float* sd) {
    train::adv_moments_host(adv, total, idx, B, mean, sd);
}
// qs_ppo_grad: returns the refused samples, or -1; flags [B] or null: per sample bit 0 = unclipped branch, bit 1 = clipped
int qsept_grad(const qs_policy_desc* da, const qs_policy_desc* dc, const float* pa, const float* pc, const float* log_std, const float* obs,
               const float* actions, const float* old_log_prob, const float* adv, const float* returns, long long total, const long long* idx, int B,
               const qs_ppo_hyper* hy, float* grad, float* stats, unsigned char* flags) {
    Net na, nc;
    char err[512];
    if (train::check_train(*da, *dc, na, nc, err, sizeof(err))) return -1;
    return train::grad_host(na, nc, pa, pc, log_std, obs, actions, old_log_prob, adv, returns, total, idx, B, *hy, grad, stats, flags);
}
// qs_ppo_adam on the flat arrays [n]: returns the norm before clipping
float qsept_adam(float* p, float* m, float* v, const float* grad, int n, const qs_ppo_hyper* hy, int step) {
    return train::adam_host(p, m, v, grad, n, *hy, step);
}
}
