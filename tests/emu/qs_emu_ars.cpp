// qs_emu_ars.cpp -- TEST-ONLY host build of ARS's bookkeeping (quadruped-springs_amd/csrc/qs_ars.h): what k_ars_perturb, k_ars_begin,
// k_ars_account, k_ars_returns, k_ars_select and k_ars_apply compute, as plain loops over their lanes.  sqrtf is this platform's libm.
#include <stddef.h>
#include "../../quadruped-springs_amd/csrc/qs_ars.h"

namespace ars = qs::ars;

extern "C" {
// 0, or -1 with the reason qs_ars_create would give in err
int qsea_check(int n_envs, int n_delta, int n_params, int episodes_per_env, char* err, int err_size) {
    return ars::check_shape(n_envs, n_delta, n_params, episodes_per_env, err, (size_t)err_size);
}
void qsea_perturb(const float* theta, const float* delta, int n_delta, int n_params, float sigma, float* cand) {
    ars::perturb_host(theta, delta, n_delta, n_params, sigma, cand);
}
void qsea_begin(float* ret, int* len, int* episodes, uint8_t* alive, int n_envs, int* n_alive) { ars::begin_host(ret, len, episodes, alive, n_envs, n_alive); }
void qsea_account(float* ret, int* len, int* episodes, uint8_t* alive, const float* raw_reward, const uint8_t* done, int n_envs, int episodes_per_env, int* n_alive) {
    ars::account_host(ret, len, episodes, alive, raw_reward, done, n_envs, episodes_per_env, n_alive);
}
long long qsea_returns(const float* ret, const int* len, int n_envs, int n_delta, float alive_bonus_offset, float* R) {
    return ars::returns_host(ret, len, n_envs, n_delta, alive_bonus_offset, R);
}
void qsea_select(const float* R, int n_delta, int b, float lr, int* idx, float* w, float* stats) { ars::select_host(R, n_delta, b, lr, idx, w, stats); }
void qsea_apply(float* theta, const float* delta, int n_params, const int* idx, const float* w, int b, float step) {
    ars::apply_host(theta, delta, n_params, idx, w, b, step);
}
}
