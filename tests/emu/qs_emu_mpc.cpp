// qs_emu_mpc.cpp -- TEST-ONLY host build of the sampling planner (quadruped-springs_amd/csrc/qs_mpc.h): what k_mpc_sample, k_mpc_feed,
// k_mpc_finish and k_mpc_set_plan compute, as plain loops over their lanes.  rintf, fmaf, ldexpf and the division are this platform's libm
// and hardware (all exact or correctly rounded).
#include <stddef.h>
#include "../../quadruped-springs_amd/csrc/qs_mpc.h"

namespace mpc = qs::mpc;

extern "C" {
// 0, or -1 with the reason qs_mpc_create / qs_mpc_sample / qs_mpc_finish would give in err
int qsem_check(int n_robots, int n_candidates, int horizon, int action_dim, char* err, int err_size) {
    return mpc::check_shape(n_robots, n_candidates, horizon, action_dim, err, (size_t)err_size);
}
int qsem_check_sigma(float sigma, char* err, int err_size) { return mpc::check_sigma(sigma, err, (size_t)err_size); }
int qsem_check_lambda(float lambda, char* err, int err_size) { return mpc::check_lambda(lambda, err, (size_t)err_size); }
void qsem_exp_nonpos(const float* x, int n, float* out) {
    for (int i = 0; i < n; i++) out[i] = mpc::exp_nonpos(x[i]);
}
void qsem_sample(const float* plan, const float* eps, int M, int C, int H, int d, float sigma, float* seq, float* score, uint8_t* running) {
    mpc::sample_host(plan, eps, M, C, H, d, sigma, seq, score, running);
}
void qsem_feed(int step, const float* seq, float* score, uint8_t* running, int M, int C, int H, int d, const float* reward, const uint8_t* done,
               const float* reward_end, int stride, float* actions, uint8_t* active) {
    mpc::feed_host(step, seq, score, running, M, C, H, d, reward, done, reward_end, stride, actions, active);
}
void qsem_finish(const float* seq, const float* score, int M, int C, int H, int d, int method, float lambda, float* plan, float* actions, int* best,
                 float* best_score) {
    mpc::finish_host(seq, score, M, C, H, d, method, lambda, plan, actions, best, best_score);
}
void qsem_set_plan(float* plan, const float* src, const uint8_t* mask, int M, int H, int d) { mpc::set_plan_host(plan, src, mask, M, H, d); }
}
