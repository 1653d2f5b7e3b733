// qs_emu_policy.cpp -- TEST-ONLY host build of policy inference (quadruped-springs_amd/csrc/qs_policy.h): what k_policy computes, one
// environment at a time.  The fmaf chains are the kernel's bit for bit; tanhf / expf are this platform's libm, not the device's.
#include <stddef.h>
#include "../../quadruped-springs_amd/csrc/qs_policy.h"

using namespace qs::pol;

extern "C" {
// -> parameters per policy, or -1 with the reason in err
int qsepol_param_count(const qs_policy_desc* d, char* err, int err_size) {
    Net net;
    if (net_from_desc(*d, net, err, (size_t)err_size)) return -1;
    return net.n_params;
}
// params [P][n_params], obs [N][obs_dim], eps [N][A] or null, log_std [A] or null, actions [N][A], mean_out [N][A] or null, log_prob [N] or null
int qsepol_act(const qs_policy_desc* d, const float* params, const float* obs, const float* eps, const float* log_std, float* actions,
               float* mean_out, float* log_prob) {
    Net net;
    char err[256];
    if (net_from_desc(*d, net, err, sizeof(err))) return -1;
    const int n_per = d->n_envs / d->n_policies, A = net.action_dim;
    for (int i = 0; i < d->n_envs; i++)
        forward_env(net, params + (size_t)(i / n_per) * net.n_params, obs + (size_t)i * net.obs_dim, eps ? eps + (size_t)i * A : nullptr, log_std,
                    actions + (size_t)i * A, mean_out ? mean_out + (size_t)i * A : nullptr, log_prob && eps ? log_prob + i : nullptr);
    return 0;
}
// The LDS layout the host fixes for a launch (layout_sizes, waves_per_workgroup, lds_bytes of csrc/qs_policy.h): critic == null and
// row_sets == 1 as qs_policy_create calls them, critic given and row_sets == 2 as qs_ac_create does.
// out = {act_stride, w_floats, wide, waves, bytes of that launch, bytes of a one-wave launch}
int qsepol_layout(const qs_policy_desc* d, const qs_policy_desc* critic, int row_sets, int* out) {
    Net net, nc;
    char err[256];
    if (net_from_desc(*d, net, err, sizeof(err)) || (critic && net_from_desc(*critic, nc, err, sizeof(err)))) return -1;
    const Net* nets[2] = {&net, &nc};
    layout_sizes(nets, critic ? 2 : 1, out[0], out[1], out[2]);
    out[3] = waves_per_workgroup((d->n_envs / d->n_policies + TILE - 1) / TILE, d->n_policies, out[1], row_sets, out[0]);
    out[4] = (int)lds_bytes(out[1], out[3], row_sets, out[0]);
    out[5] = (int)lds_bytes(out[1], 1, row_sets, out[0]);
    return 0;
}
// this platform's tanhf (the bound of tests/test_policy_cpu.py needs its error)
void qsepol_tanh(const float* x, int n, float* y) { for (int i = 0; i < n; i++) y[i] = activate(x[i], QS_POLICY_ACT_TANH); }
}
