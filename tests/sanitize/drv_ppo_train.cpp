// drv_ppo_train.cpp -- stand-alone driver (its own main) that runs the host build of the PPO update (csrc/qs_ppo_train.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer: the four networks of tests/ppo_train_ref.py x B in {1, 17, 1000}, every array allocated at
// exactly its size, the index vector holding indices outside [0, total) that must be counted and never read; then three Adam steps.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../quadruped-springs_amd/csrc/qs_ppo_train.h"

using namespace qs::pol;
namespace train = qs::train;

static unsigned long long g_state = 88172645463325252ULL;
static float uniform() {   // xorshift64, in [-1, 1)
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (float)((double)(g_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}
static std::vector<float> noise(size_t n, float scale) { std::vector<float> v(n); for (size_t i = 0; i < n; i++) v[i] = scale * uniform(); return v; }

static qs_policy_desc desc(int obs, int out, int n_hidden, const int* hidden, int act) {
    qs_policy_desc d;
    memset(&d, 0, sizeof(d));
    d.n_envs = 16; d.n_policies = 1; d.obs_dim = obs; d.action_dim = out; d.n_hidden = n_hidden;
    for (int l = 0; l < n_hidden; l++) d.hidden[l] = hidden[l];
    d.activation = act; d.has_bias = 1; d.clip_lo = -3.0e38f; d.clip_hi = 3.0e38f;
    return d;
}

static int run(const qs_policy_desc& da, const qs_policy_desc& dc, int B) {
    Net na, nc;
    char err[512];
    if (train::check_train(da, dc, na, nc, err, sizeof(err))) { fprintf(stderr, "check_train: %s\n", err); return 1; }
    const int A = na.action_dim, n_total = train::total_params(na, nc);
    const long long total = B + 5;
    std::vector<float> pa = noise(na.n_params, 0.2f), pc = noise(nc.n_params, 0.2f), ls = noise(A, 0.3f);
    std::vector<float> obs = noise((size_t)total * na.obs_dim, 1.5f), act = noise((size_t)total * A, 1.0f), old_lp = noise(total, 0.15f), adv = noise(total, 2.0f), ret = noise(total, 1.0f);
    for (long long i = 0; i < total; i++) old_lp[i] -= 0.9f * A;
    std::vector<long long> idx(B);
    for (int s = 0; s < B; s++) idx[s] = (long long)((s * 7919LL + 3) % total);
    int bad = 0;
    const long long outside[4] = {-1, total, (1LL << 40), -(1LL << 62)};
    for (int k = 0; k < 4 && k * 5 < B; k++) { idx[k * 5] = outside[k]; bad++; }
    qs_ppo_hyper hy;
    memset(&hy, 0, sizeof(hy));
    hy.clip_range = 0.2f; hy.ent_coef = 0.01f; hy.vf_coef = 0.5f; hy.max_grad_norm = 0.5f; hy.normalize_advantage = 1;
    hy.lr = 3e-4; hy.beta_one = 0.9; hy.beta_two = 0.999; hy.adam_eps = 1e-5;
    std::vector<float> grad(n_total), stats(QS_PPO_N_STATS), p(n_total), m(n_total, 0.0f), v(n_total, 0.0f);
    const int refused = train::grad_host(na, nc, pa.data(), pc.data(), ls.data(), obs.data(), act.data(), old_lp.data(), adv.data(), ret.data(), total, idx.data(), B, hy,
                                         grad.data(), stats.data());
    if (refused != bad || stats[QS_PPO_STAT_REFUSED] != (float)bad) { fprintf(stderr, "refused %d, expected %d\n", refused, bad); return 1; }
    for (int i = 0; i < n_total; i++)
        if (!(grad[i] == grad[i])) { fprintf(stderr, "grad[%d] is not a number\n", i); return 1; }
    memcpy(p.data(), pa.data(), sizeof(float) * na.n_params);
    memcpy(p.data() + na.n_params, pc.data(), sizeof(float) * nc.n_params);
    memcpy(p.data() + na.n_params + nc.n_params, ls.data(), sizeof(float) * A);
    for (int step = 1; step <= 3; step++)
        if (!(train::adam_host(p.data(), m.data(), v.data(), grad.data(), n_total, hy, step) >= 0.0f)) { fprintf(stderr, "norm is not a number\n"); return 1; }
    return 0;
}

int main() {
    const int h6464[2] = {64, 64}, h337[2] = {33, 7}, h16[1] = {16}, h64[1] = {64};
    const qs_policy_desc pairs[4][2] = {
        {desc(28, 6, 2, h6464, QS_POLICY_ACT_TANH), desc(28, 1, 2, h6464, QS_POLICY_ACT_TANH)},
        {desc(30, 5, 2, h337, QS_POLICY_ACT_RELU), desc(30, 1, 1, h16, QS_POLICY_ACT_RELU)},
        {desc(28, 12, 0, h16, QS_POLICY_ACT_NONE), desc(28, 1, 0, h16, QS_POLICY_ACT_NONE)},
        {desc(64, 64, 1, h64, QS_POLICY_ACT_TANH), desc(64, 1, 1, h64, QS_POLICY_ACT_TANH)},
    };
    const int batches[3] = {1, 17, 1000};
    for (int n = 0; n < 4; n++)
        for (int b = 0; b < 3; b++)
            if (run(pairs[n][0], pairs[n][1], batches[b])) return 1;
    printf("ok\n");
    return 0;
}
