// drv_mpc.cpp -- stand-alone driver (its own main) that runs the host build of the sampling planner (csrc/qs_mpc.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, lane after lane, over the shapes of tests/mpc_ref.py -- (M, C, H, d) = (1, 1, 1, 6), (3, 5, 3, 6), (2, 64, 2, 12),
// (2, 70, 4, 6), (5, 130, 2, 6), (1, 4096, 1, 6), (2, 3, 170, 6) -- under both methods, with and without a mask, with non-finite scores; every
// array allocated at exactly its size.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../quadruped-springs_amd/csrc/qs_mpc.h"

namespace mpc = qs::mpc;

static unsigned long long g_state = 88172645463325252ULL;
static float uniform() {   // xorshift64, in [-1, 1)
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (float)((double)(g_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

static int run(int M, int C, int H, int d, int method, bool with_mask, bool poison) {
    char err[512];
    if (mpc::check_shape(M, C, H, d, err, sizeof(err))) { fprintf(stderr, "check_shape: %s\n", err); return 1; }
    const size_t MC = (size_t)M * C, N = (size_t)M + MC, stride = 2;
    std::vector<float> plan((size_t)M * H * d), eps(MC * H * d), seq(MC * H * d), score(MC), reward(N), reward_end(N * stride - 1), actions(N * d), best_score(M);
    std::vector<uint8_t> running(MC), done(N), active(with_mask ? N : 0);
    std::vector<int> best(M);
    for (auto& x : plan) x = uniform();
    for (auto& x : eps) x = 3.0f * uniform();
    for (auto& x : reward_end) x = 5.0f * uniform();
    mpc::set_plan_host(plan.data(), nullptr, nullptr, M, H, d);
    for (auto& x : plan) x = uniform();
    mpc::sample_host(plan.data(), eps.data(), M, C, H, d, 0.5f, seq.data(), score.data(), running.data());
    for (size_t k = 0; k < seq.size(); k++)
        if (!(seq[k] >= -1.0f && seq[k] <= 1.0f)) { fprintf(stderr, "seq[%zu] = %g\n", k, seq[k]); return 1; }
    for (int h = 0; h <= H; h++) {
        for (size_t e = 0; e < N; e++) { reward[e] = 10.0f * uniform(); done[e] = (uint8_t)(uniform() > 0.7f); }
        if (poison && h == 1) { reward[M] = mpc::from_bits(mpc::MINUS_INF_BITS); reward[N - 1] = mpc::from_bits(0x7f800000u); if (MC > 2) reward[M + 1] = mpc::from_bits(0x7fc00000u); }
        mpc::feed_host(h, seq.data(), score.data(), running.data(), M, C, H, d, h ? reward.data() : nullptr, h ? done.data() : nullptr,
                       h == H ? reward_end.data() : nullptr, (int)stride, actions.data(), with_mask ? active.data() : nullptr);
        if (with_mask)
            for (size_t i = 0; i < MC; i++)
                if (active[M + i] != running[i]) { fprintf(stderr, "active[%zu] differs from running\n", M + i); return 1; }
    }
    mpc::finish_host(seq.data(), score.data(), M, C, H, d, method, 0.3f, plan.data(), actions.data(), best.data(), best_score.data());
    for (int m = 0; m < M; m++)
        if (best[m] < 0 || best[m] >= C) { fprintf(stderr, "best[%d] = %d\n", m, best[m]); return 1; }
    for (size_t k = 0; k < plan.size(); k++)
        if (!(plan[k] >= -1.0f && plan[k] <= 1.0f)) { fprintf(stderr, "plan[%zu] = %g\n", k, plan[k]); return 1; }
    for (size_t k = 0; k < (size_t)M * d; k++)
        if (!(actions[k] >= -1.0f && actions[k] <= 1.0f)) { fprintf(stderr, "actions[%zu] = %g\n", k, actions[k]); return 1; }
    return 0;
}

int main() {
    const int shapes[7][4] = {{1, 1, 1, 6}, {3, 5, 3, 6}, {2, 64, 2, 12}, {2, 70, 4, 6}, {5, 130, 2, 6}, {1, 4096, 1, 6}, {2, 3, 170, 6}};
    for (int s = 0; s < 7; s++)
        for (int method = 0; method < 2; method++)
            for (int variant = 0; variant < 4; variant++)
                if (run(shapes[s][0], shapes[s][1], shapes[s][2], shapes[s][3], method, (variant & 1) != 0, (variant & 2) != 0)) return 1;
    for (float x = 0.0f; x > -110.0f; x -= 0.37f) {
        const float y = mpc::exp_nonpos(x);
        if (!(y >= 0.0f && y <= 1.0f)) { fprintf(stderr, "exp_nonpos(%g) = %g\n", x, y); return 1; }
    }
    if (mpc::exp_nonpos(mpc::from_bits(mpc::MINUS_INF_BITS)) != 0.0f) { fprintf(stderr, "exp_nonpos(-inf)\n"); return 1; }
    printf("ok\n");
    return 0;
}
