// drv_ars.cpp -- stand-alone driver (its own main) that runs the host build of ARS's bookkeeping (csrc/qs_ars.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, lane after lane, over the shapes of tests/test_gpu_ars.py: m in {1, 3, 64, 65, 130}, n_delta in {1, 2, 5, 64, 65,
// 1024}, n_top in {1, a middle value, n_delta}, n_params in {1, 168, 255, 256, 257, 6406}; every array allocated at exactly its size.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../quadruped-springs_amd/csrc/qs_ars.h"

namespace ars = qs::ars;

static unsigned long long g_state = 88172645463325252ULL;
static float uniform() {   // xorshift64, in [-1, 1)
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (float)((double)(g_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

static int run(int m, int n_delta, int n_top, int n_params, int episodes_per_env) {
    const int P = 2 * n_delta, N = P * m, T = 12;
    char err[512];
    if (ars::check_shape(N, n_delta, n_params, episodes_per_env, err, sizeof(err))) { fprintf(stderr, "check_shape: %s\n", err); return 1; }
    std::vector<float> theta(n_params), delta((size_t)n_delta * n_params), cand((size_t)P * n_params);
    for (auto& x : theta) x = 0.1f * uniform();
    for (auto& x : delta) x = 2.0f * uniform();
    ars::perturb_host(theta.data(), delta.data(), n_delta, n_params, 0.05f, cand.data());
    std::vector<float> ret(N), raw(N), R(P), w(n_top), stats(2);
    std::vector<int> len(N), episodes(N), idx(n_top);
    std::vector<uint8_t> alive(N), done(N);
    int n_alive = -1;
    ars::begin_host(ret.data(), len.data(), episodes.data(), alive.data(), N, &n_alive);
    if (n_alive != N) { fprintf(stderr, "n_alive %d after begin, expected %d\n", n_alive, N); return 1; }
    for (int t = 0; t < T; t++) {
        for (int e = 0; e < N; e++) { raw[e] = uniform(); done[e] = (uint8_t)(uniform() > 0.6f); }
        ars::account_host(ret.data(), len.data(), episodes.data(), alive.data(), raw.data(), done.data(), N, episodes_per_env, &n_alive);
        int count = 0;
        for (int e = 0; e < N; e++) count += alive[e];
        if (count != n_alive) { fprintf(stderr, "n_alive %d, %d flags set\n", n_alive, count); return 1; }
    }
    long long total = 0;
    for (int e = 0; e < N; e++) total += len[e];
    if (ars::returns_host(ret.data(), len.data(), N, n_delta, 0.25f, R.data()) != total) { fprintf(stderr, "the step sum is off\n"); return 1; }
    if (n_delta >= 4) { R[1] = R[0]; R[n_delta + 1] = R[n_delta]; R[3] = R[0]; R[n_delta + 3] = R[n_delta]; }   // ties
    ars::select_host(R.data(), n_delta, n_top, 0.02f, idx.data(), w.data(), stats.data());
    std::vector<char> seen(n_delta, 0);
    for (int r = 0; r < n_top; r++) {
        if (idx[r] < 0 || idx[r] >= n_delta || seen[idx[r]]) { fprintf(stderr, "idx[%d] = %d\n", r, idx[r]); return 1; }
        seen[idx[r]] = 1;
    }
    if (!(stats[0] >= 0.0f) || !(stats[1] > 0.0f)) { fprintf(stderr, "std %g, step %g\n", stats[0], stats[1]); return 1; }
    ars::apply_host(theta.data(), delta.data(), n_params, idx.data(), w.data(), n_top, stats[1]);
    for (int i = 0; i < n_params; i++)
        if (!(theta[i] == theta[i])) { fprintf(stderr, "theta[%d] is not a number\n", i); return 1; }
    return 0;
}

int main() {
    const int ms[5] = {1, 3, 64, 65, 130}, deltas[6] = {1, 2, 5, 64, 65, 1024}, params[6] = {1, 168, 255, 256, 257, 6406};
    for (int a = 0; a < 5; a++)
        for (int d = 0; d < 6; d++) {
            const int n_delta = deltas[d], tops[3] = {1, (n_delta + 1) / 2, n_delta};
            if (n_delta == 1024 && ms[a] > 3) continue;                    // (the selection does not depend on m; 266240 environments add nothing)
            for (int t = 0; t < 3; t++)
                if (run(ms[a], n_delta, tops[t], params[(a + d + t) % 6], 1 + (a + d) % 2)) return 1;
        }
    printf("ok\n");
    return 0;
}
