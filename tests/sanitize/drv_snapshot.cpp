// Stand-alone driver of csrc/qs_snapshot.h on the host (tests/test_snapshot_cpu.py builds it with -fsanitize=address,undefined): the lanes of
// k_snapshot / k_restore / k_fork_gather / k_fork one after the other on fake handle arrays of three environments in which every float is its
// own index pattern.  Usage: drv_snapshot <obs_dim>; prints "ok ..." and exits 0, or says what is wrong and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "qs_snapshot.h"

using namespace qs::snap;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float pattern(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }   // (NaN payloads and denormals among them: floats are only moved)

struct Fake {
    int n, od;
    std::vector<float> rec, push, obs, term;
    Fake(int n_, int od_, uint32_t salt) : n(n_), od(od_), rec((size_t)n_ * QS_REC), push((size_t)n_ * PUSH_F), obs((size_t)n_ * od_), term((size_t)n_ * od_) {
        for (size_t i = 0; i < rec.size(); i++) rec[i] = pattern(salt + 0x10000000u + (uint32_t)i);
        for (size_t i = 0; i < push.size(); i++) push[i] = pattern(salt + 0x20000000u + (uint32_t)i);
        for (size_t i = 0; i < obs.size(); i++) obs[i] = pattern(salt + 0x30000000u + (uint32_t)i);
        for (size_t i = 0; i < term.size(); i++) term[i] = pattern(salt + 0x7fc00000u + (uint32_t)i);   // quiet NaNs with payloads
    }
    Arrays arrays() { Arrays a; a.rec = rec.data(); a.push = push.data(); a.obs = obs.data(); a.term = term.data(); return a; }
    // the handle's float that float k of environment e's row stands for (null for the pad)
    const float* at(int e, int k) const {
        int off;
        switch (segment_of(k, od, &off)) {
        case SEG_REC: return &rec[(size_t)e * QS_REC + off];
        case SEG_PUSH: return &push[(size_t)e * PUSH_F + off];
        case SEG_OBS: return &obs[(size_t)e * od + off];
        case SEG_TERM: return &term[(size_t)e * od + off];
        default: return nullptr;
        }
    }
    size_t floats() const { return rec.size() + push.size() + obs.size() + term.size(); }
    bool same(const Fake& o) const {
        return !memcmp(rec.data(), o.rec.data(), rec.size() * 4) && !memcmp(push.data(), o.push.data(), push.size() * 4) &&
               !memcmp(obs.data(), o.obs.data(), obs.size() * 4) && !memcmp(term.data(), o.term.data(), term.size() * 4);
    }
};

int main(int argc, char** argv) {
    const int n = 3, od = argc > 1 ? atoi(argv[1]) : 27, rf = row_floats(od);
    if (od < 1 || od > MAX_OBS) { printf("obs_dim outside [1, %d]\n", MAX_OBS); return 1; }
    CHECK(rf % 4 == 0 && rf >= used_floats(od) && rf - used_floats(od) < 4, "row_floats %d", rf);

    // ---- snapshot: every float of a row is one float of the handle, every float of the handle is in exactly one place of its row
    Fake h(n, od, 0);
    const Fake h0 = h;
    std::vector<float> rows((size_t)n * rf, pattern(0xdeadbeefu));
    const uint8_t mask[3] = {1, 0, 1};
    host_snapshot(h.arrays(), n, od, mask, rows.data());
    CHECK(h.same(h0), "a snapshot changed the handle");
    size_t covered = 0;
    std::vector<uint32_t> seen;
    for (int e = 0; e < n; e++)
        for (int k = 0; k < rf; k++) {
            const float got = rows[(size_t)e * rf + k];
            if (!mask[e]) { CHECK(bits(got) == 0xdeadbeefu, "unmasked row %d float %d was written", e, k); continue; }
            const float* want = h.at(e, k);
            if (!want) { CHECK(bits(got) == 0u, "pad float %d of row %d is %08x", k, e, bits(got)); continue; }
            CHECK(bits(got) == bits(*want), "row %d float %d: %08x, the handle holds %08x", e, k, bits(got), bits(*want));
            seen.push_back(bits(got)); covered++;
        }
    CHECK(covered == h.floats() / n * 2, "%zu floats in two rows, the handle has %zu per environment", covered, h.floats() / n);
    {   // (the patterns are all different: equal counts + no duplicates = every handle float exactly once)
        std::vector<uint32_t> s = seen;
        qsort(s.data(), s.size(), 4, [](const void* a, const void* b) { const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b; return x < y ? -1 : x > y; });
        for (size_t i = 1; i < s.size(); i++) CHECK(s[i] != s[i - 1], "pattern %08x sits in two places", s[i]);
    }

    // ---- scramble, restore: the masked environments come back bit for bit, the other one stays scrambled
    host_snapshot(h.arrays(), n, od, nullptr, rows.data());
    Fake scr(n, od, 0x01000000u);
    h = scr;
    host_restore(h.arrays(), n, od, mask, rows.data());
    for (int e = 0; e < n; e++)
        for (int k = 0; k < used_floats(od); k++) {
            const Fake& want = mask[e] ? h0 : scr;
            CHECK(bits(*h.at(e, k)) == bits(*want.at(e, k)), "restore, environment %d float %d", e, k);
        }
    host_restore(h.arrays(), n, od, nullptr, rows.data());
    CHECK(h.same(h0), "a full restore does not give the handle back");

    // ---- fork: a chain (0 <- 1 while 1 <- 2) and, in a second call, a swap (0 <-> 2 with 1 left alone by -1): pre-call sources, everything
    // but the two kept fields
    std::vector<float> staging((size_t)n * rf, 0.0f);
    auto check_fork = [&](const Fake& before, const Fake& after, const int32_t* src_of, const char* what) {
        for (int i = 0; i < n; i++) {
            const bool takes = fork_takes(i, src_of[i], n);
            int kept = 0;
            for (int k = 0; k < used_floats(od); k++) {
                int off;
                const bool keeps = segment_of(k, od, &off) == SEG_REC && fork_keeps(off);
                kept += keeps;
                const int from = takes && !keeps ? src_of[i] : i;
                CHECK(bits(*after.at(i, k)) == bits(*before.at(from, k)), "%s: environment %d float %d is not environment %d's pre-call value", what, i, k, from);
            }
            CHECK(kept == 2, "%d kept fields", kept);
        }
    };
    {
        const int32_t chain[3] = {1, 2, 2};
        const Fake before = h;
        CHECK(host_fork(h.arrays(), n, od, chain, staging.data()) == 0, "chain refused");
        check_fork(before, h, chain, "chain");
        CHECK(bits(h.rec[R_EPISODE]) == bits(h0.rec[R_EPISODE]) && bits(h.rec[R_TOTAL_STEPS]) == bits(h0.rec[R_TOTAL_STEPS]), "environment 0 lost its identity");
    }
    {
        const int32_t swap[3] = {2, -1, 0};
        const Fake before = h;
        CHECK(host_fork(h.arrays(), n, od, swap, staging.data()) == 0, "swap refused");
        check_fork(before, h, swap, "swap");
    }
    {   // a source out of range: that environment is left alone and named, the others are served
        const int32_t bad[3] = {1, 3, -2};
        const Fake before = h;
        CHECK(host_fork(h.arrays(), n, od, bad, staging.data()) == 2, "the first refused environment is 1");
        const int32_t served[3] = {1, -1, -1};
        check_fork(before, h, served, "refused");
    }
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok obs_dim %d row_floats %d\n", od, rf);
    return 0;
}
