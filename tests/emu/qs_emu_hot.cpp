// qs_emu_hot.cpp -- TEST-ONLY host emulation of the step kernels' hand-over: the common-path ("HOT") builds of Env::step that
// k_step / k_step_dense launch, and behind them the full build's step<true>(..., resume) from the substep where a common-path build
// gave up (qs_hip.hip step_body).  Works on a handle of qs_emu.cpp; a separate translation unit (and library) so that the emulation
// tests that do not need these builds do not pay for compiling them.
// With LaneEmu the "wave" is one environment's quad: each environment decides its own hand-over (the GPU decides it for 16).
#include "qs_emu.h"

namespace {

struct Result { float reward, done, trunc; int resume; };

// step_body's env step of one record: the common-path build, then (resume >= 0) the full build from where it gave up
template <bool CONE, bool SOFT, bool LEAN>
Result hot_step(const qs_config& cfg, float* rec, const float* act, float* ob, uint32_t gid, int settle_n, float* tr, const float* demo, int demo_len) {
    using EF = qs::Env<LaneEmu, CONE>;
    using EH = qs::Env<LaneEmu, CONE, true, SOFT>;
    const typename EH::StepOut rh = EH::template step<false, LEAN>(cfg, rec, act, ob, gid, settle_n, tr, tr != nullptr, demo, demo_len);
    Result r = {rh.reward.v[0], rh.done.v[0], rh.trunc.v[0], rh.resume};
    if (rh.resume >= 0) {
        const typename EF::StepOut rf = EF::template step<true>(cfg, rec, act, ob, gid, settle_n, tr, tr != nullptr, demo, demo_len, rh.resume);
        r.reward = rf.reward.v[0]; r.done = rf.done.v[0]; r.trunc = rf.trunc.v[0];
    }
    return r;
}

// the builds qs_step launches (QS_PICK): the pyramid + payload_soft handle runs the pyramid's weld build, whose first substep hands over
template <bool LEAN>
Result pick(const qs_config& cfg, float* rec, const float* act, float* ob, uint32_t gid, int settle_n, float* tr, const float* demo, int demo_len) {
    if (cfg.friction_cone && cfg.payload_soft) return hot_step<true, true, LEAN>(cfg, rec, act, ob, gid, settle_n, tr, demo, demo_len);
    if (cfg.friction_cone) return hot_step<true, false, LEAN>(cfg, rec, act, ob, gid, settle_n, tr, demo, demo_len);
    return hot_step<false, false, LEAN>(cfg, rec, act, ob, gid, settle_n, tr, demo, demo_len);
}

// variant as QS_STEP_VARIANT: 1 = k_step (parameters in registers), 2 = k_step_dense (LEAN: parameters reloaded from LDS)
Result step_env(const Emu* e, int variant, float* rec, const float* act, float* ob, uint32_t gid, int settle_n, float* tr) {
    if (variant == 2) return pick<true>(e->cfg, rec, act, ob, gid, settle_n, tr, e->demo.data(), e->demo_len);
    return pick<false>(e->cfg, rec, act, ob, gid, settle_n, tr, e->demo.data(), e->demo_len);
}

}  // namespace

extern "C" {
// qse_step through the step kernel's builds; resume[i] = what the common-path build returned (-1: not handed over; else the substep,
// + RESUME_AT_BOUNDARY for a hand-over between two substeps)
int qse_step_hot(void* h, const float* actions, float* obs, float* rew, uint8_t* done, uint8_t* trunc, int variant, int32_t* resume) {
    Emu* e = (Emu*)h;
    if (variant != 1 && variant != 2) return -1;
    const int d = e->cfg.action_dim;
    for (int i = 0; i < e->cfg.n_envs; i++) {
        float* rec = &e->rec[(size_t)i * QS_REC];
        float* ob = &e->obs[(size_t)i * QS_MAX_OBS];
        float* tr = (e->trace && i == e->trace_env) ? e->trace : nullptr;
        const Result r = step_env(e, variant, rec, actions + (size_t)i * d, ob, (uint32_t)(i + e->cfg.env_id_offset), 0, tr);
        resume[i] = r.resume;
        finish_env_step(e, i, r.reward, r.done, r.trunc, obs, rew, done, trunc);
    }
    return 0;
}
int qse_resume_at_boundary(void) { return (int)E::RESUME_AT_BOUNDARY; }
// One slice of a reset's settle as a settle lane runs it (qs_hip.hip step_body with settle_n > 0): with `spawn` the record first gets the
// randomizer draws and spawn state of the next episode (the first slice); then settle_n substeps under the settling command.  variant 0 =
// the full build's step<false>, 1 / 2 = the step kernels' builds with their hand-over (resume as in qse_step_hot).
int qse_settle_slice(void* h, int settle_n, int spawn, int variant, int32_t* resume) {
    Emu* e = (Emu*)h;
    if (settle_n <= 0 || variant < 0 || variant > 2) return -1;
    static const float no_action[12] = {0};
    for (int i = 0; i < e->cfg.n_envs; i++) {
        float* rec = &e->rec[(size_t)i * QS_REC];
        float* ob = &e->obs[(size_t)i * QS_MAX_OBS];
        const uint32_t gid = (uint32_t)(i + e->cfg.env_id_offset);
        const int episode = qs::f2i(rec[R_EPISODE]) + 1;
        if (spawn) {
            if (e->cfg.friction_cone) EC::settle_spawn(e->cfg, rec, gid, episode);
            else E::settle_spawn(e->cfg, rec, gid, episode);
        }
        if (variant == 0) {
            if (e->cfg.friction_cone) EC::step(e->cfg, rec, no_action, ob, gid, settle_n);
            else E::step(e->cfg, rec, no_action, ob, gid, settle_n);
            resume[i] = -1;
        } else {
            resume[i] = step_env(e, variant, rec, no_action, ob, gid, settle_n, nullptr).resume;
        }
    }
    return 0;
}
}
