// qs_emu_push.cpp -- TEST-ONLY host emulation of a step with external pushes (qs_set_external_wrench): what step_body does with the
// handle's push rows -- each environment's row goes to its env step, which applies it on the substeps k < remaining, and the row counts
// down behind the step (0 once the episode ended) -- through the full build alone, or through the common-path build and its hand-over to
// the full build as k_step / k_step_dense run them.  Works on a handle of qs_emu.cpp, like qs_emu_hot.cpp.
#include "qs_emu.h"

namespace {

struct Result { float reward, done, trunc; int resume; };

template <bool CONE, bool SOFT, bool LEAN>
Result hot_step(const qs_config& cfg, float* rec, const float* act, float* ob, uint32_t gid, const float* push) {
    using EF = qs::Env<LaneEmu, CONE>;
    using EH = qs::Env<LaneEmu, CONE, true, SOFT>;
    const typename EH::StepOut rh = EH::template step<false, LEAN>(cfg, rec, act, ob, gid, 0, nullptr, false, nullptr, 0, 0, push);
    Result r = {rh.reward.v[0], rh.done.v[0], rh.trunc.v[0], rh.resume};
    if (rh.resume >= 0) {
        const typename EF::StepOut rf = EF::template step<true>(cfg, rec, act, ob, gid, 0, nullptr, false, nullptr, 0, rh.resume, push);
        r.reward = rf.reward.v[0]; r.done = rf.done.v[0]; r.trunc = rf.trunc.v[0];
    }
    return r;
}

template <bool LEAN> Result pick(const qs_config& cfg, float* rec, const float* act, float* ob, uint32_t gid, const float* push) {
    if (cfg.friction_cone && cfg.payload_soft) return hot_step<true, true, LEAN>(cfg, rec, act, ob, gid, push);
    if (cfg.friction_cone) return hot_step<true, false, LEAN>(cfg, rec, act, ob, gid, push);
    return hot_step<false, false, LEAN>(cfg, rec, act, ob, gid, push);
}

template <class EV> Result full_step(const qs_config& cfg, float* rec, const float* act, float* ob, uint32_t gid, const float* push) {
    const typename EV::StepOut r = EV::step(cfg, rec, act, ob, gid, 0, nullptr, false, nullptr, 0, 0, push);
    return Result{r.reward.v[0], r.done.v[0], r.trunc.v[0], -1};
}

}  // namespace

extern "C" {
// One env step of every environment with push rows push[N][8] (force 3, torque 3, remaining substeps, frame; updated in place as the
// kernel updates d_push).  variant 0 = the full build, 1 / 2 = the builds of k_step / k_step_dense with their hand-over.  resume as in
// qse_step_hot (-1 for the full build).
int qsep_step(void* h, const float* actions, float* push, int variant, float* obs, float* rew, uint8_t* done, uint8_t* trunc, int32_t* resume) {
    Emu* e = (Emu*)h;
    if (variant < 0 || variant > 2) return -1;
    const int d = e->cfg.action_dim;
    for (int i = 0; i < e->cfg.n_envs; i++) {
        float* rec = &e->rec[(size_t)i * QS_REC];
        float* ob = &e->obs[(size_t)i * QS_MAX_OBS];
        float* row = push + (size_t)i * 8;
        const float rem = row[6];
        const float* p = rem > 0.0f ? row : nullptr;
        const float* act = actions + (size_t)i * d;
        const uint32_t gid = (uint32_t)(i + e->cfg.env_id_offset);
        Result r;
        if (variant == 0) r = e->cfg.friction_cone ? full_step<EC>(e->cfg, rec, act, ob, gid, p) : full_step<E>(e->cfg, rec, act, ob, gid, p);
        else if (variant == 2) r = pick<true>(e->cfg, rec, act, ob, gid, p);
        else r = pick<false>(e->cfg, rec, act, ob, gid, p);
        resume[i] = r.resume;
        if (rem > 0.0f) row[6] = r.done > 0.5f ? 0.0f : fmaxf(rem - (float)e->cfg.action_repeat, 0.0f);
        finish_env_step(e, i, r.reward, r.done, r.trunc, obs, rew, done, trunc);
    }
    return 0;
}
}
