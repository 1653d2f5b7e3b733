// qs_emu_step.cpp -- TEST-ONLY host emulation of the env step as the step kernels run it (qs_hip.hip step_body): the handle's builds chosen
// by qs::with_build as launch_step chooses its kernel -- the common-path ("HOT") builds, plain, with the payload block's rows or with the
// rack's, the full builds behind them --, the step run by qs::step_hand_over as step_body runs it, the push row counted down behind it.
// Works on a handle of qs_emu.cpp; a library of its own so that the emulation tests that need the plain full builds only do not pay for
// compiling these.  With LaneEmu the "wave" is one environment's quad: each environment decides its own hand-over (the GPU decides it
// for 16).
#include "qs_emu.h"

extern "C" {
// One env step of every environment -- or, settle_n > 0, one slice of a reset's settle as a settle lane runs it: with `spawn` the record
// first gets the randomizer draws and spawn state of the next episode (the first slice), then settle_n substeps under the settling command
// and no outputs.
// variant as QS_STEP_VARIANT: 1 = k_step (parameters in registers), 2 = k_step_dense (LEAN: parameters reloaded from LDS), each with its
// hand-over; 0 = the full build alone.  push: null, or rows [N][8] of qs_set_external_wrench (force 3, torque 3, remaining substeps, frame),
// updated in place as the kernel updates d_push.  resume[i] = what the common-path build returned (-1: not handed over, and always for
// variant 0; else the substep, + RESUME_AT_BOUNDARY for a hand-over between two substeps).
int qse_step_build(void* h, int variant, const float* actions, float* push, int settle_n, int spawn, float* obs, float* rew, uint8_t* done, uint8_t* trunc,
                   int32_t* resume) {
    Emu* e = (Emu*)h;
    const qs_config& cfg = e->dc.cfg;
    if (variant < 0 || variant > 2 || settle_n < 0) return -1;
    static const float no_action[12] = {0};
    qs::with_build(qs::Build::of(cfg, e->rack), [&](auto cone, auto soft, auto rack) {
        using EF = qs::Env<LaneEmu, cone(), false, false, rack()>;
        for (int i = 0; i < cfg.n_envs; i++) {
            float* rec = e->record(i);
            float* ob = e->obs_row(i);
            const float* act = settle_n > 0 ? no_action : actions + (size_t)i * cfg.action_dim;
            float* tr = (e->trace && i == e->trace_env && settle_n == 0) ? e->trace : nullptr;
            float* row = push ? push + (size_t)i * 8 : nullptr;
            const float rem = row ? row[6] : 0.0f;
            const float* p = rem > 0.0f ? row : nullptr;
            if (spawn) EF::settle_spawn(cfg, rec, e->gid(i), qs::f2i(rec[R_EPISODE]) + 1);
            typename EF::StepOut r;
            if (variant == 0) { r = EF::step(cfg, rec, act, ob, e->gid(i), settle_n, tr, tr != nullptr, e->demo.data(), e->demo_len, 0, p); r.resume = -1; }
            else if (variant == 2) r = qs::step_hand_over<LaneEmu, cone(), soft(), rack(), true>(cfg, rec, act, ob, e->gid(i), settle_n, tr, tr != nullptr, e->demo.data(), e->demo_len, p);
            else r = qs::step_hand_over<LaneEmu, cone(), soft(), rack(), false>(cfg, rec, act, ob, e->gid(i), settle_n, tr, tr != nullptr, e->demo.data(), e->demo_len, p);
            resume[i] = r.resume;
            if (settle_n > 0) continue;
            // the push counts down by the step's substeps; an episode that ended cancels it
            if (rem > 0.0f) row[6] = r.done.v[0] > 0.5f ? 0.0f : fmaxf(rem - (float)cfg.action_repeat, 0.0f);
            finish_env_step<EF>(e, i, r, obs, rew, done, trunc);
        }
    });
    return 0;
}
// qse_reset / qse_reset_to in the handle's full build, RACK included (k_reset_rack: the robot spawns at the anchor, or is put at the given
// state, and is hung)
int qse_reset_build(void* h, const uint8_t* mask, const float* states) {
    Emu* e = (Emu*)h;
    qs::with_build(qs::Build::of(e->dc.cfg, e->rack), [&](auto cone, auto, auto rack) { reset_envs<qs::Env<LaneEmu, cone(), false, false, rack()>>(e, mask, states); });
    return 0;
}
}
