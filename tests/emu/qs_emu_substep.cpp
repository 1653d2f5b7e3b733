// qs_emu_substep.cpp -- TEST-ONLY host twin of tests/hip/substep_probe.hip: ONE physics substep of every build of Sim that the probe holds
// (pyramid and cone, each full and common-path; cone common-path with the payload block's rows), on records handed in, with the 4-wide
// LaneEmu type.  A library of its own: the emulation tests that need the plain full builds only do not pay for compiling these.
// With LaneEmu the "wave" is one environment's quad: each environment decides its own give-up (the GPU decides it for 16).
#include "qs_emu.h"

template <class EV> static void substep_all(const qs_config& cfg, int n, float* recs, const float* tau12, const float* push, int32_t* rc) {
    for (int i = 0; i < n; i++) {
        float* rec = recs + (size_t)i * QS_REC;
        typename EV::S::State s; typename EV::S::Par P; typename EV::S::Out o;
        EV::load_state(rec, s); EV::load_par(cfg, rec, P);
        V4 tau[3];
        for (int j = 0; j < 3; j++) {
            tau[j] = LaneEmu::ld_leg(tau12 + (size_t)i * 12, j, 3);
            o.tau_pd[j] = LaneEmu::ld_leg(rec, R_TAU_PD + j, 3); o.tau_spring[j] = LaneEmu::ld_leg(rec, R_TAU_SPRING + j, 3);
        }
        o.foot_force = LaneEmu::ld_leg(rec, R_FOOT_FORCE, 1); o.foot_contact = LaneEmu::ld_leg(rec, R_FOOT_CONTACT, 1); o.n_invalid = LaneEmu::ld(rec, R_N_INVALID);
        rc[i] = EV::S::substep(cfg, P, s, tau, o, true, cfg.payload_soft ? rec + R_BLOCK : nullptr, nullptr, true, push ? push + (size_t)i * 8 : nullptr, 0);
        EV::store_state(rec, s, o);
    }
}

extern "C" {
// the arguments of qsp_substep (tests/hip/substep_probe.hip); recs [n][QS_REC] are advanced in place.  -1: a build the probe does not hold
int qse_substep(const qs_config* cfg, int n_envs, int build, float* recs, const float* tau, const float* push, int32_t* rc) {
    if (!cfg || n_envs <= 0 || build < 0 || build > 2 || !recs || !tau || !rc) return -1;
    if (build == 2 && !(cfg->friction_cone && cfg->payload_soft)) return -1;
    QsDevCfg dc;     // (the configuration sits where the kernels' is: qs_emu.h)
    memset(&dc, 0, sizeof(dc));
    dc.cfg = *cfg; dc.rack_pos[2] = 1.0f; dc.rack_quat[3] = 1.0f;
    const qs_config& c = dc.cfg;
    if (c.friction_cone) {
        if (build == 0) substep_all<qs::Env<LaneEmu, true, false, false>>(c, n_envs, recs, tau, push, rc);
        else if (build == 1) substep_all<qs::Env<LaneEmu, true, true, false>>(c, n_envs, recs, tau, push, rc);
        else substep_all<qs::Env<LaneEmu, true, true, true>>(c, n_envs, recs, tau, push, rc);
    } else {
        if (build == 0) substep_all<qs::Env<LaneEmu, false, false, false>>(c, n_envs, recs, tau, push, rc);
        else substep_all<qs::Env<LaneEmu, false, true, false>>(c, n_envs, recs, tau, push, rc);
    }
    return 0;
}
}
