// qs_emu.h -- TEST-ONLY: what the two libraries of the host emulation share (qs_emu.cpp: the handle and the plain full builds of the env
// step; qs_emu_step.cpp: every build the step kernels run, selected and handed over as qs_hip.hip does it).  Both work on the same handle.
// Each library is ONE translation unit: the capture buffer and its entry points below exist once per library.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <vector>
// the many-rows solve's inputs, captured while steps run (qse_rare_capture; tests/test_rare_solver.py): qs_rare.h's emulation twin calls
// QS_RARE_CAPTURE with them, a no-op unless defined before the kernel headers
template <class V, class R, class P> static void rare_capture(const V& mu, const R* xr, const P* pay, const V& warm);
#define QS_RARE_CAPTURE(cfg, mu, xr, pay, mine, warm) rare_capture(mu, xr, pay, warm)
#include "../../quadruped-springs_amd/csrc/qs_env.h"

using E = qs::Env<LaneEmu>;            // friction pyramid
using EC = qs::Env<LaneEmu, true>;     // implicit cone (cfg.friction_cone): the kernels are built for both, so is this harness

// The configuration sits where the kernels' is: first member of a QsDevCfg (the RACK builds read the anchor behind it, qs_env.h
// spawn_pose; `counters` stays null, LaneEmu counts nothing).  Every Env call gets e->dc.cfg.
struct Emu {
    QsDevCfg dc;
    bool rack = false;      // qse_rack: the handle runs the RACK builds (qs_emu_step.cpp; qs_emu.cpp holds none and refuses)
    std::vector<float> rec, obs, term_obs;
    float* trace = nullptr; int trace_env = -1;
    std::vector<float> demo; int demo_len = 0;
    float* record(int i) { return &rec[(size_t)i * QS_REC]; }
    float* obs_row(int i) { return &obs[(size_t)i * QS_MAX_OBS]; }
    uint32_t gid(int i) const { return (uint32_t)(i + dc.cfg.env_id_offset); }
};

// what a step entry does with environment i's step result (the step wrote its observation into the staging row): outputs, and under
// cfg.auto_reset the terminal observation and the reset of a finished environment (k_step's auto-reset with reset_lookahead = 0).
// EV: the handle's full build
template <class EV> static void finish_env_step(Emu* e, int i, const typename EV::StepOut& r, float* obs, float* rew, uint8_t* done, uint8_t* trunc) {
    const qs_config& cfg = e->dc.cfg;
    float* ob = e->obs_row(i);
    rew[i] = r.reward.v[0]; done[i] = r.done.v[0] > 0.5f; trunc[i] = r.trunc.v[0] > 0.5f;
    if (done[i] && cfg.auto_reset) {
        memcpy(&e->term_obs[(size_t)i * QS_MAX_OBS], ob, QS_MAX_OBS * sizeof(float));
        EV::reset(cfg, e->record(i), ob, e->gid(i), true);
    }
    memcpy(obs + (size_t)i * cfg.obs_dim, ob, cfg.obs_dim * sizeof(float));
}

// qs_reset / qs_reset_to of the masked environments as k_reset / k_reset_rack run them with reset_lookahead = 0: spawn and settle in place;
// or (states) the randomizers, the given rigid-body state, the task / sensor / filter reset, zero action history
template <class EV> static void reset_envs(Emu* e, const uint8_t* mask, const float* states) {
    const qs_config& cfg = e->dc.cfg;
    for (int i = 0; i < cfg.n_envs; i++) {
        if (mask && !mask[i]) continue;
        float* rec = e->record(i);
        if (states) {
            EV::randomize(cfg, rec, e->gid(i), qs::f2i(rec[R_EPISODE]) + 1, false);
            memcpy(rec + R_POS, states + (size_t)i * 37, 37 * sizeof(float));
            for (int k = 0; k < 4; k++) { rec[R_WARM + k] = 0.0f; rec[R_FOOT_FORCE + k] = 0.0f; rec[R_FOOT_CONTACT + k] = 0.0f; }
            if (e->rack) for (int k = 0; k < 6; k++) rec[R_BLOCK + RK_LAM + k] = 0.0f;
            rec[R_N_INVALID] = 0.0f;
            for (int k = 0; k < 24; k++) rec[R_TAU_PD + k] = 0.0f;
            if (cfg.payload_soft) EV::place_block(cfg, rec);
        }
        EV::reset(cfg, rec, e->obs_row(i), e->gid(i), states == nullptr);
        if (states) for (int k = 0; k < 12 + 24 + 24; k++) rec[R_LAST_ACTION + k] = 0.0f;
    }
}

// One environment's row set, laid out as tests/hip/rare_probe.hip takes it: rows [4 legs][12][16] (a Row's fields in struct order), mu,
// mine, warm [4], the payload rows [59] (w 36, rhs 6, dinv 6, diag 6, rB 3, mI, act; a RACK build: the rack's rows), then 1 if the solve
// had such rows at all.
enum { RARE_ROW_F = 16, RARE_ROWS = 4 * 12 * RARE_ROW_F, RARE_ENV = RARE_ROWS, RARE_WARM = RARE_ENV + 2, RARE_PAY = RARE_WARM + 4, RARE_PAY_F = 59,
       RARE_HAS_PAY = RARE_PAY + RARE_PAY_F, RARE_REC = RARE_HAS_PAY + 1 };
// (static, not inline: an inline variable is one per PROCESS once two libraries are loaded, and each library captures its own solves)
static std::mutex g_cap_mu;
static std::vector<float> g_cap;
static size_t g_cap_max = 0;

template <class V, class R, class P> static void rare_capture(const V& mu, const R* xr, const P* pay, const V& warm) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    if (g_cap.size() >= g_cap_max * RARE_REC) return;
    float r[RARE_REC] = {};
    for (int L = 0; L < 4; L++)
        for (int k = 0; k < 12; k++) {
            float* q = r + (12 * L + k) * RARE_ROW_F;
            for (int i = 0; i < 3; i++) { q[i] = xr[k].jq[i].v[L]; q[3 + i] = xr[k].u[i].v[L]; }
            for (int i = 0; i < 6; i++) q[6 + i] = xr[k].w[i].v[L];
            q[12] = xr[k].rhs.v[L]; q[13] = xr[k].dinv.v[L]; q[14] = xr[k].act.v[L]; q[15] = xr[k].diag.v[L];
        }
    r[RARE_ENV] = mu.v[0]; r[RARE_ENV + 1] = 1.0f;
    for (int L = 0; L < 4; L++) r[RARE_WARM + L] = warm.v[L];
    if (pay) {
        float* q = r + RARE_PAY;
        for (int k = 0; k < 6; k++) {
            for (int i = 0; i < 6; i++) q[6 * k + i] = pay->w[k][i].v[0];
            q[36 + k] = pay->rhs[k].v[0]; q[42 + k] = pay->dinv[k].v[0]; q[48 + k] = pay->diag[k].v[0];
        }
        q[54] = pay->rB.x.v[0]; q[55] = pay->rB.y.v[0]; q[56] = pay->rB.z.v[0]; q[57] = pay->mI.v[0]; q[58] = pay->act.v[0];
        r[RARE_HAS_PAY] = 1.0f;
    }
    g_cap.insert(g_cap.end(), r, r + RARE_REC);
}

extern "C" {
// capture the inputs of the next `max_sets` many-rows solves of this library's builds (0: stop); qse_rare_captured copies them out
// (RARE_REC floats each) and clears
int qse_rare_capture(int max_sets) { std::lock_guard<std::mutex> lk(g_cap_mu); g_cap.clear(); g_cap_max = (size_t)(max_sets > 0 ? max_sets : 0); return RARE_REC; }
int qse_rare_captured(float* out) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    const int n = (int)(g_cap.size() / RARE_REC);
    if (out) { memcpy(out, g_cap.data(), g_cap.size() * sizeof(float)); g_cap.clear(); g_cap_max = 0; }
    return n;
}
}
