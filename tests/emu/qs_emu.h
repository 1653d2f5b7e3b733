// qs_emu.h -- TEST-ONLY: what the two translation units of the host emulation share (qs_emu.cpp: the full builds of the env step;
// qs_emu_hot.cpp: the common-path builds and their hand-over to the full build).  Both work on the same handle.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../quadruped-springs_amd/csrc/qs_env.h"

using E = qs::Env<LaneEmu>;            // friction pyramid
using EC = qs::Env<LaneEmu, true>;     // implicit cone (cfg.friction_cone): the kernels are built for both, so is this harness

struct Emu {
    qs_config cfg;
    std::vector<float> rec, obs, term_obs;
    float* trace = nullptr; int trace_env = -1;
    std::vector<float> demo; int demo_len = 0;
};

// what qse_step does with environment i's step result (the step wrote its observation into the staging row `ob`): outputs, and under
// cfg.auto_reset the terminal observation and the reset of a finished environment (k_step's auto-reset with reset_lookahead = 0)
static inline void finish_env_step(Emu* e, int i, float rw, float dn, float tc, float* obs, float* rew, uint8_t* done, uint8_t* trunc) {
    float* rec = &e->rec[(size_t)i * QS_REC];
    float* ob = &e->obs[(size_t)i * QS_MAX_OBS];
    rew[i] = rw; done[i] = dn > 0.5f; trunc[i] = tc > 0.5f;
    if (done[i] && e->cfg.auto_reset) {
        memcpy(&e->term_obs[(size_t)i * QS_MAX_OBS], ob, QS_MAX_OBS * sizeof(float));
        if (e->cfg.friction_cone) EC::reset(e->cfg, rec, ob, (uint32_t)(i + e->cfg.env_id_offset), true);
        else E::reset(e->cfg, rec, ob, (uint32_t)(i + e->cfg.env_id_offset), true);
    }
    memcpy(obs + (size_t)i * e->cfg.obs_dim, ob, e->cfg.obs_dim * sizeof(float));
}
