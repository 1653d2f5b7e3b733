// qs_emu_rack.cpp -- TEST-ONLY host emulation of a handle with a rack (qs_create_ex with qs_rack::on = 1): the RACK builds of Env (resets
// that spawn at the anchor and hang the robot, the rack's six rows in the full build and in the common-path builds with their hand-over, as
// k_step_rack / k_step_dense_rack / k_reset_rack run them), qs_set_rack and the QS_INFO_RACK row.  Works on a handle of qs_emu.cpp, like
// qs_emu_push.cpp; the anchor comes with every call (the kernels read it behind the configuration, QsDevCfg).
#include <mutex>
// the many-rows solve's inputs, captured while steps run (qser_rare_capture), in qs_emu.cpp's layout (RARE_*): the rack's rows where the
// payload block's go
template <class V, class R, class P> static void rare_capture(const V& mu, const R* xr, const P* pay, const V& warm);
#define QS_RARE_CAPTURE(cfg, mu, xr, pay, mine, warm) rare_capture(mu, xr, pay, warm)
#include "qs_emu.h"

enum { RARE_ROW_F = 16, RARE_ROWS = 4 * 12 * RARE_ROW_F, RARE_ENV = RARE_ROWS, RARE_WARM = RARE_ENV + 2, RARE_PAY = RARE_WARM + 4, RARE_PAY_F = 59,
       RARE_HAS_PAY = RARE_PAY + RARE_PAY_F, RARE_REC = RARE_HAS_PAY + 1 };
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

namespace {

struct Result { float reward, done, trunc; int resume; };

QsDevCfg dev_cfg(const qs_config& cfg, const float* anchor) {
    QsDevCfg dc;
    memset(&dc, 0, sizeof(dc));
    dc.cfg = cfg;
    for (int i = 0; i < 3; i++) dc.rack_pos[i] = anchor[i];
    for (int i = 0; i < 4; i++) dc.rack_quat[i] = anchor[3 + i];
    return dc;
}

template <bool CONE> using EF = qs::Env<LaneEmu, CONE, false, false, true>;

template <bool CONE, bool LEAN>
Result hot_step(const qs_config& cfg, float* rec, const float* act, float* ob, uint32_t gid) {
    using EH = qs::Env<LaneEmu, CONE, true, CONE, true>;   // k_step_rack<CONE>: the common-path build holds the rack's rows under the cone
    const typename EH::StepOut rh = EH::template step<false, LEAN>(cfg, rec, act, ob, gid);
    Result r = {rh.reward.v[0], rh.done.v[0], rh.trunc.v[0], rh.resume};
    if (rh.resume >= 0) {
        const typename EF<CONE>::StepOut rf = EF<CONE>::template step<true>(cfg, rec, act, ob, gid, 0, nullptr, false, nullptr, 0, rh.resume);
        r.reward = rf.reward.v[0]; r.done = rf.done.v[0]; r.trunc = rf.trunc.v[0];
    }
    return r;
}

template <bool CONE> Result full_step(const qs_config& cfg, float* rec, const float* act, float* ob, uint32_t gid) {
    const typename EF<CONE>::StepOut r = EF<CONE>::step(cfg, rec, act, ob, gid);
    return Result{r.reward.v[0], r.done.v[0], r.trunc.v[0], -1};
}

void rack_reset(const qs_config& cfg, float* rec, float* ob, uint32_t gid, bool settle) {
    if (cfg.friction_cone) EF<true>::reset(cfg, rec, ob, gid, settle);
    else EF<false>::reset(cfg, rec, ob, gid, settle);
}

}  // namespace

extern "C" {
// reset (settle in place, as k_reset_rack with reset_lookahead = 0) of the masked environments; anchor = position 3, quaternion xyzw 4
int qser_reset(void* h, const float* anchor, const uint8_t* mask) {
    Emu* e = (Emu*)h;
    const QsDevCfg dc = dev_cfg(e->cfg, anchor);
    for (int i = 0; i < e->cfg.n_envs; i++)
        if (!mask || mask[i]) rack_reset(dc.cfg, &e->rec[(size_t)i * QS_REC], &e->obs[(size_t)i * QS_MAX_OBS], (uint32_t)(i + e->cfg.env_id_offset), true);
    return 0;
}
// qs_reset_to on a rack handle (k_reset_rack with states): the robot at the given state, hung, the rack's impulses zero
int qser_reset_to(void* h, const float* anchor, const uint8_t* mask, const float* states) {
    Emu* e = (Emu*)h;
    const QsDevCfg dc = dev_cfg(e->cfg, anchor);
    for (int i = 0; i < e->cfg.n_envs; i++) {
        if (mask && !mask[i]) continue;
        float* rec = &e->rec[(size_t)i * QS_REC];
        const uint32_t gid = (uint32_t)(i + e->cfg.env_id_offset);
        E::randomize(dc.cfg, rec, gid, qs::f2i(rec[R_EPISODE]) + 1, false);
        memcpy(rec + R_POS, states + (size_t)i * 37, 37 * sizeof(float));
        for (int k = 0; k < 4; k++) { rec[R_WARM + k] = 0.0f; rec[R_FOOT_FORCE + k] = 0.0f; rec[R_FOOT_CONTACT + k] = 0.0f; }
        for (int k = 0; k < 6; k++) rec[R_BLOCK + RK_LAM + k] = 0.0f;
        rec[R_N_INVALID] = 0.0f;
        for (int k = 0; k < 24; k++) rec[R_TAU_PD + k] = 0.0f;
        rack_reset(dc.cfg, rec, &e->obs[(size_t)i * QS_MAX_OBS], gid, false);
        for (int k = 0; k < 12 + 24 + 24; k++) rec[R_LAST_ACTION + k] = 0.0f;
    }
    return 0;
}
// qs_set_rack (k_set_rack)
int qser_set_rack(void* h, const uint8_t* mask, int hung) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++) {
        if (mask && !mask[i]) continue;
        float* b = &e->rec[(size_t)i * QS_REC + R_BLOCK];
        b[RK_HUNG] = hung ? 1.0f : 0.0f;
        for (int k = 0; k < 6; k++) b[RK_LAM + k] = 0.0f;
    }
    return 0;
}
// One env step of every environment.  variant 0 = the full build, 1 / 2 = k_step_rack's / k_step_dense_rack's common-path build and its
// hand-over; resume as qse_step_hot (-1 for the full build).  cfg.auto_reset: a finished environment is reset on the rack, in place.
int qser_step(void* h, const float* anchor, const float* actions, int variant, float* obs, float* rew, uint8_t* done, uint8_t* trunc, int32_t* resume) {
    Emu* e = (Emu*)h;
    if (variant < 0 || variant > 2) return -1;
    const QsDevCfg dc = dev_cfg(e->cfg, anchor);
    const qs_config& cfg = dc.cfg;
    const int d = cfg.action_dim;
    for (int i = 0; i < cfg.n_envs; i++) {
        float* rec = &e->rec[(size_t)i * QS_REC];
        float* ob = &e->obs[(size_t)i * QS_MAX_OBS];
        const float* act = actions + (size_t)i * d;
        const uint32_t gid = (uint32_t)(i + cfg.env_id_offset);
        Result r;
        if (variant == 0) r = cfg.friction_cone ? full_step<true>(cfg, rec, act, ob, gid) : full_step<false>(cfg, rec, act, ob, gid);
        else if (variant == 2) r = cfg.friction_cone ? hot_step<true, true>(cfg, rec, act, ob, gid) : hot_step<false, true>(cfg, rec, act, ob, gid);
        else r = cfg.friction_cone ? hot_step<true, false>(cfg, rec, act, ob, gid) : hot_step<false, false>(cfg, rec, act, ob, gid);
        resume[i] = r.resume;
        rew[i] = r.reward; done[i] = r.done > 0.5f; trunc[i] = r.trunc > 0.5f;
        if (done[i] && cfg.auto_reset) {
            memcpy(&e->term_obs[(size_t)i * QS_MAX_OBS], ob, QS_MAX_OBS * sizeof(float));
            rack_reset(cfg, rec, ob, gid, true);
        }
        memcpy(obs + (size_t)i * cfg.obs_dim, ob, cfg.obs_dim * sizeof(float));
    }
    return 0;
}
// capture the inputs of the next `max_sets` many-rows solves of the RACK builds (0: stop); qser_rare_captured copies them out and clears
int qser_rare_capture(int max_sets) { std::lock_guard<std::mutex> lk(g_cap_mu); g_cap.clear(); g_cap_max = (size_t)(max_sets > 0 ? max_sets : 0); return RARE_REC; }
int qser_rare_captured(float* out) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    const int n = (int)(g_cap.size() / RARE_REC);
    if (out) { memcpy(out, g_cap.data(), g_cap.size() * sizeof(float)); g_cap.clear(); g_cap_max = 0; }
    return n;
}
// the QS_INFO_RACK rows [N, 8] (k_rack_info)
int qser_info(void* h, const float* anchor, float* out) {
    Emu* e = (Emu*)h;
    const float inv_dt = (float)(1.0 / e->cfg.dt);
    for (int i = 0; i < e->cfg.n_envs; i++) {
        const float* r = &e->rec[(size_t)i * QS_REC];
        float* o = out + (size_t)i * 8;
        o[0] = r[R_BLOCK + RK_HUNG];
        for (int k = 0; k < 6; k++) o[1 + k] = r[R_BLOCK + RK_LAM + k] * inv_dt;
        const float dx = r[R_POS] - anchor[0], dy = r[R_POS + 1] - anchor[1], dz = r[R_POS + 2] - anchor[2];
        o[7] = sqrtf(dx * dx + dy * dy + dz * dz);
    }
    return 0;
}
}
