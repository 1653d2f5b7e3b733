// qs_emu.cpp -- TEST-ONLY host emulation of the quad-per-environment kernels.
// Instantiates the kernel arithmetic of quadruped-springs_amd/csrc/qs_env.h with the 4-wide LaneEmu type so that the
// CPU test-suite (no GPU in the build container) can compare it with the oracle.  Never linked into the product.
#include <mutex>
// the many-rows solve's inputs, captured while steps run (qse_rare_capture; tests/test_rare_solver.py): qs_rare.h's emulation twin calls
// QS_RARE_CAPTURE with them, a no-op unless defined before the kernel headers
template <class V, class R, class P> static void rare_capture(const V& mu, const R* xr, const P* pay, const V& warm);
#define QS_RARE_CAPTURE(cfg, mu, xr, pay, mine, warm) rare_capture(mu, xr, pay, warm)
#include "qs_emu.h"

// One environment's row set, laid out as tests/hip/rare_probe.hip takes it: rows [4 legs][12][16] (a Row's fields in struct order), mu,
// mine, warm [4], the payload rows [59] (w 36, rhs 6, dinv 6, diag 6, rB 3, mI, act), then 1 if the solve had payload rows at all.
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

template <bool CONE> static void rare_solve_impl(const qs_config& cfg, int n_envs, const float* rows, const float* env, const float* warm, const float* pay,
                                                 float* lam12, float* plam) {
    using Ty = qs::SimTypes<LaneEmu>;
    for (int e = 0; e < n_envs; e++) {
        typename Ty::Row xr[12];
        for (int k = 0; k < 12; k++)
            for (int L = 0; L < 4; L++) {
                const float* q = rows + ((size_t)(4 * e + L) * 12 + k) * RARE_ROW_F;
                for (int i = 0; i < 3; i++) { xr[k].jq[i].v[L] = q[i]; xr[k].u[i].v[L] = q[3 + i]; }
                for (int i = 0; i < 6; i++) xr[k].w[i].v[L] = q[6 + i];
                xr[k].rhs.v[L] = q[12]; xr[k].dinv.v[L] = q[13]; xr[k].act.v[L] = q[14]; xr[k].diag.v[L] = q[15];
            }
        typename Ty::PayRows pr;
        if (pay) {
            const float* q = pay + (size_t)e * RARE_PAY_F;
            for (int k = 0; k < 6; k++) {
                for (int i = 0; i < 6; i++) pr.w[k][i] = V4(q[6 * k + i]);
                pr.rhs[k] = V4(q[36 + k]); pr.dinv[k] = V4(q[42 + k]); pr.diag[k] = V4(q[48 + k]);
            }
            pr.rB = qs::mk3<V4>(V4(q[54]), V4(q[55]), V4(q[56])); pr.mI = V4(q[57]); pr.act = V4(q[58]);
        }
        const bool mine = env[2 * e + 1] > 0.5f;
        const M4 m = {{mine, mine, mine, mine}};
        const float* wp = warm + 4 * (size_t)e;
        V4 lam[12], pl[6];
        qs::RareSolver<LaneEmu, CONE>::solve(cfg, V4(env[2 * e]), xr, pay ? &pr : nullptr, m, V4(wp[0], wp[1], wp[2], wp[3]), nullptr, lam, pl);
        for (int L = 0; L < 4; L++)
            for (int k = 0; k < 12; k++) lam12[(size_t)(4 * e + L) * 12 + k] = lam[k].v[L];
        for (int k = 0; k < 6; k++) plam[(size_t)e * 6 + k] = pl[k].v[0];
    }
}

static void init_record(const qs_config& cfg, float* r, int env) {
    memset(r, 0, QS_REC * sizeof(float));
    r[R_EPISODE] = qs::i2f(-1);
    r[R_QUAT + 3] = 1.0f; r[R_POS + 2] = 0.32f; r[R_TASK + T_FIRST_JUMP] = 1.0f;
    for (int L = 0; L < 4; L++) { r[R_Q + 3 * L + 1] = 0.78539816339f; r[R_Q + 3 * L + 2] = -1.57079632679f; }
    E::randomize(cfg, r, (uint32_t)(env + cfg.env_id_offset), -1, true);
}

template <class EV> static void phys_step_impl(Emu* e, int i, const float* tau12) {
    float* rec = &e->rec[(size_t)i * QS_REC];
    typename EV::S::State s; typename EV::S::Par P; typename EV::S::Out o;
    EV::load_state(rec, s); EV::load_par(e->cfg, rec, P);
    V4 tau[3];
    for (int j = 0; j < 3; j++) { tau[j] = LaneEmu::ld_leg(tau12, j, 3); o.tau_pd[j] = V4(0.0f); o.tau_spring[j] = V4(0.0f); }
    EV::S::substep(e->cfg, P, s, tau, o, true, e->cfg.payload_soft ? rec + R_BLOCK : nullptr);
    EV::store_state(rec, s, o);
}

extern "C" {
void* qse_create(const qs_config* cfg) {
    Emu* e = new Emu();
    e->cfg = *cfg;
    e->rec.assign((size_t)cfg->n_envs * QS_REC, 0.0f);
    e->obs.assign((size_t)cfg->n_envs * QS_MAX_OBS, 0.0f);
    e->term_obs.assign((size_t)cfg->n_envs * QS_MAX_OBS, 0.0f);
    for (int i = 0; i < cfg->n_envs; i++) init_record(e->cfg, &e->rec[(size_t)i * QS_REC], i);
    return e;
}
void qse_destroy(void* h) { delete (Emu*)h; }
int qse_set_trace(void* h, int env, float* rows) { Emu* e = (Emu*)h; e->trace_env = env; e->trace = env >= 0 ? rows : nullptr; return 0; }
int qse_reset(void* h, const uint8_t* mask) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++)
        if (!mask || mask[i]) {
            if (e->cfg.friction_cone) EC::reset(e->cfg, &e->rec[(size_t)i * QS_REC], &e->obs[(size_t)i * QS_MAX_OBS], (uint32_t)(i + e->cfg.env_id_offset), true);
            else E::reset(e->cfg, &e->rec[(size_t)i * QS_REC], &e->obs[(size_t)i * QS_MAX_OBS], (uint32_t)(i + e->cfg.env_id_offset), true);
        }
    return 0;
}
// qs_reset_to (k_reset with states): randomizers, the given rigid-body state, task / sensor / filter reset, zero action history
int qse_reset_to(void* h, const uint8_t* mask, const float* states) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++) {
        if (mask && !mask[i]) continue;
        float* rec = &e->rec[(size_t)i * QS_REC];
        const uint32_t gid = (uint32_t)(i + e->cfg.env_id_offset);
        E::randomize(e->cfg, rec, gid, qs::f2i(rec[R_EPISODE]) + 1, false);
        memcpy(rec + R_POS, states + (size_t)i * 37, 37 * sizeof(float));
        for (int k = 0; k < 4; k++) { rec[R_WARM + k] = 0.0f; rec[R_FOOT_FORCE + k] = 0.0f; rec[R_FOOT_CONTACT + k] = 0.0f; }
        rec[R_N_INVALID] = 0.0f;
        for (int k = 0; k < 24; k++) rec[R_TAU_PD + k] = 0.0f;
        if (e->cfg.payload_soft) E::place_block(e->cfg, rec);
        E::reset(e->cfg, rec, &e->obs[(size_t)i * QS_MAX_OBS], gid, false);
        for (int k = 0; k < 12 + 24 + 24; k++) rec[R_LAST_ACTION + k] = 0.0f;
    }
    return 0;
}
int qse_set_demo(void* h, const float* rows, int length) {
    Emu* e = (Emu*)h;
    e->demo.assign(rows, rows + (size_t)length * (e->cfg.action_dim + 38));
    e->demo_len = length;
    return 0;
}
int qse_set_demo_counter(void* h, const uint8_t* mask, const int32_t* values) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++)
        if (!mask || mask[i]) { float* r = &e->rec[(size_t)i * QS_REC + R_DEMO]; r[0] = r[1] = (float)values[i]; }
    return 0;
}
int qse_get_obs(void* h, float* obs) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++) memcpy(obs + (size_t)i * e->cfg.obs_dim, &e->obs[(size_t)i * QS_MAX_OBS], e->cfg.obs_dim * sizeof(float));
    return 0;
}
// infos[i]["terminal_observation"] of the last episode each environment finished (auto_reset)
int qse_get_term_obs(void* h, float* obs) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++) memcpy(obs + (size_t)i * e->cfg.obs_dim, &e->term_obs[(size_t)i * QS_MAX_OBS], e->cfg.obs_dim * sizeof(float));
    return 0;
}
int qse_step(void* h, const float* actions, float* obs, float* rew, uint8_t* done, uint8_t* trunc) {
    Emu* e = (Emu*)h;
    const int d = e->cfg.action_dim;
    for (int i = 0; i < e->cfg.n_envs; i++) {
        float* rec = &e->rec[(size_t)i * QS_REC];
        float* ob = &e->obs[(size_t)i * QS_MAX_OBS];
        float* tr = (e->trace && i == e->trace_env) ? e->trace : nullptr;
        float rw, dn, tc;
        if (e->cfg.friction_cone) { EC::StepOut r = EC::step(e->cfg, rec, actions + (size_t)i * d, ob, (uint32_t)(i + e->cfg.env_id_offset), 0, tr, tr != nullptr, e->demo.data(), e->demo_len); rw = r.reward.v[0]; dn = r.done.v[0]; tc = r.trunc.v[0]; }
        else { E::StepOut r = E::step(e->cfg, rec, actions + (size_t)i * d, ob, (uint32_t)(i + e->cfg.env_id_offset), 0, tr, tr != nullptr, e->demo.data(), e->demo_len); rw = r.reward.v[0]; dn = r.done.v[0]; tc = r.trunc.v[0]; }
        finish_env_step(e, i, rw, dn, tc, obs, rew, done, trunc);
    }
    return 0;
}
int qse_get_state(void* h, float* st) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++) memcpy(st + (size_t)i * 37, &e->rec[(size_t)i * QS_REC + R_POS], 37 * sizeof(float));
    return 0;
}
int qse_set_state(void* h, const float* st) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++) {
        float* r = &e->rec[(size_t)i * QS_REC];
        memcpy(r + R_POS, st + (size_t)i * 37, 37 * sizeof(float));
        for (int k = 0; k < 4; k++) r[R_WARM + k] = 0.0f;
        if (e->cfg.payload_soft) E::place_block(e->cfg, r);
    }
    return 0;
}
// the payload block as its own body (cfg.payload_soft): [N, 20], the oracle's qso_get_block row
int qse_get_block(void* h, float* out) {
    Emu* e = (Emu*)h;
    for (int i = 0; i < e->cfg.n_envs; i++) memcpy(out + (size_t)i * QS_BLOCK_DIM, &e->rec[(size_t)i * QS_REC + R_BLOCK], QS_BLOCK_DIM * sizeof(float));
    return 0;
}
float* qse_records(void* h) { return ((Emu*)h)->rec.data(); }
int qse_rec_size(void) { return QS_REC; }
int qse_field(const char* name) {
#define F(n) if (!strcmp(name, #n)) return n;
    F(R_POS) F(R_QUAT) F(R_VLIN) F(R_VANG) F(R_Q) F(R_QD) F(R_WARM) F(R_LAST_ACTION) F(R_XHIST) F(R_YHIST) F(R_SIM_STEP) F(R_ENV_STEP)
    F(R_EPISODE) F(R_TOTAL_STEPS) F(R_TASK) F(R_NEW_TAU) F(R_PARAMS) F(R_FOOT_FORCE) F(R_FOOT_CONTACT) F(R_N_INVALID) F(R_TAU_PD)
    F(R_TAU_SPRING) F(R_POSE_CACHE) F(R_CPG) F(R_DEMO) F(R_WRAP) F(R_BLOCK)
#undef F
    return -1;
}
// the separating-axis box / box test of the self-collision rule (qs_core.h obb_overlap); R row-major with the axes as COLUMNS
int qse_obb_overlap(const float* ca, const float* Ra, const float* ha, const float* cb, const float* Rb, const float* hb) {
    using S = E::S;
    auto col = [](const float* R, int j) { return qs::mk3<V4>(V4(R[j]), V4(R[3 + j]), V4(R[6 + j])); };
    S::H3 HA = {{ha[0], ha[1], ha[2]}}, HB = {{hb[0], hb[1], hb[2]}};
    M4 m = S::obb_overlap(qs::mk3<V4>(V4(ca[0]), V4(ca[1]), V4(ca[2])), col(Ra, 0), col(Ra, 1), col(Ra, 2), HA,
                          qs::mk3<V4>(V4(cb[0]), V4(cb[1]), V4(cb[2])), col(Rb, 0), col(Rb, 1), col(Rb, 2), HB);
    return m.v[0] ? 1 : 0;
}
// the emulation twin of the many-rows solve (RareSolver<LaneEmu, cfg.friction_cone>) on row sets laid out as tests/hip/rare_probe.hip's
// qsp_rare_solve takes them: rows [n_envs x 4][12][16], env [n_envs][2] (mu, mine), warm [n_envs x 4], pay [n_envs][59] or null
int qse_rare_solve(const qs_config* cfg, int n_envs, const float* rows, const float* env, const float* warm, const float* pay, float* lam12, float* plam) {
    if (cfg->friction_cone) rare_solve_impl<true>(*cfg, n_envs, rows, env, warm, pay, lam12, plam);
    else rare_solve_impl<false>(*cfg, n_envs, rows, env, warm, pay, lam12, plam);
    return 0;
}
// capture the inputs of the next `max_sets` many-rows solves (0: stop); qse_rare_captured copies them out (RARE_REC floats each) and clears
int qse_rare_capture(int max_sets) { std::lock_guard<std::mutex> lk(g_cap_mu); g_cap.clear(); g_cap_max = (size_t)(max_sets > 0 ? max_sets : 0); return RARE_REC; }
int qse_rare_captured(float* out) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    const int n = (int)(g_cap.size() / RARE_REC);
    if (out) { memcpy(out, g_cap.data(), g_cap.size() * sizeof(float)); g_cap.clear(); g_cap_max = 0; }
    return n;
}
// one physics substep of env `i` under given joint torques (KATs on the kernel arithmetic)
int qse_phys_step(void* h, int i, const float* tau12) {
    Emu* e = (Emu*)h;
    if (e->cfg.friction_cone) phys_step_impl<EC>(e, i, tau12);
    else phys_step_impl<E>(e, i, tau12);
    return 0;
}
}
