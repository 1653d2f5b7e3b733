// substep_probe.hip -- TEST-ONLY: ONE physics substep (Sim<LaneDev, CONE, HOT, SOFT>::substep, quadruped-springs_amd/csrc/qs_core.h) on records
// handed in from the host, compiled with the product's hipcc options.  Never linked into the product.
//
// One wave per block, 16 records per wave, lane 4 e + K = leg K of environment e.  As in the step kernels the wave's records sit in LDS
// while it works on them (QS_REC floats apart) and `scratch_row` is the environment's row of a 16 x QS_MAX_OBS LDS block, which the
// many-rows solve borrows (wave_scratch, qs_lane.h).  Per environment: Env::load_state, Env::load_par, substep(cfg, P, s, tau, o, true, blk,
// scratch_row, true, push, 0), Env::store_state -- what tests/emu/qs_emu_substep.cpp does on the host.  What this compiles is the
// substep's source in a small kernel: the register allocation of the copy inlined into k_step / k_step_dense is not what runs here.
//
// The configuration is handed over as the step kernels get it: the first member of a QsDevCfg in device memory with a real counter block
// behind it (LaneDev::count_rare_path / count_self_narrow add to it) and solo = 0.
//
// Inputs, for n_envs = 16 x the number of blocks:
//   recs [n_envs][QS_REC]       the records (parameters, rigid-body state, warm start, payload block)
//   tau  [n_envs][12]           joint torques
//   push [n_envs][8] or null    rows of qs_set_external_wrench: force 3, torque 3, remaining substeps, frame
// Outputs: the records after the substep (state, warm start, foot force, foot contact, n_invalid, the payload block), substep's return
// value per environment, the counter block.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>
#include "../../quadruped-springs_amd/csrc/qs_env.h"

enum { PROBE_PUSH_F = 8 /* = QS_PUSH_F (qs_hip.hip) */, PROBE_COUNTERS = 32, PROBE_BUILD_FULL = 0, PROBE_BUILD_HOT = 1, PROBE_BUILD_HOT_SOFT = 2 };
static_assert(qs::RarePos::SCRATCH_FLOATS + 64 <= 16 * QS_MAX_OBS, "the many-rows solver's LDS (rows, impulses, dummy record) fits the wave's rows");
static_assert(PROBE_COUNTERS > QS_DEVCTR_SOLO_PATH, "the counter block holds every counter the lanes add to");
static_assert(QS_REC % 4 == 0 && R_BLOCK + QS_BLOCK_DIM <= QS_REC && R_TAU_SPRING + 12 <= QS_REC, "a record holds every field the substep moves");

template <bool CONE, bool HOT, bool SOFT>
__global__ __launch_bounds__(64) void k_substep_probe(const QsDevCfg* __restrict__ dc, const float* __restrict__ rec_in, const float* __restrict__ tau_in,
                                                      const float* __restrict__ push, float* __restrict__ rec_out, int* __restrict__ rc_out) {
    using EV = qs::Env<LaneDev, CONE, HOT, SOFT>;
    using S = typename EV::S;
    __shared__ __attribute__((aligned(16))) float s_rec[16 * QS_REC];
    __shared__ __attribute__((aligned(16))) float scr[16 * QS_MAX_OBS];
    const qs_config& cfg = dc->cfg;
    const int lane = (int)threadIdx.x, slot = lane >> 2, env = (int)blockIdx.x * 16 + slot;
    const size_t base = (size_t)blockIdx.x * 16 * QS_REC;
    for (int i = lane; i < 16 * QS_REC; i += 64) s_rec[i] = rec_in[base + i];
    for (int i = lane; i < 16 * QS_MAX_OBS; i += 64) scr[i] = 0.0f;
    __syncthreads();
    float* rec = s_rec + slot * QS_REC;
    typename S::State s; typename S::Par P; typename S::Out o;
    EV::load_state(rec, s); EV::load_par(cfg, rec, P);
    float tau[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        tau[j] = LaneDev::ld_leg(tau_in + (size_t)env * 12, j, 3);
        o.tau_pd[j] = LaneDev::ld_leg(rec, R_TAU_PD + j, 3); o.tau_spring[j] = LaneDev::ld_leg(rec, R_TAU_SPRING + j, 3);
    }
    o.foot_force = LaneDev::ld_leg(rec, R_FOOT_FORCE, 1); o.foot_contact = LaneDev::ld_leg(rec, R_FOOT_CONTACT, 1); o.n_invalid = LaneDev::ld(rec, R_N_INVALID);
    // (blk: always the record's block.  Without a rack substep() reads it only under cfg.payload_soft, so this is Env::step's
    // `cfg.payload_soft ? rec + R_BLOCK : nullptr`; that select, a per-lane pointer whose null test the compiler takes for divergent, stops
    // hipcc 7.2 in this kernel's full build with "illegal VGPR to SGPR copy")
    const int rc = S::substep(cfg, P, s, tau, o, true, rec + R_BLOCK, scr + slot * QS_MAX_OBS, true, push ? push + (size_t)env * PROBE_PUSH_F : nullptr, 0);
    LaneDev::sync();
    EV::store_state(rec, s, o);
    if ((lane & 3) == 0) rc_out[env] = rc;
    __syncthreads();
    for (int i = lane; i < 16 * QS_REC; i += 64) rec_out[base + i] = s_rec[i];
}

template <bool CONE>
static hipError_t launch(int build, int blocks, const QsDevCfg* dc, const float* rec, const float* tau, const float* push, float* out, int* rc) {
    switch (build) {
    case PROBE_BUILD_FULL: k_substep_probe<CONE, false, false><<<blocks, 64>>>(dc, rec, tau, push, out, rc); break;
    case PROBE_BUILD_HOT: k_substep_probe<CONE, true, false><<<blocks, 64>>>(dc, rec, tau, push, out, rc); break;
    default:
        if constexpr (CONE) k_substep_probe<true, true, true><<<blocks, 64>>>(dc, rec, tau, push, out, rc);   // (the payload's rows: implicit cone only)
        else return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" {
// build: 0 = the full build (HOT = false), 1 = the common-path build (HOT), 2 = the common-path build with the payload block's rows (HOT,
// SOFT: cfg.friction_cone and cfg.payload_soft only).  counters: null, or PROBE_COUNTERS values out.
// Error codes: hipError_t values from the runtime; -1 bad arguments.
int qsp_substep(const qs_config* cfg, int n_envs, int build, const float* recs, const float* tau, const float* push, float* recs_out, int* rc_out,
                unsigned long long* counters) {
    if (!cfg || n_envs <= 0 || n_envs % 16 || build < PROBE_BUILD_FULL || build > PROBE_BUILD_HOT_SOFT || !recs || !tau || !recs_out || !rc_out) return -1;
    if (build == PROBE_BUILD_HOT_SOFT && !(cfg->friction_cone && cfg->payload_soft)) return -1;
    if (cfg->solver_iters < 1 || cfg->solver_iters > 1000 || !(cfg->dt > 0.0)) return -1;
    const size_t n_rec = (size_t)n_envs * QS_REC, n_tau = (size_t)n_envs * 12, n_push = push ? (size_t)n_envs * PROBE_PUSH_F : 0, n_rc = (size_t)n_envs;
    const size_t total = 2 * n_rec + n_tau + n_push + n_rc;     // (floats; rc_out as 4-byte integers)
    float* d = nullptr;
    QsDevCfg* d_dc = nullptr;
    unsigned long long* d_ctr = nullptr;
    hipError_t err = hipMalloc(&d, total * sizeof(float));
    if (err != hipSuccess) return (int)err;
    auto step = [&](hipError_t e) { if (err == hipSuccess) err = e; };
    step(hipMalloc(&d_dc, sizeof(QsDevCfg)));
    step(hipMalloc(&d_ctr, PROBE_COUNTERS * sizeof(unsigned long long)));
    float *d_rec = d, *d_out = d_rec + n_rec, *d_tau = d_out + n_rec, *d_push = d_tau + n_tau;
    int* d_rc = (int*)(d_push + n_push);
    if (err == hipSuccess) {
        QsDevCfg dc;
        memset(&dc, 0, sizeof(dc));
        dc.cfg = *cfg; dc.counters = d_ctr; dc.rack_pos[2] = 1.0f; dc.rack_quat[3] = 1.0f; dc.solo = 0;
        step(hipMemcpy(d_dc, &dc, sizeof(dc), hipMemcpyHostToDevice));
        step(hipMemset(d_ctr, 0, PROBE_COUNTERS * sizeof(unsigned long long)));
        step(hipMemcpy(d_rec, recs, n_rec * sizeof(float), hipMemcpyHostToDevice));
        step(hipMemcpy(d_tau, tau, n_tau * sizeof(float), hipMemcpyHostToDevice));
        if (push) step(hipMemcpy(d_push, push, n_push * sizeof(float), hipMemcpyHostToDevice));
        step(hipMemset(d_out, 0xFF, n_rec * sizeof(float)));    // (NaN: an output the kernel does not write shows)
        step(hipMemset(d_rc, 0xFF, n_rc * sizeof(int)));        // (-1)
    }
    if (err == hipSuccess) {
        const float* pp = push ? d_push : nullptr;
        step(cfg->friction_cone ? launch<true>(build, n_envs / 16, d_dc, d_rec, d_tau, pp, d_out, d_rc) : launch<false>(build, n_envs / 16, d_dc, d_rec, d_tau, pp, d_out, d_rc));
        step(hipDeviceSynchronize());
        step(hipMemcpy(recs_out, d_out, n_rec * sizeof(float), hipMemcpyDeviceToHost));
        step(hipMemcpy(rc_out, d_rc, n_rc * sizeof(int), hipMemcpyDeviceToHost));
        if (counters) step(hipMemcpy(counters, d_ctr, PROBE_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    hipError_t ef = hipFree(d);
    if (d_dc) { const hipError_t e2 = hipFree(d_dc); if (ef == hipSuccess) ef = e2; }
    if (d_ctr) { const hipError_t e2 = hipFree(d_ctr); if (ef == hipSuccess) ef = e2; }
    return (int)(err != hipSuccess ? err : ef);
}
int qsp_substep_rec_floats(void) { return QS_REC; }
int qsp_substep_counters(void) { return PROBE_COUNTERS; }
}
