// rare_probe.hip -- TEST-ONLY: the many-rows contact solve (RareSolver<LaneDev, CONE>, quadruped-springs_amd/csrc/qs_rare.h) on rows
// handed in from the host, compiled with the product's hipcc options.  Never linked into the product.
//
// One wave per block, 16 environments per wave, lane 4 e + K = leg K of environment e, as Sim::substep calls the solver; the wave's
// scratch is 16 x QS_MAX_OBS floats of LDS, as wave_scratch() gives it in the step kernels.  What this compiles is the solver's source in a
// small kernel: the register allocation of the copy inlined into k_step / k_step_dense is not what runs here.
//
// Inputs, for n_envs = 16 x the number of blocks:
//   rows [n_envs x 4][12][16]  per lane, its leg's twelve Rows in struct order (jq 3, u 3, w 6, rhs, dinv, act, diag)
//   env  [n_envs][2]           mu, mine (> 0.5: the environment has rows for this solve)
//   warm [n_envs x 4]          per lane, the foot's warm-start impulse (already x warmstart x act)
//   pay  [n_envs][PAY] or null the payload rows: w 36, rhs 6, dinv 6, diag 6, rB 3, mI, act
// Outputs: lam12 [n_envs x 4][12] per lane, plam [n_envs][6] per environment.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../quadruped-springs_amd/csrc/qs_core.h"

using Ty = qs::SimTypes<LaneDev>;   // (LaneDev: qs_lane.h, outside the namespace)
using Row = Ty::Row;
using PayRows = Ty::PayRows;

enum { PROBE_ROW_FLOATS = 16, PROBE_PAY_FLOATS = 59, PROBE_ENV_FLOATS = 2 };
static_assert(sizeof(Row) == PROBE_ROW_FLOATS * sizeof(float), "Row is sixteen floats");
static_assert(qs::RarePos::SCRATCH_FLOATS + 64 <= 16 * QS_MAX_OBS, "the solver's LDS (rows, impulses, dummy record) fits the wave's rows");

template <bool CONE, int CORE>
__global__ __launch_bounds__(64) void k_rare_probe(qs_config cfg, const float* __restrict__ rows, const float* __restrict__ env, const float* __restrict__ warm,
                                                   const float* __restrict__ pay, float* __restrict__ lam12_out, float* __restrict__ plam_out) {
    __shared__ float scr[16 * QS_MAX_OBS];
    const int lane = (int)threadIdx.x, gl = (int)blockIdx.x * 64 + lane, ge = gl >> 2;
    Row xr[12];
    const float* rp = rows + (size_t)gl * 12 * PROBE_ROW_FLOATS;
#pragma unroll
    for (int r = 0; r < 12; r++) {
        const float* q = rp + r * PROBE_ROW_FLOATS;
        for (int i = 0; i < 3; i++) { xr[r].jq[i] = q[i]; xr[r].u[i] = q[3 + i]; }
        for (int i = 0; i < 6; i++) xr[r].w[i] = q[6 + i];
        xr[r].rhs = q[12]; xr[r].dinv = q[13]; xr[r].act = q[14]; xr[r].diag = q[15];
    }
    PayRows pr = {};
    if (pay) {
        const float* q = pay + (size_t)ge * PROBE_PAY_FLOATS;
        for (int k = 0; k < 6; k++) {
            for (int i = 0; i < 6; i++) pr.w[k][i] = q[6 * k + i];
            pr.rhs[k] = q[36 + k]; pr.dinv[k] = q[42 + k]; pr.diag[k] = q[48 + k];
        }
        pr.rB.x = q[54]; pr.rB.y = q[55]; pr.rB.z = q[56]; pr.mI = q[57]; pr.act = q[58];
    }
    const float mu = env[(size_t)ge * PROBE_ENV_FLOATS], mine = env[(size_t)ge * PROBE_ENV_FLOATS + 1];
    float lam12[12], plam[6];
    qs::RareSolver<LaneDev, CONE>::template solve<CORE>(cfg, mu, xr, pay ? &pr : nullptr, mine > 0.5f, warm[gl], scr, lam12, plam);
#pragma unroll
    for (int r = 0; r < 12; r++) lam12_out[(size_t)gl * 12 + r] = lam12[r];
    if ((lane & 3) == 0)
#pragma unroll
        for (int k = 0; k < 6; k++) plam_out[(size_t)ge * 6 + k] = plam[k];
}

template <bool CONE>
static hipError_t launch(int core, int blocks, const qs_config& cfg, const float* rows, const float* env, const float* warm, const float* pay, float* lam, float* plam) {
    switch (core) {
    case 0: k_rare_probe<CONE, 0><<<blocks, 64>>>(cfg, rows, env, warm, pay, lam, plam); break;
    case 1: k_rare_probe<CONE, 1><<<blocks, 64>>>(cfg, rows, env, warm, pay, lam, plam); break;
    case 2: k_rare_probe<CONE, 2><<<blocks, 64>>>(cfg, rows, env, warm, pay, lam, plam); break;
    default: k_rare_probe<CONE, 3><<<blocks, 64>>>(cfg, rows, env, warm, pay, lam, plam); break;
    }
    return hipGetLastError();
}

extern "C" {
// Error codes: hipError_t values from the runtime; -1 bad arguments; -2 a forced <0, 4> / <0, 6> given an environment it cannot hold.
int qsp_rare_solve(const qs_config* cfg, int n_envs, int core, const float* rows, const float* env, const float* warm, const float* pay,
                   float* lam12, float* plam) {
    if (!cfg || n_envs <= 0 || n_envs % 16 || core < 0 || core > 3 || !rows || !env || !warm || !lam12 || !plam) return -1;
    if (core == 1 || core == 2) {
        const int cap = core == 1 ? 4 : 6;
        for (int e = 0; e < n_envs; e++) {
            if (env[(size_t)e * PROBE_ENV_FLOATS + 1] <= 0.5f) continue;
            int nA = pay && pay[(size_t)e * PROBE_PAY_FLOATS + 58] > 0.5f ? 6 : 0, nB = 0;
            for (int K = 0; K < 4; K++) {
                const float* rp = rows + ((size_t)(4 * e + K) * 12) * PROBE_ROW_FLOATS;
                for (int j = 0; j < 3; j++) nA += rp[(9 + j) * PROBE_ROW_FLOATS + 14] > 0.5f ? 1 : 0;
                for (int c = 0; c < 3; c++) nB += rp[(3 * c) * PROBE_ROW_FLOATS + 14] > 0.5f ? 1 : 0;
            }
            if (nA > 0 || nB > cap) return -2;
        }
    }
    const size_t n_rows = (size_t)n_envs * 4 * 12 * PROBE_ROW_FLOATS, n_env = (size_t)n_envs * PROBE_ENV_FLOATS, n_warm = (size_t)n_envs * 4,
                 n_pay = pay ? (size_t)n_envs * PROBE_PAY_FLOATS : 0, n_lam = (size_t)n_envs * 4 * 12, n_plam = (size_t)n_envs * 6;
    const size_t total = n_rows + n_env + n_warm + n_pay + n_lam + n_plam;
    float* d = nullptr;
    hipError_t err = hipMalloc(&d, total * sizeof(float));
    if (err != hipSuccess) return (int)err;
    float *d_rows = d, *d_env = d_rows + n_rows, *d_warm = d_env + n_env, *d_pay = d_warm + n_warm, *d_lam = d_pay + n_pay, *d_plam = d_lam + n_lam;
    auto step = [&](hipError_t e) { if (err == hipSuccess) err = e; };
    step(hipMemcpy(d_rows, rows, n_rows * sizeof(float), hipMemcpyHostToDevice));
    step(hipMemcpy(d_env, env, n_env * sizeof(float), hipMemcpyHostToDevice));
    step(hipMemcpy(d_warm, warm, n_warm * sizeof(float), hipMemcpyHostToDevice));
    if (pay) step(hipMemcpy(d_pay, pay, n_pay * sizeof(float), hipMemcpyHostToDevice));
    step(hipMemset(d_lam, 0xFF, (n_lam + n_plam) * sizeof(float)));   // (NaN: an output the kernel does not write shows)
    if (err == hipSuccess) {
        const float* pp = pay ? d_pay : nullptr;
        step(cfg->friction_cone ? launch<true>(core, n_envs / 16, *cfg, d_rows, d_env, d_warm, pp, d_lam, d_plam)
                                : launch<false>(core, n_envs / 16, *cfg, d_rows, d_env, d_warm, pp, d_lam, d_plam));
        step(hipDeviceSynchronize());
        step(hipMemcpy(lam12, d_lam, n_lam * sizeof(float), hipMemcpyDeviceToHost));
        step(hipMemcpy(plam, d_plam, n_plam * sizeof(float), hipMemcpyDeviceToHost));
    }
    const hipError_t ef = hipFree(d);
    return (int)(err != hipSuccess ? err : ef);
}
int qsp_row_floats(void) { return PROBE_ROW_FLOATS; }
int qsp_pay_floats(void) { return PROBE_PAY_FLOATS; }
}
