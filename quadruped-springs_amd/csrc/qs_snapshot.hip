// qs_snapshot.hip -- k_snapshot / k_restore / k_fork_gather / k_fork and the C ABI of device snapshots (qs_snapshot_info, qs_snapshot, qs_restore,
// qs_fork; include/qs_amd.h).  The row's layout and the lane-level copy are qs_snapshot.h's.
//
// Launch geometry: workgroups of four waves, one wave per environment's row (wave w of block b owns environment 4 b + w): the 74 float4 of
// record and push row in two rounds of 16-byte accesses over consecutive lanes, the two observation parts as one float per lane.  The test
// that decides whether a wave moves its row (mask, src_of) reads one wave-uniform address and branches the whole wave.  No LDS; the only
// atomic is the refusal counter of k_fork_gather.  Everything runs on the handle's stream and nothing waits for the device.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include "../../include/qs_amd.h"
#include "qs_snapshot.h"
#include "qs_host.h"

namespace {
using namespace qs::snap;
enum { WAVES = 4 };

// the environment of this wave (the same in all of its lanes: taken through the scalar file, so that what is tested on it branches the wave)
__device__ __forceinline__ int wave_env() { return (int)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)); }

__global__ __launch_bounds__(WAVES * WAVE) void k_snapshot(Arrays a, int n, int od, const uint8_t* __restrict__ mask, float* __restrict__ rows) {
    const int e = wave_env();
    if (e >= n || (mask && !mask[e])) return;
    move_row<false, false>((int)(threadIdx.x % WAVE), a, e, e, rows + (size_t)e * row_floats(od), od);
}

// also re-seats the look-ahead window of a restored environment: la.cur = la.handed = the episode of the restored record, so that the
// planning scan (k_lookahead_plan, qs_hip.hip) queues the states of the K episodes behind it again.  Slots that hold other episodes keep
// their tags and are simply not taken (lookahead_take compares the tag); the settles in flight are left alone.
__global__ __launch_bounds__(WAVES * WAVE) void k_restore(Arrays a, int n, int od, const uint8_t* __restrict__ mask, const float* __restrict__ rows,
                                                          int* __restrict__ la_cur, int* __restrict__ la_handed) {
    const int e = wave_env();
    if (e >= n || (mask && !mask[e])) return;
    const int lane = (int)(threadIdx.x % WAVE);
    const float ep = move_row<true, false>(lane, a, e, e, const_cast<float*>(rows) + (size_t)e * row_floats(od), od);
    if (la_cur && lane == R_EPISODE / 4) { const int X = __float_as_int(ep); la_cur[e] = X; la_handed[e] = X; }
}

// qs_fork, first launch: the row environment i is going to be -- its source's, with i's own kept fields (qs_snapshot.h) -- into the staging
// row i.  A source outside [-1, n) is refused and recorded.
__global__ __launch_bounds__(WAVES * WAVE) void k_fork_gather(Arrays a, int n, int od, const int32_t* __restrict__ src_of, float* __restrict__ staging,
                                                              unsigned long long* __restrict__ refused) {
    const int i = wave_env();
    if (i >= n) return;
    const int s = src_of[i];
    if (s < -1 || s >= n) { if (threadIdx.x % WAVE == 0) atomicCAS(refused, 0ull, (unsigned long long)i + 1ull); return; }
    if (!fork_takes(i, s, n)) return;
    move_row<false, true>((int)(threadIdx.x % WAVE), a, s, i, staging + (size_t)i * row_floats(od), od);
}
// second launch: the staged rows into their environments (every source was read by the launch before)
__global__ __launch_bounds__(WAVES * WAVE) void k_fork(Arrays a, int n, int od, const int32_t* __restrict__ src_of, const float* __restrict__ staging) {
    const int i = wave_env();
    if (i >= n || !fork_takes(i, src_of[i], n)) return;
    move_row<true, false>((int)(threadIdx.x % WAVE), a, i, i, const_cast<float*>(staging) + (size_t)i * row_floats(od), od);
}

Arrays arrays_of(const QsSnapshotView& v) { Arrays a; a.rec = v.rec; a.push = v.push; a.obs = v.obs; a.term = v.term; return a; }
unsigned grid_of(int n) { return (unsigned)((n + WAVES - 1) / WAVES); }
}  // namespace

extern "C" {

int qs_snapshot_info(const qs_handle* h, struct qs_snapshot_info* out) {
    if (!h || !out) QS_FAIL(-1, "null argument");
    QsSnapshotView v;
    qs_snapshot_view(const_cast<qs_handle*>(h), &v);
    const qs_config& c = *v.cfg;
    memset(out, 0, sizeof(*out));
    out->n_envs = c.n_envs; out->row_floats = row_floats(c.obs_dim); out->rec_floats = QS_REC; out->push_floats = PUSH_F; out->obs_dim = c.obs_dim;
    out->layout_version = LAYOUT_VERSION;
    out->bytes = (uint64_t)c.n_envs * (uint64_t)out->row_floats * sizeof(float);
    const int32_t lay[] = { LAYOUT_VERSION, QS_REC, c.obs_dim, c.action_dim, c.n_envs, c.task, c.wrapper_mode, c.action_space_mode, c.payload_soft, v.rack->on };
    out->layout_digest = fnv1a(lay, sizeof(lay));
    out->config_digest = fnv1a(v.rack, sizeof(qs_rack), fnv1a(v.cfg, sizeof(qs_config)));
    return 0;
}

int qs_snapshot(qs_handle* h, const uint8_t* mask, float* rows) {
    if (!h || !rows) QS_FAIL(-1, "null argument");
    if ((uintptr_t)rows % 16 != 0) QS_FAIL(-1, "qs_snapshot: rows must start on 16 bytes");
    QsSnapshotView v;
    qs_snapshot_view(h, &v);
    DeviceGuard guard(v.device);
    hipLaunchKernelGGL(k_snapshot, dim3(grid_of(v.cfg->n_envs)), dim3(WAVES * WAVE), 0, v.stream, arrays_of(v), v.cfg->n_envs, v.cfg->obs_dim, mask, rows);
    QS_HIP(hipGetLastError());
    return 0;
}

int qs_restore(qs_handle* h, const uint8_t* mask, const float* rows) {
    if (!h || !rows) QS_FAIL(-1, "null argument");
    if ((uintptr_t)rows % 16 != 0) QS_FAIL(-1, "qs_restore: rows must start on 16 bytes");
    QsSnapshotView v;
    qs_snapshot_view(h, &v);
    DeviceGuard guard(v.device);
    hipLaunchKernelGGL(k_restore, dim3(grid_of(v.cfg->n_envs)), dim3(WAVES * WAVE), 0, v.stream, arrays_of(v), v.cfg->n_envs, v.cfg->obs_dim, mask, rows,
                       v.la_K > 0 ? v.la_cur : nullptr, v.la_K > 0 ? v.la_handed : nullptr);
    QS_HIP(hipGetLastError());
    *v.push_live = 1;   // a push may be pending in the rows: the step launches read the push rows again (until a reset of all)
    return 0;
}

int qs_fork(qs_handle* h, const int32_t* src_of) {
    if (!h || !src_of) QS_FAIL(-1, "null argument");
    QsSnapshotView v;
    qs_snapshot_view(h, &v);
    DeviceGuard guard(v.device);
    const int n = v.cfg->n_envs, od = v.cfg->obs_dim;
    if (!*v.fork_rows) QS_HIP(hipMalloc(v.fork_rows, (size_t)n * row_floats(od) * sizeof(float)));
    hipLaunchKernelGGL(k_fork_gather, dim3(grid_of(n)), dim3(WAVES * WAVE), 0, v.stream, arrays_of(v), n, od, src_of, *v.fork_rows, v.fork_refused);
    hipLaunchKernelGGL(k_fork, dim3(grid_of(n)), dim3(WAVES * WAVE), 0, v.stream, arrays_of(v), n, od, src_of, (const float*)*v.fork_rows);
    QS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
