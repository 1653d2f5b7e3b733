// qs_snapshot.h -- the row of a device snapshot and the lane-level copies of k_snapshot / k_restore / k_fork_gather / k_fork (qs_snapshot.hip),
// shared with their TEST-ONLY host build (tests/test_snapshot_cpu.py compiles this header with g++ and runs the lanes one after the other).
//
// ONE ROW PER ENVIRONMENT, float32, `row_floats(obs_dim)` long:
//
//     [ record: QS_REC | push row: PUSH_F | last observation: obs_dim | terminal observation: obs_dim | zero pad to a multiple of 4 ]
//       0                QS_REC             QS_REC + PUSH_F             QS_REC + PUSH_F + obs_dim
//
//   record                the environment's whole record (qs_layout.h), its unused floats [QS_REC_END, QS_REC) included: everything a step reads
//   push row              qs_set_external_wrench's row: force 3, torque 3, remaining substeps, frame
//   last observation      what qs_get_obs answers with
//   terminal observation  QS_INFO_TERMINAL_OBS
// A row starts on 16 bytes (row_floats is a multiple of 4), and so do its record and its push row: those 74 float4 move as 16-byte accesses,
// consecutive lanes taking consecutive float4 (a record is a 1152-byte row on 128-byte lines, a push row 32 bytes).  The observation rows of
// the handle ([N, obs_dim]) and the terminal observation inside a row start on 16 bytes only when obs_dim is a multiple of 4, so both
// observation parts move as single floats, lane i taking float i (obs_dim <= 64 = one wave).
// Whoever changes this layout or qs_layout.h bumps LAYOUT_VERSION: it is hashed into qs_snapshot_info::layout_digest, which refuses older rows.
//
// A FORK (qs_fork: environment i becomes a copy of environment s) moves the same row from s to i EXCEPT the two record fields that are the
// identity of i and stay its own:
//     R_EPISODE      keys the randomizer draws of i's resets and names the look-ahead slots i takes (qs_hip.hip lookahead_take)
//     R_TOTAL_STEPS  keys i's observation-noise stream
// fork_keeps() says so once; everything else -- R_SIM_STEP and R_ENV_STEP included, they are the age of the episode that was copied -- is s's.
//
// Every copy is written for ONE LANE of a wave that owns the row: all of the lane's loads are issued before its first store (the rule of
// copy_settled, qs_hip.hip: written load-store-load-store a row is a chain of trips to memory, one after the other).
#pragma once
#include <stdint.h>
#include "qs_layout.h"

#if defined(__HIPCC__)
#define QSN_HD __host__ __device__ __forceinline__
#else
#define QSN_HD inline
#endif

namespace qs {
namespace snap {

enum { LAYOUT_VERSION = 1 };
enum { PUSH_F = 8 /* = QS_PUSH_F (qs_hip.hip) */, MAX_OBS = 64, WAVE = 64 };
enum { REC_V4 = QS_REC / 4, PUSH_V4 = PUSH_F / 4, VEC4 = REC_V4 + PUSH_V4, ROUNDS4 = (VEC4 + WAVE - 1) / WAVE };
static_assert(QS_REC % 4 == 0 && PUSH_F % 4 == 0, "record and push row are whole float4");
static_assert(MAX_OBS <= WAVE, "one lane per observation float");
// the kept fields sit in the float4 that lanes R_EPISODE / 4 and R_TOTAL_STEPS / 4 move in round 0
static_assert(R_EPISODE % 4 == 3 && R_TOTAL_STEPS % 4 == 0 && R_TOTAL_STEPS / 4 < WAVE, "where a fork's kept fields lie in their float4");

QSN_HD int push_off() { return QS_REC; }
QSN_HD int obs_off() { return QS_REC + PUSH_F; }
QSN_HD int term_off(int od) { return QS_REC + PUSH_F + od; }
QSN_HD int used_floats(int od) { return QS_REC + PUSH_F + 2 * od; }
QSN_HD int row_floats(int od) { return (used_floats(od) + 3) & ~3; }
QSN_HD bool fork_keeps(int rec_float) { return rec_float == R_EPISODE || rec_float == R_TOTAL_STEPS; }

// where float k of a row lives in the handle (the tests' map of the layout; the kernels do not go through it)
enum { SEG_REC = 0, SEG_PUSH = 1, SEG_OBS = 2, SEG_TERM = 3, SEG_PAD = 4 };
QSN_HD int segment_of(int k, int od, int* off) {
    if (k < push_off()) { *off = k; return SEG_REC; }
    if (k < obs_off()) { *off = k - push_off(); return SEG_PUSH; }
    if (k < term_off(od)) { *off = k - obs_off(); return SEG_OBS; }
    if (k < used_floats(od)) { *off = k - term_off(od); return SEG_TERM; }
    *off = k - used_floats(od);
    return SEG_PAD;
}

struct alignas(16) F4 { float x, y, z, w; };
// the handle's arrays a row is made of
struct Arrays { float* rec; float* push; float* obs; float* term; };

#if defined(__HIP_DEVICE_COMPILE__)
// (keeps the loaded values in front of the predicated stores: without a use of its own the compiler sinks each load into its store's branch)
__device__ __forceinline__ void keep(const F4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }
__device__ __forceinline__ void keep(float v) { asm volatile("" ::"v"(v)); }
#else
inline void keep(const F4&) {}
inline void keep(float) {}
#endif

// One lane's share of a row's move between environment `env` of the handle and `row`.
//   IN = false: handle -> row (k_snapshot; k_fork_gather with IDENT: the row then carries the kept fields of environment `ident`, the
//               destination, in the place of env's -- it is what `ident` becomes)
//   IN = true:  row -> handle (k_restore, k_fork)
// Returns the row's R_EPISODE field in the lane that moved it (lane R_EPISODE / 4; k_restore re-seats the look-ahead window with it).
template <bool IN, bool IDENT>
QSN_HD float move_row(int lane, const Arrays& a, int env, int ident, float* row, int od) {
    F4* const rec4 = reinterpret_cast<F4*>(a.rec + (size_t)env * QS_REC);
    F4* const push4 = reinterpret_cast<F4*>(a.push + (size_t)env * PUSH_F);
    F4* const row4 = reinterpret_cast<F4*>(row);
    F4 v[ROUNDS4];
#pragma unroll
    for (int r = 0; r < ROUNDS4; r++) {
        const int q = lane + r * WAVE, qq = q < VEC4 ? q : 0;     // (beyond the range: the first float4 again, never stored)
        const F4* h = qq < REC_V4 ? rec4 + qq : push4 + (qq - REC_V4);
        v[r] = IN ? row4[qq] : *h;
    }
    const int l = lane < od ? lane : 0;
    float* const ho = a.obs + (size_t)env * od + l;
    float* const ht = a.term + (size_t)env * od + l;
    float* const ro = row + obs_off() + l;
    float* const rt = row + term_off(od) + l;
    const float o = IN ? *ro : *ho, t = IN ? *rt : *ht;
    float k_ep = 0.0f, k_ts = 0.0f;
    if (IDENT) {
        const float* mine = a.rec + (size_t)ident * QS_REC;
        k_ep = mine[R_EPISODE]; k_ts = mine[R_TOTAL_STEPS];
    }
#pragma unroll
    for (int r = 0; r < ROUNDS4; r++) keep(v[r]);
    keep(o); keep(t);
    if (IDENT) {
        keep(k_ep); keep(k_ts);
        if (lane == R_EPISODE / 4) v[0].w = k_ep;
        if (lane == R_TOTAL_STEPS / 4) v[0].x = k_ts;
    }
#pragma unroll
    for (int r = 0; r < ROUNDS4; r++) {
        const int q = lane + r * WAVE;
        if (q < VEC4) {
            F4* h = q < REC_V4 ? rec4 + q : push4 + (q - REC_V4);
            if (IN) *h = v[r]; else row4[q] = v[r];
        }
    }
    if (lane < od) {
        if (IN) { *ho = o; *ht = t; } else { *ro = o; *rt = t; }
    }
    if (!IN && lane < row_floats(od) - used_floats(od)) row[used_floats(od) + lane] = 0.0f;
    return v[0].w;
}

// FNV-1a, 64 bit: the digests of qs_snapshot_info
QSN_HD uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

// qs_fork: environment i takes a row from source s (-1 or i itself: left alone; outside [-1, n): refused)
QSN_HD bool fork_takes(int i, int s, int n) { return s >= 0 && s < n && s != i; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The four kernels on the host, lane after lane (TEST ONLY).  rows: [n][row_floats(od)]; mask: n bytes or null.
inline void host_snapshot(const Arrays& a, int n, int od, const uint8_t* mask, float* rows) {
    for (int e = 0; e < n; e++)
        if (!mask || mask[e])
            for (int lane = 0; lane < WAVE; lane++) move_row<false, false>(lane, a, e, e, rows + (size_t)e * row_floats(od), od);
}
inline void host_restore(const Arrays& a, int n, int od, const uint8_t* mask, float* rows) {
    for (int e = 0; e < n; e++)
        if (!mask || mask[e])
            for (int lane = 0; lane < WAVE; lane++) move_row<true, false>(lane, a, e, e, rows + (size_t)e * row_floats(od), od);
}
// qs_fork: gather every destination's row into `staging` ([n][row_floats(od)]), then scatter; returns 1 + the first refused environment, or 0
inline int host_fork(const Arrays& a, int n, int od, const int32_t* src_of, float* staging) {
    int refused = 0;
    for (int i = 0; i < n; i++) {
        if (src_of[i] < -1 || src_of[i] >= n) { if (!refused) refused = 1 + i; continue; }
        if (fork_takes(i, src_of[i], n))
            for (int lane = 0; lane < WAVE; lane++) move_row<false, true>(lane, a, src_of[i], i, staging + (size_t)i * row_floats(od), od);
    }
    for (int i = 0; i < n; i++)
        if (fork_takes(i, src_of[i], n))
            for (int lane = 0; lane < WAVE; lane++) move_row<true, false>(lane, a, i, i, staging + (size_t)i * row_floats(od), od);
    return refused;
}
#endif

}  // namespace snap
}  // namespace qs
