// Host-side helpers shared by the C-ABI translation units (qs_hip.hip, qs_norm.hip, qs_render.hip, qs_policy.hip, qs_ppo.hip, qs_snapshot.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>

// The error path of every entry point: the reason goes into the calling thread's text (qs_last_error; defined in qs_hip.hip), the code is returned.
extern thread_local char qs_g_err[512];
#define QS_FAIL(code, ...) do { snprintf(qs_g_err, sizeof(qs_g_err), __VA_ARGS__); return (code); } while (0)
#define QS_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) QS_FAIL(-2, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)
// 0 if `device` is a visible HIP device, or -3 with the reason in qs_g_err (there is no CPU path); every *_create asks it first (qs_hip.hip)
int qs_check_device(int device);

// Entry points run on the handle's device whatever the calling thread's current device is, and leave that as they found it.
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(int d) : dev(d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define QS_ON_DEVICE(h) DeviceGuard qs_guard_((h)->device)

// What qs_render (qs_render.hip) reads of a simulation handle (defined in qs_hip.hip, which owns the handle's layout).
struct qs_handle;
struct QsRenderView {
    const float* rec;              // records [n_envs][QS_REC]
    int n_envs, payload_soft, device;
    hipStream_t stream;
    unsigned long long* refused;   // device counter: 1 + the first position of env_ids that held an id out of range, 0 if none
};
int qs_render_view(qs_handle* h, QsRenderView* v);

// What the snapshot entries (qs_snapshot.hip) read and write of a simulation handle.
struct qs_config;
struct qs_rack;
struct QsSnapshotView {
    const qs_config* cfg; const qs_rack* rack;
    float* rec; float* push; float* obs; float* term;   // records [N][QS_REC], push rows [N][QS_PUSH_F], last and terminal observations [N][obs_dim]
    int* la_cur; int* la_handed; int la_K;              // the look-ahead window (null / 0 without one)
    int device;
    hipStream_t stream;
    unsigned long long* fork_refused;   // device counter: 1 + the first environment whose source qs_fork refused, 0 if none
    float** fork_rows;                  // the handle's staging rows of qs_fork [N][row_floats] (allocated at the first fork, freed by qs_destroy)
    int* push_live;                     // qs_restore sets it: a push may be pending in the restored rows
};
int qs_snapshot_view(qs_handle* h, QsSnapshotView* v);
