// Host-side helpers shared by the C-ABI translation units: the error path, the device guard and the views of a simulation handle (qs_hip.hip,
// qs_render.hip, qs_snapshot.hip), and the skeleton of a small handle -- create, destroy, set_stream, launch, copy out -- for qs_norm.hip,
// qs_policy.hip, qs_ppo.hip, qs_ppo_train.hip, qs_ars.hip and qs_mpc.hip (qs_hip.hip's own create and destroy are not of that kind: partial
// build, host path, look-ahead).  A new handle starts from the skeleton.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

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

// ---- the skeleton of a handle H { int device; hipStream_t stream; ... }
// *_create, first half: *h = a zero-filled H on `device` (after the caller's own argument checks); 0, or the code with the reason in qs_g_err
template <class H> int qs_new_handle(H** out, int device, H** h) {
    if (!out) QS_FAIL(-1, "null argument");
    if (int rc = qs_check_device(device)) return rc;
    *h = new (std::nothrow) H();
    if (!*h) QS_FAIL(-4, "out of host memory");
    memset(*h, 0, sizeof(H));
    (*h)->device = device;
    return 0;
}

// *_create, second half: the handle's device arrays, zero-filled (a getter before the first launch reads zeros, not what the allocator left).
// The first error sticks and skips the rest; the caller may put a HIP call of its own into the chain through `e`.
struct ZeroedAlloc {
    hipError_t e = hipSuccess;
    template <class T> void operator()(T** p, size_t count) {
        if (e == hipSuccess) e = hipMalloc((void**)p, count * sizeof(T));
        if (e == hipSuccess) e = hipMemset(*p, 0, count * sizeof(T));
    }
    // false if every step succeeded; otherwise qs_g_err = "<what>: <HIP's reason>" and the caller destroys the handle and returns -2
    __attribute__((format(printf, 2, 3))) bool failed(const char* what, ...) {
        if (e == hipSuccess) return false;
        va_list ap;
        va_start(ap, what);
        const int n = vsnprintf(qs_g_err, sizeof(qs_g_err), what, ap);
        va_end(ap);
        if (n >= 0 && (size_t)n < sizeof(qs_g_err)) snprintf(qs_g_err + n, sizeof(qs_g_err) - n, ": %s", hipGetErrorString(e));
        return true;
    }
};

// *_destroy: waits for the handle's stream, then free_all(h) (the hipFree of every device array; null ones are fine) and the handle itself
template <class H, class FreeAll> void qs_delete_handle(H* h, FreeAll free_all) {
    if (!h) return;
    QS_ON_DEVICE(h);
    hipStreamSynchronize(h->stream);
    free_all(h);
    delete h;
}

// *_set_stream
template <class H> int qs_set_stream_of(H* h, void* s) { if (!h) QS_FAIL(-1, "null handle"); h->stream = (hipStream_t)s; return 0; }

// the grid of one lane per element
inline unsigned qs_blocks(long long n, int block) { return (unsigned)((n + block - 1) / block); }
// behind every hipLaunchKernelGGL
#define QS_LAUNCHED() QS_HIP(hipGetLastError())

// *_get: every file maps its `what` to a span of the handle's memory; the stream-ordered copy into the caller's device buffer is this
struct QsSpan { const void* src; size_t bytes; };
template <class H> int qs_copy_out(H* h, QsSpan span, void* dev_out) {
    const void* src = span.src;
    const size_t bytes = span.bytes;
    QS_ON_DEVICE(h);
    QS_HIP(hipMemcpyAsync(dev_out, src, bytes, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

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
