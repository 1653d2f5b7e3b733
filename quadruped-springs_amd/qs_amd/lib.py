"""ctypes binding of the C ABI declared in include/qs_amd.h (libqs_hip.so, built by quadruped-springs_amd/build.py).

There is no CPU path: if the library is missing or no HIP device is usable this module raises."""
import ctypes as C
import os

from .config import QsConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QS_LIB_PATH") or os.path.join(_HERE, "libqs_hip.so")   # QS_LIB_PATH: kernel experiments (another build of the same ABI)

ABI_VERSION = 8   # the last QS_ABI_VERSION that changed a struct or an existing entry point: the Structures below are that version's layouts
ABI_LIBRARY = 9   # QS_ABI_VERSION of include/qs_amd.h this file was written against, the number load() demands of the library (9 added entries only)


class HostResult(C.Structure):
    """qs_host_result (include/qs_amd.h): where the results of a host-path step lie in the handle's page-locked host memory."""
    _fields_ = [("obs", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p), ("terminal_rows", C.c_void_p),
                ("terminal_cap", C.c_int32)]


class NormIO(C.Structure):
    """qs_norm_io (include/qs_amd.h): the arrays of a step for qs_norm_step_io and, optionally, where the normalised ones go."""
    _fields_ = [("obs", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p), ("trunc", C.c_void_p), ("term_obs", C.c_void_p), ("tail_rows", C.c_void_p),
                ("tail_cap", C.c_int32),
                ("out_obs", C.c_void_p), ("out_rew", C.c_void_p), ("out_done", C.c_void_p), ("out_trunc", C.c_void_p), ("out_tail", C.c_void_p),
                ("raw_obs", C.c_void_p), ("raw_rew", C.c_void_p), ("tail_count", C.c_void_p)]


class QsCamera(C.Structure):
    """qs_camera (include/qs_amd.h): a camera of qs_render / qs_render_states."""
    _fields_ = [("target", C.c_float * 3), ("distance", C.c_float), ("yaw_deg", C.c_float), ("pitch_deg", C.c_float), ("fov_deg", C.c_float),
                ("near_clip", C.c_float), ("far_clip", C.c_float), ("follow_base", C.c_int32), ("draw_payload", C.c_int32)]


class QsPolicyDesc(C.Structure):
    """qs_policy_desc (include/qs_amd.h): the network of qs_policy_create."""
    _fields_ = [("n_envs", C.c_int32), ("n_policies", C.c_int32), ("obs_dim", C.c_int32), ("action_dim", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * 4), ("activation", C.c_int32), ("squash_output", C.c_int32), ("has_bias", C.c_int32),
                ("clip_lo", C.c_float), ("clip_hi", C.c_float)]


class QsRack(C.Structure):
    """qs_rack (include/qs_amd.h): the rack of qs_create_ex (Quadruped(on_rack=True))."""
    _fields_ = [("on", C.c_int32), ("anchor_pos", C.c_float * 3), ("anchor_quat", C.c_float * 4)]


class QsPpoHyper(C.Structure):
    """qs_ppo_hyper (include/qs_amd.h): the hyper-parameters of qs_ppo_grad and qs_ppo_adam."""
    _fields_ = [("clip_range", C.c_float), ("ent_coef", C.c_float), ("vf_coef", C.c_float), ("max_grad_norm", C.c_float),
                ("normalize_advantage", C.c_int32), ("reserved", C.c_int32),
                ("lr", C.c_double), ("beta_one", C.c_double), ("beta_two", C.c_double), ("adam_eps", C.c_double)]


class SnapshotInfo(C.Structure):
    """struct qs_snapshot_info (include/qs_amd.h): which handles a snapshot's rows fit (qs_amd/snapshot.py hands it on)."""
    _fields_ = [("bytes", C.c_uint64), ("n_envs", C.c_int32), ("row_floats", C.c_int32), ("rec_floats", C.c_int32), ("push_floats", C.c_int32),
                ("obs_dim", C.c_int32), ("layout_version", C.c_int32), ("layout_digest", C.c_uint64), ("config_digest", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# every struct with a body in include/qs_amd.h, by its C name (tests/test_abi_cpu.py holds field types, sizes and offsets to the header and a C compile of it)
STRUCTS = {"qs_config": QsConfig, "qs_rack": QsRack, "qs_host_result": HostResult, "qs_norm_io": NormIO, "qs_camera": QsCamera,
           "qs_policy_desc": QsPolicyDesc, "qs_ppo_hyper": QsPpoHyper, "qs_snapshot_info": SnapshotInfo}

PPO_STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "grad_norm", "refused", "loss")   # QS_PPO_STAT_*

_P, _vp, _i32, _f32, _f64, _ll = C.POINTER, C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong
_out, _u64p, _pd, _desc, _hyper = _P(_vp), _P(C.c_uint64), _P(_f64), _P(QsPolicyDesc), _P(QsPpoHyper)
# The binding, stated once: (entry point, return type, argument types) for every prototype of include/qs_amd.h, in the header's order.  A new
# entry point is its prototype there and its row here; tests/test_abi_cpu.py holds every row to the header, kind by kind.  Array arguments are
# c_void_p (callers pass data pointers as plain integers); POINTER(...) is kept for what callers pass with byref().
SIGNATURES = (
    ("qs_create", _i32, (_P(QsConfig), _i32, _out)),
    ("qs_create_ex", _i32, (_P(QsConfig), _P(QsRack), _i32, _out)),
    ("qs_set_rack", _i32, (_vp, _vp, _i32)),
    ("qs_destroy", None, (_vp,)),
    ("qs_set_stream", _i32, (_vp, _vp)),
    ("qs_reset", _i32, (_vp, _vp)),
    ("qs_reset_to", _i32, (_vp, _vp, _vp)),
    ("qs_get_obs", _i32, (_vp, _vp)),
    ("qs_set_demo", _i32, (_vp, _vp, _i32)),
    ("qs_set_demo_counter", _i32, (_vp, _vp, _vp)),
    ("qs_step", _i32, (_vp,) * 6),
    ("qs_get_state", _i32, (_vp, _vp)),
    ("qs_set_external_wrench", _i32, (_vp, _vp, _vp, _vp, _i32)),
    ("qs_set_state", _i32, (_vp, _vp)),
    ("qs_info_dim", _i32, (_vp, _i32)),
    ("qs_get_info", _i32, (_vp, _i32, _vp)),
    ("qs_set_params", _i32, (_vp, _i32, _vp)),
    ("qs_stats", _i32, (_vp, _u64p, _u64p)),
    ("qs_step_fused", _i32, (_vp, _vp, _vp)),
    ("qs_step_masked", _i32, (_vp,) * 7),
    ("qs_host_step_begin", _i32, (_vp, _vp)),
    ("qs_host_step_end", _i32, (_vp, _P(HostResult))),
    ("qs_counter", _i32, (_vp, _i32, _u64p)),
    ("qs_counters_async", _i32, (_vp, _vp)),
    ("qs_enable_timing", _i32, (_vp, _i32)),
    ("qs_last_step_kernel_ms", _i32, (_vp, _P(_f32))),
    ("qs_settle_lanes", _i32, (_vp, _i32)),
    ("qs_solo_waves", _i32, (_vp, _i32, _f32)),
    ("qs_set_trace", _i32, (_vp, _i32, _vp)),
    ("qs_norm_create", _i32, (_i32, _i32, _f64, _f64, _f64, _f64, _i32, _out)),
    ("qs_norm_destroy", None, (_vp,)),
    ("qs_norm_set_stream", _i32, (_vp, _vp)),
    ("qs_norm_set_stats", _i32, (_vp, _vp, _vp, _f64, _f64, _f64, _f64)),
    ("qs_norm_dims", _i32, (_vp, _P(_i32), _P(_i32), _P(_i32))),
    ("qs_norm_get_stats", _i32, (_vp, _vp, _vp, _pd, _pd, _pd, _pd)),
    ("qs_norm_reset", _i32, (_vp, _vp, _i32, _i32)),
    ("qs_norm_step", _i32, (_vp,) * 5 + (_i32,) * 3 + (_vp,) * 2),
    ("qs_norm_step_masked", _i32, (_vp,) * 6 + (_i32,) * 3 + (_vp,) * 2),
    ("qs_norm_step_io", _i32, (_vp, _P(NormIO), _i32, _i32, _i32)),
    ("qs_host_set_norm", _i32, (_vp, _vp, _i32, _i32, _i32, _vp, _vp)),
    ("qs_render", _i32, (_vp, _vp, _i32, _P(QsCamera), _i32, _i32, _vp, _vp, _vp)),
    ("qs_render_states", _i32, (_vp, _vp, _i32, _P(QsCamera), _i32, _i32, _vp, _vp, _vp, _vp)),
    ("qs_policy_create", _i32, (_desc, _i32, _out)),
    ("qs_policy_destroy", None, (_vp,)),
    ("qs_policy_set_stream", _i32, (_vp, _vp)),
    ("qs_policy_param_count", _i32, (_vp,)),
    ("qs_policy_set_params", _i32, (_vp, _vp)),
    ("qs_policy_act", _i32, (_vp,) * 7),
    ("qs_ac_create", _i32, (_desc, _desc, _i32, _out)),
    ("qs_ac_destroy", None, (_vp,)),
    ("qs_ac_set_stream", _i32, (_vp, _vp)),
    ("qs_ac_set_params", _i32, (_vp, _vp, _vp)),
    ("qs_ac_collect", _i32, (_vp,) * 9),
    ("qs_ac_values", _i32, (_vp,) * 4),
    ("qs_ac_bootstrap", _i32, (_vp, _vp, _vp, _f32, _vp)),
    ("qs_gae", _i32, (_vp,) * 5 + (_i32, _i32, _f32, _f32, _vp, _vp, _vp)),
    ("qs_ppo_create", _i32, (_desc, _desc, _i32, _i32, _out)),
    ("qs_ppo_destroy", None, (_vp,)),
    ("qs_ppo_set_stream", _i32, (_vp, _vp)),
    ("qs_ppo_bind", _i32, (_vp,) * 6),
    ("qs_ppo_grad", _i32, (_vp,) * 6 + (_ll, _vp, _i32, _hyper, _vp, _vp)),
    ("qs_ppo_adam", _i32, (_vp, _vp, _hyper, _i32, _vp)),
    ("qs_ppo_refusals", _i32, (_vp, _u64p)),
    ("qs_ars_create", _i32, (_i32,) * 5 + (_out,)),
    ("qs_ars_destroy", None, (_vp,)),
    ("qs_ars_set_stream", _i32, (_vp, _vp)),
    ("qs_ars_perturb", _i32, (_vp, _vp, _vp, _f32, _vp)),
    ("qs_ars_begin", _i32, (_vp,)),
    ("qs_ars_account", _i32, (_vp, _vp, _vp)),
    ("qs_ars_alive", _i32, (_vp, _P(_i32))),
    ("qs_ars_returns", _i32, (_vp, _f32)),
    ("qs_ars_finish", _i32, (_vp, _vp, _vp, _i32, _f32, _f32)),
    ("qs_ars_get", _i32, (_vp, _i32, _vp)),
    ("qs_mpc_create", _i32, (_i32,) * 5 + (_out,)),
    ("qs_mpc_destroy", None, (_vp,)),
    ("qs_mpc_set_stream", _i32, (_vp, _vp)),
    ("qs_mpc_sample", _i32, (_vp, _vp, _f32)),
    ("qs_mpc_feed", _i32, (_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp)),
    ("qs_mpc_finish", _i32, (_vp, _i32, _f32, _vp)),
    ("qs_mpc_get", _i32, (_vp, _i32, _vp)),
    ("qs_mpc_set_plan", _i32, (_vp, _vp, _vp)),
    ("qs_snapshot_info", _i32, (_vp, _P(SnapshotInfo))),
    ("qs_snapshot", _i32, (_vp, _vp, _vp)),
    ("qs_restore", _i32, (_vp, _vp, _vp)),
    ("qs_fork", _i32, (_vp, _vp)),
    ("qs_norm_get_returns", _i32, (_vp, _vp)),
    ("qs_norm_set_returns", _i32, (_vp, _vp)),
    ("qs_last_error", C.c_char_p, ()),
    ("qs_version", C.c_char_p, ()),
    ("qs_abi_version", _i32, ()),
)
EXPORTS = tuple(name for name, *_ in SIGNATURES)

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python quadruped-springs_amd/build.py` (needs hipcc). "
                           "The simulation step has no CPU fallback.")
    # The library must share ONE HIP runtime with PyTorch (device pointers and streams cross the boundary).  torch
    # wheels bundle their own libamdhip64 / libhsa-runtime64; importing torch first makes the loader satisfy this
    # library's DT_NEEDED entry with the runtime torch already mapped.  Loaded the other way round the process ends up
    # with two HSA runtimes and the second one sees no device (measured on the MI355X box, tools/diag_hip_runtime.py).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    missing = []
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is None:
            missing.append(name)
        else:
            fn.restype, fn.argtypes = restype, argtypes
    # (QS_ALLOW_ABI_MISMATCH=1: the A/B tools that time an older round's library through QS_LIB_PATH on entry points that did not change;
    # the entries such a library lacks stay unbound)
    if os.environ.get("QS_ALLOW_ABI_MISMATCH") != "1":
        have = lib.qs_abi_version() if "qs_abi_version" not in missing else "none (a library of round 4 or earlier)"
        rebuild = "rebuild it (python quadruped-springs_amd/build.py --force)"
        if have != ABI_LIBRARY:
            raise RuntimeError(f"{LIB_PATH} speaks ABI {have}, this binding was written against ABI {ABI_LIBRARY} of include/qs_amd.h: {rebuild}")
        if missing:
            raise RuntimeError(f"{LIB_PATH} reports ABI {have} and does not export {', '.join(missing)}, which include/qs_amd.h declares: {rebuild}")
    _lib = lib
    return lib


def source_sha(lib=None):
    """The fingerprint of the source tree the loaded library says it was compiled from (build.py's source_fingerprint(), passed to the
    compiler as QS_SOURCE_SHA and returned inside qs_version()); None for a library that does not say (round 5 or earlier)."""
    import re
    m = re.search(r"source ([0-9a-f]{64})", (lib or load()).qs_version().decode())
    return m.group(1) if m else None


def check(rc):
    if rc != 0:
        raise RuntimeError("qs_amd: " + load().qs_last_error().decode())
