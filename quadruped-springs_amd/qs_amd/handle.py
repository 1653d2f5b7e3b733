"""What every device handle of this package does the same way, stated once: the checks and conversions of tensor arguments (plain
functions: no library, no device needed) and DeviceHandle, the base of a Python object that owns one handle of the C ABI (stream
hand-off, argument check, getter, lifecycle).  A new handle starts here and from the skeleton in csrc/qs_host.h."""
import ctypes as C
from functools import cached_property

import numpy as np
import torch      # (at import, unlike elsewhere in the package: tensor_arg runs several times per environment step)

from . import lib as _lib


def ptr(t):
    """the tensor's memory as the library takes it; None stays None (an optional argument)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def tensor_arg(name, x, shape, dtype, device, owner, kind_error=ValueError):
    """-> ptr(x) for a contiguous tensor of `dtype` and `shape` on `device`; anything else raises before any launch (kind_error for what
    is no tensor or has another dtype, ValueError for the rest).  owner: the word for the object in the message ("learner", "policy")"""
    if not torch.is_tensor(x):
        raise kind_error(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype != dtype:
        raise kind_error(f"{name} must be {str(dtype).rpartition('.')[2]}, got {x.dtype}")   # ("float32": the name without its module)
    if x.device != device:
        raise ValueError(f"{name} is on {x.device}, this {owner} on {device}")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(x.shape)}, expected {tuple(shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return C.c_void_p(x.data_ptr())


def to_device_nowait(array, device):
    """a host array on `device` without a synchronous copy: page-locked staging (the caching host allocator keeps the staging block until
    the copy on the stream has read it), then an asynchronous copy"""
    h = torch.from_numpy(np.ascontiguousarray(array))
    return h if torch.device(device).type == "cpu" else h.pin_memory().to(device, non_blocking=True)


def env_mask(indices, n, device):
    """Who is meant, as the uint8 [n] tensor on `device` the kernels read (None: no mask = everybody).  A bool or uint8 tensor on the device
    is a mask: shape (n,), used as it is.  Any other tensor on the device holds ids and is not looked at on the host (index_fill_ takes
    the value as a kernel argument; `m[idx] = 1` stages a host scalar and synchronises).  Anything on the host -- an int, a list, an
    array, a host tensor -- holds ids, which are checked here and go over through page-locked staging.  Nothing waits for the device."""
    if indices is None:
        return None
    if not isinstance(device, torch.device):
        device = torch.device(device)
    if torch.is_tensor(indices) and indices.device == device:
        if indices.dtype in (torch.bool, torch.uint8):
            if tuple(indices.shape) != (n,):
                raise ValueError(f"a mask must have shape {(n,)}, got {tuple(indices.shape)}")
            m = indices.contiguous()
            return m.view(torch.uint8) if m.dtype == torch.bool else m
        return torch.zeros(n, dtype=torch.uint8, device=device).index_fill_(0, indices.to(torch.int64).reshape(-1), 1)
    if isinstance(indices, (np.ndarray, torch.Tensor)):
        indices = indices.tolist()
    idx = np.asarray(indices if isinstance(indices, (int, np.integer)) else list(indices), np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError(f"environment ids must lie in [0, {n}), got {idx.min()} .. {idx.max()}")
    m = np.zeros(n, np.uint8)
    m[idx] = 1
    return to_device_nowait(m, device)


def active_mask(active, num_envs, device):
    """step_tensor's `active` as the contiguous uint8 [N] tensor the step kernel reads: a bool or uint8 tensor of shape [num_envs] on
    `device`; anything else raises ValueError before any launch"""
    if not torch.is_tensor(active):
        raise ValueError(f"active must be a bool or uint8 torch tensor of shape {(num_envs,)} on {device}, got {type(active).__name__}")
    if active.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"active must be a bool or uint8 tensor, got {active.dtype}")
    if tuple(active.shape) != (num_envs,):
        raise ValueError(f"active must have shape {(num_envs,)}, got {tuple(active.shape)}")
    if active.device != torch.device(device):
        raise ValueError(f"active is on {active.device}, the environments on {device}")
    a = active.contiguous()
    return a.view(torch.uint8) if a.dtype == torch.bool else a


def takes_active(env):
    """whether env.step_tensor has the active= keyword (QuadrupedVecEnv, DeviceVecNormalize); asked once, in a constructor"""
    import inspect
    try:
        return "active" in inspect.signature(env.step_tensor).parameters
    except (AttributeError, TypeError, ValueError):
        return False


def auto_reset_of(env):
    """True / False where the environment (or what it wraps) says, None where it does not"""
    e = env
    while e is not None:
        if hasattr(e, "auto_reset"):
            return bool(e.auto_reset)
        if hasattr(e, "cfg") and hasattr(e.cfg, "auto_reset"):
            return bool(e.cfg.auto_reset)
        e = getattr(e, "venv", None)
    return None


def raw_reward_of(env, rew):
    """the reward of the step that returned `rew` before any normalisation: a DeviceVecNormalize keeps it in old_reward"""
    return env.old_reward if hasattr(env, "venv") and hasattr(env, "old_reward") else rew


class DeviceHandle:
    """An object with self.lib (the loaded library), self.torch, self.device and self.h, a handle of the C ABI's family `_prefix`
    ({prefix}_create / _set_stream / _destroy).  `_owner` is the word for it in the messages of _arg."""
    _prefix = None
    _owner = "handle"

    @cached_property
    def _set_stream(self):
        return getattr(self.lib, self._prefix + "_set_stream")

    def _stream(self):
        """the next launches of this handle go onto torch's current stream of its device"""
        _lib.check(self._set_stream(self.h, C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)))

    def _arg(self, name, x, shape, dtype=None):
        return tensor_arg(name, x, shape, dtype or self.torch.float32, self.device, self._owner)

    def _get(self, what, table, out):
        """out[what] filled with the handle's `what` ({prefix}_get by table[what]): a reused buffer, a stream-ordered copy"""
        buf = out[what]
        self._stream()
        _lib.check(getattr(self.lib, self._prefix + "_get")(self.h, table[what], ptr(buf)))
        return buf

    def close(self):
        """frees the handle ({prefix}_destroy waits for its stream first); a second call does nothing"""
        h = vars(self).get("h")          # (not getattr: a wrapper's __getattr__ would answer with the handle of what it wraps)
        if h:
            self.h = C.c_void_p()        # later calls reach the library with a null handle and fail with its error text
            getattr(self.lib, self._prefix + "_destroy")(h)

    _free = close                        # what __del__ does: the handle alone (a subclass's close() may close more than the object owns)

    def __del__(self):
        try:
            self._free()
        except Exception:  # noqa: BLE001  (interpreter shutdown: the library may be gone already)
            pass
