"""EnvSnapshot: the environments of a QuadrupedVecEnv as one float32 row each (include/qs_amd.h qs_snapshot; layout in csrc/qs_snapshot.h),
with the fields of qs_snapshot_info that say which handles the rows fit, and `extras` for what the wrappers around the environment carry.

save() / load() use one .npz: the rows (as their uint32 bit patterns: NaN payloads and negative zeros survive), one JSON header, and one
entry per array of `extras`.  numpy only; load() lands on the CPU and QuadrupedVecEnv.restore moves the rows to the device."""
import json

import numpy as np

from .lib import SnapshotInfo  # noqa: F401  (the Structure lies with the other mirrors of the header; importable from here as before)

INFO_FIELDS = ("bytes", "n_envs", "row_floats", "rec_floats", "push_floats", "obs_dim", "layout_version", "layout_digest", "config_digest")
# the fields two snapshots / handles must share for rows to fit (in the order they are compared and named), then what makes a resume exact
LAYOUT_FIELDS = ("n_envs", "row_floats", "rec_floats", "push_floats", "obs_dim", "layout_version", "layout_digest")
FORMAT = 1


def first_difference(have, want, strict=True):
    """the first field in which the header `have` (of a snapshot) does not fit `want` (of a handle), or None: the layout fields always,
    config_digest under strict"""
    for k in LAYOUT_FIELDS + (("config_digest",) if strict else ()):
        if int(have[k]) != int(want[k]):
            return k
    return None


def check_fits(have, want, strict=True):
    k = first_difference(have, want, strict)
    if k is not None:
        hint = " (strict=True demands the same configuration, seed included; strict=False takes any snapshot of the same layout)" if k == "config_digest" else ""
        raise ValueError(f"the snapshot does not fit this environment: {k} is {int(have[k])}, the environment's is {int(want[k])}{hint}")


def _flatten(value, path, arrays):
    """extras -> a JSON-able tree whose arrays (numpy, torch) and nested snapshots are references into `arrays`"""
    if isinstance(value, EnvSnapshot):
        return {"__snapshot__": value._pack(path, arrays)}
    if isinstance(value, dict):
        return {"__dict__": {str(k): _flatten(v, f"{path}/{k}", arrays) for k, v in value.items()}}
    if isinstance(value, (list, tuple)):
        return {"__list__": [_flatten(v, f"{path}/{i}", arrays) for i, v in enumerate(value)]}
    if hasattr(value, "detach") and hasattr(value, "cpu"):   # a torch tensor
        value = value.detach().cpu().numpy()
    if isinstance(value, np.ndarray):
        arrays[path] = value
        return {"__array__": path}
    if isinstance(value, np.generic):
        value = value.item()
    if value is None or isinstance(value, (bool, int, float, str)):
        return value
    raise TypeError(f"extras{path}: cannot save a {type(value).__name__}")


def _unflatten(node, z):
    if isinstance(node, dict):
        if "__snapshot__" in node:
            return EnvSnapshot._unpack(node["__snapshot__"], z)
        if "__dict__" in node:
            return {k: _unflatten(v, z) for k, v in node["__dict__"].items()}
        if "__list__" in node:
            return [_unflatten(v, z) for v in node["__list__"]]
        if "__array__" in node:
            return z[node["__array__"]]
    return node


class EnvSnapshot:
    def __init__(self, rows, info, extras=None):
        """rows: float32 tensor [n_envs, row_floats] on any device; info: the qs_snapshot_info fields as a dict; extras: a dict for wrappers
        (DeviceVecNormalize keeps its statistics and returns there, ReferenceStateInitVecEnv its generator's state)"""
        self.rows = rows
        self.info = {k: int(info[k]) for k in INFO_FIELDS}
        self.extras = {} if extras is None else extras

    def __getattr__(self, name):   # snap.n_envs, snap.layout_digest, ...
        if name in INFO_FIELDS:
            return self.__dict__["info"][name]
        raise AttributeError(name)

    def _pack(self, path, arrays):
        rows = self.rows
        if hasattr(rows, "detach"):
            rows = rows.detach().cpu().numpy()
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        arrays[path + "/rows"] = rows.view(np.uint32)
        # (the digests are 64-bit: JSON numbers beyond 2^53 do not survive every reader, so they travel as strings)
        return {"rows": path + "/rows", "info": {k: str(v) for k, v in self.info.items()}, "extras": _flatten(self.extras, path + "/extras", arrays)}

    @classmethod
    def _unpack(cls, node, z):
        import torch
        rows = np.ascontiguousarray(z[node["rows"]]).view(np.float32)
        return cls(torch.from_numpy(rows.copy()), {k: int(v) for k, v in node["info"].items()}, _unflatten(node["extras"], z))

    def save(self, path):
        arrays = {}
        header = {"format": FORMAT, "snapshot": self._pack("", arrays)}
        with open(path, "wb") as f:   # (a file object: np.savez would append ".npz" to a bare name)
            np.savez(f, header=np.frombuffer(json.dumps(header).encode(), dtype=np.uint8), **{"a" + k: v for k, v in arrays.items()})

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            header = json.loads(bytes(z["header"]).decode())
            if header.get("format") != FORMAT:
                raise ValueError(f"{path}: snapshot file format {header.get('format')!r}, this build reads {FORMAT}")
            return cls._unpack(header["snapshot"], {k[1:]: z[k] for k in z.files if k != "header"})
