"""DevicePolicy: `model.predict(obs, deterministic=True)` of load_model.py:132 as ONE HIP launch for all environments (k_policy,
csrc/qs_policy.hip), with one parameter row per block of environments for ARS's candidates.

The networks are the reference's: an SB3 PPO MlpPolicy (two tanh layers of 64, a linear action head, a state-independent log_std) and
sb3_contrib's ARS policies (linear without bias, or a small MLP).  Parameters are one float32 device tensor [n_policies, n_params] in
`torch.nn.utils.parameters_to_vector` order (per layer weight [out, in], then bias [out]): the flat theta ARS perturbs.

`from_state_dict` / `load` map SB3's parameter names as stable_baselines3 1.5 / sb3_contrib 1.5 are remembered to write them; neither
package was available to check them against, so a key that is missing raises and lists the keys that were found."""
import ctypes as C

import numpy as np

from . import lib as _lib
from .handle import DeviceHandle, ptr, tensor_arg

ACTIVATIONS = {"none": 0, "tanh": 1, "relu": 2}
MAX_HIDDEN = 4


def layer_shapes(obs_dim, action_dim, net_arch):
    dims = [int(obs_dim)] + [int(w) for w in net_arch] + [int(action_dim)]
    return [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)]


def param_count(obs_dim, action_dim, net_arch, bias=True):
    return sum(o * i + (o if bias else 0) for o, i in layer_shapes(obs_dim, action_dim, net_arch))


def flatten_layers(layers, bias=True):
    """[(weight [out, in], bias [out] or None), ...] -> the flat float32 parameter vector (parameters_to_vector order)"""
    parts = []
    for w, b in layers:
        parts.append(np.asarray(w, np.float32).reshape(-1))
        if bias:
            parts.append(np.asarray(b, np.float32).reshape(-1))
    return np.concatenate(parts)


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _pick(sd, key, shape=None):
    if key not in sd:
        raise KeyError(f"state dict has no '{key}'; its keys are {sorted(sd.keys())}")
    v = _to_numpy(sd[key])
    if shape is not None and tuple(v.shape) != tuple(shape):
        raise ValueError(f"'{key}' has shape {tuple(v.shape)}, expected {tuple(shape)}")
    return v


def layers_from_state_dict(sd, algo="ppo", head="policy"):
    """-> ([(weight, bias or None), ...], log_std or None) from an SB3 policy state dict.  PPO: mlp_extractor.policy_net.{0,2,..} then
    action_net (head="value": mlp_extractor.value_net.* then value_net), log_std; ARS: action_net.{0,2,..} (a bare action_net.weight for
    the linear policy), biases only where the dict has them."""
    if algo == "ppo":
        trunk, last = ("mlp_extractor.policy_net", "action_net") if head == "policy" else ("mlp_extractor.value_net", "value_net")
        if head not in ("policy", "value"):
            raise ValueError(f"head = {head!r} is neither 'policy' nor 'value'")
        layers, i = [], 0
        while f"{trunk}.{i}.weight" in sd:
            layers.append((_pick(sd, f"{trunk}.{i}.weight"), _pick(sd, f"{trunk}.{i}.bias")))
            i += 2
        layers.append((_pick(sd, f"{last}.weight"), _pick(sd, f"{last}.bias")))
        return layers, (_pick(sd, "log_std") if head == "policy" else None)
    if algo == "ars":
        if "action_net.weight" in sd:
            return [(_pick(sd, "action_net.weight"), _to_numpy(sd["action_net.bias"]) if "action_net.bias" in sd else None)], None
        layers, i = [], 0
        while f"action_net.{i}.weight" in sd:
            layers.append((_pick(sd, f"action_net.{i}.weight"), _to_numpy(sd[f"action_net.{i}.bias"]) if f"action_net.{i}.bias" in sd else None))
            i += 2
        if not layers:
            _pick(sd, "action_net.0.weight")
        return layers, None
    raise ValueError(f"algo = {algo!r} is neither 'ppo' nor 'ars'")


def spec_from_layers(layers, log_std=None, activation="tanh", squash_output=False):
    """what DevicePolicy.from_spec builds from: the network's shape and its flat parameter vector, checked layer against layer"""
    bias = layers[0][1] is not None
    for i, (w, b) in enumerate(layers):
        if w.ndim != 2 or (i and w.shape[1] != layers[i - 1][0].shape[0]):
            raise ValueError(f"layer {i}: weight of shape {tuple(w.shape)} does not follow a layer of {layers[i - 1][0].shape[0] if i else '?'} outputs")
        if (b is not None) != bias:
            raise ValueError(f"layer {i}: {'has a bias, layer 0 has none' if bias is False else 'has no bias, layer 0 has one'}")
        if bias and tuple(b.shape) != (w.shape[0],):
            raise ValueError(f"layer {i}: bias of shape {tuple(b.shape)}, expected ({w.shape[0]},)")
    action_dim = layers[-1][0].shape[0]
    if log_std is not None and tuple(np.shape(log_std)) != (action_dim,):
        raise ValueError(f"'log_std' has shape {tuple(np.shape(log_std))}, expected ({action_dim},)")
    return dict(obs_dim=layers[0][0].shape[1], action_dim=action_dim, net_arch=tuple(w.shape[0] for w, _ in layers[:-1]), activation=activation,
                squash_output=bool(squash_output), bias=bias, params=flatten_layers(layers, bias), log_std=None if log_std is None else np.asarray(log_std, np.float32))


def spec_from_module(module):
    from torch import nn
    layers, acts = [], []
    for m in module:
        if isinstance(m, nn.Linear):
            layers.append((_to_numpy(m.weight), None if m.bias is None else _to_numpy(m.bias)))
            acts.append("none")
        elif isinstance(m, (nn.Tanh, nn.ReLU)) and layers and acts[-1] == "none":
            acts[-1] = "tanh" if isinstance(m, nn.Tanh) else "relu"
        else:
            raise ValueError(f"from_module reads Linear layers with one Tanh or ReLU between them, not {type(m).__name__} here")
    if not layers:
        raise ValueError("from_module: no Linear layer")
    hidden = set(acts[:-1])
    if len(hidden) > 1 or acts[-1] == "relu":
        raise ValueError(f"from_module: one activation for all hidden layers and none or Tanh after the last, got {acts}")
    return spec_from_layers(layers, None, hidden.pop() if hidden else "none", acts[-1] == "tanh")


def spec_from_state_dict(sd, algo="ppo", activation="tanh", head="policy"):
    layers, log_std = layers_from_state_dict(sd, algo, head)
    return spec_from_layers(layers, log_std, activation)


def state_dict_from_zip(path):
    import io
    import zipfile
    import torch
    with zipfile.ZipFile(path) as z:
        if "policy.pth" not in z.namelist():
            raise KeyError(f"{path} has no 'policy.pth'; it holds {z.namelist()}")
        return torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu")


class DevicePolicy(DeviceHandle):
    _prefix, _owner = "qs_policy", "policy"

    def __init__(self, obs_dim, action_dim, net_arch=(64, 64), activation="tanh", squash_output=False, bias=True, num_envs=1, n_policies=1,
                 clip=(-1.0, 1.0), device=0):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        net_arch = tuple(int(w) for w in net_arch)
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation = {activation!r} is none of {sorted(ACTIVATIONS)}")
        if len(net_arch) > MAX_HIDDEN:
            raise ValueError(f"net_arch = {net_arch} has more than {MAX_HIDDEN} hidden layers")
        self.obs_dim, self.action_dim, self.net_arch, self.activation = int(obs_dim), int(action_dim), net_arch, activation
        self.squash_output, self.bias, self.num_envs, self.n_policies = bool(squash_output), bool(bias), int(num_envs), int(n_policies)
        lo, hi = (-3.0e38, 3.0e38) if clip is None else (float(clip[0]), float(clip[1]))
        self.clip = (lo, hi)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        d = _lib.QsPolicyDesc(self.num_envs, self.n_policies, self.obs_dim, self.action_dim, len(net_arch), (C.c_int32 * 4)(*net_arch), ACTIVATIONS[activation],
                              int(self.squash_output), int(self.bias), lo, hi)
        self.h = C.c_void_p()
        _lib.check(self.lib.qs_policy_create(C.byref(d), self.device.index or 0, C.byref(self.h)))
        self.n_params = self.lib.qs_policy_param_count(self.h)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._params = None       # the tensor the handle points into: kept alive here
        self.log_std = torch.zeros(self.action_dim, **f32)
        self._actions = torch.zeros((self.num_envs, self.action_dim), **f32)
        self._mean = torch.zeros((self.num_envs, self.action_dim), **f32)
        self._log_prob = torch.zeros(self.num_envs, **f32)

    # ---- parameters
    def set_params(self, params):
        """params: [n_policies, n_params] or [n_params] (one policy for every block), a float32 tensor on this device or a numpy array.
        A [n_policies, n_params] contiguous device tensor is used in place, not copied: writing into it changes the next act()."""
        t = self.torch
        p = params if t.is_tensor(params) else t.as_tensor(np.asarray(params, np.float32))
        if p.dim() == 1:
            p = p.unsqueeze(0).expand(self.n_policies, -1)
        if tuple(p.shape) != (self.n_policies, self.n_params):
            raise ValueError(f"params has shape {tuple(params.shape)}, expected ({self.n_policies}, {self.n_params}) or ({self.n_params},)")
        p = p.to(device=self.device, dtype=t.float32).contiguous()
        _lib.check(self.lib.qs_policy_set_params(self.h, ptr(p)))
        self._params = p

    def get_params(self):
        """the [n_policies, n_params] device tensor act() reads"""
        if self._params is None:
            raise RuntimeError("DevicePolicy.get_params before set_params")
        return self._params

    def set_log_std(self, log_std):
        self.log_std.copy_(self.torch.as_tensor(_to_numpy(log_std), dtype=self.torch.float32).reshape(self.action_dim))

    # ---- inference
    def _arg(self, name, x, shape):
        return tensor_arg(name, x, shape, self.torch.float32, self.device, self._owner, kind_error=TypeError)

    def act(self, obs, eps=None, log_std=None, want_mean=False, want_log_prob=False):
        """-> actions [N, action_dim], clipped; with want_mean / want_log_prob a tuple (actions, mean, log_prob) with None for what was not
        asked for.  eps [N, action_dim] (e.g. torch.randn) makes it a sample mean + exp(log_std) * eps; log_std defaults to the policy's.
        The returned tensors are this object's reused buffers, valid until the next act(); the launch is on torch's current stream."""
        if self._params is None:
            raise RuntimeError("DevicePolicy.act before set_params")
        if want_log_prob and eps is None:
            raise ValueError("want_log_prob needs eps")
        p_obs = self._arg("obs", obs, (self.num_envs, self.obs_dim))
        p_eps = None if eps is None else self._arg("eps", eps, (self.num_envs, self.action_dim))
        ls = self.log_std if log_std is None else log_std
        p_ls = None if eps is None else self._arg("log_std", ls, (self.action_dim,))
        self._stream()
        _lib.check(self.lib.qs_policy_act(self.h, p_obs, p_eps, p_ls, ptr(self._actions), ptr(self._mean) if want_mean else None,
                                          ptr(self._log_prob) if want_log_prob else None))
        if want_mean or want_log_prob:
            return self._actions, (self._mean if want_mean else None), (self._log_prob if want_log_prob else None)
        return self._actions

    def predict(self, obs, state=None, episode_start=None, deterministic=True):
        """SB3's BasePolicy.predict: numpy in -> (numpy actions, None); a device tensor in -> (a copy of the action tensor, None)."""
        t = self.torch
        is_np = not t.is_tensor(obs)
        o = t.as_tensor(np.ascontiguousarray(obs, np.float32), device=self.device) if is_np else obs
        eps = None if deterministic else t.randn((self.num_envs, self.action_dim), dtype=t.float32, device=self.device)
        a = self.act(o.reshape(self.num_envs, self.obs_dim), eps=eps)
        return (a.cpu().numpy() if is_np else a.clone()), None

    # ---- construction from torch / SB3 objects (the reading is spec_from_*, below: host code that needs no device)
    @classmethod
    def from_spec(cls, spec, num_envs, **kw):
        self = cls(spec["obs_dim"], spec["action_dim"], net_arch=spec["net_arch"], activation=spec["activation"], squash_output=spec["squash_output"],
                   bias=spec["bias"], num_envs=num_envs, **kw)
        self.set_params(spec["params"])
        if spec["log_std"] is not None:
            self.set_log_std(spec["log_std"])
        return self

    @classmethod
    def from_module(cls, module, num_envs, **kw):
        """a torch.nn.Sequential of Linear layers with Tanh or ReLU (or nothing) between them; a Tanh after the last Linear = squash_output"""
        return cls.from_spec(spec_from_module(module), num_envs, **kw)

    @classmethod
    def from_state_dict(cls, sd, algo="ppo", num_envs=1, activation="tanh", head="policy", **kw):
        """An SB3 policy's state dict (names as remembered from stable_baselines3 1.5 / sb3_contrib 1.5, see the module docstring; the
        activation is not in a state dict).  head="value" (PPO): the value network as a policy of action_dim 1 without clipping -- read its
        output with act(obs, want_mean=True)."""
        if head == "value":
            kw.setdefault("clip", None)
        return cls.from_spec(spec_from_state_dict(sd, algo, activation, head), num_envs, **kw)

    @classmethod
    def load(cls, path, num_envs, algo="ppo", activation="tanh", head="policy", **kw):
        """an SB3 model .zip: its `policy.pth` is a torch state dict (read with zipfile + torch.load; stable_baselines3 is not imported)"""
        return cls.from_state_dict(state_dict_from_zip(path), algo=algo, num_envs=num_envs, activation=activation, head=head, **kw)

    def close(self):
        super().close()
        self._params = None


# ---- ARS (sb3_contrib/ars/ars.py): plumbing in torch, the candidates' forward passes are DevicePolicy's
def ars_population(theta, deltas, sigma):
    """theta [n_params], deltas [n_delta, n_params] -> [2 n_delta, n_params]: theta + sigma * deltas first, theta - sigma * deltas second"""
    import torch
    return torch.cat([theta + sigma * deltas, theta - sigma * deltas], 0)


def ars_update(theta, deltas, returns_plus, returns_minus, step_size, n_top):
    """ARS._do_one_update: keep the n_top directions with the largest max(r+, r-), step along sum (r+ - r-) delta scaled by
    step_size / (n_top * std of the kept returns + 1e-6).  -> the new theta"""
    import torch
    top = torch.argsort(torch.maximum(returns_plus, returns_minus), descending=True)[:n_top]
    rp, rm = returns_plus[top], returns_minus[top]
    std = torch.cat([rp, rm]).std()
    return theta + step_size / (n_top * std + 1e-6) * ((rp - rm) @ deltas[top])
