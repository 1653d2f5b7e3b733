"""float64 numpy reference of policy inference (csrc/qs_policy.h) with a running error bound for the float32 computation, the cases the
parity tests run, and the record they keep (profiles/policy_parity.json).

The bound, per output element (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1, for a chain of K fused multiply-adds
that starts from the bias):   e(l+1) = |W_l| e_l + gamma_(K+1) (|W_l| |h_l| + |b_l|),   gamma_n = n u / (1 - n u),   u = 2^-24,   e_0 = 0
(the observation is given in float32).  relu and the clamp are 1-Lipschitz and exact.  tanh is 1-Lipschitz and adds its implementation's
own error c u |tanh|: c = 2 x the largest |tanhf(x) - tanh(x)| / ulp measured over 10^6 points of [-10, 10] on the host emulation's libm
and on the device (no ulp figure for tanhf was found in the ROCm documentation of the build image); an error of m ulp is at most
2 m u |tanh|, so c = 2 m is what the measurements themselves support.  Both measurements are kept in profiles/policy_parity.json."""
import json
import os

import numpy as np

U = 2.0 ** -24
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(REPO, "profiles", "policy_parity.json")


def gamma(n):
    return n * U / (1.0 - n * U)


def load_record():
    with open(PARITY_JSON) as f:
        return json.load(f)


def tanh_c(rec=None):
    """c of the bound: 2 x the larger of the measured ulp errors of tanhf (a side not measured yet counts as absent)"""
    m = (rec or load_record())["tanhf_max_ulp_error"]
    return 2.0 * max(v for v in m.values() if v is not None)


def record(section, key, value):
    """profiles/policy_parity.json[section][key] = value (best effort: a read-only tree is no test failure)"""
    try:
        rec = load_record()
        rec.setdefault(section, {})[key] = value
        tmp = "%s.%d.tmp" % (PARITY_JSON, os.getpid())
        with open(tmp, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        os.replace(tmp, PARITY_JSON)
    except OSError:
        pass


def tanh_points(n=1_000_000):
    return np.linspace(-10.0, 10.0, n).astype(np.float32)


def max_ulp_error(x32, y32):
    """max |y32 - tanh(x32)| / ulp(tanh(x32)) with tanh in float64 and ulp of the float32 nearest to it"""
    ref = np.tanh(x32.astype(np.float64))
    return float(np.max(np.abs(y32.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)))


def split_params(theta, obs_dim, action_dim, net_arch, bias):
    """one policy's flat row -> [(W [out, in], b [out] or None), ...] (parameters_to_vector order)"""
    dims = [obs_dim] + list(net_arch) + [action_dim]
    out, off = [], 0
    for i in range(len(dims) - 1):
        o, k = dims[i + 1], dims[i]
        W = theta[off:off + o * k].reshape(o, k); off += o * k
        b = None
        if bias:
            b = theta[off:off + o]; off += o
        out.append((W, b))
    assert off == theta.size
    return out


def forward(params, obs, obs_dim, action_dim, net_arch, activation, squash_output, bias, n_policies, c):
    """params [P, n_params] float32, obs [N, obs_dim] float32 -> mean [N, A] float64 and its error bound [N, A] for the float32 result"""
    n = obs.shape[0]
    n_per = n // n_policies
    mean, bound = np.zeros((n, action_dim)), np.zeros((n, action_dim))
    for p in range(n_policies):
        h = obs[p * n_per:(p + 1) * n_per].astype(np.float64)
        e = np.zeros_like(h)
        layers = split_params(np.asarray(params[p], np.float64), obs_dim, action_dim, net_arch, bias)
        for li, (W, b) in enumerate(layers):
            last = li == len(layers) - 1
            kind = ("tanh" if squash_output else "none") if last else activation
            aW = np.abs(W)
            z = h @ W.T + (0.0 if b is None else b)
            e = e @ aW.T + gamma(W.shape[1] + 1) * (np.abs(h) @ aW.T + (0.0 if b is None else np.abs(b)))
            if kind == "tanh":
                h = np.tanh(z)
                e = e + c * U * np.abs(h)
            elif kind == "relu":
                h = np.maximum(z, 0.0)
            else:
                h = z
        mean[p * n_per:(p + 1) * n_per], bound[p * n_per:(p + 1) * n_per] = h, e
    return mean, bound


# ---- the cases of the parity tests: four networks x two weight scales, each over action_dim x P x environments per policy
NETS = {
    "ars_linear": dict(obs_dim=28, net_arch=(), activation="none", bias=False),
    "relu16": dict(obs_dim=28, net_arch=(16,), activation="relu", bias=True),
    "tanh64x64": dict(obs_dim=28, net_arch=(64, 64), activation="tanh", bias=True),
    "tanh256x4": dict(obs_dim=64, net_arch=(256, 256, 256, 256), activation="tanh", bias=True),
}
SCALES = (1.0, 10.0)             # x 10: tanh saturates and the clamp to [-1, 1] bites
ACTION_DIMS = (4, 5, 6, 12)
POLICIES = (1, 2, 64)
ENVS_PER_POLICY = (32, 20)       # a multiple of the kernel's 16-environment tile, and not (N = 40 at P = 2)


def make_params(rng, obs_dim, action_dim, net_arch, bias, n_policies, scale=1.0):
    """torch.nn.Linear's initial range, uniform(-1 / sqrt(in), 1 / sqrt(in)) for weights and biases, times `scale`"""
    dims = [obs_dim] + list(net_arch) + [action_dim]
    rows = []
    for _ in range(n_policies):
        parts = []
        for i in range(len(dims) - 1):
            r = scale / np.sqrt(dims[i])
            parts.append(rng.uniform(-r, r, dims[i + 1] * dims[i]))
            if bias:
                parts.append(rng.uniform(-r, r, dims[i + 1]))
        rows.append(np.concatenate(parts))
    return np.asarray(rows, np.float32)


def make_obs(rng, n, obs_dim):
    """normalised observations as VecNormalize hands them out: unit normal, clipped to +-10"""
    return np.clip(rng.standard_normal((n, obs_dim)) * 1.5, -10.0, 10.0).astype(np.float32)


def cases(net_name, scale):
    """yields (tag, dict(obs_dim, action_dim, net_arch, activation, squash_output, bias, n_policies), params, obs)"""
    net = NETS[net_name]
    seed = sorted(NETS).index(net_name) * 10 + int(scale)
    for a in ACTION_DIMS:
        for P in POLICIES:
            for n_per in ENVS_PER_POLICY:
                rng = np.random.default_rng([seed, a, P, n_per])
                kw = dict(net, action_dim=a, squash_output=False, n_policies=P)
                params = make_params(rng, net["obs_dim"], a, net["net_arch"], net["bias"], P, scale)
                yield f"{net_name}-x{scale:g}-A{a}-P{P}-n{n_per}", kw, params, make_obs(rng, P * n_per, net["obs_dim"])
