"""float64 restatement of one minibatch of the PPO update (csrc/qs_ppo_train.h), the per-parameter scale S, the undecided samples, the
cases and the yardstick the CPU and GPU tests of the update share.

The yardstick.  g64 = float64 autograd (CPU) on qs_amd.ppo.ppo_loss and evaluate_actions of float64 copies of the modules; the peer = the same
in float32.  S[i] = the sum over samples of the absolute per-sample terms of parameter i in float64 (|delta|^T |h| for weights, sum |delta|
for biases, sum |dlp (z^2 - 1)| + ent_coef for log_std).  With u = 2^-24,  r_peer = max_i |g_peer[i] - g64[i]| / (u S[i]).  A float32
evaluation g passes if  |g[i] - g64[i]| <= 5 r_peer u S[i] for every i, and, per network (actor with
log_std; critic),  ||g - g64|| / ||g64|| <= 5 x the peer's.  5 is tests/yardstick.py's FACTOR; r_peer is measured per case, never written down.

Undecided samples.  The float32 mean is within e_mean of the float64 one (the running bound of tests/policy_ref.py, restated here per layer),
so z_j = (a_j - mean_j) inv_std_j is within dz_j = inv_std_j e_mean_j + 4 u |z_j| (one subtraction, one product, expf's last bits), and
    log_prob is within  e_lp = sum_j (|z_j| dz_j + 3 u (z_j^2 / 2 + |log_std_j| + log(2 pi) / 2)) + gamma_A sum_j |term_j|
(each term: one product, one fmaf, one subtraction; the sum: A - 1 additions).  The ratio r = exp(log_prob - old) is then within
r (e_lp + u |lr| + 4 u) of the float64 one: a sample whose float64 r lies that close to 1 - c or 1 + c may fall either side (its clip flag, and
for the side on which the clamped branch is the minimum, its whole policy gradient |A r| / B).  Under relu a sample with a hidden
pre-activation within its forward bound of 0 may switch that unit.  At most 1 % of a case's samples may be undecided (a cap on the cases, not a tolerance).
What an undecided sample is granted: where the evaluation's own branch decisions are known (the host twin reports them per sample, the peer's are
recomputed in float32 torch, the device's are the twin's when both count the same number of clipped samples), float64 takes THOSE branches on
the clip-edge samples and nothing is granted, elementwise or normwise.  Where they are not known, a clip-edge sample is granted its policy terms
|A r| / B elementwise (never a critic term, never normwise).  A relu-undecided sample is granted its absolute terms in its own network."""
import copy
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import policy_ref as R  # noqa: E402
from yardstick import FACTOR  # noqa: E402

U = 2.0 ** -24
HALF_LOG_2PI = 0.9189385332046727

# obs-arch-out of the actor, the critic's arch
NETS = {
    "tanh-28-64x64-6": dict(obs_dim=28, action_dim=6, net_arch=(64, 64), vf_arch=(64, 64), activation="tanh"),
    "relu-30-33x7-5": dict(obs_dim=30, action_dim=5, net_arch=(33, 7), vf_arch=(16,), activation="relu"),
    "none-28-12": dict(obs_dim=28, action_dim=12, net_arch=(), vf_arch=(), activation="none"),
    "tanh-64-64-64": dict(obs_dim=64, action_dim=64, net_arch=(64,), vf_arch=(64,), activation="tanh"),
}
PARTS = 1024                                       # csrc/qs_ppo_train.h (the CPU test checks it against the host build)
# 1: no normalisation; 16: one tile; 17: a partial tile, two parts (two waves of a workgroup); 100; 1000: several workgroups' parts;
# 16 * PARTS + 1, + 2: the smallest B at which a part owns a second tile (the tiles are dealt round), and one more
# 2 * 16 * PARTS + 16 * 5 + 1: every part owns two full tiles, parts 0 .. 4 a full third one, part 5 a third one of one sample
BATCHES = (1, 16, 17, 100, 1000, 16 * PARTS + 1, 16 * PARTS + 2, 2 * 16 * PARTS + 16 * 5 + 1)
HYPER = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, normalize_advantage=True)


def make_policy(net, seed, device="cpu"):
    """a DeviceActorCritic with torch.nn.Linear's initial ranges, biases not zero, the action head scaled so that z is not all noise"""
    import torch
    from qs_amd.ppo import DeviceActorCritic
    torch.manual_seed(seed)
    pol = DeviceActorCritic(net["obs_dim"], net["action_dim"], net_arch=net["net_arch"], vf_arch=net["vf_arch"], activation=net["activation"], num_envs=16,
                            ortho_init=False, device=device)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        [m for m in pol.actor if isinstance(m, torch.nn.Linear)][-1].weight.mul_(0.25)
        pol.log_std.copy_((0.3 * torch.randn(net["action_dim"], generator=g)).to(pol.log_std.device))
    return pol


def copy_of(pol, dtype):
    """an object with evaluate_actions over copies of pol's modules in `dtype` on the CPU"""
    import torch
    from qs_amd.ppo import DeviceActorCritic
    c = types.SimpleNamespace(torch=torch)
    c.actor = copy.deepcopy(pol.actor).to(device="cpu", dtype=dtype)
    c.critic = copy.deepcopy(pol.critic).to(device="cpu", dtype=dtype)
    c.log_std = torch.nn.Parameter(pol.log_std.detach().to(device="cpu", dtype=dtype).clone())
    c.evaluate_actions = types.MethodType(DeviceActorCritic.evaluate_actions, c)
    c.parameters = lambda: list(c.actor.parameters()) + list(c.critic.parameters()) + [c.log_std]
    return c


def make_data(pol, total, seed):
    """float32 rollout arrays [total, ...]: observations as VecNormalize hands them out, actions sampled from the policy, old_log_prob =
    log_prob + 0.15 N(0, 1), advantages = 2 N(0, 1) + 0.3, returns = value + N(0, 1)"""
    import torch
    rng = np.random.default_rng([seed, total])
    obs = R.make_obs(rng, total, pol.obs_dim)
    c = copy_of(pol, torch.float64)
    with torch.no_grad():
        o = torch.as_tensor(obs, dtype=torch.float64)
        mean, value = c.actor(o), c.critic(o).flatten()
        act = (mean + c.log_std.exp() * torch.as_tensor(rng.standard_normal(mean.shape))).to(torch.float32)
        _, lp, _ = c.evaluate_actions(o, act.double())
    return dict(observations=obs, actions=act.numpy(), old_log_prob=(lp.numpy() + 0.15 * rng.standard_normal(total)).astype(np.float32),
                advantages=(2.0 * rng.standard_normal(total) + 0.3).astype(np.float32), returns=(value.numpy() + rng.standard_normal(total)).astype(np.float32))


def autograd(pol, data, idx, hyper, dtype):
    """ppo_loss + evaluate_actions of a copy in `dtype` on data[idx] -> (flat gradient [actor | critic | log_std] float64, stats dict)"""
    import torch
    from qs_amd.ppo import ppo_loss
    c = copy_of(pol, dtype)
    mb = {k: torch.as_tensor(v[idx]).to(dtype) for k, v in data.items()}
    values, log_prob, entropy = c.evaluate_actions(mb["observations"], mb["actions"])
    loss, info = ppo_loss(values, log_prob, entropy, values.detach(), mb["old_log_prob"], mb["advantages"], mb["returns"], hyper["clip_range"], None,
                          hyper["ent_coef"], hyper["vf_coef"], hyper["normalize_advantage"])
    loss.backward()
    g = torch.cat([p.grad.reshape(-1) for p in c.parameters()]).double().numpy()
    return g, {k: float(v) for k, v in info.items()}


def _layers(flat, obs_dim, out_dim, arch):
    return R.split_params(np.asarray(flat, np.float64), obs_dim, out_dim, arch, True)


def _forward(layers, x, activation, c_tanh):
    """-> hs [h_-1 = x, h_0, ...] (post-activations), pre [pre-activations], e_pre [their float32 bounds], e (bound of the output)"""
    h, e = x, np.zeros_like(x)
    hs, pre, e_pre = [x], [], []
    for li, (W, b) in enumerate(layers):
        aW = np.abs(W)
        z = h @ W.T + b
        e = e @ aW.T + R.gamma(W.shape[1] + 1) * (np.abs(h) @ aW.T + np.abs(b))
        pre.append(z); e_pre.append(e)
        if li < len(layers) - 1 and activation == "tanh":
            h = np.tanh(z); e = e + c_tanh * U * np.abs(h)
        elif li < len(layers) - 1 and activation == "relu":
            h = np.maximum(z, 0.0)
        else:
            h = z
        hs.append(h)
    return hs, pre, e_pre, e


def _backward(layers, hs, delta, activation, absolute):
    """delta [B, out] at the last layer -> flat [n_params]: the gradient, or with `absolute` the sum of the absolute per-sample terms"""
    out = []
    d = np.abs(delta) if absolute else delta
    for li in reversed(range(len(layers))):
        W, _ = layers[li]
        hp = hs[li]
        out.append(np.concatenate([(d.T @ (np.abs(hp) if absolute else hp)).reshape(-1), d.sum(0)]))
        if li > 0:
            da = 1.0 - hp * hp if activation == "tanh" else ((hp > 0).astype(np.float64) if activation == "relu" else np.ones_like(hp))
            d = (d @ (np.abs(W) if absolute else W)) * da
    return np.concatenate(out[::-1])


def restate(pol, data, idx, hyper, batch=None, flags=None):
    """The float64 restatement of csrc/qs_ppo_train.h on data[idx] (every index in range; batch = the divisor B, len(idx) by default; the
    advantages are normalised over idx) -> dict(g, S, S_undecided, undecided [B] bool, stats, ratio, ...).
    flags [B] uint8 (bit 0: the unclipped branch carried the gradient, bit 1: counted as clipped) are the decisions of the float32 evaluation the
    restatement is for: the clip-edge undecided samples, and only they, then take THOSE branches, and get no slack at all.  Without flags they
    keep float64's branches and S_undecided grants each its policy terms |A r| / B (actor and log_std; a clip edge cannot move the critic).
    A relu-undecided sample (a hidden pre-activation within its forward bound of 0) is granted its absolute terms in the network whose unit it is."""
    net = dict(obs_dim=pol.obs_dim, action_dim=pol.action_dim)
    la = _layers(pol.actor_params.detach().cpu().numpy(), net["obs_dim"], net["action_dim"], pol.net_arch)
    lc = _layers(pol.critic_params.detach().cpu().numpy(), net["obs_dim"], 1, pol.vf_arch)
    ls = pol.log_std.detach().cpu().numpy().astype(np.float64)
    c_tanh = R.tanh_c() if pol.activation == "tanh" else 0.0
    d = {k: np.asarray(v[idx], np.float64) for k, v in data.items()}
    n = len(idx)
    B = float(n if batch is None else batch)
    c, ent, vf = hyper["clip_range"], hyper["ent_coef"], hyper["vf_coef"]
    adv = d["advantages"]
    if hyper["normalize_advantage"] and n > 1:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    hs_a, pre_a, epre_a, e_mean = _forward(la, d["observations"], pol.activation, c_tanh)
    hs_c, pre_c, epre_c, _ = _forward(lc, d["observations"], pol.activation, c_tanh)
    inv = np.exp(-ls)
    z = (d["actions"] - hs_a[-1]) * inv
    terms = -0.5 * z * z - ls - HALF_LOG_2PI
    lp = terms.sum(1)
    lr = lp - d["old_log_prob"]
    r = np.exp(lr)
    u1, u2 = adv * r, adv * np.clip(r, 1.0 - c, 1.0 + c)
    on = u1 <= u2
    clipped = np.abs(r - 1.0) > c
    value = hs_c[-1][:, 0]
    dv = 2.0 * vf * (value - d["returns"]) / B
    # the undecided
    dz = inv * e_mean + 4.0 * U * np.abs(z)
    e_lp = (np.abs(z) * dz + 3.0 * U * (0.5 * z * z + np.abs(ls) + HALF_LOG_2PI)).sum(1) + R.gamma(max(z.shape[1], 1)) * np.abs(terms).sum(1)
    e_r = r * (e_lp + U * np.abs(lr) + 4.0 * U)
    und_clip = (np.abs(r - (1.0 - c)) <= e_r) | (np.abs(r - (1.0 + c)) <= e_r)
    und_relu = [np.zeros(n, bool), np.zeros(n, bool)]
    if pol.activation == "relu":
        for k, (pre, epre) in enumerate(((pre_a, epre_a), (pre_c, epre_c))):
            for zl, el in zip(pre[:-1], epre[:-1]):
                und_relu[k] |= (np.abs(zl) <= el).any(1)
    disagree = 0
    if flags is not None:
        f_on, f_clipped = (np.asarray(flags) & 1) != 0, (np.asarray(flags) & 2) != 0
        disagree = int((f_clipped != clipped)[~und_clip & ~und_relu[0]].sum())     # a decided sample on the other side: a finding
        on, clipped = np.where(und_clip, f_on, on), np.where(und_clip, f_clipped, clipped)
    dlp = np.where(on, -u1 / B, 0.0)

    def actor(dl, absolute, rows=slice(None)):
        ga = _backward(la, [h[rows] for h in hs_a], (dl[:, None] * z * inv)[rows], pol.activation, absolute)
        gl = (dl[:, None] * (z * z - 1.0))[rows]
        return ga, (np.abs(gl).sum(0) if absolute else gl.sum(0))

    def critic(absolute, rows=slice(None)):
        return _backward(lc, [h[rows] for h in hs_c], dv[rows, None], pol.activation, absolute)

    ga, gl = actor(dlp, False)
    g = np.concatenate([ga, critic(False), gl - ent])
    Sa, Sl = actor(dlp, True)
    S = np.concatenate([Sa, critic(True), Sl + ent])
    rows_a = und_relu[0] | (und_clip if flags is None else False)
    ua, ul = actor(np.abs(u1) / B, True, rows_a) if rows_a.any() else (np.zeros_like(Sa), np.zeros_like(Sl))
    S_und = np.concatenate([ua, critic(True, und_relu[1]) if und_relu[1].any() else np.zeros(S.size - Sa.size - Sl.size), ul])
    S_relu = S_und
    if flags is None and und_clip.any():           # (the normwise slack is the relu-undecided samples' alone)
        ra, rl = actor(np.abs(u1) / B, True, und_relu[0]) if und_relu[0].any() else (np.zeros_like(Sa), np.zeros_like(Sl))
        S_relu = np.concatenate([ra, S_und[Sa.size:S.size - Sl.size], rl])
    stats = dict(policy_loss=-np.minimum(u1, u2).sum() / B, value_loss=((d["returns"] - value) ** 2).sum() / B, entropy_loss=-(ls + 0.5 + HALF_LOG_2PI).sum(),
                 approx_kl=((r - 1.0) - lr).sum() / B, clip_fraction=clipped.sum() / B)
    # A statistic's scale, the floor under the peer's single draw in hold_stats: the mean over the samples of what one unit roundoff of the
    # float32 numbers a term is made of moves the term by.  The policy and kl terms are functions of log_prob, a float32 number of magnitude
    # |lp| (about 90 at action_dim 64) that the contract builds as an ascending sum of A like-signed terms: its representation alone is good to
    # u |lp|, its sum to gamma_A |lp|, and d(A r)/d lp = A r, d((r - 1) - lr)/d lp = r - 1; hence |term| (1 + |lp|) for the policy term and
    # |r - 1| (1 + |lp|) + |lr| for kl.  The value term (ret - v)^2 is a function of v: 2 |ret - v| |v| + the term.  Counting u |lp| and not
    # gamma_A |lp| keeps the floor at ONE rounding per float32 number; without the |lp| factor the floor would ask the evaluation to know
    # log_prob to better than float32 can hold it.
    alp = np.abs(lp)
    scale = dict(policy_loss=(np.abs(np.minimum(u1, u2)) * (1.0 + alp)).sum() / B, value_loss=((d["returns"] - value) ** 2 + 2.0 * np.abs(d["returns"] - value) * np.abs(value)).sum() / B,
                 entropy_loss=np.abs(ls + 0.5 + HALF_LOG_2PI).sum(), approx_kl=(np.abs(r - 1.0) * (1.0 + alp) + np.abs(lr)).sum() / B)
    return dict(stat_scale=scale, g=g, S=S, S_undecided=S_und, S_relu=S_relu, undecided=und_clip | und_relu[0] | und_relu[1], undecided_clip=und_clip, stats=stats, ratio=r,
                adv=adv, disagree=disagree, forced=flags is not None, n_actor=sum(W.size + b.size for W, b in la), n_critic=sum(W.size + b.size for W, b in lc))


def peer_flags(pol, data, idx, hyper):
    """the branch decisions of the peer, torch float32 on the CPU: flags as restate() takes them"""
    import torch
    c = copy_of(pol, torch.float32)
    mb = {k: torch.as_tensor(v[idx]) for k, v in data.items()}
    with torch.no_grad():
        _, log_prob, _ = c.evaluate_actions(mb["observations"], mb["actions"])
        adv = mb["advantages"]
        if hyper["normalize_advantage"] and adv.numel() > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(log_prob - mb["old_log_prob"])
        u1, u2 = adv * ratio, adv * torch.clamp(ratio, 1.0 - hyper["clip_range"], 1.0 + hyper["clip_range"])
        return ((u1 <= u2).numpy().astype(np.uint8) | ((torch.abs(ratio - 1.0) > hyper["clip_range"]).numpy().astype(np.uint8) << 1))


def networks(ref):
    """index sets of the two networks in the flat gradient: actor with log_std, critic"""
    n = ref["g"].size
    na, nc = ref["n_actor"], ref["n_critic"]
    return dict(actor=np.r_[0:na, na + nc:n], critic=np.r_[na:na + nc])


def measure(g, ref, g64=None, slack=False):
    """-> (worst elementwise ratio |g - g64| / (u S), with `slack` outside what ref's undecided samples may move; {network: ||g - g64|| / ||g64||}).
    g64 defaults to ref's own gradient (float64 with ref's branches).  The peer is measured without slack: r_peer is the plain ratio."""
    g64 = ref["g"] if g64 is None else g64
    err = np.abs(np.asarray(g, np.float64) - g64)
    if slack:
        err = np.maximum(err - ref["S_undecided"], 0.0)
    S = ref["S"]                                   # (a parameter no sample reaches, a dead relu unit's: S = 0, and only an exact 0 passes)
    worst = float(np.max(np.where(S > 0, err / np.where(S > 0, U * S, 1.0), np.where(err > 0, np.inf, 0.0))))
    return worst, {k: float(np.linalg.norm((np.asarray(g, np.float64) - g64)[ix]) / np.linalg.norm(g64[ix])) for k, ix in networks(ref).items()}


def hold(name, g, ref, peer, g64=None):
    """asserts the yardstick for evaluation `g` given the peer's measure; -> the record of the case.  Slack: elementwise ref's S_undecided
    (nothing for a clip-edge sample whose branch ref was given), normwise the relu-undecided samples' terms alone (nothing for tanh / none)."""
    r_peer, norm_peer = peer
    worst, norms = measure(g, ref, g64, slack=True)
    rec = dict(r_peer=r_peer, worst=worst, norm=norms, norm_peer=norm_peer, undecided=int(ref["undecided"].sum()), forced=bool(ref["forced"]),
               slack_samples=int(ref["undecided"].sum() - (ref["undecided_clip"] & ref["forced"]).sum()))
    print(f"{name}: r_peer {r_peer:.4f}  worst {worst:.4f} ({worst / r_peer:.2f} x)  normwise " +
          "  ".join(f"{k} {norms[k]:.3e} ({norms[k] / norm_peer[k]:.2f} x)" for k in norms) + f"  undecided {rec['undecided']} (branches given: {rec['forced']})")
    assert worst <= FACTOR * r_peer, (name, "elementwise", worst, r_peer)
    for k in norms:
        ix = networks(ref)[k]
        # (the relu-undecided samples' terms: a unit's sign cannot be read back from an evaluation, so it cannot be given to float64.  One sample's
        # terms are about 1 / B of S, far above 5 x the peer's error, so a relu case WITH such samples is close to vacuous normwise; the tanh and none
        # networks run the same code with nothing granted)
        slack = np.linalg.norm(ref["S_relu"][ix]) / np.linalg.norm((ref["g"] if g64 is None else g64)[ix])
        assert norms[k] <= FACTOR * norm_peer[k] + slack, (name, "normwise", k, norms[k], norm_peer[k], slack)
    return rec


def yardstick(name, pol, data, idx, hyper, g, flags, g_other=None):
    """The whole rule for evaluation g whose branch decisions are `flags` (None: not known): float64 with those branches on the clip-edge
    samples as the reference, the peer measured against float64 with ITS OWN branches.  g_other: hold g against that evaluation instead of
    float64 (the device against the twin), same S, same r_peer.  -> (record, ref)"""
    ref = restate(pol, data, idx, hyper, flags=flags)
    assert ref["undecided"].mean() <= 0.01, (name, "undecided", float(ref["undecided"].mean()))
    assert ref["disagree"] == 0, (name, "decided samples whose clip flag differs from float64's", ref["disagree"])
    ref_peer = restate(pol, data, idx, hyper, flags=peer_flags(pol, data, idx, hyper))
    import torch
    peer = measure(autograd(pol, data, idx, hyper, torch.float32)[0], ref_peer)
    return hold(name, g, ref, peer, None if g_other is None else np.asarray(g_other, np.float64)), ref


def hold_stats(name, st, ref, st_peer, st64, B):
    """The statistics of evaluation `st` (a dict): losses and approx_kl within 5 x the peer's distance from float64 autograd's, clip_fraction
    exact up to the undecided samples (half a sample for the float32 quotient); -> the record.
    One scalar of the peer is ONE draw of a rounding error and may be any fraction of a unit roundoff by luck (measured on the twin's cases:
    the peer's entropy_loss between 0.01 and 0.6 u of the sum of its absolute terms), so the peer's distance counts as at least u x the
    statistic's scale (restate(), where the count behind it is written down): no float32 evaluation owes more than its format's precision."""
    rec = {}
    for k in ("policy_loss", "value_loss", "entropy_loss", "approx_kl"):
        err, err_peer, floor = abs(float(st[k]) - st64[k]), abs(st_peer[k] - st64[k]), U * ref["stat_scale"][k]
        rec[k] = (err, err_peer, floor)
        print(f"{name}: {k} {float(st[k]):.9g}  float64 {st64[k]:.9g}  error {err:.3e}  the peer's {err_peer:.3e}  u x scale {floor:.3e}")
    for k, (err, err_peer, floor) in rec.items():
        assert err <= FACTOR * max(err_peer, floor), (name, k, err, err_peer, floor)
    free = 0 if ref["forced"] else int(ref["undecided_clip"].sum())          # (with the evaluation's own branches the count is exact)
    assert abs(float(st["clip_fraction"]) - ref["stats"]["clip_fraction"]) * B <= free + 0.5, (name, st["clip_fraction"], ref["stats"]["clip_fraction"])
    return rec


def case(net_name, B, seed=0, hyper=None):
    """-> (pol on the CPU, data with total = B + 7 rows, idx: a permutation's first B entries).  The data's seed is the first of
    seed, seed + 1, ... with no undecided sample, where eight tries find one, else the one of the eight with the fewest (at B of some thousands
    there always are a few).  The choice looks at the float64 restatement alone, never at an evaluation under test."""
    pol = make_policy(NETS[net_name], seed + 11 * sorted(NETS).index(net_name))
    total = B + 7
    idx = np.random.default_rng([seed, B, 5]).permutation(total)[:B].astype(np.int64)
    best = None
    for k in range(8):
        data = make_data(pol, total, seed + k)
        n = int(restate(pol, data, idx, hyper or HYPER)["undecided"].sum())
        if n == 0:
            return pol, data, idx
        if best is None or n < best[0]:
            best = (n, data)
    return pol, best[1], idx


def descs(pol):
    """(actor, critic) qs_policy_desc of a DeviceActorCritic"""
    import ctypes as C
    from qs_amd.lib import QsPolicyDesc
    from qs_amd.policy import ACTIVATIONS

    def desc(out_dim, arch):
        return QsPolicyDesc(16, 1, pol.obs_dim, out_dim, len(arch), (C.c_int32 * 4)(*arch), ACTIVATIONS[pol.activation], 0, 1, -3.0e38, 3.0e38)
    return desc(pol.action_dim, pol.net_arch), desc(1, pol.vf_arch)


def twin_grad(pol, data, idx, hyper):
    """the host twin (tests/emu/emu_ppo_train.py) on data[idx] -> (grad, stats as a dict, refused, per-sample flags)"""
    from emu import emu_ppo_train as E
    from qs_amd import lib
    da, dc = descs(pol)
    g, st, refused = E.grad(da, dc, pol.actor_params.detach().cpu().numpy(), pol.critic_params.detach().cpu().numpy(), pol.log_std.detach().cpu().numpy(),
                            data["observations"], data["actions"], data["old_log_prob"], data["advantages"], data["returns"], idx, E.hyper(**hyper))
    return g, dict(zip(lib.PPO_STATS, st.tolist())), refused, E.grad.last_flags


def fill(buf, data):
    """data (make_data's arrays, T * N rows) into a DeviceRolloutBuffer"""
    import torch
    for name, key in (("observations", "observations"), ("actions", "actions"), ("log_probs", "old_log_prob"), ("advantages", "advantages"), ("returns", "returns")):
        getattr(buf, name).copy_(torch.as_tensor(data[key]).reshape(getattr(buf, name).shape))


def learner(pol, data, n_steps, num_envs, **kw):
    """a DevicePPO on the GPU without an environment whose policy holds pol's parameters and whose buffer holds `data`"""
    import torch
    from qs_amd import DeviceActorCritic, DevicePPO
    dev = DeviceActorCritic(pol.obs_dim, pol.action_dim, net_arch=pol.net_arch, vf_arch=pol.vf_arch, activation=pol.activation, num_envs=num_envs)
    with torch.no_grad():
        dev.actor_params.copy_(pol.actor_params); dev.critic_params.copy_(pol.critic_params); dev.log_std.copy_(pol.log_std)
    algo = DevicePPO(None, dev, n_steps=n_steps, **kw)
    fill(algo.buffer, data)
    return algo


# ---- clip and Adam: the float64 formula on the same float32 inputs, and a bound on a float32 evaluation of the stated sequence
NORM_BLOCK = 256                                   # csrc/qs_ppo_train.h


def adam64(p, m, v, g, t, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5):
    """torch's clip_grad_norm_ and Adam (no weight decay, no amsgrad) in float64 -> (p, m, v, norm, bounds on a float32 evaluation's p, m and v).

    The bound counts the roundings of csrc/qs_ppo_train.h's sequence (u = 2^-24, gamma_k as in ppo_ref):
      norm: a block's fmaf chain and the chain of blocks add positive terms, relative error gamma_(NORM_BLOCK + blocks); sqrtf halves it, + u
      coef = fminf(1, max / (norm + 1e-6)): one addition, one division;   gc = g coef: one product            -> e_g relative
      m' = fmaf(b1, m, omb1 gc):  b1, omb1 rounded once each, one product, one fmaf  -> dm <= (e_g + 3 u) |omb1 gc| + 2 u |b1 m| + u |m'|
      v' likewise with gc twice                                                      -> dv <= (2 e_g + 4 u) omb2 gc^2 + 2 u b2 v + u v'
      denom = sqrtf(v') / bc2_sqrt + eps: sqrt (dv / 2 v' + u), bc2_sqrt rounded, one division, eps rounded, one addition
      p' = p - (step_size m') / denom: step_size rounded, one product, one division, one subtraction"""
    p, m, v, g = (np.asarray(x, np.float64) for x in (p, m, v, g))
    b1, b2 = betas
    nb = (g.size + NORM_BLOCK - 1) // NORM_BLOCK
    norm = np.sqrt((g * g).sum())
    big = max_grad_norm is None
    coef = 1.0 if big else min(1.0, max_grad_norm / (norm + 1e-6))
    e_g = (0.0 if big else 0.5 * (NORM_BLOCK + nb) * U / (1 - (NORM_BLOCK + nb) * U) + 4 * U) + U
    gc = g * coef
    m1 = b1 * m + (1 - b1) * gc
    v1 = b2 * v + (1 - b2) * gc * gc
    dm = (e_g + 3 * U) * np.abs((1 - b1) * gc) + 2 * U * np.abs(b1 * m) + U * np.abs(m1)
    dv = (2 * e_g + 4 * U) * (1 - b2) * gc * gc + 2 * U * b2 * v + U * v1
    bc = np.sqrt(1 - b2 ** t)
    root = np.sqrt(v1)
    denom = root / bc + eps
    d_denom = (np.where(v1 > 0, dv / np.where(v1 > 0, 2 * root, 1.0), 0.0) + 3 * U * root) / bc + U * denom + U * eps
    ss = lr / (1 - b1 ** t)
    q = ss * m1 / denom
    dq = ss * dm / denom + np.abs(q) * (d_denom / denom + 3 * U)
    p1 = p - q
    return p1, m1, v1, norm, 1.01 * (dq + U * np.abs(p1)), 1.01 * dm, 1.01 * dv
