"""float64 numpy restatements of what on-device PPO collection computes (csrc/qs_ppo.h), with a running error bound for the float32 GAE:
SB3's RolloutBuffer.compute_returns_and_advantage and the loss of PPO.train as stable_baselines3 1.5 is remembered to write them.

The GAE bound.  With u = 2^-24, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) and, at step t,
a = gamma * lambda * nnt, the float32 sequence of csrc/qs_ppo.h is
    delta^ = fl(fl(gamma nnt nv + r) - v)                       two roundings (gamma * nnt is exact: nnt is 0 or 1)
    gae^   = fl(a^ gae^' + delta^),  a^ = fl(gamma lambda) nnt   one rounding each
so   |delta^ - delta| <= gamma_2 (|gamma nnt nv| + |r| + |v|)   and, writing E for |gae^ - gae| and ' for step t + 1,
    E <= a (1 + gamma_2) E' + gamma_2 a |gae'| + (1 + u) |delta^ - delta| + u |delta|
      <= a (1 + gamma_2) E' + gamma_3 (a |gae'| + |gamma nnt nv| + |r| + |v| + |delta|):
every step adds a few unit roundoffs of the magnitudes it touches, and what earlier steps (later t) added comes down the walk multiplied
by gamma * lambda per step.  return^ = fl(gae^ + v) adds one rounding:  |return^ - return| <= (1 + u) E + u (|return| + E)."""
import numpy as np

U = 2.0 ** -24


def gamma_k(k):
    return k * U / (1.0 - k * U)


def gae(rewards, values, episode_starts, last_values, last_dones, gamma, lam):
    """SB3's loop in float64 on float32 inputs [T, N] -> advantages, returns, and the bounds on a float32 evaluation's error of each"""
    r, v, es = (np.asarray(x, np.float64) for x in (rewards, values, episode_starts))
    T, N = r.shape
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    adv, ret, adv_bound, ret_bound = (np.zeros((T, N)) for _ in range(4))
    last_gae, E = np.zeros(N), np.zeros(N)
    for t in reversed(range(T)):
        if t == T - 1:
            nnt, nv = 1.0 - np.asarray(last_dones, np.float64), np.asarray(last_values, np.float64)
        else:
            nnt, nv = 1.0 - es[t + 1], v[t + 1]
        delta = r[t] + g * nv * nnt - v[t]
        a = g * l * nnt
        E = a * (1.0 + gamma_k(2)) * E + gamma_k(3) * (a * np.abs(last_gae) + np.abs(g * nnt * nv) + np.abs(r[t]) + np.abs(v[t]) + np.abs(delta))
        last_gae = delta + a * last_gae
        adv[t], ret[t] = last_gae, last_gae + v[t]
        adv_bound[t], ret_bound[t] = E, (1.0 + U) * E + U * (np.abs(ret[t]) + E)
    return adv, ret, adv_bound, ret_bound


def gae_data(rng, T, N, p_start=0.1):
    """random float32 [T, N] rewards and values, episode starts with probability p_start, last values and last dones"""
    return (rng.standard_normal((T, N)).astype(np.float32), (3.0 * rng.standard_normal((T, N))).astype(np.float32),
            (rng.random((T, N)) < p_start).astype(np.float32), (3.0 * rng.standard_normal(N)).astype(np.float32), (rng.random(N) < 0.3).astype(np.uint8))


def ppo_loss(values, log_prob, entropy, old_values, old_log_prob, advantages, returns, clip_range, clip_range_vf, ent_coef, vf_coef, normalize_advantage):
    """PPO.train's loss of one minibatch in float64 numpy -> (loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction)"""
    values, log_prob, old_values, old_log_prob, adv, returns = (np.asarray(x, np.float64) for x in (values, log_prob, old_values, old_log_prob, advantages, returns))
    if normalize_advantage and adv.size > 1:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)          # torch.Tensor.std is the unbiased one
    log_ratio = log_prob - old_log_prob
    ratio = np.exp(log_ratio)
    policy_loss = -np.minimum(adv * ratio, adv * np.clip(ratio, 1.0 - clip_range, 1.0 + clip_range)).mean()
    pred = values if clip_range_vf is None else old_values + np.clip(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = ((returns - pred) ** 2).mean()
    entropy_loss = -np.mean(-log_prob) if entropy is None else -np.mean(np.asarray(entropy, np.float64))
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    return loss, policy_loss, value_loss, entropy_loss, np.mean((ratio - 1.0) - log_ratio), np.mean(np.abs(ratio - 1.0) > clip_range)
