"""PPO with the collection on the device: DeviceActorCritic (actor and critic in ONE HIP launch per collected step, k_actor_critic,
csrc/qs_ppo.hip), DeviceRolloutBuffer ([T, N, ...] device tensors, GAE in one launch, k_gae) and DevicePPO (SB3's PPO loop: the rollout
on the device; the update -- SB3's PPO.train -- in torch with autograd, or with update="device" in HIP as well: per minibatch the gradient
by index from the rollout arrays, k_ppo_grad, and clip + Adam in place, k_ppo_adam, csrc/qs_ppo_train.hip).

The parameters live ONCE: one flat float32 tensor per network in `torch.nn.utils.parameters_to_vector` order, which the kernels read in
place, and torch.nn modules whose Parameters are views into those tensors, which autograd and the optimiser work on.  An optimiser step
is therefore what the next collected step computes with: no copy, no set_params.

Only separate actor and critic trunks (SB3 MlpPolicy's default net_arch = dict(pi=[64, 64], vf=[64, 64])).  The formulas, defaults and
state-dict names are stable_baselines3 1.5's as remembered (ppo/ppo.py, common/on_policy_algorithm.py, common/buffers.py,
common/policies.py); the package was not available to check them against."""
import ctypes as C
import math

import numpy as np

from . import lib as _lib
from .handle import DeviceHandle, ptr, raw_reward_of
from .policy import ACTIVATIONS, MAX_HIDDEN, _to_numpy, layer_shapes, layers_from_state_dict, param_count, state_dict_from_zip

NO_CLIP = 3.0e38
UPDATE_MAX_HIDDEN, UPDATE_MAX_WIDTH = 2, 64      # what update="device" takes (csrc/qs_ppo_train.h)


def _sequential(flat, obs_dim, out_dim, arch, activation):
    """a torch.nn.Sequential over `flat` [n_params]: every Linear's weight and bias is a Parameter that VIEWS its slice of flat"""
    import torch
    nn = torch.nn
    act = {"tanh": nn.Tanh, "relu": nn.ReLU, "none": None}[activation]
    mods, off = [], 0
    shapes = layer_shapes(obs_dim, out_dim, arch)
    for i, (o, k) in enumerate(shapes):
        lin = nn.Linear(k, o, device="meta")
        lin.weight = nn.Parameter(flat[off:off + o * k].view(o, k)); off += o * k
        lin.bias = nn.Parameter(flat[off:off + o]); off += o
        mods.append(lin)
        if act is not None and i < len(shapes) - 1:
            mods.append(act())
    assert off == flat.numel()
    return nn.Sequential(*mods)


class DeviceActorCritic(DeviceHandle):
    """SB3's ActorCriticPolicy (MlpPolicy) with separate trunks.  `device` an int (cuda:<int>) or anything torch.device takes; on a
    device that is not a GPU only the torch side exists (evaluate_actions, state_dict, the parameter views): collect / predict raise."""
    _prefix, _owner = "qs_ac", "policy"

    def __init__(self, obs_dim, action_dim, net_arch=(64, 64), vf_arch=None, activation="tanh", num_envs=1, clip=(-1.0, 1.0), log_std_init=0.0,
                 ortho_init=True, device=0):
        import torch
        self.torch = torch
        nn = torch.nn
        net_arch = tuple(int(w) for w in net_arch)
        vf_arch = net_arch if vf_arch is None else tuple(int(w) for w in vf_arch)
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation = {activation!r} is none of {sorted(ACTIVATIONS)}")
        if max(len(net_arch), len(vf_arch)) > MAX_HIDDEN:
            raise ValueError(f"net_arch = {net_arch} / vf_arch = {vf_arch} has more than {MAX_HIDDEN} hidden layers")
        self.obs_dim, self.action_dim, self.net_arch, self.vf_arch, self.activation = int(obs_dim), int(action_dim), net_arch, vf_arch, activation
        self.num_envs = int(num_envs)
        self.clip = (-NO_CLIP, NO_CLIP) if clip is None else (float(clip[0]), float(clip[1]))
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.actor_params = torch.zeros(param_count(self.obs_dim, self.action_dim, net_arch), **f32)
        self.critic_params = torch.zeros(param_count(self.obs_dim, 1, vf_arch), **f32)
        self.actor = _sequential(self.actor_params, self.obs_dim, self.action_dim, net_arch, activation)
        self.critic = _sequential(self.critic_params, self.obs_dim, 1, vf_arch, activation)
        self.log_std = nn.Parameter(torch.full((self.action_dim,), float(log_std_init), **f32))
        self._init_weights(ortho_init)
        self.h = None
        if self.device.type == "cuda":
            self.lib = _lib.load()

            def desc(out_dim, arch, lo, hi):
                return _lib.QsPolicyDesc(self.num_envs, 1, self.obs_dim, out_dim, len(arch), (C.c_int32 * 4)(*arch), ACTIVATIONS[activation], 0, 1, lo, hi)
            self.h = C.c_void_p()
            _lib.check(self.lib.qs_ac_create(C.byref(desc(self.action_dim, net_arch, *self.clip)), C.byref(desc(1, vf_arch, -NO_CLIP, NO_CLIP)),
                                             self.device.index or 0, C.byref(self.h)))
            _lib.check(self.lib.qs_ac_set_params(self.h, ptr(self.actor_params), ptr(self.critic_params)))
            n, a = self.num_envs, self.action_dim
            self.env_actions = torch.zeros((n, a), **f32)          # the clipped actions of the last collect / predict
            self._scratch = None                                   # rows for predict / predict_values

    def _init_weights(self, ortho_init):
        """ActorCriticPolicy._build: orthogonal with gain sqrt(2) for the trunks, 0.01 for the action head, 1 for the value head, biases 0;
        without ortho_init torch.nn.Linear's own uniform ranges"""
        torch = self.torch
        with torch.no_grad():
            for net, last_gain in ((self.actor, 0.01), (self.critic, 1.0)):
                lins = [m for m in net if isinstance(m, torch.nn.Linear)]
                for i, lin in enumerate(lins):
                    if ortho_init:
                        torch.nn.init.orthogonal_(lin.weight, gain=last_gain if i == len(lins) - 1 else math.sqrt(2.0))
                        lin.bias.zero_()
                    else:
                        r = 1.0 / math.sqrt(lin.in_features)
                        lin.weight.uniform_(-r, r)
                        lin.bias.uniform_(-r, r)

    def parameters(self):
        """what an optimiser takes: the view-Parameters of both networks and log_std"""
        return list(self.actor.parameters()) + list(self.critic.parameters()) + [self.log_std]

    # ---- the device side
    def _need_device(self, what):
        if self.h is None:
            raise RuntimeError(f"DeviceActorCritic.{what} runs on a GPU; this one was built on {self.device} (there is no CPU path)")

    def collect(self, obs, eps, obs_row, action_row, value_row, log_prob_row):
        """One collected step in one launch: samples a = mean(obs) + exp(log_std) * eps, writes obs, the unclipped a, V(obs) and
        log_prob(a) into the given rows (row t of a rollout buffer) and returns the clipped actions for the environment (a reused buffer,
        valid until the next collect).  On torch's current stream."""
        self._need_device("collect")
        n, o, a = self.num_envs, self.obs_dim, self.action_dim
        args = (self._arg("obs", obs, (n, o)), self._arg("eps", eps, (n, a)), ptr(self.log_std.data), ptr(self.env_actions),
                self._arg("obs_row", obs_row, (n, o)), self._arg("action_row", action_row, (n, a)), self._arg("value_row", value_row, (n,)),
                self._arg("log_prob_row", log_prob_row, (n,)))
        self._stream()
        _lib.check(self.lib.qs_ac_collect(self.h, *args))
        return self.env_actions

    def predict_values(self, obs, mask=None, out=None):
        """V(obs) [N] (ActorCriticPolicy.predict_values); with a uint8 mask [N] only the masked entries of `out` are written"""
        self._need_device("predict_values")
        t = self.torch
        if out is None:
            out = t.zeros(self.num_envs, dtype=t.float32, device=self.device)
        p_mask = None if mask is None else self._arg("mask", mask, (self.num_envs,), t.uint8)
        args = (self._arg("obs", obs, (self.num_envs, self.obs_dim)), p_mask, self._arg("out", out, (self.num_envs,)))
        self._stream()
        _lib.check(self.lib.qs_ac_values(self.h, *args))
        return out

    def bootstrap(self, terminal_obs, truncated, gamma, rewards):
        """rewards[i] = fmaf(gamma, V(terminal_obs[i]), rewards[i]) where truncated[i], in place"""
        self._need_device("bootstrap")
        n = self.num_envs
        args = (self._arg("terminal_obs", terminal_obs, (n, self.obs_dim)), self._arg("truncated", truncated, (n,), self.torch.uint8))
        p_rew = self._arg("rewards", rewards, (n,))
        self._stream()
        _lib.check(self.lib.qs_ac_bootstrap(self.h, *args, float(gamma), p_rew))
        return rewards

    def predict(self, obs, state=None, episode_start=None, deterministic=True):
        """SB3's BasePolicy.predict through the collect kernel (noise 0 when deterministic): numpy in -> (numpy actions, None); a device
        tensor in -> (a copy of the action tensor, None).  Actions are clipped to the action Box."""
        self._need_device("predict")
        t = self.torch
        n, o, a = self.num_envs, self.obs_dim, self.action_dim
        is_np = not t.is_tensor(obs)
        ob = t.as_tensor(np.ascontiguousarray(obs, np.float32), device=self.device) if is_np else obs
        if self._scratch is None:
            f32 = dict(dtype=t.float32, device=self.device)
            self._scratch = (t.zeros((n, o), **f32), t.zeros((n, a), **f32), t.zeros(n, **f32), t.zeros(n, **f32))
        eps = t.zeros((n, a), dtype=t.float32, device=self.device) if deterministic else t.randn((n, a), dtype=t.float32, device=self.device)
        act = self.collect(ob.reshape(n, o).contiguous(), eps, *self._scratch)
        return (act.cpu().numpy() if is_np else act.clone()), None

    # ---- the torch side (autograd)
    def evaluate_actions(self, obs, actions):
        """ActorCriticPolicy.evaluate_actions -> (values [B], log_prob [B], entropy [B]) with autograd through the view-Parameters"""
        t = self.torch
        mean = self.actor(obs)
        values = self.critic(obs).flatten()
        dist = t.distributions.Normal(mean, self.log_std.exp().expand_as(mean))
        return values, dist.log_prob(actions).sum(-1), dist.entropy().sum(-1)

    # ---- SB3's names
    def state_dict(self):
        """under SB3's MlpPolicy keys (mlp_extractor.policy_net.*, mlp_extractor.value_net.*, action_net.*, value_net.*, log_std): copies"""
        sd = {"log_std": self.log_std.detach().clone()}
        for net, trunk, last in ((self.actor, "mlp_extractor.policy_net", "action_net"), (self.critic, "mlp_extractor.value_net", "value_net")):
            lins = [m for m in net if isinstance(m, self.torch.nn.Linear)]
            for i, lin in enumerate(lins):
                name = last if i == len(lins) - 1 else f"{trunk}.{2 * i}"
                sd[f"{name}.weight"], sd[f"{name}.bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
        return sd

    def load_state_dict(self, sd):
        """writes an SB3 MlpPolicy state dict INTO the flat tensors (the views and the kernels see it at once)"""
        t = self.torch
        with t.no_grad():
            for net, head in ((self.actor, "policy"), (self.critic, "value")):
                layers, log_std = layers_from_state_dict(sd, "ppo", head)
                lins = [m for m in net if isinstance(m, t.nn.Linear)]
                if len(layers) != len(lins):
                    raise ValueError(f"the state dict's {head} network has {len(layers)} layers, this one {len(lins)}")
                for lin, (w, b) in zip(lins, layers):
                    if tuple(w.shape) != tuple(lin.weight.shape) or tuple(b.shape) != tuple(lin.bias.shape):
                        raise ValueError(f"the state dict's {head} network has a layer of shape {tuple(w.shape)}, this one {tuple(lin.weight.shape)}")
                    lin.weight.copy_(t.as_tensor(w, dtype=t.float32))
                    lin.bias.copy_(t.as_tensor(b, dtype=t.float32))
                if log_std is not None:
                    self.log_std.copy_(t.as_tensor(_to_numpy(log_std), dtype=t.float32).reshape(self.action_dim))

    @classmethod
    def from_state_dict(cls, sd, num_envs=1, activation="tanh", **kw):
        """An SB3 PPO MlpPolicy state dict (names as remembered from stable_baselines3 1.5; the activation is not in a state dict)."""
        pi, _ = layers_from_state_dict(sd, "ppo", "policy")
        vf, _ = layers_from_state_dict(sd, "ppo", "value")
        self = cls(pi[0][0].shape[1], pi[-1][0].shape[0], net_arch=tuple(w.shape[0] for w, _ in pi[:-1]), vf_arch=tuple(w.shape[0] for w, _ in vf[:-1]),
                   activation=activation, num_envs=num_envs, ortho_init=False, **kw)
        self.load_state_dict(sd)
        return self

    @classmethod
    def load(cls, path, num_envs, activation="tanh", **kw):
        """an SB3 model .zip: its `policy.pth` (stable_baselines3 is not imported)"""
        return cls.from_state_dict(state_dict_from_zip(path), num_envs=num_envs, activation=activation, **kw)


class DeviceRolloutBuffer:
    """SB3's RolloutBuffer as [T, N, ...] float32 tensors on the device (episode_starts 0 / 1 as float32, as SB3 keeps them)."""

    def __init__(self, n_steps, num_envs, obs_dim, action_dim, gamma=0.99, gae_lambda=0.95, device=0):
        import torch
        self.torch = torch
        self.n_steps, self.num_envs, self.obs_dim, self.action_dim = int(n_steps), int(num_envs), int(obs_dim), int(action_dim)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        T, N = self.n_steps, self.num_envs
        f32 = dict(dtype=torch.float32, device=self.device)
        self.observations = torch.zeros((T, N, self.obs_dim), **f32)
        self.actions = torch.zeros((T, N, self.action_dim), **f32)
        for name in ("rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            setattr(self, name, torch.zeros((T, N), **f32))

    def compute_returns_and_advantage(self, last_values, dones):
        """RolloutBuffer.compute_returns_and_advantage in one launch (k_gae): last_values [N] float32, dones [N] uint8 or bool (the flags
        of the rollout's last step).  On torch's current stream."""
        t = self.torch
        if self.device.type != "cuda":
            raise RuntimeError(f"DeviceRolloutBuffer.compute_returns_and_advantage runs on a GPU; this buffer is on {self.device} (there is no CPU path)")
        lv = last_values.to(device=self.device, dtype=t.float32).reshape(self.num_envs).contiguous()
        ld = dones.to(device=self.device).reshape(self.num_envs).contiguous()
        ld = ld.view(t.uint8) if ld.dtype == t.bool else ld.to(t.uint8)
        with t.cuda.device(self.device):
            _lib.check(_lib.load().qs_gae(ptr(self.rewards), ptr(self.values), ptr(self.episode_starts), ptr(lv), ptr(ld), self.n_steps, self.num_envs,
                                          self.gamma, self.gae_lambda, ptr(self.advantages), ptr(self.returns),
                                          C.c_void_p(t.cuda.current_stream(self.device).cuda_stream)))
        self._keep = (lv, ld)      # alive until the kernel has read them

    def get(self, batch_size=None, generator=None):
        """yields dicts of minibatches (observations, actions, old_values, old_log_prob, advantages, returns) over one shuffled pass;
        batch_size None = everything at once.  Index gathers on the device."""
        t = self.torch
        total = self.n_steps * self.num_envs
        perm = t.randperm(total, device=self.device, generator=generator)
        flat = dict(observations=self.observations.view(total, self.obs_dim), actions=self.actions.view(total, self.action_dim),
                    old_values=self.values.view(total), old_log_prob=self.log_probs.view(total), advantages=self.advantages.view(total),
                    returns=self.returns.view(total))
        bs = total if batch_size is None else int(batch_size)
        for start in range(0, total, bs):
            idx = perm[start:start + bs]
            yield {k: v.index_select(0, idx) for k, v in flat.items()}


def ppo_loss(values, log_prob, entropy, old_values, old_log_prob, advantages, returns, clip_range=0.2, clip_range_vf=None, ent_coef=0.0,
             vf_coef=0.5, normalize_advantage=True):
    """The loss of one minibatch of SB3's PPO.train -> (loss, dict(policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction)); the
    dict's entries are detached tensors.  entropy None: approximated by -log_prob, as SB3 does."""
    import torch
    if normalize_advantage and advantages.numel() > 1:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    log_ratio = log_prob - old_log_prob
    ratio = torch.exp(log_ratio)
    policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range)).mean()
    values_pred = values if clip_range_vf is None else old_values + torch.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = torch.nn.functional.mse_loss(returns, values_pred)
    entropy_loss = -torch.mean(-log_prob) if entropy is None else -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        approx_kl = torch.mean((ratio - 1.0) - log_ratio)
        clip_fraction = torch.mean((torch.abs(ratio - 1.0) > clip_range).float())
    return loss, dict(policy_loss=policy_loss.detach(), value_loss=value_loss.detach(), entropy_loss=entropy_loss.detach(), approx_kl=approx_kl,
                      clip_fraction=clip_fraction)


class _PpoUpdate(DeviceHandle):
    """the qs_ppo handle of DevicePPO(update="device"), next to its policy's qs_ac handle"""
    _prefix, _owner = "qs_ppo", "learner"

    def __init__(self, learner):
        self.lib, self.torch, self.device, self.h = _lib.load(), learner.torch, learner.device, C.c_void_p()


class DevicePPO:
    """SB3's PPO over a QuadrupedVecEnv(auto_reset=True) or a DeviceVecNormalize around one.  env may be None for a learner that is only
    handed buffers (train())."""

    def __init__(self, env, policy, n_steps=128, batch_size=None, n_epochs=10, learning_rate=3e-4, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                 clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, target_kl=None, normalize_advantage=True, seed=0, update="torch"):
        """update: "torch" = PPO.train in torch with autograd (any policy a DeviceActorCritic takes, clip_range_vf); "device" = the same
        minibatches through qs_ppo_grad / qs_ppo_adam, for at most 2 hidden layers per network, widths and action_dim up to 64,
        clip_range_vf None and a constant learning_rate and clip_range: anything else raises ValueError here"""
        import torch
        self.torch = torch
        self.env, self.policy = env, policy
        if update not in ("torch", "device"):
            raise ValueError(f'update = {update!r} is neither "torch" nor "device"')
        self.update = update
        if update == "device":
            self._check_device_update(policy, learning_rate, clip_range, clip_range_vf)
        if env is not None:
            if (env.num_envs, env.obs_dim, env.action_dim) != (policy.num_envs, policy.obs_dim, policy.action_dim):
                raise ValueError(f"the environment has (num_envs, obs_dim, action_dim) = {(env.num_envs, env.obs_dim, env.action_dim)}, the policy "
                                 f"{(policy.num_envs, policy.obs_dim, policy.action_dim)}")
            if not getattr(env, "auto_reset", True):
                raise ValueError("DevicePPO needs an environment with auto_reset=True")
        self.n_steps, self.n_epochs = int(n_steps), int(n_epochs)
        self.batch_size = self.n_steps * policy.num_envs // 4 if batch_size is None else int(batch_size)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.clip_range, self.clip_range_vf, self.ent_coef, self.vf_coef = clip_range, clip_range_vf, ent_coef, vf_coef
        self.max_grad_norm, self.target_kl, self.normalize_advantage = max_grad_norm, target_kl, normalize_advantage
        self.device = policy.device
        self.buffer = DeviceRolloutBuffer(self.n_steps, policy.num_envs, policy.obs_dim, policy.action_dim, gamma, gae_lambda, device=self.device)
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=learning_rate, eps=1e-5)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self.num_timesteps = 0
        self._last_obs = None
        self._update = None           # the _PpoUpdate of update="device" on a GPU
        if update == "device":
            self._init_device_update(learning_rate)
        if env is not None:
            T, N = self.n_steps, policy.num_envs
            f32 = dict(dtype=torch.float32, device=self.device)
            self._normalised = raw_reward_of(env, None) is not None      # (a DeviceVecNormalize: its step_tensor also takes terminal_obs=)
            self._last_done = torch.ones(N, dtype=torch.uint8, device=self.device)      # the first step of the first rollout starts an episode
            self._term = torch.zeros((N, policy.obs_dim), **f32)
            self._last_values = torch.zeros(N, **f32)
            self._raw_rewards = torch.zeros((T, N), **f32)                                 # before normalisation and bootstrap: the printed returns
            self._ep_ret = torch.zeros(N, **f32)
            self._t_index = torch.arange(T, device=self.device).unsqueeze(1).expand(T, N)

    # ---- collection
    def _step(self, actions):
        """-> (obs, rew, done, truncated, raw reward) with the terminal observations of this step (normalised like obs) in self._term"""
        env = self.env
        if self._normalised:
            obs, rew, done, trunc = env.step_tensor(actions, terminal_obs=self._term)
            return obs, rew, done, trunc, env.old_reward
        obs, rew, done, trunc = env.step_tensor(actions)
        from .vec_env import INFO
        _lib.check(env.lib.qs_get_info(env.h, INFO["terminal_obs"], ptr(self._term)))   # (on the stream step_tensor has just set)
        return obs, rew, done, trunc, rew

    def collect_rollouts(self):
        """OnPolicyAlgorithm.collect_rollouts: fills self.buffer with n_steps steps of every environment and computes advantages and
        returns.  One torch.randn per rollout; per step one k_actor_critic launch, the environment step, three small copies (reward,
        raw reward, episode start) and the bootstrap launch for truncated environments.  Nothing waits for the device."""
        t, buf, pol = self.torch, self.buffer, self.policy
        if self._last_obs is None:
            self._last_obs = self.env.reset_tensor()
        eps = t.randn((self.n_steps, pol.num_envs, pol.action_dim), dtype=t.float32, device=self.device, generator=self.generator)
        obs, done = self._last_obs, self._last_done
        with t.no_grad():
            for k in range(self.n_steps):
                buf.episode_starts[k].copy_(done)
                actions = pol.collect(obs, eps[k], buf.observations[k], buf.actions[k], buf.values[k], buf.log_probs[k])
                obs, rew, done, trunc, raw = self._step(actions)
                buf.rewards[k].copy_(rew)
                self._raw_rewards[k].copy_(raw)
                pol.bootstrap(self._term, trunc, self.gamma, buf.rewards[k])
            pol.predict_values(obs, out=self._last_values)
            buf.compute_returns_and_advantage(self._last_values, done)
        self._last_obs, self._last_done = obs, done
        self.num_timesteps += self.n_steps * pol.num_envs

    def episode_stats(self):
        """-> (sum of the raw returns of the episodes that ended inside the last rollout, their number) as device tensors; carries the
        running returns over to the next rollout.  Call once per rollout."""
        t, buf = self.torch, self.buffer
        dones = t.cat([buf.episode_starts[1:], self._last_done.to(t.float32).unsqueeze(0)], 0) > 0.5
        c = t.cumsum(self._raw_rewards, 0) + self._ep_ret                            # the return so far, never reset
        last = t.cummax(t.where(dones, self._t_index, -1), 0).values                  # the latest end at or before t
        prev = t.cat([t.full_like(last[:1], -1), last[:-1]], 0)                       # ... strictly before t
        base = t.where(prev >= 0, c.gather(0, prev.clamp(min=0)), t.zeros_like(c))
        ret_sum, count = ((c - base) * dones).sum(), dones.sum()
        self._ep_ret = c[-1] - t.where(last[-1] >= 0, c.gather(0, last[-1:].clamp(min=0))[0], t.zeros_like(c[-1]))
        return ret_sum, count

    # ---- the update on the device
    @staticmethod
    def _check_device_update(policy, learning_rate, clip_range, clip_range_vf):
        why = None
        for who, arch in (("actor", policy.net_arch), ("critic", policy.vf_arch)):
            if len(arch) > UPDATE_MAX_HIDDEN:
                why = why or f"the {who} has {len(arch)} hidden layers, the device update takes at most {UPDATE_MAX_HIDDEN}"
            if any(w > UPDATE_MAX_WIDTH for w in arch):
                why = why or f"the {who}'s widths {tuple(arch)} exceed {UPDATE_MAX_WIDTH} (a layer's weight-gradient tiles stay in registers)"
        if policy.action_dim > UPDATE_MAX_WIDTH:
            why = why or f"action_dim = {policy.action_dim} exceeds {UPDATE_MAX_WIDTH}"
        if clip_range_vf is not None:
            why = why or f"clip_range_vf = {clip_range_vf!r} is not supported (only None)"
        if callable(learning_rate) or callable(clip_range):
            why = why or "learning_rate and clip_range must be constants, not schedules"
        if why:
            raise ValueError(f'DevicePPO(update="device"): {why}; update="torch" takes it')

    def _hyper(self):
        return _lib.QsPpoHyper(float(self.clip_range), float(self.ent_coef), float(self.vf_coef), NO_CLIP if self.max_grad_norm is None else float(self.max_grad_norm),
                               int(bool(self.normalize_advantage)), 0, float(self.learning_rate), 0.9, 0.999, 1e-5)

    def _init_device_update(self, learning_rate):
        """Adam's state as two flat tensors over [actor | critic | log_std] (exp_avg, exp_avg_sq), the last gradient (grad), the step count;
        on a GPU the qs_ppo handle bound to the policy's own parameter memory"""
        t, pol = self.torch, self.policy
        self.learning_rate = float(learning_rate)
        n = pol.actor_params.numel() + pol.critic_params.numel() + pol.action_dim
        f32 = dict(dtype=t.float32, device=self.device)
        self.exp_avg, self.exp_avg_sq, self.grad = t.zeros(n, **f32), t.zeros(n, **f32), t.zeros(n, **f32)
        self._stats = t.zeros(len(_lib.PPO_STATS), **f32)
        self.adam_step = 0
        if self.device.type != "cuda":
            return
        up = self._update = _PpoUpdate(self)
        self.lib = up.lib

        def desc(out_dim, arch):
            return _lib.QsPolicyDesc(pol.num_envs, 1, pol.obs_dim, out_dim, len(arch), (C.c_int32 * 4)(*arch), ACTIVATIONS[pol.activation], 0, 1, -NO_CLIP, NO_CLIP)
        _lib.check(up.lib.qs_ppo_create(C.byref(desc(pol.action_dim, pol.net_arch)), C.byref(desc(1, pol.vf_arch)), self.n_steps * pol.num_envs,
                                        self.device.index or 0, C.byref(up.h)))
        _lib.check(up.lib.qs_ppo_bind(up.h, ptr(pol.actor_params), ptr(pol.critic_params), ptr(pol.log_std.data), ptr(self.exp_avg), ptr(self.exp_avg_sq)))

    @property
    def hp(self):
        """the qs_ppo handle (None without one: update="torch", or no GPU)"""
        return None if self._update is None else self._update.h

    def _read_stats(self):
        """the statistics of the last minibatch as python floats (waits for the device); raises if any minibatch since the last read
        refused samples (the handle's counter, qs_ppo_refusals, which this read clears)"""
        out = dict(zip(_lib.PPO_STATS, self._stats.cpu().tolist()))
        count = C.c_uint64(0)
        _lib.check(self.lib.qs_ppo_refusals(self.hp, C.byref(count)))
        if count.value > 0:
            raise RuntimeError(f"qs_ppo_grad refused {count.value} samples since the last statistics read: indices outside [0, total)")
        return out

    def grad_minibatch(self, idx):
        """qs_ppo_grad for the minibatch idx (int64 tensor of indices into the flat [T * N] rollout) -> self.grad, self._stats; on torch's
        current stream, waits for nothing"""
        t, buf = self.torch, self.buffer
        if self.hp is None:
            raise RuntimeError(f'DevicePPO(update="device") trains on a GPU; this one was built on {self.device} (there is no CPU path)')
        p_idx = self._update._arg("idx", idx, getattr(idx, "shape", ()), t.int64)      # (any shape: its numel() indices)
        self._hy = self._hyper()
        self._update._stream()
        _lib.check(self.lib.qs_ppo_grad(self.hp, ptr(buf.observations), ptr(buf.actions), ptr(buf.log_probs), ptr(buf.advantages), ptr(buf.returns),
                                        buf.n_steps * buf.num_envs, p_idx, idx.numel(), C.byref(self._hy), ptr(self.grad), ptr(self._stats)))

    def adam_minibatch(self):
        """qs_ppo_adam with self.grad: clip_grad_norm_ and optimizer.step() in place on the policy's parameters"""
        self.adam_step += 1
        _lib.check(self.lib.qs_ppo_adam(self.hp, ptr(self.grad), C.byref(self._hy), self.adam_step, ptr(self._stats)))

    def _train_device(self):
        t = self.torch
        total, bs = self.n_steps * self.policy.num_envs, self.batch_size
        epochs_run, go_on, ran = 0, True, False
        for _ in range(self.n_epochs):
            perm = t.randperm(total, device=self.device, generator=self.generator)     # (DeviceRolloutBuffer.get's, from the same generator)
            for start in range(0, total, bs):
                self.grad_minibatch(perm[start:start + bs])
                ran = True
                if self.target_kl is not None and self._read_stats()["approx_kl"] > 1.5 * self.target_kl:
                    go_on = False
                    break
                self.adam_minibatch()
            if not go_on:
                break
            epochs_run += 1
        s = self._read_stats() if ran else {}                             # (n_epochs = 0: nothing ran, every figure is nan)
        out = {k: s.get(k, float("nan")) for k in ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")}
        out["grad_norm"] = s.get("grad_norm", float("nan")) if go_on else float("nan")      # (the early stop skips the step that would have measured it)
        out["n_epochs_run"] = epochs_run
        return out

    def close(self):
        """frees the qs_ppo handle (as its garbage collection does, and the end of a `with` block)"""
        if self._update is not None:
            self._update.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- the update
    def train(self):
        """SB3's PPO.train on self.buffer -> dict(approx_kl, policy_loss, value_loss, entropy_loss, clip_fraction, grad_norm, n_epochs_run)
        of python floats (the one host synchronisation, at the end; with target_kl one per minibatch, as the early stop needs the value).
        grad_norm is the last minibatch's norm before clipping (nan if the early stop skipped that step)."""
        if self.update == "device":
            return self._train_device()
        t, pol = self.torch, self.policy
        params = pol.parameters()
        last, epochs_run, go_on, norm = None, 0, True, None
        for _ in range(self.n_epochs):
            for mb in self.buffer.get(self.batch_size, generator=self.generator):
                values, log_prob, entropy = pol.evaluate_actions(mb["observations"], mb["actions"])
                loss, info = ppo_loss(values, log_prob, entropy, mb["old_values"], mb["old_log_prob"], mb["advantages"], mb["returns"], self.clip_range,
                                      self.clip_range_vf, self.ent_coef, self.vf_coef, self.normalize_advantage)
                last = info
                if self.target_kl is not None and float(info["approx_kl"]) > 1.5 * self.target_kl:
                    go_on = False
                    break
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                norm = t.nn.utils.clip_grad_norm_(params, float("inf") if self.max_grad_norm is None else self.max_grad_norm)
                self.optimizer.step()
            if not go_on:
                break
            epochs_run += 1
        out = {k: float(v) for k, v in last.items()}
        out["grad_norm"] = float(norm) if go_on and norm is not None else float("nan")
        out["n_epochs_run"] = epochs_run
        return out

    def learn(self, total_timesteps, log=print):
        """collect, train, one line per iteration (the line's mean return is the iteration's one host synchronisation besides train()'s)"""
        it = 0
        while self.num_timesteps < total_timesteps:
            self.collect_rollouts()
            ret_sum, count = self.episode_stats()
            info = self.train()
            n = int(count)
            mean_ret = float(ret_sum) / n if n else float("nan")
            log(f"iteration {it:3d}: timesteps {self.num_timesteps:9d}   episodes {n:6d}   mean return {mean_ret:9.3f}   approx_kl {info['approx_kl']:.4f}   "
                f"value_loss {info['value_loss']:.4f}   epochs {info['n_epochs_run']}")
            it += 1
        return self
