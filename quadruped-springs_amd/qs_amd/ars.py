"""DeviceARS: sb3_contrib's ARS (Augmented Random Search, the reference's first training step, load_model.py:45) with an iteration's
bookkeeping on the device (csrc/qs_ars.hip): the candidates theta +- delta_std * delta in one launch into the tensor DevicePolicy reads in
place, the episode accounting of the rollout as one small launch per environment step, and ARS._do_one_update -- the candidates' returns,
the choice of the n_top best directions, the step -- as three launches.  The host waits for the device once per `check_every` steps (to see
whether every episode has ended), not once per step; nothing else leaves the GPU.  No floating-point atomics and a summation order that
is a function of the shapes alone (csrc/qs_ars.h): a run is reproducible bit for bit from its seed.

All 2 n_delta candidates are evaluated in ONE rollout: candidate p drives the block of environments [p m, (p + 1) m), m = num_envs / (2 n_delta),
which is DevicePolicy(n_policies=2 n_delta)'s rule; the + candidates come first.  A candidate's return is the SUM over its block
(sb3_contrib sums a candidate's n_eval_episodes the same way; the update is invariant to a common factor only through its std).

The formulas, keyword names and defaults are sb3_contrib 1.5's as remembered (ars/ars.py); the package was not available to check them
against.  Two rules are this project's own and are stated as such: ties between directions go to the lower index (torch.argsort leaves them
unspecified), and an environment still running at `horizon` contributes what it has collected."""
import ctypes as C

from . import lib as _lib
from .handle import DeviceHandle, auto_reset_of, ptr, raw_reward_of, takes_active

MAX_DELTA = 1024      # csrc/qs_ars.h: the selection is one workgroup
GET = dict(ret=0, len=1, episodes=2, alive=3, n_alive=4, steps=5, returns=6, idx=7, w=8, stats=9)   # QS_ARS_GET_*


class DeviceARS(DeviceHandle):
    """ARS over a QuadrupedVecEnv or a DeviceVecNormalize around one.  `policy` is a DevicePolicy(num_envs=N, n_policies=2 n_delta) (anything
    with n_params, n_policies, num_envs, device and set_params).  env may be None for a learner that is only handed rewards and dones
    (begin / account / finish)."""
    _prefix, _owner = "qs_ars", "learner"

    def __init__(self, env, policy, n_delta=8, n_top=None, learning_rate=0.02, delta_std=0.05, zero_policy=True, alive_bonus_offset=0.0,
                 episodes_per_env=1, horizon=300, check_every=16, seed=0, freeze_done=False):
        """freeze_done=True: rollout() steps with active = the environments still alive (step_tensor(active=)), so a robot whose episodes
        are over is no longer stepped -- it lies on the floor, on the slow many-rows contact path, and every launch waits for its slowest
        wave.  The accounts ignore dead environments either way: on an environment without observation normalisation in training mode the
        per-environment returns and lengths, the candidates' returns, idx, w and theta are the same bits as with freeze_done=False.  Under a
        DeviceVecNormalize(training=True) the running statistics then see living robots only, so the results differ by design."""
        import torch
        self.torch = torch
        self.env, self.policy = env, policy
        self.n_delta = int(n_delta)
        self.n_top = self.n_delta if n_top is None else int(n_top)
        P = 2 * self.n_delta
        if self.n_delta < 1 or self.n_delta > MAX_DELTA:
            raise ValueError(f"n_delta = {n_delta} is outside [1, {MAX_DELTA}] (the selection is one workgroup)")
        if not 1 <= self.n_top <= self.n_delta:
            raise ValueError(f"n_top = {n_top} is outside [1, n_delta = {self.n_delta}]")
        if int(policy.n_policies) != P:
            raise ValueError(f"policy.n_policies = {policy.n_policies}, expected 2 * n_delta = {P}")
        self.num_envs, self.n_params = int(policy.num_envs), int(policy.n_params)
        if self.num_envs < P or self.num_envs % P:
            raise ValueError(f"num_envs = {self.num_envs} is not divisible by the 2 * n_delta = {P} candidates")
        self.episodes_per_env, self.horizon, self.check_every = int(episodes_per_env), int(horizon), int(check_every)
        for name in ("episodes_per_env", "horizon", "check_every"):
            if getattr(self, name) < 1:
                raise ValueError(f"{name} = {getattr(self, name)} must be positive")
        if env is not None:
            if int(env.num_envs) != self.num_envs:
                raise ValueError(f"the environment has num_envs = {env.num_envs}, the policy {self.num_envs}")
            if self.episodes_per_env > 1 and auto_reset_of(env) is not True:
                raise ValueError(f"episodes_per_env = {self.episodes_per_env} needs an environment with auto_reset=True (an environment that is not reset "
                                 "has no second episode)")
        self.learning_rate, self.delta_std, self.alive_bonus_offset = float(learning_rate), float(delta_std), float(alive_bonus_offset)
        self.freeze_done = bool(freeze_done)
        if self.freeze_done and env is not None and not takes_active(env):
            raise ValueError(f"freeze_done=True needs an environment whose step_tensor takes active= ({type(env).__name__}.step_tensor does not)")
        self.device = policy.device
        if self.device.type != "cuda":
            raise ValueError(f"policy.device = {self.device}: DeviceARS has no CPU path")
        self.block = self.num_envs // P
        self.lib = _lib.load()
        f32 = dict(dtype=torch.float32, device=self.device)
        if zero_policy:
            self.theta = torch.zeros(self.n_params, **f32)
        else:
            if getattr(policy, "_params", None) is None:
                raise ValueError("zero_policy=False takes theta from the policy's first parameter row: call policy.set_params first")
            self.theta = policy.get_params()[0].clone()
        self.candidates = torch.zeros((P, self.n_params), **f32)
        policy.set_params(self.candidates)                                  # kept in place: perturb() writes what the next act() reads
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self.h = C.c_void_p()
        _lib.check(self.lib.qs_ars_create(self.num_envs, self.n_delta, self.n_params, self.episodes_per_env, self.device.index or 0, C.byref(self.h)))
        i32 = dict(dtype=torch.int32, device=self.device)
        self._out = dict(ret=torch.zeros(self.num_envs, **f32), len=torch.zeros(self.num_envs, **i32), episodes=torch.zeros(self.num_envs, **i32),
                         alive=torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device), n_alive=torch.zeros(1, **i32),
                         steps=torch.zeros(1, dtype=torch.int64, device=self.device), returns=torch.zeros(P, **f32), idx=torch.zeros(self.n_delta, **i32),
                         w=torch.zeros(self.n_delta, **f32), stats=torch.zeros(2, **f32))
        self.delta = None
        self.num_timesteps = 0
        self.iteration = 0
        self.last_rollout_steps = 0

    def get(self, what):
        """a device tensor with the handle's `what` (one of GET; a reused buffer, a stream-ordered copy): ret, len, episodes, alive [N];
        n_alive, steps [1]; returns [2 n_delta]; idx, w [n_top] of the last finish; stats [2] = std, step"""
        out = self._get(what, GET, self._out)
        return out[:self.n_top] if what in ("idx", "w") else out

    # ---- the steps of an iteration (csrc/qs_ars.h 1-6)
    def sample_delta(self):
        t = self.torch
        return t.randn((self.n_delta, self.n_params), dtype=t.float32, device=self.device, generator=self.generator)

    def perturb(self, delta):
        """candidates = theta +- delta_std * delta, written into the tensor the policy reads; delta is kept for finish()"""
        p = self._arg("delta", delta, (self.n_delta, self.n_params))
        self._stream()
        _lib.check(self.lib.qs_ars_perturb(self.h, ptr(self.theta), p, self.delta_std, ptr(self.candidates)))
        self.delta = delta
        return self.candidates

    def begin(self):
        self._stream()
        _lib.check(self.lib.qs_ars_begin(self.h))

    def account(self, raw_reward, done):
        """one environment step: raw_reward float32 [N], done uint8 [N]"""
        pr, pd = self._arg("raw_reward", raw_reward, (self.num_envs,)), self._arg("done", done, (self.num_envs,), self.torch.uint8)
        self._stream()
        _lib.check(self.lib.qs_ars_account(self.h, pr, pd))

    def alive(self):
        """the number of environments still alive (waits for the device)"""
        n = C.c_int(-1)
        self._stream()
        _lib.check(self.lib.qs_ars_alive(self.h, C.byref(n)))
        return n.value

    def candidate_returns(self):
        """the per-candidate returns [2 n_delta] of the accounts as they are (+ candidates first)"""
        self._stream()
        _lib.check(self.lib.qs_ars_returns(self.h, self.alive_bonus_offset))
        return self.get("returns")

    def finish(self, delta=None):
        """returns, selection and the step on theta, in place and stream-ordered; delta defaults to the last perturb()'s"""
        delta = self.delta if delta is None else delta
        if delta is None:
            raise RuntimeError("DeviceARS.finish before perturb")
        p = self._arg("delta", delta, (self.n_delta, self.n_params))
        self._stream()
        _lib.check(self.lib.qs_ars_finish(self.h, ptr(self.theta), p, self.n_top, self.learning_rate, self.alive_bonus_offset))

    # ---- sb3_contrib's surface
    def _step(self, actions, active=None):
        """-> (obs, raw reward, done)"""
        obs, rew, done, _ = self.env.step_tensor(actions) if active is None else self.env.step_tensor(actions, active=active)
        return obs, raw_reward_of(self.env, rew), done

    def rollout(self):
        """One episode batch of every candidate (the candidates must be in place: perturb): -> the per-candidate returns [2 n_delta].  Stops
        when no environment is alive, looked at every check_every steps, or at horizon."""
        if self.env is None:
            raise RuntimeError("DeviceARS.rollout needs an environment")
        obs = self.env.reset_tensor()
        self.begin()
        steps = 0
        while steps < self.horizon:
            # (freeze_done: the alive flags as the previous step's account left them, a stream-ordered copy -- no wait)
            obs, raw, done = self._step(self.policy.act(obs), self.get("alive") if self.freeze_done else None)
            self.account(raw, done)
            steps += 1
            if steps % self.check_every == 0 and self.alive() == 0:
                break
        self.last_rollout_steps = steps
        return self.candidate_returns()

    evaluate_candidates = rollout

    def train_iteration(self):
        """ARS._do_one_update: draw the directions, evaluate the candidates, step.  -> the per-candidate returns (a reused device tensor)"""
        self.perturb(self.sample_delta())
        returns = self.rollout()
        self.finish()
        self.iteration += 1
        return returns

    _do_one_update = train_iteration

    def learn(self, total_timesteps, log=print):
        """iterations until num_timesteps (the device's sum of episode lengths) reaches total_timesteps; one line per iteration"""
        while self.num_timesteps < total_timesteps:
            returns = self.train_iteration()
            self.num_timesteps += int(self.get("steps").item())
            if log:
                std, step = self.get("stats").tolist()
                r = returns / self.block
                log(f"iteration {self.iteration:3d}: timesteps {self.num_timesteps:9d}  mean return {r.mean().item():9.3f}  best candidate {r.max().item():9.3f}  "
                    f"std of the kept {std:9.3f}  step {step:.3e}")
        return self

    def to_policy(self, num_envs):
        """a one-policy DevicePolicy of the same network on a copy of theta"""
        from .policy import DevicePolicy
        p = self.policy
        pol = DevicePolicy(p.obs_dim, p.action_dim, net_arch=p.net_arch, activation=p.activation, squash_output=p.squash_output, bias=p.bias,
                           num_envs=num_envs, n_policies=1, clip=p.clip, device=self.device)
        pol.set_params(self.theta.clone().unsqueeze(0))
        return pol

    def state_dict(self):
        """theta in the key names policy.layers_from_state_dict(algo="ars") reads (sb3_contrib's ARS policies, as remembered): a bare
        action_net.weight for the linear policy, action_net.{0, 2, ..} for an MLP; biases where the policy has them"""
        from .policy import layer_shapes
        p = self.policy
        shapes = layer_shapes(p.obs_dim, p.action_dim, p.net_arch)
        flat, at, sd = self.theta.detach().cpu(), 0, {}
        for l, (o, i) in enumerate(shapes):
            name = "action_net" if len(shapes) == 1 else f"action_net.{2 * l}"
            sd[f"{name}.weight"] = flat[at:at + o * i].reshape(o, i).clone()
            at += o * i
            if p.bias:
                sd[f"{name}.bias"] = flat[at:at + o].clone()
                at += o
        assert at == self.n_params
        return sd
