"""DeviceMPC: sampling MPC over device forks (examples/mpc.py's predictive sampling, and MPPI) with the planner's bookkeeping on the device
(csrc/qs_mpc.hip).  M real robots and C candidates each live in ONE handle of N = M (1 + C) environments: the real robots are the
environments [0, M), candidate c of robot m is environment M + m C + c.  A control step is one fork (every real robot into its candidates),
one launch that samples the H-step action sequences around the plan (candidate 0 is the plan itself), per horizon step one small launch
next to the step kernel (`feed`: the score of the step before, the running flags, the next slab of actions, the active mask), and one launch
that chooses (`finish`: the best candidate, or MPPI's weighted mean) and shifts the plan.  Nothing leaves the GPU and the host waits for
nothing.  No floating-point atomics and a summation order that is a function of the shapes alone (csrc/qs_mpc.h): a run is reproducible bit
for bit from its seed, under either method.

Two rules are this project's own and are stated as such: among candidates of equal score the lowest index wins (torch.argmax leaves ties
unspecified on the device), and a score that is not finite counts as -inf (a robot whose scores are all non-finite keeps its plan)."""
import ctypes as C

from . import lib as _lib
from .handle import DeviceHandle, env_mask, ptr, raw_reward_of, takes_active

MAX_CANDIDATES = 4096      # csrc/qs_mpc.h: a robot's weights lie in one workgroup's LDS
MAX_ELEMENTS = 1024        # horizon * action_dim: one lane per element of a sequence
METHOD = dict(best=0, mppi=1)                                                      # QS_MPC_BEST, QS_MPC_MPPI
GET = dict(plan=0, seq=1, score=2, running=3, best=4, best_score=5)                # QS_MPC_GET_*


class DeviceMPC(DeviceHandle):
    """The planner over a QuadrupedVecEnv, or a DeviceVecNormalize(training=False) around one (the scores then use old_reward, the raw
    reward, as DeviceARS does).  env may be None for a planner that is only handed rewards and dones (sample / feed / finish); it then needs
    action_dim and device."""
    _prefix, _owner = "qs_mpc", "planner"

    def __init__(self, env, n_robots, n_candidates, horizon, sigma=0.5, method="best", temperature=1.0, freeze_done=False, seed=0,
                 action_dim=None, device=None):
        """method "best": the best of the C candidates is the next plan; "mppi": the mean of the candidates under the weights
        exp((score - max) / temperature).  freeze_done=True: the rollouts step with the mask `feed` writes (step_tensor(active=)) -- the real
        robots are frozen while their candidates roll out, so no snapshot and restore of them is taken, and a candidate whose episode has
        ended is no longer stepped; the real robots' one step then steps them alone.  The scores ignore a candidate from the end of its
        episode on either way: states, plans and scores are the same bits as with freeze_done=False."""
        import torch
        self.torch = torch
        self.env = env
        self.M, self.C, self.H = int(n_robots), int(n_candidates), int(horizon)
        for name, v in (("n_robots", self.M), ("n_candidates", self.C), ("horizon", self.H)):
            if v < 1:
                raise ValueError(f"{name} = {v} must be positive")
        if self.C > MAX_CANDIDATES:
            raise ValueError(f"n_candidates = {self.C} is above {MAX_CANDIDATES} (a robot's weights lie in one workgroup's LDS)")
        self.num_envs = self.M * (1 + self.C)
        if method not in METHOD:
            raise ValueError(f"method must be one of {sorted(METHOD)}, got {method!r}")
        self.method, self.sigma, self.temperature = method, float(sigma), float(temperature)
        if not self.temperature > 0.0 or self.temperature == float("inf"):
            raise ValueError(f"temperature = {temperature} must be a positive finite number")
        if self.sigma != self.sigma or abs(self.sigma) == float("inf"):
            raise ValueError(f"sigma = {sigma} must be finite")
        self.freeze_done = bool(freeze_done)
        if env is not None:
            if type(env).__name__ == "ShardedVecEnv":
                raise ValueError("DeviceMPC does not take a ShardedVecEnv: the real robots and their candidates live in one handle")
            if int(env.num_envs) != self.num_envs:
                raise ValueError(f"the environment has num_envs = {env.num_envs}, expected n_robots * (1 + n_candidates) = {self.num_envs}")
            if hasattr(env, "venv") and getattr(env, "training", False):
                raise ValueError("DeviceMPC takes a DeviceVecNormalize with training=False (the candidates' rollouts must not move the statistics)")
            if self.freeze_done and not takes_active(env):
                raise ValueError(f"freeze_done=True needs an environment whose step_tensor takes active= ({type(env).__name__}.step_tensor does not)")
            self.d, self.device = int(env.action_dim), env.device
        else:
            if action_dim is None:
                raise ValueError("a planner without an environment needs action_dim")
            self.d, self.device = int(action_dim), torch.device("cuda", 0) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device = {self.device}: DeviceMPC has no CPU path")
        if self.d < 1 or self.H * self.d > MAX_ELEMENTS:
            raise ValueError(f"horizon * action_dim = {self.H * self.d} is outside [1, {MAX_ELEMENTS}] (one lane per element of a sequence)")
        self.lib = _lib.load()
        self.h = C.c_void_p()
        _lib.check(self.lib.qs_mpc_create(self.M, self.C, self.H, self.d, self.device.index or 0, C.byref(self.h)))
        M, MC, H, d, n = self.M, self.M * self.C, self.H, self.d, self.num_envs
        f32, i32, u8 = (dict(dtype=dt, device=self.device) for dt in (torch.float32, torch.int32, torch.uint8))
        self.actions = torch.zeros((n, d), **f32)          # [:M] the real robots' (written by finish), [M:] the candidates' (written by feed)
        self.active = torch.ones(n, **u8)                   # the mask feed writes under freeze_done
        self._out = dict(plan=torch.zeros((M, H, d), **f32), seq=torch.zeros((H, MC, d), **f32), score=torch.zeros(MC, **f32),
                         running=torch.zeros(MC, **u8), best=torch.zeros(M, **i32), best_score=torch.zeros(M, **f32))
        # the source of every environment for the fork: -1 (left alone) for the real robots, robot m for its candidates
        self.src_of = torch.cat([torch.full((M,), -1, **i32), torch.arange(M, **i32).repeat_interleave(self.C)])
        self.real_mask = torch.zeros(n, **u8)
        self.real_mask[:M] = 1
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self._keep = None
        self._hold = None

    def get(self, what):
        """a device tensor with the handle's `what` (one of GET; a reused buffer, a stream-ordered copy): plan [M, H, d]; seq [H, M C, d];
        score float32 and running uint8 [M C]; best int32 and best_score float32 [M] of the last finish"""
        return self._get(what, GET, self._out)

    # ---- the steps of a control step (csrc/qs_mpc.h 1-3)
    def sample_eps(self):
        t = self.torch
        return t.randn((self.H, self.M * self.C, self.d), dtype=t.float32, device=self.device, generator=self.generator)

    def sample(self, eps):
        """the candidates' sequences from eps [H, M C, d]: candidate 0 is the plan, the others clamp(plan + sigma * eps, -1, 1)"""
        p = self._arg("eps", eps, (self.H, self.M * self.C, self.d))
        self._stream()
        _lib.check(self.lib.qs_mpc_sample(self.h, p, self.sigma))
        self._hold = eps

    def feed(self, h, reward=None, done=None, reward_end=None):
        """horizon step h = 0 .. H: accounts the step before it (reward float32 [N], done uint8 [N]; h >= 1), copies step h's actions into
        self.actions[M:] (h < H), at h == H adds reward_end [N, k] (its first column) where a candidate is still running; under freeze_done
        writes self.active"""
        t, n = self.torch, self.num_envs
        h = int(h)
        if not 0 <= h <= self.H:
            raise ValueError(f"h = {h} is outside [0, horizon = {self.H}]")
        pr = pd = pe = None
        stride = 0
        if h >= 1:
            pr, pd = self._arg("reward", reward, (n,)), self._arg("done", done, (n,), t.uint8)
        if h == self.H:
            if not t.is_tensor(reward_end) or reward_end.dim() != 2:
                raise ValueError("reward_end must be a float32 tensor [N, k] (get_info('reward_end'))")
            pe, stride = self._arg("reward_end", reward_end, (n, reward_end.shape[1])), int(reward_end.shape[1])
        self._stream()
        _lib.check(self.lib.qs_mpc_feed(self.h, h, pr, pd, pe, stride, ptr(self.actions), ptr(self.active) if self.freeze_done else None))
        self._hold = (reward, done, reward_end)

    def finish(self):
        """the choice: self.actions[:M] = the chosen sequences' first actions, the plan = the rest with the last action held"""
        self._stream()
        _lib.check(self.lib.qs_mpc_finish(self.h, METHOD[self.method], self.temperature, ptr(self.actions)))

    def set_plan(self, plan):
        p = self._arg("plan", plan, (self.M, self.H, self.d))
        self._stream()
        _lib.check(self.lib.qs_mpc_set_plan(self.h, p, None))
        self._hold = plan

    def reset_plan(self, indices=None):
        """zero plans for the robots `indices` (None: all): robot ids, or a bool / uint8 mask [M] on the device (used as it is, no wait)"""
        m = env_mask(indices, self.M, self.device)
        self._stream()
        _lib.check(self.lib.qs_mpc_set_plan(self.h, None, ptr(m)))
        self._hold = m

    # ---- the control loop
    def _step(self, active=None):
        """-> (raw reward, done) of one step of every environment under self.actions"""
        _, rew, done, _ = self.env.step_tensor(self.actions) if active is None else self.env.step_tensor(self.actions, active=active)
        return raw_reward_of(self.env, rew), done

    def plan(self):
        """One control step's planning: fork, sample, H feeds and steps, finish.  Leaves the chosen first actions in self.actions[:M], the
        next plan in the handle, and the real robots where they were."""
        if self.env is None:
            raise RuntimeError("DeviceMPC.plan needs an environment")
        env = self.env
        env.fork(src_of=self.src_of)
        if not self.freeze_done:
            self._keep = env.snapshot(indices=self.real_mask, out=self._keep)     # the real robots step along: put back below
        self.sample(self.sample_eps())
        rew = done = None
        for h in range(self.H):
            self.feed(h, rew, done)
            rew, done = self._step(self.active if self.freeze_done else None)
        self.feed(self.H, rew, done, env.get_info("reward_end"))
        self.finish()
        if not self.freeze_done:
            env.restore(self._keep, indices=self.real_mask)

    def step(self):
        """plan(), then the one step the real robots take under the chosen actions -> their rows of (obs, rew, done, truncated) (views of the
        environment's reused buffers).  A robot whose episode ended in that step starts the next one from a zero plan."""
        self.plan()
        env = self.env
        if self.freeze_done:
            obs, rew, done, trunc = env.step_tensor(self.actions, active=self.real_mask)      # the candidates are forked again before they are read
        else:
            obs, rew, done, trunc = env.step_tensor(self.actions)
        M = self.M
        self.reset_plan(done[:M])
        return obs[:M], rew[:M], done[:M], trunc[:M]
