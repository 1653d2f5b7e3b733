"""DeviceVecNormalize: SB3's VecNormalize (stable_baselines3 1.5.1a7, common/vec_env/vec_normalize.py) with its running
statistics and the normalisation on the GPU, for consumers that keep observations on the device.

The reference applies VecNormalize at load_model.py:109-137 / get_demonstrations.py:71 (`VecNormalize.load(stats, env)`, then
`training = False`, `norm_reward = False`).  SB3's own numpy VecNormalize also wraps QuadrupedVecEnv unchanged; this class is
for `step_tensor` users.  Statistics are float64 on the device; `get_stats` / `set_stats` / `save` / `load` exchange them as the
attributes SB3 pickles (obs_rms.mean/var/count, ret_rms.mean/var/count, clip_obs, clip_reward, gamma, epsilon)."""
import ctypes as C

import numpy as np

from . import lib as _lib
from .handle import DeviceHandle, active_mask, env_mask, ptr


class DeviceVecNormalize(DeviceHandle):
    _prefix, _owner = "qs_norm", "wrapper"

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        self.venv = venv
        self.torch = venv.torch
        self.lib = _lib.load()
        self.num_envs, self.obs_dim, self.action_dim, self.device = venv.num_envs, venv.obs_dim, venv.action_dim, venv.device
        self.observation_space, self.action_space = venv.observation_space, venv.action_space
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.h = C.c_void_p()
        _lib.check(self.lib.qs_norm_create(self.num_envs, self.obs_dim, clip_obs, clip_reward, gamma, epsilon, self.device.index or 0, C.byref(self.h)))
        t = self.torch
        self.old_obs = t.zeros((self.num_envs, self.obs_dim), dtype=t.float32, device=self.device)
        self.old_reward = t.zeros(self.num_envs, dtype=t.float32, device=self.device)
        self._term = t.zeros((self.num_envs, self.obs_dim), dtype=t.float32, device=self.device)

    # ---- device path
    def reset_tensor(self, mask=None):
        obs = self.venv.reset_tensor(mask)
        self.old_obs.copy_(obs)
        self._stream()
        _lib.check(self.lib.qs_norm_reset(self.h, ptr(obs), int(self.training), int(self.norm_obs)))
        return obs

    def step_tensor(self, actions, terminal_obs=None, active=None):
        """-> (obs, rew, done, truncated): normalised in place in the environment's reused buffers; the raw values of this step
        stay in `old_obs` / `old_reward` (VecNormalize.get_original_obs / get_original_reward).  terminal_obs: a float32 [N, obs_dim]
        tensor on the device that receives the step's terminal observations (get_info("terminal_obs")) normalised with this step's
        statistics, as VecNormalize.step_wait normalises infos[i]["terminal_observation"].
        active: the environment's step_tensor(active=) mask (qs_norm_step_masked).  With training=True the batch moments of observations and
        returns are taken over the active rows only, the batch count is their number, and only their returns advance and are cleared at
        done; a step without an active row updates nothing.  Every row, frozen ones included, is normalised with the step's statistics, and
        old_obs / old_reward hold every row."""
        if active is None:
            obs, rew, done, trunc = self.venv.step_tensor(actions)
            m = None
        else:
            m = active_mask(active, self.num_envs, self.device)
            obs, rew, done, trunc = self.venv.step_tensor(actions, active=m)
        p_term = None
        if terminal_obs is not None:
            from .vec_env import INFO
            p_term = self._arg("terminal_obs", terminal_obs, (self.num_envs, self.obs_dim))
            _lib.check(self.lib.qs_get_info(self.venv.h, INFO["terminal_obs"], p_term))      # (on the stream venv.step_tensor has just set)
        self._stream()
        if m is None:
            _lib.check(self.lib.qs_norm_step(self.h, ptr(obs), ptr(rew), ptr(done), p_term, int(self.training), int(self.norm_obs),
                                             int(self.norm_reward), ptr(self.old_obs), ptr(self.old_reward)))
        else:
            _lib.check(self.lib.qs_norm_step_masked(self.h, ptr(obs), ptr(rew), ptr(done), ptr(m), p_term, int(self.training),
                                                    int(self.norm_obs), int(self.norm_reward), ptr(self.old_obs), ptr(self.old_reward)))
        return obs, rew, done, trunc

    def normalize_obs(self, obs):
        """normalize_obs on a host array with the current statistics (vec_normalize.py:_normalize_obs)."""
        if not self.norm_obs:
            return obs
        s = self.get_stats()
        return np.clip((obs - s["obs_mean"]) / np.sqrt(s["obs_var"] + self.epsilon), -self.clip_obs, self.clip_obs).astype(np.float32)

    def normalize_reward(self, reward):
        """normalize_reward on a host array with the current statistics (vec_normalize.py:normalize_reward)."""
        if not self.norm_reward:
            return reward
        s = self.get_stats()
        return np.clip(reward / np.sqrt(s["ret_var"] + self.epsilon), -self.clip_reward, self.clip_reward)

    def unnormalize_obs(self, obs):
        if not self.norm_obs:
            return obs
        s = self.get_stats()
        return obs * np.sqrt(s["obs_var"] + self.epsilon) + s["obs_mean"]

    def unnormalize_reward(self, reward):
        if not self.norm_reward:
            return reward
        return reward * np.sqrt(self.get_stats()["ret_var"] + self.epsilon)

    @property
    def obs_rms(self):
        """a snapshot of the running statistics under the names SB3 uses (RunningMeanStd.mean / .var / .count); set_stats writes them"""
        from types import SimpleNamespace
        s = self.get_stats()
        return SimpleNamespace(mean=s["obs_mean"], var=s["obs_var"], count=s["obs_count"])

    @property
    def ret_rms(self):
        from types import SimpleNamespace
        s = self.get_stats()
        return SimpleNamespace(mean=s["ret_mean"], var=s["ret_var"], count=s["ret_count"])

    def get_original_obs(self):
        return self.old_obs.cpu().numpy().copy()

    def get_original_reward(self):
        return self.old_reward.cpu().numpy().copy()

    # ---- SB3 VecEnv surface (numpy): load_model.py:109-137 -- env = VecNormalize.load(stats, env); env.step(numpy actions)
    def reset(self):
        return self.reset_tensor().cpu().numpy().copy()

    def step_async(self, actions):
        """The wrapped environment's host path with this normalisation attached (qs_host_set_norm): the step writes its result block on the
        device, VecNormalize.step_wait's work runs on it in place (one more launch), ONE copy brings observations, rewards, flags and the
        step's terminal observations -- normalised -- to page-locked host memory."""
        v = self.venv
        v._stream()
        _lib.check(self.lib.qs_host_set_norm(v.h, self.h, int(self.training), int(self.norm_obs), int(self.norm_reward), ptr(self.old_obs),
                                             ptr(self.old_reward)))
        v._terminal_hook = self.normalize_obs      # (only used when more episodes end in one step than the compact list holds)
        try:
            v.step_async(actions)
        except Exception:
            self._detach()
            raise

    def step_wait(self):
        """-> (obs, rewards, dones, infos) as VecNormalize.step_wait returns them: normalised observations / rewards, and
        infos[i]["terminal_observation"] normalised with the statistics of this step (vec_normalize.py step_wait)."""
        try:
            return self.venv.step_wait()
        finally:
            self._detach()

    def _detach(self):
        v = self.venv
        v._terminal_hook = None
        if v.h:
            self.lib.qs_host_set_norm(v.h, None, 0, 0, 0, None, None)

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    # ---- statistics
    def get_stats(self):
        o = self.obs_dim
        mean, var = np.zeros(o), np.zeros(o)
        oc, rm, rv, rc = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        _lib.check(self.lib.qs_norm_get_stats(self.h, mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), C.byref(oc), C.byref(rm),
                                              C.byref(rv), C.byref(rc)))
        return dict(obs_mean=mean, obs_var=var, obs_count=oc.value, ret_mean=rm.value, ret_var=rv.value, ret_count=rc.value)

    def set_stats(self, obs_mean, obs_var, obs_count, ret_mean=0.0, ret_var=1.0, ret_count=1e-4):
        m, v = np.ascontiguousarray(obs_mean, np.float64), np.ascontiguousarray(obs_var, np.float64)
        assert m.shape == (self.obs_dim,) and v.shape == (self.obs_dim,)
        _lib.check(self.lib.qs_norm_set_stats(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), float(obs_count), float(ret_mean),
                                              float(ret_var), float(ret_count)))

    # ---- snapshots and forks (QuadrupedVecEnv.snapshot / restore / fork)
    def _returns(self):
        r = self.torch.empty(self.num_envs, dtype=self.torch.float64, device=self.device)
        self._stream()
        _lib.check(self.lib.qs_norm_get_returns(self.h, ptr(r)))
        return r

    def _set_returns(self, r):
        r = self.torch.as_tensor(r, dtype=self.torch.float64).to(self.device).contiguous()
        if tuple(r.shape) != (self.num_envs,):
            raise ValueError(f"returns must have shape {(self.num_envs,)}, got {tuple(r.shape)}")
        self._stream()
        _lib.check(self.lib.qs_norm_set_returns(self.h, ptr(r)))
        self._returns_keep = r

    def snapshot(self, indices=None, out=None):
        """The wrapped environment's snapshot with this wrapper's state in extras["vec_normalize"]: the float64 statistics, the
        per-environment discounted returns, old_obs / old_reward.  The statistics belong to all environments: they are saved and restored
        whole whatever `indices` says.  Reading the statistics waits for the stream (qs_norm_get_stats)."""
        snap = self.venv.snapshot(indices, out)
        snap.extras["vec_normalize"] = dict(stats={k: np.asarray(v, np.float64) for k, v in self.get_stats().items()}, returns=self._returns(),
                                            old_obs=self.old_obs.clone(), old_reward=self.old_reward.clone())
        return snap

    def restore(self, snap, indices=None, strict=True):
        """-> the observation as the step before the snapshot returned it (normalised with the restored statistics)"""
        t = self.torch
        x = snap.extras.get("vec_normalize")
        if x is None:
            raise ValueError("the snapshot carries no vec_normalize state: it was taken below this wrapper (restore it there: env.venv.restore)")
        obs = self.venv.restore(snap, indices, strict)
        st = {k: np.asarray(v, np.float64) for k, v in x["stats"].items()}
        self._stream()
        self.set_stats(st["obs_mean"], st["obs_var"], float(st["obs_count"]), float(st["ret_mean"]), float(st["ret_var"]), float(st["ret_count"]))
        ret = t.as_tensor(x["returns"], dtype=t.float64).to(self.device)
        old_obs = t.as_tensor(x["old_obs"], dtype=t.float32).to(self.device)
        old_rew = t.as_tensor(x["old_reward"], dtype=t.float32).to(self.device)
        if indices is None:
            self._set_returns(ret)
            self.old_obs.copy_(old_obs); self.old_reward.copy_(old_rew)
        else:
            m = env_mask(indices, self.num_envs, self.device).bool()
            self._set_returns(t.where(m, ret, self._returns()))
            self.old_obs.copy_(t.where(m[:, None], old_obs, self.old_obs)); self.old_reward.copy_(t.where(m, old_rew, self.old_reward))
        if self.norm_obs:   # the handle keeps raw observations: normalise the returned buffer as a step does, without touching the statistics
            s = self.get_stats()
            mean = t.as_tensor(s["obs_mean"], dtype=t.float64, device=self.device)
            inv = 1.0 / t.sqrt(t.as_tensor(s["obs_var"], dtype=t.float64, device=self.device) + self.epsilon)
            obs.copy_(((obs.double() - mean) * inv).clamp(-self.clip_obs, self.clip_obs).float())
        return obs

    def fork(self, src=None, dst=None, src_of=None):
        """QuadrupedVecEnv.fork; the forked environments take their sources' discounted returns and old_obs / old_reward as well"""
        t = self.torch
        so = self.venv.fork(src, dst, src_of).to(t.int64)
        me = t.arange(self.num_envs, device=self.device)
        take = t.where((so >= 0) & (so < self.num_envs), so, me)
        self._set_returns(self._returns()[take])
        self.old_obs.copy_(self.old_obs[take]); self.old_reward.copy_(self.old_reward[take])
        return so

    def save(self, path):
        np.savez(path, clip_obs=self.clip_obs, clip_reward=self.clip_reward, gamma=self.gamma, epsilon=self.epsilon, norm_obs=self.norm_obs,
                 norm_reward=self.norm_reward, **self.get_stats())

    @classmethod
    def load(cls, path, venv):
        """`path`: an .npz written by save(), or an SB3 VecNormalize pickle (needs stable_baselines3 importable)."""
        if str(path).endswith(".npz"):
            z = np.load(path)
            self = cls(venv, clip_obs=float(z["clip_obs"]), clip_reward=float(z["clip_reward"]), gamma=float(z["gamma"]), epsilon=float(z["epsilon"]),
                       norm_obs=bool(z["norm_obs"]), norm_reward=bool(z["norm_reward"]))
            self.set_stats(z["obs_mean"], z["obs_var"], float(z["obs_count"]), float(z["ret_mean"]), float(z["ret_var"]), float(z["ret_count"]))
            return self
        import pickle
        with open(path, "rb") as f:
            sb3 = pickle.load(f)
        self = cls(venv, clip_obs=sb3.clip_obs, clip_reward=sb3.clip_reward, gamma=sb3.gamma, epsilon=sb3.epsilon, norm_obs=sb3.norm_obs,
                   norm_reward=sb3.norm_reward)
        self.set_stats(sb3.obs_rms.mean, sb3.obs_rms.var, sb3.obs_rms.count, sb3.ret_rms.mean, sb3.ret_rms.var, sb3.ret_rms.count)
        return self

    def _free(self):
        """the statistics' handle alone, which is all __del__ frees: the wrapped environment may outlive its wrapper"""
        if vars(self).get("h"):
            self._detach()          # (the environment's host path must not keep a pointer to the statistics that go away now)
        DeviceHandle.close(self)

    def close(self):
        self._free()
        self.venv.close()

    def __getattr__(self, name):   # everything else is the wrapped environment's
        return getattr(self.venv, name)
