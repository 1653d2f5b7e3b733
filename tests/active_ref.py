"""Test infrastructure: what DeviceVecNormalize.step_tensor(active=) computes, restated in float64 numpy on top of oracle/vecnorm.py (read
only).  RunningMeanStd.update sees the active rows only, only their returns advance and are cleared at done, a step without an active
row updates nothing, and every row is normalised with the step's statistics."""
import numpy as np

from oracle.vecnorm import VecNormalizeRef


class MaskedVecNormalizeRef(VecNormalizeRef):
    def __init__(self, n_envs, obs_dim, **kw):
        kw.setdefault("moments_dtype", np.float64)
        super().__init__(n_envs, obs_dim, **kw)

    def step(self, obs, rewards, dones, term_obs=None, active=None):
        if active is None:
            return super().step(obs, rewards, dones, term_obs)
        on = np.asarray(active).astype(bool)
        if self.training and self.norm_obs and on.any():
            self.obs_rms.update(obs[on])
        obs = self.normalize_obs(obs)
        if self.training:
            self.returns[on] = self.returns[on] * self.gamma + rewards[on]
            if on.any():
                self.ret_rms.update(self.returns[on])
        rewards = self.normalize_reward(rewards)
        if term_obs is not None:
            term_obs = self.normalize_obs(term_obs)
        self.returns[np.asarray(dones).astype(bool) & on] = 0
        return obs, rewards, term_obs

    def stats(self):
        return dict(obs_mean=self.obs_rms.mean, obs_var=self.obs_rms.var, obs_count=self.obs_rms.count, ret_mean=self.ret_rms.mean,
                    ret_var=self.ret_rms.var, ret_count=self.ret_rms.count)
