"""Test infrastructure, no GPU: what csrc/qs_norm.hip computes at every entry point (reset, step, masked step; the norm_obs / norm_reward /
training flags; terminal observations; raw copies), restated in float64 numpy on top of oracle/vecnorm.py and tests/active_ref.py (both read
only), and the case table of tests/test_gpu_norm_shapes.py and tests/test_norm_ref_cpu.py: shapes, data with a seed per case, mask sequences.

A case is one reset, six training steps and two evaluation steps on fabricated arrays.  Between the reset and the first step both sides are
given SETTLED statistics (qs_norm_set_stats): each column's nominal mean and variance with a count of n.  RunningMeanStd starts from mean 0,
variance 1, count 1e-4, and a first batch at mean 1000 leaves 1e6 * 1e-4 / n in the running variance for good (0.2 at n = 513, against the
column's own 1e-4): an error of the batch variance would be diluted below every bound.  The reset itself is compared on the prior.

The tolerances are the figures of test_gpu_parity.py::test_vec_normalize_kernels_against_torch_float64; a mean is judged in units of its
column's spread (|d mean| <= 1e-10 |mean| + 1e-9 sqrt(var)).  The per-environment returns are float64 on both sides (returns * gamma + reward,
fused on the device or not: one rounding) and are held to the figure of the returns' moments."""
import numpy as np

from active_ref import MaskedVecNormalizeRef

GAMMA, EPS, CLIP_OBS, CLIP_REW = 0.99, 1e-8, 5.0, 10.0
OUT_TOL = 2e-6                      # outputs: atol = rtol
VAR_RTOL = 1e-9                     # variances
MOM_RTOL, MOM_ATOL = 1e-9, 1e-10    # counts, the returns' moments, the per-environment returns
MEAN_REL, MEAN_STD = 1e-10, 1e-9    # |d mean| <= MEAN_REL |mean| + MEAN_STD sqrt(var)
QN_MAX_PARTS = 512
TRAIN_STEPS, EVAL_STEPS = 6, 2

WIDTHS = [(200, o) for o in (1, 31, 32, 33, 63, 64, 65, 255)]       # C = o + 1 on both sides of every 32-column chunk edge; four blocks, the last of 8 rows
SIZES = [(n, 33) for n in (1, 7, 9, 64, 65, 513, 4097, 32769)]
COMBINED = [(4097, 255)]
SHAPES = WIDTHS + SIZES + COMBINED
OFFSET_REWARDS = (200, 32)          # the case whose rewards are N(1000, 0.01): the returns column, alone in its chunk, carries the offset
FLAG_SHAPES = [(200, 33), (513, 32)]
FLAGS = [(t, o, r) for t in (1, 0) for o in (1, 0) for r in (1, 0)]  # (training, norm_obs, norm_reward)
MASK_SHAPES = [(513, 33), (4097, 65)]
MASKS = ("rows_0_100_off", "middle_block_and_first_rows_off", "only_last_row", "none", "random_60", "ones")   # one per training step, in this order
PLANTED = 1e3                       # what the uncounted first rows of every block hold in the N(0, 1) columns under the second mask

KINDS = 6
#        N(0, 1)     N(1000, 0.01)  constant 0.3                     N(0, 1e4)   0/1 flag, 1 %    N(-5, 30), two rows at +-8 sigma
NOMINAL = [(0.0, 1.0), (1000.0, 1e-4), (float(np.float32(0.3)), 0.0), (0.0, 1e8), (0.01, 0.0099), (-5.0, 900.0)]


def layout(n):
    """(rows_per_block, n_parts) of a handle of n environments: the formula of qs_norm_create"""
    rows = ((n + QN_MAX_PARTS - 1) // QN_MAX_PARTS + 7) // 8 * 8
    rows = max(rows, 64)
    return rows, (n + rows - 1) // rows


def seed_of(n, o, tag=0):
    return [n, o, tag]


def columns(rng, n, o):
    """float32 [n, o]: column c is of kind c % 6.  Kind 5 would leave +-5 standard deviations about once in 2e6 values; with two rows or
    more, one row holds the mean + 8 and one the mean - 8 standard deviations, so that both edges of clip_obs = 5 are hit in every step."""
    x = np.empty((n, o), np.float64)
    for c in range(o):
        k = c % KINDS
        if k == 0:
            x[:, c] = rng.normal(0.0, 1.0, n)
        elif k == 1:
            x[:, c] = rng.normal(1000.0, 0.01, n)
        elif k == 2:
            x[:, c] = 0.3
        elif k == 3:
            x[:, c] = rng.normal(0.0, 1e4, n)
        elif k == 4:
            x[:, c] = rng.random(n) < 0.01
        else:
            x[:, c] = rng.normal(-5.0, 30.0, n)
            if n >= 2:
                hi, lo = rng.choice(n, 2, replace=False)
                x[hi, c], x[lo, c] = -5.0 + 240.0, -5.0 - 240.0
    return x.astype(np.float32)


def settled(o, offset_rewards=False):
    """-> (obs_mean, obs_var, ret_mean, ret_var): the statistics a long run would have reached, column by column; the counts are n"""
    mean = np.array([NOMINAL[c % KINDS][0] for c in range(o)], np.float64)
    var = np.array([NOMINAL[c % KINDS][1] for c in range(o)], np.float64)
    return (mean, var, 1000.0, 1e-4) if offset_rewards else (mean, var, 1.0, 9.0)


def masks(n, rng):
    """the six masks of a masked case, uint8 [n], in the order of MASKS"""
    rows, parts = layout(n)
    first = np.arange(0, n, rows)
    a = np.ones(n, np.uint8); a[:100] = 0
    b = np.ones(n, np.uint8); mid = parts // 2; b[mid * rows:(mid + 1) * rows] = 0; b[first] = 0
    c = np.zeros(n, np.uint8); c[n - 1] = 1
    d = np.zeros(n, np.uint8)
    e = (rng.random(n) < 0.6).astype(np.uint8)
    f = np.ones(n, np.uint8)
    return [a, b, c, d, e, f]


def initial_returns(n, o):
    """float64 [n]: the per-environment returns both sides are given after the reset (qs_norm_set_returns), so that the first step already
    advances returns that differ; zeros in the case of OFFSET_REWARDS, whose first batch of returns is then N(1000, 0.01) itself"""
    if (n, o) == OFFSET_REWARDS:
        return np.zeros(n)
    return np.random.default_rng(seed_of(n, o, 98)).normal(0.0, 2.0, n)


def reset_obs(n, o):
    return columns(np.random.default_rng(seed_of(n, o, 99)), n, o)


def sequence(n, o, masked=False):
    """the eight steps of case (n, o): dicts of obs, term [n, o] float32, rew [n] float32, done [n] uint8, active (uint8 [n] or None),
    training.  Dones: 2 % of the rows; all in step 2, none in step 4.  masked: MASKS, one per training step; the first uncounted row of
    every step has its done flag set (a return that must not clear), and under the second mask the uncounted first rows of the blocks
    hold PLANTED in the N(0, 1) columns: the kernel's pivot is the block's first row whatever its flag."""
    act = masks(n, np.random.default_rng(seed_of(n, o, 77))) if masked else [None] * TRAIN_STEPS
    out = []
    for k in range(TRAIN_STEPS + EVAL_STEPS):
        rng = np.random.default_rng(seed_of(n, o, k))
        obs, term = columns(rng, n, o), columns(rng, n, o)
        rew = (rng.normal(1000.0, 0.01, n) if (n, o) == OFFSET_REWARDS else rng.normal(1.0, 3.0, n)).astype(np.float32)
        done = (rng.random(n) < 0.02).astype(np.uint8)
        if k == 2:
            done[:] = 1
        if k == 4:
            done[:] = 0
        active = act[k] if k < TRAIN_STEPS else None
        if active is not None:
            off = np.nonzero(active == 0)[0]
            if len(off) and k != 4:
                done[off[0]] = 1
            if MASKS[k] == "middle_block_and_first_rows_off":
                obs[np.arange(0, n, layout(n)[0])[:, None], np.arange(0, o, KINDS)[None, :]] = PLANTED
        out.append(dict(obs=obs, term=term, rew=rew, done=done, active=active, training=int(k < TRAIN_STEPS)))
    return out


def exact_moments(x):
    """(mean, variance) over axis 0 in np.longdouble: what the float64 reference itself is judged against, nothing else"""
    x = np.asarray(x, np.longdouble)
    mean = x.sum(0) / x.shape[0]
    return mean, np.square(x - mean).sum(0) / x.shape[0]


class NormRef(MaskedVecNormalizeRef):
    """One handle of qs_norm.hip in float64: the flags are given per call, as the C ABI takes them.  `batch` holds the arrays the last
    training step took its moments from (the counted rows of the observations, their advanced returns)."""

    def __init__(self, n, o, norm_obs=1, norm_reward=1):
        super().__init__(n, o, training=True, norm_obs=bool(norm_obs), norm_reward=bool(norm_reward), clip_obs=CLIP_OBS, clip_reward=CLIP_REW, gamma=GAMMA,
                         epsilon=EPS)
        self.batch = {}

    def set_stats(self, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count):
        self.obs_rms.mean, self.obs_rms.var, self.obs_rms.count = np.array(obs_mean, np.float64), np.array(obs_var, np.float64), float(obs_count)
        self.ret_rms.mean, self.ret_rms.var, self.ret_rms.count = float(ret_mean), float(ret_var), float(ret_count)

    def reset_arrays(self, obs, training):
        self.training = bool(training)
        return self.reset(obs)

    def step_arrays(self, obs, rew, done, term, active=None, training=1):
        """-> dict(obs, rew, term, raw_obs, raw_rew) as the device leaves them (float32)"""
        self.training = bool(training)
        rew64 = rew.astype(np.float64)
        if self.training:     # (the returns as the moments see them: step() clears them at done before it comes back)
            on = slice(None) if active is None else np.asarray(active).astype(bool)
            self.batch = dict(obs=obs[on] if self.norm_obs else None, returns=self.returns[on] * self.gamma + rew64[on])
        o, r, t = self.step(obs, rew64, done, term, active=active)
        return dict(obs=o, rew=np.asarray(r, np.float32), term=t, raw_obs=obs.copy(), raw_rew=rew.copy())


def run_reference(n, o, flags=(1, 1, 1), masked=False, on_step=None):
    """The whole case on the reference.  on_step(k, ref, step, expected) after the reset (k = -1, step = dict(obs=...)) and after every step."""
    training, norm_obs, norm_reward = flags
    ref = NormRef(n, o, norm_obs, norm_reward)
    obs0 = reset_obs(n, o)
    exp = dict(obs=ref.reset_arrays(obs0, training))
    if on_step:
        on_step(-1, ref, dict(obs=obs0), exp)
    mean, var, rm, rv = settled(o, (n, o) == OFFSET_REWARDS)
    ref.set_stats(mean, var, float(n), rm, rv, float(n))
    ref.returns = initial_returns(n, o)
    for k, s in enumerate(sequence(n, o, masked)):
        exp = ref.step_arrays(s["obs"], s["rew"], s["done"], s["term"], s["active"], s["training"] and training)
        if on_step:
            on_step(k, ref, s, exp)
    return ref
