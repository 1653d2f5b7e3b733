"""QuadrupedVecEnv: N Go1 environments advanced by one HIP kernel launch per step.

Duck-types stable_baselines3.common.vec_env.VecEnv as the reference's consumer uses it (load_model.py:109-137:
num_envs, observation_space, action_space, reset, step_async/step_wait/step, auto-reset with
infos[i]["terminal_observation"] and infos[i]["TimeLimit.truncated"], get_attr/set_attr/env_method/env_is_wrapped, seed).
State lives on the GPU; `step_tensor` keeps actions / observations there for on-device learners."""
import ctypes as C

import numpy as np

from . import lib as _lib
from .config import DEMO_FILES, OBSERVATION_EPS, build_config
from .handle import DeviceHandle, active_mask, env_mask, ptr, to_device_nowait   # (active_mask: also imported from here by its users)
from .render import DEFAULT_SIZE, as_camera, check_request, rgb_view, tile_images
from .spaces import Box, SB3VecEnv

INFO = dict(foot_force=0, foot_contact=1, torque=2, spring_torque=3, task=4, n_invalid=5, params=6, counters=7,
            last_action=8, terminal_obs=9, wrapper=10, filtered_action=11, reward_end=12, payload_block=13, external_wrench=14, rack=15)
PHASE = ("policy", "take_off", "landing", "rest")
PARAM = dict(mu=0, spring_k=1, spring_b=2, kp=3, kd=4, all=5)
FRAME = dict(link=1, world=2)   # QS_FRAME_LINK / QS_FRAME_WORLD = pybullet.LINK_FRAME / WORLD_FRAME


class QuadrupedVecEnv(DeviceHandle, SB3VecEnv):
    _prefix, _owner = "qs", "environment"

    def __init__(self, num_envs=1, device=0, auto_reset=True, reset_lookahead=None, copy_outputs=True, solo_waves=None, solo_reach=None, **env_kwargs):
        """reset_lookahead = K: every environment keeps the settled reset states of its next K episodes ready (computed by extra workgroups
        of the step kernel while the environments step), so a reset is a copy; results are bitwise those of K = 0, where every reset runs
        the reference's 2500-substep settle in place (gym_env.py:278-297, 323-329).  Default: 16 with auto_reset, 0 without.  What K = 16
        costs: N x 16 x 1152 bytes of slots plus five staging slices of min(2 N, 131072) records (151 + 94 MB at N = 8192, 1.2 + 0.75 GB at
        N = 65536) and N x 16 settles inside the constructor (0.1 s at N = 8192, 0.8 s at 65536); every launch also carries the settle
        lanes' workgroups of five full cohorts, of which those beyond the cohort's jobs leave at once (5120 of them at N = 8192: 0.4 % of the
        launch; 40960 next to 4096 working ones at N = 65536: under 1 %).  A handle whose episodes never end early can do with K = 2.
        copy_outputs=False: step() / step_wait() return views of the page-locked result block instead of copies (valid until the end of
        the next step: two blocks alternate).
        solo_waves = F / solo_reach = metres: see solo_waves() (None: the library's defaults)."""
        cfg, meta = build_config(n_envs=num_envs, auto_reset=auto_reset, **env_kwargs)
        cfg.reset_lookahead = int((16 if auto_reset else 0) if reset_lookahead is None else reset_lookahead)
        self._setup(cfg, meta, device, copy_outputs)
        if solo_waves is not None or solo_reach is not None:
            self.solo_waves(solo_waves, solo_reach)

    @classmethod
    def from_config(cls, cfg, meta, device=0, copy_outputs=True, load_demo=True):
        """A handle for a qs_config built (and possibly edited) by the caller: build_config(...) -> (cfg, meta).  load_demo=False leaves
        the demonstration of a DEMO task to a later set_demo()."""
        self = cls.__new__(cls)
        self._setup(cfg, meta, device, copy_outputs, load_demo)
        return self

    def _setup(self, cfg, meta, device, copy_outputs, load_demo=True):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("QuadrupedVecEnv needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.torch = torch
        self.lib = _lib.load()
        self.cfg, self.meta = cfg, meta
        self.num_envs = int(cfg.n_envs)
        self.device = torch.device("cuda", device)
        lay = self.meta["layout"]
        self.observation_space = Box(lay["low"] - OBSERVATION_EPS, lay["high"] + OBSERVATION_EPS, dtype=np.float32)  # gym_env.py:160-164
        d = self.cfg.action_dim
        self.action_space = Box(-np.ones(d), np.ones(d), dtype=np.float32)                                       # gym_env.py:179-182
        self.action_dim, self.obs_dim = d, self.cfg.obs_dim
        self._init_vec_env_base()
        self.h = C.c_void_p()
        self._create(device)
        n, o = self.num_envs, self.obs_dim
        with torch.cuda.device(self.device):
            self._obs = torch.zeros((n, o), dtype=torch.float32, device=self.device)
            self._rew = torch.zeros(n, dtype=torch.float32, device=self.device)
            self._done = torch.zeros(n, dtype=torch.uint8, device=self.device)
            self._trunc = torch.zeros(n, dtype=torch.uint8, device=self.device)
            self._act = torch.zeros((n, d), dtype=torch.float32, device=self.device)
        self._views, self._infos, self._dirty = {}, [{} for _ in range(self.num_envs)], []
        self._terminal_hook = None     # DeviceVecNormalize.step_async: normalises the per-environment terminal observations (overflow of the compact list)
        self.copy_outputs = bool(copy_outputs)
        self._trace = None
        self._push_keep = None        # the inputs of the last apply_external_force, alive until its kernel has read them
        self._active_keep = None      # the mask of the last step_tensor(active=), likewise
        self.render_mode = None
        self.render_indices = None        # environments get_images / render draw (None = all, as SB3 renders every sub-environment)
        self.render_size = DEFAULT_SIZE   # (width, height)
        self.camera_mode = "CLASSIC"      # qs_amd.render.CAMERA_MODES, or a render.Camera
        self._render_all = None           # device int32 [0, N) for render_indices = None
        self._render_keep = None          # the ids of the last render, alive until its kernel has read them
        self.demo_list, self.demo_length = None, 0
        if load_demo and self.meta["task_env"] in DEMO_FILES:
            if self.meta["demo"] is None:
                self.close()
                raise ValueError(f"task {self.meta['task_env']} imitates a demonstration: pass demo=<array [L, action_dim + 38] or path of the "
                                 f".npy> (the reference loads demonstrations/{DEMO_FILES[self.meta['task_env']]}, task_base.py:173)")
            self.set_demo(self.meta["demo"])

    def _create(self, device):
        """the device handle, with the rack of meta["rack"] when on_rack=True (qs_create_ex)"""
        rk = self.meta.get("rack")
        self.on_rack = bool(rk and rk["on"])
        if self.on_rack:
            r = _lib.QsRack()
            r.on = 1
            for i in range(3):
                r.anchor_pos[i] = float(rk["pos"][i])
            for i in range(4):
                r.anchor_quat[i] = float(rk["quat"][i])
            _lib.check(self.lib.qs_create_ex(C.byref(self.cfg), C.byref(r), device, C.byref(self.h)))
        else:
            _lib.check(self.lib.qs_create(C.byref(self.cfg), device, C.byref(self.h)))

    def set_rack(self, hung, indices=None):
        """Release (hung=False) or hang again (hung=True) the robots of `indices` (None = all) for the rest of their current episode: a
        reset hangs every robot again (on_rack=True handles only).  Never waits for the device."""
        if not self.on_rack:
            raise RuntimeError("set_rack needs a handle created with on_rack=True")
        mask = env_mask(indices, self.num_envs, self.device)
        if mask is not None:
            self._rack_keep = mask
        self._stream()
        _lib.check(self.lib.qs_set_rack(self.h, ptr(mask), 1 if hung else 0))

    def _init_vec_env_base(self):
        """stable_baselines3.common.vec_env.VecEnv.__init__(num_envs, observation_space, action_space) when SB3 is importable and this
        class therefore IS a VecEnv (qs_amd/spaces.py): SB3's wrappers (VecNormalize.load(stats, env), load_model.py:120) read what the base
        class sets up, and isinstance(env, VecEnv) holds.  Without SB3 the base is `object` and there is nothing to call."""
        if SB3VecEnv is not object:
            SB3VecEnv.__init__(self, self.num_envs, self.observation_space, self.action_space)

    # ---- device-resident API
    def reset_tensor(self, mask=None, states=None):
        """reset() of the masked environments (all when mask is None).  With `states` ([N,37], layout of get_state) the robots are
        placed there instead of being spawned and settled: reference-state initialisation (set_robot_desired_state)."""
        self._stream()
        m = None
        if mask is not None:
            m = self.torch.as_tensor(mask, device=self.device).to(self.torch.uint8).contiguous()
        if states is not None:
            st = self.torch.as_tensor(states, dtype=self.torch.float32, device=self.device).reshape(self.num_envs, 37).contiguous()
            _lib.check(self.lib.qs_reset_to(self.h, ptr(m), ptr(st)))
        else:
            _lib.check(self.lib.qs_reset(self.h, ptr(m)))
        _lib.check(self.lib.qs_get_obs(self.h, ptr(self._obs)))
        return self._obs

    def step_tensor(self, actions, active=None):
        """actions: float32 CUDA tensor [N, action_dim] -> (obs, rew, done, truncated) CUDA tensors (reused buffers).
        active: a bool or uint8 tensor [N] on the handle's device, None for none (qs_step_masked).  An environment with active[e] == 0 is
        frozen for this step: nobody steps it, nothing of it changes (record, pending push, look-ahead window, counters), no reset happens
        to it; its row of obs is its last observation, its reward 0, done and truncated 0.  The active ones get the bits they get without a
        mask.  A wave of 16 consecutive environments that are all frozen costs the launch next to nothing, and a frozen robot that lies on
        the floor keeps no wave-mate waiting.  Handles without a parked record (reset_lookahead=0, KEEP randomizer) are correct and no
        faster; payload="soft" handles refuse a mask."""
        a = actions
        if a.dtype != self.torch.float32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=self.torch.float32).contiguous()
        if a.shape != (self.num_envs, self.action_dim):
            raise ValueError(f"actions must have shape {(self.num_envs, self.action_dim)}, got {tuple(a.shape)}")
        m = None if active is None else active_mask(active, self.num_envs, self.device)
        self._stream()
        if m is None:
            _lib.check(self.lib.qs_step(self.h, ptr(a), ptr(self._obs), ptr(self._rew), ptr(self._done), ptr(self._trunc)))
        else:
            _lib.check(self.lib.qs_step_masked(self.h, ptr(a), ptr(m), ptr(self._obs), ptr(self._rew), ptr(self._done), ptr(self._trunc)))
        self._active_keep = m
        return self._obs, self._rew, self._done, self._trunc

    def step_fused(self, actions, out):
        """One step with a single output: `out` [N, obs_dim + 2] float32 CUDA tensor = observation | reward | done + 2 * truncated
        (the row a sharded run all-gathers, qs_amd/sharded.py)."""
        pa, po = self._arg("actions", actions, (self.num_envs, self.action_dim)), self._arg("out", out, (self.num_envs, self.obs_dim + 2))
        self._stream()
        _lib.check(self.lib.qs_step_fused(self.h, pa, po))
        return out

    def get_state(self):
        out = self.torch.empty((self.num_envs, 37), dtype=self.torch.float32, device=self.device)
        self._stream()
        _lib.check(self.lib.qs_get_state(self.h, ptr(out)))
        return out

    def set_state(self, state):
        s = self.torch.as_tensor(state, dtype=self.torch.float32, device=self.device).contiguous().reshape(self.num_envs, 37)
        self._stream()
        _lib.check(self.lib.qs_set_state(self.h, ptr(s)))

    def get_info(self, which):
        k = INFO[which] if isinstance(which, str) else int(which)
        dim = self.lib.qs_info_dim(self.h, k)
        out = self.torch.empty((self.num_envs, dim), dtype=self.torch.float32, device=self.device)
        self._stream()
        _lib.check(self.lib.qs_get_info(self.h, k, ptr(out)))
        return out

    def set_params(self, which, values):
        k = PARAM[which] if isinstance(which, str) else int(which)
        v = self.torch.as_tensor(values, dtype=self.torch.float32, device=self.device).contiguous()
        self._stream()
        _lib.check(self.lib.qs_set_params(self.h, k, ptr(v)))
        self.torch.cuda.current_stream(self.device).synchronize()  # `v` may be a temporary

    def apply_external_force(self, force, torque=None, substeps=None, frame="world", indices=None):
        """Push the trunks (Quadruped.apply_external_force, quadruped.py:338-343, batched): force [N,3] or [3] (N), torque likewise (N m,
        default 0), acting at each trunk's centre of mass on the next `substeps` physics substeps of the environment (None = one env
        step, action_repeat substeps; an int or [N] ints; 0 cancels), counted on the device across env steps.  frame "world": the vectors
        stay fixed in the world frame; "link": they are fixed to the trunk and turn with it.  indices: the environments pushed (None = all);
        the others keep what they had.  A new push replaces an environment's earlier one; a reset cancels it.
        Accepts numpy arrays, lists, host tensors or tensors on the device, and never waits for the device: host data is checked here and
        goes over through page-locked staging without blocking (so a learner may push every step); device tensors are checked by the
        kernel, and a refused row (negative duration, non-finite value) is reported by the next call that waits for the device anyway
        (stats() or counter() raise; include/qs_amd.h)."""
        t = self.torch
        if frame not in FRAME:
            raise ValueError(f"frame must be one of {sorted(FRAME)}, got {frame!r}")
        n = self.num_envs

        def rows(x, name):
            if isinstance(x, t.Tensor) and x.device == self.device:
                v = x.to(dtype=t.float32)
                if v.shape not in ((3,), (n, 3)):
                    raise ValueError(f"{name} must have shape (3,) or {(n, 3)}, got {tuple(v.shape)}")
            else:
                a = (x.detach().cpu().numpy() if isinstance(x, t.Tensor) else np.asarray(x)).astype(np.float32)
                if a.shape not in ((3,), (n, 3)):
                    raise ValueError(f"{name} must have shape (3,) or {(n, 3)}, got {tuple(a.shape)}")
                if not np.all(np.isfinite(a)):
                    raise ValueError(f"{name} must be finite")
                v = to_device_nowait(a, self.device)
            return v.expand(n, 3)

        self._stream()
        f = rows(force, "force")
        tq = t.zeros((n, 3), dtype=t.float32, device=self.device) if torque is None else rows(torque, "torque")
        w = t.cat([f, tq], dim=1).contiguous()
        k = self.cfg.action_repeat if substeps is None else substeps
        if isinstance(k, t.Tensor) and k.device == self.device:
            if k.dtype.is_floating_point or k.dtype == t.bool:
                raise ValueError(f"substeps must be an integer tensor, got {k.dtype}")
            k = k.to(dtype=t.int32)
            if k.shape not in ((), (n,)):
                raise ValueError(f"substeps must be a scalar or have shape {(n,)}, got {tuple(k.shape)}")
            k = k.expand(n)
        else:
            a = k.detach().cpu().numpy() if isinstance(k, t.Tensor) else np.asarray(k)
            if a.dtype.kind not in "iu" or np.any(a < 0):
                raise ValueError(f"substeps must be a non-negative integer (or [N] of them), got {k!r}")
            if a.shape not in ((), (n,)):
                raise ValueError(f"substeps must be a scalar or have shape {(n,)}, got {tuple(a.shape)}")
            if np.any(a > 2 ** 31 - 1):
                raise ValueError("substeps must fit an int32")
            k = t.full((n,), int(a), dtype=t.int32, device=self.device) if a.shape == () else to_device_nowait(a.astype(np.int32), self.device)
        k = k.contiguous()
        m = env_mask(indices, n, self.device)
        _lib.check(self.lib.qs_set_external_wrench(self.h, ptr(m), ptr(w), ptr(k), FRAME[frame]))
        # (everything here is ordered on the current stream; the references keep the device buffers from going back to the caching
        # allocator before the kernel has read them, the staging blocks are held by the host allocator until their copies are done)
        self._push_keep = (w, k, m)

    # ---- snapshots and forks (include/qs_amd.h qs_snapshot / qs_restore / qs_fork)
    def snapshot_info(self):
        """the qs_snapshot_info fields of this handle as a dict: the row's size, and the digests that say which snapshots fit it"""
        info = _lib.SnapshotInfo()
        _lib.check(self.lib.qs_snapshot_info(self.h, C.byref(info)))
        return info.as_dict()

    def snapshot(self, indices=None, out=None):
        """The environments `indices` (None = all) as an EnvSnapshot: one row per environment with everything a step reads (the record, the
        pending push, the last and the terminal observation).  One launch on the current stream; nothing is waited for.  out: an earlier
        snapshot of this handle whose tensor is written again -- only the rows of `indices` change -- so a control loop allocates nothing."""
        from .snapshot import EnvSnapshot, check_fits
        t = self.torch
        info = self.snapshot_info()
        if out is None:
            rows = t.zeros((info["n_envs"], info["row_floats"]), dtype=t.float32, device=self.device)
            snap = EnvSnapshot(rows, info)
        else:
            check_fits(out.info, info, strict=True)
            rows, snap = out.rows, out
        p_rows = self._arg("out.rows", rows, (info["n_envs"], info["row_floats"]))
        m = env_mask(indices, self.num_envs, self.device)
        self._stream()
        _lib.check(self.lib.qs_snapshot(self.h, ptr(m), p_rows))
        self._snap_keep = m
        return snap

    def restore(self, snap, indices=None, strict=True):
        """The environments `indices` (None = all) go back to `snap`; returns the observation tensor, as reset_tensor does.  strict=True
        demands a snapshot of the same configuration (equal config_digest): from there the handle continues bit for bit as the run the
        snapshot was taken from.  strict=False takes any snapshot of the same layout (equal layout_digest), e.g. of another seed: the robots
        continue under THIS handle's configuration.  Anything else raises ValueError naming the first differing field.  The `infos` entries
        of the restored environments are cleared (dicts handed out earlier are not changed under copy_outputs=True)."""
        from .snapshot import check_fits
        t = self.torch
        check_fits(snap.info, self.snapshot_info(), strict=strict)
        rows = snap.rows
        if tuple(rows.shape) != (snap.info["n_envs"], snap.info["row_floats"]) or rows.dtype != t.float32:
            raise ValueError(f"snapshot rows must be float32 of shape {(snap.info['n_envs'], snap.info['row_floats'])}, got {rows.dtype} {tuple(rows.shape)}")
        if rows.device != self.device or not rows.is_contiguous():
            rows = rows.contiguous().to(self.device)
        m = env_mask(indices, self.num_envs, self.device)
        self._stream()
        _lib.check(self.lib.qs_restore(self.h, ptr(m), ptr(rows)))
        _lib.check(self.lib.qs_get_obs(self.h, ptr(self._obs)))
        self._snap_keep = (m, rows)
        if not self._dirty:
            pass                                   # (every filled entry is listed there: a device-only loop never looks at its indices on the host)
        elif indices is None:
            self._forget_infos(None)
        elif isinstance(indices, t.Tensor) and indices.dtype in (t.bool, t.uint8):
            self._forget_infos(t.nonzero(indices).flatten().tolist())
        else:
            self._forget_infos(self._indices(indices.tolist() if isinstance(indices, (np.ndarray, t.Tensor)) else indices))
        return self._obs

    def _forget_infos(self, idx):
        """the infos entries of environments `idx` (None = all) say nothing any more"""
        idx = range(self.num_envs) if idx is None else idx
        for i in idx:
            if self._infos[i]:
                if self.copy_outputs:
                    self._infos[i] = {}
                else:
                    self._infos[i].clear()
        gone = set(idx)
        self._dirty = [i for i in self._dirty if i not in gone]

    def fork(self, src=None, dst=None, src_of=None):
        """Copy environments inside the handle, in one call (a gather launch and a scatter launch, every source read before any destination is
        written: chains and swaps are legal).  src: one index or [M]; dst: the indices that receive them -- one source broadcasts, M sources
        need M destinations; dst=None with one source means every other environment.  Or src_of: an int32 [N] tensor on the device, the
        source of every environment (-1 or its own index: left alone), which goes straight to the kernel.  A fork takes its source's whole
        record, push and observations but keeps its own episode number and total-step counter: its future randomizer draws, its noise
        stream and its look-ahead window stay its own.  Host indices are checked here and raise; a device src_of outside [-1, N) leaves
        that environment alone and makes the next stats() / counter() raise, naming it.  Returns the device int32 [N] sources used."""
        t = self.torch
        n = self.num_envs
        if src_of is not None:
            if src is not None or dst is not None:
                raise ValueError("give either src (and dst) or src_of")
            if not (isinstance(src_of, t.Tensor) and src_of.device == self.device):
                a = np.asarray(src_of)
                if a.dtype.kind not in "iu" or a.shape != (n,):
                    raise ValueError(f"src_of must be {n} integers, got {a.dtype} {a.shape}")
                if a.min() < -1 or a.max() >= n:
                    raise ValueError(f"sources must lie in [-1, {n}), got {a.min()} .. {a.max()}")
                so = to_device_nowait(a.astype(np.int32), self.device)
            else:
                if src_of.dtype.is_floating_point or src_of.dtype == t.bool or tuple(src_of.shape) != (n,):
                    raise ValueError(f"src_of must be an integer tensor of shape {(n,)}, got {src_of.dtype} {tuple(src_of.shape)}")
                so = src_of.to(t.int32).contiguous()
        else:
            if src is None:
                raise ValueError("fork needs src or src_of")
            s = np.atleast_1d(np.asarray(src.tolist() if isinstance(src, t.Tensor) else src))
            if s.dtype.kind not in "iu" or s.ndim != 1 or s.size == 0:
                raise ValueError(f"src must be an index or a list of indices, got {src!r}")
            if dst is None:
                if s.size != 1:
                    raise ValueError("dst=None needs exactly one source (it then goes to every other environment)")
                d = np.array([i for i in range(n) if i != int(s[0])], np.int64)
            else:
                d = np.atleast_1d(np.asarray(dst.tolist() if isinstance(dst, t.Tensor) else dst))
                if d.size and (d.dtype.kind not in "iu" or d.ndim != 1):
                    raise ValueError(f"dst must be a list of indices, got {dst!r}")
                d = d.astype(np.int64)
            if s.size != 1 and s.size != d.size:
                raise ValueError(f"{s.size} sources for {d.size} destinations: give one source, or one per destination")
            for name, a in (("src", s), ("dst", d)):
                if a.size and (a.min() < 0 or a.max() >= n):
                    raise ValueError(f"{name} must lie in [0, {n}), got {a.min()} .. {a.max()}")
            if np.unique(d).size != d.size:
                raise ValueError("dst names an environment twice")
            a = np.full(n, -1, np.int32)
            a[d] = s.astype(np.int32) if s.size > 1 else np.int32(s[0])
            so = to_device_nowait(a, self.device)
        self._stream()
        _lib.check(self.lib.qs_fork(self.h, ptr(so)))
        _lib.check(self.lib.qs_get_obs(self.h, ptr(self._obs)))
        self._fork_keep = so
        return so

    def stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.qs_stats(self.h, C.byref(a), C.byref(b)))
        return dict(settle_substeps=a.value, resets=b.value)

    COUNTERS = dict(settle_substeps=0, resets=1, lookahead_served=2, lookahead_settled=3, limit_path_substeps=4, self_narrow_substeps=5,
                    reset_stalls=6, lookahead_backlog=7, solo_path_substeps=8)

    def counter(self, which):
        v = C.c_uint64(0)
        _lib.check(self.lib.qs_counter(self.h, self.COUNTERS[which] if isinstance(which, str) else int(which), C.byref(v)))
        return int(v.value)

    def counters_snapshot(self):
        """The counters as they stand at this point of the stream, in a device tensor [8] (int64; index = COUNTERS, entry 7 unused) -- no
        synchronisation: read it (.cpu()) whenever convenient."""
        out = self.torch.zeros(8, dtype=self.torch.int64, device=self.device)
        self._stream()
        _lib.check(self.lib.qs_counters_async(self.h, ptr(out)))
        return out

    def solo_waves(self, f=None, reach=None):
        """Solo waves (qs_solo_waves): up to `f` robots per launch that are about to put a link on the floor -- one within `reach` metres of
        its contact range at the end of the previous step -- step in a workgroup of their own instead of holding up their fifteen
        wave-mates.  f = 0: off; None: keep (the library starts with 128, or QS_SOLO_WAVES).  Results do not change, only the launch time.
        counter("solo_path_substeps") / counter("limit_path_substeps") is the share of the many-rows wave-substeps they take."""
        if not hasattr(self.lib, "qs_solo_waves"):
            raise RuntimeError("this libqs_hip.so has no qs_solo_waves: rebuild it (python quadruped-springs_amd/build.py --force)")
        if f is None:   # keep the count: an unchanged F needs the current one, which only the library knows -- so reach alone goes through F = -1
            f = -1
        _lib.check(self.lib.qs_solo_waves(self.h, int(f), float(reach if reach is not None else 0.0)))

    def enable_timing(self, on=True):
        """True / False: arm / disarm the batch timing of the step kernel; 2: close the batch now (the closing event goes onto the stream,
        last_step_kernel_ms() waits for it whenever it is called)."""
        self._stream()
        _lib.check(self.lib.qs_enable_timing(self.h, int(on)))

    def last_step_kernel_ms(self):
        ms = C.c_float()
        _lib.check(self.lib.qs_last_step_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    TRACE_FIELDS = dict(time=(0, 1), base_position=(1, 4), base_quaternion=(4, 8), base_linear_velocity=(8, 11), base_angular_velocity=(11, 14),
                        joint_angles=(14, 26), joint_velocities=(26, 38), torques=(38, 50), spring_tau=(50, 62), feet_normal_forces=(62, 66),
                        feet_in_contact=(66, 70))

    def set_trace(self, env=0):
        """Per-substep tap on one environment (the reference's set_sub_step_callback users: evaluation_wrapper.py:14,
        monitor_state.py:66-85).  env=None switches it off.  Read the rows of the last step with get_trace()."""
        if env is None:
            self._trace = None
            _lib.check(self.lib.qs_set_trace(self.h, -1, None))
            return
        self._trace = self.torch.zeros((self.cfg.action_repeat, 70), dtype=self.torch.float32, device=self.device)
        _lib.check(self.lib.qs_set_trace(self.h, int(env), ptr(self._trace)))

    def get_trace(self, as_dict=True):
        """Rows [action_repeat, 70] of the traced environment for the most recent step; with as_dict the monitor_state.py
        quantities, incl. the spring energy 0.5 k (q - q_rest)^2 with the gated stiffness of springs.py:34-61."""
        rows = self._trace.cpu().numpy().astype(np.float64)
        if not as_dict:
            return rows
        out = {k: rows[:, a:b] for k, (a, b) in self.TRACE_FIELDS.items()}
        out["time"] = out["time"][:, 0]
        return out

    # ---- DEMO tasks (task_base.py:169-220)
    def set_demo(self, rows):
        """The demonstration the DEMO task imitates: [L, action_dim + 38] rows as demo_rows() / GetDemonstrationWrapper record them."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.action_dim + 38:
            raise ValueError(f"demonstration rows have {self.action_dim + 38} entries, got shape {rows.shape}")
        t = self.torch.from_numpy(rows).to(self.device)
        self._stream()
        _lib.check(self.lib.qs_set_demo(self.h, ptr(t), int(rows.shape[0])))   # synchronises: `t` may go
        self.demo_list, self.demo_length = rows, int(rows.shape[0])

    def set_demo_counter(self, values, mask=None):
        """task.set_demo_counter (task_base.py:219-220) of the masked environments; after reset_tensor(mask, states=...)."""
        t = self.torch
        v = t.as_tensor(values, device=self.device).to(t.int32).expand(self.num_envs).contiguous()
        m = None if mask is None else t.as_tensor(mask, device=self.device).to(t.uint8).contiguous()
        self._stream()
        _lib.check(self.lib.qs_set_demo_counter(self.h, ptr(m), ptr(v)))

    def demo_counter(self):
        return self.get_info("task")[:, 44].to(self.torch.int64)

    @staticmethod
    def demo_states(rows, action_dim):
        """[K, 37] rigid-body states (layout of get_state) of demonstration rows (read_demo order: a, q, qd, pos, quat, vlin, vang, flag)."""
        r = np.atleast_2d(np.asarray(rows, dtype=np.float32))
        d = action_dim
        return np.concatenate([r[:, d + 24:d + 37], r[:, d:d + 24]], axis=1)

    # ---- demonstration rows (get_demonstration_wrapper.py:35-70)
    def demo_rows(self, done=None):
        """[N, d + 38] on the device: the row GetDemonstrationWrapper._get_demo records after a step -- filtered action (d), joint
        angles 12, joint velocities 12, base position 3, quaternion 4, linear velocity 3, angular velocity 3, landing_started 1
        (latched once the controller has switched and vz <= 0; cleared when the episode ends).  Call it once per step with that
        step's `done` (tensor or array; default: the buffer step_tensor filled)."""
        t = self.torch
        st = self.get_state()
        if getattr(self, "_landing_started", None) is None:
            self._landing_started = t.zeros(self.num_envs, dtype=t.bool, device=self.device)
        switched = self.get_info("task")[:, 0] > 0.5
        self._landing_started |= switched & (st[:, 9] <= 0.0)
        act = (self.get_info("filtered_action") if self.cfg.enable_filter else self.get_info("last_action"))[:, : self.action_dim]
        rows = t.cat([act, st[:, 13:37], st[:, 0:13], self._landing_started.to(t.float32)[:, None]], dim=1)
        d = self._done.bool() if done is None else t.as_tensor(np.asarray(done) if not t.is_tensor(done) else done, device=self.device).bool()
        self._landing_started &= ~d
        return rows

    @staticmethod
    def read_demo(demo, action_dim=6, num_joints=12):
        """get_demonstration_wrapper.py:61-70: split one row into (action, q, qd, base_pos, base_quat, lin_vel, ang_vel, landing)."""
        cuts = np.cumsum([action_dim, num_joints, num_joints, 3, 4, 3, 3, 1])
        return [demo[a:b] for a, b in zip(np.concatenate(([0], cuts[:-1])), cuts)]

    def settle_lanes(self, on=True):
        """Switch the settle lanes of the look-ahead resets on / off (qs_settle_lanes; on from construction).  Off: resets use up the
        states that are ready, then settle in place."""
        self._stream()
        _lib.check(self.lib.qs_settle_lanes(self.h, int(bool(on))))

    # ---- SB3 VecEnv surface (numpy)
    def reset(self):
        return self.reset_tensor().cpu().numpy().copy()

    def step_async(self, actions):
        """VecEnv.step_async: the actions go to the device and the step and the copy of its results back are enqueued (qs_host_step_begin);
        nothing is waited for."""
        a = np.ascontiguousarray(actions, dtype=np.float32)
        if a.size != self.num_envs * self.action_dim:
            raise ValueError(f"actions must have shape {(self.num_envs, self.action_dim)}, got {a.shape}")
        self._stream()
        rc = self.lib.qs_host_step_begin(self.h, a.ctypes.data_as(C.c_void_p))
        if rc != 0:
            msg = self.lib.qs_last_error().decode()
            # a failure BEHIND the step's launch leaves the step pending (include/qs_amd.h): close it, so that the next step_async starts clean
            self.lib.qs_host_step_end(self.h, C.byref(_lib.HostResult()))
            raise RuntimeError("qs_amd: " + msg)

    def _host_views(self, res):
        """numpy views of the result block qs_host_step_end points at (one set per host block: two alternate)."""
        key = res.obs
        views = self._views.get(key)
        if views is None:
            n, o = self.num_envs, self.obs_dim
            f32, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
            views = (np.ctypeslib.as_array(C.cast(res.obs, f32), shape=(n, o)), np.ctypeslib.as_array(C.cast(res.rew, f32), shape=(n,)),
                     np.ctypeslib.as_array(C.cast(res.done, u8), shape=(n,)).view(np.bool_),
                     np.ctypeslib.as_array(C.cast(res.truncated, u8), shape=(n,)).view(np.bool_),
                     np.ctypeslib.as_array(C.cast(res.terminal_rows, f32), shape=(res.terminal_cap, o + 1)))
            self._views[key] = views
        return views

    def _entry(self, old, truncated, terminal_observation):
        """the info dict of an environment whose episode ended in this step: a new one under copy_outputs, the old one refilled otherwise"""
        if self.copy_outputs:
            return {"TimeLimit.truncated": truncated, "terminal_observation": terminal_observation}
        old["TimeLimit.truncated"] = truncated; old["terminal_observation"] = terminal_observation
        return old

    def step_wait(self):
        """VecEnv.step_wait: (obs [N, o] float32, rewards [N] float32, dones [N] bool, infos) -- the SB3 convention of load_model.py:113-133:
        finished environments are already reset, their last observation is infos[i]["terminal_observation"], infos[i]["TimeLimit.truncated"]
        says whether the time limit ended the episode (gym_env.py:246).  One H2D copy, the step, ONE D2H copy into page-locked host memory;
        the arrays returned are copies of it (copy_outputs=False: views, valid until the end of the NEXT step).  `infos` is ONE list
        of N dicts kept by the environment, of which a step touches only the entries of environments that have (or had) something to
        say.  With copy_outputs=True (the default) such an entry gets a NEW dict: a dict handed out by an earlier step is never changed,
        so a consumer may keep the ones it cares about (a replay buffer that stores terminal observations); the LIST is the same object
        every step -- copy it (list(infos)) to keep a whole step's worth.  copy_outputs=False reuses the dicts in place as well."""
        res = _lib.HostResult()
        _lib.check(self.lib.qs_host_step_end(self.h, C.byref(res)))
        obs, rew, done, trunc, term = self._host_views(res)
        if self.copy_outputs:
            obs, rew, done = obs.copy(), rew.copy(), done.copy()
        infos = self._infos
        if self.copy_outputs:
            for i in self._dirty:
                infos[i] = {}
        else:
            for i in self._dirty:
                infos[i].clear()
        dirty = self._dirty = []
        idx = np.flatnonzero(done)
        if idx.size:
            if not self.cfg.auto_reset:
                for i in idx.tolist():
                    infos[i] = self._entry(infos[i], bool(trunc[i]), obs[i].copy())
            else:
                rows = term[: idx.size] if idx.size <= term.shape[0] else None
                if rows is None:    # more episode ends than the compact list holds: the per-environment array
                    full = self.get_info("terminal_obs").cpu().numpy()
                    if self._terminal_hook is not None:      # DeviceVecNormalize: the per-environment array holds raw observations
                        full = self._terminal_hook(full)
                    for i in idx.tolist():
                        infos[i] = self._entry(infos[i], bool(trunc[i]), full[i])
                else:
                    rows = rows.copy()
                    envs = rows[:, 0].view(np.int32)
                    for k, i in enumerate(envs.tolist()):
                        infos[i] = self._entry(infos[i], bool(trunc[i]), rows[k, 1:])
            dirty.extend(idx.tolist())
        if self.cfg.wrapper_mode:
            # the reference's LandingWrapper / GoToRestWrapper loop over env.step inside one wrapper.step; here every inner
            # step is one launch and the ones whose action was scripted are flagged, so a learner can mask them out.  Only the
            # environments in a scripted phase get the keys (read them with infos[i].get("scripted", False)).
            w = self.get_info("wrapper").cpu().numpy()
            for i in np.nonzero((w[:, 0] > 0.5) | (w[:, 1] > 0.5))[0].tolist():
                if self.copy_outputs and not infos[i]:
                    infos[i] = {}            # (an empty dict may have been handed out by an earlier step: it stays empty)
                infos[i]["scripted"] = bool(w[i, 1])
                infos[i]["phase"] = PHASE[int(w[i, 0])]
                dirty.append(i)
        return obs, rew, done, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def seed(self, seed=None):
        """VecEnv.seed(seed) (SB3: each sub-environment gets seed + index; load_model.py's make_vec_env(seed=...) calls it right after the
        constructor).  Randomness here is counter based -- Philox streams keyed by (seed, global environment id, episode / step), which
        also key the reset states settled ahead of time -- so a new seed means a new device handle: the old one is destroyed and one
        with cfg.seed = seed created in its place.  EVERY ENVIRONMENT IS UNRESET AFTERWARDS, as after the constructor: call reset()
        next (what SB3's own flow does).  seed=None leaves everything as it is.  Returns SB3's list: seed + i for environment i (None s
        when nothing was changed)."""
        if seed is None:
            return [None] * self.num_envs
        seed = int(seed)
        if seed < 0:
            raise ValueError(f"seed must be a non-negative integer, got {seed}")
        self.close()
        self.cfg.seed = seed
        self._views, self._dirty = {}, []
        self._infos = [{} for _ in range(self.num_envs)]
        self._create(self.device.index or 0)
        if self.demo_list is not None:
            self.set_demo(self.demo_list)
        self._trace = None
        return [seed + i for i in range(self.num_envs)]

    def get_attr(self, attr_name, indices=None):
        return [getattr(self, attr_name)] * len(self._indices(indices))

    def set_attr(self, attr_name, value, indices=None):
        setattr(self, attr_name, value)

    def env_method(self, method_name, *args, indices=None, **kwargs):
        return [getattr(self, method_name)(*args, **kwargs)] * len(self._indices(indices))

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(self._indices(indices))

    # ---- camera images (QuadrupedGymEnv.render, utils/camera.py:35-59, for many environments at once; include/qs_amd.h qs_render)
    def _render_ids(self, indices):
        """device int32 ids; host ids are checked here and go over through page-locked staging without blocking"""
        t = self.torch
        if indices is None:
            if self._render_all is None:
                self._render_all = t.arange(self.num_envs, dtype=t.int32, device=self.device)
            return self._render_all
        if isinstance(indices, t.Tensor) and indices.device == self.device:
            if indices.dtype.is_floating_point or indices.dtype == t.bool or indices.dim() != 1:
                raise ValueError(f"indices must be a 1-D integer tensor, got {indices.dtype} {tuple(indices.shape)}")
            return indices.to(t.int32).contiguous()   # (not inspected on the host: an id out of range draws sky, id -2, and stats() raises)
        a = np.asarray(self._indices(indices.tolist() if isinstance(indices, (np.ndarray, t.Tensor)) else indices))
        if a.dtype.kind not in "iu" or a.ndim != 1:
            raise ValueError(f"indices must be integers, got {indices!r}")
        if a.size and (a.min() < 0 or a.max() >= self.num_envs):
            raise ValueError(f"environment ids must lie in [0, {self.num_envs}), got {a.min()} .. {a.max()}")
        return to_device_nowait(a.astype(np.int32), self.device)

    def _render(self, indices, camera, width, height, depth, segmentation):
        t = self.torch
        cam = as_camera(self.camera_mode if camera is None else camera)
        w0, h0 = self.render_size
        width, height = int(w0 if width is None else width), int(h0 if height is None else height)
        ids = self._render_ids(self.render_indices if indices is None else indices)
        m = ids.shape[0]
        check_request(m, width, height, "render_indices or render_size")
        self._stream()
        rgba = t.empty((m, height, width), dtype=t.int32, device=self.device)
        d = t.empty((m, height, width), dtype=t.float32, device=self.device) if depth else None
        sg = t.empty((m, height, width), dtype=t.int32, device=self.device) if segmentation else None
        c = cam.to_c()
        _lib.check(self.lib.qs_render(self.h, ptr(ids), m, C.byref(c), width, height, ptr(rgba), ptr(d), ptr(sg)))
        self._render_keep = ids
        return rgba, d, sg

    def render_tensor(self, indices=None, camera=None, width=None, height=None, depth=False, segmentation=False):
        """Camera images of the environments `indices` (None: render_indices; a list, an array or a device tensor of ids), on the device and
        without waiting for it: (rgb uint8 [M, H, W, 3], a view of the packed RGBA buffer; depth float32 [M, H, W] in metres along the view
        axis or None; segmentation int32 [M, H, W] or None).  camera: a mode name of qs_amd.render.CAMERA_MODES or a render.Camera (None:
        camera_mode); width / height default to render_size.  Host ids out of range raise here; ids in a device tensor are not inspected:
        such an image is sky with segmentation id -2, and the next stats() / counter() raises."""
        rgba, d, sg = self._render(indices, camera, width, height, depth, segmentation)
        return rgb_view(rgba), d, sg

    def get_images(self, indices=None):
        """VecEnv.get_images: one uint8 [H, W, 3] array per environment of render_indices (None = all), camera_mode, render_size"""
        rgba, _, _ = self._render(indices, None, None, None, False, False)
        host = rgba.cpu().numpy().view(np.uint8).reshape(*rgba.shape, 4)
        return [np.ascontiguousarray(host[i, :, :, :3]) for i in range(host.shape[0])]

    def render(self, mode="rgb_array", indices=None):
        """VecEnv.render: the images of get_images tiled as SB3 tiles them (tile_images); only mode "rgb_array" (no window here)"""
        if mode != "rgb_array":
            raise NotImplementedError(f"render mode {mode!r}: only 'rgb_array' (this build has no window)")
        return tile_images(self.get_images(indices))

    def _indices(self, indices):
        if indices is None:
            return list(range(self.num_envs))
        return [indices] if isinstance(indices, int) else list(indices)
