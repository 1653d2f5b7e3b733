"""Device snapshots on the GPU (qs_snapshot / qs_restore / qs_fork through QuadrupedVecEnv and the wrappers): a restored handle is bit for bit the
run that was never interrupted -- noise, randomizers, auto-resets and look-ahead on --, a fork is its source in another lane with its own
identity, and the look-ahead window is rebuilt behind a restore.

N = 40 (three waves, the last one partial), seed 3, JUMPING_IN_PLACE / PPO_BASIC / springs / GROUND_RANDOMIZER, reset_lookahead 4 unless a test
says otherwise.  Actions are "held bang-bang": every 8th step a fresh choice of -1 / +1 per action entry, held in between -- the float32 oracle
resets 30 of the 40 environments between steps 30 and 90 under it (38 with the filter off, noise and TEST_RANDOMIZER), where independent
uniform actions reset 4 of 40 in 120 steps."""
import ast

import numpy as np
import pytest

from test_gpu_round2 import RAW, torch_cuda, vec_env  # noqa: F401

pytestmark = pytest.mark.gpu

N = 40
BASE = dict(env_randomizer_mode="GROUND_RANDOMIZER", seed=3, auto_reset=True, reset_lookahead=4)


def held_bang_bang(n, d, steps):
    rng = np.random.default_rng(11)
    out = np.zeros((steps, n, d), np.float32)
    for i in range(steps):
        out[i] = rng.choice([-1, 1], (n, d)).astype(np.float32) if i % 8 == 0 else out[i - 1]
    return out


def roll(v, acts):
    """step_tensor under `acts` [T, N, d] -> what every step returned, on the host: observation, reward, done, truncated, and the
    terminal_observation rows of the environments that ended (zeros elsewhere)"""
    t = v.torch
    dev = t.as_tensor(acts, device=v.device)
    rec = dict(obs=[], rew=[], done=[], trunc=[], term=[])
    for a in dev:
        obs, rew, done, trunc = v.step_tensor(a)
        term = v.get_info("terminal_obs") * done[:, None].to(t.float32)
        for k, x in zip(("obs", "rew", "done", "trunc", "term"), (obs, rew, done, trunc, term)):
            rec[k].append(x.clone())
    return {k: t.stack(x).cpu().numpy() for k, x in rec.items()}


def assert_same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{what}: {k} differs first at (step, environment, ...) {bad[0].tolist()}, {len(bad)} entries in all"


def bits(x):
    return x.detach().cpu().numpy().view(np.uint32)


VARIANTS = dict(filter_on={}, noise_test_randomizer=dict(noise=True, env_randomizer_mode="TEST_RANDOMIZER", enable_action_filter=False),
                lookahead0=dict(reset_lookahead=0), step_variant2={})


def resume_run(torch, monkeypatch, variant):
    """reset, 30 steps, snapshot, 60 steps recorded, restore -> (handle, snapshot, the 90 actions, the record, the observation restore returned,
    the observation of step 29)"""
    if variant == "step_variant2":
        monkeypatch.setenv("QS_STEP_VARIANT", "2")
    v = vec_env(N, **dict(BASE, **VARIANTS[variant]))
    acts = held_bang_bang(N, v.action_dim, 90)
    v.reset_tensor()
    before = roll(v, acts[:30])
    snap = v.snapshot()
    first = roll(v, acts[30:])
    back = v.restore(snap).clone()
    return v, snap, acts, first, back, before["obs"][-1]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_exact_resume(torch_cuda, monkeypatch, variant):
    """1. reset, 30 steps, snapshot, 60 more steps; restore and the same 60 actions again: both passes bitwise equal in observation, reward,
    done, truncated and terminal observations -- with at least 20 of the 40 environments reset inside the replayed window (the oracle gives
    30, and 38 for the noise variant), or the test proves nothing about resets."""
    v, snap, acts, first, back, obs29 = resume_run(torch_cuda, monkeypatch, variant)
    assert np.array_equal(bits(back), obs29.view(np.uint32)), "restore returns the observation of the step before the snapshot"
    second = roll(v, acts[30:])
    reset_envs = int(first["done"].any(axis=0).sum())
    print(f"{variant}: {int(first['done'].sum())} resets of {reset_envs} environments in steps [30, 90)")
    assert reset_envs >= 20, f"only {reset_envs} of {N} environments reset inside the replayed window"
    assert_same(first, second, variant)
    v.close()


def test_resume_in_another_handle_through_a_file(torch_cuda, monkeypatch, tmp_path):
    """2. the snapshot goes through a file into a second handle with the same keywords, whose 60 steps are bitwise the first handle's; the
    first keeps running in between and is not disturbed"""
    from qs_amd.snapshot import EnvSnapshot
    a = vec_env(N, **BASE)
    acts = held_bang_bang(N, a.action_dim, 90)
    a.reset_tensor()
    roll(a, acts[:30])
    path = str(tmp_path / "snap.npz")
    a.snapshot().save(path)
    first_half = roll(a, acts[30:50])
    b = vec_env(N, **BASE)
    loaded = EnvSnapshot.load(path)
    assert loaded.rows.device.type == "cpu"
    b.restore(loaded)
    b_half = roll(b, acts[30:50])
    second_half = roll(a, acts[50:])
    b_rest = roll(b, acts[50:])
    assert int(np.concatenate([first_half["done"], second_half["done"]]).any(axis=0).sum()) >= 20
    assert_same(first_half, b_half, "steps 30 .. 49")
    assert_same(second_half, b_rest, "steps 50 .. 89")
    # another seed: refused as an exact resume, taken as a layout-compatible one
    c = vec_env(N, **dict(BASE, seed=4))
    with pytest.raises(ValueError, match="config_digest"):
        c.restore(loaded)
    c.restore(loaded, strict=False)
    assert np.array_equal(bits(c.get_state()), bits(EnvSnapshot.load(path).rows[:, 24:61].contiguous()))
    d = vec_env(N, **dict(BASE, wrapper="LANDING"))
    with pytest.raises(ValueError, match="layout_digest"):
        d.restore(loaded, strict=False)
    for x in (a, b, c, d):
        x.close()


GETTERS = ("task", "wrapper", "external_wrench", "torque", "foot_force", "last_action", "filtered_action", "counters", "params", "terminal_obs")


def everything(v, rack=False):
    out = {k: bits(v.get_info(k)) for k in GETTERS + (("rack",) if rack else ())}
    out["state"] = bits(v.get_state())
    return out


def test_everything_a_getter_can_see_comes_back(torch_cuda, golden):
    """3. snapshot -> 15 steps -> restore: get_state, the info getters, last and filtered action and the observation are bitwise what they
    were -- with the LANDING wrapper's phase machine and a pending 25-substep push on every third environment, on a rack with every fourth
    robot released, on a CPG handle (oscillators) and on a DEMO handle (counter)"""
    torch = torch_cuda

    def check(v, rack=False, prepare=None):
        acts = held_bang_bang(N, v.action_dim, 40)
        v.reset_tensor()
        roll(v, acts[:12])
        if prepare:
            prepare(v)
        obs, _, _, _ = v.step_tensor(torch.as_tensor(acts[12], device=v.device))
        obs = obs.clone()
        want = everything(v, rack)
        snap = v.snapshot()
        roll(v, acts[13:28])
        moved = everything(v, rack)
        assert any(not np.array_equal(moved[k], want[k]) for k in want)
        back = v.restore(snap)
        assert np.array_equal(bits(back), bits(obs))
        got = everything(v, rack)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        return want

    def push(v):
        v.apply_external_force(np.tile([30.0, -20.0, 10.0], (N, 1)).astype(np.float32), torque=[1.0, 2.0, -1.0], substeps=25, frame="link",
                               indices=list(range(0, N, 3)))

    v = vec_env(N, **dict(BASE, wrapper="LANDING"))
    want = check(v, prepare=push)
    left = want["external_wrench"].view(np.float32)[:, 6]
    # 25 substeps, one step of 10 taken: the push is pending in the snapshot (an episode that ended in that step cancelled its own)
    assert np.isin(left[0::3], (15, 0)).all() and (left[0::3] == 15).sum() >= 7 and (np.delete(left, np.s_[0::3]) == 0).all()
    v.close()

    v = vec_env(N, **dict(BASE, on_rack=True))
    want = check(v, rack=True, prepare=lambda v: v.set_rack(False, indices=list(range(0, N, 4))))
    hung = want["rack"].view(np.float32)[:, 0]
    assert (hung[0::4] == 0).sum() >= 5 and (np.delete(hung, np.s_[0::4]) == 1).all()      # (a reset in that step hangs its robot again)
    v.close()

    # CPG: the oscillators are state a getter does not show; the replayed steps show them
    v = vec_env(N, **dict(BASE, task_env="BACKFLIP", observation_space_mode="PPO_BACKFLIP", action_space_mode="CPG", seed=4))
    acts = held_bang_bang(N, v.action_dim, 40)
    v.reset_tensor()
    roll(v, acts[:10])
    snap = v.snapshot()
    first = roll(v, acts[10:30])
    v.restore(snap)
    assert_same(first, roll(v, acts[10:30]), "CPG")
    v.close()

    g = golden("demo.npz")
    kw = ast.literal_eval(str(g["demo_jip_kwargs"]))
    v = vec_env(8, auto_reset=True, demo=g["demo_jip_demo"], seed=3, **kw)
    v.reset_tensor()
    acts = held_bang_bang(8, v.action_dim, 30)
    roll(v, acts[:7])
    c0 = v.demo_counter().cpu().numpy()
    snap = v.snapshot()
    first = roll(v, acts[7:20])
    assert not np.array_equal(v.demo_counter().cpu().numpy(), c0)
    v.restore(snap)
    assert np.array_equal(v.demo_counter().cpu().numpy(), c0)
    assert_same(first, roll(v, acts[7:20]), "DEMO")
    v.close()


def test_masked_restore(torch_cuda):
    """4. restoring the odd environments rewinds them and leaves the even ones bitwise where they were (against a control handle that took
    the same steps and no restore)"""
    v, ctl = vec_env(N, **BASE), vec_env(N, **BASE)
    acts = held_bang_bang(N, v.action_dim, 70)
    v.reset_tensor(); ctl.reset_tensor()
    roll(v, acts[:30]); roll(ctl, acts[:30])
    snap = v.snapshot()
    at30 = everything(v)
    roll(v, acts[30:50]); roll(ctl, acts[30:50])
    odd = list(range(1, N, 2))
    obs = v.restore(snap, indices=odd).clone()
    got, there = everything(v), everything(ctl)
    for k in got:
        assert np.array_equal(got[k][1::2], at30[k][1::2]), f"{k}: the odd environments are back at step 30"
        assert np.array_equal(got[k][0::2], there[k][0::2]), f"{k}: the even environments were not touched"
    assert np.array_equal(bits(obs)[0::2], bits(ctl._obs)[0::2])
    # a masked snapshot writes only its rows
    rows0 = snap.rows.clone()
    v.snapshot(indices=[0, 2], out=snap)
    changed = (bits(snap.rows) != bits(rows0)).any(axis=1)
    assert changed[[0, 2]].all() and not np.delete(changed, [0, 2]).any()
    # both halves step on as their own runs: the even ones with the control handle
    a, b = roll(v, acts[50:]), roll(ctl, acts[50:])
    assert_same({k: x[:, 0::2] for k, x in a.items()}, {k: x[:, 0::2] for k, x in b.items()}, "even environments after the masked restore")
    v.close(); ctl.close()


def test_fork(torch_cuda):
    """5. fork(0): every environment is environment 0 in another lane / wave / the partial wave, bitwise, up to and including the first step
    in which environment 0 is done (of that step the terminal observation: the returned row is already the next episode's); episode numbers stay their own; a chain and a swap read pre-call sources; what is not named is a control
    handle's; a source of N is refused and reported; with noise the states agree and the observations do not"""
    torch = torch_cuda
    kw = dict(BASE, noise=False)
    v, ctl = vec_env(N, **kw), vec_env(N, **kw)
    acts = held_bang_bang(N, v.action_dim, 12)
    v.reset_tensor(); ctl.reset_tensor()
    # (different episode numbers to keep: environments 5 .. 9 take one more reset)
    extra = np.zeros(N, np.uint8); extra[5:10] = 1
    v.reset_tensor(extra); ctl.reset_tensor(extra)
    roll(v, acts); roll(ctl, acts)
    ep0 = v.get_info("counters").cpu().numpy()[:, 2].copy()
    ts0 = v.get_info("counters").cpu().numpy()[:, 3].copy()
    assert ep0[5] == ep0[0] + 1
    src_state = bits(v.get_state())[0].copy()
    v.fork(0)
    assert np.array_equal(bits(v.get_state()), np.tile(src_state, (N, 1)))
    assert np.array_equal(v.get_info("counters").cpu().numpy()[:, 2], ep0), "R_EPISODE stays each environment's own"
    assert np.array_equal(v.get_info("counters").cpu().numpy()[:, 3], ts0), "R_TOTAL_STEPS stays each environment's own"
    shared = np.tile(held_bang_bang(1, v.action_dim, 25), (1, N, 1))
    rec, ref = roll(v, shared), roll(ctl, shared)
    done0 = np.flatnonzero(rec["done"][:, 0])
    upto = int(done0[0]) + 1 if done0.size else 25
    print(f"environment 0 is done first in step {done0[0] if done0.size else None} of 25")
    # (the observation ROW of the step in which an environment is done is its next episode's first, SB3's convention, and that episode is the
    # fork's own: the step's own observation is the terminal one, compared below)
    for k in ("obs", "rew", "done", "trunc"):
        x = rec[k][:upto - 1] if k == "obs" and done0.size else rec[k][:upto]
        x = x.view(np.uint32) if x.dtype.kind == "f" else x
        assert (x == x[:, :1]).all(), f"{k}: some fork left environment 0's path, first at (step, environment) {np.argwhere(x != x[:, :1])[0][:2].tolist()}"
    tm = rec["term"][:upto].view(np.uint32)
    assert (tm == tm[:, :1]).all(), "terminal observations"
    assert_same({k: x[:, :1] for k, x in rec.items()}, {k: x[:, :1] for k, x in ref.items()}, "the source against the control handle")
    v.close(); ctl.close()

    # chain, swap, unnamed environments, refusal
    v, ctl = vec_env(N, **kw), vec_env(N, **kw)
    v.reset_tensor(); ctl.reset_tensor()
    roll(v, acts); roll(ctl, acts)
    pre = everything(ctl)
    src_of = np.full(N, -1, np.int32)
    src_of[[1, 2]] = [2, 3]            # a chain: 1 <- 2 while 2 <- 3
    src_of[[20, 39]] = [39, 20]        # a swap across waves (39 sits in the partial wave)
    src_of[7] = 7                      # its own index: left alone
    v.fork(src_of=src_of)
    got = everything(v)
    kept = dict(counters=[2, 3])       # columns of the getter that are the kept fields
    for k in got:
        for i in range(N):
            s = src_of[i] if src_of[i] >= 0 else i
            want = pre[k][s].copy()
            if k in kept:
                want[kept[k]] = pre[k][i][kept[k]]
            assert np.array_equal(got[k][i], want), f"{k}: environment {i} should hold environment {s}'s pre-call values"
    obs = v._obs                       # (fork leaves the handle's last observations there, as restore does)
    assert np.array_equal(bits(obs)[1], bits(ctl._obs)[2]) and np.array_equal(bits(obs)[39], bits(ctl._obs)[20])
    # host indices are checked on the host
    for bad in (dict(src=N), dict(src=0, dst=[N]), dict(src=[0, 1], dst=[2]), dict(src=0, dst=[3, 3]), dict(src_of=np.full(N, N))):
        with pytest.raises(ValueError):
            v.fork(**bad)
    # a device src_of goes straight to the kernel: N leaves that environment alone and the next counter() names it
    before = everything(v)
    dev_src = torch.full((N,), -1, dtype=torch.int32, device=v.device)
    dev_src[11] = N
    dev_src[12] = 0
    v.fork(src_of=dev_src)
    with pytest.raises(RuntimeError, match=r"qs_fork refused the source of environment 11\b"):
        v.counter("resets")
    v.counter("resets")                # reported once
    after = everything(v)
    assert np.array_equal(after["state"][11], before["state"][11]) and np.array_equal(after["state"][12], before["state"][0])
    v.close(); ctl.close()

    # noise: each fork keeps its own noise stream
    v = vec_env(N, **dict(BASE, noise=True))
    v.reset_tensor()
    roll(v, acts)
    v.fork(0)
    obs, _, _, _ = v.step_tensor(torch.as_tensor(shared[0], device=v.device))
    st = bits(v.get_state())
    assert (st == st[:1]).all(), "the forks' states agree bitwise after one step"
    o = bits(obs)
    assert all((o[i] != o[0]).any() for i in range(1, N)), "every fork's observation carries its own noise"
    v.close()


def test_the_lookahead_window_is_rebuilt(torch_cuda):
    """6. settle_steps = 100 (one settle takes 10 launches).  Snapshot at step 20, steps to 60, restore; then 40 launches with zero actions --
    three settle epochs plus 10, where the design's bound for a wanted state is one epoch of settling plus at most a fifth of an epoch
    waiting for a cohort.  A reset of every environment then takes its look-ahead state: reset_stalls does not move and lookahead_served
    rises by 40.  At least 10 environments were rewound by the restore (the oracle gives 22, at most two episodes each, below K).  An
    implementation that restores the records and leaves `handed` alone fails exactly here."""
    torch = torch_cuda
    v = vec_env(N, **dict(BASE, settle_steps=100))
    acts = held_bang_bang(N, v.action_dim, 60)
    v.reset_tensor()
    roll(v, acts[:20])
    snap = v.snapshot()
    ep20 = v.get_info("counters").cpu().numpy()[:, 2].copy()
    roll(v, acts[20:])
    ep60 = v.get_info("counters").cpu().numpy()[:, 2].copy()
    rewound = int((ep60 > ep20).sum())
    print(f"{rewound} environments rewound, by at most {int((ep60 - ep20).max())} episodes")
    assert rewound >= 10
    v.restore(snap)
    assert np.array_equal(v.get_info("counters").cpu().numpy()[:, 2], ep20)
    zero = torch.zeros((N, v.action_dim), device=v.device)
    for _ in range(40):
        v.step_tensor(zero)
    stalls, served = v.counter("reset_stalls"), v.counter("lookahead_served")
    v.reset_tensor()
    stalls1, served1 = v.counter("reset_stalls"), v.counter("lookahead_served")
    print(f"reset_stalls {stalls} -> {stalls1}, lookahead_served {served} -> {served1}")
    assert stalls1 == stalls
    assert served1 == served + N
    v.close()


def test_a_restored_handle_is_an_ordinary_handle(torch_cuda):
    """7. after a snapshot, more steps and a restore, yardstick.resynced_parity holds the handle to the oracle for 20 steps as it holds a
    fresh one.  resynced_parity resets the device and the oracles itself when an episode ends, so the handle is one without auto-reset
    (this test resets finished environments by hand), and because the ground randomizer draws per (seed, environment, episode) the
    oracles are reset as often as each environment of the handle was."""
    import yardstick as Y
    from oracle.qso import Oracle
    torch = torch_cuda
    n = 16
    v = vec_env(n, **dict(BASE, auto_reset=False))
    acts = held_bang_bang(n, v.action_dim, 40)

    def run(rows):
        for a in rows:
            _, _, done, _ = v.step_tensor(torch.as_tensor(a, device=v.device))
            if bool(done.any()):
                v.reset_tensor(done.clone())

    v.reset_tensor()
    run(acts[:30])
    snap = v.snapshot()
    run(acts[30:])
    v.restore(snap)
    v.reset_tensor()
    episodes = v.get_info("counters").cpu().numpy()[:, 2].astype(int)
    o, o32 = Oracle(v.cfg), Oracle(v.cfg, "f32")
    for k in range(int(episodes.max()) + 1):
        m = (episodes >= k).astype(np.uint8)
        o.reset(m); o32.reset(m)
    assert np.array_equal(o.get_info(7)[:, 2].astype(int), episodes)
    rec = Y.resynced_parity(o, o32, Y.VecEnvDevice(v), v.cfg, v.meta["layout"], steps=20)
    assert rec["env_steps"] >= 20 * n - 4 and len(rec["outliers"]) <= 1, rec
    o.close(); o32.close(); v.close()


def test_reference_state_init_wrapper(torch_cuda, golden, tmp_path):
    """8b. ReferenceStateInitVecEnv carries its generator's state and reset counters: after a restore (through a file) the finished
    environments are re-seated in the same rows of the demonstration as the first time, and every step is bitwise the same"""
    from qs_amd import EnvSnapshot, QuadrupedVecEnv, ReferenceStateInitVecEnv
    torch = torch_cuda
    g = golden("demo.npz")
    kw = ast.literal_eval(str(g["demo_jip_kwargs"]))
    n = 16
    venv = ReferenceStateInitVecEnv(QuadrupedVecEnv(num_envs=n, auto_reset=True, demo=g["demo_jip_demo"], noise=False, seed=3, **kw), seed=11)
    acts = torch.as_tensor(held_bang_bang(n, venv.action_dim, 80), device=venv.device)
    venv.reset_tensor()

    def run(rows):
        out = []
        for a in rows:
            obs, rew, done, trunc = venv.step_tensor(a)
            out.append((bits(obs), bits(rew), done.cpu().numpy().copy(), venv.random_el.copy(), venv.demo_counter().cpu().numpy()))
        return out

    run(acts[:20])
    path = str(tmp_path / "rsi.npz")
    venv.snapshot().save(path)
    first = run(acts[20:])
    reseated = int(sum(x[2].sum() for x in first))
    print(f"{reseated} re-seatings in the replayed window")
    assert reseated >= 1
    venv.restore(EnvSnapshot.load(path))
    second = run(acts[20:])
    for t, (x, y) in enumerate(zip(first, second)):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), f"step {20 + t}"
    venv.close()


def test_wrappers(torch_cuda, tmp_path):
    """8. DeviceVecNormalize(training=True): snapshot -> 20 steps -> restore -> the same 20 actions give bitwise the same normalised
    observations, rewards and statistics, also through a file.  The numpy path (env.step) works right after a restore and returns what
    step_tensor returns from the same snapshot.  QuadrupedGymEnv round-trips one robot."""
    from qs_amd import DeviceVecNormalize
    from qs_amd.env.quadruped_gym_env import QuadrupedGymEnv
    from qs_amd.snapshot import EnvSnapshot
    torch = torch_cuda
    env = DeviceVecNormalize(vec_env(N, **BASE), training=True)
    acts = held_bang_bang(N, env.action_dim, 50)
    env.reset_tensor()
    roll(env, acts[:30])
    snap = env.snapshot()
    path = str(tmp_path / "norm.npz")
    snap.save(path)
    stats30 = env.get_stats()
    first = roll(env, acts[30:])
    stats50 = env.get_stats()
    for s in (snap, EnvSnapshot.load(path)):
        env.restore(s)
        back = env.get_stats()
        assert all(np.array_equal(np.asarray(back[k]), np.asarray(stats30[k])) for k in stats30)
        assert_same(first, roll(env, acts[30:]), "DeviceVecNormalize")
        again = env.get_stats()
        assert all(np.array_equal(np.asarray(again[k]), np.asarray(stats50[k])) for k in stats50), "the statistics after the replay"
    # a fork under the wrapper takes the source's discounted return along
    ret = env._returns().cpu().numpy()
    env.fork(3, [4, 5])
    ret1 = env._returns().cpu().numpy()
    assert ret1[4] == ret[3] and ret1[5] == ret[3] and np.array_equal(np.delete(ret1, [4, 5]), np.delete(ret, [4, 5]))
    env.close()

    # the numpy path right after a restore
    v = vec_env(N, **BASE)
    acts = held_bang_bang(N, v.action_dim, 60)
    v.reset()
    for a in acts[:30]:
        _, _, _, infos = v.step(a)
    held = [i for i in range(N) if infos[i]]
    snap = v.snapshot()
    dev = roll(v, acts[30:])
    v.restore(snap)
    assert all(not d for d in v._infos)
    for t, a in enumerate(acts[30:]):
        obs, rew, done, infos = v.step(a)
        assert np.array_equal(obs.view(np.uint32), dev["obs"][t].view(np.uint32)) and np.array_equal(rew.view(np.uint32), dev["rew"][t].view(np.uint32))
        assert np.array_equal(done, dev["done"][t].astype(bool))
        for i in np.flatnonzero(done):
            assert np.array_equal(infos[i]["terminal_observation"].view(np.uint32), dev["term"][t][i].view(np.uint32))
            assert infos[i]["TimeLimit.truncated"] == bool(dev["trunc"][t][i])
    assert dev["done"].any()
    print(f"{len(held)} infos entries were filled at the snapshot")
    v.close()

    g = QuadrupedGymEnv(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, enable_action_filter=True,
                        env_randomizer_mode="GROUND_RANDOMIZER", seed=3, noise=True)
    g.reset()
    one = held_bang_bang(1, g.action_dim, 30)[:, 0]
    for a in one[:10]:
        last = g.step(a)[0]
    snap = g.snapshot()
    first = [g.step(a) for a in one[10:]]
    back = g.restore(snap)
    assert all(np.array_equal(back[k], last[k]) for k in last)
    assert np.array_equal(g._last_action, one[9].astype(np.float64))
    second = [g.step(a) for a in one[10:]]
    for x, y in zip(first, second):
        assert all(np.array_equal(x[0][k], y[0][k]) for k in x[0]) and x[1:3] == y[1:3]
    g.close()
