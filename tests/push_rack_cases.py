"""The schedules under which external pushes and the rack are held to the oracle (TEST INFRASTRUCTURE): one definition for the CPU twins on
the host emulation (test_emu_push.py, test_emu_rack.py) and for the GPU tests (test_gpu_push.py, test_gpu_rack.py), which run them through
yardstick.resynced_parity, and the coverage each must reach -- a test may not pass by avoiding the case it exists for.  Seeds and
magnitudes are chosen so that the float64 and the float32 oracle alone meet the counts."""
import numpy as np

import yardstick as Y

N = 16          # one wave per handle
DEFAULT = dict(task_env="JUMPING_IN_PLACE", observation_space_mode="PPO_BASIC", enable_springs=True, enable_action_filter=True,
               env_randomizer_mode="NONE", noise=False, auto_reset=False, body_contacts=True, settle_steps=300)
RAW = dict(task_env="NO_TASK", observation_space_mode="ENCODER", enable_action_filter=False, isRLGymInterface=False, motor_control_mode="TORQUE")
RACK = dict(task_env="NO_TASK", on_rack=True, noise=False, auto_reset=False, body_contacts=True, settle_steps=300, env_randomizer_mode="NONE")


def ground_pushes(steps, seed, durations=(0, 1, 5, 25)):
    """every 3rd step a push of +-150 N / +-8 N m on every environment, durations drawn from `durations`, world and link frame in turn"""
    rng = np.random.default_rng(seed)
    sched = {}
    for k, i in enumerate(range(0, steps, 3)):
        w = np.concatenate([rng.uniform(-150, 150, (N, 3)), rng.uniform(-8, 8, (N, 3))], 1)
        sched[i] = [("push", w, rng.choice(durations, N).astype(np.int32), "world" if k % 2 == 0 else "link", None)]
    return sched


def topple_pushes(steps, seed):
    """every 5th step a lateral shove of 300 - 600 N with a roll torque of 150 - 250 N m for 60 substeps on half of the environments (the
    halves in turn): robots that hold their stance under PD go over onto their sides all the same (with 60 - 90 N m, what throws a limp
    robot, the legs catch nearly every one) -- impacts through the many-rows solve"""
    rng = np.random.default_rng(seed)
    sched = {}
    for k, i in enumerate(range(0, steps, 5)):
        side = rng.choice([-1.0, 1.0], N)
        w = np.zeros((N, 6))
        w[:, 1] = side * rng.uniform(300.0, 600.0, N)
        w[:, 3] = -side * rng.uniform(150.0, 250.0, N)
        sched[i] = [("push", w, np.full(N, 60, np.int32), "world", np.arange(N) % 2 == k % 2)]
    return sched


def long_pushes(steps, seed):
    """pushes of 25 substeps every 8th step: with action_repeat = 4 the count crosses six env steps"""
    rng = np.random.default_rng(seed)
    sched = {}
    for k, i in enumerate(range(0, steps, 8)):
        w = np.concatenate([rng.uniform(-150, 150, (N, 3)), rng.uniform(-8, 8, (N, 3))], 1)
        sched[i] = [("push", w, np.full(N, 25, np.int32), "world" if k % 2 == 0 else "link", None)]
    return sched


def rehang(steps, seed):
    """a third of the environments released at step 4, all hung again at step 12 while they are still falling: the rack's bound binds"""
    return {4: [("rack", False, np.arange(N) % 3 == 0)], 12: [("rack", True, None)]}


def stop_actions(i, a):
    """raw torques: the calves of half of the environments against their stops, one way then the other (test_gpu_rack.stop_actions)"""
    a = a * np.float32(0.3)
    a[: N // 2, 2::3] = -30.0 if i % 8 < 4 else 30.0
    return a


def low_anchor(cfg_kw):
    """the rack's anchor 4 mm below the height the robot settles at when it stands free: the feet bear on the floor while it hangs"""
    from oracle.qso import Oracle
    from qs_amd.config import build_config
    cfg, _ = build_config(n_envs=1, **{k: v for k, v in cfg_kw.items() if k != "on_rack"})
    o = Oracle(cfg)
    o.reset()
    z = float(o.get_state()[0, 2])
    o.close()
    return np.array([0.0, 0.0, z - 0.004], np.float32)


# name -> (build_config keywords, steps, schedule builder or None, actions or None, coverage: record key -> least count)
PUSH_CASES = {
    "ground_cone": (dict(DEFAULT), 40, ground_pushes, None, dict(push_contact_env_steps=100)),
    "ground_pyramid": (dict(DEFAULT, friction_model="pyramid"), 40, ground_pushes, None, dict(push_contact_env_steps=100)),
    # (NO_TASK: a toppled robot stays down and goes on being compared; under a task its first impact ends the episode)
    "topple": (dict(DEFAULT, task_env="NO_TASK"), 30, topple_pushes, None, dict(push_contact_env_steps=100, impact_env_steps=30)),
    "repeat4": (dict(DEFAULT, action_repeat=4, time_step=0.0025), 40, long_pushes, None, dict(push_contact_env_steps=100)),
}
RACK_CASES = {
    "hung_cone": (dict(RACK), 40, None, None, dict()),
    "hung_pyramid": (dict(RACK, friction_model="pyramid"), 40, None, None, dict()),
    "low_anchor": (dict(RACK), 40, None, None, dict(rack_contact_rows=100)),
    # three sweeps instead of fifty: an unconverged PGS keeps the ORDER of its rows in its result (the rack's before the contacts); converged,
    # every order gives the same answer
    "low_anchor_sweeps3": (dict(RACK), 40, None, None, dict(rack_contact_rows=100)),
    "rehang": (dict(RACK), 40, rehang, None, dict(rack_bound_rows=20)),
    "stops": (dict(RACK, env_randomizer_mode="GROUND_RANDOMIZER", **RAW), 14, None, stop_actions, dict(rack_limit_rows=16)),
}


class OracleDevice:
    """the oracle's float32 build behind the device protocol: what the same formulation gives in the kernels' precision"""

    def __init__(self, cfg, meta):
        from oracle.qso import Oracle
        self.o = Oracle(cfg, "f32", rack=meta["rack"] if meta["rack"]["on"] else None)
        self.o.reset()

    def set_state(self, s):
        self.o.set_state(s)

    def get_state(self):
        return self.o.get_state()

    def step(self, a):
        return self.o.step(a)

    def reset(self, mask):
        self.o.reset(mask)

    def reset_to(self, mask, states):
        self.o.reset_to(states, mask)

    def extra(self):
        out = dict(torque=self.o.get_info(2), foot_force=self.o.get_info(0), reward_end=self.o.eval_reward(1))
        if self.o.on_rack:
            out["rack"] = self.o.get_info(15)
        return out

    def flags(self):
        return self.o.get_info(1)

    def set_push(self, wrench, substeps, frame, mask=None):
        self.o.set_external_wrench(wrench, substeps, frame, mask)

    def push_left(self):
        return self.o.get_info(14)[:, 6]

    def set_rack(self, hung, mask=None):
        self.o.set_rack(hung, mask)

    def hung(self):
        return self.o.get_info(15)[:, 0]


def build(case, table):
    """-> cfg, meta, steps, schedule, actions, coverage of a case (the low-anchor case moves meta["rack"]["pos"], as from_config takes it)"""
    from qs_amd.config import build_config
    kw, steps, sched, actions, cover = table[case]
    cfg, meta = build_config(n_envs=N, **kw)
    if case == "stops":
        cfg.tau_max[:] = [40.0, 40.0, 40.0]
    if case.startswith("low_anchor"):
        meta["rack"]["pos"] = low_anchor(kw)
    if case == "low_anchor_sweeps3":
        cfg.solver_iters = 3
    return cfg, meta, steps, (sched(steps, 7) if sched else None), actions, cover


def run(case, table, make_device, seed=1):
    """the case through resynced_parity: make_device(cfg, meta) -> an object of the device protocol (already reset); -> the record"""
    from oracle.qso import Oracle
    cfg, meta, steps, sched, actions, cover = build(case, table)
    rack = meta["rack"] if meta["rack"]["on"] else None
    o, o32 = Oracle(cfg, rack=rack), Oracle(cfg, "f32", rack=rack)
    dev = make_device(cfg, meta)
    o.reset(); o32.reset()
    rec = Y.resynced_parity(o, o32, dev, cfg, meta["layout"], steps=steps, seed=seed, schedule=sched if sched is not None else {}, actions=actions)
    o.close(); o32.close()
    rec["case"], rec["coverage_required"] = case, cover
    return rec


def check(rec, name, what="device"):
    """the coverage the case exists for, the yardstick's caps, the percentile rule over the impact rows; one line into
    push_rack_parity.jsonl next to the other parity records (test_gpu_parity.record_jsonl)"""
    out = {k: v for k, v in rec.items() if not isinstance(v, (dict, list)) or k in ("coverage_required", "outliers")}
    out.update(test=name, compared=what)
    for g in ("rack_force", "rack_torque"):
        if rec.get("rack_own_smooth", {}).get(g):
            out[g + "_own_smooth_p50_p90_p99"] = Y.percentiles(rec["rack_own_smooth"][g])
    pct = {}
    for g, _, _, tol in Y.STATE_GROUPS:
        pct[g] = dict(device_p50_p90_p99=Y.percentiles(rec["impact_dev"][g]), oracle32_p50_p90_p99=Y.percentiles(rec["impact_own"][g]), tol=tol)
    out["impact"] = pct
    print("push / rack parity:", out)
    from test_gpu_parity import record_jsonl
    record_jsonl("push_rack_parity", out)
    for key, least in rec["coverage_required"].items():
        assert rec[key] >= least, f"{name}: {key} = {rec[key]}, the case needs at least {least}"
    assert len(rec["outliers"]) <= 1, rec["outliers"]      # (each within 3 x its bound: asserted where it was found)
    for g, r in pct.items():
        if len(rec["impact_dev"][g]) >= 30:
            dev, own = r["device_p50_p90_p99"], r["oracle32_p50_p90_p99"]
            assert dev[1] <= r["tol"] + 2 * own[1] and dev[2] <= r["tol"] + 2 * own[2], f"{name} {g}: |{what} - oracle64| p50 / p90 / p99 {dev} against the float32 oracle's own {own}"
    return out
