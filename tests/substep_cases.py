"""Case families for ONE physics substep (TEST INFRASTRUCTURE; shared by tests/test_substep_cpu.py and tests/test_gpu_substep.py): records,
torques and pushes with fixed seeds, the float64 and the float32 oracle's substep from them, and the bounds a float32 implementation of the
same substep is held to.

A draw is kept only if, judged in float64 alone, it sits clear of every switch of the substep: no ground-contact candidate (feet, trunk
corners, hip cylinders, both ends of the thigh boxes, both ends of the calf boxes, the payload block) within MARGIN of its contact range, no
joint within MARGIN of a stop, and the float64 oracle's list of link-link contacts unchanged under joint displacements that move the links by
more than MARGIN.  The candidates' heights are restated here in numpy float64 (heights()) and checked against the float64 oracle's own
contact list of every draw (Oracle.contacts).  At most CAP of a family's draws may be rejected: the generators aim well clear of the
switches, the rejections are what chance leaves."""
import functools
import math

import numpy as np

import yardstick as Y
from emu import emu as E
from oracle.qso import Oracle
from qs_amd.config import build_config

MARGIN = 1e-5           # m, rad
CAP = 0.05
N_FAMILY, N_DRAWS = 256, 272        # 16 waves kept of 17 drawn: at most 13 of the 272 may be rejected (CAP), so 256 are always left
TAU_FLIGHT = 2.0        # N m (gen_flight)
TWIN_RATIO = 0.7        # the host twin's worst |twin - oracle64| / bound, at most (tests/test_substep_cpu.py)

HIP_X, HIP_Y, THIGH_Y, LEG_Z, FOOT_R = 0.1881, 0.04675, 0.08, -0.213, 0.02            # go1.urdf, as csrc/qs_core.h and oracle/qso_phys.c state them
THR_FOOT, THR_TRUNK, THR_HIP, THR_THIGH, THR_CALF, THR_PAYLOAD = 0.000727, 0.00407, 0.00139, 0.00433, 0.00429, 0.00173
TRUNK_HALF, HIP_CYL_H, HIP_CYL_R = (0.1881, 0.04675, 0.057), 0.02, 0.046
THIGH_HALF, CALF_HALF, PAYLOAD_HALF = (0.017, 0.01225), 0.008, 0.05
JLO, JHI = Y.JOINT_LO, Y.JOINT_HI
R_PARAMS, R_POS, R_WARM, R_N_INVALID, R_FOOT_FORCE, R_FOOT_CONTACT, R_BLOCK = 0, 24, 61, 173, 211, 215, 244       # csrc/qs_layout.h (checked against Emu.field in the CPU test)
P_MU, P_M_PAY, P_R_PAY = 0, 20, 21

BASE = dict(noise=False, isRLGymInterface=False, motor_control_mode="TORQUE", task_env="NO_TASK", observation_space_mode="ENCODER", enable_action_filter=False,
            enable_springs=False, body_contacts=True, env_randomizer_mode="NONE")
# body_contacts on everywhere; self-collision on and off; 30 sweeps at 1 ms and 60 at 2 ms; residual threshold 0 and 1e-7; both friction models
CONFIGS = {
    "cone": dict(friction_model="cone", self_collision=True, solver_residual_threshold=0.0),
    "pyramid": dict(friction_model="pyramid", self_collision=True, solver_residual_threshold=0.0),
    "cone_thr_noself": dict(friction_model="cone", self_collision=False, solver_residual_threshold=1e-7),
    "pyramid_thr_noself": dict(friction_model="pyramid", self_collision=False, solver_residual_threshold=1e-7),
    "cone_dt2": dict(friction_model="cone", self_collision=True, solver_residual_threshold=1e-7, time_step=0.002, action_repeat=5),
    "pyramid_dt2": dict(friction_model="pyramid", self_collision=False, solver_residual_threshold=0.0, time_step=0.002, action_repeat=5),
    # the mass randomizer's draws (masses, payload 0 - 1 kg and where it sits) under both mass-to-inertia rules; the payload as a body of its own
    "cone_mass_shape": dict(friction_model="cone", self_collision=True, solver_residual_threshold=0.0, env_randomizer_mode="MASS_RANDOMIZER", mass_inertia_rule="collision_shape"),
    "pyramid_mass_scale": dict(friction_model="pyramid", self_collision=True, solver_residual_threshold=1e-7, env_randomizer_mode="MASS_RANDOMIZER", mass_inertia_rule="scale"),
    "cone_soft": dict(friction_model="cone", self_collision=True, solver_residual_threshold=0.0, env_randomizer_mode="MASS_RANDOMIZER", payload="soft"),
}
PLAIN = ["cone", "pyramid", "cone_thr_noself", "pyramid_thr_noself", "cone_dt2", "pyramid_dt2"]
MASSES = ["cone_mass_shape", "pyramid_mass_scale", "cone_soft"]
FAMILIES = ["flight", "stance", "stops", "fallen"]
# (family, configuration) of the tests: every family under both friction models, each other setting at least once per family
MATRIX = [(f, c) for f in FAMILIES for c in PLAIN] + [("parameters", c) for c in MASSES] + [("stance", "cone_soft")]      # (the last: the common-path build with the payload's rows, finishing)
EDGES = [("edges", c) for c in ("cone", "pyramid", "cone_soft")]


def builds_of(config):
    return ["full", "hot"] + (["hot_soft"] if CONFIGS[config].get("payload") == "soft" else [])


def config(name, n):
    return build_config(n_envs=n, **dict(BASE, **CONFIGS[name]))[0]


# ---------------------------------------------------------------- geometry in float64
def _rot(quat):
    x, y, z, w = (quat[:, k] / np.linalg.norm(quat, axis=1) for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def heights(s, m_pay=None, r_pay=None, blocks=None):
    """Heights above the plane of everything that can touch it, for states [n, 37] in float64: `foot` [n, 4] (the sphere's lowest point),
    `cand` [n, 4, 5] (per leg: the trunk corner on its side, its hip cylinder, the thigh box at its hip end and at its knee end, the calf box
    at its knee end -- the support-point candidates), `calf_lo` [n, 4] (the calf box at its foot end: counted, never a support point),
    `payload` [n] (its box's lowest corner; nan without a payload).  blocks [n, 20]: the payload as a body of its own."""
    s = np.asarray(s, np.float64)
    n = len(s)
    Rz = _rot(s[:, 3:7])[:, 2, :]            # world z of the base axes
    zc = s[:, 2]
    out = dict(foot=np.zeros((n, 4)), cand=np.zeros((n, 4, 5)), calf_lo=np.zeros((n, 4)))
    for L in range(4):
        fx, sy = (1.0 if L < 2 else -1.0), (1.0 if L & 1 else -1.0)
        q1, q2, q3 = s[:, 13 + 3 * L], s[:, 14 + 3 * L], s[:, 15 + 3 * L]
        s1, c1, s2, c2, s23, c23 = np.sin(q1), np.cos(q1), np.sin(q2), np.cos(q2), np.sin(q2 + q3), np.cos(q2 + q3)
        o = np.zeros(n)
        p1 = np.stack([fx * HIP_X + o, sy * HIP_Y + o, o], 1)
        Yv = np.stack([o, c1, s1], 1)
        p2 = p1 + Yv * (sy * THIGH_Y)
        X2, Z2 = np.stack([c2, s1 * s2, -c1 * s2], 1), np.stack([s2, -s1 * c2, c1 * c2], 1)
        p3 = p2 + Z2 * LEG_Z
        X3, Z3 = np.stack([c23, s1 * s23, -c1 * s23], 1), np.stack([s23, -s1 * c23, c1 * c23], 1)
        rf = p3 + Z3 * LEG_Z
        dot = lambda a, b: (a * b).sum(axis=1)
        az, gx2, gx3 = dot(Rz, Yv), dot(Rz, X2), dot(Rz, X3)
        th_off = np.abs(gx2) * THIGH_HALF[0] + np.abs(az) * THIGH_HALF[1]
        cf_off = (np.abs(gx3) + np.abs(az)) * CALF_HALF
        out["foot"][:, L] = zc + dot(Rz, rf) - FOOT_R
        out["cand"][:, L, 0] = zc + Rz[:, 0] * fx * TRUNK_HALF[0] + Rz[:, 1] * sy * TRUNK_HALF[1] - np.abs(Rz[:, 2]) * TRUNK_HALF[2]
        out["cand"][:, L, 1] = zc + dot(Rz, p1) - HIP_CYL_H * np.abs(az) - HIP_CYL_R * np.sqrt(np.maximum(1 - az * az, 0.0))
        out["cand"][:, L, 2] = zc + dot(Rz, p2) - th_off
        out["cand"][:, L, 3] = zc + dot(Rz, p3) - th_off
        out["cand"][:, L, 4] = zc + dot(Rz, p3) - cf_off
        out["calf_lo"][:, L] = zc + dot(Rz, rf) - cf_off
    pay = np.full(n, np.nan)
    if m_pay is not None:
        if blocks is not None:
            Rb = _rot(blocks[:, 3:7])[:, 2, :]
            h = blocks[:, 2] - np.abs(Rb).sum(axis=1) * PAYLOAD_HALF
        else:
            h = zc + (Rz * r_pay).sum(axis=1) - np.abs(Rz).sum(axis=1) * PAYLOAD_HALF
        pay = np.where(m_pay > 0, h, np.nan)
    out["payload"] = pay
    return out


CAND_THR = np.array([THR_TRUNK, THR_HIP, THR_THIGH, THR_THIGH, THR_CALF])


def ground_clearance(h, slop=None):
    """[n]: the least |height - contact range| over every candidate of heights(): the ground margin of a draw; with `slop` also the least
    |height + slop| over the support-point candidates (the depth at which a candidate's rows exist whatever its speed: a switch as well)"""
    d = [np.abs(h["foot"] - THR_FOOT).min(axis=1), np.abs(h["cand"] - CAND_THR).reshape(len(h["foot"]), -1).min(axis=1), np.abs(h["calf_lo"] - THR_CALF).min(axis=1)]
    d.append(np.where(np.isnan(h["payload"]), np.inf, np.abs(h["payload"] - THR_PAYLOAD)))
    if slop is not None:
        d.append(np.abs(h["cand"] + slop).reshape(len(h["foot"]), -1).min(axis=1))
    return np.min(np.stack(d, 1), axis=1)


def ground_links(h):
    """per environment the set of (link index as Oracle.contacts numbers it; -1 the payload) within contact range of the plane"""
    out = []
    for i in range(len(h["foot"])):
        links = set()
        for L in range(4):
            if h["foot"][i, L] < THR_FOOT:
                links.add(5 + 4 * L)
            if h["cand"][i, L, 0] < THR_TRUNK:
                links.add(0)
            if h["cand"][i, L, 1] < THR_HIP:
                links.add(2 + 4 * L)
            if min(h["cand"][i, L, 2], h["cand"][i, L, 3]) < THR_THIGH:
                links.add(3 + 4 * L)
            if min(h["cand"][i, L, 4], h["calf_lo"][i, L]) < THR_CALF:
                links.add(4 + 4 * L)
        if h["payload"][i] < THR_PAYLOAD:
            links.add(-1)
        out.append(links)
    return out


def joint_clearance(s):
    q = np.asarray(s, np.float64)[:, 13:25]
    return np.minimum(np.abs(q - JLO), np.abs(JHI - q)).min(axis=1)


# ---------------------------------------------------------------- generators: states [n, 37], torques [n, 12], warm start [n, 4], mu [n]
def _unit(rng, n, k):
    v = rng.normal(size=(n, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _euler_quat(roll, pitch, yaw):
    from scipy.spatial.transform import Rotation as Rot
    return Rot.from_euler("xyz", np.stack([roll, pitch, yaw], 1)).as_quat()


def gen_flight(rng, n, cfg):
    """no contact: any attitude, |omega| up to 8 rad/s, joints across their range, |qd| up to 20 rad/s and a tenth with a joint rate beyond
    vel_cap (the clamp); torques uniform within +-TAU_FLIGHT.  (Not up to tau_max: the float32 CRBA + Schur path about the base origin
    rounds a torque-driven change of the joint rates 5 - 8 x as coarsely as the float32 ABA does -- about 8 ulp of the change against 1.5,
    measured on the host twin: one joint at tau_max is 1e4 rad/s2 on a calf -- where it sits at 2.5 x in the velocity-product terms.  That
    much is the algorithm.  A bound of FACTOR x the oracle's own rounding cannot hold a family whose errors are torque-driven: the twin
    reads 0.8 - 1.4 x the bound with every joint uniform up to tau_max, 1.2 - 2.4 x with one saturated joint per environment, 0.6 - 1.25 x
    with N(0, 5 N m), and 0.3 - 0.5 x here.  A wrong term of the dynamics is a relative error of the acceleration, far above eight ulp at
    any torque.)"""
    s = np.zeros((n, 37))
    s[:, 0:2] = rng.uniform(-1, 1, (n, 2)); s[:, 2] = rng.uniform(0.9, 1.5, n)
    s[:, 3:7] = _unit(rng, n, 4)
    s[:, 7:10] = rng.normal(size=(n, 3))
    s[:, 10:13] = _unit(rng, n, 3) * rng.uniform(0, 8, (n, 1))
    s[:, 13:25] = JLO + (JHI - JLO) * rng.uniform(0.02, 0.98, (n, 12))
    s[:, 25:37] = _unit(rng, n, 12) * rng.uniform(0, 20, (n, 1))
    fast = np.arange(n) % 10 == 3
    s[fast, 25 + rng.integers(0, 12, int(fast.sum()))] = float(cfg.vel_cap) * rng.choice([-1.0, 1.0], int(fast.sum())) * rng.uniform(1.01, 1.3, int(fast.sum()))
    tmax = np.tile(np.asarray(cfg.tau_max[:3], np.float64), 4)
    tau = np.clip(rng.uniform(-1, 1, (n, 12)) * TAU_FLIGHT, -tmax, tmax)
    return s, tau, np.zeros((n, 4)), rng.uniform(0.5, 1.0, n)


def gen_calm(rng, n, cfg):
    """flight with the legs near their stance angles: nothing for the self-collision rule's broad phase, so the common-path build stays (the
    quiet wave-mates of edges())"""
    s, tau, warm, mu = gen_flight(rng, n, cfg)
    s[:, 13:25] = np.tile([0.0, 0.8, -1.6], 4) + rng.uniform(-0.2, 0.2, (n, 12))
    return s, tau, warm, mu


FOOT_SETS = [(), (0,), (3,), (0, 3), (1, 2), (0, 2), (1, 3), (0, 1), (0, 1, 2), (1, 2, 3), (0, 1, 2, 3), (0, 1, 2, 3)]   # none, single, diagonal, same side, same end, three, all


def gen_stance(rng, n, cfg):
    """standing, tilted up to 0.15 rad: every count of touching feet from 0 to 4 (diagonal and same-side pairs among them), penetrations from
    0.2 to 2 mm or a gap inside the 0.727 mm contact range, the other feet 5 - 40 mm up; mu 0.5 - 1; warm start zero or not; hip torques and a
    sideways drift so that some feet slide and some stick"""
    s = np.zeros((n, 37))
    s[:, 0:2] = rng.uniform(-1, 1, (n, 2)); s[:, 2] = rng.uniform(0.25, 0.29, n)
    s[:, 3:7] = _euler_quat(rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n), rng.uniform(-math.pi, math.pi, n))
    s[:, 13:25:3] = rng.uniform(-0.15, 0.15, (n, 4)); s[:, 14:25:3] = rng.uniform(0.6, 1.0, (n, 4))
    touch = np.zeros((n, 4), bool)
    for i in range(n):
        touch[i, list(FOOT_SETS[i % len(FOOT_SETS)])] = True
    gap = rng.uniform(0, 1, (n, 4)) < 0.25
    target = np.where(touch, np.where(gap, rng.uniform(5e-5, THR_FOOT - 5e-5, (n, 4)), -rng.uniform(2e-4, 2e-3, (n, 4))), rng.uniform(5e-3, 4e-2, (n, 4)))
    lo, hi = np.full((n, 4), -2.6), np.full((n, 4), -0.9)       # the foot's height falls as the knee opens: bisect the calf angle
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        s[:, 15:25:3] = mid
        above = heights(s)["foot"] > target
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    s[:, 15:25:3] = 0.5 * (lo + hi)
    slide = (np.arange(n) // len(FOOT_SETS)) % 2 == 1
    s[:, 7:10] = rng.normal(size=(n, 3)) * 0.05
    s[slide, 7:9] += _unit(rng, int(slide.sum()), 2) * rng.uniform(0.05, 0.4, (int(slide.sum()), 1))
    s[:, 10:13] = rng.normal(size=(n, 3)) * 0.3
    s[:, 25:37] = rng.normal(size=(n, 12))
    tau = rng.normal(size=(n, 12)) * 5.0
    tau[:, 0::3] = rng.uniform(-15, 15, (n, 4)) * (rng.uniform(0, 1, (n, 4)) < 0.5)
    warm = np.where(touch & (rng.uniform(0, 1, (n, 1)) < 0.5), rng.uniform(0.0, 0.06, (n, 4)), 0.0) * (float(cfg.dt) / 1e-3)
    return s, tau, warm, rng.uniform(0.5, 1.0, n)


def gen_stops(rng, n, cfg):
    """in the air, one to three joints 2e-4 to 2e-2 rad beyond a stop (the full build's limit rows run, the common-path build gives up),
    torques partly driving them further in"""
    s, tau, warm, mu = gen_flight(rng, n, cfg)
    s[:, 13:25] = JLO + (JHI - JLO) * rng.uniform(0.1, 0.9, (n, 12))
    s[:, 25:37] = rng.normal(size=(n, 12)) * 3.0
    s[:, 10:13] = rng.normal(size=(n, 3))
    for i in range(n):
        for j in rng.choice(12, 1 + i % 3, replace=False):
            low = rng.uniform() < 0.5
            beyond = rng.uniform(2e-4, 2e-2)
            s[i, 13 + j] = JLO[j] - beyond if low else JHI[j] + beyond
            if rng.uniform() < 0.5:
                tau[i, j] = (-1 if low else 1) * rng.uniform(5, 30)
    return s, tau, warm, mu


def gen_fallen(rng, n, cfg, nose_down=True):
    """lying on a side, the back, the belly or nose-down (fallen_states of tests/test_gpu_round2.py with more attitudes), legs folded,
    dropped from 1 mm and left to come to rest on trunk, hips, thighs and calves (settle_fallen: a robot lowered until its lowest point
    touches rests on ONE point, which no lying robot does); then small velocities and torques"""
    s = np.zeros((n, 37))
    s[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    roll = rng.choice([0.0, 1.45, -1.45, 3.0, 0.7, -2.6], n)
    pitch = np.where((np.arange(n) % 6 == 5) & nose_down, rng.choice([-1.3, 1.3], n), 0.0) + rng.uniform(-0.5, 0.5, n)
    s[:, 3:7] = _euler_quat(roll, pitch, rng.uniform(-math.pi, math.pi, n))
    s[:, 13:25] = np.tile([0.0, 1.2, -2.2], 4) + rng.uniform(-0.2, 0.2, (n, 12))       # (-2.4 there: the floor then presses calves into their stop)
    s[:, 2] = 1e-3
    return s, rng.uniform(-1, 1, (n, 12)) * TAU_FLIGHT, np.zeros((n, 4)), rng.uniform(0.5, 1.0, n)      # (torques: see gen_flight)


SETTLE_STEPS = 300


def settle_fallen(cfg, s, params, rng):
    """the float64 oracle's SETTLE_STEPS substeps from the dropped states under a joint PD (40 N m / rad, 1 N m s / rad towards the drawn
    joint angles); then the robot is pressed 0.2 - 2 mm into the floor -- a robot at rest sits with every contact AT the depth where its
    row switches on (the contact slop), which is no place to compare roundings -- and given the velocities of a robot that stirs: N(0, 0.02
    m/s), N(0, 0.05 rad/s), joint rates N(0, 0.2 rad/s).  (Settling on until nobody moves was tried: a robot fully at rest has no sliding
    direction, and the friction rows of such draws put the host twin at 9 - 16 x the bound over absolute differences of 5e-5 m/s.)"""
    n = len(s)
    c2 = build_config(n_envs=n, **dict(BASE, friction_model="cone", self_collision=False, solver_residual_threshold=0.0))[0]
    c2.unit_inertia, c2.payload_soft = cfg.unit_inertia, 0
    o = Oracle(c2)
    try:
        o.set_state(s); o.set_params(5, params)
        q0 = s[:, 13:25].copy()
        for _ in range(SETTLE_STEPS):
            st = o.get_state()
            tau = np.clip(40.0 * (q0 - st[:, 13:25]) - 1.0 * st[:, 25:37], -20.0, 20.0)
            for i in range(n):
                o.phys_step(i, tau[i])
        out = o.get_state().astype(np.float64)
    finally:
        o.close()
    out[:, 2] -= rng.uniform(2e-4, 2e-3, n)
    out[:, 7:10] += rng.normal(size=(n, 3)) * 0.02
    out[:, 10:13] += rng.normal(size=(n, 3)) * 0.05
    out[:, 25:37] += rng.normal(size=(n, 12)) * 0.2
    out[:, 3:7] /= np.linalg.norm(out[:, 3:7], axis=1, keepdims=True)
    return out


def _drop(s, params, blocks_of):
    """fallen robots: lowered until the lowest candidate sits where its draw says (s[:, 2] holds the wanted height of the lowest point)"""
    want = s[:, 2].copy()
    s[:, 2] = 0.0
    h = heights(s, params[:, P_M_PAY], params[:, P_R_PAY:P_R_PAY + 3])
    low = np.minimum(np.minimum(h["foot"].min(axis=1), h["cand"].reshape(len(s), -1).min(axis=1)), h["calf_lo"].min(axis=1))
    low = np.fmin(low, h["payload"])
    s[:, 2] = want - low
    return s


def gen_parameters(rng, n, cfg):
    """flight, stance and fallen draws in turn under the mass randomizer's parameters; a third with a push pending (see pushes()).  The
    fallen ones lie on a side, the back (where the payload touches) or the belly: with the nose-down ones of gen_fallen among them -- after
    SETTLE_STEPS still balanced on two knees -- the host twin read 0.82 x the bound in this family, above TWIN_RATIO; the fallen family
    keeps them under every plain configuration."""
    parts = [gen_flight(rng, n, cfg), gen_stance(rng, n, cfg), gen_fallen(rng, n, cfg, nose_down=False)]
    pick = np.arange(n) % 3
    out = [np.where((pick == 0).reshape(-1, *[1] * (parts[0][k].ndim - 1)), parts[0][k], np.where((pick == 1).reshape(-1, *[1] * (parts[0][k].ndim - 1)), parts[1][k], parts[2][k]))
           for k in range(4)]
    return out[0], out[1], out[2], out[3], pick == 2


def pushes(rng, n):
    """[n, 8]: every third environment pushed at the trunk, world and link frame in turn, 1 - 10 substeps left"""
    p = np.zeros((n, 8), np.float32)
    on = np.arange(n) % 3 == 1
    p[:, 0:3] = rng.normal(size=(n, 3)) * 60.0
    p[:, 3:6] = rng.normal(size=(n, 3)) * 6.0
    p[:, 6] = np.where(on, rng.integers(1, 11, n), 0)
    p[:, 7] = 1 + (np.arange(n) // 3) % 2
    p[~on, :6] = 0.0
    return p


GENERATORS = dict(calm=gen_calm, flight=gen_flight, stance=gen_stance, stops=gen_stops, fallen=gen_fallen, parameters=gen_parameters)
SEEDS = dict(calm=100, flight=101, stance=102, stops=103, fallen=104, parameters=105)


# ---------------------------------------------------------------- oracle runs
def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def oracle_substep(cfg, precision, states, params, warm, tau, push=None, contacts=False):
    """the oracle's phys_step of every environment from (states, params, warm, push): dict of state [n, 37], foot_force, foot_contact [n, 4],
    warm [n, 4] (the normal impulse: force x dt), n_invalid [n], block [n, 13] or None; contacts: per environment the (body b, link a, link b)
    of its contact list"""
    n = len(states)
    o = Oracle(cfg, precision)
    try:
        o.set_state(states); o.set_params(5, params); o.set_warm(warm)
        if push is not None:
            for frame in (1, 2):
                m = (push[:, 7] == frame) & (push[:, 6] > 0)
                if m.any():
                    o.set_external_wrench(push[:, :6], push[:, 6].astype(np.int32), frame, m)
        lists = []
        for i in range(n):
            o.phys_step(i, tau[i])
            if contacts:
                lists.append([(b, la, lb) for (_, b, la, lb, _, _) in o.contacts(i)])
        ff = o.get_info(0).astype(np.float64)
        blk = None
        if cfg.payload_soft:
            b = o.block()
            blk = np.concatenate([b["pos"], b["quat"], b["v"], b["w"]], 1).astype(np.float64)
        return dict(state=o.get_state().astype(np.float64), foot_force=ff, foot_contact=o.get_info(1).astype(np.float64), warm=ff * float(cfg.dt),
                    n_invalid=o.get_info(5)[:, 0].astype(np.float64), block=blk, contacts=lists)
    finally:
        o.close()


def from_records(cfg, rec, ret=None):
    """the same dict from records after a substep (the device's or the twin's)"""
    rec = np.asarray(rec, np.float64)
    return dict(state=rec[:, R_POS:R_POS + 37], foot_force=rec[:, R_FOOT_FORCE:R_FOOT_FORCE + 4], foot_contact=rec[:, R_FOOT_CONTACT:R_FOOT_CONTACT + 4],
                warm=rec[:, R_WARM:R_WARM + 4], n_invalid=rec[:, R_N_INVALID], block=rec[:, R_BLOCK:R_BLOCK + 13] if cfg.payload_soft else None, ret=ret)


def make_records(cfg, states, params_edit, warm):
    """records of an Emu of cfg in `states`: the handle's own parameter draws, edited by params_edit(params [n, 24]), the payload block placed
    where its constraint wants it, the warm start set.  -> (records [n, QS_REC] float32, params float64)"""
    e = E.Emu(cfg)
    rec = e.records()
    params_edit(rec[:, R_PARAMS:R_PARAMS + 24])
    e.set_state(states)
    rec[:, R_WARM:R_WARM + 4] = warm
    return rec.copy(), rec[:, R_PARAMS:R_PARAMS + 24].astype(np.float64)


class Case:
    """a family's kept draws under one configuration: cfg, records, tau, push, the two oracles' results, what was rejected"""


@functools.lru_cache(maxsize=None)
def family(name, config_name):
    """N_DRAWS draws of the family, those clear of every switch (in float64 alone) kept in order, the first N_FAMILY of them the case"""
    rng = np.random.default_rng(SEEDS[name] + 1000 * list(CONFIGS).index(config_name))
    cfg = config(config_name, N_DRAWS)
    g = GENERATORS[name](rng, N_DRAWS, cfg)
    s, tau, warm, mu = (_f32(x) for x in g[:4])
    s[:, 3:7] /= np.linalg.norm(s[:, 3:7], axis=1, keepdims=True); s = _f32(s)
    masses = bool(cfg.randomizer_flags & 2)

    def edit(p):
        if not masses:      # (the mass randomizer's handles draw mu as well)
            p[:, P_MU] = mu
    lying = g[4] if name == "parameters" else np.full(N_DRAWS, name == "fallen")
    rec, params = make_records(cfg, s, edit, warm)
    if lying.any():
        s[lying] = _f32(settle_fallen(cfg, _drop(s[lying], params[lying], None), params[lying], rng))
        s[:, 3:7] /= np.linalg.norm(s[:, 3:7], axis=1, keepdims=True); s = _f32(s)
        rec, params = make_records(cfg, s, edit, warm)
    push = pushes(rng, N_DRAWS) if name == "parameters" else None
    blocks = rec[:, R_BLOCK:R_BLOCK + 20].astype(np.float64) if cfg.payload_soft else None
    h = heights(s, params[:, P_M_PAY], params[:, P_R_PAY:P_R_PAY + 3], blocks)
    o64 = oracle_substep(cfg, "f64", s, params, warm, tau, push, contacts=True)
    why = dict(ground=ground_clearance(h, float(cfg.contact_slop)) <= MARGIN)
    jc = joint_clearance(s)
    why["joint"] = (jc <= MARGIN) if name != "stops" else (jc <= 1e-4)          # (stops: every joint clearly past a stop or clearly inside)
    clear = ~(why["ground"] | why["joint"])
    # heights() against the oracle's own list: the links on the plane
    want = ground_links(h)
    got = [set((la if la >= 0 else -1) for (bb, la, lb) in c if bb == 0) for c in o64["contacts"]]
    mismatch = [i for i in range(N_DRAWS) if clear[i] and want[i] != got[i]]
    assert not mismatch, f"{name} / {config_name}: heights() and the float64 oracle's contact list disagree in draws {mismatch[:5]}: {want[mismatch[0]]} against {got[mismatch[0]]}"
    if cfg.self_collision:      # link-link contacts: the oracle's list under joint displacements that move the links by more than MARGIN
        base = [sorted((la, lb) for (bb, la, lb) in c if bb == 1) for c in o64["contacts"]]
        for _ in range(4):
            sp = s.copy()
            sp[:, 13:25] += rng.choice([-1.0, 1.0], (N_DRAWS, 12)) * 1e-4
            alt = oracle_substep(cfg, "f64", sp, params, warm, tau, push, contacts=True)["contacts"]
            same = np.array([base[i] == sorted((la, lb) for (bb, la, lb) in alt[i] if bb == 1) for i in range(N_DRAWS)])
            why["self"] = why.get("self", np.zeros(N_DRAWS, bool)) | ~same
            clear &= same
    keep = np.flatnonzero(clear)[:N_FAMILY]
    c = Case()
    c.name, c.config_name, c.rejected, c.draws = name, config_name, int((~clear).sum()), N_DRAWS
    c.kept, c.rejected_by = len(keep), {k: int(v.sum()) for k, v in why.items()}
    c.cfg = config(config_name, len(keep))
    c.rec, c.tau, c.push = rec[keep], tau[keep].astype(np.float32), None if push is None else push[keep]
    c.states, c.params, c.warm = s[keep], params[keep], warm[keep]
    c.o64 = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in o64.items() if k != "contacts"}
    c.o32 = oracle_substep(c.cfg, "f32", c.states, c.params, c.warm, c.tau.astype(np.float64), c.push)
    c.self_contacts = np.array([sum(1 for (bb, la, lb) in o64["contacts"][i] if bb == 1) for i in keep])
    return c


@functools.lru_cache(maxsize=None)
def edges(config_name):
    """48 environments: wave 0 = a standing robot in slot 0 among fifteen in calm flight; wave 1 = a fallen one in slot 15 among fifteen in
    calm flight; wave 2 = every family in turn, the same standing robot in slot 5 and the same fallen one in slot 9 (case.twice: the pairs
    of environments with the same input).  Taken from the families' kept draws (their margins hold)."""
    masses = CONFIGS[config_name].get("env_randomizer_mode") == "MASS_RANDOMIZER"
    fams = {k: (family("parameters", config_name) if masses and k != "calm" else family(k, config_name)) for k in FAMILIES + ["calm"]}

    def rows(k, count, start=0):
        f = fams[k]
        if masses and k != "calm":      # the parameters family holds flight, stance and fallen draws: pick by what the float64 oracle saw
            feet, links = f.o64["foot_contact"].sum(axis=1), f.o64["n_invalid"]
            idx = np.flatnonzero({"flight": (feet == 0) & (links == 0), "stops": (feet == 0) & (links == 0), "fallen": links > 0, "stance": (feet > 1) & (links == 0)}[k])
        elif k == "fallen":             # (a robot that came to rest on its folded legs' feet alone is a standing one)
            idx = np.flatnonzero(f.o64["n_invalid"] > 0)
        else:
            idx = np.arange(f.kept)
        return [(f, int(i)) for i in idx[start:start + count]]
    stand, lie = rows("stance", 1, 10)[0], rows("fallen", 1, 3)[0]
    w0 = [stand] + rows("calm", 15)
    w1 = rows("calm", 15, 15) + [lie]
    w2 = [rows(FAMILIES[k % 4], 1, 20 + k // 4)[0] for k in range(16)]
    w2[5], w2[9] = stand, lie
    pick = w0 + w1 + w2
    c = Case()
    c.name, c.config_name, c.rejected, c.draws, c.kept = "edges", config_name, 0, len(pick), len(pick)
    c.cfg = config(config_name, len(pick))
    take = lambda attr: np.stack([getattr(f, attr)[i] for f, i in pick])
    c.rec, c.tau, c.states, c.params, c.warm = take("rec"), take("tau"), take("states"), take("params"), take("warm")
    c.push = np.stack([f.push[i] if f.push is not None else np.zeros(8, np.float32) for f, i in pick]) if any(f.push is not None for f, _ in pick) else None
    c.o64 = oracle_substep(c.cfg, "f64", c.states, c.params, c.warm, c.tau.astype(np.float64), c.push)
    c.o32 = oracle_substep(c.cfg, "f32", c.states, c.params, c.warm, c.tau.astype(np.float64), c.push)
    c.twice = ((0, 32 + 5), (31, 32 + 9))
    return c


# ---------------------------------------------------------------- bounds
GROUPS = (("position", "state", 0, 3, 0.0), ("quaternion", "state", 3, 7, 0.0), ("linear_velocity", "state", 7, 10, 0.0), ("angular_velocity", "state", 10, 13, 0.0),
          ("q", "state", 13, 25, 0.0), ("qd", "state", 25, 37, 0.0), ("foot_force", "foot_force", 0, 4, Y.EXTRA_RTOL["foot_force"]), ("warm", "warm", 0, 4, Y.EXTRA_RTOL["foot_force"]),
          ("block_pose", "block", 0, 7, 0.0), ("block_velocity", "block", 7, 13, 0.0))


def group_errors(a, b):
    """{group: [n] the largest |a - b| inside the group}, for two result dicts"""
    out = {}
    for g, field, lo, hi, _ in GROUPS:
        if a.get(field) is not None and b.get(field) is not None:
            out[g] = np.abs(np.asarray(a[field], np.float64)[:, lo:hi] - np.asarray(b[field], np.float64)[:, lo:hi]).max(axis=1)
    return out


def bounds(case):
    """{group: [n]} FACTOR x max(own_i, P99 of own over the case) + the group's relative term x the float64 value's size, own = |oracle32 -
    oracle64|: the project's allowance for another rounding of the same step, from the reference alone"""
    own = group_errors(case.o32, case.o64)
    out = {}
    for g, field, lo, hi, rtol in GROUPS:
        if g in own:
            ref = np.abs(np.asarray(case.o64[field], np.float64)[:, lo:hi]).max(axis=1)
            out[g] = Y.FACTOR * np.maximum(own[g], np.percentile(own[g], 99)) + rtol * ref
    return out


def ratios(case, got, ref=None, rows=None):
    """{group: (worst |got - ref| / bound, environment, |d|, bound)}; ref: default the float64 oracle; a zero bound holds a zero error only"""
    ref = ref or case.o64
    err, b = group_errors(got, ref), bounds(case)
    out = {}
    for g in err:
        e_, b_ = (err[g], b[g]) if rows is None else (err[g][rows], b[g][rows])
        if not len(e_):
            continue
        r = np.where(e_ == 0, 0.0, e_ / np.maximum(b_, 1e-300))
        i = int(np.argmax(r))
        out[g] = (float(r[i]), i if rows is None else int(np.flatnonzero(rows)[i] if np.asarray(rows).dtype == bool else np.asarray(rows)[i]), float(e_[i]), float(b_[i]))
    return out


def quantiles(case, got):
    """{group: dict(device = p50 / p90 / p99 / max of |got - oracle64|, oracle32 = the same of the oracle's own)}: recorded, not asserted"""
    err, own = group_errors(got, case.o64), group_errors(case.o32, case.o64)
    q = lambda x: [float(v) for v in np.percentile(x, [50, 90, 99])] + [float(np.max(x))]
    return {g: dict(device=q(err[g]), oracle32=q(own[g])) for g in err}


def fold_waves(ret):
    """what a wave of 16 returns where each environment alone returns `ret`: the votes are wave-wide -- 1 if any gives up, else 2 if any
    foresees it, else 0"""
    r = np.asarray(ret).reshape(-1, 16)
    w = np.where((r == 1).any(axis=1), 1, np.where((r == 2).any(axis=1), 2, 0))
    return np.repeat(w, 16)


def bits(x):
    """float32 bit patterns with -0 as +0"""
    return (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)


STATE_COLS = np.r_[R_POS:R_POS + 37, R_WARM:R_WARM + 4]


# ---------------------------------------------------------------- what the CPU and the GPU tests both check
OUT_COLS = np.r_[R_POS:R_POS + 37, R_WARM:R_WARM + 4, R_FOOT_FORCE:R_FOOT_FORCE + 4, R_FOOT_CONTACT:R_FOOT_CONTACT + 4, R_N_INVALID:R_N_INVALID + 1]


def out_cols(cfg):
    """the record's columns a substep writes: state, warm start, foot force, foot contact, n_invalid, and the payload block where there is one"""
    return np.r_[OUT_COLS, R_BLOCK:R_BLOCK + 20] if cfg.payload_soft else OUT_COLS


def kept_cols(cfg):
    """what a common-path build that gives up hands back as it came: state, warm start, the payload block"""
    return np.r_[STATE_COLS, R_BLOCK:R_BLOCK + 20] if cfg.payload_soft else STATE_COLS


def check_against_oracle(case, got, label, limit=1.0, rows=None):
    """a full build's (or, on `rows`, a finished common-path build's) result against the float64 oracle: every group inside limit x its
    bound, contact flags and invalid-contact counts equal"""
    r = ratios(case, got, rows=rows)
    bad = {g: v for g, v in r.items() if v[0] > limit}
    assert not bad, f"{label}: group -> (|result - oracle64| / bound, environment, |d|, bound) {bad}"
    m = slice(None) if rows is None else rows
    assert np.array_equal(got["foot_contact"][m], case.o64["foot_contact"][m]), f"{label}: foot contact flags"
    assert np.array_equal(got["n_invalid"][m], case.o64["n_invalid"][m]), f"{label}: invalid contacts {np.flatnonzero(got['n_invalid'] != case.o64['n_invalid'])[:8].tolist()}"
    return r


def check_common_path(case, rec_hot, ret_hot, rec_full, expect_ret, bitwise, label):
    """a common-path build's records and return values: the return values are `expect_ret`; where it gave up (1) state, warm start and block
    are the input's bit for bit; where it finished (0, 2) its result is the full build's `rec_full` -- bit for bit on the rows of `bitwise`
    ([n] bool), inside the bound (as a second rounding of the oracle's step) on the others"""
    assert np.array_equal(ret_hot, expect_ret), f"{label}: substep returned {ret_hot.tolist()} where {np.asarray(expect_ret).tolist()} is due"
    gave_up = ret_hot == 1
    kc, oc = kept_cols(case.cfg), out_cols(case.cfg)
    assert np.array_equal(bits(rec_hot[gave_up][:, kc]), bits(case.rec[gave_up][:, kc])), f"{label}: a build that gives up leaves the state as it found it"
    done = ~gave_up
    same = (bits(rec_hot[:, oc]) == bits(rec_full[:, oc])).all(axis=1)
    off = np.flatnonzero(done & bitwise & ~same)
    assert not len(off), f"{label}: common-path and full build differ in environments {off[:8].tolist()}"
    rest = done & ~bitwise
    if rest.any():
        check_against_oracle(case, from_records(case.cfg, rec_hot), label + " (finished rows)", rows=rest)
    return dict(gave_up=int(gave_up.sum()), finished=int(done.sum()), foresaw=int((ret_hot == 2).sum()), bitwise_equal_to_full=int((done & same).sum()))
