/*
 * qs_amd.h -- C ABI of the MI355X-native batched Go1 + PEA simulation step.
 *
 * This is the drop-in boundary for the hot path of francescovezzi/quadruped-springs.  The reference has no FFI:
 * the path sits behind the Python class QuadrupedGymEnv, so every entry point names the Python-level interface
 * it replaces (paths relative to the reference's quadruped_spring/ package):
 *
 *   qs_create      QuadrupedGymEnv.__init__                      env/quadruped_gym_env.py:52-155
 *   qs_reset       QuadrupedGymEnv.reset (+ randomizers, settle)  env/quadruped_gym_env.py:278-329,
 *                                                                 env/env_randomizers/env_randomizer.py:19-122,279-291
 *   qs_step        QuadrupedGymEnv.step for N environments        env/quadruped_gym_env.py:227-256
 *                  (filter, action map, ApplyAction = PD + PEA,   utils/action_filter.py:110-121,
 *                   stepSimulation x action_repeat, task,          env/quadruped.py:288-320, env/quadruped_motor.py:45-104,
 *                   reward, termination, sensors)                  env/springs.py:28-74, env/tasks/, env/sensors/
 *   qs_get_obs     QuadrupedGymEnv.get_observation                env/quadruped_gym_env.py:343-345
 *   qs_get_state / qs_set_state    Quadruped state getters / reset_desired_state   env/quadruped.py:107-207, 521-525
 *   qs_get_info    GetContactInfo, GetMotorTorques, task scalars  env/quadruped.py:209-258, env/tasks/task_base.py:44-59
 *   qs_set_params  set_spring_stiffness/damping, changeDynamics(lateralFriction), kp/kd swaps of the landing wrappers
 *                                                                 env/quadruped.py:732-742, env/wrappers/landing_wrapper.py:22-30
 *   qs_render      QuadrupedGymEnv.render(mode="rgb_array")      env/quadruped_gym_env.py:334-335, utils/camera.py:35-59
 *   qs_policy_act  model.predict(obs, deterministic=...)          load_model.py:132 (SB3 BasePolicy.predict; sb3_contrib ARS.evaluate_candidates)
 *
 * Conventions
 *   - plain pointers and sizes only; all array arguments are DEVICE pointers (HIP) owned by the caller, row-major,
 *     float32 unless stated; the handle owns the persistent per-environment records.
 *   - returns 0 on success, a negative code on failure with text in qs_last_error(); never throws.
 *   - a handle is driven by one host thread; work is enqueued on the stream given to qs_set_stream (default: the
 *     null stream) and is asynchronous with respect to the host.  Handles are independent (one per GPU rank).
 *   - there is no CPU fallback: qs_create fails if no HIP device is usable.
 */
#ifndef QS_AMD_H
#define QS_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { QS_ACT_DEFAULT = 0, QS_ACT_SYMMETRIC = 1, QS_ACT_SYMMETRIC_NO_HIP = 2, QS_ACT_CPG = 3 /* build extension */ };  /* control_interface/collection.py:49 */
enum { QS_MOTOR_PD = 0, QS_MOTOR_CARTESIAN_PD = 1, QS_MOTOR_TORQUE = 2 };       /* control_interface/collection.py:33 */
enum {                                                                          /* tasks/task_collection.py:19-37 */
    QS_TASK_NO_TASK = 0, QS_TASK_JUMPING_IN_PLACE = 1, QS_TASK_JUMPING_FORWARD = 2,
    QS_TASK_CONT_JUMPING_FORWARD = 3, QS_TASK_CONT_JUMPING_FORWARD2 = 4,
    QS_TASK_JUMPING_IN_PLACE_PPO = 5, QS_TASK_JUMPING_FORWARD_PPO = 6, QS_TASK_BACKFLIP = 7,
    QS_TASK_JUMPING_IN_PLACE_PPO_HP = 8, QS_TASK_JUMPING_FORWARD_PPO_HP = 9, QS_TASK_BACKFLIP_PPO = 10,
    QS_TASK_CONT_JUMPING_FORWARD3 = 11, QS_TASK_CONT_JUMPING_FORWARD_PPO = 12,
    /* imitation tasks (TaskJumpingDemo task_base.py:169-220, TaskJumpingDemo2 :402-453; robot_tasks.py:222-247): the rows come
     * through qs_set_demo, not from the demonstrations/<name>.npy files the reference loads (its repository does not hold them) */
    QS_TASK_JUMPING_IN_PLACE_DEMO = 13, QS_TASK_JUMPING_FORWARD_DEMO = 14, QS_TASK_BACKFLIP_DEMO = 15,
    QS_TASK_CONT_JUMPING_FORWARD_DEMO = 16,
};
enum {                                                                          /* sensors/robot_sensors.py */
    QS_SENS_JOINT_POS = 0, QS_SENS_JOINT_VEL = 1, QS_SENS_PITCH = 2, QS_SENS_HEIGHT = 3, QS_SENS_VEL_Z = 4,
    QS_SENS_LANDING = 5, QS_SENS_JUMPING = 6, QS_SENS_PITCH_RATE = 7, QS_SENS_VEL_X = 8, QS_SENS_BOOL_CONTACT = 9,
    QS_SENS_LIN_VEL = 10, QS_SENS_ANG_VEL = 11, QS_SENS_FEET_POS = 12, QS_SENS_FEET_VEL = 13,
    QS_SENS_PITCH_BACKFLIP = 14, QS_SENS_RPY = 15, QS_SENS_QUAT = 16,
};
#define QS_RAND_GROUND 1   /* env_randomizer.py:279-291 */
#define QS_RAND_MASSES 2   /* env_randomizer.py:19-83 */
#define QS_RAND_SPRINGS 4  /* env_randomizer.py:86-122 */
#define QS_RAND_KEEP 8     /* reset keeps the parameters last written by qs_set_params */
enum { QS_WRAP_NONE = 0, QS_WRAP_LANDING = 1, QS_WRAP_GO_TO_REST = 2, QS_WRAP_LANDING2 = 3, QS_WRAP_LANDING_BACKFLIP = 4,
       QS_WRAP_LANDING_BACKFLIP2 = 5, QS_WRAP_LANDING_CONTINUOUS = 6 };
enum { QS_PHASE_POLICY = 0, QS_PHASE_TAKEOFF = 1, QS_PHASE_LANDING = 2, QS_PHASE_REST = 3 };

#define QS_MAX_SENSORS 16
#define QS_MAX_OBS 64
#define QS_STATE_DIM 37    /* pos3 quat4(xyzw) vlin3 vang3 q12 qd12 */
#define QS_PARAM_DIM 24    /* mu, k3, b3, rest3, kp3, kd3, m_trunk, m_leg3, m_payload, r_payload3 */
#define QS_TASK_DIM 48
#define QS_TRACE_DIM 70 /* floats per substep row of the trace tap, see qs_set_trace */    /* 32 task scalars, pose cache 9 (pos, vel, rpy), n_invalid, foot-force sum, sim_step, 4 spare */

/* Keyword arguments of QuadrupedGymEnv.__init__ (gym_env.py:52-70) resolved to numbers by the host
 * (quadruped-springs_amd/qs_amd/config.py); constants come from go1/configs_go1_*.py. */
typedef struct qs_config {
    int32_t n_envs;
    int32_t action_dim;          /* 12 / 6 / 4 (action_interface.py:12,27,56); 5 for the CPG layer */
    int32_t action_space_mode;
    int32_t motor_control_mode;
    int32_t symm_idx;            /* motor_interface.py:15,56 */
    int32_t rl_interface;        /* isRLGymInterface */
    int32_t task;
    int32_t n_sensors;
    int32_t sensors[QS_MAX_SENSORS];
    int32_t obs_dim;
    int32_t enable_springs;
    int32_t enable_filter;
    int32_t enable_interp;
    int32_t action_repeat;
    int32_t solver_iters;        /* int(300 / action_repeat), gym_env.py:113 */
    int32_t settle_steps;        /* 2500, gym_env.py:115 */
    int32_t max_sim_steps;       /* truncation when sim_step_counter > max_sim_steps (sim time > 10 s, gym_env.py:245) */
    int32_t randomizer_flags;
    int32_t noise_enabled;
    int32_t auto_reset;          /* SB3 VecEnv convention: finished environments are reset inside qs_step */
    int32_t reset_lookahead;     /* K: reset states kept ready per environment.  A reset's settled state depends on (seed, global environment
                                  * id, episode number) only, so the states of an environment's next K episodes are computed ahead of
                                  * time -- at qs_create for episodes 0 .. K-1, then one per reset by extra workgroups of the step kernel
                                  * (qs_settle_lanes) -- and a reset copies its own.  0: every reset runs the 2500-substep settle in place.
                                  * Either way the results are bitwise the same; K only decides when the settle work is done.  A reset
                                  * whose state is not ready (K consecutive episodes shorter than one settle) settles in place and is
                                  * counted (QS_COUNTER_RESET_STALLS).  Ignored under QS_RAND_KEEP.  N x K x 1152 bytes. */
    int32_t env_id_offset;       /* global id of environment 0 (sharded runs): RNG streams are keyed by the global id */
    int32_t wrapper_mode;        /* QS_WRAP_*: none, or one of the reference's six landing / go-to-rest wrappers as a per-environment phase machine */
    uint64_t seed;
    double dt;
    double filt_b[3], filt_a[3]; /* scipy.signal.butter(2, 3 Hz) at 1/env_dt, action_filter.py:191-213 */
    float gravity;
    float kp[3], kd[3], tau_max[3];
    float cmd_lo[12], cmd_hi[12];
    float settle_cmd[12];
    float settle_action[12];
    float spring_k[3], spring_b[3], spring_rest[3];
    float fallen_height;
    float leg_len[3];
    float contact_erp, joint_erp, warmstart, vel_cap;
    float obs_noise_std[QS_MAX_OBS];
    float task_p[16];
    float contact_slop;        /* btContactSolverInfo::m_linearSlop (PhysicsServerCommandProcessor sets 1e-5): added to a contact's distance
                                * before the positional / speculative error terms of its normal row */
    int32_t body_contacts;     /* 1: trunk / hip / thigh / calf primitives that touch the plane push back (normal + friction rows in the
                                * many-rows solve, at most two support points per leg); 0: they only count as invalid contacts (quadruped.py:243-249) */
    int32_t self_collision;    /* 1: link-link contacts that involve a calf are detected and counted as invalid contacts
                                * (URDF_USE_SELF_COLLISION quadruped.py:533-539, rule :237-241); 0: no link-link test */
    int32_t info_fields;       /* 1: every step also writes the info block of the records (foot forces and flags, motor and spring torque, the
                                * task's pose cache: what QS_INFO_FOOT_FORCE / _FOOT_CONTACT / _TORQUE / _SPRING_TORQUE and the cache slots of
                                * QS_INFO_TASK return); 0: a learner that reads observations, rewards and done flags only skips those stores,
                                * and the getters fail */
    int32_t payload_soft;      /* 0: the payload block of the mass randomizer is welded to the trunk (the default: same motion to micrometres,
                                * tests/test_body_contacts.py, and the common-path kernel); 1: a second body held by a six-row fixed constraint
                                * in the same PGS, as the reference builds it (quadruped.py:796-819): under the implicit cone its rows ride
                                * with the foot rows in the common-path solver (about 3x the step time: the constraint's rows need all the
                                * sweeps), under the friction pyramid every substep takes the many-rows solve; its state: QS_INFO_PAYLOAD_BLOCK */
    float support_margin;      /* m/s.  body_contacts: a non-foot support point inside its contact range gets its rows once its normal row comes this
                                * close to acting on the substep's predicted velocities (a point still approaching has speculative rows that end
                                * every sweep at zero impulse: the same solve at the many-rows price); >= 1e30: EVERY point in range
                                * gets its rows, as Bullet and the oracle build them (parity / debug runs).  Default 0.5. */
    float reserved_f[2];
    /* Hopf-oscillator CPG action layer (hopf_network.py:26-173); BASELINE.json configs[4] */
    float cpg_phi[16];         /* coupling phase matrix PHI[i][j] of the gait (hopf_network.py:74-115) */
    float cpg_lo[5], cpg_hi[5];/* action -> (omega_swing, omega_stance, mu, des_step_len, robot_height) */
    float cpg_clearance, cpg_penetration, cpg_coupling, cpg_alpha;  /* :42-43, :35, :142 */
    float solver_residual_threshold; /* PyBullet setPhysicsEngineParameter(solverResidualThreshold): a sweep whose largest
                                      * squared velocity change is <= this ends the solve; 0 = always `solver_iters` sweeps */
    int32_t friction_cone;     /* 0: friction pyramid, each direction clamped on its own and left alone while its normal impulse is zero
                                * (btMultiBodyConstraintSolver::solveSingleIteration without implicit cone friction); 1: the two friction
                                * rows of a contact are updated together and projected onto the disc of radius mu x normal impulse
                                * (resolveConeFrictionConstraintRows, PyBullet's enableConeFriction) */
    /* scripted phases of env/wrappers/landing_wrapper.py:18-69 and go_to_rest_wrapper.py:22-95 */
    float landing_action[12];  /* get_landing_action(), gym_env.py:375-379 */
    float landing_kp, landing_kd; /* landing_wrapper.py:22-27 */
    float rest_kp, rest_kd, rest_time; /* go_to_rest_wrapper.py:16-19, 26-32 */
    float reserved_h[3];
    /* Inertia tensors about the centre of mass PER UNIT MASS (xx, xy, xz, yy, yz, zz; link axes, sign convention of the FR leg) of
     * hip, thigh, calf and trunk: a link of mass m has the tensor m * unit_inertia.  mass_inertia_rule = "scale": the URDF tensor over the
     * URDF mass.  "collision_shape": what Bullet's changeDynamics(mass=...) (quadruped.py:761,776) leaves behind -- the box inertia of the
     * collision compound's AABB in the link's principal frame.  The host fills the table (qs_amd/config.py). */
    float unit_inertia[4][6];
} qs_config;

typedef struct qs_handle qs_handle;

int qs_create(const qs_config* cfg, int device, qs_handle** out);
/* The rack (Quadruped(on_rack=True), quadruped.py:86-96, 474-484): createConstraint(robot, -1, -1, -1, JOINT_FIXED, [0,0,0], [0,0,0],
 * anchor_pos, childFrameOrientation = anchor_quat) -- the base origin held at anchor_pos with the base frame parallel to anchor_quat (xyzw)
 * by six rows in the same PGS as the contacts: three on the pivot along the world axes, three on the frames' relative rotation; ERP
 * cfg.joint_erp, impulse bound 500 N x dt, swept after the joint-limit rows and before the contacts, as the payload block's fixed constraint
 * (cfg.payload_soft) with the world in the place of the block.  on = 1: every reset spawns the robot at the anchor pose and settles it hung
 * there (look-ahead reset states included); a handle created with on = 0 (or through qs_create) has no rack.  Refused together with
 * cfg.payload_soft.  Under the friction pyramid every substep of a wave with a hung robot runs in the full build. */
typedef struct qs_rack {
    int32_t on;
    float anchor_pos[3];
    float anchor_quat[4];   /* xyzw; normalised by qs_create_ex, which refuses a zero or non-finite one */
} qs_rack;
/* qs_create with an optional rack (NULL: none; qs_create(cfg, dev, out) = qs_create_ex(cfg, NULL, dev, out)) */
int qs_create_ex(const qs_config* cfg, const qs_rack* rack, int device, qs_handle** out);
/* Releases (hung = 0) or hangs again (hung = 1) the masked environments (mask: device pointer to n_envs bytes, NULL = all) for the rest of
 * their current episode: a reset always hangs the robot again (so the look-ahead reset states never depend on this call).  Re-hanging
 * pulls the base back to the anchor at the ERP rate, within the impulse bound.  Stream-ordered, no host synchronisation.  Fails on a handle
 * without a rack. */
int qs_set_rack(qs_handle* h, const uint8_t* mask, int hung);
void qs_destroy(qs_handle* h);
int qs_set_stream(qs_handle* h, void* hip_stream);
/* mask: device pointer to n_envs bytes, or NULL for all environments */
int qs_reset(qs_handle* h, const uint8_t* mask);
/* Reference-state initialisation (reference_state_initialization_wrapper.py:25-43 -> set_robot_desired_state, quadruped.py:521-525,
 * gym_env.py:289-290): reset of the masked environments that runs the randomizers, places the robot at states[env] ([N,37], layout of
 * qs_get_state) instead of spawning and settling it, then resets task, sensors and filter as every reset does. */
int qs_reset_to(qs_handle* h, const uint8_t* mask, const float* states);
int qs_get_obs(qs_handle* h, float* obs /*[N,obs_dim]*/);
/* The demonstration of the DEMO tasks: rows[length][action_dim + 38] (device memory; copied) in the layout
 * GetDemonstrationWrapper._get_demo records (get_demonstration_wrapper.py:35-58: filtered action, q 12, qd 12, base position 3,
 * quaternion 4, linear velocity 3, angular velocity 3, landing flag).  Replaces `np.load(self.demo_path)` (task_base.py:173);
 * qs_step fails for a DEMO task until it was called.  Row `demo counter` is compared with the action of each step; the counter
 * and its value at the start of the episode are slots 44 and 45 of QS_INFO_TASK. */
int qs_set_demo(qs_handle* h, const float* rows, int length);
/* task.set_demo_counter(value) (task_base.py:219-220) for the masked environments (mask NULL = all), as
 * ReferenceStateInitializationWrapper.reset does after set_robot_desired_state (reference_state_initialization_wrapper.py:25-33):
 * call it after qs_reset_to.  values[N] int32, device memory. */
int qs_set_demo_counter(qs_handle* h, const uint8_t* mask, const int32_t* values);
int qs_step(qs_handle* h, const float* actions /*[N,action_dim]*/, float* obs /*[N,obs_dim]*/, float* rew /*[N]*/,
            uint8_t* done /*[N]*/, uint8_t* truncated /*[N]*/);
int qs_get_state(qs_handle* h, float* state /*[N,37]*/);
/* A push on the trunk (Quadruped.apply_external_force, quadruped.py:338-343: pybullet.applyExternalForce on link 0 at its centre of mass):
 * force F and torque tau, acting at the trunk's centre of mass (its inertial origin), on the next `substeps` physics substeps each masked
 * environment steps -- counted on the device, across env-step boundaries.  QS_FRAME_WORLD: the vectors are fixed in the world frame;
 * QS_FRAME_LINK: fixed to the trunk, turning with it.  Setting a push again replaces the earlier one; substeps = 0 cancels it; a reset of the
 * environment (auto-reset in a step, qs_reset, qs_reset_to) cancels it, and so does the step in which its episode ends (with or without auto-reset: the
 * environment has to be reset before it steps again); qs_set_state keeps it; settles never see it.  pybullet clears external
 * forces after every stepSimulation: the reference's apply_external_force is substeps = 1, QS_FRAME_LINK, tau = 0.
 * Device pointers, stream-ordered, no host synchronisation: mask NULL = every environment, wrench [N,6] (F, tau), substeps [N].  Fails for an
 * unknown frame.  A selected row with a negative duration or a non-finite value is not taken (the environment keeps its push); as checking
 * device data here would synchronise, the refusal is reported by the next qs_stats or qs_counter (which wait for the device anyway): it
 * fails once, naming the first refused environment. */
enum { QS_FRAME_LINK = 1, QS_FRAME_WORLD = 2 };   /* pybullet.LINK_FRAME / WORLD_FRAME */
int qs_set_external_wrench(qs_handle* h, const uint8_t* mask, const float* wrench /*[N,6]: F, tau*/, const int32_t* substeps /*[N]*/, int frame);
int qs_set_state(qs_handle* h, const float* state /*[N,37]*/);
enum {
    QS_INFO_FOOT_FORCE = 0, QS_INFO_FOOT_CONTACT = 1, QS_INFO_TORQUE = 2, QS_INFO_SPRING_TORQUE = 3, QS_INFO_TASK = 4,
    QS_INFO_N_INVALID = 5, QS_INFO_PARAMS = 6, QS_INFO_COUNTERS = 7, QS_INFO_LAST_ACTION = 8, QS_INFO_TERMINAL_OBS = 9,
    QS_INFO_FILTERED_ACTION = 11,  /* [N,12]: output of the action filter at the last step (get_last_filtered_action, gym_env.py:385-387) */
    QS_INFO_REWARD_END = 12,  /* [N,1]: get_reward_end_episode() (gym_env.py:363-365): the end-of-episode bonus / malus the task would add
                               * if the episode ended in the current state */
    QS_INFO_PAYLOAD_BLOCK = 13,  /* [N,20], cfg.payload_soft only: the block's centre 3, quaternion 4, linear 3 and angular 3 velocity (world), the
                                  * six impulses of its fixed constraint at the last substep, the distance between the two pivots */
    QS_INFO_WRAPPER = 10,  /* [N,4]: phase after the step (0 policy, 1 take-off hold, 2 landing, 3 rest), scripted (the step just
                            * made ignored the caller's action), timer, end time */
    QS_INFO_EXTERNAL_WRENCH = 14,  /* [N,8]: the push of qs_set_external_wrench: force 3, torque 3 (as set, in their frame), remaining substeps,
                                    * frame */
    QS_INFO_RACK = 15,  /* [N,8], handles with a rack only: 1 while the robot is hung (0 released), the rack's force 3 and torque 3 on the trunk
                         * over the last substep (world frame, torque about the pivot; impulses / dt), the distance from the base origin to the
                         * anchor */
};
int qs_info_dim(const qs_handle* h, int which);
int qs_get_info(qs_handle* h, int which, float* out /*[N, qs_info_dim]*/);
enum { QS_PARAM_MU = 0, QS_PARAM_SPRING_K = 1, QS_PARAM_SPRING_B = 2, QS_PARAM_KP = 3, QS_PARAM_KD = 4, QS_PARAM_ALL = 5 };
int qs_set_params(qs_handle* h, int which, const float* vals);
/* number of env-steps' worth of settle substeps executed so far (reset cost accounting) */
int qs_stats(qs_handle* h, uint64_t* settle_substeps, uint64_t* resets);
/* qs_step with ONE output array: fused[N][obs_dim + 2] = observation | reward | done + 2 * truncated (floats).  This is the
 * buffer a sharded run all-gathers to the learner rank (one collective per step, qs_amd/sharded.py), written by the step
 * kernel itself instead of being packed from four arrays afterwards. */
int qs_step_fused(qs_handle* h, const float* actions, float* fused);
/* qs_step with a per-environment pause.  active [N] uint8, device memory; NULL makes it qs_step.  An environment with active[e] == 0 is
 * FROZEN for this launch: nobody steps it.  Unchanged: its record (every field, the info block and warm start included), its last
 * observation, its pending push (no countdown), its look-ahead window, the handle's counters, the trace tap's rows if it is the tapped
 * environment.  Written for it: obs[e] = its last observation, rew[e] = 0, done[e] = 0, truncated[e] = 0.  It is not reset, gets no
 * terminal observation and is not counted as a reset.  Every active environment's results are bit for bit those of qs_step.
 * A wave (16 consecutive environments) without an active one leaves after reading the mask; in a wave with work, a frozen environment's
 * quad steps the handle's parked record -- a robot hanging in the air that asks for no rare path -- and stores nothing, so a robot on the
 * floor that is frozen holds up nobody.  With solo waves, a frozen environment is its home wave's again in the next launch.
 * Handles without a parked record (cfg.reset_lookahead = 0, QS_RAND_KEEP) step a private copy of the frozen environment's own record
 * instead and store nothing: correct, not faster (and the rare paths' counters still count it).  Refused with payload_soft (the parked
 * record does not carry the payload block along).  qs_step_fused and qs_host_step_* take no mask. */
int qs_step_masked(qs_handle* h, const float* actions, const uint8_t* active /*[N] or NULL*/, float* obs, float* rew, uint8_t* done, uint8_t* truncated);
/* ---- Host (numpy) path: the SB3 consumer of load_model.py:113-133 hands over HOST arrays.  qs_host_step_begin = VecEnv.step_async:
 * `actions` is a host array [N, action_dim] (any memory; copied into page-locked staging before the call returns); the step is enqueued on
 * the handle's stream with its action and result pointers IN that page-locked host memory, mapped into the device's address space: the
 * kernel reads its 24 B of actions per environment and writes its result rows over PCIe itself, the waves that finish first while the
 * others still compute (QS_HOST_PATH=copy in the environment: an H2D and a D2H copy around the step instead; 47 against 55 M env-steps/s
 * at N = 8192).  qs_host_step_end = VecEnv.step_wait: waits for the step and points `out` at the results in page-locked host memory
 * owned by the handle: two blocks alternate, so the arrays of a step stay valid until the end of the
 * NEXT step.  terminal_rows: the observations of the environments that ended their episode in this step BEFORE their auto-reset
 * (SB3: infos[i]["terminal_observation"]) as a compact list -- row r = [environment index (int32 bits), observation], in no particular
 * order; the number of rows is the number of set `done` flags, of which the list holds the first terminal_cap (256, or N if smaller):
 * a step that ends more episodes than that reads the rest with qs_get_info(QS_INFO_TERMINAL_OBS). */
typedef struct qs_host_result {
    const float* obs;            /* [N, obs_dim] */
    const float* rew;            /* [N] */
    const uint8_t* done;         /* [N] 0 / 1 */
    const uint8_t* truncated;    /* [N] 0 / 1: done by the time limit, not by the task (gym_env.py:245-246) */
    const float* terminal_rows;  /* [terminal_cap, 1 + obs_dim] */
    int32_t terminal_cap;
} qs_host_result;
/* Failures: one BEFORE the step's launch (bad arguments, a DEMO task without its demonstration, the previous step not collected) leaves the
 * handle as it was.  One BEHIND the launch (the attached normalisation or the copy of the block failed) is returned by qs_host_step_begin
 * and the step STAYS pending -- the simulation has advanced --: qs_host_step_end waits for it, reports the same failure once more and
 * closes the step; the host block then does not hold that step's results. */
int qs_host_step_begin(qs_handle* h, const float* actions);
int qs_host_step_end(qs_handle* h, qs_host_result* out);

/* Telemetry counters (synchronises the stream). */
enum { QS_COUNTER_SETTLE_SUBSTEPS = 0,      /* settle substeps executed (k_reset, in-step settles, settle lanes) */
       QS_COUNTER_RESETS = 1,               /* environment resets */
       QS_COUNTER_LOOKAHEAD_SERVED = 2,     /* resets that took a look-ahead state */
       QS_COUNTER_LOOKAHEAD_SETTLED = 3,    /* look-ahead states the settle lanes have delivered */
       QS_COUNTER_LIMIT_PATH_SUBSTEPS = 4,  /* wave-substeps in which some joint of the wave's 16 environments sat at a stop or (body_contacts)
                                               a non-foot link touched the plane: those run the many-rows solve (of this handle; per
                                               process before round 4) */
       QS_COUNTER_SELF_NARROW_SUBSTEPS = 5, /* wave-substeps (the last of an env step) whose self-collision broad phase found a calf close
                                               enough to another leg or the trunk to run the link-link tests (of this handle) */
       QS_COUNTER_RESET_STALLS = 6,         /* resets of a handle with reset_lookahead > 0 whose state was not ready: settled in place */
       QS_COUNTER_LOOKAHEAD_BACKLOG = 7,    /* reset states the environments' look-ahead windows lack and no settle lane has taken yet */
       QS_COUNTER_SOLO_PATH_SUBSTEPS = 8    /* of LIMIT_PATH_SUBSTEPS: those of solo waves (qs_solo_waves), which hold up no wave-mate */ };
int qs_counter(qs_handle* h, int which, uint64_t* value);
/* The counters 0 .. 6 as they stand at this point of the handle's stream, copied to `dev_out[8]` (DEVICE memory; entry 7 is left alone) by
 * copies enqueued on the stream: nothing is waited for.  For a reader that wants the counters of a region without idling the device in
 * front of it (bench.py: a synchronising read right before a short timed region made its first launch ~100 us late). */
int qs_counters_async(qs_handle* h, uint64_t* dev_out);
/* Average duration of the step-kernel launches of a BATCH of qs_step calls, from two HIP events on the handle's stream: one recorded in
 * front of the first step launched after qs_enable_timing(h, 1), one recorded by qs_last_step_kernel_ms, which waits for it, returns
 * elapsed milliseconds / launches since the first event and starts the next batch.  For bench.py's roofline leg: the figure covers the
 * timed region itself and includes the gaps between back-to-back launches, so it can never be shorter than the kernel's own duration nor
 * longer than the wall time per step (a pair of events around every single 0.07-ms launch read 5 % high).  qs_enable_timing(h, 2) closes
 * the batch without waiting: the closing event is recorded on the stream there and qs_last_step_kernel_ms, whenever it is called, waits for
 * that one (a caller that times the region on its own clock keeps the wait out of it). */
int qs_enable_timing(qs_handle* h, int on);
int qs_last_step_kernel_ms(qs_handle* h, float* ms);
/* The settle lanes of a handle with cfg.reset_lookahead > 0 (on from qs_create).  While on, every qs_step launch carries extra
 * workgroups that advance resets (gym_env.py:278-297, 325-327: randomizer draws, spawn, 2500 substeps under the settling command) by
 * action_repeat substeps each, through the same substep loop as the environments; a finished one goes to its environment's look-ahead
 * slot.  An epoch = the settle_steps / action_repeat launches one settle takes; the lanes work in five cohorts that start a fifth of an
 * epoch apart, each taking at its start what the environments' windows lack (environment e in episode X wants X + 1 .. X + K).  Off:
 * nothing is settled ahead (the settles in progress start over when the lanes come back), resets use up the states that are ready and
 * then settle in place -- results do not change, only when the work is done. */
int qs_settle_lanes(qs_handle* h, int on);
/* Solo waves of a handle with look-ahead reset states.  A robot that ends an env step with a non-foot link within `reach` metres of its
 * contact range is stepped, in the next launch, by a workgroup of its own -- one of `f` extra workgroups at the front of the grid -- next to
 * fifteen copies of a parked record instead of next to its fifteen wave-mates: the many-rows substeps of its fall then hold up nobody and
 * skip the common-path solve that only the mates need.  Results do not change, bit for bit; only who computes them.  f = 0 switches them
 * off, f = -1 keeps the count; f up to 512.  reach <= 0 keeps the current one.  Defaults: QS_SOLO_WAVES / QS_SOLO_REACH in the environment at qs_create, else
 * 128 workgroups and 0.02 m.  They run only where they fit next to the environments' waves and the settle lanes on otherwise idle SIMDs,
 * in the one-wave-per-SIMD kernels, with cfg.body_contacts and without rack or soft payload; elsewhere the setting is kept and nothing
 * happens.  QS_COUNTER_SOLO_PATH_SUBSTEPS / QS_COUNTER_LIMIT_PATH_SUBSTEPS is the share of the many-rows wave-substeps they take.
 * Fails for f > 0 on a handle without look-ahead states (cfg.reset_lookahead = 0, or QS_RAND_KEEP). */
int qs_solo_waves(qs_handle* h, int f, float reach);
/* Per-substep trace tap for ONE environment (evaluation_wrapper.py:14,36-41 set_sub_step_callback; monitor_state.py:66-85):
 * while set, every qs_step writes action_repeat rows of QS_TRACE_DIM floats into `rows` (device memory, caller owned), one per
 * physics substep of environment `env`: sim time, base position 3, quaternion xyzw 4, linear velocity 3, angular velocity 3,
 * joint angles 12, joint velocities 12, applied motor torque 12, spring torque 12, foot normal force 4, foot contact 4.
 * env < 0 or rows == NULL switches it off. */
int qs_set_trace(qs_handle* h, int env, float* rows);

/* ---- SB3 VecNormalize on device (stable_baselines3 1.5.1a7: common/vec_env/vec_normalize.py, common/running_mean_std.py),
 * as applied by the reference at load_model.py:109-137 and get_demonstrations.py:71.  Operates in place on the device arrays
 * a step / reset produced; statistics are float64.  norm handles are independent of simulation handles. */
typedef struct qs_norm qs_norm;
int qs_norm_create(int n_envs, int obs_dim, double clip_obs, double clip_reward, double gamma, double epsilon, int device, qs_norm** out);
void qs_norm_destroy(qs_norm* h);
int qs_norm_set_stream(qs_norm* h, void* hip_stream);
/* host arrays [obs_dim]; RunningMeanStd.mean / .var / .count of obs_rms and ret_rms (VecNormalize.load / save) */
int qs_norm_set_stats(qs_norm* h, const double* obs_mean, const double* obs_var, double obs_count, double ret_mean, double ret_var, double ret_count);
/* what the handle was created for (any pointer may be NULL) */
int qs_norm_dims(const qs_norm* h, int* n_envs, int* obs_dim, int* device);
int qs_norm_get_stats(qs_norm* h, double* obs_mean, double* obs_var, double* obs_count, double* ret_mean, double* ret_var, double* ret_count);
/* VecNormalize.reset: returns <- 0, obs_rms.update(obs) if training && norm_obs, obs <- normalize_obs(obs) */
int qs_norm_reset(qs_norm* h, float* obs /* [N,o] */, int training, int norm_obs);
/* VecNormalize.step_wait: obs_rms.update(obs); obs <- normalize_obs(obs); returns <- returns*gamma + rew; ret_rms.update(returns);
 * rew <- normalize_reward(rew); term_obs (may be NULL) <- normalize_obs(term_obs); returns[done] <- 0.
 * raw_obs [N,o] / raw_rew [N] (either may be NULL) receive the values before normalisation: VecNormalize.old_obs / old_reward
 * (get_original_obs / get_original_reward), written by the same pass */
int qs_norm_step(qs_norm* h, float* obs /* [N,o] */, float* rew /* [N] */, const uint8_t* done /* [N] */, float* term_obs /* [N,o] or NULL */,
                 int training, int norm_obs, int norm_reward, float* raw_obs, float* raw_rew);
/* qs_norm_step after a qs_step_masked.  active [N] uint8, device memory; NULL makes it qs_norm_step.  When training, the batch moments of
 * observations and of returns are taken over the rows with active[i] != 0 only, the batch count is their number (summed on the device),
 * and only those rows' returns advance (returns <- returns*gamma + rew) and go to zero at done; a step without an active row leaves the
 * statistics as they are.  Every row, frozen ones included, is normalised with the step's statistics, and raw_obs / raw_rew receive every
 * row.  A mask of ones gives the bits of qs_norm_step. */
int qs_norm_step_masked(qs_norm* h, float* obs /* [N,o] */, float* rew /* [N] */, const uint8_t* done /* [N] */, const uint8_t* active /* [N] or NULL */,
                        float* term_obs /* [N,o] or NULL */, int training, int norm_obs, int norm_reward, float* raw_obs, float* raw_rew);

/* qs_norm_step with everything a host-path step carries.  The arrays of the step (device memory): obs [N,o], rew [N], done [N], trunc [N]
 * (may be NULL), term_obs [N,o] (may be NULL), tail_rows = the compact list of the step's terminal observations, [tail_cap][1 + o] (may
 * be NULL; qs_host_result::terminal_rows while still on the device).  out_* all NULL: normalised in place.  Otherwise out_obs / out_rew
 * receive the normalised arrays, out_done / out_trunc / out_tail copies of the flags and the (normalised) list -- e.g. mapped host memory,
 * which the kernel then writes itself; the inputs stay raw (term_obs is normalised in place either way).  raw_obs / raw_rew as in
 * qs_norm_step. */
typedef struct qs_norm_io {
    float* obs; float* rew; const uint8_t* done; const uint8_t* trunc; float* term_obs; float* tail_rows; int32_t tail_cap;
    float* out_obs; float* out_rew; uint8_t* out_done; uint8_t* out_trunc; float* out_tail;
    float* raw_obs; float* raw_rew;
    const uint64_t* tail_count;   /* device memory, may be NULL: how many rows of tail_rows this step filled (only those are normalised / copied;
                                   * NULL: all tail_cap rows) */
} qs_norm_io;
int qs_norm_step_io(qs_norm* h, const qs_norm_io* io, int training, int norm_obs, int norm_reward);
/* VecNormalize around the HOST path (load_model.py:109-137: VecNormalize.load(stats, env), then env.step(numpy actions)): from the next
 * qs_host_step_begin on, the step's results pass through `norm` (qs_norm_step_io: statistics update if training, observations, rewards
 * and the terminal observations of the compact list normalised) before they reach the host block, so that qs_host_step_end hands out
 * what VecNormalize.step_wait returns.  raw_obs [N,o] / raw_rew [N] (device memory, may be NULL): the values before normalisation
 * (get_original_obs / get_original_reward).  norm == NULL switches it off (at any time); it is switched on between two steps, not between
 * a begin and its end.  The handle keeps the pointer, not the object: switch it off (or destroy the simulation handle) before
 * qs_norm_destroy(norm).  Fails -- before anything is launched -- if `norm` was created for another number of environments, another
 * observation width or another device than `h`. */
int qs_host_set_norm(qs_handle* h, qs_norm* norm, int training, int norm_obs, int norm_reward, float* raw_obs, float* raw_rew);

/* ---- Camera images (QuadrupedGymEnv.render(mode="rgb_array") -> utils/camera.py:35-59, which calls pybullet.getCameraImage with
 * computeViewMatrixFromYawPitchRoll(target, distance, yaw, pitch, roll 0, upAxisIndex 2) and computeProjectionMatrixFOV(fov, W / H, near,
 * far)).  Every environment is its own world: its image shows its robot (the collision primitives of go1.urdf -- trunk box, hip housings,
 * thigh-shoulder cylinders, thigh and calf boxes, foot spheres -- posed by the state row, plus the payload block when the parameters carry
 * a payload mass > 0), the plane z = 0 as a checkerboard of 1 m squares and a constant sky; one directional light, Lambert shading plus
 * ambient, hard shadows cast by the robot; one ray through each pixel centre (row 0 at the top).  Camera: R = Rz(yaw) Rx(pitch) (degrees),
 * eye = target + R (0, -distance, 0), up = R (0, 0, 1), looking at the target, fov vertical; hits nearer than near_clip along the view axis
 * are ignored and nothing beyond far_clip is drawn.  (Our reading of Bullet's C API; camera modes: qs_amd/render.py CAMERA_MODES.)
 * Outputs, row-major [m, height, width]: rgba packed RGBA8 (R in the low byte, A = 255); depth (may be NULL) in metres along the view axis,
 * far_clip for sky; seg (may be NULL) int32: -1 sky, 0 ground, 1 trunk, 2 + 4 leg + part (legs in q order; part 0 hip, 1 thigh box and
 * shoulder cylinder, 2 calf, 3 foot), 18 payload block.  A pixel depends on its environment's state, the camera and the image size only.
 * Fails (nothing launched) for m < 0, width or height outside [1, 8192], a null rgba, fov_deg outside (0, 180) or 0 < near_clip < far_clip
 * not holding.  Stream-ordered, no host synchronisation, no allocation. */
typedef struct qs_camera {
    float target[3];      /* world position; with follow_base: an offset added to the base position */
    float distance, yaw_deg, pitch_deg, fov_deg, near_clip, far_clip;
    int32_t follow_base;  /* 1: target = base position + target */
    int32_t draw_payload; /* 0: leave the payload block out */
} qs_camera;
/* The handle's environments env_ids[0..m) (device int32), read straight from the records, on the handle's stream.  Under cfg.payload_soft
 * the block is drawn at its own pose.  An id outside [0, n_envs) draws sky with segmentation id -2, and the next qs_stats or qs_counter
 * (which wait for the device anyway) fails once, naming its position in env_ids. */
int qs_render(qs_handle* h, const int32_t* env_ids, int m, const qs_camera* cam, int width, int height,
              uint32_t* rgba /*[m,H,W]*/, float* depth /*[m,H,W] or NULL*/, int32_t* seg /*[m,H,W] or NULL*/);
/* Any [m,37] state rows in device memory (qs_get_state layout), e.g. a recorded rollout or the trace tap's rows; params [m,24] (layout of
 * QS_INFO_PARAMS; the payload block sits at r_payload in the base frame) or NULL (no payload block).  On `stream` (a hipStream_t, NULL = the
 * null stream) of the current device. */
int qs_render_states(const float* states, const float* params, int m, const qs_camera* cam, int width, int height,
                     uint32_t* rgba, float* depth, int32_t* seg, void* stream);

/* ---- Policy inference (load_model.py:132 `action, _ = model.predict(obs, deterministic=True)`: SB3 BasePolicy.predict on a PPO MlpPolicy
 * -- two tanh layers of 64 -- or an sb3_contrib ARS policy -- linear without bias, or a small MLP; and sb3_contrib ARS.evaluate_candidates,
 * which runs one perturbed parameter vector per episode).  One launch computes for every environment i, with policy p = i / (n_envs / n_policies):
 *     h = obs[i];  h <- act(W_l[p] h + b_l[p]) for each hidden layer;  mean = W_out[p] h + b_out[p]  (tanh of it under squash_output)
 *     a = mean + exp(log_std) * eps[i]                          if eps != NULL (DiagGaussianDistribution.sample with the caller's noise)
 *     log_prob[i] = sum_j (-eps_ij^2 / 2 - log_std_j - log(2 pi) / 2)      if asked for (Normal(mean, std).log_prob(a).sum(-1), before clipping)
 *     actions[i] = clamp(a, clip_lo, clip_hi)                   BasePolicy.predict clips to the action Box;  mean_out[i] = mean (not clipped)
 * in float32, every pre-activation one fmaf chain in ascending k that starts from the bias (csrc/qs_policy.h), so an environment's result does
 * not depend on the other environments of the batch.  Parameters: ONE device array [n_policies][qs_policy_param_count()], per policy layer by
 * layer the weight [out][in] row-major and then the bias [out] (none at all without has_bias): torch.nn.utils.parameters_to_vector over a
 * Sequential of Linear layers, the flat theta that ARS perturbs.  Limits: obs_dim <= 64, at most QS_POLICY_MAX_HIDDEN hidden layers, every
 * width and action_dim <= 256, n_policies divides n_envs; a descriptor outside them fails with text in qs_last_error().
 * Policy handles are independent of simulation handles. */
#define QS_POLICY_MAX_HIDDEN 4
enum { QS_POLICY_ACT_NONE = 0, QS_POLICY_ACT_TANH = 1, QS_POLICY_ACT_RELU = 2 };
typedef struct qs_policy qs_policy;
typedef struct qs_policy_desc {
    int32_t n_envs, n_policies, obs_dim, action_dim, n_hidden, hidden[QS_POLICY_MAX_HIDDEN];
    int32_t activation;      /* QS_POLICY_ACT_*: of the hidden layers */
    int32_t squash_output;   /* tanh on the last layer's output (SB3 squash_output) */
    int32_t has_bias;        /* 0: no layer has a bias (sb3_contrib's linear ARS policy) */
    float clip_lo, clip_hi;  /* the action Box; -3e38 / 3e38 for none (finite: the kernels are built with -ffinite-math-only) */
} qs_policy_desc;
int qs_policy_create(const qs_policy_desc* d, int device, qs_policy** out);
void qs_policy_destroy(qs_policy* p);
int qs_policy_set_stream(qs_policy* p, void* hip_stream);
/* parameters of ONE policy (a negative code for a null handle) */
int qs_policy_param_count(const qs_policy* p);
/* dev_params [n_policies][param_count] in device memory.  The handle KEEPS THE POINTER and copies nothing: every later qs_policy_act reads
 * the array as it is then (an ARS population rewritten in place needs no second call); the caller keeps it alive until the handle is
 * destroyed or given another array. */
int qs_policy_set_params(qs_policy* p, const float* dev_params);
/* obs [N, obs_dim], eps [N, action_dim] or NULL (deterministic), log_std [action_dim] (required with eps), actions [N, action_dim],
 * mean_out [N, action_dim] or NULL, log_prob [N] or NULL (needs eps).  Stream-ordered, no host synchronisation, no allocation. */
int qs_policy_act(qs_policy* p, const float* obs, const float* eps, const float* log_std, float* actions, float* mean_out, float* log_prob);

/* ---- PPO collection on the device (stable_baselines3 1.5 as remembered: OnPolicyAlgorithm.collect_rollouts, ActorCriticPolicy.forward,
 * RolloutBuffer.add / compute_returns_and_advantage).  Actor and critic are two separate networks (MlpPolicy's default
 * net_arch = dict(pi=[64, 64], vf=[64, 64])), each described like a qs_policy and computed by the same chain (csrc/qs_policy.h, csrc/qs_ppo.h):
 * action, value and log-prob of an environment are the bits two qs_policy handles give for the same parameters.  Shared trunks are not
 * supported.  Handles are independent of simulation handles; every call is stream-ordered, without host synchronisation or allocation. */
typedef struct qs_ac qs_ac;
/* ActorCriticPolicy.__init__ for an MlpPolicy with separate trunks.  Refuses, with text in qs_last_error(): n_policies != 1 in either
 * descriptor, differing n_envs or obs_dim, a critic with action_dim != 1, with squash_output or with finite clips (a value is neither
 * squashed nor clipped: clip_lo <= -3e38, clip_hi >= 3e38), and whatever qs_policy_create refuses. */
int qs_ac_create(const qs_policy_desc* actor, const qs_policy_desc* critic, int device, qs_ac** out);
void qs_ac_destroy(qs_ac* h);
int qs_ac_set_stream(qs_ac* h, void* hip_stream);
/* The two flat parameter arrays in device memory (each as in qs_policy_set_params, one row).  The handle KEEPS THE POINTERS and copies
 * nothing: an optimiser step written into the arrays (torch.optim.Adam.step on parameters that are views of them) is what the next call reads. */
int qs_ac_set_params(qs_ac* h, const float* actor_params, const float* critic_params);
/* One step of collect_rollouts in one launch: `actions, values, log_probs = policy(obs)`, `clipped_actions = np.clip(actions, low, high)`
 * and RolloutBuffer.add(obs, actions, ., ., values, log_probs).  obs [N, obs_dim], eps [N, action_dim] (required: the sample's noise, e.g. a
 * row of one torch.randn per rollout), log_std [action_dim]; env_actions [N, action_dim] receives the CLIPPED action the environment steps
 * with; obs_row [N, obs_dim], action_row [N, action_dim] (the UNCLIPPED action, as SB3 stores it), value_row [N], log_prob_row [N] are
 * row t of the caller's [T, N, ...] storage.  The observation is read from global memory once. */
int qs_ac_collect(qs_ac* h, const float* obs, const float* eps, const float* log_std, float* env_actions, float* obs_row, float* action_row,
                  float* value_row, float* log_prob_row);
/* policy.predict_values(obs): values_out[i] = V(obs[i]) for every i with mask[i] != 0 (mask uint8 [N], device memory; NULL = every
 * environment); the others are not written.  collect_rollouts calls it for the last observation of a rollout. */
int qs_ac_values(qs_ac* h, const float* obs, const uint8_t* mask_or_null, float* values_out);
/* collect_rollouts' time-limit bootstrap (`rewards[idx] += gamma * policy.predict_values(terminal_observation)` where
 * infos[idx]["TimeLimit.truncated"]): rewards_inout[i] = fmaf(gamma, V(terminal_obs[i]), rewards_inout[i]) where truncated[i] != 0; the
 * others are not touched.  terminal_obs [N, obs_dim] (QS_INFO_TERMINAL_OBS, normalised by qs_norm_step's term_obs under VecNormalize). */
int qs_ac_bootstrap(qs_ac* h, const float* terminal_obs, const uint8_t* truncated, float gamma, float* rewards_inout);
/* RolloutBuffer.compute_returns_and_advantage(last_values, dones) as one launch, one lane per environment.  Arrays [T][N] float32 in
 * device memory: rewards, values, episode_starts (0 or 1), advantages and returns (outputs); last_values [N], last_dones [N] uint8.  Per
 * environment, t = T-1 ... 0:  nnt = 1 - (t == T-1 ? last_done : episode_start[t+1]);  nv = (t == T-1 ? last_value : value[t+1]);
 * delta = fmaf(gamma * nnt, nv, reward[t]) - value[t];  gae = fmaf(gamma * lambda * nnt, gae, delta);  advantage[t] = gae;
 * return[t] = gae + value[t].  Needs no handle: on `hip_stream` (a hipStream_t, NULL = the null stream) of the current device. */
int qs_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values, const uint8_t* last_dones, int T, int N,
           float gamma, float lambda, float* advantages, float* returns, void* hip_stream);

/* ---- The PPO update on the device (stable_baselines3 1.5 as remembered: PPO.train's minibatch -- evaluate_actions, the clipped loss,
 * loss.backward, clip_grad_norm_, Adam.step).  The arithmetic, its roundings and its summation order are csrc/qs_ppo_train.h.  For the
 * policies a qs_ac has, narrowed: obs_dim <= 64, at most 2 hidden layers per network, every width and action_dim <= 64, biases on every
 * layer, no squash; clip_range_vf is not supported.  Every call is stream-ordered, waits for nothing and allocates nothing. */
typedef struct qs_ppo qs_ppo;
typedef struct qs_ppo_hyper {
    float clip_range, ent_coef, vf_coef;
    float max_grad_norm;             /* 3e38 for none */
    int32_t normalize_advantage;     /* skipped for a minibatch of one sample */
    int32_t reserved;
    double lr, beta_one, beta_two, adam_eps;   /* torch.optim.Adam(lr, betas, eps); no weight decay, no amsgrad */
} qs_ppo_hyper;
enum { QS_PPO_STAT_POLICY_LOSS = 0, QS_PPO_STAT_VALUE_LOSS = 1, QS_PPO_STAT_ENTROPY_LOSS = 2, QS_PPO_STAT_APPROX_KL = 3,
       QS_PPO_STAT_CLIP_FRACTION = 4, QS_PPO_STAT_GRAD_NORM = 5, QS_PPO_STAT_REFUSED = 6, QS_PPO_STAT_LOSS = 7, QS_PPO_N_STATS = 8 };
/* PPO.__init__'s share: the two networks (as for a qs_ac; n_envs is not used) and the largest minibatch.  Refuses, with text in
 * qs_last_error(), what lies outside the limits above and a layout that does not fit a compute unit's LDS; such a handle is never launched. */
int qs_ppo_create(const qs_policy_desc* actor, const qs_policy_desc* critic, int max_batch, int device, qs_ppo** out);
void qs_ppo_destroy(qs_ppo* h);
int qs_ppo_set_stream(qs_ppo* h, void* hip_stream);
/* policy.parameters() and the optimiser's state: the flat parameter arrays of a qs_ac, log_std [action_dim], and Adam's two moments
 * [n_actor + n_critic + action_dim] (actor, critic, log_std in that order), all float32 in device memory.  The handle KEEPS THE POINTERS. */
int qs_ppo_bind(qs_ppo* h, float* actor_params, float* critic_params, float* log_std, float* exp_avg, float* exp_avg_sq);
/* One minibatch of PPO.train up to and including loss.backward(): rollout_data is taken BY INDEX from the flat [total, ...] rollout arrays
 * (RolloutBuffer.get's gathers are not materialised): observations [total, obs_dim], actions [total, action_dim], old_log_prob, advantages,
 * returns [total]; indices [batch] int64.  grad_out [n_actor + n_critic + action_dim] receives the gradient of
 * policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, stats_out [QS_PPO_N_STATS] the minibatch's statistics (grad_norm is
 * written by the Adam call).  An index outside [0, total) is not read: its sample contributes nothing, is counted in
 * stats_out[QS_PPO_STAT_REFUSED] and in the handle's refusal counter. */
int qs_ppo_grad(qs_ppo* h, const float* observations, const float* actions, const float* old_log_prob, const float* advantages, const float* returns,
                long long total, const long long* indices, int batch, const qs_ppo_hyper* hyper, float* grad_out, float* stats_out);
/* clip_grad_norm_(policy.parameters(), max_grad_norm) and optimizer.step(), step = 1, 2, ...: in place on the bound parameters and moments.
 * grad is what the handle's last gradient call wrote (its sums of squares are the handle's); stats_inout[QS_PPO_STAT_GRAD_NORM] receives the norm before clipping. */
int qs_ppo_adam(qs_ppo* h, const float* grad, const qs_ppo_hyper* hyper, int step, float* stats_inout);
/* samples refused since the last call (waits for the handle's stream) */
int qs_ppo_refusals(qs_ppo* h, unsigned long long* out);

/* ---- ARS's bookkeeping on the device (sb3_contrib 1.5 as remembered: ARS.evaluate_candidates' episode accounting and ARS._do_one_update; the
 * package was not available to check against).  The arithmetic, its roundings and its summation order are csrc/qs_ars.h.  n_envs = P m
 * environments for P = 2 n_delta candidates; candidate p owns the environments [p m, (p + 1) m), as a qs_policy with n_policies = P does; the
 * + candidates come first.  The handle owns the per-environment accounts (return, length, episodes, alive), two counters (environments
 * alive, steps summed) and the results of the last finish.  Every call but qs_ars_alive is stream-ordered, waits for nothing and allocates
 * nothing; there are no floating-point atomics, so the same inputs give the same bits. */
typedef struct qs_ars qs_ars;
/* Refuses, with text in qs_last_error(): n_delta outside [1, 1024], n_envs that is no positive multiple of 2 n_delta, n_params < 1,
 * episodes_per_env < 1. */
int qs_ars_create(int n_envs, int n_delta, int n_params, int episodes_per_env, int device, qs_ars** out);
void qs_ars_destroy(qs_ars* h);
int qs_ars_set_stream(qs_ars* h, void* hip_stream);
/* candidates [2 n_delta][n_params] (what qs_policy_set_params was given) = theta [n_params] +- sigma * delta [n_delta][n_params] */
int qs_ars_perturb(qs_ars* h, const float* theta, const float* delta, float sigma, float* candidates);
/* the start of a rollout: every account zero, every environment alive */
int qs_ars_begin(qs_ars* h);
/* One environment step: raw_reward [n_envs] float32 (before any normalisation), done [n_envs] uint8.  An alive environment adds the reward and
 * one step; where done it counts an episode and dies at episodes_per_env of them.  A dead environment changes nothing. */
int qs_ars_account(qs_ars* h, const float* raw_reward, const uint8_t* done);
/* the number of environments alive, copied to the host (WAITS for the handle's stream) */
int qs_ars_alive(qs_ars* h, int* out);
/* the candidates' returns R_p = sum over the block of (return + alive_bonus_offset * length), and the sum of all lengths */
int qs_ars_returns(qs_ars* h, float alive_bonus_offset);
/* qs_ars_returns, then ARS._do_one_update: the n_top directions with the largest max(R+, R-) (ties: the lower index first, this project's
 * rule), step = learning_rate / (n_top * std of their 2 n_top returns + 1e-6), theta += step * sum (R+ - R-) delta, in place.  delta is the
 * array qs_ars_perturb was given.  Refuses n_top outside [1, n_delta]. */
int qs_ars_finish(qs_ars* h, float* theta, const float* delta, int n_top, float learning_rate, float alive_bonus_offset);
/* Getters: a stream-ordered copy into DEVICE memory.  RET float32 [n_envs], LEN and EPISODES int32 [n_envs], ALIVE uint8 [n_envs], N_ALIVE
 * int32 [1], STEPS uint64 [1] (of the last returns / finish), RETURNS float32 [2 n_delta], IDX int32 [n_delta] and W float32 [n_delta] (the
 * first n_top entries are the last finish's), STATS float32 [2] = std, step. */
enum { QS_ARS_GET_RET = 0, QS_ARS_GET_LEN = 1, QS_ARS_GET_EPISODES = 2, QS_ARS_GET_ALIVE = 3, QS_ARS_GET_N_ALIVE = 4, QS_ARS_GET_STEPS = 5,
       QS_ARS_GET_RETURNS = 6, QS_ARS_GET_IDX = 7, QS_ARS_GET_W = 8, QS_ARS_GET_STATS = 9 };
int qs_ars_get(qs_ars* h, int what, void* dev_out);

/* ---- The sampling planner on the device (predictive sampling and MPPI over device forks, examples/mpc.py).  The arithmetic, its roundings, its
 * summation order and its two own rules (ties go to the lower candidate, a score that is not finite counts as -inf) are csrc/qs_mpc.h.
 * n_robots real robots are the environments [0, M); candidate c of robot m is environment M + m C + c, N = M (1 + C).  The handle owns the plan
 * [M][H][d], the sampled sequences [H][M C][d], the candidates' scores and running flags [M C] and the last choice [M].  Every call is
 * stream-ordered, waits for nothing and allocates nothing after create; there are no floating-point atomics, so the same inputs give the
 * same bits. */
typedef struct qs_mpc qs_mpc;
enum { QS_MPC_BEST = 0, QS_MPC_MPPI = 1 };
/* Refuses, with text in qs_last_error(): n_robots, n_candidates, horizon or action_dim < 1, n_candidates > 4096, horizon * action_dim > 1024,
 * products that leave 31 bits.  The plan starts at zero. */
int qs_mpc_create(int n_robots, int n_candidates, int horizon, int action_dim, int device, qs_mpc** out);
void qs_mpc_destroy(qs_mpc* h);
int qs_mpc_set_stream(qs_mpc* h, void* hip_stream);
/* The sequences of a control step from eps [H][M C][d] (standard normal, filled by the caller): candidate 0 is the plan as it stands, the others
 * clamp(plan + sigma * eps, -1, 1); every score 0, every candidate running.  Refuses a sigma that is not finite. */
int qs_mpc_sample(qs_mpc* h, const float* eps, float sigma);
/* Horizon step `step` = 0 .. H, one launch next to the environment step.  For step >= 1 it accounts the environment step before it from
 * reward [N] and done [N]: a running candidate adds its reward, then stops running where done.  For step < H it copies the sequences' slab
 * of that step into actions[M:] (actions [N][d]).  At step == H a candidate still running adds reward_end[(M + i) * reward_end_stride].
 * active_or_null [N], where given, receives the candidates' running flags and 0 for the real robots (qs_step_masked's mask).  reward and
 * done may be null at step 0, reward_end below step H. */
int qs_mpc_feed(qs_mpc* h, int step, const float* reward, const uint8_t* done, const float* reward_end, int reward_end_stride, float* actions,
                uint8_t* active_or_null);
/* The choice: per robot the best candidate (QS_MPC_BEST) or the mean under the weights exp((score - max) / lambda) (QS_MPC_MPPI; refuses a
 * lambda that is not positive and finite).  actions[m] = the chosen sequence's first action, the plan = the rest, the last action held. */
int qs_mpc_finish(qs_mpc* h, int method, float lambda, float* actions);
/* Getters: a stream-ordered copy into DEVICE memory.  PLAN float32 [M][H][d], SEQ float32 [H][M C][d], SCORE float32 [M C], RUNNING uint8
 * [M C], BEST int32 [M] and BEST_SCORE float32 [M] of the last finish. */
enum { QS_MPC_GET_PLAN = 0, QS_MPC_GET_SEQ = 1, QS_MPC_GET_SCORE = 2, QS_MPC_GET_RUNNING = 3, QS_MPC_GET_BEST = 4, QS_MPC_GET_BEST_SCORE = 5 };
int qs_mpc_get(qs_mpc* h, int what, void* dev_out);
/* The plans of the robots with mask_or_null[m] != 0 (null: all) become plan_or_null's rows [M][H][d] (null: zero). */
int qs_mpc_set_plan(qs_mpc* h, const float* plan_or_null, const uint8_t* mask_or_null);

/* ---- Device snapshots: save, restore and fork environments (what pybullet.saveState / restoreState are to the reference's simulator; the CPU
 * oracle's qso_snapshot / qso_restore).  A snapshot is one row of qs_snapshot_info::row_floats floats per environment, in DEVICE memory owned by
 * the caller (16-byte aligned): [the environment's whole record | its push row | its last observation | its terminal observation], layout in
 * csrc/qs_snapshot.h.  That is everything a step reads: the rigid-body state, the action filter's history and the last action, the task block,
 * the wrapper's phase machine, the CPG's oscillators, the demo counter, the episode / step / noise counters, the randomised parameters, the
 * payload block or the rack's hung flag, the pending push.  Randomizer draws are keyed by (seed, global environment id, episode), observation
 * noise by (seed, environment id, total steps), and both counters are in the record: a restored handle continues bit for bit as the run that
 * was never interrupted, noise, randomizers, auto-resets and look-ahead included.
 * Not part of a snapshot and left untouched by qs_restore and qs_fork: the telemetry counters (qs_counter, qs_stats), the trace tap, the
 * demonstration table, the stream, the timing state and the host path's result blocks.  The handle's configuration and rack are not part of
 * it either: the digests below say whether a row fits a handle.
 * All three calls are stream-ordered and never wait for the device. */
struct qs_snapshot_info {
    uint64_t bytes;              /* n_envs * row_floats * 4: the size of the rows */
    int32_t n_envs, row_floats, rec_floats, push_floats, obs_dim;
    int32_t layout_version;      /* bumped by whoever changes csrc/qs_layout.h or the row (csrc/qs_snapshot.h) */
    uint64_t layout_digest;      /* FNV-1a over what gives a row its meaning: layout_version, the record's stride, obs_dim, action_dim, n_envs, task,
                                  * wrapper mode, action-space mode, payload_soft, rack on.  Rows restore only into a handle with the same one. */
    uint64_t config_digest;      /* FNV-1a over every byte of the handle's qs_config and qs_rack: equal = the same simulation (an exact resume);
                                  * rows with the same layout_digest and another config_digest (another seed, other gains) restore as well and
                                  * continue under the handle's own configuration */
};
/* (a struct tag, not a typedef: the entry below carries the same name) */
int qs_snapshot_info(const qs_handle* h, struct qs_snapshot_info* out);
/* handle -> rows.  mask: device [N] bytes or NULL = all; rows: device [N, row_floats].  The rows of unmasked environments are not written. */
int qs_snapshot(qs_handle* h, const uint8_t* mask, float* rows);
/* rows -> handle: record, push row, last observation (qs_get_obs answers with it) and terminal observation of the masked environments.  The
 * look-ahead window of a restored environment is re-seated on the restored episode X: the states of X + 1 .. X + K are queued again; a slot
 * that holds another episode is not taken (its tag says so) and that reset settles in place, counted as a stall, with the same bits.  A push may
 * be pending in the rows, so the step launches read the push rows again (one float per environment) until a reset of all environments.  The
 * caller checks the digests (qs_amd/snapshot.py does): the library cannot know where the rows came from. */
int qs_restore(qs_handle* h, const uint8_t* mask, const float* rows);
/* Environment to environment inside the handle.  src_of: device [N] int32, the source of each environment; -1 or its own index = leave alone.
 * For every i with a source s != i in range, record, push row and both observations of i become those of s, EXCEPT the record's episode
 * number and total-step counter, which stay i's own: the fork keeps its identity -- its future randomizer draws, its noise stream and its
 * look-ahead window -- so no look-ahead slot is invalidated and the window is not touched.  The call behaves as if every source were read
 * before any destination is written (chains i <- j <- k and swaps are legal): a gather launch into staging rows owned by the handle
 * (allocated at the first fork), then a scatter launch.  A source outside [-1, N) leaves that environment alone, and the next qs_stats or
 * qs_counter fails once, naming the first such environment (as for qs_set_external_wrench). */
int qs_fork(qs_handle* h, const int32_t* src_of);
/* VecNormalize.returns, the per-environment discounted returns a qs_norm carries between steps: device [N] float64, stream-ordered copies.
 * With qs_norm_get_stats / qs_norm_set_stats they are all of a normalisation handle's state. */
int qs_norm_get_returns(qs_norm* h, double* returns /* device [N] */);
int qs_norm_set_returns(qs_norm* h, const double* returns /* device [N] */);

const char* qs_last_error(void);
const char* qs_version(void);
/* Bumped whenever the meaning or type of an existing entry point's argument or of a struct field changes (a caller built against an older
 * header would pass garbage without any loader error): 5 = round 5 (qs_norm_create takes its four float arguments as double since round 4;
 * qs_config::reserved_f[0] became support_margin); 6 = qs_set_external_wrench, QS_INFO_EXTERNAL_WRENCH; 7 = qs_camera, qs_render, qs_render_states; 8 = qs_rack, qs_create_ex,
 * qs_set_rack, QS_INFO_RACK.  (The qs_policy_* entries were added under 8: they change no existing entry point, argument or field.)  9 = qs_ac_*, qs_gae (PPO collection; additive, every earlier entry keeps its signature, so structs and calls written against 8 stay valid; qs_amd/lib.py keeps 8 as the version of its struct layouts and demands 9 of the library).  (qs_snapshot_info, qs_snapshot, qs_restore, qs_fork, qs_norm_get_returns and qs_norm_set_returns were added under 9, as the qs_policy_* entries under 8: they change no existing entry point, argument or field.)  (The qs_ppo_* entries and qs_ppo_hyper, the PPO update, were added under 9 in the same way, and so were the qs_ars_* entries, ARS's bookkeeping, and qs_step_masked and qs_norm_step_masked, the per-environment pause.; and the qs_mpc_* entries, the sampling planner.)  A binding compares it with the QS_ABI_VERSION of the header it was written against. */
#define QS_ABI_VERSION 9
int qs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
