/*
 * emei_hip.h — C ABI of libemei_hip.so, the MI355X (gfx950) env-step engine.
 *
 * The reference (polixir/emei) has no FFI boundary: its "operator API" for this path is the Python
 * class surface.  Each entry point below names the reference interface it replaces (file:line under
 * /root/reference).  All pointers are caller-owned DEVICE-ACCESSIBLE pointers (device memory, e.g.
 * torch.Tensor.data_ptr(), or pinned host memory mapped into the device address space), contiguous,
 * never retained past the call (one exception: the gathered buffers handed to emei_set_obs_peers stay registered, and are written by
 * every following rollout, until the list is replaced or cleared).  The library never allocates outputs, never
 * synchronises the stream and never throws across the boundary.  `stream` is a hipStream_t passed
 * as void* (NULL = the default stream).  One handle <-> one device: calls on a handle must be made with
 * that device current (checked: EMEI_ERR_INVALID otherwise; emei_create itself restores the caller's
 * current device).  A handle is not thread-safe, distinct handles are.
 *
 * Return value: 0 = ok, negative = error (EMEI_ERR_*); emei_last_error() gives a thread-local text.
 */
#ifndef EMEI_HIP_H
#define EMEI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  1: emei_config of 64 B.  2: integrator / noise layout / per-coordinate sigmas (328 B), env_params (400 B),
 * emei_set_seed, emei_last_rollout_kernel, emei_config.solver (the former reserved0; reserved words MUST be zero).
 * 3: the *_io stateless entry points (float64 observations), emei_freeze / emei_unfreeze snapshot the reset key,
 *    emei_model_constants, emei_get_solver_cap_hits.
 * 4: emei_model_invweights.
 * 5: emei_step_host (page-locked host values in and out; for n_envs == 1 of the 4-state family one launch whose last store is a
 *    completion word the library polls).
 * 6: emei_config.ode_method (classic control's ODE_approximation(method="rk4"), opt-in) and emei_config.rollout_chunk_steps
 *    (struct_size 408; a 400-byte caller gets euler / automatic), emei_get_rollout_faults, EMEI_NEXT_OBS_ODE_RK4.
 * 7: emei_set_obs_peers + emei_peer_buffer_create / open / close / destroy (multi-GPU observation return by peer writes from the
 *    rollout kernel), EMEI_KERNEL_PEND_STAGED_PEERS_FREQ1 / EMEI_KERNEL_PEND_STAGED_PEERS.
 * 8: emei_evaluate_sequences (K candidate action sequences per env scored from the current or a given state in one launch).
 *    Additive under 8 (no existing prototype or struct changes): emei_plan_shooting_workspace_bytes, emei_sample_candidates,
 *    emei_plan_shooting (random-shooting planning with the candidates drawn and arg-maxed on the device);
 *    emei_plan_mppi_workspace_bytes, emei_plan_mppi (the MPPI update of a nominal sequence: the return-weighted mean of the same
 *    candidates, redrawn on the device);
 *    emei_sample_candidates_sigma (the Gaussian candidates with a sigma per entry), emei_plan_cem_workspace_bytes, emei_plan_cem
 *    (one cross-entropy-method iteration: exact per-env selection of the n_elites best candidates on the device, their mean and
 *    standard deviation);
 *    emei_mpc_mppi_workspace_bytes, emei_mpc_mppi (receding-horizon MPPI control episodes of the 4-state family in one launch:
 *    plan, act, step, auto-reset and warm start per control step without leaving the device), EMEI_KERNEL_PEND_MPC_MPPI;
 *    emei_mpc_cem_workspace_bytes, emei_mpc_cem (the same control episodes with the cross-entropy method as the planner: `iterations`
 *    refits of emei_plan_cem per control step, the per-entry sigma kept on the device), EMEI_KERNEL_PEND_MPC_CEM;
 *    emei_mpc_mppi and emei_mpc_cem also serve the four InvertedDoublePendulum envs (any integrator, either precision, no
 *    observation noise) on kernels of the body family, EMEI_KERNEL_BODY_MPC_MPPI / EMEI_KERNEL_BODY_MPC_CEM;
 *    emei_rollout_policy with struct emei_policy (closed-loop rollouts under a small feedback policy a_t = pi(obs_t), one ReLU hidden
 *    layer or affine, evaluated per lane inside the rollout launch: every env on its family's kernel), EMEI_KERNEL_PEND_POLICY /
 *    EMEI_KERNEL_BODY_POLICY / EMEI_KERNEL_BODY_POLICY_RK4;
 *    emei_evaluate_policies (the policy-side counterpart of emei_evaluate_sequences: n_policies stacked struct emei_policy networks,
 *    each scored on every env from the envs' current or given states in one launch; the handle is untouched, no kernel id);
 *    emei_rollout_policy_noisy with struct emei_policy_noise (emei_rollout_policy with exploration noise drawn in the lanes: Gaussian
 *    with a given or a network-head standard deviation on the continuous envs, epsilon-greedy on the discrete ones),
 *    EMEI_KERNEL_PEND_POLICY_NOISY / EMEI_KERNEL_BODY_POLICY_NOISY / EMEI_KERNEL_BODY_POLICY_NOISY_RK4;
 *    emei_rollout_policy_deep and emei_evaluate_policies_deep with struct emei_policy_deep (the three policy calls for a network with
 *    two ReLU hidden layers of up to EMEI_POLICY_DEEP_MAX_HIDDEN units each; struct emei_policy and its entry points are unchanged),
 *    EMEI_KERNEL_PEND_POLICY_DEEP / EMEI_KERNEL_BODY_POLICY_DEEP / EMEI_KERNEL_BODY_POLICY_DEEP_RK4;
 *    emei_plan_policy_workspace_bytes, emei_plan_policy (shooting and MPPI around a feedback policy: n_candidates closed-loop rollouts
 *    of one struct emei_policy per env under struct emei_policy_noise, the policy evaluated in the lanes that score them; the handle
 *    is untouched, no kernel id);
 *    emei_plan_policy_deep (emei_plan_policy around a struct emei_policy_deep network, with an optional terminal value — a second
 *    struct emei_policy_deep with one output, added to the return of every candidate that never terminated; the workspace is
 *    emei_plan_policy_workspace_bytes'; the handle is untouched, no kernel id);
 *    emei_mpc_policy_workspace_bytes, emei_mpc_policy (policy-guided control episodes in one launch: per control step emei_plan_policy
 *    around a one-layer struct emei_policy under a noise seed that advances by seed_stride, the best or the weighted-mean first
 *    action, emei_step and auto-reset, for the envs emei_mpc_mppi serves), EMEI_KERNEL_PEND_MPC_POLICY / EMEI_KERNEL_BODY_MPC_POLICY
 *    in an enum of their own (enum emei_kernel_id_mpc_policy);
 *    emei_evaluate_sequences_value, emei_plan_shooting_value, emei_plan_mppi_value, emei_plan_cem_value and
 *    emei_plan_value_workspace_bytes (the four open-loop plan calls with emei_plan_policy_deep's terminal value — a struct
 *    emei_policy_deep with one output, added to the return of every candidate that never terminated; the handle is untouched, no
 *    kernel id). */
#define EMEI_ABI_VERSION 8

#if defined(__GNUC__)
#define EMEI_API __attribute__((visibility("default")))
#else
#define EMEI_API
#endif

/* Environments (reference classes). */
enum emei_env_id {
    EMEI_CARTPOLE_SWINGUP = 0,      /* emei/envs/classic_control/cartpole.py:135-156 */
    EMEI_CARTPOLE_BALANCING = 1,    /* emei/envs/classic_control/cartpole.py:115-132 */
    EMEI_IP_REBOUND_BALANCING = 2,  /* emei/envs/mujoco/inverted_pendulum.py:52-79   */
    EMEI_IP_BOUNDARY_BALANCING = 3, /* emei/envs/mujoco/inverted_pendulum.py:82-111  */
    EMEI_IP_REBOUND_SWINGUP = 4,    /* emei/envs/mujoco/inverted_pendulum.py:114-146 */
    EMEI_IP_BOUNDARY_SWINGUP = 5,   /* emei/envs/mujoco/inverted_pendulum.py:149-183 */
    EMEI_HALFCHEETAH_RUNNING = 6,   /* emei/envs/mujoco/half_cheetah.py:16-67        */
    EMEI_IDP_REBOUND_BALANCING = 7,  /* emei/envs/mujoco/inverted_double_pendulum.py:63-90   */
    EMEI_IDP_BOUNDARY_BALANCING = 8, /* emei/envs/mujoco/inverted_double_pendulum.py:93-123  */
    EMEI_IDP_REBOUND_SWINGUP = 9,    /* emei/envs/mujoco/inverted_double_pendulum.py:126-153 */
    EMEI_IDP_BOUNDARY_SWINGUP = 10,  /* emei/envs/mujoco/inverted_double_pendulum.py:156-196 */
    EMEI_HOPPER_RUNNING = 11,        /* emei/envs/mujoco/hopper.py:17-106 */
    EMEI_NUM_ENVS_IDS = 12
};

/* Arithmetic the kernels compute in.
 * REF  : float64 state and derivative, mirroring the reference's own precision (classic control:
 *        float64 accumulator += float32(derivative)*float32(dt), base_control.py:162-164 and
 *        cartpole.py:60; MuJoCo bodies: float64 throughout).  State arrays in HBM are float64.
 * F32  : float32 state and arithmetic (fast mode; not bit-faithful on long chaotic trajectories). */
enum emei_precision { EMEI_PRECISION_REF = 0, EMEI_PRECISION_F32 = 1 };

/* Time integrator of the MuJoCo-backed bodies (mujoco_env.py:70-79).  Classic control ignores the
 * kwarg exactly like the reference (base_control.py:73 never forwards `method`).
 * EULER          : MuJoCo Euler velocity update + emei's position override q += dt*v_old (:94-97,169-195)
 * SEMI_IMPLICIT  : MuJoCo Euler as it is: v' = v + dt*qacc, q += dt*v'
 * RK4            : MuJoCo's 4-stage Runge-Kutta (mjINT_RK4): full forward dynamics at every stage */
enum emei_integrator { EMEI_INTEG_EULER = 0, EMEI_INTEG_SEMI_IMPLICIT = 1, EMEI_INTEG_RK4 = 2 };

/* `method` of ODE_approximation for the classic-control envs (base_control.py:133-173).  The reference's step() never
 * passes it (:73), so every classic-control env is integrated with EULER whatever its `integrator` kwarg says — that stays the
 * default.  RK4 is the function's other branch (:165-170), reachable only by calling ODE_approximation directly; selecting it
 * here is an explicit opt-in and reproduces that branch's float32 / float64 promotion chain (k stages are float32 arrays,
 * the stage states float64).  Ignored by the MuJoCo-backed bodies (their switch is `integrator`). */
enum emei_ode_method { EMEI_ODE_EULER = 0, EMEI_ODE_RK4 = 1 };

/* How Gaussian init / observation noise is laid out over the coordinates of one env.
 * IID      : an independent draw per coordinate (the evident intent of additive_gaussian_noise)
 * SHARED   : what the reference actually does for its only working batch size, B = 1: the row
 *            slicing of mujoco_env.py:243-244 adds ONE draw to every qpos entry and ONE to every qvel */
enum emei_noise_layout { EMEI_NOISE_IID = 0, EMEI_NOISE_SHARED = 1 };

/* Constraint solver of the MuJoCo-backed bodies with several simultaneous constraints (HalfCheetah, Hopper):
 * NEWTON : MuJoCo's primal formulation as documented — one row per violated joint limit, the 2 (condim - 1) edges of the
 *          pyramidal friction cone per contact, regularisers from the qpos0 inverse weights — solved to convergence
 *          by Newton's method on the active set; Euler's implicit joint damping applied after the solve (the default)
 * SWEEP1 : one fixed-order Gauss-Seidel sweep with box-clamped friction (round 1; ~5x cheaper, kept for comparison) */
enum emei_solver { EMEI_SOLVER_NEWTON = 0, EMEI_SOLVER_SWEEP1 = 1 };

/* dtype of the `actions` argument of emei_step / emei_rollout. */
enum emei_action_dtype { EMEI_ACT_U8 = 0, EMEI_ACT_I32 = 1, EMEI_ACT_I64 = 2, EMEI_ACT_F32 = 3 };

/* flags of emei_step / emei_rollout */
#define EMEI_FLAG_AUTO_RESET 1u /* re-initialise an env on the device when done (terminal|truncated) */

/* done byte written by emei_step / emei_rollout */
#define EMEI_DONE_TERMINAL 1u  /* reference `terminal` (get_batch_terminal) */
#define EMEI_DONE_TRUNCATED 2u /* gym TimeLimit `truncated` (register_env.py max_episode_steps) */

/* error codes */
#define EMEI_OK 0
#define EMEI_ERR_INVALID -1     /* bad argument (the reference asserts / raises ValueError) */
#define EMEI_ERR_HIP -2         /* a HIP runtime call failed */
#define EMEI_ERR_UNSUPPORTED -3 /* the reference raises NotImplementedError here */
#define EMEI_ERR_STATE -4       /* call order: e.g. step before reset (base_control.py:67) */

#define EMEI_MAX_STATE_DIM 32
#define EMEI_MAX_ENV_PARAMS 8

/* Indices into env_params.  HalfCheetahRunning (half_cheetah.py:23-24) uses 0-1; HopperRunning
 * (hopper.py:25-31) uses 0-7.  Defaults: cheetah 1.0, 0.1; hopper 1.0, 1e-3, 1.0, 1 (True), -100, 100,
 * 0.7, +inf.  The Hopper's healthy_angle_range is accepted by the Python class and, as in the reference
 * (np.logical_and's third argument is `out=`, hopper.py:91), never applied. */
enum emei_env_param {
    EMEI_PARAM_FORWARD_REWARD_WEIGHT = 0,
    EMEI_PARAM_CTRL_COST_WEIGHT = 1,
    EMEI_PARAM_HEALTHY_REWARD = 2,
    EMEI_PARAM_TERMINATE_WHEN_UNHEALTHY = 3, /* 0 / 1 */
    EMEI_PARAM_HEALTHY_STATE_LO = 4,
    EMEI_PARAM_HEALTHY_STATE_HI = 5,
    EMEI_PARAM_HEALTHY_Z_LO = 6,
    EMEI_PARAM_HEALTHY_Z_HI = 7
};

typedef struct emei_env emei_env; /* opaque */

typedef struct emei_config {
    uint32_t struct_size;       /* = sizeof(emei_config), ABI evolution */
    int32_t env_id;             /* enum emei_env_id */
    int64_t n_envs;             /* env instances owned by this handle (this rank's shard) */
    int32_t freq_rate;          /* substeps per step (base_control.py:17, mujoco_env.py:42) */
    int32_t precision;          /* enum emei_precision */
    double real_time_scale;     /* dt of ONE substep; NOT divided by freq_rate (base_control.py:73) */
    int32_t max_episode_steps;  /* TimeLimit (register_env.py:14-66); 0 = never truncate */
    int32_t device;             /* HIP device ordinal */
    uint64_t seed;              /* key of the device-side reset generator */
    uint64_t env_index_offset;  /* global index of env 0 of this shard (results independent of sharding) */
    double init_noise;          /* sigma of the Gaussian init noise on qpos of the MuJoCo bodies (mujoco_env.py:31) */
    /* -- fields below exist from ABI version 2 (struct_size 328); a version-1 caller (struct_size 64)
     *    gets integrator = EULER, IID layout, init_sigma[*] = init_noise, no observation noise.  A
     *    version-2 caller states every sigma in the arrays; `init_noise` above is then ignored. ------ */
    int32_t integrator;         /* enum emei_integrator (mujoco_env.py:70-79) */
    int32_t noise_layout;       /* enum emei_noise_layout */
    /* Per-coordinate sigmas in state order (qpos entries, then qvel entries): the float, (pos, vel)
     * tuple and {joint: (pos, vel)} dict forms of init_noise_params / obs_noise_params
     * (mujoco_env.py:218-227) all reduce to this.  obs_sigma is the noise added to the state after
     * EVERY substep (mujoco_env.py:98-104); all zero = off.  With the SHARED layout only the entries
     * of joint 0 (index 0 and state_dim/2) are used, as in the reference. */
    float init_sigma[EMEI_MAX_STATE_DIM];
    float obs_sigma[EMEI_MAX_STATE_DIM];
    /* -- from struct_size 400: constructor parameters of the reward / terminal functions.  Bit k of
     *    env_param_mask set = env_params[k] overrides the reference's default (enum emei_env_param). ---- */
    uint32_t env_param_mask;
    uint32_t solver;            /* enum emei_solver (this field was `reserved0`, always 0, before) */
    double env_params[EMEI_MAX_ENV_PARAMS];
    /* -- from struct_size 408 (ABI 6) --------------------------------------------------------------------------------- */
    int32_t ode_method;          /* enum emei_ode_method: CartPole only (base_control.py:165-170); 0 = what step() runs */
    /* emei_rollout of the bodies that run one-wave blocks (HalfCheetah, Hopper with the NEWTON solver, the double pendulum):
     * the launch is cut into work items of (64 envs) x (a chunk of steps), handed out chunk-major by an atomic ticket to
     * persistent one-wave workers, so that a SIMD that finishes early takes the next item instead of idling until the slowest
     * wave of the launch ends; an env's state travels between its items through the handle's state arrays, results are
     * bit-identical to the one-piece launch.
     *   0 = automatic: on when the shard has more waves than the device holds at once, with the guided schedule (each chunk
     *       half of the steps that remain, at least three: long items first, short items last)
     *  -1 = off (one-piece launches)
     *   k > 0 = k steps per item
     *  -(100 m + g), m = 1 .. 15, g = 1 .. 6 = the guided schedule with 1 / 2^g of the remaining steps per chunk, at least m (tuning) */
    int32_t rollout_chunk_steps;
} emei_config;
#define EMEI_CONFIG_SIZE_V1 64u

/* -- lifecycle ------------------------------------------------------------------------------- */
/* Replaces Env.__init__(freq_rate, real_time_scale, integrator, ...) (base_control.py:14-30;
 * mujoco_env.py:24-62).  Allocates the state SoA on cfg->device. */
EMEI_API int emei_create(const emei_config* cfg, emei_env** out);
EMEI_API int emei_destroy(emei_env* h);
EMEI_API const char* emei_last_error(void);
EMEI_API int emei_abi_version(void);

/* Debug / test getter: the model constants the kernels of `env_id` are COMPILED from, in physical terms, so that a test
 * can pin them to the reference's only data for the MuJoCo-backed bodies (the XML files under emei/envs/mujoco/assets;
 * tests/test_model_constants.py).  Writes at most `capacity` doubles to `out`, returns the count (negative = error;
 * EMEI_ERR_UNSUPPORTED for the classic-control CartPole, whose constants are cartpole.py:22-27 literals).  Host only.
 *   InvertedPendulum x4 (17): gravity, cart mass, pole mass, pole inertia about its com, com distance from the hinge, tilt of
 *       the pole axis at theta = 0, gear, ctrlrange lo, hi, slider range lo, hi, limit solref time constant, solimp dmin, dmax, width,
 *       hinge range lo, hi (rad; a limit row of the Balancing variants, freed by the SwingUp variants)
 *   InvertedDoublePendulum x4 (17): gravity x, gravity z, cart mass, pole mass, pole inertia about its com, pole com distance,
 *       pole-1 length, gear, ctrlrange lo, hi, slider range lo, hi, joint margin, limit solref time constant, solimp dmin, dmax, width
 *   HalfCheetahRunning (148) / HopperRunning (84), nb = 7 / 4 bodies, ng = 8 / 4 capsules, nj = 6 / 3 actuated hinges:
 *       gravity; per body in XML order {mass, com x, com z (body frame), inertia about the com, origin x, origin z (parent frame;
 *       root: world)}; per capsule in XML order {body, end-sphere centre 0 x, z, centre 1 x, z (body frame), radius, pair friction
 *       with the floor}; per actuated joint {stiffness, damping, armature, range lo, hi (rad), gear}; contact margin, contact
 *       solref time constant, solimp dmin, dmax, width, limit solref time constant, solimp dmin, dmax, width, ctrlrange lo, hi,
 *       rootz ref, sign of the leg hinges' axis (+1: +y, -1: -y)
 *
 * WHICH FILE: these are the constants of emei's OWN XML files under emei/envs/mujoco/assets.  An installed reference passes a RELATIVE
 * model_path (inverted_pendulum.py:28, half_cheetah.py:48) to gym's MujocoEnv, which resolves it against GYM's assets directory —
 * gym's files are not in the build image, the fields in which they differ from emei's are unknown. */
EMEI_API int emei_model_constants(int env_id, double* out, int capacity);

/* Debug / test getter: the qpos0 inverse weights (MuJoCo's mj_setConst: dof_invweight0 = (M0^-1)_jj of a joint, body_invweight0 =
 * trace(J_com M0^-1 J_com') / 3 of a body) that scale the constraint regularisers R = (1 - d) / d * diagApprox of the kernels of
 * `env_id` — computed at compile time from the kernels' OWN model (absolute-angle inertia at qpos0), so that a test can compare
 * them with the oracle's joint-space derivation as two independent computations (tests/test_oracle_solver.py; what is being
 * restated: mujoco.mj_step behind mujoco_env.py:93).  Same calling convention as emei_model_constants.  Host only.
 *   InvertedPendulum x4 (2): slider, hinge.   InvertedDoublePendulum x4 (1): slider.
 *   HalfCheetahRunning (13): the six leg hinges in XML order, then the seven bodies in XML order.
 *   HopperRunning (7): thigh, leg, foot hinges, then torso, thigh, leg, foot bodies. */
EMEI_API int emei_model_invweights(int env_id, double* out, int capacity);

/* Static facts about an env id: obs_dim, act_dim (0 = discrete scalar action), state_dim. */
EMEI_API int emei_env_dims(int env_id, int* obs_dim, int* act_dim, int* state_dim);

/* -- reset / state --------------------------------------------------------------------------- */
/* Env.reset(seed=) on the device (base_control.py:38-47; mujoco_env.py:130-140): every env gets a
 * fresh initial state from the counter-based generator keyed by `seed`; step counters and episode
 * counters are zeroed.  (The reference's host PCG64 / MT19937 streams are reproduced on the host and
 * uploaded with emei_set_state when bit parity of the initial state is wanted.) */
EMEI_API int emei_reset(emei_env* h, uint64_t seed, void* stream);

/* Upload / download the internal state as a row-major [n_envs, state_dim] float64 array
 * (`self.state` of base_control.py:28,46,74; (qpos,qvel) of mujoco_env.py:116,132).
 * emei_set_state zeroes the step counters when reset_counters != 0. */
EMEI_API int emei_set_state(emei_env* h, const double* state_aos, int reset_counters, void* stream);
EMEI_API int emei_get_state(emei_env* h, double* state_aos, void* stream);
/* current observation as float64 [n_envs, obs_dim] (current_obs, mujoco_env.py:153-155;
 * inverted_pendulum.py:45-49) */
EMEI_API int emei_get_obs(emei_env* h, double* obs_aos, void* stream);

/* Freezable.freeze / unfreeze (base_control.py:32-36; mujoco_env.py:114-120): device-to-device
 * snapshot / restore of the state SoA, the counters and the key of the reset generator (so that the auto-reset episodes of
 * the restored trajectory draw what they would have drawn, whatever reset(seed=) happened in between). */
EMEI_API int emei_freeze(emei_env* h, void* stream);
EMEI_API int emei_unfreeze(emei_env* h, void* stream);

/* Newton solves of this handle's HalfCheetah / Hopper rollouts that ended at the iteration cap (24 passes) WITHOUT meeting their
 * stopping rule, since emei_create: count_out [1] uint64 (device-accessible).  The kernels' iteration takes unit Newton steps
 * without a line search; it has never been seen to need more than 9 passes, and this counter is how that is checked
 * (tests/test_gpu_parity_sweeps.py, tests/test_gpu_long_horizon.py assert 0).  Always 0 for the other envs and the SWEEP1 solver. */
EMEI_API int emei_get_solver_cap_hits(emei_env* h, uint64_t* count_out, void* stream);

/* Work items of this handle's chunked body rollouts (emei_config.rollout_chunk_steps) that gave up waiting for the item that
 * precedes them on the same envs (a bounded wait: 2 s of the device's 100 MHz counter) and were skipped, since emei_create:
 * count_out [1] uint64 (device-accessible).  Must stay 0 — an item's predecessor has always started before it (tickets are
 * handed out in start order); a non-zero count means a rollout's outputs are incomplete. */
EMEI_API int emei_get_rollout_faults(emei_env* h, uint64_t* count_out, void* stream);

/* Re-key the device reset generator without touching the state: the seed of Env.reset(seed=) reaches the
 * handle also when the initial state itself is drawn on the host and uploaded with emei_set_state
 * (base_control.py:38-47: gym seeds np_random, every later auto-reset episode must depend on it too). */
EMEI_API int emei_set_seed(emei_env* h, uint64_t seed);

/* -- the hot path ---------------------------------------------------------------------------- */
/* Env.step(action) for all n_envs instances (base_control.py:61-83; mujoco_env.py:157-167):
 *   actions   [n_envs] (discrete) or [n_envs, act_dim] (continuous), dtype per action_dtype
 *   obs_out   [n_envs, obs_dim] float32  next observation (before any auto-reset)
 *   reward_out[n_envs] float32
 *   done_out  [n_envs] uint8   EMEI_DONE_* bits
 * Any output pointer may be NULL to skip that output. */
EMEI_API int emei_step(emei_env* h, const void* actions, int action_dtype, float* obs_out, float* reward_out,
              uint8_t* done_out, uint32_t flags, void* stream);

/* The gym single-env call itself — `obs, reward, terminal, truncated, info = env.step(action)` of base_control.py:61-83 /
 * mujoco_env.py:157-167 with HOST values in and out — as one synchronous call: every pointer is page-locked host memory
 * that the device can address (hipHostMalloc / hipHostRegister / torch pin_memory), the kernels read the action from it
 * and write the results into it, and the function returns when the results are visible to the host.
 *   actions_host  as `actions` of emei_step
 *   obs64_host    [n_envs, obs_dim] float64: the observation of the STATE after the step (the float64 array the reference
 *                 returns; after an auto-reset the new episode's first observation, as emei_get_obs)
 *   obs32_host, reward_host, done_host: as emei_step (the step's own observation, before any auto-reset)
 * One launch and no stream synchronisation for a single env of the 4-state family (the kernel's last store is a completion
 * word the host polls); step + emei_get_obs + a stream synchronisation otherwise.  None of the pointers may be NULL. */
EMEI_API int emei_step_host(emei_env* h, const void* actions_host, int action_dtype, double* obs64_host, float* obs32_host,
                   float* reward_host, uint8_t* done_host, uint32_t flags, void* stream);

/* n_steps fused steps in ONE launch, state kept in registers (the caller loops of zoo/util.py:54-73
 * and emei/util.py:14-36 collapsed): actions [n_steps, n_envs(, act_dim)], obs_out
 * [n_steps, n_envs, obs_dim], reward_out [n_steps, n_envs], done_out [n_steps, n_envs].
 * Results are identical to n_steps calls of emei_step. */
EMEI_API int emei_rollout(emei_env* h, int32_t n_steps, const void* actions, int action_dtype, float* obs_out,
                 float* reward_out, uint8_t* done_out, uint32_t flags, void* stream);

/* Candidate action sequences scored from the envs' current states, for planners (random shooting, CEM, MPPI, or the true
 * dynamics as an "oracle model"): the query EmeiEnv serves model-based callers with freeze() "for rollout-test or query" and
 * get_batch_next_obs (core.py:18-37,190-193), fused — one launch, the state in registers, nothing per step written out.
 * Candidate (i, k), i < n_envs, k < n_candidates, starts from env i's start state: the handle's current state (start_state NULL)
 * or row i of start_state [n_envs, state_dim] float64 in emei_set_state's layout.  For t = 0 .. horizon - 1 it applies
 * actions[t, i, k] — [horizon, n_envs, n_candidates] (discrete) or [horizon, n_envs, n_candidates, act_dim] float32, dtype per
 * action_dtype as emei_rollout takes it — with exactly the arithmetic emei_rollout runs for this handle.  Outputs, [n_envs,
 * n_candidates] each:
 *   return_out    sum over t < L of discount^t * r_t: r_t is the step's reward as the rollout stores it (float32), widened; the
 *                 sum is accumulated in float64 in step order, discount^t a float64 running product from 1.0
 *   length_out    L = index of the first step whose terminal bit is set + 1, or horizon (the terminal step's reward counts)
 *   final_obs_out [n_envs, n_candidates, obs_dim] float32: the observation of step L - 1 as the rollout emits it (NULL: skipped)
 * No observation noise; TimeLimit counters, truncation and auto-reset are not consulted.  The handle is not touched (state,
 * counters, reset key, frozen snapshot); freeze() is not required.  horizon >= 1, n_candidates >= 1, 0 < discount <= 1 and
 * n_envs * n_candidates < 2^31, else EMEI_ERR_INVALID.  Newton solves that end at the iteration cap count into
 * emei_get_solver_cap_hits.  Neither allocates nor synchronises (capturable). */
EMEI_API int emei_evaluate_sequences(emei_env* h, int32_t horizon, int32_t n_candidates, const void* actions, int action_dtype,
                                     double discount, const double* start_state, double* return_out, int32_t* length_out,
                                     float* final_obs_out, void* stream);

/* Random-shooting planning on the true dynamics, the planner's answer to the query above (core.py:18-37,190-193: freeze() "for
 * rollout-test or query", get_batch_next_obs): the candidates are drawn in the lanes that score them and arg-maxed on the device,
 * so neither the [horizon, n_envs, n_candidates] actions nor the [n_envs, n_candidates] returns ever exist in memory.
 *
 * The candidates (normative).  Candidate (i, k) owns the 32-bit word stream
 *     W[m] = philox4x32_10(key = seed, counter = (g lo, g hi, k, m >> 2)).v[m & 3],   g = emei_config.env_index_offset + i
 * — Philox4x32-10 as the reset generator runs it, k in the counter word that has the episode there — and u(w) = (w >> 8) * 2^-24.
 * A sequence is a pure function of (seed, g, k): reproducible, independent of sharding, recoverable from k alone.
 *   discrete envs (act_dim 0): action[t] = u(W[t]) < p ? 1 : 0, p = 0.5 (nominal NULL: 1 - the top bit of W[t]) or
 *       nominal[t, i], float32 [horizon, n_envs] Bernoulli probabilities; sigma is ignored
 *   continuous, nominal NULL: action[t, a] = fmaf(u(W[t * act_dim + a]), hi - lo, lo) in float32, [lo, hi] the env's ctrlrange
 *       (the kernels' model constants: +-3 for the InvertedPendulum family, +-1 otherwise)
 *   continuous, nominal = float32 [horizon, n_envs, act_dim] means: c = t * act_dim + a, q = c >> 1, (z0, z1) = the reset
 *       generator's Box-Muller of (W[2q], W[2q + 1]), z = (c & 1) ? z1 : z0, action = min(max(fmaf((float)sigma, z, mean), lo), hi)
 *   continuous, nominal and a sigma_map = float32 [horizon, n_envs, act_dim] in nominal's layout (emei_sample_candidates_sigma,
 *       emei_plan_cem): the same z, action = min(max(fmaf(sigma_map[t, i, a], z, mean), lo), hi) — the map replaces the scalar.  An
 *       entry of 0 is legal and gives the clipped mean itself.  Negative or non-finite entries are the caller's error: the result for
 *       that env is unspecified, the call does not fault.
 *
 * emei_sample_candidates writes them out, actions_out [horizon, n_envs, n_candidates(, act_dim)] in emei_evaluate_sequences'
 * layout and in action_dtype (U8 / I32 / I64 for the discrete envs, F32 for the continuous ones): for tests and for callers that
 * want the sequences themselves.  It needs no state.
 *
 * emei_plan_shooting scores candidate (i, k) exactly as emei_evaluate_sequences scores those actions — the same start state
 * rule (start_state NULL: the handle's state), the per-step arithmetic of emei_rollout, ret = sum over t < L of discount^t *
 * (double)(float)r_t in step order, L = the first terminal step + 1 or horizon; no observation noise, TimeLimit or auto-reset; the
 * handle is untouched, its reset key included (seed is this call's own key) — and returns per env i
 *   best_index_out[i]      k*, the best candidate
 *   best_return_out[i]     ret(i, k*)
 *   best_length_out[i]     L(i, k*) (NULL: skipped)
 *   best_action_out[i(, :)]       candidate k*'s action at t = 0, in action_dtype
 *   best_sequence_out[t, i(, :)]  its whole sequence, [horizon, n_envs(, act_dim)] (NULL: skipped)
 * Order: candidate a beats b if ret_a > ret_b, or if ret_b is NaN and ret_a is not; otherwise the lower k wins.  k* is the first
 * index of the maximum, NaN counts as below everything (-inf included), all-NaN gives k* = 0 with a NaN return.  The result does
 * not depend on how an env's candidates fall onto waves or blocks.
 * workspace: emei_plan_shooting_workspace_bytes(n_envs, n_candidates) bytes of device memory, 16-byte aligned, contents
 * irrelevant before and after (one record per (wave, env) segment of the first of the call's two launches).
 * EMEI_ERR_INVALID before any HIP call, scalars first: horizon < 1, n_candidates < 1, discount outside (0, 1]; then a NULL
 * handle; nominal with sigma not finite or <= 0 on a continuous env; n_envs * n_candidates > 2^31 - 1 (or horizon * act_dim);
 * a wrong action_dtype; NULL workspace, best_action_out, best_return_out or best_index_out.  EMEI_ERR_STATE without a state.
 * Neither allocates nor synchronises (capturable).  Newton solves that end at the iteration cap count into
 * emei_get_solver_cap_hits. */
/* bytes of device scratch emei_plan_shooting needs for this shape; host only, no handle, no HIP call.
 * Negative (EMEI_ERR_INVALID) if n_envs < 1, n_candidates < 1 or n_envs * n_candidates > 2^31 - 1. */
EMEI_API int64_t emei_plan_shooting_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_sample_candidates(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                    double sigma, void* actions_out, int action_dtype, void* stream);
EMEI_API int emei_plan_shooting(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal, double sigma,
                                double discount, const double* start_state, void* workspace, void* best_action_out,
                                int action_dtype, void* best_sequence_out, double* best_return_out, int32_t* best_index_out,
                                int32_t* best_length_out, void* stream);

/* MPPI planning on the true dynamics (information-theoretic MPC; the planner-side use of the query core.py:18-37,190-193 serves):
 * the nominal sequence is replaced by the return-weighted (soft-max) mean of the candidates emei_plan_shooting would score.  A
 * candidate is a pure function of (seed, g, k), so a second pass redraws every candidate — no dynamics — and accumulates the
 * mean: nothing of size horizon * n_envs * n_candidates is ever stored (8 bytes per candidate are, in the workspace).
 *
 * Candidates, start-state rule, per-step arithmetic, return r_k = ret(i, k) and length are exactly emei_plan_shooting's for the
 * same (seed, nominal, sigma, discount, start_state), and (k*, r*) is its winner under the planner's order.  nominal NULL: fair
 * coins / uniform draws on the ctrlrange.
 *
 * Weights (normative), per env i, float64:
 *     r* is NaN (every return is NaN)                        w_k = 1 for all k
 *     otherwise, r_k is NaN                                  w_k = 0
 *     otherwise, r_k == r* (a +-inf maximum and all ties)    w_k = 1
 *     otherwise                                              w_k = exp((r_k - r*) / temperature)   (-inf gives 0)
 * hence Z = sum_k w_k >= 1.  Outputs:
 *   nominal_out[t, i(, a)]  float32 [horizon, n_envs(, act_dim)] in nominal's layout:
 *                           (float)(sum_k w_k * (double)action_k[t, a] / Z), action_k the float32 value of the candidate
 *                           specification above (0.f or 1.f for the discrete envs); sums and quotient in float64, one rounding to
 *                           float32.  A new mean inside the ctrlrange (continuous) or a Bernoulli probability in [0, 1] (discrete):
 *                           either is a valid `nominal` of the next call.  Required.  It may be the same pointer as nominal (in
 *                           place); any other overlap is undefined.  Entry (t, i, a) depends on nominal only at (t, i, a): it is
 *                           read before it is written, and no other env's entries are touched.
 *   best_index_out[i]       k*, and
 *   best_return_out[i]      r*: bit-identical to emei_plan_shooting's (either may be NULL)
 *   ess_out[i]              Z^2 / sum_k w_k^2, float64, the effective sample size (NULL: skipped)
 * Reproducibility: everything written for env i is a pure function of (seed, g = env_index_offset + i, n_candidates, horizon, env
 * i's nominal entries, sigma, r_.).  The summation tree depends on k only (candidates k = l mod 64 in ascending order, then a
 * butterfly over l) — not on how candidates fall onto waves or blocks, on n_envs or on the shard — so repeated calls, graph replays
 * and different shardings give the same bits (up to the lane dependence of r_k the HalfCheetah documents, 1e-9 relative).
 * workspace: emei_plan_mppi_workspace_bytes(n_envs, n_candidates) bytes of device memory, 16-byte aligned, contents irrelevant
 * before and after (emei_plan_shooting's records plus 8 bytes per candidate).
 * EMEI_ERR_INVALID before any HIP call, scalars first: horizon < 1, n_candidates < 1, discount outside (0, 1], temperature not
 * finite or <= 0; then a NULL handle; emei_plan_shooting's other checks (sigma with a nominal on a continuous env, n_envs *
 * n_candidates, horizon * act_dim); NULL workspace or nominal_out.  EMEI_ERR_STATE without a state.  The handle is untouched.
 * Neither allocates nor synchronises (capturable).  Newton solves that end at the iteration cap count into
 * emei_get_solver_cap_hits. */
/* bytes of device scratch emei_plan_mppi needs for this shape; host only, no handle, no HIP call.
 * Negative (EMEI_ERR_INVALID) where emei_plan_shooting_workspace_bytes is. */
EMEI_API int64_t emei_plan_mppi_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_plan_mppi(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal, double sigma,
                            double discount, double temperature, const double* start_state, void* workspace, float* nominal_out,
                            double* best_return_out, int32_t* best_index_out, double* ess_out, void* stream);

/* emei_sample_candidates for the Gaussian mode with a sigma per entry (the sigma_map clause of the candidate specification above):
 * actions_out float32 [horizon, n_envs, n_candidates, act_dim].  emei_sample_candidates' checks, and EMEI_ERR_INVALID for a NULL
 * nominal, a NULL sigma_map, or a discrete env. */
EMEI_API int emei_sample_candidates_sigma(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                          const float* sigma_map, void* actions_out, int action_dtype, void* stream);

/* One iteration of the cross-entropy method on the true dynamics (the planner of PETS / PlaNet-style MPC; the planner-side use of
 * the query core.py:18-37,190-193 serves): the sampling distribution (nominal, sigma) is refitted to the n_elites best of the
 * candidates emei_plan_shooting would score.  The elites are selected exactly and per env on the device and redrawn, so nothing of
 * size horizon * n_envs * n_candidates is ever stored (8 bytes per candidate are, in the workspace).
 *
 * Candidates, start-state rule, per-step arithmetic, return r_k = ret(i, k) and (k*, r*) are exactly emei_plan_shooting's for the
 * same (seed, nominal, sigma, discount, start_state); with a sigma_map, those of the sigma_map clause of the candidate
 * specification (nominal required, the scalar sigma ignored).
 *
 * The elite set (normative).  Per env i the n_candidates candidates are sorted by the planner's order: a comes before b if
 * ret_a > ret_b, or if ret_b is NaN and ret_a is not; otherwise the lower k comes first.  So +0.0 and -0.0 tie, all NaNs tie with
 * each other and come last, +-inf are ordinary values.  E_i is the first n_elites candidates of that sequence; it depends on the
 * returns and on k only — not on waves, blocks, n_envs or the shard.  (k*, r*) is its first member.
 *
 * The moments (normative), float64, a_k the float32 value of the candidate specification:
 *   discrete envs    mean_out[t, i] = (float)(sum_{k in E} a_k / n_elites), a_k in {0, 1}: a Bernoulli probability, the next call's
 *                    nominal.  std_out and sigma_map must be NULL, sigma is ignored.
 *   continuous envs  m0 = (double)nominal[t, i, a], or (double)(0.5f * (lo + hi)) with nominal NULL; d_k = (double)a_k - m0,
 *                    S1 = sum_{k in E} d_k, S2 = sum_{k in E} d_k^2 (the shifted one-pass form: meaningful when sigma has collapsed),
 *                    mean_out[t, i, a] = (float)(m0 + S1 / n_elites)
 *                    std_out[t, i, a]  = (float)sqrt(max(S2 / n_elites - (S1 / n_elites)^2, 0))   the population value; may be NULL
 *   Summation tree: emei_plan_mppi's — the members k = l mod 64 in ascending k, then a butterfly over the lanes l, distances 1, 2, .., 32 — a function
 *   of k alone, so repeated calls, graph replays and different shardings give the same bits (up to the lane dependence of r_k the
 *   HalfCheetah documents).
 * Outputs: mean_out, std_out float32 [horizon, n_envs(, act_dim)] in nominal's layout; mean_out may be the same pointer as nominal and
 * std_out the same pointer as sigma_map (in place: entry (t, i, a) of either is read before it is written, by env i's wave only); any
 * other overlap is undefined.
 *   best_index_out[i], best_return_out[i]  k*, r*: bit-identical to emei_plan_shooting's (either may be NULL)
 *   elite_return_out[i]                    the return of the LAST member of E_i, float64: the admission threshold; NaN if NaN returns
 *                                          had to be admitted (NULL: skipped)
 * workspace: emei_plan_cem_workspace_bytes(n_envs, n_candidates) bytes of device memory, 16-byte aligned, contents irrelevant before
 * and after (at least emei_plan_mppi's).
 * EMEI_ERR_INVALID before any HIP call, scalars first: horizon < 1, n_candidates < 1, n_elites < 1 or > n_candidates, discount outside
 * (0, 1]; then a NULL handle; emei_plan_shooting's candidate checks (with a nominal and no sigma_map on a continuous env, sigma finite
 * and > 0; n_envs * n_candidates; horizon * act_dim); a sigma_map without a nominal; a sigma_map or a std_out on a discrete env; NULL
 * workspace or mean_out.  EMEI_ERR_STATE without a state.  The handle is untouched.  Neither allocates nor synchronises (capturable).
 * Newton solves that end at the iteration cap count into emei_get_solver_cap_hits. */
/* bytes of device scratch emei_plan_cem needs for this shape; host only, no handle, no HIP call.
 * Negative (EMEI_ERR_INVALID) where emei_plan_mppi_workspace_bytes is. */
EMEI_API int64_t emei_plan_cem_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_plan_cem(emei_env* h, int32_t horizon, int32_t n_candidates, int32_t n_elites, uint64_t seed, const float* nominal,
                           double sigma, const float* sigma_map, double discount, const double* start_state, void* workspace,
                           float* mean_out, float* std_out, double* best_return_out, int32_t* best_index_out,
                           double* elite_return_out, void* stream);

/* Receding-horizon MPPI control on the true dynamics, whole episodes in ONE launch (plus a small one that packs the done mask): what
 * the loop "emei_plan_mppi, threshold / first entry, emei_step, shift the nominal" does in three launches and a handful of array
 * operations per control step.  For the 4-state family on its own kernels (CartPole, CartPoleRK4, InvertedPendulum with the euler
 * integrator and no observation noise) and for the InvertedDoublePendulum (all four envs, any integrator, either precision, init noise
 * in either layout, no observation noise; its observation row is six floats: obs_out is [n_steps, n_envs, 6]), where a plan is
 * microseconds of arithmetic and the loop is bound by launches.
 *
 * Semantics (normative).  For every env i and t = 0 .. n_steps - 1, m being env i's column of `nominal`:
 *   1. Clamp.  m[h(, a)] = fminf(fmaxf(m[h(, a)], nominal_lo), nominal_hi); -inf / +inf: no clamp.  Non-finite nominal entries are the
 *      caller's error: the results of that env are unspecified (the call does not fault).
 *   2. Plan.  Exactly emei_plan_mppi(h, horizon, n_candidates, seed + t (mod 2^64), nominal = m, sigma, discount, temperature,
 *      start_state = NULL, nominal_out = m) for env i: the same candidates (seed + t, g = env_index_offset + i, k), the same start
 *      state (the env's current one), returns, (k*, r*), weight case analysis and summation tree (lane l adds its candidates
 *      k = l, l + 64, .. in ascending order, then the butterfly d = 1 .. 32), one rounding to float32.
 *      plan_return_out[t, i] = r*, ess_out[t, i] as emei_plan_mppi's ess_out (float64 [n_steps, n_envs]; either may be NULL).
 *   3. Act.  Continuous envs: a_t = m[0, :]; discrete envs: a_t = (m[0] >= 0.5f) ? 1 : 0.  actions_out[t, i(, :)] in action_dtype
 *      (U8 / I32 / I64 discrete, F32 continuous), [n_steps, n_envs(, act_dim)].  Required.
 *   4. Step.  Exactly emei_step(a_t, flags) for env i, with emei_rollout's arithmetic: the TimeLimit counter, the EMEI_DONE_* bits
 *      and EMEI_FLAG_AUTO_RESET with the handle's reset key and episode counter.  obs_out / reward_out / done_out at [t, i] as
 *      emei_rollout writes them; any of the three may be NULL.
 *   5. Warm start.  The step was done and auto-reset is on: m[h] = refill for all h (a new episode gets no warm start).  Otherwise
 *      m[h] = m[h + 1] for h < horizon - 1 and m[horizon - 1] = refill.
 * After the call `nominal` (float32 [horizon, n_envs(, act_dim)], in/out, required) holds m after the last shift, ready for the next
 * call, and the handle is as after the equivalent loop: state, step and episode counters, the done mask emei_compact_done reads.
 * Every output is bit-identical to that loop's.
 * Consequences.  Chunking: n_steps = a + b in one call equals a call with (a, seed) followed by one with (b, seed + a) — a large
 * n_steps * n_candidates * horizon is ONE long kernel, and splitting it costs nothing but launches.  Sharding: results depend on g,
 * not on n_envs or the shard.  Stream: the call neither allocates nor synchronises (capturable).
 * Work split: one wave per env, its candidates spread over the 64 lanes; many candidates with few envs favour emei_plan_mppi's route,
 * which spreads all candidates over the device.
 * workspace: emei_mpc_mppi_workspace_bytes(n_envs, n_candidates) = 8 * n_envs * n_candidates bytes of device memory, 8-byte aligned,
 * contents irrelevant before and after.
 * EMEI_ERR_INVALID before any HIP call, scalars first, in this order: n_steps < 1, horizon < 1, n_candidates < 1; discount outside
 * (0, 1]; temperature not finite or <= 0; refill not finite, nominal_lo > nominal_hi or either NaN; horizon > EMEI_MPC_MAX_HORIZON
 * (the nominal lives in LDS); then a NULL handle; emei_plan_shooting's candidate checks (sigma finite and > 0 on a continuous env,
 * n_envs * n_candidates, a wrong action_dtype), unknown flags; NULL nominal, workspace or actions_out.  EMEI_ERR_STATE without a
 * state.  EMEI_ERR_UNSUPPORTED, the message naming the reason, for the other handles emei_rollout runs on the body kernels
 * (HalfCheetah, Hopper; InvertedPendulum with another integrator or observation noise), for an InvertedDoublePendulum handle with
 * observation noise (the plan steps the model without it) and for a handle with observation peers set (emei_set_obs_peers). */
#define EMEI_MPC_MAX_HORIZON 256
/* bytes of device scratch emei_mpc_mppi needs for this shape; host only, no handle, no HIP call.
 * Negative (EMEI_ERR_INVALID) where emei_plan_mppi_workspace_bytes is. */
EMEI_API int64_t emei_mpc_mppi_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_mpc_mppi(emei_env* h, int32_t n_steps, int32_t horizon, int32_t n_candidates, uint64_t seed, float* nominal,
                           double sigma, double discount, double temperature, float refill, float nominal_lo, float nominal_hi,
                           void* workspace, void* actions_out, int action_dtype, float* obs_out, float* reward_out, uint8_t* done_out,
                           double* plan_return_out, double* ess_out, uint32_t flags, void* stream);

/* Receding-horizon control with the cross-entropy method as the planner (PETS / PlaNet-style MPC on the true dynamics), whole episodes
 * in ONE launch (plus the small one that packs the done mask): what the loop "`iterations` times emei_plan_cem in place, first entry,
 * emei_step, shift the mean" does in 2 * iterations + 1 launches and a handful of array operations per control step.  The same envs
 * as emei_mpc_mppi: the 4-state family on its own kernels, and the InvertedDoublePendulum without observation noise (obs_out
 * [n_steps, n_envs, 6]: its observation row is six floats).
 *
 * Semantics (normative).  For every env i and t = 0 .. n_steps - 1, m being env i's column of `nominal` and, on continuous envs, s a
 * per-entry sigma column of the same shape that lives only inside the call:
 *   1. Iterate.  For j = 0 .. iterations - 1:
 *      (a) Clamp.  m[h(, a)] = fminf(fmaxf(m[h(, a)], nominal_lo), nominal_hi); -inf / +inf: no clamp.
 *      (b) Continuous envs, j = 0 only: s[h, a] = (float)sigma — the distribution's width is reset at every control step, only the
 *          mean is warm-started.
 *      (c) Refit.  Exactly emei_plan_cem(h, horizon, n_candidates, n_elites, seed + t*iterations + j (mod 2^64), nominal = m,
 *          sigma_map = s (continuous) / NULL (discrete), discount, start_state = NULL, mean_out = m, std_out = s / NULL) for env i: the
 *          same candidates (the sigma_map clause of the candidate specification; g = env_index_offset + i), the same start state (the
 *          env's current one), returns, planner's order and elite set E_i, shifted moments and summation tree (lane l adds its
 *          members k = l, l + 64, .. in ascending order, then the butterfly d = 1 .. 32), one rounding to float32.
 *      (d) Continuous envs: s[h, a] = fmaxf(s[h, a], (float)sigma_min); sigma_min = 0: no floor.
 *      After the last iteration plan_return_out[t, i] = r* and elite_return_out[t, i] = the admission threshold, as emei_plan_cem's
 *      best_return_out and elite_return_out (float64 [n_steps, n_envs]; either may be NULL).
 *   2. Act.  Continuous envs: a_t = m[0, :]; discrete envs: a_t = (m[0] >= 0.5f) ? 1 : 0.  actions_out[t, i(, :)] in action_dtype
 *      (U8 / I32 / I64 discrete, F32 continuous), [n_steps, n_envs(, act_dim)].  Required.
 *   3. Step.  Exactly emei_step(a_t, flags) for env i, with emei_rollout's arithmetic: the TimeLimit counter, the EMEI_DONE_* bits
 *      and EMEI_FLAG_AUTO_RESET with the handle's reset key and episode counter.  obs_out / reward_out / done_out at [t, i] as
 *      emei_rollout writes them; any of the three may be NULL.
 *   4. Warm start.  The step was done and auto-reset is on: m[h] = refill for all h (a new episode gets no warm start).  Otherwise
 *      m[h] = m[h + 1] for h < horizon - 1 and m[horizon - 1] = refill.
 * After the call `nominal` (float32 [horizon, n_envs(, act_dim)], in/out, required) holds m after the last shift, and the handle is as
 * after the equivalent loop: state, step and episode counters, the done mask emei_compact_done reads.  Every output is bit-identical
 * to that loop's.
 * Consequences.  Chunking: n_steps = a + b in one call equals a call with (a, seed) followed by one with (b, seed + a*iterations).
 * Sharding: results depend on g, not on n_envs or the shard.  Stream: the call neither allocates nor synchronises (capturable).
 * Non-finite nominal entries are the caller's error: the results of that env are unspecified (the call does not fault).  Smoothing of
 * the mean and elites kept across iterations are out of scope: emei_plan_cem's two-launch route serves them.
 * Work split: one wave per env, as emei_mpc_mppi.
 * workspace: emei_mpc_cem_workspace_bytes(n_envs, n_candidates) = 8 * n_envs * n_candidates bytes of device memory, 8-byte aligned,
 * contents irrelevant before and after.
 * EMEI_ERR_INVALID before any HIP call, scalars first, in this order: n_steps < 1, horizon < 1, n_candidates < 1, n_elites outside
 * [1, n_candidates], discount outside (0, 1], iterations < 1, refill not finite, nominal_lo > nominal_hi or either NaN, sigma_min not
 * finite or < 0, horizon > EMEI_MPC_MAX_HORIZON (the mean and the sigma live in LDS); then a NULL handle; emei_plan_shooting's
 * candidate checks (sigma finite and > 0 on a continuous env, n_envs * n_candidates), a wrong action_dtype, unknown flags; NULL
 * nominal, workspace or actions_out.  EMEI_ERR_STATE without a state.  EMEI_ERR_UNSUPPORTED exactly where emei_mpc_mppi gives it:
 * a handle emei_rollout runs on the body kernels other than an InvertedDoublePendulum without observation noise, and a handle with
 * observation peers set. */
/* bytes of device scratch emei_mpc_cem needs for this shape; host only, no handle, no HIP call.
 * Negative (EMEI_ERR_INVALID) where emei_plan_mppi_workspace_bytes is. */
EMEI_API int64_t emei_mpc_cem_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_mpc_cem(emei_env* h, int32_t n_steps, int32_t horizon, int32_t n_candidates, int32_t n_elites, int32_t iterations,
                          uint64_t seed, float* nominal, double sigma, double sigma_min, double discount, float refill,
                          float nominal_lo, float nominal_hi, void* workspace, void* actions_out, int action_dtype,
                          float* obs_out, float* reward_out, uint8_t* done_out, double* plan_return_out, double* elite_return_out,
                          uint32_t flags, void* stream);

/* Closed-loop rollouts under a feedback policy a_t = pi(obs_t), n_steps env-steps in ONE launch: what the agent.predict loop of
 * zoo/util.py:54-73 does with one emei_get_obs / emei_episode_init_obs, the policy's own launches and one emei_step per step.  The policy
 * is a small network — one ReLU hidden layer, or affine — evaluated per lane inside the rollout kernel; the weights are the same for
 * every env and are read through wave-uniform addresses (scalar loads).  They are DEVICE pointers, read during the launch and not
 * retained; they must not overlap any output of the call.
 *
 * Semantics (normative).  For every env i and t = 0 .. n_steps - 1:
 *   1. Observe.  x_0 is row i of emei_get_obs, rounded to float32.  For t > 0, x_t is the observation row of step t - 1 as
 *      emei_rollout writes it; if that step was done under EMEI_FLAG_AUTO_RESET, x_t is instead what emei_episode_init_obs gives for
 *      (i, the new episode).  Observation noise, where the handle has it, is in the row as the rollout emits it.
 *   2. Policy.  All sums run in ascending index order, in float64 (a product of two float32 values is exact in float64, so fused and
 *      unfused multiply-add give the same bits).
 *        hidden > 0: for j ascending, z = (double)b1[j]; for k ascending, z = z + (double)w1[j,k] * (double)x[k]; h_j = (float)z;
 *                    h_j = h_j > 0.f ? h_j : 0.f (NaN gives 0).
 *        hidden == 0: h = x.
 *        y_q = (double)b2[q]; for j ascending, y_q = y_q + (double)w2[q,j] * (double)h_j.
 *        continuous envs, EMEI_POLICY_OUT_CLIP: a_q = fminf(fmaxf((float)y_q, lo), hi), [lo, hi] the ctrlrange of the candidate
 *                    specification above (+-3 for the InvertedPendulum family, +-1 otherwise); NaN gives lo.
 *        continuous envs, EMEI_POLICY_OUT_TANH: a_q = (float)(0.5*(hi+lo) + 0.5*(hi-lo) * tanh(y_q)) in float64, the device's float64
 *                    tanh: this mode is NOT pinned bit for bit (within one float32 spacing at max(|lo|, |hi|) of a correctly rounded tanh).
 *        discrete envs: a = y_0 >= 0 ? 1 : 0 (NaN gives 0); out_mode is ignored.
 *      actions_out[t, i(, :)] in action_dtype (U8 / I32 / I64 for the discrete envs, F32 for the continuous ones),
 *      [n_steps, n_envs(, act_dim)].
 *   3. Step.  Exactly emei_step(a_t, flags) for env i, with emei_rollout's arithmetic: the TimeLimit counter, the EMEI_DONE_* bits,
 *      EMEI_FLAG_AUTO_RESET with the handle's reset key and episode counter, the observation-noise counters; obs_out / reward_out /
 *      done_out at [t, i] as emei_rollout writes them.
 * Each of the four outputs may be NULL.  After the call the handle is as after the equivalent loop: state, step and episode counters,
 * the done mask emei_compact_done reads.
 * Consequences.  Replay: feeding actions_out to emei_rollout from the same start reproduces the other three outputs bit for bit.
 * Chunking: n_steps = a + b in one call equals two calls wherever (float)emei_get_obs equals the row the last step emitted (the second
 * call observes the state, the single call the emitted row).  Sharding: results depend on the global env index, not on the shard.
 * Stream: the call neither allocates nor synchronises (capturable).
 * Kernels: pend_policy_rollout_kernel for every handle emei_rollout runs on the 4-state family's kernels (the loop of the generic
 * pend_rollout_kernel, any n, any n_steps); body_policy_rollout_kernel for every handle on the body kernels, always as a one-piece
 * launch: the chunked work-queue launch (emei_config.rollout_chunk_steps) is NOT used by this call.
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: n_steps < 1; NULL policy; struct_size wrong;
 * hidden < 0 or > EMEI_POLICY_MAX_HIDDEN; unknown out_mode; reserved != 0; a NULL handle; NULL w2 or b2; hidden > 0 with NULL w1 or
 * b1; a wrong action_dtype; unknown flags.  EMEI_ERR_STATE without a state.  EMEI_ERR_UNSUPPORTED for a handle with observation peers
 * set (emei_set_obs_peers). */
enum emei_policy_out { EMEI_POLICY_OUT_CLIP = 0, EMEI_POLICY_OUT_TANH = 1 };
#define EMEI_POLICY_MAX_HIDDEN 1024
typedef struct emei_policy {
    uint32_t struct_size;   /* = sizeof(emei_policy) */
    int32_t hidden;         /* width of the one hidden layer (ReLU); 0 = an affine policy */
    int32_t out_mode;       /* enum emei_policy_out; ignored by the discrete envs */
    int32_t reserved;       /* must be 0 */
    const float* w1;        /* [hidden, obs_dim] row-major; NULL when hidden == 0 */
    const float* b1;        /* [hidden];                    NULL when hidden == 0 */
    const float* w2;        /* [n_out, hidden], or [n_out, obs_dim] when hidden == 0 */
    const float* b2;        /* [n_out];  n_out = act_dim, or 1 for the discrete envs */
} emei_policy;
EMEI_API int emei_rollout_policy(emei_env* h, int32_t n_steps, const emei_policy* policy, void* actions_out, int action_dtype,
                                 float* obs_out, float* reward_out, uint8_t* done_out, uint32_t flags, void* stream);

/* emei_rollout_policy under a STOCHASTIC behaviour policy, the way every policy dataset of the reference's zoo is sampled
 * (zoo/main.py:109-122, zoo/util.py:56: agent.predict(obs, deterministic=False)): Gaussian exploration on the continuous envs,
 * epsilon-greedy on the discrete ones.  The noise is drawn inside the lanes from a counter-based stream and never exists in memory.
 * std / ws / bs are DEVICE pointers like the weights: read during the launch, not retained, not overlapping any output.
 *
 * Semantics (normative).  Everything is emei_rollout_policy's clause list (Observe, Policy, Step), its outputs and the state it leaves
 * in the handle, with one addition to clause 2.
 *   Noise words.  Step t of the call, for env i with g = env_index_offset + i, owns the word stream
 *        W[m] = philox4x32_10(key = seed + t (mod 2^64), counter = (g lo, g hi, 0, m >> 2)).v[m & 3]
 *      — the stream of candidate k = 0 of the candidate specification above under the key seed + t: a pure function of (seed, t, g),
 *      independent of the shard, of n_envs, of episodes and of auto-resets.  A planner call (emei_sample_candidates, emei_plan_*,
 *      emei_mpc_*) given the same key draws candidate 0 of env g from the same words; that coincidence is harmless (the two calls
 *      consume the words for different purposes, and neither reads the other's results), but distinct seeds keep them independent.
 *   Continuous envs, EMEI_POLICY_NOISE_GAUSS and EMEI_POLICY_NOISE_GAUSS_HEAD.  For component q, p = q >> 1 and (z0, z1) = the reset
 *      generator's Box-Muller of (W[2p], W[2p + 1]); z_q = (q & 1) ? z1 : z0 — the normals the candidate specification draws at step 0.
 *      After the ascending sum that gives y_q one more term is added, last:  y_q = y_q + (double)s_q * (double)z_q  (a product of two
 *      float32 values, exact in float64).  The output clause (CLIP or TANH, with its NaN handling) then acts on that y_q, unchanged:
 *      under CLIP Gaussian exploration on a deterministic actor (TD3, DDPG) or a PPO Gaussian, under TANH SAC's squashed Gaussian.
 *        GAUSS: s_q = std[q], or (float)sigma when std is NULL.  Entries are used as they are; a non-finite entry gives a non-finite
 *               y_q, which the output clause handles (the call does not fault).
 *        GAUSS_HEAD: l_q = (double)bs[q]; for j ascending, l_q = l_q + (double)ws[q,j] * (double)h_j, h the hidden activations y_q
 *               uses (hidden == 0: the inputs x); s_q = (float)exp(fmin(fmax(l_q, (double)log_std_min), (double)log_std_max)), the
 *               device's float64 exp: this mode is NOT pinned bit for bit, like EMEI_POLICY_OUT_TANH.
 *   Discrete envs, EMEI_POLICY_NOISE_EPS_GREEDY.  With u(w) = (w >> 8) * 2^-24: explore = u(W[0]) < (float)sigma;
 *      a = explore ? (u(W[1]) < 0.5f ? 1 : 0) : (y_0 >= 0 ? 1 : 0) — the candidate specification's discrete draws at t = 0 with
 *      p = epsilon and at t = 1 with p = 0.5.
 * Consequences.  Replay: emei_rollout(actions_out) reproduces the other outputs bit for bit in every mode.  Chunking: n_steps = a + b
 * equals a call with (a, seed) followed by one with (b, seed + a), under emei_rollout_policy's observation condition.  Sharding:
 * results depend on g only.  Stream: the call neither allocates nor synchronises.  With s_q = 0 for all q, or epsilon 0, the actions
 * equal emei_rollout_policy's as values.
 * Kernels: pend_policy_rollout_noisy_kernel / body_policy_rollout_noisy_kernel, emei_rollout_policy's kernels with the noisy
 * evaluation; the action of step t + 1 of the body kernel is computed at the end of step t under the key seed + t + 1.
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: emei_rollout_policy's checks up to and
 * including policy.reserved; NULL noise; noise.struct_size wrong; unknown noise.mode; noise.reserved != 0; GAUSS with std NULL: sigma
 * not finite or < 0; EPS_GREEDY: sigma outside [0, 1] or NaN; GAUSS_HEAD: log_std_min > log_std_max or either NaN, then NULL ws or bs;
 * a NULL handle; emei_rollout_policy's weight, dtype and flag checks; a GAUSS mode on a discrete env or EPS_GREEDY on a continuous
 * one.  EMEI_ERR_STATE and EMEI_ERR_UNSUPPORTED where emei_rollout_policy gives them. */
enum emei_policy_noise_mode {
    EMEI_POLICY_NOISE_GAUSS = 0,       /* continuous envs: a std per action component, given */
    EMEI_POLICY_NOISE_GAUSS_HEAD = 1,  /* continuous envs: the std from a log-std head next to the output layer (SAC's actor) */
    EMEI_POLICY_NOISE_EPS_GREEDY = 2   /* discrete envs */
};
typedef struct emei_policy_noise {
    uint32_t struct_size;   /* = sizeof(emei_policy_noise) */
    int32_t mode;           /* enum emei_policy_noise_mode */
    uint64_t seed;          /* this call's own key; the handle's reset key is not involved */
    double sigma;           /* GAUSS with std NULL: the std of every component, finite, >= 0.  EPS_GREEDY: epsilon in [0, 1] */
    const float* std;       /* GAUSS: [n_out] device floats, or NULL (then sigma) */
    const float* ws;        /* GAUSS_HEAD: [n_out, hidden] ([n_out, obs_dim] when hidden == 0), laid out as w2 */
    const float* bs;        /* GAUSS_HEAD: [n_out] */
    float log_std_min, log_std_max;   /* GAUSS_HEAD: clamp of the head's output (SAC: -20, 2); min <= max, neither NaN */
    int32_t reserved;       /* 0 */
} emei_policy_noise;
EMEI_API int emei_rollout_policy_noisy(emei_env* h, int32_t n_steps, const emei_policy* policy, const emei_policy_noise* noise,
                                       void* actions_out, int action_dtype, float* obs_out, float* reward_out, uint8_t* done_out,
                                       uint32_t flags, void* stream);

/* A population of feedback policies scored from the envs' current states in ONE launch, for policy search (evolution strategies and
 * ARS over perturbed policies, CEM over policy weights, population-based training, choosing among checkpoints): the policy-side
 * counterpart of emei_evaluate_sequences.  `stacked` is a struct emei_policy whose pointers each name P = n_policies networks laid end
 * to end — w1 [P, hidden, obs_dim], b1 [P, hidden], w2 [P, n_out, hidden] ([P, n_out, obs_dim] when hidden == 0), b2 [P, n_out] —
 * with hidden and out_mode shared by the population.  DEVICE pointers, read during the launch and not retained; they must not overlap
 * any output of the call.
 *
 * Semantics (normative).  For every pair (p, i), p < n_policies, i < n_envs, and t = 0 .. horizon - 1:
 *   1. Start.  The pair starts from env i's start state, emei_evaluate_sequences' rule: the handle's current state (start_state NULL)
 *      or row i of start_state [n_envs, state_dim] float64 in emei_set_state's layout, narrowed as emei_set_state narrows it.
 *   2. Observe.  x_0 is the observation of that state as emei_get_obs gives it, rounded to float32.  For t > 0, x_t is the float32
 *      observation row that step t - 1 emits.
 *   3. Policy.  a_t = pi_p(x_t): exactly clause 2 ("Policy") of emei_rollout_policy with member p's weights — float64 sums in
 *      ascending index order, the hidden unit rounded to float32 before the ReLU, the clip / tanh / threshold output and its NaN handling.
 *   4. Step and score.  The per-step arithmetic emei_rollout runs for this handle, scored as emei_evaluate_sequences scores:
 *      ret = sum over t < L of discount^t * (double)(float)r_t, accumulated in float64 in step order, discount^t a float64 running
 *      product from 1.0; L = index of the first step whose terminal bit is set + 1, or horizon (the terminal step's reward counts).
 *      A pair past its terminal step keeps stepping without accumulating; its wave leaves once none of its pairs is live.
 * Not consulted: observation noise, the TimeLimit counters, truncation and auto-reset.  The handle is untouched: state, counters,
 * reset key, frozen snapshot, the done mask emei_compact_done reads and emei_last_rollout_kernel.  Newton solves that end at the
 * iteration cap count into emei_get_solver_cap_hits, as for the other queries.
 * Outputs, policy-major:
 *   return_out    [n_policies, n_envs] float64: ret.  Required.
 *   length_out    [n_policies, n_envs] int32: L.  May be NULL.
 *   final_obs_out [n_policies, n_envs, obs_dim] float32: the observation row of step L - 1.  May be NULL.
 * Consequences.  Replay: candidate k = p of emei_evaluate_sequences, fed the actions_out of an emei_rollout_policy run with policy p
 * from the same start and without EMEI_FLAG_AUTO_RESET, has the same return, length and final observation — bit for bit under
 * EMEI_POLICY_OUT_CLIP and on the discrete envs, up to the HalfCheetah's lane lending (its wave-mates differ between the two calls).
 * Sharding: results depend on the global env index, not on the shard.  Stream: the call neither allocates nor synchronises
 * (capturable).
 * Kernels: pend_policy_eval_kernel for every handle emei_rollout runs on the 4-state family's kernels, body_policy_eval_kernel for
 * every handle on the body kernels.  One lane per pair; a block serves one policy (block b: policy b / nb, env block b % nb with
 * nb = ceil(n_envs / 256)), so the weights are read through wave-uniform addresses (scalar loads), and wave w of a policy holds envs
 * 64 w .. 64 w + 63 as in emei_rollout_policy.
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: horizon < 1; n_policies < 1; discount outside
 * (0, 1]; NULL stacked; struct_size wrong; hidden < 0 or > EMEI_POLICY_MAX_HIDDEN; unknown out_mode; reserved != 0; a NULL handle;
 * NULL w2 or b2; hidden > 0 with NULL w1 or b1; NULL return_out; n_envs * n_policies > 2^31 - 1, or more than 2^31 - 1 blocks.
 * EMEI_ERR_STATE without a state and without start_state. */
EMEI_API int emei_evaluate_policies(emei_env* h, int32_t horizon, int32_t n_policies, const emei_policy* stacked, double discount,
                                    const double* start_state, double* return_out, int32_t* length_out, float* final_obs_out,
                                    void* stream);

/* Planning around a feedback policy, the planner of model-based offline RL (MBOP, LOOP, POLO; the policy-prior half of POPLIN and
 * TD-MPC): per env, n_candidates CLOSED-LOOP rollouts of one policy under exploration noise from the env's start state, scored on the
 * true dynamics, and the best or the return-weighted first action.  emei_plan_shooting and emei_plan_mppi draw their candidates around
 * an open-loop nominal; here the candidate is the policy itself reacting to every observation of its own rollout, evaluated in the
 * lane that scores it: the [horizon, n_envs, n_candidates] actions never exist in memory.  `policy` and `noise` are
 * emei_rollout_policy_noisy's structs with DEVICE pointers, read during the launches and not retained; they must not overlap any
 * output or the workspace.
 *
 * Semantics (normative).  Candidate (i, k), i < n_envs, k < n_candidates, g = env_index_offset + i, is a rollout of `horizon` steps:
 *   1. Start and observe.  Clauses 1 and 2 of emei_evaluate_policies: the start is the handle's current state (start_state NULL) or
 *      row i of start_state [n_envs, state_dim] float64, narrowed as emei_set_state narrows it; x_0 is the float32 observation of that
 *      state, x_t the float32 observation row that step t - 1 emits.
 *   2. Policy.  a_t = clause 2 ("Policy") of emei_rollout_policy with the noise clause of emei_rollout_policy_noisy, where step t of
 *      candidate k owns the word stream
 *          W[m] = philox4x32_10(key = seed + t (mod 2^64), counter = (g lo, g hi, k, m >> 2)).v[m & 3]
 *      — the noisy rollout's stream with k in the counter word that holds 0 there.  All three noise modes are served: GAUSS with std
 *      or sigma, GAUSS_HEAD, EPS_GREEDY.
 *      Candidate 0 takes NO noise: its y_q is the deterministic one (selected after the draw, not by a zero std: a y_q of -0.0 keeps
 *      its sign, a non-finite std does not reach it), and on a discrete env it never explores.  Candidate 0 is the prior itself, so
 *      the plan is never worse than the policy under the model.  (The words of candidate 0 are the ones emei_rollout_policy_noisy
 *      would consume under the same seed; this call does not use them.)
 *   3. Step and score.  Clause 4 of emei_evaluate_policies: the per-step arithmetic emei_rollout runs for this handle; ret(i, k) = sum
 *      over t < L of discount^t * (double)(float)r_t, float64 in step order, discount^t a float64 running product from 1.0; L(i, k) =
 *      the first terminal step + 1, or horizon.  No observation noise, no TimeLimit, no auto-reset.  A candidate past its terminal
 *      step keeps stepping without accumulating; a wave leaves once none of its lanes is live.
 *   4. Select.  (k*, r*) is the first candidate under the planner's order (emei_plan_shooting): ret_a > ret_b wins, NaN comes last,
 *      ties go to the lower k.
 *   5. Weights.  emei_plan_mppi's case analysis with `temperature` on r_k = ret(i, k), and its summation tree: lane l adds the
 *      candidates k = l, l + 64, .. in ascending order, then a butterfly over the lanes with d = 1, 2, .., 32 — a function of k alone.
 * Outputs, per env i:
 *   best_action_out[i(, :)]  candidate k*'s action at t = 0, in action_dtype (U8 / I32 / I64 discrete, F32 continuous).  Required.
 *   mean_action_out[i(, a)]  float32 [n_envs(, act_dim)]: (float)(sum_k w_k * (double)a_k[0, a] / Z), a_k[0, :] candidate k's float32
 *                            action at t = 0 (0.f / 1.f on the discrete envs: the weighted share of action 1); sums and quotient in
 *                            float64, one rounding.  NULL: skipped.
 *   best_return_out[i], best_index_out[i], best_length_out[i]   r*, k*, L(i, k*).  Each may be NULL.
 *   return_out[i, k]         float64 [n_envs, n_candidates]: ret(i, k).  May be NULL.
 *   ess_out[i]               Z^2 / sum_k w_k^2, float64.  May be NULL.
 * With mean_action_out and ess_out both NULL no weights are formed and `temperature` is neither consulted nor checked.
 * Consequences.  Sharding: results depend on g, not on the shard (up to the lane dependence of r_k the HalfCheetah documents, 1e-9
 * relative).  Stream: the call neither allocates nor synchronises (capturable); repeated calls and graph replays give the same bits.
 * Candidate 0 equals emei_evaluate_policies with n_policies = 1 on the same policy, start and discount (return and length; bit for bit
 * except for the HalfCheetah's lane lending).  n_candidates = 1 is legal: the deterministic policy's first action, return and length.
 * The actions of candidate k are those the per-step loop "observe, evaluate the policy with candidate k's noise, emei_step" takes;
 * fed to emei_evaluate_sequences they give return_out and the lengths.  The handle is untouched: state, counters, reset key, frozen
 * snapshot, the done mask and emei_last_rollout_kernel.  Newton solves that end at the iteration cap count into
 * emei_get_solver_cap_hits, as for the other queries.
 * Kernels: pend_policy_plan_kernel / body_policy_plan_kernel — the DRAWN + KEEP loop of the family's plan kernel, one lane per
 * candidate j = i * n_candidates + k, the weights read through wave-uniform addresses (scalar loads) — then
 * plan_policy_finish_kernel, one wave per env.  EMEI_POLICY_OUT_TANH and EMEI_POLICY_NOISE_GAUSS_HEAD are not pinned bit for bit, as
 * in the rollouts.
 * workspace: emei_plan_policy_workspace_bytes(n_envs, n_candidates) bytes of device memory, 16-byte aligned, contents irrelevant
 * before and after.  The first launch STORES every candidate's action of step 0 (the finish launch reads them back instead of
 * evaluating the policy again), so the workspace is emei_plan_mppi's plus 24 bytes per candidate (six float32 slots, the widest
 * action of the envs: the function takes no handle).
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: horizon < 1; n_candidates < 1; discount
 * outside (0, 1]; with a non-NULL mean_action_out or ess_out, temperature not finite or <= 0; emei_rollout_policy's struct checks up
 * to and including policy.reserved; NULL noise, then emei_rollout_policy_noisy's noise checks in their order; a NULL handle; NULL w2 or
 * b2, hidden > 0 with NULL w1 or b1; n_envs * n_candidates > 2^31 - 1; a wrong action_dtype; NULL workspace, then NULL
 * best_action_out; a GAUSS mode on a discrete env or EPS_GREEDY on a continuous one.  EMEI_ERR_STATE without a state and without
 * start_state. */
/* bytes of device scratch emei_plan_policy needs for this shape; host only, no handle, no HIP call.
 * Negative (EMEI_ERR_INVALID) where emei_plan_shooting_workspace_bytes is. */
EMEI_API int64_t emei_plan_policy_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_plan_policy(emei_env* h, int32_t horizon, int32_t n_candidates, const emei_policy* policy,
                              const emei_policy_noise* noise, double discount, double temperature, const double* start_state,
                              void* workspace, void* best_action_out, int action_dtype, float* mean_action_out,
                              double* best_return_out, int32_t* best_index_out, int32_t* best_length_out, double* return_out,
                              double* ess_out, void* stream);

/* emei_rollout_policy / emei_rollout_policy_noisy / emei_evaluate_policies for a network with TWO ReLU hidden layers — the shape of
 * the actors the reference's zoo trains (stable-baselines3 MlpPolicy: 256-256 ReLU, SAC with a mean head, a log-std head and a tanh
 * squash; TD3, DDPG and most PPO actors likewise).  struct emei_policy is unchanged; the deep network has a struct and two entry
 * points of its own.  The six weight arrays are DEVICE pointers, read during the launch and not retained; they must not overlap any
 * output of the call.
 *
 * Semantics (normative).  emei_rollout_policy_deep is emei_rollout_policy (noise NULL) or emei_rollout_policy_noisy (noise given),
 * emei_evaluate_policies_deep is emei_evaluate_policies, clause for clause — Observe, Step, Start, scoring, the outputs, the state the
 * handle is left in — except for the network of clause 2 ("Policy").  All sums run in ascending index order, in float64 (a product of
 * two float32 values is exact in float64, so fused and unfused multiply-add give the same bits):
 *        for j ascending, z = (double)b1[j]; for k ascending, z = z + (double)w1[j,k] * (double)x[k]; h1_j = (float)z;
 *                    h1_j = h1_j > 0.f ? h1_j : 0.f (NaN gives 0).
 *        for i ascending, z = (double)b2[i]; for j ascending, z = z + (double)w2[i,j] * (double)h1_j; h2_i = (float)z;
 *                    h2_i = h2_i > 0.f ? h2_i : 0.f (NaN gives 0).
 *        y_q = (double)b3[q]; for i ascending, y_q = y_q + (double)w3[q,i] * (double)h2_i.
 *      What follows y_q is emei_rollout_policy's and emei_rollout_policy_noisy's text with h2 in the place of h: the CLIP, TANH and
 *      threshold output clauses and their NaN handling; the noise term y_q = y_q + (double)s_q * (double)z_q, added last; the
 *      EMEI_POLICY_NOISE_GAUSS_HEAD head ws [n_out, hidden2], l_q = (double)bs[q] + the ascending sum of (double)ws[q,i] * (double)h2_i;
 *      epsilon-greedy; the noise words W[m] of (seed + t, g).  As there, TANH and GAUSS_HEAD are not pinned bit for bit.
 *      emei_evaluate_policies_deep: `stacked` names P = n_policies networks laid end to end — w1 [P, hidden1, obs_dim], b1 [P, hidden1],
 *      w2 [P, hidden2, hidden1], b2 [P, hidden2], w3 [P, n_out, hidden2], b3 [P, n_out] — hidden1, hidden2 and out_mode shared.
 * Consequences.  Those of the one-layer calls: replay through emei_rollout (bit for bit in every mode) and through
 * emei_evaluate_sequences; chunking, (a + b, seed) = (a, seed) then (b, seed + a); sharding, results depend on the global env index
 * only; the calls neither allocate nor synchronise (capturable).  A deep network whose first layer is (e_k, -e_k) rows with zero
 * biases and whose second layer is (w1[i,k], -w1[i,k]) computes the one-layer network's sums with zero terms between them: the same
 * bits (finite weights and observations).
 * Kernels: pend_policy_rollout_deep_kernel / body_policy_rollout_deep_kernel (one kernel per family, the noise a wave-uniform switch)
 * and pend_policy_eval_deep_kernel / body_policy_eval_deep_kernel, all launched as ONE-WAVE blocks: the wave keeps h1 in a tile of
 * dynamic LDS of 256 * ceil(hidden1 / 4) * 4 bytes (float32, lane-minor in groups of four units: 64 KiB at the cap) next to its
 * kernel's static LDS; wave w holds envs 64 w .. 64 w + 63 as in the one-layer calls, and a block of the population call serves one
 * policy (block b: policy b / nb, env wave b % nb, nb = ceil(n_envs / 64)).
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: the scalars (n_steps < 1; horizon < 1,
 * n_policies < 1, discount outside (0, 1]); NULL policy / stacked; struct_size wrong; hidden1, then hidden2, outside
 * [1, EMEI_POLICY_DEEP_MAX_HIDDEN]; unknown out_mode; reserved != 0; with a non-NULL noise, emei_rollout_policy_noisy's checks of it in
 * their order; a NULL handle; NULL w1, b1, w2, b2, w3 or b3, in this order; a wrong action_dtype, then unknown flags (the population
 * call: NULL return_out, then n_envs * n_policies > 2^31 - 1 or more than 2^31 - 1 blocks); a GAUSS mode on a discrete env or
 * EPS_GREEDY on a continuous one.  EMEI_ERR_STATE and EMEI_ERR_UNSUPPORTED where the one-layer calls give them. */
#define EMEI_POLICY_DEEP_MAX_HIDDEN 256
typedef struct emei_policy_deep {
    uint32_t struct_size;   /* = sizeof(emei_policy_deep) */
    int32_t hidden1;        /* width of the first hidden layer (ReLU), 1 .. EMEI_POLICY_DEEP_MAX_HIDDEN */
    int32_t hidden2;        /* width of the second hidden layer (ReLU), 1 .. EMEI_POLICY_DEEP_MAX_HIDDEN */
    int32_t out_mode;       /* enum emei_policy_out; ignored by the discrete envs */
    const float* w1;        /* [hidden1, obs_dim] row-major */
    const float* b1;        /* [hidden1] */
    const float* w2;        /* [hidden2, hidden1] */
    const float* b2;        /* [hidden2] */
    const float* w3;        /* [n_out, hidden2];  n_out = act_dim, or 1 for the discrete envs */
    const float* b3;        /* [n_out] */
    int64_t reserved;       /* must be 0 */
} emei_policy_deep;
EMEI_API int emei_rollout_policy_deep(emei_env* h, int32_t n_steps, const emei_policy_deep* policy, const emei_policy_noise* noise,
                                      void* actions_out, int action_dtype, float* obs_out, float* reward_out, uint8_t* done_out,
                                      uint32_t flags, void* stream);
EMEI_API int emei_evaluate_policies_deep(emei_env* h, int32_t horizon, int32_t n_policies, const emei_policy_deep* stacked,
                                         double discount, const double* start_state, double* return_out, int32_t* length_out,
                                         float* final_obs_out, void* stream);

/* emei_plan_policy for a network with TWO ReLU hidden layers, with an optional TERMINAL VALUE: the whole planner of MBOP, LOOP, POLO
 * and TD-MPC — n_candidates closed-loop rollouts of a trained 256-256 actor per env under exploration noise, each scored on the true
 * dynamics for `horizon` steps plus a learned value of the observation it ends in, then the best or the return-weighted first
 * action.  `policy` and `noise` are emei_rollout_policy_deep's structs, `value` is a second struct emei_policy_deep or NULL; all with
 * DEVICE pointers, read during the launches and not retained; they must not overlap any output or the workspace.
 *
 * Semantics (normative).  emei_plan_policy's text clause for clause — 1. Start and observe, 3. Step and score, 4. Select, 5. Weights,
 * the outputs, the consequences — with two changes:
 *   2. Policy.  The network is emei_rollout_policy_deep's: h1, h2 and y_q with float64 ascending sums, h1 and h2 rounded to float32
 *      before the ReLU, NaN gives 0; what follows y_q is its noise clause — the term (double)s_q * (double)z_q added last, the
 *      EMEI_POLICY_NOISE_GAUSS_HEAD head ws [n_out, hidden2] on h2, epsilon-greedy on the discrete envs — and its output clauses.
 *      Step t of candidate k draws from the word stream of emei_plan_policy,
 *          W[m] = philox4x32_10(key = seed + t (mod 2^64), counter = (g lo, g hi, k, m >> 2)).v[m & 3].
 *      Candidate 0 takes NO noise, selected after the draw: a y_q of -0.0 keeps its sign, a non-finite std does not reach it, and on a
 *      discrete env it never explores.
 *   3b. Terminal value, with `value` non-NULL.  `value` names a network of emei_rollout_policy_deep's arithmetic with n_out = 1 —
 *      w1 [hidden1, obs_dim], b1 [hidden1], w2 [hidden2, hidden1], b2 [hidden2], w3 [1, hidden2], b3 [1] — whose widths are its own
 *      (each in [1, EMEI_POLICY_DEEP_MAX_HIDDEN]); its out_mode is ignored.  A candidate that set no terminal bit in any of its
 *      `horizon` steps gets one more term,
 *          ret = ret + g_H * (double)v,
 *      where g_H is the running product discount^t after `horizon` multiplications (the float64 variable clause 3 carries) and
 *      v = (float)y_0 of the value network on x_H, the float32 observation row that step horizon - 1 emits.  There is no output
 *      clause: a NaN y_0 stays NaN, the return becomes NaN and the planner's order puts it last.  The product is rounded to float64
 *      and then added (no fused multiply-add).  A candidate that terminated gets nothing, at whichever step, the last one included.
 *      L(i, k) is unchanged by the value.  return_out, (k*, r*), the weights, the mean and the ESS all use the bootstrapped returns.
 *      `value` NULL: no bootstrap, and every consequence of emei_plan_policy holds with the deep network — candidate 0 equals
 *      emei_evaluate_policies_deep with n_policies = 1; the returns equal emei_evaluate_sequences on the actions of the per-step loop.
 * A one-layer struct emei_policy is served exactly through the embedding emei_rollout_policy_deep documents (first layer (e_k, -e_k)
 * rows with zero biases, second layer (w1[i,k], -w1[i,k])).
 * Kernels: pend_policy_plan_deep_kernel / body_policy_plan_deep_kernel — the loop of the family's one-layer plan kernel, one lane per
 * candidate j = i * n_candidates + k, launched as ONE-WAVE blocks whose dynamic LDS is the wave's h1 tile, sized by the wider first
 * layer of `policy` and `value` (64 KiB at the cap); the value is evaluated in the same tile after the loop, skipped by a wave all of
 * whose candidates terminated — then plan_policy_finish_kernel, unchanged.  EMEI_POLICY_OUT_TANH and EMEI_POLICY_NOISE_GAUSS_HEAD are
 * not pinned bit for bit, as in the rollouts.
 * workspace: emei_plan_policy_workspace_bytes(n_envs, n_candidates) bytes, as emei_plan_policy's.
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: horizon < 1; n_candidates < 1; discount
 * outside (0, 1]; with a non-NULL mean_action_out or ess_out, temperature not finite or <= 0; NULL policy, then policy.struct_size,
 * policy.hidden1, then policy.hidden2, outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN], policy.out_mode, policy.reserved; NULL noise, then
 * emei_rollout_policy_noisy's noise checks in their order; with a non-NULL value, value.struct_size, value.hidden1, value.hidden2,
 * value.reserved; a NULL handle; NULL policy w1, b1, w2, b2, w3 or b3, in this order, then the value's likewise; n_envs * n_candidates
 * > 2^31 - 1; a wrong action_dtype; NULL workspace, then NULL best_action_out; a GAUSS mode on a discrete env or EPS_GREEDY on a
 * continuous one.  EMEI_ERR_STATE without a state and without start_state. */
EMEI_API int emei_plan_policy_deep(emei_env* h, int32_t horizon, int32_t n_candidates, const emei_policy_deep* policy,
                                   const emei_policy_noise* noise, const emei_policy_deep* value, double discount, double temperature,
                                   const double* start_state, void* workspace, void* best_action_out, int action_dtype,
                                   float* mean_action_out, double* best_return_out, int32_t* best_index_out, int32_t* best_length_out,
                                   double* return_out, double* ess_out, void* stream);

/* Policy-guided receding-horizon control, whole episodes in ONE launch (plus the small one that packs the done mask): what the loop
 * "emei_plan_policy with a fresh noise seed, best or weighted-mean first action, emei_step" does in three launches and a new noise
 * struct per control step — the controller of MBOP, LOOP and POLO run on the true dynamics.  The envs are emei_mpc_mppi's: the
 * 4-state family on its own kernels and the four InvertedDoublePendulum envs (any integrator, either precision, no observation
 * noise; obs_out is [n_steps, n_envs, 6]) on the body family.  Unlike emei_mpc_mppi there is no nominal to carry from one control
 * step to the next — the policy is the warm start — so there is no horizon cap.  `policy` and `noise` are emei_plan_policy's structs
 * (one-layer struct emei_policy only; all three noise modes, both output modes) with DEVICE pointers, read during the launch and not
 * retained; they must not overlap any output or the workspace.
 *
 * Semantics (normative).  For every env i, g = env_index_offset + i, and t = 0 .. n_steps - 1:
 *   1. Plan.  Exactly emei_plan_policy(h, horizon, n_candidates, policy, noise_t, discount, temperature, start_state = NULL, ...) for
 *      env i, where noise_t is `noise` with seed = noise.seed + t * seed_stride (mod 2^64): step h of candidate k draws from
 *          W[m] = philox4x32_10(key = noise.seed + t * seed_stride + h (mod 2^64), counter = (g lo, g hi, k, m >> 2)).v[m & 3].
 *      Candidate 0 takes NO noise.  The start is the env's current state, x_0 its float32 observation.  Scoring, the planner's order,
 *      the weight case analysis and the summation tree are emei_plan_policy's: lane l adds the candidates k = l, l + 64, .. in
 *      ascending order, then the butterfly d = 1 .. 32.
 *      plan_return_out[t, i] = r*, plan_index_out[t, i] = k* (int32), ess_out[t, i] as emei_plan_policy's ess_out; float64 / int32
 *      [n_steps, n_envs], each may be NULL.
 *   2. Act.  EMEI_MPC_POLICY_ACT_BEST: a_t is what best_action_out would hold, candidate k*'s action at step 0.
 *      EMEI_MPC_POLICY_ACT_MEAN: on the continuous envs a_t is the float32 mean_action_out value; on the discrete envs
 *      a_t = (mean >= 0.5f) ? 1 : 0.  actions_out[t, i(, :)] in action_dtype (U8 / I32 / I64 discrete, F32 continuous),
 *      [n_steps, n_envs(, act_dim)].  Required.  `temperature` is consulted and checked only with ACT_MEAN or a non-NULL ess_out.
 *   3. Step.  Clause 4 of emei_mpc_mppi: exactly emei_step(a_t, flags) for env i, with emei_rollout's arithmetic: the TimeLimit
 *      counter, the EMEI_DONE_* bits and EMEI_FLAG_AUTO_RESET with the handle's reset key and episode counter.  obs_out / reward_out /
 *      done_out at [t, i] as emei_rollout writes them; any of the three may be NULL.  After a reset the next plan observes the new
 *      episode's state.
 * After the call the handle is as after the equivalent loop: state, step and episode counters, the done mask emei_compact_done
 * reads.  Every output is bit-identical to that loop's.
 * Consequences.  Chunking: n_steps = a + b in one call equals a call with (a, noise.seed) followed by one with
 * (b, noise.seed + a * seed_stride).  Replay: actions_out fed to emei_rollout from the same start reproduces obs_out, reward_out and
 * done_out.  Sharding: results depend on g only, not on n_envs or the shard.  Stream: the call neither allocates nor synchronises
 * (capturable).  n_candidates = 1 is the deterministic policy: the actions of emei_rollout_policy.  Seed stride: any value is legal;
 * with seed_stride >= horizon the keys of consecutive control steps do not overlap (with seed_stride = 1 step h + 1 of control step t
 * and step h of control step t + 1 draw from the same key).
 * Work split: one wave per env, its candidates spread over the 64 lanes (pend_mpc_policy_kernel / body_mpc_policy_kernel); many
 * candidates with few envs favour emei_plan_policy's route, which spreads all candidates over the device.
 * workspace: emei_mpc_policy_workspace_bytes(n_envs, n_candidates) = 12 * n_envs * n_candidates bytes rounded up to a multiple of 8,
 * device memory, 8-byte aligned, contents irrelevant before and after: every candidate's float64 return [n_envs, n_candidates], then
 * its float32 action of step 0 (every env served has one action component).
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: n_steps < 1; horizon < 1; n_candidates < 1;
 * discount outside (0, 1]; unknown act_mode; with ACT_MEAN or a non-NULL ess_out, temperature not finite or <= 0;
 * emei_rollout_policy's struct checks up to and including policy.reserved; NULL noise, then emei_rollout_policy_noisy's noise checks
 * in their order; a NULL handle; NULL w2 or b2, hidden > 0 with NULL w1 or b1; n_envs * n_candidates > 2^31 - 1; a wrong
 * action_dtype; unknown flags; NULL workspace, then NULL actions_out; a GAUSS mode on a discrete env or EPS_GREEDY on a continuous
 * one.  EMEI_ERR_STATE without a state.  EMEI_ERR_UNSUPPORTED where emei_mpc_mppi gives it, with its messages: the other handles
 * that step on the body kernels (HalfCheetah, Hopper; InvertedPendulum with another integrator or observation noise), an
 * InvertedDoublePendulum handle with observation noise, a handle with observation peers set. */
enum emei_mpc_policy_act { EMEI_MPC_POLICY_ACT_BEST = 0, EMEI_MPC_POLICY_ACT_MEAN = 1 };
/* bytes of device scratch emei_mpc_policy needs for this shape; host only, no handle, no HIP call.
 * Negative (EMEI_ERR_INVALID) where emei_plan_mppi_workspace_bytes is. */
EMEI_API int64_t emei_mpc_policy_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_mpc_policy(emei_env* h, int32_t n_steps, int32_t horizon, int32_t n_candidates, const emei_policy* policy,
                             const emei_policy_noise* noise, uint64_t seed_stride, int32_t act_mode, double discount,
                             double temperature, void* workspace, void* actions_out, int action_dtype, float* obs_out,
                             float* reward_out, uint8_t* done_out, double* plan_return_out, int32_t* plan_index_out, double* ess_out,
                             uint32_t flags, void* stream);

/* A TERMINAL VALUE for the open-loop planners: emei_evaluate_sequences, emei_plan_shooting, emei_plan_mppi and emei_plan_cem with a
 * learned value of the observation the horizon ends in on top of every candidate's return — MPPI with a terminal cost, PETS /
 * PlaNet-style CEM with a critic, the planner of TD-MPC and POLO without an actor — at one network evaluation per candidate, not one
 * per step.  `value` is a struct emei_policy_deep with n_out = 1, as emei_plan_policy_deep's: w1 [hidden1, obs_dim], b1 [hidden1],
 * w2 [hidden2, hidden1], b2 [hidden2], w3 [1, hidden2], b3 [1]; the widths are its own, each in [1, EMEI_POLICY_DEEP_MAX_HIDDEN];
 * out_mode is ignored; its pointers are DEVICE pointers, read during the launch and not retained.  `value` is required here: without
 * one, call the plain entry point.
 *
 * Semantics (normative).  Each of the four calls is its plain counterpart clause for clause — the candidates (a pure function of
 * (seed, g, k)), the start-state rule, the per-step arithmetic, L(i, k), the untouched handle, "neither allocates nor synchronises"
 * — with one clause added:
 *   Terminal value.  A candidate that set no terminal bit in any of its `horizon` steps gets
 *       ret = ret + g_H * (double)v,
 *   where g_H is the float64 running product of the discount after `horizon` multiplications and v = (float)y_0 of the value network
 *   in emei_rollout_policy_deep's arithmetic (float64 ascending sums, h1 / h2 rounded to float32 before the ReLU, NaN gives 0),
 *   evaluated on x_H, the float32 observation row that step horizon - 1 emits — the row final_obs_out holds for that candidate.  The
 *   product is rounded to float64 and then added (no fused multiply-add).  There is no output clause: a NaN y_0 makes the return NaN,
 *   and the planner's order puts it last.  A candidate that terminated gets nothing, at whichever step, the last one included (its
 *   L equals horizon too: L does not tell the two apart).  L and final_obs_out are unchanged by the value.
 * Everything downstream uses the bootstrapped returns: return_out, the planner's order, (k*, r*) and the best_* outputs; the MPPI
 * weights, mean and ESS; the CEM elite set, moments and elite_return_out.  The candidates do not depend on the returns, so the second
 * launches are the plain calls' (plan_finish, plan_mppi_finish, plan_cem_finish redraw the same candidates).
 * Kernels: pend_plan_value_kernel / body_plan_value_kernel — the loop of pend_plan_kernel / body_plan_kernel, one lane per candidate
 * j = i * n_candidates + k, launched as ONE-WAVE blocks whose dynamic LDS is the wave's h1 tile (64 KiB at the cap); the value is
 * evaluated after the loop, skipped by a wave all of whose candidates terminated.  The handle is untouched, no kernel id.
 * workspace (the three planners): emei_plan_value_workspace_bytes(n_envs, n_candidates) bytes of device memory, 16-byte aligned,
 * contents irrelevant before and after; it equals emei_plan_cem_workspace_bytes (emei_plan_shooting_value keeps every return too)
 * and is negative where that is.  Host only, no handle, no HIP call.
 * EMEI_ERR_INVALID before any HIP call, each message naming the argument, in this order: the plain call's scalar checks in its order
 * (horizon, n_candidates[, n_elites before], discount[, temperature]); NULL value; value.struct_size, value.hidden1, value.hidden2,
 * value.reserved; a NULL handle; NULL value w1, b1, w2, b2, w3, b3, in this order; the plain call's remaining checks in its order.
 * EMEI_ERR_STATE where the plain call gives it. */
EMEI_API int64_t emei_plan_value_workspace_bytes(int64_t n_envs, int32_t n_candidates);
EMEI_API int emei_evaluate_sequences_value(emei_env* h, int32_t horizon, int32_t n_candidates, const void* actions, int action_dtype,
                                           double discount, const emei_policy_deep* value, const double* start_state,
                                           double* return_out, int32_t* length_out, float* final_obs_out, void* stream);
EMEI_API int emei_plan_shooting_value(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                      double sigma, double discount, const emei_policy_deep* value, const double* start_state,
                                      void* workspace, void* best_action_out, int action_dtype, void* best_sequence_out,
                                      double* best_return_out, int32_t* best_index_out, int32_t* best_length_out, void* stream);
EMEI_API int emei_plan_mppi_value(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal, double sigma,
                                  double discount, const emei_policy_deep* value, double temperature, const double* start_state,
                                  void* workspace, float* nominal_out, double* best_return_out, int32_t* best_index_out, double* ess_out,
                                  void* stream);
EMEI_API int emei_plan_cem_value(emei_env* h, int32_t horizon, int32_t n_candidates, int32_t n_elites, uint64_t seed, const float* nominal,
                                 double sigma, const float* sigma_map, double discount, const emei_policy_deep* value,
                                 const double* start_state, void* workspace, float* mean_out, float* std_out, double* best_return_out,
                                 int32_t* best_index_out, double* elite_return_out, void* stream);

/* Which kernel the LAST emei_step / emei_rollout of this handle launched (enum emei_kernel_id): a debug /
 * test getter, so that a parity test can assert that the path it checked is the path bench.py times. */
enum emei_kernel_id {
    EMEI_KERNEL_NONE = 0,
    EMEI_KERNEL_PEND_STAGED_FREQ1 = 1, /* pend_rollout_staged_kernel<Env, ActT, true>  (freq_rate == 1) */
    EMEI_KERNEL_PEND_STAGED = 2,       /* pend_rollout_staged_kernel<Env, ActT, false> */
    EMEI_KERNEL_PEND_GENERIC_FULL = 3, /* pend_rollout_kernel<Env, ActT, true>: ragged n, short T or unaligned buffers */
    EMEI_KERNEL_PEND_GENERIC = 4,      /* pend_rollout_kernel<Env, ActT, false>: some output pointer is NULL */
    EMEI_KERNEL_BODY = 5,              /* body_rollout_kernel<Body, false> (euler / semi-implicit euler) */
    EMEI_KERNEL_BODY_RK4 = 6,          /* body_rollout_kernel<Body, true> */
    EMEI_KERNEL_BODY_CHUNKED = 7,      /* body_rollout_kernel<Body, false> as (64 envs) x (chunk of steps) work items (rollout_chunk_steps) */
    EMEI_KERNEL_BODY_RK4_CHUNKED = 8,  /* body_rollout_kernel<Body, true> likewise */
    EMEI_KERNEL_PEND_STAGED_PEERS_FREQ1 = 9, /* pend_rollout_staged_peers_kernel<Env, ActT, true>: with the peer stores of emei_set_obs_peers */
    EMEI_KERNEL_PEND_STAGED_PEERS = 10,      /* pend_rollout_staged_peers_kernel<Env, ActT, false> */
    EMEI_KERNEL_PEND_MPC_MPPI = 11,          /* pend_mpc_mppi_kernel<Env>: emei_mpc_mppi (it steps the handle, so it reports here) */
    EMEI_KERNEL_PEND_MPC_CEM = 12,           /* pend_mpc_cem_kernel<Env>: emei_mpc_cem (likewise) */
    EMEI_KERNEL_BODY_MPC_MPPI = 13,          /* body_mpc_mppi_kernel<Body, RK4>: emei_mpc_mppi on an InvertedDoublePendulum handle */
    EMEI_KERNEL_BODY_MPC_CEM = 14,           /* body_mpc_cem_kernel<Body, RK4>: emei_mpc_cem on an InvertedDoublePendulum handle */
    EMEI_KERNEL_PEND_POLICY = 15,            /* pend_policy_rollout_kernel<Env>: emei_rollout_policy (it steps the handle, so it reports here) */
    EMEI_KERNEL_BODY_POLICY = 16,            /* body_policy_rollout_kernel<Body, false>: emei_rollout_policy on the body kernels */
    EMEI_KERNEL_BODY_POLICY_RK4 = 17,        /* body_policy_rollout_kernel<Body, true> */
    EMEI_KERNEL_PEND_POLICY_NOISY = 18,      /* pend_policy_rollout_noisy_kernel<Env>: emei_rollout_policy_noisy */
    EMEI_KERNEL_BODY_POLICY_NOISY = 19,      /* body_policy_rollout_noisy_kernel<Body, false> */
    EMEI_KERNEL_BODY_POLICY_NOISY_RK4 = 20,  /* body_policy_rollout_noisy_kernel<Body, true> */
    EMEI_KERNEL_PEND_POLICY_DEEP = 21,       /* pend_policy_rollout_deep_kernel<Env>: emei_rollout_policy_deep, with or without noise */
    EMEI_KERNEL_BODY_POLICY_DEEP = 22,       /* body_policy_rollout_deep_kernel<Body, false> */
    EMEI_KERNEL_BODY_POLICY_DEEP_RK4 = 23    /* body_policy_rollout_deep_kernel<Body, true> */
};
EMEI_API int emei_last_rollout_kernel(emei_env* h);
/* The ids of emei_mpc_policy's kernels, which emei_last_rollout_kernel reports as well (the call steps the handle).  An enum of their
 * own: enum emei_kernel_id is the closed list 0 .. 23 that the bindings of the earlier entry points mirror value for value, and it
 * stays that list; these continue its numbering. */
enum emei_kernel_id_mpc_policy {
    EMEI_KERNEL_PEND_MPC_POLICY = 24, /* pend_mpc_policy_kernel<Env>: emei_mpc_policy on the 4-state kernels */
    EMEI_KERNEL_BODY_MPC_POLICY = 25  /* body_mpc_policy_kernel<Body, RK4>: emei_mpc_policy on an InvertedDoublePendulum handle */
};

/* --- Multi-GPU observation return by PEER WRITES (one process per GPU; north_star: "shards env instances across up to 8 GPUs of one node
 * ... only for the batched observation return"; SURVEY §5: "hipIpc peer writes from the step kernel's epilogue").  The reference has no
 * counterpart (it is a single-process CPU library: zoo/util.py:54-73 steps one env); this replaces the RCCL all-gather that follows a
 * rollout launch: the rollout kernel itself stores every step's observation row into the gathered buffer of every rank, so the block is
 * neither re-read from HBM nor moved by a separate collective.
 *
 * emei_set_obs_peers: from now on emei_rollout (emei_step likewise: it is a rollout of one step, hence refused) ALSO stores the observation of step t, env i at
 *     ((float*)peer_obs[p])[((int64_t)t * row_envs + col_offset + i) * obs_dim + k],  k < obs_dim,  for every p < n_peers
 * i.e. each peer buffer is a gathered block [n_steps, row_envs, obs_dim] float32 and this handle's envs are its columns
 * [col_offset, col_offset + n_envs).  peer_obs[p] are device pointers valid on this handle's device: memory of this process, or of another
 * rank mapped with emei_peer_buffer_open (16-byte aligned; row_envs >= col_offset + n_envs; each holds max_steps rows: a rollout of
 * more steps is refused with EMEI_ERR_INVALID instead of writing past them).  n_peers = 0 switches it off; at most EMEI_MAX_OBS_PEERS (a rank's own gathered buffer counts as one).
 * Built for the staged kernel of the CartPole family (BASELINE configs[4]'s env; n_envs a multiple of 64, n_steps >= 16, 16-byte
 * aligned buffers): any other rollout with peers set FAILS with EMEI_ERR_UNSUPPORTED — nothing is skipped silently.
 * Ordering is the caller's: a peer may read a block once the writer's launch has completed (stream / event synchronisation on the
 * writer, then any host-side barrier between the ranks), and the writer may reuse a buffer once its readers are done. */
#define EMEI_MAX_OBS_PEERS 8
EMEI_API int emei_set_obs_peers(emei_env* h, int n_peers, void* const* peer_obs, int64_t row_envs, int64_t col_offset, int32_t max_steps);

/* Device memory another process of this node can map: hipMalloc + hipIpcGetMemHandle / hipIpcOpenMemHandle (the handle is 64 opaque
 * bytes to be carried to the other rank by whatever the host side has: torch.distributed.all_gather_object, MPI, a pipe).  `device` is
 * the HIP device ordinal of the CALLER (the creator allocates there; the opener maps the creator's memory into that device's address
 * space, peer access over xGMI).  A buffer is closed by every opener before its creator destroys it. */
typedef struct emei_ipc_handle { unsigned char bytes[64]; } emei_ipc_handle;
EMEI_API int emei_peer_buffer_create(int device, uint64_t bytes, void** dev_ptr_out, emei_ipc_handle* handle_out);
EMEI_API int emei_peer_buffer_open(int device, const emei_ipc_handle* handle, void** dev_ptr_out);
EMEI_API int emei_peer_buffer_close(int device, void* dev_ptr);
EMEI_API int emei_peer_buffer_destroy(int device, void* dev_ptr);

/* Sorted indices of the envs whose last step reported done (wavefront-ballot compaction of the done
 * masks the step kernels leave behind): idx_out [n_envs] int32 (first *count_out entries valid),
 * count_out [1] int32. */
EMEI_API int emei_compact_done(emei_env* h, int32_t* idx_out, int32_t* count_out, void* stream);

/* Per-env counters of the handle: steps since the last reset (TimeLimit) and the episode index (the
 * counter word of the device reset generator).  Either pointer may be NULL. */
EMEI_API int emei_get_counters(emei_env* h, int32_t* steps_out, uint32_t* episode_out, void* stream);

/* Initial observation the DEVICE reset gives env `env_index[k]` (local index in this handle) at the
 * start of episode `episode[k]`: what Env.reset() would return for that (env, episode) pair.  Used to
 * rebuild `observations` after an auto-reset when a rollout is turned into an offline dataset
 * (schema of zoo/util.py:16-30,62-67): obs_out [count, obs_dim] float32. */
EMEI_API int emei_episode_init_obs(emei_env* h, int64_t count, const int64_t* env_index, const uint32_t* episode,
                                   float* obs_out, void* stream);

/* -- stateless batched reward / terminal (model-based-RL callers) ---------------------------- */
/* EmeiEnv.get_batch_reward / get_batch_terminal (core.py:182-188; cartpole.py:124-129,145-151;
 * inverted_pendulum.py:73-183; half_cheetah.py:59-67): obs, pre_obs [n, obs_dim] float32,
 * action [n, act_dim] float32 (may be NULL where the env ignores it), out [n]. */
EMEI_API int emei_reward(int env_id, int64_t n, const float* obs, const float* pre_obs, const float* action,
                double real_time_scale, int32_t freq_rate, float* reward_out, void* stream);
EMEI_API int emei_terminal(int env_id, int64_t n, const float* obs, uint8_t* terminal_out, void* stream);

/* The same with constructor parameters (enum emei_env_param; mask 0 = the defaults above). */
EMEI_API int emei_reward_ex(int env_id, int64_t n, const float* obs, const float* pre_obs, const float* action,
                   double real_time_scale, int32_t freq_rate, uint32_t env_param_mask, const double* env_params,
                   float* reward_out, void* stream);
EMEI_API int emei_terminal_ex(int env_id, int64_t n, const float* obs, uint32_t env_param_mask, const double* env_params,
                     uint8_t* terminal_out, void* stream);

/* The same three functions on the dtype the CALLER holds (enum emei_io_dtype).  The reference evaluates
 * get_batch_reward / get_batch_terminal on float64 arrays (cartpole.py:124-129,145-151; inverted_pendulum.py:73-183;
 * half_cheetah.py:59-67; hopper.py:95-106): with EMEI_IO_F64 obs / pre_obs / action are float64 [n, dim] and are
 * NOT narrowed — thresholds (|x| < 5, x_l < x < x_r, z ranges) and the x-difference of the forward reward are evaluated
 * on the caller's float64 values; reward_out is float64 [n].  EMEI_IO_F32 is the float32 form above. */
enum emei_io_dtype { EMEI_IO_F32 = 0, EMEI_IO_F64 = 1 };
/* flags of emei_reward_io */
#define EMEI_REWARD_BATCH_CTRL_COST 1u /* HalfCheetahRunning / HopperRunning only: the control cost is np.sum(np.square(action)) over the
                                          WHOLE batch, as half_cheetah.py:61 executes for B > 1 (no axis argument); the
                                          default (0) sums per env = step() semantics */
EMEI_API int emei_reward_io(int env_id, int64_t n, int io_dtype, const void* obs, const void* pre_obs, const void* action,
                   double real_time_scale, int32_t freq_rate, uint32_t env_param_mask, const double* env_params,
                   uint32_t flags, void* reward_out, void* stream);
EMEI_API int emei_terminal_io(int env_id, int64_t n, int io_dtype, const void* obs, uint32_t env_param_mask,
                     const double* env_params, uint8_t* terminal_out, void* stream);

/* EmeiEnv.get_batch_next_obs (core.py:190-193; abstract in the reference, no env implements it):
 * one step from caller-supplied float32 observations without touching any handle state.
 * obs [n, obs_dim], action as in emei_step, next_obs_out [n, obs_dim]. */
EMEI_API int emei_next_obs(int env_id, int64_t n, const float* obs, const void* actions, int action_dtype,
                  double real_time_scale, int32_t freq_rate, int32_t precision, float* next_obs_out,
                  void* stream);

/* The same for every env whose observation determines its state (CartPole, InvertedPendulum, HalfCheetah,
 * Hopper; the InvertedDoublePendulum's observation "wrap", inverted_double_pendulum.py:59, is not
 * invertible -> EMEI_ERR_UNSUPPORTED), with the integrator of mujoco_env.py:70-79 (classic control
 * ignores it).  No observation noise is added. */
EMEI_API int emei_next_obs_ex(int env_id, int64_t n, const float* obs, const void* actions, int action_dtype,
                     double real_time_scale, int32_t freq_rate, int32_t precision, int32_t integrator,
                     float* next_obs_out, void* stream);

/* emei_next_obs_ex on the caller's dtype: obs and next_obs_out are [n, obs_dim] of io_dtype (float64 observations enter the
 * float64 state unrounded); actions as in emei_step.  `integrator` may carry EMEI_NEXT_OBS_ODE_RK4 for the classic-control
 * envs (enum emei_ode_method RK4: ODE_approximation(method="rk4"), base_control.py:165-170); ignored by the other envs. */
#define EMEI_NEXT_OBS_ODE_RK4 0x100
EMEI_API int emei_next_obs_io(int env_id, int64_t n, int io_dtype, const void* obs, const void* actions, int action_dtype,
                     double real_time_scale, int32_t freq_rate, int32_t precision, int32_t integrator,
                     void* next_obs_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMEI_HIP_H */
