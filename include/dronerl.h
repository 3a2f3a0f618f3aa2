/*
 * dronerl.h -- C ABI of libdronerl.so, the MI355X (gfx950) batched
 * quadrotor environment and PPO kernels.
 *
 * Boundary.  The reference's env boundary is the gym.Env pair
 *   DroneGymEnv.reset() -> obs(15,) f32               /root/reference/drone.py:270-271 (-> 48-75)
 *   DroneGymEnv.step(a(4,) f32) -> (obs, r, done, {})  /root/reference/drone.py:266-268 (-> 81-159)
 * consumed through SB3 DummyVecEnv + VecMonitor (train.py:33-35), and the
 * batched variant VectorizedDroneEnv.reset/step (vectorized_drone.py:38-57,
 * 135-216).  This library replaces that whole layer (L0 physics + L1 env API
 * + L2 vectorisation) with one GPU-resident batch of N envs.
 *
 * Conventions
 *  - Every data pointer passed to a compute entry point is DEVICE memory
 *    (e.g. a torch tensor's data_ptr on the handle's device) or, for the
 *    per-step I/O of dr_reset / dr_step / dr_step_monitored, pinned host
 *    memory (hipHostMalloc): the kernel then reads the actions from and
 *    writes its outputs to host memory over PCIe (zero-copy), so a
 *    host-buffer step is one launch and one stream sync.  The caller owns
 *    all I/O buffers; the library owns the persistent env state (SoA).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *    Compute entry points only enqueue work: they are asynchronous with
 *    respect to the host and safe to capture into a hipGraph.
 *  - Return value: DR_OK (0) or a negative DR_ERR_* code.  A message for the
 *    last error on a handle is available from dr_last_error(handle);
 *    dr_last_error(NULL) reports errors that happened without a handle
 *    (dr_create).  No C++ exception crosses this ABI.
 *  - A handle is not thread-safe; use one handle per host thread.
 *  - Layouts: actions (N,4) f32 row-major; obs (N,15) f32 row-major for the
 *    "gym" variant, (N,12) for "vectorized"; rewards (N,) f32; dones (N,) u8.
 */
#ifndef DRONERL_H_
#define DRONERL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_ABI_VERSION 16

enum dr_status {
    DR_OK = 0,
    DR_ERR_INVALID = -1,   /* bad argument / shape / null handle          */
    DR_ERR_HIP = -2,       /* a HIP runtime call or kernel launch failed  */
    DR_ERR_NOMEM = -3,     /* device allocation failed                    */
    DR_ERR_UNSUPPORTED = -4
};

enum dr_variant {
    DR_VARIANT_GYM = 0,        /* DroneGymEnv, drone.py:13-274             */
    DR_VARIANT_VECTORIZED = 1, /* VectorizedDroneEnv, vectorized_drone.py  */
    /* Moving-target trajectory tracking (BASELINE.json configs[4]; an
       extension with no reference oracle, spec in DESIGN.md section 11):
       gym physics, reset and curriculum; the target moves per axis k as
       c_k + a_k sin(w_k t + ph_k) with per-episode (a, w, ph), a = eps * U,
       so eps = 0 reproduces DR_VARIANT_GYM exactly; obs (N,18) = gym obs +
       target velocity; reward = the gym reward against the moving target. */
    DR_VARIANT_MOVING = 2,
    /* Smooth control (an extension with no reference oracle, spec in
       DESIGN.md section 14): the gym env with a first-order motor lag and an
       action-rate penalty.  Per env the force f each motor applies is state
       (DR_FIELD_MOTOR, HOVER = f32(9.81 / 4) after every reset); a step with
       command a forms, in f32, s = |a - f|^2, f' = (1 - alpha) f + alpha a,
       runs the gym step on f' and reports reward - rate_penalty * s;
       obs (N,19) = gym obs + f'.  alpha / rate_penalty: dr_set_smoothing;
       at their defaults (1, 0) the variant is DR_VARIANT_GYM bit for bit. */
    DR_VARIANT_SMOOTH = 3,
    /* Tag (an extension with no reference oracle, spec in DESIGN.md section
       15): envs 2j (pursuer, role +1) and 2j+1 (evader, role -1) of the
       global numbering form a pair; num_envs and env_id_offset must be even.
       Each drone flies the gym dynamics on its own action.  With d the
       distance between the partners' new positions, the pursuer's reward is
       g = 0.01 * (-d), plus 1 while d < tag_radius, the evader's is -g, and a
       drone that crashes pays crash_penalty on top.  A pair's episode ends
       for both when either crashes or reaches the step limit; both reset as
       the gym env does.  obs (N,19) = the gym's first 12, partner - own
       position, partner - own velocity, the role.  tag_radius /
       crash_penalty: dr_set_tag (defaults 0.25, 0). */
    DR_VARIANT_TAG = 4,
    /* Quaternion attitude, RK4 integration (the opt-in non-parity mode; an
       extension with no reference oracle, spec in DESIGN.md section 16): the
       gym env's task -- reset draws, curriculum, reward, crash rule, step
       limit, auto-reset, monitor -- on the state (p, v, unit quaternion q =
       (w, x, y, z) body -> world, body rates omega).  The action is held over
       the step; y = (p, v, q, omega) advances by one classic RK4 step of
       p' = v, v' = R(q) e3 T / m - g e3, q' = q (x) (0, omega) / 2 and the
       gym's angular dynamics, then q is normalised.  No trigonometric
       function, no gimbal-lock singularity.  A reset sets q = (1, 0, 0, 0).
       obs (N,16) = p, v, q, omega, target - p.  The attitude is
       DR_FIELD_QUAT; DR_FIELD_EULER is refused (DR_ERR_UNSUPPORTED). */
    DR_VARIANT_RK4 = 5
};

enum dr_state_dtype {
    DR_STATE_F64 = 0,  /* reference precision (numpy float64 state)       */
    DR_STATE_F32 = 1   /* fp32 state: half the state bytes, unit-floor parity */
};

enum dr_rng_mode {
    /* reset uniforms from counter-based Philox4x32-10 keyed by seed with
       counter (episode number, global env id, tag|block): two blocks give
       the five draws as 32-bit uniforms w * 2^-32.  Reproducible and
       independent of how many other envs reset, or in which order.      */
    DR_RNG_PHILOX = 0,
    /* reset uniforms read from a caller-provided device buffer (N,5) f64,
       row i = the 5 draws env i's next reset consumes, in the reference's
       draw order (pos x, pos y, target x, y, z; drone.py:57,73).  This is
       how parity runs replay numpy's MT19937 stream.                     */
    DR_RNG_HOST_UNIFORMS = 1
};

enum dr_field {   /* dr_get_state / dr_set_state, all device buffers      */
    DR_FIELD_POS = 0,       /* (N,3) f64                                     */
    DR_FIELD_VEL = 1,       /* (N,3) f64                                     */
    DR_FIELD_EULER = 2,     /* (N,3) f64  roll, pitch, yaw (never wrapped)   */
    DR_FIELD_OMEGA = 3,     /* (N,3) f64                                     */
    DR_FIELD_TARGET = 4,    /* (N,3) f64                                     */
    DR_FIELD_STEP = 5,      /* (N,)  i32  current_step (drone.py:28,155)     */
    DR_FIELD_EP_NUM = 6,    /* (N,)  i32  ep_num (drone.py:18,61)            */
    DR_FIELD_EPS = 7,       /* (N,)  f64  curriculum eps (drone.py:33,70)    */
    DR_FIELD_EP_RETURN = 8, /* (N,)  f32  running episode return (monitor)   */
    DR_FIELD_EP_LENGTH = 9, /* (N,)  i32  running episode length (monitor)   */
    DR_FIELD_MOTION = 10,   /* (N,9) f32  moving variant: a xyz, w xyz, ph xyz
                               (DR_FIELD_TARGET is then the motion centre)  */
    DR_FIELD_MOTOR = 11,    /* (N,4) f32  smooth variant: the force each motor
                               applies (the lag filter's state)             */
    DR_FIELD_QUAT = 12,     /* (N,4) in the handle's state dtype (f64 or f32),
                               rk4 variant: the attitude (w, x, y, z); a zero
                               quaternion written here is the caller's error */
    DR_FIELD_WIND = 13,     /* (N,6) f32  gym variant after a non-neutral
                               dr_set_wind: the episode's mean wind xyz, the
                               gust xyz (m/s); DR_ERR_UNSUPPORTED before      */
    DR_FIELD_WAYPOINT = 14, /* (N,2) i32  gym variant after dr_set_waypoints:
                               j, the current waypoint's index within the
                               episode, and q, the reaches since enabling;
                               DR_ERR_UNSUPPORTED before                      */
    DR_FIELD_AIRFRAME = 15  /* (N,6) f32  gym variant after a non-neutral
                               dr_set_airframe: the episode's mass scale m,
                               inertia scale s, motor gains g0..g3; a written
                               m or s that is not positive and finite is the
                               caller's error; DR_ERR_UNSUPPORTED before      */
};

typedef struct dr_config {
    int64_t num_envs;       /* N >= 1                                        */
    int32_t variant;        /* enum dr_variant                               */
    int32_t state_dtype;    /* enum dr_state_dtype                           */
    int32_t rng_mode;       /* enum dr_rng_mode                              */
    int32_t auto_reset;     /* 1: DummyVecEnv semantics (reset a done env in
                               the same step, obs_out = reset obs); 0: raw
                               env semantics (caller resets).  Ignored (0)
                               for the vectorized variant, which never
                               auto-resets (vectorized_drone.py:211-213).    */
    int32_t device;         /* HIP device ordinal                            */
    int32_t max_steps;      /* 0 = variant default (200 gym, 1000 vectorized) */
    uint64_t seed;          /* Philox key                                    */
    int64_t env_id_offset;  /* global id of env 0 (rank * N for DP shards)   */
    double dt;              /* 0 = reference default 0.02 (drone.py:14)      */
} dr_config;

typedef struct dr_handle dr_handle;

/* Library ABI version (DR_ABI_VERSION of the build). */
int dr_abi_version(void);

/* Create N envs on cfg->device.  Mirrors the reference constructor: every
   env performs one reset (drone.py:46), so ep_num starts at 1.  In
   DR_RNG_HOST_UNIFORMS mode no uniform buffer exists yet, so that first
   reset uses u = 0.5 for all five draws (pos (0,0,1); the target is
   (0,0,1) anyway while eps = 0).  Replaces DroneGymEnv.__init__
   (drone.py:255-264) and VectorizedDroneEnv.__init__ (vectorized_drone.py:13-36).
   Synchronous: returns after the state is initialised. */
int dr_create(const dr_config *cfg, dr_handle **out);
int dr_destroy(dr_handle *h);

int64_t dr_num_envs(const dr_handle *h);
int dr_obs_dim(const dr_handle *h);   /* 15 gym, 12 vectorized, 18 moving, 19 smooth / tag, 16 rk4 */

/* Reset every env and write (N,obs_dim) obs.  Replaces DroneEnv.reset
   (drone.py:48-75) called on each env by VecEnv.reset, and
   VectorizedDroneEnv.reset (vectorized_drone.py:38-57). */
int dr_reset(dr_handle *h, float *obs_out, void *stream);

/* Reset only envs with mask[i] != 0 ((N,) u8); obs_out rows of other envs are
   rewritten with their current obs.  (DummyVecEnv-free callers, test
   harnesses.)  Not available for the vectorized variant.  DR_VARIANT_TAG
   resets a pair (envs 2j, 2j+1) if either member's byte is set. */
int dr_reset_masked(dr_handle *h, const uint8_t *mask, float *obs_out,
                    void *stream);

/* One env step for all N envs.  Replaces DroneEnv.step (drone.py:81-159)
   looped by DummyVecEnv.step_wait, and VectorizedDroneEnv.step
   (vectorized_drone.py:135-216).
     actions        (N,4) f32, NOT clipped (the reference env does not clip)
     obs_out        (N,obs_dim) f32; with auto_reset, rows of done envs hold
                    the reset observation (DummyVecEnv semantics)
     rew_out        (N,) f32 (SB3 buffers rewards as f32)
     done_out       (N,) u8
     terminal_obs_out  nullable (N,obs_dim) f32: for done envs the obs
                    BEFORE the auto-reset ("terminal_observation"); rows of
                    envs that are not done are left untouched.            */
int dr_step(dr_handle *h, const float *actions, float *obs_out,
            float *rew_out, uint8_t *done_out, float *terminal_obs_out,
            void *stream);

/* dr_step plus VecMonitor bookkeeping (running f32 return, i32 length per
   env): for done envs the finished episode's return/length are written to
   ep_return_out / ep_length_out ((N,) each; other rows untouched) and the
   running counters restart.  SB3 VecMonitor.step_wait equivalent. */
int dr_step_monitored(dr_handle *h, const float *actions, float *obs_out,
                      float *rew_out, uint8_t *done_out,
                      float *terminal_obs_out, float *ep_return_out,
                      int32_t *ep_length_out, void *stream);

/* dr_step_monitored plus the gymnasium TimeLimit split: truncated_out (N) u8
   (non-null) gets 1 where the episode ended at the step limit without a
   crash (drone.py:155-157 vs 154), 0 elsewhere.  The reference's env reports
   both as terminated (SB3 sees it through shimmy's GymV21 compatibility), so
   only PPOConfig.bootstrap_timeouts uses it: SB3's rewards[i] += gamma *
   V(terminal_obs[i]) for truncated envs.  (ABI v12.) */
int dr_step_monitored_trunc(dr_handle *h, const float *actions, float *obs_out,
                            float *rew_out, uint8_t *done_out, float *terminal_obs_out,
                            float *ep_return_out, int32_t *ep_length_out,
                            uint8_t *truncated_out, void *stream);

/* Device-side state access (parity injection, checkpointing, get_attr). */
int dr_get_state(dr_handle *h, int field, void *out, void *stream);
/* dr_get_state for k selected envs: out row j = field of env env_ids[j]
   ((k,3) f64 for vector fields, (k,) for scalars, (k,9) f32 for MOTION, (k,4) f32 for MOTOR).
   The per-step `get_attr('pos')` of TrajectoryTensorboardCallback
   (traj_tb.py:34) without copying the whole batch. */
int dr_gather_state(dr_handle *h, int field, const int32_t *env_ids, int64_t k,
                    void *out, void *stream);
int dr_set_state(dr_handle *h, int field, const void *in, void *stream);

/* DR_RNG_HOST_UNIFORMS: device pointer to (N,5) f64 ((N,14) for the moving
   variant: the 5 gym draws, then a xyz, w xyz, ph xyz) read by every later
   reset until replaced.  The buffer must stay alive while work using it is
   in flight. */
int dr_set_reset_uniforms(dr_handle *h, const double *u_dev);

/* Replace the Philox key used by later resets (VecEnv.seed).  Takes effect
   for work enqueued after the call. */
int dr_set_seed(dr_handle *h, uint64_t seed);

/* DR_VARIANT_SMOOTH: the lag blend alpha = dt / (tau + dt) in (0, 1] and the
   action-rate penalty rate_penalty >= 0 (defaults 1 and 0: the gym env).
   DR_ERR_INVALID for a null handle, values out of range or non-finite;
   DR_ERR_UNSUPPORTED on the other variants.  Takes effect for work enqueued
   after the call (the two values are launch arguments, not device state).
   dr_get_smoothing reads them back (either pointer may be NULL). */
int dr_set_smoothing(dr_handle *h, float alpha, float rate_penalty);
int dr_get_smoothing(const dr_handle *h, float *alpha, float *rate_penalty);

/* DR_VARIANT_TAG: the tag radius (> 0, default 0.25) and the crash penalty
   (>= 0, default 0).  DR_ERR_INVALID for a null handle, values out of range or
   non-finite; DR_ERR_UNSUPPORTED on the other variants.  Takes effect for work
   enqueued after the call (launch arguments, not device state).  dr_get_tag
   reads them back (either pointer may be NULL). */
int dr_set_tag(dr_handle *h, float tag_radius, float crash_penalty);
int dr_get_tag(const dr_handle *h, float *tag_radius, float *crash_penalty);

/* DR_VARIANT_GYM: wind, gusts and linear drag, an
   option of the gym env, all four neutral at 0:
     drag        k >= 0, linear drag per unit mass (1/s), k * dt <= 1
     wind_speed  W >= 0, bound of each axis of the per-episode mean wind (m/s)
     gust_sigma  s >= 0, stationary standard deviation of each gust axis (m/s)
     gust_rate   beta in [0, 1], the gust's per-step mean reversion
   Per env six f32 words are state (DR_FIELD_WIND): the mean wind m and the
   gust g.  With (key, counter) -> Philox4x32-10 block, gid the global env id
   and words -> uniforms u = w * 2^-32 as for the reset draws:
     reset into episode ep:  m_k = W * f32(2 u_k - 1) from the block of counter
       (ep, gid_lo, gid_hi, TAG_RESET | 2) (f32 product), g = 0; in
       DR_RNG_HOST_UNIFORMS mode too (the host buffer keeps its (N,5) meaning)
     step from step counter s of episode ep, ahead of the gym step:
       xi_k = f32(2 u_k - 1) from the first three words of the block of counter
       (ep, gid_lo, gid_hi, 0x47000000 | s);
       g_k <- b * g_k + c * xi_k in f32, one rounding per operation, with
       b = 1.0f - beta and c = (float)((double)s * sqrt(3 (1 - (double)b^2)))
       formed here once per call (xi has variance 1/3: the stationary std of g
       is s);
       w_k = (S)(m_k + g_k) (f32 add, then the cast to the state scalar S);
       v_k <- v_k + ((S)k * (w_k - v_k)) * dt;
       then the gym step, unchanged, on the updated velocity.
   The observation stays the gym's 15 floats: the wind is not observed.
   The first non-neutral call allocates the six arrays and fills m for every
   env's CURRENT episode (so m is a function of key, env and episode whenever
   wind was switched on): that call is synchronous (it waits for the device)
   and must not be made during graph capture.  Until then the handle allocates
   nothing more and launches exactly the gym's kernels; afterwards it launches
   the wind kernels, also at all-zero parameters (where every result equals
   the gym's).  A later change of W applies from each env's next reset; k, s,
   beta apply to work enqueued after the call.  dr_rollout* on such a handle
   runs the one-role kernel at every size and is bitwise k dr_step calls.
   DR_ERR_INVALID for a null handle, a negative or non-finite value, beta > 1
   or k * dt > 1; DR_ERR_UNSUPPORTED on the other variants and on handles
   with max_steps >= 2^24 (the gust counter holds s in 24 bits).  dr_get_wind
   reads the four values back (any pointer may be NULL). */
int dr_set_wind(dr_handle *h, float drag, float wind_speed, float gust_sigma,
                float gust_rate);
int dr_get_wind(const dr_handle *h, float *drag, float *wind_speed, float *gust_sigma,
                float *gust_rate);

/* DR_VARIANT_GYM: waypoint courses, an option of the
   gym env: the target moves on when the drone reaches it.
     reach_radius  R > 0, finite: the distance below which a waypoint counts
     reach_bonus   B >= 0, finite: the reward added in the step of a reach
   Per env two i32 words are state (DR_FIELD_WAYPOINT): j, the index of the
   current waypoint within the episode (= the reaches this episode; every reset
   sets it to 0), and q, the reaches since enabling (resets never touch it).
   The current waypoint is DR_FIELD_TARGET.  One step of an env with global id
   gid in episode ep (ep_num), curriculum eps and target c, S the state scalar:
     1. the gym physics, unchanged; d = sqrt((dx dx + dy dy) + dz dz) of the
        new position minus c, in S, the gym's expression;
     2. r = (S)0.01 * (-d); reached = d < (S)R (false for NaN); where reached,
        r += (S)B;
     3. crash, the step counter and done are the gym's;
     4. where reached: j <- j + 1, q <- q + 1, and with u_k = w_k * 2^-32 of the
        first three words of the Philox4x32-10 block of counter
        (ep, gid_lo, gid_hi, 0x57000000 | j) under the handle's seed,
        c <- ((S)(eps u_0), (S)(eps u_1), (S)(eps u_2 + 1.0 + 0.0)), f64
        operations and a cast, the expressions of the reset's target draw
        (while eps == 0, c = (0, 0, 1) and no block is drawn); at most one
        advance per step;
     5. the obs, and the terminal obs, are the gym's 15 floats of the state
        AFTER the advance: the next waypoint is observed only once it is current;
     6. done with auto-reset: the gym reset, and j <- 0; q keeps its value, a
        reach in the terminal step included.  Without auto-reset the advanced
        state stays.
   At eps = 0 with (R, B) = (0.05, 1) every output equals the gym's; at any
   values obs[:, :12], done, ep_num and the resets do (the physics never reads
   the target).  In DR_RNG_HOST_UNIFORMS mode waypoints come from Philox too
   (the host buffer keeps its (N,5) meaning).
   The first call allocates the two arrays, zeroed: that call is synchronous
   (it waits for the device) and must not be made during graph capture.  Until
   then the handle allocates nothing more and launches exactly the gym's
   kernels; afterwards it launches the waypoint kernels, and there is no way
   back.  Later calls change R and B only, for work enqueued after the call
   (launch arguments).  dr_rollout* on such a handle runs the one-role kernel
   at every size and is bitwise k dr_step calls.
   DR_ERR_INVALID for a null handle, R <= 0, B < 0 or a non-finite value;
   DR_ERR_UNSUPPORTED on the other variants, on a handle whose wind is enabled
   and on handles with max_steps >= 2^24 (the counter holds j in 24 bits).  On
   a waypoint handle a non-neutral dr_set_wind is DR_ERR_UNSUPPORTED.
   dr_get_waypoints reads the two values back, (0, 0) before enabling (either
   pointer may be NULL). */
int dr_set_waypoints(dr_handle *h, float reach_radius, float reach_bonus);
int dr_get_waypoints(const dr_handle *h, float *reach_radius, float *reach_bonus);

/* DR_VARIANT_GYM: per-episode airframe randomisation,
   an option of the gym env.  Each spread is finite and in [0, 0.9]; all three
   are neutral at 0:
     mass_spread     sigma_m, half-width of the mass scale m around 1
     inertia_spread  sigma_I, half-width of the inertia scale s around 1
     motor_spread    sigma_g, half-width of each motor gain g_j around 1
   The vehicle of an episode has mass m * 1 kg, inertia s * (0.005, 0.005,
   0.01) and motors that deliver g_j times their command.  Per env six f32
   words are state (DR_FIELD_AIRFRAME): m, s, g0..g3.  With (key, counter) ->
   Philox4x32-10 block under the handle's seed, gid the global env id and
   xi = f32(2 u - 1) of a word's uniform u = w * 2^-32 (exact in f64, one
   rounding):
     reset into episode ep:  m = 1.0f + sigma_m * xi of word 0 and
       s = 1.0f + sigma_I * xi of word 1 of the block of counter
       (ep, gid_lo, gid_hi, 0x46000000 | 0); g_j = 1.0f + sigma_g * xi_j of the
       four words of block 0x46000000 | 1; every operation one f32 rounding; in
       DR_RNG_HOST_UNIFORMS mode too (the host buffer keeps its (N,5) meaning)
     step, S the state scalar, everything not named here the gym's:
       a'_j = g_j * a_j (f32), and the gym's motor mixes are taken on a';
       im = 1.0f / m, is = 1.0f / s (IEEE f32 divides);
       the three accelerations use (r_k2 * T) * (S)im where the gym has
       (r_k2 * T) / (S)mass;
       tau_phi = ((S)factor * (S)mix_phi) * (S)is, likewise theta, and the yaw
       torque is (S)(k_yaw * mix_psi) * (S)is.  One common inertia scale leaves
       the gyroscopic terms unchanged, so only the torques scale.
   At m = s = g = 1 every inserted product is by exactly 1 and the step is the
   gym's bit for bit.  The observation stays the gym's 15 floats: the airframe
   is not observed.
   The first non-neutral call allocates the six arrays and fills them for
   every env's CURRENT episode (so the field is a function of key, env and
   episode whenever the option was switched on): that call is synchronous (it
   waits for the device) and must not be made during graph capture.  Until
   then the handle allocates nothing more and launches exactly the gym's
   kernels; afterwards it launches the airframe kernels, also at all-zero
   spreads.  Later calls change the spreads only, which apply from each env's
   next reset (resets are their only readers).  dr_reset and dr_reset_masked
   redraw the field of the rows they reset.  dr_rollout* on such a handle runs
   the one-role kernel at every size and is bitwise k dr_step calls.
   DR_ERR_INVALID for a null handle or a value that is not in [0, 0.9] (NaN
   included); DR_ERR_UNSUPPORTED on the other variants and on a handle with
   wind or waypoints enabled; on an airframe handle a non-neutral dr_set_wind
   and any dr_set_waypoints are DR_ERR_UNSUPPORTED.  A refused call changes
   nothing.  dr_get_airframe reads the three values back (any pointer may be
   NULL).  These additions break no caller: DR_ABI_VERSION stays 16. */
int dr_set_airframe(dr_handle *h, float mass_spread, float inertia_spread, float motor_spread);
int dr_get_airframe(const dr_handle *h, float *mass_spread, float *inertia_spread,
                    float *motor_spread);

/* Synthetic random policy: out (n,4) f32 i.i.d. U[lo,hi) from Philox keyed
   by seed with counter (env_id_offset + i, step).  Not part of the
   reference; it generates the benchmark's action stream. */
int dr_random_actions(int64_t n, uint64_t seed, int64_t env_id_offset,
                      int64_t step, float lo, float hi, float *out,
                      void *stream);

/* K successive steps in ONE launch, the state held in registers between
   steps: outputs identical, bit for bit, to k calls of
   dr_step(h, actions + t*N*4, obs_out + t*N*obs_dim, rew_out + t*N,
   done_out + t*N, NULL) for t = 0..k-1 (auto-reset per the handle; no
   terminal obs, no VecMonitor counters).  The random-policy rollout loop
   `a = action_space.sample(); env.step(a)` over DroneEnv.step
   (drone.py:81-159) k times, without the per-step state round trip
   through HBM or the per-launch gap.
     actions   (k,N,4) f32, 16-byte aligned
     obs_out   (k,N,obs_dim) f32; rew_out (k,N) f32; done_out (k,N) u8
   k * N <= 2^31.  DR_RNG_HOST_UNIFORMS handles with auto-reset are
   DR_ERR_UNSUPPORTED (their reset draws are supplied per step).  (ABI v11.) */
int dr_rollout(dr_handle *h, int32_t k, const float *actions, float *obs_out,
               float *rew_out, uint8_t *done_out, void *stream);

/* dr_rollout with its kernel's start / end recorded into two hipEvent_t
   (either may be NULL) by hipExtLaunchKernel: the events take the dispatch
   packet's own timestamps, so timing a launch adds no packets to the
   stream (a benchmark's hipEventRecord pair costs several microseconds of
   host and queue time around a ~35 us launch).  Same outputs as
   dr_rollout.  (ABI v13.) */
int dr_rollout_timed(dr_handle *h, int32_t k, const float *actions, float *obs_out,
                     float *rew_out, uint8_t *done_out, void *stream,
                     void *start_event, void *stop_event);

/* dr_rollout on the synthetic random policy drawn in-kernel: step t's
   actions are exactly dr_random_actions(N, action_seed, env_id_offset of
   the handle, action_step0 + t, lo, hi).  actions_out nullable: (k,N,4) f32
   copy of the drawn actions.  (ABI v11.) */
int dr_rollout_random(dr_handle *h, int32_t k, uint64_t action_seed,
                      int64_t action_step0, float lo, float hi, float *actions_out,
                      float *obs_out, float *rew_out, uint8_t *done_out,
                      void *stream);

const char *dr_last_error(const dr_handle *h);

/* ---------------------------------------------------------------------------
 * PPO kernels (stable-baselines3 PPO arithmetic; the
 * reference calls it at train.py:36-43, 63-68).  All buffers are device
 * memory; layouts are time-major (T,N) so a fixed step is contiguous.
 * ------------------------------------------------------------------------- */

/* GAE reverse scan, RolloutBuffer.compute_returns_and_advantage:
   delta_t = r_t + g*V_{t+1}*(1-start_{t+1}) - V_t,
   A_t = delta_t + g*l*(1-start_{t+1})*A_{t+1}; the last step uses
   (1-last_dones) and last_values; R = A + V.  All arithmetic is f32 with
   numpy's NEP-50 rounding: gamma -> f32, gamma*lambda formed in f64 then
   rounded to f32 (SB3 multiplies two python floats first). */
int dr_gae(int64_t T, int64_t N, const float *rewards, const float *values,
           const uint8_t *episode_starts, const float *last_values,
           const uint8_t *last_dones, double gamma, double gae_lambda,
           float *advantages, float *returns, void *stream);

/* Diagonal-Gaussian action sampling for the rollout:
   a = mean + exp(log_std) * z, z ~ N(0,1) (Philox + Box-Muller keyed by
   (seed, counter, row)); logp = sum_j log N(a_j; mean_j, std_j);
   actions_clipped = clip(a, lo, hi) (what SB3 passes to env.step).
   actions_raw / logp / actions_clipped may each be NULL. */
int dr_policy_sample(int64_t n, const float *mean, const float *log_std,
                     uint64_t seed, uint64_t counter, float lo, float hi,
                     float *actions_raw, float *actions_clipped, float *logp,
                     void *stream);

/* dr_policy_sample with counter = *counter_base + counter_offset, the base
   read on the device (8-byte aligned u64): a rollout loop captured once
   into a hipGraph draws fresh noise on every replay when the caller
   advances the base between replays.  Bitwise dr_policy_sample for the same
   counter.  (ABI v8.) */
int dr_policy_sample_dev(int64_t n, const float *mean, const float *log_std,
                         uint64_t seed, const uint64_t *counter_base,
                         uint64_t counter_offset, float lo, float hi,
                         float *actions_raw, float *actions_clipped, float *logp,
                         void *stream);

/* Uniform random permutation of [0,n) (RolloutBuffer.get's
   np.random.permutation): the stable argsort of 64-bit Philox keys, by a
   bucket pass on the top key bits plus per-bucket bitonic sorts (no state
   kept across launches: graph-capturable).  dr_permutation_workspace_bytes
   gives the scratch size for n. */
size_t dr_permutation_workspace_bytes(int64_t n);
int dr_permutation(int64_t n, uint64_t seed, uint64_t counter, int32_t *out,
                   void *workspace, size_t workspace_bytes, void *stream);
/* dr_permutation with counter = *counter_base + counter_offset, the base a
   device u64 (8-byte aligned): graph-capturable epochs.  (ABI v9.) */
int dr_permutation_dev(int64_t n, uint64_t seed, const uint64_t *counter_base,
                       uint64_t counter_offset, int32_t *out, void *workspace,
                       size_t workspace_bytes, void *stream);

/* Gather a minibatch: dst[k,:] = src[idx[k],:] for row width `width`
   (floats), k < m.  Used to form minibatches from the flat rollout. */
int dr_gather_rows(int64_t m, int64_t width, const int32_t *idx,
                   const float *src, float *dst, void *stream);

/* A whole PPO.train minibatch in one launch (RolloutBuffer.get's
   `self.observations[batch_inds]` etc.): obs_out[r,:] = obs[idx[r],:]
   (obs_dim floats), actions_out[r,:] = actions[idx[r],:] (4 floats, rows
   16-byte aligned), aux_out[r,:] = aux[idx[r],:] (old_logp, advantage,
   return).  With adv_part non-null it also writes the per-256-row
   (count, mean, M2) partials of the gathered advantages that
   dr_ppo_head_loss_backward's normalisation consumes: pass the head's
   workspace and normalize_advantage = 2 there to skip its own pass. */
int dr_gather_minibatch(int64_t m, const int32_t *idx, int64_t obs_dim,
                        const float *obs, const float *actions,
                        const float *aux, float *obs_out, float *actions_out,
                        float *aux_out, float *adv_part, void *stream);

/* One-line rollout records (ABI v16, round 6): the PPO.train minibatch
   gather of RolloutBuffer.get (`self.observations[batch_inds]`,
   `self.actions[...]`, old log-probs / advantages / returns) reads one
   aligned 128-B line per row instead of three arrays' lines.
   dr_pack_rollout_records writes record r (DR_RECORD_FLOATS floats) from
   rollout row r once per iteration: floats 0 .. obs_dim-1 = obs[r,:], from
   a = 4 ceil(obs_dim / 4): a .. a+3 = actions[r,:], a+4 .. a+6 = (logp[r],
   adv[r], ret[r]), the rest 0 (obs_dim <= 24: 16 / 20 for the 15-d gym and
   18-d moving obs; actions and records 16-byte aligned; n rows).
   dr_gather_records then writes exactly dr_gather_minibatch's outputs
   (obs_out (m, obs_dim), actions_out (m, 4), aux_out (m, 3), the advantage
   partials when adv_part is non-null) from the records of rows idx[0..m). */
#define DR_RECORD_FLOATS 32
int dr_pack_rollout_records(int64_t n, int64_t obs_dim, const float *obs,
                            const float *actions, const float *logp, const float *adv,
                            const float *ret, float *records, void *stream);
int dr_gather_records(int64_t m, const int32_t *idx, int64_t obs_dim, const float *records,
                      float *obs_out, float *actions_out, float *aux_out, float *adv_part,
                      void *stream);

/* Tanh-layer backward fused with the bias gradient (the MLP backward of
   PPO.train): grad_z = grad_h * (1 - h^2) for an (m, n) activation h =
   tanh(z), and bias_grad[j] = sum_i grad_z[i, j].  n must be a multiple of
   4 and <= 1024.  `workspace` >= dr_tanh_backward_workspace_bytes(m, n). */
size_t dr_tanh_backward_workspace_bytes(int64_t m, int64_t n);
int dr_tanh_backward(int64_t m, int64_t n, const float *grad_h, const float *h,
                     float *grad_z, float *bias_grad, void *workspace,
                     size_t workspace_bytes, void *stream);

/* First MLP layer forward fused with its activation: h = tanh(x W^T + b)
   for x (m,k), W (n,k), b (n), h (m,n) (SB3 MlpExtractor's Linear + Tanh,
   the narrow-input layer).  k in {4,8,12,15,16,18,19,24,32}; n % 4 == 0,
   n <= 256; h 16-byte aligned.  Replaces an addmm plus a separate tanh pass
   over the (m,n) activation.  `rows` (nullable, m int32): input row r is
   x[rows[r]] -- a minibatch read in place from the rollout buffer through
   its permutation (RolloutBuffer.get without the gather copy). */
int dr_linear_tanh(int64_t m, int64_t k, int64_t n, const float *x,
                   const int32_t *rows, const float *w, const float *b, float *h,
                   void *stream);

/* dr_linear_tanh for both MLPs of the actor-critic (pi: w0/b0/h0, vf:
   w1/b1/h1) over the same input rows, in one launch. */
int dr_linear_tanh2(int64_t m, int64_t k, int64_t n, const float *x,
                    const int32_t *rows, const float *w0, const float *b0,
                    float *h0, const float *w1, const float *b1, float *h1,
                    void *stream);

/* Backward of the first layer h = tanh(x W^T + b), fused: for grad_h (m,n)
   = dLoss/dh, forms grad_z = grad_h * (1 - h^2) in registers (never stored)
   and writes grad_w (n,k) = grad_z^T x and grad_b (n) = sum_r grad_z
   (dr_tanh_backward + the weight-gradient GEMM in one pass; the input
   gradient of the first layer is not needed).  k as dr_linear_tanh; n % 4
   == 0, n <= 256; grad_h and h 16-byte aligned.  `rows` as dr_linear_tanh
   (x row r = x[rows[r]]).  Deterministic.
   `workspace` >= dr_first_layer_backward_workspace_bytes(m, k, n). */
size_t dr_first_layer_backward_workspace_bytes(int64_t m, int64_t k, int64_t n);
int dr_first_layer_backward(int64_t m, int64_t k, int64_t n, const float *grad_h,
                            const float *h, const float *x, const int32_t *rows,
                            float *grad_w, float *grad_b, void *workspace,
                            size_t workspace_bytes, void *stream);

/* dr_first_layer_backward for both MLPs (net 0: grad_h0/h0 -> grad_w0/
   grad_b0, net 1: grad_h1/h1 -> grad_w1/grad_b1) over the same input x in
   one launch (plus one column-sum and one finish launch for both).
   Bitwise the same results as two dr_first_layer_backward calls.  defer
   != 0 leaves the last reduction (and the grad_w / grad_b writes) to
   dr_grad_finish_clip_adam.
   `workspace` >= dr_first_layer_backward2_workspace_bytes(m, k, n). */
size_t dr_first_layer_backward2_workspace_bytes(int64_t m, int64_t k, int64_t n);
int dr_first_layer_backward2(int64_t m, int64_t k, int64_t n, const float *x,
                             const int32_t *rows, const float *grad_h0,
                             const float *h0, float *grad_w0, float *grad_b0,
                             const float *grad_h1, const float *h1,
                             float *grad_w1, float *grad_b1, int defer,
                             void *workspace, size_t workspace_bytes,
                             void *stream);

/* Policy heads for rollouts (ActorCriticPolicy.forward's action_net /
   value_net): mean (m,4) = h_pi W_act^T + b_act, value (m) = h_vf W_val^T +
   b_val, for the top hidden activations h_pi, h_vf (m,hd), hd % 4 == 0,
   hd <= 256.  With preact != 0 the inputs are the top layer's
   PRE-activations z and tanh(z + zb) is applied on load (the layer's
   separate tanh pass is then skipped); zb_pi / zb_vf (nullable, hd floats,
   16-byte aligned; only with preact) are the top layer's biases when its
   GEMM left them out.  Row buffers 16-byte aligned. */
int dr_policy_heads(int64_t m, int64_t hd, int preact, const float *h_pi,
                    const float *h_vf, const float *zb_pi, const float *zb_vf,
                    const float *w_act, const float *b_act, const float *w_val,
                    const float *b_val, float *mean, float *value, void *stream);

/* One PPO.train minibatch step from the top hidden layer down, fused:
   heads (as dr_policy_heads), the loss of dr_ppo_loss (aux = interleaved
   (m,3) rows of old_logp, advantage, return; with `rows` non-null, minibatch
   row r reads actions / aux row rows[r]), and the backward through the
   heads and the top tanh:
     gz_pi = (dL/dmean W_act) * (1 - h_pi^2),  gz_vf = (dL/dvalue W_val) *
     (1 - h_vf^2)   (m,hd) each, for the hidden-layer backward,
   plus the gradients of W_act (4,hd), b_act (4), W_val (1,hd), b_val (1),
   the top hidden biases b_pi, b_vf (hd) and log_std (4), and stats (8) as
   dr_ppo_loss.  Gradient outputs are written (not accumulated); they may be
   views into one flat gradient buffer.  Deterministic (fixed-order partial
   sums).  `preact`, zb_pi, zb_vf as dr_policy_heads (h_pi / h_vf
   pre-activations; grad_z uses tanh(z + zb)).  `workspace` >= dr_ppo_head_workspace_bytes(m, hd).
   normalize_advantage: 0 off, 1 on, 2 on with the advantage partials
   already written to the head of `workspace` by dr_gather_minibatch.
   defer != 0: the gradient / stats outputs are NOT written here; the
   reduced partials stay in `workspace` for dr_grad_finish_clip_adam (defer
   2: unreduced, for a finish with head_direct = 1; no grouping launch). */
size_t dr_ppo_head_workspace_bytes(int64_t m, int64_t hd);
int dr_ppo_head_loss_backward(int64_t m, int64_t hd, int preact, const float *h_pi,
                              const float *h_vf, const float *zb_pi,
                              const float *zb_vf, const float *w_act,
                              const float *b_act, const float *w_val,
                              const float *b_val, const float *log_std,
                              const float *actions, const float *aux,
                              const int32_t *rows, float clip_range,
                              float ent_coef, float vf_coef,
                              int normalize_advantage, float *gz_pi,
                              float *gz_vf, float *g_w_act, float *g_b_act,
                              float *g_w_val, float *g_b_val, float *g_b_pi,
                              float *g_b_vf, float *g_log_std, float *stats,
                              int defer, void *workspace, size_t workspace_bytes,
                              void *stream);

/* Fused PPO loss + gradient of the loss w.r.t. the policy head outputs
   (PPO.train: normalised advantage, ratio/clip surrogate, value MSE,
   entropy).  Inputs for a minibatch of m rows:
     mean (m,4), log_std (4), values (m), actions (m,4), old_logp (m),
     advantages (m), returns (m); old_logp / advantages / returns are read
     with element stride aux_stride (1: three arrays; 3: one interleaved
     (m,3) array of rows (old_logp, advantage, return), the rollout
     buffer's gathered minibatch, no repacking copies).
   Outputs:
     grad_mean (m,4), grad_values (m), grad_log_std (4): dLoss/d(.)
     stats (8) f32: [loss, policy_loss, value_loss, entropy_loss,
                     clip_fraction, approx_kl, adv_mean, adv_std]
   `workspace` >= dr_ppo_loss_workspace_bytes(m). */
size_t dr_ppo_loss_workspace_bytes(int64_t m);
int dr_ppo_loss(int64_t m, const float *mean, const float *log_std,
                const float *values, const float *actions,
                const float *old_logp, const float *advantages,
                const float *returns, int64_t aux_stride, float clip_range,
                float ent_coef,
                float vf_coef, int normalize_advantage, float *grad_mean,
                float *grad_values, float *grad_log_std, float *stats,
                void *workspace, size_t workspace_bytes, void *stream);

/* clip_grad_norm_(max_norm) + Adam step over one flat fp32 parameter
   buffer (torch.optim.Adam semantics, bias-corrected, eps outside sqrt).
   `step` is the 1-based Adam step count.  grad_norm_out (1) f32 nullable.
   lr / betas / eps are doubles because torch forms 1-beta, lr/bias_correction
   from Python floats before rounding them to f32 scalars.
   `workspace` >= dr_adam_workspace_bytes(n). */
size_t dr_adam_workspace_bytes(int64_t n);
int dr_clip_adam(int64_t n, float *params, float *grads, float *exp_avg,
                 float *exp_avg_sq, double lr, double beta1, double beta2,
                 double eps, float max_grad_norm, int64_t step,
                 float *grad_norm_out, void *workspace,
                 size_t workspace_bytes, void *stream);

/* The deferred reductions of one fused PPO.train minibatch step (the
   single-GPU path): the level-2 partial sums left by
   dr_ppo_head_loss_backward(..., defer = 1) and
   dr_first_layer_backward2(..., defer = 1), and the split-K chunk sum of
   the weight gradients above the first layer,
     chunk_dst[g*chunk_size + i] = sum_c chunks[(g*chunk_count + c)*chunk_size + i].
   Any of the three sources may be NULL (segment skipped); together they
   must write every entry of the flat gradient passed to
   dr_grad_finish_clip_adam, whose norm they also form. */
typedef struct dr_grad_finish {
    const void *head_workspace;      /* dr_ppo_head_loss_backward's */
    int64_t head_m, head_hd;
    const float *log_std;
    float ent_coef, vf_coef;
    float *g_w_act, *g_b_act, *g_w_val, *g_b_val, *g_b_pi, *g_b_vf, *g_log_std;
    float *stats;                    /* (8), as dr_ppo_head_loss_backward */
    const void *first_workspace;     /* dr_first_layer_backward2's */
    int64_t first_m, first_k, first_n;
    float *g_w0, *g_b0, *g_w1, *g_b1;
    const float *chunks;
    int64_t chunk_groups, chunk_count, chunk_size;
    float *chunk_dst;
    /* 0: first_workspace holds dr_first_layer_backward2's level-1 groups;
       > 0: that many per-block rows at its start, left by
       dr_gemm_x6_bwd_first(..., direct = 1) (= dr_gemm_x6_bwd_first_rows(m);
       summed by the finish, no grouping launch).  (ABI v15.) */
    int64_t first_rows;
    /* 0: head_workspace holds the level-1 groups; 1: the head kernel's
       per-block rows, left by dr_ppo_head_loss_backward(..., defer = 2)
       (summed by the finish in the grouped order: bitwise the same).
       (ABI v15.) */
    int64_t head_direct;
} dr_grad_finish;

/* dr_clip_adam fused with the deferred gradient finish: one launch reduces
   every deferred partial into `grads` (and the loss stats) and forms the
   norm partials, a second applies clip_grad_norm_ + Adam.  Two launches
   instead of six.  `workspace` >= dr_grad_finish_workspace_bytes(f). */
size_t dr_grad_finish_workspace_bytes(const dr_grad_finish *f);
int dr_grad_finish_clip_adam(const dr_grad_finish *f, int64_t n, float *params,
                             float *grads, float *exp_avg, float *exp_avg_sq,
                             double lr, double beta1, double beta2,
                             double eps, float max_grad_norm, int64_t step,
                             float *grad_norm_out, void *workspace,
                             size_t workspace_bytes, void *stream);

/* Host-only: torch.optim.Adam's step-dependent scalars for step >= 1, as
   dr_clip_adam / dr_grad_finish_clip_adam form them: out[0] = lr /
   (1 - beta1^step), out[1] = sqrt(1 - beta2^step), in double, then f32.
   (ABI v9.) */
int dr_adam_schedule(double lr, double beta1, double beta2, int64_t step, float *out);

/* dr_grad_finish_clip_adam with the step's two scalars read on the device
   from `sched` (2 floats, 8-byte aligned, filled from dr_adam_schedule):
   a training loop captured once into a hipGraph replays with the right
   bias corrections when the host rewrites the schedule between replays.
   Bitwise dr_grad_finish_clip_adam for the same step.  (ABI v9.) */
int dr_grad_finish_clip_adam_sched(const dr_grad_finish *f, int64_t n, float *params,
                                   float *grads, float *exp_avg, float *exp_avg_sq,
                                   double lr, double beta1, double beta2, double eps,
                                   float max_grad_norm, const float *sched,
                                   float *grad_norm_out, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* The data-parallel split of dr_grad_finish_clip_adam_sched (SB3 PPO.train
   + the north_star's one gradient all-reduce per optimizer step over ranks,
   /root/reference/train.py:63-68): dr_grad_finish_run reduces every deferred
   partial of `f` into the flat gradient (and the loss stats) in ONE launch;
   the caller then sums the gradient over ranks (RCCL all-reduce) and
   dr_clip_adam_sched applies clip_grad_norm_ + Adam to grad_scale * grads
   (grad_scale = 1 / world: the mean) with the step's scalars read on the
   device from `sched` (dr_adam_schedule).  At grad_scale 1 the pair is
   bitwise dr_grad_finish_clip_adam_sched; both are graph-capturable.
   dr_grad_finish_run's `workspace` >= dr_grad_finish_workspace_bytes(f);
   dr_clip_adam_sched's >= dr_adam_workspace_bytes(n).  (ABI v12.) */
int dr_grad_finish_run(const dr_grad_finish *f, void *workspace, size_t workspace_bytes,
                   void *stream);
int dr_clip_adam_sched(int64_t n, float *params, float *grads, float *exp_avg,
                       float *exp_avg_sq, double beta1, double beta2, double eps,
                       float max_grad_norm, float grad_scale, const float *sched,
                       float *grad_norm_out, void *workspace, size_t workspace_bytes,
                       void *stream);

/* KL control of the optimizer step: SB3's target_kl
   early stop and a KL-adaptive learning rate, decided on the device by the
   launch that applies Adam, so a training loop captured into a hipGraph needs
   no host round trip.  `control` is device memory of num_steps + 1 slots of
   16 bytes, (stopped u32, taken u32, lr f32, pad); optimizer step `step` of
   the iteration reads slot `step` and writes slot `step + 1` (the caller
   fills slot 0: stopped 0, taken 0, the learning rate).  `kl` points at this
   step's approx_kl (stats[5] of the loss), final before the launch.  In this
   order:
     1. slot.stopped: nothing is applied; params, exp_avg, exp_avg_sq and grads
        stay as they are (grads unclipped), grad_norm_out is still written, the
        next slot is a copy;
     2. stop_kl > 0 and kl > stop_kl (false for NaN): stopped <- 1, taken and
        lr carried, nothing applied (the tripping minibatch is not applied);
     3. adaptive: kl > kl_high: lr <- max(lr / 1.5f, lr_min); else 0 < kl <
        kl_low: lr <- min(lr * 1.5f, lr_max) (f32, one rounding per operation);
     4. clip_grad_norm_ + Adam exactly as dr_clip_adam_sched at grad_scale 1,
        with the step scalars sched[taken] (`sched`: (num_steps, 2) rows of
        dr_adam_schedule, 8-byte aligned) -- step_size = sched[taken][0], or
        with adaptive (a table built at lr 1) lr * sched[taken][0]; the next
        slot gets (0, taken + 1, lr).
   Every block of the launch takes the same decision from the same words; there
   is no atomic, so reruns and graph replays are bitwise equal. */
typedef struct dr_kl_gate {
    void *control;
    int64_t num_steps, step;
    const float *kl;
    const float *sched;
    float stop_kl;                   /* f32(1.5 * target_kl); 0: no target */
    int32_t adaptive;                /* 0 / 1 */
    float kl_high, kl_low;           /* 2 * desired_kl, desired_kl / 2 */
    float lr_min, lr_max;
} dr_kl_gate;

/* dr_clip_adam_sched (grad_scale 1) and dr_grad_finish_clip_adam_sched behind
   the gate.  Workspaces as theirs.  (ABI v16.) */
int dr_clip_adam_kl(int64_t n, float *params, float *grads, float *exp_avg,
                    float *exp_avg_sq, double beta1, double beta2, double eps,
                    float max_grad_norm, const dr_kl_gate *gate, float *grad_norm_out,
                    void *workspace, size_t workspace_bytes, void *stream);
int dr_grad_finish_clip_adam_kl(const dr_grad_finish *f, int64_t n, float *params,
                                float *grads, float *exp_avg, float *exp_avg_sq,
                                double beta1, double beta2, double eps,
                                float max_grad_norm, const dr_kl_gate *gate,
                                float *grad_norm_out, void *workspace,
                                size_t workspace_bytes, void *stream);

/* ---- fp32-accurate 256 x 256 layer GEMM on the bf16 matrix cores ---------
   Replaces the torch fp32 Linear of SB3's MlpExtractor 256 -> 256 layer
   (forward z = h W^T and the input gradient grad_h = grad_z W; reference
   policy net_arch at /root/reference/train.py:36-43).  Operands are split
   exactly into three bf16 planes and multiplied with six MFMA products per
   element pair (csrc/gemm_x6.hip); the error against an f64 GEMM is below
   the f32 MFMA GEMM's.  (ABI v10.) */

/* Bytes of the pre-split weight image of `batch` (1 or 2) 256 x 256 layers. */
size_t dr_gemm_x6_weights_bytes(int64_t batch);

/* Split `batch` row-major 256 x 256 f32 weights w (consecutive) into the
   image dr_gemm_x6 reads: transpose 0 for C = A W^T, 1 for C = A W, 2 for
   both in one launch (the transpose-0 image at img, the transpose-1 image
   right after it).  img 16-byte aligned, dr_gemm_x6_weights_bytes(batch)
   bytes (twice that for transpose 2). */
int dr_gemm_x6_split_weights(int64_t batch, const float *w, int transpose, void *img,
                             void *stream);

/* C[b] = A[b] . Bt[b]^T for b < batch: A (batch, m, 256) f32, C (batch, m,
   256) f32, Bt given by img.  m a positive multiple of 128; a, img and c
   16-byte aligned.  Deterministic. */
int dr_gemm_x6(int64_t batch, int64_t m, const float *a, const void *img, float *c,
               void *stream);

/* The layer's weight gradient on the same arithmetic, split over `chunks`
   row chunks: ws[b][c] (256 x 256) = G[b][rows of chunk c]^T H[b][rows of
   chunk c] for G (batch, m, 256) = grad_z and H (batch, m, 256) = the layer
   input (torch's split-K bmm layout; the caller sums the chunks).
   m / chunks a positive multiple of 32; pointers 16-byte aligned.
   Deterministic.  (ABI v10.) */
int dr_gemm_x6_wgrad(int64_t batch, int64_t m, int64_t chunks, const float *g, const float *h,
                     float *ws, void *stream);

/* The first-layer operand image of dr_gemm_x6_bwd_first: the minibatch
   observations x (m x k f32 row-major, k <= 15) with a constant 1 as the
   16th feature, split exactly into three bf16 planes in the MFMA fragment
   order (dr_gemm_x6_x_bytes(m) bytes, 16-byte aligned).  (ABI v15.) */
size_t dr_gemm_x6_x_bytes(int64_t m);
int dr_gemm_x6_split_x(int64_t m, int64_t k, const float *x, void *ximg, void *stream);

/* The 256 x 256 layer's input gradient with the first layer's backward
   fused into its epilogue (replaces dr_gemm_x6(2, m, grad_z, img W-form,
   grad_h) followed by dr_first_layer_backward2(..., defer = 1); PPO.train's
   backward through SB3's MlpExtractor, /root/reference/train.py:36-43):
   grad_h1 = grad_z W per net stays in registers, grad_z1 = grad_h1 (1 - h^2)
   with h (2, m, 256) the first layer's activations, and the first layer's
   weight and bias gradients accumulate on the matrix cores against ximg
   (dr_gemm_x6_split_x of the same minibatch's x, k = 15).  `workspace` is
   dr_first_layer_backward2's (>= dr_first_layer_backward2_workspace_bytes(m,
   15, 256)) and is left exactly as its defer = 1 form leaves it: the next
   dr_grad_finish / dr_grad_finish_clip_adam with first_workspace =
   workspace writes the gradients.  With direct != 0 the kernel's per-block
   rows are left at the workspace start instead (no grouping launch) for a
   finish with first_rows = dr_gemm_x6_bwd_first_rows(m).  batch 2, m a
   positive multiple of 128, pointers 16-byte aligned.  Deterministic.
   (ABI v15.) */
int dr_gemm_x6_bwd_first(int64_t batch, int64_t m, int64_t k, const float *grad_z,
                         const void *img, const float *h, const void *ximg, void *workspace,
                         size_t workspace_bytes, int direct, void *stream);
/* The number of per-block rows dr_gemm_x6_bwd_first(..., direct = 1) leaves
   at m rows on the current device (0 for an invalid m). */
int64_t dr_gemm_x6_bwd_first_rows(int64_t m);

/* dr_linear_tanh2 (k = 15, n = 256) with the x6 GEMMs' operand images built
   by extra blocks of the same launch: both weight forms of the 256 x 256
   layer into img (dr_gemm_x6_split_weights(2, w256, 2, img) -- w256 the
   (2, 256, 256) weights of both nets) and, with ximg non-null, the
   observation image of dr_gemm_x6_bwd_first (dr_gemm_x6_split_x of x, read
   through rows when given; m a multiple of 128).  The same bytes as the
   separate launches.  (ABI v15.) */
int dr_linear_tanh2_x6(int64_t m, int64_t k, int64_t n, const float *x, const int32_t *rows,
                       const float *w0, const float *b0, float *h0, const float *w1,
                       const float *b1, float *h1, const float *w256, void *img, void *ximg,
                       void *stream);

/* ---------------------------------------------------------------------------
 * VecNormalize: stable-baselines3's running
 * observation / reward normalisation with its statistics as device state, so
 * that it can sit inside a captured rollout.  All buffers are device memory.
 *
 * A RunningMeanStd is (count, mean, var) in f64, initially (1e-4, 0, 1).  Its
 * update over the N rows of a batch takes per column bm = mean(x), bv = the
 * population variance of x, bc = N, and sets
 *     d = bm - mean;  tot = count + bc;
 *     mean <- mean + d * bc / tot;
 *     var  <- (var * count + bv * bc + d * d * count * bc / tot) / tot;
 *     count <- tot.
 * State: obs_rms f64[1 + 2 D] = count, mean[D], var[D]; ret_rms f64[3] =
 * count, mean, var; returns f64[N], the running discounted return per env.
 *
 * dr_vecnorm_step, in this order (flags: DR_VECNORM_*):
 *   1. TRAINING and OBS: obs_rms.update(obs), the f32 values widened exactly;
 *   2. obs_out = f32(clip((f64(obs) - mean) / sqrt(var + epsilon), -clip_obs,
 *      clip_obs)) with the statistics as they now are (OBS off: a copy);
 *   3. TRAINING and REWARD: returns <- returns * gamma + rewards, then
 *      ret_rms.update(returns) over all N envs, done ones included (SB3
 *      updates ret_rms whenever training but reads it only with REWARD: here
 *      it stays untouched without REWARD);
 *   4. rew_out = f32(clip(f64(rewards) / sqrt(ret_var + epsilon),
 *      -clip_reward, clip_reward)) (REWARD off: a copy);
 *   5. with terminal_obs: rows of done envs are normalised as in 2 into
 *      terminal_obs_out; rows of envs that are not done are left untouched;
 *   6. returns[done] <- 0.
 * rewards == NULL is the reset form: returns <- 0 for every env, then 1 and 2
 * (dones and the terminal buffers must be NULL too).  obs_out may be obs and
 * rew_out may be rewards (in place).  The moments are one pass of per-block
 * (n, mean, M2) partials merged in a fixed order (Chan et al.), all in f64,
 * bv = M2 / N: results depend on the inputs alone and are bitwise equal from
 * run to run and under graph replay.  At most three launches, no host sync, no
 * atomics; nothing is kept in `workspace` between calls.
 * Non-finite inputs get no special treatment: a NaN or inf in a column poisons
 * that column's statistics for good, as in SB3, and the clip passes NaN on.
 *
 * DR_ERR_INVALID, before any HIP call, with a dr_last_error(NULL) message:
 * n or m < 1, obs_dim outside [1, 24], a clip that is not > 0 and finite,
 * epsilon < 0 or non-finite, a non-finite gamma, unknown flag bits, a missing
 * buffer, or a workspace smaller than dr_vecnorm_workspace_bytes(n, obs_dim).
 * These additions break no caller: DR_ABI_VERSION stays 16.
 * ------------------------------------------------------------------------- */
enum dr_vecnorm_flags {
    DR_VECNORM_OBS = 1,       /* normalise observations                      */
    DR_VECNORM_REWARD = 2,    /* normalise rewards                           */
    DR_VECNORM_TRAINING = 4   /* advance the statistics                      */
};

size_t dr_vecnorm_workspace_bytes(int64_t n, int64_t obs_dim);

/* obs_rms <- (1e-4, 0, 1), ret_rms <- (1e-4, 0, 1), returns <- 0. */
int dr_vecnorm_init(int64_t n, int64_t obs_dim, double *obs_rms, double *ret_rms,
                    double *returns, void *stream);

int dr_vecnorm_step(int64_t n, int64_t obs_dim, const float *obs, const float *rewards,
                    const uint8_t *dones, const float *terminal_obs, int flags, double gamma,
                    double clip_obs, double clip_reward, double epsilon, double *obs_rms,
                    double *ret_rms, double *returns, float *obs_out, float *rew_out,
                    float *terminal_obs_out, void *workspace, size_t workspace_bytes,
                    void *stream);

/* Step 2 alone on m rows (any m) with frozen statistics: evaluation, and the
   minibatches of callers that keep raw observations. */
int dr_vecnorm_apply(int64_t m, int64_t obs_dim, const float *obs, const double *obs_rms,
                     double clip_obs, double epsilon, float *obs_out, void *stream);

/* VecNormalize.unnormalize_obs: obs_out = f32(f64(obs_norm) * sqrt(var +
   epsilon) + mean) on m rows (the clip is not undone). */
int dr_vecnorm_unapply(int64_t m, int64_t obs_dim, const float *obs_norm, const double *obs_rms,
                       double epsilon, float *obs_out, void *stream);

/* ---------------------------------------------------------------------------
 * SensorModel: what the policy sees of the env's clean
 * observation -- per-column noise, a per-episode bias and a per-episode
 * latency -- as a wrapper with its state on the device, so that it can sit
 * inside a captured rollout, around any variant and any env option.  The obs
 * width is unchanged.  All buffers are device memory, owned by the caller and
 * separate (there is no packed state blob, so a checkpoint and a test can read
 * each word):
 *     state  int32[3][n]      ep (u32 bits), s, d per env
 *     bias   float[n][obs_dim]
 *     ring   float[delay_hi + 1][n][obs_dim]   clean observations
 * ep counts the episodes the wrapper has started for the env, s the
 * deliveries since the episode began, d is the episode's delay in steps.  The
 * wrapper reads none of the env's counters.
 *
 * Episode start (every env at dr_sensor_reset; in dr_sensor_step an env whose
 * done is set, obs being the new episode's first observation): ep <- 0 at a
 * reset, ep + 1 after a done; s <- 0; with the Philox blocks of counter
 * (ep, gid_lo, gid_hi, word) under the key `seed`, gid = env_id_offset + env,
 *     d      <- delay_lo + ((uint64(w0 of word 0x53000000) * (delay_hi -
 *               delay_lo + 1)) >> 32)
 *     bias_c <- beta_c * pm1(word c % 4 of block 0x53000000 | (1 + c / 4)),
 * pm1(w) = f32(2 (w 2^-32) - 1); all delay_hi + 1 ring slots <- obs.
 * Delivery at count s: x = ring[(s - d) mod (delay_hi + 1)];
 *     e_c = bias_c + sigma'_c * pm1(word c % 4 of block
 *           ((0x60 + c / 4) << 24) | (s & 0xffffff)),
 * sigma'_c = f32(f64(sigma_c) * sqrt(3)); out_c = x_c + e_c, or x_c - e_m for
 * a column with mirror[c] = m >= 0; a column whose sigma and beta (its
 * source's, for a mirror) are both 0 is delivered unchanged, x_c.  Every f32
 * operation rounds once, none is contracted.  s enters the counter modulo
 * 2^24: episodes must be shorter than that.
 * dr_sensor_step per env: not done -- s <- s + 1, ring[s mod L] <- obs,
 * deliver; done -- with the terminal pair, terminal_out[env] is the delivery
 * the old episode would have made at s + 1 with terminal_obs[env] as that
 * step's clean row (rows of envs that are not done are left untouched); then
 * the episode start on obs[env] and its delivery at count 0.  obs_out may be
 * obs.  One launch each, no atomics, no host sync: results are bitwise equal
 * from run to run and under graph replay.
 *
 * DR_ERR_INVALID, before any HIP call, with a dr_last_error(NULL) message
 * naming the argument: a null config, n < 1, obs_dim outside [1, 24], a
 * negative or non-finite sigma or beta, a mirror index outside [-1, c), a
 * delay pair that is not 0 <= delay_lo <= delay_hi <= 15, a missing buffer,
 * terminal_obs without terminal_out or the reverse.
 * These additions break no caller: DR_ABI_VERSION stays 16.
 * ------------------------------------------------------------------------- */
#define DR_SENSOR_MAX_DIM 24
#define DR_SENSOR_MAX_DELAY 15

typedef struct dr_sensor_config {
    int32_t delay_lo, delay_hi;          /* the delay is drawn from [lo, hi]     */
    uint64_t seed;                       /* Philox key                           */
    int64_t env_id_offset;               /* global id of env 0                   */
    float sigma[DR_SENSOR_MAX_DIM];      /* noise std per column                 */
    float beta[DR_SENSOR_MAX_DIM];       /* bias half-width per column           */
    int32_t mirror[DR_SENSOR_MAX_DIM];   /* -1, or the column whose error this
                                            one shows with the opposite sign     */
} dr_sensor_config;

int dr_sensor_reset(const dr_sensor_config *cfg, int64_t n, int64_t obs_dim, const float *obs,
                    int32_t *state, float *bias, float *ring, float *obs_out, void *stream);

int dr_sensor_step(const dr_sensor_config *cfg, int64_t n, int64_t obs_dim, const float *obs,
                   const uint8_t *dones, const float *terminal_obs, int32_t *state, float *bias,
                   float *ring, float *obs_out, float *terminal_out, void *stream);

/* ---------------------------------------------------------------------------
 * MPPIPlanner: model-predictive path integral control
 * on the gym env's own step.  For every env it flies `samples` perturbed
 * action sequences `horizon` steps ahead from the env's 15-float observation,
 * weights them by exponentiated return and outputs the first action of the
 * weighted mean; the mean, shifted by one step, warm-starts the next call.
 * The planner's model is the nominal airframe in still air; it reads no env
 * handle, only the observation a policy would see.  All buffers are device
 * memory, owned by the caller and separate:
 *     nominal  float[n][horizon][4]   the warm start U
 *     calls    uint32[n]              plan steps since the reset
 * dr_mppi_reset: every nominal entry <- f32(9.81 / 4) (hover), calls <- 0.
 * dr_mppi_step for env e (gid = env_id_offset + e), with S = samples,
 * H = horizon, M = f32(3 * 9.81 / 4), clip(x) = x < 0 ? 0 : x > M ? M : x:
 *  0. where dones is given and dones[e] is set, obs[e] opens a new episode:
 *     U <- hover first.
 *  1. Start state in f64: p, v, euler, omega = (double)obs[0..11]; target_k =
 *     (double)obs[k] + (double)obs[12 + k].
 *  2. Sample s at step h: a_k = clip(U[h][k]) for s = 0, else
 *     clip(U[h][k] + sigma' * pm1(w_k)) in f32, one rounding per operation,
 *     w the Philox4x32-10 block of counter (calls, gid_lo, gid_hi, 0x4D000000 |
 *     (s * H + h)) under the key `seed`, pm1(w) = f32(2 (w 2^-32) - 1),
 *     sigma' = f32(sigma * sqrt(3)).
 *  3. The sample steps the gym env's f64 step (dt = 0.02, no reset inside the
 *     horizon).  While it has not crashed before step h,
 *         J <- J + disc[h] * ((double)(float)r - (crash ? crash_cost : 0)),
 *     r and crash that step's reward and crash flag, disc[0] = 1, disc[h] =
 *     disc[h - 1] * gamma.  A sample that never crashed ends with J <- J -
 *     terminal_weight * d, d = sqrt((dx dx + dy dy) + dz dz) from the final
 *     position to the target.
 *  4. Jmax = the maximum J over the samples whose J is not NaN; w_s =
 *     exp((J_s - Jmax) / temperature), 0 where J_s is NaN; W = sum of w_s, all
 *     in f64 and in a fixed order.  Where Jmax is not finite (no sample has a
 *     finite return: a NaN observation) the nominal is left as it is (as step
 *     0 left it) and actions_out[e] = clip(U[0]); calls still counts on.
 *  5. U_new[h][k] = f32(sum_s w_s * (double)a_s[h][k] / W).
 *  6. actions_out[e] = U_new[0]; nominal[h] <- U_new[h + 1] for h < H - 1,
 *     nominal[H - 1] <- U_new[H - 1]; calls <- calls + 1.
 *  7. costs_out, where given: double[n][S], every J_s.
 * One launch each, asynchronous on `stream`, no atomics, no host sync: results
 * are bitwise equal from run to run and under graph replay.  The config is
 * copied into the kernel's arguments at the call.
 *
 * DR_ERR_INVALID, before any HIP call, with a dr_last_error(NULL) message
 * naming the argument: a null config, n < 1, samples not one of 64, 128, 256,
 * 512, 1024, horizon outside [1, 32], sigma, crash_cost or terminal_weight
 * negative or not finite, temperature not > 0 and finite, gamma outside
 * (0, 1], a missing nominal, calls, obs or actions_out.
 * These additions break no caller: DR_ABI_VERSION stays 16.
 * ------------------------------------------------------------------------- */
#define DR_MPPI_MAX_SAMPLES 1024
#define DR_MPPI_MAX_HORIZON 32

typedef struct dr_mppi_config {
    int32_t samples;                     /* S: 64, 128, 256, 512 or 1024         */
    int32_t horizon;                     /* H: 1 .. 32 steps                     */
    double sigma;                        /* action noise std, newtons per motor  */
    double temperature;                  /* lambda                               */
    double gamma;                        /* discount per step                    */
    double crash_cost;                   /* what the step that crashes pays      */
    double terminal_weight;              /* on the final distance to the target  */
    uint64_t seed;                       /* Philox key                           */
    int64_t env_id_offset;               /* global id of env 0                   */
} dr_mppi_config;

int dr_mppi_reset(const dr_mppi_config *cfg, int64_t n, float *nominal, uint32_t *calls,
                  void *stream);

int dr_mppi_step(const dr_mppi_config *cfg, int64_t n, const float *obs, const uint8_t *dones,
                 float *nominal, uint32_t *calls, float *actions_out, double *costs_out,
                 void *stream);

/* ---------------------------------------------------------------------------
 * GradPlanner: gradient trajectory planning by the
 * adjoint of the gym env's own step.  For every env it takes `iterations` Adam
 * steps on the warm-started action sequence U, each on the gradient of a
 * quadratic tracking cost through `horizon` steps of the gym env's f64 step,
 * and outputs the first action; the sequence, shifted by one step, warm-starts
 * the next call.  The model is the nominal airframe in still air; it reads no
 * env handle, only the 15-float observation a policy would see.  Device
 * buffers, owned by the caller and separate:
 *     nominal    float[n][horizon][4]   the warm start U
 *     workspace  dr_gplan_workspace_bytes(n, horizon) bytes, 8-byte aligned;
 *                scratch of one call, nothing is kept in it between calls
 * dr_gplan_reset: every nominal entry <- f32(9.81 / 4) (hover).
 * dr_gplan_step for env e, with H = horizon, M = f32(3 * 9.81 / 4), clip(x) =
 * x < 0 ? 0 : x > M ? M : x, hover = (double)f32(9.81 / 4):
 *  0. where dones is given and dones[e] is set, obs[e] opens a new episode:
 *     U <- hover first.
 *  1. Start state in f64: p, v, euler, omega = (double)obs[0..11]; target_k =
 *     (double)obs[k] + (double)obs[12 + k].
 *  2. The cost of U: H gym steps (dt = 0.02, no reset, the crash rule and the
 *     bonus play no part) on a_h = clip(U[h]); after step h, on the new state,
 *         c <- c + ((((w_pos |p - target|^2 + w_vel |v|^2) + w_att |euler|^2)
 *                    + w_rate |omega|^2) + w_effort |a_h - hover|^2),
 *     |x|^2 = (x0 x0 + x1 x1) + x2 x2, and after the last step
 *         c <- c + (w_pos_final |p - target|^2 + w_vel_final |v|^2).
 *  3. g = dc/dU, double[H][4], by the adjoint of the step; the f32 casts and
 *     the clip are taken as the identity.
 *  4. Adam, fresh at every call (m = s = 0), for it = 1 .. iterations:
 *         m <- beta1 m + (1 - beta1) g;  s <- beta2 s + (1 - beta2) (g g);
 *         U <- clip((float)((double)U - (lr (m / (1 - beta1^it)))
 *                                       / (sqrt(s / (1 - beta2^it)) + adam_eps)))
 *     with beta^it the running product, and g taken anew on the updated U.
 *  5. Where the cost or a gradient entry of iteration 1 is not finite (a NaN
 *     observation) the nominal is left as step 0 left it and actions_out[e] =
 *     clip(U[0]); no other env is touched.
 *  6. actions_out[e] = U[0]; nominal[h] <- U[h + 1] for h < H - 1,
 *     nominal[H - 1] <- U[H - 1].
 *  7. cost_out, where given: double[n], the cost of the incoming nominal (as
 *     step 0 left it); grad_out, where given: double[n][H][4], its gradient.
 * One launch each, asynchronous on `stream`, no atomics, no host sync: results
 * are bitwise equal from run to run and under graph replay.  The config is
 * copied into the kernel's arguments at the call.
 *
 * DR_ERR_INVALID, before any HIP call, with a dr_last_error(NULL) message
 * naming the argument: a null config, n < 1, horizon outside [1, 32],
 * iterations outside [1, 64], lr or adam_eps not > 0 and finite, beta1 or
 * beta2 outside [0, 1), a weight negative or not finite, a missing nominal,
 * obs, actions_out or workspace, a workspace that is not 8-byte aligned or
 * smaller than dr_gplan_workspace_bytes(n, horizon) (which is 0 for an n or a
 * horizon outside its range).
 * These additions break no caller: DR_ABI_VERSION stays 16.
 * ------------------------------------------------------------------------- */
#define DR_GPLAN_MAX_HORIZON 32
#define DR_GPLAN_MAX_ITERATIONS 64

typedef struct dr_gplan_config {
    int32_t horizon;                     /* H: 1 .. 32 steps                     */
    int32_t iterations;                  /* Adam steps per call: 1 .. 64         */
    double lr;                           /* Adam step, newtons per motor         */
    double beta1, beta2, adam_eps;
    double w_pos, w_vel, w_att, w_rate;  /* per step, on the new state           */
    double w_effort;                     /* per step, on a_h - hover             */
    double w_pos_final, w_vel_final;     /* on the state after the last step     */
} dr_gplan_config;

size_t dr_gplan_workspace_bytes(int64_t n, int32_t horizon);

int dr_gplan_reset(const dr_gplan_config *cfg, int64_t n, float *nominal, void *stream);

int dr_gplan_step(const dr_gplan_config *cfg, int64_t n, const float *obs, const uint8_t *dones,
                  float *nominal, void *workspace, size_t workspace_bytes, float *actions_out,
                  double *cost_out, double *grad_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DRONERL_H_ */
