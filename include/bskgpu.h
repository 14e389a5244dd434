/*
 * bskgpu.h — C-ABI of libbskgpu.so: batched MI355X (gfx950) spacecraft propagator.
 *
 * This is the drop-in boundary for ONE hot path of atharris/basilisk_env: the per-env-step
 * call into the Basilisk engine,
 *     LEOPowerAttitudeSimulator.run_sim -> ConfigureStopTime + ExecuteSimulation
 *     (reference basilisk_env/simulators/leoPowerAttitudeSimulator.py:535-644, hot call :594-595)
 * for N independent spacecraft at once.  Plain pointers and sizes only; no torch / numpy types.
 * Every entry point returns 0 on success or a negative BSK_E* code and never throws.
 * `bsk_last_error()` returns a thread-local message for the last failure on this thread.
 *
 * Ownership: the caller owns every host buffer; the library owns every device buffer.
 * One handle <-> one device <-> one HIP stream.  A handle is not thread-safe; distinct handles are.
 * There is NO CPU fallback: bsk_create fails with BSK_ENODEV when no gfx950 device is usable.
 *
 * Layouts are structure-of-arrays, fp64: field f of env i lives at buf[f * n_envs + i]
 * on the host side of this ABI (the device side pads the env stride to a multiple of 256).
 */
#ifndef BSKGPU_H
#define BSKGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSK_ABI_VERSION 4u
#define BSK_MAX_RW 4
#define BSK_MAX_THR 8
#define BSK_MAX_SH_DEGREE 70

/* error codes */
#define BSK_OK 0
#define BSK_EINVAL (-1)   /* bad argument / config */
#define BSK_ENODEV (-2)   /* no usable gfx950 device */
#define BSK_ENOMEM (-3)   /* device allocation failed */
#define BSK_EHIP (-4)     /* HIP runtime error (see bsk_last_error) */
#define BSK_EABI (-5)     /* bsk_config abi_version / struct_size mismatch */

/* gravity models (reference: gravBodyFactory, leoPowerAttitudeSimulator.py:217-232; the only
 * spherical-harmonics call site is opNav_models/BSK_OpNavDynamics.py:211-214) */
enum { BSK_GRAV_PM = 0, BSK_GRAV_PM_J2 = 1, BSK_GRAV_SH = 2 };

/* flags */
#define BSK_FLAG_SUN_THIRD_BODY 0x1u /* Sun third-body gravity (leoPowerAttitudeSimulator.py:227) */
#define BSK_FLAG_POWER 0x2u          /* eclipse + solar panel + battery (…Simulator.py:286-288,326-345) */
#define BSK_FLAG_DESAT 0x4u          /* action 2 fires the thruster octet (…Simulator.py:574-588) */
#define BSK_FLAG_DRAG 0x8u           /* exponential atmosphere + facet drag (…Simulator.py:265-284) */
#define BSK_FLAG_AUTO_RESET 0x10u    /* device-side masked auto-reset from a staged IC pool */
#define BSK_FLAG_EPISODE_STATS 0x40u /* device-resident episode statistics (the Monitor convention of envs/leoPowerAttitudeEnvironment.py:130-135
                                        without the host): running return per env, return / length of the episode that just ended,
                                        a 0 / 1 done byte; bsk_get_episode_device.  16 B more HBM traffic per env-step */
#define BSK_FLAG_OBS_ROWMAJOR 0x80u  /* the step kernel also writes the observation row-major, f64[n_envs][5] (what the reference's
                                        (5,1) observation stacks to, envs/leoPowerAttitudeEnvironment.py:43-45): a policy on the GPU
                                        reshapes it without a copy kernel.  40 B more per env-step */
#define BSK_FLAG_LDS_SCRATCH 0x20u   /* bare propagator only: stage the RK4 accumulator (12 doubles per spacecraft) in
                                        LDS between the stages instead of VGPRs: 3 waves per SIMD instead of 2.
                                        Same results bit for bit; timings in DESIGN.md §4 */

/* State field indices of the SoA state block, bsk_get_state / bsk_set_state / bsk_reset `ic`.
 * n_fields = BSK_NF_BASE + n_rw (wheel speeds) + BSK_NF_TAIL.                                   */
enum {
    BSK_F_R = 0,      /* r_BN_N   [m]      3 fields  (scObject.hub.r_CN_NInit,  …Simulator.py:252) */
    BSK_F_V = 3,      /* v_BN_N   [m/s]    3 fields  (…Simulator.py:253)                            */
    BSK_F_SIGMA = 6,  /* sigma_BN [-]      3 fields  (…Simulator.py:258)                            */
    BSK_F_OMEGA = 9,  /* omega_BN_B [rad/s] 3 fields (…Simulator.py:259)                            */
    BSK_NF_BASE = 12, /* wheel speeds Omega_i [rad/s] follow: n_rw fields (…Simulator.py:303-305)   */
};
/* tail fields after the wheel speeds */
enum {
    BSK_T_LEXT = 0,    /* external disturbance torque L_B [N m] 3 fields (…Simulator.py:291-298)    */
    BSK_T_UCMD = 3,    /* held wheel motor torque u_s [N m]: BSK_MAX_RW fields (zero-order hold)    */
    BSK_T_CHARGE = 7,  /* battery stored charge [W s] 1 field (…Simulator.py:343)                   */
    /* desaturation state (BSK_FLAG_DESAT; zero otherwise) */
    BSK_T_THR_REM = 8,  /* thrMomentumDumping: on-time still owed per thruster [s], BSK_MAX_THR fields */
    BSK_T_THR_LIM = 16, /* current burst: on-time per thruster in half dyn steps (integer-valued)     */
    BSK_T_THR_T0 = 24,  /* RK4 tick at which the current burst started                               */
    BSK_T_THR_CNT = 25, /* thrMomentumDumping counter (control periods until the next burst)         */
    /* FSW task order (bsk_config.fsw_lag): the wheel torque that the NEXT FSW tick will apply, i.e.
     * rwMotorTorque(MRP_Feedback(att_guidance of the last tick)); zero after a reset (empty message) */
    BSK_T_UPEND = 26,   /* BSK_MAX_RW fields                                                           */
    BSK_T_SBR = 30,     /* |sigma_BR| of the att_guidance message the last FSW tick wrote (bsk_config.nav_lag) */
    BSK_NF_TAIL = 31,
};

typedef struct bsk_config {
    uint32_t abi_version; /* = BSK_ABI_VERSION */
    uint32_t struct_size; /* = sizeof(bsk_config) */

    /* integrator / schedule (reference: dynRate .1, fswRate 1.0 — leoPowerAttitudeEnvironment.py:185) */
    double dt;         /* RK4 step [s]                                                       */
    int32_t fsw_every; /* RK4 steps per FSW update (fswRate / dynRate)                       */
    int32_t gravity_model;
    int32_t sh_degree; /* used when gravity_model == BSK_GRAV_SH                             */
    int32_t n_rw;      /* 0..BSK_MAX_RW                                                      */
    uint32_t flags;
    int32_t max_length; /* episode length in env steps (leoPowerAttitudeEnvironment.py:25)   */
    /* 1 (default, reference order): mrpControlTask runs MRP_Feedback BEFORE attTrackingError
     * (AddModelToTask order, …Simulator.py:484-486), so the controller consumes the att_guidance
     * message of the PREVIOUS FSW tick: the wheel torque lags the guidance by one FSW period and
     * the first tick after a reset commands zero (empty message).  0: guidance and control on the
     * same tick (the order the module names suggest).                                           */
    int32_t fsw_lag;
    /* 1 (default, reference priorities): the FSW tasks are created with priorities 100 / 50 (…Simulator.py:383-386),
     * the dynamics tasks with the default (:101-103), and Basilisk runs higher priorities first at equal time: the
     * FSW tick at time k*fsw_every*dt executes BEFORE the dynamics task integrates to that time — on the navigation
     * and wheel-speed messages of one integrator step earlier — and its commands (wheel torque, thruster burst) are
     * latched when the dynamics task runs, i.e. act from that time on.  The tick at t = 0 finds messages nobody has
     * written yet (zeros); a tick that coincides with the end of an env step belongs to that step, with its mode
     * (ExecuteSimulation runs the tasks scheduled at its stop time); obs[0] is the att_guidance message as the last
     * FSW tick left it.  0: an FSW tick works on the state of its own time, belongs to the env step that starts
     * there, and obs[0] is the tracking error of the end-of-step state.                                          */
    int32_t nav_lag;

    /* gravity constants (leo_orbit.py:30; REQ_EARTH at …Simulator.py:146) */
    double mu;      /* m^3/s^2 */
    double req;     /* m       */
    double j2;      /* -        */
    double planet_rate; /* rad/s, planet-fixed frame rotation about inertial z (SH only)     */

    /* hub (…Simulator.py:245-250) */
    double inertia[9]; /* I_sc about B, body frame, row-major [kg m^2] */
    double mass;       /* kg */

    /* reaction wheels (actuatorPrimatives.py:7-63; 4-wheel pyramid BSK_OpNavDynamics.py:278-291) */
    double gs[BSK_MAX_RW][3]; /* spin axes, body frame, unit */
    double js[BSK_MAX_RW];    /* spin-axis inertia [kg m^2]   */
    double u_max;             /* motor torque saturation [N m] */
    double u_min;             /* motor torque dead-band [N m]  */
    double f_coulomb;         /* Coulomb friction torque [N m] */

    /* FSW (…Simulator.py:170-180, 407-449) */
    double K, P;            /* MRP_Feedback gains (Ki < 0: integral feedback off) */
    double sigma_R0N[3];    /* inertial3D reference                               */
    double ctrl_axes[9];    /* rwMotorTorque controlAxes_B, row-major             */

    /* env constants (leoPowerAttitudeEnvironment.py:36-42; …Simulator.py:641) */
    double wheel_limit;     /* rad/s */
    double power_max;       /* W h   */
    double reward_mult;
    double failure_penalty;
    double r_min;           /* |r| below this ends the episode ("orbit decayed") */

    /* power system (…Simulator.py:158-167) */
    double panel_normal[3]; /* nHat_B */
    double panel_area, panel_efficiency;
    double power_draw;       /* W, negative = sink */
    double storage_capacity; /* W s */
    double solar_flux;       /* W/m^2 at 1 AU */

    /* Sun (replaces spice_interface, …Simulator.py:219-225): position at t = 0 and velocity,
       inertial, Earth-centred; advanced linearly once per env step like the 180 s SPICE task */
    double sun_r0[3];
    double sun_v[3];
    double mu_sun;

    /* desaturation (actuatorPrimatives.py:66-161; …Simulator.py:183-190, 452-478) */
    int32_t n_thr;
    int32_t thr_max_counter;
    double thr_pos[BSK_MAX_THR][3];
    double thr_dir[BSK_MAX_THR][3];
    double thr_max_thrust;     /* N   (MOOG Monarc-1: 0.9)                                   */
    double thr_min_fire_time;  /* s   thrMomentumDumping.thrMinFireTime (…Simulator.py:190)   */
    double thr_min_on_time;    /* s   thruster MinOnTime (MOOG Monarc-1: 0.02)               */
                               /*     with BSK_FLAG_DESAT both times are finite and >= 0, and floor(thr_min_on_time * 2 / dt)
                                      <= 65535: a burst limit is kept in 16 bits (bsk_create refuses the config otherwise) */
    double hs_min;             /* N m s  thrMomentumManagement.hs_min (…Simulator.py:183)     */

    /* drag (…Simulator.py:147-148, 272-281) */
    double base_density, scale_height;
    int32_t n_facets;
    int32_t pad0_;
    double facet_area[8], facet_cd[8];
    double facet_normal[8][3], facet_pos[8][3];
} bsk_config;

typedef struct bsk_handle bsk_handle;

/* Fill `cfg` with the reference scenario's constants (…Simulator.py:127-191) for `n_rw` wheels
 * (3 = actuatorPrimatives.py triad, 4 = BSK_OpNavDynamics.py:278-291 pyramid, 0 = none). */
int bsk_default_config(bsk_config* cfg, int n_rw, int gravity_model);

/* Replaces LEOPowerAttitudeSimulator.__init__ (…Simulator.py:67-117) for n_envs spacecraft.
 * `stream` may be NULL (the library creates its own hipStream_t) or an existing hipStream_t. */
int bsk_create(const bsk_config* cfg, int n_envs, int device_id, void* stream, bsk_handle** out);
void bsk_destroy(bsk_handle* h);

/* Normalised spherical-harmonic coefficients Cbar/Sbar, index l*(l+1)/2+m, 0<=m<=l<=degree. */
int bsk_set_gravity_sh(bsk_handle* h, int degree, const double* cbar, const double* sbar);

/* Replaces set_ICs + hub/wheel/battery initialisation (…Simulator.py:119-193, 249-259, 303-305, 343)
 * and reset_init's IC replay (leoPowerAttitudeEnvironment.py:202-216).
 * mask: NULL = all envs, else uint8[n_envs] (non-zero = reset this env).
 * ic: host SoA [n_fields][n_envs] as in the field enums above; step counters are zeroed. */
int bsk_reset(bsk_handle* h, const uint8_t* mask, const double* ic);

/* Replaces run_sim(action) (…Simulator.py:535-644) + the env's reward/done logic
 * (leoPowerAttitudeEnvironment.py:98-127,161-170) for every env: mode switch, `substeps` RK4
 * steps with the FSW chain every fsw_every steps, observation/reward/done.  Asynchronous on
 * the handle's stream.  actions: int32[n_envs] in {0,1,2} (host pointer; copied H2D). */
int bsk_step(bsk_handle* h, const int32_t* actions, int substeps);
/* Same, actions already resident in device memory (no PCIe traffic on the step path). */
int bsk_step_device(bsk_handle* h, const int32_t* d_actions, int substeps);
/* Same, actions as int64 in device memory (what torch's argmax returns: no conversion kernel between policy and step);
 * the kernel reads the low word of each little-endian element. */
int bsk_step_device_i64(bsk_handle* h, const int64_t* d_actions, int substeps);

/* Open-loop rollout: `n_steps` env steps of `substeps` RK4 sub-steps each, enqueued by ONE call - at the bare level (point mass / J2, no
 * BSK_FLAG_POWER) as ONE launch with the spacecraft's state kept in registers across the steps; at the scenario levels and with the
 * harmonics, where an env step is milliseconds of arithmetic, as one step launch + one history-row launch per env step.  What the reference's own mains do - whole episodes under one constant action
 * (envs/leoPowerAttitudeEnvironment.py:218-231; ...Simulator.py:657-694: 360 steps of action 0) - and what evaluating a fixed action
 * sequence does, without a launch, a state round trip through memory and a host visit per env step.
 *   d_actions   int32[n_steps][n_envs] in DEVICE memory, or NULL: `constant_action` at every step
 *   d_obs_hist  f64[n_steps][5][n_envs], d_reward_hist f64[n_steps][n_envs], d_reason_hist u8[n_steps][n_envs] in DEVICE memory
 *               (each may be NULL): row t = what bsk_get_obs would have returned after step t of n_steps calls of bsk_step_device -
 *               where the device-side auto-reset restarted an env, its observation row is the NEW episode's first observation (as
 *               in the observation buffers), reward and reason are the finished step's.
 * Afterwards every buffer of the handle - state, counters, observation / reward / reason / done mask, terminal observations,
 * episode counts and statistics - holds, bit for bit, what `n_steps` calls of bsk_step_device with the same actions leave.
 * Per env step the fused launch reads 4 bytes (none for a constant action) and writes 49.  Asynchronous on the handle's stream (a
 * constant action at the unfused levels goes through the handle's own action buffer, the one bsk_step stages host actions in). */
int bsk_step_n(bsk_handle* h, const int32_t* d_actions, int32_t constant_action, int substeps, int n_steps,
               double* d_obs_hist, double* d_reward_hist, uint8_t* d_reason_hist);

/* Host copies of the last step's outputs (synchronises the stream).  Any pointer may be NULL.
 * obs: f64[5][n_envs] = [|sigma_BR|, |omega_BN_B|, |Omega|/wheel_limit, charge/3600/power_max,
 * shadow factor] (…Simulator.py:636-638 + leoPowerAttitudeEnvironment.py:107-108);
 * reward f64[n_envs]; done uint8[n_envs]; done_reason uint8[n_envs] bit-or of BSK_DONE_*. */
#define BSK_DONE_LENGTH 0x1
#define BSK_DONE_WHEELS 0x2
#define BSK_DONE_BATTERY 0x4
#define BSK_DONE_ORBIT 0x8
int bsk_get_obs(bsk_handle* h, double* obs, double* reward, uint8_t* done, uint8_t* done_reason);

/* bsk_get_obs + bsk_get_state behind ONE stream synchronisation (the single-env mirror reads both after every step:
 * …Simulator.py:598-619 pulls the same quantities from the message logs).  Any pointer may be NULL. */
int bsk_get_obs_state(bsk_handle* h, double* obs, double* reward, uint8_t* done_reason, double* state);

/* The same read-back with the observation as the row-major f64[n_envs][5] block the kernel writes under BSK_FLAG_OBS_ROWMAJOR (one
 * contiguous copy; the layout a VecEnv hands out as (N, 5, 1): no transposition on the host).  BSK_EINVAL without the flag.  Any
 * pointer may be NULL.  Synchronises. */
int bsk_get_obs_rowmajor(bsk_handle* h, double* obs_n5, double* reward, uint8_t* done_reason);
/* Device pointers of the output buffers (for the RCCL gather / zero-copy hand-off).
 * obs stride (envs per field) is returned in *stride; done_mask is uint64[ceil(n/64)]. */
int bsk_get_obs_device(bsk_handle* h, double** d_obs, double** d_reward, uint64_t** d_done_mask,
                       uint8_t** d_done_reason, int64_t* stride);

/* Device-resident stepping ("so training loops stay on-GPU"; replaces the host read-back of
 * …Simulator.py:598-619 for a policy that lives on the same GPU).
 * bsk_get_stream: the hipStream_t the handle launches on, so that a caller can order its own work against the step
 * kernel with events / stream waits instead of a host synchronisation (or hand its own stream to bsk_create).
 * bsk_get_terminal_obs_device: device pointers of the terminal observations f64[5][stride] and the per-env
 * finished-episode counts int32[stride] of the device-side auto-reset (NULL until a pool is staged).
 * bsk_get_state_device: the state slab f64[n_fields][*stride] itself (read-only for the caller between steps).  ITS stride need not be
 * the observation buffers' (every other [stride] on this page is bsk_get_obs_device's: n_envs rounded up to 256): for batches of
 * 65 536 ... 98 304 spacecraft the slab's rows carry 256 B of padding each.  That is an EMPIRICAL constant - the K = 1 launch measured
 * 2.6 % shorter at 65 536 and 0.5 % at 98 304 with the rows an odd multiple of 256 B apart, nothing either way at 32 768 / 131 072,
 * slightly longer at 4 Mi (profiles/r06/stride_pad.txt); the mechanism is not established - so always take the stride from here. */
/* bsk_get_episode_device (BSK_FLAG_EPISODE_STATS / BSK_FLAG_OBS_ROWMAJOR; pointers are NULL where the flag is off):
 *   ep_return   f64[stride]  return of the running episode, this step's reward included; 0 where a device-side reset fired
 *   term_return f64[stride], term_len int32[stride]: 'r' and 'l' of info['episode'] for the envs whose done byte is set at this
 *               step ('l' = env steps taken before this one, as the reference counts: ...Environment.py:133)
 *   done        u8[stride]   0 / 1 (a torch.bool view needs no kernel)
 *   obs_rowmajor f64[n_envs][5]
 * Every reset leaves the NEW episode's first observation [|sigma_BN|, |omega|, |Omega|/limit, charge/3600/power_max, 1] in the
 * observation buffers of the envs it restarts, so that a device-resident loop never has to compute or upload a reset observation.
 *  - The step kernel's own auto-reset (BSK_FLAG_AUTO_RESET) KEEPS that step's reward, reason and done byte - the finished episode's
 *    last transition is what the step reports - and zeroes only ep_return (the new episode's running return).
 *  - The explicit entry points (bsk_reset, bsk_reset_from_pool, bsk_reset_from_pool_device) ALSO zero reward, reason, done and
 *    ep_return of the envs they restart: a consumer that reads those buffers on the device must have consumed the last step's
 *    values - or be ordered before the reset on the handle's stream - before it calls a masked reset entry point, or the
 *    terminal reward and penalty of the restarted envs are gone (bsk_get_batch_stats* still report the last step's sums: the
 *    snapshot is taken before the zeroing).
 * HIP graphs: the device-resident entry points (bsk_step_device*, bsk_reset_from_pool_device, bsk_get_batch_stats_device) may be
 * captured.  The library notices the capture and from then on evaluates nothing at enqueue time for that handle (batch scalars
 * are re-formed on every request, the bare levels read the battery charge in every launch), so replays stay correct after a later
 * bsk_set_state / bsk_set_ic_pool / bsk_reset; launch GEOMETRY (substeps, kernel form) is what was captured. */
int bsk_get_episode_device(bsk_handle* h, double** d_ep_return, double** d_term_return, int32_t** d_term_len, uint8_t** d_done,
                           double** d_obs_rowmajor);
int bsk_get_stream(bsk_handle* h, void** stream);
int bsk_get_terminal_obs_device(bsk_handle* h, double** d_term_obs, int32_t** d_episodes);
int bsk_get_state_device(bsk_handle* h, double** d_state, int64_t* stride);

/* Batch scalars of the LAST STEP: sum of its rewards and number of done envs, formed in a fixed order (bitwise
 * reproducible: per 64 envs an xor butterfly, the wave sums w = t mod 256 added in ascending order by thread t, a halving tree
 * over the 256 partials) from the reward buffer and the per-wave done ballots by two small launches of their own (a
 * multi-workgroup first level: one sum per 64 envs; a single workgroup joins them) - once, when first asked for, or just before
 * a reset entry point zeroes the restarted envs' rewards (up to 65 536 spacecraft the join is one wave making the same additions).
 * A step does NOT produce them unless bsk_set_step_stats says so: its epilogue carries the done ballot (one 64-bit mask per wave) and
 * no reward reduction.  After a reset entry point the scalars stay the last STEP's until the next step launch - also on a handle whose
 * launches replay from a HIP graph: the reset seals the snapshot on the device (env 0's counter word and episode number, which every
 * step launch changes) and a later request leaves a sealed snapshot alone.  (Synchronises.) */
int bsk_get_batch_stats(bsk_handle* h, double* reward_sum, int64_t* n_done);
/* The same two scalars left ON the device as f64[2] = {sum of rewards, number of done envs}, enqueued on the handle's stream
 * without synchronising: the operand of the one all-reduce a sharded batch needs. */
int bsk_get_batch_stats_device(bsk_handle* h, double** d_stats2);
/* For consumers that ask for the batch scalars after EVERY step (the per-step all-reduce of a sharded batch, a monitor): on != 0
 * makes every step launch (bsk_step*, not bsk_step_n) form the first level - the sum per 64 envs, same butterfly - in its own
 * epilogue, behind its stores, so that a request costs the join launch alone (batches of up to 2 Mi spacecraft; larger ones keep the
 * two-level form, which is as fast there).  Same bits either way.  Default off: a step that nobody asks about pays nothing.  (Takes effect with the next launch; a handle whose launches have been captured into a HIP graph keeps
 * the two-level form - replays step without the host's knowledge.) */
int bsk_set_step_stats(bsk_handle* h, int on);
/* The halves form of the one-sub-step launch (bsk_kernel_info): mode -1 (default) the handle's size window,
 * 0 never, 1 every launch the form is complete for, at any batch size (measurement and tests: the results are the same bits in
 * either form).  Takes effect with the next launch. */
int bsk_set_halves_form(bsk_handle* h, int mode);

/* Full state read-back / injection, host SoA [n_fields][n_envs] (parity tests, reset_init). */
int bsk_n_fields(const bsk_handle* h);
int bsk_get_state(bsk_handle* h, double* state);
int bsk_set_state(bsk_handle* h, const double* state);
/* per-env counters: env steps and RK4 ticks since reset, int32[n_envs] each (may be NULL) */
int bsk_get_counters(bsk_handle* h, int32_t* steps, int32_t* ticks);
/* Restore the per-env counters (checkpoint / resume together with bsk_set_state): steps in 0..2^20-1,
 * ticks >= 0, int32[n_envs] each, both required.  The FSW phase follows as ticks mod fsw_every. */
int bsk_set_counters(bsk_handle* h, const int32_t* steps, const int32_t* ticks);

/* Device-side auto-reset (BSK_FLAG_AUTO_RESET; reference reset semantics,
 * envs/leoPowerAttitudeEnvironment.py:172-191, without the host round trip).  Stage a pool of
 * initial conditions, host SoA [n_fields][n_pool].  When an env finishes, the step kernel itself
 * reloads it from pool slot  ((env_base + env) * 2654435761 + episode * 40503 + 12345) mod 2^32 mod n_pool
 * (episode = that env's count of finished episodes; env_base: bsk_set_env_base, 0 unless the batch is sharded), zeroes its counters, writes the NEW episode's
 * initial observation [|sigma_BN|, |omega|, |Omega|/limit, charge/3600/power_max, 1] to obs and keeps
 * the finished episode's last observation in the terminal-observation buffer. */
int bsk_set_ic_pool(bsk_handle* h, int n_pool, const double* ic_pool);
/* On-device IC sampler: fill the pool with `n_pool` initial conditions drawn on the GPU with the
 * reference's distributions (set_ICs, …Simulator.py:119-193; leo_orbit.py:25-40; sc_attitudes.py:3-13):
 * a = 6 871 km, e~U[0,.05), i~U[-90,90) deg, Omega, omega, f~U[0,360) deg -> elem2rv; sigma~U[0,1)^3;
 * omega~U(+-1e-5)^3 rad/s; L_ext = 2e-4 N(0,1)^3 N m; wheel speeds U(-800,800) RPM; charge U(8,20) W h.
 * Random numbers: Philox4x32-10, key = seed, counter = (slot, draw index): slot k is reproducible
 * on its own.  Needs BSK_FLAG_AUTO_RESET.  bsk_reset_from_pool then (re)starts every env (mask NULL)
 * or the masked envs from the pool with the slot rule above, without any host data. */
int bsk_sample_ic_pool(bsk_handle* h, int n_pool, uint64_t seed);
int bsk_reset_from_pool(bsk_handle* h, const uint8_t* mask);
/* Same with the mask (or NULL) in DEVICE memory, asynchronous on the handle's stream: no host data, no copy, no synchronisation. */
int bsk_reset_from_pool_device(bsk_handle* h, const uint8_t* d_mask);
/* bsk_reset_from_pool_device with a slot rule that the members of a population SHARE (bsk_population_rollout: member m drives envs
 * [m E, (m + 1) E), E = envs_per_member), so that every member of a generation is scored on the same E episodes:
 *     g = (uint32)(env_base + env)           the 32-bit global index of the rule above
 *     q = g mod envs_per_member
 *     e = the low 32 bits of *d_epoch, a DEVICE word the kernel reads when it runs (NULL: e = 0)
 *     slot = (q * 2654435761 + e * 40503 + 12345) mod 2^32 mod n_pool
 * Envs with equal q restart from the same slot, and a new epoch draws anew: with the optimiser's generation word
 * (bsk_es_generation_device) as the epoch a replayed graph moves on by itself.  Everything else is bsk_reset_from_pool_device:
 * counters zeroed, the env's episode count + 1 (auto-resets inside a rollout go on with the per-env rule above), the new episode's
 * first observation written, reward / reason / done / ep_return zeroed, the batch-scalar snapshot before and its seal after; d_mask
 * (DEVICE memory, or NULL for every env) as there.  Enqueue-only on the handle's stream: no copy, no synchronisation; capturable.
 * envs_per_member is any value >= 1 - no multiple of 64, and it need not divide n_envs.  An episode is a deterministic function of
 * its initial condition and the actions, so identical members then score identically under BSK_POLICY_GREEDY; BSK_POLICY_SAMPLE
 * still draws its uniform per GLOBAL env index, so sampled actions differ between members on the same initial condition.
 * BSK_EINVAL before anything is launched: a NULL handle, no pool staged, envs_per_member < 1. */
int bsk_reset_from_pool_shared(bsk_handle* h, int envs_per_member, const uint64_t* d_epoch, const uint8_t* d_mask);
/* Host copy of the staged pool, SoA [n_fields][n_pool] (n_pool as staged; the caller sizes the buffer):
 * lets the host replay a device-side reset (reset_init, leoPowerAttitudeEnvironment.py:202-216). */
int bsk_get_ic_pool(bsk_handle* h, double* ic_pool);
/* terminal observations f64[5][n_envs] (valid for envs whose done flag is set) and per-env
 * finished-episode counts int32[n_envs]; either pointer may be NULL.  Synchronises. */
int bsk_get_terminal_obs(bsk_handle* h, double* term_obs, int32_t* episodes);

/* Sharded batches (one handle per GPU): the GLOBAL index of this handle's env 0.  The device-side
 * reset's slot rule hashes env_base + local index, so a batch split over several handles restarts its envs from
 * exactly the pool slots the unsplit batch would use.  Default 0. */
int bsk_set_env_base(bsk_handle* h, int64_t env_base);

/* Epoch offset [s] added to every spacecraft's own clock (ticks * dt) when the Sun position
 * sun_r0 + sun_v * t is evaluated at the start of an env step (default 0). */
int bsk_set_sim_time(bsk_handle* h, double t_seconds);

/* Forks (branching a batch: tree search, receding-horizon lookahead, population training that copies the best envs over the worst).
 * bsk_fork_device: env j of dst becomes an exact copy of env map[j] of src (map[j] == -1: env j is left as it is).
 * d_map: int32[n_dst] in DEVICE memory.  src may be dst.  Copied per forked env: every field of the state slab, the counter word
 * (steps, ticks and FSW phase), the observation rows, reward, reason and done-mask bit; the row-major observation, ep_return,
 * term_return, term_len, the done byte, terminal observation and episode count where dst has the buffer - from src where src has it
 * too, else zero (the row-major observation is then the same observation taken from src's rows).  NOT copied: env_base - a forked
 * env that later auto-resets restarts from pool_slot(dst's env_base + j, copied episode count), the bsk_set_ic_pool rule.
 *  - Compatibility: BSK_EINVAL unless both handles are on one device, have equal n_rw and byte-identical bsk_configs except for the
 *    flag bits AUTO_RESET, EPISODE_STATS, OBS_ROWMAJOR and LDS_SCRATCH (they change outputs or the kernel form, never the
 *    arithmetic), equal bsk_set_sim_time values and, at BSK_GRAV_SH, equal bsk_set_gravity_sh coefficients.
 *  - A map entry that is neither -1 nor in [0, n_src) is treated as -1 (nothing out of range is read) and raises dst's device error
 *    word: the next synchronising entry point on dst returns BSK_EHIP once.
 *  - Ordering: enqueued on dst's stream, no copy and no synchronisation (capturable into a HIP graph).  When the streams differ,
 *    dst's stream first waits for the work queued on src's stream, and src's stream then waits for the fork, so that later work on
 *    src cannot overwrite rows the fork still reads (under capture, keep both handles on the capturing stream).
 *  - In-handle forks (src == dst; overlapping maps such as permutations allowed): every destination receives its source's values
 *    from before the call.  They gather into a scratch block the first in-handle fork allocates and the handle keeps; that first
 *    call cannot be captured (BSK_EINVAL under capture).
 *  - Afterwards dst behaves as after bsk_set_state (the bare levels read the battery charge again), and bsk_get_batch_stats reports
 *    the sums over its buffers as the fork left them (a reset's seal on the last step's scalars is lifted on the device).
 * bsk_fork: the same with the map in host memory (staged on dst's stream); synchronises dst's stream and reports the device error. */
int bsk_fork_device(bsk_handle* dst, bsk_handle* src, const int32_t* d_map);
int bsk_fork(bsk_handle* dst, bsk_handle* src, const int32_t* map);
/* Choosing among rollouts: n_branch branches in groups of `group` consecutive ones (n_branch a multiple of group), histories
 * d_reward_hist f64[n_steps][n_branch] and d_reason_hist u8[n_steps][n_branch] (bsk_step_n's layout), all in DEVICE memory.
 * Value of branch b:  v = 0, g = 1; for t = 0 .. n_steps-1: v = v + g * reward[t][b]; g = g * gamma; stop after the first t with
 * reason[t][b] != 0 (its reward included) - each operation rounded on its own, no FMA, so a restatement in numpy gives the same bits.
 * Best branch of a group: the greatest value, ties to the lowest index, NaN loses to every number (a group of NaNs picks its first).
 * Outputs: d_values f64[n_branch] (may be NULL), d_best_value f64[n_groups] (may be NULL), d_best_action int32[n_groups] =
 * d_first_action[best branch].  Enqueued on `stream` (a hipStream_t, NULL = the null stream) of the current device; no copy, no
 * synchronisation, capturable. */
int bsk_select_branches(const double* d_reward_hist, const uint8_t* d_reason_hist, const int32_t* d_first_action,
                        int n_steps, int n_branch, int group, double gamma,
                        double* d_values, double* d_best_value, int32_t* d_best_action, void* stream);
/* bsk_select_branches with a value at the leaf (n-step lookahead bootstrapped from a learned value, such as bsk_policy_value's of
 * the branches' last observations).  The loop is bsk_select_branches': v = v + g * reward[t][b]; g = g * gamma, stopping after the
 * first t with reason[t][b] != 0.  Then, ONLY when no step of the branch ended its episode:  v = v + g * (double)d_leaf_value[b],
 * g the factor the loop left (n_steps multiplications by gamma), the product and the sum each rounded on their own, no FMA.  A
 * branch whose episode ended takes no leaf term - also one that ended at the last step, by length for instance: nothing follows
 * an ended episode.  The choice rule is unchanged (greatest value, ties to the lowest index, a NaN loses): a NaN leaf makes the
 * value of a branch that did not end NaN, so it loses.  d_leaf_value: f32[n_branch] in DEVICE memory; it is not read for a branch
 * that ended.  Outputs, ordering and refusals as bsk_select_branches, plus BSK_EINVAL for a NULL d_leaf_value.  With a leaf of
 * zeros every output equals bsk_select_branches' except where v + 0.0 differs from v (v = -0.0). */
int bsk_select_branches_boot(const double* d_reward_hist, const uint8_t* d_reason_hist, const int32_t* d_first_action,
                             int n_steps, int n_branch, int group, double gamma, const float* d_leaf_value,
                             double* d_values, double* d_best_value, int32_t* d_best_action, void* stream);
/* One level of a beam search (BeamPlanner in basilisk_env_amd/planning.py): the `width` best action sequences of every root.
 * Slot s (n_roots * width of them) belongs to root s / width and holds a bsk_beam_slot: `value` the discounted return so far,
 * `first` the sequence's first action, flags bit 0 (BSK_BEAM_VALID) the slot holds a sequence, bit 1 (BSK_BEAM_LIVE) no step of it
 * has ended its episode yet.  Candidate c (3 * width * n_roots of them) is env c of the children handle after one env step:
 * parent slot p = c / 3, action a = c % 3, d_reward f64[] and d_reason u8[] the children's outputs (bsk_get_obs_device).
 *  - level 0 (d_in ignored, may be NULL): c is valid iff p % width == 0 (slot 0 of each root is the one real parent);
 *    value = 0.0 + weight * reward[c], live = reason[c] == 0, first = a.
 *  - level >= 1: c is valid iff p is valid and (p is live or a == 0): a finished sequence continues as ONE candidate, not three.
 *    value = p live ? value[p] + weight * reward[c] : value[p] (product and sum each rounded on their own, no FMA: the order of
 *    bsk_select_branches), live = live[p] && reason[c] == 0, first = first[p].
 *  - an invalid candidate has value NaN, first -1 and no flags.
 *  - order within a root: valid candidates before invalid ones; valid ones by bsk_select_branches' rule (the greater value first,
 *    NaN after every number, equal values to the lower index); invalid ones by index.
 * Outputs: the candidate of rank r < width fills d_out[root * width + r], and d_map[root * width + r] = c when it is valid, -1
 * otherwise (the map of bsk_fork_device that moves the children into the next level's parents); d_best_value[root] and
 * d_best_action[root] are the value and first action of rank 0 (valid whenever the root has a valid candidate, as at level 0
 * and whenever d_in is the previous level's d_out).  `weight` is the level's discount w_t: w_0 = 1, w_t = w_{t-1} * gamma.
 * Without BSK_FLAG_DESAT actions 1 and 2 command the same thing: their children tie exactly and both take a slot.
 * BSK_EINVAL (before any launch): a NULL pointer other than d_in at level 0, width outside 1..BSK_BEAM_MAX_WIDTH, n_roots < 1,
 * 3 * width * n_roots >= 2^31, level < 0, a non-finite weight, d_in == d_out.  d_in and d_out are distinct buffers (the caller
 * double-buffers them).  Enqueued on `stream` (a hipStream_t, NULL = the null stream) of the current device; no copy, no
 * synchronisation, capturable. */
#define BSK_BEAM_MAX_WIDTH 81
#define BSK_BEAM_VALID 1u
#define BSK_BEAM_LIVE 2u
typedef struct bsk_beam_slot {
    double value;
    int32_t first;
    uint32_t flags;
} bsk_beam_slot;
int bsk_beam_select(const double* d_reward, const uint8_t* d_reason, int n_roots, int width, int level, double weight,
                    const bsk_beam_slot* d_in, bsk_beam_slot* d_out, int32_t* d_map, double* d_best_value, int32_t* d_best_action,
                    void* stream);
/* bsk_beam_select that ranks a level by "return so far + value of where the candidate stands".  Every candidate's value, first,
 * flags and validity are exactly bsk_beam_select's.  Its KEY is
 *  - value + boot_weight * (double)d_leaf_value[c] when it is valid and live after this step (the product, then the sum, each
 *    rounded on its own, no FMA);
 *  - value when it is valid but not live (an ended episode has nothing after it);
 *  - NaN when it is invalid.
 * The order within a root is bsk_beam_select's with the key in place of the value: valid before invalid, the greater key first,
 * NaN after every number, equal keys to the lower index.  d_leaf_value: f32[3 * width * n_roots] in DEVICE memory, read for live
 * candidates only (bsk_policy_value of the children's observations).  boot_weight: the discount of the step AFTER this level,
 * w_{t+1} = w_t * gamma; finite.
 * Outputs: d_out[root * width + r] holds the candidate of rank r with its UN-bootstrapped value - the next level continues the
 * true return and the leaf term is never accumulated twice; d_map as bsk_beam_select; d_key[root * width + r] (f64, may be NULL)
 * the key of rank r; d_best_value[root] the key of rank 0 and d_best_action[root] that candidate's first action.
 * Refusals, ordering and capture as bsk_beam_select, plus BSK_EINVAL for a NULL d_leaf_value and a non-finite boot_weight. */
int bsk_beam_select_boot(const double* d_reward, const uint8_t* d_reason, int n_roots, int width, int level, double weight,
                         double boot_weight, const float* d_leaf_value,
                         const bsk_beam_slot* d_in, bsk_beam_slot* d_out, int32_t* d_map, double* d_key,
                         double* d_best_value, int32_t* d_best_action, void* stream);

/* A policy of the library's own: one or two multilayer perceptrons over the five observation rows, evaluated by ONE launch - action
 * (and, optionally, its log-probability, the value and the three logits) out.  An extra beside the reference surface, like forks
 * and planning: the reference's agent (stable-baselines MlpPolicy) runs its network outside the env.
 *  - action network: 5 inputs, n_hidden = 0..3 hidden layers, each 16 ... 128 units wide in multiples of 16, 3 outputs (logits);
 *    optional value network (has_value = 1): the same rules for v_n_hidden / v_hidden, 1 output; one hidden activation per network,
 *    BSK_POLICY_RELU (z > 0 ? z : 0) or BSK_POLICY_TANH.
 *  - `params`, f32: in_scale[5], in_shift[5], then per layer W[out][in] row-major (torch's nn.Linear.weight) and b[out]; the action
 *    network's layers first, then the value network's.  bsk_policy_n_params floats in all.
 * Evaluation per spacecraft, all in f32:
 *  1. x_i = fmaf((float)obs_i, in_scale_i, in_shift_i), obs_i the f64 observation converted round-to-nearest-even;
 *  2. per layer and output j: z_j = b_j, then for k = 0, 1, ... ascending z_j = fmaf(W[j][k], h_k, z_j) - one k-ordered chain of fused
 *     multiply-adds from the bias, one rounding per step, nothing wider inside (no split-K, no pairwise sums);
 *  3. hidden h = act(z); the last layer is linear;
 *  4. BSK_POLICY_GREEDY: the index of the greatest logit, ties to the lowest index, a NaN loses to every number (three NaNs pick 0):
 *     the rule of bsk_select_branches;
 *  5. BSK_POLICY_SAMPLE: m = max logits, e_i = expf(l_i - m), p_i = e_i / ((e_0 + e_1) + e_2), u = (w0 >> 8) * 2^-24 with w0 the first
 *     word of philox4x32_10(counter = (env_lo, env_hi, draw_lo, draw_hi), key = (seed_lo, seed_hi)), env = env_base + j (64 bit),
 *     draw the policy's 64-bit draw counter; action = 0 if u < p_0, else 1 if u < p_0 + p_1, else 2;
 *  6. logp = (l_a - m) - logf((e_0 + e_1) + e_2) of the chosen action a (either mode), value, and the logits.
 * For RELU networks logits and value are therefore reproducible bit for bit by any restatement that makes the same chain
 * (basilisk_env_amd/policy.py does, in numpy).  Non-finite observations are outside the numerical contract; nothing out of range
 * is read or written for them and the action stays in {0, 1, 2}.
 * A policy belongs to one device.  It is not thread-safe and serves ONE stream at a time: its draw counter and its scratch row of
 * actions are single, so two streams' launches would race on them. */
#define BSK_POLICY_RELU 0
#define BSK_POLICY_TANH 1
#define BSK_POLICY_GREEDY 0
#define BSK_POLICY_SAMPLE 1
typedef struct bsk_policy_spec {
    uint32_t abi_version; /* = BSK_ABI_VERSION */
    uint32_t struct_size; /* = sizeof(bsk_policy_spec) */
    int32_t n_hidden;     /* action network: hidden layers, 0..3 */
    int32_t hidden[3];
    int32_t activation;
    int32_t has_value;    /* 0 / 1 */
    int32_t v_n_hidden;   /* value network (ignored without has_value) */
    int32_t v_hidden[3];
    int32_t v_activation;
} bsk_policy_spec;
typedef struct bsk_policy bsk_policy;
/* Floats in `params` for this spec, or BSK_EINVAL / BSK_EABI. */
int bsk_policy_n_params(const bsk_policy_spec* spec);
/* `params`: host pointer, copied.  seed = 0, draw = 0.  BSK_ENODEV when no gfx950 device is usable (the spec is checked first). */
int bsk_policy_create(const bsk_policy_spec* spec, const float* params, int device_id, bsk_policy** out);
/* New parameters (host pointer), ordered after everything queued on the policy's device (a policy keeps no stream of its own).
 * Synchronises the device. */
int bsk_policy_set_params(bsk_policy* p, const float* params);
void bsk_policy_destroy(bsk_policy* p);
/* Seed and draw counter of sample mode.  A sample-mode launch reads the counter on the device and a one-thread launch behind it adds
 * one, so that a launch captured into a HIP graph draws new numbers on every replay; greedy launches leave it alone.  Both entry
 * points are ordered after everything queued on the policy's device and synchronise it. */
int bsk_policy_set_rng(bsk_policy* p, uint64_t seed, uint64_t draw);
int bsk_policy_get_rng(bsk_policy* p, uint64_t* seed, uint64_t* draw);
/* Evaluate the policy for n spacecraft.  Raw DEVICE pointers, like bsk_select_branches: enqueued on `stream` (a hipStream_t, NULL =
 * the null stream) of the policy's device; no copy, no synchronisation, capturable.
 *   d_obs     f64[5][obs_stride], obs_stride >= n: the layout of bsk_get_obs_device (no row-major copy needed)
 *   env_base  >= 0: global index of spacecraft 0 (sample mode's counter; what bsk_set_env_base gives a sharded handle)
 *   d_action  int32[n] in {0, 1, 2}: what bsk_step_device reads in place
 *   d_logp    f32[n] or NULL;  d_value f32[n] or NULL (non-NULL without a value network: BSK_EINVAL)
 *   d_logits  f32[3][out_stride] or NULL (out_stride >= n)
 * Every argument is checked before anything is launched. */
int bsk_policy_act(bsk_policy* p, const double* d_obs, int64_t obs_stride, int n, int64_t env_base, int mode,
                   int32_t* d_action, float* d_logp, float* d_value, float* d_logits, int64_t out_stride, void* stream);
/* The value network alone, ONE launch: steps 1 - 3 of the evaluation above applied to the value network only -
 * x_i = fmaf((float)obs_i, in_scale_i, in_shift_i), every unit one k-ascending fmaf chain from its bias, d_value[j] the single
 * output - so that d_value equals, bit for bit and for both activations, what bsk_policy_act writes into its d_value for the same
 * columns.  What a planner reads at its leaves (bsk_select_branches_boot, bsk_beam_select_boot).
 *   d_obs     f64[5][obs_stride], obs_stride >= n, as bsk_policy_act
 *   d_value   f32[n]; nothing beyond d_value[n - 1] is written and no column beyond n - 1 is read
 * No action network is evaluated.  The launch touches NEITHER the policy's draw counter NOR its scratch row of actions - the two
 * things that make a policy single-stream - and reads only the parameters: it may run on any stream beside the policy's other
 * launches (bsk_policy_set_params still waits for it, like for every launch on the device).  Enqueued on `stream` of the policy's
 * device: no copy, no synchronisation, no allocation; capturable from the first call.
 * BSK_EINVAL (before any launch): a NULL p, d_obs or d_value, n outside 1 .. 2^28, obs_stride < n, a policy without a value
 * network. */
int bsk_policy_value(bsk_policy* p, const double* d_obs, int64_t obs_stride, int n, float* d_value, void* stream);
/* Closed-loop rollout: per env step t = 0 .. n_steps-1, (a) the policy on the handle's own observation buffers with the handle's
 * env_base - actions into row t of d_action_hist (int32[n_steps][n_envs]; a scratch row of the policy when NULL), log-probability and
 * value into row t of d_logp_hist / d_value_hist (f32[n_steps][n_envs], may be NULL): they belong to the observation the action was
 * chosen FROM; (b) bsk_step_device with those actions; (c) row t of bsk_step_n's histories (each may be NULL).  All DEVICE memory,
 * enqueued on the handle's stream: no copy, no synchronisation, capturable once the policy's scratch row exists (a first call that
 * must allocate it returns BSK_EINVAL under capture: the rule of in-handle forks).  Afterwards every buffer of the handle holds, bit
 * for bit, what n_steps rounds of bsk_policy_act + bsk_step_device leave, and the draw counter has advanced by n_steps in sample
 * mode.  Works at every level and with the harmonics; with BSK_FLAG_AUTO_RESET episodes restart inside the rollout as in bsk_step_n.
 * BSK_EINVAL when policy and handle live on different devices. */
int bsk_policy_rollout(bsk_policy* p, bsk_handle* h, int mode, int substeps, int n_steps,
                       double* d_obs_hist, double* d_reward_hist, uint8_t* d_reason_hist,
                       int32_t* d_action_hist, float* d_logp_hist, float* d_value_hist);

/* A population of policies: n_members parameter sets of ONE spec on the device, evaluated side by side - what forks were made for
 * ("population training"): evolution strategies, CEM, population-based training.  The library has no autograd; gradient-free
 * search over the parameters is one of the two ways a policy is trained on it (the other: a supervised fit, bsk_fit_* below).
 * Member <-> env rule: with envs_per_member = E, spacecraft j belongs to member j / E - member m drives the envs [m * E, (m + 1) * E)
 * of one handle (or the columns of one observation block).  E is a multiple of 64 and n = n_members * E exactly: a group of 64
 * spacecraft never straddles two members.
 * Evaluation is the policy's, steps 1-6 above, with member j / E's parameter block (its own in_scale / in_shift included) in place
 * of the single one; the same code evaluates both, so bsk_population_act equals, bit for bit and for either activation, n_members
 * calls of bsk_policy_act with member m's parameters on columns [m * E, (m + 1) * E) and env_base + m * E.  One draw counter serves
 * the population: sample mode reads philox at counter (env_base + j, draw) and one launch advances draw by one.
 * Parameter blocks are in the C-ABI layout of bsk_policy_create, bsk_policy_n_params(spec) floats per member, member after member.
 * Fitness (bsk_population_rollout), per env - the value rule of bsk_select_branches, accumulated step by step with no
 * [n_steps][n] history: v = 0, g = 1, len = 0, alive; after each env step t, while alive:
 *     v = v + g * reward  (product and sum each rounded on their own, no FMA);  len += 1;  g = g * gamma;
 *     the env stops being alive after the first step with reason != 0 (that step's reward is included).
 *   With BSK_FLAG_AUTO_RESET the env restarts and goes on stepping; its later episodes do not count.
 * Per member, in f64 and in this order (numpy repeats it: basilisk_env_amd/policy.py population_fitness_ref):
 *     s[l] = v[m*E + l], then s[l] = s[l] + v[m*E + l + 64*i] for i = 1, 2, ... ascending      (l = 0 .. 63)
 *     for stride = 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l + stride] for l < stride
 *     fitness[m] = s[0] / E
 *   and mean_len[m] the same over (double)len.  No atomics: the result does not depend on the launch shape.
 * A population belongs to one device, is not thread-safe and serves ONE stream at a time (its draw counter, running values and
 * scratch row of actions are single). */
typedef struct bsk_population bsk_population;
/* `params`: host pointer to n_members blocks, copied; NULL: every member all-zero.  seed = 0, draw = 0.  Checked in this order:
 * the spec (BSK_EINVAL / BSK_EABI), n_members in 1..2^22 (BSK_EINVAL), then the device (BSK_ENODEV when no gfx950 device is
 * usable). */
int bsk_population_create(const bsk_policy_spec* spec, int n_members, const float* params, int device_id, bsk_population** out);
void bsk_population_destroy(bsk_population* pop);
/* As bsk_policy_set_rng / bsk_policy_get_rng: ordered after everything queued on the population's device, and synchronise it. */
int bsk_population_set_rng(bsk_population* pop, uint64_t seed, uint64_t draw);
int bsk_population_get_rng(bsk_population* pop, uint64_t* seed, uint64_t* draw);
/* New parameters for ALL members from a host pointer (n_members blocks).  Ordered after everything queued on the population's
 * device; synchronises it. */
int bsk_population_set_params(bsk_population* pop, const float* params);
/* New parameters for the members first .. first + count - 1 from DEVICE memory (d_params: count blocks): one launch on `stream` (a
 * hipStream_t, NULL = the null stream) repacks them into the device's layout - the same bits bsk_population_set_params leaves -
 * with no copy and no synchronisation; capturable.  Other members keep theirs.  The caller orders it against launches that read
 * the population (the same stream does).  BSK_EINVAL: NULL pointers, first < 0, count < 1, first + count > n_members. */
int bsk_population_set_params_device(bsk_population* pop, const float* d_params, int first, int count, void* stream);
/* Member `member`'s parameters in the C-ABI layout (host pointer, bsk_policy_n_params floats): the block bsk_policy_create takes.
 * Synchronises the device.  BSK_EINVAL for a member outside 0..n_members-1. */
int bsk_population_get_member(bsk_population* pop, int member, float* params);
/* bsk_policy_act with the member rule: arguments, layouts and checks as there, plus envs_per_member.  BSK_EINVAL (before anything
 * is launched) also when envs_per_member is not a positive multiple of 64 or n != n_members * envs_per_member. */
int bsk_population_act(bsk_population* pop, const double* d_obs, int64_t obs_stride, int n, int envs_per_member, int64_t env_base,
                       int mode, int32_t* d_action, float* d_logp, float* d_value, float* d_logits, int64_t out_stride, void* stream);
/* One generation: bsk_policy_rollout under the member rule, envs_per_member = n_envs / n_members, with the fitness formed on the
 * device.  Per env step ONE policy launch serves all members, then bsk_step_device, then one launch that writes row t of the
 * histories (the six pointers of bsk_policy_rollout, each may be NULL) and advances every env's value; behind the last step one
 * launch writes
 *   d_env_value f64[n_envs], d_env_len int32[n_envs]: v and len of every env;  d_fitness f64[n_members], d_mean_len f64[n_members]
 * (each may be NULL).  The handle's buffers end as n_members separate bsk_policy_rollout calls on handles of E envs with env_base
 * + m * E would leave them, bit for bit.  All DEVICE memory, enqueued on the handle's stream: no copy, no synchronisation,
 * capturable once the population's scratch rows fit the handle (a first call of a size must allocate them and returns BSK_EINVAL
 * under capture).  Uses the handle's env_base; works at every level, with the harmonics and with BSK_FLAG_AUTO_RESET.
 * BSK_EINVAL before anything is launched: a NULL population or handle, substeps or n_steps < 1, a bad mode, n_envs not
 * n_members * E with E a positive multiple of 64, d_value_hist without a value network, population and handle on different
 * devices, a non-finite gamma, and bsk_step_n's preconditions (harmonics not set, auto-reset without a pool). */
int bsk_population_rollout(bsk_population* pop, bsk_handle* h, int mode, int substeps, int n_steps, double gamma,
                           double* d_obs_hist, double* d_reward_hist, uint8_t* d_reason_hist,
                           int32_t* d_action_hist, float* d_logp_hist, float* d_value_hist,
                           double* d_env_value, int32_t* d_env_len, double* d_fitness, double* d_mean_len);

/* Episode outcomes: how the episodes that count towards the fitness ended and which actions they used, per member - what a fitness
 * value cannot say ("the batteries run flat" against "every episode reaches the length limit").  The reason byte and the action row
 * of an env step exist for one launch; the summary is formed where the fitness is formed, with no [n_steps][n_envs] history and no
 * host.  Off by default: a population that never calls bsk_population_set_outcomes launches the kernels of the definition above
 * with the arguments it passed before.  With rows attached every later bsk_population_rollout
 *   - takes the launch with the value rule at every env step, whether a fitness output was asked for or not (an attached
 *     bsk_obs_stats object then counts by the alive bytes, as under a rollout that forms fitness), and in that same launch, for
 *     every env that is alive BEFORE step t (its first episode has not ended: the `alive` of the value rule), with a_t the action
 *     the policy launch of step t wrote (0, 1 or 2) and q_t the step's reason byte:
 *         act_n[a_t] = act_n[a_t] + 1;      if q_t != 0: end_reason = q_t
 *     act_n int32[3] and end_reason uint8 per env, both zero at step 0.  An env still alive behind the last step keeps
 *     end_reason == 0; under BSK_FLAG_AUTO_RESET later episodes are not counted, exactly as in the fitness;
 *   - behind the last step, next to the launch that writes the fitness, issues one launch of one wave per member that writes
 *     d_rows[m][0 .. BSK_OUTCOME_COLS - 1] over member m's envs e = 0 .. E - 1 (v_e = the env's value, what d_env_value holds):
 *         col 0 .. 3   the number of envs whose end_reason has BSK_DONE_LENGTH, _WHEELS, _BATTERY, _ORBIT set (a byte with two bits
 *                      set counts in both)
 *         col 4        the number of envs with end_reason == 0: unfinished when the rollout ended
 *         col 5 .. 7   the sum of act_n[0], act_n[1], act_n[2]: steps taken under each action while alive; 5 + 6 + 7 is the
 *                      member's sum of d_env_len
 *         col 8        the sum of x_e = v_e * v_e, each product rounded on its own, in the order of the fitness:
 *                        s[l] = x_l;  s[l] = s[l] + x_(l+64c) for c = 1, 2, ... ascending while l + 64c < E        (l = 0 .. 63)
 *                        for stride = 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l + stride] for l < stride;   col 8 = s[0]
 *         col 9, 10    the minimum and the maximum of v_e in the same order, under the rule "candidate x replaces incumbent m when
 *                      x < m (max: x > m) or m is a NaN":  m[l] = v_l;  then x = v_(l+64c) ascending;  then for stride = 32 ... 1
 *                      and l < stride the candidate m[l + stride] against the incumbent m[l];  the result is m[0].  All-NaN
 *                      gives a NaN; -0.0 and +0.0 compare equal, so which of the two is reported follows from the order.
 *     Counts are summed as integers and converted to f64 once: exact and independent of any order.  f64 * and + only, no FMA, no
 *     atomics, no dependence on the launch shape (basilisk_env_amd/policy_ref.py: population_outcomes_ref repeats it bit for bit).
 * The accumulators are allocated like the population's scratch rows: by the first rollout of a size that has rows attached, which
 * returns BSK_EINVAL under capture.  Fitness, histories and every buffer of the handle are what the same rollout leaves without
 * rows attached, bit for bit.
 * bsk_population_set_outcomes: d_rows is DEVICE memory, f64[n_members][BSK_OUTCOME_COLS], on the population's device (the rollout
 * checks the handle against that device, like everything else, before anything is launched); it stays attached and is the caller's
 * to keep alive.  NULL detaches.  No launch, no copy, no synchronisation.  BSK_EINVAL for a NULL population. */
#define BSK_OUTCOME_COLS 11
int bsk_population_set_outcomes(bsk_population* pop, double* d_rows);

/* An evolution strategy on the device: antithetic Gaussian perturbations with centred-rank utilities (Salimans et al. 2017), the
 * optimiser a population was given bsk_population_set_params_device for - its candidates never leave the device and its noise is
 * never stored: ask and tell regenerate it from (seed, generation, pair, parameter).  Reset, ask, rollout and tell are one stream
 * of launches, so a captured graph replays generation after generation with no host in the loop.
 * An optimiser holds theta f64[n_params] (the C-ABI parameter layout of bsk_policy_create), sigma > 0, lr, frozen (the first
 * `frozen` floats are never perturbed nor moved; 10 covers in_scale and in_shift), an even n_members = P, a 64-bit seed and a
 * 64-bit generation counter g kept in device words like the policy's {seed, draw}.
 * Noise z(g, i, j) of generation g, pair i = 0 .. P/2 - 1, parameter j: ONE Philox4x32-10 call under the key (seed low word, seed
 * high word) at the counter (j, i, g low word, g high word).  From its words w0, w1: k = (w0 >> 6) * 2^26 + (w1 >> 6), a 52-bit
 * integer; u = (k + 0.5) * 2^-52, exact and inside (0, 1); z = the inverse normal CDF of u in f64 + - * /, sqrt and integer
 * operations only, each rounded on its own (no FMA, no library log / exp), so that numpy repeats it bit for bit
 * (basilisk_env_amd/policy.py: es_noise_ref).  It is Wichura's AS 241 (PPND16) with a series logarithm; |z| <= 8.2096:
 *     q = u - 0.5
 *     |q| <= 0.425:  r = 0.180625 - q*q;  z = q * A(r) / B(r)
 *     else:  p = (q < 0) ? u : 1 - u  (exact);  r = sqrt(-ln(p));
 *            z = (r <= 5) ? C(r - 1.6) / D(r - 1.6) : E(r - 5) / F(r - 5);  z = (q < 0) ? -z : z
 *     ln(p): p = m * 2^e, m in [0.5, 1) (frexp); if m < 0.7071067811865476: m = 2m, e = e - 1
 *            s = (m - 1) / (m + 1); s2 = s*s; t = 1/23; for k = 10 .. 0: t = t*s2 + 1/(2k+1)   (the constants rounded to f64)
 *            ln(p) = e * 0.6931471805599453 + (2 * s) * t
 *     A .. F: degree 7, Horner from the highest coefficient (X = X*x + coef); AS 241's coefficients, lowest first:
 *     A: 3.3871328727963666080, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
 *        4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3
 *     B: 1, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3,
 *        2.1213794301586595867e4, 3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3
 *     C: 1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
 *        1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4
 *     D: 1, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1,
 *        1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9
 *     E: 6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
 *        2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7
 *     F: 1, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
 *        7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15
 * ask: member 2i is (float)(theta_j + sigma * z(g,i,j)), member 2i + 1 is (float)(theta_j - sigma * z(g,i,j)); for j < frozen both
 *   are (float)theta_j.  Product and sum each round in f64, the conversion rounds to nearest even.  Written straight into the
 *   population's device layout (its padding as zeros), every float exactly once.
 * tell, given fitness f64[P] in device memory (greater is better):
 *   1. rank_k = the number of members that beat member k under the rule of bsk_select_branches: the greater value wins, a NaN is
 *      below every number, ties (and NaNs) go to the lower index.
 *   2. u_k = 0.5 - (double)rank_k / max(P - 1, 1)  (basilisk_env_amd/policy.py: centred_ranks);  w_i = u_2i - u_2i+1.
 *   3. for every j >= frozen, in the fitness tree's order:
 *        s[l] = w_l * z(g,l,j), or +0.0 when l >= P/2                                  (l = 0 .. 63)
 *        s[l] = s[l] + w_(l+64m) * z(g, l+64m, j) for m = 1, 2, ... ascending while l + 64m < P/2
 *        for stride = 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l + stride] for l < stride
 *        theta_j = theta_j + c * s[0],  c = lr / ((double)P * sigma) formed once on the host
 *      No atomics: the result does not depend on the launch shape (policy.py: es_tell_ref repeats it bit for bit).
 *   4. behind the update a one-thread launch makes generation = generation + 1, so a captured graph advances on every replay.
 *   tell does not require that ask ran: it uses generation g's noise either way, and the caller orders the two.
 * An optimiser belongs to one device, is not thread-safe and serves ONE stream at a time (its scratch is single). */
typedef struct bsk_es bsk_es;
/* `theta`: host pointer to bsk_policy_n_params(spec) floats, copied (as doubles); NULL: zeros.  generation = 0.  All device scratch
 * is allocated here.  Checked in this order: the spec (BSK_EINVAL / BSK_EABI); BSK_EINVAL for n_members odd, below 2 or above
 * 65536 (the ranking compares every pair of members), sigma not finite or not positive, lr not finite, frozen outside
 * 0..n_params; then the device (BSK_ENODEV when no gfx950 device is usable). */
int bsk_es_create(const bsk_policy_spec* spec, int n_members, const float* theta, double sigma, double lr, int frozen, uint64_t seed,
                  int device_id, bsk_es** out);
void bsk_es_destroy(bsk_es* es);
/* This generation's members into ALL members of `pop`: one launch on `stream` (a hipStream_t, NULL = the null stream), no copy, no
 * synchronisation; capturable.  The caller orders it against launches that read the population (the same stream does).
 * BSK_EINVAL before anything is launched: NULL pointers, a population with a different n_members or a different spec, or one on
 * a different device. */
int bsk_es_ask(bsk_es* es, bsk_population* pop, void* stream);
/* Ranks d_fitness (DEVICE memory, f64[n_members]: what bsk_population_rollout's d_fitness holds), moves theta and advances the
 * generation: three launches on `stream` (two more with a log, bsk_es_set_log, and two more under bsk_es_set_validation), no copy,
 * no synchronisation; capturable.  BSK_EINVAL for NULL pointers. */
int bsk_es_tell(bsk_es* es, const double* d_fitness, void* stream);
/* theta (host pointer, f64[n_params], or NULL) and the generation counter (or NULL).  Ordered after everything queued on the
 * optimiser's device; synchronises it. */
int bsk_es_get_state(bsk_es* es, double* theta, uint64_t* generation);
/* A new theta (host pointer, f64[n_params]; NULL: keep) and generation counter.  Synchronises the device. */
int bsk_es_set_state(bsk_es* es, const double* theta, uint64_t generation);

/* The generation counter as a DEVICE word (read-only for the caller; valid for the optimiser's lifetime): the epoch of
 * bsk_reset_from_pool_shared.  No launch, no copy, no synchronisation.  BSK_EINVAL for NULL pointers. */
int bsk_es_generation_device(bsk_es* es, const uint64_t** d_generation);

/* The update rule of bsk_es_tell.  BSK_ES_SGD (the default) is step 3 above.  BSK_ES_ADAM drives the same estimate through Adam
 * (Kingma & Ba 2015) with an L2 penalty, as the reference implementation of Salimans et al. 2017 does.  Every operation is rounded
 * on its own in f64, no FMA; / and sqrt are the plain correctly rounded ones, as in the inverse normal CDF above
 * (basilisk_env_amd/policy.py: es_tell_adam_ref repeats it bit for bit).  Steps 1 - 3 are unchanged up to s[0] (the same ranking
 * kernel, the same lane-strided sum and tree: ONE device function behind both update kernels).  State: m, v f64[n_params] and two
 * device words beta_pow = {beta1^t, beta2^t} after t tells.  Constants formed once on the host:
 * cg = 1.0 / ((double)P * sigma), a1 = 1.0 - beta1, a2 = 1.0 - beta2.  For every j >= frozen:
 *     p1 = beta_pow[0] * beta1          p2 = beta_pow[1] * beta2
 *     g  = cg * s[0] - weight_decay * theta_j
 *     m_j = beta1 * m_j + a1 * g
 *     v_j = beta2 * v_j + (a2 * g) * g
 *     theta_j = theta_j + (lr * (m_j / (1.0 - p1))) / (sqrt(v_j / (1.0 - p2)) + eps)
 * (greater fitness is better: g is an ascent direction and the penalty pulls theta towards zero).  Behind the update the one-thread
 * launch of step 4 stores beta_pow[0] = beta_pow[0] * beta1, beta_pow[1] = beta_pow[1] * beta2 and generation + 1.  tell stays three
 * launches, no copy, no synchronisation, capturable.  Frozen parameters have no moments that move: their m and v stay 0.
 * bsk_es_set_optimizer synchronises the device; on the first selection of Adam it allocates m, v and beta_pow, on EVERY selection of
 * Adam it zeroes m and v and sets beta_pow = {1.0, 1.0}; theta and the generation are left alone.  BSK_ES_SGD ignores the other
 * arguments and restores step 3 (the moments are kept allocated, unused).  BSK_EINVAL before anything is launched: a NULL
 * optimiser, an unknown kind; for Adam beta1 or beta2 outside [0, 1), eps not finite or <= 0, weight_decay not finite or < 0. */
#define BSK_ES_SGD 0
#define BSK_ES_ADAM 1
int bsk_es_set_optimizer(bsk_es* es, int kind, double beta1, double beta2, double eps, double weight_decay);
/* The moments to / from host memory: m, v f64[n_params], beta_pow f64[2]; each may be NULL (get: not asked for; set: keep).
 * Synchronise the device.  BSK_EINVAL for a NULL optimiser and while the optimiser is BSK_ES_SGD. */
int bsk_es_get_moments(bsk_es* es, double* m, double* v, double* beta_pow);
int bsk_es_set_moments(bsk_es* es, const double* m, const double* v, const double* beta_pow);

/* A step size per parameter, adapted on the device: PGPE's symmetric-sampling rule (Sehnke et al. 2010) on the centred-rank
 * utilities, from the same pairs that move theta.  Off by default (BSK_ES_SIGMA_FIXED): an optimiser that never selects
 * BSK_ES_SIGMA_PGPE launches the kernels of the definition above with the arguments it passed before.  Under either update rule;
 * + - * / only, every operation rounded on its own in f64 with plain /, no FMA (basilisk_env_amd/policy_ref.py: es_ask_sigma_ref
 * and es_tell_pgpe_ref repeat it bit for bit).
 * State: sigma_vec f64[n_params] in device memory, allocated at the first selection of BSK_ES_SIGMA_PGPE and on EVERY selection
 * filled with the sigma of bsk_es_create (as Adam's moments are zeroed on every selection).  Entries j < frozen are carried, but
 * never read by a kernel and never moved.  Being device state, sigma_vec moves on by itself under a replayed graph.
 * ask: member 2i is (float)(theta_j + sigma_vec[j] * z(g,i,j)), member 2i + 1 the same with -; product and sum each round in f64;
 *   j < frozen as above.
 * tell, steps 1 and 2: rank_k and u_k as above; w_i = u_2i - u_2i+1 as above and in addition q_i = u_2i + u_2i+1.
 * tell, step 3, for every j >= frozen, z = z(g,i,j) from ONE evaluation, two sums, each in the order of step 3 above (lane l takes
 *   its pairs l, l + 64, ... ascending from the first, +0.0 with none; then the tree with strides 32 ... 1):
 *        s[0] over w_i * z                       r[0] over q_i * (z * z - 1.0)
 *   With sg = sigma_vec[j] as it was before this tell and Pd = (double)P:
 *        BSK_ES_SGD:   theta_j = theta_j + (lr / (Pd * sg)) * s[0]
 *        BSK_ES_ADAM:  the rule of bsk_es_set_optimizer with cg = 1.0 / (Pd * sg), formed per parameter
 *        sigma:        d = (cs * r[0]) * sg,  cs = lr_sigma / Pd formed once on the host
 *                      lim = max_change * sg
 *                      d = d > lim ? lim : (d < -lim ? -lim : d)
 *                      n = sg + d
 *                      n = n < sigma_min ? sigma_min : n
 *                      n = n > sigma_max ? sigma_max : n
 *                      sigma_vec[j] = n
 *   r[0] is finite by construction: the utilities and z are finite.
 * Step 4 is unchanged; tell stays three launches, no copy, no synchronisation, capturable.
 * Consequences.  A uniform sigma_vec with lr_sigma = 0 gives the optimiser of BSK_ES_SIGMA_FIXED bit for bit under both update
 * rules (d = +-0, sg + d = sg).  At P = 2, q_0 = 0 always: sigma never moves.  Under a fitness that is linear in the parameters
 * and has no ties the two members of a pair mirror each other in the ranking (rank_2i + rank_2i+1 = P - 1), every q_i is exactly 0
 * and sigma keeps its bits; two pairs whose fitness differs by less than the rounding of the members to float count as tied here.
 * |d| <= max_change * sg before the bounds apply, so max_change < 1 keeps sigma positive.
 * bsk_es_set_sigma_adaptation synchronises the device.  BSK_ES_SIGMA_FIXED ignores the other arguments and restores the one sigma
 * of bsk_es_create (the vector stays allocated, unused).  Theta, the generation and the Adam state are left alone; bsk_es_set_optimizer
 * and bsk_es_set_state leave sigma_vec alone.  BSK_EINVAL before anything is launched: a NULL optimiser, an unknown kind; for PGPE
 * lr_sigma not finite or < 0, max_change not finite or outside (0, 1), sigma_min not finite or <= 0, sigma_max not finite or
 * < sigma_min, the sigma of bsk_es_create outside [sigma_min, sigma_max]. */
#define BSK_ES_SIGMA_FIXED 0
#define BSK_ES_SIGMA_PGPE 1
int bsk_es_set_sigma_adaptation(bsk_es* es, int kind, double lr_sigma, double max_change, double sigma_min, double sigma_max);
/* sigma_vec to / from host memory, f64[n_params] (for checkpoints).  Synchronise the device.  BSK_EINVAL for NULL pointers and while
 * the kind is BSK_ES_SIGMA_FIXED; set also for any entry that is not finite and positive (nothing is written then). */
int bsk_es_get_sigma(bsk_es* es, double* sigma);
int bsk_es_set_sigma(bsk_es* es, const double* sigma);

/* A training log and the best member so far, kept on the device: what a replayed graph of reset, ask, rollout and tell leaves for
 * the user besides theta - how every generation scored, and the candidate that scored best.  Both are small reductions over what
 * lies in device memory when tell runs: the P fitness values, and theta, sigma and the generation word, from which ask's members
 * are regenerated exactly.  Off by default: an optimiser that never calls bsk_es_set_log launches the kernels of the definitions
 * above with the arguments it passed before.  f64 + and * only, every operation rounded on its own, no FMA, no atomics
 * (basilisk_env_amd/policy_ref.py: es_log_row_ref and es_best_ref repeat it bit for bit).
 * State of a log of capacity C >= 1, all in device memory:
 *     log_gen uint64[C], all ones after enabling;   log_row f64[C][8], zeros after enabling;
 *     the champion: best_params f32[n_params] in the C-ABI parameter layout (zeros), best_fitness f64 (the NaN 0x7FF8000000000000),
 *                   best_generation uint64 (all ones), best_member int32 (-1);
 *     two candidate words {take, b} that the two kernels below use between them.
 * With a log on, bsk_es_tell issues two more launches IN FRONT of the update, so that theta, sigma_vec and the
 * generation word are still the ones ask used: five launches, still no copy, no synchronisation, capturable.
 * The first launch is one wave.  g = the generation word as read, slot = g mod C (of the whole 64-bit word), f = the P values:
 *   order: the rule of step 1 above - the greater value wins, a NaN is below every number, ties (and NaNs) go to the lower index; with
 *     the index it is a strict total order, so -0.0 against +0.0 is decided by the index and no result depends on the order in
 *     which the lanes join.  b = the member that nobody beats;  wst = among the members that are not NaN the one that beats no
 *     other of them, -1 when every member is NaN.
 *   sums, each in the library's one order: x_k = f_k, or +0.0 where f_k is NaN;
 *        s[l] = x_l, or +0.0 when l >= P                                              (l = 0 .. 63)
 *        s[l] = s[l] + x_(l+64m) for m = 1, 2, ... ascending while l + 64m < P
 *        for stride = 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l + stride] for l < stride
 *     S1 = s[0] over x_k;  S2 the same over x_k * x_k;  cnt = the number of members that are not NaN (an integer);
 *     L1 the same over mean_len[k] when d_mean_len is bound, +0.0 otherwise.  (+inf and -inf among the values make S1 a NaN: which
 *     NaN is not defined.)
 *   row:  log_row[slot] = {f[b], wst >= 0 ? f[wst] : the NaN 0x7FF8000000000000, S1, S2, (double)cnt, (double)b, L1,
 *                          bound ? mean_len[b] : 0.0};   log_gen[slot] = g.
 *     Means and variances are the reader's division: the device stores sums.
 *   champion:  take = f[b] is not NaN and (best_fitness is NaN or f[b] > best_fitness) - a tie keeps the older champion, a
 *     generation of NaNs never takes;  when take: best_fitness = f[b], best_generation = g, best_member = b;  always: the
 *     candidate words = {take, b}.
 * The second launch has one thread per parameter j and does nothing unless take; otherwise best_params[j] is exactly the float ask
 * writes for member b of generation g: (float)theta_j for j < frozen, else (float)(theta_j + s_j * z(g, b >> 1, j)) for an even
 * b and (float)(theta_j - s_j * z(g, b >> 1, j)) for an odd one, s_j = sigma, or sigma_vec[j] under BSK_ES_SIGMA_PGPE; product and
 * sum each round in f64 (one text behind this kernel and ask).  The kernel boundary orders the two launches: no atomics, no fence,
 * as the policy's draw counter is ordered.
 * The champion is "what ask would write now": it is the member that was evaluated as long as the caller moves neither theta nor
 * sigma between ask and tell.  A loop of reset, ask, rollout, tell and bsk_es_apply_obs_norm does not: the normalisation is written
 * BEHIND tell.
 * bsk_es_set_log: capacity > 0 allocates (or frees and allocates again) and sets everything above to its initial value;
 * d_mean_len is DEVICE memory, f64[n_members], or NULL - what bsk_population_rollout's d_mean_len writes; it stays bound and is
 * the caller's to keep alive.  capacity == 0 turns the log off and frees it.  Synchronises the device.  Theta, the generation,
 * Adam's state and sigma_vec are left alone; bsk_es_set_state, bsk_es_set_optimizer and bsk_es_set_sigma_adaptation leave the log
 * and the champion alone.  BSK_EINVAL: a NULL optimiser, a negative capacity, and while the stream of the optimiser's last ask /
 * tell / bsk_es_apply_obs_norm is being captured (nothing is changed then, and the capture stays valid). */
int bsk_es_set_log(bsk_es* es, int capacity, const double* d_mean_len);
/* The whole ring to host memory: gen uint64[C], rows f64[C][8] (either may be NULL); a slot whose log_gen is all ones has never
 * been written.  Synchronises the device.  BSK_EINVAL for a NULL optimiser and with no log. */
int bsk_es_get_log(bsk_es* es, uint64_t* gen, double* rows);
/* The champion to / from host memory: params f32[n_params], fitness, generation, member; each may be NULL (get: not asked for;
 * set: keep).  For a checkpoint that resumes bit for bit, like bsk_es_get_moments.  Synchronise the device.  BSK_EINVAL for a NULL
 * optimiser and with no log. */
int bsk_es_get_best(bsk_es* es, float* params, double* fitness, uint64_t* generation, int32_t* member);
int bsk_es_set_best(bsk_es* es, const float* params, const double* fitness, const uint64_t* generation, const int32_t* member);
/* best_params as a DEVICE pointer (read-only for the caller; valid until the next bsk_es_set_log or bsk_es_destroy): what
 * bsk_population_set_params_device takes, so the champion is loaded into a policy's member with no host in between.  No launch, no
 * copy, no synchronisation.  BSK_EINVAL for NULL pointers and with no log. */
int bsk_es_best_device(bsk_es* es, const float** d_params);

/* Validation on fixed episodes, inside each generation: how good the CENTRE theta is - what the method deploys - on episodes that
 * do not change from one generation to the next.  A log row describes the perturbed members on that generation's own episodes,
 * and the champion above is the maximum of a noisy score over members and generations; neither is a learning curve.  Here the
 * population gets V more members, P .. P + V - 1, that hold the centre; the handle gets V * E more envs, which the caller restarts
 * from fixed pool slots (bsk_reset_from_pool_shared with the epoch words below, under a mask); the rollout scores them in the
 * launches it issues anyway; the ranking, the log, the champion and the update never see them.  Off by default: an optimiser that
 * never calls bsk_es_set_validation launches the kernels of the definitions above with the arguments it passed before.  f64 + and /
 * only, every operation rounded on its own, no atomics (basilisk_env_amd/policy_ref.py: es_center_ref and es_validate_ref repeat
 * it bit for bit).
 * State with V = n_val members and a ring of C = capacity rows, all in device memory:
 *     val_epoch uint64[V] = epoch0 + v (mod 2^64), constant until the next bsk_es_set_validation: member P + v's epoch word;
 *     val_gen uint64[C], all ones;   val_row f64[C][4], zeros;
 *     the validated champion: val_best_params f32[n_params] in the C-ABI parameter layout (zeros), val_best_fitness f64 (the NaN
 *                   0x7FF8000000000000), val_best_generation uint64 (all ones);
 *     one candidate word `take` that the two kernels of tell use between them.
 * With validation on:
 * bsk_es_ask takes a population of P + V members of the optimiser's spec (one of P members is BSK_EINVAL; with validation off one
 *   of P + V is).  The ask kernel of the definitions above writes members 0 .. P - 1 exactly as before - the device layout is
 *   member-major, it is the same launch on the same pointer - and ONE more launch writes every float of the device blocks of
 *   members P .. P + V - 1: the plain (float)theta_j of its source element under the gather ask uses, for every j, frozen or not,
 *   and zero for the padding.  No sigma * 0 is added: a -0.0 in theta stays -0.0.
 * bsk_es_tell takes d_fitness f64[P + V].  Ranking, log, champion and update read the first P values with the kernels and the
 *   arguments they have.  Two more launches run IN FRONT of the update, behind the log's two when both are on, so theta and the
 *   generation word are still the ones ask used.  The first is one thread: g = the generation word, slot = g mod C (of the whole
 *   64-bit word);
 *        s = f[P];  for v = 1 .. V - 1 ascending: s = s + f[P + v];  f_c = s / (double)V;
 *        L_c the same over mean_len[P + v] when d_mean_len is bound, +0.0 otherwise;
 *        take = f_c is not NaN and (val_best_fitness is NaN or f_c > val_best_fitness) - a tie keeps the older champion, a NaN among
 *          the V values makes f_c a NaN, which never takes;  when take: val_best_fitness = f_c, val_best_generation = g;
 *        always: val_row[slot] = {f_c, L_c, take ? 1.0 : 0.0, (double)V}, val_gen[slot] = g, the candidate word = take.
 *   The second has one thread per parameter j and does nothing unless take; then val_best_params[j] = (float)theta_j, the float the
 *   members P .. P + V - 1 held.  The kernel boundary orders the two launches, as it does for the log: no atomics, no fence.
 * The validation members' observations must not enter an attached normalisation (bsk_population_set_obs_stats_members), and their
 * envs restart under their own mask; a run with validation on then trains bit for bit as the same run with it off.  Under
 * BSK_POLICY_GREEDY f_c is a deterministic function of theta; BSK_POLICY_SAMPLE still draws per global env index and draw counter.
 * A validation env that finishes restarts by the per-env rule; its later episodes do not count, as everywhere.
 * bsk_es_set_validation: n_val in 1..16 with capacity >= 1 allocates (or frees and allocates again) and sets everything above to
 * its initial value; d_mean_len is DEVICE memory, f64[P + V], or NULL - what bsk_population_rollout's d_mean_len writes; it stays
 * bound and is the caller's to keep alive.  n_val == 0 turns validation off and frees it.  Synchronises the device.  Theta, the
 * generation, Adam's state, sigma_vec, the log and the champion are left alone.  BSK_EINVAL before anything else: a NULL
 * optimiser, n_val outside 0..16, capacity < 1 with n_val > 0; then, as bsk_es_set_log, while the stream of the optimiser's last
 * ask / tell / bsk_es_apply_obs_norm is being captured (nothing is changed then, and the capture stays valid). */
int bsk_es_set_validation(bsk_es* es, int n_val, int capacity, uint64_t epoch0, const double* d_mean_len);
/* The whole ring to host memory: gen uint64[C], rows f64[C][4] (either may be NULL); a slot whose val_gen is all ones has never
 * been written.  Synchronises the device.  BSK_EINVAL for a NULL optimiser and with validation off. */
int bsk_es_get_validation_log(bsk_es* es, uint64_t* gen, double* rows);
/* The validated champion to / from host memory: params f32[n_params], fitness, generation; each may be NULL (get: not asked for;
 * set: keep).  For a checkpoint that resumes bit for bit.  Synchronise the device.  BSK_EINVAL for a NULL optimiser and with
 * validation off. */
int bsk_es_get_validated_best(bsk_es* es, float* params, double* fitness, uint64_t* generation);
int bsk_es_set_validated_best(bsk_es* es, const float* params, const double* fitness, const uint64_t* generation);
/* val_best_params as a DEVICE pointer - what bsk_population_set_params_device takes - and the V epoch words as DEVICE words - what
 * bsk_reset_from_pool_shared takes as d_epoch, d_epochs + v for member P + v.  Read-only for the caller; valid until the next
 * bsk_es_set_validation or bsk_es_destroy.  No launch, no copy, no synchronisation.  BSK_EINVAL for NULL pointers and with
 * validation off. */
int bsk_es_validated_best_device(bsk_es* es, const float** d_params);
int bsk_es_validation_epochs_device(bsk_es* es, const uint64_t** d_epochs);

/* The outcome ring: a third record beside the training log and the validation log - what the members of every generation DID, from
 * the rows bsk_population_set_outcomes has the generation's rollout write.  Off by default: an optimiser that never calls
 * bsk_es_set_outcome_log launches the kernels of the definitions above with the arguments it passed before.
 * State of a ring of capacity C >= 1, all in device memory: out_gen uint64[C], all ones after enabling; out_row
 * f64[C][3 * BSK_OUTCOME_COLS], zeros after enabling.  With the ring on bsk_es_tell issues ONE more launch of one wave IN FRONT of
 * the update (behind the log's and the validation's launches where those are on).  It reads the generation word, the first P
 * fitness values and d_rows, and writes only its own ring: ranking, log, champion, update and validation neither read what it
 * writes nor are read by it.  g = the generation word, slot = g mod C (of the whole 64-bit word), R = d_rows:
 *   block A, out_row[slot][0 .. 10], totals over the P ranked members:
 *        col 0 .. 7   the sum over m < P of R[m][col], each converted to an integer, summed as integers, converted to f64 once
 *        col 8        the sum of R[m][8] in the library's one order:  s[l] = R[l][8], or +0.0 when l >= P;  s[l] = s[l] + R[l + 64c][8]
 *                     for c = 1, 2, ... ascending while l + 64c < P;  the tree of strides 32 ... 1;  s[0]
 *        col 9, 10    R[m][9] and R[m][10] combined in the same order by the rule of the member rows (the candidate replaces when it
 *                     is smaller - col 10: greater - or the incumbent is a NaN);  a lane with no member holds the NaN
 *                     0x7FF8000000000000, which every number replaces and which replaces no number
 *   block B, out_row[slot][11 .. 21]:  R[b], the row of the member tell's ranking puts first (rank 0: the member nobody beats under
 *        the order of step 1 above), copied
 *   block C, out_row[slot][22 .. 32]:  block A's rule over the validation members m = P .. P + V - 1 (bsk_es_set_validation), l
 *        counting from member P; with validation off every entry is +0.0
 *   out_gen[slot] = g.   (basilisk_env_amd/policy_ref.py: es_outcome_row_ref repeats the row bit for bit.)
 * bsk_es_set_outcome_log: capacity > 0 allocates (or frees and allocates again) an empty ring; d_rows is DEVICE memory,
 * f64[P + V][BSK_OUTCOME_COLS] - the rows attached to the population the optimiser asks into - it stays bound and is the caller's to
 * keep alive.  capacity == 0 turns the ring off and frees it.  Synchronises the device; everything else of the optimiser is left
 * alone.  BSK_EINVAL: a NULL optimiser, a negative capacity, a NULL d_rows with capacity > 0, and, as bsk_es_set_log, while the
 * stream of the optimiser's last ask / tell / bsk_es_apply_obs_norm is being captured. */
int bsk_es_set_outcome_log(bsk_es* es, int capacity, const double* d_rows);
/* The whole ring to host memory: gen uint64[C], rows f64[C][3 * BSK_OUTCOME_COLS] (either may be NULL); a slot whose out_gen is all
 * ones has never been written.  Synchronises the device.  BSK_EINVAL for a NULL optimiser and with the ring off. */
int bsk_es_get_outcome_log(bsk_es* es, uint64_t* gen, double* rows);

/* Running statistics of the five observation rows, formed on the device: what gives a policy its in_scale / in_shift.  Salimans et
 * al. 2017 and ARS V2 (Mania et al. 2018) normalise the observations by the mean and standard deviation of everything the search
 * has seen so far; the sums behind them are a reduction over data that already lies in the handle's observation rows when the
 * policy launch reads them, so they are formed there, in the stream and in a fixed order, like the fitness.  Opt-in: with no
 * statistics object attached every entry point issues the launches it issued before and leaves the same bits.
 * All arithmetic is f64 with plain + - * / and sqrt, each operation rounded on its own (no FMA); no atomics, and no result depends
 * on the launch shape (basilisk_env_amd/policy_ref.py repeats it bit for bit: obs_stats_accumulate_ref, obs_stats_totals_ref,
 * obs_norm_ref).
 * An object of capacity n_cap spacecraft owns, with W = ceil(n_cap / 64), in device memory and all zero after creation:
 *     part[w][0..9] f64, w = 0 .. W - 1: per wave of 64 spacecraft, entries 0..4 the sums and entries 5..9 the sums of squares of
 *                   the observation rows k = 0 .. 4;   cnt[w] uint64: the number of observations behind them;
 *     tot[0..9] f64 and tot_n uint64: their totals.
 * accumulate, given d_obs f64[5][obs_stride], n and d_alive uint8[n] or NULL - ONE launch, one lane per spacecraft, wave w the
 * spacecraft 64 w .. 64 w + 63:
 *     lane l of wave w has i = 64 w + l and COUNTS when i < n and (d_alive is NULL or d_alive[i] != 0);
 *     per row k:  x = counts ? obs[k][i] : +0.0;   q = x * x;   s1[l] = x, s2[l] = q;
 *     each of the ten values through the fitness tree: for stride = 32, 16, 8, 4, 2, 1:  s[l] = s[l] + s[l + stride] for l < stride;
 *     part[w][k] = part[w][k] + s1[0];   part[w][5 + k] = part[w][5 + k] + s2[0];   cnt[w] = cnt[w] + the number of lanes that count;
 *     a wave in which no lane counts stores nothing.
 *   join, a second launch behind it (behind the LAST step where a rollout accumulates), for each of the ten columns c:
 *     s[l] = part[l][c], or +0.0 when l >= W;  s[l] = s[l] + part[l + 64 m][c] for m = 1, 2, ... ascending while l + 64 m < W
 *     the tree again;  tot[c] = s[0];   tot_n = the sum of cnt[0 .. W - 1] (integer).
 * The normalisation out of the totals (bsk_es_apply_obs_norm), per row k; nothing is written while tot_n == 0:
 *     N = (double)tot_n;   mean = tot[k] / N;   e2 = tot[5 + k] / N;   var = e2 - mean * mean;   var = var > 0 ? var : 0;
 *     sd = sqrt(var);   scale = sd >= std_min ? 1.0 / sd : 0.0;   shift = 0.0 - mean * scale;
 *     theta[k] = scale (in_scale_k);   theta[5 + k] = shift (in_shift_k).
 *   A row that has not varied - the fifth at the start of training - is switched off (scale = 0) and never multiplied by 1 / tiny:
 *   the rule of ARS.  There is no clip: the policy's definition has none.
 * A statistics object belongs to one device, is not thread-safe and serves ONE stream at a time. */
typedef struct bsk_obs_stats bsk_obs_stats;
/* BSK_EINVAL for a NULL `out` and n_cap outside 1..2^28; then the device (BSK_ENODEV when no gfx950 device is usable).
 * Synchronises the device. */
int bsk_obs_stats_create(int n_cap, int device_id, bsk_obs_stats** out);
/* The object is not owned by what it is attached to: destroying one that is still attached to a policy or a population (detach
 * with NULL first) is the caller's error.  Waits for the device first, like every destroy. */
void bsk_obs_stats_destroy(bsk_obs_stats* stats);
/* The two launches above on `stream` (a hipStream_t, NULL = the null stream) of the object's device: raw DEVICE pointers, no copy,
 * no synchronisation, capturable.  d_obs in the layout of bsk_get_obs_device.  BSK_EINVAL before anything is launched: a NULL
 * stats or d_obs, n < 1, n > n_cap, obs_stride < n. */
int bsk_obs_stats_accumulate(bsk_obs_stats* stats, const double* d_obs, int64_t obs_stride, int n, const uint8_t* d_alive, void* stream);
/* tot_n and, per row, mean and var as defined above (var after the clamp), formed on the host from the totals with the operations
 * of the kernel; all three +0 while nothing has been counted.  Each pointer may be NULL.  Ordered after everything queued on the
 * object's device; synchronises it. */
int bsk_obs_stats_get(bsk_obs_stats* stats, uint64_t* count, double* mean5, double* var5);
/* tot[10] and tot_n as DEVICE words (read-only for the caller; valid for the object's lifetime and as fresh as the last join).  No
 * launch, no copy, no synchronisation.  BSK_EINVAL for NULL pointers. */
int bsk_obs_stats_totals_device(bsk_obs_stats* stats, const double** d_tot10, const uint64_t** d_count);
/* The partial rows to / from host memory, part f64[W][10] and cnt uint64[W]: what a checkpoint needs to resume bit for bit (the
 * totals are a function of them, and set forms them again).  get: either may be NULL; set: BSK_EINVAL for a NULL one.  Both
 * synchronise the device. */
int bsk_obs_stats_get_state(bsk_obs_stats* stats, double* part, uint64_t* cnt);
int bsk_obs_stats_set_state(bsk_obs_stats* stats, const double* part, const uint64_t* cnt);
/* Everything back to zero: one memset on `stream`, no copy, no synchronisation. */
int bsk_obs_stats_reset(bsk_obs_stats* stats, void* stream);
/* Attach `stats` to a population / a policy (NULL detaches).  From then on bsk_population_rollout / bsk_policy_rollout accumulate,
 * on the handle's stream and in front of every launch of the policy, the observation the action is chosen FROM, and join once
 * behind the last step: one more launch per env step, one more per rollout.  A population rollout that forms fitness (any of its
 * four fitness outputs given) counts with d_alive = NULL at step 0 and with the alive bytes of its value rule afterwards - as the
 * previous step left them - so exactly the observations of the episode that counts towards the fitness are counted, and tot_n
 * grows by the sum of d_env_len; every other rollout counts every env at every step.  The rollout returns BSK_EINVAL before
 * anything is launched when the handle's n_envs exceeds the capacity of the attached object or the two live on different devices.
 * BSK_EINVAL for a NULL population / policy. */
int bsk_population_set_obs_stats(bsk_population* pop, bsk_obs_stats* stats);
int bsk_policy_set_obs_stats(bsk_policy* p, bsk_obs_stats* stats);
/* Only the envs of the first n_counted members of `pop` feed an attached object (default: all n_members): the accumulate launch of
 * bsk_population_rollout gets n = n_counted * envs_per_member in place of the handle's n_envs, and that is what the capacity is
 * checked against; the kernels are the same.  With n_counted = P under bsk_es_set_validation the validation members' observations
 * never enter the normalisation.  BSK_EINVAL for a NULL population and n_counted outside 1..n_members. */
int bsk_population_set_obs_stats_members(bsk_population* pop, int n_counted);
/* The normalisation above, straight into the optimiser's device theta[0..9]: ONE launch of five threads on `stream`, no copy, no
 * synchronisation, capturable.  bsk_es_ask writes (float)theta_j of frozen parameters into every member, so the next generation
 * runs normalised with no further call.  BSK_EINVAL before anything is launched: NULL pointers, an optimiser with frozen < 10
 * (the search would perturb and move what this call sets), std_min not finite or not positive, optimiser and statistics on
 * different devices. */
int bsk_es_apply_obs_norm(bsk_es* es, bsk_obs_stats* stats, double std_min, void* stream);

/* Fitting a policy to labelled observations on the device: cross-entropy of the action network against int32 labels and,
 * optionally, value_coef * squared error of the value network against f64 targets, by Adam on an f64 master copy of the
 * parameters - planner distillation (behaviour cloning) when the labels are a planner's d_best_action, and the backward pass any
 * other gradient method would stand on.  A fit is attached to ONE policy, reads its device parameters and writes them at every
 * step; policy_kernel, its arguments and its outputs are what they are without a fit.
 * The arithmetic is the definition; f32 unless it says f64, every fmaf one rounding, every other operation rounded on its own.
 *  Forward, per sample: the policy's definition above (x_i, then per unit one k-ascending fmaf chain from the bias), every layer's
 *   activations h_l kept.
 *  Output deltas, action network: m, e_i = expf(l_i - m), s = (e_0 + e_1) + e_2 as in steps 5 / 6 above; p_i = e_i / s;
 *   g_i = p_i - (i == label ? 1.0f : 0.0f).  A sample CONTRIBUTES when its index is below n, its alive byte is non-zero (NULL: all
 *   are) and its label is 0, 1 or 2; for every other sample each g_i is +0.0f, and it is not counted.
 *  Output delta, value network (with targets only): vc = (float)value_coef; d = v - (float)target; g_v = vc * d; +0.0f where the
 *   sample does not contribute.  Without targets the value network is not evaluated, gets no gradient, and the step leaves its
 *   parameters, m and v alone.
 *  Backward through a layer with weights W[j][k], pre-activation deltas d_z[j] and inputs h[k]:
 *   d_h[k] = the j-ascending chain acc = fmaf(W[j][k], d_z[j], acc) from +0.0f;
 *   RELU: d_z_prev[k] = h[k] > 0 ? d_h[k] : +0.0f;   TANH: d_z_prev[k] = d_h[k] * fmaf(-h[k], h[k], 1.0f).
 *   in_scale and in_shift (the first 10 floats) get no gradient and never move.
 *  Block gradients: samples are taken in blocks of 64 consecutive indices 64 b .. 64 b + 63, the last block filled with samples
 *   that do not contribute.  GW_b[j][k] = the sample-ascending chain acc = fmaf(d_z[j][s], h[k][s], acc) from +0.0f;
 *   Gb_b[j] = the sample-ascending chain acc = acc + d_z[j][s] from +0.0f.
 *  Across blocks and calls, f64: A_p = A_p + (double)G_b,p for b ascending, one accumulator per parameter that every accumulate
 *   before the next step continues; a uint64 count of the contributing samples beside it.
 *  Diagnostics, one row of four f64 per accumulate, each a sum over the samples of a block ascending from +0.0 and then over the
 *   blocks ascending from +0.0:  [0] -(double)logp of the label, logp = (l_label - m) - logf(s) of step 6, contributing samples
 *   (others add +0.0);  [1] ((double)d * (double)d) * 0.5 (+0.0 without targets);  [2] the contributing samples whose greedy
 *   action (step 4) is the label;  [3] the contributing samples.
 *  Step: nothing moves while count == 0.  Otherwise for every parameter p >= 10 (of the action network alone when no accumulate
 *   since the last step carried targets), f64 and no FMA:  g = A_p / (double)count + weight_decay * theta_p;  m_p, v_p and the
 *   step term exactly as under bsk_es_set_optimizer;  theta_p = theta_p - (lr * (m_p / (1.0 - p1))) / (sqrt(v_p / (1.0 - p2)) + eps)
 *   - a descent, where the evolution strategy ascends.  A one-thread launch behind it moves beta_pow and the step counter on and
 *   zeroes the count (A_p is zeroed by the update); a last launch writes (float)theta into the policy's device layout.
 * RELU networks: gradients, A, count and the step are reproducible bit for bit from the device's own output deltas
 * (basilisk_env_amd/policy_ref.py: fit_backward_ref, fit_accumulate_ref, fit_step_ref).  expf, logf and tanhf are the device
 * library's: the output deltas, the diagnostics' first column and everything behind a TANH layer are reproducible to a bound.
 * A fit belongs to its policy's device, is not thread-safe and serves ONE stream at a time, like a population.  The policy must
 * outlive it.  bsk_policy_set_params on the attached policy does NOT update theta - the next step would overwrite the policy with
 * the old theta's successor: give the fit the same parameters through bsk_fit_set_state. */
typedef struct bsk_fit bsk_fit;
/* theta := the policy's current parameters (synchronises the device, copies).  BSK_EINVAL: NULL pointers; lr or value_coef not
 * finite or negative; beta1 or beta2 outside [0, 1), eps not finite or <= 0, weight_decay not finite or < 0. */
int bsk_fit_create(bsk_policy* p, double lr, double beta1, double beta2, double eps, double weight_decay, double value_coef,
                   bsk_fit** out);
void bsk_fit_destroy(bsk_fit* f);
/* Two launches on `stream` (a hipStream_t, NULL = the null stream): raw DEVICE pointers, no copy, no synchronisation; capturable
 * once an accumulate of at least this n has allocated the scratch of the block gradients (a call that must allocate returns
 * BSK_EINVAL under capture).
 *   d_obs           f64[5][obs_stride], obs_stride >= n: the layout of bsk_get_obs_device
 *   d_label         int32[n]: what bsk_select_branches / bsk_beam_select leave in d_best_action
 *   d_value_target  f64[n] or NULL (non-NULL with a policy that has no value network: BSK_EINVAL)
 *   d_alive         uint8[n] or NULL
 *   d_dlogits       f32[3][out_stride] or NULL: the g_i of every sample (out_stride >= n)
 * BSK_EINVAL before anything is launched: NULL fit / d_obs / d_label, n < 1 or above 2^28, a stride below n. */
int bsk_fit_accumulate(bsk_fit* f, const double* d_obs, int64_t obs_stride, int n, const int32_t* d_label,
                       const double* d_value_target, const uint8_t* d_alive, float* d_dlogits, int64_t out_stride, void* stream);
/* The step above: three launches on `stream`, no copy, no synchronisation, capturable.  The learning rate is an argument of the
 * launch: a captured graph keeps the one it was captured with. */
int bsk_fit_step(bsk_fit* f, void* stream);
/* The diagnostics row of the last accumulate as DEVICE words, f64[4] (read-only for the caller; valid for the fit's lifetime).  No
 * launch, no copy, no synchronisation. */
int bsk_fit_stats_device(bsk_fit* f, const double** d_row4);
/* theta, m, v f64[n_params], beta_pow f64[2] and the number of steps that moved something; each may be NULL.  Synchronises.  The
 * accumulators A and the count are not part of it: a checkpoint is taken behind a step, where they are zero. */
int bsk_fit_get_state(bsk_fit* f, double* theta, double* m, double* v, double* beta_pow, uint64_t* steps);
/* The same back (NULL: keep; steps always): for a checkpoint that resumes bit for bit, and for new parameters of the policy - a
 * theta given here is also written to the attached policy as (float)theta.  Whatever has been accumulated since the last step is
 * discarded: A, the count and the diagnostics row are zeroed, as behind a step.  Synchronises. */
int bsk_fit_set_state(bsk_fit* f, const double* theta, const double* m, const double* v, const double* beta_pow, uint64_t steps);
/* A new learning rate for the steps enqueued from now on.  BSK_EINVAL when not finite or negative. */
int bsk_fit_set_lr(bsk_fit* f, double lr);
/* The alive bytes of a loop that collects samples from a handle while it steps it (d_alive of bsk_fit_accumulate), by the rule of the
 * population's fitness - an env stops being alive after the first step with reason != 0, and stays out when BSK_FLAG_AUTO_RESET
 * starts its next episode.  first != 0, in front of the loop's first step: d_alive[j] = 1 for every env, and d_reason is not read -
 * the observation every env holds then counts, whatever its last step before the loop left in the reason bytes (an env whose
 * episode is over and that has not been reset is the caller's to reset or to mask).  first == 0, behind each step, with the reason
 * bytes of bsk_get_obs_device:  d_alive[j] = d_alive[j] != 0 && d_reason[j] == 0.  Bytes 1 / 0.  One launch on `stream` of the current
 * device, no copy, no synchronisation, capturable.  BSK_EINVAL for NULL pointers and n < 1. */
int bsk_fit_alive_mask(const uint8_t* d_reason, int n, int first, uint8_t* d_alive, void* stream);

/* Policy-gradient training on top of the fit: an advantage estimator over the histories of bsk_policy_rollout, and the output
 * deltas of a clipped surrogate (PPO; without old log-probabilities plain A2C / REINFORCE) with an entropy bonus in the place of the
 * cross-entropy's.  Everything behind the output deltas is bsk_fit_accumulate's, unchanged.
 *
 * Generalised advantage estimation (Schulman et al. 2016), ONE launch.  Layouts are bsk_policy_rollout's: histories
 * [n_steps][stride], stride >= n_envs.
 *   d_last_value  f32[n_envs] or NULL (= 0): the value of the observation the handle holds after the rollout (bsk_policy_value on
 *                 the handle's observation buffers)
 *   d_adv         f32[n_steps][stride];   d_ret  f64[n_steps][stride] or NULL (f64: it is d_value_target of the fit)
 * Per env j, all f64, no FMA, every operation rounded on its own; gl = gamma * lambda formed once on the host:
 *   carry = 0;  next_v = d_last_value ? (double)last_value[j] : 0
 *   for t = n_steps - 1 .. 0:   v = (double)value[t][j]
 *     reason[t][j] == 0:  delta = (reward[t][j] + gamma * next_v) - v;  carry = delta + gl * carry
 *     otherwise:          delta = reward[t][j] - v;                     carry = delta
 *     adv[t][j] = (float)carry;  ret[t][j] = carry + v;  next_v = v
 * EVERY reason != 0 cuts the bootstrap, the time limit (BSK_DONE_LENGTH) included: the rule of stable-baselines' PPO2, under
 * which the reference's agent was trained - and the only correct one under BSK_FLAG_AUTO_RESET, where value[t + 1] already belongs
 * to the first observation of the next episode.
 * One thread per env walks t downwards; every load and store is coalesced along j; no atomics and no cross-lane traffic, so the
 * launch shape enters no bit (basilisk_env_amd/policy_ref.py: gae_ref, equal bit for bit).  Enqueued on `stream` of the current
 * device: no copy, no synchronisation, no allocation; capturable from the first call.  Columns j >= n_envs are neither read nor
 * written.  BSK_EINVAL before any launch: a NULL history or d_adv; n_steps < 1, n_envs < 1, stride < n_envs; gamma or lambda outside
 * [0, 1] or not finite. */
int bsk_gae(const double* d_reward_hist, const uint8_t* d_reason_hist, const float* d_value_hist, const float* d_last_value,
            int n_steps, int n_envs, int64_t stride, double gamma, double lambda, float* d_adv, double* d_ret, void* stream);
/* bsk_fit_accumulate in everything - scratch rule and capturability, which samples contribute (index below n, alive byte non-zero,
 * d_action in 0..2), the value network's term, block gradients, fold, count, bsk_fit_step, the diagnostics row of
 * bsk_fit_stats_device with d_action in the label's place - but the output deltas of the action network, one more row of
 * diagnostics and one more launch in front (three in all): lp_i below is formed by the policy's own evaluation code for all three
 * actions and read by the fit's kernel, so that it is the logp of bsk_policy_act to the bit; its 3 n floats are part of the scratch.
 *   d_action    int32[n]: the action taken (d_action_hist of the rollout);  d_adv  f32[n]: its advantage (bsk_gae)
 *   d_logp_old  f32[n]: the log-probability the action was taken with (d_logp_hist), or NULL: no ratio, no clipping
 * The loss per sample is  L = -min(r A, clamp(r, lo, hi) A) - ent_coef H,  r = exp(lp_a - logp_old),  H = -sum_i p_i lp_i.
 * With d lp_a / d l_i = (i == a) - p_i:  d(-r A) / d l_i = A r (p_i - (i == a)), and the min takes the clamped branch - whose
 * gradient is zero - exactly where A > 0 and r > hi or A < 0 and r < lo;  d(-H) / d l_i = p_i (lp_i + H).
 * Per sample, all f32, every operation rounded on its own unless written fmaf;  hi = 1.0f + (float)clip, lo = 1.0f - (float)clip
 * and ec = (float)ent_coef formed once on the host:
 *   m, e_i, s as in steps 5 / 6 of the policy's definition;  p_i = e_i / s;  ls = logf(s);  lp_i = (l_i - m) - ls
 *   (expf and logf are the device library's as the compiler expands them: p_i is the p_i of bsk_fit_accumulate, bit for bit, and
 *   lp_i the logp of policy_kernel, bit for bit - in their last bit the two need not stem from one s)
 *   A = d_adv[j];  a = d_action[j]
 *   d_logp_old == NULL:  r = 1.0f, clipped = false
 *   otherwise:           d = lp_a - d_logp_old[j];  r = expf(d);  clipped = (A > 0 && r > hi) || (A < 0 && r < lo)
 *   clipped || A == 0:   gp_i = +0.0f   (the product with c = +0.0f, its sign dropped)
 *   otherwise:           c = A * r;  gp_i = c * (p_i - (i == a ? 1.0f : 0.0f))
 *   ec == 0:  g_i = gp_i
 *   else:     H = -((p_0 * lp_0 + p_1 * lp_1) + p_2 * lp_2);  q_i = p_i * (lp_i + H);  g_i = fmaf(ec, q_i, gp_i)
 * A sample that does not contribute gets +0.0f for each g_i and is not counted, and its d_adv, d_logp_old and d_value_target words
 * (and its d_value_old word in bsk_fit_accumulate_ppo) are NOT READ: they may hold anything, NaN included - an env past its first
 * episode keeps stale history words.  Its observation is read, and must be finite.  Non-finite advantages and old log-probabilities
 * of a contributing sample are outside the numerical contract, as non-finite observations are.  It follows that (1) with d_logp_old == NULL, A = 1 and
 * ent_coef = 0 the deltas, A_p and the count are bsk_fit_accumulate's for label = action, bit for bit; (2) lp_a is formed as
 * policy_kernel forms logp, so with unchanged parameters and d_logp_old from bsk_policy_act or the rollout d is +0.0f, r is 1.0f
 * and nothing is clipped; (3) a sample with A == 0 and ec == 0 contributes +0.0f deltas and is still counted.
 * The policy-gradient row, f64[4] behind bsk_fit_pg_stats_device, written by every bsk_fit_accumulate_pg in the order of the first
 * row (sample-ascending inside a block from +0.0, then block-ascending from +0.0; contributing samples only):
 *   [0] the sum of -(double)d, an estimate of the KL divergence from the old policy (+0.0 without d_logp_old)
 *   [1] the sum of (double)H (computed for this row also when ec == 0)     [2] the clipped samples
 *   [3] the sum of (double)A * (double)r
 * BSK_EINVAL before any launch, beyond bsk_fit_accumulate's rules: NULL d_action or d_adv; clip not finite or outside (0, 1) when
 * d_logp_old is given; ent_coef not finite or negative. */
int bsk_fit_accumulate_pg(bsk_fit* f, const double* d_obs, int64_t obs_stride, int n, const int32_t* d_action, const float* d_adv,
                          const float* d_logp_old, double clip, double ent_coef, const double* d_value_target,
                          const uint8_t* d_alive, float* d_dlogits, int64_t out_stride, void* stream);
/* The policy-gradient row of the last bsk_fit_accumulate_pg as DEVICE words, f64[4] (read-only for the caller; valid for the fit's
 * lifetime; zero before the first).  No launch, no copy, no synchronisation. */
int bsk_fit_pg_stats_device(bsk_fit* f, const double** d_row4);

/* The two things stable-baselines' PPO2 does to every minibatch beyond the clipped surrogate, and the observation normalisation of
 * the evolution strategy for the fit.  All three are off until asked for; without them every entry point above issues the launches,
 * with the arguments, it issued before.  Both reductions are f64 in a fixed order, every operation rounded on its own (no FMA), no
 * atomics: basilisk_env_amd/policy_ref.py repeats them bit for bit (adv_normalize_ref, fit_grad_norm_ref, fit_step_ref).
 *
 * Advantage normalisation, (A - mean) / (sd + eps) over a block d_adv f32[rows][stride] of which the columns below n are used - the
 * rows of one minibatch out of bsk_gae.  d_alive uint8[rows][stride] or NULL; a sample COUNTS when its column is below n and its alive
 * byte is non-zero (NULL: all are).  d_out f32[rows][stride] may be d_adv.  THREE launches, W = ceil(n / 64):
 *  partial sums - wave w is the columns 64 w .. 64 w + 63, lane l the column c = 64 w + l; from a1 = a2 = +0.0 and k = 0 the lane walks
 *   t = 0 .. rows - 1 ascending:  xd = counts ? (double)adv[t][c] : +0.0;  a1 = a1 + xd;  a2 = a2 + xd * xd (the product of two
 *   widened floats is exact);  k = k + (counts ? 1 : 0).  a1 and a2 each through the fitness tree of the observation statistics
 *   above (stride 32 ... 1), k through its integer twin;  part[w] = (a1[0], a2[0]), cnt[w] = k[0] - WRITTEN, not added to: nothing
 *   is carried from call to call.
 *  join - for each of the two columns of part: s[l] = part[l], or +0.0 when l >= W;  s[l] = s[l] + part[l + 64 m] for m = 1, 2, ...
 *   ascending while l + 64 m < W;  the tree;  S1, S2 = s[0].  N = the integer sum of cnt.  With N == 0 the four words below become
 *   +0.0 and d_out is NOT written.  Otherwise, as for an observation row:  mean = S1 / (double)N;  e2 = S2 / (double)N;
 *   var = e2 - mean * mean;  var = var > 0 ? var : 0;  sd = sqrt(var);  inv = 1.0 / (sd + eps).
 *  apply - a sample that counts:  out[t][c] = (float)(((double)adv[t][c] - mean) * inv);  any other with c < n:  +0.0f.  Columns at
 *   and above n are neither read nor written.
 * d_work: bsk_adv_normalize_work_bytes(n) = 8 * (4 + 3 W) bytes of device memory, 8-byte aligned, the caller's; after the call its
 * first four f64 words are {mean, sd, inv, (double)N} and the rest is scratch (part, cnt).  Enqueued on `stream` of the current
 * device: no copy, no synchronisation, no allocation; capturable from the first call.  All samples equal give sd = 0 and outputs
 * of +-0 (or (x - mean) / eps where the mean's rounding leaves a difference): eps keeps them finite, as in PPO2.
 * BSK_EINVAL before any launch: a NULL d_adv, d_out or d_work; rows < 1, n < 1, stride < n; rows * stride > 2^31; eps not finite or
 * not positive.  bsk_adv_normalize_work_bytes returns 0 for n < 1. */
int64_t bsk_adv_normalize_work_bytes(int n);
int bsk_adv_normalize(const float* d_adv, const uint8_t* d_alive, int rows, int n, int64_t stride, double eps, float* d_out, void* d_work,
                      void* stream);
/* Clipping of the gradient's global norm inside bsk_fit_step (TensorFlow's clip_by_global_norm, PPO2's max_grad_norm).  max_norm = 0
 * (the default) is off: bsk_fit_step is the three launches above.  Otherwise ONE launch goes in front of them, one workgroup of
 * 1 024 threads over the parameters p = 10 .. n_upd - 1 the step moves (the action network's alone when no accumulate since the last
 * step carried targets), f64, no FMA:
 *   g_q = A[10 + q] / (double)count, the division of the step;  thread i:  s = g_i * g_i, or +0.0 when there is no q = i;
 *   s = s + g_q * g_q for q = i + 1024, i + 2048, ... ascending;  each of the sixteen waves joins its 64 lanes in the fitness tree;
 *   S = ((w_0 + w_1) + w_2) + ... + w_15;  norm = sqrt(S);  scale = max_norm / (norm > max_norm ? norm : max_norm)
 *   - exactly 1.0 while norm <= max_norm (and for a NaN norm);  count == 0:  {norm, scale} = {+0.0, 1.0}.
 * and the step uses  g = (A_p / (double)count) * scale + weight_decay * theta_p:  the L2 term is added behind the clip.  It follows
 * that (1) with max_norm above the norm theta, m, v, beta_pow and the step counter are the unclipped step's bit for bit, since
 * x * 1.0 is x; (2) the norm reported is the norm before clipping.
 * BSK_EINVAL: a NULL fit; max_norm negative or not finite.  No launch; it holds for the steps enqueued from now on, and a captured
 * graph keeps what it was captured with. */
int bsk_fit_set_max_grad_norm(bsk_fit* f, double max_norm);
/* {norm, scale} of the last step taken with clipping on, as DEVICE words f64[2] ({+0.0, 1.0} before the first; read-only for the
 * caller; valid for the fit's lifetime).  No launch, no copy, no synchronisation. */
int bsk_fit_grad_norm_device(bsk_fit* f, const double** d_row2);
/* bsk_es_apply_obs_norm for the fit: the normalisation out of the totals of `stats` into the fit's f64 theta[0..9] - which no step
 * moves - and (float)theta into the attached policy's device layout.  TWO launches on `stream`, no copy, no synchronisation,
 * capturable.  While nothing has been counted theta is not written.  theta[10..], m and v are never touched.  BSK_EINVAL before
 * anything is launched: NULL pointers, std_min not finite or not positive, fit and statistics on different devices. */
int bsk_fit_apply_obs_norm(bsk_fit* f, bsk_obs_stats* stats, double std_min, void* stream);

/* The last two pieces of PPO2's update: minibatches drawn from a new permutation of all n_steps * n_envs samples in every epoch,
 * and the clipped value loss (cliprange_vf).  Both are off until asked for; without them every entry point above issues the
 * launches, with the arguments, it issued before.
 *
 * The permutation of [0, N), 1 <= N < 2^31, is never stored: it is a function of two uint64 DEVICE words {seed, epoch}, the
 * caller's, as the policy's {seed, draw} are.  All arithmetic is uint32 unless stated (policy_ref.py: pg_perm_ref, equal bit for
 * bit; csrc/bsk_shuffle.hpp):
 *   b = max(2, bit_length(N - 1));  a = b >> 1;  c = b - a    - an unbalanced Feistel network over 2^b < 2 N values
 *   the eight round keys  k[4 i .. 4 i + 3] = philox4x32_10(c0 = epoch_lo, c1 = epoch_hi, c2 = 0x50475348, c3 = i;
 *                                                            key = seed_lo, seed_hi)  for i = 0, 1
 *   fmix(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 *   perm(q):  x = q;  repeat
 *               L = x >> c;  R = x & (2^c - 1);  wl = a;  wr = c
 *               for r = 0 .. 7:  F = fmix(R ^ k[r]) & (2^wl - 1);  (L, R) = (R, L ^ F);  swap(wl, wr)
 *               x = (L << wr) | R
 *             until x < N   (cycle walking)
 * The walk always ends - the cycle of q under the permutation of 2^b values returns to q < N - and has NO cap: a cap would break
 * the bijection.  Its mean length is below two trips.
 *
 * bsk_pg_gather: one minibatch out of the rollout histories into contiguous buffers, ONE launch, one thread per output position.
 * N = n_steps * n_envs;  output position i in [0, m) takes sample s = perm(q0 + i), or s = q0 + i with d_state == NULL;
 * t = s / n_envs, j = s % n_envs.  The histories are [n_steps][stride] (d_action_hist int32, d_adv, d_logp_hist and d_value_hist
 * f32, d_ret f64) and d_obs_hist f64[n_steps][5][stride], word r of the sample at [t][r][j];  d_obs_out is f64[5][out_stride] - a
 * chunk of it is bsk_fit_accumulate_pg's d_obs as it is -, the other outputs [m], and d_index_out int32[m] receives s.  Each
 * history and its output are both NULL or both given; d_index_out may be given alone.  Columns j >= n_envs of the histories are not
 * read, and nothing but positions 0 .. m - 1 of an output (of each of the five rows of d_obs_out) is written.  Enqueued on
 * `stream` of the current device: no copy, no synchronisation, no allocation; capturable from the first call, and a replayed
 * graph reads the state words as they are THEN.  The stores are coalesced, the loads scattered by construction.
 * BSK_EINVAL before any launch: n_steps < 1, n_envs < 1, N >= 2^31, stride < n_envs; q0 < 0, m < 1, q0 + m > N; out_stride < m
 * with d_obs_hist; a history without its output or the reverse; nothing to write.
 * bsk_pg_shuffle_advance: epoch += 1, ONE launch of one thread, under the same terms.  BSK_EINVAL: d_state NULL. */
int bsk_pg_gather(const uint64_t* d_state, int n_steps, int n_envs, int64_t stride, int64_t q0, int m, const double* d_obs_hist,
                  const int32_t* d_action_hist, const float* d_adv, const float* d_logp_hist, const double* d_ret,
                  const float* d_value_hist, double* d_obs_out, int64_t out_stride, int32_t* d_action_out, float* d_adv_out,
                  float* d_logp_out, double* d_ret_out, float* d_value_out, int32_t* d_index_out, void* stream);
int bsk_pg_shuffle_advance(uint64_t* d_state, void* stream);
/* bsk_fit_accumulate_pg - which is this call with d_value_old = NULL, clip_vf = 0, d_dvalue = NULL - with PPO2's value loss
 * max((v - R)^2, (v_old + clamp(v - v_old, -clip_vf, clip_vf) - R)^2) / 2 in the squared error's place.  d_value_old f32[n]: the
 * values the rollout recorded (d_value_hist);  d_dvalue f32[n] or NULL: receives the value network's output delta of every sample
 * below n, +0.0f where the sample does not contribute - the counterpart of d_dlogits.  With either pointer the block launch is a
 * third instantiation of the kernel and the fold one over ten terms per block; with neither, the launches of bsk_fit_accumulate_pg.
 * Per contributing sample, f32, every operation rounded on its own;  cv = (float)clip_vf:
 *   v = the value network's output;  R = (float)d_value_target[j];  d = v - R
 *   d_value_old == NULL:  delta = value_coef * d, the term (double)d * (double)d / 2    (bsk_fit_accumulate's text)
 *   otherwise  vo = d_value_old[j];  dv = v - vo
 *     -cv <= dv && dv <= cv:  as above
 *     else  vc = vo + (dv > 0 ? cv : -cv);  d2 = vc - R
 *       d2 * d2 > d * d:  the clipped branch holds the max and its gradient is zero:  delta = +0.0f, the term is
 *                         (double)d2 * (double)d2 / 2, and the sample is VALUE-CLIPPED
 *       otherwise:        as above (a tie is the unclipped branch's)
 * Column [1] of the first diagnostics row sums the term above.  A third row, f64[2] behind bsk_fit_vclip_stats_device, is written
 * in the first row's order by launches with d_value_old ONLY: [0] the value-clipped samples, [1] the sum of the unclipped
 * (double)d * (double)d / 2.  It follows that with clip_vf above every |dv| the accumulators and the first two rows are
 * bsk_fit_accumulate_pg's bit for bit.
 * BSK_EINVAL before any launch, beyond bsk_fit_accumulate_pg's rules: d_value_old or d_dvalue without d_value_target (and so
 * without a value network); clip_vf not finite or <= 0 when d_value_old is given. */
int bsk_fit_accumulate_ppo(bsk_fit* f, const double* d_obs, int64_t obs_stride, int n, const int32_t* d_action, const float* d_adv,
                           const float* d_logp_old, double clip, double ent_coef, const double* d_value_target,
                           const float* d_value_old, double clip_vf, const uint8_t* d_alive, float* d_dlogits, int64_t out_stride,
                           float* d_dvalue, void* stream);
/* The value-clip row as DEVICE words, f64[2] (read-only for the caller; valid for the fit's lifetime; zero before the first launch
 * with d_value_old).  No launch, no copy, no synchronisation. */
int bsk_fit_vclip_stats_device(bsk_fit* f, const double** d_row2);

/* A training log for the policy-gradient loop: a ring of rows f64[capacity][BSK_PG_LOG_COLS] in DEVICE memory, the caller's, one row
 * per iteration, formed by small launches behind bsk_gae and behind the last bsk_fit_step - so that a loop replayed from a graph,
 * with no host in it, still says how the episodes went.  Free functions of the current device; none allocates, copies or
 * synchronises, all are capturable from the first call.  Nothing here writes a buffer that training reads.  All f64, every
 * operation rounded on its own (no FMA), no atomics, a fixed order: basilisk_env_amd/policy_ref.py repeats it bit for bit
 * (pg_episodes_ref, pg_log_update_ref).  The row (PG_LOG_COLUMNS in Python); counts are integers converted to f64 once:
 *   [0] episodes ended in this rollout      [1], [2] the sum and the sum of squares of their undiscounted returns
 *   [3], [4] the least and the greatest of those returns (NaN with none)      [5] the sum of their lengths in steps
 *   [6 .. 9] ends by BSK_DONE_LENGTH, _WHEELS, _BATTERY, _ORBIT (a reason byte with two bits set counts in both, the outcome rows'
 *   rule)      [10 .. 12] steps under action 0, 1, 2 (any other value is counted nowhere)      [13] the sum of all rewards
 *   [14] the explained variance 1 - var(ret - value) / var(ret), PPO2's explained_variance      [15] the sum of (ret - value)^2
 *   [16 .. 19] the policy-gradient diagnostics row (bsk_fit_pg_stats_device) summed over every accumulate of the iteration
 *   [20 .. 23] the same sum of the fit's row (bsk_fit_stats_device)
 *   [24] the sum of the gradient norms of the iteration's steps      [25] the steps whose gradient was clipped (scale < 1.0)
 *
 * bsk_pg_episodes: columns 0 .. 15 from the histories of one rollout, [n_steps][stride] in bsk_policy_rollout's layout, TWO
 * launches.  d_action_hist may be NULL (columns 10 .. 12 are then 0); d_value_hist and d_ret (bsk_gae's) both or neither.  The
 * return and the length of every env's RUNNING episode are carried from call to call in d_ep_return f64[n_envs] and d_ep_len
 * int32[n_envs], the caller's: zero bytes mean a fresh env, and an episode that began before the state was zeroed reports only what
 * was seen of it.  Per env j, from R = d_ep_return[j], L = d_ep_len[j], rows t = 0 .. n_steps - 1 ASCENDING, sums from +0.0, the
 * extremes from NaN, counts from 0:
 *   R = R + reward[t][j];  L = L + 1;  s_rew = s_rew + reward[t][j];  act_n[action[t][j]] += 1
 *   y = ret[t][j];  v = (double)value[t][j];  e = y - v;  s_y = s_y + y;  s_y2 = s_y2 + y * y;  s_e = s_e + e;  s_e2 = s_e2 + e * e
 *   reason[t][j] != 0:  s_R = s_R + R;  s_R2 = s_R2 + R * R;  mn, mx take R under the rule of the outcome rows (the candidate
 *     replaces the incumbent when it is smaller / greater or the incumbent is a NaN);  n_ep += 1;  len_sum += L;  one count per set
 *     bit of the four;  then R = +0.0, L = 0
 * and R, L are written back.  Wave w is the envs 64 w .. 64 w + 63 (a lane at or above n_envs brings +0.0, NaN and 0): the seven
 * sums {s_R, s_R2, s_rew, s_y, s_y2, s_e, s_e2} each through the fitness tree of the observation statistics (stride 32 ... 1), the
 * two extremes through the same tree under their rule (lane l the incumbent, lane l + stride the candidate), the ten counts {n_ep,
 * len_sum, the four ends, the three actions, the samples walked} as integers; lane 0 WRITES the 19 words of wave w into d_work - no
 * state is carried there.  The join is bsk_adv_normalize's per column: s[l] = the entries w = l, l + 64, ... ascending from the
 * first (+0.0, or NaN, with none), then the tree.  With N the samples walked, as for an observation row:
 *   mean_y = S_y / N;  var_y = max(S_y2 / N - mean_y * mean_y, 0);  likewise var_e;  [14] = 1.0 - var_e / var_y,
 * NaN when var_y == 0 (PPO2's rule) or without the value and return histories ([15] is then +0.0).
 * The row goes to slot *d_counter % capacity of d_ring, slot 0 with d_counter NULL; columns 16 .. 25 are left as they are.
 * d_work: bsk_pg_episodes_work_bytes(n_envs) = 8 * 19 * ceil(n_envs / 64) bytes, 8-byte aligned (0 for n_envs < 1).  Columns at or
 * above n_envs of a strided history are neither read nor written.  One env per lane: latency-bound at 65 536 envs, as bsk_gae is.
 * BSK_EINVAL before any launch: NULL reward, reason, state, work or ring pointers; exactly one of d_value_hist and d_ret;
 * n_steps < 1, n_envs < 1, stride < n_envs, capacity < 1; n_steps * stride > 2^31.
 *
 * bsk_pg_log_update: columns 16 .. 25 of the slot, ONE launch of one wave.  d_diag f64[n_rows][8]: [16 + c] = the sum of column c,
 * rows ascending from the first.  d_norms f64[n_norms][2] = {norm, scale} rows (bsk_fit_grad_norm_device) or NULL: [24] = the sum
 * of the norms ascending from the first, [25] = the rows with scale < 1.0; with NULL +0.0 and 0.  Columns 0 .. 15 are left as they
 * are.  BSK_EINVAL: NULL d_diag or d_ring; n_rows < 1; capacity < 1; d_norms given with n_norms < 1.
 *
 * bsk_pg_log_advance: d_gen[*d_counter % capacity] = *d_counter;  *d_counter += 1 - ONE launch of one thread.  d_gen
 * uint64[capacity] names the iteration every slot holds (the caller fills it with all ones: never written).  BSK_EINVAL: NULL d_gen
 * or d_counter; capacity < 1. */
#define BSK_PG_LOG_COLS 26
size_t bsk_pg_episodes_work_bytes(int n_envs);
int bsk_pg_episodes(const double* d_reward_hist, const uint8_t* d_reason_hist, const int32_t* d_action_hist, const float* d_value_hist,
                    const double* d_ret, int n_steps, int n_envs, int64_t stride, double* d_ep_return, int32_t* d_ep_len, void* d_work,
                    double* d_ring, int capacity, const uint64_t* d_counter, void* stream);
int bsk_pg_log_update(const double* d_diag, int n_rows, const double* d_norms, int n_norms, double* d_ring, int capacity,
                      const uint64_t* d_counter, void* stream);
int bsk_pg_log_advance(uint64_t* d_gen, int capacity, uint64_t* d_counter, void* stream);

/* Reward scaling for the policy-gradient loop: the rewards of a rollout divided by the running standard deviation of the discounted
 * return and clipped - what stable-baselines' VecNormalize(norm_reward=True) does to every PPO2 run -, so that the value network
 * regresses targets of order one whatever the reward's unit.  A free function of the current device; it does not allocate, copy or
 * synchronise and is capturable from the first call.  All f64, every operation rounded on its own (no FMA), no atomics, a fixed
 * order: basilisk_env_amd/policy_ref.py repeats it bit for bit (reward_norm_ref).
 *
 * d_state: BSK_REWARD_NORM_STATE_WORDS = 8 words of 8 bytes in DEVICE memory, the caller's; all zero means fresh:
 *   [0] sum of the running returns seen      [1] sum of their squares      [2] their number (uint64)
 *   [3] mean      [4] var      [5] sd      [6] the number of updating calls (uint64)      [7] 0
 * d_ret_run f64[n_envs], the caller's: the running discounted return of every env, carried from call to call (zeros: fresh envs).
 * The histories are [n_steps][stride] in bsk_policy_rollout's layout; W = ceil(n_envs / 64).
 *
 * With update != 0, TWO launches in front of the apply:
 *  walk - wave w is the envs 64 w .. 64 w + 63, lane l the env j = 64 w + l; from R = d_ret_run[j], a1 = a2 = +0.0 and k = 0 the lane
 *   walks t = 0 .. n_steps - 1 ASCENDING:
 *     R = gamma * R + reward[t][j]  (the product rounded, then the sum);  a1 = a1 + R;  a2 = a2 + R * R;  k = k + 1;
 *     reason[t][j] != 0:  R = +0.0  - AFTER it was counted, VecNormalize's order
 *   and d_ret_run[j] = R.  a1 and a2 each through the fitness tree of the observation statistics above (stride 32 ... 1; a lane at
 *   or above n_envs brings +0.0 and 0), k through its integer twin;  work[w] = (a1[0], a2[0], k[0]) - WRITTEN, not added to: the
 *   partial rows hold no state from call to call.
 *  join - bsk_adv_normalize's rule per column of work: s[l] = work[l], or +0.0 when l >= W;  s[l] = s[l] + work[l + 64 m] for
 *   m = 1, 2, ... ascending while l + 64 m < W;  the tree;  S1, S2 = s[0];  K = the integer sum of the counts.  Then one thread:
 *     sum = sum + S1;  sum_sq = sum_sq + S2;  count += K;  calls += 1;
 *     mean = sum / (double)count;  var = max(sum_sq / (double)count - mean * mean, 0)  (as for an observation row);
 *     sd = sqrt(var + eps);  word [7] = 0.
 * Always, ONE launch:
 *  apply - d = (count != 0) ? sd : 1.0, read from the state as it is behind the join;  for every t and every j < n_envs
 *     y = reward[t][j] / d;  out[t][j] = y > clip ? clip : (y < -clip ? -clip : y)      - a NaN passes through.
 *   Elementwise, each thread its own element: d_out may be d_reward_hist.
 * So the statistics take in the WHOLE rollout first and then the whole rollout is scaled by one number.  This deviates from
 * VecNormalize on purpose: it updates its statistics step by step, so the steps of one rollout are divided by n_steps different
 * numbers and the very first by the deviation of a single step's returns.  Here the scale is defined in the first rollout, and a
 * rollout costs three launches instead of n_steps.  As there, the mean is not subtracted, and the returns are discounted forward in
 * time from the past, which is not the return the value network regresses.
 * With update == 0 only the apply is launched: the statistics are frozen and d_ret_run and d_work are neither read nor written (they
 * may be NULL), as for evaluation.  On a fresh state that is the identity under the clip.
 * d_work: bsk_reward_norm_work_bytes(n_envs) = 8 * 3 * W bytes, 8-byte aligned (0 for n < 1).  Columns at or above n_envs of a
 * strided history are neither read nor written.  The walk is one env per lane: latency-bound at 65 536 envs, as bsk_gae is.
 * BSK_EINVAL before any launch: a NULL history, d_state or d_out; update != 0 with a NULL d_ret_run or d_work; n_steps < 1,
 * n_envs < 1, stride < n_envs; n_steps * stride > 2^31; gamma outside [0, 1] or not finite; eps negative or not finite; clip not
 * greater than 0, or NaN (+inf is allowed: nothing is then clipped). */
#define BSK_REWARD_NORM_STATE_WORDS 8
int64_t bsk_reward_norm_work_bytes(int n);
int bsk_reward_norm(const double* d_reward_hist, const uint8_t* d_reason_hist, int n_steps, int n_envs, int64_t stride, double gamma,
                    double eps, double clip, int update, double* d_ret_run, void* d_state, void* d_work, double* d_out, void* stream);

/* Schedules for the policy-gradient loop and a KL stop per update: lr, clip, clip_vf and ent_coef annealed over the run, and the
 * remaining steps of an update dropped once the policy has moved too far - both as state in DEVICE words of the fit, so that a
 * replayed graph carries them (arguments by value are baked into a capture).  Off by default; off, every entry point above enqueues
 * the kernels it always did with the arguments it always did.
 *
 * The fit owns BSK_FIT_SCHEDULE_WORDS = 8 words of 8 bytes (bsk_fit_schedule_device; not part of bsk_fit_get_state / _set_state):
 *   [0] lr now (f64)   [1] clip now (f64)   [2] clip_vf now (f64)   [3] ent_coef now (f64)   [4] iteration (uint64)
 *   [5] gate (uint64: 0 open, 1 closed)   [6] steps skipped in this iteration (uint64)
 *   [7] the minibatch's mean KL that closed the gate (f64), +0.0 while it is open
 * The rule, all f64, every operation rounded on its own (no FMA), for a pair {a, b} at iteration `it` of `total`:
 *   total == 0 or it == 0:  a, exactly;      it >= total:  b, exactly (not a + (b - a));
 *   otherwise:  a + (b - a) * ((double)it / (double)total).
 * PPO2's lr * (1 - (update - 1) / nupdates) is the rule with b = 0.
 *
 * bsk_fit_set_schedule: attaches *s (NULL: detaches).  Attaching writes the words of iteration 0 with the gate open, and
 *  synchronises.  BSK_EINVAL unless, for BOTH ends of a pair: lr finite and not negative; clip in (0, 1); clip_vf finite and
 *  positive; ent_coef finite and not negative; and total < 2^53; kl_stop 0 (no stop) or finite and positive.
 * While a schedule is attached:
 *  bsk_fit_accumulate_pg / _ppo launch scheduled instantiations of the block kernel, which take
 *    clip_hi = 1.0f + (float)word[1],  clip_lo = 1.0f - (float)word[1],  ent_coef = (float)word[3],  clip_vf = (float)word[2]
 *   - the roundings these entry points apply to their arguments, so a scheduled launch is bit for bit the unscheduled one called
 *   with the words' values.  Their scalar arguments clip, ent_coef and clip_vf are still validated, and then not read.  Whether
 *   d_logp_old and d_value_old are given still decides ratio and value clip.  bsk_fit_accumulate is untouched.
 *  bsk_fit_step launches a scheduled instantiation of the Adam kernel, which takes lr = word[0]; the fit's own lr is not read.
 * bsk_fit_schedule_begin - ONE launch of one thread at the start of an update: words [0..3] from word [4] by the rule; gate = 0,
 *  skipped = 0, word [7] = +0.0.
 * bsk_fit_kl_gate - ONE launch of one wave, in front of a step's launches: d_diag f64[n_rows][8], rows in the loop's log layout
 *  (the policy-gradient row {kl_sum, entropy_sum, clipped, surrogate_sum}, then the diagnostics row {nll_sum, value_loss_sum,
 *  correct, count}) of the accumulates since the last step.  S = column 0 and N = column 7, each summed ascending FROM the first
 *  row;  mean = S / N.  The gate closes when it is closed already, or when N > 0 and !(mean <= kl_stop): a NaN mean closes it, a mean
 *  exactly at kl_stop does not.  On the closing transition word [7] = mean.  Whenever it is closed, now or earlier: the fit's
 *  count = 0 and skipped += 1 - the bsk_fit_step behind it is then the no-op it is with nothing accumulated: A is cleared, theta, m,
 *  v, beta_pow and steps do not move.  The KL is the loop's estimator mean(logp_old - logp), which can be negative.  Accumulates
 *  behind a closed gate still run and are discarded: the launch sequence is static, which is what a graph needs.
 * bsk_fit_schedule_end - ONE launch of one thread at the end of an update: with d_ring f64[capacity][BSK_SCHED_LOG_COLS] given,
 *  row [iteration % capacity] = {(double)iteration, lr, clip, clip_vf, ent_coef, (double)skipped, word [7], (double)gate}; then
 *  iteration += 1.  A ring memset to 0xFF reads as NaN iterations: never written.
 * The three allocate nothing, copy nothing and do not synchronise: capturable from the first call.  BSK_EINVAL with no schedule
 * attached; bsk_fit_kl_gate also with kl_stop == 0, a NULL d_diag or n_rows < 1; bsk_fit_schedule_end with d_ring given and
 * capacity < 1.
 * bsk_fit_get_schedule_state copies the eight words out; bsk_fit_set_schedule_state writes the words of `iteration` with the gate
 * open (BSK_EINVAL with no schedule attached) - for checkpoints; both synchronise. */
#define BSK_FIT_SCHEDULE_WORDS 8
#define BSK_SCHED_LOG_COLS 8
typedef struct bsk_fit_schedule {
    double lr[2], clip[2], clip_vf[2], ent_coef[2];     /* {a, b}: the value at iteration 0, the value from iteration `total` on */
    uint64_t total;
    double kl_stop;
} bsk_fit_schedule;
int bsk_fit_set_schedule(bsk_fit* f, const bsk_fit_schedule* s);
int bsk_fit_schedule_begin(bsk_fit* f, void* stream);
int bsk_fit_kl_gate(bsk_fit* f, const double* d_diag, int n_rows, void* stream);
int bsk_fit_schedule_end(bsk_fit* f, double* d_ring, int capacity, void* stream);
int bsk_fit_schedule_device(bsk_fit* f, const uint64_t** d_words8);
int bsk_fit_get_schedule_state(bsk_fit* f, uint64_t* words8);
int bsk_fit_set_schedule_state(bsk_fit* f, uint64_t iteration);

/* Synchronises the handle's stream.  Like every synchronising entry point (bsk_get_obs*, bsk_get_state, bsk_get_batch_stats,
 * bsk_get_terminal_obs) it then checks the handle's device error word and returns BSK_EHIP when a kernel raised it: the
 * three-wave form's barrier-free exchange gives up after 2^20 polls instead of hanging, and says so here. */
int bsk_sync(bsk_handle* h);

/* Process-wide counts of the host <-> device copies and stream synchronisations this library has issued (tests assert that the
 * device-resident entry points issue none).  Either pointer may be NULL. */
int bsk_debug_counters(int64_t* n_copies, int64_t* n_syncs);
/* Probe builds only (csrc/bsk_probes.hpp; all zeros from the product library): the word every wavefront of the last launch left
 * in the handle's debug buffer, uint64[ceil(n_envs / 64)].  Synchronises. */
int bsk_debug_words(bsk_handle* h, uint64_t* words);

/* Per-launch timing of the step kernel with hipEvents recorded on the handle's stream around
 * each launch.  begin() arms it (capacity launches); end() synchronises and reports the mean
 * kernel duration in milliseconds over the launches seen since begin(). */
int bsk_profile_begin(bsk_handle* h, int capacity);
/* stride 1 (default): every launch is stamped.  stride > 1: a pair of launches is stamped every
 * `stride` launches and only the second of the pair is counted (the first absorbs the transition
 * from un-stamped back-to-back launches).  Stamping costs ~5 us of launch throughput per stamped
 * launch on MI355X, so a timed region samples instead of stamping every launch. */
int bsk_profile_set_stride(bsk_handle* h, int stride);
int bsk_profile_end(bsk_handle* h, double* mean_kernel_ms, int* n_launches);
/* Same, also copying the individual kernel durations [ms] of the first min(cap, n) counted launches
 * into samples_ms (so that a caller can report median / min / max beside the mean). */
int bsk_profile_end_samples(bsk_handle* h, double* mean_kernel_ms, int* n_launches, float* samples_ms, int cap);

/* Measurement aid: the fp64 FMA rate device `device_id` sustains with `waves_per_simd` waves of independent v_fma_f64 chains per
 * SIMD (median of `repeats` timed launches of ~2-4 ms after three warm-up launches): TFLOP/s of the whole device and
 * nanoseconds per FMA wave-instruction and SIMD.  bench.py prints it beside its fp64 rooflines, whose `peak` stays the nominal
 * 78.6 TFLOP/s. */
int bsk_calibrate_fp64(int device_id, int waves_per_simd, int repeats, double* tflops, double* ns_per_fma_per_simd);

/* Kernel resource facts for DESIGN.md / bench: name of the kernel variant the handle's LAST launch ran, its VGPR count, static
 * LDS bytes and the launch geometry.  The variant is chosen per launch: batches of <= 16 384 spacecraft run launches of >= 16
 * sub-steps in a wave-split form of the same arithmetic (bit-identical results: "...,pair" at the power level - a dynamics and
 * an FSW + environment wave per 64 spacecraft, 128-thread workgroups - and "...,tri" at the full-scenario level - a
 * translational, a rotational and the FSW + environment wave, 192-thread workgroups), everything else the
 * single-wave form - except one-sub-step launches of the bare level (point mass or J2, with wheels, nav_lag != 0, no IC pool) for
 * batches of 128 to 256 spacecraft per CU of the device (32 768 - 65 536 on a whole MI355X), which run "...,halves": a rotational and
 * a translational wave per 64 spacecraft, 128-thread workgroups, bit-identical results (bsk_set_halves_form: off / on at any size).
 * BSKGPU_PAIR / BSKGPU_TRI = 0 | 1 in the environment of bsk_create switch a form off / on for every launch.
 * Before the first launch: the single-wave form of the config (harmonics: the form of the last bsk_set_gravity_sh, the one-wave
 * DPP form before any). */
int bsk_kernel_info(bsk_handle* h, char* name, int name_cap, int* vgprs, int* lds_bytes,
                    int* block, int* grid);

const char* bsk_last_error(void);
const char* bsk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BSKGPU_H */
