/*
 * quadrace.h -- C ABI of libquadrace.so: the MI355X-native (gfx950) vectorised quadrotor race
 * environment that replaces the NumPy hot path of tudelft/optimal_quad_control_RL.
 *
 * What each entry point replaces (R: = "3D quad race.ipynb", I: = "3D quad race INDI inner loop.ipynb",
 * raw .ipynb line numbers as in SURVEY.md section 0):
 *
 *   qr_create / qr_set_track      Quadcopter3DGates.__init__            R:288-360   I:143-214
 *   qr_set_residual               torch.load(NNDroneModel .pt)          R:227-245   (c_code/nn_thrust.c, nn_moment.c layout)
 *   qr_set_disturbance            env.disturbance_ranges / _scale       R:355-358, R:772-781
 *   qr_set_limits                 env.max_steps / env.dt                R:345-346, I:648
 *   qr_set_pause                  env.pause                             R:360, R:570-572
 *   qr_set_pause_if_collision     env.pause_if_collision                R:293, R:573-578
 *   qr_seed                       VecEnv.seed (no-op upstream)          R:600-601
 *   qr_reset                      reset() / reset_(dones)               R:452-496   I:267-299
 *   qr_step                       step_async() + step_wait()            R:498-595   I:301-385
 *   qr_observe                    update_states_gate()                  R:365-450   I:218-265
 *   qr_get_state / qr_set_state   direct attribute access to world_states, disturbances, target_gates,
 *                                 step_counts                           R:803, R:4499-4500
 *   qr_get_track_tables           gate_pos_rel / gate_yaw_rel           R:307-319   (pinned by c_code/nn_controller.c:40-60)
 *
 * Conventions (precedent: the reference's own ctypes use, R:4395-4417 -- POINTER(c_float) arguments,
 * caller-allocated outputs):
 *   - every function returns 0 on success, <0 on error (see QR_E_*); qr_last_error() gives text
 *     (thread-local). No exception crosses this boundary.
 *   - all buffer arguments named *_dev are DEVICE pointers (HBM of the GPU the env was created on) owned
 *     by the caller (e.g. torch tensor .data_ptr()); the library never frees or retains them beyond the
 *     kernels it enqueues in that call.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). Calls enqueue work and return
 *     without synchronising; results are ordered on that stream.
 *   - a handle is bound to one GPU and is not thread-safe.  Every entry point that touches the device makes the
 *     handle's GPU the current HIP device first (and leaves it current), so one process may drive handles on
 *     several GPUs; `stream` must belong to that GPU.
 *   - there is NO CPU fallback: qr_create fails with QR_E_NO_DEVICE when no gfx950 device is visible.
 *
 * Layouts at the boundary are the reference's row-major arrays: actions [N][4], obs [N][obs_len],
 * rewards [N] f32, dones [N] u8, world [N][S] (S = 16 E2E / 13 INDI), disturbances [N][6].
 * Internally the state lives in HBM as planar float4 structure-of-arrays.
 */
#ifndef QUADRACE_H
#define QUADRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libquadrace.so is built with -fvisibility=hidden: only what this header declares is exported */
#pragma GCC visibility push(default)

#define QR_ABI_VERSION 3   /* additive since 3 (no signature changed): qr_rollout_kernel_name (round 4), qr_set_rollout_form (round 5),
                             qr_evaluate_policy (round 8), qr_record_policy / qr_record_row_len (round 9),
                             qr_policy_bank_* / qr_evaluate_policy_bank (round 10),
                             qr_condition_bank_* / qr_evaluate_policy_grid (round 11), qr_rollout_policy_conditions (round 12),
                             qr_blackbox_policy (round 13), qr_rollout_policy_population (round 14),
                             qr_ppo_population_create / _destroy / _epoch / _status (round 15),
                             qr_ppo_population_load_bank / qr_ppo_population_prepare / qr_policy_bank_read (round 16),
                             qr_ppo_population_exploit (round 18), qr_es_* (round 19),
                             qr_dynamics_* / qr_evaluate_policy_dynamics_grid (round 20),
                             qr_rollout_policy_dynamics / qr_vehicle_physical_count / qr_vehicle_bank_sample (round 21),
                             qr_sensing_* / qr_evaluate_policy_sensing_grid (round 22),
                             qr_rollout_policy_sensing (round 23),
                             qr_rollout_policy_history / qr_evaluate_policy_history_grid (round 24),
                             qr_blackbox_policy_grid (round 25),
                             qr_rollout_policy_privileged / qr_ppo_grad_privileged / qr_ppo_minibatch_privileged /
                             qr_ppo_epoch_privileged (round 26) */

enum {
    QR_OK = 0,
    QR_E_INVALID = -1,   /* bad argument */
    QR_E_NO_DEVICE = -2, /* no HIP device / not gfx950 */
    QR_E_HIP = -3,       /* a HIP runtime call failed */
    QR_E_STATE = -4      /* call not valid in the current state (e.g. step before set_track) */
};

enum { QR_VARIANT_E2E = 0, QR_VARIANT_INDI = 1 };

#define QR_MAX_GATES 32
#define QR_MAX_GATES_AHEAD 4
#define QR_RESIDUAL_FLOATS 740 /* 289 thrust + 451 moment */

typedef struct qr_env qr_env;

typedef struct qr_config {
    int32_t variant;            /* QR_VARIANT_E2E | QR_VARIANT_INDI */
    int32_t num_envs;           /* N >= 1 (envs simulated by this handle / this GPU) */
    int32_t gates_ahead;        /* 0..QR_MAX_GATES_AHEAD (R:292) */
    int32_t device;             /* HIP device ordinal */
    int32_t pause_if_collision; /* R:293, R:573-578 */
    int32_t reserved0;
    uint64_t env_id_base;       /* global index of local env 0 (multi-GPU sharding: RNG stream id) */
} qr_config;

int qr_abi_version(void);
const char* qr_last_error(void);

int qr_create(const qr_config* cfg, qr_env** out);
int qr_destroy(qr_env* env);

/* sizes: S (world-state length) and obs_len = S + 4*gates_ahead (+4 disturbance terms for E2E) */
int qr_state_len(const qr_env* env);
int qr_obs_len(const qr_env* env);
int qr_num_envs(const qr_env* env);

/* Host arrays: gate_pos [G][3], gate_yaw [G], start_pos [3]. Computes the relative-gate tables. */
int qr_set_track(qr_env* env, const float* gate_pos, const float* gate_yaw, int32_t num_gates,
                 const float* start_pos);
/* Host outputs (any may be NULL): gate_pos_rel [G][3], gate_yaw_rel [G]. */
int qr_get_track_tables(const qr_env* env, float* gate_pos_rel, float* gate_yaw_rel);

/* Host array of QR_RESIDUAL_FLOATS f32 (thrust W1[32][7] b1[32] W2[1][32] b2[1]; moment W1[32][10]
 * b1[32] W2[3][32] b2[3]) or NULL to disable the residual model (BASELINE config 1). E2E only. */
int qr_set_residual(qr_env* env, const float* blob, size_t n_floats);

/* Host array ranges[6][2] = (min,max) for (Mx,My,Mz,Fx,Fy,Fz); scale = disturbance_scale. E2E only. */
int qr_set_disturbance(qr_env* env, const float* ranges, float scale);

int qr_set_limits(qr_env* env, int32_t max_steps, float dt);
int qr_set_pause(qr_env* env, int32_t pause);
/* env.pause_if_collision after construction (qr_config.pause_if_collision sets the initial value) */
int qr_set_pause_if_collision(qr_env* env, int32_t on);

/* Terminal observations (what SB3 bootstraps time-limit truncations from, `infos[i]["terminal_observation"]`, R:589-594).
 * With a device buffer registered, every env that finishes an episode at a step writes the gate-frame observation of its
 * FINAL state -- taken before the auto-reset -- to row [env] (qr_step: buffer [N][obs_len]) or row [k][env] (qr_step_many,
 * qr_step_launches, qr_rollout_policy: buffer [K][N][obs_len], k = step within the call).  Rows of envs that did not
 * finish are not touched.  NULL (default) switches it off.  `rows` is the leading dimension of the buffer ([rows][N][obs_len];
 * 1 for a plain [N][obs_len] buffer): a K-step call with K > rows fails with QR_E_INVALID instead of writing past the end.
 * (The reference itself hands SB3 the post-reset row, a consequence of filling `infos` after reset_(): see DESIGN.md.) */
int qr_set_terminal_obs(qr_env* env, float* term_obs_dev, int32_t rows);

/* Philox4x32-10 key for the in-kernel reset RNG; also zeroes the per-env episode counters. */
int qr_seed(qr_env* env, uint64_t seed);

/* reset_(mask): mask_dev = NULL resets every env (reset()). Writes the gate-frame observation of ALL
 * envs to obs_out_dev [N][obs_len] (may be NULL). */
int qr_reset(qr_env* env, const uint8_t* mask_dev, float* obs_out_dev, void* stream);

/* One env step for all N envs (one fused kernel): residual MLP -> Euler integration -> reward ->
 * gate pass / collision / ground / bounds / max-steps -> (auto-reset) -> gate-frame observation.
 * trunc_out_dev (may be NULL) receives max_steps_reached per env ("TimeLimit.truncated").
 * With pause set, obs_out_dev is left untouched (the reference does not refresh it, R:570-572). */
int qr_step(qr_env* env, const float* actions_dev, float* obs_out_dev, float* rew_out_dev,
            uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream);

/* K consecutive steps with pre-recorded actions [K][N][4]; outputs are [K][N][...] (trunc may be NULL).
 * Bit-identical to K calls of qr_step, but executed as ONE fused rollout kernel that keeps the env state in
 * registers between steps (no per-step launch, state traffic or end-of-kernel write-back). */
int qr_step_many(qr_env* env, int32_t num_steps, const float* actions_dev, float* obs_out_dev,
                 float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream);

/* The same K steps as K separate step kernels (the kernels K calls of qr_step enqueue, without the per-call FFI cost):
 * the calling pattern of a closed loop whose policy runs between steps.  The K launches are captured once into a
 * hipGraph (K kernel nodes in a chain) and replayed while (K, buffers, env configuration) stay the same: dependent
 * kernel nodes of a graph start ~1 us sooner after each other than dependent launches on a stream. */
int qr_step_launches(qr_env* env, int32_t num_steps, const float* actions_dev, float* obs_out_dev,
                     float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream);

/* update_states(): recompute the observation from the current state. */
int qr_observe(qr_env* env, float* obs_out_dev, void* stream);

/* Diagnostic: out_dev [N][7] = (vbx, vby, vbz, thrust, Mx, My, Mz) -- body velocity (get_body_velocity, R:155) and the
 * residual thrust / moment MLP outputs (thrust_moment_model_world_states, R:254-262) for the CURRENT state of every env,
 * computed by the device functions the step kernels inline.  E2E with residual weights only. */
int qr_probe_residual(qr_env* env, float* out_dev, void* stream);

/* Row-major copies of the internal state (device pointers; any may be NULL).
 * dist is ignored for INDI. target/steps are int32. episode = per-env reset counter (RNG stream position). */
int qr_get_state(qr_env* env, float* world_dev, float* dist_dev, int32_t* target_dev, int32_t* steps_dev,
                 uint32_t* episode_dev, void* stream);
int qr_set_state(qr_env* env, const float* world_dev, const float* dist_dev, const int32_t* target_dev,
                 const int32_t* steps_dev, const uint32_t* episode_dev, void* stream);

/* Timing hooks for benchmarks (both block until the work is done).
 * qr_last_step_many_ms: hipEvent time (ms) from before the first to after the last launch of the most recent
 *   qr_step_many / qr_step_launches call, on its launch stream (back-to-back kernels; rocprofv3 shows no gaps).
 * qr_profile_steps: like qr_step_many, but brackets EVERY step kernel with its own hipEvent pair on the
 *   launch stream and returns the mean single-kernel duration (ms) and the whole-region time (ms). */
int qr_last_step_many_ms(qr_env* env, float* total_ms);
/* The hipEvent bracket behind qr_last_step_many_ms costs two marker packets per K-step call; on = 0 drops it (default: on).
 * It is also skipped, whatever the setting, while the caller is capturing `stream` into a hipGraph. */
int qr_set_timing(qr_env* env, int32_t on);
/* Name of the device kernel a qr_step_many call on this handle launches NOW (it depends on the env count, the variant, the mode
 * flags and whether a terminal-observation buffer is registered), e.g. "rollout_fast_mlp_kernel" -- the symbol rocprofv3 lists as
 * qr::<name><variant, gates_ahead>.  Benchmarks print it so that profiles and counter evidence can be matched to the run. */
const char* qr_rollout_kernel_name(const qr_env* env);
/* Which family of fused kernels qr_step_many may pick from (all produce bit-identical results; this is a testing / A-B hook, there is
 * no environment variable): AUTO = by env count and mode; flags MULTI_WAVE = the forms built for more than
 * one workgroup per CU, at any env count; GENERAL = the general kernels (every mode) for every launch (the two may be or-ed); ONE_WAVE = the forms built for one
 * workgroup per CU at any env count (slower there: profiles/r05_one_wave_ab.txt). */
enum { QR_ROLLOUT_AUTO = 0, QR_ROLLOUT_MULTI_WAVE = 1, QR_ROLLOUT_GENERAL = 2, QR_ROLLOUT_ONE_WAVE = 4 /* the one-wave-per-SIMD forms at any env count */ };
int qr_set_rollout_form(qr_env* env, int32_t form);
int qr_profile_steps(qr_env* env, int32_t num_steps, const float* actions_dev, float* obs_out_dev,
                     float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream,
                     float* mean_kernel_ms, float* region_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Policy network on the matrix cores: the MLP the reference trains and deploys,
 * obs[obs_len] -> 120 -> 120 -> 120 -> 4 with ReLU (SB3 MlpPolicy net_arch pi=[120,120,120], R:783; generated C twin
 * c_code/neural_network.c:397-430 nn_forward).  f16 operands, f32 accumulation.  Replaces `model.predict(env.states,
 * deterministic=True)` (R:801) between env steps without leaving the GPU.
 *   weights: host float32 arrays in torch.nn.Linear layout, w[out][in], b[out].
 *   obs_len: an observation length of the race envs (13 + 4 gates_ahead, 20 + 4 gates_ahead; gates_ahead 0..4) or 16, the raw-state
 *   observation of the predecessor envs (quad3d.h); anything else is QR_E_INVALID.  The same holds for qr_policy_bank_create.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct qr_policy qr_policy;
int qr_policy_create(int32_t obs_len, int32_t device, qr_policy** out);
int qr_policy_destroy(qr_policy* policy);
const char* qr_policy_last_error(void);
int qr_policy_set_weights(qr_policy* policy, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, const float* b3, const float* w4, const float* b4);
/* obs_dev [n][obs_len] row-major -> mean_out_dev [n][4] (action means, i.e. the deterministic action before clipping) */
int qr_policy_forward(qr_policy* policy, int32_t n, const float* obs_dev, float* mean_out_dev, void* stream);
/* The same network at the reference's precision (round 6): both operands of every layer as two f16 pieces (w x ~ W0 X0 + W1 X0 + W0 X1,
 * f32 accumulation on the matrix core: three matrix instructions per K-step) -- float32-class results (max |d mean| vs the reference's
 * generated nn_forward, c_code/neural_network.c:397-430, at the 1e-6 level instead of 7e-4) for evaluation and for precision="f32"
 * collection (its update half is qr_ppo_grad_f32class below); qr_policy_forward stays the throughput path.  Same arguments. */
int qr_policy_forward_f32class(qr_policy* policy, int32_t n, const float* obs_dev, float* mean_out_dev, void* stream);

/* Closed-loop rollout: K steps of  obs -> policy -> a ~ N(mean, exp(log_std)^2) -> env.step(clip(a, -1, 1))  in ONE
 * kernel (PPO's collect phase, R:820 -> SB3 collect_rollouts, without leaving the chip).  Row t of the outputs is
 * (obs_t the action was computed from, unclipped action_t, log-prob_t of that action, reward_t, done_t[, trunc_t]);
 * last_obs_dev [N][obs_len] (may be NULL) receives the observation after the last step (value bootstrap).
 * log_std: host float[4].  Action noise is Philox4x32-10 + Box-Muller keyed by (noise_seed, global env id,
 * first_step + t): pass the number of steps already taken as first_step.  `deterministic` is a set of flags (0 / 1 as before):
 * QR_ROLLOUT_DETERMINISTIC: action = mean; QR_ROLLOUT_F32CLASS (round 6): the policy forward inside the kernel is the reference-precision
 * one of qr_policy_forward_f32class (slower: three matrix instructions per K-step, low-piece weights read from global memory).
 * qr_last_step_many_ms() reports this launch too. */
enum { QR_ROLLOUT_DETERMINISTIC = 1, QR_ROLLOUT_F32CLASS = 2 };
int qr_rollout_policy(qr_env* env, qr_policy* policy, int32_t num_steps, const float* log_std, uint64_t noise_seed,
                      uint64_t first_step, int32_t deterministic, float* obs_out_dev, float* act_out_dev,
                      float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                      float* last_obs_dev, void* stream);

/* Closed-loop EVALUATION of a policy: K steps of  obs -> policy -> env.step(clip(mean, -1, 1))  in ONE kernel that stores nothing per
 * step and keeps the lap / crash accounting in registers -- what a user of the reference does after training (deterministic flight,
 * gate-passage and lap times FP:261-289, crash rate R:4487-4519).  The env state afterwards is the state after K closed-loop steps,
 * bit-identical to qr_rollout_policy(..., QR_ROLLOUT_DETERMINISTIC) with the same K.
 * rec_dev [N][QR_EVAL_REC_INTS] int32 (16-byte aligned), all times in STEPS (seconds = steps * dt):
 *   [0] gate passes counted   [1] crashes (done && !trunc)   [2] time-limit ends (trunc)   [3] passes since this env's last (re)start
 *   [4] step index of its last lap boundary or (re)start     [5] steps evaluated so far (cumulative over calls)
 *   [6..13] sum of lap durations, lap 1..QR_EVAL_MAX_LAPS since a (re)start   [14..21] number of laps counted, lap 1..8   [22], [23] 0
 * Per step: [5] += 1; a PASS is a step that does not end the episode and after which the target gate differs from the one before it
 * (a pass on a finishing step is not counted); on a pass [0] += 1, [3] += 1 and, when [3] is a multiple of gates_per_lap, lap number
 * j = [3] / gates_per_lap is complete: if j <= 8, [5 + j] += [5] - [4] and [13 + j] += 1; then [4] = [5].  On done: [1] or [2] += 1,
 * [3] = 0, [4] = [5].  Lap 1 therefore runs from the (re)start, laps 2.. are flying laps.
 * recf_dev [N][QR_EVAL_REC_FLOATS] float32 (16-byte aligned; may be NULL) = {return of the running episode, sum of the finished
 * episodes' returns, sum of their squares, 0}: sequential float32 adds in step order (the finished episodes number [1] + [2]).
 * Both records are READ at the start of the call and written at its end: zero them for a fresh evaluation, pass them again to
 * continue one (K = 2000 in one call equals 1200 then 800); pass the SAME gates_per_lap when continuing: the running lap's position is
 * re-derived from [3] with the value of the current call.  gates_per_lap is an argument because a track may list its gates more
 * than once (square_track(): 8 rows, a lap is 4 passes).
 * flags: 0 or QR_ROLLOUT_F32CLASS.  QR_E_INVALID: NULL or misaligned record, num_steps < 1, gates_per_lap < 1, another flag, policy
 * obs_len != env obs_len, a track with fewer than two gates (a pass cannot move the target).  QR_E_STATE: pause / pause_if_collision
 * set (evaluation is defined for the default mode), a policy without weights.  A registered terminal-observation buffer is not written.
 * qr_last_step_many_ms() reports this launch too. */
#define QR_EVAL_REC_INTS 24
#define QR_EVAL_MAX_LAPS 8
#define QR_EVAL_REC_FLOATS 4
int qr_evaluate_policy(qr_env* env, qr_policy* policy, int32_t num_steps, int32_t gates_per_lap, int32_t flags,
                       int32_t* rec_dev, float* recf_dev, void* stream);

/* Evaluation of a BANK of policies in one launch, on shared random numbers: what a user holds after a run is many policies (a checkpoint
 * every few rollouts, several seeds), and "which one do I keep?" is one call instead of one qr_evaluate_policy per policy.
 * A bank owns two contiguous device arrays [capacity][image] (the f16 images and the low pieces); qr_policy_bank_set fills slot
 * `slot` in [0, capacity) from the argument layout of qr_policy_set_weights, and the slot's two images are bit-identical to what a
 * qr_policy given the same arrays holds.  It synchronises the device first, like qr_policy_set_weights.
 * qr_evaluate_policy_bank flies slot p, p in [0, num_policies), on envs [p E, (p + 1) E) of the handle, E = envs_per_policy: a 256-env
 * workgroup stages the image of ITS policy.  Records have the layout and semantics of qr_evaluate_policy: rec_dev [N][QR_EVAL_REC_INTS],
 * recf_dev [N][QR_EVAL_REC_FLOATS] (may be NULL), N = num_policies * E, rows [p E, (p + 1) E) belong to policy p; both are read at the start
 * and written at the end, so a call can be continued.  The env state afterwards is the state after num_steps closed-loop steps.
 * GROUP-LOCAL RESET STREAM: inside THIS call an env that ends its episode draws its restart from the Philox stream of env id
 * env_id_base + (i mod E) instead of env_id_base + i (same key, episode counter and block index).  Env j of every group therefore draws
 * the same restart for the same episode number, and group p flies exactly what an E-env handle with the same seed, env_id_base and
 * start state flies under qr_evaluate_policy with the same weights.  This is a property of this call alone: every other entry point on
 * the same handle (qr_reset, qr_step, qr_step_many, qr_rollout_policy, qr_evaluate_policy, qr_record_policy) keeps resetting with the
 * handle's ordinary ids, so qr_reset gives the groups DIFFERENT starts; copy one group's state onto the others (qr_get_state /
 * qr_set_state) for common starts.
 * Refused before anything is launched (qr_last_error / qr_policy_last_error set): everything qr_evaluate_policy refuses; QR_E_INVALID:
 * NULL bank, num_policies < 1 or > capacity, envs_per_policy < 256 or not a multiple of 256, num_policies * envs_per_policy !=
 * qr_num_envs(env), bank obs_len or device differing from the env's; QR_E_STATE: a slot in [0, num_policies) that was never set.
 * qr_last_step_many_ms() reports this launch too. */
typedef struct qr_policy_bank qr_policy_bank;
int qr_policy_bank_create(int32_t obs_len, int32_t device, int32_t capacity, qr_policy_bank** out);
int qr_policy_bank_destroy(qr_policy_bank* bank);
int qr_policy_bank_capacity(const qr_policy_bank* bank);
int qr_policy_bank_set(qr_policy_bank* bank, int32_t slot, const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* w3, const float* b3, const float* w4, const float* b4);
int qr_evaluate_policy_bank(qr_env* env, qr_policy_bank* bank, int32_t num_policies, int32_t envs_per_policy,
                            int32_t num_steps, int32_t gates_per_lap, int32_t flags,
                            int32_t* rec_dev, float* recf_dev, void* stream);

/* Evaluation of a GRID of policies x flight CONDITIONS in one launch: "how does this policy hold up when the conditions are not the ones
 * it trained under?" (other disturbance ranges or scale, another track or start, another time limit) is one call instead of one
 * reconfigured handle per condition, and every cell draws the same random numbers.
 * A condition is what qr_set_track + qr_set_disturbance + the max_steps of qr_set_limits configure on a handle, plus the lap length
 * gates_per_lap.  A condition bank owns one device array [capacity][image]; qr_condition_bank_set fills slot `slot` in [0, capacity)
 * from HOST arrays with the argument layout of those setters: gate_pos [num_gates][3], gate_yaw [num_gates], start_pos [3], dist_ranges
 * [6][2] (lo, hi) or NULL, dist_scale.  The slot's image is a header of the per-condition scalars (num_gates, max_steps, gates_per_lap,
 * the observation scaling of the disturbances) followed by [reset table | gate rows], byte for byte what a handle of the bank's variant
 * holds after the three setters with the same values: the handle and the bank build it with the same host functions.  dist_ranges NULL
 * stands for a handle on which qr_set_disturbance was never called (all-zero ranges, scale 1; dist_scale is ignored); for the INDI
 * variant, which has no disturbances, it must be NULL.  qr_condition_bank_set synchronises the device first, like the setters.
 * QR_E_INVALID: NULL bank or track array, slot outside [0, capacity), num_gates outside 2..QR_MAX_GATES (the evaluators need two gates),
 * gates_per_lap < 1, dist_ranges given for INDI.
 * qr_evaluate_policy_grid: group g in [0, num_groups) = envs [g E, (g + 1) E) of the handle, E = envs_per_group, flies slot
 * policy_of_group[g] of `policies` under slot condition_of_group[g] of `conditions` (two HOST int32 arrays of num_groups entries, any
 * order, repeats allowed).  A 256-env workgroup stages the weight image of ITS policy and the table image of ITS condition; num_gates,
 * max_steps, the observation scaling and gates_per_lap are the condition's.  The residual weights, dt, pause flags and gates_ahead stay
 * the handle's, and the handle's own track / disturbance / max_steps configuration is not used by this call.  Records have the layout
 * and the continue-a-call behaviour of qr_evaluate_policy (rows [g E, (g + 1) E) belong to group g); restarts use the GROUP-LOCAL RESET
 * STREAM of qr_evaluate_policy_bank (env id env_id_base + (i mod E)).
 * CONTRACT: group g flies bit for bit (records and the env state afterwards) what an E-env handle flies under qr_evaluate_policy with
 * the weights of policy policy_of_group[g] and that condition's gates_per_lap, when that handle has been configured by qr_set_track,
 * qr_set_disturbance (not called where the condition's dist_ranges is NULL) and qr_set_limits with the values of condition
 * condition_of_group[g], has the same seed, env_id_base, variant, gates_ahead, residual weights and dt, and starts from the same state.
 * Every cell of a policies x conditions grid therefore sees the same uniform draws; only the condition's own scaling of them differs.
 * The two maps are validated on the host -- no index reaches the device unchecked -- and copied to a device array the handle owns; a
 * map that differs from the previous call's is copied after a device synchronisation (an earlier launch may still read the array).
 * Refused before anything is launched or copied (qr_last_error set, records and state untouched): everything qr_evaluate_policy_bank
 * refuses, with envs_per_group in the role of envs_per_policy (num_groups < 1, num_groups * envs_per_group != qr_num_envs(env), ...);
 * QR_E_INVALID: NULL condition bank or map array, an index outside its bank's capacity, a condition bank of another variant or device;
 * QR_E_STATE: a referenced slot of either bank that was never set, or a new map while `stream` is being captured.
 * qr_last_step_many_ms() reports this launch too. */
typedef struct qr_condition_bank qr_condition_bank;
int qr_condition_bank_create(int32_t variant, int32_t device, int32_t capacity, qr_condition_bank** out);
int qr_condition_bank_destroy(qr_condition_bank* bank);
int qr_condition_bank_capacity(const qr_condition_bank* bank);
int qr_condition_bank_set(qr_condition_bank* bank, int32_t slot, const float* gate_pos, const float* gate_yaw, int32_t num_gates,
                          const float* start_pos, const float* dist_ranges, float dist_scale, int32_t max_steps, int32_t gates_per_lap);
int qr_evaluate_policy_grid(qr_env* env, qr_policy_bank* policies, qr_condition_bank* conditions, int32_t num_groups,
                            int32_t envs_per_group, const int32_t* policy_of_group, const int32_t* condition_of_group,
                            int32_t num_steps, int32_t flags, int32_t* rec_dev, float* recf_dev, void* stream);

/* Evaluation of a grid of policies x flight conditions x VEHICLES in one launch: "which parameter error breaks this policy first, and by
 * how much may the real vehicle differ before lap time or crash rate moves?" (thrust coefficient, drag, motor time constant, inertia, the
 * INDI rate lags) is one call instead of one edited literal and one rebuild per vehicle.  A constant external disturbance of a condition
 * does not cover it: a force offset is not a 15 % error of the thrust coefficient.
 * A vehicle is the coefficient TABLE of the variant's equations of motion, each entry in the form and with the sign in which it enters the
 * arithmetic (the reference's identified parameters, pre-folded; R = "3D quad race.ipynb", I = "3D quad race INDI inner loop.ipynb").
 * E2E, 22 entries (W_i = rotor speed in rpm, w_i = normalised speed, u_i = command, vb = body velocity):
 *    0  motor map gain (w_max - w_min)/2 = 4000                 W_i = [0] w_i + [1]                       R:92-93, 106-109
 *    1  motor map offset (w_max + w_min)/2 = 7000                                                         R:92-93, 106-109
 *    2  -k_x                                                    Fx = [2] vbx sum(W) + F_ext_x             R:78, 125
 *    3  -k_y                                                    Fy = [3] vby sum(W) + F_ext_y             R:79, 126
 *    4  -k_w                                                    T  = [4] sum(W^2) + F_ext_z               R:81, 124
 *    5  -k_z                                                         + [5] vbz sum(W)                     R:80, 124
 *    6  -k_h                                                         + [6] (vbx^2 + vby^2)                R:82, 124
 *    7  g                                                       v' = R (Fx, Fy, T) + (0, 0, [7])          R:73, 138
 *    8  1/Ixx                                                   p' = [8] M_ext_x                          R:74, 144
 *    9  (Iyy - Izz)/Ixx                                              + [9] q r                            R:74-76, 144
 *   10  k_pv/Ixx                                                     + [10] vby                           R:84, 129, 144
 *   11  k_p/Ixx                                                      + [11] (W1^2 - W2^2 - W3^2 + W4^2)   R:83, 129, 144
 *   12  1/Iyy                                                   q' = [12] M_ext_y                         R:75, 145
 *   13  (Izz - Ixx)/Iyy                                              + [13] p r                           R:74-76, 145
 *   14  k_qv/Iyy                                                     + [14] vbx                           R:86, 130, 145
 *   15  k_q/Iyy                                                      + [15] (W1^2 + W2^2 - W3^2 - W4^2)   R:85, 130, 145
 *   16  1/Izz                                                   r' = [16] M_ext_z                         R:76, 146
 *   17  (Ixx - Iyy)/Izz                                              + [17] p q                           R:74-76, 146
 *   18  -k_rr/Izz                                                    + [18] r                             R:89, 131, 146
 *   19  -k_r2 [0] / (tau Izz)                                        + [19] (u1 - u2 + u3 - u4)           R:88, 91, 117-121, 131, 146
 *   20  (k_r2/tau - k_r1) [0] / Izz                                  + [20] (w1 - w2 + w3 - w4)           R:87-88, 91, 131, 146
 *   21  1/tau                                                   w_i' = [21] (u_i - w_i)                   R:91, 112-115
 * INDI, 12 entries:
 *    0  -k_x                                                    Dx = [0] vbx                              I:73, 86
 *    1  -k_y                                                    Dy = [1] vby                              I:74, 87
 *    2  -(T_max - T_min)/2 = -8                                 -T = [2] T_norm + [3]                     I:69-70, 94
 *    3  -(T_max + T_min)/2 = -8                                                                           I:69-70, 94
 *    4  g                                                       v' = R (Dx, Dy, -T) + (0, 0, [4])         I:55, 95
 *    5, 6   -1/tau_p, p_max/tau_p                               p' = [5] p + [6] p_cmd                    I:58, 63-64, 101
 *    7, 8   -1/tau_q, q_max/tau_q                               q' = [7] q + [8] q_cmd                    I:59, 65-66, 102
 *    9, 10  -1/tau_r, r_max/tau_r                               r' = [9] r + [10] r_cmd                   I:60, 67-68, 103
 *   11  1/tau_T                                                 T_norm' = [11] (T_cmd - T_norm)           I:61, 104
 * (the INDI table has no constant term in the rate equations: symmetric rate ranges only.)
 * qr_dynamics_count(variant) = 22 / 12 (QR_E_INVALID for an unknown variant).  qr_dynamics_nominal writes the nominal table -- the very
 * constexpr arrays every kernel of the library is compiled from -- to `out` [count]; host only, no device needed; count must equal
 * qr_dynamics_count(variant).  A dynamics bank owns one device array [capacity][32 floats] (a slot is 128 bytes: the table, then zeros);
 * qr_dynamics_bank_set fills slot `slot` in [0, capacity) from the HOST array coeffs [count], or with the nominal table where coeffs is
 * NULL, after synchronising the device like the other setters; QR_E_INVALID: NULL bank, slot outside the bank, a count other than the
 * variant's, a coefficient that is not finite.  qr_dynamics_bank_read copies a slot's table back to the host (QR_E_STATE: slot never set).
 * qr_evaluate_policy_dynamics_grid is qr_evaluate_policy_grid with the third bank and the third HOST map: group g flies slot
 * policy_of_group[g] of `policies` under slot condition_of_group[g] of `conditions` as the vehicle in slot dynamics_of_group[g] of
 * `dynamics`.  A 256-env workgroup loads its 32-float slot once, ahead of the step loop, through uniform-address loads, and keeps the
 * coefficients in scalar registers: no load of a coefficient inside the loop, no LDS for them.  Everything else -- policy image, condition
 * image, GROUP-LOCAL RESET STREAM, records, continue-a-call behaviour, the copy of the maps to a device array of the handle -- is
 * qr_evaluate_policy_grid's.
 * CONTRACT: (1) a group whose slot holds the nominal table (set from NULL, or from the values qr_dynamics_nominal returns) flies bit for
 * bit what qr_evaluate_policy_grid flies for the same policy and condition from the same state: records, float records, the env state and
 * the observation afterwards.  The runtime form performs the floating-point operations of the literal form in the same order, with every
 * sign in the table.  (2) A group depends on its (policy, condition, dynamics) triple only: the same triple at another group index, or in
 * other slots of the three banks, flies bit for bit the same from the same group-local state; and K steps in one call equal K calls of one
 * step through the same record buffers.
 * NOT modelled: the residual thrust / moment MLPs and the observation are the handle's -- a perturbed vehicle adds the same learned
 * residual and is observed in the same units; there is no scale on the residual.  Observation noise and command delay are the fourth
 * axis of qr_evaluate_policy_sensing_grid (below), which takes a dynamics bank too.
 * Refused before anything is launched or copied (qr_last_error set, records and state untouched): everything qr_evaluate_policy_grid
 * refuses, in its order; and next to the condition bank's refusals the dynamics bank's -- QR_E_INVALID: NULL dynamics bank or map, a
 * dynamics bank of another variant or device, an index outside the bank; QR_E_STATE: a referenced slot that was never set. */
typedef struct qr_dynamics_bank qr_dynamics_bank;
int qr_dynamics_count(int32_t variant);
int qr_dynamics_nominal(int32_t variant, float* out, int32_t count);
int qr_dynamics_bank_create(int32_t variant, int32_t device, int32_t capacity, qr_dynamics_bank** out);
int qr_dynamics_bank_destroy(qr_dynamics_bank* bank);
int qr_dynamics_bank_capacity(const qr_dynamics_bank* bank);
int qr_dynamics_bank_set(qr_dynamics_bank* bank, int32_t slot, const float* coeffs, int32_t count);
int qr_dynamics_bank_read(const qr_dynamics_bank* bank, int32_t slot, float* out, int32_t count);
int qr_evaluate_policy_dynamics_grid(qr_env* env, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                                     int32_t num_groups, int32_t envs_per_group, const int32_t* policy_of_group,
                                     const int32_t* condition_of_group, const int32_t* dynamics_of_group, int32_t num_steps, int32_t flags,
                                     int32_t* rec_dev, float* recf_dev, void* stream);

/* Evaluation of a grid of policies x flight conditions x vehicles x SENSING in one launch: "which sensing error breaks this policy first,
 * and how many control periods of latency can it fly with?"  Every other closed-loop entry point feeds the policy the exact state of the
 * step and applies its command in the same step; on a real vehicle the state comes from an estimator with noise and the command reaches
 * the motors some control periods late.
 * A SENSING SLOT is 32 floats (128 bytes, 16-byte aligned, like a dynamics slot): sigma[0..7], then the command delay as an int32 bit
 * pattern, then zeros.  sigma is indexed by a GROUP of observation entries (S = 16 for E2E, 13 for INDI; GA = gates ahead; L = the
 * observation length), in the units of the observation the policy sees:
 *    0  o[0..2]                    position in the gate frame
 *    1  o[3..5]                    velocity in the gate frame
 *    2  o[6..8]                    roll, pitch, yaw relative to the gate
 *    3  o[9..11]                   body rates
 *    4  o[12..S-1]                 actuator state (motor speeds / T_norm)
 *    5  o[S+4a+0..2], a < GA       relative position of gate a ahead
 *    6  o[S+4a+3]                  relative yaw of gate a ahead
 *    7  o[S+4GA..L-1] (E2E only)   disturbance columns
 * OBSERVATION NOISE: at step t the policy is evaluated on o~[j] = add_rn(o[j], mul_rn(sigma[group(j)], eps[j])) -- two roundings, no
 * FMA.  The env's own observation and state are untouched.  eps[4q..4q+3] is one Philox4x32-10 block with the uniforms and the Box-Muller
 * arithmetic of the action noise (qr_rollout_policy); counter (gid lo, gid hi, step lo, (step hi & 0xFFFFFF) | (q << 24)) with
 * gid = env_id_base + the index of the env WITHIN ITS GROUP (the id of the group-local reset stream: every cell of a grid draws the same
 * eps), step = first_step + t, q < 9; key (noise_seed lo ^ 0x6A09E667, noise_seed hi ^ 0x3C6EF372), distinct from the reset, action-noise
 * and ES keys.  The noise costs ceil(L / 4) Philox blocks per step when it is on; a slot whose eight sigmas are all zero draws nothing and
 * adds nothing (a workgroup-uniform branch): the policy then sees o itself, bit for bit.
 * COMMAND DELAY: d = delay in [0, 4].  a_t = clip(mean_t) is computed from o~_t.  With d = 0 the env steps with a_t; otherwise with the
 * command computed d steps earlier, and with (0, 0, 0, 0) for the first d steps of an episode: the queue of an env is cleared to zeros by
 * the step that ends its episode (auto-reset, crash and time limit alike).  The queue lives across launches in the caller's pending_dev,
 * float [n][16], 16-byte aligned: pending[i][4j..4j+3] is the command computed j + 1 steps ago; entries with j >= d are written as zeros.
 * Zero it when the envs are (re)started.
 * NOT modelled: bias or drift, correlated noise, an estimator that runs slower than the control loop, quantisation; noise on the entries
 * of a command history (qr_rollout_policy_history below: the controller knows its own commands).
 * A sensing bank owns one device array [capacity][32 floats] and belongs to no variant.  qr_sensing_bank_set fills slot `slot` from the
 * HOST array sigma8 [8] (NULL = the ideal sensor: all zeros) and `delay`, after synchronising the device like the other setters;
 * QR_E_INVALID: NULL bank, slot outside the bank, a sigma that is negative or not finite, delay outside [0, 4].  qr_sensing_bank_read
 * copies a slot back (QR_E_STATE: slot never set).
 * qr_evaluate_policy_sensing_grid is qr_evaluate_policy_dynamics_grid with the fourth bank and the fourth HOST map: group g flies through
 * the sensor of slot sensing_of_group[g].  A 256-env workgroup loads its slot once, ahead of the step loop, through uniform-address loads
 * and keeps sigma and d in scalar registers; inside the step loop there is no load of a slot value, no atomic and no global store, and no
 * workgroup waits for another.  Records, restarts, continue-a-call behaviour are qr_evaluate_policy_grid's: K steps in one call equal K
 * calls of one step with first_step advanced, through the same rec, recf and pending.
 * CONTRACT: (1) a group whose slot is ideal (set from NULL) flies bit for bit what qr_evaluate_policy_dynamics_grid flies for the same
 * policy, condition and vehicle from the same state -- records, float records, env state, observation -- and leaves its rows of pending
 * zero.  (2) A group depends on its (policy, condition, dynamics, sensing) quadruple only.
 * qr_sensing_noise writes mul_rn(sigma[group(j)], eps[j]) as rows out_dev [num_steps][envs_per_group][L] for the group-local envs
 * 0..envs_per_group-1 of `env` (its variant, gates_ahead and env_id_base) under slot `slot`: what the evaluator adds to the observations,
 * from the same device function.  An all-zero slot writes +0.0f.  num_steps <= 65535.
 * Refused before anything is launched or copied (qr_last_error set; records, pending, state and output untouched): everything
 * qr_evaluate_policy_dynamics_grid refuses, in its order; then QR_E_INVALID: a NULL sensing bank, map or pending_dev, a misaligned
 * pending_dev, a sensing bank of another device, an index outside the bank, first_step + num_steps > 2^56; QR_E_STATE: a referenced slot
 * that was never set. */
typedef struct qr_sensing_bank qr_sensing_bank;
int qr_sensing_bank_create(int32_t device, int32_t capacity, qr_sensing_bank** out);
int qr_sensing_bank_destroy(qr_sensing_bank* bank);
int qr_sensing_bank_capacity(const qr_sensing_bank* bank);
int qr_sensing_bank_set(qr_sensing_bank* bank, int32_t slot, const float* sigma8, int32_t delay);
int qr_sensing_bank_read(const qr_sensing_bank* bank, int32_t slot, float* sigma8, int32_t* delay);
int qr_evaluate_policy_sensing_grid(qr_env* env, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                                    qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* policy_of_group,
                                    const int32_t* condition_of_group, const int32_t* dynamics_of_group, const int32_t* sensing_of_group,
                                    int32_t num_steps, int32_t flags, uint64_t noise_seed, uint64_t first_step, float* pending_dev,
                                    int32_t* rec_dev, float* recf_dev, void* stream);
int qr_sensing_noise(qr_env* env, qr_sensing_bank* sensing, int32_t slot, int32_t envs_per_group, int32_t num_steps, uint64_t noise_seed,
                     uint64_t first_step, float* out_dev, void* stream);

/* Closed-loop rollout across a MIX of flight conditions in one launch: PPO's collect phase (qr_rollout_policy: same policy forward, same
 * action noise, same rows, terminal-observation rows, last_obs and state write-back) with the group map and the condition bank of
 * qr_evaluate_policy_grid, so that one policy trains on several tracks, disturbance ranges / scales or time limits without one handle
 * and one launch per condition.  Group g in [0, num_groups) = envs [g E, (g + 1) E) of the handle, E = envs_per_group, flies under slot
 * condition_of_group[g] of `conditions` (HOST int32 array of num_groups entries, any order, repeats allowed): a 256-env workgroup stages
 * the table image of ITS condition; num_gates, max_steps and the observation scaling of the disturbances are the condition's (its
 * gates_per_lap is not used).  The residual weights, dt, flags and gates_ahead stay the handle's, and the handle's own track /
 * disturbance / max_steps configuration is not used by this call.  The E2E observation's disturbance terms are therefore normalised
 * by each condition's own ranges, as on a handle configured with it.
 * ORDINARY ENV IDS: unlike the two bank evaluators, the reset stream and the action noise are keyed by env_id_base + i, as in
 * qr_rollout_policy -- training wants independent envs, not common random numbers across groups.
 * CONTRACT: group g produces bit for bit (rows [t][g E, (g + 1) E) of every output, its terminal-observation rows, its last_obs rows
 * and the env state afterwards) what an E-env handle produces under qr_rollout_policy with the same policy, log_std, noise_seed,
 * first_step and flags, when that handle has been configured by qr_set_track, qr_set_disturbance (not called where the condition's
 * dist_ranges is NULL) and qr_set_limits with the values of condition condition_of_group[g], has env_id_base = this handle's + g E,
 * the same seed, variant, gates_ahead, residual weights and dt, and starts from the same state.  COROLLARY: when every group names a
 * condition equal to the handle's own configuration, the call equals qr_rollout_policy on the handle itself, bit for bit.
 * A registered terminal-observation buffer is honoured (num_steps <= its rows, as in every K-step entry point).  The map is validated
 * on the host -- no index reaches the device unchecked -- and copied to the device array the handle owns under the rule of
 * qr_evaluate_policy_grid: a map that differs from the previous call's is copied after a device synchronisation.
 * Refused before anything is launched or copied (qr_last_error set, outputs and state untouched): everything qr_rollout_policy refuses;
 * QR_E_INVALID: NULL condition bank or map, num_groups < 1, envs_per_group < 256 or not a multiple of 256, num_groups * envs_per_group
 * != qr_num_envs(env), an index outside the bank's capacity, a bank of another variant or device; QR_E_STATE: a referenced slot that
 * was never set, pause / pause_if_collision set, or a new map while `stream` is being captured.
 * flags: QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS.  qr_last_step_many_ms() reports this launch too. */
int qr_rollout_policy_conditions(qr_env* env, qr_policy* policy, qr_condition_bank* conditions,
                                 int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group,
                                 int32_t num_steps, const float* log_std, uint64_t noise_seed, uint64_t first_step,
                                 int32_t flags, float* obs_out_dev, float* act_out_dev, float* logp_out_dev,
                                 float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                                 float* last_obs_dev, void* stream);

/* Closed-loop rollout across a MIX of VEHICLES in one launch: qr_rollout_policy_conditions with a dynamics bank and a second HOST map,
 * so that one policy trains on an ensemble of vehicles (domain randomisation over the identified parameters) in one collect launch.
 * Group g additionally flies the coefficients of slot dynamics_of_group[g] of `dynamics` in its equations of motion.  A 256-env
 * workgroup reads its (dynamics, condition) map entry and loads its 32-float slot once, ahead of the step loop, through uniform-address
 * loads, and keeps every coefficient in a scalar register: no load of a coefficient inside the loop, no LDS and no vector register for
 * them.  Everything else -- policy forward, action noise, ORDINARY ENV IDS, condition image, output rows, terminal-observation rows,
 * last_obs, state write-back, the copy of the maps to the device array of the handle -- is qr_rollout_policy_conditions'.
 * CONTRACT: (1) a group whose slot holds the nominal table (set from NULL, or from the values qr_dynamics_nominal returns) produces bit
 * for bit what qr_rollout_policy_conditions produces for that group: every output, the terminal-observation rows, last_obs and the env
 * state afterwards.  (2) Group g of a G-group call equals the one-group call on an E-env handle that has env_id_base = this handle's
 * + g E, is configured with the group's condition and is given the same slot, seed, policy and first_step: rows [t][g E, (g + 1) E) of
 * every output, the terminal-observation rows, last_obs and the env state afterwards, bit for bit.  COROLLARY: K steps in one call equal
 * K calls of one step with first_step advanced.
 * NOT observed: the E2E residual networks and the observation stay the env's; the policy does not see which vehicle it flies.
 * Refused before anything is launched or copied (qr_last_error set, outputs and state untouched): everything
 * qr_rollout_policy_conditions refuses, in its order; then the dynamics bank's refusals as qr_evaluate_policy_dynamics_grid words them --
 * QR_E_INVALID: NULL dynamics bank or map, a dynamics bank of another variant or device, an index outside the bank; QR_E_STATE: a
 * referenced slot that was never set; and last QR_E_STATE for a new pair of maps while `stream` is being captured.
 * flags: QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS.  qr_last_step_many_ms() reports this launch too. */
int qr_rollout_policy_dynamics(qr_env* env, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                               int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group,
                               const int32_t* dynamics_of_group, int32_t num_steps, const float* log_std, uint64_t noise_seed,
                               uint64_t first_step, int32_t flags, float* obs_out_dev, float* act_out_dev, float* logp_out_dev,
                               float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                               float* last_obs_dev, void* stream);

/* Closed-loop rollout under OBSERVATION NOISE and COMMAND DELAY in one launch: qr_rollout_policy_dynamics with a sensing bank, a third
 * HOST map and the command queues, so that a policy trains under the sensor qr_evaluate_policy_sensing_grid measures it with (sensor
 * randomisation: a sensor per group of envs).  Group g additionally flies through slot sensing_of_group[g] of `sensing`; the slot, the
 * sigma groups, the Philox stream and the queue are the ones described at qr_sensing_bank above, from the same device functions.  A
 * 256-env workgroup loads its slot once, ahead of the step loop, and keeps sigma and d in scalar registers; inside the loop there is no
 * load of a slot value and no atomic, and no workgroup waits for another.
 * OBSERVATION NOISE: at call-step k the policy is evaluated on o~[j] = add_rn(o[j], mul_rn(sigma[group(j)], eps[j])), and obs_out[k] holds
 * that NOISY row -- the one act_out[k] and logp_out[k] belong to.  The env's state is untouched.  Counter and key as in the evaluator
 * with step = first_step + k and ONE deliberate difference: gid is the ORDINARY env id env_id_base + i that the reset stream and the
 * action noise of this call use, not the group-local id -- training wants independent envs, not common random numbers across groups.
 * noise_seed keys both streams (each under its own tweak); the action noise is bit for bit qr_rollout_policy_dynamics' for the same
 * noise_seed and first_step.  last_obs_dev carries the noise of call-step num_steps.
 * TERMINAL-OBSERVATION ROWS ARE CLEAN: a registered buffer receives the observation of the terminal state without noise, as in every
 * other entry point.  They feed the time-limit bootstrap only.
 * COMMAND DELAY: the env flies the clipped command computed d steps earlier, (0, 0, 0, 0) for the first d steps of an episode; act_out[k]
 * and logp_out[k] remain this step's unclipped sample and its log-prob, rew_out[k] is the reward of the step flown.  pending_dev is the
 * evaluator's float [n][16], 16-byte aligned, read and written in its canonical order: a buffer passes between the two calls.  Zero it
 * when the envs are (re)started.
 * CONTRACT: (1) a group whose slot is ideal (all sigma 0, d = 0) produces bit for bit what qr_rollout_policy_dynamics produces for that
 * group -- every output, the terminal-observation rows, last_obs and the env state afterwards -- and its rows of pending are written as
 * zeros.  (2) Group g of a G-group call equals the one-group call on an E-env handle that has env_id_base = this handle's + g E, is
 * configured with the group's condition and is given the same slots, seed, policy, first_step and rows of pending.  (3) K steps in one
 * call equal K calls of one step with first_step advanced and pending carried.  (4) last_obs of a call is, bit for bit, row 0 of obs_out
 * of the next call when that call is given first_step + num_steps.  (5) Terminal-observation rows are clean.
 * Refused before anything is launched or copied (qr_last_error set; outputs, pending and state untouched): everything
 * qr_rollout_policy_dynamics refuses, in its order; then the sensing bank's refusals as qr_evaluate_policy_sensing_grid words them --
 * QR_E_INVALID: NULL sensing bank or map, a sensing bank of another device, an index outside the bank, first_step + num_steps >= 2^56;
 * QR_E_STATE: a referenced slot that was never set; then QR_E_INVALID: a NULL or misaligned pending_dev; and last QR_E_STATE for new maps
 * while `stream` is being captured.  The host maps are copied to device arrays the handle owns under the rule of qr_evaluate_policy_grid.
 * flags: QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS.  qr_last_step_many_ms() reports this launch too. */
int qr_rollout_policy_sensing(qr_env* env, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                              qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group,
                              const int32_t* dynamics_of_group, const int32_t* sensing_of_group, int32_t num_steps, const float* log_std,
                              uint64_t noise_seed, uint64_t first_step, int32_t flags, float* pending_dev, float* obs_out_dev,
                              float* act_out_dev, float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                              float* last_obs_dev, void* stream);

/* COMMAND HISTORY: the two sensing calls for a policy that OBSERVES ITS LAST COMMANDS.  Under a command delay of d control steps the env
 * flies the command computed d steps ago while the policy sees only the observation of the step: that observation is no Markov state of
 * the delayed system -- the commands computed and not yet flown are hidden from the network that computed them.  The remedy, for delay
 * and for unknown actuator lag alike, is to append the last few commands to the policy's input; an onboard controller can do the same,
 * because it always knows what it sent.
 * qr_rollout_policy_history is qr_rollout_policy_sensing, and qr_evaluate_policy_history_grid is qr_evaluate_policy_sensing_grid, with
 * `history` = H directly behind sensing_of_group.  DEFINITION (both calls):
 *   RANGE     H in [1, 4 - gates_ahead].  The policy's row at call-step k is [ o~_k | h_k ] of L' = L + 4 H floats, L = qr_obs_len(env).
 *             L + 4 H is the observation length of an env with gates_ahead + H gates ahead, and for gates_ahead + H <= 4 that is a
 *             length every network kernel of the library exists for: `policy` (the bank) is created with obs_len = L', and the policy
 *             forward, the PPO update, the bank loader and ES run on it unchanged.  That is the reason for the bound.
 *   SENSOR    o~_k is exactly what the sensing call feeds: the env's observation with the slot's noise -- stream, key, counter and sigma
 *             groups unchanged.  The noise touches the first L entries only; the history part is exact.
 *   HISTORY   h_k = (u_{k-1}, u_{k-2}, ..., u_{k-H}), newest first, four floats each: the clipped commands COMPUTED at those steps of the
 *             current episode -- the computed ones, not the flown ones -- and zeros for steps before the episode's start.
 *   END       the step that ends an episode clears the history together with the queue: one event.
 *   TERMINAL  rows are L' wide: [ clean observation of the terminal state | u_k, u_{k-1}, ..., u_{k-H+1} ], what the policy would have seen
 *             next had the episode gone on (the first part clean, as in the sensing call).  In qr_rollout_policy_history the buffer
 *             registered with qr_set_terminal_obs is read as [rows][N][L'].  obs_out_dev is [num_steps][N][L'], last_obs_dev [N][L'].
 *   PENDING   pending_dev [n][16] keeps its canonical layout and carries max(d, H) entries: entry j < max(d, H) is the clipped command
 *             computed j + 1 steps ago in this episode, everything behind is zero.  The delay still flies entry d - 1.  d (per group,
 *             from the sensing slot) and H (per launch) are independent.  The buffer passes between all four sensing / history calls.
 * Noise on the history entries is NOT modelled (the list at qr_sensing_bank above).
 * CONTRACT: (1) K steps in one call equal K calls of one step with first_step advanced through the same pending (and rec / recf).
 * (2) A group depends only on its (policy,) condition, dynamics and sensing entries and on H.  (3) The action-noise and observation-noise
 * streams are bit for bit the sensing call's for the same noise_seed and first_step.  (4) The definition above.
 * A 256-env workgroup keeps the slot values in scalar registers; no load of a slot value in the step loop, no atomics, no workgroup that
 * waits for another; LDS within the footprint of the sensing call at gates_ahead = 4.
 * Refused before anything is launched or copied (qr_last_error set; outputs, records, pending and state untouched): everything the sensing
 * twin refuses, in its order, with two changes: QR_E_INVALID for `history` outside [1, 4 - gates_ahead], directly before the
 * observation-length comparison; and that comparison requires the policy's (bank's) obs_len == qr_obs_len(env) + 4 * history. */
int qr_rollout_policy_history(qr_env* env, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                              qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group,
                              const int32_t* dynamics_of_group, const int32_t* sensing_of_group, int32_t history, int32_t num_steps,
                              const float* log_std, uint64_t noise_seed, uint64_t first_step, int32_t flags, float* pending_dev,
                              float* obs_out_dev, float* act_out_dev, float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev,
                              uint8_t* trunc_out_dev, float* last_obs_dev, void* stream);
int qr_evaluate_policy_history_grid(qr_env* env, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                                    qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* policy_of_group,
                                    const int32_t* condition_of_group, const int32_t* dynamics_of_group, const int32_t* sensing_of_group,
                                    int32_t history, int32_t num_steps, int32_t flags, uint64_t noise_seed, uint64_t first_step,
                                    float* pending_dev, int32_t* rec_dev, float* recf_dev, void* stream);

/* PRIVILEGED CRITIC, the collect half: the sensing / history rollout that ALSO stores the row before the sensor's noise.  Under
 * observation noise the policy must read the noisy row, because that is what it will fly on; the value network is never flown -- it is
 * a training device and may read what the simulator knows (asymmetric actor-critic).  Nothing that is evaluated, recorded or exported
 * changes: those paths use the actor only.
 * qr_rollout_policy_privileged is qr_rollout_policy_history with two more device pointers: critic_obs_out_dev directly behind
 * obs_out_dev, critic_last_obs_dev directly behind last_obs_dev.  DEFINITION:
 *   RANGE     `history` = H in [0, 4 - gates_ahead].  H = 0 is the form of qr_rollout_policy_sensing (the TWIN for H = 0), H >= 1 the form of
 *             qr_rollout_policy_history (the twin for H >= 1).  L' = qr_obs_len(env) + 4 H; `policy` has obs_len = L'.
 *   CLEAN ROW critic_obs_out_dev [num_steps][N][L'], 16-byte aligned: row k is c_k = [ o_k | h_k ].  o_k is the env's observation at
 *             call-step k BEFORE the sensor's noise, with the condition's scaling of the disturbance columns as the kernel forms it:
 *             obs_out_dev[k] = [ o~_k | h_k ] is the slot's noise added to exactly this o_k.  h_k is the history tail of the policy's row;
 *             it is exact in both rows.
 *   LAST ROW  critic_last_obs_dev [N][L'] or NULL, 16-byte aligned: [ o_K | h_K ], bit for bit row 0 of critic_obs_out_dev of the next
 *             launch called with first_step + num_steps through the same pending_dev.
 *   IDEAL     a slot with all sigmas zero still gets its clean rows written; they then equal obs_out_dev bit for bit.
 *   TERMINAL  rows are unchanged: they are clean already and serve both networks.
 * CONTRACT: every other output, pending_dev and the env state are bit for bit those of the twin launch with the same arguments, whatever
 * the two new pointers are; the action-noise, observation-noise and reset streams do not move.  K steps in one call equal K calls of one
 * step with first_step advanced through the same pending_dev, the clean rows included.
 * The clean row leaves through the wave's observation tile in LDS in front of the noise: no new LDS, no atomics, no workgroup that waits
 * for another, no load of a slot value in the step loop.
 * Refused before anything is launched or copied (qr_last_error set; outputs, pending and state untouched): everything the twin refuses, in
 * its order; QR_E_INVALID for a NULL or misaligned critic_obs_out_dev (or a misaligned critic_last_obs_dev), directly behind the check of
 * obs_out_dev / act / logp / rew / done; QR_E_INVALID for `history` outside [0, 4 - gates_ahead] where the history call refuses its range. */
int qr_rollout_policy_privileged(qr_env* env, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                                 qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group,
                                 const int32_t* dynamics_of_group, const int32_t* sensing_of_group, int32_t history, int32_t num_steps,
                                 const float* log_std, uint64_t noise_seed, uint64_t first_step, int32_t flags, float* pending_dev,
                                 float* obs_out_dev, float* critic_obs_out_dev, float* act_out_dev, float* logp_out_dev, float* rew_out_dev,
                                 uint8_t* done_out_dev, uint8_t* trunc_out_dev, float* last_obs_dev, float* critic_last_obs_dev, void* stream);

/* Fresh vehicles drawn ON THE DEVICE (the qr_vehicle_* pair works on a qr_dynamics_bank; the qr_dynamics_* names stay the eight entry
 * points of the bank and its table, which work on coefficient tables, while these two work on PHYSICAL parameters): qr_vehicle_bank_sample fills slots [first_slot, first_slot + num_slots) of `bank` with one launch
 * (one thread per slot), so that resampling an ensemble between rollouts makes no qr_dynamics_bank_set calls and reads nothing back.
 * A vehicle is drawn in PHYSICAL parameters and folded into the coefficient table above.  Their order, = qr_vehicle_physical_count:
 *   E2E, 19:   Ixx Iyy Izz k_x k_y k_z k_w k_h k_p k_pv k_q k_qv k_r1 k_r2 k_rr tau w_min w_max g
 *   INDI, 11:  k_x k_y T_max tau_p tau_q tau_r tau_T p_max q_max r_max g          (T_min = 0 and symmetric rate ranges: the table's form)
 * phys_lo / phys_hi: HOST double arrays [count], read during the call.  Physical parameter j of slot s is
 *   lo[j] + (hi[j] - lo[j]) * (double)u,   u = (word >> 8) * 2^-24 in float32,   word = word j % 4 of
 *   Philox4x32-10(counter = (s, j / 4, draw lo, draw hi), key = (seed lo ^ QR_DYNAMICS_SAMPLE_KEY_LO, seed hi ^ QR_DYNAMICS_SAMPLE_KEY_HI)),
 * s the slot's index in the bank (a slot's vehicle does not depend on first_slot), draw a 64-bit counter of the caller (the resample
 * count).  The key tweak differs from the action noise's (0x9E3779B9, 0x85EBCA6B), the ES noise's and the reset stream's (none).  The
 * parameters are folded in float64, every operation rounded on its own (no fused multiply-add) in the order of the table's formulas read
 * left to right -- half = (w_max - w_min) / 2; [1] = half + w_min; [19] = ((-k_r2 * half) / tau) / Izz; [20] = ((k_r2 * half) / tau -
 * k_r1 * half) / Izz -- and rounded ONCE to float32; entries past the variant's count stay zero.  lo == hi == the identified values
 * reproduces the folded reference table.  Slots outside the range are untouched; sampled slots count as set.  Stream-ordered on `stream`;
 * the call does not synchronise (a launch that still reads the bank must be ordered before it by the caller's stream).
 * Refused before anything is launched (QR_E_INVALID): NULL bank or bounds, count != qr_vehicle_physical_count of the bank's variant,
 * first_slot < 0, num_slots < 1 or a range that leaves the bank, a bound that is not finite, lo > hi, lo <= 0 for Ixx, Iyy, Izz, tau
 * (E2E) or tau_p, tau_q, tau_r, tau_T (INDI), hi[w_min] >= lo[w_max]. */
#define QR_DYNAMICS_PHYSICAL_E2E 19
#define QR_DYNAMICS_PHYSICAL_INDI 11
#define QR_DYNAMICS_SAMPLE_KEY_LO 0xC2B2AE35u
#define QR_DYNAMICS_SAMPLE_KEY_HI 0x27D4EB2Fu
int qr_vehicle_physical_count(int32_t variant);
int qr_vehicle_bank_sample(qr_dynamics_bank* bank, int32_t first_slot, int32_t num_slots, const double* phys_lo, const double* phys_hi,
                            int32_t count, uint64_t seed, uint64_t draw, void* stream);

/* Closed-loop rollout for a POPULATION of policies in one launch: qr_rollout_policy_conditions with the policy half of the group map
 * read too and the sampling arguments per group, so that P learners of a seed or hyper-parameter sweep collect in one launch instead
 * of P handles and P launches of a few workgroups each.  Group g in [0, num_groups) = envs [g E, (g + 1) E) of the handle, E =
 * envs_per_group, flies slot policy_of_group[g] of `policies` under slot condition_of_group[g] of `conditions` (HOST int32 arrays of
 * num_groups entries, any order, repeats allowed), sampling with log_std[g] (HOST float [num_groups][4]) and the action-noise key
 * noise_seed[g] (HOST uint64 [num_groups]).  first_step and flags are launch-wide.  A 256-env workgroup stages the weight image of ITS
 * slot and the table image of ITS condition; everything else is qr_rollout_policy_conditions': ORDINARY ENV IDS (reset stream and
 * action noise keyed by env_id_base + i), the same rows, terminal-observation rows, last_obs and state write-back.
 * CONTRACT: group g produces bit for bit (rows [t][g E, (g + 1) E) of every output, its terminal-observation rows, its last_obs rows
 * and the env state afterwards) what an E-env handle produces under qr_rollout_policy with the weights of slot policy_of_group[g],
 * log_std[g], noise_seed[g], the same first_step and flags, when that handle is configured with the values of condition
 * condition_of_group[g] (as in qr_rollout_policy_conditions' contract), has env_id_base = this handle's + g E, the same seed, variant,
 * gates_ahead, residual weights and dt, and starts from the same state.  COROLLARY: with one slot, one log_std and one seed in every
 * group the call equals qr_rollout_policy_conditions with that slot's weights, bit for bit.
 * The map and the per-group sampling values are validated / computed on the host (the values with the arithmetic of
 * qr_rollout_policy) and copied to device arrays the handle owns under the rule of qr_evaluate_policy_grid: contents that differ from
 * the previous call's are copied after a device synchronisation.
 * Refused before anything is launched or copied (qr_last_error set, outputs and state untouched): everything
 * qr_rollout_policy_conditions refuses; everything qr_evaluate_policy_grid refuses about its policy bank (QR_E_INVALID: NULL bank, bank
 * obs_len != qr_obs_len(env), bank on another GPU, an index outside its capacity; QR_E_STATE: a referenced slot without weights);
 * QR_E_INVALID: NULL policy_of_group, log_std or noise_seed; QR_E_STATE: a new map, log_std or noise_seed while `stream` is being
 * captured.
 * flags: QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS.  qr_last_step_many_ms() reports this launch too. */
int qr_rollout_policy_population(qr_env* env, qr_policy_bank* policies, qr_condition_bank* conditions,
                                 int32_t num_groups, int32_t envs_per_group,
                                 const int32_t* policy_of_group, const int32_t* condition_of_group,
                                 int32_t num_steps, const float* log_std, const uint64_t* noise_seed,
                                 uint64_t first_step, int32_t flags, float* obs_out_dev, float* act_out_dev,
                                 float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                                 float* last_obs_dev, void* stream);

/* Closed-loop FLIGHT RECORDER: the K steps of qr_rollout_policy (same policy forward, same action noise keyed by (noise_seed, global env id,
 * first_step + t), same env arithmetic and reset stream: the env state afterwards is bit-identical to qr_rollout_policy with the same
 * arguments) in ONE kernel whose whole per-step output is one packed float32 row per env -- what a user of the reference logs to plot a
 * flight (I:666-695: world_states, the commanded actions and step_counts * dt per step).  No observation, log-prob, reward, done or
 * truncation arrays are written, and no terminal-observation rows.
 * rows_dev [num_steps][rec_envs][R] float32, contiguous, 16-byte aligned, R = qr_record_row_len() = S + QR_RECORD_EXTRA (S = 16 E2E / 13 INDI):
 *   [0, S)      world state BEFORE the step: what qr_get_state would return, the state the action was computed from
 *   [S, S + 4)  the command the env received: clip(action, -1, 1)
 *   [S + 4]     reward of the step
 *   [S + 5]     how the step ended: 0.0 running, 1.0 crash (done && !trunc), 2.0 time limit (trunc) -- the split of qr_evaluate_policy's [1], [2]
 *   [S + 6]     target gate index before the step, as a float
 *   [S + 7]     the env's step count before the step, as a float (exact below 2^24): 0.0 marks the first row of an episode; time = value * dt
 * A row pairs a state with the command applied IN that state.  rec_envs = M, 1 <= M <= N: rows are written for envs [0, M) only, all N envs
 * still fly (the env state afterwards does not depend on M), memory beyond [num_steps][M][R] is never written.  The rows of a full wave
 * (64 consecutive envs below M) leave the chip as one contiguous block of 64 R floats per step.
 * flags: QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS, as in qr_rollout_policy; log_std: host float[4].
 * QR_E_INVALID: NULL policy, log_std or rows_dev, misaligned rows_dev, num_steps < 1, rec_envs outside 1..N, another flag bit, policy
 * obs_len != env obs_len, policy on another GPU.  QR_E_STATE: pause / pause_if_collision set, a policy without weights.  A failed call
 * launches nothing.  A registered terminal-observation buffer is not written.  qr_last_step_many_ms() reports this launch too. */
#define QR_RECORD_EXTRA 8
int qr_record_row_len(const qr_env* env);   /* S + QR_RECORD_EXTRA */
int qr_record_policy(qr_env* env, qr_policy* policy, int32_t num_steps, const float* log_std, uint64_t noise_seed,
                     uint64_t first_step, int32_t flags, int32_t rec_envs, float* rows_dev, void* stream);

/* Closed-loop BLACK BOX: the K steps of qr_record_policy (same forward, noise stream, env arithmetic, reset stream and row layout; the env
 * state afterwards is bit-identical to qr_record_policy / qr_rollout_policy with the same arguments, whatever trigger, window and rec_envs
 * are) in ONE kernel that keeps only the last W = window rows of each env and stops overwriting an env's rows when its episode ends the
 * way `trigger` selects: the seconds before each crash, at W M rows instead of num_steps M.
 * ring_dev [W][rec_envs][R] float32, 16-byte aligned, R = qr_record_row_len(): the row of call-step k of env i goes to
 *   ring_dev[(first_step + k) mod W][i] iff env i was ARMED at the start of that step.  An armed env FREEZES at the end of a step whose end
 *   code (row column S + 5: 1 crash, 2 time limit) has its bit in `trigger` (QR_BLACKBOX_ON_CRASH | QR_BLACKBOX_ON_TIME_LIMIT; 0 never
 *   freezes: the ring is then "the last W steps"), so the triggering row is the last one stored.  A frozen env keeps flying and resetting.
 * st_dev [rec_envs][QR_BLACKBOX_ST_INTS] int32, 16-byte aligned, READ at the start of the call and written at its end: zero it for a fresh
 *   log, pass it again to continue one.  [0] 0 armed / 1 frozen; [1] rows stored for this env so far (cumulative); [2] ring slot of the
 *   trigger row, -1 while armed; [3] cause bits of the trigger step, 0 while armed: 1 ground (z > 0), 2 out of bounds (|x| or |y| > 10 or a
 *   |rate| > 1000), 4 time limit, 8 gate collision (a crash with neither bit 1 nor bit 2), taken from the terminal state.
 *   The valid rows of env i are min(st[1], W) rows that END at slot st[2] if it is frozen, at slot (first_step + num_steps - 1) mod W if it
 *   is armed, oldest first going backwards modulo W.  Slots that hold no valid row were never written.
 * term_dev [rec_envs][S] float32 or NULL: the world state of a frozen env at the END of its trigger step -- after the integration, before
 *   the auto-reset (what the terminal observation is taken from).  Rows of armed envs are not written.
 * CONTINUATION: a second call with first_step advanced by the first call's num_steps, the same window and the same three buffers gives the
 *   ring, status and terminal states of one call over all the steps.
 * Memory beyond [W][rec_envs][R], [rec_envs][4] and [rec_envs][S] is never written; all N envs fly (rec_envs only cuts what is kept).
 * flags, log_std, noise_seed: as in qr_record_policy.  Refused before anything is launched (qr_last_error set, buffers and state untouched):
 * everything qr_record_policy refuses, NULL or misaligned ring_dev / st_dev, trigger outside 0..3, window < 1.  qr_last_step_many_ms()
 * reports this launch too. */
#define QR_BLACKBOX_ST_INTS 4
enum { QR_BLACKBOX_ON_CRASH = 1, QR_BLACKBOX_ON_TIME_LIMIT = 2 };
int qr_blackbox_policy(qr_env* env, qr_policy* policy, int32_t num_steps, const float* log_std, uint64_t noise_seed,
                       uint64_t first_step, int32_t flags, int32_t trigger, int32_t window, int32_t rec_envs, float* ring_dev,
                       int32_t* st_dev, float* term_dev, void* stream);

/* BLACK BOX AND FLIGHT RECORDER OF THE SENSING-GRID EVALUATOR: the launch of qr_evaluate_policy_history_grid with the black box of
 * qr_blackbox_policy riding in its step loop, so that the crash log of a cell belongs to the numbers the evaluator reports for that cell:
 * per group the policy slot, condition, vehicle and sensor, the optional command history, the group-local reset and noise streams and
 * deterministic clip(mean) actions.  A black box that never freezes (trigger 0) with window = num_steps is the flight recorder of a cell.
 * Every argument up to and including recf_dev has the meaning, the order and the refusals of qr_evaluate_policy_history_grid, with one
 * extension: `history` may be 0, the call is then the twin of qr_evaluate_policy_sensing_grid and the bank's obs_len is the env's.
 * CONTRACT (1), the evaluator half: rec_dev, recf_dev, pending_dev and the env state after the call are bit for bit what the evaluator twin
 * produces for the same arguments, whatever trigger, window, rec_per_group and the three black-box buffers are.
 * The black-box half follows qr_blackbox_policy -- row layout R = qr_record_row_len(), status [.][QR_BLACKBOX_ST_INTS], cause bits, trigger
 * bits, armed / frozen rule, continuation rule (consecutive first_step, same window, same buffers and the same pending / rec / recf) --
 * and differs in this:
 *   WHICH ENVS   M = rec_per_group, 1 <= M <= envs_per_group: the first M envs of every group are recorded; env g E + j, j < M, owns column
 *                c = g M + j of ring_dev [W][G M][R], st_dev [G M][4] and term_dev [G M][S] (or NULL), G = num_groups, E = envs_per_group.
 *                All envs fly, and nothing beyond these extents is ever written.
 *   RING SLOT    the row of call-step k goes to slot (first_step + k) mod W; the same first_step advances the sensor's noise stream.
 *   THE ROW UNDER A SENSOR
 *                [0, S)       the TRUE world state before the step (what qr_get_state would return), not the noisy observation
 *                [S, S + 4)   the command the env RECEIVED, the command flown: under a delay d the clipped command computed d steps earlier
 *                             in the episode, zeros for the episode's first d steps
 *                [S + 4 ..)   unchanged: reward of the step flown, end code, target gate before the step, the episode's step count before it
 *                Not recorded: the noisy row the policy saw, the commands computed and not yet flown (they are in pending_dev after the
 *                call), and any stochastic or training-keyed form (ordinary env ids, action noise).
 *   TRIGGER STEP the terminal world state and the cause bits are taken where qr_blackbox_policy takes them, after the integration and before
 *                the auto-reset; the step that freezes an env is also the step that clears its queue and history (the evaluator's one event).
 * A wave's 64 rows leave as one contiguous block iff all its envs lie below M and the block is 16-byte aligned in every group (R % 4 == 0 or
 * M % 4 == 0); otherwise per lane.  No atomics, no workgroup that waits for another, no load of a slot value in the step loop.
 * Refused before anything is launched or copied (qr_last_error set; every buffer and the state untouched): everything
 * qr_evaluate_policy_history_grid refuses, in its order, with `history` checked against [0, 4 - gates_ahead]; then, in qr_blackbox_policy's
 * order and wording, NULL or misaligned ring_dev / st_dev, misaligned term_dev, rec_per_group outside 1..envs_per_group, trigger outside
 * 0..3, window < 1.  qr_last_step_many_ms() reports this launch too. */
int qr_blackbox_policy_grid(qr_env* env, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                            qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* policy_of_group,
                            const int32_t* condition_of_group, const int32_t* dynamics_of_group, const int32_t* sensing_of_group,
                            int32_t history, int32_t num_steps, int32_t flags, uint64_t noise_seed, uint64_t first_step,
                            float* pending_dev, int32_t* rec_dev, float* recf_dev,
                            int32_t trigger, int32_t window, int32_t rec_per_group, float* ring_dev, int32_t* st_dev, float* term_dev,
                            void* stream);

/* ---- PPO minibatch update on the matrix cores (replaces SB3's PPO.train inner loop, R:783-795 / R:820) -------------
 * Networks: policy obs -> 120 -> 120 -> 120 -> 4 and value obs -> 120 -> 120 -> 120 -> 1 (ReLU), log_std[4].
 * Parameters live in ONE flat float32 device vector owned by the caller (torch Linear layouts, w[out][in]):
 *   [ pi: w1 b1 w2 b2 w3 b3 w4 b4 | vf: w1 b1 w2 b2 w3 b3 w4 b4 | log_std[4] ]        (qr_ppo_num_params floats)
 * Loss (SB3): -mean(min(A r, A clip(r, 1-eps, 1+eps))) + vf_coef * mse(v, ret) - ent_coef * mean(entropy), with the
 * advantages of the minibatch normalised to zero mean / unit (unbiased) std; gradients are clipped to max_grad_norm
 * (global L2) and applied with Adam (torch.optim.Adam semantics).  Forward / backward GEMMs use f16 operands with f32
 * accumulation; parameters, gradient accumulation and Adam are f32.
 * Rollout rows (obs [rows][obs_len], act [rows][4], old_logp / adv / ret [rows]) are device arrays; idx_dev[B] selects
 * the rows of this minibatch (64 <= B <= max_minibatch; a last, partial group of 64 rows is masked inside the gradient kernel --
 * the reference's batch_size is 5000, R:792).  obs_len: the lengths qr_policy_create accepts (the race envs' and 16). */
typedef struct qr_ppo qr_ppo;
int qr_ppo_create(int32_t obs_len, int32_t device, int32_t max_minibatch, qr_ppo** out);
/* The same with explicit choices (verification / A-B; qr_ppo_create = flags 0 = the measured-fastest form; the library reads no
 * environment variable): PARTIAL_F32 keeps the per-workgroup gradient partials in f32 instead of bf16 (twice the bytes through the
 * fabric; the form the kernel is verified in to f32 summation noise); NO_EPOCH_GRAPH makes qr_ppo_epoch enqueue plain launches
 * instead of replaying a captured graph.  Any other bit is QR_E_INVALID (bits 2 and 4 selected the round 1-2 forms of the gradient
 * kernel, removed in round 6). */
enum { QR_PPO_PARTIAL_F32 = 1, QR_PPO_NO_EPOCH_GRAPH = 8 };
int qr_ppo_create_ex(int32_t obs_len, int32_t device, int32_t max_minibatch, int32_t flags, qr_ppo** out);
int qr_ppo_destroy(qr_ppo* ppo);
int qr_ppo_num_params(const qr_ppo* ppo);
/* builds the f16 operand images from the parameters: call once before the first qr_ppo_minibatch and after any
 * change of theta made outside this library */
int qr_ppo_pack(qr_ppo* ppo, const float* theta_dev, void* stream);
/* gradient only (no clipping, no optimiser step; the operand images are rebuilt first unless theta_dev is the vector they were
 * last built from / kept in step with): grad_out_dev [num_params + 4] -- the gradient followed by this
 * minibatch's statistics {sum of per-sample surrogate losses, sum of squared value errors, sum of approx-KL terms, number
 * of clipped samples}; stats_dev (may be NULL) float[4] is ACCUMULATED into with the same four sums */
int qr_ppo_grad(qr_ppo* ppo, const float* theta_dev, const float* obs_dev, const float* act_dev,
                const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B,
                float clip, float vf_coef, float ent_coef, float* grad_out_dev, float* stats_dev, void* stream);
/* The same gradient at the reference's precision (round 6): every matrix product of the forward pass, the backward pass and the weight
 * gradients on the matrix core with BOTH operands as three bf16 pieces (x = X0 + X1 + X2 exactly; six matrix instructions per K-step) and f32
 * accumulation, fixed summation order (csrc/quadrace_ppo_f32.hip) -- float32-class like the reference's torch update (R:783-795; cosine against
 * float64 autograd 1 - 1e-13 instead of 0.9985), several times slower than qr_ppo_grad.  Same arguments, same grad_out layout; theta_dev is read
 * directly (no operand images); 2 <= B <= 2 097 120.  Follow with qr_ppo_apply for the step.  Its ~20 launches are replayed as one graph per distinct
 * argument set (up to 256 sets per handle are kept): pass the same buffers from call to call to hit it; QR_PPO_NO_EPOCH_GRAPH or a capturing
 * `stream` gives plain launches. */
int qr_ppo_grad_f32class(qr_ppo* ppo, const float* theta_dev, const float* obs_dev, const float* act_dev,
                         const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B,
                         float clip, float vf_coef, float ent_coef, float* grad_out_dev, float* stats_dev, void* stream);
/* one complete minibatch update of theta (and the Adam moments).  adam_step = 1, 2, ...: the caller counts the updates; adam_step = 0:
 * the library's device-resident count of optimiser steps REALLY taken is used and advanced (launches turned into no-ops by the
 * early stop or a non-finite gradient norm do not count, like torch.optim.Adam under SB3) -- see qr_ppo_adam_step.  lr >= 0 (a
 * negative or NaN learning rate is QR_E_INVALID, here and in qr_ppo_apply / qr_ppo_epoch).
 * Two launches:
 * ONE gradient kernel (forward, loss, backward and the weight gradients of 128 samples per workgroup and pass; per-workgroup
 * partial sums, rounded to bf16 when they leave the workgroup) and ONE kernel that sums the partials in f32 in a fixed order, takes
 * the global norm across a grid-wide barrier, clips, applies Adam and re-packs the f16 operand images.  (Other forms of the kernels: qr_ppo_create_ex.)
 *  A non-finite gradient norm makes
 * the whole update a no-op (counted, see qr_ppo_status).  stats_dev (may be NULL) float[4] is accumulated into. */
int qr_ppo_minibatch(qr_ppo* ppo, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev,
                     const float* act_dev, const float* old_logp_dev, const float* adv_dev, const float* ret_dev,
                     const int32_t* idx_dev, int32_t B, float clip, float vf_coef, float ent_coef, float max_grad_norm,
                     float lr, float beta1, float beta2, float eps, int32_t adam_step, float* stats_dev, void* stream);
/* Announces an epoch: idx_dev [num_minibatches * B] is the permutation whose consecutive slices of B rows will be passed,
 * in order, to qr_ppo_minibatch / qr_ppo_grad.  One launch computes the advantage mean / std sums of every minibatch
 * (otherwise each minibatch call spends a launch on its own).  Optional. */
int qr_ppo_epoch_begin(qr_ppo* ppo, const float* adv_dev, const int32_t* idx_dev, int32_t B, int32_t num_minibatches,
                       void* stream);
/* num_epochs whole epochs: per epoch num_minibatches consecutive qr_ppo_minibatch updates on the rows perm_dev[k B .. (k + 1) B),
 * preceded by the qr_ppo_epoch_begin statistics launch -- enqueued as ONE replayed hipGraph (dependent nodes of a graph start
 * sooner after each other than dependent stream launches, and the host issues one launch instead of 2 num_minibatches + 1 per
 * epoch).  The graph is captured on first use and re-captured when an argument changes.  Uses the device-resident Adam step count
 * (adam_step = 0 semantics) and hands `lr` to the kernels through device memory, so a learning-rate schedule does not force a
 * re-capture.  perm_dev [num_minibatches * B] int32:
 *   device_shuffle == 0: the caller's permutation (num_epochs must be 1; rewrite its CONTENT in place between calls);
 *   device_shuffle != 0: the buffer is FILLED at the start of every epoch with a fresh pseudo-random permutation of
 *     [0, num_minibatches * B) -- a keyed 8-round Feistel bijection, cycle-walked, O(1) per element instead of the radix sort behind
 *     torch.randperm -- keyed by (seed, number of epochs shuffled so far), see qr_ppo_shuffle_state. */
int qr_ppo_epoch(qr_ppo* ppo, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev, const float* act_dev,
                 const float* old_logp_dev, const float* adv_dev, const float* ret_dev, int32_t* perm_dev, int32_t B,
                 int32_t num_minibatches, int32_t num_epochs, int32_t device_shuffle, float clip, float vf_coef, float ent_coef,
                 float max_grad_norm, float lr, float beta1, float beta2, float eps, float* stats_dev, void* stream);
/* state2[0] = seed of the on-device permutations, state2[1] = epochs shuffled so far; set == 0 reads, set != 0 writes.  Blocks. */
int qr_ppo_shuffle_state(qr_ppo* ppo, uint64_t* state2, int32_t set, void* stream);
/* device-resident optimiser step count: set == 0 reads it into *value (for a checkpoint), set != 0 writes *value (after loading
 * one).  Blocks. */
int qr_ppo_adam_step(qr_ppo* ppo, int32_t* value, int32_t set, void* stream);
/* SB3's `target_kl` early stop, decided on the device: before an optimiser step is taken the update kernel compares the
 * minibatch's mean approx-KL with 1.5 * target_kl; if it is larger the step is NOT taken and a sticky stop flag makes every
 * later qr_ppo_minibatch / qr_ppo_apply launch a no-op, until qr_ppo_control(..., clear != 0) (call it at the start of
 * each PPO.train()).  target_kl <= 0 disables the check.  No host synchronisation is involved. */
int qr_ppo_control(qr_ppo* ppo, float target_kl, int32_t clear, void* stream);
/* blocks; out4 = {stopped (0/1), optimiser steps taken since the last clear, updates skipped for a non-finite gradient
 * norm, grid-barrier timeouts (must be 0)} */
int qr_ppo_status(qr_ppo* ppo, int32_t* out4, void* stream);

/* forward pass of one network with the current operand images (net 0: action means; net 1: value in column 0): out_dev [n][4] */
int qr_ppo_forward(qr_ppo* ppo, int32_t net, int32_t n, const float* obs_dev, float* out_dev, void* stream);
/* GAE(lambda) over a rollout buffer [T][N] (SB3 RolloutBuffer.compute_returns_and_advantage; done = 0 / 1 floats).
 * term_val_dev (may be NULL) [T][N] = V(terminal observation) at the steps that ended by the time limit and 0 elsewhere:
 * gamma * term_val is added to those rewards, which is how SB3's collect_rollouts bootstraps truncated episodes (R:589-594
 * hands it `terminal_observation` / `TimeLimit.truncated`); without it truncations count as terminations.  When ep_*_dev are
 * given, the running episode return / length / gate count per env are updated (from the raw rewards) and the sums over finished
 * episodes ACCUMULATED into fin_dev[4] = {sum return, sum length, sum gates, episodes} (VecMonitor, R:769) */
int qr_ppo_gae(qr_ppo* ppo, int32_t T, int32_t N, const float* rew_dev, const float* done_dev, const float* val_dev,
               const float* last_val_dev, const float* term_val_dev, float gamma, float lam, float* adv_out_dev,
               float* ret_out_dev, float* ep_ret_dev, float* ep_len_dev, float* ep_gates_dev, float* fin_dev, void* stream);
/* data-parallel training (one process per GPU): each rank computes qr_ppo_grad on its own rows, the caller averages the
 * [num_params + 4] vector across ranks (a single all-reduce of ~250 KB over RCCL: gradient AND minibatch statistics), then
 * every rank applies the identical update: global-norm clip, Adam, operand re-pack -- and takes the identical target-KL
 * decision, because the KL sum travelled with the gradient.  B = rows per rank of this minibatch.  stats_dev as above.
 * adam_step as in qr_ppo_minibatch (0 = the device-resident count). */
int qr_ppo_apply(qr_ppo* ppo, float* theta_dev, float* adam_m_dev, float* adam_v_dev, float* grad_dev, int32_t B,
                 float max_grad_norm, float lr, float beta1, float beta2, float eps, int32_t adam_step, float* stats_dev,
                 void* stream);

/* PRIVILEGED CRITIC, the update half: the three update calls whose VALUE network reads rows of its own.  Each is its twin -- qr_ppo_grad,
 * qr_ppo_minibatch, qr_ppo_epoch -- with `const float* critic_obs_dev` directly behind obs_dev.  DEFINITION:
 *   ROWS      critic_obs_dev [rows][obs_len], indexed by the same idx_dev / perm_dev as obs_dev.  The policy network's workgroups gather
 *             their rows from obs_dev, the value network's workgroups from critic_obs_dev.  Everything else is the twin's: advantage
 *             statistics, loss, clip, partials (bf16 or QR_PPO_PARTIAL_F32), apply kernel, Adam, re-pack, early stop, non-finite guard,
 *             device shuffle, epoch graph (QR_PPO_NO_EPOCH_GRAPH honoured; critic_obs_dev is part of the graph's key).
 *   SPLIT     qr_ppo_grad_privileged(obs = A, critic_obs = C): the policy network's entries of grad_out_dev (the four log_std entries
 *             included) and statistics [0], [2], [3] are bit for bit those of qr_ppo_grad(obs = A); the value network's entries and
 *             statistic [1] are bit for bit those of qr_ppo_grad(obs = C).
 *   TWIN      with critic_obs_dev a different buffer of the same content as obs_dev, each call leaves grad_out, theta, both Adam moments,
 *             both operand images, the status quadruple, stats, the Adam step count and the shuffle state bit for bit where its twin does.
 *   COMPOSE   qr_ppo_minibatch_privileged = qr_ppo_grad_privileged + qr_ppo_apply; qr_ppo_epoch_privileged = the per-minibatch calls on
 *             the permutation the buffer holds, replayed graph or plain launches.
 * Refused (QR_E_INVALID, nothing launched): a NULL critic_obs_dev, then everything the twin refuses, in its order.  The f32-class gradient
 * (qr_ppo_grad_f32class) and the population update have no privileged form. */
int qr_ppo_grad_privileged(qr_ppo* ppo, const float* theta_dev, const float* obs_dev, const float* critic_obs_dev, const float* act_dev,
                           const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B,
                           float clip, float vf_coef, float ent_coef, float* grad_out_dev, float* stats_dev, void* stream);
int qr_ppo_minibatch_privileged(qr_ppo* ppo, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev,
                                const float* critic_obs_dev, const float* act_dev, const float* old_logp_dev, const float* adv_dev,
                                const float* ret_dev, const int32_t* idx_dev, int32_t B, float clip, float vf_coef, float ent_coef,
                                float max_grad_norm, float lr, float beta1, float beta2, float eps, int32_t adam_step, float* stats_dev,
                                void* stream);
int qr_ppo_epoch_privileged(qr_ppo* ppo, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev,
                            const float* critic_obs_dev, const float* act_dev, const float* old_logp_dev, const float* adv_dev,
                            const float* ret_dev, int32_t* perm_dev, int32_t B, int32_t num_minibatches, int32_t num_epochs,
                            int32_t device_shuffle, float clip, float vf_coef, float ent_coef, float max_grad_norm, float lr, float beta1,
                            float beta2, float eps, float* stats_dev, void* stream);

/* ---- the update of a POPULATION of learners: one minibatch of all members in three launches -------------------------------------
 * A population object BORROWS num_members existing qr_ppo handles (1..256; it does not own them: destroy it before them) that share
 * obs_len, device and creation flags.  ALL per-member state stays in the member's handle -- operand images, stop flag, Adam step count,
 * learning rate, shuffle seed and count, target_kl (qr_ppo_control), partial buffers -- so a member can be read and checkpointed
 * (qr_ppo_adam_step, qr_ppo_shuffle_state, qr_ppo_status) and trained alone again (qr_ppo_epoch, qr_ppo_minibatch) afterwards; the
 * object itself owns a device-resident table of the members' arguments and a scratch area.
 * qr_ppo_population_epoch: for every member p what qr_ppo_epoch(members[p], args[p]..., B, num_minibatches, num_epochs, device_shuffle, ...,
 * stream) does -- args is a HOST array [num_members] of the arguments qr_ppo_epoch takes per handle; stats_dev may be NULL, nothing
 * else -- but one minibatch of ALL members is three launches (csrc/quadrace_ppo_population.hip): a gradient kernel over (workgroups, 2
 * nets, members), a reduce kernel and a step kernel over (247, members).  No kernel waits for another workgroup: the kernel boundary
 * between reduce and step replaces the single-member apply kernel's grid barrier, so the members' barrier counters are never touched
 * (qr_ppo_status's fourth value stays what it was).  The per-epoch launches (permutation, advantage sums) are issued once per member.
 * CONTRACT: afterwards every member is bit for bit where qr_ppo_epoch on that handle with that member's arguments leaves it: theta,
 * both Adam moments, the operand images, the Adam step count, the status quadruple, the shuffle state, the content of perm_dev and
 * stats_dev.  Same operations in the same order; the members do not influence each other (one member's early stop or non-finite
 * gradient leaves the others untouched).
 * Like qr_ppo_epoch the launches of a call are ONE linear captured hipGraph, cached while the argument set stays the same (every
 * pointer and scalar of args except lr, B, the counts, device_shuffle, the members' shuffle seeds and target_kl); each member's lr reaches
 * the device in the arguments of one small kernel, so a schedule does not force a re-capture.  Members created with
 * QR_PPO_NO_EPOCH_GRAPH get plain launches.  A changed argument set is uploaded with a stream-ordered copy and ONE synchronisation of `stream`.
 * Refused before anything is launched (QR_E_INVALID, qr_last_error set, all buffers untouched): create -- NULL members / out, a NULL or
 * repeated handle, num_members outside 1..256, members that differ in obs_len, device or flags; epoch -- NULL pop / args, B < 64 or above
 * any member's max_minibatch, num_minibatches or num_epochs outside qr_ppo_epoch's ranges, num_epochs > 1 without device_shuffle, a NULL
 * member pointer other than stats_dev, a negative or NaN lr, and a `stream` that is being captured by the caller (the call uploads and
 * synchronises, and launches a graph of its own: it cannot become nodes of another graph; no caller in this repository needs that).
 * qr_ppo_population_status: out [num_members][4], row p as qr_ppo_status(members[p]); blocks once for all members.
 * The f32-class gradient path and the data-parallel path have no population form. */
typedef struct qr_ppo_population qr_ppo_population;
typedef struct {   /* one member's arguments, the ones qr_ppo_epoch takes */
    float *theta_dev, *adam_m_dev, *adam_v_dev;
    const float *obs_dev, *act_dev, *old_logp_dev, *adv_dev, *ret_dev;
    int32_t* perm_dev;
    float clip, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, eps;
    float* stats_dev;
} qr_ppo_member_args;
int qr_ppo_population_create(qr_ppo* const* members, int32_t num_members, qr_ppo_population** out);
int qr_ppo_population_destroy(qr_ppo_population* pop);
int qr_ppo_population_epoch(qr_ppo_population* pop, const qr_ppo_member_args* args, int32_t B, int32_t num_minibatches,
                            int32_t num_epochs, int32_t device_shuffle, void* stream);
int qr_ppo_population_status(qr_ppo_population* pop, int32_t* out, void* stream);

/* ---- the rest of a population round on the device: bank load, values, sanitising, GAE (csrc/quadrace_population_prepare.hip) ------------
 * Everything between the collect launch (qr_rollout_policy_population) and qr_ppo_population_epoch, for all P members of `pop`, in a fixed
 * number of launches whatever P is, with ONE blocking host read per round.
 * qr_ppo_population_load_bank: ONE launch, grid (ceil(image / 256), P).  Slot first_slot + p of `bank` receives BOTH images of member p's
 * actor -- the f16 image and the low pieces f16(w - f16(clamp w)), saturated to the f16 range, 0 for a NaN weight -- packed on the device
 * from theta_dev[p] (a HOST array [P] of device pointers to the members' flat parameter vectors; the actor is the block at offset 0 of the
 * layout qr_ppo_num_params defines).  CONTRACT: the slot is bit for bit what qr_policy_bank_set writes when given the same eight float
 * arrays.  The slots are marked as set.  No host packing, no copy, no synchronisation: the launch is ordered on `stream` like any other.
 * Refused before anything is launched (QR_E_INVALID): a NULL argument or a NULL entry of theta_dev, a bank whose obs_len or device
 * differs from the population's, first_slot < 0 or first_slot + P > capacity.
 * qr_policy_bank_read: one image of one slot to host memory (which: 0 = the f16 image, 1 = the low pieces; bytes = the image's size, 16
 * bytes per half8 element).  Blocks.  QR_E_INVALID on an unset slot or a wrong byte count.
 * qr_ppo_population_prepare: `sh` describes the outputs of the ONE collect launch, [K][N][...] as qr_rollout_policy_population wrote them;
 * members is a HOST array [P]: member p owns columns [first_env, first_env + E) and its own contiguous [K][E][...] buffers.  Four launches
 * with the member index in the grid -- values (the member's value image, the one qr_ppo_forward(members[p], 1, ...) uses, over its K E
 * rollout rows, its E last_obs rows and, when both term_obs and term_val are given, its K E term_obs rows, read in place), gather +
 * sanitise, GAE + episode state, report -- then one blocking copy of report_host [P][8]: non-finite rows, truncations, sum ep_ret d,
 * sum ep_len d, sum ep_gates d, episodes, sum of the sanitised rewards, 0.  The counts are exact; the sums are double sums of the float
 * per-step terms in a fixed order (lane, wave, workgroup, workgroups in index order): two identical calls report identical bits.
 * CONTRACT: every member buffer ends bit for bit where the composition of the existing calls leaves it: the member's columns copied
 * (done as 0 / 1 float), val = qr_ppo_forward(net 1) of its rows, a row with a non-finite observation, action, log-prob, reward or value
 * written as +0.0 in obs, act, old_logp, rew and val, last_val and term_val = (trunc ? V(term_obs) : 0) with non-finite values replaced by
 * 0, qr_ppo_gae on the sanitised buffers with the member's gamma and lam (term_val NULL: no time-limit bootstrap for this member), adv =
 * ret = 0 on the zeroed rows, ep_ret / ep_len / ep_gates updated by qr_ppo_gae's expressions (all three or none).
 * Plain launches on `stream`: no graph, no atomic, no flag, no workgroup that waits for another.  The member table is device-resident and
 * uploaded with a stream-ordered copy when it changes; the bad-row mask and the workgroup partials live in scratch the population object
 * owns, allocated on first use and regrown when (K, E) ask for more.
 * Refused before anything is launched (QR_E_INVALID, qr_last_error set, all buffers untouched): NULL pop, sh, members or report_host; K < 1;
 * E < 256, E not a multiple of 256, N not a multiple of E; a NULL shared array other than term_obs; a first_env that is not a multiple of E
 * inside [0, N); two members with the same first_env; any NULL member pointer other than term_val, or the three ep_* pointers given only in
 * part; term_val given without sh->term_obs; non-finite gamma or lam; and a `stream` that is being captured by the caller (the call
 * allocates, uploads and blocks on its report: it cannot become nodes of another graph).
 * The f32-class forward has no form here. */
typedef struct {   /* the ONE collect launch's outputs, [K][N][...] as qr_rollout_policy_population wrote them */
    int32_t K, N, E;                       /* E = envs per member, a multiple of 256 */
    const float *obs, *act, *logp, *rew;   /* [K][N][L], [K][N][4], [K][N], [K][N] */
    const uint8_t *done, *trunc;           /* [K][N] */
    const float *last_obs;                 /* [N][L] */
    const float *term_obs;                 /* [K][N][L] or NULL */
} qr_ppo_prepare_shared;
typedef struct {   /* member p: its envs are columns [first_env, first_env + E) of the shared arrays */
    int32_t first_env;
    float gamma, lam;
    float *obs, *act, *old_logp, *rew, *done, *val;   /* the member's own contiguous [K][E][...] buffers (done as 0/1 float) */
    float *term_val;                                   /* [K][E], or NULL: no time-limit bootstrap for this member */
    float *last_val;                                   /* [E] */
    float *adv, *ret;                                  /* [K][E] */
    float *ep_ret, *ep_len, *ep_gates;                 /* [E] running episode state, updated in place (all three or none) */
} qr_ppo_prepare_member;
int qr_ppo_population_load_bank(qr_ppo_population* pop, const float* const* theta_dev, qr_policy_bank* bank, int32_t first_slot, void* stream);
int qr_policy_bank_read(const qr_policy_bank* bank, int32_t slot, int32_t which, void* out_host, size_t bytes);
int qr_ppo_population_prepare(qr_ppo_population* pop, const qr_ppo_prepare_shared* sh, const qr_ppo_prepare_member* members,
                              double* report_host, void* stream);

/* ---- exploit: overwrite members of a population with copies of other members, in one launch (csrc/quadrace_ppo_population.hip) ---------
 * The device half of population-based training.  theta_dev, adam_m_dev, adam_v_dev: HOST arrays [P] of device pointers to the members'
 * flat parameter vectors and Adam moments (as qr_ppo_population_load_bank takes theta_dev).  src_of: HOST array [P]; src_of[p] == p leaves
 * member p alone, any other value s makes p a DESTINATION and s its SOURCE.  log_std_shift: HOST array [P], or NULL for all zeros; only
 * the destinations' entries are used.
 * For every destination p with source s, in ONE launch for all destinations (grid (ceil(n / 256), destinations); no launch at all when
 * there is none): theta[p] <- theta[s], m[p] <- m[s], v[p] <- v[s]; the four log_std entries of theta[p] become
 * theta[s][n - 4 + i] + log_std_shift[p] (one float32 add, also when the shift is 0); both f16 operand images of handle p are rewritten
 * from the new vector, element by element with qr_ppo_pack's gather (padding and the constant-1 bias unit included); PpoCtrl::adam_t of p
 * <- that of s, copied on the device.  Everything else in p's handle stays p's own -- stop flag, applied / skipped counts, barrier words,
 * lr, shuffle seed and count, target_kl, partial buffers, stats_dev -- and so do its rollout buffers and envs.  Members that are not
 * destinations are not touched at all.
 * CONTRACT: afterwards member p is bit for bit where this composition of existing calls leaves it: three hipMemcpy device-to-device copies
 * from s, a float32 add of the shift into the last four entries of theta[p], qr_ppo_pack(p, theta[p]), qr_ppo_adam_step(p, &t_s, set) --
 * theta, both Adam moments, the operand images, the Adam step count, and an untouched status quadruple, shuffle state and stats.  A later
 * qr_ppo_population_epoch or qr_ppo_epoch on any member runs exactly as after the composition, and their cached graphs stay valid: no
 * pointer moved.
 * A plain launch on `stream`: no host read, no graph, no atomic, no flag, no workgroup that waits for another.  Which member takes whom and
 * the shifts ride in the kernel arguments; the table of the members' pointers is device-resident, owned by the population object, and
 * uploaded with a stream-ordered copy and one synchronisation of `stream` when a pointer moved -- in practice by the first call only.
 * Refused before anything is launched (QR_E_INVALID, qr_last_error set, all buffers untouched): a NULL pop, pointer array, array entry
 * or src_of; an index outside [0, P); a source that is itself a destination (src_of[src_of[p]] != src_of[p]: one launch may not read what
 * it writes); a non-finite entry of log_std_shift; and a `stream` that is being captured by the caller. */
int qr_ppo_population_exploit(qr_ppo_population* pop, float* const* theta_dev, float* const* adam_m_dev, float* const* adam_v_dev,
                              const int32_t* src_of, const float* log_std_shift, void* stream);

/* ---- evolution strategies on the policy bank: optimise what the evaluator measures (csrc/quadrace_es.hip) --------------------------------
 * What it replaces: nothing in the reference -- its user trains on the shaped reward and then MEASURES lap time and crash rate.  The
 * integers qr_evaluate_policy_bank counts are not differentiable; ES climbs them directly.  One generation is P = 2 num_pairs antithetic
 * members of ONE actor parameter vector in bank slots, flown by qr_evaluate_policy_bank on common random numbers (its group-local reset
 * stream), scored, and turned into an update -- a fixed number of launches whatever P is.  1 <= num_pairs <= 128 is a DELIBERATE limit:
 * P = 256 is the pointer table of the one bank-load launch, and 256 policies x 256 envs is the 65 536-env launch the evaluators are tuned for.
 * PARAMETER VECTOR: the actor block only, pi: w1 b1 w2 b2 w3 b3 w4 b4 in torch Linear layout, n = qr_es_num_params = 120 L + 29 644
 * floats (a multiple of 4 for every L) -- layout and offset of the first n floats of a qr_ppo parameter vector, so theta_dev may point
 * into a trainer's own vector.  obs_len: what qr_policy_bank_create accepts.
 * THE NOISE (one device function, used by all three kernels): parameters 4q .. 4q + 3 of pair i in generation g come from ONE
 * Philox4x32-10 block x = Philox(counter = (q, i, g lo, g hi), key = (seed lo ^ 0x2545F491, seed hi ^ 0x4F6CDD1D)).  The two tweak
 * constants differ from the reset stream's key (the env seed itself) and from the action noise's 0x9E3779B9 / 0x85EBCA6B, so the three
 * streams never share bits.  Uniforms and Box-Muller are the action noise's: u1 = ((x >> 8) + 1) 2^-24, u2 = (x >> 8) 2^-24,
 * r = fast_sqrt(-2 __logf(u1)), (sin, cos) = qr_sincos(6.283185307179586f * u2); (x0, x1) -> eps[4q] = r cos, eps[4q + 1] = r sin,
 * (x2, x3) -> eps[4q + 2], eps[4q + 3].  Member 2i is theta[j] + (sigma * eps_ij), member 2i + 1 is theta[j] - (sigma * eps_ij): the
 * product and the sum are two separately rounded float32 operations.
 * qr_es_noise: a diagnostic that is also the hook of this spec: eps_dev [num_pairs][n] receives the raw eps.  ONE launch.
 * qr_es_perturb: TWO launches.  theta_pop [P][n] is written (to theta_pop_dev when given, else to scratch the handle owns), then slot
 * first_slot + p of `bank` receives BOTH images of member p, packed by the kernel of qr_ppo_population_load_bank with its table pointed at
 * the rows of theta_pop.  CONTRACT: the slot is bit for bit what qr_policy_bank_set writes when handed member p's float32 parameters --
 * the f16 image (inf beyond the f16 range) and the low pieces f16(w - f16(clamp w)), saturated, 0 for a NaN weight.  The slots are marked
 * as set.  No host packing, no copy, no synchronisation.
 * qr_es_fitness: ONE launch, one workgroup per policy.  Policy p owns rows [p E, (p + 1) E), E = envs_per_policy, of records laid out as
 * qr_evaluate_policy_bank writes them.  summary_dev [P][8] (may be NULL): s0 gate passes, s1 crashes, s2 time-limit ends, s3 lap-1 count,
 * s4 lap-1 steps, s5 flying-lap count (laps 2..8), s6 flying-lap steps -- int64 sums, hence exact in any order, stored as double -- and
 * s7 = the sum over the policy's envs of (double)recf[., 1] + (double)recf[., 0] (0 when recf_dev is NULL), added in ONE fixed order:
 * chunks of 256 envs; inside a chunk a halving tree over x[0..255] (x[t] += x[t + 128], then + 64, ..., + 1, for t below the stride);
 * the chunks' x[0] added in ascending order to a sum that starts at 0.  The score, in double, in the order written, every multiply and
 * add rounded on its own:  F_p = (w_gate s0 + w_crash s1 + w_timeout s2 + w_return s7) / E + w_lap * (s5 > 0 ? s6 / s5 : no_lap_steps).
 * qr_es_update: ONE launch over n / 4 threads; every thread regenerates its num_pairs noise blocks, nothing of size [pairs][n] is read.
 * Utilities u_p from fitness_dev [P]: QR_ES_SHAPE_CENTERED_RANK: rank_p = #{q : F_q < F_p} + #{q < p : F_q == F_p}, where a NaN score
 * ranks below everything and NaNs among themselves by index (ranks by counting: a permutation of 0 .. P - 1),
 * u_p = (float)rank_p / (float)(P - 1) - 0.5f;  QR_ES_SHAPE_NONE: u_p = (float)F_p.  util_dev [P] (may be NULL) receives u.
 * Per pair d_i = u_{2i} - u_{2i+1}; per parameter j, all in float32 and each operation rounded on its own:
 *   g = 0; for i ascending: g = g + d_i * eps_ij;   g = g * (1.0f / ((float)P * sigma));   g = g - weight_decay * theta[j];
 *   m = beta1 * m + (1.0f - beta1) * g;   v = beta2 * v + ((1.0f - beta2) * g) * g;
 *   theta = theta + div_rn(lr * (m * c1), sqrt_rn(v * c2) + eps)                                                        (Adam ASCENT)
 * where div_rn and sqrt_rn are the correctly rounded (IEEE round-to-nearest) float32 quotient and square root -- __fdiv_rn and sqrtf in
 * the kernel; not the __fsqrt_rn of the HIP headers, which expands to the native 1-ulp instruction -- and the bias corrections c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t), t = adam_step >= 1 counted by the caller, computed on the
 * host in double from the float32 betas and passed as float.  CONTRACT: theta, m, v and u end bit for bit where a NumPy float32
 * restatement of these lines, fed with qr_es_noise's eps, leaves them.
 * Plain launches on `stream`: no graph, no atomic, no flag, no workgroup that waits for another, no host read.
 * Refused before anything is launched (QR_E_INVALID, qr_last_error set, all buffers and the bank untouched): a NULL handle or required
 * pointer; num_pairs outside 1..128; an obs_len the bank does not accept; sigma not finite or <= 0; lr negative or NaN; adam_step < 1;
 * an unknown shaping; envs_per_policy < 256 or not a multiple of 256; a bank whose obs_len or device differs from the handle's;
 * first_slot < 0 or first_slot + P > capacity; a rec_dev, eps_dev, theta, moment or theta_pop pointer that is not 16-byte aligned.
 * QR_E_NO_DEVICE from qr_es_create where no gfx950 is visible (no CPU fallback). */
typedef struct qr_es qr_es;
enum { QR_ES_SHAPE_CENTERED_RANK = 0, QR_ES_SHAPE_NONE = 1 };
typedef struct {
    double w_gate, w_crash, w_timeout, w_return, w_lap;   /* weights of s0, s1, s2, s7 (per env) and of the mean flying-lap steps */
    double no_lap_steps;                                   /* stands for the mean flying-lap steps of a policy without a flying lap */
    int32_t reserved[2];                                   /* 0 */
} qr_es_fitness_weights;
int qr_es_create(int32_t obs_len, int32_t device, int32_t num_pairs, qr_es** out);
int qr_es_destroy(qr_es* es);
int qr_es_num_params(const qr_es* es);
int qr_es_noise(qr_es* es, uint64_t seed, uint64_t generation, float* eps_dev, void* stream);
int qr_es_perturb(qr_es* es, const float* theta_dev, float sigma, uint64_t seed, uint64_t generation, qr_policy_bank* bank,
                  int32_t first_slot, float* theta_pop_dev, void* stream);
int qr_es_fitness(qr_es* es, const int32_t* rec_dev, const float* recf_dev, int32_t envs_per_policy, const qr_es_fitness_weights* w,
                  double* summary_dev, double* fitness_dev, void* stream);
int qr_es_update(qr_es* es, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const double* fitness_dev, float sigma, uint64_t seed,
                 uint64_t generation, int32_t shaping, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t adam_step,
                 float* util_dev, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* QUADRACE_H */
