/*
 * quad3d.h -- C ABI (part of libquadrace.so) for the two PREDECESSOR environments of the reference's
 * "3D quad.ipynb" (SURVEY.md section 8(f) #4), on MI355X (gfx950).  Q3: = that notebook (cell numbers).
 *
 *   kind Q3_KIND_HOVER   class Quadcopter3DVec       Q3 cell 6   hover-at-origin task; float64 state/reward
 *                        (the reference allocates np.zeros((N,16)) = float64), float32 actions
 *   kind Q3_KIND_GATES   class Quadcopter3DVecGates  Q3 cell 14  fly the gate sequence once; float32 state,
 *                        the observation is the raw 16-state (no gate frame)
 *
 * What each entry point replaces:
 *   q3_create                  __init__                              Q3 cell 6 / cell 14
 *   q3_set_track               __init__(gates_pos, gate_yaw, start_pos)          cell 14
 *   q3_set_limits              env.max_steps / env.dt                            cell 6, 14
 *   q3_set_thresholds          env.pos_threshold ... rat_threshold               cell 6
 *   q3_seed                    seed() (a no-op upstream; resets draw from NumPy's global generator)
 *   q3_reset                   reset() / reset_(dones)
 *   q3_step                    step_async() + step_wait(): f_func (cell 2) forward-Euler step, reward,
 *                              termination, auto-reset; returns `self.states`
 *   q3_step_many               K x q3_step in one kernel with the state held in registers
 *   q3_rollout_policy          SB3's collect_rollouts() on these envs: K x [policy forward, Gaussian sample, clip, q3_step] in one kernel
 *   q3_evaluate_policy         the loop a user writes after training: fly the deterministic policy, count how the episodes end and how
 *                              long the successful ones take -- one kernel, one 12-int record per env, nothing stored per step
 *   q3_evaluate_policy_bank    the same for many policies (checkpoints of a run) in one launch, every one on the same starts
 *   q3_get_state/q3_set_state  attribute access to env.states / target_gates / step_counts
 *
 * Conventions are those of quadrace.h: 0 on success, QR_E_* (<0) on error with text in qr_last_error();
 * *_dev arguments are DEVICE pointers owned by the caller; `stream` is a hipStream_t as void*; calls enqueue
 * and return; one handle per GPU, not thread-safe; NO CPU fallback.
 *
 * Element type T of states / rewards: double for Q3_KIND_HOVER, float for Q3_KIND_GATES (q3_elem_size()).
 * Layouts are the reference's row-major arrays: states [N][16] T, actions [N][4] float, rewards [N] T, dones [N] u8.
 */
#ifndef QUAD3D_H
#define QUAD3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libquadrace.so is built with -fvisibility=hidden: only what this header declares is exported */
#pragma GCC visibility push(default)

enum { Q3_KIND_HOVER = 0, Q3_KIND_GATES = 1 };

typedef struct q3_env q3_env;

/* env_id_base: global id of this handle's env 0 (keys the reset stream, so shards of one big env agree with it) */
int q3_create(int kind, int num_envs, int device, uint64_t env_id_base, q3_env** out);
int q3_destroy(q3_env* env);
int q3_num_envs(const q3_env* env);
int q3_elem_size(const q3_env* env); /* 8 (hover) or 4 (gates) */

/* host pointers; gate_pos [G][3], gate_yaw [G], G <= 32 (values are rounded to float32 like astype(np.float32)) */
int q3_set_track(q3_env* env, const float* gate_pos, const float* gate_yaw, int num_gates, const float start_pos[3]);
int q3_set_limits(q3_env* env, int max_steps, double dt);
int q3_set_thresholds(q3_env* env, double pos, double vel, double ang, double rat);
int q3_seed(q3_env* env, uint64_t seed);

/* reset_(mask): mask_dev = NULL resets every env (reset()); states_out_dev (may be NULL) receives env.states */
int q3_reset(q3_env* env, const uint8_t* mask_dev, void* states_out_dev, void* stream);

/* one step_wait(); any output pointer may be NULL.  trunc = the envs for which the reference sets
 * infos[i]["TimeLimit.truncated"] (hover: max_steps or out of bounds; gates: max_steps) */
int q3_step(q3_env* env, const float* actions_dev, void* states_out_dev, void* rew_out_dev, uint8_t* done_out_dev,
            uint8_t* trunc_out_dev, void* stream);

/* K steps in one launch: actions [K][N][4]; rew_out [K][N] T and done_out [K][N] (either may be NULL);
 * states_out (may be NULL) = env.states after the last step */
int q3_step_many(q3_env* env, const float* actions_dev, int num_steps, void* rew_out_dev, uint8_t* done_out_dev,
                 void* states_out_dev, void* stream);

/* K steps in one launch WITH what a trainer consumes (round 6): states_steps_out [K][N][16] T = env.states after every step (the
 * array step_wait() returns, Q3:399 / Q3:744: the first state of the next episode for an env that finished), rew_out [K][N] T,
 * done_out / trunc_out [K][N] (the last three may be NULL).  Same results as K x q3_step, bit for bit. */
int q3_rollout(q3_env* env, const float* actions_dev, int num_steps, void* states_steps_out_dev, void* rew_out_dev,
               uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream);

/* Closed-loop rollout: K x [obs = float32(env.states) -> policy (quadrace.h: qr_policy with obs_len 16, 3 x 120 ReLU, on the matrix
 * cores) -> action = mean + exp(log_std) * N(0,1) -> q3_step(clip(action, -1, 1))] in ONE kernel, for either kind.  Bit for bit what K
 * rounds of [qr_policy_forward (or qr_policy_forward_f32class) on the float32 cast of the states, the sampling arithmetic
 * a = fmaf(std, eps, mean), q3_step] give.  The noise stream is qr_rollout_policy's: Philox4x32-10 with counter (global env id lo, hi,
 * step lo, hi), global env id = env_id_base + i, step = first_step + k, key = noise_seed ^ (0x9E3779B9, 0x85EBCA6B); Box-Muller.
 *   flags: QR_ROLLOUT_DETERMINISTIC (action = mean) | QR_ROLLOUT_F32CLASS (the reference-precision forward); log_std: host float[4].
 *   Outputs are float32 / uint8 for BOTH kinds: obs_out [K][N][16] = the observation each action was computed from, act_out [K][N][4]
 *   = the UNCLIPPED action, logp_out [K][N] its log-probability, rew_out [K][N] = (float)reward, done_out / trunc_out [K][N].
 *   term_obs_dev [K][N][16] (may be NULL): row [k][i] receives the float32 cast of the state after the integration and BEFORE the
 *   auto-reset for an env whose step k ended; rows of envs that did not finish are not written.
 *   last_obs_dev [N][16] (may be NULL): float32 cast of env.states after the last step.  states_out_dev [N][16] T (may be NULL): env.states
 *   after the last step in the env's own type, as in q3_step_many.  trunc_out_dev may be NULL.
 * Refused before anything is launched (env state and buffers untouched, text in qr_last_error()).  QR_E_INVALID: a null env, policy,
 * log_std or required output; num_steps < 1; another flag bit; a policy whose obs_len is not 16 or that lives on another device; an
 * obs_out / act_out / term_obs / last_obs / states_out pointer that is not 16-byte aligned.  QR_E_STATE: a policy without weights, a
 * gates env without a track. */
struct qr_policy;
int q3_rollout_policy(q3_env* env, struct qr_policy* policy, int32_t num_steps, const float* log_std, uint64_t noise_seed,
                      uint64_t first_step, int32_t flags, float* obs_out_dev, float* act_out_dev, float* logp_out_dev,
                      float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev, float* term_obs_dev,
                      float* last_obs_dev, void* states_out_dev, void* stream);

/* Closed-loop evaluation: K x [obs = float32(env.states) -> policy -> q3_step(clip(mean, -1, 1))] in ONE kernel with NO store inside the
 * step loop, for either kind: what a user does right after training -- fly the deterministic policy, count how its episodes end, time
 * the ones that succeed.  The env state after the call equals q3_rollout_policy(QR_ROLLOUT_DETERMINISTIC) after the same num_steps.
 *   flags: 0 or QR_ROLLOUT_F32CLASS (the reference-precision forward).
 *   rec_dev [N][Q3_EVAL_REC_INTS] int32, rows 16-byte aligned; READ at the start and written at the end: zero it for a fresh evaluation,
 *   pass it again to continue one.  All times are in steps.
 *     [0] steps evaluated (cumulative)   [1] SUCCESS ends   [2] TIMEOUT ends   [3] OOB ends   [4] GROUND ends (hover: 0)
 *     [5] COLLISION ends (hover: 0)      [6] sum of the lengths of SUCCESS episodes           [7] sum of the lengths of all ended episodes
 *     [8] gate passes on steps that do not end the episode (hover: 0)   [9] shortest SUCCESS episode so far, 0 = none yet   [10], [11] 0
 *   An episode's length is the env's step counter at its end (after the increment, before the reset).  The end causes are exclusive:
 *     hover  SUCCESS = goal reached inside the bounds before the limit (done and no TimeLimit.truncated); else TIMEOUT if the step
 *            counter reached max_steps; else OOB
 *     gates  SUCCESS = final gate passed; else TIMEOUT if max_steps was reached; else GROUND (pre-step z > 0); else OOB (the reference's
 *            pre-step predicate on x, y, p, q, r); else COLLISION
 *   recf_dev [N][Q3_EVAL_REC_FLOATS] float32 (may be NULL), read and written like rec_dev: {return of the running episode, sum of the
 *   returns of the finished episodes, sum of their squares, 0}, sequential float32 sums of (float)reward in step order, no FMA.
 * Refused before anything is enqueued (env state and records untouched, text in qr_last_error()).  QR_E_INVALID: a null env, policy or
 * rec_dev; num_steps < 1; another flag bit; a policy whose obs_len is not 16 or that lives on another device; a rec_dev / recf_dev that
 * is not 16-byte aligned.  QR_E_STATE: a policy without weights, a gates env without a track. */
#define Q3_EVAL_REC_INTS 12
#define Q3_EVAL_REC_FLOATS 4
int q3_evaluate_policy(q3_env* env, struct qr_policy* policy, int32_t num_steps, int32_t flags, int32_t* rec_dev, float* recf_dev,
                       void* stream);

/* The same for a BANK of policies in one launch (quadrace.h: qr_policy_bank_create(16, capacity, ...)): slot p, p < num_policies, flies
 * envs [p E, (p + 1) E), E = envs_per_policy; rows [p E, (p + 1) E) of rec_dev / recf_dev belong to it.  Inside this call an env that
 * ends its episode restarts from the reset stream of its index WITHIN its group (env id = env_id_base + (i mod E)), so groups that start
 * equal see the same starts and restarts, and group p flies bit for bit what an E-env handle with the same seed and env_id_base flies
 * under q3_evaluate_policy with policy p.
 * Refusals as above, and QR_E_INVALID: a null bank; envs_per_policy not a positive multiple of 256; num_policies * envs_per_policy !=
 * num_envs; num_policies above the bank's capacity.  QR_E_STATE: a slot below num_policies that was never set (named in the message). */
struct qr_policy_bank;
int q3_evaluate_policy_bank(q3_env* env, struct qr_policy_bank* bank, int32_t num_policies, int32_t envs_per_policy, int32_t num_steps,
                            int32_t flags, int32_t* rec_dev, float* recf_dev, void* stream);

/* episode counters [N] u32 (the position of each env in its reset stream; q3_seed zeroes them): set_dev (may be NULL) is copied in first,
 * then get_dev (may be NULL) receives them.  With q3_get_state / q3_set_state this is everything a checkpoint needs to resume bit for bit. */
int q3_episode_counts(q3_env* env, uint32_t* get_dev, const uint32_t* set_dev, void* stream);

/* states [N][16] T, target [N] i32 (gates only; ignored / zero for hover), steps [N] i32; any may be NULL */
int q3_get_state(q3_env* env, void* states_dev, int32_t* target_dev, int32_t* steps_dev, void* stream);
int q3_set_state(q3_env* env, const void* states_dev, const int32_t* target_dev, const int32_t* steps_dev, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
