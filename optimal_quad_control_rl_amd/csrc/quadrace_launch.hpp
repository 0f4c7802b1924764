// quadrace_launch.hpp -- the host side every translation unit of libquadrace.so shares: the run-time -> compile-time dispatch of
// (variant, gates_ahead) and of the observation length, the launch of a kernel with dynamic LDS, and the prototypes of the functions
// that are defined in one unit and called from another.  Host code, but included by files that are compiled for both sides: everything
// here is a template, `inline`, or a declaration (nothing is visible outside the library: -fvisibility=hidden, exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>
#include <type_traits>

#include "../../include/quadrace.h"
#include "quadrace_device.hpp"
#include "quadrace_host.hpp"   // set_last_error, QR_HIP, stream_is_capturing
#include "quadrace_policy.hpp"

namespace qr {

inline dim3 grid_for(int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// ---------------------------------------------------------------------------------------------------
// compile-time dispatch: keeps every observation index static (registers, no scratch).  `f` is a generic lambda that receives the
// value(s) as std::integral_constant; the legal values are listed here and nowhere else.
// ---------------------------------------------------------------------------------------------------
// gates_ahead -> f(integral_constant<int, GA>); hipErrorInvalidValue for a value outside 0..4
template <typename F>
hipError_t dispatch_ga(int gates_ahead, F&& f) {
#ifdef QR_GA_ONLY  // developer builds (ISA inspection, tools/phase_probe.py): instantiate one gates_ahead value only
    if (gates_ahead != QR_GA_ONLY) return hipErrorInvalidValue;
    return f(std::integral_constant<int, QR_GA_ONLY>{});
#else
    switch (gates_ahead) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return hipErrorInvalidValue;
    }
#endif
}
// (variant, gates_ahead) -> f(integral_constant<int, V>, integral_constant<int, GA>)
template <typename F>
hipError_t dispatch_vg(int variant, int gates_ahead, F&& f) {
    return dispatch_ga(gates_ahead, [&](auto ga) {
        return variant == kE2E ? f(std::integral_constant<int, kE2E>{}, ga) : f(std::integral_constant<int, kINDI>{}, ga);
    });
}
// command history -> f(integral_constant<int, H>) for 1 <= H <= 4 - GA (quadrace_rollout_history.hip, quadrace_eval_history.hip): the row
// of an env with GA gates ahead and H commands is as long as the row of GA + H gates ahead, a length the network kernels have up to 4;
// hipErrorInvalidValue outside
template <int GA, typename F>
hipError_t dispatch_history(int history, F&& f) {
    if constexpr (GA + 1 <= 4) if (history == 1) return f(std::integral_constant<int, 1>{});
    if constexpr (GA + 2 <= 4) if (history == 2) return f(std::integral_constant<int, 2>{});
    if constexpr (GA + 3 <= 4) if (history == 3) return f(std::integral_constant<int, 3>{});
    if constexpr (GA + 4 <= 4) if (history == 4) return f(std::integral_constant<int, 4>{});
    return hipErrorInvalidValue;
}
// observation length -> f(integral_constant<int, L>): every length the two env variants can produce (gates_ahead 0..4: 13 + 4g, 20 + 4g)
// and 16, the raw-state observation of the predecessor envs (include/quad3d.h).  The caller
// supplies what an illegal length yields: `invalid()` runs only then (it may record an error message).
template <typename F, typename Invalid>
auto dispatch_L(int L, F&& f, Invalid&& invalid) -> decltype(invalid()) {
    switch (L) {
        case 13: return f(std::integral_constant<int, 13>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 17: return f(std::integral_constant<int, 17>{});
        case 21: return f(std::integral_constant<int, 21>{});
        case 25: return f(std::integral_constant<int, 25>{});
        case 29: return f(std::integral_constant<int, 29>{});
        case 20: return f(std::integral_constant<int, 20>{});
        case 24: return f(std::integral_constant<int, 24>{});
        case 28: return f(std::integral_constant<int, 28>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 36: return f(std::integral_constant<int, 36>{});
        default: return invalid();
    }
}

// ---------------------------------------------------------------------------------------------------
// kernels with dynamic LDS.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE property of a kernel, and one process may
// drive handles on several GPUs (include/quadrace.h): the mask of the device ordinals a kernel has been configured on lives HERE, one
// per kernel (per instantiation of configure_dynamic_lds), so a launch site can neither forget it nor share it between two kernels.
// ---------------------------------------------------------------------------------------------------
inline hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes, unsigned long long& done_mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && ((done_mask >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) done_mask |= 1ull << dev;
    return e;
}
// the limit of `Kernel` on the CURRENT device (idempotent; not a stream operation, so it may run before a graph capture)
template <auto Kernel>
hipError_t configure_dynamic_lds(size_t bytes) {
    static unsigned long long configured = 0;   // per device ordinal
    return ensure_dynamic_lds(reinterpret_cast<const void*>(Kernel), bytes, configured);
}
template <auto Kernel, typename... Args>
hipError_t launch_dynamic_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
    if (hipError_t e = configure_dynamic_lds<Kernel>(lds)) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// defined in one translation unit, called from another
// ---------------------------------------------------------------------------------------------------
// quadrace_kernels.hip
hipError_t launch_step(int variant, const Params& P, const float* actions, float* obs, float* rew, uint8_t* done,
                       uint8_t* trunc, hipStream_t st);
const char* rollout_kernel_name(int variant, const Params& P, int form);
hipError_t launch_rollout(int variant, const Params& P, int form, int K, const float* actions, float* obs, float* rew,
                          uint8_t* done, uint8_t* trunc, hipStream_t st);
hipError_t launch_rollout_policy(int variant, const Params& P, const PolicyArgs& A, int K, float* obs, float* act,
                                 float* logp, float* rew, uint8_t* done, uint8_t* trunc, float* last_obs,
                                 hipStream_t st);
hipError_t launch_reset(int variant, const Params& P, const uint8_t* mask, float* obs, hipStream_t st);
hipError_t launch_observe(int variant, const Params& P, float* obs, hipStream_t st);
hipError_t launch_clear_episode(const Params& P, hipStream_t st);
hipError_t launch_residual_probe(const Params& P, float* out, hipStream_t st);
hipError_t launch_get_state(int variant, const Params& P, float* world, float* dist, int32_t* target, int32_t* steps,
                            uint32_t* episode, hipStream_t st);
hipError_t launch_set_state(int variant, const Params& P, const float* world, const float* dist,
                            const int32_t* target, const int32_t* steps, const uint32_t* episode, hipStream_t st);

// quadrace_kernels_mlp.hip: the two fused E2E + residual-MLP rollout kernels (one workgroup per CU / lean form)
hipError_t launch_rollout_mlp(bool lean, const Params& P, int K, const float4* a4, float* obs, float* rew, uint8_t* done,
                              uint8_t* trunc, hipStream_t st);

// quadrace_eval.hip: the closed-loop evaluation kernel (qr_evaluate_policy)
hipError_t launch_eval_policy(int variant, const Params& P, const PolicyArgs& A, int K, int gates_per_lap, int32_t* rec, float* recf,
                              hipStream_t st);

// quadrace_eval_bank.hip: the same for a bank of policies (qr_evaluate_policy_bank): workgroup b flies image b / (envs_per_policy / kBlock)
hipError_t launch_eval_policy_bank(int variant, const Params& P, const half8* bank, const half8* bank_lo, bool f32class, int num_policies,
                                   int envs_per_policy, int K, int gates_per_lap, int32_t* rec, float* recf, hipStream_t st);

// quadrace_eval_grid.hip: a grid of policies x flight conditions (qr_evaluate_policy_grid): the workgroups of group g = b / (envs_per_group /
// kBlock) fly policy map[g].x under condition map[g].y; conds = slot 0 of [capacity][kCondSlotFloats]
hipError_t launch_eval_policy_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const int2* map,
                                   bool f32class, int num_groups, int envs_per_group, int K, int32_t* rec, float* recf, hipStream_t st);

// quadrace_eval_dynamics.hip: the same grid with a third axis, the coefficients of the equations of motion
// (qr_evaluate_policy_dynamics_grid): group g flies policy map[g].x under condition map[g].y as the vehicle of dynamics slot map[g].z
// (map[g].w is not read); dyns = slot 0 of [capacity][kDynSlotFloats].  dynamics_nominal: the variant's nominal table and its length
// (nullptr, 0 for an unknown variant)
hipError_t launch_eval_policy_dynamics_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const float* dyns,
                                            const int4* map, bool f32class, int num_groups, int envs_per_group, int K, int32_t* rec, float* recf,
                                            hipStream_t st);
const float* dynamics_nominal(int variant, int* count);

// quadrace_eval_sensing.hip: the same grid with a fourth axis, observation noise and command delay (qr_evaluate_policy_sensing_grid):
// group g flies policy map[g].x under condition map[g].y as vehicle map[g].z through the sensor of slot map[g].w; sens = slot 0 of
// [capacity][kSensingSlotFloats]; pending = the command queues [n][kSensingQueueFloats].  launch_sensing_noise (qr_sensing_noise): what
// the evaluator adds to the observations of the group-local envs 0..envs_per_group-1 under `slot` (a pointer to the slot itself), rows
// out [K][envs_per_group][obs_len]; K <= 65535
hipError_t launch_eval_policy_sensing_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const float* dyns,
                                           const float* sens, const int4* map, bool f32class, int num_groups, int envs_per_group, int K,
                                           uint64_t noise_seed, uint64_t first_step, float* pending, int32_t* rec, float* recf, hipStream_t st);
hipError_t launch_sensing_noise(int variant, const Params& P, const float* slot, int envs_per_group, int K, uint64_t noise_seed, uint64_t first_step,
                                float* out, hipStream_t st);

// quadrace_rollout_cond.hip: the closed-loop rollout across a mix of flight conditions (qr_rollout_policy_conditions): the workgroups of
// group g fly under condition map[g].y (map[g].x is not read); conds = slot 0 of [capacity][kCondSlotFloats]
hipError_t launch_rollout_policy_cond(int variant, const Params& P, const PolicyArgs& A, const float* conds, const int2* map, int num_groups,
                                      int envs_per_group, int K, float* obs, float* act, float* logp, float* rew, uint8_t* done,
                                      uint8_t* trunc, float* last_obs, hipStream_t st);

// quadrace_rollout_dynamics.hip: the same rollout across a mix of VEHICLES (qr_rollout_policy_dynamics): the workgroups of group g fly
// under condition map[g].y as the vehicle of dynamics slot map[g].x; dyns = slot 0 of [capacity][kDynSlotFloats].  launch_dynamics_sample
// (qr_vehicle_bank_sample): slots [first_slot, first_slot + num_slots) <- vehicles drawn between the HOST bounds lo / hi (already
// validated; the variant's physical count each), one thread per slot, stream-ordered.  dynamics_physical_names: the physical
// parameters of a variant in the header's order and their count (nullptr, 0 for an unknown variant)
hipError_t launch_rollout_policy_dynamics(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const int2* map,
                                          int num_groups, int envs_per_group, int K, float* obs, float* act, float* logp, float* rew, uint8_t* done,
                                          uint8_t* trunc, float* last_obs, hipStream_t st);
hipError_t launch_dynamics_sample(int variant, float* slots, int first_slot, int num_slots, const double* lo, const double* hi, uint64_t seed,
                                  uint64_t draw, hipStream_t st);
const char* const* dynamics_physical_names(int variant, int* count);

// quadrace_rollout_sensing.hip: the vehicle-mix rollout under observation noise and command delay (qr_rollout_policy_sensing): group g
// additionally flies through the sensor of slot sen_map[g]; sens = slot 0 of [capacity][kSensingSlotFloats]; pending = the command
// queues [n][kSensingQueueFloats], read and written; the observation noise is keyed by (noise_seed, ordinary env id, first_step + k)
hipError_t launch_rollout_policy_sensing(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const float* sens,
                                         const int2* map, const int* sen_map, int num_groups, int envs_per_group, int K, uint64_t noise_seed,
                                         uint64_t first_step, float* pending, float* obs, float* act, float* logp, float* rew, uint8_t* done,
                                         uint8_t* trunc, float* last_obs, hipStream_t st);

// quadrace_rollout_history.hip / quadrace_eval_history.hip: the two sensing calls for a policy whose row carries its last `history`
// clipped commands behind the observation (qr_rollout_policy_history, qr_evaluate_policy_history_grid): the sensing call's arguments and
// history in [1, 4 - gates_ahead]; the policy / the bank has obs_len + 4 history inputs, obs / last_obs / the terminal buffer rows of that
// length; pending carries max(delay, history) entries
hipError_t launch_rollout_policy_history(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const float* sens,
                                         const int2* map, const int* sen_map, int history, int num_groups, int envs_per_group, int K,
                                         uint64_t noise_seed, uint64_t first_step, float* pending, float* obs, float* act, float* logp, float* rew,
                                         uint8_t* done, uint8_t* trunc, float* last_obs, hipStream_t st);
// quadrace_rollout_privileged.hip: launch_rollout_policy_history with history in [0, 4 - gates_ahead] (0: the sensing call's launch) that
// also stores the rows a privileged critic reads (qr_rollout_policy_privileged): critic_obs [K][n][obs_len + 4 history] = the row before
// the sensor's noise with the same history tail, 16-byte aligned, required; critic_last_obs [n][obs_len + 4 history] or null
hipError_t launch_rollout_policy_privileged(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const float* sens,
                                            const int2* map, const int* sen_map, int history, int num_groups, int envs_per_group, int K,
                                            uint64_t noise_seed, uint64_t first_step, float* pending, float* obs, float* critic_obs, float* act,
                                            float* logp, float* rew, uint8_t* done, uint8_t* trunc, float* last_obs, float* critic_last_obs,
                                            hipStream_t st);
hipError_t launch_eval_policy_history_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const float* dyns,
                                           const float* sens, const int4* map, int history, bool f32class, int num_groups, int envs_per_group, int K,
                                           uint64_t noise_seed, uint64_t first_step, float* pending, int32_t* rec, float* recf, hipStream_t st);

// quadrace_rollout_population.hip: the closed-loop rollout for a population of policies (qr_rollout_policy_population): the workgroups of
// group g fly policy map[g].x under condition map[g].y and sample with table[g]; A carries the launch-wide step counter, deterministic
// and f32class only.  One entry = the sampling values of one (log_std, noise seed): 32 bytes, read by one scalar load.
struct PopulationEntry {
    float std[4];               // exp(log_std)
    float logp_const;           // -sum(log_std) - 2*log(2*pi)
    uint32_t seed_lo, seed_hi;  // Philox key of the action noise
    uint32_t pad;
};
static_assert(sizeof(PopulationEntry) == 32, "PopulationEntry is the 32-byte device table entry");
// The sampling values of every closed-loop entry point (rollout, condition mix, population, recorder, black box, q3 rollout), computed
// HERE and nowhere else: the tests demand that they agree bit for bit.  The pad stays zero (the table is compared bytewise).
inline PopulationEntry sampling_entry(const float log_std[4], uint64_t noise_seed) {
    PopulationEntry t{};
    float sum_log_std = 0.0f;
    for (int c = 0; c < 4; ++c) {
        t.std[c] = expf(log_std[c]);
        sum_log_std += log_std[c];
    }
    t.logp_const = -sum_log_std - 2.0f * 1.8378770664093453f;  // 4 * 0.5 * log(2*pi)
    // Domain separation: the reset stream is Philox(counter = (env id, episode, block), key = env seed), the action
    // noise Philox(counter = (env id, step), key = noise seed).  With equal seeds the two would share random bits
    // whenever (episode, block) == (step lo, step hi); the noise key is therefore tweaked by a fixed odd constant.
    t.seed_lo = (uint32_t)noise_seed ^ 0x9E3779B9u;
    t.seed_hi = (uint32_t)(noise_seed >> 32) ^ 0x85EBCA6Bu;
    return t;
}
// the sampling fields of a launch's PolicyArgs: the entry, the call's first step and its flags (the weights are the caller's)
inline void set_sampling(PolicyArgs& A, const PopulationEntry& t, uint64_t first_step, int flags) {
    A.f32class = (flags & QR_ROLLOUT_F32CLASS) ? 1 : 0;
    for (int c = 0; c < 4; ++c) A.std[c] = t.std[c];
    A.logp_const = t.logp_const;
    A.seed_lo = t.seed_lo;
    A.seed_hi = t.seed_hi;
    A.step_lo = (uint32_t)first_step;
    A.step_hi = (uint32_t)(first_step >> 32);
    A.deterministic = (flags & QR_ROLLOUT_DETERMINISTIC) ? 1 : 0;
}
hipError_t launch_rollout_policy_population(int variant, const Params& P, const PolicyArgs& A, const half8* bank, const half8* bank_lo,
                                            const float* conds, const int2* map, const PopulationEntry* table, int num_groups, int envs_per_group,
                                            int K, float* obs, float* act, float* logp, float* rew, uint8_t* done, uint8_t* trunc, float* last_obs,
                                            hipStream_t st);

// quadrace_record.hip: the closed-loop flight recorder (qr_record_policy): one packed row per env-step, rows [K][rec_envs][S + 8]
hipError_t launch_record_policy(int variant, const Params& P, const PolicyArgs& A, int K, int rec_envs, float* rows, hipStream_t st);

// quadrace_blackbox.hip: the closed-loop black box (qr_blackbox_policy): the last `window` rows of each env in ring [window][rec_envs][S + 8],
// frozen at the step that ends an episode the way `trigger` selects; slot0 = first_step mod window; st_rec [rec_envs][4]; term may be null
hipError_t launch_blackbox_policy(int variant, const Params& P, const PolicyArgs& A, int K, int rec_envs, int trigger, int window, int slot0,
                                  float* ring, int32_t* st_rec, float* term, hipStream_t st);

// quadrace_blackbox_grid.hip: the black box of the sensing-grid evaluator (qr_blackbox_policy_grid): launch_eval_policy_history_grid's
// arguments with history in [0, 4 - gates_ahead] (0: the sensing grid's launch), then the black box's -- the first rec_per_group envs of every
// group own columns of ring [window][num_groups * rec_per_group][S + 8], st_rec [..][4], term [..][S] or null; slot0 = first_step mod window
hipError_t launch_blackbox_policy_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const float* dyns,
                                       const float* sens, const int4* map, int history, bool f32class, int num_groups, int envs_per_group, int K,
                                       uint64_t noise_seed, uint64_t first_step, float* pending, int32_t* rec, float* recf, int trigger, int window,
                                       int rec_per_group, int slot0, float* ring, int32_t* st_rec, float* term, hipStream_t st);

// quadrace_policy.hip
hipError_t launch_policy(int L, const half8* w, int n, const float* obs, float* mean, hipStream_t st);
hipError_t launch_policy_f32class(int L, const half8* w0, const half8* w1, int n, const float* obs, float* mean, hipStream_t st);
const half8* policy_weights(const qr_policy* p);   // accessors for the closed-loop rollout entry point in quadrace_abi.hip
const half8* policy_weights_lo(const qr_policy* p);
int policy_obs_len(const qr_policy* p);
int policy_device(const qr_policy* p);
const half8* bank_weights(const qr_policy_bank* b);   // the same for a bank of policies (qr_evaluate_policy_bank)
const half8* bank_weights_lo(const qr_policy_bank* b);
int bank_obs_len(const qr_policy_bank* b);
int bank_device(const qr_policy_bank* b);
int bank_capacity(const qr_policy_bank* b);
int bank_first_unset(const qr_policy_bank* b, int num_policies);
bool bank_slot_set(const qr_policy_bank* b, int slot);   // slot in [0, capacity) and filled (qr_evaluate_policy_grid)
half8* bank_weights_mut(qr_policy_bank* b);              // for qr_ppo_population_load_bank: the slots are packed on the device ...
half8* bank_weights_lo_mut(qr_policy_bank* b);
void bank_mark_set(qr_policy_bank* b, int first_slot, int count);   // ... and marked as set on the host

// quadrace_population_prepare.hip: the one launch of the bank-load kernel (qr_ppo_population_load_bank, and qr_es_perturb of quadrace_es.hip):
// slot first_slot + p of (bank, bank_lo) <- both images of the actor block at theta[p], p < P <= 256; a QR_* code, qr_last_error set
int launch_population_load_bank(int L, const float* const* theta, int P, half8* bank, half8* bank_lo, int first_slot, hipStream_t st);

// ---------------------------------------------------------------------------------------------------
// what the entry points of quadrace_abi.hip and quad3d.hip refuse about a policy handle or a bank: observation length, then device.
// `who` names the entry point; a message is built on the failing path only.  `len_rule` completes "policy obs_len " / "bank obs_len ",
// `noun` is what the device message calls the bank.  The weights are fetched by a call of their own: the entry points place that
// refusal differently (before these two in the rollouts, after them everywhere else).
// ---------------------------------------------------------------------------------------------------
inline int check_policy_handle(const qr_policy* p, int obs_len, int device, const char* who, const char* len_rule = "!= env obs_len") {
    if (policy_obs_len(p) != obs_len) return set_last_error(QR_E_INVALID, std::string(who) + ": policy obs_len " + len_rule);
    if (policy_device(p) != device) return set_last_error(QR_E_INVALID, std::string(who) + ": policy on another GPU");
    return QR_OK;
}
inline int fetch_policy_weights(const qr_policy* p, const char* who, const half8*& w) {
    w = policy_weights(p);
    return w ? QR_OK : set_last_error(QR_E_STATE, std::string(who) + ": the policy has no weights");
}
inline int check_policy_bank(const qr_policy_bank* b, int obs_len, int device, const char* who, const char* noun = "policy bank",
                             const char* len_rule = "!= env obs_len") {
    if (bank_obs_len(b) != obs_len) return set_last_error(QR_E_INVALID, std::string(who) + ": bank obs_len " + len_rule);
    if (bank_device(b) != device) return set_last_error(QR_E_INVALID, std::string(who) + ": " + noun + " on another GPU");
    return QR_OK;
}

}  // namespace qr
