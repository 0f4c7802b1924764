// quadrace_rollout_privileged.hip -- PPO's collect phase for a PRIVILEGED CRITIC (qr_rollout_policy_privileged): the launch function, the
// checks and the instantiations of rollout_policy_group_kernel<V, GA, kF32, false, true, RuntimeSensing, H, true>
// (quadrace_rollout_group.hpp, where the kernel and everything about this mode is written down): the sensing mode (H = 0) or the
// command-history mode (H >= 1) of the grouped rollout that also stores the row BEFORE the sensor's noise.
// Why: under observation noise the policy must read the noisy row o~_k, but the value network is a training device that is never flown:
// it may read what the simulator knows (asymmetric actor-critic).  The clean row is in the kernel's registers one statement before the
// noise is added; this mode writes it out instead of dropping it.
// What the rows hold: critic_obs_out[k] = [o_k | h_k], rows of obs_len + 4 H floats, o_k the env's observation at call-step k before the
// noise (condition scaling included), h_k the history tail of the policy's row (exact in both rows); critic_last_obs = [o_K | h_K], bit for
// bit row 0 of critic_obs_out of the next launch called with first_step + K through the same `pending`.  Every other output, `pending`
// and the env state are those of qr_rollout_policy_sensing (H = 0) / qr_rollout_policy_history (H >= 1): the action-noise,
// observation-noise and reset streams do not move.  15 (GA, H) pairs per variant and precision.
// A translation unit of its own, compiled with the flags of quadrace_rollout_sensing.hip (the build's defaults): the code objects of the
// other sources do not change when this one does.
#include "quadrace_rollout_group.hpp"

namespace qr {

// dynamic LDS, as the sensing and history modes carve it: policy image (f16) | reset table | gate rows | observation tiles | command
// queues, at the policy's row length.  The clean row goes through the same tiles: no new LDS.
template <int L>
constexpr size_t rollout_privileged_lds_bytes() {
    return (size_t)PolicyDims<L>::kTotalHalf8 * 16 +
           sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * L + kSensingQueueFloats * kBlock);
}
static_assert(rollout_privileged_lds_bytes<obs_len<kE2E, 4>()>() <= 160 * 1024, "the largest row (36 floats) is the sensing mode's largest: one workgroup per CU");

// dispatch_history with H = 0 (the sensing call's form) in front
template <int GA, typename F>
static hipError_t dispatch_history0(int history, F&& f) {
    if (history == 0) return f(std::integral_constant<int, 0>{});
    return dispatch_history<GA>(history, static_cast<F&&>(f));
}

// the arguments of launch_rollout_policy_history with `history` in [0, 4 - P.gates_ahead], and the two critic buffers: critic_obs
// [K][n][obs_len + 4 history] (required, 16-byte aligned: the caller has checked), critic_last_obs [n][obs_len + 4 history] or null.
// envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n are checked again here: a grid that does not match P.n would read
// and write out of bounds.
hipError_t launch_rollout_policy_privileged(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const float* sens,
                                            const int2* map, const int* sen_map, int history, int num_groups, int envs_per_group, int K,
                                            uint64_t noise_seed, uint64_t first_step, float* pending, float* obs, float* critic_obs, float* act,
                                            float* logp, float* rew, uint8_t* done, uint8_t* trunc, float* last_obs, float* critic_last_obs,
                                            hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !conds || !dyns || !sens || !map || !sen_map || !pending || ((uintptr_t)pending & 15) || K < 1 || !critic_obs ||
        ((uintptr_t)critic_obs & 15) || ((uintptr_t)critic_last_obs & 15))
        return hipErrorInvalidValue;
    const SensingStream stream = sensing_stream(noise_seed, first_step);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        return dispatch_history0<GA>(history, [&](auto h) {
            constexpr int H = decltype(h)::value;
            constexpr size_t lds = rollout_privileged_lds_bytes<obs_len<V, GA + H>()>();
            float4* act4 = reinterpret_cast<float4*>(act);
            const dim3 grid((unsigned)(P.n / kBlock));
            const int wgs = envs_per_group / kBlock;
            const half8* no_bank = nullptr;   // one policy per launch: A.weights / A.weights_lo and A's sampling arguments
            const PopulationEntry* no_table = nullptr;
            if (A.f32class)
                return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, true, false, true, RuntimeSensing, H, true>>(
                    grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map, no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, dyns,
                    sens, sen_map, pending, stream, critic_obs, critic_last_obs);
            return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, false, false, true, RuntimeSensing, H, true>>(
                grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map, no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, dyns, sens,
                sen_map, pending, stream, critic_obs, critic_last_obs);
        });
    });
}

}  // namespace qr
