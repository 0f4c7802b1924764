// quadrace_rollout_sensing.hip -- PPO's collect phase under OBSERVATION NOISE and COMMAND DELAY in one launch (qr_rollout_policy_sensing):
// the launch function and the instantiations of rollout_policy_group_kernel<V, GA, kF32, false, true, RuntimeSensing>
// (quadrace_rollout_group.hpp, where the kernel and everything about this mode is written down): the vehicle mode -- one policy per
// launch, a condition and a vehicle per group of envs, ORDINARY env ids -- with a sensor per group.  The sensor is the sensing-grid
// evaluator's (quadrace_sensing.hpp: slot, stream, sensing_noise4, and the queue layout of eval_policy_body), so a checkpoint is trained
// under what qr_evaluate_policy_sensing_grid measures, and a `pending` buffer passes between the two calls.
// What the rows hold: obs_out[k] is the NOISY row the action was computed from; act_out[k] / logp_out[k] are this step's unclipped sample
// and its log-prob; rew_out[k] is the reward of the step flown (with the command of d steps ago); last_obs carries the noise of call-step
// K.  TERMINAL-OBSERVATION ROWS ARE CLEAN (the observation of the terminal state, as store_terminal_obs writes it in every mode): they
// feed the time-limit bootstrap only, and a second noise draw on divergent lanes is not worth it.
// A translation unit of its own, compiled with the flags of quadrace_rollout_cond.hip and quadrace_rollout_dynamics.hip (the build's
// defaults): the code objects of the other sources do not change when this one does.
#include "quadrace_rollout_group.hpp"

namespace qr {

// dynamic LDS of the sensing mode: policy image (f16) | reset table | gate rows | observation tiles | command queues
template <int L>
constexpr size_t rollout_sensing_lds_bytes() {
    return (size_t)PolicyDims<L>::kTotalHalf8 * 16 +
           sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * L + kSensingQueueFloats * kBlock);
}
static_assert(rollout_sensing_lds_bytes<obs_len<kE2E, 4>()>() <= 160 * 1024, "the largest form (E2E, gates_ahead 4) fits one workgroup per CU");

// conds / dyns / map as launch_rollout_policy_dynamics; sens: [capacity][kSensingSlotFloats] floats; sen_map: [num_groups] sensing slots;
// pending: [n][kSensingQueueFloats], 16-byte aligned; every index of both maps already checked against its bank by the caller.
// envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n are checked again here: a grid that does not match P.n would read
// and write out of bounds.
hipError_t launch_rollout_policy_sensing(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const float* sens,
                                         const int2* map, const int* sen_map, int num_groups, int envs_per_group, int K, uint64_t noise_seed,
                                         uint64_t first_step, float* pending, float* obs, float* act, float* logp, float* rew, uint8_t* done,
                                         uint8_t* trunc, float* last_obs, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !conds || !dyns || !sens || !map || !sen_map || !pending || ((uintptr_t)pending & 15) || K < 1)
        return hipErrorInvalidValue;
    const SensingStream stream = sensing_stream(noise_seed, first_step);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        constexpr size_t lds = rollout_sensing_lds_bytes<obs_len<V, GA>()>();
        float4* act4 = reinterpret_cast<float4*>(act);
        const dim3 grid((unsigned)(P.n / kBlock));
        const int wgs = envs_per_group / kBlock;
        const half8* no_bank = nullptr;   // one policy per launch: A.weights / A.weights_lo and A's sampling arguments
        const PopulationEntry* no_table = nullptr;
        float* no_critic = nullptr;   // no privileged-critic rows: the two last arguments are not read
        if (A.f32class)
            return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, true, false, true, RuntimeSensing>>(
                grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map, no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, dyns, sens,
                sen_map, pending, stream, no_critic, no_critic);
        return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, false, false, true, RuntimeSensing>>(
            grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map, no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, dyns, sens,
            sen_map, pending, stream, no_critic, no_critic);
    });
}

}  // namespace qr
