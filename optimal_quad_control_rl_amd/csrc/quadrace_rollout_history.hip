// quadrace_rollout_history.hip -- PPO's collect phase for a policy that OBSERVES ITS LAST COMMANDS (qr_rollout_policy_history): the launch
// function, the checks and the instantiations of rollout_policy_group_kernel<V, GA, kF32, false, true, RuntimeSensing, H>
// (quadrace_rollout_group.hpp, where the kernel and everything about this mode is written down): the sensing mode of the grouped rollout
// with the last H clipped commands computed in the episode appended to the policy's row, [o~_k | u_{k-1}, ..., u_{k-H}].
// Why: under a command delay of d control steps the observation alone is no Markov state of what is flown -- the commands computed and not
// yet flown are hidden from the network that computed them.  The controller knows what it sent, so the history part is exact (no noise).
// The row is obs_len<V, GA>() + 4 H = obs_len<V, GA + H>() floats long, a length every network kernel of the library is instantiated
// for as long as GA + H <= 4: the policy forward in both precisions, the PPO update, the bank loader and ES run unchanged on the longer
// length.  10 (GA, H) pairs per variant and precision.
// What the rows hold: obs_out[k] is the [noisy observation | history] row the action was computed from, rows of obs_len + 4 H floats;
// act / logp / rew / done / trunc as qr_rollout_policy_sensing; last_obs carries the noise of call-step K and the history after K steps;
// terminal rows are [clean observation of the terminal state | u_k, ..., u_{k-H+1}], the registered buffer read as [rows][N][obs_len + 4 H];
// `pending` carries max(d, H) entries in canonical order.
// A translation unit of its own, compiled with the flags of quadrace_rollout_sensing.hip (the build's defaults): the code objects of the
// other sources do not change when this one does.
#include "quadrace_rollout_group.hpp"

namespace qr {

// dynamic LDS, as the sensing mode carves it: policy image (f16) | reset table | gate rows | observation tiles | command queues, at the
// policy's row length
template <int L>
constexpr size_t rollout_history_lds_bytes() {
    return (size_t)PolicyDims<L>::kTotalHalf8 * 16 +
           sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * L + kSensingQueueFloats * kBlock);
}
static_assert(rollout_history_lds_bytes<obs_len<kE2E, 4>()>() <= 160 * 1024, "the largest row (36 floats) is the sensing mode's largest: one workgroup per CU");

// the arguments of launch_rollout_policy_sensing and `history` in [1, 4 - P.gates_ahead]: A's weights are images of a policy of
// obs_len + 4 history inputs, obs / last_obs / the registered terminal buffer have rows of that length (the caller has checked the
// policy's length; the buffers are the caller's word, as everywhere).  envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n
// are checked again here: a grid that does not match P.n would read and write out of bounds.
hipError_t launch_rollout_policy_history(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const float* sens,
                                         const int2* map, const int* sen_map, int history, int num_groups, int envs_per_group, int K,
                                         uint64_t noise_seed, uint64_t first_step, float* pending, float* obs, float* act, float* logp, float* rew,
                                         uint8_t* done, uint8_t* trunc, float* last_obs, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !conds || !dyns || !sens || !map || !sen_map || !pending || ((uintptr_t)pending & 15) || K < 1)
        return hipErrorInvalidValue;
    const SensingStream stream = sensing_stream(noise_seed, first_step);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        return dispatch_history<GA>(history, [&](auto h) {
            constexpr int H = decltype(h)::value;
            constexpr size_t lds = rollout_history_lds_bytes<obs_len<V, GA + H>()>();
            float4* act4 = reinterpret_cast<float4*>(act);
            const dim3 grid((unsigned)(P.n / kBlock));
            const int wgs = envs_per_group / kBlock;
            const half8* no_bank = nullptr;   // one policy per launch: A.weights / A.weights_lo and A's sampling arguments
            const PopulationEntry* no_table = nullptr;
            float* no_critic = nullptr;   // no privileged-critic rows: the two last arguments are not read
            if (A.f32class)
                return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, true, false, true, RuntimeSensing, H>>(
                    grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map, no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, dyns,
                    sens, sen_map, pending, stream, no_critic, no_critic);
            return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, false, false, true, RuntimeSensing, H>>(
                grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map, no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, dyns, sens,
                sen_map, pending, stream, no_critic, no_critic);
        });
    });
}

}  // namespace qr
