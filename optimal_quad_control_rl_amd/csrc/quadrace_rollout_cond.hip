// quadrace_rollout_cond.hip -- PPO's collect phase across a MIX of flight conditions in one launch (qr_rollout_policy_conditions):
// the launch function and the instantiations of rollout_policy_group_kernel<V, GA, kF32, false> (quadrace_rollout_group.hpp, where the
// kernel and everything about it is written down): one policy per launch, a condition per group of envs.  The map is the grid
// evaluator's (policy, condition) array; the policy half is not read here.
// A translation unit of its own, compiled with the flags of quadrace_kernels.hip (where rollout_policy_kernel is instantiated: SLP
// vectoriser on; the -fno-slp-vectorize of quadrace_kernels_mlp.hip was measured for the open-loop fused kernels at two waves per
// SIMD, this one runs one workgroup per CU like its twin), so that the closed-loop kernels stay comparable.
#include "quadrace_rollout_group.hpp"

namespace qr {

// conds: [capacity][kCondSlotFloats] floats; map: [num_groups] (unused, condition), every index already checked against the bank by the
// caller.  envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n are checked again here: a grid that does not match P.n
// would read and write out of bounds.
hipError_t launch_rollout_policy_cond(int variant, const Params& P, const PolicyArgs& A, const float* conds, const int2* map, int num_groups,
                                      int envs_per_group, int K, float* obs, float* act, float* logp, float* rew, uint8_t* done,
                                      uint8_t* trunc, float* last_obs, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !conds || !map)
        return hipErrorInvalidValue;
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value, L = obs_len<V, GA>();
        const size_t lds = (size_t)PolicyDims<L>::kTotalHalf8 * 16 + sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * L);
        float4* act4 = reinterpret_cast<float4*>(act);
        const dim3 grid((unsigned)(P.n / kBlock));
        const int wgs = envs_per_group / kBlock;
        const float* no_dyns = nullptr;   // the nominal vehicle: the literals of the instruction stream
        const float* no_sens = nullptr;   // no sensor either: the four arguments behind dyns are not read
        const int* no_sen_map = nullptr;
        float* no_pending = nullptr;
        float* no_critic = nullptr;    // no privileged-critic rows: the two last arguments are not read
        const half8* no_bank = nullptr;   // one policy per launch: A.weights / A.weights_lo and A's sampling arguments
        const PopulationEntry* no_table = nullptr;
        if (A.f32class)
            return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, true, false>>(grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map,
                                                                                       no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, no_dyns,
                                                                                       no_sens, no_sen_map, no_pending, SensingStream{}, no_critic, no_critic);
        return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, false, false>>(grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds, map,
                                                                                    no_table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, no_dyns,
                                                                                    no_sens, no_sen_map, no_pending, SensingStream{}, no_critic, no_critic);
    });
}

}  // namespace qr
