// quadrace_rollout_population.hip -- PPO's collect phase for a POPULATION of policies in one launch (qr_rollout_policy_population):
// the launch function and the instantiations of rollout_policy_group_kernel<V, GA, kF32, true> (quadrace_rollout_group.hpp, where the
// kernel and everything about it is written down): group g flies policy map[g].x of the bank under condition map[g].y and samples
// with table[g].  A carries the launch-wide step counter, deterministic and f32class only.
// A translation unit of its own, compiled with the flags of quadrace_kernels.hip like quadrace_rollout_cond.hip, so that the closed-loop
// rollout kernels stay comparable.
#include "quadrace_rollout_group.hpp"

namespace qr {

// bank / bank_lo: [capacity][PolicyDims<L>::kTotalHalf8] half8; conds: [capacity][kCondSlotFloats] floats; map: [num_groups] (policy,
// condition), every index already checked against its bank by the caller; table: [num_groups] sampling arguments.  A carries the
// launch-wide step counter, deterministic and f32class only.  envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n are
// checked again here: a grid that does not match P.n would read and write out of bounds.
hipError_t launch_rollout_policy_population(int variant, const Params& P, const PolicyArgs& A, const half8* bank, const half8* bank_lo,
                                            const float* conds, const int2* map, const PopulationEntry* table, int num_groups, int envs_per_group,
                                            int K, float* obs, float* act, float* logp, float* rew, uint8_t* done, uint8_t* trunc, float* last_obs,
                                            hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !bank || !bank_lo || !conds || !map || !table)
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
        if (A.f32class)
            return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, true, true>>(grid, dim3(kBlock), lds, st, P, A, bank, bank_lo, conds, map,
                                                                                      table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, no_dyns,
                                                                                      no_sens, no_sen_map, no_pending, SensingStream{}, no_critic, no_critic);
        return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, false, true>>(grid, dim3(kBlock), lds, st, P, A, bank, bank_lo, conds, map,
                                                                                   table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs, no_dyns,
                                                                                   no_sens, no_sen_map, no_pending, SensingStream{}, no_critic, no_critic);
    });
}

}  // namespace qr
