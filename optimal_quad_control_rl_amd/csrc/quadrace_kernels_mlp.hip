// quadrace_kernels_mlp.hip -- launcher of the two fused E2E + residual-MLP rollout kernels (rollout_fast_mlp_kernel,
// rollout_lean_mlp_kernel of quadrace_env_kernels.hpp), which are therefore instantiated in THIS translation unit and in no other.
//
// build.py compiles it WITHOUT the SLP vectoriser (PER_SOURCE_FLAGS): next to their matrix instructions, and above all at two waves per
// SIMD where a packed-f32 instruction costs 1.3 x a scalar one (profiles/r04_valu_rate.txt), the vectoriser's packed operations and
// the ~80 register moves that feed them are a net loss there: 1 Mi envs 40.5 -> 42.3 G env-steps/s, 65 536 envs + 1.5 %
// (profiles/r05_slp_ab.txt).  The INDI and per-step kernels keep it (INDI at 65 536 envs loses 8 % without).  Same arithmetic either
// way: the vectoriser packs, it does not re-associate (-ffp-contract=off, explicit fmaf) -- the forms stay bit-identical
// (tests/test_gpu_round4.py).
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"

namespace qr {

hipError_t launch_rollout_mlp(bool lean, const Params& P, int K, const float4* a4, float* obs, float* rew, uint8_t* done,
                              uint8_t* trunc, hipStream_t st) {
    return dispatch_ga(P.gates_ahead, [&](auto ga) {
        constexpr int GA = decltype(ga)::value;
        if (lean)   // the lean forms' LDS is dynamic (more than the 64 KB a static array may have)
            return launch_dynamic_lds<rollout_lean_mlp_kernel<kE2E, GA>>(grid_for(P.n), dim3(kBlock), lean_lds_bytes<kE2E, GA, true>(), st,
                                                                         P, K, a4, obs, rew, done, trunc);
        hipLaunchKernelGGL((rollout_fast_mlp_kernel<kE2E, GA>), grid_for(P.n), dim3(kBlock), 0, st, P, K, a4, obs, rew, done, trunc);
        return hipGetLastError();
    });
}

}  // namespace qr
