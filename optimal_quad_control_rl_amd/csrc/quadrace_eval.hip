// quadrace_eval.hip -- closed-loop policy EVALUATION (qr_evaluate_policy): eval_policy_body (quadrace_eval_body.hpp: step loop, lap /
// crash accounting, record layout) over one handle and one policy.  Lane i is env i of the handle, flies the policy of PolicyArgs
// under the handle's own tables and scalars, and draws its resets as env P.gid + i.  The grid rounds N up to whole workgroups, so
// this is the evaluator with tail lanes.  A translation unit of its own: the code objects of the other sources do not change when
// this one does.
#include "quadrace_eval_body.hpp"
#include "quadrace_launch.hpp"

namespace qr {

template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
eval_policy_kernel(Params P, PolicyArgs A, int K, int gates_per_lap, int4* __restrict__ rec, float4* __restrict__ recf) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    eval_policy_body<V, GA, kF32, true>(P, A.weights, A.weights_lo, P.tables + kOffResetImage, i, i, K, gates_per_lap, rec, recf);
}

hipError_t launch_eval_policy(int variant, const Params& P, const PolicyArgs& A, int K, int gates_per_lap, int32_t* rec, float* recf,
                              hipStream_t st) {
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        constexpr size_t lds = eval_lds_bytes<obs_len<V, GA>()>();
        int4* rec4 = reinterpret_cast<int4*>(rec);
        float4* recf4 = reinterpret_cast<float4*>(recf);
        if (A.f32class)
            return launch_dynamic_lds<eval_policy_kernel<V, GA, true>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, gates_per_lap, rec4, recf4);
        return launch_dynamic_lds<eval_policy_kernel<V, GA, false>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, gates_per_lap, rec4, recf4);
    });
}

}  // namespace qr
