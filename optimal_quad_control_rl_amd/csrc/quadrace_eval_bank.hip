// quadrace_eval_bank.hip -- closed-loop evaluation of a BANK of policies in one launch (qr_evaluate_policy_bank): eval_policy_body
// (quadrace_eval_body.hpp: step loop, lap / crash accounting, record layout) with two inputs of its own:
//   * per-workgroup policy: the launch carries P policies x E envs per policy, E a multiple of kBlock, N = P E exactly.  A 256-env
//     workgroup already stages the policy image into its own LDS and never shares it, so workgroup b stages image p = b / (E / kBlock)
//     of the bank ([capacity][PolicyDims<L>::kTotalHalf8] half8, each image byte for byte what qr_policy_set_weights produces) and, in
//     the f32-class form, reads the low pieces of policy p from global memory.  p and both image bases are workgroup-uniform: they
//     are derived from blockIdx alone and stay in scalar registers.
//   * group-local reset stream: the Philox counter's env id of lane i is P.gid + (i mod E) instead of P.gid + i (64-bit carry as
//     everywhere); key, episode counter and block index are unchanged.  Env j of every group therefore draws the same reset values
//     for the same episode number: groups that start from the same state see identical starts, disturbances and restarts for as
//     long as their own flying allows (common random numbers), and group p flies exactly what an E-env handle with the same seed
//     and env_id_base flies under qr_evaluate_policy.
// Tables and scalars are the handle's.  A translation unit of its own: the code objects of the other sources do not change when this
// one does.  There are no tail lanes (N = P E, E a multiple of kBlock: the host refuses anything else).
#include "quadrace_eval_body.hpp"
#include "quadrace_launch.hpp"

namespace qr {

// bank / bank_lo: image 0 of the two arrays; wgs_per_policy = E / kBlock
template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
eval_policy_bank_kernel(Params P, const half8* __restrict__ bank, const half8* __restrict__ bank_lo, int wgs_per_policy, int K,
                        int gates_per_lap, int4* __restrict__ rec, float4* __restrict__ recf) {
    using D = PolicyDims<obs_len<V, GA>()>;
    // workgroup-uniform (blockIdx only): the policy of this workgroup, its images, and the workgroup's first env within its group
    const int pol = (int)blockIdx.x / wgs_per_policy;
    const int local0 = ((int)blockIdx.x - pol * wgs_per_policy) * kBlock;
    const half8* __restrict__ img = bank + (size_t)pol * D::kTotalHalf8;
    const half8* __restrict__ img_lo = bank_lo + (size_t)pol * D::kTotalHalf8;
    const int i = blockIdx.x * kBlock + threadIdx.x;   // < P.n: the grid is exactly P.n / kBlock workgroups
    eval_policy_body<V, GA, kF32, false>(P, img, img_lo, P.tables + kOffResetImage, i, local0 + (int)threadIdx.x, K, gates_per_lap, rec, recf);
}

// bank / bank_lo: [>= num_policies][PolicyDims<L>::kTotalHalf8] half8.  The caller guarantees envs_per_policy % kBlock == 0 and
// num_policies * envs_per_policy == P.n (checked again here: a grid that does not match P.n would read and write out of bounds).
hipError_t launch_eval_policy_bank(int variant, const Params& P, const half8* bank, const half8* bank_lo, bool f32class, int num_policies,
                                   int envs_per_policy, int K, int gates_per_lap, int32_t* rec, float* recf, hipStream_t st) {
    if (num_policies < 1 || envs_per_policy < kBlock || envs_per_policy % kBlock != 0 ||
        (long long)num_policies * envs_per_policy != (long long)P.n)
        return hipErrorInvalidValue;
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        constexpr size_t lds = eval_lds_bytes<obs_len<V, GA>()>();
        int4* rec4 = reinterpret_cast<int4*>(rec);
        float4* recf4 = reinterpret_cast<float4*>(recf);
        const dim3 grid((unsigned)(P.n / kBlock));
        const int wgs = envs_per_policy / kBlock;
        if (f32class)
            return launch_dynamic_lds<eval_policy_bank_kernel<V, GA, true>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, wgs, K, gates_per_lap, rec4, recf4);
        return launch_dynamic_lds<eval_policy_bank_kernel<V, GA, false>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, wgs, K, gates_per_lap, rec4, recf4);
    });
}

}  // namespace qr
