// quadrace_eval_grid.hip -- closed-loop evaluation of a GRID of policies x flight conditions in one launch (qr_evaluate_policy_grid):
// eval_policy_body (quadrace_eval_body.hpp: step loop, lap / crash accounting, record layout) with the group-local reset stream of
// eval_policy_bank_kernel (quadrace_eval_bank.hip) and two inputs of its own:
//   * per-workgroup policy AND condition from a group map: the launch carries num_groups groups x E envs, E a multiple of kBlock,
//     N = num_groups E exactly.  Workgroup b belongs to group g = b / (E / kBlock) and reads the map entry (policy index, condition
//     index) of g: one 8-byte load from an address that derives from blockIdx alone, so it is a scalar load, and the policy image
//     base, the low-piece base and the condition base built from it stay in scalar registers, as the bank kernel keeps img / img_lo.
//     The host has validated both indices against the banks' capacities before the launch (qr_evaluate_policy_grid).
//   * per-workgroup condition image: a slot of the condition bank is [CondHeader | reset table | gate rows] (quadrace_device.hpp),
//     the last two byte for byte what a handle configured with the condition holds from kOffResetImage on.  The workgroup stages
//     THAT table image into its LDS instead of P.tables + kOffResetImage, and a kernel-local copy of Params takes num_gates,
//     max_steps, obs_lo and obs_inv from the header (scalar loads again: uniform address, memory no store of this kernel touches
//     before them); gates_per_lap comes from the header too.  The residual-MLP table, dt, flags and gates_ahead stay the handle's.
// Every cell of a policies x conditions grid therefore draws the SAME uniform reset values (group-local stream) and differs only in
// the condition's own scaling of them, and group g flies exactly what an E-env handle configured with its condition flies under
// qr_evaluate_policy with its policy's weights.  A translation unit of its own: the code objects of the other sources do not change
// when this one does.  There are no tail lanes (the host refuses anything else).
#include "quadrace_eval_body.hpp"
#include "quadrace_launch.hpp"

namespace qr {

// bank / bank_lo: image 0 of the two policy arrays; conds: slot 0 of the condition bank; map[g] = (policy, condition) of group g;
// wgs_per_group = E / kBlock
template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
eval_policy_grid_kernel(Params P0, const half8* __restrict__ bank, const half8* __restrict__ bank_lo, const float* __restrict__ conds,
                        const int2* __restrict__ map, int wgs_per_group, int K, int4* __restrict__ rec, float4* __restrict__ recf) {
    using D = PolicyDims<obs_len<V, GA>()>;
    // workgroup-uniform (blockIdx only): the group of this workgroup, its map entry, its images, and the workgroup's first env within its group
    const int grp = (int)blockIdx.x / wgs_per_group;
    const int local0 = ((int)blockIdx.x - grp * wgs_per_group) * kBlock;
    const int2 pc = map[grp];
    const half8* __restrict__ img = bank + (size_t)pc.x * D::kTotalHalf8;
    const half8* __restrict__ img_lo = bank_lo + (size_t)pc.x * D::kTotalHalf8;
    const float* __restrict__ cond = conds + (size_t)pc.y * kCondSlotFloats;
    const CondHeader* __restrict__ hdr = reinterpret_cast<const CondHeader*>(cond);
    Params P = P0;   // the handle's, with the condition's scalars
    P.num_gates = hdr->num_gates;
    P.max_steps = hdr->max_steps;
    const int gates_per_lap = hdr->gates_per_lap;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        P.obs_lo[c] = hdr->obs_lo[c];
        P.obs_inv[c] = hdr->obs_inv[c];
    }
    const int i = blockIdx.x * kBlock + threadIdx.x;   // < P.n: the grid is exactly P.n / kBlock workgroups
    eval_policy_body<V, GA, kF32, false>(P, img, img_lo, cond + kCondHeaderFloats, i, local0 + (int)threadIdx.x, K, gates_per_lap, rec, recf);
}

// bank / bank_lo: [capacity][PolicyDims<L>::kTotalHalf8] half8; conds: [capacity][kCondSlotFloats] floats; map: [num_groups] (policy,
// condition), every index already checked against its bank by the caller.  envs_per_group % kBlock == 0 and num_groups *
// envs_per_group == P.n are checked again here: a grid that does not match P.n would read and write out of bounds.
hipError_t launch_eval_policy_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const int2* map,
                                   bool f32class, int num_groups, int envs_per_group, int K, int32_t* rec, float* recf, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !bank || !bank_lo || !conds || !map)
        return hipErrorInvalidValue;
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        constexpr size_t lds = eval_lds_bytes<obs_len<V, GA>()>();
        int4* rec4 = reinterpret_cast<int4*>(rec);
        float4* recf4 = reinterpret_cast<float4*>(recf);
        const dim3 grid((unsigned)(P.n / kBlock));
        const int wgs = envs_per_group / kBlock;
        if (f32class)
            return launch_dynamic_lds<eval_policy_grid_kernel<V, GA, true>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, map, wgs, K, rec4, recf4);
        return launch_dynamic_lds<eval_policy_grid_kernel<V, GA, false>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, map, wgs, K, rec4, recf4);
    });
}

}  // namespace qr
