// quadrace_eval_history.hip -- the sensing-grid evaluator for policies that OBSERVE THEIR LAST COMMANDS (qr_evaluate_policy_history_grid):
// eval_policy_sensing_grid_kernel (quadrace_eval_sensing.hip) with the policy bank at obs_len + 4 H inputs and eval_policy_body's history
// mode (quadrace_eval_body.hpp): the row the policy sees at call-step k is [o~_k | u_{k-1}, ..., u_{k-H}], the last H clipped commands
// COMPUTED in the current episode behind the noisy observation, zeros before the episode's start, cleared by the step that ends it.
// The sensor, its stream (gid = env_id_base + the env's index within its GROUP) and the command queue are the sensing evaluator's; the
// caller's `pending` [n][16] carries max(d, H) entries in canonical order and passes between this call, qr_evaluate_policy_sensing_grid,
// qr_rollout_policy_sensing and qr_rollout_policy_history.  obs_len<V, GA>() + 4 H = obs_len<V, GA + H>(): for GA + H <= 4 a length the
// policy bank and the forward already have; 10 (GA, H) pairs per variant and precision.
// The step loop, the accounting and the records are eval_policy_body's.  No atomics, no workgroup that waits for another, no global store
// inside the step loop.  A translation unit of its own with the flags of quadrace_eval_sensing.hip: the code objects of the other sources
// do not change when this one does.
#include "quadrace_eval_body.hpp"
#include "quadrace_launch.hpp"
#include "quadrace_sensing.hpp"

namespace qr {

// the arguments of eval_policy_sensing_grid_kernel; bank / bank_lo hold images of PolicyDims<obs_len<V, GA + H>()>
template <int V, int GA, int H, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
eval_policy_history_grid_kernel(Params P0, const half8* __restrict__ bank, const half8* __restrict__ bank_lo, const float* __restrict__ conds,
                                const float* __restrict__ dyns, const float* __restrict__ sens, const int4* __restrict__ map, int wgs_per_group, int K,
                                SensingStream stream, float* __restrict__ pending, int4* __restrict__ rec, float4* __restrict__ recf) {
    using D = PolicyDims<obs_len<V, GA + H>()>;
    // workgroup-uniform (blockIdx only): the group of this workgroup, its map entry, its images, and the workgroup's first env within its group
    const int grp = (int)blockIdx.x / wgs_per_group;
    const int local0 = ((int)blockIdx.x - grp * wgs_per_group) * kBlock;
    const int4 pcds = map[grp];
    const half8* __restrict__ img = bank + (size_t)pcds.x * D::kTotalHalf8;
    const half8* __restrict__ img_lo = bank_lo + (size_t)pcds.x * D::kTotalHalf8;
    const float* __restrict__ cond = conds + (size_t)pcds.y * kCondSlotFloats;
    const RuntimeDyn<V> dyn = load_dynamics<V>(dyns + (size_t)pcds.z * kDynSlotFloats);
    SensingRegs sen;
    load_sensing(sens + (size_t)pcds.w * kSensingSlotFloats, stream, pending, sen);
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
    eval_policy_body<V, GA, kF32, false, RuntimeDyn<V>, RuntimeSensing, H>(P, img, img_lo, cond + kCondHeaderFloats, i, local0 + (int)threadIdx.x, K,
                                                                           gates_per_lap, rec, recf, &dyn, &sen);
}

// the arguments of launch_eval_policy_sensing_grid and `history` in [1, 4 - P.gates_ahead]; the bank's images have obs_len + 4 history
// inputs (checked by the caller).  envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n are checked again here: a grid that
// does not match P.n would read and write out of bounds.
hipError_t launch_eval_policy_history_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const float* dyns,
                                           const float* sens, const int4* map, int history, bool f32class, int num_groups, int envs_per_group, int K,
                                           uint64_t noise_seed, uint64_t first_step, float* pending, int32_t* rec, float* recf, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !bank || !bank_lo || !conds || !dyns || !sens || !map || !pending || ((uintptr_t)pending & 15) || !rec || K < 1)
        return hipErrorInvalidValue;
    const SensingStream stream = sensing_stream(noise_seed, first_step);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        return dispatch_history<GA>(history, [&](auto h) {
            constexpr int H = decltype(h)::value;
            constexpr size_t lds = eval_lds_bytes<obs_len<V, GA + H>()>() + sizeof(float) * kSensingQueueFloats * kBlock;
            int4* rec4 = reinterpret_cast<int4*>(rec);
            float4* recf4 = reinterpret_cast<float4*>(recf);
            const dim3 grid((unsigned)(P.n / kBlock));
            const int wgs = envs_per_group / kBlock;
            if (f32class)
                return launch_dynamic_lds<eval_policy_history_grid_kernel<V, GA, H, true>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, dyns, sens, map,
                                                                                           wgs, K, stream, pending, rec4, recf4);
            return launch_dynamic_lds<eval_policy_history_grid_kernel<V, GA, H, false>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, dyns, sens, map,
                                                                                        wgs, K, stream, pending, rec4, recf4);
        });
    });
}

}  // namespace qr
