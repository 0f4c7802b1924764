// quadrace_eval_sensing.hip -- closed-loop evaluation of a grid of policies x flight conditions x vehicles x SENSING in one launch
// (qr_evaluate_policy_sensing_grid): eval_policy_dynamics_grid_kernel (quadrace_eval_dynamics.hip) with the map's fourth entry read and
// a fourth bank.  "Which sensing error breaks this policy first, and how many control periods of latency can it fly with?" is one launch
// instead of a host loop of one launch per step.
// The sensor itself -- the slot and its load, the sigma groups, the Philox stream of the observation noise, sensing_noise4 and the
// RuntimeSensing class -- is quadrace_sensing.hpp, shared with the sensing mode of the grouped rollout (quadrace_rollout_sensing.hip).
// What is this unit's own: gid = env_id_base + the env's index within its GROUP (the id of the group-local reset stream: every cell of
// a grid draws the same eps), and the command queue as a ring in the lane's own LDS column behind the lap sums (eval_policy_body), which
// travels between launches in the caller's `pending` [n][16] in canonical order.
// ONE device function, sensing_noise4, gives sigma x eps to the evaluator and to sensing_noise_kernel (qr_sensing_noise: the rows the
// tests hold the stream's spec by).  The step loop, the accounting and the records are eval_policy_body's.  No atomics, no workgroup that
// waits for another, no global store inside the step loop.  A translation unit of its own: the code objects of the other sources do not
// change when this one does.
#include "quadrace_eval_body.hpp"
#include "quadrace_launch.hpp"
#include "quadrace_sensing.hpp"

namespace qr {

// bank / bank_lo: image 0 of the two policy arrays; conds / dyns / sens: slot 0 of the condition, dynamics and sensing banks;
// map[g] = (policy, condition, dynamics, sensing) of group g; wgs_per_group = E / kBlock; pending: [n][kSensingQueueFloats]
template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
eval_policy_sensing_grid_kernel(Params P0, const half8* __restrict__ bank, const half8* __restrict__ bank_lo, const float* __restrict__ conds,
                                const float* __restrict__ dyns, const float* __restrict__ sens, const int4* __restrict__ map, int wgs_per_group, int K,
                                SensingStream stream, float* __restrict__ pending, int4* __restrict__ rec, float4* __restrict__ recf) {
    using D = PolicyDims<obs_len<V, GA>()>;
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
    eval_policy_body<V, GA, kF32, false, RuntimeDyn<V>, RuntimeSensing>(P, img, img_lo, cond + kCondHeaderFloats, i, local0 + (int)threadIdx.x, K,
                                                                        gates_per_lap, rec, recf, &dyn, &sen);
}

// out [K][E][L]: mul_rn(sigma[group(j)], eps[j]) of the group-local envs 0..E-1 at call-steps 0..K-1 -- what the evaluator adds to the
// observation of env (group, e) at step first_step + k.  grid (ceil(E / kBlock), K); an all-zero slot writes +0.0f.
template <int V, int GA>
__global__ void __launch_bounds__(kBlock)
sensing_noise_kernel(uint32_t base_lo, uint32_t base_hi, const float* __restrict__ slot, int E, SensingStream stream, float* __restrict__ out) {
    constexpr int L = obs_len<V, GA>();
    SensingRegs sen;
    load_sensing(slot, stream, nullptr, sen);
    const int e = blockIdx.x * kBlock + threadIdx.x, k = blockIdx.y;
    if (e >= E) return;
    const uint32_t gid_lo = base_lo + (uint32_t)e;
    const uint32_t gid_hi = base_hi + (gid_lo < base_lo ? 1u : 0u);
    float row[L];
#pragma unroll
    for (int j = 0; j < L; ++j) row[j] = 0.0f;
    if (sen.noise_on) sensing_noise_row<V, GA>(sen, gid_lo, gid_hi, k, row, false);
    float* dst = out + ((size_t)k * E + e) * L;
#pragma unroll
    for (int j = 0; j < L; ++j) dst[j] = row[j];
}

// bank / bank_lo / conds / dyns / map as launch_eval_policy_dynamics_grid; sens: [capacity][kSensingSlotFloats] floats; every index of the
// map already checked against its bank by the caller.  envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n are checked
// again here: a grid that does not match P.n would read and write out of bounds.
hipError_t launch_eval_policy_sensing_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const float* dyns,
                                           const float* sens, const int4* map, bool f32class, int num_groups, int envs_per_group, int K,
                                           uint64_t noise_seed, uint64_t first_step, float* pending, int32_t* rec, float* recf, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !bank || !bank_lo || !conds || !dyns || !sens || !map || !pending || !rec || K < 1)
        return hipErrorInvalidValue;
    const SensingStream stream = sensing_stream(noise_seed, first_step);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        constexpr size_t lds = eval_lds_bytes<obs_len<V, GA>()>() + sizeof(float) * kSensingQueueFloats * kBlock;
        int4* rec4 = reinterpret_cast<int4*>(rec);
        float4* recf4 = reinterpret_cast<float4*>(recf);
        const dim3 grid((unsigned)(P.n / kBlock));
        const int wgs = envs_per_group / kBlock;
        if (f32class)
            return launch_dynamic_lds<eval_policy_sensing_grid_kernel<V, GA, true>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, dyns, sens, map, wgs,
                                                                                    K, stream, pending, rec4, recf4);
        return launch_dynamic_lds<eval_policy_sensing_grid_kernel<V, GA, false>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, dyns, sens, map, wgs,
                                                                                 K, stream, pending, rec4, recf4);
    });
}

// slot: the slot of the sensing bank to dump; out: [K][envs_per_group][obs_len] floats.  K <= 65535 (grid.y).
hipError_t launch_sensing_noise(int variant, const Params& P, const float* slot, int envs_per_group, int K, uint64_t noise_seed, uint64_t first_step,
                                float* out, hipStream_t st) {
    if (!slot || !out || envs_per_group < 1 || K < 1 || K > 65535) return hipErrorInvalidValue;
    const SensingStream stream = sensing_stream(noise_seed, first_step);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        const dim3 grid((unsigned)((envs_per_group + kBlock - 1) / kBlock), (unsigned)K);
        hipLaunchKernelGGL((sensing_noise_kernel<V, GA>), grid, dim3(kBlock), 0, st, P.gid_lo, P.gid_hi, slot, envs_per_group, stream, out);
        return hipGetLastError();
    });
}

}  // namespace qr
