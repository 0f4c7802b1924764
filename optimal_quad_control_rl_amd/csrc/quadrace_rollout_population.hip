// quadrace_rollout_population.hip -- PPO's collect phase for a POPULATION of policies in one launch (qr_rollout_policy_population):
// rollout_policy_cond_kernel (quadrace_rollout_cond.hip) with BOTH halves of the group map read and the sampling arguments per group.
//   * group map: as there, num_groups groups x E envs, E a multiple of kBlock, N = num_groups E exactly; workgroup b belongs to group
//     g = b / (E / kBlock) and reads map[g] = (policy slot, condition slot) from an address that derives from blockIdx alone: one
//     8-byte scalar load, and the three bases built from it (weight image, low-piece image, condition image) stay in scalar registers,
//     as eval_policy_grid_kernel keeps them.  The host has validated both indices against the banks' capacities.
//   * weights: the workgroup stages image map[g].x of the policy bank (bank + slot * PolicyDims<L>::kTotalHalf8) into its LDS where
//     rollout_policy_cond_kernel stages A.weights; the f32-class forward reads that slot's low pieces from global memory, as
//     eval_policy_bank_kernel does.
//   * sampling arguments: table[g] is one 32-byte PopulationEntry (quadrace_launch.hpp): std[4], logp_const, seed_lo, seed_hi, pad,
//     the values rollout_policy_args computes for the group's log_std and noise seed.  Its address derives from blockIdx alone and no
//     store of this kernel touches the table: one 32-byte scalar load, and the values stay in scalar registers where the kernel
//     arguments A.std / A.logp_const / A.seed_lo / A.seed_hi of the twin sit.  step_lo / step_hi, deterministic and f32class stay
//     launch-wide (PolicyArgs; its weight pointers and per-launch sampling fields are not read here).
// Nothing else differs: env ids are the handle's ordinary ones (P.gid + i), the rollout rows, terminal-observation rows, last_obs and
// the state write-back are rollout_policy_kernel's, the noise slices and their pins are verbatim, and there are no tail lanes.  Group
// g therefore computes what an E-env handle with env_id_base + g E, configured with the group's condition, computes under
// qr_rollout_policy with the weights of its slot, its log_std and its seed (tests/test_gpu_rollout_population.py demands bit equality).
//
// The step loop RESTATES rollout_policy_cond_kernel's statement for statement, the way that file restates rollout_policy_kernel:
// the existing kernels' matrix-instruction schedules are pinned with sched_barriers and their code objects must not move when this
// unit is added (tools/isa_digest.py), so no shared header is touched.  A translation unit of its own, compiled with the flags of
// quadrace_kernels.hip like quadrace_rollout_cond.hip, so that the closed-loop rollout kernels stay comparable.
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"

namespace qr {

// bank / bank_lo: image 0 of the two policy arrays; conds: slot 0 of the condition bank; map[g] = (policy, condition) of group g;
// table[g] = sampling arguments of group g; wgs_per_group = E / kBlock
template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
rollout_policy_population_kernel(Params P0, PolicyArgs A, const half8* __restrict__ bank, const half8* __restrict__ bank_lo,
                                 const float* __restrict__ conds, const int2* __restrict__ map, const PopulationEntry* __restrict__ table,
                                 int wgs_per_group, int K, float* __restrict__ obs_out, float4* __restrict__ act_out,
                                 float* __restrict__ logp_out, float* __restrict__ rew_out, uint8_t* __restrict__ done_out,
                                 uint8_t* __restrict__ trunc_out, float* __restrict__ last_obs_out) {
    constexpr int L = obs_len<V, GA>();
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);                                   // policy weights (f16)
    float* rtab = reinterpret_cast<float*>(smem + (size_t)D::kTotalHalf8 * 16);  // reset table | gate rows | obs tiles
    float* gates = rtab + kResetTableFloats;
    // workgroup-uniform (blockIdx only): the group of this workgroup, its map entry, its images, its sampling arguments, and the
    // handle's Params with the condition's scalars
    const int grp = (int)blockIdx.x / wgs_per_group;
    const int2 pc = map[grp];
    const half8* __restrict__ img = bank + (size_t)pc.x * D::kTotalHalf8;
    const half8* __restrict__ img_lo = bank_lo + (size_t)pc.x * D::kTotalHalf8;
    const float* __restrict__ cond = conds + (size_t)pc.y * kCondSlotFloats;
    const CondHeader* __restrict__ hdr = reinterpret_cast<const CondHeader*>(cond);
    const PopulationEntry S = table[grp];
    Params P = P0;
    P.num_gates = hdr->num_gates;
    P.max_steps = hdr->max_steps;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        P.obs_lo[c] = hdr->obs_lo[c];
        P.obs_inv[c] = hdr->obs_inv[c];
    }
    const int i = blockIdx.x * kBlock + threadIdx.x;   // < P.n: the grid is exactly P.n / kBlock workgroups
    const int lane = threadIdx.x & 63;
    Env<V> e;
    load_env<V>(P, i, e);
    MlpRegs mlp;
    const bool use_mlp = (V == kE2E) && (P.flags & kFlagResidual);
    if (use_mlp) mlp_load_regs(P.tables, lane, mlp);
    {
        const float4* s4 = reinterpret_cast<const float4*>(img);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int j = threadIdx.x; j < D::kTotalHalf8; j += kBlock) d4[j] = s4[j];
    }
    {   // [reset table | gate rows] of the condition, as stage_tables copies the handle's (counts are multiples of 4)
        const float4* s4 = reinterpret_cast<const float4*>(cond + kCondHeaderFloats);
        float4* d4 = reinterpret_cast<float4*>(rtab);
        const int count4 = (kResetTableFloats + P.num_gates * kGateStride) / 4;
        for (int j = threadIdx.x; j < count4; j += kBlock) d4[j] = s4[j];
    }
    __syncthreads();
    const uint32_t gid_lo = P.gid_lo + (uint32_t)i;   // ordinary ids: reset stream and noise of env i of the handle
    const uint32_t gid_hi = P.gid_hi + (gid_lo < P.gid_lo ? 1u : 0u);
    const size_t n = (size_t)P.n;
    const int wave_first = i - lane;
    float* tile = gates + kMaxGates * kGateStride + (threadIdx.x >> 6) * 64 * L;
    bool any_reset = false;
    float stash[reset_value_count<V>()];   // the lane's own next reset draws (reset_from_stash)
    bool stash_ok = false;
    float o[L];
    observe<V, GA>(P, gates, e, o);
    for (int k = 0; k < K; ++k) {
        // ---- action noise: rollout_policy_kernel's slices, verbatim (drawn in deterministic mode too and then multiplied out); the
        // Philox key is the group's
        float mean[4];
        float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t pc4[4];
        float bm_u1a, bm_u2a, bm_u1b, bm_u2b, bm_ra, bm_rb, bm_sa, bm_ca, bm_sb, bm_cb;
        auto pin_u = [](uint32_t& x) { asm volatile("" : "+v"(x)); };
        auto pin_f = [](float& x) { asm volatile("" : "+v"(x)); };
        auto noise_slice = [&](int slot) {
            if (slot >= 1 && slot <= 11) { pin_u(pc4[0]); pin_u(pc4[1]); pin_u(pc4[2]); pin_u(pc4[3]); }
            if (slot == 12) pin_f(bm_u1a);
            if (slot == 13) pin_f(bm_u1b);
            if (slot == 14) pin_f(bm_u2a);
            if (slot == 15) pin_f(bm_u2b);
            if (slot == 16) { pin_f(bm_ra); pin_f(bm_rb); pin_f(bm_sa); pin_f(bm_sb); }
            if (slot == 0) {
                const uint32_t s_lo = A.step_lo + (uint32_t)k;
                pc4[0] = gid_lo; pc4[1] = gid_hi; pc4[2] = s_lo; pc4[3] = A.step_hi + (s_lo < A.step_lo ? 1u : 0u);
            } else if (slot <= 10) {
                philox4x32_round(pc4, S.seed_lo, S.seed_hi, slot - 1);
            } else if (slot == 11) {  // Box-Muller: two pairs of normals from four uniforms (u1 in (0,1], u2 in [0,1))
                bm_u1a = (float)((pc4[0] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2a = u01(pc4[1]);
                bm_u1b = (float)((pc4[2] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2b = u01(pc4[3]);
            } else if (slot == 12) {
                bm_ra = fast_sqrt(-2.0f * __logf(bm_u1a));
            } else if (slot == 13) {
                bm_rb = fast_sqrt(-2.0f * __logf(bm_u1b));
            } else if (slot == 14) {
                qr_sincos(6.283185307179586f * bm_u2a, bm_sa, bm_ca);
            } else if (slot == 15) {
                qr_sincos(6.283185307179586f * bm_u2b, bm_sb, bm_cb);
            } else if (slot == 16) {
                eps[0] = bm_ra * bm_ca; eps[1] = bm_ra * bm_sa; eps[2] = bm_rb * bm_cb; eps[3] = bm_rb * bm_sb;
            }
        };
        // The observation row of this step (the policy's input) is stored under the third layer's MFMAs: LDS transpose in slot 0,
        // coalesced block store in slot 2 (every wave is full).
        auto obs_slice = [&](int slot) {
            if (slot == 0) obs_tile_write<V, GA>(tile, lane, o);
            if (slot == 2) obs_tile_flush<V, GA>(tile, obs_out + (size_t)k * n * L, (size_t)wave_first, lane);
        };
        if constexpr (kF32) {
#pragma unroll
            for (int slot = 0; slot <= 16; ++slot) noise_slice(slot);
            obs_slice(0);
            obs_slice(2);
            policy_forward_f32class<L>(W, img_lo, lane, o, mean);
        } else {
            policy_forward<L>(W, lane, o, mean, noise_slice, obs_slice);
        }
        float a[4] = {mean[0], mean[1], mean[2], mean[3]};
        float logp = S.logp_const;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float en = A.deterministic ? 0.0f : eps[c];   // fmaf(std, 0, mean) = mean, fmaf(-0, 0, logp) = logp
            a[c] = fmaf(S.std[c], en, mean[c]);
            logp = fmaf(-0.5f * en, en, logp);
        }
        // rollout buffer row t: the observation the action was computed from (stored above), the unclipped action, its log-prob
        stream_store(act_out + (size_t)k * n + i, make_float4(a[0], a[1], a[2], a[3]));
        stream_store(logp_out + (size_t)k * n + i, logp);
        const float u[4] = {fminf(fmaxf(a[0], -1.0f), 1.0f), fminf(fmaxf(a[1], -1.0f), 1.0f),
                            fminf(fmaxf(a[2], -1.0f), 1.0f), fminf(fmaxf(a[3], -1.0f), 1.0f)};
        bool done, trunc, did_reset;
        const float reward = step_env<V>(P, gates, rtab, tile, mlp, lane, true, e, u, gid_lo, gid_hi, done, trunc, did_reset,
                                         [&](bool fin) { store_terminal_obs<V, GA>(P, gates, e, (size_t)k * n, i, fin); },
                                         [&](bool need) { reset_from_stash<V>(P, rtab, need, e, gid_lo, gid_hi, stash, stash_ok); });
        any_reset |= did_reset;
        stream_store(rew_out + (size_t)k * n + i, reward);
        stream_store(done_out + (size_t)k * n + i, (uint8_t)(done ? 1 : 0));
        if (trunc_out) stream_store(trunc_out + (size_t)k * n + i, (uint8_t)(trunc ? 1 : 0));
        observe<V, GA>(P, gates, e, o);
    }
    if (last_obs_out) store_obs_coalesced<V, GA>(tile, last_obs_out, (size_t)wave_first, lane, o);
    define_exit_values<V>(e);
    P.ts[i] = pack_ts<V>(e);
    store_world<V>(P, i, e);
    if (any_reset) store_dist<V>(P, i, e);
}

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
        if (A.f32class)
            return launch_dynamic_lds<rollout_policy_population_kernel<V, GA, true>>(grid, dim3(kBlock), lds, st, P, A, bank, bank_lo, conds, map,
                                                                                     table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs);
        return launch_dynamic_lds<rollout_policy_population_kernel<V, GA, false>>(grid, dim3(kBlock), lds, st, P, A, bank, bank_lo, conds, map,
                                                                                  table, wgs, K, obs, act4, logp, rew, done, trunc, last_obs);
    });
}

}  // namespace qr
