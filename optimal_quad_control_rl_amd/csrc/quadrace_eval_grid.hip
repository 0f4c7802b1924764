// quadrace_eval_grid.hip -- closed-loop evaluation of a GRID of policies x flight conditions in one launch (qr_evaluate_policy_grid):
// eval_policy_bank_kernel (quadrace_eval_bank.hip: step loop, lap / crash accounting, group-local reset stream) written out again,
// with two differences:
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
// when this one does.  There are no tail lanes (the host refuses anything else), so every lane is an env and every lane stores.
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"

namespace qr {

static_assert(QR_EVAL_REC_INTS == 24 && QR_EVAL_MAX_LAPS == 8 && QR_EVAL_REC_FLOATS == 4, "record layout of include/quadrace.h");

// bank / bank_lo: image 0 of the two policy arrays; conds: slot 0 of the condition bank; map[g] = (policy, condition) of group g;
// wgs_per_group = E / kBlock
template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
eval_policy_grid_kernel(Params P0, const half8* __restrict__ bank, const half8* __restrict__ bank_lo, const float* __restrict__ conds,
                        const int2* __restrict__ map, int wgs_per_group, int K, int4* __restrict__ rec, float4* __restrict__ recf) {
    constexpr int L = obs_len<V, GA>();
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);                                   // policy weights (f16) of THIS workgroup's policy
    float* rtab = reinterpret_cast<float*>(smem + (size_t)D::kTotalHalf8 * 16);  // reset table | gate rows | lap sums and counts
    float* gates = rtab + kResetTableFloats;
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
    const int lane = threadIdx.x & 63;
    Env<V> e;
    load_env<V>(P, i, e);
    // the lane's record: read here, written behind the loop (a caller continues an evaluation by passing the same buffers again)
    const int4 r0 = rec[(size_t)i * 6], r1 = rec[(size_t)i * 6 + 1];
    // lap sums / counts [16][kBlock] live in LDS, as in eval_policy_kernel: touched at lap boundaries only, indexed by the lap number
    int* laps = reinterpret_cast<int*>(gates + kMaxGates * kGateStride) + threadIdx.x;
    {   // (register pressure: v[] lives only from these four loads to the 16 LDS writes below, all ahead of the weight staging and the loop)
        const int4 b = rec[(size_t)i * 6 + 2], c = rec[(size_t)i * 6 + 3], d = rec[(size_t)i * 6 + 4], f = rec[(size_t)i * 6 + 5];
        const int v[2 * QR_EVAL_MAX_LAPS] = {r1.z, r1.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w, f.x, f.y};
#pragma unroll
        for (int q = 0; q < 2 * QR_EVAL_MAX_LAPS; ++q) laps[q * kBlock] = v[q];   // own column only: no barrier needed
    }
    int n_gates = r0.x, n_crash = r0.y, n_limit = r0.z, since = r0.w, lap_t0 = r1.x, now = r1.y;
    // passes into the running lap and laps finished since the (re)start: kept instead of dividing `since` on every step
    int lap_no = since / gates_per_lap, in_lap = since - lap_no * gates_per_lap;
    float ep_ret = 0.0f, ret_sum = 0.0f, ret_sq = 0.0f;
    if (recf) {
        const float4 f = recf[i];
        ep_ret = f.x; ret_sum = f.y; ret_sq = f.z;
    }
    MlpRegs mlp;
    const bool use_mlp = (V == kE2E) && (P.flags & kFlagResidual);
    if (use_mlp) mlp_load_regs(P.tables, lane, mlp);
    {
        const float4* s4 = reinterpret_cast<const float4*>(img);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int j = threadIdx.x; j < D::kTotalHalf8; j += kBlock) d4[j] = s4[j];
    }
    {   // the condition's [reset table | gate rows], as stage_tables copies the handle's (counts are multiples of 4, slots 16-byte aligned)
        const float4* s4 = reinterpret_cast<const float4*>(cond + kCondHeaderFloats);
        float4* d4 = reinterpret_cast<float4*>(rtab);
        const int count4 = (kResetTableFloats + P.num_gates * kGateStride) / 4;
        for (int j = threadIdx.x; j < count4; j += kBlock) d4[j] = s4[j];
    }
    __syncthreads();
    // the reset stream's env id: the env's index WITHIN its group
    const uint32_t gid_lo = P.gid_lo + (uint32_t)(local0 + (int)threadIdx.x);
    const uint32_t gid_hi = P.gid_hi + (gid_lo < P.gid_lo ? 1u : 0u);
    bool any_reset = false;
    float stash[reset_value_count<V>()];   // the lane's own next reset draws (reset_from_stash)
    bool stash_ok = false;
    float o[L];
    observe<V, GA>(P, gates, e, o);
    for (int k = 0; k < K; ++k) {
        float mean[4];
        if constexpr (kF32) policy_forward_f32class<L>(W, img_lo, lane, o, mean);
        else policy_forward<L>(W, lane, o, mean);
        const float u[4] = {fminf(fmaxf(mean[0], -1.0f), 1.0f), fminf(fmaxf(mean[1], -1.0f), 1.0f),
                            fminf(fmaxf(mean[2], -1.0f), 1.0f), fminf(fmaxf(mean[3], -1.0f), 1.0f)};
        const int target_before = e.target;
        bool done, trunc, did_reset;
        const float reward = step_env<V>(P, gates, rtab, nullptr, mlp, lane, true, e, u, gid_lo, gid_hi, done, trunc, did_reset,
                                         [](bool) {}, [&](bool need) { reset_from_stash<V>(P, rtab, need, e, gid_lo, gid_hi, stash, stash_ok); });
        any_reset |= did_reset;
        // ---- accounting (tests/eval_spec.py, same order).  A pass on the step that ends the episode is not counted: the reset has
        // replaced the target, and that episode's lap count is void anyway.
        now += 1;
        const bool pass = !done && e.target != target_before;
        if (pass) {
            n_gates += 1;
            since += 1;
            in_lap += 1;
            if (in_lap == gates_per_lap) {   // a lap boundary: rare and divergent, so a branch (skipped by the whole wave most steps)
                in_lap = 0;
                lap_no += 1;
                if (lap_no <= QR_EVAL_MAX_LAPS) {
                    laps[(lap_no - 1) * kBlock] += now - lap_t0;
                    laps[(QR_EVAL_MAX_LAPS + lap_no - 1) * kBlock] += 1;
                }
                lap_t0 = now;
            }
        }
        ep_ret = add_rn(ep_ret, reward);
        if (done) {
            if (trunc) n_limit += 1; else n_crash += 1;
            since = 0; in_lap = 0; lap_no = 0;
            lap_t0 = now;
            ret_sum = add_rn(ret_sum, ep_ret);
            ret_sq = add_rn(ret_sq, mul_rn(ep_ret, ep_ret));
            ep_ret = 0.0f;
        }
        observe<V, GA>(P, gates, e, o);
    }
    int4* row = rec + (size_t)i * 6;
    int lap_sum[QR_EVAL_MAX_LAPS], lap_cnt[QR_EVAL_MAX_LAPS];
#pragma unroll
    for (int q = 0; q < QR_EVAL_MAX_LAPS; ++q) {
        lap_sum[q] = laps[q * kBlock];
        lap_cnt[q] = laps[(QR_EVAL_MAX_LAPS + q) * kBlock];
    }
    row[0] = make_int4(n_gates, n_crash, n_limit, since);
    row[1] = make_int4(lap_t0, now, lap_sum[0], lap_sum[1]);
    row[2] = make_int4(lap_sum[2], lap_sum[3], lap_sum[4], lap_sum[5]);
    row[3] = make_int4(lap_sum[6], lap_sum[7], lap_cnt[0], lap_cnt[1]);
    row[4] = make_int4(lap_cnt[2], lap_cnt[3], lap_cnt[4], lap_cnt[5]);
    row[5] = make_int4(lap_cnt[6], lap_cnt[7], 0, 0);
    if (recf) recf[i] = make_float4(ep_ret, ret_sum, ret_sq, 0.0f);
    define_exit_values<V>(e);
    P.ts[i] = pack_ts<V>(e);
    store_world<V>(P, i, e);
    if (any_reset) store_dist<V>(P, i, e);
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
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value, L = obs_len<V, GA>();
        const size_t lds = (size_t)PolicyDims<L>::kTotalHalf8 * 16 + sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + 2 * QR_EVAL_MAX_LAPS * kBlock);
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
