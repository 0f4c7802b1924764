// quadrace_eval_bank.hip -- closed-loop evaluation of a BANK of policies in one launch (qr_evaluate_policy_bank): the step loop and
// the lap / crash accounting of eval_policy_kernel (quadrace_eval.hip; record layout: include/quadrace.h, restated on the CPU in
// tests/eval_spec.py), with two differences:
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
// A translation unit of its own: the code objects of the other sources do not change when this one does.  There are no tail lanes
// (N = P E, E a multiple of kBlock: the host refuses anything else), so every lane is an env and every lane stores.
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"

namespace qr {

static_assert(QR_EVAL_REC_INTS == 24 && QR_EVAL_MAX_LAPS == 8 && QR_EVAL_REC_FLOATS == 4, "record layout of include/quadrace.h");

// bank / bank_lo: image 0 of the two arrays; wgs_per_policy = E / kBlock
template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
eval_policy_bank_kernel(Params P, const half8* __restrict__ bank, const half8* __restrict__ bank_lo, int wgs_per_policy, int K,
                        int gates_per_lap, int4* __restrict__ rec, float4* __restrict__ recf) {
    constexpr int L = obs_len<V, GA>();
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);                                   // policy weights (f16) of THIS workgroup's policy
    float* rtab = reinterpret_cast<float*>(smem + (size_t)D::kTotalHalf8 * 16);  // reset table | gate rows | lap sums and counts
    float* gates = rtab + kResetTableFloats;
    // workgroup-uniform (blockIdx only): the policy of this workgroup, its images, and the workgroup's first env within its group
    const int pol = (int)blockIdx.x / wgs_per_policy;
    const int local0 = ((int)blockIdx.x - pol * wgs_per_policy) * kBlock;
    const half8* __restrict__ img = bank + (size_t)pol * D::kTotalHalf8;
    const half8* __restrict__ img_lo = bank_lo + (size_t)pol * D::kTotalHalf8;
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
    stage_tables(P, rtab, kOffResetImage, kResetTableFloats + P.num_gates * kGateStride);
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

// bank / bank_lo: [>= num_policies][PolicyDims<L>::kTotalHalf8] half8.  The caller guarantees envs_per_policy % kBlock == 0 and
// num_policies * envs_per_policy == P.n (checked again here: a grid that does not match P.n would read and write out of bounds).
hipError_t launch_eval_policy_bank(int variant, const Params& P, const half8* bank, const half8* bank_lo, bool f32class, int num_policies,
                                   int envs_per_policy, int K, int gates_per_lap, int32_t* rec, float* recf, hipStream_t st) {
    if (num_policies < 1 || envs_per_policy < kBlock || envs_per_policy % kBlock != 0 ||
        (long long)num_policies * envs_per_policy != (long long)P.n)
        return hipErrorInvalidValue;
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value, L = obs_len<V, GA>();
        const size_t lds = (size_t)PolicyDims<L>::kTotalHalf8 * 16 + sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + 2 * QR_EVAL_MAX_LAPS * kBlock);
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
