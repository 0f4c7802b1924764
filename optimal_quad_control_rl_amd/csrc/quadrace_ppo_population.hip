// quadrace_ppo_population.hip -- the PPO minibatch update of a POPULATION of learners: one minibatch of all P members is THREE launches
// (qr_ppo_population_epoch), where P handles driven by qr_ppo_epoch one after another take 2 P.
//
// Why kernels of its own: ppo_apply_kernel (quadrace_ppo.hip) spins on a grid-wide barrier that relies on all of its workgroups being
// resident; several of them in flight, or one beside gradient workgroups that own a CU each, break that assumption, and P x 247 workgroups
// do not fit under one barrier.  Here NO kernel waits for another workgroup: the apply kernel is cut in two at its barrier and the
// kernel boundary takes the barrier's place.  No spin, no flag, no atomic, no cooperative launch; PpoCtrl::arrive / go / gen /
// barrier_timeouts of the members are never touched.
//
//   grad     ppo_population_grad_kernel, grid (wgs, 2, P): ppo_grad_kernel's work for every member at once.  A workgroup reads ITS
//            member's entry of a device-resident table (PopMember; the address derives from blockIdx alone: scalar loads, and what the
//            twin holds in kernel-argument registers sits in the same kind of register here); the minibatch index k is a launch argument:
//            idx = perm + k B, acc = mbstats + 2 k.  Partials and per-wave sums go to the member's own qr_ppo buffers.
//   reduce   ppo_population_reduce_kernel, grid (247, P): the first half of ppo_apply_kernel -- DenseMap thread -> parameter, reduce_grad_element,
//            block_sum2_f64 of g^2 -- writing the gradient element, the workgroup's squared sum (the float the barrier word carries in
//            the twin) and the last block's minibatch statistics to the member's scratch area, plus a snapshot of PpoCtrl::stop / adam_t
//            as they stood BEFORE this minibatch (the step kernel's last block rewrites them while its other blocks still start).
//   step     ppo_population_step_kernel, grid (247, P): the second half.  EVERY workgroup adds its member's squared sums in the barrier
//            master's order (lane q over slots q, q + 64, ... in double, then wave_sum_f64), takes the same target-KL and finiteness verdicts,
//            the same clip and torch.optim.Adam expressions with the member's device-resident adam_t and lr, and scatters the f16 copies
//            into the member's images; the last block does the master's bookkeeping under the same conditions.
//
// The gradient kernel RESTATES ppo_grad_kernel statement for statement (the way quadrace_rollout_population.hip restates its twin): the
// existing kernels' schedules are pinned and their code objects must not move (tools/isa_digest.py).  The reasons for every choice in the
// body are written down at the twin and not repeated here.  The profiling stamps (QR_PHASE_TIMING) are not carried over.
// The per-epoch launches (shuffle, table zeroing, advantage sums) are the existing kernels, issued once per member (qr::ppo_epoch_prologue).
#include <cstring>
#include <vector>

#include "quadrace_ppo_device.hpp"

namespace qr {

// One member's entry of the device-resident table: everything its workgroups need, found from blockIdx alone.
struct PopMember {
    PpoBatch b;          // rollout arrays, B, G, clip, vf_coef, ent_coef, stop, theta, images, wave_out, stats as fill_batch() sets them;
                         // idx = the member's WHOLE permutation, acc = its WHOLE advantage-sum table (the kernels add k B / 2 k)
    void* partial;       // the member's partial buffer (bf16 or f32: the launch knows)
    float *theta, *m, *v;
    PpoCtrl* ctrl;
    float max_norm, beta1, beta2, eps;
    float kl_limit;      // 1.5 * target_kl * B; <= 0: no early stop
    int pad_;
    // scratch owned by the population object, rewritten by every minibatch's reduce launch and read by its step launch
    float* grad;         // [workgroups * kApplyThreads] gradient element of thread j
    float* sq;           // [workgroups] squared sums, as floats
    float* mb;           // [0..3] the last block's red[4..7]; [4], [5] as int: PpoCtrl::stop / adam_t before this minibatch
};
constexpr int kMaxPopulation = 256;
struct PopLr { float v[kMaxPopulation]; };

// PpoCtrl::lr of every member <- the call's values: they travel in the kernel arguments (see ppo_set_lr_kernel), so a learning-rate
// schedule does not force a re-capture
__global__ void __launch_bounds__(kMaxPopulation) ppo_population_lr_kernel(const PopMember* __restrict__ table, int num_members, PopLr lr) {
    const int p = (int)threadIdx.x;
    if (p < num_members) table[p].ctrl->lr = lr.v[p];
}

template <int L, typename PT>
__global__ void __launch_bounds__(512, 1) ppo_population_grad_kernel(const PopMember* __restrict__ table, int k) {
    using D = PpoDims<L>;
    using P = PolicyDims<L>;
    constexpr int KS1 = P::kSteps1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);
    half8* E = W + D::kImage;
    const unsigned lds_base = (unsigned)(size_t)smem;
    // the member of this workgroup and its minibatch k, in the form the twin receives as kernel arguments
    const PopMember& M = table[blockIdx.z];
    PpoBatch a = M.b;
    a.idx += (size_t)k * a.B;
    a.acc += 2 * k;
    PT* __restrict__ partial = reinterpret_cast<PT*>(M.partial);
    const int net = blockIdx.y;
    const int stop_flag = *a.stop;
    const int wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int role = wave8 >> 2;          // 0: chain wave, 1: dW wave
    const int wave = wave8 & 3;
    const int et = wave & 1;
    const int O = net == 0 ? 4 : 1;
    PT* gn = partial + ((size_t)blockIdx.x * 2 + net) * D::kRawSlots;
    const float scale = 1.0f / (float)a.B;
    const int pairs = (a.G + 1) / 2;
    const f32x16p zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (role == 0) {
    for (int pair = blockIdx.x, pass = 0; pair < pairs; pair += gridDim.x, ++pass) {
        int lane = (int)(threadIdx.x & 63), tid = (int)threadIdx.x;
        asm volatile("" : "+v"(lane), "+v"(tid));
        const int c = lane & 31, h = lane >> 5;
        float* stash = reinterpret_cast<float*>(E + kExHalf8) + wave * 32 + c;
            // =========================================== chain waves ===========================================================
            const int g = 2 * pair + (wave >> 1);
            const bool live = g < a.G;
            const int pos = (live ? g : a.G - 1) * 64 + 32 * et + c;
            const bool row_ok = pos < a.B;
            const int b = a.idx[row_ok ? pos : a.B - 1];
            float xin[KS1][8];
            {
                const float* row = a.obs + (size_t)b * L;
#pragma unroll
                for (int s = 0; s < KS1; ++s)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int kk = 16 * s + 8 * h + j;
                        xin[s][j] = row[kk < L ? kk : L - 1];
                    }
            }
            const float4 act_v = net == 0 ? reinterpret_cast<const float4*>(a.act)[b] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float old_logp_in = a.old_logp[b], adv_in = a.adv[b], ret_in = a.ret[b];
            const double acc_s1 = a.acc[0], acc_s2 = a.acc[1];
            float log_std_v[4];
            {
                const float* log_std = a.theta + net_off(L, 4).total + net_off(L, 1).total;
#pragma unroll
                for (int q = 0; q < 4; ++q) log_std_v[q] = log_std[q];
            }
            __syncthreads();   // pass 0: [A] W1 staged / later passes: [S0]
            if (stop_flag) return;   // uniform over the member's workgroups
            if (h == 0) {
                stash[0 * kStashRows] = act_v.x;
                stash[1 * kStashRows] = act_v.y;
                stash[2 * kStashRows] = act_v.z;
                stash[3 * kStashRows] = act_v.w;
                stash[4 * kStashRows] = old_logp_in;
                stash[5 * kStashRows] = adv_in;
                stash[6 * kStashRows] = ret_in;
            }
            half8 in[KS1];
#pragma unroll
            for (int s = 0; s < KS1; ++s) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kk = 16 * s + 8 * h + j;
                    v[j] = kk < L ? xin[s][j] : (kk == L ? 1.0f : 0.0f);
                }
                in[s] = sat_pack(v);
            }
            const bool valid = h == 0 && live && row_ok;
            constexpr bool kHM = true;
            uint32_t m1[2] = {0u, 0u}, m2[2] = {0u, 0u}, m3[2] = {0u, 0u};
            half8 h1[8], h2[8], h3[8];
            const u32x4p* hm_e = reinterpret_cast<const u32x4p*>(E + 4 * 8 * 64 + wave * 8 * 64) + (lane ^ (h << 2));
            const u32x4p* hm_o = reinterpret_cast<const u32x4p*>(E + 4 * 8 * 64 + wave * 8 * 64) + (lane ^ ((h | 2) << 2));
            mlp_layer<KS1, false, true, kHM>(W, lane, in, h1, m1);
            if (pass == 0) __syncthreads();   // [B] W2 staged
            mlp_layer<8, false, true, kHM>(W + P::kOff2, lane, h1, h2, m2);
            if (pass == 0) __syncthreads();   // [C] W3 staged
            mlp_layer<8, false, true, kHM>(W + P::kOff3, lane, h2, h3, m3);
            if (pass == 0) __syncthreads();   // [S0] W4 staged
            half8 w4[8], w4t[4];
#pragma unroll
            for (int s = 0; s < 8; ++s) w4[s] = W[P::kOff4 + s * 64 + (lane ^ ((h | ((s & 1) << 1)) << 2))];
            {
                const unsigned a40 = lds_base + tr_lane_out(lane, 0, true) + 16u * (unsigned)P::kOff4;
                const unsigned a41 = lds_base + tr_lane_out(lane, 1, true) + 16u * (unsigned)P::kOff4;
                w4t[0] = lds_tr_pair2<16 * 128 * 0>(a40, a41);
                w4t[1] = lds_tr_pair2<16 * 128 * 1>(a40, a41);
                w4t[2] = lds_tr_pair2<16 * 128 * 2>(a40, a41);
                w4t[3] = lds_tr_pair2<16 * 128 * 3>(a40, a41);
            }
            float out4[4];
            {
                f32x16p acc = zero;
#pragma unroll
                for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w4[s], h3[s], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) out4[r] = acc[r];
            }
            // ---- per-sample loss gradients (x B; the 1/B of the batch means is applied when the tiles are stored)
            float wsum[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            const float* st_ = stash;
            float dout[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (net == 0) {
                const float act[4] = {st_[0 * kStashRows], st_[1 * kStashRows], st_[2 * kStashRows], st_[3 * kStashRows]};
                const float old_logp_v = st_[4 * kStashRows], adv_v = st_[5 * kStashRows];
                float z[4], inv_std[4], logp = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float ls = log_std_v[q];
                    inv_std[q] = __expf(-ls);
                    z[q] = (act[q] - out4[q]) * inv_std[q];
                    logp += -0.5f * z[q] * z[q] - ls - 0.9189385332046727f;
                }
                const float log_ratio = valid ? logp - old_logp_v : 0.0f;
                const float ratio = __expf(log_ratio);
                const double amean = acc_s1 / a.B;
                const double avar = fmax((acc_s2 - a.B * amean * amean) / (a.B > 1 ? a.B - 1 : 1), 0.0);
                const float A = valid ? (adv_v - (float)amean) * (float)(1.0 / (sqrt(avar) + 1e-8)) : 0.0f;
                const bool flows = A >= 0.0f ? (ratio <= 1.0f + a.clip) : (ratio >= 1.0f - a.clip);
                const float gl = (flows && valid) ? -A * ratio : 0.0f;
                float dls[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    dout[q] = gl * z[q] * inv_std[q];
                    dls[q] = gl * (z[q] * z[q] - 1.0f);
                }
                const float clipped_ratio = fminf(fmaxf(ratio, 1.0f - a.clip), 1.0f + a.clip);
#pragma unroll
                for (int q = 0; q < 4; ++q) wsum[q] = dls[q];
                wsum[4] = valid ? -fminf(A * ratio, A * clipped_ratio) : 0.0f;
                wsum[5] = valid ? (ratio - 1.0f) - log_ratio : 0.0f;
                wsum[6] = valid && fabsf(ratio - 1.0f) > a.clip ? 1.0f : 0.0f;
            } else {
                const float err = valid ? out4[0] - st_[6 * kStashRows] : 0.0f;
                dout[0] = a.vf_coef * 2.0f * err;
                wsum[4] = err * err;
            }
            // ---- layer 4 operands: d4 transposed by the identity MFMA, h3 as natural packs
            half8 d4;
            {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (j < 4 && valid) ? dout[j < 4 ? j : 0] : 0.0f;
                d4 = sat_pack(v);
                half8 id;
#pragma unroll
                for (int j = 0; j < 8; ++j) id[j] = (8 * h + j == c) ? (_Float16)1.0f : (_Float16)0.0f;
                const f32x16p acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(d4, id, zero, 0, 0, 0);
                E[(0 * 8 + 2 * wave) * 64 + lane] = plain_pack(acc, 0);
                E[(0 * 8 + 2 * wave + 1) * 64 + lane] = plain_pack(acc, 1);
            }
            packs_to_lds(h3, E + 4 * 8 * 64, wave, lane);
            __syncthreads();   // [S1] layer-4 operands published
            // d3 = (W4^T d4) * relu'(z3)
            half8 dA[8], dB[8];
            lds_tr_wait<0>(w4t[0], w4t[1]);
            lds_tr_wait<0>(w4t[2], w4t[3]);
            u32x4p hm3[2][4];
            if constexpr (kHM) {
#pragma unroll
                for (int q = 0; q < 4; ++q) hm3[0][q] = ((q & 1) ? hm_o : hm_e)[q * 64];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x16p acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w4t[t], d4, zero, 0, 0, 0);
                if constexpr (kHM) {
                    if (t == 1) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) hm3[1][q] = ((q & 1) ? hm_o : hm_e)[(4 + q) * 64];
                    }
                    dA[2 * t] = mask_pack_h(acc, 0, hm3[t >> 1][2 * (t & 1)]);
                    dA[2 * t + 1] = mask_pack_h(acc, 1, hm3[t >> 1][2 * (t & 1) + 1]);
                } else {
                    dA[2 * t] = mask_pack(acc, m3[t >> 1], t, 0);
                    dA[2 * t + 1] = mask_pack(acc, m3[t >> 1], t, 1);
                }
            }
            chain_stats_out(a, wsum, net, live, lane, g, et, scale);
            __syncthreads();   // [S2] the dW waves are done reading the layer-4 operands
            packs_to_lds(dA, E, wave, lane);
            packs_to_lds(h2, E + 4 * 8 * 64, wave, lane);
            __syncthreads();   // [S3] layer-3 operands published
            mlp_layer_bwd<P::kOff3, kHM>(lds_base + tr_lane_hidden(lane, 0, true), lds_base + tr_lane_hidden(lane, 1, true), dA, dB, m2, hm_e, hm_o);   // d2
            __syncthreads();   // [S4]
            packs_to_lds(dB, E, wave, lane);
            packs_to_lds(h1, E + 4 * 8 * 64, wave, lane);
            __syncthreads();   // [S5] layer-2 operands published
            mlp_layer_bwd<P::kOff2, kHM>(lds_base + tr_lane_hidden(lane, 0, true), lds_base + tr_lane_hidden(lane, 1, true), dB, dA, m1, hm_e, hm_o);   // d1
            __syncthreads();   // [S6]
            // ---- layer 1 operands: d1 as natural packs, x0 transposed by the identity MFMA
            packs_to_lds(dA, E, wave, lane);
#pragma unroll
            for (int ut = 0; ut < D::kIT; ++ut) {
                f32x16p acc = zero;
#pragma unroll
                for (int s = 0; s < KS1; ++s) {
                    half8 id;
#pragma unroll
                    for (int j = 0; j < 8; ++j) id[j] = (16 * s + 8 * h + j == 32 * ut + c) ? (_Float16)1.0f : (_Float16)0.0f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(in[s], id, acc, 0, 0, 0);
                }
                E[((4 + ut) * 8 + 2 * wave) * 64 + lane] = plain_pack(acc, 0);
                E[((4 + ut) * 8 + 2 * wave + 1) * 64 + lane] = plain_pack(acc, 1);
            }
            __syncthreads();   // [S7] layer-1 operands published
        }
    } else {
        // the operand image is staged by the four dW waves, layer by layer, each workgroup in its own rotation
        {
            const f32x4p* src = reinterpret_cast<const f32x4p*>(a.images + (size_t)net * D::kImage);
            f32x4p* dst = reinterpret_cast<f32x4p*>(W);
            const int t256 = (int)(threadIdx.x & 255);
            constexpr int n1 = P::kOff2 / 256, n2 = (P::kOff3 - P::kOff2) / 256, n3 = (P::kOff4 - P::kOff3) / 256, n4 = (D::kImage - P::kOff4) / 256;
            static_assert(P::kOff2 % 256 == 0 && P::kOff3 % 256 == 0 && P::kOff4 % 256 == 0 && D::kImage % 256 == 0, "image layers are whole 256-chunk blocks");
            const int rot = (int)blockIdx.x;
            f32x4p i1[n1], i2[n2], i3[n3], i4[n4];
#pragma unroll
            for (int q = 0; q < n1; ++q) i1[q] = src[((q + rot) % n1) * 256 + t256];
#pragma unroll
            for (int q = 0; q < n2; ++q) i2[q] = src[P::kOff2 + ((q + rot) % n2) * 256 + t256];
#pragma unroll
            for (int q = 0; q < n3; ++q) i3[q] = src[P::kOff3 + ((q + rot) % n3) * 256 + t256];
#pragma unroll
            for (int q = 0; q < n4; ++q) i4[q] = src[P::kOff4 + ((q + rot) % n4) * 256 + t256];
            auto put = [&](int i, const f32x4p& v) { dst[i ^ (((i >> 5) & 3) << 2)] = v; };   // chunk swizzle
#pragma unroll
            for (int q = 0; q < n1; ++q) put(((q + rot) % n1) * 256 + t256, i1[q]);
            __syncthreads();   // [A] W1 staged
            if (stop_flag) return;   // (the chain waves leave at the same barrier)
#pragma unroll
            for (int q = 0; q < n2; ++q) put(P::kOff2 + ((q + rot) % n2) * 256 + t256, i2[q]);
            __syncthreads();   // [B] W2 staged
#pragma unroll
            for (int q = 0; q < n3; ++q) put(P::kOff3 + ((q + rot) % n3) * 256 + t256, i3[q]);
            __syncthreads();   // [C] W3 staged
#pragma unroll
            for (int q = 0; q < n4; ++q) put(P::kOff4 + ((q + rot) % n4) * 256 + t256, i4[q]);
        }
        f32x16p dw4 = zero, dw3[2][2] = {{zero, zero}, {zero, zero}}, dw2[2][2] = {{zero, zero}, {zero, zero}}, dw1[2][2] = {{zero, zero}, {zero, zero}};
    for (int pair = blockIdx.x, pass = 0; pair < pairs; pair += gridDim.x, ++pass) {
        int lane = (int)(threadIdx.x & 63), tid = (int)threadIdx.x;
        asm volatile("" : "+v"(lane), "+v"(tid));
        const unsigned ex_lane0 = lds_base + 16u * (unsigned)D::kImage + ex_lane_const(lane, 0);
        const unsigned ex_lane1 = lds_base + 16u * (unsigned)D::kImage + ex_lane_const(lane, 1);
            // ============================================= dW waves ============================================================
            __syncthreads();   // [S0]
            if (stop_flag) return;
            const bool last = pair + (int)gridDim.x >= pairs;
            const int to0 = 2 * (wave >> 1), ti0 = 2 * (wave & 1);
            __syncthreads();   // [S1]
            dw_tile_old_tr_half<0>(E, ex_lane0 + 2048u * (unsigned)wave, ex_lane1 + 2048u * (unsigned)wave, lane, dw4);   // tile (0, wave)
            dw_tile_old_tr_half<4>(E, ex_lane0 + 2048u * (unsigned)wave, ex_lane1 + 2048u * (unsigned)wave, lane, dw4);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();   // [S2]
            __syncthreads();   // [S3]
            dw_block_tr(ex_lane0 + 2048u * (unsigned)to0, ex_lane1 + 2048u * (unsigned)to0, ex_lane0 + 2048u * (unsigned)ti0, ex_lane1 + 2048u * (unsigned)ti0, dw3);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();   // [S4]
            if (last) store_dw_tile_raw<PT>(dw4, gn + (D::kRawT4 + wave) * 1024, O, lane, scale);
            if (last) {
#pragma unroll
                for (int bt = 0; bt < 2; ++bt)
#pragma unroll
                    for (int bi = 0; bi < 2; ++bi) store_dw_tile_raw<PT, true>(dw3[bt][bi], gn + (D::kRawT3 + 4 * (to0 + bt) + ti0 + bi) * 1024, kH - 32 * (to0 + bt), lane, scale);
            }
            __syncthreads();   // [S5]
            dw_block_tr(ex_lane0 + 2048u * (unsigned)to0, ex_lane1 + 2048u * (unsigned)to0, ex_lane0 + 2048u * (unsigned)ti0, ex_lane1 + 2048u * (unsigned)ti0, dw2);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();   // [S6]
            __syncthreads();   // [S7]
            if (last) {
#pragma unroll
                for (int bt = 0; bt < 2; ++bt)
#pragma unroll
                    for (int bi = 0; bi < 2; ++bi) store_dw_tile_raw<PT, true>(dw2[bt][bi], gn + (D::kRawT2 + 4 * (to0 + bt) + ti0 + bi) * 1024, kH - 32 * (to0 + bt), lane, scale);
            }
            dw_tiles_tr_old_half<D::kIT, 0>(ex_lane0 + 2048u * (unsigned)wave, ex_lane1 + 2048u * (unsigned)wave, E + 4 * 8 * 64, lane, dw1);   // tiles (wave, 0..kIT-1)
            dw_tiles_tr_old_half<D::kIT, 4>(ex_lane0 + 2048u * (unsigned)wave, ex_lane1 + 2048u * (unsigned)wave, E + 4 * 8 * 64, lane, dw1);
            __builtin_amdgcn_sched_barrier(0);
            if (last) {
#pragma unroll
                for (int bi = 0; bi < D::kIT; ++bi) store_dw_tile_raw<PT, true>(dw1[0][bi], gn + (D::kIT * wave + bi) * 1024, kH - 32 * wave, lane, scale);
            }
        }
    }
}

// thread j of a member's reduce / step grid -> its parameter i (n: none) and its column pj in the partial table: ppo_apply_kernel's map
// for accumulator-order partials
template <int L>
__device__ __forceinline__ void population_thread_map(int j, int n, int& i, int& pj, bool& slot_thread) {
    using DM = DenseMap<L>;
    constexpr int S = PpoDims<L>::kRawSlots, T = DM::kDenseThreads;
    const int n4 = net_off(L, 4).total;
    int p = -1;
    pj = 0;
    if (j < T) { DM::map(j, 4, pj, p); i = p < 0 ? n : p; }
    else if (j < 2 * T) { DM::map(j - T, 1, pj, p); pj += S; i = p < 0 ? n : n4 + p; }
    else i = j - 2 * T < 4 ? n - 4 + (j - 2 * T) : n;
    slot_thread = j < 2 * T;
}

// chunks = workgroups per net of the gradient launch, Gw = chain waves per net (2 G): the same for every member
template <int L>
__global__ void __launch_bounds__(kApplyThreads, 2) ppo_population_reduce_kernel(const PopMember* __restrict__ table, int chunks, int Gw, int partial_bf16) {
    const PopMember& M = table[blockIdx.y];
    const PpoCtrl* c = M.ctrl;
    const int stop_flag = c->stop;       // set by an EARLIER launch: uniform over the member's workgroups
    const int adam_t = c->adam_t;
    const bool last_block = blockIdx.x == gridDim.x - 1;
    if (last_block && threadIdx.x == 0) {   // as they stand before this minibatch: the step launch's last block rewrites the originals
        int* snap = reinterpret_cast<int*>(M.mb + 4);
        snap[0] = stop_flag;
        snap[1] = adam_t;
    }
    if (stop_flag) return;  // SB3: no update after the early stop (and nothing is accumulated)
    ApplyArgs a{};
    a.n = ppo_num_params(L);
    a.partial = reinterpret_cast<const float*>(M.partial);
    a.partial_bf16 = partial_bf16;
    a.partial_raw = 2 * PpoDims<L>::kRawSlots;
    a.owner_from = 2 * DenseMap<L>::kDenseThreads;
    a.chunks = chunks;
    a.wave_out = M.b.wave_out;
    a.Gw = Gw;
    a.ent_coef = M.b.ent_coef;
    const int n = a.n;
    const int j = blockIdx.x * kApplyThreads + threadIdx.x;
    int i, pj;
    bool slot_thread;
    population_thread_map<L>(j, n, i, pj, slot_thread);
    __shared__ float red[8];
    const float g = reduce_grad_element(a, i, pj, slot_thread, red);
    M.grad[j] = g;
    double sq = (double)g * g, unused = 0.0;
    block_sum2_f64<kApplyThreads>(sq, unused);
    if (threadIdx.x == 0) M.sq[blockIdx.x] = (float)sq;   // the float the twin's barrier word carries
    if (last_block && threadIdx.x < 4) M.mb[threadIdx.x] = red[4 + threadIdx.x];
}

template <int L>
__global__ void __launch_bounds__(kApplyThreads, 2) ppo_population_step_kernel(const PopMember* __restrict__ table) {
    const PopMember& M = table[blockIdx.y];
    PpoCtrl* c = M.ctrl;
    const int* snap = reinterpret_cast<const int*>(M.mb + 4);
    if (snap[0]) return;                 // stopped by an earlier minibatch: the reduce launch wrote nothing else
    const int adam_t = snap[1];
    const float lr_dev = c->lr;
    const int n = ppo_num_params(L);
    const int j = blockIdx.x * kApplyThreads + threadIdx.x;
    int i, pj;
    bool slot_thread;
    population_thread_map<L>(j, n, i, pj, slot_thread);
    const bool last_block = blockIdx.x == gridDim.x - 1;
    const bool owns = i < n;
    const float m_in = owns ? M.m[i] : 0.0f, v_in = owns ? M.v[i] : 0.0f, th_in = owns ? M.theta[i] : 0.0f;
    const float g = M.grad[j];
    // the squared norm: every workgroup forms it itself, in the order of the twin's barrier master
    __shared__ float nsq_s;
    if (threadIdx.x < 64) {
        double total = 0.0;
        for (int q = threadIdx.x; q < (int)gridDim.x; q += 64) total += (double)M.sq[q];
        total = wave_sum_f64(total);
        if (threadIdx.x == 0) nsq_s = (float)total;
    }
    __syncthreads();
    const float norm_sq = nsq_s;
    const float kl_sum = M.mb[2];
    const bool stop_now = M.kl_limit > 0.0f && kl_sum > M.kl_limit;   // SB3: checked BEFORE the optimiser step of this minibatch
    const bool finite = norm_sq <= 3.0e38f;                           // false for inf and NaN
    if (!stop_now && finite && i < n) {
        const float norm = sqrtf(norm_sq);
        const float clip = fminf(1.0f, M.max_norm / (norm + 1e-6f));  // torch.nn.utils.clip_grad_norm_
        const float gc = g * clip;
        const float mi = M.beta1 * m_in + (1.0f - M.beta1) * gc;
        const float vi = M.beta2 * v_in + (1.0f - M.beta2) * gc * gc;
        M.m[i] = mi;
        M.v[i] = vi;
        const float bc1 = 1.0f - powf(M.beta1, (float)(adam_t + 1));
        const float bc2_sqrt = sqrtf(1.0f - powf(M.beta2, (float)(adam_t + 1)));
        const float lr = lr_dev;
        const float th = th_in - (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + M.eps);  // torch.optim.Adam
        M.theta[i] = th;
        const int n4 = net_off(L, 4).total, n1 = net_off(L, 1).total;
        half8* images = const_cast<half8*>(M.b.images);
        if (i < n4) pack_scatter<L>(reinterpret_cast<_Float16*>(images), 4, i, th);
        else if (i < n4 + n1) pack_scatter<L>(reinterpret_cast<_Float16*>(images + PpoDims<L>::kImage), 1, i - n4, th);
    }
    if (last_block && threadIdx.x == 0) {
        if (M.b.stats)
            for (int q = 0; q < 4; ++q) M.b.stats[q] += M.mb[q];
        if (stop_now) c->stop = 1;
        else if (finite) { c->applied += 1; c->adam_t = adam_t + 1; }
        else c->skipped_nonfinite += 1;
    }
}

}  // namespace qr

// ------------------------------------------------------------------------------------------------------------------------
struct qr_ppo_population {
    std::vector<qr_ppo*> members;   // borrowed
    int L = 0, device = 0;
    bool partial_bf16 = true, epoch_graph = true;
    int workgroups = 0;             // of one member in the reduce / step launches
    qr::PopMember* d_table = nullptr;
    float* d_scratch = nullptr;     // [members][scratch_floats]: grad | sq | mb
    size_t scratch_floats = 0;
    // what d_table holds and what the cached graph was captured for
    std::vector<qr::PopMember> h_table;
    bool table_valid = false;
    hipGraphExec_t exec = nullptr;
    std::vector<unsigned long long> g_seeds;
    int g_B = 0, g_M = 0, g_E = 0, g_shuffle = 0;
    hipStream_t capture_stream = nullptr;
    void* prepare = nullptr;        // what qr_ppo_population_prepare owns (quadrace_population_prepare.hip), released with the object
};

namespace qr {   // what quadrace_population_prepare.hip needs of the object
int population_size(const qr_ppo_population* pop) { return pop ? (int)pop->members.size() : 0; }
int population_obs_len(const qr_ppo_population* pop) { return pop ? pop->L : -1; }
int population_device(const qr_ppo_population* pop) { return pop ? pop->device : -1; }
qr_ppo* population_member(const qr_ppo_population* pop, int p) { return pop->members[(size_t)p]; }
void*& population_prepare_slot(qr_ppo_population* pop) { return pop->prepare; }
}  // namespace qr

namespace {

int popfail(int code, const std::string& m) { return qr::set_last_error(code, m); }

#define POP_HIP(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess) return popfail(QR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

template <typename F>
int dispatch_L(int L, F&& f) {
    return qr::dispatch_L(L, f, [] { return popfail(QR_E_INVALID, "qr_ppo_population: the members' obs_len is not an observation length of the envs"); });
}

template <int L>
struct PopOps {
    using D = qr::PpoDims<L>;
    static constexpr size_t kLdsFused = ((size_t)D::kImage + qr::kExHalf8) * 16 + 7 * qr::kStashRows * sizeof(float);   // = PpoOps<L>::kLdsFused
    static constexpr int kThreads = 2 * qr::DenseMap<L>::kDenseThreads + 4;
    static constexpr int kWorkgroups = (kThreads + qr::kApplyThreads - 1) / qr::kApplyThreads;
    static int configure(const qr_ppo_population* pop) {
        if (pop->partial_bf16) POP_HIP((qr::configure_dynamic_lds<qr::ppo_population_grad_kernel<L, __bf16>>(kLdsFused)));
        else POP_HIP((qr::configure_dynamic_lds<qr::ppo_population_grad_kernel<L, float>>(kLdsFused)));
        return QR_OK;
    }
    // minibatch k of every member: three launches
    static int minibatch(const qr_ppo_population* pop, int B, int k, hipStream_t st) {
        const int P = (int)pop->members.size();
        const int G = (B + 63) / 64, pairs = (G + 1) / 2;
        const int wgs = pairs < qr_ppo::kFusedChunks ? pairs : qr_ppo::kFusedChunks;
        if (pop->partial_bf16)
            hipLaunchKernelGGL((qr::ppo_population_grad_kernel<L, __bf16>), dim3(wgs, 2, P), dim3(512), kLdsFused, st, pop->d_table, k);
        else
            hipLaunchKernelGGL((qr::ppo_population_grad_kernel<L, float>), dim3(wgs, 2, P), dim3(512), kLdsFused, st, pop->d_table, k);
        hipLaunchKernelGGL(qr::ppo_population_reduce_kernel<L>, dim3(kWorkgroups, P), dim3(qr::kApplyThreads), 0, st, pop->d_table, wgs, 2 * G,
                           pop->partial_bf16 ? 1 : 0);
        hipLaunchKernelGGL(qr::ppo_population_step_kernel<L>, dim3(kWorkgroups, P), dim3(qr::kApplyThreads), 0, st, pop->d_table);
        POP_HIP(hipGetLastError());
        return QR_OK;
    }
};

}  // namespace

extern "C" {

int qr_ppo_population_create(qr_ppo* const* members, int32_t num_members, qr_ppo_population** out) {
    if (!out) return popfail(QR_E_INVALID, "qr_ppo_population_create: null output");
    *out = nullptr;
    if (!members || num_members < 1 || num_members > qr::kMaxPopulation)
        return popfail(QR_E_INVALID, "qr_ppo_population_create: num_members must be 1..256 and members non-null");
    for (int p = 0; p < num_members; ++p) {
        if (!members[p]) return popfail(QR_E_INVALID, "qr_ppo_population_create: null member handle");
        for (int q = 0; q < p; ++q)
            if (members[q] == members[p]) return popfail(QR_E_INVALID, "qr_ppo_population_create: a handle is listed twice");
        const qr_ppo *a = members[0], *b = members[p];
        if (a->L != b->L || a->device != b->device || a->partial_bf16 != b->partial_bf16 || a->epoch_graph != b->epoch_graph)
            return popfail(QR_E_INVALID, "qr_ppo_population_create: the members must share obs_len, device and flags");
    }
    qr_ppo_population* pop = new qr_ppo_population();
    pop->members.assign(members, members + num_members);
    pop->L = members[0]->L;
    pop->device = members[0]->device;
    pop->partial_bf16 = members[0]->partial_bf16;
    pop->epoch_graph = members[0]->epoch_graph;
    const int rc = dispatch_L(pop->L, [&](auto Lc) {
        pop->workgroups = PopOps<decltype(Lc)::value>::kWorkgroups;
        return (int)QR_OK;
    });
    if (rc != QR_OK) { delete pop; return rc; }
    pop->scratch_floats = (size_t)pop->workgroups * qr::kApplyThreads + (size_t)((pop->workgroups + 63) / 64 * 64) + 8;
    hipError_t e = hipSetDevice(pop->device);
    if (e == hipSuccess) e = hipMalloc((void**)&pop->d_table, sizeof(qr::PopMember) * (size_t)num_members);
    if (e == hipSuccess) e = hipMalloc((void**)&pop->d_scratch, sizeof(float) * pop->scratch_floats * (size_t)num_members);
    if (e == hipSuccess) e = hipMemset(pop->d_scratch, 0, sizeof(float) * pop->scratch_floats * (size_t)num_members);
    if (e != hipSuccess) {
        qr_ppo_population_destroy(pop);
        return popfail(QR_E_HIP, std::string("qr_ppo_population_create: ") + hipGetErrorString(e));
    }
    *out = pop;
    return QR_OK;
}

int qr_ppo_population_destroy(qr_ppo_population* pop) {
    if (!pop) return QR_OK;
    (void)hipSetDevice(pop->device);
    (void)hipDeviceSynchronize();
    if (pop->exec) (void)hipGraphExecDestroy(pop->exec);
    if (pop->capture_stream) (void)hipStreamDestroy(pop->capture_stream);
    (void)hipFree(pop->d_table);
    (void)hipFree(pop->d_scratch);
    qr::population_prepare_release(pop->prepare);
    delete pop;
    return QR_OK;
}

int qr_ppo_population_epoch(qr_ppo_population* pop, const qr_ppo_member_args* args, int32_t B, int32_t num_minibatches, int32_t num_epochs,
                            int32_t device_shuffle, void* stream) {
    if (!pop || !args) return popfail(QR_E_INVALID, "qr_ppo_population_epoch: null argument");
    const int P = (int)pop->members.size();
    if (B < 64 || num_minibatches < 1 || num_minibatches > qr_ppo::kMaxEpochMinibatches)
        return popfail(QR_E_INVALID, "qr_ppo_population_epoch: bad minibatch size / count");
    if (num_epochs < 1 || num_epochs > 64 || (num_epochs > 1 && !device_shuffle))
        return popfail(QR_E_INVALID, "qr_ppo_population_epoch: num_epochs > 1 needs device_shuffle (the caller cannot rewrite the permutations in between)");
    for (int p = 0; p < P; ++p) {
        const qr_ppo_member_args& a = args[p];
        if (B > pop->members[p]->max_B) return popfail(QR_E_INVALID, "qr_ppo_population_epoch: B is above a member's max_minibatch");
        if (!a.theta_dev || !a.adam_m_dev || !a.adam_v_dev || !a.obs_dev || !a.act_dev || !a.old_logp_dev || !a.adv_dev || !a.ret_dev || !a.perm_dev)
            return popfail(QR_E_INVALID, "qr_ppo_population_epoch: a member's argument is null");
        if (!(a.lr >= 0.0f)) return popfail(QR_E_INVALID, "qr_ppo_population_epoch: a member's learning rate is negative or NaN");
    }
    POP_HIP(hipSetDevice(pop->device));
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return popfail(QR_E_INVALID, "qr_ppo_population_epoch: `stream` is being captured (the call uploads the member table and launches a graph of its own)");
    // the member table this call needs
    std::vector<qr::PopMember> table((size_t)P);
    std::memset(table.data(), 0, sizeof(qr::PopMember) * (size_t)P);   // padding included: the table is compared bytewise below
    std::vector<unsigned long long> seeds((size_t)P);
    qr::PopLr lrs;
    std::memset(&lrs, 0, sizeof(lrs));
    for (int p = 0; p < P; ++p) {
        qr_ppo* h = pop->members[p];
        const qr_ppo_member_args& a = args[p];
        qr::PopMember& m = table[(size_t)p];
        m.b.obs = a.obs_dev; m.b.act = a.act_dev; m.b.old_logp = a.old_logp_dev; m.b.adv = a.adv_dev; m.b.ret = a.ret_dev;
        m.b.idx = a.perm_dev;
        m.b.B = B; m.b.G = (B + 63) / 64;
        m.b.clip = a.clip; m.b.vf_coef = a.vf_coef; m.b.ent_coef = a.ent_coef;
        m.b.acc = h->d_mbstats;
        m.b.stop = &h->d_ctrl->stop;
        m.b.theta = a.theta_dev;
        m.b.images = h->d_images;
        m.b.wave_out = h->d_wave;
        m.b.stats = a.stats_dev;
        m.partial = h->d_partial;
        m.theta = a.theta_dev; m.m = a.adam_m_dev; m.v = a.adam_v_dev;
        m.ctrl = h->d_ctrl;
        m.max_norm = a.max_grad_norm; m.beta1 = a.beta1; m.beta2 = a.beta2; m.eps = a.eps;
        m.kl_limit = h->target_kl > 0.0f ? 1.5f * h->target_kl * (float)B : 0.0f;
        float* scratch = pop->d_scratch + (size_t)p * pop->scratch_floats;
        m.grad = scratch;
        m.sq = scratch + (size_t)pop->workgroups * qr::kApplyThreads;
        m.mb = m.sq + (pop->workgroups + 63) / 64 * 64;
        seeds[(size_t)p] = h->shuffle_seed;
        lrs.v[p] = a.lr;
    }
    const bool same_table = pop->table_valid && std::memcmp(table.data(), pop->h_table.data(), sizeof(qr::PopMember) * (size_t)P) == 0;
    if (!same_table) {
        // stream-ordered behind whatever earlier calls left on `st`; synchronised, so the host copy may go
        POP_HIP(hipMemcpyAsync(pop->d_table, table.data(), sizeof(qr::PopMember) * (size_t)P, hipMemcpyHostToDevice, st));
        POP_HIP(hipStreamSynchronize(st));
        pop->h_table = table;
        pop->table_valid = true;
    }
    hipLaunchKernelGGL(qr::ppo_population_lr_kernel, dim3(1), dim3(qr::kMaxPopulation), 0, st, pop->d_table, P, lrs);
    POP_HIP(hipGetLastError());
    for (int p = 0; p < P; ++p) {   // the step kernel keeps each member's images in step with its vector; its own epoch table is not armed
        pop->members[p]->packed_theta = args[p].theta_dev;
        pop->members[p]->epoch_idx = nullptr;
    }
    if (int rc = dispatch_L(pop->L, [&](auto Lc) { return PopOps<decltype(Lc)::value>::configure(pop); })) return rc;
    auto enqueue = [&](hipStream_t s) -> int {
        for (int e = 0; e < num_epochs; ++e) {
            for (int p = 0; p < P; ++p)   // per epoch and member: the existing shuffle / table-zeroing / advantage-sum kernels
                if (int rc = qr::ppo_epoch_prologue(pop->members[p], args[p].adv_dev, args[p].perm_dev, B, num_minibatches, device_shuffle, s))
                    return rc;
            for (int k = 0; k < num_minibatches; ++k)
                if (int rc = dispatch_L(pop->L, [&](auto Lc) { return PopOps<decltype(Lc)::value>::minibatch(pop, B, k, s); })) return rc;
        }
        return QR_OK;
    };
    if (!pop->epoch_graph) return enqueue(st);
    const bool hit = pop->exec && same_table && pop->g_B == B && pop->g_M == num_minibatches && pop->g_E == num_epochs &&
                     pop->g_shuffle == device_shuffle && pop->g_seeds == seeds;
    if (!hit) {
        if (pop->exec) { (void)hipGraphExecDestroy(pop->exec); pop->exec = nullptr; }
        if (!pop->capture_stream) POP_HIP(hipStreamCreateWithFlags(&pop->capture_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        POP_HIP(hipStreamBeginCapture(pop->capture_stream, hipStreamCaptureModeRelaxed));
        const int rc = enqueue(pop->capture_stream);
        const hipError_t end = hipStreamEndCapture(pop->capture_stream, &graph);
        if (rc != QR_OK || end != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc != QR_OK ? rc : popfail(QR_E_HIP, std::string("qr_ppo_population_epoch: graph capture failed: ") + hipGetErrorString(end));
        }
        const hipError_t inst = hipGraphInstantiate(&pop->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (inst != hipSuccess) {
            pop->exec = nullptr;
            return popfail(QR_E_HIP, std::string("qr_ppo_population_epoch: hipGraphInstantiate: ") + hipGetErrorString(inst));
        }
        pop->g_B = B; pop->g_M = num_minibatches; pop->g_E = num_epochs; pop->g_shuffle = device_shuffle; pop->g_seeds = seeds;
    }
    POP_HIP(hipGraphLaunch(pop->exec, st));
    return QR_OK;
}

int qr_ppo_population_status(qr_ppo_population* pop, int32_t* out, void* stream) {
    if (!pop || !out) return popfail(QR_E_INVALID, "qr_ppo_population_status: null argument");
    POP_HIP(hipSetDevice(pop->device));
    hipStream_t st = (hipStream_t)stream;
    for (size_t p = 0; p < pop->members.size(); ++p)
        POP_HIP(hipMemcpyAsync(out + 4 * p, &pop->members[p]->d_ctrl->stop, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    POP_HIP(hipStreamSynchronize(st));
    return QR_OK;
}

}  // extern "C"
