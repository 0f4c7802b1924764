// quadrace_ppo_f32.hip -- the PPO minibatch GRADIENT at the reference's precision (round 6; VERDICT r05 item 3, second half).
//
// The reference trains in float32 (SB3 / torch, R:783-795).  ppo_grad_kernel (quadrace_ppo.hip) is the throughput path: every GEMM operand
// rounded to ONE f16 (gradient cosine >= 0.9985 against float32 autograd).  This file is the accuracy path: the same loss, the same
// gradient vector layout, every matrix product on the matrix core with BOTH operands split into THREE bf16 pieces (exactly: 3 x 8 mantissa
// bits, float32's exponent range)
//     a = A0 + A1 + A2,  b = B0 + B1 + B2,   a b ~ A0 B0 + A0 B1 + A1 B0 + A1 B1 + A0 B2 + A2 B0    (six matrix instructions per K-step),
// f32 accumulation -- the idea of the residual MLPs' split first layer (quadrace_device.hpp) and of policy_forward_f32class, as ONE generic
// strided GEMM kernel that serves the forward layers, the backward layers and the weight gradients:
//     C[m][n] = sum_k A(m, k) B(k, n)     A(m, k) = A[rowA(m) sAm + k sAk],  B(k, n) = B[rowB(k) sBk + n sBn]   (+ bias, ReLU, ReLU mask)
// Activations and deltas live in f32 scratch (HBM).  One launch serves the same product of BOTH networks: 11 GEMM launches + 4 reductions + 3
// loss kernels per minibatch, replayed as one cached hipGraph per distinct argument set (187 us per 5 000-row update on MI355X).  The result
// goes to qr_ppo_apply (global-norm clip, Adam, operand re-pack: f32 arithmetic already), like the data-parallel path's gradient.
//   * deltas are kept UNSCALED (the 1 / B of the batch mean is applied when the weight gradients are reduced);
//   * bf16 pieces, not f16: a first version with two f16 pieces per operand (as in the forward kernels) lost the low piece of every value
//     below 0.25 to f16's 2^-24 quantum -- 1e-3 relative on a 40 000-row weight gradient; with three bf16 pieces the cosine against float64
//     autograd is 1 - 1e-13 and the relative error 3e-7 ... 9e-7 (tests/test_gpu_ppo_kernel.py);
//   * no atomics: the weight-gradient GEMMs split K (= the minibatch's rows) over workgroups that write partial tiles, summed in a fixed order.
// Loss conventions = ppo_grad_kernel's (SB3 PPO.train): clipped surrogate with per-minibatch normalised advantages (unbiased std + 1e-8),
// vf_coef * mse, entropy of the state-independent Gaussian; statistics {sum surrogate, sum squared value error, sum approx-kl, clipped count}.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "../../include/quadrace.h"
#include "quadrace_host.hpp"
#include "quadrace_policy.hpp"

struct qr_ppo;
namespace qr {
int ppo_handle_info(const qr_ppo* p, int* L, int* device, int* max_B, int* num_params);  // quadrace_ppo.hip
void** ppo_f32_scratch_slot(qr_ppo* p);                                                  // quadrace_ppo.hip: one hipMalloc'ed block, freed by qr_ppo_destroy
size_t* ppo_f32_scratch_bytes(qr_ppo* p);

constexpr int kHid = kPolHidden;   // 120
constexpr int kF32Slices = 64, kF32Ld = 128;   // split-K layers of a weight gradient; row stride of its partial tiles
void** ppo_f32_graphs_slot(qr_ppo* p);   // quadrace_ppo.hip: owned by the handle, released through ppo_f32_release_graphs
hipStream_t* ppo_capture_stream_slot(qr_ppo* p);
bool ppo_uses_graphs(const qr_ppo* p);
void ppo_f32_release_graphs(void* cache);

struct GemmArgs {
    const float* A; long sAm, sAk; const int* idxA;   // rowA(m) = idxA ? idxA[m] : m
    const float* B; long sBk, sBn; const int* idxB;   // rowB(k) = idxB ? idxB[k] : k
    int b_ones_col;                                   // >= 0: B(k, b_ones_col) = 1 (the bias column of a weight gradient)
    float* C; long sCm;                               // C[m sCm + n]; split-K: slice z at C + z * c_slice
    long c_slice;
    int M, N, K, k_per_slice;
    const float* bias;                                // epilogue: + bias[n]
    int relu;                                         // epilogue: max(., 0)
    const float* mask; long sMask;                    // epilogue: 0 where mask[m sMask + n] <= 0 (ReLU derivative from the stored activation)
};

// Three bf16 pieces: x = X0 + X1 + X2 EXACTLY (8 + 8 + 8 mantissa bits, float32's exponent range -- every difference below is exact in
// f32).  The gradient path uses bf16 where the forward kernels use two f16 pieces: deltas and small activations (|x| < 0.25) would fall
// below f16's 2^-24 quantum in their low piece (measured: 1e-3 relative on a 40 000-row weight gradient), bf16 has no such floor.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split8(const float* v, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        p0[j] = (__bf16)v[j];
        const float r1 = v[j] - (float)p0[j];
        p1[j] = (__bf16)r1;
        p2[j] = (__bf16)(r1 - (float)p1[j]);
    }
}

// One launch serves the same layer of BOTH networks (the policy's and the value function's chains are independent).
struct GemmPair { GemmArgs g[2]; int slices; };   // blockIdx.z = net * slices + K slice

// 256 threads = 4 waves = ONE 32 x 32 tile of C (blockIdx.x: column tile, blockIdx.y: row tile), network and K slice blockIdx.z.  The slice's
// K-steps go round the 4 waves -- a layer (K <= 120, one slice) is a chain of 2 K-steps per wave, a weight gradient (K = the minibatch's rows,
// >= 256 rows per slice) of >= 4 -- and the 4 accumulators are summed through LDS in wave order.
__global__ void __launch_bounds__(256) gemm_f32class_kernel(GemmPair pr) {
    const int z_net = blockIdx.z / pr.slices, z_slice = blockIdx.z - z_net * pr.slices;
    const GemmArgs& g = pr.g[z_net];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tm = blockIdx.y, tn = blockIdx.x;
    if (tm * 32 >= g.M) return;                               // workgroup-uniform
    const int c = lane & 31, h = lane >> 5;
    const int m = tm * 32 + c, n = tn * 32 + c;
    const bool m_ok = m < g.M, n_ok = n < g.N;
    const long rowA = m_ok ? (long)(g.idxA ? g.idxA[m] : m) * g.sAm : 0;
    const int k_lo = z_slice * g.k_per_slice;
    const int k_hi = min(g.K, k_lo + g.k_per_slice);
    const f32x16p zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    f32x16p acc = zero;
    // operands of one K-step: this lane's 8 k-slots (k0 + 8 h + j).  Contiguous-in-k operands (sAk / sBk == 1: the forward layers' inputs and
    // weights, the backward layers' deltas; rows are 32-byte aligned by construction) come as two 16-byte loads, everything else as eight
    // 4-byte loads that are coalesced across the lanes (consecutive lanes = consecutive m / n).
    const bool a_vec = g.sAk == 1 && (g.sAm & 7) == 0 && (reinterpret_cast<uintptr_t>(g.A) & 15) == 0;
    const bool b_vec = g.sBk == 1 && g.idxB == nullptr && (g.sBn & 7) == 0 && g.b_ones_col < 0 && (reinterpret_cast<uintptr_t>(g.B) & 15) == 0;
    auto load = [&](int k0, float* a, float* b) {
        const int kb = k0 + 8 * h;
        if (a_vec && m_ok && kb + 8 <= k_hi) {
            const float4 u = *reinterpret_cast<const float4*>(g.A + rowA + kb), v = *reinterpret_cast<const float4*>(g.A + rowA + kb + 4);
            a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w; a[4] = v.x; a[5] = v.y; a[6] = v.z; a[7] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = (m_ok && kb + j < k_hi) ? g.A[rowA + (long)(kb + j) * g.sAk] : 0.0f;
        }
        if (b_vec && n_ok && kb + 8 <= k_hi) {
            const float* q = g.B + (long)n * g.sBn + kb;
            const float4 u = *reinterpret_cast<const float4*>(q), v = *reinterpret_cast<const float4*>(q + 4);
            b[0] = u.x; b[1] = u.y; b[2] = u.z; b[3] = u.w; b[4] = v.x; b[5] = v.y; b[6] = v.z; b[7] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kb + j;
                float bv = 0.0f;
                if (n_ok && k < k_hi) {
                    if (n == g.b_ones_col) bv = 1.0f;
                    else bv = g.B[(long)(g.idxB ? g.idxB[k] : k) * g.sBk + (long)n * g.sBn];
                }
                b[j] = bv;
            }
        }
    };
    constexpr int kStride = 64;
    const int k_first = k_lo + 16 * wave;
    float a[8], b[8], an[8], bn[8];
    if (k_first < k_hi) load(k_first, a, b);
    for (int k0 = k_first; k0 < k_hi; k0 += kStride) {
        const bool more = k0 + kStride < k_hi;
        if (more) load(k0 + kStride, an, bn);     // the next K-step's loads fly while this one is split and multiplied
        bf16x8 a0, a1, a2, b0, b1, b2;
        split8(a, a0, a1, a2);
        split8(b, b0, b1, b2);
        // a b = sum of the piece products down to 2^-16 of the leading one (the dropped a1 b2, a2 b1, a2 b2 are <= 2^-23 |a b|); small terms first
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
        if (more) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] = an[j]; b[j] = bn[j]; }
        }
    }
    float* C = g.C + (long)z_slice * g.c_slice;
    const float bias = (g.bias && n_ok) ? g.bias[n] : 0.0f;
    auto finish = [&](int r, float sum) {   // lane l, register r: row (r & 3) + 8 (r >> 2) + 4 h of the tile, column c
        const int mm = tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (mm >= g.M || !n_ok) return;
        float v = sum + bias;
        if (g.relu) v = fmaxf(v, 0.0f);
        if (g.mask && !(g.mask[(long)mm * g.sMask + n] > 0.0f)) v = 0.0f;
        C[(long)mm * g.sCm + n] = v;
    };
    __shared__ float red[4][16][64];
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {        // wave w finishes registers 4 w .. 4 w + 3
        const int r = 4 * wave + j;
        finish(r, ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane]);
    }
}

// sum and sum of squares of the minibatch's advantages, one workgroup, fixed order -> acc[0..1] (double)
__global__ void __launch_bounds__(1024) f32_adv_stats_kernel(const float* __restrict__ adv, const int* __restrict__ idx, int B, double* __restrict__ acc) {
    __shared__ double s1[1024], s2[1024];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < B; i += 1024) {
        const double v = (double)adv[idx[i]];
        a += v; b += v * v;
    }
    s1[threadIdx.x] = a; s2[threadIdx.x] = b;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { s1[threadIdx.x] += s1[threadIdx.x + off]; s2[threadIdx.x] += s2[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { acc[0] = s1[0]; acc[1] = s2[0]; }
}

// per-sample loss gradients (UNSCALED: x B) from the two networks' outputs; per-workgroup partial sums of d log_std and the statistics
struct LossArgs {
    const float *mean, *value;          // [B][4] (policy output), [B][4] (value output in column 0)
    const float *act, *old_logp, *adv, *ret, *log_std;
    const int* idx;
    const double* adv_acc;
    int B;
    float clip, vf_coef;
    float *d_mean, *d_value;            // [B][4], [B][4] (column 0)
    float* partial;                     // [blocks][8]: d log_std[4], surrogate, squared value error, approx kl, clipped
};
__global__ void __launch_bounds__(256) f32_loss_kernel(LossArgs a) {
    __shared__ float red[8][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float t[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (i < a.B) {
        const int row = a.idx[i];
        const double amean = a.adv_acc[0] / a.B;
        const double avar = fmax((a.adv_acc[1] - a.B * amean * amean) / (a.B > 1 ? a.B - 1 : 1), 0.0);
        const float A = (a.adv[row] - (float)amean) * (float)(1.0 / (sqrt(avar) + 1e-8));
        float z[4], inv_std[4], logp = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ls = a.log_std[k];
            inv_std[k] = expf(-ls);
            z[k] = (a.act[(size_t)row * 4 + k] - a.mean[(size_t)i * 4 + k]) * inv_std[k];
            logp += -0.5f * z[k] * z[k] - ls - 0.9189385332046727f;
        }
        const float log_ratio = logp - a.old_logp[row];
        const float ratio = expf(log_ratio);
        const bool flows = A >= 0.0f ? (ratio <= 1.0f + a.clip) : (ratio >= 1.0f - a.clip);
        const float gl = flows ? -A * ratio : 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a.d_mean[(size_t)i * 4 + k] = gl * z[k] * inv_std[k];
            t[k] = gl * (z[k] * z[k] - 1.0f);
        }
        const float clipped_ratio = fminf(fmaxf(ratio, 1.0f - a.clip), 1.0f + a.clip);
        t[4] = -fminf(A * ratio, A * clipped_ratio);
        t[6] = (ratio - 1.0f) - log_ratio;
        t[7] = fabsf(ratio - 1.0f) > a.clip ? 1.0f : 0.0f;
        const float err = a.value[(size_t)i * 4] - a.ret[row];
        a.d_value[(size_t)i * 4 + 0] = a.vf_coef * 2.0f * err;
        a.d_value[(size_t)i * 4 + 1] = 0.0f; a.d_value[(size_t)i * 4 + 2] = 0.0f; a.d_value[(size_t)i * 4 + 3] = 0.0f;
        t[5] = err * err;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[k][threadIdx.x] = t[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int k = 0; k < 8; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 8) a.partial[(size_t)blockIdx.x * 8 + threadIdx.x] = red[threadIdx.x][0];
}

// log_std gradient + statistics from the loss kernel's per-workgroup sums (one wave, fixed order)
__global__ void __launch_bounds__(64) f32_finish_kernel(const float* __restrict__ partial, int blocks, int B, float ent_coef, float* __restrict__ grad,
                                                        int num_params, float* __restrict__ stats) {
    const int k = threadIdx.x;
    if (k >= 8) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += (double)partial[(size_t)b * 8 + k];
    if (k < 4) {
        grad[num_params - 4 + k] = (float)(s / B) - ent_coef;
    } else {
        grad[num_params + (k - 4)] = (float)s;
        if (stats) stats[k - 4] += (float)s;
    }
}

// weight gradient of one layer (both networks: blockIdx.y) from its split-K partial tiles: dW[out][in] and db[out] (column `in` of the
// partial) x 1 / B, fixed order
struct ReduceArgs { const float* partial[2]; int out_dim[2]; float* gw[2]; float* gb[2]; int slices; long slice_stride; int in_dim, ld; float scale; };
__global__ void __launch_bounds__(256) f32_dw_reduce_kernel(ReduceArgs a) {
    const int net = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.out_dim[net] * (a.in_dim + 1)) return;
    const int m = e / (a.in_dim + 1), n = e % (a.in_dim + 1);
    const float* partial = a.partial[net];
    const float* q = partial + (size_t)m * a.ld + n;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;   // four interleaved chains (the loads of one round fly together), fixed order
    int z = 0;
    for (; z + 4 <= a.slices; z += 4) {
        s0 += q[(size_t)z * a.slice_stride]; s1 += q[(size_t)(z + 1) * a.slice_stride];
        s2 += q[(size_t)(z + 2) * a.slice_stride]; s3 += q[(size_t)(z + 3) * a.slice_stride];
    }
    for (; z < a.slices; ++z) s0 += q[(size_t)z * a.slice_stride];
    float s = ((s0 + s1) + (s2 + s3)) * a.scale;
    if (n < a.in_dim) a.gw[net][(size_t)m * a.in_dim + n] = s;
    else a.gb[net][m] = s;
}

}  // namespace qr

namespace {

struct NetOff32 { int w[4], b[4], total; };
NetOff32 net_off32(int L, int O) {   // = net_off() of quadrace_ppo.hip: [w1 b1 w2 b2 w3 b3 w4 b4]
    NetOff32 o;
    const int H = qr::kHid;
    const int in[4] = {L, H, H, H}, out[4] = {H, H, H, O};
    int p = 0;
    for (int l = 0; l < 4; ++l) { o.w[l] = p; p += out[l] * in[l]; o.b[l] = p; p += out[l]; }
    o.total = p;
    return o;
}

void launch_gemm(const qr::GemmArgs& g0, const qr::GemmArgs& g1, int slices, hipStream_t st) {
    qr::GemmPair pr;
    pr.g[0] = g0; pr.g[1] = g1; pr.slices = slices;
    const int M = g0.M > g1.M ? g0.M : g1.M, N = g0.N > g1.N ? g0.N : g1.N;
    const int tiles_m = (M + 31) / 32;
    // every product in the wave-K form: a layer is one slice, a weight gradient `slices` of them over blockIdx.z
    hipLaunchKernelGGL(qr::gemm_f32class_kernel, dim3((N + 31) / 32, tiles_m, 2 * slices), dim3(256), 0, st, pr);
}

// One call's arguments: the key of its cached graph (the launches address nothing else that changes from call to call).
struct GradCall {
    const float *theta, *obs, *act, *old_logp, *adv, *ret; const int32_t* idx; int32_t B; float clip, vf_coef, ent_coef; float *grad, *stats;
    bool operator==(const GradCall& o) const {
        return theta == o.theta && obs == o.obs && act == o.act && old_logp == o.old_logp && adv == o.adv && ret == o.ret && idx == o.idx && B == o.B &&
               clip == o.clip && vf_coef == o.vf_coef && ent_coef == o.ent_coef && grad == o.grad && stats == o.stats;
    }
};
struct GraphCache {
    static constexpr size_t kMax = 256;   // a training loop revisits the same (minibatch offset, buffers) set every epoch; beyond this the oldest goes
    std::vector<std::pair<GradCall, hipGraphExec_t>> entries;
    size_t next_victim = 0;
};

// the launches of one gradient evaluation, in order, on `st`
void enqueue_grad(const GradCall& c, int L, int max_B, int np, float* base, hipStream_t st) {
    const int H = qr::kHid, B = c.B;
    constexpr int kSlices = qr::kF32Slices, kLd = qr::kF32Ld;
    const size_t R = (size_t)max_B, n_h = R * H, n_o = R * 4;
    float* Hn[2][3]; float* OUT[2]; float* DA[2]; float* DB[2]; float* D4[2]; float* PART[2];
    float* q = base;
    for (int net = 0; net < 2; ++net) {
        for (int l = 0; l < 3; ++l) { Hn[net][l] = q; q += n_h; }
        OUT[net] = q; q += n_o;
        DA[net] = q; q += n_h;
        DB[net] = q; q += n_h;
        D4[net] = q; q += n_o;
        PART[net] = q; q += (size_t)kSlices * H * kLd;
    }
    float* LOSSP = q; q += ((R + 255) / 256) * 8;
    double* ADV = reinterpret_cast<double*>(q);   // 8-byte aligned: every block above is a multiple of 2 floats
    const int outs[2] = {4, 1};
    const NetOff32 off[2] = {net_off32(L, 4), net_off32(L, 1)};
    const float* th[2] = {c.theta, c.theta + off[0].total};
    const float* log_std = c.theta + off[0].total + off[1].total;
    const int in[4] = {L, H, H, H};
    // ---- forward, both nets per launch
    for (int l = 0; l < 4; ++l) {
        qr::GemmArgs g[2];
        for (int net = 0; net < 2; ++net) {
            g[net] = qr::GemmArgs{};
            if (l == 0) { g[net].A = c.obs; g[net].sAm = L; g[net].sAk = 1; g[net].idxA = c.idx; }
            else { g[net].A = Hn[net][l - 1]; g[net].sAm = H; g[net].sAk = 1; }
            g[net].B = th[net] + off[net].w[l]; g[net].sBk = 1; g[net].sBn = in[l]; g[net].b_ones_col = -1;      // B(k, n) = W[n][k]
            g[net].C = l < 3 ? Hn[net][l] : OUT[net]; g[net].sCm = l < 3 ? H : 4;
            g[net].M = B; g[net].N = l < 3 ? H : outs[net]; g[net].K = in[l]; g[net].k_per_slice = in[l];
            g[net].bias = th[net] + off[net].b[l]; g[net].relu = l < 3;
        }
        launch_gemm(g[0], g[1], 1, st);
    }
    // ---- loss
    hipLaunchKernelGGL(qr::f32_adv_stats_kernel, dim3(1), dim3(1024), 0, st, c.adv, c.idx, B, ADV);
    qr::LossArgs la{};
    la.mean = OUT[0]; la.value = OUT[1]; la.act = c.act; la.old_logp = c.old_logp; la.adv = c.adv; la.ret = c.ret; la.log_std = log_std;
    la.idx = c.idx; la.adv_acc = ADV; la.B = B; la.clip = c.clip; la.vf_coef = c.vf_coef; la.d_mean = D4[0]; la.d_value = D4[1]; la.partial = LOSSP;
    const int lblocks = (B + 255) / 256;
    hipLaunchKernelGGL(qr::f32_loss_kernel, dim3(lblocks), dim3(256), 0, st, la);
    hipLaunchKernelGGL(qr::f32_finish_kernel, dim3(1), dim3(64), 0, st, LOSSP, lblocks, B, c.ent_coef, c.grad, np, c.stats);
    // ---- backward + weight gradients, layer 4 down to 1, both nets per launch
    // >= 256 rows per slice (4 K-steps per wave), at most kSlices slices: few enough partial tiles that their traffic stays below the operands'
    int k_per_slice = (((B + kSlices - 1) / kSlices) + 63) / 64 * 64;
    if (k_per_slice < 256) k_per_slice = 256;
    const int slices = (B + k_per_slice - 1) / k_per_slice;
    const float* delta[2] = {D4[0], D4[1]};     // [B][ld_delta]
    int ld_delta = 4;
    for (int l = 3; l >= 0; --l) {
        // dW_l [out][in + 1] = delta^T x [h_(l-1) | 1], K = the minibatch's rows, split over `slices` workgroup layers
        qr::GemmArgs g[2];
        qr::ReduceArgs r{};
        for (int net = 0; net < 2; ++net) {
            const int out = l < 3 ? H : outs[net];
            float* gnet = c.grad + (net == 0 ? 0 : off[0].total);
            g[net] = qr::GemmArgs{};
            g[net].A = delta[net]; g[net].sAm = 1; g[net].sAk = ld_delta;                              // A(m = unit, k = row) = delta[row][m]
            if (l == 0) { g[net].B = c.obs; g[net].sBk = L; g[net].sBn = 1; g[net].idxB = c.idx; }
            else { g[net].B = Hn[net][l - 1]; g[net].sBk = H; g[net].sBn = 1; }
            g[net].b_ones_col = in[l];
            g[net].C = PART[net]; g[net].sCm = kLd; g[net].c_slice = (long)H * kLd;
            g[net].M = out; g[net].N = in[l] + 1; g[net].K = B; g[net].k_per_slice = k_per_slice;
            r.partial[net] = PART[net]; r.out_dim[net] = out; r.gw[net] = gnet + off[net].w[l]; r.gb[net] = gnet + off[net].b[l];
        }
        launch_gemm(g[0], g[1], slices, st);
        r.slices = slices; r.slice_stride = (long)H * kLd; r.in_dim = in[l]; r.ld = kLd; r.scale = 1.0f / (float)B;
        hipLaunchKernelGGL(qr::f32_dw_reduce_kernel, dim3((H * (in[l] + 1) + 255) / 256, 2), dim3(256), 0, st, r);
        if (l == 0) break;
        // delta_(l-1) [B][in] = (delta_l [B][out] x W_l [out][in]) where h_(l-1) > 0
        qr::GemmArgs b[2];
        for (int net = 0; net < 2; ++net) {
            const int out = l < 3 ? H : outs[net];
            b[net] = qr::GemmArgs{};
            b[net].A = delta[net]; b[net].sAm = ld_delta; b[net].sAk = 1;
            b[net].B = th[net] + off[net].w[l]; b[net].sBk = in[l]; b[net].sBn = 1; b[net].b_ones_col = -1;   // B(k = out unit, n = in unit) = W[k][n]
            float* dst = (delta[net] == DA[net]) ? DB[net] : DA[net];
            b[net].C = dst; b[net].sCm = H;
            b[net].M = B; b[net].N = in[l]; b[net].K = out; b[net].k_per_slice = out;
            b[net].mask = Hn[net][l - 1]; b[net].sMask = H;
        }
        launch_gemm(b[0], b[1], 1, st);
        for (int net = 0; net < 2; ++net) delta[net] = b[net].C;
        ld_delta = H;
    }
}

}  // namespace

namespace qr {
void ppo_f32_release_graphs(void* cache) {   // qr_ppo_destroy
    GraphCache* gc = static_cast<GraphCache*>(cache);
    if (!gc) return;
    for (auto& e : gc->entries) (void)hipGraphExecDestroy(e.second);
    delete gc;
}
}  // namespace qr

extern "C" {

int qr_ppo_grad_f32class(qr_ppo* p, const float* theta_dev, const float* obs_dev, const float* act_dev, const float* old_logp_dev,
                         const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B, float clip, float vf_coef,
                         float ent_coef, float* grad_out_dev, float* stats_dev, void* stream) {
    int L = 0, device = 0, max_B = 0, np = 0;
    if (!p || qr::ppo_handle_info(p, &L, &device, &max_B, &np) != QR_OK) return qr::set_last_error(QR_E_INVALID, "qr_ppo_grad_f32class: null handle");
    if (!theta_dev || !obs_dev || !act_dev || !old_logp_dev || !adv_dev || !ret_dev || !idx_dev || !grad_out_dev)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_grad_f32class: null argument");
    if (B < 2 || B > max_B) return qr::set_last_error(QR_E_INVALID, "qr_ppo_grad_f32class: minibatch size must be >= 2 and <= max_minibatch");
    if ((B + 31) / 32 > 65535)   // the layer GEMMs put the 32-row tiles on grid.y
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_grad_f32class: at most 2 097 120 rows per minibatch");
    if (net_off32(L, 4).total + net_off32(L, 1).total + 4 != np) return qr::set_last_error(QR_E_STATE, "qr_ppo_grad_f32class: parameter layout mismatch");
    QR_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const int H = qr::kHid;
    // ---- scratch (one block per handle, sized for max_minibatch), per net: H1 H2 H3 [R][120], OUT [R][4], deltas DA DB [R][120], D4 [R][4],
    //      weight-gradient partial tiles [kF32Slices][120][128]; then the loss partial sums and the advantage sums
    const size_t R = (size_t)max_B;
    const size_t floats = 2 * (5 * R * H + 2 * R * 4 + (size_t)qr::kF32Slices * H * qr::kF32Ld) + ((R + 255) / 256) * 8 + 8;
    void** slot = qr::ppo_f32_scratch_slot(p);
    size_t* have = qr::ppo_f32_scratch_bytes(p);
    if (*slot == nullptr || *have < floats * sizeof(float)) {
        if (*slot) { QR_HIP(hipDeviceSynchronize()); (void)hipFree(*slot); *slot = nullptr; }
        QR_HIP(hipMalloc(slot, floats * sizeof(float)));
        *have = floats * sizeof(float);
    }
    const GradCall call{theta_dev, obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev, idx_dev, B, clip, vf_coef, ent_coef, grad_out_dev, stats_dev};
    // not qr::stream_is_capturing: no NULL-stream test and `== Active`, which differs for an invalidated capture
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool caller_captures = hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
    if (caller_captures || !qr::ppo_uses_graphs(p)) {   // a graph launch cannot be captured: plain nodes into the caller's graph
        enqueue_grad(call, L, max_B, np, static_cast<float*>(*slot), st);
        QR_HIP(hipGetLastError());
        return QR_OK;
    }
    // ~20 dependent launches of microseconds each: replayed as one graph per distinct argument set (a training loop's minibatch
    // offsets into its permutation buffer recur every epoch), captured on first sight
    void** gslot = qr::ppo_f32_graphs_slot(p);
    if (!*gslot) *gslot = new GraphCache();
    GraphCache& gc = *static_cast<GraphCache*>(*gslot);
    hipGraphExec_t exec = nullptr;
    for (auto& e : gc.entries)
        if (e.first == call) { exec = e.second; break; }
    if (!exec) {
        hipStream_t* cap = qr::ppo_capture_stream_slot(p);
        if (!*cap) QR_HIP(hipStreamCreateWithFlags(cap, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        QR_HIP(hipStreamBeginCapture(*cap, hipStreamCaptureModeRelaxed));
        enqueue_grad(call, L, max_B, np, static_cast<float*>(*slot), *cap);
        const hipError_t end = hipStreamEndCapture(*cap, &graph);
        if (end != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return qr::set_last_error(QR_E_HIP, std::string("qr_ppo_grad_f32class: graph capture failed: ") + hipGetErrorString(end));
        }
        const hipError_t inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (inst != hipSuccess) return qr::set_last_error(QR_E_HIP, std::string("qr_ppo_grad_f32class: hipGraphInstantiate: ") + hipGetErrorString(inst));
        if (gc.entries.size() < GraphCache::kMax) {
            gc.entries.emplace_back(call, exec);
        } else {   // the replaced graph may still be running on the caller's stream
            QR_HIP(hipDeviceSynchronize());
            (void)hipGraphExecDestroy(gc.entries[gc.next_victim].second);
            gc.entries[gc.next_victim] = std::make_pair(call, exec);
            gc.next_victim = (gc.next_victim + 1) % GraphCache::kMax;
        }
    }
    QR_HIP(hipGraphLaunch(exec, st));
    return QR_OK;
}

}  // extern "C"
