// quadrace_es.hip -- evolution strategies on the policy bank (qr_es_*): what optimises the quantity the bank evaluator MEASURES (flying-lap
// steps, crashes: integers, not differentiable) instead of the shaped reward PPO climbs.  One generation = P = 2 num_pairs antithetic
// members of ONE actor parameter vector, flown by qr_evaluate_policy_bank on common random numbers, in a fixed number of launches:
//
//   qr_es_noise     ONE launch: the raw noise eps [num_pairs][n] (a diagnostic, and the hook the tests hold the stream's spec by)
//   qr_es_perturb   TWO launches: es_perturb_kernel writes the population matrix theta_pop [P][n] (one Philox block per thread = 4
//                   parameters of both members of a pair, float4 stores); the bank-load kernel of quadrace_population_prepare.hip, its table
//                   pointed at the rows of theta_pop, packs slots first_slot .. first_slot + P - 1 (launch_population_load_bank: the kernel is
//                   SHARED, neither copied nor restated)
//   qr_es_fitness   ONE launch, one workgroup per policy: evaluation records -> 8 summary numbers and one score per policy
//   qr_es_update    ONE launch over n / 4 threads: utilities from the scores (ranks by counting), the gradient estimate with the noise
//                   REGENERATED per thread (nothing of size [pairs][n] is stored or read), weight decay, Adam ascent
//
// The noise of all three is ONE device function, es_noise4.  Plain launches on the caller's stream: no graph, no atomic, no flag, and no
// workgroup waits for another.  The library is built with -ffp-contract=off: every product and sum below is rounded on its own, in the
// order written, which is the order include/quadrace.h states and tests/es_spec.py restates.
#include <cmath>
#include <cstring>

#include "quadrace_ppo_device.hpp"

namespace qr {

constexpr int kEsMaxPairs = 128;     // P = 256 = the table of the one bank-load launch; 256 policies x 256 envs = the 65 536-env launch
constexpr int kEsBlock = 256;
constexpr int kEsUpdateBlock = 64;   // n / 4 threads in all (8 131 at L = 24): one wave per workgroup spreads them over the CUs
// Domain separation (see sampling_entry, quadrace_launch.hpp): the reset stream keys Philox with the env seed itself, the action noise with
// seed ^ (0x9E3779B9, 0x85EBCA6B); the ES noise with seed ^ (kEsTweak0, kEsTweak1), so equal seeds never give the three equal keys.
constexpr uint32_t kEsTweak0 = 0x2545F491u, kEsTweak1 = 0x4F6CDD1Du;

struct EsStream { uint32_t k0, k1, g_lo, g_hi; };   // key and generation words of one (seed, generation)
inline EsStream es_stream(uint64_t seed, uint64_t generation) {
    EsStream s;
    s.k0 = (uint32_t)seed ^ kEsTweak0;
    s.k1 = (uint32_t)(seed >> 32) ^ kEsTweak1;
    s.g_lo = (uint32_t)generation;
    s.g_hi = (uint32_t)(generation >> 32);
    return s;
}

// THE noise: eps[4 q .. 4 q + 3] of pair i = one Philox4x32-10 block, counter (q, i, generation lo, hi), uniforms and Box-Muller exactly
// the action noise's (rollout_policy_kernel's noise_slice): (x0, x1) -> r cos, r sin; (x2, x3) -> the second pair.
__device__ __forceinline__ void es_noise4(uint32_t q, uint32_t i, const EsStream& s, float (&eps)[4]) {
    uint32_t x[4];
    philox4x32_10(q, i, s.g_lo, s.g_hi, s.k0, s.k1, x);
    const float u1a = (float)((x[0] >> 8) + 1u) * 5.9604644775390625e-8f, u2a = u01(x[1]);
    const float u1b = (float)((x[2] >> 8) + 1u) * 5.9604644775390625e-8f, u2b = u01(x[3]);
    const float ra = fast_sqrt(-2.0f * __logf(u1a)), rb = fast_sqrt(-2.0f * __logf(u1b));
    float sa, ca, sb, cb;
    qr_sincos(6.283185307179586f * u2a, sa, ca);
    qr_sincos(6.283185307179586f * u2b, sb, cb);
    eps[0] = ra * ca; eps[1] = ra * sa; eps[2] = rb * cb; eps[3] = rb * sb;
}

// grid (ceil(n4 / 256), num_pairs): thread q of row i
__global__ void __launch_bounds__(kEsBlock) es_noise_kernel(float4* __restrict__ eps_out, int n4, EsStream s) {
    const int q = blockIdx.x * kEsBlock + threadIdx.x;
    if (q >= n4) return;
    float e[4];
    es_noise4((uint32_t)q, blockIdx.y, s, e);
    eps_out[(size_t)blockIdx.y * n4 + q] = make_float4(e[0], e[1], e[2], e[3]);
}

// members 2 i and 2 i + 1: theta + (sigma eps), theta - (sigma eps), two roundings each
__global__ void __launch_bounds__(kEsBlock) es_perturb_kernel(const float4* __restrict__ theta, float sigma, float4* __restrict__ pop, int n4,
                                                              EsStream s) {
    const int q = blockIdx.x * kEsBlock + threadIdx.x;
    if (q >= n4) return;
    float e[4];
    es_noise4((uint32_t)q, blockIdx.y, s, e);
    const float4 t = theta[q];
    const float d0 = sigma * e[0], d1 = sigma * e[1], d2 = sigma * e[2], d3 = sigma * e[3];
    const size_t row = (size_t)(2 * blockIdx.y) * n4 + q;
    pop[row] = make_float4(t.x + d0, t.y + d1, t.z + d2, t.w + d3);
    pop[row + n4] = make_float4(t.x - d0, t.y - d1, t.z - d2, t.w - d3);
}

struct EsWeights { double w_gate, w_crash, w_timeout, w_return, w_lap, no_lap_steps; };

// one workgroup per policy p: rows [p E, (p + 1) E) of the records.  s0..s6 are integer sums (exact in any order); s7 is a double sum in
// the ONE order the header states: chunks of 256 envs, a halving tree inside a chunk, the chunks added in ascending order.
__global__ void __launch_bounds__(kEsBlock) es_fitness_kernel(const int4* __restrict__ rec, const float* __restrict__ recf, int E, EsWeights w,
                                                              double* __restrict__ summary, double* __restrict__ fitness) {
    __shared__ double tree[kEsBlock];
    __shared__ long long part[7][kEsBlock / 64];
    const int p = blockIdx.x, t = threadIdx.x;
    long long s[7] = {0, 0, 0, 0, 0, 0, 0};
    double s7 = 0.0;
    for (int c = 0; c < E / kEsBlock; ++c) {
        const size_t env = (size_t)p * E + (size_t)c * kEsBlock + t;
        const int4* r = rec + env * (QR_EVAL_REC_INTS / 4);
        const int4 a = r[0], l0 = r[1], l1 = r[2], l2 = r[3], l3 = r[4], l4 = r[5];
        // ints [6..13] = lap step sums = (l0.z, l0.w, l1.x .. l1.w, l2.x, l2.y), ints [14..21] = lap counts = (l2.z, l2.w, l3.x .. l3.w, l4.x, l4.y)
        s[0] += a.x; s[1] += a.y; s[2] += a.z;
        s[3] += l2.z; s[4] += l0.z;
        s[5] += (long long)l2.w + l3.x + l3.y + l3.z + l3.w + l4.x + l4.y;
        s[6] += (long long)l0.w + l1.x + l1.y + l1.z + l1.w + l2.x + l2.y;
        tree[t] = recf ? (double)recf[env * QR_EVAL_REC_FLOATS + 1] + (double)recf[env * QR_EVAL_REC_FLOATS] : 0.0;
        __syncthreads();
#pragma unroll
        for (int off = kEsBlock / 2; off > 0; off >>= 1) {
            if (t < off) tree[t] += tree[t + off];
            __syncthreads();
        }
        if (t == 0) s7 += tree[0];
        __syncthreads();   // tree[] is rewritten by the next chunk
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        long long v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((t & 63) == 0) part[k][t >> 6] = v;
    }
    __syncthreads();
    if (t == 0) {
        double d[8];
#pragma unroll
        for (int k = 0; k < 7; ++k) d[k] = (double)(part[k][0] + part[k][1] + part[k][2] + part[k][3]);
        d[7] = s7;
        if (summary)
            for (int k = 0; k < 8; ++k) summary[(size_t)p * 8 + k] = d[k];
        const double lap = d[5] > 0.0 ? d[6] / d[5] : w.no_lap_steps;
        fitness[p] = (w.w_gate * d[0] + w.w_crash * d[1] + w.w_timeout * d[2] + w.w_return * d[7]) / (double)E + w.w_lap * lap;
    }
}

struct EsAdam { float lr, beta1, beta2, omb1, omb2, eps, weight_decay, c1, c2, scale; };

// a NaN score ranks below everything, NaNs among themselves by index
__device__ __forceinline__ bool es_less(double a, double b) { return (a != a) ? (b == b) : (a < b); }
__device__ __forceinline__ bool es_same(double a, double b) { return (a != a) ? (b != b) : (a == b); }

// n4 threads: thread q owns parameters 4 q .. 4 q + 3.  Every workgroup forms the P utilities in LDS (P <= 256: ranks by counting), then
// each thread walks the pairs in ascending order with the regenerated noise.
__global__ void __launch_bounds__(kEsUpdateBlock) es_update_kernel(float4* __restrict__ theta, float4* __restrict__ m, float4* __restrict__ v,
                                                                   const double* __restrict__ fitness, int num_pairs, int shaping, int n4, EsStream s,
                                                                   EsAdam A, float* __restrict__ util) {
    __shared__ double F[2 * kEsMaxPairs];
    __shared__ float u[2 * kEsMaxPairs];
    const int P = 2 * num_pairs, t = threadIdx.x;
    for (int p = t; p < P; p += kEsUpdateBlock) F[p] = fitness[p];
    __syncthreads();
    for (int p = t; p < P; p += kEsUpdateBlock) {
        float up;
        if (shaping == QR_ES_SHAPE_CENTERED_RANK) {
            const double f = F[p];
            int rank = 0;
            for (int k = 0; k < P; ++k) rank += (es_less(F[k], f) || (k < p && es_same(F[k], f))) ? 1 : 0;
            up = __fdiv_rn((float)rank, (float)(P - 1)) - 0.5f;
        } else {
            up = (float)F[p];
        }
        u[p] = up;
        if (util && blockIdx.x == 0) util[p] = up;
    }
    __syncthreads();
    const int q = blockIdx.x * kEsUpdateBlock + t;
    if (q >= n4) return;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < num_pairs; ++i) {
        const float d = u[2 * i] - u[2 * i + 1];
        float e[4];
        es_noise4((uint32_t)q, (uint32_t)i, s, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = g[k] + d * e[k];
    }
    const float4 t4 = theta[q], m4 = m[q], v4 = v[q];
    float th[4] = {t4.x, t4.y, t4.z, t4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float gk = g[k] * A.scale;
        gk = gk - A.weight_decay * th[k];
        mm[k] = A.beta1 * mm[k] + A.omb1 * gk;
        vv[k] = A.beta2 * vv[k] + (A.omb2 * gk) * gk;
        // the quotient and the root correctly rounded (IEEE), as NumPy's: sqrtf, not the __fsqrt_rn of this toolchain's headers, which
        // expands to the native 1-ulp v_sqrt_f32
        th[k] = th[k] + __fdiv_rn(A.lr * (mm[k] * A.c1), sqrtf(vv[k] * A.c2) + A.eps);
    }
    theta[q] = make_float4(th[0], th[1], th[2], th[3]);
    m[q] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    v[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
}

}  // namespace qr

struct qr_es {
    int L = 0, device = 0, num_pairs = 0, n = 0;
    float* d_pop = nullptr;   // [P][n]: the population matrix of a qr_es_perturb call without theta_pop_dev
};

namespace {

bool finite_host(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return (u & 0x7F800000u) != 0x7F800000u;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
int invalid(const char* msg) { return qr::set_last_error(QR_E_INVALID, msg); }

}  // namespace

extern "C" {

int qr_es_create(int32_t obs_len, int32_t device, int32_t num_pairs, qr_es** out) {
    if (!out) return invalid("qr_es_create: null output");
    *out = nullptr;
    if (!qr::dispatch_L(obs_len, [](auto) { return true; }, [] { return false; }))
        return invalid("qr_es_create: obs_len must be an observation length qr_policy_bank_create accepts (13 + 4g, 20 + 4g, or 16)");
    if (num_pairs < 1 || num_pairs > qr::kEsMaxPairs) return invalid("qr_es_create: num_pairs must be in 1..128");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return qr::set_last_error(QR_E_NO_DEVICE, "qr_es_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return invalid("qr_es_create: bad device ordinal");
    QR_HIP(hipSetDevice(device));
    qr_es* es = new qr_es();
    es->L = obs_len;
    es->device = device;
    es->num_pairs = num_pairs;
    es->n = qr::net_off(obs_len, 4).total;
    static_assert(qr::kH % 4 == 0, "n = 120 L + 29 644 is a multiple of 4 for every L");
    if (hipMalloc((void**)&es->d_pop, sizeof(float) * (size_t)es->n * 2 * (size_t)num_pairs) != hipSuccess) {
        delete es;
        return qr::set_last_error(QR_E_HIP, "qr_es_create: hipMalloc failed");
    }
    *out = es;
    return QR_OK;
}

int qr_es_destroy(qr_es* es) {
    if (!es) return QR_OK;
    (void)hipSetDevice(es->device);
    (void)hipDeviceSynchronize();
    if (es->d_pop) (void)hipFree(es->d_pop);
    delete es;
    return QR_OK;
}

int qr_es_num_params(const qr_es* es) { return es ? es->n : invalid("qr_es_num_params: null handle"); }

int qr_es_noise(qr_es* es, uint64_t seed, uint64_t generation, float* eps_dev, void* stream) {
    if (!es || !eps_dev) return invalid("qr_es_noise: null argument");
    if (!aligned16(eps_dev)) return invalid("qr_es_noise: eps_dev must be 16-byte aligned");
    QR_HIP(hipSetDevice(es->device));
    const int n4 = es->n / 4;
    hipLaunchKernelGGL(qr::es_noise_kernel, dim3((n4 + qr::kEsBlock - 1) / qr::kEsBlock, es->num_pairs), dim3(qr::kEsBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(eps_dev), n4, qr::es_stream(seed, generation));
    QR_HIP(hipGetLastError());
    return QR_OK;
}

int qr_es_perturb(qr_es* es, const float* theta_dev, float sigma, uint64_t seed, uint64_t generation, qr_policy_bank* bank, int32_t first_slot,
                  float* theta_pop_dev, void* stream) {
    if (!es || !theta_dev || !bank) return invalid("qr_es_perturb: null argument");
    if (!finite_host(sigma) || !(sigma > 0.0f)) return invalid("qr_es_perturb: sigma must be finite and > 0");
    if (!aligned16(theta_dev) || !aligned16(theta_pop_dev)) return invalid("qr_es_perturb: theta_dev and theta_pop_dev must be 16-byte aligned");
    if (qr::bank_obs_len(bank) != es->L || qr::bank_device(bank) != es->device)
        return invalid("qr_es_perturb: the bank's obs_len or device differs from the handle's");
    const int P = 2 * es->num_pairs;
    if (first_slot < 0 || (long long)first_slot + P > (long long)qr::bank_capacity(bank))
        return invalid("qr_es_perturb: slots [first_slot, first_slot + 2 num_pairs) must lie in [0, capacity)");
    QR_HIP(hipSetDevice(es->device));
    hipStream_t st = (hipStream_t)stream;
    float* pop = theta_pop_dev ? theta_pop_dev : es->d_pop;
    const int n4 = es->n / 4;
    hipLaunchKernelGGL(qr::es_perturb_kernel, dim3((n4 + qr::kEsBlock - 1) / qr::kEsBlock, es->num_pairs), dim3(qr::kEsBlock), 0, st,
                       reinterpret_cast<const float4*>(theta_dev), sigma, reinterpret_cast<float4*>(pop), n4, qr::es_stream(seed, generation));
    QR_HIP(hipGetLastError());
    const float* rows[2 * qr::kEsMaxPairs];
    for (int p = 0; p < P; ++p) rows[p] = pop + (size_t)p * es->n;
    const int rc = qr::launch_population_load_bank(es->L, rows, P, qr::bank_weights_mut(bank), qr::bank_weights_lo_mut(bank), (int)first_slot, st);
    if (rc != QR_OK) return rc;
    qr::bank_mark_set(bank, first_slot, P);
    return QR_OK;
}

int qr_es_fitness(qr_es* es, const int32_t* rec_dev, const float* recf_dev, int32_t envs_per_policy, const qr_es_fitness_weights* w,
                  double* summary_dev, double* fitness_dev, void* stream) {
    if (!es || !rec_dev || !w || !fitness_dev) return invalid("qr_es_fitness: null argument");
    if (envs_per_policy < 256 || envs_per_policy % 256 != 0) return invalid("qr_es_fitness: envs_per_policy must be a multiple of 256 (>= 256)");
    if (!aligned16(rec_dev)) return invalid("qr_es_fitness: rec_dev must be 16-byte aligned");
    QR_HIP(hipSetDevice(es->device));
    qr::EsWeights k;
    k.w_gate = w->w_gate; k.w_crash = w->w_crash; k.w_timeout = w->w_timeout; k.w_return = w->w_return; k.w_lap = w->w_lap;
    k.no_lap_steps = w->no_lap_steps;
    hipLaunchKernelGGL(qr::es_fitness_kernel, dim3(2 * es->num_pairs), dim3(qr::kEsBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4*>(rec_dev), recf_dev, (int)envs_per_policy, k, summary_dev, fitness_dev);
    QR_HIP(hipGetLastError());
    return QR_OK;
}

int qr_es_update(qr_es* es, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const double* fitness_dev, float sigma, uint64_t seed,
                 uint64_t generation, int32_t shaping, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t adam_step,
                 float* util_dev, void* stream) {
    if (!es || !theta_dev || !adam_m_dev || !adam_v_dev || !fitness_dev) return invalid("qr_es_update: null argument");
    if (!finite_host(sigma) || !(sigma > 0.0f)) return invalid("qr_es_update: sigma must be finite and > 0");
    if (!(lr >= 0.0f)) return invalid("qr_es_update: lr must not be negative or NaN");
    if (adam_step < 1) return invalid("qr_es_update: adam_step must be >= 1 (the caller counts the steps)");
    if (shaping != QR_ES_SHAPE_CENTERED_RANK && shaping != QR_ES_SHAPE_NONE) return invalid("qr_es_update: unknown shaping");
    if (!aligned16(theta_dev) || !aligned16(adam_m_dev) || !aligned16(adam_v_dev))
        return invalid("qr_es_update: theta_dev, adam_m_dev and adam_v_dev must be 16-byte aligned");
    QR_HIP(hipSetDevice(es->device));
    qr::EsAdam A;
    A.lr = lr; A.beta1 = beta1; A.beta2 = beta2; A.eps = eps; A.weight_decay = weight_decay;
    A.omb1 = 1.0f - beta1;
    A.omb2 = 1.0f - beta2;
    A.c1 = (float)(1.0 / (1.0 - std::pow((double)beta1, (double)adam_step)));   // the bias corrections: in double on the host, passed as float
    A.c2 = (float)(1.0 / (1.0 - std::pow((double)beta2, (double)adam_step)));
    A.scale = 1.0f / ((float)(2 * es->num_pairs) * sigma);
    const int n4 = es->n / 4;
    hipLaunchKernelGGL(qr::es_update_kernel, dim3((n4 + qr::kEsUpdateBlock - 1) / qr::kEsUpdateBlock), dim3(qr::kEsUpdateBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(theta_dev), reinterpret_cast<float4*>(adam_m_dev), reinterpret_cast<float4*>(adam_v_dev), fitness_dev,
                       es->num_pairs, (int)shaping, n4, qr::es_stream(seed, generation), A, util_dev);
    QR_HIP(hipGetLastError());
    return QR_OK;
}

}  // extern "C"
