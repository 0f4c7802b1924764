// quadrace_ppo.hip -- PPO minibatch update on the gfx950 matrix cores (BASELINE config 5).
//
// The reference trains with SB3's PPO (R:783-795): two separate ReLU MLPs  obs[L] -> 120 -> 120 -> 120 -> {4 | 1}
// (policy mean / value), a state-independent log-std, clipped surrogate + vf_coef * MSE value loss, per-minibatch
// advantage normalisation, global grad-norm clipping, Adam.  With the collect phase fused into one kernel
// (qr_rollout_policy) torch's minibatch update was > 95 % of training time: ~100 small launches around
// 16 k x 120 x 120 GEMMs.  Here one minibatch is two launches (grad, apply) plus one adv_stats launch per EPOCH:
//
//   adv_stats   sum / sum of squares of the advantages of EVERY minibatch of an epoch in one launch (qr_ppo_epoch_begin;
//               SB3 normalises per minibatch; the gradient kernel finishes the maths)
//   grad        ppo_grad_kernel (quadrace_ppo_device.hpp; launched here in its direct mode): a workgroup = 8 waves = 128 samples of one net per pass.  Chain waves 0-3: one 32-sample tile each --
//               forward (f16 MFMA chain of quadrace_policy.hpp), per-sample loss gradients, backward through W^T read out of the SAME
//               LDS image (ds_read_b64_tr_b16); activations h_l and deltas d_l stay in registers in the "lane = sample" form and are
//               published per layer as natural packs to a 64 KB exchange area in LDS.  dW waves 4-7 read them back transposed
//               (lane = unit, k = sample) and form dW_l = d_l^T x h_(l-1): 2 x 2 weight tiles per wave, k = the workgroup's 128
//               samples, plain stores to partial[workgroup][slot] in accumulator order -- bf16 by default (the partials' trip
//               through the fabric is what bounds a 16 384-row update; QR_PPO_PARTIAL_F32 keeps f32) -- widened again and summed in
//               f32 in a fixed order by `apply`.  Biases ride along as the constant-1 unit of every layer.  No atomics anywhere:
//               log-std gradients and loss statistics leave as per-wave sums.
//   apply       ONE kernel: sums the partials and the per-wave sums into the gradient, accumulates its squared norm, crosses a
//               grid-wide barrier (247 co-resident workgroups), then clip scale, torch.optim.Adam arithmetic, and each thread
//               scatters its new parameter as f16 into the operand image of the next minibatch; SB3's target-KL early stop is
//               decided here, on the device, before the step is taken
//   (pack       the gather form of the same image layout: initial images / after external changes of theta;
//    reduce     gradient + minibatch statistics only, for the data-parallel path: qr_ppo_grad -> all-reduce -> qr_ppo_apply)
// The earlier forms of `grad` (rounds 1-2: a two-kernel split through an HBM scratch buffer; a 4-wave fused kernel with one dependent
// chain per wave) are gone since round 6; docs/history/DESIGN_rounds1-4.md describes them.
//
// Operand layouts are those of quadrace_policy.hpp (verified on MI355X with tools/ubench/mfma_layout.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "../../include/quadrace.h"
#include "quadrace_launch.hpp"
#include "quadrace_ppo_device.hpp"

namespace qr {


// ---- pack: f32 parameters -> f16 operand images -----------------------------------------------------------------------
template <int L>
__global__ void __launch_bounds__(256) ppo_pack_kernel(const float* __restrict__ theta, half8* __restrict__ images) {
    using D = PpoDims<L>;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int net = blockIdx.y;
    if (e >= D::kImage) return;
    images[(size_t)net * D::kImage + e] = pack_gather<L>(theta, net, e);   // quadrace_ppo_device.hpp
}

// ---- adv_stats: sum and sum of squares of the advantages of minibatch mb = blockIdx.y, rows idx[mb * B + 0..B), into
// table[mb][0..1] (the table is zeroed by a memset before the launch; the gradient kernel turns the sums into mean / rstd) ----------

// ---- epoch permutation on the device: a keyed bijection instead of a sort ---------------------------------------------------------
// SB3 draws np.random.permutation(rows) per epoch; torch.randperm on the GPU is a radix sort of random keys (0.24 ms for 2 Mi rows:
// 5 % of an epoch of matrix-core updates).  perm[i] = E_k(i) with E_k an 8-round alternating (unbalanced) Feistel network over
// ceil(log2 n) bits, cycle-walked into [0, n): every round XORs one half with a keyed hash of the other, so E_k is a bijection for
// ANY key; the key is (seed, epoch count) -- the count lives on the device (PpoCtrl::shuffle_count, bumped by the statistics kernel
// that follows in the same graph), so a replayed graph shuffles differently every epoch.  O(1) per element, no scratch, 20 us.
__device__ __forceinline__ uint32_t shuffle_mix(uint32_t x, uint32_t k) {
    uint32_t h = x * 0x9E3779B1u + k;
    h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13; h *= 0xC2B2AE3Du; h ^= h >> 16;
    return h;
}
// element i of the permutation of [0, n) keyed by (seed, c)
__device__ __forceinline__ unsigned int shuffle_index(unsigned int i, unsigned int n, unsigned long long seed, unsigned long long c) {
    unsigned int bits = 2;
    while ((1ull << bits) < n) ++bits;
    const unsigned int lb = bits >> 1, rb = bits - lb;
    const unsigned int lmask = (1u << lb) - 1u, rmask = (1u << rb) - 1u;
    uint32_t key[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {   // round keys: SplitMix64-style finaliser of (seed, epoch count, round) -- wave-uniform: scalar code
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (c * 8ull + (unsigned long long)r + 1ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        key[r] = (uint32_t)(z ^ (z >> 31));
    }
    unsigned int x = i;
    do {   // cycle walking: the image of a value < n is revisited until it lands below n again (expected < 2 iterations)
        unsigned int l = x >> rb, r_ = x & rmask;
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
            l ^= shuffle_mix(r_, key[r]) & lmask;
            r_ ^= shuffle_mix(l, key[r + 1]) & rmask;
        }
        x = (l << rb) | r_;
    } while (x >= n);
    return x;
}
__global__ void __launch_bounds__(256) ppo_shuffle_kernel(int* __restrict__ perm, unsigned int n, unsigned long long seed,
                                                          const unsigned long long* __restrict__ count) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    perm[i] = (int)shuffle_index(i, n, seed, *count);
}

// Clears the advantage-sum table ahead of ppo_adv_stats_kernel.  A KERNEL, not hipMemsetAsync: inside qr_ppo_epoch's captured graph
// a memset node was seen to lose its ordering against the kernel nodes around it on REPLAY (ROCm 7.2: whole epochs whose sums
// were cleared mid-accumulation -> non-finite gradients, every update of the epoch skipped; tests/test_gpu_round2.py config-5 loop).
// PpoCtrl::lr <- lr (qr_ppo_epoch): a kernel node, not a host-to-device copy -- the value travels in the kernel arguments, so nothing on
// the host has to outlive the launch, and captured into a caller's graph the node replays the value it was captured with
__global__ void ppo_set_lr_kernel(float* __restrict__ dst, float lr) { *dst = lr; }

__global__ void __launch_bounds__(256) ppo_zero_table_kernel(double* __restrict__ table, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) table[i] = 0.0;
}

// (same-address f64 atomics serialise at ~15 ns each: one pair per 1024-thread block, not one per wave)
__global__ void __launch_bounds__(1024) ppo_adv_stats_kernel(const float* __restrict__ adv, const int* __restrict__ idx, int B,
                                                             double* __restrict__ table, unsigned long long* __restrict__ bump) {
    if (bump && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *bump += 1ull;   // the shuffle kernel BEFORE this launch has read it
    const int i = blockIdx.x * 1024 + threadIdx.x;
    const double x = i < B ? (double)adv[idx[(size_t)blockIdx.y * B + i]] : 0.0;
    double s1 = x, s2 = x * x;
    block_sum2_f64<1024>(s1, s2);
    if (threadIdx.x == 0) {
        unsafeAtomicAdd(table + 2 * blockIdx.y + 0, s1);
        unsafeAtomicAdd(table + 2 * blockIdx.y + 1, s2);
    }
}

// ---- gradient reduction, global norm, clip, Adam, operand re-pack: ONE kernel ----------------------------------------------

template <int L>
__global__ void __launch_bounds__(kApplyThreads, 2) ppo_apply_kernel(ApplyArgs a) {   // <= 256 VGPRs: two workgroups per CU are resident
    PpoCtrl* c = a.ctrl;
    const int stop_flag = c->stop;       // set by an EARLIER launch: uniform over the grid; tested after the reduction below
    const unsigned int gen = c->gen;
    const int adam_t = c->adam_t;        // like `gen`: read by everybody before anybody arrives at the barrier, bumped by the master after it
    const float lr_dev = c->lr;
    const int n = a.n;
#ifdef QR_PHASE_TIMING
    PPO_WALL(a.aticks, (size_t)blockIdx.x * 8 + 0);
#endif
    const int j = blockIdx.x * kApplyThreads + threadIdx.x;
    // the thread's parameter: natural order -> j itself; accumulator-order partials -> DenseMap (the unused rows of the value net's
    // output quad and the tail of the last workgroup own nothing: i = n), the four log_std entries ride behind the two nets
    int i = j;
    int pj = j;
    bool slot_thread = false;
    if (a.partial_raw > 0 && !a.ext_grad) {
        using M = DenseMap<L>;
        constexpr int S = PpoDims<L>::kRawSlots, T = M::kDenseThreads;
        const int n4 = net_off(L, 4).total;
        int p = -1;
        pj = 0;
        if (j < T) { M::map(j, 4, pj, p); i = p < 0 ? n : p; }
        else if (j < 2 * T) { M::map(j - T, 1, pj, p); pj += S; i = p < 0 ? n : n4 + p; }
        else i = j - 2 * T < 4 ? n - 4 + (j - 2 * T) : n;
        slot_thread = j < 2 * T;
    }
    const bool last_block = blockIdx.x == gridDim.x - 1;
    __shared__ float red[8];
    // Adam state and parameter of this element: loaded NOW, together with the chunk partials, so that their round trip is over
    // before the grid barrier releases (they do not depend on the norm): measured -0.15 us
    const bool owns = a.take_step && i < n;
    const float m_in = owns ? a.m[i] : 0.0f, v_in = owns ? a.v[i] : 0.0f, th_in = owns ? a.theta[i] : 0.0f;
    const float g = reduce_grad_element(a, i, pj, slot_thread, red);
#ifdef QR_PHASE_TIMING
    PPO_WALL(a.aticks, (size_t)blockIdx.x * 8 + 1);
#endif
    if (a.grad_out) {
        if (i < n) a.grad_out[i] = g;
        if (last_block && threadIdx.x < 4) a.grad_out[n + threadIdx.x] = red[4 + threadIdx.x];
    }
    if (!a.take_step) {
        if (last_block && threadIdx.x < 4 && a.stats) a.stats[threadIdx.x] += red[4 + threadIdx.x];
        return;
    }
    if (stop_flag) return;  // SB3: no update after the early stop
    // ---- squared norm across the grid: every workgroup of this launch is resident (247 x 256 threads on 256 CUs).
    // Arrive: one 64-bit store per workgroup = generation | f32 sum.  The LAST workgroup is the master (it owns the minibatch
    // statistics, so it can take the target-KL decision itself): its first wave polls all arrival words (one coalesced load per 64
    // workgroups), adds the sums in a fixed order and releases `go` = generation | verdict bits | f32 total.  Everybody else
    // polls that one word.  RELAXED polling (an agent-scope ACQUIRE load invalidates the XCD's L2 on every iteration and slowed
    // the workgroups still summing partials); nothing but the polled word itself is consumed, so no fence is needed.  Bounded.
    double sq = (double)g * g, unused = 0.0;
    block_sum2_f64<kApplyThreads>(sq, unused);
#ifdef QR_PHASE_TIMING
    PPO_WALL(a.aticks, (size_t)blockIdx.x * 8 + 2);
#endif
    const unsigned int want = (gen + 1u) & kGoGenMask;
    if (threadIdx.x == 0) {
        const unsigned long long word = ((unsigned long long)want << 32) | (unsigned long long)__float_as_uint((float)sq);
        __hip_atomic_store(&c->arrive[blockIdx.x], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (last_block && threadIdx.x < 64) {
        bool all = false;
        double total = 0.0;
        for (int spins = 0; !all && spins < (1 << 20); ++spins) {
            bool mine = true;
            total = 0.0;
            for (int q = threadIdx.x; q < (int)gridDim.x; q += 64) {
                const unsigned long long w = __hip_atomic_load(&c->arrive[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                mine = mine && (unsigned int)(w >> 32) == want;
                total += (double)__uint_as_float((unsigned int)w);
            }
            all = __ballot(mine) == ~0ull;
            if (!all) __builtin_amdgcn_s_sleep(1);
        }
        total = wave_sum_f64(total);   // lanes in a fixed order: one value, whatever the arrival order was
        if (threadIdx.x == 0) {
            if (!all) atomicAdd(&c->barrier_timeouts, 1);
            const float nsq = (float)total;
            const bool stop_m = a.kl_limit > 0.0f && red[6] > a.kl_limit;   // SB3: checked BEFORE the optimiser step of this minibatch
            const bool finite_m = nsq <= 3.0e38f;                            // false for inf and NaN
            c->gen = gen + 1u;   // every workgroup has read `gen` before it arrived; visible to the next launch
            // a barrier that timed out (never observed) releases with the non-finite verdict: NOBODY steps on a norm that lacks
            // some workgroups' sums (the launch is counted in barrier_timeouts and in skipped_nonfinite)
            const unsigned int hi = want | (stop_m ? kGoStop : 0u) | ((finite_m && all) ? 0u : kGoNonFinite);
            __hip_atomic_store(&c->go, ((unsigned long long)hi << 32) | (unsigned long long)__float_as_uint(nsq), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __shared__ unsigned long long go_s;
    if (threadIdx.x == 0) {
        unsigned long long w = 0;
        int spins = 0;
        while ((((unsigned int)((w = __hip_atomic_load(&c->go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32)) & kGoGenMask) != want) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > (1 << 20)) {  // never observed
                atomicAdd(&c->barrier_timeouts, 1);
                w = ((unsigned long long)(want | kGoNonFinite) << 32);   // take no step on a broken barrier
                break;
            }
        }
        go_s = w;
    }
    __syncthreads();
#ifdef QR_PHASE_TIMING
    PPO_WALL(a.aticks, (size_t)blockIdx.x * 8 + 3);
#endif
    const unsigned long long gw = go_s;
    const float norm_sq = __uint_as_float((unsigned int)gw);
    const bool stop_now = ((unsigned int)(gw >> 32) & kGoStop) != 0u;
    const bool finite = ((unsigned int)(gw >> 32) & kGoNonFinite) == 0u;
    if (!stop_now && finite && i < n) {
        const float norm = sqrtf(norm_sq);
        const float clip = fminf(1.0f, a.max_norm / (norm + 1e-6f));  // torch.nn.utils.clip_grad_norm_
        const float gc = g * clip;
        const float mi = a.beta1 * m_in + (1.0f - a.beta1) * gc;
        const float vi = a.beta2 * v_in + (1.0f - a.beta2) * gc * gc;
        a.m[i] = mi;
        a.v[i] = vi;
        // bias corrections: host-computed for a caller-counted step, or from the device's own count of steps really taken (the
        // same float expressions as adam_constants())
        const float bc1 = a.device_step ? 1.0f - powf(a.beta1, (float)(adam_t + 1)) : a.bc1;
        const float bc2_sqrt = a.device_step ? sqrtf(1.0f - powf(a.beta2, (float)(adam_t + 1))) : a.bc2_sqrt;
        const float lr = a.device_lr ? lr_dev : a.lr;
        const float th = th_in - (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + a.eps);  // torch.optim.Adam
        a.theta[i] = th;
        // operand images of the next minibatch: this parameter's f16 copies (log_std has none)
        const int n4 = net_off(L, 4).total, n1 = net_off(L, 1).total;
        if (i < n4) pack_scatter<L>(reinterpret_cast<_Float16*>(a.images), 4, i, th);
        else if (i < n4 + n1) pack_scatter<L>(reinterpret_cast<_Float16*>(a.images + PpoDims<L>::kImage), 1, i - n4, th);
    }
    if (last_block && threadIdx.x == 0) {
        if (a.stats)
            for (int k = 0; k < 4; ++k) a.stats[k] += red[4 + k];
        if (stop_now) c->stop = 1;
        else if (finite) { c->applied += 1; c->adam_t = adam_t + 1; }
        else c->skipped_nonfinite += 1;
    }
#ifdef QR_PHASE_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PPO_WALL(a.aticks, (size_t)blockIdx.x * 8 + 4);
#endif
}

// ---- GAE(lambda) and episode statistics over a rollout buffer [T][N] (what SB3's RolloutBuffer.compute_returns_and_advantage
// and VecMonitor do on the host): one lane = one env.  done is 0 / 1 as float.  term_val (optional) = V(terminal observation)
// at the steps that ended by the time limit, 0 elsewhere: SB3's collect_rollouts adds gamma * V(terminal_obs) to the reward
// of a truncated step before the buffer sees it (the episode still ends there: no bootstrap through the reset).
__global__ void __launch_bounds__(256) ppo_gae_kernel(int T, int N, const float* __restrict__ rew, const float* __restrict__ done,
                                                      const float* __restrict__ val, const float* __restrict__ last_val,
                                                      const float* __restrict__ term_val, float gamma,
                                                      float lam, float* __restrict__ adv, float* __restrict__ ret,
                                                      float* __restrict__ ep_ret, float* __restrict__ ep_len,
                                                      float* __restrict__ ep_gates, float* __restrict__ fin) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f;
    if (i < N) {
        float last = 0.0f, next_val = last_val[i];
        for (int t = T - 1; t >= 0; --t) {
            const size_t e = (size_t)t * N + i;
            const float nonterminal = 1.0f - done[e], v = val[e];
            const float r = term_val ? fmaf(gamma, term_val[e], rew[e]) : rew[e];
            const float delta = r + gamma * next_val * nonterminal - v;
            last = delta + gamma * lam * nonterminal * last;
            adv[e] = last;
            ret[e] = last + v;
            next_val = v;
        }
        if (ep_ret) {
            float er = ep_ret[i], el = ep_len[i], eg = ep_gates[i];
            for (int t = 0; t < T; ++t) {
                const size_t e = (size_t)t * N + i;
                const float r = rew[e], d = done[e];
                er += r;
                el += 1.0f;
                eg += r > 5.0f ? 1.0f : 0.0f;  // gate reward 10 - 10 * d2g (R:537)
                f0 += er * d; f1 += el * d; f2 += eg * d; f3 += d;
                const float keep = 1.0f - d;
                er *= keep; el *= keep; eg *= keep;
            }
            ep_ret[i] = er; ep_len[i] = el; ep_gates[i] = eg;
        }
    }
    if (fin) {  // finished-episode sums: wave reduction, one atomic per wave and statistic
        f0 = wave_sum(f0); f1 = wave_sum(f1); f2 = wave_sum(f2); f3 = wave_sum(f3);
        if ((threadIdx.x & 63) == 0 && f3 > 0.0f) {
            unsafeAtomicAdd(fin + 0, f0); unsafeAtomicAdd(fin + 1, f1); unsafeAtomicAdd(fin + 2, f2); unsafeAtomicAdd(fin + 3, f3);
        }
    }
}

}  // namespace qr

// ------------------------------------------------------------------------------------------------------------------------

namespace qr {
const half8* ppo_policy_image(const qr_ppo* p) { return p ? p->d_images : nullptr; }
// what quadrace_ppo_f32.hip needs of a handle
int ppo_handle_info(const qr_ppo* p, int* L, int* device, int* max_B, int* num_params) {
    if (!p) return QR_E_INVALID;
    *L = p->L; *device = p->device; *max_B = p->max_B; *num_params = p->num_params;
    return QR_OK;
}
void** ppo_f32_scratch_slot(qr_ppo* p) { return &p->f32_scratch; }
size_t* ppo_f32_scratch_bytes(qr_ppo* p) { return &p->f32_scratch_bytes; }
void** ppo_f32_graphs_slot(qr_ppo* p) { return &p->f32_graphs; }
hipStream_t* ppo_capture_stream_slot(qr_ppo* p) { return &p->capture_stream; }
bool ppo_uses_graphs(const qr_ppo* p) { return p->epoch_graph; }
void ppo_f32_release_graphs(void* cache);   // quadrace_ppo_f32.hip
}  // namespace qr

namespace {

template <int L>
struct PpoOps {
    using D = qr::PpoDims<L>;
    static int pack(qr_ppo* p, const float* theta, hipStream_t st) {
        hipLaunchKernelGGL(qr::ppo_pack_kernel<L>, dim3((D::kImage + 255) / 256, 2), dim3(256), 0, st, theta, p->d_images);
        QR_HIP(hipGetLastError());
        return QR_OK;
    }
    // advantage statistics of this minibatch: the epoch table when the rows were announced by qr_ppo_epoch_begin, else one launch
    static int adv_stats(qr_ppo* p, qr::PpoBatch& b, hipStream_t st) {
        // the table is consumed strictly in order (entry k serves the call whose rows are idx_all + k * B); anything else
        // disarms it, so a recycled buffer address can never pick up the sums of an older permutation
        if (p->epoch_idx && b.B == p->epoch_B && p->epoch_cursor < p->epoch_count &&
            b.idx == p->epoch_idx + (size_t)p->epoch_cursor * b.B) {
            b.acc = p->d_mbstats + 2 * p->epoch_cursor;
            if (++p->epoch_cursor == p->epoch_count) p->epoch_idx = nullptr;
            return QR_OK;
        }
        p->epoch_idx = nullptr;
        double* slot = p->d_mbstats + 2 * qr_ppo::kMaxEpochMinibatches;
        hipLaunchKernelGGL(qr::ppo_zero_table_kernel, dim3(1), dim3(256), 0, st, slot, 2);
        hipLaunchKernelGGL(qr::ppo_adv_stats_kernel, dim3((b.B + 1023) / 1024, 1), dim3(1024), 0, st, b.adv, b.idx, b.B, slot,
                           (unsigned long long*)nullptr);
        b.acc = slot;
        return QR_OK;
    }
    static constexpr size_t kLdsFused = ((size_t)D::kImage + qr::kExHalf8) * 16 + 7 * qr::kStashRows * sizeof(float);
    // dynamic-LDS limit of the gradient kernel on the CURRENT device (idempotent; not a stream operation, so it also runs
    // before a graph capture instead of inside it)
    static int configure(qr_ppo* p, bool privileged = false) {
        if (privileged) {   // the privileged-critic form of the same kernel (qr_ppo_grad_privileged): an instantiation of its own
            if (p->partial_bf16) QR_HIP((qr::configure_dynamic_lds<qr::ppo_grad_kernel<L, __bf16, false, true>>(kLdsFused)));
            else QR_HIP((qr::configure_dynamic_lds<qr::ppo_grad_kernel<L, float, false, true>>(kLdsFused)));
            return QR_OK;
        }
        if (p->partial_bf16) {
            QR_HIP((qr::configure_dynamic_lds<qr::ppo_grad_kernel<L, __bf16, false>>(kLdsFused)));
        } else {
            QR_HIP((qr::configure_dynamic_lds<qr::ppo_grad_kernel<L, float, false>>(kLdsFused)));
        }
        return QR_OK;
    }
    // one kernel: forward, backward and the weight gradients of 128 samples per workgroup and pass; partial gradients of every workgroup
    // in d_partial, per-wave sums in d_wave; returns the number of partials per network.  critic_obs: null, or the rows the value network's
    // workgroups gather instead of b.obs (the privileged critic: the same launch of the kernel's kPriv form)
    static int grad(qr_ppo* p, qr::PpoBatch b, hipStream_t st, int* chunks_out, const float* critic_obs = nullptr) {
        constexpr size_t lds_f = kLdsFused;
        if (int rc = configure(p, critic_obs != nullptr)) return rc;
        if (int rc = adv_stats(p, b, st)) return rc;
        const int pairs = (b.G + 1) / 2;
        const int wgs = pairs < qr_ppo::kFusedChunks ? pairs : qr_ppo::kFusedChunks;
        const qr::PopMember* no_table = nullptr;   // direct mode: the minibatch and its partial are the arguments
        const float* no_critic = nullptr;
        if (critic_obs && p->partial_bf16)
            hipLaunchKernelGGL((qr::ppo_grad_kernel<L, __bf16, false, true>), dim3(wgs, 2), dim3(512), lds_f, st, b,
                               reinterpret_cast<__bf16*>(p->d_partial), no_table, 0, critic_obs);
        else if (critic_obs)
            hipLaunchKernelGGL((qr::ppo_grad_kernel<L, float, false, true>), dim3(wgs, 2), dim3(512), lds_f, st, b, p->d_partial, no_table, 0,
                               critic_obs);
        else if (p->partial_bf16)
            hipLaunchKernelGGL((qr::ppo_grad_kernel<L, __bf16, false>), dim3(wgs, 2), dim3(512), lds_f, st, b,
                               reinterpret_cast<__bf16*>(p->d_partial), no_table, 0, no_critic);
        else
            hipLaunchKernelGGL((qr::ppo_grad_kernel<L, float, false>), dim3(wgs, 2), dim3(512), lds_f, st, b, p->d_partial, no_table, 0, no_critic);
        QR_HIP(hipGetLastError());
        *chunks_out = wgs;
        return QR_OK;
    }
    static int apply(qr_ppo* p, qr::ApplyArgs a, hipStream_t st) {
        a.ctrl = p->d_ctrl;
        a.images = p->d_images;
        a.n = p->num_params;
        a.partial = p->d_partial;
        // the role-split gradient kernel leaves its partials in accumulator order: one thread per slot (+ one workgroup for log_std)
        const bool raw = !a.ext_grad;
        a.partial_bf16 = (raw && p->partial_bf16) ? 1 : 0;
        a.partial_raw = raw ? 2 * D::kRawSlots : 0;
        a.wave_out = p->d_wave;
#ifdef QR_PHASE_TIMING
        a.aticks = p->apply_ticks;
#endif
        const int threads = raw ? 2 * qr::DenseMap<L>::kDenseThreads + 4 : p->num_params;
        a.owner_from = threads - 4;
        static_assert((2 * qr::DenseMap<L>::kDenseThreads + 4 + qr::kApplyThreads - 1) / qr::kApplyThreads <= 512,
                      "grid barrier: arrive[512], two resident workgroups per CU");
        hipLaunchKernelGGL(qr::ppo_apply_kernel<L>, dim3((threads + qr::kApplyThreads - 1) / qr::kApplyThreads),
                           dim3(qr::kApplyThreads), 0, st, a);
        QR_HIP(hipGetLastError());
        return QR_OK;
    }
};

template <typename F>
int dispatch_L(int L, F&& f) {   // qr::dispatch_L with this file's failure: the message goes to qr_last_error()
    return qr::dispatch_L(L, f, [] { return qr::set_last_error(QR_E_INVALID, "obs_len must be an observation length of the race envs (13 + 4g, 20 + 4g) or 16 (the predecessor envs)"); });
}

int fill_batch(qr_ppo* p, qr::PpoBatch& b, const float* theta, const float* obs, const float* act, const float* old_logp,
               const float* adv, const float* ret, const int32_t* idx, int32_t B, float clip, float vf_coef, float ent_coef,
               float* stats) {
    if (!p || !theta || !obs || !act || !old_logp || !adv || !ret || !idx) return qr::set_last_error(QR_E_INVALID, "qr_ppo: null argument");
    // (the gradient kernel masks the tail of a last, partial group of 64 rows)
    if (B < 64 || B > p->max_B)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo: minibatch size must be >= 64 and <= max_minibatch");
    b.obs = obs; b.act = act; b.old_logp = old_logp; b.adv = adv; b.ret = ret; b.idx = idx;
    b.B = B; b.G = (B + 63) / 64;
    b.clip = clip; b.vf_coef = vf_coef; b.ent_coef = ent_coef;
    b.acc = nullptr;
    b.theta = theta;
    b.images = p->d_images;
    b.wave_out = p->d_wave;
    b.stats = stats;
    b.stop = &p->d_ctrl->stop;
#ifdef QR_PHASE_TIMING
    b.ticks = p->ticks;
#endif
    return QR_OK;
}

// adam_step >= 1: the caller counts the steps (bias corrections computed here); adam_step == 0: the device's own count of steps
// really taken (PpoCtrl::adam_t).  device_lr: the learning rate is PpoCtrl::lr (qr_ppo_epoch writes it; library-internal mode --
// the extern "C" entry points take lr >= 0 and reject anything else).
void adam_constants(qr::ApplyArgs& a, float max_grad_norm, float lr, bool device_lr, float beta1, float beta2, float eps, int adam_step) {
    a.max_norm = max_grad_norm; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.device_step = adam_step == 0;
    a.device_lr = device_lr ? 1 : 0;
    const int t = adam_step > 0 ? adam_step : 1;
    a.bc1 = 1.0f - powf(beta1, (float)t);
    a.bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)t));
}

}  // namespace

extern "C" {

int qr_ppo_create(int32_t obs_len, int32_t device, int32_t max_minibatch, qr_ppo** out) {
    return qr_ppo_create_ex(obs_len, device, max_minibatch, 0, out);
}

int qr_ppo_create_ex(int32_t obs_len, int32_t device, int32_t max_minibatch, int32_t flags, qr_ppo** out) {
    if (!out) return qr::set_last_error(QR_E_INVALID, "qr_ppo_create: null output");
    if (flags < 0 || (flags & ~(QR_PPO_PARTIAL_F32 | QR_PPO_NO_EPOCH_GRAPH)))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_create_ex: unknown flag");
    *out = nullptr;
    if (max_minibatch < 64 || max_minibatch % 64 != 0) return qr::set_last_error(QR_E_INVALID, "qr_ppo_create: max_minibatch must be a multiple of 64");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return qr::set_last_error(QR_E_NO_DEVICE, "qr_ppo_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return qr::set_last_error(QR_E_INVALID, "qr_ppo_create: bad device ordinal");
    qr_ppo* p = new qr_ppo();
    p->L = obs_len;
    p->device = device;
    p->max_B = max_minibatch;
    const int rc = dispatch_L(obs_len, [&](auto Lc) {
        using D = qr::PpoDims<decltype(Lc)::value>;
        p->image_half8 = D::kImage;
        p->raw_slots = 2 * D::kRawSlots;
        return (int)QR_OK;
    });
    if (rc != QR_OK) { delete p; return rc; }
    p->num_params = qr::ppo_num_params(obs_len);
    // which forms of the kernels this handle uses: explicit flags (the library reads no environment variable)
    p->partial_bf16 = !(flags & QR_PPO_PARTIAL_F32);
    p->epoch_graph = !(flags & QR_PPO_NO_EPOCH_GRAPH);
    QR_HIP(hipSetDevice(device));
    const size_t mbbytes = (size_t)(qr_ppo::kMaxEpochMinibatches + 1) * 2 * sizeof(double);
    hipError_t e = hipMalloc((void**)&p->d_images, (size_t)2 * p->image_half8 * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_partial, (size_t)qr_ppo::kFusedChunks * (p->raw_slots > p->num_params ? p->raw_slots : p->num_params) * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_wave, (size_t)2 * 2 * (max_minibatch / 64) * 8 * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_ctrl, sizeof(qr::PpoCtrl));
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_mbstats, mbbytes);
    if (e == hipSuccess) e = hipMemset(p->d_ctrl, 0, sizeof(qr::PpoCtrl));
    if (e == hipSuccess) e = hipMemset(p->d_mbstats, 0, mbbytes);
    if (e != hipSuccess) {
        qr_ppo_destroy(p);
        return qr::set_last_error(QR_E_HIP, std::string("qr_ppo_create: ") + hipGetErrorString(e));
    }
    *out = p;
    return QR_OK;
}

int qr_ppo_destroy(qr_ppo* p) {
    if (!p) return QR_OK;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(p->d_images);
    (void)hipFree(p->d_partial);
    (void)hipFree(p->d_wave);
    (void)hipFree(p->d_ctrl);
    (void)hipFree(p->d_mbstats);
    qr::ppo_f32_release_graphs(p->f32_graphs);
    if (p->f32_scratch) (void)hipFree(p->f32_scratch);
    if (p->eg.exec) (void)hipGraphExecDestroy(p->eg.exec);
    if (p->capture_stream) (void)hipStreamDestroy(p->capture_stream);
    delete p;
    return QR_OK;
}

#ifdef QR_PHASE_TIMING
__attribute__((visibility("default"))) int qr_ppo_debug_set_ticks(qr_ppo* p, unsigned long long* ticks_dev) { p->ticks = ticks_dev; return QR_OK; }
__attribute__((visibility("default"))) int qr_ppo_debug_set_apply_ticks(qr_ppo* p, unsigned long long* ticks_dev) { p->apply_ticks = ticks_dev; return QR_OK; }
#endif

int qr_ppo_num_params(const qr_ppo* p) { return p ? p->num_params : qr::set_last_error(QR_E_INVALID, "qr_ppo_num_params: null handle"); }

int qr_ppo_pack(qr_ppo* p, const float* theta_dev, void* stream) {
    if (!p || !theta_dev) return qr::set_last_error(QR_E_INVALID, "qr_ppo_pack: null argument");
    QR_HIP(hipSetDevice(p->device));
    p->packed_theta = theta_dev;
    return dispatch_L(p->L, [&](auto Lc) { return PpoOps<decltype(Lc)::value>::pack(p, theta_dev, (hipStream_t)stream); });
}

int qr_ppo_control(qr_ppo* p, float target_kl, int32_t clear, void* stream) {
    if (!p) return qr::set_last_error(QR_E_INVALID, "qr_ppo_control: null handle");
    QR_HIP(hipSetDevice(p->device));
    p->target_kl = target_kl;
    if (clear) {  // stop flag and counters (the barrier counters that follow them in PpoCtrl keep running)
        QR_HIP(hipMemsetAsync(&p->d_ctrl->stop, 0, 4 * sizeof(int), (hipStream_t)stream));
    }
    return QR_OK;
}

int qr_ppo_status(qr_ppo* p, int32_t* out4, void* stream) {
    if (!p || !out4) return qr::set_last_error(QR_E_INVALID, "qr_ppo_status: null argument");
    QR_HIP(hipSetDevice(p->device));
    QR_HIP(hipMemcpyAsync(out4, &p->d_ctrl->stop, 4 * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    QR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return QR_OK;
}

static int epoch_begin_impl(qr_ppo* p, const float* adv_dev, const int32_t* idx_dev, int32_t B, int32_t num_minibatches, void* stream,
                            unsigned long long* bump);
int qr_ppo_epoch_begin(qr_ppo* p, const float* adv_dev, const int32_t* idx_dev, int32_t B, int32_t num_minibatches, void* stream) {
    return epoch_begin_impl(p, adv_dev, idx_dev, B, num_minibatches, stream, nullptr);
}
static int epoch_begin_impl(qr_ppo* p, const float* adv_dev, const int32_t* idx_dev, int32_t B, int32_t num_minibatches, void* stream,
                            unsigned long long* bump) {
    if (!p || !adv_dev || !idx_dev) return qr::set_last_error(QR_E_INVALID, "qr_ppo_epoch_begin: null argument");
    if (B < 64 || B > p->max_B || num_minibatches < 1 || num_minibatches > qr_ppo::kMaxEpochMinibatches)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_epoch_begin: bad minibatch size / count");
    QR_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(qr::ppo_zero_table_kernel, dim3((2 * num_minibatches + 255) / 256), dim3(256), 0, st, p->d_mbstats, 2 * num_minibatches);
    hipLaunchKernelGGL(qr::ppo_adv_stats_kernel, dim3((B + 1023) / 1024, num_minibatches), dim3(1024), 0, st, adv_dev, idx_dev, B,
                       p->d_mbstats, bump);
    QR_HIP(hipGetLastError());
    p->epoch_idx = idx_dev;
    p->epoch_B = B;
    p->epoch_count = num_minibatches;
    p->epoch_cursor = 0;
    return QR_OK;
}

// critic_obs_dev: null (qr_ppo_grad), or the value network's rows (qr_ppo_grad_privileged, which has refused a null one)
static int ppo_grad_impl(qr_ppo* p, const float* theta_dev, const float* obs_dev, const float* critic_obs_dev, const float* act_dev,
                         const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B, float clip,
                         float vf_coef, float ent_coef, float* grad_out_dev, float* stats_dev, void* stream) {
    qr::PpoBatch b;
    if (int rc = fill_batch(p, b, theta_dev, obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev, idx_dev, B, clip, vf_coef, ent_coef, stats_dev))
        return rc;
    if (!grad_out_dev) return qr::set_last_error(QR_E_INVALID, "qr_ppo_grad: null grad_out");
    QR_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_L(p->L, [&](auto Lc) {
        constexpr int L = decltype(Lc)::value;
        // the operand images are current when they were built from this vector by qr_ppo_pack or kept in step with it by
        // qr_ppo_minibatch / qr_ppo_apply (callers that edit theta themselves call qr_ppo_pack, as documented)
        if (p->packed_theta != theta_dev) {
            if (int r = PpoOps<L>::pack(p, theta_dev, st)) return r;
            p->packed_theta = theta_dev;
        }
        int chunks = 0;
        if (int r = PpoOps<L>::grad(p, b, st, &chunks, critic_obs_dev)) return r;
        qr::ApplyArgs a{};
        a.grad_out = grad_out_dev;
        a.chunks = chunks;
        a.Gw = 2 * b.G;
        a.ent_coef = ent_coef;
        a.stats = stats_dev;
        a.take_step = 0;
        return PpoOps<L>::apply(p, a, st);
    });
}

int qr_ppo_grad(qr_ppo* p, const float* theta_dev, const float* obs_dev, const float* act_dev, const float* old_logp_dev,
                const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B, float clip, float vf_coef,
                float ent_coef, float* grad_out_dev, float* stats_dev, void* stream) {
    return ppo_grad_impl(p, theta_dev, obs_dev, nullptr, act_dev, old_logp_dev, adv_dev, ret_dev, idx_dev, B, clip, vf_coef, ent_coef, grad_out_dev,
                         stats_dev, stream);
}

// qr_ppo_grad whose value network reads its own rows: net 1's workgroups gather from critic_obs_dev [rows][obs_len] by the same idx_dev
int qr_ppo_grad_privileged(qr_ppo* p, const float* theta_dev, const float* obs_dev, const float* critic_obs_dev, const float* act_dev,
                           const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B, float clip,
                           float vf_coef, float ent_coef, float* grad_out_dev, float* stats_dev, void* stream) {
    if (p && !critic_obs_dev) return qr::set_last_error(QR_E_INVALID, "qr_ppo_grad_privileged: null critic_obs_dev (qr_ppo_grad is the call without one)");
    return ppo_grad_impl(p, theta_dev, obs_dev, critic_obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev, idx_dev, B, clip, vf_coef, ent_coef,
                         grad_out_dev, stats_dev, stream);
}

// critic_obs_dev (last): null, or the value network's rows (the privileged forms)
static int ppo_minibatch_impl(qr_ppo* p, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev, const float* act_dev,
                              const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B,
                              float clip, float vf_coef, float ent_coef, float max_grad_norm, float lr, bool device_lr, float beta1,
                              float beta2, float eps, int32_t adam_step, float* stats_dev, void* stream, const float* critic_obs_dev = nullptr) {
    qr::PpoBatch b;
    if (int rc = fill_batch(p, b, theta_dev, obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev, idx_dev, B, clip, vf_coef, ent_coef, stats_dev))
        return rc;
    if (!adam_m_dev || !adam_v_dev || adam_step < 0) return qr::set_last_error(QR_E_INVALID, "qr_ppo_minibatch: bad Adam state");
    QR_HIP(hipSetDevice(p->device));
    p->packed_theta = theta_dev;   // the apply kernel keeps the images in step with this vector
    hipStream_t st = (hipStream_t)stream;
    return dispatch_L(p->L, [&](auto Lc) {
        constexpr int L = decltype(Lc)::value;
        int chunks = 0;
        if (int r = PpoOps<L>::grad(p, b, st, &chunks, critic_obs_dev)) return r;  // images were packed by the previous call (or qr_ppo_pack)
        qr::ApplyArgs a{};
        a.theta = theta_dev; a.m = adam_m_dev; a.v = adam_v_dev;
        a.chunks = chunks;
        a.Gw = 2 * b.G;
        a.ent_coef = ent_coef;
        a.stats = stats_dev;
        a.kl_limit = p->target_kl > 0.0f ? 1.5f * p->target_kl * (float)B : 0.0f;
        a.take_step = 1;
        adam_constants(a, max_grad_norm, lr, device_lr, beta1, beta2, eps, adam_step);
        return PpoOps<L>::apply(p, a, st);
    });
}

int qr_ppo_minibatch(qr_ppo* p, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev, const float* act_dev,
                     const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t B,
                     float clip, float vf_coef, float ent_coef, float max_grad_norm, float lr, float beta1, float beta2, float eps,
                     int32_t adam_step, float* stats_dev, void* stream) {
    if (!(lr >= 0.0f)) return qr::set_last_error(QR_E_INVALID, "qr_ppo_minibatch: the learning rate must be >= 0");
    return ppo_minibatch_impl(p, theta_dev, adam_m_dev, adam_v_dev, obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev, idx_dev, B, clip,
                              vf_coef, ent_coef, max_grad_norm, lr, false, beta1, beta2, eps, adam_step, stats_dev, stream);
}

// qr_ppo_minibatch whose value network reads its own rows (qr_ppo_grad_privileged + qr_ppo_apply in the same two launches)
int qr_ppo_minibatch_privileged(qr_ppo* p, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev, const float* critic_obs_dev,
                                const float* act_dev, const float* old_logp_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev,
                                int32_t B, float clip, float vf_coef, float ent_coef, float max_grad_norm, float lr, float beta1, float beta2,
                                float eps, int32_t adam_step, float* stats_dev, void* stream) {
    if (p && !critic_obs_dev)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_minibatch_privileged: null critic_obs_dev (qr_ppo_minibatch is the call without one)");
    if (!(lr >= 0.0f)) return qr::set_last_error(QR_E_INVALID, "qr_ppo_minibatch: the learning rate must be >= 0");
    return ppo_minibatch_impl(p, theta_dev, adam_m_dev, adam_v_dev, obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev, idx_dev, B, clip,
                              vf_coef, ent_coef, max_grad_norm, lr, false, beta1, beta2, eps, adam_step, stats_dev, stream, critic_obs_dev);
}

// Data-parallel training: every rank calls qr_ppo_grad on its shard of the minibatch, the caller averages the [n + 4] vector
// (gradient + minibatch statistics: one all-reduce over RCCL), then every rank applies the same update with qr_ppo_apply --
// including the same target-KL decision, because the KL sum travels with the gradient.
int qr_ppo_apply(qr_ppo* p, float* theta_dev, float* adam_m_dev, float* adam_v_dev, float* grad_dev, int32_t B, float max_grad_norm,
                 float lr, float beta1, float beta2, float eps, int32_t adam_step, float* stats_dev, void* stream) {
    if (!p || !theta_dev || !adam_m_dev || !adam_v_dev || !grad_dev || adam_step < 0 || B < 1 || !(lr >= 0.0f))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_apply: bad argument (null pointer, adam_step < 0, B < 1 or a learning rate below 0)");
    QR_HIP(hipSetDevice(p->device));
    p->packed_theta = theta_dev;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_L(p->L, [&](auto Lc) {
        constexpr int L = decltype(Lc)::value;
        qr::ApplyArgs a{};
        a.theta = theta_dev; a.m = adam_m_dev; a.v = adam_v_dev;
        a.ext_grad = grad_dev;
        a.stats = stats_dev;
        a.kl_limit = p->target_kl > 0.0f ? 1.5f * p->target_kl * (float)B : 0.0f;
        a.take_step = 1;
        adam_constants(a, max_grad_norm, lr, false, beta1, beta2, eps, adam_step);
        return PpoOps<L>::apply(p, a, st);
    });
}

// Device-resident optimiser step count (see PpoCtrl::adam_t): read it for a checkpoint, set it when one is loaded.
int qr_ppo_adam_step(qr_ppo* p, int32_t* value, int32_t set, void* stream) {
    if (!p || !value) return qr::set_last_error(QR_E_INVALID, "qr_ppo_adam_step: null argument");
    if (set && *value < 0) return qr::set_last_error(QR_E_INVALID, "qr_ppo_adam_step: negative step count");
    QR_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (set) QR_HIP(hipMemcpyAsync(&p->d_ctrl->adam_t, value, sizeof(int32_t), hipMemcpyHostToDevice, st));
    else QR_HIP(hipMemcpyAsync(value, &p->d_ctrl->adam_t, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    QR_HIP(hipStreamSynchronize(st));
    return QR_OK;
}

// On-device epoch permutations (qr_ppo_epoch with device_shuffle): state[0] = seed, state[1] = epochs shuffled so far.
// set == 0 reads both (for a checkpoint), set != 0 writes both.  Blocks.
int qr_ppo_shuffle_state(qr_ppo* p, uint64_t* state2, int32_t set, void* stream) {
    if (!p || !state2) return qr::set_last_error(QR_E_INVALID, "qr_ppo_shuffle_state: null argument");
    QR_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (set) {
        p->shuffle_seed = state2[0];
        QR_HIP(hipMemcpyAsync(&p->d_ctrl->shuffle_count, &state2[1], sizeof(uint64_t), hipMemcpyHostToDevice, st));
    } else {
        state2[0] = p->shuffle_seed;
        QR_HIP(hipMemcpyAsync(&state2[1], &p->d_ctrl->shuffle_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    QR_HIP(hipStreamSynchronize(st));
    return QR_OK;
}

// One whole epoch: the advantage statistics of every minibatch, then num_minibatches x (gradient kernel, apply kernel) on the rows
// perm[k B .. (k + 1) B), k = 0 .. num_minibatches - 1 -- enqueued as ONE replayed hipGraph.  Dependent kernel nodes of a graph start
// ~1 us sooner after each other than dependent stream launches (tools/ubench/launch_floor.hip), and there are 2 x 128 of them per
// epoch at the config-5 shape; the host issues one graph launch instead of 257 kernel launches.  Replays are valid because nothing a
// node's arguments name changes: the permutation is rewritten IN PLACE by the caller, the Adam step count and the learning rate
// are read from device memory, the early-stop flag is sticky on the device.  The graph is re-captured when any argument changes.
// critic_obs_dev: null (qr_ppo_epoch), or the value network's rows (qr_ppo_epoch_privileged, which has refused a null one); part of the
// graph's key: the same handle may serve both calls
static int ppo_epoch_impl(qr_ppo* p, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev, const float* critic_obs_dev,
                          const float* act_dev, const float* old_logp_dev, const float* adv_dev, const float* ret_dev, int32_t* perm_dev, int32_t B,
                          int32_t num_minibatches, int32_t num_epochs, int32_t device_shuffle, float clip, float vf_coef, float ent_coef,
                          float max_grad_norm, float lr, float beta1, float beta2, float eps, float* stats_dev, void* stream) {
    if (!p || !theta_dev || !adam_m_dev || !adam_v_dev || !obs_dev || !act_dev || !old_logp_dev || !adv_dev || !ret_dev || !perm_dev)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_epoch: null argument");
    if (B < 64 || B > p->max_B || num_minibatches < 1 || num_minibatches > qr_ppo::kMaxEpochMinibatches || !(lr >= 0.0f))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_epoch: bad minibatch size / count / learning rate");
    if (num_epochs < 1 || num_epochs > 64 || (num_epochs > 1 && !device_shuffle))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_epoch: num_epochs > 1 needs device_shuffle (the caller cannot rewrite the permutation in between)");
    QR_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const bool caller_captures = qr::stream_is_capturing(st);
    // the learning rate travels through device memory (it may follow a schedule; the epoch graph's nodes read PpoCtrl::lr).  Written by
    // a one-thread kernel: when the CALLER captures `st`, this node carries the value of the capturing call (lr is frozen into that
    // graph, like every other scalar argument of the call).
    hipLaunchKernelGGL(qr::ppo_set_lr_kernel, dim3(1), dim3(1), 0, st, &p->d_ctrl->lr, lr);
    QR_HIP(hipGetLastError());
    p->packed_theta = theta_dev;
    // per-device kernel attributes are set outside the capture (not a stream operation)
    if (int rc = dispatch_L(p->L, [&](auto Lc) { return PpoOps<decltype(Lc)::value>::configure(p, critic_obs_dev != nullptr); })) return rc;
    const unsigned int rows = (unsigned int)B * (unsigned int)num_minibatches;
    auto enqueue = [&](hipStream_t s) -> int {
        for (int e = 0; e < num_epochs; ++e) {
            if (device_shuffle) {   // perm = keyed bijection of [0, rows) for (seed, device-resident epoch count)
                hipLaunchKernelGGL(qr::ppo_shuffle_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, perm_dev, rows, p->shuffle_seed,
                                   &p->d_ctrl->shuffle_count);
                QR_HIP(hipGetLastError());
            }
            if (int rc = epoch_begin_impl(p, adv_dev, perm_dev, B, num_minibatches, s, device_shuffle ? &p->d_ctrl->shuffle_count : nullptr))
                return rc;
            for (int k = 0; k < num_minibatches; ++k)
                if (int rc = ppo_minibatch_impl(p, theta_dev, adam_m_dev, adam_v_dev, obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev,
                                                perm_dev + (size_t)k * B, B, clip, vf_coef, ent_coef, max_grad_norm, 0.0f, true, beta1,
                                                beta2, eps, 0, stats_dev, s, critic_obs_dev))
                    return rc;
        }
        return QR_OK;
    };
    if (caller_captures || !p->epoch_graph) return enqueue(st);   // a graph launch cannot be captured: plain nodes into the caller's graph
    qr_ppo::EpochGraph& g = p->eg;
    const bool hit = g.exec && g.theta == theta_dev && g.m == adam_m_dev && g.v == adam_v_dev && g.obs == obs_dev && g.critic == critic_obs_dev &&
                     g.act == act_dev &&
                     g.old_logp == old_logp_dev && g.adv == adv_dev && g.ret == ret_dev && g.perm == perm_dev && g.stats == stats_dev &&
                     g.B == B && g.M == num_minibatches && g.E == num_epochs && g.shuffle == device_shuffle && g.seed == p->shuffle_seed &&
                     g.clip == clip && g.vf_coef == vf_coef && g.ent_coef == ent_coef &&
                     g.max_grad_norm == max_grad_norm && g.beta1 == beta1 && g.beta2 == beta2 && g.eps == eps && g.target_kl == p->target_kl;
    if (!hit) {
        if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
        if (!p->capture_stream) QR_HIP(hipStreamCreateWithFlags(&p->capture_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        QR_HIP(hipStreamBeginCapture(p->capture_stream, hipStreamCaptureModeRelaxed));
        const int rc = enqueue(p->capture_stream);
        const hipError_t end = hipStreamEndCapture(p->capture_stream, &graph);
        if (rc != QR_OK || end != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc != QR_OK ? rc : qr::set_last_error(QR_E_HIP, std::string("qr_ppo_epoch: graph capture failed: ") + hipGetErrorString(end));
        }
        const hipError_t inst = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (inst != hipSuccess) {
            g.exec = nullptr;
            return qr::set_last_error(QR_E_HIP, std::string("qr_ppo_epoch: hipGraphInstantiate: ") + hipGetErrorString(inst));
        }
        g.theta = theta_dev; g.m = adam_m_dev; g.v = adam_v_dev; g.obs = obs_dev; g.critic = critic_obs_dev; g.act = act_dev; g.old_logp = old_logp_dev;
        g.adv = adv_dev; g.ret = ret_dev; g.perm = perm_dev; g.stats = stats_dev; g.B = B; g.M = num_minibatches;
        g.E = num_epochs; g.shuffle = device_shuffle; g.seed = p->shuffle_seed;
        g.clip = clip; g.vf_coef = vf_coef; g.ent_coef = ent_coef; g.max_grad_norm = max_grad_norm; g.beta1 = beta1; g.beta2 = beta2;
        g.eps = eps; g.target_kl = p->target_kl;
    }
    // the capture consumed the epoch table's host-side cursor; a replay does not run that host code, so leave it disarmed
    p->epoch_idx = nullptr;
    QR_HIP(hipGraphLaunch(g.exec, st));
    return QR_OK;
}

int qr_ppo_epoch(qr_ppo* p, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev, const float* act_dev,
                 const float* old_logp_dev, const float* adv_dev, const float* ret_dev, int32_t* perm_dev, int32_t B,
                 int32_t num_minibatches, int32_t num_epochs, int32_t device_shuffle, float clip, float vf_coef, float ent_coef,
                 float max_grad_norm, float lr, float beta1, float beta2, float eps, float* stats_dev, void* stream) {
    return ppo_epoch_impl(p, theta_dev, adam_m_dev, adam_v_dev, obs_dev, nullptr, act_dev, old_logp_dev, adv_dev, ret_dev, perm_dev, B, num_minibatches,
                          num_epochs, device_shuffle, clip, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, eps, stats_dev, stream);
}

// qr_ppo_epoch whose value network reads its own rows: every minibatch of the epoch is qr_ppo_minibatch_privileged
int qr_ppo_epoch_privileged(qr_ppo* p, float* theta_dev, float* adam_m_dev, float* adam_v_dev, const float* obs_dev, const float* critic_obs_dev,
                            const float* act_dev, const float* old_logp_dev, const float* adv_dev, const float* ret_dev, int32_t* perm_dev, int32_t B,
                            int32_t num_minibatches, int32_t num_epochs, int32_t device_shuffle, float clip, float vf_coef, float ent_coef,
                            float max_grad_norm, float lr, float beta1, float beta2, float eps, float* stats_dev, void* stream) {
    if (p && !critic_obs_dev) return qr::set_last_error(QR_E_INVALID, "qr_ppo_epoch_privileged: null critic_obs_dev (qr_ppo_epoch is the call without one)");
    return ppo_epoch_impl(p, theta_dev, adam_m_dev, adam_v_dev, obs_dev, critic_obs_dev, act_dev, old_logp_dev, adv_dev, ret_dev, perm_dev, B,
                          num_minibatches, num_epochs, device_shuffle, clip, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, eps, stats_dev, stream);
}

// Forward pass of one of the two networks with the operand images of the last pack (0 = policy means, 1 = value in column 0):
// out_dev [n][4].  Same kernel as qr_policy_forward.
int qr_ppo_forward(qr_ppo* p, int32_t net, int32_t n, const float* obs_dev, float* out_dev, void* stream) {
    if (!p || !obs_dev || !out_dev || n < 1 || net < 0 || net > 1) return qr::set_last_error(QR_E_INVALID, "qr_ppo_forward: bad argument");
    QR_HIP(hipSetDevice(p->device));
    const hipError_t e = qr::launch_policy(p->L, p->d_images + (size_t)net * p->image_half8, n, obs_dev, out_dev, (hipStream_t)stream);
    if (e != hipSuccess) return qr::set_last_error(QR_E_HIP, std::string("qr_ppo_forward: ") + hipGetErrorString(e));
    return QR_OK;
}

// GAE(lambda) advantages / returns of a rollout [T][N] and (optionally) episode statistics; see ppo_gae_kernel.
int qr_ppo_gae(qr_ppo* p, int32_t T, int32_t N, const float* rew_dev, const float* done_dev, const float* val_dev,
               const float* last_val_dev, const float* term_val_dev, float gamma, float lam, float* adv_out_dev, float* ret_out_dev,
               float* ep_ret_dev, float* ep_len_dev, float* ep_gates_dev, float* fin_dev, void* stream) {
    if (!p || !rew_dev || !done_dev || !val_dev || !last_val_dev || !adv_out_dev || !ret_out_dev || T < 1 || N < 1)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_gae: bad argument");
    if (ep_ret_dev && (!ep_len_dev || !ep_gates_dev)) return qr::set_last_error(QR_E_INVALID, "qr_ppo_gae: episode state needs all three arrays");
    QR_HIP(hipSetDevice(p->device));
    hipLaunchKernelGGL(qr::ppo_gae_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, N, rew_dev, done_dev, val_dev,
                       last_val_dev, term_val_dev, gamma, lam, adv_out_dev, ret_out_dev, ep_ret_dev, ep_len_dev, ep_gates_dev, fin_dev);
    QR_HIP(hipGetLastError());
    return QR_OK;
}

}  // extern "C"

namespace qr {
int ppo_epoch_prologue(qr_ppo* p, const float* adv_dev, int32_t* perm_dev, int32_t B, int32_t num_minibatches, int32_t device_shuffle,
                       hipStream_t s) {
    if (device_shuffle) {
        const unsigned int rows = (unsigned int)B * (unsigned int)num_minibatches;
        hipLaunchKernelGGL(ppo_shuffle_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, perm_dev, rows, p->shuffle_seed, &p->d_ctrl->shuffle_count);
        QR_HIP(hipGetLastError());
    }
    const int rc = epoch_begin_impl(p, adv_dev, perm_dev, B, num_minibatches, s, device_shuffle ? &p->d_ctrl->shuffle_count : nullptr);
    p->epoch_idx = nullptr;   // the population's kernels address the table themselves
    return rc;
}
}  // namespace qr
