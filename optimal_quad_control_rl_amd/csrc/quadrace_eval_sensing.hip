// quadrace_eval_sensing.hip -- closed-loop evaluation of a grid of policies x flight conditions x vehicles x SENSING in one launch
// (qr_evaluate_policy_sensing_grid): eval_policy_dynamics_grid_kernel (quadrace_eval_dynamics.hip) with the map's fourth entry read and
// a fourth bank.  "Which sensing error breaks this policy first, and how many control periods of latency can it fly with?" is one launch
// instead of a host loop of one launch per step.
//   * a sensing slot is kSensingSlotFloats floats (128 bytes, 16-byte aligned): sigma[0..7], one per group of observation entries
//     (sensing_group below; include/quadrace.h has the table), then the command delay d in [0, kMaxDelay] as an int32 bit pattern, then
//     zeros.  The workgroup loads its slot ONCE, ahead of the step loop, through uniform-address loads, and pins sigma and d to scalar
//     registers: no load of a slot value inside the loop.
//   * observation noise: at step t the policy is evaluated on o~[j] = add_rn(o[j], mul_rn(sigma[group(j)], eps[j])); the env's own
//     observation and state are untouched (eval_policy_body rebuilds o from the state behind every step).  eps[4 q .. 4 q + 3] is one
//     Philox4x32-10 block, counter (gid lo, gid hi, step lo, (step hi & 0xFFFFFF) | (q << 24)), gid = env_id_base + the env's index
//     within its GROUP (the id of the group-local reset stream: every cell of a grid draws the same eps), step = first_step + t, key
//     (seed lo ^ kSensingTweak0, seed hi ^ kSensingTweak1); uniforms and Box-Muller are the action noise's.  ceil(L / 4) blocks per step;
//     a slot whose eight sigmas are all zero draws nothing (a workgroup-uniform branch) and the policy sees o itself.
//   * command delay: the env flies the command computed d steps earlier, (0, 0, 0, 0) for the first d steps of an episode; the queue
//     is a ring in the lane's own LDS column behind the lap sums (eval_policy_body) and travels between launches in the caller's
//     `pending` [n][16] in canonical order.
// ONE device function, sensing_noise4, gives sigma x eps to the evaluator and to sensing_noise_kernel (qr_sensing_noise: the rows the
// tests hold the stream's spec by).  The step loop, the accounting and the records are eval_policy_body's.  No atomics, no workgroup that
// waits for another, no global store inside the step loop.  A translation unit of its own: the code objects of the other sources do not
// change when this one does.
#include "quadrace_eval_body.hpp"
#include "quadrace_launch.hpp"

namespace qr {

// Domain separation: the reset stream keys Philox with the env seed itself, the action noise with seed ^ (0x9E3779B9, 0x85EBCA6B), the ES
// noise with seed ^ (0x2545F491, 0x4F6CDD1D); the observation noise with these
constexpr uint32_t kSensingTweak0 = 0x6A09E667u, kSensingTweak1 = 0x3C6EF372u;
constexpr int kSensingSigmas = 8;

// sigma group of observation entry j (S = the state part: 16 for E2E, 13 for INDI)
template <int V, int GA>
constexpr int sensing_group(int j) {
    constexpr int S = Env<V>::S;
    if (j < 3) return 0;                                 // position in the gate frame
    if (j < 6) return 1;                                 // velocity in the gate frame
    if (j < 9) return 2;                                 // roll, pitch, yaw relative to the gate
    if (j < 12) return 3;                                // body rates
    if (j < S) return 4;                                 // actuator state
    if (j < S + 4 * GA) return ((j - S) & 3) == 3 ? 6 : 5;   // gate a ahead: relative position | relative yaw
    return 7;                                            // disturbance columns (E2E)
}

// what a workgroup holds of its slot and of the call, all workgroup-uniform
struct SensingRegs {
    float sigma[kSensingSigmas];
    int delay;
    bool noise_on;                 // any sigma != 0
    uint32_t k0, k1;               // the Philox key
    uint32_t step_lo, step_hi;     // first_step
    float* pending;                // [n][kSensingQueueFloats]
};

struct SensingStream { uint32_t k0, k1, step_lo, step_hi; };
inline SensingStream sensing_stream(uint64_t seed, uint64_t first_step) {
    SensingStream s;
    s.k0 = (uint32_t)seed ^ kSensingTweak0;
    s.k1 = (uint32_t)(seed >> 32) ^ kSensingTweak1;
    s.step_lo = (uint32_t)first_step;
    s.step_hi = (uint32_t)(first_step >> 32);
    return s;
}

// one slot of a sensing bank -> the register set, every value pinned to a scalar register (`slot` derives from blockIdx alone and no store
// of the kernel touches the bank)
__device__ __forceinline__ void load_sensing(const float* __restrict__ slot, const SensingStream& s, float* pending, SensingRegs& r) {
#pragma unroll
    for (int g = 0; g < kSensingSigmas; ++g) r.sigma[g] = slot[g];
    r.delay = __float_as_int(slot[kSensingSigmas]);
#pragma unroll
    for (int g = 0; g < kSensingSigmas; ++g) asm volatile("" : "+s"(r.sigma[g]));
    asm volatile("" : "+s"(r.delay));
    bool on = false;
#pragma unroll
    for (int g = 0; g < kSensingSigmas; ++g) on |= r.sigma[g] != 0.0f;
    r.noise_on = on;
    r.k0 = s.k0; r.k1 = s.k1; r.step_lo = s.step_lo; r.step_hi = s.step_hi;
    r.pending = pending;
}

// THE noise: delta[c] = mul_rn(sigma[group(4 q + c)], eps[4 q + c]) of env `gid` at call-step k, c = 0..3 (entries at or past L are
// computed and ignored by the callers).  Uniforms and Box-Muller exactly the action noise's (rollout_policy_kernel's noise_slice, es_noise4):
// (x0, x1) -> r cos, r sin; (x2, x3) -> the second pair.
template <int V, int GA, int Q>
__device__ __forceinline__ void sensing_noise4(const SensingRegs& r, uint32_t gid_lo, uint32_t gid_hi, int k, float (&delta)[4]) {
    constexpr int L = obs_len<V, GA>();
    const uint32_t s_lo = r.step_lo + (uint32_t)k;
    const uint32_t s_hi = r.step_hi + (s_lo < r.step_lo ? 1u : 0u);
    uint32_t x[4];
    philox4x32_10(gid_lo, gid_hi, s_lo, (s_hi & 0xFFFFFFu) | ((uint32_t)Q << 24), r.k0, r.k1, x);
    const float u1a = (float)((x[0] >> 8) + 1u) * 5.9604644775390625e-8f, u2a = u01(x[1]);
    const float u1b = (float)((x[2] >> 8) + 1u) * 5.9604644775390625e-8f, u2b = u01(x[3]);
    const float ra = fast_sqrt(-2.0f * __logf(u1a)), rb = fast_sqrt(-2.0f * __logf(u1b));
    float sa, ca, sb, cb;
    qr_sincos(6.283185307179586f * u2a, sa, ca);
    qr_sincos(6.283185307179586f * u2b, sb, cb);
    const float eps[4] = {ra * ca, ra * sa, rb * cb, rb * sb};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        constexpr int kLast = L - 1;
        const int j = 4 * Q + c < L ? 4 * Q + c : kLast;
        delta[c] = mul_rn(r.sigma[sensing_group<V, GA>(j)], eps[c]);
    }
}

template <int V, int GA, int Q = 0>
__device__ __forceinline__ void sensing_noise_row(const SensingRegs& r, uint32_t gid_lo, uint32_t gid_hi, int k, float* o, bool add) {
    constexpr int L = obs_len<V, GA>();
    if constexpr (4 * Q < L) {
        float delta[4];
        sensing_noise4<V, GA, Q>(r, gid_lo, gid_hi, k, delta);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * Q + c < L) o[4 * Q + c] = add ? add_rn(o[4 * Q + c], delta[c]) : delta[c];
        sensing_noise_row<V, GA, Q + 1>(r, gid_lo, gid_hi, k, o, add);
    }
}

// the sensing class of eval_policy_body: the three hooks
struct RuntimeSensing {
    using Arg = const SensingRegs*;
    static constexpr bool kOn = true;
    static __device__ __forceinline__ int delay(Arg r) { return r->delay; }
    static __device__ __forceinline__ float* pending(Arg r) { return r->pending; }
    template <int V, int GA>
    static __device__ __forceinline__ void perturb(Arg r, uint32_t gid_lo, uint32_t gid_hi, int k, float* o) {
        if (r->noise_on) sensing_noise_row<V, GA>(*r, gid_lo, gid_hi, k, o, true);
    }
};

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
