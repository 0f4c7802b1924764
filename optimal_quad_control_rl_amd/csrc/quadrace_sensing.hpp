// quadrace_sensing.hpp -- the SENSOR between an env and its policy, for every kernel that flies one: the sensing-grid evaluator
// (quadrace_eval_sensing.hip: eval_policy_body with RuntimeSensing, and sensing_noise_kernel) and the sensing mode of the grouped
// closed-loop rollout (quadrace_rollout_sensing.hip: rollout_policy_group_kernel with RuntimeSensing).  ONE set of device functions:
// the slot load, the sigma group of an observation entry, the Philox stream and its key tweaks, sigma x eps of four entries, the noisy
// row, and the two sensing classes a kernel is instantiated with.  What a kernel adds itself is the command queue: a ring in the lane's
// own LDS column, read from and written back to the caller's `pending` [n][kSensingQueueFloats] in canonical order (eval_policy_body
// and rollout_policy_group_kernel carry the same statements).
//   * a sensing slot is kSensingSlotFloats floats (128 bytes, 16-byte aligned): sigma[0..7], one per group of observation entries
//     (sensing_group below; include/quadrace.h has the table), then the command delay d in [0, kMaxDelay] as an int32 bit pattern, then
//     zeros.  The workgroup loads its slot ONCE, ahead of the step loop, through uniform-address loads, and pins sigma and d to scalar
//     registers: no load of a slot value inside the loop.
//   * observation noise: at step t the policy is evaluated on o~[j] = add_rn(o[j], mul_rn(sigma[group(j)], eps[j])); the env's own
//     observation and state are untouched (the callers rebuild o from the state behind every step).  eps[4 q .. 4 q + 3] is one
//     Philox4x32-10 block, counter (gid lo, gid hi, step lo, (step hi & 0xFFFFFF) | (q << 24)), step = first_step + t, key
//     (seed lo ^ kSensingTweak0, seed hi ^ kSensingTweak1); uniforms and Box-Muller are the action noise's.  ceil(L / 4) blocks per step;
//     a slot whose eight sigmas are all zero draws nothing (a workgroup-uniform branch) and the policy sees o itself.  WHICH gid is the
//     caller's: the evaluator passes the group-local id (every cell of a grid draws the same eps), the rollout the ordinary env id.
#pragma once
#include "quadrace_env_kernels.hpp"

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

// The two sensing classes of eval_policy_body and rollout_policy_group_kernel.  IdealSensing (their default, the argument a dummy): the
// policy sees the observation of the step and its command flies in the step; no code.  RuntimeSensing: the three hooks --
// perturb<V, GA>(sen, gid, k, o) in front of the forward, delay(sen) / pending(sen) for the command queue between clip_action and step_env.
struct IdealSensing {
    using Arg = int;
    static constexpr bool kOn = false;
};

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

}  // namespace qr
