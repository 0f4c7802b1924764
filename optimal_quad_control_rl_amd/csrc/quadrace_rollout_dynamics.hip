// quadrace_rollout_dynamics.hip -- PPO's collect phase across a MIX of VEHICLES in one launch (qr_rollout_policy_dynamics): the launch
// function and the instantiations of rollout_policy_group_kernel<V, GA, kF32, false, true> (quadrace_rollout_group.hpp, where the kernel
// and everything about it is written down): one policy per launch, a condition AND a vehicle per group of envs.  The map is the grid
// evaluator's int2 array with the dynamics slot in the half the single-policy mode never read: map[g] = (dynamics, condition).
// Also here: the device sampler of the dynamics bank (qr_vehicle_bank_sample), which draws the physical parameters of a range of slots
// and folds them into coefficient tables without a host round trip, and the order of the physical parameters as the host names them.
// A translation unit of its own, compiled with the flags of quadrace_rollout_cond.hip (the build's defaults): the code objects of the
// other sources do not change when this one does, and the vehicle mode stays comparable with the condition mode it is timed against.
#include "quadrace_rollout_group.hpp"

namespace qr {

// conds: [capacity][kCondSlotFloats] floats; dyns: [capacity][kDynSlotFloats] floats; map: [num_groups] (dynamics, condition), every index
// already checked against its bank by the caller.  envs_per_group % kBlock == 0 and num_groups * envs_per_group == P.n are checked again
// here: a grid that does not match P.n would read and write out of bounds.
hipError_t launch_rollout_policy_dynamics(int variant, const Params& P, const PolicyArgs& A, const float* conds, const float* dyns, const int2* map,
                                          int num_groups, int envs_per_group, int K, float* obs, float* act, float* logp, float* rew, uint8_t* done,
                                          uint8_t* trunc, float* last_obs, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !conds || !dyns || !map)
        return hipErrorInvalidValue;
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value, L = obs_len<V, GA>();
        const size_t lds = (size_t)PolicyDims<L>::kTotalHalf8 * 16 + sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * L);
        float4* act4 = reinterpret_cast<float4*>(act);
        const dim3 grid((unsigned)(P.n / kBlock));
        const int wgs = envs_per_group / kBlock;
        const half8* no_bank = nullptr;   // one policy per launch: A.weights / A.weights_lo and A's sampling arguments
        const PopulationEntry* no_table = nullptr;
        const float* no_sens = nullptr;   // no sensor: the four arguments behind dyns are not read
        const int* no_sen_map = nullptr;
        float* no_pending = nullptr;
        float* no_critic = nullptr;    // no privileged-critic rows: the two last arguments are not read
        if (A.f32class)
            return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, true, false, true>>(grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds,
                                                                                             map, no_table, wgs, K, obs, act4, logp, rew, done, trunc,
                                                                                             last_obs, dyns,
                                                                                             no_sens, no_sen_map, no_pending, SensingStream{}, no_critic, no_critic);
        return launch_dynamic_lds<rollout_policy_group_kernel<V, GA, false, false, true>>(grid, dim3(kBlock), lds, st, P, A, no_bank, no_bank, conds,
                                                                                          map, no_table, wgs, K, obs, act4, logp, rew, done, trunc,
                                                                                          last_obs, dyns,
                                                                                          no_sens, no_sen_map, no_pending, SensingStream{}, no_critic, no_critic);
    });
}

// ---- the sampler of the dynamics bank ------------------------------------------------------------------------------------------------------
// The physical parameters in the order of include/quadrace.h (= dynamics.PHYSICAL[variant] in Python).
enum : int { kPIxx = 0, kPIyy, kPIzz, kPKx, kPKy, kPKz, kPKw, kPKh, kPKp, kPKpv, kPKq, kPKqv, kPKr1, kPKr2, kPKrr, kPTau, kPWMin, kPWMax, kPG };
enum : int { kQKx = 0, kQKy, kQTMax, kQTauP, kQTauQ, kQTauR, kQTauT, kQPMax, kQQMax, kQRMax, kQG };
static_assert(kPG + 1 == QR_DYNAMICS_PHYSICAL_E2E && kQG + 1 == QR_DYNAMICS_PHYSICAL_INDI, "the header's counts");
static const char* const kPhysE2ENames[QR_DYNAMICS_PHYSICAL_E2E] = {"Ixx", "Iyy", "Izz", "k_x", "k_y", "k_z", "k_w", "k_h", "k_p", "k_pv", "k_q", "k_qv",
                                                                    "k_r1", "k_r2", "k_rr", "tau", "w_min", "w_max", "g"};
static const char* const kPhysINDINames[QR_DYNAMICS_PHYSICAL_INDI] = {"k_x", "k_y", "T_max", "tau_p", "tau_q", "tau_r", "tau_T", "p_max", "q_max", "r_max",
                                                                      "g"};
const char* const* dynamics_physical_names(int variant, int* count) {
    if (variant == kE2E) {
        *count = QR_DYNAMICS_PHYSICAL_E2E;
        return kPhysE2ENames;
    }
    if (variant == kINDI) {
        *count = QR_DYNAMICS_PHYSICAL_INDI;
        return kPhysINDINames;
    }
    *count = 0;
    return nullptr;
}

// the bounds of one call, by value in the kernel arguments: no device copy of a host array, nothing to keep alive behind the launch
struct DynRanges {
    double lo[QR_DYNAMICS_PHYSICAL_E2E], hi[QR_DYNAMICS_PHYSICAL_E2E];
};

// One thread per slot: slot s = first_slot + thread, physical parameter j = lo[j] + (hi[j] - lo[j]) * (double)u01(word j % 4 of
// Philox4x32-10(counter (s, j / 4, draw lo, draw hi), key)), then the fold of dynamics.fold_physical in float64 in its operation order
// -- every product, quotient and difference rounded on its own (contraction off: an a*b+c fused here would differ from NumPy in the last
// bit) -- and ONE rounding to float32.  The slot's 32 floats are written whole: the table, then zeros.
template <int V>
__global__ void __launch_bounds__(64)
dynamics_sample_kernel(float* __restrict__ slots, int first_slot, int num_slots, DynRanges R, uint32_t k0, uint32_t k1, uint32_t draw_lo,
                       uint32_t draw_hi) {
#pragma clang fp contract(off)
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= num_slots) return;
    const int s = first_slot + t;
    constexpr int kCount = V == kE2E ? QR_DYNAMICS_PHYSICAL_E2E : QR_DYNAMICS_PHYSICAL_INDI;
    double p[kCount];
#pragma unroll
    for (int b = 0; b < (kCount + 3) / 4; ++b) {
        uint32_t x[4];
        philox4x32_10((uint32_t)s, (uint32_t)b, draw_lo, draw_hi, k0, k1, x);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int j = 4 * b + w;
            if (j < kCount) {
                const double span = R.hi[j] - R.lo[j];
                const double part = span * (double)u01(x[w]);
                p[j] = R.lo[j] + part;
            }
        }
    }
    double c[kDynSlotFloats];
#pragma unroll
    for (int k = 0; k < kDynSlotFloats; ++k) c[k] = 0.0;
    if constexpr (V == kE2E) {
        const double half = (p[kPWMax] - p[kPWMin]) / 2.0;
        c[kEMotorGain] = half;
        c[kEMotorOffset] = half + p[kPWMin];
        c[kENegKx] = -p[kPKx];
        c[kENegKy] = -p[kPKy];
        c[kENegKw] = -p[kPKw];
        c[kENegKz] = -p[kPKz];
        c[kENegKh] = -p[kPKh];
        c[kEG] = p[kPG];
        c[kEPM] = 1.0 / p[kPIxx];
        c[kEPQR] = (p[kPIyy] - p[kPIzz]) / p[kPIxx];
        c[kEPVby] = p[kPKpv] / p[kPIxx];
        c[kEPW] = p[kPKp] / p[kPIxx];
        c[kEQM] = 1.0 / p[kPIyy];
        c[kEQPR] = (p[kPIzz] - p[kPIxx]) / p[kPIyy];
        c[kEQVbx] = p[kPKqv] / p[kPIyy];
        c[kEQW] = p[kPKq] / p[kPIyy];
        c[kERM] = 1.0 / p[kPIzz];
        c[kERPQ] = (p[kPIxx] - p[kPIyy]) / p[kPIzz];
        c[kERR] = -p[kPKrr] / p[kPIzz];
        const double neg_cmd = -p[kPKr2] * half;       // -k_r2 * half / tau / Izz, left to right
        const double neg_cmd_tau = neg_cmd / p[kPTau];
        c[kERCmd] = neg_cmd_tau / p[kPIzz];
        const double cmd = p[kPKr2] * half;            // (k_r2 * half / tau - k_r1 * half) / Izz
        const double cmd_tau = cmd / p[kPTau];
        const double mot = p[kPKr1] * half;
        const double mix = cmd_tau - mot;
        c[kERMotor] = mix / p[kPIzz];
        c[kEMotorLag] = 1.0 / p[kPTau];
    } else {
        c[kINegKx] = -p[kQKx];
        c[kINegKy] = -p[kQKy];
        c[kIThrustGain] = -p[kQTMax] / 2.0;
        c[kIThrustOffset] = -p[kQTMax] / 2.0;
        c[kIG] = p[kQG];
        c[kIPLag] = -1.0 / p[kQTauP];
        c[kIPCmd] = p[kQPMax] / p[kQTauP];
        c[kIQLag] = -1.0 / p[kQTauQ];
        c[kIQCmd] = p[kQQMax] / p[kQTauQ];
        c[kIRLag] = -1.0 / p[kQTauR];
        c[kIRCmd] = p[kQRMax] / p[kQTauR];
        c[kITLag] = 1.0 / p[kQTauT];
    }
    float4* dst = reinterpret_cast<float4*>(slots + (size_t)s * kDynSlotFloats);   // a slot is 128 bytes, 16-byte aligned
#pragma unroll
    for (int k = 0; k < kDynSlotFloats / 4; ++k)
        dst[k] = make_float4((float)c[4 * k + 0], (float)c[4 * k + 1], (float)c[4 * k + 2], (float)c[4 * k + 3]);
}

// slots: slot 0 of [capacity][kDynSlotFloats]; lo / hi: HOST arrays of the variant's physical count, already validated; the slot range is
// inside the bank (the caller's check).  Stream-ordered, no synchronisation.
hipError_t launch_dynamics_sample(int variant, float* slots, int first_slot, int num_slots, const double* lo, const double* hi, uint64_t seed,
                                  uint64_t draw, hipStream_t st) {
    int count = 0;
    if (!dynamics_physical_names(variant, &count) || !slots || !lo || !hi || first_slot < 0 || num_slots < 1) return hipErrorInvalidValue;
    DynRanges R{};
    for (int j = 0; j < count; ++j) {
        R.lo[j] = lo[j];
        R.hi[j] = hi[j];
    }
    // Domain separation: the reset stream's key is the env seed itself, the action noise's seed ^ (0x9E3779B9, 0x85EBCA6B), the ES noise's
    // seed ^ (0x2545F491, 0x4F6CDD1D); the vehicle draws take a tweak of their own (include/quadrace.h)
    const uint32_t k0 = (uint32_t)seed ^ QR_DYNAMICS_SAMPLE_KEY_LO, k1 = (uint32_t)(seed >> 32) ^ QR_DYNAMICS_SAMPLE_KEY_HI;
    const dim3 grid((unsigned)((num_slots + 63) / 64)), block(64);
    if (variant == kE2E)
        hipLaunchKernelGGL(dynamics_sample_kernel<kE2E>, grid, block, 0, st, slots, first_slot, num_slots, R, k0, k1, (uint32_t)draw, (uint32_t)(draw >> 32));
    else
        hipLaunchKernelGGL(dynamics_sample_kernel<kINDI>, grid, block, 0, st, slots, first_slot, num_slots, R, k0, k1, (uint32_t)draw, (uint32_t)(draw >> 32));
    return hipGetLastError();
}

}  // namespace qr
