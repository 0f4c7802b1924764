// quadrace_kernels.hip -- host side of the env kernels (quadrace_env_kernels.hpp): which kernel runs a K-step call, and the launchers
// quadrace_abi.hip calls (prototypes in quadrace_launch.hpp).  Also the two kernels that are no templates.  The launcher of the two fused
// E2E + residual-MLP rollout kernels is a translation unit of its own, quadrace_kernels_mlp.hip.
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"

namespace qr {

// qr_probe_residual: body velocity (R:103) and the residual thrust / moment MLP outputs (R:254-262) of the CURRENT state
// of every env, row [vbx vby vbz thrust Mx My Mz] -- the same device functions the step kernels inline, exposed so that
// parity tests can pin them directly against the reference's fixture rows instead of through finite differences.
__global__ void __launch_bounds__(kBlock) residual_probe_kernel(Params P, float* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = i < P.n;   // MFMA / permlane are wave-wide: tail lanes shadow env 0
    Env<kE2E> e;
    load_env<kE2E>(P, active ? i : 0, e);
    MlpRegs mlp;
    mlp_load_regs(P.tables, lane, mlp);
    const Rot R = make_rot(e.s[6], e.s[7], e.s[8]);
    float vb[3];
    vb[0] = fmaf(e.s[3], R.r00, fmaf(e.s[4], R.r10, e.s[5] * R.r20));
    vb[1] = fmaf(e.s[3], R.r01, fmaf(e.s[4], R.r11, e.s[5] * R.r21));
    vb[2] = fmaf(e.s[3], R.r02, fmaf(e.s[4], R.r12, e.s[5] * R.r22));
    const float x[10] = {e.s[12], e.s[13], e.s[14], e.s[15], vb[0], vb[1], vb[2], e.s[9], e.s[10], e.s[11]};
    float thrust, moment[3];
    residual_mlp(mlp, lane, x, thrust, moment);
    if (!active) return;
    float* o = out + (size_t)i * 7;
    o[0] = vb[0]; o[1] = vb[1]; o[2] = vb[2]; o[3] = thrust; o[4] = moment[0]; o[5] = moment[1]; o[6] = moment[2];
}

// qr_seed: restart every env's reset stream (episode counter = 0)
__global__ void __launch_bounds__(kBlock) clear_episode_kernel(Params P) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    int2 ts = P.ts[i];
    ts.x &= 0xFF;
    P.ts[i] = ts;
}

// ---------------------------------------------------------------------------------------------------
// host-callable launchers (used by quadrace_abi.hip)
// ---------------------------------------------------------------------------------------------------
// one workgroup per kBlock envs, static LDS only
template <typename Kernel, typename... Args>
static hipError_t launch_env(Kernel kernel, const Params& P, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kernel, grid_for(P.n), dim3(kBlock), 0, st, P, args...);
    return hipGetLastError();
}

hipError_t launch_step(int variant, const Params& P, const float* actions, float* obs, float* rew, uint8_t* done,
                       uint8_t* trunc, hipStream_t st) {
    const float4* a4 = reinterpret_cast<const float4*>(actions);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        return launch_env(step_kernel<decltype(v)::value, decltype(ga)::value>, P, st, a4, obs, rew, done, trunc);
    });
}

static int n_wgs(int n) { return (n + kBlock - 1) / kBlock; }
static int device_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
    }
    return cus;
}
// Which kernel runs a K-step call -- ONE selection, used by the launcher and by qr_rollout_kernel_name() (bench.py prints the symbol
// rocprofv3 will show, and looks its counter evidence up under that name):
//   at most one workgroup per CU, default mode (no pause flags, no terminal-observation rows):
//       E2E + residual MLPs -> rollout_fast_mlp_kernel, E2E without -> rollout_fast_kernel, INDI -> rollout_stash_kernel (HBM-bound at
//       65 536 envs: the general stash kernel is as fast per step, 2 443 vs 2 503 cycles, and has the shorter prologue)
//   at most one workgroup per CU, any other mode -> rollout_stash_kernel
//   more workgroups, default mode: E2E + residual MLPs -> rollout_lean_mlp_kernel, INDI / E2E without -> rollout_lean_kernel up to four
//       workgroups per CU;
//   more workgroups, anything else -> rollout_kernel
// `form` = qr_set_rollout_form(), two flags: QR_ROLLOUT_MULTI_WAVE (bit 0: the forms built for more than one workgroup per CU at any
// env count), QR_ROLLOUT_GENERAL (bit 1: rollout_stash_kernel / rollout_kernel for every launch); 0 = QR_ROLLOUT_AUTO (the table above).  All forms are
// bit-identical (tests/test_gpu_round4.py); the setter exists for tests and A/B runs -- there is no environment variable.
enum RolloutKernel { kRkFastMlp, kRkFast, kRkStash, kRkLeanMlp, kRkLean, kRkPlain };
static RolloutKernel select_rollout(int variant, const Params& P, int form) {
    const bool plain_mode = !(P.flags & (kFlagPause | kFlagPauseIfCollision)) && P.term_obs == nullptr && !(form & 2);
    const bool mlp = variant == kE2E && (P.flags & kFlagResidual);
    if ((form & 4) || (n_wgs(P.n) <= device_cus() && !(form & 1))) {   // one wave per SIMD: the register file of a whole SIMD per wave (reset stash, operands in registers)
        if (plain_mode && mlp) return kRkFastMlp;
        if (plain_mode && variant == kE2E) return kRkFast;
        return kRkStash;
    }
    if (plain_mode && mlp) return kRkLeanMlp;
    // without the MLPs the model is memory-bound, and the lean form's LDS (52 KB: three workgroups per CU) is its occupancy limit where
    // the general form has four: INDI 61.8 vs 56.4 G env-steps/s at 262 144 envs (4 workgroups of work per CU), 56.4 vs 58.0 at 1 Mi
    if (plain_mode && (n_wgs(P.n) <= 4 * device_cus())) return kRkLean;
    return kRkPlain;
}

const char* rollout_kernel_name(int variant, const Params& P, int form) {
    switch (select_rollout(variant, P, form)) {
        case kRkFastMlp: return "rollout_fast_mlp_kernel";
        case kRkFast: return "rollout_fast_kernel";
        case kRkStash: return "rollout_stash_kernel";
        case kRkLeanMlp: return "rollout_lean_mlp_kernel";
        case kRkLean: return "rollout_lean_kernel";
        default: return "rollout_kernel";
    }
}

hipError_t launch_rollout(int variant, const Params& P, int form, int K, const float* actions, float* obs, float* rew,
                          uint8_t* done, uint8_t* trunc, hipStream_t st) {
    const float4* a4 = reinterpret_cast<const float4*>(actions);
    switch (select_rollout(variant, P, form)) {
        case kRkFastMlp: return launch_rollout_mlp(false, P, K, a4, obs, rew, done, trunc, st);
        case kRkLeanMlp: return launch_rollout_mlp(true, P, K, a4, obs, rew, done, trunc, st);
        case kRkFast:
            return dispatch_ga(P.gates_ahead, [&](auto ga) {
                return launch_env(rollout_fast_kernel<kE2E, decltype(ga)::value>, P, st, K, a4, obs, rew, done, trunc);
            });
        case kRkLean:   // the lean forms' LDS is dynamic (more than the 64 KB a static array may have)
            return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
                constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
                return launch_dynamic_lds<rollout_lean_kernel<V, GA>>(grid_for(P.n), dim3(kBlock), lean_lds_bytes<V, GA, false>(), st, P, K,
                                                                      a4, obs, rew, done, trunc);
            });
        case kRkStash:
            return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
                return launch_env(rollout_stash_kernel<decltype(v)::value, decltype(ga)::value>, P, st, K, a4, obs, rew, done, trunc);
            });
        default:
            return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
                return launch_env(rollout_kernel<decltype(v)::value, decltype(ga)::value>, P, st, K, a4, obs, rew, done, trunc);
            });
    }
}

hipError_t launch_rollout_policy(int variant, const Params& P, const PolicyArgs& A, int K, float* obs, float* act,
                                 float* logp, float* rew, uint8_t* done, uint8_t* trunc, float* last_obs,
                                 hipStream_t st) {
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value, L = obs_len<V, GA>();
        const size_t lds = (size_t)PolicyDims<L>::kTotalHalf8 * 16 +
                           sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * L);
        float4* act4 = reinterpret_cast<float4*>(act);
        if (A.f32class)
            return launch_dynamic_lds<rollout_policy_kernel<V, GA, true>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, obs, act4, logp,
                                                                          rew, done, trunc, last_obs);
        return launch_dynamic_lds<rollout_policy_kernel<V, GA, false>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, obs, act4, logp,
                                                                       rew, done, trunc, last_obs);
    });
}

hipError_t launch_reset(int variant, const Params& P, const uint8_t* mask, float* obs, hipStream_t st) {
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        return launch_env(reset_kernel<decltype(v)::value, decltype(ga)::value>, P, st, mask, obs);
    });
}

hipError_t launch_observe(int variant, const Params& P, float* obs, hipStream_t st) {
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        return launch_env(observe_kernel<decltype(v)::value, decltype(ga)::value>, P, st, obs);
    });
}

hipError_t launch_residual_probe(const Params& P, float* out, hipStream_t st) { return launch_env(residual_probe_kernel, P, st, out); }

hipError_t launch_clear_episode(const Params& P, hipStream_t st) { return launch_env(clear_episode_kernel, P, st); }

hipError_t launch_get_state(int variant, const Params& P, float* world, float* dist, int32_t* target, int32_t* steps,
                            uint32_t* episode, hipStream_t st) {
    return launch_env(variant == kE2E ? get_state_kernel<kE2E> : get_state_kernel<kINDI>, P, st, world, dist, target, steps, episode);
}

hipError_t launch_set_state(int variant, const Params& P, const float* world, const float* dist,
                            const int32_t* target, const int32_t* steps, const uint32_t* episode, hipStream_t st) {
    return launch_env(variant == kE2E ? set_state_kernel<kE2E> : set_state_kernel<kINDI>, P, st, world, dist, target, steps, episode);
}

}  // namespace qr
