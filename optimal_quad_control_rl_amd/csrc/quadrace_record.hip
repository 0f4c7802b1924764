// quadrace_record.hip -- the on-device FLIGHT RECORDER (qr_record_policy): K x [obs -> MFMA policy -> a = mean + std * eps -> env.step(clip(a))]
// in one kernel, the closed loop of rollout_policy_kernel (quadrace_env_kernels.hpp), whose whole per-step output is ONE packed row per
// env: the world state the action was computed from, the command the env received, the reward, how the step ended, the target gate and
// the episode clock (layout: include/quadrace.h).  The opposite extreme of eval_policy_kernel (quadrace_eval.hip), which stores nothing
// per step.  A translation unit of its own: the code objects of the other sources do not change when this one does.
//
// Noise draws, env arithmetic, reset stream and the end-of-kernel state write-back are rollout_policy_kernel's, statement for statement
// (tests/test_gpu_record.py demands bit equality with it); what that kernel stores (observation, unclipped action, log-prob, reward, done,
// trunc, terminal observations: six streams) is not stored here, and the log-prob is not computed.  The three tile helpers are in
// quadrace_record_tiles.hpp, which the black box includes too.
//
// Write shape: the rows [k][wave_first .. wave_first + 64) of a full wave are one contiguous block of 64 R floats.  Each lane assembles its
// row in a wave-private LDS tile (the pre-step world columns go there BEFORE the step, so that no copy of the state is held in registers
// across step_env; the command and the four trailing columns behind it), and the wave streams the block out with 16-byte-per-lane stores
// in the MFMA shadow of the NEXT step's policy forward -- the stores are issued and never waited for inside the loop.
//   LDS traffic of the transposed write (64 lanes, row stride R floats): E2E R = 24 -> six ds_write_b128 per step; a b128 write is served
//   in groups of 8 consecutive lanes with banks (a/4) mod 32, and 8 rows of 24 floats start at banks 0, 24, 16, 8, 0, ... : each bank of
//   a group is touched by exactly 4 lanes' quads -- no worse than any other 16-byte write of 8 lanes (128 B through 32 banks), and the
//   register-to-LDS transfer, not the array, sets the cost of a wide write.  INDI R = 21 is odd: its ds_write_b32 are conflict-free.
//   The flush reads the tile linearly (ds_read_b128, consecutive lanes on consecutive 16-byte slots: conflict-free).
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"
#include "quadrace_record_tiles.hpp"

namespace qr {

static_assert(QR_RECORD_EXTRA == 8, "row layout of include/quadrace.h");

template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
record_policy_kernel(Params P, PolicyArgs A, int K, int M, float* __restrict__ rows) {
    constexpr int L = obs_len<V, GA>(), S = Env<V>::S, R = S + QR_RECORD_EXTRA;
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);                                   // policy weights (f16)
    float* rtab = reinterpret_cast<float*>(smem + (size_t)D::kTotalHalf8 * 16);  // reset table | gate rows | record tiles
    float* gates = rtab + kResetTableFloats;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = i < P.n;   // MFMA / permlane are wave-wide: tail lanes shadow env 0 and store nothing
    const int ii = active ? i : 0;
    Env<V> e;
    load_env<V>(P, ii, e);
    MlpRegs mlp;
    const bool use_mlp = (V == kE2E) && (P.flags & kFlagResidual);
    if (use_mlp) mlp_load_regs(P.tables, lane, mlp);
    {
        const float4* s4 = reinterpret_cast<const float4*>(A.weights);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int j = threadIdx.x; j < D::kTotalHalf8; j += kBlock) d4[j] = s4[j];
    }
    stage_tables(P, rtab, kOffResetImage, kResetTableFloats + P.num_gates * kGateStride);
    __syncthreads();
    const uint32_t gid_lo = P.gid_lo + (uint32_t)ii;
    const uint32_t gid_hi = P.gid_hi + (gid_lo < P.gid_lo ? 1u : 0u);
    // Which rows this wave records, as SCALAR values: the branches on them are wave-uniform jumps, not EXEC masks (the flush runs
    // between the pinned matrix instructions of the forward).  rec_envs <= n, so a wave below it is a full wave.
    const int wave_first = __builtin_amdgcn_readfirstlane(i - lane);
    const bool rec_wave = wave_first < M;                                              // some lane of the wave is recorded
    const bool rec_block = wave_first + 64 <= M && (R % 4 == 0 || (M & 3) == 0);       // all 64, and every step's block 16-byte aligned
    const bool rec_lane = rec_wave && !rec_block && i < M;                             // this lane stores its own row
    float* tile = gates + kMaxGates * kGateStride + (threadIdx.x >> 6) * 64 * R;
    float* trow = tile + lane * R;
    const size_t step_floats = (size_t)M * R;
    float* out_prev = rows + (size_t)(rec_block ? wave_first : (rec_lane ? i : 0)) * R;   // where the rows of step k - 1 go
    bool any_reset = false;
    float stash[reset_value_count<V>()];   // the lane's own next reset draws (reset_from_stash)
    bool stash_ok = false;
    float o[L];
    observe<V, GA>(P, gates, e, o);
    for (int k = 0; k < K; ++k) {
        // a lane-masked store block stays outside the forward's pinned schedule: the rows of step k - 1 of a wave without a block
        if (k > 0 && rec_lane) rec_row_flush<R>(trow, out_prev);
        // ---- action noise: rollout_policy_kernel's slices, verbatim (drawn in deterministic mode too and then multiplied out)
        float mean[4];
        float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t pc[4];
        float bm_u1a, bm_u2a, bm_u1b, bm_u2b, bm_ra, bm_rb, bm_sa, bm_ca, bm_sb, bm_cb;
        auto pin_u = [](uint32_t& x) { asm volatile("" : "+v"(x)); };
        auto pin_f = [](float& x) { asm volatile("" : "+v"(x)); };
        auto noise_slice = [&](int slot) {
            if (slot >= 1 && slot <= 11) { pin_u(pc[0]); pin_u(pc[1]); pin_u(pc[2]); pin_u(pc[3]); }
            if (slot == 12) pin_f(bm_u1a);
            if (slot == 13) pin_f(bm_u1b);
            if (slot == 14) pin_f(bm_u2a);
            if (slot == 15) pin_f(bm_u2b);
            if (slot == 16) { pin_f(bm_ra); pin_f(bm_rb); pin_f(bm_sa); pin_f(bm_sb); }
            if (slot == 0) {
                const uint32_t s_lo = A.step_lo + (uint32_t)k;
                pc[0] = gid_lo; pc[1] = gid_hi; pc[2] = s_lo; pc[3] = A.step_hi + (s_lo < A.step_lo ? 1u : 0u);
            } else if (slot <= 10) {
                philox4x32_round(pc, A.seed_lo, A.seed_hi, slot - 1);
            } else if (slot == 11) {  // Box-Muller: two pairs of normals from four uniforms (u1 in (0,1], u2 in [0,1))
                bm_u1a = (float)((pc[0] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2a = u01(pc[1]);
                bm_u1b = (float)((pc[2] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2b = u01(pc[3]);
            } else if (slot == 12) {
                bm_ra = fast_sqrt(-2.0f * __logf(bm_u1a));
            } else if (slot == 13) {
                bm_rb = fast_sqrt(-2.0f * __logf(bm_u1b));
            } else if (slot == 14) {
                qr_sincos(6.283185307179586f * bm_u2a, bm_sa, bm_ca);
            } else if (slot == 15) {
                qr_sincos(6.283185307179586f * bm_u2b, bm_sb, bm_cb);
            } else if (slot == 16) {
                eps[0] = bm_ra * bm_ca; eps[1] = bm_ra * bm_sa; eps[2] = bm_rb * bm_cb; eps[3] = bm_rb * bm_sb;
            }
        };
        // Under the third layer's MFMAs: slot 0 streams out the block of step k - 1 (complete since the end of that step), slot 2 puts the
        // world columns of step k -- the state this forward's observation was taken from -- into the tile (LDS operations of one wave
        // execute in order: the flush's reads come first).
        auto rec_slice = [&](int slot) {
            if (slot == 0 && k > 0 && rec_block) rec_tile_flush<R>(tile, out_prev, lane);
            if (slot == 2 && rec_wave) rec_tile_write<R, 0, S>(trow, e.s);
        };
        if constexpr (kF32) {
#pragma unroll
            for (int slot = 0; slot <= 16; ++slot) noise_slice(slot);
            rec_slice(0);
            rec_slice(2);
            policy_forward_f32class<L>(W, A.weights_lo, lane, o, mean);
        } else {
            policy_forward<L>(W, lane, o, mean, noise_slice, rec_slice);
        }
        if (k > 0) out_prev += step_floats;
        float a[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float en = A.deterministic ? 0.0f : eps[c];   // fmaf(std, 0, mean) = mean
            a[c] = fmaf(A.std[c], en, mean[c]);
        }
        float u[4];
        clip_action(a, u);
        const int target_before = e.target, steps_before = e.steps;
        bool done, trunc, did_reset;
        const float reward = step_env<V>(P, gates, rtab, nullptr, mlp, lane, active, e, u, gid_lo, gid_hi, done, trunc, did_reset,
                                         [](bool) {}, [&](bool need) { reset_from_stash<V>(P, rtab, need, e, gid_lo, gid_hi, stash, stash_ok); });
        any_reset |= did_reset;
        if (rec_wave) {
            const float tail[8] = {u[0], u[1], u[2], u[3], reward, done ? (trunc ? 2.0f : 1.0f) : 0.0f, (float)target_before, (float)steps_before};
            rec_tile_write<R, S, 8>(trow, tail);
        }
        observe<V, GA>(P, gates, e, o);
    }
    // the rows of the last step
    if (rec_block) rec_tile_flush<R>(tile, out_prev, lane);
    else if (rec_lane) rec_row_flush<R>(trow, out_prev);
    if (!active) return;
    define_exit_values<V>(e);
    P.ts[i] = pack_ts<V>(e);
    store_world<V>(P, i, e);
    if (any_reset) store_dist<V>(P, i, e);
}

hipError_t launch_record_policy(int variant, const Params& P, const PolicyArgs& A, int K, int rec_envs, float* rows, hipStream_t st) {
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value, L = obs_len<V, GA>(), R = Env<V>::S + QR_RECORD_EXTRA;
        const size_t lds = (size_t)PolicyDims<L>::kTotalHalf8 * 16 + sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * R);
        if (A.f32class)
            return launch_dynamic_lds<record_policy_kernel<V, GA, true>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, rec_envs, rows);
        return launch_dynamic_lds<record_policy_kernel<V, GA, false>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, rec_envs, rows);
    });
}

}  // namespace qr
