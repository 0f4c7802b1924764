// quadrace_blackbox.hip -- the on-device BLACK BOX (qr_blackbox_policy): the closed loop of the flight recorder (quadrace_record.hip), all
// N envs, but each env keeps only its last W rows, in a ring [W][M][R], and stops overwriting them when its episode ends the way the
// caller asked about (crash, time limit, either, never).  The footprint is W M rows instead of K M; the write traffic is at most the
// recorder's.  What an env looked like in the seconds before it crashed is then in the ring, oldest to newest ending at the trigger row,
// together with the terminal world state (after the integration, before the auto-reset) and the cause of the end.
//
// The step loop RESTATES record_policy_kernel's, statement for statement, the way quadrace_rollout_group.hpp restates the rollout
// kernel's: that kernel's matrix-instruction schedule is pinned, and a body shared with it moves its code.  The three
// tile helpers are not restated: both units take them from quadrace_record_tiles.hpp.  Policy forward, noise slices, clip, step_env
// with reset_from_stash, observe, the end-of-kernel write-back and the row layout R = S + QR_RECORD_EXTRA are the recorder's: the env
// state after the call is bit-identical to qr_record_policy / qr_rollout_policy, whatever trigger, window and rec_envs are.
//
// What differs:
//   * ring addressing: the row of call-step k goes to slot (first_step + k) mod W, the same slot for every lane, so the rows of a full,
//     16-byte-aligned wave below M are still one contiguous block of 64 R floats, streamed out in slot 0 of the next step's third layer.
//   * armed / frozen: a lane stores the row of a step iff it was armed at the START of that step (the triggering row itself is stored),
//     and freezes at the end of a step whose end code the trigger selects.  A frozen env flies and resets on exactly as before.
//   * the flush path of the rows of step k is a SCALAR decided by a ballot at the end of step k (a wave-uniform jump between the pinned
//     matrix instructions, not an EXEC mask): every lane was armed and the wave qualifies for the block -> block; some lane was armed
//     -> the per-lane flush at the loop top, masked by "was armed"; none -> nothing is stored.  A wave without an armed lane also stops
//     filling its tile.
//   * the trigger step, inside step_env's before_reset hook where e.s is the terminal state: the lane stores it to term [M][S] right
//     there (rare, outside the pinned schedule, nothing held in registers across the loop) and derives the cause bits from it with the
//     comparisons of step_dynamics.
//   * status st [M][4] int32 {frozen, rows stored so far, ring slot of the trigger row or -1, cause bits}: read at the start, written at
//     the end, so a call can be continued (consecutive first_step, same window, same buffers).
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"
#include "quadrace_record_tiles.hpp"

namespace qr {

static_assert(QR_RECORD_EXTRA == 8 && QR_BLACKBOX_ST_INTS == 4, "row and status layout of include/quadrace.h");

enum : int { kFlushNone = 0, kFlushBlock = 1, kFlushLanes = 2 };

// slot0 = first_step mod window (the host's 64-bit remainder); term may be null
template <int V, int GA, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
blackbox_policy_kernel(Params P, PolicyArgs A, int K, int M, int trigger, int window, int slot0, float* __restrict__ ring,
                       int4* __restrict__ st, float* __restrict__ term) {
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
    // Which rows this wave may record, as SCALAR values (rec_envs <= n, so a wave below it is a full wave).
    const int wave_first = __builtin_amdgcn_readfirstlane(i - lane);
    const bool rec_block = wave_first + 64 <= M && (R % 4 == 0 || (M & 3) == 0);       // all 64, and every slot's block 16-byte aligned
    const bool rec_env = i < M;                                                        // this env has a ring column and a status
    float* tile = gates + kMaxGates * kGateStride + (threadIdx.x >> 6) * 64 * R;
    float* trow = tile + lane * R;
    const size_t slot_floats = (size_t)M * R;
    const size_t row_off = (size_t)(rec_env ? i : 0) * R;   // this lane's row inside a slot
    const size_t block_off = (size_t)(rec_block ? wave_first : 0) * R;
    // the status: read here, written at the end
    int4 status = make_int4(1, 0, -1, 0);
    if (rec_env) status = st[i];
    if (status.x == 0) { status.z = -1; status.w = 0; }   // an armed env has no trigger row yet: a zeroed status is a fresh one
    bool armed = rec_env && status.x == 0;
    bool was_armed = false;                         // armed at the start of the step whose row sits in the tile
    bool live = __ballot(armed) != 0ull;            // scalar: some lane of the wave is armed at the start of this step
    int flush_prev = kFlushNone;                    // scalar: how the rows of step k - 1 leave
    int slot = slot0 == 0 ? window - 1 : slot0 - 1; // scalar: ring slot of step k - 1 (advanced behind the forward)
    bool any_reset = false;
    float stash[reset_value_count<V>()];   // the lane's own next reset draws (reset_from_stash)
    bool stash_ok = false;
    float o[L];
    observe<V, GA>(P, gates, e, o);
    for (int k = 0; k < K; ++k) {
        // a lane-masked store block stays outside the forward's pinned schedule: the rows of step k - 1 of a wave without a block
        if (flush_prev == kFlushLanes && was_armed) rec_row_flush<R>(trow, ring + (size_t)slot * slot_floats + row_off);
        // ---- action noise: rollout_policy_kernel's slices, verbatim (drawn in deterministic mode too and then multiplied out)
        float mean[4];
        float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t pc[4];
        float bm_u1a, bm_u2a, bm_u1b, bm_u2b, bm_ra, bm_rb, bm_sa, bm_ca, bm_sb, bm_cb;
        auto pin_u = [](uint32_t& x) { asm volatile("" : "+v"(x)); };
        auto pin_f = [](float& x) { asm volatile("" : "+v"(x)); };
        auto noise_slice = [&](int ns) {
            if (ns >= 1 && ns <= 11) { pin_u(pc[0]); pin_u(pc[1]); pin_u(pc[2]); pin_u(pc[3]); }
            if (ns == 12) pin_f(bm_u1a);
            if (ns == 13) pin_f(bm_u1b);
            if (ns == 14) pin_f(bm_u2a);
            if (ns == 15) pin_f(bm_u2b);
            if (ns == 16) { pin_f(bm_ra); pin_f(bm_rb); pin_f(bm_sa); pin_f(bm_sb); }
            if (ns == 0) {
                const uint32_t s_lo = A.step_lo + (uint32_t)k;
                pc[0] = gid_lo; pc[1] = gid_hi; pc[2] = s_lo; pc[3] = A.step_hi + (s_lo < A.step_lo ? 1u : 0u);
            } else if (ns <= 10) {
                philox4x32_round(pc, A.seed_lo, A.seed_hi, ns - 1);
            } else if (ns == 11) {  // Box-Muller: two pairs of normals from four uniforms (u1 in (0,1], u2 in [0,1))
                bm_u1a = (float)((pc[0] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2a = u01(pc[1]);
                bm_u1b = (float)((pc[2] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2b = u01(pc[3]);
            } else if (ns == 12) {
                bm_ra = fast_sqrt(-2.0f * __logf(bm_u1a));
            } else if (ns == 13) {
                bm_rb = fast_sqrt(-2.0f * __logf(bm_u1b));
            } else if (ns == 14) {
                qr_sincos(6.283185307179586f * bm_u2a, bm_sa, bm_ca);
            } else if (ns == 15) {
                qr_sincos(6.283185307179586f * bm_u2b, bm_sb, bm_cb);
            } else if (ns == 16) {
                eps[0] = bm_ra * bm_ca; eps[1] = bm_ra * bm_sa; eps[2] = bm_rb * bm_cb; eps[3] = bm_rb * bm_sb;
            }
        };
        // Under the third layer's MFMAs: slot 0 streams out the block of step k - 1 (complete since the end of that step), slot 2 puts the
        // world columns of step k into the tile (LDS operations of one wave execute in order: the flush's reads come first).  Both
        // conditions are scalars.
        auto rec_slice = [&](int rs) {
            if (rs == 0 && flush_prev == kFlushBlock) rec_tile_flush<R>(tile, ring + (size_t)slot * slot_floats + block_off, lane);
            if (rs == 2 && live) rec_tile_write<R, 0, S>(trow, e.s);
        };
        if constexpr (kF32) {
#pragma unroll
            for (int ns = 0; ns <= 16; ++ns) noise_slice(ns);
            rec_slice(0);
            rec_slice(2);
            policy_forward_f32class<L>(W, A.weights_lo, lane, o, mean);
        } else {
            policy_forward<L>(W, lane, o, mean, noise_slice, rec_slice);
        }
        slot = slot + 1 == window ? 0 : slot + 1;   // now the slot of step k
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
        bool hit = false;
        const float reward = step_env<V>(P, gates, rtab, nullptr, mlp, lane, active, e, u, gid_lo, gid_hi, done, trunc, did_reset,
                                         [&](bool d) {
                                             // the trigger step: e.s is the terminal state (after the integration, before the auto-reset)
                                             hit = armed && d && ((trunc ? 2 : 1) & trigger) != 0;
                                             if (hit) {
                                                 const bool ground = e.s[2] > 0.0f;
                                                 const bool oob = (fabsf(e.s[0]) > 10.0f) || (fabsf(e.s[1]) > 10.0f) || (fabsf(e.s[9]) > 1000.0f) ||
                                                                  (fabsf(e.s[10]) > 1000.0f) || (fabsf(e.s[11]) > 1000.0f);
                                                 status.w = (ground ? 1 : 0) | (oob ? 2 : 0) | (trunc ? 4 : 0) | (!trunc && !ground && !oob ? 8 : 0);
                                                 status.z = slot;
                                                 if (term != nullptr) {
#pragma unroll
                                                     for (int q = 0; q < S; ++q) term[(size_t)i * S + q] = e.s[q];
                                                 }
                                             }
                                         },
                                         [&](bool need) { reset_from_stash<V>(P, rtab, need, e, gid_lo, gid_hi, stash, stash_ok); });
        any_reset |= did_reset;
        if (live) {
            const float tail[8] = {u[0], u[1], u[2], u[3], reward, done ? (trunc ? 2.0f : 1.0f) : 0.0f, (float)target_before, (float)steps_before};
            rec_tile_write<R, S, 8>(trow, tail);
        }
        // the row of this step is stored iff the lane was armed at its start; how it leaves is decided for the whole wave
        was_armed = armed;
        status.y += armed ? 1 : 0;
        if (hit) { armed = false; status.x = 1; }
        const unsigned long long stored = __ballot(was_armed);
        flush_prev = stored == 0ull ? kFlushNone : (rec_block && stored == ~0ull ? kFlushBlock : kFlushLanes);
        live = __ballot(armed) != 0ull;
        observe<V, GA>(P, gates, e, o);
    }
    // the rows of the last step
    if (flush_prev == kFlushBlock) rec_tile_flush<R>(tile, ring + (size_t)slot * slot_floats + block_off, lane);
    else if (flush_prev == kFlushLanes && was_armed) rec_row_flush<R>(trow, ring + (size_t)slot * slot_floats + row_off);
    if (!active) return;
    if (rec_env) st[i] = status;
    define_exit_values<V>(e);
    P.ts[i] = pack_ts<V>(e);
    store_world<V>(P, i, e);
    if (any_reset) store_dist<V>(P, i, e);
}

hipError_t launch_blackbox_policy(int variant, const Params& P, const PolicyArgs& A, int K, int rec_envs, int trigger, int window, int slot0,
                                  float* ring, int32_t* st_rec, float* term, hipStream_t st) {
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value, L = obs_len<V, GA>(), R = Env<V>::S + QR_RECORD_EXTRA;
        const size_t lds = (size_t)PolicyDims<L>::kTotalHalf8 * 16 + sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + kBlock * R);
        int4* st4 = reinterpret_cast<int4*>(st_rec);
        if (A.f32class)
            return launch_dynamic_lds<blackbox_policy_kernel<V, GA, true>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, rec_envs, trigger, window,
                                                                           slot0, ring, st4, term);
        return launch_dynamic_lds<blackbox_policy_kernel<V, GA, false>>(grid_for(P.n), dim3(kBlock), lds, st, P, A, K, rec_envs, trigger, window,
                                                                        slot0, ring, st4, term);
    });
}

}  // namespace qr
