// quadrace_eval_body.hpp -- the ONE body of the closed-loop policy evaluators: K x [obs -> MFMA policy -> action = clip(mean) ->
// env.step] with the lap / crash accounting a user reads after training (gate passes, crashes, time-limit ends, lap durations by lap
// number, episode returns) kept in registers next to the env state.  eval_policy_kernel (quadrace_eval.hip), eval_policy_bank_kernel
// (quadrace_eval_bank.hip) and eval_policy_grid_kernel (quadrace_eval_grid.hip) each derive their inputs and call it; the record and
// its accounting exist here and in tests/eval_spec.py, nowhere else.  The dynamics-, sensing- and history-grid kernels call it with their
// classes, and blackbox_policy_grid_kernel (quadrace_blackbox_grid.hip) with a recording class on top: the one form with a per-step output.
//
// The step loop is rollout_policy_kernel's (quadrace_env_kernels.hpp) without everything an evaluation throws away: no action noise
// (no Philox / Box-Muller slices between the matrix instructions), no observation tile, no observation / action / log-prob / reward /
// done rows -- NO global store inside the step loop.  What leaves the kernel is one 24-int record and one 4-float record per env
// (layout: include/quadrace.h, restated on the CPU in tests/eval_spec.py) and the env state after K steps, stored exactly as the
// rollout kernel stores it.
//
// All times are integer step counts, so every sum is exact; the float record is three sequential float32 sums (one add per step, one
// multiply and two adds per finished episode, no FMA), which NumPy float32 reproduces bit for bit.
#pragma once
#include "../../include/quadrace.h"
#include "quadrace_env_kernels.hpp"
#include "quadrace_sensing.hpp"

namespace qr {

static_assert(QR_EVAL_REC_INTS == 24 && QR_EVAL_MAX_LAPS == 8 && QR_EVAL_REC_FLOATS == 4, "record layout of include/quadrace.h");

// dynamic LDS of a kernel that calls eval_policy_body: policy image (f16) | reset table | gate rows | lap sums and counts [16][kBlock]
// (the carve-up at the top of eval_policy_body)
template <int L>
constexpr size_t eval_lds_bytes() {
    return (size_t)PolicyDims<L>::kTotalHalf8 * 16 + sizeof(float) * (kResetTableFloats + kMaxGates * kGateStride + 2 * QR_EVAL_MAX_LAPS * kBlock);
}

// What a kernel supplies (256-thread workgroups, eval_lds_bytes<L>() of dynamic LDS, called by every lane):
//   P              the Params to fly under (the handle's, or a copy with a condition's scalars)
//   img, img_lo    the policy image this workgroup flies and its low pieces (f32-class form only), workgroup-uniform
//   tab            the [reset table | gate rows] image to stage, 16-byte aligned, workgroup-uniform
//   i              the lane's env: state planes, rec and recf are indexed by it
//   rid            the lane's id in the reset stream: the Philox counter's env id is P.gid + rid (64-bit carry as everywhere)
//   gates_per_lap  passes that make a lap
//   C, dyn         the coefficients of the equations of motion: NominalDyn<V> (the literals; the default, dyn a dummy) or RuntimeDyn<V> with
//                  dyn = the set the kernel has loaded into workgroup-uniform registers (quadrace_eval_dynamics.hip)
//   Sn, sen        what lies between the env and the policy (quadrace_sensing.hpp): IdealSensing (the default, sen a dummy: the policy sees
//                  the observation of the step and its command flies in the step; no code) or RuntimeSensing, which supplies
//                  three hooks -- perturb<V, GA>(sen, gid, k, o) in front of the forward, delay(sen) / pending(sen) for the command queue
//                  between clip_action and step_env -- and kSensingQueueFloats more floats of dynamic LDS per lane behind the lap sums
//   H              (RuntimeSensing only; quadrace_eval_history.hip) the policy's row carries the last H clipped commands COMPUTED in the
//                  current episode behind the noisy observation, [o~_k | u_{k-1}, ..., u_{k-H}]: img / img_lo are images of a policy of
//                  obs_len<V, GA + H>() inputs and the kernel supplies eval_lds_bytes of THAT length; the tail is read from and written back
//                  to entries 0 .. H - 1 of `pending`, cleared with the queue (rollout_policy_group_kernel carries the same statements)
//   Rec, rc        what leaves the kernel PER STEP: NoRecording (the default, rc a dummy: nothing -- no global store inside the step loop; no
//                  code) or a recording class (quadrace_blackbox_grid.hip; RuntimeSensing only) whose State<V> carries the black box of
//                  quadrace_blackbox.hip through the loop: begin ahead of it, flush_lanes at its top, slice(s, e.s) in the matrix-instruction
//                  shadow of the third layer, advance behind the forward, on_end inside step_env's before_reset hook (e.s is the terminal
//                  state), row_tail behind the step, finish / store_status behind the loop -- and kBlock rows of R floats of dynamic LDS
//                  behind the command queue.  The row's command is the one FLOWN (u behind the queue), its state the true e.s.
// kTail: lanes with i >= P.n exist (MFMA / permlane are wave-wide: they shadow env 0 and store nothing); without it i < P.n holds
// for every lane, every lane is an env and every lane stores.
struct NoRecording {
    using Arg = int;
    static constexpr bool kOn = false;
    template <int V>
    struct State {};
};

template <int V, int GA, bool kF32, bool kTail, class C = NominalDyn<V>, class Sn = IdealSensing, int H = 0, class Rec = NoRecording>
__device__ __forceinline__ void eval_policy_body(const Params& P, const half8* __restrict__ img, const half8* __restrict__ img_lo,
                                                 const float* __restrict__ tab, int i, int rid, int K, int gates_per_lap,
                                                 int4* __restrict__ rec, float4* __restrict__ recf, typename C::Arg dyn = typename C::Arg(),
                                                 typename Sn::Arg sen = typename Sn::Arg(), typename Rec::Arg rc = typename Rec::Arg()) {
    static_assert(!Rec::kOn || (Sn::kOn && !kTail), "a recording class rides on the sensing-grid form: every lane an env, the tile behind the queue");
    static_assert(H == 0 || (Sn::kOn && H >= 1 && GA + H <= 4), "the command history needs the sensing hooks, 1 <= H <= 4 - GA");
    constexpr int LE = obs_len<V, GA>();       // the env's row: observe, the sensor's noise
    constexpr int L = obs_len<V, GA + H>();    // the policy's row [o~ | h] = LE + 4 H floats (H = 0: LE)
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);                                   // policy weights (f16) of THIS workgroup's policy
    float* rtab = reinterpret_cast<float*>(smem + (size_t)D::kTotalHalf8 * 16);  // reset table | gate rows | lap sums and counts
    float* gates = rtab + kResetTableFloats;
    const int lane = threadIdx.x & 63;
    const bool active = !kTail || i < P.n;
    const int ii = active ? i : 0;
    Env<V> e;
    load_env<V>(P, ii, e);
    // the lane's record: read here, written behind the loop (a caller continues an evaluation by passing the same buffers again)
    const int4 r0 = rec[(size_t)ii * 6], r1 = rec[(size_t)ii * 6 + 1];
    // lap sums / counts [16][kBlock] live in LDS: they are touched at lap boundaries only (a few times per thousand steps), indexed by
    // the lap number, and 16 registers held through the policy forward are 16 registers the f32-class forward does not have
    int* laps = reinterpret_cast<int*>(gates + kMaxGates * kGateStride) + threadIdx.x;
    {   // (register pressure: v[] lives only from these four loads to the 16 LDS writes below, all ahead of the weight staging and the loop)
        const int4 b = rec[(size_t)ii * 6 + 2], c = rec[(size_t)ii * 6 + 3], d = rec[(size_t)ii * 6 + 4], f = rec[(size_t)ii * 6 + 5];
        const int v[2 * QR_EVAL_MAX_LAPS] = {r1.z, r1.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w, f.x, f.y};
#pragma unroll
        for (int q = 0; q < 2 * QR_EVAL_MAX_LAPS; ++q) laps[q * kBlock] = v[q];   // own column only: no barrier needed
    }
    int n_gates = r0.x, n_crash = r0.y, n_limit = r0.z, since = r0.w, lap_t0 = r1.x, now = r1.y;
    // passes into the running lap and laps finished since the (re)start: kept instead of dividing `since` on every step
    int lap_no = since / gates_per_lap, in_lap = since - lap_no * gates_per_lap;
    float ep_ret = 0.0f, ret_sum = 0.0f, ret_sq = 0.0f;
    if (recf) {
        const float4 f = recf[ii];
        ep_ret = f.x; ret_sum = f.y; ret_sq = f.z;
    }
    MlpRegs mlp;
    const bool use_mlp = (V == kE2E) && (P.flags & kFlagResidual);
    if (use_mlp) mlp_load_regs(P.tables, lane, mlp);
    {
        const float4* s4 = reinterpret_cast<const float4*>(img);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int j = threadIdx.x; j < D::kTotalHalf8; j += kBlock) d4[j] = s4[j];
    }
    {   // [reset table | gate rows], as stage_tables copies the handle's (counts are multiples of 4)
        const float4* s4 = reinterpret_cast<const float4*>(tab);
        float4* d4 = reinterpret_cast<float4*>(rtab);
        const int count4 = (kResetTableFloats + P.num_gates * kGateStride) / 4;
        for (int j = threadIdx.x; j < count4; j += kBlock) d4[j] = s4[j];
    }
    __syncthreads();
    const uint32_t gid_lo = P.gid_lo + (uint32_t)(active ? rid : 0);
    const uint32_t gid_hi = P.gid_hi + (gid_lo < P.gid_lo ? 1u : 0u);
    // the command queue (Sn::kOn only): a ring of d = delay commands in the lane's own LDS column behind the lap sums.  The command of
    // call-step k sits in ring slot k mod d, the same slot for every lane -- a cleared queue is all zeros, so an episode end moves nothing.
    // The caller's buffer holds it in canonical order (entry j = the command computed j + 1 steps ago), so slot d - 1 - j <- entry j.
    if constexpr (Sn::kOn) {
        const int d = Sn::delay(sen);
        if (d > 0) {
            float* ring = reinterpret_cast<float*>(laps + 2 * QR_EVAL_MAX_LAPS * kBlock);
            const float4* pend = reinterpret_cast<const float4*>(Sn::pending(sen)) + (size_t)ii * kMaxDelay;
#pragma unroll
            for (int j = 0; j < kMaxDelay; ++j) {
                if (j < d) {
                    const float4 c = pend[j];
                    float* slot = ring + (d - 1 - j) * 4 * kBlock;
                    slot[0] = c.x; slot[kBlock] = c.y; slot[2 * kBlock] = c.z; slot[3 * kBlock] = c.w;
                }
            }
        }
    }
    int ring_pos = 0;   // (Sn::kOn only) k mod d
    bool any_reset = false;
    float stash[reset_value_count<V>()];   // the lane's own next reset draws (reset_from_stash)
    bool stash_ok = false;
    [[maybe_unused]] typename Rec::template State<V> rs;
    if constexpr (Rec::kOn)   // the record tile: kBlock rows behind the command queue
        rs.begin(rc, reinterpret_cast<float*>(laps - threadIdx.x + 2 * QR_EVAL_MAX_LAPS * kBlock) + kSensingQueueFloats * kBlock, rid, lane);
    float o[L];
    observe<V, GA>(P, gates, e, o);
    if constexpr (H > 0) {   // h_0 = the caller's queue, entries 0 .. H - 1 (whatever d is)
        const float4* pend = reinterpret_cast<const float4*>(Sn::pending(sen)) + (size_t)ii * kMaxDelay;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float4 c = pend[j];
            o[LE + 4 * j] = c.x; o[LE + 4 * j + 1] = c.y; o[LE + 4 * j + 2] = c.z; o[LE + 4 * j + 3] = c.w;
        }
    }
    for (int k = 0; k < K; ++k) {
        if constexpr (Sn::kOn) Sn::template perturb<V, GA>(sen, gid_lo, gid_hi, k, o);   // o is rebuilt from the state behind the step
        float mean[4];
        if constexpr (Rec::kOn) {   // the rows of step k - 1 leave and the state of step k enters the tile under the third layer
            rs.flush_lanes();
            auto rec_slice = [&](int s) { rs.slice(s, e.s); };
            if constexpr (kF32) {
                rec_slice(0);
                rec_slice(2);
                policy_forward_f32class<L>(W, img_lo, lane, o, mean);
            } else {
                policy_forward<L>(W, lane, o, mean, NoFiller(), rec_slice);
            }
            rs.advance();
        } else if constexpr (kF32) {
            policy_forward_f32class<L>(W, img_lo, lane, o, mean);
        } else {
            policy_forward<L>(W, lane, o, mean);
        }
        float u[4];
        clip_action(mean, u);
        [[maybe_unused]] float uc[4];   // (H > 0 only) the command COMPUTED in this step: what enters the history, whatever flies
        if constexpr (H > 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) uc[c] = u[c];
        }
        if constexpr (Sn::kOn) {   // the env flies the command computed d steps ago; this step's command takes its ring slot
            const int d = Sn::delay(sen);
            if (d > 0) {
                float* slot = reinterpret_cast<float*>(laps + 2 * QR_EVAL_MAX_LAPS * kBlock) + ring_pos * 4 * kBlock;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float old = slot[c * kBlock];
                    slot[c * kBlock] = u[c];
                    u[c] = old;
                }
                ring_pos = ring_pos + 1 == d ? 0 : ring_pos + 1;
            }
        }
        const int target_before = e.target;
        [[maybe_unused]] const int steps_before = e.steps;
        bool done, trunc, did_reset;
        const float reward = step_env<V, 0, C>(P, gates, rtab, nullptr, mlp, lane, active, e, u, gid_lo, gid_hi, done, trunc, did_reset,
                                               [&](bool d) {
                                                   if constexpr (Rec::kOn) rs.on_end(d, trunc, e.s);
                                               },
                                               [&](bool need) { reset_from_stash<V>(P, rtab, need, e, gid_lo, gid_hi, stash, stash_ok); }, dyn);
        any_reset |= did_reset;
        if constexpr (Rec::kOn) rs.row_tail(u, reward, done, trunc, target_before, steps_before);
        // ---- accounting (tests/eval_spec.py, same order).  A pass on the step that ends the episode is not counted: the reset has
        // replaced the target, and that episode's lap count is void anyway.
        now += 1;
        const bool pass = !done && e.target != target_before;
        if (pass) {
            n_gates += 1;
            since += 1;
            in_lap += 1;
            if (in_lap == gates_per_lap) {   // a lap boundary: rare and divergent, so a branch (skipped by the whole wave most steps)
                in_lap = 0;
                lap_no += 1;
                if (lap_no <= QR_EVAL_MAX_LAPS) {
                    laps[(lap_no - 1) * kBlock] += now - lap_t0;
                    laps[(QR_EVAL_MAX_LAPS + lap_no - 1) * kBlock] += 1;
                }
                lap_t0 = now;
            }
        }
        ep_ret = add_rn(ep_ret, reward);
        if (done) {
            if (trunc) n_limit += 1; else n_crash += 1;
            since = 0; in_lap = 0; lap_no = 0;
            lap_t0 = now;
            ret_sum = add_rn(ret_sum, ep_ret);
            ret_sq = add_rn(ret_sq, mul_rn(ep_ret, ep_ret));
            ep_ret = 0.0f;
            if constexpr (Sn::kOn) {   // the step that ends an episode clears the queue: the next d steps fly (0, 0, 0, 0)
                if (Sn::delay(sen) > 0) {
                    float* ring = reinterpret_cast<float*>(laps + 2 * QR_EVAL_MAX_LAPS * kBlock);
#pragma unroll
                    for (int q = 0; q < kSensingQueueFloats; ++q) ring[q * kBlock] = 0.0f;
                }
            }
        }
        observe<V, GA>(P, gates, e, o);
        if constexpr (H > 0) {   // h_{k+1}: the tail moves on by one command, this step's enters in front; an episode end clears it
#pragma unroll
            for (int j = 4 * H - 1; j >= 4; --j) o[LE + j] = done ? 0.0f : o[LE + j - 4];
#pragma unroll
            for (int c = 0; c < 4; ++c) o[LE + c] = done ? 0.0f : uc[c];
        }
    }
    if constexpr (Rec::kOn) rs.finish();   // the rows of the last step
    if (!active) return;
    if constexpr (Rec::kOn) rs.store_status();
    int4* row = rec + (size_t)i * 6;
    int lap_sum[QR_EVAL_MAX_LAPS], lap_cnt[QR_EVAL_MAX_LAPS];
#pragma unroll
    for (int q = 0; q < QR_EVAL_MAX_LAPS; ++q) {
        lap_sum[q] = laps[q * kBlock];
        lap_cnt[q] = laps[(QR_EVAL_MAX_LAPS + q) * kBlock];
    }
    row[0] = make_int4(n_gates, n_crash, n_limit, since);
    row[1] = make_int4(lap_t0, now, lap_sum[0], lap_sum[1]);
    row[2] = make_int4(lap_sum[2], lap_sum[3], lap_sum[4], lap_sum[5]);
    row[3] = make_int4(lap_sum[6], lap_sum[7], lap_cnt[0], lap_cnt[1]);
    row[4] = make_int4(lap_cnt[2], lap_cnt[3], lap_cnt[4], lap_cnt[5]);
    row[5] = make_int4(lap_cnt[6], lap_cnt[7], 0, 0);
    if (recf) recf[i] = make_float4(ep_ret, ret_sum, ret_sq, 0.0f);
    if constexpr (Sn::kOn) {   // the queue in canonical order: entry j = slot (K - 1 - j) mod d for j < d, zeros behind
        const int d = Sn::delay(sen);
        const float* ring = reinterpret_cast<const float*>(laps + 2 * QR_EVAL_MAX_LAPS * kBlock);
        float4* pend = reinterpret_cast<float4*>(Sn::pending(sen)) + (size_t)i * kMaxDelay;
#pragma unroll
        for (int j = 0; j < kMaxDelay; ++j) {
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (j < d) {
                int p = ring_pos - 1 - j;
                p += p < 0 ? d : 0;
                const float* slot = ring + p * 4 * kBlock;
                c = make_float4(slot[0], slot[kBlock], slot[2 * kBlock], slot[3 * kBlock]);
            }
            if constexpr (H > 0) {   // max(d, H) entries: the tail holds entries 0 .. H - 1 (equal to the ring's where both hold one)
                if (j < H) c = make_float4(o[LE + 4 * j], o[LE + 4 * j + 1], o[LE + 4 * j + 2], o[LE + 4 * j + 3]);
            }
            pend[j] = c;
        }
    }
    define_exit_values<V>(e);
    P.ts[i] = pack_ts<V>(e);
    store_world<V>(P, i, e);
    if (any_reset) store_dist<V>(P, i, e);
}

}  // namespace qr
