// quadrace_rollout_group.hpp -- the ONE kernel behind the grouped closed-loop rollouts: qr_rollout_policy_conditions
// (quadrace_rollout_cond.hip, kPop = false), qr_rollout_policy_population (quadrace_rollout_population.hip, kPop = true),
// qr_rollout_policy_dynamics (quadrace_rollout_dynamics.hip, kPop = false, kDyn = true) and qr_rollout_policy_sensing
// (quadrace_rollout_sensing.hip, kDyn = true, Sn = RuntimeSensing), and behind qr_rollout_policy_history (quadrace_rollout_history.hip: the
// sensing mode with H > 0) and qr_rollout_policy_privileged (quadrace_rollout_privileged.hip: the sensing / history mode with kPriv = true).
// Included by those six units and by nothing else; each keeps its launch function, its checks and its instantiations.
//
// K x [obs -> MFMA policy -> a = mean + std * eps -> env.step(clip(a))] with the rollout rows, the terminal-observation rows, last_obs
// and the end-of-kernel state write-back of rollout_policy_kernel (quadrace_env_kernels.hpp), and the inputs of eval_policy_grid_kernel
// (quadrace_eval_grid.hip):
//   * group map: the launch carries num_groups groups x E envs, E a multiple of kBlock, N = num_groups E exactly.  Workgroup b belongs
//     to group g = b / (E / kBlock) and reads map[g] = (policy slot, condition slot) from an address that derives from blockIdx alone:
//     a scalar load, and the bases built from it stay in scalar registers, as eval_policy_grid_kernel keeps them.  The host has
//     validated every index it passes against the banks' capacities.
//   * condition image: a slot of the condition bank is [CondHeader | reset table | gate rows] (quadrace_device.hpp).  A kernel-local
//     copy of Params takes num_gates, max_steps, obs_lo and obs_inv from the header (scalar loads: uniform address, memory no store of
//     this kernel touches), and the workgroup stages the slot's table image into its LDS where rollout_policy_kernel stages
//     P.tables + kOffResetImage.  The header's gates_per_lap is not used (a rollout counts no laps).  The residual-MLP table, dt,
//     flags and gates_ahead stay the handle's.
// What the mode decides, in the prologue and nowhere else:
//   kPop = false   one policy per launch: the weight image and its low pieces are A.weights / A.weights_lo, the sampling arguments are
//                  A.std / A.logp_const / A.seed_*; only the condition half of the map entry is read (a 4-byte load); bank, bank_lo and
//                  table are passed as null.
//   kPop = true    both halves of the map entry are read (one 8-byte load): the workgroup stages image map[g].x of the policy bank
//                  (bank + slot * PolicyDims<L>::kTotalHalf8), the f32-class forward reads that slot's low pieces from global memory as
//                  eval_policy_bank_kernel does, and the sampling arguments are table[g], one 32-byte PopulationEntry
//                  (quadrace_launch.hpp) read by one scalar load, which stays in scalar registers where the other mode's kernel
//                  arguments sit.  A's weight pointers and per-launch sampling fields are not read; step_lo / step_hi, deterministic
//                  and f32class stay launch-wide.
//   kDyn = true    (with kPop = false only; qr_rollout_policy_dynamics) the single-policy mode with a VEHICLE per group: both halves of
//                  the map entry are read (one 8-byte load), map[g] = (dynamics slot, condition slot); the workgroup loads its 128-byte
//                  slot of the dynamics bank (dyns + slot * kDynSlotFloats) once, in the prologue, through uniform-address loads and
//                  pins every entry to a scalar register (load_dynamics, quadrace_device.hpp), and the step is
//                  step_env<V, 0, RuntimeDyn<V>> on that set: no load in the step loop, no LDS, no vector register for a coefficient.
//                  A slot that holds the nominal table flies bit for bit what kDyn = false flies (the same fmaf nesting, the sign in
//                  the table).  `dyns` is the LAST parameter: the arguments of the two older modes keep their offsets and neighbours,
//                  and those modes pass it as null.  The residual networks and the observation stay the env's: the vehicle is not
//                  observed.
//   Sn = RuntimeSensing   (with kDyn = true only; qr_rollout_policy_sensing) the vehicle mode with a SENSOR per group (quadrace_sensing.hpp:
//                  the slot, the stream and the device functions are the sensing-grid evaluator's).  The workgroup loads slot
//                  sen_map[grp] of the sensing bank once, in the prologue (load_sensing): sigma and the delay d stay in scalar registers,
//                  no load of a slot value in the step loop.
//                  OBSERVATION NOISE: at call-step k the row o is perturbed in place BEFORE the forward, o~[j] = add_rn(o[j],
//                  mul_rn(sigma[group(j)], eps[j])), so obs_slice stores the NOISY row to obs_out[k] -- the row the action and its
//                  log-prob belong to -- and observe() rebuilds o from the untouched state behind the step.  The Philox counter's env
//                  id is the ORDINARY id gid this kernel already uses (not the evaluator's group-local one: training wants
//                  independent envs), step = first_step + k, the key the sensing tweak of the seed: the action-noise stream (its own
//                  tweak) does not move.  A slot with all sigmas zero draws nothing (workgroup-uniform branch).  last_obs is
//                  perturbed with k = K before it is stored: bit for bit row 0 of the next launch called with first_step + K.
//                  TERMINAL-OBSERVATION ROWS STAY CLEAN, by decision: store_terminal_obs writes the observation of the terminal
//                  state as in every other mode.  These rows feed the time-limit bootstrap only, and a second noise draw on divergent
//                  lanes (a few lanes per thousand steps) is not worth its instructions in every step.
//                  COMMAND DELAY: the env flies the clipped command computed d steps earlier, (0, 0, 0, 0) for the first d steps of an
//                  episode; act_out[k] / logp_out[k] stay this step's unclipped sample and its log-prob, rew_out[k] is the reward of
//                  the step flown.  The queue is eval_policy_body's: a ring of clipped commands in the lane's own LDS column behind
//                  the observation tiles (kSensingQueueFloats * kBlock more floats of dynamic LDS), slot k mod d, cleared by the step
//                  that ends an episode, read from and written back to `pending` [n][16] in canonical order (entry j = the command
//                  computed j + 1 steps ago, zeros behind d), so a buffer passes between the evaluator and this kernel.
//                  sens, sen_map, pending and stream come AFTER dyns: every older mode keeps its argument offsets and passes nulls.
//                  No atomics, no workgroup that waits for another.
//   H > 0          (with Sn = RuntimeSensing only; qr_rollout_policy_history, quadrace_rollout_history.hip) the sensing mode with a COMMAND
//                  HISTORY in the policy's row: at call-step k the row is [o~_k | u_{k-1}, ..., u_{k-H}], L = obs_len<V, GA + H>() = LE + 4 H
//                  floats, u_j the clipped command COMPUTED (not flown) at step j of the current episode, zeros before the episode's start.
//                  The network side (PolicyDims, the forward, the LDS tile, the row stores) is instantiated at L, an observation length every
//                  network kernel already has because GA + H <= 4; the env side (observe, step_env, the sensor's noise) stays at GA and touches
//                  o[0 .. LE) only: the history is exact.  The tail lives in o[LE .. L): loaded from entries 0 .. H - 1 of `pending` in the
//                  prologue, moved on by one command behind each step (cleared by the step that ends an episode, with the ring), stored to
//                  `pending` in the epilogue, which then carries max(d, H) entries.  The delay ring is untouched: d and H are independent.
//                  Terminal rows are L wide, [clean observation | u_k, ..., u_{k-H+1}] (store_terminal_obs_history below): P.term_obs is read
//                  as [rows][N][L] in this mode.
//   kPriv = true   (with Sn = RuntimeSensing only, H >= 0; qr_rollout_policy_privileged, quadrace_rollout_privileged.hip) the sensing / history mode
//                  that ALSO stores the row a privileged critic reads: c_k = [o_k | h_k], the observation BEFORE the sensor's noise (with the
//                  condition's scaling, as observe() forms it) and the same exact history tail, to critic_obs_out[k], rows of L floats.  The
//                  clean row leaves through the wave's observation tile in front of perturb (store_obs_coalesced); the noisy row reuses the
//                  tile behind it (one wave's LDS operations stay in order: no barrier, no new LDS), so the forward and its pinned schedule
//                  see what they see in the other modes.  critic_last_obs_out (may be null) = [o_K | h_K], stored in front of the noise of
//                  call-step K.  Nothing else is computed differently: every other output, `pending` and the env state are those of the
//                  kPriv = false launch.  The two pointers are the LAST parameters; every older mode passes nulls.
// Unlike the grid evaluator the reset stream and the action noise are keyed by the handle's ORDINARY env ids (P.gid + i): training
// wants independent envs, not common random numbers across groups.  Group g therefore computes what an E-env handle with
// env_id_base + g E, configured with the group's condition, computes under qr_rollout_policy with the group's weights, log_std and seed
// (tests/test_gpu_rollout_conditions.py and tests/test_gpu_rollout_population.py demand bit equality).
//
// The step loop RESTATES rollout_policy_kernel's, statement for statement, the way quadrace_record.hip does, instead of sharing a
// body with it: that kernel's matrix-instruction schedule is pinned with sched_barriers and its code object must not move
// (tools/isa_digest.py), so quadrace_env_kernels.hpp is left untouched.  What differs: there are no tail lanes (the host refuses
// anything else), so every lane is an env, every wave is full, and the `active` / `full_wave` tests are gone.  The modes, in
// turn, are one template and not two restatements: a bool mode, real __restrict__ parameters, the mode's prologue under `if constexpr`
// ("A variant of a pinned kernel without a copy").  The parameter list is the population mode's, the three pointers it alone
// reads NOT last: of the two orders this is the one under which more of the 40 instantiations kept their code (DESIGN.md has the count).
#pragma once
#include "quadrace_env_kernels.hpp"
#include "quadrace_launch.hpp"
#include "quadrace_sensing.hpp"

namespace qr {

// store_terminal_obs (quadrace_env_kernels.hpp) for a row with a command history: [clean observation of the terminal state | u_k,
// u_{k-1}, ..., u_{k-H+1}] -- `uc` the command computed in the step that ended the episode, `tail` the history that step's row carried
// (its first 4 (H - 1) floats move back by one command) -- to row [row_base + i] of P.term_obs read as rows of obs_len<V, GA + H>() floats.
template <int V, int GA, int H>
__device__ __forceinline__ void store_terminal_obs_history(const Params& P, const float* __restrict__ gates, const Env<V>& e, size_t row_base, int i,
                                                           bool write, const float* uc, const float* tail) {
    if (P.term_obs == nullptr || !write) return;
    constexpr int LE = obs_len<V, GA>(), L = obs_len<V, GA + H>();
    float to[L];
    observe<V, GA>(P, gates, e, to);
#pragma unroll
    for (int c = 0; c < 4; ++c) to[LE + c] = uc[c];
#pragma unroll
    for (int j = 4; j < 4 * H; ++j) to[LE + j] = tail[j - 4];
    store_obs<V, GA + H>(P.term_obs + row_base * L, i, to);
}

// conds: slot 0 of the condition bank; map[g] = (policy, condition) of group g; wgs_per_group = E / kBlock; kPop: bank / bank_lo = image 0
// of the two policy arrays, table[g] = sampling arguments of group g; kDyn: dyns = slot 0 of the dynamics bank, map[g] = (dynamics, condition);
// Sn::kOn: sens = slot 0 of the sensing bank, sen_map[g] = the sensing slot of group g, pending = the command queues [n][kSensingQueueFloats]
template <int V, int GA, bool kF32, bool kPop, bool kDyn = false, class Sn = IdealSensing, int H = 0, bool kPriv = false>
__global__ void __launch_bounds__(kBlock, 1)
rollout_policy_group_kernel(Params P0, PolicyArgs A, const half8* __restrict__ bank, const half8* __restrict__ bank_lo,
                            const float* __restrict__ conds, const int2* __restrict__ map, const PopulationEntry* __restrict__ table,
                            int wgs_per_group, int K, float* __restrict__ obs_out, float4* __restrict__ act_out,
                            float* __restrict__ logp_out, float* __restrict__ rew_out, uint8_t* __restrict__ done_out,
                            uint8_t* __restrict__ trunc_out, float* __restrict__ last_obs_out, const float* __restrict__ dyns,
                            const float* __restrict__ sens, const int* __restrict__ sen_map, float* __restrict__ pending, SensingStream stream,
                            float* __restrict__ critic_obs_out, float* __restrict__ critic_last_obs_out) {
    static_assert(!(kPop && kDyn), "the vehicle mode is a single-policy mode");
    static_assert(!Sn::kOn || kDyn, "the sensing mode is a mode of the vehicle mode");
    static_assert(H == 0 || (Sn::kOn && H >= 1 && GA + H <= 4), "the command history is a mode of the sensing mode, 1 <= H <= 4 - GA");
    static_assert(!kPriv || Sn::kOn, "the privileged-critic rows are a mode of the sensing mode");
    constexpr int LE = obs_len<V, GA>();       // the env's row: observe, the sensor's noise
    constexpr int L = obs_len<V, GA + H>();    // the policy's row [o~ | h] = LE + 4 H floats: the network, the tiles, the row stores (H = 0: LE)
    using D = PolicyDims<L>;
    using C = std::conditional_t<kDyn, RuntimeDyn<V>, NominalDyn<V>>;   // where the step takes the coefficients of the equations of motion from
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);                                   // policy weights (f16)
    float* rtab = reinterpret_cast<float*>(smem + (size_t)D::kTotalHalf8 * 16);  // reset table | gate rows | obs tiles
    float* gates = rtab + kResetTableFloats;
    // workgroup-uniform (blockIdx only): the group of this workgroup, its map entry, its images, its sampling arguments, and the
    // handle's Params with the condition's scalars
    const int grp = (int)blockIdx.x / wgs_per_group;
    const half8* __restrict__ img;
    const half8* __restrict__ img_lo;
    const float* __restrict__ cond;
    PopulationEntry S;   // std, logp_const, seed_lo, seed_hi of the group
    std::conditional_t<kDyn, RuntimeDyn<V>, int> dyn{};   // kDyn: the group's vehicle, in scalar registers from here on; else a dummy
    if constexpr (kPop) {
        const int2 pc = map[grp];
        img = bank + (size_t)pc.x * D::kTotalHalf8;
        img_lo = bank_lo + (size_t)pc.x * D::kTotalHalf8;
        cond = conds + (size_t)pc.y * kCondSlotFloats;
        S = table[grp];
    } else {
        img = A.weights;
        img_lo = A.weights_lo;
        if constexpr (kDyn) {
            const int2 dc = map[grp];
            cond = conds + (size_t)dc.y * kCondSlotFloats;
            dyn = load_dynamics<V>(dyns + (size_t)dc.x * kDynSlotFloats);
        } else {
            cond = conds + (size_t)map[grp].y * kCondSlotFloats;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) S.std[c] = A.std[c];
        S.logp_const = A.logp_const;
        S.seed_lo = A.seed_lo;
        S.seed_hi = A.seed_hi;
    }
    std::conditional_t<Sn::kOn, SensingRegs, int> sen{};   // Sn::kOn: the group's sensor, sigma and delay in scalar registers; else a dummy
    typename Sn::Arg sen_arg;
    if constexpr (Sn::kOn) {
        load_sensing(sens + (size_t)sen_map[grp] * kSensingSlotFloats, stream, pending, sen);
        sen_arg = &sen;
    } else {
        sen_arg = 0;
    }
    typename C::Arg dyn_arg;   // NominalDyn: a dummy int, nothing travels; RuntimeDyn: the kernel's own set (everything that takes it is inlined)
    if constexpr (kDyn) dyn_arg = &dyn; else dyn_arg = 0;
    const CondHeader* __restrict__ hdr = reinterpret_cast<const CondHeader*>(cond);
    Params P = P0;
    P.num_gates = hdr->num_gates;
    P.max_steps = hdr->max_steps;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        P.obs_lo[c] = hdr->obs_lo[c];
        P.obs_inv[c] = hdr->obs_inv[c];
    }
    const int i = blockIdx.x * kBlock + threadIdx.x;   // < P.n: the grid is exactly P.n / kBlock workgroups
    const int lane = threadIdx.x & 63;
    Env<V> e;
    load_env<V>(P, i, e);
    MlpRegs mlp;
    const bool use_mlp = (V == kE2E) && (P.flags & kFlagResidual);
    if (use_mlp) mlp_load_regs(P.tables, lane, mlp);
    {
        const float4* s4 = reinterpret_cast<const float4*>(img);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int j = threadIdx.x; j < D::kTotalHalf8; j += kBlock) d4[j] = s4[j];
    }
    {   // [reset table | gate rows] of the condition, as stage_tables copies the handle's (counts are multiples of 4)
        const float4* s4 = reinterpret_cast<const float4*>(cond + kCondHeaderFloats);
        float4* d4 = reinterpret_cast<float4*>(rtab);
        const int count4 = (kResetTableFloats + P.num_gates * kGateStride) / 4;
        for (int j = threadIdx.x; j < count4; j += kBlock) d4[j] = s4[j];
    }
    __syncthreads();
    const uint32_t gid_lo = P.gid_lo + (uint32_t)i;   // ordinary ids: reset stream and noise of env i of the handle
    const uint32_t gid_hi = P.gid_hi + (gid_lo < P.gid_lo ? 1u : 0u);
    const size_t n = (size_t)P.n;
    const int wave_first = i - lane;
    float* tile = gates + kMaxGates * kGateStride + (threadIdx.x >> 6) * 64 * L;
    // the command queue (Sn::kOn only), as eval_policy_body keeps it: a ring of d = delay commands in the lane's own LDS column behind the
    // observation tiles.  The command of call-step k sits in ring slot k mod d, the same slot for every lane -- a cleared queue is all
    // zeros, so an episode end moves nothing.  The caller's buffer holds it in canonical order (entry j = the command computed j + 1 steps
    // ago), so slot d - 1 - j <- entry j.  Own column only: no barrier.
    float* ring = gates + kMaxGates * kGateStride + kBlock * L + threadIdx.x;
    if constexpr (Sn::kOn) {
        const int d = Sn::delay(sen_arg);
        if (d > 0) {
            const float4* pend = reinterpret_cast<const float4*>(Sn::pending(sen_arg)) + (size_t)i * kMaxDelay;
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
    float o[L];
    observe<V, GA>(P, gates, e, o);
    if constexpr (H > 0) {   // h_0 = the caller's queue, entries 0 .. H - 1 (whatever d is)
        const float4* pend = reinterpret_cast<const float4*>(Sn::pending(sen_arg)) + (size_t)i * kMaxDelay;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float4 c = pend[j];
            o[LE + 4 * j] = c.x; o[LE + 4 * j + 1] = c.y; o[LE + 4 * j + 2] = c.z; o[LE + 4 * j + 3] = c.w;
        }
    }
    for (int k = 0; k < K; ++k) {
        // (kPriv) the critic's row [o_k | h_k] leaves before the noise exists; the tile is free again when obs_slice writes the noisy row
        if constexpr (kPriv) store_obs_coalesced<V, GA + H>(tile, critic_obs_out + (size_t)k * n * L, (size_t)wave_first, lane, o);
        // the policy's input is the noisy row (and obs_slice stores it); o is rebuilt from the state behind the step
        if constexpr (Sn::kOn) Sn::template perturb<V, GA>(sen_arg, gid_lo, gid_hi, k, o);
        // ---- action noise: rollout_policy_kernel's slices, verbatim (drawn in deterministic mode too and then multiplied out); the
        // Philox key is the group's
        float mean[4];
        float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t pc4[4];
        float bm_u1a, bm_u2a, bm_u1b, bm_u2b, bm_ra, bm_rb, bm_sa, bm_ca, bm_sb, bm_cb;
        auto pin_u = [](uint32_t& x) { asm volatile("" : "+v"(x)); };
        auto pin_f = [](float& x) { asm volatile("" : "+v"(x)); };
        auto noise_slice = [&](int slot) {
            if (slot >= 1 && slot <= 11) { pin_u(pc4[0]); pin_u(pc4[1]); pin_u(pc4[2]); pin_u(pc4[3]); }
            if (slot == 12) pin_f(bm_u1a);
            if (slot == 13) pin_f(bm_u1b);
            if (slot == 14) pin_f(bm_u2a);
            if (slot == 15) pin_f(bm_u2b);
            if (slot == 16) { pin_f(bm_ra); pin_f(bm_rb); pin_f(bm_sa); pin_f(bm_sb); }
            if (slot == 0) {
                const uint32_t s_lo = A.step_lo + (uint32_t)k;
                pc4[0] = gid_lo; pc4[1] = gid_hi; pc4[2] = s_lo; pc4[3] = A.step_hi + (s_lo < A.step_lo ? 1u : 0u);
            } else if (slot <= 10) {
                philox4x32_round(pc4, S.seed_lo, S.seed_hi, slot - 1);
            } else if (slot == 11) {  // Box-Muller: two pairs of normals from four uniforms (u1 in (0,1], u2 in [0,1))
                bm_u1a = (float)((pc4[0] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2a = u01(pc4[1]);
                bm_u1b = (float)((pc4[2] >> 8) + 1u) * 5.9604644775390625e-8f; bm_u2b = u01(pc4[3]);
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
        // The observation row of this step (the policy's input) is stored under the third layer's MFMAs: LDS transpose in slot 0,
        // coalesced block store in slot 2 (every wave is full).
        auto obs_slice = [&](int slot) {
            if (slot == 0) obs_tile_write<V, GA + H>(tile, lane, o);
            if (slot == 2) obs_tile_flush<V, GA + H>(tile, obs_out + (size_t)k * n * L, (size_t)wave_first, lane);
        };
        if constexpr (kF32) {
#pragma unroll
            for (int slot = 0; slot <= 16; ++slot) noise_slice(slot);
            obs_slice(0);
            obs_slice(2);
            policy_forward_f32class<L>(W, img_lo, lane, o, mean);
        } else {
            policy_forward<L>(W, lane, o, mean, noise_slice, obs_slice);
        }
        float a[4] = {mean[0], mean[1], mean[2], mean[3]};
        float logp = S.logp_const;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float en = A.deterministic ? 0.0f : eps[c];   // fmaf(std, 0, mean) = mean, fmaf(-0, 0, logp) = logp
            a[c] = fmaf(S.std[c], en, mean[c]);
            logp = fmaf(-0.5f * en, en, logp);
        }
        // rollout buffer row t: the observation the action was computed from (stored above), the unclipped action, its log-prob
        stream_store(act_out + (size_t)k * n + i, make_float4(a[0], a[1], a[2], a[3]));
        stream_store(logp_out + (size_t)k * n + i, logp);
        float u[4];
        clip_action(a, u);
        [[maybe_unused]] float uc[4];   // (H > 0 only) the command COMPUTED in this step: what enters the history, whatever flies
        if constexpr (H > 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) uc[c] = u[c];
        }
        if constexpr (Sn::kOn) {   // the env flies the command computed d steps ago; this step's command takes its ring slot
            const int d = Sn::delay(sen_arg);
            if (d > 0) {
                float* slot = ring + ring_pos * 4 * kBlock;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float old = slot[c * kBlock];
                    slot[c * kBlock] = u[c];
                    u[c] = old;
                }
                ring_pos = ring_pos + 1 == d ? 0 : ring_pos + 1;
            }
        }
        bool done, trunc, did_reset;
        const float reward = step_env<V, 0, C>(P, gates, rtab, tile, mlp, lane, true, e, u, gid_lo, gid_hi, done, trunc, did_reset,
                                               [&](bool fin) {
                                                   if constexpr (H > 0) store_terminal_obs_history<V, GA, H>(P, gates, e, (size_t)k * n, i, fin, uc, o + LE);
                                                   else store_terminal_obs<V, GA>(P, gates, e, (size_t)k * n, i, fin);
                                               },
                                               [&](bool need) { reset_from_stash<V>(P, rtab, need, e, gid_lo, gid_hi, stash, stash_ok); },
                                               dyn_arg);
        any_reset |= did_reset;
        if constexpr (Sn::kOn) {   // the step that ends an episode clears the queue: the next d steps fly (0, 0, 0, 0)
            if (done && Sn::delay(sen_arg) > 0) {
#pragma unroll
                for (int q = 0; q < kSensingQueueFloats; ++q) ring[q * kBlock] = 0.0f;
            }
        }
        stream_store(rew_out + (size_t)k * n + i, reward);
        stream_store(done_out + (size_t)k * n + i, (uint8_t)(done ? 1 : 0));
        if (trunc_out) stream_store(trunc_out + (size_t)k * n + i, (uint8_t)(trunc ? 1 : 0));
        observe<V, GA>(P, gates, e, o);
        if constexpr (H > 0) {   // h_{k+1}: the tail moves on by one command, this step's enters in front; an episode end clears it
#pragma unroll
            for (int j = 4 * H - 1; j >= 4; --j) o[LE + j] = done ? 0.0f : o[LE + j - 4];
#pragma unroll
            for (int c = 0; c < 4; ++c) o[LE + c] = done ? 0.0f : uc[c];
        }
    }
    if constexpr (kPriv) {   // [o_K | h_K]: row 0 of critic_obs_out of a launch with first_step + K
        if (critic_last_obs_out) store_obs_coalesced<V, GA + H>(tile, critic_last_obs_out, (size_t)wave_first, lane, o);
    }
    if constexpr (Sn::kOn) {
        // last_obs is what the policy sees next: the noise of call-step K, row 0 of a launch with first_step + K
        if (last_obs_out) Sn::template perturb<V, GA>(sen_arg, gid_lo, gid_hi, K, o);
    }
    if (last_obs_out) store_obs_coalesced<V, GA + H>(tile, last_obs_out, (size_t)wave_first, lane, o);
    if constexpr (Sn::kOn) {   // the queue in canonical order: entry j = slot (K - 1 - j) mod d for j < d, zeros behind
        const int d = Sn::delay(sen_arg);
        float4* pend = reinterpret_cast<float4*>(Sn::pending(sen_arg)) + (size_t)i * kMaxDelay;
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
