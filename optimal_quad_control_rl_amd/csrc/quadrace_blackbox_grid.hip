// quadrace_blackbox_grid.hip -- the BLACK BOX AND FLIGHT RECORDER OF THE SENSING-GRID EVALUATOR (qr_blackbox_policy_grid): the launch of
// eval_policy_history_grid_kernel (quadrace_eval_history.hip; H = 0: of eval_policy_sensing_grid_kernel, quadrace_eval_sensing.hip) --
// per group a policy slot, a condition, a vehicle and a sensor, the optional command history, the group-local reset and noise streams,
// action = clip(mean) -- with the black box of quadrace_blackbox.hip riding in the step loop, so that the crash log of a cell belongs to
// the numbers the evaluator prints for that cell.  The step loop, the accounting, the records, the command queue and the history are
// eval_policy_body's (quadrace_eval_body.hpp): this unit instantiates it with a RECORDING CLASS, the one more defaulted template
// parameter of that body; every statement the class adds sits under `if constexpr`, and the evaluators' code objects do not change.
// rec, recf, pending and the env state after the call are bit for bit the evaluator twin's, whatever the black-box arguments are.
//
// What the recording class carries is blackbox_policy_kernel's, statement for statement: ring slot (first_step + k) mod W, armed / frozen,
// the scalar flush path decided by a ballot (block / per lane / none), the trigger step inside step_env's before_reset hook, the status
// read at the start and written at the end.  What differs:
//   * which envs: the first M = rec_per_group envs of every group; env g E + j, j < M, owns column g M + j of ring [W][G M][R], st [G M][4]
//     and term [G M][S].  Groups are multiples of 256 envs, so a wave's first j is (blockIdx % wgs_per_group) * 256 + 64 * wave and a wave
//     is a block iff that + 64 <= M and the block is 16-byte aligned in every group (R % 4 == 0 or M % 4 == 0).
//   * the row under a sensor: [0, S) the TRUE world state before the step (not the noisy observation), [S, S + 4) the command FLOWN (under
//     a delay d the clipped command computed d steps earlier in the episode, zeros for its first d steps).
//   * no action noise: nothing between the matrix instructions but the tile traffic (f16 operands: the rows of step k - 1 leave in slot 0
//     of step k's third layer, the state of step k enters the tile in slot 2).
// No atomics, no workgroup that waits for another, no load of a slot value in the step loop, no store that is waited for inside it.
// A translation unit of its own with the flags of quadrace_eval_sensing.hip.
#include "quadrace_eval_body.hpp"
#include "quadrace_launch.hpp"
#include "quadrace_record_tiles.hpp"
#include "quadrace_sensing.hpp"

namespace qr {

static_assert(QR_RECORD_EXTRA == 8 && QR_BLACKBOX_ST_INTS == 4, "row and status layout of include/quadrace.h");

// workgroup-uniform: the group, the extents and the three buffers (term may be null); slot0 = first_step mod window (the host's 64-bit remainder)
struct BlackboxGridArgs {
    int grp, num_groups, M, trigger, window, slot0;
    float* ring;
    int4* st;
    float* term;
};

struct BlackboxGridRecording {
    using Arg = const BlackboxGridArgs*;
    static constexpr bool kOn = true;
    enum : int { kFlushNone = 0, kFlushBlock = 1, kFlushLanes = 2 };

    template <int V>
    struct State {
        static constexpr int S = Env<V>::S, R = S + QR_RECORD_EXTRA;
        Arg a;
        int lane;
        float *tile, *trow;
        size_t slot_floats, col, row_off, block_off;
        bool rec_block, rec_env;   // scalar: the wave is one block | this env has a ring column and a status
        int4 status;
        bool armed, was_armed;     // was_armed: armed at the start of the step whose row sits in the tile
        bool live;                 // scalar: some lane of the wave is armed at the start of this step
        bool hit;
        int flush_prev;            // scalar: how the rows of step k - 1 leave
        int slot;                  // scalar: ring slot of step k - 1 (advanced behind the forward)

        // tiles: kBlock rows of R floats; j = the lane's index within its group
        __device__ __forceinline__ void begin(Arg rc, float* tiles, int j, int lane_) {
            a = rc;
            lane = lane_;
            const int M = rc->M;
            const int wave_first = __builtin_amdgcn_readfirstlane(j - lane);
            rec_block = wave_first + 64 <= M && (R % 4 == 0 || (M & 3) == 0);
            rec_env = j < M;
            tile = tiles + (threadIdx.x >> 6) * 64 * R;
            trow = tile + lane * R;
            slot_floats = (size_t)rc->num_groups * M * R;
            col = (size_t)rc->grp * M + (rec_env ? j : 0);   // (a lane without a column never uses it)
            row_off = col * R;
            block_off = ((size_t)rc->grp * M + (rec_block ? wave_first : 0)) * R;
            status = make_int4(1, 0, -1, 0);
            if (rec_env) status = rc->st[col];
            if (status.x == 0) { status.z = -1; status.w = 0; }   // an armed env has no trigger row yet: a zeroed status is a fresh one
            armed = rec_env && status.x == 0;
            was_armed = false;
            live = __ballot(armed) != 0ull;
            hit = false;
            flush_prev = kFlushNone;
            slot = rc->slot0 == 0 ? rc->window - 1 : rc->slot0 - 1;
        }
        // loop top: a lane-masked store block stays outside the forward's schedule (the rows of step k - 1 of a wave without a block)
        __device__ __forceinline__ void flush_lanes() {
            if (flush_prev == kFlushLanes && was_armed) rec_row_flush<R>(trow, a->ring + (size_t)slot * slot_floats + row_off);
        }
        // under the third layer's matrix instructions: slot 0 streams out the block of step k - 1, slot 2 puts the world columns of step k
        // into the tile (LDS operations of one wave execute in order: the flush's reads come first).  Both conditions are scalars.
        __device__ __forceinline__ void slice(int s, const float (&world)[S]) {
            if (s == 0 && flush_prev == kFlushBlock) rec_tile_flush<R>(tile, a->ring + (size_t)slot * slot_floats + block_off, lane);
            if (s == 2 && live) rec_tile_write<R, 0, S>(trow, world);
        }
        __device__ __forceinline__ void advance() { slot = slot + 1 == a->window ? 0 : slot + 1; }   // now the slot of step k
        // the trigger step: `world` is the terminal state (after the integration, before the auto-reset)
        __device__ __forceinline__ void on_end(bool d, bool trunc, const float (&world)[S]) {
            hit = armed && d && ((trunc ? 2 : 1) & a->trigger) != 0;
            if (hit) {
                const bool ground = world[2] > 0.0f;
                const bool oob = (fabsf(world[0]) > 10.0f) || (fabsf(world[1]) > 10.0f) || (fabsf(world[9]) > 1000.0f) ||
                                 (fabsf(world[10]) > 1000.0f) || (fabsf(world[11]) > 1000.0f);
                status.w = (ground ? 1 : 0) | (oob ? 2 : 0) | (trunc ? 4 : 0) | (!trunc && !ground && !oob ? 8 : 0);
                status.z = slot;
                if (a->term != nullptr) {
#pragma unroll
                    for (int q = 0; q < S; ++q) a->term[col * S + q] = world[q];
                }
            }
        }
        // behind the step: the row's tail, and how the wave's rows of this step leave
        __device__ __forceinline__ void row_tail(const float (&u)[4], float reward, bool done, bool trunc, int target_before, int steps_before) {
            if (live) {
                const float tail[8] = {u[0], u[1], u[2], u[3], reward, done ? (trunc ? 2.0f : 1.0f) : 0.0f, (float)target_before, (float)steps_before};
                rec_tile_write<R, S, 8>(trow, tail);
            }
            was_armed = armed;
            status.y += armed ? 1 : 0;
            if (hit) { armed = false; status.x = 1; }
            hit = false;
            const unsigned long long stored = __ballot(was_armed);
            flush_prev = stored == 0ull ? kFlushNone : (rec_block && stored == ~0ull ? kFlushBlock : kFlushLanes);
            live = __ballot(armed) != 0ull;
        }
        __device__ __forceinline__ void finish() {
            if (flush_prev == kFlushBlock) rec_tile_flush<R>(tile, a->ring + (size_t)slot * slot_floats + block_off, lane);
            else if (flush_prev == kFlushLanes && was_armed) rec_row_flush<R>(trow, a->ring + (size_t)slot * slot_floats + row_off);
        }
        __device__ __forceinline__ void store_status() {
            if (rec_env) a->st[col] = status;
        }
    };
};

// dynamic LDS: policy image at obs_len<V, GA + H> | tables | lap sums | command queue | record tile
template <int V, int GA, int H>
constexpr size_t blackbox_grid_lds_bytes() {
    return eval_lds_bytes<obs_len<V, GA + H>()>() + sizeof(float) * kSensingQueueFloats * kBlock + sizeof(float) * kBlock * (Env<V>::S + QR_RECORD_EXTRA);
}
static_assert(blackbox_grid_lds_bytes<kE2E, 0, 4>() == 145280 && blackbox_grid_lds_bytes<kE2E, 4, 0>() == 145280 &&
                  blackbox_grid_lds_bytes<kE2E, 2, 2>() <= 160 * 1024,
              "the largest form (E2E, GA + H = 4, R = 24) must fit the 160 KB of a CU: 84 KB image + 1.9 KB tables + 16 + 16 + 24 KB");

// the arguments of eval_policy_history_grid_kernel (H = 0: eval_policy_sensing_grid_kernel's) and the black box's
template <int V, int GA, int H, bool kF32>
__global__ void __launch_bounds__(kBlock, 1)
blackbox_policy_grid_kernel(Params P0, const half8* __restrict__ bank, const half8* __restrict__ bank_lo, const float* __restrict__ conds,
                            const float* __restrict__ dyns, const float* __restrict__ sens, const int4* __restrict__ map, int wgs_per_group, int K,
                            SensingStream stream, float* __restrict__ pending, int4* __restrict__ rec, float4* __restrict__ recf, int num_groups, int M,
                            int trigger, int window, int slot0, float* __restrict__ ring, int4* __restrict__ st, float* __restrict__ term) {
    using D = PolicyDims<obs_len<V, GA + H>()>;
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
    const BlackboxGridArgs bb = {grp, num_groups, M, trigger, window, slot0, ring, st, term};
    const int i = blockIdx.x * kBlock + threadIdx.x;   // < P.n: the grid is exactly P.n / kBlock workgroups
    eval_policy_body<V, GA, kF32, false, RuntimeDyn<V>, RuntimeSensing, H, BlackboxGridRecording>(
        P, img, img_lo, cond + kCondHeaderFloats, i, local0 + (int)threadIdx.x, K, gates_per_lap, rec, recf, &dyn, &sen, &bb);
}

// history -> f(integral_constant<int, H>), H in [0, 4 - GA]
template <int GA, typename F>
static hipError_t dispatch_history0(int history, F&& f) {
    if (history == 0) return f(std::integral_constant<int, 0>{});
    return dispatch_history<GA>(history, static_cast<F&&>(f));
}

// the arguments of launch_eval_policy_history_grid with `history` in [0, 4 - P.gates_ahead], and the black box's.  The extents are checked
// again here: a grid that does not match P.n, or a column past the buffers, would read and write out of bounds.
hipError_t launch_blackbox_policy_grid(int variant, const Params& P, const half8* bank, const half8* bank_lo, const float* conds, const float* dyns,
                                       const float* sens, const int4* map, int history, bool f32class, int num_groups, int envs_per_group, int K,
                                       uint64_t noise_seed, uint64_t first_step, float* pending, int32_t* rec, float* recf, int trigger, int window,
                                       int rec_per_group, int slot0, float* ring, int32_t* st_rec, float* term, hipStream_t st) {
    if (num_groups < 1 || envs_per_group < kBlock || envs_per_group % kBlock != 0 || (long long)num_groups * envs_per_group != (long long)P.n ||
        !bank || !bank_lo || !conds || !dyns || !sens || !map || !pending || ((uintptr_t)pending & 15) || !rec || K < 1)
        return hipErrorInvalidValue;
    if (rec_per_group < 1 || rec_per_group > envs_per_group || trigger < 0 || trigger > 3 || window < 1 || slot0 < 0 || slot0 >= window || !ring ||
        !st_rec || (((uintptr_t)ring | (uintptr_t)st_rec) & 15))
        return hipErrorInvalidValue;
    const SensingStream stream = sensing_stream(noise_seed, first_step);
    return dispatch_vg(variant, P.gates_ahead, [&](auto v, auto ga) {
        constexpr int V = decltype(v)::value, GA = decltype(ga)::value;
        return dispatch_history0<GA>(history, [&](auto h) {
            constexpr int H = decltype(h)::value;
            constexpr size_t lds = blackbox_grid_lds_bytes<V, GA, H>();
            static_assert(lds <= 160 * 1024, "LDS of a CU");
            int4* rec4 = reinterpret_cast<int4*>(rec);
            float4* recf4 = reinterpret_cast<float4*>(recf);
            int4* st4 = reinterpret_cast<int4*>(st_rec);
            const dim3 grid((unsigned)(P.n / kBlock));
            const int wgs = envs_per_group / kBlock;
            if (f32class)
                return launch_dynamic_lds<blackbox_policy_grid_kernel<V, GA, H, true>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, dyns, sens, map, wgs,
                                                                                       K, stream, pending, rec4, recf4, num_groups, rec_per_group, trigger,
                                                                                       window, slot0, ring, st4, term);
            return launch_dynamic_lds<blackbox_policy_grid_kernel<V, GA, H, false>>(grid, dim3(kBlock), lds, st, P, bank, bank_lo, conds, dyns, sens, map, wgs,
                                                                                    K, stream, pending, rec4, recf4, num_groups, rec_per_group, trigger,
                                                                                    window, slot0, ring, st4, term);
        });
    });
}

}  // namespace qr
