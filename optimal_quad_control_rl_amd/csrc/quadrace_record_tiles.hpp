// quadrace_record_tiles.hpp -- the wave-private LDS tile through which the flight recorder (quadrace_record.hip) and the black box
// (quadrace_blackbox.hip) assemble their packed rows [R = S + QR_RECORD_EXTRA floats per env and step] and stream them out; the write
// shape and its LDS traffic are described at the top of quadrace_record.hip.  Included by those two units and by the black box of the
// sensing-grid evaluator (quadrace_blackbox_grid.hip), and by nothing else.
#pragma once
#include "quadrace_env_kernels.hpp"

namespace qr {

// columns [C0, C0 + NV) of this lane's tile row
template <int R, int C0, int NV>
__device__ __forceinline__ void rec_tile_write(float* __restrict__ row, const float (&v)[NV]) {
    if constexpr (R % 4 == 0 && C0 % 4 == 0 && NV % 4 == 0) {
        float4* r4 = reinterpret_cast<float4*>(row + C0);
#pragma unroll
        for (int q = 0; q < NV / 4; ++q) r4[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else {
#pragma unroll
        for (int q = 0; q < NV; ++q) row[C0 + q] = v[q];   // odd row stride: conflict-free ds_write_b32
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the wave's 64 finished rows -> block[0 .. 64 R): every round with the whole wave (see obs_tile_flush on why the last, partial round
// clamps its index instead of masking lanes off)
template <int R>
__device__ __forceinline__ void rec_tile_flush(const float* __restrict__ tile, float* __restrict__ block, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    constexpr int kVec = 16 * R;
    const float4* t4 = reinterpret_cast<const float4*>(tile);
    float4* g4 = reinterpret_cast<float4*>(block);
#pragma unroll
    for (int t = 0; t < (kVec + 63) / 64; ++t) {
        const int e = t * 64 + lane;
        const int ec = (t + 1) * 64 <= kVec || e < kVec ? e : kVec - 1;
        stream_store(g4 + ec, t4[ec]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// one lane's own row (ragged tail wave, a wave cut by rec_envs, a block that is not 16-byte aligned): tile row -> dst[0 .. R)
template <int R>
__device__ __forceinline__ void rec_row_flush(const float* __restrict__ row, float* __restrict__ dst) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if constexpr (R % 4 == 0) {   // rows of 96 bytes in a 16-byte aligned buffer
#pragma unroll
        for (int q = 0; q < R / 4; ++q) stream_store(reinterpret_cast<float4*>(dst) + q, reinterpret_cast<const float4*>(row)[q]);
    } else {
#pragma unroll
        for (int q = 0; q < R; ++q) stream_store(dst + q, row[q]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

}  // namespace qr
