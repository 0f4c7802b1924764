// quad3d.hip -- the predecessor environments of the reference's "3D quad.ipynb" on gfx950 (include/quad3d.h).
//
//   Quadcopter3DVec (hover, float64)  Q3 cell 6      Quadcopter3DVecGates (float32)  Q3 cell 14      f_func  Q3 cell 2
//
// One lane = one env.  The reference's only state is the row-major `states[N][16]` array, which is also what step_wait
// returns, so HBM holds exactly that array (64 B / 128 B rows; the step kernel moves a block's rows as one contiguous
// slab of coalesced 16-byte accesses and transposes through LDS) plus step / target / episode counters.  Both envs are HBM-bound in
// the limit (about 230 B resp. 420 B per env-step against ~0.6 k resp. ~2 k flops); at 65 536 envs a launch is
// latency-bound like the race env's, which is what q3_step_many (state in registers across K steps) removes.
// Arithmetic follows the lambdified f_func term by term (-ffp-contract=off), in the element type of the reference's
// arrays; actions are float32 in both envs (SB3 hands float32), so constant*action products round in float32.
//
// Resets: Philox4x32-10 keyed (seed, global env id, episode, block) -- the reference draws from NumPy's global
// generator, the distributions are the reference's; Box-Muller with fixed-polynomial log / sin / cos so the CPU oracle
// used by the tests reproduces every draw bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/quad3d.h"
#include "../../include/quadrace.h"
#include "quadrace_device.hpp"
#include "quadrace_launch.hpp"   // the host support (quadrace_host.hpp), launch_dynamic_lds, the policy accessors and checks; quadrace_policy.hpp

namespace {

constexpr int kQ3Block = 256;
constexpr int kQ3MaxGates = 32;

struct Q3Params {
    int n, num_gates, max_steps, pad;
    double dt;
    double pos_thr, vel_thr, ang_thr, rat_thr;
    uint32_t seed_lo, seed_hi;
    uint32_t gid_lo, gid_hi;               // env_id_base
    float start[4];
    float gate[kQ3MaxGates][4];            // x, y, z, yaw (float32, like astype(np.float32))
    float gate_normal[kQ3MaxGates][2];     // cosf / sinf of the float32 yaw
};

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; static constexpr int kPerRow = 4; };
template <> struct Vec16<double> { using type = double2; static constexpr int kPerRow = 8; };

template <typename T>
__device__ __forceinline__ void load_row(const T* __restrict__ base, size_t i, T s[16]) {
    using V = typename Vec16<T>::type;
    const V* p = reinterpret_cast<const V*>(base + 16 * i);
    V v[Vec16<T>::kPerRow];
#pragma unroll
    for (int k = 0; k < Vec16<T>::kPerRow; ++k) v[k] = p[k];
    memcpy(s, v, sizeof(v));
}
template <typename T>
__device__ __forceinline__ void store_row(T* __restrict__ base, size_t i, const T s[16]) {
    using V = typename Vec16<T>::type;
    V* p = reinterpret_cast<V*>(base + 16 * i);
    V v[Vec16<T>::kPerRow];
    memcpy(v, s, sizeof(v));
#pragma unroll
    for (int k = 0; k < Vec16<T>::kPerRow; ++k) p[k] = v[k];
}

__device__ __forceinline__ void trig(float x, float& s, float& c) { s = sinf(x); c = cosf(x); }
__device__ __forceinline__ void trig(double x, double& s, double& c) { s = sin(x); c = cos(x); }
__device__ __forceinline__ float tangent(float x) { return tanf(x); }
__device__ __forceinline__ double tangent(double x) { return tan(x); }
// constant * float32 action, rounded in float32 (NumPy: python float times float32 array), then widened to T
template <typename T>
__device__ __forceinline__ T ua(double c, float u) { return (T)((float)c * u); }

// f_func of Q3 cell 2 (w_max = 12000: W = 4500 w + 7500; moments on the world velocities v_y, v_x)
template <typename T>
__device__ __forceinline__ void f_q3(const T* s, const float* u, T* ds) {
    const T vx = s[3], vy = s[4], vz = s[5], p = s[9], q = s[10], r = s[11];
    const T w1 = s[12], w2 = s[13], w3 = s[14], w4 = s[15];
    T sph, cph, sth, cth, sps, cps;
    trig(s[6], sph, cph);
    trig(s[7], sth, cth);
    trig(s[8], sps, cps);
    const T tth = tangent(s[7]);
    const T r01 = sph * sth * cps - sps * cph, r11 = sph * sps * sth + cph * cps;
    const T r02 = sph * sps + sth * cph * cps, r12 = -sph * cps + sps * sth * cph;
    const T S = (T)4500 * w1 + (T)4500 * w2 + (T)4500 * w3 + (T)4500 * w4 + (T)30000;
    const T W1 = (T)4500 * w1 + (T)7500, W2 = (T)4500 * w2 + (T)7500;
    const T W3 = (T)4500 * w3 + (T)7500, W4 = (T)4500 * w4 + (T)7500;
    const T W1s = W1 * W1, W2s = W2 * W2, W3s = W3 * W3, W4s = W4 * W4;
    const T kx = (T)1.07933887e-5, ky = (T)9.65250793e-6, kz = (T)2.7862899e-5;
    const T kw = (T)4.36301076e-8, kh = (T)0.0625501332;
    const T vby = vx * r01 + vy * r11 + vz * sph * cth;
    const T vbx = vx * cps * cth + vy * sps * cth - vz * sth;
    const T Tt = -kw * W1s - kw * W2s - kw * W3s - kw * W4s - (kz * vx * r02 + kz * vy * r12 + kz * vz * cph * cth) * S -
                 kh * (vby * vby) - kh * (vbx * vbx);
    const T Fy = -ky * vx * r01 - ky * vy * r11 - ky * vz * sph * cth;  // times S below, in source order
    const T Fx = -kx * vx * cps * cth - kx * vy * sps * cth + kx * vz * sth;
    ds[0] = vx;
    ds[1] = vy;
    ds[2] = vz;
    ds[3] = r02 * Tt + r01 * Fy * S + Fx * S * cps * cth;
    ds[4] = r12 * Tt + r11 * Fy * S + Fx * S * sps * cth;
    ds[5] = Fy * S * sph * cth - Fx * S * sth + Tt * cph * cth + (T)9.81;
    ds[6] = p + q * sph * tth + r * cph * tth;
    ds[7] = q * cph - r * sph;
    ds[8] = q * sph / cth + r * cph / cth;
    ds[9] = (T)-0.896247240618101 * q * r - (T)8.79803364238411 * vy + (T)1.55842505518764e-6 * W1s -
            (T)1.55842505518764e-6 * W2s - (T)1.55842505518764e-6 * W3s + (T)1.55842505518764e-6 * W4s;
    ds[10] = (T)0.924315619967794 * p * r + (T)10.4077084541063 * vx + (T)9.79081191626409e-7 * W1s +
             (T)9.79081191626409e-7 * W2s - (T)9.79081191626409e-7 * W3s - (T)9.79081191626409e-7 * W4s;
    ds[11] = (T)-0.163583252190847 * p * q - (T)0.395780237098345 * r - ua<T>(15.0045045277507, u[0]) +
             ua<T>(15.0045045277507, u[1]) - ua<T>(15.0045045277507, u[2]) + ua<T>(15.0045045277507, u[3]) +
             (T)9.37324867332035 * w1 - (T)9.37324867332035 * w2 + (T)9.37324867332035 * w3 - (T)9.37324867332035 * w4;
    ds[12] = ua<T>(16.6666666666667, u[0]) - (T)16.6666666666667 * w1;
    ds[13] = ua<T>(16.6666666666667, u[1]) - (T)16.6666666666667 * w2;
    ds[14] = ua<T>(16.6666666666667, u[2]) - (T)16.6666666666667 * w3;
    ds[15] = ua<T>(16.6666666666667, u[3]) - (T)16.6666666666667 * w4;
}

// ---- reset RNG (this build's specification; the tests restate it on the CPU) -------------------------------------------------
__device__ __forceinline__ void q3_block(const Q3Params& P, int i, uint32_t episode, int block, uint32_t o[4]) {
    const uint32_t lo = P.gid_lo + (uint32_t)i;
    const uint32_t hi = P.gid_hi + (lo < P.gid_lo ? 1u : 0u);
    qr::philox4x32_10(lo, hi, episode, (uint32_t)block, P.seed_lo, P.seed_hi, o);
}

__device__ __forceinline__ float q3_log(float x) {  // x in (0, 1]; Cephes logf scheme, float32 operations only
    uint32_t b = __float_as_uint(x);
    int e = (int)(b >> 23) - 126;
    float m = __uint_as_float((b & 0x007fffffu) | 0x3f000000u);
    if (m < 0.707106781186547524f) {
        e -= 1;
        m = m + m - 1.0f;
    } else {
        m = m - 1.0f;
    }
    const float z = m * m;
    float y = 7.0376836292e-2f;
    y = y * m + -1.1514610310e-1f;
    y = y * m + 1.1676998740e-1f;
    y = y * m + -1.2420140846e-1f;
    y = y * m + 1.4249322787e-1f;
    y = y * m + -1.6668057665e-1f;
    y = y * m + 2.0000714765e-1f;
    y = y * m + -2.4999993993e-1f;
    y = y * m + 3.3333331174e-1f;
    y = y * m * z;
    const float fe = (float)e;
    y = y + -2.12194440e-4f * fe;
    y = y + -0.5f * z;
    float r = m + y;
    r = r + 0.693359375f * fe;
    return r;
}

__device__ __forceinline__ void q3_normal_pair(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;
    const float t = (float)(b >> 8) * 2.384185791015625e-7f;
    const int quad = (int)t;
    const float x = (t - (float)quad - 0.5f) * 1.5707963267948966f;
    const float z = x * x;
    float sp = -1.9515295891e-4f;
    sp = sp * z + 8.3321608736e-3f;
    sp = sp * z + -1.6666654611e-1f;
    const float sn = x + x * z * sp;
    float cp = 2.443315711809948e-5f;
    cp = cp * z + -1.388731625493765e-3f;
    cp = cp * z + 4.166664568298827e-2f;
    const float cs = 1.0f - 0.5f * z + z * z * cp;
    const float rad = sqrtf(-2.0f * q3_log(u1));
    const float c = quad == 0 ? cs : (quad == 1 ? -sn : (quad == 2 ? -cs : sn));
    const float s = quad == 0 ? sn : (quad == 1 ? cs : (quad == 2 ? -sn : -cs));
    z0 = rad * c;
    z1 = rad * s;
}

template <typename T>
struct Q3Env {
    T s[16];
    int target, steps;
    uint32_t episode;
};

// reset_ of Q3 cell 6: x,y,z U(-5,5); v, phi, theta U(-1,1); psi U(-pi,pi); rates, w U(-1,1)
__device__ __forceinline__ void q3_reset_env(const Q3Params& P, int i, Q3Env<double>& e) {
    const uint32_t ep = e.episode;
    e.episode = ep + 1u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t o[4];
        q3_block(P, i, ep, b, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = 4 * b + k;
            const double u = (double)o[k] * 2.3283064365386963e-10;
            const double hi = j < 3 ? 5.0 : (j == 8 ? 3.141592653589793 : 1.0);
            e.s[j] = -hi + (hi - -hi) * u;
        }
    }
    e.steps = 0;
}

// reset_ of Q3 cell 14: random segment midpoint + 0.1 N(0,1); v 0.1 N; angles N; rates 0.1 N; w U(-1,1); target = segment
__device__ __forceinline__ void q3_reset_env(const Q3Params& P, int i, Q3Env<float>& e) {
    const uint32_t ep = e.episode;
    e.episode = ep + 1u;
    float nrm[12];
    uint32_t o[4];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        q3_block(P, i, ep, b, o);
        q3_normal_pair(o[0], o[1], nrm[4 * b + 0], nrm[4 * b + 1]);
        q3_normal_pair(o[2], o[3], nrm[4 * b + 2], nrm[4 * b + 3]);
    }
    q3_block(P, i, ep, 3, o);
#pragma unroll
    for (int k = 0; k < 4; ++k) e.s[12 + k] = -1.0f + 2.0f * ((float)(o[k] >> 8) * 5.9604644775390625e-8f);
    q3_block(P, i, ep, 4, o);
    const int seg = (int)__umulhi(o[0], (uint32_t)P.num_gates);
    const float* p0 = seg == 0 ? P.start : P.gate[seg - 1];
    const float* p1 = P.gate[seg];
#pragma unroll
    for (int k = 0; k < 3; ++k) e.s[k] = 0.1f * nrm[k] + (p0[k] + p1[k]) / 2.0f;
#pragma unroll
    for (int k = 3; k < 6; ++k) e.s[k] = 0.1f * nrm[k];
#pragma unroll
    for (int k = 6; k < 9; ++k) e.s[k] = nrm[k];
#pragma unroll
    for (int k = 9; k < 12; ++k) e.s[k] = 0.1f * nrm[k];
    e.steps = 0;
    e.target = seg;
}

// before_reset(): called for an env whose step ended, with e.s = the state after the integration, before q3_reset_env replaces it
// (the terminal observation of the closed-loop kernel); the other kernels pass nothing
// (taken BY VALUE: as a forwarding reference the empty default perturbed operand order and copy placement in q3_step_kernel and
// q3_rollout_kernel; by value they compile to the instructions they had without the hook -- tools/isa_digest.py)
struct Q3NoHook {
    __device__ __forceinline__ void operator()() const {}
};

// Quadcopter3DVec.step_wait (Q3 cell 6)
template <class BeforeReset = Q3NoHook>
__device__ __forceinline__ double q3_step_env(const Q3Params& P, int i, Q3Env<double>& e, const float u[4], bool& done,
                                              bool& trunc, BeforeReset before_reset = BeforeReset()) {
    double ds[16];
    e.steps += 1;
    f_q3<double>(e.s, u, ds);
#pragma unroll
    for (int k = 0; k < 16; ++k) e.s[k] = e.s[k] + P.dt * ds[k];
    const double* s = e.s;
    const double npos = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const double nvel = sqrt(s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
    const double nang = sqrt(s[6] * s[6] + s[7] * s[7] + s[8] * s[8]);
    const double nrat = sqrt(s[9] * s[9] + s[10] * s[10] + s[11] * s[11]);
    double reward = -0.002 * npos + -0.002 * nvel + -0.0001 * nang + -0.0001 * nrat;
    const bool ang_ok = fabs(s[6]) < P.ang_thr && fabs(s[7]) < P.ang_thr && fabs(s[8]) < P.ang_thr;
    const bool rat_ok = fabs(s[9]) < P.rat_thr && fabs(s[10]) < P.rat_thr && fabs(s[11]) < P.rat_thr;
    const bool goal = npos < P.pos_thr && nvel < P.vel_thr && ang_ok && rat_ok;
    if (goal) reward = 100.0;
    const bool oob = fabs(s[0]) > 10.0 || fabs(s[1]) > 10.0 || fabs(s[2]) > 10.0 || fabs(s[6]) > 3.141592653589793 ||
                     fabs(s[7]) > 3.141592653589793;
    if (oob) reward = -1.0;
    const bool max_steps = e.steps >= P.max_steps;
    done = goal || oob || max_steps;
    trunc = max_steps || oob;
    if (done) {
        before_reset();
        q3_reset_env(P, i, e);
    }
    return reward;
}

// Quadcopter3DVecGates.step_wait (Q3 cell 14)
template <class BeforeReset = Q3NoHook>
__device__ __forceinline__ float q3_step_env(const Q3Params& P, int i, Q3Env<float>& e, const float u[4], bool& done,
                                             bool& trunc, BeforeReset before_reset = BeforeReset()) {
    float ds[16], ns[16];
    const float dt = (float)P.dt;
    const float* s = e.s;
    e.steps += 1;
    f_q3<float>(s, u, ds);
#pragma unroll
    for (int k = 0; k < 16; ++k) ns[k] = s[k] + dt * ds[k];
    const int g = min(max(e.target, 0), P.num_gates - 1);  // (an out-of-range target_gates raises IndexError upstream)
    const float gx = P.gate[g][0], gy = P.gate[g][1], gz = P.gate[g][2];
    const float ox = s[0] - gx, oy = s[1] - gy, oz = s[2] - gz;
    const float nx = ns[0] - gx, ny = ns[1] - gy, nz = ns[2] - gz;
    const float d2g_old = sqrtf(ox * ox + oy * oy + oz * oz);
    const float d2g_new = sqrtf(nx * nx + ny * ny + nz * nz);
    const float rat_penalty = 0.0001f * sqrtf(ns[9] * ns[9] + ns[10] * ns[10] + ns[11] * ns[11]);
    float reward = d2g_old - d2g_new - rat_penalty;
    const float n0 = P.gate_normal[g][0], n1 = P.gate_normal[g][1];
    const float proj_old = ox * n0 + oy * n1, proj_new = nx * n0 + ny * n1;
    const bool crossed = proj_old < 0.0f && proj_new > 0.0f;
    const bool inside = fabsf(nx) < 0.5f && fabsf(ny) < 0.5f && fabsf(nz) < 0.5f;
    const bool outside = fabsf(nx) > 0.5f || fabsf(ny) > 0.5f || fabsf(nz) > 0.5f;
    const bool gate_passed = crossed && inside, gate_collision = crossed && outside;
    if (gate_collision) reward = -10.0f;
    const bool ground = s[2] > 0.0f;  // the reference tests the PRE-step state here ...
    if (ground) reward = -10.0f;
    const bool oob = fabsf(s[0]) > 10.0f || fabsf(s[1]) > 10.0f || fabsf(s[9]) > 1000.0f || fabsf(s[10]) > 1000.0f ||
                     fabsf(s[11]) > 1000.0f;  // ... and here (no reward override)
    const bool max_steps = e.steps >= P.max_steps;
    if (gate_passed) e.target += 1;
    const bool final_passed = e.target >= P.num_gates;
    if (final_passed) reward = 10.0f;
    done = max_steps || gate_collision || ground || final_passed || oob;
    trunc = max_steps;
#pragma unroll
    for (int k = 0; k < 16; ++k) e.s[k] = ns[k];
    if (done) {
        before_reset();
        q3_reset_env(P, i, e);
    }
    return reward;
}

template <typename T>
struct Q3Buffers {
    T* states;          // [N][16]
    int32_t* target;    // [N]
    int32_t* steps;     // [N]
    uint32_t* episode;  // [N]
};

template <typename T>
__device__ __forceinline__ void q3_load(const Q3Buffers<T>& B, int i, Q3Env<T>& e) {
    load_row<T>(B.states, i, e.s);
    e.target = B.target[i];
    e.steps = B.steps[i];
    e.episode = B.episode[i];
}
template <typename T>
__device__ __forceinline__ void q3_store(const Q3Buffers<T>& B, int i, const Q3Env<T>& e) {
    store_row<T>(B.states, i, e.s);
    B.target[i] = e.target;
    B.steps[i] = e.steps;
    B.episode[i] = e.episode;
}

// Block-cooperative row I/O for the per-step kernel: the block's 256 rows are one contiguous slab (16 / 32 KB); it is moved
// with fully coalesced 16-byte accesses (consecutive lanes -> consecutive addresses) and transposed to lane = row through
// LDS (row stride padded by 16 bytes against bank conflicts).  Measured at 1 Mi envs against per-lane row accesses: see
// DESIGN.md section 10.
template <typename T>
struct RowTile {
    using V = typename Vec16<T>::type;
    static constexpr int kCh = Vec16<T>::kPerRow;      // 16-byte chunks per row
    static constexpr int kStride = kCh + 1;            // LDS row stride in chunks (padded)
    static constexpr int kLdsChunks = kQ3Block * kStride;
};

template <typename T>
__device__ __forceinline__ void tile_load_rows(const T* __restrict__ base, int row0, int rows, typename RowTile<T>::V* lds, T s[16]) {
    using R = RowTile<T>;
    using V = typename R::V;
    const V* src = reinterpret_cast<const V*>(base + (size_t)16 * row0);
#pragma unroll
    for (int q = 0; q < R::kCh; ++q) {
        const int cidx = q * kQ3Block + threadIdx.x;   // chunk index within the slab
        if (cidx < rows * R::kCh) lds[(cidx / R::kCh) * R::kStride + (cidx % R::kCh)] = src[cidx];
    }
    __syncthreads();
    V v[R::kCh];
#pragma unroll
    for (int k = 0; k < R::kCh; ++k) v[k] = lds[threadIdx.x * R::kStride + k];
    memcpy(s, v, sizeof(v));
}

// writes the block's rows to up to two destinations (the state array and the caller's states_out)
template <typename T>
__device__ __forceinline__ void tile_store_rows(T* __restrict__ dst0, T* __restrict__ dst1, int row0, int rows,
                                                typename RowTile<T>::V* lds, const T s[16]) {
    using R = RowTile<T>;
    using V = typename R::V;
    V v[R::kCh];
    memcpy(v, s, sizeof(v));
#pragma unroll
    for (int k = 0; k < R::kCh; ++k) lds[threadIdx.x * R::kStride + k] = v[k];
    __syncthreads();
    V* d0 = reinterpret_cast<V*>(dst0 + (size_t)16 * row0);
    V* d1 = dst1 ? reinterpret_cast<V*>(dst1 + (size_t)16 * row0) : nullptr;
#pragma unroll
    for (int q = 0; q < R::kCh; ++q) {
        const int cidx = q * kQ3Block + threadIdx.x;
        if (cidx < rows * R::kCh) {
            const V x = lds[(cidx / R::kCh) * R::kStride + (cidx % R::kCh)];
            d0[cidx] = x;
            if (d1) d1[cidx] = x;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kQ3Block) void q3_step_kernel(Q3Params P, Q3Buffers<T> B, const float4* __restrict__ actions,
                                                           T* __restrict__ states_out, T* __restrict__ rew_out,
                                                           uint8_t* __restrict__ done_out,
                                                           uint8_t* __restrict__ trunc_out) {
    __shared__ typename RowTile<T>::V lds[RowTile<T>::kLdsChunks];
    const int row0 = blockIdx.x * kQ3Block;
    const int rows = min(kQ3Block, P.n - row0);
    const int i = row0 + threadIdx.x;
    const bool active = i < P.n;
    const int ii = active ? i : row0;  // ragged-tail lanes shadow the block's first env (they take part in the barriers)
    Q3Env<T> e;
    tile_load_rows<T>(B.states, row0, rows, lds, e.s);
    if (!active) load_row<T>(B.states, ii, e.s);
    e.target = B.target[ii];
    e.steps = B.steps[ii];
    e.episode = B.episode[ii];
    const float4 a = actions[ii];
    const float u[4] = {a.x, a.y, a.z, a.w};
    bool done, trunc;
    const T reward = q3_step_env(P, ii, e, u, done, trunc);
    tile_store_rows<T>(B.states, states_out, row0, rows, lds, e.s);
    if (!active) return;
    B.target[i] = e.target;
    B.steps[i] = e.steps;
    B.episode[i] = e.episode;
    if (rew_out) rew_out[i] = reward;
    if (done_out) done_out[i] = done ? 1 : 0;
    if (trunc_out) trunc_out[i] = trunc ? 1 : 0;
}

// a wave's 64 rows = one contiguous [64][16] block of a row-major array: transposed through a wave-private LDS tile and written with
// 16-byte-per-lane stores that cover whole cache lines (per-lane row stores would scatter 16-byte pieces over 64 lines per instruction)
template <typename T>
__device__ __forceinline__ void wave_store_rows(T* __restrict__ dst, size_t wave_row0, int rows_in_wave, typename RowTile<T>::V* tile,
                                                int lane, const T s[16]) {
    using R = RowTile<T>;
    using V = typename R::V;
    V v[R::kCh];
    memcpy(v, s, sizeof(v));
#pragma unroll
    for (int k = 0; k < R::kCh; ++k) tile[lane * R::kStride + k] = v[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    V* d = reinterpret_cast<V*>(dst + (size_t)16 * wave_row0);
#pragma unroll
    for (int q = 0; q < R::kCh; ++q) {
        const int cidx = q * 64 + lane;
        if (cidx < rows_in_wave * R::kCh) {   // streaming store: nothing in this launch reads the rows again
            typedef float f32x4n __attribute__((ext_vector_type(4)));
            static_assert(sizeof(V) == sizeof(f32x4n), "16-byte chunks");
            const V x = tile[(cidx / R::kCh) * R::kStride + (cidx % R::kCh)];
            __builtin_nontemporal_store(__builtin_bit_cast(f32x4n, x), reinterpret_cast<f32x4n*>(d + cidx));
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the tile may be rewritten
}

// kRows: also write env.states after EVERY step to states_steps [K][N][16] and the truncation flags to trunc_out [K][N] -- the rollout
// a trainer consumes (q3_rollout); without them (q3_step_many) a step moves its action in and reward / done out only.
template <typename T, bool kRows>
__global__ __launch_bounds__(kQ3Block) void q3_rollout_kernel(Q3Params P, Q3Buffers<T> B, const float4* __restrict__ actions,
                                                              int K, T* __restrict__ rew_out, uint8_t* __restrict__ done_out,
                                                              uint8_t* __restrict__ trunc_out, T* __restrict__ states_steps,
                                                              T* __restrict__ states_out) {
    __shared__ typename RowTile<T>::V lds[kRows ? RowTile<T>::kLdsChunks : 1];
    const int i = blockIdx.x * kQ3Block + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave_row0 = i - lane;
    if (wave_row0 >= P.n) return;               // whole wave past the end
    const bool active = i < P.n;
    if (!kRows && !active) return;
    const int ii = active ? i : wave_row0;      // kRows: ragged-tail lanes shadow the wave's first env (they move rows of the tile)
    const int rows_in_wave = min(64, P.n - wave_row0);
    typename RowTile<T>::V* tile = lds + (kRows ? (threadIdx.x >> 6) * 64 * RowTile<T>::kStride : 0);
    Q3Env<T> e;
    q3_load(B, ii, e);
    float4 a = actions[ii];
    for (int k = 0; k < K; ++k) {
        const float u[4] = {a.x, a.y, a.z, a.w};
        if (k + 1 < K) a = actions[(size_t)(k + 1) * P.n + ii];  // next step's action is in flight during this step
        bool done, trunc;
        const T reward = q3_step_env(P, ii, e, u, done, trunc);
        if (active) {
            if (rew_out) rew_out[(size_t)k * P.n + i] = reward;
            if (done_out) done_out[(size_t)k * P.n + i] = done ? 1 : 0;
            if (kRows && trunc_out) trunc_out[(size_t)k * P.n + i] = trunc ? 1 : 0;
        }
        if constexpr (kRows) wave_store_rows<T>(states_steps + (size_t)k * P.n * 16, (size_t)wave_row0, rows_in_wave, tile, lane, e.s);
    }
    if (!active) return;
    q3_store(B, i, e);
    if (states_out) store_row<T>(states_out, i, e.s);
}

template <typename T>
__global__ __launch_bounds__(kQ3Block) void q3_reset_kernel(Q3Params P, Q3Buffers<T> B, const uint8_t* __restrict__ mask,
                                                            T* __restrict__ states_out) {
    const int i = blockIdx.x * kQ3Block + threadIdx.x;
    if (i >= P.n) return;
    Q3Env<T> e;
    q3_load(B, i, e);
    if (!mask || mask[i]) {
        q3_reset_env(P, i, e);
        q3_store(B, i, e);
    }
    if (states_out) store_row<T>(states_out, i, e.s);
}

template <typename T>
__global__ __launch_bounds__(kQ3Block) void q3_copy_state_kernel(int n, Q3Buffers<T> B, T* states_out, int32_t* target_out,
                                                                 int32_t* steps_out, const T* states_in,
                                                                 const int32_t* target_in, const int32_t* steps_in) {
    const int i = blockIdx.x * kQ3Block + threadIdx.x;
    if (i >= n) return;
    T s[16];
    if (states_in) {
        load_row<T>(states_in, i, s);
        store_row<T>(B.states, i, s);
    }
    if (target_in) B.target[i] = target_in[i];
    if (steps_in) B.steps[i] = steps_in[i];
    if (states_out) {
        load_row<T>(B.states, i, s);
        store_row<T>(states_out, i, s);
    }
    if (target_out) target_out[i] = B.target[i];
    if (steps_out) steps_out[i] = B.steps[i];
}

// ---------------------------------------------------------------------------------------------------
// Closed-loop rollout (q3_rollout_policy): policy network + Gaussian action sampling + env step, K times in one kernel -- PPO's collect
// phase for the two predecessor envs.  The step RESTATES rollout_policy_kernel's (quadrace_env_kernels.hpp) statement for statement with
// the q3 env in the middle: same noise slices in the second hidden layer's shadow, same observation-row store under the third layer,
// same sampling arithmetic, one 256-env workgroup per CU.  The observation of both envs is the state row itself, rounded to float32.
//   T = double (hover) / float (gates); kF32: the f32-class forward (policy_forward_f32class) instead of the f16-operand one.
// ---------------------------------------------------------------------------------------------------
constexpr int kQ3ObsLen = 16;
constexpr int kQ3ObsTileChunks = 64 * RowTile<float>::kStride;   // one wave's [64][16] float32 rows, row stride padded (16-byte chunks)
constexpr size_t kQ3PolicyLdsBytes = (size_t)qr::PolicyDims<kQ3ObsLen>::kTotalHalf8 * 16 + (size_t)(kQ3Block / 64) * kQ3ObsTileChunks * 16;

__device__ __forceinline__ void q3_obs_tile_write(float4* __restrict__ tile, int lane, const float* o) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[lane * RowTile<float>::kStride + k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// full waves only: 256 chunks, every round with the whole wave
__device__ __forceinline__ void q3_obs_tile_flush(const float4* __restrict__ tile, float* __restrict__ obs_out, size_t wave_first_env, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float4* g4 = reinterpret_cast<float4*>(obs_out + wave_first_env * kQ3ObsLen);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int cidx = q * 64 + lane;
        qr::stream_store(g4 + cidx, tile[(cidx >> 2) * RowTile<float>::kStride + (cidx & 3)]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void q3_store_obs(float* __restrict__ obs_out, size_t i, const float* o) {
    float4* r4 = reinterpret_cast<float4*>(obs_out + i * kQ3ObsLen);
#pragma unroll
    for (int k = 0; k < 4; ++k) qr::stream_store(r4 + k, make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]));
}

template <typename T, bool kF32>
__global__ void __launch_bounds__(kQ3Block, 1)
q3_rollout_policy_kernel(Q3Params P, Q3Buffers<T> B, qr::PolicyArgs A, int K, float* __restrict__ obs_out, float4* __restrict__ act_out,
                         float* __restrict__ logp_out, float* __restrict__ rew_out, uint8_t* __restrict__ done_out,
                         uint8_t* __restrict__ trunc_out, float* __restrict__ term_obs, float* __restrict__ last_obs_out,
                         T* __restrict__ states_out) {
    using namespace qr;
    constexpr int L = kQ3ObsLen;
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);   // policy weights (f16) | obs tiles
    const int i = blockIdx.x * kQ3Block + threadIdx.x;
    const int lane = threadIdx.x & 63;
    {
        const float4* s4 = reinterpret_cast<const float4*>(A.weights);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int j = threadIdx.x; j < D::kTotalHalf8; j += kQ3Block) d4[j] = s4[j];
    }
    __syncthreads();
    const int wave_first = i - lane;
    if (wave_first >= P.n) return;              // whole wave past the end (no workgroup barrier follows)
    const bool active = i < P.n;
    const int ii = active ? i : wave_first;     // ragged-tail lanes shadow the wave's first env: they take part in every matrix
                                                // instruction and wave barrier and store nothing
    const bool full_wave = wave_first + 64 <= P.n;
    float4* tile = reinterpret_cast<float4*>(smem + (size_t)D::kTotalHalf8 * 16) + (threadIdx.x >> 6) * kQ3ObsTileChunks;
    Q3Env<T> e;
    q3_load(B, ii, e);
    const uint32_t gid_lo = P.gid_lo + (uint32_t)ii;
    const uint32_t gid_hi = P.gid_hi + (gid_lo < P.gid_lo ? 1u : 0u);
    const size_t n = (size_t)P.n;
    float o[L];
#pragma unroll
    for (int c = 0; c < L; ++c) o[c] = (float)e.s[c];
    for (int k = 0; k < K; ++k) {
        // Action noise eps ~ N(0, 1)^4: rollout_policy_kernel's slices, verbatim (drawn in deterministic mode too and then multiplied out)
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
        // the observation row of this step (the policy's input) is stored under the third layer's MFMAs (full waves)
        auto obs_slice = [&](int slot) {
            if (slot == 0 && full_wave) q3_obs_tile_write(tile, lane, o);
            if (slot == 2 && full_wave) q3_obs_tile_flush(tile, obs_out + (size_t)k * n * L, (size_t)wave_first, lane);
        };
        if constexpr (kF32) {
#pragma unroll
            for (int slot = 0; slot <= 16; ++slot) noise_slice(slot);
            obs_slice(0);
            obs_slice(2);
            policy_forward_f32class<L>(W, A.weights_lo, lane, o, mean);
        } else {
            policy_forward<L>(W, lane, o, mean, noise_slice, obs_slice);
        }
        float a[4] = {mean[0], mean[1], mean[2], mean[3]};
        float logp = A.logp_const;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float ec = A.deterministic ? 0.0f : eps[c];   // fmaf(std, 0, mean) = mean, fmaf(-0, 0, logp) = logp
            a[c] = fmaf(A.std[c], ec, mean[c]);
            logp = fmaf(-0.5f * ec, ec, logp);
        }
        // rollout buffer row t: the observation the action was computed from (stored above), the unclipped action, its log-prob
        if (!full_wave && active) q3_store_obs(obs_out + (size_t)k * n * L, (size_t)i, o);
        if (active) {
            stream_store(act_out + (size_t)k * n + i, make_float4(a[0], a[1], a[2], a[3]));
            stream_store(logp_out + (size_t)k * n + i, logp);
        }
        float u[4];
        clip_action(a, u);
        bool done, trunc;
        const T reward = q3_step_env(P, ii, e, u, done, trunc, [&]() {
            if (term_obs == nullptr || !active) return;   // the final state of the episode, before the auto-reset replaces it
            float* row = term_obs + ((size_t)k * n + i) * L;
#pragma unroll
            for (int c = 0; c < L; ++c) row[c] = (float)e.s[c];
        });
        if (active) {
            stream_store(rew_out + (size_t)k * n + i, (float)reward);
            stream_store(done_out + (size_t)k * n + i, (uint8_t)(done ? 1 : 0));
            if (trunc_out) stream_store(trunc_out + (size_t)k * n + i, (uint8_t)(trunc ? 1 : 0));
        }
#pragma unroll
        for (int c = 0; c < L; ++c) o[c] = (float)e.s[c];
    }
    if (!active) return;
    if (last_obs_out) q3_store_obs(last_obs_out, (size_t)i, o);
    q3_store(B, i, e);
    if (states_out) store_row<T>(states_out, i, e.s);
}

// ---------------------------------------------------------------------------------------------------
// Closed-loop evaluation (q3_evaluate_policy, q3_evaluate_policy_bank): q3_rollout_policy_kernel's step loop without everything an
// evaluation throws away -- no noise slices, no observation tile, no obs / act / logp / rew / done / term rows, NO global store inside
// the step loop.  What leaves the kernel is one 12-int record and one 4-float record per env (layout: include/quad3d.h, restated on
// the CPU in tests/q3_eval_spec.py, same order) and the env state after K steps, which equals q3_rollout_policy's in deterministic mode.
// How an episode ended is decided from the pre-step state (gates: ground and out of bounds are the reference's PRE-step predicates),
// from what the before_reset hook sees (step counter and target after the step, before the reset replaces them) and from done / trunc:
//   hover  SUCCESS = done && !trunc (goal, inside bounds, before the limit); else TIMEOUT if the step counter reached max_steps; else OOB
//   gates  SUCCESS = final gate passed; else TIMEOUT if trunc; else GROUND; else OOB; else COLLISION
// All times are integer step counts; the float record is three sequential float32 sums without FMA, as in eval_policy_body.
//   i: the lane's env (state, rec, recf);  rid: its id in the reset stream (what q3_step_env / q3_block receive as `i`)
//   kTail: lanes with i >= P.n exist: they shadow the wave's first env (MFMA is wave-wide) and store nothing
// ---------------------------------------------------------------------------------------------------
static_assert(Q3_EVAL_REC_INTS == 12 && Q3_EVAL_REC_FLOATS == 4, "record layout of include/quad3d.h");
constexpr size_t kQ3EvalLdsBytes = (size_t)qr::PolicyDims<kQ3ObsLen>::kTotalHalf8 * 16;   // the policy image, nothing else

template <typename T, bool kF32, bool kTail>
__device__ __forceinline__ void q3_eval_body(const Q3Params& P, const qr::half8* __restrict__ img, const qr::half8* __restrict__ img_lo,
                                             int i, int rid, int K, int4* __restrict__ rec, float4* __restrict__ recf,
                                             const Q3Buffers<T>& B) {
    using namespace qr;
    constexpr int L = kQ3ObsLen;
    constexpr bool kGates = sizeof(T) == sizeof(float);
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);   // policy weights (f16) of THIS workgroup's policy
    const int lane = threadIdx.x & 63;
    {
        const float4* s4 = reinterpret_cast<const float4*>(img);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int j = threadIdx.x; j < D::kTotalHalf8; j += kQ3Block) d4[j] = s4[j];
    }
    __syncthreads();
    bool active = true;
    int ii = i, rr = rid;
    if constexpr (kTail) {
        const int wave_first = i - lane;
        if (wave_first >= P.n) return;          // whole wave past the end (no workgroup barrier follows)
        active = i < P.n;
        if (!active) {                          // ragged-tail lanes shadow the wave's first env and store nothing
            ii = wave_first;
            rr = rid - lane;
        }
    }
    Q3Env<T> e;
    q3_load(B, ii, e);
    // the lane's record: read here, written behind the loop (a caller continues an evaluation by passing the same buffers again)
    const int4 r0 = rec[(size_t)ii * 3], r1 = rec[(size_t)ii * 3 + 1], r2 = rec[(size_t)ii * 3 + 2];
    int n_steps = r0.x, n_success = r0.y, n_timeout = r0.z, n_oob = r0.w, n_ground = r1.x, n_collision = r1.y;
    int len_success = r1.z, len_all = r1.w, n_pass = r2.x, best = r2.y;
    float ep_ret = 0.0f, ret_sum = 0.0f, ret_sq = 0.0f;
    if (recf) {
        const float4 f = recf[ii];
        ep_ret = f.x; ret_sum = f.y; ret_sq = f.z;
    }
    float o[L];
#pragma unroll
    for (int c = 0; c < L; ++c) o[c] = (float)e.s[c];
    for (int k = 0; k < K; ++k) {
        float mean[4];
        if constexpr (kF32) {
            // The low pieces are read from global memory at the same addresses every step, and this loop has no store that could
            // alias them: left alone the compiler hoists all of those loads in front of the loop and spills them (1.8-1.9 KB of
            // scratch per lane, 1.5 x the rollout kernel's time).  An opaque copy of the (workgroup-uniform) base per step keeps
            // them inside the step, where the rollout kernel has them.
            const half8* lo = img_lo;
            asm volatile("" : "+s"(lo));
            policy_forward_f32class<L>(W, lo, lane, o, mean);
        } else {
            policy_forward<L>(W, lane, o, mean);
        }
        float u[4];
        clip_action(mean, u);
        const int target_before = e.target;
        bool pre_ground = false, pre_oob = false;
        if constexpr (kGates) {                 // the reference tests the PRE-step state for these two
            pre_ground = e.s[2] > (T)0;
            pre_oob = fabsf((float)e.s[0]) > 10.0f || fabsf((float)e.s[1]) > 10.0f || fabsf((float)e.s[9]) > 1000.0f ||
                      fabsf((float)e.s[10]) > 1000.0f || fabsf((float)e.s[11]) > 1000.0f;
        }
        int end_len = 0;                        // the step counter at the end: after the increment, before the reset
        bool end_final = false;                 // the target at the end: after e.target += 1, before the reset
        bool done, trunc;
        const T reward = q3_step_env(P, rr, e, u, done, trunc, [&]() {
            end_len = e.steps;
            if constexpr (kGates) end_final = e.target >= P.num_gates;
        });
        // ---- accounting (tests/q3_eval_spec.py, same order).  A pass on the step that ends the episode is not counted here: a final
        // pass is the SUCCESS end, and any other end has replaced the target
        n_steps += 1;
        if (!done && e.target != target_before) n_pass += 1;
        ep_ret = add_rn(ep_ret, (float)reward);
        if (done) {
            bool success, timeout;
            if constexpr (kGates) {
                success = end_final;
                timeout = !success && trunc;
                const bool ground = !success && !timeout && pre_ground;
                const bool oob = !success && !timeout && !ground && pre_oob;
                const bool collision = !success && !timeout && !ground && !oob;
                n_ground += ground ? 1 : 0;
                n_oob += oob ? 1 : 0;
                n_collision += collision ? 1 : 0;
            } else {
                success = !trunc;
                timeout = !success && end_len >= P.max_steps;
                n_oob += (!success && !timeout) ? 1 : 0;
            }
            n_success += success ? 1 : 0;
            n_timeout += timeout ? 1 : 0;
            len_all += end_len;
            if (success) {
                len_success += end_len;
                best = (best == 0 || end_len < best) ? end_len : best;
            }
            ret_sum = add_rn(ret_sum, ep_ret);
            ret_sq = add_rn(ret_sq, mul_rn(ep_ret, ep_ret));
            ep_ret = 0.0f;
        }
#pragma unroll
        for (int c = 0; c < L; ++c) o[c] = (float)e.s[c];
    }
    if (!active) return;
    int4* row = rec + (size_t)i * 3;
    row[0] = make_int4(n_steps, n_success, n_timeout, n_oob);
    row[1] = make_int4(n_ground, n_collision, len_success, len_all);
    row[2] = make_int4(n_pass, best, 0, 0);
    if (recf) recf[i] = make_float4(ep_ret, ret_sum, ret_sq, 0.0f);
    q3_store(B, i, e);
}

template <typename T, bool kF32>
__global__ void __launch_bounds__(kQ3Block, 1)
q3_eval_policy_kernel(Q3Params P, Q3Buffers<T> B, const qr::half8* __restrict__ img, const qr::half8* __restrict__ img_lo, int K,
                      int4* __restrict__ rec, float4* __restrict__ recf) {
    const int i = blockIdx.x * kQ3Block + threadIdx.x;
    q3_eval_body<T, kF32, true>(P, img, img_lo, i, i, K, rec, recf, B);
}

// A bank of policies in one launch: P policies x E envs per policy, E a multiple of kQ3Block and N = P E exactly (no tail lanes: the
// host refuses anything else).  Workgroup b stages image b / (E / kQ3Block) of the bank, and the reset stream is group-local: lane i
// draws with env id (i mod E), so group p flies exactly what an E-env handle with the same seed and env_id_base flies under
// q3_evaluate_policy.  The policy index, both image bases and the group's first env are derived from blockIdx alone.
template <typename T, bool kF32>
__global__ void __launch_bounds__(kQ3Block, 1)
q3_eval_policy_bank_kernel(Q3Params P, Q3Buffers<T> B, const qr::half8* __restrict__ bank, const qr::half8* __restrict__ bank_lo,
                           int wgs_per_policy, int K, int4* __restrict__ rec, float4* __restrict__ recf) {
    using D = qr::PolicyDims<kQ3ObsLen>;
    const int pol = (int)blockIdx.x / wgs_per_policy;
    const int local0 = ((int)blockIdx.x - pol * wgs_per_policy) * kQ3Block;
    const qr::half8* __restrict__ img = bank + (size_t)pol * D::kTotalHalf8;
    const qr::half8* __restrict__ img_lo = bank_lo + (size_t)pol * D::kTotalHalf8;
    const int i = blockIdx.x * kQ3Block + threadIdx.x;   // < P.n: the grid is exactly P.n / kQ3Block workgroups
    q3_eval_body<T, kF32, false>(P, img, img_lo, i, local0 + (int)threadIdx.x, K, rec, recf, B);
}

}  // namespace

struct q3_env {
    int kind = 0, device = 0;
    bool has_track = false;
    Q3Params P{};
    void* d_states = nullptr;
    int32_t* d_target = nullptr;
    int32_t* d_steps = nullptr;
    uint32_t* d_episode = nullptr;
    template <typename T>
    Q3Buffers<T> buffers() const { return Q3Buffers<T>{static_cast<T*>(d_states), d_target, d_steps, d_episode}; }
    int grid() const { return (P.n + kQ3Block - 1) / kQ3Block; }
};

namespace {
const char* const kQ3LenRule = "must be 16 (the state row is the observation)";

int q3_ready(const q3_env* e) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    if (e->kind == Q3_KIND_GATES && !e->has_track) return qr::set_last_error(QR_E_STATE, "q3_set_track has not been called");
    return QR_OK;
}

template <typename T>
hipError_t q3_launch_rollout_policy(q3_env* e, const qr::PolicyArgs& A, int K, float* obs, float* act, float* logp, float* rew,
                                           uint8_t* done, uint8_t* trunc, float* term_obs, float* last_obs, void* states_out, hipStream_t st) {
    float4* act4 = reinterpret_cast<float4*>(act);
    T* so = static_cast<T*>(states_out);
    if (A.f32class)
        return qr::launch_dynamic_lds<q3_rollout_policy_kernel<T, true>>(dim3(e->grid()), dim3(kQ3Block), kQ3PolicyLdsBytes, st, e->P,
                                                                         e->buffers<T>(), A, K, obs, act4, logp, rew, done, trunc, term_obs,
                                                                         last_obs, so);
    return qr::launch_dynamic_lds<q3_rollout_policy_kernel<T, false>>(dim3(e->grid()), dim3(kQ3Block), kQ3PolicyLdsBytes, st, e->P,
                                                                      e->buffers<T>(), A, K, obs, act4, logp, rew, done, trunc, term_obs,
                                                                      last_obs, so);
}

template <typename T>
hipError_t q3_launch_eval_policy(q3_env* e, const qr::half8* img, const qr::half8* img_lo, bool f32class, int K, int32_t* rec, float* recf,
                                 hipStream_t st) {
    int4* rec4 = reinterpret_cast<int4*>(rec);
    float4* recf4 = reinterpret_cast<float4*>(recf);
    if (f32class)
        return qr::launch_dynamic_lds<q3_eval_policy_kernel<T, true>>(dim3(e->grid()), dim3(kQ3Block), kQ3EvalLdsBytes, st, e->P, e->buffers<T>(),
                                                                      img, img_lo, K, rec4, recf4);
    return qr::launch_dynamic_lds<q3_eval_policy_kernel<T, false>>(dim3(e->grid()), dim3(kQ3Block), kQ3EvalLdsBytes, st, e->P, e->buffers<T>(), img,
                                                                   img_lo, K, rec4, recf4);
}

// The caller guarantees envs_per_policy % kQ3Block == 0 and num_policies * envs_per_policy == P.n (checked again here: a grid that does
// not match P.n would read and write out of bounds).
template <typename T>
hipError_t q3_launch_eval_policy_bank(q3_env* e, const qr::half8* bank, const qr::half8* bank_lo, bool f32class, int num_policies,
                                      int envs_per_policy, int K, int32_t* rec, float* recf, hipStream_t st) {
    if (num_policies < 1 || envs_per_policy < kQ3Block || envs_per_policy % kQ3Block != 0 ||
        (long long)num_policies * envs_per_policy != (long long)e->P.n)
        return hipErrorInvalidValue;
    int4* rec4 = reinterpret_cast<int4*>(rec);
    float4* recf4 = reinterpret_cast<float4*>(recf);
    const dim3 grid((unsigned)(e->P.n / kQ3Block));
    const int wgs = envs_per_policy / kQ3Block;
    if (f32class)
        return qr::launch_dynamic_lds<q3_eval_policy_bank_kernel<T, true>>(grid, dim3(kQ3Block), kQ3EvalLdsBytes, st, e->P, e->buffers<T>(), bank,
                                                                           bank_lo, wgs, K, rec4, recf4);
    return qr::launch_dynamic_lds<q3_eval_policy_bank_kernel<T, false>>(grid, dim3(kQ3Block), kQ3EvalLdsBytes, st, e->P, e->buffers<T>(), bank,
                                                                        bank_lo, wgs, K, rec4, recf4);
}

// what q3_evaluate_policy and q3_evaluate_policy_bank refuse alike (`who` names the entry point in the message)
int q3_check_eval_args(const q3_env* e, int K, int flags, const int32_t* rec, const float* recf, const std::string& w) {
    if (!e) return qr::set_last_error(QR_E_INVALID, w + "null q3_env handle");
    if (!rec) return qr::set_last_error(QR_E_INVALID, w + "rec_dev is null");
    if (K < 1) return qr::set_last_error(QR_E_INVALID, w + "num_steps must be >= 1");
    if (flags != 0 && flags != QR_ROLLOUT_F32CLASS) return qr::set_last_error(QR_E_INVALID, w + "`flags` takes 0 or QR_ROLLOUT_F32CLASS");
    if (((uintptr_t)rec | (uintptr_t)recf) & 15u) return qr::set_last_error(QR_E_INVALID, w + "rec_dev / recf_dev must be 16-byte aligned");
    return QR_OK;
}

}  // namespace

extern "C" {

int q3_create(int kind, int num_envs, int device, uint64_t env_id_base, q3_env** out) {
    if (!out) return qr::set_last_error(QR_E_INVALID, "out is null");
    *out = nullptr;
    if (kind != Q3_KIND_HOVER && kind != Q3_KIND_GATES) return qr::set_last_error(QR_E_INVALID, "kind must be Q3_KIND_HOVER or Q3_KIND_GATES");
    if (num_envs < 1) return qr::set_last_error(QR_E_INVALID, "num_envs must be >= 1");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return qr::set_last_error(QR_E_NO_DEVICE, "no HIP device visible: libquadrace has no CPU fallback");
    if (device < 0 || device >= count) return qr::set_last_error(QR_E_INVALID, "device index out of range");
    hipDeviceProp_t prop;
    QR_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return qr::set_last_error(QR_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    QR_HIP(hipSetDevice(device));
    q3_env* e = new q3_env();
    e->kind = kind;
    e->device = device;
    e->P.n = num_envs;
    e->P.max_steps = 1000;  // Q3 cell 6 / 14 __init__
    e->P.dt = 0.01;
    e->P.pos_thr = 0.3;
    e->P.vel_thr = 0.3;
    e->P.ang_thr = 10 * 3.141592653589793 / 180;
    e->P.rat_thr = 10 * 3.141592653589793 / 180;
    e->P.gid_lo = (uint32_t)env_id_base;
    e->P.gid_hi = (uint32_t)(env_id_base >> 32);
    const size_t n = (size_t)num_envs, esz = kind == Q3_KIND_HOVER ? 8 : 4;
    hipError_t err = hipMalloc(&e->d_states, n * 16 * esz);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_target), n * 4);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_steps), n * 4);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_episode), n * 4);
    if (err == hipSuccess) err = hipMemset(e->d_states, 0, n * 16 * esz);  // np.zeros
    if (err == hipSuccess) err = hipMemset(e->d_target, 0, n * 4);
    if (err == hipSuccess) err = hipMemset(e->d_steps, 0, n * 4);
    if (err == hipSuccess) err = hipMemset(e->d_episode, 0, n * 4);
    if (err != hipSuccess) {
        q3_destroy(e);
        return qr::set_last_error(QR_E_HIP, std::string("allocating env state: ") + hipGetErrorString(err));
    }
    *out = e;
    return QR_OK;
}

int q3_destroy(q3_env* e) {
    if (!e) return QR_OK;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(e->d_states);
    (void)hipFree(e->d_target);
    (void)hipFree(e->d_steps);
    (void)hipFree(e->d_episode);
    delete e;
    return QR_OK;
}

int q3_num_envs(const q3_env* e) { return e ? e->P.n : qr::set_last_error(QR_E_INVALID, "null q3_env handle"); }
int q3_elem_size(const q3_env* e) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    return e->kind == Q3_KIND_HOVER ? 8 : 4;
}

int q3_set_track(q3_env* e, const float* gate_pos, const float* gate_yaw, int G, const float start_pos[3]) {
    if (!e || !gate_pos || !gate_yaw || !start_pos) return qr::set_last_error(QR_E_INVALID, "null argument");
    if (e->kind != Q3_KIND_GATES) return qr::set_last_error(QR_E_STATE, "q3_set_track applies to Q3_KIND_GATES only");
    if (G < 1 || G > kQ3MaxGates) return qr::set_last_error(QR_E_INVALID, "num_gates must be in 1..32");
    e->P.num_gates = G;
    for (int g = 0; g < G; ++g) {
        for (int k = 0; k < 3; ++k) e->P.gate[g][k] = gate_pos[3 * g + k];
        e->P.gate[g][3] = gate_yaw[g];
        e->P.gate_normal[g][0] = cosf(gate_yaw[g]);  // np.cos / np.sin of the float32 yaw (Q3 cell 14 step_wait)
        e->P.gate_normal[g][1] = sinf(gate_yaw[g]);
    }
    for (int k = 0; k < 3; ++k) e->P.start[k] = start_pos[k];
    e->has_track = true;
    return QR_OK;
}

int q3_set_limits(q3_env* e, int max_steps, double dt) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    if (max_steps < 1 || !(dt > 0.0)) return qr::set_last_error(QR_E_INVALID, "max_steps must be >= 1 and dt > 0");
    e->P.max_steps = max_steps;
    e->P.dt = dt;
    return QR_OK;
}

int q3_set_thresholds(q3_env* e, double pos, double vel, double ang, double rat) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    if (e->kind != Q3_KIND_HOVER) return qr::set_last_error(QR_E_STATE, "q3_set_thresholds applies to Q3_KIND_HOVER only");
    e->P.pos_thr = pos;
    e->P.vel_thr = vel;
    e->P.ang_thr = ang;
    e->P.rat_thr = rat;
    return QR_OK;
}

int q3_seed(q3_env* e, uint64_t seed) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    QR_HIP(hipSetDevice(e->device));
    e->P.seed_lo = (uint32_t)seed;
    e->P.seed_hi = (uint32_t)(seed >> 32);
    QR_HIP(hipDeviceSynchronize());
    QR_HIP(hipMemset(e->d_episode, 0, (size_t)e->P.n * 4));
    return QR_OK;
}

int q3_reset(q3_env* e, const uint8_t* mask, void* states_out, void* stream) {
    if (int rc = q3_ready(e)) return rc;
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e->kind == Q3_KIND_HOVER)
        q3_reset_kernel<double><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<double>(), mask, static_cast<double*>(states_out));
    else
        q3_reset_kernel<float><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<float>(), mask, static_cast<float*>(states_out));
    QR_HIP(hipGetLastError());
    return QR_OK;
}

int q3_step(q3_env* e, const float* actions, void* states_out, void* rew_out, uint8_t* done_out, uint8_t* trunc_out,
            void* stream) {
    if (int rc = q3_ready(e)) return rc;
    if (!actions) return qr::set_last_error(QR_E_INVALID, "actions_dev is null");
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float4* a = reinterpret_cast<const float4*>(actions);
    if (e->kind == Q3_KIND_HOVER)
        q3_step_kernel<double><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<double>(), a, static_cast<double*>(states_out),
                                                              static_cast<double*>(rew_out), done_out, trunc_out);
    else
        q3_step_kernel<float><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<float>(), a, static_cast<float*>(states_out),
                                                             static_cast<float*>(rew_out), done_out, trunc_out);
    QR_HIP(hipGetLastError());
    return QR_OK;
}

static int q3_launch_rollout(q3_env* e, const float* actions, int K, void* states_steps, void* rew_out, uint8_t* done_out,
                             uint8_t* trunc_out, void* states_out, void* stream) {
    if (int rc = q3_ready(e)) return rc;
    if (!actions) return qr::set_last_error(QR_E_INVALID, "actions_dev is null");
    if (K < 1) return qr::set_last_error(QR_E_INVALID, "num_steps must be >= 1");
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float4* a = reinterpret_cast<const float4*>(actions);
    if (e->kind == Q3_KIND_HOVER) {
        if (states_steps)
            q3_rollout_kernel<double, true><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<double>(), a, K, static_cast<double*>(rew_out), done_out,
                                                                           trunc_out, static_cast<double*>(states_steps), static_cast<double*>(states_out));
        else
            q3_rollout_kernel<double, false><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<double>(), a, K, static_cast<double*>(rew_out), done_out,
                                                                            nullptr, nullptr, static_cast<double*>(states_out));
    } else {
        if (states_steps)
            q3_rollout_kernel<float, true><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<float>(), a, K, static_cast<float*>(rew_out), done_out,
                                                                          trunc_out, static_cast<float*>(states_steps), static_cast<float*>(states_out));
        else
            q3_rollout_kernel<float, false><<<e->grid(), kQ3Block, 0, st>>>(e->P, e->buffers<float>(), a, K, static_cast<float*>(rew_out), done_out,
                                                                           nullptr, nullptr, static_cast<float*>(states_out));
    }
    QR_HIP(hipGetLastError());
    return QR_OK;
}

int q3_step_many(q3_env* e, const float* actions, int K, void* rew_out, uint8_t* done_out, void* states_out, void* stream) {
    return q3_launch_rollout(e, actions, K, nullptr, rew_out, done_out, nullptr, states_out, stream);
}

int q3_rollout(q3_env* e, const float* actions, int K, void* states_steps_out, void* rew_out, uint8_t* done_out, uint8_t* trunc_out,
               void* stream) {
    if (!states_steps_out) return qr::set_last_error(QR_E_INVALID, "states_steps_out_dev is null (q3_step_many is the form without per-step rows)");
    return q3_launch_rollout(e, actions, K, states_steps_out, rew_out, done_out, trunc_out, nullptr, stream);
}

// Every refusal comes before anything is enqueued: a failed call leaves the env and the buffers untouched.
int q3_rollout_policy(q3_env* e, qr_policy* policy, int32_t K, const float* log_std, uint64_t noise_seed, uint64_t first_step, int32_t flags,
                      float* obs_out, float* act_out, float* logp_out, float* rew_out, uint8_t* done_out, uint8_t* trunc_out, float* term_obs,
                      float* last_obs, void* states_out, void* stream) {
    const char* who = "q3_rollout_policy";
    const std::string w = std::string(who) + ": ";
    if (!e) return qr::set_last_error(QR_E_INVALID, w + "null q3_env handle");
    if (!policy || !log_std) return qr::set_last_error(QR_E_INVALID, w + "null policy handle or log_std");
    if (K < 1) return qr::set_last_error(QR_E_INVALID, w + "num_steps must be >= 1");
    if (!obs_out || !act_out || !logp_out || !rew_out || !done_out) return qr::set_last_error(QR_E_INVALID, w + "obs/act/logp/rew/done buffers are required");
    if (flags < 0 || flags > (QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS))
        return qr::set_last_error(QR_E_INVALID, w + "`flags` takes QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS");
    if (int rc = qr::check_policy_handle(policy, kQ3ObsLen, e->device, who, kQ3LenRule)) return rc;
    if (((uintptr_t)obs_out | (uintptr_t)act_out | (uintptr_t)term_obs | (uintptr_t)last_obs | (uintptr_t)states_out) & 15u)
        return qr::set_last_error(QR_E_INVALID, w + "obs_out / act_out / term_obs / last_obs / states_out must be 16-byte aligned");
    qr::PolicyArgs A{};
    if (int rc = qr::fetch_policy_weights(policy, who, A.weights)) return rc;
    if (int rc = q3_ready(e)) return rc;
    A.weights_lo = qr::policy_weights_lo(policy);
    qr::set_sampling(A, qr::sampling_entry(log_std, noise_seed), first_step, flags);   // the action-noise stream of qr_rollout_policy
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e->kind == Q3_KIND_HOVER)
        QR_HIP(q3_launch_rollout_policy<double>(e, A, K, obs_out, act_out, logp_out, rew_out, done_out, trunc_out, term_obs, last_obs, states_out, st));
    else
        QR_HIP(q3_launch_rollout_policy<float>(e, A, K, obs_out, act_out, logp_out, rew_out, done_out, trunc_out, term_obs, last_obs, states_out, st));
    return QR_OK;
}

// Every refusal comes before anything is enqueued: a failed call leaves the env and the records untouched.
int q3_evaluate_policy(q3_env* e, qr_policy* policy, int32_t K, int32_t flags, int32_t* rec, float* recf, void* stream) {
    const char* who = "q3_evaluate_policy";
    const std::string w = std::string(who) + ": ";
    if (!policy) return qr::set_last_error(QR_E_INVALID, w + "null policy handle");
    if (int rc = q3_check_eval_args(e, K, flags, rec, recf, w)) return rc;
    if (int rc = qr::check_policy_handle(policy, kQ3ObsLen, e->device, who, kQ3LenRule)) return rc;
    const qr::half8* wt = nullptr;
    if (int rc = qr::fetch_policy_weights(policy, who, wt)) return rc;
    if (e->kind == Q3_KIND_GATES && !e->has_track) return qr::set_last_error(QR_E_STATE, w + "q3_set_track has not been called");
    const bool f32class = (flags & QR_ROLLOUT_F32CLASS) != 0;
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e->kind == Q3_KIND_HOVER)
        QR_HIP(q3_launch_eval_policy<double>(e, wt, qr::policy_weights_lo(policy), f32class, K, rec, recf, st));
    else
        QR_HIP(q3_launch_eval_policy<float>(e, wt, qr::policy_weights_lo(policy), f32class, K, rec, recf, st));
    return QR_OK;
}

int q3_evaluate_policy_bank(q3_env* e, qr_policy_bank* bank, int32_t num_policies, int32_t envs_per_policy, int32_t K, int32_t flags,
                            int32_t* rec, float* recf, void* stream) {
    const char* who = "q3_evaluate_policy_bank";
    const std::string w = std::string(who) + ": ";
    if (!bank) return qr::set_last_error(QR_E_INVALID, w + "null bank handle");
    if (int rc = q3_check_eval_args(e, K, flags, rec, recf, w)) return rc;
    if (int rc = qr::check_policy_bank(bank, kQ3ObsLen, e->device, who, "bank", kQ3LenRule)) return rc;
    if (num_policies < 1 || num_policies > qr::bank_capacity(bank)) return qr::set_last_error(QR_E_INVALID, w + "num_policies must be in 1..capacity");
    if (envs_per_policy < kQ3Block || envs_per_policy % kQ3Block != 0)
        return qr::set_last_error(QR_E_INVALID, w + "envs_per_policy must be a positive multiple of 256 (one workgroup serves one policy)");
    if ((long long)num_policies * envs_per_policy != (long long)e->P.n)
        return qr::set_last_error(QR_E_INVALID, w + "num_policies * envs_per_policy must equal num_envs");
    const int unset = qr::bank_first_unset(bank, num_policies);
    if (unset >= 0) return qr::set_last_error(QR_E_STATE, w + "slot " + std::to_string(unset) + " of the bank has no weights");
    if (e->kind == Q3_KIND_GATES && !e->has_track) return qr::set_last_error(QR_E_STATE, w + "q3_set_track has not been called");
    const bool f32class = (flags & QR_ROLLOUT_F32CLASS) != 0;
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e->kind == Q3_KIND_HOVER)
        QR_HIP(q3_launch_eval_policy_bank<double>(e, qr::bank_weights(bank), qr::bank_weights_lo(bank), f32class, num_policies, envs_per_policy, K,
                                                  rec, recf, st));
    else
        QR_HIP(q3_launch_eval_policy_bank<float>(e, qr::bank_weights(bank), qr::bank_weights_lo(bank), f32class, num_policies, envs_per_policy, K,
                                                 rec, recf, st));
    return QR_OK;
}

int q3_get_state(q3_env* e, void* states, int32_t* target, int32_t* steps, void* stream) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e->kind == Q3_KIND_HOVER)
        q3_copy_state_kernel<double><<<e->grid(), kQ3Block, 0, st>>>(e->P.n, e->buffers<double>(), static_cast<double*>(states),
                                                                    target, steps, nullptr, nullptr, nullptr);
    else
        q3_copy_state_kernel<float><<<e->grid(), kQ3Block, 0, st>>>(e->P.n, e->buffers<float>(), static_cast<float*>(states),
                                                                   target, steps, nullptr, nullptr, nullptr);
    QR_HIP(hipGetLastError());
    return QR_OK;
}

int q3_set_state(q3_env* e, const void* states, const int32_t* target, const int32_t* steps, void* stream) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e->kind == Q3_KIND_HOVER)
        q3_copy_state_kernel<double><<<e->grid(), kQ3Block, 0, st>>>(e->P.n, e->buffers<double>(), nullptr, nullptr, nullptr,
                                                                    static_cast<const double*>(states), target, steps);
    else
        q3_copy_state_kernel<float><<<e->grid(), kQ3Block, 0, st>>>(e->P.n, e->buffers<float>(), nullptr, nullptr, nullptr,
                                                                   static_cast<const float*>(states), target, steps);
    QR_HIP(hipGetLastError());
    return QR_OK;
}

int q3_episode_counts(q3_env* e, uint32_t* get_dev, const uint32_t* set_dev, void* stream) {
    if (!e) return qr::set_last_error(QR_E_INVALID, "null q3_env handle");
    QR_HIP(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bytes = (size_t)e->P.n * 4;
    if (set_dev) QR_HIP(hipMemcpyAsync(e->d_episode, set_dev, bytes, hipMemcpyDeviceToDevice, st));
    if (get_dev) QR_HIP(hipMemcpyAsync(get_dev, e->d_episode, bytes, hipMemcpyDeviceToDevice, st));
    return QR_OK;
}

}  // extern "C"
