// quadrace_policy.hip -- policy-network kernels (see quadrace_policy.hpp) and their host side.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/quadrace.h"
#include "quadrace_launch.hpp"

namespace qr {

constexpr int kPolBlock = 256;

// cooperative copy of the packed f16 weights (16-byte elements) into LDS
__device__ __forceinline__ void stage_policy(const half8* __restrict__ src, half8* dst, int count) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = threadIdx.x; i < count; i += kPolBlock) d4[i] = s4[i];
}

// obs [n][L] row-major -> mean actions [n][4]
template <int L>
__global__ void __launch_bounds__(kPolBlock, 1)
policy_kernel(const half8* __restrict__ weights, int n, const float* __restrict__ obs, float4* __restrict__ mean_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);
    const int i = blockIdx.x * kPolBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int ii = i < n ? i : 0;  // ragged-tail lanes shadow env 0 (MFMA / swaps are wave-wide)
    float o[L];
    const float* row = obs + (size_t)ii * L;
    if constexpr (L % 4 == 0) {
#pragma unroll
        for (int k = 0; k < L / 4; ++k) {
            const float4 v = reinterpret_cast<const float4*>(row)[k];
            o[4 * k] = v.x; o[4 * k + 1] = v.y; o[4 * k + 2] = v.z; o[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < L; ++k) o[k] = row[k];
    }
    stage_policy(weights, W, PolicyDims<L>::kTotalHalf8);
    __syncthreads();
    float mean[4];
    policy_forward<L>(W, lane, o, mean);
    if (i < n) mean_out[i] = make_float4(mean[0], mean[1], mean[2], mean[3]);
}

hipError_t launch_policy(int L, const half8* w, int n, const float* obs, float* mean, hipStream_t st) {
    return dispatch_L(L, [&](auto Lc) {
        constexpr int kL = decltype(Lc)::value;
        return launch_dynamic_lds<policy_kernel<kL>>(dim3((n + kPolBlock - 1) / kPolBlock), dim3(kPolBlock),
                                                     (size_t)PolicyDims<kL>::kTotalHalf8 * 16, st, w, n, obs, reinterpret_cast<float4*>(mean));
    }, [] { return hipErrorInvalidValue; });
}

template <int L>
__global__ void __launch_bounds__(kPolBlock, 1)
policy_f32class_kernel(const half8* __restrict__ w0, const half8* __restrict__ w1, int n, const float* __restrict__ obs,
                       float4* __restrict__ mean_out) {
    using D = PolicyDims<L>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);
    const int i = blockIdx.x * kPolBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int ii = i < n ? i : 0;  // ragged-tail lanes shadow env 0 (MFMA / swaps are wave-wide)
    float o[L];
    const float* row = obs + (size_t)ii * L;
#pragma unroll
    for (int k = 0; k < L; ++k) o[k] = row[k];
    stage_policy(w0, W, D::kTotalHalf8);
    __syncthreads();
    float mean[4];
    policy_forward_f32class<L>(W, w1, lane, o, mean);
    if (i < n) mean_out[i] = make_float4(mean[0], mean[1], mean[2], mean[3]);
}

hipError_t launch_policy_f32class(int L, const half8* w0, const half8* w1, int n, const float* obs, float* mean, hipStream_t st) {
    return dispatch_L(L, [&](auto Lc) {
        constexpr int kL = decltype(Lc)::value;
        return launch_dynamic_lds<policy_f32class_kernel<kL>>(dim3((n + kPolBlock - 1) / kPolBlock), dim3(kPolBlock),
                                                              (size_t)PolicyDims<kL>::kTotalHalf8 * 16, st, w0, w1, n, obs,
                                                              reinterpret_cast<float4*>(mean));
    }, [] { return hipErrorInvalidValue; });
}

}  // namespace qr

struct qr_policy {
    int L = 0, device = 0;
    int steps1 = 0;
    size_t total_half8 = 0;
    qr::half8* d_weights = nullptr;      // W0 = f16(w): the image of the f16-operand kernels
    qr::half8* d_weights_lo = nullptr;   // W1 = f16(w - W0): the low pieces, same layout (f32-class forward only)
    bool has_weights = false;
};

// A bank of policies for qr_evaluate_policy_bank: two contiguous device arrays [capacity][total_half8] half8 (the f16 images and the
// low pieces), slot s at element s * total_half8, each slot bit-identical to the two images of a qr_policy given the same arrays.
struct qr_policy_bank {
    int L = 0, device = 0, capacity = 0;
    int steps1 = 0;
    size_t total_half8 = 0;
    qr::half8* d_weights = nullptr;
    qr::half8* d_weights_lo = nullptr;
    std::vector<uint8_t> is_set;   // per slot: qr_policy_bank_set has succeeded
};

namespace {
inline int rho(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
}  // namespace

namespace qr {  // accessors for the closed-loop rollout entry point in quadrace_abi.hip
const half8* policy_weights(const qr_policy* p) { return (p && p->has_weights) ? p->d_weights : nullptr; }
const half8* policy_weights_lo(const qr_policy* p) { return (p && p->has_weights) ? p->d_weights_lo : nullptr; }
int policy_obs_len(const qr_policy* p) { return p ? p->L : -1; }
int policy_device(const qr_policy* p) { return p ? p->device : -1; }
// the same for a bank (qr_evaluate_policy_bank in quadrace_abi.hip)
const half8* bank_weights(const qr_policy_bank* b) { return b ? b->d_weights : nullptr; }
const half8* bank_weights_lo(const qr_policy_bank* b) { return b ? b->d_weights_lo : nullptr; }
int bank_obs_len(const qr_policy_bank* b) { return b ? b->L : -1; }
int bank_device(const qr_policy_bank* b) { return b ? b->device : -1; }
int bank_capacity(const qr_policy_bank* b) { return b ? b->capacity : -1; }
int bank_first_unset(const qr_policy_bank* b, int num_policies) {   // first slot of [0, num_policies) never set, or -1
    for (int s = 0; s < num_policies && s < b->capacity; ++s)
        if (!b->is_set[(size_t)s]) return s;
    return -1;
}
bool bank_slot_set(const qr_policy_bank* b, int slot) { return b && slot >= 0 && slot < b->capacity && b->is_set[(size_t)slot]; }
// mutable access for qr_ppo_population_load_bank (quadrace_population_prepare.hip), which packs slots on the device
half8* bank_weights_mut(qr_policy_bank* b) { return b ? b->d_weights : nullptr; }
half8* bank_weights_lo_mut(qr_policy_bank* b) { return b ? b->d_weights_lo : nullptr; }
void bank_mark_set(qr_policy_bank* b, int first_slot, int count) {
    for (int s = first_slot; s < first_slot + count && s < b->capacity; ++s)
        if (s >= 0) b->is_set[(size_t)s] = 1;
}
}  // namespace qr

namespace {
// The two packed images of one network (PolicyDims<L> layout, total_half8 half8 each) from torch.nn.Linear arrays, w[out][in], b[out]:
// what qr_policy_set_weights uploads, and what a slot of a qr_policy_bank holds.  Returns the number of half8 elements written.
size_t pack_policy_images(int L, int steps1, size_t total_half8, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, const float* b3, const float* w4, const float* b4, std::vector<__half>& img,
                          std::vector<__half>& img_lo) {
    const int H = qr::kPolHidden, BU = qr::kPolBiasUnit;
    img.assign(total_half8 * 8, __float2half(0.0f));
    img_lo.assign(total_half8 * 8, __float2half(0.0f));
    // every packed value as two f16 pieces: W0 = f16(w) (the f16-operand image), W1 = f16(w - W0) (exact difference in f32; the image
    // of the low pieces for the f32-class forward).  A weight beyond the f16 range saturates in W0 and W1 carries the rest.
    auto put = [&](size_t idx, float w) {
        float c = w;
        if (c > 65504.0f) c = 65504.0f;
        if (c < -65504.0f) c = -65504.0f;
        const __half h0 = __float2half(c);
        img[idx] = __float2half(w);   // (unchanged behaviour of the f16 image: inf beyond the range, as before)
        float r = w - __half2float(h0);
        if (r > 65504.0f) r = 65504.0f;
        if (r < -65504.0f) r = -65504.0f;
        img_lo[idx] = (w == w) ? __float2half(r) : __float2half(0.0f);
    };
    // padded weight accessors incl. the bias column and the constant-1 unit
    auto W1 = [&](int row, int k) -> float {  // row < 128, k < 16*steps1 ; input k == L is the constant 1
        if (row < H) return k < L ? w1[row * L + k] : (k == L ? b1[row] : 0.0f);
        return (row == BU && k == L) ? 1.0f : 0.0f;
    };
    auto WH = [&](const float* w, const float* b, int row, int hid) -> float {  // hidden layers: in = hidden units
        if (row < H) return hid < H ? w[row * H + hid] : (hid == BU ? b[row] : 0.0f);
        return (row == BU && hid == BU) ? 1.0f : 0.0f;
    };
    auto W4 = [&](int row, int hid) -> float {  // 4 output rows in a 32-row tile
        if (row < 4) return hid < H ? w4[row * H + hid] : (hid == BU ? b4[row] : 0.0f);
        return 0.0f;
    };
    size_t e = 0;  // half8 element index
    for (int t = 0; t < 4; ++t)
        for (int s = 0; s < steps1; ++s)
            for (int l = 0; l < 64; ++l, ++e)
                for (int j = 0; j < 8; ++j) put(e * 8 + j, W1(32 * t + (l & 31), 16 * s + 8 * (l >> 5) + j));
    for (int layer = 0; layer < 2; ++layer) {
        const float* w = layer == 0 ? w2 : w3;
        const float* b = layer == 0 ? b2 : b3;
        for (int t = 0; t < 4; ++t)
            for (int sp = 0; sp < 8; ++sp)
                for (int l = 0; l < 64; ++l, ++e)
                    for (int j = 0; j < 8; ++j) {
                        const int hid = 32 * (sp >> 1) + rho(8 * (sp & 1) + j, l >> 5);
                        put(e * 8 + j, WH(w, b, 32 * t + (l & 31), hid));
                    }
    }
    for (int sp = 0; sp < 8; ++sp)
        for (int l = 0; l < 64; ++l, ++e)
            for (int j = 0; j < 8; ++j) {
                const int hid = 32 * (sp >> 1) + rho(8 * (sp & 1) + j, l >> 5);
                put(e * 8 + j, W4(l & 31, hid));
            }
    return e;
}
}  // namespace

extern "C" {

const char* qr_policy_last_error(void) { return qr_last_error(); }  // same thread-local message as the env calls

int qr_policy_create(int32_t obs_len, int32_t device, qr_policy** out) {
    if (!out) return qr::set_last_error(QR_E_INVALID, "qr_policy_create: null output");
    *out = nullptr;
    if (!qr::dispatch_L(obs_len, [](auto) { return true; }, [] { return false; }))
        return qr::set_last_error(QR_E_INVALID, "qr_policy_create: obs_len must be an observation length of the race envs (13 + 4g, 20 + 4g) or 16 (the predecessor envs)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return qr::set_last_error(QR_E_NO_DEVICE, "qr_policy_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return qr::set_last_error(QR_E_INVALID, "qr_policy_create: bad device ordinal");
    if (hipSetDevice(device) != hipSuccess) return qr::set_last_error(QR_E_HIP, "qr_policy_create: hipSetDevice failed");
    qr_policy* p = new qr_policy();
    p->L = obs_len;
    p->device = device;
    p->steps1 = (obs_len + 1 + 15) / 16;
    p->total_half8 = (size_t)4 * p->steps1 * 64 + 2 * 4 * 8 * 64 + 8 * 64;
    if (hipMalloc((void**)&p->d_weights, p->total_half8 * 16) != hipSuccess ||
        hipMalloc((void**)&p->d_weights_lo, p->total_half8 * 16) != hipSuccess) {
        if (p->d_weights) (void)hipFree(p->d_weights);
        delete p;
        return qr::set_last_error(QR_E_HIP, "qr_policy_create: hipMalloc failed");
    }
    *out = p;
    return QR_OK;
}

int qr_policy_destroy(qr_policy* p) {
    if (!p) return QR_OK;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    if (p->d_weights) (void)hipFree(p->d_weights);
    if (p->d_weights_lo) (void)hipFree(p->d_weights_lo);
    delete p;
    return QR_OK;
}

// torch.nn.Linear layout: w[out][in], b[out]
int qr_policy_set_weights(qr_policy* p, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, const float* b3, const float* w4, const float* b4) {
    if (!p || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4)
        return qr::set_last_error(QR_E_INVALID, "qr_policy_set_weights: null argument");
    std::vector<__half> img, img_lo;
    const size_t e = pack_policy_images(p->L, p->steps1, p->total_half8, w1, b1, w2, b2, w3, b3, w4, b4, img, img_lo);
    if (e != p->total_half8) return qr::set_last_error(QR_E_STATE, "qr_policy_set_weights: internal packing size mismatch");
    if (hipSetDevice(p->device) != hipSuccess) return qr::set_last_error(QR_E_HIP, "hipSetDevice failed");
    if (hipDeviceSynchronize() != hipSuccess) return qr::set_last_error(QR_E_HIP, "hipDeviceSynchronize failed");
    if (hipMemcpy(p->d_weights, img.data(), img.size() * sizeof(__half), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_weights_lo, img_lo.data(), img_lo.size() * sizeof(__half), hipMemcpyHostToDevice) != hipSuccess)
        return qr::set_last_error(QR_E_HIP, "qr_policy_set_weights: upload failed");
    p->has_weights = true;
    return QR_OK;
}

int qr_policy_forward(qr_policy* p, int32_t n, const float* obs_dev, float* mean_out_dev, void* stream) {
    if (!p || !obs_dev || !mean_out_dev || n < 1) return qr::set_last_error(QR_E_INVALID, "qr_policy_forward: bad argument");
    if (!p->has_weights) return qr::set_last_error(QR_E_STATE, "qr_policy_forward: qr_policy_set_weights has not been called");
    hipError_t e = qr::launch_policy(p->L, p->d_weights, n, obs_dev, mean_out_dev, (hipStream_t)stream);
    if (e != hipSuccess) return qr::set_last_error(QR_E_HIP, std::string("qr_policy_forward: ") + hipGetErrorString(e));
    return QR_OK;
}

int qr_policy_forward_f32class(qr_policy* p, int32_t n, const float* obs_dev, float* mean_out_dev, void* stream) {
    if (!p || !obs_dev || !mean_out_dev || n < 1) return qr::set_last_error(QR_E_INVALID, "qr_policy_forward_f32class: bad argument");
    if (!p->has_weights) return qr::set_last_error(QR_E_STATE, "qr_policy_forward_f32class: qr_policy_set_weights has not been called");
    hipError_t e = qr::launch_policy_f32class(p->L, p->d_weights, p->d_weights_lo, n, obs_dev, mean_out_dev, (hipStream_t)stream);
    if (e != hipSuccess) return qr::set_last_error(QR_E_HIP, std::string("qr_policy_forward_f32class: ") + hipGetErrorString(e));
    return QR_OK;
}

// ---- bank of policies (qr_evaluate_policy_bank) ----
int qr_policy_bank_create(int32_t obs_len, int32_t device, int32_t capacity, qr_policy_bank** out) {
    if (!out) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_create: null output");
    *out = nullptr;
    if (!qr::dispatch_L(obs_len, [](auto) { return true; }, [] { return false; }))
        return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_create: obs_len must be an observation length of the race envs (13 + 4g, 20 + 4g) or 16 (the predecessor envs)");
    if (capacity < 1) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_create: capacity must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return qr::set_last_error(QR_E_NO_DEVICE, "qr_policy_bank_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_create: bad device ordinal");
    if (hipSetDevice(device) != hipSuccess) return qr::set_last_error(QR_E_HIP, "qr_policy_bank_create: hipSetDevice failed");
    qr_policy_bank* b = new qr_policy_bank();
    b->L = obs_len;
    b->device = device;
    b->capacity = capacity;
    b->steps1 = (obs_len + 1 + 15) / 16;
    b->total_half8 = (size_t)4 * b->steps1 * 64 + 2 * 4 * 8 * 64 + 8 * 64;
    b->is_set.assign((size_t)capacity, 0);
    const size_t bytes = (size_t)capacity * b->total_half8 * 16;
    if (hipMalloc((void**)&b->d_weights, bytes) != hipSuccess || hipMalloc((void**)&b->d_weights_lo, bytes) != hipSuccess) {
        if (b->d_weights) (void)hipFree(b->d_weights);
        delete b;
        return qr::set_last_error(QR_E_HIP, "qr_policy_bank_create: hipMalloc failed");
    }
    *out = b;
    return QR_OK;
}

int qr_policy_bank_destroy(qr_policy_bank* b) {
    if (!b) return QR_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    if (b->d_weights) (void)hipFree(b->d_weights);
    if (b->d_weights_lo) (void)hipFree(b->d_weights_lo);
    delete b;
    return QR_OK;
}

int qr_policy_bank_capacity(const qr_policy_bank* b) { return b ? b->capacity : qr::set_last_error(QR_E_INVALID, "qr_policy_bank_capacity: null bank"); }

int qr_policy_bank_set(qr_policy_bank* b, int32_t slot, const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* w3, const float* b3, const float* w4, const float* b4) {
    if (!b || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_set: null argument");
    if (slot < 0 || slot >= b->capacity) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_set: slot must be in [0, capacity)");
    std::vector<__half> img, img_lo;
    const size_t e = pack_policy_images(b->L, b->steps1, b->total_half8, w1, b1, w2, b2, w3, b3, w4, b4, img, img_lo);
    if (e != b->total_half8) return qr::set_last_error(QR_E_STATE, "qr_policy_bank_set: internal packing size mismatch");
    if (hipSetDevice(b->device) != hipSuccess) return qr::set_last_error(QR_E_HIP, "hipSetDevice failed");
    if (hipDeviceSynchronize() != hipSuccess) return qr::set_last_error(QR_E_HIP, "hipDeviceSynchronize failed");   // a launch may still read the slot
    const size_t off = (size_t)slot * b->total_half8;
    if (hipMemcpy(b->d_weights + off, img.data(), img.size() * sizeof(__half), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->d_weights_lo + off, img_lo.data(), img_lo.size() * sizeof(__half), hipMemcpyHostToDevice) != hipSuccess) {
        b->is_set[(size_t)slot] = 0;
        return qr::set_last_error(QR_E_HIP, "qr_policy_bank_set: upload failed");
    }
    b->is_set[(size_t)slot] = 1;
    return QR_OK;
}

int qr_policy_bank_read(const qr_policy_bank* b, int32_t slot, int32_t which, void* out_host, size_t bytes) {
    if (!b || !out_host) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_read: null argument");
    if (slot < 0 || slot >= b->capacity || !b->is_set[(size_t)slot]) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_read: slot must be a set slot in [0, capacity)");
    if (which < 0 || which > 1) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_read: which must be 0 (f16 image) or 1 (low pieces)");
    if (bytes != b->total_half8 * 16) return qr::set_last_error(QR_E_INVALID, "qr_policy_bank_read: bytes must be the size of one image");
    if (hipSetDevice(b->device) != hipSuccess) return qr::set_last_error(QR_E_HIP, "hipSetDevice failed");
    if (hipDeviceSynchronize() != hipSuccess) return qr::set_last_error(QR_E_HIP, "hipDeviceSynchronize failed");   // a load launch may still write the slot
    const qr::half8* src = (which == 0 ? b->d_weights : b->d_weights_lo) + (size_t)slot * b->total_half8;
    if (hipMemcpy(out_host, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return qr::set_last_error(QR_E_HIP, "qr_policy_bank_read: download failed");
    return QR_OK;
}

}  // extern "C"
