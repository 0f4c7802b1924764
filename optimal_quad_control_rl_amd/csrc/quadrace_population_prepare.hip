// quadrace_population_prepare.hip -- what lies between the collect launch (qr_rollout_policy_population) and the update launches
// (qr_ppo_population_epoch) of a population round, for ALL P members in a fixed number of launches:
//
//   qr_ppo_population_load_bank   ONE launch, grid (ceil(kTotalHalf8 / 256), P): slot first_slot + p of a policy bank <- both images of member p's
//                                 actor, packed on the device from the member's flat parameter vector.  ppo_pack_kernel's index arithmetic for
//                                 net 0 (quadrace_ppo.hip) restated, plus the low pieces with the rule of pack_policy_images (quadrace_policy.hip).
//   qr_ppo_population_prepare     FOUR launches, a member index in the grid as in ppo_grad_kernel's member mode, then one blocking copy:
//       value     population_value_kernel: policy_forward<L> with the member's VALUE image over its K E rollout rows, its E last_obs rows and
//                 (time-limit bootstrap) its K E term_obs rows, read in place from the shared [K][N][..] arrays of the collect launch; a
//                 256-row tile of term_obs without a truncation is not evaluated (term_val = 0 there)
//       gather    population_gather_kernel: the member's columns into its own contiguous buffers, done as 0 / 1 float, rows with a
//                 non-finite observation, action, log-prob, reward or value zeroed; the bad-row mask goes to scratch
//       gae       population_gae_kernel: ppo_gae_kernel (quadrace_ppo.hip) statement for statement on the sanitised buffers, adv = ret = 0 on bad
//                 rows, the running episode state, and the workgroup's partial sums of the report
//       report    population_report_kernel: per member, the workgroup partials added in index order
//
// Plain launches on the caller's stream: no graph, no atomic, no flag, and no workgroup waits for another (the kernel boundaries order the
// four steps).  The library is built with -ffp-contract=off, so the float expressions restated here round exactly as their twins do.
#include <cstring>
#include <vector>

#include "quadrace_ppo_device.hpp"

namespace qr {

constexpr int kPrepMaxMembers = 256;   // = the population object's limit (qr_ppo_population_create)
constexpr int kPrepBlock = 256;        // rows of a tile: E is a multiple, so the rows of a tile are contiguous in the shared arrays

struct PrepThetas { const float* v[kPrepMaxMembers]; };   // the members' parameter vectors travel in the kernel arguments (2 KB): no upload

__device__ __forceinline__ bool prep_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// ---- bank load: theta (net 0 block at offset 0) -> the f16 image and the image of the low pieces of slot first_slot + blockIdx.y ----------
template <int L>
__global__ void __launch_bounds__(256) population_load_bank_kernel(PrepThetas thetas, half8* __restrict__ bank, half8* __restrict__ bank_lo,
                                                                   int first_slot) {
    using P = PolicyDims<L>;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P::kTotalHalf8) return;
    const float* th = thetas.v[blockIdx.y];
    constexpr int O = 4;
    const NetOff o = net_off(L, O);
    const int lane = e & 63, c = lane & 31, h = lane >> 5;
    half8 v, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float val = 0.0f;
        if (e < P::kOff2) {  // layer 1: row = output unit, k = input index (natural order), input L = constant 1
            const int t = e / (P::kSteps1 * 64), s = (e / 64) % P::kSteps1;
            const int row = 32 * t + c, k = 16 * s + 8 * h + j;
            if (row < kH) val = k < L ? th[o.w1 + row * L + k] : (k == L ? th[o.b1 + row] : 0.0f);
            else val = (row == kPolBiasUnit && k == L) ? 1.0f : 0.0f;
        } else if (e < P::kOff4) {  // layers 2, 3: k-slots named in accumulator-row order
            const bool third = e >= P::kOff3;
            const int e2 = e - (third ? P::kOff3 : P::kOff2);
            const int t = e2 / 512, sp = (e2 / 64) % 8;
            const int row = 32 * t + c, hid = 32 * (sp >> 1) + rho_(8 * (sp & 1) + j, h);
            const int ow = third ? o.w3 : o.w2, ob = third ? o.b3 : o.b2;
            if (row < kH) val = hid < kH ? th[ow + row * kH + hid] : (hid == kPolBiasUnit ? th[ob + row] : 0.0f);
            else val = (row == kPolBiasUnit && hid == kPolBiasUnit) ? 1.0f : 0.0f;
        } else {  // output layer: rows 0..O-1 of one 32-row tile
            const int sp = (e - P::kOff4) / 64;
            const int hid = 32 * (sp >> 1) + rho_(8 * (sp & 1) + j, h);
            if (c < O) val = hid < kH ? th[o.w4 + c * kH + hid] : (hid == kPolBiasUnit ? th[o.b4 + c] : 0.0f);
        }
        v[j] = (_Float16)val;   // inf beyond the f16 range, as qr_policy_bank_set's image
        // the low piece f16(w - f16(clamp w)): saturated to the f16 range, 0 for a NaN weight (pack_policy_images' `put`)
        float cl = val;
        if (cl > 65504.0f) cl = 65504.0f;
        if (cl < -65504.0f) cl = -65504.0f;
        float r = val - (float)(_Float16)cl;
        if (r > 65504.0f) r = 65504.0f;
        if (r < -65504.0f) r = -65504.0f;
        lo[j] = (val == val) ? (_Float16)r : (_Float16)0.0f;
    }
    const size_t at = (size_t)(first_slot + (int)blockIdx.y) * P::kTotalHalf8 + (size_t)e;
    bank[at] = v;
    bank_lo[at] = lo;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------------------
struct PrepShared {   // qr_ppo_prepare_shared, as the kernels receive it
    int K, N, E;
    const float *obs, *act, *logp, *rew;
    const uint8_t *done, *trunc;
    const float *last_obs, *term_obs;
};
// One member's entry of the device-resident table (found from blockIdx.y alone)
struct PrepMember {
    int first_env;
    float gamma, lam;
    int pad_;
    const half8* image;       // the member's value image: what qr_ppo_forward(member, 1, ...) stages
    float *obs, *act, *old_logp, *rew, *done, *val, *term_val, *last_val, *adv, *ret, *ep_ret, *ep_len, *ep_gates;
    uint8_t* bad;             // [K][E] scratch: 1 = a row zeroed by the gather launch
    double* partial;          // [E / 256][8] scratch: the GAE launch's workgroup partials of the report
    double* report;           // [8]
};

// values: tiles of 256 rows; a workgroup stages its member's value image once and walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...
//   tiles [0, K c)             rollout rows (step t, chunk c of the member's E / 256)  -> val, un-sanitised (the gather launch reads it)
//   tiles [K c, K c + c)       last_obs rows                                           -> last_val = nan_to_num(V, 0, 0, 0)
//   tiles [K c + c, 2 K c + c) term_obs rows (member with term_val)                    -> term_val = trunc ? nan_to_num(V) : 0
template <int L>
__global__ void __launch_bounds__(kPrepBlock, 1) population_value_kernel(const PrepMember* __restrict__ table, PrepShared sh) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half8* W = reinterpret_cast<half8*>(smem);
    const PrepMember& M = table[blockIdx.y];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int cpe = sh.E / kPrepBlock, roll = sh.K * cpe;
    const bool with_term = sh.term_obs != nullptr && M.term_val != nullptr;
    const int total = roll + cpe + (with_term ? roll : 0);
    {
        const float4* s4 = reinterpret_cast<const float4*>(M.image);
        float4* d4 = reinterpret_cast<float4*>(W);
        for (int i = tid; i < PolicyDims<L>::kTotalHalf8; i += kPrepBlock) d4[i] = s4[i];
    }
    __syncthreads();
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
        int kind = 0, q = tile;
        if (q >= roll) { kind = 1; q -= roll; }
        if (kind == 1 && q >= cpe) { kind = 2; q -= cpe; }
        const int t = kind == 1 ? 0 : q / cpe, c = kind == 1 ? q : q % cpe;
        const size_t src = (size_t)t * sh.N + (size_t)M.first_env + (size_t)c * kPrepBlock + (size_t)tid;   // row of the shared arrays
        const size_t dst = (size_t)t * sh.E + (size_t)c * kPrepBlock + (size_t)tid;                         // row of the member's buffers
        bool tr = false;
        if (kind == 2) {
            tr = sh.trunc[src] != 0;
            if (!__syncthreads_or(tr ? 1 : 0)) {   // uniform: no time limit hit in this tile (the common case), nothing to evaluate
                M.term_val[dst] = 0.0f;
                continue;
            }
        }
        const float* row = (kind == 0 ? sh.obs : kind == 1 ? sh.last_obs : sh.term_obs) + src * L;
        float o[L];
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
        float mean[4];
        policy_forward<L>(W, lane, o, mean);
        const float v = mean[0];
        if (kind == 0) M.val[dst] = v;
        else if (kind == 1) M.last_val[dst] = prep_finite(v) ? v : 0.0f;
        else M.term_val[dst] = (tr && prep_finite(v)) ? v : 0.0f;
    }
}

// gather + sanitise: one tile = 256 rows of one step; the observations move as 256 L contiguous floats (element i of the tile belongs to
// row i / L), the per-row scalars by the row's own thread
template <int L>
__global__ void __launch_bounds__(kPrepBlock) population_gather_kernel(const PrepMember* __restrict__ table, PrepShared sh) {
    __shared__ int badrow[kPrepBlock];
    const PrepMember& M = table[blockIdx.y];
    const int tid = (int)threadIdx.x;
    const int cpe = sh.E / kPrepBlock, tiles = sh.K * cpe;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int t = tile / cpe, c = tile % cpe;
        const size_t src0 = (size_t)t * sh.N + (size_t)M.first_env + (size_t)c * kPrepBlock;
        const size_t dst0 = (size_t)t * sh.E + (size_t)c * kPrepBlock;
        badrow[tid] = 0;
        __syncthreads();
        const float* so = sh.obs + src0 * L;
        float x[L];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            x[k] = so[k * kPrepBlock + tid];
            if (!prep_finite(x[k])) badrow[(k * kPrepBlock + tid) / L] = 1;   // every writer stores the same value
        }
        const float4 a = reinterpret_cast<const float4*>(sh.act)[src0 + tid];
        const float lp = sh.logp[src0 + tid], r = sh.rew[src0 + tid], v = M.val[dst0 + tid];
        const uint8_t d = sh.done[src0 + tid];
        if (!(prep_finite(a.x) && prep_finite(a.y) && prep_finite(a.z) && prep_finite(a.w) && prep_finite(lp) && prep_finite(r) && prep_finite(v)))
            badrow[tid] = 1;
        __syncthreads();
        float* dobs = M.obs + dst0 * L;
#pragma unroll
        for (int k = 0; k < L; ++k) dobs[k * kPrepBlock + tid] = badrow[(k * kPrepBlock + tid) / L] ? 0.0f : x[k];
        const bool bad = badrow[tid] != 0;
        reinterpret_cast<float4*>(M.act)[dst0 + tid] = bad ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : a;
        M.old_logp[dst0 + tid] = bad ? 0.0f : lp;
        M.rew[dst0 + tid] = bad ? 0.0f : r;
        M.val[dst0 + tid] = bad ? 0.0f : v;
        M.done[dst0 + tid] = (float)d;
        M.bad[dst0 + tid] = bad ? 1 : 0;
        __syncthreads();   // badrow is reset at the top of the next tile
    }
}

// GAE(lambda) + episode state: ppo_gae_kernel with T = K, N = E and the member's buffers; one lane = one env.  The report's terms are formed
// as floats (the twin's expressions) and added in double: lane over t ascending, wave_sum_f64, the four waves in order.
__global__ void __launch_bounds__(kPrepBlock) population_gae_kernel(const PrepMember* __restrict__ table, PrepShared sh) {
    __shared__ double red[8][kPrepBlock / 64];
    const PrepMember& M = table[blockIdx.y];
    const int T = sh.K, N = sh.E;
    const int i = blockIdx.x * kPrepBlock + threadIdx.x;   // < E: the grid is E / 256 workgroups
    const float gamma = M.gamma, lam = M.lam;
    const float *rew = M.rew, *done = M.done, *val = M.val, *term_val = M.term_val;
    const uint8_t* bad = M.bad;
    float *adv = M.adv, *ret = M.ret;
    {
        float last = 0.0f, next_val = M.last_val[i];
        for (int t = T - 1; t >= 0; --t) {
            const size_t e = (size_t)t * N + i;
            const float nonterminal = 1.0f - done[e], v = val[e];
            const float r = term_val ? fmaf(gamma, term_val[e], rew[e]) : rew[e];
            const float delta = r + gamma * next_val * nonterminal - v;
            last = delta + gamma * lam * nonterminal * last;
            const bool b = bad[e] != 0;
            adv[e] = b ? 0.0f : last;
            ret[e] = b ? 0.0f : last + v;
            next_val = v;
        }
    }
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // bad rows, truncations, f0, f1, f2, f3, sum reward, -
    {
        const bool with_ep = M.ep_ret != nullptr;
        float er = with_ep ? M.ep_ret[i] : 0.0f, el = with_ep ? M.ep_len[i] : 0.0f, eg = with_ep ? M.ep_gates[i] : 0.0f;
        const uint8_t* trunc = sh.trunc + (size_t)M.first_env + i;
        for (int t = 0; t < T; ++t) {
            const size_t e = (size_t)t * N + i;
            const float r = rew[e], d = done[e];
            s[0] += bad[e] ? 1.0 : 0.0;
            s[1] += trunc[(size_t)t * sh.N] ? 1.0 : 0.0;
            s[6] += (double)r;
            if (with_ep) {
                er += r;
                el += 1.0f;
                eg += r > 5.0f ? 1.0f : 0.0f;  // gate reward 10 - 10 * d2g (R:537)
                const float f0 = er * d, f1 = el * d, f2 = eg * d;
                s[2] += (double)f0; s[3] += (double)f1; s[4] += (double)f2; s[5] += (double)d;
                const float keep = 1.0f - d;
                er *= keep; el *= keep; eg *= keep;
            }
        }
        if (with_ep) { M.ep_ret[i] = er; M.ep_len[i] = el; M.ep_gates[i] = eg; }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const double w = wave_sum_f64(s[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double w = 0.0;
#pragma unroll
        for (int k = 0; k < kPrepBlock / 64; ++k) w += red[threadIdx.x][k];
        M.partial[(size_t)blockIdx.x * 8 + threadIdx.x] = w;
    }
}

// report[p][q] = the member's workgroup partials added in index order
__global__ void __launch_bounds__(64) population_report_kernel(const PrepMember* __restrict__ table, int wgs) {
    const PrepMember& M = table[blockIdx.x];
    if (threadIdx.x < 8) {
        double w = 0.0;
        for (int k = 0; k < wgs; ++k) w += M.partial[(size_t)k * 8 + threadIdx.x];
        M.report[threadIdx.x] = w;
    }
}

// what the population object keeps for qr_ppo_population_prepare
struct PrepState {
    PrepMember* d_table = nullptr;
    std::vector<PrepMember> h_table;   // what d_table holds (and the source of its upload)
    bool table_valid = false;
    uint8_t* d_bad = nullptr;          // [P][K E]
    size_t bad_rows = 0;               // rows per member d_bad was allocated for
    double* d_partial = nullptr;       // [P][E / 256][8]
    size_t partial_wgs = 0;            // workgroups per member d_partial was allocated for
    double* d_report = nullptr;        // [P][8]
};

void population_prepare_release(void* state) {
    PrepState* s = static_cast<PrepState*>(state);
    if (!s) return;
    (void)hipFree(s->d_table);
    (void)hipFree(s->d_bad);
    (void)hipFree(s->d_partial);
    (void)hipFree(s->d_report);
    delete s;
}

}  // namespace qr

namespace {

template <typename F>
int dispatch_L(int L, F&& f) {
    return qr::dispatch_L(L, f, [] { return qr::set_last_error(QR_E_INVALID, "qr_ppo_population: the members' obs_len is not an observation length of the envs"); });
}

bool finite_host(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return (u & 0x7F800000u) != 0x7F800000u;
}

}  // namespace

namespace qr {
// the ONE launch of population_load_bank_kernel, for qr_ppo_population_load_bank and for qr_es_perturb (quadrace_es.hip), which points the
// table at the rows of its population matrix: slot first_slot + p <- both images of the actor block at theta[p], p < P <= kPrepMaxMembers.
// The caller has checked the bank and made its device current.  Returns a QR_* code (qr_last_error set).
int launch_population_load_bank(int L, const float* const* theta, int P, half8* bank, half8* bank_lo, int first_slot, hipStream_t st) {
    if (P < 1 || P > kPrepMaxMembers) return set_last_error(QR_E_INVALID, "the bank load takes 1..256 parameter vectors per launch");
    PrepThetas thetas;
    std::memset(&thetas, 0, sizeof(thetas));
    for (int p = 0; p < P; ++p) thetas.v[p] = theta[p];
    return ::dispatch_L(L, [&](auto Lc) {   // this file's failure message
        constexpr int kL = decltype(Lc)::value;
        static_assert(PpoDims<kL>::kImage == PolicyDims<kL>::kTotalHalf8, "the updater's actor image has the layout of a bank slot");
        hipLaunchKernelGGL(population_load_bank_kernel<kL>, dim3((PolicyDims<kL>::kTotalHalf8 + 255) / 256, P), dim3(256), 0, st, thetas, bank, bank_lo,
                           first_slot);
        QR_HIP(hipGetLastError());
        return (int)QR_OK;
    });
}
}  // namespace qr

extern "C" {

int qr_ppo_population_load_bank(qr_ppo_population* pop, const float* const* theta_dev, qr_policy_bank* bank, int32_t first_slot, void* stream) {
    if (!pop || !theta_dev || !bank) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_load_bank: null argument");
    const int P = qr::population_size(pop);
    for (int p = 0; p < P; ++p)
        if (!theta_dev[p]) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_load_bank: a member's theta_dev is null");
    if (qr::bank_obs_len(bank) != qr::population_obs_len(pop) || qr::bank_device(bank) != qr::population_device(pop))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_load_bank: the bank's obs_len or device differs from the population's");
    if (first_slot < 0 || (long long)first_slot + P > (long long)qr::bank_capacity(bank))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_load_bank: slots [first_slot, first_slot + members) must lie in [0, capacity)");
    QR_HIP(hipSetDevice(qr::population_device(pop)));
    const int rc = qr::launch_population_load_bank(qr::population_obs_len(pop), theta_dev, P, qr::bank_weights_mut(bank), qr::bank_weights_lo_mut(bank),
                                                   (int)first_slot, (hipStream_t)stream);
    if (rc != QR_OK) return rc;
    qr::bank_mark_set(bank, first_slot, P);
    return QR_OK;
}

int qr_ppo_population_prepare(qr_ppo_population* pop, const qr_ppo_prepare_shared* sh, const qr_ppo_prepare_member* members, double* report_host,
                              void* stream) {
    if (!pop || !sh || !members || !report_host) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: null argument");
    const int P = qr::population_size(pop);
    const int K = sh->K, N = sh->N, E = sh->E;
    if (K < 1) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: K must be >= 1");
    if (E < 256 || E % 256 != 0 || N < E || N % E != 0)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: E must be a multiple of 256 (>= 256) and N a multiple of E");
    if (!sh->obs || !sh->act || !sh->logp || !sh->rew || !sh->done || !sh->trunc || !sh->last_obs)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: a shared array other than term_obs is null");
    if ((unsigned long long)K * (unsigned long long)N > 0x7FFFFFFFull)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: K * N is beyond 2^31 - 1 rows");
    for (int p = 0; p < P; ++p) {
        const qr_ppo_prepare_member& m = members[p];
        if (m.first_env < 0 || m.first_env >= N || m.first_env % E != 0)
            return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: first_env must be a multiple of E inside [0, N)");
        for (int q = 0; q < p; ++q)
            if (members[q].first_env == m.first_env) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: two members share a first_env");
        if (!m.obs || !m.act || !m.old_logp || !m.rew || !m.done || !m.val || !m.last_val || !m.adv || !m.ret)
            return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: a member's buffer other than term_val / ep_* is null");
        const int eps = (m.ep_ret ? 1 : 0) + (m.ep_len ? 1 : 0) + (m.ep_gates ? 1 : 0);
        if (eps != 0 && eps != 3) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: episode state needs all three arrays");
        if (m.term_val && !sh->term_obs) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: term_val needs the shared term_obs");
        if (!finite_host(m.gamma) || !finite_host(m.lam)) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: gamma / lam must be finite");
    }
    QR_HIP(hipSetDevice(qr::population_device(pop)));
    hipStream_t st = (hipStream_t)stream;
    if (qr::stream_is_capturing(st))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_prepare: `stream` is being captured (the call allocates, uploads the member table and blocks on its report)");
    // the object's scratch: allocated on first use, regrown when (K, E) ask for more
    void*& slot = qr::population_prepare_slot(pop);
    if (!slot) slot = new qr::PrepState();
    qr::PrepState* S = static_cast<qr::PrepState*>(slot);
    const size_t rows = (size_t)K * (size_t)E, wgs = (size_t)(E / 256);
    if (!S->d_table) QR_HIP(hipMalloc((void**)&S->d_table, sizeof(qr::PrepMember) * (size_t)P));
    if (!S->d_report) QR_HIP(hipMalloc((void**)&S->d_report, sizeof(double) * 8 * (size_t)P));
    if (rows > S->bad_rows) {
        QR_HIP(hipStreamSynchronize(st));   // an earlier call's launches may still use the old block
        if (S->d_bad) { (void)hipFree(S->d_bad); S->d_bad = nullptr; S->bad_rows = 0; }
        QR_HIP(hipMalloc((void**)&S->d_bad, rows * (size_t)P));
        S->bad_rows = rows;
    }
    if (wgs > S->partial_wgs) {
        QR_HIP(hipStreamSynchronize(st));
        if (S->d_partial) { (void)hipFree(S->d_partial); S->d_partial = nullptr; S->partial_wgs = 0; }
        QR_HIP(hipMalloc((void**)&S->d_partial, sizeof(double) * 8 * wgs * (size_t)P));
        S->partial_wgs = wgs;
    }
    std::vector<qr::PrepMember> table((size_t)P);
    std::memset(table.data(), 0, sizeof(qr::PrepMember) * (size_t)P);   // padding included: the table is compared bytewise below
    for (int p = 0; p < P; ++p) {
        const qr_ppo_prepare_member& m = members[p];
        const qr_ppo* h = qr::population_member(pop, p);
        qr::PrepMember& d = table[(size_t)p];
        d.first_env = m.first_env; d.gamma = m.gamma; d.lam = m.lam;
        d.image = h->d_images + (size_t)h->image_half8;
        d.obs = m.obs; d.act = m.act; d.old_logp = m.old_logp; d.rew = m.rew; d.done = m.done; d.val = m.val;
        d.term_val = m.term_val; d.last_val = m.last_val; d.adv = m.adv; d.ret = m.ret;
        d.ep_ret = m.ep_ret; d.ep_len = m.ep_len; d.ep_gates = m.ep_gates;
        d.bad = S->d_bad + (size_t)p * S->bad_rows;
        d.partial = S->d_partial + (size_t)p * S->partial_wgs * 8;
        d.report = S->d_report + (size_t)p * 8;
    }
    if (!(S->table_valid && std::memcmp(table.data(), S->h_table.data(), sizeof(qr::PrepMember) * (size_t)P) == 0)) {
        // stream-ordered behind whatever earlier calls left on `st`; h_table stays untouched until this call's closing synchronisation
        S->h_table = table;
        S->table_valid = false;
        QR_HIP(hipMemcpyAsync(S->d_table, S->h_table.data(), sizeof(qr::PrepMember) * (size_t)P, hipMemcpyHostToDevice, st));
        S->table_valid = true;
    }
    qr::PrepShared s;
    s.K = K; s.N = N; s.E = E;
    s.obs = sh->obs; s.act = sh->act; s.logp = sh->logp; s.rew = sh->rew; s.done = sh->done; s.trunc = sh->trunc;
    s.last_obs = sh->last_obs; s.term_obs = sh->term_obs;
    const int cpe = E / 256;
    const long long roll = (long long)K * cpe, vtiles = 2 * roll + cpe;
    const int spread = 1024 / P > 1 ? 1024 / P : 1;   // workgroups per member: enough to fill the GPU, few enough to amortise the image staging
    const int vgrid = (int)(vtiles < spread ? vtiles : spread), ggrid = (int)(roll < 4 * spread ? roll : 4 * spread);
    const int rc = dispatch_L(qr::population_obs_len(pop), [&](auto Lc) {
        constexpr int L = decltype(Lc)::value;
        QR_HIP((qr::launch_dynamic_lds<qr::population_value_kernel<L>>(dim3(vgrid, P), dim3(qr::kPrepBlock), (size_t)qr::PolicyDims<L>::kTotalHalf8 * 16, st,
                                                                         (const qr::PrepMember*)S->d_table, s)));
        hipLaunchKernelGGL(qr::population_gather_kernel<L>, dim3(ggrid, P), dim3(qr::kPrepBlock), 0, st, (const qr::PrepMember*)S->d_table, s);
        return (int)QR_OK;
    });
    if (rc != QR_OK) return rc;
    hipLaunchKernelGGL(qr::population_gae_kernel, dim3(cpe, P), dim3(qr::kPrepBlock), 0, st, (const qr::PrepMember*)S->d_table, s);
    hipLaunchKernelGGL(qr::population_report_kernel, dim3(P), dim3(64), 0, st, (const qr::PrepMember*)S->d_table, cpe);
    QR_HIP(hipGetLastError());
    QR_HIP(hipMemcpyAsync(report_host, S->d_report, sizeof(double) * 8 * (size_t)P, hipMemcpyDeviceToHost, st));
    QR_HIP(hipStreamSynchronize(st));   // the round's one blocking read
    return QR_OK;
}

}  // extern "C"
