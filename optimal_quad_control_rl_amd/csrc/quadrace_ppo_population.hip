// quadrace_ppo_population.hip -- the PPO minibatch update of a POPULATION of learners: one minibatch of all P members is THREE launches
// (qr_ppo_population_epoch), where P handles driven by qr_ppo_epoch one after another take 2 P.
//
// Why kernels of its own: ppo_apply_kernel (quadrace_ppo.hip) spins on a grid-wide barrier that relies on all of its workgroups being
// resident; several of them in flight, or one beside gradient workgroups that own a CU each, break that assumption, and P x 247 workgroups
// do not fit under one barrier.  Here NO kernel waits for another workgroup: the apply kernel is cut in two at its barrier and the
// kernel boundary takes the barrier's place.  No spin, no flag, no atomic, no cooperative launch; PpoCtrl::arrive / go / gen /
// barrier_timeouts of the members are never touched.
//
//   grad     ppo_grad_kernel in member mode, grid (wgs, 2, P): the gradient kernel's work for every member at once.  A workgroup reads ITS
//            member's entry of a device-resident table (PopMember; the address derives from blockIdx alone: scalar loads, and what the
//            twin holds in kernel-argument registers sits in the same kind of register here); the minibatch index k is a launch argument:
//            idx = perm + k B, acc = mbstats + 2 k.  Partials and per-wave sums go to the member's own qr_ppo buffers.
//   reduce   ppo_population_reduce_kernel, grid (247, P): the first half of ppo_apply_kernel -- DenseMap thread -> parameter, reduce_grad_element,
//            block_sum2_f64 of g^2 -- writing the gradient element, the workgroup's squared sum (the float the barrier word carries in
//            the twin) and the last block's minibatch statistics to the member's scratch area, plus a snapshot of PpoCtrl::stop / adam_t
//            as they stood BEFORE this minibatch (the step kernel's last block rewrites them while its other blocks still start).
//   step     ppo_population_step_kernel, grid (247, P): the second half.  EVERY workgroup adds its member's squared sums in the barrier
//            master's order (lane q over slots q, q + 64, ... in double, then wave_sum_f64), takes the same target-KL and finiteness verdicts,
//            the same clip and torch.optim.Adam expressions with the member's device-resident adam_t and lr, and scatters the f16 copies
//            into the member's images; the last block does the master's bookkeeping under the same conditions.
//
// The gradient kernel and PopMember live in quadrace_ppo_device.hpp: ONE template, ppo_grad_kernel<L, PT, kMember>.  Member mode changes
// its first statements only: the minibatch and the partial come from table[blockIdx.z] at minibatch k instead of the kernel arguments.
// The per-epoch launches (shuffle, table zeroing, advantage sums) are the existing kernels, issued once per member (qr::ppo_epoch_prologue).
#include <cstring>
#include <vector>

#include "quadrace_ppo_device.hpp"

namespace qr {

constexpr int kMaxPopulation = 256;
struct PopLr { float v[kMaxPopulation]; };

// PpoCtrl::lr of every member <- the call's values: they travel in the kernel arguments (see ppo_set_lr_kernel), so a learning-rate
// schedule does not force a re-capture
__global__ void __launch_bounds__(kMaxPopulation) ppo_population_lr_kernel(const PopMember* __restrict__ table, int num_members, PopLr lr) {
    const int p = (int)threadIdx.x;
    if (p < num_members) table[p].ctrl->lr = lr.v[p];
}

// thread j of a member's reduce / step grid -> its parameter i (n: none) and its column pj in the partial table: ppo_apply_kernel's map
// for accumulator-order partials
template <int L>
__device__ __forceinline__ void population_thread_map(int j, int n, int& i, int& pj, bool& slot_thread) {
    using DM = DenseMap<L>;
    constexpr int S = PpoDims<L>::kRawSlots, T = DM::kDenseThreads;
    const int n4 = net_off(L, 4).total;
    int p = -1;
    pj = 0;
    if (j < T) { DM::map(j, 4, pj, p); i = p < 0 ? n : p; }
    else if (j < 2 * T) { DM::map(j - T, 1, pj, p); pj += S; i = p < 0 ? n : n4 + p; }
    else i = j - 2 * T < 4 ? n - 4 + (j - 2 * T) : n;
    slot_thread = j < 2 * T;
}

// chunks = workgroups per net of the gradient launch, Gw = chain waves per net (2 G): the same for every member
template <int L>
__global__ void __launch_bounds__(kApplyThreads, 2) ppo_population_reduce_kernel(const PopMember* __restrict__ table, int chunks, int Gw, int partial_bf16) {
    const PopMember& M = table[blockIdx.y];
    const PpoCtrl* c = M.ctrl;
    const int stop_flag = c->stop;       // set by an EARLIER launch: uniform over the member's workgroups
    const int adam_t = c->adam_t;
    const bool last_block = blockIdx.x == gridDim.x - 1;
    if (last_block && threadIdx.x == 0) {   // as they stand before this minibatch: the step launch's last block rewrites the originals
        int* snap = reinterpret_cast<int*>(M.mb + 4);
        snap[0] = stop_flag;
        snap[1] = adam_t;
    }
    if (stop_flag) return;  // SB3: no update after the early stop (and nothing is accumulated)
    ApplyArgs a{};
    a.n = ppo_num_params(L);
    a.partial = reinterpret_cast<const float*>(M.partial);
    a.partial_bf16 = partial_bf16;
    a.partial_raw = 2 * PpoDims<L>::kRawSlots;
    a.owner_from = 2 * DenseMap<L>::kDenseThreads;
    a.chunks = chunks;
    a.wave_out = M.b.wave_out;
    a.Gw = Gw;
    a.ent_coef = M.b.ent_coef;
    const int n = a.n;
    const int j = blockIdx.x * kApplyThreads + threadIdx.x;
    int i, pj;
    bool slot_thread;
    population_thread_map<L>(j, n, i, pj, slot_thread);
    __shared__ float red[8];
    const float g = reduce_grad_element(a, i, pj, slot_thread, red);
    M.grad[j] = g;
    double sq = (double)g * g, unused = 0.0;
    block_sum2_f64<kApplyThreads>(sq, unused);
    if (threadIdx.x == 0) M.sq[blockIdx.x] = (float)sq;   // the float the twin's barrier word carries
    if (last_block && threadIdx.x < 4) M.mb[threadIdx.x] = red[4 + threadIdx.x];
}

template <int L>
__global__ void __launch_bounds__(kApplyThreads, 2) ppo_population_step_kernel(const PopMember* __restrict__ table) {
    const PopMember& M = table[blockIdx.y];
    PpoCtrl* c = M.ctrl;
    const int* snap = reinterpret_cast<const int*>(M.mb + 4);
    if (snap[0]) return;                 // stopped by an earlier minibatch: the reduce launch wrote nothing else
    const int adam_t = snap[1];
    const float lr_dev = c->lr;
    const int n = ppo_num_params(L);
    const int j = blockIdx.x * kApplyThreads + threadIdx.x;
    int i, pj;
    bool slot_thread;
    population_thread_map<L>(j, n, i, pj, slot_thread);
    const bool last_block = blockIdx.x == gridDim.x - 1;
    const bool owns = i < n;
    const float m_in = owns ? M.m[i] : 0.0f, v_in = owns ? M.v[i] : 0.0f, th_in = owns ? M.theta[i] : 0.0f;
    const float g = M.grad[j];
    // the squared norm: every workgroup forms it itself, in the order of the twin's barrier master
    __shared__ float nsq_s;
    if (threadIdx.x < 64) {
        double total = 0.0;
        for (int q = threadIdx.x; q < (int)gridDim.x; q += 64) total += (double)M.sq[q];
        total = wave_sum_f64(total);
        if (threadIdx.x == 0) nsq_s = (float)total;
    }
    __syncthreads();
    const float norm_sq = nsq_s;
    const float kl_sum = M.mb[2];
    const bool stop_now = M.kl_limit > 0.0f && kl_sum > M.kl_limit;   // SB3: checked BEFORE the optimiser step of this minibatch
    const bool finite = norm_sq <= 3.0e38f;                           // false for inf and NaN
    if (!stop_now && finite && i < n) {
        const float norm = sqrtf(norm_sq);
        const float clip = fminf(1.0f, M.max_norm / (norm + 1e-6f));  // torch.nn.utils.clip_grad_norm_
        const float gc = g * clip;
        const float mi = M.beta1 * m_in + (1.0f - M.beta1) * gc;
        const float vi = M.beta2 * v_in + (1.0f - M.beta2) * gc * gc;
        M.m[i] = mi;
        M.v[i] = vi;
        const float bc1 = 1.0f - powf(M.beta1, (float)(adam_t + 1));
        const float bc2_sqrt = sqrtf(1.0f - powf(M.beta2, (float)(adam_t + 1)));
        const float lr = lr_dev;
        const float th = th_in - (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + M.eps);  // torch.optim.Adam
        M.theta[i] = th;
        const int n4 = net_off(L, 4).total, n1 = net_off(L, 1).total;
        half8* images = const_cast<half8*>(M.b.images);
        if (i < n4) pack_scatter<L>(reinterpret_cast<_Float16*>(images), 4, i, th);
        else if (i < n4 + n1) pack_scatter<L>(reinterpret_cast<_Float16*>(images + PpoDims<L>::kImage), 1, i - n4, th);
    }
    if (last_block && threadIdx.x == 0) {
        if (M.b.stats)
            for (int q = 0; q < 4; ++q) M.b.stats[q] += M.mb[q];
        if (stop_now) c->stop = 1;
        else if (finite) { c->applied += 1; c->adam_t = adam_t + 1; }
        else c->skipped_nonfinite += 1;
    }
}

// ---- exploit: destination members become copies of source members (qr_ppo_population_exploit) ----------------------------------------
// What a member is to this kernel: device-resident, one entry per member, uploaded when a pointer moves.  What a CALL says -- which
// members are overwritten, from whom, with which log_std shift -- is 2 KB and rides in the kernel arguments like PopLr.
struct ExploitMember {
    float *theta, *m, *v;
    half8* images;            // [2][kImage]
    PpoCtrl* ctrl;
};
struct ExploitPlan {          // entry d of the launch's grid.y: member dst[d] <- member src[d], log_std + shift[d]
    unsigned char dst[kMaxPopulation], src[kMaxPopulation];
    float shift[kMaxPopulation];
};
constexpr int kExploitThreads = 256;

// grid (ceil(n / 256), destinations).  Thread e copies parameter e (theta with the shift added to the four log_std entries, both Adam
// moments) and, below 2 kImage, gathers half8 element e of the destination's images from the SOURCE's theta -- ppo_pack_kernel's element,
// so the images are what qr_ppo_pack makes of the new vector (log_std is in no image, and a source is never a destination: nothing this
// launch reads is written by it).  The last block copies the Adam step count.  Nothing waits for anything.
template <int L>
__global__ void __launch_bounds__(kExploitThreads) ppo_population_exploit_kernel(const ExploitMember* __restrict__ table, ExploitPlan plan) {
    const ExploitMember& D = table[plan.dst[blockIdx.y]];
    const ExploitMember& S = table[plan.src[blockIdx.y]];
    const float shift = plan.shift[blockIdx.y];
    const int n = ppo_num_params(L);
    const int e = blockIdx.x * kExploitThreads + threadIdx.x;
    if (e < n) {
        const float th = S.theta[e];
        D.theta[e] = e >= n - 4 ? th + shift : th;
        D.m[e] = S.m[e];
        D.v[e] = S.v[e];
    }
    constexpr int kImage = PpoDims<L>::kImage;
    if (e < 2 * kImage) {
        const int net = e >= kImage ? 1 : 0;
        D.images[e] = pack_gather<L>(S.theta, net, e - net * kImage);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) D.ctrl->adam_t = S.ctrl->adam_t;
}

}  // namespace qr

// ------------------------------------------------------------------------------------------------------------------------
struct qr_ppo_population {
    std::vector<qr_ppo*> members;   // borrowed
    int L = 0, device = 0;
    bool partial_bf16 = true, epoch_graph = true;
    int workgroups = 0;             // of one member in the reduce / step launches
    qr::PopMember* d_table = nullptr;
    float* d_scratch = nullptr;     // [members][scratch_floats]: grad | sq | mb
    size_t scratch_floats = 0;
    // what d_table holds and what the cached graph was captured for
    std::vector<qr::PopMember> h_table;
    bool table_valid = false;
    hipGraphExec_t exec = nullptr;
    std::vector<unsigned long long> g_seeds;
    int g_B = 0, g_M = 0, g_E = 0, g_shuffle = 0;
    hipStream_t capture_stream = nullptr;
    void* prepare = nullptr;        // what qr_ppo_population_prepare owns (quadrace_population_prepare.hip), released with the object
    // qr_ppo_population_exploit: the members as its kernel sees them, allocated on first use
    qr::ExploitMember* d_exploit = nullptr;
    std::vector<qr::ExploitMember> h_exploit;
    bool exploit_valid = false;
};

namespace qr {   // what quadrace_population_prepare.hip needs of the object
int population_size(const qr_ppo_population* pop) { return pop ? (int)pop->members.size() : 0; }
int population_obs_len(const qr_ppo_population* pop) { return pop ? pop->L : -1; }
int population_device(const qr_ppo_population* pop) { return pop ? pop->device : -1; }
qr_ppo* population_member(const qr_ppo_population* pop, int p) { return pop->members[(size_t)p]; }
void*& population_prepare_slot(qr_ppo_population* pop) { return pop->prepare; }
}  // namespace qr

namespace {

template <typename F>
int dispatch_L(int L, F&& f) {
    return qr::dispatch_L(L, f, [] { return qr::set_last_error(QR_E_INVALID, "qr_ppo_population: the members' obs_len is not an observation length of the envs"); });
}

template <int L>
struct PopOps {
    using D = qr::PpoDims<L>;
    static constexpr size_t kLdsFused = ((size_t)D::kImage + qr::kExHalf8) * 16 + 7 * qr::kStashRows * sizeof(float);   // = PpoOps<L>::kLdsFused
    static constexpr int kThreads = 2 * qr::DenseMap<L>::kDenseThreads + 4;
    static constexpr int kWorkgroups = (kThreads + qr::kApplyThreads - 1) / qr::kApplyThreads;
    static int configure(const qr_ppo_population* pop) {
        if (pop->partial_bf16) QR_HIP((qr::configure_dynamic_lds<qr::ppo_grad_kernel<L, __bf16, true>>(kLdsFused)));
        else QR_HIP((qr::configure_dynamic_lds<qr::ppo_grad_kernel<L, float, true>>(kLdsFused)));
        return QR_OK;
    }
    // minibatch k of every member: three launches
    static int minibatch(const qr_ppo_population* pop, int B, int k, hipStream_t st) {
        const int P = (int)pop->members.size();
        const int G = (B + 63) / 64, pairs = (G + 1) / 2;
        const int wgs = pairs < qr_ppo::kFusedChunks ? pairs : qr_ppo::kFusedChunks;
        const qr::PopMember* table = pop->d_table;   // member mode: the minibatch and the partial argument are passed empty
        if (pop->partial_bf16)
            hipLaunchKernelGGL((qr::ppo_grad_kernel<L, __bf16, true>), dim3(wgs, 2, P), dim3(512), kLdsFused, st, qr::PpoBatch{},
                               static_cast<__bf16*>(nullptr), table, k, static_cast<const float*>(nullptr));
        else
            hipLaunchKernelGGL((qr::ppo_grad_kernel<L, float, true>), dim3(wgs, 2, P), dim3(512), kLdsFused, st, qr::PpoBatch{},
                               static_cast<float*>(nullptr), table, k, static_cast<const float*>(nullptr));
        hipLaunchKernelGGL(qr::ppo_population_reduce_kernel<L>, dim3(kWorkgroups, P), dim3(qr::kApplyThreads), 0, st, pop->d_table, wgs, 2 * G,
                           pop->partial_bf16 ? 1 : 0);
        hipLaunchKernelGGL(qr::ppo_population_step_kernel<L>, dim3(kWorkgroups, P), dim3(qr::kApplyThreads), 0, st, pop->d_table);
        QR_HIP(hipGetLastError());
        return QR_OK;
    }
};

}  // namespace

extern "C" {

int qr_ppo_population_create(qr_ppo* const* members, int32_t num_members, qr_ppo_population** out) {
    if (!out) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_create: null output");
    *out = nullptr;
    if (!members || num_members < 1 || num_members > qr::kMaxPopulation)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_create: num_members must be 1..256 and members non-null");
    for (int p = 0; p < num_members; ++p) {
        if (!members[p]) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_create: null member handle");
        for (int q = 0; q < p; ++q)
            if (members[q] == members[p]) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_create: a handle is listed twice");
        const qr_ppo *a = members[0], *b = members[p];
        if (a->L != b->L || a->device != b->device || a->partial_bf16 != b->partial_bf16 || a->epoch_graph != b->epoch_graph)
            return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_create: the members must share obs_len, device and flags");
    }
    qr_ppo_population* pop = new qr_ppo_population();
    pop->members.assign(members, members + num_members);
    pop->L = members[0]->L;
    pop->device = members[0]->device;
    pop->partial_bf16 = members[0]->partial_bf16;
    pop->epoch_graph = members[0]->epoch_graph;
    const int rc = dispatch_L(pop->L, [&](auto Lc) {
        pop->workgroups = PopOps<decltype(Lc)::value>::kWorkgroups;
        return (int)QR_OK;
    });
    if (rc != QR_OK) { delete pop; return rc; }
    pop->scratch_floats = (size_t)pop->workgroups * qr::kApplyThreads + (size_t)((pop->workgroups + 63) / 64 * 64) + 8;
    hipError_t e = hipSetDevice(pop->device);
    if (e == hipSuccess) e = hipMalloc((void**)&pop->d_table, sizeof(qr::PopMember) * (size_t)num_members);
    if (e == hipSuccess) e = hipMalloc((void**)&pop->d_scratch, sizeof(float) * pop->scratch_floats * (size_t)num_members);
    if (e == hipSuccess) e = hipMemset(pop->d_scratch, 0, sizeof(float) * pop->scratch_floats * (size_t)num_members);
    if (e != hipSuccess) {
        qr_ppo_population_destroy(pop);
        return qr::set_last_error(QR_E_HIP, std::string("qr_ppo_population_create: ") + hipGetErrorString(e));
    }
    *out = pop;
    return QR_OK;
}

int qr_ppo_population_destroy(qr_ppo_population* pop) {
    if (!pop) return QR_OK;
    (void)hipSetDevice(pop->device);
    (void)hipDeviceSynchronize();
    if (pop->exec) (void)hipGraphExecDestroy(pop->exec);
    if (pop->capture_stream) (void)hipStreamDestroy(pop->capture_stream);
    (void)hipFree(pop->d_table);
    (void)hipFree(pop->d_scratch);
    (void)hipFree(pop->d_exploit);
    qr::population_prepare_release(pop->prepare);
    delete pop;
    return QR_OK;
}

int qr_ppo_population_epoch(qr_ppo_population* pop, const qr_ppo_member_args* args, int32_t B, int32_t num_minibatches, int32_t num_epochs,
                            int32_t device_shuffle, void* stream) {
    if (!pop || !args) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_epoch: null argument");
    const int P = (int)pop->members.size();
    if (B < 64 || num_minibatches < 1 || num_minibatches > qr_ppo::kMaxEpochMinibatches)
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_epoch: bad minibatch size / count");
    if (num_epochs < 1 || num_epochs > 64 || (num_epochs > 1 && !device_shuffle))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_epoch: num_epochs > 1 needs device_shuffle (the caller cannot rewrite the permutations in between)");
    for (int p = 0; p < P; ++p) {
        const qr_ppo_member_args& a = args[p];
        if (B > pop->members[p]->max_B) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_epoch: B is above a member's max_minibatch");
        if (!a.theta_dev || !a.adam_m_dev || !a.adam_v_dev || !a.obs_dev || !a.act_dev || !a.old_logp_dev || !a.adv_dev || !a.ret_dev || !a.perm_dev)
            return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_epoch: a member's argument is null");
        if (!(a.lr >= 0.0f)) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_epoch: a member's learning rate is negative or NaN");
    }
    QR_HIP(hipSetDevice(pop->device));
    hipStream_t st = (hipStream_t)stream;
    if (qr::stream_is_capturing(st))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_epoch: `stream` is being captured (the call uploads the member table and launches a graph of its own)");
    // the member table this call needs
    std::vector<qr::PopMember> table((size_t)P);
    std::memset(table.data(), 0, sizeof(qr::PopMember) * (size_t)P);   // padding included: the table is compared bytewise below
    std::vector<unsigned long long> seeds((size_t)P);
    qr::PopLr lrs;
    std::memset(&lrs, 0, sizeof(lrs));
    for (int p = 0; p < P; ++p) {
        qr_ppo* h = pop->members[p];
        const qr_ppo_member_args& a = args[p];
        qr::PopMember& m = table[(size_t)p];
        m.b.obs = a.obs_dev; m.b.act = a.act_dev; m.b.old_logp = a.old_logp_dev; m.b.adv = a.adv_dev; m.b.ret = a.ret_dev;
        m.b.idx = a.perm_dev;
        m.b.B = B; m.b.G = (B + 63) / 64;
        m.b.clip = a.clip; m.b.vf_coef = a.vf_coef; m.b.ent_coef = a.ent_coef;
        m.b.acc = h->d_mbstats;
        m.b.stop = &h->d_ctrl->stop;
        m.b.theta = a.theta_dev;
        m.b.images = h->d_images;
        m.b.wave_out = h->d_wave;
        m.b.stats = a.stats_dev;
        m.partial = h->d_partial;
        m.theta = a.theta_dev; m.m = a.adam_m_dev; m.v = a.adam_v_dev;
        m.ctrl = h->d_ctrl;
        m.max_norm = a.max_grad_norm; m.beta1 = a.beta1; m.beta2 = a.beta2; m.eps = a.eps;
        m.kl_limit = h->target_kl > 0.0f ? 1.5f * h->target_kl * (float)B : 0.0f;
        float* scratch = pop->d_scratch + (size_t)p * pop->scratch_floats;
        m.grad = scratch;
        m.sq = scratch + (size_t)pop->workgroups * qr::kApplyThreads;
        m.mb = m.sq + (pop->workgroups + 63) / 64 * 64;
        seeds[(size_t)p] = h->shuffle_seed;
        lrs.v[p] = a.lr;
    }
    const bool same_table = pop->table_valid && std::memcmp(table.data(), pop->h_table.data(), sizeof(qr::PopMember) * (size_t)P) == 0;
    if (!same_table) {
        // stream-ordered behind whatever earlier calls left on `st`; synchronised, so the host copy may go
        QR_HIP(hipMemcpyAsync(pop->d_table, table.data(), sizeof(qr::PopMember) * (size_t)P, hipMemcpyHostToDevice, st));
        QR_HIP(hipStreamSynchronize(st));
        pop->h_table = table;
        pop->table_valid = true;
    }
    hipLaunchKernelGGL(qr::ppo_population_lr_kernel, dim3(1), dim3(qr::kMaxPopulation), 0, st, pop->d_table, P, lrs);
    QR_HIP(hipGetLastError());
    for (int p = 0; p < P; ++p) {   // the step kernel keeps each member's images in step with its vector; its own epoch table is not armed
        pop->members[p]->packed_theta = args[p].theta_dev;
        pop->members[p]->epoch_idx = nullptr;
    }
    if (int rc = dispatch_L(pop->L, [&](auto Lc) { return PopOps<decltype(Lc)::value>::configure(pop); })) return rc;
    auto enqueue = [&](hipStream_t s) -> int {
        for (int e = 0; e < num_epochs; ++e) {
            for (int p = 0; p < P; ++p)   // per epoch and member: the existing shuffle / table-zeroing / advantage-sum kernels
                if (int rc = qr::ppo_epoch_prologue(pop->members[p], args[p].adv_dev, args[p].perm_dev, B, num_minibatches, device_shuffle, s))
                    return rc;
            for (int k = 0; k < num_minibatches; ++k)
                if (int rc = dispatch_L(pop->L, [&](auto Lc) { return PopOps<decltype(Lc)::value>::minibatch(pop, B, k, s); })) return rc;
        }
        return QR_OK;
    };
    if (!pop->epoch_graph) return enqueue(st);
    const bool hit = pop->exec && same_table && pop->g_B == B && pop->g_M == num_minibatches && pop->g_E == num_epochs &&
                     pop->g_shuffle == device_shuffle && pop->g_seeds == seeds;
    if (!hit) {
        if (pop->exec) { (void)hipGraphExecDestroy(pop->exec); pop->exec = nullptr; }
        if (!pop->capture_stream) QR_HIP(hipStreamCreateWithFlags(&pop->capture_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        QR_HIP(hipStreamBeginCapture(pop->capture_stream, hipStreamCaptureModeRelaxed));
        const int rc = enqueue(pop->capture_stream);
        const hipError_t end = hipStreamEndCapture(pop->capture_stream, &graph);
        if (rc != QR_OK || end != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc != QR_OK ? rc : qr::set_last_error(QR_E_HIP, std::string("qr_ppo_population_epoch: graph capture failed: ") + hipGetErrorString(end));
        }
        const hipError_t inst = hipGraphInstantiate(&pop->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (inst != hipSuccess) {
            pop->exec = nullptr;
            return qr::set_last_error(QR_E_HIP, std::string("qr_ppo_population_epoch: hipGraphInstantiate: ") + hipGetErrorString(inst));
        }
        pop->g_B = B; pop->g_M = num_minibatches; pop->g_E = num_epochs; pop->g_shuffle = device_shuffle; pop->g_seeds = seeds;
    }
    QR_HIP(hipGraphLaunch(pop->exec, st));
    return QR_OK;
}

int qr_ppo_population_exploit(qr_ppo_population* pop, float* const* theta_dev, float* const* adam_m_dev, float* const* adam_v_dev,
                              const int32_t* src_of, const float* log_std_shift, void* stream) {
    if (!pop || !theta_dev || !adam_m_dev || !adam_v_dev || !src_of) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_exploit: null argument");
    const int P = (int)pop->members.size();
    for (int p = 0; p < P; ++p) {
        if (!theta_dev[p] || !adam_m_dev[p] || !adam_v_dev[p]) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_exploit: a member's pointer is null");
        if (src_of[p] < 0 || src_of[p] >= P) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_exploit: src_of holds an index outside [0, members)");
        if (log_std_shift && !std::isfinite(log_std_shift[p])) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_exploit: a log_std_shift is not finite");
    }
    qr::ExploitPlan plan;
    std::memset(&plan, 0, sizeof(plan));
    int destinations = 0;
    for (int p = 0; p < P; ++p) {
        const int s = src_of[p];
        if (s == p) continue;
        if (src_of[s] != s)
            return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_exploit: a source is itself a destination (one launch may not read what it writes)");
        const float shift = log_std_shift ? log_std_shift[p] : 0.0f;
        plan.dst[destinations] = (unsigned char)p;
        plan.src[destinations] = (unsigned char)s;
        plan.shift[destinations] = shift;
        ++destinations;
    }
    QR_HIP(hipSetDevice(pop->device));
    hipStream_t st = (hipStream_t)stream;
    if (qr::stream_is_capturing(st))
        return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_exploit: `stream` is being captured (the call may allocate and upload the member table)");
    if (destinations == 0) return QR_OK;
    // the members as the kernel sees them: uploaded when a pointer moved (in practice: by the first call)
    std::vector<qr::ExploitMember> table((size_t)P);
    for (int p = 0; p < P; ++p) {
        qr_ppo* h = pop->members[p];
        table[(size_t)p] = qr::ExploitMember{theta_dev[p], adam_m_dev[p], adam_v_dev[p], h->d_images, h->d_ctrl};
    }
    static_assert(sizeof(qr::ExploitMember) == 5 * sizeof(void*), "no padding: the table is compared bytewise");
    if (!pop->exploit_valid || std::memcmp(table.data(), pop->h_exploit.data(), sizeof(qr::ExploitMember) * (size_t)P) != 0) {
        if (!pop->d_exploit) QR_HIP(hipMalloc((void**)&pop->d_exploit, sizeof(qr::ExploitMember) * (size_t)P));
        // stream-ordered behind whatever earlier calls left on `st`; synchronised, so the host copy may go
        pop->exploit_valid = false;
        QR_HIP(hipMemcpyAsync(pop->d_exploit, table.data(), sizeof(qr::ExploitMember) * (size_t)P, hipMemcpyHostToDevice, st));
        QR_HIP(hipStreamSynchronize(st));
        pop->h_exploit = table;
        pop->exploit_valid = true;
    }
    if (int rc = dispatch_L(pop->L, [&](auto Lc) {
            constexpr int L = decltype(Lc)::value;
            const int n = qr::ppo_num_params(L), images = 2 * qr::PpoDims<L>::kImage;
            const int blocks = ((n > images ? n : images) + qr::kExploitThreads - 1) / qr::kExploitThreads;
            hipLaunchKernelGGL(qr::ppo_population_exploit_kernel<L>, dim3(blocks, destinations), dim3(qr::kExploitThreads), 0, st,
                               (const qr::ExploitMember*)pop->d_exploit, plan);
            QR_HIP(hipGetLastError());
            return (int)QR_OK;
        }))
        return rc;
    for (int d = 0; d < destinations; ++d) {   // as qr_ppo_pack leaves the handle: its images belong to this vector
        pop->members[plan.dst[d]]->packed_theta = theta_dev[plan.dst[d]];
    }
    return QR_OK;
}

int qr_ppo_population_status(qr_ppo_population* pop, int32_t* out, void* stream) {
    if (!pop || !out) return qr::set_last_error(QR_E_INVALID, "qr_ppo_population_status: null argument");
    QR_HIP(hipSetDevice(pop->device));
    hipStream_t st = (hipStream_t)stream;
    for (size_t p = 0; p < pop->members.size(); ++p)
        QR_HIP(hipMemcpyAsync(out + 4 * p, &pop->members[p]->d_ctrl->stop, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    QR_HIP(hipStreamSynchronize(st));
    return QR_OK;
}

}  // extern "C"
