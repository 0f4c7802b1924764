// quadrace_abi.hip -- host side of libquadrace.so: the extern "C" boundary declared in include/quadrace.h.
// Owns the planar HBM state of one env shard, the constant tables, and enqueues the gfx950 kernels on the
// caller's stream.  There is deliberately no CPU execution path: without a gfx950 device qr_create fails.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/quadrace.h"
#include "quadrace_launch.hpp"

struct qr_env {
    qr_config cfg{};
    int S = 0, L = 0;
    qr::Params P{};
    void* slab = nullptr;       // one HBM allocation holding every state plane
    float* d_tables = nullptr;  // [gate rows | fused MLP table]
    int num_gates = 0;
    int rollout_form = 0;       // QR_ROLLOUT_AUTO | _MULTI_WAVE | _GENERAL (qr_set_rollout_form)
    int term_rows = 0;          // leading dimension of the registered terminal-observation buffer (K-step calls need K <= rows)
    bool has_track = false;
    std::vector<float> gate_pos, gate_yaw, gate_pos_rel, gate_yaw_rel;
    float mlp_table[qr::kMlpTableFloats] = {};
    // host-side configuration that only reaches the device through the tables
    float start[3] = {0.0f, 0.0f, 0.0f};
    float dist_lo[6] = {}, dist_hi[6] = {};
    float dist_scale = 1.0f;  // R:358
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing_valid = false;
    bool timing = true;         // qr_set_timing: bracket the K-step calls with hipEvents (two marker packets per call)
    // qr_step_launches: the K step-kernel launches of one call, captured once into a hipGraph and replayed while the
    // arguments stay the same (measured, tools/ubench/launch_floor.hip: back-to-back dependent launches cost 2.6 us
    // each on a stream and 1.5 us as consecutive kernel nodes of a graph)
    struct StepGraph {
        hipGraphExec_t exec = nullptr;
        int K = 0;
        const void *act = nullptr, *obs = nullptr, *rew = nullptr, *done = nullptr, *trunc = nullptr;
        qr::Params P{};
    } sg;
    hipStream_t capture_stream = nullptr;
    // a per-group table of the last launch in a device array of the handle, [cap] entries, and its host mirror (upload_table)
    template <typename T>
    struct DeviceTable {
        T* d = nullptr;
        int cap = 0;
        std::vector<T> host;
    };
    DeviceTable<int2> group_map;                  // qr_evaluate_policy_grid and the group rollouts: (policy or dynamics, condition) per group
    DeviceTable<qr::PopulationEntry> pop_table;   // qr_rollout_policy_population: the sampling values per group
    DeviceTable<int4> dyn_map;                    // qr_evaluate_policy_dynamics_grid: (policy, condition, dynamics, 0) per group
    DeviceTable<int4> sen_map;                    // qr_evaluate_policy_sensing_grid: (policy, condition, dynamics, sensing) per group
    DeviceTable<int> rollout_sen_map;             // qr_rollout_policy_sensing: the sensing slot per group (the pair travels in group_map)
};

// A bank of flight conditions for qr_evaluate_policy_grid: [capacity][qr::kCondSlotFloats] floats on the device, slot s =
// [CondHeader | reset table | gate rows], built by the functions that build a handle's tables (condition_obs_scale,
// gate_relative_table, build_condition_image below).
struct qr_condition_bank {
    int variant = 0, device = 0, capacity = 0;
    float* d_slots = nullptr;
    std::vector<uint8_t> is_set;   // per slot: qr_condition_bank_set has succeeded
};

// A bank of vehicles for qr_evaluate_policy_dynamics_grid: [capacity][qr::kDynSlotFloats] floats on the device, slot s = the variant's
// coefficient table of quadrace_device.hpp followed by zeros.
struct qr_dynamics_bank {
    int variant = 0, device = 0, capacity = 0;
    float* d_slots = nullptr;
    std::vector<uint8_t> is_set;   // per slot: qr_dynamics_bank_set has succeeded, or qr_vehicle_bank_sample has enqueued its draw
};

// A bank of sensors for qr_evaluate_policy_sensing_grid: [capacity][qr::kSensingSlotFloats] floats on the device, slot s = sigma[0..7],
// the command delay as an int32 bit pattern, zeros.
struct qr_sensing_bank {
    int device = 0, capacity = 0;
    float* d_slots = nullptr;
    std::vector<uint8_t> is_set;   // per slot: qr_sensing_bank_set has succeeded
};

namespace {

// observation scaling of the constant disturbances (R:414-448): if min == max the range becomes (min-1, max+1).  Shared by the
// handle (Params::obs_lo / obs_inv) and the header of a condition image.
void condition_obs_scale(const float* dist_lo, const float* dist_hi, float* obs_lo, float* obs_inv) {
    static const int col[4] = {0, 1, 2, 5};
    for (int c = 0; c < 4; ++c) {
        float lo = dist_lo[col[c]], hi = dist_hi[col[c]];
        if (lo == hi) { lo -= 1.0f; hi += 1.0f; }
        obs_lo[c] = lo;
        obs_inv[c] = 1.0f / (hi - lo);
    }
}
void update_obs_scale(qr_env* e) { condition_obs_scale(e->dist_lo, e->dist_hi, e->P.obs_lo, e->P.obs_inv); }

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace

namespace qr {
// shared with quadrace_policy.hip: one thread-local error string behind qr_last_error()
int set_last_error(int code, const std::string& msg) { return fail(code, msg); }
}  // namespace qr

namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// gate i expressed in the frame of gate i-1, looped track (R:307-319), float32 like the reference: pos_rel [G][3], yaw_rel [G]
void gate_relative_table(const float* gate_pos, const float* gate_yaw, int G, float* pos_rel, float* yaw_rel) {
    for (int i = 0; i < G; ++i) {
        const int j = (i + G - 1) % G;
        const float dx = gate_pos[3 * i + 0] - gate_pos[3 * j + 0];
        const float dy = gate_pos[3 * i + 1] - gate_pos[3 * j + 1];
        const float c = cosf(gate_yaw[j]), s = sinf(gate_yaw[j]);
        volatile float cx = c * dx, sy = s * dy, sx = -s * dx, cy = c * dy;  // no host FMA contraction
        pos_rel[3 * i + 0] = cx + sy;
        pos_rel[3 * i + 1] = sx + cy;
        pos_rel[3 * i + 2] = gate_pos[3 * i + 2] - gate_pos[3 * j + 2];
        yaw_rel[i] = gate_yaw[i] - gate_yaw[j];
    }
}

// The condition-dependent part of the device table image, [reset table | gate rows]: img[0 .. kResetTableFloats + G * kGateStride),
// zero-filled by the caller.  What a handle holds from kOffResetImage on, and what a slot of a qr_condition_bank holds behind its header.
void build_condition_image(int variant, const float* start, const float* dist_lo, const float* dist_hi, float dist_scale, int G,
                           const float* gate_pos, const float* gate_yaw, const float* gate_pos_rel, const float* gate_yaw_rel, float* img) {
    // reset table rows (lo, hi - lo, add, mul): value = ((lo + (hi-lo)*u) + add) * mul   (R:455-489 / I:270-296)
    float* R = img;
    auto row = [&](int t, float lo, float hi, float add, float mul) {
        volatile float span = hi - lo;  // float32 subtraction, like the oracle / the reference's ranges
        R[4 * t + 0] = lo; R[4 * t + 1] = span; R[4 * t + 2] = add; R[4 * t + 3] = mul;
    };
    const float pi9 = 0.3490658503988659f, pi = 3.141592653589793f;
    for (int t = 0; t < 3; ++t) row(t, -0.5f, 0.5f, start[t], 1.0f);
    for (int t = 3; t < 6; ++t) row(t, -0.5f, 0.5f, 0.0f, 1.0f);
    row(6, -pi9, pi9, 0.0f, 1.0f);
    row(7, -pi9, pi9, 0.0f, 1.0f);
    row(8, -pi, pi, 0.0f, 1.0f);
    for (int t = 9; t < 12; ++t) row(t, -0.1f, 0.1f, 0.0f, 1.0f);
    if (variant == QR_VARIANT_E2E) {
        for (int t = 12; t < 16; ++t) row(t, -1.0f, 1.0f, 0.0f, 1.0f);
        for (int k = 0; k < 6; ++k) row(16 + k, dist_lo[k], dist_hi[k], 0.0f, dist_scale);
    } else {
        row(12, -0.1f, 0.1f, 0.0f, 1.0f);
    }
    for (int g = 0; g < G; ++g) {
        float* grow = img + qr::kResetTableFloats + g * qr::kGateStride;
        grow[0] = gate_pos[3 * g + 0];
        grow[1] = gate_pos[3 * g + 1];
        grow[2] = gate_pos[3 * g + 2];
        grow[3] = gate_yaw[g];
        grow[4] = cosf(gate_yaw[g]);  // the reference evaluates np.cos/np.sin on the f32 yaw every step (R:372-375,528)
        grow[5] = sinf(gate_yaw[g]);
        grow[8] = gate_pos_rel[3 * g + 0];
        grow[9] = gate_pos_rel[3 * g + 1];
        grow[10] = gate_pos_rel[3 * g + 2];
        grow[11] = gate_yaw_rel[g];
    }
}

int upload_tables(qr_env* e) {
    const int gate_floats = e->num_gates * qr::kGateStride;
    // device image: [MLP table | reset table | gate rows]
    std::vector<float> host(qr::kOffGatesImage + gate_floats, 0.0f);
    std::memcpy(host.data(), e->mlp_table, sizeof(e->mlp_table));
    build_condition_image(e->cfg.variant, e->start, e->dist_lo, e->dist_hi, e->dist_scale, e->num_gates, e->gate_pos.data(), e->gate_yaw.data(),
                          e->gate_pos_rel.data(), e->gate_yaw_rel.data(), host.data() + qr::kOffResetImage);
    QR_HIP(hipDeviceSynchronize());  // configuration setters are rare: do not race kernels still reading the table
    QR_HIP(hipMemcpy(e->d_tables, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    return QR_OK;
}

// A host may hold handles on several GPUs in one process: every entry point that touches the device first makes the
// handle's GPU current (kernels launch on the CURRENT device; a stream of another device would be rejected).
int bind_device(const qr_env* e) {
    if (!e) return fail(QR_E_INVALID, "null env handle");
    QR_HIP(hipSetDevice(e->cfg.device));
    return QR_OK;
}

int check_ready(const qr_env* e) {
    if (int rc = bind_device(e)) return rc;
    if (!e->has_track) return fail(QR_E_STATE, "qr_set_track has not been called");
    return QR_OK;
}

// hipEvent bracket of a K-step call: skipped when switched off (qr_set_timing) or while the caller captures `st` into a graph
bool want_events(const qr_env* e, hipStream_t st) { return e->timing && !qr::stream_is_capturing(st); }

// K-step entry points write terminal observations to row [k][env]: the registered buffer must hold K rows of N envs
int check_term_rows(const qr_env* e, int K, const char* who) {
    if (e->P.term_obs && K > e->term_rows)
        return fail(QR_E_INVALID, std::string(who) + ": num_steps exceeds the rows of the registered terminal-observation buffer "
                                  "(qr_set_terminal_obs); register a [K][N][obs_len] buffer or NULL first");
    return QR_OK;
}

// What every closed-loop evaluator (qr_evaluate_policy, _bank, _grid) refuses about its own arguments and the handle's mode, in the
// order they all refuse it.  gates_per_lap: the entry point's argument, or nullptr where it has none (the grid evaluator takes it
// from its condition headers, which qr_condition_bank_set has checked).
int check_eval_args(const qr_env* e, int K, const int32_t* gates_per_lap, int flags, const int32_t* rec_dev, const float* recf_dev,
                    const char* who) {
    const std::string w = std::string(who) + ": ";
    if (!rec_dev) return fail(QR_E_INVALID, w + "rec_dev is required");
    if (((uintptr_t)rec_dev | (uintptr_t)recf_dev) & 15) return fail(QR_E_INVALID, w + "the record buffers must be 16-byte aligned");
    if (K < 1) return fail(QR_E_INVALID, w + "num_steps must be >= 1");
    if (gates_per_lap && *gates_per_lap < 1) return fail(QR_E_INVALID, w + "gates_per_lap must be >= 1");
    if (flags & ~QR_ROLLOUT_F32CLASS) return fail(QR_E_INVALID, w + "`flags` takes QR_ROLLOUT_F32CLASS or 0");
    if (e->num_gates < 2) return fail(QR_E_INVALID, w + "the track has one gate: a pass cannot move the target, so passes cannot be counted");
    if (e->P.flags & (qr::kFlagPause | qr::kFlagPauseIfCollision))
        return fail(QR_E_STATE, w + "lap accounting is defined for the default mode, not for pause / pause_if_collision");
    return QR_OK;
}

// Group shape of the bank and grid evaluators: `groups` groups (argument `count_name`) of envs_per_<unit> envs each, whole workgroups,
// covering the handle exactly.  groups >= 1 is the caller's check (its message differs between the two).
int check_group_shape(const qr_env* e, int groups, int envs_per_group, const char* count_name, const char* unit, const char* who) {
    const std::string w = std::string(who) + ": ", envs_name = std::string("envs_per_") + unit;
    if (envs_per_group < qr::kBlock || envs_per_group % qr::kBlock != 0)
        return fail(QR_E_INVALID, w + envs_name + " must be a multiple of 256, at least 256 (one workgroup serves one " + unit + ")");
    if ((int64_t)groups * envs_per_group != (int64_t)e->cfg.num_envs)
        return fail(QR_E_INVALID, w + count_name + " * " + envs_name + " must equal the env count of the handle");
    return QR_OK;
}

// What the three group entry points (qr_evaluate_policy_grid, qr_rollout_policy_conditions, qr_rollout_policy_population) refuse about
// the condition bank and the group shape, in the order they all refuse it.
int check_condition_groups(const qr_env* e, const qr_condition_bank* conditions, int num_groups, int envs_per_group, const char* who) {
    if (conditions->variant != e->cfg.variant) return fail(QR_E_INVALID, std::string(who) + ": condition bank of another variant");
    if (conditions->device != e->cfg.device) return fail(QR_E_INVALID, std::string(who) + ": condition bank on another GPU");
    if (num_groups < 1) return fail(QR_E_INVALID, std::string(who) + ": num_groups must be >= 1");
    return check_group_shape(e, num_groups, envs_per_group, "num_groups", "group", who);
}

// The group maps of the same three: first every index against its bank, then every slot it names filled; within a pass group by group,
// the policy before the condition.  No index reaches the device that has not passed here.  policy_of_group = nullptr: no policy bank
// (qr_rollout_policy_conditions).
int check_group_indices(const qr_policy_bank* policies, const int32_t* policy_of_group, const qr_condition_bank* conditions,
                        const int32_t* condition_of_group, int num_groups, const char* who) {
    const int pcap = policy_of_group ? qr::bank_capacity(policies) : 0;
    const auto at = [who](const char* map, int g) { return std::string(who) + ": " + map + "[" + std::to_string(g) + "] is outside the "; };
    const auto slot = [who](int s) { return std::string(who) + ": slot " + std::to_string(s) + " of the "; };
    for (int g = 0; g < num_groups; ++g) {
        if (policy_of_group && (policy_of_group[g] < 0 || policy_of_group[g] >= pcap))
            return fail(QR_E_INVALID, at("policy_of_group", g) + "policy bank");
        if (condition_of_group[g] < 0 || condition_of_group[g] >= conditions->capacity)
            return fail(QR_E_INVALID, at("condition_of_group", g) + "condition bank");
    }
    for (int g = 0; g < num_groups; ++g) {
        if (policy_of_group && !qr::bank_slot_set(policies, policy_of_group[g]))
            return fail(QR_E_STATE, slot(policy_of_group[g]) + "policy bank has no weights");
        if (!conditions->is_set[(size_t)condition_of_group[g]])
            return fail(QR_E_STATE, slot(condition_of_group[g]) + "condition bank was never set");
    }
    return QR_OK;
}

// What qr_evaluate_policy_dynamics_grid and qr_rollout_policy_dynamics refuse about the dynamics bank, in two steps that stand where the
// condition bank's two steps stand: the bank against the handle, then every index against the bank and every slot it names filled.
int check_dynamics_bank(const qr_env* e, const qr_dynamics_bank* dynamics, const char* who) {
    if (dynamics->variant != e->cfg.variant) return fail(QR_E_INVALID, std::string(who) + ": dynamics bank of another variant");
    if (dynamics->device != e->cfg.device) return fail(QR_E_INVALID, std::string(who) + ": dynamics bank on another GPU");
    return QR_OK;
}
int check_dynamics_indices(const qr_dynamics_bank* dynamics, const int32_t* dynamics_of_group, int num_groups, const char* who) {
    const std::string w = std::string(who) + ": ";
    for (int g = 0; g < num_groups; ++g)
        if (dynamics_of_group[g] < 0 || dynamics_of_group[g] >= dynamics->capacity)
            return fail(QR_E_INVALID, w + "dynamics_of_group[" + std::to_string(g) + "] is outside the dynamics bank");
    for (int g = 0; g < num_groups; ++g)
        if (!dynamics->is_set[(size_t)dynamics_of_group[g]])
            return fail(QR_E_STATE, w + "slot " + std::to_string(dynamics_of_group[g]) + " of the dynamics bank was never set");
    return QR_OK;
}

// A per-group table of a launch (the group map, the sampling table) in a device array of the handle.  An equal table (byte for byte; any
// pad is zero) is already there; another one is copied after a device synchronisation, like the tables (an earlier launch may still
// read the array), which a stream under capture does not allow.  `noun` / `these`: what the capture refusal calls the table.
template <typename T>
bool table_is_current(const qr_env::DeviceTable<T>& t, const std::vector<T>& table) {
    return t.d && table.size() == t.host.size() && std::memcmp(table.data(), t.host.data(), table.size() * sizeof(T)) == 0;
}
template <typename T>
int upload_table(qr_env::DeviceTable<T>& t, const std::vector<T>& table, hipStream_t st, const char* who, const char* noun, const char* these) {
    const size_t bytes = table.size() * sizeof(T);
    if (table_is_current(t, table)) return QR_OK;
    if (qr::stream_is_capturing(st))
        return fail(QR_E_STATE, std::string(who) + ": a new " + noun + " is uploaded after a device synchronisation, which a stream under "
                                                   "capture does not allow; call once with " + these + " outside the capture");
    QR_HIP(hipDeviceSynchronize());
    t.host.clear();   // nothing valid on the device until the copy below has succeeded
    if ((int)table.size() > t.cap) {
        if (t.d) (void)hipFree(t.d);
        t.d = nullptr;
        t.cap = 0;
        QR_HIP(hipMalloc((void**)&t.d, bytes));
        t.cap = (int)table.size();
    }
    QR_HIP(hipMemcpy(t.d, table.data(), bytes, hipMemcpyHostToDevice));
    t.host = table;
    return QR_OK;
}
// the (policy, condition) map of a launch; policy_of_group = nullptr: the policy half is zero
int upload_group_map(qr_env* e, const int32_t* policy_of_group, const int32_t* condition_of_group, int num_groups, hipStream_t st, const char* who) {
    std::vector<int2> map((size_t)num_groups);
    for (int g = 0; g < num_groups; ++g) map[(size_t)g] = make_int2(policy_of_group ? policy_of_group[g] : 0, condition_of_group[g]);
    return upload_table(e->group_map, map, st, who, "group map", "this map");
}

// One launch on `st` inside the hipEvent bracket of want_events: QR_TIMED_LAUNCH(e, st, launcher call).  A failed launch reports the
// call's text, as QR_HIP does.
#define QR_TIMED_LAUNCH(e, st, expr) timed_launch(e, st, #expr, [&] { return (expr); })
template <typename Launch>
int timed_launch(qr_env* e, hipStream_t st, const char* what, Launch&& launch) {
    const bool ev = want_events(e, st);
    if (ev) QR_HIP(hipEventRecord(e->ev0, st));
    if (hipError_t err = launch()) return fail(QR_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
    if (ev) QR_HIP(hipEventRecord(e->ev1, st));
    e->timing_valid = ev;
    return QR_OK;
}

// the open-loop entry points (qr_step, qr_step_many, qr_step_launches, qr_profile_steps) need these four; trunc may be null
int check_step_buffers(const float* actions, const float* obs, const float* rew, const uint8_t* done, const char* who) {
    if (!actions || !obs || !rew || !done) return fail(QR_E_INVALID, std::string(who) + ": actions/obs/rew/done buffers are required");
    return QR_OK;
}

// step k of a K-step call as one launch of the step kernel: row k of the [K][N][...] buffers and of the terminal-observation rows
hipError_t launch_step_row(const qr_env* e, int k, const float* actions, float* obs, float* rew, uint8_t* done, uint8_t* trunc, hipStream_t st) {
    const size_t row = (size_t)k * (size_t)e->cfg.num_envs;
    qr::Params Pk = e->P;
    if (Pk.term_obs) Pk.term_obs += row * e->L;
    return qr::launch_step(e->cfg.variant, Pk, actions + row * 4, obs + row * e->L, rew + row, done + row, trunc ? trunc + row : nullptr, st);
}

// What the closed-loop rollouts (qr_rollout_policy, _conditions, _population) refuse first, in one order: `required` = the entry
// point's handles and arrays are all there.
int check_rollout_common(const qr_env* e, int K, bool required, const float* obs, const float* act, const float* logp, const float* rew,
                         const uint8_t* done, const char* who) {
    if (K < 1 || !required) return fail(QR_E_INVALID, std::string(who) + ": bad argument");
    if (int rc = check_term_rows(e, K, who)) return rc;
    if (!obs || !act || !logp || !rew || !done) return fail(QR_E_INVALID, std::string(who) + ": obs/act/logp/rew/done buffers are required");
    if (e->P.flags & (qr::kFlagPause | qr::kFlagPauseIfCollision))
        return fail(QR_E_STATE, std::string(who) + ": pause / pause_if_collision envs are evaluation modes; use qr_step");
    return QR_OK;
}

}  // namespace

extern "C" {

int qr_abi_version(void) { return QR_ABI_VERSION; }
const char* qr_last_error(void) { return g_err.c_str(); }

int qr_create(const qr_config* cfg, qr_env** out) {
    if (!cfg || !out) return fail(QR_E_INVALID, "qr_create: null argument");
    *out = nullptr;
    if (cfg->variant != QR_VARIANT_E2E && cfg->variant != QR_VARIANT_INDI)
        return fail(QR_E_INVALID, "qr_create: unknown variant");
    if (cfg->num_envs < 1) return fail(QR_E_INVALID, "qr_create: num_envs must be >= 1");
    if (cfg->gates_ahead < 0 || cfg->gates_ahead > QR_MAX_GATES_AHEAD)
        return fail(QR_E_INVALID, "qr_create: gates_ahead out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(QR_E_NO_DEVICE, "qr_create: no HIP device visible (libquadrace has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(QR_E_INVALID, "qr_create: bad device ordinal");
    hipDeviceProp_t prop;
    QR_HIP(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(QR_E_NO_DEVICE, std::string("qr_create: device is ") + prop.gcnArchName + ", kernels are gfx950-only");
    QR_HIP(hipSetDevice(cfg->device));

    qr_env* e = new qr_env();
    e->cfg = *cfg;
    const bool e2e = cfg->variant == QR_VARIANT_E2E;
    e->S = e2e ? 16 : 13;
    e->L = e->S + 4 * cfg->gates_ahead + (e2e ? 4 : 0);  // R:330 / I:185
    const int n = cfg->num_envs;
    const size_t ns = align_up((size_t)n, qr::kBlock);
    // slab layout (every region 256-byte aligned)
    const size_t sz_ws = align_up(sizeof(float4) * ns * (e2e ? 4 : 3), 256);
    const size_t sz_tn = e2e ? 0 : align_up(sizeof(float) * ns, 256);
    const size_t sz_dA = e2e ? align_up(sizeof(float4) * ns, 256) : 0;
    const size_t sz_dB = e2e ? align_up(sizeof(float2) * ns, 256) : 0;
    const size_t sz_ts = align_up(sizeof(int2) * ns, 256);
    const size_t total = sz_ws + sz_tn + sz_dA + sz_dB + sz_ts;
    if (hipMalloc(&e->slab, total) != hipSuccess) {
        delete e;
        return fail(QR_E_HIP, "qr_create: hipMalloc of the state slab failed");
    }
    if (hipMalloc((void**)&e->d_tables, sizeof(float) * (qr::kOffGatesImage + qr::kMaxGates * qr::kGateStride)) != hipSuccess) {
        (void)hipFree(e->slab);
        delete e;
        return fail(QR_E_HIP, "qr_create: hipMalloc of the table buffer failed");
    }
    (void)hipMemset(e->slab, 0, total);
    char* p = static_cast<char*>(e->slab);
    qr::Params& P = e->P;
    P.ws = reinterpret_cast<float4*>(p); p += sz_ws;
    P.tn = e2e ? nullptr : reinterpret_cast<float*>(p); p += sz_tn;
    P.dA = e2e ? reinterpret_cast<float4*>(p) : nullptr; p += sz_dA;
    P.dB = e2e ? reinterpret_cast<float2*>(p) : nullptr; p += sz_dB;
    P.ts = reinterpret_cast<int2*>(p);
    P.tables = e->d_tables;
    P.n = n;
    P.n_stride = (int)ns;
    P.num_gates = 0;
    P.gates_ahead = cfg->gates_ahead;
    P.max_steps = 1200;  // R:345
    P.dt = 0.01f;        // R:346
    P.flags = cfg->pause_if_collision ? qr::kFlagPauseIfCollision : 0;
    P.seed_lo = P.seed_hi = 0;
    P.gid_lo = (uint32_t)cfg->env_id_base;
    P.gid_hi = (uint32_t)(cfg->env_id_base >> 32);
    update_obs_scale(e);
    (void)hipEventCreate(&e->ev0);
    (void)hipEventCreate(&e->ev1);
    *out = e;
    return QR_OK;
}

int qr_destroy(qr_env* e) {
    if (!e) return QR_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->sg.exec) (void)hipGraphExecDestroy(e->sg.exec);
    if (e->capture_stream) (void)hipStreamDestroy(e->capture_stream);
    if (e->slab) (void)hipFree(e->slab);
    if (e->d_tables) (void)hipFree(e->d_tables);
    if (e->group_map.d) (void)hipFree(e->group_map.d);
    if (e->pop_table.d) (void)hipFree(e->pop_table.d);
    if (e->dyn_map.d) (void)hipFree(e->dyn_map.d);
    if (e->sen_map.d) (void)hipFree(e->sen_map.d);
    if (e->rollout_sen_map.d) (void)hipFree(e->rollout_sen_map.d);
    delete e;
    return QR_OK;
}

int qr_state_len(const qr_env* e) { return e ? e->S : QR_E_INVALID; }
int qr_obs_len(const qr_env* e) { return e ? e->L : QR_E_INVALID; }
int qr_num_envs(const qr_env* e) { return e ? e->cfg.num_envs : QR_E_INVALID; }

int qr_set_track(qr_env* e, const float* gate_pos, const float* gate_yaw, int32_t G, const float* start_pos) {
    if (!e || !gate_pos || !gate_yaw || !start_pos) return fail(QR_E_INVALID, "qr_set_track: null argument");
    if (G < 1 || G > QR_MAX_GATES) return fail(QR_E_INVALID, "qr_set_track: num_gates must be in 1..QR_MAX_GATES");
    QR_HIP(hipSetDevice(e->cfg.device));
    e->num_gates = G;
    e->gate_pos.assign(gate_pos, gate_pos + 3 * G);
    e->gate_yaw.assign(gate_yaw, gate_yaw + G);
    e->gate_pos_rel.assign(3 * G, 0.0f);
    e->gate_yaw_rel.assign(G, 0.0f);
    gate_relative_table(gate_pos, gate_yaw, G, e->gate_pos_rel.data(), e->gate_yaw_rel.data());
    for (int k = 0; k < 3; ++k) e->start[k] = start_pos[k];
    e->P.num_gates = G;
    e->has_track = true;
    return upload_tables(e);
}

int qr_get_track_tables(const qr_env* e, float* gate_pos_rel, float* gate_yaw_rel) {
    if (!e) return fail(QR_E_INVALID, "null env handle");
    if (!e->has_track) return fail(QR_E_STATE, "qr_set_track has not been called");
    if (gate_pos_rel) std::memcpy(gate_pos_rel, e->gate_pos_rel.data(), sizeof(float) * 3 * e->num_gates);
    if (gate_yaw_rel) std::memcpy(gate_yaw_rel, e->gate_yaw_rel.data(), sizeof(float) * e->num_gates);
    return QR_OK;
}

int qr_set_residual(qr_env* e, const float* blob, size_t n_floats) {
    if (!e) return fail(QR_E_INVALID, "qr_set_residual: null env");
    if (e->cfg.variant != QR_VARIANT_E2E) return fail(QR_E_INVALID, "qr_set_residual: E2E variant only");
    QR_HIP(hipSetDevice(e->cfg.device));
    if (!blob) {
        e->P.flags &= ~qr::kFlagResidual;
        return QR_OK;
    }
    if (n_floats != QR_RESIDUAL_FLOATS) return fail(QR_E_INVALID, "qr_set_residual: expected 740 floats");
    // layer 1 (W1, b1 of both networks) runs on f16 matrix-core operands, each weight as two f16 pieces: a weight beyond the f16 range
    // would turn into inf - inf = NaN pieces where the reference's float32 layer gives a finite value -- refused, not approximated.
    // Layer 2 (W2, b2) is float32 arithmetic like the reference's: any finite value is accepted there.
    for (size_t k = 0; k < n_floats; ++k) {
        const bool layer1 = k < 224 + 32 || (k >= 289 && k < 289 + 320 + 32);
        if (!std::isfinite(blob[k]))
            return fail(QR_E_INVALID, "qr_set_residual: weights must be finite");
        if (layer1 && std::fabs(blob[k]) > 65504.0f)
            return fail(QR_E_INVALID, "qr_set_residual: first-layer weights and biases must be within +-65504 (the f16 range of the matrix-core operands)");
    }
    // reference order (c_code/nn_thrust.c, nn_moment.c): W1[out][in], b1, W2[out][in], b2 per network
    const float* tW1 = blob;         const float* tb1 = tW1 + 224;
    const float* tW2 = tb1 + 32;     const float* tb2 = tW2 + 32;
    const float* mW1 = tb2 + 1;      const float* mb1 = mW1 + 320;
    const float* mW2 = mb1 + 32;     const float* mb2 = mW2 + 96;
    // device image: MFMA A operands, layer-2 weights per wave half, output biases (see quadrace_device.hpp)
    float* T = e->mlp_table;
    std::memset(T, 0, sizeof(e->mlp_table));
    // layer 1: every weight and bias as two f16 pieces w = W0 + W1 (round to nearest even; w - W0 is exact in float32), laid out as
    // the A operands of the five v_mfma_f32_32x32x16_f16 instructions per env tile (quadrace_device.hpp, "Residual-MLP table")
    auto piece0 = [](float w) { return (_Float16)w; };
    auto piece1 = [](float w) { return (_Float16)(w - (float)(_Float16)w); };
    _Float16* A = reinterpret_cast<_Float16*>(T + qr::kOffTabA);
    auto slot = [&](int q, int lane, int j) -> _Float16& { return A[((size_t)q * 64 + lane) * 8 + j]; };
    for (int row = 0; row < 32; ++row) {
        const int lo = row, hi = row + 32;   // lanes holding k-slots 0..7 / 8..15 of this hidden row
        for (int k = 0; k < 7; ++k) {
            slot(0, lo, k) = piece0(tW1[row * 7 + k]);   slot(0, hi, k) = piece0(tW1[row * 7 + k]);    // X0 W0 | X1 W0
            slot(1, lo, k) = piece1(tW1[row * 7 + k]);                                                  // X0 W1 | 0
            slot(2, lo, k) = piece0(mW1[row * 10 + k]);  slot(2, hi, k) = piece0(mW1[row * 10 + k]);
            slot(3, lo, k) = piece1(mW1[row * 10 + k]);
        }
        slot(0, lo, 7) = piece0(tb1[row]);  slot(1, lo, 7) = piece1(tb1[row]);   // k-slot 7 of the low half multiplies the constant 1
        slot(2, lo, 7) = piece0(mb1[row]);  slot(3, lo, 7) = piece1(mb1[row]);
        for (int k = 0; k < 3; ++k) {        // rates p, q, r: [X0 (3), 0, X1 (3), 0] in both halves
            slot(4, lo, k) = piece0(mW1[row * 10 + 7 + k]);  slot(4, lo, 4 + k) = piece0(mW1[row * 10 + 7 + k]);   // X0 W0, X1 W0
            slot(4, hi, k) = piece1(mW1[row * 10 + 7 + k]);                                                          // X0 W1
        }
    }
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            // x 2^40 (exact): the kernels' ReLU leaves max(x, 0) * 2^-40, see relu2_scaled() in quadrace_device.hpp
            T[qr::kOffTabW2 + 64 * h + r] = tW2[row] * qr::kReluUp;
            for (int m = 0; m < 3; ++m) T[qr::kOffTabW2 + 64 * h + 16 + 16 * m + r] = mW2[m * 32 + row] * qr::kReluUp;
        }
    T[qr::kOffB2 + 0] = tb2[0];
    for (int o = 0; o < 3; ++o) T[qr::kOffB2 + 1 + o] = mb2[o];
    e->P.flags |= qr::kFlagResidual;
    if (e->has_track) return upload_tables(e);
    return QR_OK;
}

int qr_set_disturbance(qr_env* e, const float* ranges, float scale) {
    if (!e || !ranges) return fail(QR_E_INVALID, "qr_set_disturbance: null argument");
    if (e->cfg.variant != QR_VARIANT_E2E) return fail(QR_E_INVALID, "qr_set_disturbance: E2E variant only");
    for (int k = 0; k < 6; ++k) {
        e->dist_lo[k] = ranges[2 * k + 0];
        e->dist_hi[k] = ranges[2 * k + 1];
    }
    e->dist_scale = scale;
    update_obs_scale(e);
    QR_HIP(hipSetDevice(e->cfg.device));
    return upload_tables(e);  // the reset table carries the disturbance ranges
}

int qr_set_limits(qr_env* e, int32_t max_steps, float dt) {
    if (!e) return fail(QR_E_INVALID, "qr_set_limits: null env");
    e->P.max_steps = max_steps;
    e->P.dt = dt;
    return QR_OK;
}

int qr_set_pause(qr_env* e, int32_t pause) {
    if (!e) return fail(QR_E_INVALID, "qr_set_pause: null env");
    if (pause) e->P.flags |= qr::kFlagPause; else e->P.flags &= ~qr::kFlagPause;
    return QR_OK;
}

int qr_set_pause_if_collision(qr_env* e, int32_t on) {
    if (!e) return fail(QR_E_INVALID, "qr_set_pause_if_collision: null env");
    e->cfg.pause_if_collision = on ? 1 : 0;
    if (on) e->P.flags |= qr::kFlagPauseIfCollision; else e->P.flags &= ~qr::kFlagPauseIfCollision;
    return QR_OK;
}

int qr_set_terminal_obs(qr_env* e, float* term_obs_dev, int32_t rows) {
    if (!e) return fail(QR_E_INVALID, "qr_set_terminal_obs: null env");
    if (term_obs_dev && rows < 1) return fail(QR_E_INVALID, "qr_set_terminal_obs: rows must be >= 1");
    e->P.term_obs = term_obs_dev;
    e->term_rows = term_obs_dev ? rows : 0;
    return QR_OK;
}

int qr_seed(qr_env* e, uint64_t seed) {
    if (!e) return fail(QR_E_INVALID, "qr_seed: null env");
    QR_HIP(hipSetDevice(e->cfg.device));
    e->P.seed_lo = (uint32_t)seed;
    e->P.seed_hi = (uint32_t)(seed >> 32);
    QR_HIP(qr::launch_clear_episode(e->P, nullptr));
    QR_HIP(hipStreamSynchronize(nullptr));
    return QR_OK;
}

int qr_reset(qr_env* e, const uint8_t* mask_dev, float* obs_out_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    QR_HIP(qr::launch_reset(e->cfg.variant, e->P, mask_dev, obs_out_dev, (hipStream_t)stream));
    return QR_OK;
}

int qr_step(qr_env* e, const float* actions_dev, float* obs_out_dev, float* rew_out_dev, uint8_t* done_out_dev,
            uint8_t* trunc_out_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (int rc = check_step_buffers(actions_dev, obs_out_dev, rew_out_dev, done_out_dev, "qr_step")) return rc;
    QR_HIP(qr::launch_step(e->cfg.variant, e->P, actions_dev, obs_out_dev, rew_out_dev, done_out_dev, trunc_out_dev,
                           (hipStream_t)stream));
    return QR_OK;
}

int qr_step_many(qr_env* e, int32_t K, const float* actions_dev, float* obs_out_dev, float* rew_out_dev,
                 uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (K < 1) return fail(QR_E_INVALID, "qr_step_many: num_steps must be >= 1");
    if (int rc = check_term_rows(e, K, "qr_step_many")) return rc;
    if (int rc = check_step_buffers(actions_dev, obs_out_dev, rew_out_dev, done_out_dev, "qr_step_many")) return rc;
    hipStream_t st = (hipStream_t)stream;
    // one launch: the fused rollout kernel keeps the env state in registers across the K steps
    return QR_TIMED_LAUNCH(e, st, qr::launch_rollout(e->cfg.variant, e->P, e->rollout_form, K, actions_dev, obs_out_dev, rew_out_dev, done_out_dev,
                                                      trunc_out_dev, st));
}

int qr_step_launches(qr_env* e, int32_t K, const float* actions_dev, float* obs_out_dev, float* rew_out_dev,
                     uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (K < 1) return fail(QR_E_INVALID, "qr_step_launches: num_steps must be >= 1");
    if (int rc = check_term_rows(e, K, "qr_step_launches")) return rc;
    if (int rc = check_step_buffers(actions_dev, obs_out_dev, rew_out_dev, done_out_dev, "qr_step_launches")) return rc;
    hipStream_t st = (hipStream_t)stream;
    // a caller that is itself capturing `stream` into a graph gets plain kernel nodes (a graph launch cannot be captured)
    if (qr::stream_is_capturing(st)) {
        for (int k = 0; k < K; ++k) QR_HIP(launch_step_row(e, k, actions_dev, obs_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, st));
        e->timing_valid = false;
        return QR_OK;
    }
    qr_env::StepGraph& g = e->sg;
    const bool hit = g.exec && g.K == K && g.act == actions_dev && g.obs == obs_out_dev && g.rew == rew_out_dev &&
                     g.done == done_out_dev && g.trunc == trunc_out_dev && std::memcmp(&g.P, &e->P, sizeof(e->P)) == 0;
    if (!hit) {  // (re)capture: K kernel nodes in a chain; kernel parameters (incl. Params) are baked into the nodes
        if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
        if (!e->capture_stream) QR_HIP(hipStreamCreateWithFlags(&e->capture_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        QR_HIP(hipStreamBeginCapture(e->capture_stream, hipStreamCaptureModeThreadLocal));
        hipError_t err = hipSuccess;
        for (int k = 0; k < K && err == hipSuccess; ++k)
            err = launch_step_row(e, k, actions_dev, obs_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, e->capture_stream);
        const hipError_t end = hipStreamEndCapture(e->capture_stream, &graph);
        if (err != hipSuccess || end != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return fail(QR_E_HIP, std::string("qr_step_launches: graph capture failed: ") +
                                      hipGetErrorString(err != hipSuccess ? err : end));
        }
        const hipError_t inst = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (inst != hipSuccess) {
            g.exec = nullptr;
            return fail(QR_E_HIP, std::string("qr_step_launches: hipGraphInstantiate: ") + hipGetErrorString(inst));
        }
        g.K = K; g.act = actions_dev; g.obs = obs_out_dev; g.rew = rew_out_dev; g.done = done_out_dev; g.trunc = trunc_out_dev;
        std::memcpy(&g.P, &e->P, sizeof(e->P));  // byte copy: compared with memcmp above
    }
    return QR_TIMED_LAUNCH(e, st, hipGraphLaunch(g.exec, st));
}

// What qr_rollout_policy and qr_rollout_policy_conditions refuse about their shared arguments and the handle's mode, in one order; on
// success A holds the weights and the sampling arguments of the launch.  history: null, or the command history of
// qr_rollout_policy_history -- its range is refused directly before the observation length, which is then the env's + 4 * history.
// critic: null, or the two buffers of qr_rollout_policy_privileged -- its range of history starts at 0, and a NULL or misaligned
// critic_obs_out_dev is refused directly behind the buffers of check_rollout_common.
struct CriticRows { float* obs; float* last_obs; };
static int check_history(const qr_env* e, int history, const char* who, int lowest = 1) {
    if (history < lowest || history > 4 - e->cfg.gates_ahead)
        return fail(QR_E_INVALID, std::string(who) + ": history must be in [" + std::to_string(lowest) + ", 4 - gates_ahead] (the row of obs_len + 4 * history floats must be a "
                                                     "length the policy kernels have: gates_ahead + history <= 4)");
    return QR_OK;
}
static int rollout_policy_args(const qr_env* e, qr_policy* policy, int K, const float* log_std, uint64_t noise_seed, uint64_t first_step,
                               int flags, const float* obs_out_dev, const float* act_out_dev, const float* logp_out_dev,
                               const float* rew_out_dev, const uint8_t* done_out_dev, const char* who, qr::PolicyArgs& A,
                               const int32_t* history = nullptr, const CriticRows* critic = nullptr) {
    if (int rc = check_rollout_common(e, K, policy && log_std, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, who)) return rc;
    if (critic) {
        if (!critic->obs) return fail(QR_E_INVALID, std::string(who) + ": critic_obs_out_dev is required");
        if (((uintptr_t)critic->obs & 15) || ((uintptr_t)critic->last_obs & 15))
            return fail(QR_E_INVALID, std::string(who) + ": critic_obs_out_dev and critic_last_obs_dev must be 16-byte aligned");
    }
    A = qr::PolicyArgs{};
    if (int rc = qr::fetch_policy_weights(policy, who, A.weights)) return rc;
    if (history) {
        if (int rc = check_history(e, *history, who, critic ? 0 : 1)) return rc;
        if (int rc = qr::check_policy_handle(policy, e->L + 4 * *history, e->cfg.device, who, "!= env obs_len + 4 * history")) return rc;
    } else if (int rc = qr::check_policy_handle(policy, e->L, e->cfg.device, who)) {
        return rc;
    }
    if (flags < 0 || flags > (QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS))
        return fail(QR_E_INVALID, std::string(who) + ": `deterministic` takes QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS");
    A.weights_lo = qr::policy_weights_lo(policy);
    qr::set_sampling(A, qr::sampling_entry(log_std, noise_seed), first_step, flags);
    return QR_OK;
}

int qr_rollout_policy(qr_env* e, qr_policy* policy, int32_t K, const float* log_std, uint64_t noise_seed,
                      uint64_t first_step, int32_t deterministic, float* obs_out_dev, float* act_out_dev,
                      float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                      float* last_obs_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    qr::PolicyArgs A{};
    if (int rc = rollout_policy_args(e, policy, K, log_std, noise_seed, first_step, deterministic, obs_out_dev, act_out_dev, logp_out_dev,
                                     rew_out_dev, done_out_dev, "qr_rollout_policy", A))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    return QR_TIMED_LAUNCH(e, st, qr::launch_rollout_policy(e->cfg.variant, e->P, A, K, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev,
                                                             done_out_dev, trunc_out_dev, last_obs_dev, st));
}

int qr_evaluate_policy(qr_env* e, qr_policy* policy, int32_t K, int32_t gates_per_lap, int32_t flags, int32_t* rec_dev,
                       float* recf_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (!policy) return fail(QR_E_INVALID, "qr_evaluate_policy: null policy handle");
    if (int rc = check_eval_args(e, K, &gates_per_lap, flags, rec_dev, recf_dev, "qr_evaluate_policy")) return rc;
    if (int rc = qr::check_policy_handle(policy, e->L, e->cfg.device, "qr_evaluate_policy")) return rc;
    qr::PolicyArgs A{};   // no sampling: only the weight images are read
    if (int rc = qr::fetch_policy_weights(policy, "qr_evaluate_policy", A.weights)) return rc;
    A.weights_lo = qr::policy_weights_lo(policy);
    A.f32class = (flags & QR_ROLLOUT_F32CLASS) ? 1 : 0;
    A.deterministic = 1;
    hipStream_t st = (hipStream_t)stream;
    return QR_TIMED_LAUNCH(e, st, qr::launch_eval_policy(e->cfg.variant, e->P, A, K, gates_per_lap, rec_dev, recf_dev, st));
}

// The refusals come first and in full: nothing is enqueued (no event, no launch) unless every argument is valid.
int qr_evaluate_policy_bank(qr_env* e, qr_policy_bank* bank, int32_t num_policies, int32_t envs_per_policy, int32_t K,
                            int32_t gates_per_lap, int32_t flags, int32_t* rec_dev, float* recf_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (!bank) return fail(QR_E_INVALID, "qr_evaluate_policy_bank: null bank handle");
    if (int rc = check_eval_args(e, K, &gates_per_lap, flags, rec_dev, recf_dev, "qr_evaluate_policy_bank")) return rc;
    if (int rc = qr::check_policy_bank(bank, e->L, e->cfg.device, "qr_evaluate_policy_bank", "bank")) return rc;
    if (num_policies < 1 || num_policies > qr::bank_capacity(bank))
        return fail(QR_E_INVALID, "qr_evaluate_policy_bank: num_policies must be in 1..capacity");
    if (int rc = check_group_shape(e, num_policies, envs_per_policy, "num_policies", "policy", "qr_evaluate_policy_bank")) return rc;
    const int unset = qr::bank_first_unset(bank, num_policies);
    if (unset >= 0) return fail(QR_E_STATE, "qr_evaluate_policy_bank: slot " + std::to_string(unset) + " of the bank has no weights");
    hipStream_t st = (hipStream_t)stream;
    return QR_TIMED_LAUNCH(e, st, qr::launch_eval_policy_bank(e->cfg.variant, e->P, qr::bank_weights(bank), qr::bank_weights_lo(bank), (flags & QR_ROLLOUT_F32CLASS) != 0,
                                       num_policies, envs_per_policy, K, gates_per_lap, rec_dev, recf_dev, st));
}

// ---- bank of flight conditions (qr_evaluate_policy_grid) ----
int qr_condition_bank_create(int32_t variant, int32_t device, int32_t capacity, qr_condition_bank** out) {
    if (!out) return fail(QR_E_INVALID, "qr_condition_bank_create: null output");
    *out = nullptr;
    if (variant != QR_VARIANT_E2E && variant != QR_VARIANT_INDI) return fail(QR_E_INVALID, "qr_condition_bank_create: unknown variant");
    if (capacity < 1) return fail(QR_E_INVALID, "qr_condition_bank_create: capacity must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(QR_E_NO_DEVICE, "qr_condition_bank_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(QR_E_INVALID, "qr_condition_bank_create: bad device ordinal");
    QR_HIP(hipSetDevice(device));
    qr_condition_bank* b = new qr_condition_bank();
    b->variant = variant;
    b->device = device;
    b->capacity = capacity;
    b->is_set.assign((size_t)capacity, 0);
    const size_t bytes = (size_t)capacity * qr::kCondSlotFloats * sizeof(float);
    if (hipMalloc((void**)&b->d_slots, bytes) != hipSuccess) {
        delete b;
        return fail(QR_E_HIP, "qr_condition_bank_create: hipMalloc failed");
    }
    (void)hipMemset(b->d_slots, 0, bytes);
    *out = b;
    return QR_OK;
}

int qr_condition_bank_destroy(qr_condition_bank* b) {
    if (!b) return QR_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    if (b->d_slots) (void)hipFree(b->d_slots);
    delete b;
    return QR_OK;
}

int qr_condition_bank_capacity(const qr_condition_bank* b) { return b ? b->capacity : fail(QR_E_INVALID, "qr_condition_bank_capacity: null bank"); }

int qr_condition_bank_set(qr_condition_bank* b, int32_t slot, const float* gate_pos, const float* gate_yaw, int32_t G, const float* start_pos,
                          const float* dist_ranges, float dist_scale, int32_t max_steps, int32_t gates_per_lap) {
    if (!b) return fail(QR_E_INVALID, "qr_condition_bank_set: null bank");
    if (!gate_pos || !gate_yaw || !start_pos) return fail(QR_E_INVALID, "qr_condition_bank_set: null track argument");
    if (slot < 0 || slot >= b->capacity) return fail(QR_E_INVALID, "qr_condition_bank_set: slot must be in [0, capacity)");
    if (G < 2 || G > QR_MAX_GATES) return fail(QR_E_INVALID, "qr_condition_bank_set: num_gates must be in 2..QR_MAX_GATES (the evaluators need two gates)");
    if (gates_per_lap < 1) return fail(QR_E_INVALID, "qr_condition_bank_set: gates_per_lap must be >= 1");
    if (dist_ranges && b->variant != QR_VARIANT_E2E)
        return fail(QR_E_INVALID, "qr_condition_bank_set: dist_ranges must be NULL for the INDI variant (it has no disturbances)");
    // NULL ranges = a handle on which qr_set_disturbance was never called: all-zero ranges, scale 1
    float dist_lo[6] = {}, dist_hi[6] = {};
    if (dist_ranges)
        for (int k = 0; k < 6; ++k) {
            dist_lo[k] = dist_ranges[2 * k + 0];
            dist_hi[k] = dist_ranges[2 * k + 1];
        }
    else
        dist_scale = 1.0f;
    std::vector<float> host(qr::kCondSlotFloats, 0.0f);
    qr::CondHeader h{};
    h.num_gates = G;
    h.max_steps = max_steps;
    h.gates_per_lap = gates_per_lap;
    condition_obs_scale(dist_lo, dist_hi, h.obs_lo, h.obs_inv);
    std::memcpy(host.data(), &h, sizeof(h));
    std::vector<float> pos_rel(3 * (size_t)G), yaw_rel((size_t)G);
    gate_relative_table(gate_pos, gate_yaw, G, pos_rel.data(), yaw_rel.data());
    build_condition_image(b->variant, start_pos, dist_lo, dist_hi, dist_scale, G, gate_pos, gate_yaw, pos_rel.data(), yaw_rel.data(),
                          host.data() + qr::kCondHeaderFloats);
    QR_HIP(hipSetDevice(b->device));
    QR_HIP(hipDeviceSynchronize());   // a launch may still read the slot
    if (hipMemcpy(b->d_slots + (size_t)slot * qr::kCondSlotFloats, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        b->is_set[(size_t)slot] = 0;
        return fail(QR_E_HIP, "qr_condition_bank_set: upload failed");
    }
    b->is_set[(size_t)slot] = 1;
    return QR_OK;
}

// The refusals come first and in full: nothing is enqueued or copied unless every argument is valid, and no index reaches the device
// that has not been checked against its bank here.
int qr_evaluate_policy_grid(qr_env* e, qr_policy_bank* policies, qr_condition_bank* conditions, int32_t num_groups, int32_t envs_per_group,
                            const int32_t* policy_of_group, const int32_t* condition_of_group, int32_t K, int32_t flags, int32_t* rec_dev,
                            float* recf_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (!policies) return fail(QR_E_INVALID, "qr_evaluate_policy_grid: null policy bank handle");
    if (!conditions) return fail(QR_E_INVALID, "qr_evaluate_policy_grid: null condition bank handle");
    if (!policy_of_group || !condition_of_group) return fail(QR_E_INVALID, "qr_evaluate_policy_grid: the two group maps are required");
    if (int rc = check_eval_args(e, K, nullptr, flags, rec_dev, recf_dev, "qr_evaluate_policy_grid")) return rc;
    const char* who = "qr_evaluate_policy_grid";
    if (int rc = qr::check_policy_bank(policies, e->L, e->cfg.device, who)) return rc;
    if (int rc = check_condition_groups(e, conditions, num_groups, envs_per_group, who)) return rc;
    if (int rc = check_group_indices(policies, policy_of_group, conditions, condition_of_group, num_groups, who)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_group_map(e, policy_of_group, condition_of_group, num_groups, st, who)) return rc;
    return QR_TIMED_LAUNCH(e, st, qr::launch_eval_policy_grid(e->cfg.variant, e->P, qr::bank_weights(policies), qr::bank_weights_lo(policies), conditions->d_slots,
                                       e->group_map.d, (flags & QR_ROLLOUT_F32CLASS) != 0, num_groups, envs_per_group, K, rec_dev, recf_dev, st));
}

// ---- bank of vehicles (qr_evaluate_policy_dynamics_grid) ----
int qr_dynamics_count(int32_t variant) {
    int count = 0;
    if (!qr::dynamics_nominal(variant, &count)) return fail(QR_E_INVALID, "qr_dynamics_count: unknown variant");
    return count;
}

int qr_dynamics_nominal(int32_t variant, float* out, int32_t count) {
    int n = 0;
    const float* table = qr::dynamics_nominal(variant, &n);
    if (!table) return fail(QR_E_INVALID, "qr_dynamics_nominal: unknown variant");
    if (!out) return fail(QR_E_INVALID, "qr_dynamics_nominal: null output");
    if (count != n) return fail(QR_E_INVALID, "qr_dynamics_nominal: count must equal qr_dynamics_count(variant)");
    std::memcpy(out, table, (size_t)n * sizeof(float));
    return QR_OK;
}

int qr_dynamics_bank_create(int32_t variant, int32_t device, int32_t capacity, qr_dynamics_bank** out) {
    if (!out) return fail(QR_E_INVALID, "qr_dynamics_bank_create: null output");
    *out = nullptr;
    if (variant != QR_VARIANT_E2E && variant != QR_VARIANT_INDI) return fail(QR_E_INVALID, "qr_dynamics_bank_create: unknown variant");
    if (capacity < 1) return fail(QR_E_INVALID, "qr_dynamics_bank_create: capacity must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(QR_E_NO_DEVICE, "qr_dynamics_bank_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(QR_E_INVALID, "qr_dynamics_bank_create: bad device ordinal");
    QR_HIP(hipSetDevice(device));
    qr_dynamics_bank* b = new qr_dynamics_bank();
    b->variant = variant;
    b->device = device;
    b->capacity = capacity;
    b->is_set.assign((size_t)capacity, 0);
    const size_t bytes = (size_t)capacity * qr::kDynSlotFloats * sizeof(float);
    if (hipMalloc((void**)&b->d_slots, bytes) != hipSuccess) {
        delete b;
        return fail(QR_E_HIP, "qr_dynamics_bank_create: hipMalloc failed");
    }
    (void)hipMemset(b->d_slots, 0, bytes);
    *out = b;
    return QR_OK;
}

int qr_dynamics_bank_destroy(qr_dynamics_bank* b) {
    if (!b) return QR_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    if (b->d_slots) (void)hipFree(b->d_slots);
    delete b;
    return QR_OK;
}

int qr_dynamics_bank_capacity(const qr_dynamics_bank* b) { return b ? b->capacity : fail(QR_E_INVALID, "qr_dynamics_bank_capacity: null bank"); }

int qr_dynamics_bank_set(qr_dynamics_bank* b, int32_t slot, const float* coeffs, int32_t count) {
    if (!b) return fail(QR_E_INVALID, "qr_dynamics_bank_set: null bank");
    if (slot < 0 || slot >= b->capacity) return fail(QR_E_INVALID, "qr_dynamics_bank_set: slot must be in [0, capacity)");
    int n = 0;
    const float* nominal = qr::dynamics_nominal(b->variant, &n);
    if (count != n) return fail(QR_E_INVALID, "qr_dynamics_bank_set: count must equal qr_dynamics_count of the bank's variant");
    const float* src = coeffs ? coeffs : nominal;   // NULL = the nominal vehicle
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(src[k])) return fail(QR_E_INVALID, "qr_dynamics_bank_set: coefficient " + std::to_string(k) + " is not finite");
    float host[qr::kDynSlotFloats] = {};
    std::memcpy(host, src, (size_t)n * sizeof(float));
    QR_HIP(hipSetDevice(b->device));
    QR_HIP(hipDeviceSynchronize());   // a launch may still read the slot
    if (hipMemcpy(b->d_slots + (size_t)slot * qr::kDynSlotFloats, host, sizeof(host), hipMemcpyHostToDevice) != hipSuccess) {
        b->is_set[(size_t)slot] = 0;
        return fail(QR_E_HIP, "qr_dynamics_bank_set: upload failed");
    }
    b->is_set[(size_t)slot] = 1;
    return QR_OK;
}

int qr_dynamics_bank_read(const qr_dynamics_bank* b, int32_t slot, float* out, int32_t count) {
    if (!b) return fail(QR_E_INVALID, "qr_dynamics_bank_read: null bank");
    if (!out) return fail(QR_E_INVALID, "qr_dynamics_bank_read: null output");
    if (slot < 0 || slot >= b->capacity) return fail(QR_E_INVALID, "qr_dynamics_bank_read: slot must be in [0, capacity)");
    int n = 0;
    (void)qr::dynamics_nominal(b->variant, &n);
    if (count != n) return fail(QR_E_INVALID, "qr_dynamics_bank_read: count must equal qr_dynamics_count of the bank's variant");
    if (!b->is_set[(size_t)slot]) return fail(QR_E_STATE, "qr_dynamics_bank_read: slot " + std::to_string(slot) + " of the dynamics bank was never set");
    QR_HIP(hipSetDevice(b->device));
    QR_HIP(hipDeviceSynchronize());
    QR_HIP(hipMemcpy(out, b->d_slots + (size_t)slot * qr::kDynSlotFloats, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return QR_OK;
}

// qr_evaluate_policy_grid with a third bank and a third map: the same refusals in the same order, the dynamics bank's next to the
// condition bank's.  Nothing is enqueued or copied unless every argument is valid.
int qr_evaluate_policy_dynamics_grid(qr_env* e, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics, int32_t num_groups,
                                     int32_t envs_per_group, const int32_t* policy_of_group, const int32_t* condition_of_group,
                                     const int32_t* dynamics_of_group, int32_t K, int32_t flags, int32_t* rec_dev, float* recf_dev, void* stream) {
    const char* who = "qr_evaluate_policy_dynamics_grid";
    const std::string w = std::string(who) + ": ";
    if (int rc = check_ready(e)) return rc;
    if (!policies) return fail(QR_E_INVALID, w + "null policy bank handle");
    if (!conditions) return fail(QR_E_INVALID, w + "null condition bank handle");
    if (!dynamics) return fail(QR_E_INVALID, w + "null dynamics bank handle");
    if (!policy_of_group || !condition_of_group || !dynamics_of_group) return fail(QR_E_INVALID, w + "the three group maps are required");
    if (int rc = check_eval_args(e, K, nullptr, flags, rec_dev, recf_dev, who)) return rc;
    if (int rc = qr::check_policy_bank(policies, e->L, e->cfg.device, who)) return rc;
    if (int rc = check_condition_groups(e, conditions, num_groups, envs_per_group, who)) return rc;
    if (int rc = check_dynamics_bank(e, dynamics, who)) return rc;
    if (int rc = check_group_indices(policies, policy_of_group, conditions, condition_of_group, num_groups, who)) return rc;
    if (int rc = check_dynamics_indices(dynamics, dynamics_of_group, num_groups, who)) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int4> map((size_t)num_groups);
    for (int g = 0; g < num_groups; ++g) map[(size_t)g] = make_int4(policy_of_group[g], condition_of_group[g], dynamics_of_group[g], 0);
    if (int rc = upload_table(e->dyn_map, map, st, who, "group map", "this map")) return rc;
    return QR_TIMED_LAUNCH(e, st, qr::launch_eval_policy_dynamics_grid(e->cfg.variant, e->P, qr::bank_weights(policies), qr::bank_weights_lo(policies),
                                       conditions->d_slots, dynamics->d_slots, e->dyn_map.d, (flags & QR_ROLLOUT_F32CLASS) != 0, num_groups,
                                       envs_per_group, K, rec_dev, recf_dev, st));
}

// ---- bank of sensors (qr_evaluate_policy_sensing_grid) ----
int qr_sensing_bank_create(int32_t device, int32_t capacity, qr_sensing_bank** out) {
    if (!out) return fail(QR_E_INVALID, "qr_sensing_bank_create: null output");
    *out = nullptr;
    if (capacity < 1) return fail(QR_E_INVALID, "qr_sensing_bank_create: capacity must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(QR_E_NO_DEVICE, "qr_sensing_bank_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(QR_E_INVALID, "qr_sensing_bank_create: bad device ordinal");
    QR_HIP(hipSetDevice(device));
    qr_sensing_bank* b = new qr_sensing_bank();
    b->device = device;
    b->capacity = capacity;
    b->is_set.assign((size_t)capacity, 0);
    const size_t bytes = (size_t)capacity * qr::kSensingSlotFloats * sizeof(float);
    if (hipMalloc((void**)&b->d_slots, bytes) != hipSuccess) {
        delete b;
        return fail(QR_E_HIP, "qr_sensing_bank_create: hipMalloc failed");
    }
    (void)hipMemset(b->d_slots, 0, bytes);
    *out = b;
    return QR_OK;
}

int qr_sensing_bank_destroy(qr_sensing_bank* b) {
    if (!b) return QR_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    if (b->d_slots) (void)hipFree(b->d_slots);
    delete b;
    return QR_OK;
}

int qr_sensing_bank_capacity(const qr_sensing_bank* b) { return b ? b->capacity : fail(QR_E_INVALID, "qr_sensing_bank_capacity: null bank"); }

int qr_sensing_bank_set(qr_sensing_bank* b, int32_t slot, const float* sigma8, int32_t delay) {
    if (!b) return fail(QR_E_INVALID, "qr_sensing_bank_set: null bank");
    if (slot < 0 || slot >= b->capacity) return fail(QR_E_INVALID, "qr_sensing_bank_set: slot must be in [0, capacity)");
    float host[qr::kSensingSlotFloats] = {};   // NULL = the ideal sensor: no noise
    for (int k = 0; k < 8 && sigma8; ++k) {
        if (!std::isfinite(sigma8[k]) || sigma8[k] < 0.0f)
            return fail(QR_E_INVALID, "qr_sensing_bank_set: sigma " + std::to_string(k) + " must be finite and >= 0");
        host[k] = sigma8[k] == 0.0f ? 0.0f : sigma8[k];   // (-0.0f -> +0.0f)
    }
    if (delay < 0 || delay > qr::kMaxDelay) return fail(QR_E_INVALID, "qr_sensing_bank_set: delay must be in [0, 4]");
    std::memcpy(&host[8], &delay, sizeof(delay));
    QR_HIP(hipSetDevice(b->device));
    QR_HIP(hipDeviceSynchronize());   // a launch may still read the slot
    if (hipMemcpy(b->d_slots + (size_t)slot * qr::kSensingSlotFloats, host, sizeof(host), hipMemcpyHostToDevice) != hipSuccess) {
        b->is_set[(size_t)slot] = 0;
        return fail(QR_E_HIP, "qr_sensing_bank_set: upload failed");
    }
    b->is_set[(size_t)slot] = 1;
    return QR_OK;
}

int qr_sensing_bank_read(const qr_sensing_bank* b, int32_t slot, float* sigma8, int32_t* delay) {
    if (!b) return fail(QR_E_INVALID, "qr_sensing_bank_read: null bank");
    if (!sigma8 || !delay) return fail(QR_E_INVALID, "qr_sensing_bank_read: null output");
    if (slot < 0 || slot >= b->capacity) return fail(QR_E_INVALID, "qr_sensing_bank_read: slot must be in [0, capacity)");
    if (!b->is_set[(size_t)slot]) return fail(QR_E_STATE, "qr_sensing_bank_read: slot " + std::to_string(slot) + " of the sensing bank was never set");
    float host[9];
    QR_HIP(hipSetDevice(b->device));
    QR_HIP(hipDeviceSynchronize());
    QR_HIP(hipMemcpy(host, b->d_slots + (size_t)slot * qr::kSensingSlotFloats, sizeof(host), hipMemcpyDeviceToHost));
    std::memcpy(sigma8, host, 8 * sizeof(float));
    std::memcpy(delay, &host[8], sizeof(int32_t));
    return QR_OK;
}

// the Philox counter of the observation noise keeps 56 bits of the step: its top byte carries the block number
static bool sensing_steps_fit(uint64_t first_step, int K) {
    const uint64_t limit = (uint64_t)1 << 56;
    return first_step <= limit && (uint64_t)K <= limit - first_step;
}

// qr_evaluate_policy_dynamics_grid with a fourth bank and a fourth map: its refusals in its order, then the sensing bank's.  Nothing is
// enqueued or copied unless every argument is valid.  history: null (qr_evaluate_policy_sensing_grid), or the command history of
// qr_evaluate_policy_history_grid: its range is refused directly before the bank's observation length, which is then the env's + 4 * history.
// bb: null, or the black box of qr_blackbox_policy_grid: history may then be 0, and the black box's own refusals (qr_blackbox_policy's, in
// its order and wording) follow everything the evaluator refuses.
struct BlackboxGridCall {
    int32_t trigger, window, rec_per_group;
    float* ring_dev;
    int32_t* st_dev;
    float* term_dev;
};
static int evaluate_policy_sensing_grid(const char* who, const int32_t* history, qr_env* e, qr_policy_bank* policies, qr_condition_bank* conditions,
                                        qr_dynamics_bank* dynamics, qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group,
                                        const int32_t* policy_of_group, const int32_t* condition_of_group, const int32_t* dynamics_of_group,
                                        const int32_t* sensing_of_group, int32_t K, int32_t flags, uint64_t noise_seed, uint64_t first_step,
                                        float* pending_dev, int32_t* rec_dev, float* recf_dev, void* stream,
                                        const BlackboxGridCall* bb = nullptr) {
    const std::string w = std::string(who) + ": ";
    if (int rc = check_ready(e)) return rc;
    if (!policies) return fail(QR_E_INVALID, w + "null policy bank handle");
    if (!conditions) return fail(QR_E_INVALID, w + "null condition bank handle");
    if (!dynamics) return fail(QR_E_INVALID, w + "null dynamics bank handle");
    if (!policy_of_group || !condition_of_group || !dynamics_of_group) return fail(QR_E_INVALID, w + "the three group maps are required");
    if (int rc = check_eval_args(e, K, nullptr, flags, rec_dev, recf_dev, who)) return rc;
    if (history && bb && *history == 0) {
        if (int rc = qr::check_policy_bank(policies, e->L, e->cfg.device, who)) return rc;
    } else if (history) {
        if (int rc = check_history(e, *history, who, bb ? 0 : 1)) return rc;
        if (int rc = qr::check_policy_bank(policies, e->L + 4 * *history, e->cfg.device, who, "policy bank", "!= env obs_len + 4 * history")) return rc;
    } else if (int rc = qr::check_policy_bank(policies, e->L, e->cfg.device, who)) {
        return rc;
    }
    if (int rc = check_condition_groups(e, conditions, num_groups, envs_per_group, who)) return rc;
    if (int rc = check_dynamics_bank(e, dynamics, who)) return rc;
    if (int rc = check_group_indices(policies, policy_of_group, conditions, condition_of_group, num_groups, who)) return rc;
    if (int rc = check_dynamics_indices(dynamics, dynamics_of_group, num_groups, who)) return rc;
    // the sensing bank's own
    if (!sensing) return fail(QR_E_INVALID, w + "null sensing bank handle");
    if (!sensing_of_group) return fail(QR_E_INVALID, w + "sensing_of_group is required");
    if (!pending_dev) return fail(QR_E_INVALID, w + "pending_dev is required");
    if ((uintptr_t)pending_dev & 15) return fail(QR_E_INVALID, w + "pending_dev must be 16-byte aligned");
    if (sensing->device != e->cfg.device) return fail(QR_E_INVALID, w + "sensing bank on another GPU");
    for (int g = 0; g < num_groups; ++g)
        if (sensing_of_group[g] < 0 || sensing_of_group[g] >= sensing->capacity)
            return fail(QR_E_INVALID, w + "sensing_of_group[" + std::to_string(g) + "] is outside the sensing bank");
    if (!sensing_steps_fit(first_step, K)) return fail(QR_E_INVALID, w + "first_step + num_steps must not exceed 2^56");
    for (int g = 0; g < num_groups; ++g)
        if (!sensing->is_set[(size_t)sensing_of_group[g]])
            return fail(QR_E_STATE, w + "slot " + std::to_string(sensing_of_group[g]) + " of the sensing bank was never set");
    if (bb) {   // the black box's own, as qr_blackbox_policy words them (num_steps and the flags are the evaluator's, above)
        if (!bb->ring_dev || !bb->st_dev) return fail(QR_E_INVALID, w + "ring_dev and st_dev are required");
        if (((uintptr_t)bb->ring_dev | (uintptr_t)bb->st_dev) & 15) return fail(QR_E_INVALID, w + "ring_dev and st_dev must be 16-byte aligned");
        if ((uintptr_t)bb->term_dev & 3) return fail(QR_E_INVALID, w + "term_dev must be 4-byte aligned");
        if (bb->rec_per_group < 1 || bb->rec_per_group > envs_per_group) return fail(QR_E_INVALID, w + "rec_per_group must be in 1..envs_per_group");
        if (bb->trigger < 0 || bb->trigger > (QR_BLACKBOX_ON_CRASH | QR_BLACKBOX_ON_TIME_LIMIT))
            return fail(QR_E_INVALID, w + "`trigger` takes QR_BLACKBOX_ON_CRASH | QR_BLACKBOX_ON_TIME_LIMIT");
        if (bb->window < 1) return fail(QR_E_INVALID, w + "window must be >= 1");
    }
    hipStream_t st = (hipStream_t)stream;
    std::vector<int4> map((size_t)num_groups);
    for (int g = 0; g < num_groups; ++g)
        map[(size_t)g] = make_int4(policy_of_group[g], condition_of_group[g], dynamics_of_group[g], sensing_of_group[g]);
    if (int rc = upload_table(e->sen_map, map, st, who, "group map", "this map")) return rc;
    if (bb) {
        const int slot0 = (int)(first_step % (uint64_t)bb->window);   // the ring slot of the call's first step
        return QR_TIMED_LAUNCH(e, st, qr::launch_blackbox_policy_grid(e->cfg.variant, e->P, qr::bank_weights(policies), qr::bank_weights_lo(policies),
                                           conditions->d_slots, dynamics->d_slots, sensing->d_slots, e->sen_map.d, *history,
                                           (flags & QR_ROLLOUT_F32CLASS) != 0, num_groups, envs_per_group, K, noise_seed, first_step, pending_dev, rec_dev,
                                           recf_dev, bb->trigger, bb->window, bb->rec_per_group, slot0, bb->ring_dev, bb->st_dev, bb->term_dev, st));
    }
    if (history)
        return QR_TIMED_LAUNCH(e, st, qr::launch_eval_policy_history_grid(e->cfg.variant, e->P, qr::bank_weights(policies), qr::bank_weights_lo(policies),
                                           conditions->d_slots, dynamics->d_slots, sensing->d_slots, e->sen_map.d, *history,
                                           (flags & QR_ROLLOUT_F32CLASS) != 0, num_groups, envs_per_group, K, noise_seed, first_step, pending_dev, rec_dev,
                                           recf_dev, st));
    return QR_TIMED_LAUNCH(e, st, qr::launch_eval_policy_sensing_grid(e->cfg.variant, e->P, qr::bank_weights(policies), qr::bank_weights_lo(policies),
                                       conditions->d_slots, dynamics->d_slots, sensing->d_slots, e->sen_map.d, (flags & QR_ROLLOUT_F32CLASS) != 0,
                                       num_groups, envs_per_group, K, noise_seed, first_step, pending_dev, rec_dev, recf_dev, st));
}

int qr_evaluate_policy_sensing_grid(qr_env* e, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                                    qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* policy_of_group,
                                    const int32_t* condition_of_group, const int32_t* dynamics_of_group, const int32_t* sensing_of_group, int32_t K,
                                    int32_t flags, uint64_t noise_seed, uint64_t first_step, float* pending_dev, int32_t* rec_dev, float* recf_dev,
                                    void* stream) {
    return evaluate_policy_sensing_grid("qr_evaluate_policy_sensing_grid", nullptr, e, policies, conditions, dynamics, sensing, num_groups, envs_per_group,
                                        policy_of_group, condition_of_group, dynamics_of_group, sensing_of_group, K, flags, noise_seed, first_step,
                                        pending_dev, rec_dev, recf_dev, stream);
}

// qr_evaluate_policy_sensing_grid for a bank of policies that observe their last `history` commands
int qr_evaluate_policy_history_grid(qr_env* e, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics,
                                    qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group, const int32_t* policy_of_group,
                                    const int32_t* condition_of_group, const int32_t* dynamics_of_group, const int32_t* sensing_of_group, int32_t history,
                                    int32_t K, int32_t flags, uint64_t noise_seed, uint64_t first_step, float* pending_dev, int32_t* rec_dev,
                                    float* recf_dev, void* stream) {
    return evaluate_policy_sensing_grid("qr_evaluate_policy_history_grid", &history, e, policies, conditions, dynamics, sensing, num_groups, envs_per_group,
                                        policy_of_group, condition_of_group, dynamics_of_group, sensing_of_group, K, flags, noise_seed, first_step,
                                        pending_dev, rec_dev, recf_dev, stream);
}

// the evaluator's launch (history 0: the sensing grid's) with the black box riding in the step loop
int qr_blackbox_policy_grid(qr_env* e, qr_policy_bank* policies, qr_condition_bank* conditions, qr_dynamics_bank* dynamics, qr_sensing_bank* sensing,
                            int32_t num_groups, int32_t envs_per_group, const int32_t* policy_of_group, const int32_t* condition_of_group,
                            const int32_t* dynamics_of_group, const int32_t* sensing_of_group, int32_t history, int32_t K, int32_t flags,
                            uint64_t noise_seed, uint64_t first_step, float* pending_dev, int32_t* rec_dev, float* recf_dev, int32_t trigger,
                            int32_t window, int32_t rec_per_group, float* ring_dev, int32_t* st_dev, float* term_dev, void* stream) {
    const BlackboxGridCall bb = {trigger, window, rec_per_group, ring_dev, st_dev, term_dev};
    return evaluate_policy_sensing_grid("qr_blackbox_policy_grid", &history, e, policies, conditions, dynamics, sensing, num_groups, envs_per_group,
                                        policy_of_group, condition_of_group, dynamics_of_group, sensing_of_group, K, flags, noise_seed, first_step,
                                        pending_dev, rec_dev, recf_dev, stream, &bb);
}

// the rows the evaluator adds to the observations of one group under one slot: refusals first, then one launch
int qr_sensing_noise(qr_env* e, qr_sensing_bank* sensing, int32_t slot, int32_t envs_per_group, int32_t K, uint64_t noise_seed, uint64_t first_step,
                     float* out_dev, void* stream) {
    const std::string w = "qr_sensing_noise: ";
    if (int rc = bind_device(e)) return rc;
    if (!sensing) return fail(QR_E_INVALID, w + "null sensing bank handle");
    if (!out_dev) return fail(QR_E_INVALID, w + "out_dev is required");
    if (envs_per_group < 1) return fail(QR_E_INVALID, w + "envs_per_group must be >= 1");
    if (K < 1 || K > 65535) return fail(QR_E_INVALID, w + "num_steps must be in [1, 65535]");
    if (sensing->device != e->cfg.device) return fail(QR_E_INVALID, w + "sensing bank on another GPU");
    if (slot < 0 || slot >= sensing->capacity) return fail(QR_E_INVALID, w + "slot is outside the sensing bank");
    if (!sensing_steps_fit(first_step, K)) return fail(QR_E_INVALID, w + "first_step + num_steps must not exceed 2^56");
    if (!sensing->is_set[(size_t)slot]) return fail(QR_E_STATE, w + "slot " + std::to_string(slot) + " of the sensing bank was never set");
    if (hipError_t err = qr::launch_sensing_noise(e->cfg.variant, e->P, sensing->d_slots + (size_t)slot * qr::kSensingSlotFloats, envs_per_group, K,
                                                  noise_seed, first_step, out_dev, (hipStream_t)stream))
        return fail(QR_E_HIP, w + hipGetErrorString(err));
    return QR_OK;
}

// The refusals come first and in full, as in qr_evaluate_policy_grid; the map travels in that call's (policy, condition) array with
// the policy half zero.
int qr_rollout_policy_conditions(qr_env* e, qr_policy* policy, qr_condition_bank* conditions, int32_t num_groups, int32_t envs_per_group,
                                 const int32_t* condition_of_group, int32_t K, const float* log_std, uint64_t noise_seed, uint64_t first_step,
                                 int32_t flags, float* obs_out_dev, float* act_out_dev, float* logp_out_dev, float* rew_out_dev,
                                 uint8_t* done_out_dev, uint8_t* trunc_out_dev, float* last_obs_dev, void* stream) {
    const char* who = "qr_rollout_policy_conditions";
    if (int rc = check_ready(e)) return rc;
    qr::PolicyArgs A{};
    if (int rc = rollout_policy_args(e, policy, K, log_std, noise_seed, first_step, flags, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev,
                                     done_out_dev, who, A))
        return rc;
    if (!conditions) return fail(QR_E_INVALID, "qr_rollout_policy_conditions: null condition bank handle");
    if (!condition_of_group) return fail(QR_E_INVALID, "qr_rollout_policy_conditions: the group map is required");
    if (int rc = check_condition_groups(e, conditions, num_groups, envs_per_group, who)) return rc;
    if (int rc = check_group_indices(nullptr, nullptr, conditions, condition_of_group, num_groups, who)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_group_map(e, nullptr, condition_of_group, num_groups, st, who)) return rc;
    return QR_TIMED_LAUNCH(e, st, qr::launch_rollout_policy_cond(e->cfg.variant, e->P, A, conditions->d_slots, e->group_map.d, num_groups, envs_per_group, K,
                                       obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, last_obs_dev, st));
}

// qr_rollout_policy_conditions with the dynamics bank and its map: that entry point's refusals in its order, then the dynamics bank's in
// the words of qr_evaluate_policy_dynamics_grid, then the copy of the map.  The pair travels in the (policy, condition) array of the
// handle, the dynamics slot in the half the single-policy kernel never read.
int qr_rollout_policy_dynamics(qr_env* e, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics, int32_t num_groups,
                               int32_t envs_per_group, const int32_t* condition_of_group, const int32_t* dynamics_of_group, int32_t K,
                               const float* log_std, uint64_t noise_seed, uint64_t first_step, int32_t flags, float* obs_out_dev, float* act_out_dev,
                               float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev, float* last_obs_dev,
                               void* stream) {
    const char* who = "qr_rollout_policy_dynamics";
    const std::string w = std::string(who) + ": ";
    if (int rc = check_ready(e)) return rc;
    qr::PolicyArgs A{};
    if (int rc = rollout_policy_args(e, policy, K, log_std, noise_seed, first_step, flags, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev,
                                     done_out_dev, who, A))
        return rc;
    if (!conditions) return fail(QR_E_INVALID, w + "null condition bank handle");
    if (!condition_of_group) return fail(QR_E_INVALID, w + "the condition map is required");
    if (int rc = check_condition_groups(e, conditions, num_groups, envs_per_group, who)) return rc;
    if (int rc = check_group_indices(nullptr, nullptr, conditions, condition_of_group, num_groups, who)) return rc;
    if (!dynamics) return fail(QR_E_INVALID, w + "null dynamics bank handle");
    if (!dynamics_of_group) return fail(QR_E_INVALID, w + "the dynamics map is required");
    if (int rc = check_dynamics_bank(e, dynamics, who)) return rc;
    if (int rc = check_dynamics_indices(dynamics, dynamics_of_group, num_groups, who)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_group_map(e, dynamics_of_group, condition_of_group, num_groups, st, who)) return rc;
    return QR_TIMED_LAUNCH(e, st, qr::launch_rollout_policy_dynamics(e->cfg.variant, e->P, A, conditions->d_slots, dynamics->d_slots, e->group_map.d, num_groups,
                                       envs_per_group, K, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev,
                                       last_obs_dev, st));
}

// qr_rollout_policy_dynamics with the sensing bank, its map and the command queues: that entry point's refusals in its order, then the
// sensing bank's in the words of qr_evaluate_policy_sensing_grid, then pending_dev, then the copy of the maps.  The (dynamics, condition)
// pair travels in the handle's group map as in qr_rollout_policy_dynamics, the sensing slots in an array of their own; under capture
// BOTH must already be on the device, and the test comes before either copy.  history: null (qr_rollout_policy_sensing), or the command
// history of qr_rollout_policy_history (rollout_policy_args refuses its range and compares the policy's length with the longer row).
// critic: null, or the two buffers of qr_rollout_policy_privileged (with history, which may then be 0).
static int rollout_policy_sensing(const char* who, const int32_t* history, qr_env* e, qr_policy* policy, qr_condition_bank* conditions,
                                  qr_dynamics_bank* dynamics, qr_sensing_bank* sensing, int32_t num_groups, int32_t envs_per_group,
                                  const int32_t* condition_of_group, const int32_t* dynamics_of_group, const int32_t* sensing_of_group, int32_t K,
                                  const float* log_std, uint64_t noise_seed, uint64_t first_step, int32_t flags, float* pending_dev, float* obs_out_dev,
                                  float* act_out_dev, float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                                  float* last_obs_dev, void* stream, const CriticRows* critic = nullptr) {
    const std::string w = std::string(who) + ": ";
    if (!e) return fail(QR_E_INVALID, w + "null env handle");
    if (int rc = check_ready(e)) return rc;
    qr::PolicyArgs A{};
    if (int rc = rollout_policy_args(e, policy, K, log_std, noise_seed, first_step, flags, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev,
                                     done_out_dev, who, A, history, critic))
        return rc;
    if (!conditions) return fail(QR_E_INVALID, w + "null condition bank handle");
    if (!condition_of_group) return fail(QR_E_INVALID, w + "the condition map is required");
    if (int rc = check_condition_groups(e, conditions, num_groups, envs_per_group, who)) return rc;
    if (int rc = check_group_indices(nullptr, nullptr, conditions, condition_of_group, num_groups, who)) return rc;
    if (!dynamics) return fail(QR_E_INVALID, w + "null dynamics bank handle");
    if (!dynamics_of_group) return fail(QR_E_INVALID, w + "the dynamics map is required");
    if (int rc = check_dynamics_bank(e, dynamics, who)) return rc;
    if (int rc = check_dynamics_indices(dynamics, dynamics_of_group, num_groups, who)) return rc;
    // the sensing bank's own
    if (!sensing) return fail(QR_E_INVALID, w + "null sensing bank handle");
    if (!sensing_of_group) return fail(QR_E_INVALID, w + "sensing_of_group is required");
    if (sensing->device != e->cfg.device) return fail(QR_E_INVALID, w + "sensing bank on another GPU");
    for (int g = 0; g < num_groups; ++g)
        if (sensing_of_group[g] < 0 || sensing_of_group[g] >= sensing->capacity)
            return fail(QR_E_INVALID, w + "sensing_of_group[" + std::to_string(g) + "] is outside the sensing bank");
    // last_obs carries the noise of step first_step + num_steps: that step, too, must fit the counter's 56 bits
    if (!sensing_steps_fit(first_step, K) || first_step + (uint64_t)K == (uint64_t)1 << 56)
        return fail(QR_E_INVALID, w + "first_step + num_steps must stay below 2^56");
    for (int g = 0; g < num_groups; ++g)
        if (!sensing->is_set[(size_t)sensing_of_group[g]])
            return fail(QR_E_STATE, w + "slot " + std::to_string(sensing_of_group[g]) + " of the sensing bank was never set");
    if (!pending_dev) return fail(QR_E_INVALID, w + "pending_dev is required");
    if ((uintptr_t)pending_dev & 15) return fail(QR_E_INVALID, w + "pending_dev must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int2> map((size_t)num_groups);
    std::vector<int> smap((size_t)num_groups);
    for (int g = 0; g < num_groups; ++g) {
        map[(size_t)g] = make_int2(dynamics_of_group[g], condition_of_group[g]);
        smap[(size_t)g] = sensing_of_group[g];
    }
    if (qr::stream_is_capturing(st) && !(table_is_current(e->group_map, map) && table_is_current(e->rollout_sen_map, smap)))
        return fail(QR_E_STATE, w + "new group maps are uploaded after a device synchronisation, which a stream under capture does not allow; "
                                    "call once with these maps outside the capture");
    if (int rc = upload_table(e->group_map, map, st, who, "group map", "this map")) return rc;
    if (int rc = upload_table(e->rollout_sen_map, smap, st, who, "sensing map", "this map")) return rc;
    if (critic)
        return QR_TIMED_LAUNCH(e, st, qr::launch_rollout_policy_privileged(e->cfg.variant, e->P, A, conditions->d_slots, dynamics->d_slots, sensing->d_slots,
                                           e->group_map.d, e->rollout_sen_map.d, *history, num_groups, envs_per_group, K, noise_seed, first_step,
                                           pending_dev, obs_out_dev, critic->obs, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev,
                                           last_obs_dev, critic->last_obs, st));
    if (history)
        return QR_TIMED_LAUNCH(e, st, qr::launch_rollout_policy_history(e->cfg.variant, e->P, A, conditions->d_slots, dynamics->d_slots, sensing->d_slots,
                                           e->group_map.d, e->rollout_sen_map.d, *history, num_groups, envs_per_group, K, noise_seed, first_step,
                                           pending_dev, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, last_obs_dev,
                                           st));
    return QR_TIMED_LAUNCH(e, st, qr::launch_rollout_policy_sensing(e->cfg.variant, e->P, A, conditions->d_slots, dynamics->d_slots, sensing->d_slots,
                                       e->group_map.d, e->rollout_sen_map.d, num_groups, envs_per_group, K, noise_seed, first_step, pending_dev,
                                       obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, last_obs_dev, st));
}

int qr_rollout_policy_sensing(qr_env* e, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics, qr_sensing_bank* sensing,
                              int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group, const int32_t* dynamics_of_group,
                              const int32_t* sensing_of_group, int32_t K, const float* log_std, uint64_t noise_seed, uint64_t first_step, int32_t flags,
                              float* pending_dev, float* obs_out_dev, float* act_out_dev, float* logp_out_dev, float* rew_out_dev,
                              uint8_t* done_out_dev, uint8_t* trunc_out_dev, float* last_obs_dev, void* stream) {
    return rollout_policy_sensing("qr_rollout_policy_sensing", nullptr, e, policy, conditions, dynamics, sensing, num_groups, envs_per_group,
                                  condition_of_group, dynamics_of_group, sensing_of_group, K, log_std, noise_seed, first_step, flags, pending_dev,
                                  obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, last_obs_dev, stream);
}

// qr_rollout_policy_sensing for a policy that observes its last `history` commands: rows of obs_len + 4 * history floats
int qr_rollout_policy_history(qr_env* e, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics, qr_sensing_bank* sensing,
                              int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group, const int32_t* dynamics_of_group,
                              const int32_t* sensing_of_group, int32_t history, int32_t K, const float* log_std, uint64_t noise_seed, uint64_t first_step,
                              int32_t flags, float* pending_dev, float* obs_out_dev, float* act_out_dev, float* logp_out_dev, float* rew_out_dev,
                              uint8_t* done_out_dev, uint8_t* trunc_out_dev, float* last_obs_dev, void* stream) {
    return rollout_policy_sensing("qr_rollout_policy_history", &history, e, policy, conditions, dynamics, sensing, num_groups, envs_per_group,
                                  condition_of_group, dynamics_of_group, sensing_of_group, K, log_std, noise_seed, first_step, flags, pending_dev,
                                  obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, last_obs_dev, stream);
}

// qr_rollout_policy_history (history >= 1) / qr_rollout_policy_sensing (history == 0) that also stores the rows before the sensor's noise
int qr_rollout_policy_privileged(qr_env* e, qr_policy* policy, qr_condition_bank* conditions, qr_dynamics_bank* dynamics, qr_sensing_bank* sensing,
                                 int32_t num_groups, int32_t envs_per_group, const int32_t* condition_of_group, const int32_t* dynamics_of_group,
                                 const int32_t* sensing_of_group, int32_t history, int32_t K, const float* log_std, uint64_t noise_seed,
                                 uint64_t first_step, int32_t flags, float* pending_dev, float* obs_out_dev, float* critic_obs_out_dev,
                                 float* act_out_dev, float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev,
                                 float* last_obs_dev, float* critic_last_obs_dev, void* stream) {
    const CriticRows critic{critic_obs_out_dev, critic_last_obs_dev};
    return rollout_policy_sensing("qr_rollout_policy_privileged", &history, e, policy, conditions, dynamics, sensing, num_groups, envs_per_group,
                                  condition_of_group, dynamics_of_group, sensing_of_group, K, log_std, noise_seed, first_step, flags, pending_dev,
                                  obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, last_obs_dev, stream, &critic);
}

int qr_vehicle_physical_count(int32_t variant) {
    int count = 0;
    if (!qr::dynamics_physical_names(variant, &count)) return fail(QR_E_INVALID, "qr_vehicle_physical_count: unknown variant");
    return count;
}

// Every refusal comes before the launch; the slots count as set from here on (the kernel is ordered on `stream` before whatever the
// caller enqueues behind it).  No synchronisation.
int qr_vehicle_bank_sample(qr_dynamics_bank* b, int32_t first_slot, int32_t num_slots, const double* phys_lo, const double* phys_hi, int32_t count,
                            uint64_t seed, uint64_t draw, void* stream) {
    const std::string w = "qr_vehicle_bank_sample: ";
    if (!b) return fail(QR_E_INVALID, w + "null bank");
    if (!phys_lo || !phys_hi) return fail(QR_E_INVALID, w + "the two bounds are required");
    int n = 0;
    const char* const* names = qr::dynamics_physical_names(b->variant, &n);
    if (count != n) return fail(QR_E_INVALID, w + "count must equal qr_vehicle_physical_count of the bank's variant");
    if (first_slot < 0 || num_slots < 1 || (int64_t)first_slot + num_slots > (int64_t)b->capacity)
        return fail(QR_E_INVALID, w + "slots [first_slot, first_slot + num_slots) must be a non-empty range inside [0, capacity)");
    for (int j = 0; j < n; ++j) {
        if (!std::isfinite(phys_lo[j]) || !std::isfinite(phys_hi[j])) return fail(QR_E_INVALID, w + "a bound of " + names[j] + " is not finite");
        if (phys_lo[j] > phys_hi[j]) return fail(QR_E_INVALID, w + "lo > hi for " + names[j]);
    }
    int w_min = -1, w_max = -1;
    for (int j = 0; j < n; ++j) {
        const std::string name = names[j];
        const bool positive = b->variant == QR_VARIANT_E2E ? (name == "Ixx" || name == "Iyy" || name == "Izz" || name == "tau") : name.rfind("tau_", 0) == 0;
        if (positive && !(phys_lo[j] > 0.0)) return fail(QR_E_INVALID, w + name + " must be positive: lo <= 0");
        if (name == "w_min") w_min = j;
        if (name == "w_max") w_max = j;
    }
    if (w_min >= 0 && phys_hi[w_min] >= phys_lo[w_max]) return fail(QR_E_INVALID, w + "hi[w_min] must be below lo[w_max]");
    QR_HIP(hipSetDevice(b->device));
    if (hipError_t err = qr::launch_dynamics_sample(b->variant, b->d_slots, first_slot, num_slots, phys_lo, phys_hi, seed, draw, (hipStream_t)stream))
        return fail(QR_E_HIP, w + hipGetErrorString(err));
    for (int s = first_slot; s < first_slot + num_slots; ++s) b->is_set[(size_t)s] = 1;
    return QR_OK;
}

// The refusals come first and in full: what qr_rollout_policy_conditions refuses, what qr_evaluate_policy_grid refuses about its policy
// bank, and the NULL arrays; nothing is enqueued or copied before the last of them.  Entry g of the sampling table holds the bits
// qr_rollout_policy would use for log_std[g] and noise_seed[g] (qr::sampling_entry).
int qr_rollout_policy_population(qr_env* e, qr_policy_bank* policies, qr_condition_bank* conditions, int32_t num_groups, int32_t envs_per_group,
                                 const int32_t* policy_of_group, const int32_t* condition_of_group, int32_t K, const float* log_std,
                                 const uint64_t* noise_seed, uint64_t first_step, int32_t flags, float* obs_out_dev, float* act_out_dev,
                                 float* logp_out_dev, float* rew_out_dev, uint8_t* done_out_dev, uint8_t* trunc_out_dev, float* last_obs_dev,
                                 void* stream) {
    const char* who = "qr_rollout_policy_population";
    if (int rc = check_ready(e)) return rc;
    if (int rc = check_rollout_common(e, K, policies && log_std && noise_seed, obs_out_dev, act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, who))
        return rc;
    if (int rc = qr::check_policy_bank(policies, e->L, e->cfg.device, who)) return rc;
    if (flags < 0 || flags > (QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS))
        return fail(QR_E_INVALID, std::string(who) + ": `flags` takes QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS");
    if (!conditions) return fail(QR_E_INVALID, std::string(who) + ": null condition bank handle");
    if (!policy_of_group || !condition_of_group) return fail(QR_E_INVALID, std::string(who) + ": the two group maps are required");
    if (int rc = check_condition_groups(e, conditions, num_groups, envs_per_group, who)) return rc;
    if (int rc = check_group_indices(policies, policy_of_group, conditions, condition_of_group, num_groups, who)) return rc;
    qr::PolicyArgs A{};   // launch-wide: the step counter and the two flags; weights and sampling values are per group
    qr::set_sampling(A, qr::PopulationEntry{}, first_step, flags);
    std::vector<qr::PopulationEntry> table((size_t)num_groups);
    for (int g = 0; g < num_groups; ++g) table[(size_t)g] = qr::sampling_entry(log_std + 4 * (size_t)g, noise_seed[g]);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_group_map(e, policy_of_group, condition_of_group, num_groups, st, who)) return rc;
    if (int rc = upload_table(e->pop_table, table, st, who, "sampling table (log_std, noise_seed per group)", "these values")) return rc;
    return QR_TIMED_LAUNCH(e, st, qr::launch_rollout_policy_population(e->cfg.variant, e->P, A, qr::bank_weights(policies), qr::bank_weights_lo(policies),
                                       conditions->d_slots, e->group_map.d, e->pop_table.d, num_groups, envs_per_group, K, obs_out_dev,
                                       act_out_dev, logp_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, last_obs_dev, st));
}

int qr_record_row_len(const qr_env* e) { return e ? e->S + QR_RECORD_EXTRA : QR_E_INVALID; }

int qr_record_policy(qr_env* e, qr_policy* policy, int32_t K, const float* log_std, uint64_t noise_seed, uint64_t first_step,
                     int32_t flags, int32_t rec_envs, float* rows_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (!policy) return fail(QR_E_INVALID, "qr_record_policy: null policy handle");
    if (!log_std) return fail(QR_E_INVALID, "qr_record_policy: log_std is required");
    if (!rows_dev) return fail(QR_E_INVALID, "qr_record_policy: rows_dev is required");
    if ((uintptr_t)rows_dev & 15) return fail(QR_E_INVALID, "qr_record_policy: rows_dev must be 16-byte aligned");
    if (K < 1) return fail(QR_E_INVALID, "qr_record_policy: num_steps must be >= 1");
    if (rec_envs < 1 || rec_envs > e->cfg.num_envs) return fail(QR_E_INVALID, "qr_record_policy: rec_envs must be in 1..num_envs");
    if (flags & ~(QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS))
        return fail(QR_E_INVALID, "qr_record_policy: `flags` takes QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS");
    if (e->P.flags & (qr::kFlagPause | qr::kFlagPauseIfCollision))
        return fail(QR_E_STATE, "qr_record_policy: pause / pause_if_collision envs are evaluation modes; use qr_step");
    if (int rc = qr::check_policy_handle(policy, e->L, e->cfg.device, "qr_record_policy")) return rc;
    qr::PolicyArgs A{};   // the sampling arguments of qr_rollout_policy (same noise stream); the kernel computes no log-prob
    if (int rc = qr::fetch_policy_weights(policy, "qr_record_policy", A.weights)) return rc;
    A.weights_lo = qr::policy_weights_lo(policy);
    qr::set_sampling(A, qr::sampling_entry(log_std, noise_seed), first_step, flags);
    hipStream_t st = (hipStream_t)stream;
    return QR_TIMED_LAUNCH(e, st, qr::launch_record_policy(e->cfg.variant, e->P, A, K, rec_envs, rows_dev, st));
}

int qr_blackbox_policy(qr_env* e, qr_policy* policy, int32_t K, const float* log_std, uint64_t noise_seed, uint64_t first_step,
                       int32_t flags, int32_t trigger, int32_t window, int32_t rec_envs, float* ring_dev, int32_t* st_dev, float* term_dev,
                       void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (!policy) return fail(QR_E_INVALID, "qr_blackbox_policy: null policy handle");
    if (!log_std) return fail(QR_E_INVALID, "qr_blackbox_policy: log_std is required");
    if (!ring_dev || !st_dev) return fail(QR_E_INVALID, "qr_blackbox_policy: ring_dev and st_dev are required");
    if (((uintptr_t)ring_dev | (uintptr_t)st_dev) & 15) return fail(QR_E_INVALID, "qr_blackbox_policy: ring_dev and st_dev must be 16-byte aligned");
    if ((uintptr_t)term_dev & 3) return fail(QR_E_INVALID, "qr_blackbox_policy: term_dev must be 4-byte aligned");
    if (K < 1) return fail(QR_E_INVALID, "qr_blackbox_policy: num_steps must be >= 1");
    if (rec_envs < 1 || rec_envs > e->cfg.num_envs) return fail(QR_E_INVALID, "qr_blackbox_policy: rec_envs must be in 1..num_envs");
    if (trigger < 0 || trigger > (QR_BLACKBOX_ON_CRASH | QR_BLACKBOX_ON_TIME_LIMIT))
        return fail(QR_E_INVALID, "qr_blackbox_policy: `trigger` takes QR_BLACKBOX_ON_CRASH | QR_BLACKBOX_ON_TIME_LIMIT");
    if (window < 1) return fail(QR_E_INVALID, "qr_blackbox_policy: window must be >= 1");
    if (flags & ~(QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS))
        return fail(QR_E_INVALID, "qr_blackbox_policy: `flags` takes QR_ROLLOUT_DETERMINISTIC | QR_ROLLOUT_F32CLASS");
    if (e->P.flags & (qr::kFlagPause | qr::kFlagPauseIfCollision))
        return fail(QR_E_STATE, "qr_blackbox_policy: pause / pause_if_collision envs are evaluation modes; use qr_step");
    if (int rc = qr::check_policy_handle(policy, e->L, e->cfg.device, "qr_blackbox_policy")) return rc;
    qr::PolicyArgs A{};   // the sampling arguments of qr_record_policy / qr_rollout_policy (same noise stream)
    if (int rc = qr::fetch_policy_weights(policy, "qr_blackbox_policy", A.weights)) return rc;
    A.weights_lo = qr::policy_weights_lo(policy);
    qr::set_sampling(A, qr::sampling_entry(log_std, noise_seed), first_step, flags);
    const int slot0 = (int)(first_step % (uint64_t)window);   // the ring slot of the call's first step
    hipStream_t st = (hipStream_t)stream;
    return QR_TIMED_LAUNCH(e, st, qr::launch_blackbox_policy(e->cfg.variant, e->P, A, K, rec_envs, trigger, window, slot0, ring_dev, st_dev, term_dev, st));
}

int qr_observe(qr_env* e, float* obs_out_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;
    if (!obs_out_dev) return fail(QR_E_INVALID, "qr_observe: null output");
    QR_HIP(qr::launch_observe(e->cfg.variant, e->P, obs_out_dev, (hipStream_t)stream));
    return QR_OK;
}

int qr_probe_residual(qr_env* e, float* out_dev, void* stream) {
    if (int rc = bind_device(e)) return rc;
    if (!out_dev) return fail(QR_E_INVALID, "qr_probe_residual: null output");
    if (e->cfg.variant != QR_VARIANT_E2E || !(e->P.flags & qr::kFlagResidual))
        return fail(QR_E_STATE, "qr_probe_residual: needs an E2E env with residual weights");
    QR_HIP(qr::launch_residual_probe(e->P, out_dev, (hipStream_t)stream));
    return QR_OK;
}

int qr_get_state(qr_env* e, float* world_dev, float* dist_dev, int32_t* target_dev, int32_t* steps_dev,
                 uint32_t* episode_dev, void* stream) {
    if (int rc = bind_device(e)) return rc;
    QR_HIP(qr::launch_get_state(e->cfg.variant, e->P, world_dev, dist_dev, target_dev, steps_dev, episode_dev,
                                (hipStream_t)stream));
    return QR_OK;
}

int qr_set_state(qr_env* e, const float* world_dev, const float* dist_dev, const int32_t* target_dev,
                 const int32_t* steps_dev, const uint32_t* episode_dev, void* stream) {
    if (int rc = check_ready(e)) return rc;  // target is reduced modulo num_gates
    QR_HIP(qr::launch_set_state(e->cfg.variant, e->P, world_dev, dist_dev, target_dev, steps_dev, episode_dev,
                                (hipStream_t)stream));
    return QR_OK;
}

const char* qr_rollout_kernel_name(const qr_env* e) {
    if (!e) return "";
    return qr::rollout_kernel_name(e->cfg.variant, e->P, e->rollout_form);
}

int qr_set_rollout_form(qr_env* e, int32_t form) {
    if (!e) return fail(QR_E_INVALID, "qr_set_rollout_form: null env");
    if (form < 0 || form > (QR_ROLLOUT_MULTI_WAVE | QR_ROLLOUT_GENERAL | QR_ROLLOUT_ONE_WAVE)) return fail(QR_E_INVALID, "qr_set_rollout_form: unknown form");
    e->rollout_form = form;
    return QR_OK;
}

int qr_set_timing(qr_env* e, int32_t on) {
    if (!e) return fail(QR_E_INVALID, "qr_set_timing: null env");
    e->timing = on != 0;
    if (!e->timing) e->timing_valid = false;
    return QR_OK;
}

int qr_last_step_many_ms(qr_env* e, float* total_ms) {
    if (!e || !total_ms) return fail(QR_E_INVALID, "qr_last_step_many_ms: null argument");
    if (int rc = bind_device(e)) return rc;
    if (!e->timing_valid) return fail(QR_E_STATE, "qr_last_step_many_ms: no qr_step_many call recorded");
    QR_HIP(hipEventSynchronize(e->ev1));
    QR_HIP(hipEventElapsedTime(total_ms, e->ev0, e->ev1));
    return QR_OK;
}

int qr_profile_steps(qr_env* e, int32_t K, const float* actions_dev, float* obs_out_dev, float* rew_out_dev,
                     uint8_t* done_out_dev, uint8_t* trunc_out_dev, void* stream, float* mean_kernel_ms,
                     float* region_ms) {
    if (int rc = check_ready(e)) return rc;
    if (K < 1 || !mean_kernel_ms || !region_ms) return fail(QR_E_INVALID, "qr_profile_steps: bad argument");
    if (int rc = check_term_rows(e, K, "qr_profile_steps")) return rc;
    if (int rc = check_step_buffers(actions_dev, obs_out_dev, rew_out_dev, done_out_dev, "qr_profile_steps")) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<hipEvent_t> ev(2 * (size_t)K);
    for (auto& x : ev) QR_HIP(hipEventCreate(&x));
    for (int k = 0; k < K; ++k) {
        QR_HIP(hipEventRecord(ev[2 * k], st));
        QR_HIP(launch_step_row(e, k, actions_dev, obs_out_dev, rew_out_dev, done_out_dev, trunc_out_dev, st));
        QR_HIP(hipEventRecord(ev[2 * k + 1], st));
    }
    QR_HIP(hipEventSynchronize(ev[2 * K - 1]));
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        float ms = 0.0f;
        QR_HIP(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
        sum += ms;
    }
    QR_HIP(hipEventElapsedTime(region_ms, ev[0], ev[2 * K - 1]));
    *mean_kernel_ms = (float)(sum / K);
    for (auto& x : ev) (void)hipEventDestroy(x);
    return QR_OK;
}

#if defined(QR_PHASE_TIMING) || defined(QR_CLOCK_PROBE)
// profiling builds only (tools/phase_timing.py, tools/clock_probe.py): device buffer [n_waves][16] of shader-clock stamps, or NULL
__attribute__((visibility("default"))) int qr_debug_set_ticks(qr_env* e, unsigned long long* ticks_dev) {
    if (!e) return QR_E_INVALID;
    e->P.ticks = ticks_dev;
    e->P.tick_on = ticks_dev != nullptr;
    return QR_OK;
}
#endif

}  // extern "C"
