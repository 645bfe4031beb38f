// wbc_engine.cpp — host side of the C-ABI (include/wbc.h): device buffers, stream ordering,
// kernel launches.  Replaces the per-object state of the reference's WholeBodyController
// (include/anymal_wbc/whole_body_controller.hpp:106-166) with batched device buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "wbc.h"
#include "wbc_anymal_model.h"
#include "wbc_layout.h"


extern "C" hipError_t wbc_launch_step(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_update(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_solve_general(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_solve_stance(const wbc::KernelArgs* a, hipStream_t st);
// The default step's launchers (wbc_launch_update_solve_<unit> of wbc_kernel_<unit>.hip), indexed by
// wbc::StepInstance: kStepLaunchers[wbc::step_instance(...)] is a step's; the base-body units'
// (WBC_STEP_UNITS_BB) follow the nine, the limits units' (WBC_STEP_UNITS_LM) those, the force-bound units'
// (WBC_STEP_UNITS_FN) the limits units', the force-task units' (WBC_STEP_UNITS_FT) the force-bound units'
#define X(unit) extern "C" hipError_t wbc_launch_update_solve_##unit(const wbc::KernelArgs* a, hipStream_t st);
WBC_STEP_UNITS(X)
WBC_STEP_UNITS_BB(X)
WBC_STEP_UNITS_LM(X)
WBC_STEP_UNITS_FN(X)
WBC_STEP_UNITS_FT(X)
#undef X
#define X(unit) wbc_launch_update_solve_##unit,
static hipError_t (*const kStepLaunchers[])(const wbc::KernelArgs*, hipStream_t) = {WBC_STEP_UNITS(X) WBC_STEP_UNITS_BB(X) WBC_STEP_UNITS_LM(X)
                                                                                       WBC_STEP_UNITS_FN(X) WBC_STEP_UNITS_FT(X)};
#undef X
static_assert(sizeof(kStepLaunchers) / sizeof(kStepLaunchers[0]) == wbc::STEP_LAUNCHER_COUNT_FT, "one launcher per instance");
extern "C" hipError_t wbc_launch_modes(const wbc::KernelArgs* a, hipStream_t st);
// the mode loop's objective instance (wbc_kernel_modes_obj.hip) and the selection after it (WBC_BEST)
extern "C" hipError_t wbc_launch_modes_obj(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_best_modes(const double* obj, const int32_t* status, const double* tau, const double* grf,
                                            int states, int modes, int32_t* best, double* bobj, double* btau, double* bgrf,
                                            hipStream_t st);
// the default step's duals instances (wbc_kernel_du0.hip stateless, wbc_kernel_du1.hip stateful: wbc_step
// with WBC_DUALS), declared here and not in wbc_layout.h's lists: a flag picks them, not the tables in force
extern "C" hipError_t wbc_launch_update_solve_du0(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_update_solve_du1(const wbc::KernelArgs* a, hipStream_t st);
// and the limits units' duals instances (wbc_kernel_lmd0.hip, wbc_kernel_lmd1.hip: WBC_DUALS under a limits table)
extern "C" hipError_t wbc_launch_update_solve_lmd0(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_update_solve_lmd1(const wbc::KernelArgs* a, hipStream_t st);
// and the force-bound units' duals instances (wbc_kernel_fnd0.hip, wbc_kernel_fnd1.hip: wbc_step with WBC_DUALS_FORCE,
// KernelArgs::dual as [B][WBC_DUAL_FORCE_LEN])
extern "C" hipError_t wbc_launch_update_solve_fnd0(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_update_solve_fnd1(const wbc::KernelArgs* a, hipStream_t st);
// and the force-task units' duals instances (wbc_kernel_ftd0.hip, wbc_kernel_ftd1.hip: wbc_step with WBC_DUALS_TASK,
// the same [B][WBC_DUAL_FORCE_LEN] under KernelArgs::ft)
extern "C" hipError_t wbc_launch_update_solve_ftd0(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_update_solve_ftd1(const wbc::KernelArgs* a, hipStream_t st);
extern "C" hipError_t wbc_launch_reset(double* hist, const uint8_t* mask, int batch, hipStream_t st);
extern "C" hipError_t wbc_launch_qmap(const uint8_t* masks, int batch, int32_t* map, hipStream_t st);
extern "C" hipError_t wbc_preload_resident();
extern "C" hipError_t wbc_launch_resident(const wbc::KernelArgs* a, wbc::ResidentBox* box, const void* pin_in,
                                          void* own_in, int in_words, unsigned long long seq0, unsigned long long idle_ticks,
                                          hipStream_t st);

namespace {
thread_local std::string g_err;

int32_t fail(int32_t code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define WBC_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) return fail(WBC_ERR_HIP, std::string(#call ": ") + hipGetErrorString(e_)); \
    } while (0)
}  // namespace

// A per-robot table of the default step ([B][row] doubles): the engine's own device table (allocated
// at the first set from the host; has_own: it holds a table), a caller's device table, and the one in
// force: the caller's, else the engine's own when set, else none.
struct RobotTable {
    size_t row;
    double* own = nullptr;
    bool has_own = false;
    const double* bound = nullptr;
    const double* in_force = nullptr;
    explicit RobotTable(size_t row_len) : row(row_len) {}
};

// What a step reads and writes: the handle's bindings (wbc_step), or a cycle's packed blocks with
// the wave map of their masks (enqueue_cycle).  qmap: the map of the engine's own masks.
struct StepIO {
    wbc::ConstInputView in;
    wbc::OutputView out;
    const int32_t* qmap;
};

struct wbc_engine {
    int32_t batch = 0;
    int32_t device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    wbc_model* d_model = nullptr;
    wbc_params* d_params = nullptr;
    double* d_limg = nullptr;  // the step kernel's LDS image of the model + friction table (wbc_layout.h)
    wbc_params params{};  // host copy, passed by value in the kernel arguments (KernelArgs::pv)
    // per-robot parameters (KernelArgs::rp, [B][WBC_RP_LEN]; without a table in force: the
    // engine-wide params) and per-robot ground normals at the feet (KernelArgs::cn, [B][WBC_CN_LEN];
    // without: flat ground).  The kernels that read normals are per-robot-parameter instances, so
    // without a parameter table in force their step reads d_rp_uni: the engine-wide params in B rows
    // (built at the first use; params never change)
    RobotTable rp{WBC_RP_LEN};
    RobotTable cn{WBC_CN_LEN};
    double* d_rp_uni = nullptr;
    // per-robot base bodies (KernelArgs::bb, [B][WBC_BB_LEN]; without: the model's base).  The kernels
    // that read them are contact-normal instances, so without normals in force their step reads
    // d_cn_flat: (0, 0, 1) at every foot in B rows (built at the first use), and d_rp_uni as above.
    // base_row: the model's own base as a row (what wbc_get_base_body returns without a table)
    RobotTable bb{WBC_BB_LEN};
    double* d_cn_flat = nullptr;
    double base_row[WBC_BB_LEN] = {};
    // owned inputs: one device block [pose | nu | qj | ref | contacts | switching] (so a host cycle
    // is one H2D copy), and the outputs one block [tau | grf | status | iters | x] (wbc_layout.h
    // input_view / output_view: own_in, own_out)
    void* d_inblk = nullptr;
    void* d_outblk = nullptr;
    void* h_in = nullptr;   // pinned staging of the same layouts (wbc_cycle, allocated on first use)
    void* h_out = nullptr;
    wbc::InputView own_in{};
    wbc::OutputView own_out{};
    uint8_t* d_mask = nullptr;
    // contact-mode hypotheses (wbc_set_modes): n_modes > 0 turns the inputs into B / n_modes states
    int32_t n_modes = 0;
    uint8_t* d_modes = nullptr;
    // the update shared by mode_loop hypotheses per wave (KernelArgs::mloop; 1 = one per segment)
    // and the hypotheses' order, chunk by chunk (plan_mode_loop)
    int32_t mode_loop = 1;
    uint8_t mode_order[16] = {};
    // wbc_step_modes with WBC_OBJECTIVE / WBC_BEST: the hypotheses' objectives [B] and, per state (at
    // most B of them), the best hypothesis, its objective, tau and grf; allocated at the first step that
    // carries the flag.  modes_flags: which of the two flags the last wbc_step_modes carried
    double* d_obj = nullptr;
    int32_t* d_best = nullptr;
    double* d_best_obj = nullptr;
    double* d_best_tau = nullptr;
    double* d_best_grf = nullptr;
    uint32_t modes_flags = 0;
    // wbc_step with WBC_DUALS: the multipliers [B][WBC_DUAL_LEN], allocated at the first step that carries
    // the flag; step_duals: the last wbc_step carried it.  Its kernels are base-body instances, so without
    // a base-body table in force their step reads d_bb_def: base_row in B rows (built at the first use),
    // and d_cn_flat / d_rp_uni as the base-body kernels do
    // wbc_step with WBC_DUALS_FORCE: the multipliers [B][WBC_DUAL_FORCE_LEN] in a buffer of their own (the strides
    // differ), allocated at the first step that carries that flag; without a force-bound table in force its step
    // reads d_fn_none: (-inf x 4, +inf x 4) in B rows (built at the first use).  step_duals: what the last wbc_step
    // wrote, which the four getters consult
    // wbc_step with WBC_DUALS_TASK: d_dual48 again (DUALS_48); without a force-task table in force its step reads
    // d_ft_plain: (0 x 12, 1, 0) in B rows (built at the first use)
    double* d_dual = nullptr;
    double* d_bb_def = nullptr;
    double* d_dual48 = nullptr;
    double* d_fn_none = nullptr;
    double* d_ft_plain = nullptr;
    enum StepDuals { DUALS_NONE, DUALS_40, DUALS_48 };
    StepDuals step_duals = DUALS_NONE;
    // per-robot torque bounds and per-foot friction (KernelArgs::lm, [B][WBC_LM_LEN]; without: -+max_torque
    // and friction).  The kernels that read them are base-body instances, so without a base-body table in
    // force their step reads d_bb_def, and d_cn_flat / d_rp_uni as the base-body kernels do
    RobotTable lm{WBC_LM_LEN};
    // per-foot normal-force bounds (KernelArgs::fn, [B][WBC_FN_LEN]; without: no such rows).  The kernels that
    // read them are limits and base-body instances; without a limits table in force they take each robot's
    // own -+max_torque and friction (a null KernelArgs::lm), the other tables as the limits kernels do
    RobotTable fn{WBC_FN_LEN};
    // per-robot reference contact forces and their weight (KernelArgs::ft, [B][WBC_FT_LEN]; without: the plain
    // regulariser).  The kernels that read them are force-bound instances: without a force-bound table in force
    // their step reads d_fn_none, the other tables as the force-bound kernels do
    RobotTable ft{WBC_FT_LEN};
    // bound (possibly external) inputs
    wbc::ConstInputView in{};
    // state / outputs
    double* d_hist = nullptr;
    double* d_work = nullptr;
    int32_t* d_fb = nullptr;  // elimination fallback counters [2] + list [B] (KernelArgs::fb)
    int32_t parity = 0;       // fallback counter of the next elimination update
    // four-contact rows among the engine's own contact masks (d_contacts, as last copied from the
    // host) and among the mode masks: the stance elimination runs when every QP of a step has
    // mask 15 (known only for the engine's own masks; device-bound masks take the general path)
    int64_t n_stance_own = 0;
    int32_t modes_stance = 0;
    bool elim = false;        // the last update's choice (its solve follows it)
    int32_t elim_parity = 0;  // and its fallback counter
    double* d_dbg = nullptr;
    // bound (possibly external) outputs
    wbc::OutputView out{};
    // the default step's wave map (KernelArgs::qmap): QPs grouped by contact mask, four to a wave.
    // For the engine's own masks it is built on the host whenever they are copied (qmap_waves waves;
    // 0 = every mask equal, no map needed); for device-bound masks wbc_qmap_kernel builds it on the
    // stream before each step
    int32_t* d_qmap = nullptr;
    // a zero-copy cycle ran last: the engine's own input / output blocks (and wave map) are behind the
    // pinned ones until sync_own copies them (before any other call that reads or writes them)
    bool zc_stale = false;
    int32_t* h_qmap = nullptr;  // pinned
    int32_t qmap_waves = 0;
    bool qmap_host = true;  // qmap_waves / d_qmap describe d_contacts (not after a change of modes)
    bool updated = false;
    bool timed = false;    // a WBC_TIMED step has recorded ev0 / ev1
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // device addresses of the pinned cycle buffers (zero-copy cycle: the step reads h_in and writes
    // h_out directly, no copies, and takes the map of its masks from h_qmap); null when the batch
    // takes the copy path
    wbc::ConstInputView m_in{};
    wbc::OutputView m_out{};
    const int32_t* m_qmap = nullptr;
    // the resident control cycle (WBC_RESIDENT): mailbox (pinned, coherent), its stream, whether a
    // resident wave runs and with which step flags, the last command posted, when it last answered
    wbc::ResidentBox* res_box = nullptr;
    wbc::ResidentBox* res_box_dev = nullptr;
    hipStream_t res_stream = nullptr;
    bool res_on = false;
    uint32_t res_flags = 0;
    unsigned long long res_seq = 0;
    std::chrono::steady_clock::time_point res_last{};
};

namespace {
template <class T>
hipError_t dalloc(T** p, size_t n) {
    return hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * (n ? n : 1));
}

// wbc_cycle runs zero-copy up to this batch size (enqueue_cycle)
[[maybe_unused]] constexpr size_t kZeroCopyMaxBatch = 64;

// rows of the input arrays: one per robot, or one per state when mode hypotheses are set
size_t input_rows(const wbc_engine* h) { return (size_t)(h->n_modes ? h->batch / h->n_modes : h->batch); }

StepIO bound_io(const wbc_engine* h) { return {h->in, h->out, h->d_qmap}; }

wbc::KernelArgs make_args(wbc_engine* h, uint32_t flags, const wbc::ConstInputView& in, const wbc::OutputView& out) {
    wbc::KernelArgs a;
    a.model = h->d_model;
    a.params = h->d_params;
    a.limg = h->d_limg;
    a.pv = h->params;
    // limits, force bounds or a force task: their kernels read rp, cn and bb
    const bool lf = h->lm.in_force || h->fn.in_force || h->ft.in_force;
    a.rp = h->rp.in_force ? h->rp.in_force : ((h->cn.in_force || h->bb.in_force || lf) ? h->d_rp_uni : nullptr);
    a.cn = h->cn.in_force ? h->cn.in_force : ((h->bb.in_force || lf) ? h->d_cn_flat : nullptr);
    a.bb = h->bb.in_force ? h->bb.in_force : (lf ? h->d_bb_def : nullptr);
    a.lm = h->lm.in_force;
    a.fn = h->fn.in_force ? h->fn.in_force : (h->ft.in_force ? h->d_fn_none : nullptr);
    a.ft = h->ft.in_force;
    a.base_pose = in.pose;
    a.nu = in.nu;
    a.qj = in.qj;
    a.ref = in.ref;
    a.contacts = in.contacts;
    a.switching = in.switching;
    a.hist = h->d_hist;
    a.work = h->d_work;
    a.tau = out.tau;
    a.grf = out.grf;
    a.x = (flags & WBC_NO_X) ? nullptr : out.x;
    a.status = out.status;
    a.iters = out.iters;
    a.dbg = h->d_dbg;
    a.batch = h->batch;
    a.stateful = (flags & WBC_STATELESS) ? 0 : 1;
    a.debug = (flags & WBC_DEBUG) ? 1 : 0;
    a.cold = (flags & WBC_COLD) ? 1 : 0;
    a.modes = 0;
    a.mode_masks = h->d_modes;
    a.elim = 0;
    a.parity = 0;
    a.fb = h->d_fb;
    a.fb_cap = h->batch;
    a.qmap = nullptr;
    a.nwaves = (h->batch + wbc::QMAP_SEG - 1) / wbc::QMAP_SEG;
    a.mloop = 0;
    std::memset(a.mode_order, 0, sizeof(a.mode_order));
    a.obj = nullptr;
    a.dual = nullptr;
    return a;
}
wbc::KernelArgs make_args(wbc_engine* h, uint32_t flags) { return make_args(h, flags, h->in, h->out); }

// Host wave map of the engine's own contact masks (copied on the stream; the callers synchronize
// before the host buffer is reused)
hipError_t upload_qmap(wbc_engine* h, const uint8_t* masks) {
    h->qmap_waves = wbc::qmap_build(masks, h->batch, h->h_qmap);
    h->qmap_host = true;
    if (!h->qmap_waves) return hipSuccess;
    return hipMemcpyAsync(h->d_qmap, h->h_qmap, (size_t)h->qmap_waves * wbc::QMAP_SEG * sizeof(int32_t),
                          hipMemcpyHostToDevice, h->stream);
}

// wait for every launch the engine queued so far: a stream synchronize of the bound stream (its
// own, or the caller's, which must still be alive: include/wbc.h, wbc_set_stream).  No event is
// recorded per launch: an event packet between two steps costs ~3 us of the ~36 us step (measured
// on MI355X, 103.5 -> 112.3 M solves/s on the headline config without it).
hipError_t drain(wbc_engine* h) { return h->stream ? hipStreamSynchronize(h->stream) : hipSuccess; }

// Mode hypotheses per wave and their order (wbc_layout.h mode_loop_plan) for this engine's batch
// and device: every SIMD (4 per CU) should get a wave.  WBC_MODES_M (a divisor of K) overrides M
// (A/B runs, tests).
void plan_mode_loop(wbc_engine* h, const uint8_t* modes, int32_t K) {
    const int64_t groups = (h->batch / K + 3) / 4;
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus <= 0) cus = 256;
    const char* e = std::getenv("WBC_MODES_M");
    h->mode_loop = wbc::mode_loop_plan(modes, K, groups, 4LL * cus, e ? std::atoi(e) : 0, h->mode_order);
}

int64_t count_stance(const uint8_t* masks, size_t n) {
    int64_t c = 0;
    for (size_t i = 0; i < n; ++i) c += (masks[i] & 15) == 15;
    return c;
}

// The resident cycle's mailbox (pinned, coherent) and stream; at wbc_create for B <= 4 (a few ms that
// would otherwise land on the first resident cycle)
hipError_t resident_alloc(wbc_engine* h) {
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, sizeof(wbc::ResidentBox), hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    std::memset(p, 0, sizeof(wbc::ResidentBox));
    h->res_box = static_cast<wbc::ResidentBox*>(p);
    void* d = nullptr;
    e = hipHostGetDevicePointer(&d, p, 0);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->res_stream, hipStreamNonBlocking);
    h->res_box_dev = static_cast<wbc::ResidentBox*>(d);
    h->res_seq = 0;
    return e;
}

// At most one resident wave runs per process: a resident kernel holds its hardware queue
// between cycles, and streams share the GPU_MAX_HW_QUEUES queues, so another engine's work could wait
// behind it until its idle exit.  g_res_owner is the engine whose wave runs; every start and stop of a
// resident wave holds g_res_mu, and every other engine's call that launches work stops that wave first
// (sync_own).  Streams of other libraries (torch) are not covered: INTEGRATION.md states the limit.
std::recursive_mutex g_res_mu;
wbc_engine* g_res_owner = nullptr;

// The resident cycle's wave (WBC_RESIDENT) ends: WBC_RESIDENT_STOP posted, then its stream drained
// (it may have ended by itself after its idle time: then it is idle at once).  Bounded: a wave that
// does not end within kResidentStopWait (stuck inside a step) is reported, not waited for forever.
constexpr auto kResidentStopWait = std::chrono::seconds(2);
hipError_t resident_stop(wbc_engine* h) {
    std::lock_guard<std::recursive_mutex> lk(g_res_mu);
    if (!h->res_on) return hipSuccess;
    h->res_on = false;
    if (g_res_owner == h) g_res_owner = nullptr;
    __atomic_store_n(&h->res_box->cmd, wbc::WBC_RESIDENT_STOP, __ATOMIC_RELEASE);
    const auto deadline = std::chrono::steady_clock::now() + kResidentStopWait;
    hipError_t e;
    while ((e = hipStreamQuery(h->res_stream)) == hipErrorNotReady) {
        if (std::chrono::steady_clock::now() > deadline) return hipErrorLaunchTimeOut;
        std::this_thread::yield();
    }
    __atomic_store_n(&h->res_box->cmd, h->res_seq, __ATOMIC_RELEASE);  // the next wave starts from res_seq
    return e;
}

// Another engine's resident wave on this engine's device, stopped before this engine launches work.
hipError_t stop_foreign_resident(wbc_engine* h) {
    std::lock_guard<std::recursive_mutex> lk(g_res_mu);
    if (!g_res_owner || g_res_owner == h || g_res_owner->device != h->device) return hipSuccess;
    return resident_stop(g_res_owner);
}

// After a zero-copy wbc_cycle the cycle's inputs, outputs and wave map live in the pinned blocks;
// copy them into the engine's own device buffers, so every other call sees the state a copying
// cycle leaves (synchronous: the pinned blocks are rewritten by the next cycle).  A resident cycle
// wave is stopped first, this engine's or another engine's on the same device (every other call goes
// through here).
hipError_t sync_own(wbc_engine* h) {
    {
        hipError_t e = resident_stop(h);
        if (e == hipSuccess) e = stop_foreign_resident(h);
        if (e != hipSuccess) return e;
    }
    if (!h->zc_stale) return hipSuccess;
    const size_t B = (size_t)h->batch;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_inblk, h->h_in, wbc::input_block_bytes(B), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->d_outblk, h->h_out, wbc::output_block_bytes(B), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && h->qmap_waves)
        e = hipMemcpyAsync(h->d_qmap, h->h_qmap, (size_t)h->qmap_waves * wbc::QMAP_SEG * sizeof(int32_t),
                           hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) h->zc_stale = false;
    return e;
}

// Stance elimination for this update: on when every QP has mask 15 (a mixed batch would pay the
// elimination in the update kernel's mixed waves and a second solve kernel's latency; measured
// slower, profiles/r02/k), which the host knows for its own contact masks and for mode masks.
void begin_update(wbc_engine* h, wbc::KernelArgs& a) {
    bool all = false;
    if (h->n_modes) all = h->modes_stance == h->n_modes;
    else if (a.contacts == h->own_in.contacts) all = h->n_stance_own == h->batch;
    h->elim = all;
    // the fallback counters alternate between elimination updates only: the update with parity p
    // fills fb[p] and clears fb[p ^ 1], which only the next elimination update uses (an update
    // without the elimination neither fills nor clears a list, so it must not move the parity)
    h->elim_parity = h->parity;
    if (h->elim) h->parity ^= 1;
    a.elim = h->elim ? 1 : 0;
    a.parity = h->elim_parity;
}

// The step reads the engine's own masks (copied by the host, counted and mapped at copy time): those
// of its own input block, or of the zero-copy cycle's pinned block
bool own_masks(const wbc_engine* h, const wbc::KernelArgs& a) {
    return a.contacts == h->own_in.contacts || (h->m_in.contacts && a.contacts == h->m_in.contacts);
}

// The default step (wbc_update_solve_kernel: every QP reduced to 12 variables and solved in the
// update wave) solves its own fallbacks in the wave that found them (no list), so it
// leaves the fallback list and its parity to the split path's elimination updates.  Its waves each
// hold QPs of one contact mask: the wave map (the engine's own masks: built when they were copied,
// `qmap` its device address; device-bound masks: built on the stream now under WBC_GROUP), or under
// mode hypotheses the arithmetic map.
hipError_t begin_step16(wbc_engine* h, wbc::KernelArgs& a, uint32_t flags, const int32_t* qmap) {
    a.elim = 1;
    h->elim = false;  // a later wbc_solve needs its own wbc_update
    if (a.modes) {
        const int S = h->batch / a.modes;
        a.nwaves = ((S + wbc::QMAP_SEG - 1) / wbc::QMAP_SEG) * a.modes;
        return hipSuccess;
    }
    if (own_masks(h, a) && h->qmap_host) {
#ifndef WBC_NO_QMAP  // (A/B builds only: the unmapped step)
        if (h->qmap_waves) {
            a.qmap = qmap;
            a.nwaves = h->qmap_waves;
        }
#endif
        return hipSuccess;
    }
    // device-bound masks: the map is built on the stream when the caller asks for it (WBC_GROUP);
    // otherwise waves take four consecutive QPs (same results; a wave of mixed masks costs more)
    if (!(flags & WBC_GROUP)) return hipSuccess;
    a.qmap = h->d_qmap;
    a.nwaves = wbc::qmap_capacity(h->batch) / wbc::QMAP_SEG;
    return wbc_launch_qmap(a.contacts, h->batch, h->d_qmap, h->stream);
}

// The default step's QPs are all stance QPs of the stance form: stateless, the engine's own masks
// (copied by the host, counted at copy time), every one 15, no map and no mode hypotheses.
bool step_all_stance(const wbc_engine* h, const wbc::KernelArgs& a) {
#ifdef WBC_NO_STANCE_TU  // (A/B builds only: the mixed-form kernel for every step)
    return false;
#else
    return own_masks(h, a) && h->qmap_host && h->n_stance_own == h->batch && !a.stateful && !a.modes && !a.qmap;
#endif
}

hipError_t launch_solves(wbc_engine* h, wbc::KernelArgs& a) {
    a.elim = h->elim ? 1 : 0;
    a.parity = h->elim_parity;
    return h->elim ? wbc_launch_solve_stance(&a, h->stream) : wbc_launch_solve_general(&a, h->stream);
}

// The per-robot tables are read by the default wbc_step (and the plain wbc_cycle) only: with one in
// force `call` is refused, outright (forms = 0) or when `flags` ask for one of `forms`.  The
// parameter table is named before the normals, then the base bodies, the limits, the force bounds, the force task last; `allowed` says
// what the call may still do.
int32_t refuse_tables(const wbc_engine* h, const char* call, uint32_t flags, uint32_t forms, const char* allowed) {
    if (forms && !(flags & forms)) return WBC_OK;
    const char* form = !forms ? nullptr : (flags & WBC_SPLIT) ? "WBC_SPLIT" : (flags & WBC_FUSED) ? "WBC_FUSED" : "WBC_RESIDENT";
    static const struct { RobotTable wbc_engine::*table; const char *what, *is, *clear; } kTables[] = {
        {&wbc_engine::rp, "a per-robot parameter table", " is in force", "it with wbc_set_robot_params"},
        {&wbc_engine::cn, "contact normals", " are in force", "them with wbc_set_contact_normals"},
        {&wbc_engine::bb, "a per-robot base body table", " is in force", "it with wbc_set_base_body"},
        {&wbc_engine::lm, "per-robot limits", " are in force", "them with wbc_set_limits"},
        {&wbc_engine::fn, "per-foot force bounds", " are in force", "them with wbc_set_force_bounds"},
        {&wbc_engine::ft, "a per-robot force task", " is in force", "it with wbc_set_force_task"},
    };
    for (const auto& t : kTables) {
        if (!(h->*t.table).in_force) continue;
        const std::string what = t.what;
        return fail(WBC_ERR_STATE, std::string(call) + ": " + (form ? form + (" with " + what) + " in force" : what + t.is) +
                                       " (" + allowed + "; clear " + t.clear + "(h, NULL))");
    }
    return WBC_OK;
}

// WBC_OBJECTIVE and WBC_BEST belong to wbc_step_modes' default form; every other call refuses them
constexpr uint32_t kModeOutFlags = WBC_OBJECTIVE | WBC_BEST;
int32_t refuse_mode_out_flags(const char* call, uint32_t flags) {
    if (!(flags & kModeOutFlags)) return WBC_OK;
    return fail(WBC_ERR_ARG, std::string(call) + ": WBC_OBJECTIVE / WBC_BEST are wbc_step_modes flags");
}
// WBC_DUALS belongs to wbc_step's default form; every other call refuses it
int32_t refuse_duals_flag(const char* call, uint32_t flags) {
    if (!(flags & WBC_DUALS)) return WBC_OK;
    return fail(WBC_ERR_ARG, std::string(call) + ": WBC_DUALS is a flag of the default wbc_step");
}
// and so does WBC_DUALS_FORCE (after every other check of the call)
int32_t refuse_force_duals_flag(const char* call, uint32_t flags) {
    if (!(flags & WBC_DUALS_FORCE)) return WBC_OK;
    return fail(WBC_ERR_ARG, std::string(call) + ": WBC_DUALS_FORCE is a flag of the default wbc_step");
}
// and so does WBC_DUALS_TASK (after every other check of the call)
int32_t refuse_task_duals_flag(const char* call, uint32_t flags) {
    if (!(flags & WBC_DUALS_TASK)) return WBC_OK;
    return fail(WBC_ERR_ARG, std::string(call) + ": WBC_DUALS_TASK is a flag of the default wbc_step");
}
}  // namespace

extern "C" {

int32_t wbc_default_params(wbc_params* p) {
    if (!p) return fail(WBC_ERR_ARG, "null params");
    std::memset(p, 0, sizeof(*p));
    p->friction = 1.0;       // params_controller.yaml:2
    p->loop_rate = 400.0;    // :3
    p->max_torque = 80.0;    // :4
    p->kp = 6000.0;          // :5
    p->kp_z = 10000.0;       // :6
    p->kd = 1800.0;          // :7
    p->ki = 0.0;             // :8
    p->kp_swing = 250.0;     // :9
    p->kd_swing = 20.0;      // :10
    p->slack_weight = 1000.0;  // :11
    const double pose[6] = {0.0, 0.0, 0.50, 0.0, 0.0, 0.0};  // :12
    std::memcpy(p->initial_reference_pose, pose, sizeof(pose));
    p->gravity = 9.81;       // hpp:30
    p->max_wsr = 100;        // cpp:517
    return WBC_OK;
}

int32_t wbc_anymal_model(wbc_model* m) {
    if (!m) return fail(WBC_ERR_ARG, "null model");
    *m = WBC_ANYMAL_MODEL;
    return WBC_OK;
}

int32_t wbc_create(const wbc_model* model, const wbc_params* params, int32_t batch, int32_t device, wbc_engine** out) {
    if (!out || batch <= 0) return fail(WBC_ERR_ARG, "wbc_create: bad arguments");
    if (batch > wbc::QMAP_MAX_BATCH) return fail(WBC_ERR_ARG, "wbc_create: batch above 2^27 - 1 (the wave map's index range)");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(WBC_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(WBC_ERR_ARG, "wbc_create: bad device index");
    WBC_HIP(hipSetDevice(device));
    wbc_engine* h = new (std::nothrow) wbc_engine();
    if (!h) return fail(WBC_ERR_ARG, "out of host memory");
    h->batch = batch;
    h->device = device;
    wbc_model m = model ? *model : WBC_ANYMAL_MODEL;
    wbc_params p;
    if (params) p = *params;
    else wbc_default_params(&p);
    if (p.loop_rate <= 0.0 || p.max_wsr <= 0) {
        delete h;
        return fail(WBC_ERR_ARG, "wbc_create: invalid params");
    }
    h->params = p;
    const size_t B = (size_t)batch;
#define ALLOC(ptr, n)                                             \
    if (dalloc(&h->ptr, (n)) != hipSuccess) {                     \
        wbc_destroy(h);                                           \
        return fail(WBC_ERR_HIP, "hipMalloc failed: " #ptr);      \
    }
    ALLOC(d_model, 1);
    ALLOC(d_params, 1);
    ALLOC(d_limg, wbc::LIMG_LEN);
    // (the input block in whole 8-byte words: the resident cycle copies it by words)
    if (hipMalloc(&h->d_inblk, 8 * wbc::input_block_words(B)) != hipSuccess ||
        hipMalloc(&h->d_outblk, wbc::output_block_bytes(B)) != hipSuccess) {
        wbc_destroy(h);
        return fail(WBC_ERR_HIP, "hipMalloc failed: input/output blocks");
    }
    h->own_in = wbc::input_view(h->d_inblk, B);
    h->own_out = wbc::output_view(h->d_outblk, B);
    ALLOC(d_mask, B);
    ALLOC(d_modes, WBC_MAX_MODES);
    ALLOC(d_hist, B * wbc::HIST_LEN);
    ALLOC(d_work, B * wbc::WORK_LEN);
    ALLOC(d_fb, 2 + B);
    ALLOC(d_dbg, B * WBC_DBG_LEN);
    ALLOC(d_qmap, wbc::qmap_capacity(batch) + wbc::qmap_scratch(batch));  // + the device builder's scratch
#undef ALLOC
    if (hipHostMalloc(&h->h_qmap, sizeof(int32_t) * wbc::qmap_capacity(batch), hipHostMallocMapped) != hipSuccess) {
        wbc_destroy(h);
        return fail(WBC_ERR_HIP, "hipHostMalloc failed: wave map");
    }
    if (B <= (size_t)wbc::QMAP_SEG) {  // the resident cycle's code and mailbox, made ready now
        (void)wbc_preload_resident();
        if (resident_alloc(h) != hipSuccess) {
            wbc_destroy(h);
            return fail(WBC_ERR_HIP, "resident cycle mailbox / stream");
        }
    }
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        wbc_destroy(h);
        return fail(WBC_ERR_HIP, "stream/event creation failed");
    }
    h->stream = h->own_stream;
    h->n_stance_own = B;  // d_contacts starts as all-stance (15), below
    h->in = wbc::const_view(h->own_in);
    h->out = h->own_out;
    hipStream_t st = h->stream;
    wbc::LdsImage limg;
    wbc::build_lds_image(m, p.friction, limg);
    h->base_row[WBC_BB_MASS] = m.base_mass;
    for (int i = 0; i < 3; ++i) h->base_row[WBC_BB_COM + i] = m.base_com[i];
    for (int i = 0; i < 9; ++i) h->base_row[WBC_BB_INERTIA + i] = m.base_inertia[i];
    if (hipMemcpyAsync(h->d_model, &m, sizeof(m), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(h->d_params, &p, sizeof(p), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(h->d_limg, &limg, sizeof(limg), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(h->own_in.pose, 0, B * WBC_POSE_LEN * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->own_in.nu, 0, B * WBC_NU_LEN * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->own_in.qj, 0, B * WBC_NUM_JOINTS * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->own_in.ref, 0, B * WBC_REF_LEN * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->own_in.contacts, 15, B, st) != hipSuccess ||
        hipMemsetAsync(h->own_in.switching, 0, B, st) != hipSuccess ||
        hipMemsetAsync(h->own_out.status, 0, B * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(h->own_out.iters, 0, B * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(h->own_out.tau, 0, B * WBC_NUM_JOINTS * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->own_out.grf, 0, B * WBC_NUM_JOINTS * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->own_out.x, 0, B * WBC_NV * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->d_dbg, 0, B * WBC_DBG_LEN * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(h->d_fb, 0, (2 + B) * sizeof(int32_t), st) != hipSuccess ||
        wbc_launch_reset(h->d_hist, nullptr, batch, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        wbc_destroy(h);
        return fail(WBC_ERR_HIP, "wbc_create: initialisation failed");
    }
    *out = h;
    return WBC_OK;
}

int32_t wbc_destroy(wbc_engine* h) {
    if (!h) return WBC_OK;
    (void)hipSetDevice(h->device);
    // drain the engine's in-flight work before freeing (the bound stream; never the whole device,
    // which would also wait for other engines' and the caller's unrelated work)
    (void)drain(h);
    {
        std::lock_guard<std::recursive_mutex> lk(g_res_mu);
        (void)resident_stop(h);
        if (g_res_owner == h) g_res_owner = nullptr;  // never left pointing at a freed engine
    }
    if (h->res_box) (void)hipHostFree(h->res_box);
    if (h->res_stream) (void)hipStreamDestroy(h->res_stream);
    void* ptrs[] = {h->d_model, h->d_params, h->d_limg, h->d_inblk, h->d_outblk, h->d_mask, h->d_modes, h->d_hist, h->d_work,
                    h->d_fb, h->d_dbg, h->d_qmap, h->rp.own, h->cn.own, h->d_rp_uni, h->bb.own, h->d_cn_flat,
                    h->d_obj, h->d_best, h->d_best_obj, h->d_best_tau, h->d_best_grf, h->d_dual, h->d_bb_def, h->lm.own, h->fn.own,
                    h->d_dual48, h->d_fn_none, h->ft.own, h->d_ft_plain};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_in) (void)hipHostFree(h->h_in);
    if (h->h_out) (void)hipHostFree(h->h_out);
    if (h->h_qmap) (void)hipHostFree(h->h_qmap);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return WBC_OK;
}

int32_t wbc_batch(const wbc_engine* h) { return h ? h->batch : 0; }

int32_t wbc_set_stream(wbc_engine* h, void* stream) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    const hipStream_t next = stream ? reinterpret_cast<hipStream_t>(stream) : h->own_stream;
    if (next != h->stream) {
        // work already queued on the old stream still reads the engine's buffers: let it finish
        // before any call on the new stream can overwrite them
        WBC_HIP(hipSetDevice(h->device));
        WBC_HIP(drain(h));
    }
    h->stream = next;
    return WBC_OK;
}

int32_t wbc_set_state(wbc_engine* h, const double* base_pose, const double* nu, const double* qj) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    WBC_HIP(hipSetDevice(h->device));
    const size_t B = input_rows(h);
    if (base_pose) { WBC_HIP(hipMemcpyAsync(h->own_in.pose, base_pose, B * WBC_POSE_LEN * sizeof(double), hipMemcpyHostToDevice, h->stream)); h->in.pose = h->own_in.pose; }
    if (nu) { WBC_HIP(hipMemcpyAsync(h->own_in.nu, nu, B * WBC_NU_LEN * sizeof(double), hipMemcpyHostToDevice, h->stream)); h->in.nu = h->own_in.nu; }
    if (qj) { WBC_HIP(hipMemcpyAsync(h->own_in.qj, qj, B * WBC_NUM_JOINTS * sizeof(double), hipMemcpyHostToDevice, h->stream)); h->in.qj = h->own_in.qj; }
    WBC_HIP(hipStreamSynchronize(h->stream));  // host buffers may be reused by the caller
    return WBC_OK;
}

int32_t wbc_set_reference(wbc_engine* h, const double* ref, const uint8_t* contacts, const uint8_t* switching) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    WBC_HIP(hipSetDevice(h->device));
    const size_t B = input_rows(h);
    if (ref) { WBC_HIP(hipMemcpyAsync(h->own_in.ref, ref, B * WBC_REF_LEN * sizeof(double), hipMemcpyHostToDevice, h->stream)); h->in.ref = h->own_in.ref; }
    if (contacts) {
        WBC_HIP(hipMemcpyAsync(h->own_in.contacts, contacts, B, hipMemcpyHostToDevice, h->stream));
        h->in.contacts = h->own_in.contacts;
        h->n_stance_own = count_stance(contacts, B);
        // the wave map of these masks (rows = QPs; under mode hypotheses contacts[] is not read)
        if (!h->n_modes) WBC_HIP(upload_qmap(h, contacts));
    }
    if (switching) { WBC_HIP(hipMemcpyAsync(h->own_in.switching, switching, B, hipMemcpyHostToDevice, h->stream)); h->in.switching = h->own_in.switching; }
    WBC_HIP(hipStreamSynchronize(h->stream));
    return WBC_OK;
}

int32_t wbc_bind_device_inputs(wbc_engine* h, const double* d_base_pose, const double* d_nu, const double* d_qj,
                               const double* d_ref, const uint8_t* d_contacts, const uint8_t* d_switching) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    h->in.pose = d_base_pose ? d_base_pose : h->own_in.pose;
    h->in.nu = d_nu ? d_nu : h->own_in.nu;
    h->in.qj = d_qj ? d_qj : h->own_in.qj;
    h->in.ref = d_ref ? d_ref : h->own_in.ref;
    h->in.contacts = d_contacts ? d_contacts : h->own_in.contacts;
    h->in.switching = d_switching ? d_switching : h->own_in.switching;
    return WBC_OK;
}

int32_t wbc_bind_device_outputs(wbc_engine* h, double* d_tau, double* d_grf, double* d_x, int32_t* d_status,
                                int32_t* d_iters) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    h->out.tau = d_tau ? d_tau : h->own_out.tau;
    h->out.grf = d_grf ? d_grf : h->own_out.grf;
    h->out.x = d_x ? d_x : h->own_out.x;
    h->out.status = d_status ? d_status : h->own_out.status;
    h->out.iters = d_iters ? d_iters : h->own_out.iters;
    return WBC_OK;
}

// the engine-wide params as a row of the parameter table (the reserved column 0)
static void rp_engine_row(const wbc_params& p, double* row) {
    const double r[WBC_RP_LEN] = {p.friction, p.max_torque, p.kp, p.kp_z, p.kd, p.ki, p.kp_swing, p.kd_swing, p.slack_weight, 0.0};
    std::memcpy(row, r, sizeof(r));
}
// an engine-owned device table of B equal rows (built once: *slot stays)
static int32_t ensure_uniform(wbc_engine* h, double** slot, const double* row, size_t len, const char* what) {
    if (*slot) return WBC_OK;
    const size_t B = (size_t)h->batch;
    std::vector<double> t(B * len);
    for (size_t b = 0; b < B; ++b) std::memcpy(t.data() + b * len, row, len * sizeof(double));
    WBC_HIP(hipSetDevice(h->device));
    double* d = nullptr;
    if (dalloc(&d, B * len) != hipSuccess) return fail(WBC_ERR_HIP, std::string("hipMalloc failed: ") + what);
    const hipError_t e = hipMemcpy(d, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(WBC_ERR_HIP, std::string("hipMemcpy failed: ") + what + ": " + hipGetErrorString(e));
    }
    *slot = d;
    return WBC_OK;
}
static const double kFlatNormals[WBC_CN_LEN] = {0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0};
// the uniform parameter table the contact-normal kernels read when no parameter table is in force
static int32_t ensure_rp_uniform(wbc_engine* h) {
    double row[WBC_RP_LEN];
    rp_engine_row(h->params, row);
    return ensure_uniform(h, &h->d_rp_uni, row, WBC_RP_LEN, "d_rp_uni");
}
// and the flat normals the base-body kernels read when no normals are in force
static int32_t ensure_rp_cn_uniform(wbc_engine* h) {
    if (const int32_t rc = ensure_rp_uniform(h)) return rc;
    return ensure_uniform(h, &h->d_cn_flat, kFlatNormals, WBC_CN_LEN, "d_cn_flat");
}

// and the model's base in B rows, which the limits kernels (and the duals kernels) read when no
// base-body table is in force
static int32_t ensure_rp_cn_bb_uniform(wbc_engine* h) {
    if (const int32_t rc = ensure_rp_cn_uniform(h)) return rc;
    return ensure_uniform(h, &h->d_bb_def, h->base_row, WBC_BB_LEN, "d_bb_def");
}
// and the no-bounds rows a WBC_DUALS_FORCE step reads when no force-bound table is in force
static int32_t ensure_fn_none(wbc_engine* h) {
    const double inf = std::numeric_limits<double>::infinity();
    const double row[WBC_FN_LEN] = {-inf, -inf, -inf, -inf, inf, inf, inf, inf};
    return ensure_uniform(h, &h->d_fn_none, row, WBC_FN_LEN, "d_fn_none");
}

// The three calls of a per-robot table (RobotTable), for the parameters and for the normals.  What
// differs is passed in: `call` (the C entry point, for messages), `what` (the own table's name in
// allocation errors), row_error (why the host refuses row b, or "" for a row it accepts), uniform
// (the table's kernels read other tables too: ensure_rp_uniform, ensure_rp_cn_uniform, ensure_rp_cn_bb_uniform; or null) and,
// to read back without a table in force, the default rows.
// Set from the host: a refused table leaves the previous one in force.
static int32_t table_set(wbc_engine* h, RobotTable wbc_engine::*which, const double* table, const char* call,
                         const char* what, std::string (*row_error)(const double* row), int32_t (*uniform)(wbc_engine*)) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    RobotTable& t = h->*which;
    if (!table) {  // back to no table of the engine's own (or to a caller's bound table)
        t.has_own = false;
        t.in_force = t.bound;
        return WBC_OK;
    }
    const size_t B = (size_t)h->batch;
    for (size_t b = 0; b < B; ++b) {
        const std::string why = row_error(table + b * t.row);
        if (!why.empty()) return fail(WBC_ERR_ARG, std::string(call) + ": row " + std::to_string(b) + ", " + why);
    }
    WBC_HIP(sync_own(h));
    if (uniform) {
        if (const int32_t rc = uniform(h)) return rc;
    }
    WBC_HIP(hipSetDevice(h->device));
    if (!t.own && dalloc(&t.own, B * t.row) != hipSuccess) return fail(WBC_ERR_HIP, std::string("hipMalloc failed: ") + what);
    WBC_HIP(hipMemcpyAsync(t.own, table, B * t.row * sizeof(double), hipMemcpyHostToDevice, h->stream));
    WBC_HIP(hipStreamSynchronize(h->stream));  // the host table may be reused by the caller
    t.has_own = true;
    if (!t.bound) t.in_force = t.own;
    return WBC_OK;
}
// Bind a caller's device table (no copy, no host validation), or unbind it (null)
static int32_t table_bind(wbc_engine* h, RobotTable wbc_engine::*which, const double* d_table, const char* call,
                          int32_t (*uniform)(wbc_engine*)) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    RobotTable& t = h->*which;
    if (d_table && (reinterpret_cast<uintptr_t>(d_table) & 15u))
        return fail(WBC_ERR_ARG, std::string(call) + ": the table must be 16-byte aligned");
    if (d_table && uniform) {
        if (const int32_t rc = uniform(h)) return rc;
    }
    t.bound = d_table;
    t.in_force = d_table ? d_table : (t.has_own ? t.own : nullptr);
    return WBC_OK;
}
// Read back the table in force, or `defaults` in every row
static int32_t table_get(wbc_engine* h, RobotTable wbc_engine::*which, double* table, const double* defaults) {
    if (!h || !table) return fail(WBC_ERR_ARG, "null argument");
    const RobotTable& t = h->*which;
    const size_t B = (size_t)h->batch;
    if (t.in_force) {
        WBC_HIP(sync_own(h));
        WBC_HIP(hipSetDevice(h->device));
        WBC_HIP(hipMemcpyAsync(table, t.in_force, B * t.row * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        WBC_HIP(hipStreamSynchronize(h->stream));
    } else {
        for (size_t b = 0; b < B; ++b) std::memcpy(table + b * t.row, defaults, t.row * sizeof(double));
    }
    return WBC_OK;
}

static std::string rp_row_error(const double* row) {
    static const char* const names[WBC_RP_LEN - 1] = {"friction", "max_torque", "kp", "kp_z", "kd", "ki", "kp_swing", "kd_swing",
                                                      "slack_weight"};
    const int c = wbc::rp_bad_column(row);
    if (c < 0) return "";
    char val[32];
    std::snprintf(val, sizeof(val), "%g", row[c]);
    return "column " + std::to_string(c) + " (" + names[c] + ") = " + val +
           ": need finite entries, friction >= 0, max_torque >= 0, slack_weight > 0";
}
static std::string bb_row_error(const double* row) {
    static const char* const names[WBC_BB_LEN - 1] = {"mass", "com_x", "com_y", "com_z", "I_xx", "I_xy", "I_xz", "I_yx", "I_yy",
                                                      "I_yz", "I_zx", "I_zy", "I_zz"};
    const int c = wbc::bb_bad_entry(row);
    if (c < 0) return "";
    char val[32];
    std::snprintf(val, sizeof(val), "%g", row[c]);
    return "column " + std::to_string(c) + " (" + names[c] + ") = " + val +
           ": need finite entries, mass > 0 and a symmetric (to 1e-9 of its trace), positive definite inertia";
}
static std::string lm_row_error(const double* row) {
    const int c = wbc::lm_bad_column(row);
    if (c < 0) return "";
    const char* group = c < WBC_LM_TAU_MAX ? "tau_min" : c < WBC_LM_FRICTION ? "tau_max" : "friction";
    const int k = c < WBC_LM_TAU_MAX ? c : c < WBC_LM_FRICTION ? c - WBC_LM_TAU_MAX : c - WBC_LM_FRICTION;
    char val[32];
    std::snprintf(val, sizeof(val), "%g", row[c]);
    return "column " + std::to_string(c) + " (" + group + "[" + std::to_string(k) + "]) = " + val +
           ": need finite entries, tau_min <= tau_max per joint, friction >= 0";
}
static std::string cn_row_error(const double* row) {
    static const char* const feet[WBC_NUM_LEGS] = {"LH", "LF", "RF", "RH"};
    const int l = wbc::cn_bad_foot(row);
    if (l < 0) return "";
    const double* m = row + 3 * l;
    char val[96];
    std::snprintf(val, sizeof(val), "(%g, %g, %g)", m[0], m[1], m[2]);
    return "foot " + std::to_string(l) + " (" + feet[l] + ") = " + val +
           ": need finite entries, 0.25 <= |m|^2 <= 4 and m_z / |m| >= 0.5";
}

int32_t wbc_set_robot_params(wbc_engine* h, const double* table) {
    return table_set(h, &wbc_engine::rp, table, "wbc_set_robot_params", "d_rp", rp_row_error, nullptr);
}
int32_t wbc_bind_device_robot_params(wbc_engine* h, const double* d_table) {
    return table_bind(h, &wbc_engine::rp, d_table, "wbc_bind_device_robot_params", nullptr);
}
int32_t wbc_get_robot_params(wbc_engine* h, double* table) {
    if (!h || !table) return fail(WBC_ERR_ARG, "null argument");
    double row[WBC_RP_LEN];
    rp_engine_row(h->params, row);
    if (const int32_t rc = table_get(h, &wbc_engine::rp, table, row)) return rc;
    for (size_t b = 0; b < (size_t)h->batch; ++b) table[b * WBC_RP_LEN + WBC_RP_LEN - 1] = 0.0;  // the reserved column
    return WBC_OK;
}

int32_t wbc_set_contact_normals(wbc_engine* h, const double* table) {
    return table_set(h, &wbc_engine::cn, table, "wbc_set_contact_normals", "d_cn", cn_row_error, ensure_rp_uniform);
}
int32_t wbc_bind_device_contact_normals(wbc_engine* h, const double* d_table) {
    return table_bind(h, &wbc_engine::cn, d_table, "wbc_bind_device_contact_normals", ensure_rp_uniform);
}
int32_t wbc_get_contact_normals(wbc_engine* h, double* table) {
    return table_get(h, &wbc_engine::cn, table, kFlatNormals);
}

int32_t wbc_set_base_body(wbc_engine* h, const double* table) {
    return table_set(h, &wbc_engine::bb, table, "wbc_set_base_body", "d_bb", bb_row_error, ensure_rp_cn_uniform);
}
int32_t wbc_bind_device_base_body(wbc_engine* h, const double* d_table) {
    return table_bind(h, &wbc_engine::bb, d_table, "wbc_bind_device_base_body", ensure_rp_cn_uniform);
}
int32_t wbc_get_base_body(wbc_engine* h, double* table) {
    if (!h || !table) return fail(WBC_ERR_ARG, "null argument");
    if (const int32_t rc = table_get(h, &wbc_engine::bb, table, h->base_row)) return rc;
    for (size_t b = 0; b < (size_t)h->batch; ++b) table[b * WBC_BB_LEN + WBC_BB_LEN - 1] = 0.0;  // the reserved column
    return WBC_OK;
}

int32_t wbc_set_limits(wbc_engine* h, const double* table) {
    return table_set(h, &wbc_engine::lm, table, "wbc_set_limits", "d_lm", lm_row_error, ensure_rp_cn_bb_uniform);
}
int32_t wbc_bind_device_limits(wbc_engine* h, const double* d_table) {
    return table_bind(h, &wbc_engine::lm, d_table, "wbc_bind_device_limits", ensure_rp_cn_bb_uniform);
}
// Without a limits table: each robot's -+max_torque and friction, from its parameter row when a
// parameter table is in force, else from the engine-wide params
int32_t wbc_get_limits(wbc_engine* h, double* table) {
    if (!h || !table) return fail(WBC_ERR_ARG, "null argument");
    if (h->lm.in_force) return table_get(h, &wbc_engine::lm, table, nullptr);
    const size_t B = (size_t)h->batch;
    std::vector<double> rp(B * WBC_RP_LEN);
    if (const int32_t rc = wbc_get_robot_params(h, rp.data())) return rc;
    for (size_t b = 0; b < B; ++b) {
        double* row = table + b * WBC_LM_LEN;
        const double T = rp[b * WBC_RP_LEN + WBC_RP_MAX_TORQUE], mu = rp[b * WBC_RP_LEN + WBC_RP_FRICTION];
        for (int j = 0; j < WBC_NUM_JOINTS; ++j) {
            row[WBC_LM_TAU_MIN + j] = -T;
            row[WBC_LM_TAU_MAX + j] = T;
        }
        for (int l = 0; l < WBC_NUM_LEGS; ++l) row[WBC_LM_FRICTION + l] = mu;
    }
    return WBC_OK;
}

static std::string fn_row_error(const double* row) {
    const int c = wbc::fn_bad_column(row);
    if (c < 0) return "";
    const char* group = c < WBC_FN_MAX ? "fn_min" : "fn_max";
    char val[32];
    std::snprintf(val, sizeof(val), "%g", row[c]);
    return "column " + std::to_string(c) + " (" + group + "[" + std::to_string(c % WBC_NUM_LEGS) + "]) = " + val +
           ": need no NaN, fn_min < +inf, fn_max > -inf and fn_min <= fn_max per foot";
}
// The force-bound kernels read the parameter, normal and base-body tables too (the engine's own where none
// is in force) and take a null limits table (each robot's own -+max_torque and friction)
int32_t wbc_set_force_bounds(wbc_engine* h, const double* table) {
    return table_set(h, &wbc_engine::fn, table, "wbc_set_force_bounds", "d_fn", fn_row_error, ensure_rp_cn_bb_uniform);
}
int32_t wbc_bind_device_force_bounds(wbc_engine* h, const double* d_table) {
    return table_bind(h, &wbc_engine::fn, d_table, "wbc_bind_device_force_bounds", ensure_rp_cn_bb_uniform);
}
int32_t wbc_get_force_bounds(wbc_engine* h, double* table) {
    const double inf = std::numeric_limits<double>::infinity();
    const double none[WBC_FN_LEN] = {-inf, -inf, -inf, -inf, inf, inf, inf, inf};
    return table_get(h, &wbc_engine::fn, table, none);
}

static std::string ft_row_error(const double* row) {
    const int c = wbc::ft_bad_column(row);
    if (c < 0) return "";
    char val[32];
    std::snprintf(val, sizeof(val), "%g", row[c]);
    const std::string name = c < WBC_FT_WEIGHT ? "f_ref[" + std::to_string(c / 3) + "][" + std::to_string(c % 3) + "]" : "weight";
    return "column " + std::to_string(c) + " (" + name + ") = " + val + ": need finite f_ref and a finite weight > 0";
}
// The force-task kernels read every other table too: the engine's own parameter, normal, base-body and no-bounds
// tables where none is in force, and a null limits table as the force-bound kernels take it
static int32_t ensure_ft_tables(wbc_engine* h) {
    if (const int32_t rc = ensure_rp_cn_bb_uniform(h)) return rc;
    return ensure_fn_none(h);
}
static const double kPlainForceTask[WBC_FT_LEN] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
// the plain-task rows a WBC_DUALS_TASK step reads when no force-task table is in force
static int32_t ensure_ft_plain(wbc_engine* h) { return ensure_uniform(h, &h->d_ft_plain, kPlainForceTask, WBC_FT_LEN, "d_ft_plain"); }
int32_t wbc_set_force_task(wbc_engine* h, const double* table) {
    return table_set(h, &wbc_engine::ft, table, "wbc_set_force_task", "d_ft", ft_row_error, ensure_ft_tables);
}
int32_t wbc_bind_device_force_task(wbc_engine* h, const double* d_table) {
    return table_bind(h, &wbc_engine::ft, d_table, "wbc_bind_device_force_task", ensure_ft_tables);
}
int32_t wbc_get_force_task(wbc_engine* h, double* table) {
    if (!h || !table) return fail(WBC_ERR_ARG, "null argument");
    if (const int32_t rc = table_get(h, &wbc_engine::ft, table, kPlainForceTask)) return rc;
    for (size_t b = 0; b < (size_t)h->batch; ++b) table[b * WBC_FT_LEN + WBC_FT_LEN - 1] = 0.0;  // the reserved column
    return WBC_OK;
}

int32_t wbc_reset(wbc_engine* h, const uint8_t* mask) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    WBC_HIP(hipSetDevice(h->device));
    const uint8_t* dm = nullptr;
    if (mask) {
        WBC_HIP(hipMemcpyAsync(h->d_mask, mask, (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
        dm = h->d_mask;
    }
    WBC_HIP(wbc_launch_reset(h->d_hist, dm, h->batch, h->stream));
    WBC_HIP(hipStreamSynchronize(h->stream));
    h->updated = false;
    return WBC_OK;
}

int32_t wbc_update(wbc_engine* h, uint32_t flags) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    if (h->n_modes) return fail(WBC_ERR_STATE, "wbc_update: mode hypotheses are set (use wbc_step_modes, or wbc_set_modes(h, 0, NULL))");
    if (const int32_t rc = refuse_tables(h, "wbc_update", flags, 0, "default wbc_step only")) return rc;
    if (const int32_t rc = refuse_mode_out_flags("wbc_update", flags)) return rc;
    if (const int32_t rc = refuse_duals_flag("wbc_update", flags)) return rc;
    if (const int32_t rc = refuse_force_duals_flag("wbc_update", flags)) return rc;
    if (const int32_t rc = refuse_task_duals_flag("wbc_update", flags)) return rc;
    WBC_HIP(hipSetDevice(h->device));
    wbc::KernelArgs a = make_args(h, flags);
    begin_update(h, a);
    WBC_HIP(wbc_launch_update(&a, h->stream));
    h->updated = true;
    return WBC_OK;
}

int32_t wbc_solve(wbc_engine* h, uint32_t flags) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    if (h->n_modes) return fail(WBC_ERR_STATE, "wbc_solve: mode hypotheses are set (use wbc_step_modes, or wbc_set_modes(h, 0, NULL))");
    if (const int32_t rc = refuse_tables(h, "wbc_solve", flags, 0, "default wbc_step only")) return rc;
    if (const int32_t rc = refuse_mode_out_flags("wbc_solve", flags)) return rc;
    if (const int32_t rc = refuse_duals_flag("wbc_solve", flags)) return rc;
    if (!h->updated) return fail(WBC_ERR_STATE, "wbc_solve before wbc_update");
    if (const int32_t rc = refuse_force_duals_flag("wbc_solve", flags)) return rc;
    if (const int32_t rc = refuse_task_duals_flag("wbc_solve", flags)) return rc;
    WBC_HIP(hipSetDevice(h->device));
    wbc::KernelArgs a = make_args(h, flags);
    WBC_HIP(launch_solves(h, a));
    return WBC_OK;  // the assembled problem stays valid: solving it again gives the same result
}

// One step on the inputs, outputs and wave map of `io` (wbc_step: the handle's bindings;
// enqueue_cycle: the cycle's blocks)
static int32_t step_on(wbc_engine* h, uint32_t flags, const StepIO& io) {
    WBC_HIP(sync_own(h));
    if (h->n_modes) return fail(WBC_ERR_STATE, "wbc_step: mode hypotheses are set (use wbc_step_modes, or wbc_set_modes(h, 0, NULL))");
    if (const int32_t rc = refuse_tables(h, "wbc_step", flags, WBC_SPLIT | WBC_FUSED, "default form only")) return rc;
    if (const int32_t rc = refuse_mode_out_flags("wbc_step", flags)) return rc;
    // WBC_DUALS_FORCE implies WBC_DUALS, whose bit is ignored beside it (as WBC_BEST implies WBC_OBJECTIVE): the 48-entry
    // form has kernels, a buffer and getters of its own, and WBC_DUALS alone keeps its refusal under force bounds
    // WBC_DUALS_TASK implies WBC_DUALS_FORCE in the same way: the same 48 entries, buffer and getters from the force-task
    // units' duals instances, with or without a force-task table; the two older flags keep their refusals under one
    const bool dtask = (flags & WBC_DUALS_TASK) != 0;
    const bool dforce = (flags & WBC_DUALS_FORCE) != 0 && !dtask;
    const bool duals = (flags & WBC_DUALS) != 0 && !dforce && !dtask;
    if (duals && (flags & (WBC_SPLIT | WBC_FUSED | WBC_RESIDENT)))
        return fail(WBC_ERR_ARG, "wbc_step: WBC_DUALS belongs to the default form (not WBC_SPLIT / WBC_FUSED / WBC_RESIDENT)");
    if (duals && h->fn.in_force)
        return fail(WBC_ERR_STATE, "wbc_step: WBC_DUALS with per-foot force bounds in force (the 40 multipliers have no entry "
                                   "for a force row; clear them with wbc_set_force_bounds(h, NULL))");
    if ((duals || dforce) && h->ft.in_force)
        return fail(WBC_ERR_STATE, std::string("wbc_step: ") + (dforce ? "WBC_DUALS_FORCE" : "WBC_DUALS") +
                                       " with a per-robot force task in force (no duals instance reads the table; clear it "
                                       "with wbc_set_force_task(h, NULL))");
    if (dforce && (flags & (WBC_SPLIT | WBC_FUSED | WBC_RESIDENT)))
        return fail(WBC_ERR_ARG, "wbc_step: WBC_DUALS_FORCE belongs to the default form (not WBC_SPLIT / WBC_FUSED / WBC_RESIDENT)");
    if (dtask && (flags & (WBC_SPLIT | WBC_FUSED | WBC_RESIDENT)))
        return fail(WBC_ERR_ARG, "wbc_step: WBC_DUALS_TASK belongs to the default form (not WBC_SPLIT / WBC_FUSED / WBC_RESIDENT)");
    h->step_duals = wbc_engine::DUALS_NONE;
    if (duals || dforce || dtask) {  // the engine's own tables for the ones the caller has not set, and the buffer
        if (const int32_t rc = ensure_rp_cn_bb_uniform(h)) return rc;
    }
    if ((dforce || dtask) && !h->fn.in_force) {
        if (const int32_t rc = ensure_fn_none(h)) return rc;
    }
    if (dtask && !h->ft.in_force) {
        if (const int32_t rc = ensure_ft_plain(h)) return rc;
    }
    WBC_HIP(hipSetDevice(h->device));
    if (duals && !h->d_dual) WBC_HIP(dalloc(&h->d_dual, (size_t)h->batch * WBC_DUAL_LEN));
    if ((dforce || dtask) && !h->d_dual48) WBC_HIP(dalloc(&h->d_dual48, (size_t)h->batch * WBC_DUAL_FORCE_LEN));
    wbc::KernelArgs a = make_args(h, flags, io.in, io.out);
    if (duals || dforce || dtask) {
        if (!a.rp) a.rp = h->d_rp_uni;
        if (!a.cn) a.cn = h->d_cn_flat;
        if (!a.bb) a.bb = h->d_bb_def;
        a.dual = duals ? h->d_dual : h->d_dual48;
    }
    if ((dforce || dtask) && !a.fn) a.fn = h->d_fn_none;  // (a missing limits table stays a null KernelArgs::lm, as in fn0 / fn1)
    if (dtask && !a.ft) a.ft = h->d_ft_plain;
    const bool timed = (flags & WBC_TIMED) != 0;  // event packets cost a few us between kernels
    if (timed) WBC_HIP(hipEventRecord(h->ev0, h->stream));
    if (flags & WBC_SPLIT) {
        // the split kernels: update (records to HBM), then the general / stance solve kernels
        begin_update(h, a);
        WBC_HIP(wbc_launch_update(&a, h->stream));
        WBC_HIP(launch_solves(h, a));
    } else if (flags & WBC_FUSED) {
        WBC_HIP(wbc_launch_step(&a, h->stream));  // one robot per wave, the general method
    } else {
        // default: one kernel, every QP reduced to 12 variables and solved in the update wave.  Its
        // instance (wbc_layout.h step_instance, one kernel unit each): a stateless step whose masks the
        // host knows to be all 15 (no map then) runs the stance-only one, scheduled for it alone
        // (DESIGN.md 4.22), any other step the stateless or the stateful one; the same three under a
        // per-robot parameter table in force and under contact normals, which read the
        // parameter table too (the caller's, or the engine's uniform one), and under a
        // base-body table, which reads normals and parameters too; the stateless or the
        // stateful one under a limits table, which reads all three, under a force-bound table
        //  and under a force-task table, which reads every other one
        WBC_HIP(begin_step16(h, a, flags, io.qmap));
        // WBC_DUALS: the duals instance of (stateful), whatever the tables and masks; under
        // a limits table the limits units' own
        // WBC_DUALS_FORCE: the force-bound units' duals instance, whatever the tables
        // WBC_DUALS_TASK: the force-task units' duals instance, whatever the tables
        if (dtask) {
            WBC_HIP((a.stateful ? wbc_launch_update_solve_ftd1 : wbc_launch_update_solve_ftd0)(&a, h->stream));
        } else if (dforce) {
            WBC_HIP((a.stateful ? wbc_launch_update_solve_fnd1 : wbc_launch_update_solve_fnd0)(&a, h->stream));
        } else if (duals && a.lm) {
            WBC_HIP((a.stateful ? wbc_launch_update_solve_lmd1 : wbc_launch_update_solve_lmd0)(&a, h->stream));
        } else if (duals) {
            WBC_HIP((a.stateful ? wbc_launch_update_solve_du1 : wbc_launch_update_solve_du0)(&a, h->stream));
        } else {
            WBC_HIP(kStepLaunchers[wbc::step_instance(a.cn != nullptr, a.rp != nullptr, step_all_stance(h, a), a.stateful != 0, a.bb != nullptr,
                                                      a.lm != nullptr, a.fn != nullptr, a.ft != nullptr)](&a, h->stream));
        }
    }
    if (timed) {
        WBC_HIP(hipEventRecord(h->ev1, h->stream));
        h->timed = true;
    }
    h->updated = false;
    h->step_duals = (dforce || dtask) ? wbc_engine::DUALS_48 : duals ? wbc_engine::DUALS_40 : wbc_engine::DUALS_NONE;
    return WBC_OK;
}

int32_t wbc_step(wbc_engine* h, uint32_t flags) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    return step_on(h, flags, bound_io(h));
}

int32_t wbc_set_modes(wbc_engine* h, int32_t n_modes, const uint8_t* modes) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    // contacts[] copied while modes were set hold S rows only: the engine's own masks get their
    // wave map on the device from here on, until the next wbc_set_reference / wbc_cycle with masks
    h->qmap_host = false;
    h->modes_flags = 0;  // the objective and best-mode buffers describe the previous hypotheses
    if (n_modes == 0) {
        h->n_modes = 0;
        return WBC_OK;
    }
    if (n_modes < 0 || n_modes > WBC_MAX_MODES || !modes || h->batch % n_modes != 0)
        return fail(WBC_ERR_ARG, "wbc_set_modes: need 1 <= n_modes <= WBC_MAX_MODES dividing the batch, and masks");
    for (int32_t k = 0; k < n_modes; ++k)
        if (modes[k] > 15) return fail(WBC_ERR_ARG, "wbc_set_modes: contact masks are 4-bit");
    WBC_HIP(hipSetDevice(h->device));
    WBC_HIP(hipMemcpyAsync(h->d_modes, modes, (size_t)n_modes, hipMemcpyHostToDevice, h->stream));
    WBC_HIP(hipStreamSynchronize(h->stream));
    h->n_modes = n_modes;
    h->modes_stance = (int32_t)count_stance(modes, (size_t)n_modes);
    plan_mode_loop(h, modes, n_modes);
    return WBC_OK;
}

int32_t wbc_step_modes(wbc_engine* h, uint32_t flags) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    if (!h->n_modes) return fail(WBC_ERR_STATE, "wbc_step_modes: no mode hypotheses set (wbc_set_modes)");
    if (const int32_t rc = refuse_tables(h, "wbc_step_modes", flags, 0, "default wbc_step only")) return rc;
    if (!(flags & WBC_STATELESS)) return fail(WBC_ERR_ARG, "wbc_step_modes: hypotheses are cold steps (WBC_STATELESS)");
    if (flags & WBC_DEBUG) return fail(WBC_ERR_ARG, "wbc_step_modes: no debug records for hypotheses");
    if (const int32_t rc = refuse_duals_flag("wbc_step_modes", flags)) return rc;
    if (const int32_t rc = refuse_force_duals_flag("wbc_step_modes", flags)) return rc;
    if (const int32_t rc = refuse_task_duals_flag("wbc_step_modes", flags)) return rc;
    const uint32_t mode_out = (flags & WBC_BEST) ? kModeOutFlags : (flags & WBC_OBJECTIVE);  // WBC_BEST implies WBC_OBJECTIVE
    if (mode_out && (flags & WBC_SPLIT))
        return fail(WBC_ERR_ARG, "wbc_step_modes: WBC_OBJECTIVE / WBC_BEST belong to the default form (not WBC_SPLIT)");
    WBC_HIP(hipSetDevice(h->device));
    const size_t B = (size_t)h->batch;
    if (mode_out && !h->d_obj) WBC_HIP(dalloc(&h->d_obj, B));
    if ((mode_out & WBC_BEST) && !h->d_best_grf) {  // (the last of the four: a failed allocation is tried again)
        if (!h->d_best) WBC_HIP(dalloc(&h->d_best, B));
        if (!h->d_best_obj) WBC_HIP(dalloc(&h->d_best_obj, B));
        if (!h->d_best_tau) WBC_HIP(dalloc(&h->d_best_tau, B * WBC_NUM_JOINTS));
        WBC_HIP(dalloc(&h->d_best_grf, B * WBC_NUM_JOINTS));
    }
    h->modes_flags = 0;
    wbc::KernelArgs a = make_args(h, flags);
    a.modes = h->n_modes;
    const bool timed = (flags & WBC_TIMED) != 0;
    if (timed) WBC_HIP(hipEventRecord(h->ev0, h->stream));
    if (flags & WBC_SPLIT) {
        // split form: the update once per state (problem records to HBM), the general / stance
        // solve kernels once per hypothesis
        begin_update(h, a);
        wbc::KernelArgs au = a;
        au.batch = h->batch / h->n_modes;
        WBC_HIP(wbc_launch_update(&au, h->stream));
        WBC_HIP(launch_solves(h, a));
    } else if (h->mode_loop > 1 || mode_out) {
        // default, many states: one update per state and wave, then mode_loop hypotheses in turn; with
        // WBC_OBJECTIVE / WBC_BEST the loop's objective instance at every mode_loop, 1 included
        a.elim = 1;
        h->elim = false;
        a.mloop = h->mode_loop;
        std::memcpy(a.mode_order, h->mode_order, sizeof(a.mode_order));
        const int64_t S = h->batch / h->n_modes;
        a.nwaves = (int32_t)(((S + wbc::QMAP_SEG - 1) / wbc::QMAP_SEG) * (h->n_modes / h->mode_loop));
        if (mode_out) {
            a.obj = h->d_obj;
            WBC_HIP(wbc_launch_modes_obj(&a, h->stream));
            if (mode_out & WBC_BEST)
                WBC_HIP(wbc_launch_best_modes(a.obj, a.status, a.tau, a.grf, (int)S, h->n_modes, h->d_best, h->d_best_obj,
                                              h->d_best_tau, h->d_best_grf, h->stream));
        } else {
            WBC_HIP(wbc_launch_modes(&a, h->stream));
        }
    } else {
        // default: each hypothesis reduced and solved in its own 16-lane segment
        WBC_HIP(begin_step16(h, a, flags, h->d_qmap));
        WBC_HIP(kStepLaunchers[wbc::step_instance(false, false, false, a.stateful != 0)](&a, h->stream));
    }
    if (timed) {
        WBC_HIP(hipEventRecord(h->ev1, h->stream));
        h->timed = true;
    }
    h->updated = false;
    h->modes_flags = mode_out;
    return WBC_OK;
}

}  // extern "C"
namespace {
// One cycle's device work on the engine stream, from the packed pinned inputs (h_in) to the packed
// pinned outputs (h_out): one H2D copy, the wave map's copy when the masks differ, the step on the
// engine's own input and output blocks (the caller's bindings stay as they are), one D2H copy (x,
// last in the block, only without WBC_NO_X).
int32_t enqueue_cycle(wbc_engine* h, uint32_t flags) {
    h->zc_stale = false;  // this cycle's blocks replace whatever was pending
    const size_t B = (size_t)h->batch;
    const bool zc = h->m_in.pose != nullptr;
    if (!zc) {
        WBC_HIP(hipMemcpyAsync(h->d_inblk, h->h_in, wbc::input_block_bytes(B), hipMemcpyHostToDevice, h->stream));
        if (h->qmap_waves)
            WBC_HIP(hipMemcpyAsync(h->d_qmap, h->h_qmap, (size_t)h->qmap_waves * wbc::QMAP_SEG * sizeof(int32_t),
                                   hipMemcpyHostToDevice, h->stream));
    }
    // the step's input and output block: the engine's device buffers, or (zero-copy) the pinned
    // host buffers through their device addresses, in the same layouts
    const int32_t rc = zc ? step_on(h, flags, {h->m_in, h->m_out, h->m_qmap})
                          : step_on(h, flags, {wbc::const_view(h->own_in), h->own_out, h->d_qmap});
    // zero-copy: the pinned blocks hold this cycle's inputs (and map) whether or not the step ran, and
    // the host-side mask count / map already describe them, so the own buffers follow them at the next
    // sync_own in either case (on a failed step too, so d_contacts never lags n_stance_own / h_qmap)
    h->zc_stale = zc;
    if (rc != WBC_OK) return rc;
    if (!zc)
        WBC_HIP(hipMemcpyAsync(h->h_out, h->d_outblk, wbc::output_block_bytes(B, !(flags & WBC_NO_X)), hipMemcpyDeviceToHost,
                               h->stream));
    return WBC_OK;
}
// The resident cycle (WBC_RESIDENT, B <= 4): start the wave if it is not running (or runs with other
// flags, or may have ended by itself: no answer for 40 ms, against its 100 ms idle limit), post the
// cycle, wait for its answer (bounded), and leave the outputs in the pinned output block.
constexpr unsigned long long kResidentIdleTicks = 10000000ull;  // 100 ms of the 100 MHz constant clock
constexpr auto kResidentRestart = std::chrono::milliseconds(40);
constexpr auto kResidentAnswer = std::chrono::seconds(2);
int32_t resident_cycle(wbc_engine* h, uint32_t flags) {
    using clk = std::chrono::steady_clock;
    std::lock_guard<std::recursive_mutex> lk(g_res_mu);
    // wbc_cycle has written this cycle's pinned inputs and the host's mask count / map: the own
    // buffers follow them at the next sync_own whether or not the cycle below succeeds (as
    // enqueue_cycle does on every path), so d_contacts never lags n_stance_own / h_qmap
    h->zc_stale = true;
    const size_t B = (size_t)h->batch;
    WBC_HIP(stop_foreign_resident(h));
    if (h->res_on && (h->res_flags != flags || clk::now() - h->res_last > kResidentRestart)) WBC_HIP(resident_stop(h));
    const auto launch = [&](unsigned long long seq0) -> hipError_t {
        // work queued on the engine stream (a reset, copies) completes before the wave reads the history
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return e;
        // the step reads the engine's own device input block (the wave copies the pinned block into it
        // every cycle) and writes the pinned output block through its device address
        wbc::KernelArgs a = make_args(h, flags, wbc::const_view(h->own_in), h->m_out);
        a.elim = 1;  // as begin_step16: the default step
        a.qmap = nullptr;  // one wave: its robots in batch order
        a.nwaves = 1;
        __atomic_store_n(&h->res_box->exited, 0ull, __ATOMIC_RELEASE);
        e = wbc_launch_resident(&a, h->res_box_dev, h->m_in.pose, h->d_inblk, (int)wbc::input_block_words(B), seq0,
                                kResidentIdleTicks, h->res_stream);
        if (e != hipSuccess) return e;
        h->res_on = true;
        h->res_flags = flags;
        g_res_owner = h;
        return hipSuccess;
    };
    if (!h->res_on) {
        if (!h->res_box) WBC_HIP(resident_alloc(h));
        __atomic_store_n(&h->res_box->cmd, h->res_seq, __ATOMIC_RELEASE);
        WBC_HIP(launch(h->res_seq));
    }
    const unsigned long long seq = ++h->res_seq;
    __atomic_store_n(&h->res_box->cmd, seq, __ATOMIC_RELEASE);  // the inputs (pinned) are written before
    const auto deadline = clk::now() + kResidentAnswer;
    bool relaunched = false;
    while (__atomic_load_n(&h->res_box->done, __ATOMIC_ACQUIRE) != seq) {
        if (!relaunched && __atomic_load_n(&h->res_box->exited, __ATOMIC_ACQUIRE) == 1ull &&
            __atomic_load_n(&h->res_box->done, __ATOMIC_ACQUIRE) != seq) {
            // the wave reached its idle limit just before this cycle was posted (the host thread
            // stalled past kResidentRestart's margin): start a new one from the previous cycle; it
            // picks the posted cycle up
            h->res_on = false;
            if (g_res_owner == h) g_res_owner = nullptr;  // (launch sets it again on success)
            WBC_HIP(launch(seq - 1));
            relaunched = true;
        }
        if (clk::now() > deadline) {
            (void)resident_stop(h);
            return fail(WBC_ERR_HIP, "wbc_cycle: the resident step did not answer");
        }
        __builtin_ia32_pause();
    }
    h->res_last = clk::now();
    return WBC_OK;
}
}  // namespace
extern "C" {

int32_t wbc_cycle(wbc_engine* h, const double* base_pose, const double* nu, const double* qj, const double* ref,
                  const uint8_t* contacts, const uint8_t* switching, uint32_t flags, double* tau, double* grf, double* x,
                  int32_t* status, int32_t* iters) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    if (h->n_modes) return fail(WBC_ERR_STATE, "wbc_cycle: mode hypotheses are set");
    if (!base_pose || !nu || !qj || !ref || !contacts || !switching) return fail(WBC_ERR_ARG, "wbc_cycle: null input");
    if (const int32_t rc = refuse_tables(h, "wbc_cycle", flags, WBC_SPLIT | WBC_FUSED | WBC_RESIDENT, "plain cycle only")) return rc;
    if (const int32_t rc = refuse_mode_out_flags("wbc_cycle", flags)) return rc;
    if (const int32_t rc = refuse_duals_flag("wbc_cycle", flags)) return rc;
    if (const int32_t rc = refuse_force_duals_flag("wbc_cycle", flags)) return rc;
    if (const int32_t rc = refuse_task_duals_flag("wbc_cycle", flags)) return rc;
    WBC_HIP(hipSetDevice(h->device));
    const size_t B = (size_t)h->batch;
    if (!h->h_in) {
        WBC_HIP(hipHostMalloc(&h->h_in, 8 * wbc::input_block_words(B), hipHostMallocMapped));  // (whole words: the resident copy)
        WBC_HIP(hipHostMalloc(&h->h_out, wbc::output_block_bytes(B), hipHostMallocMapped));
#ifndef WBC_CYCLE_COPY  // (A/B builds only: the copy cycle at every batch size)
        // Small batches (the B = 1 drop-in) run zero-copy: the step reads the pinned input block and
        // writes the pinned output block through their device addresses (a few hundred bytes over
        // PCIe inside the kernel instead of an H2D and a D2H copy, each a separate queued operation).
        if (B <= kZeroCopyMaxBatch) {
            void *mi = nullptr, *mo = nullptr, *mq = nullptr;
            if (hipHostGetDevicePointer(&mi, h->h_in, 0) == hipSuccess &&
                hipHostGetDevicePointer(&mo, h->h_out, 0) == hipSuccess &&
                hipHostGetDevicePointer(&mq, h->h_qmap, 0) == hipSuccess) {
                h->m_in = wbc::input_view(static_cast<const void*>(mi), B);
                h->m_out = wbc::output_view(mo, B);
                h->m_qmap = static_cast<const int32_t*>(mq);
            }
            (void)hipGetLastError();
        }
#endif
    }
    // pack the host inputs in the device block's layout (pinned), one H2D copy
    const wbc::InputView hp = wbc::input_view(h->h_in, B);
    std::memcpy(hp.pose, base_pose, B * WBC_POSE_LEN * sizeof(double));
    std::memcpy(hp.nu, nu, B * WBC_NU_LEN * sizeof(double));
    std::memcpy(hp.qj, qj, B * WBC_NUM_JOINTS * sizeof(double));
    std::memcpy(hp.ref, ref, B * WBC_REF_LEN * sizeof(double));
    std::memcpy(hp.contacts, contacts, B);
    std::memcpy(hp.switching, switching, B);
    h->n_stance_own = count_stance(contacts, B);  // d_contacts holds these masks from here on
    h->qmap_waves = wbc::qmap_build(contacts, h->batch, h->h_qmap);  // uploaded by enqueue_cycle
    h->qmap_host = true;
    if (!x) flags |= WBC_NO_X;
    if ((flags & WBC_RESIDENT) && h->m_in.pose && B <= (size_t)wbc::QMAP_SEG && !(flags & (WBC_SPLIT | WBC_FUSED | WBC_DEBUG))) {
        const int32_t rc = resident_cycle(h, flags & ~WBC_RESIDENT);
        if (rc != WBC_OK) return rc;
    } else {
        if (h->res_on) WBC_HIP(resident_stop(h));
        const int32_t rc = enqueue_cycle(h, flags & ~WBC_RESIDENT);
        if (rc != WBC_OK) return rc;
        WBC_HIP(hipStreamSynchronize(h->stream));
    }
    const wbc::OutputView o = wbc::output_view(h->h_out, B);
    if (tau) std::memcpy(tau, o.tau, B * WBC_NUM_JOINTS * sizeof(double));
    if (grf) std::memcpy(grf, o.grf, B * WBC_NUM_JOINTS * sizeof(double));
    if (status) std::memcpy(status, o.status, B * sizeof(int32_t));
    if (iters) std::memcpy(iters, o.iters, B * sizeof(int32_t));
    if (x) std::memcpy(x, o.x, B * WBC_NV * sizeof(double));
    return WBC_OK;
}

int32_t wbc_synchronize(wbc_engine* h) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(hipSetDevice(h->device));
    WBC_HIP(hipStreamSynchronize(h->stream));
    return WBC_OK;
}

int32_t wbc_get_output(wbc_engine* h, double* tau, double* grf, double* x, int32_t* status, int32_t* iters) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    WBC_HIP(hipSetDevice(h->device));
    const size_t B = (size_t)h->batch;
    hipStream_t st = h->stream;
    if (tau) WBC_HIP(hipMemcpyAsync(tau, h->out.tau, B * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (grf) WBC_HIP(hipMemcpyAsync(grf, h->out.grf, B * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (x) WBC_HIP(hipMemcpyAsync(x, h->out.x, B * WBC_NV * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status) WBC_HIP(hipMemcpyAsync(status, h->out.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (iters) WBC_HIP(hipMemcpyAsync(iters, h->out.iters, B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    WBC_HIP(hipStreamSynchronize(st));
    return WBC_OK;
}

int32_t wbc_device_outputs(wbc_engine* h, double** d_tau, double** d_grf, double** d_x, int32_t** d_status,
                           int32_t** d_iters) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    WBC_HIP(sync_own(h));
    if (d_tau) *d_tau = h->out.tau;
    if (d_grf) *d_grf = h->out.grf;
    if (d_x) *d_x = h->out.x;
    if (d_status) *d_status = h->out.status;
    if (d_iters) *d_iters = h->out.iters;
    return WBC_OK;
}

int32_t wbc_get_debug(wbc_engine* h, double* out) {
    if (!h || !out) return fail(WBC_ERR_ARG, "null argument");
    WBC_HIP(hipSetDevice(h->device));
    WBC_HIP(hipMemcpyAsync(out, h->d_dbg, (size_t)h->batch * WBC_DBG_LEN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    WBC_HIP(hipStreamSynchronize(h->stream));
    return WBC_OK;
}

int32_t wbc_get_duals(wbc_engine* h, double* dual) {
    if (!h || !dual) return fail(WBC_ERR_ARG, "null argument");
    if (h->step_duals == wbc_engine::DUALS_48)
        return fail(WBC_ERR_STATE, "wbc_get_duals: the last wbc_step carried WBC_DUALS_FORCE (48 entries per robot: "
                                   "wbc_get_force_duals / wbc_device_force_duals)");
    if (h->step_duals != wbc_engine::DUALS_40) return fail(WBC_ERR_STATE, "wbc_get_duals: the last wbc_step did not carry WBC_DUALS");
    WBC_HIP(hipSetDevice(h->device));
    WBC_HIP(hipMemcpyAsync(dual, h->d_dual, (size_t)h->batch * WBC_DUAL_LEN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    WBC_HIP(hipStreamSynchronize(h->stream));
    return WBC_OK;
}

int32_t wbc_device_duals(wbc_engine* h, double** d_dual) {
    if (!h || !d_dual) return fail(WBC_ERR_ARG, "null argument");
    if (h->step_duals == wbc_engine::DUALS_48)
        return fail(WBC_ERR_STATE, "wbc_device_duals: the last wbc_step carried WBC_DUALS_FORCE (48 entries per robot: "
                                   "wbc_get_force_duals / wbc_device_force_duals)");
    if (h->step_duals != wbc_engine::DUALS_40) return fail(WBC_ERR_STATE, "wbc_device_duals: the last wbc_step did not carry WBC_DUALS");
    *d_dual = h->d_dual;
    return WBC_OK;
}

int32_t wbc_get_force_duals(wbc_engine* h, double* dual) {
    if (!h || !dual) return fail(WBC_ERR_ARG, "null argument");
    if (h->step_duals != wbc_engine::DUALS_48)
        return fail(WBC_ERR_STATE, "wbc_get_force_duals: the last wbc_step did not carry WBC_DUALS_FORCE");
    WBC_HIP(hipSetDevice(h->device));
    WBC_HIP(hipMemcpyAsync(dual, h->d_dual48, (size_t)h->batch * WBC_DUAL_FORCE_LEN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    WBC_HIP(hipStreamSynchronize(h->stream));
    return WBC_OK;
}

int32_t wbc_device_force_duals(wbc_engine* h, double** d_dual) {
    if (!h || !d_dual) return fail(WBC_ERR_ARG, "null argument");
    if (h->step_duals != wbc_engine::DUALS_48)
        return fail(WBC_ERR_STATE, "wbc_device_force_duals: the last wbc_step did not carry WBC_DUALS_FORCE");
    *d_dual = h->d_dual48;
    return WBC_OK;
}

int32_t wbc_get_objective(wbc_engine* h, double* obj) {
    if (!h || !obj) return fail(WBC_ERR_ARG, "null argument");
    if (!(h->modes_flags & WBC_OBJECTIVE)) return fail(WBC_ERR_STATE, "wbc_get_objective: the last wbc_step_modes did not carry WBC_OBJECTIVE");
    WBC_HIP(hipSetDevice(h->device));
    WBC_HIP(hipMemcpyAsync(obj, h->d_obj, (size_t)h->batch * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    WBC_HIP(hipStreamSynchronize(h->stream));
    return WBC_OK;
}

int32_t wbc_device_objective(wbc_engine* h, double** d_obj) {
    if (!h || !d_obj) return fail(WBC_ERR_ARG, "null argument");
    if (!(h->modes_flags & WBC_OBJECTIVE)) return fail(WBC_ERR_STATE, "wbc_device_objective: the last wbc_step_modes did not carry WBC_OBJECTIVE");
    *d_obj = h->d_obj;
    return WBC_OK;
}

int32_t wbc_get_best_modes(wbc_engine* h, int32_t* best, double* obj, double* tau, double* grf) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    if (!(h->modes_flags & WBC_BEST)) return fail(WBC_ERR_STATE, "wbc_get_best_modes: the last wbc_step_modes did not carry WBC_BEST");
    WBC_HIP(hipSetDevice(h->device));
    const size_t S = input_rows(h);
    hipStream_t st = h->stream;
    if (best) WBC_HIP(hipMemcpyAsync(best, h->d_best, S * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (obj) WBC_HIP(hipMemcpyAsync(obj, h->d_best_obj, S * sizeof(double), hipMemcpyDeviceToHost, st));
    if (tau) WBC_HIP(hipMemcpyAsync(tau, h->d_best_tau, S * WBC_NUM_JOINTS * sizeof(double), hipMemcpyDeviceToHost, st));
    if (grf) WBC_HIP(hipMemcpyAsync(grf, h->d_best_grf, S * WBC_NUM_JOINTS * sizeof(double), hipMemcpyDeviceToHost, st));
    WBC_HIP(hipStreamSynchronize(st));
    return WBC_OK;
}

int32_t wbc_device_best_modes(wbc_engine* h, int32_t** d_best, double** d_obj, double** d_tau, double** d_grf) {
    if (!h) return fail(WBC_ERR_ARG, "null handle");
    if (!(h->modes_flags & WBC_BEST)) return fail(WBC_ERR_STATE, "wbc_device_best_modes: the last wbc_step_modes did not carry WBC_BEST");
    if (d_best) *d_best = h->d_best;
    if (d_obj) *d_obj = h->d_best_obj;
    if (d_tau) *d_tau = h->d_best_tau;
    if (d_grf) *d_grf = h->d_best_grf;
    return WBC_OK;
}

int32_t wbc_modes_per_wave(wbc_engine* h, int32_t* m) {
    if (!h || !m) return fail(WBC_ERR_ARG, "null handle or output");
    *m = h->n_modes ? h->mode_loop : 0;
    return WBC_OK;
}

int32_t wbc_last_kernel_ms(wbc_engine* h, double* ms) {
    if (!h || !ms) return fail(WBC_ERR_ARG, "null argument");
    if (!h->timed) return fail(WBC_ERR_STATE, "no wbc_step ran with WBC_TIMED");
    float f = 0.f;
    WBC_HIP(hipEventSynchronize(h->ev1));
    WBC_HIP(hipEventElapsedTime(&f, h->ev0, h->ev1));
    *ms = (double)f;
    return WBC_OK;
}

const char* wbc_last_error(void) { return g_err.c_str(); }

// shared with the planner's C-ABI (wbc_planner.hip): one error string per thread for the library
void wbc_internal_set_error(const char* msg) { g_err = msg ? msg : ""; }

}  // extern "C"
