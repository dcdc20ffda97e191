// C-ABI for the rigid-body model, InverseKinematics and KinoDynMP (include/bunmpc.h), host side.
// Mirrors (behaviour, not code) ISL/include/ik/inverse_kinematics.hpp + ISL/src/ik/*.cpp and
// ISL/src/motion_planner/kino_dyn.cpp; all numerics run in ik_ddp.hip / biconvex_admm.hip.
#include "../../include/bunmpc.h"
#include "../../include/bunmpc_turn.h"
#include "ik_types.h"
#include "id_types.h"
#include "perturb_types.h"

namespace bunmpc {
int launch_wb_plan(const RobotModelDev *model, const bmpc_wb_plan_batch_t &d, const bmpc_terrain_t *t, double *normals, const bmpc_turn_t *turn,
                   hipStream_t st);                                                             // plan_gen.hip
int check_turn(const bmpc_turn_t *turn, bool wb);                                               // plan_gen.hip
int check_terrain(const bmpc_terrain_t *t);                                                     // plan_gen.hip
int model_on_device(const void *model, int *nframes, const RobotModelDev **dev);                // defined below, for cc_goals.hip
int check_cone_batch(const bmpc_batch_t *d, const bmpc_cone_t *c, const bmpc_contact_frame_t *fr);   // bunmpc_capi.hip
}

#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <iostream>
#include <map>
#include <mutex>
#include <utility>
#include <string>
#include <vector>

namespace {

int ik_fail(int code, const std::string &msg) { return bunmpc::set_error(code, msg); }

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return ik_fail(BMPC_DEVICE_ERROR, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Dev {
    void *p = nullptr; size_t bytes = 0;
    ~Dev() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    double *d() const { return static_cast<double *>(p); }
};

}  // namespace

struct bmpc_model {
    bunmpc::RobotModelDev host;
    Dev dev;            // device copy, uploaded lazily
    bool uploaded = false;
    std::mutex upload_lock;     // batches of several host threads may share one model (bunmpc_amd/pipeline.py)
    int upload() {
        std::lock_guard<std::mutex> hold(upload_lock);
        if (uploaded) return BMPC_OK;
        HIP_TRY(dev.ensure(sizeof(host)));
        HIP_TRY(hipMemcpy(dev.p, &host, sizeof(host), hipMemcpyHostToDevice));
        uploaded = true;
        return BMPC_OK;
    }
    const bunmpc::RobotModelDev *dptr() const { return static_cast<const bunmpc::RobotModelDev *>(dev.p); }
};

// one residual cost of a node, as the reference's CostModelSum holds it (name -> item)
struct IkItem { int kind; double wt; int frame; std::vector<double> ref; };  // kind: 0 frame 1 com 2 mom 3 state 4 ctrl

struct bmpc_ik {
    const bmpc_model *model;
    int n_col;
    std::vector<double> dt;
    std::vector<std::map<std::string, IkItem>> nodes;   // n_col + 1 (last = terminal)
    // results of the last optimize
    std::vector<double> xs, us;
    int iters = 0, status = 0;
    double cost = 0, stop = 0;
    bool solved = false;
    Dev din, dws, dactive;
};

struct bmpc_kinodyn {
    const bmpc_model *model;
    double m; int n_eff, dyn_col, ik_col;
    bmpc_biconvex_t *dyn; bmpc_ik *ik;
    double wt_com = 0, wt_mom = 0;
    bool profile = false;
    double solve_times[3] = {0, 0, 0};
    Dev dtmp;
};

namespace {

int add_item(bmpc_ik *h, int t, const char *name, IkItem item) {
    if (t < 0 || t > h->n_col) return ik_fail(BMPC_BAD_ARG, "time step out of range");
    auto &m = h->nodes[t];
    const std::string key = name ? name : "";
    if (m.count(key)) {   // crocoddyl CostModelSum::addCost refuses duplicates with this message
        std::cout << "Warning: we couldn't add the " << key << " cost item, it already existed." << std::endl;
        return BMPC_OK;
    }
    m[key] = std::move(item);
    return BMPC_OK;
}

// pack the accumulated costs into the kernel's per-node task blocks
int pack_tasks(const bmpc_ik *h, std::vector<double> &tasks) {
    using namespace bunmpc;
    const int nn = h->n_col + 1;
    tasks.assign((size_t)nn * kNodeTaskDoubles, 0.0);
    for (int t = 0; t < nn; ++t) {
        double *tk = tasks.data() + (size_t)t * kNodeTaskDoubles;
        int slots = 0, ncom = 0, nmom = 0, nst = 0, nct = 0;
        for (const auto &kv : h->nodes[t]) {
            const IkItem &it = kv.second;
            switch (it.kind) {
            case 0:
                if (slots == kFrameSlots) return ik_fail(BMPC_BAD_ARG, "more than 4 frame-translation costs on one node");
                tk[5 * slots] = it.wt; tk[5 * slots + 1] = it.frame;
                for (int c = 0; c < 3; ++c) tk[5 * slots + 2 + c] = it.ref[c];
                ++slots; break;
            case 1:
                if (ncom++) return ik_fail(BMPC_BAD_ARG, "more than one CoM cost on one node");
                tk[5 * kFrameSlots] = it.wt;
                for (int c = 0; c < 3; ++c) tk[5 * kFrameSlots + 1 + c] = it.ref[c];
                break;
            case 2:
                if (nmom++) return ik_fail(BMPC_BAD_ARG, "more than one momentum cost on one node");
                tk[5 * kFrameSlots + 4] = it.wt;
                for (int c = 0; c < 6; ++c) tk[5 * kFrameSlots + 5 + c] = it.ref[c];
                break;
            case 3:
                if (nst++) return ik_fail(BMPC_BAD_ARG, "more than one state regularisation on one node");
                tk[5 * kFrameSlots + 11] = it.wt; break;
            case 4:
                if (nct++) return ik_fail(BMPC_BAD_ARG, "more than one control regularisation on one node");
                tk[5 * kFrameSlots + 12] = it.wt; break;
            }
        }
    }
    return BMPC_OK;
}

constexpr int kMaxIkCol = 255;
// The checks on a batch descriptor and the kernel arguments made from it (more_arrays / more_error: the caller's further arrays are there /
// what is wrong with its further arguments, or null -- reported in their place among the checks).  Uploads the model.  B == 0 passes the
// checks and fills nothing: the caller returns before any launch.
int args_from_batch(const bmpc_ik_batch_t *d, int maxiter, bool more_arrays, const char *more_error, bunmpc::IkBatchArgs *a) {
    using namespace bunmpc;
    if (!d || !d->model) return ik_fail(BMPC_BAD_ARG, "null batch descriptor / model");
    if (d->B < 0 || d->n_col < 1 || maxiter < 1) return ik_fail(BMPC_BAD_ARG, "bad sizes");
    if (d->n_col > kMaxIkCol) return ik_fail(BMPC_BAD_ARG, "n_col > 255 is not supported");
    if (!d->x0 || !d->dt || !d->tasks || !d->state_w || !d->x_reg || !d->ctrl_w || !d->ws || !d->active || !more_arrays)
        return ik_fail(BMPC_BAD_ARG, "missing array");
    if (more_error) return ik_fail(BMPC_BAD_ARG, more_error);
    if (d->B == 0) return BMPC_OK;
    auto *model = const_cast<bmpc_model *>(d->model);
    if (int rc = model->upload()) return rc;
    *a = IkBatchArgs{};      // (every field below unset: zero, the list pointers null)
    a->B = d->B; a->T = d->n_col; a->maxiter = maxiter; a->model = model->dptr(); a->bwd_waves = 1; a->n_launch = d->B;
    a->x0 = d->x0; a->dt = d->dt; a->tasks = d->tasks; a->state_w = d->state_w; a->x_reg = d->x_reg; a->ctrl_w = d->ctrl_w; a->ws = d->ws; a->active = d->active;
    a->s_state_w = d->s_state_w; a->s_ctrl_w = d->s_ctrl_w; a->s_x_reg = d->s_x_reg ? d->s_x_reg : kNX; a->sn_state_w = d->sn_state_w; a->sn_x_reg = d->sn_x_reg; a->sn_ctrl_w = d->sn_ctrl_w;
    if (d->active_list) {      // the pieces of that scratch (ik_types.h::active_list_ints)
        a->list = d->active_list; a->count = a->list + 2 * (long)a->B; a->wcount = a->count + 2; a->wide = a->wcount + 2;
        a->err = a->wide + 2 * kWideMax; a->near = a->err + 2; a->xmeta = a->near + 2; a->xlist = a->xmeta + 4;
    }
    return BMPC_OK;
}

// The scheduling knobs (ik_plan.h): ONE store of the process-wide defaults, which the bmpc_ik_set_* entry points update; a batch may
// carry its own thresholds in bmpc_ik_batch_t.sched.  A DDP loop takes one copy when it starts (resolve_knobs) and reads no global
// afterwards: a setter called meanwhile (another host thread) changes the next loop, never one that is running.
std::mutex g_knobs_lock; bunmpc::IkKnobs g_knobs;
template <class T> T set_knob(T bunmpc::IkKnobs::*field, T value) {      // returns the old setting
    std::lock_guard<std::mutex> hold(g_knobs_lock);
    return std::exchange(g_knobs.*field, value);
}
// the knobs of one loop: a field of bmpc_ik_batch_t.sched (null: none) of 0 = the process default, < 0 = never, n > 0 = n
bunmpc::IkKnobs resolve_knobs(const bmpc_ik_sched_t *sched) {
    bunmpc::IkKnobs k;
    { std::lock_guard<std::mutex> hold(g_knobs_lock); k = g_knobs; }
    if (!sched) return k;
    auto pick = [](int field, int &knob) { if (field != 0) knob = field < 0 ? 0 : field; };
    pick(sched->spec_below, k.spec_below); pick(sched->all_steps_below, k.all_steps); pick(sched->gains_wave_below, k.gains_wave_below);
    pick(sched->express_cap, k.express_cap); k.debug_inject = sched->debug_inject;
    return k;
}

// Two host-mapped words and events per (device, stream), through which the kernels' active counter reaches the DDP loop.
// Keyed by the stream, not by the host thread: a stream's publishes are ordered among themselves, so a late publish of one
// batch can never overwrite the counter of another batch running on a different stream; and the few entries (one per stream
// ever used) live as long as the library, whatever threads come and go (bunmpc_amd/pipeline.py starts workers per call).
struct ActiveWord {
    int *host[2] = {nullptr, nullptr}, *dev[2] = {nullptr, nullptr};      // eight ints each: active, index-check code, list length, express taken, iterations (fused-direct)
    hipStream_t side = nullptr;                 // the express lane's stream (ik_fused_kernel beside the batch's own kernels)
    hipEvent_t x_go = nullptr, x_done = nullptr;
    // evs[0]: spinning waits, evs[1]: blocking waits (hipEventBlockingSync: the waiting host thread sleeps until the interrupt --
    // with eight ranks of up to three pool threads each on a 16-core cgroup, spinning waits would fight the other ranks' loops)
    hipEvent_t evs[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    std::mutex in_use;      // one DDP loop at a time per stream (two host threads driving one stream would interleave anyway)
    int ensure() {
        if (host[0]) return BMPC_OK;
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&host[k]), 8 * sizeof(int), hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev[k]), host[k], 0));
            HIP_TRY(hipEventCreateWithFlags(&evs[0][k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&evs[1][k], hipEventDisableTiming | hipEventBlockingSync));
        }
        // A stream of the HIGHEST priority: the HIP runtime multiplexes streams of one priority onto a few hardware queues, and
        // sharing one with the caller's stream would put the lane's persistent kernel (milliseconds) IN FRONT of the batch's own
        // kernels instead of beside them (seen in bench.py, whose process holds a dozen streams: 19.8 ms per batch solve instead
        // of 15.1); queues are per priority level, and the lane's workgroups should be placed first anyway.
        int pr_least = 0, pr_greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest) != hipSuccess ||
            hipStreamCreateWithPriority(&side, hipStreamNonBlocking, pr_greatest) != hipSuccess) {
            (void)hipGetLastError();        // no priorities on this runtime: an ordinary stream still gives correct results
            HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        }
        HIP_TRY(hipEventCreateWithFlags(&x_go, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&x_done, hipEventDisableTiming | hipEventBlockingSync));
        return BMPC_OK;
    }
};
std::mutex g_active_words_lock;
std::map<std::pair<int, hipStream_t>, ActiveWord *> &active_words() {
    static auto *m = new std::map<std::pair<int, hipStream_t>, ActiveWord *>;   // never destroyed: the HIP runtime may be gone at exit
    return *m;
}
ActiveWord *active_word_for(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> hold(g_active_words_lock);
    ActiveWord *&w = active_words()[{dev, st}];
    if (!w) w = new ActiveWord;
    return w;
}

// bmpc_ik_set_profile(1): hipEvents around every kernel of the DDP loop; the summed times per kernel of the last batch
// solve are read back with bmpc_ik_last_profile.  For measurement passes only (the events cost launch slots).
bool g_profile = false;
double g_last_profile[5] = {0, 0, 0, 0, 0};     // ms: state, calcdiff, backward, forward, everything else in the loop
std::mutex g_profile_lock;

int index_check_failed(int code) {
    static const char *what[] = {"", "active-list entry out of range", "active-list length out of range", "active-list append past its end",
                                 "wide-list entry out of range", "the fused kernel's tick watchdog fired"};
    return ik_fail(BMPC_DEVICE_ERROR, std::string("IK-DDP index check failed: ") + what[code > 0 && code < 6 ? code : 0] +
                   " (code " + std::to_string(code) + "); results of this batch are invalid");
}

// the DDP iteration loop (SolverDDP::solve): four launches per iteration, stop when every problem is done
int run_ddp(bunmpc::IkBatchArgs a, hipStream_t st, int *iters_run, const bunmpc::IkKnobs knobs) {
    using namespace bunmpc;
    a.near_stop = knobs.express_near;
    const IkBatchPlan batch = plan_batch(a.B, a.T, a.maxiter, a.list != nullptr, knobs);
    const bool prof = g_profile;
    std::vector<hipEvent_t> pev;
    auto stamp = [&]() -> int {
        if (!prof) return BMPC_OK;
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(e, st));
        pev.push_back(e);
        return BMPC_OK;
    };
    ActiveWord *wp = active_word_for(st);
    if (!wp) return ik_fail(BMPC_DEVICE_ERROR, "hipGetDevice failed");
    ActiveWord &w = *wp;
    std::lock_guard<std::mutex> hold(w.in_use);
    if (int rc = w.ensure()) return rc;
    // Every return below (the error ones too) leaves with the side stream idle: work queued there reads xmeta / xlist, which the
    // next batch on this stream rewrites as soon as w.in_use is free.
    struct SideDrain {
        hipStream_t side; bool armed = false;
        ~SideDrain() { if (armed) (void)hipStreamSynchronize(side); }
    } side_drain{w.side};
    hipEvent_t *ev = w.evs[knobs.blocking_waits ? 1 : 0];
    HIP_TRY(ik_launch_init(a, st));
    if (knobs.debug_inject == 1 && a.list) HIP_TRY(hipMemsetAsync(a.list, 0x7f, sizeof(int), st));      // tests: an entry far out of range
    // A handful of problems (the single-problem handles of the drop-in classes above all): every one of them gets a CU of its own
    // from the first iteration on -- the whole DDP in ONE launch of the fused kernel, no host look in between.
    if (batch.fused_direct) {
        HIP_TRY(ik_launch_fused(a, batch.fused_grid, false, st));
        HIP_TRY(ik_launch_publish_active(a, 0, w.dev[0], st, a.B));
        HIP_TRY(hipEventRecord(ev[0], st));
        HIP_TRY(hipEventSynchronize(ev[0]));
        const volatile int *hw = static_cast<volatile int *>(w.host[0]);
        if (iters_run) *iters_run = hw[4];        // the most iterations any problem of the batch ran (one launch: there is no host loop to count)
        if (prof) {                               // no per-kernel split exists on this path: the profile of an earlier batch must not stand
            std::lock_guard<std::mutex> hold_p(g_profile_lock);
            for (int k = 0; k < 5; ++k) g_last_profile[k] = 0.0;
        }
        if (hw[1]) return index_check_failed(hw[1]);
        if (hw[0] != 0) return ik_fail(BMPC_DEVICE_ERROR, "the fused kernel left problems unsolved");
        return BMPC_OK;
    }
    // The host looks at the active counter after every iteration while many problems are iterating (iterations are long
    // there and the line-search mapping depends on it); once few are left it enqueues kTailChunk iterations per look --
    // kernels of a finished problem return at once, so an iteration too many costs a few microseconds.  And it looks
    // one chunk late: the next chunk is enqueued BEFORE the host waits for the counter of the one before, so the queue
    // never drains while the host turns around (at the end one chunk of no-op kernels runs out on its own).
    // The express lane (ik_select_kernel / ik_fused_kernel): in front of the early iterations a one-workgroup kernel looks at the
    // batch and -- once, when it finds it converging fast with a thin tail of laggards -- moves the laggards-to-be off the active
    // list; the fused kernel enqueued behind it on the side stream runs them to the end at their own pace, on CUs of their own,
    // while the batch goes on without them.  The decision is the device's (the host would learn of it an iteration late); the
    // host enqueues the pair until a look tells it that the lane has taken its problems, or the window has passed.
    bool express_taken = false;
    int express_enqueued = 0, active = a.B, it = 0, it_end[2] = {0, 0};
    auto enqueue_chunk = [&](int slot) -> int {
        const IkIterPlan plan = plan_iteration(active, a.B, a.T, a.list != nullptr, a.wide != nullptr, knobs);
        a.fwd_spec = plan.fwd; a.bwd_waves = plan.bwd_waves; a.n_launch = plan.n_launch;      // (n_launch: the host's latest look at the counter)
        for (int k = 0; k < plan.chunk && it < a.maxiter; ++k, ++it) {
            a.iter = it;
            if (batch.express_cap > 0 && !express_taken && it >= kExpressFirstIter && it <= kExpressLastIter) {
                HIP_TRY(ik_launch_select(a, batch.express_cap, knobs.debug_inject == 2, st));
                HIP_TRY(hipEventRecord(w.x_go, st));
                HIP_TRY(hipStreamWaitEvent(w.side, w.x_go, 0));
                side_drain.armed = true;
                HIP_TRY(ik_launch_fused(a, batch.express_grid, true, w.side));
                HIP_TRY(hipEventRecord(w.x_done, w.side));
                ++express_enqueued;
            }
            for (const IkLaunch *l : {&plan.state, &plan.calcdiff, &plan.backward, &plan.forward}) {
                if (int rc = stamp()) return rc;
                HIP_TRY(ik_launch(*l, a, st));
            }
            if (int rc = stamp()) return rc;
        }
        HIP_TRY(ik_launch_publish_active(a, it, w.dev[slot], st));
        HIP_TRY(hipEventRecord(ev[slot], st));
        it_end[slot] = it;
        return BMPC_OK;
    };
    int slot = 0, it_done = 0, index_err = 0, all_active = a.B;
    if (a.maxiter > 0 && active > 0) {
        if (int rc = enqueue_chunk(slot)) return rc;
        for (;;) {
            const bool more = it < a.maxiter;
            if (more) { if (int rc = enqueue_chunk(slot ^ 1)) return rc; }
            HIP_TRY(hipEventSynchronize(ev[slot]));
            const volatile int *hw = static_cast<volatile int *>(w.host[slot]);
            all_active = hw[0];
            index_err = hw[1];
            active = hw[2] >= 0 ? hw[2] : hw[0];     // what the batch's own kernels still run over (the express lane's problems are not on the list)
            express_taken = express_taken || hw[3] != 0;
            it_done = it_end[slot];
            if (index_err) active = 0;       // an index of the list code was out of range: stop, report below
            if (active <= 0 || !more) {
                // the chunk enqueued ahead (no-op kernels and one more publish into the other word) must have drained before
                // this stream's words can serve another batch
                if (more) HIP_TRY(hipEventSynchronize(ev[slot ^ 1]));
                break;
            }
            slot ^= 1;
        }
    }
    if (iters_run) *iters_run = it_done;     // iterations up to the look that found every problem done (not the chunk enqueued ahead)
    if (express_enqueued > 0) {
        // the lane's kernel ends when its last problem has: the caller's stream is ordered behind it, and one more look tells
        // whether it left an error code (or a problem) behind
        HIP_TRY(hipStreamWaitEvent(st, w.x_done, 0));
        HIP_TRY(ik_launch_publish_active(a, it, w.dev[0], st));
        HIP_TRY(hipEventRecord(ev[0], st));
        HIP_TRY(hipEventSynchronize(ev[0]));
        const volatile int *hw = static_cast<volatile int *>(w.host[0]);
        all_active = hw[0];
        if (!index_err) index_err = hw[1];
        side_drain.armed = false;      // the look above came behind x_done: the side stream has drained
    }
    if (index_err) return index_check_failed(index_err);
    if (prof && !pev.empty()) {
        HIP_TRY(hipEventSynchronize(pev.back()));
        double acc[5] = {0, 0, 0, 0, 0};
        for (size_t i = 0; i + 1 < pev.size(); ++i) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, pev[i], pev[i + 1]));
            acc[i % 5 < 4 ? i % 5 : 4] += ms;     // five stamps per iteration: the fifth interval is the gap to the next iteration
        }
        for (hipEvent_t e : pev) (void)hipEventDestroy(e);
        std::lock_guard<std::mutex> hold(g_profile_lock);
        for (int k = 0; k < 5; ++k) g_last_profile[k] = acc[k];
    }
    return BMPC_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------ model ----
bmpc_model_t *bmpc_model_create(int nj, const int *parent, const double *R, const double *p, const double *axis,
                                const double *mass, const double *com, const double *inertia, int nframes,
                                const int *frame_body, const double *frame_p) {
    using namespace bunmpc;
    if (nj != kMaxJoints) { ik_fail(BMPC_BAD_ARG, "the kernels are built for 12 revolute joints after the free-flyer"); return nullptr; }
    if (nframes < 0 || nframes > kMaxFrames) { ik_fail(BMPC_BAD_ARG, "too many frames"); return nullptr; }
    auto *m = new bmpc_model;
    RobotModelDev &h = m->host;
    std::memset(&h, 0, sizeof(h));
    h.nj = nj; h.nframes = nframes;
    for (int i = 0; i < nj; ++i) {
        h.parent[i] = parent[i];
        if (parent[i] >= i || parent[i] < -1) { delete m; ik_fail(BMPC_BAD_ARG, "joints must be listed parents first"); return nullptr; }
        std::memcpy(h.R[i], R + 9 * i, sizeof(double) * 9);
        h.R_identity[i] = 1;
        for (int c = 0; c < 9; ++c) if (R[9 * i + c] != (c % 4 == 0 ? 1.0 : 0.0)) h.R_identity[i] = 0;
        std::memcpy(h.p[i], p + 3 * i, sizeof(double) * 3);
        std::memcpy(h.axis[i], axis + 3 * i, sizeof(double) * 3);
    }
    // serial chains only: every joint has at most one child, chain_end = last descendant
    for (int i = 0; i < nj; ++i) {
        int nchild = 0;
        for (int j = 0; j < nj; ++j) nchild += parent[j] == i;
        if (nchild > 1) { delete m; ik_fail(BMPC_BAD_ARG, "branching below the base is not supported"); return nullptr; }
    }
    for (int i = nj - 1; i >= 0; --i) {
        h.chain_end[i] = i;
        for (int j = i + 1; j < nj; ++j) if (parent[j] == i) h.chain_end[i] = h.chain_end[j];
    }
    for (int i = 0; i < nj; ++i)   // the subtree of joint i must be the contiguous index range i..chain_end[i]
        for (int j = i + 1; j <= h.chain_end[i]; ++j)
            if (parent[j] != j - 1) { delete m; ik_fail(BMPC_BAD_ARG, "chains must be numbered contiguously"); return nullptr; }
    // the register-resident kinematics (rbd_quad.h) assume 4 legs of 3 joints: 3L hangs off the base, 3L+j off 3L+j-1
    for (int i = 0; i < nj; ++i)
        if (parent[i] != (i % 3 == 0 ? -1 : i - 1)) { delete m; ik_fail(BMPC_BAD_ARG, "expected 4 legs x 3 joints, numbered leg by leg"); return nullptr; }
    h.total_mass = 0;
    for (int b = 0; b <= nj; ++b) {
        h.mass[b] = mass[b]; h.total_mass += mass[b];
        std::memcpy(h.com[b], com + 3 * b, sizeof(double) * 3);
        const double *I = inertia + 9 * b;
        h.inertia[b][0] = I[0]; h.inertia[b][1] = I[1]; h.inertia[b][2] = I[2];
        h.inertia[b][3] = I[4]; h.inertia[b][4] = I[5]; h.inertia[b][5] = I[8];
        double *r = h.rec[b];
        for (int c = 0; c < 3; ++c) { r[c] = b > 0 ? h.p[b - 1][c] : 0.0; r[3 + c] = b > 0 ? h.axis[b - 1][c] : 0.0; r[7 + c] = h.com[b][c]; }
        r[6] = h.mass[b];
        for (int c = 0; c < 6; ++c) r[10 + c] = h.inertia[b][c];
    }
    for (int f = 0; f < nframes; ++f) {
        if (frame_body[f] < 0 || frame_body[f] > nj) { delete m; ik_fail(BMPC_BAD_ARG, "frame body out of range"); return nullptr; }
        h.frame_body[f] = frame_body[f];
        std::memcpy(h.frame_p[f], frame_p + 3 * f, sizeof(double) * 3);
    }
    return m;
}
void bmpc_model_destroy(bmpc_model_t *m) { delete m; }

// t == nullptr with terrain == false: flat ground (bmpc_wb_plan_batch_device); turn == nullptr: w_des = 0 (the calls of bunmpc.h)
static int wb_plan_batch(const bmpc_wb_plan_batch_t *d, bool terrain, const bmpc_terrain_t *t, double *normals, const bmpc_turn_t *turn,
                         void *hip_stream) {
    if (!d || !d->model) return ik_fail(BMPC_BAD_ARG, "null descriptor or model");
    if (d->B < 0 || d->n_col < 1 || d->ik_col < 1 || d->ik_col > d->n_col) return ik_fail(BMPC_BAD_ARG, "bad sizes");
    if (!d->gait || !d->x || !d->t0 || !d->v_des_body) return ik_fail(BMPC_BAD_ARG, "missing input array");
    if (!d->com || !d->feet0 || !d->v_des || !d->w_des || !d->hip_off || !d->amom || !d->x_init || !d->cnt_plan || !d->swing_time ||
        !d->dt || !d->X_nom || !d->X_ter || !d->ik_tasks)
        return ik_fail(BMPC_BAD_ARG, "missing output array");
    for (int j = 0; j < 4; ++j)
        if (d->foot_frame[j] < 0 || d->foot_frame[j] >= d->model->host.nframes) return ik_fail(BMPC_BAD_ARG, "foot frame out of range");
    if (terrain)
        if (int rc = bunmpc::check_terrain(t)) return rc;
    if (turn)
        if (int rc = bunmpc::check_turn(turn, true)) return rc;
    if (d->B == 0) return BMPC_OK;
    bmpc_model *m = const_cast<bmpc_model *>(d->model);
    if (int rc = m->upload()) return rc;
    return bunmpc::launch_wb_plan(m->dptr(), *d, t, normals, turn, static_cast<hipStream_t>(hip_stream));
}
int bmpc_wb_plan_batch_device(const bmpc_wb_plan_batch_t *d, void *hip_stream) { return wb_plan_batch(d, false, nullptr, nullptr, nullptr, hip_stream); }
int bmpc_wb_plan_batch_terrain_device(const bmpc_wb_plan_batch_t *d, const bmpc_terrain_t *t, double *normals, void *hip_stream) {
    return wb_plan_batch(d, true, t, normals, nullptr, hip_stream);
}
// include/bunmpc_turn.h; a NULL terrain is flat ground here, and its normals are then not looked at
int bmpc_wb_plan_batch_turn_device(const void *wb_plan, const void *terrain, double *normals, const bmpc_turn_t *turn, void *hip_stream) {
    return wb_plan_batch(static_cast<const bmpc_wb_plan_batch_t *>(wb_plan), terrain != nullptr, static_cast<const bmpc_terrain_t *>(terrain),
                         terrain ? normals : nullptr, turn, hip_stream);
}
int bmpc_id_batch_device(const bmpc_id_batch_t *d, void *hip_stream) {
    using namespace bunmpc;
    if (!d || !d->model) return ik_fail(BMPC_BAD_ARG, "null descriptor or model");
    if (d->n < 0) return ik_fail(BMPC_BAD_ARG, "n < 0");
    if (d->n > 0 && (!d->q_des || !d->v_des || !d->a_des || !d->f)) return ik_fail(BMPC_BAD_ARG, "missing desired-state / force array");
    if ((d->q == nullptr) != (d->v == nullptr)) return ik_fail(BMPC_BAD_ARG, "q and v must be given together");
    if (d->n > 0 && !d->tau_ff && !d->tau_fb && !d->action && !d->state) return ik_fail(BMPC_BAD_ARG, "no output array");
    for (int i = 0; i < 12; ++i)
        if (d->action && d->kp[i] == 0.0) return ik_fail(BMPC_BAD_ARG, "kp = 0 with the pd_target action asked for");
    IdLaunch a;
    a.d = *d;
    if (!d->q) { a.d.q = d->q_des; a.d.v = d->v_des; a.d.s_q = d->s_q_des; a.d.s_v = d->s_v_des; }
    const RobotModelDev &h = d->model->host;
    for (int L = 0; L < 4; ++L) { a.leg_foot[L] = -1; a.leg_foot_k[L] = 0; a.leg_foot_p[L][0] = a.leg_foot_p[L][1] = a.leg_foot_p[L][2] = 0.0; }
    for (int j = 0; j < 4; ++j) {
        const int f = d->foot_frame[j];
        if (f < 0 || f >= h.nframes) return ik_fail(BMPC_BAD_ARG, "foot frame out of range");
        const int body = h.frame_body[f];
        if (body < 1) return ik_fail(BMPC_BAD_ARG, "an end effector on the base: each must hang off a leg");
        const int L = (body - 1) / 3;
        if (a.leg_foot[L] >= 0) return ik_fail(BMPC_BAD_ARG, "two end effectors on one leg");
        a.leg_foot[L] = j; a.leg_foot_k[L] = (body - 1) % 3;
        for (int c = 0; c < 3; ++c) a.leg_foot_p[L][c] = h.frame_p[f][c];
    }
    if (d->n == 0) return BMPC_OK;
    bmpc_model *m = const_cast<bmpc_model *>(d->model);
    if (int rc = m->upload()) return rc;
    a.model = m->dptr();
    return launch_id_batch(a, static_cast<hipStream_t>(hip_stream));
}

int bmpc_perturb_batch_device(const bmpc_perturb_batch_t *d, void *hip_stream) {
    using namespace bunmpc;
    if (!d || !d->model) return ik_fail(BMPC_BAD_ARG, "null descriptor or model");
    if (d->B < 0 || d->K < 1) return ik_fail(BMPC_BAD_ARG, "B < 0 or K < 1");
    for (int j = 0; j < 4; ++j)
        if (d->foot_frame[j] < 0 || d->foot_frame[j] >= d->model->host.nframes) return ik_fail(BMPC_BAD_ARG, "foot frame out of range");
    for (int g = 0; g < 4; ++g)
        if (!(d->sigma[g] >= 0.0)) return ik_fail(BMPC_BAD_ARG, "negative or NaN sigma");
    if (d->B == 0) return BMPC_OK;
    if (!d->q || !d->v || !d->contact || !d->z) return ik_fail(BMPC_BAD_ARG, "missing input array");
    if (!d->q_out || !d->v_out || !d->chosen) return ik_fail(BMPC_BAD_ARG, "missing output array");
    bmpc_model *m = const_cast<bmpc_model *>(d->model);
    if (int rc = m->upload()) return rc;
    PerturbLaunch a;
    a.d = *d;
    a.model = m->dptr();
    return launch_perturb(a, static_cast<hipStream_t>(hip_stream));
}

int bmpc_ik_set_profile(int on) { const int old = g_profile; g_profile = on != 0; return old; }
void bmpc_ik_last_profile(double *ms5) {
    std::lock_guard<std::mutex> hold(g_profile_lock);
    for (int k = 0; k < 5; ++k) ms5[k] = g_last_profile[k];
}
// self test of the state operators (host arrays): x0, x1 [n][37], dx [n][36] -> diff(x0, x1) and x0 (+) dx by the quaternion
// versions the forward pass uses (dq, iq) and by the rotation-matrix versions (dr, ir)
int bmpc_ik_selftest_state_ops(const double *x0, const double *x1, const double *dx, int n, double *dq, double *dr, double *iq, double *ir) {
    using namespace bunmpc;
    if (!x0 || !x1 || !dx || !dq || !dr || !iq || !ir || n < 1) return ik_fail(BMPC_BAD_ARG, "bad selftest arguments");
    Dev in, out;
    const size_t nx = (size_t)n * kNX, nd = (size_t)n * kNDX;
    HIP_TRY(in.ensure(sizeof(double) * (2 * nx + nd)));
    HIP_TRY(out.ensure(sizeof(double) * (2 * nx + 2 * nd)));
    HIP_TRY(hipMemcpy(in.d(), x0, sizeof(double) * nx, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.d() + nx, x1, sizeof(double) * nx, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.d() + 2 * nx, dx, sizeof(double) * nd, hipMemcpyHostToDevice));
    HIP_TRY(ik_launch_state_ops_selftest(in.d(), in.d() + nx, in.d() + 2 * nx, n, out.d(), out.d() + nd, out.d() + 2 * nd, out.d() + 2 * nd + nx, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dq, out.d(), sizeof(double) * nd, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dr, out.d() + nd, sizeof(double) * nd, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(iq, out.d() + 2 * nd, sizeof(double) * nx, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ir, out.d() + 2 * nd + nx, sizeof(double) * nx, hipMemcpyDeviceToHost));
    return BMPC_OK;
}
// the process-wide defaults of the scheduling knobs (ik_plan.h); each returns the old setting
int bmpc_ik_set_speculative_below(int n_active) { return set_knob(&bunmpc::IkKnobs::spec_below, n_active); }
int bmpc_ik_set_spec_one_wave_above(int n_active) { return set_knob(&bunmpc::IkKnobs::spec_one_wave_above, n_active); }
int bmpc_ik_set_all_steps(int n_active) { return set_knob(&bunmpc::IkKnobs::all_steps, n_active); }
int bmpc_ik_set_gains_wave_below(int n_active) { return set_knob(&bunmpc::IkKnobs::gains_wave_below, n_active); }
int bmpc_ik_set_calcdiff_one_wave_above(int n_pairs) { return set_knob(&bunmpc::IkKnobs::calcdiff_one_wave_above, n_pairs); }
int bmpc_ik_set_express_capacity(int n) { return set_knob(&bunmpc::IkKnobs::express_cap, n); }
int bmpc_ik_set_fused_direct_max(int n) { return set_knob(&bunmpc::IkKnobs::fused_direct, n); }
int bmpc_ik_set_blocking_waits(int on) { return set_knob(&bunmpc::IkKnobs::blocking_waits, int(on != 0)); }
double bmpc_ik_set_express_near(double stop) { return set_knob(&bunmpc::IkKnobs::express_near, stop); }
void bmpc_ik_kernel_occupancy(int *out8) { bunmpc::ik_kernel_occupancy(out8); }
int bmpc_ik_batch_struct_size(void) { return (int)sizeof(bmpc_ik_batch_t); }
double bmpc_model_total_mass(const bmpc_model_t *m) { return m ? m->host.total_mass : 0.0; }

// ----------------------------------------------------------- InverseKinematics ----
bmpc_ik_t *bmpc_ik_create(const bmpc_model_t *model, int n_col) {
    if (!model || n_col < 1) { ik_fail(BMPC_BAD_ARG, "bad InverseKinematics arguments"); return nullptr; }
    if (n_col > kMaxIkCol) { ik_fail(BMPC_BAD_ARG, "n_col > 255 is not supported"); return nullptr; }
    auto *h = new bmpc_ik;
    h->model = model; h->n_col = n_col;
    h->dt.assign(n_col, 0.0);
    h->nodes.resize(n_col + 1);
    return h;
}
void bmpc_ik_destroy(bmpc_ik_t *h) { delete h; }
int bmpc_ik_n_col(const bmpc_ik_t *h) { return h ? h->n_col : 0; }

int bmpc_ik_setup_costs(bmpc_ik_t *h, const double *dt, int n) {   // inverse_kinematics.cpp:37-52
    if (!h || !dt) return ik_fail(BMPC_BAD_ARG, "null argument");
    if (n < h->n_col) return ik_fail(BMPC_BAD_ARG, "dt must have n_col entries");
    h->dt.assign(dt, dt + h->n_col);
    return BMPC_OK;
}

#define IK_CHECK(...)                                                              \
    if (!h) return ik_fail(BMPC_BAD_ARG, "null handle");                           \
    { const void *ptrs_[] = {__VA_ARGS__};                                         \
      for (const void *p_ : ptrs_) if (!p_) return ik_fail(BMPC_BAD_ARG, "null array argument"); }

static int check_frame(const bmpc_ik *h, int frame) {
    if (frame < 0 || frame >= h->model->host.nframes) return ik_fail(BMPC_BAD_ARG, "frame id out of range");
    return BMPC_OK;
}

int bmpc_ik_add_position_tracking_task(bmpc_ik_t *h, int frame, int sn, int en, const double *traj3, double wt, const char *name) {
    IK_CHECK(traj3);
    if (int rc = check_frame(h, frame)) return rc;
    for (int i = sn; i < en; ++i) {   // end_effector_tasks.cpp:8-19: name + std::to_string(i)
        const std::string nm = std::string(name ? name : "") + std::to_string(i);
        if (int rc = add_item(h, i, nm.c_str(), IkItem{0, wt, frame, {traj3[0], traj3[1], traj3[2]}})) return rc;
    }
    return BMPC_OK;
}
int bmpc_ik_add_position_tracking_task_single(bmpc_ik_t *h, int frame, const double *traj3, double wt, const char *name, int time_step) {
    IK_CHECK(traj3);
    if (int rc = check_frame(h, frame)) return rc;
    if (time_step < 0 || time_step >= h->n_col) return ik_fail(BMPC_BAD_ARG, "time step out of range");
    return add_item(h, time_step, name, IkItem{0, wt, frame, {traj3[0], traj3[1], traj3[2]}});
}
int bmpc_ik_add_terminal_position_tracking_task(bmpc_ik_t *h, int frame, const double *traj3, double wt, const char *name) {
    IK_CHECK(traj3);
    if (int rc = check_frame(h, frame)) return rc;
    return add_item(h, h->n_col, name, IkItem{0, wt, frame, {traj3[0], traj3[1], traj3[2]}});
}
int bmpc_ik_add_velocity_tracking_task(bmpc_ik_t *h) {   // end_effector_tasks.cpp:49-56: a stub in the reference too
    IK_CHECK(h);
    std::cout << "function not implemented" << std::endl;
    return BMPC_OK;
}
static int add_traj(bmpc_ik *h, int kind, int width, int sn, int en, const double *traj, int rows, double wt, const char *name, int is_terminal) {
    if (!is_terminal) {
        if (sn < 0 || en > h->n_col || rows < en - sn) return ik_fail(BMPC_BAD_ARG, "trajectory shorter than the node range");
        for (int i = sn; i < en; ++i) {
            std::vector<double> r(traj + (size_t)(i - sn) * width, traj + (size_t)(i - sn + 1) * width);
            if (int rc = add_item(h, i, name, IkItem{kind, wt, -1, r})) return rc;
        }
        return BMPC_OK;
    }
    if (rows < 1) return ik_fail(BMPC_BAD_ARG, "empty trajectory");
    return add_item(h, h->n_col, name, IkItem{kind, wt, -1, std::vector<double>(traj, traj + width)});
}
int bmpc_ik_add_com_position_tracking_task(bmpc_ik_t *h, int sn, int en, const double *traj, int rows, double wt, const char *name, int is_terminal) {
    IK_CHECK(traj);
    return add_traj(h, 1, 3, sn, en, traj, rows, wt, name, is_terminal);   // com_tasks.cpp:8-28
}
int bmpc_ik_add_centroidal_momentum_tracking_task(bmpc_ik_t *h, int sn, int en, const double *traj, int rows, double wt, const char *name, int is_terminal) {
    IK_CHECK(traj);
    return add_traj(h, 2, 6, sn, en, traj, rows, wt, name, is_terminal);   // com_tasks.cpp:30-50
}
// regularisation items carry their own vectors (ref = [stateWeights 36 | x_reg 37] or [controlWeights 18]): the acyclic
// generator gives every node its own (abstract_acyclic_gen.py:225-290)
static IkItem state_item(double wt, const double *w, const double *xr) {
    IkItem it{3, wt, -1, std::vector<double>(w, w + bunmpc::kNDX)};
    it.ref.insert(it.ref.end(), xr, xr + bunmpc::kNX);
    return it;
}
static IkItem ctrl_item(double wt, const double *w) { return IkItem{4, wt, -1, std::vector<double>(w, w + bunmpc::kNV)}; }
int bmpc_ik_add_state_regularization_cost(bmpc_ik_t *h, int sn, int en, double wt, const char *name, const double *w36, const double *xreg37, int is_terminal) {
    IK_CHECK(w36, xreg37);   // regularization_costs.cpp:8-36
    if (is_terminal) return add_item(h, h->n_col, name, state_item(wt, w36, xreg37));
    if (sn < 0 || en > h->n_col) return ik_fail(BMPC_BAD_ARG, "node range out of bounds");
    for (int i = sn; i < en; ++i) if (int rc = add_item(h, i, name, state_item(wt, w36, xreg37))) return rc;
    return BMPC_OK;
}
int bmpc_ik_add_state_regularization_cost_single(bmpc_ik_t *h, int time_step, double wt, const char *name, const double *w36, const double *xreg37) {
    IK_CHECK(w36, xreg37);
    if (time_step < 0 || time_step >= h->n_col) return ik_fail(BMPC_BAD_ARG, "time step out of range");
    return add_item(h, time_step, name, state_item(wt, w36, xreg37));
}
int bmpc_ik_add_ctrl_regularization_cost(bmpc_ik_t *h, int sn, int en, double wt, const char *name, const double *w18, const double *ureg18, int is_terminal) {
    IK_CHECK(w18);   // regularization_costs.cpp:66-93; u_reg is ignored there (ResidualModelControl(state_))
    (void)ureg18;
    if (is_terminal) return add_item(h, h->n_col, name, ctrl_item(wt, w18));
    if (sn < 0 || en > h->n_col) return ik_fail(BMPC_BAD_ARG, "node range out of bounds");
    for (int i = sn; i < en; ++i) if (int rc = add_item(h, i, name, ctrl_item(wt, w18))) return rc;
    return BMPC_OK;
}
int bmpc_ik_add_ctrl_regularization_cost_single(bmpc_ik_t *h, int time_step, double wt, const char *name, const double *w18, const double *ureg18) {
    IK_CHECK(w18);
    (void)ureg18;
    if (time_step < 0 || time_step >= h->n_col) return ik_fail(BMPC_BAD_ARG, "time step out of range");
    return add_item(h, time_step, name, ctrl_item(wt, w18));
}

int bmpc_ik_workspace_doubles(int n_col) { return (int)bunmpc::IkLayout::make(n_col).total; }

// InverseKinematics::optimize (inverse_kinematics.cpp:54-71): ShootingProblem + SolverDDP::solve(), then fresh cost sums
int bmpc_ik_optimize(bmpc_ik_t *h, const double *x0) {
    using namespace bunmpc;
    IK_CHECK(x0);
    auto *model = const_cast<bmpc_model *>(h->model);
    const int T = h->n_col, nn = T + 1;
    std::vector<double> tasks;
    if (int rc = pack_tasks(h, tasks)) return rc;     // host-side validation first: its errors need no GPU
    if (int rc = model->upload()) return rc;
    const IkLayout L = IkLayout::make(T);
    // per-node regularisation vectors (nodes without the cost keep a neutral reference; their weight is 0 anyway)
    std::vector<double> sw((size_t)nn * kNDX, 0.0), xr((size_t)nn * kNX, 0.0), cw((size_t)nn * kNV, 0.0);
    for (int t = 0; t < nn; ++t) {
        xr[(size_t)t * kNX + 6] = 1.0;
        for (const auto &kv : h->nodes[t]) {
            const IkItem &it = kv.second;
            if (it.kind == 3) {
                std::copy(it.ref.begin(), it.ref.begin() + kNDX, sw.begin() + (size_t)t * kNDX);
                std::copy(it.ref.begin() + kNDX, it.ref.end(), xr.begin() + (size_t)t * kNX);
            } else if (it.kind == 4) std::copy(it.ref.begin(), it.ref.end(), cw.begin() + (size_t)t * kNV);
        }
    }
    // staging: x0 | dt | tasks | state_w | x_reg | ctrl_w
    std::vector<double> stage;
    auto push = [&](const double *p, size_t n) { size_t o = stage.size(); stage.insert(stage.end(), p, p + n); return o; };
    const size_t o_x0 = push(x0, kNX), o_dt = push(h->dt.data(), T), o_tk = push(tasks.data(), tasks.size()),
                 o_sw = push(sw.data(), sw.size()), o_xr = push(xr.data(), xr.size()), o_cw = push(cw.data(), cw.size());
    HIP_TRY(h->din.ensure(sizeof(double) * stage.size()));
    HIP_TRY(h->dws.ensure(sizeof(double) * (size_t)L.total));
    HIP_TRY(h->dactive.ensure(sizeof(int) * (1 + active_list_ints(1))));     // the counter + a one-problem active list (index checks, fused kernel)
    HIP_TRY(hipMemcpy(h->din.p, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice));
    const double *d = h->din.d();
    bmpc_ik_batch_t b{};      // (a zero sched: the process's knobs)
    b.B = 1; b.n_col = T; b.maxiter = 100; b.model = model; b.x0 = d + o_x0; b.dt = d + o_dt; b.tasks = d + o_tk; b.state_w = d + o_sw; b.x_reg = d + o_xr; b.ctrl_w = d + o_cw;
    b.sn_state_w = kNDX; b.sn_x_reg = kNX; b.sn_ctrl_w = kNV; b.ws = h->dws.d(); b.active = static_cast<int *>(h->dactive.p); b.active_list = b.active + 1;
    if (int rc = bmpc_ik_solve_batch_device(&b, nullptr)) return rc;
    h->xs.resize((size_t)nn * kNX); h->us.resize((size_t)T * kNV);
    double scal[16];
    HIP_TRY(hipMemcpy(h->xs.data(), h->dws.d() + L.xs, sizeof(double) * h->xs.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->us.data(), h->dws.d() + L.us, sizeof(double) * h->us.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(scal, h->dws.d() + L.scal, sizeof(scal), hipMemcpyDeviceToHost));
    h->iters = (int)scal[S_ITERS]; h->status = (int)scal[S_STATUS]; h->cost = scal[S_COST]; h->stop = scal[S_STOP];
    h->solved = true;
    for (auto &m : h->nodes) m.clear();   // rcost_arr_[i] / tcost_model_ replaced by empty CostModelSums
    return BMPC_OK;
}
int bmpc_ik_get_xs(const bmpc_ik_t *h, double *xs) {
    IK_CHECK(xs);
    if (!h->solved) return ik_fail(BMPC_BAD_ARG, "optimize has not been called");
    std::memcpy(xs, h->xs.data(), sizeof(double) * h->xs.size());
    return BMPC_OK;
}
int bmpc_ik_get_us(const bmpc_ik_t *h, double *us) {
    IK_CHECK(us);
    if (!h->solved) return ik_fail(BMPC_BAD_ARG, "optimize has not been called");
    std::memcpy(us, h->us.data(), sizeof(double) * h->us.size());
    return BMPC_OK;
}
static int com_mom(bmpc_ik *h, double *com, double *mom) {
    using namespace bunmpc;
    if (!h->solved) return ik_fail(BMPC_BAD_ARG, "optimize has not been called");
    const int nn = h->n_col + 1;
    Dev out;
    HIP_TRY(out.ensure(sizeof(double) * nn * 9));
    const IkLayout L = IkLayout::make(h->n_col);
    HIP_TRY(ik_launch_com_mom(h->model->dptr(), h->dws.d() + L.xs, out.d(), out.d() + nn * 3, nn, nullptr));
    if (com) HIP_TRY(hipMemcpy(com, out.d(), sizeof(double) * nn * 3, hipMemcpyDeviceToHost));
    if (mom) HIP_TRY(hipMemcpy(mom, out.d() + nn * 3, sizeof(double) * nn * 6, hipMemcpyDeviceToHost));
    return BMPC_OK;
}
int bmpc_ik_return_opt_com(bmpc_ik_t *h, double *com) { IK_CHECK(com); return com_mom(h, com, nullptr); }   // :73-82
int bmpc_ik_return_opt_mom(bmpc_ik_t *h, double *mom) { IK_CHECK(mom); return com_mom(h, nullptr, mom); }   // :84-93
int bmpc_ik_last_stats(const bmpc_ik_t *h, int *iters, int *status, double *cost, double *stop) {
    IK_CHECK(h);
    if (iters) *iters = h->iters;
    if (status) *status = h->status;
    if (cost) *cost = h->cost;
    if (stop) *stop = h->stop;
    return BMPC_OK;
}

// batch: many independent IK problems, everything on the device
int bmpc_ik_solve_batch_device(const bmpc_ik_batch_t *d, void *hip_stream) {
    bunmpc::IkBatchArgs a;
    if (int rc = args_from_batch(d, d ? d->maxiter : 0, true, nullptr, &a)) return rc;
    if (d->B == 0) return BMPC_OK;
    int iters = 0, rc = run_ddp(a, static_cast<hipStream_t>(hip_stream), &iters, resolve_knobs(&d->sched));
    if (d->iters_run) *d->iters_run = iters;
    return rc;
}
int bmpc_ik_centroidal_state_device(const bmpc_model_t *model, const double *x, double *out9, int B, void *hip_stream) {
    if (!model || !x || !out9) return ik_fail(BMPC_BAD_ARG, "null argument");
    auto *m = const_cast<bmpc_model *>(model);
    if (int rc = m->upload()) return rc;
    HIP_TRY(bunmpc::ik_launch_centroidal_state(m->dptr(), x, out9, B, static_cast<hipStream_t>(hip_stream)));
    return BMPC_OK;
}
// Self test of the derivative and Riccati passes (tests/test_ik_passes_gpu.py): ONE ik_state + ik_calcdiff + ik_backward launch
// at the caller's trajectory -- the launchers of the DDP loop, no forward pass, no host loop; the caller reads the workspace back
int bmpc_ik_selftest_passes(const bmpc_ik_batch_t *d, const double *xs, const double *us, int feasible, double xreg, int calcdiff_kernel,
                            int bwd_waves, void *hip_stream) {
    using namespace bunmpc;
    IkBatchArgs a;
    const char *bad = (feasible != 0 && feasible != 1) || (calcdiff_kernel != 0 && calcdiff_kernel != 1) || (bwd_waves != 1 && bwd_waves != 2)
                          ? "feasible and calcdiff_kernel must be 0 or 1, bwd_waves 1 or 2" : !(xreg >= 1e-9 && xreg < 1e9) ? "xreg outside [1e-9, 1e9)" : nullptr;
    if (int rc = args_from_batch(d, 1, xs && us, bad, &a)) return rc;
    if (d->B == 0) return BMPC_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    IkKnobs knobs = resolve_knobs(nullptr);      // the plan of a first look at the whole batch, with the two kernels under test forced through their knobs
    knobs.calcdiff_one_wave_above = calcdiff_kernel == 1 ? 0 : INT_MAX;
    knobs.gains_wave_below = bwd_waves == 2 ? INT_MAX : 0;
    const IkIterPlan plan = plan_iteration(a.B, a.B, a.T, a.list != nullptr, a.wide != nullptr, knobs);
    a.bwd_waves = plan.bwd_waves;
    HIP_TRY(ik_launch_init(a, st));
    HIP_TRY(ik_launch_selftest_set(a, xs, us, feasible, xreg, st));
    HIP_TRY(ik_launch(plan.state, a, st));
    HIP_TRY(ik_launch(plan.calcdiff, a, st));
    HIP_TRY(ik_launch_selftest_keep_costs(a, st));      // (the Riccati pass overwrites the parked node costs with the gaps)
    HIP_TRY(ik_launch(plan.backward, a, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BMPC_OK;
}
int bmpc_ik_last_calcdiff_kernel(void) { return bunmpc::ik_last_calcdiff_kernel(); }
// TEST ONLY: plan_batch + plan_iteration (ik_plan.h) of a batch shape under the process's knobs and `sched`; no GPU call
int bmpc_ik_plan_iteration(int B, int n_col, int maxiter, int has_list, int has_wide, int active, const bmpc_ik_sched_t *sched, bmpc_ik_iter_plan_t *out) {
    using namespace bunmpc;
    if (!out) return ik_fail(BMPC_BAD_ARG, "null plan");
    *out = bmpc_ik_iter_plan_t{};
    if (B < 1 || n_col < 1 || n_col > kMaxIkCol || maxiter < 1 || active < 1 || active > B) return out->status = ik_fail(BMPC_BAD_ARG, "bad sizes");
    const IkKnobs knobs = resolve_knobs(sched);
    const IkBatchPlan b = plan_batch(B, n_col, maxiter, has_list != 0, knobs);
    const IkIterPlan p = plan_iteration(active, B, n_col, has_list != 0, has_wide != 0, knobs);
    *out = bmpc_ik_iter_plan_t{BMPC_OK, b.fused_direct, b.express_cap, b.fused_grid, b.express_grid, p.chunk, p.fwd, p.bwd_waves, p.n_launch, {}, {}, {}, {},
                               kMaxFusedCol, kExpressFirstIter, kExpressLastIter, kTailChunk};
    const IkLaunch *from[4] = {&p.state, &p.calcdiff, &p.backward, &p.forward};
    bmpc_ik_planned_launch_t *to[4] = {&out->state, &out->calcdiff, &out->backward, &out->forward};
    for (int i = 0; i < 4; ++i) {
        std::strncpy(to[i]->kernel, kIkKernelNames[from[i]->kernel], sizeof(to[i]->kernel) - 1);
        to[i]->grid = from[i]->grid; to[i]->block = from[i]->block;
    }
    return BMPC_OK;
}
int bmpc_ik_layout_all(int n_col, long *offsets, int n) {
    const bunmpc::IkLayout L = bunmpc::IkLayout::make(n_col);
    const long all[] = {L.xs, L.us, L.scal, L.K, L.kff, L.fs, L.Lx, L.Lqq, L.xnext, L.Hn, L.Lu, L.Luu, L.A6, L.B6, L.nrs, L.njl, L.ncs, L.total, L.Quuk};
    const int have = (int)(sizeof(all) / sizeof(all[0]));
    for (int i = 0; offsets && i < n && i < have; ++i) offsets[i] = all[i];
    return have;
}
void bmpc_ik_layout(int n_col, long *offsets8) { (void)bmpc_ik_layout_all(n_col, offsets8, 8); }   // xs, us, scal, K, kff, fs, Lx, Lqq: for callers that read the workspace

long bmpc_ik_active_list_ints(long B) { return bunmpc::active_list_ints(B); }

void bmpc_ik_layout_trace(int n_col, long *offset, int *iters, int *width) {   // the per-iteration telemetry rows of a problem's workspace
    const bunmpc::IkLayout L = bunmpc::IkLayout::make(n_col);
    if (offset) *offset = L.trace;
    if (iters) *iters = bunmpc::kTraceIters;
    if (width) *width = bunmpc::kTraceDoubles;
}

// batch of KinoDynMP::optimize calls, device resident: centroidal state of (q, v) -> ADMM (cold start)
// -> tracking references -> IK-DDP.  cone == nullptr: the centroidal stage is bmpc_biconvex_solve_batch_device; otherwise it goes
// through the cone entry points (their kernels, and their refusals first: nothing is written or launched for a batch they refuse)
static int kinodyn_solve_batch(const bmpc_kinodyn_batch_t *d, const bmpc_cone_t *cone, const bmpc_contact_frame_t *frames, void *hip_stream) {
    if (!d || !d->x || !d->ik.model) return ik_fail(BMPC_BAD_ARG, "null KinoDyn batch descriptor");
    if (d->dyn.B != d->ik.B || d->ik.n_col > d->dyn.n_col) return ik_fail(BMPC_BAD_ARG, "inconsistent batch sizes / horizons");
    if (d->dyn.n_eff != 4) return ik_fail(BMPC_BAD_ARG, "KinoDynMP: n_eff must be 4 (the whole-body model is a 12-joint quadruped)");
    if (cone)
        if (int rc = bunmpc::check_cone_batch(&d->dyn, cone, frames)) return rc;
    if (d->dyn.B == 0) return BMPC_OK;
    auto *model = const_cast<bmpc_model *>(d->ik.model);
    if (int rc = model->upload()) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(bunmpc::ik_launch_centroidal_state(model->dptr(), d->x, const_cast<double *>(d->dyn.x_init), d->dyn.B, st));
    if (int rc = cone ? bmpc_biconvex_solve_batch_cone_frames_device(&d->dyn, cone, frames, hip_stream) : bmpc_biconvex_solve_batch_device(&d->dyn, hip_stream))
        return rc;
    HIP_TRY(bunmpc::ik_launch_fill_refs(const_cast<double *>(d->ik.tasks), d->dyn.X, d->dyn.m, d->dyn.B, d->dyn.n_col,
                                        d->ik.n_col, st));
    return bmpc_ik_solve_batch_device(&d->ik, hip_stream);
}
int bmpc_kinodyn_solve_batch_device(const bmpc_kinodyn_batch_t *d, void *hip_stream) { return kinodyn_solve_batch(d, nullptr, nullptr, hip_stream); }
int bmpc_kinodyn_solve_batch_cone_device(const bmpc_kinodyn_batch_t *d, const bmpc_cone_t *cone, const bmpc_contact_frame_t *frames, void *hip_stream) {
    return kinodyn_solve_batch(d, cone, frames, hip_stream);
}

// ------------------------------------------------------------------- KinoDynMP ----
bmpc_kinodyn_t *bmpc_kinodyn_create(const bmpc_model_t *model, double m, int n_eff, int dyn_col, int ik_col) {
    if (!model || ik_col < 1 || ik_col > dyn_col) { ik_fail(BMPC_BAD_ARG, "bad KinoDynMP arguments"); return nullptr; }
    if (n_eff != 4) { ik_fail(BMPC_BAD_ARG, "KinoDynMP: n_eff must be 4 (the whole-body model is a 12-joint quadruped)"); return nullptr; }
    auto *h = new bmpc_kinodyn;
    h->model = model; h->m = m; h->n_eff = n_eff; h->dyn_col = dyn_col; h->ik_col = ik_col;
    h->dyn = bmpc_biconvex_create(m, dyn_col, n_eff);
    h->ik = bmpc_ik_create(model, ik_col);
    if (!h->dyn || !h->ik) { bmpc_biconvex_destroy(h->dyn); bmpc_ik_destroy(h->ik); delete h; return nullptr; }
    std::cout << "Initialized Kino-Dyn planner" << std::endl;   // kino_dyn.cpp:8
    return h;
}
void bmpc_kinodyn_destroy(bmpc_kinodyn_t *h) { if (h) { bmpc_biconvex_destroy(h->dyn); bmpc_ik_destroy(h->ik); delete h; } }
bmpc_biconvex_t *bmpc_kinodyn_return_dyn(bmpc_kinodyn_t *h) { return h ? h->dyn : nullptr; }
bmpc_ik_t *bmpc_kinodyn_return_ik(bmpc_kinodyn_t *h) { return h ? h->ik : nullptr; }
int bmpc_kinodyn_set_com_tracking_weight(bmpc_kinodyn_t *h, double w) { IK_CHECK(h); h->wt_com = w; return BMPC_OK; }
int bmpc_kinodyn_set_mom_tracking_weight(bmpc_kinodyn_t *h, double w) { IK_CHECK(h); h->wt_mom = w; return BMPC_OK; }
int bmpc_kinodyn_compute_solve_times(bmpc_kinodyn_t *h) { IK_CHECK(h); h->profile = true; return BMPC_OK; }
int bmpc_kinodyn_return_solve_times(const bmpc_kinodyn_t *h, double *t3) { IK_CHECK(t3); std::memcpy(t3, h->solve_times, sizeof(h->solve_times)); return BMPC_OK; }

// KinoDynMP::optimize (kino_dyn.cpp:39-81)
int bmpc_kinodyn_optimize(bmpc_kinodyn_t *h, const double *q, const double *v, int dyn_iters, int kino_dyn_iters) {
    using namespace bunmpc;
    IK_CHECK(q, v);
    (void)kino_dyn_iters;   // unused in the reference as well
    const auto t1 = std::chrono::steady_clock::now();
    auto *model = const_cast<bmpc_model *>(h->model);
    if (int rc = model->upload()) return rc;
    double x0[kNX];
    std::memcpy(x0, q, sizeof(double) * kNQ);
    std::memcpy(x0 + kNQ, v, sizeof(double) * kNV);
    // computeCentroidalMomentum(q, v) -> [com, vcom, hg.angular]
    HIP_TRY(h->dtmp.ensure(sizeof(double) * (kNX + 9)));
    HIP_TRY(hipMemcpy(h->dtmp.p, x0, sizeof(x0), hipMemcpyHostToDevice));
    HIP_TRY(ik_launch_centroidal_state(model->dptr(), h->dtmp.d(), h->dtmp.d() + kNX, 1, nullptr));
    double c9[9];
    HIP_TRY(hipMemcpy(c9, h->dtmp.d() + kNX, sizeof(c9), hipMemcpyDeviceToHost));
    // set_warm_starts (kino_dyn.cpp:83-99): X = tile(c9), F = 0, P = 0
    const int H = h->dyn_col, nx = 9 * (H + 1), nf = 3 * h->n_eff * H;
    std::vector<double> X(nx), F(nf, 0.0), P(nx, 0.0);
    for (int i = 0; i <= H; ++i) std::memcpy(X.data() + 9 * i, c9, sizeof(c9));
    if (int rc = bmpc_biconvex_set_warm_start_vars(h->dyn, X.data(), F.data(), P.data())) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    int rc_dyn = bmpc_biconvex_optimize(h->dyn, c9, dyn_iters);
    if (rc_dyn != BMPC_OK && rc_dyn != BMPC_DIVERGED) return rc_dyn;
    const auto t3 = std::chrono::steady_clock::now();
    std::vector<double> com((size_t)(H + 1) * 3), mom((size_t)(H + 1) * 6);
    bmpc_biconvex_return_opt_com(h->dyn, com.data());
    bmpc_biconvex_return_opt_mom(h->dyn, mom.data());
    const int T = h->ik_col;
    // kino_dyn.cpp:53-56
    if (int rc = bmpc_ik_add_centroidal_momentum_tracking_task(h->ik, 0, T, mom.data(), T, h->wt_mom, "mom_track", 0)) return rc;
    if (int rc = bmpc_ik_add_centroidal_momentum_tracking_task(h->ik, 0, T, mom.data() + 6 * T, 1, h->wt_mom, "mom_track_ter", 1)) return rc;
    if (int rc = bmpc_ik_add_com_position_tracking_task(h->ik, 0, T, com.data(), T, h->wt_com, "com_track", 0)) return rc;
    if (int rc = bmpc_ik_add_com_position_tracking_task(h->ik, 0, T, com.data() + 3 * T, 1, h->wt_com, "com_track", 1)) return rc;
    const auto t4 = std::chrono::steady_clock::now();
    if (int rc = bmpc_ik_optimize(h->ik, x0)) return rc;
    const auto t5 = std::chrono::steady_clock::now();
    if (h->profile) {
        h->solve_times[0] = std::chrono::duration<double>(t3 - t2).count();
        h->solve_times[1] = std::chrono::duration<double>(t5 - t4).count();
        h->solve_times[2] = std::chrono::duration<double>(t5 - t1).count();
        std::cout << "Dyn optimize time : " << h->solve_times[0] << std::endl;
        std::cout << "Kin optimize time : " << h->solve_times[1] << std::endl;
        std::cout << "Total optimize time : " << h->solve_times[2] << std::endl;
        std::cout << "===============================================" << std::endl;
    }
    return rc_dyn;
}

}  // extern "C"

// cc_goals.hip (include/bunmpc_goals.h takes the model as an opaque pointer): the model's frame count and, with dev != nullptr,
// its device copy, uploaded on first use
int bunmpc::model_on_device(const void *model, int *nframes, const RobotModelDev **dev) {
    bmpc_model *m = const_cast<bmpc_model *>(static_cast<const bmpc_model *>(model));
    *nframes = m->host.nframes;
    if (dev) {
        if (int rc = m->upload()) return rc;
        *dev = m->dptr();
    }
    return BMPC_OK;
}
