// dcol_capi.cpp — host side of the C-ABI declared in include/dcol.h.
//
//  * dcol_table_create: digests the primitive descriptors into DevShape records and a pool
//    of orthant-row descriptors (DevRow), uploaded once to HBM.  This is the static part of
//    problem_matrices() (primitives/problem_matrices.py:4-209): the per-type constant rows;
//    the pose-dependent part (DCM, rotation, h) runs inside the kernel.
//  * dcol_plan_create: the plan's layout (dcol_plan.hpp plan_layout: each pair classified --
//    combine_problem_matrices.py:3-70 cases 1-3 vs the unsupported case 4 -- and bucketed by
//    kernel variant (N, NSOC, OMAX)) and its device state.
//  * dcol_plan_run: one kernel launch per non-empty bucket, asynchronous on the caller's
//    stream, no allocation (graph-capturable) -- or, for a small plan that mixes variants,
//    ONE fused launch covering every bucket (dcol_kernels_fused.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/dcol.h"
#include "dcol_device.hpp"
#include "dcol_host.hpp"
#include "dcol_launch.hpp"
#include "dcol_plan.hpp"

using namespace dcol;
using namespace dcol_host;

namespace {

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(DCOL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
};

// The side streams of a device, created once per process at the first table of the device
// and shared by all tables.  Early on purpose: HIP maps streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES, 4 by default) in creation order, and side streams created after a
// framework's stream pool (torch creates 32 at its first side stream) can share a queue with
// each other or with the caller's stream, which serialises the fan-out -- measured on the
// 1M mixed plan: 1.25 ms per solve with late side streams, 1.10 ms with early ones.
struct DeviceSide {
    std::mutex mu;
    bool tried = false, ok = false;
    hipStream_t s[kSideStreams] = {};
};
DeviceSide& device_side(int dev) {
    static DeviceSide g[64];
    return g[dev & 63];
}
// The plan policy's knobs (dcol_plan.hpp PlanPolicy), read from the environment once per
// process, at their first use
const PlanPolicy& plan_policy() {
    static const PlanPolicy pol = PlanPolicy::from_env();
    return pol;
}
// side streams per device, and those a plan that fills the GPU fans out over
int side_streams() { return plan_policy().side_streams; }
int large_side_streams() { return plan_policy().side_streams_large; }

// dcol_prox_pair's one-pair server: how long (us) it stays resident without a request
// (DCOL_PAIR_SERVER_IDLE_US, default 1000); DCOL_PAIR_SERVER=0: no server, one launch per
// call.  Read per call (tests switch it).
int pair_server_idle_us() {
    const char* on = std::getenv("DCOL_PAIR_SERVER");
    if (on && std::atoi(on) == 0) return 0;
    const char* e = std::getenv("DCOL_PAIR_SERVER_IDLE_US");
    const long v = e ? std::atol(e) : 1000;
    return v < 0 ? 0 : (v > 1000000 ? 1000000 : (int)v);
}
// Tables of the process, so that dcol_shutdown can stop every resident pair server before
// the process's HIP context and the servers' mapped mailboxes go away.  dcol_shutdown runs
// from an exit handler registered at the first server start -- after the HIP runtime
// initialised, so before its own exit-time teardown (exit handlers run last-registered
// first) -- and from the Python binding's atexit hook (dcol_amd/_lib.py).  Lock order:
// g_tables_mu, then a table's mu (dcol_prox_pair holds only the latter).
std::mutex g_tables_mu;
std::vector<dcol_table*> g_tables;
std::atomic<bool> g_shutdown{false};   // set by dcol_shutdown: no new server starts
std::atomic<int> g_server_tables{0};   // tables whose pair server was ever started
std::once_flag g_exit_hook;
// how long table destroy / shutdown / a restart wait for a server to leave (it leaves at its
// next poll, i.e. after at most the solve in hand: microseconds)
constexpr int kServerStopMs = 5000;

bool device_side_streams(int dev, hipStream_t out[kSideStreams]) {
    DeviceSide& d = device_side(dev);
    std::lock_guard<std::mutex> lk(d.mu);
    if (!d.tried) {
        d.tried = true;
        d.ok = true;
        for (int i = 0; d.ok && i < side_streams(); ++i) d.ok = hipStreamCreateWithFlags(&d.s[i], hipStreamNonBlocking) == hipSuccess;
        if (!d.ok) (void)hipGetLastError();
    }
    if (d.ok)
        for (int i = 0; i < side_streams(); ++i) out[i] = d.s[i];
    return d.ok;
}

}  // namespace

static_assert(dcol::kRec == DCOL_REC, "record width");

namespace dcol {
// pairs rejected on the host (unsupported combination / too many rows)
__global__ void __launch_bounds__(256) reject_kernel(KArgs A, int32_t code) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n) return;
    const int64_t pi = A.perm ? (int64_t)A.perm[A.slot0 + t] : (A.slot0 + t);
    const int64_t B = A.B;
    const double nan = __builtin_nan("");
    if (A.alpha) A.alpha[pi] = nan;
    if (A.iters) A.iters[pi] = 0;
    if (A.status) A.status[pi] = code;
    if ((A.flags & F_CONTACT) && A.contact)
        for (int q = 0; q < 3; ++q) A.contact[q * B + pi] = nan;
    if ((A.flags & (F_GRAD_FD | F_GRAD_ENV | F_GRAD_IMP)) && A.grad)
        for (int q = 0; q < 12; ++q) A.grad[q * B + pi] = nan;
    if ((A.flags & F_JAC) && A.jac)
        for (int q = 0; q < 48; ++q) A.jac[q * B + pi] = nan;
    if (A.rec) {
        double* r = A.rec + (int64_t)kRec * pi;
        for (int q = 0; q < 13; ++q) r[q] = nan;
        r[13] = rec_ints(code, 0);
    }
}

// The first order of a hinted launch's table (plan_hints): a grid of nothing but filler waves
// (hint_blocks 0, one window each) over zero hint bytes, i.e. the identity order with its
// gathered ids and its "none" entries
template <int LPP>
__global__ void __launch_bounds__(kBlock) hint_table_init(KArgs A) {
#if defined(__HIP_DEVICE_COMPILE__)
    hint_fill<LPP>(A);
#endif
}

}  // namespace dcol

struct dcol_table {
    int device = 0;
    std::vector<DevShape> shapes;
    std::vector<DevRow> rows;
    DevShape* d_shapes = nullptr;
    DevRow* d_rows = nullptr;
    // staging for dcol_prox_batch_host: device buffer + pinned host buffer (grow-only)
    std::mutex mu;
    void* stage = nullptr;
    size_t stage_bytes = 0;
    void* hstage = nullptr;
    size_t hstage_bytes = 0;
    int simds = 1024;   // SIMDs of the device (CUs x 4): below one wave per SIMD a launch is latency-bound
    // side streams for the concurrent variant launches of mixed plans: the process-wide set
    // of the device (device_side_streams), shared by every table
    hipStream_t side[kSideStreams] = {};
    bool side_ready = false;
    // dcol_prox_pair: one-pair plans per (shape1, shape2), at most DCOL_PAIR_PLANS_MAX, least
    // recently used first out (pair_lru: most recent at the front), a stream for their
    // launches, and the device-mapped pinned mailbox (PairBox: poses, outputs, the request of
    // the one-pair server and its stream)
    std::list<std::pair<int64_t, dcol_plan*>> pair_lru;
    std::unordered_map<int64_t, std::list<std::pair<int64_t, dcol_plan*>>::iterator> pair_plans;
    hipStream_t pair_stream = nullptr;
    hipStream_t server_stream = nullptr;
    PairBox* pair_host = nullptr;
    PairBox* pair_dev = nullptr;
    int64_t wall_ticks_us = 0;     // device wall-clock ticks per microsecond (0: unknown, no server)
    bool server_launched = false;  // a server was launched at least once (destroy stops it)
    int64_t n_served = 0, n_launched = 0, n_starts = 0;   // dcol_table_pair_stats
    int32_t srv_mismatch = 0;      // consecutive calls whose flags / tol / max_iter differ from the server's
    std::atomic<bool> stop_req{false};   // a batch launch asked the server to leave (yield_pair_servers)
    double srv_us = 0.0, srv_cycles = 0.0;
};

// A bucket of the plan's layout with its device state
struct Launch : Bucket {
    Launch() = default;
    Launch(const Bucket& b) : Bucket(b) {}
    // suspend / resume pair (DCOL_PLAN_SUSPEND): continuation entries, their buffers
    bool susp = false;
    int susp_fields = 0;
    int64_t susp_cap = 0;
    int32_t* d_susp_count = nullptr;
    int32_t* d_susp_pi = nullptr;
    double* d_susp_state = nullptr;
};

struct dcol_plan {
    const dcol_table* table = nullptr;
    int64_t B = 0;
    int32_t* d_s1 = nullptr;
    int32_t* d_s2 = nullptr;
    int32_t* d_perm = nullptr;   // nullptr when the whole batch is one variant
    bool owns = false;           // device arrays owned (false: views into table staging)
    PlanLayout lay;              // what the plan launches (dcol_plan.hpp plan_layout)
    std::vector<Launch> launches;   // lay.buckets, each with its device state
    hipEvent_t fork = nullptr;   // recorded on the caller's stream, awaited by the side streams
    hipEvent_t join[kSideStreams] = {};
    FusedSeg* d_segs = nullptr;  // lay.segs on the device
    void* d_susp = nullptr;      // DCOL_PLAN_SUSPEND scratch (one allocation for every such launch)
    bool jac = false;            // DCOL_PLAN_JACOBIAN: dense-row buckets (plan_layout_jac), no order hint
    // Order-hint state (plan_hints; dcol_device.hpp hint_fill_window): per stream the plan has
    // run on, two zero-filled uint8[B] buffers (one allocation), indexed by global slot, and
    // two launch-order tables of one HintEntry per lane group of every hinted launch's padded
    // grid (one allocation; 32 B per padded slot and stream in all), started at the identity
    // order.  Run k on the stream solves in the order of tab[k % 2] and writes its counts to
    // buf[k % 2]; its filler waves read buf[(k + 1) % 2] (run k - 1's counts) and write
    // tab[(k + 1) % 2], which nothing of run k reads.  Per stream, because dcol_plan_run takes
    // a const plan and runs concurrently on several streams.  Created lazily (never while the
    // stream captures), freed at dcol_plan_destroy; streams past kHintStreams run without a
    // hint.  mutable + mutex: dcol_plan_run's plan is const.
    static constexpr int kHintStreams = 8;
    struct HintState {
        hipStream_t stream = nullptr;
        uint8_t* buf = nullptr;     // [2][B]
        HintEntry* tab = nullptr;   // [2][entries]
        int64_t entries = 0;
        std::vector<int64_t> tab0;  // per launch: its base entry in a table, -1: not a hinted launch
        uint64_t runs = 0;
    };
    mutable std::mutex hint_mu;
    mutable HintState hints[kHintStreams];
    mutable int n_hints = 0;
    ~dcol_plan() {
        if (fork) (void)hipEventDestroy(fork);
        for (hipEvent_t& e : join)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// Stop a table's pair server, if one may be running: raise `stop` and wait for the server
// stream to drain, at most timeout_ms.  false: it did not drain -- the wave may still read
// the mailbox, which must then stay allocated.  The caller holds t->mu (or owns t).
bool stop_pair_server(dcol_table* t, int timeout_ms) {
    if (!t->server_launched || !t->pair_host) return true;
    __atomic_store_n(&t->pair_host->stop, 1, __ATOMIC_SEQ_CST);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(t->server_stream);
        if (q != hipErrorNotReady) {
            if (q != hipSuccess) (void)hipGetLastError();
            break;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms)) return false;
        std::this_thread::yield();
    }
    __atomic_store_n(&t->pair_host->stop, 0, __ATOMIC_SEQ_CST);
    __atomic_store_n(&t->pair_host->alive, 0, __ATOMIC_SEQ_CST);
    return true;
}

// A batch launch that can fill `device` (a plan that is not small: PlanLayout::small) asks
// every resident pair server there to leave (it does after
// the request in hand, at its next poll), without waiting: a kernel resident beside a batch
// plan slowed the plan by 1.3-2x depending on the server stream's kind and the number of
// hardware queues (tools/server_tax.py, profiles/r05_d/, r05_e/), so the latency path gives
// way to the throughput path.  The table's next dcol_prox_pair drains it and starts a new
// server (one launch, ~10 us).  Small plans (ALTRO-sized batches, one-pair launches) leave it
// resident: a caller interleaving them with drop-in calls would otherwise restart the server
// at nearly every pair call, and a latency-bound plan of a few waves is not what the
// server's hardware-queue tax was measured on.
void yield_pair_servers(int device) {
    if (g_server_tables.load(std::memory_order_acquire) == 0) return;
    static const bool off = [] {   // DCOL_PAIR_SERVER_YIELD=0: the server stays (A/B: tools/server_tax.py)
        const char* e = std::getenv("DCOL_PAIR_SERVER_YIELD");
        return e && std::atoi(e) == 0;
    }();
    if (off) return;
    std::lock_guard<std::mutex> lk(g_tables_mu);
    for (dcol_table* t : g_tables) {
        // (pair_host is published by dcol_prox_pair with a release store after its memset)
        PairBox* h = __atomic_load_n(&t->pair_host, __ATOMIC_ACQUIRE);
        if (t->device != device || !h) continue;
        if (!__atomic_load_n(&h->alive, __ATOMIC_ACQUIRE)) continue;
        __atomic_store_n(&h->stop, 1, __ATOMIC_SEQ_CST);
        t->stop_req.store(true, std::memory_order_release);
    }
}

hipError_t launch_variant(int N, int nsoc, int omax, int lpp, int flags, const KArgs& a, hipStream_t st, int oe = 0) {
    if (oe > 0) {
        if (N == 5 && nsoc == 1) return launch_part_n5s1(omax, oe, lpp, flags, a, st);
        if (N == 5 && nsoc == 2) return launch_part_n5s2(omax, oe, lpp, flags, a, st);
        if (N == 6 && nsoc == 1) return launch_part_n6s1(omax, oe, lpp, flags, a, st);
        if (N == 6 && nsoc == 2) {   // the ball-row copies first (a bucket's list order), then the dense ones
            const hipError_t e = launch_part_n6s2(omax, oe, lpp, flags, a, st);
            return e == hipErrorInvalidValue ? launch_part_n6s2_dense(omax, oe, lpp, flags, a, st) : e;
        }
        return hipErrorInvalidValue;
    }
    if (N == 4) return launch_n4(nsoc, omax, lpp, flags, a, st);
    if (N == 5) return launch_n5(nsoc, omax, lpp, flags, a, st);
    if (N == 6) return launch_n6(nsoc, omax, lpp, flags, a, st);
    if (N == 7) return launch_n7(nsoc, omax, lpp, flags, a, st);
    if (N == 8) return launch_n8(nsoc, omax, lpp, flags, a, st);
    return hipErrorInvalidValue;
}

// the contact-point Jacobian copy of a dense-row bucket (dcol_kernels_jac.hip)
hipError_t launch_jac(int N, int nsoc, int omax, int lpp, const KArgs& a, hipStream_t st) {
    if (N == 4) return launch_jac_n4(nsoc, omax, lpp, a, st);
    if (N == 5) return launch_jac_n5(nsoc, omax, lpp, a, st);
    if (N == 6) return launch_jac_n6(nsoc, omax, lpp, a, st);
    if (N == 7) return launch_jac_n7(nsoc, omax, lpp, a, st);
    if (N == 8) return launch_jac_n8(nsoc, omax, lpp, a, st);
    return hipErrorInvalidValue;
}

}  // namespace

extern "C" {

int dcol_abi_version(void) { return DCOL_ABI_VERSION; }

const char* dcol_status_string(int32_t s) {
    switch (s) {
        case DCOL_OK: return "ok";
        case DCOL_MAXITER: return "Maximum number of iterations reached, PDIP failed";
        case DCOL_UNSUPPORTED: return "Failed to combine problem matrices.";
        case DCOL_NOT_PD: return "Matrix is not positive definite";
        case DCOL_NONFINITE: return "array must not contain infs or NaNs";
        case DCOL_TOO_LARGE:
            return "pair exceeds the engine's orthant-row capacity (1024 rows; 32 for a case-4 pair without "
                   "DCOL_PLAN_CASE4_STREAM, 128 with the contact-point Jacobian)";
        default: return "unknown status";
    }
}

const char* dcol_last_error(void) { return last_error().c_str(); }

int dcol_device_count(int32_t* count) {
    if (!count) return fail(DCOL_ERR_ARG, "count is NULL");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    *count = n;
    return DCOL_SUCCESS;
}

int dcol_table_create(const dcol_shape_desc* shapes, int32_t n, int32_t device, dcol_table** out) {
    if (!out || n < 0 || (n > 0 && !shapes)) return fail(DCOL_ERR_ARG, "dcol_table_create: bad arguments");
    *out = nullptr;
    auto* t = new (std::nothrow) dcol_table();
    if (!t) return fail(DCOL_ERR_NOMEM, "host allocation failed");
    t->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            t->simds = 4 * cus;
        else
            (void)hipGetLastError();
    }
    t->shapes.resize(n);
    init_row_pool(t->rows);
    for (int32_t i = 0; i < n; ++i) {
        int rc = digest_shape(shapes[i], i, t->shapes[i], t->rows);
        if (rc != DCOL_SUCCESS) {
            delete t;
            return rc;
        }
    }
    if (t->shapes.empty()) t->shapes.resize(1);
    DeviceGuard g(device);
    hipError_t e = hipMalloc(&t->d_shapes, sizeof(DevShape) * t->shapes.size());
    if (e == hipSuccess) e = hipMalloc(&t->d_rows, sizeof(DevRow) * t->rows.size());
    if (e == hipSuccess) e = hipMemcpy(t->d_shapes, t->shapes.data(), sizeof(DevShape) * t->shapes.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_rows, t->rows.data(), sizeof(DevRow) * t->rows.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (t->d_shapes) (void)hipFree(t->d_shapes);
        if (t->d_rows) (void)hipFree(t->d_rows);
        delete t;
        return fail(DCOL_ERR_HIP, std::string("dcol_table_create: ") + hipGetErrorString(e));
    }
    t->shapes.resize(n);
    t->side_ready = device_side_streams(device, t->side);   // early: see DeviceSide
    {
        std::lock_guard<std::mutex> lk(g_tables_mu);
        g_tables.push_back(t);
    }
    *out = t;
    return DCOL_SUCCESS;
}

int dcol_table_destroy(dcol_table* t) {
    if (!t) return DCOL_SUCCESS;
    DeviceGuard g(t->device);
    // the server exits at its next poll; one that does not (a hung device) keeps the whole
    // table -- its wave may still read the shape table and the mailbox -- registered, so that
    // dcol_shutdown still sees it and can stop it before the process's HIP context goes away,
    // and the call fails.  Only a table whose server has left is unregistered and freed.
    {
        std::lock_guard<std::mutex> tl(t->mu);
        if (!stop_pair_server(t, kServerStopMs))
            return fail(DCOL_ERR_HIP, "dcol_table_destroy: the pair server did not stop within 5 s (table kept)");
    }
    {
        std::lock_guard<std::mutex> lk(g_tables_mu);
        g_tables.erase(std::remove(g_tables.begin(), g_tables.end(), t), g_tables.end());
        if (t->server_launched) g_server_tables.fetch_sub(1, std::memory_order_acq_rel);
    }
    for (auto& kv : t->pair_lru) dcol_plan_destroy(kv.second);
    if (t->pair_stream) (void)hipStreamDestroy(t->pair_stream);
    if (t->server_stream) (void)hipStreamDestroy(t->server_stream);
    if (t->pair_host) (void)hipHostFree(t->pair_host);
    if (t->d_shapes) (void)hipFree(t->d_shapes);
    if (t->d_rows) (void)hipFree(t->d_rows);
    if (t->stage) (void)hipFree(t->stage);
    if (t->hstage) (void)hipHostFree(t->hstage);
    delete t;
    return DCOL_SUCCESS;
}

int dcol_table_size(const dcol_table* t, int32_t* n) {
    if (!t || !n) return fail(DCOL_ERR_ARG, "dcol_table_size: NULL argument");
    *n = (int32_t)t->shapes.size();
    return DCOL_SUCCESS;
}

int dcol_pair_dims(const dcol_table* t, int32_t s1, int32_t s2, int32_t* m, int32_t* n, int32_t* n_soc, int32_t* status) {
    if (!t) return fail(DCOL_ERR_ARG, "dcol_pair_dims: NULL table");
    const int32_t ns = (int32_t)t->shapes.size();
    if (s1 < 0 || s1 >= ns || s2 < 0 || s2 >= ns) return fail(DCOL_ERR_ARG, "dcol_pair_dims: shape id out of range");
    const DevShape& a = t->shapes[s1];
    const DevShape& b = t->shapes[s2];
    PairClass c = classify(a, b);
    const int q1 = a.soc_kind == SOC_NONE ? 0 : (a.soc_kind == SOC_CONE ? 3 : 4);
    const int q2 = b.soc_kind == SOC_NONE ? 0 : (b.soc_kind == SOC_CONE ? 3 : 4);
    if (m) *m = c.o + q1 + q2;
    if (n) *n = c.N;
    if (n_soc) *n_soc = c.nsoc;
    if (status) *status = c.status;
    return DCOL_SUCCESS;
}

}  // extern "C"

namespace {
// DCOL_PLAN_SUSPEND: every large solve bucket with a suspend / resume variant gets its
// continuation buffers (entries: DCOL_SUSPEND_T per wave, default 4; DCOL_NO_SUSPEND=1
// disables).  Allocates; returns DCOL_SUCCESS or an error.
int susp_t_env() {
    static const int t = [] {
        const char* e = std::getenv("DCOL_SUSPEND_T");
        return std::getenv("DCOL_NO_SUSPEND") ? 0 : (e ? std::max(0, std::atoi(e)) : 4);
    }();
    return t;
}
int susp_min_env() {
    static const int m = [] {
        const char* e = std::getenv("DCOL_SUSPEND_MIN");
        return e ? std::max(0, std::atoi(e)) : 6;
    }();
    return m;
}
int plan_susp(const dcol_table* t, dcol_plan* p) {
    const int T = susp_t_env();
    if (T <= 0 || p->lay.fused()) return DCOL_SUCCESS;   // packed plans too: ADVICE.md (kept as is)
    size_t bytes = 0;
    for (Launch& L : p->launches) {
        int f = 0;
        if (L.kind != 0 || L.n * L.lpp < 64LL * t->simds || !susp_available(L.N, L.nsoc, L.omax, L.lpp, L.flags(), L.oe, &f))
            continue;
        L.susp = true;
        L.susp_fields = f;
        L.susp_cap = ((L.n * L.lpp + 63) / 64) * (int64_t)T;
        bytes += 256 + (size_t)L.susp_cap * (sizeof(int32_t) + sizeof(double) * f);
    }
    if (bytes == 0) return DCOL_SUCCESS;
    DeviceGuard g(t->device);
    hipError_t e = hipMalloc(&p->d_susp, bytes);
    if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("suspend scratch: ") + hipGetErrorString(e));
    char* c = static_cast<char*>(p->d_susp);
    for (Launch& L : p->launches) {
        if (!L.susp) continue;
        L.d_susp_count = reinterpret_cast<int32_t*>(c);
        c += 256;
        L.d_susp_state = reinterpret_cast<double*>(c);
        c += sizeof(double) * L.susp_fields * (size_t)L.susp_cap;
        L.d_susp_pi = reinterpret_cast<int32_t*>(c);
        c += sizeof(int32_t) * (size_t)L.susp_cap;
    }
    return DCOL_SUCCESS;
}

int ensure_fanout(const dcol_table* tc, dcol_plan* p) {
    if (p->lay.lanes <= 1) return DCOL_SUCCESS;
    dcol_table* t = const_cast<dcol_table*>(tc);
    DeviceGuard g(t->device);
    if (!t->side_ready) return fail(DCOL_ERR_HIP, "side streams of the device could not be created");
    hipError_t e = hipEventCreateWithFlags(&p->fork, hipEventDisableTiming);
    for (int i = 0; e == hipSuccess && i < p->lay.lanes - 1; ++i) e = hipEventCreateWithFlags(&p->join[i], hipEventDisableTiming);
    if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("fan-out events: ") + hipGetErrorString(e));
    return DCOL_SUCCESS;
}

// The plan's layout under the process's policy, and its launches
int plan_build(const dcol_table* t, int64_t B, const int32_t* s1, const int32_t* s2, bool case4, bool allow_fuse,
               dcol_plan* p, bool jac = false, bool jac_stream = false, bool case4_stream = false) {
    const int rc = jac ? plan_layout_jac(t->shapes, t->simds, B, s1, s2, case4, plan_policy(), p->lay, jac_stream, case4_stream)
                       : plan_layout(t->shapes, t->simds, B, s1, s2, case4, allow_fuse, plan_policy(), p->lay, case4_stream);
    if (rc != DCOL_SUCCESS) return rc;
    p->jac = jac;
    p->table = t;
    p->B = B;
    p->launches.assign(p->lay.buckets.begin(), p->lay.buckets.end());
    return DCOL_SUCCESS;
}
}  // namespace

extern "C" {

int dcol_plan_create(const dcol_table* t, int64_t B, const int32_t* s1, const int32_t* s2, dcol_plan** out) {
    return dcol_plan_create_ex(t, B, s1, s2, 0, out);
}

int dcol_plan_create_ex(const dcol_table* t, int64_t B, const int32_t* s1, const int32_t* s2, int32_t options,
                        dcol_plan** out) {
    if (!t || !out || B < 0 || (B > 0 && (!s1 || !s2))) return fail(DCOL_ERR_ARG, "dcol_plan_create: bad arguments");
    if (options & ~(DCOL_PLAN_CASE4 | DCOL_PLAN_NO_FUSE | DCOL_PLAN_SUSPEND | DCOL_PLAN_JACOBIAN | DCOL_PLAN_JACOBIAN_STREAM |
                    DCOL_PLAN_CASE4_STREAM))
        return fail(DCOL_ERR_ARG, "dcol_plan_create_ex: unknown option bits");
    if ((options & DCOL_PLAN_CASE4_STREAM) && !(options & DCOL_PLAN_CASE4))
        return fail(DCOL_ERR_ARG, "dcol_plan_create_ex: DCOL_PLAN_CASE4_STREAM needs DCOL_PLAN_CASE4");
    if ((options & DCOL_PLAN_JACOBIAN_STREAM) && !(options & DCOL_PLAN_JACOBIAN))
        return fail(DCOL_ERR_ARG, "dcol_plan_create_ex: DCOL_PLAN_JACOBIAN_STREAM needs DCOL_PLAN_JACOBIAN");
    if ((options & DCOL_PLAN_JACOBIAN) && (options & DCOL_PLAN_SUSPEND))
        return fail(DCOL_ERR_ARG, "dcol_plan_create_ex: DCOL_PLAN_JACOBIAN cannot be combined with DCOL_PLAN_SUSPEND");
    if (B > INT32_MAX) return fail(DCOL_ERR_ARG, "dcol_plan_create: B exceeds 2^31-1");
    *out = nullptr;
    auto* p = new (std::nothrow) dcol_plan();
    if (!p) return fail(DCOL_ERR_NOMEM, "host allocation failed");
    int rc = plan_build(t, B, s1, s2, (options & DCOL_PLAN_CASE4) != 0, (options & DCOL_PLAN_NO_FUSE) == 0, p,
                        (options & DCOL_PLAN_JACOBIAN) != 0, (options & DCOL_PLAN_JACOBIAN_STREAM) != 0,
                        (options & DCOL_PLAN_CASE4_STREAM) != 0);
    if (rc != DCOL_SUCCESS) {
        delete p;
        return rc;
    }
    p->owns = true;
    if (B == 0) {
        *out = p;
        return DCOL_SUCCESS;
    }
    DeviceGuard g(t->device);
    hipError_t e = hipMalloc(&p->d_s1, sizeof(int32_t) * B);
    if (e == hipSuccess) e = hipMalloc(&p->d_s2, sizeof(int32_t) * B);
    if (e == hipSuccess) e = hipMemcpy(p->d_s1, s1, sizeof(int32_t) * B, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_s2, s2, sizeof(int32_t) * B, hipMemcpyHostToDevice);
    // (a lone streamed bucket too: its slots are sorted by row count)
    if (e == hipSuccess && (p->launches.size() > 1 || (p->launches[0].stream && B > 1))) {
        e = hipMalloc(&p->d_perm, sizeof(int32_t) * B);
        if (e == hipSuccess) e = hipMemcpy(p->d_perm, p->lay.perm.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice);
    }
    std::vector<int32_t>().swap(p->lay.perm);   // lives on the device from here on
    if (e == hipSuccess && p->lay.fused()) {
        const size_t sb = sizeof(FusedSeg) * p->lay.segs.size();
        e = hipMalloc(&p->d_segs, sb);
        if (e == hipSuccess) e = hipMemcpy(p->d_segs, p->lay.segs.data(), sb, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        dcol_plan_destroy(p);
        return fail(DCOL_ERR_HIP, std::string("dcol_plan_create: ") + hipGetErrorString(e));
    }
    rc = ensure_fanout(t, p);
    if (rc == DCOL_SUCCESS && (options & DCOL_PLAN_SUSPEND)) rc = plan_susp(t, p);
    if (rc != DCOL_SUCCESS) {
        dcol_plan_destroy(p);
        return rc;
    }
    *out = p;
    return DCOL_SUCCESS;
}

int dcol_plan_destroy(dcol_plan* p) {
    if (!p) return DCOL_SUCCESS;
    if (p->table && p->owns) {
        DeviceGuard g(p->table->device);
        if (p->d_s1) (void)hipFree(p->d_s1);
        if (p->d_s2) (void)hipFree(p->d_s2);
        if (p->d_perm) (void)hipFree(p->d_perm);
        if (p->d_segs) (void)hipFree(p->d_segs);
        if (p->d_susp) (void)hipFree(p->d_susp);
    }
    if (p->table && p->n_hints > 0) {
        DeviceGuard g(p->table->device);
        for (int i = 0; i < p->n_hints; ++i) {
            if (p->hints[i].buf) (void)hipFree(p->hints[i].buf);
            if (p->hints[i].tab) (void)hipFree(p->hints[i].tab);
        }
    }
    delete p;
    return DCOL_SUCCESS;
}

int dcol_plan_suspended(const dcol_plan* p, int64_t* n) {
    if (!p || !n) return fail(DCOL_ERR_ARG, "dcol_plan_suspended: NULL argument");
    *n = 0;
    if (!p->d_susp) return DCOL_SUCCESS;
    DeviceGuard g(p->table->device);
    for (const Launch& L : p->launches) {
        if (!L.susp) continue;
        int32_t c = 0;
        const hipError_t e = hipMemcpy(&c, L.d_susp_count, sizeof(c), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_plan_suspended: ") + hipGetErrorString(e));
        *n += c;
    }
    return DCOL_SUCCESS;
}

int dcol_plan_num_launches(const dcol_plan* p, int32_t* n) {
    if (!p || !n) return fail(DCOL_ERR_ARG, "dcol_plan_num_launches: NULL argument");
    int32_t k = 0;
    for (const Launch& L : p->launches) k += (L.kind != 0 || !p->lay.fused());
    *n = k + (p->lay.fused() ? 1 : 0);
    return DCOL_SUCCESS;
}

int dcol_plan_num_streams(const dcol_plan* p, int32_t* n) {
    if (!p || !n) return fail(DCOL_ERR_ARG, "dcol_plan_num_streams: NULL argument");
    *n = p->lay.fused() ? 1 : p->lay.lanes;
    return DCOL_SUCCESS;
}

int dcol_plan_launch_form(const dcol_plan* p, int32_t* form) {
    if (!p || !form) return fail(DCOL_ERR_ARG, "dcol_plan_launch_form: NULL argument");
    *form = !p->lay.fused() ? DCOL_FORM_BUCKETS : (p->lay.packed ? DCOL_FORM_PACKED : DCOL_FORM_FUSED);
    return DCOL_SUCCESS;
}

int dcol_plan_num_buckets(const dcol_plan* p, int32_t* n) {
    if (!p || !n) return fail(DCOL_ERR_ARG, "dcol_plan_num_buckets: NULL argument");
    *n = (int32_t)p->launches.size();
    return DCOL_SUCCESS;
}

int dcol_plan_bucket(const dcol_plan* p, int32_t i, int32_t info[8], int64_t* pairs) {
    if (!p || !info || !pairs) return fail(DCOL_ERR_ARG, "dcol_plan_bucket: NULL argument");
    if (i < 0 || i >= (int32_t)p->launches.size()) return fail(DCOL_ERR_ARG, "dcol_plan_bucket: index out of range");
    const Launch& L = p->launches[(size_t)i];
    const bool solve = L.kind == 0;
    const int32_t v[8] = {L.kind, solve ? L.N : 0, solve ? L.nsoc : 0, solve ? L.omax : 0, solve ? L.lpp : 0,
                          solve ? L.oe : 0, solve ? L.flags() : 0, solve ? 0 : L.code};
    for (int k = 0; k < 8; ++k) info[k] = v[k];
    *pairs = L.n;
    return DCOL_SUCCESS;
}

}  // extern "C"

namespace {
// waves per order-hint window (DCOL_HINT_WAVES, 1..kHintWavesMax; A/B runs)
int hint_waves() {
    static const int ww = [] {
        const char* e = std::getenv("DCOL_HINT_WAVES");
        const int v = e ? std::atoi(e) : kHintWavesDefault;
        return std::min(std::max(v, 1), kHintWavesMax);
    }();
    return ww;
}

// windows per filler wave (DCOL_HINT_FILL_WINDOWS, 1..8; A/B runs).  Swept 1 / 2 / 4 at 4
// waves per window: DESIGN.md section 5
int hint_fill_windows() {
    static const int fw = [] {
        const char* e = std::getenv("DCOL_HINT_FILL_WINDOWS");
        return std::min(std::max(e ? std::atoi(e) : 1, 1), 8);
    }();
    return fw;
}

bool hinted_launch(const Launch& L) { return L.kind == 0 && !L.susp && !L.stream; }

// the identity order of launch L (entries from tab0) into tab, on st; rd: zero hint bytes
hipError_t hint_table_start(const dcol_plan* p, const Launch& L, const uint8_t* rd, HintEntry* tab, int64_t tab0,
                            hipStream_t st) {
    KArgs a{};
    a.s1 = p->d_s1;
    a.s2 = p->d_s2;
    a.perm = p->d_perm;
    a.B = p->B;
    a.slot0 = L.slot0;
    a.n = L.n;
    a.hint_r = rd;
    a.hint_ww = hint_waves();
    a.hint_wins = hint_windows(L.n, L.lpp, a.hint_ww);
    a.hint_tab_w = tab;
    a.hint_tab0 = tab0;
    a.hint_blocks = 0;
    a.hint_fw = 1;
    const dim3 grid((unsigned)hint_filler_blocks(a.hint_wins, 1)), block(kBlock);
    switch (L.lpp) {
        case 1: hipLaunchKernelGGL(hint_table_init<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(hint_table_init<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(hint_table_init<4>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(hint_table_init<8>, grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// What a hinted run of p on st reads and writes (dcol_plan::HintState)
struct HintRun {
    const uint8_t* rd = nullptr;        // the previous run's iteration counts (zeros before it)
    uint8_t* wr = nullptr;              // where this run leaves its own
    const HintEntry* tab_r = nullptr;   // this run's order
    HintEntry* tab_w = nullptr;         // where this run's filler waves leave the next run's
    const int64_t* tab0 = nullptr;      // per launch of the plan: its base entry
};

// The order-hint state of this run of p on st.  false: the run goes without a hint
// (DCOL_NO_ORDER_HINT=1; a plan with no hinted launch; a first run on a capturing stream; more
// than kHintStreams streams; no memory).  A run captured into a graph keeps the buffers it was
// captured with at every replay: the table it reads is never written by a replay, a frozen,
// consistent order.
bool plan_hints(const dcol_plan* p, hipStream_t st, HintRun* R) {
    static const bool off = [] {
        const char* e = std::getenv("DCOL_NO_ORDER_HINT");
        return e && *e && *e != '0';
    }();
    if (off || p->jac || p->lay.fused() || p->B >= (int64_t)1 << 31) return false;
    bool any = false;
    for (const Launch& L : p->launches) any = any || hinted_launch(L);
    if (!any) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (capturing) (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(p->hint_mu);
    dcol_plan::HintState* S = nullptr;
    for (int i = 0; i < p->n_hints && !S; ++i)
        if (p->hints[i].stream == st) S = &p->hints[i];
    if (!S) {
        if (capturing || p->n_hints >= dcol_plan::kHintStreams) return false;
        // every hinted launch's share of a table, in launch order
        const int ww = hint_waves();
        std::vector<int64_t> tab0(p->launches.size(), -1);
        int64_t entries = 0;
        for (size_t i = 0; i < p->launches.size(); ++i) {
            const Launch& L = p->launches[i];
            if (!hinted_launch(L)) continue;
            tab0[i] = entries;
            entries += (int64_t)hint_windows(L.n, L.lpp, ww) * ww * (64 / L.lpp);
        }
        uint8_t* b = nullptr;
        HintEntry* tab = nullptr;
        bool ok = hipMalloc(&b, 2 * (size_t)p->B) == hipSuccess &&
                  hipMalloc(&tab, 2 * (size_t)entries * sizeof(HintEntry)) == hipSuccess &&
                  hipMemsetAsync(b, 0, 2 * (size_t)p->B, st) == hipSuccess;
        for (size_t i = 0; ok && i < p->launches.size(); ++i)
            for (int k = 0; ok && k < 2 && tab0[i] >= 0; ++k)
                ok = hint_table_start(p, p->launches[i], b, tab + k * entries, tab0[i], st) == hipSuccess;
        if (!ok) {
            // (a start kernel already queued may still run: let it before its memory goes)
            (void)hipGetLastError();
            (void)hipStreamSynchronize(st);
            (void)hipGetLastError();
            if (b) (void)hipFree(b);
            if (tab) (void)hipFree(tab);
            return false;
        }
        S = &p->hints[p->n_hints++];
        S->stream = st;
        S->buf = b;
        S->tab = tab;
        S->entries = entries;
        S->tab0 = std::move(tab0);
        S->runs = 0;
    }
    const uint64_t k = S->runs & 1;
    R->wr = S->buf + k * (size_t)p->B;
    R->rd = S->buf + (k ^ 1) * (size_t)p->B;
    R->tab_r = S->tab + k * S->entries;
    R->tab_w = S->tab + (k ^ 1) * S->entries;
    R->tab0 = S->tab0.data();
    if (!capturing) ++S->runs;
    return true;
}

// dcol_plan_run with an optional record output (rec: [B][DCOL_REC], written by the solver
// epilogues; then alpha / grad / iters / status may be NULL)
// hint: the run may use and leave an order hint (not dcol_prox_batch_host's plan, which
// runs once, nor dcol_prox_pair's one-pair plans, which have nothing to order)
int plan_run_rec(const dcol_plan* p, const double* pose1, const double* pose2, double tol, int32_t max_iter,
                 int32_t flags, double* alpha, double* contact, double* grad, int32_t* iters, int32_t* status,
                 double* rec, void* stream, bool yield = true, bool hint = true, double* jac = nullptr) {
    if (!p) return fail(DCOL_ERR_ARG, "dcol_plan_run: NULL plan");
    // (the pair call's own launch path keeps it).  A small plan keeps it too -- unless it is
    // launched on the null stream: the server runs on a blocking stream (CU-masked streams
    // have no non-blocking form), so null-stream work waits for it to leave, i.e. for its idle
    // time (DCOL_PAIR_SERVER_IDLE_US) -- asking it to leave now costs a restart instead.
    if (yield && (!p->lay.small || stream == nullptr)) yield_pair_servers(p->table->device);
    // The contact-point Jacobian: jac is set by dcol_plan_run_jac alone, after its checks, and
    // then the plan's dense-row buckets launch their Jacobian copies (the streamed buckets of a
    // DCOL_PLAN_JACOBIAN_STREAM plan: the streamed kernels' Jacobian copies).  The kernels' F_JAC bit
    // follows jac, so DCOL_JACOBIAN in any other caller's flags is dropped here (it had no
    // meaning before ABI 5).
    const bool want_jac = jac != nullptr;
    flags = want_jac ? (flags | DCOL_JACOBIAN) : (flags & ~DCOL_JACOBIAN);
    if (p->B == 0) return DCOL_SUCCESS;
    if (!pose1 || !pose2 || (!alpha && !rec))
        return fail(DCOL_ERR_ARG, "dcol_plan_run: pose1, pose2 and alpha are required");
    if ((flags & DCOL_CONTACT) && !contact) return fail(DCOL_ERR_ARG, "dcol_plan_run: DCOL_CONTACT needs contact[]");
    if ((flags & DCOL_GRAD_ANY) && !grad && !rec) return fail(DCOL_ERR_ARG, "dcol_plan_run: gradient flag needs grad[]");
    if (max_iter < 0) return fail(DCOL_ERR_ARG, "dcol_plan_run: max_iter < 0");
    const dcol_table* t = p->table;
    DeviceGuard g(t->device);
    // the launch checks below read the thread's last HIP error: clear one a caller's earlier
    // HIP call left behind (not ours to report)
    (void)hipGetLastError();
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    KArgs a;
    a.shapes = t->d_shapes;
    a.rows = t->d_rows;
    a.s1 = p->d_s1;
    a.s2 = p->d_s2;
    a.pose1 = pose1;
    a.pose2 = pose2;
    a.perm = p->d_perm;
    a.B = p->B;
    a.tol = tol;
    a.max_iter = max_iter;
    a.flags = flags;
    a.alpha = alpha;
    a.contact = contact;
    a.grad = grad;
    a.iters = iters;
    a.status = status;
    a.rec = rec;
    a.susp_t = 0;
    a.susp_min = 0;
    a.susp_count = nullptr;
    a.susp_pi = nullptr;
    a.susp_state = nullptr;
    a.susp_cap = 0;
    a.jac = want_jac ? jac : nullptr;
    // a run without envelope / implicit gradients may take a bucket's FD-only copy (LF_FDONLY)
    const int fdonly = (flags & (DCOL_GRAD_ENVELOPE | DCOL_GRAD_IMPLICIT)) ? 0 : LF_FDONLY;
    const bool fan = p->lay.lanes > 1 && p->fork;
    hipError_t e = hipSuccess;
    // (before the fork: the side streams' launches then follow a new state's zero fill and
    // first tables)
    HintRun hr;
    const bool hinted = hint && plan_hints(p, st, &hr);
    if (fan) {
        e = hipEventRecord(p->fork, st);
        for (int l = 1; e == hipSuccess && l < p->lay.lanes; ++l) e = hipStreamWaitEvent(t->side[l - 1], p->fork, 0);
        if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_plan_run fork: ") + hipGetErrorString(e));
    }
    const size_t nl = p->launches.size();
    for (size_t li = 0; li < nl; ++li) {
        const size_t lx = p->lay.issue.size() == nl ? (size_t)p->lay.issue[li] : li;
        const Launch& L = p->launches[lx];
        if (L.kind == 0 && p->lay.fused()) continue;   // covered by the fused launch below
        a.slot0 = L.slot0;
        a.n = L.n;
        hipStream_t ls = (fan && L.lane > 0) ? t->side[L.lane - 1] : st;
        if (L.kind == 1) {
            const int64_t grid = (L.n + kBlock - 1) / kBlock;
            hipLaunchKernelGGL(reject_kernel, dim3(grid), dim3(kBlock), 0, ls, a, L.code);
            e = hipGetLastError();
        } else if (L.susp) {   // main + resume launch pair (plan_susp)
            KArgs b = a;
            b.susp_t = susp_t_env();
            b.susp_min = susp_min_env();
            b.susp_count = L.d_susp_count;
            b.susp_pi = L.d_susp_pi;
            b.susp_state = L.d_susp_state;
            b.susp_cap = L.susp_cap;
            e = hipMemsetAsync(L.d_susp_count, 0, sizeof(int32_t), ls);
            if (e == hipSuccess) e = launch_susp(L.N, L.nsoc, L.omax, L.lpp, L.flags(), L.oe, b, ls);
        } else if (want_jac) {   // (a Jacobian plan: dense rows or a streamed bucket's JAC copy, no hint)
            // (N >= 7: the case-4 streamed instances, units of their own)
            e = !L.stream ? launch_jac(L.N, L.nsoc, L.omax, L.lpp, a, ls)
                          : (L.N >= 7 ? launch_stream_c4_jac(L.N, L.nsoc, a, ls) : launch_stream_jac(L.N, L.nsoc, a, ls));
        } else if (L.stream) {   // a wave per pair: nothing to regroup, so no hint
            e = L.N >= 7 ? launch_stream_c4(L.N, L.nsoc, a, ls) : launch_stream(L.N, L.nsoc, a, ls);
        } else {
            const int split = (L.oe > 0 && L.lpp == 2 && split_enabled() && split_built(L.N, L.nsoc, L.omax, L.oe))
                                  ? LF_SPLIT : 0;
            KArgs b = a;
            if (hinted) {   // every solve bucket of the "one bucket" and "buckets" forms
                b.hint_r = hr.rd;
                b.hint_w = hr.wr;
                b.hint_ww = hint_waves();
                b.hint_wins = hint_windows(L.n, L.lpp, b.hint_ww);
                b.hint_tab_r = hr.tab_r;
                b.hint_tab_w = hr.tab_w;
                b.hint_tab0 = hr.tab0[lx];
                b.hint_blocks = hint_solve_blocks(b.hint_wins, b.hint_ww);
                b.hint_fw = hint_fill_windows();
            }
            e = launch_variant(L.N, L.nsoc, L.omax, L.lpp, L.flags() | fdonly | split, b, ls, L.oe);
        }
        if (e != hipSuccess) break;
    }
    if (e == hipSuccess && p->lay.fused()) {
        a.slot0 = 0;
        a.n = 0;
        e = p->lay.packed ? launch_packed(a, p->d_segs, (int)p->lay.segs.size(), p->lay.fused_blocks, st)
                          : launch_fused(a, p->d_segs, (int)p->lay.segs.size(), p->lay.fused_blocks, st);
    }
    if (fan) {   // join even after a failed launch, so the side streams never run ahead
        for (int l = 1; l < p->lay.lanes; ++l) {
            hipError_t j = hipEventRecord(p->join[l - 1], t->side[l - 1]);
            if (j == hipSuccess) j = hipStreamWaitEvent(st, p->join[l - 1], 0);
            if (e == hipSuccess) e = j;
        }
    }
    if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_plan_run launch: ") + hipGetErrorString(e));
    return DCOL_SUCCESS;
}
}  // namespace

extern "C" {

int dcol_plan_run(const dcol_plan* p, const double* pose1, const double* pose2, double tol, int32_t max_iter,
                  int32_t flags, double* alpha, double* contact, double* grad, int32_t* iters, int32_t* status,
                  void* stream) {
    return plan_run_rec(p, pose1, pose2, tol, max_iter, flags, alpha, contact, grad, iters, status, nullptr, stream);
}

int dcol_plan_run_jac(const dcol_plan* p, const double* pose1, const double* pose2, double tol, int32_t max_iter,
                      int32_t flags, double* alpha, double* contact, double* grad, double* jac, int32_t* iters,
                      int32_t* status, void* stream) {
    if (!p) return fail(DCOL_ERR_ARG, "dcol_plan_run_jac: NULL plan");
    const bool want = (flags & DCOL_JACOBIAN) != 0;
    if (want && !p->jac)
        return fail(DCOL_ERR_ARG, "dcol_plan_run_jac: DCOL_JACOBIAN needs a plan made with DCOL_PLAN_JACOBIAN");
    if (want && !jac) return fail(DCOL_ERR_ARG, "dcol_plan_run_jac: DCOL_JACOBIAN needs jac[]");
    return plan_run_rec(p, pose1, pose2, tol, max_iter, flags, alpha, contact, grad, iters, status, nullptr, stream,
                        true, true, want ? jac : nullptr);
}

int dcol_prox_pair(const dcol_table* tc, int32_t s1, int32_t s2, const double* pose1, const double* pose2, double tol,
                   int32_t max_iter, int32_t flags, double* alpha, double* contact, double* grad, int32_t* iters,
                   int32_t* status) {
    if (!tc || !pose1 || !pose2 || !alpha) return fail(DCOL_ERR_ARG, "dcol_prox_pair: NULL argument");
    if ((flags & DCOL_CONTACT) && !contact) return fail(DCOL_ERR_ARG, "dcol_prox_pair: DCOL_CONTACT needs contact");
    if ((flags & DCOL_GRAD_ANY) && !grad) return fail(DCOL_ERR_ARG, "dcol_prox_pair: gradient flag needs grad");
    if (max_iter < 0) return fail(DCOL_ERR_ARG, "dcol_prox_pair: max_iter < 0");
    const int32_t ns = (int32_t)tc->shapes.size();
    if (s1 < 0 || s1 >= ns || s2 < 0 || s2 >= ns) return fail(DCOL_ERR_ARG, "dcol_prox_pair: shape id out of range");
    dcol_table* t = const_cast<dcol_table*>(tc);
    std::lock_guard<std::mutex> lk(t->mu);
    DeviceGuard g(t->device);
    if (!t->pair_host) {
        // fine-grained coherent on purpose: the server's handshake (system-scope atomics on
        // req / done / alive / stop) needs host and device to see each other's stores while
        // the wave runs, whatever HIP_HOST_COHERENT says
        PairBox* hb = nullptr;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&hb), sizeof(PairBox),
                                     hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
        if (e == hipSuccess) {
            std::memset(hb, 0, sizeof(PairBox));   // flags and sequence numbers start at 0
            hb->xcd = -1;                           // no server yet
        }
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&t->pair_dev), hb, 0);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&t->pair_stream, hipStreamNonBlocking);
        // The server stream: a CU-masked stream (mask = every CU), because HIP never pools a
        // CU-masked stream into a shared hardware queue -- the resident server gets a queue of
        // its own instead of sharing one (GPU_MAX_HW_QUEUES, 4 by default) with the caller's
        // or the side streams, whose kernels would otherwise wait behind it until it idles
        // out.  Not a high-priority stream: a resident kernel on a high-priority queue slowed
        // a normal-priority 100k batch plan 1.7-1.8x whatever its poll rate, a normal or
        // CU-masked one by nothing measurable (tools/server_tax.py, profiles/r05_d/).
        // DCOL_PAIR_SERVER_STREAM=normal / high: those alternatives (A/B).
        const char* sk = std::getenv("DCOL_PAIR_SERVER_STREAM");
        if (e == hipSuccess && sk && (std::strcmp(sk, "normal") == 0 || std::strcmp(sk, "high") == 0)) {
            int prio_lo = 0, prio_hi = 0;
            if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) {
                (void)hipGetLastError();
                prio_lo = prio_hi = 0;
            }
            e = hipStreamCreateWithPriority(&t->server_stream, hipStreamNonBlocking,
                                            std::strcmp(sk, "high") == 0 ? prio_hi : prio_lo);
        } else if (e == hipSuccess) {
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus <= 0) {
                (void)hipGetLastError();
                cus = 256;
            }
            std::vector<uint32_t> mask((cus + 31) / 32, 0u);
            for (int c = 0; c < cus; ++c) mask[c / 32] |= 1u << (c % 32);
            e = hipExtStreamCreateWithCUMask(&t->server_stream, (uint32_t)mask.size(), mask.data());
        }
        int khz = 0;
        if (e == hipSuccess && hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, t->device) != hipSuccess) {
            (void)hipGetLastError();
            khz = 0;
        }
        if (e != hipSuccess) {   // (never published: nothing else has seen hb)
            if (hb) (void)hipHostFree(hb);
            if (t->pair_stream) (void)hipStreamDestroy(t->pair_stream);
            t->pair_dev = nullptr;
            t->pair_stream = nullptr;
            return fail(DCOL_ERR_HIP, std::string("dcol_prox_pair staging: ") + hipGetErrorString(e));
        }
        t->wall_ticks_us = khz > 0 ? (int64_t)khz / 1000 : 0;
        // published after its initialisation: yield_pair_servers reads it without t->mu
        __atomic_store_n(&t->pair_host, hb, __ATOMIC_RELEASE);
    }
    const int64_t key = (int64_t)s1 * ns + s2;
    // (DCOL_CASE4_STREAM implies DCOL_CASE4; both are host-call flags, stripped below)
    const bool c4s = (flags & DCOL_CASE4_STREAM) != 0;
    const bool c4 = c4s || (flags & DCOL_CASE4) != 0;
    flags &= ~(DCOL_CASE4 | DCOL_CASE4_STREAM);
    const int64_t nkeys = (int64_t)ns * ns;
    const int64_t ck = c4s ? -1 - nkeys - key : (c4 ? -1 - key : key);   // case-4 plans apart, streamed ones too
    dcol_plan* plan = nullptr;
    auto it = t->pair_plans.find(ck);
    if (it != t->pair_plans.end()) {
        t->pair_lru.splice(t->pair_lru.begin(), t->pair_lru, it->second);   // now the most recent
        plan = it->second->second;
    } else {
        const int rc = dcol_plan_create_ex(t, 1, &s1, &s2,
                                           c4s ? (DCOL_PLAN_CASE4 | DCOL_PLAN_CASE4_STREAM) : (c4 ? DCOL_PLAN_CASE4 : 0), &plan);
        if (rc != DCOL_SUCCESS) return rc;
        // the least recently used plan makes room (no launch of it is in flight: every call
        // synchronises its stream before returning)
        if ((int)t->pair_lru.size() >= DCOL_PAIR_PLANS_MAX) {
            t->pair_plans.erase(t->pair_lru.back().first);
            dcol_plan_destroy(t->pair_lru.back().second);
            t->pair_lru.pop_back();
        }
        t->pair_lru.emplace_front(ck, plan);
        t->pair_plans.emplace(ck, t->pair_lru.begin());
    }
    PairBox* h = t->pair_host;
    PairBox* d = t->pair_dev;
    // a batch launch asked the server to leave: drain it (it left at its next poll) and clear
    // the stop flag, so the server started below stays
    if (t->stop_req.exchange(false, std::memory_order_acq_rel) && !stop_pair_server(t, kServerStopMs))
        return fail(DCOL_ERR_HIP, "dcol_prox_pair: the pair server did not stop within 5 s");
    std::memcpy(h->pose1, pose1, 6 * sizeof(double));
    std::memcpy(h->pose2, pose2, 6 * sizeof(double));
    // SoA of one pair = the 6 values in order; the kernel reads / writes the mapped memory.
    const bool single = plan->launches.size() == 1 && plan->launches[0].kind == 0 && !plan->lay.fused() &&
                         !plan->launches[0].susp && plan->lay.lanes <= 1;
    // The one-pair server (PairBox, dcol_kernels_server.hip): a resident workgroup polls the
    // mailbox, so a call whose variant the fused kernel has (the server switches over the
    // same solver copies) costs no launch.
    const int idle_us = pair_server_idle_us();
    const Launch& L0 = plan->launches[0];
    int vid = (single && idle_us > 0 && t->wall_ticks_us > 0 && ns <= (1 << kPairBoxIdBits) && L0.lpp < 65536 &&
               !g_shutdown.load(std::memory_order_acquire))
                  ? fused_vid(L0.N, L0.nsoc, L0.omax, L0.lpp, L0.flags(), L0.oe) : -1;
    const int32_t kflags = flags & ~DCOL_CASE4;
    // Flags / tolerance / iteration cap are the server's launch arguments.  A call with others
    // while a server runs takes the launch path below, and only the second such call in a
    // row restarts the server with the new ones: an ALTRO loop switches between
    // proximity_mrp and proximity_gradient per phase (one launched call, then a restart), a
    // caller alternating the two call by call keeps the server for one of them instead of
    // restarting it at every call (47 us per call measured, against 32).
    bool restart = false;
    if (vid >= 0 && t->server_launched && (h->flags != kflags || h->tol != tol || h->max_iter != max_iter)) {
        if (hipStreamQuery(t->server_stream) == hipSuccess) {   // no server left: a fresh start
            __atomic_store_n(&h->alive, 0, __ATOMIC_SEQ_CST);
            t->srv_mismatch = 0;
        } else if (++t->srv_mismatch < 2) {
            vid = -1;
        } else {
            restart = true;
            t->srv_mismatch = 0;
        }
    } else if (vid >= 0) {
        t->srv_mismatch = 0;
    }
    if (vid >= 0) {
        const auto start_server = [&]() -> hipError_t {
            KArgs a;
            a.shapes = t->d_shapes;
            a.rows = t->d_rows;
            a.s1 = nullptr;   // the shape ids come with each request (PairBox::ids)
            a.s2 = nullptr;
            a.pose1 = d->pose1;
            a.pose2 = d->pose2;
            a.perm = nullptr;
            a.B = 1;
            a.slot0 = 0;
            a.n = 1;
            a.tol = tol;
            a.max_iter = max_iter;
            a.flags = kflags;
            a.alpha = &d->alpha;
            a.contact = d->contact;
            a.grad = d->grad;
            a.iters = &d->iters;
            a.status = &d->status;
            a.rec = nullptr;
            a.susp_t = 0;
            a.susp_min = 0;
            a.susp_count = nullptr;
            a.susp_pi = nullptr;
            a.susp_state = nullptr;
            a.susp_cap = 0;
#ifdef DCOL_STAMPS
            a.stamps = d->stamps;   // (diagnostic build) solve_one's phase stamps of each request
#endif
            h->flags = kflags;
            h->tol = tol;
            h->max_iter = max_iter;
            // a resident wave must not outlive the process's HIP context: stop every server
            // at exit (the handler runs before the HIP runtime's own, registered earlier)
            std::call_once(g_exit_hook, [] { std::atexit([] { (void)dcol_shutdown(); }); });
            if (!t->server_launched) g_server_tables.fetch_add(1, std::memory_order_acq_rel);
            t->server_launched = true;
            ++t->n_starts;
            const char* ps = std::getenv("DCOL_PAIR_SERVER_POLL_SLEEP");
            return launch_pair_server(a, d, (int64_t)idle_us * t->wall_ticks_us, ps ? std::atoi(ps) : 0, t->server_stream);
        };
        if (restart && !stop_pair_server(t, kServerStopMs))   // it leaves at its next poll, then start anew
            return fail(DCOL_ERR_HIP, "dcol_prox_pair: the pair server did not stop within 5 s");
        const uint32_t useq = (uint32_t)(h->req >> 32) + 1u;
        const int32_t seq = (int32_t)useq;
        h->ids = ((uint64_t)(useq & 0xffffu) << 48) | ((uint64_t)(uint32_t)s2 << kPairBoxIdBits) | (uint64_t)(uint32_t)s1;
        __atomic_store_n(&h->req, ((uint64_t)useq << 32) | ((uint64_t)(uint32_t)L0.lpp << 16) | (uint64_t)(uint32_t)vid,
                         __ATOMIC_SEQ_CST);
        // a server that cleared `alive` before this request re-checks `req` on its way out
        // (and serves it), or it is gone: then start one (a redundant one queues behind the
        // old one on the server stream, finds nothing to do and leaves after the idle time)
        if (__atomic_load_n(&h->alive, __ATOMIC_SEQ_CST) == 0) {
            const hipError_t e = start_server();
            if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_prox_pair server: ") + hipGetErrorString(e));
        }
        int restarts = 0;
        const auto t_post = std::chrono::steady_clock::now();
        for (uint64_t spin = 1;; ++spin) {
            if (__atomic_load_n(&h->done, __ATOMIC_ACQUIRE) == seq) break;
            if ((spin & 4095) == 0) {   // a failed server surfaces here; an idle stream with the request
                const hipError_t q = hipStreamQuery(t->server_stream);   // unserved gets a new server
                if (q == hipErrorNotReady && std::chrono::steady_clock::now() - t_post > std::chrono::seconds(30)) {
                    // a server that never answers (not expected: a solve takes microseconds):
                    // make it leave, so the next call starts clean, and report
                    (void)stop_pair_server(t, kServerStopMs);
                    return fail(DCOL_ERR_HIP, "dcol_prox_pair: the pair server did not answer within 30 s");
                }
                if (q == hipSuccess && __atomic_load_n(&h->done, __ATOMIC_ACQUIRE) != seq) {
                    const hipError_t e = ++restarts > 2 ? hipErrorLaunchFailure : start_server();
                    if (e != hipSuccess)
                        return fail(DCOL_ERR_HIP, std::string("dcol_prox_pair server: ") + hipGetErrorString(e));
                } else if (q != hipSuccess && q != hipErrorNotReady) {
                    return fail(DCOL_ERR_HIP, std::string("dcol_prox_pair server: ") + hipGetErrorString(q));
                }
            }
        }
        ++t->n_served;
        t->srv_us += (double)h->solve_ticks / (double)t->wall_ticks_us;
        t->srv_cycles += (double)h->solve_cycles;
        *alpha = h->alpha;
        if (contact && (flags & DCOL_CONTACT)) std::memcpy(contact, h->contact, 3 * sizeof(double));
        if (grad && (flags & DCOL_GRAD_ANY)) std::memcpy(grad, h->grad, 12 * sizeof(double));
        if (iters) *iters = h->iters;
        if (status) *status = h->status;
        return DCOL_SUCCESS;
    }
    // Otherwise one launch on the pair stream, synchronised.  (A completion flag released by
    // the kernel and polled here saved ~2.5 us per call, but its epilogue cost the one-lane
    // row-partitioned x polytope kernels 4-5 % of throughput; the server serves the latency
    // path now.)
    int rc = plan_run_rec(plan, d->pose1, d->pose2, tol, max_iter, flags & ~DCOL_CASE4, &d->alpha, d->contact,
                          d->grad, &d->iters, &d->status, nullptr, t->pair_stream, false, false);
    if (rc != DCOL_SUCCESS) return rc;
    ++t->n_launched;
    const hipError_t e = hipStreamSynchronize(t->pair_stream);
    if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_prox_pair: ") + hipGetErrorString(e));
    *alpha = h->alpha;
    if (contact && (flags & DCOL_CONTACT)) std::memcpy(contact, h->contact, 3 * sizeof(double));
    if (grad && (flags & DCOL_GRAD_ANY)) std::memcpy(grad, h->grad, 12 * sizeof(double));
    if (iters) *iters = h->iters;
    if (status) *status = h->status;
    return DCOL_SUCCESS;
}

int dcol_debug_pair_stamps(const dcol_table* tc, uint64_t out[16]) {
    if (!tc || !out) return fail(DCOL_ERR_ARG, "dcol_debug_pair_stamps: NULL argument");
#ifdef DCOL_STAMPS
    dcol_table* t = const_cast<dcol_table*>(tc);
    std::lock_guard<std::mutex> lk(t->mu);
    if (!t->pair_host) return fail(DCOL_ERR_ARG, "dcol_debug_pair_stamps: no pair call yet");
    for (int k = 0; k < 16; ++k) out[k] = __atomic_load_n(&t->pair_host->stamps[k], __ATOMIC_ACQUIRE);
    return DCOL_SUCCESS;
#else
    return fail(DCOL_ERR_ARG, "dcol_debug_pair_stamps: not a stamps build (make stamps)");
#endif
}

int dcol_table_stop_pair_server(const dcol_table* tc) {
    if (!tc) return fail(DCOL_ERR_ARG, "dcol_table_stop_pair_server: NULL table");
    dcol_table* t = const_cast<dcol_table*>(tc);
    std::lock_guard<std::mutex> lk(t->mu);
    DeviceGuard g(t->device);
    if (!stop_pair_server(t, kServerStopMs))
        return fail(DCOL_ERR_HIP, "dcol_table_stop_pair_server: the pair server did not stop within 5 s");
    return DCOL_SUCCESS;
}

int dcol_table_pair_server_running(const dcol_table* tc, int32_t* running) {
    if (!tc || !running) return fail(DCOL_ERR_ARG, "dcol_table_pair_server_running: NULL argument");
    dcol_table* t = const_cast<dcol_table*>(tc);
    std::lock_guard<std::mutex> lk(t->mu);
    DeviceGuard g(t->device);
    *running = 0;
    if (t->server_launched) {
        const hipError_t q = hipStreamQuery(t->server_stream);
        if (q == hipErrorNotReady)
            *running = 1;
        else if (q != hipSuccess)
            return fail(DCOL_ERR_HIP, std::string("dcol_table_pair_server_running: ") + hipGetErrorString(q));
    }
    return DCOL_SUCCESS;
}

int dcol_shutdown(void) {
    g_shutdown.store(true, std::memory_order_release);
    std::lock_guard<std::mutex> lk(g_tables_mu);
    int running = 0, stuck = 0;
    for (dcol_table* t : g_tables) {
        std::lock_guard<std::mutex> tl(t->mu);
        if (!t->server_launched) continue;
        DeviceGuard g(t->device);
        if (hipStreamQuery(t->server_stream) == hipErrorNotReady) ++running;
        (void)hipGetLastError();
        if (!stop_pair_server(t, kServerStopMs)) ++stuck;
    }
    if (const char* dbg = std::getenv("DCOL_DEBUG_SHUTDOWN"); dbg && *dbg && *dbg != '0')
        std::fprintf(stderr, "dcol_shutdown: %zu tables, %d pair servers running, %d stopped, %d did not stop\n",
                     g_tables.size(), running, running - stuck, stuck);
    return stuck ? fail(DCOL_ERR_HIP, "dcol_shutdown: a pair server did not stop within 5 s") : DCOL_SUCCESS;
}

int dcol_table_pair_plans(const dcol_table* tc, int32_t* n) {
    if (!tc || !n) return fail(DCOL_ERR_ARG, "dcol_table_pair_plans: NULL argument");
    dcol_table* t = const_cast<dcol_table*>(tc);
    std::lock_guard<std::mutex> lk(t->mu);
    *n = (int32_t)t->pair_lru.size();
    return DCOL_SUCCESS;
}

int dcol_table_pair_stats(const dcol_table* tc, int64_t* served, int64_t* launched, int64_t* server_starts,
                          double* server_solve_us, double* server_solve_cycles, int32_t* server_xcd) {
    if (!tc) return fail(DCOL_ERR_ARG, "dcol_table_pair_stats: NULL table");
    dcol_table* t = const_cast<dcol_table*>(tc);
    std::lock_guard<std::mutex> lk(t->mu);
    if (served) *served = t->n_served;
    if (launched) *launched = t->n_launched;
    if (server_starts) *server_starts = t->n_starts;
    if (server_solve_us) *server_solve_us = t->srv_us;
    if (server_solve_cycles) *server_solve_cycles = t->srv_cycles;
    if (server_xcd) *server_xcd = t->pair_host ? __atomic_load_n(&t->pair_host->xcd, __ATOMIC_ACQUIRE) : -1;
    return DCOL_SUCCESS;
}

#ifdef DCOL_CHECK_EXEC
// diagnostic build only (make check-exec; not in include/dcol.h): DPP reads from an
// inactive source lane counted over every kernel launched so far (tools/check_exec.py)
int dcol_debug_exec_violations(uint64_t* out, int32_t reset) {
    if (!out) return fail(DCOL_ERR_ARG, "dcol_debug_exec_violations: NULL out");
    (void)hipDeviceSynchronize();
    uint64_t total = 0;
#define DCOL_EXEC_SUM(tag) total += exec_violations_##tag(reset != 0);
    DCOL_EXEC_TAGS(DCOL_EXEC_SUM)
    DCOL_EXEC_SUM(capi)
#undef DCOL_EXEC_SUM
    *out = total;
    return DCOL_SUCCESS;
}
#endif

#ifdef DCOL_CHECK_EXEC
}  // extern "C"
namespace dcol {
// positive control of the DPP-source check: in each wave the odd lanes leave, then the even
// lanes take a 2-lane group sum whose partner lane is inactive -- 32 counted reads per wave
__global__ void __launch_bounds__(64) exec_selftest_kernel(double* out) {
    const int l = (int)threadIdx.x;
    if (l & 1) return;
    out[l] = Grp<2>::sum((double)l);
}
DCOL_EXEC_READER(capi)
}  // namespace dcol
extern "C" {
int dcol_debug_exec_selftest(uint64_t* counted) {
    if (!counted) return fail(DCOL_ERR_ARG, "dcol_debug_exec_selftest: NULL out");
    double* d = nullptr;
    if (hipMalloc(&d, 64 * sizeof(double)) != hipSuccess) return fail(DCOL_ERR_HIP, "selftest alloc");
    (void)exec_violations_capi(true);
    hipLaunchKernelGGL(exec_selftest_kernel, dim3(1), dim3(64), 0, 0, d);
    (void)hipDeviceSynchronize();
    *counted = exec_violations_capi(true);
    (void)hipFree(d);
    return DCOL_SUCCESS;
}
#endif

// dcol_prox_batch_host, and with jac (host [B][4][12]) dcol_prox_jacobian_host: the same
// staging with 48 B more output doubles behind the gradient, a DCOL_PLAN_JACOBIAN layout
// (DCOL_JACOBIAN_STREAM in flags: with DCOL_PLAN_JACOBIAN_STREAM)
static int prox_batch_host(const dcol_table* tc, int64_t B, const int32_t* s1, const int32_t* s2, const double* pose1,
                           const double* pose2, double tol, int32_t max_iter, int32_t flags, double* alpha,
                           double* contact, double* grad, double* jac, int32_t* iters, int32_t* status) {
    if (!tc || B < 0) return fail(DCOL_ERR_ARG, "dcol_prox_batch_host: bad arguments");
    if (B == 0) return DCOL_SUCCESS;
    if (!s1 || !s2 || !pose1 || !pose2 || !alpha) return fail(DCOL_ERR_ARG, "dcol_prox_batch_host: NULL array");
    if (B > INT32_MAX) return fail(DCOL_ERR_ARG, "dcol_prox_batch_host: B exceeds 2^31-1");
    dcol_table* t = const_cast<dcol_table*>(tc);
    std::lock_guard<std::mutex> lk(t->mu);
    dcol_plan p;   // transient, device arrays are views into the table's staging buffer
    // (DCOL_JACOBIAN_STREAM: a host-call flag like DCOL_CASE4, not a kernel flag)
    const bool jac_stream = jac != nullptr && (flags & DCOL_JACOBIAN_STREAM) != 0;
    flags &= ~DCOL_JACOBIAN_STREAM;
    // (DCOL_CASE4_STREAM: likewise; it implies DCOL_CASE4)
    const bool case4_stream = (flags & DCOL_CASE4_STREAM) != 0;
    const bool case4 = case4_stream || (flags & DCOL_CASE4) != 0;
    flags &= ~DCOL_CASE4_STREAM;
    int rc = plan_build(t, B, s1, s2, case4, true, &p, jac != nullptr, jac_stream, case4_stream);
    if (rc != DCOL_SUCCESS) return rc;
    rc = ensure_fanout(t, &p);
    if (rc != DCOL_SUCCESS) return rc;
    DeviceGuard g(t->device);
    // staging: doubles pose1[6B] pose2[6B] | alpha[B] contact[3B] grad[12B] ; fused segments ;
    // ints s1 s2 perm iters status
    const size_t nin = (size_t)12 * B, nout = (size_t)(jac ? 64 : 16) * B;
    const size_t segb = sizeof(FusedSeg) * p.lay.segs.size();
    const size_t bytes = (nin + nout) * sizeof(double) + segb + 5 * (size_t)B * sizeof(int32_t);
    if (t->stage_bytes < bytes) {
        if (t->stage) (void)hipFree(t->stage);
        t->stage = nullptr;
        t->stage_bytes = 0;
        hipError_t e = hipMalloc(&t->stage, bytes);
        if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_prox_batch_host staging: ") + hipGetErrorString(e));
        t->stage_bytes = bytes;
    }
    double* dp1 = static_cast<double*>(t->stage);
    double* dp2 = dp1 + 6 * B;
    double* dal = dp1 + nin;
    double* dct = dal + B;
    double* dgr = dct + 3 * B;
    double* djc = jac ? dgr + 12 * B : nullptr;
    FusedSeg* dsg = reinterpret_cast<FusedSeg*>(dp1 + nin + nout);
    p.d_segs = p.lay.fused() ? dsg : nullptr;
    int32_t* ib = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(dsg) + segb);
    p.d_s1 = ib;
    p.d_s2 = ib + B;
    p.d_perm = p.launches.size() > 1 ? ib + 2 * B : nullptr;
    int32_t* dit = ib + 3 * B;
    int32_t* dst = ib + 4 * B;
    // pinned host staging (DMA at full link rate): [pose soa (12B) | outputs (16B)] doubles,
    // then [s1 | s2 | perm | iters | status] ints
    const size_t hbytes = (nin + nout) * sizeof(double) + 5 * (size_t)B * sizeof(int32_t);
    if (t->hstage_bytes < hbytes) {
        if (t->hstage) (void)hipHostFree(t->hstage);
        t->hstage = nullptr;
        t->hstage_bytes = 0;
        hipError_t e = hipHostMalloc(&t->hstage, hbytes, hipHostMallocDefault);
        if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_prox_batch_host pinned staging: ") + hipGetErrorString(e));
        t->hstage_bytes = hbytes;
    }
    double* soa = static_cast<double*>(t->hstage);
    double* outd = soa + nin;
    int32_t* ids = reinterpret_cast<int32_t*>(outd + nout);
    for (int64_t i = 0; i < B; ++i)
        for (int q = 0; q < 6; ++q) {
            soa[q * B + i] = pose1[6 * i + q];
            soa[(6 + q) * B + i] = pose2[6 * i + q];
        }
    std::memcpy(ids, s1, sizeof(int32_t) * B);
    std::memcpy(ids + B, s2, sizeof(int32_t) * B);
    std::memcpy(ids + 2 * B, p.lay.perm.data(), sizeof(int32_t) * B);
    // one H2D copy: [pose1 soa | pose2 soa] then [s1 | s2 | perm]
    hipError_t e = hipMemcpy(dp1, soa, sizeof(double) * nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ib, ids, sizeof(int32_t) * 3 * B, hipMemcpyHostToDevice);
    if (e == hipSuccess && segb) e = hipMemcpy(dsg, p.lay.segs.data(), segb, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_prox_batch_host H2D: ") + hipGetErrorString(e));
    rc = plan_run_rec(&p, dp1, dp2, tol, max_iter, flags, dal, dct, dgr, dit, dst, nullptr, nullptr, true, false, djc);
    if (rc != DCOL_SUCCESS) return rc;
    e = hipMemcpy(outd, dal, sizeof(double) * nout, hipMemcpyDeviceToHost);   // synchronises
    if (e == hipSuccess) e = hipMemcpy(ids + 3 * B, dit, sizeof(int32_t) * 2 * B, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("dcol_prox_batch_host D2H: ") + hipGetErrorString(e));
    if (iters) std::memcpy(iters, ids + 3 * B, sizeof(int32_t) * B);
    if (status) std::memcpy(status, ids + 4 * B, sizeof(int32_t) * B);
    std::memcpy(alpha, outd, sizeof(double) * B);
    if (contact && (flags & DCOL_CONTACT))
        for (int64_t i = 0; i < B; ++i)
            for (int q = 0; q < 3; ++q) contact[3 * i + q] = outd[(size_t)B + q * B + i];
    if (grad && (flags & DCOL_GRAD_ANY))
        for (int64_t i = 0; i < B; ++i)
            for (int q = 0; q < 12; ++q) grad[12 * i + q] = outd[(size_t)4 * B + q * B + i];
    if (jac)
        for (int64_t i = 0; i < B; ++i)
            for (int q = 0; q < 48; ++q) jac[48 * i + q] = outd[(size_t)16 * B + q * B + i];
    return DCOL_SUCCESS;
}

int dcol_prox_batch_host(const dcol_table* tc, int64_t B, const int32_t* s1, const int32_t* s2, const double* pose1,
                         const double* pose2, double tol, int32_t max_iter, int32_t flags, double* alpha,
                         double* contact, double* grad, int32_t* iters, int32_t* status) {
    return prox_batch_host(tc, B, s1, s2, pose1, pose2, tol, max_iter, flags, alpha, contact, grad, nullptr, iters,
                           status);
}

int dcol_prox_jacobian_host(const dcol_table* tc, int64_t B, const int32_t* s1, const int32_t* s2, const double* pose1,
                            const double* pose2, double tol, int32_t max_iter, int32_t flags, double* alpha,
                            double* contact, double* grad, double* jac, int32_t* iters, int32_t* status) {
    if (!jac && B > 0) return fail(DCOL_ERR_ARG, "dcol_prox_jacobian_host: jac is required");
    if ((flags & DCOL_CONTACT) && !contact) return fail(DCOL_ERR_ARG, "dcol_prox_jacobian_host: DCOL_CONTACT needs contact");
    if ((flags & DCOL_GRAD_ANY) && !grad) return fail(DCOL_ERR_ARG, "dcol_prox_jacobian_host: gradient flag needs grad");
    return prox_batch_host(tc, B, s1, s2, pose1, pose2, tol, max_iter, flags, alpha, contact, grad, jac, iters, status);
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// multi-GPU: one all-gather of the packed per-pair record (include/dcol.h).
// RCCL is resolved with dlopen on first use, so libdcol.so itself has no link-time
// dependency on it (single-GPU users never load it).
// ------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {

struct Rccl {
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) init_rank = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    bool ok = false;
};

// The collective library: librccl, or the one DCOL_RCCL_LIB names (a test stand-in with
// the same five entry points, tests/fake_rccl/), resolved per library path on first use
const Rccl& rccl() {
    static std::mutex mu;
    static std::map<std::string, Rccl> libs;
    const char* env = std::getenv("DCOL_RCCL_LIB");
    const std::string path = (env && *env) ? env : "";
    std::lock_guard<std::mutex> lk(mu);
    auto it = libs.find(path);
    if (it != libs.end()) return it->second;
    Rccl x;
    void* h = nullptr;
    if (!path.empty()) {
        h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    } else {
        h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    }
    if (h) {
        x.get_unique_id = reinterpret_cast<decltype(&ncclGetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
        x.init_rank = reinterpret_cast<decltype(&ncclCommInitRank)>(dlsym(h, "ncclCommInitRank"));
        x.destroy = reinterpret_cast<decltype(&ncclCommDestroy)>(dlsym(h, "ncclCommDestroy"));
        x.all_gather = reinterpret_cast<decltype(&ncclAllGather)>(dlsym(h, "ncclAllGather"));
        x.error_string = reinterpret_cast<decltype(&ncclGetErrorString)>(dlsym(h, "ncclGetErrorString"));
        x.ok = x.get_unique_id && x.init_rank && x.destroy && x.all_gather && x.error_string;
    }
    return libs.emplace(path, x).first->second;   // std::map: references stay valid
}

std::string rccl_error(const Rccl& api, ncclResult_t r) {
    return api.error_string ? api.error_string(r) : std::to_string((int)r);
}

}  // namespace

struct dcol_comm {
    const Rccl* api = nullptr;   // the library the communicator was made with
    ncclComm_t comm = nullptr;
    int32_t nranks = 0, rank = 0, device = 0;
};

namespace dcol {
// rec[i] = [alpha, grad(12), (int32 status, int32 iters)] (dcol_amd/dist.py REC layout);
// rows >= n NaN.
// A block packs kPackRows records: each thread gathers one record's fields from the SoA
// outputs (coalesced reads) into LDS, then the block streams the contiguous
// kPackRows * DCOL_REC doubles out with consecutive threads on consecutive addresses
// (coalesced writes; a record-per-thread store pattern strides 120 B per lane).
constexpr int kPackRows = 256;
__global__ void __launch_bounds__(kPackRows) pack_records(int64_t n, int64_t cap, const double* alpha,
                                                          const double* grad, const int32_t* iters,
                                                          const int32_t* status, double* rec) {
    __shared__ double tile[kPackRows * DCOL_REC];
    const int64_t r0 = (int64_t)blockIdx.x * kPackRows;
    const int64_t i = r0 + threadIdx.x;
    const double nan = __builtin_nan("");
    double* o = tile + DCOL_REC * threadIdx.x;
    if (i < n) {
        o[0] = alpha[i];
#pragma unroll
        for (int c = 0; c < 12; ++c) o[1 + c] = grad ? grad[c * n + i] : nan;
        // the int32 pair in one 8-byte slot (status low, iters high: little-endian)
        o[13] = __longlong_as_double((long long)(((unsigned long long)(unsigned)iters[i] << 32) |
                                                 (unsigned long long)(unsigned)status[i]));
    } else {
#pragma unroll
        for (int c = 0; c < DCOL_REC; ++c) o[c] = nan;
    }
    __syncthreads();
    const int64_t rows = (cap - r0) < kPackRows ? (cap - r0) : kPackRows;
    double* dst = rec + DCOL_REC * r0;
    for (int64_t e = threadIdx.x; e < rows * DCOL_REC; e += kPackRows) dst[e] = tile[e];
}
}  // namespace dcol

extern "C" {

int dcol_comm_unique_id(uint8_t id[DCOL_COMM_ID_BYTES]) {
    if (!id) return fail(DCOL_ERR_ARG, "dcol_comm_unique_id: id is NULL");
    const Rccl& api = rccl();
    if (!api.ok) return fail(DCOL_ERR_HIP, "dcol_comm_unique_id: librccl not loadable");
    ncclUniqueId u;
    ncclResult_t r = api.get_unique_id(&u);
    if (r != ncclSuccess) return fail(DCOL_ERR_HIP, "ncclGetUniqueId: " + rccl_error(api, r));
    static_assert(sizeof(u.internal) == DCOL_COMM_ID_BYTES, "unique id size");
    std::memcpy(id, u.internal, DCOL_COMM_ID_BYTES);
    return DCOL_SUCCESS;
}

int dcol_comm_create(const uint8_t id[DCOL_COMM_ID_BYTES], int32_t nranks, int32_t rank, int32_t device,
                     dcol_comm** out) {
    if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks || device < 0)
        return fail(DCOL_ERR_ARG, "dcol_comm_create: bad arguments");
    *out = nullptr;
    const Rccl& api = rccl();
    if (!api.ok) return fail(DCOL_ERR_HIP, "dcol_comm_create: librccl not loadable");
    DeviceGuard g(device);
    ncclUniqueId u;
    std::memcpy(u.internal, id, DCOL_COMM_ID_BYTES);
    auto* c = new (std::nothrow) dcol_comm();
    if (!c) return fail(DCOL_ERR_NOMEM, "dcol_comm_create");
    c->api = &api;
    ncclResult_t r = api.init_rank(&c->comm, nranks, u, rank);
    if (r != ncclSuccess) {
        delete c;
        return fail(DCOL_ERR_HIP, "ncclCommInitRank: " + rccl_error(api, r));
    }
    c->nranks = nranks;
    c->rank = rank;
    c->device = device;
    *out = c;
    return DCOL_SUCCESS;
}

int dcol_comm_destroy(dcol_comm* c) {
    if (!c) return DCOL_SUCCESS;
    if (c->comm) (void)c->api->destroy(c->comm);
    delete c;
    return DCOL_SUCCESS;
}

int dcol_prox_batch_multi_gpu(const dcol_plan* p, dcol_comm* c, const double* pose1, const double* pose2, double tol,
                              int32_t max_iter, int32_t flags, int64_t cap, double* alpha, double* grad,
                              int32_t* iters, int32_t* status, double* rec_local, double* rec_all, void* stream) {
    if (!p || !c || !rec_all || (rec_local && (!alpha || !iters || !status)))
        return fail(DCOL_ERR_ARG, "dcol_prox_batch_multi_gpu: NULL argument");
    if (cap < p->B) return fail(DCOL_ERR_ARG, "dcol_prox_batch_multi_gpu: cap < shard size");
    if (p->table->device != c->device)
        return fail(DCOL_ERR_ARG, "dcol_prox_batch_multi_gpu: plan and communicator on different devices");
    const bool gather = (flags & DCOL_NO_GATHER) == 0;
    if (!gather && rec_local) return fail(DCOL_ERR_ARG, "dcol_prox_batch_multi_gpu: DCOL_NO_GATHER is in place only");
    const int32_t rflags = flags & ~(DCOL_CONTACT | DCOL_NO_GATHER);   // the record carries no contact point
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!rec_local) {
        // in place: the solver epilogues write this rank's records straight into its slice of
        // rec_all (no pack pass, no local copy inside the all-gather); rows past the shard
        // are all-ones bytes (NaN doubles, int pair (-1, -1))
        double* mine = rec_all + (size_t)c->rank * (size_t)cap * DCOL_REC;
        int rc = plan_run_rec(p, pose1, pose2, tol, max_iter, rflags, alpha, nullptr,
                              (rflags & DCOL_GRAD_ANY) ? grad : nullptr, iters, status, mine, stream);
        if (rc != DCOL_SUCCESS) return rc;
        DeviceGuard g(c->device);
        if (cap > p->B) {
            const hipError_t e = hipMemsetAsync(mine + (size_t)p->B * DCOL_REC, 0xFF,
                                                (size_t)(cap - p->B) * DCOL_REC * sizeof(double), st);
            if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("record tail: ") + hipGetErrorString(e));
        }
        if (!gather) return DCOL_SUCCESS;
        ncclResult_t r = c->api->all_gather(mine, rec_all, (size_t)cap * DCOL_REC, ncclDouble, c->comm, st);
        if (r != ncclSuccess) return fail(DCOL_ERR_HIP, "ncclAllGather: " + rccl_error(*c->api, r));
        return DCOL_SUCCESS;
    }
    int rc = dcol_plan_run(p, pose1, pose2, tol, max_iter, rflags, alpha, nullptr,
                           (rflags & DCOL_GRAD_ANY) ? grad : nullptr, iters, status, stream);
    if (rc != DCOL_SUCCESS) return rc;
    DeviceGuard g(c->device);
    const bool want_grad = (rflags & DCOL_GRAD_ANY) && grad;
    if (cap > 0) {
        const int64_t grid = (cap + kPackRows - 1) / kPackRows;
        hipLaunchKernelGGL(pack_records, dim3(grid), dim3(kPackRows), 0, st, p->B, cap, alpha, want_grad ? grad : nullptr,
                           iters, status, rec_local);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(DCOL_ERR_HIP, std::string("pack_records: ") + hipGetErrorString(e));
    }
    ncclResult_t r = c->api->all_gather(rec_local, rec_all, (size_t)cap * DCOL_REC, ncclDouble, c->comm, st);
    if (r != ncclSuccess) return fail(DCOL_ERR_HIP, "ncclAllGather: " + rccl_error(*c->api, r));
    return DCOL_SUCCESS;
}

int dcol_comm_all_gather(dcol_comm* c, int64_t cap, double* rec_all, void* stream) {
    if (!c || !rec_all || cap < 0) return fail(DCOL_ERR_ARG, "dcol_comm_all_gather: bad arguments");
    DeviceGuard g(c->device);
    double* mine = rec_all + (size_t)c->rank * (size_t)cap * DCOL_REC;
    ncclResult_t r = c->api->all_gather(mine, rec_all, (size_t)cap * DCOL_REC, ncclDouble, c->comm,
                                        reinterpret_cast<hipStream_t>(stream));
    if (r != ncclSuccess) return fail(DCOL_ERR_HIP, "ncclAllGather: " + rccl_error(*c->api, r));
    return DCOL_SUCCESS;
}

}  // extern "C"
