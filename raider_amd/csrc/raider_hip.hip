// libraider_hip.so - C ABI (include/raider_hip.h) + the remaining kernels.  gfx950 only.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC raider_hip.hip -o libraider_hip.so
// Every launcher of a kernel templated on the cube's element type (the point path, the two ray passes, the cube build) picks it with by_dtype
// (beside launch_lds); two cubes' grids are compared with same_grid_dtype (above rdr_cube_blend); the gathers' one device body is gather_points
// (cube_kernels.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/raider_hip.h"
#include "raider_kernels.h"

using namespace rdr;

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

constexpr int MAX_SLICES = 512;   // height slices per rdr_raytrace_slices call

enum { SLOT_IN0 = 0, SLOT_IN1, SLOT_IN2, SLOT_IN3, SLOT_IN4, SLOT_IN5, SLOT_IN6, SLOT_OUT0, SLOT_OUT1, SLOT_OUT2, SLOT_AUX,
       SLOT_PT0, SLOT_PT1, SLOT_PT2, SLOT_PT3, SLOT_PT4, SLOT_PT5, SLOT_TMPCUBE, SLOT_TMPAXES,      // rdr_point_delays: points, delays, the intermediate cube
       SLOT_DEFL, SLOT_DEFL_TOK,                                                                     // rdr_deflate_encode: the sub-blocks' slots; the workgroups' token scratch
       NSLOT };

struct rdr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t copy_stream = nullptr;      // host<->device transfers of the pipelined host-buffer ray tracing
    hipStream_t down_stream = nullptr;      // downloads that run under the uploads of the next chunk (rdr_point_delays)
    hipStream_t stream = nullptr;
    int num_cus = 256;
    size_t lds_max = 64u << 10;             // largest dynamic LDS allocation of one workgroup
    size_t total_mem = 0;
    std::string name;
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evs[4];   // HIP event pairs around every launch, per kernel kind
    size_t ev_used[4] = {0, 0, 0, 0};
    DevBuf slot[NSLOT];
    unsigned long long* d_maxlen = nullptr;   // [MAX_SLICES][MAX_LEVELS]
    int* d_flags = nullptr;                   // [MAX_SLICES]
    int* d_nparts = nullptr;                  // [MAX_LEVELS] (rdr_ray_march's host-given partition)
    int* d_nslow = nullptr;                   // [2] rays sent to the generic kernels by the last pass 1; waves of it that skipped the level loop
    int* d_tilectr = nullptr;                 // [4][8] per-XCD tile counters of the four ray-kernel launches of a step
    // value buffers of destroyed cubes, kept for the next cube of the same size: a job that blends / builds a cube per date or per call
    // (cli/raider.py:817-819, the intermediate cubes of the point branch) then allocates nothing - hipMalloc + hipFree of a 400 MB cube
    // are 0.2 ms of host time AND a device-wide synchronisation.  A buffer is handed on with the event recorded when its cube died.
    struct PoolEntry { void* p; size_t bytes; std::vector<hipEvent_t> evs; };   // one event per stream the context has launched on
    std::vector<PoolEntry> cube_pool;
    std::vector<hipStream_t> ext_streams;     // caller streams handed to rdr_set_stream so far (a cube may still be read on any of them)
    bool ext_overflow = false;                // more than 8 of them: destroyed cubes are freed synchronously instead of pooled
    size_t cube_pool_bytes = 0, cube_pool_limit = (size_t)4 << 30;
    DevBuf ws;                                // pass 1 -> pass 2 workspace (field-major ray records, 232 B per ray)
    DevBuf side;                              // level crossings of the generic rays (compact columns of K+1 doubles)
    int64_t side_cap = 0;                     // columns of `side` in the current layout
    DevBuf lev;                               // level table of pass 2: [nslices][nz + 1] LevelRec (level_table_kernel)
    int* d_sidectr = nullptr;                 // [1] next free column
    // the one-kernel ray route (trace_one_pass)
    int* d_onepass = nullptr;                 // [OP_WORDS] its device state (RayParams::one_pass)
    DevBuf probe;                             // tile list of its probe, kept while the scene's tiling and the stream stay what they were
    struct { int tiles_x = 0; int64_t tiles_y = 0; hipStream_t stream = nullptr; int64_t count = 0; } probe_key;
    DevBuf gridtrig;                          // sines / cosines of the batch's latitudes and longitudes (grid_trig_kernel)
    int64_t one_pass_calls = 0;               // calls that took the route
    int64_t one_pass_redos = 0;               // ... whose classic passes ran, as of the last partition the host read back
    int* h_word = nullptr;                    // [16] page-locked host words: flags read back WITHOUT stalling the host before the final sync
    // Small host inputs (axes, level lists, a cube's three axes) go up through a ring of page-locked buffers: the caller's array is consumed by a
    // memcpy before the call returns and the device copy is REALLY asynchronous (from pageable memory hipMemcpyAsync first waits for everything
    // queued on the stream - ADVICE r5).  A slot is reused only after the event recorded behind its last copy.
    struct PinSlot { void* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
    static constexpr int PIN_SLOTS = 16;
    static constexpr size_t PIN_MAX = (size_t)1 << 20;
    PinSlot pin[PIN_SLOTS];
    int pin_next = 0;
    hipEvent_t staged_ev = nullptr;           // recorded behind a LARGE host input's copy and waited for: the source is consumed when the entry returns
    // cubes made from DEVICE sources are created without a host synchronisation (round 5): their NaN verdict lands in one of these page-locked
    // words and is read when somebody asks (rdr_cube_has_nan), after the cube's ready event; nan_owner[i] = the cube word i is pending for
    static constexpr int NAN_SLOTS = 256;
    int* nan_words = nullptr;
    const struct rdr_cube* nan_owner[NAN_SLOTS] = {};
    int nan_next = 0;
    int64_t side_forced = -1;                 // rdr_set_side_capacity
    int64_t last_nskip = 0;                   // waves of the last rdr_ray_prepass that skipped the per-level length loop
    int64_t last_nslow = 0;                   // generic rays seen by the last pass 1 whose count the host happened to read back
    int wall_khz = 0;                         // rate of the wall counter (rdr_clock_sample_begin)
    int64_t point_upload_bytes = 0;           // host bytes of query points / divisors the last rdr_*_epochs point call copied up (rdr_point_upload_bytes)
    int last_nan_output = -1;                 // rdr_build_cube (host arrays): 1 / 0 = its last result holds / does not hold a NaN; -1 unknown
    size_t ws_limit = (size_t)48 << 30;       // cap on that workspace; bigger batches are marched in chunks
    // which ray batch the stored records belong to (a later rdr_ray_march reuses them only for the identical batch)
    struct { const void* cube = nullptr; const void* vals = nullptr; LccParams proj = {0, 0, 0, 0, 0, 0, 0, 0}; int64_t n = -1; double ht = 0, zref = 0; const void* a = nullptr; const void* b = nullptr; const void* c = nullptr; const void* d = nullptr; int K = 0; bool valid = false; } wsig;
    std::string err;
};

struct rdr_cube {
    rdr_ctx* ctx = nullptr;
    int64_t ny = 0, nx = 0, nz = 0;
    int dtype = RDR_F32;
    void* d_vals = nullptr;     // interleaved (wet,hydro), (y,x,z) z fastest
    double* d_axes = nullptr;   // ys | xs | zs ascending
    std::vector<double> ys, xs, zs;
    int uni[3] = {0, 0, 0};
    int exact[2] = {0, 0};
    double inv_d[3] = {0, 0, 0};
    LccParams proj = {0, 0, 0, 0, 0, 0, 0, 0};   // kind 0: the cube axes are lon/lat degrees
    // corner-quad copy for large random point sets (cube_kernels.h): built on demand, owned by the cube
    mutable void* d_quad = nullptr;
    mutable size_t quad_bytes = 0;
    mutable int quad_nblk = 0;
    mutable int big_point_calls = 0;             // rdr_interp3 calls that would have profited
    mutable std::mutex quad_mutex;               // one builder of the quad copy per cube
    mutable bool has_nan = false;                // a NaN among the fields (seen while packing; blends: either source's)
    // asynchronous creation (device sources): `ready_ev` is recorded on `ready_stream` after the last kernel that writes the buffers; any use
    // on another stream waits for it (cube_wait); nan_slot >= 0: the packing kernel's verdict is still in ctx->nan_words[nan_slot]
    mutable hipEvent_t ready_ev = nullptr;
    hipStream_t ready_stream = nullptr;
    mutable int nan_slot = -1;
    size_t alloc_bytes = 0;                      // bytes of the ONE allocation behind d_vals (values | axes); 0: not owned (scratch cube, view)
    // views (rdr_cube_view): `base` != NULL marks a handle that shares base's buffers and corner-quad copy and owns only its projection
    const rdr_cube* base = nullptr;
    mutable int views = 0;                       // live views of THIS cube (guarded by g_view_mutex)
    mutable bool doomed = false;                 // destroyed while views were alive: the last view frees the buffers
    mutable std::atomic<bool> foreign{false};    // used from a context other than its own: its buffers are freed synchronously, never pooled
    // caller streams (rdr_set_stream) this cube was read or written on: its buffers are pooled behind events on THESE streams, not on every
    // stream the context ever saw (guarded by g_view_mutex; last_stream: the common case - the same stream again - without the lock)
    mutable std::vector<hipStream_t> used_streams;
    mutable std::atomic<hipStream_t> last_stream{nullptr};
};
// One lock for the state that a cube shares with its OWNING context and that another context's thread may touch (a cube is usable from any
// context): view counts, the pending-NaN-verdict slots (nan_owner) and the pool of buffers of destroyed cubes.  Recursive: settling a verdict
// happens inside a creation.
static std::recursive_mutex g_view_mutex;
static inline const rdr_cube* root(const rdr_cube* q) { return q->base ? q->base : q; }
// every entry point that reads a cube says so: work enqueued by ANOTHER context is not covered by the events the owner records at destroy
static inline void note_use(const rdr_ctx* c, const rdr_cube* q) {
    if (!c || !q) return;
    const rdr_cube* r = root(q);
    if (r->ctx != c) r->foreign.store(true, std::memory_order_relaxed);
    if (r->last_stream.load(std::memory_order_relaxed) != c->stream) {
        std::lock_guard<std::recursive_mutex> guard(g_view_mutex);
        if (std::find(r->used_streams.begin(), r->used_streams.end(), c->stream) == r->used_streams.end()) r->used_streams.push_back(c->stream);
        r->last_stream.store(c->stream, std::memory_order_relaxed);
    }
    // a cube created asynchronously on another stream: this stream's work is ordered after its completion
    if (r->ready_ev && r->ready_stream != c->stream) { (void)hipStreamWaitEvent(c->stream, r->ready_ev, 0); (void)hipGetLastError(); }
}
// the pending NaN verdict of an asynchronously created cube (waits for the cube's ready event: the only host wait of such a cube)
static void cube_resolve_nan(const rdr_cube* r) {
    std::lock_guard<std::recursive_mutex> guard(g_view_mutex);         // (a cube may be asked from two contexts' threads at once)
    if (r->nan_slot < 0) return;
    rdr_ctx* c = r->ctx;
    if (r->ready_ev) (void)hipEventSynchronize(r->ready_ev);
    r->has_nan = c->nan_words[r->nan_slot] != 0;
    c->nan_owner[r->nan_slot] = nullptr;
    r->nan_slot = -1;
}


static int fail(rdr_ctx* ctx, int code, const std::string& msg) {
    g_err = msg;
    if (ctx) ctx->err = msg;
    return code;
}

#define HIPCHECK(ctx, expr)                                                                         \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            (void)hipGetLastError();   /* reported here: a later launch check must not find it again */ \
            return fail(ctx, _e == hipErrorOutOfMemory ? RDR_ERR_OOM : RDR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
        }                                                                                           \
    } while (0)

// mark `q` complete-on-stream: everything enqueued on c->stream so far finishes before any other stream touches it
static int cube_mark_ready(rdr_ctx* c, rdr_cube* q) {
    HIPCHECK(c, hipEventCreateWithFlags(&q->ready_ev, hipEventDisableTiming));
    HIPCHECK(c, hipEventRecord(q->ready_ev, c->stream));
    q->ready_stream = c->stream;
    return RDR_OK;
}

static void pool_drain(rdr_ctx* c);
// hipMalloc that, when the device is out of memory, first gives back what the context itself is hoarding - the pooled buffers of destroyed
// cubes (up to 4 GiB) - and tries once more: a job that would fit must not fail on the library's own cache.
static int dev_malloc(rdr_ctx* ctx, void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && !ctx->cube_pool.empty()) {
        (void)hipGetLastError();
        pool_drain(ctx);
        e = hipMalloc(p, bytes);
    }
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); *p = nullptr; return fail(ctx, RDR_ERR_OOM, "out of device memory (" + std::to_string(bytes >> 20) + " MiB asked)"); }
    if (e != hipSuccess) { *p = nullptr; return fail(ctx, RDR_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    return RDR_OK;
}

// `b` holds at least `bytes` (a new allocation: at least min_cap).  Too small: the context stream is waited for - work on it may still
// use the old buffer -, the old buffer is freed, the new one allocated, in that order (the device never holds both).
static int grow(rdr_ctx* ctx, DevBuf& b, size_t bytes, size_t min_cap = 0) {
    if (b.cap >= bytes) return RDR_OK;
    if (b.p) { HIPCHECK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHECK(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    const size_t cap = std::max(bytes, min_cap);
    const int rc = dev_malloc(ctx, &b.p, cap); if (rc) return rc;
    b.cap = cap;
    return RDR_OK;
}

static int ensure(rdr_ctx* ctx, int s, size_t bytes, void** out) {
    DevBuf& b = ctx->slot[s];
    if (bytes > ((size_t)1 << 46)) return fail(ctx, RDR_ERR_INVALID, "a size argument is negative or beyond 64 TiB");
    const int rc = grow(ctx, b, bytes, (size_t)1 << 16); if (rc) return rc;
    *out = b.p;
    return RDR_OK;
}

// Host bytes -> device, stream-ordered, with the source CONSUMED when this returns whatever memory it lives in (pageable or page-locked):
// up to PIN_MAX through the ring of page-locked buffers (the host never waits for earlier work on the stream); larger ones copied from where
// they are and waited for (one event behind the copy - which is what a pageable copy costs anyway).
// (several host pieces that land back to back on the device go up as ONE copy: every copy is a packet of its own on the stream - four of
// them per step showed as +20 us on the 0.13 ms step of BASELINE configs[1])
struct HostPart { const void* p; size_t bytes; };
static int upload(rdr_ctx* ctx, void* dst, const void* src, size_t bytes);
static int upload_parts(rdr_ctx* ctx, void* dst, const HostPart* parts, int nparts) {
    size_t bytes = 0;
    for (int i = 0; i < nparts; ++i) bytes += parts[i].bytes;
    if (bytes == 0) return RDR_OK;
    if (nparts == 1) return upload(ctx, dst, parts[0].p, bytes);
    if (bytes > rdr_ctx::PIN_MAX) {               // too large for the ring: piece by piece
        size_t o = 0;
        for (int i = 0; i < nparts; ++i) { const int rc = upload(ctx, static_cast<char*>(dst) + o, parts[i].p, parts[i].bytes); if (rc) return rc; o += parts[i].bytes; }
        return RDR_OK;
    }
    std::vector<char> tmp;                        // (small: at most PIN_MAX; the ring path of upload() consumes it before returning)
    tmp.resize(bytes);
    size_t o = 0;
    for (int i = 0; i < nparts; ++i) { std::memcpy(tmp.data() + o, parts[i].p, parts[i].bytes); o += parts[i].bytes; }
    return upload(ctx, dst, tmp.data(), bytes);
}

static int upload(rdr_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return RDR_OK;
    if (bytes <= rdr_ctx::PIN_MAX) {
        rdr_ctx::PinSlot& ps = ctx->pin[ctx->pin_next];
        ctx->pin_next = (ctx->pin_next + 1) % rdr_ctx::PIN_SLOTS;
        bool ok = true;
        if (ps.used) { ok = hipEventSynchronize(ps.ev) == hipSuccess; ps.used = false; }
        if (ok && ps.cap < bytes) {
            if (ps.p) { (void)hipHostFree(ps.p); ps.p = nullptr; ps.cap = 0; }
            const size_t cap = std::max(bytes, (size_t)1 << 14);
            ok = hipHostMalloc(&ps.p, cap, hipHostMallocDefault) == hipSuccess;
            if (ok) ps.cap = cap; else ps.p = nullptr;
        }
        if (ok && !ps.ev) ok = hipEventCreateWithFlags(&ps.ev, hipEventDisableTiming) == hipSuccess;
        if (ok) {
            std::memcpy(ps.p, src, bytes);
            HIPCHECK(ctx, hipMemcpyAsync(dst, ps.p, bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHECK(ctx, hipEventRecord(ps.ev, ctx->stream));
            ps.used = true;
            return RDR_OK;
        }
        (void)hipGetLastError();                  // (no page-locked memory to be had: the plain copy below)
    }
    HIPCHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (!ctx->staged_ev) HIPCHECK(ctx, hipEventCreateWithFlags(&ctx->staged_ev, hipEventDisableTiming));
    HIPCHECK(ctx, hipEventRecord(ctx->staged_ev, ctx->stream));
    HIPCHECK(ctx, hipEventSynchronize(ctx->staged_ev));
    return RDR_OK;
}

// input staging: host -> scratch slot (the host buffer is consumed when this returns), device -> passthrough
static int stage_in(rdr_ctx* ctx, int s, const void* src, size_t bytes, int loc, const void** dev) {
    if (!src) { *dev = nullptr; return RDR_OK; }
    if (loc == RDR_DEVICE) { *dev = src; return RDR_OK; }
    void* d;
    int rc = ensure(ctx, s, bytes, &d);
    if (rc) return rc;
    rc = upload(ctx, d, src, bytes);
    if (rc) return rc;
    *dev = d;
    return RDR_OK;
}

static int stage_out(rdr_ctx* ctx, int s, void* dst, size_t bytes, int loc, void** dev) {
    if (loc == RDR_DEVICE) { *dev = dst; return RDR_OK; }
    return ensure(ctx, s, bytes, dev);
}

static int finish_out(rdr_ctx* ctx, void* dst, const void* dev, size_t bytes, int loc) {
    if (loc == RDR_DEVICE || !dst) return RDR_OK;
    HIPCHECK(ctx, hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return RDR_OK;
}

// The stage / launch check / download / synchronise sequence of ONE call of an entry point, over the four functions above.  Every argument
// is named once, with its size: in() and out() hand out SLOT_IN0.. and SLOT_OUT0.. in the order of the calls (an absent - NULL - argument
// still takes its turn, so the others keep their slots), an explicit slot is for the few calls that deviate; finish() downloads what out()
// and inout() staged, with the sizes they were given.  The first failure is kept in `rc` and turns every later method into a no-op that
// returns NULL: an entry point tests `rc` once, before it launches.  Fixed arrays only, and no HIP call that the four functions do not make.
struct Staged {
    rdr_ctx* c; int loc, oloc; int rc = RDR_OK;
    int nin = 0, nout = 0, ndown = 0;
    struct { void* host; const void* dev; size_t bytes; } down[6];
    Staged(rdr_ctx* ctx, int loc_) : c(ctx), loc(loc_), oloc(loc_) {}
    Staged(rdr_ctx* ctx, int loc_, int out_loc) : c(ctx), loc(loc_), oloc(out_loc) {}   // outputs in another place than the inputs

    template <typename T> const T* in(const T* p, size_t bytes, int slot = -1) {
        const void* d = nullptr;
        if (slot < 0) slot = SLOT_IN0 + nin++;
        if (!rc) rc = stage_in(c, slot, p, bytes, loc, &d);
        return rc ? nullptr : static_cast<const T*>(d);
    }
    template <typename T> T* out(T* p, size_t bytes, int slot = -1) {      // p == NULL: an optional output that was not asked for
        void* d = nullptr;
        if (slot < 0) slot = SLOT_OUT0 + nout++;
        if (!p || rc) return nullptr;
        rc = stage_out(c, slot, p, bytes, oloc, &d);
        return rc ? nullptr : static_cast<T*>(download(p, d, bytes));
    }
    template <typename T> T* inout(T* p, size_t bytes, int slot) {         // staged up as an input, downloaded as an output
        const void* d = nullptr;
        if (!p || rc) return nullptr;
        rc = stage_in(c, slot, p, bytes, loc, &d);
        return rc ? nullptr : static_cast<T*>(download(p, const_cast<void*>(d), bytes));
    }
    template <typename T> T* scratch(int slot, size_t bytes) {             // device-only working memory of the call
        void* d = nullptr;
        if (!rc) rc = ensure(c, slot, bytes, &d);
        return rc ? nullptr : static_cast<T*>(d);
    }
    // a small table that comes from the HOST whatever `loc` says: its parts land back to back in `slot`, as one copy, and are consumed on return
    template <typename T> T* table(int slot, const HostPart* parts, int nparts) {
        size_t bytes = 0;
        for (int i = 0; i < nparts; ++i) bytes += parts[i].bytes;
        T* d = scratch<T>(slot, bytes);
        if (!rc) rc = upload_parts(c, d, parts, nparts);
        return rc ? nullptr : d;
    }
    // after the launch: its error, the downloads in the order they were staged, the host's wait when the outputs are its own (or `always`)
    int finish(bool always_sync = false) {
        if (rc) return rc;
        HIPCHECK(c, hipGetLastError());
        for (int i = 0; i < ndown; ++i) { rc = finish_out(c, down[i].host, down[i].dev, down[i].bytes, oloc); if (rc) return rc; }
        if (oloc == RDR_HOST || always_sync) HIPCHECK(c, hipStreamSynchronize(c->stream));
        return RDR_OK;
    }
private:
    void* download(void* host, void* dev, size_t bytes) {
        if (ndown == 6) { rc = fail(c, RDR_ERR_INVALID, "Staged: more than 6 outputs in one call"); return nullptr; }
        down[ndown++] = {host, dev, bytes};
        return dev;
    }
};

struct KTimer {
    rdr_ctx* c; int which; hipEvent_t stop = nullptr;
    KTimer(rdr_ctx* ctx, int w) : c(ctx), which(w) {
        if (!c->profiling) return;
        auto& v = c->evs[which];
        if (c->ev_used[which] == v.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            v.emplace_back(a, b);
        }
        auto& pr = v[c->ev_used[which]++];
        (void)hipEventRecord(pr.first, c->stream);
        stop = pr.second;
    }
    ~KTimer() { if (stop) (void)hipEventRecord(stop, c->stream); }
};

static inline int grid_for(int64_t n, int block, int max_blocks) {
    int64_t g = (n + block - 1) / block;
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, max_blocks));
}

// Large host-buffer calls overlap their PCIe transfers with the kernels (interp_pipeline, raytrace_pipelined, the group-by-group
// download of rdr_raytrace_slices) unless RAIDER_HIP_NO_PIPELINE is set.
static bool pipelining() {
    static const bool on = std::getenv("RAIDER_HIP_NO_PIPELINE") == nullptr;
    return on;
}

// Launch with `sm` bytes of dynamic LDS; allocations beyond the 64 KB default need the kernel's limit raised first (long
// non-uniform axes: their (node, 1/spacing) tables live in LDS, 16 B per node).
template <typename... KArgs, typename... Args>
static hipError_t launch_lds(void (*kern)(KArgs...), dim3 g, dim3 b, size_t sm, hipStream_t s, Args&&... args) {
    if (sm > (size_t)(48u << 10)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, g, b, sm, s, std::forward<Args>(args)...);
    return hipGetLastError();
}

// f(float2()) or f(double2()) by the cube's dtype, and what f returns: a generic lambda takes the element type of its kernel from the tag
template <typename F>
static auto by_dtype(const rdr_cube* q, F&& f) -> decltype(f(float2())) {
    if (q->dtype == RDR_F32) return f(float2());
    return f(double2());
}

// ---- kernels other than the two ray passes (raider_kernels.h) ---------------------------------------------------------
#include "cube_kernels.h"
#include "producer_kernels.h"
#include "orbit_kernels.h"
#include "aztime_kernels.h"
#include "native_kernels.h"
#include "proj_kernels.h"
#include "epoch_kernels.h"
#include "raster_kernels.h"
#include "tiff_kernels.h"
#include "deflate_kernels.h"
#include "inflate_kernels.h"
#include "variogram_kernels.h"
#include "cell_variogram_kernels.h"
#include "grid_stats_kernels.h"
#include "seasonal_kernels.h"
#include "variogram_fit_kernels.h"

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// (definitions below get C linkage from their extern "C" declarations in include/raider_hip.h)

int rdr_version(void) { return 102; }

// sha256[:16] over the sources of this translation unit, handed in by the build recipe (-DRDR_SOURCE_HASH=...; __graft_entry__.build):
// lets the loader prove that the binary it opened was compiled from the tree it sits in (mtimes do not survive a copy).
#ifndef RDR_SOURCE_HASH
#define RDR_SOURCE_HASH "unknown"
#endif
static const char k_source_hash[] = "rdr-source-hash:" RDR_SOURCE_HASH;      // (the marker lets the build recipe read it without dlopen)
const char* rdr_source_hash(void) { return k_source_hash + 16; }

const char* rdr_last_error(rdr_ctx* ctx) { return (ctx && !ctx->err.empty()) ? ctx->err.c_str() : g_err.c_str(); }

int rdr_create(int device, rdr_ctx** out) {
    if (!out) return fail(nullptr, RDR_ERR_INVALID, "rdr_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, RDR_ERR_NODEVICE, std::string("rdr_create: no HIP device available (") +
                    (e != hipSuccess ? hipGetErrorString(e) : "device count 0") + "); raider_amd has no CPU fallback");
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= count) return fail(nullptr, RDR_ERR_INVALID, "rdr_create: device index out of range");
    rdr_ctx* c = new rdr_ctx();
    c->device = device;
    const int rc = [&]() -> int {
        HIPCHECK(nullptr, hipSetDevice(device));
        hipDeviceProp_t prop;
        HIPCHECK(nullptr, hipGetDeviceProperties(&prop, device));
        c->num_cus = prop.multiProcessorCount;
        c->total_mem = prop.totalGlobalMem;
        c->lds_max = std::max<size_t>(prop.sharedMemPerBlock, prop.maxSharedMemoryPerMultiProcessor);
        c->name = prop.name;
        if (c->name.empty()) c->name = std::string("AMD ") + prop.gcnArchName;   // amdgpu.ids may be absent on the box
        HIPCHECK(nullptr, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        HIPCHECK(nullptr, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HIPCHECK(nullptr, hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
        c->stream = c->own_stream;
        HIPCHECK(nullptr, hipMalloc((void**)&c->d_maxlen, (size_t)MAX_SLICES * MAX_LEVELS * sizeof(unsigned long long)));
        HIPCHECK(nullptr, hipMalloc((void**)&c->d_flags, (MAX_SLICES + 4) * sizeof(int)));      // (+ the cube packer's NaN word)
        HIPCHECK(nullptr, hipMalloc((void**)&c->d_nparts, MAX_LEVELS * sizeof(int)));
        HIPCHECK(nullptr, hipMalloc((void**)&c->d_nslow, 2 * sizeof(int)));
        HIPCHECK(nullptr, hipMalloc((void**)&c->d_tilectr, 32 * sizeof(int)));
        HIPCHECK(nullptr, hipMalloc((void**)&c->d_sidectr, sizeof(int)));
        HIPCHECK(nullptr, hipMemset(c->d_sidectr, 0, sizeof(int)));
        HIPCHECK(nullptr, hipMalloc((void**)&c->d_onepass, OP_WORDS * sizeof(int)));
        HIPCHECK(nullptr, hipMemset(c->d_onepass, 0, OP_WORDS * sizeof(int)));
        HIPCHECK(nullptr, hipHostMalloc((void**)&c->h_word, 16 * sizeof(int), hipHostMallocDefault));
        HIPCHECK(nullptr, hipHostMalloc((void**)&c->nan_words, rdr_ctx::NAN_SLOTS * sizeof(int), hipHostMallocDefault));
        HIPCHECK(nullptr, hipMemset(c->d_nslow, 0, 2 * sizeof(int)));
        return RDR_OK;
    }();
    if (rc) { rdr_destroy(c); return rc; }
    if (const char* e = std::getenv("RAIDER_HIP_WORKSPACE_BYTES")) c->ws_limit = (size_t)std::strtoull(e, nullptr, 10);
    if (const char* e = std::getenv("RAIDER_HIP_CUBE_POOL_BYTES")) c->cube_pool_limit = (size_t)std::strtoull(e, nullptr, 10);
    *out = c;
    return RDR_OK;
}

void rdr_destroy(rdr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& b : c->slot) if (b.p) (void)hipFree(b.p);
    for (auto& e : c->cube_pool) { for (auto ev : e.evs) (void)hipEventDestroy(ev); (void)hipFree(e.p); }
    if (c->d_maxlen) (void)hipFree(c->d_maxlen);
    if (c->d_flags) (void)hipFree(c->d_flags);
    if (c->d_nparts) (void)hipFree(c->d_nparts);
    if (c->d_nslow) (void)hipFree(c->d_nslow);
    if (c->d_tilectr) (void)hipFree(c->d_tilectr);
    if (c->ws.p) (void)hipFree(c->ws.p);
    if (c->side.p) (void)hipFree(c->side.p);
    if (c->lev.p) (void)hipFree(c->lev.p);
    if (c->d_sidectr) (void)hipFree(c->d_sidectr);
    if (c->d_onepass) (void)hipFree(c->d_onepass);
    if (c->probe.p) (void)hipFree(c->probe.p);
    if (c->gridtrig.p) (void)hipFree(c->gridtrig.p);
    if (c->h_word) (void)hipHostFree(c->h_word);
    if (c->nan_words) (void)hipHostFree(c->nan_words);
    for (auto& ps : c->pin) { if (ps.ev) (void)hipEventDestroy(ps.ev); if (ps.p) (void)hipHostFree(ps.p); }
    if (c->staged_ev) (void)hipEventDestroy(c->staged_ev);
    for (auto& v : c->evs) for (auto& pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    delete c;
}

int rdr_set_stream(rdr_ctx* c, void* s) {
    if (!c) return fail(nullptr, RDR_ERR_INVALID, "ctx is NULL");
    // NULL is HIP's legacy default stream (what torch.cuda.current_stream().cuda_stream is unless the caller
    // switched streams); (void*)-1 restores the ctx's private stream
    const hipStream_t before = c->stream;
    const hipStream_t want = (s == (void*)(intptr_t)-1) ? c->own_stream : (hipStream_t)s;
    if (want != before) {
        // the context's scratch slots, flag words and asynchronously created cubes are shared by whatever stream it launches on: work on the
        // new stream is ordered after everything enqueued on the old one (one event; calls no longer end with a host synchronisation)
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
            if (hipEventRecord(ev, before) == hipSuccess) (void)hipStreamWaitEvent(want, ev, 0);
            (void)hipEventDestroy(ev);
        }
        (void)hipGetLastError();
    }
    if (s == (void*)(intptr_t)-1) c->stream = c->own_stream;
    else {
        c->stream = (hipStream_t)s;
        std::lock_guard<std::recursive_mutex> guard(g_view_mutex);
        if (std::find(c->ext_streams.begin(), c->ext_streams.end(), c->stream) == c->ext_streams.end()) {
            if (c->ext_streams.size() < 8) c->ext_streams.push_back(c->stream); else c->ext_overflow = true;
        }
    }
    return RDR_OK;
}

int rdr_forget_stream(rdr_ctx* c, void* s) {
    if (!c) return fail(nullptr, RDR_ERR_INVALID, "ctx is NULL");
    const hipStream_t st = (hipStream_t)s;
    if (c->stream == st && st != c->own_stream) {           // still the current one: finish its work, go back to the private stream
        HIPCHECK(c, hipStreamSynchronize(st));
        c->stream = c->own_stream;
    }
    std::lock_guard<std::recursive_mutex> guard(g_view_mutex);
    c->ext_streams.erase(std::remove(c->ext_streams.begin(), c->ext_streams.end(), st), c->ext_streams.end());
    if (c->ext_streams.size() < 8) c->ext_overflow = false;
    return RDR_OK;
}

int rdr_synchronize(rdr_ctx* c) {
    if (!c) return fail(nullptr, RDR_ERR_INVALID, "ctx is NULL");
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

int rdr_device_info(rdr_ctx* c, char* name, int name_len, int* cus, int64_t* mem) {
    if (!c) return fail(nullptr, RDR_ERR_INVALID, "ctx is NULL");
    if (name && name_len > 0) { std::strncpy(name, c->name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (cus) *cus = c->num_cus;
    if (mem) *mem = (int64_t)c->total_mem;
    return RDR_OK;
}

// Page-locked host memory for result arrays: a device -> host copy into it runs at the link rate without first-touch page faults
// (measured on the MI355X box: 512 MB into fresh pageable pages 31 ms, into resident or pinned pages 9.5 ms = 54 GB/s) and truly
// asynchronously, so the download of finished height slices overlaps the kernels of the next ones (rdr_raytrace_slices).
int rdr_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes <= 0) return fail(nullptr, RDR_ERR_INVALID, "rdr_host_alloc: bad argument");
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(nullptr, RDR_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    *out = p;
    return RDR_OK;
}

int rdr_host_free(void* p) {
    if (!p) return RDR_OK;
    const hipError_t e = hipHostFree(p);
    if (e != hipSuccess) return fail(nullptr, RDR_ERR_HIP, std::string("hipHostFree: ") + hipGetErrorString(e));
    return RDR_OK;
}

int rdr_set_workspace_limit(rdr_ctx* c, int64_t bytes) {
    if (!c || bytes < (int64_t)1 << 20) return fail(c, RDR_ERR_INVALID, "rdr_set_workspace_limit: need at least 1 MiB");
    c->ws_limit = (size_t)bytes;
    c->wsig.valid = false;
    return RDR_OK;
}

// every pooled buffer back to the device (waits for the events they were retired with)
static void pool_drain(rdr_ctx* c) {
    std::lock_guard<std::recursive_mutex> guard(g_view_mutex);
    while (!c->cube_pool.empty()) {
        rdr_ctx::PoolEntry e = c->cube_pool.front();
        c->cube_pool.erase(c->cube_pool.begin());
        c->cube_pool_bytes -= e.bytes;
        for (auto ev : e.evs) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
        (void)hipFree(e.p);
    }
    (void)hipGetLastError();
}

int rdr_trim(rdr_ctx* c, int64_t keep_bytes, int64_t* released) {
    if (!c || keep_bytes < 0) return fail(c, RDR_ERR_INVALID, "rdr_trim: NULL context or a negative size");
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->down_stream));
    HIPCHECK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if (c->stream != c->own_stream) HIPCHECK(c, hipStreamSynchronize(c->own_stream));
    const size_t keep = (size_t)keep_bytes;
    size_t freed = 0;
    auto drop = [&](DevBuf& b) { if (b.p && b.cap > keep) { if (hipFree(b.p) == hipSuccess) freed += b.cap; b.p = nullptr; b.cap = 0; } };
    for (auto& b : c->slot) drop(b);
    if ((c->ws.p && c->ws.cap > keep) || (c->side.p && c->side.cap > keep)) c->wsig.valid = false;      // (the stored ray records go with them)
    drop(c->ws);
    if (c->side.p && c->side.cap > keep) { drop(c->side); c->side_cap = 0; }
    drop(c->lev);
    std::lock_guard<std::recursive_mutex> guard(g_view_mutex);
    while (!c->cube_pool.empty() && c->cube_pool_bytes > keep) {          // oldest first
        rdr_ctx::PoolEntry e = c->cube_pool.front();
        c->cube_pool.erase(c->cube_pool.begin());
        c->cube_pool_bytes -= e.bytes;
        for (auto ev : e.evs) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
        if (hipFree(e.p) == hipSuccess) freed += e.bytes;
    }
    (void)hipGetLastError();
    if (released) *released = (int64_t)freed;
    return RDR_OK;
}

int rdr_set_side_capacity(rdr_ctx* c, int64_t columns) {
    if (!c) return fail(nullptr, RDR_ERR_INVALID, "ctx is NULL");
    c->side_forced = columns < 0 ? -1 : columns;
    c->wsig.valid = false;
    return RDR_OK;
}

int64_t rdr_generic_ray_count(rdr_ctx* c) { return c ? c->last_nslow : -1; }
int64_t rdr_skipped_wave_count(rdr_ctx* c) { return c ? c->last_nskip : -1; }
int64_t rdr_one_pass_count(rdr_ctx* c) { return c ? c->one_pass_calls : -1; }
int64_t rdr_one_pass_redo_count(rdr_ctx* c) { return c ? c->one_pass_redos : -1; }

int rdr_set_profiling(rdr_ctx* c, int on) {
    if (!c) return fail(nullptr, RDR_ERR_INVALID, "ctx is NULL");
    c->profiling = on != 0;
    for (auto& u : c->ev_used) u = 0;
    return RDR_OK;
}

// Shader clock while other kernels run: ONE wave on the copy stream sleeps for `ms` of wall time and reads the shader-clock counter
// (s_memtime) and the 100 MHz wall counter (s_memrealtime) before and after - cycles per wall tick = the clock the chip actually ran
// at during those milliseconds (under fp64-dense kernels it sits near 2.0 GHz, not at the 2.4 GHz of the data sheet).
__global__ void clock_sample_kernel(long long wall_ticks, long long* out) {
    if (threadIdx.x != 0) return;
    const long long c0 = clock64(), w0 = wall_clock64();
    while (wall_clock64() - w0 < wall_ticks) __builtin_amdgcn_s_sleep(127);
    const long long c1 = clock64(), w1 = wall_clock64();
    out[0] = c1 - c0; out[1] = w1 - w0;
}

int rdr_clock_sample_begin(rdr_ctx* c, double ms) {
    if (!c || !(ms > 0) || ms > 60000.0) return fail(c, RDR_ERR_INVALID, "rdr_clock_sample_begin: NULL context or a duration outside (0, 60000] ms");
    HIPCHECK(c, hipSetDevice(c->device));
    int khz = 0;
    HIPCHECK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    if (khz <= 0) return fail(c, RDR_ERR_HIP, "rdr_clock_sample_begin: the device reports no wall-clock rate");
    long long* out = reinterpret_cast<long long*>(c->h_word + 4);      // (page-locked and device-visible: the wave writes it directly)
    out[0] = 0; out[1] = 0;
    c->wall_khz = khz;
    hipLaunchKernelGGL(clock_sample_kernel, dim3(1), dim3(64), 0, c->copy_stream, (long long)(ms * khz), out);
    HIPCHECK(c, hipGetLastError());
    return RDR_OK;
}

int rdr_clock_sample_end(rdr_ctx* c, double* ghz) {
    if (!c || !ghz) return fail(c, RDR_ERR_INVALID, "rdr_clock_sample_end: NULL argument");
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->copy_stream));
    const long long* out = reinterpret_cast<const long long*>(c->h_word + 4);
    if (out[1] <= 0 || c->wall_khz <= 0) return fail(c, RDR_ERR_INVALID, "rdr_clock_sample_end: no sample was started on this context");
    *ghz = (double)out[0] / ((double)out[1] / (c->wall_khz * 1e3)) / 1e9;
    return RDR_OK;
}

int rdr_profile_get(rdr_ctx* c, int which, int* count, float* total_ms) {
    if (!c || which < 0 || which > 3 || !count || !total_ms) return fail(c, RDR_ERR_INVALID, "rdr_profile_get: bad argument");
    float tot = 0;
    for (size_t i = 0; i < c->ev_used[which]; ++i) {
        float ms = 0;
        HIPCHECK(c, hipEventSynchronize(c->evs[which][i].second));
        HIPCHECK(c, hipEventElapsedTime(&ms, c->evs[which][i].first, c->evs[which][i].second));
        tot += ms;
    }
    *count = (int)c->ev_used[which];
    *total_ms = tot;
    return RDR_OK;
}

// ---- cube ---------------------------------------------------------------------------------------
static int axis_check(const double* g, int64_t n, int* flip) {
    if (n < 2) return -1;
    bool asc = true, desc = true;
    for (int64_t i = 1; i < n; ++i) {
        if (!(g[i] > g[i - 1])) asc = false;
        if (!(g[i] < g[i - 1])) desc = false;
    }
    if (!asc && !desc) return -1;
    *flip = desc ? 1 : 0;
    return 0;
}

static void axis_uniformity(const std::vector<double>& g, int* uni, double* inv_d, int* exact = nullptr) {
    const int64_t n = (int64_t)g.size();
    const double span = g[n - 1] - g[0];
    *inv_d = (double)(n - 1) / span;
    double worst = 0;
    for (int64_t i = 0; i < n; ++i) worst = std::max(worst, std::fabs((g[i] - g[0]) * (*inv_d) - (double)i));
    *uni = worst < 0.25 ? 1 : 0;   // guess lands within +-1 cell; fix-up loops make it exact
    if (exact) *exact = worst < 1e-11 ? 1 : 0;   // uniform to round-off: cell index and weight from arithmetic alone (cell_xy)
}

template <typename T2>
static CubeView<T2> make_view(const rdr_cube* q) {
    CubeView<T2> v;
    v.v = (const T2*)q->d_vals;
    v.axes = q->d_axes;
    v.ny = (int)q->ny; v.nx = (int)q->nx; v.nz = (int)q->nz;
    v.y_lo = q->ys.front(); v.y_hi = q->ys.back();
    v.x_lo = q->xs.front(); v.x_hi = q->xs.back();
    v.z_lo = q->zs.front(); v.z_hi = q->zs.back();
    v.inv_dy = q->inv_d[0]; v.inv_dx = q->inv_d[1]; v.inv_dz = q->inv_d[2];
    v.uni_y = q->uni[0]; v.uni_x = q->uni[1]; v.uni_z = q->uni[2];
    v.exact_y = q->exact[0]; v.exact_x = q->exact[1];
    v.small = (q->ny * q->nx < (1 << 24)) && (q->nz < (1 << 24)) &&
              ((uint64_t)q->ny * q->nx * q->nz * sizeof(T2) < (1ULL << 32));
    return v;
}

// the zenith / station kernels stage the axes in LDS when they fit 48 KB, else read them from global memory
static bool axes_fit_lds(const rdr_cube* q) { return (size_t)(q->ny + q->nx + q->nz) * sizeof(double) <= (48u << 10); }
static size_t axes_smem(const rdr_cube* q) { return axes_fit_lds(q) ? (size_t)(q->ny + q->nx + q->nz) * sizeof(double) : 0; }

// The three axes of a cube from DEVICE copies of the arrays they were given as (any of them possibly descending): one tiny launch instead of
// one more host copy on the stream (rdr_build_cube_to_cube: the AOI axes went up for the build already).
struct DevAxes { const double* y = nullptr; const double* x = nullptr; const double* z = nullptr; int fy = 0, fx = 0, fz = 0; };
__global__ void axes_from_device_kernel(DevAxes a, int ny, int nx, int nz, double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ny + nx + nz; i += gridDim.x * blockDim.x) {
        double v;
        if (i < ny) v = a.y[a.fy ? ny - 1 - i : i];
        else if (i < ny + nx) { const int j = i - ny; v = a.x[a.fx ? nx - 1 - j : j]; }
        else { const int j = i - ny - nx; v = a.z[a.fz ? nz - 1 - j : j]; }
        out[i] = v;
    }
}

static int cube_alloc(rdr_ctx* c, rdr_cube* q, const DevAxes* dev_axes = nullptr) {
    const size_t esz = q->dtype == RDR_F32 ? 8 : 16;
    const size_t total = (size_t)q->ny * q->nx * q->nz;
    // ONE allocation: the values, then (256 B aligned) the three axes
    const size_t vbytes = (total * esz + 255) / 256 * 256;
    const size_t bytes = vbytes + (size_t)(q->ny + q->nx + q->nz) * sizeof(double);
    q->alloc_bytes = bytes;
    std::unique_lock<std::recursive_mutex> guard(g_view_mutex);
    for (size_t i = 0; i < c->cube_pool.size(); ++i) {
        if (c->cube_pool[i].bytes != bytes) continue;
        const rdr_ctx::PoolEntry e = c->cube_pool[i];
        c->cube_pool.erase(c->cube_pool.begin() + (long)i);
        c->cube_pool_bytes -= bytes;
        // (its previous cube's last work on every stream this context launches on was enqueued before these events: whatever stream
        // builds the new cube waits for them)
        hipError_t w = hipSuccess;
        for (auto ev : e.evs) { if (w == hipSuccess) w = hipStreamWaitEvent(c->stream, ev, 0); (void)hipEventDestroy(ev); }
        if (w != hipSuccess) { (void)hipDeviceSynchronize(); (void)hipFree(e.p); (void)hipGetLastError(); break; }
        q->d_vals = e.p;
        break;
    }
    if (!q->d_vals) { const int rc = dev_malloc(c, &q->d_vals, bytes); if (rc) { q->alloc_bytes = 0; return rc; } }     // (out of memory: the pool is drained, then once more)
    guard.unlock();
    q->d_axes = reinterpret_cast<double*>(static_cast<char*>(q->d_vals) + vbytes);
    std::vector<double> ax;
    ax.insert(ax.end(), q->ys.begin(), q->ys.end());
    ax.insert(ax.end(), q->xs.begin(), q->xs.end());
    ax.insert(ax.end(), q->zs.begin(), q->zs.end());
    // (stream-ordered: a pooled buffer may still be read by work enqueued before the event above; through the page-locked ring: the host
    // does not wait for what the stream is still doing - creation from device sources really is asynchronous)
    if (dev_axes && dev_axes->y) {
        hipLaunchKernelGGL(axes_from_device_kernel, dim3((unsigned)((ax.size() + 255) / 256)), dim3(256), 0, c->stream, *dev_axes, (int)q->ny, (int)q->nx, (int)q->nz, q->d_axes);
        HIPCHECK(c, hipGetLastError());
    } else { const int rc = upload(c, q->d_axes, ax.data(), ax.size() * sizeof(double)); if (rc) return rc; }
    axis_uniformity(q->ys, &q->uni[0], &q->inv_d[0], &q->exact[0]);
    axis_uniformity(q->xs, &q->uni[1], &q->inv_d[1], &q->exact[1]);
    axis_uniformity(q->zs, &q->uni[2], &q->inv_d[2]);
    return RDR_OK;
}

static int cube_create_impl(rdr_ctx* c, const double* ys, int64_t ny, const double* xs, int64_t nx, const double* zs, int64_t nz,
                            const void* wet, const void* hydro, int dtype, int64_t sy, int64_t sx, int64_t sz, int loc,
                            rdr_cube** out, const double* const* dev_yxz);

int rdr_cube_create(rdr_ctx* c, const double* ys, int64_t ny, const double* xs, int64_t nx, const double* zs, int64_t nz,
                    const void* wet, const void* hydro, int dtype, int64_t sy, int64_t sx, int64_t sz, int loc,
                    rdr_cube** out) {
    return cube_create_impl(c, ys, ny, xs, nx, zs, nz, wet, hydro, dtype, sy, sx, sz, loc, out, nullptr);
}

// dev_yxz: device copies of the three axis arrays AS GIVEN (before any flip), or NULL: the axes go up from the host
static int cube_create_impl(rdr_ctx* c, const double* ys, int64_t ny, const double* xs, int64_t nx, const double* zs, int64_t nz,
                            const void* wet, const void* hydro, int dtype, int64_t sy, int64_t sx, int64_t sz, int loc,
                            rdr_cube** out, const double* const* dev_yxz) {
    if (!c || !out || !ys || !xs || !zs || !wet || !hydro) return fail(c, RDR_ERR_INVALID, "rdr_cube_create: NULL argument");
    const bool swapped = (dtype & RDR_BYTESWAPPED) != 0;       // the source fields are in the other byte order (NetCDF-3: big-endian)
    dtype &= ~RDR_BYTESWAPPED;
    if (dtype != RDR_F32 && dtype != RDR_F64) return fail(c, RDR_ERR_INVALID, "rdr_cube_create: dtype must be RDR_F32 or RDR_F64 (optionally | RDR_BYTESWAPPED)");
    if (nz > MAX_LEVELS) return fail(c, RDR_ERR_INVALID, "rdr_cube_create: more than 512 z levels");
    if (ny + nx + nz > 100000) return fail(c, RDR_ERR_INVALID, "rdr_cube_create: axes too long");
    int fy, fx, fz;
    if (axis_check(ys, ny, &fy) || axis_check(xs, nx, &fx) || axis_check(zs, nz, &fz))
        return fail(c, RDR_ERR_INVALID, "The points in each dimension must be strictly ascending or descending (and >= 2)");
    HIPCHECK(c, hipSetDevice(c->device));
    rdr_cube* q = new rdr_cube();
    q->ctx = c; q->ny = ny; q->nx = nx; q->nz = nz; q->dtype = dtype;
    q->ys.assign(ys, ys + ny); q->xs.assign(xs, xs + nx); q->zs.assign(zs, zs + nz);
    if (fy) std::reverse(q->ys.begin(), q->ys.end());
    if (fx) std::reverse(q->xs.begin(), q->xs.end());
    if (fz) std::reverse(q->zs.begin(), q->zs.end());
    DevAxes da;
    if (dev_yxz) { da.y = dev_yxz[0]; da.x = dev_yxz[1]; da.z = dev_yxz[2]; da.fy = fy; da.fx = fx; da.fz = fz; }
    int rc = cube_alloc(c, q, dev_yxz ? &da : nullptr);
    if (rc) { rdr_cube_destroy(q); return rc; }
    const size_t total = (size_t)ny * nx * nz;
    const size_t esz = dtype == RDR_F32 ? 4 : 8;
    // span of the strided source (non-negative strides)
    if (sy < 0 || sx < 0 || sz < 0) { rdr_cube_destroy(q); return fail(c, RDR_ERR_INVALID, "rdr_cube_create: negative strides not supported"); }
    const size_t span = (size_t)((ny - 1) * sy + (nx - 1) * sx + (nz - 1) * sz + 1);
    const void *dw, *dh;
    rc = stage_in(c, SLOT_IN0, wet, span * esz, loc, &dw); if (rc) { rdr_cube_destroy(q); return rc; }
    rc = stage_in(c, SLOT_IN1, hydro, span * esz, loc, &dh); if (rc) { rdr_cube_destroy(q); return rc; }
    const int g = grid_for((int64_t)total, 256, c->num_cus * 8);
    int* const nf = c->d_flags + MAX_SLICES;      // (a word of the flag array no ray batch uses)
    hipError_t e = hipMemsetAsync(nf, 0, sizeof(int), c->stream);
    if (e != hipSuccess) { rdr_cube_destroy(q); return fail(c, RDR_ERR_HIP, hipGetErrorString(e)); }
#define RDR_PACK(T, T2, SW) hipLaunchKernelGGL((pack_cube_kernel<T, T2, SW>), dim3(g), dim3(256), 0, c->stream, (const T*)dw, (const T*)dh, \
                                               (T2*)q->d_vals, ny, nx, nz, sy, sx, sz, fy, fx, fz, nf)
    // x-contiguous sources (file order (z, y, x); the planar results behind an intermediate delay cube): the LDS-transposing kernel
    const bool xfast = sx == 1 && nx >= 8 && nz >= 8;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(ny * ((nx + 31) / 32) * ((nz + 31) / 32), (int64_t)c->num_cus * 16));
#define RDR_PACKX(T, T2, SW) hipLaunchKernelGGL((pack_cube_xfast_kernel<T, T2, SW>), dim3(gx), dim3(256), 0, c->stream, (const T*)dw, (const T*)dh, \
                                                (T2*)q->d_vals, ny, nx, nz, sy, sz, fy, fx, fz, nf)
    {
        KTimer t(c, 2);       // (the packing of an intermediate delay cube is part of the point branch's step: bench.py --workload c2 counts it)
        if (xfast) {
            if (dtype == RDR_F32) { if (swapped) RDR_PACKX(float, float2, true); else RDR_PACKX(float, float2, false); }
            else { if (swapped) RDR_PACKX(double, double2, true); else RDR_PACKX(double, double2, false); }
        } else if (dtype == RDR_F32) { if (swapped) RDR_PACK(float, float2, true); else RDR_PACK(float, float2, false); }
        else { if (swapped) RDR_PACK(double, double2, true); else RDR_PACK(double, double2, false); }
    }
#undef RDR_PACKX
#undef RDR_PACK
    e = hipGetLastError();
    if (e != hipSuccess) { rdr_cube_destroy(q); return fail(c, RDR_ERR_HIP, hipGetErrorString(e)); }
    if (loc == RDR_DEVICE) {
        // DEVICE sources (intermediate delay cubes, cubes made from tensors): no host synchronisation.  The verdict travels into a page-locked
        // word and is read when asked for (rdr_cube_has_nan -> cube_resolve_nan); other streams wait for the ready event (note_use).
        std::unique_lock<std::recursive_mutex> guard(g_view_mutex);                // (the slots are also released by whoever destroys a cube)
        int slot = c->nan_next; c->nan_next = (c->nan_next + 1) % rdr_ctx::NAN_SLOTS;
        if (c->nan_owner[slot]) cube_resolve_nan(c->nan_owner[slot]);              // (a cube 256 creations ago that nobody asked: settle it now)
        c->nan_words[slot] = 0;
        e = hipMemcpyAsync(&c->nan_words[slot], nf, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { guard.unlock(); rdr_cube_destroy(q); return fail(c, RDR_ERR_HIP, hipGetErrorString(e)); }
        rc = cube_mark_ready(c, q);
        if (rc) { guard.unlock(); rdr_cube_destroy(q); return rc; }
        q->nan_slot = slot; c->nan_owner[slot] = q;
        *out = q;
        return RDR_OK;
    }
    // HOST sources: the staging slots are free again and the cube is complete when the call returns
    int has_nan = 0;
    e = hipMemcpyAsync(&has_nan, nf, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { rdr_cube_destroy(q); return fail(c, RDR_ERR_HIP, hipGetErrorString(e)); }
    q->has_nan = has_nan != 0;
    *out = q;
    return RDR_OK;
}

static int cone_params(rdr_ctx* c, const char* who, int kind, const double* p, int np, LccParams& out);

// The buffers of a dead cube.  Pooled (no synchronisation) with one event per stream the owning context has ever launched on - its own
// three and every caller stream handed to rdr_set_stream (a torch stream adopted earlier may still be reading the cube) - or, when that
// cannot be established (another context used the cube, more caller streams than are tracked, an event that cannot be recorded - e.g.
// on a stream the caller has destroyed), freed after a device-wide synchronisation.
static void cube_release(rdr_cube* q) {
    rdr_ctx* c = q->ctx;
    if (c) (void)hipSetDevice(c->device);
    // (may run on a thread of ANOTHER context - the last view of a destroyed source: the owner's slots and pool are under the shared lock)
    std::lock_guard<std::recursive_mutex> guard(g_view_mutex);
    if (c && q->nan_slot >= 0) { c->nan_owner[q->nan_slot] = nullptr; q->nan_slot = -1; }     // (nobody asked: the word is free again)
    if (q->ready_ev) { (void)hipEventDestroy(q->ready_ev); q->ready_ev = nullptr; }
    bool pooled = false;
    const bool foreign = q->foreign.load(std::memory_order_relaxed);
    if (c && q->d_vals && q->alloc_bytes > 0 && !foreign && !c->ext_overflow && c->cube_pool.size() < 6 &&
        c->cube_pool_bytes + q->alloc_bytes <= c->cube_pool_limit) {
        // the context's own three streams, and of the caller streams only those this cube was used on AND the context still knows
        // (rdr_forget_stream drops a stream the caller is about to destroy: no event is ever recorded on a dead handle)
        std::vector<hipStream_t> st = {c->own_stream, c->copy_stream, c->down_stream};
        for (auto s_ : c->ext_streams)
            if (std::find(q->used_streams.begin(), q->used_streams.end(), s_) != q->used_streams.end()) st.push_back(s_);
        if (std::find(st.begin(), st.end(), c->stream) == st.end()) st.push_back(c->stream);
        std::vector<hipEvent_t> evs;
        bool ok = true;
        for (auto s_ : st) {
            hipEvent_t ev = nullptr;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ok = false; break; }
            evs.push_back(ev);
            if (hipEventRecord(ev, s_) != hipSuccess) { ok = false; break; }
        }
        if (ok) {
            // (the corner-quad copy is freed, not pooled: wait for the same events first - every stream that may still be reading it)
            if (q->d_quad) for (auto ev : evs) (void)hipEventSynchronize(ev);
            c->cube_pool.push_back({q->d_vals, q->alloc_bytes, evs});
            c->cube_pool_bytes += q->alloc_bytes;
            pooled = true;
        } else { for (auto ev : evs) (void)hipEventDestroy(ev); (void)hipGetLastError(); }
    }
    if (!pooled) (void)hipDeviceSynchronize();
    if (!pooled && q->d_vals && q->alloc_bytes > 0) (void)hipFree(q->d_vals);       // (the axes live in the same allocation)
    if (q->d_quad) (void)hipFree(q->d_quad);
    delete q;
}

void rdr_cube_destroy(rdr_cube* q) {
    if (!q) return;
    const rdr_cube* dead_root = nullptr;
    {
        std::lock_guard<std::recursive_mutex> guard(g_view_mutex);
        if (q->base) {                                  // a view: only the handle goes; the last view of a destroyed source frees the buffers
            const rdr_cube* r = q->base;
            delete q;
            if (--r->views == 0 && r->doomed) dead_root = r;
            q = nullptr;
        } else if (q->views > 0) { q->doomed = true; q = nullptr; }
    }
    if (dead_root) cube_release(const_cast<rdr_cube*>(dead_root));
    if (q) cube_release(q);
}

int rdr_cube_view(rdr_ctx* c, const rdr_cube* src, int kind, const double* p, int np, rdr_cube** out) {
    if (!c || !src || !out) return fail(c, RDR_ERR_INVALID, "rdr_cube_view: NULL argument");
    *out = nullptr;
    LccParams L = src->proj;
    if (kind == RDR_PROJ_LONLAT) L = LccParams{0, 0, 0, 0, 0, 0, 0, 0};
    else if (kind != -1) { const int rc = cone_params(c, "rdr_cube_view", kind, p, np, L); if (rc) return rc; }
    const rdr_cube* r = root(src);
    if (c->device != r->ctx->device) return fail(c, RDR_ERR_INVALID, "rdr_cube_view: the context is on another device than the cube");
    rdr_cube* v = new rdr_cube();
    v->ctx = c; v->ny = r->ny; v->nx = r->nx; v->nz = r->nz; v->dtype = r->dtype;
    v->d_vals = r->d_vals; v->d_axes = r->d_axes; v->ys = r->ys; v->xs = r->xs; v->zs = r->zs;
    for (int i = 0; i < 3; ++i) { v->uni[i] = r->uni[i]; v->inv_d[i] = r->inv_d[i]; }
    v->exact[0] = r->exact[0]; v->exact[1] = r->exact[1];
    v->proj = L; v->alloc_bytes = 0; v->base = r;
    note_use(c, r);
    { std::lock_guard<std::recursive_mutex> guard(g_view_mutex); ++r->views; }
    *out = v;
    return RDR_OK;
}

int rdr_cube_has_nan(const rdr_cube* q) {
    if (!q) return -1;
    const rdr_cube* r = root(q);                  // (a view's verdict is its source's)
    cube_resolve_nan(r);
    return r->has_nan ? 1 : 0;
}

int rdr_cube_shape(const rdr_cube* q, int64_t* ny, int64_t* nx, int64_t* nz, int* dtype) {
    if (!q) return fail(nullptr, RDR_ERR_INVALID, "cube is NULL");
    if (ny) *ny = q->ny; if (nx) *nx = q->nx; if (nz) *nz = q->nz; if (dtype) *dtype = q->dtype;
    return RDR_OK;
}

int rdr_cube_axes(const rdr_cube* q, double* ys, double* xs, double* zs) {
    if (!q) return fail(nullptr, RDR_ERR_INVALID, "cube is NULL");
    if (ys) std::copy(q->ys.begin(), q->ys.end(), ys);
    if (xs) std::copy(q->xs.begin(), q->xs.end(), xs);
    if (zs) std::copy(q->zs.begin(), q->zs.end(), zs);
    return RDR_OK;
}

// LccParams of a conic model CRS from the C ABI's parameter array (shared by rdr_cube_set_projection / rdr_transform_cone)
static int cone_params(rdr_ctx* c, const char* who, int kind, const double* p, int np, LccParams& out) {
    const std::string w(who);
    if (kind == RDR_PROJ_STERE) {
        if (!p || np < 8) return fail(c, RDR_ERR_INVALID, w + ": STERE needs 8 parameters (a, es, lat_0, lat_ts, k_0, lon_0, x_0, y_0)");
        if (!(p[0] > 0) || p[1] < 0 || p[1] >= 1 || std::fabs(std::fabs(p[2]) - 90.0) > 1e-9 || (p[3] == p[3] && (std::fabs(p[3]) > 90 || p[3] * p[2] < 0)) || !(p[4] > 0))
            return fail(c, RDR_ERR_INVALID, w + ": only the POLAR stereographic aspect is supported (lat_0 = +-90, lat_ts in the same hemisphere, k_0 > 0)");
        out = stere_setup(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
        return RDR_OK;
    }
    if (kind != RDR_PROJ_LCC || !p || np < 8) return fail(c, RDR_ERR_INVALID, w + ": LCC needs 8 parameters (a, es, lat_1, lat_2, lat_0, lon_0, x_0, y_0)");
    if (!(p[0] > 0) || p[1] < 0 || p[1] >= 1 || std::fabs(p[2]) >= 90 || std::fabs(p[3]) >= 90 || std::fabs(p[2] + p[3]) < 1e-10)
        return fail(c, RDR_ERR_INVALID, w + ": invalid LCC parameters");
    out = lcc_setup(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
    return RDR_OK;
}

int rdr_cube_set_projection(rdr_cube* q, int kind, const double* p, int np) {
    if (!q) return fail(nullptr, RDR_ERR_INVALID, "cube is NULL");
    if (kind == RDR_PROJ_LONLAT) { q->proj = LccParams{0, 0, 0, 0, 0, 0, 0, 0}; return RDR_OK; }
    LccParams L;
    const int rc = cone_params(q->ctx, "rdr_cube_set_projection", kind, p, np, L);
    if (rc) return rc;
    q->proj = L;
    return RDR_OK;
}

int rdr_transform_cone(rdr_ctx* c, int kind, const double* p, int np, int direction, const double* in_a, const double* in_b, int64_t n,
                       double* out_a, double* out_b, int loc) {
    if (!c || (n > 0 && (!in_a || !in_b || !out_a || !out_b))) return fail(c, RDR_ERR_INVALID, "rdr_transform_cone: NULL argument");
    if (direction != 0 && direction != 1) return fail(c, RDR_ERR_INVALID, "rdr_transform_cone: direction is 0 (forward) or 1 (inverse)");
    LccParams L;
    int rc = cone_params(c, "rdr_transform_cone", kind, p, np, L); if (rc) return rc;
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_transform_cone: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *da = S.in(in_a, (size_t)n * 8), *db = S.in(in_b, (size_t)n * 8);
    double *oa = S.out(out_a, (size_t)n * 8), *ob = S.out(out_b, (size_t)n * 8);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(cone_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, L, direction, da, db, n, oa, ob);
    return S.finish();
}

int rdr_project_points(rdr_ctx* c, const rdr_cube* q, const double* lat, const double* lon, int64_t n, double* y, double* x, int loc) {
    if (!c || !q || !lat || !lon || !y || !x) return fail(c, RDR_ERR_INVALID, "rdr_project_points: NULL argument");
    note_use(c, q);
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_project_points: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    if (q->proj.kind == 0) {     // lon/lat cube: identity
        const hipMemcpyKind k = loc == RDR_HOST ? hipMemcpyHostToHost : hipMemcpyDeviceToDevice;
        HIPCHECK(c, hipMemcpyAsync(y, lat, (size_t)n * 8, k, c->stream));
        HIPCHECK(c, hipMemcpyAsync(x, lon, (size_t)n * 8, k, c->stream));
        if (loc == RDR_HOST) HIPCHECK(c, hipStreamSynchronize(c->stream));
        return RDR_OK;
    }
    Staged S(c, loc);
    const double *a = S.in(lat, (size_t)n * 8), *b = S.in(lon, (size_t)n * 8);
    double *oy = S.out(y, (size_t)n * 8), *ox = S.out(x, (size_t)n * 8);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(lcc_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, q->proj, a, b, n, oy, ox);
    return S.finish();
}

int rdr_transform_tm(rdr_ctx* c, const double* p, int np, int direction, const double* in_a, const double* in_b, int64_t n, double* out_a,
                     double* out_b, int loc) {
    if (!c || !p || np < 7 || (n > 0 && (!in_a || !in_b || !out_a || !out_b))) return fail(c, RDR_ERR_INVALID, "rdr_transform_tm: NULL argument / 7 parameters (a, es, lat_0, lon_0, k_0, x_0, y_0)");
    if (!(p[0] > 0) || p[1] < 0 || p[1] >= 1 || std::fabs(p[2]) > 90 || !(p[4] > 0)) return fail(c, RDR_ERR_INVALID, "rdr_transform_tm: invalid transverse-Mercator parameters");
    if (direction != 0 && direction != 1) return fail(c, RDR_ERR_INVALID, "rdr_transform_tm: direction is 0 (forward) or 1 (inverse)");
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_transform_tm: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    const TmParams T = tm_setup(p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
    Staged S(c, loc);
    const double *da = S.in(in_a, (size_t)n * 8), *db = S.in(in_b, (size_t)n * 8);
    double *oa = S.out(out_a, (size_t)n * 8), *ob = S.out(out_b, (size_t)n * 8);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(tm_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, T, direction, da, db, n, oa, ob);
    return S.finish();
}

// ---- output grids in a projected CRS (transformPoints of delay.py:207-209,262-263 on the (ny, nx) meshgrid) -------------------------
// grid_kind RDR_GRID_TM: params as rdr_transform_tm; RDR_PROJ_LCC / RDR_PROJ_STERE: params as rdr_cube_set_projection.
struct GridCrs { int kind; TmParams T; LccParams L; };

static int grid_crs(rdr_ctx* c, const char* who, int kind, const double* p, int np, GridCrs& g) {
    const std::string w(who);
    g.kind = kind;
    if (kind == RDR_GRID_TM) {
        if (!p || np < 7) return fail(c, RDR_ERR_INVALID, w + ": RDR_GRID_TM needs 7 parameters (a, es, lat_0, lon_0, k_0, x_0, y_0)");
        if (!(p[0] > 0) || p[1] < 0 || p[1] >= 1 || std::fabs(p[2]) > 90 || !(p[4] > 0)) return fail(c, RDR_ERR_INVALID, w + ": invalid transverse-Mercator parameters");
        g.T = tm_setup(p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
        return RDR_OK;
    }
    if (kind == RDR_PROJ_LCC || kind == RDR_PROJ_STERE) return cone_params(c, who, kind, p, np, g.L);
    return fail(c, RDR_ERR_INVALID, w + ": grid_kind is RDR_GRID_TM, RDR_PROJ_LCC or RDR_PROJ_STERE");
}

static int grid_counts(rdr_ctx* c, const char* who, int64_t nx, int64_t ny) {
    if (nx < 0 || ny < 0) return fail(c, RDR_ERR_INVALID, std::string(who) + ": negative count");
    if (nx > ((int64_t)1 << 31) || ny > ((int64_t)1 << 31) || (nx > 0 && ny > ((int64_t)1 << 34) / nx))
        return fail(c, RDR_ERR_INVALID, std::string(who) + ": grid too large");
    return RDR_OK;
}

// The nodes of the grid (device axes dx[nx], dy[ny]) as (lat, lon) deg, or - model->kind == 1 - as (y, x) in the conic model CRS: the
// meshgrid, then tm_kernel / cone_kernel direction 1 (then cone_kernel direction 0 with the model's cone), each launched as
// rdr_transform_tm / rdr_transform_cone launch it - the same bits as transformPoints.  t0, t1, u0, u1: nx*ny doubles of scratch each;
// (*oy, *ox) point into them.
static int grid_nodes(rdr_ctx* c, const GridCrs& g, const double* dx, int64_t nx, const double* dy, int64_t ny, const LccParams* model,
                      double* t0, double* t1, double* u0, double* u1, const double** oy, const double** ox) {
    const int64_t n = nx * ny;
    const dim3 gs(grid_for(n, 256, c->num_cus * 8));
    hipLaunchKernelGGL(grid_mesh_kernel, gs, dim3(256), 0, c->stream, dx, nx, dy, ny, t0, t1);
    if (g.kind == RDR_GRID_TM) hipLaunchKernelGGL(tm_kernel, gs, dim3(256), 0, c->stream, g.T, 1, (const double*)t0, (const double*)t1, n, u0, u1);
    else hipLaunchKernelGGL(cone_kernel, gs, dim3(256), 0, c->stream, g.L, 1, (const double*)t0, (const double*)t1, n, u0, u1);
    *oy = u0; *ox = u1;
    if (model && model->kind == 1) {
        hipLaunchKernelGGL(cone_kernel, gs, dim3(256), 0, c->stream, *model, 0, (const double*)u0, (const double*)u1, n, t0, t1);
        *oy = t0; *ox = t1;
    }
    HIPCHECK(c, hipGetLastError());
    return RDR_OK;
}

int rdr_grid_geodetic(rdr_ctx* c, int grid_kind, const double* params, int nparams, const double* xpts, int64_t nx, const double* ypts, int64_t ny,
                      double* lat, double* lon, int loc) {
    static const char* who = "rdr_grid_geodetic";
    if (!c || !xpts || !ypts || !lat || !lon) return fail(c, RDR_ERR_INVALID, "rdr_grid_geodetic: NULL argument");
    GridCrs g;
    int rc = grid_crs(c, who, grid_kind, params, nparams, g); if (rc) return rc;
    rc = grid_counts(c, who, nx, ny); if (rc) return rc;
    const int64_t n = nx * ny;
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *dx = S.in(xpts, (size_t)nx * 8), *dy = S.in(ypts, (size_t)ny * 8);
    double* t = S.scratch<double>(SLOT_IN2, (size_t)n * 16);
    double *ola = S.out(lat, (size_t)n * 8), *olo = S.out(lon, (size_t)n * 8);
    if (S.rc) return S.rc;
    const double *oy, *ox;
    rc = grid_nodes(c, g, dx, nx, dy, ny, nullptr, t, t + n, ola, olo, &oy, &ox);
    if (rc) return rc;
    return S.finish();
}

// the same shape, dtype and axis vectors: what the two-epoch blends and the blended point gathers ask of their cubes
static bool same_grid_dtype(const rdr_cube* a, const rdr_cube* b) {
    return a->ny == b->ny && a->nx == b->nx && a->nz == b->nz && a->dtype == b->dtype && a->ys == b->ys && a->xs == b->xs && a->zs == b->zs;
}

int rdr_cube_blend(rdr_ctx* c, const rdr_cube* a, double w1, const rdr_cube* b, double w2, rdr_cube** out) {
    if (!c || !a || !b || !out) return fail(c, RDR_ERR_INVALID, "rdr_cube_blend: NULL argument");
    note_use(c, a); note_use(c, b);
    if (!same_grid_dtype(a, b))
        return fail(c, RDR_ERR_INVALID, "rdr_cube_blend: cubes are not on the same grid / dtype");
    HIPCHECK(c, hipSetDevice(c->device));
    rdr_cube* q = new rdr_cube();
    q->ctx = c; q->ny = a->ny; q->nx = a->nx; q->nz = a->nz; q->dtype = a->dtype;
    q->ys = a->ys; q->xs = a->xs; q->zs = a->zs; q->proj = a->proj;
    q->has_nan = rdr_cube_has_nan(a) == 1 || rdr_cube_has_nan(b) == 1;
    int rc = cube_alloc(c, q);
    if (rc) { rdr_cube_destroy(q); return rc; }
    const int64_t nscal = 2 * a->ny * a->nx * a->nz;                  // (wet, hydro) pairs as one flat array
    const int vec = a->dtype == RDR_F32 ? 4 : 2;
    // one pass: a grid that covers the array once (4 vectors per lane) streams at 6.4 TB/s; a persistent 8-16 blocks per CU grid
    // looping over it measured 4.8-5.4 TB/s (tools/probes/blend_probe.hip)
    const int g = grid_for((nscal / vec + 3) / 4, 256, 1 << 22);
    {
        KTimer t(c, 3);
        by_dtype(a, [&](auto tag) {
            typedef decltype(tag.x) T;
            hipLaunchKernelGGL((blend_kernel<T>), dim3(g), dim3(256), 0, c->stream, (const T*)a->d_vals, (T)w1, (const T*)b->d_vals, (T)w2, (T*)q->d_vals, nscal);
        });
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rdr_cube_destroy(q); return fail(c, RDR_ERR_HIP, hipGetErrorString(e)); }
    rc = cube_mark_ready(c, q);                    // (no host synchronisation: device sources, device result - other streams wait for the event)
    if (rc) { rdr_cube_destroy(q); return rc; }
    *out = q;
    return RDR_OK;
}

int rdr_inverse_time_weights(rdr_ctx* c, const double* az, int64_t n, const double* dates, int32_t nd, double window_s, double regularizer,
                             double* weights, int loc) {
    if (!c || !az || !dates || !weights) return fail(c, RDR_ERR_INVALID, "rdr_inverse_time_weights: NULL argument");
    if (nd < 1) return fail(c, RDR_ERR_INVALID, "No dates provided");
    if (nd > 8) return fail(c, RDR_ERR_INVALID, "rdr_inverse_time_weights: at most 8 dates");
    DateSet D; D.nd = nd; D.reg = regularizer;
    for (int i = 0; i < nd; ++i) {
        D.date[i] = dates[i];
        for (int j = 0; j < i; ++j) if (dates[j] == dates[i]) return fail(c, RDR_ERR_INVALID, "Dates provided must be unique");
    }
    if (window_s < 0) {                                  // s1_azimuth_timing.py:375-376: infer the model time step
        if (nd < 2) return fail(c, RDR_ERR_INVALID, "rdr_inverse_time_weights: the temporal window cannot be inferred from one date");
        window_s = std::fabs(dates[1] - dates[0]);
        for (int i = 2; i < nd; ++i) window_s = std::min(window_s, std::fabs(dates[i] - dates[0]));
    }
    D.window = window_s;
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_inverse_time_weights: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double* da = S.in(az, (size_t)n * 8);
    double* dw = S.out(weights, (size_t)n * nd * 8);
    if (S.rc) return S.rc;
    HIPCHECK(c, hipMemsetAsync(c->d_flags, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(time_weights_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, D, da, n, dw, c->d_flags);
    int f = 0;
    HIPCHECK(c, hipMemcpyAsync(&f, c->d_flags, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    const int rc = S.finish(true);                       // (always waits: the flag is read here)
    if (rc) return rc;
    if (!f) return fail(c, RDR_ERR_INVALID, "No dates provided are within temporal window");
    return RDR_OK;
}

int rdr_cube_blend_weighted(rdr_ctx* c, const rdr_cube* const* cubes, int32_t nd, const double* weights, int loc, rdr_cube** out) {
    if (!c || !cubes || !weights || !out) return fail(c, RDR_ERR_INVALID, "rdr_cube_blend_weighted: NULL argument");
    if (nd < 1 || nd > 8) return fail(c, RDR_ERR_INVALID, "rdr_cube_blend_weighted: 1..8 cubes");
    const rdr_cube* a = cubes[0];
    CubeSet S; S.nd = nd;
    for (int i = 0; i < nd; ++i) {
        const rdr_cube* b = cubes[i];
        if (!b) return fail(c, RDR_ERR_INVALID, "rdr_cube_blend_weighted: NULL cube");
        note_use(c, b);
        if (!same_grid_dtype(a, b))
            return fail(c, RDR_ERR_INVALID, "rdr_cube_blend_weighted: cubes are not on the same grid / dtype");
        S.v[i] = b->d_vals;
    }
    HIPCHECK(c, hipSetDevice(c->device));
    const int64_t total = a->ny * a->nx * a->nz;
    const void* dwt;
    int rc = stage_in(c, SLOT_IN0, weights, (size_t)total * nd * 8, loc, &dwt); if (rc) return rc;
    rdr_cube* q = new rdr_cube();
    q->ctx = c; q->ny = a->ny; q->nx = a->nx; q->nz = a->nz; q->dtype = RDR_F64;
    q->ys = a->ys; q->xs = a->xs; q->zs = a->zs; q->proj = a->proj;
    rc = cube_alloc(c, q);
    if (rc) { rdr_cube_destroy(q); return rc; }
    const int g = grid_for(total, 256, c->num_cus * 8);
    {
        KTimer t(c, 3);
        by_dtype(a, [&](auto t) { hipLaunchKernelGGL((blend_weighted_kernel<decltype(t)>), dim3(g), dim3(256), 0, c->stream, S, (const double*)dwt, a->ny, a->nx, a->nz, (double2*)q->d_vals); });
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { rdr_cube_destroy(q); return fail(c, RDR_ERR_HIP, hipGetErrorString(e)); }
    *out = q;
    return RDR_OK;
}

// ---- GUNW phase conversion (aria/calcGUNW.py:54-59): delay [m] -> interferometric phase [rad] ------------------------
// ds['wet'] * phase2range with phase2range = -4 pi / wavelength; a Python float is a weak scalar, so f32 delays are
// multiplied in f32 by the f32-rounded factor and f64 delays in f64.
template <typename T>
__global__ __launch_bounds__(256) void phase_kernel(const T* __restrict__ wet, const T* __restrict__ hyd, int64_t n, T factor,
                                                    T* __restrict__ owet, T* __restrict__ ohyd) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        owet[i] = wet[i] * factor;
        ohyd[i] = hyd[i] * factor;
    }
}

int rdr_delays_to_phase(rdr_ctx* c, const void* wet, const void* hydro, int64_t n, int dtype, double wavelength, void* wet_out, void* hydro_out, int loc) {
    if (!c || !wet || !hydro || !wet_out || !hydro_out) return fail(c, RDR_ERR_INVALID, "rdr_delays_to_phase: NULL argument");
    if (dtype != RDR_F32 && dtype != RDR_F64) return fail(c, RDR_ERR_INVALID, "rdr_delays_to_phase: dtype must be RDR_F32 or RDR_F64");
    if (!(wavelength > 0.0)) return fail(c, RDR_ERR_INVALID, "rdr_delays_to_phase: wavelength must be positive");
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_delays_to_phase: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * (dtype == RDR_F32 ? 4 : 8);
    Staged S(c, loc);
    const void *dw = S.in(wet, bytes), *dh = S.in(hydro, bytes);
    void *ow = S.out(wet_out, bytes), *oh = S.out(hydro_out, bytes);
    if (S.rc) return S.rc;
    const double phase2range = (-4.0 * 3.141592653589793) / wavelength;       // calcGUNW.py:54
    const int g = grid_for(n, 256, c->num_cus * 8);
    if (dtype == RDR_F32)
        hipLaunchKernelGGL(phase_kernel<float>, dim3(g), dim3(256), 0, c->stream, (const float*)dw, (const float*)dh, n, (float)phase2range, (float*)ow, (float*)oh);
    else
        hipLaunchKernelGGL(phase_kernel<double>, dim3(g), dim3(256), 0, c->stream, (const double*)dw, (const double*)dh, n, phase2range, (double*)ow, (double*)oh);
    return S.finish();
}

int rdr_cube_read(rdr_ctx* c, const rdr_cube* q, void* wet, void* hydro) {
    if (!c || !q || !wet || !hydro) return fail(c, RDR_ERR_INVALID, "rdr_cube_read: NULL argument");
    note_use(c, q);
    HIPCHECK(c, hipSetDevice(c->device));
    const int64_t total = q->ny * q->nx * q->nz;
    const size_t esz = q->dtype == RDR_F32 ? 4 : 8;
    void *dw, *dh;
    int rc = ensure(c, SLOT_OUT0, total * esz, &dw); if (rc) return rc;
    rc = ensure(c, SLOT_OUT1, total * esz, &dh); if (rc) return rc;
    const int g = grid_for(total, 256, c->num_cus * 8);
    by_dtype(q, [&](auto tag) {
        typedef decltype(tag) T2; typedef decltype(tag.x) T;
        hipLaunchKernelGGL((unpack_cube_kernel<T, T2>), dim3(g), dim3(256), 0, c->stream, (const T2*)q->d_vals, (T*)dw, (T*)dh, total);
    });
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(wet, dw, total * esz, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpyAsync(hydro, dh, total * esz, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

// ---- zenith / projected ---------------------------------------------------------------------------
// ---- corner-quad copy (cube_kernels.h): when, and how --------------------------------------------------------------------------
static size_t quad_need_bytes(const rdr_cube* q, int* nblk) {
    const int cpb = q->dtype == RDR_F32 ? Quad<float2>::CPB : Quad<double2>::CPB;
    *nblk = (int)((q->nz - 1 + cpb - 1) / cpb);
    return (size_t)(q->ny - 1) * (size_t)(q->nx - 1) * (size_t)*nblk * 128;
}

static int quad_build(rdr_ctx* c, const rdr_cube* q_any) {
    const rdr_cube* const q = root(q_any);              // (the copy belongs to the buffers, i.e. to the source of a view)
    // (one builder per cube: two contexts sharing a cube must not both allocate and publish a copy)
    std::lock_guard<std::mutex> guard(q->quad_mutex);
    if (q->d_quad) return RDR_OK;
    int nblk = 0;
    const size_t need = quad_need_bytes(q, &nblk);
    void* dq = nullptr;
    { const int rc_ = dev_malloc(c, &dq, need); if (rc_) return rc_; }
    struct Pub { const rdr_cube* q; void* p; size_t need; int nblk; bool ok = false;
                 ~Pub() { if (ok) { q->quad_bytes = need; q->quad_nblk = nblk; q->d_quad = p; } else (void)hipFree(p); } } pub{q, dq, need, nblk};
    const int64_t parts = (int64_t)(need / 16);
    const int g = (grid_for(parts, 256, c->num_cus * 32) + 7) / 8 * 8;       // a multiple of 8: one share of the ranges per XCD (quad_build_kernel)
    by_dtype(q, [&](auto t) { hipLaunchKernelGGL((quad_build_kernel<decltype(t)>), dim3(g), dim3(256), 0, c->stream, (const decltype(t)*)q->d_vals, (int)q->ny, (int)q->nx, (int)q->nz, nblk, (uint4*)dq); });
    HIPCHECK(c, hipGetLastError());
    // one-time, like rdr_cube_create: the copy must be complete before it is PUBLISHED - any other stream (a context switched to
    // torch's stream, a second context sharing the cube) may read it from then on.  0.7 ms of a build that happens once per cube.
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    pub.ok = true;
    return RDR_OK;
}

// Policy of the automatic build: only for point sets and cubes large enough that the four-lines-per-point gather is what bounds
// the call (>= 256 k points, a cube beyond 192 MB - smaller ones live in L2 / the 256 MB Infinity Cache), only when the copy fits a quarter
// of the free memory.  When: by TIME, from the measured rates (profiles/r03_secondary.json, r04_secondary.json: 5 M stations on the
// 400 MB HRRR-sized cube) - the direct gather moves 572 B per point at 6.5 TB/s (88 ps), the quad gather 168 B at 5.65 TB/s (30 ps),
// the build writes the copy at 3.0 TB/s: building at the FIRST large call pays when n x 58 ps > bytes / 3.0 TB/s, i.e. n x 175 B >
// the copy's bytes (12 M points for that cube; a 5 M-station one-shot is FASTER from the (y,x,z) cube: 0.43 ms against 0.72 + 0.15 -
// fewer HBM bytes per point is not the goal, time is), else from the second large call on the cube (then the copy has paid for itself
// by the end of that call).  RAIDER_HIP_POINT_INDEX=0 never, =1 at the first large call, =2 second call only.
static bool quad_wanted(rdr_ctx* c, const rdr_cube* q_any, int64_t n) {
    const rdr_cube* const q = root(q_any);
    if (q->d_quad) return true;
    static const int env = []() { const char* e = std::getenv("RAIDER_HIP_POINT_INDEX"); return e ? std::atoi(e) : -1; }();
    if (env == 0) return false;
    const size_t cube_bytes = (size_t)q->ny * q->nx * q->nz * (q->dtype == RDR_F32 ? 8 : 16);
    // (round 5: 32 MB -> 192 MB.  A 38.8 MB f64 cube - the intermediate delay cube of BASELINE configs[1] - is Infinity-Cache resident: 10^6
    // points from it take 23.7 us directly, 32.0 us from the copy, which also costs 54 us to build; profiles/r05_c2_counters.json at 458657a3)
    if (n < (1 << 18) || cube_bytes < ((size_t)192 << 20) || q->ny < 2 || q->nx < 2 || q->nz < 2) return false;
    int nblk; const size_t need = quad_need_bytes(q, &nblk);
    const bool pays_now = env != 2 && (double)n * 175.0 > (double)need;
    if (++q->big_point_calls < 2 && env != 1 && !pays_now) return false;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b / 4) return false;
    (void)c;
    return true;
}

int rdr_cube_point_index(rdr_ctx* c, rdr_cube* q_any, int mode) {
    if (!c || !q_any) return fail(c, RDR_ERR_INVALID, "rdr_cube_point_index: NULL argument");
    const rdr_cube* const q = root(q_any);
    note_use(c, q);
    HIPCHECK(c, hipSetDevice(c->device));
    if (mode == 0) {
        std::lock_guard<std::mutex> guard(q->quad_mutex);
        if (q->d_quad) { HIPCHECK(c, q->foreign.load() ? hipDeviceSynchronize() : hipStreamSynchronize(c->stream)); HIPCHECK(c, hipFree(q->d_quad)); q->d_quad = nullptr; q->quad_bytes = 0; q->quad_nblk = 0; }
        q->big_point_calls = 0;
        return RDR_OK;
    }
    if (mode != 1) return fail(c, RDR_ERR_INVALID, "rdr_cube_point_index: mode is 0 (free) or 1 (build)");
    if (q->ny < 2 || q->nx < 2 || q->nz < 2) return fail(c, RDR_ERR_INVALID, "rdr_cube_point_index: the cube needs two nodes per axis");
    return quad_build(c, q);
}

int64_t rdr_cube_point_index_bytes(const rdr_cube* q) { return q ? (int64_t)root(q)->quad_bytes : -1; }

// a second epoch blended in at the corners (rdr_interp3_blend): vb == NULL for an ordinary gather
// pair != NULL: the blend was made as a PAIRED cube in the context's scratch (rdr_interp3_blend_cube) - the gather reads that
struct BlendSpec { const void* vb = nullptr; double w1 = 1.0, w2 = 0.0; const void* pair = nullptr; bool want_pair = false; };

static void launch_interp(rdr_ctx* c, const rdr_cube* q, const PointQuery& Qk, int64_t cnt, double* dwk, double* dhk, bool quad, const BlendSpec& B = BlendSpec()) {
    const int g = grid_for(cnt, 256, c->num_cus * 8);
    KTimer t(c, 2);
    by_dtype(q, [&](auto tag) {
        typedef decltype(tag) T2;
        const CubeView<T2> v = make_view<T2>(q);
        const int lds = (int)axes_fit_lds(q);
        if (B.pair)
            hipLaunchKernelGGL((interp_points_pair_kernel<T2>), dim3(g), dim3(256), axes_smem(q), c->stream, v, (const T2*)B.pair, Qk, cnt, dwk, dhk, lds);
        else if (B.vb)
            hipLaunchKernelGGL((interp_points_blend_kernel<T2>), dim3(g), dim3(256), axes_smem(q), c->stream, v, (const T2*)B.vb, B.w1, B.w2, Qk, cnt, dwk, dhk, lds);
        else if (quad)
            hipLaunchKernelGGL((interp_points_quad_kernel<T2>), dim3(g), dim3(256), axes_smem(q), c->stream, v, (const uint4*)root(q)->d_quad, root(q)->quad_nblk,
                               Qk, cnt, dwk, dhk, lds);
        else
            hipLaunchKernelGGL((interp_points_kernel<T2>), dim3(g), dim3(256), axes_smem(q), c->stream, v, Qk, cnt, dwk, dhk, lds);
    });
}

// An error return must not leave asynchronous copies into (or out of) the caller's buffers in flight: whoever enqueued on the three
// streams arms this; leaving the scope on any path but the disarmed one waits for all of them.
struct StreamsQuiesce {
    rdr_ctx* c; bool armed = true;
    explicit StreamsQuiesce(rdr_ctx* ctx) : c(ctx) {}
    ~StreamsQuiesce() {
        if (!armed) return;
        (void)hipStreamSynchronize(c->down_stream); (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
    }
};

// The events of one pipelined call, destroyed on every exit path.  Declared BEFORE the call's StreamsQuiesce: they are then destroyed
// only once the streams are idle.
struct EventList {
    std::vector<hipEvent_t> v;
    ~EventList() { for (auto& e : v) if (e) (void)hipEventDestroy(e); }
    bool add(size_t n) {                        // n more events (no timing); false: one of them could not be created
        for (size_t i = 0; i < n; ++i) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
            v.push_back(e);
        }
        return true;
    }
};

// Large HOST point sets: the points go up (copy stream) and the delays come down (download stream) in chunks, the download of chunk k
// under the upload of chunk k+1 (PCIe is full duplex), the gathers on the ctx stream in between - 40-48 B per point cross the link,
// which is all such a call costs (the gather itself: 0.03 ms per 10^6 points).  Uploads on their OWN stream also run under whatever
// the ctx stream is still doing (rdr_point_delays: the build of the intermediate cube).  `slots`: device scratch for y, x, z, proj,
// wet, hydro.  Synchronises all three streams before it returns.  (A download into pageable memory blocks the host thread instead of
// overlapping: still correct.)
// One cube (vals == NULL, D = 1: launch_interp with its quad / blend variants) or a date series (vals[D]: the value buffers of D cubes on
// q's grid, launch_interp_epochs): chunk k of the points - and of a shared divisor - goes up ONCE, the epoch groups gather from it, the D
// result chunks (wet / hydro are [D][n]) come down.  pstride == n: per-date divisors proj[D][n] go up with their chunk, D pieces.
// Every host-to-device copy of points and divisors is counted in c->point_upload_bytes.
static void launch_interp_epochs(rdr_ctx* c, const rdr_cube* q, const void* const* vals, int D, const PointQuery& Q, int64_t pstride, int64_t cnt, int64_t estride,
                                 double* dw, double* dh);
static int interp_pipeline_impl(rdr_ctx* c, const char* who, const rdr_cube* q, bool quad, const BlendSpec& B, const void* const* vals, int D, const double* y,
                                const double* x, const double* z, int64_t n, PointQuery Q, const double* proj, int64_t pstride, double* wet, double* hydro,
                                const int* slots) {
    const bool has_proj = Q.pmode == 1 || Q.pmode == 3;
    const size_t ystride = x ? 1 : 3;
    const int64_t np = pstride ? D : 1;
    void *dy, *dx = nullptr, *dz = nullptr, *dp = nullptr, *dw = nullptr, *dh = nullptr;
    int rc = ensure(c, slots[0], (size_t)n * ystride * 8, &dy); if (rc) return rc;
    if (x) { rc = ensure(c, slots[1], (size_t)n * 8, &dx); if (rc) return rc; rc = ensure(c, slots[2], (size_t)n * 8, &dz); if (rc) return rc; }
    if (has_proj) { rc = ensure(c, slots[3], (size_t)n * np * 8, &dp); if (rc) return rc; }
    if (wet) { rc = ensure(c, slots[4], (size_t)n * D * 8, &dw); if (rc) return rc; }
    if (hydro) { rc = ensure(c, slots[5], (size_t)n * D * 8, &dh); if (rc) return rc; }
    // chunks of >= 512 k points (a copy call costs 10-20 us: 1 MB copies would spend as long on calls as on bytes), at most 8
    const int nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(8, n >> 19));
    EventList evs;
    if (!evs.add((size_t)2 * nchunk)) return fail(c, RDR_ERR_HIP, std::string(who) + ": event creation failed");
    StreamsQuiesce quiesce(c);                  // (declared after the events: they are destroyed only once the streams are idle)
    auto up = [&](void* dst, const void* src, size_t bytes) {
        c->point_upload_bytes += (int64_t)bytes;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->copy_stream);
    };
    for (int k = 0; k < nchunk; ++k) {
        const int64_t o = n * k / nchunk, cnt = n * (k + 1) / nchunk - o;
        HIPCHECK(c, up((double*)dy + o * ystride, y + o * ystride, (size_t)cnt * ystride * 8));
        if (x) {
            HIPCHECK(c, up((double*)dx + o, x + o, (size_t)cnt * 8));
            HIPCHECK(c, up((double*)dz + o, z + o, (size_t)cnt * 8));
        }
        if (has_proj)
            for (int64_t e = 0; e < np; ++e) HIPCHECK(c, up((double*)dp + e * n + o, proj + e * n + o, (size_t)cnt * 8));
        HIPCHECK(c, hipEventRecord(evs.v[2 * k], c->copy_stream));
        HIPCHECK(c, hipStreamWaitEvent(c->stream, evs.v[2 * k], 0));
        PointQuery Qk = Q;
        Qk.y = (const double*)dy + o * ystride;
        Qk.x = x ? (const double*)dx + o : nullptr; Qk.z = x ? (const double*)dz + o : nullptr;
        Qk.proj = has_proj ? (const double*)dp + o : nullptr;
        double* const dwk = dw ? (double*)dw + o : nullptr;
        double* const dhk = dh ? (double*)dh + o : nullptr;
        if (vals) launch_interp_epochs(c, q, vals, D, Qk, pstride, cnt, n, dwk, dhk);
        else launch_interp(c, q, Qk, cnt, dwk, dhk, quad, B);
        HIPCHECK(c, hipGetLastError());
        HIPCHECK(c, hipEventRecord(evs.v[2 * k + 1], c->stream));
        HIPCHECK(c, hipStreamWaitEvent(c->down_stream, evs.v[2 * k + 1], 0));
        for (int64_t e = 0; e < D; ++e) {
            if (wet) HIPCHECK(c, hipMemcpyAsync(wet + e * n + o, (double*)dw + e * n + o, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->down_stream));
            if (hydro) HIPCHECK(c, hipMemcpyAsync(hydro + e * n + o, (double*)dh + e * n + o, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->down_stream));
        }
    }
    HIPCHECK(c, hipStreamSynchronize(c->down_stream));
    HIPCHECK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    quiesce.armed = false;
    return RDR_OK;
}

static int interp_pipeline(rdr_ctx* c, const char* who, const rdr_cube* q, bool quad, const double* y, const double* x, const double* z, int64_t n,
                           PointQuery Q, const double* proj, double* wet, double* hydro, const int* slots, const BlendSpec& B = BlendSpec()) {
    return interp_pipeline_impl(c, who, q, quad, B, nullptr, 1, y, x, z, n, Q, proj, 0, wet, hydro, slots);
}

static int point_query_args(rdr_ctx* c, const char* who, const double* y, const double* x, const double* z, int64_t n, int pmode, const double* proj,
                            const double* wet, const double* hydro) {
    if (n < 0) return fail(c, RDR_ERR_INVALID, std::string(who) + ": negative count");
    if (n > 0 && (!y || (x && !z) || (!x && z) || (!wet && !hydro))) return fail(c, RDR_ERR_INVALID, std::string(who) + ": NULL argument");
    if (pmode < 0 || pmode > 3) return fail(c, RDR_ERR_INVALID, std::string(who) + ": proj_mode is 0 (none), 1 (incidence array), 2 (one incidence) or 3 (divisor array)");
    if (n > 0 && (pmode == 1 || pmode == 3) && !proj) return fail(c, RDR_ERR_INVALID, std::string(who) + ": proj_mode 1 / 3 need the proj array");
    return RDR_OK;
}

// stage_in for query points and divisors: what is really copied from the host is counted (rdr_point_upload_bytes)
static int stage_points_in(rdr_ctx* ctx, int s, const void* src, size_t bytes, int loc, const void** dev) {
    if (src && loc != RDR_DEVICE) ctx->point_upload_bytes += (int64_t)bytes;
    return stage_in(ctx, s, src, bytes, loc, dev);
}

// the pipelined gather's scratch (y, x, z, proj, wet, hydro) of the gather entries, and of the point-delay drivers (whose build holds the others)
static const int k_gather_slots[6] = {SLOT_IN0, SLOT_IN1, SLOT_IN2, SLOT_IN3, SLOT_OUT0, SLOT_OUT1};
static const int k_point_slots[6] = {SLOT_PT0, SLOT_PT1, SLOT_PT2, SLOT_PT3, SLOT_PT4, SLOT_PT5};

static PointQuery make_query(int pmode, double inc0) {
    PointQuery Q; std::memset(&Q, 0, sizeof(Q));
    Q.pmode = pmode; Q.inc0 = inc0;
    return Q;
}

// The gather of n points at `loc` for D dates, NOT pipelined, in this order: y, x, z and the divisors (pstride == n: D blocks of them)
// through stage_points_in - so counted - into SLOT_IN0..3, the [D][n] outputs staged in SLOT_OUT0 / 1, launch(Q, dw, dh) and its error,
// the downloads, the host's wait when the outputs are its own.
template <typename Launch>
static int gather_staged(rdr_ctx* c, PointQuery Q, const double* y, const double* x, const double* z, const double* proj, int64_t pstride, int64_t n, int D,
                         double* wet, double* hydro, int loc, Launch&& launch) {
    const size_t ystride = x ? 1 : 3;                                  // doubles per point behind `y`
    const size_t np = pstride ? (size_t)D : 1, obytes = (size_t)n * (size_t)D * 8;
    const void* d; void *dw = nullptr, *dh = nullptr;
    int rc = stage_points_in(c, SLOT_IN0, y, (size_t)n * ystride * 8, loc, &d); if (rc) return rc; Q.y = (const double*)d;
    if (x) {
        rc = stage_points_in(c, SLOT_IN1, x, (size_t)n * 8, loc, &d); if (rc) return rc; Q.x = (const double*)d;
        rc = stage_points_in(c, SLOT_IN2, z, (size_t)n * 8, loc, &d); if (rc) return rc; Q.z = (const double*)d;
    }
    if (Q.pmode == 1 || Q.pmode == 3) { rc = stage_points_in(c, SLOT_IN3, proj, (size_t)n * np * 8, loc, &d); if (rc) return rc; Q.proj = (const double*)d; }
    if (wet) { rc = stage_out(c, SLOT_OUT0, wet, obytes, loc, &dw); if (rc) return rc; }
    if (hydro) { rc = stage_out(c, SLOT_OUT1, hydro, obytes, loc, &dh); if (rc) return rc; }
    launch(Q, (double*)dw, (double*)dh);
    HIPCHECK(c, hipGetLastError());
    rc = finish_out(c, wet, dw, obytes, loc); if (rc) return rc;
    rc = finish_out(c, hydro, dh, obytes, loc); if (rc) return rc;
    if (loc == RDR_HOST) HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

// the point query behind rdr_interp3 / rdr_interp3_project: y/x/z three arrays (x != NULL) or y = packed (n,3); pmode / proj / inc0 as
// PointQuery (cube_kernels.h); either output may be NULL (it is then neither written nor downloaded)
static int interp3_impl(rdr_ctx* c, const char* who, const rdr_cube* q, const double* y, const double* x, const double* z, int64_t n, int pmode,
                        const double* proj, double inc0, double* wet, double* hydro, int loc, const BlendSpec& B_in = BlendSpec()) {
    if (!c || !q) return fail(c, RDR_ERR_INVALID, std::string(who) + ": NULL argument");
    note_use(c, q);
    int rc = point_query_args(c, who, y, x, z, n, pmode, proj, wet, hydro); if (rc) return rc;
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    BlendSpec B = B_in;
    if (B.want_pair) {
        // the blend as a cube, written ONCE in the layout the gather reads best (blend_pair_kernel), into the context's scratch: it never
        // becomes an rdr_cube, so no other kernel can be handed the paired layout
        const size_t esz = q->dtype == RDR_F32 ? 8 : 16;
        const int64_t npx = (q->nx + 1) / 2;
        void* dp;
        rc = ensure(c, SLOT_TMPCUBE, (size_t)q->ny * npx * q->nz * 2 * esz, &dp); if (rc) return rc;
        const int zv = (q->dtype == RDR_F32 && q->nz % 2 == 0) ? 2 : 1;
        const int g = grid_for(q->ny * npx * (q->nz / zv), 256, 1 << 22);
        {
            KTimer t(c, 3);
            by_dtype(q, [&](auto tag) {
                typedef decltype(tag) T2;
                typedef decltype(tag.x) T;
                auto launch = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3(g), dim3(256), 0, c->stream, (const T2*)q->d_vals, (T)B.w1, (const T2*)B.vb, (T)B.w2, (T2*)dp, (int)q->ny, (int)q->nx,
                                       (int)q->nz);
                };
                if constexpr (sizeof(T) == 4) { if (zv == 2) return launch(blend_pair_kernel<float2, 2>); }
                launch(blend_pair_kernel<T2, 1>);
            });
        }
        HIPCHECK(c, hipGetLastError());
        B.pair = dp;
    }
    const PointQuery Q = make_query(pmode, inc0);
    const bool quad = !B.vb && quad_wanted(c, q, n);
    if (quad) { rc = quad_build(c, q); if (rc) return rc; }
    if (loc == RDR_HOST && n >= (1 << 18) && pipelining()) {
        return interp_pipeline(c, who, q, quad, y, x, z, n, Q, proj, wet, hydro, k_gather_slots, B);
    }
    return gather_staged(c, Q, y, x, z, proj, 0, n, 1, wet, hydro, loc,
                         [&](const PointQuery& Qd, double* dw, double* dh) { launch_interp(c, q, Qd, n, dw, dh, quad, B); });
}

int rdr_interp3(rdr_ctx* c, const rdr_cube* q, const double* pts, int64_t n, double* wet, double* hydro, int loc) {
    return interp3_impl(c, "rdr_interp3", q, pts, nullptr, nullptr, n, 0, nullptr, 0.0, wet, hydro, loc);
}

int rdr_interp3_blend(rdr_ctx* c, const rdr_cube* a, double w1, const rdr_cube* b, double w2, const double* y, const double* x, const double* z, int64_t n,
                      double* wet, double* hydro, int loc) {
    if (!c || !a || !b) return fail(c, RDR_ERR_INVALID, "rdr_interp3_blend: NULL argument");
    note_use(c, b);
    if (!same_grid_dtype(a, b))
        return fail(c, RDR_ERR_INVALID, "rdr_interp3_blend: the two epochs are not on the same grid / dtype");
    BlendSpec B; B.vb = b->d_vals; B.w1 = w1; B.w2 = w2;
    return interp3_impl(c, "rdr_interp3_blend", a, y, x, z, n, 0, nullptr, 0.0, wet, hydro, loc, B);
}

int rdr_interp3_blend_cube(rdr_ctx* c, const rdr_cube* a, double w1, const rdr_cube* b, double w2, const double* y, const double* x, const double* z, int64_t n,
                           double* wet, double* hydro, int loc) {
    if (!c || !a || !b) return fail(c, RDR_ERR_INVALID, "rdr_interp3_blend_cube: NULL argument");
    note_use(c, b);
    if (!same_grid_dtype(a, b))
        return fail(c, RDR_ERR_INVALID, "rdr_interp3_blend_cube: the two epochs are not on the same grid / dtype");
    if (a->ny > INT32_MAX || a->nx > INT32_MAX || a->nz > INT32_MAX) return fail(c, RDR_ERR_INVALID, "rdr_interp3_blend_cube: axis longer than 2^31");
    BlendSpec B; B.vb = b->d_vals; B.w1 = w1; B.w2 = w2; B.want_pair = true;
    return interp3_impl(c, "rdr_interp3_blend_cube", a, y, x, z, n, 0, nullptr, 0.0, wet, hydro, loc, B);
}

int rdr_interp3_project(rdr_ctx* c, const rdr_cube* q, const double* y, const double* x, const double* z, int64_t n, int proj_mode,
                        const double* proj, double inc0, double* wet, double* hydro, int loc) {
    return interp3_impl(c, "rdr_interp3_project", q, y, x, z, n, proj_mode, proj, inc0, wet, hydro, loc);
}

// _build_cube (delay.py:196-216).  keep == NULL: the public entry (results to the caller's wet / hydro at `loc`); keep != NULL: the results
// stay in the context's scratch (planar (z,y,x), keep[0] = wet, keep[1] = hydro) for rdr_build_cube_to_cube, nothing is downloaded.
static int build_cube_impl(rdr_ctx* c, const rdr_cube* q, const double* xpts, int64_t nx, const double* ypts, int64_t ny,
                           const double* zpts, int64_t nz, double* wet, double* hydro, int loc, double** keep, const double** dev_yxz = nullptr,
                           const GridCrs* grid = nullptr) {
    if (!c || !q || !xpts || !ypts || !zpts || (!keep && (!wet || !hydro))) return fail(c, RDR_ERR_INVALID, "rdr_build_cube: NULL argument");
    note_use(c, q);
    if (nx < 0 || ny < 0 || nz < 0) return fail(c, RDR_ERR_INVALID, "rdr_build_cube: negative count");
    const int64_t n = nx * ny * nz;
    c->last_nan_output = -1;                  // (also for an empty build: the previous call's verdict is not this one's)
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    const void *dx, *dy, *dz; void *dw, *dh;
    int rc;
    if (loc == RDR_HOST) {                        // the three axes in one slot, one copy
        void* d;
        rc = ensure(c, SLOT_IN0, (size_t)(nx + ny + nz) * 8, &d); if (rc) return rc;
        const HostPart parts[3] = {{xpts, (size_t)nx * 8}, {ypts, (size_t)ny * 8}, {zpts, (size_t)nz * 8}};
        rc = upload_parts(c, d, parts, 3); if (rc) return rc;
        dx = d; dy = static_cast<const double*>(d) + nx; dz = static_cast<const double*>(d) + nx + ny;
    } else { dx = xpts; dy = ypts; dz = zpts; }
    if (dev_yxz) { dev_yxz[0] = (const double*)dy; dev_yxz[1] = (const double*)dx; dev_yxz[2] = (const double*)dz; }
    rc = stage_out(c, SLOT_OUT0, wet, (size_t)n * 8, keep ? RDR_HOST : loc, &dw); if (rc) return rc;
    rc = stage_out(c, SLOT_OUT1, hydro, (size_t)n * 8, keep ? RDR_HOST : loc, &dh); if (rc) return rc;
    // Setup kernel: per-node and per-height records (24 B / 16 B) into scratch; then the gather: 64 x 4-node tiles x chunks of
    // heights - enough chunks that a small grid still fills the chip, as few as possible otherwise.
    const int64_t nodes = nx * ny;
    void *dn, *dl;
    rc = ensure(c, SLOT_IN3, (size_t)nodes * sizeof(BuildNode), &dn); if (rc) return rc;
    rc = ensure(c, SLOT_IN4, (size_t)nz * sizeof(BuildLevel), &dl); if (rc) return rc;
    double* tbl = nullptr;                        // a projected grid (rdr_build_cube_grid): its nodes in the cube's CRS, 4 x 8 B per node of scratch
    if (grid) { void* t; rc = ensure(c, SLOT_IN1, (size_t)nodes * 32, &t); if (rc) return rc; tbl = (double*)t; }
    const int64_t ntile = ((nx + 63) / 64) * ((ny + 3) / 4);
    const int64_t want_tiles = (int64_t)c->num_cus * 8;
    int64_t nchunks = std::min<int64_t>(nz, std::max<int64_t>(1, (want_tiles + ntile - 1) / ntile));
    nchunks = std::max<int64_t>(nchunks, (nz + BUILD_ZCHUNK_MAX - 1) / BUILD_ZCHUNK_MAX);      // the per-height table of a chunk lives in LDS
    if (nchunks > 65535) return fail(c, RDR_ERR_INVALID, "rdr_build_cube: more than 65535 x 1024 heights");
    const int64_t zchunk = (nz + nchunks - 1) / nchunks;
    nchunks = (nz + zchunk - 1) / zchunk;
    const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(ntile, (int64_t)c->num_cus * 16)), (unsigned)nchunks);
    // staging area of the tile footprint | per-height z weights (8 B) and cells (4 B) | footprint bounds + flag
    const size_t sm = (size_t)BUILD_STAGE_BYTES + (size_t)zchunk * 12 + 32;
    {
        KTimer t(c, 2);
        const int gs = grid_for(nodes + nz, 256, c->num_cus * 8);
        const double *qy = nullptr, *qx = nullptr;
        if (grid) { rc = grid_nodes(c, *grid, (const double*)dx, nx, (const double*)dy, ny, &q->proj, tbl, tbl + nodes, tbl + 2 * nodes, tbl + 3 * nodes, &qy, &qx); if (rc) return rc; }
        const hipError_t e = by_dtype(q, [&](auto tag) {
            typedef decltype(tag) T2;
            hipError_t e_;
            if (grid)
                e_ = launch_lds(build_cube_setup_table_kernel<T2>, dim3(gs), dim3(256), axes_smem(q), c->stream, make_view<T2>(q), qy, qx, nodes,
                                (const double*)dz, nz, (BuildNode*)dn, (BuildLevel*)dl, (int)axes_fit_lds(q));
            else
                e_ = launch_lds(build_cube_setup_kernel<T2>, dim3(gs), dim3(256), axes_smem(q), c->stream, make_view<T2>(q), q->proj, (const double*)dx, nx,
                                (const double*)dy, ny, (const double*)dz, nz, (BuildNode*)dn, (BuildLevel*)dl, (int)axes_fit_lds(q));
            if (e_ == hipSuccess)
                e_ = launch_lds(build_cube_kernel<T2>, g, dim3(256), sm, c->stream, (const T2*)q->d_vals, (int)q->ny, (int)q->nx, (int)q->nz,
                                (const BuildNode*)dn, (const BuildLevel*)dl, nx, ny, nz, zchunk, (double*)dw, (double*)dh);
            return e_;
        });
        if (e != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("build_cube_kernel launch: ") + hipGetErrorString(e));
    }
    if (keep) { keep[0] = (double*)dw; keep[1] = (double*)dh; return RDR_OK; }
    // np.isnan(result).any() (delay.py:187) answered here, before the outputs leave the device (rdr_last_nan_output)
    int* const nf = c->d_flags + MAX_SLICES + 1;
    if (loc == RDR_HOST) {
        HIPCHECK(c, hipMemsetAsync(nf, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(nan_scan_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, (const double*)dw, (const double*)dh, n, n, nf);
        HIPCHECK(c, hipGetLastError());
    }
    rc = finish_out(c, wet, dw, (size_t)n * 8, loc); if (rc) return rc;
    rc = finish_out(c, hydro, dh, (size_t)n * 8, loc); if (rc) return rc;
    if (loc == RDR_HOST) {
        int f = 0;
        HIPCHECK(c, hipMemcpyAsync(&f, nf, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        c->last_nan_output = (f & 64) ? 1 : 0;
    }
    return RDR_OK;
}

int rdr_build_cube(rdr_ctx* c, const rdr_cube* q, const double* xpts, int64_t nx, const double* ypts, int64_t ny,
                   const double* zpts, int64_t nz, double* wet, double* hydro, int loc) {
    return build_cube_impl(c, q, xpts, nx, ypts, ny, zpts, nz, wet, hydro, loc, nullptr);
}

int rdr_build_cube_grid(rdr_ctx* c, const rdr_cube* q, int grid_kind, const double* params, int nparams, const double* xpts, int64_t nx,
                        const double* ypts, int64_t ny, const double* zpts, int64_t nz, double* wet, double* hydro, int loc) {
    if (!c || !q || !xpts || !ypts || !zpts || !wet || !hydro) return fail(c, RDR_ERR_INVALID, "rdr_build_cube_grid: NULL argument");
    GridCrs g;
    int rc = grid_crs(c, "rdr_build_cube_grid", grid_kind, params, nparams, g); if (rc) return rc;
    rc = grid_counts(c, "rdr_build_cube_grid", nx, ny); if (rc) return rc;
    return build_cube_impl(c, q, xpts, nx, ypts, ny, zpts, nz, wet, hydro, loc, nullptr, nullptr, &g);
}

int rdr_last_nan_output(rdr_ctx* c) { return c ? c->last_nan_output : -1; }

// host copy of an axis given at `loc` (the cube keeps its axes on the host as well)
static int axis_to_host(rdr_ctx* c, const double* a, int64_t n, int loc, std::vector<double>& out) {
    out.resize((size_t)std::max<int64_t>(n, 0));
    if (n <= 0) return RDR_OK;
    if (loc == RDR_DEVICE) {
        HIPCHECK(c, hipMemcpyAsync(out.data(), a, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
    } else std::copy(a, a + n, out.begin());
    return RDR_OK;
}

static int build_to_cube(rdr_ctx* c, const char* who, const rdr_cube* q, const GridCrs* grid, const double* xpts, int64_t nx, const double* ypts,
                         int64_t ny, const double* zpts, int64_t nz, int loc, rdr_cube** out) {
    if (nx < 2 || ny < 2 || nz < 2) return fail(c, RDR_ERR_INVALID, std::string(who) + ": the delay cube needs two nodes per axis");
    HIPCHECK(c, hipSetDevice(c->device));
    std::vector<double> hx, hy, hz;
    int rc = axis_to_host(c, xpts, nx, loc, hx); if (rc) return rc;
    rc = axis_to_host(c, ypts, ny, loc, hy); if (rc) return rc;
    rc = axis_to_host(c, zpts, nz, loc, hz); if (rc) return rc;
    double* planar[2] = {nullptr, nullptr};
    const double* dev_yxz[3] = {nullptr, nullptr, nullptr};       // the axes as the build has them on the device (scratch slot / the caller's arrays)
    rc = build_cube_impl(c, q, xpts, nx, ypts, ny, zpts, nz, nullptr, nullptr, loc, planar, dev_yxz, grid); if (rc) return rc;
    // planar (z,y,x) results -> interleaved (y,x,z) cube with axes (ypts, xpts, zpts): what getInterpolators(ds, 'ztd') builds from the
    // Dataset of writeResultsToXarray (delay.py:113, delayFcns.py:40-41), descending axes flipped as scipy does; its NaN scan
    // (delayFcns.py:50-52 on this cube == np.isnan(result).any(), delay.py:187) comes with the packing
    return cube_create_impl(c, hy.data(), ny, hx.data(), nx, hz.data(), nz, planar[0], planar[1], RDR_F64, nx, 1, ny * nx, RDR_DEVICE, out, dev_yxz);
}

int rdr_build_cube_to_cube(rdr_ctx* c, const rdr_cube* q, const double* xpts, int64_t nx, const double* ypts, int64_t ny,
                           const double* zpts, int64_t nz, int loc, rdr_cube** out) {
    if (!c || !q || !xpts || !ypts || !zpts || !out) return fail(c, RDR_ERR_INVALID, "rdr_build_cube_to_cube: NULL argument");
    return build_to_cube(c, "rdr_build_cube_to_cube", q, nullptr, xpts, nx, ypts, ny, zpts, nz, loc, out);
}

int rdr_build_cube_grid_to_cube(rdr_ctx* c, const rdr_cube* q, int grid_kind, const double* params, int nparams, const double* xpts, int64_t nx,
                                const double* ypts, int64_t ny, const double* zpts, int64_t nz, int loc, rdr_cube** out) {
    static const char* who = "rdr_build_cube_grid_to_cube";
    if (!c || !q || !xpts || !ypts || !zpts || !out) return fail(c, RDR_ERR_INVALID, "rdr_build_cube_grid_to_cube: NULL argument");
    GridCrs g;
    int rc = grid_crs(c, who, grid_kind, params, nparams, g); if (rc) return rc;
    rc = grid_counts(c, who, nx, ny); if (rc) return rc;
    return build_to_cube(c, who, q, &g, xpts, nx, ypts, ny, zpts, nz, loc, out);
}


// The intermediate cube of the point branch as a scratch object: shape and axes of the output grid (descending axes flipped as scipy
// does, fy / fx / fz say which), no buffers yet.  Returns non-zero when an axis is not strictly monotonic.
static int scratch_cube_init(rdr_cube& tmp, rdr_ctx* c, const double* xpts, int64_t nx, const double* ypts, int64_t ny, const double* zpts, int64_t nz,
                             int* fy, int* fx, int* fz) {
    if (axis_check(ypts, ny, fy) || axis_check(xpts, nx, fx) || axis_check(zpts, nz, fz)) return -1;
    tmp.ctx = c; tmp.ny = ny; tmp.nx = nx; tmp.nz = nz; tmp.dtype = RDR_F64;
    tmp.ys.assign(ypts, ypts + ny); tmp.xs.assign(xpts, xpts + nx); tmp.zs.assign(zpts, zpts + nz);
    if (*fy) std::reverse(tmp.ys.begin(), tmp.ys.end());
    if (*fx) std::reverse(tmp.xs.begin(), tmp.xs.end());
    if (*fz) std::reverse(tmp.zs.begin(), tmp.zs.end());
    axis_uniformity(tmp.ys, &tmp.uni[0], &tmp.inv_d[0], &tmp.exact[0]);
    axis_uniformity(tmp.xs, &tmp.uni[1], &tmp.inv_d[1], &tmp.exact[1]);
    axis_uniformity(tmp.zs, &tmp.uni[2], &tmp.inv_d[2]);
    return 0;
}

// what the point-delay drivers ask of their output grid
static int point_grid_args(rdr_ctx* c, const std::string& w, int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return fail(c, RDR_ERR_INVALID, w + ": the delay cube needs two nodes per axis");
    if (nz > MAX_LEVELS) return fail(c, RDR_ERR_INVALID, w + ": more than 512 height levels");
    if (ny + nx + nz > 100000) return fail(c, RDR_ERR_INVALID, w + ": axes too long");
    return RDR_OK;
}

// The intermediate cube(s) of the point-delay drivers, in this order: `tmp` described (scratch_cube_init), hipSetDevice, D value regions
// in SLOT_TMPCUBE (tmp.d_vals: the first), the axes' slot (tmp.d_axes), and ax = ys | xs | zs - which the CALLER sends up, on its
// stream and under its StreamsQuiesce.  Scratch objects: values and axes live in context slots, nothing is ever destroyed.
static int scratch_cube_setup(rdr_ctx* c, rdr_cube& tmp, const double* xpts, int64_t nx, const double* ypts, int64_t ny, const double* zpts, int64_t nz,
                              int D, int* fy, int* fx, int* fz, std::vector<double>& ax) {
    if (scratch_cube_init(tmp, c, xpts, nx, ypts, ny, zpts, nz, fy, fx, fz))
        return fail(c, RDR_ERR_INVALID, "The points in each dimension must be strictly ascending or descending (and >= 2)");
    HIPCHECK(c, hipSetDevice(c->device));
    void *dvals, *daxes;
    int rc = ensure(c, SLOT_TMPCUBE, (size_t)ny * nx * nz * sizeof(double2) * (size_t)D, &dvals); if (rc) return rc;
    rc = ensure(c, SLOT_TMPAXES, (size_t)(ny + nx + nz) * 8, &daxes); if (rc) return rc;
    tmp.d_vals = dvals; tmp.d_axes = (double*)daxes;
    ax.insert(ax.end(), tmp.ys.begin(), tmp.ys.end()); ax.insert(ax.end(), tmp.xs.begin(), tmp.xs.end()); ax.insert(ax.end(), tmp.zs.begin(), tmp.zs.end());
    return RDR_OK;
}

// planar (z, y, x) build results -> the interleaved (y, x, z) values of the intermediate cube, NaN verdict into *nf
static void pack_planar(rdr_ctx* c, double* const* planar, double2* dvals, int64_t ny, int64_t nx, int64_t nz, int fy, int fx, int fz, int* nf) {
    if (nx >= 8 && nz >= 8)        // x is contiguous - the LDS-transposing packer (cube_kernels.h)
        hipLaunchKernelGGL((pack_cube_xfast_kernel<double, double2, false>), dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ny * ((nx + 31) / 32) * ((nz + 31) / 32), (int64_t)c->num_cus * 16))),
                           dim3(256), 0, c->stream, (const double*)planar[0], (const double*)planar[1], dvals, ny, nx, nz, nx, ny * nx, fy, fx, fz, nf);
    else
        hipLaunchKernelGGL((pack_cube_kernel<double, double2, false>), dim3(grid_for(ny * nx * nz, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (const double*)planar[0], (const double*)planar[1], dvals, ny, nx, nz, nx, (int64_t)1, ny * nx, fy, fx, fz, nf);
}

// a large job's intermediates (16 B per cell of the cube + 16 B per cell of planar results) are not kept for the life of the context
static void scratch_trim_point_delays(rdr_ctx* c) {
    static const size_t keep = []() { const char* e = std::getenv("RAIDER_HIP_SCRATCH_KEEP_BYTES"); return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)4 << 30; }();
    for (int s_ : {SLOT_TMPCUBE, SLOT_OUT0, SLOT_OUT1}) {
        DevBuf& b = c->slot[s_];
        if (b.p && b.cap > keep) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    }
}

// tropo_delay's point branch for a zenith / projected line of sight (delay.py:96-128) in ONE call: _build_cube on the output grid
// (xpts, ypts, zpts) -> the intermediate cube packed as getInterpolators(ds, 'ztd') would wrap it -> trilinear gather at the query
// points -> delay / cos(inc).  Everything is enqueued before anything is waited for: the points travel up (copy stream) while the
// intermediate cube is built (ctx stream), the cube lives in the context's scratch (no allocation per call), its NaN verdict
// (delay.py:187) comes back with the final synchronisation.  Same kernels, same arithmetic as the separate entries: same bits.
static int point_delays_impl(rdr_ctx* c, const char* who, const rdr_cube* q, const GridCrs* grid, const double* xpts, int64_t nx, const double* ypts,
                             int64_t ny, const double* zpts, int64_t nz, const double* y, const double* x, const double* z, int64_t n, int proj_mode,
                             const double* proj, double inc0, double* wet, double* hydro, int32_t* cube_has_nan) {
    int rc = point_grid_args(c, who, nx, ny, nz); if (rc) return rc;
    rc = point_query_args(c, who, y, x, z, n, proj_mode, proj, wet, hydro); if (rc) return rc;
    int fy, fx, fz;
    rdr_cube tmp;
    std::vector<double> ax;
    rc = scratch_cube_setup(c, tmp, xpts, nx, ypts, ny, zpts, nz, 1, &fy, &fx, &fz, ax); if (rc) return rc;
    StreamsQuiesce quiesce(c);                  // (`ax`, the caller's points and outputs: nothing may still be copying when an error returns)
    HIPCHECK(c, hipMemcpyAsync(tmp.d_axes, ax.data(), ax.size() * 8, hipMemcpyHostToDevice, c->stream));
    double* planar[2] = {nullptr, nullptr};
    rc = build_cube_impl(c, q, xpts, nx, ypts, ny, zpts, nz, nullptr, nullptr, RDR_HOST, planar, nullptr, grid); if (rc) return rc;
    int* const nf = c->d_flags + MAX_SLICES + 2;
    HIPCHECK(c, hipMemsetAsync(nf, 0, sizeof(int), c->stream));
    pack_planar(c, planar, (double2*)tmp.d_vals, ny, nx, nz, fy, fx, fz, nf);
    HIPCHECK(c, hipGetLastError());
    // (into a page-locked word: a pageable destination would stall the host here until the cube is built - and the upload of the
    // points, which is to run UNDER that build, with it)
    c->h_word[0] = 0;
    HIPCHECK(c, hipMemcpyAsync(&c->h_word[0], nf, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (n > 0) {
        rc = interp_pipeline(c, who, &tmp, false, y, x, z, n, make_query(proj_mode, inc0), proj, wet, hydro, k_point_slots); if (rc) return rc;
    } else HIPCHECK(c, hipStreamSynchronize(c->stream));
    quiesce.armed = false;                      // (both branches have synchronised)
    if (cube_has_nan) *cube_has_nan = c->h_word[0] != 0;
    scratch_trim_point_delays(c);
    return RDR_OK;
}

int rdr_point_delays(rdr_ctx* c, const rdr_cube* q, const double* xpts, int64_t nx, const double* ypts, int64_t ny, const double* zpts, int64_t nz,
                     const double* y, const double* x, const double* z, int64_t n, int proj_mode, const double* proj, double inc0,
                     double* wet, double* hydro, int32_t* cube_has_nan) {
    if (!c || !q || !xpts || !ypts || !zpts) return fail(c, RDR_ERR_INVALID, "rdr_point_delays: NULL argument");
    return point_delays_impl(c, "rdr_point_delays", q, nullptr, xpts, nx, ypts, ny, zpts, nz, y, x, z, n, proj_mode, proj, inc0, wet, hydro, cube_has_nan);
}

int rdr_point_delays_grid(rdr_ctx* c, const rdr_cube* q, int grid_kind, const double* params, int nparams, const double* xpts, int64_t nx,
                          const double* ypts, int64_t ny, const double* zpts, int64_t nz, const double* y, const double* x, const double* z, int64_t n,
                          int proj_mode, const double* proj, double inc0, double* wet, double* hydro, int32_t* cube_has_nan) {
    static const char* who = "rdr_point_delays_grid";
    if (!c || !q || !xpts || !ypts || !zpts) return fail(c, RDR_ERR_INVALID, "rdr_point_delays_grid: NULL argument");
    GridCrs g;
    const int rc = grid_crs(c, who, grid_kind, params, nparams, g); if (rc) return rc;
    return point_delays_impl(c, who, q, &g, xpts, nx, ypts, ny, zpts, nz, y, x, z, n, proj_mode, proj, inc0, wet, hydro, cube_has_nan);
}

static int project_impl(rdr_ctx* c, const char* who, double* wet, double* hydro, int pmode, const double* proj, int64_t n, int loc) {
    if (!c || (!wet && !hydro) || !proj) return fail(c, RDR_ERR_INVALID, std::string(who) + ": NULL argument");
    if (n < 0) return fail(c, RDR_ERR_INVALID, std::string(who) + ": negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double* di = S.in(proj, (size_t)n * 8);
    double *dwi = S.inout(wet, (size_t)n * 8, SLOT_OUT0), *dhi = S.inout(hydro, (size_t)n * 8, SLOT_OUT1);   // divided in place
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(project_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, dwi, dhi, pmode, di, 0.0, n);
    return S.finish();
}

int rdr_project_cosinc(rdr_ctx* c, double* wet, double* hydro, const double* inc, int64_t n, int loc) {
    return project_impl(c, "rdr_project_cosinc", wet, hydro, 1, inc, n, loc);
}

int rdr_project_divide(rdr_ctx* c, double* wet, double* hydro, const double* divisor, int64_t n, int loc) {
    return project_impl(c, "rdr_project_divide", wet, hydro, 3, divisor, n, loc);
}

// ---- rays -------------------------------------------------------------------------------------------
static int levels_host(const std::vector<double>& zs, double ht, double zref, std::vector<double>& lo, std::vector<double>& hi,
                       std::vector<int>& kz) {
    const int nz = (int)zs.size();
    const double ztop = zs[nz - 1];
    for (int zz = 0; zz < nz - 1; ++zz) {
        double l = zs[zz], h = zs[zz + 1];
        if (h == ztop) h -= 0.01;
        if (h < ht || l >= zref) continue;
        if (l < ht) l = ht;
        if (h > zref) h = zref;
        if (std::fabs(h - l) < 1.0) continue;
        lo.push_back(l); hi.push_back(h); kz.push_back(zz);
    }
    return (int)lo.size();
}

static int fail_no_levels(rdr_ctx* c) {
    return fail(c, RDR_ERR_NO_LEVELS, "no weather-model interval contributes to the ray integral (build_ray -> None)");
}

int rdr_ray_levels(const rdr_cube* q, double ht, double zref, int32_t* K, double* lo, double* hi, int32_t* kz) {
    if (!q || !K) return fail(nullptr, RDR_ERR_INVALID, "rdr_ray_levels: NULL argument");
    std::vector<double> l, h; std::vector<int> z;
    *K = levels_host(q->zs, ht, zref, l, h, z);
    if (lo) std::copy(l.begin(), l.end(), lo);
    if (hi) std::copy(h.begin(), h.end(), hi);
    if (kz) std::copy(z.begin(), z.end(), kz);
    if (*K == 0) return fail_no_levels(q->ctx);
    return RDR_OK;
}

int rdr_nparts(const double* maxlen, int32_t K, double max_seg, int32_t* nparts) {
    if (!maxlen || !nparts) return fail(nullptr, RDR_ERR_INVALID, "rdr_nparts: NULL argument");
    if (K < 0 || !(max_seg > 0.0)) return fail(nullptr, RDR_ERR_INVALID, "rdr_nparts: K >= 0 and MAX_SEGMENT_LENGTH > 0");
    for (int k = 0; k < K; ++k) {
        const double parts = std::ceil(maxlen[k] / max_seg) + 1;   // delay.py:283
        nparts[k] = (parts >= 1 && parts <= 2147483647.0) ? (int32_t)parts : 2147483647;
    }
    return RDR_OK;
}

static int check_rays(rdr_ctx* c, const rdr_rays* r) {
    if (!r) return fail(c, RDR_ERR_INVALID, "rays is NULL");
    if (r->n < 0) return fail(c, RDR_ERR_INVALID, "rays->n negative");
    if (r->origin_mode == RDR_ORIGIN_GRID) {
        if (!r->xpts || !r->ypts || r->nx * r->ny != r->n) return fail(c, RDR_ERR_INVALID, "GRID rays need xpts, ypts and n == nx*ny");
    } else if (r->origin_mode == RDR_ORIGIN_LLH) {
        if (!r->lat || !r->lon) return fail(c, RDR_ERR_INVALID, "LLH rays need lat and lon");
    } else if (r->origin_mode == RDR_ORIGIN_XYZ) {
        if (!r->xyz) return fail(c, RDR_ERR_INVALID, "XYZ rays need xyz");
        if (r->los_mode != RDR_LOS_VEC && (!r->lat || !r->lon)) return fail(c, RDR_ERR_INVALID, "XYZ rays with inc/heading or zenith LOS need lat and lon too");
    } else return fail(c, RDR_ERR_INVALID, "unknown origin_mode");
    if (r->los_mode == RDR_LOS_VEC) { if (!r->los) return fail(c, RDR_ERR_INVALID, "LOS_VEC needs los"); }
    else if (r->los_mode == RDR_LOS_INC_HD) { if (!r->inc) return fail(c, RDR_ERR_INVALID, "LOS_INC_HD needs inc (and hd, or hd0 for one heading)"); }
    else if (r->los_mode != RDR_LOS_INC_HD_SCALAR && r->los_mode != RDR_LOS_ZENITH) return fail(c, RDR_ERR_INVALID, "unknown los_mode");
    return RDR_OK;
}

// stage every ray array the mode needs; fills P (one slice; los_mult > 1: the look-vector / incidence / heading arrays hold
// los_mult consecutive blocks of n rays, one per height slice)
static int stage_rays(rdr_ctx* c, const rdr_rays* r, RayParams& P, int64_t los_mult = 1) {
    std::memset(&P, 0, sizeof(P));
    P.n = r->n; P.origin_mode = r->origin_mode; P.los_mode = r->los_mode; P.nx = r->nx; P.ny = r->ny;
    P.inc0 = r->inc0; P.hd0 = r->hd0;
    const int loc = r->loc;
    const void* d;
    int rc;
    if (r->origin_mode == RDR_ORIGIN_GRID) {
        rc = stage_in(c, SLOT_IN0, r->xpts, (size_t)r->nx * 8, loc, &d); if (rc) return rc; P.xpts = (const double*)d;
        rc = stage_in(c, SLOT_IN1, r->ypts, (size_t)r->ny * 8, loc, &d); if (rc) return rc; P.ypts = (const double*)d;
    } else {
        rc = stage_in(c, SLOT_IN0, r->lat, (size_t)r->n * 8, loc, &d); if (rc) return rc; P.lat = (const double*)d;
        rc = stage_in(c, SLOT_IN1, r->lon, (size_t)r->n * 8, loc, &d); if (rc) return rc; P.lon = (const double*)d;
        if (r->origin_mode == RDR_ORIGIN_XYZ) { rc = stage_in(c, SLOT_IN2, r->xyz, (size_t)r->n * 24, loc, &d); if (rc) return rc; P.xyz = (const double*)d; }
    }
    const size_t nl = (size_t)r->n * (size_t)los_mult;
    if (r->los_mode == RDR_LOS_VEC) { rc = stage_in(c, SLOT_IN3, r->los, nl * 24, loc, &d); if (rc) return rc; P.los = (const double*)d; }
    else if (r->los_mode == RDR_LOS_INC_HD) {
        rc = stage_in(c, SLOT_IN4, r->inc, nl * 8, loc, &d); if (rc) return rc; P.inc = (const double*)d;
        if (r->hd) { rc = stage_in(c, SLOT_IN5, r->hd, nl * 8, loc, &d); if (rc) return rc; P.hd = (const double*)d; }   // NULL: hd0 for every ray
    }
    if (r->hts) {                                           // per-ray origin heights (one batch = one slice)
        if (los_mult != 1) return fail(c, RDR_ERR_INVALID, "per-ray heights (rays->hts) and height slices exclude each other");
        rc = stage_in(c, SLOT_IN6, r->hts, (size_t)r->n * 8, loc, &d); if (rc) return rc; P.ht_ray = (const double*)d;
    }
    if (r->origin_mode == RDR_ORIGIN_GRID) {
        P.tiles_x = (int)((r->nx + TILE - 1) / TILE);
        P.ntiles = (int64_t)P.tiles_x * ((r->ny + TILE - 1) / TILE);
    } else {
        P.tiles_x = 1;
        P.ntiles = (r->n + BLOCK - 1) / BLOCK;
    }
    P.nslices = 1; P.tiles_per_slice = std::max<int64_t>(P.ntiles, 1); P.hts = nullptr; P.los_stride = 0;
    P.maxlen_bits = c->d_maxlen; P.flags = c->d_flags;
    P.ws = nullptr; P.nslots = 0; P.tile_begin = 0; P.tile_count = P.ntiles; P.nslow = c->d_nslow;
    return RDR_OK;
}

static size_t ray_smem(const rdr_cube* q) {
    return ray_smem_bytes(q->ny, q->nx, q->nz, q->exact[0], q->exact[1]);
}
// dynamic + the static LDS of the ray kernels (march_kernel's staging block for f64 cubes: 4 waves x 48 x 16 B): what must fit the CU
static size_t ray_lds_total(const rdr_cube* q) { return ray_smem(q) + (q->dtype == RDR_F64 ? (size_t)(BLOCK / 64) * 48 * 16 : 16); }

// Persistent grid of `per_cu` workgroups per CU; tiles are handed out dynamically (TileWalk: one device atomic per tile and
// XCD band), so the grid only has to cover the resident workgroups (3-4 per CU) with a little slack.  Measured on the bench
// scene (tools/probe_passes.py, RAIDER_HIP_BLOCKS_PER_CU = 4 .. 24): 4-8 per CU are equal (march 6.52 ms), 24 costs 2 % in
// per-workgroup table set-up.  (With a static equal share per workgroup the same sweep needed 24 per CU to hide the
// imbalance and was still 2-7 % slower.)
static int ray_grid(rdr_ctx* c, int64_t ntiles, int per_cu) {
    static const int forced = []() { const char* e = std::getenv("RAIDER_HIP_BLOCKS_PER_CU"); return e ? std::atoi(e) : 0; }();
    if (forced > 0) per_cu = forced;
    int64_t g = std::min<int64_t>(ntiles, (int64_t)c->num_cus * per_cu);
    g = std::max<int64_t>(8, (g + 7) / 8 * 8);   // multiple of 8 (one share per XCD)
    return (int)g;
}

// Workspace = ray records (WS_NFIELDS doubles per ray slot, every ray) + the side buffer (K+1 crossings per GENERIC ray).
static size_t ws_tile_bytes() { return (size_t)WS_NFIELDS * BLOCK * sizeof(double); }

// Side-buffer columns for a launch of `slots` ray slots: rays the static classification rejects are rare (none at all on most
// scenes), so 1/32 of the batch is provisioned up front; when the host has seen a larger count on this context (dateline or polar
// scenes: every slice of a tropo_delay call repeats it) that count is used.  Rays beyond the capacity are still integrated
// correctly - pass 2 recomputes their crossings.
static int64_t side_columns(rdr_ctx* c, int64_t slots, int K, size_t budget_left) {
    if (c->side_forced >= 0) return std::min<int64_t>(c->side_forced, slots);
    int64_t want = std::max<int64_t>(65536, slots / 32);
    if (c->last_nslow > 0) want = std::max<int64_t>(want, c->last_nslow + c->last_nslow / 16 + 1024);
    want = std::min<int64_t>(want, slots);
    const size_t col = (size_t)(K + 1) * sizeof(double);
    want = std::min<int64_t>(want, (int64_t)(budget_left / col));
    return std::max<int64_t>(want, 0);
}

static size_t ws_budget(rdr_ctx* c) {
    size_t free_b = 0, total_b = 0;
    size_t budget = c->ws_limit;
    const size_t held = c->ws.cap + c->side.cap;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max(held, free_b / 2 + held));
    return budget;
}

// Largest number of tiles whose records (plus a 1/32 side buffer) fit the workspace limit / half of the free device memory.
static int64_t ws_chunk_tiles(rdr_ctx* c, int K) {
    const size_t per_tile = ws_tile_bytes() + (size_t)(K + 1) * sizeof(double) * BLOCK / 32;
    return (int64_t)std::max<size_t>(1, ws_budget(c) / per_tile);
}

// Reserve records for `tiles` tiles and point P at them (records, side buffer, side counter).
static int ws_reserve(rdr_ctx* c, int64_t tiles, int K, RayParams& P) {
    const size_t need = (size_t)tiles * ws_tile_bytes();
    int rc = grow(c, c->ws, need); if (rc) return rc;
    const size_t budget = ws_budget(c);
    const int64_t cols = side_columns(c, tiles * BLOCK, K, budget > need ? budget - need : 0);
    rc = grow(c, c->side, (size_t)cols * (K + 1) * sizeof(double)); if (rc) return rc;
    c->side_cap = cols;
    P.ws = (double*)c->ws.p;
    P.side = cols > 0 ? (double*)c->side.p : nullptr; P.side_cap = cols; P.side_ctr = c->d_sidectr;
    return RDR_OK;
}

// the records written by the last pass 1 (wsig_match): same layout, nothing re-reserved
static void ws_attach(rdr_ctx* c, RayParams& P) {
    P.ws = (double*)c->ws.p;
    P.side = c->side_cap > 0 ? (double*)c->side.p : nullptr; P.side_cap = c->side_cap; P.side_ctr = c->d_sidectr;
}

static void wsig_set(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, double ht, double zref, int K, bool valid) {
    c->wsig.cube = q; c->wsig.vals = q->d_vals; c->wsig.proj = q->proj; c->wsig.n = r->n; c->wsig.ht = ht; c->wsig.zref = zref; c->wsig.K = K; c->wsig.valid = valid;
    c->wsig.a = r->origin_mode == RDR_ORIGIN_GRID ? (const void*)r->xpts : (r->origin_mode == RDR_ORIGIN_XYZ ? (const void*)r->xyz : (const void*)r->lat);
    c->wsig.b = r->origin_mode == RDR_ORIGIN_GRID ? (const void*)r->ypts : (const void*)r->lon;
    c->wsig.c = r->los_mode == RDR_LOS_VEC ? (const void*)r->los : (const void*)r->inc;
    c->wsig.d = (const void*)r->hts;
}

static bool wsig_match(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, double ht, double zref, int K) {
    if (!c->wsig.valid || c->wsig.cube != q || c->wsig.vals != q->d_vals || std::memcmp(&c->wsig.proj, &q->proj, sizeof(LccParams)) != 0 || c->wsig.n != r->n || c->wsig.ht != ht || c->wsig.zref != zref || c->wsig.K != K) return false;
    if (r->loc != RDR_DEVICE) return false;   // host arrays may have been rewritten in place between the two calls
    const void* a = r->origin_mode == RDR_ORIGIN_GRID ? (const void*)r->xpts : (r->origin_mode == RDR_ORIGIN_XYZ ? (const void*)r->xyz : (const void*)r->lat);
    const void* b = r->origin_mode == RDR_ORIGIN_GRID ? (const void*)r->ypts : (const void*)r->lon;
    const void* cc = r->los_mode == RDR_LOS_VEC ? (const void*)r->los : (const void*)r->inc;
    return a == c->wsig.a && b == c->wsig.b && cc == c->wsig.c && (const void*)r->hts == c->wsig.d;
}

// pass 1 over tiles [tb, tb+tc): optional reduction (P.maxlen_bits != null) and/or record store (P.ws != null)
// nslots_total > 0: the launch is one chunk of a larger record buffer (field stride nslots_total, P.ws already offset to the
// chunk's first slot) and the slow-ray count accumulates over the chunks (reset_nslow only for the first one).
// RAIDER_HIP_PASS1_SKIP=0: every wave runs the per-level length loop of pass 1 (the A/B switch of the wave bound; read once per process)
static bool pass1_skip_on() {
    static const int on = []() { const char* e = std::getenv("RAIDER_HIP_PASS1_SKIP"); return e ? std::atoi(e) : 1; }();
    return on != 0;
}

// ---- one selector per kernel family: the instantiation a launcher launches IS the one rdr_ray_kernel_attributes reports -------------
// the light pass-1 kernel; om: the input form of the batch (crossings_kernel's OM: 1 GRID + look vectors, 2 GRID + incidence, 0 the rest)
template <typename T2>
static auto crossings_fn(bool lcc, int om, bool per_ray) -> void (*)(CubeView<T2>, RayParams, LccParams) {
#define RDR_X(LCC_, OM_) (per_ray ? crossings_kernel<T2, false, LCC_, OM_, true> : crossings_kernel<T2, false, LCC_, OM_, false>)
#define RDR_X_OM(LCC_) (om == 1 ? RDR_X(LCC_, 1) : om == 2 ? RDR_X(LCC_, 2) : RDR_X(LCC_, 0))
    return lcc ? RDR_X_OM(true) : RDR_X_OM(false);
#undef RDR_X_OM
#undef RDR_X
}

// the light pass-2 kernel of one cube (grid: march_grid; per-ray heights are built for REGULAR and run-time flags only)
template <typename T2>
static auto march_fn(int grid, bool per_ray) -> void (*)(CubeView<T2>, RayParams, LccParams) {
    if (per_ray) return grid == 1 ? march_kernel<T2, false, 1, true> : march_kernel<T2, false, 0, true>;
    return grid == 1 ? march_kernel<T2, false, 1> : grid == 2 ? march_kernel<T2, false, 2> : march_kernel<T2, false, 0>;
}

// the stacked light pass-2 kernel of E epochs (grid, per_ray as in march_fn)
template <typename T2, int E>
static auto march_epochs_fn(int grid, bool per_ray) -> void (*)(CubeView<T2>, EpochCubes<T2, E>, RayParams, int64_t) {
    if (per_ray) return grid == 1 ? march_epochs_kernel<T2, E, 1, true> : march_epochs_kernel<T2, E, 0, true>;
    return grid == 1 ? march_epochs_kernel<T2, E, 1, false> : grid == 2 ? march_epochs_kernel<T2, E, 2, false> : march_epochs_kernel<T2, E, 0, false>;
}

static int launch_crossings(rdr_ctx* c, const rdr_cube* q, RayParams P, int64_t tb, int64_t tc, int64_t nslots_total = 0, bool reset_nslow = true) {
    P.tile_begin = tb; P.tile_count = tc; P.nslots = nslots_total > 0 ? nslots_total : tc * BLOCK;
    // the lon/lat slice instantiations may skip the level loop per wave; their two tables lie behind the common LDS layout and are
    // allocated for that launch alone (a cube whose tables leave no room for them is traced without the skip, as before)
    const bool skippable = pass1_skip_on() && q->proj.kind != 1 && !P.ht_ray && P.maxlen_bits != nullptr &&
                           ray_lds_total(q) + skip_smem_bytes(q->nz) <= c->lds_max;
    P.skip_levels = skippable ? 1 : 0;
    const int g = ray_grid(c, tc, 8);
    if (ray_lds_total(q) > c->lds_max)
        return fail(c, RDR_ERR_INVALID, "ray tracing: the cube's non-uniform horizontal axes and level tables need " + std::to_string(ray_lds_total(q)) +
                    " B of LDS per workgroup, the device offers " + std::to_string(c->lds_max) + " (resample the cube to uniform axes or crop it)");
    if (reset_nslow) {
        HIPCHECK(c, hipMemsetAsync(c->d_nslow, 0, 2 * sizeof(int), c->stream));
        HIPCHECK(c, hipMemsetAsync(c->d_sidectr, 0, sizeof(int), c->stream));
    }
    HIPCHECK(c, hipMemsetAsync(c->d_tilectr, 0, 16 * sizeof(int), c->stream));
    P.tile_ctr = c->d_tilectr;
    const size_t sm = ray_smem(q);
    hipError_t e = hipSuccess;
    {
        KTimer t(c, 0);
        const size_t sm_light = sm + (skippable ? skip_smem_bytes(q->nz) : 0);
        const bool lcc = q->proj.kind == 1;
        // input form of the batch, fixed at compile time for the two hot ones (crossings_kernel's OM parameter)
        const int om = P.origin_mode != RDR_ORIGIN_GRID ? 0 : (P.los_mode == RDR_LOS_VEC ? 1 : 2);
        const dim3 G(g), B(BLOCK);
        e = by_dtype(q, [&](auto t) { return launch_lds(crossings_fn<decltype(t)>(lcc, om, P.ht_ray != nullptr), G, B, sm_light, c->stream, make_view<decltype(t)>(q), P, q->proj); });
    }
    if (e != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("crossings_kernel launch: ") + hipGetErrorString(e));
    // generic-geodesy mop-up of the rays the classification rejected (returns at once when there are none)
    P.tile_ctr = c->d_tilectr + 8;
    e = by_dtype(q, [&](auto t) { return launch_lds(crossings_kernel<decltype(t), true>, dim3(g), dim3(BLOCK), sm, c->stream, make_view<decltype(t)>(q), P, q->proj); });
    if (e != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("crossings_kernel launch: ") + hipGetErrorString(e));
    return RDR_OK;
}

// The light pass-2 instantiation a cube takes (GRID of march_kernel / march_epochs_kernel): 1 REGULAR, 2 TABLES, 0 run-time flags.
// Per-ray heights are built for REGULAR and run-time flags only.
static int march_grid(const rdr_cube* q, bool per_ray) {
    const bool small = make_view<float2>(q).small && (q->dtype == RDR_F32 || make_view<double2>(q).small);
    if (!small) return 0;
    if (q->exact[0] && q->exact[1]) return 1;
    return (!per_ray && !q->exact[0] && !q->exact[1] && q->uni[0] && q->uni[1]) ? 2 : 0;
}

// The level table of a pass 2 over slices [s0, s0 + ns) of P's batch (level_table_kernel: one workgroup per slice, all inputs on the
// device, no host synchronisation) and P.lev -> it.  ONCE per pass 2 - by whoever runs the pass-2 launches of a partition (ray_passes,
// raytrace_pipelined, the record-reusing marches), not per chunk of tiles - after the slices' partition is complete on the stream and
// inside the timing scope of pass 2.  Per-ray heights: nothing reads a table (P.lev stays null).
static int launch_level_table(rdr_ctx* c, const rdr_cube* q, RayParams& P, int64_t s0, int64_t ns) {
    P.lev = nullptr;
    if (P.ht_ray || ns <= 0) return RDR_OK;
    { const int rc = grow(c, c->lev, (size_t)P.nslices * (size_t)(q->nz + 1) * sizeof(LevelRec)); if (rc) return rc; }
    P.lev = (const LevelRec*)c->lev.p;
    hipError_t e;
    {
        KTimer t(c, 1);
        e = launch_lds(level_table_kernel<float2>, dim3((unsigned)ns), dim3(BLOCK), ray_smem_bytes(0, 0, q->nz, 1, 1), c->stream, make_view<float2>(q), P, (int)s0,
                       (LevelRec*)c->lev.p);
    }
    if (e != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("level_table_kernel launch: ") + hipGetErrorString(e));
    return RDR_OK;
}

// a light slice march without its level table is a driver's mistake, not something to trace around
static int check_level_table(rdr_ctx* c, const RayParams& P) {
    if (!P.ht_ray && !P.lev) return fail(c, RDR_ERR_INVALID, "pass 2 was launched without its level table (launch_level_table)");
    return RDR_OK;
}

// generic-ray mop-up of pass 2 on the records of P, tile counters d_tilectr + 24 (zero_ctr: not yet zeroed); the kernel returns at once
// when pass 1 found no generic ray
static int launch_march_generic(rdr_ctx* c, const rdr_cube* q, RayParams P, dim3 G, dim3 B, size_t sm, bool zero_ctr) {
    if (zero_ctr) HIPCHECK(c, hipMemsetAsync(c->d_tilectr + 24, 0, 8 * sizeof(int), c->stream));
    P.tile_ctr = c->d_tilectr + 24;
    const hipError_t e = by_dtype(q, [&](auto t) { return launch_lds(march_kernel<decltype(t), true>, G, B, sm, c->stream, make_view<decltype(t)>(q), P, q->proj); });
    if (e != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("march_kernel launch: ") + hipGetErrorString(e));
    return RDR_OK;
}

static int launch_march(rdr_ctx* c, const rdr_cube* q, RayParams P, int64_t tb, int64_t tc, int64_t nslots_total = 0) {
    P.tile_begin = tb; P.tile_count = tc; P.nslots = nslots_total > 0 ? nslots_total : tc * BLOCK;
    { const int rc = check_level_table(c, P); if (rc) return rc; }
    static const int stage_f64 = []() { const char* e = std::getenv("RAIDER_HIP_F64_STAGE"); return e ? std::atoi(e) : 1; }();
    P.stage_f64 = stage_f64;
    const int g = ray_grid(c, tc, 8);
    HIPCHECK(c, hipMemsetAsync(c->d_tilectr + 16, 0, 16 * sizeof(int), c->stream));     // (the mop-up's counters too)
    P.tile_ctr = c->d_tilectr + 16;
    const size_t sm = ray_smem(q);
    const dim3 G(g), B(BLOCK);
    hipError_t e = hipSuccess;
    {
        KTimer t(c, 1);
        const bool per_ray = P.ht_ray != nullptr;
        const int grid = march_grid(q, per_ray);
        e = by_dtype(q, [&](auto t) { return launch_lds(march_fn<decltype(t)>(grid, per_ray), G, B, sm, c->stream, make_view<decltype(t)>(q), P, q->proj); });
    }
    if (e != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("march_kernel launch: ") + hipGetErrorString(e));
    return launch_march_generic(c, q, P, G, B, sm, false);
}

// epochs per stacked launch: 4, or RAIDER_HIP_EPOCHS_MAX = 1 / 2 / 4 (tools/bench_epochs.py compares them; 1 = the one-epoch march per epoch)
static int epochs_max() {
    const char* e = std::getenv("RAIDER_HIP_EPOCHS_MAX");
    const int v = e ? std::atoi(e) : EPOCHS_MAX;
    return v >= 4 ? 4 : v >= 2 ? 2 : 1;
}

// Epochs of the next stacked launch of a series with `left` epochs to go: 4, then 2, then 1 (engine.epoch_groups; 1: the one-epoch
// kernel), capped by emax = epochs_max().  A per-ray-height series on f64 cubes goes in pairs - its E = 4 instantiation is spill-free
// at one wave per SIMD only (EpochWaves; DESIGN.md 5d has the measurements) - unless RAIDER_HIP_EPOCHS_PR_F64_MAX = 1 / 2 / 4 says
// otherwise (tools/bench_epochs.py compares them).
static int epoch_group(int dtype, bool per_ray, int left, int emax) {
    if (per_ray && dtype == RDR_F64) {
        const char* env = std::getenv("RAIDER_HIP_EPOCHS_PR_F64_MAX");
        emax = std::min(emax, env ? std::atoi(env) : 2);
    }
    return (left >= 4 && emax >= 4) ? 4 : (left >= 2 && emax >= 2) ? 2 : 1;
}

// the stacked light kernel of E epochs on the cubes qs[0..E) (grid: march_grid of the batch; per-ray heights from P.ht_ray)
template <typename T2, int E>
static hipError_t launch_stacked(rdr_ctx* c, const rdr_cube* const* qs, int grid, const RayParams& P, int64_t estride, dim3 G, dim3 B, size_t sm) {
    EpochCubes<T2, E> ev;
    for (int j = 0; j < E; ++j) ev.v[j] = (const T2*)qs[j]->d_vals;
    return launch_lds(march_epochs_fn<T2, E>(grid, P.ht_ray != nullptr), G, B, sm, c->stream, make_view<T2>(qs[0]), ev, P, estride);
}

// pass 2 of D epochs over tiles [tb, tb+tc) on the records of ONE pass 1: groups of 4 / 2 epochs (epoch_group) take the stacked
// marcher - its per-ray-height loop when the batch has per-ray heights (P.ht_ray; one slice) - plus the generic kernel once per epoch;
// a last single epoch takes launch_march, whose instantiations the stacked ones match bit for bit.
// P.wet / P.hyd: epoch 0's [nslices][n] block, epoch e's is estride doubles further.
static int launch_march_epochs(rdr_ctx* c, const rdr_cube* const* qs, int D, RayParams P, int64_t tb, int64_t tc, int64_t estride) {
    const rdr_cube* q = qs[0];
    { const int rc = check_level_table(c, P); if (rc) return rc; }
    const int emax = epochs_max();
    const bool per_ray = P.ht_ray != nullptr;
    const int grid = march_grid(q, per_ray);
    const int g = ray_grid(c, tc, 8);
    const size_t sm = ray_smem(q);
    const dim3 G(g), B(BLOCK);
    for (int e = 0; e < D;) {
        const int ge = epoch_group(q->dtype, per_ray, D - e, emax);
        RayParams Pe = P;
        Pe.wet = P.wet + (int64_t)e * estride; Pe.hyd = P.hyd + (int64_t)e * estride;
        if (ge == 1) {
            const int rc = launch_march(c, qs[e], Pe, tb, tc); if (rc) return rc;
            ++e;
            continue;
        }
        Pe.tile_begin = tb; Pe.tile_count = tc; Pe.nslots = tc * BLOCK;
        HIPCHECK(c, hipMemsetAsync(c->d_tilectr + 16, 0, 8 * sizeof(int), c->stream));
        Pe.tile_ctr = c->d_tilectr + 16;
        hipError_t err = hipSuccess;
        {
            KTimer t(c, 1);
            err = by_dtype(q, [&](auto t) {
                return ge == 4 ? launch_stacked<decltype(t), 4>(c, qs + e, grid, Pe, estride, G, B, sm) : launch_stacked<decltype(t), 2>(c, qs + e, grid, Pe, estride, G, B, sm);
            });
        }
        if (err != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("march_epochs_kernel launch: ") + hipGetErrorString(err));
        for (int j = 0; j < ge; ++j) {                  // generic rays, epoch by epoch, on the same records and side buffer
            RayParams Pj = Pe;
            Pj.wet = Pe.wet + (int64_t)j * estride; Pj.hyd = Pe.hyd + (int64_t)j * estride;
            const int rc = launch_march_generic(c, qs[e + j], Pj, G, B, sm, true); if (rc) return rc;
        }
        e += ge;
    }
    return RDR_OK;
}

// Registers / LDS / scratch of the light ray kernel a GRID + look-vector batch on this cube launches, read from the LOADED code
// object (hipFuncGetAttributes) - what bench.py prints, instead of a profiler's metadata column.
int rdr_ray_kernel_attributes(rdr_ctx* c, const rdr_cube* q, int which, int32_t* vgprs, int32_t* static_lds, int32_t* dynamic_lds,
                              int32_t* scratch, int32_t* max_threads) {
    if (!c || !q || which < 0 || which > 7) return fail(c, RDR_ERR_INVALID, "rdr_ray_kernel_attributes: bad argument");
    const bool lcc = q->proj.kind == 1;
    const bool pr = which == 2 || which == 3 || which >= 6;      // 2 / 3: the per-ray-height instantiations of pass 1 / pass 2; 6 / 7: of the stacked march
    const int grid = march_grid(q, pr);
    const void* const fn = by_dtype(q, [&](auto tag) -> const void* {
        typedef decltype(tag) T2;
        // 4 / 5 (sliced), 6 / 7 (per-ray heights): the stacked march (march_epochs_kernel), E = 2 / 4
        if (which >= 4) return (which & 1) != 0 ? (const void*)march_epochs_fn<T2, 4>(grid, pr) : (const void*)march_epochs_fn<T2, 2>(grid, pr);
        if ((which & 1) == 0) return (const void*)crossings_fn<T2>(lcc, 1, pr);
        return (const void*)march_fn<T2>(grid, pr);
    });
    hipFuncAttributes a;
    HIPCHECK(c, hipFuncGetAttributes(&a, fn));
    if (vgprs) *vgprs = a.numRegs;
    if (static_lds) *static_lds = (int32_t)a.sharedSizeBytes;
    if (dynamic_lds) *dynamic_lds = (int32_t)ray_smem(q);
    if (scratch) *scratch = (int32_t)a.localSizeBytes;
    if (max_threads) *max_threads = a.maxThreadsPerBlock;
    return RDR_OK;
}

// ---- the one-kernel route (trace_kernel, raider_kernels.h) -----------------------------------------------------------------------------
// RAIDER_HIP_ONE_PASS=0: every call takes the two passes (the A/B switch of the route; read once per process, like RAIDER_HIP_PASS1_SKIP)
static bool one_pass_on() {
    static const int on = []() { const char* e = std::getenv("RAIDER_HIP_ONE_PASS"); return e ? std::atoi(e) : 1; }();
    return on != 0;
}

// LDS of a trace_kernel launch: the common layout, pass 1's two skip tables and the park behind them
static size_t trace_smem(const rdr_cube* q) { return ray_smem(q) + skip_smem_bytes(q->nz) + trace_park_bytes(); }

// May this pass 1 + pass 2 over ONE slice of `per` tiles go through trace_kernel?  One f32 lon/lat cube on exactly uniform axes (march_kernel's
// REGULAR), GRID origins with per-pixel look vectors (the one input form trace_kernel is built for: the sincos of an incidence / heading batch
// puts it into scratch), no per-ray heights, a partition to be reduced, device arrays, 2 < K <= 128 (the limits of the wave bound), records
// that fit one group - they are still reserved, for the classic passes behind - and the kernel's LDS.
static bool one_pass_eligible(rdr_ctx* c, const rdr_cube* q, const RayParams& P, int K, int64_t per, int64_t nslices, int64_t fit, bool device_rays) {
    return one_pass_on() && device_rays && q->dtype == RDR_F32 && q->proj.kind == 0 && march_grid(q, false) == 1 &&
           P.origin_mode == RDR_ORIGIN_GRID && P.los_mode == RDR_LOS_VEC && !P.ht_ray && !P.hts && nslices == 1 && P.nslices == 1 &&
           P.maxlen_bits != nullptr && !P.nparts_override && K > 2 && K <= 128 && per <= fit && per < ((int64_t)1 << 31) &&
           ray_lds_total(q) + skip_smem_bytes(q->nz) + trace_park_bytes() <= c->lds_max;
}

// The probe's tiles of a scene of tiles_x x tiles_y tiles: its four border rows and columns - the edges of a swath hold its longest rays -
// and every eighth tile of every eighth row inside: 2 / tiles_x + 2 / tiles_y + 1 / 64 of the scene, 3 % of the headline one.
static std::vector<int> probe_tiles(int tiles_x, int64_t tiles_y) {
    std::vector<int> v;
    for (int64_t ty = 0; ty < tiles_y; ++ty) {
        const bool edge_row = ty == 0 || ty == tiles_y - 1;
        for (int tx = 0; tx < tiles_x; ++tx)
            if (edge_row || tx == 0 || tx == tiles_x - 1 || (ty % 8 == 4 && tx % 8 == 4)) v.push_back((int)(ty * tiles_x + tx));
    }
    return v;
}

// One slice of `per` tiles (P: records reserved, outputs set) through the route.  Everything is enqueued, nothing is waited for:
//   grid_trig_kernel, the probe (crossings_kernel, reduce only, over probe_tiles)                      profiling scope 0
//   level_table_kernel, partition_check_kernel<false>, trace_kernel, partition_check_kernel<true>       profiling scope 1
//   the classic launch_crossings + launch_level_table + launch_march with RayParams::one_pass set: they return at their top unless
//   the check - or trace_kernel itself - raised OP_NEED, and overwrite every output when they run.
static int trace_one_pass(rdr_ctx* c, const rdr_cube* q, const RayParams& P, int K, int64_t per) {
    int rc = grow(c, c->gridtrig, (size_t)(P.ny + P.nx) * 2 * sizeof(double)); if (rc) return rc;
    if (c->probe_key.tiles_x != P.tiles_x || c->probe_key.tiles_y != per / P.tiles_x || c->probe_key.stream != c->stream) {
        const std::vector<int> list = probe_tiles(P.tiles_x, per / P.tiles_x);
        rc = grow(c, c->probe, list.size() * sizeof(int)); if (rc) return rc;
        rc = upload(c, c->probe.p, list.data(), list.size() * sizeof(int)); if (rc) return rc;
        c->probe_key.tiles_x = P.tiles_x; c->probe_key.tiles_y = per / P.tiles_x; c->probe_key.stream = c->stream; c->probe_key.count = (int64_t)list.size();
    }
    RayParams Pp = P;                                      // the probe: pass 1 as the chunked schedule launches it, over the list
    Pp.ws = nullptr; Pp.one_pass = nullptr; Pp.tile_list = (const int*)c->probe.p;
    {
        KTimer t(c, 0);
        hipLaunchKernelGGL(grid_trig_kernel, dim3((unsigned)std::min<int64_t>(64, (P.ny + P.nx + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, P, (double*)c->gridtrig.p);
    }
    HIPCHECK(c, hipGetLastError());
    rc = launch_crossings(c, q, Pp, 0, c->probe_key.count); if (rc) return rc;
    RayParams Pt = P;                                      // trace_kernel on the probed partition
    Pt.ws = nullptr; Pt.tile_list = nullptr; Pt.one_pass = nullptr; Pt.grid_trig = (const double*)c->gridtrig.p;
    rc = launch_level_table(c, q, Pt, 0, 1); if (rc) return rc;
    Pt.one_pass = c->d_onepass;
    Pt.tile_begin = 0; Pt.tile_count = per; Pt.nslots = 0; Pt.skip_levels = pass1_skip_on() ? 1 : 0;
    HIPCHECK(c, hipMemsetAsync(c->d_tilectr + 16, 0, 8 * sizeof(int), c->stream));
    Pt.tile_ctr = c->d_tilectr + 16;
    hipError_t e;
    {
        KTimer t(c, 1);
        hipLaunchKernelGGL(partition_check_kernel<false>, dim3(1), dim3(BLOCK), 0, c->stream, Pt, K);
        e = launch_lds(trace_kernel<float2, 1, 1>, dim3(ray_grid(c, per, 8)), dim3(BLOCK), trace_smem(q), c->stream, make_view<float2>(q), Pt, q->proj);
        hipLaunchKernelGGL(partition_check_kernel<true>, dim3(1), dim3(BLOCK), 0, c->stream, Pt, K);
    }
    if (e != hipSuccess) return fail(c, RDR_ERR_HIP, std::string("trace_kernel launch: ") + hipGetErrorString(e));
    HIPCHECK(c, hipGetLastError());
    ++c->one_pass_calls;
    RayParams Pc = P;                                      // the two classic passes, conditional on OP_NEED
    Pc.one_pass = c->d_onepass;
    rc = launch_crossings(c, q, Pc, 0, per); if (rc) return rc;
    rc = launch_level_table(c, q, Pc, 0, 1); if (rc) return rc;
    return launch_march(c, q, Pc, 0, per);
}

// The workspace schedule of pass 1 + pass 2 over `nslices` slices of `per` tiles each (tiles numbered slice-major), `fit` tiles of
// ray records at a time (ws_chunk_tiles).  Whole slices fit: groups of up to `max_group` slices, each one pass 1 that stores the
// records and one pass 2 on them, then after_group(first slice, slices).  Otherwise, per slice: pass 1 reduction only, then chunked
// (pass-1 store, pass-2) pairs.  reduce == false: the partition is already on the device (rdr_ray_march[_device]) - pass 1 only
// stores.  `march` is pass 2 (NULL: launch_march on q).
static int ray_passes(rdr_ctx* c, const rdr_cube* q, const RayParams& P, int K, int64_t per, int64_t nslices, int64_t fit, int64_t max_group,
                      bool reduce, const std::function<int(const RayParams&, int64_t, int64_t)>& march = nullptr,
                      const std::function<int(int64_t, int64_t)>& after_group = nullptr, bool device_rays = false) {
    const auto pass2 = [&](const RayParams& Pm, int64_t tb, int64_t tc) { return march ? march(Pm, tb, tc) : launch_march(c, q, Pm, tb, tc); };
    // one slice of one cube whose rays may be fitted and marched in one kernel (one_pass_eligible): trace_one_pass; device_rays: the batch's
    // arrays are device arrays
    if (reduce && !march && !after_group && one_pass_eligible(c, q, P, K, per, nslices, fit, device_rays)) {
        RayParams Pg = P;
        const int rc = ws_reserve(c, per, K, Pg); if (rc) return rc;      // (as the two passes reserve them: the classic launches behind write them)
        return trace_one_pass(c, q, Pg, K, per);
    }
    if (per <= fit) {
        const int64_t g = std::min<int64_t>(max_group, std::max<int64_t>(1, fit / per));
        for (int64_t s0 = 0; s0 < nslices; s0 += g) {
            const int64_t ns = std::min<int64_t>(g, nslices - s0);
            RayParams Pg = P;
            if (!reduce) Pg.maxlen_bits = nullptr;
            int rc = ws_reserve(c, ns * per, K, Pg); if (rc) return rc;
            rc = launch_crossings(c, q, Pg, s0 * per, ns * per); if (rc) return rc;
            Pg.maxlen_bits = P.maxlen_bits;
            rc = launch_level_table(c, q, Pg, s0, ns); if (rc) return rc;
            rc = pass2(Pg, s0 * per, ns * per); if (rc) return rc;
            if (after_group) { rc = after_group(s0, ns); if (rc) return rc; }
        }
        return RDR_OK;
    }
    for (int64_t s = 0; s < nslices; ++s) {
        int rc;
        if (reduce) {
            RayParams Ps = P;
            Ps.ws = nullptr;
            rc = launch_crossings(c, q, Ps, s * per, per); if (rc) return rc;
        }
        RayParams Pw = P;
        rc = ws_reserve(c, fit, K, Pw); if (rc) return rc;
        rc = launch_level_table(c, q, Pw, s, 1); if (rc) return rc;      // (the slice's partition is complete: once for all its chunks)
        for (int64_t tb = 0; tb < per; tb += fit) {
            const int64_t tc = std::min<int64_t>(fit, per - tb);
            RayParams Pc = Pw;
            Pc.maxlen_bits = nullptr;                      // store only, no reduction
            rc = launch_crossings(c, q, Pc, s * per + tb, tc); if (rc) return rc;
            Pc.maxlen_bits = P.maxlen_bits;
            rc = pass2(Pc, s * per + tb, tc); if (rc) return rc;
        }
    }
    return RDR_OK;
}

// What the five one-batch ray entries do before their own work.  check(): every cube noted as used, max_seg, check_rays, device arrays
// where the entry insists on them (`device_only`: its message), the levels K of (ht, zref) on cube 0 - none is RDR_ERR_NO_LEVELS.
// stage(): hipSetDevice, stage_rays of the batch it is GIVEN (raytrace_impl holds arrays back for its chunked upload), P.ht / zref /
// max_seg.  Between the two an entry puts its empty-batch return and samples wsig_match - before stage(), always.
struct RayCall {
    int K = 0;
    RayParams P;
    double ht = 0, zref = 0, max_seg = 0;
    int check(rdr_ctx* c, const char* who, const rdr_cube* const* qs, int D, const rdr_rays* r, double ht_, double zref_, double max_seg_,
              const char* device_only = nullptr) {
        for (int e = 0; e < D; ++e) note_use(c, qs[e]);
        if (!(max_seg_ > 0)) return fail(c, RDR_ERR_INVALID, std::string(who) + ": MAX_SEGMENT_LENGTH must be positive");
        const int rc = check_rays(c, r); if (rc) return rc;
        if (device_only && r->loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, std::string(who) + device_only);
        std::vector<double> lo, hi; std::vector<int> kz;
        K = levels_host(qs[0]->zs, ht_, zref_, lo, hi, kz);
        if (K == 0) return fail_no_levels(c);
        ht = ht_; zref = zref_; max_seg = max_seg_;
        return RDR_OK;
    }
    int stage(rdr_ctx* c, const rdr_rays* r) {
        HIPCHECK(c, hipSetDevice(c->device));
        const int rc = stage_rays(c, r, P); if (rc) return rc;
        P.ht = ht; P.zref = zref; P.max_seg = max_seg;
        return RDR_OK;
    }
};

// A fresh partition for `nslices` slices: their length maxima and flags zeroed on the stream, in that order; the stored ray records
// belong to the old one.
static int partition_reset(rdr_ctx* c, int64_t nslices) {
    HIPCHECK(c, hipMemsetAsync(c->d_maxlen, 0, (size_t)nslices * MAX_LEVELS * sizeof(unsigned long long), c->stream));
    HIPCHECK(c, hipMemsetAsync(c->d_flags, 0, (size_t)nslices * sizeof(int), c->stream));
    c->wsig.valid = false;
    return RDR_OK;
}

// Pass 1 of a whole batch for the two prepass entries (nothing for an empty one).  Device arrays whose records all fit: they are kept
// for the march that normally follows - ws_reserve before the launch, wsig_set after it.
static int prepass_records(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, RayCall& R) {
    if (r->n <= 0) return RDR_OK;
    const bool keep = r->loc == RDR_DEVICE && R.P.ntiles <= ws_chunk_tiles(c, R.K);
    int rc;
    if (keep) { rc = ws_reserve(c, R.P.ntiles, R.K, R.P); if (rc) return rc; }
    rc = launch_crossings(c, q, R.P, 0, R.P.ntiles); if (rc) return rc;
    if (keep) wsig_set(c, q, r, R.ht, R.zref, R.K, true);
    return RDR_OK;
}

// Pass 2 of the two march entries on a partition that is already on the device.  reuse (wsig_match, sampled before the rays were staged):
// the stored records of the same batch - attach, level table, march; else ray_passes re-runs a store-only pass 1.  Either way the records
// are spent afterwards.
static int march_on_records(rdr_ctx* c, const rdr_cube* q, RayCall& R, bool reuse) {
    int rc;
    if (reuse) { ws_attach(c, R.P); rc = launch_level_table(c, q, R.P, 0, 1); if (!rc) rc = launch_march(c, q, R.P, 0, R.P.ntiles); }
    else rc = ray_passes(c, q, R.P, R.K, R.P.ntiles, 1, ws_chunk_tiles(c, R.K), 1, false);
    c->wsig.valid = false;
    return rc;
}

// The partition back on the host: `nmax` length maxima, `nflags` slice flags, `more` (a slice series' epoch flags; may be absent), the
// slow-ray counter - and the skipped-wave counter behind it for `nskip` - copied in that order, ONE wait, last_nslow (last_nskip) set.
static int partition_read(rdr_ctx* c, double* maxlen, size_t nmax, int* flags, size_t nflags, bool nskip, void* more = nullptr, const void* d_more = nullptr,
                          size_t more_bytes = 0) {
    int ctr[2] = {0, 0}, redo = 0;
    HIPCHECK(c, hipMemcpyAsync(maxlen, c->d_maxlen, nmax * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpyAsync(flags, c->d_flags, nflags * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (more_bytes) HIPCHECK(c, hipMemcpyAsync(more, d_more, more_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpyAsync(ctr, c->d_nslow, (nskip ? 2 : 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (c->one_pass_calls > 0) HIPCHECK(c, hipMemcpyAsync(&redo, c->d_onepass + OP_REDO, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if (c->one_pass_calls > 0) c->one_pass_redos = redo;
    c->last_nslow = ctr[0];
    if (nskip) c->last_nskip = ctr[1];
    return RDR_OK;
}

// Host-buffer ray tracing with the PCIe transfers overlapped: the look vectors (24 B per ray, the bulk of the input) go up in
// row chunks on the copy stream while pass 1 runs on the chunks that have arrived; after the last chunk the slice-level
// partition is complete, pass 2 runs chunk by chunk and each chunk's outputs come down while the next is integrated.
// (hipMemcpyAsync from pageable memory blocks the HOST thread, not the device: kernels launched before it keep running.)
// An error return waits for all three streams (StreamsQuiesce): nothing is left copying into or out of the caller's arrays.
static int raytrace_pipelined(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, RayParams P, int K, double* d_los, double* d_hts, double* dw, double* dh,
                              double* wet, double* hydro) {
    const int64_t tile_rows = P.ntiles / P.tiles_x;
    const int nchunk = (int)std::min<int64_t>(8, tile_rows);
    int rc = ws_reserve(c, P.ntiles, K, P); if (rc) return rc;
    double* const ws = P.ws;
    const int64_t nslots_total = P.ntiles * BLOCK;
    if (d_los) P.los = d_los;                  // (else the look vectors come from inc / heading or zenith: nothing to upload)
    if (d_hts) P.ht_ray = d_hts;               // per-pixel heights travel with the look vectors, chunk by chunk
    EventList ev;                              // [0, nchunk): a chunk's upload; [nchunk, 2 nchunk): its pass 2
    if (!ev.add((size_t)2 * nchunk)) return fail(c, RDR_ERR_HIP, "pipelined ray tracing: event creation failed");
    StreamsQuiesce quiesce(c);
    const auto ok = [](hipError_t e) { return e == hipSuccess; };
    auto range = [&](int k, int64_t& tb, int64_t& tc, int64_t& r0, int64_t& cnt) {
        const int64_t t0 = tile_rows * k / nchunk, t1 = tile_rows * (k + 1) / nchunk;
        tb = t0 * P.tiles_x; tc = (t1 - t0) * P.tiles_x;
        if (r->origin_mode == RDR_ORIGIN_GRID) { r0 = t0 * TILE * r->nx; cnt = std::min<int64_t>(t1 * TILE, r->ny) * r->nx - r0; }
        else { r0 = tb * BLOCK; cnt = std::min<int64_t>((tb + tc) * BLOCK, r->n) - r0; }
    };
    for (int k = 0; k < nchunk; ++k) {
        int64_t tb, tc, r0, cnt; range(k, tb, tc, r0, cnt);
        if ((d_los && !ok(hipMemcpyAsync(d_los + 3 * r0, r->los + 3 * r0, (size_t)cnt * 24, hipMemcpyHostToDevice, c->copy_stream))) ||
            (d_hts && !ok(hipMemcpyAsync(d_hts + r0, r->hts + r0, (size_t)cnt * 8, hipMemcpyHostToDevice, c->copy_stream))) ||
            ((d_los || d_hts) && (!ok(hipEventRecord(ev.v[k], c->copy_stream)) || !ok(hipStreamWaitEvent(c->stream, ev.v[k], 0)))))
            return fail(c, RDR_ERR_HIP, "pipelined ray tracing: look-vector / height upload failed");
        RayParams Pk = P; Pk.ws = ws + tb * BLOCK;
        rc = launch_crossings(c, q, Pk, tb, tc, nslots_total, k == 0); if (rc) return rc;
    }
    rc = launch_level_table(c, q, P, 0, 1); if (rc) return rc;      // (every chunk's pass 1 is enqueued: the partition is complete)
    for (int k = 0; k < nchunk; ++k) {
        int64_t tb, tc, r0, cnt; range(k, tb, tc, r0, cnt);
        RayParams Pk = P; Pk.ws = ws + tb * BLOCK;
        rc = launch_march(c, q, Pk, tb, tc, nslots_total); if (rc) return rc;
        if (!ok(hipEventRecord(ev.v[nchunk + k], c->stream))) return fail(c, RDR_ERR_HIP, "pipelined ray tracing: event");
    }
    for (int k = 0; k < nchunk; ++k) {
        int64_t tb, tc, r0, cnt; range(k, tb, tc, r0, cnt);
        if (!ok(hipStreamWaitEvent(c->copy_stream, ev.v[nchunk + k], 0)) ||
            !ok(hipMemcpyAsync(wet + r0, dw + r0, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->copy_stream)) ||
            !ok(hipMemcpyAsync(hydro + r0, dh + r0, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->copy_stream)))
            return fail(c, RDR_ERR_HIP, "pipelined ray tracing: output download failed");
    }
    if (!ok(hipStreamSynchronize(c->copy_stream)) || !ok(hipStreamSynchronize(c->stream))) return fail(c, RDR_ERR_HIP, "pipelined ray tracing: sync");
    quiesce.armed = false;
    return RDR_OK;
}

static int flags_to_status(rdr_ctx* c, int flags) {
    if (!(flags & RDR_FLAG_ANY_FINITE)) return fail(c, RDR_ERR_ALL_NAN, "geo2rdr did not converge. Check orbit coverage");
    if (flags & RDR_FLAG_ANY_NAN) return fail(c, RDR_ERR_NAN_LENGTH, "some ray lengths are NaN: the number of integration parts (delay.py:283) is undefined");
    if (flags & RDR_FLAG_BAD_HEIGHT) return fail(c, RDR_ERR_INVALID, "per-ray heights: a ray starts below the height the batch's level table was built for (pass ht <= min(rays->hts))");
    if (flags & RDR_FLAG_DIVERGED) return fail(c, RDR_ERR_INVALID, "ray lengths diverged: a model level asks for fewer than 2 or more than 65536 integration parts (are the look vectors unit vectors?)");
    return RDR_OK;
}

int rdr_ray_prepass(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, double ht, double zref, double* maxlen, int32_t* flags) {
    if (!c || !q || !maxlen) return fail(c, RDR_ERR_INVALID, "rdr_ray_prepass: NULL argument");
    RayCall R;                                   // (no empty-batch return: an empty batch still delivers its zeroed partition)
    int rc = R.check(c, "rdr_ray_prepass", &q, 1, r, ht, zref, 1000.0); if (rc) return rc;
    rc = R.stage(c, r); if (rc) return rc;
    rc = partition_reset(c, 1); if (rc) return rc;
    rc = prepass_records(c, q, r, R); if (rc) return rc;
    int f = 0;
    rc = partition_read(c, maxlen, (size_t)R.K, &f, 1, true); if (rc) return rc;
    if (flags) *flags = f;
    return RDR_OK;
}

int rdr_ray_prepass_device(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, double ht, double zref, double* partition) {
    if (!c || !q || !partition) return fail(c, RDR_ERR_INVALID, "rdr_ray_prepass_device: NULL argument");
    RayCall R;                                   // (no empty-batch return, as in rdr_ray_prepass)
    int rc = R.check(c, "rdr_ray_prepass_device", &q, 1, r, ht, zref, 1000.0, ": rays must be device arrays"); if (rc) return rc;
    rc = R.stage(c, r); if (rc) return rc;
    rc = partition_reset(c, 1); if (rc) return rc;
    rc = prepass_records(c, q, r, R); if (rc) return rc;
    hipLaunchKernelGGL(pack_partition_kernel, dim3(1), dim3(256), 0, c->stream, c->d_maxlen, c->d_flags, R.K, partition);
    HIPCHECK(c, hipGetLastError());
    return RDR_OK;
}

int rdr_ray_march_device(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, double ht, double zref, double max_seg, const double* partition,
                         double* wet, double* hydro) {
    if (!c || !q || !partition || !wet || !hydro) return fail(c, RDR_ERR_INVALID, "rdr_ray_march_device: NULL argument");
    RayCall R;
    int rc = R.check(c, "rdr_ray_march_device", &q, 1, r, ht, zref, max_seg, ": rays and outputs must be device arrays"); if (rc) return rc;
    if (r->n == 0) return RDR_OK;
    const bool reuse = wsig_match(c, q, r, ht, zref, R.K);
    rc = R.stage(c, r); if (rc) return rc;
    R.P.wet = wet; R.P.hyd = hydro;
    hipLaunchKernelGGL(unpack_partition_kernel, dim3(1), dim3(256), 0, c->stream, partition, R.K, c->d_maxlen, c->d_flags);
    HIPCHECK(c, hipGetLastError());
    return march_on_records(c, q, R, reuse);
}

// The level table pass 2 would read for slices at hts[] with the given partition, back on the host (tests, diagnostics): the same kernel
// on the same inputs - nParts rows (the rdr_ray_march form) or length maxima and max_seg (what pass 1 leaves on the device).
int rdr_level_table(rdr_ctx* c, const rdr_cube* q, const double* hts, int32_t nslices, double zref, const int32_t* nparts, const double* maxlen,
                    int32_t ld, double max_seg, void* records) {
    if (!c || !q || !hts || !records || (nparts == nullptr) == (maxlen == nullptr))
        return fail(c, RDR_ERR_INVALID, "rdr_level_table: NULL argument, or not exactly one of nparts / maxlen");
    if (nslices < 1 || nslices > MAX_SLICES) return fail(c, RDR_ERR_INVALID, "rdr_level_table: 1..512 slices per call");
    if (ld < (int32_t)q->nz - 1 || ld > MAX_LEVELS) return fail(c, RDR_ERR_INVALID, "rdr_level_table: rows of nz-1 .. 512 entries");
    if (maxlen && !(max_seg > 0)) return fail(c, RDR_ERR_INVALID, "rdr_level_table: MAX_SEGMENT_LENGTH must be positive");
    note_use(c, q);
    HIPCHECK(c, hipSetDevice(c->device));
    RayParams P;
    std::memset(&P, 0, sizeof(P));
    P.nslices = nslices; P.ht = hts[0]; P.zref = zref; P.max_seg = maxlen ? max_seg : 1000.0;
    // rows of MAX_LEVELS entries, as the kernels index them: nParts as they are, maxima as their bit patterns
    std::vector<unsigned long long> rows(maxlen ? (size_t)nslices * MAX_LEVELS : 0, 0ULL);
    std::vector<int> irows(nparts ? (size_t)nslices * MAX_LEVELS : 0, 0);
    for (int s = 0; s < nslices; ++s)
        for (int k = 0; k < ld; ++k) {
            if (nparts) irows[(size_t)s * MAX_LEVELS + k] = nparts[(size_t)s * ld + k];
            else std::memcpy(&rows[(size_t)s * MAX_LEVELS + k], &maxlen[(size_t)s * ld + k], 8);
        }
    const void *dht, *drows;
    int rc = stage_in(c, SLOT_AUX, hts, (size_t)nslices * 8, RDR_HOST, &dht); if (rc) return rc;
    rc = nparts ? stage_in(c, SLOT_IN4, irows.data(), irows.size() * sizeof(int), RDR_HOST, &drows)
                : stage_in(c, SLOT_IN4, rows.data(), rows.size() * 8, RDR_HOST, &drows);
    if (rc) return rc;
    P.hts = (const double*)dht;
    if (nparts) P.nparts_override = (const int*)drows; else P.maxlen_bits = (unsigned long long*)const_cast<void*>(drows);
    rc = launch_level_table(c, q, P, 0, nslices); if (rc) return rc;
    HIPCHECK(c, hipMemcpyAsync(records, P.lev, (size_t)nslices * (size_t)(q->nz + 1) * sizeof(LevelRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

int rdr_ray_march(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, double ht, double zref, const int32_t* nparts, int32_t flags,
                  double* wet, double* hydro) {
    if (!c || !q || !nparts || !wet || !hydro) return fail(c, RDR_ERR_INVALID, "rdr_ray_march: NULL argument");
    RayCall R;
    int rc = R.check(c, "rdr_ray_march", &q, 1, r, ht, zref, 1000.0); if (rc) return rc;
    const int K = R.K;
    for (int k = 0; k < K; ++k) if (nparts[k] < 2 || nparts[k] > MAX_NPARTS) return fail(c, RDR_ERR_INVALID, "rdr_ray_march: nparts out of range (2..65536)");
    if (r->n == 0) return RDR_OK;
    const bool reuse = wsig_match(c, q, r, ht, zref, K);
    rc = R.stage(c, r); if (rc) return rc;
    RayParams& P = R.P;
    HIPCHECK(c, hipMemcpyAsync(c->d_nparts, nparts, (size_t)K * sizeof(int), hipMemcpyHostToDevice, c->stream));
    int f = flags;
    HIPCHECK(c, hipMemcpyAsync(c->d_flags, &f, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));   // nparts / f are caller / stack memory
    P.nparts_override = c->d_nparts;
    void *dw, *dh;
    rc = stage_out(c, SLOT_OUT0, wet, (size_t)r->n * 8, r->loc, &dw); if (rc) return rc;
    rc = stage_out(c, SLOT_OUT1, hydro, (size_t)r->n * 8, r->loc, &dh); if (rc) return rc;
    P.wet = (double*)dw; P.hyd = (double*)dh;
    rc = march_on_records(c, q, R, reuse); if (rc) return rc;
    rc = finish_out(c, wet, dw, (size_t)r->n * 8, r->loc); if (rc) return rc;
    rc = finish_out(c, hydro, dh, (size_t)r->n * 8, r->loc); if (rc) return rc;
    if (r->loc == RDR_HOST) HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

// One batch of rays through D epoch cubes qs[] (epochs_check; D = 1: rdr_raytrace), per-ray heights (rays->hts) included: one pass 1
// through ray_passes' workspace schedule, every chunk's pass 2 through launch_march_epochs.  Epoch e's delays are block e of [D][n];
// nparts_out / flags_out are pass 1's, shared by every epoch.  The entries have checked their NULL arguments; `who` prefixes the rest.
static int raytrace_impl(rdr_ctx* c, const char* who, const rdr_cube* const* qs, int32_t D, const rdr_rays* r, double ht, double zref,
                         double max_seg, double* wet, double* hydro, int32_t* nparts_out, int32_t* flags_out) {
    const rdr_cube* q = qs[0];
    RayCall R;
    int rc = R.check(c, who, qs, D, r, ht, zref, max_seg); if (rc) return rc;
    if (r->n == 0) return RDR_OK;
    const int K = R.K;
    RayParams& P = R.P;
    // one epoch, large host-buffer batches with per-ray look vectors: overlap the PCIe transfers with the two passes (raytrace_pipelined)
    bool pipelined = D == 1 && r->loc == RDR_HOST && r->n >= (1 << 21) && pipelining();
    const bool los_chunks = pipelined && r->los_mode == RDR_LOS_VEC;
    const bool hts_chunks = pipelined && r->hts != nullptr;
    rdr_rays rr = *r;
    if (los_chunks) rr.los = nullptr;                      // the look vectors are uploaded chunk by chunk below
    if (hts_chunks) rr.hts = nullptr;                      // ... and so are per-pixel heights
    rc = R.stage(c, &rr); if (rc) return rc;
    if (pipelined && P.ntiles > ws_chunk_tiles(c, K)) {   // records do not fit: ordinary (chunked-march) path
        const void* d;
        if (los_chunks) {
            rc = stage_in(c, SLOT_IN3, r->los, (size_t)r->n * 24, r->loc, &d); if (rc) return rc;
            P.los = (const double*)d;
        }
        if (hts_chunks) {
            rc = stage_in(c, SLOT_IN6, r->hts, (size_t)r->n * 8, r->loc, &d); if (rc) return rc;
            P.ht_ray = (const double*)d;
        }
        pipelined = false;
    }
    const size_t bytes = (size_t)r->n * (size_t)D * 8;
    void *dw, *dh;
    rc = stage_out(c, SLOT_OUT0, wet, bytes, r->loc, &dw); if (rc) return rc;
    rc = stage_out(c, SLOT_OUT1, hydro, bytes, r->loc, &dh); if (rc) return rc;
    P.wet = (double*)dw; P.hyd = (double*)dh;
    rc = partition_reset(c, 1); if (rc) return rc;
    if (pipelined) {
        void *dl = nullptr, *dhts = nullptr;
        if (los_chunks) { rc = ensure(c, SLOT_IN3, (size_t)r->n * 24, &dl); if (rc) return rc; }
        if (hts_chunks) { rc = ensure(c, SLOT_IN6, (size_t)r->n * 8, &dhts); if (rc) return rc; }
        rc = raytrace_pipelined(c, q, r, P, K, (double*)dl, (double*)dhts, (double*)dw, (double*)dh, wet, hydro); if (rc) return rc;
    } else {
        // one slice: pass 1 reduces AND stores the ray records when they all fit, pass 2 streams them back; else chunked
        std::function<int(const RayParams&, int64_t, int64_t)> march;      // (one epoch: ray_passes' own launch_march)
        if (D > 1) march = [&](const RayParams& Pm, int64_t tb, int64_t tc) { return launch_march_epochs(c, qs, D, Pm, tb, tc, (int64_t)r->n); };
        rc = ray_passes(c, q, P, K, P.ntiles, 1, ws_chunk_tiles(c, K), 1, true, march, nullptr, D == 1 && r->loc == RDR_DEVICE); if (rc) return rc;
        rc = finish_out(c, wet, dw, bytes, r->loc); if (rc) return rc;
        rc = finish_out(c, hydro, dh, bytes, r->loc); if (rc) return rc;
    }
    const bool need_sync = r->loc == RDR_HOST || nparts_out || flags_out;
    if (need_sync) {
        std::vector<double> ml(K);
        int f = 0;
        rc = partition_read(c, ml.data(), (size_t)K, &f, 1, false); if (rc) return rc;
        if (nparts_out) rdr_nparts(ml.data(), K, max_seg, nparts_out);
        if (flags_out) *flags_out = f;
        return flags_to_status(c, f);
    }
    return RDR_OK;
}

int rdr_raytrace(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, double ht, double zref, double max_seg, double* wet,
                 double* hydro, int32_t* nparts_out, int32_t* flags_out) {
    if (!c || !q || !wet || !hydro) return fail(c, RDR_ERR_INVALID, "rdr_raytrace: NULL argument");
    return raytrace_impl(c, "rdr_raytrace", &q, 1, r, ht, zref, max_seg, wet, hydro, nparts_out, flags_out);
}

// ---- height slices, and a time series of E weather epochs through one ray geometry (rdr_raytrace_slices[_epochs]) -----------------
// Every epoch must be the same grid: shape, dtype, bitwise-equal axes and the same projection - then one pass-1 record set (ray
// polynomials, crossings, the slice partition) serves them all.  Returns RDR_OK or RDR_ERR_INVALID naming the first epoch that differs.
static int epochs_check(rdr_ctx* c, const char* who, const rdr_cube* const* qs, int32_t ncubes) {
    const std::string w(who);
    if (!c) return fail(nullptr, RDR_ERR_INVALID, w + ": NULL context");
    if (!qs) return fail(c, RDR_ERR_INVALID, w + ": cubes is NULL");
    if (ncubes <= 0) return fail(c, RDR_ERR_INVALID, w + ": ncubes must be >= 1");
    for (int32_t e = 0; e < ncubes; ++e)
        if (!qs[e]) return fail(c, RDR_ERR_INVALID, w + ": cubes[" + std::to_string(e) + "] is NULL");
    const rdr_cube* a = qs[0];
    for (int32_t e = 1; e < ncubes; ++e) {
        const rdr_cube* b = qs[e];
        const std::string tag = w + ": epoch " + std::to_string(e) + " ";
        if (b->ny != a->ny || b->nx != a->nx || b->nz != a->nz)
            return fail(c, RDR_ERR_INVALID, tag + "has shape (" + std::to_string(b->ny) + ", " + std::to_string(b->nx) + ", " + std::to_string(b->nz) +
                                                 "), epoch 0 (" + std::to_string(a->ny) + ", " + std::to_string(a->nx) + ", " + std::to_string(a->nz) + ")");
        if (b->dtype != a->dtype) return fail(c, RDR_ERR_INVALID, tag + "has another dtype than epoch 0 (float32 / float64 cubes do not mix)");
        const char* names[3] = {"y", "x", "z"};
        const std::vector<double>* ax[3] = {&a->ys, &a->xs, &a->zs};
        const std::vector<double>* bx[3] = {&b->ys, &b->xs, &b->zs};
        for (int k = 0; k < 3; ++k)
            if (std::memcmp(ax[k]->data(), bx[k]->data(), ax[k]->size() * sizeof(double)) != 0)
                return fail(c, RDR_ERR_INVALID, tag + "has another " + names[k] + " axis than epoch 0 (the axes must be bitwise equal)");
        const LccParams &p = a->proj, &r = b->proj;
        if (p.kind != r.kind || std::memcmp(&p.n, &r.n, sizeof(double)) || std::memcmp(&p.aF, &r.aF, sizeof(double)) || std::memcmp(&p.rho0, &r.rho0, sizeof(double)) ||
            std::memcmp(&p.lam0, &r.lam0, sizeof(double)) || std::memcmp(&p.x0, &r.x0, sizeof(double)) || std::memcmp(&p.y0, &r.y0, sizeof(double)) ||
            std::memcmp(&p.e, &r.e, sizeof(double)))
            return fail(c, RDR_ERR_INVALID, tag + "has another projection (kind " + std::to_string(r.kind) + ") than epoch 0 (kind " + std::to_string(p.kind) + " or other parameters)");
    }
    return RDR_OK;
}

// ---- a date series at query points (rdr_interp3_project_epochs, rdr_point_delays_epochs) --------------------------------------------
// The gather of D epochs that share one grid: `q` describes that grid (shape, axes, dtype), vals[e] is epoch e's value buffer.
template <typename T2, int E>
static void launch_points_stacked(rdr_ctx* c, const rdr_cube* q, const void* const* vals, const PointQuery& Q, int64_t pstride, int64_t cnt, int64_t estride,
                                  double* dw, double* dh) {
    EpochCubes<T2, E> ev;
    for (int j = 0; j < E; ++j) ev.v[j] = (const T2*)vals[j];
    const int g = grid_for(cnt, 256, c->num_cus * 8);
    hipLaunchKernelGGL((interp_points_epochs_kernel<T2, E>), dim3(g), dim3(256), axes_smem(q), c->stream, make_view<T2>(q), ev, Q, pstride, cnt, estride, dw, dh,
                       (int)axes_fit_lds(q));
}

// groups of 4, then 2, then 1 epochs (epoch_group).  dw / dh: epoch 0's block, epoch e's is
// estride doubles further; Q.proj: epoch 0's divisors, epoch e's pstride doubles further (pstride 0: shared).
static void launch_interp_epochs(rdr_ctx* c, const rdr_cube* q, const void* const* vals, int D, const PointQuery& Q, int64_t pstride, int64_t cnt, int64_t estride,
                                 double* dw, double* dh) {
    const int emax = epochs_max();
    for (int e = 0; e < D;) {
        const int ge = epoch_group(q->dtype, false, D - e, emax);
        PointQuery Qe = Q;
        if (Qe.proj) Qe.proj += (int64_t)e * pstride;
        double* we = dw ? dw + (int64_t)e * estride : nullptr;
        double* he = dh ? dh + (int64_t)e * estride : nullptr;
        KTimer t(c, 2);
        by_dtype(q, [&](auto tag) {
            typedef decltype(tag) T2;
            if (ge == 4) launch_points_stacked<T2, 4>(c, q, vals + e, Qe, pstride, cnt, estride, we, he);
            else if (ge == 2) launch_points_stacked<T2, 2>(c, q, vals + e, Qe, pstride, cnt, estride, we, he);
            else launch_points_stacked<T2, 1>(c, q, vals + e, Qe, pstride, cnt, estride, we, he);
        });
        e += ge;
    }
}

// the checks the two entries share, after epochs_check: the point query's own, and the divisor stride
static int epochs_point_args(rdr_ctx* c, const char* who, const double* y, const double* x, const double* z, int64_t n, int pmode, const double* proj,
                             int64_t proj_stride, const double* wet, const double* hydro) {
    int rc = point_query_args(c, who, y, x, z, n, pmode, proj, wet, hydro); if (rc) return rc;
    if (proj_stride != 0 && proj_stride != n)
        return fail(c, RDR_ERR_INVALID, std::string(who) + ": proj_stride is 0 (one proj[n] for every epoch) or n (proj[ncubes][n]), got " + std::to_string(proj_stride));
    return RDR_OK;
}

int rdr_interp3_project_epochs(rdr_ctx* c, const rdr_cube* const* cubes, int32_t ncubes, const double* y, const double* x, const double* z, int64_t n,
                               int proj_mode, const double* proj, int64_t proj_stride, double inc0, double* wet, double* hydro, int loc) {
    static const char* who = "rdr_interp3_project_epochs";
    int rc = epochs_check(c, who, cubes, ncubes); if (rc) return rc;
    rc = epochs_point_args(c, who, y, x, z, n, proj_mode, proj, proj_stride, wet, hydro); if (rc) return rc;
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, std::string(who) + ": loc is RDR_HOST or RDR_DEVICE");
    c->point_upload_bytes = 0;
    if (ncubes == 1) return interp3_impl(c, who, cubes[0], y, x, z, n, proj_mode, proj, inc0, wet, hydro, loc);
    if (loc == RDR_DEVICE) {
        // Device-resident points: there is no upload to share, and the one-cube gather per date is the faster one (measured, DESIGN.md 5d:
        // it keeps one cube's lines in L2 at a time and takes the corner-quad copy on large cubes) - the per-date loop behind this entry.
        const int64_t ps = (proj_mode == 1 || proj_mode == 3) ? proj_stride : 0;
        for (int32_t e = 0; e < ncubes; ++e) {
            rc = interp3_impl(c, who, cubes[e], y, x, z, n, proj_mode, proj ? proj + (int64_t)e * ps : nullptr, inc0, wet ? wet + (int64_t)e * n : nullptr,
                              hydro ? hydro + (int64_t)e * n : nullptr, loc);
            if (rc) return rc;
        }
        return RDR_OK;
    }
    const rdr_cube* q = cubes[0];
    for (int32_t e = 0; e < ncubes; ++e) note_use(c, cubes[e]);
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    const int D = ncubes;
    std::vector<const void*> vals((size_t)D);
    for (int e = 0; e < D; ++e) vals[(size_t)e] = cubes[e]->d_vals;
    const PointQuery Q = make_query(proj_mode, inc0);
    const int64_t pstride = (proj_mode == 1 || proj_mode == 3) ? proj_stride : 0;
    if (loc == RDR_HOST && n >= (1 << 18) && pipelining()) {
        return interp_pipeline_impl(c, who, q, false, BlendSpec(), vals.data(), D, y, x, z, n, Q, proj, pstride, wet, hydro, k_gather_slots);
    }
    return gather_staged(c, Q, y, x, z, proj, pstride, n, D, wet, hydro, loc, [&](const PointQuery& Qd, double* dw, double* dh) {
        launch_interp_epochs(c, q, vals.data(), D, Qd, pstride, n, n, dw, dh);
    });
}

int64_t rdr_point_upload_bytes(const rdr_ctx* c) { return c ? c->point_upload_bytes : -1; }

// point_delays_impl for D dates: the D intermediate cubes built one after the other (build_cube_impl + the packer, as there) into D
// regions of one scratch allocation, each with its own NaN word; the points travel up ONCE on the copy stream under the first build;
// one gather pass (interp_pipeline_impl) then serves every date.  Same kernels and arithmetic per date as rdr_point_delays[_grid]:
// the same bits.
int rdr_point_delays_epochs(rdr_ctx* c, const rdr_cube* const* cubes, int32_t ncubes, int grid_kind, const double* params, int nparams,
                            const double* xpts, int64_t nx, const double* ypts, int64_t ny, const double* zpts, int64_t nz,
                            const double* y, const double* x, const double* z, int64_t n, int proj_mode, const double* proj, int64_t proj_stride, double inc0,
                            double* wet, double* hydro, int32_t* cube_has_nan) {
    static const char* who = "rdr_point_delays_epochs";
    const std::string w(who);
    int rc = epochs_check(c, who, cubes, ncubes); if (rc) return rc;
    if (!xpts || !ypts || !zpts) return fail(c, RDR_ERR_INVALID, w + ": NULL argument");
    if (nparams < 0) return fail(c, RDR_ERR_INVALID, w + ": negative nparams");
    GridCrs g;
    const GridCrs* grid = nullptr;
    if (nparams > 0) { rc = grid_crs(c, who, grid_kind, params, nparams, g); if (rc) return rc; grid = &g; }
    rc = epochs_point_args(c, who, y, x, z, n, proj_mode, proj, proj_stride, wet, hydro); if (rc) return rc;
    c->point_upload_bytes = 0;
    if (ncubes == 1) return point_delays_impl(c, who, cubes[0], grid, xpts, nx, ypts, ny, zpts, nz, y, x, z, n, proj_mode, proj, inc0, wet, hydro, cube_has_nan);
    rc = point_grid_args(c, w, nx, ny, nz); if (rc) return rc;
    // the intermediate cubes: ONE scratch description (shape, axes), D value regions (they do not fit: RDR_ERR_OOM, the caller goes date by date)
    const int D = ncubes;
    const size_t total = (size_t)ny * nx * nz;
    int fy, fx, fz;
    rdr_cube tmp;
    std::vector<double> ax;
    rc = scratch_cube_setup(c, tmp, xpts, nx, ypts, ny, zpts, nz, D, &fy, &fx, &fz, ax); if (rc) return rc;
    void* dnan;
    rc = ensure(c, SLOT_OUT2, (size_t)D * sizeof(int), &dnan); if (rc) return rc;
    std::vector<const void*> vals((size_t)D);
    std::vector<int> nanw((size_t)D, 0);
    StreamsQuiesce quiesce(c);                  // (`ax`, `nanw`, the caller's points and outputs: nothing may still be copying when an error returns)
    HIPCHECK(c, hipMemcpyAsync(tmp.d_axes, ax.data(), ax.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipMemsetAsync(dnan, 0, (size_t)D * sizeof(int), c->stream));
    for (int e = 0; e < D; ++e) {
        double2* dv = (double2*)tmp.d_vals + (size_t)e * total;
        vals[(size_t)e] = dv;
        int* const nf = (int*)dnan + e;
        double* planar[2] = {nullptr, nullptr};
        rc = build_cube_impl(c, cubes[e], xpts, nx, ypts, ny, zpts, nz, nullptr, nullptr, RDR_HOST, planar, nullptr, grid); if (rc) return rc;
        pack_planar(c, planar, dv, ny, nx, nz, fy, fx, fz, nf);
        HIPCHECK(c, hipGetLastError());
    }
    if (n > 0) {
        const int64_t pstride = (proj_mode == 1 || proj_mode == 3) ? proj_stride : 0;
        rc = interp_pipeline_impl(c, who, &tmp, false, BlendSpec(), vals.data(), D, y, x, z, n, make_query(proj_mode, inc0), proj, pstride, wet, hydro, k_point_slots);
        if (rc) return rc;
    }
    // the D NaN words, after everything else has been enqueued (a pageable destination: the host waits here, with nothing left to overlap)
    HIPCHECK(c, hipMemcpyAsync(nanw.data(), dnan, (size_t)D * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    quiesce.armed = false;
    if (cube_has_nan) for (int e = 0; e < D; ++e) cube_has_nan[e] = nanw[(size_t)e] != 0;
    scratch_trim_point_delays(c);
    return RDR_OK;
}

// Several height slices of _build_cube_ray in ONE pass-1 / pass-2 launch pair (delay.py:256-323 loops over them): a production
// job is ~20 heights x 1e4-1e5 rays (aria/prepFromGUNW.py:173,180), and one such slice fills a fraction of the chip.  Tiles are
// numbered slice-major; per-level maxima / flags / nParts stay per slice (RayParams), so the result is what slice-by-slice
// calls give, bit for bit.  The D epoch cubes qs[] (epochs_check) share that pass 1; pass 2 runs per epoch (launch_march_epochs),
// epoch e's delays are block e of [D][nslices][n] and its flags row e of flags_out.  D = 1 is rdr_raytrace_slices.
// The entries have checked their own arguments (NULL, the cubes, per-ray heights, a series' empty batch); `who` prefixes the rest.
// keep == NULL: the public entries; keep != NULL: the delays stay in the context's scratch (planar, keep[0] = wet, keep[1] = hydro)
// for the _to_cube(s) entries - nothing is downloaded, the partition outputs are still read back.
static int raytrace_slices_impl(rdr_ctx* c, const char* who, const rdr_cube* const* qs, int32_t D, const rdr_rays* r, const double* hts,
                                int32_t nslices, int32_t los_per_slice, double zref, double max_seg, double* wet, double* hydro,
                                int32_t* K_out, int32_t* nparts_out, int32_t ld, int32_t* flags_out, double** keep) {
    const std::string w(who);
    const rdr_cube* q = qs[0];
    for (int32_t e = 0; e < D; ++e) note_use(c, qs[e]);
    if (nslices < 1 || nslices > MAX_SLICES) return fail(c, RDR_ERR_INVALID, w + ": 1..512 slices per call");
    if (!(max_seg > 0)) return fail(c, RDR_ERR_INVALID, w + ": MAX_SEGMENT_LENGTH must be positive");
    if (nparts_out && ld < (int32_t)q->nz - 1) return fail(c, RDR_ERR_INVALID, w + ": nparts_out needs a row length of at least nz-1");
    int rc = check_rays(c, r); if (rc) return rc;
    if (r->origin_mode == RDR_ORIGIN_XYZ && nslices > 1) return fail(c, RDR_ERR_INVALID, w + ": XYZ origins belong to one height; use GRID or LLH origins");
    std::vector<int> Ks(nslices);
    int Kmax = 0;
    for (int s = 0; s < nslices; ++s) {
        std::vector<double> lo, hi; std::vector<int> kz;
        Ks[s] = levels_host(q->zs, hts[s], zref, lo, hi, kz);
        Kmax = std::max(Kmax, Ks[s]);
        if (K_out) K_out[s] = Ks[s];
    }
    if (r->n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    RayParams P;
    rc = stage_rays(c, r, P, los_per_slice ? nslices : 1); if (rc) return rc;
    const int64_t per = P.ntiles;                                   // tiles of one slice
    const size_t nout = (size_t)r->n * nslices, total = nout * (size_t)D;
    void *dw, *dh;
    const int out_loc = keep ? RDR_DEVICE : r->loc;                 // where the delays end up
    rc = stage_out(c, SLOT_OUT0, wet, total * 8, keep ? RDR_HOST : r->loc, &dw); if (rc) return rc;
    rc = stage_out(c, SLOT_OUT1, hydro, total * 8, keep ? RDR_HOST : r->loc, &dh); if (rc) return rc;
    // RDR_FLAG_NAN_OUTPUT: one epoch's bits go straight into the slice flags; several epochs keep theirs apart ([D][nslices])
    int* dnan = c->d_flags;
    if (D > 1) { void* def; rc = ensure(c, SLOT_OUT2, (size_t)D * nslices * sizeof(int), &def); if (rc) return rc; dnan = (int*)def; }
    if (keep) { keep[0] = (double*)dw; keep[1] = (double*)dh; }
    const void* dht;
    rc = stage_in(c, SLOT_AUX, hts, (size_t)nslices * 8, RDR_HOST, &dht); if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));                   // (hts is the caller's memory)
    P.nslices = nslices; P.tiles_per_slice = per; P.hts = (const double*)dht; P.los_stride = los_per_slice ? r->n : 0;
    P.ntiles = per * nslices;
    P.ht = hts[0]; P.zref = zref; P.max_seg = max_seg;
    P.wet = (double*)dw; P.hyd = (double*)dh;
    rc = partition_reset(c, nslices); if (rc) return rc;
    if (D > 1) HIPCHECK(c, hipMemsetAsync(dnan, 0, (size_t)D * nslices * sizeof(int), c->stream));
    const int K = std::max(Kmax, 1);
    const int64_t fit = ws_chunk_tiles(c, K);
    // Host outputs of a large one-epoch batch come down slice group by slice group on the copy stream while the next groups are
    // integrated (all kernels are enqueued first: a copy into pageable memory blocks the host thread, not the device).
    const bool pipe = D == 1 && out_loc == RDR_HOST && nslices >= 2 && nout * 16 >= ((size_t)32 << 20) && per <= fit && pipelining();
    // a NaN anywhere in the outputs of slices [s0, s0+ns) of [D][nslices] -> their RDR_FLAG_NAN_OUTPUT (the caller's np.isnan(...).any(), delay.py:187)
    const auto nan_scan = [&](int64_t s0, int64_t ns) {
        hipLaunchKernelGGL(nan_scan_kernel, dim3(grid_for(ns * r->n, 256, c->num_cus * 8)), dim3(256), 0, c->stream,
                           (const double*)dw + (size_t)s0 * r->n, (const double*)dh + (size_t)s0 * r->n, (int64_t)ns * r->n, (int64_t)r->n, dnan + s0);
        HIPCHECK(c, hipGetLastError());
        return RDR_OK;
    };
    EventList gev;                                       // one per finished group
    std::vector<std::pair<int64_t, int64_t>> groups;
    // groups of whole slices: usually one; up to 8 when the outputs are downloaded group by group
    rc = ray_passes(c, q, P, K, per, nslices, fit, pipe ? std::max<int64_t>(1, (nslices + 7) / 8) : nslices, true,
                    [&](const RayParams& Pm, int64_t tb, int64_t tc) { return launch_march_epochs(c, qs, D, Pm, tb, tc, (int64_t)nout); },
                    [&](int64_t s0, int64_t ns) {
                        if (!pipe) return RDR_OK;
                        const int rc_ = nan_scan(s0, ns); if (rc_) return rc_;
                        if (!gev.add(1) || hipEventRecord(gev.v.back(), c->stream) != hipSuccess) return fail(c, RDR_ERR_HIP, w + ": event");
                        groups.emplace_back(s0, ns);
                        return RDR_OK;
                    });
    if (rc) return rc;
    if (pipe) {
        int status = RDR_OK;
        for (size_t k = 0; k < groups.size() && status == RDR_OK; ++k) {
            const size_t off = (size_t)groups[k].first * r->n, cnt = (size_t)groups[k].second * r->n;
            if (hipStreamWaitEvent(c->copy_stream, gev.v[k], 0) != hipSuccess ||
                hipMemcpyAsync(wet + off, (const double*)dw + off, cnt * 8, hipMemcpyDeviceToHost, c->copy_stream) != hipSuccess ||
                hipMemcpyAsync(hydro + off, (const double*)dh + off, cnt * 8, hipMemcpyDeviceToHost, c->copy_stream) != hipSuccess)
                status = fail(c, RDR_ERR_HIP, w + ": output download failed");
        }
        if (hipStreamSynchronize(c->copy_stream) != hipSuccess && status == RDR_OK) status = fail(c, RDR_ERR_HIP, w + ": sync");
        if (status != RDR_OK) return status;
    } else {
        rc = nan_scan(0, (int64_t)D * nslices); if (rc) return rc;   // (scan the finished outputs before they leave)
        rc = finish_out(c, wet, dw, total * 8, out_loc); if (rc) return rc;
        rc = finish_out(c, hydro, dh, total * 8, out_loc); if (rc) return rc;
    }
    const bool need_sync = r->loc == RDR_HOST || nparts_out || flags_out;
    if (need_sync) {
        std::vector<double> ml((size_t)nslices * MAX_LEVELS);
        std::vector<int> f(nslices), ef(D > 1 ? (size_t)D * nslices : 0);
        rc = partition_read(c, ml.data(), ml.size(), f.data(), (size_t)nslices, false, ef.data(), dnan, ef.size() * sizeof(int)); if (rc) return rc;
        for (int s = 0; s < nslices; ++s) {
            if (nparts_out) rdr_nparts(ml.data() + (size_t)s * MAX_LEVELS, Ks[s], max_seg, nparts_out + (size_t)s * ld);
            if (flags_out)
                for (int32_t e = 0; e < D; ++e) flags_out[(size_t)e * nslices + s] = f[s] | (D > 1 ? ef[(size_t)e * nslices + s] : 0);
        }
    }
    return RDR_OK;
}

// The _to_cube(s) entries: raytrace_slices_impl with its delays left in scratch, made into D float64 cubes with axes (ypts, xpts, hts)
// on the device.  The entries have checked that the batch is a GRID (or an LLH batch with its grid's axes, cube_batch) of at least two
// nodes per axis.
static int raytrace_slices_to_cubes(rdr_ctx* c, const char* who, const rdr_cube* const* qs, int32_t D, const rdr_rays* r, const double* hts,
                                    int32_t nslices, int32_t los_per_slice, double zref, double max_seg, int32_t* K_out, int32_t* nparts_out,
                                    int32_t ld, int32_t* flags_out, rdr_cube** out) {
    HIPCHECK(c, hipSetDevice(c->device));
    std::vector<double> hx, hy;
    int rc = axis_to_host(c, r->xpts, r->nx, r->loc, hx); if (rc) return rc;
    rc = axis_to_host(c, r->ypts, r->ny, r->loc, hy); if (rc) return rc;
    double* planar[2] = {nullptr, nullptr};
    rc = raytrace_slices_impl(c, who, qs, D, r, hts, nslices, los_per_slice, zref, max_seg, nullptr, nullptr, K_out, nparts_out, ld, flags_out, planar);
    if (rc) return rc;
    const size_t nout = (size_t)r->n * nslices;
    for (int32_t e = 0; e < D; ++e) out[e] = nullptr;
    for (int32_t e = 0; e < D; ++e) {
        rc = rdr_cube_create(c, hy.data(), r->ny, hx.data(), r->nx, hts, nslices, planar[0] + e * nout, planar[1] + e * nout, RDR_F64, r->nx, 1,
                             r->ny * r->nx, RDR_DEVICE, &out[e]);
        if (rc) {
            for (int32_t j = 0; j < e; ++j) { rdr_cube_destroy(out[j]); out[j] = nullptr; }
            return rc;
        }
    }
    return RDR_OK;
}

// the batches a delay cube can be made of: GRID, or LLH origins of a projected output grid (rdr_grid_geodetic) that carry the grid's
// axes in xpts / ypts with n == nx * ny
static bool cube_batch(const rdr_rays* r) {
    if (r->origin_mode == RDR_ORIGIN_GRID) return true;
    return r->origin_mode == RDR_ORIGIN_LLH && r->xpts && r->ypts && r->nx > 0 && r->ny > 0 && r->nx <= r->n / r->ny && r->nx * r->ny == r->n;
}

static const char k_one_batch[] = "rdr_raytrace_slices: per-ray heights (rays->hts) describe ONE batch; use rdr_raytrace";

// what a series refuses on top of the checks rdr_raytrace_slices makes (r is not NULL)
static int series_rays_check(rdr_ctx* c, const std::string& w, const rdr_rays* r) {
    if (r->n == 0) return fail(c, RDR_ERR_INVALID, w + ": empty ray batch");
    if (r->hts) return fail(c, RDR_ERR_INVALID, w + ": per-ray heights (rays->hts) are not supported in a series");
    return RDR_OK;
}

int rdr_raytrace_slices(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, const double* hts, int32_t nslices, int32_t los_per_slice,
                        double zref, double max_seg, double* wet, double* hydro, int32_t* K_out, int32_t* nparts_out, int32_t ld,
                        int32_t* flags_out) {
    if (!c || !q || !hts || !wet || !hydro) return fail(c, RDR_ERR_INVALID, "rdr_raytrace_slices: NULL argument");
    if (r && r->hts) return fail(c, RDR_ERR_INVALID, k_one_batch);
    return raytrace_slices_impl(c, "rdr_raytrace_slices", &q, 1, r, hts, nslices, los_per_slice, zref, max_seg, wet, hydro, K_out, nparts_out,
                                ld, flags_out, nullptr);
}

int rdr_raytrace_slices_to_cube(rdr_ctx* c, const rdr_cube* q, const rdr_rays* r, const double* hts, int32_t nslices, int32_t los_per_slice,
                                double zref, double max_seg, int32_t* K_out, int32_t* nparts_out, int32_t ld, int32_t* flags_out,
                                rdr_cube** out) {
    if (!c || !q || !r || !hts || !out) return fail(c, RDR_ERR_INVALID, "rdr_raytrace_slices_to_cube: NULL argument");
    if (!cube_batch(r)) return fail(c, RDR_ERR_INVALID, "rdr_raytrace_slices_to_cube: the delay cube is a GRID batch (xpts, ypts) x heights, or an LLH batch of nx * ny rays with its grid's axes");
    if (r->nx < 2 || r->ny < 2 || nslices < 2) return fail(c, RDR_ERR_INVALID, "rdr_raytrace_slices_to_cube: the delay cube needs two nodes per axis");
    if (r->hts) return fail(c, RDR_ERR_INVALID, k_one_batch);
    return raytrace_slices_to_cubes(c, "rdr_raytrace_slices", &q, 1, r, hts, nslices, los_per_slice, zref, max_seg, K_out, nparts_out, ld,
                                    flags_out, out);
}

int rdr_raytrace_slices_epochs(rdr_ctx* c, const rdr_cube* const* cubes, int32_t ncubes, const rdr_rays* r, const double* hts, int32_t nslices,
                               int32_t los_per_slice, double zref, double max_seg, double* wet, double* hydro, int32_t* K_out, int32_t* nparts_out,
                               int32_t ld, int32_t* flags_out) {
    static const char* who = "rdr_raytrace_slices_epochs";
    int rc = epochs_check(c, who, cubes, ncubes); if (rc) return rc;
    if (!r || !hts || !wet || !hydro) return fail(c, RDR_ERR_INVALID, std::string(who) + ": NULL argument");
    rc = series_rays_check(c, who, r); if (rc) return rc;
    return raytrace_slices_impl(c, who, cubes, ncubes, r, hts, nslices, los_per_slice, zref, max_seg, wet, hydro, K_out, nparts_out, ld,
                                flags_out, nullptr);
}

int rdr_raytrace_slices_epochs_to_cubes(rdr_ctx* c, const rdr_cube* const* cubes, int32_t ncubes, const rdr_rays* r, const double* hts,
                                        int32_t nslices, int32_t los_per_slice, double zref, double max_seg, int32_t* K_out, int32_t* nparts_out,
                                        int32_t ld, int32_t* flags_out, rdr_cube** out) {
    static const char* who = "rdr_raytrace_slices_epochs_to_cubes";
    int rc = epochs_check(c, who, cubes, ncubes); if (rc) return rc;
    if (!r || !hts || !out) return fail(c, RDR_ERR_INVALID, std::string(who) + ": NULL argument");
    if (!cube_batch(r)) return fail(c, RDR_ERR_INVALID, std::string(who) + ": the delay cubes are a GRID batch (xpts, ypts) x heights, or an LLH batch of nx * ny rays with its grid's axes");
    if (r->nx < 2 || r->ny < 2 || nslices < 2) return fail(c, RDR_ERR_INVALID, std::string(who) + ": the delay cubes need two nodes per axis");
    rc = series_rays_check(c, who, r); if (rc) return rc;
    return raytrace_slices_to_cubes(c, who, cubes, ncubes, r, hts, nslices, los_per_slice, zref, max_seg, K_out, nparts_out, ld, flags_out, out);
}

// rdr_raytrace for D epoch cubes on ONE ray batch (raytrace_impl).  D = 1 is rdr_raytrace itself (with its pipelined host upload).
int rdr_raytrace_epochs(rdr_ctx* c, const rdr_cube* const* cubes, int32_t ncubes, const rdr_rays* r, double ht, double zref, double max_seg,
                        double* wet, double* hydro, int32_t* nparts_out, int32_t* flags_out) {
    static const char* who = "rdr_raytrace_epochs";
    int rc = epochs_check(c, who, cubes, ncubes); if (rc) return rc;
    if (!wet || !hydro) return fail(c, RDR_ERR_INVALID, std::string(who) + ": NULL argument");
    if (ncubes == 1) return rdr_raytrace(c, cubes[0], r, ht, zref, max_seg, wet, hydro, nparts_out, flags_out);
    return raytrace_impl(c, who, cubes, ncubes, r, ht, zref, max_seg, wet, hydro, nparts_out, flags_out);
}

int rdr_top_of_atmosphere(rdr_ctx* c, const double* xyz, const double* los, int64_t n, double h, const double* factor, double* pos, int loc) {
    if (!c || !xyz || !los || !pos) return fail(c, RDR_ERR_INVALID, "rdr_top_of_atmosphere: NULL argument");
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_top_of_atmosphere: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *dx = S.in(xyz, (size_t)n * 24), *dl = S.in(los, (size_t)n * 24), *df = S.in(factor, (size_t)n * 8);   // (factor is optional)
    double* dp = S.out(pos, (size_t)n * 24);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(toa_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, dx, dl, n, h, df, dp);
    return S.finish();
}

int rdr_build_ray(rdr_ctx* c, const double* model_zs, int64_t nz, double ht, const double* xyz, const double* los, int64_t n,
                  double zref, int32_t* K_out, double* lengths, double* low, double* high, int loc) {
    if (!c || !model_zs || !xyz || !los || !K_out) return fail(c, RDR_ERR_INVALID, "rdr_build_ray: NULL argument");
    if (nz < 2) return fail(c, RDR_ERR_INVALID, "rdr_build_ray: need at least 2 model levels");
    std::vector<double> zs(model_zs, model_zs + nz), lo, hi; std::vector<int> kz;
    const int K = levels_host(zs, ht, zref, lo, hi, kz);
    *K_out = K;
    if (K == 0) return fail_no_levels(c);
    if (!lengths || !low || !high) return RDR_OK;   // size query
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_build_ray: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *dx = S.in(xyz, (size_t)n * 24), *dl = S.in(los, (size_t)n * 24);
    double *dlen = S.out(lengths, (size_t)K * n * 8), *dlo = S.out(low, (size_t)K * n * 24), *dhi = S.out(high, (size_t)K * n * 24);
    const HostPart tab[2] = {{lo.data(), (size_t)K * 8}, {hi.data(), (size_t)K * 8}};           // the level table: K lower | K upper bounds
    const double* dtab = S.table<double>(SLOT_AUX, tab, 2);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(build_ray_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, dx, dl, n, K, dtab, dlen, dlo, dhi);
    return S.finish();
}

// ---- geodesy ------------------------------------------------------------------------------------------
int rdr_lla2ecef(rdr_ctx* c, const double* lat, const double* lon, const double* h, int64_t n, double* xyz, int loc) {
    if (!c || !lat || !lon || !h || !xyz) return fail(c, RDR_ERR_INVALID, "rdr_lla2ecef: NULL argument");
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_lla2ecef: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *a = S.in(lat, (size_t)n * 8), *b = S.in(lon, (size_t)n * 8), *d = S.in(h, (size_t)n * 8);
    double* o = S.out(xyz, (size_t)n * 24);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(lla2ecef_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, a, b, d, n, o);
    return S.finish();
}

int rdr_ecef2lla(rdr_ctx* c, const double* xyz, int64_t n, double* lon, double* lat, double* h, int loc) {
    if (!c || !xyz || !lon || !lat || !h) return fail(c, RDR_ERR_INVALID, "rdr_ecef2lla: NULL argument");
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_ecef2lla: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double* a = S.in(xyz, (size_t)n * 24);
    double *o0 = S.out(lon, (size_t)n * 8), *o1 = S.out(lat, (size_t)n * 8), *o2 = S.out(h, (size_t)n * 8);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(ecef2lla_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, a, n, o0, o1, o2);
    return S.finish();
}

int rdr_look_vectors(rdr_ctx* c, const rdr_rays* r, double ht, double* los) {
    (void)ht;
    if (!c || !los) return fail(c, RDR_ERR_INVALID, "rdr_look_vectors: NULL argument");
    int rc = check_rays(c, r); if (rc) return rc;
    if (r->origin_mode == RDR_ORIGIN_XYZ && (!r->lat || !r->lon) && r->los_mode != RDR_LOS_VEC)
        return fail(c, RDR_ERR_INVALID, "rdr_look_vectors: lat/lon required");
    if (r->n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    RayParams P;
    rc = stage_rays(c, r, P); if (rc) return rc;
    Staged S(c, r->loc);
    double* o = S.out(los, (size_t)r->n * 24);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(look_kernel, dim3(grid_for(r->n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, P, o);
    return S.finish();
}

int rdr_cubes_from_model_levels(rdr_ctx* c, const double* ys, int64_t ny, const double* xs, int64_t nx, const double* zs3, const double* p,
                                const double* t, const double* hum, int humidity_type, int64_t nlev, const double* new_z, int64_t nz,
                                double k1, double k2, double k3, double zmin, int loc, rdr_cube** pointwise, rdr_cube** total,
                                float* t_out, float* p_out, float* e_out) {
    if (!c || !ys || !xs || !zs3 || !p || !t || !hum || !new_z || !pointwise || !total) return fail(c, RDR_ERR_INVALID, "rdr_cubes_from_model_levels: NULL argument");
    if (humidity_type != 0 && humidity_type != 1) return fail(c, RDR_ERR_INVALID, "Not a valid humidity type");
    if (nlev < 2 || nlev > 1024 || nz < 2 || nz + 1 > MAX_LEVELS) return fail(c, RDR_ERR_INVALID, "rdr_cubes_from_model_levels: unsupported number of levels");
    int fy, fx, fz;
    if (axis_check(ys, ny, &fy) || axis_check(xs, nx, &fx) || axis_check(new_z, nz, &fz) || fy || fx || fz)
        return fail(c, RDR_ERR_INVALID, "rdr_cubes_from_model_levels: x, y and the new z levels must be strictly ascending");
    HIPCHECK(c, hipSetDevice(c->device));
    double zlow = new_z[0];
    const int pad = zmin < zlow ? 1 : 0;                              // _adjust_grid, weatherModel.py:376-378
    const int64_t nzo = nz + pad, ncol = ny * nx;
    rdr_cube* q[2] = {new rdr_cube(), new rdr_cube()};
    for (int i = 0; i < 2; ++i) {
        q[i]->ctx = c; q[i]->ny = ny; q[i]->nx = nx; q[i]->nz = nzo; q[i]->dtype = i == 0 ? RDR_F32 : RDR_F64;
        q[i]->ys.assign(ys, ys + ny); q[i]->xs.assign(xs, xs + nx);
        if (pad) q[i]->zs.push_back(zmin);
        q[i]->zs.insert(q[i]->zs.end(), new_z, new_z + nz);
        int rc = cube_alloc(c, q[i]);
        if (rc) { rdr_cube_destroy(q[0]); rdr_cube_destroy(q[1]); return rc; }
    }
    auto bail = [&](int rc) { rdr_cube_destroy(q[0]); rdr_cube_destroy(q[1]); return rc; };
    ProducerParams P;
    const void* d;
    const size_t nb = (size_t)ncol * nlev * 8;
    int rc;
    rc = stage_in(c, SLOT_IN0, zs3, nb, loc, &d); if (rc) return bail(rc); P.zs = (const double*)d;
    rc = stage_in(c, SLOT_IN1, p, nb, loc, &d); if (rc) return bail(rc); P.p = (const double*)d;
    rc = stage_in(c, SLOT_IN2, t, nb, loc, &d); if (rc) return bail(rc); P.t = (const double*)d;
    rc = stage_in(c, SLOT_IN3, hum, nb, loc, &d); if (rc) return bail(rc); P.hum = (const double*)d;
    void* dz;
    rc = ensure(c, SLOT_AUX, (size_t)nz * 8, &dz); if (rc) return bail(rc);
    if (hipMemcpyAsync(dz, new_z, (size_t)nz * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return bail(fail(c, RDR_ERR_HIP, "rdr_cubes_from_model_levels: copy of the level table failed"));
    P.new_z = (const double*)dz;
    P.ncol = ncol; P.nlev = (int)nlev; P.hum_type = humidity_type; P.nz = (int)nz; P.pad = pad;
    P.k1 = (float)k1; P.k2 = (float)k2; P.k3 = (float)k3; P.zmin = zmin; P.R_v = 461.524; P.R_d = 287.06;   // weatherModel.py:78-79
    P.pw = (float2*)q[0]->d_vals; P.tot = (double2*)q[1]->d_vals;
    void *dt_ = nullptr, *dp_ = nullptr, *de_ = nullptr;
    const size_t ob = (size_t)ncol * nzo * 4;
    if (t_out && p_out && e_out) {
        rc = stage_out(c, SLOT_OUT0, t_out, ob, loc, &dt_); if (rc) return bail(rc);
        rc = stage_out(c, SLOT_OUT1, p_out, ob, loc, &dp_); if (rc) return bail(rc);
        rc = stage_out(c, SLOT_OUT2, e_out, ob, loc, &de_); if (rc) return bail(rc);
    }
    P.t_out = (float*)dt_; P.p_out = (float*)dp_; P.e_out = (float*)de_;
    const size_t per_wave = ((size_t)4 * nlev + 3 * nzo + (5 * nzo + 1) / 2 + 1) * 8;
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>((ncol + 3) / 4, (int64_t)c->num_cus * 8));
    if (per_wave * 4 > c->lds_max)
        return bail(fail(c, RDR_ERR_INVALID, "rdr_cubes_from_model_levels: " + std::to_string(nlev) + " model levels -> " + std::to_string(nzo) +
                         " output levels need " + std::to_string(per_wave * 4) + " B of LDS per workgroup, the device offers " + std::to_string(c->lds_max)));
    hipError_t e;
    {
        KTimer tm(c, 3);
        e = launch_lds(producer_kernel, dim3(g), dim3(256), per_wave * 4, c->stream, P);
    }
    if (e == hipSuccess && dt_) {
        if (finish_out(c, t_out, dt_, ob, loc) || finish_out(c, p_out, dp_, ob, loc) || finish_out(c, e_out, de_, ob, loc)) return bail(RDR_ERR_HIP);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return bail(fail(c, RDR_ERR_HIP, std::string("producer_kernel: ") + hipGetErrorString(e)));
    *pointwise = q[0]; *total = q[1];
    return RDR_OK;
}

int rdr_ecmwf_model_levels(rdr_ctx* c, const float* z_surf, const float* lnsp, const float* t, const float* q, const float* lats,
                           const double* a, const double* b, int32_t nlev, int64_t ny, int64_t nx, double R_d, double* p_out, double* zs_out, int loc) {
    if (!c || !z_surf || !lnsp || !t || !q || !lats || !a || !b || !p_out || !zs_out) return fail(c, RDR_ERR_INVALID, "rdr_ecmwf_model_levels: NULL argument");
    if (nlev < 1 || ny < 1 || nx < 1) return fail(c, RDR_ERR_INVALID, "rdr_ecmwf_model_levels: empty grid");
    HIPCHECK(c, hipSetDevice(c->device));
    const int64_t ncol = ny * nx;
    // the small tables (latitudes, a, b) always come from the host; the fields and the outputs follow `loc`
    Staged S(c, loc);
    const HostPart tab[3] = {{a, (size_t)(nlev + 1) * 8}, {b, (size_t)(nlev + 1) * 8}, {lats, (size_t)ny * 4}};
    const double* da = S.table<double>(SLOT_AUX, tab, 3);
    const float *dz = S.in(z_surf, (size_t)ncol * 4), *ds = S.in(lnsp, (size_t)ncol * 4);
    const float *dt_ = S.in(t, (size_t)ncol * nlev * 4), *dq = S.in(q, (size_t)ncol * nlev * 4);
    double *dp = S.out(p_out, (size_t)ncol * nlev * 8), *dh = S.out(zs_out, (size_t)ncol * nlev * 8);
    if (S.rc) return S.rc;
    const double* db = da + (nlev + 1); const float* dl = (const float*)(db + (nlev + 1));
    hipLaunchKernelGGL(ecmwf_levels_kernel, dim3(grid_for(ncol, 256, c->num_cus * 8)), dim3(256), 0, c->stream, dz, ds, dt_, dq, dl, da, db, (int)nlev, ny, nx,
                       R_d, dp, dh);
    return S.finish(true);                              // (always waits: the tables in SLOT_AUX must outlive the kernel)
}

int rdr_pressure_level_state(rdr_ctx* c, const double* height, int height_kind, const double* p, int p_ndim, const double* t, const double* hum,
                             const double* lats, int lat_ndim, int64_t nlev, int64_t ny, int64_t nx, int top_first, int rows_descending,
                             int cols_descending, double* zs_out, double* p_out, double* t_out, double* hum_out, int loc, int out_loc) {
    if (!c || !height || !p || !t || !hum || !lats || !zs_out || !p_out || !t_out || !hum_out)
        return fail(c, RDR_ERR_INVALID, "rdr_pressure_level_state: NULL argument");
    if (nlev < 1 || ny < 1 || nx < 1) return fail(c, RDR_ERR_INVALID, "rdr_pressure_level_state: empty grid");
    if (nlev > ((int64_t)1 << 40) / ny / nx) return fail(c, RDR_ERR_INVALID, "rdr_pressure_level_state: grid too large");
    if (height_kind < 0 || height_kind > 2)
        return fail(c, RDR_ERR_INVALID, "rdr_pressure_level_state: height_kind must be 0 (geopotential), 1 (geopotential height) or 2 (geometric height)");
    if ((p_ndim != 1 && p_ndim != 3) || (lat_ndim != 1 && lat_ndim != 2))
        return fail(c, RDR_ERR_INVALID, "rdr_pressure_level_state: pressure is a level list (1) or a field (3), latitude per row (1) or per node (2)");
    if ((top_first | rows_descending | cols_descending) & ~1) return fail(c, RDR_ERR_INVALID, "rdr_pressure_level_state: order flags must be 0 or 1");
    if ((loc != RDR_HOST && loc != RDR_DEVICE) || (out_loc != RDR_HOST && out_loc != RDR_DEVICE))
        return fail(c, RDR_ERR_INVALID, "rdr_pressure_level_state: loc and out_loc must be RDR_HOST or RDR_DEVICE");
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t nb = (size_t)nlev * ny * nx * 8;
    PressureLevelParams P;
    Staged S(c, loc, out_loc);
    P.height = S.in(height, nb);
    P.p = S.in(p, p_ndim == 3 ? nb : (size_t)nlev * 8);
    P.t = S.in(t, nb);
    P.hum = S.in(hum, nb);
    P.lats = S.in(lats, (size_t)ny * (lat_ndim == 2 ? nx : 1) * 8);
    P.zs_out = S.out(zs_out, nb); P.p_out = S.out(p_out, nb); P.t_out = S.out(t_out, nb);
    P.hum_out = S.out(hum_out, nb, SLOT_AUX);            // (a fourth output: there are three output slots)
    if (S.rc) return S.rc;
    P.nlev = nlev; P.ny = ny; P.nx = nx;
    P.height_kind = height_kind; P.p_3d = p_ndim == 3; P.lat_2d = lat_ndim == 2;
    P.top_first = top_first; P.flip_rows = rows_descending; P.flip_cols = cols_descending;
    const int64_t ntiles = ny * ((nx + 31) / 32) * ((nlev + 31) / 32);
    hipLaunchKernelGGL(pressure_levels_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)c->num_cus * 16))), dim3(256), 0, c->stream, P);
    return S.finish();
}

int rdr_orbit_look_vectors(rdr_ctx* c, const double* sv_t, const double* sv_pos, const double* sv_vel, int64_t nsv, const double* xyz,
                           int64_t n, double threshold, int maxiter, double* los, double* aztime, double* srange, int loc) {
    if (!c || !sv_t || !sv_pos || !sv_vel || !xyz || !los) return fail(c, RDR_ERR_INVALID, "rdr_orbit_look_vectors: NULL argument");
    if (nsv < 4) return fail(c, RDR_ERR_INVALID, "state_to_los: At least 4 state vectors are required for orbit interpolation");
    for (int64_t i = 1; i < nsv; ++i) if (!(sv_t[i] > sv_t[i - 1])) return fail(c, RDR_ERR_INVALID, "rdr_orbit_look_vectors: state-vector times must be strictly increasing");
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_orbit_look_vectors: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    // the (small) state-vector table always comes from the host; targets / outputs follow `loc`
    Staged S(c, loc);
    const HostPart tab[3] = {{sv_t, (size_t)nsv * 8}, {sv_pos, (size_t)nsv * 24}, {sv_vel, (size_t)nsv * 24}};
    double* dt_ = S.table<double>(SLOT_AUX, tab, 3);
    const double* dx = S.in(xyz, (size_t)n * 24);
    double *dl = S.out(los, (size_t)n * 24), *da = S.out(aztime, (size_t)n * 8), *dr = S.out(srange, (size_t)n * 8);   // (aztime, srange: optional)
    if (S.rc) return S.rc;
    double* dp_ = dt_ + nsv; double* dv_ = dp_ + 3 * nsv;
    if (nsv <= ORBIT_LDS_MAX_SV) {
        // state vectors + per-segment reciprocals in LDS, division-free Hermite evaluation (orbit_los_fast_kernel)
        const size_t smem = ((size_t)nsv * 7 + (size_t)(nsv - 3) * 16) * sizeof(double);
        hipLaunchKernelGGL(orbit_los_fast_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), smem, c->stream, dt_, dp_, dv_, (int)nsv,
                           dx, n, threshold, maxiter, dl, da, dr);
    } else {
        hipLaunchKernelGGL(orbit_los_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, dt_, dp_, dv_, (int)nsv,
                           dx, n, threshold, maxiter, dl, da, dr);
    }
    return S.finish();
}

// ---- azimuth-time-grid combination in one pass (aztime_kernels.h) ------------------------------------------------------------------
// two epoch arrays of one call must lie on one grid (the dtype may differ: pointwise cubes are f32, total cubes f64)
static int same_grid_check(rdr_ctx* c, const char* who, const rdr_cube* a, const rdr_cube* b) {
    const LccParams &p = a->proj, &r = b->proj;
    if (a->ny != b->ny || a->nx != b->nx || a->nz != b->nz || a->ys != b->ys || a->xs != b->xs || a->zs != b->zs || p.kind != r.kind ||
        std::memcmp(&p.n, &r.n, sizeof(double)) || std::memcmp(&p.aF, &r.aF, sizeof(double)) || std::memcmp(&p.rho0, &r.rho0, sizeof(double)) ||
        std::memcmp(&p.lam0, &r.lam0, sizeof(double)) || std::memcmp(&p.x0, &r.x0, sizeof(double)) || std::memcmp(&p.y0, &r.y0, sizeof(double)) ||
        std::memcmp(&p.e, &r.e, sizeof(double)))
        return fail(c, RDR_ERR_INVALID, std::string(who) + ": the pointwise and the total cubes are not on the same grid / projection");
    return RDR_OK;
}

int rdr_cube_blend_azimuth_time(rdr_ctx* c, const rdr_cube* const* pointwise, const rdr_cube* const* total, int32_t nd, const double* lat2d,
                                const double* lon2d, int loc, const double* sv_t, const double* sv_pos, const double* sv_vel, int64_t nsv,
                                const double* dates_s, double window_s, double reg, int64_t offset_us, rdr_cube** out_pointwise,
                                rdr_cube** out_total, double* time_grid, int32_t* flags) {
    static const char* who = "rdr_cube_blend_azimuth_time";
    const std::string w(who);
    if (!c) return fail(nullptr, RDR_ERR_INVALID, w + ": NULL context");
    if (!pointwise && !total) return fail(c, RDR_ERR_INVALID, w + ": pointwise and total are both NULL");
    if (nd < 1 || nd > 8) return fail(c, RDR_ERR_INVALID, w + ": nd must be 1..8");
    if (pointwise && !out_pointwise) return fail(c, RDR_ERR_INVALID, w + ": out_pointwise is NULL");
    if (total && !out_total) return fail(c, RDR_ERR_INVALID, w + ": out_total is NULL");
    if (!lat2d || !lon2d) return fail(c, RDR_ERR_INVALID, w + ": lat2d / lon2d is NULL");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, w + ": loc must be RDR_HOST or RDR_DEVICE");
    if (!sv_t || !sv_pos || !sv_vel) return fail(c, RDR_ERR_INVALID, w + ": sv_t / sv_pos / sv_vel is NULL");
    if (nsv < 4) return fail(c, RDR_ERR_INVALID, "state_to_los: At least 4 state vectors are required for orbit interpolation");
    if (nsv > ORBIT_LDS_MAX_SV) return fail(c, RDR_ERR_INVALID, w + ": nsv exceeds the " + std::to_string(ORBIT_LDS_MAX_SV) + " state vectors the LDS tables hold");
    for (int64_t i = 1; i < nsv; ++i) if (!(sv_t[i] > sv_t[i - 1])) return fail(c, RDR_ERR_INVALID, w + ": state-vector times must be strictly increasing");
    if (!dates_s) return fail(c, RDR_ERR_INVALID, w + ": dates_s is NULL");
    if (!flags) return fail(c, RDR_ERR_INVALID, w + ": flags is NULL");
    if (!(reg >= 0.0)) return fail(c, RDR_ERR_INVALID, w + ": reg must be >= 0");
    AzTimeArgs A; std::memset(&A, 0, sizeof(A));
    A.D.nd = nd; A.D.reg = reg;
    for (int i = 0; i < nd; ++i) {
        if (!(dates_s[i] == dates_s[i])) return fail(c, RDR_ERR_INVALID, w + ": dates_s holds a NaN");
        A.D.date[i] = dates_s[i];
        for (int j = 0; j < i; ++j) if (dates_s[j] == dates_s[i]) return fail(c, RDR_ERR_INVALID, "Dates provided must be unique");
    }
    if (window_s < 0) {                                  // s1_azimuth_timing.py:375-376: infer the model time step
        if (nd < 2) return fail(c, RDR_ERR_INVALID, w + ": the temporal window cannot be inferred from one date");
        window_s = std::fabs(dates_s[1] - dates_s[0]);
        for (int i = 2; i < nd; ++i) window_s = std::min(window_s, std::fabs(dates_s[i] - dates_s[0]));
    }
    if (!(window_s == window_s)) return fail(c, RDR_ERR_INVALID, w + ": window_s is NaN");
    A.D.window = window_s;
    int rc;
    if (pointwise) { rc = epochs_check(c, who, pointwise, nd); if (rc) return rc; }
    if (total) { rc = epochs_check(c, who, total, nd); if (rc) return rc; }
    if (pointwise && total) { rc = same_grid_check(c, who, pointwise[0], total[0]); if (rc) return rc; }
    const rdr_cube* a = pointwise ? pointwise[0] : total[0];
    for (int i = 0; i < nd; ++i) {
        if (pointwise) { note_use(c, pointwise[i]); A.P.v[i] = pointwise[i]->d_vals; }
        if (total) { note_use(c, total[i]); A.T.v[i] = total[i]->d_vals; }
    }
    A.P.nd = A.T.nd = nd;
    HIPCHECK(c, hipSetDevice(c->device));
    const int64_t nvox = a->ny * a->nx * a->nz;
    const size_t n2 = (size_t)a->ny * a->nx;
    // the (small) state-vector table always comes from the host, as in rdr_orbit_look_vectors; lat2d / lon2d / the time grid follow `loc`
    void* dtab;
    rc = ensure(c, SLOT_AUX, (size_t)nsv * 7 * 8, &dtab); if (rc) return rc;
    double* dt_ = (double*)dtab; double* dp_ = dt_ + nsv; double* dv_ = dp_ + 3 * nsv;
    const HostPart parts[3] = {{sv_t, (size_t)nsv * 8}, {sv_pos, (size_t)nsv * 24}, {sv_vel, (size_t)nsv * 24}};
    rc = upload_parts(c, dtab, parts, 3); if (rc) return rc;
    const void *dla, *dlo; void* dg = nullptr;
    rc = stage_in(c, SLOT_IN0, lat2d, n2 * 8, loc, &dla); if (rc) return rc;
    rc = stage_in(c, SLOT_IN1, lon2d, n2 * 8, loc, &dlo); if (rc) return rc;
    if (time_grid) { rc = stage_out(c, SLOT_OUT0, time_grid, (size_t)nvox * 8, loc, &dg); if (rc) return rc; }
    rdr_cube* q[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
        if (!(k == 0 ? pointwise : total)) continue;
        q[k] = new rdr_cube();
        q[k]->ctx = c; q[k]->ny = a->ny; q[k]->nx = a->nx; q[k]->nz = a->nz; q[k]->dtype = RDR_F64;
        q[k]->ys = a->ys; q[k]->xs = a->xs; q[k]->zs = a->zs; q[k]->proj = a->proj;
        rc = cube_alloc(c, q[k]);
        if (rc) { for (rdr_cube* x : q) if (x) rdr_cube_destroy(x); return rc; }
    }
    auto drop = [&]() { if (q[0]) rdr_cube_destroy(q[0]); if (q[1]) rdr_cube_destroy(q[1]); };
    A.st = dt_; A.sp = dp_; A.sv = dv_; A.nsv = (int)nsv;
    A.lat2d = (const double*)dla; A.lon2d = (const double*)dlo; A.zs = root(a)->d_axes + a->ny + a->nx;
    A.ny = a->ny; A.nx = a->nx; A.nz = a->nz;
    A.offset_us = (long long)offset_us;
    A.out_p = q[0] ? (double2*)q[0]->d_vals : nullptr; A.out_t = q[1] ? (double2*)q[1]->d_vals : nullptr;
    A.tgrid = (double*)dg; A.flags = c->d_flags;
    hipError_t e = hipMemsetAsync(c->d_flags, 0, sizeof(int), c->stream);
    if (e == hipSuccess) {
        KTimer t(c, 3);
        const int g = grid_for(nvox, 256, c->num_cus * 8);
        const size_t smem = orbit_tables_bytes(nsv);
        const bool pf = !pointwise || pointwise[0]->dtype == RDR_F32, tf = !total || total[0]->dtype == RDR_F32;
        if (pf && tf) hipLaunchKernelGGL((aztime_blend_kernel<float2, float2>), dim3(g), dim3(256), smem, c->stream, A);
        else if (pf) hipLaunchKernelGGL((aztime_blend_kernel<float2, double2>), dim3(g), dim3(256), smem, c->stream, A);
        else if (tf) hipLaunchKernelGGL((aztime_blend_kernel<double2, float2>), dim3(g), dim3(256), smem, c->stream, A);
        else hipLaunchKernelGGL((aztime_blend_kernel<double2, double2>), dim3(g), dim3(256), smem, c->stream, A);
        e = hipGetLastError();
    }
    int f = 0;
    if (e == hipSuccess && time_grid && loc == RDR_HOST) e = hipMemcpyAsync(time_grid, dg, (size_t)nvox * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&f, c->d_flags, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); drop(); return fail(c, e == hipErrorOutOfMemory ? RDR_ERR_OOM : RDR_ERR_HIP, w + ": " + hipGetErrorString(e)); }
    *flags = (f & 1) | ((f & 4) ? 0 : 2);
    if (out_pointwise) *out_pointwise = q[0];
    if (out_total) *out_total = q[1];
    return RDR_OK;
}

// ---- native extensions ------------------------------------------------------------------------------------
int rdr_interp_nd(rdr_ctx* c, int32_t ndim, const double* const* axes, const int64_t* axis_len, const double* values,
                  const double* q, int64_t n, int has_fill, double fill, double* out, int loc) {
    if (!c || !axes || !axis_len || !values || (n > 0 && (!q || !out))) return fail(c, RDR_ERR_INVALID, "rdr_interp_nd: NULL argument");
    if (ndim < 1 || ndim > 8) return fail(c, RDR_ERR_INVALID, "rdr_interp_nd: 1 <= ndim <= 8 supported on device");
    if (n < 0) return fail(c, RDR_ERR_INVALID, "rdr_interp_nd: negative count");
    if (n == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    NdParams P; std::memset(&P, 0, sizeof(P));
    P.ndim = ndim;
    int64_t tot_axes = 0, nvals = 1;
    for (int d = 0; d < ndim; ++d) {
        if (axis_len[d] < 2) return fail(c, RDR_ERR_INVALID, "rdr_interp_nd: every axis needs >= 2 points");
        P.len[d] = axis_len[d]; P.off[d] = tot_axes; tot_axes += axis_len[d]; nvals *= axis_len[d];
    }
    int64_t s = 1;
    for (int d = ndim - 1; d >= 0; --d) { P.stride[d] = s; s *= axis_len[d]; }
    // axes are always host-side tuples of small 1-D arrays in the reference API; accept device too
    Staged S(c, loc);
    double* dax;
    if (loc == RDR_HOST) {
        HostPart tab[8];
        for (int d = 0; d < ndim; ++d) tab[d] = HostPart{axes[d], (size_t)axis_len[d] * 8};
        dax = S.table<double>(SLOT_AUX, tab, ndim);
    } else {
        dax = S.scratch<double>(SLOT_AUX, (size_t)tot_axes * 8);
        if (S.rc) return S.rc;
        for (int d = 0; d < ndim; ++d)
            HIPCHECK(c, hipMemcpyAsync(dax + P.off[d], axes[d], (size_t)axis_len[d] * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    const double *dv = S.in(values, (size_t)nvals * 8), *dq = S.in(q, (size_t)n * ndim * 8);
    double* dout = S.out(out, (size_t)n * 8);
    if (S.rc) return S.rc;
    {
        KTimer t(c, 2);
        hipLaunchKernelGGL(interp_nd_kernel, dim3(grid_for(n, 256, c->num_cus * 8)), dim3(256), 0, c->stream, P, (const double*)dax, dv, dq, n, has_fill, fill,
                           dout);
    }
    return S.finish();
}

int rdr_interp_along_axis(rdr_ctx* c, const double* points, const double* values, int64_t ncol, int64_t m, const double* q,
                          int64_t mq, int has_fill, double fill, double* out, int loc) {
    if (!c || !points || !values || !q || !out) return fail(c, RDR_ERR_INVALID, "rdr_interp_along_axis: NULL argument");
    if (m < 2) return fail(c, RDR_ERR_INVALID, "rdr_interp_along_axis: axis needs >= 2 points");
    if (ncol < 0 || mq < 0) return fail(c, RDR_ERR_INVALID, "rdr_interp_along_axis: negative count");
    if (ncol * mq == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *dp = S.in(points, (size_t)ncol * m * 8), *dv = S.in(values, (size_t)ncol * m * 8), *dq = S.in(q, (size_t)ncol * mq * 8);
    double* dout = S.out(out, (size_t)ncol * mq * 8);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(along_axis_kernel, dim3(grid_for(ncol * mq, 256, c->num_cus * 8)), dim3(256), 0, c->stream, dp, dv, ncol, m, dq, mq, has_fill, fill, dout);
    return S.finish();
}

int64_t rdr_make_points_count(double max_len, double step) {
    // makePoints.pyx:30-33: Npts = int(max_len//step) (+1 if max_len % step != 0); python float // and %
    if (!(step > 0) || !(max_len >= 0)) return -1;
    double mod = std::fmod(max_len, step);
    double div = (max_len - mod) / step;
    double fl = std::floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return (int64_t)fl + (mod != 0.0 ? 1 : 0);
}

int rdr_make_points(rdr_ctx* c, double max_len, const double* sp, const double* slv, int64_t nrays, double step, double* out, int loc) {
    if (!c || !sp || !slv || !out) return fail(c, RDR_ERR_INVALID, "rdr_make_points: NULL argument");
    const int64_t npts = rdr_make_points_count(max_len, step);
    if (npts < 0) return fail(c, RDR_ERR_INVALID, "rdr_make_points: need max_len >= 0 and step > 0");
    if (nrays < 0) return fail(c, RDR_ERR_INVALID, "rdr_make_points: negative count");
    if (nrays * npts == 0) return RDR_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *ds = S.in(sp, (size_t)nrays * 24), *dl = S.in(slv, (size_t)nrays * 24);
    double* dout = S.out(out, (size_t)nrays * 3 * npts * 8);
    if (S.rc) return S.rc;
    {
        KTimer t(c, 3);
        hipLaunchKernelGGL(make_points_kernel, dim3(grid_for(nrays * 3 * npts, 256, c->num_cus * 8)), dim3(256), 0, c->stream, ds, dl, nrays, npts, step, dout);
    }
    return S.finish();
}


// ---- georeferenced rasters (raster_kernels.h): DEM sampling and lat / lon raster bounds ---------------------------------------------
static int raster_elem_size(int dtype) { return dtype == RDR_I16 ? 2 : dtype == RDR_F32 ? 4 : dtype == RDR_F64 ? 8 : 0; }

template <typename T>
static void launch_raster_sample(rdr_ctx* c, int method, const void* raster, const RasterGeo& g, const double* x, const double* y, int64_t n,
                                 int has_nodata, double nodata, double* out) {
    const dim3 G(grid_for(n, 256, c->num_cus * 8)), B(256);
    KTimer t(c, 2);
    if (method == RASTER_NEAREST)
        hipLaunchKernelGGL((raster_sample_kernel<T, RASTER_NEAREST>), G, B, 0, c->stream, (const T*)raster, g, x, y, n, has_nodata, nodata, out);
    else
        hipLaunchKernelGGL((raster_sample_kernel<T, RASTER_LINEAR>), G, B, 0, c->stream, (const T*)raster, g, x, y, n, has_nodata, nodata, out);
}

int rdr_raster_sample(rdr_ctx* c, const void* raster, int dtype, int64_t height, int64_t width, const double* gt6, const double* x,
                      const double* y, int64_t n, int method, int has_nodata, double nodata, double* out, int loc) {
    if (!c || !raster || !gt6 || !x || !y || !out) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: NULL argument");
    const int esize = raster_elem_size(dtype);
    if (!esize) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: dtype must be RDR_I16, RDR_F32 or RDR_F64");
    if (height <= 0 || width <= 0 || height > ((int64_t)1 << 31) || width > ((int64_t)1 << 31) || height * width > ((int64_t)1 << 40))
        return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: the raster needs positive sizes (at most 2^40 pixels)");
    if (n <= 0) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: the point count must be positive");
    if (method != RASTER_NEAREST && method != RASTER_LINEAR) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: method must be 0 (nearest) or 1 (linear)");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: loc must be RDR_HOST or RDR_DEVICE");
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(gt6[i])) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: the geotransform is not finite");
    if (gt6[1] == 0.0 || gt6[5] == 0.0) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: the geotransform has a zero pixel size");
    if (gt6[2] != 0.0 || gt6[4] != 0.0) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: rotated geotransforms are not supported (north-up rasters only)");
    if (method == RASTER_LINEAR && (height < 2 || width < 2)) return fail(c, RDR_ERR_INVALID, "rdr_raster_sample: linear sampling needs two pixels per axis");
    HIPCHECK(c, hipSetDevice(c->device));
    const RasterGeo g{height, width, gt6[0], gt6[1], gt6[3], gt6[5]};
    Staged S(c, loc);
    const void* dr = S.in(raster, (size_t)(height * width) * esize);
    const double *dx = S.in(x, (size_t)n * 8), *dy = S.in(y, (size_t)n * 8);
    double* dout = S.out(out, (size_t)n * 8);
    if (S.rc) return S.rc;
    if (dtype == RDR_I16) launch_raster_sample<int16_t>(c, method, dr, g, dx, dy, n, has_nodata != 0, nodata, dout);
    else if (dtype == RDR_F32) launch_raster_sample<float>(c, method, dr, g, dx, dy, n, has_nodata != 0, nodata, dout);
    else launch_raster_sample<double>(c, method, dr, g, dx, dy, n, has_nodata != 0, nodata, dout);
    return S.finish();
}

template <typename T>
static void launch_raster_bounds(rdr_ctx* c, int grid, const void* a, const void* b, int64_t n, int has_nodata, double nodata, double* partial) {
    hipLaunchKernelGGL(raster_bounds_kernel<T>, dim3(grid), dim3(256), 0, c->stream, (const T*)a, (const T*)b, n, has_nodata, nodata, partial);
}

int rdr_raster_bounds(rdr_ctx* c, const void* a, const void* b, int dtype, int64_t n, int has_nodata, double nodata, double* out6, int loc) {
    if (!c || !a || !out6) return fail(c, RDR_ERR_INVALID, "rdr_raster_bounds: NULL argument");
    const int esize = raster_elem_size(dtype);
    if (!esize) return fail(c, RDR_ERR_INVALID, "rdr_raster_bounds: dtype must be RDR_I16, RDR_F32 or RDR_F64");
    if (n <= 0 || n > ((int64_t)1 << 40)) return fail(c, RDR_ERR_INVALID, "rdr_raster_bounds: the element count must be positive (at most 2^40)");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, "rdr_raster_bounds: loc must be RDR_HOST or RDR_DEVICE");
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const void *da = S.in(a, (size_t)n * esize), *db = S.in(b, (size_t)n * esize);       // (b is optional)
    // one lane takes 16 bytes per step; the grid is sized from the compute-unit count and strides over the rest
    const int grid = grid_for((n * esize + 15) / 16, 256, c->num_cus * 8);
    double* dpart = S.scratch<double>(SLOT_AUX, (size_t)grid * 6 * 8);
    double* dout = S.out(out6, 6 * 8);
    if (S.rc) return S.rc;
    {
        KTimer t(c, 3);
        if (dtype == RDR_I16) launch_raster_bounds<int16_t>(c, grid, da, db, n, has_nodata != 0, nodata, dpart);
        else if (dtype == RDR_F32) launch_raster_bounds<float>(c, grid, da, db, n, has_nodata != 0, nodata, dpart);
        else launch_raster_bounds<double>(c, grid, da, db, n, has_nodata != 0, nodata, dpart);
        hipLaunchKernelGGL(raster_bounds_final_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)dpart, grid, dout);
    }
    return S.finish();
}


// ---- GeoTIFF segments (tiff_kernels.h): LZW decoding and raster assembly -----------------------------------------------------------
// The shared check of a segment table's entry: `bytes` bytes at `off` lie inside a source buffer of `src_bytes` (decoders and the encoder)
static int segment_in_source(rdr_ctx* c, const std::string& w, int64_t i, int64_t off, int64_t bytes, int64_t src_bytes) {
    if (off < 0 || bytes < 0 || off > src_bytes || bytes > src_bytes - off)
        return fail(c, RDR_ERR_INVALID, w + ": segment " + std::to_string(i) + " does not lie inside the source buffer");
    return RDR_OK;
}

// What the segment decoders refuse before the device is touched.
static int decode_segments_check(rdr_ctx* c, const char* who, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                                 const int64_t* seg_out_bytes, const void* out, int64_t out_stride, const int32_t* status, int loc) {
    const std::string w(who);
    if (!c || !src || !seg_offset || !seg_bytes || !seg_out_bytes || !out || !status) return fail(c, RDR_ERR_INVALID, w + ": NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, w + ": loc must be RDR_HOST or RDR_DEVICE");
    if (src_bytes <= 0 || nseg <= 0 || nseg > (1 << 24)) return fail(c, RDR_ERR_INVALID, w + ": need a non-empty buffer and 1 .. 2^24 segments");
    if (out_stride <= 0 || out_stride > ((int64_t)1 << 31) - 256 || nseg * out_stride > ((int64_t)1 << 40))
        return fail(c, RDR_ERR_INVALID, w + ": out_stride must be positive and below 2 GiB (at most 2^40 bytes in all)");
    for (int64_t i = 0; i < nseg; ++i) {
        const int rc = segment_in_source(c, w, i, seg_offset[i], seg_bytes[i], src_bytes); if (rc) return rc;
        if (seg_bytes[i] >= ((int64_t)1 << 31) - 256) return fail(c, RDR_ERR_INVALID, w + ": segment " + std::to_string(i) + " is 2 GiB or longer");
        if (seg_out_bytes[i] < 0 || seg_out_bytes[i] > out_stride)
            return fail(c, RDR_ERR_INVALID, w + ": segment " + std::to_string(i) + " would write beyond its slot of out_stride bytes");
    }
    return RDR_OK;
}

// One driver for the two segment decoders (LZW strips / tiles, zlib streams): segment i of `src` is decoded into out + i * out_stride, one
// wave per segment.  `launch(grid, src, tab, out, status, produced)` starts the kernel; tab = offsets | bytes | out bytes, nseg each.
template <typename Launch>
static int decode_segments(rdr_ctx* c, const char* who, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                           const int64_t* seg_out_bytes, void* out, int64_t out_stride, int32_t* status, int64_t* produced, int loc, int per_cu,
                           Launch&& launch) {
    { const int rc = decode_segments_check(c, who, src, src_bytes, seg_offset, seg_bytes, nseg, seg_out_bytes, out, out_stride, status, loc); if (rc) return rc; }
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const uint8_t* dsrc = S.in(static_cast<const uint8_t*>(src), (size_t)src_bytes);
    const HostPart tabs[3] = {{seg_offset, (size_t)nseg * 8}, {seg_bytes, (size_t)nseg * 8}, {seg_out_bytes, (size_t)nseg * 8}};
    const int64_t* tab = S.table<int64_t>(SLOT_IN1, tabs, 3);   // the three tables are host arrays whatever `loc` says
    uint8_t* dout = S.out(static_cast<uint8_t*>(out), (size_t)(nseg * out_stride));
    int32_t* dstat = S.out(status, (size_t)nseg * 4);
    int64_t* dprod = S.out(produced, (size_t)nseg * 8);         // (optional)
    if (S.rc) return S.rc;
    // bytes of a slot the stream does not reach keep their value: a host `out` goes up first
    if (loc == RDR_HOST) { const int rc = upload(c, dout, out, (size_t)(nseg * out_stride)); if (rc) return rc; }
    // one wave per segment; a compute unit holds `per_cu` of the kernel's workgroups (by their LDS), the grid strides over the rest
    launch((int)std::min<int64_t>(nseg, (int64_t)c->num_cus * per_cu), dsrc, tab, dout, dstat, dprod);
    return S.finish();
}

int rdr_tiff_lzw_decode(rdr_ctx* c, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                        const int64_t* seg_out_bytes, void* out, int64_t out_stride, int32_t* status, int loc) {
    // five of the 29 KB workgroups per compute unit
    return decode_segments(c, "rdr_tiff_lzw_decode", src, src_bytes, seg_offset, seg_bytes, nseg, seg_out_bytes, out, out_stride, status, nullptr, loc, 5,
                           [&](int grid, const uint8_t* dsrc, const int64_t* tab, uint8_t* dout, int32_t* dstat, int64_t*) {
        hipLaunchKernelGGL(tiff_lzw_kernel, dim3(grid), dim3(64), 0, c->stream, dsrc, src_bytes, tab, tab + nseg, tab + 2 * nseg, (int)nseg, dout, out_stride, dstat);
    });
}

int rdr_tiff_assemble(rdr_ctx* c, const void* segs, int64_t seg_stride, int64_t height, int64_t width, int64_t tile_h, int64_t tile_w, int predictor,
                      int swap, int sample_bytes, int planar, int bands, int band, void* out, int loc) {
    if (!c || !segs || !out) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: loc must be RDR_HOST or RDR_DEVICE");
    if (sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4 && sample_bytes != 8) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: samples of 1, 2, 4 or 8 bytes");
    if (height <= 0 || width <= 0 || tile_h <= 0 || tile_w <= 0 || height > ((int64_t)1 << 31) || width > ((int64_t)1 << 31) || tile_h > ((int64_t)1 << 31) ||
        tile_w > ((int64_t)1 << 31))
        return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: raster and segment sizes must be positive (below 2^31)");
    if (predictor != 1 && predictor != 2) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: predictor must be 1 (none) or 2 (horizontal differencing)");
    if (planar != 1 && planar != 2) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: planar must be 1 (chunky) or 2 (planar)");
    if (bands <= 0 || bands > 65535 || band < -1 || band >= bands) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: 1 .. 65535 bands; band is -1 (all) or 0 .. bands - 1");
    const int64_t tiles_x = (width + tile_w - 1) / tile_w, tiles_y = (height + tile_h - 1) / tile_h;
    const int64_t spp = planar == 2 ? 1 : bands, nplanes = planar == 2 ? bands : 1;
    // (tile_h * sample_bytes < 2^35 and tile_w * spp < 2^47: neither product overflows; their product is formed only once it is known to fit)
    if (tile_w * spp > ((int64_t)1 << 40) / (tile_h * sample_bytes) || seg_stride < tile_h * tile_w * spp * sample_bytes || seg_stride % 8 != 0)
        return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: seg_stride must hold one decoded segment and be a multiple of 8");
    const int64_t nsegs = tiles_x * tiles_y * nplanes, nout = band < 0 ? bands : 1;
    if (nsegs > ((int64_t)1 << 42) / seg_stride || nout * height * width > ((int64_t)1 << 40)) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: the raster is beyond 2^40 samples");
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t out_bytes = (size_t)(nout * height * width) * sample_bytes;
    Staged S(c, loc);
    const void* dsegs = S.in(segs, (size_t)(nsegs * seg_stride));
    void* dout = S.out(out, out_bytes);
    if (S.rc) return S.rc;
    if ((reinterpret_cast<uintptr_t>(dsegs) | reinterpret_cast<uintptr_t>(dout)) % sample_bytes != 0) return fail(c, RDR_ERR_INVALID, "rdr_tiff_assemble: buffers must be aligned to the sample size");
    if (predictor == 1 && !swap && tiles_x == 1 && tiles_y == 1 && tile_w == width && (bands == 1 || planar == 2)) {
        // one strip (per plane) that is the raster already: a copy per output band
        for (int64_t b = 0; b < nout; ++b)
            HIPCHECK(c, hipMemcpyAsync((char*)dout + b * (out_bytes / nout), (const char*)dsegs + (band < 0 ? b : band) * seg_stride, out_bytes / nout,
                                       hipMemcpyDeviceToDevice, c->stream));
    } else {
        const TiffLayout L{height, width, tile_h, tile_w, tiles_x, tiles_y, seg_stride, bands, planar, band, predictor, swap != 0};
        const int64_t nrows = (planar == 2 && band < 0 ? bands : 1) * tiles_x * tiles_y * tile_h;
        const dim3 G(grid_for(nrows, 4, c->num_cus * 16)), B(256);
        if (sample_bytes == 1) hipLaunchKernelGGL(tiff_assemble_kernel<uint8_t>, G, B, 0, c->stream, (const uint8_t*)dsegs, L, (uint8_t*)dout);
        else if (sample_bytes == 2) hipLaunchKernelGGL(tiff_assemble_kernel<uint16_t>, G, B, 0, c->stream, (const uint8_t*)dsegs, L, (uint16_t*)dout);
        else if (sample_bytes == 4) hipLaunchKernelGGL(tiff_assemble_kernel<uint32_t>, G, B, 0, c->stream, (const uint8_t*)dsegs, L, (uint32_t*)dout);
        else hipLaunchKernelGGL(tiff_assemble_kernel<uint64_t>, G, B, 0, c->stream, (const uint8_t*)dsegs, L, (uint64_t*)dout);
    }
    return S.finish();
}


// ---- zlib streams and HDF5 chunks (deflate_kernels.h) ------------------------------------------------------------------------------
int64_t rdr_deflate_bound(int64_t n) {
    if (n < 0) n = 0;
    return n + 5 * ((n + DEFL_SUB - 1) / DEFL_SUB) + 6;        // a stored block per sub-block, 78 01 and the Adler-32
}

int rdr_deflate_encode_tables(rdr_ctx* c, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg, int tables,
                              void* out, int64_t out_capacity, int64_t* out_offset, int64_t* block_counts, int loc) {
    if (!c || !src || !seg_offset || !seg_bytes || !out || !out_offset) return fail(c, RDR_ERR_INVALID, "rdr_deflate_encode: NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, "rdr_deflate_encode: loc must be RDR_HOST or RDR_DEVICE");
    if (tables != RDR_DEFL_FIXED && tables != RDR_DEFL_DYNAMIC) return fail(c, RDR_ERR_INVALID, "rdr_deflate_encode: tables must be RDR_DEFL_FIXED or RDR_DEFL_DYNAMIC");
    if (src_bytes <= 0 || src_bytes > ((int64_t)1 << 40) || nseg <= 0 || nseg > (1 << 24))
        return fail(c, RDR_ERR_INVALID, "rdr_deflate_encode: need a non-empty buffer (at most 2^40 bytes) and 1 .. 2^24 segments");
    int64_t need = 0, nsub = 0;
    for (int64_t i = 0; i < nseg; ++i) {
        if (seg_bytes[i] <= 0) return fail(c, RDR_ERR_INVALID, "rdr_deflate_encode: segment " + std::to_string(i) + " is empty");
        const int rc = segment_in_source(c, "rdr_deflate_encode", i, seg_offset[i], seg_bytes[i], src_bytes); if (rc) return rc;
        need += rdr_deflate_bound(seg_bytes[i]);
        nsub += (seg_bytes[i] + DEFL_SUB - 1) / DEFL_SUB;
        if (need > ((int64_t)1 << 41)) return fail(c, RDR_ERR_INVALID, "rdr_deflate_encode: the segments hold more than 2^40 bytes");
    }
    if (out_capacity < need)
        return fail(c, RDR_ERR_INVALID, "rdr_deflate_encode: out_capacity " + std::to_string(out_capacity) + " is below the sum of the bounds, " + std::to_string(need));
    HIPCHECK(c, hipSetDevice(c->device));
    std::vector<DeflSub> subs((size_t)nsub);
    {
        int64_t k = 0;
        for (int64_t i = 0; i < nseg; ++i)
            for (int64_t o = 0; o < seg_bytes[i]; o += DEFL_SUB, ++k) {
                const int64_t m = std::min<int64_t>(DEFL_SUB, seg_bytes[i] - o);
                subs[(size_t)k] = DeflSub{seg_offset[i] + o, 0, (int32_t)m, (o == 0 ? 1 : 0) | (o + m == seg_bytes[i] ? 2 : 0), 0u, 0};
            }
    }
    Staged S(c, loc);
    const uint8_t* dsrc = S.in(static_cast<const uint8_t*>(src), (size_t)src_bytes);
    const HostPart sub_table{subs.data(), (size_t)nsub * sizeof(DeflSub)};
    const DeflSub* dsubs = S.table<DeflSub>(SLOT_IN1, &sub_table, 1);
    uint8_t* dslots = S.scratch<uint8_t>(SLOT_DEFL, (size_t)nsub * DEFL_SLOT);
    DeflResult* dres = S.scratch<DeflResult>(SLOT_OUT1, (size_t)nsub * sizeof(DeflResult));
    // one wave per sub-block; a compute unit holds three of these 53 KB workgroups, the grid strides over the rest
    const unsigned grid = (unsigned)std::min<int64_t>(nsub, (int64_t)c->num_cus * 3);
    uint32_t* dtok = tables == RDR_DEFL_DYNAMIC ? S.scratch<uint32_t>(SLOT_DEFL_TOK, (size_t)grid * DEFL_SUB * sizeof(uint32_t)) : nullptr;
    if (S.rc) return S.rc;
    if (tables == RDR_DEFL_DYNAMIC)
        hipLaunchKernelGGL(deflate_encode_dyn_kernel, dim3(grid), dim3(64), 0, c->stream, dsrc, dsubs, nsub, dslots, dres, dtok);
    else
        hipLaunchKernelGGL(deflate_encode_kernel, dim3(grid), dim3(64), 0, c->stream, dsrc, dsubs, nsub, dslots, dres);
    HIPCHECK(c, hipGetLastError());
    std::vector<DeflResult> res((size_t)nsub);
    HIPCHECK(c, hipMemcpyAsync(res.data(), dres, (size_t)nsub * sizeof(DeflResult), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    // sizes -> offsets; the sub-blocks' Adler sums -> the streams' (A' = A + s1, B' = B + n A + s2: adler32_combine's rule)
    int64_t pos = 0, seg = 0;
    uint32_t A = 1u, B = 0u;
    int64_t kinds[3] = {0, 0, 0};                                  // stored, fixed, dynamic sub-blocks
    for (int64_t k = 0; k < nsub; ++k) {
        DeflSub& d = subs[(size_t)k];
        const DeflResult& r = res[(size_t)k];
        if (r.fixed_bytes < 0 || r.fixed_bytes >= d.n + 5 || r.s1 >= 65521u || r.s2 >= 65521u) return fail(c, RDR_ERR_HIP, "rdr_deflate_encode: the encoder returned an impossible size");
        if (d.flags & 1) { out_offset[seg] = pos; A = 1u; B = 0u; }
        d.dst_off = pos;
        d.fixed_bytes = r.fixed_bytes;
        ++kinds[r.fixed_bytes > 0 ? (r.pad == 2 ? 2 : 1) : 0];
        B = (uint32_t)((B + (uint64_t)d.n % 65521u * A + r.s2) % 65521u);
        A = (A + r.s1) % 65521u;
        pos += ((d.flags & 1) ? 2 : 0) + (r.fixed_bytes > 0 ? r.fixed_bytes : d.n + 5) + ((d.flags & 2) ? 4 : 0);
        if (d.flags & 2) { d.adler = (B << 16) | A; ++seg; }
    }
    out_offset[nseg] = pos;
    if (pos > out_capacity) return fail(c, RDR_ERR_HIP, "rdr_deflate_encode: the streams exceed their bound");       // (cannot happen: every sub-block is at most n + 5)
    S.table<DeflSub>(SLOT_IN1, &sub_table, 1);                       // (the same table again, with the offsets, sizes and checksums filled in)
    uint8_t* dout = S.out(static_cast<uint8_t*>(out), (size_t)pos);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(deflate_pack_kernel, dim3((unsigned)std::min<int64_t>(nsub, (int64_t)c->num_cus * 8)), dim3(256), 0, c->stream, dsrc, dsubs, nsub,
                       (const uint8_t*)dslots, dout, pos);
    const int rc = S.finish(true);                                   // (always waits, as the size pass above did)
    if (rc) return rc;
    if (block_counts) { block_counts[0] = kinds[0]; block_counts[1] = kinds[1]; block_counts[2] = kinds[2]; }
    return RDR_OK;
}

int rdr_deflate_encode(rdr_ctx* c, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg, void* out,
                       int64_t out_capacity, int64_t* out_offset, int loc) {
    return rdr_deflate_encode_tables(c, src, src_bytes, seg_offset, seg_bytes, nseg, RDR_DEFL_FIXED, out, out_capacity, out_offset, nullptr, loc);
}

int rdr_tiff_predict(rdr_ctx* c, const void* in, int sample_bytes, int64_t height, int64_t width, void* out, int loc) {
    if (!c || !in || !out) return fail(c, RDR_ERR_INVALID, "rdr_tiff_predict: NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, "rdr_tiff_predict: loc must be RDR_HOST or RDR_DEVICE");
    if (sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4 && sample_bytes != 8) return fail(c, RDR_ERR_INVALID, "rdr_tiff_predict: samples of 1, 2, 4 or 8 bytes");
    if (height <= 0 || width <= 0 || height > ((int64_t)1 << 31) || width > ((int64_t)1 << 31) || height * width > ((int64_t)1 << 36))
        return fail(c, RDR_ERR_INVALID, "rdr_tiff_predict: raster sizes must be positive, at most 2^36 samples");
    if (in == out) return fail(c, RDR_ERR_INVALID, "rdr_tiff_predict: in and out must be different buffers");
    HIPCHECK(c, hipSetDevice(c->device));
    const int64_t n = height * width;
    Staged S(c, loc);
    const void* din = S.in(in, (size_t)n * sample_bytes);
    void* dout = S.out(out, (size_t)n * sample_bytes);
    if (S.rc) return S.rc;
    if ((reinterpret_cast<uintptr_t>(din) | reinterpret_cast<uintptr_t>(dout)) % sample_bytes != 0) return fail(c, RDR_ERR_INVALID, "rdr_tiff_predict: buffers must be aligned to the sample size");
    const dim3 G(grid_for(n, 256, c->num_cus * 16)), Bk(256);
    if (sample_bytes == 1) hipLaunchKernelGGL(tiff_predict_kernel<uint8_t>, G, Bk, 0, c->stream, (const uint8_t*)din, n, width, (uint8_t*)dout);
    else if (sample_bytes == 2) hipLaunchKernelGGL(tiff_predict_kernel<uint16_t>, G, Bk, 0, c->stream, (const uint16_t*)din, n, width, (uint16_t*)dout);
    else if (sample_bytes == 4) hipLaunchKernelGGL(tiff_predict_kernel<uint32_t>, G, Bk, 0, c->stream, (const uint32_t*)din, n, width, (uint32_t*)dout);
    else hipLaunchKernelGGL(tiff_predict_kernel<uint64_t>, G, Bk, 0, c->stream, (const uint64_t*)din, n, width, (uint64_t*)dout);
    return S.finish();
}

// The chunk grid of an array of `ndim` axes (rdr_h5_chunks and its inverse): shape and chunk padded to four axes with ones in front, every
// size and product checked (at most 2^36 elements, padding included).  *array_elems: elements of the array; *nchunks: chunks of the grid.
// G.total_elems is left to the caller - all chunks one way, the present ones the other.
static int h5_chunk_grid(rdr_ctx* c, const char* who, int elem_bytes, int ndim, const int64_t* shape, const int64_t* chunk, H5ChunkGrid& G, int64_t* array_elems,
                         int64_t* nchunks) {
    const std::string w(who);
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return fail(c, RDR_ERR_INVALID, w + ": elements of 1, 2, 4 or 8 bytes");
    if (ndim < 1 || ndim > 4) return fail(c, RDR_ERR_INVALID, w + ": 1 .. 4 dimensions");
    *array_elems = *nchunks = G.chunk_elems = 1;
    for (int d = 0; d < 4; ++d) { G.shape[d] = G.chunk[d] = G.nchunk[d] = 1; }
    for (int d = 0; d < ndim; ++d) {
        const int64_t s = shape[d], k = chunk[d];
        if (s <= 0 || k <= 0 || s > ((int64_t)1 << 31) || k > ((int64_t)1 << 31)) return fail(c, RDR_ERR_INVALID, w + ": shape and chunk sizes must be positive (below 2^31)");
        const int e = 4 - ndim + d;
        G.shape[e] = s; G.chunk[e] = k; G.nchunk[e] = (s + k - 1) / k;
        if (*array_elems > ((int64_t)1 << 36) / s || G.chunk_elems > ((int64_t)1 << 36) / k) return fail(c, RDR_ERR_INVALID, w + ": more than 2^36 elements");
        *array_elems *= s; G.chunk_elems *= k;
        *nchunks *= G.nchunk[e];
        if (*nchunks > ((int64_t)1 << 36) / G.chunk_elems) return fail(c, RDR_ERR_INVALID, w + ": more than 2^36 elements");
    }
    return RDR_OK;
}

int rdr_h5_chunks(rdr_ctx* c, const void* array, int elem_bytes, int ndim, const int64_t* shape, const int64_t* chunk, const void* fill, int shuffle,
                  void* out, int loc) {
    if (!c || !array || !shape || !chunk || !fill || !out) return fail(c, RDR_ERR_INVALID, "rdr_h5_chunks: NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, "rdr_h5_chunks: loc must be RDR_HOST or RDR_DEVICE");
    H5ChunkLayout L{};
    int64_t in_elems, nchunks;
    const int rc = h5_chunk_grid(c, "rdr_h5_chunks", elem_bytes, ndim, shape, chunk, L, &in_elems, &nchunks); if (rc) return rc;
    L.total_elems = nchunks * L.chunk_elems;
    L.es = elem_bytes; L.shuffle = shuffle != 0;
    std::memcpy(L.fill, fill, (size_t)elem_bytes);
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const uint8_t* din = S.in(static_cast<const uint8_t*>(array), (size_t)in_elems * elem_bytes);
    uint8_t* dout = S.out(static_cast<uint8_t*>(out), (size_t)L.total_elems * elem_bytes);
    if (S.rc) return S.rc;
    hipLaunchKernelGGL(h5_chunks_kernel, dim3(grid_for(L.total_elems, 256, c->num_cus * 16)), dim3(256), 0, c->stream, din, L, dout);
    return S.finish();
}


// ---- zlib streams decoded on the device, and chunks put back into an array (inflate_kernels.h) -------------------------------------
int rdr_inflate_decode(rdr_ctx* c, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                       const int64_t* seg_out_bytes, void* out, int64_t out_stride, int32_t* status, int64_t* produced, int loc) {
    // three of the 44 KB workgroups per compute unit
    return decode_segments(c, "rdr_inflate_decode", src, src_bytes, seg_offset, seg_bytes, nseg, seg_out_bytes, out, out_stride, status, produced, loc, 3,
                           [&](int grid, const uint8_t* dsrc, const int64_t* tab, uint8_t* dout, int32_t* dstat, int64_t* dprod) {
        hipLaunchKernelGGL(inflate_kernel, dim3(grid), dim3(64), 0, c->stream, dsrc, src_bytes, tab, tab + nseg, tab + 2 * nseg, (int)nseg, dout, out_stride, dstat,
                           dprod, (const int32_t*)nullptr);
    });
}

// The same streams with the long ones cut at their flush points (inflate_kernels.h): scan -> the candidates' count comes down -> measure ->
// the records come down -> the plan, on the host -> the whole streams through inflate_kernel, the pieces through inflate_piece_kernel, the
// pieces' checksums folded on the device.  A call without a candidate is rdr_inflate_decode's launch behind the scan.  Always synchronises.
int rdr_inflate_decode_split(rdr_ctx* c, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                             const int64_t* seg_out_bytes, void* out, int64_t out_stride, int32_t* status, int64_t* produced, int64_t* pieces, int loc) {
    { const int rc = decode_segments_check(c, "rdr_inflate_decode_split", src, src_bytes, seg_offset, seg_bytes, nseg, seg_out_bytes, out, out_stride, status, loc); if (rc) return rc; }
    HIPCHECK(c, hipSetDevice(c->device));
    std::vector<int64_t> base((size_t)nseg + 1);                  // the streams' slots: the start and the candidate windows (infl_slots)
    std::vector<uint32_t> count((size_t)nseg);
    std::vector<int64_t> npieces((size_t)nseg, 1);
    int64_t longest = 0;
    base[0] = 0;
    for (int64_t i = 0; i < nseg; ++i) {
        base[(size_t)i + 1] = base[(size_t)i] + infl_slots(infl_clip32(seg_bytes[i]));
        longest = std::max(longest, seg_bytes[i]);
    }
    const int64_t total = base[(size_t)nseg];
    Staged S(c, loc);
    const uint8_t* dsrc = S.in(static_cast<const uint8_t*>(src), (size_t)src_bytes);
    const HostPart tabs[3] = {{seg_offset, (size_t)nseg * 8}, {seg_bytes, (size_t)nseg * 8}, {seg_out_bytes, (size_t)nseg * 8}};
    const int64_t* tab = S.table<int64_t>(SLOT_IN1, tabs, 3);
    uint8_t* dout = S.out(static_cast<uint8_t*>(out), (size_t)(nseg * out_stride));
    int32_t* dstat = S.out(status, (size_t)nseg * 4);
    int64_t* dprod = S.out(produced, (size_t)nseg * 8);         // (optional)
    const HostPart base_part{base.data(), ((size_t)nseg + 1) * 8};
    const int64_t* dbase = S.table<int64_t>(SLOT_IN2, &base_part, 1);
    uint32_t* dcand = S.scratch<uint32_t>(SLOT_IN3, (size_t)total * 4);
    uint32_t* dcount = S.scratch<uint32_t>(SLOT_IN4, (size_t)nseg * 4);
    if (S.rc) return S.rc;
    if (loc == RDR_HOST) { const int rc = upload(c, dout, out, (size_t)(nseg * out_stride)); if (rc) return rc; }
    HIPCHECK(c, hipMemsetAsync(dcand, 0xff, (size_t)total * 4, c->stream));
    HIPCHECK(c, hipMemsetAsync(dcount, 0, (size_t)nseg * 4, c->stream));
    {
        const dim3 G((unsigned)grid_for(longest, 256 * 8, c->num_cus * 4), (unsigned)std::min<int64_t>(nseg, 4096));
        hipLaunchKernelGGL(infl_scan_kernel, G, dim3(256), 0, c->stream, dsrc, src_bytes, tab, tab + nseg, (int)nseg, dbase, total, dcand, dcount);
    }
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(count.data(), dcount, (size_t)nseg * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    int64_t with_candidates = 0;
    for (int64_t i = 0; i < nseg; ++i) with_candidates += count[(size_t)i] != 0u;
    const int serial_grid = (int)std::min<int64_t>(nseg, (int64_t)c->num_cus * 3);
    if (with_candidates == 0) {
        hipLaunchKernelGGL(inflate_kernel, dim3(serial_grid), dim3(64), 0, c->stream, dsrc, src_bytes, tab, tab + nseg, tab + 2 * nseg, (int)nseg, dout, out_stride,
                           dstat, dprod, (const int32_t*)nullptr);
    } else {
        InflPiece* drec = S.scratch<InflPiece>(SLOT_IN5, (size_t)total * sizeof(InflPiece));
        if (S.rc) return S.rc;
        HIPCHECK(c, hipMemsetAsync(drec, 0xff, (size_t)total * sizeof(InflPiece), c->stream));
        hipLaunchKernelGGL(infl_measure_kernel, dim3((unsigned)std::min<int64_t>(total, (int64_t)c->num_cus * 15)), dim3(64), 0, c->stream, dsrc, src_bytes, tab,
                           tab + nseg, tab + 2 * nseg, (int)nseg, out_stride, dbase, total, dcand, dcount, drec);
        HIPCHECK(c, hipGetLastError());
        std::vector<InflPiece> rec;
        std::vector<InflJob> jobs;
        std::vector<int32_t> whole;                               // the streams that stay whole
        try { rec.resize((size_t)total); jobs.reserve((size_t)total); } catch (const std::bad_alloc&) { return fail(c, RDR_ERR_OOM, "rdr_inflate_decode_split: no host memory for the plan"); }
        HIPCHECK(c, hipMemcpyAsync(rec.data(), drec, (size_t)total * sizeof(InflPiece), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < nseg; ++i) {
            uint32_t n = 0;
            if (count[(size_t)i]) {
                const size_t at = jobs.size();
                const uint32_t nslots = (uint32_t)(base[(size_t)i + 1] - base[(size_t)i]);
                jobs.resize(at + nslots);
                n = infl_plan(rec.data() + base[(size_t)i], nslots, infl_clip32(std::min(seg_out_bytes[i], out_stride)), (int32_t)i, jobs.data() + at);
                if (n < 2) n = 0;                                 // (one piece: the whole stream, which inflate_kernel decodes in one pass)
                jobs.resize(at + n);
            }
            if (n) npieces[(size_t)i] = n; else whole.push_back((int32_t)i);
        }
        const int64_t njobs = (int64_t)jobs.size(), nwhole = (int64_t)whole.size();
        if (nwhole) {
            const HostPart part{whole.data(), (size_t)nwhole * 4};
            const int32_t* dlist = S.table<int32_t>(SLOT_IN6, &part, 1);
            if (S.rc) return S.rc;
            hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)std::min<int64_t>(nwhole, (int64_t)c->num_cus * 3)), dim3(64), 0, c->stream, dsrc, src_bytes, tab, tab + nseg,
                               tab + 2 * nseg, (int)nwhole, dout, out_stride, dstat, dprod, dlist);
            HIPCHECK(c, hipGetLastError());
        }
        if (njobs) {
            const HostPart part{jobs.data(), (size_t)njobs * sizeof(InflJob)};
            const InflJob* djobs = S.table<InflJob>(SLOT_IN5, &part, 1);          // (the records have come down: their slot is free)
            InflJobOut* dres = S.scratch<InflJobOut>(SLOT_AUX, (size_t)njobs * sizeof(InflJobOut));
            if (S.rc) return S.rc;
            hipLaunchKernelGGL(inflate_piece_kernel, dim3((unsigned)std::min<int64_t>(njobs, (int64_t)c->num_cus * 3)), dim3(64), 0, c->stream, dsrc, src_bytes, tab,
                               tab + nseg, tab + 2 * nseg, (int)nseg, dout, out_stride, djobs, njobs, dres);
            HIPCHECK(c, hipGetLastError());
            hipLaunchKernelGGL(infl_fold_kernel, dim3((unsigned)grid_for(njobs, 256, c->num_cus * 4)), dim3(256), 0, c->stream, djobs, (const InflJobOut*)dres, njobs,
                               (int)nseg, dstat, dprod);
        }
    }
    const int rc = S.finish(true);
    if (rc) return rc;
    if (pieces) std::memcpy(pieces, npieces.data(), (size_t)nseg * 8);
    return RDR_OK;
}

int rdr_h5_unchunk(rdr_ctx* c, const void* chunks, int64_t chunk_stride, const int64_t* chunk_index, int64_t npresent, int elem_bytes, int ndim,
                   const int64_t* shape, const int64_t* chunk, int shuffle, int swap, void* out, int loc) {
    if (!c || !chunks || !chunk_index || !shape || !chunk || !out) return fail(c, RDR_ERR_INVALID, "rdr_h5_unchunk: NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, "rdr_h5_unchunk: loc must be RDR_HOST or RDR_DEVICE");
    H5UnchunkLayout L{};
    int64_t out_elems, nchunks;
    const int rc = h5_chunk_grid(c, "rdr_h5_unchunk", elem_bytes, ndim, shape, chunk, L, &out_elems, &nchunks); if (rc) return rc;
    if (npresent <= 0 || npresent > nchunks) return fail(c, RDR_ERR_INVALID, "rdr_h5_unchunk: 1 .. " + std::to_string(nchunks) + " chunks may be present");
    if (chunk_stride < L.chunk_elems * elem_bytes || chunk_stride > ((int64_t)1 << 40) / npresent)
        return fail(c, RDR_ERR_INVALID, "rdr_h5_unchunk: chunk_stride must hold one decoded chunk (at most 2^40 bytes in all)");
    try {                                                       // each index inside the grid and at most once: a sorted copy of the table, never the grid
        std::vector<int64_t> sorted(chunk_index, chunk_index + npresent);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.front() < 0 || sorted.back() >= nchunks) return fail(c, RDR_ERR_INVALID, "rdr_h5_unchunk: a chunk index lies outside the chunk grid");
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(c, RDR_ERR_INVALID, "rdr_h5_unchunk: a chunk index is given twice");
    } catch (const std::bad_alloc&) {
        return fail(c, RDR_ERR_OOM, "rdr_h5_unchunk: no host memory to check the chunk table");
    }
    L.total_elems = npresent * L.chunk_elems;
    L.chunk_stride = chunk_stride;
    L.es = elem_bytes; L.shuffle = shuffle != 0; L.swap = swap != 0;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const uint8_t* din = S.in(static_cast<const uint8_t*>(chunks), (size_t)(npresent * chunk_stride));
    const HostPart index{chunk_index, (size_t)npresent * 8};      // (a host array whatever `loc` says)
    const int64_t* dtab = S.table<int64_t>(SLOT_IN1, &index, 1);
    uint8_t* dout = S.out(static_cast<uint8_t*>(out), (size_t)out_elems * elem_bytes);
    if (S.rc) return S.rc;
    if (npresent < nchunks) HIPCHECK(c, hipMemsetAsync(dout, 0, (size_t)out_elems * elem_bytes, c->stream));      // absent chunks read as 0
    hipLaunchKernelGGL(h5_unchunk_kernel, dim3(grid_for(L.total_elems, 256, c->num_cus * 16)), dim3(256), 0, c->stream, din, dtab, L, dout);
    return S.finish();
}


// ---- all-pair variograms of a station series (variogram_kernels.h; raider_amd/variogram.py) ----------------------------------------
// what both entries refuse before the device is touched
static int pair_args(rdr_ctx* c, const char* who, bool null_arg, int64_t n, int nd, int loc) {
    const std::string w(who);
    if (null_arg) return fail(c, RDR_ERR_INVALID, w + ": NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, w + ": loc must be RDR_HOST or RDR_DEVICE");
    if (n < 2 || n > ((int64_t)1 << 20)) return fail(c, RDR_ERR_INVALID, w + ": n must be 2 .. 2^20 points (got " + std::to_string(n) + ")");
    if (nd < 1 || nd > 4096) return fail(c, RDR_ERR_INVALID, w + ": nd must be 1 .. 4096 dates (got " + std::to_string(nd) + ")");
    return RDR_OK;
}

// workgroups of a pair launch: one per tile pair, at most four per compute unit (RAIDER_HIP_VARIOGRAM_GRID: another cap, for tests)
static int pair_grid(const rdr_ctx* c, int64_t n) {
    const int64_t nt = (n + VG_TILE - 1) / VG_TILE, ntp = nt * (nt + 1) / 2;
    int64_t cap = (int64_t)c->num_cus * 4;
    if (const char* e = std::getenv("RAIDER_HIP_VARIOGRAM_GRID")) { const long v = std::atol(e); if (v >= 1 && v <= 4096) cap = v; }
    return (int)std::min(ntp, cap);
}

// date groups of 4, then 2, then 1 (engine.epoch_groups): f(first date, dates)
template <typename F>
static void pair_date_groups(int nd, F&& f) {
    for (int d0 = 0; d0 < nd;) {
        const int g = nd - d0 >= 4 ? 4 : nd - d0 >= 2 ? 2 : 1;
        f(d0, g);
        d0 += g;
    }
}

int rdr_pair_distance_max(rdr_ctx* c, const double* x, const double* y, int64_t n, const double* values, int nd, double* hmax, int loc) {
    const int bad = pair_args(c, "rdr_pair_distance_max", !c || !x || !y || !values || !hmax, n, nd, loc); if (bad) return bad;
    HIPCHECK(c, hipSetDevice(c->device));
    Staged S(c, loc);
    const double *dx = S.in(x, (size_t)n * 8), *dy = S.in(y, (size_t)n * 8), *dv = S.in(values, (size_t)nd * n * 8);
    double* dh = S.out(hmax, (size_t)nd * 8);
    unsigned long long* dm = S.scratch<unsigned long long>(SLOT_AUX, (size_t)nd * 8);
    if (S.rc) return S.rc;
    HIPCHECK(c, hipMemsetAsync(dm, 0, (size_t)nd * 8, c->stream));
    const int grid = pair_grid(c, n);
    pair_date_groups(nd, [&](int d0, int g) {
        if (g == 4) hipLaunchKernelGGL(pair_hmax_kernel<4>, dim3(grid), dim3(VG_TILE), 0, c->stream, dx, dy, dv, (int)n, d0, dm);
        else if (g == 2) hipLaunchKernelGGL(pair_hmax_kernel<2>, dim3(grid), dim3(VG_TILE), 0, c->stream, dx, dy, dv, (int)n, d0, dm);
        else hipLaunchKernelGGL(pair_hmax_kernel<1>, dim3(grid), dim3(VG_TILE), 0, c->stream, dx, dy, dv, (int)n, d0, dm);
    });
    hipLaunchKernelGGL(pair_hmax_finish_kernel, dim3((nd + 255) / 256), dim3(256), 0, c->stream, dm, nd, dh);
    return S.finish();
}

int rdr_pair_variogram(rdr_ctx* c, const double* x, const double* y, int64_t n, const double* values, int nd, const double* edges, int nedge_rows,
                       int nbins, int64_t* count, double* lag_sum, double* gamma_sum, int loc) {
    static const char* who = "rdr_pair_variogram";
    const int bad = pair_args(c, who, !c || !x || !y || !values || !edges || !count || !lag_sum || !gamma_sum, n, nd, loc); if (bad) return bad;
    if (nbins < 1 || nbins > VG_MAXB) return fail(c, RDR_ERR_INVALID, std::string(who) + ": nbins must be 1 .. 64 (got " + std::to_string(nbins) + ")");
    if (nedge_rows != 1 && nedge_rows != nd)
        return fail(c, RDR_ERR_INVALID, std::string(who) + ": nedge_rows must be 1 or nd = " + std::to_string(nd) + " (got " + std::to_string(nedge_rows) + ")");
    const size_t ne = (size_t)nbins + 1, nedges = (size_t)nedge_rows * ne;
    // edge rows: finite and strictly ascending (a row on the device is read back for the check: at most 65 numbers per row)
    std::vector<double> back;
    const double* he = edges;
    if (loc == RDR_DEVICE) {
        HIPCHECK(c, hipSetDevice(c->device));
        back.resize(nedges);
        HIPCHECK(c, hipMemcpyAsync(back.data(), edges, nedges * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        he = back.data();
    }
    for (int r = 0; r < nedge_rows; ++r)
        for (size_t k = 0; k < ne; ++k) {
            const double e = he[r * ne + k];
            if (!std::isfinite(e)) return fail(c, RDR_ERR_INVALID, std::string(who) + ": edge row " + std::to_string(r) + " holds a value that is not finite");
            if (k && !(e > he[r * ne + k - 1]))
                return fail(c, RDR_ERR_INVALID, std::string(who) + ": edge row " + std::to_string(r) + " is not strictly ascending at index " + std::to_string(k));
        }
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t nout = (size_t)nd * nbins;
    const int grid = pair_grid(c, n);
    Staged S(c, loc);
    const double *dx = S.in(x, (size_t)n * 8), *dy = S.in(y, (size_t)n * 8), *dv = S.in(values, (size_t)nd * n * 8), *de = S.in(edges, nedges * 8);
    long long* dc = reinterpret_cast<long long*>(S.out(count, nout * 8));
    double *dl = S.out(lag_sum, nout * 8), *dg = S.out(gamma_sum, nout * 8);
    const size_t part = (size_t)grid * 4 * nbins;                 // elements of one partial array of the largest date group
    double* dpart = S.scratch<double>(SLOT_AUX, 3 * part * 8);
    if (S.rc) return S.rc;
    unsigned long long* pc = reinterpret_cast<unsigned long long*>(dpart);
    double *pl = dpart + part, *pg = dpart + 2 * part;
    const int per_date = nedge_rows > 1 ? 1 : 0;
    pair_date_groups(nd, [&](int d0, int g) {
        if (g == 4) hipLaunchKernelGGL(pair_variogram_kernel<4>, dim3(grid), dim3(VG_TILE), 0, c->stream, dx, dy, dv, (int)n, d0, de, per_date, nbins, pc, pl, pg);
        else if (g == 2) hipLaunchKernelGGL(pair_variogram_kernel<2>, dim3(grid), dim3(VG_TILE), 0, c->stream, dx, dy, dv, (int)n, d0, de, per_date, nbins, pc, pl, pg);
        else hipLaunchKernelGGL(pair_variogram_kernel<1>, dim3(grid), dim3(VG_TILE), 0, c->stream, dx, dy, dv, (int)n, d0, de, per_date, nbins, pc, pl, pg);
        hipLaunchKernelGGL(pair_reduce_kernel, dim3((g * nbins + 63) / 64), dim3(64), 0, c->stream, pc, pl, pg, grid, g * nbins, (long long)d0 * nbins, dc, dl, dg);
    });
    return S.finish();
}

// ---- per-grid-cell variograms in one pass (cell_variogram_kernels.h; raider_amd/variogram.py: grid_variograms) ----------------------
int rdr_cell_variogram(rdr_ctx* c, const double* x, const double* y, int64_t n, const int64_t* cell_start, int ncells, const double* values, int nd,
                       int deramp, int min_valid, const double* edges, int nbins, int64_t* nvalid, double* hmax, int32_t* status, int64_t* count,
                       double* lag_sum, double* gamma_sum, double* edges_out, double* residuals, int64_t* tot_count, double* tot_lag, double* tot_gamma,
                       int loc) {
    static const char* who = "rdr_cell_variogram";
    const std::string w(who);
    const int bad = pair_args(c, who, !c || !x || !y || !cell_start || !values || !nvalid || !hmax || !status || !count || !lag_sum || !gamma_sum, n, nd, loc);
    if (bad) return bad;
    if (nbins < 1 || nbins > VG_MAXB) return fail(c, RDR_ERR_INVALID, w + ": nbins must be 1 .. 64 (got " + std::to_string(nbins) + ")");
    if (ncells < 1 || ncells > (1 << 20)) return fail(c, RDR_ERR_INVALID, w + ": ncells must be 1 .. 2^20 cells (got " + std::to_string(ncells) + ")");
    if (min_valid < 0) return fail(c, RDR_ERR_INVALID, w + ": min_valid must not be negative (got " + std::to_string(min_valid) + ")");
    if (deramp != 0 && deramp != 1) return fail(c, RDR_ERR_INVALID, w + ": deramp must be 0 or 1 (got " + std::to_string(deramp) + ")");
    if (residuals && !deramp) return fail(c, RDR_ERR_INVALID, w + ": residuals are written only with deramp = 1");
    const bool totals = tot_count || tot_lag || tot_gamma;
    if (totals && !(tot_count && tot_lag && tot_gamma)) return fail(c, RDR_ERR_INVALID, w + ": tot_count, tot_lag and tot_gamma come together or not at all");
    if (totals && !edges) return fail(c, RDR_ERR_INVALID, w + ": totals need given edges (one row per cell)");
    const size_t ne = (size_t)nbins + 1, nedges = edges ? (size_t)ncells * ne : 0;
    // cell_start and the edge rows are checked on the host (arrays on the device are read back: ncells + 1 and ncells * (nbins + 1) numbers)
    std::vector<int64_t> back_cs; std::vector<double> back_e;
    const int64_t* hcs = cell_start; const double* he = edges;
    if (loc == RDR_DEVICE) {
        HIPCHECK(c, hipSetDevice(c->device));
        back_cs.resize((size_t)ncells + 1);
        HIPCHECK(c, hipMemcpyAsync(back_cs.data(), cell_start, ((size_t)ncells + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        if (edges) { back_e.resize(nedges); HIPCHECK(c, hipMemcpyAsync(back_e.data(), edges, nedges * 8, hipMemcpyDeviceToHost, c->stream)); }
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        hcs = back_cs.data(); if (edges) he = back_e.data();
    }
    if (hcs[0] != 0) return fail(c, RDR_ERR_INVALID, w + ": cell_start[0] must be 0 (got " + std::to_string(hcs[0]) + ")");
    if (hcs[ncells] != n) return fail(c, RDR_ERR_INVALID, w + ": cell_start[ncells] must be n = " + std::to_string(n) + " (got " + std::to_string(hcs[ncells]) + ")");
    for (int k = 0; k < ncells; ++k)
        if (hcs[k + 1] < hcs[k]) return fail(c, RDR_ERR_INVALID, w + ": cell_start is not ascending at index " + std::to_string(k + 1));
    for (int r = 0; edges && r < ncells; ++r)
        for (size_t k = 0; k < ne; ++k) {
            const double e = he[r * ne + k];
            if (!std::isfinite(e)) return fail(c, RDR_ERR_INVALID, w + ": edge row " + std::to_string(r) + " holds a value that is not finite");
            if (k && !(e > he[r * ne + k - 1]))
                return fail(c, RDR_ERR_INVALID, w + ": edge row " + std::to_string(r) + " is not strictly ascending at index " + std::to_string(k));
        }
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t cd = (size_t)ncells * nd, vbytes = (size_t)nd * n * 8;
    const void* d;
    CellVgArgs A{};
    int rc = stage_in(c, SLOT_IN0, x, (size_t)n * 8, loc, &d); if (rc) return rc; A.x = (const double*)d;
    rc = stage_in(c, SLOT_IN1, y, (size_t)n * 8, loc, &d); if (rc) return rc; A.y = (const double*)d;
    rc = stage_in(c, SLOT_IN2, cell_start, ((size_t)ncells + 1) * 8, loc, &d); if (rc) return rc; A.cell_start = (const long long*)d;
    rc = stage_in(c, SLOT_IN3, values, vbytes, loc, &d); if (rc) return rc; A.values = (const double*)d;
    rc = stage_in(c, SLOT_IN4, edges, nedges * 8, loc, &d); if (rc) return rc; A.edges = (const double*)d;
    // the outputs: where they are (loc = device), or back to back in one slot from which they are downloaded (loc = host)
    struct Out { void* host; size_t bytes; void* dev; };
    Out outs[11] = {{nvalid, cd * 8, nullptr}, {hmax, cd * 8, nullptr}, {status, cd * 4, nullptr}, {count, cd * nbins * 8, nullptr},
                    {lag_sum, cd * nbins * 8, nullptr}, {gamma_sum, cd * nbins * 8, nullptr}, {edges_out, cd * ne * 8, nullptr}, {residuals, vbytes, nullptr},
                    {tot_count, (size_t)ncells * nbins * 8, nullptr}, {tot_lag, (size_t)ncells * nbins * 8, nullptr}, {tot_gamma, (size_t)ncells * nbins * 8, nullptr}};
    if (loc == RDR_DEVICE) {
        for (Out& o : outs) o.dev = o.host;
    } else {
        size_t total = 0;
        for (Out& o : outs) if (o.host) total += (o.bytes + 15) & ~(size_t)15;
        void* base; rc = ensure(c, SLOT_OUT0, total, &base); if (rc) return rc;
        size_t off = 0;
        for (Out& o : outs) if (o.host) { o.dev = static_cast<char*>(base) + off; off += (o.bytes + 15) & ~(size_t)15; }
    }
    A.n = n; A.nd = nd; A.deramp = deramp; A.min_valid = min_valid; A.nbins = nbins;
    A.nvalid = (long long*)outs[0].dev; A.hmax = (double*)outs[1].dev; A.status = (int*)outs[2].dev; A.count = (long long*)outs[3].dev;
    A.lag = (double*)outs[4].dev; A.gamma = (double*)outs[5].dev; A.edges_out = (double*)outs[6].dev; A.resid = (double*)outs[7].dev;
    if (deramp && !A.resid) { void* t; rc = ensure(c, SLOT_AUX, vbytes, &t); if (rc) return rc; A.resid = (double*)t; }   // (cells beyond LDS read them back)
    // date groups of 4, then 2, then 1: one launch per group size, a workgroup per (cell, group)
    const int n4 = nd / 4, d2 = n4 * 4, n2 = (nd - d2) / 2, d1 = d2 + n2 * 2, n1 = nd - d1;
    if (n4) hipLaunchKernelGGL(cell_variogram_kernel<4>, dim3((unsigned)ncells * n4), dim3(VG_TILE), 0, c->stream, A, 0, n4);
    if (n2) hipLaunchKernelGGL(cell_variogram_kernel<2>, dim3((unsigned)ncells * n2), dim3(VG_TILE), 0, c->stream, A, d2, n2);
    if (n1) hipLaunchKernelGGL(cell_variogram_kernel<1>, dim3((unsigned)ncells * n1), dim3(VG_TILE), 0, c->stream, A, d1, n1);
    if (totals) {
        const long long nt = (long long)ncells * nbins;
        hipLaunchKernelGGL(cell_totals_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, A.count, A.lag, A.gamma, A.status, ncells, nd, nbins,
                           (long long*)outs[8].dev, (double*)outs[9].dev, (double*)outs[10].dev);
    }
    HIPCHECK(c, hipGetLastError());
    for (Out& o : outs) { rc = finish_out(c, o.host, o.dev, o.bytes, loc); if (rc) return rc; }
    if (loc == RDR_HOST) HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

// ---- gridded station statistics (grid_stats_kernels.h; raider_amd/station_stats.py: grid_statistics) --------------------------------
int rdr_grid_stats(rdr_ctx* c, const double* values, int64_t n, int nd, const int64_t* cell_start, int ncells, int64_t* st_nobs, double* st_mean,
                   double* st_median, double* st_stdev, int64_t* nstations, double* mean_of_means, double* mean_of_medians, double* mean_of_stdevs,
                   int64_t* cell_nobs, double* abs_mean, double* abs_median, double* abs_stdev, int loc) {
    const std::string w("rdr_grid_stats");
    if (!c || !values || !cell_start) return fail(c, RDR_ERR_INVALID, w + ": NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, w + ": loc must be RDR_HOST or RDR_DEVICE");
    if (n < 1 || n > ((int64_t)1 << 20)) return fail(c, RDR_ERR_INVALID, w + ": n must be 1 .. 2^20 stations (got " + std::to_string(n) + ")");
    if (nd < 1 || nd > 4096) return fail(c, RDR_ERR_INVALID, w + ": nd must be 1 .. 4096 dates (got " + std::to_string(nd) + ")");
    if (ncells < 1 || ncells > (1 << 20)) return fail(c, RDR_ERR_INVALID, w + ": ncells must be 1 .. 2^20 cells (got " + std::to_string(ncells) + ")");
    // a group comes whole (its median apart) or not at all
    const bool st_any = st_nobs || st_mean || st_stdev || st_median, st_all = st_nobs && st_mean && st_stdev;
    const bool of_any = nstations || mean_of_means || mean_of_stdevs || mean_of_medians, of_all = nstations && mean_of_means && mean_of_stdevs;
    const bool ab_any = cell_nobs || abs_mean || abs_stdev || abs_median, ab_all = cell_nobs && abs_mean && abs_stdev;
    if (st_any && !st_all) return fail(c, RDR_ERR_INVALID, w + ": st_nobs, st_mean and st_stdev come together or not at all (st_median only with them)");
    if (of_any && !of_all)
        return fail(c, RDR_ERR_INVALID, w + ": nstations, mean_of_means and mean_of_stdevs come together or not at all (mean_of_medians only with them)");
    if (ab_any && !ab_all) return fail(c, RDR_ERR_INVALID, w + ": cell_nobs, abs_mean and abs_stdev come together or not at all (abs_median only with them)");
    if (!st_any && !of_any && !ab_any) return fail(c, RDR_ERR_INVALID, w + ": every output group is NULL");
    // cell_start is checked on the host (an array on the device is read back: ncells + 1 numbers)
    std::vector<int64_t> back_cs;
    const int64_t* hcs = cell_start;
    if (loc == RDR_DEVICE) {
        HIPCHECK(c, hipSetDevice(c->device));
        back_cs.resize((size_t)ncells + 1);
        HIPCHECK(c, hipMemcpyAsync(back_cs.data(), cell_start, ((size_t)ncells + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        hcs = back_cs.data();
    }
    if (hcs[0] != 0) return fail(c, RDR_ERR_INVALID, w + ": cell_start[0] must be 0 (got " + std::to_string(hcs[0]) + ")");
    if (hcs[ncells] != n) return fail(c, RDR_ERR_INVALID, w + ": cell_start[ncells] must be n = " + std::to_string(n) + " (got " + std::to_string(hcs[ncells]) + ")");
    for (int k = 0; k < ncells; ++k) {
        if (hcs[k + 1] < hcs[k]) return fail(c, RDR_ERR_INVALID, w + ": cell_start is not ascending at index " + std::to_string(k + 1));
        if ((hcs[k + 1] - hcs[k]) * nd > (int64_t)2147483647)
            return fail(c, RDR_ERR_INVALID, w + ": cell " + std::to_string(k) + " holds more than 2^31 - 1 slots (" + std::to_string(hcs[k + 1] - hcs[k]) +
                        " stations x " + std::to_string(nd) + " dates)");
    }
    HIPCHECK(c, hipSetDevice(c->device));
    const void* d;
    GridStatsArgs A{};
    int rc = stage_in(c, SLOT_IN0, values, (size_t)nd * n * 8, loc, &d); if (rc) return rc; A.values = (const double*)d;
    rc = stage_in(c, SLOT_IN1, cell_start, ((size_t)ncells + 1) * 8, loc, &d); if (rc) return rc; A.cell_start = (const long long*)d;
    // the outputs: where they are (loc = device), or back to back in one slot from which they are downloaded (loc = host)
    struct Out { void* host; size_t bytes; void* dev; };
    const size_t sb = (size_t)n * 8, cb = (size_t)ncells * 8;
    Out outs[12] = {{st_nobs, sb, nullptr}, {st_mean, sb, nullptr}, {st_median, sb, nullptr}, {st_stdev, sb, nullptr},
                    {nstations, cb, nullptr}, {mean_of_means, cb, nullptr}, {mean_of_medians, cb, nullptr}, {mean_of_stdevs, cb, nullptr},
                    {cell_nobs, cb, nullptr}, {abs_mean, cb, nullptr}, {abs_median, cb, nullptr}, {abs_stdev, cb, nullptr}};
    if (loc == RDR_DEVICE) {
        for (Out& o : outs) o.dev = o.host;
    } else {
        size_t total = 0;
        for (Out& o : outs) if (o.host) total += (o.bytes + 15) & ~(size_t)15;
        void* base; rc = ensure(c, SLOT_OUT0, total, &base); if (rc) return rc;
        size_t off = 0;
        for (Out& o : outs) if (o.host) { o.dev = static_cast<char*>(base) + off; off += (o.bytes + 15) & ~(size_t)15; }
    }
    // station statistics that only the cell means read live in a work array of the context
    void* st[4] = {outs[0].dev, outs[1].dev, outs[2].dev, outs[3].dev};
    const bool need[4] = {st_any || of_any, st_any || of_any, st_median || mean_of_medians, st_any || of_any};
    if ((need[0] && !st[0]) || (need[2] && !st[2])) {
        void* t; rc = ensure(c, SLOT_AUX, 4 * sb, &t); if (rc) return rc;
        for (int k = 0; k < 4; ++k) if (need[k] && !st[k]) st[k] = static_cast<char*>(t) + k * sb;
    }
    A.n = n; A.nd = nd;
    A.st_nobs = (long long*)st[0]; A.st_mean = (double*)st[1]; A.st_median = need[2] ? (double*)st[2] : nullptr; A.st_stdev = (double*)st[3];
    A.nstations = (long long*)outs[4].dev; A.mean_of_means = (double*)outs[5].dev; A.mean_of_medians = (double*)outs[6].dev; A.mean_of_stdevs = (double*)outs[7].dev;
    A.cell_nobs = (long long*)outs[8].dev; A.abs_mean = (double*)outs[9].dev; A.abs_median = (double*)outs[10].dev; A.abs_stdev = (double*)outs[11].dev;
    if (need[0]) hipLaunchKernelGGL(grid_stats_station_kernel, dim3((unsigned)((n + GS_STATIONS - 1) / GS_STATIONS)), dim3(GS_TILE), 0, c->stream, A);
    if (of_any || ab_any) hipLaunchKernelGGL(grid_stats_cell_kernel, dim3((unsigned)ncells), dim3(GS_TILE), 0, c->stream, A);
    HIPCHECK(c, hipGetLastError());
    for (Out& o : outs) { rc = finish_out(c, o.host, o.dev, o.bytes, loc); if (rc) return rc; }
    if (loc == RDR_HOST) HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

// ---- seasonal sinusoids (seasonal_kernels.h; raider_amd/seasonal.py: seasonal_fits, grid_seasonal) -------------------------------------
int rdr_seasonal_fit(rdr_ctx* c, const double* t, const double* values, int64_t n, int nd, const double* omega, int k, int scan, double min_span,
                     double min_frac, const int64_t* cell_start, int ncells, double* station, double* cells, int loc) {
    const std::string w("rdr_seasonal_fit");
    if (!c || !t || !values || !omega || !station) return fail(c, RDR_ERR_INVALID, w + ": NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, w + ": loc must be RDR_HOST or RDR_DEVICE");
    if (n < 1 || n > ((int64_t)1 << 20)) return fail(c, RDR_ERR_INVALID, w + ": n must be 1 .. 2^20 stations (got " + std::to_string(n) + ")");
    if (nd < 1 || nd > 4096) return fail(c, RDR_ERR_INVALID, w + ": nd must be 1 .. 4096 dates (got " + std::to_string(nd) + ")");
    if (k < 1 || k > 4096) return fail(c, RDR_ERR_INVALID, w + ": k must be 1 .. 4096 frequencies (got " + std::to_string(k) + ")");
    if (scan != 0 && scan != 1) return fail(c, RDR_ERR_INVALID, w + ": scan must be 0 or 1");
    if (!scan && k != 1) return fail(c, RDR_ERR_INVALID, w + ": the fixed mode (scan = 0) takes one frequency (got k = " + std::to_string(k) + ")");
    if (!(min_span >= 0.0) || !std::isfinite(min_span)) return fail(c, RDR_ERR_INVALID, w + ": min_span must be finite and >= 0");
    if (!std::isfinite(min_frac)) return fail(c, RDR_ERR_INVALID, w + ": min_frac must be finite");
    for (int i = 0; i < k; ++i) {
        if (!std::isfinite(omega[i]) || !(omega[i] > 0.0)) return fail(c, RDR_ERR_INVALID, w + ": omega[" + std::to_string(i) + "] must be finite and > 0");
        if (i && !(omega[i] > omega[i - 1])) return fail(c, RDR_ERR_INVALID, w + ": omega must ascend (index " + std::to_string(i) + ")");
    }
    double tmin = t[0], tmax = t[0];
    for (int d = 0; d < nd; ++d) {
        if (!std::isfinite(t[d])) return fail(c, RDR_ERR_INVALID, w + ": t[" + std::to_string(d) + "] is not finite");
        tmin = std::min(tmin, t[d]); tmax = std::max(tmax, t[d]);
    }
    if ((cell_start == nullptr) != (cells == nullptr)) return fail(c, RDR_ERR_INVALID, w + ": cell_start and cells come together or not at all");
    if (cells && (ncells < 1 || ncells > (1 << 20))) return fail(c, RDR_ERR_INVALID, w + ": ncells must be 1 .. 2^20 cells (got " + std::to_string(ncells) + ")");
    HIPCHECK(c, hipSetDevice(c->device));
    if (cells) {                                  // cell_start is checked on the host (an array on the device is read back)
        std::vector<int64_t> back_cs;
        const int64_t* hcs = cell_start;
        if (loc == RDR_DEVICE) {
            back_cs.resize((size_t)ncells + 1);
            HIPCHECK(c, hipMemcpyAsync(back_cs.data(), cell_start, ((size_t)ncells + 1) * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(c, hipStreamSynchronize(c->stream));
            hcs = back_cs.data();
        }
        if (hcs[0] != 0) return fail(c, RDR_ERR_INVALID, w + ": cell_start[0] must be 0 (got " + std::to_string(hcs[0]) + ")");
        if (hcs[ncells] != n) return fail(c, RDR_ERR_INVALID, w + ": cell_start[ncells] must be n = " + std::to_string(n) + " (got " + std::to_string(hcs[ncells]) + ")");
        for (int g = 0; g < ncells; ++g)
            if (hcs[g + 1] < hcs[g]) return fail(c, RDR_ERR_INVALID, w + ": cell_start is not ascending at index " + std::to_string(g + 1));
    }
    SeasonalArgs A{};
    A.n = n; A.nd = nd; A.k = k; A.scan = scan; A.ncells = cells ? ncells : 0;
    A.min_span = min_span; A.min_frac = min_frac; A.t_ref = 0.5 * (tmin + tmax);
    A.ntiles = (k + SF_KT - 1) / SF_KT;
    const unsigned nblk = (unsigned)((n + 63) / 64);
    // enough waves to fill the device: the frequency tiles are cut into segments, which changes no result
    A.nseg = scan ? std::max(1, std::min(A.ntiles, (int)((8192 + nblk - 1) / nblk))) : 0;
    A.tiles_per_seg = scan ? (A.ntiles + A.nseg - 1) / A.nseg : 0;
    if (scan) A.nseg = (A.ntiles + A.tiles_per_seg - 1) / A.tiles_per_seg;
    std::vector<double> small((size_t)nd + k);
    for (int d = 0; d < nd; ++d) small[d] = t[d] - A.t_ref;
    for (int i = 0; i < k; ++i) small[(size_t)nd + i] = omega[i];
    const void* d;
    int rc = stage_in(c, SLOT_IN0, values, (size_t)nd * n * 8, loc, &d); if (rc) return rc; A.values = (const double*)d;
    rc = stage_in(c, SLOT_IN1, cell_start, ((size_t)ncells + 1) * 8, loc, &d); if (rc) return rc; A.cell_start = (const long long*)d;
    rc = stage_in(c, SLOT_IN2, small.data(), small.size() * 8, RDR_HOST, &d); if (rc) return rc;
    A.tau = (const double*)d; A.omega = A.tau + nd;
    const size_t tab_b = scan ? (size_t)A.ntiles * nd * SF_KT * sizeof(double2) : 0, prep_b = (size_t)5 * n * 8, best_b = (size_t)A.nseg * 2 * n * 8;
    void* aux; rc = ensure(c, SLOT_AUX, tab_b + prep_b + best_b, &aux); if (rc) return rc;
    A.table = (double2*)aux; A.prep = (double*)(static_cast<char*>(aux) + tab_b); A.best = (double*)(static_cast<char*>(aux) + tab_b + prep_b);
    const size_t sb = (size_t)SF_NCOL * n * 8, cb = cells ? (size_t)2 * SF_NREF * ncells * 8 : 0;
    void* ds = station; void* dc = cells;
    if (loc == RDR_HOST) {
        void* base; rc = ensure(c, SLOT_OUT0, sb + cb, &base); if (rc) return rc;
        ds = base; dc = cells ? static_cast<char*>(base) + sb : nullptr;
    }
    A.station = (double*)ds; A.cells = (double*)dc;
    hipLaunchKernelGGL(seasonal_prep_kernel, dim3(nblk), dim3(64), 0, c->stream, A);
    if (scan) {
        const long long total = (long long)A.ntiles * nd * SF_KT;
        hipLaunchKernelGGL(seasonal_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, A);
        hipLaunchKernelGGL(seasonal_scan_kernel, dim3(nblk, (unsigned)A.nseg), dim3(64), 0, c->stream, A);
    }
    hipLaunchKernelGGL(seasonal_fit_kernel, dim3(nblk), dim3(64), 0, c->stream, A);
    if (cells) hipLaunchKernelGGL(seasonal_cell_kernel, dim3((unsigned)(((long long)ncells * SF_NREF + 255) / 256)), dim3(256), 0, c->stream, A);
    HIPCHECK(c, hipGetLastError());
    rc = finish_out(c, station, ds, sb, loc); if (rc) return rc;
    rc = finish_out(c, cells, dc, cb, loc); if (rc) return rc;
    if (loc == RDR_HOST) HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}

// ---- exponential variogram models (variogram_fit_kernels.h; raider_amd/variogram.py: fit_variograms) -----------------------------------
int rdr_variogram_fit(rdr_ctx* c, const double* h, const double* gamma, int64_t nfits, int m, const double* ub, double f_scale, int k_scan,
                      double* params, double* cost, double* rmse, int64_t* n, int32_t* status, int32_t* flags, int loc) {
    const std::string w("rdr_variogram_fit");
    if (!c || !h || !gamma || !params || !cost || !rmse || !n || !status || !flags) return fail(c, RDR_ERR_INVALID, w + ": NULL argument");
    if (loc != RDR_HOST && loc != RDR_DEVICE) return fail(c, RDR_ERR_INVALID, w + ": loc must be RDR_HOST or RDR_DEVICE");
    if (nfits < 1 || nfits > ((int64_t)1 << 22)) return fail(c, RDR_ERR_INVALID, w + ": nfits must be 1 .. 2^22 rows (got " + std::to_string(nfits) + ")");
    if (m < 1 || m > 65536) return fail(c, RDR_ERR_INVALID, w + ": m must be 1 .. 65536 columns (got " + std::to_string(m) + ")");
    if (nfits * m > ((int64_t)1 << 30)) return fail(c, RDR_ERR_INVALID, w + ": nfits x m must not exceed 2^30 values (got " + std::to_string(nfits * m) + ")");
    if (!std::isfinite(f_scale) || !(f_scale > 0.0)) return fail(c, RDR_ERR_INVALID, w + ": f_scale must be finite and > 0");
    if (k_scan < 64 || k_scan > 4096 || k_scan % 64) return fail(c, RDR_ERR_INVALID, w + ": k_scan must be a multiple of 64 in 64 .. 4096 (got " + std::to_string(k_scan) + ")");
    HIPCHECK(c, hipSetDevice(c->device));
    VarioFitArgs A{};
    const void* d;
    const size_t vb = (size_t)nfits * m * 8;
    int rc = stage_in(c, SLOT_IN0, h, vb, loc, &d); if (rc) return rc; A.h = (const double*)d;
    rc = stage_in(c, SLOT_IN1, gamma, vb, loc, &d); if (rc) return rc; A.gamma = (const double*)d;
    rc = stage_in(c, SLOT_IN2, ub, (size_t)nfits * 24, loc, &d); if (rc) return rc; A.ub = (const double*)d;
    // the outputs: where they are (loc = device), or back to back in one slot from which they are downloaded (loc = host)
    struct Out { void* host; size_t bytes; void* dev; };
    const size_t fb = (size_t)nfits * 8;
    Out outs[6] = {{params, 3 * fb, nullptr}, {cost, fb, nullptr}, {rmse, fb, nullptr}, {n, fb, nullptr}, {status, fb / 2, nullptr}, {flags, fb / 2, nullptr}};
    if (loc == RDR_DEVICE) {
        for (Out& o : outs) o.dev = o.host;
    } else {
        size_t total = 0;
        for (Out& o : outs) total += (o.bytes + 15) & ~(size_t)15;
        void* base; rc = ensure(c, SLOT_OUT0, total, &base); if (rc) return rc;
        size_t off = 0;
        for (Out& o : outs) { o.dev = static_cast<char*>(base) + off; off += (o.bytes + 15) & ~(size_t)15; }
    }
    A.nfits = nfits; A.m = m; A.k_scan = k_scan; A.f_scale = f_scale;
    A.params = (double*)outs[0].dev; A.cost = (double*)outs[1].dev; A.rmse = (double*)outs[2].dev; A.n = (long long*)outs[3].dev;
    A.status = (int*)outs[4].dev; A.flags = (int*)outs[5].dev;
    // one wave per row in each launch; a row is fitted by the instantiation its number of present columns selects
    const size_t lds = (size_t)(128 + 64 * std::min(m, 64)) * 8;
    hipLaunchKernelGGL(variogram_fit_kernel<false>, dim3((unsigned)nfits), dim3(64), lds, c->stream, A);
    if (m > 64) hipLaunchKernelGGL(variogram_fit_kernel<true>, dim3((unsigned)nfits), dim3(64), 0, c->stream, A);
    HIPCHECK(c, hipGetLastError());
    for (Out& o : outs) { rc = finish_out(c, o.host, o.dev, o.bytes, loc); if (rc) return rc; }
    if (loc == RDR_HOST) HIPCHECK(c, hipStreamSynchronize(c->stream));
    return RDR_OK;
}
