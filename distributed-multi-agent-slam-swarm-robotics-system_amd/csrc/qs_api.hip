// qs_api.hip -- the C ABI of include/quasar_slam.h: context, device memory, and the per-batch
// pipeline  decode (K0) -> SLAM drift (K4) -> raycast (K1) [-> EKF (K5)]  on one HIP stream.
#include <math.h>
#include <algorithm>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qs_internal.h"

static thread_local std::string g_create_err;
static void chain_stats_poll(qs_ctx *c, bool synced, const unsigned int *fresh);
static int flush_edge_rays(qs_ctx *c);      // exact-trig mode: rays waiting for libm end points (defined with the ingest path)
#define FLUSHCHK(c) do { int rcf__ = flush_edge_rays(c); if (rcf__ != QS_OK) return rcf__; } while (0)

static int qs_fail(qs_ctx *c, int code, const char *what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}
#define HIPCHK(c, x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return qs_fail((c), QS_E_HIP, #x, e__); } while (0)
#define ARGCHK(c, cond) do { if (!(cond)) return qs_fail((c), QS_E_INVAL, "invalid argument: " #cond); } while (0)
#define HIPRET(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return e__; } while (0)     // (helpers that return hipError_t)

struct ScopedEvent {                        // an event of one call, destroyed with its scope (as DevBuf frees a buffer)
    hipEvent_t e = nullptr;
    ScopedEvent() = default;
    ScopedEvent(const ScopedEvent &) = delete;
    ScopedEvent &operator=(const ScopedEvent &) = delete;
    ~ScopedEvent() { if (e) hipEventDestroy(e); }
};
static const size_t QS_IO_WS_FLOOR = (size_t)1 << 16;      // qs_ctx::io_ws doubles from 64 KiB

extern "C" const char *qs_version(void) { return "quasar-slam-amd 0.1 (gfx950)"; }

extern "C" int qs_config_default(qs_config *cfg)
{
    if (!cfg) return QS_E_INVAL;
    memset(cfg, 0, sizeof *cfg);
    cfg->size = 200; cfg->res = 0.05; cfg->ox = -5.0; cfg->oy = -5.0;      // dual_bot_mapper.py:87-90
    cfg->separation = 0.0;                                                  // :715
    cfg->min_dist = 0.05; cfg->max_dist = 1.20;                             // :57-58
    cfg->closure_radius = 0.60; cfg->min_poses_between = 30; cfg->closure_correction = 0.5;  // :97-99
    cfg->max_agent = 2;                                                     // :842
    cfg->bots_per_graph = 0;
    cfg->enable_counts = 1;
    cfg->enable_ekf = 0;
    cfg->ekf_metres_per_tick = 0.0107;        // simulation_tools/generate_fake_dual_session.py:462
    cfg->device = 0;
    cfg->raycast_mode = 0;
    cfg->exact_trig = 1;
    return QS_OK;
}

// smallest double T with sqrt(T) >= radius: (s < T) <=> (sqrt(s) < radius) for correctly rounded sqrt
static double r2_threshold_for(double radius)
{
    if (!(radius > 0)) return 0.0;
    double t = radius * radius;
    while (sqrt(t) >= radius) t = nextafter(t, 0.0);
    while (sqrt(t) < radius) t = nextafter(t, INFINITY);
    return t;
}

// a graph array grown to new_cap, its first old_n entries kept; on failure the old array stays as it was
template <typename T>
static hipError_t grow_array(DevBuf<T> &a, long long old_n, long long new_cap, hipStream_t st)
{
    DevBuf<T> q;
    HIPRET(q.alloc((size_t)new_cap));
    if (a.p && old_n > 0) {
        HIPRET(hipMemcpyAsync(q.p, a.p, (size_t)old_n * sizeof(T), hipMemcpyDeviceToDevice, st));
        HIPRET(hipStreamSynchronize(st));
    }
    a = std::move(q);                        // (frees the old array)
    return hipSuccess;
}

// nodes (first node of every directory entry + the overflow pool): "empty" (idx bytes 0x7f -> a huge node
// index) and unlinked (next 0)
static hipError_t grow_pool(qs_ctx *c, QsGraphBufs &G, long long old_cap, long long new_cap)
{
    const size_t fixed = 1 + c->dir_entries, n_new = fixed + (size_t)new_cap, n_old = fixed + (size_t)old_cap;
    const size_t keep = G.nodes.p ? n_old : 0;          // nodes and links copied over; the rest start empty
    DevBuf<QsLmNode> nodes; DevBuf<unsigned int> next, misc;
    HIPRET(nodes.alloc(n_new));
    HIPRET(next.alloc(n_new));
    HIPRET(misc.alloc((size_t)new_cap));
    HIPRET(hipMemsetAsync(nodes.p + keep, 0x7f, (n_new - keep) * sizeof(QsLmNode), c->stream));
    HIPRET(hipMemsetAsync(next.p + keep, 0, (n_new - keep) * sizeof(unsigned int), c->stream));
    if (G.nodes.p) {
        HIPRET(hipMemcpyAsync(nodes.p, G.nodes.p, n_old * sizeof(QsLmNode), hipMemcpyDeviceToDevice, c->stream));
        HIPRET(hipMemcpyAsync(next.p, G.nd_next.p, n_old * sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
        if (old_cap > 0) HIPRET(hipMemcpyAsync(misc.p, G.misc.p, (size_t)old_cap * sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPRET(hipStreamSynchronize(c->stream));
    G.nodes = std::move(nodes); G.nd_next = std::move(next); G.misc = std::move(misc);
    return hipSuccess;
}

static int graph_reserve(qs_ctx *c, int g, long long need_lms, long long need_cls, long long have_lms,
                         long long have_cls)
{
    QsGraphBufs &G = c->graphs[g];
    bool changed = false;
    if (!G.dir.p) {
        HIPCHK(c, G.dir.alloc(c->dir_entries));
        HIPCHK(c, hipMemsetAsync(G.dir.p, 0, c->dir_entries * sizeof(QsDirEntry), c->stream));
        changed = true;
    }
    if (need_lms > G.cap_lms) {
        long long cap = G.cap_lms ? G.cap_lms : 1024;
        while (cap < need_lms) cap *= 2;
        HIPCHK(c, grow_array(G.lm_x, have_lms, cap, c->stream));
        HIPCHK(c, grow_array(G.lm_y, have_lms, cap, c->stream));
        HIPCHK(c, grow_array(G.lm_idx, have_lms, cap, c->stream));
        HIPCHK(c, grow_array(G.lm_type, have_lms, cap, c->stream));
        HIPCHK(c, grow_pool(c, G, G.cap_lms, cap));
        G.cap_lms = cap; changed = true;
    }
    if (need_cls > G.cap_cls) {
        long long cap = G.cap_cls ? G.cap_cls : 256;
        while (cap < need_cls) cap *= 2;
        HIPCHK(c, grow_array(G.cl_lm_idx, have_cls, cap, c->stream));
        HIPCHK(c, grow_array(G.cl_node_idx, have_cls, cap, c->stream));
        HIPCHK(c, grow_array(G.cl_dx, have_cls, cap, c->stream));
        HIPCHK(c, grow_array(G.cl_dy, have_cls, cap, c->stream));
        HIPCHK(c, grow_array(G.cl_agent, have_cls, cap, c->stream));
        G.cap_cls = cap; changed = true;
    }
    if (changed) {
        // the view: pointers and capacities from the arrays; the counters live on the device and are preserved
        QsGraphDev v;
        HIPCHK(c, hipMemcpyAsync(&v, c->d_graphs.p + g, sizeof v, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        v.cap_lms = G.cap_lms; v.cap_cls = G.cap_cls;
        v.lm_x = G.lm_x.p; v.lm_y = G.lm_y.p; v.lm_idx = G.lm_idx.p; v.lm_type = G.lm_type.p;
        v.cl_lm_idx = G.cl_lm_idx.p; v.cl_node_idx = G.cl_node_idx.p; v.cl_dx = G.cl_dx.p; v.cl_dy = G.cl_dy.p; v.cl_agent = G.cl_agent.p;
        v.dir = G.dir.p; v.nodes = G.nodes.p; v.nd_next = G.nd_next.p; v.misc = G.misc.p;
        v.node_cap = (long long)G.nodes.cap;
        if (!v.nodes_used) v.nodes_used = (unsigned int)(1 + c->dir_entries);
        HIPCHK(c, hipMemcpyAsync(c->d_graphs.p + g, &v, sizeof v, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return QS_OK;
}

static int reset_state(qs_ctx *c)
{
    HIPCHK(c, hipMemsetAsync(c->d_stamps.p, 0, c->cells * sizeof(unsigned int), c->stream));
    if (c->d_counts.p) HIPCHK(c, hipMemsetAsync(c->d_counts.p, 0, c->cells * sizeof(unsigned long long), c->stream));
    if (c->d_counts_fused.p) HIPCHK(c, hipMemsetAsync(c->d_counts_fused.p, 0, c->cells * sizeof(unsigned long long), c->stream));
    c->counts_view_fused = false;             // the views read the local counters until the session's first fuse
    c->dirty_since_fuse = false;
    if (c->d_dirty.p) HIPCHK(c, hipMemsetAsync(c->d_dirty.p, 0, c->dirty_words * sizeof(unsigned int), c->stream));
    if (c->d_counts_sent.p) HIPCHK(c, hipMemsetAsync(c->d_counts_sent.p, 0, c->cells * sizeof(unsigned long long), c->stream));
    c->sf_state = 0;
    HIPCHK(c, qs_launch_reset_small(c));      // drift, zone boxes, counters, per-graph batch counts, EKF state, flags: one launch
    // the bucket index of every graph: only what the session used of it (directory entries, first nodes,
    // pool nodes), found from the landmark log on the device; then the graphs' counters and the bots' last
    // closure (:271).  All enqueued: a reset does not wait for the GPU.
    HIPCHK(c, qs_launch_slam_reset_index(c));
    for (int g = 0; g < c->n_graphs; g++) { c->lms_upper[g] = 0; c->cls_upper[g] = 0; }
    c->next_seq = 0; c->epoch_base = 0; c->last_n = 0; c->last_has_poses = false; c->n_rebases = 0; c->edge_rays_total = 0;
    c->last_sweeps = false; c->last_sweeps_n = 0;
    c->pile_mode = false;
    c->edge_maybe = false; c->edge_overflow_total = 0;      // (rays still waiting belonged to the old session: the flags are cleared above)
    return QS_OK;
}

extern "C" int qs_create(const qs_config *cfg, qs_ctx **out)
{
    if (!cfg || !out) return qs_fail(nullptr, QS_E_INVAL, "qs_create: null argument");
    *out = nullptr;
    if (cfg->size < 4 || cfg->size % 4 != 0 || cfg->size > 32768)
        return qs_fail(nullptr, QS_E_INVAL, "qs_create: size must be a multiple of 4 in [4, 32768]");
    if (!(cfg->res > 0) || !isfinite(cfg->ox) || !isfinite(cfg->oy))
        return qs_fail(nullptr, QS_E_INVAL, "qs_create: bad resolution/origin");
    if (cfg->max_agent < 1 || cfg->max_agent > QS_MAX_AGENT)
        return qs_fail(nullptr, QS_E_INVAL, "qs_create: max_agent must be in [1, 255]");
    if (cfg->shard_bots < 0 || cfg->shard_rank < 0 || (cfg->shard_bots > 0 && (int64_t)cfg->shard_rank * cfg->shard_bots >= cfg->max_agent))
        return qs_fail(nullptr, QS_E_INVAL, "qs_create: shard_rank * shard_bots must lie below max_agent");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return qs_fail(nullptr, QS_E_NODEV, "qs_create: no HIP device (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return qs_fail(nullptr, QS_E_NODEV, "qs_create: bad device ordinal");

    qs_ctx *c = new qs_ctx();
    c->cfg = *cfg;
    c->device = cfg->device;
    c->bots_per_graph = cfg->bots_per_graph > 0 ? cfg->bots_per_graph : cfg->max_agent;
    c->n_graphs = (cfg->max_agent + c->bots_per_graph - 1) / c->bots_per_graph;
    c->win = cfg->min_poses_between < 1 ? 1 : (cfg->min_poses_between > QS_WIN_MAX ? QS_WIN_MAX : cfg->min_poses_between);
    c->r2_threshold = r2_threshold_for(cfg->closure_radius);
    c->cells = (size_t)cfg->size * cfg->size;
    c->geom = QsGeom{cfg->size, cfg->res, cfg->ox, cfg->oy, cfg->min_dist, cfg->max_dist, 1.0 / cfg->res};
    c->b.own_lo = cfg->shard_bots > 0 ? cfg->shard_rank * cfg->shard_bots + 1 : 1;      // the agents whose rays this context casts
    c->b.own_hi = cfg->shard_bots > 0 ? std::min(cfg->max_agent, (cfg->shard_rank + 1) * cfg->shard_bots) : cfg->max_agent;
    {   // landmark buckets: edge a hair above the closure radius, so that two points closer than the
        // radius are never two buckets apart whatever the rounding of (v - b0) / cell.  The directory is a
        // hash table over the cells, sized for one entry per cell of the configured world (2^20 at most).
        const double cell = cfg->closure_radius > 0 ? cfg->closure_radius * (1.0 + 1e-9) : 1.0;
        double nbd = ceil(cfg->size * cfg->res / cell) + 1.0;
        if (!(nbd >= 1)) nbd = 1;
        if (nbd > 1024) nbd = 1024;
        unsigned int slab = 256;
        while ((double)slab < nbd * nbd) slab <<= 1;
        c->bg = QsBucketGeom{cfg->ox, cfg->oy, cell, 1.0 / cell, slab - 1, 0};
        c->dir_entries = (size_t)QS_NTYPES * slab;
    }
    const int nb = cfg->max_agent + 1;
#define CREATE_CHK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { int rc__ = qs_fail(nullptr, QS_E_HIP, #x, e__); qs_destroy(c); return rc__; } } while (0)
    CREATE_CHK(hipSetDevice(c->device));
    CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
    CREATE_CHK(c->d_stamps.alloc(c->cells));
    if (cfg->enable_counts) CREATE_CHK(c->d_counts.alloc(c->cells));
    CREATE_CHK(c->d_offset.alloc(nb));
    CREATE_CHK(c->d_drift.alloc((size_t)nb * 2));
    CREATE_CHK(c->d_last_closure.alloc(nb));
    CREATE_CHK(c->d_zone.alloc((size_t)nb * 4));
    CREATE_CHK(c->d_counters.alloc(QS_CNT_N));
    CREATE_CHK(c->d_graph_batch.alloc((size_t)c->n_graphs * 2));
    CREATE_CHK(c->d_ekf.alloc((size_t)nb * 44));
    CREATE_CHK(c->d_ekf_prev.alloc((size_t)nb * 4));
    CREATE_CHK(c->d_flags.alloc(QS_N_FLAGS));
    CREATE_CHK(hipMemset(c->d_flags.p, 0, QS_N_FLAGS * sizeof(unsigned int)));
    CREATE_CHK(hipHostMalloc((void **)&c->h_chain_stat, 8 * sizeof(unsigned int), hipHostMallocDefault));
    memset(c->h_chain_stat, 0, 8 * sizeof(unsigned int));
    CREATE_CHK(hipEventCreateWithFlags(&c->ev_chain_stat, hipEventDisableTiming));
    if (const char *e = getenv("QS_CHAIN_MODE")) c->chain_form = strcmp(e, "window") == 0 ? QS_CHAIN_WINDOW : strcmp(e, "free") == 0 ? QS_CHAIN_FREE : strcmp(e, "free_posting") == 0 ? QS_CHAIN_FREE_POSTING : QS_CHAIN_AUTO;
    CREATE_CHK(c->d_graphs.alloc((size_t)c->n_graphs));
    CREATE_CHK(hipMemset(c->d_graphs.p, 0, (size_t)c->n_graphs * sizeof(QsGraphDev)));
    c->graphs.resize(c->n_graphs);
    c->lms_upper.assign(c->n_graphs, 0);
    c->cls_upper.assign(c->n_graphs, 0);
    std::vector<double> off(nb, 0.0);
    if (cfg->max_agent >= 2) off[2] = cfg->separation;                       // :851-852
    CREATE_CHK(hipMemcpy(c->d_offset.p, off.data(), nb * sizeof(double), hipMemcpyHostToDevice));
#undef CREATE_CHK
    for (int g = 0; g < c->n_graphs; g++) {
        int rc = graph_reserve(c, g, 1024, 256, 0, 0);
        if (rc != QS_OK) { g_create_err = c->err; qs_destroy(c); return rc; }
    }
    int rc = reset_state(c);
    if (rc != QS_OK) { g_create_err = c->err; qs_destroy(c); return rc; }
    *out = c;
    return QS_OK;
}

// The filter's stream keeps off the lowest 32 CUs.  Its kernels run beside the loop-closure chain, whose workgroups
// (one per pose graph, each a whole CU's worth of latency-bound waves) lose ~10 % when scan kernels share their
// SIMDs; with 32 CUs left alone the dispatcher puts the chain there (64 bots / 32 graphs: chain 1.26 -> 1.15 ms,
// step 1.89 -> 1.80 ms; tools/ekf_cu_mask_probe.sh).  QS_EKF_CU_MASK = hex words (lowest CUs first) overrides,
// "none" switches the mask off; a device too small for it, or a refusal, falls back to an ordinary stream.
// ONE masked stream per device, shared by its contexts (the last one destroys it): a second CU-masked queue on the same GPU
// slows every kernel of the process by 30-50 % (measured: two contexts, each with its own masked stream, 1.81 ->
// 2.79 ms per 64-bot step; tools/secondary_probe.py).  Contexts of one process then run their filters one after
// the other, which is how they are driven anyway (a caller serialises the calls on a context).
static hipStream_t g_masked[64] = {};       // per device: the CU-masked stream its contexts' filters run on
static int g_masked_users[64] = {};
static std::mutex g_masked_mutex;           // (contexts are independent: two threads may create / destroy theirs at the same time)

static int ekf_stream_acquire(qs_ctx *c)
{
    const char *mk = getenv("QS_EKF_CU_MASK");
    std::vector<uint32_t> words;
    if (mk && *mk && strcmp(mk, "none") != 0) {
        char *end = nullptr;
        for (const char *q = mk; *q;) { words.push_back((uint32_t)strtoul(q, &end, 16)); if (end == q) break; q = (*end == ',') ? end + 1 : end; }
    } else if (!mk || !*mk) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount >= 128) {
            words.assign((size_t)(prop.multiProcessorCount + 31) / 32, 0xffffffffu);
            words[0] = 0u;
        }
    }
    if (!words.empty() && c->device < 64) {
        std::lock_guard<std::mutex> lk(g_masked_mutex);
        if (!g_masked[c->device] && hipExtStreamCreateWithCUMask(&g_masked[c->device], (uint32_t)words.size(), words.data()) != hipSuccess) {
            (void)hipGetLastError();
            g_masked[c->device] = nullptr;
        }
        c->ekf_stream = g_masked[c->device];
        c->ekf_stream_shared = c->ekf_stream != nullptr;
        if (c->ekf_stream_shared) g_masked_users[c->device]++;
    }
    if (!c->ekf_stream)
        HIPCHK(c, hipStreamCreateWithFlags(&c->ekf_stream, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_decoded, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_ekf_done, hipEventDisableTiming));
    return QS_OK;
}

static void ekf_stream_release(qs_ctx *c)
{
    if (c->ekf_stream) {
        hipStreamSynchronize(c->ekf_stream);
        if (!c->ekf_stream_shared) hipStreamDestroy(c->ekf_stream);
        else if (c->device < 64) {
            std::lock_guard<std::mutex> lk(g_masked_mutex);
            if (--g_masked_users[c->device] == 0) {                          // the last context of the device takes the shared stream with it
                hipStreamDestroy(g_masked[c->device]);                       // (a profiler's exit handler trips over a CU-masked queue left behind)
                g_masked[c->device] = nullptr;
            }
        }
    }
    if (c->ev_decoded) hipEventDestroy(c->ev_decoded);
    if (c->ev_ekf_done) hipEventDestroy(c->ev_ekf_done);
}

extern "C" int qs_destroy(qs_ctx *c)
{
    if (!c) return QS_OK;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->h_chain_stat) hipHostFree(c->h_chain_stat);
    if (c->ev_chain_stat) hipEventDestroy(c->ev_chain_stat);
    for (auto &p : c->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    ekf_stream_release(c);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;                                      // (every device block is a DevBuf: they free themselves)
    return QS_OK;
}

extern "C" const char *qs_last_error(const qs_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

extern "C" int qs_set_stream(qs_ctx *c, void *hip_stream)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hip_stream) {
        if (c->own_stream) { hipStreamDestroy(c->stream); c->own_stream = false; }
        c->stream = (hipStream_t)hip_stream;
    } else if (!c->own_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return QS_OK;
}

extern "C" int qs_set_chain_form(qs_ctx *c, int form)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, form == QS_CHAIN_AUTO || form == QS_CHAIN_FREE || form == QS_CHAIN_WINDOW || form == QS_CHAIN_FREE_POSTING);
    c->chain_form = form;
    return QS_OK;
}

extern "C" int qs_chain_form(qs_ctx *c)
{
    if (!c) return QS_E_INVAL;
    return !c->chain_last_free ? QS_CHAIN_WINDOW : c->chain_last_posting ? QS_CHAIN_FREE_POSTING : QS_CHAIN_FREE;
}

extern "C" int qs_sync(qs_ctx *c)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_reset(qs_ctx *c)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    return reset_state(c);
}

extern "C" int qs_set_bot_offset(qs_ctx *c, int32_t bot, double off_x)
{
    ARGCHK(c, c != nullptr);
    if (bot < 1 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_set_bot_offset: bot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->d_offset.p + bot, &off_x, sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

// ---- timing (StageTimer: qs_internal.h) -----------------------------------------------------------
extern "C" int qs_timing_enable(qs_ctx *c, int32_t enable)
{
    ARGCHK(c, c != nullptr);
    c->timing = enable != 0;
    return QS_OK;
}

extern "C" int qs_stage_times(qs_ctx *c, double ms[QS_STAGE_N], uint64_t launches[QS_STAGE_N], int32_t reset)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &p : c->pending) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) { c->stage_ms[p.stage] += t; c->stage_launches[p.stage]++; }
        c->ev_pool.push_back(p.a); c->ev_pool.push_back(p.b);
    }
    c->pending.clear();
    for (int s = 0; s < QS_STAGE_N; s++) { if (ms) ms[s] = c->stage_ms[s]; if (launches) launches[s] = c->stage_launches[s]; }
    if (reset) for (int s = 0; s < QS_STAGE_N; s++) { c->stage_ms[s] = 0; c->stage_launches[s] = 0; }
    return QS_OK;
}

// ---- batch buffers --------------------------------------------------------------------------
// the arrays of QsBatch and QsSlamBatch for cap records, carved from base (nullptr: only the size); returns the bytes
static size_t batch_layout(const qs_ctx *c, void *base, size_t cap, QsBatch &b, QsSlamBatch &sb)
{
    const size_t nblk = (size_t)qs_slam_blocks(cap), G = (size_t)c->n_graphs, nb = (size_t)c->cfg.max_agent + 2;
    Carve k(base);
    b.accept = k.take<unsigned char>(cap);
    b.map_ok = c->cfg.shard_bots > 0 ? k.take<unsigned char>(cap) : b.accept;     // an array of its own only in a shard
    b.agent = k.take<unsigned char>(cap); b.lm = k.take<unsigned char>(cap);
    b.px = k.take<double>(cap); b.py = k.take<double>(cap); b.yaw = k.take<double>(cap);
    b.dist = k.take<float4>(cap); b.enc = k.take<int>(cap);
    b.rx = k.take<double>(cap); b.ry = k.take<double>(cap);
    b.hit = k.take<double2>(4 * cap); b.hit_valid = k.take<unsigned char>(4 * cap);
    sb.node = k.take<long long>(cap); sb.ev_node = k.take<long long>(cap);
    sb.ev_agent = k.take<unsigned char>(cap); sb.ev_type = k.take<unsigned char>(cap);
    sb.ev_px = k.take<double>(cap); sb.ev_py = k.take<double>(cap);
    sb.ev_base = k.take<unsigned int>(G + 1); sb.acc_total = k.take<unsigned int>(G);
    sb.blk_acc = k.take<unsigned int>(G * nblk); sb.blk_ev = k.take<unsigned int>(G * nblk);
    sb.agent_ev = k.take<unsigned int>(nb); sb.acl_cnt = k.take<unsigned int>(nb);
    sb.acl_node = k.take<long long>(cap); sb.acl_dx = k.take<double>(cap); sb.acl_dy = k.take<double>(cap);
    sb.drift_start = k.take<double>(2 * nb);
    return k.bytes;
}

// room for n records; a growth that fails leaves the old arrays as they were
static int ensure_batch(qs_ctx *c, size_t n)
{
    if (n <= c->cap_batch) return QS_OK;
    size_t cap = c->cap_batch ? c->cap_batch : 1024;
    while (cap < n) cap *= 2;
    QsBatch b = c->b;
    QsSlamBatch sb = c->sb;
    DevBuf<char> slab;
    HIPCHK(c, slab.alloc(batch_layout(c, nullptr, cap, b, sb)));
    batch_layout(c, slab.p, cap, b, sb);
    if (c->cfg.exact_trig) {
        if (!c->d_edge.p) HIPCHK(c, c->d_edge.alloc(QS_EDGE_CAP));
        b.edge = c->d_edge.p; b.edge_n = c->d_flags.p; b.edge_cap = QS_EDGE_CAP;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));              // (the old arrays may still be in use)
    c->batch_ws = std::move(slab);
    c->b = b; c->sb = sb;
    c->cap_batch = cap;
    return QS_OK;
}

// Stamp ordinals are 30 bits (so stamps stay below 2^31 and an int32 MAX all-reduce is valid).
static const uint64_t QS_EPOCH_LIMIT = (1ull << 28) - 2;
static bool epoch_would_rebase(const qs_ctx *c, uint64_t seq0, size_t n_seq)
{
    return seq0 + n_seq - c->epoch_base > QS_EPOCH_LIMIT;
}
static int ensure_epoch(qs_ctx *c, uint64_t seq0, size_t n_seq)
{
    if (seq0 < c->epoch_base) return qs_fail(c, QS_E_INVAL, "seq0 precedes the current stamp epoch (sequence numbers must not decrease)");
    if (n_seq > QS_EPOCH_LIMIT) return qs_fail(c, QS_E_RANGE, "batch too large for one stamp epoch (2^28 records)");
    if (epoch_would_rebase(c, seq0, n_seq)) {
        // A rebase collapses every written cell to ordinal 1.  In one mapper that keeps the order against all later
        // writes; in a shard -- of a round-robin stream (seq_stride > 1) or of a replicated pose graph (shard_bots > 0:
        // every rank sees every packet but casts only its own agents' rays) -- two ranks' unfused writes to one cell
        // would tie afterwards, so the shards must have exchanged their stamps first (dist.ShardedMapper does: it asks
        // qs_epoch_query before every ingest).
        if ((c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0) && c->dirty_since_fuse)
            return qs_fail(c, QS_E_STATE, "this batch crosses a stamp epoch: fuse the shards' grids (all-reduce + qs_mark_fused) first");
        { int rcf = flush_edge_rays(c); if (rcf != QS_OK) return rcf; }     // waiting rays carry stamps of the epoch that ends here
        HIPCHK(c, qs_launch_rebase(c));
        c->epoch_base = seq0 ? seq0 - 1 : 0;
        c->n_rebases++;
    }
    return QS_OK;
}

extern "C" int qs_epoch_query(qs_ctx *c, uint64_t seq0, size_t n, int32_t *would_rebase)
{
    ARGCHK(c, c != nullptr && would_rebase != nullptr);
    if (seq0 == UINT64_MAX) seq0 = c->next_seq;
    const uint64_t sstride = c->cfg.seq_stride > 0 ? (uint64_t)c->cfg.seq_stride : 1;
    *would_rebase = (n > 0 && epoch_would_rebase(c, seq0 - seq0 % sstride, n * sstride)) ? 1 : 0;
    return QS_OK;
}

extern "C" int qs_mark_fused(qs_ctx *c)
{
    ARGCHK(c, c != nullptr);
    c->dirty_since_fuse = false;
    return QS_OK;
}

static int reserve_graphs_for_batch(qs_ctx *c, size_t n)
{
    bool need_sync = false;
    for (int g = 0; g < c->n_graphs; g++)
        if (c->lms_upper[g] + (long long)n > c->graphs[g].cap_lms || c->cls_upper[g] + (long long)n > c->graphs[g].cap_cls)
            need_sync = true;
    if (!need_sync) {
        for (int g = 0; g < c->n_graphs; g++) { c->lms_upper[g] += (long long)n; c->cls_upper[g] += (long long)n; }
        return QS_OK;
    }
    // The batch's landmark events per graph are known on the device only.  Asking costs a host sync in the
    // middle of the pipeline (every launch after the decode waits for it), so when memory allows, the graphs
    // that are short are simply grown to the safe bound -- every record a landmark of that graph -- and the
    // next batches of this size go through without a question: ~260 B per unit of capacity (log, closures,
    // side list, worst-case node pool), against 288 GB.
    {
        const double unit = 2 * 8 + 8 + 1 + 2 * 8 + 2 * 8 + 4 + sizeof(QsLmNode) + 4;
        double extra = 0;
        for (int g = 0; g < c->n_graphs; g++) {
            const long long nl = c->lms_upper[g] + (long long)n, nc = c->cls_upper[g] + (long long)n;
            if (nl > c->graphs[g].cap_lms) extra += (double)(2 * nl - c->graphs[g].cap_lms) * unit;     // (capacities double)
            if (!c->graphs[g].nodes.p) extra += (double)(1 + c->dir_entries) * (sizeof(QsLmNode) + 4 + sizeof(QsDirEntry));   // first nodes
            if (nc > c->graphs[g].cap_cls) extra += (double)(2 * nc - c->graphs[g].cap_cls) * 32.0;
        }
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && extra <= 0.25 * (double)free_b) {
            for (int g = 0; g < c->n_graphs; g++) {
                const long long nl = c->lms_upper[g] + (long long)n, nc = c->cls_upper[g] + (long long)n;
                int rc = graph_reserve(c, g, nl, nc, c->lms_upper[g], c->cls_upper[g]);
                if (rc != QS_OK) return rc;
                c->lms_upper[g] = nl; c->cls_upper[g] = nc;
            }
            return QS_OK;
        }
    }
    // tighten the bounds with the exact device-side numbers, then grow what is really short
    std::vector<QsGraphDev> cur(c->n_graphs);
    std::vector<unsigned long long> gb((size_t)c->n_graphs * 2);
    HIPCHK(c, hipMemcpyAsync(cur.data(), c->d_graphs.p, cur.size() * sizeof(QsGraphDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(gb.data(), c->d_graph_batch.p, gb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int g = 0; g < c->n_graphs; g++) {
        const long long ev = (long long)gb[2 * g + 1];
        const long long need_l = cur[g].n_lms + ev, need_c = cur[g].n_cls + ev;
        int rc = graph_reserve(c, g, need_l, need_c, cur[g].n_lms, cur[g].n_cls);
        if (rc != QS_OK) return rc;
        c->lms_upper[g] = need_l; c->cls_upper[g] = need_c;
    }
    return QS_OK;
}

// Exact-trig mode (qs_config.exact_trig, default on): rays the device did not decide (raycast_common.h, qs_edge_ray) wait in
// a list of self-contained records (pose, distance, stamp) and get their end points from libm here -- math.cos / math.sin of
// the reference are glibc's -- before they are cast with the stamps their ingest gave them (stamps make the order
// irrelevant).  An ingest does not wait for this: the list is flushed at the next point where the map can be OBSERVED (any
// call that reads or hands out the grid, the counters or the pose graphs; qs_sync; before a stamp rebase) and dropped by
// qs_reset.  The same synchronisation brings the graphs' real landmark / closure counts (capacity planning starts from them,
// not from "every record so far was a landmark") and the pile flag of the loop-closure chain.
// Which instantiation of the free-running loop-closure chain suits the stream (slam.hip, qs_launch_slam): with or without the
// owners posting their landmarks' poses.  The kernels keep running totals in device words (decisions that had to wait for the
// committer / scans of the posted poses; closures); every ingest asks for a copy of them into pinned memory behind itself and
// looks, before it launches its own chain, at whatever copy has landed by then -- nobody waits.  More than 1 in 8: posting on;
// fewer than 1 in 16: off again (both instantiations count the same events); more scans than closures even so (a stream
// that hardly ever matches: the adversarial one spread over an 8192^2 world): the per-window kernel, until its queries
// that find nothing are fewer than half its closures.
static void chain_stats_poll(qs_ctx *c, bool synced, const unsigned int *fresh)
{
    // fresh: the four totals as a synchronising call has just read them (newer than any copy in flight, which has landed too)
    if (!fresh && !c->chain_stat_pending) return;
    if (!fresh && !synced && hipEventQuery(c->ev_chain_stat) != hipSuccess) { (void)hipGetLastError(); return; }
    c->chain_stat_pending = false;
    unsigned int *now = c->h_chain_stat, *seen = c->h_chain_stat + 4;
    if (fresh) for (int i = 0; i < 4; i++) now[i] = fresh[i];
    const uint64_t f_miss = now[0] - seen[0], f_hit = now[1] - seen[1], w_miss = now[2] - seen[2], w_hit = now[3] - seen[3];
    if (c->chain_windowed) { if (w_miss + w_hit >= 256 && w_miss * 2 < w_hit) c->chain_windowed = false; }   // (back to posting)
    else if (f_miss + f_hit >= 256) {
        if (!c->chain_posting) { if (f_miss * 8 > f_hit) c->chain_posting = true; }
        else if (f_miss > f_hit) c->chain_windowed = true;   // more scans than closures: the per-window kernel's LDS windows are cheaper
        else if (f_miss * 16 < f_hit) c->chain_posting = false;
    }
    for (int i = 0; i < 4; i++) seen[i] = now[i];
}
static int chain_stats_request(qs_ctx *c)
{
    if (c->chain_stat_pending) return QS_OK;                 // (the copy in flight will do)
    // one ingest in four: the copy is a blit kernel with a barrier either side (~20 us of a 1.4 ms step when the stream is
    // 64 bots), and what it carries only ever changes the choice of an instantiation
    if ((c->chain_stat_tick++ & 3u) != 0) return QS_OK;
    HIPCHK(c, hipMemcpyAsync(c->h_chain_stat, c->d_flags.p + QS_FLAG_CHAIN_MISS, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_chain_stat, c->stream));
    c->chain_stat_pending = true;
    return QS_OK;
}

static int flush_edge_rays(qs_ctx *c)
{
    if (!c->edge_maybe && !c->flags_maybe) return QS_OK;
    unsigned int fl[QS_N_FLAGS] = {0};
    HIPCHK(c, hipMemcpyAsync(fl, c->d_flags.p, sizeof fl, hipMemcpyDeviceToHost, c->stream));
    std::vector<QsGraphDev> cur((size_t)c->n_graphs);
    HIPCHK(c, hipMemcpyAsync(cur.data(), c->d_graphs.p, cur.size() * sizeof(QsGraphDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->edge_maybe = false; c->flags_maybe = false;
    for (int g = 0; g < c->n_graphs; g++) { c->lms_upper[g] = cur[g].n_lms; c->cls_upper[g] = cur[g].n_cls; }
    if (fl[QS_FLAG_PILE]) c->pile_mode = true;           // a landmark pile has formed: the chain kernel's DENSE variant from now on
    chain_stats_poll(c, true, fl + QS_FLAG_CHAIN_MISS);
    const unsigned int n_edge = fl[QS_FLAG_EDGE_N] < QS_EDGE_CAP ? fl[QS_FLAG_EDGE_N] : QS_EDGE_CAP;
    c->edge_overflow_total += fl[QS_FLAG_EDGE_OVF];
    if (n_edge == 0) return QS_OK;
    c->edge_rays_total += n_edge;
    std::vector<QsEdgeRec> recs(n_edge);
    HIPCHK(c, hipMemcpy(recs.data(), c->d_edge.p, (size_t)n_edge * sizeof(QsEdgeRec), hipMemcpyDeviceToHost));
    const size_t bytes = (size_t)n_edge * 4 * sizeof(double);
    HIPCHK(c, c->io_ws.reserve(bytes, c->stream, QS_IO_WS_FLOOR));
    double *d = (double *)c->io_ws.p;
    std::vector<double> h((size_t)n_edge * 4);
    static const double kPi = 3.141592653589793;                                              // math.pi
    static const double off[4] = {0.0, kPi / 2, kPi, -kPi / 2};                               // :61-66
    for (unsigned int e = 0; e < n_edge; e++) {
        const QsEdgeRec &r = recs[e];
        const double dd = (double)r.d;
        const bool sweep = r.beam >= 0;                                                        // a servo-sweep beam (sweep.hip)
        const int sensor = (int)(((r.key_free >> 1) - 1) & 3);                                 // ordinal = 4 * arrival index + sensor + 1
        const double a = sweep ? r.yaw + (double)(r.beam - 90) * (kPi / 180.0)                 // math.radians(i - 90)
                               : r.yaw + off[sensor];                                          // :887
        const double lo = sweep ? c->sweep_min : c->cfg.min_dist, hi = sweep ? c->sweep_max : c->cfg.max_dist;
        const bool valid = (lo < dd) && (dd <= hi);                                            // :888
        const double range = valid ? dd : ((dd > lo) ? ((hi < dd) ? hi : dd) : hi);            // :900
        h[4 * e] = r.rx + range * cos(a);                                                      // :890 / :901
        h[4 * e + 1] = r.ry + range * sin(a);                                                  // :891 / :902
        h[4 * e + 2] = valid ? 1.0 : 0.0;
        h[4 * e + 3] = 0.0;
    }
    HIPCHK(c, hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_edge_cast(c, n_edge, d));
    HIPCHK(c, hipMemsetAsync(c->d_flags.p, 0, sizeof(unsigned int), c->stream));                 // the list is empty again
    HIPCHK(c, hipMemsetAsync(c->d_flags.p + 2, 0, sizeof(unsigned int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                                // h goes out of scope
    return QS_OK;
}

// at a point where the host waits for the stream anyway: the chain's flags (pile, form statistics)
static int read_pile_flag(qs_ctx *c)
{
    c->flags_maybe = true;
    return flush_edge_rays(c);
}

static int ingest_device(qs_ctx *c, const uint8_t *d_pkts, size_t n, size_t stride, const uint16_t *d_lens,
                         const double *d_time, uint64_t seq0)
{
    if (seq0 == UINT64_MAX) seq0 = c->next_seq;
    c->last_n = n; c->last_has_poses = true; c->last_sweeps = false;
    if (n == 0) return QS_OK;
    int rc = ensure_batch(c, n);
    if (rc != QS_OK) return rc;
    c->b.n = n;
    const uint64_t sstride = c->cfg.seq_stride > 0 ? (uint64_t)c->cfg.seq_stride : 1;
    // epoch decisions use the stride-aligned range so that all ranks of a sharded stream agree
    rc = ensure_epoch(c, seq0 - seq0 % sstride, n * sstride);
    if (rc != QS_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_graph_batch.p, 0, (size_t)c->n_graphs * 2 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->sb.agent_ev, 0, ((size_t)c->cfg.max_agent + 2) * sizeof(unsigned int), c->stream));
    { StageTimer t(c, QS_STAGE_DECODE); HIPCHK(c, qs_launch_decode(c, d_pkts, n, stride, d_lens)); t.stop(); }
    rc = reserve_graphs_for_batch(c, n);
    if (rc != QS_OK) return rc;
    if (c->cfg.enable_ekf) {
        // fork: the filter only needs the decoded fields, never the map (and the map never the filter)
        if (!c->ekf_stream) { int rce = ekf_stream_acquire(c); if (rce != QS_OK) return rce; }
        HIPCHK(c, hipEventRecord(c->ev_decoded, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->ekf_stream, c->ev_decoded, 0));
        { StageTimer t(c, QS_STAGE_EKF, c->ekf_stream); HIPCHK(c, n >= QS_EKF_SCAN_MIN_BATCH ? qs_launch_ekf_scan(c, n, d_time, c->ekf_stream)
                                                   : qs_launch_ekf_ingest(c, n, d_time, c->ekf_stream)); t.stop(); }
        HIPCHK(c, hipEventRecord(c->ev_ekf_done, c->ekf_stream));
    }
    chain_stats_poll(c, false, nullptr);
    { StageTimer t(c, QS_STAGE_SLAM); HIPCHK(c, qs_launch_slam(c, n)); t.stop(); }
    { int rcs = chain_stats_request(c); if (rcs != QS_OK) return rcs; }
    {
        StageTimer t(c, QS_STAGE_RAYCAST);
        // auto (0): a handful of packets (the live UDP path: <= 20 per frame) is one direct kernel instead
        // of the four tiled passes -- same cells either way; 1 = always direct, 2 = always tiled
        if (c->cfg.raycast_mode == 1 || (c->cfg.raycast_mode == 0 && n <= QS_DIRECT_MAX_BATCH))
            HIPCHK(c, qs_launch_raycast_direct(c, n, seq0));
        else HIPCHK(c, qs_launch_raycast_tiled(c, n, seq0));
        t.stop();
    }
    if (c->cfg.enable_ekf) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ekf_done, 0));   // join
    if (c->b.edge) c->edge_maybe = true;                 // resolved at the next point the map is observed (flush_edge_rays)
    c->flags_maybe = true;
    c->next_seq = seq0 + n * sstride;
    c->dirty_since_fuse = true;
    return QS_OK;
}

extern "C" int qs_ingest_device(qs_ctx *c, const uint8_t *d_pkts, size_t n, size_t stride, const uint16_t *d_lens,
                                const double *d_time, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (d_pkts != nullptr && stride >= QS_PACKET_SIZE_V1));
    HIPCHK(c, hipSetDevice(c->device));
    return ingest_device(c, d_pkts, n, stride, d_lens, d_time, seq0);
}

// device staging of host-side records: bytes of records, one length and one receive time per (shortest) record
struct Staging { unsigned char *pkts; unsigned short *lens; double *time; };
static size_t staging_layout(void *base, size_t cap, Staging &s)
{
    Carve k(base);
    s.pkts = k.take<unsigned char>(cap);
    s.lens = k.take<unsigned short>(cap / QS_PACKET_SIZE_V1 + 1);
    s.time = k.take<double>(cap / QS_PACKET_SIZE_V1 + 1);
    return k.bytes;
}

// staging for `bytes` of records, laid out for the smallest power-of-two multiple of 64 KiB that holds them (the block
// only grows: the layout of a larger multiple needs more bytes)
static int reserve_staging(qs_ctx *c, size_t bytes, Staging &s)
{
    size_t cap = (size_t)1 << 16;
    while (cap < bytes) cap *= 2;
    HIPCHK(c, c->stage_ws.reserve(staging_layout(nullptr, cap, s), c->stream));
    staging_layout(c->stage_ws.p, cap, s);
    return QS_OK;
}

extern "C" int qs_ingest(qs_ctx *c, const uint8_t *pkts, size_t n, size_t stride, const uint16_t *lens,
                         const double *recv_time, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pkts != nullptr && stride >= QS_PACKET_SIZE_V1));
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) { c->last_n = 0; return QS_OK; }
    const size_t bytes = n * stride;
    Staging s;
    { int rcs = reserve_staging(c, bytes, s); if (rcs != QS_OK) return rcs; }
    HIPCHK(c, hipMemcpyAsync(s.pkts, pkts, bytes, hipMemcpyHostToDevice, c->stream));
    if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens, n * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    if (recv_time) HIPCHK(c, hipMemcpyAsync(s.time, recv_time, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int rc = ingest_device(c, s.pkts, n, stride, lens ? s.lens : nullptr, recv_time ? s.time : nullptr, seq0);
    if (rc != QS_OK) return rc;
    // this call waits for the GPU anyway (the caller's buffers are free when it returns): the waiting edge rays are resolved
    // now, and the graphs' real landmark / closure counts and the pile flag come along
    if (c->cfg.exact_trig) c->edge_maybe = true;
    return read_pile_flag(c);
}

extern "C" int qs_last_batch(qs_ctx *c, uint8_t *accepted, double *pose, size_t n)
{
    ARGCHK(c, c != nullptr);
    if (!c->last_has_poses || n != c->last_n) return qs_fail(c, QS_E_INVAL, "qs_last_batch: n does not match the last ingest");
    if (n == 0) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint8_t> acc(n);
    HIPCHK(c, hipMemcpyAsync(acc.data(), c->b.accept, n, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> rx, ry, yaw;
    if (pose) {
        rx.resize(n); ry.resize(n); yaw.resize(n);
        HIPCHK(c, hipMemcpyAsync(rx.data(), c->b.rx, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(ry.data(), c->b.ry, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(yaw.data(), c->b.yaw, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++) {
        if (accepted) accepted[i] = acc[i];
        if (pose) {
            pose[3 * i] = acc[i] ? rx[i] : NAN; pose[3 * i + 1] = acc[i] ? ry[i] : NAN; pose[3 * i + 2] = acc[i] ? yaw[i] : NAN;
        }
    }
    return QS_OK;
}

extern "C" int qs_last_hits(qs_ctx *c, double *xy, uint8_t *valid, size_t n)
{
    ARGCHK(c, c != nullptr && xy != nullptr && valid != nullptr);
    if (!c->last_has_poses || n != c->last_n) return qs_fail(c, QS_E_INVAL, "qs_last_hits: n does not match the last ingest");
    if (n == 0) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint8_t> acc(n);
    HIPCHK(c, qs_launch_hits(c, n));
    HIPCHK(c, hipMemcpyAsync(acc.data(), c->b.accept, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(xy, c->b.hit, 4 * n * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(valid, c->b.hit_valid, 4 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++)
        if (!acc[i]) for (int s = 0; s < 4; s++) valid[4 * i + s] = 0;
    return QS_OK;
}

// ---- servo sweeps (sweep.hip; semantics in include/quasar_slam.h) ----------------------------------------------------------
// Records per chunk: the tiled raycast's ray slots (8 B) and tile records (up to 4 x 8 B) of one chunk, 184 slots per
// record, stay under 0.5 GiB; the host path stages one chunk's records at a time.
static const size_t QS_SWEEP_CHUNK = (size_t)1 << 16;

static int sweeps_begin(qs_ctx *c, size_t n, size_t stride, uint64_t &seq0)
{
    if (stride != QS_SWEEP_SIZE_V0 && stride != QS_SWEEP_SIZE_V0_ODO)
        return qs_fail(c, QS_E_INVAL, "qs_ingest_sweeps: stride must be 743 (v0) or 751 (v0 + odometry)");
    if (c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0)
        return qs_fail(c, QS_E_INVAL, "qs_ingest_sweeps: sharded contexts (seq_stride > 1, shard_bots > 0) do not take sweeps");
    HIPCHK(c, hipSetDevice(c->device));
    if (seq0 == UINT64_MAX) seq0 = c->next_seq;
    c->last_n = 0; c->last_has_poses = false;              // qs_last_batch / qs_last_hits: length mismatch from here on
    c->last_sweeps = false; c->last_sweeps_n = 0;
    if (n == 0) return QS_OK;
    int rc = ensure_batch(c, 1);                           // the exact-trig waiting list lives with the batch buffers
    if (rc != QS_OK) return rc;
    HIPCHK(c, c->sweep_acc.reserve(n, c->stream, 1024));
    HIPCHK(c, c->sweep_pose.reserve(3 * n, c->stream, 3 * 1024));
    HIPCHK(c, c->sweep_hv.reserve(QS_SWEEP_SLOTS * std::min(n, QS_SWEEP_CHUNK), c->stream));
    return QS_OK;
}

// records [k0, k0 + m) of the call, at d_pkts (already offset to record k0)
static int sweeps_chunk(qs_ctx *c, const uint8_t *d_pkts, size_t m, size_t stride, const uint16_t *d_lens, uint64_t seq0, size_t k0)
{
    const uint64_t s0 = seq0 + (uint64_t)QS_SWEEP_SEQS * k0;
    int rc = ensure_epoch(c, s0, QS_SWEEP_SEQS * m);
    if (rc != QS_OK) return rc;
    // auto: by ray slots, as the 4-ray path decides by its 4 rays per packet
    const bool tiled = c->cfg.raycast_mode == 2 || (c->cfg.raycast_mode == 0 && QS_SWEEP_SLOTS * m > 4 * (size_t)QS_DIRECT_MAX_BATCH);
    StageTimer t(c, QS_STAGE_RAYCAST);
    HIPCHK(c, qs_launch_sweeps(c, d_pkts, m, stride, d_lens, s0, tiled, c->sweep_acc.p + k0, c->sweep_pose.p + 3 * k0, c->sweep_hv.p));
    t.stop();
    c->dirty_since_fuse = true;
    return QS_OK;
}

static void sweeps_end(qs_ctx *c, size_t n, uint64_t seq0)
{
    if (c->b.edge) c->edge_maybe = true;                   // resolved at the next point the map is observed (flush_edge_rays)
    c->next_seq = seq0 + (uint64_t)QS_SWEEP_SEQS * n;
    c->last_sweeps = true; c->last_sweeps_n = n;
}

extern "C" int qs_ingest_sweeps_device(qs_ctx *c, const uint8_t *d_pkts, size_t n, size_t stride, const uint16_t *d_lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || d_pkts != nullptr);
    int rc = sweeps_begin(c, n, stride, seq0);
    if (rc != QS_OK || n == 0) return rc;
    for (size_t k0 = 0; k0 < n; k0 += QS_SWEEP_CHUNK) {
        const size_t m = std::min(QS_SWEEP_CHUNK, n - k0);
        rc = sweeps_chunk(c, d_pkts + k0 * stride, m, stride, d_lens ? d_lens + k0 : nullptr, seq0, k0);
        if (rc != QS_OK) return rc;
    }
    sweeps_end(c, n, seq0);
    return QS_OK;
}

extern "C" int qs_ingest_sweeps(qs_ctx *c, const uint8_t *pkts, size_t n, size_t stride, const uint16_t *lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || pkts != nullptr);
    int rc = sweeps_begin(c, n, stride, seq0);
    if (rc != QS_OK || n == 0) return rc;
    for (size_t k0 = 0; k0 < n; k0 += QS_SWEEP_CHUNK) {
        const size_t m = std::min(QS_SWEEP_CHUNK, n - k0);
        Staging s;
        rc = reserve_staging(c, m * stride, s);            // (stream-ordered: the previous chunk's kernels have read theirs)
        if (rc != QS_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, m * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, m * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        rc = sweeps_chunk(c, s.pkts, m, stride, lens ? s.lens : nullptr, seq0, k0);
        if (rc != QS_OK) return rc;
    }
    sweeps_end(c, n, seq0);
    // as qs_ingest: the call waits for the GPU anyway, so the waiting edge beams are resolved now
    return read_pile_flag(c);
}

extern "C" int qs_last_sweeps(qs_ctx *c, uint8_t *accepted, double *pose, size_t n)
{
    ARGCHK(c, c != nullptr);
    if (!c->last_sweeps || n != c->last_sweeps_n) return qs_fail(c, QS_E_INVAL, "qs_last_sweeps: n does not match the last sweep ingest");
    if (n == 0) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint8_t> acc(n);
    std::vector<double> p(pose ? 3 * n : 0);
    HIPCHK(c, hipMemcpyAsync(acc.data(), c->sweep_acc.p, n, hipMemcpyDeviceToHost, c->stream));
    if (pose) HIPCHK(c, hipMemcpyAsync(p.data(), c->sweep_pose.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++) {
        if (accepted) accepted[i] = acc[i];
        if (pose) for (int q = 0; q < 3; q++) pose[3 * i + q] = acc[i] ? p[3 * i + q] : NAN;
    }
    return QS_OK;
}

extern "C" int qs_set_sweep_filter(qs_ctx *c, double smin, double smax)
{
    ARGCHK(c, c != nullptr);
    if (!(isfinite(smin) && isfinite(smax) && smin >= 0 && smin < smax))
        return qs_fail(c, QS_E_INVAL, "qs_set_sweep_filter: need finite 0 <= smin < smax");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = flush_edge_rays(c);                           // waiting beams are resolved with the filter they were cast with
    if (rc != QS_OK) return rc;
    c->sweep_min = smin; c->sweep_max = smax;
    return QS_OK;
}

// ---- OccupancyGrid object API ---------------------------------------------------------------
extern "C" int qs_update_rays(qs_ctx *c, const double *rx, const double *ry, const double *hx, const double *hy,
                              const uint8_t *valid, size_t n, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    if (n == 0) return QS_OK;
    ARGCHK(c, rx && ry && hx && hy && valid);
    HIPCHK(c, hipSetDevice(c->device));
    if (seq0 == UINT64_MAX) seq0 = c->next_seq;
    const size_t n_seq = (n + 3) / 4;
    int rc = ensure_epoch(c, seq0, n_seq);
    if (rc != QS_OK) return rc;
    // staging lives with the context (grown on demand): the object API's update_ray is one ray per call
    HIPCHK(c, c->io_ws.reserve(4 * n * sizeof(double) + n, c->stream, QS_IO_WS_FLOOR));
    double *d = (double *)c->io_ws.p; unsigned char *dv = (unsigned char *)(d + 4 * n);
    const double *src[4] = {rx, ry, hx, hy};
    for (int q = 0; q < 4; q++)
        HIPCHK(c, hipMemcpyAsync(d + q * n, src[q], n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dv, valid, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_update_rays(c, d, d + n, d + 2 * n, d + 3 * n, dv, n, seq0));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dirty_since_fuse = true;
    c->next_seq = seq0 + n_seq;
    c->last_has_poses = false; c->last_sweeps = false;
    return QS_OK;
}

extern "C" int qs_world_to_grid(qs_ctx *c, const double *w, size_t n, int32_t axis, int64_t *out)
{
    ARGCHK(c, c != nullptr);
    if (n == 0) return QS_OK;
    ARGCHK(c, w && out);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> d; DevBuf<long long> o;
    HIPCHK(c, d.alloc(n));
    HIPCHK(c, o.alloc(n));
    HIPCHK(c, hipMemcpyAsync(d.p, w, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_world_to_grid(c, d.p, n, axis, o.p));
    HIPCHK(c, hipMemcpyAsync(out, o.p, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_grid_i8_device(qs_ctx *c, int8_t *out_dev)
{
    ARGCHK(c, c != nullptr && out_dev != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    HIPCHK(c, qs_launch_view_i8(c, (signed char *)out_dev));
    return QS_OK;
}

extern "C" int qs_grid_i8(qs_ctx *c, int8_t *out_host)
{
    ARGCHK(c, c != nullptr && out_host != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    DevBuf<signed char> d;
    HIPCHK(c, d.alloc(c->cells));
    HIPCHK(c, qs_launch_view_i8(c, d.p));
    HIPCHK(c, hipMemcpyAsync(out_host, d.p, c->cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_grid_counts(qs_ctx *c, int32_t *hits_host, int32_t *misses_host)
{
    ARGCHK(c, c != nullptr && hits_host && misses_host);
    if (!c->d_counts.p) return qs_fail(c, QS_E_INVAL, "qs_grid_counts: context created with enable_counts = 0");
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    DevBuf<int> d;
    HIPCHK(c, d.alloc(2 * c->cells));
    HIPCHK(c, qs_launch_split_counts(c, d.p, d.p + c->cells));
    HIPCHK(c, hipMemcpyAsync(hits_host, d.p, c->cells * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(misses_host, d.p + c->cells, c->cells * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_grid_logodds(qs_ctx *c, float l_occ, float l_free, float lmin, float lmax, float *out_host)
{
    ARGCHK(c, c != nullptr && out_host);
    if (!c->d_counts.p) return qs_fail(c, QS_E_INVAL, "qs_grid_logodds: context created with enable_counts = 0");
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    DevBuf<float> d;
    HIPCHK(c, d.alloc(c->cells));
    HIPCHK(c, qs_launch_logodds(c, l_occ, l_free, lmin, lmax, d.p));
    HIPCHK(c, hipMemcpyAsync(out_host, d.p, c->cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_device_buffers(qs_ctx *c, void **stamps_dev, size_t *stamps_bytes, void **counts_dev, size_t *counts_bytes)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);                                   // whoever gets the buffers may read them (a collective)
    if (stamps_dev) *stamps_dev = c->d_stamps.p;
    if (stamps_bytes) *stamps_bytes = c->cells * sizeof(unsigned int);
    if (counts_dev) *counts_dev = c->d_counts.p;
    if (counts_bytes) *counts_bytes = c->d_counts.p ? c->cells * sizeof(unsigned long long) : 0;
    return QS_OK;
}

// ---- SLAM state -------------------------------------------------------------------------------
static int read_graph(qs_ctx *c, int32_t graph, QsGraphDev &g)
{
    if (graph < 0 || graph >= c->n_graphs) return qs_fail(c, QS_E_RANGE, "graph index out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(&g, c->d_graphs.p + graph, sizeof g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->lms_upper[graph] = g.n_lms; c->cls_upper[graph] = g.n_cls;      // exact now: nothing is in flight
    return QS_OK;
}

extern "C" int qs_slam_sizes(qs_ctx *c, int32_t graph, int64_t *n_nodes, int64_t *n_landmarks, int64_t *n_closures)
{
    ARGCHK(c, c != nullptr);
    QsGraphDev g;
    int rc = read_graph(c, graph, g);
    if (rc != QS_OK) return rc;
    if (n_nodes) *n_nodes = g.n_nodes;
    if (n_landmarks) *n_landmarks = g.n_lms;
    if (n_closures) *n_closures = g.n_cls;
    return QS_OK;
}

extern "C" int qs_slam_closures(qs_ctx *c, int32_t graph, int64_t *idx2, double *corr2, size_t cap)
{
    ARGCHK(c, c != nullptr && idx2 && corr2);
    QsGraphDev g;
    int rc = read_graph(c, graph, g);
    if (rc != QS_OK) return rc;
    const size_t n = (size_t)g.n_cls;
    if (n > cap) return qs_fail(c, QS_E_RANGE, "qs_slam_closures: capacity too small");
    if (n == 0) return QS_OK;
    std::vector<long long> a(n), b(n); std::vector<double> dx(n), dy(n);
    HIPCHK(c, hipMemcpy(a.data(), g.cl_lm_idx, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(b.data(), g.cl_node_idx, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(dx.data(), g.cl_dx, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(dy.data(), g.cl_dy, n * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) { idx2[2 * i] = a[i]; idx2[2 * i + 1] = b[i]; corr2[2 * i] = dx[i]; corr2[2 * i + 1] = dy[i]; }
    return QS_OK;
}

// agent_id of every closure's closing node (what get_correction_for_agent reads through self.nodes[node_idx], :335)
extern "C" int qs_slam_closure_agents(qs_ctx *c, int32_t graph, uint8_t *agents, size_t cap)
{
    ARGCHK(c, c != nullptr && agents);
    QsGraphDev g;
    int rc = read_graph(c, graph, g);
    if (rc != QS_OK) return rc;
    const size_t n = (size_t)g.n_cls;
    if (n > cap) return qs_fail(c, QS_E_RANGE, "qs_slam_closure_agents: capacity too small");
    if (n) HIPCHK(c, hipMemcpy(agents, g.cl_agent, n, hipMemcpyDeviceToHost));
    return QS_OK;
}

extern "C" int qs_slam_landmarks(qs_ctx *c, int32_t graph, double *xy, int64_t *type_idx, size_t cap)
{
    ARGCHK(c, c != nullptr && xy && type_idx);
    QsGraphDev g;
    int rc = read_graph(c, graph, g);
    if (rc != QS_OK) return rc;
    const size_t n = (size_t)g.n_lms;
    if (n > cap) return qs_fail(c, QS_E_RANGE, "qs_slam_landmarks: capacity too small");
    if (n == 0) return QS_OK;
    std::vector<double> x(n), y(n); std::vector<long long> idx(n); std::vector<unsigned char> t(n);
    HIPCHK(c, hipMemcpy(x.data(), g.lm_x, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(y.data(), g.lm_y, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(idx.data(), g.lm_idx, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(t.data(), g.lm_type, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) { xy[2 * i] = x[i]; xy[2 * i + 1] = y[i]; type_idx[2 * i] = t[i]; type_idx[2 * i + 1] = idx[i]; }
    return QS_OK;
}

// PoseGraphSLAM.add_pose, batched (object API): poses as given, no rays, no EKF.
extern "C" int qs_slam_add_poses(qs_ctx *c, const double *x, const double *y, const uint8_t *agent, const uint8_t *landmark,
                                 size_t n, uint8_t *closed, double *corr2)
{
    ARGCHK(c, c != nullptr);
    if (n == 0) return QS_OK;
    ARGCHK(c, x && y && agent && landmark);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_batch(c, n);
    if (rc != QS_OK) return rc;
    const int G = c->n_graphs, nb = c->cfg.max_agent + 2;
    std::vector<unsigned char> acc(n);
    std::vector<unsigned long long> gb((size_t)G * 2, 0);
    std::vector<unsigned int> aev(nb, 0);
    for (size_t i = 0; i < n; i++) {
        const bool ok = agent[i] >= 1 && agent[i] <= c->cfg.max_agent && isfinite(x[i]) && isfinite(y[i]);
        acc[i] = ok ? 1 : 0;
        if (!ok) continue;
        const int g = (agent[i] - 1) / c->bots_per_graph;
        gb[2 * g]++;
        if (landmark[i]) { gb[2 * g + 1]++; aev[agent[i]]++; }
    }
    HIPCHK(c, hipMemcpyAsync(c->b.accept, acc.data(), n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->b.agent, agent, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->b.lm, landmark, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->b.px, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->b.py, y, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_graph_batch.p, gb.data(), gb.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sb.agent_ev, aev.data(), aev.size() * sizeof(unsigned int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));           // host vectors above go out of use
    c->b.n = n;
    rc = reserve_graphs_for_batch(c, n);
    if (rc != QS_OK) return rc;
    std::vector<QsGraphDev> before(G), after(G);
    HIPCHK(c, hipMemcpyAsync(before.data(), c->d_graphs.p, (size_t)G * sizeof(QsGraphDev), hipMemcpyDeviceToHost, c->stream));
    chain_stats_poll(c, false, nullptr);
    HIPCHK(c, qs_launch_slam(c, n, true));
    { int rcs = chain_stats_request(c); if (rcs != QS_OK) return rcs; }
    HIPCHK(c, hipMemcpyAsync(after.data(), c->d_graphs.p, (size_t)G * sizeof(QsGraphDev), hipMemcpyDeviceToHost, c->stream));
    std::vector<long long> node(n);
    HIPCHK(c, hipMemcpyAsync(node.data(), c->sb.node, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = read_pile_flag(c);
    if (rc != QS_OK) return rc;
    c->last_has_poses = false;
    if (closed) memset(closed, 0, n);
    if (corr2) for (size_t i = 0; i < 2 * n; i++) corr2[i] = 0.0;
    if (!closed && !corr2) return QS_OK;
    for (int g = 0; g < G; g++) {
        const long long k0 = before[g].n_cls, k1 = after[g].n_cls;
        if (k1 <= k0) continue;
        const size_t m = (size_t)(k1 - k0);
        std::vector<long long> cn(m); std::vector<double> dx(m), dy(m);
        HIPCHK(c, hipMemcpy(cn.data(), after[g].cl_node_idx + k0, m * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(dx.data(), after[g].cl_dx + k0, m * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(dy.data(), after[g].cl_dy + k0, m * 8, hipMemcpyDeviceToHost));
        size_t q = 0;     // closures and poses of one graph are both in node order
        for (size_t i = 0; i < n && q < m; i++) {
            if (!acc[i] || (agent[i] - 1) / c->bots_per_graph != g) continue;
            if (node[i] == cn[q]) {
                if (closed) closed[i] = 1;
                if (corr2) { corr2[2 * i] = dx[q]; corr2[2 * i + 1] = dy[q]; }
                q++;
            }
        }
    }
    return QS_OK;
}

extern "C" int qs_drift(qs_ctx *c, int32_t bot, double out[2])
{
    ARGCHK(c, c != nullptr && out);
    if (bot < 1 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_drift: bot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->d_drift.p + 2 * bot, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

// ---- ZONE ---------------------------------------------------------------------------------------
extern "C" int qs_zone(qs_ctx *c, int32_t bot, double out[4], int32_t *valid)
{
    ARGCHK(c, c != nullptr && out && valid);
    if (bot < 1 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_zone: bot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long z[4];
    HIPCHK(c, hipMemcpyAsync(z, c->d_zone.p + 4 * bot, sizeof z, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *valid = z[0] != QS_ORD_MIN_IDENT;                      // compute_bounding_box: None if no points  :704
    for (int i = 0; i < 4; i++) out[i] = *valid ? qs_double_from_ord(z[i]) : NAN;
    return QS_OK;
}

extern "C" int qs_zone_packet(qs_ctx *c, int32_t bot, int32_t online, uint8_t out[QS_ZONE_SIZE])
{
    ARGCHK(c, c != nullptr && out);
    float f[4] = {999.0f, 999.0f, -999.0f, -999.0f};       // send_zone_to_bot(None)  :679-681
    if (online) {
        double z[4]; int32_t valid = 0;
        int rc = qs_zone(c, bot, z, &valid);
        if (rc != QS_OK) return rc;
        if (valid) for (int i = 0; i < 4; i++) f[i] = (float)z[i];   // struct.pack('<4sffff')  :683-684
    }
    memcpy(out, "ZONE", 4);
    memcpy(out + 4, f, 16);
    return QS_OK;
}

// ---- fuse / merge ---------------------------------------------------------------------------------
extern "C" int qs_fuse_buffers_range(qs_ctx *c, const void *const *stamps_dev, const void *const *counts_dev, size_t n,
                                     size_t cell_offset, size_t n_cells, int32_t counts_into_fused)
{
    ARGCHK(c, c != nullptr);
    if (n == 0 || n_cells == 0) return QS_OK;
    ARGCHK(c, stamps_dev != nullptr || counts_dev != nullptr);
    ARGCHK(c, cell_offset % 4 == 0 && n_cells % 4 == 0 && cell_offset + n_cells <= c->cells);
    if (counts_dev && counts_into_fused && !c->d_counts_fused.p)
        return qs_fail(c, QS_E_INVAL, "qs_fuse_buffers_range: no fused counter snapshot (call qs_fused_counts first)");
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long *dc = c->cfg.enable_counts ? (counts_into_fused ? c->d_counts_fused.p : c->d_counts.p) : nullptr;
    HIPCHK(c, qs_launch_fuse(c, (const unsigned int *const *)stamps_dev, (const unsigned long long *const *)counts_dev, n,
                             cell_offset, n_cells, dc));
    if (!counts_into_fused) HIPCHK(c, qs_launch_sf_mark_range(c, cell_offset, n_cells));   // a local fold writes the grid too
    return QS_OK;
}

extern "C" int qs_fuse_buffers(qs_ctx *c, const void *const *stamps_dev, const void *const *counts_dev, size_t n)
{
    ARGCHK(c, c != nullptr);
    if (n == 0) return QS_OK;
    ARGCHK(c, stamps_dev != nullptr);
    return qs_fuse_buffers_range(c, stamps_dev, counts_dev, n, 0, c->cells, 0);
}

// Counters are per-context sums of this context's own writes.  A collective must not add into them (a second
// all-reduce would add the peers' totals again): it sums a SNAPSHOT.  This call copies the local counters into the
// context's second buffer (allocated on first use) on the context's stream and returns it; the caller sums it over the
// ranks in place.  qs_counts_source(ctx, 1) points the counter / log-odds views at it.
extern "C" int qs_fused_counts(qs_ctx *c, void **fused_dev, size_t *bytes)
{
    ARGCHK(c, c != nullptr && fused_dev != nullptr);
    if (!c->d_counts.p) return qs_fail(c, QS_E_INVAL, "qs_fused_counts: context created with enable_counts = 0");
    if (c->d_dirty.p) return qs_fail(c, QS_E_STATE, "qs_fused_counts: dirty tracking is on -- the fused counters accumulate the sparse fuse's deltas");
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    const size_t nb = c->cells * sizeof(unsigned long long);
    if (!c->d_counts_fused.p) HIPCHK(c, c->d_counts_fused.alloc(c->cells));
    HIPCHK(c, hipMemcpyAsync(c->d_counts_fused.p, c->d_counts.p, nb, hipMemcpyDeviceToDevice, c->stream));
    *fused_dev = c->d_counts_fused.p;
    if (bytes) *bytes = nb;
    return QS_OK;
}

extern "C" int qs_fused_counts_buffer(qs_ctx *c, void **fused_dev, size_t *bytes)
{
    ARGCHK(c, c != nullptr && fused_dev != nullptr);
    *fused_dev = c->d_counts_fused.p;
    if (bytes) *bytes = c->d_counts_fused.p ? c->cells * sizeof(unsigned long long) : 0;
    return QS_OK;
}

extern "C" int qs_counts_source(qs_ctx *c, int32_t fused)
{
    ARGCHK(c, c != nullptr);
    if (fused && !c->d_counts_fused.p) return qs_fail(c, QS_E_INVAL, "qs_counts_source: no fused snapshot yet (qs_fused_counts)");
    c->counts_view_fused = fused != 0;
    return QS_OK;
}

// ---- sparse fuse (sparse_fuse.hip; protocol in include/quasar_slam.h) --------------------------------------------------
extern "C" int qs_dirty_tracking(qs_ctx *c, int32_t enable)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!enable) {
        c->geom.dirty = nullptr; c->geom.dirty_pitch = 0;
        c->d_dirty = DevBuf<unsigned int>();
        c->sf_state = 0;
        c->counts_view_fused = false;         // the fused counters stop following the ranks: the views read the own ones
        return QS_OK;
    }
    if (c->d_dirty.p) return QS_OK;
    if (c->dirty_since_fuse) return qs_fail(c, QS_E_STATE, "qs_dirty_tracking: the grid has unfused writes (enable it after qs_create / qs_reset / a fuse)");
    c->blocks_x = (c->cfg.size + QS_DIRTY_BLOCK_W - 1) / QS_DIRTY_BLOCK_W;
    c->blocks_y = (c->cfg.size + QS_DIRTY_BLOCK_H - 1) / QS_DIRTY_BLOCK_H;
    const int pitch = (c->blocks_x + 31) / 32;
    c->dirty_words = (size_t)c->blocks_y * pitch;
    if (c->d_counts.p) {
        const size_t nb = c->cells * sizeof(unsigned long long);
        if (!c->d_counts_sent.p) HIPCHK(c, c->d_counts_sent.alloc(c->cells));
        // the fused counters accumulate deltas from here on: they start as "nothing sent", the local counters as all delta
        HIPCHK(c, hipMemsetAsync(c->d_counts_sent.p, 0, nb, c->stream));
        if (!c->d_counts_fused.p) HIPCHK(c, c->d_counts_fused.alloc(c->cells));
        HIPCHK(c, hipMemsetAsync(c->d_counts_fused.p, 0, nb, c->stream));
        // counters written before tracking was switched on have no dirty bit: everything is marked once
    }
    // the bitmap last, published with geom.dirty: tracking is on (d_dirty set) only once everything it writes exists
    HIPCHK(c, c->d_dirty.alloc(c->dirty_words));
    c->geom.dirty = c->d_dirty.p; c->geom.dirty_pitch = pitch;
    HIPCHK(c, hipMemsetAsync(c->d_dirty.p, 0, c->dirty_words * sizeof(unsigned int), c->stream));
    if (c->next_seq != 0) HIPCHK(c, qs_launch_sf_mark_range(c, 0, c->cells));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_dirty_blocks(qs_ctx *c, size_t *n_blocks, size_t *block_cells)
{
    ARGCHK(c, c != nullptr && n_blocks != nullptr);
    if (!c->d_dirty.p) return qs_fail(c, QS_E_STATE, "qs_dirty_blocks: dirty tracking is off (qs_dirty_tracking)");
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    HIPCHK(c, c->io_ws.reserve(sizeof(unsigned long long), c->stream, QS_IO_WS_FLOOR));
    unsigned long long v = 0;
    HIPCHK(c, qs_launch_sf_popcount(c, (unsigned long long *)c->io_ws.p));
    HIPCHK(c, hipMemcpyAsync(&v, c->io_ws.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_blocks = (size_t)v;
    if (block_cells) *block_cells = (size_t)QS_DIRTY_BLOCK_W * QS_DIRTY_BLOCK_H;
    return QS_OK;
}

// the per-rank arrays of a fuse of `world` ranks, carved from base (nullptr: only the size); returns the bytes
static size_t sf_layout(const qs_ctx *c, void *base, int world, unsigned int *&bitmaps, unsigned int *&lists, unsigned int *&counts)
{
    Carve k(base);
    bitmaps = k.take<unsigned int>((size_t)world * c->dirty_words);
    lists = k.take<unsigned int>((size_t)world * c->dirty_words * 32);
    counts = k.take<unsigned int>((size_t)world);
    return k.bytes;
}

extern "C" int qs_sparse_fuse_begin(qs_ctx *c, int32_t world, int32_t rank, void **bitmaps_dev, size_t *bitmap_bytes)
{
    ARGCHK(c, c != nullptr && bitmaps_dev != nullptr && bitmap_bytes != nullptr);
    ARGCHK(c, world >= 1 && world <= QS_SPARSE_MAX_WORLD && rank >= 0 && rank < world);
    if (!c->d_dirty.p) return qs_fail(c, QS_E_STATE, "qs_sparse_fuse_begin: dirty tracking is off (qs_dirty_tracking)");
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    // a fuse begun here that never reached apply: its blocks did not travel, so they go into this one (before a change of
    // world reallocates the bitmaps).  Nothing else was committed: the counter deltas are taken from `sent`, which only
    // apply advances.
    if (c->sf_state != 0) { HIPCHK(c, qs_launch_sf_restore(c)); c->sf_state = 0; }
    if (world != c->sf_world) {                              // (a growth that fails leaves the old arrays as they were)
        unsigned int *bm, *li, *co;
        DevBuf<char> meta;
        HIPCHK(c, meta.alloc(sf_layout(c, nullptr, world, bm, li, co)));
        HIPCHK(c, hipStreamSynchronize(c->stream));          // (the old arrays may still be in use)
        c->sf_meta = std::move(meta);
        sf_layout(c, c->sf_meta.p, world, c->d_sf_bitmaps, c->d_sf_lists, c->d_sf_counts);
        c->sf_world = world;
        c->sf_n.assign(world, 0); c->sf_off.assign((size_t)world + 1, 0);
    }
    c->sf_rank = rank;
    const size_t nb = c->dirty_words * sizeof(unsigned int);
    HIPCHK(c, hipMemcpyAsync(c->d_sf_bitmaps + (size_t)rank * c->dirty_words, c->d_dirty.p, nb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_dirty.p, 0, nb, c->stream));
    *bitmaps_dev = c->d_sf_bitmaps; *bitmap_bytes = nb;
    c->sf_state = 1;
    return QS_OK;
}

extern "C" int qs_sparse_fuse_plan(qs_ctx *c, uint32_t *n_blocks, size_t *offsets, void **payload_dev, size_t *block_bytes)
{
    ARGCHK(c, c != nullptr && n_blocks != nullptr && offsets != nullptr && payload_dev != nullptr);
    if (c->sf_state != 1) return qs_fail(c, QS_E_STATE, "qs_sparse_fuse_plan: call qs_sparse_fuse_begin (and all-gather the bitmaps) first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, qs_launch_sf_lists(c));
    HIPCHK(c, hipMemcpyAsync(c->sf_n.data(), c->d_sf_counts, (size_t)c->sf_world * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t bb = qs_sf_block_bytes(c);
    size_t run = 0;
    for (int s = 0; s < c->sf_world; s++) { c->sf_off[s] = run; run += (size_t)c->sf_n[s] * bb; n_blocks[s] = c->sf_n[s]; offsets[s] = c->sf_off[s]; }
    c->sf_off[c->sf_world] = run; offsets[c->sf_world] = run;
    HIPCHK(c, c->sf_payload.reserve(run, c->stream, (size_t)1 << 20));        // doubling from 1 MiB
    HIPCHK(c, qs_launch_sf_pack(c, c->sf_n[c->sf_rank], c->sf_payload.p + c->sf_off[c->sf_rank]));
    *payload_dev = c->sf_payload.p;
    if (block_bytes) *block_bytes = bb;
    c->sf_state = 2;
    return QS_OK;
}

extern "C" int qs_sparse_fuse_apply(qs_ctx *c)
{
    ARGCHK(c, c != nullptr);
    if (c->sf_state != 2) return qs_fail(c, QS_E_STATE, "qs_sparse_fuse_apply: call qs_sparse_fuse_plan (and exchange the segments) first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, qs_launch_sf_apply(c));
    c->sf_state = 0;
    c->dirty_since_fuse = false;
    if (c->d_counts.p) c->counts_view_fused = true;
    return QS_OK;
}

extern "C" int qs_fuse(qs_ctx *dst, qs_ctx *const *srcs, size_t n)
{
    ARGCHK(dst, dst != nullptr);
    if (n == 0) return QS_OK;
    ARGCHK(dst, srcs != nullptr);
    std::vector<const void *> st(n), ct(n);
    bool counts = dst->d_counts.p != nullptr;
    for (size_t i = 0; i < n; i++) {
        qs_ctx *s = srcs[i];
        if (!s || s->device != dst->device || s->cfg.size != dst->cfg.size || s->cfg.res != dst->cfg.res ||
            s->cfg.ox != dst->cfg.ox || s->cfg.oy != dst->cfg.oy)
            return qs_fail(dst, QS_E_INVAL, "qs_fuse: source grids must share device and geometry with dst");
        if (s->epoch_base != dst->epoch_base || s->n_rebases != dst->n_rebases)
            return qs_fail(dst, QS_E_INVAL, "qs_fuse: source and destination are in different stamp epochs");
        { HIPCHK(dst, hipSetDevice(s->device)); int rcs = flush_edge_rays(s); if (rcs != QS_OK) return qs_fail(dst, rcs, s->err.c_str()); }
        HIPCHK(dst, hipStreamSynchronize(s->stream));
        st[i] = s->d_stamps.p; ct[i] = s->d_counts.p;
        if (!s->d_counts.p) counts = false;
    }
    int rc = qs_fuse_buffers(dst, st.data(), counts ? ct.data() : nullptr, n);
    if (rc != QS_OK) return rc;
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    return QS_OK;
}

extern "C" int qs_grid_to_pcd(qs_ctx *c, const int8_t *grid, int32_t h, int32_t w, double res, double ox, double oy,
                              double *xy, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && grid != nullptr && n_out != nullptr && h > 0 && w > 0);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)h * w, n_chunks = (cells + 1023) / 1024;
    DevBuf<signed char> dg; DevBuf<unsigned int> dchunk; DevBuf<unsigned long long> dcount; DevBuf<double> dxy;
    HIPCHK(c, dg.alloc(cells));
    HIPCHK(c, dchunk.alloc(n_chunks));
    HIPCHK(c, dcount.alloc(1));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(dg.p, grid, cells, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_grid_to_pcd(c, dg.p, h, w, res, ox, oy, nullptr, 0, dcount.p, dchunk.p));
    HIPCHK(c, hipMemcpyAsync(&total, dcount.p, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = (size_t)total;
    if (!xy || total == 0) return QS_OK;
    const size_t m = total < cap ? (size_t)total : cap;
    HIPCHK(c, dxy.alloc(2 * (size_t)total));
    HIPCHK(c, qs_launch_grid_to_pcd(c, dg.p, h, w, res, ox, oy, dxy.p, (size_t)total, dcount.p, dchunk.p));
    HIPCHK(c, hipMemcpyAsync(xy, dxy.p, 2 * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_rasterise(qs_ctx *c, const double *xy, size_t n, double res, int32_t dims[2], double origin[2], int8_t *grid)
{
    ARGCHK(c, c != nullptr && dims && origin && res > 0);
    if (n == 0) { dims[0] = dims[1] = 0; return QS_OK; }      // publish_global_map returns early  :88-93
    ARGCHK(c, xy != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> dxy; DevBuf<unsigned long long> dbox; DevBuf<signed char> dg;
    unsigned long long box[4] = {QS_ORD_MIN_IDENT, QS_ORD_MIN_IDENT, QS_ORD_MAX_IDENT, QS_ORD_MAX_IDENT};
    HIPCHK(c, dxy.alloc(2 * n));
    HIPCHK(c, dbox.alloc(4));
    HIPCHK(c, hipMemcpyAsync(dxy.p, xy, 2 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dbox.p, box, sizeof box, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_bbox(c, dxy.p, n, dbox.p));
    HIPCHK(c, hipMemcpyAsync(box, dbox.p, sizeof box, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double mnx = qs_double_from_ord(box[0]), mny = qs_double_from_ord(box[1]);
    const double mxx = qs_double_from_ord(box[2]), mxy = qs_double_from_ord(box[3]);
    const double wd = ceil((mxx - mnx) / res), hd = ceil((mxy - mny) / res);     // :103-104
    if (!(wd >= 0 && wd < 65536 && hd >= 0 && hd < 65536)) return qs_fail(c, QS_E_RANGE, "qs_rasterise: canvas too large");
    const int w = (int)wd + 1, h = (int)hd + 1;
    dims[0] = h; dims[1] = w; origin[0] = mnx; origin[1] = mny;
    if (!grid) return QS_OK;
    HIPCHK(c, dg.alloc((size_t)h * w));
    HIPCHK(c, qs_launch_rasterise(c, dxy.p, n, res, mnx, mny, h, w, dg.p));
    HIPCHK(c, hipMemcpyAsync(grid, dg.p, (size_t)h * w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

// ---- ICP / voxel down-sample (map_merger.py:45-60; Open3D semantics, parity unpinned) ------------------
// The correspondence search (nearest target of every source point) has two implementations with identical results:
// the scalar fp64 brute force and the MFMA-screened one (icp.hip).  mode 0 = auto (MFMA from 64 targets up).
struct NnPlan { double cx = 0, cy = 0, t2max = 0; size_t n_pad = 0; bool mfma = false; DevBuf<double> planes, part_d2, thr_seed; DevBuf<int> part_j; };

static hipError_t nn_prepare(qs_ctx *c, const double *dst_xy, size_t n_dst, const double2 *d_dst, int mode, NnPlan &pl, size_t n_src)
{
    pl.mfma = mode == 2 || (mode == 0 && n_dst >= 64);
    if (!pl.mfma) return hipSuccess;
    double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (size_t j = 0; j < n_dst; j++) {
        const double x = dst_xy[2 * j], y = dst_xy[2 * j + 1];
        if (isfinite(x)) { mnx = x < mnx ? x : mnx; mxx = x > mxx ? x : mxx; }
        if (isfinite(y)) { mny = y < mny ? y : mny; mxy = y > mxy ? y : mxy; }
    }
    pl.cx = isfinite(mnx) ? 0.5 * (mnx + mxx) : 0.0; pl.cy = isfinite(mny) ? 0.5 * (mny + mxy) : 0.0;
    const double hx = isfinite(mnx) ? mxx - pl.cx : 0.0, hy = isfinite(mny) ? mxy - pl.cy : 0.0;
    pl.t2max = 1.0001 * (hx * hx + hy * hy) + 1e-300;          // >= every finite target's centred squared norm
    pl.n_pad = (n_dst + 15) / 16 * 16;
    HIPRET(pl.planes.alloc(3 * pl.n_pad));
    HIPRET(qs_launch_icp_prep(c, d_dst, n_dst, pl.n_pad, pl.cx, pl.cy, pl.planes.p));
    // per-part results and the sources' threshold seeds (the targets are cut into parts: icp.hip)
    unsigned int groups, parts, cpp;
    qs_icp_nn_plan(n_src, pl.n_pad, &groups, &parts, &cpp);
    HIPRET(pl.part_j.alloc((size_t)parts * n_src));
    HIPRET(pl.part_d2.alloc((size_t)parts * n_src));
    return pl.thr_seed.alloc(n_src);
}

static hipError_t nn_run(qs_ctx *c, const NnPlan &pl, const double2 *d_src, size_t n_src, const double2 *d_dst, size_t n_dst,
                         double max_d2, int *d_corr, double *d_d2)
{
    if (pl.mfma) return qs_launch_icp_nn_mfma(c, d_src, n_src, d_dst, n_dst, pl.planes.p, pl.n_pad, pl.cx, pl.cy, pl.t2max, max_d2, d_corr, d_d2,
                                              pl.part_j.p, pl.part_d2.p, pl.thr_seed.p);
    return qs_launch_icp_nn(c, d_src, n_src, d_dst, n_dst, max_d2, d_corr, d_d2);
}

// Build extension (the correspondence step of registration_icp on its own; used by the tests and tools/bench_icp_nn.py):
// corr[i] = index of the target nearest to source i if closer than max_dist, else -1 (ties: lowest index); d2[i] its squared
// distance (0 without a correspondence).  ms (may be NULL): HIP-event time of {the search kernel, the operand preparation}.
extern "C" int qs_nn_search(qs_ctx *c, const double *src_xy, size_t n_src, const double *dst_xy, size_t n_dst, double max_dist,
                            int32_t mode, int32_t *corr, double *d2, float ms[2])
{
    ARGCHK(c, c != nullptr && corr != nullptr && d2 != nullptr);
    ARGCHK(c, n_src > 0 && n_dst > 0 && src_xy && dst_xy && max_dist > 0 && mode >= 0 && mode <= 2);
    ARGCHK(c, n_dst < (size_t)1 << 31);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double2> d_src, d_dst; DevBuf<int> d_corr; DevBuf<double> d_d2;
    NnPlan pl;
    ScopedEvent ev[4];
    HIPCHK(c, d_src.alloc(n_src));
    HIPCHK(c, d_dst.alloc(n_dst));
    HIPCHK(c, d_corr.alloc(n_src));
    HIPCHK(c, d_d2.alloc(n_src));
    for (auto &v : ev) HIPCHK(c, hipEventCreate(&v.e));
    HIPCHK(c, hipMemcpyAsync(d_src.p, src_xy, n_src * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_dst.p, dst_xy, n_dst * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(ev[0].e, c->stream));
    HIPCHK(c, nn_prepare(c, dst_xy, n_dst, d_dst.p, mode, pl, n_src));
    HIPCHK(c, hipEventRecord(ev[1].e, c->stream));
    HIPCHK(c, nn_run(c, pl, d_src.p, n_src, d_dst.p, n_dst, max_dist * max_dist, d_corr.p, d_d2.p));      // warm (code load, caches)
    HIPCHK(c, hipEventRecord(ev[2].e, c->stream));
    HIPCHK(c, nn_run(c, pl, d_src.p, n_src, d_dst.p, n_dst, max_dist * max_dist, d_corr.p, d_d2.p));
    HIPCHK(c, hipEventRecord(ev[3].e, c->stream));
    HIPCHK(c, hipMemcpyAsync(corr, d_corr.p, n_src * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(d2, d_d2.p, n_src * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ms) { hipEventElapsedTime(&ms[0], ev[2].e, ev[3].e); hipEventElapsedTime(&ms[1], ev[0].e, ev[1].e); }
    return QS_OK;
}

extern "C" int qs_icp(qs_ctx *c, const double *src_xy, size_t n_src, const double *dst_xy, size_t n_dst, double max_dist,
                      int32_t max_iter, double rel_fitness, double rel_rmse, double T[9], double *fitness, double *rmse,
                      int32_t *iters)
{
    ARGCHK(c, c != nullptr && T != nullptr && fitness != nullptr && rmse != nullptr);
    ARGCHK(c, n_src > 0 && n_dst > 0 && src_xy && dst_xy && max_dist > 0 && max_iter >= 0);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb = (n_src + 255) / 256;
    DevBuf<double2> d_src, d_dst; DevBuf<int> d_corr; DevBuf<double> d_d2, d_part, d_out;
    HIPCHK(c, d_src.alloc(n_src));
    HIPCHK(c, d_dst.alloc(n_dst));
    HIPCHK(c, d_corr.alloc(n_src));
    HIPCHK(c, d_d2.alloc(n_src));
    HIPCHK(c, d_part.alloc(nb * 6));
    HIPCHK(c, d_out.alloc(6));
    HIPCHK(c, hipMemcpyAsync(d_src.p, src_xy, n_src * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_dst.p, dst_xy, n_dst * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    NnPlan pl;
    HIPCHK(c, nn_prepare(c, dst_xy, n_dst, d_dst.p, 0, pl, n_src));     // the targets do not move: operands once per registration
    double tc = 1.0, ts = 0.0, tx = 0.0, ty = 0.0;          // accumulated transform
    double out[6] = {0};
    const double zero4[4] = {0, 0, 0, 0};
    auto evaluate = [&](double &fit, double &rm) -> hipError_t {
        HIPRET(nn_run(c, pl, d_src.p, n_src, d_dst.p, n_dst, max_dist * max_dist, d_corr.p, d_d2.p));
        HIPRET(qs_launch_icp_sums(c, d_src.p, n_src, d_dst.p, d_corr.p, d_d2.p, 0, zero4, d_part.p, d_out.p));
        HIPRET(hipMemcpyAsync(out, d_out.p, sizeof out, hipMemcpyDeviceToHost, c->stream));
        HIPRET(hipStreamSynchronize(c->stream));
        fit = out[0] / (double)n_src;
        rm = out[0] > 0 ? sqrt(out[1] / out[0]) : 0.0;
        return hipSuccess;
    };
    double fit = 0, rm = 0;
    int it = 0;
    HIPCHK(c, evaluate(fit, rm));
    for (; it < max_iter; it++) {
        double uc = 1.0, us = 0.0, ux = 0.0, uy = 0.0;       // ComputeTransformation: identity without correspondences
        if (out[0] > 0) {
            const double nn = out[0];
            const double means[4] = {out[2] / nn, out[3] / nn, out[4] / nn, out[5] / nn};
            double o2[6];
            HIPCHK(c, qs_launch_icp_sums(c, d_src.p, n_src, d_dst.p, d_corr.p, d_d2.p, 1, means, d_part.p, d_out.p));
            HIPCHK(c, hipMemcpyAsync(o2, d_out.p, sizeof o2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            const double theta = atan2(o2[1], o2[0]);
            uc = cos(theta); us = sin(theta);
            ux = means[2] - (uc * means[0] - us * means[1]);
            uy = means[3] - (us * means[0] + uc * means[1]);
        }
        // transformation = update * transformation
        const double nc = uc * tc - us * ts, ns = us * tc + uc * ts;
        const double nx = uc * tx - us * ty + ux, ny = us * tx + uc * ty + uy;
        tc = nc; ts = ns; tx = nx; ty = ny;
        HIPCHK(c, qs_launch_icp_transform(c, d_src.p, n_src, uc, us, ux, uy));
        const double bfit = fit, brm = rm;
        HIPCHK(c, evaluate(fit, rm));
        if (fabs(bfit - fit) < rel_fitness && fabs(brm - rm) < rel_rmse) { it++; break; }
    }
    T[0] = tc; T[1] = -ts; T[2] = tx; T[3] = ts; T[4] = tc; T[5] = ty; T[6] = 0; T[7] = 0; T[8] = 1;
    *fitness = fit; *rmse = rm;
    if (iters) *iters = it;
    return QS_OK;
}

// Diagnostic: measured fp64 MFMA rate of this GPU (dense v_mfma_f64_16x16x4_f64, every CU, 2 waves per SIMD), TFLOP/s.
extern "C" int qs_diag_mfma_f64_rate(qs_ctx *c, double *tflops)
{
    ARGCHK(c, c != nullptr && tflops != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> sink;
    ScopedEvent a, b;
    const int blocks = 256 * 2, iters = 20000;             // 2 workgroups of 4 waves per CU
    HIPCHK(c, sink.alloc(1));
    HIPCHK(c, hipEventCreate(&a.e));
    HIPCHK(c, hipEventCreate(&b.e));
    HIPCHK(c, qs_launch_mfma_f64_rate(c, blocks, 1000, sink.p));
    HIPCHK(c, hipEventRecord(a.e, c->stream));
    HIPCHK(c, qs_launch_mfma_f64_rate(c, blocks, iters, sink.p));
    HIPCHK(c, hipEventRecord(b.e, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, a.e, b.e));
    const double flops = (double)blocks * 4 /* waves */ * iters * 4 /* MFMAs */ * (2.0 * 16 * 16 * 4);
    *tflops = flops / (ms * 1e-3) / 1e12;
    return QS_OK;
}

// Diagnostic: measured latencies of the primitives of one loop-closure decision (diag.hip), shader-clock cycles.
extern "C" int qs_diag_latencies(qs_ctx *c, double out[QS_DIAG_LAT_N])
{
    ARGCHK(c, c != nullptr && out != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    const unsigned int n2 = 1u << 18, n1 = 1u << 11;            // 1 MiB: past the 32 KiB L1, inside the 4 MiB L2; 8 KiB: inside L1
    std::vector<unsigned int> h2(n2), h1(n1);
    for (unsigned int k = 0; k < n2; k++) h2[k] = (k * 1664525u + 1013904223u) & (n2 - 1);     // full-period LCG: one cycle through all entries
    for (unsigned int k = 0; k < n1; k++) h1[k] = (k * 1664525u + 1013904223u) & (n1 - 1);
    DevBuf<unsigned int> d2, d1; DevBuf<double> d_out;
    double h_out[16] = {0};
    HIPCHK(c, d2.alloc(n2));
    HIPCHK(c, d1.alloc(n1));
    HIPCHK(c, d_out.alloc(16));
    HIPCHK(c, hipMemcpyAsync(d2.p, h2.data(), n2 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d1.p, h1.data(), n1 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_out.p, 0, sizeof h_out, c->stream));
    HIPCHK(c, qs_launch_diag_latencies(c, d2.p, d1.p, d_out.p));          // (warm: code load)
    HIPCHK(c, qs_launch_diag_latencies(c, d2.p, d1.p, d_out.p));
    HIPCHK(c, hipMemcpyAsync(h_out, d_out.p, sizeof h_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < QS_DIAG_LAT_N; i++) out[i] = h_out[i];
    return QS_OK;
}

extern "C" int qs_voxel_downsample(qs_ctx *c, const double *xy, size_t n, double voxel, double *out_xy, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr && voxel > 0);
    *n_out = 0;
    if (n == 0) return QS_OK;
    ARGCHK(c, xy != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    double mnx = xy[0], mny = xy[1];
    for (size_t i = 1; i < n; i++) { if (xy[2 * i] < mnx) mnx = xy[2 * i]; if (xy[2 * i + 1] < mny) mny = xy[2 * i + 1]; }
    mnx -= voxel * 0.5; mny -= voxel * 0.5;                 // voxel_min_bound = min_bound - voxel_size / 2
    std::vector<unsigned long long> keys(n);
    {
        DevBuf<double2> d; DevBuf<unsigned long long> dk;
        HIPCHK(c, d.alloc(n));
        HIPCHK(c, dk.alloc(n));
        HIPCHK(c, hipMemcpyAsync(d.p, xy, n * sizeof(double2), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, qs_launch_voxel_keys(c, d.p, n, mnx, mny, voxel, dk.p));
        HIPCHK(c, hipMemcpyAsync(keys.data(), dk.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    // group by voxel (ascending key), average in input order: a handful of points per ROS callback
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    size_t k = 0;
    for (size_t p = 0; p < n;) {
        size_t q = p; double sx = 0, sy = 0;
        while (q < n && keys[order[q]] == keys[order[p]]) { sx += xy[2 * order[q]]; sy += xy[2 * order[q] + 1]; q++; }
        if (out_xy && k < cap) { out_xy[2 * k] = sx / (double)(q - p); out_xy[2 * k + 1] = sy / (double)(q - p); }
        k++; p = q;
    }
    *n_out = k;
    return QS_OK;
}

// ---- frontiers ------------------------------------------------------------------------------------
static int frontier_run(qs_ctx *c, int mode, int32_t min_cluster, int32_t *xy, int64_t *stats5, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    HIPCHK(c, c->frontier_ws.reserve(qs_frontier_layout(c, nullptr).bytes, c->stream));
    void *ws = c->frontier_ws.p;
    HIPCHK(c, qs_launch_frontier_label(c, ws, mode != 0));
    HIPCHK(c, qs_launch_frontier_compact(c, ws, mode == 2 ? 0 : mode, 0, nullptr, nullptr, 0));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, qs_frontier_layout(c, ws).total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode != 1) {
        // cells (mode 0: gx, gy), or every frontier cell with the first cell (row-major) of its 4-connected cluster (mode 2:
        // gx, gy, root linear index)
        *n_out = (size_t)total;
        if (!xy || total == 0) return QS_OK;
        const size_t per = mode == 0 ? 2 : 3, m = total < cap ? (size_t)total : cap;
        DevBuf<int> d;
        HIPCHK(c, d.alloc(per * (size_t)total));
        HIPCHK(c, qs_launch_frontier_compact(c, ws, mode, 1, d.p, nullptr, (size_t)total));
        HIPCHK(c, hipMemcpyAsync(xy, d.p, per * m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return QS_OK;
    }
    // clusters: all components come back in first-cell order; the size filter keeps that order (:228-229)
    std::vector<long long> all(5 * (size_t)total);
    if (total) {
        DevBuf<long long> d;
        HIPCHK(c, d.alloc(5 * (size_t)total));
        HIPCHK(c, qs_launch_frontier_compact(c, ws, 1, 1, nullptr, d.p, (size_t)total));
        HIPCHK(c, hipMemcpyAsync(all.data(), d.p, all.size() * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    size_t k = 0;
    for (size_t i = 0; i < (size_t)total; i++) {
        if (all[5 * i] < min_cluster) continue;
        if (stats5 && k < cap) memcpy(stats5 + 5 * k, &all[5 * i], 5 * sizeof(long long));
        k++;
    }
    *n_out = k;
    return QS_OK;
}

extern "C" int qs_frontier_cells(qs_ctx *c, int32_t *xy, size_t cap, size_t *n_out)
{ return frontier_run(c, 0, 0, xy, nullptr, cap, n_out); }

extern "C" int qs_frontier_members(qs_ctx *c, int32_t *xy_root, size_t cap, size_t *n_out)
{ return frontier_run(c, 2, 0, xy_root, nullptr, cap, n_out); }

extern "C" int qs_frontier_clusters(qs_ctx *c, int32_t min_cluster, int64_t *stats5, size_t cap, size_t *n_out)
{ return frontier_run(c, 1, min_cluster, nullptr, stats5, cap, n_out); }

// frontier target assignment (frontier_targets.hip): centroids on the device, top-K lists, the greedy pass; the pass
// stops at a bot whose full list is ineligible, a whole-GPU scan decides that bot, and the pass resumes from it
extern "C" int qs_frontier_targets(qs_ctx *c, int32_t min_cluster, double separation, const double *bot_xy, size_t n_bots,
                                   int64_t *target_idx, double *target_xy, double *centroids_xy, size_t cap,
                                   size_t *n_centroids, uint64_t stats[4])
{
    ARGCHK(c, c != nullptr);
    if (n_bots > QS_FT_MAX_BOTS) return qs_fail(c, QS_E_INVAL, "qs_frontier_targets: n_bots above QS_FT_MAX_BOTS");
    ARGCHK(c, n_bots == 0 || (bot_xy && target_idx && target_xy));
    ARGCHK(c, cap == 0 || centroids_xy);
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    HIPCHK(c, c->frontier_ws.reserve(qs_frontier_layout(c, nullptr).bytes, c->stream));
    void *fws = c->frontier_ws.p;
    HIPCHK(c, qs_launch_frontier_label(c, fws, true));
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 0, nullptr));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, qs_frontier_layout(c, fws).total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n_cent = (size_t)total;
    HIPCHK(c, c->ft_ws.reserve(qs_ft_layout(nullptr, n_cent, n_bots).bytes, c->stream));
    const QsFtLayout F = qs_ft_layout(c->ft_ws.p, n_cent, n_bots);
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 1, F.cent));
    uint64_t fallbacks = 0;
    std::vector<long long> tidx(n_bots, -1);
    std::vector<double> txy(2 * n_bots);
    if (n_bots && n_cent) {
        const double r2_sep = r2_threshold_for(separation);        // s < r2_sep <=> sqrt(s) < separation (0: nothing is too close)
        HIPCHK(c, hipMemcpyAsync(F.bots, bot_xy, n_bots * sizeof(double2), hipMemcpyHostToDevice, c->stream));
        int start = 0, m = 0, pending = 0;
        for (;;) {
            HIPCHK(c, qs_launch_ft_assign(c, c->ft_ws.p, n_cent, n_bots, r2_sep, start, m, pending));
            QsFtState st;
            HIPCHK(c, hipMemcpyAsync(&st, F.st, sizeof st, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (!st.stop) break;
            if (st.next_bot < start || st.next_bot >= (int)n_bots || (pending && st.next_bot == start))
                return qs_fail(c, QS_E_HIP, "qs_frontier_targets: greedy pass made no progress");
            fallbacks++;
            start = st.next_bot; m = st.m; pending = 1;
            HIPCHK(c, qs_launch_ft_fallback(c, c->ft_ws.p, n_cent, n_bots, r2_sep, start, m));
        }
        HIPCHK(c, hipMemcpyAsync(tidx.data(), F.tgt_idx, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(txy.data(), F.tgt_xy, n_bots * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    }
    const size_t nc = n_cent < cap ? n_cent : cap;
    if (nc) HIPCHK(c, hipMemcpyAsync(centroids_xy, F.cent, nc * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t b = 0; b < n_bots; b++) {
        target_idx[b] = tidx[b];
        if (tidx[b] >= 0) { target_xy[2 * b] = txy[2 * b]; target_xy[2 * b + 1] = txy[2 * b + 1]; }
    }
    if (n_centroids) *n_centroids = n_cent;
    if (stats) { stats[0] = n_cent; stats[1] = QS_FT_K; stats[2] = fallbacks; stats[3] = 0; }
    return QS_OK;
}

// ---- path planning (plan.hip) ------------------------------------------------------------------------
static int plan_params(qs_ctx *c, const qs_plan_params *p, qs_plan_params &out)
{
    out = p ? *p : qs_plan_params{2, 10, 200, 0};        // the defaults (include/quasar_slam.h)
    if (out.clearance < 0 || out.clearance > QS_PLAN_MAX_CLEARANCE)
        return qs_fail(c, QS_E_INVAL, "path planning: clearance must lie in [0, QS_PLAN_MAX_CLEARANCE]");
    if (out.snap_radius < 0 || out.snap_radius > QS_PLAN_MAX_SNAP)
        return qs_fail(c, QS_E_INVAL, "path planning: snap_radius must lie in [0, QS_PLAN_MAX_SNAP]");
    if (out.lookahead < 1 || out.lookahead > QS_PLAN_MAX_LOOKAHEAD)
        return qs_fail(c, QS_E_INVAL, "path planning: lookahead must lie in [1, QS_PLAN_MAX_LOOKAHEAD]");
    return QS_OK;
}

// the mask and the census for n requests (layout of the planner workspace); bbox[0] > bbox[2]: no traversable cell
static int plan_begin(qs_ctx *c, int clearance, size_t n, size_t path_cap, QsPlanLayout &L, unsigned int bbox[4])
{
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    HIPCHK(c, c->plan_ws.reserve(qs_plan_layout(nullptr, c->cfg.size, n, path_cap).bytes, c->stream));
    L = qs_plan_layout(c->plan_ws.p, c->cfg.size, n, path_cap);
    HIPCHK(c, hipMemsetAsync(L.stats, 0, 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, qs_launch_plan_trav(c, L, clearance));
    HIPCHK(c, hipMemcpyAsync(bbox, L.bbox, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

// the fields of requests g0 .. g0 + gn: seed, then rounds in batches of QS_PLAN_ROUND_BATCH without a sync (a round that
// finds its list empty returns at once), the live count read once per batch; then the walk
#define QS_PLAN_ROUND_BATCH 8
static int plan_group(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], size_t n, size_t g0, size_t gn,
                      int lookahead, size_t path_cap)
{
    HIPCHK(c, qs_launch_plan_seed(c, L, bbox, n, g0, gn));
    for (unsigned int r = 1;; r += QS_PLAN_ROUND_BATCH) {
        for (unsigned int k = 0; k < QS_PLAN_ROUND_BATCH; k++) HIPCHK(c, qs_launch_plan_round(c, L, bbox, gn, r + k));
        unsigned int live = 0;
        HIPCHK(c, hipMemcpyAsync(&live, L.cnt + (r + QS_PLAN_ROUND_BATCH) % 3, sizeof live, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!live) break;
        if (r > 0x7fffffffu) return qs_fail(c, QS_E_STATE, "path planning: the relaxation did not settle");
    }
    if (lookahead > 0) HIPCHK(c, qs_launch_plan_walk(c, L, bbox, n, g0, gn, lookahead, path_cap));
    return QS_OK;
}

extern "C" int qs_traversable(qs_ctx *c, int32_t clearance, uint8_t *mask_host)
{
    ARGCHK(c, c != nullptr && mask_host != nullptr);
    if (clearance < 0 || clearance > QS_PLAN_MAX_CLEARANCE)
        return qs_fail(c, QS_E_INVAL, "qs_traversable: clearance must lie in [0, QS_PLAN_MAX_CLEARANCE]");
    QsPlanLayout L;
    unsigned int bbox[4];
    int rc = plan_begin(c, clearance, 0, 0, L, bbox);
    if (rc != QS_OK) return rc;
    const size_t size = (size_t)c->cfg.size, mp = (size_t)L.mp;
    std::vector<unsigned int> bits(size * mp);
    HIPCHK(c, hipMemcpy(bits.data(), L.mask, bits.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    for (size_t y = 0; y < size; y++)
        for (size_t x = 0; x < size; x++) mask_host[y * size + x] = (bits[y * mp + (x >> 5)] >> (x & 31)) & 1u;
    return QS_OK;
}

extern "C" int qs_plan_field(qs_ctx *c, const qs_plan_params *params, const double goal_xy[2], uint32_t *field_host)
{
    ARGCHK(c, c != nullptr && goal_xy != nullptr && field_host != nullptr);
    qs_plan_params p;
    int rc = plan_params(c, params, p);
    if (rc != QS_OK) return rc;
    QsPlanLayout L;
    unsigned int bbox[4];
    rc = plan_begin(c, p.clearance, 1, 0, L, bbox);
    if (rc != QS_OK) return rc;
    const size_t size = (size_t)c->cfg.size;
    std::fill(field_host, field_host + size * size, 0xffffffffu);
    if (bbox[0] > bbox[2]) return QS_OK;                  // nothing is traversable
    const double xy[4] = {goal_xy[0], goal_xy[1], goal_xy[0], goal_xy[1]};   // (start = goal: only the field is wanted)
    HIPCHK(c, hipMemcpyAsync(L.xy, xy, sizeof xy, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_plan_snap(c, L, 2, p.snap_radius));
    rc = plan_group(c, L, bbox, 1, 0, 1, 0, 0);
    if (rc != QS_OK) return rc;
    // the bounding box's cells that lie on the grid, rows of the field into rows of the host array
    const size_t x0 = (size_t)bbox[0] * 64, y0 = (size_t)bbox[1] * 64, fw = (size_t)(bbox[2] - bbox[0] + 1) * 64;
    const size_t fh = (size_t)(bbox[3] - bbox[1] + 1) * 64;
    const size_t w = std::min(fw, size - x0), h = std::min(fh, size - y0);
    HIPCHK(c, hipMemcpy2D(field_host + y0 * size + x0, size * sizeof(uint32_t), L.fields, fw * sizeof(uint32_t),
                          w * sizeof(uint32_t), h, hipMemcpyDeviceToHost));
    return QS_OK;
}

extern "C" int qs_plan_paths(qs_ctx *c, const qs_plan_params *params, const double *start_xy, const double *goal_xy, size_t n,
                             int32_t *status, int32_t *wp_cell_xy, double *wp_xy, uint32_t *cost, int32_t *path_xy,
                             size_t path_cap, int64_t *path_len, uint64_t stats[4])
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (start_xy && goal_xy && status && wp_cell_xy && wp_xy && cost));
    ARGCHK(c, path_cap == 0 || path_xy != nullptr);
    ARGCHK(c, n <= ((size_t)1 << 24));
    qs_plan_params p;
    int rc = plan_params(c, params, p);
    if (rc != QS_OK) return rc;
    QsPlanLayout L;
    unsigned int bbox[4];
    rc = plan_begin(c, p.clearance, n, path_cap, L, bbox);
    if (rc != QS_OK) return rc;
    uint64_t groups = 0;
    unsigned long long st[4] = {0, 0, 0, 0};
    std::vector<int4> out(n, make_int4(QS_PLAN_NO_START, -1, -1, -1));
    std::vector<long long> plen(n, 0);
    if (n && bbox[0] <= bbox[2]) {
        std::vector<double> xy(4 * n);
        memcpy(xy.data(), start_xy, 2 * n * sizeof(double));
        memcpy(xy.data() + 2 * n, goal_xy, 2 * n * sizeof(double));
        HIPCHK(c, hipMemcpyAsync(L.xy, xy.data(), xy.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, qs_launch_plan_snap(c, L, 2 * n, p.snap_radius));
        const size_t g = qs_plan_group(L, bbox, n);
        if (g == 0) return qs_fail(c, QS_E_STATE, "qs_plan_paths: workspace holds no field");
        for (size_t g0 = 0; g0 < n; g0 += g, groups++) {
            rc = plan_group(c, L, bbox, n, g0, std::min(g, n - g0), p.lookahead, path_cap);
            if (rc != QS_OK) return rc;
        }
        HIPCHK(c, hipMemcpyAsync(out.data(), L.out4, n * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(plen.data(), L.plen, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        if (path_cap) HIPCHK(c, hipMemcpyAsync(path_xy, L.path, n * path_cap * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st, L.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }   // (no traversable cell: every start fails to snap, QS_PLAN_NO_START, what the snap kernel would say)
    for (size_t i = 0; i < n; i++) {
        const int4 o = out[i];
        if (o.x < 0) return qs_fail(c, QS_E_STATE, "qs_plan_paths: a path walk found no descending move");
        status[i] = o.x;
        const bool ok = o.x == QS_PLAN_OK;
        wp_cell_xy[2 * i] = ok ? o.y : -1;
        wp_cell_xy[2 * i + 1] = ok ? o.z : -1;
        wp_xy[2 * i] = ok ? c->cfg.ox + (o.y + 0.5) * c->cfg.res : NAN;        // grid_to_world :127-131
        wp_xy[2 * i + 1] = ok ? c->cfg.oy + (o.z + 0.5) * c->cfg.res : NAN;
        cost[i] = ok ? (uint32_t)o.w : 0xffffffffu;
        if (path_len) path_len[i] = ok ? plen[i] : 0;
    }
    if (stats) { stats[0] = st[0]; stats[1] = st[1]; stats[2] = groups; stats[3] = st[3]; }
    return QS_OK;
}

// ---- EKF --------------------------------------------------------------------------------------------
extern "C" int qs_ekf_init(qs_ctx *c, int32_t bot, double t, const double x0[6])
{
    ARGCHK(c, c != nullptr);
    if (bot < 1 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_ekf_init: bot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    double f[44] = {0};
    for (int i = 0; i < 6; i++) { f[i] = x0 ? x0[i] : 0.0; f[6 + 7 * i] = 1.0; }     // x0, P = I  ekf.cpp:5-19
    f[42] = t; f[43] = 1.0;
    HIPCHK(c, hipMemcpyAsync(c->d_ekf.p + (size_t)bot * 44, f, sizeof f, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_ekf_step(qs_ctx *c, const int32_t *bot_ids, const double *omega_m, const double *t, const double *z_v,
                           const double *z_omega, size_t n, int32_t do_update)
{
    ARGCHK(c, c != nullptr);
    if (n == 0) return QS_OK;
    ARGCHK(c, bot_ids && omega_m && t && (!do_update || (z_v && z_omega)));
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<int> db; DevBuf<double> dd;
    HIPCHK(c, db.alloc(n));
    HIPCHK(c, dd.alloc(4 * n));
    HIPCHK(c, hipMemcpyAsync(db.p, bot_ids, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dd.p, omega_m, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dd.p + n, t, n * 8, hipMemcpyHostToDevice, c->stream));
    if (do_update) {
        HIPCHK(c, hipMemcpyAsync(dd.p + 2 * n, z_v, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dd.p + 3 * n, z_omega, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, qs_launch_ekf_step(c, db.p, dd.p, dd.p + n, dd.p + 2 * n, dd.p + 3 * n, n, do_update));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_ekf_state(qs_ctx *c, int32_t bot, double x[6], double P[36])
{
    ARGCHK(c, c != nullptr);
    if (bot < 1 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_ekf_state: bot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    double f[44];
    HIPCHK(c, hipMemcpyAsync(f, c->d_ekf.p + (size_t)bot * 44, sizeof f, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (x) memcpy(x, f, 6 * sizeof(double));
    if (P) memcpy(P, f + 6, 36 * sizeof(double));
    return QS_OK;
}

extern "C" int qs_counters(qs_ctx *c, uint64_t out[QS_CNT_N])
{
    ARGCHK(c, c != nullptr && out);
    HIPCHK(c, hipSetDevice(c->device));
    FLUSHCHK(c);
    unsigned long long v[QS_CNT_N];
    HIPCHK(c, hipMemcpyAsync(v, c->d_counters.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < QS_CNT_N; i++) out[i] = v[i];
    out[QS_CNT_REBASES] = c->n_rebases;
    out[QS_CNT_EDGE_RAYS] = c->edge_rays_total;
    out[QS_CNT_EDGE_OVERFLOW] = c->edge_overflow_total;
    return QS_OK;
}

// ---- checkpoint / restore (format and contract in include/quasar_slam.h; grid kernels in checkpoint.hip) ----------------
// The file's body (everything after the header) is assembled in one device buffer (qs_ctx::ck_stage) -- bots, counters,
// logs and block ids by device-to-device copies, the blocks by the pack kernel -- and crosses to the host in one copy; the
// host fills in the parts it holds (scalars, graph sizes) and the header.  A restore sends the body back in one copy and
// scatters it the same way.
static uint32_t ck_crc32(const uint8_t *p, size_t n)       // zlib's CRC-32 (reflected 0xEDB88320), slicing by 8
{
    static uint32_t T[8][256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            T[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < 8; s++) T[s][i] = (T[s - 1][i] >> 8) ^ T[0][T[s - 1][i] & 0xff];
    });
    uint32_t c = 0xffffffffu;
    while (n >= 8) {
        uint32_t a, b;
        memcpy(&a, p, 4); memcpy(&b, p + 4, 4);
        a ^= c;
        c = T[7][a & 0xff] ^ T[6][(a >> 8) & 0xff] ^ T[5][(a >> 16) & 0xff] ^ T[4][a >> 24] ^
            T[3][b & 0xff] ^ T[2][(b >> 8) & 0xff] ^ T[1][(b >> 16) & 0xff] ^ T[0][b >> 24];
        p += 8; n -= 8;
    }
    while (n--) c = T[0][(c ^ *p++) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

static size_t ck_pad8(size_t v) { return (v + 7) & ~(size_t)7; }
template <typename T> static void ck_put(uint8_t *b, size_t off, T v) { memcpy(b + off, &v, sizeof v); }
template <typename T> static T ck_get(const uint8_t *b, size_t off) { T v; memcpy(&v, b + off, sizeof v); return v; }

static const size_t CK_SCALARS_BYTES = 72;
static size_t ck_graph_bytes(long long L, long long C) { return 24 * (size_t)L + ck_pad8((size_t)L) + 32 * (size_t)C + ck_pad8((size_t)C); }
static size_t ck_bots_bytes(int nb) { return (size_t)nb * (1 + 2 + 1 + 4 + 44 + 4) * 8; }

// block geometry of the dirty bitmap (whether tracking is on or not)
struct CkGeom { int blocks_x, blocks_y, pitch; size_t words; };
static CkGeom ck_geom(const qs_ctx *c)
{
    CkGeom g;
    g.blocks_x = (c->cfg.size + QS_DIRTY_BLOCK_W - 1) / QS_DIRTY_BLOCK_W;
    g.blocks_y = (c->cfg.size + QS_DIRTY_BLOCK_H - 1) / QS_DIRTY_BLOCK_H;
    g.pitch = (g.blocks_x + 31) / 32;
    g.words = (size_t)g.blocks_y * g.pitch;
    return g;
}

// where the sections of a body lie: [kind] -> (offset, length), offsets from the start of the file
struct CkLayout {
    size_t off[QS_CKPT_DIRTY + 1] = {0}, len[QS_CKPT_DIRTY + 1] = {0};
    size_t header_bytes = 0, total = 0;
    int n_sections = 0;
};
static CkLayout ck_layout(int nb, int n_graphs, const std::vector<long long> &L, const std::vector<long long> &C, size_t n_blocks,
                          size_t block_bytes, bool tracking, size_t dirty_words)
{
    CkLayout y;
    y.n_sections = tracking ? 7 : 6;
    y.header_bytes = QS_CKPT_HEADER_FIXED + 24 * (size_t)y.n_sections;
    y.len[QS_CKPT_SCALARS] = CK_SCALARS_BYTES;
    y.len[QS_CKPT_BOTS] = ck_bots_bytes(nb);
    y.len[QS_CKPT_COUNTERS] = QS_CNT_N * 8;
    size_t gb = (size_t)n_graphs * 24;
    for (int g = 0; g < n_graphs; g++) gb += ck_graph_bytes(L[g], C[g]);
    y.len[QS_CKPT_GRAPHS] = gb;
    y.len[QS_CKPT_BLOCK_IDS] = 4 * n_blocks;
    y.len[QS_CKPT_BLOCKS] = n_blocks * block_bytes;
    y.len[QS_CKPT_DIRTY] = tracking ? 4 * dirty_words : 0;
    size_t at = y.header_bytes;
    for (int k = QS_CKPT_SCALARS; k <= (tracking ? QS_CKPT_DIRTY : QS_CKPT_BLOCKS); k++) { y.off[k] = at; at += ck_pad8(y.len[k]); }
    y.total = at;
    return y;
}

// the configuration fields a checkpoint must agree on (include/quasar_slam.h), at their header offsets
struct CkField { const char *name; int off; bool is_f64; };
static const CkField CK_FIELDS[] = {
    {"size", 32, false}, {"min_poses_between", 36, false}, {"max_agent", 40, false}, {"bots_per_graph", 44, false},
    {"enable_counts", 48, false}, {"enable_ekf", 52, false}, {"seq_stride", 56, false}, {"shard_bots", 60, false},
    {"shard_rank", 64, false}, {"exact_trig", 68, false},
    {"res", 80, true}, {"ox", 88, true}, {"oy", 96, true}, {"min_dist", 104, true}, {"max_dist", 112, true},
    {"closure_radius", 120, true}, {"closure_correction", 128, true}, {"ekf_metres_per_tick", 136, true}};
static void ck_put_config(uint8_t *h, const qs_config &cf, bool tracking)
{
    const int32_t iv[12] = {cf.size, cf.min_poses_between, cf.max_agent, cf.bots_per_graph, cf.enable_counts ? 1 : 0,
                            cf.enable_ekf ? 1 : 0, cf.seq_stride, cf.shard_bots, cf.shard_rank, cf.exact_trig ? 1 : 0,
                            tracking ? 1 : 0, 0};
    const double dv[8] = {cf.res, cf.ox, cf.oy, cf.min_dist, cf.max_dist, cf.closure_radius, cf.closure_correction,
                          cf.ekf_metres_per_tick};
    memcpy(h + 32, iv, sizeof iv);
    memcpy(h + 80, dv, sizeof dv);
}

static int ck_planes(bool counts, bool tracking) { return !counts ? 1 : (tracking ? 4 : 2); }

extern "C" int qs_checkpoint(qs_ctx *c, uint8_t *buf, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->sf_state != 0) return qs_fail(c, QS_E_STATE, "qs_checkpoint: a sparse fuse is in flight (finish it with qs_sparse_fuse_apply)");
    FLUSHCHK(c);                                             // waiting exact-trig rays go into the saved grid
    unsigned long long cnt[QS_CNT_N];
    std::vector<QsGraphDev> cur((size_t)c->n_graphs);
    HIPCHK(c, hipMemcpyAsync(cnt, c->d_counters.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cur.data(), c->d_graphs.p, cur.size() * sizeof(QsGraphDev), hipMemcpyDeviceToHost, c->stream));
    // census: the blocks that hold anything, listed on the device
    const CkGeom gm = ck_geom(c);
    HIPCHK(c, c->ck_census.reserve(gm.words * 33 + 1, c->stream));
    unsigned int *d_bm = c->ck_census.p, *d_list = d_bm + gm.words, *d_count = d_list + gm.words * 32;
    HIPCHK(c, qs_launch_ck_census(c, d_bm, gm.words, gm.pitch, gm.blocks_x, d_list, d_count));
    unsigned int n_blk = 0;
    HIPCHK(c, hipMemcpyAsync(&n_blk, d_count, sizeof n_blk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (cnt[QS_CNT_SLAM_ROUNDS] >> 40)
        return qs_fail(c, QS_E_STATE, "qs_checkpoint: a loop-closure chain wait timed out (bit 40 of QS_CNT_SLAM_ROUNDS): the map may be wrong");
    const bool tracking = c->d_dirty.p != nullptr;
    const int planes = ck_planes(c->d_counts.p != nullptr, tracking), nb = c->cfg.max_agent + 1, G = c->n_graphs;
    std::vector<long long> L(G), C(G);
    for (int g = 0; g < G; g++) {
        L[g] = cur[g].n_lms; C[g] = cur[g].n_cls;
        if (L[g] > cur[g].cap_lms || C[g] > cur[g].cap_cls)
            return qs_fail(c, QS_E_STATE, "qs_checkpoint: a pose graph's log outgrew its capacity: the map may be wrong");
    }
    const CkLayout y = ck_layout(nb, G, L, C, n_blk, qs_ck_block_bytes(planes), tracking, gm.words);
    *n_out = y.total;
    if (!buf) return QS_OK;
    if (cap < y.total) return qs_fail(c, QS_E_RANGE, "qs_checkpoint: cap is below the checkpoint's size (query it with buf == NULL)");
    // the body on the device, offsets relative to header_bytes
    const size_t hb = y.header_bytes, body = y.total - hb;
    HIPCHK(c, c->ck_stage.reserve(body, c->stream));
    unsigned char *st = c->ck_stage.p;
    auto d2d = [&](size_t off, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(st + off - hb, src, bytes, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    };
    {
        size_t o = y.off[QS_CKPT_BOTS];
        HIPCHK(c, d2d(o, c->d_offset.p, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(o, c->d_drift.p, nb * 16)); o += nb * 16;
        HIPCHK(c, d2d(o, c->d_last_closure.p, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(o, c->d_zone.p, nb * 32)); o += nb * 32;
        HIPCHK(c, d2d(o, c->d_ekf.p, (size_t)nb * 44 * 8)); o += (size_t)nb * 44 * 8;
        HIPCHK(c, d2d(o, c->d_ekf_prev.p, nb * 32));
    }
    HIPCHK(c, d2d(y.off[QS_CKPT_COUNTERS], c->d_counters.p, QS_CNT_N * 8));
    {
        size_t o = y.off[QS_CKPT_GRAPHS] + (size_t)G * 24;
        for (int g = 0; g < G; g++) {
            const QsGraphDev &q = cur[g];
            const size_t l = (size_t)L[g], k = (size_t)C[g];
            HIPCHK(c, d2d(o, q.lm_x, 8 * l)); HIPCHK(c, d2d(o + 8 * l, q.lm_y, 8 * l)); HIPCHK(c, d2d(o + 16 * l, q.lm_idx, 8 * l));
            HIPCHK(c, d2d(o + 24 * l, q.lm_type, l));
            o += 24 * l + ck_pad8(l);
            HIPCHK(c, d2d(o, q.cl_lm_idx, 8 * k)); HIPCHK(c, d2d(o + 8 * k, q.cl_node_idx, 8 * k));
            HIPCHK(c, d2d(o + 16 * k, q.cl_dx, 8 * k)); HIPCHK(c, d2d(o + 24 * k, q.cl_dy, 8 * k));
            HIPCHK(c, d2d(o + 32 * k, q.cl_agent, k));
            o += 32 * k + ck_pad8(k);
        }
    }
    HIPCHK(c, d2d(y.off[QS_CKPT_BLOCK_IDS], d_list, 4 * (size_t)n_blk));
    HIPCHK(c, qs_launch_ck_pack(c, d_list, n_blk, gm.pitch, planes, st + y.off[QS_CKPT_BLOCKS] - hb));
    if (tracking) HIPCHK(c, d2d(y.off[QS_CKPT_DIRTY], c->d_dirty.p, 4 * gm.words));
    memset(buf, 0, hb);
    HIPCHK(c, hipMemcpyAsync(buf + hb, st, body, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // what the host holds, then the header
    {
        uint8_t *s = buf + y.off[QS_CKPT_SCALARS];
        memset(s, 0, ck_pad8(CK_SCALARS_BYTES));
        ck_put<uint64_t>(s, 0, c->next_seq); ck_put<uint64_t>(s, 8, c->epoch_base); ck_put<uint64_t>(s, 16, c->n_rebases);
        ck_put<uint64_t>(s, 24, c->edge_rays_total); ck_put<uint64_t>(s, 32, c->edge_overflow_total);
        ck_put<double>(s, 40, c->sweep_min); ck_put<double>(s, 48, c->sweep_max);
        ck_put<uint32_t>(s, 56, c->dirty_since_fuse ? 1u : 0u); ck_put<uint32_t>(s, 60, c->counts_view_fused ? 1u : 0u);
        ck_put<uint32_t>(s, 64, (uint32_t)G); ck_put<uint32_t>(s, 68, (uint32_t)nb);
        uint8_t *gh = buf + y.off[QS_CKPT_GRAPHS];
        for (int g = 0; g < G; g++) {
            ck_put<int64_t>(gh, 24 * g, cur[g].n_nodes); ck_put<int64_t>(gh, 24 * g + 8, L[g]); ck_put<int64_t>(gh, 24 * g + 16, C[g]);
        }
        // padding after the host-side arrays and the byte arrays: zeros, so that equal sessions give equal files
        for (int k = QS_CKPT_SCALARS; k <= QS_CKPT_DIRTY; k++)
            if (y.off[k]) memset(buf + y.off[k] + y.len[k], 0, ck_pad8(y.len[k]) - y.len[k]);
        size_t o = y.off[QS_CKPT_GRAPHS] + (size_t)G * 24;
        for (int g = 0; g < G; g++) {
            const size_t l = (size_t)L[g], k = (size_t)C[g];
            memset(buf + o + 24 * l + l, 0, ck_pad8(l) - l); o += 24 * l + ck_pad8(l);
            memset(buf + o + 32 * k + k, 0, ck_pad8(k) - k); o += 32 * k + ck_pad8(k);
        }
    }
    memcpy(buf, QS_CKPT_MAGIC, 4);
    ck_put<uint32_t>(buf, 4, QS_CKPT_VERSION); ck_put<uint32_t>(buf, 8, (uint32_t)hb); ck_put<uint32_t>(buf, 12, (uint32_t)y.n_sections);
    ck_put<uint64_t>(buf, 16, y.total);
    ck_put_config(buf, c->cfg, tracking);
    for (int k = QS_CKPT_SCALARS, i = 0; i < y.n_sections; k++, i++) {
        const size_t e = QS_CKPT_HEADER_FIXED + 24 * (size_t)i;
        ck_put<uint32_t>(buf, e, (uint32_t)k); ck_put<uint64_t>(buf, e + 8, y.off[k]); ck_put<uint64_t>(buf, e + 16, y.len[k]);
    }
    ck_put<uint32_t>(buf, 24, ck_crc32(buf + hb, body));
    return QS_OK;
}

// everything qs_restore changes, after the host-side checks: on failure the caller resets the context
static int ck_apply(qs_ctx *c, const uint8_t *buf, const CkLayout &y, bool tracking, int planes, const CkGeom &gm,
                    const std::vector<long long> &L, const std::vector<long long> &C, const std::vector<long long> &N, size_t n_blk)
{
    int rc = reset_state(c);
    if (rc != QS_OK) return rc;
    if (tracking != (c->d_dirty.p != nullptr)) {
        rc = qs_dirty_tracking(c, tracking ? 1 : 0);          // (after the reset: no unfused writes, sequence counter 0)
        if (rc != QS_OK) return rc;
    }
    const int G = c->n_graphs, nb = c->cfg.max_agent + 1;
    for (int g = 0; g < G; g++) {                            // the logs' capacities (nothing to keep: the graphs are reset)
        rc = graph_reserve(c, g, L[g], C[g], 0, 0);
        if (rc != QS_OK) return rc;
    }
    const size_t hb = y.header_bytes, body = y.total - hb;
    HIPCHK(c, c->ck_stage.reserve(body, c->stream));
    unsigned char *st = c->ck_stage.p;
    HIPCHK(c, hipMemcpyAsync(st, buf + hb, body, hipMemcpyHostToDevice, c->stream));
    auto d2d = [&](void *dst, size_t off, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, st + off - hb, bytes, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    };
    {
        size_t o = y.off[QS_CKPT_BOTS];
        HIPCHK(c, d2d(c->d_offset.p, o, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(c->d_drift.p, o, nb * 16)); o += nb * 16;
        HIPCHK(c, d2d(c->d_last_closure.p, o, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(c->d_zone.p, o, nb * 32)); o += nb * 32;
        HIPCHK(c, d2d(c->d_ekf.p, o, (size_t)nb * 44 * 8)); o += (size_t)nb * 44 * 8;
        HIPCHK(c, d2d(c->d_ekf_prev.p, o, nb * 32));
    }
    HIPCHK(c, d2d(c->d_counters.p, y.off[QS_CKPT_COUNTERS], QS_CNT_N * 8));
    const unsigned int *d_list = (const unsigned int *)(st + y.off[QS_CKPT_BLOCK_IDS] - hb);
    HIPCHK(c, qs_launch_ck_unpack(c, d_list, (unsigned int)n_blk, gm.pitch, planes, st + y.off[QS_CKPT_BLOCKS] - hb));
    if (tracking) HIPCHK(c, d2d(c->d_dirty.p, y.off[QS_CKPT_DIRTY], 4 * gm.words));
    // closure logs in place; landmark logs through the index rebuild (slam.hip), which appends them again
    std::vector<QsIndexLog> logs((size_t)G);
    {
        size_t o = y.off[QS_CKPT_GRAPHS] + (size_t)G * 24;
        for (int g = 0; g < G; g++) {
            const QsGraphBufs &q = c->graphs[g];
            const size_t l = (size_t)L[g], k = (size_t)C[g];
            const unsigned char *s = st + o - hb;
            logs[g] = QsIndexLog{(const double *)s, (const double *)(s + 8 * l), (const long long *)(s + 16 * l), s + 24 * l,
                                 L[g], N[g], C[g]};
            o += 24 * l + ck_pad8(l);
            HIPCHK(c, d2d(q.cl_lm_idx.p, o, 8 * k)); HIPCHK(c, d2d(q.cl_node_idx.p, o + 8 * k, 8 * k));
            HIPCHK(c, d2d(q.cl_dx.p, o + 16 * k, 8 * k)); HIPCHK(c, d2d(q.cl_dy.p, o + 24 * k, 8 * k));
            HIPCHK(c, d2d(q.cl_agent.p, o + 32 * k, k));
            o += 32 * k + ck_pad8(k);
        }
    }
    DevBuf<QsIndexLog> d_logs;
    HIPCHK(c, d_logs.alloc((size_t)G));
    HIPCHK(c, hipMemcpyAsync(d_logs.p, logs.data(), (size_t)G * sizeof(QsIndexLog), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_slam_rebuild_index(c, d_logs.p));
    HIPCHK(c, hipStreamSynchronize(c->stream));              // (d_logs and the caller's buffer go out of use)
    const uint8_t *s = buf + y.off[QS_CKPT_SCALARS];
    c->next_seq = ck_get<uint64_t>(s, 0); c->epoch_base = ck_get<uint64_t>(s, 8); c->n_rebases = ck_get<uint64_t>(s, 16);
    c->edge_rays_total = ck_get<uint64_t>(s, 24); c->edge_overflow_total = ck_get<uint64_t>(s, 32);
    c->sweep_min = ck_get<double>(s, 40); c->sweep_max = ck_get<double>(s, 48);
    c->dirty_since_fuse = ck_get<uint32_t>(s, 56) != 0;
    c->counts_view_fused = tracking && c->d_counts.p && ck_get<uint32_t>(s, 60) != 0;   // (the dense snapshot is not saved)
    // the graphs' real counts and the pile flag the rebuild left, as at any synchronisation point
    return read_pile_flag(c);
}

extern "C" int qs_restore(qs_ctx *c, const uint8_t *buf, size_t n)
{
    ARGCHK(c, c != nullptr && buf != nullptr);
    char msg[256];
#define CK_BAD(...) do { snprintf(msg, sizeof msg, __VA_ARGS__); return qs_fail(c, QS_E_INVAL, msg); } while (0)
    if (n < QS_CKPT_HEADER_FIXED) CK_BAD("qs_restore: truncated header (%zu bytes)", n);
    if (memcmp(buf, QS_CKPT_MAGIC, 4) != 0) CK_BAD("qs_restore: bad magic (not a checkpoint)");
    const uint32_t version = ck_get<uint32_t>(buf, 4);
    if (version != QS_CKPT_VERSION) CK_BAD("qs_restore: unknown format version %u (this library reads %d)", version, QS_CKPT_VERSION);
    const uint32_t hb = ck_get<uint32_t>(buf, 8), n_sec = ck_get<uint32_t>(buf, 12);
    const uint64_t total = ck_get<uint64_t>(buf, 16);
    if ((n_sec != 6 && n_sec != 7) || hb != QS_CKPT_HEADER_FIXED + 24 * n_sec || n < hb) CK_BAD("qs_restore: bad header or section table");
    if (total != n) CK_BAD("qs_restore: length %zu does not match the header's %llu (truncated?)", n, (unsigned long long)total);
    if (ck_crc32(buf + hb, n - hb) != ck_get<uint32_t>(buf, 24)) CK_BAD("qs_restore: CRC mismatch (corrupted checkpoint)");
    // configuration: every field that changes a result
    const bool tracking = ck_get<int32_t>(buf, 72) != 0;
    uint8_t mine[QS_CKPT_HEADER_FIXED];
    memset(mine, 0, sizeof mine);
    ck_put_config(mine, c->cfg, tracking);
    for (const CkField &f : CK_FIELDS) {
        if (memcmp(buf + f.off, mine + f.off, f.is_f64 ? 8 : 4) == 0) continue;
        if (f.is_f64) CK_BAD("qs_restore: configuration field '%s' does not match (checkpoint %.17g, context %.17g)", f.name,
                             ck_get<double>(buf, f.off), ck_get<double>(mine, f.off));
        CK_BAD("qs_restore: configuration field '%s' does not match (checkpoint %d, context %d)", f.name, ck_get<int32_t>(buf, f.off),
               ck_get<int32_t>(mine, f.off));
    }
    if (c->sf_state != 0) return qs_fail(c, QS_E_STATE, "qs_restore: a sparse fuse is in flight (finish it with qs_sparse_fuse_apply)");
    // sections: the table against the layout the section contents imply
    size_t off[QS_CKPT_DIRTY + 1] = {0}, len[QS_CKPT_DIRTY + 1] = {0};
    for (uint32_t i = 0; i < n_sec; i++) {
        const size_t e = QS_CKPT_HEADER_FIXED + 24 * (size_t)i;
        const uint32_t kind = ck_get<uint32_t>(buf, e);
        const uint64_t o = ck_get<uint64_t>(buf, e + 8), l = ck_get<uint64_t>(buf, e + 16);
        if (kind < QS_CKPT_SCALARS || kind > QS_CKPT_DIRTY || off[kind] || o < hb || o % 8 || o > n || l > n - o)
            CK_BAD("qs_restore: bad section table entry %u", i);
        off[kind] = (size_t)o; len[kind] = (size_t)l;
    }
    const int G = c->n_graphs, nb = c->cfg.max_agent + 1;
    if (!off[QS_CKPT_SCALARS] || len[QS_CKPT_SCALARS] != CK_SCALARS_BYTES) CK_BAD("qs_restore: bad scalars section");
    if (ck_get<uint32_t>(buf, off[QS_CKPT_SCALARS] + 64) != (uint32_t)G || ck_get<uint32_t>(buf, off[QS_CKPT_SCALARS] + 68) != (uint32_t)nb)
        CK_BAD("qs_restore: graph / bot counts do not match");
    if (!off[QS_CKPT_GRAPHS] || len[QS_CKPT_GRAPHS] < (size_t)G * 24) CK_BAD("qs_restore: truncated graphs section");
    std::vector<long long> L(G), C(G), N(G);
    for (int g = 0; g < G; g++) {
        N[g] = ck_get<int64_t>(buf, off[QS_CKPT_GRAPHS] + 24 * g);
        L[g] = ck_get<int64_t>(buf, off[QS_CKPT_GRAPHS] + 24 * g + 8);
        C[g] = ck_get<int64_t>(buf, off[QS_CKPT_GRAPHS] + 24 * g + 16);
        if (N[g] < 0 || L[g] < 0 || C[g] < 0 || L[g] > N[g] || C[g] > N[g] || (uint64_t)L[g] > n || (uint64_t)C[g] > n)
            CK_BAD("qs_restore: bad sizes of graph %d", g);
    }
    const CkGeom gm = ck_geom(c);
    const int planes = ck_planes(c->d_counts.p != nullptr, tracking);
    const size_t n_blk = len[QS_CKPT_BLOCK_IDS] / 4;
    const CkLayout y = ck_layout(nb, G, L, C, n_blk, qs_ck_block_bytes(planes), tracking, gm.words);
    if (y.header_bytes != hb || y.total != n || y.n_sections != (int)n_sec) CK_BAD("qs_restore: section lengths do not add up");
    for (int k = QS_CKPT_SCALARS; k <= (tracking ? QS_CKPT_DIRTY : QS_CKPT_BLOCKS); k++)
        if (off[k] != y.off[k] || len[k] != y.len[k]) CK_BAD("qs_restore: section %d has the wrong offset or length", k);
    // block ids: ascending, every one a block of this grid (the unpack kernel writes where they point)
    {
        const uint8_t *ids = buf + off[QS_CKPT_BLOCK_IDS];
        long long prev = -1;
        for (size_t i = 0; i < n_blk; i++) {
            const uint32_t b = ck_get<uint32_t>(ids, 4 * i);
            const uint32_t by = b / (uint32_t)(32 * gm.pitch), bx = b % (uint32_t)(32 * gm.pitch);
            if ((long long)b <= prev || by >= (uint32_t)gm.blocks_y || bx >= (uint32_t)gm.blocks_x) CK_BAD("qs_restore: bad block id at %zu", i);
            prev = b;
        }
    }
#undef CK_BAD
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = ck_apply(c, buf, y, tracking, planes, gm, L, C, N, n_blk);
    if (rc != QS_OK) {                                       // half-restored: leave what a new context would show
        const std::string e = c->err;
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        reset_state(c);
        c->err = e;
    }
    return rc;
}
