// qs_api.hip -- the core of the C ABI of include/quasar_slam.h: context, device memory, the sync point, and the per-batch
// pipeline  decode (K0) -> SLAM drift (K4) -> raycast (K1) [-> EKF (K5)]  on one HIP stream.  The entry points of the
// other subsystems live next to their kernels (sweep.hip, grid_ops.hip, sparse_fuse.hip, checkpoint.hip, frontier*.hip,
// plan.hip, icp.hip, ekf.hip, diag.hip) and share the helpers declared in qs_internal.h's "host side of the C ABI".
#include <math.h>
#include <algorithm>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qs_internal.h"
#include "raycast_common.h"

static thread_local std::string g_create_err;

int qs_fail(qs_ctx *c, int code, const char *what, hipError_t e)
{
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

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

double r2_threshold_for(double radius)
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

int graph_reserve(qs_ctx *c, int g, long long need_lms, long long need_cls, long long have_lms, long long have_cls)
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

int reset_state(qs_ctx *c)
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
    c->last_sweeps = false; c->last_sweeps_n = 0; c->last_matches = false; c->last_matches_n = 0;
    c->last_checks = false; c->last_checks_n = 0;
    c->pile_mode = false;
    c->edge_maybe = false; c->edge_overflow_total = 0;      // (rays still waiting belonged to the old session: the flags are cleared above)
    if (c->veil_tab.p) {                                    // bot veil, V2: an empty table (the setting itself is kept)
        HIPCHK(c, hipMemsetAsync(c->veil_tab.p, 0, c->veil_tab.cap * sizeof(int4), c->stream));
        HIPCHK(c, hipMemsetAsync(c->veil_total.p, 0, sizeof(unsigned long long), c->stream));
    }
    c->last_veil = false;
    c->last_sveil = false;
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
    CREATE_CHK(c->d_scout.alloc(2));
    CREATE_CHK(hipMemset(c->d_scout.p, 0, 2 * sizeof(unsigned int)));
    CREATE_CHK(hipHostMalloc((void **)&c->h_chain_stat, 8 * sizeof(unsigned int), hipHostMallocDefault));
    memset(c->h_chain_stat, 0, 8 * sizeof(unsigned int));
    CREATE_CHK(hipEventCreateWithFlags(&c->ev_chain_stat, hipEventDisableTiming));
    if (const char *e = getenv("QS_CHAIN_SCOUT")) c->chain_scout = strcmp(e, "1") == 0;          // (qs_set_chain_scout's default, for A/B runs)
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

extern "C" int qs_set_chain_lean(qs_ctx *c, int32_t mode, int64_t limit)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, mode == QS_CHAIN_LEAN_AUTO || mode == QS_CHAIN_LEAN_OFF);
    c->chain_lean_mode = mode;
    c->chain_lean_limit = limit > 0 && limit < 0x7f7f7f7fll ? limit : 0x7f7f7f7fll;
    return QS_OK;
}

extern "C" int qs_chain_lean(qs_ctx *c)
{
    if (!c) return QS_E_INVAL;
    if (!c->chain_last_lean_asked) return 0;
    unsigned int refused = 0;
    HIPCHK(c, hipMemcpyAsync(&refused, c->d_flags.p + QS_FLAG_CHAIN_FULL, sizeof refused, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return refused != c->chain_lean_seq ? 1 : 0;
}

extern "C" int qs_set_chain_plan(qs_ctx *c, int32_t on)
{
    ARGCHK(c, c != nullptr);
    c->chain_plan = on != 0;
    return QS_OK;
}

extern "C" int qs_chain_plan(qs_ctx *c)
{
    if (!c) return QS_E_INVAL;
    if (!c->chain_last_plan) return 0;
    return qs_chain_lean(c);                     // (a plan was built: walked by every graph that ran the lean owner)
}

// diagnostic: bot's part of the plan the last launch built (the batch arrays keep it until the next ingest writes them again)
extern "C" int qs_chain_plan_read(qs_ctx *c, int32_t bot, int32_t *node, uint32_t *r, uint32_t *skip, size_t cap, size_t *n_own,
                                  uint32_t *first)
{
    ARGCHK(c, c != nullptr && n_own && first);
    ARGCHK(c, (node && r && skip) || (!node && !r && !skip));
    if (bot < 1 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_chain_plan_read: bot out of range");
    if (!c->chain_last_plan) return qs_fail(c, QS_E_STATE, "qs_chain_plan_read: the last ingest had no plan");
    HIPCHK(c, hipSetDevice(c->device));
    unsigned int range[2] = {0, 0}, f = 0;
    HIPCHK(c, hipMemcpyAsync(range, c->sb.agent_ev + bot, sizeof range, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&f, c->sb.pl_first + bot, sizeof f, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n = range[1] - range[0];
    *n_own = n; *first = f;
    if (!node) return QS_OK;
    if (n > cap) return qs_fail(c, QS_E_RANGE, "qs_chain_plan_read: capacity too small");
    std::vector<QsPlanRec> rec(n);
    if (n) HIPCHK(c, hipMemcpy(rec.data(), c->sb.pl_rec + range[0], n * sizeof(QsPlanRec), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) { node[i] = rec[i].node; r[i] = rec[i].r; skip[i] = rec[i].skip; }
    return QS_OK;
}

extern "C" int qs_set_chain_lookahead(qs_ctx *c, int32_t on)
{
    ARGCHK(c, c != nullptr);
    c->chain_lookahead = on != 0;
    return QS_OK;
}

extern "C" int qs_chain_lookahead(qs_ctx *c)
{
    if (!c) return QS_E_INVAL;
    return c->chain_lookahead ? 1 : 0;
}

extern "C" int qs_set_chain_scout(qs_ctx *c, int32_t on)
{
    ARGCHK(c, c != nullptr);
    c->chain_scout = on != 0;
    return QS_OK;
}

extern "C" int qs_chain_scout(qs_ctx *c, uint64_t *staged, uint64_t *fallback)
{
    ARGCHK(c, c != nullptr && staged && fallback);
    *staged = 0; *fallback = 0;
    if (!c->chain_last_scout) return QS_OK;      // (no launch yet, or one without scouts)
    HIPCHK(c, hipSetDevice(c->device));
    unsigned int cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(cnt, c->d_scout.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *staged = cnt[0]; *fallback = cnt[1];
    return QS_OK;
}

extern "C" int qs_sync(qs_ctx *c)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
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
    sb.pl_rec = k.take<QsPlanRec>(cap); sb.pl_blk = k.take<unsigned int>(nb * (size_t)qs_slam_plan_blocks(cap));
    sb.pl_first = k.take<unsigned int>(nb);
    return k.bytes;
}

int ensure_batch(qs_ctx *c, size_t n)
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
int ensure_epoch(qs_ctx *c, uint64_t seq0, size_t n_seq)
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
        SYNCCHK(c);                                         // waiting rays carry stamps of the epoch that ends here
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

int sync_host_state(qs_ctx *c, bool host_waits)
{
    if (host_waits) c->flags_maybe = true;
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
        const QsRange g = sweep ? qs_range_rule(dd, c->sweep_min, c->sweep_max) : qs_range_rule(dd, c->cfg.min_dist, c->cfg.max_dist);
        h[4 * e] = r.rx + g.range * cos(a);                                                    // :890 / :901 (libm: what this mode is for)
        h[4 * e + 1] = r.ry + g.range * sin(a);                                                // :891 / :902
        h[4 * e + 2] = g.valid ? 1.0 : 0.0;
        h[4 * e + 3] = 0.0;
    }
    HIPCHK(c, hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_edge_cast(c, n_edge, d));
    HIPCHK(c, hipMemsetAsync(c->d_flags.p, 0, sizeof(unsigned int), c->stream));                 // the list is empty again
    HIPCHK(c, hipMemsetAsync(c->d_flags.p + 2, 0, sizeof(unsigned int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                                // h goes out of scope
    return QS_OK;
}

int qs_batch_prepare(qs_ctx *c, size_t n)
{
    int rc = ensure_batch(c, n);
    if (rc != QS_OK) return rc;
    c->b.n = n;
    HIPCHK(c, hipMemsetAsync(c->d_graph_batch.p, 0, (size_t)c->n_graphs * 2 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->sb.agent_ev, 0, ((size_t)c->cfg.max_agent + 2) * sizeof(unsigned int), c->stream));
    return QS_OK;
}

int qs_batch_slam(qs_ctx *c, size_t n)
{
    int rc = reserve_graphs_for_batch(c, n);
    if (rc != QS_OK) return rc;
    chain_stats_poll(c, false, nullptr);
    { StageTimer t(c, QS_STAGE_SLAM); HIPCHK(c, qs_launch_slam(c, n)); t.stop(); }
    c->flags_maybe = true;
    return chain_stats_request(c);
}

static int ingest_device(qs_ctx *c, const uint8_t *d_pkts, size_t n, size_t stride, const uint16_t *d_lens,
                         const double *d_time, uint64_t seq0)
{
    if (seq0 == UINT64_MAX) seq0 = c->next_seq;
    c->last_n = n; c->last_has_poses = true; c->last_sweeps = false; c->last_matches = false; c->last_checks = false;
    c->last_veil = c->veil_radius > 0 && n > 0;
    if (n == 0) return QS_OK;
    int rc = qs_batch_prepare(c, n);
    if (rc != QS_OK) return rc;
    const uint64_t sstride = c->cfg.seq_stride > 0 ? (uint64_t)c->cfg.seq_stride : 1;
    // epoch decisions use the stride-aligned range so that all ranks of a sharded stream agree
    rc = ensure_epoch(c, seq0 - seq0 % sstride, n * sstride);
    if (rc != QS_OK) return rc;
    { StageTimer t(c, QS_STAGE_DECODE); HIPCHK(c, qs_launch_decode(c, d_pkts, n, stride, d_lens)); t.stop(); }
    if (c->cfg.enable_ekf) {
        // fork: the filter only needs the decoded fields, never the map (and the map never the filter)
        if (!c->ekf_stream) { int rce = ekf_stream_acquire(c); if (rce != QS_OK) return rce; }
        HIPCHK(c, hipEventRecord(c->ev_decoded, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->ekf_stream, c->ev_decoded, 0));
        { StageTimer t(c, QS_STAGE_EKF, c->ekf_stream); HIPCHK(c, n >= QS_EKF_SCAN_MIN_BATCH ? qs_launch_ekf_scan(c, n, d_time, c->ekf_stream)
                                                   : qs_launch_ekf_ingest(c, n, d_time, c->ekf_stream)); t.stop(); }
        HIPCHK(c, hipEventRecord(c->ev_ekf_done, c->ekf_stream));
    }
    rc = qs_batch_slam(c, n);
    if (rc != QS_OK) return rc;
    {
        StageTimer t(c, QS_STAGE_RAYCAST);
        // auto (0): a handful of packets (the live UDP path: <= 20 per frame) is one direct kernel instead
        // of the four tiled passes -- same cells either way; 1 = always direct, 2 = always tiled
        // (a veiled context always takes the tiled form: the direct kernel writes the end cell before anything could veil it)
        if (c->cfg.raycast_mode == 1 || (c->cfg.raycast_mode == 0 && n <= QS_DIRECT_MAX_BATCH && c->veil_radius == 0))
            HIPCHK(c, qs_launch_raycast_direct(c, n, seq0));
        else HIPCHK(c, qs_launch_raycast_tiled(c, n, seq0));
        t.stop();
    }
    if (c->cfg.enable_ekf) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ekf_done, 0));   // join
    if (c->b.edge) c->edge_maybe = true;                 // resolved at the next point the map is observed (sync_host_state)
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

static size_t staging_layout(void *base, size_t cap, Staging &s)
{
    Carve k(base);
    s.pkts = k.take<unsigned char>(cap);
    s.lens = k.take<unsigned short>(cap / QS_PACKET_SIZE_V1 + 1);
    s.time = k.take<double>(cap / QS_PACKET_SIZE_V1 + 1);
    return k.bytes;
}

int reserve_staging(qs_ctx *c, size_t bytes, Staging &s)
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
    return sync_host_state(c, true);
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
    c->last_has_poses = false; c->last_sweeps = false; c->last_matches = false; c->last_checks = false;
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

extern "C" int qs_device_buffers(qs_ctx *c, void **stamps_dev, size_t *stamps_bytes, void **counts_dev, size_t *counts_bytes)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);                                   // whoever gets the buffers may read them (a collective)
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
    rc = sync_host_state(c, true);
    if (rc != QS_OK) return rc;
    c->last_has_poses = false; c->last_sweep_graph = false;      // (the batch arrays are this call's now)
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
    SYNCCHK(c);
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
        { HIPCHK(dst, hipSetDevice(s->device)); int rcs = sync_host_state(s, false); if (rcs != QS_OK) return qs_fail(dst, rcs, s->err.c_str()); }
        HIPCHK(dst, hipStreamSynchronize(s->stream));
        st[i] = s->d_stamps.p; ct[i] = s->d_counts.p;
        if (!s->d_counts.p) counts = false;
    }
    int rc = qs_fuse_buffers(dst, st.data(), counts ? ct.data() : nullptr, n);
    if (rc != QS_OK) return rc;
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    return QS_OK;
}

extern "C" int qs_counters(qs_ctx *c, uint64_t out[QS_CNT_N])
{
    ARGCHK(c, c != nullptr && out);
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    unsigned long long v[QS_CNT_N];
    HIPCHK(c, hipMemcpyAsync(v, c->d_counters.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < QS_CNT_N; i++) out[i] = v[i];
    out[QS_CNT_REBASES] = c->n_rebases;
    out[QS_CNT_EDGE_RAYS] = c->edge_rays_total;
    out[QS_CNT_EDGE_OVERFLOW] = c->edge_overflow_total;
    return QS_OK;
}
