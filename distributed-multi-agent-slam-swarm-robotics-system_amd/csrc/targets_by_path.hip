// targets_by_path.hip -- frontier targets ranked by path cost over the mapped free space.
// The rules are this build's own (include/quasar_slam.h, "frontier targets by path cost"), all integer once the centroids
// exist.  The centroids are frontier_targets.hip's; the mask, the census, the snap, the fields and the walk are plan.hip's
// (plan_common.h).  New here is the stage between them:
//
//   cells    : the centroids and the bots snap in ONE launch of the planner's snap kernel; a second kernel turns the
//              centroids' cells into offsets into a field (the bounding box of the census) and counts who has a cell;
//   fields   : one field per bot with a cell, seeded at the bot (the moves are symmetric: the field of a bot's cell holds
//              the cost to every cell), in groups that fit QS_PLAN_WS_CAP, relaxed by the planner's host-driven rounds;
//   gather   : while a group's fields are resident, one wave per (bot, chunk of TP_CHUNK centroids): lanes read the
//              centroids' offsets coalesced, gather field[offset], and the wave keeps the TP_K smallest 64-bit keys
//              (cost << 32) | k in a sorted list across lanes 0..TP_K-1 (ballot insertion, one shfl_up).  Infinite costs
//              never enter a list.  One wave per bot then merges its chunk lists into the exact top-K;
//   greedy   : ONE wave walks the bots in order; a bot takes the first entry of its list that is neither taken nor within
//              `separation` of a target assigned so far (frontier_targets.hip's fp64 test).  The list is the true top-K by
//              the key the rule orders by, so its first eligible entry is the minimum over every eligible centroid.  When a
//              full list is entirely ineligible the pass stops: the host recomputes that bot's field, a whole-GPU scan over
//              all centroids finds its pick, and the pass resumes (counted in stats);
//   waypoints: the body of qs_plan_paths for the assigned pairs: fields seeded at the assigned centroids' cells, the walk.
// No device-side waits, no grid-wide barriers, no graphs.
#include <stdio.h>
#include <string.h>
#include <algorithm>

#include "plan_common.h"

#define TP_K 32                   // candidates per bot
#define TP_CHUNK 1024             // centroids per (bot, chunk) work item of the gather
#define TP_BOTS_PER_BLOCK 4       // one wave per bot, 4 waves per workgroup (they read the same centroid offsets)
#define TP_FB_BLOCK 256
#define TP_NOKEY 0xffffffffffffffffull
#define TP_NOCELL 0xffffffffu

static_assert(TP_K <= QS_WAVE, "one list entry per lane");

struct QsTbpState { int next_bot, m, stop, pad; };   // greedy pass: first bot not yet decided, targets so far, 1 = needs a full scan
// the workspace of one call, carved from ws (nullptr: only the bytes the block needs)
struct QsTbpLayout {
    QsTbpState *st;
    unsigned long long *count;            // [2] centroids, bots with a cell
    double2 *xy;                          // [n_cent + n_bots] centroids, then bots
    long long *cell;                      // [n_cent + n_bots] their cells (gy * size + gx), -1 = none
    unsigned int *coff;                   // [n_cent] offset of the centroid's cell in a field, TP_NOCELL = none
    long long *fcell;                     // [n_bots] the cells of the bots that have one, in bot order ...
    int *fbot;                            // [n_bots] ... and their bots
    unsigned long long *part;             // [n_bots][n_chunks][K] chunk lists
    unsigned long long *list;             // [n_bots][K] the top-K of a bot (by bot)
    int *list_len;                        // [n_bots]
    double2 *asg_xy; int *asg_idx;        // [n_bots] the targets so far: centroid position, index
    long long *tgt_idx;                   // [n_bots] per bot: the centroid or -1
    unsigned int *tgt_cost;               // [n_bots]
    int *tgt_status;                      // [n_bots]
    long long *pair;                      // [2 n_bots] start cells of the assigned bots (in assignment order), then their goals
    int *pair_bot;                        // [n_bots] the bot of each pair
    unsigned long long *fb_key;           // [n_fb] per-block minima of a fallback scan
    size_t bytes;
};

static inline size_t tp_chunks(size_t n_cent) { return (n_cent + TP_CHUNK - 1) / TP_CHUNK; }
static inline size_t tp_fb_blocks(size_t n_cent) { return (n_cent + TP_FB_BLOCK - 1) / TP_FB_BLOCK; }

static QsTbpLayout qs_tbp_layout(void *ws, size_t n_cent, size_t n_bots)
{
    QsTbpLayout L;
    Carve k(ws);
    L.st = k.take<QsTbpState>(1);
    L.count = k.take<unsigned long long>(2);
    L.xy = k.take<double2>(n_cent + n_bots);
    L.cell = k.take<long long>(n_cent + n_bots);
    L.coff = k.take<unsigned int>(n_cent);
    L.fcell = k.take<long long>(n_bots);
    L.fbot = k.take<int>(n_bots);
    L.part = k.take<unsigned long long>(n_bots * tp_chunks(n_cent) * TP_K);
    L.list = k.take<unsigned long long>(n_bots * TP_K);
    L.list_len = k.take<int>(n_bots);
    L.asg_xy = k.take<double2>(n_bots);
    L.asg_idx = k.take<int>(n_bots);
    L.tgt_idx = k.take<long long>(n_bots);
    L.tgt_cost = k.take<unsigned int>(n_bots);
    L.tgt_status = k.take<int>(n_bots);
    L.pair = k.take<long long>(2 * n_bots);
    L.pair_bot = k.take<int>(n_bots);
    L.fb_key = k.take<unsigned long long>(tp_fb_blocks(n_cent));
    L.bytes = k.bytes;
    return L;
}

// ---- cells -> field offsets ---------------------------------------------------------------------------------------------
// cell[0 .. n_cent): the centroids; cell[n_cent .. n_cent + n_bots): the bots.  A cell that exists is traversable, so it
// lies in the bounding box of the census.
__global__ void __launch_bounds__(256)
qs_tbp_offsets_kernel(const long long *__restrict__ cell, int n_cent, int n_bots, int size, PlBox B,
                      unsigned int *__restrict__ coff, unsigned long long *__restrict__ count)
{
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    long long c = -1;
    if (i < n_cent + n_bots) c = cell[i];
    if (i < n_cent) {
        unsigned int o = TP_NOCELL;
        if (c >= 0) {
            const int fx = (int)(c % size) - B.bx0 * PL_T, fy = (int)(c / size) - B.by0 * PL_T;
            if (fx >= 0 && fy >= 0 && fx < B.fw && fy < B.fh) o = (unsigned int)fy * (unsigned int)B.fw + (unsigned int)fx;
        }
        coff[i] = o;
    }
    const unsigned long long mc = __ballot(i < n_cent && c >= 0), mb = __ballot(i >= n_cent && c >= 0);
    if (lane == 0) {
        if (mc) atomicAdd(&count[0], (unsigned long long)__popcll(mc));
        if (mb) atomicAdd(&count[1], (unsigned long long)__popcll(mb));
    }
}

// ---- the wave-resident sorted list of 64-bit keys ---------------------------------------------------------------------
// Lanes 0..K-1 hold the list in ascending order; empty entries are TP_NOKEY and sort last.  Keys are distinct (the low
// word is the centroid).  Insert the wave-uniform candidate ck unless K entries already come before it.
__device__ inline void tp_insert(unsigned long long &lk, unsigned long long ck, int lane)
{
    const unsigned long long m = __ballot(lane < TP_K && lk < ck);
    const int p = __popcll(m);                          // entries before the candidate: lanes 0..p-1
    if (p >= TP_K) return;
    const unsigned long long uk = __shfl_up(lk, 1);
    if (lane > p && lane < TP_K) lk = uk;
    if (lane == p) lk = ck;
}

// candidates (one per lane, TP_NOKEY = none) into the list, in lane order
__device__ inline void tp_offer(unsigned long long &lk, unsigned long long key, int lane)
{
    const unsigned long long kth = __shfl(lk, TP_K - 1);
    unsigned long long m = __ballot(key < kth);         // false for TP_NOKEY
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        tp_insert(lk, __shfl(key, src), lane);
    }
}

// one wave per (field of the group, chunk of centroids): fields[f] is the field of bot fbot[g0 + f]
__global__ void __launch_bounds__(64 * TP_BOTS_PER_BLOCK)
qs_tbp_gather_kernel(const unsigned int *__restrict__ fields, size_t fcells, const unsigned int *__restrict__ coff, int n_cent,
                     const int *__restrict__ fbot, int g0, int gn, int n_chunks, unsigned long long *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.y * TP_BOTS_PER_BLOCK + (threadIdx.x >> 6), chunk = blockIdx.x;
    if (f >= gn) return;                                // whole waves; no workgroup barrier below
    const unsigned int *fld = fields + (size_t)f * fcells;
    unsigned long long lk = TP_NOKEY;
    const int lo = chunk * TP_CHUNK, hi = min(lo + TP_CHUNK, n_cent);
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        unsigned long long key = TP_NOKEY;
        if (j < hi) {
            const unsigned int o = coff[j];
            if (o != TP_NOCELL) {
                const unsigned int v = fld[o];
                if (v != PL_INF) key = ((unsigned long long)v << 32) | (unsigned int)j;
            }
        }
        tp_offer(lk, key, lane);
    }
    if (lane < TP_K) part[((size_t)fbot[g0 + f] * n_chunks + chunk) * TP_K + lane] = lk;
}

// one wave per bot with a cell: merge its chunk lists into the exact top-K (list, list_len = entries in it)
__global__ void __launch_bounds__(64 * TP_BOTS_PER_BLOCK)
qs_tbp_merge_kernel(const int *__restrict__ fbot, int n_live, int n_chunks, const unsigned long long *__restrict__ part,
                    unsigned long long *__restrict__ list, int *__restrict__ list_len)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * TP_BOTS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n_live) return;
    const int bot = fbot[i];
    unsigned long long lk = TP_NOKEY;
    const size_t n = (size_t)n_chunks * TP_K, base0 = (size_t)bot * n;
    for (size_t base = 0; base < n; base += 64) {
        const size_t e = base + lane;
        tp_offer(lk, e < n ? part[base0 + e] : TP_NOKEY, lane);
    }
    if (lane < TP_K) list[(size_t)bot * TP_K + lane] = lk;
    const int len = __popcll(__ballot(lane < TP_K && lk != TP_NOKEY));
    if (lane == 0) list_len[bot] = len;
}

// ---- the greedy pass: one wave, the bots in order -------------------------------------------------------------------
// Targets assigned so far live in LDS (and in asg_* / pair* for a resumed pass and for the waypoints).  fb_pending: the
// previous launch stopped at start_bot and a fallback scan has left its per-block minima in fb_key.
__global__ void __launch_bounds__(64)
qs_tbp_greedy_kernel(const double2 *__restrict__ cent, const long long *__restrict__ cent_cell,
                     const long long *__restrict__ bot_cell, int n_bots, double r2_sep,
                     const unsigned long long *__restrict__ list, const int *__restrict__ list_len, int start_bot, int start_m,
                     int fb_pending, const unsigned long long *__restrict__ fb_key, int n_fb, double2 *__restrict__ asg_xy,
                     int *__restrict__ asg_idx, long long *__restrict__ pair, int *__restrict__ pair_bot,
                     long long *__restrict__ tgt_idx, unsigned int *__restrict__ tgt_cost, int *__restrict__ tgt_status,
                     QsTbpState *__restrict__ st)
{
    __shared__ double2 s_xy[QS_FT_MAX_BOTS];
    __shared__ int s_idx[QS_FT_MAX_BOTS];
    const int lane = threadIdx.x;
    int m = start_m, b = start_bot;
    for (int j = lane; j < m; j += 64) { s_xy[j] = asg_xy[j]; s_idx[j] = asg_idx[j]; }
    __syncthreads();
    auto assign = [&](unsigned long long key) {
        const int k = (int)(key & 0xffffffffull);
        const double2 t = cent[k];
        if (lane == 0) {
            s_xy[m] = t; s_idx[m] = k; asg_xy[m] = t; asg_idx[m] = k;
            pair[m] = bot_cell[b]; pair[n_bots + m] = cent_cell[k]; pair_bot[m] = b;
            tgt_idx[b] = k; tgt_cost[b] = (unsigned int)(key >> 32); tgt_status[b] = QS_PLAN_OK;
        }
        m++;
        __syncthreads();
    };
    auto none = [&](int status) {
        if (lane == 0) { tgt_idx[b] = -1; tgt_cost[b] = PL_INF; tgt_status[b] = status; }
    };
    if (fb_pending) {
        unsigned long long k = TP_NOKEY;
        for (int q = lane; q < n_fb; q += 64) k = fb_key[q] < k ? fb_key[q] : k;
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(k, off);
            k = o < k ? o : k;
        }
        if (k != TP_NOKEY) assign(k);
        else none(QS_PLAN_UNREACHABLE);
        b++;
    }
    for (; b < n_bots; b++) {
        if (bot_cell[b] < 0) { none(QS_PLAN_NO_START); continue; }
        const int len = list_len[b];
        const unsigned long long *lst = list + (size_t)b * TP_K;
        unsigned long long pick = TP_NOKEY;
        for (int e = 0; e < len; e++) {
            const unsigned long long key = lst[e];
            const int k = (int)(key & 0xffffffffull);
            const double2 q = cent[k];
            bool blk = false;
            for (int j = lane; j < m; j += 64) {
                const double2 t = s_xy[j];
                const double dx = q.x - t.x, dy = q.y - t.y;
                blk |= s_idx[j] == k || dx * dx + dy * dy < r2_sep;      // taken / too close (qs_frontier_targets' test)
            }
            if (__ballot(blk) == 0) { pick = key; break; }
        }
        if (pick != TP_NOKEY) assign(pick);
        else if (len == TP_K) {                          // a full list, all of it ineligible: a whole-GPU scan decides
            if (lane == 0) { st->next_bot = b; st->m = m; st->stop = 1; }
            return;
        } else none(QS_PLAN_UNREACHABLE);                // the list holds every centroid with a finite cost
    }
    if (lane == 0) { st->next_bot = n_bots; st->m = m; st->stop = 0; }
}

// ---- the fallback: every centroid for one bot, whose field is fields[0] -----------------------------------------------
__global__ void __launch_bounds__(TP_FB_BLOCK)
qs_tbp_fallback_kernel(const unsigned int *__restrict__ fld, const unsigned int *__restrict__ coff,
                       const double2 *__restrict__ cent, int n_cent, int m, double r2_sep, const double2 *__restrict__ asg_xy,
                       const int *__restrict__ asg_idx, unsigned long long *__restrict__ fb_key)
{
    __shared__ double2 s_xy[TP_FB_BLOCK];
    __shared__ int s_idx[TP_FB_BLOCK];
    __shared__ unsigned long long s_k[TP_FB_BLOCK / QS_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x * TP_FB_BLOCK + tid;
    double2 q = make_double2(0.0, 0.0);
    unsigned long long k = TP_NOKEY;
    if (j < n_cent) {
        q = cent[j];
        const unsigned int o = coff[j];
        if (o != TP_NOCELL) {
            const unsigned int v = fld[o];
            if (v != PL_INF) k = ((unsigned long long)v << 32) | (unsigned int)j;
        }
    }
    for (int t0 = 0; t0 < m; t0 += TP_FB_BLOCK) {
        __syncthreads();
        if (t0 + tid < m) { s_xy[tid] = asg_xy[t0 + tid]; s_idx[tid] = asg_idx[t0 + tid]; }
        __syncthreads();
        const int tn = min(TP_FB_BLOCK, m - t0);
        for (int t = 0; t < tn && k != TP_NOKEY; t++) {
            const double dx = q.x - s_xy[t].x, dy = q.y - s_xy[t].y;
            if (s_idx[t] == j || dx * dx + dy * dy < r2_sep) k = TP_NOKEY;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = o < k ? o : k;
    }
    if (lane == 0) s_k[wave] = k;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TP_FB_BLOCK / QS_WAVE; w++) k = s_k[w] < k ? s_k[w] : k;
        fb_key[blockIdx.x] = k;
    }
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int qs_frontier_targets_by_path(qs_ctx *c, int32_t min_cluster, double separation, const qs_plan_params *params,
                                           const double *bot_xy, size_t n_bots, int64_t *target_idx, double *target_xy,
                                           uint32_t *cost, int32_t *status, int32_t *wp_cell_xy, double *wp_xy,
                                           double *centroids_xy, size_t cap, size_t *n_centroids, uint64_t stats[8])
{
    ARGCHK(c, c != nullptr);
    if (n_bots > QS_FT_MAX_BOTS) return qs_fail(c, QS_E_INVAL, "qs_frontier_targets_by_path: n_bots above QS_FT_MAX_BOTS");
    ARGCHK(c, n_bots == 0 || (bot_xy && target_idx && target_xy && cost && status));
    ARGCHK(c, (wp_cell_xy == nullptr) == (wp_xy == nullptr));
    ARGCHK(c, cap == 0 || centroids_xy);
    qs_plan_params p;
    int rc = plan_params(c, params, p);
    if (rc != QS_OK) return rc;
    // the centroids (frontier_targets.hip's), counted first
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, c->frontier_ws.reserve(qs_frontier_layout(c, nullptr).bytes, c->stream));
    void *fws = c->frontier_ws.p;
    HIPCHK(c, qs_launch_frontier_label(c, fws, true));
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 0, nullptr));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, qs_frontier_layout(c, fws).total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n_cent = (size_t)total, n_end = n_cent + n_bots;
    HIPCHK(c, c->tbp_ws.reserve(qs_tbp_layout(nullptr, n_cent, n_bots).bytes, c->stream));
    const QsTbpLayout T = qs_tbp_layout(c->tbp_ws.p, n_cent, n_bots);
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 1, T.xy));
    // the mask and the census; the cells of the centroids and the bots
    QsPlanLayout L;
    unsigned int bbox[4];
    rc = plan_begin(c, p.clearance, n_bots, 0, L, bbox);
    if (rc != QS_OK) return rc;
    const bool any_trav = bbox[0] <= bbox[2];
    uint64_t groups = 0, fallbacks = 0;
    unsigned long long count[2] = {0, 0}, st[4] = {0, 0, 0, 0};
    std::vector<long long> tidx(n_bots, -1), bcell(n_bots, -1);
    std::vector<unsigned int> tcost(n_bots, PL_INF);
    std::vector<int> tstat(n_bots, QS_PLAN_NO_START);
    std::vector<int4> out(n_bots, make_int4(0, -1, -1, -1));
    int m = 0;
    if (n_bots && any_trav) {
        const PlBox B = pl_box(bbox);
        const size_t fcells = (size_t)B.fw * B.fh;
        HIPCHK(c, hipMemcpyAsync(T.xy + n_cent, bot_xy, n_bots * sizeof(double2), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(T.count, 0, 2 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipMemsetAsync(T.list_len, 0, n_bots * sizeof(int), c->stream));
        HIPCHK(c, qs_launch_plan_snap(c, L, T.xy, T.cell, n_end, p.snap_radius, L.stats + 3));
        hipLaunchKernelGGL(qs_tbp_offsets_kernel, dim3((unsigned int)((n_end + 255) / 256)), dim3(256), 0, c->stream, T.cell,
                           (int)n_cent, (int)n_bots, c->cfg.size, B, T.coff, T.count);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(bcell.data(), T.cell + n_cent, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(count, T.count, sizeof count, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // one field per bot with a cell, in groups; each group's costs gathered into chunk lists while it is resident
        std::vector<long long> fcell;
        std::vector<int> fbot;
        for (size_t b = 0; b < n_bots; b++)
            if (bcell[b] >= 0) { fcell.push_back(bcell[b]); fbot.push_back((int)b); }
        const size_t n_live = fcell.size();
        const int nch = (int)tp_chunks(n_cent);
        if (n_live && n_cent) {
            HIPCHK(c, hipMemcpyAsync(T.fcell, fcell.data(), n_live * sizeof(long long), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(T.fbot, fbot.data(), n_live * sizeof(int), hipMemcpyHostToDevice, c->stream));
            const size_t g = qs_plan_group(L, bbox, n_live);
            if (g == 0) return qs_fail(c, QS_E_STATE, "qs_frontier_targets_by_path: workspace holds no field");
            for (size_t g0 = 0; g0 < n_live; g0 += g, groups++) {
                const size_t gn = std::min(g, n_live - g0);
                rc = plan_fields(c, L, bbox, T.fcell, T.fcell, g0, gn);
                if (rc != QS_OK) return rc;
                const unsigned int gy = (unsigned int)((gn + TP_BOTS_PER_BLOCK - 1) / TP_BOTS_PER_BLOCK);
                hipLaunchKernelGGL(qs_tbp_gather_kernel, dim3((unsigned int)nch, gy), dim3(64 * TP_BOTS_PER_BLOCK), 0, c->stream,
                                   L.fields, fcells, T.coff, (int)n_cent, T.fbot, (int)g0, (int)gn, nch, T.part);
                HIPCHK(c, hipGetLastError());
            }
            hipLaunchKernelGGL(qs_tbp_merge_kernel, dim3((unsigned int)((n_live + TP_BOTS_PER_BLOCK - 1) / TP_BOTS_PER_BLOCK)),
                               dim3(64 * TP_BOTS_PER_BLOCK), 0, c->stream, T.fbot, (int)n_live, nch, T.part, T.list, T.list_len);
            HIPCHK(c, hipGetLastError());
        }
        // the greedy pass; a bot whose full list is ineligible gets its field again and a scan of every centroid
        const double r2_sep = r2_threshold_for(separation);        // s < r2_sep <=> sqrt(s) < separation
        int start = 0, pending = 0;
        for (;;) {
            hipLaunchKernelGGL(qs_tbp_greedy_kernel, dim3(1), dim3(64), 0, c->stream, T.xy, T.cell, T.cell + n_cent, (int)n_bots,
                               r2_sep, T.list, T.list_len, start, m, pending, T.fb_key, (int)tp_fb_blocks(n_cent), T.asg_xy,
                               T.asg_idx, T.pair, T.pair_bot, T.tgt_idx, T.tgt_cost, T.tgt_status, T.st);
            HIPCHK(c, hipGetLastError());
            QsTbpState gs;
            HIPCHK(c, hipMemcpyAsync(&gs, T.st, sizeof gs, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            m = gs.m;
            if (!gs.stop) break;
            if (gs.next_bot < start || gs.next_bot >= (int)n_bots || (pending && gs.next_bot == start))
                return qs_fail(c, QS_E_HIP, "qs_frontier_targets_by_path: greedy pass made no progress");
            fallbacks++;
            groups++;
            start = gs.next_bot; pending = 1;
            rc = plan_fields(c, L, bbox, T.cell + n_cent, T.cell + n_cent, (size_t)start, 1);
            if (rc != QS_OK) return rc;
            hipLaunchKernelGGL(qs_tbp_fallback_kernel, dim3((unsigned int)tp_fb_blocks(n_cent)), dim3(TP_FB_BLOCK), 0, c->stream,
                               L.fields, T.coff, T.xy, (int)n_cent, m, r2_sep, T.asg_xy, T.asg_idx, T.fb_key);
            HIPCHK(c, hipGetLastError());
        }
        // waypoints: qs_plan_paths' fields and walks for the m assigned pairs (starts pair[0..m), goals pair[n_bots ..))
        if (wp_xy && m) {
            const size_t g = qs_plan_group(L, bbox, (size_t)m);
            for (size_t g0 = 0; g0 < (size_t)m; g0 += g, groups++) {
                const size_t gn = std::min(g, (size_t)m - g0);
                rc = plan_fields(c, L, bbox, T.pair, T.pair + n_bots, g0, gn);
                if (rc != QS_OK) return rc;
                HIPCHK(c, qs_launch_plan_walk(c, L, bbox, T.pair, T.pair + n_bots, g0, gn, p.lookahead, 0));
            }
            HIPCHK(c, hipMemcpyAsync(out.data(), L.out4, (size_t)m * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(tidx.data(), T.tgt_idx, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(tcost.data(), T.tgt_cost, n_bots * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(tstat.data(), T.tgt_status, n_bots * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st, L.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    } else if (any_trav && n_cent) {                     // no bots: the centroids' cells are still counted
        HIPCHK(c, hipMemsetAsync(T.count, 0, 2 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, qs_launch_plan_snap(c, L, T.xy, T.cell, n_cent, p.snap_radius, L.stats + 3));
        hipLaunchKernelGGL(qs_tbp_offsets_kernel, dim3((unsigned int)((n_cent + 255) / 256)), dim3(256), 0, c->stream, T.cell,
                           (int)n_cent, 0, c->cfg.size, pl_box(bbox), T.coff, T.count);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(count, T.count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    }   // (no traversable cell: nothing snaps, every bot is QS_PLAN_NO_START, what the snap kernel would say)
    const size_t nc = n_cent < cap ? n_cent : cap;
    if (nc) HIPCHK(c, hipMemcpyAsync(centroids_xy, T.xy, nc * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    std::vector<double2> axy((size_t)m);
    if (m) HIPCHK(c, hipMemcpyAsync(axy.data(), T.asg_xy, (size_t)m * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    std::vector<int> abot((size_t)m);
    if (m) HIPCHK(c, hipMemcpyAsync(abot.data(), T.pair_bot, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t b = 0; b < n_bots; b++) {
        target_idx[b] = tidx[b];
        target_xy[2 * b] = target_xy[2 * b + 1] = NAN;
        cost[b] = tcost[b];
        status[b] = tstat[b];
        if (wp_xy) {
            wp_cell_xy[2 * b] = wp_cell_xy[2 * b + 1] = -1;
            wp_xy[2 * b] = wp_xy[2 * b + 1] = NAN;
        }
    }
    for (int i = 0; i < m; i++) {
        const int b = abot[i];
        if (b < 0 || b >= (int)n_bots || tidx[b] < 0) return qs_fail(c, QS_E_STATE, "qs_frontier_targets_by_path: assignment list is inconsistent");
        target_xy[2 * b] = axy[i].x; target_xy[2 * b + 1] = axy[i].y;
        if (!wp_xy) continue;
        const int4 o = out[i];
        // both ends have cells and the cost is finite: the walk cannot fail, and its cost is the bot field's (symmetric moves)
        if (o.x != QS_PLAN_OK || (unsigned int)o.w != tcost[b]) {
            char msg[160];
            snprintf(msg, sizeof msg, "qs_frontier_targets_by_path: bot %d: the waypoint's path (status %d, cost %u) disagrees "
                     "with the assignment's cost %u", b, o.x, (unsigned int)o.w, tcost[b]);
            return qs_fail(c, QS_E_STATE, msg);
        }
        wp_cell_xy[2 * b] = o.y; wp_cell_xy[2 * b + 1] = o.z;
        wp_xy[2 * b] = c->cfg.ox + (o.y + 0.5) * c->cfg.res;        // grid_to_world :127-131
        wp_xy[2 * b + 1] = c->cfg.oy + (o.z + 0.5) * c->cfg.res;
    }
    if (n_centroids) *n_centroids = n_cent;
    if (stats) {
        stats[0] = n_cent; stats[1] = count[0]; stats[2] = count[1]; stats[3] = groups;
        stats[4] = st[0]; stats[5] = st[1]; stats[6] = fallbacks; stats[7] = 0;
    }
    return QS_OK;
}
