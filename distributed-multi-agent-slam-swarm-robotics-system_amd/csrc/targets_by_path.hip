// targets_by_path.hip -- frontier targets ranked by path cost over the mapped free space.
// The rules are this build's own (include/quasar_slam.h, "frontier targets by path cost"), all integer once the centroids
// exist.  The centroids are frontier_targets.hip's; the mask, the census, the snap, the fields and the walk are plan.hip's
// (plan_common.h).  New here is the stage between them:
//
//   cells    : the centroids and the bots snap in ONE launch of the planner's snap kernel; a second kernel turns the
//              centroids' cells into offsets into a field (the bounding box of the census) and counts who has a cell;
//   fields   : one field per bot with a cell, seeded at the bot (the moves are symmetric: the field of a bot's cell holds
//              the cost to every cell), in groups that fit QS_PLAN_WS_CAP, relaxed by the planner's host-driven rounds;
//   gather   : while a group's fields are resident, one wave per (bot, chunk of AS_CHUNK centroids): lanes read the
//              centroids' offsets coalesced, gather field[offset], and the wave keeps the AS_K smallest 64-bit keys
//              (cost << 32) | k in a sorted list across lanes 0..AS_K-1 (ballot insertion, one shfl_up).  Infinite costs
//              never enter a list.  One wave per bot then merges its chunk lists into the exact top-K;
//   greedy   : ONE wave walks the bots in order; a bot takes the first entry of its list that is neither taken nor within
//              `separation` of a target assigned so far (frontier_targets.hip's fp64 test).  The list is the true top-K by
//              the key the rule orders by, so its first eligible entry is the minimum over every eligible centroid.  When a
//              full list is entirely ineligible the pass stops: the host recomputes that bot's field, a whole-GPU scan over
//              all centroids finds its pick, and the pass resumes (counted in stats);
//   waypoints: plan.hip's waypoint stage for the assigned pairs: fields seeded at the assigned centroids' cells, the walk.
// No device-side waits, no grid-wide barriers, no graphs.
// The sorted list, the blocked test, the greedy walk and the host's stop / resume loop are assign_common.h's, shared with
// frontier_targets.hip; here are the entry they order by, the gather that produces the chunk lists and the fallback's key.
// The stages are written over that entry, so qs_frontier_targets_by_gain (§4.17) is the same call with another order: its
// entry carries (cost + bias, gain, centroid), and the gains come from gain.hip before the mask is built.
// The argument check and the per-bot epilogue ahead of the call also serve qs_frontier_targets_by_territory (§4.16).
#include <stdio.h>
#include <string.h>
#include <algorithm>

#include "assign_common.h"
#include "plan_common.h"

#define TP_NOKEY 0xffffffffffffffffull

// the workspace of one call, carved from ws (nullptr: only the bytes the block needs)
template <typename E>
struct QsTbpLayout {
    QsAssignState *st;
    QsTgtLayout tg;                       // what territory.hip's workspace holds too (plan_common.h)
    long long *fcell;                     // [n_bots] the cells of the bots that have one, in bot order ...
    int *fbot;                            // [n_bots] ... and their bots
    typename E::Item *part;               // [n_bots][n_chunks][K] chunk lists
    typename E::Item *list;               // [n_bots][K] the top-K of a bot (by bot)
    int *list_len;                        // [n_bots]
    double2 *asg_xy; int *asg_idx;        // [n_bots] the targets so far: centroid position, index
    typename E::Item *fb_key;             // [n_fb] per-block minima of a fallback scan
    size_t bytes;
};

template <typename E>
static QsTbpLayout<E> qs_tbp_layout(void *ws, size_t n_cent, size_t n_bots)
{
    QsTbpLayout<E> L;
    Carve k(ws);
    L.st = k.take<QsAssignState>(1);
    L.tg = qs_tgt_layout(k, n_cent, n_bots);
    L.fcell = k.take<long long>(n_bots);
    L.fbot = k.take<int>(n_bots);
    L.part = k.take<typename E::Item>(n_bots * as_chunks(n_cent) * AS_K);
    L.list = k.take<typename E::Item>(n_bots * AS_K);
    L.list_len = k.take<int>(n_bots);
    L.asg_xy = k.take<double2>(n_bots);
    L.asg_idx = k.take<int>(n_bots);
    L.fb_key = k.take<typename E::Item>(as_fb_blocks(n_cent));
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

hipError_t qs_launch_tbp_offsets(qs_ctx *c, const long long *cell, size_t n_cent, size_t n_bots, const unsigned int bbox[4],
                                 unsigned int *coff, unsigned long long *count)
{
    const size_t n_end = n_cent + n_bots;
    if (!n_end) return hipSuccess;
    hipLaunchKernelGGL(qs_tbp_offsets_kernel, dim3((unsigned int)((n_end + 255) / 256)), dim3(256), 0, c->stream, cell,
                       (int)n_cent, (int)n_bots, c->cfg.size, pl_box(bbox), coff, count);
    return hipGetLastError();
}

// ---- the entries of the lists -------------------------------------------------------------------------------------------
// The stages below are written once over the entry E a rule orders by; beyond assign_common.h's interface an entry has
//   typedef Aux                          what the rule needs beside a field, passed by value to the kernels
//   static E make(cost, j, Aux)          the entry of centroid j at a finite cost
//   static unsigned int cost(Item, Aux)  the cost an item of a list stands for
// and its Part is a plain array of Items.
//
// §4.12: the 64-bit key (cost << 32) | centroid.  Keys are distinct (the low word is the centroid); TP_NOKEY is the empty entry.
struct TpNoAux {};
struct TpEntry {
    unsigned long long key;
    typedef unsigned long long *Part;
    typedef const unsigned long long *CPart;
    typedef unsigned long long Item;
    typedef TpNoAux Aux;
    __device__ static TpEntry none() { return {TP_NOKEY}; }
    __device__ bool valid() const { return key != TP_NOKEY; }
    __device__ bool before(TpEntry o) const { return key < o.key; }
    template <typename F> __device__ TpEntry map(F f) const { return {f(key)}; }
    __device__ static TpEntry load(const CPart p, size_t o) { return {p[o]}; }
    __device__ void store(const Part p, size_t o) const { p[o] = key; }
    __device__ Item item() const { return key; }
    __device__ static int centroid(Item it) { return (int)(it & 0xffffffffull); }
    __device__ static TpEntry make(unsigned int cost, int j, Aux) { return {((unsigned long long)cost << 32) | (unsigned int)j}; }
    __device__ static unsigned int cost(Item it, Aux) { return (unsigned int)(it >> 32); }
};

// §4.17 (G6): (cost + bias, gain, centroid); a comes before b when (cost_a + bias) * gain_b < (cost_b + bias) * gain_a, ties
// to the smaller cost, then the lower centroid: a strict total order.  cost + bias < 2^33 and gain < 2^15 (the cells of a
// disc of QS_GAIN_MAX_RANGE), so the products are exact in 64 bits.  The empty entry has gain 0 and so comes after every
// entry with a gain: 0 < cb * gain on one side, cb * gain < 0 never on the other.  Written without short-circuits, as ft_before.
struct GnItem { unsigned long long cb; unsigned int gain; int k; };
struct GnAux { const int *gain; unsigned int bias; };
struct GnEntry {
    unsigned long long cb; unsigned int gain; int k;
    typedef GnItem *Part;
    typedef const GnItem *CPart;
    typedef GnItem Item;
    typedef GnAux Aux;
    __device__ static GnEntry none() { return {1ull << 40, 0u, 0x7fffffff}; }
    __device__ bool valid() const { return gain != 0; }
    __device__ bool before(GnEntry o) const
    {
        const unsigned long long l = cb * o.gain, r = o.cb * gain;
        return (l < r) | ((l == r) & ((cb < o.cb) | ((cb == o.cb) & (k < o.k))));
    }
    template <typename F> __device__ GnEntry map(F f) const { return {f(cb), f(gain), f(k)}; }
    __device__ static GnEntry load(const CPart p, size_t o) { const GnItem i = p[o]; return {i.cb, i.gain, i.k}; }
    __device__ void store(const Part p, size_t o) const { p[o] = item(); }
    __device__ Item item() const { return {cb, gain, k}; }
    __device__ static int centroid(Item it) { return it.k; }
    __device__ static GnEntry make(unsigned int cost, int j, Aux a) { return {(unsigned long long)cost + a.bias, (unsigned int)a.gain[j], j}; }
    __device__ static unsigned int cost(Item it, Aux a) { return (unsigned int)(it.cb - a.bias); }
};

// the entry of centroid j in the field fld: made of its cost there, or none
template <typename E>
__device__ inline E tp_key(const unsigned int *__restrict__ fld, const unsigned int *__restrict__ coff, int j, typename E::Aux aux)
{
    const unsigned int o = coff[j];
    if (o != TP_NOCELL) {
        const unsigned int v = fld[o];
        if (v != PL_INF) return E::make(v, j, aux);
    }
    return E::none();
}

// one wave per (field of the group, chunk of centroids): fields[f] is the field of bot fbot[g0 + f]
template <typename E>
__global__ void __launch_bounds__(64 * AS_BOTS_PER_BLOCK)
qs_tbp_gather_kernel(const unsigned int *__restrict__ fields, size_t fcells, const unsigned int *__restrict__ coff, int n_cent,
                     const int *__restrict__ fbot, int g0, int gn, int n_chunks, typename E::Aux aux,
                     typename E::Item *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.y * AS_BOTS_PER_BLOCK + (threadIdx.x >> 6), chunk = blockIdx.x;
    if (f >= gn) return;                                // whole waves; no workgroup barrier below
    const unsigned int *fld = fields + (size_t)f * fcells;
    E l = E::none();
    const int lo = chunk * AS_CHUNK, hi = min(lo + AS_CHUNK, n_cent);
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        as_offer(l, j < hi ? tp_key<E>(fld, coff, j, aux) : E::none(), lane);
    }
    if (lane < AS_K) l.store(part, ((size_t)fbot[g0 + f] * n_chunks + chunk) * AS_K + lane);
}

// one wave per bot with a cell: merge its chunk lists into the exact top-K (list, list_len = entries in it)
template <typename E>
__global__ void __launch_bounds__(64 * AS_BOTS_PER_BLOCK)
qs_tbp_merge_kernel(const int *__restrict__ fbot, int n_live, int n_chunks, const typename E::Item *__restrict__ part,
                    typename E::Item *__restrict__ list, int *__restrict__ list_len)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * AS_BOTS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n_live) return;
    const int bot = fbot[i];
    const size_t n = (size_t)n_chunks * AS_K;
    int len;
    const E l = as_merge_lists<E>(part, (size_t)bot * n, n, lane, len);
    if (lane < AS_K) list[(size_t)bot * AS_K + lane] = l.item();
    if (lane == 0) list_len[bot] = len;
}

// ---- the greedy pass (assign_common.h): a decision leaves the centroid, the cost, a status and, for the waypoints, the
// (start, goal) cells of the assigned bots in assignment order.  A bot without a cell has no list to look at.
template <typename E>
struct TpPolicy {
    const long long *cent_cell, *bot_cell;
    int n_bots;
    typename E::Aux aux;
    long long *pair; int *pair_bot;
    long long *tgt_idx; unsigned int *tgt_cost; int *tgt_status;
    __device__ void assigned(int b, int m, typename E::Item it, double2) const
    {
        const int k = E::centroid(it);
        pair[m] = bot_cell[b]; pair[n_bots + m] = cent_cell[k]; pair_bot[m] = b;
        tgt_idx[b] = k; tgt_cost[b] = E::cost(it, aux); tgt_status[b] = QS_PLAN_OK;
    }
    __device__ void none(int b, int status) const { tgt_idx[b] = -1; tgt_cost[b] = PL_INF; tgt_status[b] = status; }
    __device__ void unassigned(int b) const { none(b, QS_PLAN_UNREACHABLE); }
    __device__ bool skip(int b, int lane) const
    {
        if (bot_cell[b] >= 0) return false;
        if (lane == 0) none(b, QS_PLAN_NO_START);
        return true;
    }
};

template <typename E>
__global__ void __launch_bounds__(64)
qs_tbp_greedy_kernel(const double2 *__restrict__ cent, const long long *__restrict__ cent_cell,
                     const long long *__restrict__ bot_cell, int n_bots, double r2_sep, typename E::Aux aux,
                     const typename E::Item *__restrict__ list, const int *__restrict__ list_len, int start_bot, int start_m,
                     int fb_pending, const typename E::Item *__restrict__ fb_key, int n_fb, double2 *__restrict__ asg_xy,
                     int *__restrict__ asg_idx, long long *__restrict__ pair, int *__restrict__ pair_bot,
                     long long *__restrict__ tgt_idx, unsigned int *__restrict__ tgt_cost, int *__restrict__ tgt_status,
                     QsAssignState *__restrict__ st)
{
    as_greedy_walk<E>(TpPolicy<E>{cent_cell, bot_cell, n_bots, aux, pair, pair_bot, tgt_idx, tgt_cost, tgt_status}, cent, n_bots,
                      r2_sep, list, list_len, start_bot, start_m, fb_pending, fb_key, n_fb, asg_xy, asg_idx, st);
}

// ---- the fallback: every centroid for one bot, whose field is fields[0] -----------------------------------------------
template <typename E>
__global__ void __launch_bounds__(AS_FB_BLOCK)
qs_tbp_fallback_kernel(const unsigned int *__restrict__ fld, const unsigned int *__restrict__ coff,
                       const double2 *__restrict__ cent, int n_cent, int m, double r2_sep, const double2 *__restrict__ asg_xy,
                       const int *__restrict__ asg_idx, typename E::Aux aux, typename E::Item *__restrict__ fb_key)
{
    const int j = blockIdx.x * AS_FB_BLOCK + threadIdx.x;
    double2 q = make_double2(0.0, 0.0);
    E e = E::none();
    if (j < n_cent) { q = cent[j]; e = tp_key<E>(fld, coff, j, aux); }
    as_fallback_block<E>(e.valid(), j, q, m, r2_sep, asg_xy, asg_idx, fb_key, [&] { return e; });
}

// ---- what the three path-cost entry points share (plan_common.h) ----------------------------------------------------------
int tbp_check_args(qs_ctx *c, const char *who, size_t n_bots, const double *bot_xy, const QsTargetsOut &o,
                   const double *centroids_xy, size_t cap, const qs_plan_params *params, qs_plan_params &p)
{
    const auto [target_idx, target_xy, cost, status, wp_cell_xy, wp_xy] = o;
    ARGCHK(c, c != nullptr);
    if (n_bots > QS_FT_MAX_BOTS) return qs_fail(c, QS_E_INVAL, (std::string(who) + ": n_bots above QS_FT_MAX_BOTS").c_str());
    ARGCHK(c, n_bots == 0 || (bot_xy && target_idx && target_xy && cost && status));
    ARGCHK(c, (wp_cell_xy == nullptr) == (wp_xy == nullptr));
    ARGCHK(c, cap == 0 || centroids_xy);
    return plan_params(c, params, p);
}

int tbp_finish(qs_ctx *c, const char *who, const char *whose, const QsTargetsHost &H, size_t m, const QsTargetsOut &o)
{
    const size_t n_bots = H.idx.size();
    for (size_t b = 0; b < n_bots; b++) {
        o.target_idx[b] = H.idx[b];
        o.target_xy[2 * b] = H.xy[b].x; o.target_xy[2 * b + 1] = H.xy[b].y;
        o.cost[b] = H.cost[b];
        o.status[b] = H.status[b];
        if (o.wp_xy) {
            o.wp_cell_xy[2 * b] = o.wp_cell_xy[2 * b + 1] = -1;
            o.wp_xy[2 * b] = o.wp_xy[2 * b + 1] = NAN;
        }
    }
    for (size_t i = 0; i < m; i++) {
        const int b = H.pair_bot[i];
        if (b < 0 || b >= (int)n_bots || H.idx[b] < 0)
            return qs_fail(c, QS_E_STATE, (std::string(who) + ": assignment list is inconsistent").c_str());
        if (!o.wp_xy) continue;
        const int4 w = H.out4[i];
        // both ends have cells and the cost is finite: the walk cannot fail, and its cost is the bot's (symmetric moves)
        if (w.x != QS_PLAN_OK || (unsigned int)w.w != H.cost[b]) {
            char msg[192];
            snprintf(msg, sizeof msg, "%s: bot %d: the waypoint's path (status %d, cost %u) disagrees with the %s cost %u", who, b,
                     w.x, (unsigned int)w.w, whose, H.cost[b]);
            return qs_fail(c, QS_E_STATE, msg);
        }
        o.wp_cell_xy[2 * b] = w.y; o.wp_cell_xy[2 * b + 1] = w.z;
        o.wp_xy[2 * b] = c->cfg.ox + (w.y + 0.5) * c->cfg.res;        // grid_to_world :127-131
        o.wp_xy[2 * b + 1] = c->cfg.oy + (w.z + 0.5) * c->cfg.res;
    }
    return QS_OK;
}

// ---- the call, over the entry E its rule orders by ----------------------------------------------------------------------
// rank(fws, n_cent, aux), called once the frontier workspace is labelled and the n_cent centroids are counted, enqueues what
// the rule needs beside the fields and fills aux (QS_OK or the call's failure).  stats[7] is left 0 for the caller.
template <typename E, typename Rank>
static int tbp_run(qs_ctx *c, const char *who, int32_t min_cluster, double separation, const qs_plan_params *params, Rank rank,
                   const double *bot_xy, size_t n_bots, const QsTargetsOut &o, double *centroids_xy, size_t cap,
                   size_t *n_centroids, uint64_t stats[8])
{
    qs_plan_params p;
    int rc = tbp_check_args(c, who, n_bots, bot_xy, o, centroids_xy, cap, params, p);
    if (rc != QS_OK) return rc;
    // the centroids (frontier_targets.hip's), counted first
    void *fws;
    size_t n_cent;
    rc = qs_count_centroids(c, min_cluster, fws, n_cent);
    if (rc != QS_OK) return rc;
    const size_t n_end = n_cent + n_bots;
    HIPCHK(c, c->tbp_ws.reserve(qs_tbp_layout<E>(nullptr, n_cent, n_bots).bytes, c->stream));
    const QsTbpLayout<E> T = qs_tbp_layout<E>(c->tbp_ws.p, n_cent, n_bots);
    const QsTgtLayout &S = T.tg;
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 1, S.xy));
    typename E::Aux aux{};
    rc = rank(fws, n_cent, aux);
    if (rc != QS_OK) return rc;
    // the mask and the census; the cells of the centroids and the bots
    QsPlanLayout L;
    unsigned int bbox[4];
    rc = plan_begin(c, p.clearance, n_bots, 0, L, bbox);
    if (rc != QS_OK) return rc;
    const bool any_trav = bbox[0] <= bbox[2];
    const std::string name(who);
    uint64_t groups = 0, fallbacks = 0;
    unsigned long long count[2] = {0, 0}, st[4] = {0, 0, 0, 0};
    std::vector<long long> bcell(n_bots, -1);
    QsTargetsHost H(n_bots);
    int m = 0;
    if (n_bots && any_trav) {
        const PlBox B = pl_box(bbox);
        const size_t fcells = (size_t)B.fw * B.fh;
        HIPCHK(c, hipMemcpyAsync(S.xy + n_cent, bot_xy, n_bots * sizeof(double2), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(S.count, 0, 2 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipMemsetAsync(T.list_len, 0, n_bots * sizeof(int), c->stream));
        HIPCHK(c, qs_launch_plan_snap(c, L, S.xy, S.cell, n_end, p.snap_radius, L.stats + 3));
        HIPCHK(c, qs_launch_tbp_offsets(c, S.cell, n_cent, n_bots, bbox, S.coff, S.count));
        HIPCHK(c, hipMemcpyAsync(bcell.data(), S.cell + n_cent, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(count, S.count, sizeof count, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // one field per bot with a cell, in groups; each group's costs gathered into chunk lists while it is resident
        std::vector<long long> fcell;
        std::vector<int> fbot;
        for (size_t b = 0; b < n_bots; b++)
            if (bcell[b] >= 0) { fcell.push_back(bcell[b]); fbot.push_back((int)b); }
        const size_t n_live = fcell.size();
        const int nch = (int)as_chunks(n_cent);
        if (n_live && n_cent) {
            HIPCHK(c, hipMemcpyAsync(T.fcell, fcell.data(), n_live * sizeof(long long), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(T.fbot, fbot.data(), n_live * sizeof(int), hipMemcpyHostToDevice, c->stream));
            const size_t g = qs_plan_group(L, bbox, n_live);
            if (g == 0) return qs_fail(c, QS_E_STATE, (name + ": workspace holds no field").c_str());
            for (size_t g0 = 0; g0 < n_live; g0 += g, groups++) {
                const size_t gn = std::min(g, n_live - g0);
                rc = plan_fields(c, L, bbox, T.fcell, T.fcell, g0, gn);
                if (rc != QS_OK) return rc;
                const unsigned int gy = (unsigned int)((gn + AS_BOTS_PER_BLOCK - 1) / AS_BOTS_PER_BLOCK);
                hipLaunchKernelGGL(qs_tbp_gather_kernel<E>, dim3((unsigned int)nch, gy), dim3(64 * AS_BOTS_PER_BLOCK), 0, c->stream,
                                   L.fields, fcells, S.coff, (int)n_cent, T.fbot, (int)g0, (int)gn, nch, aux, T.part);
                HIPCHK(c, hipGetLastError());
            }
            hipLaunchKernelGGL(qs_tbp_merge_kernel<E>, dim3((unsigned int)((n_live + AS_BOTS_PER_BLOCK - 1) / AS_BOTS_PER_BLOCK)),
                               dim3(64 * AS_BOTS_PER_BLOCK), 0, c->stream, T.fbot, (int)n_live, nch, T.part, T.list, T.list_len);
            HIPCHK(c, hipGetLastError());
        }
        // the greedy pass; a bot whose full list is ineligible gets its field again and a scan of every centroid
        const double r2_sep = r2_threshold_for(separation);        // s < r2_sep <=> sqrt(s) < separation
        const int nfb = (int)as_fb_blocks(n_cent);
        rc = as_run_greedy(c, (name + ": greedy pass made no progress").c_str(), T.st, n_bots,
            [&](int start, int m, int pending) {
                hipLaunchKernelGGL(qs_tbp_greedy_kernel<E>, dim3(1), dim3(64), 0, c->stream, S.xy, S.cell, S.cell + n_cent, (int)n_bots,
                                   r2_sep, aux, T.list, T.list_len, start, m, pending, T.fb_key, nfb, T.asg_xy, T.asg_idx, S.pair,
                                   S.pair_bot, S.tgt_idx, S.tgt_cost, S.tgt_status, T.st);
                return hipGetLastError();
            },
            [&](int bot, int m) {                                   // the bot's field again, then every centroid for it
                groups++;
                const int rcf = plan_fields(c, L, bbox, S.cell + n_cent, S.cell + n_cent, (size_t)bot, 1);
                if (rcf != QS_OK) return rcf;
                hipLaunchKernelGGL(qs_tbp_fallback_kernel<E>, dim3((unsigned int)nfb), dim3(AS_FB_BLOCK), 0, c->stream, L.fields, S.coff,
                                   S.xy, (int)n_cent, m, r2_sep, T.asg_xy, T.asg_idx, aux, T.fb_key);
                HIPCHK(c, hipGetLastError());
                return (int)QS_OK;
            }, m, fallbacks);
        if (rc != QS_OK) return rc;
        // waypoints for the m assigned pairs (starts pair[0..m), goals pair[n_bots ..))
        if (o.wp_xy && m) {
            rc = plan_waypoints(c, who, L, bbox, S.pair, S.pair + n_bots, (size_t)m, p.lookahead, 0, groups, H.out4.data());
            if (rc != QS_OK) return rc;
        }
        HIPCHK(c, hipMemcpyAsync(H.idx.data(), S.tgt_idx, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(H.cost.data(), S.tgt_cost, n_bots * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(H.status.data(), S.tgt_status, n_bots * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st, L.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    } else if (any_trav && n_cent) {                     // no bots: the centroids' cells are still counted
        HIPCHK(c, hipMemsetAsync(S.count, 0, 2 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, qs_launch_plan_snap(c, L, S.xy, S.cell, n_cent, p.snap_radius, L.stats + 3));
        HIPCHK(c, qs_launch_tbp_offsets(c, S.cell, n_cent, 0, bbox, S.coff, S.count));
        HIPCHK(c, hipMemcpyAsync(count, S.count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    }   // (no traversable cell: nothing snaps, every bot is QS_PLAN_NO_START, what the snap kernel would say)
    const size_t nc = n_cent < cap ? n_cent : cap;
    if (nc) HIPCHK(c, hipMemcpyAsync(centroids_xy, S.xy, nc * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    std::vector<double2> axy((size_t)m);
    if (m) HIPCHK(c, hipMemcpyAsync(axy.data(), T.asg_xy, (size_t)m * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    if (m) HIPCHK(c, hipMemcpyAsync(H.pair_bot.data(), S.pair_bot, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; i++)                          // the targets' positions into bot order (tbp_finish refuses a bot out of range)
        if (H.pair_bot[i] >= 0 && H.pair_bot[i] < (int)n_bots) H.xy[H.pair_bot[i]] = axy[i];
    rc = tbp_finish(c, who, "assignment's", H, (size_t)m, o);
    if (rc != QS_OK) return rc;
    if (n_centroids) *n_centroids = n_cent;
    if (stats) {
        stats[0] = n_cent; stats[1] = count[0]; stats[2] = count[1]; stats[3] = groups;
        stats[4] = st[0]; stats[5] = st[1]; stats[6] = fallbacks; stats[7] = 0;
    }
    return QS_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int qs_frontier_targets_by_path(qs_ctx *c, int32_t min_cluster, double separation, const qs_plan_params *params,
                                           const double *bot_xy, size_t n_bots, int64_t *target_idx, double *target_xy,
                                           uint32_t *cost, int32_t *status, int32_t *wp_cell_xy, double *wp_xy,
                                           double *centroids_xy, size_t cap, size_t *n_centroids, uint64_t stats[8])
{
    return tbp_run<TpEntry>(c, "qs_frontier_targets_by_path", min_cluster, separation, params,
                            [](void *, size_t, TpNoAux &) { return (int)QS_OK; }, bot_xy, n_bots,
                            {target_idx, target_xy, cost, status, wp_cell_xy, wp_xy}, centroids_xy, cap, n_centroids, stats);
}

// §4.17: the same stages ordered by G6; the gains (gain.hip) are computed while the frontier workspace is still labelled
extern "C" int qs_frontier_targets_by_gain(qs_ctx *c, int32_t min_cluster, double separation, const qs_plan_params *params,
                                           const qs_gain_params *gain_params, const double *bot_xy, size_t n_bots,
                                           int64_t *target_idx, double *target_xy, uint32_t *cost, int32_t *status,
                                           int32_t *wp_cell_xy, double *wp_xy, double *centroids_xy, size_t cap,
                                           size_t *n_centroids, int32_t *target_gain, uint64_t stats[8])
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n_bots == 0 || target_gain);
    qs_gain_params g = {QS_GAIN_DEFAULT_RANGE, QS_GAIN_DEFAULT_BIAS, {0, 0}};
    if (gain_params) g = *gain_params;
    int rc = gain_range(c, g.range, "qs_frontier_targets_by_gain");
    if (rc != QS_OK) return rc;
    if (g.bias > QS_GAIN_MAX_BIAS) return qs_fail(c, QS_E_INVAL, "qs_frontier_targets_by_gain: bias above QS_GAIN_MAX_BIAS");
    if (g.reserved[0] || g.reserved[1]) return qs_fail(c, QS_E_INVAL, "qs_frontier_targets_by_gain: reserved must be 0");
    std::vector<int> hgain;
    rc = tbp_run<GnEntry>(c, "qs_frontier_targets_by_gain", min_cluster, separation, params,
        [&](void *fws, size_t n_cent, GnAux &aux) {
            HIPCHK(c, c->gain_ws.reserve(qs_gain_layout(nullptr, n_cent).bytes, c->stream));
            const QsGainLayout G = qs_gain_layout(c->gain_ws.p, n_cent);
            HIPCHK(c, qs_launch_gain(c, fws, min_cluster, g.range, n_cent, G));
            hgain.resize(n_cent);             // (read after the call's last synchronise)
            if (n_cent) HIPCHK(c, hipMemcpyAsync(hgain.data(), G.gain, n_cent * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            aux = GnAux{G.gain, g.bias};
            return (int)QS_OK;
        }, bot_xy, n_bots, {target_idx, target_xy, cost, status, wp_cell_xy, wp_xy}, centroids_xy, cap, n_centroids, stats);
    if (rc != QS_OK) return rc;
    for (size_t b = 0; b < n_bots; b++) target_gain[b] = target_idx[b] >= 0 ? hgain[(size_t)target_idx[b]] : 0;
    if (stats) for (int v : hgain) stats[7] += (uint64_t)v;
    return QS_OK;
}
