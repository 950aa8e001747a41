// territory.hip -- the mapped free space partitioned among the bots by path cost.
// The rules are this build's own (include/quasar_slam.h, "territories"), all integer.  The mask, the census, the snap, the
// worklist ring and the waypoint stage are plan.hip's (plan_common.h); the centroids are frontier_targets.hip's, their field
// offsets, the argument check and the per-bot epilogue targets_by_path.hip's.  New here:
//
//   seed     : ONE field over the bounding box of the census, of 64-bit keys (cost << 32) | bot.  Every bot with a cell
//              writes key = bot at its cell by atomicMin (bots that share a cell: the lowest stays) and enters its tile,
//              and the tiles across a border or corner it sits on, in the first list; the round mark keeps a tile that
//              several bots seed to one entry;
//   rounds   : plan.hip's round kernel and round driver, instantiated for the 64-bit key (plan_rounds_key64): halo,
//              segmented min-plus scans along rows, columns and both diagonals both ways, border-improvement bits,
//              neighbour append.  A candidate is key[n] + (step << 32), so the minimum orders by cost first, then by
//              bot: the fixpoint is rule T3 and is unique;
//   split    : one pass over the final field writes owner and cost where asked and reduces area and box per bot: a wave
//              holds a tile row, loops a ballot over the distinct owners of the row, and its first lane of each owner
//              issues one 64-bit atomicAdd and four atomicMin / atomicMax.  Integer atomics: the result is exact;
//   centroids: gather key at each centroid's field offset; atomicMin of (cost << 32) | k into the owner's slot; one wave
//              turns the slots into targets and the (start, goal) pairs of the assigned bots, in bot order;
//   waypoints: plan.hip's waypoint stage for those pairs, as qs_frontier_targets_by_path runs it.
// No device-side waits, no grid-wide barriers, no graphs.
#include <math.h>
#include <algorithm>

#include "territory_layout.h"

static_assert(PL_T == QS_WAVE, "one lane per cell of a tile row");

#define TK_INF 0xffffffffffffffffull

// ---- per-bot state of a call: empty slot, no cells, the empty box as the identities of min and max ------------------
__global__ void __launch_bounds__(PL_BLOCK)
qs_terr_init_kernel(int n_bots, unsigned long long *__restrict__ slot, unsigned long long *__restrict__ area, int *__restrict__ box)
{
    const int b = blockIdx.x * PL_BLOCK + threadIdx.x;
    if (b >= n_bots) return;
    slot[b] = TK_INF;
    area[b] = 0;
    box[4 * b] = box[4 * b + 1] = 0x7fffffff;
    box[4 * b + 2] = box[4 * b + 3] = -1;
}

// ---- seed ------------------------------------------------------------------------------------------------------------
// As qs_plan_seed_kernel (plan.hip): the seed cell never improves, so a bot on a tile's border row, column or corner also
// enters the tiles across it.  marks: 1 = in the list of round 1.
__global__ void __launch_bounds__(PL_BLOCK)
qs_terr_seed_kernel(const long long *__restrict__ bot_cell, int n_bots, int size, PlBox B, const unsigned int *__restrict__ tile_any,
                    int gtx, unsigned long long *__restrict__ key, unsigned int *__restrict__ list, unsigned int *__restrict__ cnt,
                    unsigned int *__restrict__ marks)
{
    const int b = blockIdx.x * PL_BLOCK + threadIdx.x;
    if (b >= n_bots) return;
    const long long s = bot_cell[b];
    if (s < 0) return;
    const int fx = (int)(s % size) - B.bx0 * PL_T, fy = (int)(s / size) - B.by0 * PL_T;
    if (fx < 0 || fy < 0 || fx >= B.fw || fy >= B.fh) return;      // (a cell is traversable, so it lies in the box)
    atomicMin(&key[(size_t)fy * B.fw + fx], (unsigned long long)b);
    const int tx = fx / PL_T, ty = fy / PL_T;
    const int ex = fx % PL_T == 0 ? -1 : (fx % PL_T == PL_T - 1 ? 1 : 0), ey = fy % PL_T == 0 ? -1 : (fy % PL_T == PL_T - 1 ? 1 : 0);
    for (int k = 0; k < 4; k++) {                           // the tile, then those across x, across y, across the corner
        const int nx = tx + ((k & 1) ? ex : 0), ny = ty + ((k & 2) ? ey : 0);
        if (((k & 1) && !ex) || ((k & 2) && !ey)) continue;
        if (nx < 0 || ny < 0 || nx >= B.ntx || ny >= B.nty || !tile_any[(size_t)(B.by0 + ny) * gtx + B.bx0 + nx]) continue;
        const unsigned int item = (unsigned int)(ny * B.ntx + nx);
        if (atomicExch(&marks[item], 1u) != 1u) list[atomicAdd(&cnt[1], 1u)] = item;
    }
}

// ---- split -------------------------------------------------------------------------------------------------------------
// one workgroup per tile of the box, a wave per tile row.  owner / cost (optional, [size][size], preset to -1 / unreached)
// get the owned cells; area and box get one set of atomics per distinct owner of a row.
__global__ void __launch_bounds__(PL_BLOCK)
qs_terr_split_kernel(const unsigned long long *__restrict__ key, PlBox B, int size, const unsigned int *__restrict__ tile_any,
                     int gtx, short *__restrict__ owner, unsigned int *__restrict__ cost, unsigned long long *__restrict__ area,
                     int *__restrict__ box)
{
    if (!tile_any[(size_t)(B.by0 + blockIdx.y) * gtx + B.bx0 + blockIdx.x]) return;      // no traversable cell: no key
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fx = blockIdx.x * PL_T + lane, gx0 = (B.bx0 + blockIdx.x) * PL_T, gx = gx0 + lane;
    for (int y = wave; y < PL_T; y += PL_BLOCK / QS_WAVE) {
        const int fy = blockIdx.y * PL_T + y, gy = B.by0 * PL_T + fy;
        const unsigned long long k = key[(size_t)fy * B.fw + fx];
        const int o = k == TK_INF || gx >= size || gy >= size ? -1 : (int)(unsigned int)k;
        if (o >= 0) {
            if (owner) owner[(size_t)gy * size + gx] = (short)o;
            if (cost) cost[(size_t)gy * size + gx] = (unsigned int)(k >> 32);
        }
        unsigned long long todo = __ballot(o >= 0);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int ow = __shfl(o, lead);
            const unsigned long long mm = __ballot(o == ow);
            if (lane == lead) {
                atomicAdd(&area[ow], (unsigned long long)__popcll(mm));
                atomicMin(&box[4 * ow], gx0 + __ffsll((long long)mm) - 1);
                atomicMin(&box[4 * ow + 1], gy);
                atomicMax(&box[4 * ow + 2], gx0 + 63 - __clzll((long long)mm));
                atomicMax(&box[4 * ow + 3], gy);
            }
            todo &= ~mm;
        }
    }
}

// ---- centroids -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PL_BLOCK)
qs_terr_gather_kernel(const unsigned long long *__restrict__ key, const unsigned int *__restrict__ coff, int n_cent,
                      int *__restrict__ cent_owner, unsigned int *__restrict__ cent_cost, unsigned long long *__restrict__ slot,
                      unsigned long long *__restrict__ count)
{
    const int k = blockIdx.x * PL_BLOCK + threadIdx.x;
    unsigned long long v = TK_INF;
    if (k < n_cent) {
        const unsigned int o = coff[k];
        if (o != TP_NOCELL) v = key[o];
        cent_owner[k] = v == TK_INF ? -1 : (int)(unsigned int)v;
        cent_cost[k] = v == TK_INF ? PL_INF : (unsigned int)(v >> 32);
        if (v != TK_INF) atomicMin(&slot[(unsigned int)v], (v & 0xffffffff00000000ull) | (unsigned int)k);
    }
    const unsigned long long m = __ballot(v != TK_INF);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&count[2], (unsigned long long)__popcll(m));
}

// one wave: the slots into targets; the assigned bots' (start, goal) cells compacted in bot order for the waypoint stage
__global__ void __launch_bounds__(64)
qs_terr_targets_kernel(const unsigned long long *__restrict__ slot, const double2 *__restrict__ xy, const long long *__restrict__ cell,
                       int n_cent, int n_bots, long long *__restrict__ tgt_idx, double2 *__restrict__ tgt_xy,
                       unsigned int *__restrict__ tgt_cost, int *__restrict__ tgt_status, long long *__restrict__ pair,
                       int *__restrict__ pair_bot, unsigned long long *__restrict__ count)
{
    const int lane = threadIdx.x;
    int m = 0;
    for (int base = 0; base < n_bots; base += 64) {
        const int b = base + lane;
        bool got = false;
        long long bc = -1;
        int k = -1;
        if (b < n_bots) {
            bc = cell[n_cent + b];
            const unsigned long long s = bc >= 0 ? slot[b] : TK_INF;
            got = s != TK_INF;
            k = got ? (int)(unsigned int)s : -1;
            tgt_idx[b] = k;
            tgt_cost[b] = got ? (unsigned int)(s >> 32) : PL_INF;
            tgt_status[b] = bc < 0 ? QS_PLAN_NO_START : (got ? QS_PLAN_OK : QS_PLAN_UNREACHABLE);
            tgt_xy[b] = got ? xy[k] : make_double2(NAN, NAN);
        }
        const unsigned long long mm = __ballot(got);
        if (got) {
            const int i = m + __popcll(mm & ((1ull << lane) - 1ull));
            pair[i] = bc; pair[n_bots + i] = cell[k]; pair_bot[i] = b;
        }
        m += __popcll(mm);
    }
    if (lane == 0) count[3] = (unsigned long long)m;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// What both entry points share: the mask and the census, the cells of the centroids (T.tg.xy[0 .. n_cent), already on the
// device) and of the bots, the partition, and area / box / owner / cost.  bcell: the bots' cells, on the host.
static int terr_partition(qs_ctx *c, const qs_plan_params &p, const QsTerrLayout &T, const double *bot_xy, size_t n_cent,
                          size_t n_bots, QsPlanLayout &L, unsigned int bbox[4], std::vector<long long> &bcell)
{
    int rc = plan_begin(c, p.clearance, std::max(n_bots, (size_t)1), 0, L, bbox);
    if (rc != QS_OK) return rc;
    const QsTgtLayout &S = T.tg;
    const size_t cells = (size_t)c->cfg.size * c->cfg.size, n_end = n_cent + n_bots;
    HIPCHK(c, hipMemsetAsync(S.count, 0, 4 * sizeof(unsigned long long), c->stream));
    if (T.owner) HIPCHK(c, hipMemsetAsync(T.owner, 0xff, cells * sizeof(short), c->stream));            // -1
    if (T.cost) HIPCHK(c, hipMemsetAsync(T.cost, 0xff, cells * sizeof(unsigned int), c->stream));       // unreached
    if (n_bots) {
        hipLaunchKernelGGL(qs_terr_init_kernel, dim3((unsigned int)((n_bots + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0,
                           c->stream, (int)n_bots, T.slot, T.area, T.box);
        HIPCHK(c, hipGetLastError());
    }
    bcell.assign(n_bots, -1);
    if (bbox[0] > bbox[2]) return QS_OK;                  // nothing is traversable: nothing snaps, nobody owns anything
    const PlBox B = pl_box(bbox);
    const size_t fcells = (size_t)B.fw * B.fh, tiles = (size_t)B.ntx * B.nty;
    if (fcells > T.field_cells || tiles > L.item_cap) return qs_fail(c, QS_E_STATE, "territories: the census box exceeds the workspace");
    HIPCHK(c, hipMemsetAsync(T.key, 0xff, fcells * sizeof(unsigned long long), c->stream));
    if (n_end) {
        if (n_bots) HIPCHK(c, hipMemcpyAsync(S.xy + n_cent, bot_xy, n_bots * sizeof(double2), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, qs_launch_plan_snap(c, L, S.xy, S.cell, n_end, p.snap_radius, L.stats + 3));
        HIPCHK(c, qs_launch_tbp_offsets(c, S.cell, n_cent, n_bots, bbox, S.coff, S.count));
    }
    if (!n_bots) return QS_OK;
    HIPCHK(c, hipMemcpyAsync(bcell.data(), S.cell + n_cent, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(L.marks, 0, tiles * sizeof(unsigned int), c->stream));
    HIPCHK(c, hipMemsetAsync(L.cnt, 0, 3 * sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(qs_terr_seed_kernel, dim3((unsigned int)((n_bots + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, c->stream,
                       S.cell + n_cent, (int)n_bots, c->cfg.size, B, L.tile_any, L.gtx, T.key, L.list1, L.cnt, L.marks);
    HIPCHK(c, hipGetLastError());
    rc = plan_rounds_key64(c, L, bbox, T.key);
    if (rc != QS_OK) return rc;
    hipLaunchKernelGGL(qs_terr_split_kernel, dim3(B.ntx, B.nty), dim3(PL_BLOCK), 0, c->stream, T.key, B, c->cfg.size, L.tile_any,
                       L.gtx, T.owner, T.cost, T.area, T.box);
    HIPCHK(c, hipGetLastError());
    return QS_OK;
}

// status, area and box of the bots from what terr_partition left (the stream is synchronised here); returns the cells owned
static int terr_per_bot(qs_ctx *c, const QsTerrLayout &T, const std::vector<long long> &bcell, bool any_trav, int32_t *status,
                        int64_t *area, int32_t *box, uint64_t &owned)
{
    const size_t n_bots = bcell.size();
    std::vector<unsigned long long> a(n_bots, 0);
    std::vector<int> bx(4 * n_bots, -1);
    if (n_bots && any_trav) {
        HIPCHK(c, hipMemcpyAsync(a.data(), T.area, n_bots * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(bx.data(), T.box, 4 * n_bots * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    owned = 0;
    for (size_t b = 0; b < n_bots; b++) {
        if (status) status[b] = bcell[b] < 0 ? QS_PLAN_NO_START : QS_PLAN_OK;
        owned += a[b];
        if (area) area[b] = (int64_t)a[b];
        if (box)
            for (int k = 0; k < 4; k++) box[4 * b + k] = a[b] ? bx[4 * b + k] : -1;
    }
    return QS_OK;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
extern "C" int qs_territories(qs_ctx *c, const qs_plan_params *params, const double *bot_xy, size_t n_bots, int16_t *owner_host,
                              uint32_t *cost_host, int32_t *status, int64_t *area, int32_t *box, uint64_t stats[8])
{
    ARGCHK(c, c != nullptr);
    if (n_bots > QS_FT_MAX_BOTS) return qs_fail(c, QS_E_INVAL, "qs_territories: n_bots above QS_FT_MAX_BOTS");
    ARGCHK(c, n_bots == 0 || (bot_xy && status && area && box));
    qs_plan_params p;
    int rc = plan_params(c, params, p);
    if (rc != QS_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    const int size = c->cfg.size;
    HIPCHK(c, c->terr_ws.reserve(qs_terr_layout(nullptr, size, 0, n_bots, owner_host != nullptr, cost_host != nullptr).bytes, c->stream));
    const QsTerrLayout T = qs_terr_layout(c->terr_ws.p, size, 0, n_bots, owner_host != nullptr, cost_host != nullptr);
    QsPlanLayout L;
    unsigned int bbox[4];
    std::vector<long long> bcell;
    rc = terr_partition(c, p, T, bot_xy, 0, n_bots, L, bbox, bcell);
    if (rc != QS_OK) return rc;
    const size_t cells = (size_t)size * size;
    unsigned long long st[4] = {0, 0, 0, 0}, count[4] = {0, 0, 0, 0};
    if (owner_host) HIPCHK(c, hipMemcpyAsync(owner_host, T.owner, cells * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    if (cost_host) HIPCHK(c, hipMemcpyAsync(cost_host, T.cost, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, L.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(count, T.tg.count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    uint64_t owned = 0;
    rc = terr_per_bot(c, T, bcell, bbox[0] <= bbox[2], status, area, box, owned);
    if (rc != QS_OK) return rc;
    if (stats) {
        stats[0] = st[0]; stats[1] = st[1]; stats[2] = count[1]; stats[3] = owned;
        stats[4] = stats[5] = stats[6] = stats[7] = 0;
    }
    return QS_OK;
}

extern "C" int qs_frontier_targets_by_territory(qs_ctx *c, int32_t min_cluster, const qs_plan_params *params, const double *bot_xy,
                                                size_t n_bots, int64_t *target_idx, double *target_xy, uint32_t *cost,
                                                int32_t *status, int32_t *wp_cell_xy, double *wp_xy, int64_t *area, int32_t *box,
                                                double *centroids_xy, int32_t *centroid_owner, size_t cap, size_t *n_centroids,
                                                uint64_t stats[8])
{
    static const char who[] = "qs_frontier_targets_by_territory";
    const QsTargetsOut o{target_idx, target_xy, cost, status, wp_cell_xy, wp_xy};
    qs_plan_params p;
    int rc = tbp_check_args(c, who, n_bots, bot_xy, o, centroids_xy, cap, params, p);
    if (rc != QS_OK) return rc;
    ARGCHK(c, n_bots == 0 || (area && box));
    // the centroids (frontier_targets.hip's), counted first
    void *fws;
    size_t n_cent;
    rc = qs_count_centroids(c, min_cluster, fws, n_cent);
    if (rc != QS_OK) return rc;
    HIPCHK(c, c->terr_ws.reserve(qs_terr_layout(nullptr, c->cfg.size, n_cent, n_bots, false, false).bytes, c->stream));
    const QsTerrLayout T = qs_terr_layout(c->terr_ws.p, c->cfg.size, n_cent, n_bots, false, false);
    const QsTgtLayout &S = T.tg;
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 1, S.xy));
    // the partition, then who owns each centroid and each bot's cheapest
    QsPlanLayout L;
    unsigned int bbox[4];
    std::vector<long long> bcell;
    rc = terr_partition(c, p, T, bot_xy, n_cent, n_bots, L, bbox, bcell);
    if (rc != QS_OK) return rc;
    const bool any_trav = bbox[0] <= bbox[2];
    const size_t nc = n_cent < cap ? n_cent : cap;
    unsigned long long count[4] = {0, 0, 0, 0}, st[4] = {0, 0, 0, 0};
    QsTargetsHost H(n_bots);
    if (any_trav && n_cent) {
        hipLaunchKernelGGL(qs_terr_gather_kernel, dim3((unsigned int)((n_cent + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0,
                           c->stream, T.key, S.coff, (int)n_cent, T.cent_owner, T.cent_cost, T.slot, S.count);
        HIPCHK(c, hipGetLastError());
        if (centroid_owner && nc)
            HIPCHK(c, hipMemcpyAsync(centroid_owner, T.cent_owner, nc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    } else if (centroid_owner) {
        std::fill(centroid_owner, centroid_owner + nc, -1);
    }
    if (any_trav && n_bots) {
        hipLaunchKernelGGL(qs_terr_targets_kernel, dim3(1), dim3(64), 0, c->stream, T.slot, S.xy, S.cell, (int)n_cent, (int)n_bots,
                           S.tgt_idx, T.tgt_xy, S.tgt_cost, S.tgt_status, S.pair, S.pair_bot, S.count);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(H.idx.data(), S.tgt_idx, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(H.cost.data(), S.tgt_cost, n_bots * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(H.status.data(), S.tgt_status, n_bots * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(H.xy.data(), T.tgt_xy, n_bots * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    }
    if (any_trav) HIPCHK(c, hipMemcpyAsync(count, S.count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t m = (size_t)count[3];
    if (m > n_bots) return qs_fail(c, QS_E_STATE, "qs_frontier_targets_by_territory: assignment list is inconsistent");
    const bool walk = wp_xy && m;
    if (walk) {
        uint64_t groups = 0;                              // (not among this call's stats)
        rc = plan_waypoints(c, who, L, bbox, S.pair, S.pair + n_bots, m, p.lookahead, 0, groups, H.out4.data());
        if (rc != QS_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(H.pair_bot.data(), S.pair_bot, m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    if (nc) HIPCHK(c, hipMemcpyAsync(centroids_xy, S.xy, nc * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, L.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    uint64_t owned = 0;
    rc = terr_per_bot(c, T, bcell, any_trav, nullptr, area, box, owned);
    if (rc != QS_OK) return rc;
    rc = tbp_finish(c, who, "partition's", H, walk ? m : 0, o);      // (no walk: the pairs' bots stayed on the device)
    if (rc != QS_OK) return rc;
    if (n_centroids) *n_centroids = n_cent;
    if (stats) {
        stats[0] = st[0]; stats[1] = st[1]; stats[2] = count[1]; stats[3] = owned;
        stats[4] = n_cent; stats[5] = count[0]; stats[6] = count[2]; stats[7] = 0;
    }
    return QS_OK;
}
