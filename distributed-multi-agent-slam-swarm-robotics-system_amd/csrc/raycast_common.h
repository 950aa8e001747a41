// raycast_common.h -- device helpers shared by the direct and the tile-binned raycast.
#pragma once
#include "qs_internal.h"

#define QS_LL_BAD (-0x7fffffffffffffffll - 1)
#define QS_MAX_RAY_CELLS (1 << 24)   // ABI limit on one ray's length in cells (update_rays API)

// OccupancyGrid.world_to_grid  dual_bot_mapper.py:121-125: int((w - o) / res) -- fp64
// subtract, fp64 DIVIDE (not a multiply by 1/res: (0.05+5)/0.05 = 100.99999999999999 -> 100),
// truncation toward zero (not floor: (-5.049+5)/0.05 = -0.98 -> 0).
__device__ inline long long qs_w2g_ll(double w, double o, double res)
{
    const double q = (w - o) / res;
    if (!(fabs(q) < 9.0e15)) return QS_LL_BAD;   // CPython would raise / walk 1e15 cells
    return (long long)q;
}

// Same value as an int, without the divide in the common case.  qa = (w - o) * (1 / res) is within
// 2^-51 |q| of the correctly rounded quotient q; for |qa| < 1e9 that is < 5e-7, so when qa is more than
// 1e-4 away from every integer, no integer lies between qa and q and int(q) == int(qa).  Otherwise
// (one coordinate in ~5000, e.g. the 100.99999999999999 case above) the quotient itself decides.
// Cells beyond +-2^30 are clamped there: every grid is < 2^14 wide, so such an end point can only
// make a ray miss the grid or exceed the QS_MAX_RAY_CELLS limit, clamped or not.
#define QS_CELL_CLAMP (1 << 30)
__device__ inline bool qs_w2g_i32(double w, double o, const QsGeom &geo, int &out)
{
    const double qa = (w - o) * geo.inv_res;
    if (fabs(qa) < 1.0e9 && fabs(qa - rint(qa)) > 1.0e-4) { out = (int)qa; return true; }
    const long long q = qs_w2g_ll(w, o, geo.res);
    if (q == QS_LL_BAD) return false;
    out = q > QS_CELL_CLAMP ? QS_CELL_CLAMP : (q < -QS_CELL_CLAMP ? -QS_CELL_CLAMP : (int)q);
    return true;
}

// Sparse fuse (sparse_fuse.hip): a writer that goes straight to the grid marks the block of every cell it writes.  The bit
// is read first: a ray's cells share a block four to sixteen at a time and the rays of a batch share rooms, so almost
// every mark finds its bit set and costs one cached load (a stale 0 only repeats the atomic; bits are never cleared
// while writers run).
__device__ inline void qs_mark_dirty(const QsGeom &geo, int x, int y)
{
    if (geo.dirty) {
        unsigned int *w = geo.dirty + qs_dirty_word(x, y, geo.dirty_pitch);
        const unsigned int m = qs_dirty_mask(x);
        if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & m)) atomicOr(w, m);
    }
}

struct QsRay { double ex, ey; bool valid; };

// Stamp of a ray's free cells: (ordinal << 1) | 0 with ordinal = the ray's arrival index + 1 (bit 0: the occupied bit of a cell
// stamp).  Packets: arrival index ord_base + ord_stride * packet + sensor; sweeps: ord_base + ray slot.
__host__ __device__ inline unsigned int qs_stamp_key(unsigned long long arrival) { return (unsigned int)((arrival + 1) << 1); }
// the arrival index of sequence number seq0's first ray in the current stamp epoch, and the step from one packet to the next
inline unsigned long long qs_ord_base(const qs_ctx *c, uint64_t seq0) { return 4ull * (seq0 - c->epoch_base); }
inline unsigned long long qs_ord_stride(const qs_ctx *c) { return 4ull * (unsigned long long)(c->cfg.seq_stride > 0 ? c->cfg.seq_stride : 1); }

// sin and cos of a ray heading: the device library's fp64 sincos (one argument reduction for both;
// same bits as its separate sin and cos).  A Cody-Waite + fdlibm-kernel version for |a| < 1e5 was
// measured at -2 us per 1 M packets on this pass and dropped: not worth a second implementation of a
// value that decides cells.
__device__ inline void qs_sincos(double x, double *sn, double *cs) { sincos(x, sn, cs); }

// The range rule of dual_bot_mapper.py:888 / :900 for the trust filter lo < d <= hi: hit_valid = lo < d <= hi; invalid rays
// extend to min(d, hi) if d > lo else hi and only clear cells.  NaN compares false everywhere, which gives the reference's
// behaviour (a full-length free ray) without a special case.  The host's exact-trig loop (qs_api.hip) applies the same rule.
struct QsRange { bool valid; double range; };
__host__ __device__ inline QsRange qs_range_rule(double d, double lo, double hi)
{
    QsRange g;
    g.valid = (lo < d) && (d <= hi);                                                   // :888
    g.range = g.valid ? d : ((d > lo) ? ((hi < d) ? hi : d) : hi);                     // :900
    return g;
}

// end point of the ray of that range from (rx, ry) at heading a: one multiply and one add per axis (no FMA: the library is
// built with -ffp-contract=off)
__device__ inline QsRay qs_ray_end(double rx, double ry, double a, const QsRange &g)
{
    double sa, ca;
    qs_sincos(a, &sa, &ca);
    QsRay r;
    r.valid = g.valid;
    r.ex = rx + g.range * ca;                                                         // :890 / :901
    r.ey = ry + g.range * sa;                                                         // :891 / :902
    return r;
}

// dual_bot_mapper.py:886-903: sensor order front(0), left(+pi/2), back(pi), right(-pi/2)
__device__ inline QsRay qs_project_ray(double rx, double ry, double yaw, double d, int s, const QsGeom &geo)
{
    const double kPi = 3.141592653589793;   // math.pi
    const double ang = s == 0 ? 0.0 : (s == 1 ? kPi / 2 : (s == 2 ? kPi : -kPi / 2));   // :61-66
    return qs_ray_end(rx, ry, yaw + ang, qs_range_rule(d, geo.min_dist, geo.max_dist));   // :887
}

// Exact-trig mode.  The device library's sin / cos may differ from glibc's (the reference's math.cos / math.sin) in
// the last bit; after `r * cos + rx` that is at most one ulp of the end point (< 6e-13 cells at 200 m and 5 cm), which
// can only change int((w - o) / res) if the quotient lies that close to an integer.  Rays whose end-point quotient is
// within 1e-9 (+ 1e-14 relative) of an integer on either axis are therefore not decided here: the host recomputes their
// end points with libm and casts them with their own stamps (any order gives the same grid).
__device__ inline bool qs_edge_coord(double w, double o, const QsGeom &geo)
{
    const double qa = (w - o) * geo.inv_res;
    return fabs(qa - rint(qa)) <= 1.0e-9 + fabs(qa) * 1.0e-14;
}
__device__ inline bool qs_edge_ray(const QsRay &ray, const QsGeom &geo)
{
    return qs_edge_coord(ray.ex, geo.ox, geo) || qs_edge_coord(ray.ey, geo.oy, geo);
}

// leave the ray to the host; false: the list is full (the caller casts the ray with the device's end point after all)
// beam: index of a servo-sweep beam (sweep.hip), -1 for the four rays of a QuasarPacket
__device__ inline bool qs_edge_defer(const QsBatch &b, double rx, double ry, double yaw, float d, unsigned int key_free,
                                     int beam = -1)
{
    const unsigned int slot = atomicAdd(b.edge_n, 1u);
    if (slot >= b.edge_cap) { atomicAdd(b.edge_n + 2, 1u); return false; }
    QsEdgeRec rec; rec.rx = rx; rec.ry = ry; rec.yaw = yaw; rec.d = d; rec.key_free = key_free; rec.beam = beam; rec.pad = 0;
    b.edge[slot] = rec;
    return true;
}

struct QsLine { int x0, y0, x1, y1, dx, dy, sx, sy; };

// Grid end points of a ray and the Bresenham set-up of :158-165.  Returns false when no cell
// of the ray can be inside the grid (or the ray exceeds the ABI length limit): the reference
// would walk the same cells and skip every one of them (:149, :155).
__device__ inline bool qs_line_setup(const QsRay &ray, double rx, double ry, const QsGeom &geo, QsLine &ln)
{
    int x0, y0, x1, y1;
    bool ok = qs_w2g_i32(rx, geo.ox, geo, x0);                                                      // :142
    ok = qs_w2g_i32(ry, geo.oy, geo, y0) && ok;
    ok = qs_w2g_i32(ray.ex, geo.ox, geo, x1) && ok;                                                 // :143
    ok = qs_w2g_i32(ray.ey, geo.oy, geo, y1) && ok;
    if (!ok) return false;
    const int xlo = min(x0, x1), xhi = max(x0, x1), ylo = min(y0, y1), yhi = max(y0, y1);
    // |coordinates| <= 2^30: the differences below are exact in 32-bit unsigned arithmetic
    const unsigned int dx = (unsigned int)xhi - (unsigned int)xlo, dy = (unsigned int)yhi - (unsigned int)ylo;
    if (xhi < 0 || yhi < 0 || xlo >= geo.size || ylo >= geo.size) return false;
    if (dx > QS_MAX_RAY_CELLS || dy > QS_MAX_RAY_CELLS) return false;
    ln.x0 = x0; ln.y0 = y0; ln.x1 = x1; ln.y1 = y1;
    ln.dx = (int)dx; ln.dy = (int)dy;                                                                // :161-162
    ln.sx = x0 < x1 ? 1 : -1; ln.sy = y0 < y1 ? 1 : -1;                                             // :163-164
    return true;
}

// The walk of :158-178 straight into the grid, one global atomic per cell (the direct form); returns the cells written.
// The last cell is written only for an observed hit (:148-150); cells outside the grid are skipped (:149, :155).
template <bool COUNTS>
__device__ inline unsigned int qs_cast_line(const QsLine &ln, bool valid, unsigned int key_free, const QsGeom &geo,
                                            unsigned int *__restrict__ stamps, unsigned long long *__restrict__ counts)
{
    unsigned int cells = 0;
    int x = ln.x0, y = ln.y0, err = ln.dx - ln.dy;
    for (;;) {
        const bool last = (x == ln.x1 && y == ln.y1);
        if ((!last || valid) && x >= 0 && x < geo.size && y >= 0 && y < geo.size) {
            const size_t c = (size_t)y * geo.size + x;
            atomicMax(&stamps[c], key_free | (last ? 1u : 0u));
            qs_mark_dirty(geo, x, y);
            if (COUNTS) atomicAdd(&counts[c], last ? (1ull << 32) : 1ull);
            cells++;
        }
        if (last) break;
        const int e2 = 2 * err;
        if (e2 > -ln.dy) { err -= ln.dy; x += ln.sx; }
        if (e2 < ln.dx) { err += ln.dx; y += ln.sy; }
    }
    return cells;
}

// What every raycast kernel does with a projected ray before its cells.  Exact-trig mode: a ray on a cell edge is left to the
// host (qs_edge_defer); otherwise the Bresenham set-up.  true: ln holds a line to walk or bin.
// d: the raw range (the host projects from it again); beam: a sweep's beam index, -1 for the four rays of a QuasarPacket
__device__ inline bool qs_ray_line(const QsRay &ray, double rx, double ry, double yaw, float d, unsigned int key_free, int beam,
                                   const QsBatch &b, const QsGeom &geo, QsLine &ln)
{
    if (b.edge && qs_edge_ray(ray, geo) && qs_edge_defer(b, rx, ry, yaw, d, key_free, beam))
        return false;                                      // the host decides this ray's cells (qs_api.hip: sync_host_state)
    return qs_line_setup(ray, rx, ry, geo, ln);
}

// The direct sink of a projected ray: deferred, or cast with one global atomic per cell; returns the cells written.
template <bool COUNTS>
__device__ inline unsigned int qs_ray_direct(const QsRay &ray, double rx, double ry, double yaw, float d, unsigned int key_free, int beam,
                                             const QsBatch &b, const QsGeom &geo, unsigned int *__restrict__ stamps,
                                             unsigned long long *__restrict__ counts)
{
    QsLine ln;
    if (!qs_ray_line(ray, rx, ry, yaw, d, key_free, beam, b, geo, ln)) return 0;
    return qs_cast_line<COUNTS>(ln, ray.valid, key_free, geo, stamps, counts);
}

// A thread's counts of what it cast, folded into the workgroup's LDS words s_cnt[QS_TALLY_WORDS] (zeroed by qs_tally_init before
// a barrier) and, after another barrier, flushed by one thread with one atomic per counter.  accepted: the sweep kernels' accepted
// records (the packet path's datagrams and accepted packets are the decoder's to count).
#define QS_TALLY_WORDS 4
struct QsTally { unsigned int rays = 0, cells = 0, hits = 0, accepted = 0; };

__device__ inline void qs_tally_init(unsigned int *s_cnt, int tid) { if (tid < QS_TALLY_WORDS) s_cnt[tid] = 0; }
__device__ inline void qs_tally_fold(const QsTally &t, unsigned int *s_cnt)
{
    if (t.rays) atomicAdd(&s_cnt[0], t.rays);
    if (t.cells) atomicAdd(&s_cnt[1], t.cells);
    if (t.hits) atomicAdd(&s_cnt[2], t.hits);
    if (t.accepted) atomicAdd(&s_cnt[3], t.accepted);
}
__device__ inline void qs_tally_flush(const unsigned int *s_cnt, unsigned long long *__restrict__ counters)
{
    if (s_cnt[0]) atomicAdd(&counters[QS_CNT_RAYS], (unsigned long long)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&counters[QS_CNT_CELLS], (unsigned long long)s_cnt[1]);
    if (s_cnt[2]) atomicAdd(&counters[QS_CNT_HITS], (unsigned long long)s_cnt[2]);
}
// the sweep kernels' form: the workgroup's records are datagrams that no decoder has counted
__device__ inline void qs_tally_flush(const unsigned int *s_cnt, unsigned long long *__restrict__ counters, unsigned long long datagrams)
{
    atomicAdd(&counters[QS_CNT_DATAGRAMS], datagrams);
    if (s_cnt[3]) atomicAdd(&counters[QS_CNT_ACCEPTED], (unsigned long long)s_cnt[3]);
    qs_tally_flush(s_cnt, counters);
}

// Host side: launches the COUNTS = true or the COUNTS = false instantiation of a kernel, as the context was created.
template <typename... P, typename... A>
inline void qs_launch_counts(const qs_ctx *c, void (*on)(P...), void (*off)(P...), dim3 grid, dim3 block, size_t lds, A... args)
{
    hipLaunchKernelGGL(c->cfg.enable_counts ? on : off, grid, block, lds, c->stream, args...);
}

// Bounding box of a bot's hit points and path (compute_bounding_box, dual_bot_mapper.py:702-706),
// exact min / max in any order.  The workgroup's copy lives in LDS as doubles and takes native
// ds_min_f64 / ds_max_f64 atomics without return: eight instructions per ray, no key conversion and
// nothing to wait for.  (Measured alternatives, 1 M packets: read-compare-then-atomic on ordered u64
// keys +25 us on the pass, per-thread register boxes flushed on a bot change +15 us -- the bot of a
// thread's next ray differs 60 % of the time on the 2-bot stream; this form +6 us.)
#define QS_ZONE_LDS_INIT(z, t) do { (z)[t][0] = __builtin_inf(); (z)[t][1] = __builtin_inf(); \
                                    (z)[t][2] = -__builtin_inf(); (z)[t][3] = -__builtin_inf(); } while (0)

__device__ inline void qs_zone_point(double (*s_zone)[4], int agent, double x, double y)
{
    double *z = s_zone[agent];
    __hip_atomic_fetch_min(&z[0], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_min(&z[1], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_max(&z[2], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_max(&z[3], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// fold the workgroup's box of bot t into the session's (order-preserving u64 keys in HBM).  The
// session's box rarely moves: read first, serialise on its 4 words only when it does.
__device__ inline void qs_zone_commit(const double (*s_zone)[4], int t, unsigned long long *__restrict__ zone)
{
    if (!(s_zone[t][0] <= s_zone[t][2])) return;        // no point of this bot in this workgroup
    const volatile unsigned long long *zg = zone + 4 * t;
    const unsigned long long k0 = qs_ord_from_double(s_zone[t][0]), k1 = qs_ord_from_double(s_zone[t][1]);
    const unsigned long long k2 = qs_ord_from_double(s_zone[t][2]), k3 = qs_ord_from_double(s_zone[t][3]);
    if (k0 < zg[0]) atomicMin(&zone[4 * t + 0], k0);
    if (k1 < zg[1]) atomicMin(&zone[4 * t + 1], k1);
    if (k2 > zg[2]) atomicMax(&zone[4 * t + 2], k2);
    if (k3 > zg[3]) atomicMax(&zone[4 * t + 3], k3);
}
