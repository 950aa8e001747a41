// sweep.hip -- servo-sweep packets ("Quasar-Lite": pose + 181 ranges from -90 to +90 degrees about the heading) into the
// occupancy grid.  Semantics (include/quasar_slam.h, qs_ingest_sweeps): the reference's top-down sweep mapper
// (generate_topdown_map.py:39-57: beam angle ryaw + math.radians(i - 90), trust filter 0.1 < d <= 1.2) cast with its own
// OccupancyGrid.update_ray (dual_bot_mapper.py:136-179), pose = f32 pose + bot offset + the bot's drift correction.
//
// A record is 743 (v0) or 751 (v0 + odometry) bytes, so its ranges start at byte 19 or 27 of a record that starts at any
// byte: one WAVE per record.  The wave loads the record as aligned dwords (three coalesced 256-byte rows), stages them in
// its LDS slot, and each lane then takes beams lane, lane + 64, lane + 128: every range is one v_alignbyte of two LDS dwords
// (all ranges of a record share one shift), every header field a broadcast read.
//
// Sweep k of a call owns 184 ray slots (46 sequence numbers x 4), beam i slot 184 k + i with stamp ordinal
// 4 * (seq0 + 46 k) + i + 1; slots 181..183 are "no ray".  That is the slot / stamp layout passes B1, C, D of the tiled raycast
// already use for four rays per packet (raycast_tiled.h), so they run unchanged over the sweep's slots:
//   qs_sweep_rays_kernel    pass A: projection, grid end points, edge test, ray slots + hit flags, per-tile LDS histogram row;
//                           rays longer than a tile go to the grid directly (as qs_rays_kernel)
//   qs_sweep_direct_kernel  the whole cast with one global atomic per cell (small calls, raycast_mode 1)
// A sweep adds no pose-graph node, landmark, EKF step or zone point: those belong to the 42 / 41-byte path -- unless the context
// is in graph mode (qs_set_sweep_graph; sweep_graph.hip).  Then, before any chunk is mapped, a signature pass decides every record of
// the call and derives its landmark byte from the ranges, the unchanged SLAM stage adds the nodes and runs the loop-closure chain,
// and these kernels' GRAPH instantiations take acceptance and pose from the batch it left (sw_head_t) and add the zone points.
// The matched ingest (qs_ingest_sweeps_matched*, at the end of this file) runs match.hip's kernel over the whole call and then
// these kernels' CORR instantiations, which add each record's correction to its pose before anything else.
// The guarded ingest (qs_ingest_sweeps_checked*, same place) runs check.hip's kernel over the whole call and then these kernels'
// VETO instantiations, which treat a record its check contradicts as a rejected one.
// The bot veil for sweeps (veil.hip, rules S0-S8), while it acts, is a stage between pass A and the sort of every chunk: it reads what
// pass A left (accept, pose, ray slots, hit flags) and hands passes C and D the flags with the veiled beams taken out.
#include <math.h>
#include <algorithm>

#include "raycast_tiled.h"
#include "raycast_common.h"
#include "sweep_common.h"

#define SW_DIRECT_BLOCK 256       // direct kernel: 4 records per workgroup
#define QS_SWEEP_NO_VEIL ((size_t)-1)      // "the sweep veil is not acting" where a launch is told which record of the call it starts at

// beam i: angle ryaw + math.radians(i - 90) -- CPython's radians is x * (pi / 180), one multiply and one add (no FMA: the
// library is built with -ffp-contract=off); hit and free-ray rule as qs_project_ray's (A6): NaN, 0 and negative ranges give
// a full-length free ray
__device__ inline QsRay sw_beam(const SwHead &h, int i, double d, double smin, double smax)
{
    const double kRad = 3.141592653589793 / 180.0;
    return qs_ray_end(h.rx, h.ry, h.yaw + (double)(i - 90) * kRad, qs_range_rule(d, smin, smax));
}

__device__ inline void sw_out(const QsSweepArgs &a, size_t k, const SwHead &h)
{
    a.accept[k] = h.ok ? 1 : 0;
    if (h.ok) { a.pose[3 * k] = h.rx; a.pose[3 * k + 1] = h.ry; a.pose[3 * k + 2] = h.yaw; }
}

// graph mode's zone points of one record: every lane keeps the box of its own beams' hit points (lane 0 starts from the pose the
// sweep is cast from, paths[agent].append :878-879), the wave folds the 64 boxes -- min and max are exact in any order -- and
// lane 0 puts the result into the workgroup's box of the bot: eight LDS atomics per record (qs_zone_point for the low and for the
// high corner), not four per hit beam
struct SwBox { double x0, y0, x1, y1; };
__device__ inline SwBox sw_box(const SwHead &h)
{
    const bool p = h.ok && (threadIdx.x & (QS_WAVE - 1)) == 0;
    return SwBox{p ? h.rx : __builtin_inf(), p ? h.ry : __builtin_inf(), p ? h.rx : -__builtin_inf(), p ? h.ry : -__builtin_inf()};
}
__device__ inline void sw_box_point(SwBox &b, double x, double y)
{
    b.x0 = fmin(b.x0, x); b.y0 = fmin(b.y0, y); b.x1 = fmax(b.x1, x); b.y1 = fmax(b.y1, y);
}
// (every lane of the wave is here: the record's acceptance is uniform over it)
__device__ inline void sw_box_commit(SwBox b, double (*s_zone)[4], int agent, int lane)
{
    #pragma unroll
    for (int m = QS_WAVE / 2; m >= 1; m >>= 1) {
        b.x0 = fmin(b.x0, __shfl_xor(b.x0, m)); b.y0 = fmin(b.y0, __shfl_xor(b.y0, m));
        b.x1 = fmax(b.x1, __shfl_xor(b.x1, m)); b.y1 = fmax(b.y1, __shfl_xor(b.y1, m));
    }
    if (lane == 0) { qs_zone_point(s_zone, agent, b.x0, b.y0); qs_zone_point(s_zone, agent, b.x1, b.y1); }
}

// ---- pass A of the tiled raycast -----------------------------------------------------------------------------------------
// Workgroup w owns records [w * pk_per_wg, (w + 1) * pk_per_wg) (pk_per_wg a multiple of 16), its 16 waves one record each per
// round, and writes ray slots [184 * that range) plus its row of the tile table.
// CORR: the matched ingest's instantiation (every pose gets its record's correction first); the plain ingest's is CORR = false
// GRAPH: graph mode's (acceptance and pose from the batch slice; path and cloud points into the bots' zone boxes)
// VETO: the guarded ingest's (a record its check contradicts is a rejected record)
template <bool COUNTS, bool CORR, bool GRAPH, bool VETO>
__global__ void __launch_bounds__(QT_BIN_BLOCK)
qs_sweep_rays_kernel(QsSweepArgs a, QsBatch b, QsGeom geo, QtWorkspace ws, unsigned char *__restrict__ hit_valid,
                     unsigned int *__restrict__ stamps, unsigned long long *__restrict__ counts,
                     unsigned long long *__restrict__ counters)
{
    constexpr int NW = QT_BIN_BLOCK / QS_WAVE;
    extern __shared__ unsigned int s_hist[];                       // [n_tiles]
    __shared__ unsigned int s_rec[NW][SW_DW];
    __shared__ unsigned int s_cnt[QS_TALLY_WORDS];
    __shared__ double s_zone[GRAPH ? QS_MAX_AGENT + 1 : 1][4];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    for (int t = tid; t < ws.n_tiles; t += QT_BIN_BLOCK) s_hist[t] = 0;
    if (GRAPH) for (int t = tid; t <= a.max_agent; t += QT_BIN_BLOCK) QS_ZONE_LDS_INIT(s_zone, t);
    qs_tally_init(s_cnt, tid);
    const size_t k0 = (size_t)blockIdx.x * ws.pk_per_wg;
    const size_t k1 = (k0 + ws.pk_per_wg < a.n) ? k0 + ws.pk_per_wg : a.n;
    QsTally my;
    for (size_t kb = k0; kb < k1; kb += NW) {                     // (uniform over the workgroup)
        const size_t k = kb + wave;
        __syncthreads();                                           // the previous round's records are parsed
        sw_stage(a, k < k1 ? k : a.n, s_rec[wave], lane);
        __syncthreads();
        if (k >= k1) continue;
        const unsigned int *s = s_rec[wave];
        const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
        SwHead h = sw_head_t<GRAPH>(a, k, s, mis);
        if (CORR) sw_correct(a, k, h);
        if (VETO) sw_veto(a, k, h);
        if (lane == 0) { sw_out(a, k, h); my.accepted += h.ok ? 1u : 0u; }
        SwBox box = sw_box(h);
        #pragma unroll
        for (int q = 0; q < 3; q++) {
            const int i = lane + QS_WAVE * q;
            if (i >= 4 * QS_SWEEP_SEQS) break;
            const size_t r = QS_SWEEP_SLOTS * k + i;
            uint2 rec = make_uint2((unsigned int)QT_NO_RAY & 0xffffu, 0u);
            bool valid = false;
            if (h.ok && i < QS_SWEEP_BEAMS) {
                const float df = __uint_as_float(sw_u32(s, mis, a.ranges_off + 4u * (unsigned int)i));
                const QsRay ray = sw_beam(h, i, (double)df, a.smin, a.smax);
                valid = ray.valid;
                if (GRAPH && valid) sw_box_point(box, ray.ex, ray.ey);         // point_clouds[..].append  :892
                my.hits += valid ? 1u : 0u;
                my.rays++;
                rec = qt_ray_bin<COUNTS>(ray, h.rx, h.ry, h.yaw, df, qs_stamp_key(a.ord_base + r), i, b, geo, ws, s_hist, stamps, counts,
                                         my.cells);
            }
            ws.rays[r] = rec;
            hit_valid[r] = valid ? 1 : 0;
        }
        if (GRAPH && h.ok) sw_box_commit(box, s_zone, h.agent, lane);
    }
    qs_tally_fold(my, s_cnt);
    __syncthreads();
    unsigned int *row = ws.table + (size_t)blockIdx.x * ws.n_tiles;
    for (int t = tid; t < ws.n_tiles; t += QT_BIN_BLOCK) row[t] = s_hist[t];
    if (GRAPH) for (int t = tid; t <= a.max_agent; t += QT_BIN_BLOCK) qs_zone_commit(s_zone, t, a.zone);
    if (tid == 0) qs_tally_flush(s_cnt, counters, (unsigned long long)(k1 - k0));
}

// ---- direct form: one wave per record, every cell one global atomic --------------------------------------------------------
template <bool COUNTS, bool CORR, bool GRAPH, bool VETO>
__global__ void __launch_bounds__(SW_DIRECT_BLOCK)
qs_sweep_direct_kernel(QsSweepArgs a, QsBatch b, QsGeom geo, unsigned int *__restrict__ stamps,
                       unsigned long long *__restrict__ counts, unsigned long long *__restrict__ counters)
{
    constexpr int NW = SW_DIRECT_BLOCK / QS_WAVE;
    __shared__ unsigned int s_rec[NW][SW_DW];
    __shared__ unsigned int s_cnt[QS_TALLY_WORDS];
    __shared__ double s_zone[GRAPH ? QS_MAX_AGENT + 1 : 1][4];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    qs_tally_init(s_cnt, tid);
    if (GRAPH) for (int t = tid; t <= a.max_agent; t += SW_DIRECT_BLOCK) QS_ZONE_LDS_INIT(s_zone, t);
    const size_t k = (size_t)blockIdx.x * NW + wave;
    sw_stage(a, k, s_rec[wave], lane);
    __syncthreads();
    QsTally my;
    if (k < a.n) {
        const unsigned int *s = s_rec[wave];
        const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
        SwHead h = sw_head_t<GRAPH>(a, k, s, mis);
        if (CORR) sw_correct(a, k, h);
        if (VETO) sw_veto(a, k, h);
        if (lane == 0) { sw_out(a, k, h); my.accepted = h.ok ? 1u : 0u; }
        if (h.ok) {
            SwBox box = sw_box(h);
            #pragma unroll
            for (int q = 0; q < 3; q++) {
                const int i = lane + QS_WAVE * q;
                if (i >= QS_SWEEP_BEAMS) break;
                const float df = __uint_as_float(sw_u32(s, mis, a.ranges_off + 4u * (unsigned int)i));
                const QsRay ray = sw_beam(h, i, (double)df, a.smin, a.smax);
                if (GRAPH && ray.valid) sw_box_point(box, ray.ex, ray.ey);     // point_clouds[..].append  :892
                my.hits += ray.valid ? 1u : 0u;
                my.rays++;
                my.cells += qs_ray_direct<COUNTS>(ray, h.rx, h.ry, h.yaw, df, qs_stamp_key(a.ord_base + QS_SWEEP_SLOTS * k + i), i, b, geo,
                                                  stamps, counts);
            }
            if (GRAPH) sw_box_commit(box, s_zone, h.agent, lane);
        }
    }
    qs_tally_fold(my, s_cnt);
    __syncthreads();
    if (GRAPH) for (int t = tid; t <= a.max_agent; t += SW_DIRECT_BLOCK) qs_zone_commit(s_zone, t, a.zone);
    if (tid == 0) {
        const size_t k0 = (size_t)blockIdx.x * NW;
        qs_tally_flush(s_cnt, counters, (unsigned long long)(a.n - k0 < (size_t)NW ? a.n - k0 : (size_t)NW));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// n records of one chunk; seq0 of record 0; outputs per record (accept [n], pose [n][3]), hit flags [184 n]; veil_k0: QS_SWEEP_NO_VEIL,
// or (the sweep veil is acting, S0) the record of the call these records start at
template <bool CORR, bool GRAPH, bool VETO = false>
static hipError_t qs_launch_sweeps_t(qs_ctx *c, const QsSweepArgs &a, size_t n, bool tiled, unsigned char *hit_valid, size_t veil_k0)
{
    if (!tiled || !qs_tiled_supported(c)) {
        const unsigned int blocks = (unsigned int)((n + SW_DIRECT_BLOCK / QS_WAVE - 1) / (SW_DIRECT_BLOCK / QS_WAVE));
        qs_launch_counts(c, qs_sweep_direct_kernel<true, CORR, GRAPH, VETO>, qs_sweep_direct_kernel<false, CORR, GRAPH, VETO>, dim3(blocks),
                         dim3(SW_DIRECT_BLOCK), 0, a, c->b, c->geom, c->d_stamps.p, c->d_counts.p, c->d_counters.p);
        return hipGetLastError();
    }
    QtWorkspace ws;
    hipError_t e = qt_workspace(c, QS_SWEEP_SLOTS * n, ws);
    if (e != hipSuccess) return e;
    // records per workgroup: a multiple of the 16 waves, at most QT_MAX_WG workgroups
    constexpr size_t NW = QT_BIN_BLOCK / QS_WAVE;
    size_t per = (n + QT_MAX_WG - 1) / QT_MAX_WG;
    per = (per + NW - 1) / NW * NW;
    ws.pk_per_wg = per;
    ws.rays_per_wg = QS_SWEEP_SLOTS * per;
    ws.nwg = (int)((n + per - 1) / per);
    const auto on = qs_sweep_rays_kernel<true, CORR, GRAPH, VETO>, off = qs_sweep_rays_kernel<false, CORR, GRAPH, VETO>;
    size_t lds = 0;
    e = qt_dyn_lds(ws, (const void *)on, (const void *)off, lds);
    if (e != hipSuccess) return e;
    StageTimer t_rays(c, QS_STAGE_RC_RAYS);
    qs_launch_counts(c, on, off, dim3(ws.nwg), dim3(QT_BIN_BLOCK), lds, a, c->b, c->geom, ws, hit_valid, c->d_stamps.p, c->d_counts.p,
                     c->d_counters.p);
    t_rays.stop();
    const unsigned char *hv = hit_valid;
    if (veil_k0 != QS_SWEEP_NO_VEIL) {                     // bot veil, S3-S4: passes C and D read hit_valid & !veiled instead
        e = qs_launch_sweep_veil(c, a.pkts, a.stride, a.accept, a.pose, ws.rays, n, veil_k0, &hv);
        if (e != hipSuccess) return e;
    }
    // slot r = 184 k + i has arrival index ord_base + 4 (r >> 2) + (r & 3) = ord_base + r: the 4-ray layout's
    return qt_launch_sort_raster(c, ws, QS_SWEEP_SLOTS * n, hv, a.ord_base, 4ull, lds);
}

// what every sweep kernel reads of the context (match.hip fills its own with it too).  graph_k0: QS_SWEEP_NO_GRAPH, or the record of
// a graph-mode call these n records start at -- their slice of the batch that qs_sweep_graph_pass left
void qs_sweep_args(const qs_ctx *c, const unsigned char *d_pkts, size_t n, size_t stride, const unsigned short *d_lens, size_t graph_k0,
                   QsSweepArgs &a)
{
    a.pkts = d_pkts; a.n = n; a.stride = stride; a.lens = d_lens;
    a.ranges_off = stride == QS_SWEEP_SIZE_V0 ? 19u : 27u;
    a.max_agent = c->cfg.max_agent;
    a.offset = c->d_offset.p; a.drift = c->d_drift.p;
    a.smin = c->sweep_min; a.smax = c->sweep_max;
    a.accept = nullptr; a.pose = nullptr; a.ord_base = 0; a.corr = nullptr;
    a.g_accept = a.g_agent = nullptr; a.g_rx = a.g_ry = nullptr; a.zone = nullptr; a.veto = nullptr;
    if (graph_k0 != QS_SWEEP_NO_GRAPH) {
        a.g_accept = c->b.accept + graph_k0; a.g_agent = c->b.agent + graph_k0;
        a.g_rx = c->b.rx + graph_k0; a.g_ry = c->b.ry + graph_k0;
        a.zone = c->d_zone.p;
    }
}

// n records of one chunk; seq0 of record 0; outputs per record (accept [n], pose [n][3]), hit flags [184 n]; corr: the
// matched ingest's corrections of these records, nullptr for the plain ingest; veto: the guarded ingest's checks of them (never
// with corr or in graph mode), nullptr otherwise; graph_k0 as qs_sweep_args takes it; veil_k0 as qs_launch_sweeps_t takes it
static hipError_t qs_launch_sweeps(qs_ctx *c, const unsigned char *d_pkts, size_t n, size_t stride, const unsigned short *d_lens,
                                   uint64_t seq0, bool tiled, unsigned char *accept, double *pose, unsigned char *hit_valid,
                                   const qs_sweep_match *corr, const qs_sweep_check *veto, size_t graph_k0, size_t veil_k0)
{
    if (n == 0) return hipSuccess;
    QsSweepArgs a;
    qs_sweep_args(c, d_pkts, n, stride, d_lens, graph_k0, a);
    a.accept = accept; a.pose = pose;
    a.ord_base = qs_ord_base(c, seq0);
    a.corr = corr; a.veto = veto;
    if (veto) return qs_launch_sweeps_t<false, false, true>(c, a, n, tiled, hit_valid, veil_k0);
    if (a.g_accept)
        return corr ? qs_launch_sweeps_t<true, true>(c, a, n, tiled, hit_valid, veil_k0) : qs_launch_sweeps_t<false, true>(c, a, n, tiled, hit_valid, veil_k0);
    return corr ? qs_launch_sweeps_t<true, false>(c, a, n, tiled, hit_valid, veil_k0) : qs_launch_sweeps_t<false, false>(c, a, n, tiled, hit_valid, veil_k0);
}

// ---- C ABI: servo sweeps (semantics in include/quasar_slam.h) --------------------------------------------------------
// Records per chunk: the tiled raycast's ray slots (8 B) and tile records (up to 4 x 8 B) of one chunk, 184 slots per
// record, stay under 0.5 GiB; the host path stages one chunk's records at a time.
static const size_t QS_SWEEP_CHUNK = (size_t)1 << 16;

static int sweeps_begin(qs_ctx *c, size_t n, size_t stride, uint64_t &seq0)
{
    // the refusals first: a refused ingest leaves what the last ingest was, all of it (qs_last_sweeps and the four calls below)
    if (stride != QS_SWEEP_SIZE_V0 && stride != QS_SWEEP_SIZE_V0_ODO)
        return qs_fail(c, QS_E_INVAL, "qs_ingest_sweeps: stride must be 743 (v0) or 751 (v0 + odometry)");
    if (c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0)
        return qs_fail(c, QS_E_INVAL, "qs_ingest_sweeps: sharded contexts (seq_stride > 1, shard_bots > 0) do not take sweeps");
    c->last_matches = false; c->last_matches_n = 0;        // qs_last_sweep_matches: only after a matched ingest
    c->last_checks = false; c->last_checks_n = 0;          // qs_last_sweep_checks: only after a guarded ingest
    c->last_sweep_graph = false;                           // qs_last_sweep_nodes: only after an ingest in graph mode
    c->last_sveil = false;                                 // qs_last_sweeps_veiled: zeros unless the sweep veil acted
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

// records [k0, k0 + m) of the call, at d_pkts (already offset to record k0); graph: the call runs in graph mode
static int sweeps_chunk(qs_ctx *c, const uint8_t *d_pkts, size_t m, size_t stride, const uint16_t *d_lens, uint64_t seq0, size_t k0,
                        bool graph, const qs_sweep_match *corr, const qs_sweep_check *veto, bool veil)
{
    const uint64_t s0 = seq0 + (uint64_t)QS_SWEEP_SEQS * k0;
    int rc = ensure_epoch(c, s0, QS_SWEEP_SEQS * m);
    if (rc != QS_OK) return rc;
    // auto: by ray slots, as the 4-ray path decides by its 4 rays per packet
    // (S6: with the sweep veil acting always the tiled form -- the direct kernel writes the end cell before anything could veil it)
    const bool tiled = veil || c->cfg.raycast_mode == 2 || (c->cfg.raycast_mode == 0 && QS_SWEEP_SLOTS * m > 4 * (size_t)QS_DIRECT_MAX_BATCH);
    StageTimer t(c, QS_STAGE_RAYCAST);
    HIPCHK(c, qs_launch_sweeps(c, d_pkts, m, stride, d_lens, s0, tiled, c->sweep_acc.p + k0, c->sweep_pose.p + 3 * k0, c->sweep_hv.p,
                               corr, veto, graph ? k0 : QS_SWEEP_NO_GRAPH, veil ? k0 : QS_SWEEP_NO_VEIL));
    t.stop();
    c->dirty_since_fuse = true;
    return QS_OK;
}

// The four entry points' one routine.  host: pkts / lens are the caller's host buffers, staged one chunk at a time into the one
// staging block (stream-ordered: the previous chunk's kernels have read theirs), and the call ends by waiting for the GPU.
// matched: the matched ingest (semantics in include/quasar_slam.h, "sweep matching"; params as qs_match_setup takes them): every
// record of the call is matched against the map as it stands before the call (match.hip), then the records are mapped chunk by
// chunk from their corrected poses.
// checked: the guarded ingest ("sweep check"; cparams as qs_check_setup takes them; never together with matched): every record of the
// call is checked against the map as it stands before the call (check.hip), then the chunks are mapped by kernels that treat a
// contradicted record as a rejected one.
static int sweeps_ingest(qs_ctx *c, bool matched, const qs_match_params *params, bool checked, const qs_check_params *cparams,
                         const uint8_t *pkts, bool host, size_t n, size_t stride, const uint16_t *lens, uint64_t seq0)
{
    QsMatchSetup setup;
    QsCheckSetup csetup;
    const QsMatchSetup *ms = matched ? &setup : nullptr;
    const QsCheckSetup *cs = checked ? &csetup : nullptr;
    int rc = matched ? qs_match_setup(c, params, "qs_ingest_sweeps_matched", setup) : QS_OK;
    if (rc == QS_OK && checked) rc = qs_check_setup(c, cparams, "qs_ingest_sweeps_checked", csetup);
    if (rc != QS_OK) return rc;
    if (checked && c->sweep_graph)
        return qs_fail(c, QS_E_STATE, "qs_ingest_sweeps_checked: not in graph mode (a withheld sweep would still be a pose-graph node)");
    rc = sweeps_begin(c, n, stride, seq0);
    if (rc != QS_OK || n == 0) return rc;
    if (ms) HIPCHK(c, c->match_out.reserve(n, c->stream, 1024));
    if (cs) HIPCHK(c, c->check_out.reserve(n, c->stream, 1024));
    // bot veil, S0: the sweep stage acts only with the switch on and a radius; otherwise nothing of it is touched
    const bool veil = c->veil_sweeps && c->veil_radius > 0;
    if (veil) HIPCHK(c, qs_sweep_veil_reserve(c, std::min(n, QS_SWEEP_CHUNK), n));
    const bool pre = ms || cs;                             // a pass over the whole call before any of it is mapped
    if (pre) SYNCCHK(c);                                   // it reads the map: waiting edge beams go in first
    // Graph mode (qs_set_sweep_graph): before any chunk is mapped or matched, the pass over the whole call that decides every
    // record, adds the nodes and runs the chain (sweep_graph.hip; a host call stages every chunk for it once more).  Every later
    // launch of the call is then told which record of the call its records start at, and reads acceptance, agent and pose from
    // that slice of the batch -- the match starts from the chain's poses
    const bool graph = c->sweep_graph;
    if (graph) {
        rc = qs_sweep_graph_pass(c, pkts, host, n, stride, lens, QS_SWEEP_CHUNK);
        if (rc != QS_OK) return rc;
    }
    qs_sweep_match *corr = ms ? c->match_out.p : nullptr;
    qs_sweep_check *veto = cs ? c->check_out.p : nullptr;
    if (ms && !host) HIPCHK(c, qs_launch_match(c, *ms, pkts, n, stride, lens, corr, nullptr, graph ? 0 : QS_SWEEP_NO_GRAPH));
    if (cs && !host) HIPCHK(c, qs_launch_check(c, *cs, pkts, n, stride, lens, veto, nullptr));
    // host and matched or guarded: the staging block holds one chunk, so a call of several chunks stages each of them twice, first
    // (pass 0) to match or check them all against the map nobody has written yet, then (pass 1, the only one otherwise) to map them
    const bool one = n <= QS_SWEEP_CHUNK;
    for (int pass = (pre && host && !one) ? 0 : 1; pass < 2; pass++)
        for (size_t k0 = 0; k0 < n; k0 += QS_SWEEP_CHUNK) {
            const size_t m = std::min(QS_SWEEP_CHUNK, n - k0);
            const uint8_t *d_pkts = pkts + k0 * stride;
            const uint16_t *d_lens = lens ? lens + k0 : nullptr;
            if (host) {
                Staging s;
                rc = reserve_staging(c, m * stride, s);
                if (rc != QS_OK) return rc;
                HIPCHK(c, hipMemcpyAsync(s.pkts, d_pkts, m * stride, hipMemcpyHostToDevice, c->stream));
                if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, d_lens, m * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
                d_pkts = s.pkts; d_lens = lens ? s.lens : nullptr;
                if (ms && (pass == 0 || one))
                    HIPCHK(c, qs_launch_match(c, *ms, d_pkts, m, stride, d_lens, corr + k0, nullptr, graph ? k0 : QS_SWEEP_NO_GRAPH));
                if (cs && (pass == 0 || one)) HIPCHK(c, qs_launch_check(c, *cs, d_pkts, m, stride, d_lens, veto + k0, nullptr));
            }
            if (pass == 1) {
                rc = sweeps_chunk(c, d_pkts, m, stride, d_lens, seq0, k0, graph, ms ? corr + k0 : nullptr, cs ? veto + k0 : nullptr, veil);
                if (rc != QS_OK) return rc;
            }
        }
    c->last_sweep_graph = graph;
    if (c->b.edge) c->edge_maybe = true;                   // resolved at the next point the map is observed (sync_host_state)
    c->next_seq = seq0 + (uint64_t)QS_SWEEP_SEQS * n;
    c->last_sweeps = true; c->last_sweeps_n = n;
    c->last_sveil = veil;
    if (ms) { c->last_matches = true; c->last_matches_n = n; }
    if (cs) { c->last_checks = true; c->last_checks_n = n; }
    // host, as qs_ingest: the call waits for the GPU anyway, so the waiting edge beams are resolved now
    return host ? sync_host_state(c, true) : QS_OK;
}

extern "C" int qs_ingest_sweeps_device(qs_ctx *c, const uint8_t *d_pkts, size_t n, size_t stride, const uint16_t *d_lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || d_pkts != nullptr);
    return sweeps_ingest(c, false, nullptr, false, nullptr, d_pkts, false, n, stride, d_lens, seq0);
}

extern "C" int qs_ingest_sweeps(qs_ctx *c, const uint8_t *pkts, size_t n, size_t stride, const uint16_t *lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || pkts != nullptr);
    return sweeps_ingest(c, false, nullptr, false, nullptr, pkts, true, n, stride, lens, seq0);
}

extern "C" int qs_ingest_sweeps_matched_device(qs_ctx *c, const qs_match_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                               const uint16_t *d_lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || d_pkts != nullptr);
    return sweeps_ingest(c, true, params, false, nullptr, d_pkts, false, n, stride, d_lens, seq0);
}

extern "C" int qs_ingest_sweeps_matched(qs_ctx *c, const qs_match_params *params, const uint8_t *pkts, size_t n, size_t stride,
                                        const uint16_t *lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || pkts != nullptr);
    return sweeps_ingest(c, true, params, false, nullptr, pkts, true, n, stride, lens, seq0);
}

extern "C" int qs_ingest_sweeps_checked_device(qs_ctx *c, const qs_check_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                               const uint16_t *d_lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || d_pkts != nullptr);
    return sweeps_ingest(c, false, nullptr, true, params, d_pkts, false, n, stride, d_lens, seq0);
}

extern "C" int qs_ingest_sweeps_checked(qs_ctx *c, const qs_check_params *params, const uint8_t *pkts, size_t n, size_t stride,
                                        const uint16_t *lens, uint64_t seq0)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || pkts != nullptr);
    return sweeps_ingest(c, false, nullptr, true, params, pkts, true, n, stride, lens, seq0);
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
    SYNCCHK(c);                                            // waiting beams are resolved with the filter they were cast with
    c->sweep_min = smin; c->sweep_max = smax;
    return QS_OK;
}
