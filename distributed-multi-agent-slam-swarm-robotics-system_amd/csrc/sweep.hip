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
// A sweep adds no pose-graph node, landmark, EKF step or zone point: those belong to the 42 / 41-byte path.
#include <math.h>
#include <algorithm>

#include "raycast_tiled.h"
#include "raycast_common.h"

#define SW_DW 192                 // LDS dwords per staged record: >= (3 + 751 + 3) / 4 + 1 (the alignbyte reads one dword ahead)
#define SW_DIRECT_BLOCK 256       // direct kernel: 4 records per workgroup
#define SW_MAGIC 0x4c525351u      // 'Q','S','R','L'

struct QsSweepArgs {
    const unsigned char *pkts;    // record k at pkts + k * stride (this chunk)
    size_t n, stride;
    const unsigned short *lens;   // [n] or nullptr (every length == stride)
    unsigned int ranges_off;      // byte offset of r_0: 19 (v0) or 27 (v0 + odometry)
    int max_agent;
    const double *offset, *drift; // [max_agent + 1], [max_agent + 1][2]: read on the device, after every earlier launch
    double smin, smax;            // trust filter: smin < d <= smax
    unsigned char *accept;        // [n] out
    double *pose;                 // [n][3] out: rx, ry, yaw of accepted records
    unsigned long long ord_base;  // 4 * (seq0 - epoch_base) of record 0
};

// the record's dwords [addr & ~3, addr + stride) into s[0 .. 191]; dwords that reach outside the caller's buffer (its first and
// last bytes need not be dword-aligned) are read bytewise
__device__ inline void sw_stage(const QsSweepArgs &a, size_t k, unsigned int *s, int lane)
{
    const unsigned long long base = (unsigned long long)a.pkts, end = base + a.n * a.stride;
    const unsigned long long addr0 = base + k * a.stride, w0 = addr0 & ~3ull;
    unsigned int v[3];
    #pragma unroll
    for (int q = 0; q < 3; q++) {
        const unsigned long long p = w0 + 4ull * (unsigned long long)(lane + QS_WAVE * q);
        v[q] = 0;
        if (k < a.n && p < addr0 + a.stride) {
            if (p >= base && p + 4 <= end) v[q] = *(const unsigned int *)p;
            else
                for (int j = 0; j < 4; j++)
                    if (p + j >= base && p + j < end) v[q] |= (unsigned int)*(const unsigned char *)(p + j) << (8 * j);
        }
    }
    #pragma unroll
    for (int q = 0; q < 3; q++) s[lane + QS_WAVE * q] = v[q];
}

// little-endian u32 at byte o of the staged record (mis = the record's start within its first dword)
__device__ inline unsigned int sw_u32(const unsigned int *s, unsigned int mis, unsigned int o)
{
    const unsigned int b = mis + o;
    return __builtin_amdgcn_alignbyte(s[(b >> 2) + 1], s[b >> 2], b & 3u);
}

struct SwHead { bool ok; double rx, ry, yaw; };

__device__ inline SwHead sw_head(const QsSweepArgs &a, size_t k, const unsigned int *s, unsigned int mis)
{
    SwHead h{false, 0.0, 0.0, 0.0};
    const int len = a.lens ? (int)a.lens[k] : (int)a.stride;
    const int agent = (int)(sw_u32(s, mis, 4) & 0xffu);
    h.ok = len == (int)a.stride && sw_u32(s, mis, 0) == SW_MAGIC && agent >= 1 && agent <= a.max_agent;
    if (h.ok) {
        const float x = __uint_as_float(sw_u32(s, mis, 5)), y = __uint_as_float(sw_u32(s, mis, 9));
        h.rx = ((double)x + a.offset[agent]) + a.drift[2 * agent];      // offset first, then drift (:851-857)
        h.ry = (double)y + a.drift[2 * agent + 1];
        h.yaw = (double)__uint_as_float(sw_u32(s, mis, 13));
    }
    return h;
}

// beam i: angle ryaw + math.radians(i - 90) -- CPython's radians is x * (pi / 180), one multiply and one add (no FMA: the
// library is built with -ffp-contract=off); hit and free-ray rule as qs_project_ray's (A6): NaN, 0 and negative ranges give
// a full-length free ray
__device__ inline QsRay sw_beam(const SwHead &h, int i, double d, double smin, double smax)
{
    const double kRad = 3.141592653589793 / 180.0;
    const double a = h.yaw + (double)(i - 90) * kRad;
    QsRay r;
    r.valid = (smin < d) && (d <= smax);
    const double range = r.valid ? d : ((d > smin) ? ((smax < d) ? smax : d) : smax);
    double sa, ca;
    qs_sincos(a, &sa, &ca);
    r.ex = h.rx + range * ca;
    r.ey = h.ry + range * sa;
    return r;
}

__device__ inline void sw_out(const QsSweepArgs &a, size_t k, const SwHead &h)
{
    a.accept[k] = h.ok ? 1 : 0;
    if (h.ok) { a.pose[3 * k] = h.rx; a.pose[3 * k + 1] = h.ry; a.pose[3 * k + 2] = h.yaw; }
}

// ---- pass A of the tiled raycast -----------------------------------------------------------------------------------------
// Workgroup w owns records [w * pk_per_wg, (w + 1) * pk_per_wg) (pk_per_wg a multiple of 16), its 16 waves one record each per
// round, and writes ray slots [184 * that range) plus its row of the tile table.
template <bool COUNTS>
__global__ void __launch_bounds__(QT_BIN_BLOCK)
qs_sweep_rays_kernel(QsSweepArgs a, QsBatch b, QsGeom geo, QtWorkspace ws, unsigned char *__restrict__ hit_valid,
                     unsigned int *__restrict__ stamps, unsigned long long *__restrict__ counts,
                     unsigned long long *__restrict__ counters)
{
    constexpr int NW = QT_BIN_BLOCK / QS_WAVE;
    extern __shared__ unsigned int s_hist[];                       // [n_tiles]
    __shared__ unsigned int s_rec[NW][SW_DW];
    __shared__ unsigned int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    for (int t = tid; t < ws.n_tiles; t += QT_BIN_BLOCK) s_hist[t] = 0;
    if (tid < 4) s_cnt[tid] = 0;
    const size_t k0 = (size_t)blockIdx.x * ws.pk_per_wg;
    const size_t k1 = (k0 + ws.pk_per_wg < a.n) ? k0 + ws.pk_per_wg : a.n;
    unsigned int my_cells = 0, my_rays = 0, my_hits = 0, my_acc = 0;
    for (size_t kb = k0; kb < k1; kb += NW) {                     // (uniform over the workgroup)
        const size_t k = kb + wave;
        __syncthreads();                                           // the previous round's records are parsed
        sw_stage(a, k < k1 ? k : a.n, s_rec[wave], lane);
        __syncthreads();
        if (k >= k1) continue;
        const unsigned int *s = s_rec[wave];
        const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
        const SwHead h = sw_head(a, k, s, mis);
        if (lane == 0) { sw_out(a, k, h); my_acc += h.ok ? 1u : 0u; }
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
                my_hits += valid ? 1u : 0u;
                my_rays++;
                const unsigned int key_free = (unsigned int)((a.ord_base + r + 1) << 1);
                QsLine ln;
                if (b.edge && qs_edge_ray(ray, geo) && qs_edge_defer(b, h.rx, h.ry, h.yaw, df, key_free, i)) {
                    // the host decides this beam's cells (qs_api.hip: sync_host_state)
                } else if (qs_line_setup(ray, h.rx, h.ry, geo, ln)) {
                    if (ln.dx < QT_TILE && ln.dy < QT_TILE) {
                        int tx_lo, tx_hi, ty_lo, ty_hi;
                        qt_tile_range(ln.x0, ln.y0, ln.x1, ln.y1, geo.size, tx_lo, tx_hi, ty_lo, ty_hi);
                        const int t00 = ty_lo * ws.tiles_x + tx_lo;
                        const bool wx = tx_hi > tx_lo, wy = ty_hi > ty_lo;
                        atomicAdd(&s_hist[t00], 1u);
                        if (wx) atomicAdd(&s_hist[t00 + 1], 1u);
                        if (wy) atomicAdd(&s_hist[t00 + ws.tiles_x], 1u);
                        if (wx && wy) atomicAdd(&s_hist[t00 + ws.tiles_x + 1], 1u);
                        rec = make_uint2(((unsigned int)ln.x0 & 0xffffu) | ((unsigned int)ln.y0 << 16),
                                         ((unsigned int)ln.x1 & 0xffffu) | ((unsigned int)ln.y1 << 16));
                    } else {
                        my_cells += qs_cast_line<COUNTS>(ln, valid, key_free, geo, stamps, counts);   // long ray (fine resolution)
                    }
                }
            }
            ws.rays[r] = rec;
            hit_valid[r] = valid ? 1 : 0;
        }
    }
    if (my_rays) atomicAdd(&s_cnt[0], my_rays);
    if (my_cells) atomicAdd(&s_cnt[1], my_cells);
    if (my_hits) atomicAdd(&s_cnt[2], my_hits);
    if (my_acc) atomicAdd(&s_cnt[3], my_acc);
    __syncthreads();
    unsigned int *row = ws.table + (size_t)blockIdx.x * ws.n_tiles;
    for (int t = tid; t < ws.n_tiles; t += QT_BIN_BLOCK) row[t] = s_hist[t];
    if (tid == 0) {
        atomicAdd(&counters[QS_CNT_DATAGRAMS], (unsigned long long)(k1 - k0));
        if (s_cnt[3]) atomicAdd(&counters[QS_CNT_ACCEPTED], (unsigned long long)s_cnt[3]);
        if (s_cnt[0]) atomicAdd(&counters[QS_CNT_RAYS], (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&counters[QS_CNT_CELLS], (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&counters[QS_CNT_HITS], (unsigned long long)s_cnt[2]);
    }
}

// ---- direct form: one wave per record, every cell one global atomic --------------------------------------------------------
template <bool COUNTS>
__global__ void __launch_bounds__(SW_DIRECT_BLOCK)
qs_sweep_direct_kernel(QsSweepArgs a, QsBatch b, QsGeom geo, unsigned int *__restrict__ stamps,
                       unsigned long long *__restrict__ counts, unsigned long long *__restrict__ counters)
{
    constexpr int NW = SW_DIRECT_BLOCK / QS_WAVE;
    __shared__ unsigned int s_rec[NW][SW_DW];
    __shared__ unsigned int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    if (tid < 4) s_cnt[tid] = 0;
    const size_t k = (size_t)blockIdx.x * NW + wave;
    sw_stage(a, k, s_rec[wave], lane);
    __syncthreads();
    unsigned int my_cells = 0, my_rays = 0, my_hits = 0;
    if (k < a.n) {
        const unsigned int *s = s_rec[wave];
        const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
        const SwHead h = sw_head(a, k, s, mis);
        if (lane == 0) { sw_out(a, k, h); if (h.ok) atomicAdd(&s_cnt[3], 1u); }
        if (h.ok) {
            #pragma unroll
            for (int q = 0; q < 3; q++) {
                const int i = lane + QS_WAVE * q;
                if (i >= QS_SWEEP_BEAMS) break;
                const float df = __uint_as_float(sw_u32(s, mis, a.ranges_off + 4u * (unsigned int)i));
                const QsRay ray = sw_beam(h, i, (double)df, a.smin, a.smax);
                my_hits += ray.valid ? 1u : 0u;
                my_rays++;
                const unsigned int key_free = (unsigned int)((a.ord_base + QS_SWEEP_SLOTS * k + i + 1) << 1);
                QsLine ln;
                if (b.edge && qs_edge_ray(ray, geo) && qs_edge_defer(b, h.rx, h.ry, h.yaw, df, key_free, i)) {
                    // the host decides this beam's cells (qs_api.hip: sync_host_state)
                } else if (qs_line_setup(ray, h.rx, h.ry, geo, ln)) {
                    my_cells += qs_cast_line<COUNTS>(ln, ray.valid, key_free, geo, stamps, counts);
                }
            }
        }
    }
    if (my_rays) atomicAdd(&s_cnt[0], my_rays);
    if (my_cells) atomicAdd(&s_cnt[1], my_cells);
    if (my_hits) atomicAdd(&s_cnt[2], my_hits);
    __syncthreads();
    if (tid == 0) {
        const size_t k0 = (size_t)blockIdx.x * NW;
        atomicAdd(&counters[QS_CNT_DATAGRAMS], (unsigned long long)(a.n - k0 < (size_t)NW ? a.n - k0 : (size_t)NW));
        if (s_cnt[3]) atomicAdd(&counters[QS_CNT_ACCEPTED], (unsigned long long)s_cnt[3]);
        if (s_cnt[0]) atomicAdd(&counters[QS_CNT_RAYS], (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&counters[QS_CNT_CELLS], (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&counters[QS_CNT_HITS], (unsigned long long)s_cnt[2]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// n records of one chunk; seq0 of record 0; outputs per record (accept [n], pose [n][3]), hit flags [184 n]
static hipError_t qs_launch_sweeps(qs_ctx *c, const unsigned char *d_pkts, size_t n, size_t stride, const unsigned short *d_lens,
                                   uint64_t seq0, bool tiled, unsigned char *accept, double *pose, unsigned char *hit_valid)
{
    if (n == 0) return hipSuccess;
    QsSweepArgs a;
    a.pkts = d_pkts; a.n = n; a.stride = stride; a.lens = d_lens;
    a.ranges_off = stride == QS_SWEEP_SIZE_V0 ? 19u : 27u;
    a.max_agent = c->cfg.max_agent;
    a.offset = c->d_offset.p; a.drift = c->d_drift.p;
    a.smin = c->sweep_min; a.smax = c->sweep_max;
    a.accept = accept; a.pose = pose;
    a.ord_base = 4ull * (seq0 - c->epoch_base);
    if (!tiled || !qs_tiled_supported(c)) {
        const unsigned int blocks = (unsigned int)((n + SW_DIRECT_BLOCK / QS_WAVE - 1) / (SW_DIRECT_BLOCK / QS_WAVE));
        if (c->cfg.enable_counts)
            hipLaunchKernelGGL(qs_sweep_direct_kernel<true>, dim3(blocks), dim3(SW_DIRECT_BLOCK), 0, c->stream, a, c->b, c->geom,
                               c->d_stamps.p, c->d_counts.p, c->d_counters.p);
        else
            hipLaunchKernelGGL(qs_sweep_direct_kernel<false>, dim3(blocks), dim3(SW_DIRECT_BLOCK), 0, c->stream, a, c->b, c->geom,
                               c->d_stamps.p, c->d_counts.p, c->d_counters.p);
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
    const void *pass_a[2] = {(const void *)qs_sweep_rays_kernel<true>, (const void *)qs_sweep_rays_kernel<false>};
    size_t lds = 0;
    e = qt_dyn_lds(ws, pass_a, 2, lds);
    if (e != hipSuccess) return e;
    StageTimer t_rays(c, QS_STAGE_RC_RAYS);
    if (c->cfg.enable_counts)
        hipLaunchKernelGGL(qs_sweep_rays_kernel<true>, dim3(ws.nwg), dim3(QT_BIN_BLOCK), lds, c->stream, a, c->b, c->geom, ws,
                           hit_valid, c->d_stamps.p, c->d_counts.p, c->d_counters.p);
    else
        hipLaunchKernelGGL(qs_sweep_rays_kernel<false>, dim3(ws.nwg), dim3(QT_BIN_BLOCK), lds, c->stream, a, c->b, c->geom, ws,
                           hit_valid, c->d_stamps.p, c->d_counts.p, c->d_counters.p);
    t_rays.stop();
    // slot r = 184 k + i has stamp ordinal ord_base + 4 (r >> 2) + (r & 3) + 1 = ord_base + r + 1: the 4-ray layout's
    return qt_launch_sort_raster(c, ws, QS_SWEEP_SLOTS * n, hit_valid, a.ord_base, 4ull, lds);
}

// ---- C ABI: servo sweeps (semantics in include/quasar_slam.h) --------------------------------------------------------
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
    if (c->b.edge) c->edge_maybe = true;                   // resolved at the next point the map is observed (sync_host_state)
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
    return sync_host_state(c, true);
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
