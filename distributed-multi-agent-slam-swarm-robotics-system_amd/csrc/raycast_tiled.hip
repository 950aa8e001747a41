// raycast_tiled.hip -- K1 (production form): tile-binned, LDS-staged raycast.
// Same semantics as raycast.hip (dual_bot_mapper.py:882-903, :136-179); different schedule.
//
// Why: the reference workloads revisit the same few hundred cells thousands of times per batch
// (two robots circling one room).  One global atomic per cell write then serialises on a few
// cache lines.  Here the cell writes of a batch are sorted by 64x64-cell grid tile, each
// workgroup rasters up to QT_CHUNK rays of ONE tile into an LDS copy of that tile (ds_max_u32 /
// ds_add_u32), and only the touched cells of the tile are merged into the HBM grid, one
// coalesced 256-byte row per wave-instruction.
//
// The sort is a counting sort with NO global atomics (measured: single-lane global atomics on a
// handful of hot lines cost ~6.5 ns each and dominated the first version, profiles/r01):
//   pass A  qs_rays_kernel      NWG persistent workgroups, one THREAD per packet: projection of
//                                the 4 rays (fp64 sincos), grid end points, zone / hit outputs,
//                                per-tile record counts in an LDS histogram, written as one row
//                                of the table T[wg][tile].  Rays longer than one tile (fine
//                                resolutions) are written to the grid directly.
//   pass B1 qs_table_scan_kernel per tile: exclusive scan of its column of T over the workgroups.
//   pass B2 (inside pass C)      exclusive scans over the tiles: record base and work-item base.
//   pass C  qs_scatter_kernel    same workgroup decomposition as A: LDS cursors (= table row +
//                                tile base) hand out record slots; one 16-byte record per
//                                overlapped tile (<= 2x2 per ray).
//   pass D  qs_raster_kernel     per work item (tile, <= QT_CHUNK records): LDS raster + merge.
//
// HBM traffic per packet (4 rays, ~1.4 tile records per ray): 45 B decoded fields + 64 B ray
// end points written and read + ~90 B records written and read, independent of how many cells
// each ray covers; the per-cell work happens in LDS.
#include "raycast_tiled.h"
#include "raycast_common.h"
#include <cstdlib>

// ---- pass A -----------------------------------------------------------------------------------
template <bool COUNTS>
__global__ void __launch_bounds__(QT_BIN_BLOCK)
qs_rays_kernel(size_t n, QsBatch b, QsGeom geo, QtWorkspace ws, unsigned int *__restrict__ stamps,
               unsigned long long *__restrict__ counts, unsigned long long ord_base, unsigned long long ord_stride,
               unsigned long long *__restrict__ zone, int max_agent, unsigned long long *__restrict__ counters)
{
    extern __shared__ unsigned int s_hist[];                       // [n_tiles]
    __shared__ double s_zone[QS_MAX_AGENT + 1][4];
    __shared__ unsigned int s_cnt[QS_TALLY_WORDS];
    const int tid = threadIdx.x;
    for (int t = tid; t < ws.n_tiles; t += QT_BIN_BLOCK) s_hist[t] = 0;
    for (int t = tid; t <= max_agent; t += QT_BIN_BLOCK) QS_ZONE_LDS_INIT(s_zone, t);
    qs_tally_init(s_cnt, tid);
    __syncthreads();

    // one THREAD per ray (4 per packet): small per-thread state, so twice the waves of a
    // thread-per-packet form fit a SIMD, and every store of the pass is a full coalesced row
    const size_t r0 = 4 * (size_t)blockIdx.x * ws.pk_per_wg;
    const size_t r1 = (r0 + 4 * ws.pk_per_wg < 4 * n) ? r0 + 4 * ws.pk_per_wg : 4 * n;
    QsTally my;
    // the inputs of the NEXT ray are requested before the current one is processed: a thread's rays
    // are 256 packets apart, so every iteration would otherwise start with a full HBM round trip
    unsigned char acc_n = 0, agent_n = 0;
    double rx_n = 0, ry_n = 0, yaw_n = 0;
    float df_n = 0;
    if (r0 + tid < r1) {
        const size_t r = r0 + tid, i = r >> 2;
        acc_n = b.map_ok[i]; agent_n = b.agent[i]; rx_n = b.rx[i]; ry_n = b.ry[i]; yaw_n = b.yaw[i];
        df_n = ((const float *)b.dist)[r];
    }
    for (size_t r = r0 + tid; r < r1; r += QT_BIN_BLOCK) {
        const size_t i = r >> 2;
        const int s = (int)(r & 3);
        const unsigned char acc = acc_n;
        const int agent = agent_n;
        const double rx = rx_n, ry = ry_n, yaw = yaw_n;
        const float df = df_n;
        if (r + QT_BIN_BLOCK < r1) {
            const size_t rn = r + QT_BIN_BLOCK, in = rn >> 2;
            acc_n = b.map_ok[in]; agent_n = b.agent[in]; rx_n = b.rx[in]; ry_n = b.ry[in]; yaw_n = b.yaw[in];
            df_n = ((const float *)b.dist)[rn];
        }
        uint2 rec = make_uint2((unsigned int)QT_NO_RAY & 0xffffu, 0u);
        bool valid = false;
        if (acc) {
            const QsRay ray = qs_project_ray(rx, ry, yaw, (double)df, s, geo);
            valid = ray.valid;
            // compute_bounding_box over hits U path (:702-706, :930-940): exact min/max, any order
            if (s == 0) qs_zone_point(s_zone, agent, rx, ry);                // paths[agent].append  :878-879
            if (valid) qs_zone_point(s_zone, agent, ray.ex, ray.ey);         // point_clouds[..].append  :892
            my.hits += valid ? 1u : 0u;
            my.rays++;
            rec = qt_ray_bin<COUNTS>(ray, rx, ry, yaw, df, qs_stamp_key(ord_base + ord_stride * i + s), -1, b, geo, ws, s_hist,
                                     stamps, counts, my.cells);
        }
        ws.rays[r] = rec;
        b.hit_valid[r] = valid ? 1 : 0;
    }
    qs_tally_fold(my, s_cnt);
    __syncthreads();
    unsigned int *row = ws.table + (size_t)blockIdx.x * ws.n_tiles;
    for (int t = tid; t < ws.n_tiles; t += QT_BIN_BLOCK) row[t] = s_hist[t];
    for (int t = tid; t <= max_agent; t += QT_BIN_BLOCK) qs_zone_commit(s_zone, t, zone);
    if (tid == 0) qs_tally_flush(s_cnt, counters);
}

// ---- pass B1: per tile, exclusive scan of its table column over the workgroups -------------------
// One 1024-thread workgroup per 64 tiles: thread (seg, t) owns rows [seg * R, (seg + 1) * R) of
// tile column t (R = ceil(nwg / 16) <= 32); a wave reads one 256-byte row segment per instruction
// and all R loads of a thread are in flight together, so the column costs one HBM round trip.  The 16
// segment sums of a column are combined through LDS and the running offsets written back.
#define QT_SCAN_TILES 64
#define QT_SCAN_SEGS 16
#define QT_SCAN_ROWS (QT_MAX_WG / QT_SCAN_SEGS)

__global__ void __launch_bounds__(QT_SCAN_TILES * QT_SCAN_SEGS)
qs_table_scan_kernel(QtWorkspace ws)
{
    __shared__ unsigned int s_part[QT_SCAN_SEGS][QT_SCAN_TILES];
    const int tid = threadIdx.x;
    const int lt = tid & (QT_SCAN_TILES - 1), seg = tid >> 6;
    const int t = blockIdx.x * QT_SCAN_TILES + lt;
    const int R = (ws.nwg + QT_SCAN_SEGS - 1) / QT_SCAN_SEGS;
    const int w0 = seg * R;
    const bool live = t < ws.n_tiles;
    unsigned int v[QT_SCAN_ROWS];
    unsigned int sum = 0;
    #pragma unroll
    for (int q = 0; q < QT_SCAN_ROWS; q++) {
        v[q] = (live && q < R && w0 + q < ws.nwg) ? ws.table[(size_t)(w0 + q) * ws.n_tiles + t] : 0u;
    }
    #pragma unroll
    for (int q = 0; q < QT_SCAN_ROWS; q++) sum += v[q];
    s_part[seg][lt] = sum;
    __syncthreads();
    unsigned int run = 0, total = 0;
    #pragma unroll
    for (int q = 0; q < QT_SCAN_SEGS; q++) { const unsigned int p = s_part[q][lt]; if (q < seg) run += p; total += p; }
    #pragma unroll
    for (int q = 0; q < QT_SCAN_ROWS; q++) {
        if (live && q < R && w0 + q < ws.nwg) ws.table[(size_t)(w0 + q) * ws.n_tiles + t] = run;
        run += v[q];
    }
    if (live && seg == 0) ws.tile_count[t] = total;
}

// ---- pass C: scatter tile records ---------------------------------------------------------------
__global__ void __launch_bounds__(QT_BIN_BLOCK)
qs_scatter_kernel(size_t n_rays, const unsigned char *__restrict__ hit_valid, QtWorkspace ws, int size,
                  unsigned long long ord_base, unsigned long long ord_stride)
{
    extern __shared__ unsigned int s_cur[];                        // [n_tiles] next record slot per tile
    __shared__ unsigned int s_wrec[QT_BIN_BLOCK / QS_WAVE], s_wchk[QT_BIN_BLOCK / QS_WAVE];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const unsigned int *row = ws.table + (size_t)blockIdx.x * ws.n_tiles;
    // pass B2, folded in: every workgroup scans the tile counts itself (16 KB of L2-resident reads, two
    // barriers) instead of waiting for a one-workgroup kernel in between: record base of every tile into
    // the LDS cursors; workgroup 0 also publishes record base and work-item base for the raster pass
    {
        const int per = (ws.n_tiles + QT_BIN_BLOCK - 1) / QT_BIN_BLOCK;
        const int lo = min(tid * per, ws.n_tiles), hi = min(lo + per, ws.n_tiles);
        unsigned int a = 0, c = 0;
        for (int t = lo; t < hi; t++) { const unsigned int v = ws.tile_count[t]; a += v; c += (v + QT_CHUNK - 1) / QT_CHUNK; }
        unsigned int ia = a, ic = c;                               // inclusive scan inside the wave
        #pragma unroll
        for (int off = 1; off < QS_WAVE; off <<= 1) {
            const unsigned int va = __shfl_up(ia, off), vc = __shfl_up(ic, off);
            if (lane >= off) { ia += va; ic += vc; }
        }
        if (lane == QS_WAVE - 1) { s_wrec[wave] = ia; s_wchk[wave] = ic; }
        __syncthreads();
        unsigned int ra = ia - a, rc = ic - c;
        for (int w = 0; w < wave; w++) { ra += s_wrec[w]; rc += s_wchk[w]; }
        const bool pub = blockIdx.x == 0;
        for (int t = lo; t < hi; t++) {
            const unsigned int v = ws.tile_count[t];
            s_cur[t] = ra + row[t];
            if (pub) { ws.tile_base[t] = ra; ws.chunk_base[t] = rc; }
            ra += v; rc += (v + QT_CHUNK - 1) / QT_CHUNK;
        }
        if (pub && tid == QT_BIN_BLOCK - 1) { ws.tile_base[ws.n_tiles] = ra; ws.chunk_base[ws.n_tiles] = rc; }
    }
    __syncthreads();
    const size_t r0 = (size_t)blockIdx.x * ws.rays_per_wg;
    const size_t r1 = (r0 + ws.rays_per_wg < n_rays) ? r0 + ws.rays_per_wg : n_rays;
    for (size_t r = r0 + tid; r < r1; r += QT_BIN_BLOCK) {
        const uint2 ray = ws.rays[r];
        const int x0 = (short)(ray.x & 0xffffu), y0 = (short)(ray.x >> 16);
        if (x0 == QT_NO_RAY) continue;
        const int x1 = (short)(ray.y & 0xffffu), y1 = (short)(ray.y >> 16);
        int tx_lo, tx_hi, ty_lo, ty_hi;
        qt_tile_range(x0, y0, x1, y1, size, tx_lo, tx_hi, ty_lo, ty_hi);
        // stamp of the ray's free cells; bit 0 (the occupied bit of a cell stamp) carries "the end
        // cell was observed" into the raster pass
        const unsigned int key = (unsigned int)((ord_base + ord_stride * (r >> 2) + (r & 3) + 1) << 1) | (hit_valid[r] ? 1u : 0u);
        // dx, dy < 64: the tile box is 1 x 1, 2 x 1, 1 x 2 or 2 x 2 (same enumeration as pass A)
        #pragma unroll
        for (int q = 0; q < 4; q++) {
            const int tx = tx_lo + (q & 1), ty = ty_lo + (q >> 1);
            if (tx > tx_hi || ty > ty_hi) continue;
            const unsigned int slot = atomicAdd(&s_cur[ty * ws.tiles_x + tx], 1u);
            const int ox = tx << QT_TILE_SHIFT, oy = ty << QT_TILE_SHIFT;   // tile origin: |coord - origin| < 128
            ws.recs[slot] = make_uint2(((unsigned int)(x0 - ox) & 0xffu) | (((unsigned int)(y0 - oy) & 0xffu) << 8) |
                                       (((unsigned int)(x1 - ox) & 0xffu) << 16) | ((unsigned int)(y1 - oy) << 24), key);
        }
    }
}

// ---- pass D: LDS raster + merge -------------------------------------------------------------------
// Persistent workgroups: workgroup w takes the contiguous run of work items [w * per, (w + 1) * per).
// Items are in tile order, so consecutive items mostly belong to the same tile (two robots in one
// room: ~300 items per tile); the LDS tile keeps accumulating across them and is merged into the HBM
// grid only when the tile changes.  Every merge of a shared tile is ~3000 device-scope atomics on
// the same few hundred cache lines as every other workgroup of that tile, so merging once per run
// instead of once per item takes most of that traffic away (and the empty workgroups of a
// one-item-per-workgroup launch with it).
#define QT_FLUSH_ITEMS 31                // 16-bit LDS counters: <= 31 * QT_CHUNK writes per cell between merges

template <bool COUNTS>
__device__ inline void qt_merge_tile(unsigned int *s_stamp, unsigned int *s_cnt, unsigned int *s_cells, int tid, int tile,
                                     bool exclusive, const QtWorkspace &ws, int size, unsigned int *__restrict__ stamps,
                                     unsigned long long *__restrict__ counts)
{
    // one 64-cell (256 B) grid row per wave-instruction.  A thread owns QT_CELLS / QT_BLOCK cells of
    // one column; all its grid loads are issued before the first store so an exclusive merge costs
    // one HBM round trip, not one per row.
    constexpr int PER = QT_CELLS / QT_BLOCK;
    constexpr int ROWS = QT_BLOCK / QT_TILE;              // rows covered by the workgroup per step
    const int tx0 = (tile % ws.tiles_x) << QT_TILE_SHIFT, ty0 = (tile / ws.tiles_x) << QT_TILE_SHIFT;
    const int mx = tid & (QT_TILE - 1), my = tid >> QT_TILE_SHIFT;
    // cells beyond the grid edge (partial tiles) are never written in LDS: v == 0 / kk == 0 there
    const size_t g0 = (size_t)(ty0 + my) * size + (tx0 + mx);
    const size_t gstep = (size_t)ROWS * size;
    unsigned int writes = 0;
    {   // stamps: cell-wise max  (:150 / :156 last writer wins)
        unsigned int v[PER], g[PER];
        #pragma unroll
        for (int q = 0; q < PER; q++) v[q] = s_stamp[(my + q * ROWS) * QT_PITCH + mx];
        if (ws.dirty) {
            // sparse fuse: a wave holds one 64-cell tile row per q = four blocks side by side; every cell written in LDS
            // has a stamp there, so the ballot of v != 0 is the row's written cells
            #pragma unroll
            for (int q = 0; q < PER; q++) {
                const unsigned long long wm = __builtin_amdgcn_ballot_w64(v[q] != 0);
                if (wm != 0 && (tid & (QS_WAVE - 1)) == 0) {
                    const unsigned int nib = ((wm & 0xffffull) ? 1u : 0u) | ((wm & 0xffff0000ull) ? 2u : 0u) |
                                             ((wm & 0xffff00000000ull) ? 4u : 0u) | ((wm >> 48) ? 8u : 0u);
                    const int gy = ty0 + my + q * ROWS;
                    unsigned int *w = ws.dirty + qs_dirty_word(tx0, gy, ws.dirty_pitch);
                    const unsigned int m = nib << ((tx0 / QS_DIRTY_BLOCK_W) & 31);   // tx0 is a multiple of 64: the nibble stays in one word
                    if ((__atomic_load_n(w, __ATOMIC_RELAXED) & m) != m) atomicOr(w, m);
                }
            }
        }
        if (exclusive) {
            #pragma unroll
            for (int q = 0; q < PER; q++) g[q] = v[q] != 0 ? stamps[g0 + q * gstep] : 0xffffffffu;
            #pragma unroll
            for (int q = 0; q < PER; q++) if (v[q] > g[q]) stamps[g0 + q * gstep] = v[q];
        } else {
            #pragma unroll
            for (int q = 0; q < PER; q++) if (v[q] != 0) atomicMax(&stamps[g0 + q * gstep], v[q]);
        }
    }
    if (COUNTS) {   // hit / miss counters: cell-wise sum
        unsigned int kk[PER];
        unsigned long long gc[PER];
        #pragma unroll
        for (int q = 0; q < PER; q++) {
            kk[q] = s_cnt[(my + q * ROWS) * QT_PITCH + mx];
            writes += (kk[q] >> 16) + (kk[q] & 0xffffu);
        }
        if (exclusive) {
            #pragma unroll
            for (int q = 0; q < PER; q++) gc[q] = kk[q] != 0 ? counts[g0 + q * gstep] : 0;
            #pragma unroll
            for (int q = 0; q < PER; q++)
                if (kk[q] != 0) counts[g0 + q * gstep] = gc[q] + (((unsigned long long)(kk[q] >> 16) << 32) | (kk[q] & 0xffffu));
        } else {
            #pragma unroll
            for (int q = 0; q < PER; q++)
                if (kk[q] != 0) atomicAdd(&counts[g0 + q * gstep], ((unsigned long long)(kk[q] >> 16) << 32) | (kk[q] & 0xffffu));
        }
        // cell writes (statistic): the LDS counters hold them
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) writes += __shfl_xor(writes, off);
        if ((tid & (QS_WAVE - 1)) == 0 && writes) atomicAdd(s_cells, writes);
    }
}

template <bool COUNTS>
__global__ void __launch_bounds__(QT_BLOCK, 8)
qs_raster_kernel(QtWorkspace ws, int size, unsigned int *__restrict__ stamps,
                 unsigned long long *__restrict__ counts, unsigned long long *__restrict__ counters)
{
    // + 64 scratch cells: a lane whose current cell is outside the tile (or whose walk has ended)
    // aims its two LDS atomics at its own scratch word instead of branching around them
    __shared__ unsigned int s_stamp[QT_LDS_CELLS + QS_WAVE];
    __shared__ unsigned int s_cnt[COUNTS ? QT_LDS_CELLS + QS_WAVE : 1];   // hi16 hits, lo16 misses
    __shared__ unsigned int s_cells;
    const int tid = threadIdx.x;
    const unsigned int n_items = ws.chunk_base[ws.n_tiles];
    const unsigned int per = (n_items + gridDim.x - 1) / gridDim.x;
    const unsigned int first = blockIdx.x * per;
    const unsigned int last = min(first + per, n_items);
    if (first >= last) return;
    if (tid == 0) s_cells = 0;
    // tile of the first work item: last t with chunk_base[t] <= first
    int tile;
    {
        int lo = 0, hi = ws.n_tiles;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ws.chunk_base[mid] <= first) lo = mid; else hi = mid; }
        tile = lo;
    }
    // Lane -> record mapping.  Records of a tile are in arrival order, so neighbouring records are the
    // four rays of one packet and the packets of the same bot a few centimetres apart: 64 consecutive
    // records walk nearly the same cells in lockstep and their LDS atomics serialise on the same
    // addresses.  Each wave therefore takes 8 groups of 8 consecutive records (two packets: 8
    // different rays), the groups QT_BLOCK / 8 records apart.
    const int lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const unsigned int slot = (unsigned int)((lane >> 3) * (QT_BLOCK / 8) + wave * 8 + (lane & 7));
    const int scratch4 = 4 * (QT_LDS_CELLS + lane);     // byte offset of this lane's scratch cell
    unsigned int wave_cells = 0;                        // wave-uniform count of cell writes (!COUNTS)
    int cur_tile = -1, since_flush = 0;

    for (unsigned int item = first; item < last; item++) {
        while (ws.chunk_base[tile + 1] <= item) tile++;          // tiles without records own no items
        if (tile != cur_tile || since_flush == QT_FLUSH_ITEMS) {
            if (cur_tile >= 0) {
                __syncthreads();
                const bool excl = ws.chunk_base[cur_tile] >= first && ws.chunk_base[cur_tile + 1] <= last;
                qt_merge_tile<COUNTS>(s_stamp, s_cnt, &s_cells, tid, cur_tile, excl, ws, size, stamps, counts);
                __syncthreads();
            }
            for (int c = tid; c < QT_LDS_CELLS / 4; c += QT_BLOCK) {
                ((uint4 *)s_stamp)[c] = make_uint4(0, 0, 0, 0);
                if (COUNTS) ((uint4 *)s_cnt)[c] = make_uint4(0, 0, 0, 0);
            }
            __syncthreads();
            cur_tile = tile; since_flush = 0;
        }
        since_flush++;
        const unsigned int rb = ws.tile_base[tile] + (item - ws.chunk_base[tile]) * QT_CHUNK;
        const unsigned int re = min(rb + QT_CHUNK, ws.tile_base[tile] + ws.tile_count[tile]);
        const int tx0 = (tile % ws.tiles_x) << QT_TILE_SHIFT, ty0 = (tile / ws.tiles_x) << QT_TILE_SHIFT;
        const int tw = min(QT_TILE, size - tx0), th = min(QT_TILE, size - ty0);
        const unsigned int tw4 = 4u * (unsigned int)tw, tha = 4u * QT_PITCH * (unsigned int)th;
        for (unsigned int j0 = rb; j0 < re; j0 += QT_BLOCK) {
            const unsigned int j = j0 + slot;
            // Walk state in major/minor form.  The walk of dual_bot_mapper.py:166-178 advances its
            // major axis in EVERY iteration and reaches (x1, y1) after exactly max(dx, dy) of them
            // (property-tested on the CPU: tests/, test_bresenham_major_axis_property), so with
            //   E = err (x-major, dx >= dy) or -err (y-major)
            // the pair of tests `e2 > -dy`, `e2 < dx` (:172-177) is ONE test per cell: the minor axis
            // steps iff 2 E < dmaj, i.e. E < (dmaj + 1) >> 1, and E += minor ? dmaj - dmin : -dmin.
            // The last cell (x1, y1) is the only one that can be marked occupied (:150): it is written
            // before the loop, and `x == x1 and y == y1` (:169) becomes a countdown over the
            // k = max(dx, dy) free cells.
            // x4 = 4 x and ya = 4 QT_PITCH y: the cell's LDS byte offset is their sum
            int x4 = 0, ya = 0, k = 0, E = 0, H = 0, incA = 0, incB = 0, sx_c = 0, sx_n = 0, sy_c = 0, sy_n = 0;
            unsigned int key_free = 0;
            bool wl = false;
            if (j < re) {
                const uint2 rec = ws.recs[j];
                const int x = (signed char)(rec.x & 0xffu), x1 = (signed char)((rec.x >> 16) & 0xffu);
                const int y1 = (signed char)(rec.x >> 24);
                const int y = (signed char)((rec.x >> 8) & 0xffu);
                key_free = rec.y & ~1u;
                const int dx = abs(x1 - x), dy = abs(y1 - y);                  // :161-162
                const int sx4 = x < x1 ? 4 : -4, sy = y < y1 ? 4 * QT_PITCH : -4 * QT_PITCH;   // :163-164, in bytes
                const bool xmaj = dx >= dy;
                const int dmaj = xmaj ? dx : dy, dmin = xmaj ? dy : dx;
                k = dmaj; E = dmaj - dmin; H = (dmaj + 1) >> 1; incA = dmaj - dmin; incB = -dmin;
                sx_c = sx4; sx_n = xmaj ? sx4 : 0; sy_c = sy; sy_n = xmaj ? 0 : sy;
                x4 = x << 2; ya = y * (4 * QT_PITCH);
                wl = (rec.y & 1u) && (unsigned int)x1 < (unsigned int)tw && (unsigned int)y1 < (unsigned int)th;
                if (wl) {                                                      // :148-150 occupied end cell
                    const int c = y1 * QT_PITCH + x1;
                    atomicMax(&s_stamp[c], key_free | 1u);
                    if (COUNTS) atomicAdd(&s_cnt[c], 0x10000u);
                }
            }
            if (!COUNTS) wave_cells += (unsigned int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(wl));
            for (int it = 0; __any(it < k); it++) {                            // :152-156 free cells
                const bool w = it < k && (unsigned int)x4 < tw4 && (unsigned int)ya < tha;
                const int a = w ? ya + x4 : scratch4;
                atomicMax((unsigned int *)((char *)s_stamp + a), key_free);
                if (COUNTS) atomicAdd((unsigned int *)((char *)s_cnt + a), 1u);
                if (!COUNTS) wave_cells += (unsigned int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(w));
                const bool minor = E < H;
                E += minor ? incA : incB;
                x4 += minor ? sx_c : sx_n;
                ya += minor ? sy_c : sy_n;
            }
        }
    }
    if (!COUNTS && lane == 0 && wave_cells) atomicAdd(&s_cells, wave_cells);
    __syncthreads();
    {
        const bool excl = ws.chunk_base[cur_tile] >= first && ws.chunk_base[cur_tile + 1] <= last;
        qt_merge_tile<COUNTS>(s_stamp, s_cnt, &s_cells, tid, cur_tile, excl, ws, size, stamps, counts);
    }
    __syncthreads();
    if (tid == 0 && s_cells) atomicAdd(&counters[QS_CNT_CELLS], (unsigned long long)s_cells);
}

// ---- host side ------------------------------------------------------------------------------------
static inline int qt_n_tiles(const qs_ctx *c)
{
    const int tiles_x = (c->cfg.size + QT_TILE - 1) / QT_TILE;
    return tiles_x * tiles_x;
}

bool qs_tiled_supported(const qs_ctx *c) { return qt_n_tiles(c) <= QT_MAX_TILES; }

// the workspace of up to cap_rays ray slots (4 per packet) over ws.n_tiles tiles, carved from base (nullptr: only the
// size); returns its bytes
static size_t qt_layout(void *base, size_t cap_rays, QtWorkspace &ws)
{
    const size_t n_pk = (cap_rays + 3) / 4, tiles = (size_t)ws.n_tiles;
    Carve k(base);
    ws.table = k.take<unsigned int>((size_t)QT_MAX_WG * tiles);
    ws.tile_count = k.take<unsigned int>(tiles + 1);
    ws.tile_base = k.take<unsigned int>(tiles + 1);
    ws.chunk_base = k.take<unsigned int>(tiles + 1);
    ws.rays = k.take<uint2>(4 * n_pk);
    ws.recs = k.take<uint2>(16 * n_pk);
    return k.bytes;
}

hipError_t qt_workspace(qs_ctx *c, size_t cap_rays, QtWorkspace &ws)
{
    ws.tiles_x = (c->cfg.size + QT_TILE - 1) / QT_TILE;
    ws.n_tiles = ws.tiles_x * ws.tiles_x;
    hipError_t e = c->bin_ws.reserve(qt_layout(nullptr, cap_rays, ws), c->stream);
    if (e != hipSuccess) return e;
    qt_layout(c->bin_ws.p, cap_rays, ws);
    ws.dirty = c->geom.dirty; ws.dirty_pitch = c->geom.dirty_pitch;
    return hipSuccess;
}

hipError_t qt_dyn_lds(const QtWorkspace &ws, const void *on, const void *off, size_t &lds)
{
    lds = (size_t)ws.n_tiles * sizeof(unsigned int);
    if (lds <= 32 * 1024) return hipSuccess;
    // large grids (up to 8192^2: 16384 tiles) need more dynamic LDS than the 64 KiB default allows
    // next to the static arrays; the CU has 160 KiB
    for (const void *k : {(const void *)qs_scatter_kernel, on, off}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t qt_launch_sort_raster(qs_ctx *c, const QtWorkspace &ws, size_t n_rays, const unsigned char *hit_valid,
                                 unsigned long long ord_base, unsigned long long ord_stride, size_t lds)
{
    // upper bound on raster work items: every record in a full chunk, plus one partial chunk per tile
    size_t max_items = (4 * n_rays) / QT_CHUNK + (size_t)ws.n_tiles + 8;
    if (max_items > 4 * n_rays) max_items = 4 * n_rays;
    StageTimer t_sort(c, QS_STAGE_RC_SORT);
    hipLaunchKernelGGL(qs_table_scan_kernel, dim3((ws.n_tiles + QT_SCAN_TILES - 1) / QT_SCAN_TILES),
                       dim3(QT_SCAN_TILES * QT_SCAN_SEGS), 0, c->stream, ws);
    hipLaunchKernelGGL(qs_scatter_kernel, dim3(ws.nwg), dim3(QT_BIN_BLOCK), lds, c->stream, n_rays, hit_valid, ws,
                       c->cfg.size, ord_base, ord_stride);
    t_sort.stop();
    // QS_RASTER_WGS (environment, read once): fewer persistent raster workgroups than the default -- a tuning
    // knob, and how the tests reach the long-run paths (tile changes inside a run, the 31-item flush)
    static const int env_wgs = [] { const char *e = getenv("QS_RASTER_WGS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : QT_RASTER_WGS; }();
    const unsigned int raster_wgs = (unsigned int)(max_items < (size_t)env_wgs ? max_items : (size_t)env_wgs);
    StageTimer t_raster(c, QS_STAGE_RC_RASTER);
    qs_launch_counts(c, qs_raster_kernel<true>, qs_raster_kernel<false>, dim3(raster_wgs), dim3(QT_BLOCK), 0, ws, c->cfg.size,
                     c->d_stamps.p, c->d_counts.p, c->d_counters.p);
    t_raster.stop();
    return hipGetLastError();
}

hipError_t qs_launch_raycast_tiled(qs_ctx *c, size_t n, uint64_t seq0)
{
    if (n == 0) return hipSuccess;
    if (!qs_tiled_supported(c)) return qs_launch_raycast_direct(c, n, seq0);
    QtWorkspace ws;
    hipError_t e = qt_workspace(c, 4 * c->cap_batch, ws);
    if (e != hipSuccess) return e;
    // packets per workgroup: a multiple of 64, at least 256, and at most QT_MAX_WG workgroups
    size_t per = (n + QT_MAX_WG - 1) / QT_MAX_WG;
    per = per < 256 ? 256 : ((per + 63) & ~(size_t)63);
    ws.pk_per_wg = per;
    ws.rays_per_wg = 4 * per;
    ws.nwg = (int)((n + per - 1) / per);

    const unsigned long long ord_base = qs_ord_base(c, seq0), ord_stride = qs_ord_stride(c);
    size_t lds = 0;
    e = qt_dyn_lds(ws, (const void *)qs_rays_kernel<true>, (const void *)qs_rays_kernel<false>, lds);
    if (e != hipSuccess) return e;
    StageTimer t_rays(c, QS_STAGE_RC_RAYS);
    qs_launch_counts(c, qs_rays_kernel<true>, qs_rays_kernel<false>, dim3(ws.nwg), dim3(QT_BIN_BLOCK), lds, n, c->b, c->geom, ws,
                     c->d_stamps.p, c->d_counts.p, ord_base, ord_stride, c->d_zone.p, c->cfg.max_agent, c->d_counters.p);
    t_rays.stop();
    const unsigned char *hit_valid = c->b.hit_valid;
    if (c->veil_radius > 0) {                        // bot veil: passes C and D read hit_valid & !veiled instead
        e = qs_launch_veil(c, ws.rays, n, &hit_valid);
        if (e != hipSuccess) return e;
    }
    return qt_launch_sort_raster(c, ws, 4 * n, hit_valid, ord_base, ord_stride, lds);
}
