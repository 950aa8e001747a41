// veil.hip -- the bot veil (include/quasar_slam.h, rules V1-V7): a packet beam that ends on another bot of the swarm is cast
// as a free ray without its end cell.  A stage of the tiled raycast between pass A and the sort (raycast_tiled.hip): pass A
// has written every ray's absolute end cells (QtWorkspace::rays) and its hit flag; passes C and D read the hit flag only
// through the pointer handed to qt_launch_sort_raster, and a ray whose flag is 0 is cast FREE up to its end cell.  The stage
// writes a second flag array (hit_valid & !veiled) and hands that on; QsBatch::hit_valid stays what the filter judged.
//
// "Where was bot b last heard before packet i" is a question in arrival order over the whole call.  It is answered per
// block of QV_BLOCK packets:
//   qs_veil_cells_kernel  one thread per packet: its cell (V1), packed i16 x 2; per block and bot the block-local index + 1
//                         of the bot's last packet with a cell (an LDS max per packet, one row write per block)
//   qs_veil_scan_kernel   one wave per bot: "latest cell" carried over the blocks (64 blocks per step, a wave scan), seeded
//                         from the context's table; the cell known at every block's entry; the final value back into the
//                         table (V6)
//   qs_veil_mark_kernel   one workgroup per block: thread p looks at every earlier packet q of its block (q speaks for its
//                         bot iff the bot has no packet in (q, p)) and at the entry row for the bots without a packet before
//                         p; all of these are wave-uniform LDS reads (broadcast, no bank conflicts)
// No global atomics but the one statistics word (one per workgroup that veiled anything), no wait for host or device.
#include "raycast_tiled.h"
#include <cstring>
#include <vector>

#define QV_BLOCK 256                      // packets per block = threads of every workgroup here (bots are 1..255: one thread per bot)
#define QV_NONE 0x00008000u               // packed cell "none": x = -32768
#define QV_CLAMP_LO (-16384)              // cells are packed after clamping: the end cell of a binned ray lies within 64 cells of
#define QV_CLAMP_HI 24576                 //   a grid of at most 8192 cells, so a clamped coordinate is > 8000 cells from every one

struct QvWorkspace {
    unsigned int *cell;                   // [n] packed cell of an accepted packet that has one, QV_NONE otherwise
    unsigned short *blk_last;             // [blocks][QV_BLOCK] per bot: block-local index + 1 of its last packet with a cell, 0 = none
    unsigned int *blk_in;                 // [blocks][QV_BLOCK] per bot: the packed cell known when the block begins
    unsigned char *veiled;                // [4 n] the flags qs_last_veiled reads
    unsigned char *hit;                   // [4 n] hit_valid & !veiled: what passes C and D see
};

__host__ __device__ inline unsigned int qv_pack(int x, int y)
{
    x = x < QV_CLAMP_LO ? QV_CLAMP_LO : (x > QV_CLAMP_HI ? QV_CLAMP_HI : x);
    y = y < QV_CLAMP_LO ? QV_CLAMP_LO : (y > QV_CLAMP_HI ? QV_CLAMP_HI : y);
    return ((unsigned int)x & 0xffffu) | ((unsigned int)y << 16);
}
__device__ inline bool qv_none(unsigned int v) { return (v & 0xffffu) == QV_NONE; }

// V1: world_to_grid on both axes; none for a pose that is not finite or whose cell lies beyond +-2^30
__device__ inline bool qv_cell(double rx, double ry, const QsGeom &geo, int &x, int &y)
{
    if (!qs_w2g_i32(rx, geo.ox, geo, x) || !qs_w2g_i32(ry, geo.oy, geo, y)) return false;
    return x > -QS_CELL_CLAMP && x < QS_CELL_CLAMP && y > -QS_CELL_CLAMP && y < QS_CELL_CLAMP;
}

__global__ void __launch_bounds__(QV_BLOCK)
qs_veil_cells_kernel(size_t n, QsBatch b, QsGeom geo, QvWorkspace vw)
{
    __shared__ unsigned int s_last[QV_BLOCK];
    const int tid = threadIdx.x;
    s_last[tid] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * QV_BLOCK + tid;
    unsigned int cell = QV_NONE;
    if (i < n && b.accept[i]) {                                    // V3: accept decides (this context is not a shard)
        int x, y;
        if (qv_cell(b.rx[i], b.ry[i], geo, x, y)) {
            cell = qv_pack(x, y);
            atomicMax(&s_last[b.agent[i]], (unsigned int)tid + 1u);
        }
    }
    if (i < n) vw.cell[i] = cell;
    __syncthreads();
    vw.blk_last[(size_t)blockIdx.x * QV_BLOCK + tid] = (unsigned short)s_last[tid];
}

__global__ void __launch_bounds__(QV_BLOCK)
qs_veil_scan_kernel(int n_blocks, QsBatch b, QsGeom geo, QvWorkspace vw, int4 *__restrict__ tab, int max_agent)
{
    const int lane = threadIdx.x & (QS_WAVE - 1);
    const int bot = 1 + blockIdx.x * (QV_BLOCK / QS_WAVE) + (threadIdx.x >> 6);
    if (bot > max_agent) return;                                   // (wave-uniform)
    const int4 t = tab[bot];
    unsigned int carry = t.z ? qv_pack(t.x, t.y) : QV_NONE;
    long long last_i = -1;                                         // the bot's last packet with a cell in this call
    for (int b0 = 0; b0 < n_blocks; b0 += QS_WAVE) {
        const int blk = b0 + lane;
        unsigned int v = QV_NONE;
        long long mine = -1;
        if (blk < n_blocks) {
            const unsigned int l = vw.blk_last[(size_t)blk * QV_BLOCK + bot];
            if (l) { mine = (long long)blk * QV_BLOCK + (l - 1); v = vw.cell[mine]; }
        }
        // inclusive scan of "the latest cell" over the 64 blocks (a (+) b = b unless b is none), the carry entering at lane 0
        unsigned int inc = (lane == 0 && qv_none(v)) ? carry : v;
        #pragma unroll
        for (int off = 1; off < QS_WAVE; off <<= 1) {
            const unsigned int u = __shfl_up(inc, off);
            if (lane >= off && qv_none(inc)) inc = u;
        }
        const unsigned int prev = __shfl_up(inc, 1);
        if (blk < n_blocks) vw.blk_in[(size_t)blk * QV_BLOCK + bot] = lane == 0 ? carry : prev;
        carry = __shfl(inc, QS_WAVE - 1);
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const long long o = __shfl_xor(mine, off); mine = o > mine ? o : mine; }
        if (mine >= 0) last_i = mine;
    }
    if (lane == 0 && last_i >= 0) {                                // V6, from the pose itself: the table holds unclamped cells
        int x = 0, y = 0;
        qv_cell(b.rx[last_i], b.ry[last_i], geo, x, y);
        tab[bot] = make_int4(x, y, 1, 0);
    }
}

__global__ void __launch_bounds__(QV_BLOCK)
qs_veil_mark_kernel(size_t n, QsBatch b, const uint2 *__restrict__ rays, QvWorkspace vw, int size, int radius, int max_agent,
                    unsigned long long *__restrict__ total)
{
    __shared__ unsigned int s_cell[QV_BLOCK];      // packed cell of packet q
    __shared__ unsigned int s_meta[QV_BLOCK];      // agent of packet q (0: it does not count) | index of the agent's next packet << 8
    __shared__ unsigned int s_next[QV_BLOCK];
    __shared__ unsigned int s_in[QV_BLOCK];        // per bot: the cell known at the block's entry
    __shared__ unsigned int s_lim[QV_BLOCK];       // per bot: 1 + index of its first packet in the block (QV_BLOCK + 1: none); 0 = no entry cell
    __shared__ unsigned int s_tally;
    const int tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * QV_BLOCK + tid;
    const unsigned int cell = i < n ? vw.cell[i] : QV_NONE;
    const int agent = qv_none(cell) ? 0 : (int)b.agent[i];          // (a packet without a cell is not accepted or has no binned ray)
    s_cell[tid] = cell;
    s_meta[tid] = (unsigned int)agent;
    if (tid == 0) s_tally = 0;
    __syncthreads();
    {   // thread = bot: the chain of its packets, from the back
        unsigned int last = QV_BLOCK;
        if (tid >= 1 && tid <= max_agent)
            for (int q = QV_BLOCK - 1; q >= 0; q--)
                if (s_meta[q] == (unsigned int)tid) { s_next[q] = last; last = (unsigned int)q; }
        const unsigned int in = (tid >= 1 && tid <= max_agent) ? vw.blk_in[(size_t)blockIdx.x * QV_BLOCK + tid] : QV_NONE;
        s_in[tid] = in;
        s_lim[tid] = qv_none(in) ? 0u : last + 1u;
    }
    __syncthreads();
    if (agent) s_meta[tid] = (unsigned int)agent | (s_next[tid] << 8);
    __syncthreads();

    // this packet's rays: V4's first two conditions, and an end cell inside the grid
    int ex[4], ey[4];
    unsigned int elig = 0, hv = 0;
    if (i < n) hv = *(const unsigned int *)(b.hit_valid + 4 * i);
    if (agent && hv) {
        const uint4 r01 = ((const uint4 *)(rays + 4 * i))[0], r23 = ((const uint4 *)(rays + 4 * i))[1];
        const unsigned int rx0[4] = {r01.x, r01.z, r23.x, r23.z}, rx1[4] = {r01.y, r01.w, r23.y, r23.w};
        #pragma unroll
        for (int s = 0; s < 4; s++) {
            ex[s] = (short)(rx1[s] & 0xffffu); ey[s] = (short)(rx1[s] >> 16);
            const bool binned = (short)(rx0[s] & 0xffffu) != QT_NO_RAY;
            if (((hv >> (8 * s)) & 0xffu) && binned && (unsigned int)ex[s] < (unsigned int)size && (unsigned int)ey[s] < (unsigned int)size)
                elig |= 1u << s;
        }
    }
    const int px = (short)(cell & 0xffffu), py = (short)(cell >> 16);
    const int lim = QT_TILE + radius, r2 = radius * radius;        // a binned ray ends less than 64 cells from its pose on each axis
    unsigned int veil = 0;
    auto test = [&](unsigned int c) {
        const int bx = (short)(c & 0xffffu), by = (short)(c >> 16);
        if (abs(bx - px) > lim || abs(by - py) > lim) return;
        #pragma unroll
        for (int s = 0; s < 4; s++) {
            const int dx = ex[s] - bx, dy = ey[s] - by;
            if (((elig >> s) & 1u) && dx * dx + dy * dy <= r2) veil |= 1u << s;
        }
    };
    if (elig) {
        for (int q = 0; q < tid; q++) {                            // V3: the bots heard earlier in this block
            const unsigned int m = s_meta[q];
            const int a = (int)(m & 0xffu);
            if (a != 0 && a != agent && (m >> 8) >= (unsigned int)tid) test(s_cell[q]);
        }
        for (int a = 1; a <= max_agent; a++)                       // ... and those heard before it
            if (a != agent && s_lim[a] > (unsigned int)tid) test(s_in[a]);
    }
    if (i < n) {
        unsigned int vb = 0;
        #pragma unroll
        for (int s = 0; s < 4; s++) vb |= ((veil >> s) & 1u) << (8 * s);
        *(unsigned int *)(vw.veiled + 4 * i) = vb;
        *(unsigned int *)(vw.hit + 4 * i) = hv & ~(vb * 0xffu);    // V5
    }
    unsigned int cnt = (unsigned int)__builtin_popcount(veil);
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((tid & (QS_WAVE - 1)) == 0 && cnt) atomicAdd(&s_tally, cnt);
    __syncthreads();
    if (tid == 0 && s_tally) atomicAdd(total, (unsigned long long)s_tally);
}

// cell[bot] = (x, y), or unknown; bot 0: every bot forgotten (the kernel's arguments travel by value: nothing for the host to keep)
__global__ void qs_veil_table_kernel(int4 *tab, int bot, int x, int y, int known)
{
    if (bot > 0) { if (threadIdx.x == 0) tab[bot] = make_int4(x, y, known, 0); }
    else tab[threadIdx.x] = make_int4(0, 0, 0, 0);
}

// ---- host side ------------------------------------------------------------------------------------
static size_t qs_veil_layout(void *base, size_t cap, QvWorkspace &vw)
{
    const size_t blocks = (cap + QV_BLOCK - 1) / QV_BLOCK;
    Carve k(base);
    vw.cell = k.take<unsigned int>(cap);
    vw.blk_last = k.take<unsigned short>(blocks * QV_BLOCK);
    vw.blk_in = k.take<unsigned int>(blocks * QV_BLOCK);
    vw.veiled = k.take<unsigned char>(4 * cap);
    vw.hit = k.take<unsigned char>(4 * cap);
    return k.bytes;
}

// the table and the statistics word, allocated by the first call that needs them (a context that never asks has neither)
static int veil_state(qs_ctx *c)
{
    if (c->veil_tab.p) return QS_OK;
    DevBuf<int4> tab;
    DevBuf<unsigned long long> total;
    HIPCHK(c, tab.alloc(QV_BLOCK));
    HIPCHK(c, total.alloc(1));
    HIPCHK(c, hipMemsetAsync(tab.p, 0, QV_BLOCK * sizeof(int4), c->stream));
    HIPCHK(c, hipMemsetAsync(total.p, 0, sizeof(unsigned long long), c->stream));
    c->veil_tab = std::move(tab); c->veil_total = std::move(total);
    return QS_OK;
}

hipError_t qs_launch_veil(qs_ctx *c, const uint2 *rays, size_t n, const unsigned char **hit_valid)
{
    QvWorkspace vw;
    HIPRET(c->veil_ws.reserve(qs_veil_layout(nullptr, c->cap_batch, vw), c->stream));
    qs_veil_layout(c->veil_ws.p, c->cap_batch, vw);
    const int blocks = (int)((n + QV_BLOCK - 1) / QV_BLOCK), per = QV_BLOCK / QS_WAVE;
    StageTimer t(c, QS_STAGE_VEIL_INTERNAL);
    hipLaunchKernelGGL(qs_veil_cells_kernel, dim3(blocks), dim3(QV_BLOCK), 0, c->stream, n, c->b, c->geom, vw);
    hipLaunchKernelGGL(qs_veil_scan_kernel, dim3((c->cfg.max_agent + per - 1) / per), dim3(QV_BLOCK), 0, c->stream, blocks, c->b,
                       c->geom, vw, c->veil_tab.p, c->cfg.max_agent);
    hipLaunchKernelGGL(qs_veil_mark_kernel, dim3(blocks), dim3(QV_BLOCK), 0, c->stream, n, c->b, rays, vw, c->cfg.size,
                       c->veil_radius, c->cfg.max_agent, c->veil_total.p);
    t.stop();
    c->veil_flags = vw.veiled;
    *hit_valid = vw.hit;
    return hipGetLastError();
}

extern "C" int qs_set_bot_veil(qs_ctx *c, int32_t radius_cells)
{
    ARGCHK(c, c != nullptr);
    if (radius_cells == 0) { c->veil_radius = 0; return QS_OK; }
    if (radius_cells < 0 || radius_cells > QS_BOT_VEIL_MAX_RADIUS)
        return qs_fail(c, QS_E_INVAL, "qs_set_bot_veil: the radius must lie in 0..32 cells");
    if (c->cfg.raycast_mode == 1 || !qs_tiled_supported(c))
        return qs_fail(c, QS_E_INVAL, "qs_set_bot_veil: the veil is a stage of the tiled raycast (raycast_mode 1, or a grid too large for it)");
    if (c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0)
        return qs_fail(c, QS_E_INVAL, "qs_set_bot_veil: sharded contexts are not supported");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = veil_state(c);
    if (rc != QS_OK) return rc;
    c->veil_radius = radius_cells;
    return QS_OK;
}

extern "C" int qs_bot_veil(qs_ctx *c, int32_t *radius_cells)
{
    ARGCHK(c, c != nullptr && radius_cells != nullptr);
    *radius_cells = c->veil_radius;
    return QS_OK;
}

extern "C" int qs_bot_veil_place(qs_ctx *c, int32_t bot, double x, double y)
{
    ARGCHK(c, c != nullptr);
    if (bot < 1 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_bot_veil_place: bot out of range");
    // V1 on the host: one subtraction, one division, truncation -- the same IEEE operations as qs_w2g_ll
    const double qx = (x - c->cfg.ox) / c->cfg.res, qy = (y - c->cfg.oy) / c->cfg.res;
    const double lim = (double)(1 << 30);
    if (!(fabs(qx) < lim) || !(fabs(qy) < lim)) return qs_fail(c, QS_E_RANGE, "qs_bot_veil_place: the position has no cell");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = veil_state(c);
    if (rc != QS_OK) return rc;
    hipLaunchKernelGGL(qs_veil_table_kernel, dim3(1), dim3(QS_WAVE), 0, c->stream, c->veil_tab.p, (int)bot, (int)qx, (int)qy, 1);
    HIPCHK(c, hipGetLastError());
    return QS_OK;
}

extern "C" int qs_bot_veil_forget(qs_ctx *c, int32_t bot)
{
    ARGCHK(c, c != nullptr);
    if (bot < 0 || bot > c->cfg.max_agent) return qs_fail(c, QS_E_RANGE, "qs_bot_veil_forget: bot out of range");
    if (!c->veil_tab.p) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qs_veil_table_kernel, dim3(1), dim3(bot ? QS_WAVE : QV_BLOCK), 0, c->stream, c->veil_tab.p, (int)bot, 0, 0, 0);
    HIPCHK(c, hipGetLastError());
    return QS_OK;
}

extern "C" int qs_bot_veil_cells(qs_ctx *c, int32_t *xy, uint8_t *known)
{
    ARGCHK(c, c != nullptr && xy != nullptr && known != nullptr);
    const int nb = c->cfg.max_agent + 1;
    std::vector<int4> tab((size_t)nb, make_int4(0, 0, 0, 0));
    if (c->veil_tab.p) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipMemcpyAsync(tab.data(), c->veil_tab.p, (size_t)nb * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int b = 0; b < nb; b++) {
        const bool k = b >= 1 && tab[b].z != 0;
        xy[2 * b] = k ? tab[b].x : 0; xy[2 * b + 1] = k ? tab[b].y : 0; known[b] = k ? 1 : 0;
    }
    return QS_OK;
}

extern "C" int qs_last_veiled(qs_ctx *c, uint8_t *veiled, size_t n)
{
    ARGCHK(c, c != nullptr && veiled != nullptr);
    if (!c->last_has_poses || n != c->last_n) return qs_fail(c, QS_E_INVAL, "qs_last_veiled: n does not match the last ingest");
    if (n == 0) return QS_OK;
    if (!c->last_veil) { memset(veiled, 0, 4 * n); return QS_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(veiled, c->veil_flags, 4 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_bot_veil_stats(qs_ctx *c, uint64_t *veiled_total)
{
    ARGCHK(c, c != nullptr && veiled_total != nullptr);
    *veiled_total = 0;
    if (!c->veil_total.p) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->veil_total.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *veiled_total = v;
    return QS_OK;
}

extern "C" int qs_bot_veil_time(qs_ctx *c, double *ms, uint64_t *launches, int32_t reset)
{
    ARGCHK(c, c != nullptr);
    int rc = qs_stage_times(c, nullptr, nullptr, 0);               // (folds the pending event pairs in)
    if (rc != QS_OK) return rc;
    if (ms) *ms = c->stage_ms[QS_STAGE_VEIL_INTERNAL];
    if (launches) *launches = c->stage_launches[QS_STAGE_VEIL_INTERNAL];
    if (reset) { c->stage_ms[QS_STAGE_VEIL_INTERNAL] = 0; c->stage_launches[QS_STAGE_VEIL_INTERNAL] = 0; }
    return QS_OK;
}
