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
// Sweep beams are veiled by a stage of the same shape (rules S0-S8), further down: it shares the table, the statistics word and
// the scan over blocks (qv_scan_bot) with the packet stage.
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

// "latest cell" of one bot carried over the blocks, by one wave: what the packet stage and the sweep stage (below) share.  cell,
// blk_last and blk_in are the stage's arrays of those names; pose_at(i, rx, ry) gives the pose record i of the call was cast from
template <class PoseAt>
__device__ inline void qv_scan_bot(int n_blocks, const unsigned int *__restrict__ cell, const unsigned short *__restrict__ blk_last,
                                   unsigned int *__restrict__ blk_in, const QsGeom &geo, int4 *__restrict__ tab, int bot, int lane,
                                   PoseAt pose_at)
{
    const int4 t = tab[bot];
    unsigned int carry = t.z ? qv_pack(t.x, t.y) : QV_NONE;
    long long last_i = -1;                                         // the bot's last record with a cell in this call
    for (int b0 = 0; b0 < n_blocks; b0 += QS_WAVE) {
        const int blk = b0 + lane;
        unsigned int v = QV_NONE;
        long long mine = -1;
        if (blk < n_blocks) {
            const unsigned int l = blk_last[(size_t)blk * QV_BLOCK + bot];
            if (l) { mine = (long long)blk * QV_BLOCK + (l - 1); v = cell[mine]; }
        }
        // inclusive scan of "the latest cell" over the 64 blocks (a (+) b = b unless b is none), the carry entering at lane 0
        unsigned int inc = (lane == 0 && qv_none(v)) ? carry : v;
        #pragma unroll
        for (int off = 1; off < QS_WAVE; off <<= 1) {
            const unsigned int u = __shfl_up(inc, off);
            if (lane >= off && qv_none(inc)) inc = u;
        }
        const unsigned int prev = __shfl_up(inc, 1);
        if (blk < n_blocks) blk_in[(size_t)blk * QV_BLOCK + bot] = lane == 0 ? carry : prev;
        carry = __shfl(inc, QS_WAVE - 1);
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const long long o = __shfl_xor(mine, off); mine = o > mine ? o : mine; }
        if (mine >= 0) last_i = mine;
    }
    if (lane == 0 && last_i >= 0) {                                // V6, from the pose itself: the table holds unclamped cells
        int x = 0, y = 0;
        double rx, ry;
        pose_at(last_i, rx, ry);
        qv_cell(rx, ry, geo, x, y);
        tab[bot] = make_int4(x, y, 1, 0);
    }
}

__global__ void __launch_bounds__(QV_BLOCK)
qs_veil_scan_kernel(int n_blocks, QsBatch b, QsGeom geo, QvWorkspace vw, int4 *__restrict__ tab, int max_agent)
{
    const int lane = threadIdx.x & (QS_WAVE - 1);
    const int bot = 1 + blockIdx.x * (QV_BLOCK / QS_WAVE) + (threadIdx.x >> 6);
    if (bot > max_agent) return;                                   // (wave-uniform)
    qv_scan_bot(n_blocks, vw.cell, vw.blk_last, vw.blk_in, geo, tab, bot, lane,
                [&](long long i, double &rx, double &ry) { rx = b.rx[i]; ry = b.ry[i]; });
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

// ---- the sweep stage (rules S0-S8) ------------------------------------------------------------------------------------------
// The same question per chunk of a sweep call, between the sweeps' pass A and the sort: pass A has left accept[k], pose[3 k ..],
// the ray slots 184 k + i and their hit flags; the agent is byte 4 of the record.  Three kernels, as above:
//   qs_sveil_cells_kernel  one thread per sweep: its cell (S1), its agent, the block rows
//   qs_sveil_scan_kernel   qv_scan_bot over the chunk's blocks, seeded from and written back to the table: the next chunk of the call
//                          and the next call find the bots where this chunk left them (S2, S5)
//   qs_sveil_mark_kernel   one workgroup per block of QV_BLOCK sweeps, one WAVE per sweep, 16 consecutive sweeps a wave.  Per bot the
//                          block keeps a bit row in LDS (bit q: sweep q of the block is the bot's and has a cell), so "b's last
//                          sweep before p" is the highest bit below p of four 64-bit words -- four independent LDS reads and a
//                          count of leading zeros, no walk and no search.  A wave asks that once, for the first sweep of its run:
//                          the lanes take the bots, four a lane at most, and keep their cells in registers; after each sweep of
//                          the run one lane replaces one register (the sweep's bot now speaks with the sweep's cell).  Per sweep
//                          the lanes screen their bots by distance from the sweep's own cell (a binned beam ends less than 64
//                          cells from it) and compact the survivors by ballot into the wave's list.  The list is usually empty:
//                          then 46 lanes copy the sweep's 184 hit flags as dwords and the rays are never read.  Otherwise the
//                          lanes take beams lane, lane + 64, lane + 128, as pass A does, and test their end cells against the
//                          list (wave-uniform LDS reads).
// The call's flags are kept as three 64-bit ballots per sweep.
#define QSV_THREADS 1024
#define QSV_WAVES (QSV_THREADS / QS_WAVE)
#define QSV_RUN (QV_BLOCK / QSV_WAVES)         // consecutive sweeps of the block a wave takes
#define QSV_BOT_ROUNDS (QV_BLOCK / QS_WAVE)    // bots a lane keeps: 1 + lane + 64 r
#define QSV_HV_DWORDS (QS_SWEEP_SLOTS / 4)     // 184 hit flags of a sweep = 46 dwords
static_assert(QSV_THREADS == 4 * QV_BLOCK, "the mark kernel clears its bit rows one 64-bit word a thread");
static_assert(QS_SWEEP_SLOTS % 4 == 0 && QSV_HV_DWORDS <= QS_WAVE && QS_SWEEP_SLOTS <= 3 * QS_WAVE, "a sweep's flags: 46 dwords, three beams a lane");

struct QsvWorkspace {
    unsigned int *cell;                   // [cap] packed cell of an accepted sweep that has one, QV_NONE otherwise
    unsigned char *agent;                 // [cap] its agent; 0: the sweep has no cell
    unsigned short *blk_last;             // [blocks][QV_BLOCK] as QvWorkspace's
    unsigned int *blk_in;                 // [blocks][QV_BLOCK]
    unsigned char *hit;                   // [184 cap] hit_valid & !veiled of one chunk: what passes C and D see
    unsigned long long *flags;            // [3 n_call] per sweep of the call: the ballots of its veiled beams 0..63, 64..127, 128..180
};

__global__ void __launch_bounds__(QV_BLOCK)
qs_sveil_cells_kernel(size_t n, const unsigned char *__restrict__ pkts, size_t stride, const unsigned char *__restrict__ accept,
                      const double *__restrict__ pose, QsGeom geo, int max_agent, QsvWorkspace vw)
{
    __shared__ unsigned int s_last[QV_BLOCK];
    const int tid = threadIdx.x;
    s_last[tid] = 0;
    __syncthreads();
    const size_t k = (size_t)blockIdx.x * QV_BLOCK + tid;
    unsigned int cell = QV_NONE;
    int agent = 0;
    if (k < n && accept[k]) {                                      // S1: a rejected or withheld record has no cell
        const int a = pkts[k * stride + 4];
        int x, y;
        if (a >= 1 && a <= max_agent && qv_cell(pose[3 * k], pose[3 * k + 1], geo, x, y)) {
            cell = qv_pack(x, y);
            agent = a;
            atomicMax(&s_last[a], (unsigned int)tid + 1u);
        }
    }
    if (k < n) { vw.cell[k] = cell; vw.agent[k] = (unsigned char)agent; }
    __syncthreads();
    vw.blk_last[(size_t)blockIdx.x * QV_BLOCK + tid] = (unsigned short)s_last[tid];
}

__global__ void __launch_bounds__(QV_BLOCK)
qs_sveil_scan_kernel(int n_blocks, const double *__restrict__ pose, QsGeom geo, QsvWorkspace vw, int4 *__restrict__ tab, int max_agent)
{
    const int lane = threadIdx.x & (QS_WAVE - 1);
    const int bot = 1 + blockIdx.x * (QV_BLOCK / QS_WAVE) + (threadIdx.x >> 6);
    if (bot > max_agent) return;                                   // (wave-uniform)
    qv_scan_bot(n_blocks, vw.cell, vw.blk_last, vw.blk_in, geo, tab, bot, lane,
                [&](long long i, double &rx, double &ry) { rx = pose[3 * i]; ry = pose[3 * i + 1]; });
}

// k_call0: the record of the call this chunk's record 0 is (the flags are the call's)
__global__ void __launch_bounds__(QSV_THREADS)
qs_sveil_mark_kernel(size_t n, size_t k_call0, const uint2 *__restrict__ rays, const unsigned char *__restrict__ hit_valid, QsvWorkspace vw,
                     int size, int radius, int max_agent, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long s_row[QV_BLOCK][4];   // per bot: which sweeps of the block are its own (and have a cell)
    __shared__ unsigned int s_cell[QV_BLOCK];           // packed cell of sweep q
    __shared__ unsigned int s_in[QV_BLOCK];             // per bot: the cell known at the block's entry
    __shared__ unsigned int s_list[QSV_WAVES][QV_BLOCK];// per wave: the cells of the bots near its sweep
    __shared__ unsigned char s_agent[QV_BLOCK];
    __shared__ unsigned int s_tally;
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const size_t k_blk = (size_t)blockIdx.x * QV_BLOCK;
    (&s_row[0][0])[tid] = 0ull;                                     // (QSV_THREADS == 4 QV_BLOCK words)
    if (tid == 0) s_tally = 0;
    int my_agent = 0;
    if (tid < QV_BLOCK) {
        const size_t k = k_blk + tid;
        s_cell[tid] = k < n ? vw.cell[k] : QV_NONE;
        my_agent = k < n ? (int)vw.agent[k] : 0;
        s_agent[tid] = (unsigned char)my_agent;
        s_in[tid] = (tid >= 1 && tid <= max_agent) ? vw.blk_in[k_blk + tid] : QV_NONE;
    }
    __syncthreads();
    if (my_agent) atomicOr(&s_row[my_agent][tid >> 6], 1ull << (tid & 63));
    __syncthreads();

    const int lim = QT_TILE + radius, r2 = radius * radius;        // a binned beam ends less than 64 cells from its pose on each axis
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned int *list = s_list[wave];
    const unsigned int *hv32 = (const unsigned int *)hit_valid;     // (184 k is a multiple of 4: a sweep's flags are 46 aligned dwords)
    unsigned int *out32 = (unsigned int *)vw.hit;
    unsigned int cnt = 0;
    // The wave takes QSV_RUN consecutive sweeps.  Lane l keeps in registers the cell bots 1 + l, 65 + l, 129 + l, 193 + l speak with
    // (S2): looked up once, for the run's first sweep -- b's last sweep with a cell before it in this block is the highest bit below it
    // in b's row, failing that the cell the block was entered with -- and then carried: after sweep p its bot speaks with p's cell.
    const int p0 = wave * QSV_RUN;
    unsigned int cur[QSV_BOT_ROUNDS];
    #pragma unroll
    for (int r = 0; r < QSV_BOT_ROUNDS; r++) {
        const int b = 1 + QS_WAVE * r + lane;
        cur[r] = QV_NONE;
        if (b <= max_agent) {
            const int pw = p0 >> 6;
            const unsigned long long below = (1ull << (p0 & 63)) - 1ull;
            int q = -1;
            #pragma unroll
            for (int j = 0; j < 4; j++) {
                unsigned long long w = s_row[b][j];
                w = j < pw ? w : (j == pw ? (w & below) : 0ull);
                if (w) q = 64 * j + 63 - __clzll((long long)w);
            }
            cur[r] = q >= 0 ? s_cell[q] : s_in[b];
        }
    }
    for (int p = p0; p < p0 + QSV_RUN; p++) {                      // (p and everything derived from it are wave-uniform)
        const size_t k = k_blk + p;
        if (k >= n) break;
        const int agent = s_agent[p];
        const unsigned int pc = s_cell[p];
        const int px = (short)(pc & 0xffffu), py = (short)(pc >> 16);
        int n_near = 0;
        if (agent) {
            #pragma unroll
            for (int r = 0; r < QSV_BOT_ROUNDS; r++) {
                if (QS_WAVE * r >= max_agent) break;
                const unsigned int c = cur[r];
                const int bx = (short)(c & 0xffffu), by = (short)(c >> 16);
                const bool near = 1 + QS_WAVE * r + lane != agent && !qv_none(c) && abs(bx - px) <= lim && abs(by - py) <= lim;
                const unsigned long long m = __ballot(near);
                if (near) list[n_near + __popcll(m & lt)] = c;
                n_near += __popcll(m);
            }
            #pragma unroll
            for (int r = 0; r < QSV_BOT_ROUNDS; r++)               // from the next sweep on this bot speaks with this cell
                if (agent - 1 == QS_WAVE * r + lane) cur[r] = pc;
        }
        __builtin_amdgcn_wave_barrier();
        if (n_near == 0) {                                          // nobody near: the flags pass through, nothing is veiled
            if (lane < QSV_HV_DWORDS) out32[QSV_HV_DWORDS * k + lane] = hv32[QSV_HV_DWORDS * k + lane];
            if (lane < 3) vw.flags[3 * (k_call0 + k) + lane] = 0ull;
            continue;
        }
        #pragma unroll
        for (int s = 0; s < 3; s++) {
            const int i = lane + QS_WAVE * s;
            bool veil = false;
            if (i < QS_SWEEP_SLOTS) {
                const size_t r = QS_SWEEP_SLOTS * k + i;
                const unsigned char hv = hit_valid[r];
                if (hv && i < QS_SWEEP_BEAMS) {                     // S3: a hit ...
                    const uint2 rec = rays[r];
                    const int ex = (short)(rec.y & 0xffffu), ey = (short)(rec.y >> 16);
                    if ((short)(rec.x & 0xffffu) != QT_NO_RAY       // ... that pass A binned ...
                        && (unsigned int)ex < (unsigned int)size && (unsigned int)ey < (unsigned int)size)   // ... and that ends in the grid
                        for (int j = 0; j < n_near; j++) {
                            const unsigned int c = list[j];
                            const int dx = ex - (short)(c & 0xffffu), dy = ey - (short)(c >> 16);
                            veil |= dx * dx + dy * dy <= r2;
                        }
                }
                vw.hit[r] = veil ? 0 : hv;                          // S4
            }
            const unsigned long long m = __ballot(veil);
            if (lane == 0) vw.flags[3 * (k_call0 + k) + s] = m;
            cnt += (unsigned int)__popcll(m);
        }
        __builtin_amdgcn_wave_barrier();                            // (the list is rewritten for the wave's next sweep)
    }
    if (lane == 0 && cnt) atomicAdd(&s_tally, cnt);                // (cnt is wave-uniform: it sums ballots)
    __syncthreads();
    if (tid == 0 && s_tally) atomicAdd(total, (unsigned long long)s_tally);
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

// cap: the sweeps of one chunk at most; n_call: the sweeps of the whole call (its flags)
static size_t qs_sveil_layout(void *base, size_t cap, size_t n_call, QsvWorkspace &vw)
{
    const size_t blocks = (cap + QV_BLOCK - 1) / QV_BLOCK;
    Carve k(base);
    vw.cell = k.take<unsigned int>(cap);
    vw.agent = k.take<unsigned char>(cap);
    vw.blk_last = k.take<unsigned short>(blocks * QV_BLOCK);
    vw.blk_in = k.take<unsigned int>(blocks * QV_BLOCK);
    vw.hit = k.take<unsigned char>(QS_SWEEP_SLOTS * cap);
    vw.flags = k.take<unsigned long long>(3 * n_call);
    return k.bytes;
}

hipError_t qs_sweep_veil_reserve(qs_ctx *c, size_t chunk_cap, size_t n_call)
{
    QsvWorkspace vw;
    HIPRET(c->sveil_ws.reserve(qs_sveil_layout(nullptr, chunk_cap, n_call, vw), c->stream));
    c->sveil_cap = chunk_cap; c->sveil_n = n_call;
    return hipSuccess;
}

hipError_t qs_launch_sweep_veil(qs_ctx *c, const unsigned char *d_pkts, size_t stride, const unsigned char *accept, const double *pose,
                                const uint2 *rays, size_t n, size_t k_call0, const unsigned char **hit_valid)
{
    if (n > c->sveil_cap || k_call0 + n > c->sveil_n) return hipErrorInvalidValue;      // (qs_sweep_veil_reserve sized it for the call)
    QsvWorkspace vw;
    qs_sveil_layout(c->sveil_ws.p, c->sveil_cap, c->sveil_n, vw);
    const int blocks = (int)((n + QV_BLOCK - 1) / QV_BLOCK), per = QV_BLOCK / QS_WAVE;
    StageTimer t(c, QS_STAGE_VEIL_INTERNAL);
    hipLaunchKernelGGL(qs_sveil_cells_kernel, dim3(blocks), dim3(QV_BLOCK), 0, c->stream, n, d_pkts, stride, accept, pose, c->geom,
                       c->cfg.max_agent, vw);
    hipLaunchKernelGGL(qs_sveil_scan_kernel, dim3((c->cfg.max_agent + per - 1) / per), dim3(QV_BLOCK), 0, c->stream, blocks, pose, c->geom,
                       vw, c->veil_tab.p, c->cfg.max_agent);
    hipLaunchKernelGGL(qs_sveil_mark_kernel, dim3(blocks), dim3(QSV_THREADS), 0, c->stream, n, k_call0, rays, *hit_valid, vw, c->cfg.size,
                       c->veil_radius, c->cfg.max_agent, c->veil_total.p);
    t.stop();
    *hit_valid = vw.hit;
    return hipGetLastError();
}

extern "C" int qs_set_bot_veil_sweeps(qs_ctx *c, int32_t on)
{
    ARGCHK(c, c != nullptr);
    c->veil_sweeps = on != 0;
    return QS_OK;
}

extern "C" int qs_bot_veil_sweeps(qs_ctx *c, int32_t *on)
{
    ARGCHK(c, c != nullptr && on != nullptr);
    *on = c->veil_sweeps ? 1 : 0;
    return QS_OK;
}

extern "C" int qs_last_sweeps_veiled(qs_ctx *c, uint8_t *veiled, size_t n)
{
    ARGCHK(c, c != nullptr && veiled != nullptr);
    if (!c->last_sweeps || n != c->last_sweeps_n)
        return qs_fail(c, QS_E_INVAL, "qs_last_sweeps_veiled: n does not match the last sweep ingest");
    if (n == 0) return QS_OK;
    memset(veiled, 0, (size_t)QS_SWEEP_BEAMS * n);
    if (!c->last_sveil) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    QsvWorkspace vw;
    qs_sveil_layout(c->sveil_ws.p, c->sveil_cap, c->sveil_n, vw);
    std::vector<unsigned long long> f(3 * n);
    HIPCHK(c, hipMemcpyAsync(f.data(), vw.flags, 3 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < n; k++)
        for (int i = 0; i < QS_SWEEP_BEAMS; i++)
            veiled[(size_t)QS_SWEEP_BEAMS * k + i] = (uint8_t)((f[3 * k + (i >> 6)] >> (i & 63)) & 1ull);
    return QS_OK;
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
