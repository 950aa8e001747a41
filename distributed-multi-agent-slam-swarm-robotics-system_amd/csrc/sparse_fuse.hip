// sparse_fuse.hip -- the grid fuse of a sharded deployment without moving the whole map.
//
// The reference keeps ONE grid that every bot writes (dual_bot_mapper.py:785).  Sharded by agent over N GPUs that grid
// exists N times, and the dense fuse (MAX all-reduce of 64 MiB of stamps + SUM of 128 MiB of counters at 4096^2) moves
// all of it after every batch although a shard's bots have written a few rooms: 3 % of the cells on configs[3].  Here
// every writer of the grid sets one bit per 4 x 16-cell block it touches (qs_internal.h: QsGeom::dirty), and a fuse moves
// only those blocks:
//   lists   every rank's bitmap (all-gathered by the caller) -> ascending block ids + count      qs_sf_lists_kernel
//   pack    this rank's blocks: 64 stamps + 64 counter deltas since its previous fuse, 768 B     qs_sf_pack_kernel
//   (the caller sends the packed segment to every peer: point-to-point, all xGMI links at once)
//   apply   every rank's segment folded in: stamps atomicMax, counter deltas atomicAdd; the own     qs_sf_apply_kernel
//           deltas are counted as sent
// Only apply commits anything.  A fuse abandoned before it (the exchange failed) is carried by the next one: begin ORs
// the bitmap it saved back into the live one (qs_sf_restore_kernel) and the deltas are still there to be taken.
// All three are HBM-streaming over the dirty blocks only: a block is 4 grid rows of 64 B (stamps) / 128 B (counters) and
// one 256 B / 512 B row of the payload per wave-instruction.
#include "qs_internal.h"

#define SF_BW QS_DIRTY_BLOCK_W
#define SF_BH QS_DIRTY_BLOCK_H
#define SF_CELLS (SF_BW * SF_BH)             // 64: one lane per cell
#define SF_LIST_BLOCK 1024

static size_t qs_sf_block_bytes(const qs_ctx *c) { return SF_CELLS * (sizeof(unsigned int) + (c->d_counts.p ? sizeof(unsigned long long) : 0)); }

// ---- mark a cell range dirty (qs_fuse_buffers*: a local fold writes the grid without going through a raycast) ---------
__global__ void qs_sf_mark_rows_kernel(unsigned int *__restrict__ dirty, int pitch, int blocks_x, int by_lo, int by_hi)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = (by_hi - by_lo) * pitch;
    if (w >= n) return;
    const int col = w % pitch;
    const int left = blocks_x - 32 * col;                    // valid blocks in this word
    const unsigned int m = left >= 32 ? 0xffffffffu : (left > 0 ? ((1u << left) - 1u) : 0u);
    if (m) atomicOr(&dirty[(size_t)by_lo * pitch + w], m);
}
hipError_t qs_launch_sf_mark_range(qs_ctx *c, size_t cell_off, size_t n_cells)
{
    if (!c->d_dirty.p || n_cells == 0) return hipSuccess;
    const int by_lo = (int)(cell_off / c->cfg.size) / SF_BH;
    const int by_hi = (int)((cell_off + n_cells - 1) / c->cfg.size) / SF_BH + 1;
    const int n = (by_hi - by_lo) * c->geom.dirty_pitch;
    hipLaunchKernelGGL(qs_sf_mark_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_dirty.p, c->geom.dirty_pitch,
                       c->blocks_x, by_lo, by_hi);
    return hipGetLastError();
}

// ---- restore: the saved row of a fuse that never reached apply back into the live bitmap -----------------------------
__global__ void qs_sf_restore_kernel(unsigned int *__restrict__ dirty, const unsigned int *__restrict__ saved, size_t words)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    const unsigned int m = saved[w];
    if (m) dirty[w] |= m;                                    // stream-ordered: nothing else writes the bitmap meanwhile
}
static hipError_t qs_launch_sf_restore(qs_ctx *c)
{
    if (!c->d_dirty.p || !c->d_sf_bitmaps || c->sf_rank >= c->sf_world) return hipSuccess;
    hipLaunchKernelGGL(qs_sf_restore_kernel, dim3((unsigned int)((c->dirty_words + 255) / 256)), dim3(256), 0, c->stream, c->d_dirty.p,
                       c->d_sf_bitmaps + (size_t)c->sf_rank * c->dirty_words, c->dirty_words);
    return hipGetLastError();
}

// ---- lists: bitmap -> ascending block ids.  One workgroup per rank's bitmap; order-preserving compaction ---------------
__global__ void __launch_bounds__(SF_LIST_BLOCK)
qs_sf_lists_kernel(const unsigned int *__restrict__ bitmaps, size_t words, int pitch, int blocks_x,
                   unsigned int *__restrict__ lists, unsigned int *__restrict__ counts)
{
    __shared__ unsigned int s_wave[SF_LIST_BLOCK / QS_WAVE];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const unsigned int *bm = bitmaps + (size_t)blockIdx.x * words;
    unsigned int *out = lists + (size_t)blockIdx.x * words * 32;
    const size_t per = (words + SF_LIST_BLOCK - 1) / SF_LIST_BLOCK;
    const size_t lo = min((size_t)tid * per, words), hi = min(lo + per, words);
    // bits beyond blocks_x in a row's last word are never blocks
    auto valid = [&](size_t w) -> unsigned int {
        const int left = blocks_x - 32 * (int)(w % pitch);
        return left >= 32 ? 0xffffffffu : (left > 0 ? ((1u << left) - 1u) : 0u);
    };
    unsigned int mine = 0;
    for (size_t w = lo; w < hi; w++) mine += __popc(bm[w] & valid(w));
    unsigned int inc = mine;
    #pragma unroll
    for (int off = 1; off < QS_WAVE; off <<= 1) { const unsigned int v = __shfl_up(inc, off); if (lane >= off) inc += v; }
    if (lane == QS_WAVE - 1) s_wave[wave] = inc;
    __syncthreads();
    unsigned int run = inc - mine;
    for (int v = 0; v < wave; v++) run += s_wave[v];
    for (size_t w = lo; w < hi; w++) {
        unsigned int m = bm[w] & valid(w);
        while (m) { const int b = __ffs(m) - 1; m &= m - 1; out[run++] = (unsigned int)(w * 32 + b); }
    }
    if (tid == SF_LIST_BLOCK - 1) counts[blockIdx.x] = run;
}
static hipError_t qs_launch_sf_lists(qs_ctx *c)
{
    hipLaunchKernelGGL(qs_sf_lists_kernel, dim3(c->sf_world), dim3(SF_LIST_BLOCK), 0, c->stream, c->d_sf_bitmaps, c->dirty_words,
                       c->geom.dirty_pitch, c->blocks_x, c->d_sf_lists, c->d_sf_counts);
    return hipGetLastError();
}
// one bitmap of the dirty-bitmap layout -> ascending block ids + count (the checkpoint's census, checkpoint.hip)
hipError_t qs_launch_sf_list_of(qs_ctx *c, const unsigned int *bitmap, size_t words, int pitch, int blocks_x, unsigned int *list,
                                unsigned int *count)
{
    hipLaunchKernelGGL(qs_sf_lists_kernel, dim3(1), dim3(SF_LIST_BLOCK), 0, c->stream, bitmap, words, pitch, blocks_x, list, count);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
qs_sf_popcount_kernel(const unsigned int *__restrict__ bm, size_t words, int pitch, int blocks_x, unsigned long long *__restrict__ out)
{
    unsigned int n = 0;
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
        const int left = blocks_x - 32 * (int)(w % pitch);
        const unsigned int m = left >= 32 ? 0xffffffffu : (left > 0 ? ((1u << left) - 1u) : 0u);
        n += __popc(bm[w] & m);
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, (unsigned long long)n);
}
static hipError_t qs_launch_sf_popcount(qs_ctx *c, unsigned long long *d_out)
{
    hipError_t e = hipMemsetAsync(d_out, 0, sizeof(unsigned long long), c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(qs_sf_popcount_kernel, dim3(64), dim3(256), 0, c->stream, c->d_dirty.p, c->dirty_words, c->geom.dirty_pitch,
                       c->blocks_x, d_out);
    return hipGetLastError();
}

// ---- pack: one wave per block, one lane per cell ---------------------------------------------------------------------
template <bool COUNTS>
__global__ void __launch_bounds__(256)
qs_sf_pack_kernel(const unsigned int *__restrict__ list, unsigned int n_blocks, int pitch, int size,
                  const unsigned int *__restrict__ stamps, const unsigned long long *__restrict__ counts,
                  const unsigned long long *__restrict__ sent, unsigned char *__restrict__ dst)
{
    const int lane = threadIdx.x & (QS_WAVE - 1);
    const unsigned int wave = blockIdx.x * (256 / QS_WAVE) + (threadIdx.x >> 6), n_waves = gridDim.x * (256 / QS_WAVE);
    constexpr size_t BB = SF_CELLS * (4 + (COUNTS ? 8 : 0));
    for (unsigned int k = wave; k < n_blocks; k += n_waves) {
        size_t cell;
        const bool in = qs_block_cell(list[k], lane, pitch, size, cell);
        unsigned char *blk = dst + (size_t)k * BB;
        ((unsigned int *)blk)[lane] = in ? stamps[cell] : 0u;
        if (COUNTS) {
            unsigned long long d = 0;
            if (in) {
                const unsigned long long cur = counts[cell], old = sent[cell];
                // hi32 hits, lo32 misses: the halves are independent counters, so the delta is taken per half
                d = ((unsigned long long)((unsigned int)(cur >> 32) - (unsigned int)(old >> 32)) << 32) |
                    (unsigned long long)((unsigned int)cur - (unsigned int)old);
            }                                                  // (`sent` advances in apply, once the segment has travelled)
            ((unsigned long long *)(blk + SF_CELLS * 4))[lane] = d;
        }
    }
}
static hipError_t qs_launch_sf_pack(qs_ctx *c, unsigned int n_own, unsigned char *dst)
{
    if (n_own == 0) return hipSuccess;
    const unsigned int *list = c->d_sf_lists + (size_t)c->sf_rank * c->dirty_words * 32;
    const unsigned int blocks = (n_own + 3) / 4 < 4096 ? (n_own + 3) / 4 : 4096;
    if (c->d_counts.p)
        hipLaunchKernelGGL(qs_sf_pack_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, list, n_own, c->geom.dirty_pitch, c->cfg.size,
                           c->d_stamps.p, c->d_counts.p, c->d_counts_sent.p, dst);
    else
        hipLaunchKernelGGL(qs_sf_pack_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, list, n_own, c->geom.dirty_pitch, c->cfg.size,
                           c->d_stamps.p, c->d_counts.p, c->d_counts_sent.p, dst);
    return hipGetLastError();
}

// ---- apply: every rank's segment.  Blocks of different ranks may coincide (rooms that share a block): atomics ------------
struct SfPlan { unsigned int first[QS_SPARSE_MAX_WORLD + 1]; size_t off[QS_SPARSE_MAX_WORLD]; int world, rank; };

template <bool COUNTS>
__global__ void __launch_bounds__(256)
qs_sf_apply_kernel(SfPlan pl, const unsigned int *__restrict__ lists, size_t list_stride, int pitch, int size,
                   const unsigned char *__restrict__ payload, unsigned int *__restrict__ stamps,
                   unsigned long long *__restrict__ fused, unsigned long long *__restrict__ sent)
{
    const int lane = threadIdx.x & (QS_WAVE - 1);
    const unsigned int wave = blockIdx.x * (256 / QS_WAVE) + (threadIdx.x >> 6), n_waves = gridDim.x * (256 / QS_WAVE);
    constexpr size_t BB = SF_CELLS * (4 + (COUNTS ? 8 : 0));
    const unsigned int total = pl.first[pl.world];
    int s = 0;
    for (unsigned int t = wave; t < total; t += n_waves) {
        while (pl.first[s + 1] <= t) s++;                                  // (t ascends: the search never goes back)
        const unsigned int k = t - pl.first[s];
        size_t cell;
        const bool in = qs_block_cell(lists[(size_t)s * list_stride + k], lane, pitch, size, cell);
        const unsigned char *blk = payload + pl.off[s] + (size_t)k * BB;
        if (s != pl.rank) {                                                  // own stamps are in place
            const unsigned int v = ((const unsigned int *)blk)[lane];
            if (in && v) atomicMax(&stamps[cell], v);
        }
        if (COUNTS) {
            const unsigned long long d = ((const unsigned long long *)(blk + SF_CELLS * 4))[lane];
            if (in && d) {
                atomicAdd(&fused[cell], d);
                if (s == pl.rank) {                                          // own block: a cell occurs once in the own list
                    // per half, with wrap-around, as pack took the delta: one 64-bit add would carry misses into hits
                    const unsigned long long old = sent[cell];
                    sent[cell] = ((unsigned long long)((unsigned int)(old >> 32) + (unsigned int)(d >> 32)) << 32) |
                                 (unsigned long long)((unsigned int)old + (unsigned int)d);
                }
            }
        }
    }
}
static hipError_t qs_launch_sf_apply(qs_ctx *c)
{
    SfPlan pl{};
    pl.world = c->sf_world; pl.rank = c->sf_rank;
    unsigned int run = 0;
    for (int s = 0; s < c->sf_world; s++) { pl.first[s] = run; run += c->sf_n[s]; pl.off[s] = c->sf_off[s]; }
    pl.first[c->sf_world] = run;
    if (run == 0) return hipSuccess;
    const unsigned int blocks = (run + 3) / 4 < 8192 ? (run + 3) / 4 : 8192;
    if (c->d_counts.p)
        hipLaunchKernelGGL(qs_sf_apply_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, pl, c->d_sf_lists, c->dirty_words * 32,
                           c->geom.dirty_pitch, c->cfg.size, c->sf_payload.p, c->d_stamps.p, c->d_counts_fused.p, c->d_counts_sent.p);
    else
        hipLaunchKernelGGL(qs_sf_apply_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, pl, c->d_sf_lists, c->dirty_words * 32,
                           c->geom.dirty_pitch, c->cfg.size, c->sf_payload.p, c->d_stamps.p, c->d_counts_fused.p, c->d_counts_sent.p);
    return hipGetLastError();
}

// ---- C ABI: sparse fuse (protocol in include/quasar_slam.h) ----------------------------------------------------------
extern "C" int qs_dirty_tracking(qs_ctx *c, int32_t enable)
{
    ARGCHK(c, c != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!enable) {
        c->geom.dirty = nullptr; c->geom.dirty_pitch = 0;
        c->d_dirty = DevBuf<unsigned int>();
        c->sf_state = 0;
        c->counts_view_fused = false;         // the fused counters stop following the ranks: the views read the own ones
        return QS_OK;
    }
    if (c->d_dirty.p) return QS_OK;
    if (c->dirty_since_fuse) return qs_fail(c, QS_E_STATE, "qs_dirty_tracking: the grid has unfused writes (enable it after qs_create / qs_reset / a fuse)");
    c->blocks_x = (c->cfg.size + QS_DIRTY_BLOCK_W - 1) / QS_DIRTY_BLOCK_W;
    c->blocks_y = (c->cfg.size + QS_DIRTY_BLOCK_H - 1) / QS_DIRTY_BLOCK_H;
    const int pitch = (c->blocks_x + 31) / 32;
    c->dirty_words = (size_t)c->blocks_y * pitch;
    if (c->d_counts.p) {
        const size_t nb = c->cells * sizeof(unsigned long long);
        if (!c->d_counts_sent.p) HIPCHK(c, c->d_counts_sent.alloc(c->cells));
        // the fused counters accumulate deltas from here on: they start as "nothing sent", the local counters as all delta
        HIPCHK(c, hipMemsetAsync(c->d_counts_sent.p, 0, nb, c->stream));
        if (!c->d_counts_fused.p) HIPCHK(c, c->d_counts_fused.alloc(c->cells));
        HIPCHK(c, hipMemsetAsync(c->d_counts_fused.p, 0, nb, c->stream));
        // counters written before tracking was switched on have no dirty bit: everything is marked once
    }
    // the bitmap last, published with geom.dirty: tracking is on (d_dirty set) only once everything it writes exists
    HIPCHK(c, c->d_dirty.alloc(c->dirty_words));
    c->geom.dirty = c->d_dirty.p; c->geom.dirty_pitch = pitch;
    HIPCHK(c, hipMemsetAsync(c->d_dirty.p, 0, c->dirty_words * sizeof(unsigned int), c->stream));
    if (c->next_seq != 0) HIPCHK(c, qs_launch_sf_mark_range(c, 0, c->cells));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_dirty_blocks(qs_ctx *c, size_t *n_blocks, size_t *block_cells)
{
    ARGCHK(c, c != nullptr && n_blocks != nullptr);
    if (!c->d_dirty.p) return qs_fail(c, QS_E_STATE, "qs_dirty_blocks: dirty tracking is off (qs_dirty_tracking)");
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, c->io_ws.reserve(sizeof(unsigned long long), c->stream, QS_IO_WS_FLOOR));
    unsigned long long v = 0;
    HIPCHK(c, qs_launch_sf_popcount(c, (unsigned long long *)c->io_ws.p));
    HIPCHK(c, hipMemcpyAsync(&v, c->io_ws.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_blocks = (size_t)v;
    if (block_cells) *block_cells = (size_t)QS_DIRTY_BLOCK_W * QS_DIRTY_BLOCK_H;
    return QS_OK;
}

// the per-rank arrays of a fuse of `world` ranks, carved from base (nullptr: only the size); returns the bytes
static size_t sf_layout(const qs_ctx *c, void *base, int world, unsigned int *&bitmaps, unsigned int *&lists, unsigned int *&counts)
{
    Carve k(base);
    bitmaps = k.take<unsigned int>((size_t)world * c->dirty_words);
    lists = k.take<unsigned int>((size_t)world * c->dirty_words * 32);
    counts = k.take<unsigned int>((size_t)world);
    return k.bytes;
}

extern "C" int qs_sparse_fuse_begin(qs_ctx *c, int32_t world, int32_t rank, void **bitmaps_dev, size_t *bitmap_bytes)
{
    ARGCHK(c, c != nullptr && bitmaps_dev != nullptr && bitmap_bytes != nullptr);
    ARGCHK(c, world >= 1 && world <= QS_SPARSE_MAX_WORLD && rank >= 0 && rank < world);
    if (!c->d_dirty.p) return qs_fail(c, QS_E_STATE, "qs_sparse_fuse_begin: dirty tracking is off (qs_dirty_tracking)");
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    // a fuse begun here that never reached apply: its blocks did not travel, so they go into this one (before a change of
    // world reallocates the bitmaps).  Nothing else was committed: the counter deltas are taken from `sent`, which only
    // apply advances.
    if (c->sf_state != 0) { HIPCHK(c, qs_launch_sf_restore(c)); c->sf_state = 0; }
    if (world != c->sf_world) {                              // (a growth that fails leaves the old arrays as they were)
        unsigned int *bm, *li, *co;
        DevBuf<char> meta;
        HIPCHK(c, meta.alloc(sf_layout(c, nullptr, world, bm, li, co)));
        HIPCHK(c, hipStreamSynchronize(c->stream));          // (the old arrays may still be in use)
        c->sf_meta = std::move(meta);
        sf_layout(c, c->sf_meta.p, world, c->d_sf_bitmaps, c->d_sf_lists, c->d_sf_counts);
        c->sf_world = world;
        c->sf_n.assign(world, 0); c->sf_off.assign((size_t)world + 1, 0);
    }
    c->sf_rank = rank;
    const size_t nb = c->dirty_words * sizeof(unsigned int);
    HIPCHK(c, hipMemcpyAsync(c->d_sf_bitmaps + (size_t)rank * c->dirty_words, c->d_dirty.p, nb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_dirty.p, 0, nb, c->stream));
    *bitmaps_dev = c->d_sf_bitmaps; *bitmap_bytes = nb;
    c->sf_state = 1;
    return QS_OK;
}

extern "C" int qs_sparse_fuse_plan(qs_ctx *c, uint32_t *n_blocks, size_t *offsets, void **payload_dev, size_t *block_bytes)
{
    ARGCHK(c, c != nullptr && n_blocks != nullptr && offsets != nullptr && payload_dev != nullptr);
    if (c->sf_state != 1) return qs_fail(c, QS_E_STATE, "qs_sparse_fuse_plan: call qs_sparse_fuse_begin (and all-gather the bitmaps) first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, qs_launch_sf_lists(c));
    HIPCHK(c, hipMemcpyAsync(c->sf_n.data(), c->d_sf_counts, (size_t)c->sf_world * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t bb = qs_sf_block_bytes(c);
    size_t run = 0;
    for (int s = 0; s < c->sf_world; s++) { c->sf_off[s] = run; run += (size_t)c->sf_n[s] * bb; n_blocks[s] = c->sf_n[s]; offsets[s] = c->sf_off[s]; }
    c->sf_off[c->sf_world] = run; offsets[c->sf_world] = run;
    HIPCHK(c, c->sf_payload.reserve(run, c->stream, (size_t)1 << 20));        // doubling from 1 MiB
    HIPCHK(c, qs_launch_sf_pack(c, c->sf_n[c->sf_rank], c->sf_payload.p + c->sf_off[c->sf_rank]));
    *payload_dev = c->sf_payload.p;
    if (block_bytes) *block_bytes = bb;
    c->sf_state = 2;
    return QS_OK;
}

extern "C" int qs_sparse_fuse_apply(qs_ctx *c)
{
    ARGCHK(c, c != nullptr);
    if (c->sf_state != 2) return qs_fail(c, QS_E_STATE, "qs_sparse_fuse_apply: call qs_sparse_fuse_plan (and exchange the segments) first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, qs_launch_sf_apply(c));
    c->sf_state = 0;
    c->dirty_since_fuse = false;
    if (c->d_counts.p) c->counts_view_fused = true;
    return QS_OK;
}
