// frontier.hip -- frontier detection and clustering on the device grid.
// Semantics: OccupancyGrid.get_frontiers / cluster_frontiers / cluster_centroid_world
// (server_nodes/dual_bot_mapper.py:181-237), called every 3 s from main() (:948-956).
//
// The reference walks the grid in a Python double loop and flood-fills with a BFS.  Here:
//   1. stencil  : interior cell is a frontier iff FREE and a 4-neighbour is UNKNOWN (:187-195),
//                 read straight from the stamp grid (stamp 0 = UNKNOWN, even = FREE);
//   2. union    : 4-connected components by union-find with atomicMin, always linking the larger
//                 root under the smaller, so a component's root is its LOWEST linear index -- the
//                 first cell the reference's row-major seed loop meets (:210), which is also what
//                 orders the reference's cluster list;
//   3. flatten + integer sums per root (count, sum gx, sum gy: what cluster_centroid_world divides);
//   4. order-preserving compaction (compact.h) of the roots -> clusters in the reference's order.
// The centroid itself (two divisions per cluster) is left to the host: it is exact integer/fp64
// arithmetic on these sums.  BFS visiting order inside a cluster is not reproduced (it only orders
// the membership lists, which nothing downstream reads).
#include <string.h>

#include "compact.h"

#define FR_BLOCK 256
#define FR_NONE 0xffffffffu

__device__ inline bool fr_is_free(unsigned int s) { return s != 0 && !(s & 1u); }

__global__ void __launch_bounds__(FR_BLOCK)
qs_frontier_mask_kernel(const unsigned int *__restrict__ stamps, int size, unsigned int *__restrict__ label)
{
    const size_t cells = (size_t)size * size;
    const size_t stride = (size_t)gridDim.x * FR_BLOCK;
    for (size_t i = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x; i < cells; i += stride) {
        const int x = (int)(i % size), y = (int)(i / size);
        unsigned int l = FR_NONE;
        if (x >= 1 && x < size - 1 && y >= 1 && y < size - 1 && fr_is_free(stamps[i])) {      // :187-190
            if (stamps[i - 1] == 0 || stamps[i + 1] == 0 || stamps[i - size] == 0 || stamps[i + size] == 0)   // :192-193
                l = (unsigned int)i;
        }
        label[i] = l;
    }
}

__device__ inline unsigned int fr_find(unsigned int *label, unsigned int x)
{
    unsigned int p = label[x];
    while (p != x) { x = p; p = label[x]; }
    return x;
}

__device__ inline void fr_unite(unsigned int *label, unsigned int a, unsigned int b)
{
    for (;;) {
        a = fr_find(label, a); b = fr_find(label, b);
        if (a == b) return;
        if (a > b) { const unsigned int t = a; a = b; b = t; }     // a < b: link b under a
        const unsigned int old = atomicMin(&label[b], a);
        if (old == b) return;
        b = old;                                                   // somebody relinked b meanwhile
    }
}

__global__ void __launch_bounds__(FR_BLOCK)
qs_frontier_union_kernel(int size, unsigned int *__restrict__ label)
{
    const size_t cells = (size_t)size * size;
    const size_t stride = (size_t)gridDim.x * FR_BLOCK;
    for (size_t i = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x; i < cells; i += stride) {
        if (label[i] == FR_NONE) continue;
        // frontier cells are interior, so i + 1 and i + size exist
        if (label[i + 1] != FR_NONE) fr_unite(label, (unsigned int)i, (unsigned int)(i + 1));
        if (label[i + size] != FR_NONE) fr_unite(label, (unsigned int)i, (unsigned int)(i + size));
    }
}

__global__ void __launch_bounds__(FR_BLOCK)
qs_frontier_stats_kernel(int size, unsigned int *__restrict__ label, unsigned int *__restrict__ cnt,
                         unsigned long long *__restrict__ sumx, unsigned long long *__restrict__ sumy)
{
    const size_t cells = (size_t)size * size;
    const size_t stride = (size_t)gridDim.x * FR_BLOCK;
    for (size_t i = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x; i < cells; i += stride) {
        if (label[i] == FR_NONE) continue;
        const unsigned int r = fr_find(label, (unsigned int)i);
        atomicAdd(&cnt[r], 1u);
        atomicAdd(&sumx[r], (unsigned long long)(i % size));
        atomicAdd(&sumy[r], (unsigned long long)(i / size));
    }
}

// the compactions (compact.h): every frontier cell (get_frontiers) -> (gx, gy), or -> (gx, gy, root); the component roots
// (cnt != 0: one per cluster, in first-cell order) -> the five statistics
struct FrCell { const unsigned int *label; __device__ bool marked(size_t i) const { return label[i] != FR_NONE; } };
struct FrRoot { const unsigned int *cnt; __device__ bool marked(size_t i) const { return cnt[i] != 0; } };
struct FrEmitXY {
    int size; int *xy;
    __device__ void put(size_t slot, size_t i) const { xy[2 * slot] = (int)(i % size); xy[2 * slot + 1] = (int)(i / size); }
};
struct FrEmitXYRoot {
    const unsigned int *label; int size; int *xy;
    __device__ void put(size_t slot, size_t i) const
    {
        unsigned int r = (unsigned int)i;                       // the cluster's first cell: walk to the root
        for (unsigned int p = label[r]; p != r; p = label[r]) r = p;
        xy[3 * slot] = (int)(i % size); xy[3 * slot + 1] = (int)(i / size); xy[3 * slot + 2] = (int)r;
    }
};
struct FrEmitStats {
    const unsigned int *cnt; const unsigned long long *sumx, *sumy; int size; long long *stats;
    __device__ void put(size_t slot, size_t i) const
    {
        const long long n = cnt[i], sx = (long long)sumx[i], sy = (long long)sumy[i];
        stats[5 * slot] = n;
        stats[5 * slot + 1] = (long long)(i % size); stats[5 * slot + 2] = (long long)(i / size);
        stats[5 * slot + 3] = sx; stats[5 * slot + 4] = sy;
    }
};

static inline unsigned int fr_blocks(size_t items)
{
    size_t b = (items + FR_BLOCK - 1) / FR_BLOCK;
    return (unsigned int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

QsFrLayout qs_frontier_layout(const qs_ctx *c, void *ws)
{
    const size_t cells = c->cells;
    Carve k(ws);
    QsFrLayout L;
    L.label = k.take<unsigned int>(cells);
    L.cnt = k.take<unsigned int>(cells);        // cnt .. sumy: one memset clears them (qs_launch_frontier_label)
    L.sumx = k.take<unsigned long long>(cells);
    L.sumy = k.take<unsigned long long>(cells);
    L.chunk = k.take<unsigned int>(qs_compact_chunks(cells));
    L.total = k.take<unsigned long long>(1);
    L.bytes = k.bytes;
    return L;
}

hipError_t qs_launch_frontier_label(qs_ctx *c, void *ws, bool with_clusters)
{
    const size_t cells = c->cells;
    const QsFrLayout L = qs_frontier_layout(c, ws);
    hipLaunchKernelGGL(qs_frontier_mask_kernel, dim3(fr_blocks(cells)), dim3(FR_BLOCK), 0, c->stream, c->d_stamps.p,
                       c->cfg.size, L.label);
    if (with_clusters) {
        hipError_t e = hipMemsetAsync(L.cnt, 0, (char *)(L.sumy + cells) - (char *)L.cnt, c->stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(qs_frontier_union_kernel, dim3(fr_blocks(cells)), dim3(FR_BLOCK), 0, c->stream, c->cfg.size, L.label);
        hipLaunchKernelGGL(qs_frontier_stats_kernel, dim3(fr_blocks(cells)), dim3(FR_BLOCK), 0, c->stream, c->cfg.size, L.label,
                           L.cnt, L.sumx, L.sumy);
    }
    return hipGetLastError();
}

// mode 0: cells, 1: cluster roots, 2: cells with their roots.  !write: count + scan (the total -> L.total); write: the ranked
// writes of the first cap items to d_xy (modes 0, 2) / d_stats (mode 1)
static hipError_t qs_launch_frontier_compact(qs_ctx *c, void *ws, int mode, bool write, int *d_xy, long long *d_stats, size_t cap)
{
    const QsFrLayout L = qs_frontier_layout(c, ws);
    const int size = c->cfg.size;
    if (mode == 0) return qs_compact(c->stream, FrCell{L.label}, c->cells, write, FrEmitXY{size, d_xy}, cap, L.chunk, L.total);
    if (mode == 2) return qs_compact(c->stream, FrCell{L.label}, c->cells, write, FrEmitXYRoot{L.label, size, d_xy}, cap, L.chunk, L.total);
    return qs_compact(c->stream, FrRoot{L.cnt}, c->cells, write, FrEmitStats{L.cnt, L.sumx, L.sumy, size, d_stats}, cap, L.chunk, L.total);
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------
static int frontier_run(qs_ctx *c, int mode, int32_t min_cluster, int32_t *xy, int64_t *stats5, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, c->frontier_ws.reserve(qs_frontier_layout(c, nullptr).bytes, c->stream));
    void *ws = c->frontier_ws.p;
    HIPCHK(c, qs_launch_frontier_label(c, ws, mode != 0));
    HIPCHK(c, qs_launch_frontier_compact(c, ws, mode, false, nullptr, nullptr, 0));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, qs_frontier_layout(c, ws).total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode != 1) {
        // cells (mode 0: gx, gy), or every frontier cell with the first cell (row-major) of its 4-connected cluster (mode 2:
        // gx, gy, root linear index)
        *n_out = (size_t)total;
        if (!xy || total == 0) return QS_OK;
        const size_t per = mode == 0 ? 2 : 3, m = total < cap ? (size_t)total : cap;
        DevBuf<int> d;
        HIPCHK(c, d.alloc(per * (size_t)total));
        HIPCHK(c, qs_launch_frontier_compact(c, ws, mode, true, d.p, nullptr, (size_t)total));
        HIPCHK(c, hipMemcpyAsync(xy, d.p, per * m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return QS_OK;
    }
    // clusters: all components come back in first-cell order; the size filter keeps that order (:228-229)
    std::vector<long long> all(5 * (size_t)total);
    if (total) {
        DevBuf<long long> d;
        HIPCHK(c, d.alloc(5 * (size_t)total));
        HIPCHK(c, qs_launch_frontier_compact(c, ws, 1, true, nullptr, d.p, (size_t)total));
        HIPCHK(c, hipMemcpyAsync(all.data(), d.p, all.size() * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    size_t k = 0;
    for (size_t i = 0; i < (size_t)total; i++) {
        if (all[5 * i] < min_cluster) continue;
        if (stats5 && k < cap) memcpy(stats5 + 5 * k, &all[5 * i], 5 * sizeof(long long));
        k++;
    }
    *n_out = k;
    return QS_OK;
}

extern "C" int qs_frontier_cells(qs_ctx *c, int32_t *xy, size_t cap, size_t *n_out)
{ return frontier_run(c, 0, 0, xy, nullptr, cap, n_out); }

extern "C" int qs_frontier_members(qs_ctx *c, int32_t *xy_root, size_t cap, size_t *n_out)
{ return frontier_run(c, 2, 0, xy_root, nullptr, cap, n_out); }

extern "C" int qs_frontier_clusters(qs_ctx *c, int32_t min_cluster, int64_t *stats5, size_t cap, size_t *n_out)
{ return frontier_run(c, 1, min_cluster, nullptr, stats5, cap, n_out); }
