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
//   4. order-preserving compaction of the roots -> clusters in the reference's order.
// The centroid itself (two divisions per cluster) is left to the host: it is exact integer/fp64
// arithmetic on these sums.  BFS visiting order inside a cluster is not reproduced (it only orders
// the membership lists, which nothing downstream reads).
#include <string.h>

#include "qs_internal.h"

#define FR_BLOCK 256
#define FR_CHUNK QS_FR_CHUNK
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

// order-preserving compaction (chunk counts -> scan -> ranked writes); MODE 0: every frontier
// cell (get_frontiers), MODE 1: component roots (one per cluster, in first-cell order)
template <int MODE>
__device__ inline bool fr_pred(const unsigned int *label, const unsigned int *cnt, size_t i)
{
    if (MODE == 0 || MODE == 2) return label[i] != FR_NONE;
    return cnt[i] != 0;
}

template <int MODE>
__global__ void __launch_bounds__(FR_BLOCK)
qs_frontier_count_kernel(const unsigned int *__restrict__ label, const unsigned int *__restrict__ cnt, size_t cells,
                         unsigned int *__restrict__ chunk_count)
{
    __shared__ unsigned int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * FR_CHUNK;
    unsigned int m = 0;
    for (int q = 0; q < FR_CHUNK / FR_BLOCK; q++) {
        const size_t i = base + q * FR_BLOCK + threadIdx.x;
        if (i < cells && fr_pred<MODE>(label, cnt, i)) m++;
    }
    if (m) atomicAdd(&s, m);
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = s;
}

__global__ void __launch_bounds__(1024)
qs_frontier_scan_kernel(unsigned int *__restrict__ chunk_count, size_t n_chunks, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long s_part[1024];
    const int tid = threadIdx.x;
    const size_t per = (n_chunks + 1023) / 1024;
    const size_t lo = min((size_t)tid * per, n_chunks), hi = min(lo + per, n_chunks);
    unsigned long long sum = 0;
    for (size_t k = lo; k < hi; k++) sum += chunk_count[k];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 1024; t++) { const unsigned long long v = s_part[t]; s_part[t] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    unsigned long long run = s_part[tid];
    for (size_t k = lo; k < hi; k++) { const unsigned int v = chunk_count[k]; chunk_count[k] = (unsigned int)run; run += v; }
}

template <int MODE>
__global__ void __launch_bounds__(FR_BLOCK)
qs_frontier_write_kernel(const unsigned int *__restrict__ label, const unsigned int *__restrict__ cnt,
                         const unsigned long long *__restrict__ sumx, const unsigned long long *__restrict__ sumy,
                         size_t cells, int size, const unsigned int *__restrict__ chunk_off,
                         int *__restrict__ out_xy, long long *__restrict__ out_stats, size_t cap)
{
    __shared__ unsigned int s_wave[FR_BLOCK / QS_WAVE];
    __shared__ unsigned int s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = chunk_off[blockIdx.x];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * FR_CHUNK;
    for (int q = 0; q < FR_CHUNK / FR_BLOCK; q++) {
        const size_t i = base + q * FR_BLOCK + tid;
        const bool on = i < cells && fr_pred<MODE>(label, cnt, i);
        const unsigned long long m = __ballot(on);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        unsigned int off = s_run;
        for (int v = 0; v < wave; v++) off += s_wave[v];
        if (on) {
            const size_t slot = off + __popcll(m & ((1ull << lane) - 1));
            if (slot < cap) {
                if (MODE == 0) { out_xy[2 * slot] = (int)(i % size); out_xy[2 * slot + 1] = (int)(i / size); }
                else if (MODE == 2) {
                    unsigned int r = (unsigned int)i;                       // the cluster's first cell: walk to the root
                    for (unsigned int p = label[r]; p != r; p = label[r]) r = p;
                    out_xy[3 * slot] = (int)(i % size); out_xy[3 * slot + 1] = (int)(i / size); out_xy[3 * slot + 2] = (int)r;
                }
                else {
                    out_stats[5 * slot] = cnt[i];
                    out_stats[5 * slot + 1] = (long long)(i % size); out_stats[5 * slot + 2] = (long long)(i / size);
                    out_stats[5 * slot + 3] = (long long)sumx[i]; out_stats[5 * slot + 4] = (long long)sumy[i];
                }
            }
        }
        __syncthreads();
        if (tid == 0) { unsigned int t = 0; for (int v = 0; v < FR_BLOCK / QS_WAVE; v++) t += s_wave[v]; s_run += t; }
        __syncthreads();
    }
}

static inline unsigned int fr_blocks(size_t items)
{
    size_t b = (items + FR_BLOCK - 1) / FR_BLOCK;
    return (unsigned int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

QsFrLayout qs_frontier_layout(const qs_ctx *c, void *ws)
{
    const size_t cells = c->cells, n_chunks = (cells + FR_CHUNK - 1) / FR_CHUNK;
    Carve k(ws);
    QsFrLayout L;
    L.label = k.take<unsigned int>(cells);
    L.cnt = k.take<unsigned int>(cells);        // cnt .. sumy: one memset clears them (qs_launch_frontier_label)
    L.sumx = k.take<unsigned long long>(cells);
    L.sumy = k.take<unsigned long long>(cells);
    L.chunk = k.take<unsigned int>(n_chunks);
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

// phase 0: count + scan (total -> *d_total); phase 1: ranked write
static hipError_t qs_launch_frontier_compact(qs_ctx *c, void *ws, int mode, int phase, int *d_xy, long long *d_stats, size_t cap)
{
    const size_t cells = c->cells, n_chunks = (cells + FR_CHUNK - 1) / FR_CHUNK;
    const QsFrLayout L = qs_frontier_layout(c, ws);
    unsigned int *label = L.label, *cnt = L.cnt, *chunk = L.chunk;
    unsigned long long *sumx = L.sumx, *sumy = L.sumy;
    if (phase == 0) {
        if (mode == 0) hipLaunchKernelGGL(qs_frontier_count_kernel<0>, dim3((unsigned int)n_chunks), dim3(FR_BLOCK), 0, c->stream, label, cnt, cells, chunk);
        else hipLaunchKernelGGL(qs_frontier_count_kernel<1>, dim3((unsigned int)n_chunks), dim3(FR_BLOCK), 0, c->stream, label, cnt, cells, chunk);
        hipLaunchKernelGGL(qs_frontier_scan_kernel, dim3(1), dim3(1024), 0, c->stream, chunk, n_chunks, L.total);
    } else {
        if (mode == 0) hipLaunchKernelGGL(qs_frontier_write_kernel<0>, dim3((unsigned int)n_chunks), dim3(FR_BLOCK), 0, c->stream, label, cnt, sumx, sumy, cells, c->cfg.size, chunk, d_xy, d_stats, cap);
        else if (mode == 2) hipLaunchKernelGGL(qs_frontier_write_kernel<2>, dim3((unsigned int)n_chunks), dim3(FR_BLOCK), 0, c->stream, label, cnt, sumx, sumy, cells, c->cfg.size, chunk, d_xy, d_stats, cap);
        else hipLaunchKernelGGL(qs_frontier_write_kernel<1>, dim3((unsigned int)n_chunks), dim3(FR_BLOCK), 0, c->stream, label, cnt, sumx, sumy, cells, c->cfg.size, chunk, d_xy, d_stats, cap);
    }
    return hipGetLastError();
}

// exclusive scan of the chunk counts a count kernel left in the workspace; the sum -> total
hipError_t qs_launch_frontier_scan(qs_ctx *c, void *ws)
{
    const QsFrLayout L = qs_frontier_layout(c, ws);
    hipLaunchKernelGGL(qs_frontier_scan_kernel, dim3(1), dim3(1024), 0, c->stream, L.chunk, (c->cells + FR_CHUNK - 1) / FR_CHUNK, L.total);
    return hipGetLastError();
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
    HIPCHK(c, qs_launch_frontier_compact(c, ws, mode == 2 ? 0 : mode, 0, nullptr, nullptr, 0));
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
        HIPCHK(c, qs_launch_frontier_compact(c, ws, mode, 1, d.p, nullptr, (size_t)total));
        HIPCHK(c, hipMemcpyAsync(xy, d.p, per * m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return QS_OK;
    }
    // clusters: all components come back in first-cell order; the size filter keeps that order (:228-229)
    std::vector<long long> all(5 * (size_t)total);
    if (total) {
        DevBuf<long long> d;
        HIPCHK(c, d.alloc(5 * (size_t)total));
        HIPCHK(c, qs_launch_frontier_compact(c, ws, 1, 1, nullptr, d.p, (size_t)total));
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
