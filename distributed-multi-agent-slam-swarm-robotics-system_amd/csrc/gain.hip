// gain.hip -- the unknown area a bot would see from a frontier cluster.
// The rules are this build's own (include/quasar_slam.h, "frontier gain"), all integer.  The clusters are frontier.hip's
// (label, count and sum planes), their order frontier_targets.hip's compaction (FtKeep), so slot k here is the k of every
// other frontier call.
//
//   roots      : the kept roots in slot order (compact.h).  The compaction keeps the cells' order, so the list ascends and a
//                root finds its slot by bisection: no root -> slot plane over the grid;
//   viewpoints : one thread per cell.  A member of a kept cluster makes the 64-bit key (d2 << 32) | cell from its cluster's
//                integer centroid and takes an atomicMin on its slot's key: the smallest (d2, gy*size + gx) as a pair (G2);
//   gain       : one 64-lane workgroup (= one wave) per cluster.  The wave loads the (2 range + 1)^2 patch of cell states
//                around the viewpoint into LDS, a byte a cell, reading the stamp rows coalesced and nothing outside the grid.
//                Lanes then take the square's cells in row-major order; a lane whose cell is UNKNOWN and in the disc walks
//                the reference's Bresenham line from the viewpoint to it over the patch and stops at the first OCCUPIED cell
//                (G3).  The line stays in the box its two ends span, so it stays in the patch and in the grid.  Visible
//                targets are counted by ballot / popcount (G4).
// No global atomics in the gain kernel, no device-side waits, no graphs.
#include <string.h>

#include "assign_common.h"
#include "compact.h"

#define GN_NOKEY 0xffffffffffffffffull
#define GN_NONE 0xffffffffu           // frontier.hip's label of a cell that is no frontier
enum { GN_UNKNOWN = 0, GN_FREE = 1, GN_OCC = 2, GN_OUT = 3 };     // a patch cell; GN_OUT is neither a target nor a blocker

struct GnEmitRoot {
    unsigned int *root; unsigned long long *key;
    __device__ void put(size_t slot, size_t i) const { root[slot] = (unsigned int)i; key[slot] = GN_NOKEY; }
};

QsGainLayout qs_gain_layout(void *ws, size_t n_cent)
{
    QsGainLayout L;
    Carve k(ws);
    L.root = k.take<unsigned int>(n_cent);
    L.key = k.take<unsigned long long>(n_cent);
    L.view = k.take<int2>(n_cent);
    L.gain = k.take<int>(n_cent);
    L.bytes = k.bytes;
    return L;
}

// ---- viewpoints (G2) ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
qs_gain_viewpoint_kernel(const unsigned int *__restrict__ label, const unsigned int *__restrict__ cnt,
                         const unsigned long long *__restrict__ sumx, const unsigned long long *__restrict__ sumy, int size,
                         int min_cluster, const unsigned int *__restrict__ root, int n_cent, unsigned long long *__restrict__ key)
{
    const size_t cells = (size_t)size * size;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += stride) {
        unsigned int r = label[i];
        if (r == GN_NONE) continue;
        for (unsigned int p = label[r]; p != r; p = label[r]) r = p;      // the cluster's first cell
        const unsigned int n = cnt[r];
        if ((long long)n < (long long)min_cluster) continue;              // FtKeep: no slot
        int lo = 0, hi = n_cent - 1;                                       // root[] ascends and holds r
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (root[mid] < r) lo = mid + 1; else hi = mid;
        }
        if (root[lo] != r) continue;
        const long long dx = (long long)(i % size) - (long long)(sumx[r] / n);
        const long long dy = (long long)(i / size) - (long long)(sumy[r] / n);
        // d2 < 2^29 (grids are < 2^14 wide) and cell < 2^32
        atomicMin(&key[lo], ((unsigned long long)(dx * dx + dy * dy) << 32) | (unsigned long long)i);
    }
}

// ---- gain (G3, G4): one wave per cluster ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
qs_gain_kernel(const unsigned int *__restrict__ stamps, int size, int range, const unsigned long long *__restrict__ key,
               int2 *__restrict__ view, int *__restrict__ gain)
{
    extern __shared__ unsigned char s_patch[];          // [W][W] cell states, W = 2 range + 1, the viewpoint in the middle
    const int k = blockIdx.x, lane = threadIdx.x;
    const unsigned long long kk = key[k];
    if (kk == GN_NOKEY) {                               // (a kept cluster has a member: not reached)
        if (lane == 0) { view[k] = make_int2(-1, -1); gain[k] = 0; }
        return;
    }
    const unsigned int cell = (unsigned int)(kk & 0xffffffffull);
    const int vx = (int)(cell % (unsigned int)size), vy = (int)(cell / (unsigned int)size);
    const int W = 2 * range + 1, x0 = vx - range, y0 = vy - range;
    for (int py = 0; py < W; py++) {
        const int gy = y0 + py;
        const bool row_in = gy >= 0 && gy < size;        // wave-uniform
        for (int px = lane; px < W; px += 64) {
            const int gx = x0 + px;
            unsigned char s = GN_OUT;
            if (row_in && gx >= 0 && gx < size) {
                const unsigned int st = stamps[(size_t)gy * size + gx];
                s = st == 0 ? GN_UNKNOWN : ((st & 1u) ? GN_OCC : GN_FREE);
            }
            s_patch[py * W + px] = s;
        }
    }
    __syncthreads();
    const int r2 = range * range, n_sq = W * W;
    int count = 0;
    for (int base = 0; base < n_sq; base += 64) {
        const int t = base + lane;
        bool vis = false;
        if (t < n_sq) {
            const int tx = t % W, ty = t / W;
            const int ddx = tx - range, ddy = ty - range;
            // the viewpoint itself is FREE, so `t != v` needs no test of its own
            if (ddx * ddx + ddy * ddy <= r2 && s_patch[t] == GN_UNKNOWN) {
                // _bresenham(v, t) (:158-179), raycast_common.h's recurrence; every cell but t itself is looked at
                const int dx = abs(ddx), dy = abs(ddy), sx = ddx > 0 ? 1 : -1, sy = ddy > 0 ? 1 : -1;
                int x = range, y = range, err = dx - dy;
                vis = true;
                while (x != tx || y != ty) {
                    if (s_patch[y * W + x] == GN_OCC) { vis = false; break; }
                    const int e2 = 2 * err;
                    if (e2 > -dy) { err -= dy; x += sx; }
                    if (e2 < dx) { err += dx; y += sy; }
                }
            }
        }
        count += __popcll(__ballot(vis));
    }
    if (lane == 0) { view[k] = make_int2(vx, vy); gain[k] = count; }
}

// the viewpoints and gains of the n_cent clusters FtKeep(min_cluster) keeps of a labelled frontier workspace whose compaction
// offsets are that predicate's (qs_launch_ft_centroids, phase 0): G.view, G.gain
hipError_t qs_launch_gain(qs_ctx *c, void *fr_ws, int32_t min_cluster, int32_t range, size_t n_cent, const QsGainLayout &G)
{
    if (!n_cent) return hipSuccess;
    const QsFrLayout F = qs_frontier_layout(c, fr_ws);
    HIPRET(qs_compact(c->stream, FtKeep{F.cnt, min_cluster}, c->cells, true, GnEmitRoot{G.root, G.key}, n_cent, F.chunk, F.total));
    const size_t blocks = (c->cells + 255) / 256;
    hipLaunchKernelGGL(qs_gain_viewpoint_kernel, dim3((unsigned int)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, c->stream,
                       F.label, F.cnt, F.sumx, F.sumy, c->cfg.size, min_cluster, G.root, (int)n_cent, G.key);
    const int W = 2 * range + 1;
    hipLaunchKernelGGL(qs_gain_kernel, dim3((unsigned int)n_cent), dim3(64), ((size_t)W * W + 15) & ~(size_t)15, c->stream,
                       c->d_stamps.p, c->cfg.size, range, G.key, G.view, G.gain);
    return hipGetLastError();
}

int gain_range(qs_ctx *c, int32_t range, const char *who)
{
    if (range >= 1 && range <= QS_GAIN_MAX_RANGE) return QS_OK;
    return qs_fail(c, QS_E_INVAL, (std::string(who) + ": range outside 1 .. QS_GAIN_MAX_RANGE").c_str());
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int qs_frontier_gain(qs_ctx *c, int32_t min_cluster, int32_t range, int32_t *viewpoint_xy, int32_t *gain, size_t cap,
                                size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr);
    ARGCHK(c, (viewpoint_xy == nullptr) == (gain == nullptr));
    int rc = gain_range(c, range, "qs_frontier_gain");
    if (rc != QS_OK) return rc;
    void *fws;
    size_t n_cent;
    rc = qs_count_centroids(c, min_cluster, fws, n_cent);
    if (rc != QS_OK) return rc;
    *n_out = n_cent;
    const size_t n = n_cent < cap ? n_cent : cap;
    if (!gain || !n) return QS_OK;
    HIPCHK(c, c->gain_ws.reserve(qs_gain_layout(nullptr, n_cent).bytes, c->stream));
    const QsGainLayout G = qs_gain_layout(c->gain_ws.p, n_cent);
    HIPCHK(c, qs_launch_gain(c, fws, min_cluster, range, n_cent, G));
    HIPCHK(c, hipMemcpyAsync(viewpoint_xy, G.view, n * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(gain, G.gain, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}
