// merge.hip -- the map merger as a device-resident session (include/quasar_slam.h: "map merge session"),
// and the voxel down-sampling that closes every merge, grouped on the device.
// Reference: server_nodes/map_merger.py:28-127.  One callback = grid_to_pcd (:64-85) -> adopt (:40-43) or registration_icp
// (:45-52) -> fitness gate (:54-56) -> transform, append, voxel_down_sample (:58-60); publish_global_map (:87-127) on request.
// Every step launches the kernels of the host-to-host entry point that does the same (grid_ops.hip, icp.hip); what is new
// here is the grouping of the voxel keys:
//   keys      qs_voxel_key_kernel (icp.hip) from the exact minimum qs_bbox_kernel finds
//   sort      stable LSD radix sort of (key, input index), 8 bits a pass, only over the bytes the box says are in use.
//             A pass is built like the tile sort of raycast_tiled.hip: qs_sort_hist_kernel leaves a row of
//             table[workgroup][digit], qs_sort_scan_kernel turns the table into first slots (digit-major, workgroups in
//             order within a digit), qs_sort_scatter_kernel adds in-workgroup ranks: a ballot per digit bit gives every
//             lane the mask of its wave's lanes with the same digit (rank = the set bits below it), wave order and round
//             order do the rest.  No global atomic anywhere: slots are a pure function of the input, equal keys keep
//             their order.
//   runs      a key that differs from its predecessor starts a voxel: the order-preserving compaction of grid_ops.hip
//             (count / scan / ranked write) leaves the runs' first positions
//   means     one lane per voxel walks its run in sorted order = input order (the sort is stable) and sums one point after
//             the other, as the host loop of qs_voxel_downsample does: a tree would round differently.
#include <math.h>
#include <utility>

#include "compact.h"

#define MS_BLOCK 256
#define MS_WAVES (MS_BLOCK / QS_WAVE)
#define MS_RADIX 256
#define MS_MAX_WG 1024                   // rows of the table (one 1024-thread workgroup scans it)
#define MS_SCAN_SEGS 4

// ---- one pass of the sort ------------------------------------------------------------------------------------------
// workgroup w owns items [w * per_wg, (w + 1) * per_wg), per_wg a multiple of MS_BLOCK
__global__ void __launch_bounds__(MS_BLOCK)
qs_sort_hist_kernel(const unsigned long long *__restrict__ keys, size_t n, int shift, size_t per_wg, unsigned int *__restrict__ table)
{
    __shared__ unsigned int s_hist[MS_RADIX];
    const int tid = threadIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    const size_t lo = (size_t)blockIdx.x * per_wg, hi = (lo + per_wg < n) ? lo + per_wg : n;
    for (size_t i = lo + tid; i < hi; i += MS_BLOCK) atomicAdd(&s_hist[(unsigned int)(keys[i] >> shift) & (MS_RADIX - 1)], 1u);   // (counts: order-free)
    __syncthreads();
    table[(size_t)blockIdx.x * MS_RADIX + tid] = s_hist[tid];
}

// table[w][d] <- items of digits below d, plus items of digit d in workgroups before w.  Thread (seg, d) owns the rows
// [seg * R, (seg + 1) * R) of column d; a wave reads 256 consecutive bytes of a row per instruction.
__global__ void __launch_bounds__(MS_SCAN_SEGS * MS_RADIX)
qs_sort_scan_kernel(unsigned int *__restrict__ table, unsigned int nwg)
{
    __shared__ unsigned int s_part[MS_SCAN_SEGS][MS_RADIX];
    __shared__ unsigned int s_wtot[MS_SCAN_SEGS * MS_RADIX / QS_WAVE];
    __shared__ unsigned int s_dig[MS_RADIX];
    const int tid = threadIdx.x, d = tid & (MS_RADIX - 1), seg = tid >> 8, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const unsigned int R = (nwg + MS_SCAN_SEGS - 1) / MS_SCAN_SEGS;
    const unsigned int w0 = min(seg * R, nwg), w1 = min(w0 + R, nwg);
    unsigned int sum = 0;
    for (unsigned int w = w0; w < w1; w++) sum += table[(size_t)w * MS_RADIX + d];
    s_part[seg][d] = sum;
    __syncthreads();
    // exclusive scan of the digit totals over the digits (threads 0..255 carry one each, the others zero)
    unsigned int tot = 0;
    if (tid < MS_RADIX) { for (int q = 0; q < MS_SCAN_SEGS; q++) tot += s_part[q][d]; }
    unsigned int inc = tot;
    #pragma unroll
    for (int off = 1; off < QS_WAVE; off <<= 1) { const unsigned int v = __shfl_up(inc, off); if (lane >= off) inc += v; }
    if (lane == QS_WAVE - 1) s_wtot[wave] = inc;
    __syncthreads();
    unsigned int excl = inc - tot;
    for (int w = 0; w < wave; w++) excl += s_wtot[w];
    if (tid < MS_RADIX) s_dig[d] = excl;
    __syncthreads();
    unsigned int run = s_dig[d];
    for (int q = 0; q < seg; q++) run += s_part[q][d];
    for (unsigned int w = w0; w < w1; w++) {
        const unsigned int v = table[(size_t)w * MS_RADIX + d];
        table[(size_t)w * MS_RADIX + d] = run;
        run += v;
    }
}

// FIRST: the pass that reads the keys as they were computed: the input index is the item's position
template <bool FIRST>
__global__ void __launch_bounds__(MS_BLOCK)
qs_sort_scatter_kernel(const unsigned long long *__restrict__ keys_in, const unsigned int *__restrict__ idx_in, size_t n, int shift,
                       size_t per_wg, const unsigned int *__restrict__ table, unsigned long long *__restrict__ keys_out,
                       unsigned int *__restrict__ idx_out)
{
    __shared__ unsigned int s_base[MS_RADIX];             // next slot of every digit for this workgroup
    __shared__ unsigned int s_wc[MS_WAVES][MS_RADIX];     // items of every digit per wave, this round
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    s_base[tid] = table[(size_t)blockIdx.x * MS_RADIX + tid];
    #pragma unroll
    for (int w = 0; w < MS_WAVES; w++) s_wc[w][tid] = 0;
    __syncthreads();
    const size_t lo = (size_t)blockIdx.x * per_wg, hi = (lo + per_wg < n) ? lo + per_wg : n;
    for (size_t base = lo; base < hi; base += MS_BLOCK) {                 // (uniform: every lane takes every round)
        const size_t i = base + tid;
        const bool valid = i < hi;
        const unsigned long long key = valid ? keys_in[i] : 0ull;
        const unsigned int idx = FIRST ? (unsigned int)i : (valid ? idx_in[i] : 0u);
        const unsigned int digit = (unsigned int)(key >> shift) & (MS_RADIX - 1);
        // the wave's lanes that hold an item of my digit
        unsigned long long same = __ballot(valid);
        #pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const unsigned int rank = __popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) s_wc[wave][digit] = __popcll(same);
        __syncthreads();
        if (valid) {
            unsigned int slot = s_base[digit] + rank;
            for (int w = 0; w < wave; w++) slot += s_wc[w][digit];
            if (slot < n) { keys_out[slot] = key; idx_out[slot] = idx; }       // (always; a slot is never taken on trust)
        }
        __syncthreads();
        unsigned int t = 0;
        #pragma unroll
        for (int w = 0; w < MS_WAVES; w++) { t += s_wc[w][tid]; s_wc[w][tid] = 0; }
        s_base[tid] += t;
        __syncthreads();
    }
}

// ---- the means: one lane per voxel, its run in sorted order ------------------------------------------------------------
__global__ void __launch_bounds__(MS_BLOCK)
qs_voxel_sum_kernel(const double2 *__restrict__ pts, const unsigned int *__restrict__ idx, const unsigned int *__restrict__ pos,
                    size_t n_vox, size_t n, double2 *__restrict__ out, size_t cap)
{
    const size_t v = (size_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= n_vox || v >= cap) return;
    const size_t p = pos[v], q = v + 1 < n_vox ? (size_t)pos[v + 1] : n;
    double sx = 0, sy = 0;
    for (size_t k = p; k < q; k++) {
        const unsigned int j = idx[k];
        if (j < n) { const double2 a = pts[j]; sx += a.x; sy += a.y; }         // (always)
    }
    out[v] = make_double2(sx / (double)(q - p), sy / (double)(q - p));
}

// local_pcd.transform(T) on the original points (map_merger.py:58): every product and sum rounded on its own
__global__ void __launch_bounds__(MS_BLOCK)
qs_merge_move_kernel(const double2 *__restrict__ in, size_t n, double t0, double t1, double t2, double t3, double t4, double t5,
                     double2 *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i < n) {
        const double2 p = in[i];
        out[i] = make_double2((t0 * p.x + t1 * p.y) + t2, (t3 * p.x + t4 * p.y) + t5);
    }
}

// ---- workspaces ----------------------------------------------------------------------------------------------------
static unsigned int sort_plan(size_t n, size_t *per_wg)
{
    size_t nwg = (n + 1023) / 1024;
    nwg = nwg < 1 ? 1 : (nwg > MS_MAX_WG ? MS_MAX_WG : nwg);
    size_t per = (n + nwg - 1) / nwg;
    per = (per + MS_BLOCK - 1) / MS_BLOCK * MS_BLOCK;
    if (per < MS_BLOCK) per = MS_BLOCK;
    *per_wg = per;
    return (unsigned int)((n + per - 1) / per);
}
// a map message on its way to a cloud: the grid (host messages only), the compaction's chunk counts, its total, a box
struct QsMergeGridLayout { signed char *grid; unsigned int *chunk; unsigned long long *count, *box4; size_t bytes; };
static QsMergeGridLayout qs_merge_grid_layout(size_t cells, bool with_grid, void *ws)
{
    Carve cv(ws);
    QsMergeGridLayout L;
    L.chunk = cv.take<unsigned int>(qs_compact_chunks(cells));
    L.count = cv.take<unsigned long long>(1);
    L.box4 = cv.take<unsigned long long>(4);
    L.grid = cv.take<signed char>(with_grid ? cells : 0);
    L.bytes = cv.bytes;
    return L;
}
// one callback's clouds (local, the copy the ICP moves, global + moved) and the arrays of a down-sampling of n_cat points
struct QsMergePtsLayout {
    double2 *local, *work, *cat;
    unsigned long long *keys[2], *count, *box4;
    unsigned int *idx[2], *pos, *chunk, *table;
    size_t bytes;
};
static QsMergePtsLayout qs_merge_pts_layout(size_t n_local, size_t n_cat, bool with_cat, void *ws)
{
    Carve cv(ws);
    QsMergePtsLayout L;
    L.local = cv.take<double2>(n_local);
    L.work = cv.take<double2>(n_local);
    L.cat = cv.take<double2>(with_cat ? n_cat : 0);
    for (int q = 0; q < 2; q++) { L.keys[q] = cv.take<unsigned long long>(n_cat); L.idx[q] = cv.take<unsigned int>(n_cat); }
    L.pos = cv.take<unsigned int>(n_cat);
    L.chunk = cv.take<unsigned int>(qs_compact_chunks(n_cat));
    L.table = cv.take<unsigned int>((size_t)MS_MAX_WG * MS_RADIX);
    L.count = cv.take<unsigned long long>(1);
    L.box4 = cv.take<unsigned long long>(4);
    L.bytes = cv.bytes;
    return L;
}
static const size_t MG_WS_FLOOR = (size_t)1 << 16;

// box of n device points, read by the host (four scalars)
static int cloud_box(qs_ctx *c, const double2 *d_xy, size_t n, unsigned long long *d_box4, double box[4])
{
    unsigned long long b[4] = {QS_ORD_MIN_IDENT, QS_ORD_MIN_IDENT, QS_ORD_MAX_IDENT, QS_ORD_MAX_IDENT};
    HIPCHK(c, hipMemcpyAsync(d_box4, b, sizeof b, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_bbox(c, (const double *)d_xy, n, d_box4));
    HIPCHK(c, hipMemcpyAsync(b, d_box4, sizeof b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < 4; q++) box[q] = qs_double_from_ord(b[q]);
    return QS_OK;
}

// bytes of a voxel coordinate that can differ between two points of the cloud: 0 .. vmax
static int bytes_in_use(double vmax)
{
    if (vmax < 256.0) return 1;
    if (vmax < 65536.0) return 2;
    if (vmax < 16777216.0) return 3;
    return 4;                                   // (also what a NaN gets: every byte)
}

// The grouping of n > 0 points (0 < n < 2^31): keys, sort, runs.  Leaves the sorted input indices in L.idx[*which], the runs'
// first positions in L.pos and their number in *n_vox.
static int voxel_group(qs_ctx *c, const double2 *d_pts, size_t n, double voxel, const QsMergePtsLayout &L, int *which, size_t *n_vox,
                       int *passes)
{
    double box[4];
    int rc = cloud_box(c, d_pts, n, L.box4, box);
    if (rc != QS_OK) return rc;
    const double mnx = box[0] - voxel * 0.5, mny = box[1] - voxel * 0.5;       // voxel_min_bound = min_bound - voxel_size / 2
    HIPCHK(c, qs_launch_voxel_keys(c, d_pts, n, mnx, mny, voxel, L.keys[0]));
    // the largest coordinates give the largest voxel indices (the key's expression is monotone), by the kernel's own operations
    const int bx = bytes_in_use(floor((box[2] - mnx) / voxel)), by = bytes_in_use(floor((box[3] - mny) / voxel));
    size_t per_wg;
    const unsigned int nwg = sort_plan(n, &per_wg);
    int cur = 0, np = 0;
    for (int q = 0; q < bx + by; q++) {
        const int shift = q < bx ? 8 * q : 32 + 8 * (q - bx);
        hipLaunchKernelGGL(qs_sort_hist_kernel, dim3(nwg), dim3(MS_BLOCK), 0, c->stream, L.keys[cur], n, shift, per_wg, L.table);
        hipLaunchKernelGGL(qs_sort_scan_kernel, dim3(1), dim3(MS_SCAN_SEGS * MS_RADIX), 0, c->stream, L.table, nwg);
        if (q == 0)
            hipLaunchKernelGGL(qs_sort_scatter_kernel<true>, dim3(nwg), dim3(MS_BLOCK), 0, c->stream, L.keys[cur], L.idx[cur], n, shift, per_wg,
                               L.table, L.keys[cur ^ 1], L.idx[cur ^ 1]);
        else
            hipLaunchKernelGGL(qs_sort_scatter_kernel<false>, dim3(nwg), dim3(MS_BLOCK), 0, c->stream, L.keys[cur], L.idx[cur], n, shift, per_wg,
                               L.table, L.keys[cur ^ 1], L.idx[cur ^ 1]);
        HIPCHK(c, hipGetLastError());
        cur ^= 1; np++;
    }
    HIPCHK(c, qs_launch_run_heads(c, L.keys[cur], n, nullptr, 0, L.count, L.chunk));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, L.count, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, qs_launch_run_heads(c, L.keys[cur], n, L.pos, n, L.count, L.chunk));
    *which = cur; *n_vox = (size_t)total;
    if (passes) *passes = np;
    return QS_OK;
}
static hipError_t voxel_means(qs_ctx *c, const double2 *d_pts, size_t n, const QsMergePtsLayout &L, int which, size_t n_vox, double2 *d_out,
                              size_t cap)
{
    const size_t m = n_vox < cap ? n_vox : cap;
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(qs_voxel_sum_kernel, dim3((unsigned int)((m + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, d_pts,
                       L.idx[which], L.pos, n_vox, n, d_out, cap);
    return hipGetLastError();
}

extern "C" int qs_voxel_downsample_device(qs_ctx *c, const double *d_xy, size_t n, double voxel, double *d_out_xy, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr && voxel > 0);
    *n_out = 0;
    if (n == 0) return QS_OK;
    ARGCHK(c, d_xy != nullptr);
    if (n >= (size_t)1 << 31) return qs_fail(c, QS_E_RANGE, "qs_voxel_downsample_device: 2^31 points or more");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->mg_pts_ws.reserve(qs_merge_pts_layout(0, n, false, nullptr).bytes, c->stream, MG_WS_FLOOR));
    const QsMergePtsLayout L = qs_merge_pts_layout(0, n, false, c->mg_pts_ws.p);
    int which = 0; size_t n_vox = 0;
    int rc = voxel_group(c, (const double2 *)d_xy, n, voxel, L, &which, &n_vox, nullptr);
    if (rc != QS_OK) return rc;
    *n_out = n_vox;
    if (d_out_xy) HIPCHK(c, voxel_means(c, (const double2 *)d_xy, n, L, which, n_vox, (double2 *)d_out_xy, cap));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

// ---- the session -------------------------------------------------------------------------------------------------------
static void result_init(qs_ctx *c, qs_merge_result *r, int status, size_t n_local)
{
    if (!r) return;
    r->status = status; r->iterations = 0;
    r->n_local = n_local; r->n_global = c->mg_n;
    r->fitness = 0; r->rmse = 0;
    for (int q = 0; q < 9; q++) r->T[q] = (q % 4 == 0) ? 1.0 : 0.0;
}

// Where a new global cloud of n points is written: the cloud's own block if it holds them, else a new block `nb` that the
// caller moves into the session once the points are there (a failure on the way leaves the old cloud and its count).
static int cloud_target(qs_ctx *c, size_t n, DevBuf<double2> &nb, double2 **dst)
{
    *dst = c->mg_cloud.p;
    if (n <= c->mg_cloud.cap) return QS_OK;
    size_t cap = c->mg_cloud.cap ? c->mg_cloud.cap : 1024;
    while (cap < n) cap *= 2;
    HIPCHK(c, nb.alloc(cap));
    *dst = nb.p;
    return QS_OK;
}

enum { MG_SRC_HOST = 0, MG_SRC_DEVICE = 1, MG_SRC_STAMPS = 2 };

// one map_callback: `grid` is a host int8 grid, a device int8 grid or a context's stamps
static int merge_callback(qs_ctx *c, int kind, const void *grid, int h, int w, double res, double ox, double oy, qs_merge_result *out)
{
    const size_t cells = (size_t)h * w;
    // 1. the local cloud
    const bool host = kind == MG_SRC_HOST;
    HIPCHK(c, c->mg_grid_ws.reserve(qs_merge_grid_layout(cells, host, nullptr).bytes, c->stream, MG_WS_FLOOR));
    const QsMergeGridLayout G = qs_merge_grid_layout(cells, host, c->mg_grid_ws.p);
    const signed char *d_grid = (const signed char *)grid;
    if (host) { HIPCHK(c, hipMemcpyAsync(G.grid, grid, cells, hipMemcpyHostToDevice, c->stream)); d_grid = G.grid; }
    auto to_pcd = [&](double *d_xy, size_t cap) -> hipError_t {
        return kind == MG_SRC_STAMPS ? qs_launch_stamps_to_pcd(c, (const unsigned int *)grid, h, w, res, ox, oy, d_xy, cap, G.count, G.chunk)
                                     : qs_launch_grid_to_pcd(c, d_grid, h, w, res, ox, oy, d_xy, cap, G.count, G.chunk);
    };
    HIPCHK(c, to_pcd(nullptr, 0));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, G.count, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n_local = (size_t)total;
    if (n_local == 0) { result_init(c, out, QS_MERGE_EMPTY, 0); return QS_OK; }                      // :37-38
    const size_t n_glob = c->mg_n, n_cat = n_glob + n_local;
    if (n_cat >= (size_t)1 << 31) return qs_fail(c, QS_E_RANGE, "map merge: 2^31 points or more");
    HIPCHK(c, c->mg_pts_ws.reserve(qs_merge_pts_layout(n_local, n_cat, true, nullptr).bytes, c->stream, MG_WS_FLOOR));
    const QsMergePtsLayout L = qs_merge_pts_layout(n_local, n_cat, true, c->mg_pts_ws.p);
    HIPCHK(c, to_pcd((double *)L.local, n_local));
    // 2. the first map is the global map                                                              :40-43
    if (n_glob == 0) {
        DevBuf<double2> nb; double2 *dst;
        int rc = cloud_target(c, n_local, nb, &dst);
        if (rc != QS_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(dst, L.local, n_local * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nb.p) c->mg_cloud = std::move(nb);
        c->mg_n = n_local; c->mg_res = res; c->mg_ox = ox; c->mg_oy = oy;
        result_init(c, out, QS_MERGE_ADOPTED, n_local);
        return QS_OK;
    }
    // 3. registration against the global cloud                                                        :45-52
    qs_merge_result r;
    result_init(c, &r, QS_MERGE_REJECTED, n_local);
    HIPCHK(c, hipMemcpyAsync(L.work, L.local, n_local * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    double box[4];
    int rc = cloud_box(c, c->mg_cloud.p, n_glob, L.box4, box);
    if (rc != QS_OK) return rc;
    rc = qs_icp_device(c, L.work, n_local, c->mg_cloud.p, n_glob, box, c->mg_icp_threshold, c->mg_icp_iterations, 1e-6, 1e-6, r.T,
                       &r.fitness, &r.rmse, &r.iterations);
    if (rc != QS_OK) return rc;
    // 4. the gate                                                                                     :54-56
    if (r.fitness < c->mg_min_fitness) { if (out) *out = r; return QS_OK; }
    // 5. transform the original points, append, down-sample                                           :58-60
    HIPCHK(c, hipMemcpyAsync(L.cat, c->mg_cloud.p, n_glob * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(qs_merge_move_kernel, dim3((unsigned int)((n_local + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, L.local,
                       n_local, r.T[0], r.T[1], r.T[2], r.T[3], r.T[4], r.T[5], L.cat + n_glob);
    HIPCHK(c, hipGetLastError());
    int which = 0; size_t n_vox = 0;
    rc = voxel_group(c, L.cat, n_cat, c->mg_res, L, &which, &n_vox, nullptr);
    if (rc != QS_OK) return rc;
    DevBuf<double2> nb; double2 *dst;
    rc = cloud_target(c, n_vox, nb, &dst);        // (the old points are in L.cat by now: the block itself may take the new ones)
    if (rc != QS_OK) return rc;
    HIPCHK(c, voxel_means(c, L.cat, n_cat, L, which, n_vox, dst, n_vox));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nb.p) c->mg_cloud = std::move(nb);
    c->mg_n = n_vox;
    r.status = QS_MERGE_MERGED; r.n_global = n_vox;
    if (out) *out = r;
    return QS_OK;
}

extern "C" int qs_merge_reset(qs_ctx *c)
{
    ARGCHK(c, c != nullptr);
    c->mg_n = 0; c->mg_res = 0.05; c->mg_ox = 0.0; c->mg_oy = 0.0;
    return QS_OK;
}

extern "C" int qs_merge_params(qs_ctx *c, double icp_threshold, int32_t icp_iterations, double min_fitness)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, icp_threshold > 0 && isfinite(icp_threshold) && icp_iterations >= 0 && min_fitness == min_fitness);
    c->mg_icp_threshold = icp_threshold; c->mg_icp_iterations = icp_iterations; c->mg_min_fitness = min_fitness;
    return QS_OK;
}

static bool grid_args_ok(const void *grid, int32_t h, int32_t w, double res, double ox, double oy)
{
    return grid != nullptr && h > 0 && w > 0 && res > 0 && isfinite(res) && isfinite(ox) && isfinite(oy);
}

extern "C" int qs_merge_grid(qs_ctx *c, const int8_t *grid, int32_t h, int32_t w, double res, double ox, double oy, qs_merge_result *out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, grid_args_ok(grid, h, w, res, ox, oy));
    HIPCHK(c, hipSetDevice(c->device));
    return merge_callback(c, MG_SRC_HOST, grid, h, w, res, ox, oy, out);
}

extern "C" int qs_merge_grid_device(qs_ctx *c, const int8_t *d_grid, int32_t h, int32_t w, double res, double ox, double oy,
                                    qs_merge_result *out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, grid_args_ok(d_grid, h, w, res, ox, oy));
    HIPCHK(c, hipSetDevice(c->device));
    return merge_callback(c, MG_SRC_DEVICE, d_grid, h, w, res, ox, oy, out);
}

extern "C" int qs_merge_map(qs_ctx *c, qs_ctx *src, qs_merge_result *out)
{
    ARGCHK(c, c != nullptr && src != nullptr);
    if (src->device != c->device) return qs_fail(c, QS_E_INVAL, "qs_merge_map: the source context is on another device");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_host_state(src, false); if (rcs != QS_OK) return src == c ? rcs : qs_fail(c, rcs, src->err.c_str()); }
    if (src != c) HIPCHK(c, hipStreamSynchronize(src->stream));          // its map as its stream leaves it
    return merge_callback(c, MG_SRC_STAMPS, src->d_stamps.p, src->cfg.size, src->cfg.size, src->cfg.res, src->cfg.ox, src->cfg.oy, out);
}

extern "C" int qs_merge_cloud(qs_ctx *c, double *xy, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr);
    *n_out = c->mg_n;
    const size_t m = c->mg_n < cap ? c->mg_n : cap;
    if (!xy || m == 0) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(xy, c->mg_cloud.p, m * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_merge_global_map(qs_ctx *c, int32_t dims[2], double origin[2], int8_t *grid)
{
    ARGCHK(c, c != nullptr && dims && origin);
    if (c->mg_n == 0) { dims[0] = dims[1] = 0; return QS_OK; }      // publish_global_map returns early  :88-93
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> dbox; DevBuf<signed char> dg;
    HIPCHK(c, dbox.alloc(4));
    double box[4];
    int rc = cloud_box(c, c->mg_cloud.p, c->mg_n, dbox.p, box);
    if (rc != QS_OK) return rc;
    const double wd = ceil((box[2] - box[0]) / c->mg_res), hd = ceil((box[3] - box[1]) / c->mg_res);     // :103-104
    if (!(wd >= 0 && wd < 65536 && hd >= 0 && hd < 65536)) return qs_fail(c, QS_E_RANGE, "qs_merge_global_map: canvas too large");
    const int w = (int)wd + 1, h = (int)hd + 1;
    dims[0] = h; dims[1] = w; origin[0] = box[0]; origin[1] = box[1];
    if (!grid) return QS_OK;
    HIPCHK(c, dg.alloc((size_t)h * w));
    HIPCHK(c, qs_launch_rasterise(c, (const double *)c->mg_cloud.p, c->mg_n, c->mg_res, box[0], box[1], h, w, dg.p));
    HIPCHK(c, hipMemcpyAsync(grid, dg.p, (size_t)h * w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}
