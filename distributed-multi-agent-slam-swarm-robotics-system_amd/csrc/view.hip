// view.hip -- the mission-control map view (MapRenderer, dual_bot_mapper.py:380-668) rendered on the device at any zoom:
// rules R0-R5 of include/quasar_slam.h ("map view").  Only the frame leaves the GPU.
//
// Passes of one call, all on the context's stream:
//   index      R0 is separable and monotone (x: non-decreasing in gx, y: non-increasing in gy; every operation of the
//              expression rounds monotonically), so the cells that can touch a frame column are one range [first, last] of
//              gx, and the same for rows: one thread per column / row finds the range by a binary search that evaluates R0's
//              own expression at the candidates (R0 is never inverted).  Minified views also get xmap[gx] = the cell's frame
//              column (-1: none).
//   occupancy  two state bits per pixel (1: a FREE cell in the footprint, 2: an OCCUPIED one) into a byte frame.
//              minified (cell_px < 2, the hot pass): a workgroup owns VW_PXT pixels of one frame row and streams the cells of
//              its footprint, every stamp once, 16 bytes per lane as grid_ops.hip does; a lane keeps its four columns over all
//              rows of the footprint in registers, then ORs them into the workgroup's pixels in LDS.
//              magnified (cell_px >= 2): a gather, one lane per pixel over the (at most 2 x 2) cells of its two ranges.
//   prims      R5: one wave per primitive scatters atomicMax(owner[pixel], index + 1): whatever the schedule, the highest
//              index that covers a pixel wins, as in the stamp grid.
//   compose    R1, R2, R3 (from the state bits), R4 (a loop over the zones' rectangles) and R5 (the owner's colour) in one
//              pass per pixel: no atomics, one 4-byte store.
// The rectangles of R4 and the columns / rows of R2 are R0 on a handful of values: the host evaluates them (this file is
// compiled with -ffp-contract=off for the host too) and uploads them with the primitives.
#include <math.h>
#include <string.h>

#include "qs_internal.h"

#define VW_BLOCK 256
#define VW_PXT 256                     // pixels of one frame row per workgroup of the minified pass
#define VW_LIMIT 1073741824.0          // R0: |value| <= 2^30 or the point is not drawn
#define VW_KEY_LOW (-(1ll << 62))      // search keys of cells R0 does not draw: below / above every pixel
#define VW_KEY_HIGH (1ll << 62)

struct ViewK {
    int w, h, size;
    double res, ox, oy, scale, offx, offy;
    int ax, bx, ay, by;                // a cell whose screen point is (sx, sy) touches pixel (px, py) when px + ax <= sx <= px + bx
                                       // and py + ay <= sy <= py + by: (0, 0) for points, (half - cell_px + 1, half) for squares
    unsigned int bg, line, free_, occ; // 0xffBBGGRR: the bytes R, G, B, 255 of a pixel
    int draw_occ;
};
struct ViewRect { int x0, y0, x1, y1; unsigned int color, pad; };      // R4: [x0, x1) x [y0, y1), clamped to one pixel round the frame

// R0 for one axis: off + w * scale (x) or off - w * scale (y), two roundings; false = not drawn
__host__ __device__ inline bool vw_r0(double off, double scale, double wv, bool neg, int &out)
{
    const double t = wv * scale;
    const double v = neg ? off - t : off + t;
    if (!(fabs(v) <= VW_LIMIT)) return false;
    out = (int)v;                      // truncation toward zero: pixel 0 takes (-1, 1)
    return true;
}
// screen coordinate of cell gi's centre o + (gi + 0.5) * res as a search key
__device__ inline long long vw_key(double off, double scale, double o, double res, int gi, bool neg)
{
    const double wv = o + ((double)gi + 0.5) * res;
    const double t = wv * scale;
    const double v = neg ? off - t : off + t;
    if (!(fabs(v) <= VW_LIMIT)) return v < 0.0 ? VW_KEY_LOW : VW_KEY_HIGH;
    return (long long)(int)v;
}
// first gi in [0, size] whose key is >= a (x axis, keys non-decreasing)
__device__ inline int vw_first_ge(const ViewK &k, long long a)
{
    int lo = 0, hi = k.size;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (vw_key(k.offx, k.scale, k.ox, k.res, mid, false) >= a) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// first gi in [0, size] whose key is <= b (y axis, keys non-increasing)
__device__ inline int vw_first_le(const ViewK &k, long long b)
{
    int lo = 0, hi = k.size;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (vw_key(k.offy, k.scale, k.oy, k.res, mid, true) <= b) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- index: colr[px] / rowr[py] = {first, last} cell of the footprint (last < first: empty); xmap (minified views) ------
__global__ void __launch_bounds__(VW_BLOCK)
qs_view_index_kernel(ViewK k, int2 *__restrict__ colr, int2 *__restrict__ rowr, int *__restrict__ xmap)
{
    const int t = blockIdx.x * VW_BLOCK + threadIdx.x;
    if (t < k.w) {
        colr[t] = make_int2(vw_first_ge(k, (long long)t + k.ax), vw_first_ge(k, (long long)t + k.bx + 1) - 1);
    } else if (t < k.w + k.h) {
        const int py = t - k.w;
        rowr[py] = make_int2(vw_first_le(k, (long long)py + k.by), vw_first_le(k, (long long)py + k.ay - 1) - 1);
    } else if (xmap && t < k.w + k.h + k.size) {
        const int gx = t - k.w - k.h;
        const long long key = vw_key(k.offx, k.scale, k.ox, k.res, gx, false);
        xmap[gx] = (key >= 0 && key < k.w) ? (int)key : -1;
    }
}

__device__ inline unsigned int vw_bits(unsigned int s) { return s == 0u ? 0u : ((s & 1u) ? 2u : 1u); }

// ---- occupancy, minified: workgroup (bx, py) owns pixels [bx * VW_PXT, ...) of frame row py ---------------------------------
__global__ void __launch_bounds__(VW_BLOCK)
qs_view_minify_kernel(ViewK k, const uint4 *__restrict__ stamps4, const int2 *__restrict__ colr, const int2 *__restrict__ rowr,
                      const int4 *__restrict__ xmap4, unsigned char *__restrict__ state)
{
    __shared__ unsigned int s_acc[VW_PXT];
    const int py = blockIdx.y, px0 = blockIdx.x * VW_PXT;
    const int npx = min(VW_PXT, k.w - px0);
    s_acc[threadIdx.x] = 0u;
    __syncthreads();
    const int2 yr = rowr[py];
    const int glo = colr[px0].x, ghi = colr[px0 + npx - 1].y;          // the cells of the workgroup's pixels: one span of columns
    if (yr.y >= yr.x && ghi >= glo) {
        const size_t row4 = (size_t)(k.size >> 2);                     // size is a multiple of 4 (qs_create): rows are 16-byte aligned
        for (int v = (glo >> 2) + (int)threadIdx.x; v <= (ghi >> 2); v += VW_BLOCK) {
            const int4 xm = xmap4[v];
            // the cells of a 16-byte group beyond the span belong to a neighbour's pixels (or to none): unsigned compare drops them
            const unsigned int p0 = (unsigned int)(xm.x - px0), p1 = (unsigned int)(xm.y - px0);
            const unsigned int p2 = (unsigned int)(xm.z - px0), p3 = (unsigned int)(xm.w - px0);
            unsigned int b0 = 0u, b1 = 0u, b2 = 0u, b3 = 0u;
            const uint4 *col = stamps4 + (size_t)yr.x * row4 + v;
            #pragma unroll 4
            for (int r = yr.x; r <= yr.y; r++, col += row4) {
                const uint4 s = *col;
                b0 |= vw_bits(s.x); b1 |= vw_bits(s.y); b2 |= vw_bits(s.z); b3 |= vw_bits(s.w);
            }
            // neighbouring cells mostly share a pixel: fold equal targets before the LDS atomics
            if (p1 == p0) { b0 |= b1; b1 = 0u; }
            if (p3 == p2) { b2 |= b3; b3 = 0u; }
            if (p2 == p0) { b0 |= b2; b2 = 0u; }
            if (b0 && p0 < (unsigned int)npx) atomicOr(&s_acc[p0], b0);
            if (b1 && p1 < (unsigned int)npx) atomicOr(&s_acc[p1], b1);
            if (b2 && p2 < (unsigned int)npx) atomicOr(&s_acc[p2], b2);
            if (b3 && p3 < (unsigned int)npx) atomicOr(&s_acc[p3], b3);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < npx) state[(size_t)py * k.w + px0 + threadIdx.x] = (unsigned char)s_acc[threadIdx.x];
}

// ---- occupancy, magnified: one lane per pixel over the cells of its two ranges ---------------------------------------------
__global__ void __launch_bounds__(VW_BLOCK)
qs_view_gather_kernel(ViewK k, const unsigned int *__restrict__ stamps, const int2 *__restrict__ colr, const int2 *__restrict__ rowr,
                      unsigned char *__restrict__ state)
{
    const int px = blockIdx.x * VW_BLOCK + threadIdx.x, py = blockIdx.y;
    if (px >= k.w) return;
    const int2 xr = colr[px], yr = rowr[py];
    unsigned int b = 0u;
    for (int gy = yr.x; gy <= yr.y; gy++)
        for (int gx = xr.x; gx <= xr.y; gx++) b |= vw_bits(stamps[(size_t)gy * k.size + gx]);
    state[(size_t)py * k.w + px] = (unsigned char)b;
}

// ---- R5: one wave per primitive ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VW_BLOCK)
qs_view_prims_kernel(ViewK k, const qs_view_prim *__restrict__ prims, unsigned int n, unsigned int *__restrict__ owner)
{
    const unsigned int wave = (blockIdx.x * VW_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= n) return;
    const qs_view_prim p = prims[wave];
    const unsigned int tag = wave + 1u;
    int sx, sy;
    if (!vw_r0(k.offx, k.scale, p.x0, false, sx) || !vw_r0(k.offy, k.scale, p.y0, true, sy)) return;
    if (p.kind == QS_VIEW_POINT) {
        if (lane == 0 && sx >= 0 && sx < k.w && sy >= 0 && sy < k.h) atomicMax(&owner[(size_t)sy * k.w + sx], tag);
    } else if (p.kind == QS_VIEW_SQUARE) {
        const int xa = max(sx - p.size / 2, 0), xb = min(sx - p.size / 2 + p.size, k.w);
        const int ya = max(sy - p.size / 2, 0), yb = min(sy - p.size / 2 + p.size, k.h);
        if (xb <= xa || yb <= ya) return;
        const int cw = xb - xa, cnt = cw * (yb - ya);                 // <= 64 * 64
        for (int i = lane; i < cnt; i += 64) atomicMax(&owner[(size_t)(ya + i / cw) * k.w + xa + i % cw], tag);
    } else {
        int ex, ey;
        if (!vw_r0(k.offx, k.scale, p.x1, false, ex) || !vw_r0(k.offy, k.scale, p.y1, true, ey)) return;
        // closed form of _bresenham (:158-179): cell j has major offset j and minor offset (2 j m + M - 1) / (2 M).
        // |coordinates| <= 2^30: M, m <= 2^31 and 2 j m + M - 1 < 2^64
        const long long dx = llabs((long long)ex - sx), dy = llabs((long long)ey - sy);
        const bool xmaj = dx >= dy;
        const long long M = xmaj ? dx : dy, m = xmaj ? dy : dx;
        const long long a0 = xmaj ? sx : sy, a1 = xmaj ? ex : ey, lim = xmaj ? k.w : k.h;
        // j clipped to the frame along the major axis: at most `lim` cells, however long the segment
        long long jlo, jhi;
        if (a0 <= a1) { jlo = max(0ll, -a0); jhi = min(M, lim - 1 - a0); }
        else { jlo = max(0ll, a0 - (lim - 1)); jhi = min(M, a0); }
        const int smaj = a0 <= a1 ? 1 : -1;
        const int smin = xmaj ? (sy < ey ? 1 : -1) : (sx < ex ? 1 : -1);
        const long long b0 = xmaj ? sy : sx, blim = xmaj ? k.h : k.w;
        for (long long j = jlo + lane; j <= jhi; j += 64) {
            const long long mo = M ? (long long)((2ull * (unsigned long long)j * (unsigned long long)m + (unsigned long long)M - 1ull) /
                                                 (2ull * (unsigned long long)M)) : 0ll;
            const long long a = a0 + smaj * j, b = b0 + smin * mo;
            if (b < 0 || b >= blim) continue;
            const long long x = xmaj ? a : b, y = xmaj ? b : a;
            atomicMax(&owner[(size_t)y * k.w + (size_t)x], tag);
        }
    }
}

// ---- compose: R1-R5 of one pixel ------------------------------------------------------------------------------------------------
__device__ inline unsigned int vw_blend(unsigned int c, unsigned int dst)      // (c * 25 + dst * 230 + 127) / 255 per channel
{
    unsigned int out = 0xff000000u;
    #pragma unroll
    for (int sh = 0; sh < 24; sh += 8) out |= ((((c >> sh) & 255u) * 25u + ((dst >> sh) & 255u) * 230u + 127u) / 255u) << sh;
    return out;
}
__global__ void __launch_bounds__(VW_BLOCK)
qs_view_compose_kernel(ViewK k, const unsigned char *__restrict__ state, const unsigned char *__restrict__ col_line,
                       const unsigned char *__restrict__ row_line, const ViewRect *__restrict__ rects, int n_rects,
                       const unsigned int *__restrict__ owner, const qs_view_prim *__restrict__ prims, unsigned int *__restrict__ out)
{
    const int px = blockIdx.x * VW_BLOCK + threadIdx.x, py = blockIdx.y;
    if (px >= k.w) return;
    const size_t idx = (size_t)py * k.w + px;
    unsigned int c = (col_line[px] | row_line[py]) ? k.line : k.bg;                       // R1, R2
    const unsigned int st = state ? state[idx] : 0u;                                      // R3
    if (k.draw_occ && (st & 2u)) c = k.occ; else if (st & 1u) c = k.free_;
    for (int z = 0; z < n_rects; z++) {                                                   // R4 (the index is wave-uniform)
        const ViewRect r = rects[z];
        if (px >= r.x0 && px < r.x1 && py >= r.y0 && py < r.y1)
            c = (px == r.x0 || px == r.x1 - 1 || py == r.y0 || py == r.y1 - 1) ? r.color : vw_blend(r.color, c);
    }
    const unsigned int own = owner ? owner[idx] : 0u;                                     // R5
    if (own) {
        const uint8_t *pc = prims[own - 1].color;
        c = 0xff000000u | pc[0] | ((unsigned int)pc[1] << 8) | ((unsigned int)pc[2] << 16);
    }
    out[idx] = c;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the one layout of qs_ctx::view_ws
struct QsViewLayout {
    unsigned char *state; unsigned int *owner; int2 *colr, *rowr; int *xmap; unsigned char *tables; qs_view_prim *prims;
    unsigned int *frame; size_t bytes;
};
static size_t vw_tables_bytes(int w, int h, size_t n_rects) { return (((size_t)w + h + 15) & ~(size_t)15) + n_rects * sizeof(ViewRect); }
static QsViewLayout qs_view_layout(int w, int h, int size, size_t n_rects, size_t n_prims, bool host_frame, void *ws)
{
    Carve cv(ws);
    QsViewLayout L{};
    const size_t px = (size_t)w * h;
    L.state = cv.take<unsigned char>(px);
    L.owner = cv.take<unsigned int>(n_prims ? px : 0);
    L.colr = cv.take<int2>(w);
    L.rowr = cv.take<int2>(h);
    L.xmap = cv.take<int>(size);
    L.tables = cv.take<unsigned char>(vw_tables_bytes(w, h, n_rects));   // col_line [w], row_line [h], padding, rects [n_rects]
    L.prims = cv.take<qs_view_prim>(n_prims);
    L.frame = cv.take<unsigned int>(host_frame ? px : 0);
    L.bytes = cv.bytes;
    return L;
}
static const size_t VW_WS_FLOOR = (size_t)1 << 20;

static unsigned int vw_rgb(const uint8_t c[4]) { return 0xff000000u | c[0] | ((unsigned int)c[1] << 8) | ((unsigned int)c[2] << 16); }

static int view_render(qs_ctx *c, const qs_view_params *p, const qs_view_zone *zones, size_t n_zones, const qs_view_prim *prims,
                       size_t n_prims, uint8_t *d_rgba, uint8_t *rgba_host)
{
    ARGCHK(c, c != nullptr && p != nullptr && (d_rgba != nullptr || rgba_host != nullptr));
    ARGCHK(c, p->width >= 1 && p->width <= QS_VIEW_MAX_DIM && p->height >= 1 && p->height <= QS_VIEW_MAX_DIM);
    ARGCHK(c, isfinite(p->scale) && p->scale > 0.0 && isfinite(p->offset_x) && isfinite(p->offset_y));
    ARGCHK(c, (long long)p->line_max - p->line_min < QS_VIEW_MAX_LINES);           // (line_max < line_min: no lines)
    ARGCHK(c, n_zones <= QS_VIEW_MAX_ZONES && (n_zones == 0 || zones != nullptr));
    ARGCHK(c, n_prims <= QS_VIEW_MAX_PRIMS && (n_prims == 0 || prims != nullptr));
    for (size_t i = 0; i < n_prims; i++) {
        const qs_view_prim &q = prims[i];
        if (q.kind < QS_VIEW_POINT || q.kind > QS_VIEW_SEGMENT) return qs_fail(c, QS_E_INVAL, "qs_render_view: unknown primitive kind");
        if (q.kind == QS_VIEW_SQUARE && (q.size < 1 || q.size > QS_VIEW_MAX_SQUARE))
            return qs_fail(c, QS_E_INVAL, "qs_render_view: a square's size is 1..64");
    }
    const double cell_scale = c->cfg.res * p->scale;
    if (!(cell_scale <= (double)QS_VIEW_MAX_CELL_PX)) return qs_fail(c, QS_E_INVAL, "qs_render_view: res * scale is beyond 2^20 pixels per cell");
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);

    const int W = p->width, H = p->height, size = c->cfg.size;
    const int cell_px = (int)cell_scale < 1 ? 1 : (int)cell_scale;                  // max(1, int(res * scale))  :494
    const int mode = cell_px >= 2 ? 2 : (p->minify ? 1 : 0);                        // gather, minified, nothing (:495-496)
    ViewK k{};
    k.w = W; k.h = H; k.size = size;
    k.res = c->cfg.res; k.ox = c->cfg.ox; k.oy = c->cfg.oy; k.scale = p->scale; k.offx = p->offset_x; k.offy = p->offset_y;
    if (cell_px >= 3) { k.bx = k.by = cell_px / 2; k.ax = k.ay = cell_px / 2 - cell_px + 1; }
    k.bg = vw_rgb(p->bg); k.line = vw_rgb(p->line); k.free_ = vw_rgb(p->free); k.occ = vw_rgb(p->occ);
    k.draw_occ = p->draw_occupied != 0;

    // R2 and R4 on the host: line columns / rows, and the zones' rectangles in array order
    std::vector<ViewRect> rects;
    rects.reserve(n_zones);
    for (size_t i = 0; i < n_zones; i++) {
        const qs_view_zone &z = zones[i];
        int sx1, sy1, sx2, sy2;
        if (!vw_r0(k.offx, k.scale, z.minx, false, sx1) || !vw_r0(k.offy, k.scale, z.maxy, true, sy1) ||
            !vw_r0(k.offx, k.scale, z.maxx, false, sx2) || !vw_r0(k.offy, k.scale, z.miny, true, sy2)) continue;
        if (!(sx2 > sx1 && sy2 > sy1)) continue;                                    // w > 0 and h > 0  :547
        if (sx2 <= 0 || sy2 <= 0 || sx1 >= W || sy1 >= H) continue;                 // nothing of it in the frame
        // an edge one pixel outside the frame is as invisible as one further out
        rects.push_back(ViewRect{sx1 < -1 ? -1 : sx1, sy1 < -1 ? -1 : sy1, sx2 > W + 1 ? W + 1 : sx2, sy2 > H + 1 ? H + 1 : sy2,
                                 vw_rgb(z.color), 0u});
    }
    const size_t tab_bytes = vw_tables_bytes(W, H, rects.size()), rect_off = tab_bytes - rects.size() * sizeof(ViewRect);
    std::vector<unsigned char> tables(tab_bytes, 0);
    for (long long v = p->line_min; v <= p->line_max; v++) {                        // :479-485
        int s;
        if (vw_r0(k.offx, k.scale, (double)v, false, s) && s >= 0 && s < W) tables[s] = 1;
        if (vw_r0(k.offy, k.scale, (double)v, true, s) && s >= 0 && s < H) tables[W + s] = 1;
    }
    if (!rects.empty()) memcpy(tables.data() + rect_off, rects.data(), rects.size() * sizeof(ViewRect));

    const bool host = rgba_host != nullptr;
    HIPCHK(c, c->view_ws.reserve(qs_view_layout(W, H, size, rects.size(), n_prims, host, nullptr).bytes, c->stream, VW_WS_FLOOR));
    const QsViewLayout L = qs_view_layout(W, H, size, rects.size(), n_prims, host, c->view_ws.p);
    HIPCHK(c, hipMemcpyAsync(L.tables, tables.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    if (n_prims) HIPCHK(c, hipMemcpyAsync(L.prims, prims, n_prims * sizeof(qs_view_prim), hipMemcpyHostToDevice, c->stream));

    const dim3 pix((W + VW_BLOCK - 1) / VW_BLOCK, H);
    if (mode) {
        const int n_idx = W + H + (mode == 1 ? size : 0);
        hipLaunchKernelGGL(qs_view_index_kernel, dim3((n_idx + VW_BLOCK - 1) / VW_BLOCK), dim3(VW_BLOCK), 0, c->stream, k, L.colr, L.rowr,
                           mode == 1 ? L.xmap : nullptr);
        if (mode == 1)
            hipLaunchKernelGGL(qs_view_minify_kernel, dim3((W + VW_PXT - 1) / VW_PXT, H), dim3(VW_BLOCK), 0, c->stream, k,
                               (const uint4 *)c->d_stamps.p, L.colr, L.rowr, (const int4 *)L.xmap, L.state);
        else
            hipLaunchKernelGGL(qs_view_gather_kernel, pix, dim3(VW_BLOCK), 0, c->stream, k, c->d_stamps.p, L.colr, L.rowr, L.state);
    }
    if (n_prims) {
        HIPCHK(c, hipMemsetAsync(L.owner, 0, (size_t)W * H * sizeof(unsigned int), c->stream));
        hipLaunchKernelGGL(qs_view_prims_kernel, dim3((unsigned int)((n_prims * 64 + VW_BLOCK - 1) / VW_BLOCK)), dim3(VW_BLOCK), 0, c->stream,
                           k, L.prims, (unsigned int)n_prims, L.owner);
    }
    unsigned int *d_out = host ? L.frame : (unsigned int *)d_rgba;
    hipLaunchKernelGGL(qs_view_compose_kernel, pix, dim3(VW_BLOCK), 0, c->stream, k, mode ? L.state : nullptr, L.tables, L.tables + W,
                       (const ViewRect *)(L.tables + rect_off), (int)rects.size(), n_prims ? L.owner : nullptr, L.prims, d_out);
    HIPCHK(c, hipGetLastError());
    if (host) {
        HIPCHK(c, hipMemcpyAsync(rgba_host, L.frame, (size_t)W * H * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return QS_OK;
}

// ---- C ABI: map view ------------------------------------------------------------------------------------------------------------
extern "C" int qs_render_view(qs_ctx *c, const qs_view_params *params, const qs_view_zone *zones, size_t n_zones,
                              const qs_view_prim *prims, size_t n_prims, uint8_t *rgba_host)
{
    ARGCHK(c, c != nullptr && rgba_host != nullptr);
    return view_render(c, params, zones, n_zones, prims, n_prims, nullptr, rgba_host);
}

extern "C" int qs_render_view_device(qs_ctx *c, const qs_view_params *params, const qs_view_zone *zones, size_t n_zones,
                                     const qs_view_prim *prims, size_t n_prims, uint8_t *d_rgba)
{
    ARGCHK(c, c != nullptr && d_rgba != nullptr);
    return view_render(c, params, zones, n_zones, prims, n_prims, d_rgba, nullptr);
}
