// plan.hip -- shortest paths over the mapped free space and TARG waypoints.
// The reference has no planner; the rules are this build's own (include/quasar_slam.h, "path planning"), all integer.
//
//   traversability : one workgroup per 64x64 tile reads the stamps of the tile and a halo of `clearance` cells into LDS
//                    and dilates the OCCUPIED cells by an exact Euclidean disc in two passes: per row the distance to
//                    the nearest OCCUPIED cell (capped at clearance + 1), then per column min over dy of dy^2 + rowdist^2.
//                    The result is a bit mask (one ballot per row of a tile) plus, per tile, whether it holds any
//                    traversable cell and the tile-aligned bounding box of those tiles (the census);
//   endpoints      : one wave per start / goal: world_to_grid, then the nearest traversable cell within snap_radius by
//                    (dx^2 + dy^2, gy * size + gx), one candidate per lane and a 64-bit key reduced across the wave;
//   fields         : one field per request over the bounding box, requests in groups that fit QS_PLAN_WS_CAP.  Rounds
//                    over a worklist of (field, tile) items, one launch per round: a workgroup loads the tile and its
//                    one-cell halo, relaxes the tile in LDS by segmented min-plus scans along rows, columns and both
//                    diagonals (both ways) until nothing changes, writes it back and appends the neighbours of every
//                    improved border to the next round's list (a per-item round mark keeps each item in a list once).
//                    The shortest-path fixpoint is unique, so the order of relaxation does not change a bit of it;
//   walk           : one wave per request: lanes 0..7 test the eight moves of the present cell in the header's order,
//                    the path cells are written as they come, and 64 of them at a time are tested for visibility
//                    (each lane walks the reference's Bresenham line from the start to its cell over the mask).
// There are no device-side waits and no grid-wide barriers: a round that finds its list empty returns at once.
#include <string.h>
#include <algorithm>

#include "plan_common.h"
#include "raycast_common.h"

static_assert(PL_T == QS_WAVE, "one lane per cell of a tile row");

// ---- traversability + census ------------------------------------------------------------------------------------
// state bytes in LDS: 0 UNKNOWN (or outside the grid), 1 FREE, 2 OCCUPIED (frontier.hip's reading of a stamp)
__global__ void __launch_bounds__(PL_BLOCK)
qs_plan_trav_kernel(const unsigned int *__restrict__ stamps, int size, int clr, int mp, unsigned int *__restrict__ mask,
                    unsigned int *__restrict__ tile_any, unsigned int *__restrict__ bbox)
{
    __shared__ unsigned char s_st[PL_R * PL_R];
    __shared__ unsigned char s_rd[PL_R * PL_T];
    __shared__ unsigned int s_any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = blockIdx.x, ty = blockIdx.y, x0 = tx * PL_T, y0 = ty * PL_T;
    const int R = PL_T + 2 * clr;
    if (tid == 0) s_any = 0;
    for (int i = tid; i < R * R; i += PL_BLOCK) {
        const int gx = x0 - clr + i % R, gy = y0 - clr + i / R;
        unsigned char v = 0;
        if (gx >= 0 && gx < size && gy >= 0 && gy < size) {
            const unsigned int s = stamps[(size_t)gy * size + gx];
            v = s == 0 ? 0 : ((s & 1u) ? 2 : 1);
        }
        s_st[i] = v;
    }
    __syncthreads();
    // row pass: distance from column x (of the tile) to the nearest OCCUPIED cell of region row r, capped at clr + 1
    for (int i = tid; i < R * PL_T; i += PL_BLOCK) {
        const int r = i / PL_T, x = i % PL_T;
        const unsigned char *row = s_st + r * R + x;        // row[clr] is the cell itself
        int d = clr + 1;
        for (int k = 0; k <= 2 * clr; k++)
            if (row[k] == 2) d = min(d, abs(k - clr));
        s_rd[i] = (unsigned char)d;
    }
    __syncthreads();
    // column pass: a FREE cell is traversable when no dy^2 + rowdist^2 <= clr^2; one ballot per tile row
    bool any = false;
    for (int y = wave; y < PL_T; y += PL_BLOCK / QS_WAVE) {
        bool ok = s_st[(y + clr) * R + lane + clr] == 1;
        for (int dy = -clr; dy <= clr && ok; dy++) {
            const int d = s_rd[(y + clr + dy) * PL_T + lane];
            if (d <= clr && dy * dy + d * d <= clr * clr) ok = false;
        }
        const unsigned long long m = __ballot(ok);
        any |= m != 0;
        if (lane < 2) mask[(size_t)(y0 + y) * mp + tx * 2 + lane] = (unsigned int)(m >> (32 * lane));
    }
    if (any && lane == 0) s_any = 1;
    __syncthreads();
    if (tid == 0) {
        tile_any[(size_t)ty * gridDim.x + tx] = s_any;
        if (s_any) {
            atomicMin(&bbox[0], (unsigned int)tx); atomicMin(&bbox[1], (unsigned int)ty);
            atomicMax(&bbox[2], (unsigned int)tx); atomicMax(&bbox[3], (unsigned int)ty);
        }
    }
}

__device__ inline bool pl_trav(const unsigned int *mask, int mp, int size, int gx, int gy)
{
    if (gx < 0 || gy < 0 || gx >= size || gy >= size) return false;
    return (mask[(size_t)gy * mp + (gx >> 5)] >> (gx & 31)) & 1u;
}

// ---- endpoints: world_to_grid, then the snap --------------------------------------------------------------------
// one wave per endpoint e (2 * n of them: starts, then goals); cell[e] = gy * size + gx or -1; *snapped counts snaps
__global__ void __launch_bounds__(PL_BLOCK)
qs_plan_snap_kernel(const double2 *__restrict__ xy, int n_end, double res, double ox, double oy, int size,
                    const unsigned int *__restrict__ mask, int mp, int radius, long long *__restrict__ cell,
                    unsigned long long *__restrict__ snapped)
{
    const int lane = threadIdx.x & 63, e = blockIdx.x * (PL_BLOCK / QS_WAVE) + (threadIdx.x >> 6);
    if (e >= n_end) return;                               // whole waves
    const double2 p = xy[e];
    const long long gx = qs_w2g_ll(p.x, ox, res), gy = qs_w2g_ll(p.y, oy, res);   // QS_LL_BAD for NaN / inf / far
    long long out = -1;
    if (gx != QS_LL_BAD && gy != QS_LL_BAD && gx >= 0 && gy >= 0 && gx < size && gy < size) {
        if (pl_trav(mask, mp, size, (int)gx, (int)gy)) {
            out = gy * size + gx;
        } else {
            const int w = 2 * radius + 1;
            unsigned long long best = ~0ull;
            for (int k = lane; k < w * w; k += QS_WAVE) {
                const int dx = k % w - radius, dy = k / w - radius;
                const int cx = (int)gx + dx, cy = (int)gy + dy;
                if (dx * dx + dy * dy <= radius * radius && pl_trav(mask, mp, size, cx, cy)) {
                    const unsigned long long key = ((unsigned long long)(dx * dx + dy * dy) << 32) |
                                                   (unsigned long long)((long long)cy * size + cx);
                    best = key < best ? key : best;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(best, off);
                best = o < best ? o : best;
            }
            if (best != ~0ull) {
                out = (long long)(best & 0xffffffffull);
                if (lane == 0) atomicAdd(snapped, 1ull);
            }
        }
    }
    if (lane == 0) cell[e] = out;
}

// ---- fields ----------------------------------------------------------------------------------------------------
// seed: field[goal] = 0 and the goal's tile in the first list (round 1: list 1, count 1 of the ring, mark 1).  A round
// appends a neighbour tile when a border cell of the tile IMPROVED, and the seed cell itself never does: a goal on a tile's
// border row or column (or corner) also puts the tiles across that border in the first list, or a goal whose only moves
// lead across the border would never leave its tile.  They read the seed through their halo.
__global__ void __launch_bounds__(PL_BLOCK)
qs_plan_seed_kernel(const long long *__restrict__ start, const long long *__restrict__ goal, int g0, int gn, int size,
                    PlBox B, size_t fcells, const unsigned int *__restrict__ tile_any, int gtx,
                    unsigned int *__restrict__ fields, unsigned int *__restrict__ list, unsigned int *__restrict__ cnt,
                    unsigned int *__restrict__ marks)
{
    const int f = blockIdx.x * PL_BLOCK + threadIdx.x;
    if (f >= gn) return;
    const long long s = start[g0 + f], g = goal[g0 + f];
    if (s < 0 || g < 0) return;
    const int fx = (int)(g % size) - B.bx0 * PL_T, fy = (int)(g / size) - B.by0 * PL_T;
    fields[(size_t)f * fcells + (size_t)fy * B.fw + fx] = 0;
    const int tx = fx / PL_T, ty = fy / PL_T;
    const int ex = fx % PL_T == 0 ? -1 : (fx % PL_T == PL_T - 1 ? 1 : 0), ey = fy % PL_T == 0 ? -1 : (fy % PL_T == PL_T - 1 ? 1 : 0);
    for (int k = 0; k < 4; k++) {                           // the tile, then those across x, across y, across the corner
        const int nx = tx + ((k & 1) ? ex : 0), ny = ty + ((k & 2) ? ey : 0);
        if (((k & 1) && !ex) || ((k & 2) && !ey)) continue;
        if (nx < 0 || ny < 0 || nx >= B.ntx || ny >= B.nty || !tile_any[(size_t)(B.by0 + ny) * gtx + B.bx0 + nx]) continue;
        const unsigned int item = (unsigned int)f * (B.ntx * B.nty) + ny * B.ntx + nx;
        marks[item] = 1;
        list[atomicAdd(&cnt[1], 1u)] = item;
    }
}

// The key a field holds: the uint32 cost (path planning), or the 64-bit (cost << 32) | bot of a multi-seeded field
// (territory.hip), whose minimum orders by cost first, then by bot.  A step adds w << shift.
template <typename K> struct PlKey;
template <> struct PlKey<unsigned int> { static constexpr unsigned int inf = PL_INF; static constexpr int shift = 0; };
template <> struct PlKey<unsigned long long> { static constexpr unsigned long long inf = ~0ull; static constexpr int shift = 32; };

// min-plus scan with step weight w along the 64 lanes of a line, in lane order: v[x] = min over k <= x of the same
// segment of v[k] + w (x - k); a segment starts at a lane whose move from the lane before is not allowed (!e)
template <typename K> __device__ inline K pl_scan(K v, bool e, unsigned int w, int lane)
{
    const K inf = PlKey<K>::inf;
    const K off = (K)(w * (unsigned int)(QS_WAVE - 1 - lane)) << PlKey<K>::shift;
    K g = v == inf ? inf : v + off;
    bool start = !e;
    for (int d = 1; d < QS_WAVE; d <<= 1) {
        const K gl = __shfl_up(g, d);
        const bool sl = __shfl_up((int)start, d) != 0;
        if (lane >= d) {
            if (!start) g = gl < g ? gl : g;
            start = start || sl;
        }
    }
    const K c = g == inf ? inf : g - off;
    return c < v ? c : v;
}

__device__ inline int pl_li(int x, int y) { return (y + 1) * PL_H + x + 1; }   // LDS index of tile cell (x, y), halo at -1 / 64

// One round: list `in` of round r (count cnt[r % 3]); appends to the other list (count cnt[(r + 1) % 3], cleared by round
// r - 1) and clears cnt[(r + 2) % 3] for round r + 1 to append to.  Invariant at the start of round r: cnt[(r + 1) % 3]
// == 0.  Grid-stride over the items; every block reads the count itself.  K: the key of the fields (PlKey).
template <typename K> __global__ void __launch_bounds__(PL_BLOCK)
qs_plan_round_kernel(K *__restrict__ fields, size_t fcells, PlBox B, const unsigned int *__restrict__ mask, int mp,
                     int size, const unsigned int *__restrict__ tile_any, int gtx, const unsigned int *__restrict__ list_in,
                     unsigned int *__restrict__ list_out, unsigned int *__restrict__ cnt, unsigned int *__restrict__ marks,
                     unsigned int r, unsigned long long *__restrict__ stats)
{
    __shared__ K s_f[PL_H * PL_H];
    __shared__ unsigned char s_t[PL_H * PL_H];
    __shared__ int s_chg;
    __shared__ unsigned int s_side;
    const K inf = PlKey<K>::inf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int n = cnt[r % 3];
    // cnt[(r + 2) % 3] holds round r - 1's count: cleared by every round, an empty one included, or round r + 2 would
    // read it again (from the other list)
    if (blockIdx.x == 0 && tid == 0) cnt[(r + 2) % 3] = 0;
    if (n == 0) return;
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&stats[0], 1ull);
    if (blockIdx.x < n && tid == 0) atomicAdd(&stats[1], (unsigned long long)((n - 1 - blockIdx.x) / gridDim.x + 1));
    const unsigned int tiles = (unsigned int)(B.ntx * B.nty);
    for (unsigned int it = blockIdx.x; it < n; it += gridDim.x) {
        const unsigned int item = list_in[it];
        const unsigned int f = item / tiles, t = item % tiles;
        const int tx = (int)(t % B.ntx), ty = (int)(t / B.ntx);
        K *fld = fields + (size_t)f * fcells;
        __syncthreads();                                   // the previous item's LDS is no longer read
        for (int i = tid; i < PL_H * PL_H; i += PL_BLOCK) {
            const int fx = tx * PL_T + i % PL_H - 1, fy = ty * PL_T + i / PL_H - 1;
            K v = inf;
            unsigned char tr = 0;
            if (fx >= 0 && fy >= 0 && fx < B.fw && fy < B.fh) {
                v = fld[(size_t)fy * B.fw + fx];
                tr = pl_trav(mask, mp, size, B.bx0 * PL_T + fx, B.by0 * PL_T + fy);
            }
            s_f[i] = v; s_t[i] = tr;
        }
        if (tid == 0) s_side = 0;
        __syncthreads();
        // border cells: the old value (to see what improved), then one relaxation from the halo (constant this visit)
        int bx = 0, by = 0;
        K old = inf;
        if (tid < 4 * PL_T - 4) {
            if (tid < PL_T) { bx = tid; by = 0; }
            else if (tid < 2 * PL_T) { bx = tid - PL_T; by = PL_T - 1; }
            else if (tid < 3 * PL_T - 2) { bx = 0; by = tid - 2 * PL_T + 1; }
            else { bx = PL_T - 1; by = tid - 3 * PL_T + 3; }
            const int c = pl_li(bx, by);
            old = s_f[c];
            if (s_t[c]) {
                K v = old;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        if (!dx && !dy) continue;
                        const int nb = pl_li(bx + dx, by + dy);
                        if (!s_t[nb] || s_f[nb] == inf) continue;
                        if (dx && dy && !(s_t[pl_li(bx + dx, by)] && s_t[pl_li(bx, by + dy)])) continue;
                        const K cand = s_f[nb] + ((K)(dx && dy ? QS_PLAN_DIAG : QS_PLAN_ORTHO) << PlKey<K>::shift);
                        v = cand < v ? cand : v;
                    }
                s_f[c] = v;
            }
        }
        // the interior: four families of 64 lines (rows, columns, diagonals, anti-diagonals), each line scanned both
        // ways; lines of one family are disjoint, so only the families are separated by barriers
        for (;;) {
            if (tid == 0) s_chg = 0;
            __syncthreads();
            for (int fam = 0; fam < 4; fam++) {
                const unsigned int w = fam < 2 ? QS_PLAN_ORTHO : QS_PLAN_DIAG;
                for (int k = wave; k < PL_T; k += PL_BLOCK / QS_WAVE) {
                    int x, y, px, py;                       // this lane's cell and the cell of the lane before
                    if (fam == 0) { x = lane; y = k; px = x - 1; py = y; }
                    else if (fam == 1) { x = k; y = lane; px = x; py = y - 1; }
                    else if (fam == 2) { x = lane; y = (lane + k) & 63; px = x - 1; py = y - 1; }
                    else { x = lane; y = (k - lane) & 63; px = x - 1; py = y + 1; }
                    const int c = pl_li(x, y);
                    bool e = lane > 0 && px >= 0 && py >= 0 && py < PL_T && s_t[c] && s_t[pl_li(px, py)];
                    if (fam >= 2) e = e && s_t[pl_li(px, y)] && s_t[pl_li(x, py)];
                    const K v0 = s_f[c];
                    K v = pl_scan<K>(v0, e, w, lane);
                    // the other way: lane j takes cell 63 - j; its move from the lane before is the move into cell 64 - j
                    const bool eb = __shfl((int)e, (QS_WAVE - lane) & 63) != 0 && lane > 0;
                    const K vb = pl_scan<K>(__shfl(v, QS_WAVE - 1 - lane), eb, w, lane);
                    v = __shfl(vb, QS_WAVE - 1 - lane);
                    if (v != v0) { s_f[c] = v; s_chg = 1; }
                }
                __syncthreads();
            }
            const int chg = s_chg;
            __syncthreads();
            if (!chg) break;
        }
        // what improved on the border: bit 0..3 = the rows / columns y = 0, y = 63, x = 0, x = 63; bit 4..7 the corners
        if (tid < 4 * PL_T - 4 && s_f[pl_li(bx, by)] != old) {
            unsigned int s = by == 0 ? 1u : 0u;
            s |= by == PL_T - 1 ? 2u : 0u;
            s |= bx == 0 ? 4u : 0u;
            s |= bx == PL_T - 1 ? 8u : 0u;
            if ((s & 5u) == 5u) s |= 16u;
            if ((s & 9u) == 9u) s |= 32u;
            if ((s & 6u) == 6u) s |= 64u;
            if ((s & 10u) == 10u) s |= 128u;
            atomicOr(&s_side, s);
        }
        for (int i = tid; i < PL_T * PL_T; i += PL_BLOCK) {
            const int x = i % PL_T, y = i / PL_T;
            const int fy = ty * PL_T + y;
            if (fy < B.fh) fld[(size_t)fy * B.fw + tx * PL_T + x] = s_f[pl_li(x, y)];
        }
        __syncthreads();
        if (tid < 8) {
            const unsigned int side = s_side;
            const int dxs[8] = {0, 0, -1, 1, -1, 1, -1, 1}, dys[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
            const int nx = tx + dxs[tid], ny = ty + dys[tid];
            if (((side >> tid) & 1u) && nx >= 0 && ny >= 0 && nx < B.ntx && ny < B.nty &&
                tile_any[(size_t)(B.by0 + ny) * gtx + B.bx0 + nx]) {
                const unsigned int ni = f * tiles + (unsigned int)(ny * B.ntx + nx);
                if (atomicExch(&marks[ni], r + 1) != r + 1) list_out[atomicAdd(&cnt[(r + 1) % 3], 1u)] = ni;
            }
        }
    }
}

// ---- walk ------------------------------------------------------------------------------------------------------
// the reference's _bresenham (dual_bot_mapper.py:158-179) from (x0, y0) to (x1, y1): every cell traversable
__device__ inline bool pl_visible(const unsigned int *mask, int mp, int size, int x0, int y0, int x1, int y1)
{
    const int dx = abs(x1 - x0), dy = abs(y1 - y0), sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
    int err = dx - dy;
    for (;;) {
        if (!pl_trav(mask, mp, size, x0, y0)) return false;
        if (x0 == x1 && y0 == y1) return true;
        const int e2 = 2 * err;
        if (e2 > -dy) { err -= dy; x0 += sx; }
        if (e2 < dx) { err += dx; y0 += sy; }
    }
}

// one wave per request of the group.  out4[r]: status, waypoint gx, gy, cost; plen[r]: cells of the path
__global__ void __launch_bounds__(PL_BLOCK)
qs_plan_walk_kernel(const unsigned int *__restrict__ fields, size_t fcells, PlBox B, const unsigned int *__restrict__ mask,
                    int mp, int size, const long long *__restrict__ start, const long long *__restrict__ goal, int g0, int gn,
                    int lookahead, int2 *__restrict__ path, size_t path_cap, int4 *__restrict__ out4,
                    long long *__restrict__ plen)
{
    const int lane = threadIdx.x & 63, f = blockIdx.x * (PL_BLOCK / QS_WAVE) + (threadIdx.x >> 6);
    if (f >= gn) return;
    const int q = g0 + f;
    const long long s = start[q], g = goal[q];
    int4 o = make_int4(s < 0 ? QS_PLAN_NO_START : QS_PLAN_NO_GOAL, -1, -1, (int)PL_INF);
    long long len = 0;
    if (s >= 0 && g >= 0) {
        const unsigned int *fld = fields + (size_t)f * fcells;
        const int ox = B.bx0 * PL_T, oy = B.by0 * PL_T;
        auto fval = [&](int gx, int gy) -> unsigned int {
            const int fx = gx - ox, fy = gy - oy;
            if (fx < 0 || fy < 0 || fx >= B.fw || fy >= B.fh) return PL_INF;
            return fld[(size_t)fy * B.fw + fx];
        };
        const int sx = (int)(s % size), sy = (int)(s / size), gx = (int)(g % size), gy = (int)(g / size);
        int cx = sx, cy = sy;
        unsigned int fc = fval(cx, cy);
        if (fc == PL_INF) {
            o.x = QS_PLAN_UNREACHABLE;
        } else {
            o = make_int4(QS_PLAN_OK, sx, sy, (int)fc);
            // E, N, W, S, NE, NW, SW, SE (N = +y)
            const int mdx = lane == 0 || lane == 4 || lane == 7 ? 1 : (lane == 2 || lane == 5 || lane == 6 ? -1 : 0);
            const int mdy = lane == 1 || lane == 4 || lane == 5 ? 1 : (lane == 3 || lane == 6 || lane == 7 ? -1 : 0);
            const unsigned int mw = lane < 4 ? QS_PLAN_ORTHO : QS_PLAN_DIAG;
            int2 mine = make_int2(0, 0);                  // this lane's cell of the present chunk of 64 path cells
            long long idx = 0;                            // index of the present cell (the start is 0)
            bool decided = lookahead < 1;
            if (lane == 0 && path_cap) path[(size_t)q * path_cap] = make_int2(sx, sy);
            while (cx != gx || cy != gy) {
                bool hit = false;
                if (lane < 8) {
                    const int nx = cx + mdx, ny = cy + mdy;
                    const bool legal = pl_trav(mask, mp, size, nx, ny) &&
                                       (lane < 4 || (pl_trav(mask, mp, size, nx, cy) && pl_trav(mask, mp, size, cx, ny)));
                    if (legal) { const unsigned int fn = fval(nx, ny); hit = fn != PL_INF && fn + mw == fc; }
                }
                const unsigned long long m = __ballot(hit);
                if (!m) { o.x = -1; break; }              // not a field: cannot happen for a converged one
                const int d = __ffsll((long long)m) - 1;
                cx += __shfl(mdx, d); cy += __shfl(mdy, d);
                fc -= __shfl((int)mw, d);
                idx++;
                if (lane == 0 && (size_t)idx < path_cap) path[(size_t)q * path_cap + idx] = make_int2(cx, cy);
                if (decided) continue;
                const int slot = (int)((idx - 1) & 63);
                if (lane == slot) mine = make_int2(cx, cy);
                const bool last = idx == lookahead || (cx == gx && cy == gy);
                if (slot == 63 || last) {
                    const bool vis = lane > slot || pl_visible(mask, mp, size, sx, sy, mine.x, mine.y);
                    const unsigned long long bad = __ballot(!vis);
                    if (bad) {
                        const int j = __ffsll((long long)bad) - 1;     // first cell that is not visible: the one before it
                        if (j > 0) { o.y = __shfl(mine.x, j - 1); o.z = __shfl(mine.y, j - 1); }
                        decided = true;
                    } else {
                        o.y = __shfl(mine.x, slot); o.z = __shfl(mine.y, slot);
                        decided = last;
                    }
                }
            }
            len = idx + 1;
        }
    }
    if (lane == 0) { out4[q] = o; plen[q] = o.x == QS_PLAN_OK ? len : 0; }
}

// ---- workspace and launchers -------------------------------------------------------------------------------------
#define QS_PLAN_ROUND_BLOCKS 1024   // workgroups of a relaxation round (they stride over its list)
static inline int pl_tiles(int size) { return (size + PL_T - 1) / PL_T; }

QsPlanLayout qs_plan_layout(void *ws, int size, size_t n, size_t path_cap)
{
    QsPlanLayout L;
    Carve k(ws);
    const int gt = pl_tiles(size);
    L.mp = 2 * gt;
    L.gtx = gt;
    const size_t worst = (size_t)gt * PL_T * gt * PL_T;          // cells of a field over the whole grid
    size_t gmax = QS_PLAN_WS_CAP / (worst * 4);
    if (gmax < 1) gmax = 1;
    if (gmax > n) gmax = n;
    L.gmax = gmax;
    L.field_words = gmax * worst;
    L.item_cap = gmax * (size_t)gt * gt;
    L.mask = k.take<unsigned int>((size_t)gt * PL_T * L.mp);
    L.tile_any = k.take<unsigned int>((size_t)gt * gt);
    L.bbox = k.take<unsigned int>(4);
    L.cnt = k.take<unsigned int>(3);
    L.stats = k.take<unsigned long long>(4);
    L.xy = k.take<double2>(2 * n);
    L.cell = k.take<long long>(2 * n);
    L.out4 = k.take<int4>(n);
    L.plen = k.take<long long>(n);
    L.path = k.take<int2>(n * path_cap);
    L.list0 = k.take<unsigned int>(L.item_cap);
    L.list1 = k.take<unsigned int>(L.item_cap);
    L.marks = k.take<unsigned int>(L.item_cap);
    L.fields = k.take<unsigned int>(L.field_words);
    L.bytes = k.bytes;
    return L;
}

static hipError_t qs_launch_plan_trav(qs_ctx *c, const QsPlanLayout &L, int clearance)
{
    const int gt = pl_tiles(c->cfg.size);
    static const unsigned int init[4] = {0xffffffffu, 0xffffffffu, 0u, 0u};
    hipError_t e = hipMemcpyAsync(L.bbox, init, sizeof init, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(qs_plan_trav_kernel, dim3(gt, gt), dim3(PL_BLOCK), 0, c->stream, c->d_stamps.p, c->cfg.size,
                       clearance, L.mp, L.mask, L.tile_any, L.bbox);
    return hipGetLastError();
}

hipError_t qs_launch_plan_snap(qs_ctx *c, const QsPlanLayout &L, const double2 *xy, long long *cell, size_t n_end, int radius,
                               unsigned long long *snapped)
{
    if (!n_end) return hipSuccess;
    const unsigned int blocks = (unsigned int)((n_end + PL_BLOCK / QS_WAVE - 1) / (PL_BLOCK / QS_WAVE));
    hipLaunchKernelGGL(qs_plan_snap_kernel, dim3(blocks), dim3(PL_BLOCK), 0, c->stream, xy, (int)n_end, c->cfg.res,
                       c->cfg.ox, c->cfg.oy, c->cfg.size, L.mask, L.mp, radius, cell, snapped);
    return hipGetLastError();
}

// requests per group
size_t qs_plan_group(const QsPlanLayout &L, const unsigned int bbox[4], size_t n)
{
    const PlBox B = pl_box(bbox);
    size_t g = L.field_words / ((size_t)B.fw * B.fh);
    return g < n ? g : n;
}

static hipError_t qs_launch_plan_seed(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], const long long *start,
                                      const long long *goal, size_t g0, size_t gn)
{
    const PlBox B = pl_box(bbox);
    const size_t fc = (size_t)B.fw * B.fh;
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)L.fields, PL_INF, gn * fc, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(L.marks, 0, gn * B.ntx * B.nty * sizeof(unsigned int), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(L.cnt, 0, 3 * sizeof(unsigned int), c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(qs_plan_seed_kernel, dim3((unsigned int)((gn + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, c->stream,
                       start, goal, (int)g0, (int)gn, c->cfg.size, B, fc, L.tile_any, L.gtx, L.fields, L.list1, L.cnt, L.marks);
    return hipGetLastError();
}

// fields: the gn fields of a group (L.fields), or the one field of 64-bit keys a caller holds
template <typename K>
static hipError_t qs_launch_plan_round(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], K *fields, size_t gn, unsigned int r)
{
    const PlBox B = pl_box(bbox);
    size_t items = gn * B.ntx * B.nty;
    const unsigned int blocks = (unsigned int)(items < QS_PLAN_ROUND_BLOCKS ? items : QS_PLAN_ROUND_BLOCKS);
    hipLaunchKernelGGL(qs_plan_round_kernel<K>, dim3(blocks), dim3(PL_BLOCK), 0, c->stream, fields, (size_t)B.fw * B.fh, B,
                       L.mask, L.mp, c->cfg.size, L.tile_any, L.gtx, (r & 1) ? L.list1 : L.list0, (r & 1) ? L.list0 : L.list1,
                       L.cnt, L.marks, r, L.stats);
    return hipGetLastError();
}

hipError_t qs_launch_plan_walk(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], const long long *start,
                               const long long *goal, size_t g0, size_t gn, int lookahead, size_t path_cap)
{
    const PlBox B = pl_box(bbox);
    const unsigned int blocks = (unsigned int)((gn + PL_BLOCK / QS_WAVE - 1) / (PL_BLOCK / QS_WAVE));
    hipLaunchKernelGGL(qs_plan_walk_kernel, dim3(blocks), dim3(PL_BLOCK), 0, c->stream, L.fields, (size_t)B.fw * B.fh, B,
                       L.mask, L.mp, c->cfg.size, start, goal, (int)g0, (int)gn, lookahead, L.path, path_cap, L.out4,
                       L.plen);
    return hipGetLastError();
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------
int plan_params(qs_ctx *c, const qs_plan_params *p, qs_plan_params &out)
{
    out = p ? *p : qs_plan_params{2, 10, 200, 0};        // the defaults (include/quasar_slam.h)
    if (out.clearance < 0 || out.clearance > QS_PLAN_MAX_CLEARANCE)
        return qs_fail(c, QS_E_INVAL, "path planning: clearance must lie in [0, QS_PLAN_MAX_CLEARANCE]");
    if (out.snap_radius < 0 || out.snap_radius > QS_PLAN_MAX_SNAP)
        return qs_fail(c, QS_E_INVAL, "path planning: snap_radius must lie in [0, QS_PLAN_MAX_SNAP]");
    if (out.lookahead < 1 || out.lookahead > QS_PLAN_MAX_LOOKAHEAD)
        return qs_fail(c, QS_E_INVAL, "path planning: lookahead must lie in [1, QS_PLAN_MAX_LOOKAHEAD]");
    return QS_OK;
}

// the mask and the census for n requests (layout of the planner workspace); bbox[0] > bbox[2]: no traversable cell
int plan_begin(qs_ctx *c, int clearance, size_t n, size_t path_cap, QsPlanLayout &L, unsigned int bbox[4])
{
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, c->plan_ws.reserve(qs_plan_layout(nullptr, c->cfg.size, n, path_cap).bytes, c->stream));
    L = qs_plan_layout(c->plan_ws.p, c->cfg.size, n, path_cap);
    HIPCHK(c, hipMemsetAsync(L.stats, 0, 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, qs_launch_plan_trav(c, L, clearance));
    HIPCHK(c, hipMemcpyAsync(bbox, L.bbox, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

// the rounds of seeded fields (list 1 holds round 1's items, marks 1): batches of QS_PLAN_ROUND_BATCH without a sync (a
// round that finds its list empty returns at once), the live count read once per batch
#define QS_PLAN_ROUND_BATCH 8
template <typename K>
static int plan_rounds_of(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], K *fields, size_t gn)
{
    for (unsigned int r = 1;; r += QS_PLAN_ROUND_BATCH) {
        for (unsigned int k = 0; k < QS_PLAN_ROUND_BATCH; k++) HIPCHK(c, qs_launch_plan_round(c, L, bbox, fields, gn, r + k));
        unsigned int live = 0;
        HIPCHK(c, hipMemcpyAsync(&live, L.cnt + (r + QS_PLAN_ROUND_BATCH) % 3, sizeof live, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!live) break;
        if (r > 0x7fffffffu) return qs_fail(c, QS_E_STATE, "path planning: the relaxation did not settle");
    }
    return QS_OK;
}

int plan_rounds_key64(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], unsigned long long *key)
{
    return plan_rounds_of(c, L, bbox, key, 1);
}

// the fields of requests g0 .. g0 + gn: seed, then the rounds
int plan_fields(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], const long long *start, const long long *goal,
                size_t g0, size_t gn)
{
    HIPCHK(c, qs_launch_plan_seed(c, L, bbox, start, goal, g0, gn));
    return plan_rounds_of(c, L, bbox, L.fields, gn);
}

// the waypoint stage (plan_common.h): per group the fields, then the walk
int plan_waypoints(qs_ctx *c, const char *who, const QsPlanLayout &L, const unsigned int bbox[4], const long long *start,
                   const long long *goal, size_t m, int lookahead, size_t path_cap, uint64_t &groups, int4 *out4)
{
    const size_t g = qs_plan_group(L, bbox, m);
    if (g == 0) return qs_fail(c, QS_E_STATE, (std::string(who) + ": workspace holds no field").c_str());
    for (size_t g0 = 0; g0 < m; g0 += g, groups++) {
        const size_t gn = std::min(g, m - g0);
        const int rc = plan_fields(c, L, bbox, start, goal, g0, gn);
        if (rc != QS_OK) return rc;
        HIPCHK(c, qs_launch_plan_walk(c, L, bbox, start, goal, g0, gn, lookahead, path_cap));
    }
    HIPCHK(c, hipMemcpyAsync(out4, L.out4, m * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    return QS_OK;
}

extern "C" int qs_traversable(qs_ctx *c, int32_t clearance, uint8_t *mask_host)
{
    ARGCHK(c, c != nullptr && mask_host != nullptr);
    if (clearance < 0 || clearance > QS_PLAN_MAX_CLEARANCE)
        return qs_fail(c, QS_E_INVAL, "qs_traversable: clearance must lie in [0, QS_PLAN_MAX_CLEARANCE]");
    QsPlanLayout L;
    unsigned int bbox[4];
    int rc = plan_begin(c, clearance, 0, 0, L, bbox);
    if (rc != QS_OK) return rc;
    const size_t size = (size_t)c->cfg.size, mp = (size_t)L.mp;
    std::vector<unsigned int> bits(size * mp);
    HIPCHK(c, hipMemcpy(bits.data(), L.mask, bits.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    for (size_t y = 0; y < size; y++)
        for (size_t x = 0; x < size; x++) mask_host[y * size + x] = (bits[y * mp + (x >> 5)] >> (x & 31)) & 1u;
    return QS_OK;
}

extern "C" int qs_plan_field(qs_ctx *c, const qs_plan_params *params, const double goal_xy[2], uint32_t *field_host)
{
    ARGCHK(c, c != nullptr && goal_xy != nullptr && field_host != nullptr);
    qs_plan_params p;
    int rc = plan_params(c, params, p);
    if (rc != QS_OK) return rc;
    QsPlanLayout L;
    unsigned int bbox[4];
    rc = plan_begin(c, p.clearance, 1, 0, L, bbox);
    if (rc != QS_OK) return rc;
    const size_t size = (size_t)c->cfg.size;
    std::fill(field_host, field_host + size * size, 0xffffffffu);
    if (bbox[0] > bbox[2]) return QS_OK;                  // nothing is traversable
    const double xy[4] = {goal_xy[0], goal_xy[1], goal_xy[0], goal_xy[1]};   // (start = goal: only the field is wanted)
    HIPCHK(c, hipMemcpyAsync(L.xy, xy, sizeof xy, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_plan_snap(c, L, L.xy, L.cell, 2, p.snap_radius, L.stats + 3));
    rc = plan_fields(c, L, bbox, L.cell, L.cell + 1, 0, 1);
    if (rc != QS_OK) return rc;
    // the bounding box's cells that lie on the grid, rows of the field into rows of the host array
    const size_t x0 = (size_t)bbox[0] * 64, y0 = (size_t)bbox[1] * 64, fw = (size_t)(bbox[2] - bbox[0] + 1) * 64;
    const size_t fh = (size_t)(bbox[3] - bbox[1] + 1) * 64;
    const size_t w = std::min(fw, size - x0), h = std::min(fh, size - y0);
    HIPCHK(c, hipMemcpy2D(field_host + y0 * size + x0, size * sizeof(uint32_t), L.fields, fw * sizeof(uint32_t),
                          w * sizeof(uint32_t), h, hipMemcpyDeviceToHost));
    return QS_OK;
}

extern "C" int qs_plan_paths(qs_ctx *c, const qs_plan_params *params, const double *start_xy, const double *goal_xy, size_t n,
                             int32_t *status, int32_t *wp_cell_xy, double *wp_xy, uint32_t *cost, int32_t *path_xy,
                             size_t path_cap, int64_t *path_len, uint64_t stats[4])
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (start_xy && goal_xy && status && wp_cell_xy && wp_xy && cost));
    ARGCHK(c, path_cap == 0 || path_xy != nullptr);
    ARGCHK(c, n <= ((size_t)1 << 24));
    qs_plan_params p;
    int rc = plan_params(c, params, p);
    if (rc != QS_OK) return rc;
    QsPlanLayout L;
    unsigned int bbox[4];
    rc = plan_begin(c, p.clearance, n, path_cap, L, bbox);
    if (rc != QS_OK) return rc;
    uint64_t groups = 0;
    unsigned long long st[4] = {0, 0, 0, 0};
    std::vector<int4> out(n, make_int4(QS_PLAN_NO_START, -1, -1, -1));
    std::vector<long long> plen(n, 0);
    if (n && bbox[0] <= bbox[2]) {
        std::vector<double> xy(4 * n);
        memcpy(xy.data(), start_xy, 2 * n * sizeof(double));
        memcpy(xy.data() + 2 * n, goal_xy, 2 * n * sizeof(double));
        HIPCHK(c, hipMemcpyAsync(L.xy, xy.data(), xy.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, qs_launch_plan_snap(c, L, L.xy, L.cell, 2 * n, p.snap_radius, L.stats + 3));
        rc = plan_waypoints(c, "qs_plan_paths", L, bbox, L.cell, L.cell + n, n, p.lookahead, path_cap, groups, out.data());
        if (rc != QS_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(plen.data(), L.plen, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        if (path_cap) HIPCHK(c, hipMemcpyAsync(path_xy, L.path, n * path_cap * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st, L.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }   // (no traversable cell: every start fails to snap, QS_PLAN_NO_START, what the snap kernel would say)
    for (size_t i = 0; i < n; i++) {
        const int4 o = out[i];
        if (o.x < 0) return qs_fail(c, QS_E_STATE, "qs_plan_paths: a path walk found no descending move");
        status[i] = o.x;
        const bool ok = o.x == QS_PLAN_OK;
        wp_cell_xy[2 * i] = ok ? o.y : -1;
        wp_cell_xy[2 * i + 1] = ok ? o.z : -1;
        wp_xy[2 * i] = ok ? c->cfg.ox + (o.y + 0.5) * c->cfg.res : NAN;        // grid_to_world :127-131
        wp_xy[2 * i + 1] = ok ? c->cfg.oy + (o.z + 0.5) * c->cfg.res : NAN;
        cost[i] = ok ? (uint32_t)o.w : 0xffffffffu;
        if (path_len) path_len[i] = ok ? plen[i] : 0;
    }
    if (stats) { stats[0] = st[0]; stats[1] = st[1]; stats[2] = groups; stats[3] = st[3]; }
    return QS_OK;
}
