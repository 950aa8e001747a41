// reloc.hip -- a sweep located against the whole map (include/quasar_slam.h, "relocalisation"): every FREE cell of the search
// box and every rotation step is a candidate pose, scored on the matcher's likelihood field; the best candidate, the best rival
// away from it and a gate on their margin are the answer.  No coarse level: the search is exhaustive and therefore exact.
//
// The unit of work is (sweep, 16 x 16-cell tile):
//   1. a census lists the tiles of the box that hold a FREE cell inside it (compact.h), once per call;
//   2. qs_reloc_score_kernel, one workgroup (4 waves) per (sweep, listed tile): the field patch of the tile plus the sweep's
//      reach all round in LDS (field_patch.h, the matcher's patch); every wave holds all 181 beams and takes rotations wave,
//      wave + 4, ...: the hit beams' cell offsets compacted by ballot into 16-bit patch offsets, then the WHOLE tile in one
//      pass, a lane per (row, four adjacent columns): per beam two dword reads and an align, byte sums spilled to 16-bit
//      halves.  The order of the rule is one 64-bit key; the tile's best goes to table[sweep][slot].  No atomics;
//   3. qs_reloc_pick_kernel: a workgroup per sweep reduces its table row to the best candidate;
//   4. the scoring kernel's EXCL instantiation over the at most 9 tiles that meet the square +-sep round the best, without the
//      candidates rule G6 excludes;
//   5. qs_reloc_final_kernel: rival = max of the table entries of all other tiles (wholly outside the square, so their stored
//      best is eligible) and the re-scored ones; gate; outputs.
// Sweeps run in chunks of RL_CHUNK through one workspace (qs_reloc_layout).
//
// A GROUP of sweeps ("relocalisation of a group", J1-J8) is located the same way from the points of all its records in the
// group's frame:
//   0. qs_reloc_points_kernel, one wave per group, stages each record of the group in turn and ballot-compacts the hit points
//      (px, py doubles) into the group's slice of the workspace, with H and the number of counting records behind them;
//   2'. qs_reloc_group_score_kernel is step 2 with the offsets formed from that list (read through L2, the same for every
//      tile's workgroup) instead of a staged record; the pass over the offsets (rl_sum_list) and the choice of the keys
//      (rl_take) are the single sweep's own routines.  A wave's offset list holds up to 16 x 181 offsets, so the second LDS
//      region is sized for four such lists (23 KiB) where the patch is smaller: one pass over one list, as for one sweep,
//      rather than a walk in pieces that would rebuild the offsets or keep partial sums per piece;
//   3-5. pick as it is; the EXCL instantiation and the final step in their group forms.
// Groups run RL_CHUNK to a launch; their first records travel as a kernel argument (RlGroupArgs::start).
//
// A TRAIL of 42-byte packets ("trail relocalisation", K1-K8) is a group whose points come from the packets themselves:
//   0. qs_reloc_trail_points_kernel, one wave per trail and a lane per record: the records staged and parsed as the trail matcher
//      does (trail_common.h), the anchor by a ballot, one sincos per counting record, four points a record about the anchor,
//      the hits ballot-compacted into the trail's slice of the group workspace; anchor, agent and the anchor's fields behind;
//   2'-4. the group form's scoring kernel, pick and EXCL instantiation as they are, over that list;
//   5. qs_reloc_trail_final_kernel: rl_finish, then the trail's own fields.
// Trails run RL_CHUNK to a launch (RlTrailArgs::start).
#include <math.h>
#include <string.h>
#include <algorithm>

#include "sweep_common.h"
#include "trail_common.h"
#include "field_patch.h"
#include "compact.h"

#define RL_BLOCK 256
#define RL_NW (RL_BLOCK / QS_WAVE)
#define RL_TILE 16
#define RL_OFFP 184               // 16-bit offsets per wave: >= 181, a multiple of 8 (16-byte reads)
#define RL_CHUNK 64               // sweeps, or groups, per launch
// points of a group: QS_RELOC_MAX_GROUP records of 181 beams.  With R = 7 the largest score is 2896 x 8 = 23 168: it fits the
// 16-bit halves the byte sums are spilled to and the 23 bits of the key's score field
#define RL_GPTS (QS_RELOC_MAX_GROUP * QS_SWEEP_BEAMS)
#define RL_GOFFP ((RL_GPTS + 7) / 8 * 8 + 8)   // 16-bit offsets per wave of the group form: 2 904

// key: (score + 1) << 41 | (511 - j) << 32 | (65535 - gy) << 16 | (65535 - gx): larger is earlier in the order of G5; 0 = none
__device__ inline unsigned long long rl_key(unsigned int score, int j, unsigned int low)
{
    return ((unsigned long long)(score + 1u) << 41) | ((unsigned long long)(511 - j) << 32) | low;
}
__device__ inline int rl_key_score(unsigned long long k) { return (int)(k >> 41) - 1; }
__device__ inline int rl_key_j(unsigned long long k) { return 511 - (int)((k >> 32) & 511u); }
__device__ inline int rl_key_gy(unsigned long long k) { return 65535 - (int)((k >> 16) & 0xffffu); }
__device__ inline int rl_key_gx(unsigned long long k) { return 65535 - (int)(k & 0xffffu); }
__device__ inline bool rl_free(unsigned int stamp) { return stamp != 0 && !(stamp & 1u); }

struct QsRelocArgs {
    int R, n_rot, sep, sep_rot, min_hits, min_percent, min_margin;
    int bx0, by0, bx1, by1;       // the search box clipped to the grid (empty: bx1 <= bx0 or by1 <= by0)
    int tx0, ty0, ntx, nty;       // the tiles it meets
    int M;                        // cells a beam's end can lie from the robot's cell: ceil(smax / res) + 1 (a group's frame: smax + travel)
    int SA, pitch;                // patch side 16 + 2 (M + R) and bytes per row (16 x an odd number)
    unsigned int off_b;           // byte offset of the second LDS region (dilation scratch, then the waves' offset lists)
    const double *tab;            // [2][181] cos, sin of the beam angles (the matcher's table)
    const double *rot;            // [n_rot][3] sin, cos of th_j and the yaw reported for it, the host's libm
    const unsigned int *stamps;
    const unsigned int *list;     // census: box-tile indices (ty - ty0) * ntx + (tx - tx0), ascending
    const unsigned long long *count;
    unsigned long long *table;    // [RL_CHUNK][table_pitch] best key per (sweep, listed tile)
    size_t table_pitch;
    unsigned long long *best;     // [RL_CHUNK]
    unsigned long long *excl;     // [RL_CHUNK][9]
    qs_sweep_reloc *out;          // [n] of this chunk
};

// what the group form adds, per chunk of at most RL_CHUNK groups; records are counted from the chunk's first
struct RlGroupArgs {
    const qs_reloc_rel *rel;      // [records of the chunk]
    double travel;
    double *pts;                  // [RL_CHUNK][2][RL_GPTS] px, py of the groups' hit points
    unsigned int *meta;           // [RL_CHUNK][2] H, counting records
    qs_group_reloc *out;          // [groups of the chunk]
    unsigned int start[RL_CHUNK + 1];   // group g's records are [start[g], start[g + 1])
};

// what the trail form adds, per chunk of at most RL_CHUNK trails; records are counted from the chunk's first.  The points and
// H / counting records go where the group form keeps them (RlGroupArgs::pts, meta)
struct RlTrailArgs {
    TrRecords r;                  // the chunk's records
    int max_agent;
    double travel2;
    double *rot;                  // [records of the chunk][2] or nullptr
    int *who;                     // [RL_CHUNK][2] anchor (index within the trail, -1: none), agent
    double *at;                   // [RL_CHUNK][2] X_a, Y_a
    qs_trail_reloc *out;          // [trails of the chunk]
    unsigned int start[RL_CHUNK + 1];   // trail t's records are [start[t], start[t + 1])
};

// ---- census ------------------------------------------------------------------------------------------------------------------
struct RlTilePred {
    const unsigned int *stamps;
    int size, bx0, by0, bx1, by1, tx0, ty0, ntx;
    __device__ bool marked(size_t i) const
    {
        const int tx = tx0 + (int)(i % (size_t)ntx), ty = ty0 + (int)(i / (size_t)ntx);
        const int x0 = max(tx * RL_TILE, bx0), x1 = min(tx * RL_TILE + RL_TILE, bx1);
        const int y0 = max(ty * RL_TILE, by0), y1 = min(ty * RL_TILE + RL_TILE, by1);
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++)
                if (rl_free(stamps[(size_t)y * size + x])) return true;
        return false;
    }
};
struct RlTileEmit {
    unsigned int *list;
    __device__ void put(size_t slot, size_t i) const { list[slot] = (unsigned int)i; }
};

// the tiles that meet the square +-sep round (gx, gy): [tlx, thx] x [tly, thy] (at most 3 x 3; may reach outside the grid)
__device__ inline void rl_square_tiles(int gx, int gy, int sep, int &tlx, int &tly, int &thx, int &thy)
{
    tlx = (gx - sep) >> 4; thx = (gx + sep) >> 4;                  // (arithmetic shift: floor for negatives)
    tly = (gy - sep) >> 4; thy = (gy + sep) >> 4;
}

// the tile of workgroup bx for sweep / group k: 0 = none and nothing to write, 1 = none, the slot gets 0, 2 = (tx, ty); EXCL: the
// best (bgx, bgy, bj) round which the tiles are re-scored
template <bool EXCL>
__device__ __forceinline__ int rl_tile(const QsRelocArgs &m, size_t k, unsigned int bx, int &tx, int &ty, int &bgx, int &bgy, int &bj)
{
    if (EXCL) {
        const unsigned long long bk = m.best[k];
        if (bk == 0) return 1;                                     // (no candidate at all: nothing to exclude)
        bgx = rl_key_gx(bk); bgy = rl_key_gy(bk); bj = rl_key_j(bk);
        int tlx, tly, thx, thy;
        rl_square_tiles(bgx, bgy, m.sep, tlx, tly, thx, thy);
        tx = tlx + (int)(bx % 3u); ty = tly + (int)(bx / 3u);
        if (tx > thx || ty > thy || tx < m.tx0 || tx >= m.tx0 + m.ntx || ty < m.ty0 || ty >= m.ty0 + m.nty) return 1;
    } else {
        if ((unsigned long long)bx >= *m.count) return 0;          // (the grid is sized for every tile of the box)
        const int ti = (int)m.list[bx];
        tx = m.tx0 + ti % m.ntx; ty = m.ty0 + ti / m.ntx;
    }
    return 2;
}

// the lane's four candidates, row `row` and columns 4 cg .. 4 cg + 3 of tile (tx, ty): which are candidates (mask), which lie in
// the square round the best (sq, EXCL), and the low halves of their keys
template <bool EXCL>
__device__ __forceinline__ void rl_lane_cells(const QsRelocArgs &m, int size, int tx, int ty, int row, int cg, int bgx, int bgy,
                                              unsigned int &mask, unsigned int &sq, unsigned int low[4])
{
    const int gy = ty * RL_TILE + row, gxb = tx * RL_TILE + 4 * cg;
    mask = 0; sq = 0;
    #pragma unroll
    for (int e = 0; e < 4; e++) {
        const int gx = gxb + e;
        low[e] = ((unsigned int)(65535 - gy) << 16) | (unsigned int)(65535 - gx);
        if (gx >= m.bx0 && gx < m.bx1 && gy >= m.by0 && gy < m.by1 && rl_free(m.stamps[(size_t)gy * size + gx])) mask |= 1u << e;
        if (EXCL && abs(gx - bgx) <= m.sep && abs(gy - bgy) <= m.sep) sq |= 1u << e;
    }
}

// the field bytes of the lane's four cells summed over the cnt offsets of list o (cnt the same in every lane), into the 16-bit
// halves lo (cells 0, 2) and hi (cells 1, 3); span = offsets whose byte sums cannot overflow
__device__ __forceinline__ void rl_sum_list(const unsigned int *A, const unsigned short *o, int cnt, int span, unsigned int lane_off,
                                            unsigned int &lo, unsigned int &hi)
{
    lo = 0; hi = 0;
    for (int b0 = 0; b0 < cnt; b0 += span) {
        const int b1 = min(b0 + span, cnt);
        unsigned int acc = 0;
        int b = b0;
        for (; b + 8 <= b1; b += 8) {                              // eight beams: one 16-byte read of offsets, sixteen dword reads in flight
            const uint4 q = *(const uint4 *)(o + b);
            acc += mt_look(A, lane_off + (q.x & 0xffffu));
            acc += mt_look(A, lane_off + (q.x >> 16));
            acc += mt_look(A, lane_off + (q.y & 0xffffu));
            acc += mt_look(A, lane_off + (q.y >> 16));
            acc += mt_look(A, lane_off + (q.z & 0xffffu));
            acc += mt_look(A, lane_off + (q.z >> 16));
            acc += mt_look(A, lane_off + (q.w & 0xffffu));
            acc += mt_look(A, lane_off + (q.w >> 16));
        }
        for (; b + 4 <= b1; b += 4) {
            const uint2 q = *(const uint2 *)(o + b);
            acc += mt_look(A, lane_off + (q.x & 0xffffu));
            acc += mt_look(A, lane_off + (q.x >> 16));
            acc += mt_look(A, lane_off + (q.y & 0xffffu));
            acc += mt_look(A, lane_off + (q.y >> 16));
        }
        for (; b < b1; b++) acc += mt_look(A, lane_off + o[b]);
        lo += acc & 0x00ff00ffu;
        hi += (acc >> 8) & 0x00ff00ffu;
    }
}

// the lane's four scores under rotation j against its best key so far
template <bool EXCL>
__device__ __forceinline__ void rl_take(const QsRelocArgs &m, unsigned int lo, unsigned int hi, unsigned int mask, unsigned int sq,
                                        const unsigned int low[4], int j, int bj, unsigned long long &best)
{
    const unsigned int sc[4] = {lo & 0xffffu, hi & 0xffffu, lo >> 16, hi >> 16};
    unsigned int use = mask;
    if (EXCL) {
        const int dj = abs(j - bj);
        if (min(dj, m.n_rot - dj) <= m.sep_rot) use &= ~sq;        // G6: too close to the best on every axis
    }
    #pragma unroll
    for (int e = 0; e < 4; e++) {
        const unsigned long long key = rl_key(sc[e], j, low[e]);
        if (((use >> e) & 1u) && key > best) best = key;
    }
}

// ---- scores of one (sweep, tile) -------------------------------------------------------------------------------------------------
template <bool EXCL>
__global__ void __launch_bounds__(RL_BLOCK)
qs_reloc_score_kernel(QsSweepArgs a, QsGeom geo, QsRelocArgs m)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ unsigned int s_rec[SW_DW];
    __shared__ unsigned long long s_key[RL_NW];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const size_t k = blockIdx.y;
    unsigned long long *dst = EXCL ? m.excl + k * 9 + blockIdx.x : m.table + k * m.table_pitch + blockIdx.x;
    int tx, ty, bgx = 0, bgy = 0, bj = 0;
    const int go = rl_tile<EXCL>(m, k, blockIdx.x, tx, ty, bgx, bgy, bj);
    if (go != 2) { if (go == 1 && tid == 0) *dst = 0; return; }
    if (wave == 0) sw_stage(a, k, s_rec, lane);
    __syncthreads();
    const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
    int agent;
    bool hit[3];
    double bx[3], by[3];
    const bool ok = sw_accept(a, k, s_rec, mis, agent);
    const int H = sw_beams(a, s_rec, mis, m.tab, lane, hit, bx, by);
    if (!ok || H == 0) { if (tid == 0) *dst = 0; return; }         // (uniform over the workgroup)

    // ---- the patch of the field: the tile and M + R cells all round --------------------------------------------------------------
    unsigned int *A = (unsigned int *)s_dyn, *B = (unsigned int *)(s_dyn + m.off_b);
    const int apron = m.M + m.R;
    mt_build_patch(A, B, m.stamps, geo.size, tx * RL_TILE - apron, ty * RL_TILE - apron, m.SA, m.pitch, m.R, tid, RL_BLOCK);

    // ---- the lane's candidates: row `row`, columns 4 cg .. 4 cg + 3 of the tile ------------------------------------------------------
    const int row = lane >> 2, cg = lane & 3;
    unsigned int mask, sq, low[4];
    rl_lane_cells<EXCL>(m, geo.size, tx, ty, row, cg, bgx, bgy, mask, sq, low);
    const unsigned int lane_off = (unsigned int)(row * m.pitch + 4 * cg);
    unsigned short *o = (unsigned short *)B + wave * RL_OFFP;      // this wave's list (the dilation is done with B)
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int span = (255 / (m.R + 1)) & ~7;                       // beams whose byte sums cannot overflow (16-byte list reads)
    unsigned long long best = 0;
    const int rounds = (m.n_rot + RL_NW - 1) / RL_NW;
    for (int r = 0; r < rounds; r++) {
        const int j = r * RL_NW + wave;
        const bool live = j < m.n_rot;                             // (uniform over the wave)
        int cnt = 0;
        if (live) {
            const double s = m.rot[3 * j], c = m.rot[3 * j + 1];
            #pragma unroll
            for (int q = 0; q < 3; q++) {
                bool in = false;
                unsigned int off = 0;
                if (hit[q]) {
                    const double ex = c * bx[q] - s * by[q], ey = s * bx[q] + c * by[q];
                    const int ax = (int)floor(ex / geo.res + 0.5), ay = (int)floor(ey / geo.res + 0.5);
                    in = ax >= -m.M && ax <= m.M && ay >= -m.M && ay <= m.M;       // (|e| <= smax: always)
                    off = (unsigned int)((ay + apron) * m.pitch + (ax + apron));
                }
                const unsigned long long bal = __ballot(in);
                if (in) o[cnt + __popcll(bal & lt)] = (unsigned short)off;
                cnt += __popcll(bal);
            }
        }
        __syncthreads();                                           // (every wave runs every round: the list is written)
        if (live) {
            cnt = __builtin_amdgcn_readfirstlane(cnt);             // (the same in every lane: the loops below are scalar)
            unsigned int lo, hi;
            rl_sum_list(A, o, cnt, span, lane_off, lo, hi);
            rl_take<EXCL>(m, lo, hi, mask, sq, low, j, bj, best);
        }
        __syncthreads();                                           // (the list is read: the next round may overwrite it)
    }
    best = mt_block_max(best, s_key, tid, RL_NW);
    if (tid == 0) *dst = best;
}

// ---- a group's points (J3, J4) ------------------------------------------------------------------------------------------------
// one wave per group of the chunk: its records in turn, the hit points of those that count compacted behind one another
__global__ void __launch_bounds__(QS_WAVE)
qs_reloc_points_kernel(QsSweepArgs a, QsRelocArgs m, RlGroupArgs g)
{
    __shared__ unsigned int s_rec[SW_DW];
    const int lane = threadIdx.x;
    const size_t k = blockIdx.x;
    double *px = g.pts + k * 2 * RL_GPTS, *py = px + RL_GPTS;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const double reach2 = g.travel * g.travel;
    int H = 0, records = 0;                                        // (the same in every lane)
    for (size_t r = g.start[k]; r < g.start[k + 1]; r++) {         // at most QS_RELOC_MAX_GROUP records: H <= RL_GPTS
        __syncthreads();                                           // (the record before is read)
        sw_stage(a, r, s_rec, lane);
        __syncthreads();
        const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + r * a.stride) & 3ull);
        int agent;
        const qs_reloc_rel rel = g.rel[r];
        const bool counts = sw_accept(a, r, s_rec, mis, agent) && isfinite(rel.tx) && isfinite(rel.ty) && isfinite(rel.s) && isfinite(rel.c)
                            && rel.tx * rel.tx + rel.ty * rel.ty <= reach2;
        if (!counts) continue;                                     // (uniform)
        records++;
        bool hit[3];
        double bx[3], by[3];
        sw_beams(a, s_rec, mis, m.tab, lane, hit, bx, by);
        #pragma unroll
        for (int q = 0; q < 3; q++) {
            const unsigned long long bal = __ballot(hit[q]);
            if (hit[q]) {
                const int i = H + __popcll(bal & lt);
                px[i] = rel.tx + (rel.c * bx[q] - rel.s * by[q]);
                py[i] = rel.ty + (rel.s * bx[q] + rel.c * by[q]);
            }
            H += __popcll(bal);
        }
    }
    if (lane == 0) { g.meta[2 * k] = (unsigned int)H; g.meta[2 * k + 1] = (unsigned int)records; }
}

// ---- a trail's points (K2-K4) ---------------------------------------------------------------------------------------------------
// one wave per trail of the chunk, a lane per record: at most 4 x 64 = 256 points, the head of the RL_GPTS a slice holds
__global__ void __launch_bounds__(QS_WAVE)
qs_reloc_trail_points_kernel(RlTrailArgs t, QsGeom geo, double *pts, unsigned int *meta)
{
    __shared__ unsigned int s_raw[TR_RAW_DW];
    const int lane = threadIdx.x;
    const size_t k = blockIdx.x;
    const size_t rec0 = t.start[k];
    const int K = (int)(t.start[k + 1] - t.start[k]);               // 1 .. 64
    const bool staged = t.r.stride <= TR_MAX_STRIDE;
    const unsigned int mis = staged ? tr_stage(t.r, rec0, K, s_raw, lane, QS_WAVE) : 0u;
    __syncthreads();

    bool ok = false;
    int agent = 0;
    float x = 0.f, y = 0.f, yaw = 0.f, dist[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane < K)
        ok = tr_parse(t.r, t.max_agent, rec0 + lane, staged, s_raw, mis + (unsigned int)lane * (unsigned int)t.r.stride, agent, x, y, yaw, dist);
    const unsigned long long acc = __ballot(ok);
    const int anchor = acc ? 63 - __clzll((long long)acc) : -1;    // K2: the last accepted record
    const int src = anchor >= 0 ? anchor : 0;
    const int bot = anchor >= 0 ? __shfl(agent, src) : 0;
    const double X = ok ? (double)x : 0.0, Y = ok ? (double)y : 0.0;
    const double ax = anchor >= 0 ? __shfl(X, src) : 0.0, ay = anchor >= 0 ? __shfl(Y, src) : 0.0;
    const double dx = X - ax, dy = Y - ay;
    const bool counts = ok && agent == bot && dx * dx + dy * dy <= t.travel2;     // K3
    const unsigned long long cb = __ballot(counts);
    double s = 0.0, c = 0.0;
    if (counts) qs_sincos((double)yaw, &s, &c);
    if (t.rot && lane < K) { double *o = t.rot + (rec0 + lane) * 2; o[0] = s; o[1] = c; }
    // T5: front (c, s), left (-s, c), back (-c, -s), right (s, -c)
    const double ux[4] = {c, -s, -c, s}, uy[4] = {s, c, -s, -c};
    double *px = pts + k * 2 * RL_GPTS, *py = px + RL_GPTS;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int H = 0;                                                     // (the same in every lane)
    #pragma unroll
    for (int j = 0; j < 4; j++) {
        const double d = (double)dist[j];
        const bool hit = counts && geo.min_dist < d && d <= geo.max_dist;
        const unsigned long long bal = __ballot(hit);
        if (hit) {
            const int i = H + __popcll(bal & lt);                  // < 256
            px[i] = dx + d * ux[j];
            py[i] = dy + d * uy[j];
        }
        H += __popcll(bal);
    }
    if (lane == 0) {
        meta[2 * k] = (unsigned int)H; meta[2 * k + 1] = (unsigned int)__popcll(cb);
        t.who[2 * k] = anchor; t.who[2 * k + 1] = bot;
        t.at[2 * k] = ax; t.at[2 * k + 1] = ay;
    }
}

// ---- scores of one (group, tile) ----------------------------------------------------------------------------------------------
template <bool EXCL>
__global__ void __launch_bounds__(RL_BLOCK)
qs_reloc_group_score_kernel(QsGeom geo, QsRelocArgs m, RlGroupArgs g)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ unsigned long long s_key[RL_NW];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const size_t k = blockIdx.y;
    unsigned long long *dst = EXCL ? m.excl + k * 9 + blockIdx.x : m.table + k * m.table_pitch + blockIdx.x;
    int tx, ty, bgx = 0, bgy = 0, bj = 0;
    const int go = rl_tile<EXCL>(m, k, blockIdx.x, tx, ty, bgx, bgy, bj);
    if (go != 2) { if (go == 1 && tid == 0) *dst = 0; return; }
    const int H = (int)g.meta[2 * k];
    if (H == 0) { if (tid == 0) *dst = 0; return; }                // (uniform over the workgroup; no counting record: H = 0)
    const double *px = g.pts + k * 2 * RL_GPTS, *py = px + RL_GPTS;

    unsigned int *A = (unsigned int *)s_dyn, *B = (unsigned int *)(s_dyn + m.off_b);
    const int apron = m.M + m.R;
    mt_build_patch(A, B, m.stamps, geo.size, tx * RL_TILE - apron, ty * RL_TILE - apron, m.SA, m.pitch, m.R, tid, RL_BLOCK);

    const int row = lane >> 2, cg = lane & 3;
    unsigned int mask, sq, low[4];
    rl_lane_cells<EXCL>(m, geo.size, tx, ty, row, cg, bgx, bgy, mask, sq, low);
    const unsigned int lane_off = (unsigned int)(row * m.pitch + 4 * cg);
    unsigned short *o = (unsigned short *)B + wave * RL_GOFFP;     // this wave's list: up to RL_GPTS offsets
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int span = (255 / (m.R + 1)) & ~7;
    const double reach = (double)m.M;
    unsigned long long best = 0;
    const int rounds = (m.n_rot + RL_NW - 1) / RL_NW;
    for (int r = 0; r < rounds; r++) {
        const int j = r * RL_NW + wave;
        const bool live = j < m.n_rot;                             // (uniform over the wave)
        int cnt = 0;
        if (live) {
            const double s = m.rot[3 * j], c = m.rot[3 * j + 1];
            for (int p0 = 0; p0 < H; p0 += QS_WAVE) {
                const int i = p0 + lane;
                bool in = false;
                unsigned int off = 0;
                if (i < H) {
                    const double x = px[i], y = py[i];
                    const double ex = c * x - s * y, ey = s * x + c * y;
                    const double fx = floor(ex / geo.res + 0.5), fy = floor(ey / geo.res + 0.5);
                    in = fx >= -reach && fx <= reach && fy >= -reach && fy <= reach;   // J5 (false for a NaN)
                    if (in) off = (unsigned int)(((int)fy + apron) * m.pitch + ((int)fx + apron));
                }
                const unsigned long long bal = __ballot(in);
                if (in) o[cnt + __popcll(bal & lt)] = (unsigned short)off;
                cnt += __popcll(bal);
            }
        }
        __syncthreads();                                           // (every wave runs every round: the list is written)
        if (live) {
            cnt = __builtin_amdgcn_readfirstlane(cnt);
            unsigned int lo, hi;
            rl_sum_list(A, o, cnt, span, lane_off, lo, hi);
            rl_take<EXCL>(m, lo, hi, mask, sq, low, j, bj, best);
        }
        __syncthreads();                                           // (the list is read: the next round may overwrite it)
    }
    best = mt_block_max(best, s_key, tid, RL_NW);
    if (tid == 0) *dst = best;
}

// ---- the best of a sweep's table row --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RL_BLOCK)
qs_reloc_pick_kernel(QsRelocArgs m)
{
    __shared__ unsigned long long s_key[RL_NW];
    const size_t k = blockIdx.x, cnt = (size_t)*m.count;
    const unsigned long long *row = m.table + k * m.table_pitch;
    unsigned long long best = 0;
    for (size_t i = threadIdx.x; i < cnt; i += RL_BLOCK) best = row[i] > best ? row[i] : best;
    best = mt_block_max(best, s_key, threadIdx.x, RL_NW);
    if (threadIdx.x == 0) m.best[k] = best;
}

// ---- rival, gate, outputs ---------------------------------------------------------------------------------------------------------
__device__ inline void rl_set_records(qs_sweep_reloc &r, int n) { r.accepted_record = (unsigned char)n; }
__device__ inline void rl_set_records(qs_group_reloc &r, int n) { r.records = (unsigned char)n; }
__device__ inline void rl_set_records(qs_trail_reloc &r, int n) { r.records = (unsigned char)n; }

// sweep or group k with H hit points from `records` counting records: rival = max of the table entries of all tiles outside the
// square round the best and of the re-scored ones; G7-G9.  Every thread of the workgroup calls it
template <typename OUT>
__device__ __forceinline__ void rl_finish(const QsGeom &geo, const QsRelocArgs &m, size_t k, int records, int H, OUT *out,
                                          unsigned long long *s_key, int tid)
{
    OUT r;
    memset(&r, 0, sizeof r);
    if (records == 0) {                                            // (uniform over the workgroup)
        r.status = QS_RELOC_NO_RECORD;
        if (tid == 0) *out = r;
        return;
    }
    const unsigned long long bk = m.best[k];
    unsigned long long rival = 0;
    if (bk != 0) {
        int tlx, tly, thx, thy;
        rl_square_tiles(rl_key_gx(bk), rl_key_gy(bk), m.sep, tlx, tly, thx, thy);
        const size_t cnt = (size_t)*m.count;
        const unsigned long long *row = m.table + k * m.table_pitch;
        for (size_t i = tid; i < cnt; i += RL_BLOCK) {
            const int ti = (int)m.list[i], tx = m.tx0 + ti % m.ntx, ty = m.ty0 + ti / m.ntx;
            if (tx >= tlx && tx <= thx && ty >= tly && ty <= thy) continue;          // re-scored without the excluded candidates
            rival = row[i] > rival ? row[i] : rival;
        }
        if (tid < 9) rival = max(rival, m.excl[k * 9 + tid]);
    }
    rival = mt_block_max(rival, s_key, tid, RL_NW);
    if (tid != 0) return;
    rl_set_records(r, records);
    r.hits = H;
    r.gx = r.gy = r.j = r.gx2 = r.gy2 = r.j2 = -1;
    if (bk == 0) {                                                 // no FREE cell in the box, or H = 0
        r.status = QS_RELOC_NO_CANDIDATE;
        *out = r;
        return;
    }
    r.status = QS_RELOC_OK;
    r.gx = rl_key_gx(bk); r.gy = rl_key_gy(bk); r.j = rl_key_j(bk); r.score = rl_key_score(bk);
    if (rival != 0) { r.gx2 = rl_key_gx(rival); r.gy2 = rl_key_gy(rival); r.j2 = rl_key_j(rival); r.score2 = rl_key_score(rival); }
    const long long full = (long long)H * (m.R + 1);
    r.accepted = H >= m.min_hits && (long long)r.score * 100 >= (long long)m.min_percent * full
                 && (long long)(r.score - r.score2) * 100 >= (long long)m.min_margin * full;
    r.x = geo.ox + ((double)r.gx + 0.5) * geo.res;
    r.y = geo.oy + ((double)r.gy + 0.5) * geo.res;
    r.yaw = m.rot[3 * r.j + 2];
    *out = r;
}

__global__ void __launch_bounds__(RL_BLOCK)
qs_reloc_final_kernel(QsSweepArgs a, QsGeom geo, QsRelocArgs m)
{
    __shared__ unsigned int s_rec[SW_DW];
    __shared__ unsigned long long s_key[RL_NW];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const size_t k = blockIdx.x;
    if (wave == 0) sw_stage(a, k, s_rec, lane);
    __syncthreads();
    const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
    int agent;
    bool hit[3];
    double bx[3], by[3];
    const bool ok = sw_accept(a, k, s_rec, mis, agent);
    const int H = sw_beams(a, s_rec, mis, m.tab, lane, hit, bx, by);
    rl_finish(geo, m, k, ok ? 1 : 0, H, m.out + k, s_key, tid);
}

__global__ void __launch_bounds__(RL_BLOCK)
qs_reloc_group_final_kernel(QsGeom geo, QsRelocArgs m, RlGroupArgs g)
{
    __shared__ unsigned long long s_key[RL_NW];
    const size_t k = blockIdx.x;
    rl_finish(geo, m, k, (int)g.meta[2 * k + 1], (int)g.meta[2 * k], g.out + k, s_key, threadIdx.x);
}

// K7: the group form's result, then what a trail adds (thread 0 wrote the result and completes it)
__global__ void __launch_bounds__(RL_BLOCK)
qs_reloc_trail_final_kernel(QsGeom geo, QsRelocArgs m, RlTrailArgs t, const unsigned int *meta)
{
    __shared__ unsigned long long s_key[RL_NW];
    const size_t k = blockIdx.x;
    const int records = (int)meta[2 * k + 1];
    rl_finish(geo, m, k, records, (int)meta[2 * k], t.out + k, s_key, threadIdx.x);
    if (threadIdx.x != 0) return;
    qs_trail_reloc *r = t.out + k;
    if (records == 0) { r->anchor = -1; return; }
    r->anchor = t.who[2 * k]; r->agent = (uint8_t)t.who[2 * k + 1];
    r->ax = t.at[2 * k]; r->ay = t.at[2 * k + 1];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct QsRelocSetup { qs_reloc_params p; int M; };

// travel: the group form's (J8) and the trail form's (K8, whose ranges end at max_dist); 0 for a single sweep, whose limit and
// text are G's
enum { RL_SWEEP, RL_GROUP, RL_TRAIL };
static int reloc_setup(qs_ctx *c, const qs_reloc_params *params, const char *who, QsRelocSetup &rs, double travel = 0.0, int form = RL_SWEEP)
{
    qs_reloc_params p = {2, 180, 4, 2, 40, 70, 5, 0, 0, 0, 0, 0};
    if (params) p = *params;
    char msg[256];
    const char *bad = nullptr;
    if (p.radius < 0 || p.radius > QS_MATCH_MAX_RADIUS) bad = "radius must lie in [0, QS_MATCH_MAX_RADIUS]";
    else if (p.n_rot < 1 || p.n_rot > QS_RELOC_MAX_ROT) bad = "n_rot must lie in [1, 360]";
    else if (p.sep < 0 || p.sep > QS_RELOC_MAX_SEP) bad = "sep must lie in [0, 16]";
    else if (p.sep_rot < 0 || p.sep_rot >= p.n_rot) bad = "sep_rot must lie in [0, n_rot)";
    else if (p.min_hits < 0) bad = "min_hits must not be negative";
    else if (p.min_percent < 0 || p.min_percent > 100) bad = "min_percent must lie in [0, 100]";
    else if (p.min_margin < 0 || p.min_margin > 100) bad = "min_margin must lie in [0, 100]";
    else if (!(travel >= 0.0) || !std::isfinite(travel)) bad = "travel must be finite and not negative";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    const double reach = ceil(((form == RL_TRAIL ? c->cfg.max_dist : c->sweep_max) + travel) / c->cfg.res);      // (travel 0: smax + 0 is smax)
    if (!(RL_TILE + 2 * (reach + p.radius + 1) <= 255))
        bad = form == RL_TRAIL ? "max_dist + travel is too large for this resolution: 16 + 2 * (ceil((max_dist + travel) / res) + radius + 1) exceeds 255"
            : form == RL_GROUP ? "smax + travel is too large for this resolution: 16 + 2 * (ceil((smax + travel) / res) + radius + 1) exceeds 255"
                               : "the sweep filter's smax is too large for this resolution: 16 + 2 * (ceil(smax / res) + radius + 1) exceeds 255";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    if (!p.use_box) { p.x0 = 0; p.y0 = 0; p.x1 = c->cfg.size; p.y1 = c->cfg.size; }
    rs.p = p;
    rs.M = (int)reach + 1;
    return QS_OK;
}

static int reloc_call_ok(qs_ctx *c, size_t n, size_t stride, const char *who)
{
    char msg[256];
    const char *bad = nullptr;
    if (stride != QS_SWEEP_SIZE_V0 && stride != QS_SWEEP_SIZE_V0_ODO) bad = "stride must be 743 (v0) or 751 (v0 + odometry)";
    else if (c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0) bad = "sharded contexts (seq_stride > 1, shard_bots > 0) do not take sweeps";
    else if (n >= ((size_t)1 << 31)) bad = "at most 2^31 - 1 records per call";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    return QS_OK;
}

// J1
static int reloc_groups_ok(qs_ctx *c, size_t n, const int32_t *gsize, size_t n_groups, const char *who)
{
    char msg[256];
    size_t sum = 0;
    for (size_t g = 0; g < n_groups; g++) {
        if (gsize[g] < 1 || gsize[g] > QS_RELOC_MAX_GROUP) {
            snprintf(msg, sizeof msg, "%s: gsize[%zu] must lie in [1, QS_RELOC_MAX_GROUP]", who, g);
            return qs_fail(c, QS_E_INVAL, msg);
        }
        sum += (size_t)gsize[g];
    }
    if (sum != n) { snprintf(msg, sizeof msg, "%s: the group sizes must sum to n", who); return qs_fail(c, QS_E_INVAL, msg); }
    return QS_OK;
}

// the workspace of one call over n_tiles box tiles, carved from ws (nullptr: only the bytes the block needs); groups: with the
// point lists of a chunk of groups
struct QsRelocLayout {
    unsigned int *chunk, *list; unsigned long long *count, *table, *best, *excl; double *pts; unsigned int *meta;
    double *at; int *who;         // a chunk of trails: the anchors' fields, anchor and agent (RlTrailArgs)
    size_t bytes;
};
static QsRelocLayout qs_reloc_layout(void *ws, size_t n_tiles, bool groups)
{
    Carve cv(ws);
    QsRelocLayout L;
    L.chunk = cv.take<unsigned int>(qs_compact_chunks(n_tiles) + 1);
    L.list = cv.take<unsigned int>(n_tiles + 1);
    L.count = cv.take<unsigned long long>(1);
    L.table = cv.take<unsigned long long>((size_t)RL_CHUNK * (n_tiles + 1));
    L.best = cv.take<unsigned long long>(RL_CHUNK);
    L.excl = cv.take<unsigned long long>((size_t)RL_CHUNK * 9);
    L.pts = groups ? cv.take<double>((size_t)RL_CHUNK * 2 * RL_GPTS) : nullptr;
    L.meta = groups ? cv.take<unsigned int>((size_t)RL_CHUNK * 2) : nullptr;
    L.at = groups ? cv.take<double>((size_t)RL_CHUNK * 2) : nullptr;
    L.who = groups ? cv.take<int>((size_t)RL_CHUNK * 2) : nullptr;
    L.bytes = cv.bytes;
    return L;
}

// what every launch of a call shares: the tables, the box and its tiles, the patch and the LDS it takes (offp: 16-bit offsets a
// wave lists), the workspace, the census.  Everything enqueued (but a workspace that has to grow waits for the stream first)
struct QsRelocPlan { QsRelocArgs m; QsRelocLayout L; size_t n_tiles, lds; };
static hipError_t reloc_prepare(qs_ctx *c, const QsRelocSetup &rs, size_t offp, bool groups, QsRelocPlan &pl)
{
    const qs_reloc_params &p = rs.p;
    static const double kTwoPi = 2.0 * 3.141592653589793;
    HIPRET(qs_beam_table(c));                                      // the beam angles' cos / sin (match.hip)
    if (c->reloc_nrot != p.n_rot) {                                // G2: the rotations' sin / cos and reported yaw, libm's
        std::vector<double> rot(3 * (size_t)QS_RELOC_MAX_ROT, 0.0);
        const double step = kTwoPi / (double)p.n_rot;
        for (int j = 0; j < p.n_rot; j++) {
            const double th = (double)j * step;
            rot[3 * j] = sin(th); rot[3 * j + 1] = cos(th); rot[3 * j + 2] = th > 3.141592653589793 ? th - kTwoPi : th;
        }
        if (!c->reloc_rot.p) HIPRET(c->reloc_rot.alloc(3 * (size_t)QS_RELOC_MAX_ROT));
        HIPRET(hipStreamSynchronize(c->stream));                   // (an earlier call may still read the old table)
        c->reloc_nrot = 0;
        HIPRET(hipMemcpy(c->reloc_rot.p, rot.data(), rot.size() * sizeof(double), hipMemcpyHostToDevice));
        c->reloc_nrot = p.n_rot;
    }
    const int size = c->cfg.size;
    QsRelocArgs &m = pl.m;
    m.R = p.radius; m.n_rot = p.n_rot; m.sep = p.sep; m.sep_rot = p.sep_rot;
    m.min_hits = p.min_hits; m.min_percent = p.min_percent; m.min_margin = p.min_margin;
    m.bx0 = std::max(p.x0, 0); m.by0 = std::max(p.y0, 0); m.bx1 = std::min(p.x1, size); m.by1 = std::min(p.y1, size);
    const bool empty = m.bx1 <= m.bx0 || m.by1 <= m.by0;
    if (empty) { m.bx0 = m.by0 = m.bx1 = m.by1 = 0; }
    m.tx0 = m.bx0 / RL_TILE; m.ty0 = m.by0 / RL_TILE;
    m.ntx = empty ? 0 : (m.bx1 - 1) / RL_TILE - m.tx0 + 1;
    m.nty = empty ? 0 : (m.by1 - 1) / RL_TILE - m.ty0 + 1;
    const size_t n_tiles = pl.n_tiles = (size_t)m.ntx * m.nty;
    m.M = rs.M;
    m.SA = RL_TILE + 2 * (m.M + m.R);                              // <= 255 (reloc_setup)
    // rows of 4 x (an odd number) dwords: the 8 rows x 4 dwords a lane group of the scoring pass reads fall on 32 different banks
    m.pitch = (m.SA + 15) & ~15;
    if (!((m.pitch >> 4) & 1)) m.pitch += 16;
    const size_t a_bytes = ((size_t)m.SA * m.pitch + 16 + 15) & ~(size_t)15;
    const size_t b_bytes = std::max((size_t)m.SA * m.pitch, (size_t)RL_NW * offp * sizeof(unsigned short));
    m.off_b = (unsigned int)a_bytes;
    pl.lds = a_bytes + ((b_bytes + 15) & ~(size_t)15);
    m.tab = c->match_tab.p; m.rot = c->reloc_rot.p; m.stamps = c->d_stamps.p;
    m.out = nullptr;

    HIPRET(c->reloc_ws.reserve(qs_reloc_layout(nullptr, n_tiles, groups).bytes, c->stream, (size_t)1 << 16));
    const QsRelocLayout L = pl.L = qs_reloc_layout(c->reloc_ws.p, n_tiles, groups);
    m.list = L.list; m.count = L.count; m.table = L.table; m.table_pitch = n_tiles + 1; m.best = L.best; m.excl = L.excl;
    if (n_tiles == 0) HIPRET(hipMemsetAsync(L.count, 0, sizeof(unsigned long long), c->stream));
    else {
        const RlTilePred pred{c->d_stamps.p, size, m.bx0, m.by0, m.bx1, m.by1, m.tx0, m.ty0, m.ntx};
        const RlTileEmit emit{L.list};
        HIPRET(qs_compact(c->stream, pred, n_tiles, false, emit, n_tiles, L.chunk, L.count));
        HIPRET(qs_compact(c->stream, pred, n_tiles, true, emit, n_tiles, L.chunk, L.count));
    }
    return hipSuccess;
}

// n device-resident records against the map as the stream finds it, into d_out; everything enqueued, nothing waited for
// (but a workspace that has to grow waits for the stream first)
static hipError_t reloc_launch(qs_ctx *c, const QsRelocSetup &rs, const unsigned char *d_pkts, size_t n, size_t stride,
                               const unsigned short *d_lens, qs_sweep_reloc *d_out)
{
    if (n == 0) return hipSuccess;
    QsRelocPlan pl;
    HIPRET(reloc_prepare(c, rs, RL_OFFP, false, pl));
    QsRelocArgs &m = pl.m;
    const size_t n_tiles = pl.n_tiles, lds = pl.lds;
    if (lds > 32 * 1024) {                                         // long reaches: up to 2 x 69 088 B (SA 254, rows of 272) of the CU's 160 KiB
        HIPRET(hipFuncSetAttribute((const void *)qs_reloc_score_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIPRET(hipFuncSetAttribute((const void *)qs_reloc_score_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    for (size_t k0 = 0; k0 < n; k0 += RL_CHUNK) {
        const unsigned int nk = (unsigned int)std::min((size_t)RL_CHUNK, n - k0);
        QsSweepArgs a;
        qs_sweep_args(c, d_pkts + k0 * stride, nk, stride, d_lens ? d_lens + k0 : nullptr, QS_SWEEP_NO_GRAPH, a);
        m.out = d_out + k0;
        if (n_tiles) {
            hipLaunchKernelGGL(qs_reloc_score_kernel<false>, dim3((unsigned int)n_tiles, nk), dim3(RL_BLOCK), lds, c->stream, a, c->geom, m);
            HIPRET(hipGetLastError());
        }
        hipLaunchKernelGGL(qs_reloc_pick_kernel, dim3(nk), dim3(RL_BLOCK), 0, c->stream, m);
        HIPRET(hipGetLastError());
        hipLaunchKernelGGL(qs_reloc_score_kernel<true>, dim3(9, nk), dim3(RL_BLOCK), lds, c->stream, a, c->geom, m);
        HIPRET(hipGetLastError());
        hipLaunchKernelGGL(qs_reloc_final_kernel, dim3(nk), dim3(RL_BLOCK), 0, c->stream, a, c->geom, m);
        HIPRET(hipGetLastError());
    }
    return hipSuccess;
}

// the same for n_groups groups (gsize: host, already checked against J1) of device-resident records
static hipError_t reloc_group_launch(qs_ctx *c, const QsRelocSetup &rs, const unsigned char *d_pkts, size_t stride, const unsigned short *d_lens,
                                     const qs_reloc_rel *d_rel, const int32_t *gsize, size_t n_groups, double travel, qs_group_reloc *d_out)
{
    if (n_groups == 0) return hipSuccess;
    QsRelocPlan pl;
    HIPRET(reloc_prepare(c, rs, RL_GOFFP, true, pl));
    const QsRelocArgs &m = pl.m;
    const size_t n_tiles = pl.n_tiles, lds = pl.lds;
    if (lds > 32 * 1024) {                                         // up to 2 x 69 KiB of the CU's 160
        HIPRET(hipFuncSetAttribute((const void *)qs_reloc_group_score_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIPRET(hipFuncSetAttribute((const void *)qs_reloc_group_score_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    size_t rec0 = 0;
    for (size_t g0 = 0; g0 < n_groups; g0 += RL_CHUNK) {
        const unsigned int ng = (unsigned int)std::min((size_t)RL_CHUNK, n_groups - g0);
        RlGroupArgs g;
        g.rel = d_rel + rec0; g.travel = travel; g.pts = pl.L.pts; g.meta = pl.L.meta; g.out = d_out + g0;
        unsigned int nr = 0;
        for (unsigned int i = 0; i <= RL_CHUNK; i++) {
            g.start[i] = nr;
            if (i < ng) nr += (unsigned int)gsize[g0 + i];
        }
        QsSweepArgs a;
        qs_sweep_args(c, d_pkts + rec0 * stride, nr, stride, d_lens ? d_lens + rec0 : nullptr, QS_SWEEP_NO_GRAPH, a);
        hipLaunchKernelGGL(qs_reloc_points_kernel, dim3(ng), dim3(QS_WAVE), 0, c->stream, a, m, g);
        HIPRET(hipGetLastError());
        if (n_tiles) {
            hipLaunchKernelGGL(qs_reloc_group_score_kernel<false>, dim3((unsigned int)n_tiles, ng), dim3(RL_BLOCK), lds, c->stream, c->geom, m, g);
            HIPRET(hipGetLastError());
        }
        hipLaunchKernelGGL(qs_reloc_pick_kernel, dim3(ng), dim3(RL_BLOCK), 0, c->stream, m);
        HIPRET(hipGetLastError());
        hipLaunchKernelGGL(qs_reloc_group_score_kernel<true>, dim3(9, ng), dim3(RL_BLOCK), lds, c->stream, c->geom, m, g);
        HIPRET(hipGetLastError());
        hipLaunchKernelGGL(qs_reloc_group_final_kernel, dim3(ng), dim3(RL_BLOCK), 0, c->stream, c->geom, m, g);
        HIPRET(hipGetLastError());
        rec0 += nr;
    }
    return hipSuccess;
}

// ---- C ABI: relocalisation (semantics in include/quasar_slam.h) ------------------------------------------------------------------
extern "C" int qs_relocalise_sweeps_device(qs_ctx *c, const qs_reloc_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                           const uint16_t *d_lens, qs_sweep_reloc *d_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (d_pkts != nullptr && d_out != nullptr));
    QsRelocSetup rs;
    int rc = reloc_setup(c, params, "qs_relocalise_sweeps", rs);
    if (rc != QS_OK) return rc;
    rc = reloc_call_ok(c, n, stride, "qs_relocalise_sweeps");
    if (rc != QS_OK || n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, reloc_launch(c, rs, d_pkts, n, stride, d_lens, d_out));
    return QS_OK;
}

extern "C" int qs_relocalise_sweeps(qs_ctx *c, const qs_reloc_params *params, const uint8_t *pkts, size_t n, size_t stride,
                                    const uint16_t *lens, qs_sweep_reloc *out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pkts != nullptr && out != nullptr));
    QsRelocSetup rs;
    int rc = reloc_setup(c, params, "qs_relocalise_sweeps", rs);
    if (rc != QS_OK) return rc;
    rc = reloc_call_ok(c, n, stride, "qs_relocalise_sweeps");
    if (rc != QS_OK || n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    const size_t chunk = (size_t)1 << 12;                          // records staged per round trip
    for (size_t k0 = 0; k0 < n; k0 += chunk) {
        const size_t nk = std::min(chunk, n - k0);
        Staging s;
        rc = reserve_staging(c, nk * stride, s);
        if (rc != QS_OK) return rc;
        HIPCHK(c, c->io_ws.reserve(nk * sizeof(qs_sweep_reloc), c->stream, QS_IO_WS_FLOOR));
        qs_sweep_reloc *d_out = (qs_sweep_reloc *)c->io_ws.p;
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, nk * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, nk * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, reloc_launch(c, rs, s.pkts, nk, stride, lens ? s.lens : nullptr, d_out));
        HIPCHK(c, hipMemcpyAsync(out + k0, d_out, nk * sizeof(qs_sweep_reloc), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return QS_OK;
}

// ---- C ABI: relocalisation of a group -------------------------------------------------------------------------------------------
static int reloc_groups_check(qs_ctx *c, const qs_reloc_params *params, size_t n, size_t stride, const int32_t *gsize, size_t n_groups,
                              double travel, QsRelocSetup &rs)
{
    int rc = reloc_setup(c, params, "qs_relocalise_groups", rs, travel, RL_GROUP);
    if (rc != QS_OK) return rc;
    rc = reloc_call_ok(c, n, stride, "qs_relocalise_groups");
    if (rc != QS_OK) return rc;
    return reloc_groups_ok(c, n, gsize, n_groups, "qs_relocalise_groups");
}

extern "C" int qs_relocalise_groups_device(qs_ctx *c, const qs_reloc_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                           const uint16_t *d_lens, const qs_reloc_rel *d_rel, const int32_t *gsize, size_t n_groups,
                                           double travel, qs_group_reloc *d_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (d_pkts != nullptr && d_rel != nullptr));
    ARGCHK(c, n_groups == 0 || (gsize != nullptr && d_out != nullptr));
    QsRelocSetup rs;
    const int rc = reloc_groups_check(c, params, n, stride, gsize, n_groups, travel, rs);
    if (rc != QS_OK || n_groups == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, reloc_group_launch(c, rs, d_pkts, stride, d_lens, d_rel, gsize, n_groups, travel, d_out));
    return QS_OK;
}

extern "C" int qs_relocalise_groups(qs_ctx *c, const qs_reloc_params *params, const uint8_t *pkts, size_t n, size_t stride,
                                    const uint16_t *lens, const qs_reloc_rel *rel, const int32_t *gsize, size_t n_groups, double travel,
                                    qs_group_reloc *out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pkts != nullptr && rel != nullptr));
    ARGCHK(c, n_groups == 0 || (gsize != nullptr && out != nullptr));
    QsRelocSetup rs;
    int rc = reloc_groups_check(c, params, n, stride, gsize, n_groups, travel, rs);
    if (rc != QS_OK || n_groups == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    const size_t chunk = (size_t)1 << 12;                          // records staged per round trip: whole groups, one at least
    size_t k0 = 0;
    for (size_t g0 = 0; g0 < n_groups;) {
        size_t g1 = g0, nk = 0;
        while (g1 < n_groups && (g1 == g0 || nk + (size_t)gsize[g1] <= chunk)) nk += (size_t)gsize[g1++];
        const size_t ng = g1 - g0;
        Staging s;
        rc = reserve_staging(c, nk * stride, s);
        if (rc != QS_OK) return rc;
        Carve cv(nullptr);
        cv.take<qs_group_reloc>(ng); cv.take<qs_reloc_rel>(nk);
        HIPCHK(c, c->io_ws.reserve(cv.bytes, c->stream, QS_IO_WS_FLOOR));
        Carve io(c->io_ws.p);
        qs_group_reloc *d_out = io.take<qs_group_reloc>(ng);
        qs_reloc_rel *d_rel = io.take<qs_reloc_rel>(nk);
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, nk * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, nk * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_rel, rel + k0, nk * sizeof(qs_reloc_rel), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, reloc_group_launch(c, rs, s.pkts, stride, lens ? s.lens : nullptr, d_rel, gsize + g0, ng, travel, d_out));
        HIPCHK(c, hipMemcpyAsync(out + g0, d_out, ng * sizeof(qs_group_reloc), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        g0 = g1; k0 += nk;
    }
    return QS_OK;
}

// ---- trail relocalisation ------------------------------------------------------------------------------------------------------
// K8 and K1, before anything is enqueued
static int reloc_trails_check(qs_ctx *c, const qs_reloc_params *params, size_t n, size_t stride, const int32_t *gsize, size_t n_groups,
                              double travel, QsRelocSetup &rs)
{
    static const char *who = "qs_relocalise_trails";
    const int rc = reloc_setup(c, params, who, rs, travel, RL_TRAIL);
    if (rc != QS_OK) return rc;
    char msg[256];
    const char *bad = nullptr;
    if (stride < QS_PACKET_SIZE_V1) bad = "stride must be at least 41";
    else if (c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0) bad = "sharded contexts (seq_stride > 1, shard_bots > 0) do not relocalise trails";
    else if (n >= ((size_t)1 << 31)) bad = "at most 2^31 - 1 records per call";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    size_t sum = 0;
    for (size_t g = 0; g < n_groups; g++) {
        if (gsize[g] < 1 || gsize[g] > QS_TRAIL_MAX_RECORDS) {
            snprintf(msg, sizeof msg, "%s: gsize[%zu] must lie in [1, QS_TRAIL_MAX_RECORDS]", who, g);
            return qs_fail(c, QS_E_INVAL, msg);
        }
        sum += (size_t)gsize[g];
    }
    if (sum != n) { snprintf(msg, sizeof msg, "%s: the group sizes must sum to n", who); return qs_fail(c, QS_E_INVAL, msg); }
    return QS_OK;
}

// n_groups trails (gsize: host, already checked against K1) of device-resident records against the map as the stream finds it;
// d_rot (optional): [records][2].  Everything enqueued, nothing waited for (but see reloc_prepare).  The scoring kernel's lists
// stand RL_GOFFP offsets apart whatever they hold, so the plan is the group form's
static hipError_t reloc_trail_launch(qs_ctx *c, const QsRelocSetup &rs, const unsigned char *d_pkts, size_t stride, const unsigned short *d_lens,
                                     const int32_t *gsize, size_t n_groups, double travel, qs_trail_reloc *d_out, double *d_rot)
{
    if (n_groups == 0) return hipSuccess;
    QsRelocPlan pl;
    HIPRET(reloc_prepare(c, rs, RL_GOFFP, true, pl));
    const QsRelocArgs &m = pl.m;
    const size_t n_tiles = pl.n_tiles, lds = pl.lds;
    if (lds > 32 * 1024) {                                         // up to 2 x 69 KiB of the CU's 160
        HIPRET(hipFuncSetAttribute((const void *)qs_reloc_group_score_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIPRET(hipFuncSetAttribute((const void *)qs_reloc_group_score_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    RlGroupArgs g;                                                 // what the scoring kernel reads of it: the lists and their lengths
    memset(&g, 0, sizeof g);
    g.travel = travel; g.pts = pl.L.pts; g.meta = pl.L.meta;
    RlTrailArgs t;
    memset(&t, 0, sizeof t);
    t.r.stride = stride; t.max_agent = c->cfg.max_agent; t.travel2 = travel * travel;
    t.who = pl.L.who; t.at = pl.L.at;
    size_t rec0 = 0;
    for (size_t g0 = 0; g0 < n_groups; g0 += RL_CHUNK) {
        const unsigned int ng = (unsigned int)std::min((size_t)RL_CHUNK, n_groups - g0);
        unsigned int nr = 0;
        for (unsigned int i = 0; i <= RL_CHUNK; i++) {
            t.start[i] = nr;
            if (i < ng) nr += (unsigned int)gsize[g0 + i];
        }
        t.r.pkts = d_pkts + rec0 * stride; t.r.lens = d_lens ? d_lens + rec0 : nullptr; t.r.nrec = nr;
        t.rot = d_rot ? d_rot + 2 * rec0 : nullptr; t.out = d_out + g0;
        hipLaunchKernelGGL(qs_reloc_trail_points_kernel, dim3(ng), dim3(QS_WAVE), 0, c->stream, t, c->geom, pl.L.pts, pl.L.meta);
        HIPRET(hipGetLastError());
        if (n_tiles) {
            hipLaunchKernelGGL(qs_reloc_group_score_kernel<false>, dim3((unsigned int)n_tiles, ng), dim3(RL_BLOCK), lds, c->stream, c->geom, m, g);
            HIPRET(hipGetLastError());
        }
        hipLaunchKernelGGL(qs_reloc_pick_kernel, dim3(ng), dim3(RL_BLOCK), 0, c->stream, m);
        HIPRET(hipGetLastError());
        hipLaunchKernelGGL(qs_reloc_group_score_kernel<true>, dim3(9, ng), dim3(RL_BLOCK), lds, c->stream, c->geom, m, g);
        HIPRET(hipGetLastError());
        hipLaunchKernelGGL(qs_reloc_trail_final_kernel, dim3(ng), dim3(RL_BLOCK), 0, c->stream, c->geom, m, t, (const unsigned int *)pl.L.meta);
        HIPRET(hipGetLastError());
        rec0 += nr;
    }
    return hipSuccess;
}

// ---- C ABI: trail relocalisation (semantics in include/quasar_slam.h) -------------------------------------------------------------
extern "C" int qs_relocalise_trails_device(qs_ctx *c, const qs_reloc_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                           const uint16_t *d_lens, const int32_t *gsize, size_t n_groups, double travel,
                                           qs_trail_reloc *d_out, double *d_rot_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || d_pkts != nullptr);
    ARGCHK(c, n_groups == 0 || (gsize != nullptr && d_out != nullptr));
    QsRelocSetup rs;
    const int rc = reloc_trails_check(c, params, n, stride, gsize, n_groups, travel, rs);
    if (rc != QS_OK || n_groups == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, reloc_trail_launch(c, rs, d_pkts, stride, d_lens, gsize, n_groups, travel, d_out, d_rot_out));
    return QS_OK;
}

extern "C" int qs_relocalise_trails(qs_ctx *c, const qs_reloc_params *params, const uint8_t *pkts, size_t n, size_t stride,
                                    const uint16_t *lens, const int32_t *gsize, size_t n_groups, double travel, qs_trail_reloc *out,
                                    double *rot_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || pkts != nullptr);
    ARGCHK(c, n_groups == 0 || (gsize != nullptr && out != nullptr));
    QsRelocSetup rs;
    int rc = reloc_trails_check(c, params, n, stride, gsize, n_groups, travel, rs);
    if (rc != QS_OK || n_groups == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    size_t k0 = 0;
    for (size_t g0 = 0; g0 < n_groups; g0 += RL_CHUNK) {           // whole trails per round trip: one launch's worth
        const size_t ng = std::min((size_t)RL_CHUNK, n_groups - g0);
        size_t nk = 0;
        for (size_t g = g0; g < g0 + ng; g++) nk += (size_t)gsize[g];
        Staging s;
        rc = reserve_staging(c, nk * stride, s);
        if (rc != QS_OK) return rc;
        Carve cv(nullptr);
        cv.take<qs_trail_reloc>(ng);
        if (rot_out) cv.take<double>(2 * nk);
        HIPCHK(c, c->io_ws.reserve(cv.bytes, c->stream, QS_IO_WS_FLOOR));
        Carve io(c->io_ws.p);
        qs_trail_reloc *d_out = io.take<qs_trail_reloc>(ng);
        double *d_rot = rot_out ? io.take<double>(2 * nk) : nullptr;
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, nk * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, nk * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, reloc_trail_launch(c, rs, s.pkts, stride, lens ? s.lens : nullptr, gsize + g0, ng, travel, d_out, d_rot));
        HIPCHK(c, hipMemcpyAsync(out + g0, d_out, ng * sizeof(qs_trail_reloc), hipMemcpyDeviceToHost, c->stream));
        if (rot_out) HIPCHK(c, hipMemcpyAsync(rot_out + 2 * k0, d_rot, 2 * nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        k0 += nk;
    }
    return QS_OK;
}
