// window_match.h -- the window search of sweep matching and trail matching (include/quasar_slam.h under those headings), once:
// a set of points held rigidly together -- a sweep's hit beams (match.hip), a trail's hit points (trail.hip) -- is shifted by
// ix, iy cells and turned by it angle steps, every candidate is scored on a patch of the likelihood field (field_patch.h), and the
// best under the rule's total order is the correction.  One WORKGROUP of WM_BLOCK threads per set, everything in dynamic LDS:
//   region A   the patch: the centre's cell +- (half + R) cells, half = reach + 1 + W, rows of wm_pitch bytes;
//   region B   the dilation's scratch, then per rotation a list of 16-bit patch offsets, one per point whose cell every shift
//              of the window keeps inside the exact part of the patch (the offset of candidate ix = iy = -W).
// A caller stages its points, calls wm_build_patch, lists each rotation's end points with wm_list (a wave per rotation), and
// after a barrier calls wm_best and, in one thread, wm_result.  The host sizes the LDS with wm_args.
#pragma once
#include <algorithm>

#include "field_patch.h"

#define WM_BLOCK 256
#define WM_NW (WM_BLOCK / QS_WAVE)
#define WM_NROT_MAX (2 * QS_MATCH_MAX_ANGLE_STEPS + 1)

// what a launch fixes for every workgroup (wm_args).  The device functions take it by value: a reference into the kernel's
// argument block costs qs_trail_kernel two VGPRs
struct WmArgs {
    int R, W, T, min_hits, min_percent;
    int half;                     // the largest patch: the centre's cell +- half, half = reach + 1 + W (a workgroup may build a smaller one)
    unsigned int off_b;           // byte offset of region B
    double step;
    const unsigned int *stamps;
};

// the patch a workgroup built: SA cells a side with the apron, rows of `pitch` bytes, byte (0, 0) at grid cell (gx0, gy0);
// c0ok: the centre has a cell at all (if not, no point has one either and nothing reads the patch)
struct WmPatch { int R, W, T, SA, pitch, gx0, gy0; bool c0ok; };

// Bytes per row of a patch SA cells a side: a multiple of 4 and an odd number of dwords, so that rows start on different banks
// -- unless the largest offset a rotation's list can hold would then pass 16 bits.  A listed cell lies in [R + W, SA - 1 - R - W]
// on both axes and its offset is that of candidate ix = iy = -W, so the largest is (SA - 1 - R - 2 W) (pitch + 1).  SA <= 253
// (qs_match_reach_setup), and only that widest patch with R = W = 0 gets there (252 * 261 = 65 772): it keeps the unpadded pitch,
// rows of 256 bytes (252 * 257 = 64 764).  Kernel and launch both ask here, so the LDS the launch sizes is what the kernel lays
// out; SA * wm_pitch(SA) does not shrink as SA grows, so a workgroup's smaller patch fits the launch's.
__host__ __device__ inline int wm_pitch(int SA, int R, int W)
{
    const int flat = (SA + 3) & ~3, odd = ((flat >> 2) & 1) ? flat : flat + 4;
    return (SA - 1 - R - 2 * W) * (odd + 1) <= 0xffff ? odd : flat;
}

// w from a checked setup, and the dynamic LDS of a launch of `kernel` whose rotations list up to offp offsets each (a multiple
// of 4: 8-byte reads): region A with 16 bytes more (a look-up reads one dword ahead), region B the larger of its two uses
inline hipError_t wm_args(const qs_ctx *c, const QsMatchSetup &ms, const void *kernel, int offp, WmArgs &w, size_t &lds)
{
    w.R = ms.R; w.W = ms.W; w.T = ms.T; w.min_hits = ms.min_hits; w.min_percent = ms.min_percent;
    w.half = ms.reach + 1 + ms.W;
    const int SA = 2 * (w.half + ms.R) + 1;
    const size_t patch = (size_t)SA * wm_pitch(SA, ms.R, ms.W);
    const size_t a_bytes = (patch + 16 + 15) & ~(size_t)15;
    const size_t b_bytes = std::max(patch, (size_t)(2 * ms.T + 1) * offp * sizeof(unsigned short));
    w.off_b = (unsigned int)a_bytes;
    w.step = ms.step;
    w.stamps = c->d_stamps.p;
    lds = a_bytes + ((b_bytes + 15) & ~(size_t)15);
    if (lds > 32 * 1024)                                           // the largest windows: up to 2 x 65 KiB of the CU's 160
        return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return hipSuccess;
}

// the patch about the cell of (x, y), +- half cells (at most w.half) and the apron, into A with B as scratch.  Every thread of
// the workgroup calls it with the same x, y and half; it ends on a barrier
__device__ __forceinline__ WmPatch wm_build_patch(const WmArgs w, const QsGeom &geo, double x, double y, int half, unsigned int *A,
                                                  unsigned int *B, int tid)
{
    WmPatch p;
    p.R = w.R; p.W = w.W; p.T = w.T;
    half = __builtin_amdgcn_readfirstlane(half);
    p.SA = 2 * (half + w.R) + 1;
    p.pitch = wm_pitch(p.SA, w.R, w.W);
    int c0x = 0, c0y = 0;
    p.c0ok = qs_w2g_i32(x, geo.ox, geo, c0x);
    p.c0ok = qs_w2g_i32(y, geo.oy, geo, c0y) && p.c0ok;
    if (!p.c0ok) { c0x = 0; c0y = 0; }
    c0x = __builtin_amdgcn_readfirstlane(c0x); c0y = __builtin_amdgcn_readfirstlane(c0y);   // (the same in every lane: scalar registers)
    p.gx0 = c0x - half - w.R; p.gy0 = c0y - half - w.R;            // grid cell of patch byte (0, 0); |c0| <= 2^30
    mt_build_patch(A, B, w.stamps, geo.size, p.gx0, p.gy0, p.SA, p.pitch, w.R, tid, WM_BLOCK);
    return p;
}

// One round of a rotation's list o, every lane of the wave: a lane with a point (live) whose end (ex, ey) has a cell every shift
// of which stays inside the exact part of the patch appends that cell's offset, compacted by ballot.  cnt: the list's length
__device__ __forceinline__ void wm_list(const WmPatch &p, const QsGeom &geo, bool live, double ex, double ey, unsigned short *o, int &cnt,
                                        int lane)
{
    bool in = false;
    unsigned int off = 0;
    if (live) {
        int cx, cy;
        bool ok = qs_w2g_i32(ex, geo.ox, geo, cx);
        ok = qs_w2g_i32(ey, geo.oy, geo, cy) && ok;
        if (ok && p.c0ok) {
            const int lo_ok = p.R + p.W, hi_ok = p.SA - 1 - p.R - p.W;
            const long long ax = (long long)cx - p.gx0, ay = (long long)cy - p.gy0;
            in = ax >= lo_ok && ax <= hi_ok && ay >= lo_ok && ay <= hi_ok;
            off = (unsigned int)((ay - p.W) * p.pitch + (ax - p.W));
        }
    }
    const unsigned long long bal = __ballot(in);
    if (in) o[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)off;
    cnt += __popcll(bal);
}

// the rule's total order as one key: score, then small ix^2 + iy^2, small |it|, small it, small iy, small ix -- every field
// "larger is better"
__device__ inline unsigned long long wm_key(unsigned int score, int ix, int iy, int it, int W, int T)
{
    return ((unsigned long long)score << 45) | ((unsigned long long)(32767 - (ix * ix + iy * iy)) << 30)
         | ((unsigned long long)(T - abs(it)) << 23) | ((unsigned long long)(T - it) << 16)
         | ((unsigned long long)(W - iy) << 8) | (unsigned long long)(W - ix);
}

// The scores of every candidate and the workgroup's best key, in thread 0.  OFF: the lists, offp entries apart, s_cnt their
// lengths (both written before a barrier); *s_score0 gets the score of candidate (0, 0, 0), readable when the call returns.
// A lane takes (rotation, iy, FOUR adjacent ix): per point two dword reads and a v_alignbyte give the four look-ups, which are
// summed as bytes (255 / (R + 1) points at a time cannot overflow one) and spilled into 16-bit sums; the offsets are read four
// at a time (one 8-byte read).  Per four look-ups: 2.25 LDS reads and about six VALU instructions
__device__ __forceinline__ unsigned long long wm_best(const WmPatch &p, const unsigned int *A, const unsigned short *OFF, int offp,
                                                      const int *s_cnt, unsigned long long *s_key, int *s_score0, int tid)
{
    const int ny = 2 * p.W + 1, G = (ny + 3) >> 2, per_rot = ny * G, NI = (2 * p.T + 1) * per_rot;
    const int span = (255 / (p.R + 1)) & ~3;                       // points whose byte sums cannot overflow
    unsigned long long best = 0;
    for (int j = tid; j < NI; j += WM_BLOCK) {
        const int ti = j / per_rot, rem = j - ti * per_rot, yi = rem / G, g = rem - yi * G;
        const unsigned int lane_off = (unsigned int)(yi * p.pitch + 4 * g);
        const unsigned short *o = OFF + ti * offp;
        const int cnt = s_cnt[ti];
        unsigned int lo = 0, hi = 0;
        for (int b0 = 0; b0 < cnt; b0 += span) {
            const int b1 = min(b0 + span, cnt);
            unsigned int acc = 0;
            int b = b0;
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
        const unsigned int sc[4] = {lo & 0xffffu, hi & 0xffffu, lo >> 16, hi >> 16};
        const int it = ti - p.T, iy = yi - p.W;
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            const int ix = 4 * g + e - p.W;
            if (ix > p.W) break;
            const unsigned long long key = wm_key(sc[e], ix, iy, it, p.W, p.T);
            best = key > best ? key : best;
            if (it == 0 && iy == 0 && ix == 0) *s_score0 = (int)sc[e];
        }
    }
    return mt_block_max(best, s_key, tid, WM_NW);                  // (its barrier hands *s_score0 over too)
}

// the fields qs_sweep_match and qs_trail_match share, from the best key, the score of (0, 0, 0) and the H hit points: the
// candidate, the gate (rule 5 of sweep matching) and the correction an accepted match yields (r comes in zeroed)
template <typename OUT>
__device__ inline void wm_result(const WmArgs w, double res, unsigned long long best, int score0, int H, OUT &r)
{
    r.ix = w.W - (int)(best & 255u);
    r.iy = w.W - (int)((best >> 8) & 255u);
    r.it = w.T - (int)((best >> 16) & 127u);
    r.score = (int)(best >> 45);
    r.score0 = score0;
    r.hits = H;
    r.accepted_match = H >= w.min_hits && (long long)r.score * 100 >= (long long)w.min_percent * H * (w.R + 1);
    if (r.accepted_match) { r.dx = (double)r.ix * res; r.dy = (double)r.iy * res; r.dyaw = (double)r.it * w.step; }
}
