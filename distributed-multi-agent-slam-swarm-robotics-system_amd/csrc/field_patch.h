// field_patch.h -- a square patch of the likelihood field (include/quasar_slam.h, "sweep matching", rule 1) built in LDS by one
// workgroup, the look-up of four adjacent cells of it, and the workgroup's maximum of a 64-bit key: shared by the window search of
// the sweep and trail matchers (window_match.h) and the relocaliser (reloc.hip).
#pragma once
#include "qs_internal.h"

__device__ inline bool mt_occupied(unsigned int stamp) { return (stamp & 1u) != 0; }     // (UNKNOWN is 0: even)

// bytewise max of three dwords
__device__ inline unsigned int mt_max3_u8x4(unsigned int a, unsigned int b, unsigned int c)
{
    unsigned int r = 0;
    #pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned int s = 8u * j;
        r |= max(max((a >> s) & 255u, (b >> s) & 255u), (c >> s) & 255u) << s;
    }
    return r;
}
// one round's new value per byte: max(old, m - 1) with m - 1 saturating at 0
__device__ inline unsigned int mt_grow_u8x4(unsigned int old, unsigned int m)
{
    unsigned int r = 0;
    #pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned int s = 8u * j, v = (m >> s) & 255u;
        r |= max((old >> s) & 255u, v ? v - 1u : 0u) << s;
    }
    return r;
}

// four adjacent field bytes from byte offset a of the patch
__device__ inline unsigned int mt_look(const unsigned int *p, unsigned int a)
{
    return __builtin_amdgcn_alignbyte(p[(a >> 2) + 1], p[a >> 2], a & 3u);
}

// max of v over the workgroup's nw waves, returned in thread 0 (other threads get their wave's): shuffles within the wave,
// s_key[nw] across the waves.  Every thread calls it, once per s_key; it holds one barrier
__device__ __forceinline__ unsigned long long mt_block_max(unsigned long long v, unsigned long long *s_key, int tid, int nw)
{
    #pragma unroll
    for (int d = QS_WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long other = __shfl_xor(v, d);
        v = other > v ? other : v;
    }
    if ((tid & (QS_WAVE - 1)) == 0) s_key[tid >> 6] = v;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < nw; w++) v = s_key[w] > v ? s_key[w] : v;
    return v;
}

// The patch whose byte (0, 0) is grid cell (gx0, gy0): SA cells a side, rows of `pitch` bytes (a multiple of 4), into A; B is
// scratch of the same size.  Bytes come from the stamps (OCCUPIED = odd stamp -> R + 1, anything else and off-grid -> 0) and
// are grown by R rounds of a separable 3-wide max that loses 1 per round, so the cells at least R inside the patch's edge hold
// L = max(0, R + 1 - Chebyshev distance).  The rounds work on dwords (four cells a lane); a patch that hangs over the grid's
// edge is cut back to the grid afterwards.  A[nd .. nd + 4) are zeroed: a look-up reads one dword ahead.  Every thread of the
// workgroup (`block` of them) calls it; it ends on a barrier.
__device__ __forceinline__ void mt_build_patch(unsigned int *A, unsigned int *B, const unsigned int *stamps, int size, int gx0, int gy0,
                                               int SA, int pitch, int R, int tid, int block)
{
    const int pd = pitch >> 2, nd = SA * pd;
    const unsigned int seed = (unsigned int)R + 1u;
    for (int i = tid; i < nd + 4; i += block) {
        unsigned int v = 0;
        if (i < nd) {
            const int y = i / pd, x4 = 4 * (i - y * pd), gy = gy0 + y;
            if (gy >= 0 && gy < size) {
                const unsigned int *row = stamps + (size_t)gy * size;
                #pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int x = x4 + j, gx = gx0 + x;
                    if (x < SA && gx >= 0 && gx < size && mt_occupied(row[gx])) v |= seed << (8 * j);
                }
            }
        }
        A[i] = v;
    }
    __syncthreads();
    for (int r = 0; r < R; r++) {
        for (int i = tid; i < nd; i += block) {                    // along x: A -> B
            const int y = i / pd, xd = i - y * pd;
            const unsigned int cur = A[i], prev = xd > 0 ? A[i - 1] : 0u, next = xd < pd - 1 ? A[i + 1] : 0u;
            B[i] = mt_max3_u8x4(__builtin_amdgcn_alignbyte(cur, prev, 3), cur, __builtin_amdgcn_alignbyte(next, cur, 1));
        }
        __syncthreads();
        for (int i = tid; i < nd; i += block) {                    // along y, minus one: B -> A
            const unsigned int up = i >= pd ? B[i - pd] : 0u, dn = i + pd < nd ? B[i + pd] : 0u;
            A[i] = mt_grow_u8x4(A[i], mt_max3_u8x4(up, B[i], dn));
        }
        __syncthreads();
    }

    if (R > 0 && (gx0 < 0 || gy0 < 0 || gx0 + SA > size || gy0 + SA > size)) {   // (uniform)
        // the patch hangs over the grid's edge: L is 0 out there, whatever the rounds grew into it (a shortest Chebyshev
        // path between two cells of the grid never needs to leave it, so the cells inside are already right)
        for (int i = tid; i < nd; i += block) {
            const int y = i / pd, x4 = 4 * (i - y * pd), gy = gy0 + y;
            unsigned int keep = 0;
            if (gy >= 0 && gy < size) {
                #pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int gx = gx0 + x4 + j;
                    if (gx >= 0 && gx < size) keep |= 0xffu << (8 * j);
                }
            }
            A[i] &= keep;
        }
        __syncthreads();
    }
}
