// checkpoint.hip -- the grid part of qs_checkpoint / qs_restore (format in include/quasar_slam.h, host side in qs_api.hip).
//
// A session writes a few rooms of a mostly empty world (3 % of the cells on configs[3]), so the file holds the grid as
// blocks of the sparse fuse's layout (QS_DIRTY_BLOCK_H x QS_DIRTY_BLOCK_W = 64 cells), and only the blocks that hold
// anything:
//   census   one coalesced pass over the saved planes -> a bitmap in the dirty-bitmap layout; the sparse fuse's list kernel
//            turns it into ascending block ids                                                         qs_ck_census_kernel
//   pack     one wave per listed block, one lane per cell: every saved plane of the block, in a fixed order   qs_ck_pack_kernel
//   unpack   the same walk the other way, into planes a reset has cleared                                   qs_ck_unpack_kernel
// A block is listed when any saved plane is nonzero in it (or, with tracking, its dirty bit is set).  Every writer of a cell
// sets its stamp, both fuses take the maximum of the stamps and a rebase keeps written cells nonzero, so the stamps alone
// would nearly do; but a local fold may bring counters without stamps (qs_fuse_buffers_range with stamps_dev == NULL), and
// such counters reach the peers' fused sums through a sparse fuse.  The census therefore reads every saved plane: the
// stamps at 4 B per cell, the counters at 8 B, the sparse fuse's two planes at 8 B each when tracking is on.
// All three are HBM streams: the census over the whole grid, pack and unpack over the listed blocks only.
#include <algorithm>

#include "qs_internal.h"

#define CK_CELLS (QS_DIRTY_BLOCK_W * QS_DIRTY_BLOCK_H)     // 64: one lane per cell

size_t qs_ck_block_bytes(int planes) { return CK_CELLS * (sizeof(unsigned int) + (size_t)(planes - 1) * sizeof(unsigned long long)); }

// ---- census: 4 cells per thread (one 16 B load of stamps, two of each 64-bit plane) ------------------------------------
__global__ void __launch_bounds__(256)
qs_ck_census_kernel(const uint4 *__restrict__ stamps, const ulonglong2 *__restrict__ counts, const ulonglong2 *__restrict__ sent,
                    const ulonglong2 *__restrict__ fused, int size, size_t quads, int pitch, unsigned int *__restrict__ bm)
{
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < quads; t += (size_t)gridDim.x * 256) {
        const uint4 s = stamps[t];
        bool nz = (s.x | s.y | s.z | s.w) != 0u;
        if (counts) { const ulonglong2 a = counts[2 * t], b = counts[2 * t + 1]; nz = nz || (a.x | a.y | b.x | b.y) != 0ull; }
        if (sent) { const ulonglong2 a = sent[2 * t], b = sent[2 * t + 1]; nz = nz || (a.x | a.y | b.x | b.y) != 0ull; }
        if (fused) { const ulonglong2 a = fused[2 * t], b = fused[2 * t + 1]; nz = nz || (a.x | a.y | b.x | b.y) != 0ull; }
        if (nz) {                                              // (size % 4 == 0: the 4 cells lie in one row and one block)
            const size_t cell = 4 * t;
            const int y = (int)(cell / (size_t)size), x = (int)(cell % (size_t)size);
            atomicOr(&bm[qs_dirty_word(x, y, pitch)], qs_dirty_mask(x));
        }
    }
}
hipError_t qs_launch_ck_census(qs_ctx *c, unsigned int *bitmap, size_t words, int pitch, int blocks_x, unsigned int *list,
                               unsigned int *count)
{
    const size_t nb = words * sizeof(unsigned int);
    // tracking on: the live dirty bitmap (same geometry) is where the census starts -- blocks marked but all zero included
    hipError_t e = c->d_dirty.p ? hipMemcpyAsync(bitmap, c->d_dirty.p, nb, hipMemcpyDeviceToDevice, c->stream)
                              : hipMemsetAsync(bitmap, 0, nb, c->stream);
    if (e != hipSuccess) return e;
    const size_t quads = c->cells / 4;
    const bool sparse = c->d_dirty.p && c->d_counts.p;
    const unsigned int blocks = (unsigned int)std::min<size_t>((quads + 255) / 256, 2048);
    hipLaunchKernelGGL(qs_ck_census_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint4 *)c->d_stamps.p,
                       (const ulonglong2 *)c->d_counts.p, (const ulonglong2 *)(sparse ? c->d_counts_sent.p : nullptr),
                       (const ulonglong2 *)(sparse ? c->d_counts_fused.p : nullptr), c->cfg.size, quads, pitch, bitmap);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return qs_launch_sf_list_of(c, bitmap, words, pitch, blocks_x, list, count);
}

// ---- pack / unpack: one wave per block, one lane per cell.  Block layout: stamps u32[64], then (planes >= 2) counters
// u64[64], then (planes == 4) sent u64[64], fused u64[64].  Lanes beyond the grid's right edge pack 0 and unpack nothing ----
__global__ void __launch_bounds__(256)
qs_ck_pack_kernel(const unsigned int *__restrict__ list, unsigned int n_blocks, int pitch, int size, int planes,
                  const unsigned int *__restrict__ stamps, const unsigned long long *__restrict__ counts,
                  const unsigned long long *__restrict__ sent, const unsigned long long *__restrict__ fused,
                  unsigned char *__restrict__ dst)
{
    const int lane = threadIdx.x & (QS_WAVE - 1);
    const unsigned int wave = blockIdx.x * (256 / QS_WAVE) + (threadIdx.x >> 6), n_waves = gridDim.x * (256 / QS_WAVE);
    const size_t bb = CK_CELLS * (4 + 8 * (size_t)(planes - 1));
    for (unsigned int k = wave; k < n_blocks; k += n_waves) {
        size_t cell;
        const bool in = qs_block_cell(list[k], lane, pitch, size, cell);
        unsigned char *blk = dst + (size_t)k * bb;
        ((unsigned int *)blk)[lane] = in ? stamps[cell] : 0u;
        unsigned long long *q = (unsigned long long *)(blk + CK_CELLS * 4);
        if (planes >= 2) q[lane] = in ? counts[cell] : 0ull;
        if (planes >= 4) { q[CK_CELLS + lane] = in ? sent[cell] : 0ull; q[2 * CK_CELLS + lane] = in ? fused[cell] : 0ull; }
    }
}

__global__ void __launch_bounds__(256)
qs_ck_unpack_kernel(const unsigned int *__restrict__ list, unsigned int n_blocks, int pitch, int size, int planes,
                    const unsigned char *__restrict__ src, unsigned int *__restrict__ stamps, unsigned long long *__restrict__ counts,
                    unsigned long long *__restrict__ sent, unsigned long long *__restrict__ fused)
{
    const int lane = threadIdx.x & (QS_WAVE - 1);
    const unsigned int wave = blockIdx.x * (256 / QS_WAVE) + (threadIdx.x >> 6), n_waves = gridDim.x * (256 / QS_WAVE);
    const size_t bb = CK_CELLS * (4 + 8 * (size_t)(planes - 1));
    for (unsigned int k = wave; k < n_blocks; k += n_waves) {
        size_t cell;
        if (!qs_block_cell(list[k], lane, pitch, size, cell)) continue;
        const unsigned char *blk = src + (size_t)k * bb;
        stamps[cell] = ((const unsigned int *)blk)[lane];
        const unsigned long long *q = (const unsigned long long *)(blk + CK_CELLS * 4);
        if (planes >= 2) counts[cell] = q[lane];
        if (planes >= 4) { sent[cell] = q[CK_CELLS + lane]; fused[cell] = q[2 * CK_CELLS + lane]; }
    }
}

// (block ids are checked on the host before either launch: ascending, and inside the grid's bitmap)
hipError_t qs_launch_ck_pack(qs_ctx *c, const unsigned int *list, unsigned int n_blocks, int pitch, int planes, unsigned char *dst)
{
    if (n_blocks == 0) return hipSuccess;
    const unsigned int blocks = (n_blocks + 3) / 4 < 4096 ? (n_blocks + 3) / 4 : 4096;
    hipLaunchKernelGGL(qs_ck_pack_kernel, dim3(blocks), dim3(256), 0, c->stream, list, n_blocks, pitch, c->cfg.size, planes,
                       c->d_stamps.p, c->d_counts.p, c->d_counts_sent.p, c->d_counts_fused.p, dst);
    return hipGetLastError();
}
hipError_t qs_launch_ck_unpack(qs_ctx *c, const unsigned int *list, unsigned int n_blocks, int pitch, int planes,
                               const unsigned char *src)
{
    if (n_blocks == 0) return hipSuccess;
    const unsigned int blocks = (n_blocks + 3) / 4 < 4096 ? (n_blocks + 3) / 4 : 4096;
    hipLaunchKernelGGL(qs_ck_unpack_kernel, dim3(blocks), dim3(256), 0, c->stream, list, n_blocks, pitch, c->cfg.size, planes, src,
                       c->d_stamps.p, c->d_counts.p, c->d_counts_sent.p, c->d_counts_fused.p);
    return hipGetLastError();
}
