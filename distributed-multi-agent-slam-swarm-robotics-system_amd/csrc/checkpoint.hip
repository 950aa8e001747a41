// checkpoint.hip -- qs_checkpoint / qs_restore (format in include/quasar_slam.h): the file on the host, the grid on the device.
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
#include <mutex>
#include <stdio.h>
#include <string.h>

#include "qs_internal.h"

#define CK_CELLS (QS_DIRTY_BLOCK_W * QS_DIRTY_BLOCK_H)     // 64: one lane per cell

// bytes of one saved block; planes 1 = stamps, 2 = + counters, 4 = + sent + fused
static size_t qs_ck_block_bytes(int planes) { return CK_CELLS * (sizeof(unsigned int) + (size_t)(planes - 1) * sizeof(unsigned long long)); }

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
static hipError_t qs_launch_ck_census(qs_ctx *c, unsigned int *bitmap, size_t words, int pitch, int blocks_x, unsigned int *list,
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
static hipError_t qs_launch_ck_pack(qs_ctx *c, const unsigned int *list, unsigned int n_blocks, int pitch, int planes, unsigned char *dst)
{
    if (n_blocks == 0) return hipSuccess;
    const unsigned int blocks = (n_blocks + 3) / 4 < 4096 ? (n_blocks + 3) / 4 : 4096;
    hipLaunchKernelGGL(qs_ck_pack_kernel, dim3(blocks), dim3(256), 0, c->stream, list, n_blocks, pitch, c->cfg.size, planes,
                       c->d_stamps.p, c->d_counts.p, c->d_counts_sent.p, c->d_counts_fused.p, dst);
    return hipGetLastError();
}
static hipError_t qs_launch_ck_unpack(qs_ctx *c, const unsigned int *list, unsigned int n_blocks, int pitch, int planes,
                                      const unsigned char *src)
{
    if (n_blocks == 0) return hipSuccess;
    const unsigned int blocks = (n_blocks + 3) / 4 < 4096 ? (n_blocks + 3) / 4 : 4096;
    hipLaunchKernelGGL(qs_ck_unpack_kernel, dim3(blocks), dim3(256), 0, c->stream, list, n_blocks, pitch, c->cfg.size, planes, src,
                       c->d_stamps.p, c->d_counts.p, c->d_counts_sent.p, c->d_counts_fused.p);
    return hipGetLastError();
}

// ---- C ABI: checkpoint / restore (format and contract in include/quasar_slam.h) --------------------------------------
// The file's body (everything after the header) is assembled in one device buffer (qs_ctx::ck_stage) -- bots, counters,
// logs and block ids by device-to-device copies, the blocks by the pack kernel -- and crosses to the host in one copy; the
// host fills in the parts it holds (scalars, graph sizes) and the header.  A restore sends the body back in one copy and
// scatters it the same way.
static uint32_t ck_crc32(const uint8_t *p, size_t n)       // zlib's CRC-32 (reflected 0xEDB88320), slicing by 8
{
    static uint32_t T[8][256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            T[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < 8; s++) T[s][i] = (T[s - 1][i] >> 8) ^ T[0][T[s - 1][i] & 0xff];
    });
    uint32_t c = 0xffffffffu;
    while (n >= 8) {
        uint32_t a, b;
        memcpy(&a, p, 4); memcpy(&b, p + 4, 4);
        a ^= c;
        c = T[7][a & 0xff] ^ T[6][(a >> 8) & 0xff] ^ T[5][(a >> 16) & 0xff] ^ T[4][a >> 24] ^
            T[3][b & 0xff] ^ T[2][(b >> 8) & 0xff] ^ T[1][(b >> 16) & 0xff] ^ T[0][b >> 24];
        p += 8; n -= 8;
    }
    while (n--) c = T[0][(c ^ *p++) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

static size_t ck_pad8(size_t v) { return (v + 7) & ~(size_t)7; }
template <typename T> static void ck_put(uint8_t *b, size_t off, T v) { memcpy(b + off, &v, sizeof v); }
template <typename T> static T ck_get(const uint8_t *b, size_t off) { T v; memcpy(&v, b + off, sizeof v); return v; }

static const size_t CK_SCALARS_BYTES = 72;
static size_t ck_graph_bytes(long long L, long long C) { return 24 * (size_t)L + ck_pad8((size_t)L) + 32 * (size_t)C + ck_pad8((size_t)C); }
static size_t ck_bots_bytes(int nb) { return (size_t)nb * (1 + 2 + 1 + 4 + 44 + 4) * 8; }

// block geometry of the dirty bitmap (whether tracking is on or not)
struct CkGeom { int blocks_x, blocks_y, pitch; size_t words; };
static CkGeom ck_geom(const qs_ctx *c)
{
    CkGeom g;
    g.blocks_x = (c->cfg.size + QS_DIRTY_BLOCK_W - 1) / QS_DIRTY_BLOCK_W;
    g.blocks_y = (c->cfg.size + QS_DIRTY_BLOCK_H - 1) / QS_DIRTY_BLOCK_H;
    g.pitch = (g.blocks_x + 31) / 32;
    g.words = (size_t)g.blocks_y * g.pitch;
    return g;
}

// where the sections of a body lie: [kind] -> (offset, length), offsets from the start of the file
struct CkLayout {
    size_t off[QS_CKPT_DIRTY + 1] = {0}, len[QS_CKPT_DIRTY + 1] = {0};
    size_t header_bytes = 0, total = 0;
    int n_sections = 0;
};
static CkLayout ck_layout(int nb, int n_graphs, const std::vector<long long> &L, const std::vector<long long> &C, size_t n_blocks,
                          size_t block_bytes, bool tracking, size_t dirty_words)
{
    CkLayout y;
    y.n_sections = tracking ? 7 : 6;
    y.header_bytes = QS_CKPT_HEADER_FIXED + 24 * (size_t)y.n_sections;
    y.len[QS_CKPT_SCALARS] = CK_SCALARS_BYTES;
    y.len[QS_CKPT_BOTS] = ck_bots_bytes(nb);
    y.len[QS_CKPT_COUNTERS] = QS_CNT_N * 8;
    size_t gb = (size_t)n_graphs * 24;
    for (int g = 0; g < n_graphs; g++) gb += ck_graph_bytes(L[g], C[g]);
    y.len[QS_CKPT_GRAPHS] = gb;
    y.len[QS_CKPT_BLOCK_IDS] = 4 * n_blocks;
    y.len[QS_CKPT_BLOCKS] = n_blocks * block_bytes;
    y.len[QS_CKPT_DIRTY] = tracking ? 4 * dirty_words : 0;
    size_t at = y.header_bytes;
    for (int k = QS_CKPT_SCALARS; k <= (tracking ? QS_CKPT_DIRTY : QS_CKPT_BLOCKS); k++) { y.off[k] = at; at += ck_pad8(y.len[k]); }
    y.total = at;
    return y;
}

// the configuration fields a checkpoint must agree on (include/quasar_slam.h), at their header offsets
struct CkField { const char *name; int off; bool is_f64; };
static const CkField CK_FIELDS[] = {
    {"size", 32, false}, {"min_poses_between", 36, false}, {"max_agent", 40, false}, {"bots_per_graph", 44, false},
    {"enable_counts", 48, false}, {"enable_ekf", 52, false}, {"seq_stride", 56, false}, {"shard_bots", 60, false},
    {"shard_rank", 64, false}, {"exact_trig", 68, false},
    {"res", 80, true}, {"ox", 88, true}, {"oy", 96, true}, {"min_dist", 104, true}, {"max_dist", 112, true},
    {"closure_radius", 120, true}, {"closure_correction", 128, true}, {"ekf_metres_per_tick", 136, true}};
static void ck_put_config(uint8_t *h, const qs_config &cf, bool tracking)
{
    const int32_t iv[12] = {cf.size, cf.min_poses_between, cf.max_agent, cf.bots_per_graph, cf.enable_counts ? 1 : 0,
                            cf.enable_ekf ? 1 : 0, cf.seq_stride, cf.shard_bots, cf.shard_rank, cf.exact_trig ? 1 : 0,
                            tracking ? 1 : 0, 0};
    const double dv[8] = {cf.res, cf.ox, cf.oy, cf.min_dist, cf.max_dist, cf.closure_radius, cf.closure_correction,
                          cf.ekf_metres_per_tick};
    memcpy(h + 32, iv, sizeof iv);
    memcpy(h + 80, dv, sizeof dv);
}

static int ck_planes(bool counts, bool tracking) { return !counts ? 1 : (tracking ? 4 : 2); }

extern "C" int qs_checkpoint(qs_ctx *c, uint8_t *buf, size_t cap, size_t *n_out)
{
    ARGCHK(c, c != nullptr && n_out != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->sf_state != 0) return qs_fail(c, QS_E_STATE, "qs_checkpoint: a sparse fuse is in flight (finish it with qs_sparse_fuse_apply)");
    SYNCCHK(c);                                             // waiting exact-trig rays go into the saved grid
    unsigned long long cnt[QS_CNT_N];
    std::vector<QsGraphDev> cur((size_t)c->n_graphs);
    HIPCHK(c, hipMemcpyAsync(cnt, c->d_counters.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cur.data(), c->d_graphs.p, cur.size() * sizeof(QsGraphDev), hipMemcpyDeviceToHost, c->stream));
    // census: the blocks that hold anything, listed on the device
    const CkGeom gm = ck_geom(c);
    HIPCHK(c, c->ck_census.reserve(gm.words * 33 + 1, c->stream));
    unsigned int *d_bm = c->ck_census.p, *d_list = d_bm + gm.words, *d_count = d_list + gm.words * 32;
    HIPCHK(c, qs_launch_ck_census(c, d_bm, gm.words, gm.pitch, gm.blocks_x, d_list, d_count));
    unsigned int n_blk = 0;
    HIPCHK(c, hipMemcpyAsync(&n_blk, d_count, sizeof n_blk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (cnt[QS_CNT_SLAM_ROUNDS] >> 40)
        return qs_fail(c, QS_E_STATE, "qs_checkpoint: a loop-closure chain wait timed out (bit 40 of QS_CNT_SLAM_ROUNDS): the map may be wrong");
    const bool tracking = c->d_dirty.p != nullptr;
    const int planes = ck_planes(c->d_counts.p != nullptr, tracking), nb = c->cfg.max_agent + 1, G = c->n_graphs;
    std::vector<long long> L(G), C(G);
    for (int g = 0; g < G; g++) {
        L[g] = cur[g].n_lms; C[g] = cur[g].n_cls;
        if (L[g] > cur[g].cap_lms || C[g] > cur[g].cap_cls)
            return qs_fail(c, QS_E_STATE, "qs_checkpoint: a pose graph's log outgrew its capacity: the map may be wrong");
    }
    const CkLayout y = ck_layout(nb, G, L, C, n_blk, qs_ck_block_bytes(planes), tracking, gm.words);
    *n_out = y.total;
    if (!buf) return QS_OK;
    if (cap < y.total) return qs_fail(c, QS_E_RANGE, "qs_checkpoint: cap is below the checkpoint's size (query it with buf == NULL)");
    // the body on the device, offsets relative to header_bytes
    const size_t hb = y.header_bytes, body = y.total - hb;
    HIPCHK(c, c->ck_stage.reserve(body, c->stream));
    unsigned char *st = c->ck_stage.p;
    auto d2d = [&](size_t off, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(st + off - hb, src, bytes, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    };
    {
        size_t o = y.off[QS_CKPT_BOTS];
        HIPCHK(c, d2d(o, c->d_offset.p, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(o, c->d_drift.p, nb * 16)); o += nb * 16;
        HIPCHK(c, d2d(o, c->d_last_closure.p, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(o, c->d_zone.p, nb * 32)); o += nb * 32;
        HIPCHK(c, d2d(o, c->d_ekf.p, (size_t)nb * 44 * 8)); o += (size_t)nb * 44 * 8;
        HIPCHK(c, d2d(o, c->d_ekf_prev.p, nb * 32));
    }
    HIPCHK(c, d2d(y.off[QS_CKPT_COUNTERS], c->d_counters.p, QS_CNT_N * 8));
    {
        size_t o = y.off[QS_CKPT_GRAPHS] + (size_t)G * 24;
        for (int g = 0; g < G; g++) {
            const QsGraphDev &q = cur[g];
            const size_t l = (size_t)L[g], k = (size_t)C[g];
            HIPCHK(c, d2d(o, q.lm_x, 8 * l)); HIPCHK(c, d2d(o + 8 * l, q.lm_y, 8 * l)); HIPCHK(c, d2d(o + 16 * l, q.lm_idx, 8 * l));
            HIPCHK(c, d2d(o + 24 * l, q.lm_type, l));
            o += 24 * l + ck_pad8(l);
            HIPCHK(c, d2d(o, q.cl_lm_idx, 8 * k)); HIPCHK(c, d2d(o + 8 * k, q.cl_node_idx, 8 * k));
            HIPCHK(c, d2d(o + 16 * k, q.cl_dx, 8 * k)); HIPCHK(c, d2d(o + 24 * k, q.cl_dy, 8 * k));
            HIPCHK(c, d2d(o + 32 * k, q.cl_agent, k));
            o += 32 * k + ck_pad8(k);
        }
    }
    HIPCHK(c, d2d(y.off[QS_CKPT_BLOCK_IDS], d_list, 4 * (size_t)n_blk));
    HIPCHK(c, qs_launch_ck_pack(c, d_list, n_blk, gm.pitch, planes, st + y.off[QS_CKPT_BLOCKS] - hb));
    if (tracking) HIPCHK(c, d2d(y.off[QS_CKPT_DIRTY], c->d_dirty.p, 4 * gm.words));
    memset(buf, 0, hb);
    HIPCHK(c, hipMemcpyAsync(buf + hb, st, body, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // what the host holds, then the header
    {
        uint8_t *s = buf + y.off[QS_CKPT_SCALARS];
        memset(s, 0, ck_pad8(CK_SCALARS_BYTES));
        ck_put<uint64_t>(s, 0, c->next_seq); ck_put<uint64_t>(s, 8, c->epoch_base); ck_put<uint64_t>(s, 16, c->n_rebases);
        ck_put<uint64_t>(s, 24, c->edge_rays_total); ck_put<uint64_t>(s, 32, c->edge_overflow_total);
        ck_put<double>(s, 40, c->sweep_min); ck_put<double>(s, 48, c->sweep_max);
        ck_put<uint32_t>(s, 56, c->dirty_since_fuse ? 1u : 0u); ck_put<uint32_t>(s, 60, c->counts_view_fused ? 1u : 0u);
        ck_put<uint32_t>(s, 64, (uint32_t)G); ck_put<uint32_t>(s, 68, (uint32_t)nb);
        uint8_t *gh = buf + y.off[QS_CKPT_GRAPHS];
        for (int g = 0; g < G; g++) {
            ck_put<int64_t>(gh, 24 * g, cur[g].n_nodes); ck_put<int64_t>(gh, 24 * g + 8, L[g]); ck_put<int64_t>(gh, 24 * g + 16, C[g]);
        }
        // padding after the host-side arrays and the byte arrays: zeros, so that equal sessions give equal files
        for (int k = QS_CKPT_SCALARS; k <= QS_CKPT_DIRTY; k++)
            if (y.off[k]) memset(buf + y.off[k] + y.len[k], 0, ck_pad8(y.len[k]) - y.len[k]);
        size_t o = y.off[QS_CKPT_GRAPHS] + (size_t)G * 24;
        for (int g = 0; g < G; g++) {
            const size_t l = (size_t)L[g], k = (size_t)C[g];
            memset(buf + o + 24 * l + l, 0, ck_pad8(l) - l); o += 24 * l + ck_pad8(l);
            memset(buf + o + 32 * k + k, 0, ck_pad8(k) - k); o += 32 * k + ck_pad8(k);
        }
    }
    memcpy(buf, QS_CKPT_MAGIC, 4);
    ck_put<uint32_t>(buf, 4, QS_CKPT_VERSION); ck_put<uint32_t>(buf, 8, (uint32_t)hb); ck_put<uint32_t>(buf, 12, (uint32_t)y.n_sections);
    ck_put<uint64_t>(buf, 16, y.total);
    ck_put_config(buf, c->cfg, tracking);
    for (int k = QS_CKPT_SCALARS, i = 0; i < y.n_sections; k++, i++) {
        const size_t e = QS_CKPT_HEADER_FIXED + 24 * (size_t)i;
        ck_put<uint32_t>(buf, e, (uint32_t)k); ck_put<uint64_t>(buf, e + 8, y.off[k]); ck_put<uint64_t>(buf, e + 16, y.len[k]);
    }
    ck_put<uint32_t>(buf, 24, ck_crc32(buf + hb, body));
    return QS_OK;
}

// everything qs_restore changes, after the host-side checks: on failure the caller resets the context
static int ck_apply(qs_ctx *c, const uint8_t *buf, const CkLayout &y, bool tracking, int planes, const CkGeom &gm,
                    const std::vector<long long> &L, const std::vector<long long> &C, const std::vector<long long> &N, size_t n_blk)
{
    int rc = reset_state(c);
    if (rc != QS_OK) return rc;
    if (tracking != (c->d_dirty.p != nullptr)) {
        rc = qs_dirty_tracking(c, tracking ? 1 : 0);          // (after the reset: no unfused writes, sequence counter 0)
        if (rc != QS_OK) return rc;
    }
    const int G = c->n_graphs, nb = c->cfg.max_agent + 1;
    for (int g = 0; g < G; g++) {                            // the logs' capacities (nothing to keep: the graphs are reset)
        rc = graph_reserve(c, g, L[g], C[g], 0, 0);
        if (rc != QS_OK) return rc;
    }
    const size_t hb = y.header_bytes, body = y.total - hb;
    HIPCHK(c, c->ck_stage.reserve(body, c->stream));
    unsigned char *st = c->ck_stage.p;
    HIPCHK(c, hipMemcpyAsync(st, buf + hb, body, hipMemcpyHostToDevice, c->stream));
    auto d2d = [&](void *dst, size_t off, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, st + off - hb, bytes, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    };
    {
        size_t o = y.off[QS_CKPT_BOTS];
        HIPCHK(c, d2d(c->d_offset.p, o, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(c->d_drift.p, o, nb * 16)); o += nb * 16;
        HIPCHK(c, d2d(c->d_last_closure.p, o, nb * 8)); o += nb * 8;
        HIPCHK(c, d2d(c->d_zone.p, o, nb * 32)); o += nb * 32;
        HIPCHK(c, d2d(c->d_ekf.p, o, (size_t)nb * 44 * 8)); o += (size_t)nb * 44 * 8;
        HIPCHK(c, d2d(c->d_ekf_prev.p, o, nb * 32));
    }
    HIPCHK(c, d2d(c->d_counters.p, y.off[QS_CKPT_COUNTERS], QS_CNT_N * 8));
    const unsigned int *d_list = (const unsigned int *)(st + y.off[QS_CKPT_BLOCK_IDS] - hb);
    HIPCHK(c, qs_launch_ck_unpack(c, d_list, (unsigned int)n_blk, gm.pitch, planes, st + y.off[QS_CKPT_BLOCKS] - hb));
    if (tracking) HIPCHK(c, d2d(c->d_dirty.p, y.off[QS_CKPT_DIRTY], 4 * gm.words));
    // closure logs in place; landmark logs through the index rebuild (slam.hip), which appends them again
    std::vector<QsIndexLog> logs((size_t)G);
    {
        size_t o = y.off[QS_CKPT_GRAPHS] + (size_t)G * 24;
        for (int g = 0; g < G; g++) {
            const QsGraphBufs &q = c->graphs[g];
            const size_t l = (size_t)L[g], k = (size_t)C[g];
            const unsigned char *s = st + o - hb;
            logs[g] = QsIndexLog{(const double *)s, (const double *)(s + 8 * l), (const long long *)(s + 16 * l), s + 24 * l,
                                 L[g], N[g], C[g]};
            o += 24 * l + ck_pad8(l);
            HIPCHK(c, d2d(q.cl_lm_idx.p, o, 8 * k)); HIPCHK(c, d2d(q.cl_node_idx.p, o + 8 * k, 8 * k));
            HIPCHK(c, d2d(q.cl_dx.p, o + 16 * k, 8 * k)); HIPCHK(c, d2d(q.cl_dy.p, o + 24 * k, 8 * k));
            HIPCHK(c, d2d(q.cl_agent.p, o + 32 * k, k));
            o += 32 * k + ck_pad8(k);
        }
    }
    DevBuf<QsIndexLog> d_logs;
    HIPCHK(c, d_logs.alloc((size_t)G));
    HIPCHK(c, hipMemcpyAsync(d_logs.p, logs.data(), (size_t)G * sizeof(QsIndexLog), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, qs_launch_slam_rebuild_index(c, d_logs.p));
    HIPCHK(c, hipStreamSynchronize(c->stream));              // (d_logs and the caller's buffer go out of use)
    const uint8_t *s = buf + y.off[QS_CKPT_SCALARS];
    c->next_seq = ck_get<uint64_t>(s, 0); c->epoch_base = ck_get<uint64_t>(s, 8); c->n_rebases = ck_get<uint64_t>(s, 16);
    c->edge_rays_total = ck_get<uint64_t>(s, 24); c->edge_overflow_total = ck_get<uint64_t>(s, 32);
    c->sweep_min = ck_get<double>(s, 40); c->sweep_max = ck_get<double>(s, 48);
    c->dirty_since_fuse = ck_get<uint32_t>(s, 56) != 0;
    c->counts_view_fused = tracking && c->d_counts.p && ck_get<uint32_t>(s, 60) != 0;   // (the dense snapshot is not saved)
    // the graphs' real counts and the pile flag the rebuild left, as at any synchronisation point
    return sync_host_state(c, true);
}

extern "C" int qs_restore(qs_ctx *c, const uint8_t *buf, size_t n)
{
    ARGCHK(c, c != nullptr && buf != nullptr);
    char msg[256];
#define CK_BAD(...) do { snprintf(msg, sizeof msg, __VA_ARGS__); return qs_fail(c, QS_E_INVAL, msg); } while (0)
    if (n < QS_CKPT_HEADER_FIXED) CK_BAD("qs_restore: truncated header (%zu bytes)", n);
    if (memcmp(buf, QS_CKPT_MAGIC, 4) != 0) CK_BAD("qs_restore: bad magic (not a checkpoint)");
    const uint32_t version = ck_get<uint32_t>(buf, 4);
    if (version != QS_CKPT_VERSION) CK_BAD("qs_restore: unknown format version %u (this library reads %d)", version, QS_CKPT_VERSION);
    const uint32_t hb = ck_get<uint32_t>(buf, 8), n_sec = ck_get<uint32_t>(buf, 12);
    const uint64_t total = ck_get<uint64_t>(buf, 16);
    if ((n_sec != 6 && n_sec != 7) || hb != QS_CKPT_HEADER_FIXED + 24 * n_sec || n < hb) CK_BAD("qs_restore: bad header or section table");
    if (total != n) CK_BAD("qs_restore: length %zu does not match the header's %llu (truncated?)", n, (unsigned long long)total);
    if (ck_crc32(buf + hb, n - hb) != ck_get<uint32_t>(buf, 24)) CK_BAD("qs_restore: CRC mismatch (corrupted checkpoint)");
    // configuration: every field that changes a result
    const bool tracking = ck_get<int32_t>(buf, 72) != 0;
    uint8_t mine[QS_CKPT_HEADER_FIXED];
    memset(mine, 0, sizeof mine);
    ck_put_config(mine, c->cfg, tracking);
    for (const CkField &f : CK_FIELDS) {
        if (memcmp(buf + f.off, mine + f.off, f.is_f64 ? 8 : 4) == 0) continue;
        if (f.is_f64) CK_BAD("qs_restore: configuration field '%s' does not match (checkpoint %.17g, context %.17g)", f.name,
                             ck_get<double>(buf, f.off), ck_get<double>(mine, f.off));
        CK_BAD("qs_restore: configuration field '%s' does not match (checkpoint %d, context %d)", f.name, ck_get<int32_t>(buf, f.off),
               ck_get<int32_t>(mine, f.off));
    }
    if (c->sf_state != 0) return qs_fail(c, QS_E_STATE, "qs_restore: a sparse fuse is in flight (finish it with qs_sparse_fuse_apply)");
    // sections: the table against the layout the section contents imply
    size_t off[QS_CKPT_DIRTY + 1] = {0}, len[QS_CKPT_DIRTY + 1] = {0};
    for (uint32_t i = 0; i < n_sec; i++) {
        const size_t e = QS_CKPT_HEADER_FIXED + 24 * (size_t)i;
        const uint32_t kind = ck_get<uint32_t>(buf, e);
        const uint64_t o = ck_get<uint64_t>(buf, e + 8), l = ck_get<uint64_t>(buf, e + 16);
        if (kind < QS_CKPT_SCALARS || kind > QS_CKPT_DIRTY || off[kind] || o < hb || o % 8 || o > n || l > n - o)
            CK_BAD("qs_restore: bad section table entry %u", i);
        off[kind] = (size_t)o; len[kind] = (size_t)l;
    }
    const int G = c->n_graphs, nb = c->cfg.max_agent + 1;
    if (!off[QS_CKPT_SCALARS] || len[QS_CKPT_SCALARS] != CK_SCALARS_BYTES) CK_BAD("qs_restore: bad scalars section");
    if (ck_get<uint32_t>(buf, off[QS_CKPT_SCALARS] + 64) != (uint32_t)G || ck_get<uint32_t>(buf, off[QS_CKPT_SCALARS] + 68) != (uint32_t)nb)
        CK_BAD("qs_restore: graph / bot counts do not match");
    if (!off[QS_CKPT_GRAPHS] || len[QS_CKPT_GRAPHS] < (size_t)G * 24) CK_BAD("qs_restore: truncated graphs section");
    std::vector<long long> L(G), C(G), N(G);
    for (int g = 0; g < G; g++) {
        N[g] = ck_get<int64_t>(buf, off[QS_CKPT_GRAPHS] + 24 * g);
        L[g] = ck_get<int64_t>(buf, off[QS_CKPT_GRAPHS] + 24 * g + 8);
        C[g] = ck_get<int64_t>(buf, off[QS_CKPT_GRAPHS] + 24 * g + 16);
        if (N[g] < 0 || L[g] < 0 || C[g] < 0 || L[g] > N[g] || C[g] > N[g] || (uint64_t)L[g] > n || (uint64_t)C[g] > n)
            CK_BAD("qs_restore: bad sizes of graph %d", g);
    }
    const CkGeom gm = ck_geom(c);
    const int planes = ck_planes(c->d_counts.p != nullptr, tracking);
    const size_t n_blk = len[QS_CKPT_BLOCK_IDS] / 4;
    const CkLayout y = ck_layout(nb, G, L, C, n_blk, qs_ck_block_bytes(planes), tracking, gm.words);
    if (y.header_bytes != hb || y.total != n || y.n_sections != (int)n_sec) CK_BAD("qs_restore: section lengths do not add up");
    for (int k = QS_CKPT_SCALARS; k <= (tracking ? QS_CKPT_DIRTY : QS_CKPT_BLOCKS); k++)
        if (off[k] != y.off[k] || len[k] != y.len[k]) CK_BAD("qs_restore: section %d has the wrong offset or length", k);
    // block ids: ascending, every one a block of this grid (the unpack kernel writes where they point)
    {
        const uint8_t *ids = buf + off[QS_CKPT_BLOCK_IDS];
        long long prev = -1;
        for (size_t i = 0; i < n_blk; i++) {
            const uint32_t b = ck_get<uint32_t>(ids, 4 * i);
            const uint32_t by = b / (uint32_t)(32 * gm.pitch), bx = b % (uint32_t)(32 * gm.pitch);
            if ((long long)b <= prev || by >= (uint32_t)gm.blocks_y || bx >= (uint32_t)gm.blocks_x) CK_BAD("qs_restore: bad block id at %zu", i);
            prev = b;
        }
    }
#undef CK_BAD
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = ck_apply(c, buf, y, tracking, planes, gm, L, C, N, n_blk);
    if (rc != QS_OK) {                                       // half-restored: leave what a new context would show
        const std::string e = c->err;
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        reset_state(c);
        c->err = e;
    }
    return rc;
}
