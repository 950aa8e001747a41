// raycast_tiled.h -- the tile-binned raycast's shared pieces: its constants, its workspace and the host helpers that run
// passes B1 / C / D over any array of ray slots.  Pass A has two producers: qs_rays_kernel (4 rays per packet,
// raycast_tiled.hip) and qs_sweep_rays_kernel (184 ray slots per servo sweep, sweep.hip).
#pragma once
#include "raycast_common.h"

#define QT_TILE 64                       // tile edge in cells: 64 x 64 x u32 = 16 KiB of LDS
#define QT_TILE_SHIFT 6
#define QT_CELLS (QT_TILE * QT_TILE)
#define QT_CHUNK 2048                    // records per raster work item
#ifndef QT_BLOCK
#define QT_BLOCK 512                     // raster workgroup: 8 waves share one 32 KiB LDS tile (A/B: 256 -> 512 threads = -5..-18 % stage time)
#endif
#ifndef QT_BIN_BLOCK
#define QT_BIN_BLOCK 1024                // pass A / C workgroup
#endif
#ifndef QT_MAX_WG
#define QT_MAX_WG 512                    // persistent workgroups of pass A / C (2 per CU)
#endif
#define QT_MAX_TILES 16384               // LDS histogram limit: 64 KiB (8192^2 cells)
#define QT_NO_RAY (-32768)              // x0 of "no ray": grids are <= 16384 cells wide, rays < 64 cells past an edge
#ifndef QT_RASTER_WGS
#define QT_RASTER_WGS 1024               // persistent raster workgroups (4 per CU)
#endif
#ifndef QT_PITCH
#define QT_PITCH 67                      // LDS row pitch in cells: bank = (x + 3 y) mod 32, see qs_raster_kernel
#endif
#define QT_LDS_CELLS (QT_TILE * QT_PITCH)

struct QtWorkspace {
    unsigned int *table;         // [nwg][n_tiles] per-workgroup record counts -> exclusive offsets
    unsigned int *tile_count;    // [n_tiles]   records per tile
    unsigned int *tile_base;     // [n_tiles+1] exclusive scan of tile_count
    unsigned int *chunk_base;    // [n_tiles+1] exclusive scan of ceil(count / QT_CHUNK)
    uint2 *rays;                 // [n_rays]    absolute grid end points, i16 x 4: (x0 | y0 << 16, x1 | y1 << 16);
                                 //             x0 = QT_NO_RAY: none
    uint2 *recs;                 // [4 n_rays]  tile records: tile-relative end points, i8 x 4; stamp | observed-hit bit
    int tiles_x, n_tiles, nwg;
    size_t pk_per_wg;            // pass A of the 4-ray path: packets per workgroup (multiple of 64)
    size_t rays_per_wg;          // pass C: ray slots per workgroup -- workgroup w owns slots [w * rays_per_wg, (w + 1) * rays_per_wg)
    unsigned int *dirty;         // sparse fuse: bitmap of written 4 x 16-cell blocks (QsGeom::dirty), or nullptr
    int dirty_pitch;
};

__device__ inline void qt_tile_range(int x0, int y0, int x1, int y1, int size, int &tx_lo, int &tx_hi,
                                     int &ty_lo, int &ty_hi)
{
    const int xlo = max(min(x0, x1), 0), xhi = min(max(x0, x1), size - 1);
    const int ylo = max(min(y0, y1), 0), yhi = min(max(y0, y1), size - 1);
    tx_lo = xlo >> QT_TILE_SHIFT; tx_hi = xhi >> QT_TILE_SHIFT;
    ty_lo = ylo >> QT_TILE_SHIFT; ty_hi = yhi >> QT_TILE_SHIFT;
}

// The tiled sink of a projected ray (pass A; arguments as qs_ray_direct's): deferred to the host, or binned -- its cells lie in
// at most 2 x 2 tiles, each of which gets one record in pass C, counted here in the workgroup's histogram s_hist -- or, when
// it is longer than a tile (fine resolutions), cast directly, its cells added to `cells`.  Returns the ray-slot record.
template <bool COUNTS>
__device__ inline uint2 qt_ray_bin(const QsRay &ray, double rx, double ry, double yaw, float d, unsigned int key_free, int beam,
                                   const QsBatch &b, const QsGeom &geo, const QtWorkspace &ws, unsigned int *s_hist,
                                   unsigned int *__restrict__ stamps, unsigned long long *__restrict__ counts, unsigned int &cells)
{
    QsLine ln;
    if (!qs_ray_line(ray, rx, ry, yaw, d, key_free, beam, b, geo, ln)) return make_uint2((unsigned int)QT_NO_RAY & 0xffffu, 0u);
    if (ln.dx >= QT_TILE || ln.dy >= QT_TILE) {
        cells += qs_cast_line<COUNTS>(ln, ray.valid, key_free, geo, stamps, counts);
        return make_uint2((unsigned int)QT_NO_RAY & 0xffffu, 0u);
    }
    int tx_lo, tx_hi, ty_lo, ty_hi;
    qt_tile_range(ln.x0, ln.y0, ln.x1, ln.y1, geo.size, tx_lo, tx_hi, ty_lo, ty_hi);
    const int t00 = ty_lo * ws.tiles_x + tx_lo;
    const bool wx = tx_hi > tx_lo, wy = ty_hi > ty_lo;      // dx, dy < 64: at most one boundary each
    atomicAdd(&s_hist[t00], 1u);
    if (wx) atomicAdd(&s_hist[t00 + 1], 1u);
    if (wy) atomicAdd(&s_hist[t00 + ws.tiles_x], 1u);
    if (wx && wy) atomicAdd(&s_hist[t00 + ws.tiles_x + 1], 1u);
    return make_uint2(((unsigned int)ln.x0 & 0xffffu) | ((unsigned int)ln.y0 << 16),
                      ((unsigned int)ln.x1 & 0xffffu) | ((unsigned int)ln.y1 << 16));
}

// host side (raycast_tiled.hip).  qt_workspace: grows the context's workspace for up to cap_rays ray slots and carves it;
// the caller fills nwg, pk_per_wg / rays_per_wg.  qt_dyn_lds: bytes of pass A / C's LDS histogram (large grids raise the
// kernels' limit: on / off are the two instantiations of the pass-A kernel beside qs_scatter_kernel).  qt_launch_sort_raster:
// passes B1, C, D over ray slots [0, n_rays) whose hit flags are hit_valid[r] and whose stamps are
// qs_stamp_key(ord_base + ord_stride * (r >> 2) + (r & 3)).
hipError_t qt_workspace(qs_ctx *c, size_t cap_rays, QtWorkspace &ws);
hipError_t qt_dyn_lds(const QtWorkspace &ws, const void *on, const void *off, size_t &lds);
hipError_t qt_launch_sort_raster(qs_ctx *c, const QtWorkspace &ws, size_t n_rays, const unsigned char *hit_valid,
                                 unsigned long long ord_base, unsigned long long ord_stride, size_t lds);
