// territory_layout.h -- the workspace of one territory call (territory.hip), apart from the kernels so that
// a host-only program can carve it over plain memory (tools/territory_layout_check.cpp).
#pragma once
#include "plan_common.h"

// carved from ws (nullptr: only the bytes the block needs) for a grid of `size` cells a side
struct QsTerrLayout {
    unsigned long long *key;              // [field_cells] the one field: (cost << 32) | bot, all ones = unreached
    unsigned long long *slot;             // [n_bots] per bot: the smallest (cost << 32) | centroid it owns
    unsigned long long *area;             // [n_bots] cells owned
    int *box;                             // [n_bots][4] min gx, min gy, max gx, max gy of them
    unsigned long long *count;            // [4] centroids with a cell, bots with a cell, centroids with an owner, assigned bots
    double2 *xy;                          // [n_cent + n_bots] centroids, then bots
    long long *cell;                      // [n_cent + n_bots] their cells (gy * size + gx), -1 = none
    unsigned int *coff;                   // [n_cent] offset of the centroid's cell in the field
    int *cent_owner;                      // [n_cent]
    unsigned int *cent_cost;              // [n_cent]
    long long *tgt_idx;                   // [n_bots] per bot: the centroid or -1
    double2 *tgt_xy;                      // [n_bots]
    unsigned int *tgt_cost;               // [n_bots]
    int *tgt_status;                      // [n_bots]
    long long *pair;                      // [2 n_bots] start cells of the assigned bots (in bot order), then their goals
    int *pair_bot;                        // [n_bots] the bot of each pair
    short *owner;                         // [size][size] when asked for, else nullptr and no bytes
    unsigned int *cost;                   // [size][size] likewise
    size_t field_cells, bytes;
};

static inline QsTerrLayout qs_terr_layout(void *ws, int size, size_t n_cent, size_t n_bots, bool want_owner, bool want_cost)
{
    QsTerrLayout L;
    Carve k(ws);
    const size_t edge = (size_t)((size + PL_T - 1) / PL_T) * PL_T, cells = (size_t)size * size;
    L.field_cells = edge * edge;          // a field over the whole grid: the census box is never larger
    L.key = k.take<unsigned long long>(L.field_cells);
    L.slot = k.take<unsigned long long>(n_bots);
    L.area = k.take<unsigned long long>(n_bots);
    L.box = k.take<int>(4 * n_bots);
    L.count = k.take<unsigned long long>(4);
    L.xy = k.take<double2>(n_cent + n_bots);
    L.cell = k.take<long long>(n_cent + n_bots);
    L.coff = k.take<unsigned int>(n_cent);
    L.cent_owner = k.take<int>(n_cent);
    L.cent_cost = k.take<unsigned int>(n_cent);
    L.tgt_idx = k.take<long long>(n_bots);
    L.tgt_xy = k.take<double2>(n_bots);
    L.tgt_cost = k.take<unsigned int>(n_bots);
    L.tgt_status = k.take<int>(n_bots);
    L.pair = k.take<long long>(2 * n_bots);
    L.pair_bot = k.take<int>(n_bots);
    L.owner = want_owner ? k.take<short>(cells) : nullptr;
    L.cost = want_cost ? k.take<unsigned int>(cells) : nullptr;
    L.bytes = k.bytes;
    return L;
}
