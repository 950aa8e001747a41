// territory_layout.h -- the workspace of one territory call (territory.hip), apart from the kernels so that
// a host-only program can carve it over plain memory (tools/territory_layout_check.hip).
#pragma once
#include "plan_common.h"

// carved from ws (nullptr: only the bytes the block needs) for a grid of `size` cells a side
struct QsTerrLayout {
    unsigned long long *key;              // [field_cells] the one field: (cost << 32) | bot, all ones = unreached
    unsigned long long *slot;             // [n_bots] per bot: the smallest (cost << 32) | centroid it owns
    unsigned long long *area;             // [n_bots] cells owned
    int *box;                             // [n_bots][4] min gx, min gy, max gx, max gy of them
    QsTgtLayout tg;                       // what targets_by_path.hip's workspace holds too; the pairs are in bot order
    int *cent_owner;                      // [n_cent]
    unsigned int *cent_cost;              // [n_cent]
    double2 *tgt_xy;                      // [n_bots] per bot: its target's position
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
    L.tg = qs_tgt_layout(k, n_cent, n_bots);
    L.cent_owner = k.take<int>(n_cent);
    L.cent_cost = k.take<unsigned int>(n_cent);
    L.tgt_xy = k.take<double2>(n_bots);
    L.owner = want_owner ? k.take<short>(cells) : nullptr;
    L.cost = want_cost ? k.take<unsigned int>(cells) : nullptr;
    L.bytes = k.bytes;
    return L;
}
