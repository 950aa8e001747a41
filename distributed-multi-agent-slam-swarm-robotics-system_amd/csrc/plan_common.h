// plan_common.h -- what plan.hip (path planning) shares with targets_by_path.hip (§4.12) and
// territory.hip (§4.16): the tile geometry, the planner's workspace, the launchers of its kernels and the waypoint stage.
// The kernels themselves stay in plan.hip.  Below that: the host frame those two files' target calls share.
#pragma once
#include <math.h>

#include "qs_internal.h"

#define PL_T 64                       // tile edge (cells)
#define PL_H (PL_T + 2)               // tile + one-cell halo
#define PL_BLOCK 256
#define PL_INF 0xffffffffu
#define PL_MAXC QS_PLAN_MAX_CLEARANCE
#define PL_R (PL_T + 2 * PL_MAXC)     // largest dilation region edge

struct PlBox { int bx0, by0, ntx, nty, fw, fh; };    // bounding box: first tile, tiles across / down, field edge in cells

// the planner's workspace, carved from ws (nullptr: only the bytes the block needs) for n requests
struct QsPlanLayout {
    unsigned int *mask;             // [tiles down * 64][mp] traversable bits, rows padded to whole tiles
    unsigned int *tile_any;         // [tiles down][tiles across] the tile holds a traversable cell
    unsigned int *bbox;             // [4] first / last tile across and down of those (the census)
    unsigned int *cnt;              // [3] list counts of a ring of rounds
    unsigned long long *stats;      // [4] rounds, tile visits, (unused), snapped endpoints
    double2 *xy;                    // [2n] starts, then goals
    long long *cell;                // [2n] their cells (gy * size + gx), -1 = none
    int4 *out4;                     // [n] status, waypoint gx, gy, cost
    long long *plen;                // [n] path cells
    int2 *path;                     // [n][path_cap]
    unsigned int *list0, *list1, *marks;   // [item_cap] worklists of (field, tile) items and their round marks
    unsigned int *fields;           // [field_words] one group's fields
    int mp, gtx;                    // mask words per row, tiles across the grid
    size_t gmax, field_words, item_cap, bytes;
};

static inline PlBox pl_box(const unsigned int bbox[4])
{
    PlBox B;
    B.bx0 = (int)bbox[0]; B.by0 = (int)bbox[1];
    B.ntx = (int)(bbox[2] - bbox[0] + 1); B.nty = (int)(bbox[3] - bbox[1] + 1);
    B.fw = B.ntx * PL_T; B.fh = B.nty * PL_T;
    return B;
}

// ---- host side of plan.hip that targets_by_path.hip and territory.hip call -----------------------------------------------
QsPlanLayout qs_plan_layout(void *ws, int size, size_t n, size_t path_cap);
// params (NULL = the defaults) checked into out; QS_E_INVAL with a message otherwise
int plan_params(qs_ctx *c, const qs_plan_params *p, qs_plan_params &out);
// the mask and the census for n requests (layout of the planner workspace); bbox[0] > bbox[2]: no traversable cell
int plan_begin(qs_ctx *c, int clearance, size_t n, size_t path_cap, QsPlanLayout &L, unsigned int bbox[4]);
// fields of a group that fit the workspace, at most n
size_t qs_plan_group(const QsPlanLayout &L, const unsigned int bbox[4], size_t n);
// n_end endpoints xy -> cell (rule 2); *snapped counts those that moved
hipError_t qs_launch_plan_snap(qs_ctx *c, const QsPlanLayout &L, const double2 *xy, long long *cell, size_t n_end, int radius,
                               unsigned long long *snapped);
// gn fields seeded at goal[g0 .. g0 + gn) (where start and goal both have a cell), then relaxed to the fixpoint
int plan_fields(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], const long long *start, const long long *goal,
                size_t g0, size_t gn);
// the rounds of ONE field of 64-bit keys (cost << 32) | seed over the census box (territory.hip): the caller has seeded it
// and entered the seeds' tiles (item = tile index) in L.list1 / L.cnt[1] with L.marks = 1, as qs_plan_seed_kernel does
int plan_rounds_key64(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], unsigned long long *key);
// the walks of requests g0 .. g0 + gn over the group's fields: L.out4, L.plen, L.path
hipError_t qs_launch_plan_walk(qs_ctx *c, const QsPlanLayout &L, const unsigned int bbox[4], const long long *start,
                               const long long *goal, size_t g0, size_t gn, int lookahead, size_t path_cap);
// the waypoint stage of `who`: the fields and walks of the m requests start[i] -> goal[i] (cells on the device) in groups
// that fit the workspace, counted in groups; then the copy of L.out4[0 .. m) to out4 is enqueued (the caller synchronises)
int plan_waypoints(qs_ctx *c, const char *who, const QsPlanLayout &L, const unsigned int bbox[4], const long long *start,
                   const long long *goal, size_t m, int lookahead, size_t path_cap, uint64_t &groups, int4 *out4);

// ---- what the path-cost target calls share (qs_frontier_targets_by_path / _by_gain / _by_territory) ---------------------
#define TP_NOCELL 0xffffffffu         // coff of a centroid without a cell

// the part of their workspaces that both carve alike
struct QsTgtLayout {
    unsigned long long *count;            // [4] centroids with a cell, bots with a cell; territory.hip: centroids with an owner, assigned bots
    double2 *xy;                          // [n_cent + n_bots] centroids, then bots
    long long *cell;                      // [n_cent + n_bots] their cells (gy * size + gx), -1 = none
    unsigned int *coff;                   // [n_cent] offset of the centroid's cell in a field, TP_NOCELL = none
    long long *tgt_idx;                   // [n_bots] per bot: the centroid or -1
    unsigned int *tgt_cost;               // [n_bots]
    int *tgt_status;                      // [n_bots]
    long long *pair;                      // [2 n_bots] start cells of the assigned bots (in assignment order), then their goals
    int *pair_bot;                        // [n_bots] the bot of each pair
};

static inline QsTgtLayout qs_tgt_layout(Carve &k, size_t n_cent, size_t n_bots)
{
    QsTgtLayout L;
    L.count = k.take<unsigned long long>(4);
    L.xy = k.take<double2>(n_cent + n_bots);
    L.cell = k.take<long long>(n_cent + n_bots);
    L.coff = k.take<unsigned int>(n_cent);
    L.tgt_idx = k.take<long long>(n_bots);
    L.tgt_cost = k.take<unsigned int>(n_bots);
    L.tgt_status = k.take<int>(n_bots);
    L.pair = k.take<long long>(2 * n_bots);
    L.pair_bot = k.take<int>(n_bots);
    return L;
}

// the per-bot arrays such a call fills (the C ABI's); wp_cell_xy and wp_xy both or neither
struct QsTargetsOut { int64_t *target_idx; double *target_xy; uint32_t *cost; int32_t *status; int32_t *wp_cell_xy; double *wp_xy; };

// host copies of what the call's kernels left: per bot, then per assigned pair in assignment order (pair_bot, the walk's out4)
struct QsTargetsHost {
    std::vector<long long> idx; std::vector<double2> xy; std::vector<unsigned int> cost; std::vector<int> status;
    std::vector<int> pair_bot; std::vector<int4> out4;
    explicit QsTargetsHost(size_t n_bots)
        : idx(n_bots, -1), xy(n_bots, make_double2(NAN, NAN)), cost(n_bots, PL_INF), status(n_bots, QS_PLAN_NO_START),
          pair_bot(n_bots, -1), out4(n_bots, make_int4(0, -1, -1, -1)) {}
};

// targets_by_path.hip.  The arguments the three entry points share, in the order they are refused, then params into p
int tbp_check_args(qs_ctx *c, const char *who, size_t n_bots, const double *bot_xy, const QsTargetsOut &o,
                   const double *centroids_xy, size_t cap, const qs_plan_params *params, qs_plan_params &p);
// H into the caller's arrays: every bot's target, cost and status, and (o.wp_xy) the waypoints of the first m pairs, each
// walk checked against the cost `whose` ("assignment's", "partition's") kernels found for its bot
int tbp_finish(qs_ctx *c, const char *who, const char *whose, const QsTargetsHost &H, size_t m, const QsTargetsOut &o);
