// qs_internal.h -- shared declarations of the HIP implementation behind include/quasar_slam.h
// gfx950 only.  All device arithmetic that decides a cell index or a loop closure is fp64
// with -ffp-contract=off (the reference is CPython double arithmetic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/quasar_slam.h"

#define QS_WAVE 64
#define QS_MAX_AGENT 255          // agent_id is one byte on the wire (dual_bot_mapper.py:41)
#define QS_WIN_MAX 32             // SLAM window: min(min_poses_between, 32) consecutive nodes

// ---- monotone double <-> uint64 map for atomic min/max of zone boxes --------------------
__host__ __device__ inline unsigned long long qs_ord_from_double(double d)
{
    unsigned long long b;
    __builtin_memcpy(&b, &d, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double qs_double_from_ord(unsigned long long k)
{
    unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
#define QS_ORD_MIN_IDENT 0xffffffffffffffffull   // identity for atomicMin
#define QS_ORD_MAX_IDENT 0ull                    // identity for atomicMax

struct QsNcclId { char internal[QS_RCCL_ID_BYTES]; };     // ncclUniqueId (rccl.h), passed by value to ncclCommInitRank

// ---- per pose-graph device state (PoseGraphSLAM, dual_bot_mapper.py:261-271) -------------
// The landmark list is kept twice: as the reference's insertion-ordered log (read-back, and
// the fallback scan), and as a spatial index: a directory (hash table over the bucket cells) of buckets
// of edge >= CLOSURE_RADIUS per landmark type, each bucket a chain of 7-entry nodes in insertion order.  A query looks at
// the 3x3 buckets around it; the first match in list order is the lowest node index among them.
#define QS_NTYPES 5               // landmark types 1..5 are indexed (LM_CORNER_L..LM_OPEN, :68-74)
#define QS_NODE_CAP 7
// The eighth index slot is the node's look-ahead word: idx[QS_NODE_LOOKAHEAD] of node n holds the index of entry 0 of n's successor
// node once that entry exists, the empty marker until then.  chain_insert_lanes (slam.hip) writes it with that entry, in the
// same batch; entries are in insertion order, so nothing in the successor chain lies below it.  x[7] and y[7] stay unused.
#define QS_NODE_LOOKAHEAD QS_NODE_CAP
struct alignas(64) QsLmNode { long long idx[8]; double x[8]; double y[8]; };   // idx 0x7f7f.. = empty slot
struct QsDirEntry { unsigned int head, tail, tail_cnt, pad; };                  // head 0 = empty bucket (insert-side bookkeeping)
struct QsBucketGeom { double bx0, by0, cell, inv_cell; unsigned int hmask, pad; };   // hmask + 1 = table entries per type

struct QsGraphDev {
    long long n_nodes;     // len(self.nodes)
    long long n_lms;       // len(self.landmarks)
    long long n_cls;       // len(self.closures)
    long long cap_lms, cap_cls;
    double *lm_x, *lm_y;   // landmark position (pose of the storing packet, pre-closure)
    long long *lm_idx;     // node index of the storing packet (ascending)
    unsigned char *lm_type;
    long long *cl_lm_idx, *cl_node_idx;
    double *cl_dx, *cl_dy;
    unsigned char *cl_agent;   // agent_id of the closing node (nodes[node_idx].agent_id, :335)
    QsDirEntry *dir;       // [QS_NTYPES][hmask + 1]
    QsLmNode *nodes;       // [node_cap]: node 0 is the null node, node 1 + t the FIRST node of directory entry t (a query
                           // goes straight to it: no directory round trip), the pool of overflow nodes after those
    unsigned int *nd_next; // [node_cap]
    unsigned int *misc;    // [cap_lms] log slots of landmarks the directory does not cover
    long long n_misc;
    unsigned int nodes_used, pad0;   // next free pool node
    long long node_cap;    // 1 + directory entries + cap_lms
};

// ---- per-batch scratch of the SLAM stage ---------------------------------------------------
// one event of an agent's plan: what the lean owner needs to start a decision on it, and where it goes on after a closure there
struct alignas(32) QsPlanRec {
    int node;              // node index (low word: the lean owner's graphs stay below 0x7f7f7f7f)
    unsigned int r;        // position in the graph's event list, from ev_base[g]
    int type;              // landmark type
    unsigned int skip;     // own index of the agent's first later event with node - this node >= MIN_POSES_BETWEEN (none: the count)
    double px, py;         // pose before drift
};
struct QsSlamBatch {
    long long *node;                       // [n] node index of each record (-1: rejected)
    long long *ev_node;                    // [n] landmark events, grouped by graph, in node order
    unsigned char *ev_agent, *ev_type;     //     agent index local to the graph, landmark type
    double *ev_px, *ev_py;                 //     pose before drift
    unsigned int *ev_base;                 // [n_graphs + 1] event range of each graph
    unsigned int *acc_total;               // [n_graphs] accepted records of each graph
    unsigned int *blk_acc, *blk_ev;        // [n_graphs][n_blocks] per-block counts -> exclusive offsets
    unsigned int *agent_ev;                // [max_agent + 2] events per bot -> exclusive prefix
    long long *acl_node;                   // [n] per-bot closure regions: node index of the closure,
    double *acl_dx, *acl_dy;               //     drift of the bot AFTER it
    unsigned int *acl_cnt;                 // [max_agent + 1] closures per bot in this batch
    double *drift_start;                   // [(max_agent + 1) * 2] drift at batch start
    int n_blocks;
    // the plan (slam.hip, plan kernels): every bot's own events in list order, bot b's at pl_rec[agent_ev[b] ..
    // agent_ev[b + 1]) -- the regions its closures have in acl_*.  pl_rec == nullptr: this launch has no plan.
    QsPlanRec *pl_rec;                     // [n]
    unsigned int *pl_blk;                  // [max_agent + 1][pl_blocks] events of the bot per block of QS_SLAM_PLAN_BLOCK events -> offsets
    unsigned int *pl_first;                // [max_agent + 1] own index of the bot's first event past its cool-down (none: its count)
    int pl_blocks;
};

// ---- geometry / constants passed by value to kernels ------------------------------------
struct QsGeom {
    int size;
    double res, ox, oy;
    double min_dist, max_dist;
    double inv_res;          // 1.0 / res: screens world_to_grid quotients, never decides one (raycast_common.h)
    unsigned int *dirty;     // sparse fuse (sparse_fuse.hip): one bit per QS_DIRTY_BLOCK_H x QS_DIRTY_BLOCK_W block of cells written
    int dirty_pitch;         //   since the last fuse, rows of dirty_pitch 32-bit words; nullptr = no tracking
};

// bit of the block that holds cell (x, y): word index and mask
__host__ __device__ inline size_t qs_dirty_word(int x, int y, int pitch) { return (size_t)(y / QS_DIRTY_BLOCK_H) * pitch + (x / QS_DIRTY_BLOCK_W) / 32; }
__host__ __device__ inline unsigned int qs_dirty_mask(int x) { return 1u << ((x / QS_DIRTY_BLOCK_W) & 31); }
// cell of lane `lane` (one lane per cell) of block `bid` = bit index in the bitmap (row by, column bx): false beyond the
// grid's right edge
__device__ inline bool qs_block_cell(unsigned int bid, int lane, int pitch, int size, size_t &cell)
{
    const int by = (int)(bid / (unsigned int)(pitch * 32)), bx = (int)(bid % (unsigned int)(pitch * 32));
    const int x = bx * QS_DIRTY_BLOCK_W + (lane & (QS_DIRTY_BLOCK_W - 1)), y = by * QS_DIRTY_BLOCK_H + (lane >> 4);
    cell = (size_t)y * size + x;
    return x < size && y < size;
}

// a ray left to the host (exact-trig mode): everything needed to cast it later, whatever has happened to its batch since
// device words read by the host at synchronisation points (qs_ctx::d_flags; qs_reset clears the first four)
enum { QS_FLAG_EDGE_N = 0,        // exact-trig mode: edge rays waiting for the host
       QS_FLAG_PILE = 1,          // a landmark pile has formed (slam.hip, DENSE)
       QS_FLAG_EDGE_OVF = 2,      // edge rays that found the waiting list full
       QS_FLAG_CHAIN_FULL = 3,    // free-running chain: the number of the last launch in which a graph was refused the lean owner
       // loop-closure chain, running totals (never cleared; the host looks at differences -- qs_api.hip, chain_stats_poll):
       QS_FLAG_CHAIN_MISS = 4,    // free-running form: decisions that waited for the frontier ...
       QS_FLAG_CHAIN_HIT = 5,     // ... and its closures
       QS_FLAG_CHAINW_MISS = 6,   // per-window form: eligible queries that found nothing ...
       QS_FLAG_CHAINW_HIT = 7,    // ... and its closures
       QS_N_FLAGS = 8 };
// key_free: stamp of its free cells ((ordinal << 1) | 0); beam: -1 = one of a QuasarPacket's four rays (sensor = ordinal & 3),
// 0..180 = beam of a servo sweep (angle yaw + (beam - 90) * pi / 180, trust filter qs_set_sweep_filter's)
struct QsEdgeRec { double rx, ry, yaw; float d; unsigned int key_free; int beam, pad; };
#define QS_EDGE_CAP (1u << 18)

// ---- decoded batch (SoA, one slot per datagram of the batch) -----------------------------
struct QsBatch {
    size_t n;
    unsigned char *accept;   // 1 = passes dual_bot_mapper.py:826-843
    unsigned char *map_ok;   // 1 = accepted AND this context casts its rays / runs its filter: the same array as accept
                             // unless the context is one shard of a replicated-pose-graph deployment (qs_config.shard_bots)
    int own_lo, own_hi;      // agents whose rays this context casts (1..max_agent when not sharded)
    QsEdgeRec *edge;         // exact-trig mode: rays whose end point lies within 1e-9 cells of a cell boundary are not cast by the
    unsigned int *edge_n;    //   device but appended here, self-contained (pose, distance, stamp): the host resolves them at the next
    unsigned int edge_cap;   //   point the map is observed (qs_api.hip: sync_host_state); edge_n[0] = records so far, [2] = rays that
                             //   found the list full and were cast with the device's trig after all
    unsigned char *agent;    // agent_id
    unsigned char *lm;       // landmark_type (0 for v1 packets)
    double *px, *py, *yaw;   // f32 fields widened; px already has the bot offset (:851-852)
    float4 *dist;            // front, left, back, right (metres)
    int *enc;                // encoder ticks
    double *rx, *ry;         // pose after drift correction (:855-857), written by the SLAM stage
    double2 *hit;            // 4 per datagram: ray end points, filled on request (qs_launch_hits)
    unsigned char *hit_valid; // MIN < d <= MAX per ray (:888); the tiled raycast writes it on the ingest path
};

// ---- owning device buffer of host code: freed when it goes out of scope or is assigned over ---------------------------
// alloc: into an empty buffer.  reserve: the one way a grown workspace changes size -- exactly `need` elements, or
// (floor > 0) floor doubled until it holds them.  The capacity is 0 from before the old block is freed until the new one
// exists, so a failed growth leaves an empty buffer, never a capacity over a null pointer.  Arrays whose contents must
// survive a growth (or whose views must stay valid if it fails) are grown by allocating a new buffer and moving it in.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;      // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { hipFree(p); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { hipFree(p); }
    hipError_t alloc(size_t n)
    {
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        return hipSuccess;
    }
    hipError_t reserve(size_t need, hipStream_t st, size_t floor = 0)
    {
        if (need <= cap) return hipSuccess;
        size_t n = floor ? floor : need;
        while (n < need) n *= 2;
        hipError_t e = hipStreamSynchronize(st);          // (the old block may still be in use)
        if (e != hipSuccess) return e;
        cap = 0;
        e = hipFree(p);
        p = nullptr;
        return e != hipSuccess ? e : alloc(n);
    }
};

// ---- workspace layout: a bump allocator over one block, every piece on a 256-byte boundary ----------------------------
// Each workspace has one layout function that carves it: run over the block it hands out the pieces, run over nullptr it
// hands out nullptrs and only adds up the bytes the block needs (hipMalloc's blocks are at least 256-byte aligned).
struct Carve {
    char *base;
    size_t bytes = 0;
    explicit Carve(void *b) : base((char *)b) {}
    template <typename T> T *take(size_t n)
    {
        T *q = base ? (T *)(base + bytes) : nullptr;
        bytes += (n * sizeof(T) + 255) & ~(size_t)255;
        return q;
    }
};

// ---- the device arrays of one pose graph; QsGraphDev, the view the kernels read, is filled from them ------------------
struct QsGraphBufs {
    DevBuf<double> lm_x, lm_y; DevBuf<long long> lm_idx; DevBuf<unsigned char> lm_type;
    DevBuf<long long> cl_lm_idx, cl_node_idx; DevBuf<double> cl_dx, cl_dy; DevBuf<unsigned char> cl_agent;
    DevBuf<QsDirEntry> dir; DevBuf<QsLmNode> nodes; DevBuf<unsigned int> nd_next, misc;
    long long cap_lms = 0, cap_cls = 0;      // entries of the landmark / closure logs (set once every array of a log has grown)
};

struct qs_ctx {
    qs_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool ekf_stream_shared = false;              // the device's one CU-masked stream (qs_api.hip): not this context's to destroy
    hipStream_t ekf_stream = nullptr;            // the EKF is independent of the map: own stream,
    hipEvent_t ev_decoded = nullptr, ev_ekf_done = nullptr;   // forked after decode, joined at the end
    std::string err;
    size_t cells = 0;
    int n_graphs = 0, bots_per_graph = 0, win = 30;
    double r2_threshold = 0.0;   // s < r2_threshold  <=>  sqrt(s) < closure_radius
    QsGeom geom;

    // Every device block the context holds is a DevBuf (freed by `delete`); the raw pointers below are views into them.
    DevBuf<unsigned int> d_stamps;               // [size][size]; 0 = UNKNOWN, else (ordinal<<1)|occ
    DevBuf<unsigned long long> d_counts;         // [size][size]; hi32 = hits, lo32 = misses (this context's own writes)
    DevBuf<unsigned long long> d_counts_fused;   // [size][size]; snapshot of d_counts that a collective sums over the ranks
    bool counts_view_fused = false;              // qs_grid_counts / qs_grid_logodds read the fused snapshot
    bool dirty_since_fuse = false;               // cells written since the last qs_mark_fused (sharded streams: rebase guard)
    // sparse fuse (sparse_fuse.hip)
    DevBuf<unsigned int> d_dirty;                // live bitmap [blocks_y][dirty_pitch]
    size_t dirty_words = 0;
    int blocks_x = 0, blocks_y = 0;
    DevBuf<unsigned long long> d_counts_sent;    // [size][size]: this context's counters as of its last sparse fuse (deltas travel)
    int sf_world = 0, sf_rank = 0;
    DevBuf<char> sf_meta;                        // the three arrays below, carved for sf_world ranks (sparse_fuse.hip: sf_layout)
    unsigned int *d_sf_bitmaps = nullptr;        // [sf_world][dirty_words]: every rank's bitmap of the fuse in flight
    unsigned int *d_sf_lists = nullptr;          // [sf_world][dirty_words * 32] block ids, ascending
    unsigned int *d_sf_counts = nullptr;         // [sf_world] blocks per rank
    DevBuf<unsigned char> sf_payload;            // every rank's segment of the fuse in flight, grown on demand
    std::vector<unsigned int> sf_n;              // host copy of d_sf_counts
    std::vector<size_t> sf_off;                  // [sf_world + 1] byte offsets of the ranks' segments in the payload
    int sf_state = 0;                            // 0 idle, 1 begun, 2 planned
    DevBuf<double> d_offset;                     // [max_agent+1]
    DevBuf<double> d_drift;                      // [max_agent+1][2]
    DevBuf<long long> d_last_closure;            // [max_agent+1]
    DevBuf<unsigned long long> d_zone;           // [max_agent+1][4] ordered-u64 minx,miny,maxx,maxy
    DevBuf<unsigned long long> d_counters;       // [QS_CNT_N]
    DevBuf<unsigned long long> d_graph_batch;    // [n_graphs][2]: accepted, landmark events of the batch
    DevBuf<double> d_ekf;                        // [max_agent+1][44]
    DevBuf<double> d_ekf_prev;                   // [max_agent+1][4]

    DevBuf<QsGraphDev> d_graphs;                 // [n_graphs] the views the kernels read (and the counters only they write)
    std::vector<QsGraphBufs> graphs;             // [n_graphs] their arrays
    std::vector<long long> lms_upper, cls_upper; // host upper bounds on n_lms / n_cls

    // batch arrays: b and sb are carved from batch_ws for cap_batch records (qs_api.hip: batch_layout)
    size_t cap_batch = 0;
    DevBuf<char> batch_ws;
    DevBuf<char> stage_ws;                       // host records staged on the device (qs_api.hip: staging_layout)
    QsBatch b{};
    QsSlamBatch sb{};
    QsBucketGeom bg{};
    size_t dir_entries = 0;      // QS_NTYPES * (hmask + 1)
    size_t last_n = 0;
    bool last_has_poses = false;

    // workspaces, grown on demand (DevBuf::reserve)
    DevBuf<char> bin_ws;                         // tile-binned raycast (raycast_tiled.hip)
    DevBuf<char> frontier_ws;                    // frontier labelling (allocated on first use)
    DevBuf<char> ft_ws;                          // frontier target assignment (frontier_targets.hip)
    DevBuf<char> plan_ws;                        // path planning (plan.hip: qs_plan_layout)
    DevBuf<char> tbp_ws;                         // targets by path cost (targets_by_path.hip: qs_tbp_layout)
    DevBuf<char> gain_ws;                        // frontier gain (gain.hip: qs_gain_layout)
    DevBuf<char> terr_ws;                        // territories (territory.hip: qs_terr_layout)
    DevBuf<char> io_ws;                          // staging of the object-API calls (qs_update_rays, views)
    DevBuf<char> view_ws;                        // map view (view.hip: qs_view_layout): state / owner frames, index tables, uploaded lists
    DevBuf<char> ekf_ws;                         // parallel-in-time EKF (ekf_scan.hip)
    DevBuf<unsigned int> ck_census;              // checkpoint (checkpoint.hip): block bitmap, block list, count
    DevBuf<unsigned char> ck_stage;              //   ... and the body of the file as it travels (both ways)
    DevBuf<unsigned char> sweep_hv;              // servo sweeps (sweep.hip): hit flags of one chunk's ray slots
    DevBuf<unsigned char> sweep_acc;             //   ... accepted flag and pose of every record of the last call
    DevBuf<double> sweep_pose;
    double sweep_min = 0.1, sweep_max = 1.2;     //   trust filter smin < d <= smax (qs_set_sweep_filter)
    size_t last_sweeps_n = 0;
    bool last_sweeps = false;                    //   the last ingest was qs_ingest_sweeps*: qs_last_sweeps may read it
    bool sweep_graph = false;                    // graph mode (qs_set_sweep_graph, sweep_graph.hip): a sweep is a pose-graph node
    qs_sweep_graph_params sg_params{5, 0, 0.40, 0.80};
    bool last_sweep_graph = false;               //   the last sweep ingest ran in graph mode: qs_last_sweep_nodes may read the batch
    DevBuf<double> match_tab;                    // sweep matching (match.hip): cos, sin of the 181 beam angles, from the host's libm
    DevBuf<qs_sweep_match> match_out;            //   ... the matches of the last matched ingest (qs_last_sweep_matches)
    size_t last_matches_n = 0;
    bool last_matches = false;
    DevBuf<qs_sweep_check> check_out;            // sweep check (check.hip): the checks of the last guarded ingest (qs_last_sweep_checks)
    size_t last_checks_n = 0;
    bool last_checks = false;
    DevBuf<double> reloc_rot;                   // relocalisation (reloc.hip): sin, cos, yaw of the reloc_nrot rotation steps, host's libm
    int reloc_nrot = 0;
    DevBuf<char> reloc_ws;                       //   ... census, score tables and picks of one chunk of sweeps (qs_reloc_layout)
    // bot veil (veil.hip): off unless qs_set_bot_veil turned it on; table and word exist from the first call that needs them
    int veil_radius = 0;                         // cells; 0 = off
    DevBuf<int4> veil_tab;                       // [256] cell[bot]: x, y, known (V2)
    DevBuf<unsigned long long> veil_total;       // [1] rays veiled since the last reset
    DevBuf<char> veil_ws;                        // cells, block rows and flags of one ingest (veil.hip: qs_veil_layout)
    unsigned char *veil_flags = nullptr;         //   ... the flags of the last veiled ingest (qs_last_veiled)
    bool last_veil = false;                      // the last packet ingest ran the veil stage
    bool veil_sweeps = false;                    // sweeps too (qs_set_bot_veil_sweeps, rules S0-S8); acts only while veil_radius > 0
    DevBuf<char> sveil_ws;                       //   ... the sweep stage's workspace (veil.hip: qs_sveil_layout), laid out for
    size_t sveil_cap = 0, sveil_n = 0;           //   sveil_cap sweeps a chunk and the sveil_n sweeps of the call whose flags it holds
    bool last_sveil = false;                     //   the last sweep ingest ran the stage (qs_last_sweeps_veiled)

    // map merge session (merge.hip): the merger node's state.  qs_reset and checkpoints leave it alone
    DevBuf<double2> mg_cloud;                    // the global cloud; grown by allocate-new-and-move (a failed growth keeps it)
    size_t mg_n = 0;                             //   ... its points
    double mg_res = 0.05, mg_ox = 0.0, mg_oy = 0.0;       // map_resolution, map_origin (map_merger.py:31-33)
    double mg_icp_threshold = 1.0, mg_min_fitness = 0.6;  // qs_merge_params (map_merger.py:46-54)
    int mg_icp_iterations = 30;
    DevBuf<char> mg_grid_ws;                     // a map message on its way to a cloud (merge.hip: qs_merge_grid_layout)
    DevBuf<char> mg_pts_ws;                      // clouds, sort and run arrays of one callback (merge.hip: qs_merge_pts_layout)

    uint64_t next_seq = 0, epoch_base = 0, n_rebases = 0;
    DevBuf<unsigned int> d_flags;                // [QS_N_FLAGS] device words the host reads at synchronisation points (QS_FLAG_*)
    DevBuf<QsEdgeRec> d_edge;                    // [QS_EDGE_CAP] the waiting rays
    bool edge_maybe = false;                     // an exact-trig ingest has run since the last flush: the list may hold rays
    bool pile_mode = false;                      // launch the chain kernel's DENSE variant
    bool flags_maybe = false;                    // a loop-closure chain has run since the flags were read last
    int chain_form = 0;                          // QS_CHAIN_AUTO / _FREE / _WINDOW (qs_set_chain_form)
    bool chain_posting = false;                  // QS_CHAIN_AUTO's present choice for graphs of few agents: the free-running kernel WITH the
                                                 // owners posting their landmarks' poses (slam.hip, qs_launch_slam)
    bool chain_windowed = false;                 // ... and beyond that: the per-window kernel (even with posted poses most queries find nothing)
    bool chain_last_free = true, chain_last_posting = false;   // the form the last launch used
    int chain_lean_mode = 0;                     // QS_CHAIN_LEAN_AUTO / _OFF (qs_set_chain_lean) ...
    long long chain_lean_limit = 0x7f7f7f7fll;   // ... and the node count below which the kernel allows it (the empty marker's low word, or less)
    unsigned int chain_lean_seq = 0;             // launches of the free-running kernel so far (what a refused graph leaves in QS_FLAG_CHAIN_FULL)
    bool chain_last_lean_asked = false;          // the last launch was that kernel with the lean owner on offer
    bool chain_plan = true;                      // the lean owner walks a per-agent plan of its events (qs_set_chain_plan) ...
    bool chain_last_plan = false;                // ... and the last launch had one built for it
    bool chain_lookahead = true;                 // the lean owner tests a node's look-ahead word before it walks on (qs_set_chain_lookahead)
    bool chain_scout = false;                    // scout waves stage the plan owner's rows in LDS (qs_set_chain_scout; graphs of <= 2 agents) ...
    bool chain_last_scout = false;               // ... and the last launch ran the kernel that has them, with a plan
    DevBuf<unsigned int> d_scout;                // [2] the last launch's decisions settled from a stage / by the owner's own loads
    unsigned int *h_chain_stat = nullptr;        // pinned: [0..3] the four running totals as copied last, [4..7] as consumed last
    hipEvent_t ev_chain_stat = nullptr;          // ... complete when the copy has landed
    bool chain_stat_pending = false;
    unsigned int chain_stat_tick = 0;            // ingests since qs_create (the copy is asked for by one in four)
    uint64_t edge_rays_total = 0;                // exact-trig mode: rays resolved on the host since the last reset
    uint64_t edge_overflow_total = 0;            //   ... and rays that found the list full (cast with the device's trig)

    // timing
    bool timing = false;
    struct Pending { int stage; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
    double stage_ms[QS_STAGE_N + 1]{};           // (+ 1: the veil stage's own pair of events, which is no QS_STAGE_* of the ABI)
    uint64_t stage_launches[QS_STAGE_N + 1]{};
};

// ---- HIP-event timing of stages and of single kernels, on the stream they are launched on -------
static inline hipEvent_t qs_ev_get(qs_ctx *c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}
#define QS_STAGE_VEIL_INTERNAL QS_STAGE_N        // qs_bot_veil_time reads it; qs_stage_times never reports it
struct StageTimer {
    qs_ctx *c; int stage; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    StageTimer(qs_ctx *c_, int s, hipStream_t st_ = nullptr) : c(c_), stage(s), st(st_ ? st_ : c_->stream)
    { if (c->timing) { a = qs_ev_get(c); b = qs_ev_get(c); hipEventRecord(a, st); } }
    void stop() { if (c->timing && a) { hipEventRecord(b, st); c->pending.push_back({stage, a, b}); a = nullptr; } }
};

// ---- host side of the C ABI: what the files that define extern "C" entry points share ----------------------------------
// qs_fail records the message (per context, or per thread before one exists) and returns the code; the macros return from
// the calling entry point (HIPRET from a helper that returns hipError_t).
int qs_fail(qs_ctx *c, int code, const char *what, hipError_t e = hipSuccess);
#define HIPCHK(c, x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return qs_fail((c), QS_E_HIP, #x, e__); } while (0)
#define ARGCHK(c, cond) do { if (!(cond)) return qs_fail((c), QS_E_INVAL, "invalid argument: " #cond); } while (0)
#define HIPRET(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return e__; } while (0)

struct ScopedEvent {                        // an event of one call, destroyed with its scope (as DevBuf frees a buffer)
    hipEvent_t e = nullptr;
    ScopedEvent() = default;
    ScopedEvent(const ScopedEvent &) = delete;
    ScopedEvent &operator=(const ScopedEvent &) = delete;
    ~ScopedEvent() { if (e) hipEventDestroy(e); }
};
static const size_t QS_IO_WS_FLOOR = (size_t)1 << 16;      // qs_ctx::io_ws doubles from 64 KiB

// smallest double T with sqrt(T) >= radius: (s < T) <=> (sqrt(s) < radius) for correctly rounded sqrt
double r2_threshold_for(double radius);
// capacity of graph g's logs for need_* entries, the first have_* kept
int graph_reserve(qs_ctx *c, int g, long long need_lms, long long need_cls, long long have_lms, long long have_cls);
int reset_state(qs_ctx *c);                              // qs_reset: an empty map, enqueued (no wait for the GPU)
int ensure_batch(qs_ctx *c, size_t n);                   // room for n records; a growth that fails leaves the old arrays
// What every ingest that feeds the pose graphs does round its own decoder, before its rays are cast.  qs_batch_prepare: room for
// n records, the batch's per-graph and per-bot counts cleared.  Then the caller's decoder fills QsBatch, graph_batch and agent_ev
// for the n records (under QS_STAGE_DECODE).  qs_batch_slam: the graphs' capacity for the batch, then the SLAM stage under
// QS_STAGE_SLAM with the chain statistics polled before it and asked for behind it.
int qs_batch_prepare(qs_ctx *c, size_t n);
int qs_batch_slam(qs_ctx *c, size_t n);
// n_seq sequence numbers from seq0 fit the stamp epoch (a rebase first if they do not)
int ensure_epoch(qs_ctx *c, uint64_t seq0, size_t n_seq);
// device staging of host-side records: bytes of records, one length and one receive time per (shortest) record, laid out for
// the smallest power-of-two multiple of 64 KiB that holds `bytes` (the block only grows)
struct Staging { unsigned char *pkts; unsigned short *lens; double *time; };
int reserve_staging(qs_ctx *c, size_t bytes, Staging &s);

// The sync point: every call that observes the map, the counters or the pose graphs goes through it first.  It resolves
// the exact-trig edge rays waiting on the device, reads the pile flag and the loop-closure chain's statistics, and sets
// the host's landmark / closure bounds to the graphs' exact counts.  Without host_waits it does nothing when no ingest or
// chain has run since the last time; host_waits: the caller waits for the stream anyway, so the flags are read regardless.
int sync_host_state(qs_ctx *c, bool host_waits);
#define SYNCCHK(c) do { int rcs__ = sync_host_state((c), false); if (rcs__ != QS_OK) return rcs__; } while (0)

// ---- kernel launchers (each defined next to its kernel) that another file calls ----------------
// decode.hip
hipError_t qs_launch_decode(qs_ctx *c, const unsigned char *d_pkts, size_t n, size_t stride,
                            const unsigned short *d_lens);
#define QS_SLAM_IDX_BLOCK 1024   // records per block of the SLAM index tables
// slam.hip
hipError_t qs_launch_slam(qs_ctx *c, size_t n, bool raw_pose = false);
hipError_t qs_launch_slam_reset_index(qs_ctx *c);              // empties the bucket index of every graph (what was used of it)
// a graph's uploaded landmark log (qs_restore) and the counters that go with it
struct QsIndexLog { const double *x, *y; const long long *idx; const unsigned char *type; long long n, n_nodes, n_cls; };
hipError_t qs_launch_slam_rebuild_index(qs_ctx *c, const QsIndexLog *d_logs);   // [n_graphs], into graphs just reset
int qs_slam_blocks(size_t n);
#define QS_SLAM_PLAN_BLOCK 256   // events per block of the plan kernels
int qs_slam_plan_blocks(size_t n);
// raycast.hip
#define QS_DIRECT_MAX_BATCH 256   // raycast_mode auto: batches up to this size take the direct kernel
hipError_t qs_launch_raycast_direct(qs_ctx *c, size_t n, uint64_t seq0);
hipError_t qs_launch_edge_cast(qs_ctx *c, unsigned int n_edge, const double *d_in);
hipError_t qs_launch_hits(qs_ctx *c, size_t n);                 // ray end points of the resident batch (qs_last_hits)
hipError_t qs_launch_update_rays(qs_ctx *c, const double *rx, const double *ry, const double *hx,
                                 const double *hy, const unsigned char *valid, size_t n,
                                 uint64_t seq0);
hipError_t qs_launch_world_to_grid(qs_ctx *c, const double *w, size_t n, int axis, long long *out);
// raycast_tiled.hip
hipError_t qs_launch_raycast_tiled(qs_ctx *c, size_t n, uint64_t seq0);
bool qs_tiled_supported(const qs_ctx *c);
// veil.hip: the veil stage over the n packets whose ray slots pass A has just written to `rays`; *hit_valid becomes the array
// of masked hit flags that passes C and D are to read
hipError_t qs_launch_veil(qs_ctx *c, const uint2 *rays, size_t n, const unsigned char **hit_valid);
// ... and the sweep stage: qs_sweep_veil_reserve once per call (chunks of at most chunk_cap sweeps, n_call sweeps in all), then
// qs_launch_sweep_veil per chunk after the sweeps' pass A (accept, pose: the chunk's; k_call0: the record of the call its record 0 is)
hipError_t qs_sweep_veil_reserve(qs_ctx *c, size_t chunk_cap, size_t n_call);
hipError_t qs_launch_sweep_veil(qs_ctx *c, const unsigned char *d_pkts, size_t stride, const unsigned char *accept, const double *pose,
                                const uint2 *rays, size_t n, size_t k_call0, const unsigned char **hit_valid);
// sweep_graph.hip: signature and acceptance of n device-resident sweep records.  lm_out == nullptr: into the batch arrays from
// record k0 on (QsBatch fields, graph_batch, agent_ev); otherwise only lm_out[k] (255 = rejected), nothing of the context
hipError_t qs_launch_sweep_signatures(qs_ctx *c, const qs_sweep_graph_params &p, const unsigned char *d_pkts, size_t n, size_t stride,
                                      const unsigned short *d_lens, size_t k0, unsigned char *lm_out);
// graph mode's pass over all n records of a sweep call before any chunk is mapped: signatures into the batch, then the SLAM stage.
// host: pkts / lens are host buffers, staged `chunk` records at a time
int qs_sweep_graph_pass(qs_ctx *c, const uint8_t *pkts, bool host, size_t n, size_t stride, const uint16_t *lens, size_t chunk);
// match.hip: the parameters of one matching call, checked against the context's sweep filter and resolution
struct QsMatchSetup { int R, W, T, min_hits, min_percent, reach; double step; };
int qs_match_setup(qs_ctx *c, const qs_match_params *params, const char *who, QsMatchSetup &ms);
// the limits of qs_match_params alone, shared with trail matching (trail.hip): p = *params or the defaults; the text of the
// first limit broken, or nullptr
const char *qs_match_params_check(const qs_match_params *params, qs_match_params &p);
// the reach limit of both, reach = ceil(. / res) cells: the patch, then the window, within QS_MATCH_MAX_REACH; fills ms from p.
// The refusal opens with `what` ("the sweep filter's smax") and names the length as `expr` ("smax")
int qs_match_reach_setup(qs_ctx *c, const char *who, const qs_match_params &p, double reach, const char *what, const char *expr,
                         QsMatchSetup &ms);
// n device-resident records matched against the map as the stream finds it; rot (optional): [n][2 T + 1][2] the (sin, cos) used;
// graph_k0 as qs_sweep_args takes it (sweep_common.h): QS_SWEEP_NO_GRAPH, or the record of a graph-mode call the n records start at
hipError_t qs_launch_match(qs_ctx *c, const QsMatchSetup &ms, const unsigned char *d_pkts, size_t n, size_t stride,
                           const unsigned short *d_lens, qs_sweep_match *out, double *rot, size_t graph_k0);
// c->match_tab, filled on first use: cos, sin of the 181 beam angles (i - 90) * (pi / 180) from the host's libm
hipError_t qs_beam_table(qs_ctx *c);
// what every call that reads sweeps without mapping them refuses: another stride, a sharded context, 2^31 records or more
int qs_sweep_call_ok(qs_ctx *c, size_t n, size_t stride, const char *who);
// check.hip: the parameters of one checking call, checked against the context's sweep filter and resolution
struct QsCheckSetup { int C, min_checked, max_bad_percent, count_missed; double tol; };
int qs_check_setup(qs_ctx *c, const qs_check_params *params, const char *who, QsCheckSetup &cs);
// n device-resident records checked against the map as the stream finds it; cls (optional): [n][181] the beams' classes
hipError_t qs_launch_check(qs_ctx *c, const QsCheckSetup &cs, const unsigned char *d_pkts, size_t n, size_t stride,
                           const unsigned short *d_lens, qs_sweep_check *out, unsigned char *cls);
// grid_ops.hip
hipError_t qs_launch_rebase(qs_ctx *c);
hipError_t qs_launch_fuse(qs_ctx *c, const unsigned int *const *d_src_stamps,
                          const unsigned long long *const *d_src_counts, size_t n_src, size_t cell_off, size_t n_cells,
                          unsigned long long *dst_counts);
hipError_t qs_launch_reset_small(qs_ctx *c);
// order-preserving compactions (compact.h): d_xy / d_pos == nullptr runs count and scan (chunk offsets into d_chunk,
// [qs_compact_chunks(items)], the total into *d_count), otherwise the ranked writes of the first `cap` items.
// cells > 50 of an int8 grid -> points; occupied (odd) stamps of a context's own map -> the same points;
// positions where a sorted key array starts a new run
hipError_t qs_launch_grid_to_pcd(qs_ctx *c, const signed char *d_grid, int h, int w, double res, double ox, double oy, double *d_xy,
                                 size_t cap, unsigned long long *d_count, unsigned int *d_chunk);
hipError_t qs_launch_stamps_to_pcd(qs_ctx *c, const unsigned int *d_stamps, int h, int w, double res, double ox, double oy, double *d_xy,
                                   size_t cap, unsigned long long *d_count, unsigned int *d_chunk);
hipError_t qs_launch_run_heads(qs_ctx *c, const unsigned long long *d_keys, size_t n, unsigned int *d_pos, size_t cap,
                               unsigned long long *d_count, unsigned int *d_chunk);
// box4 (ordered u64: min x, min y, max x, max y; the caller stores the identities first) of n points; the canvas of a cloud
hipError_t qs_launch_bbox(qs_ctx *c, const double *d_xy, size_t n, unsigned long long *d_box4);
hipError_t qs_launch_rasterise(qs_ctx *c, const double *d_xy, size_t n, double res, double minx, double miny, int h, int w,
                               signed char *d_grid);
// sparse_fuse.hip
hipError_t qs_launch_sf_mark_range(qs_ctx *c, size_t cell_off, size_t n_cells);
hipError_t qs_launch_sf_list_of(qs_ctx *c, const unsigned int *bitmap, size_t words, int pitch, int blocks_x, unsigned int *list,
                                unsigned int *count);
// frontier.hip
// the workspace of the labelling and the compactions, carved from ws (nullptr: only the bytes the block needs):
// [cells] labels, cells and sums of gx, gy per cluster (at its root); [chunks] counts of a compaction -> offsets; their sum
struct QsFrLayout { unsigned int *label, *cnt; unsigned long long *sumx, *sumy; unsigned int *chunk; unsigned long long *total; size_t bytes; };
QsFrLayout qs_frontier_layout(const qs_ctx *c, void *ws);
hipError_t qs_launch_frontier_label(qs_ctx *c, void *ws, bool with_clusters);
// frontier_targets.hip: the centroids of the clusters of a labelled frontier workspace with >= min_cluster cells, in first-cell
// order.  phase 0 counts them (QsFrLayout::total); phase 1 writes them all to d_cent, which holds that many
hipError_t qs_launch_ft_centroids(qs_ctx *c, void *fr_ws, int32_t min_cluster, int phase, double2 *d_cent);
// what every call over those centroids starts with: the sync point, the frontier workspace reserved (-> fws) and labelled,
// phase 0, and one wait for the count (-> n_cent)
int qs_count_centroids(qs_ctx *c, int32_t min_cluster, void *&fws, size_t &n_cent);
// targets_by_path.hip: cell[0 .. n_cent) of the centroids -> their offsets in a field over the census box bbox (0xffffffff =
// no cell); count[0] += centroids with a cell, count[1] += cells among cell[n_cent .. n_cent + n_bots), the bots'
hipError_t qs_launch_tbp_offsets(qs_ctx *c, const long long *cell, size_t n_cent, size_t n_bots, const unsigned int bbox[4],
                                 unsigned int *coff, unsigned long long *count);
// gain.hip: the workspace of the viewpoints and gains of n_cent clusters, carved from ws (nullptr: only the bytes the block
// needs): the kept roots in slot order, the viewpoint keys (d2 << 32) | cell, then what the calls read: (gx, gy) and the gain
struct QsGainLayout { unsigned int *root; unsigned long long *key; int2 *view; int *gain; size_t bytes; };
QsGainLayout qs_gain_layout(void *ws, size_t n_cent);
// into G.view / G.gain, for the n_cent clusters that qs_launch_ft_centroids(.., min_cluster, 0, ..) has just counted in fr_ws
hipError_t qs_launch_gain(qs_ctx *c, void *fr_ws, int32_t min_cluster, int32_t range, size_t n_cent, const QsGainLayout &G);
int gain_range(qs_ctx *c, int32_t range, const char *who);      // G5: QS_OK, or QS_E_INVAL with a message
// icp.hip
hipError_t qs_launch_voxel_keys(qs_ctx *c, const double2 *pts, size_t n, double minx, double miny, double voxel, unsigned long long *keys);
int qs_icp_device(qs_ctx *c, double2 *d_src, size_t n_src, const double2 *d_dst, size_t n_dst, const double box[4], double max_dist,
                  int32_t max_iter, double rel_fitness, double rel_rmse, double T[9], double *fitness, double *rmse, int32_t *iters);
// ekf.hip
hipError_t qs_launch_ekf_ingest(qs_ctx *c, size_t n, const double *d_time, hipStream_t st);
// ekf_scan.hip: the same filter over a large batch, parallel in time
#define QS_EKF_SCAN_MIN_BATCH 4096
hipError_t qs_launch_ekf_scan(qs_ctx *c, size_t n, const double *d_time, hipStream_t st);
