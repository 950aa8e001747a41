/*
 * quasar_slam.h -- C ABI of the MI355X-native central-mapper hot path.
 *
 * The reference (deevinandu/Distributed-Multi-Agent-SLAM-Swarm-Robotics-System) has no
 * FFI: its boundary is the Python object API used by server_nodes/dual_bot_mapper.py's
 * main() and MapRenderer.  Every entry point below names the reference interface it
 * replaces (file:line, relative to the reference tree).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every call returns 0 on success, <0 on error (QS_E_*); qs_last_error() gives text;
 *   - one context = one GPU = one mapper instance; calls on one context are serialised by
 *     the caller (the reference is single-threaded); contexts are independent;
 *   - the caller owns every buffer it passes; the library owns all device state;
 *   - "host" pointers are ordinary memory, "device" pointers are HIP device memory on the
 *     context's GPU; work is enqueued on the context's stream and host-visible results are
 *     complete when the call returns (device variants: after qs_sync()).
 */
#ifndef QUASAR_SLAM_H
#define QUASAR_SLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QS_OK 0
#define QS_E_INVAL (-1)    /* bad argument */
#define QS_E_HIP (-2)      /* HIP runtime error (text in qs_last_error) */
#define QS_E_NOMEM (-3)
#define QS_E_RANGE (-4)    /* index (bot, graph, capacity) out of range */
#define QS_E_NODEV (-5)    /* no usable GPU */
#define QS_E_STATE (-6)    /* call not valid in the context's current state (text in qs_last_error) */

/* wire formats: dual_bot_mapper.py:41-54 */
#define QS_PACKET_SIZE 42     /* QuasarPacket v2 '<4sBfffiIffffB' */
#define QS_PACKET_SIZE_V1 41  /* QuasarPacket v1 '<4sBfffiIffff'  */
#define QS_ZONE_SIZE 20       /* ZONE '<4sffff' */

typedef struct qs_ctx qs_ctx;

typedef struct qs_config {
    /* OccupancyGrid(size, resolution, origin_x, origin_y)  dual_bot_mapper.py:113-119 */
    int32_t size;
    double res, ox, oy;
    double separation;          /* --separation, added to bot 2's x   :715, :851-852 */
    double min_dist, max_dist;  /* MIN_DIST_M, MAX_DIST_M            :57-58  */
    double closure_radius;      /* CLOSURE_RADIUS                     :97  */
    int32_t min_poses_between;  /* MIN_POSES_BETWEEN                  :98  */
    double closure_correction;  /* CLOSURE_CORRECTION                 :99  */
    int32_t max_agent;          /* accept agent_id 1..max_agent; reference: 2 (:842) */
    int32_t bots_per_graph;     /* bots sharing one PoseGraphSLAM; 0 = all (reference) */
    int32_t enable_counts;      /* keep per-cell hit/miss counters (build extension) */
    int32_t enable_ekf;         /* run the firmware EKF per bot on ingest (ekf.cpp) */
    double ekf_metres_per_tick; /* encoder scale for the EKF wiring (generator: 0.0107) */
    int32_t device;             /* HIP device ordinal */
    int32_t raycast_mode;       /* 0 = auto, 1 = direct global atomics, 2 = LDS tile-binned */
    int32_t seq_stride;         /* arrival index of record i = seq0 + i*seq_stride (0 = 1); a rank of an
                                   N-way round-robin sharded stream uses seq0 = base + rank, stride N */
    int32_t shard_bots;         /* > 0: this context is shard `shard_rank` of a deployment that keeps ONE pose graph over all
                                   bots (PoseGraphSLAM is global across bots, :275, :294-309): every shard ingests the whole
                                   interleaved stream (decode + loop closure replicated, identical on all shards) but casts
                                   rays, keeps zones and runs the EKF only for its own agents
                                   shard_rank*shard_bots+1 .. (shard_rank+1)*shard_bots.  0 = the context owns every agent */
    int32_t shard_rank;
    int32_t exact_trig;         /* 1 (default): rays whose end point falls within 1e-9 cells of a cell boundary -- where a last-bit
                                   difference between the device's sin / cos and glibc's (CPython's math.cos / math.sin) could
                                   change a cell index -- are not cast by the device but wait, self-contained, for the host to
                                   recompute their end points with libm: at the next call that observes the map (grid / counter /
                                   frontier reads, qs_device_buffers, a fuse, qs_counters, qs_sync).  qs_ingest_device itself never
                                   waits for the GPU.  0: device trig only */
    int32_t reserved[3];
} qs_config;

/* reference constants (dual_bot_mapper.py:57-99) */
int qs_config_default(qs_config *cfg);

int qs_create(const qs_config *cfg, qs_ctx **out);
int qs_destroy(qs_ctx *ctx);
const char *qs_last_error(const qs_ctx *ctx);   /* ctx may be NULL: last create error */
/* run on the caller's hipStream_t (e.g. torch's current stream); NULL = own stream */
int qs_set_stream(qs_ctx *ctx, void *hip_stream);
int qs_sync(qs_ctx *ctx);
/* new session: grid -> UNKNOWN, pose graphs, drift, zones, EKF cleared (main() start, :755-785).  The fuse state goes
 * too: counters, fused counters and dirty bitmaps zeroed, a sparse fuse in flight dropped, and the counts view back on the
 * local counters until the session's first fuse -- a reset context shows what a new one would.  Dirty tracking and the
 * chain form (qs_set_chain_form) are kept.  Enqueued on the context's stream like an ingest; does not wait for the GPU. */
int qs_reset(qs_ctx *ctx);
/* per-bot x offset; bot 2 defaults to cfg.separation (:851-852) */
int qs_set_bot_offset(qs_ctx *ctx, int32_t bot, double off_x);

/* ---- ingest: the batched body of the recv loop, dual_bot_mapper.py:826-919 ------------
 * n datagrams, record i at pkts + i*stride, its length lens[i] (NULL: every length ==
 * stride).  42-byte v2 and 41-byte v1 records are decoded, anything else, a bad magic or
 * an agent outside 1..max_agent is dropped (:826-843).  recv_time (seconds, may be NULL)
 * feeds only the EKF wiring.  seq0 = arrival index of record 0 in the global stream
 * (UINT64_MAX: continue this context's own counter); later records win grid cells. */
int qs_ingest(qs_ctx *ctx, const uint8_t *pkts, size_t n, size_t stride,
              const uint16_t *lens, const double *recv_time, uint64_t seq0);
/* same with device-resident inputs; asynchronous on the context's stream */
int qs_ingest_device(qs_ctx *ctx, const uint8_t *d_pkts, size_t n, size_t stride,
                     const uint16_t *d_lens, const double *d_recv_time, uint64_t seq0);
/* per record of the LAST ingest: accepted flag and pose after offset+drift (:850-857) */
int qs_last_batch(qs_ctx *ctx, uint8_t *accepted, double *pose_xyyaw /* n x 3 */, size_t n);
/* valid hit points of the LAST ingest (point_clouds[agent][sensor].append, :892):
 * 4 slots per record in sensor order front,left,back,right; valid[i*4+s] marks used slots.
 * Computed on request from the batch that is still resident (one extra kernel): the map update itself
 * only needs the rays' grid cells. */
int qs_last_hits(qs_ctx *ctx, double *xy /* n x 4 x 2 */, uint8_t *valid /* n x 4 */, size_t n);

/* ---- bot veil (no reference counterpart: this build's own rule) --------------------------------------------------------------
 * The bots of a swarm drive in the same rooms, and a beam that ends on another bot would leave an OCCUPIED cell in free space.
 * With the veil on, a packet beam whose end cell lies within `radius` cells of the cell where another bot was last heard is
 * cast as a free ray without its end cell: the space up to the bot is free, what lies at and behind it is not known from this
 * beam.  Off by default; with it off every call, buffer and launch is what it is without this section.  All integer:
 *   V1  The cell of an accepted packet is world_to_grid (int((w - o) / res), :121-125) of its pose after offset and drift, on
 *       both axes -- the pose qs_last_batch reports.  A pose that is not finite, or whose cell on either axis does not lie
 *       strictly inside +-2^30, has no cell.
 *   V2  The context keeps a table cell[bot], bot 1..max_agent: unknown, or known with an (x, y).  qs_reset empties it;
 *       qs_restore empties it (checkpoints do not carry it; their format does not know of it).
 *   V3  For ray s of accepted packet i with agent a, and every bot b != a: the cell of the last accepted packet q < i of this
 *       call with agent b that has a cell; failing that the table's entry for b as it stood when the call began; failing that
 *       there is nothing to test for b.  Rejected packets and packets without a cell never count.
 *   V4  The ray is VEILED when all of these hold: its hit flag is set (min_dist < d <= max_dist); the tiled raycast binned it
 *       (it was not left to the host by the exact-trig rule and is shorter than 64 cells on both axes: a longer one is written
 *       directly); its end cell (x1, y1) lies inside the grid (outside there is nothing to withhold); and for some b of V3
 *       (x1 - bx)^2 + (y1 - by)^2 <= radius^2.
 *   V5  A veiled ray's free cells are written as before; its end cell gets neither stamp nor counter.  Nothing else changes:
 *       qs_last_hits, the zone boxes, QS_CNT_HITS / RAYS and the pose graph see the beam as the filter judged it.
 *       (QS_CNT_CELLS counts cells written, so it is lower by one per veiled ray.)
 *   V6  After the call cell[b] is the cell of b's last accepted packet with a cell; unchanged for bots the call did not hear.
 *   V7  Never veiled: rays left to the host (exact_trig) and rays written directly (V4); qs_update_rays.  Sweep beams are
 *       veiled only under the sweep switch (S0-S8 below); without it no sweep entry point reads or feeds the table, and sweep
 *       bots reach it through qs_bot_veil_place only.
 * A veiled context casts every packet ingest in the tiled form, whatever n is (the direct kernel writes the end cell before
 * anything could veil it); both forms write the same cells.
 * qs_set_bot_veil: radius in cells, 1..QS_BOT_VEIL_MAX_RADIUS, 0 = off; the table is kept.  QS_E_INVAL (and the setting
 * unchanged) beyond the range, for raycast_mode == 1, for a grid the tiled form does not support (more than 8192 cells a
 * side), and for sharded contexts (seq_stride > 1 or shard_bots > 0).  Kept over qs_reset and qs_restore.
 * qs_bot_veil_place: cell[bot] by V1 from a world position (a sweep bot, a charging dock given a spare id); QS_E_RANGE for a
 * bot outside 1..max_agent or a position without a cell.  qs_bot_veil_forget: cell[bot] unknown; bot 0: all of them.
 * qs_bot_veil_cells: the table; xy[2 b], xy[2 b + 1] and known[b] for b = 0..max_agent (entry 0 is never known).
 * qs_last_veiled: the flags of the last packet ingest, 4 per record (n must match, as qs_last_hits); all zero after an ingest
 * with the veil off; QS_E_INVAL unless the last ingest was a packet ingest (after a sweep ingest, qs_update_rays, qs_reset,
 * qs_restore).  qs_bot_veil_stats: rays veiled since qs_create / qs_reset / qs_restore -- a restore, into the same context too,
 * starts the count at 0 as it empties the table: a checkpoint carries neither, and QS_CNT_CELLS, which it does carry, already
 * tells what the restored map holds.  qs_bot_veil_time: with qs_timing_enable, the
 * veil stage's own milliseconds and launches (a part of QS_STAGE_RAYCAST; it is no stage of qs_stage_times).
 *
 * The veil for sweeps.  A sweep bot with another bot in front of it hits it with a fan of its 181 beams.  All integer, as V1-V7:
 *   S0  qs_set_bot_veil_sweeps sets the switch, qs_bot_veil_sweeps reads it; off by default, kept across qs_set_bot_veil, qs_reset
 *       and qs_restore.  The sweep veil ACTS only while the switch is on and the veil radius is greater than 0.  Otherwise every
 *       sweep entry point does, launches and allocates exactly what it does without this section, and the table is neither read
 *       nor fed by sweeps.  (No refusals of its own: qs_set_bot_veil has refused what the stage cannot serve.)
 *   S1  The cell of an accepted sweep is V1's world_to_grid of the pose it is cast from -- the pose qs_last_sweeps reports: after
 *       offset and drift in the plain ingest, after the correction in the matched ingest, the chain's pose in graph mode.  A pose
 *       that is not finite or lies beyond +-2^30 cells has no cell.  A rejected record has no cell and does not speak; a record
 *       the guarded ingest withholds counts as rejected.
 *   S2  For a beam of accepted sweep k with agent a, every bot b != a speaks through its last accepted sweep with a cell before k
 *       in the call -- over the whole call, across the 2^16-record chunks; failing that through the table as the call found it.
 *       The table is V2's, the one packets use: a sweep bot veils packet beams of later packet ingests, and the other way round.
 *   S3  The beam is VEILED when all of these hold: its hit flag is set (smin < d <= smax); the tiled raycast binned it (a beam of
 *       64 cells or more on an axis is written directly, a beam the exact-trig rule leaves to the host is cast later: neither is
 *       ever veiled); its end cell (x1, y1) lies inside the grid; (x1 - bx)^2 + (y1 - by)^2 <= radius^2 for some speaking b != a.
 *   S4  A veiled beam's free cells are written; its end cell gets neither stamp nor counter.  QS_CNT_RAYS, QS_CNT_HITS, graph
 *       mode's zone points and the landmark signature see the beam as the filter judged it; QS_CNT_CELLS is lower by one per
 *       veiled beam.
 *   S5  After the call the table holds the last cell of every bot heard in it, from the pose and unclamped, as V6.
 *   S6  With the sweep veil acting every sweep ingest takes the tiled form, whatever n is; both forms write the same cells.
 *   S7  qs_last_sweeps_veiled: the flags of the last sweep ingest, 181 per record (n must match, as qs_last_sweeps); all zero
 *       after an ingest during which the sweep veil was not acting.  A refused sweep ingest is no ingest: the flags of the one
 *       before it stay (below).  QS_E_INVAL where qs_last_sweeps refuses: after a packet ingest, a sweep ingest with n = 0,
 *       qs_update_rays, qs_reset, qs_restore.
 *   S8  Veiled sweep beams add to the word qs_bot_veil_stats reads; the stage's time adds to what qs_bot_veil_time reports.
 * Not veiled: what qs_check_sweeps, the matchers and the relocalisers read (beams as the filter judged them). */
#define QS_BOT_VEIL_DEFAULT_RADIUS 3
#define QS_BOT_VEIL_MAX_RADIUS 32
int qs_set_bot_veil(qs_ctx *ctx, int32_t radius_cells);
int qs_bot_veil(qs_ctx *ctx, int32_t *radius_cells);
int qs_bot_veil_place(qs_ctx *ctx, int32_t bot, double x, double y);
int qs_bot_veil_forget(qs_ctx *ctx, int32_t bot);
int qs_bot_veil_cells(qs_ctx *ctx, int32_t *xy /* (max_agent + 1) x 2 */, uint8_t *known /* max_agent + 1 */);
int qs_last_veiled(qs_ctx *ctx, uint8_t *veiled /* n x 4 */, size_t n);
int qs_bot_veil_stats(qs_ctx *ctx, uint64_t *veiled_total);
int qs_bot_veil_time(qs_ctx *ctx, double *ms, uint64_t *launches, int32_t reset);
int qs_set_bot_veil_sweeps(qs_ctx *ctx, int32_t on);
int qs_bot_veil_sweeps(qs_ctx *ctx, int32_t *on);
int qs_last_sweeps_veiled(qs_ctx *ctx, uint8_t *veiled /* n x 181 */, size_t n);

/* ---- servo sweeps ("Quasar-Lite" packets) ----------------------------------------------------------------------------
 * A sweep carries a pose and 181 ranges swept from -90 to +90 degrees about the heading:
 *   v0              '<4sBfffH181f'   743 bytes  (esp32_firmware/src/main.cpp:33-41; udp_bridge.py:25-38)
 *   v0 + odometry   '<4sBfffiIH181f' 751 bytes  (i32 encoder, u32 v2v before scan_count; udp_receiver_standalone.py:15)
 * The reference maps sweeps only in its top-down plot (generate_topdown_map.py:39-57); here they go into the occupancy grid
 * with the reference's own update_ray (:136-179), so that every cell can be checked against it:
 *   accept   length == stride (743 or 751: one format per call), magic 'QSRL', agent in 1..max_agent; scan_count is
 *            ignored (udp_bridge.py:71).  A rejected record writes nothing but still uses its sequence numbers.
 *   pose     rx = f64(x) + offset[bot] + drift_x[bot], ry = f64(y) + drift_y[bot] (offset first, then drift, as :851-857):
 *            qs_set_bot_offset / separation, and the bot's closure correction as all earlier calls on the context's stream
 *            left it (read on the device).  A sweep adds NO pose-graph node, landmark, EKF step or zone point, unless the
 *            context is in graph mode (qs_set_sweep_graph, "sweeps in the pose graph" below: off by default).
 *   beams    beam i has angle a = f64(yaw) + (i - 90) * (pi / 180) (CPython's math.radians; one multiply, one add, no FMA).
 *            d = the f32 range widened: smin < d <= smax is a hit, update_ray(rx, ry, rx + d cos a, ry + d sin a, True);
 *            any other beam (NaN, 0, negative included) a free ray of length min(d, smax) if d > smin else smax.
 *            Defaults smin = 0.1, smax = 1.2 (generate_topdown_map.py:51); qs_set_sweep_filter changes them for the
 *            context (kept over qs_reset).
 *   order    sweep k of a call owns the QS_SWEEP_SEQS sequence numbers seq0 + 46 k .. seq0 + 46 k + 45; beam i has stamp
 *            ordinal 4 (seq0 + 46 k) + i + 1, so a later beam of a sweep wins a cell over an earlier one, and a later
 *            packet of either kind over an earlier one.  Afterwards the context's next sequence number is seq0 + 46 n.
 *   writes   grid stamps, hit / miss counters (enable_counts), dirty blocks (qs_dirty_tracking): nothing else.  Counters
 *            QS_CNT_DATAGRAMS / ACCEPTED / RAYS / CELLS / HITS count sweeps and beams as they count packets and rays.
 *   trig     exact_trig: beams whose end point lies in the 1e-9 edge band are resolved on the host with libm, as rays are.
 * Any n: the call is split into chunks internally.  QS_E_INVAL for another stride, seq_stride > 1 or shard_bots > 0
 * (sharded sweeps are not supported).  After a sweep call qs_last_batch / qs_last_hits refuse (length mismatch);
 * qs_last_sweeps returns per record the accepted flag and the pose used (NaN for rejected records).
 * A refused sweep ingest -- another stride, a sharded context, a bad parameter of the matched or guarded form, the guarded form
 * in graph mode -- changes nothing: qs_last_sweeps, qs_last_sweep_matches, qs_last_sweep_checks, qs_last_sweep_nodes and
 * qs_last_sweeps_veiled go on answering for the ingest before it, and qs_last_batch / qs_last_veiled if that was a packet ingest.
 * A call with n = 0 is an ingest of nothing: the map stays, and after it all of these refuse. */
#define QS_SWEEP_SIZE_V0 743
#define QS_SWEEP_SIZE_V0_ODO 751
#define QS_SWEEP_BEAMS 181
#define QS_SWEEP_SEQS 46      /* sequence numbers per sweep: 184 stamp ordinals, beams in the first 181 */
#define QS_SWEEP_SLOTS (4 * QS_SWEEP_SEQS)
int qs_ingest_sweeps(qs_ctx *ctx, const uint8_t *pkts, size_t n, size_t stride, const uint16_t *lens, uint64_t seq0);
/* same with device-resident inputs; asynchronous on the context's stream */
int qs_ingest_sweeps_device(qs_ctx *ctx, const uint8_t *d_pkts, size_t n, size_t stride, const uint16_t *d_lens,
                            uint64_t seq0);
int qs_last_sweeps(qs_ctx *ctx, uint8_t *accepted, double *pose_xyyaw /* n x 3 */, size_t n);
/* trust filter of the sweep beams: a hit when smin < d <= smax (finite, 0 <= smin < smax) */
int qs_set_sweep_filter(qs_ctx *ctx, double smin, double smax);

/* ---- sweeps in the pose graph (graph mode; no reference counterpart: this build's own rule) ------------------------------------
 * The firmware that sends sweeps (esp32_firmware/src/main.cpp) computes no landmark byte; the one that does
 * (AgentFirmware_Bot1.ino:152-169, detectLandmark) reads fixed sonars to the front, left and right.  A sweep holds the same three
 * directions: beam 0 is right, beam 90 front, beam 180 left.  In graph mode the library derives the signature itself, adds the
 * sweep as a pose-graph node, runs the loop-closure chain and casts the sweep from the pose the chain gives it -- what the
 * 42-byte path does for a packet.  All comparisons are on exact values: a NumPy restatement (tests/sweep_graph_rules.py) agrees
 * bit for bit.
 *  setting   qs_set_sweep_graph(ctx, enable, params); params NULL = half_width 5, close 0.40, open 0.80 (the firmware's 40 cm
 *            and 80 cm).  Limits: 0 <= half_width <= 29 (the three sectors never share a beam), finite 0 < close <= open;
 *            QS_E_INVAL otherwise, the text names the field.  Kept over qs_reset (as the sweep filter and the chain form), NOT
 *            saved in a checkpoint: qs_restore leaves the context's current setting alone.  Off (the default): every call
 *            behaves as described above.  A sharded context refuses sweeps either way.
 *  accept    qs_ingest_sweeps' rule, and x, y, yaw finite (the packet path's test).  ONE decision per record: the signature
 *            pass makes it, matching and mapping read it.
 *  sectors   w = half_width.  Right: beams 0 .. 2w; front: 90 - w .. 90 + w; left: 180 - 2w .. 180; 2w + 1 beams each.  A range
 *            is usable when finite and > 0; any other (NaN, +-inf, 0, negative) counts as +inf (the firmware's timeout reads
 *            as "far", :239).  The sector value S is the element of rank w (0-based) of the 2w + 1 values ordered by (value,
 *            beam index): the median, the cheapest rule that ignores one stray echo.  w = 0: the single beams 0, 90, 180.
 *  decision  detectLandmark on S widened to fp64: X_close = S_X < close, X_open = S_X > open.  DEAD_END (4) if front, left and
 *            right are close; else CORNER_L (1) if front and left; else CORNER_R (2) if front and right; else CORRIDOR (3) if
 *            left and right are close and front is open; else OPEN (5) if all three are open; else NONE (0).
 *            (f32(0.4) widens to 0.4000000059604645, which is not < 0.40.)
 *  node      every accepted sweep is one PoseGraphSLAM.add_pose(rx, ry, yaw, agent, lm) (:273-326) in record order within the
 *            call, continuing the node index of its graph (shared with packets, per bots_per_graph): px = f64(x) +
 *            offset[bot], py = f64(y), rx = px + drift_x, ry = py + drift_y with the bot's drift BEFORE this record's own
 *            closure -- what the packet path reports as its pose.  A closure at sweep k moves the sweeps of that bot after k in
 *            the same call.  closure_radius, min_poses_between, closure_correction are the context's.
 *  mapping   beams are cast by qs_ingest_sweeps' rules from (rx, ry, yaw).  Matched ingest: signature, chain, then the match
 *            from the chain's (rx, ry) against the map as it stood before the call, then the map from rx + dx, ry + dy,
 *            yaw + dyaw.  The match correction does not enter the graph: the node is the drift-corrected packet pose.
 *  zone      per accepted sweep the pose it is cast from is a path point (:878-879) and the end point of every hit beam a cloud
 *            point (:892) of the bot's zone box (qs_zone), both from the device's trig whether or not the beam waits in the
 *            exact-trig edge band (as for packets).
 *  no EKF    the sweep entry points carry no receive time: a sweep is no EKF step in either mode.
 *  the rest  stamps, sequence numbers (46 per sweep), QS_CNT_*, dirty blocks and chunking as qs_ingest_sweeps.  The four sweep
 *            ingest entry points keep their signatures; qs_last_sweeps reports the pose each sweep was cast from. */
#define QS_SWEEP_GRAPH_MAX_HALF_WIDTH 29
typedef struct qs_sweep_graph_params { int32_t half_width, reserved; double close, open; } qs_sweep_graph_params;
int qs_set_sweep_graph(qs_ctx *ctx, int32_t enable, const qs_sweep_graph_params *params);
int qs_sweep_graph(qs_ctx *ctx, int32_t *enabled, qs_sweep_graph_params *out);
/* rule only, writes nothing to the context (tests and tools): lm_out[k] = signature, 255 for a rejected record.
 * params NULL = the context's current parameters (the defaults unless set) */
int qs_sweep_signatures(qs_ctx *ctx, const qs_sweep_graph_params *params, const uint8_t *pkts, size_t n, size_t stride,
                        const uint16_t *lens, uint8_t *lm_out);
/* same with device-resident pkts / lens / lm_out; asynchronous on the context's stream */
int qs_sweep_signatures_device(qs_ctx *ctx, const qs_sweep_graph_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                               const uint16_t *d_lens, uint8_t *d_lm_out);
/* after a sweep ingest in graph mode: node index in the record's graph (-1: rejected) and signature (255: rejected);
 * QS_E_INVAL otherwise */
int qs_last_sweep_nodes(qs_ctx *ctx, int64_t *node, uint8_t *lm, size_t n);

/* ---- sweep matching (no reference counterpart: this build's own rule) ------------------------------------------------------
 * A sweep is matched against the map before it is mapped: a window of candidate poses around the packet's pose is scored
 * on a likelihood field of the occupied cells, and the best candidate is the correction.  Integers are exact, floating
 * point is fp64 without contraction, so the device and a CPU restatement (tests/match_rules.py) agree bit for bit once
 * they share the (sin, cos) of the rotations.
 *  1. Field: for a radius R in 0..QS_MATCH_MAX_RADIUS, L[gy][gx] = max(0, R + 1 - c), c the Chebyshev distance from
 *     (gx, gy) to the nearest OCCUPIED cell of the grid (odd stamp; the 100 of qs_grid_i8).  UNKNOWN and FREE are not
 *     told apart; L = 0 outside the grid.
 *  2. Candidates (ix, iy, it): |ix|, |iy| <= window (cells), |it| <= angle_steps (steps of angle_step radians).
 *  3. Per accepted record (qs_ingest_sweeps' acceptance rule): rx, ry as qs_ingest_sweeps forms them (offset first, then
 *     the bot's drift, read on the device), yaw = f64(packet yaw).  Hit beams: smin < d_i <= smax (the context's sweep
 *     filter); only they score, H is their number.  Beam in the robot frame: bx_i = d_i * CB[i], by_i = d_i * SB[i], with
 *     CB, SB the cos / sin of (i - 90) * (pi / 180) from the HOST's libm (uploaded once per context).
 *     Rotation it: th = yaw + it * angle_step (one multiply, one add), (s, c) = the device's sincos(th): 2 T + 1 per sweep.
 *     End point ex = rx + (c * bx_i - s * by_i), ey = ry + (s * bx_i + c * by_i), in this association; its cell
 *     (cx, cy) = world_to_grid (int((w - o) / res), :121-125).  An end point whose quotient is not finite or is beyond
 *     2^30 cells in magnitude scores 0 (world_to_grid would raise).
 *     score(ix, iy, it) = sum over hit beams of L[cy + iy][cx + ix]: the translation shifts the look-up, not the pose.
 *  4. Best candidate: highest score; ties to the smallest ix*ix + iy*iy, then the smallest |it|, then the smaller it, then
 *     the smaller iy, then the smaller ix.  One total order: the answer is unique.
 *  5. Gate: accepted_match when H >= min_hits and score * 100 >= min_percent * H * (R + 1).  Then dx = ix * res,
 *     dy = iy * res, dyaw = it * angle_step (one multiply each); otherwise all three are 0.  ix, iy, it, score report the
 *     best candidate either way; score0 is the score of (0, 0, 0).  An empty map never moves a sweep.
 * A rejected record gets zeros throughout (accepted_record = 0).
 * Limits: radius <= QS_MATCH_MAX_RADIUS, angle_steps <= QS_MATCH_MAX_ANGLE_STEPS, 0 <= min_percent <= 100, angle_step
 * finite and >= 0, and ceil(smax / res) + window + radius + 2 <= QS_MATCH_MAX_REACH, so that the patch of the field a sweep
 * can reach is at most 255 cells on a side.  QS_E_INVAL beyond them; the text says which quantity is too large.
 * params NULL = radius 2, window 6, angle_steps 10, angle_step pi / 180, min_hits 20, min_percent 50.
 *
 * qs_match_sweeps* read the map (waiting exact-trig rays are flushed first) and write nothing to the context: no stamps,
 * counters, dirty blocks or sequence numbers; a checkpoint before equals one after.  rot_out (optional) receives
 * n x (2 T + 1) x 2 doubles, the (s, c) the device used for it = -T .. T (zeros for rejected records): with them as input
 * the restatement is exact, whatever the last bit of the device's sincos.
 *
 * qs_ingest_sweeps_matched*: ALL records of the call are matched against the map as it stood before the call, however
 * the call is chunked; then they are mapped by the rules of qs_ingest_sweeps from the corrected pose rx' = rx + dx,
 * ry' = ry + dy, yaw' = yaw + dyaw (beam angle yaw' + (i - 90) * (pi / 180)).  Stamps, counters, sequence numbers, refusals
 * as qs_ingest_sweeps; qs_last_sweeps reports the corrected pose, qs_last_sweep_matches the matches (n = the call's n;
 * QS_E_INVAL after any other ingest).  With exact_trig a beam in the edge band waits for the host with its corrected
 * pose.  The bot's drift, the pose graphs, the EKF and the zone points are not touched (graph mode: see above). */
#define QS_MATCH_MAX_RADIUS 7
#define QS_MATCH_MAX_ANGLE_STEPS 45
#define QS_MATCH_MAX_REACH 127
typedef struct qs_match_params { int32_t radius, window, angle_steps, min_hits, min_percent, reserved; double angle_step; } qs_match_params;
typedef struct qs_sweep_match {
    int32_t ix, iy, it, score, score0, hits;
    uint8_t accepted_record, accepted_match, pad[6];
    double dx, dy, dyaw;
} qs_sweep_match;
/* rule 1 for the whole grid: field_host[gy*size + gx] (tests and tools) */
int qs_match_field(qs_ctx *ctx, int32_t radius, uint8_t *field_host);
int qs_match_sweeps(qs_ctx *ctx, const qs_match_params *params, const uint8_t *pkts, size_t n, size_t stride,
                    const uint16_t *lens, qs_sweep_match *out, double *rot_out);
/* same with device-resident pkts / lens / out / rot_out; asynchronous on the context's stream */
int qs_match_sweeps_device(qs_ctx *ctx, const qs_match_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                           const uint16_t *d_lens, qs_sweep_match *d_out, double *d_rot_out);
int qs_ingest_sweeps_matched(qs_ctx *ctx, const qs_match_params *params, const uint8_t *pkts, size_t n, size_t stride,
                             const uint16_t *lens, uint64_t seq0);
int qs_ingest_sweeps_matched_device(qs_ctx *ctx, const qs_match_params *params, const uint8_t *d_pkts, size_t n,
                                    size_t stride, const uint16_t *d_lens, uint64_t seq0);
int qs_last_sweep_matches(qs_ctx *ctx, qs_sweep_match *out, size_t n);

/* ---- relocalisation (no reference counterpart: this build's own rule) ------------------------------------------------------
 * A sweep whose pose is unknown (a bot that rebooted, was carried, or joins a map another bot drew) is located against the
 * whole map: every FREE cell of a search box and every rotation step is a candidate pose, scored on the likelihood field of
 * sweep matching.  There is no coarse level: the search is exhaustive.  Everything is integer or uncontracted fp64 and there
 * is no device trigonometry, so the device and the CPU restatement (tests/reloc_rules.py) agree bit for bit.
 *  G1. Field: sweep-matching rule 1 with radius R: L = max(0, R + 1 - Chebyshev distance to the nearest OCCUPIED cell), 0
 *      off the grid.
 *  G2. Rotations: n_rot in 1..360; th_j = j * (2 pi / n_rot) (one divide, one multiply).  (S_j, C_j) = (sin, cos)(th_j)
 *      from the HOST's libm, uploaded as the 181 beam CB / SB are.
 *  G3. Beams: record acceptance, hit beams (smin < d <= smax, the context's sweep filter), H, bx_i = d_i * CB[i] and
 *      by_i = d_i * SB[i] exactly as in sweep-matching rule 3.  The packet's pose, the bot's offset and its drift are NOT
 *      used.  For rotation j: ex = C_j * bx_i - S_j * by_i, ey = S_j * bx_i + C_j * by_i, in this association; cell offset
 *      ax = (int)floor(ex / res + 0.5), ay likewise: the robot stands at the centre of its cell.
 *  G4. Candidates (gx, gy, j): (gx, gy) inside the search box [x0, x1) x [y0, y1) clipped to the grid, the cell FREE (0 in
 *      qs_grid_i8).  use_box = 0: the whole grid.  score = sum over hit beams of L[gy + ay_i][gx + ax_i].
 *  G5. Order: higher score first, then smaller j, then smaller gy, then smaller gx.  The best is first in this order.
 *  G6. Rival: the first candidate in the same order among those with |gx - bx*| > sep or |gy - by*| > sep or a circular
 *      rotation distance min(|j - j*|, n_rot - |j - j*|) > sep_rot, (bx*, by*, j*) the best.  None qualifies: score2 = 0,
 *      gx2 = gy2 = j2 = -1.
 *  G7. Gate: accepted when H >= min_hits and score * 100 >= min_percent * H * (R + 1) and
 *      (score - score2) * 100 >= min_margin * H * (R + 1).
 *  G8. Pose: x = ox + (gx + 0.5) * res, y likewise, yaw = th_j, minus 2 pi when th_j > pi.  Reported whether or not the
 *      gate accepts.
 *  G9. Status: QS_RELOC_OK; QS_RELOC_NO_RECORD: the record is rejected, all other fields are zero; QS_RELOC_NO_CANDIDATE:
 *      the box holds no FREE cell, or H = 0 (accepted_record = 1, hits = H, the six cell fields -1, the rest zero).  An
 *      empty map gives score 0 and is never accepted (min_percent, min_margin > 0).
 * params NULL = radius 2, n_rot 180, sep 4, sep_rot 2, min_hits 40, min_percent 70, min_margin 5, the whole grid.
 * Limits: radius <= QS_MATCH_MAX_RADIUS, 16 + 2 * (ceil(smax / res) + radius + 1) <= 255, sep <= QS_RELOC_MAX_SEP,
 * sep_rot < n_rot, min_hits >= 0, min_percent and min_margin in 0..100.  QS_E_INVAL beyond any of them; the text names the
 * quantity.  Stride, lengths and refusals as qs_match_sweeps.
 * The calls read the map (waiting exact-trig rays are flushed first) and write nothing to the context: a checkpoint taken
 * before equals one taken after. */
#define QS_RELOC_MAX_ROT 360
#define QS_RELOC_MAX_SEP 16
#define QS_RELOC_OK 0
#define QS_RELOC_NO_RECORD 1
#define QS_RELOC_NO_CANDIDATE 2
typedef struct qs_reloc_params {
    int32_t radius, n_rot, sep, sep_rot, min_hits, min_percent, min_margin, use_box;
    int32_t x0, y0, x1, y1;
} qs_reloc_params;
typedef struct qs_sweep_reloc {
    int32_t gx, gy, j, score, hits;
    int32_t gx2, gy2, j2, score2;
    int32_t status;
    uint8_t accepted_record, accepted, pad[6];
    double x, y, yaw;
} qs_sweep_reloc;
int qs_relocalise_sweeps(qs_ctx *ctx, const qs_reloc_params *params, const uint8_t *pkts, size_t n, size_t stride,
                         const uint16_t *lens, qs_sweep_reloc *out);
/* same with device-resident pkts / lens / out; asynchronous on the context's stream (a call with another n_rot than the
 * last one, or one whose workspace has to grow, waits for the stream first) */
int qs_relocalise_sweeps_device(qs_ctx *ctx, const qs_reloc_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                const uint16_t *d_lens, qs_sweep_reloc *d_out);

/* ---- relocalisation of a group (no reference counterpart: this build's own rule) ------------------------------------------
 * One sweep is often ambiguous: a straight wall, a symmetric corner or an open floor has many equally good poses.  Several
 * sweeps of one bot, each with its pose in the bot's own (odometric) frame, form one rigid constellation of hit points; it is
 * located by the rule above, scored jointly.  The device and the CPU restatement (tests/reloc_group_rules.py) agree bit for bit.
 *  J1. Groups: the n records of a call are split into n_groups runs of consecutive records; gsize[g] lies in
 *      1..QS_RELOC_MAX_GROUP and the sizes sum to n.  QS_E_INVAL otherwise.
 *  J2. Relative poses: one qs_reloc_rel per record, the position (tx, ty) of that record's robot in the group's frame and the
 *      sin / cos (s, c) of its heading relative to that frame.  They are inputs: no device trigonometry, as in G2.  The
 *      packets' pose, the bot's offset and its drift are not read.
 *  J3. A record counts when G3's acceptance rule accepts it, its four rel values are finite and
 *      tx * tx + ty * ty <= travel * travel (uncontracted).  `records` is the number of counting records of the group.
 *  J4. Hit beams and bx, by as in G3.  Points in the group's frame: px = tx + (c * bx - s * by), py = ty + (s * bx + c * by),
 *      in this association.  H = the number of hit points over all counting records of the group.
 *  J5. Under rotation j: ex = C_j * px - S_j * py, ey = S_j * px + C_j * py; ax = floor(ex / res + 0.5), ay likewise.  With
 *      M = ceil((smax + travel) / res) + 1, a point whose |ax| or |ay| exceeds M, or is not a number, scores 0 under that
 *      rotation (an honest (s, c), s * s + c * c = 1, never gets there).  score = sum over the H points of L[gy + ay][gx + ax].
 *  J6. Candidates, order, rival and gate: G4-G8 unchanged, with this H; qs_reloc_params is the same.  The reported pose is
 *      the pose of the group's frame.
 *  J7. Status: QS_RELOC_NO_RECORD when records = 0 (all other fields zero); QS_RELOC_NO_CANDIDATE when H = 0 or the box
 *      holds no FREE cell; QS_RELOC_OK otherwise.  Field conventions as in G9.
 *  J8. Limits: those of the rule above with 16 + 2 * (ceil((smax + travel) / res) + radius + 1) <= 255; travel finite and
 *      >= 0.  QS_E_INVAL beyond them; the text names the quantity.
 * A group of one record with rel = (0, 0, 0, 1) and travel 0 gives the bytes of qs_relocalise_sweeps for that record
 * (1 * bx - 0 * by and 0 + bx are exact).
 * gsize is read by the HOST in both forms: it shapes the launches and J1 is refused before anything is enqueued.  Stride,
 * lengths and refusals as qs_relocalise_sweeps.  The calls read the map and write nothing to the context. */
#define QS_RELOC_MAX_GROUP 16   /* 16 records of 181 beams score at most 2896 * 8 = 23 168 with radius 7 (csrc/reloc.hip: RL_GPTS) */
typedef struct qs_reloc_rel { double tx, ty, s, c; } qs_reloc_rel;
typedef struct qs_group_reloc {
    int32_t gx, gy, j, score, hits;
    int32_t gx2, gy2, j2, score2;
    int32_t status;
    uint8_t records, accepted, pad[6];      /* pad is zero */
    double x, y, yaw;
} qs_group_reloc;
int qs_relocalise_groups(qs_ctx *ctx, const qs_reloc_params *params, const uint8_t *pkts, size_t n, size_t stride,
                         const uint16_t *lens, const qs_reloc_rel *rel, const int32_t *gsize, size_t n_groups, double travel,
                         qs_group_reloc *out);
/* same with device-resident pkts / lens / rel / out (gsize stays a host array, see above); asynchronous on the context's
 * stream, with the exceptions of qs_relocalise_sweeps_device */
int qs_relocalise_groups_device(qs_ctx *ctx, const qs_reloc_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                const uint16_t *d_lens, const qs_reloc_rel *d_rel, const int32_t *gsize, size_t n_groups,
                                double travel, qs_group_reloc *d_out);

/* ---- trail matching (no reference counterpart: this build's own rule) ------------------------------------------------------
 * The reference's robots send 42-byte packets: a pose and four sonar ranges (front, left, back, right).  One packet cannot
 * locate itself -- four points do not fix a pose -- but a TRAIL can: the last K packets of one bot, held together rigidly by the
 * bot's own odometry, whose hit points trace the walls the bot drove along.  A trail is matched against the map as a sweep is
 * ("sweep matching" above): a window of candidate corrections scored on the likelihood field, the rotation about the trail's
 * last pose.  Everything after the per-record (sin, cos) is integer or uncontracted fp64, so the device and the CPU restatement
 * (tests/trail_rules.py) agree bit for bit once they share those.
 *  T1. Groups: the n records are n_groups consecutive groups of gsize[g] records in arrival order, 1 <= gsize[g] <=
 *      QS_TRAIL_MAX_RECORDS, the sizes sum to n.  gsize is a HOST array in both entry points (as for qs_relocalise_groups).
 *  T2. Acceptance of a record is qs_ingest's own rule: length 42 or 41 and <= stride, magic, agent in 1..max_agent, and x, y,
 *      yaw finite.  The group's ANCHOR is its last accepted record; the group's bot is the anchor's agent.
 *  T3. Pose of accepted record k: rx = (f64(x) + offset[bot]) + drift_x[bot], ry = f64(y) + drift_y[bot], the bot's drift as all
 *      earlier calls on the context's stream left it (read on the device).  ONE drift is used for the whole trail: odometry is
 *      locally rigid, and a closure in the middle of a trail is a jump of the correction, not of the robot.  (ax, ay) is the
 *      anchor's pose.
 *  T4. A record counts when it is accepted, its agent is the group's bot, and (rx - ax)^2 + (ry - ay)^2 <= travel^2
 *      (uncontracted).  `records` is the number of counting records.  With none counting the output has anchor = -1 and every
 *      other field zero.
 *  T5. Points: (s, c) = the device's sincos(f64(yaw)), one per record, reported in rot_out[k] = (s, c) (zeros for records that
 *      do not count).  Sensor directions in sensor order are exact sign flips of those two numbers: front (c, s), left (-s, c),
 *      back (-c, -s), right (s, -c).  The range d is the f32 widened; it is a hit when min_dist < d <= max_dist (the context's
 *      trust filter, dual_bot_mapper.py:888).  Only hits score; H is their number over the group.  px = rx + d * ux,
 *      py = ry + d * uy (one multiply, one add, no FMA); qx = px - ax, qy = py - ay.
 *  T6. Candidates (ix, iy, it), |ix|, |iy| <= window, |it| <= angle_steps.  (S, C) = (sin, cos) of it * angle_step (one
 *      multiply) from the HOST's libm, uploaded (as relocalisation rule G2 does).  The trail turns about the anchor:
 *      ex = ax + (C * qx - S * qy), ey = ay + (S * qx + C * qy), in this association; the cell (cx, cy) by world_to_grid, with
 *      sweep-matching rule 3's treatment of quotients that are not finite or beyond 2^30.  The translation shifts the look-up:
 *      score = sum over the H points of L[cy + iy][cx + ix], L sweep-matching rule 1 with `radius`.
 *  T7. Order and gate: sweep-matching rules 4 and 5 unchanged, with this H; score0 is the score of (0, 0, 0).  On acceptance
 *      dx = ix * res, dy = iy * res, dyaw = it * angle_step; otherwise all three are zero.  What the correction means: a pose
 *      (x, y, yaw) of that bot in the frame of T3 moves to
 *        (ax + (C (x - ax) - S (y - ay)) + dx,  ay + (S (x - ax) + C (y - ay)) + dy,  yaw + dyaw),  (S, C) of dyaw.
 *  T8. Limits: those of qs_match_params; travel finite and >= 0; ceil((max_dist + travel) / res) + window + radius + 2 <=
 *      QS_MATCH_MAX_REACH, so that the patch about the anchor stays within 255 cells a side; stride >= 41.  QS_E_INVAL beyond
 *      any of them, and the text names the quantity.  A sharded context refuses, as qs_match_sweeps does.  params NULL = the
 *      sweep-matching defaults.
 * The calls read the map (waiting exact-trig rays are flushed first) and write nothing to the context: a checkpoint taken
 * before equals one taken after. */
#define QS_TRAIL_MAX_RECORDS 64     /* 256 points score at most 256 * 8 = 2048 */
typedef struct qs_trail_match {      /* 80 bytes */
    int32_t ix, iy, it, score, score0, hits;
    int32_t records, anchor;         /* anchor: index within the group, -1 when records == 0 */
    uint8_t agent, accepted_match, pad[6];   /* pad is zero */
    double ax, ay, dx, dy, dyaw;
} qs_trail_match;
int qs_match_trails(qs_ctx *ctx, const qs_match_params *params, const uint8_t *pkts, size_t n, size_t stride,
                    const uint16_t *lens, const int32_t *gsize, size_t n_groups, double travel, qs_trail_match *out,
                    double *rot_out /* n x 2, optional */);
/* same with device-resident pkts / lens / out / rot_out (gsize stays a host array); asynchronous on the context's stream */
int qs_match_trails_device(qs_ctx *ctx, const qs_match_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                           const uint16_t *d_lens, const int32_t *gsize, size_t n_groups, double travel,
                           qs_trail_match *d_out, double *d_rot_out);

/* ---- trail relocalisation (no reference counterpart: this build's own rule) ------------------------------------------------
 * Trail matching corrects a packet bot inside a small window; it cannot FIND one.  A bot that reboots, is carried, or joins a
 * map another bot drew reports poses in a frame of its own.  Its trail -- T1-T5's -- is located over the whole map as a group
 * of sweeps is (G4-G8 / J5): every FREE cell of the search box is a candidate cell of the anchor, every rotation step a
 * candidate turn of the packet fields' frame.  Apart from one device sincos per record, which the call reports, everything is
 * integer or uncontracted fp64: fed those values the CPU restatement (tests/trail_reloc_rules.py) agrees bit for bit.
 *  K1. Groups: as T1, gsize[g] in 1..QS_TRAIL_MAX_RECORDS, summing to n; a HOST array in both entry points, refused before
 *      anything is enqueued.
 *  K2. Acceptance and anchor: as T2 (qs_ingest's rule).  The anchor is the last accepted record, the bot the anchor's agent.
 *  K3. A record counts when it is accepted, is the bot's, and (X_k - X_a)^2 + (Y_k - Y_a)^2 <= travel^2 (uncontracted),
 *      X, Y the f32 fields widened to f64.  The bot's offset and drift are NOT read: they are common to every record of the
 *      trail and cancel in K4.  With no counting record: status QS_RELOC_NO_RECORD, anchor = -1, every other field zero.
 *  K4. Points: (s, c) = the device's sincos(f64(yaw)), one per counting record, reported in rot_out[k] (zeros for the other
 *      records).  Sensor directions are T5's sign flips; a range is a hit when min_dist < d <= max_dist (the context's trust
 *      filter).  qx = (X_k - X_a) + d * ux, qy likewise: one subtract, one multiply, one add, no FMA.  H = the hits of the trail.
 *  K5. Rotations: under rotation j the offsets are J5's, applied to (qx, qy), with M = ceil((max_dist + travel) / res) + 1.  A
 *      point beyond M on an axis, or one that is not a number, scores 0 under that rotation.
 *  K6. Candidates, order, rival and gate: G4-G7 with this H.  qs_reloc_params is unchanged; NULL gives its defaults.
 *  K7. Result: the anchor stands at the centre of cell (gx, gy) and the frame of the packet fields is turned by th_j.  x, y
 *      are that cell centre, yaw is G8's, ax = X_a, ay = Y_a.  A pose (px, py, pyaw) in the packet fields' frame moves to
 *        (x + (C (px - ax) - S (py - ay)),  y + (S (px - ax) + C (py - ay)),  pyaw + yaw),  (S, C) of yaw.
 *      Statuses as J7; QS_RELOC_NO_CANDIDATE still reports records, hits, anchor, agent, ax and ay.
 *  K8. Limits: those of qs_reloc_params; travel finite and >= 0; 16 + 2 * (ceil((max_dist + travel) / res) + radius + 1) <=
 *      255; stride >= 41.  A sharded context refuses, as qs_match_trails does.  QS_E_INVAL beyond any of them, and the text
 *      names the quantity.
 * The calls read the map (waiting exact-trig rays are flushed first) and write nothing to the context: a checkpoint taken
 * before equals one taken after. */
typedef struct qs_trail_reloc {          /* 88 bytes; offsets 0..41 and 48..71 are qs_group_reloc's */
    int32_t gx, gy, j, score, hits;
    int32_t gx2, gy2, j2, score2;
    int32_t status;
    uint8_t records, accepted, agent, pad;   /* pad is zero */
    int32_t anchor;                          /* index within the group, -1 when records == 0 */
    double x, y, yaw, ax, ay;
} qs_trail_reloc;
int qs_relocalise_trails(qs_ctx *ctx, const qs_reloc_params *params, const uint8_t *pkts, size_t n, size_t stride,
                         const uint16_t *lens, const int32_t *gsize, size_t n_groups, double travel, qs_trail_reloc *out,
                         double *rot_out /* n x 2, optional */);
/* same with device-resident pkts / lens / out / rot_out (gsize stays a host array); asynchronous on the context's stream, with
 * the exceptions of qs_relocalise_sweeps_device */
int qs_relocalise_trails_device(qs_ctx *ctx, const qs_reloc_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                const uint16_t *d_lens, const int32_t *gsize, size_t n_groups, double travel,
                                qs_trail_reloc *d_out, double *d_rot_out);

/* ---- OccupancyGrid object API ----------------------------------------------------------
 * batched OccupancyGrid.update_ray(robot_x, robot_y, hit_x, hit_y, hit_valid)  :136-156 */
int qs_update_rays(qs_ctx *ctx, const double *rx, const double *ry, const double *hx,
                   const double *hy, const uint8_t *valid, size_t n, uint64_t seq0);
/* OccupancyGrid.world_to_grid  :121-125 (device evaluation of the same fp64 expression) */
int qs_world_to_grid(qs_ctx *ctx, const double *w, size_t n, int32_t axis, int64_t *out);
/* OccupancyGrid.grid: int8 [size][size], row = gy, values -1/0/100  :92-94, :119 */
int qs_grid_i8(qs_ctx *ctx, int8_t *out_host);
int qs_grid_i8_device(qs_ctx *ctx, int8_t *out_dev);
/* build extension: per-cell counts of OCCUPIED / FREE writes, and a log-odds view
 * clamp(hits*l_occ - misses*l_free, lmin, lmax) */
int qs_grid_counts(qs_ctx *ctx, int32_t *hits_host, int32_t *misses_host);
int qs_grid_logodds(qs_ctx *ctx, float l_occ, float l_free, float lmin, float lmax,
                    float *out_host);
/* raw device state, for collectives (RCCL all-reduce MAX on int32 stamps, SUM on counts) */
int qs_device_buffers(qs_ctx *ctx, void **stamps_dev, size_t *stamps_bytes,
                      void **counts_dev, size_t *counts_bytes);

/* ---- PoseGraphSLAM state  dual_bot_mapper.py:261-338 ---------------------------------- */
int qs_slam_sizes(qs_ctx *ctx, int32_t graph, int64_t *n_nodes, int64_t *n_landmarks,
                  int64_t *n_closures);
/* slam.closures: (lm_idx, node_idx), (corr_dx, corr_dy)  :270, :317 */
int qs_slam_closures(qs_ctx *ctx, int32_t graph, int64_t *idx2, double *corr2, size_t cap);
/* nodes[node_idx].agent_id of every closure's closing node (get_correction_for_agent, :328-338) */
int qs_slam_closure_agents(qs_ctx *ctx, int32_t graph, uint8_t *agents, size_t cap);
/* slam.landmarks: (x, y), (type, node_idx) in insertion order  :269, :288 */
int qs_slam_landmarks(qs_ctx *ctx, int32_t graph, double *xy, int64_t *type_idx, size_t cap);
/* PoseGraphSLAM.add_pose(x, y, yaw, agent_id, landmark_type, timestamp) -> (closure_detected,
 * correction_dx, correction_dy), batched  :273-290.  Object API: the poses are used AS GIVEN -- the
 * caller has already applied its drift correction, as main() does (:855-857) before it calls
 * add_pose (:908).  No rays are cast.  closed / corr2 (n x 2) may be NULL. */
int qs_slam_add_poses(qs_ctx *ctx, const double *x, const double *y, const uint8_t *agent,
                      const uint8_t *landmark, size_t n, uint8_t *closed, double *corr2);
/* drift_correction[bot]  :782, :910-914 */
int qs_drift(qs_ctx *ctx, int32_t bot, double out[2]);

/* ---- ZONE output  dual_bot_mapper.py:675-688, :702-706, :922-945 ----------------------- */
/* bbox over bot's valid hit points U path; *valid = 0 when the bot has no points yet */
int qs_zone(qs_ctx *ctx, int32_t bot, double out[4], int32_t *valid);
/* the 20-byte datagram sent to the OTHER bot; online == 0 lifts the zone (999,999,-999,-999) */
int qs_zone_packet(qs_ctx *ctx, int32_t bot, int32_t online, uint8_t out[QS_ZONE_SIZE]);

/* ---- grid merge ------------------------------------------------------------------------
 * shared-grid semantics of dual_bot_mapper.py:785: dst <- fuse(dst, srcs...) cell-wise
 * (latest stamp wins, counts add).  All contexts on dst's GPU, same geometry. */
int qs_fuse(qs_ctx *dst, qs_ctx *const *srcs, size_t n);
/* same over raw device buffers (e.g. peers' grids gathered by the caller) */
int qs_fuse_buffers(qs_ctx *dst, const void *const *stamps_dev, const void *const *counts_dev,
                    size_t n);
/* fuse of a RANGE of cells: dst cells [cell_offset, cell_offset + n_cells) <- fuse(dst, sources), every source pointer
 * naming the source's first cell of that range (the receive buffers of a reduce-scatter: each rank folds its peers'
 * copies of ITS slice, then the slices are all-gathered).  Either pointer array may be NULL (stamps only / counters
 * only).  counts_into_fused != 0 adds into the snapshot of qs_fused_counts instead of the local counters. */
int qs_fuse_buffers_range(qs_ctx *dst, const void *const *stamps_dev, const void *const *counts_dev,
                          size_t n, size_t cell_offset, size_t n_cells, int32_t counts_into_fused);
/* ---- sharded streams (one context per GPU, the shared grid of dual_bot_mapper.py:785 kept in N pieces) -------------
 * The local counters hold this context's own writes only and are never the target of a collective: qs_fused_counts
 * copies them into a second buffer (on the context's stream) and returns it; the caller sums THAT over the ranks, as
 * often as it likes.  qs_counts_source(ctx, 1) makes qs_grid_counts / qs_grid_logodds read the fused snapshot, until
 * qs_counts_source(ctx, 0), qs_reset or qs_dirty_tracking(ctx, 0). */
int qs_fused_counts(qs_ctx *ctx, void **fused_dev, size_t *bytes);
int qs_counts_source(qs_ctx *ctx, int32_t fused);
/* Stamp epochs: ordinals are 30 bits, so a batch that would pass 2^28 arrival indices first rebases the grid (every
 * written cell -> ordinal 1).  With seq_stride > 1 the shards must have exchanged their stamps (MAX all-reduce) since
 * their last write before that happens, or two ranks' writes to one cell would tie: qs_epoch_query tells whether the
 * next ingest (same seq0 / n) would rebase -- the answer is the same on every rank --, qs_mark_fused records that the
 * exchange has happened; an ingest that needs a rebase with unfused writes fails with QS_E_STATE. */
int qs_epoch_query(qs_ctx *ctx, uint64_t seq0, size_t n, int32_t *would_rebase);
int qs_mark_fused(qs_ctx *ctx);
/* ---- sparse fuse: only the blocks a shard has written since its last fuse travel -------------------------------------
 * The shared grid of dual_bot_mapper.py:785 kept in N pieces, fused without moving the whole map: a shard by agent writes
 * a few rooms, not the world.  With tracking on, every writer of the grid (tiled raster merge, direct rays, edge rays,
 * qs_update_rays, qs_fuse*) sets one bit per QS_DIRTY_BLOCK_H x QS_DIRTY_BLOCK_W block of cells it touches.  A fuse is
 *   qs_sparse_fuse_begin   own bitmap -> slot `rank` of a [world][bitmap_bytes] device array (live bitmap cleared);
 *                          the caller all-gathers that array over the ranks (RCCL; the slots are equal-sized);
 *   qs_sparse_fuse_plan    block lists of every rank (ascending block index), this rank's blocks packed -- 64 stamps and,
 *                          with counters, 64 counter DELTAS since this rank's previous sparse fuse -- at offsets[rank] of
 *                          one payload buffer; n_blocks / offsets (bytes, world + 1 entries) tell the caller what to send
 *                          (its own segment, to every peer) and where to receive (peer p's segment at offsets[p]);
 *   qs_sparse_fuse_apply   every received block folded in: stamps MAX into the grid, deltas ADDED to the fused counters
 *                          (which qs_grid_counts / qs_grid_logodds then read); qs_mark_fused implied.
 * Result = the dense fuse (MAX all-reduce of the stamps, SUM of the counters) bit for bit, as long as every rank's grid
 * was equal after the previous fuse (true from qs_reset on).  In this mode the fused counters accumulate deltas: do not
 * mix with qs_fused_counts (refused while tracking is on).  world <= QS_SPARSE_MAX_WORLD.
 * Only apply commits: a fuse that NO rank applied (the exchange failed after begin or plan) is carried in full by the next
 * qs_sparse_fuse_begin, which puts the blocks it had taken back into the live bitmap; the counter deltas are still there.
 * A fuse that some ranks applied and others did not cannot be repaired -- sending it again would add the appliers' deltas
 * twice --: the ranks must qs_reset.  qs_dirty_tracking(ctx, 0) returns the counts view to the local counters;
 * qs_dirty_tracking(ctx, 1) is refused while the grid has writes no fuse has carried (enable it after qs_create /
 * qs_reset / a fuse). */
#define QS_DIRTY_BLOCK_W 16
#define QS_DIRTY_BLOCK_H 4
#define QS_SPARSE_MAX_WORLD 64
int qs_dirty_tracking(qs_ctx *ctx, int32_t enable);
/* diagnostic: number of blocks marked since the last sparse fuse (waits for the stream) */
int qs_dirty_blocks(qs_ctx *ctx, size_t *n_blocks, size_t *block_cells);
int qs_sparse_fuse_begin(qs_ctx *ctx, int32_t world, int32_t rank, void **bitmaps_dev, size_t *bitmap_bytes);
int qs_sparse_fuse_plan(qs_ctx *ctx, uint32_t *n_blocks /* [world] */, size_t *offsets /* [world + 1] */,
                        void **payload_dev, size_t *block_bytes);
int qs_sparse_fuse_apply(qs_ctx *ctx);
/* The same fuse with its two exchanges on RCCL, for hosts that are not torch (dist.py drives the three steps above through
 * torch.distributed): one process per GPU, one communicator over the node's xGMI links.  qs_rccl_unique_id on rank 0, the 128
 * bytes to every rank by whatever channel the host has, qs_rccl_comm_init on every rank, then qs_sparse_fuse_rccl as often as the
 * map is to be fused: ncclAllGather of the bitmaps, one group of ncclSend / ncclRecv for the packed blocks (point to point, all
 * links at once), the fold.  stats (may be NULL): {blocks packed, bytes packed, bytes sent, bytes received} of this rank.
 * RCCL is loaded on demand (dlopen): QS_E_NODEV if it is absent.  Untested beyond one rank: the build has one GPU. */
#define QS_RCCL_ID_BYTES 128
int qs_rccl_unique_id(uint8_t out[QS_RCCL_ID_BYTES]);
int qs_rccl_comm_init(qs_ctx *ctx, const uint8_t id[QS_RCCL_ID_BYTES], int32_t world, int32_t rank, void **comm);
int qs_rccl_comm_destroy(void *comm);
int qs_sparse_fuse_rccl(qs_ctx *ctx, void *comm, int32_t world, int32_t rank, uint64_t stats[4]);
/* the fused counters as they stand (no snapshot is taken): the sum over the ranks after a fuse; NULL before the first one */
int qs_fused_counts_buffer(qs_ctx *ctx, void **fused_dev, size_t *bytes);
/* MapMerger.grid_to_pcd  server_nodes/map_merger.py:64-85: cells > 50 -> (col*res+ox,
 * row*res+oy) in row-major order.  grid: host int8 [h][w]; returns the count in *n_out. */
int qs_grid_to_pcd(qs_ctx *ctx, const int8_t *grid, int32_t h, int32_t w, double res,
                   double ox, double oy, double *xy, size_t cap, size_t *n_out);
/* MapMerger.publish_global_map  map_merger.py:87-127: points -> int8 canvas; call with
 * grid == NULL to obtain dims {h,w} and origin {min_x,min_y} first */
int qs_rasterise(qs_ctx *ctx, const double *xy, size_t n, double res, int32_t dims[2],
                 double origin[2], int8_t *grid);

/* ---- ICP registration and voxel down-sampling: MapMerger.map_callback, map_merger.py:45-60 ------
 * registration_icp(source, target, max_dist, identity, PointToPoint, max_iteration) on planar
 * clouds (Open3D semantics; parity unpinned: Open3D is not available).  T = 3x3 row-major planar
 * rigid transform source -> target; fitness = #correspondences / n_src; rmse over correspondences;
 * stops early when |d fitness| < rel_fitness and |d rmse| < rel_rmse (Open3D defaults: 1e-6).
 * Every update is the planar Kabsch step on the demeaned correspondences a' (sources), b' (targets):
 * theta = atan2(sum a' x b', sum a' . b'), translation = mean b - R mean a.  Degenerate rule: when
 * sum |a'|^2 <= 2^-80 n |mean a|^2 or sum |b'|^2 <= 2^-80 n |mean b|^2 (n correspondences; a sum of exactly 0 always
 * qualifies) all matched sources, or all matched targets, are one point up to the rounding of their mean, both sums are
 * rounding noise, and the update's rotation is the identity, theta = 0 (Umeyama on a zero covariance: U = V = I); the
 * translation stays mean b - mean a.  Genuine clouds sit far above the threshold (a room 1.0e4 m from the origin: 3.5e-8;
 * 2^-80 = 8.3e-25; degenerate ones: <= 6e-30).  With max_iter = 0: T = identity, fitness and rmse of the inputs. */
int qs_icp(qs_ctx *ctx, const double *src_xy, size_t n_src, const double *dst_xy, size_t n_dst,
           double max_dist, int32_t max_iter, double rel_fitness, double rel_rmse, double T[9],
           double *fitness, double *rmse, int32_t *iters);
/* The correspondence search of registration_icp on its own (build extension; map_merger.py:48-52 reaches it through
 * Open3D): corr[i] = nearest target of source i if closer than max_dist else -1 (ties: lowest index), d2[i] = its squared
 * distance.  mode 0 = auto, 1 = scalar fp64 brute force, 2 = distance matrix on the matrix cores
 * (v_mfma_f64_16x16x4_f64 as a screen with margin, fp64 re-evaluation of what passes): same results bit for bit.
 * ms (may be NULL): HIP-event milliseconds of {the search kernel, the operand preparation}. */
int qs_nn_search(qs_ctx *ctx, const double *src_xy, size_t n_src, const double *dst_xy, size_t n_dst,
                 double max_dist, int32_t mode, int32_t *corr, double *d2, float ms[2]);
/* Loop-closure chain (PoseGraphSLAM.check_loop_closure, dual_bot_mapper.py:292-326): which device form runs -- same closures,
 * landmarks and drifts whichever.  QS_CHAIN_AUTO (default; the environment's QS_CHAIN_MODE=free|free_posting|window at qs_create
 * overrides): the free-running form; for graphs of up to 13 bots without the owner waves posting their landmarks' poses for each
 * other (QS_CHAIN_FREE) as long as its decisions rarely find nothing in the index, with it (QS_CHAIN_FREE_POSTING) for streams
 * whose queries mostly find nothing -- decided from counts the kernels leave: every ingest has them copied to pinned memory behind
 * itself and the next ingest looks at whatever has arrived, nobody waits; kept over qs_reset: it describes the stream, not the
 * session.  QS_CHAIN_WINDOW: the per-window kernel (one barrier per window of MIN_POSES_BETWEEN nodes): the second opinion of the
 * tests, and QS_CHAIN_AUTO's last resort for a stream that hardly ever matches (more scans of posted poses than closures).
 * qs_chain_form: the form the last ingest used. */
#define QS_CHAIN_AUTO 0
#define QS_CHAIN_FREE 1
#define QS_CHAIN_WINDOW 2
#define QS_CHAIN_FREE_POSTING 3
int qs_set_chain_form(qs_ctx *ctx, int form);
int qs_chain_form(qs_ctx *ctx);
/* The owner waves of the free-running form for graphs of up to 13 bots have a lean variant: 32-bit node indices, and a decision
 * settled by the first node of each of its nine buckets where those already hold the match (buckets that have to be walked
 * further are walked on the same 32-bit terms); every other decision goes through the general query.  It exists in the
 * instantiations without posted poses (not the 8-wave one of a graph with a landmark pile); the others run the general owner.
 * Same closures, landmarks and drifts bit for bit.  Every
 * launch decides on the device, per graph, whether it applies: the graph's node count after the launch below `limit`, the node
 * table below 4 GiB, MIN_POSES_BETWEEN below 2^30, poses that get their drift (not qs_slam_add_poses).
 * mode QS_CHAIN_LEAN_AUTO (default) or QS_CHAIN_LEAN_OFF (the general owner always); limit: node count at which the lean owner
 * stops, <= 0 or above 0x7f7f7f7f: 0x7f7f7f7f (the low word of the empty-slot marker of the index).
 * qs_chain_lean: 1 if every graph of the last ingest ran the lean owner, else 0 (waits for the stream); < 0: error.
 * The counter slam_node_iters counts the lean owner's decisions that were not settled by those first nodes alone. */
#define QS_CHAIN_LEAN_AUTO 0
#define QS_CHAIN_LEAN_OFF 1
int qs_set_chain_lean(qs_ctx *ctx, int32_t mode, int64_t limit);
int qs_chain_lean(qs_ctx *ctx);

/* The lean owner finds its agent's next event in a plan: every agent's own events in list order, each with the agent's first
 * later event past the cool-down of a closure there, built by parallel kernels ahead of every launch that has the lean owner on
 * offer.  qs_set_chain_plan: on != 0 (default) builds and walks it, 0 has the lean owner stream the graph's whole event list in
 * chunks of 64 as the general owner does.  Same closures, landmarks and drifts bit for bit.
 * qs_chain_plan: 1 if the last ingest had a plan and every graph ran the lean owner, which then walked it, else 0 (waits for
 * the stream); < 0: error. */
int qs_set_chain_plan(qs_ctx *ctx, int32_t on);
int qs_chain_plan(qs_ctx *ctx);
/* diagnostic: bot's part of the plan of the last ingest, valid until the next one (waits for the stream).  n_own: the number of
 * its events in that launch; first: the own index of its first event past the cool-down it came with (none: n_own); for each
 * of them, in list order, node (the node index's low word), r (the position in its graph's event list) and skip (the own
 * index of its first later event past the cool-down of a closure there; none: n_own).  node, r, skip: arrays of cap >= n_own
 * entries, or all three NULL to ask for n_own and first alone.  QS_E_STATE if the last ingest had no plan, QS_E_RANGE if cap is
 * too small (n_own and first are set even so). */
int qs_chain_plan_read(qs_ctx *ctx, int32_t bot, int32_t *node, uint32_t *r, uint32_t *skip, size_t cap, size_t *n_own,
                       uint32_t *first);

/* Every node of a bucket chain carries, beside its seven entries, the node index of its successor node's first entry (the
 * look-ahead word; written always).  The lean owner walks a bucket on only if that index lies below the match it has: entries
 * are in insertion order, so a successor chain that starts at or above the match cannot hold an older one.
 * qs_set_chain_lookahead: on != 0 (default) tests the look-ahead word, 0 the node's own last entry, as the general query does --
 * the same instructions on another word of the node, chosen per launch.  Same closures, landmarks and drifts bit for bit; with
 * it on, fewer decisions walk (slam_node_iters).  qs_chain_lookahead: the setting, 1 or 0; < 0: error. */
int qs_set_chain_lookahead(qs_ctx *ctx, int32_t on);
int qs_chain_lookahead(qs_ctx *ctx);

/* In a graph of up to two agents the 8-wave free-running kernel has waves to spare.  One of them per owner, its scout, reads
 * ahead of the owner: after every decision it takes the candidate the plan gives after the owner's next one, the pose that
 * candidate will be queried at but for one closure's correction, and stages the first nodes of a 4 x 4 window of buckets around
 * it in LDS.  The owner settles a decision from its stage when the stage is for its candidate, holds the 3 x 3 buckets of the
 * real pose and shows a match with no bucket to walk further; any other decision it makes from its own loads, as without scouts.
 * Same closures, landmarks and drifts bit for bit.
 * qs_set_chain_scout: on != 0 runs the scouts wherever a launch has a plan, 0 (default) never; the environment's QS_CHAIN_SCOUT=1
 * at qs_create turns them on for that context.  Off by default because it measured slower: the owner's path through a stage is
 * longer in instructions than the round trip of the loads it saves (profiles/chain_scout/).
 * qs_chain_scout: of the last ingest, the owners' decisions settled from a stage and those made from their own loads (both 0
 * if that launch had no scouts: another instantiation, no plan, more than two agents a graph); waits for the stream. */
int qs_set_chain_scout(qs_ctx *ctx, int32_t on);
int qs_chain_scout(qs_ctx *ctx, uint64_t *staged, uint64_t *fallback);

/* diagnostic: measured dense fp64 MFMA rate of this GPU (TFLOP/s), the ceiling qs_nn_search mode 2 is priced against */
int qs_diag_mfma_f64_rate(qs_ctx *ctx, double *tflops);
/* diagnostic: latencies of the primitives one loop-closure decision chains together, measured on this GPU by ONE workgroup
 * (as the loop-closure chain kernels run), in shader-clock cycles:
 *   out[0] dependent global load, L2 hit     out[1] dependent global load, L1 hit     out[2] dependent LDS read
 *   out[3] dependent v_fma_f64               out[4] dependent DPP / VALU step          out[5] v_readlane -> VALU step
 *   out[6] workgroup barrier + LDS fences, 16 waves      out[7] same, 5 waves          out[8] shader clock in MHz */
#define QS_DIAG_LAT_N 9
int qs_diag_latencies(qs_ctx *ctx, double out[QS_DIAG_LAT_N]);
/* PointCloud.voxel_down_sample(voxel): mean of the points of each voxel, ascending voxel order
 * (Open3D's order is unspecified).  out_xy == NULL queries the count. */
int qs_voxel_downsample(qs_ctx *ctx, const double *xy, size_t n, double voxel, double *out_xy,
                        size_t cap, size_t *n_out);

/* The same down-sampling over a cloud that is already on the device, with the grouping there too: d_xy (n points, x y pairs)
 * and d_out_xy (room for cap points; may be NULL to query the count) are device pointers on the context's GPU and must not
 * overlap.  Returns exactly what qs_voxel_downsample returns for the same points: one point per voxel in ascending key
 * order, key (vy << 32) | vx, each mean the fp64 sum of the voxel's points taken one after the other IN INPUT ORDER, divided
 * by their number.  Keys are grouped by a stable least-significant-digit radix sort of (key, input index), 8 bits per pass,
 * over the bytes the cloud's bounding box says are in use (a room-sized cloud: 2 to 4 passes).  The input must be finite.
 * The caller's own work on the two arrays must be complete before the call; the result is complete when it returns.
 * cap < *n_out writes the first cap points. */
int qs_voxel_downsample_device(qs_ctx *ctx, const double *d_xy, size_t n, double voxel, double *d_out_xy,
                               size_t cap, size_t *n_out);

/* ---- map merge session: the MapMerger node, server_nodes/map_merger.py:28-127, with its state on the device ----------------
 * The context keeps the node's state: the global cloud (global_pcd, :31), map_resolution and map_origin (:32-33) and the ICP
 * parameters (:46-54; defaults: threshold 1.0, 30 iterations, min fitness 0.6).  One qs_merge_grid / _grid_device / _map call is
 * one map_callback (:35-62), step for step; every step runs the kernels of the entry point named beside it, so each can be
 * checked against that entry point bit for bit:
 *   1. local cloud: the cells with grid > 50 in row-major order, x = col*res + ox, y = row*res + oy [qs_grid_to_pcd].
 *      qs_merge_map reads src's own map instead, straight from its stamps (occupied = an odd stamp; geometry = src's
 *      configuration; no int8 view is built): the cloud qs_merge_grid makes of src's qs_grid_i8.  src must be on ctx's GPU
 *      (QS_E_INVAL otherwise) and may be ctx itself; its waiting edge rays are resolved first, as in every call that observes
 *      the map.  No point: QS_MERGE_EMPTY, nothing changes.
 *   2. empty global cloud: the local cloud, res and the origin are adopted: QS_MERGE_ADOPTED.
 *   3. otherwise the local cloud is registered against the global cloud [the loop of qs_icp, identity start, the session's
 *      threshold and iterations, rel_fitness = rel_rmse = 1e-6]: T, fitness, rmse, iterations are those of
 *      qs_icp(local, global).
 *   4. fitness < min_fitness: QS_MERGE_REJECTED, the global cloud is unchanged.
 *   5. the accumulated T is applied to the ORIGINAL local points (not the copy the loop moved step by step),
 *      x' = (T[0]*x + T[1]*y) + T[2], y' = (T[3]*x + T[4]*y) + T[5], products and sums rounded one by one; they are appended
 *      behind the global cloud and the whole is down-sampled at map_resolution [qs_voxel_downsample_device]: QS_MERGE_MERGED.
 *   6. qs_merge_global_map is publish_global_map (:87-127) [qs_rasterise over the resident cloud, the same QS_E_RANGE rule];
 *      dims {0, 0} while the cloud is empty.
 * No cloud crosses to the host inside a callback: the host reads scalars only (the local count, the global cloud's box, the
 * six sums of every ICP iteration, the final count).  qs_merge_grid uploads the message's grid, qs_merge_grid_device and
 * qs_merge_map upload nothing.  d_grid is a device pointer on the context's GPU whose contents are complete before the call.
 * qs_reset does not touch the session (the merger is a node of its own in the reference): qs_merge_reset empties it
 * (parameters stay).  Checkpoints do not hold the session.  out (may be NULL) reports the callback.
 * qs_merge_params: icp_threshold > 0, icp_iterations >= 0, min_fitness not NaN, else QS_E_INVAL.
 * qs_merge_cloud: *n_out = points of the global cloud; the first cap of them to xy (host, may be NULL). */
enum { QS_MERGE_EMPTY = 0, QS_MERGE_ADOPTED = 1, QS_MERGE_MERGED = 2, QS_MERGE_REJECTED = 3 };
typedef struct qs_merge_result {
    int32_t status, iterations;
    uint64_t n_local, n_global;      /* points of this map; points of the global cloud after the call */
    double fitness, rmse, T[9];      /* as qs_icp reports them; identity / 0 when no registration ran */
} qs_merge_result;
int qs_merge_reset(qs_ctx *ctx);
int qs_merge_params(qs_ctx *ctx, double icp_threshold, int32_t icp_iterations, double min_fitness);
int qs_merge_grid(qs_ctx *ctx, const int8_t *grid, int32_t h, int32_t w, double res, double ox, double oy,
                  qs_merge_result *out);
int qs_merge_grid_device(qs_ctx *ctx, const int8_t *d_grid, int32_t h, int32_t w, double res, double ox, double oy,
                         qs_merge_result *out);
int qs_merge_map(qs_ctx *ctx, qs_ctx *src, qs_merge_result *out);
int qs_merge_cloud(qs_ctx *ctx, double *xy, size_t cap, size_t *n_out);
int qs_merge_global_map(qs_ctx *ctx, int32_t dims[2], double origin[2], int8_t *grid);

/* ---- frontiers  dual_bot_mapper.py:181-237, :948-956 -------------------------------------------
 * OccupancyGrid.get_frontiers: interior FREE cells with a 4-neighbour UNKNOWN, row-major order
 * (gx, gy pairs).  xy == NULL queries the count. */
int qs_frontier_cells(qs_ctx *ctx, int32_t *xy, size_t cap, size_t *n_out);
/* cluster_frontiers + the sums cluster_centroid_world divides: 4-connected clusters of at least
 * min_cluster cells (reference: FRONTIER_MIN_CLUSTER = 3, :102) in the reference's order (by
 * first cell, row-major); 5 values per cluster: size, first_gx, first_gy, sum_gx, sum_gy.
 * stats5 == NULL queries the count. */
int qs_frontier_clusters(qs_ctx *ctx, int32_t min_cluster, int64_t *stats5, size_t cap, size_t *n_out);

/* cluster membership: every frontier cell (row-major order) with the linear index (gy*size + gx) of the first cell of
 * its 4-connected cluster; 3 values per cell: gx, gy, root.  xy_root == NULL queries the count. */
int qs_frontier_members(qs_ctx *ctx, int32_t *xy_root, size_t cap, size_t *n_out);

/* frontier target assignment: dual_bot_mapper.py:947-996 (commented out in the reference),
 * consumed by AgentFirmware_Bot1.ino:81-137.  bot_xy: n_bots positions in greedy order.
 * target_idx[b] = index into the min_cluster-filtered cluster list (qs_frontier_clusters order) or -1;
 * target_xy[b] = its centroid (untouched when -1).  centroids_xy (optional, cap entries) and
 * *n_centroids report the centroid list.  stats (optional): n_centroids, K, fallback scans, reserved.
 * Each bot in turn takes the centroid nearest to it (sqrt of dx*dx + dy*dy, fp64; ties to the lower index) among
 * those no earlier bot took and none of whose distances to an earlier target is below `separation`; a bot whose
 * position is NaN or infinite gets -1.  n_bots <= QS_FT_MAX_BOTS; n_bots == 0 and a map without clusters are valid.
 * Observes the map (flushes waiting exact-trig rays first).  Bad arguments: QS_E_INVAL. */
#define QS_FT_MAX_BOTS 1024
int qs_frontier_targets(qs_ctx *ctx, int32_t min_cluster, double separation,
                        const double *bot_xy, size_t n_bots, int64_t *target_idx, double *target_xy,
                        double *centroids_xy, size_t cap, size_t *n_centroids, uint64_t stats[4]);

/* ---- path planning over the mapped free space (no reference counterpart: this build's own rules) ----------------------
 * A path from a bot to its frontier target over the cells the map knows to be free, and the waypoint a bot can drive to
 * in a straight line (what a TARG packet carries when MissionControl plans).  All rules are integer, so the device and a
 * CPU restatement agree bit for bit.
 *  1. Traversable: a FREE cell (stamp nonzero and even; OCCUPIED = odd, UNKNOWN = 0, frontier.hip's reading) with no
 *     OCCUPIED cell within `clearance` cells: dx*dx + dy*dy <= clearance*clearance.  UNKNOWN is never traversable;
 *     clearance 0 = FREE cells only.  clearance <= QS_PLAN_MAX_CLEARANCE.
 *  2. Snapping: a position maps to a cell by world_to_grid (int((w - o) / res), :121-125).  If that cell is not
 *     traversable, it snaps to the traversable cell minimising (dx*dx + dy*dy, gy*size + gx) within snap_radius cells
 *     (dx*dx + dy*dy <= snap_radius^2).  None, or a NaN / infinite / off-grid position: QS_PLAN_NO_START / _NO_GOAL.
 *  3. Field: exact shortest-path cost to the goal cell over traversable cells; 8-connected moves, an orthogonal step
 *     costs QS_PLAN_ORTHO and a diagonal QS_PLAN_DIAG, a diagonal move needs both orthogonal neighbours traversable
 *     (no corner cutting).  uint32 costs, 0xFFFFFFFF = unreached.  The fixpoint is unique: any relaxation order gives it.
 *  4. Path: from the start cell, at each cell c the first legal move (rule 3) to a neighbour n with
 *     field[n] + step(c, n) == field[c], moves tried in the order E (+x), N (+y), W, S, NE, NW, SW, SE; it ends at the
 *     goal.  Path cells are numbered from 0 (the start); path_len counts them all, both ends included.  An infinite
 *     field[start]: QS_PLAN_UNREACHABLE.
 *  5. Waypoint: among path cells 1 .. min(lookahead, path_len - 1), a cell is visible when every cell of the reference's
 *     _bresenham(start, cell) (:158-179) is traversable; the waypoint is the cell just before the first that is not,
 *     else the last of them.  Start == goal: the waypoint is the start and the cost 0.  Its world position is
 *     grid_to_world (:127-131, the cell centre).
 * Defaults (build choices, not the reference's): clearance 2 cells (0.10 m at 0.05 m per cell; the bots follow walls at
 * 0.25 m), snap_radius 10, lookahead 200.  Every call observes the map (flushes waiting exact-trig rays first) and writes
 * no session state: a checkpoint before equals one after.  Bad arguments: QS_E_INVAL. */
#define QS_PLAN_OK 0
#define QS_PLAN_NO_START 1
#define QS_PLAN_NO_GOAL 2
#define QS_PLAN_UNREACHABLE 3
#define QS_PLAN_ORTHO 5
#define QS_PLAN_DIAG 7
#define QS_PLAN_MAX_CLEARANCE 16
#define QS_PLAN_MAX_SNAP 64
#define QS_PLAN_MAX_LOOKAHEAD 65536
/* Fields are computed a group of requests at a time; a group's fields (each the tile-aligned bounding box of the
 * traversable cells, 4 bytes a cell) fit this many bytes (one field over the whole grid when even that is larger). */
#define QS_PLAN_WS_CAP ((size_t)2 << 30)
typedef struct qs_plan_params { int32_t clearance, snap_radius, lookahead, reserved; } qs_plan_params;
/* rule 1 for the whole grid: mask_host[gy*size + gx] = 1 when traversable (tests and tools) */
int qs_traversable(qs_ctx *ctx, int32_t clearance, uint8_t *mask_host);
/* rule 3 for one goal (params NULL = defaults): field_host [size][size]; all 0xFFFFFFFF when the goal does not snap */
int qs_plan_field(qs_ctx *ctx, const qs_plan_params *params, const double goal_xy[2], uint32_t *field_host);
/* n requests (start_xy, goal_xy: n x 2).  Per request: status (QS_PLAN_*), the waypoint cell (gx, gy) and its world
 * position, the cost field[start]; path_xy (optional, path_cap cells of (gx, gy) per request) gets the first path_cap
 * cells and path_len (optional) the full length.  Requests that are not QS_PLAN_OK get (-1, -1), NaN, 0xFFFFFFFF, 0.
 * stats (optional): relaxation rounds, tile visits, request groups, snapped endpoints.  n == 0 and a map without FREE
 * cells are valid. */
int qs_plan_paths(qs_ctx *ctx, const qs_plan_params *params, const double *start_xy, const double *goal_xy, size_t n,
                  int32_t *status, int32_t *wp_cell_xy, double *wp_xy, uint32_t *cost, int32_t *path_xy, size_t path_cap,
                  int64_t *path_len, uint64_t stats[4]);

/* ---- frontier targets by path cost (no reference counterpart: this build's own rules) ------------------------------------
 * qs_frontier_targets gives a bot the centroid nearest in a straight line, which the bot may have no path to.  This call
 * ranks the centroids by the cost of the path over the mapped free space instead and returns target and waypoint together.
 * All rules are integer once the centroids exist, so the device and a CPU restatement agree bit for bit.
 *  1. Centroids: the list, order and positions of qs_frontier_targets / qs_frontier_clusters(min_cluster).
 *  2. Cells: the traversable mask is planning rule 1 with params.clearance; every bot position and every centroid
 *     position maps to a cell by planning rule 2 (world_to_grid, then the snap within params.snap_radius).  A position that
 *     does not snap (NaN, infinite, off-grid, nothing traversable in the radius) has no cell.
 *  3. Cost: cost(b, k) is the planning rule 3 shortest-path cost between bot b's cell and centroid k's cell (moves of 5 and
 *     7, no corner cutting, uint32); 0xFFFFFFFF when either has no cell or the two are not connected.  The moves are
 *     symmetric (a move and its reverse are legal together and cost the same), so ONE field seeded at the bot's cell
 *     gives the bot's cost to every centroid.  A cost of 0 (the bot stands on the centroid's cell) is valid.
 *  4. Greedy: bots in the order given.  Centroid k is eligible for bot b when cost(b, k) is finite, no earlier bot took k,
 *     and for every earlier target t `sqrt(dx*dx + dy*dy) < separation` is false (qs_frontier_targets' fp64 test between
 *     world centroid positions).  The bot takes the eligible k with the smallest (cost, k).  A bot with no cell gets
 *     status QS_PLAN_NO_START, a bot with a cell but no eligible centroid QS_PLAN_UNREACHABLE; both get index -1, NaN
 *     positions, cost 0xFFFFFFFF, and add no target.
 *  5. Waypoint: an assigned bot gets exactly what qs_plan_paths(params, bot_xy[b], target_xy[b]) returns on the same map:
 *     status QS_PLAN_OK (both ends have cells and the cost is finite), the waypoint cell, its world position, and the
 *     cost, which equals cost(b, k).  Unassigned bots get (-1, -1) and NaN.
 *  6. The call observes the map (flushes waiting exact-trig rays first) and writes no session state: a checkpoint before
 *     equals one after.  n_bots <= QS_FT_MAX_BOTS.  Argument checks are those of qs_frontier_targets and of qs_plan_params
 *     (QS_E_INVAL).  n_bots == 0, a map without clusters and a map without FREE cells are valid.
 * wp_cell_xy and wp_xy are an optional pair (both NULL: no waypoints are computed).  centroids_xy (optional, cap entries)
 * and *n_centroids report the centroid list.  stats (optional): centroids, centroids with a cell, bots with a cell, field
 * groups (bot fields, fields recomputed for a fallback, waypoint fields), relaxation rounds, tile visits, top-K fallbacks
 * (bots whose 32 cheapest centroids were all ineligible: decided by a scan of every centroid), reserved. */
int qs_frontier_targets_by_path(qs_ctx *ctx, int32_t min_cluster, double separation, const qs_plan_params *params,
                                const double *bot_xy, size_t n_bots, int64_t *target_idx, double *target_xy,
                                uint32_t *cost, int32_t *status, int32_t *wp_cell_xy, double *wp_xy,
                                double *centroids_xy, size_t cap, size_t *n_centroids, uint64_t stats[8]);

/* ---- frontier gain: clusters ranked by the unknown area a bot would see from them (this build's own rules) -----------------
 * The three target calls rank a cluster by how far away it is.  The gain of a cluster is what a bot would learn there: the
 * UNKNOWN cells in sensor range of a cell of the cluster that no OCCUPIED cell hides.  All rules are integer, so the device and
 * a CPU restatement agree bit for bit.
 *  G1 Clusters: the list and order of qs_frontier_clusters(min_cluster).
 *  G2 Viewpoint: for a cluster of n cells with sums sx, sy let cx = sx / n and cy = sy / n by integer division.  The viewpoint
 *     is the member cell minimising ((gx-cx)^2 + (gy-cy)^2, gy*size + gx), compared as a pair.  It is a FREE interior cell.
 *  G3 Visible: a target cell t != v inside the grid with dx*dx + dy*dy <= range^2 is visible from v when no cell of the
 *     reference's _bresenham(v, t) (:158-179) other than t itself is OCCUPIED.  The walk goes from v to t (it is not
 *     reversal-symmetric).  UNKNOWN and FREE cells do not block; cells outside the grid are neither targets nor counted.
 *  G4 Gain: gain[k] is the number of visible UNKNOWN targets (stamp 0).  A frontier cell has an UNKNOWN 4-neighbour, so
 *     gain >= 1 for every range >= 1.
 *  G5 Range: 1 <= range <= QS_GAIN_MAX_RANGE cells.  The default, 24, is the 1.20 m sensor range at 0.05 m per cell.
 *  G6 Order: for bot b, centroid k1 comes before k2 when (cost1 + bias) * gain2 < (cost2 + bias) * gain1 in exact 64-bit
 *     products; ties go to the smaller cost, then the lower k.  cost is rule 3 of "frontier targets by path cost".
 *     bias <= QS_GAIN_MAX_BIAS; the default, 120, is 24 orthogonal steps (a build choice).  A bias of 0 is the pure ratio: a bot
 *     standing on a centroid's cell has cost 0 there and takes that centroid.
 *  G7 Assignment: exactly rules 1-6 of "frontier targets by path cost" with "smallest (cost, k)" replaced by "first in G6's
 *     order".  Cells, snap, eligibility (finite cost, not taken, the fp64 separation test) and statuses are unchanged; the
 *     waypoint equals qs_plan_paths(bot, centroid) with the same cost; the call writes no session state.  The target position
 *     stays the centroid: the viewpoint only scores it.
 * qs_frontier_gain: viewpoint_xy (n x 2: gx, gy) and gain for the first cap clusters; both NULL queries the count.
 * qs_frontier_targets_by_gain: every argument of qs_frontier_targets_by_path, in its order, with gain_params (NULL = the
 * defaults) after params, and target_gain (n_bots, 0 when unassigned) before stats.  stats as for _by_path; entry 7 is the sum
 * of all gains.  A range outside G5, a bias above QS_GAIN_MAX_BIAS or a nonzero reserved: QS_E_INVAL.  n_bots == 0, a map
 * without clusters and a map without FREE cells are valid. */
#define QS_GAIN_MAX_RANGE 64
#define QS_GAIN_DEFAULT_RANGE 24
#define QS_GAIN_DEFAULT_BIAS 120u
#define QS_GAIN_MAX_BIAS 0x80000000u
typedef struct qs_gain_params { int32_t range; uint32_t bias; int32_t reserved[2]; } qs_gain_params;
int qs_frontier_gain(qs_ctx *ctx, int32_t min_cluster, int32_t range, int32_t *viewpoint_xy, int32_t *gain, size_t cap,
                     size_t *n_out);
int qs_frontier_targets_by_gain(qs_ctx *ctx, int32_t min_cluster, double separation, const qs_plan_params *params,
                                const qs_gain_params *gain_params, const double *bot_xy, size_t n_bots, int64_t *target_idx,
                                double *target_xy, uint32_t *cost, int32_t *status, int32_t *wp_cell_xy, double *wp_xy,
                                double *centroids_xy, size_t cap, size_t *n_centroids, int32_t *target_gain,
                                uint64_t stats[8]);

/* ---- territories: the mapped free space partitioned among the bots by path cost (this build's own rules) ------------------
 * qs_frontier_targets_by_path pays one shortest-path field per bot and assigns greedily in bot order.  Here every bot is
 * a seed of ONE field and each cell keeps the smallest (cost, bot): who is nearest by path to every free cell and every
 * frontier, how much each bot has left, and the box of its share.  All rules are integer, so the device and a CPU
 * restatement agree bit for bit.
 *  T1 Cells: the traversable mask is planning rule 1 with params.clearance; each bot position maps to a cell by planning
 *     rule 2 (world_to_grid, then the snap within params.snap_radius).  A bot whose position does not snap has no cell,
 *     gets status QS_PLAN_NO_START and owns nothing.  Several bots may have the same cell.
 *  T2 Cost: cost(b, c) is the planning rule 3 cost between bot b's cell and cell c (moves of 5 and 7, no corner cutting,
 *     uint32).
 *  T3 Owner: for a traversable cell c reached by at least one bot, key(c) is the minimum over those bots of
 *     (cost(b, c), b), compared as a pair; owner(c) is that b and cost(c) that cost: the lowest bot index wins a tie.
 *     Every other cell has owner -1 and cost 0xFFFFFFFF.
 *  T4 Per bot: area[b] is the number of cells owned (int64); box[b] is (min gx, min gy, max gx, max gy) over them, or
 *     (-1, -1, -1, -1) when there are none.  A bot with a cell owns at least that cell unless a lower-indexed bot shares
 *     it; such a bot has status QS_PLAN_OK, area 0 and the empty box.
 *  T5 Frontier targets by territory: the centroids are the list, order and positions of qs_frontier_targets(min_cluster);
 *     each snaps by rule 2; centroid_owner[k] is owner(cell_k), or -1 without a cell, and its cost likewise.  Bot b's
 *     target is the centroid it owns with the smallest (cost, k).  A bot with a cell but no owned centroid gets
 *     QS_PLAN_UNREACHABLE, index -1, NaN positions and cost 0xFFFFFFFF.  There is NO separation rule: territories are
 *     disjoint, so no two bots share a centroid, but the targets of two neighbouring bots may be close.  The waypoint
 *     pair is optional, as in qs_frontier_targets_by_path: an assigned bot gets exactly what
 *     qs_plan_paths(params, bot_xy[b], target_xy[b]) returns on the same map, and its cost equals the target's cost in
 *     the partition (the moves are symmetric).
 *  T6 Every call observes the map (flushes waiting exact-trig rays first) and writes no session state: a checkpoint
 *     before equals one after.  n_bots <= QS_FT_MAX_BOTS.  Argument checks are those of qs_plan_params (QS_E_INVAL).
 *     n_bots == 0, a map without FREE cells and a map without clusters are valid.
 * owner_host (int16) and cost_host (uint32) are optional [size][size] arrays indexed [gy][gx]; box is n_bots x 4.
 * stats (optional): relaxation rounds, tile visits (both include the waypoint stage's), bots with a cell, owned cells in
 * total, centroids, centroids with a cell, centroids with an owner, reserved (0); qs_territories leaves the centroid
 * entries 0.  centroids_xy and centroid_owner (both optional, cap entries) and *n_centroids report the centroid list. */
int qs_territories(qs_ctx *ctx, const qs_plan_params *params, const double *bot_xy, size_t n_bots,
                   int16_t *owner_host, uint32_t *cost_host, int32_t *status, int64_t *area, int32_t *box,
                   uint64_t stats[8]);
int qs_frontier_targets_by_territory(qs_ctx *ctx, int32_t min_cluster, const qs_plan_params *params,
                                     const double *bot_xy, size_t n_bots, int64_t *target_idx, double *target_xy,
                                     uint32_t *cost, int32_t *status, int32_t *wp_cell_xy, double *wp_xy, int64_t *area,
                                     int32_t *box, double *centroids_xy, int32_t *centroid_owner, size_t cap,
                                     size_t *n_centroids, uint64_t stats[8]);

/* ---- sensing a world: the sweeps and packets a bot would send from a pose in a mapped world (this build's own rules) --------
 * The inverse of the raycast: given the context's map and n poses, what does each beam return?  Any context is a world (a
 * maze painted through qs_update_rays, a restored checkpoint, a session's map); the records that come out are what
 * qs_ingest_sweeps_device / qs_ingest_device of ANOTHER context (or of this one) take.  All rules are integer apart from the
 * far point, so the device and a CPU restatement (tests/sense_rules.py) agree bit for bit away from S4's edge band.
 *  S1 Map: a cell is OCCUPIED when its stamp is odd.  The call observes the map as qs_grid_i8_device does (waiting exact-trig
 *     edge rays are resolved first) and writes no session state: no stamps, counters, sequence numbers or dirty bits, nothing a
 *     checkpoint holds.  A checkpoint before equals one after.
 *  S2 Pose: float32 x, y, yaw per record, the pose a packet can carry.  rx = f64(x), ry = f64(y); NO bot offset and NO drift
 *     are applied: the caller passes world poses.  Start cell (x0, y0) = world_to_grid(rx), world_to_grid(ry) (:121-125).  A
 *     pose that is not finite, or whose cell is beyond +-9e15 cells (CPython's int() would raise or walk forever): every beam is
 *     a no-return.  A start cell outside the grid is legal.
 *  S3 Beams: sweeps -- beam i of 181 has a = f64(yaw) + (i - 90) * (pi / 180), exactly qs_ingest_sweeps' rule.  Packets -- four
 *     beams a = f64(yaw) + {0, pi/2, pi, -pi/2} in sensor order front, left, back, right (:61-66, :887).
 *  S4 Far point: (rx + R cos a, ry + R sin a) with R = max_range: one multiply and one add per axis, no FMA, the device's
 *     sincos.  The far cell (x1, y1) is world_to_grid of it.  exact_trig has NO effect on this call: the far point is within one
 *     ulp of libm's, and only a far point that close to a cell boundary can move (x1, y1).
 *  S5 Walk: the cells of the reference's _bresenham((x0, y0), (x1, y1)) (:158-179) in order, from the pose outward (the walk is
 *     not reversal-symmetric).  Cell 0, the bot's own, never blocks; cells outside the grid are skipped, as update_ray skips
 *     them; UNKNOWN and FREE cells do not block.  The first OCCUPIED cell (hx, hy) is the hit.
 *  S6 Range: d = res * sqrt(f64(dx*dx + dy*dy)) with dx = hx - x0, dy = hy - y0: centre to centre, no trigonometry.  Noise (S7)
 *     is added, then the result is rounded to float32.  The beam returns that value when f64(f32(d)) <= R; otherwise, and when
 *     nothing was hit, it returns no_return (default 0.0f, which both ingest rules read as a full-length free ray).
 *     hit_cell = hy * size + hx, or -1 for no return.
 *     NOTE for whoever ingests the result: a wall in the neighbouring cell returns d = res, which the default trust filters
 *     (smin = 0.1, min_dist = 0.05 at res = 0.05) read as "too close" and answer with a full-length FREE ray through the wall.
 *     A mapper fed from this call wants a lower bound below one cell: qs_set_sweep_filter(0.02, R), min_dist = 0.02.
 *  S7 Noise (off when noise_amp == 0 and dropout_q16 == 0), stateless, in uncontracted fp64, 64-bit wrapping arithmetic; k is
 *     the record's index within the call:
 *         z  = seed + 0x9E3779B97F4A7C15 * (1 + (first_record + k) * 256 + beam)
 *         z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *         u  = (z >> 40) + ((z >> 16) & 0xFFFFFF)
 *         d' = d + noise_amp * (f64(u) * 2^-24 - 1.0)            (noise_amp in metres; |d' - d| < noise_amp, triangular)
 *         dropout when (z & 0xFFFF) < dropout_q16                 (reports no_return and hit_cell -1)
 *     Beams with no hit draw nothing.  first_record makes one call of n records equal two calls of n / 2.
 *  S8 Limits: 0 < R finite and ceil(R / res) + 1 <= QS_SENSE_MAX_CELLS; noise_amp >= 0 finite; dropout_q16 <= 65536; stride
 *     743 or 751 for sweeps (42 for packets is implied); beams 181 or 4; reserved zero.  Anything else: QS_E_INVAL.  n == 0 is
 *     valid; any n is accepted (host calls are chunked internally).
 * qs_sense_ranges: ranges (n x beams float32) and, optionally, hit_cell (n x beams int32).
 * qs_sense_sweeps: n sweep records of `stride` bytes, magic 'QSRL', scan_count 181, exactly the bytes protocol.pack_sweeps
 *     makes of the same fields.  qs_sense_packets: n 42-byte QuasarPacket v2 records, as protocol.pack_packets.
 *     agent (uint8 [n]) is required; enc (int32), v2v (uint32), landmark (uint8) are copied through, NULL = 0.
 * The _device twins take device pointers (pkts_out at any byte address) and are asynchronous on the context's stream.
 * Out of scope: Gaussian noise (a device log / cos would cost the bit-equality), spurious echoes, beam width, a residual
 * between a received sweep and the predicted one, anything fed to the pose graph, sensing across ranks. */
#define QS_SENSE_MAX_CELLS 255   /* patch radius C = ceil(R / res) + 1: (2 C + 1)^2 bits in rows of 64-bit words, 32 704 bytes of LDS */
typedef struct qs_sense_params {
    double   max_range, noise_amp;
    float    no_return;
    uint32_t dropout_q16;
    uint64_t seed, first_record;
    int32_t  reserved[2];
} qs_sense_params;
int qs_sense_ranges(qs_ctx *ctx, const float *pose_xyyaw, size_t n, int32_t beams, const qs_sense_params *params,
                    float *ranges, int32_t *hit_cell);
int qs_sense_ranges_device(qs_ctx *ctx, const float *d_pose_xyyaw, size_t n, int32_t beams, const qs_sense_params *params,
                           float *d_ranges, int32_t *d_hit_cell);
int qs_sense_sweeps(qs_ctx *ctx, const float *pose_xyyaw, const uint8_t *agent, const int32_t *enc, const uint32_t *v2v,
                    size_t n, const qs_sense_params *params, uint8_t *pkts_out, size_t stride);
int qs_sense_sweeps_device(qs_ctx *ctx, const float *d_pose_xyyaw, const uint8_t *d_agent, const int32_t *d_enc,
                           const uint32_t *d_v2v, size_t n, const qs_sense_params *params, uint8_t *d_pkts_out, size_t stride);
int qs_sense_packets(qs_ctx *ctx, const float *pose_xyyaw, const uint8_t *agent, const int32_t *enc, const uint32_t *v2v,
                     const uint8_t *landmark, size_t n, const qs_sense_params *params, uint8_t *pkts_out);
int qs_sense_packets_device(qs_ctx *ctx, const float *d_pose_xyyaw, const uint8_t *d_agent, const int32_t *d_enc,
                            const uint32_t *d_v2v, const uint8_t *d_landmark, size_t n, const qs_sense_params *params,
                            uint8_t *d_pkts_out);

/* ---- sweep check: does a sweep fit the map it is about to be written into? (no reference counterpart: this build's own rule) ----
 * Every beam of a sweep is predicted from the map by the walk of "sensing a world" and compared with the range the sweep carries;
 * a sweep most of whose decided beams contradict the map can be withheld from it (qs_ingest_sweeps_checked).  All comparisons
 * are integer or uncontracted fp64, so a NumPy restatement (tests/check_rules.py) agrees bit for bit once it is given the one
 * sincos the device takes per record.
 *  V1 Map: stamp 0 is UNKNOWN, an odd stamp OCCUPIED, anything else FREE; a cell outside the grid reads UNKNOWN.  The call
 *     observes the map (waiting exact-trig rays are resolved first) and writes nothing to the context: no stamps, counters,
 *     dirty blocks or sequence numbers; a checkpoint before equals one after.
 *  V2 Record and pose: acceptance is qs_ingest_sweeps' rule; rx, ry, yaw are formed exactly as that ingest forms them (offset
 *     first, then the bot's drift, read on the device; graph mode does not change them).  The pose is usable when all three are
 *     finite and both start cells (x0, y0) = world_to_grid(rx), world_to_grid(ry) exist (S2's bound).  Otherwise all 181 beams
 *     are UNSEEN and sin_yaw = cos_yaw = 0.
 *  V3 Directions: (s, c) = the device's sincos(yaw), once per record, reported as sin_yaw, cos_yaw.  Beam i points along
 *     c_i = c * CB[i] - s * SB[i], s_i = s * CB[i] + c * SB[i]; CB, SB are the host-libm tables of sweep-matching rule 3.
 *  V4 Prediction: far point (rx + smax * c_i, ry + smax * s_i), one multiply and one add per axis; its cell (x1, y1) is
 *     world_to_grid of it.  No cell, or a cell more than C = ceil(smax / res) + 1 cells from the start cell on either axis (only
 *     rounding at astronomic coordinates can do that): the beam is UNSEEN.  Otherwise walk the cells of the reference's
 *     _bresenham((x0, y0), (x1, y1)) (:158-179) after cell 0, from the pose outward.  The first cell that is not FREE ends the
 *     walk: OCCUPIED gives "hit at p", UNKNOWN (off-grid included) gives "unknown at p", with
 *     p = res * sqrt(f64(dx*dx + dy*dy)), centre to centre.  A walk that reaches the far cell over FREE cells only is "clear".
 *  V5 Measurement: d = the f32 range widened.  It is a return when smin < d <= smax (the context's sweep filter), otherwise none.
 *  V6 Class of a beam (each test is one fp64 operation followed by one compare; tol in metres):
 *         prediction      return d                                             none
 *         hit at p        d < p - tol: NEARER;  d > p + tol: FARTHER;          MISSED if smin + tol < p and p <= smax - tol,
 *                         else AGREE                                           else UNSEEN
 *         clear           NEARER                                               AGREE
 *         unknown at p    d < p - tol: NEARER;  else UNSEEN                    UNSEEN
 *  V7 Summary: the five counts sum to 181; checked = agree + nearer + farther + missed;
 *     bad = nearer + farther + (count_missed ? missed : 0).  status: QS_CHECK_NO_RECORD for a rejected record (every field of
 *     the result is zero); QS_CHECK_UNDECIDED when checked < min_checked; QS_CHECK_CONTRADICTS when
 *     bad * 100 > max_bad_percent * checked; QS_CHECK_OK otherwise.
 *  V8 Parameters: NULL = tol 2 * res, min_checked 20, max_bad_percent 30, count_missed 0.  Limits: tol finite and >= 0,
 *     min_checked in 0..181, max_bad_percent in 0..100, count_missed 0 or 1, reserved 0, and
 *     ceil(smax / res) + 1 <= QS_SENSE_MAX_CELLS for the context's sweep filter; QS_E_INVAL otherwise, the text names the field.
 *     Stride, lengths and refusals are those of qs_match_sweeps (a sharded context refuses).  n == 0 is valid; any n is accepted
 *     (host calls are chunked internally).
 *  V9 Result: one qs_sweep_check per record (pad is zero) and, optionally, cls_out uint8 [n][181]: the class of every beam,
 *     255 throughout for a rejected record.
 * qs_ingest_sweeps_checked*: ALL records of the call are checked (parameters as above) against the map as it stood before the
 * call, however the call is chunked.  A record whose status is QS_CHECK_CONTRADICTS is WITHHELD: from there on it is treated
 * exactly as a rejected record -- it writes nothing, keeps its 46 sequence numbers, counts in QS_CNT_DATAGRAMS but not in
 * QS_CNT_ACCEPTED, and qs_last_sweeps shows accepted = 0 and a NaN pose.  OK and UNDECIDED records are mapped by
 * qs_ingest_sweeps' rules (an empty map decides nothing, so it withholds nothing).  qs_last_sweep_checks returns the checks
 * (n = the call's n; QS_E_INVAL after any other ingest).  In graph mode the guarded ingest refuses with QS_E_STATE (a withheld
 * sweep would still be a node); qs_check_sweeps itself works in either mode.
 * Not built: a guarded AND matched ingest, a check of the 42-byte packets' four beams, beam width, any use of the hit / miss
 * counters (the stamp's latest word decides, as everywhere else). */
#define QS_BEAM_AGREE 0
#define QS_BEAM_NEARER 1
#define QS_BEAM_FARTHER 2
#define QS_BEAM_MISSED 3
#define QS_BEAM_UNSEEN 4
#define QS_BEAM_NO_RECORD 255
#define QS_CHECK_OK 0
#define QS_CHECK_NO_RECORD 1
#define QS_CHECK_UNDECIDED 2
#define QS_CHECK_CONTRADICTS 3
typedef struct qs_check_params { double tol; int32_t min_checked, max_bad_percent, count_missed, reserved; } qs_check_params;
typedef struct qs_sweep_check {
    int32_t agree, nearer, farther, missed, unseen, checked, bad, status;
    uint8_t accepted_record, pad[7];
    double  sin_yaw, cos_yaw;
} qs_sweep_check;
int qs_check_sweeps(qs_ctx *ctx, const qs_check_params *params, const uint8_t *pkts, size_t n, size_t stride,
                    const uint16_t *lens, qs_sweep_check *out, uint8_t *cls_out);
/* same with device-resident pkts / lens / out / cls_out; asynchronous on the context's stream */
int qs_check_sweeps_device(qs_ctx *ctx, const qs_check_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                           const uint16_t *d_lens, qs_sweep_check *d_out, uint8_t *d_cls_out);
int qs_ingest_sweeps_checked(qs_ctx *ctx, const qs_check_params *params, const uint8_t *pkts, size_t n, size_t stride,
                             const uint16_t *lens, uint64_t seq0);
int qs_ingest_sweeps_checked_device(qs_ctx *ctx, const qs_check_params *params, const uint8_t *d_pkts, size_t n,
                                    size_t stride, const uint16_t *d_lens, uint64_t seq0);
int qs_last_sweep_checks(qs_ctx *ctx, qs_sweep_check *out, size_t n);

/* ---- map view: the "Mission Control" map, MapRenderer  dual_bot_mapper.py:380-668 -------------------------------------------
 * One call renders a frame of the map for any pan and zoom on the device and hands back only the frame: [height][width][4]
 * bytes R, G, B, 255, row 0 at the top.  The layers are the reference's (:433-468) as far as its own Python pins their pixels
 * (set_at, a filled rect, a 1-pixel axis-parallel line); a NumPy restatement (tests/view_rules.py) agrees byte for byte.
 * Every expression is fp64, each operation rounded on its own; int() truncates toward zero, as Python's does.
 *  R0 screen mapping (:404-408): sx = int(offset_x + wx*scale), sy = int(offset_y - wy*scale).  A value that is not finite or
 *     beyond 2^30 in magnitude is not drawn (a zone or segment with one such corner or end is not drawn at all).  Truncation
 *     toward zero makes pixel column and row 0 take the values in (-1, 1): the reference's behaviour, kept everywhere.
 *  R1 the frame is filled with bg.
 *  R2 metre lines (:476-485): for v in line_min..line_max column sx(v) if inside [0, width) and row sy(v) if inside
 *     [0, height), in `line`.  The origin crosshair is a 2-pixel-wide pygame line: its pixels are pygame's, it is left out.
 *  R3 occupancy (:492-527): cell_px = max(1, int(res*scale)); a cell's screen point is R0 of its centre ox + (gx+0.5)*res,
 *     oy + (gy+0.5)*res; its state is the stamp's (0 UNKNOWN, odd OCCUPIED, else FREE).
 *       cell_px >= 3  each FREE cell fills the cell_px x cell_px square whose top-left is (sx - cell_px/2, sy - cell_px/2),
 *                     clipped to the frame;
 *       cell_px == 2  each FREE cell sets the pixel (sx, sy) (the reference's set_at branch);
 *       cell_px <  2  minify != 0: a pixel's footprint is the set of cells whose screen point is that pixel; with
 *                     draw_occupied the pixel is `occ` if any footprint cell is OCCUPIED, otherwise `free` if any is FREE,
 *                     otherwise it stays as R1 / R2 made it.  minify == 0: nothing is drawn (the reference: "too zoomed
 *                     out", :495-496).
 *     draw_occupied (a build extension; the reference skips OCCUPIED cells, :519-520): OCCUPIED cells are drawn by the same
 *     geometry in `occ`, after all FREE cells.
 *     The rule looks at EVERY cell.  The reference first culls to a visible cell range (:500-508) with no margin on the side of
 *     the larger indices; a cell just beyond it whose screen y lies in (-cell_px, 0) can still reach frame row 0 through the
 *     truncation toward zero, and the culled loop drops it.  Frame row 0 is the only place the two can differ.
 *  R4 zones (:537-551), in array order: (sx1, sy1) = R0(minx, maxy), (sx2, sy2) = R0(maxx, miny), w = sx2 - sx1,
 *     h = sy2 - sy1; drawn only if w > 0 and h > 0.  Every pixel of [sx1, sx1+w) x [sy1, sy1+h) becomes
 *     (c*25 + dst*230 + 127) / 255 per channel, then the 1-pixel border of that rectangle is set to c.  Later zones blend over
 *     earlier ones, borders included.  Rectangle and border geometry are the reference's; the blend arithmetic is this
 *     build's (alpha 25 of 255, rounded to nearest): pygame's own blit cannot be run where the fixtures are recorded.
 *  R5 primitives, opaque, in array order: per pixel the highest index that covers it wins.
 *       QS_VIEW_POINT    the pixel R0(x0, y0) (:574);
 *       QS_VIEW_SQUARE   size x size pixels, top-left (sx - size/2, sy - size/2) (:570-572), 1 <= size <= 64, clipped;
 *       QS_VIEW_SEGMENT  the cells of the reference's _bresenham (:158-179) from R0(x0, y0) to R0(x1, y1), both ends
 *                        inclusive, clipped to the frame, one pixel wide (the reference draws paths and closures with
 *                        pygame's width-2 lines, whose pixels are pygame's: one pixel wide is this build's rule).  Cell k has
 *                        major offset k and minor offset (2*k*m + M - 1) / (2*M), M >= m the two extents; k is clipped to the
 *                        frame along the major axis first, so a segment costs at most the frame's side, whatever its length.
 *     Robot triangles, labels and the HUD text stay with the host.
 * Parameters: 1 <= width, height <= QS_VIEW_MAX_DIM; scale finite and > 0 with res*scale <= QS_VIEW_MAX_CELL_PX; offsets
 * finite; line_max - line_min < QS_VIEW_MAX_LINES (line_max < line_min: no lines); colours are bytes R, G, B (the fourth is
 * ignored); n_zones <= QS_VIEW_MAX_ZONES, n_prims <= QS_VIEW_MAX_PRIMS; a primitive's kind is one of the three.  Anything
 * else: QS_E_INVAL.  zones / prims are host arrays in both entry points; d_rgba is device memory on the context's GPU
 * (asynchronous on the context's stream), rgba_host is complete when the call returns.
 * The call observes the map (waiting exact-trig rays are resolved first) and writes nothing to the context: stamps,
 * counters, dirty blocks and zone boxes stay as they were; a checkpoint before equals one after. */
#define QS_VIEW_MAX_DIM 8192
#define QS_VIEW_MAX_ZONES 1024
#define QS_VIEW_MAX_PRIMS (1 << 24)
#define QS_VIEW_MAX_SQUARE 64
#define QS_VIEW_MAX_LINES 65536
#define QS_VIEW_MAX_CELL_PX (1 << 20)
enum { QS_VIEW_POINT = 0, QS_VIEW_SQUARE = 1, QS_VIEW_SEGMENT = 2 };
typedef struct qs_view_params {
    int32_t width, height;                      /* MapRenderer(width, height)  :383 */
    double scale, offset_x, offset_y;           /* pixels per metre; screen position of the world origin  :395-397 */
    int32_t line_min, line_max;                 /* metre lines, the reference: -20..20  :479 */
    uint8_t bg[4], line[4], free[4], occ[4];    /* BG_COLOR, GRID_COLOR, CELL_COLOR_FREE, CELL_COLOR_OCCUPIED  :346-347, :373-374 */
    int32_t draw_occupied, minify;
    int32_t reserved[2];
} qs_view_params;
typedef struct qs_view_zone { double minx, miny, maxx, maxy; uint8_t color[4]; int32_t reserved; } qs_view_zone;
typedef struct qs_view_prim { double x0, y0, x1, y1; int32_t kind, size; uint8_t color[4]; int32_t reserved; } qs_view_prim;
int qs_render_view(qs_ctx *ctx, const qs_view_params *params, const qs_view_zone *zones, size_t n_zones,
                   const qs_view_prim *prims, size_t n_prims, uint8_t *rgba_host);
int qs_render_view_device(qs_ctx *ctx, const qs_view_params *params, const qs_view_zone *zones, size_t n_zones,
                          const qs_view_prim *prims, size_t n_prims, uint8_t *d_rgba);

/* ---- EKF  AgentFirmware_Bot1/ekf.cpp:5-92 ---------------------------------------------- */
/* On ingest (qs_config.enable_ekf) the filter of every bot runs over the batch: batches of >= 4096
 * packets in a parallel-in-time form that agrees with the step-by-step filter to rounding (~1e-12
 * relative), smaller ones step by step.  QS_CNT_EKF_WRAP_CLAMP counts chunks whose heading-wrap count
 * had to be clamped (a sign of absurd inputs; 0 on every stream seen). */
/* batched over bots: for k in 0..n: predict(omega_m[k], t[k]) then update(z_v[k], z_omega[k])
 * on bot_ids[k] (each bot at most once per call); do_update == 0: predict only.  qs_ekf_init is the constructor plus
 * EKF::init (P = I again).  Before a bot's first init, predict and update do nothing and qs_ekf_state reports the
 * constructed object: x = 0, P = I (qs_create and qs_reset store that).  A checkpoint written before they did holds
 * all zeros for such a bot and restores them: P = 0 until the bot's first init. */
int qs_ekf_init(qs_ctx *ctx, int32_t bot, double t, const double x0[6]);
int qs_ekf_step(qs_ctx *ctx, const int32_t *bot_ids, const double *omega_m, const double *t,
                const double *z_v, const double *z_omega, size_t n, int32_t do_update);
int qs_ekf_state(qs_ctx *ctx, int32_t bot, double x[6], double P[36]);

/* ---- checkpoint / restore ------------------------------------------------------------------------------------------------
 * qs_checkpoint writes the session state of a context into a byte buffer; qs_restore loads it into a context whose
 * configuration matches.  From then on every call on the restored context returns bit for bit what it would have returned on
 * the original given the same later calls: ingests (packets, sweeps), grid / counter / log-odds views, closures, closure
 * agents, landmarks, sizes, drift, zones, EKF state, frontiers and targets, qs_counters, both fuses.
 *   saved      the grid as blocks of QS_DIRTY_BLOCK_H x QS_DIRTY_BLOCK_W cells (the sparse fuse's), each block that holds
 *              anything: its stamps and counters (enable_counts), with dirty tracking also the sparse fuse's "sent" and fused
 *              counters, and the live dirty bitmap; the dirty_since_fuse flag, and with tracking the counts view; per bot the
 *              offset, drift, last closure, zone box words, EKF state (44 words) and previous values (4 words); per pose graph
 *              the node count, the landmark log and the closure log; the sequence counter, stamp epoch and rebase count; the
 *              sweep filter; the exact-trig totals; every QS_CNT_* counter.
 *   not saved  (as after qs_reset) the resident last batch (qs_last_batch / qs_last_hits / qs_last_sweeps refuse), workspaces,
 *              timing, the chain form and QS_CHAIN_AUTO's running choice (every form gives the same closures), and the dense
 *              fuse's counter snapshot (the counts view reads the local counters until the next fuse).  The landmark bucket
 *              index is not in the file: qs_restore rebuilds it on the device from the landmark log.
 *   checkpoint observes the map (resolves waiting exact-trig rays first) and waits for the GPU.  buf == NULL: *n_out = the
 *              size, nothing written.  cap < size: QS_E_RANGE (*n_out = the size).  QS_E_STATE while a sparse fuse is in
 *              flight, or when a loop-closure chain wait has timed out (bit 40 of QS_CNT_SLAM_ROUNDS): such a map may be wrong.
 *   restore    everything is checked on the host before anything changes: magic, version, lengths, CRC, block ids, and the
 *              configuration fields size, res, ox, oy, min_dist, max_dist, closure_radius, min_poses_between,
 *              closure_correction, max_agent, bots_per_graph, enable_counts, enable_ekf, ekf_metres_per_tick, seq_stride,
 *              shard_bots, shard_rank, exact_trig (device, raycast_mode and separation may differ).  A refused restore leaves
 *              the context as it was: QS_E_INVAL (qs_last_error names the first field that differs, or the failed check),
 *              QS_E_STATE while a sparse fuse is in flight.  A HIP failure after that leaves the context reset.  Dirty
 *              tracking of the context is switched to the checkpoint's.
 * Format (version 1), little-endian, every section at an 8-byte aligned offset:
 *   header   0  char magic[4] = "QSCK"     4  u32 version        8  u32 header_bytes (= 144 + 24 n_sections)
 *           12  u32 n_sections            16  u64 total_bytes   24  u32 crc32 of bytes [header_bytes, total_bytes) (zlib's)
 *           28  u32 reserved
 *           32  i32 size, min_poses_between, max_agent, bots_per_graph, enable_counts, enable_ekf, seq_stride, shard_bots,
 *               shard_rank, exact_trig, dirty_tracking, reserved
 *           80  f64 res, ox, oy, min_dist, max_dist, closure_radius, closure_correction, ekf_metres_per_tick
 *          144  section table: n_sections x {u32 kind, u32 reserved, u64 offset, u64 length}
 *   SCALARS    u64 next_seq, epoch_base, n_rebases, edge_rays, edge_overflow; f64 sweep_min, sweep_max;
 *              u32 dirty_since_fuse, counts_view_fused, n_graphs, n_bots (= max_agent + 1)                        72 bytes
 *   BOTS       n_bots x: f64 offset; f64 drift[2]; i64 last_closure; u64 zone[4]; f64 ekf[44]; f64 ekf_prev[4], as six
 *              arrays in that order (all bots' offsets, then all drifts, ...); slot 0 is no bot.  zone = min x, min y, max x,
 *              max y of the box qs_zone reports, each f64 as the u64 that orders as the number does: its bits inverted if
 *              the sign bit is set, else with the sign bit set; a bot without points holds 2^64 - 1, 2^64 - 1, 0, 0.
 *              ekf = x[6], P[36] row-major (what qs_ekf_state reports), the time of the last step, initialised (0.0 / 1.0);
 *              ekf_prev = the bot's previous packet: time, yaw, encoder count, seen (0.0 / 1.0)
 *   COUNTERS  u64[QS_CNT_N] as the device holds them (QS_CNT_REBASES / EDGE_* come from SCALARS)
 *   GRAPHS     n_graphs x {i64 n_nodes, n_landmarks, n_closures}, then per graph: landmark log f64 x[L], f64 y[L],
 *              i64 node[L], u8 type[L] (padded to 8), closure log i64 landmark[C], i64 node[C], f64 dx[C], f64 dy[C],
 *              u8 agent[C] (padded to 8)
 *   BLOCK_IDS  u32[n_blocks], ascending: block (bx, by) is by * 32 * pitch + bx, pitch = ceil(ceil(size / 16) / 32)
 *   BLOCKS     per block, cells row-major (lane = 16 * row + column): u32 stamps[64]; enable_counts: u64 counters[64];
 *              enable_counts and dirty_tracking: u64 sent[64], u64 fused[64].  Cells beyond the grid's edge are 0.  A
 *              counter word is hits << 32 | misses (the int32 pair of qs_device_buffers, misses first).
 *   DIRTY      dirty_tracking only: u32[ceil(size / 4) * pitch], the live dirty bitmap: bit (id % 32) of word (id / 32) is
 *              block id; the bits of a row beyond its last block mean nothing
 * A version the library does not know is refused. */
#define QS_CKPT_MAGIC "QSCK"
#define QS_CKPT_VERSION 1
#define QS_CKPT_HEADER_FIXED 144
enum { QS_CKPT_SCALARS = 1, QS_CKPT_BOTS, QS_CKPT_COUNTERS, QS_CKPT_GRAPHS, QS_CKPT_BLOCK_IDS, QS_CKPT_BLOCKS, QS_CKPT_DIRTY };
int qs_checkpoint(qs_ctx *ctx, uint8_t *buf, size_t cap, size_t *n_out);
int qs_restore(qs_ctx *ctx, const uint8_t *buf, size_t n);

/* ---- counters / timing ------------------------------------------------------------------ */
enum { QS_CNT_DATAGRAMS = 0, QS_CNT_ACCEPTED, QS_CNT_RAYS, QS_CNT_CELLS, QS_CNT_HITS,
       QS_CNT_CLOSURES, QS_CNT_LANDMARKS, QS_CNT_REBASES, QS_CNT_SLAM_WINDOWS, QS_CNT_SLAM_ROUNDS,
       QS_CNT_SLAM_NODE_ITERS, QS_CNT_SLAM_MISC_ITERS, QS_CNT_SLAM_CYCLES, QS_CNT_SLAM_REALTIME, QS_CNT_SLAM_CYC_A, QS_CNT_SLAM_CYC_B,
       QS_CNT_SLAM_CYC_C, QS_CNT_EKF_WRAP_CLAMP, QS_CNT_EDGE_RAYS /* exact_trig: rays resolved on the host */,
       QS_CNT_EDGE_OVERFLOW /* exact_trig: rays that found the waiting list full and were cast with the device's trig */, QS_CNT_N };
int qs_counters(qs_ctx *ctx, uint64_t out[QS_CNT_N]);
/* HIP-event timing of the pipeline stages on the context's stream.  enable != 0 brackets
 * each stage of every ingest with events; qs_stage_times returns accumulated ms and the
 * launch count per stage since the last call with reset != 0. */
enum { QS_STAGE_DECODE = 0, QS_STAGE_SLAM, QS_STAGE_RAYCAST, QS_STAGE_EKF,
       /* single kernels inside the stages above (their time is part of the stage's too) */
       QS_STAGE_SLAM_CHAIN,                     /* the loop-closure chain kernel alone (inside SLAM) */
       QS_STAGE_RC_RAYS, QS_STAGE_RC_SORT, QS_STAGE_RC_RASTER,   /* tiled raycast: pass A; passes B + C; pass D */
       QS_STAGE_N };
int qs_timing_enable(qs_ctx *ctx, int32_t enable);
int qs_stage_times(qs_ctx *ctx, double ms[QS_STAGE_N], uint64_t launches[QS_STAGE_N],
                   int32_t reset);

const char *qs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QUASAR_SLAM_H */
