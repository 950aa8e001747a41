"""Wire formats of the mapper path (host side, no GPU involved).

Mirrors server_nodes/dual_bot_mapper.py:40-54 (struct formats), :57-99 (constants) and the
packet producer struct of AgentFirmware_Bot1/AgentFirmware_Bot1.ino:172-185.
"""
import math
import struct

import numpy as np

# QuasarPacket v2 / v1 from the bots, ZONE / TARG to the bots  (dual_bot_mapper.py:41-54)
PACKET_FMT = "<4sBfffiIffffB"
PACKET_SIZE = struct.calcsize(PACKET_FMT)          # 42
PACKET_FMT_V1 = "<4sBfffiIffff"
PACKET_SIZE_V1 = struct.calcsize(PACKET_FMT_V1)    # 41
ZONE_FMT = "<4sffff"
ZONE_SIZE = struct.calcsize(ZONE_FMT)              # 20
TARGET_FMT = "<4sff"
TARGET_SIZE = struct.calcsize(TARGET_FMT)          # 12

MAX_DIST_M = 1.20
MIN_DIST_M = 0.05
SENSOR_ANGLES_RAD = {"front": 0.0, "left": math.pi / 2, "back": math.pi, "right": -math.pi / 2}
SENSOR_NAMES = ("front", "left", "back", "right")

LM_NONE, LM_CORNER_L, LM_CORNER_R, LM_CORRIDOR, LM_DEAD_END, LM_OPEN = range(6)
LANDMARK_NAMES = {LM_NONE: "NONE", LM_CORNER_L: "CORNER_L", LM_CORNER_R: "CORNER_R",
                  LM_CORRIDOR: "CORRIDOR", LM_DEAD_END: "DEAD_END", LM_OPEN: "OPEN"}

HEARTBEAT_TIMEOUT = 5.0
ZONE_UPDATE_INTERVAL = 2.0

GRID_RESOLUTION = 0.05
GRID_SIZE = 200
GRID_ORIGIN_X = -5.0
GRID_ORIGIN_Y = -5.0
CELL_UNKNOWN, CELL_FREE, CELL_OCCUPIED = -1, 0, 100

CLOSURE_RADIUS = 0.60
MIN_POSES_BETWEEN = 30
CLOSURE_CORRECTION = 0.5
FRONTIER_MIN_CLUSTER = 3
FRONTIER_SEPARATION = 1.0
TARGET_INTERVAL = 3.0
# path planning defaults (include/quasar_slam.h): build choices, the reference has no planner
PLAN_CLEARANCE = 2          # cells: 0.10 m at 0.05 m per cell (the bots follow walls at 0.25 m)
PLAN_SNAP_RADIUS = 10       # cells
PLAN_LOOKAHEAD = 200        # path cells tested for a straight drive

# numpy view of the packed 42-byte record (same field order as PACKET_FMT)
PACKET_DTYPE = np.dtype([("magic", "S4"), ("agent", "u1"), ("x", "<f4"), ("y", "<f4"), ("yaw", "<f4"),
                         ("enc", "<i4"), ("v2v", "<u4"), ("front", "<f4"), ("left", "<f4"),
                         ("back", "<f4"), ("right", "<f4"), ("lm", "u1")])
assert PACKET_DTYPE.itemsize == PACKET_SIZE


def pack_packet(agent, x, y, yaw, enc, v2v, front, left, back, right, landmark=LM_NONE) -> bytes:
    return struct.pack(PACKET_FMT, b"QSRL", agent, x, y, yaw, enc, v2v, front, left, back, right, landmark)


def pack_packets(agent, x, y, yaw, enc, v2v, dist4, landmark) -> np.ndarray:
    """Vectorised packer: arrays -> uint8 [n, 42]."""
    n = len(agent)
    rec = np.zeros(n, dtype=PACKET_DTYPE)
    rec["magic"] = b"QSRL"
    rec["agent"], rec["x"], rec["y"], rec["yaw"] = agent, x, y, yaw
    rec["enc"], rec["v2v"] = enc, v2v
    d = np.asarray(dist4, dtype=np.float32)
    rec["front"], rec["left"], rec["back"], rec["right"] = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    rec["lm"] = landmark
    return rec.view(np.uint8).reshape(n, PACKET_SIZE)


def pack_datagrams(datagrams):
    """Variable-length datagrams -> (uint8 [n, 48] zero padded, uint16 lengths); datagrams
    longer than 48 bytes are recorded with their true length and dropped by the decoder."""
    n = len(datagrams)
    buf = np.zeros((n, 48), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    for i, d in enumerate(datagrams):
        m = min(len(d), 48)
        buf[i, :m] = np.frombuffer(d[:m], dtype=np.uint8)
        lens[i] = min(len(d), 65535)
    return buf, lens


def zone_packet(box) -> bytes:
    """send_zone_to_bot's payload (dual_bot_mapper.py:675-684)."""
    if box is None:
        return struct.pack(ZONE_FMT, b"ZONE", 999.0, 999.0, -999.0, -999.0)
    return struct.pack(ZONE_FMT, b"ZONE", box[0], box[1], box[2], box[3])


def pack_target(x, y) -> bytes:
    """send_target_to_bot's payload (dual_bot_mapper.py:691-699): 12 bytes, read by AgentFirmware_Bot1.ino:81-137."""
    return struct.pack(TARGET_FMT, b"TARG", x, y)


def compute_bounding_box(points_x, points_y):
    """dual_bot_mapper.py:702-706."""
    if len(points_x) == 0:
        return None
    return (min(points_x), min(points_y), max(points_x), max(points_y))


# ---- legacy Quasar-Lite v0 packet of the ROS bridge (server_nodes/udp_bridge.py:25-38) ----------
# magic, agent_id, x, y, yaw, scan_count, 181 servo-sweep ranges; command back: 'CMD1', linear_x, angular_z
PACKET_FMT_V0 = "<4sBfffH181f"
PACKET_SIZE_V0 = struct.calcsize(PACKET_FMT_V0)      # 743
CMD_FMT = "<4sff"
PACKET_DTYPE_V0 = np.dtype([("magic", "S4"), ("agent", "u1"), ("x", "<f4"), ("y", "<f4"), ("yaw", "<f4"),
                            ("scan_count", "<u2"), ("ranges", "<f4", (181,))])
assert PACKET_DTYPE_V0.itemsize == PACKET_SIZE_V0


# the same sweep with odometry: i32 encoder, u32 v2v before scan_count (server_nodes/udp_receiver_standalone.py:15,
# room_mapper.py:21); the standalone receiver logs it as CSV (:78-82)
PACKET_FMT_V0_ODO = "<4sBfffiIH181f"
PACKET_SIZE_V0_ODO = struct.calcsize(PACKET_FMT_V0_ODO)      # 751
PACKET_DTYPE_V0_ODO = np.dtype([("magic", "S4"), ("agent", "u1"), ("x", "<f4"), ("y", "<f4"), ("yaw", "<f4"),
                                ("enc", "<i4"), ("v2v", "<u4"), ("scan_count", "<u2"), ("ranges", "<f4", (181,))])
assert PACKET_DTYPE_V0_ODO.itemsize == PACKET_SIZE_V0_ODO
SWEEP_BEAMS = 181
SWEEP_SEQS = 46              # sequence numbers one sweep uses in the mapper's stamp order (include/quasar_slam.h)
BOT_VEIL_RADIUS = 3          # cells: default radius of the bot veil (include/quasar_slam.h, "bot veil")
SWEEP_MIN_DIST_M = 0.1       # trust filter of the reference's sweep map, generate_topdown_map.py:51
SWEEP_MAX_DIST_M = 1.2
# sweeps in the pose graph (include/quasar_slam.h, "sweeps in the pose graph"): the signature rule's defaults and limits
SWEEP_GRAPH_HALF_WIDTH = 5   # beams either side of beams 0 (right), 90 (front), 180 (left) whose median is the sector's range
SWEEP_GRAPH_MAX_HALF_WIDTH = 29
SWEEP_GRAPH_CLOSE_M = 0.40   # detectLandmark's thresholds, AgentFirmware_Bot1.ino:152-169
SWEEP_GRAPH_OPEN_M = 0.80
SWEEP_LM_REJECTED = 255      # sweep_signatures / last_sweep_nodes: the record was not accepted
# sweep matching (include/quasar_slam.h, "sweep matching"): build choices, there is no reference counterpart
MATCH_RADIUS = 2             # cells the likelihood field reaches from an occupied cell
MATCH_WINDOW = 6             # candidate shifts: +- cells on both axes
MATCH_ANGLE_STEPS = 10       # candidate rotations: +- steps
MATCH_ANGLE_STEP = math.pi / 180
MATCH_MIN_HITS = 20          # a sweep with fewer hit beams is not moved
MATCH_MIN_PERCENT = 50       # ... nor one whose best score is under this share of hits * (radius + 1)
MATCH_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("it", "<i4"), ("score", "<i4"), ("score0", "<i4"), ("hits", "<i4"),
                        ("accepted_record", "u1"), ("accepted_match", "u1"), ("pad", "u1", (6,)),
                        ("dx", "<f8"), ("dy", "<f8"), ("dyaw", "<f8")])
# relocalisation (include/quasar_slam.h, "relocalisation"): build choices taken from a CPU prototype of the rule
RELOC_RADIUS = 2             # the likelihood field's reach, as MATCH_RADIUS
RELOC_N_ROT = 180            # rotation steps over the full turn
RELOC_SEP = 4                # a rival lies more than this many cells from the best on an axis ...
RELOC_SEP_ROT = 2            # ... or more than this many rotation steps
RELOC_MIN_HITS = 40
RELOC_MIN_PERCENT = 70       # the best score against hits * (radius + 1)
RELOC_MIN_MARGIN = 5         # ... and its lead over the rival, in the same percent
RELOC_MAX_ROT, RELOC_MAX_SEP = 360, 16
RELOC_OK, RELOC_NO_RECORD, RELOC_NO_CANDIDATE = 0, 1, 2
RELOC_DTYPE = np.dtype([("gx", "<i4"), ("gy", "<i4"), ("j", "<i4"), ("score", "<i4"), ("hits", "<i4"),
                        ("gx2", "<i4"), ("gy2", "<i4"), ("j2", "<i4"), ("score2", "<i4"), ("status", "<i4"),
                        ("accepted_record", "u1"), ("accepted", "u1"), ("pad", "u1", (6,)),
                        ("x", "<f8"), ("y", "<f8"), ("yaw", "<f8")])
# relocalisation of a group (include/quasar_slam.h, J1-J8)
RELOC_MAX_GROUP = 16
RELOC_TRAVEL = 2.0           # metres a record of a group may lie from the group's frame
RELOC_REL_DTYPE = np.dtype([("tx", "<f8"), ("ty", "<f8"), ("s", "<f8"), ("c", "<f8")])
GROUP_RELOC_DTYPE = np.dtype([("gx", "<i4"), ("gy", "<i4"), ("j", "<i4"), ("score", "<i4"), ("hits", "<i4"),
                              ("gx2", "<i4"), ("gy2", "<i4"), ("j2", "<i4"), ("score2", "<i4"), ("status", "<i4"),
                              ("records", "u1"), ("accepted", "u1"), ("pad", "u1", (6,)),
                              ("x", "<f8"), ("y", "<f8"), ("yaw", "<f8")])
# trail matching (include/quasar_slam.h, T1-T8): the last packets of one bot matched against the map as one rigid constellation
TRAIL_MAX_RECORDS = 64
TRAIL_TRAVEL = 4.0           # metres a record of a trail may lie from the trail's last pose
TRAIL_MATCH_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("it", "<i4"), ("score", "<i4"), ("score0", "<i4"), ("hits", "<i4"),
                              ("records", "<i4"), ("anchor", "<i4"), ("agent", "u1"), ("accepted_match", "u1"), ("pad", "u1", (6,)),
                              ("ax", "<f8"), ("ay", "<f8"), ("dx", "<f8"), ("dy", "<f8"), ("dyaw", "<f8")])
assert TRAIL_MATCH_DTYPE.itemsize == 80
# trail relocalisation (include/quasar_slam.h, "trail relocalisation"): GROUP_RELOC_DTYPE's fields where it has them
TRAIL_RELOC_DTYPE = np.dtype([("gx", "<i4"), ("gy", "<i4"), ("j", "<i4"), ("score", "<i4"), ("hits", "<i4"),
                              ("gx2", "<i4"), ("gy2", "<i4"), ("j2", "<i4"), ("score2", "<i4"), ("status", "<i4"),
                              ("records", "u1"), ("accepted", "u1"), ("agent", "u1"), ("pad", "u1"), ("anchor", "<i4"),
                              ("x", "<f8"), ("y", "<f8"), ("yaw", "<f8"), ("ax", "<f8"), ("ay", "<f8")])
assert TRAIL_RELOC_DTYPE.itemsize == 88
# sweep check (include/quasar_slam.h, "sweep check"): build choices taken from a CPU prototype of the rule
CHECK_TOL_CELLS = 2          # tol defaults to this many cells
CHECK_MIN_CHECKED = 20       # a sweep with fewer decided beams is UNDECIDED
CHECK_MAX_BAD_PERCENT = 30   # more than this share of the decided beams contradicting the map: CONTRADICTS
CHECK_COUNT_MISSED = 0       # a wall the sweep did not return is not held against it (glass, dropouts)
CHECK_LOST_AFTER = 5         # MissionControl: consecutive contradicted sweeps after which a bot counts as lost
BEAM_AGREE, BEAM_NEARER, BEAM_FARTHER, BEAM_MISSED, BEAM_UNSEEN, BEAM_NO_RECORD = 0, 1, 2, 3, 4, 255
CHECK_OK, CHECK_NO_RECORD, CHECK_UNDECIDED, CHECK_CONTRADICTS = 0, 1, 2, 3
CHECK_DTYPE = np.dtype([("agree", "<i4"), ("nearer", "<i4"), ("farther", "<i4"), ("missed", "<i4"), ("unseen", "<i4"),
                        ("checked", "<i4"), ("bad", "<i4"), ("status", "<i4"), ("accepted_record", "u1"), ("pad", "u1", (7,)),
                        ("sin_yaw", "<f8"), ("cos_yaw", "<f8")])


def reloc_rel(x, y, yaw, anchor=0):
    """The relative poses (J2) of the records of ONE group from their poses x, y, yaw (the packets' f32 fields, or anything
    array-like), RELOC_REL_DTYPE [n]: the group's frame is the pose of record `anchor`.  Formed in fp64 with libm: (dx, dy)
    from the anchor, turned into the anchor's heading, then the sin / cos of yaw - yaw0."""
    x, y, yaw = (np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1) for v in (x, y, yaw))
    out = np.zeros(len(x), dtype=RELOC_REL_DTYPE)
    if len(x) == 0:
        return out
    c0, s0 = math.cos(float(yaw[anchor])), math.sin(float(yaw[anchor]))
    for k in range(len(x)):
        dx, dy = float(x[k]) - float(x[anchor]), float(y[k]) - float(y[anchor])
        d = float(yaw[k]) - float(yaw[anchor])
        out[k] = (c0 * dx + s0 * dy, c0 * dy - s0 * dx, math.sin(d), math.cos(d))
    return out


def trail_move(match, x, y, yaw):
    """Rule T7's transform: where a pose (x, y, yaw) of the matched bot -- in the frame of T3, offset and drift included --
    lies after the correction of `match` (one TRAIL_MATCH_DTYPE record, or anything with ax, ay, dx, dy, dyaw): the turn by dyaw
    about the anchor (ax, ay), then the shift.  Scalars or arrays; fp64 with libm.  An unaccepted match (dx = dy = dyaw = 0)
    leaves the pose where it is."""
    ax, ay, dx, dy, dyaw = (float(match[k]) for k in ("ax", "ay", "dx", "dy", "dyaw"))
    s, c = math.sin(dyaw), math.cos(dyaw)
    x, y, yaw = (np.asarray(v, dtype=np.float64) for v in (x, y, yaw))
    qx, qy = x - ax, y - ay
    return ax + (c * qx - s * qy) + dx, ay + (s * qx + c * qy) + dy, yaw + dyaw


def trail_reloc_move(result, x, y, yaw):
    """Rule K7's transform: where a pose (x, y, yaw) in the frame of the located bot's packet fields lies on the map, by
    `result` (one TRAIL_RELOC_DTYPE record, or anything with x, y, yaw, ax, ay): the turn by yaw about the anchor's fields
    (ax, ay), the anchor set down at (x, y).  Scalars or arrays; fp64 with libm."""
    fx, fy, fyaw, ax, ay = (float(result[k]) for k in ("x", "y", "yaw", "ax", "ay"))
    s, c = math.sin(fyaw), math.cos(fyaw)
    x, y, yaw = (np.asarray(v, dtype=np.float64) for v in (x, y, yaw))
    qx, qy = x - ax, y - ay
    return fx + (c * qx - s * qy), fy + (s * qx + c * qy), yaw + fyaw


# ---- map view (include/quasar_slam.h, "map view"): the renderer's constants, dual_bot_mapper.py:346-377, :383-397 ----------
BG_COLOR = (22, 33, 62)
GRID_COLOR = (40, 50, 80)
CELL_COLOR_FREE = (30, 45, 70)
CELL_COLOR_OCCUPIED = (200, 200, 200)
CLOSURE_LINE_COLOR = (0, 255, 100)           # :637
BOT_COLORS = {
    1: {"main": (0, 191, 255), "path": (0, 120, 180), "front": (255, 68, 68), "left": (68, 255, 68), "back": (255, 136, 0),
        "right": (68, 136, 255), "name": "Bot1"},
    2: {"main": (255, 105, 180), "path": (180, 60, 120), "front": (204, 0, 0), "left": (0, 204, 0), "back": (204, 102, 0),
        "right": (0, 68, 204), "name": "Bot2"},
}
VIEW_WIDTH, VIEW_HEIGHT, VIEW_SCALE = 1000, 800, 100.0       # MapRenderer(width, height), self.scale  :383, :395
VIEW_SCALE_LIMITS = (20.0, 500.0)            # the zoom clamp  :419
VIEW_LINE_MIN, VIEW_LINE_MAX = -20, 20       # metre lines  :479
VIEW_CLOUD_RECENT = 2000                     # cloud points drawn per bot and sensor  :561
VIEW_CLOUD_RECT = 8                          # bot 1 left / bot 2 right are 8 x 8 squares  :563-565
VIEW_PATH_POINTS = 500                       # a path is subsampled by max(1, len // 500)  :583
VIEW_POINT, VIEW_SQUARE, VIEW_SEGMENT = 0, 1, 2
VIEW_ZONE_DTYPE = np.dtype([("box", "<f8", (4,)), ("color", "u1", (4,)), ("reserved", "<i4")])            # struct qs_view_zone
VIEW_PRIM_DTYPE = np.dtype([("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("kind", "<i4"), ("size", "<i4"),
                            ("color", "u1", (4,)), ("reserved", "<i4")])                                    # struct qs_view_prim
assert VIEW_ZONE_DTYPE.itemsize == 40 and VIEW_PRIM_DTYPE.itemsize == 48


def bot_colors(bot_id):
    """BOT_COLORS for every id: bots 1 and 2 are the reference's (:351-370).  Beyond them the reference has no colours; the
    stated rule: 'main' is the fully saturated hue (bot_id * 47) % 360 degrees (integer HSV sectors), 'path' two thirds of it,
    and the four sensor colours are bot 1's for odd ids and bot 2's for even ids."""
    if bot_id in BOT_COLORS:
        return BOT_COLORS[bot_id]
    hue = (bot_id * 47) % 360
    sector, ramp = hue // 60, (hue % 60) * 255 // 60
    main = ((255, ramp, 0), (255 - ramp, 255, 0), (0, 255, ramp), (0, 255 - ramp, 255), (ramp, 0, 255), (255, 0, 255 - ramp))[sector]
    out = dict(BOT_COLORS[1 if bot_id % 2 else 2])
    out.update(main=main, path=tuple(2 * v // 3 for v in main), name=f"Bot{bot_id}")
    return out


def pack_v0(agent, x, y, yaw, ranges, scan_count=SWEEP_BEAMS, magic=b"QSRL") -> bytes:
    return struct.pack(PACKET_FMT_V0, magic, agent, x, y, yaw, scan_count, *ranges)


def pack_v0_odo(agent, x, y, yaw, enc, v2v, ranges, scan_count=SWEEP_BEAMS, magic=b"QSRL") -> bytes:
    return struct.pack(PACKET_FMT_V0_ODO, magic, agent, x, y, yaw, enc, v2v, scan_count, *ranges)


def pack_sweeps(agent, x, y, yaw, ranges, enc=None, v2v=None, odometry=True, scan_count=SWEEP_BEAMS) -> np.ndarray:
    """Vectorised packer: arrays (ranges [n, 181]) -> uint8 [n, 751] (odometry) or [n, 743]."""
    n = len(agent)
    rec = np.zeros(n, dtype=PACKET_DTYPE_V0_ODO if odometry else PACKET_DTYPE_V0)
    rec["magic"] = b"QSRL"
    rec["agent"], rec["x"], rec["y"], rec["yaw"] = agent, x, y, yaw
    if odometry:
        rec["enc"] = 0 if enc is None else enc
        rec["v2v"] = 0 if v2v is None else v2v
    rec["scan_count"] = scan_count
    rec["ranges"] = np.asarray(ranges, dtype=np.float32).reshape(n, SWEEP_BEAMS)
    return rec.view(np.uint8).reshape(n, rec.dtype.itemsize)


def unpack_v0_odo(data: bytes):
    """None unless the size and magic match; else (agent, x, y, yaw, encoder, v2v, ranges[181])."""
    if len(data) != PACKET_SIZE_V0_ODO:
        return None
    rec = np.frombuffer(data, dtype=PACKET_DTYPE_V0_ODO)[0]
    if rec["magic"] != b"QSRL":
        return None
    return (int(rec["agent"]), float(rec["x"]), float(rec["y"]), float(rec["yaw"]), int(rec["enc"]), int(rec["v2v"]),
            rec["ranges"].copy())


def unpack_v0(data: bytes):
    """udp_bridge.py:53-75: None unless the size and magic match; else (agent, x, y, yaw, ranges[181])."""
    if len(data) != PACKET_SIZE_V0:
        return None
    rec = np.frombuffer(data, dtype=PACKET_DTYPE_V0)[0]
    if rec["magic"] != b"QSRL":
        return None
    return int(rec["agent"]), float(rec["x"]), float(rec["y"]), float(rec["yaw"]), rec["ranges"].copy()


def pack_cmd(linear_x, angular_z) -> bytes:
    """udp_bridge.py:140-146."""
    return struct.pack(CMD_FMT, b"CMD1", linear_x, angular_z)
