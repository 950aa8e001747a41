"""Built inputs for the tile-binned raycast (csrc/raycast_tiled.hip, raycast_tiled.h, raycast_common.h; sweep.hip's pass A):
streams in which every ray is placed on one of the kernels' edges -- the 64-cell bin / direct threshold, the 2 x 2 tile box,
the i8 tile-relative records, truncation toward zero at the grid's near edge, partial tiles, the raster's 2048-record items and
512-record rounds, the 16-bit LDS counters, the persistent raster runs, the pass A / C decomposition, arrival order.

Everything is exact in f32: resolutions are powers of two, origins -size * res / 2, poses on cell centres, axis ranges k * res.
    S  res = 1/16   a 1.2 m ray is 19.2 cells
    L  res = 1/64   a 1.2 m ray is 76.8 cells; front distances k / 64, k = 4..76, are valid rays of exactly k cells
    F  res = 1/128  a 1.2 m ray is 153.6 cells.  Only for the oblique threshold rays: a ray of (63, 63) cells is 89.1 cells
                    long, longer than any ray of L under the default 1.2 m trust filter
End points are at least MARGIN of a cell from every cell edge (asserted per scene in test_ray_scenes_cpu.py), so the
exact-trig mode defers nothing to the host and the device kernels decide every ray.

`restate` is an integer restatement of what passes A to D see for a scene (grid end points, bin / direct, records and items
per tile, workgroups).  It is computed from the oracle's poses and end cells and is used ONLY to prove that a scene reaches the
case it is named for -- never as an expected map: the expected map is always the oracle's.

No GPU, numpy only."""
import functools
import importlib
import math

import numpy as np

from conftest import PKG_NAME
from oracle import oracle as orc

TILE, CHUNK, FLUSH_ITEMS = 64, 2048, 31                      # raycast_tiled.h / .hip: QT_TILE, QT_CHUNK, QT_FLUSH_ITEMS
MAX_WG, SCAN_SEGS, RASTER_WGS = 512, 16, 1024                # QT_MAX_WG, QT_SCAN_SEGS, QT_RASTER_WGS
SWEEP_SLOTS = 184                                            # ray slots of one sweep (181 beams + 3 empty)
MIN_D, MAX_D = 0.05, 1.2                                     # the packet trust filter
SMIN_D, SMAX_D = 0.1, 1.2                                    # the sweep trust filter
MARGIN = 1e-3                                                # cells: least distance of any end point from a cell edge
SENSOR_ANG = (0.0, math.pi / 2, math.pi, -math.pi / 2)       # front, left, back, right
YAW4 = tuple(np.float32(v) for v in (0.0, math.pi / 2, math.pi, -math.pi / 2))    # +x, +y, -x, -y
DIR4 = ((1, 0), (0, 1), (-1, 0), (0, -1))
RES = {"S": 1.0 / 16, "L": 1.0 / 64, "F": 1.0 / 128}
SHORT = {"S": 1, "L": 4, "F": 7}                             # cells of the shortest valid distance (> 0.05 m)


def _P():
    return importlib.import_module(PKG_NAME + ".protocol")


class Geo:
    def __init__(self, kind, size):
        self.kind, self.size, self.res = kind, size, RES[kind]
        self.ox = self.oy = -size * self.res / 2
        self.short = SHORT[kind]
        self.tiles_x = (size + TILE - 1) // TILE
        self.n_tiles = self.tiles_x * self.tiles_x

    def oracle(self, max_agent=2):
        return orc.OracleMapper(self.size, self.res, self.ox, self.oy, 0.0, max_agent=max_agent)

    def at_q(self, q):
        """World coordinate of grid quotient q (cells from the origin), which must be exact in f32."""
        w = self.ox + np.asarray(q, dtype=np.float64) * self.res
        f = w.astype(np.float32)
        assert (f.astype(np.float64) == w).all(), "pose not exact in f32"
        return f

    def centre_q(self, c):
        """Quotient of the centre of cell c under int((w - o) / res), which truncates toward zero: cell c >= 0 is
        q in [c, c + 1) with centre c + 0.5, cell c < 0 is q in (c - 1, c] with centre c - 0.5.  (q = -0.5 is column 0.)"""
        c = np.asarray(c, dtype=np.int64)
        return np.where(c >= 0, c + 0.5, c - 0.5)

    def dist(self, k):
        """f32 distance of exactly k cells; k = 0: an invalid distance (0.0 <= 0.05 m), i.e. a full-length free ray."""
        return (np.asarray(k, dtype=np.float64) * self.res).astype(np.float32)


class Scene:
    def __init__(self, name, geo, kind, data, tags, meta=None, max_agent=2):
        self.name, self.geo, self.kind, self.data, self.tags = name, geo, kind, data, tags
        self.meta = meta or {}
        self.max_agent = max_agent


class _Rows:
    """Accumulates packets: pose quotients (qx, qy), f32 yaw, four f32 distances, agent, magic, a tag per packet."""

    def __init__(self, geo):
        self.geo = geo
        self.cols = [[] for _ in range(7)]

    def extend(self, qx, qy, yaw, d4, agent=1, magic=True, tag=""):
        qx = np.atleast_1d(np.asarray(qx, dtype=np.float64))
        n = len(qx)
        vals = (qx, np.broadcast_to(np.asarray(qy, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(yaw, dtype=np.float32), (n,)),
                np.broadcast_to(np.asarray(d4, dtype=np.float32), (n, 4)), np.broadcast_to(np.asarray(agent, dtype=np.uint8), (n,)),
                np.broadcast_to(np.asarray(magic, dtype=bool), (n,)), np.broadcast_to(np.asarray(tag, dtype=object), (n,)))
        for col, v in zip(self.cols, vals):
            col.append(np.array(v))

    def cell(self, cx, cy, yaw, k_front, others=None, tag="", raw_front=None, **kw):
        """One packet (or arrays of them) posed on the centre of cell (cx, cy); front ray of k_front cells (or the raw f32
        distance raw_front), the three other sensors the shortest valid distance unless given."""
        g = self.geo
        cx = np.atleast_1d(np.asarray(cx, dtype=np.int64))
        n = len(cx)
        d4 = np.empty((n, 4), dtype=np.float32)
        d4[:, 0] = g.dist(k_front) if raw_front is None else raw_front
        d4[:, 1:] = g.dist(g.short if others is None else others)
        self.extend(g.centre_q(cx), g.centre_q(np.broadcast_to(np.asarray(cy, dtype=np.int64), (n,))), yaw, d4, tag=tag, **kw)

    def aim(self, cx, cy, tx, ty, tag=""):
        """One packet on the centre of cell (cx, cy) whose front ray is a hit on the centre of cell (tx, ty); returns the yaw."""
        g = self.geo
        dqx, dqy = float(g.centre_q(tx) - g.centre_q(cx)), float(g.centre_q(ty) - g.centre_q(cy))
        yaw = np.float32(math.atan2(dqy, dqx))
        self.cell(cx, cy, yaw, 0, raw_front=np.float32(math.hypot(dqx, dqy) * g.res), tag=tag)
        return yaw

    def scene(self, name, meta=None):
        g, P = self.geo, _P()
        qx, qy, yaw, d4, agent, magic, tags = (np.concatenate(c) for c in self.cols)
        x, y = g.at_q(qx), g.at_q(qy)
        # the cells of the poses come from the oracle's world_to_grid, never from floor
        o = g.oracle()
        want_x, want_y = np.trunc(qx).astype(np.int64), np.trunc(qy).astype(np.int64)
        assert (o.world_to_grid(x.astype(np.float64), 0) == want_x).all() and (o.world_to_grid(y.astype(np.float64), 1) == want_y).all()
        n = len(x)
        buf = P.pack_packets(agent, x, y, yaw, np.zeros(n, np.int32), np.zeros(n, np.uint32), d4, np.zeros(n, np.uint8)).copy()
        buf[~magic, 0] = ord("X")
        return Scene(name, g, "packets", buf, tags, meta)


# ---- the restatement -----------------------------------------------------------------------------------------------------
def bresenham(x0, y0, x1, y1):
    """dual_bot_mapper.py:158-179 in integers (checked against oracle.bresenham in test_ray_scenes_cpu.py)."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err, out = dx - dy, []
    while True:
        out.append((x0, y0))
        if x0 == x1 and y0 == y1:
            return out
        e2 = 2 * err
        if e2 > -dy:
            err -= dy; x0 += sx
        if e2 < dx:
            err += dx; y0 += sy


def packet_decomposition(n):
    """Pass A / C of the 4-ray path: packets per workgroup, workgroups, rows per thread of the table scan (R)."""
    per = (n + MAX_WG - 1) // MAX_WG
    per = 256 if per < 256 else (per + 63) // 64 * 64
    nwg = (n + per - 1) // per
    return per, nwg, (nwg + SCAN_SEGS - 1) // SCAN_SEGS


def sweep_decomposition(n):
    per = (n + MAX_WG - 1) // MAX_WG
    per = (per + 15) // 16 * 16
    nwg = (n + per - 1) // per
    return per, nwg, (nwg + SCAN_SEGS - 1) // SCAN_SEGS


class Restated:
    """Rays of one ingest as the tiled passes see them.  All arrays are per live ray (a ray of an accepted record), in arrival
    order; `slot` is the ray's slot in the ingest (4 per packet, 184 per sweep)."""

    def __init__(self, geo, slot, n_slots, x0, y0, x1, y1, valid, margin):
        size = geo.size
        self.geo, self.slot, self.n_slots = geo, slot, n_slots
        self.x0, self.y0, self.x1, self.y1, self.valid, self.margin = x0, y0, x1, y1, valid, margin
        xlo, xhi, ylo, yhi = np.minimum(x0, x1), np.maximum(x0, x1), np.minimum(y0, y1), np.maximum(y0, y1)
        self.dx, self.dy = xhi - xlo, yhi - ylo
        self.inbox = (xhi >= 0) & (yhi >= 0) & (xlo < size) & (ylo < size)          # qs_line_setup
        self.binned = self.inbox & (self.dx < TILE) & (self.dy < TILE)              # qt_ray_bin
        self.direct = self.inbox & ~self.binned
        # qt_tile_range: the tile box after clamping to the grid
        self.tx_lo, self.tx_hi = np.clip(xlo, 0, size - 1) >> 6, np.clip(xhi, 0, size - 1) >> 6
        self.ty_lo, self.ty_hi = np.clip(ylo, 0, size - 1) >> 6, np.clip(yhi, 0, size - 1) >> 6
        ray, tile, off = [], [], []
        idx = np.arange(len(x0))
        for q in range(4):
            tx, ty = self.tx_lo + (q & 1), self.ty_lo + (q >> 1)
            ok = self.binned & (tx <= self.tx_hi) & (ty <= self.ty_hi)
            ray.append(idx[ok]); tile.append((ty * geo.tiles_x + tx)[ok])
            off.append(np.stack([x0[ok] - 64 * tx[ok], y0[ok] - 64 * ty[ok], x1[ok] - 64 * tx[ok], y1[ok] - 64 * ty[ok]], axis=1))
        ray, tile, off = np.concatenate(ray), np.concatenate(tile), np.concatenate(off)
        order = np.argsort(ray, kind="stable")                                      # records in arrival order of their rays
        self.rec_ray, self.rec_tile, self.rec_off = ray[order], tile[order], off[order]
        self.tile_count = np.bincount(self.rec_tile, minlength=geo.n_tiles)
        self.items = (self.tile_count + CHUNK - 1) // CHUNK
        self.chunk_base = np.concatenate([[0], np.cumsum(self.items)])
        self.n_items = int(self.items.sum())

    def tile(self, tx, ty):
        return ty * self.geo.tiles_x + tx

    def tile_records(self, t):
        """Rays with a record in tile t, in arrival order: position p is record p of the tile, up to pass C's own scheduling
        inside one workgroup (slots are handed out by LDS atomics)."""
        return self.rec_ray[self.rec_tile == t]

    def cells(self, r):
        return bresenham(int(self.x0[r]), int(self.y0[r]), int(self.x1[r]), int(self.y1[r]))

    def written_cells(self, r):
        """In-grid cells ray r writes: every cell but the last is free, the last is occupied iff the hit is valid."""
        c = self.cells(r)
        if not self.valid[r]:
            c = c[:-1]
        s = self.geo.size
        return [(x, y) for x, y in c if 0 <= x < s and 0 <= y < s]

    def cellless_records(self):
        """(ray, tile) of records in a tile in which the ray has no cell at all (in or out of the grid)."""
        out = []
        for r in np.unique(self.rec_ray):
            tiles = self.rec_tile[self.rec_ray == r]
            if len(tiles) < 3:
                continue                                                            # 1 x 1, 1 x 2 and 2 x 1 boxes are filled
            have = {(y >> 6) * self.geo.tiles_x + (x >> 6) for x, y in self.cells(r) if x >= 0 and y >= 0}
            out += [(int(r), int(t)) for t in tiles if int(t) not in have]
        return out

    def raster_wgs(self, env_wgs=RASTER_WGS):
        """qt_launch_sort_raster's workgroup count."""
        max_items = min(4 * self.n_slots // CHUNK + self.geo.n_tiles + 8, 4 * self.n_slots)
        return min(max_items, env_wgs)

    def raster_runs(self, env_wgs=RASTER_WGS):
        """Per raster workgroup with work: the list of (tile, items of it in this run, excl) in the order it rasters them."""
        wgs = self.raster_wgs(env_wgs)
        per = (self.n_items + wgs - 1) // wgs
        item_tile = np.repeat(np.arange(self.geo.n_tiles), self.items)
        runs = []
        for w in range(wgs):
            first, last = w * per, min((w + 1) * per, self.n_items)
            if first >= last:
                break
            run = []
            for t in item_tile[first:last]:
                if run and run[-1][0] == int(t):
                    run[-1][1] += 1
                else:
                    run.append([int(t), 1, bool(self.chunk_base[t] >= first and self.chunk_base[t + 1] <= last)])
            runs.append([tuple(v) for v in run])
        return runs


def accepted_mask(scene):
    rec = scene.data.view(_P().PACKET_DTYPE).reshape(-1)
    return (rec["magic"] == b"QSRL") & (rec["agent"] >= 1) & (rec["agent"] <= scene.max_agent)


def feed_oracle(scene):
    """The oracle fed the scene's bytes.  Sweeps: the beams of `sweep_beams` through update_rays."""
    o = scene.geo.oracle(scene.max_agent)
    if scene.kind == "packets":
        o.feed_stream(scene.data)
    else:
        o.update_rays(*sweep_beams(scene)[:5])
    return o


def _margin(geo, ex, ey):
    qx, qy = (ex - geo.ox) / geo.res, (ey - geo.oy) / geo.res
    return np.minimum(np.abs(qx - np.rint(qx)), np.abs(qy - np.rint(qy)))


def sweep_beams(scene, smin=SMIN_D, smax=SMAX_D):
    """(rx, ry, hx, hy, valid, slot) of every beam of every acceptable record, in order: include/quasar_slam.h's sweep rule
    with Python's math.cos / math.sin, as tests/test_gpu_sweeps.py::_beams."""
    P = _P()
    recs = np.ascontiguousarray(scene.data).view(P.PACKET_DTYPE_V0_ODO).reshape(-1)
    out = ([], [], [], [], [], [])
    for k, r in enumerate(recs):
        if r["magic"] != b"QSRL" or not 1 <= int(r["agent"]) <= scene.max_agent:
            continue
        px, py, yaw = float(r["x"]), float(r["y"]), float(r["yaw"])
        for i, d in enumerate(r["ranges"].tolist()):
            a = yaw + math.radians(i - 90)
            ok = smin < d <= smax
            L = d if ok else (min(d, smax) if d > smin else smax)
            for col, v in zip(out, (px, py, px + L * math.cos(a), py + L * math.sin(a), 1 if ok else 0, SWEEP_SLOTS * k + i)):
                col.append(v)
    return [np.array(v, dtype=np.float64) for v in out[:4]] + [np.array(out[4], dtype=np.uint8), np.array(out[5], dtype=np.int64)]


def restate(scene, o=None, lo=0, hi=None):
    """The restatement of one ingest of records [lo, hi) of the scene, from the oracle's poses and its world_to_grid."""
    geo = scene.geo
    o = o or feed_oracle(scene)
    if scene.kind == "sweeps":
        rx, ry, hx, hy, valid, slot = sweep_beams(scene)
        n_slots = SWEEP_SLOTS * len(scene.data)
    else:
        acc = accepted_mask(scene)
        poses = o.poses
        assert len(poses) == int(acc.sum())
        rec = scene.data.view(_P().PACKET_DTYPE).reshape(-1)[acc]
        d = np.stack([rec[k] for k in ("front", "left", "back", "right")], axis=1).astype(np.float64)
        ok = (MIN_D < d) & (d <= MAX_D)
        rng = np.where(ok, d, np.where(d > MIN_D, np.minimum(d, MAX_D), MAX_D))
        a = poses[:, 2:3] + np.array(SENSOR_ANG)[None, :]
        rx, ry = np.repeat(poses[:, 0], 4), np.repeat(poses[:, 1], 4)
        hx, hy = rx + (rng * np.cos(a)).reshape(-1), ry + (rng * np.sin(a)).reshape(-1)
        valid = ok.reshape(-1).astype(np.uint8)
        slot = (4 * np.nonzero(acc)[0][:, None] + np.arange(4)[None, :]).reshape(-1)
        n_slots = 4 * len(scene.data)
    hi = n_slots if hi is None else hi
    keep = (slot >= lo) & (slot < hi)
    x0, y0 = o.world_to_grid(rx, 0), o.world_to_grid(ry, 1)
    x1, y1 = o.world_to_grid(hx, 0), o.world_to_grid(hy, 1)
    m = _margin(geo, hx, hy)
    return Restated(geo, slot[keep] - lo, hi - lo, x0[keep], y0[keep], x1[keep], y1[keep], valid[keep].astype(bool), m[keep])


def sweep_stamps_reference(scene):
    """Stamps of a sweeps scene: last writer wins over (ordinal << 1) | occ with ordinal = slot + 1, the cells of every beam
    from oracle.bresenham over the oracle's world_to_grid (update_rays itself stamps every beam alike)."""
    geo = scene.geo
    o = geo.oracle(scene.max_agent)
    rx, ry, hx, hy, valid, slot = sweep_beams(scene)
    x0, y0, x1, y1 = o.world_to_grid(rx, 0), o.world_to_grid(ry, 1), o.world_to_grid(hx, 0), o.world_to_grid(hy, 1)
    st = np.zeros((geo.size, geo.size), dtype=np.uint32)
    for i in range(len(slot)):
        cells = orc.bresenham(int(x0[i]), int(y0[i]), int(x1[i]), int(y1[i]))
        key = (int(slot[i]) + 1) << 1
        last = len(cells) - 1
        for j, (x, y) in enumerate(cells.tolist()):
            if (j < last or valid[i]) and 0 <= x < geo.size and 0 <= y < geo.size:
                st[y, x] = max(st[y, x], key | (1 if j == last else 0))
    return st


# ---- oblique rays: (yaw, d) as f32, found once by `search_oblique` and stored ----------------------------------------------
def oblique_ok(geo, cx, cy, yaw, d, dx, dy):
    """Does the front ray of a pose on cell (cx, cy) end (dx, dy) cells away, its end point >= MARGIN from every cell edge?"""
    o = geo.oracle()
    rx, ry = float(geo.at_q(geo.centre_q(cx))), float(geo.at_q(geo.centre_q(cy)))
    d = float(np.float32(d)); a = float(np.float32(yaw))
    if not MIN_D < d <= MAX_D:
        return False
    ex, ey = rx + d * math.cos(a), ry + d * math.sin(a)
    got = (int(o.world_to_grid([ex], 0)[0]) - cx, int(o.world_to_grid([ey], 1)[0]) - cy)
    return got == (dx, dy) and float(_margin(geo, np.array([ex]), np.array([ey]))[0]) >= MARGIN


def search_oblique(geo, cx, cy, dx, dy, seed=20):
    """Seeded search for an f32 (yaw, d) whose front ray from cell (cx, cy) ends (dx, dy) cells away: the criterion is the
    oracle's end cell, kept only if the end point is >= MARGIN of a cell from every cell edge."""
    rng = np.random.default_rng(seed + 1000 * dx + dy)
    for _ in range(10000):
        yaw = np.float32(math.atan2(dy, dx) + rng.uniform(-0.004, 0.004))
        d = np.float32((math.hypot(dx, dy) + rng.uniform(-0.3, 0.3)) * geo.res)
        if oblique_ok(geo, cx, cy, yaw, d, dx, dy):
            return float(yaw), float(d)
    raise AssertionError("no oblique ray found")


OBLIQUE_POSE = (2, 2)
OBLIQUE = {   # (geometry, dx, dy) -> (yaw, d) as f32 values; found by search_oblique(Geo(kind, 132), 2, 2, dx, dy)
    ("L", 64, 1): (0.018917270004749298, 0.9991832375526428),
    ("L", 1, 64): (1.5579079389572144, 0.9959262013435364),
    ("F", 63, 63): (0.786165714263916, 0.694570004940033),
    ("F", 63, 62): (0.7738298177719116, 0.6906788945198059),
    ("F", 64, 1): (0.018917270004749298, 0.4995916187763214),
    ("F", 1, 64): (1.5579079389572144, 0.4979631006717682),
    ("F", 63, 64): (0.7909176349639893, 0.7021424174308777),
}


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def _threshold(kind):
    g = Geo(kind, 132)
    rows = _Rows(g)
    row = 3
    for k in (62, 63, 64, 65):
        for h, (ux, uy) in enumerate(DIR4):
            for c in (0, 1, 63, 64, 65):
                # the ray covers columns (rows) c .. c + k, walked in the heading's direction
                start = c if ux + uy > 0 else c + k
                cx, cy = (start, 8 + row % 116) if ux else (8 + row % 116, start)
                rows.cell(cx, cy, YAW4[h], k, tag=f"axis k={k} h={h} c={c}")
                row += 3
    for (kd, dx, dy), (yaw, d) in OBLIQUE.items():
        if kd == kind:
            rows.cell(OBLIQUE_POSE[0], OBLIQUE_POSE[1], np.float32(yaw), 0, raw_front=np.float32(d), tag=f"oblique {dx},{dy}")
    return rows.scene("threshold-" + kind)


CORNER_YAWS = tuple(np.float32(v) for v in (0.0, math.pi / 2, math.pi, -math.pi / 2, math.pi / 4, 3 * math.pi / 4, -3 * math.pi / 4,
                                            -math.pi / 4, math.atan2(1, 2), math.atan2(-2, -1)))


def _corner():
    g = Geo("S", 132)
    rows = _Rows(g)
    cy, cx = np.meshgrid(np.arange(61, 67), np.arange(61, 67), indexing="ij")
    for k in (4, 11, 19):
        for yaw in CORNER_YAWS:
            rows.cell(cx.reshape(-1), cy.reshape(-1), yaw, k, tag=f"k={k}")
    return rows.scene("corner")


def _edges(kind, size):
    g = Geo(kind, size)
    rows = _Rows(g)
    kmax = 63 if kind == "L" else 19                  # longest binned (L) / longest valid (S) ray
    kfar = 63 if kind == "L" else 17                  # ... and the longest whose oblique ray (kfar, 2) is still a valid distance
    last = size - 1
    along = (3, size // 2, size - 4)

    def side_pose(side, depth, a):
        """Cell `depth` cells outside (negative: inside) side 0..3 = left, bottom, right, top at position a along it; the
        heading that points into the grid."""
        if side == 0:
            return -depth, a, 0
        if side == 1:
            return a, -depth, 1
        if side == 2:
            return last + depth, a, 2
        return a, last + depth, 3

    for side in range(4):
        for i, m in enumerate((g.short, g.short + 4, kmax)):
            a = along[i]
            cx, cy, h = side_pose(side, m, a)
            rows.cell(cx, cy, YAW4[h], m, tag="out-in hit on the edge cell")               # ends on cell 0 / size-1: q = -0.5 side
            rows.cell(cx, cy, YAW4[h], min(m + 3, 76 if kind == "L" else 19), tag="out-in hit inside")
            if m - 1 >= g.short:
                rows.cell(cx, cy, YAW4[h], m - 1, tag="both out: ends one cell short")      # cell -1 / size: no box
            rows.cell(cx, cy, YAW4[h], 0, tag="out-in free")
        cx, cy, h = side_pose(side, -2, along[1] + 1)
        rows.cell(cx, cy, YAW4[(h + 2) % 4], 5, tag="in-out: hit not written")
        rows.cell(cx, cy, YAW4[(h + 2) % 4], 2, tag="in-in: hit on the edge cell")
    # corners: poses outside two sides at once, and a diagonal past each corner with both ends out and no cell in the grid
    for sx, sy in ((0, 0), (1, 0), (1, 1), (0, 1)):
        ex = last + 4 if sx else -4
        iy = last - 1 if sy else 1
        # from (ex, iy) to (jx, jy): a 4-cell diagonal whose cells all lie outside the grid, its bounding box overlapping it
        jx, jy = (last if sx else 0), (last + 3 if sy else -3)
        rows.aim(ex, iy, jx, jy, tag="past the corner: box overlaps, no cell")
        cx, cy = (last + 3 if sx else -3), (last + 3 if sy else -3)
        tx, ty = (last - 2 if sx else 2), (last - 2 if sy else 2)
        yaw = rows.aim(cx, cy, tx, ty, tag="corner out-in diagonal")
        rows.cell(cx, cy, yaw, 0, tag="corner out-in free diagonal")
        # outside both sides, an axis ray that stays outside on the other axis
        rows.cell(cx, cy, YAW4[2 if sx else 0], 5, tag="corner: axis ray stays out")
        # as far outside a corner as a ray still reaches it: a hit on the corner cell from kfar cells out on one axis, 2 on the other
        fx, fy = (last + kfar if sx else -kfar), (last + 2 if sy else -2)
        gx, gy = (last + 2 if sx else -2), (last + kfar if sy else -kfar)
        rows.aim(fx, fy, last if sx else 0, last if sy else 0, tag="far corner out-in x")
        rows.aim(gx, gy, last if sx else 0, last if sy else 0, tag="far corner out-in y")
    # poses at q = -1.5, -0.5, +0.5 (near edge) and size - 0.5, size + 0.5 (far edge) on both axes
    mid = g.centre_q(size // 2 - 2)
    for q in (-1.5, -0.5, 0.5, size - 0.5, size + 0.5):
        for h in range(4):
            d4 = g.dist([g.short + 2, g.short, g.short + 1, g.short])
            rows.extend(q, mid, YAW4[h], d4, tag=f"pose qx={q}")
            rows.extend(mid + 3, q, YAW4[h], d4, tag=f"pose qy={q}")
    for q in (-1.5, -0.5, 0.5):
        rows.extend(q, q, YAW4[0], g.dist([g.short + 2] * 4), tag=f"pose qx=qy={q}")
    if kind == "L" and size == 128:
        # the i8 record extremes: x1 = 127 from x0 = 190 is offset +126 in the last tile; x0 = -63 to x1 = 0 is -63
        rows.cell(190, 100, YAW4[2], 63, tag="offset +126 x")
        rows.cell(100, 190, YAW4[3], 63, tag="offset +126 y")
        rows.cell(-63, 27, YAW4[0], 63, tag="offset -63 x")
        rows.cell(27, -63, YAW4[1], 63, tag="offset -63 y")
    return rows.scene(f"edges-{kind}-{size}")


ORDER_CELL = (20, 30)                                 # the contested cell of the `order` scenes
ORDER_N = 1100


def _order(variant, last_is_hit):
    """One cell alternately occupied (packet A: front hit of 5 cells ends on it) and free (packet B: front hit of 9 cells
    crosses it).  4 records per packet, all in tile 0: 1100 packets are 4400 records = 3 chunks.
    adjacent: A and B alternate to the end; the last two packets are records 4392.. 4399 of the tile, one 8-record group.
    chunks:   A and B alternate over packets 0..399 (chunk 0), then fillers on another row; the last packet writes the cell
              again from chunk 2."""
    g = Geo("S", 64)
    rows = _Rows(g)
    cx, cy = ORDER_CELL[0] - 5, ORDER_CELL[1]
    p = np.arange(ORDER_N)
    hit = (p % 2 == 1) == last_is_hit                  # packet 1099 is a hit iff last_is_hit
    if variant == "chunks":
        hit[:400] = ~hit[:400]                          # packet 399, the last writer before the fillers, is the opposite of the last
    k = np.where(hit, 5, 9)
    if variant == "chunks":
        filler = (p >= 400) & (p < ORDER_N - 1)
        ky = np.where(filler, cy + 4 + p % 7, cy)
    else:
        ky = np.full(ORDER_N, cy)
    d4 = np.stack([g.dist(k), g.dist(np.ones(ORDER_N)), g.dist(np.ones(ORDER_N)), g.dist(np.ones(ORDER_N))], axis=1)
    rows.extend(g.centre_q(np.full(ORDER_N, cx)), g.centre_q(ky), YAW4[0], d4, tag="order")
    return rows.scene(f"order-{variant}-{'hit' if last_is_hit else 'free'}", meta={"variant": variant, "last_is_hit": last_is_hit})


UNITS_N = (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097)


def _units(n):
    """Pose 4 cells left of the border between tiles (0,0) and (1,0); the front ray (8 cells) is the only one that crosses:
    tile (1,0) gets one record per packet, tile (0,0) four."""
    g = Geo("S", 128)
    rows = _Rows(g)
    p = np.arange(n)
    rows.cell(np.full(n, 60), 10 + 3 * (p % 5), YAW4[0], np.where(p % 3 == 2, 0, 8), tag="units")
    return rows.scene(f"units-{n}", meta={"n": n})


COUNTERS_N = 16385
COUNTERS_POSE = (30, 30)


def _counters():
    """16385 packets from one pose: the pose cell takes 4 misses per packet = 65540 > 65535, all in one tile = 33 items."""
    g = Geo("S", 64)
    rows = _Rows(g)
    p = np.arange(COUNTERS_N)
    rows.cell(np.full(COUNTERS_N, COUNTERS_POSE[0]), COUNTERS_POSE[1], YAW4[0], np.where(p % 2 == 0, 6, 0), others=2, tag="counters")
    return rows.scene("counters")


RUNS_TILES = {"first": (0, 0), "partial_x": (8, 3), "middle": (4, 4), "last_full": (7, 7), "partial_y": (3, 8), "partial_xy": (8, 8)}
RUNS_MIDDLE_N = 600


def _runs():
    """520 = 8 full tiles + an 8-cell partial tile per axis.  Records only in six tiles; the middle one has 2400 = 2 items."""
    g = Geo("S", 520)
    rows = _Rows(g)
    for name, (tx, ty) in RUNS_TILES.items():
        n = RUNS_MIDDLE_N if name == "middle" else 12
        p = np.arange(n)
        w = 8 if tx == 8 else 64
        h = 8 if ty == 8 else 64
        # poses at least 2 cells inside the tile so the 1-cell side rays stay in it; the front ray (2 or 3 cells) too
        cx = 64 * tx + 2 + p % (w - 5)
        cy = 64 * ty + 2 + (p // 7) % (h - 5)
        rows.cell(cx, cy, YAW4[0], 2 + p % 2, tag=name)
    # partial tiles: rays that leave the grid over the far edge (hit not written) and a free ray that runs off it
    rows.cell(515, 200, YAW4[0], 9, tag="partial_x leaves")
    rows.cell(200, 515, YAW4[1], 0, tag="partial_y leaves free")
    return rows.scene("runs")


DECOMP_N = (255, 256, 257, 4096, 4097, 131072, 131073)


def _decomp(n):
    """Poses walk all four tiles of a 128-cell grid, hit and free fronts alternate; rejected packets (bad magic; agent 0) at
    slots 255, 256 and the last."""
    g = Geo("S", 128)
    rows = _Rows(g)
    p = np.arange(n)
    t = p % 4
    step = p // 4
    cx = 64 * (t & 1) + 8 + step % 48
    cy = 64 * (t >> 1) + 8 + (step // 48) % 48
    yaw = np.array(YAW4, dtype=np.float32)[(p // 7) % 4]
    k = np.where(p % 2 == 0, 5 + p % 3, 0)
    d4 = np.stack([g.dist(k), g.dist(1 + p % 2), g.dist(np.ones(n)), g.dist(1 + (p // 2) % 3)], axis=1)
    magic = np.ones(n, dtype=bool)
    agent = np.ones(n, dtype=np.uint8)
    bad = sorted({s for s in (255, 256, n - 1) if s < n})
    for j, s in enumerate(bad):
        if j % 2 == 0:
            magic[s] = False
        else:
            agent[s] = 0
    rows.extend(g.centre_q(cx), g.centre_q(cy), yaw, d4, agent=agent, magic=magic, tag="decomp")
    return rows.scene(f"decomp-{n}", meta={"n": n, "rejected": bad})


MANY_TILES = (0, 1023, 1024, 1025, 1087, 1088)


def _many_tiles():
    """2052 = 32 full tiles + one 4-cell partial tile per axis (grid sizes are multiples of 4, so 4 x 4 is the smallest
    partial tile there is): 33 x 33 = 1089 tiles, so pass B2 scans 2 tiles per thread; tile 1088 is the 4 x 4 corner."""
    g = Geo("S", 2052)
    rows = _Rows(g)
    for t in MANY_TILES:
        tx, ty = t % 33, t // 33
        for j in range(5):
            cx = 64 * tx + (j % 4 if tx == 32 else 3 + 11 * j)
            cy = 64 * ty + ((j + 1) % 4 if ty == 32 else 5 + 9 * j)
            rows.cell(cx, cy, YAW4[j % 4], 3 + j, others=1 + j % 2, tag=f"tile {t}")
    return rows.scene("many_tiles")


SWEEPS_N = (1, 15, 16, 17)
SWEEP_CELLS = ((63, 63), (64, 63), (63, 64), (64, 64))


def _sweep_ranges(g, px, py, yaw, cand):
    """Per beam the first candidate length (cells) whose end point is >= MARGIN from every cell edge."""
    out = np.zeros(181, dtype=np.float32)
    for i in range(181):
        a = float(yaw) + math.radians(i - 90)
        for j in range(len(cand)):
            k = cand[(i + j) % len(cand)]
            d = float(g.dist(k))
            L = d if SMIN_D < d <= SMAX_D else SMAX_D
            ex, ey = px + L * math.cos(a), py + L * math.sin(a)
            if float(_margin(g, np.array([ex]), np.array([ey]))[0]) >= MARGIN:
                out[i] = d
                break
        else:
            raise AssertionError(f"beam {i}: no candidate keeps clear of the cell edges")
    return out


def _sweeps(kind, n):
    """Built sweeps posed on the four cells round (64, 64), yaw a multiple of pi / 2, ranges k * res.  L: beams of 63 and 64
    cells (binned / direct), a few invalid ones (full-length free beams: 76.8 cells, direct).  One rejected record if n > 1."""
    g = Geo(kind, 132)
    P = _P()
    cand = (63, 64, 63, 64, 0) if kind == "L" else (19, 7, 12, 2, 0, 16)
    xs, ys, yaws, ranges = [], [], [], []
    for k in range(n):
        cx, cy = SWEEP_CELLS[k % 4]
        x, y = float(g.at_q(g.centre_q(cx))), float(g.at_q(g.centre_q(cy)))
        yaw = YAW4[(k // 4) % 4]
        xs.append(x); ys.append(y); yaws.append(yaw)
        ranges.append(_sweep_ranges(g, x, y, yaw, cand[k % len(cand):] + cand[:k % len(cand)]))
    agent = np.ones(n, dtype=np.uint8)
    buf = P.pack_sweeps(agent, np.array(xs, np.float32), np.array(ys, np.float32), np.array(yaws, np.float32), np.array(ranges)).copy()
    rejected = None
    if n > 1:
        rejected = n // 2
        buf[rejected, 0] = ord("X")
    return Scene(f"sweeps-{kind}-{n}", g, "sweeps", buf, np.full(n, "sweep", dtype=object), meta={"n": n, "rejected": rejected})


EDGE_GEOMETRIES = tuple((kind, size) for kind in ("L", "S") for size in (64, 68, 128, 132))   # 130 is no grid size: sizes are multiples of 4

BUILDERS = {"threshold-L": lambda: _threshold("L"), "threshold-F": lambda: _threshold("F"), "corner": _corner,
            "counters": _counters, "runs": _runs, "many_tiles": _many_tiles}
BUILDERS.update({f"edges-{k}-{s}": (lambda k=k, s=s: _edges(k, s)) for k, s in EDGE_GEOMETRIES})
BUILDERS.update({f"order-{v}-{'hit' if h else 'free'}": (lambda v=v, h=h: _order(v, h)) for v in ("adjacent", "chunks") for h in (True, False)})
BUILDERS.update({f"units-{n}": (lambda n=n: _units(n)) for n in UNITS_N})
BUILDERS.update({f"decomp-{n}": (lambda n=n: _decomp(n)) for n in DECOMP_N})
BUILDERS.update({f"sweeps-{k}-{n}": (lambda k=k, n=n: _sweeps(k, n)) for k in ("S", "L") for n in SWEEPS_N})


def names(prefix=""):
    return [k for k in BUILDERS if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()
