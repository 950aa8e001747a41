"""The bot veil (include/quasar_slam.h, rules V1-V7) restated with plain loops, and the built streams its tests use.

`VeilModel` takes from oracle.OracleMapper the accepted packets, their poses after drift, the cells through the oracle's
world_to_grid, and forms the rays' end points by the reference's formula with numpy and libm.  It applies V1-V6 and produces
the expected map by driving a second OracleMapper.update_rays in arrival order with `valid & ~veiled`; the expected stamps are
a per-ray replay of the oracle's own bresenham with the packets' ordinals.  The rule is all integer: the device agrees by ==.

The streams are built the way tests/ray_scenes.py builds its own: resolution 1/16, poses on cell centres, every end point at
least MARGIN of a cell from a cell edge (VeilModel.min_margin), so every ray is decided on the device.

No GPU, numpy only."""
import functools
import math

import numpy as np

import ray_scenes as rs
from oracle import oracle as orc

SIZE = 256
TILE = 64                      # a ray of 64 cells or more on an axis is written directly, never veiled (V4)
CELL_LIMIT = 1 << 30           # V1
MAX_RADIUS = 32
FAR = (20, 20)                 # where filler packets sit: further than any radius from every beam end of the scenes


def geo():
    return rs.Geo("S", SIZE)


def accepted_mask(buf, max_agent):
    rec = np.ascontiguousarray(buf).view(rs._P().PACKET_DTYPE).reshape(-1)
    return (rec["magic"] == b"QSRL") & (rec["agent"] >= 1) & (rec["agent"] <= max_agent)


@functools.lru_cache(maxsize=None)
def _line(x0, y0, x1, y1):
    return orc.bresenham(x0, y0, x1, y1).tolist()


class VeilModel:
    """One mapping session under the rule.  radius 0: the veil is off (nothing is veiled, the table is neither read nor fed)."""

    def __init__(self, g, max_agent, radius):
        self.g, self.max_agent, self.radius = g, max_agent, radius
        self.reset()

    def reset(self):                                             # V2: qs_reset empties the table
        self.o = self.g.oracle(self.max_agent)                   # fed the bytes: acceptance and poses
        self.m = self.g.oracle(self.max_agent)                   # driven ray by ray: the expected map
        self.table = {}
        self.total = 0
        self.seq = 0
        self.stamps = np.zeros((self.g.size, self.g.size), dtype=np.uint32)
        self.n_rays = self.n_hits = 0
        self.min_margin = math.inf

    def place(self, bot, x, y):
        cx, cy = int(self.o.world_to_grid([x], 0)[0]), int(self.o.world_to_grid([y], 1)[0])
        assert abs(cx) < CELL_LIMIT and abs(cy) < CELL_LIMIT
        self.table[int(bot)] = (cx, cy)

    def forget(self, bot=None):
        if bot is None:
            self.table.clear()
        else:
            self.table.pop(int(bot), None)

    def cells(self):
        """What qs_bot_veil_cells returns."""
        xy = np.zeros((self.max_agent + 1, 2), dtype=np.int32)
        known = np.zeros(self.max_agent + 1, dtype=np.uint8)
        for b, (x, y) in self.table.items():
            xy[b] = (x, y); known[b] = 1
        return xy, known

    def ingest(self, buf):
        """One packet ingest; returns (veiled uint8 [n, 4], valid uint8 [n, 4])."""
        g, o = self.g, self.o
        n = len(buf)
        acc = accepted_mask(buf, self.max_agent)
        before = len(o.poses)
        o.feed_stream(buf)
        poses = o.poses[before:]
        assert len(poses) == int(acc.sum())
        rec = np.ascontiguousarray(buf).view(rs._P().PACKET_DTYPE).reshape(-1)[acc]
        agents = rec["agent"].astype(int)
        d = np.stack([rec[k] for k in ("front", "left", "back", "right")], axis=1).astype(np.float64)
        ok = (rs.MIN_D < d) & (d <= rs.MAX_D)                                            # :888
        rng = np.where(ok, d, np.where(d > rs.MIN_D, np.minimum(d, rs.MAX_D), rs.MAX_D))  # :900
        a = poses[:, 2:3] + np.array(rs.SENSOR_ANG)[None, :]
        rx, ry = np.repeat(poses[:, 0], 4), np.repeat(poses[:, 1], 4)
        hx, hy = rx + (rng * np.cos(a)).reshape(-1), ry + (rng * np.sin(a)).reshape(-1)   # :890-891 / :901-902
        x0, y0 = o.world_to_grid(rx, 0), o.world_to_grid(ry, 1)
        x1, y1 = o.world_to_grid(hx, 0), o.world_to_grid(hy, 1)
        if len(hx):
            self.min_margin = min(self.min_margin, float(rs._margin(g, hx, hy).min()))
        valid = ok.reshape(-1)
        dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
        inbox = (np.maximum(x0, x1) >= 0) & (np.maximum(y0, y1) >= 0) & (np.minimum(x0, x1) < g.size) & (np.minimum(y0, y1) < g.size)
        binned = inbox & (dx < TILE) & (dy < TILE)                                        # V4: qt_ray_bin
        ingrid = (x1 >= 0) & (x1 < g.size) & (y1 >= 0) & (y1 < g.size)
        veiled = np.zeros(len(valid), dtype=bool)
        r2 = self.radius * self.radius
        if self.radius > 0:
            cur = dict(self.table)                                                        # V3: the table, then this call's packets
            for k in range(len(agents)):
                me = int(agents[k])
                for s in range(4):
                    r = 4 * k + s
                    if not (valid[r] and binned[r] and ingrid[r]):
                        continue
                    ex, ey = int(x1[r]), int(y1[r])
                    for b, (bx, by) in cur.items():
                        if b != me and (ex - bx) ** 2 + (ey - by) ** 2 <= r2:
                            veiled[r] = True
                            break
                cx, cy = int(x0[4 * k]), int(y0[4 * k])                                   # V1 (poses are finite: the packet was accepted)
                if abs(cx) < CELL_LIMIT and abs(cy) < CELL_LIMIT:
                    cur[me] = (cx, cy)
            self.table = cur                                                              # V6
        self.total += int(veiled.sum())
        cast = valid & ~veiled                                                            # V5
        self.m.update_rays(rx, ry, hx, hy, cast.astype(np.uint8))
        slot = np.nonzero(acc)[0]
        for k in range(len(agents)):
            for s in range(4):
                r = 4 * k + s
                cells = _line(int(x0[r]), int(y0[r]), int(x1[r]), int(y1[r]))
                key = (4 * (self.seq + int(slot[k])) + s + 1) << 1
                last = len(cells) - 1
                for j, (x, y) in enumerate(cells):
                    if (j < last or cast[r]) and 0 <= x < g.size and 0 <= y < g.size:
                        self.stamps[y, x] = max(self.stamps[y, x], key | (1 if j == last else 0))
        self.seq += n
        self.n_rays += len(valid)
        self.n_hits += int(valid.sum())                                                   # V5: QS_CNT_HITS counts what the filter judged
        out_v = np.zeros((n, 4), dtype=np.uint8)
        out_h = np.zeros((n, 4), dtype=np.uint8)
        out_v[acc] = veiled.reshape(-1, 4)
        out_h[acc] = valid.reshape(-1, 4)
        return out_v, out_h

    @property
    def grid(self):
        return self.m.grid

    @property
    def hits(self):
        return self.m.hits

    @property
    def misses(self):
        return self.m.misses

    @property
    def n_cells(self):
        return self.m.n_cells_written


# ---- scenes -----------------------------------------------------------------------------------------------------------------
class Veil:
    """A scene: a list of steps run against a mapper and a model alike.  ("ingest", buf, tags) | ("place", bot, qx, qy) |
    ("forget", bot) | ("reset",) | ("radius", r).  expect: {(ingest index, slot, sensor): veiled?} -- what the scene is named
    for, asserted on the CPU against the model (the expected flags themselves are always the model's)."""

    def __init__(self, name, radius, max_agent=3):
        self.name, self.radius, self.max_agent = name, radius, max_agent
        self.g = geo()
        self.steps, self.expect = [], {}
        self._rows, self._n_ingests = None, 0

    def rows(self):
        if self._rows is None:
            self._rows = rs._Rows(self.g)
            self._count = 0
        return self._rows

    def bot(self, agent, cx, cy, magic=True):
        """A packet of `agent` on cell (cx, cy) with four free rays (0.0 is no valid distance): it only speaks for its bot."""
        self.rows().cell(cx, cy, rs.YAW4[0], 0, others=0, agent=agent, magic=magic, tag="bot")
        self._count += 1
        return self._count - 1

    def beam(self, agent, cx, cy, h, k, veiled=None, raw=None):
        """A packet of `agent` on cell (cx, cy) whose front ray points along heading h = 0..3 (+x, +y, -x, -y) and is a hit of
        k cells (raw: the f32 distance instead); the other three are free rays.  veiled: what the scene expects of the front ray."""
        self.rows().cell(cx, cy, rs.YAW4[h], k, others=0, agent=agent, tag="beam", raw_front=raw)
        self._count += 1
        if veiled is not None:
            self.expect[(self._n_ingests, self._count - 1, 0)] = veiled
        return self._count - 1

    def fill(self, upto, agent=3):
        """Filler packets of `agent` far from everything until the ingest has `upto` packets."""
        rows = self.rows()
        n = upto - self._count
        assert n >= 0
        if n:
            rows.cell(np.full(n, FAR[0]), FAR[1], rs.YAW4[0], 0, others=0, agent=agent, tag="fill")
            self._count += n

    def end_ingest(self):
        sc = self._rows.scene(self.name)
        self.steps.append(("ingest", sc.data, sc.tags))
        self._rows = None
        self._n_ingests += 1

    def place(self, bot, cx, cy):
        g = self.g
        self.steps.append(("place", bot, float(g.at_q(g.centre_q(cx))), float(g.at_q(g.centre_q(cy)))))

    def forget(self, bot=None):
        self.steps.append(("forget", bot))

    def reset(self):
        self.steps.append(("reset",))

    def done(self):
        if self._rows is not None:
            self.end_ingest()
        return self


def snapshot(m):
    """What a session shows of its state: compared with the device by == (test_gpu_bot_veil.py)."""
    xy, known = m.cells()
    out = dict(grid=m.grid, stamps=m.stamps.copy(), hits=m.hits, misses=m.misses, xy=xy, known=known, total=m.total,
               n_rays=m.n_rays, n_hits=m.n_hits, n_cells=m.n_cells)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def run_model(sc, radius=None):
    """The scene through the model: (model, [veiled per ingest], [valid per ingest]); model.snaps: the session's snapshot
    before every reset and at the end."""
    m = VeilModel(sc.g, sc.max_agent, sc.radius if radius is None else radius)
    veiled, valid, snaps = [], [], []
    for st in sc.steps:
        if st[0] == "ingest":
            v, h = m.ingest(st[1])
            veiled.append(v); valid.append(h)
        elif st[0] == "place":
            m.place(*st[1:])
        elif st[0] == "forget":
            m.forget(st[1])
        elif st[0] == "reset":
            snaps.append(snapshot(m))
            m.reset()
    snaps.append(snapshot(m))
    m.snaps = snaps
    return m, veiled, valid


E = (110, 100)                 # where the scenes' beams end: from cell (100, 100) along +x, 10 cells
P1 = (100, 100)


def _radius_edge(radius, on, off):
    """Bot 2 at E + on (d^2 == radius^2) before the first beam, at E + off (d^2 == radius^2 + 1) before the second."""
    assert on[0] ** 2 + on[1] ** 2 == radius ** 2 and off[0] ** 2 + off[1] ** 2 == radius ** 2 + 1
    sc = Veil(f"radius-{radius}", radius)
    sc.bot(2, E[0] + on[0], E[1] + on[1])
    sc.beam(1, *P1, 0, 10, veiled=True)
    sc.bot(2, E[0] + off[0], E[1] + off[1])
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.bot(2, E[0] - on[0], E[1] - on[1])
    sc.beam(1, *P1, 0, 10, veiled=True)
    return sc.done()


def _which_pose():
    sc = Veil("which-pose", 3)
    near, far = (E[0] + 2, E[1] + 1), (E[0] + 40, E[1] + 40)
    # 0: the other bot's packet just after the beam's packet; 1: just before it
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.bot(2, *near)
    sc.beam(1, *P1, 0, 10, veiled=True)
    # two earlier packets at different cells: the later one decides
    sc.bot(2, *far)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.bot(2, *far); sc.bot(2, *near)
    sc.beam(1, *P1, 0, 10, veiled=True)
    # a rejected packet of that bot in between does not count
    sc.bot(2, *far, magic=False)
    sc.beam(1, *P1, 0, 10, veiled=True)
    sc.end_ingest()
    # the only earlier pose is the table's, from the previous ingest
    sc.beam(1, *P1, 0, 10, veiled=True)
    sc.end_ingest()
    sc.forget(2)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.end_ingest()
    # the same through bot_veil_place
    sc.place(2, *near)
    sc.beam(1, *P1, 0, 10, veiled=True)
    sc.end_ingest()
    sc.forget(None)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.end_ingest()
    sc.place(2, *near)
    sc.reset()
    sc.beam(1, *P1, 0, 10, veiled=False)
    return sc.done()


BLOCK_N = (255, 256, 257, 4097)
BLOCK_PAIRS = ((0, 1), (253, 254), (0, 255), (0, 256), (254, 255), (255, 256), (256, 257), (255, 4096), (256, 4096))


def _block_edges(n):
    """One ingest per (speaker slot, beam slot) pair that fits n packets, fillers elsewhere, a reset between them; then the
    beam at slot 0 with the speaker in the table, and the pairs the other way round (the beam first: not veiled)."""
    sc = Veil(f"blocks-{n}", 3)
    near = (E[0] + 1, E[1] - 2)
    for sp, bm in BLOCK_PAIRS:
        if bm >= n or (n > 257 and bm != n - 1):                 # (the largest batch repeats only what needs its size)
            continue
        for speaker_first in (True, False):
            a, b = (sp, bm) if speaker_first else (bm, sp)
            sc.fill(min(a, b))
            if speaker_first:
                sc.bot(2, *near)
            else:
                sc.beam(1, *P1, 0, 10, veiled=False)
            sc.fill(max(a, b))
            if speaker_first:
                sc.beam(1, *P1, 0, 10, veiled=True)
            else:
                sc.bot(2, *near)
            sc.fill(n)
            sc.end_ingest()
            sc.reset()
    sc.bot(2, *near); sc.fill(n); sc.end_ingest()
    sc.beam(1, *P1, 0, 10, veiled=True); sc.fill(n); sc.end_ingest()
    return sc.done()


def _one_bot_block():
    """Block 1 (slots 256..511) holds packets of bot 1 alone: every second one ends its beam on bot 2, heard at slot 0."""
    sc = Veil("one-bot-block", 3)
    sc.bot(2, E[0], E[1] + 3)
    sc.fill(256)
    for p in range(256):
        if p % 2 == 0:
            sc.beam(1, *P1, 0, 10, veiled=True)
        else:
            sc.beam(1, P1[0], P1[1] + 30, 0, 10, veiled=False)
    sc.fill(600)
    return sc.done()


def _many_bots():
    """255 bots on a lattice 12 cells apart, each looking at its +x neighbour from 11 cells: two rounds of 255 packets, so the
    first round fills block 0 with 255 different bots and the second crosses the block edge.  A beam is veiled iff the neighbour
    has spoken before it."""
    sc = Veil("many-bots", 2, max_agent=255)
    for rnd in range(2):
        for b in range(1, 256):
            ix, iy = (b - 1) % 16, (b - 1) // 16
            nb = b + 1 if ix < 15 and b < 255 else None
            sc.beam(b, 30 + 12 * ix, 30 + 12 * iy, 0, 11, veiled=(nb is not None and rnd == 1))
    return sc.done()


def _never():
    sc = Veil("never", 8)
    # a beam of the bot itself that ends on its own earlier cell
    sc.bot(1, *E)
    sc.beam(1, *P1, 0, 10, veiled=False)
    # a beam the range filter rejects (25 cells = 1.5625 m > 1.2 m): its free ray of 19.2 cells ends on bot 2
    sc.bot(2, P1[0] + 19, P1[1])
    sc.beam(1, *P1, 0, 0, veiled=False, raw=np.float32(25 / 16))
    # a beam whose end cell lies outside the grid, 6 cells from bot 2 on the grid's last column
    sc.bot(2, SIZE - 2, 60)
    sc.beam(1, SIZE - 6, 60, 0, 10, veiled=False)
    # ... and the same beam turned round ends inside: veiled
    sc.bot(2, SIZE - 20, 60)
    sc.beam(1, SIZE - 6, 60, 2, 10, veiled=True)
    return sc.done()


def _tile_border():
    """The bot's cell and the end cell in different 64-cell tiles, on both axes."""
    sc = Veil("tile-border", 3)
    sc.bot(2, 62, 100)
    sc.beam(1, 70, 100, 2, 6, veiled=True)          # ends on (64, 100)
    sc.bot(2, 100, 129)
    sc.beam(1, 100, 120, 1, 7, veiled=True)         # ends on (100, 127)
    sc.bot(2, 66, 66)
    sc.beam(1, 63, 70, 3, 7, veiled=False)          # ends on (63, 63): d^2 = 18
    sc.bot(2, 65, 65)
    sc.beam(1, 63, 70, 3, 7, veiled=True)           # d^2 = 8
    return sc.done()


def _mixed(n):
    """n packets of three bots that walk past each other with valid hits on all four sensors: what the V5, small-batch and
    off-means-off tests run."""
    sc = Veil(f"mixed-{n}", 3)
    p = np.arange(n)
    agent = 1 + p % 3
    step = p // 3
    cx = np.where(agent == 1, 90 + step % 30, np.where(agent == 2, 120 - step % 30, 105))
    cy = np.where(agent == 3, 90 + step % 25, np.where(agent == 2, 101, 100))
    rows = sc.rows()
    for k in range(n):
        g = sc.g
        d4 = g.dist([3 + (k % 7), 2 + (k % 3), 1 + (k % 5), 4])
        rows.extend(g.centre_q(int(cx[k])), g.centre_q(int(cy[k])), rs.YAW4[(k // 5) % 4], d4, agent=int(agent[k]), tag="mixed")
    sc._count = n
    return sc.done()


SMALL_N = (1, 4, 20)
BUILDERS = {"radius-1": lambda: _radius_edge(1, (1, 0), (1, 1)), "radius-3": lambda: _radius_edge(3, (3, 0), (3, 1)),
            "radius-32": lambda: _radius_edge(32, (32, 0), (32, 1)), "radius-5": lambda: _radius_edge(5, (3, 4), (5, 1)),
            "which-pose": _which_pose, "one-bot-block": _one_bot_block, "many-bots": _many_bots, "never": _never,
            "tile-border": _tile_border, "mixed-300": lambda: _mixed(300)}
BUILDERS.update({f"blocks-{n}": (lambda n=n: _block_edges(n)) for n in BLOCK_N})
BUILDERS.update({f"mixed-{n}": (lambda n=n: _mixed(n)) for n in SMALL_N})


def names(prefix=""):
    return [k for k in BUILDERS if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def model(name):
    """(model, veiled, valid) of a scene, computed once and shared."""
    return run_model(get(name))


# ---- the built room ---------------------------------------------------------------------------------------------------------
ROOM_C, ROOM_A, ROOM_W = 128, 6, 13      # centre cell, the bots' distance from it, the walls' distance from it (cells)
ROOM_BODY, ROOM_RADIUS = 2, 4            # body radius (cells); veil radius = body / res + 1.5 rounded up, for a stationary bot
ROOM_BOTS = ((1, -ROOM_A, 0, 0), (2, ROOM_A, 0, 2), (3, 0, -ROOM_A, 1), (4, 0, ROOM_A, 3))    # bot, dx, dy, heading: all face the centre


def room_world():
    """int8 world: walls OCCUPIED (100) on the square ring ROOM_W cells from the centre, FREE (0) inside, UNKNOWN (-1) outside."""
    w = np.full((SIZE, SIZE), -1, dtype=np.int8)
    lo, hi = ROOM_C - ROOM_W, ROOM_C + ROOM_W
    w[lo:hi + 1, lo:hi + 1] = 100
    w[lo + 1:hi, lo + 1:hi] = 0
    return w


def room_ranges():
    """Per bot of ROOM_BOTS: (pose cell, heading, four wall distances in cells front, left, back, right): axis-aligned beams in
    a square room, so each distance is a count of cells to the wall ring."""
    out = []
    for bot, dx, dy, h in ROOM_BOTS:
        cx, cy = ROOM_C + dx, ROOM_C + dy
        d = []
        for s in range(4):
            ux, uy = rs.DIR4[(h + s) % 4]                        # front, left (+90 deg), back, right
            d.append(ROOM_W - (dx * ux + dy * uy))
        out.append((bot, cx, cy, h, d))
    return out


def room_stream(shorten, rounds=3):
    """`rounds` packets of each of the four stationary bots, in turn.  shorten(pose [n, 3], agent [n], ranges f32 [n, 4]) ->
    ranges: the sim's body rule (sim.body_ranges)."""
    g = geo()
    rr = room_ranges()
    pose = np.array([[float(g.at_q(g.centre_q(cx))), float(g.at_q(g.centre_q(cy))), float(rs.YAW4[h])] for _, cx, cy, h, _ in rr])
    agent = np.array([b for b, *_ in rr], dtype=np.uint8)
    ranges = np.stack([g.dist(d) for *_, d in rr]).astype(np.float32)
    ranges = shorten(pose, agent, ranges)
    P = rs._P()
    k = len(rr)
    one = P.pack_packets(agent, pose[:, 0].astype(np.float32), pose[:, 1].astype(np.float32), pose[:, 2].astype(np.float32),
                         np.zeros(k, np.int32), np.zeros(k, np.uint32), ranges, np.zeros(k, np.uint8))
    return np.concatenate([one] * rounds)
