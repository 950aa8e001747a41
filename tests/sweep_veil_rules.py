"""The bot veil for sweeps (include/quasar_slam.h, rules S0-S8) restated with a plain loop over the records (numpy over one
record's beams and the bots), and the built scenes its tests use.

`SweepVeilModel` extends veil_rules.VeilModel, so one model holds one table, one statistics word, one map and one stamp order for
packet and sweep ingests alike (S2: the table is shared).  A sweep ingest takes acceptance and beams from ray_scenes.sweep_beams,
cells through the oracle's world_to_grid, applies S1-S5, and produces the expected map by driving the second oracle's update_rays
with `valid & ~veiled`; the expected stamps are a per-beam replay of the oracle's own bresenham with ordinal slot + 1 (after the
sequence numbers used so far).  The rule is all integer: the device agrees by ==.

The scenes are built the way tests/veil_rules.py and tests/ray_scenes.py build theirs: resolution 1/16, poses on cell centres,
every end point at least MARGIN of a cell from a cell edge (min_margin), so every beam is decided on the device.  Every beam of a
built sweep is a hit: its target beams are given, the others are short hits of 2..5 cells that stay near their own bot.

No GPU, numpy only."""
import functools
import math

import numpy as np

import ray_scenes as rs
import veil_rules as vr

SIZE, TILE, CELL_LIMIT = vr.SIZE, vr.TILE, vr.CELL_LIMIT
BEAMS, SLOTS, SEQS = 181, rs.SWEEP_SLOTS, 46
CHUNK = 1 << 16                  # records per chunk of a sweep call (csrc/sweep.hip: QS_SWEEP_CHUNK)
SHORT = (3, 4, 2, 5)             # cells: candidate lengths of a beam that is no target
E, P1 = vr.E, vr.P1              # the radius scenes: beam 90 of a sweep on P1 heading +x, 10 cells long, ends on E


def geo():
    return vr.geo()


def as_scene(g, buf, max_agent):
    return rs.Scene("sweeps", g, "sweeps", buf, None, max_agent=max_agent)


def beams_from(records, poses, smin, smax):
    """sweep_beams' formula over given poses: records [(record number, record)] are the accepted ones (accepted_records), poses
    float64 [m, 3] what each is cast from.  With the records' own poses it equals rs.sweep_beams (test_sweep_veil_rules_cpu.py)."""
    out = ([], [], [], [], [], [])
    for (k, r), (px, py, yaw) in zip(records, poses):
        px, py, yaw = float(px), float(py), float(yaw)
        for i, d in enumerate(r["ranges"].tolist()):
            a = yaw + math.radians(i - 90)
            ok = smin < d <= smax
            L = d if ok else (min(d, smax) if d > smin else smax)
            for col, v in zip(out, (px, py, px + L * math.cos(a), py + L * math.sin(a), 1 if ok else 0, SLOTS * k + i)):
                col.append(v)
    return [np.array(v, dtype=np.float64) for v in out[:4]] + [np.array(out[4], dtype=np.uint8), np.array(out[5], dtype=np.int64)]


def accepted_records(buf, max_agent, withheld=()):
    """[(record number, record)] of the records that are accepted and not withheld."""
    recs = np.ascontiguousarray(buf).view(rs._P().PACKET_DTYPE_V0_ODO).reshape(-1)
    ok = (recs["magic"] == b"QSRL") & (recs["agent"] >= 1) & (recs["agent"] <= max_agent)
    for k in withheld:
        ok[k] = False
    return [(int(k), recs[k]) for k in np.nonzero(ok)[0]]


class SweepVeilModel(vr.VeilModel):
    """One mapping session under V1-V7 and S0-S8.  sweeps: the switch (S0)."""

    def __init__(self, g, max_agent, radius, sweeps=True, smin=rs.SMIN_D, smax=rs.SMAX_D):
        self.sweeps, self.smin, self.smax = sweeps, smin, smax
        vr.VeilModel.__init__(self, g, max_agent, radius)

    def ingest_sweeps(self, buf, withheld=(), poses=None):
        """One sweep ingest of uint8 [n, 751]; returns (veiled uint8 [n, 181], valid uint8 [n, 181]).  withheld: record numbers
        the guarded ingest withholds (S1: they count as rejected).  poses: float64 [n, 3] the poses the records are cast from
        where that is not the record's own (the matched ingest, graph mode); rows of rejected records are ignored."""
        g, o = self.g, self.o
        n = len(buf)
        live = accepted_records(buf, self.max_agent, withheld)
        if poses is None and not withheld:
            rx, ry, hx, hy, valid, slot = rs.sweep_beams(as_scene(g, buf, self.max_agent), self.smin, self.smax)
        else:
            own = [(float(r["x"]), float(r["y"]), float(r["yaw"])) for _, r in live]
            rx, ry, hx, hy, valid, slot = beams_from(live, own if poses is None else [poses[k] for k, _ in live], self.smin, self.smax)
        assert len(slot) == BEAMS * len(live)
        valid = valid.astype(bool)
        x0, y0 = o.world_to_grid(rx, 0), o.world_to_grid(ry, 1)
        x1, y1 = o.world_to_grid(hx, 0), o.world_to_grid(hy, 1)
        if len(hx):
            self.min_margin = min(self.min_margin, float(rs._margin(g, hx, hy).min()))
        dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
        inbox = (np.maximum(x0, x1) >= 0) & (np.maximum(y0, y1) >= 0) & (np.minimum(x0, x1) < g.size) & (np.minimum(y0, y1) < g.size)
        binned = inbox & (dx < TILE) & (dy < TILE)                                        # S3: qt_ray_bin
        ingrid = (x1 >= 0) & (x1 < g.size) & (y1 >= 0) & (y1 < g.size)
        veiled = np.zeros(len(valid), dtype=bool)
        acting = self.sweeps and self.radius > 0                                          # S0
        if acting:
            r2 = self.radius * self.radius
            cur = dict(self.table)                                                        # S2: the table, then this call's sweeps
            for j, (k, rec) in enumerate(live):
                me = int(rec["agent"])
                others = np.array([c for b, c in cur.items() if b != me], dtype=np.int64).reshape(-1, 2)
                el = BEAMS * j + np.nonzero((valid & binned & ingrid)[BEAMS * j:BEAMS * (j + 1)])[0]          # S3's first three conditions
                if len(others) and len(el):                                                 # ... and the fourth, beams x bots
                    d2 = (x1[el, None] - others[None, :, 0]) ** 2 + (y1[el, None] - others[None, :, 1]) ** 2
                    veiled[el] = (d2 <= r2).any(axis=1)
                cx, cy = int(x0[BEAMS * j]), int(y0[BEAMS * j])                           # S1
                if math.isfinite(rx[BEAMS * j]) and math.isfinite(ry[BEAMS * j]) and abs(cx) < CELL_LIMIT and abs(cy) < CELL_LIMIT:
                    cur[me] = (cx, cy)
            self.table = cur                                                              # S5
        self.total += int(veiled.sum())                                                   # S8
        cast = valid & ~veiled                                                            # S4
        self.m.update_rays(rx, ry, hx, hy, cast.astype(np.uint8))
        base = 4 * self.seq                                                               # ordinal = slot + 1 after the sequence numbers so far
        for r in range(len(slot)):
            cells = vr._line(int(x0[r]), int(y0[r]), int(x1[r]), int(y1[r]))
            key = (base + int(slot[r]) + 1) << 1
            last = len(cells) - 1
            for j, (x, y) in enumerate(cells):
                if (j < last or cast[r]) and 0 <= x < g.size and 0 <= y < g.size:
                    self.stamps[y, x] = max(self.stamps[y, x], key | (1 if j == last else 0))
        self.seq += SEQS * n
        self.n_rays += len(valid)
        self.n_hits += int(valid.sum())                                                   # S4: as the filter judged them
        out_v = np.zeros((n, BEAMS), dtype=np.uint8)
        out_h = np.zeros((n, BEAMS), dtype=np.uint8)
        idx = np.array([k for k, _ in live], dtype=np.int64)
        if len(idx):
            out_v[idx] = veiled.reshape(-1, BEAMS)
            out_h[idx] = valid.reshape(-1, BEAMS)
        return out_v, out_h


# ---- building sweeps ------------------------------------------------------------------------------------------------------------
def _end(g, px, py, yaw, i, k):
    a = float(yaw) + math.radians(i - 90)
    d = float(g.dist(k))
    return px + d * math.cos(a), py + d * math.sin(a)


@functools.lru_cache(maxsize=None)
def _ranges(cx, cy, h, targets, smax):
    """f32 [181] for a sweep on the centre of cell (cx, cy) heading YAW4[h]: beam i of `targets` ((i, (candidate lengths in
    cells)), ...) takes the first candidate whose end point keeps MARGIN from every cell edge, every other beam the first of
    SHORT that does.  Every length must be a hit under (0.1, smax]."""
    g = geo()
    px, py, yaw = float(g.at_q(g.centre_q(cx))), float(g.at_q(g.centre_q(cy))), rs.YAW4[h]
    want = dict(targets)
    out = np.zeros(BEAMS, dtype=np.float32)
    for i in range(BEAMS):
        for k in want.get(i, SHORT):
            ex, ey = _end(g, px, py, yaw, i, k)
            if rs.SMIN_D < float(g.dist(k)) <= smax and float(rs._margin(g, np.array([ex]), np.array([ey]))[0]) >= rs.MARGIN:
                out[i] = g.dist(k)
                break
        else:
            raise AssertionError(f"beam {i} on ({cx}, {cy}): no candidate keeps clear of the cell edges")
    out.setflags(write=False)
    return out


def end_cell(cx, cy, h, i, ranges):
    """The cell beam i of such a sweep ends on, through the oracle's world_to_grid."""
    g = geo()
    o = g.oracle()
    px, py = float(g.at_q(g.centre_q(cx))), float(g.at_q(g.centre_q(cy)))
    a = float(rs.YAW4[h]) + math.radians(i - 90)
    d = float(ranges[i])
    return int(o.world_to_grid([px + d * math.cos(a)], 0)[0]), int(o.world_to_grid([py + d * math.sin(a)], 1)[0])


class SV:
    """A scene: steps run against a mapper and a model alike.  ("sweeps", buf, opts) | ("packets", buf) | ("place", bot, x, y) |
    ("forget", bot) | ("reset",).  expect: {(sweep ingest index, record, beam): veiled?} -- what the scene is named for, asserted
    on the CPU against the model (the expected flags themselves are always the model's)."""

    def __init__(self, name, radius, max_agent=3, smax=rs.SMAX_D):
        self.name, self.radius, self.max_agent, self.smax = name, radius, max_agent, smax
        self.g = geo()
        self.steps, self.expect = [], {}
        self._rows, self._n_ingests = [], 0

    def sweep(self, agent, cx, cy, h=0, targets=(), magic=True, veiled=None, raw=None):
        """A sweep of `agent` on cell (cx, cy) heading h; targets: ((beam, length in cells or tuple of candidates), ...).
        veiled: {beam: expected?}.  raw: {beam: f32 range} written over the built ranges.  Returns its record number."""
        t = tuple((i, k if isinstance(k, tuple) else (k,)) for i, k in targets)
        r = _ranges(cx, cy, h, t, self.smax)
        if raw:
            r = r.copy()
            for i, v in raw.items():
                r[i] = v
        self._rows.append((agent, cx, cy, h, r, magic))
        k = len(self._rows) - 1
        for i, v in (veiled or {}).items():
            self.expect[(self._n_ingests, k, i)] = v
        return k

    def bot(self, agent, cx, cy, magic=True):
        """A sweep that only speaks for its bot (short hits round it)."""
        return self.sweep(agent, cx, cy, magic=magic)

    def beam(self, agent, cx, cy, h, k, veiled=None):
        """A sweep whose beam 90 (straight ahead) is a hit of k cells; veiled: what the scene expects of that beam."""
        return self.sweep(agent, cx, cy, h, ((90, k),), veiled=None if veiled is None else {90: veiled})

    def fill(self, upto):
        """Rejected records until the ingest has `upto` records: they cost the restatement nothing and are silent (S1)."""
        n = upto - len(self._rows)
        assert n >= 0
        self._rows += [None] * n

    def end_ingest(self, **opts):
        g, P = self.g, rs._P()
        n = len(self._rows)
        live = [(k, r) for k, r in enumerate(self._rows) if r is not None]
        buf = np.zeros((n, P.PACKET_SIZE_V0_ODO), dtype=np.uint8)
        buf[:, :4] = np.frombuffer(b"XSRL", dtype=np.uint8)
        if live:
            idx = np.array([k for k, _ in live])
            agent = np.array([r[0] for _, r in live], dtype=np.uint8)
            x = g.at_q(g.centre_q(np.array([r[1] for _, r in live])))
            y = g.at_q(g.centre_q(np.array([r[2] for _, r in live])))
            yaw = np.array([rs.YAW4[r[3]] for _, r in live], dtype=np.float32)
            one = P.pack_sweeps(agent, x, y, yaw, np.stack([r[4] for _, r in live])).copy()
            one[np.array([not r[5] for _, r in live]), 0] = ord("X")
            buf[idx] = one
        self.steps.append(("sweeps", buf, opts))
        self._rows = []
        self._n_ingests += 1

    def packets(self, buf):
        self.steps.append(("packets", buf))

    def place(self, bot, cx, cy):
        g = self.g
        self.steps.append(("place", bot, float(g.at_q(g.centre_q(cx))), float(g.at_q(g.centre_q(cy)))))

    def forget(self, bot=None):
        self.steps.append(("forget", bot))

    def reset(self):
        self.steps.append(("reset",))

    def done(self):
        if self._rows:
            self.end_ingest()
        return self


def run_model(sc, radius=None, sweeps=True):
    """The scene through the model: (model, [veiled per ingest], [valid per ingest]) -- sweep and packet ingests in step order;
    model.snaps: the session's snapshot before every reset and at the end."""
    m = SweepVeilModel(sc.g, sc.max_agent, sc.radius if radius is None else radius, sweeps=sweeps, smax=sc.smax)
    veiled, valid, snaps = [], [], []
    for st in sc.steps:
        if st[0] == "sweeps":
            v, h = m.ingest_sweeps(st[1], **{k: v for k, v in st[2].items() if k in ("withheld",)})
            veiled.append(v); valid.append(h)
        elif st[0] == "packets":
            v, h = m.ingest(st[1])
            veiled.append(v); valid.append(h)
        elif st[0] == "place":
            m.place(*st[1:])
        elif st[0] == "forget":
            m.forget(st[1])
        elif st[0] == "reset":
            snaps.append(vr.snapshot(m))
            m.reset()
    snaps.append(vr.snapshot(m))
    m.snaps = snaps
    return m, veiled, valid


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _radius_edge(radius, on, off):
    """Bot 2 at E + on (d^2 == radius^2) before the first beam, at E + off (d^2 == radius^2 + 1) before the second."""
    assert on[0] ** 2 + on[1] ** 2 == radius ** 2 and off[0] ** 2 + off[1] ** 2 == radius ** 2 + 1
    sc = SV(f"radius-{radius}", radius)
    sc.bot(2, E[0] + on[0], E[1] + on[1])
    sc.beam(1, *P1, 0, 10, veiled=True)
    sc.bot(2, E[0] + off[0], E[1] + off[1])
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.bot(2, E[0] - on[0], E[1] - on[1])
    sc.beam(1, *P1, 0, 10, veiled=True)
    return sc.done()


BEAM_IDS = (0, 63, 64, 127, 128, 180)
BEAM_LEN = (16, 15, 17, 14)


def _each_beam():
    """One sweep ingest per beam of BEAM_IDS: bot 2 is placed on the cell that beam ends on, 14..17 cells out, where the
    sweep's other beams (2..5 cells) do not reach; radius 1 takes in at most the beam's neighbours."""
    sc = SV("each-beam", 1)
    for i in BEAM_IDS:
        t = ((i, BEAM_LEN),)
        r = _ranges(*P1, 1, tuple((b, k) for b, k in t), sc.smax)
        sc.place(2, *end_cell(*P1, 1, i, r))
        sc.sweep(1, *P1, 1, t, veiled={i: True, (i + 90) % BEAMS: False})
        sc.end_ingest()
        sc.forget(2)
    return sc.done()


def _who_speaks():
    sc = SV("who-speaks", 3)
    near, far = (E[0] + 2, E[1] + 1), (E[0] + 40, E[1] + 40)
    # 0: the other bot's sweep just after the beam's sweep; just before it
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.bot(2, *near)
    sc.beam(1, *P1, 0, 10, veiled=True)
    # two earlier sweeps at different cells: the later one decides
    sc.bot(2, *far)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.bot(2, *far); sc.bot(2, *near)
    sc.beam(1, *P1, 0, 10, veiled=True)
    # a rejected sweep of that bot in between is silent
    sc.bot(2, *far, magic=False)
    sc.beam(1, *P1, 0, 10, veiled=True)
    # the bot's own later sweep does not veil its own beam: bot 1 has stood on E, bot 2 is far away by now
    sc.bot(2, *far)
    sc.bot(1, *E)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.bot(2, *near)
    sc.end_ingest()
    # 1: an earlier sweep of the call against the table: the table says near, the call's earlier sweep says far, then near again
    sc.beam(1, *P1, 0, 10, veiled=True)
    sc.bot(2, *far)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.end_ingest()
    sc.place(2, *near)
    sc.beam(1, *P1, 0, 10, veiled=True)
    sc.end_ingest()
    sc.forget(2)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.end_ingest()
    sc.place(2, *near)
    sc.forget(None)
    sc.beam(1, *P1, 0, 10, veiled=False)
    sc.end_ingest()
    sc.place(2, *near)
    sc.reset()
    sc.beam(1, *P1, 0, 10, veiled=False)
    return sc.done()


BLOCK_N = (255, 256, 257, 4097)
BLOCK_PAIRS = vr.BLOCK_PAIRS


def _block_edges(n):
    """One ingest per (speaker record, beam record) pair that fits n records, rejected filler elsewhere, a reset between them;
    then the pairs the other way round (the beam first: not veiled), and the beam on record 0 with the speaker in the table."""
    sc = SV(f"blocks-{n}", 3)
    near = (E[0] + 1, E[1] - 2)
    for sp, bm in BLOCK_PAIRS:
        if bm >= n or (n > 257 and bm != n - 1):                 # (the largest call repeats only what needs its size)
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
    """Block 1 (records 256..511) holds sweeps of bot 1 alone -- the longest segment a block can have: every second one ends its
    beam on bot 2, heard on record 0; bot 2's sweep after the block sees bot 1 where the block left it."""
    sc = SV("one-bot-block", 3)
    sc.bot(2, E[0], E[1] + 3)
    sc.fill(256)
    for p in range(256):
        if p % 2 == 0:
            sc.beam(1, *P1, 0, 10, veiled=True)
        else:
            sc.beam(1, P1[0], P1[1] + 30, 0, 10, veiled=False)
    sc.beam(2, P1[0] - 12, P1[1] + 30, 0, 10, veiled=True)      # ends 2 cells from bot 1's last cell
    sc.fill(600)
    return sc.done()


def _many_bots():
    """255 bots on a lattice 12 cells apart, each looking at its +x neighbour from 11 cells: two rounds of 255 sweeps, so the
    first round fills block 0 with 255 different bots and the second crosses the block edge.  The beam is veiled iff the
    neighbour has spoken before it."""
    sc = SV("many-bots", 2, max_agent=255)
    for rnd in range(2):
        for b in range(1, 256):
            ix, iy = (b - 1) % 16, (b - 1) // 16
            nb = b + 1 if ix < 15 and b < 255 else None
            sc.beam(b, 30 + 12 * ix, 30 + 12 * iy, 0, 11, veiled=(nb is not None and rnd == 1))
    return sc.done()


def _chunk_edge():
    """2^16 + 1 records, all but four of them rejected: the speaker on the first chunk's last record and the beam on the second
    chunk's only record; a speaker of another bot on record 0 of the call is heard in the second chunk as well."""
    sc = SV("chunk-edge", 3)
    sc.bot(3, E[0] - 1, E[1] + 2)                                # record 0: bot 3, near E
    sc.beam(1, *P1, 0, 10, veiled=True)                          # record 1: veiled by bot 3 already
    sc.fill(CHUNK - 1)
    sc.bot(2, P1[0], P1[1] + 42)                                 # record 2^16 - 1: bot 2, beside where bot 1's second beam ends
    k = sc.sweep(1, P1[0], P1[1] + 30, 1, ((90, 10), (0, BEAM_LEN)), veiled={90: True, 0: False})      # record 2^16: ends on (100, 140)
    assert k == CHUNK
    return sc.done()


def _chunk_edge_far():
    """The same call with bot 2 out of reach: the second chunk's beam towards E is veiled by record 0's speaker alone."""
    sc = SV("chunk-edge-far", 3)
    sc.bot(3, E[0] - 1, E[1] + 2)
    sc.fill(CHUNK - 1)
    sc.bot(2, 20, 20)
    sc.sweep(1, *P1, 0, ((90, 10), (0, BEAM_LEN)), veiled={90: True, 0: False})
    return sc.done()


def _never():
    sc = SV("never", 8)
    # a beam of the bot itself that ends on its own earlier cell
    sc.bot(1, *E)
    sc.beam(1, *P1, 0, 10, veiled=False)
    # a beam the range filter rejects (25 cells = 1.5625 m > 1.2 m): its free beam of 19.2 cells ends on bot 2
    sc.bot(2, P1[0] + 19, P1[1])
    sc.sweep(1, *P1, 0, raw={90: np.float32(25 / 16)}, veiled={90: False})
    # a beam whose end cell lies outside the grid, 6 cells from bot 2 on the grid's last column
    sc.bot(2, SIZE - 2, 60)
    sc.beam(1, SIZE - 6, 60, 0, 10, veiled=False)
    # ... and the same beam turned round ends inside: veiled
    sc.bot(2, SIZE - 20, 60)
    sc.beam(1, SIZE - 6, 60, 2, 10, veiled=True)
    return sc.done()


LONG_SMAX = 5.0


def _long_beam():
    """The sweep filter raised to 5 m: a beam of 64 cells on an axis is written directly and never veiled, one of 63 is."""
    sc = SV("long-beam", 3, smax=LONG_SMAX)
    sc.bot(2, 164, 100)
    sc.beam(1, 100, 100, 0, 64, veiled=False)
    sc.bot(2, 163, 100)
    sc.beam(1, 100, 100, 0, 63, veiled=True)
    return sc.done()


def _tile_border():
    """The bot's cell and the end cell in different 64-cell tiles, on both axes."""
    sc = SV("tile-border", 3)
    sc.bot(2, 62, 100)
    sc.beam(1, 70, 100, 2, 6, veiled=True)          # ends on (64, 100)
    sc.bot(2, 100, 129)
    sc.beam(1, 100, 120, 1, 7, veiled=True)         # ends on (100, 127)
    sc.bot(2, 66, 66)
    sc.beam(1, 63, 70, 3, 7, veiled=False)          # ends on (63, 63): d^2 = 18
    sc.bot(2, 65, 65)
    sc.beam(1, 63, 70, 3, 7, veiled=True)           # d^2 = 8
    return sc.done()


def _mixed(n, apart=False):
    """n sweeps of three bots that walk past each other (in a call of four at most bot 2 starts beside where bot 1's second sweep
    ends its beam); apart: the bots far from one another (nothing to veil)."""
    sc = SV(f"mixed-{n}{'-apart' if apart else ''}", 3)
    for k in range(n):
        agent = 1 + k % 3
        step = k // 3
        if apart:
            cx, cy = (60, 60) if agent == 1 else ((190, 70) if agent == 2 else (120, 190))
            cx += step % 5
        else:
            cx = 90 + step % 10 if agent == 1 else ((112 if n > 4 else 102) - step % 10 if agent == 2 else 101)
            cy = 100 if agent == 1 else (101 if agent == 2 else 92 + step % 9)
        sc.sweep(agent, cx, cy, (k // 5) % 4, ((90, (10, 9, 11)), (30 + k % 7, (7, 8, 6)), (150 - k % 5, (12, 13, 11))))
    return sc.done()


def _with_packets():
    """The shared table: a sweep bot veils a packet beam of a later packet ingest, and a packet bot a sweep beam."""
    sc = SV("with-packets", 3)
    pk = vr.Veil("pk", 3)
    pk.beam(1, *P1, 0, 10, veiled=True)                          # bot 2 was heard through its sweep
    pk.bot(3, P1[0], P1[1] + 42)
    pk.end_ingest()
    sc.bot(2, E[0] + 2, E[1] - 1)
    sc.end_ingest()
    sc.packets(pk.steps[0][1])
    sc.sweep(1, P1[0], P1[1] + 30, 1, ((90, 10),), veiled={90: True})    # bot 3 was heard through its packet
    sc.beam(2, *P1, 0, 10, veiled=False)                         # ... and bot 1's own packet cell veils nothing of bot 1
    return sc.done()


def _guard():
    """Ingest 0 (plain): bot 1 draws short hits round P1.  Ingest 1 (guarded): bot 2 on P1 claims 9..12 cells of free space through
    them -- a contradiction, withheld (GUARD_WITHHELD): it is silent and bot 1's beam, which ends beside P1, is not veiled.  Then
    bot 3 repeats that first sweep (it agrees with the map), and bot 1's beam is veiled by it."""
    sc = SV("guard", 3)
    sc.bot(1, *P1)                                               # (bot 1's own cell veils nothing of bot 1)
    sc.end_ingest()
    k = sc.sweep(2, *P1, 0, tuple((i, (10, 11, 12, 9)) for i in range(BEAMS)))
    assert k == GUARD_WITHHELD
    sc.beam(1, P1[0] - 12, P1[1], 0, 10, veiled=False)
    sc.bot(3, *P1)
    sc.beam(1, P1[0] - 12, P1[1], 0, 10, veiled=True)
    sc.end_ingest(check=True, withheld=(GUARD_WITHHELD,))
    return sc.done()


GUARD_WITHHELD = 0
SMALL_N = (1, 4)
BUILDERS = {"guard": _guard, "radius-1": lambda: _radius_edge(1, (1, 0), (1, 1)), "radius-3": lambda: _radius_edge(3, (3, 0), (3, 1)),
            "radius-32": lambda: _radius_edge(32, (32, 0), (32, 1)), "radius-5": lambda: _radius_edge(5, (3, 4), (5, 1)),
            "each-beam": _each_beam, "who-speaks": _who_speaks, "one-bot-block": _one_bot_block, "many-bots": _many_bots,
            "chunk-edge": _chunk_edge, "chunk-edge-far": _chunk_edge_far, "never": _never, "long-beam": _long_beam,
            "tile-border": _tile_border, "mixed-60": lambda: _mixed(60), "with-packets": _with_packets}
BUILDERS.update({f"blocks-{n}": (lambda n=n: _block_edges(n)) for n in BLOCK_N})
BUILDERS.update({f"mixed-{n}": (lambda n=n: _mixed(n)) for n in SMALL_N})
BUILDERS.update({f"mixed-{n}-apart": (lambda n=n: _mixed(n, apart=True)) for n in SMALL_N})


def names(prefix=""):
    return [k for k in BUILDERS if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def model(name):
    """(model, veiled, valid) of a scene, computed once and shared."""
    return run_model(get(name))


# ---- the built room of sweep bots -----------------------------------------------------------------------------------------------
ROOM_C, ROOM_A, ROOM_W = vr.ROOM_C, vr.ROOM_A, 15        # centre cell, the bots' distance from it, the walls' distance from it
ROOM_BODY, ROOM_RADIUS = vr.ROOM_BODY, vr.ROOM_RADIUS    # body radius (cells); veil radius = body / res + 1.5 rounded up
ROOM_BOTS = vr.ROOM_BOTS                                 # bot, dx, dy, heading: all four face the centre


def room_world():
    """int8 world: walls OCCUPIED (100) on the square ring ROOM_W cells from the centre, FREE (0) inside, UNKNOWN (-1) outside."""
    w = np.full((SIZE, SIZE), -1, dtype=np.int8)
    lo, hi = ROOM_C - ROOM_W, ROOM_C + ROOM_W
    w[lo:hi + 1, lo:hi + 1] = 100
    w[lo + 1:hi, lo + 1:hi] = 0
    return w


def room_poses():
    g = geo()
    return np.array([[float(g.at_q(g.centre_q(ROOM_C + dx))), float(g.at_q(g.centre_q(ROOM_C + dy))), float(rs.YAW4[h])]
                     for _, dx, dy, h in ROOM_BOTS])


def room_wall_ranges():
    """float32 [4, 181]: per bot and beam the distance at which the beam from the bot's cell centre enters the wall ring's cells
    plus a quarter of a cell, found by walking the beam in steps of 1/64 cell through room_world (fp64)."""
    g = geo()
    w = room_world()
    poses = room_poses()
    out = np.zeros((len(poses), BEAMS), dtype=np.float32)
    for b, (px, py, yaw) in enumerate(poses):
        for i in range(BEAMS):
            a = yaw + math.radians(i - 90)
            t = 0.0
            while True:
                t += g.res / 64
                cx, cy = int((px + t * math.cos(a) - g.ox) / g.res), int((py + t * math.sin(a) - g.oy) / g.res)
                if w[cy, cx] == 100:
                    break
            out[b, i] = np.float32(t + g.res / 4)
    return out


def room_stream(shorten, rounds=2):
    """`rounds` sweeps of each of the four stationary bots, in turn.  shorten(pose [n, 3], agent [n], ranges f32 [n, 181]) ->
    ranges: the sim's body rule (sim.body_sweep_ranges)."""
    poses = room_poses()
    agent = np.array([b for b, *_ in ROOM_BOTS], dtype=np.uint8)
    ranges = shorten(poses, agent, room_wall_ranges())
    one = rs._P().pack_sweeps(agent, poses[:, 0].astype(np.float32), poses[:, 1].astype(np.float32), poses[:, 2].astype(np.float32), ranges)
    return np.concatenate([one] * rounds)
