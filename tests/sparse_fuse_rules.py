"""The sparse (dirty-block) fuse of include/quasar_slam.h ("sparse fuse") restated in numpy, for the tests: one simulated
rank per context, able to follow any order of calls -- writes, begin, plan, apply, abandoned fuses, changes of world,
tracking off and on, reset.  It is a simulator of the protocol, not a formula for the end result: what a rank holds after
a fuse that other ranks did not join, or after a write that landed between plan and apply, comes out of the same steps
the ranks take.  dense() is the formula, for the cases where the header promises equality.

Geometry of a grid of `size` cells a side (size a multiple of 4):
  blocks of 4 rows x 16 columns; blocks_x = ceil(size / 16), blocks_y = size / 4; a bitmap row is pitch = ceil(blocks_x / 32)
  32-bit words; block (bx, by) has id by * 32 * pitch + bx = its bit index in the bitmap; bits bx >= blocks_x of a row's last
  word are never blocks.  Lane (y & 3) * 16 + (x & 15) of a block is cell (x, y); lanes with x >= size are absent.
Payload: a rank's segment is its blocks in ascending id order, each block u32 stamps[64] then (with counters) u64 deltas[64]
  -- 768 bytes, 256 without counters --, absent lanes zero.  A counter word holds hits in the high half and misses in the
  low; deltas, and the `sent` they advance, are taken per half."""
import numpy as np

BLOCK_W, BLOCK_H, CELLS = 16, 4, 64
MAX_WORLD = 64                                             # QS_SPARSE_MAX_WORLD
_LO = np.uint64(0xffffffff)
_SH = np.uint64(32)


class Geometry:
    def __init__(self, size):
        if size < BLOCK_H or size % BLOCK_H:
            raise ValueError("size must be a positive multiple of 4")
        self.size = size
        self.blocks_x = -(-size // BLOCK_W)
        self.blocks_y = size // BLOCK_H
        self.pitch = -(-self.blocks_x // 32)
        self.words = self.blocks_y * self.pitch
        left = self.blocks_x - 32 * (np.arange(self.words, dtype=np.int64) % self.pitch)       # valid bits of each word
        self.valid = np.where(left >= 32, 0xffffffff, (1 << np.clip(left, 0, 31)) - 1).astype(np.uint32)

    def block_id(self, bx, by):
        return np.asarray(by, dtype=np.int64) * (32 * self.pitch) + np.asarray(bx, dtype=np.int64)

    def block_of_cell(self, x, y):
        return self.block_id(np.asarray(x, dtype=np.int64) // BLOCK_W, np.asarray(y, dtype=np.int64) // BLOCK_H)

    def block_xy(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        return ids % (32 * self.pitch), ids // (32 * self.pitch)

    def cells(self, ids):
        """(x int64 [n, 64], y int64 [n, 64], present bool [n, 64]) of every lane of the blocks `ids`."""
        bx, by = self.block_xy(ids)
        lane = np.arange(CELLS, dtype=np.int64)
        x = bx[:, None] * BLOCK_W + (lane & 15)[None, :]
        y = by[:, None] * BLOCK_H + (lane >> 4)[None, :]
        return x, y, x < self.size

    def bitmap(self, ids):
        """uint32 [words] with the bits `ids` set."""
        ids = np.asarray(ids, dtype=np.int64)
        bm = np.zeros(self.words, dtype=np.uint32)
        np.bitwise_or.at(bm, ids // 32, (np.uint32(1) << (ids % 32).astype(np.uint32)))
        return bm

    def ids(self, bitmap):
        """Ascending block ids of a bitmap, under the valid mask."""
        bm = np.asarray(bitmap, dtype=np.uint32).reshape(self.words) & self.valid
        w = np.nonzero(bm)[0]
        bits = (bm[w, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
        ww, bb = np.nonzero(bits)
        return (w[ww] * 32 + bb).astype(np.int64)

    def all_ids(self):
        by, bx = np.mgrid[0:self.blocks_y, 0:self.blocks_x]
        return np.sort(self.block_id(bx.ravel(), by.ravel()))


def _halves_sub(a, b):
    """per 32-bit half, with wrap-around: a - b"""
    return (((a >> _SH) - (b >> _SH)) & _LO) << _SH | ((a & _LO) - (b & _LO)) & _LO


def _halves_add(a, b):
    return (((a >> _SH) + (b >> _SH)) & _LO) << _SH | ((a & _LO) + (b & _LO)) & _LO


class ProtocolError(Exception):
    """A call the library refuses (state or argument)."""


class Rank:
    """One context.  stamps uint32 [size, size]; counts, sent, fused uint64 [size, size] (None without counters); live: the
    dirty bitmap uint32 [words] (None while tracking is off); saved: the bitmap begin took; state 0 idle / 1 begun / 2 planned."""

    def __init__(self, size, counts=True, tracking=True):
        self.geo = Geometry(size)
        self.with_counts = counts
        self.live = None
        self.reset()
        if tracking:
            self.tracking(True)

    # ---- state ---------------------------------------------------------------------------------------------------------------
    def reset(self):
        n = self.geo.size
        self.stamps = np.zeros((n, n), dtype=np.uint32)
        self.counts = np.zeros((n, n), dtype=np.uint64) if self.with_counts else None
        self.sent = np.zeros((n, n), dtype=np.uint64) if self.with_counts else None
        self.fused = np.zeros((n, n), dtype=np.uint64) if self.with_counts else None
        if self.live is not None:
            self.live = np.zeros(self.geo.words, dtype=np.uint32)
        self.saved, self.state = None, 0
        self.view_fused = False                            # counts() reads the fused counters after an apply
        self.unfused = False                               # writes no fuse has carried
        self.written = False                               # anything written since the reset
        self.world = self.rank = None
        self._lists = self._n = self._off = None

    def tracking(self, on):
        if not on:
            self.live, self.state, self.saved, self.view_fused = None, 0, None, False
            return
        if self.live is not None:
            return
        if self.unfused:
            raise ProtocolError("tracking: the grid has unfused writes")
        if self.with_counts:
            self.sent[:] = 0
            self.fused[:] = 0
        self.live = np.zeros(self.geo.words, dtype=np.uint32)
        if self.written:                                   # counters from before tracking have no bit: everything is marked once
            self.live = self.geo.bitmap(self.geo.all_ids())

    def write(self, x, y, stamp, hit):
        """Cells (x, y) written in order with stamps `stamp`; hit: the hit half counts, else the miss half."""
        x, y = np.asarray(x, dtype=np.int64).ravel(), np.asarray(y, dtype=np.int64).ravel()
        if len(x) == 0:
            return
        assert (x >= 0).all() and (x < self.geo.size).all() and (y >= 0).all() and (y < self.geo.size).all()
        np.maximum.at(self.stamps, (y, x), np.asarray(stamp, dtype=np.uint32).ravel())
        if self.with_counts:
            np.add.at(self.counts, (y, x), np.where(np.asarray(hit, dtype=bool).ravel(), np.uint64(1) << _SH, np.uint64(1)))
        if self.live is not None:
            self.live |= self.geo.bitmap(self.geo.block_of_cell(x, y))
        self.unfused = self.written = True

    def dirty_ids(self):
        return self.geo.ids(self.live)

    def grid(self):
        """OccupancyGrid values of the stamps: -1 unknown, 0 free, 100 occupied."""
        return np.where(self.stamps == 0, -1, np.where(self.stamps & 1, 100, 0)).astype(np.int8)

    def view(self):
        """(hits, misses) int32 as the counts view reads them: the fused counters after an apply, else the own."""
        c = self.fused if self.view_fused else self.counts
        return (c >> _SH).astype(np.uint32).view(np.int32), (c & _LO).astype(np.uint32).view(np.int32)

    # ---- the fuse ------------------------------------------------------------------------------------------------------------
    def begin(self, world, rank):
        """-> this rank's bitmap (slot `rank` of the array the ranks all-gather)."""
        if not (1 <= world <= MAX_WORLD and 0 <= rank < world):
            raise ProtocolError("begin: world / rank out of range")
        if self.live is None:
            raise ProtocolError("begin: tracking is off")
        if self.state != 0:                                # a fuse that never reached apply: its blocks go into this one
            self.live |= self.saved
            self.state = 0
        self.world, self.rank = world, rank
        self.saved = self.live.copy()
        self.live = np.zeros(self.geo.words, dtype=np.uint32)
        self.state = 1
        return self.saved.copy()

    def block_bytes(self):
        return CELLS * (4 + (8 if self.with_counts else 0))

    def plan(self, bitmaps):
        """bitmaps: uint32 [world, words], every rank's -> (n_blocks [world], offsets [world + 1] bytes, own segment bytes)."""
        if self.state != 1:
            raise ProtocolError("plan: begin first")
        bitmaps = np.asarray(bitmaps, dtype=np.uint32).reshape(self.world, self.geo.words)
        self._lists = [self.geo.ids(bitmaps[s]) for s in range(self.world)]
        self._n = np.array([len(l) for l in self._lists], dtype=np.int64)
        self._off = np.concatenate([[0], np.cumsum(self._n * self.block_bytes())]).astype(np.int64)
        x, y, there = self.geo.cells(self._lists[self.rank])
        xc = np.where(there, x, 0)
        seg = np.zeros((len(x), self.block_bytes()), dtype=np.uint8)
        seg[:, :CELLS * 4] = np.where(there, self.stamps[y, xc], 0).astype("<u4").view(np.uint8)
        if self.with_counts:
            d = np.where(there, _halves_sub(self.counts[y, xc], self.sent[y, xc]), np.uint64(0))
            seg[:, CELLS * 4:] = d.astype("<u8").view(np.uint8)
        self.state = 2
        return self._n.copy(), self._off.copy(), seg.reshape(-1)

    def apply(self, payload):
        """payload: every rank's segment at its offset (uint8 [offsets[world]])."""
        if self.state != 2:
            raise ProtocolError("apply: plan first")
        payload = np.asarray(payload, dtype=np.uint8)
        assert len(payload) == self._off[self.world]
        bb = self.block_bytes()
        for s in range(self.world):
            if self._n[s] == 0:
                continue
            seg = payload[self._off[s]:self._off[s + 1]].reshape(self._n[s], bb)
            x, y, there = self.geo.cells(self._lists[s])
            if s != self.rank:                             # own stamps are in place
                v = np.ascontiguousarray(seg[:, :CELLS * 4]).view("<u4")
                np.maximum.at(self.stamps, (y[there], x[there]), v[there])
            if self.with_counts:
                d = np.ascontiguousarray(seg[:, CELLS * 4:]).view("<u8")
                np.add.at(self.fused, (y[there], x[there]), d[there])
                if s == self.rank:                         # a cell occurs once in the own list
                    self.sent[y[there], x[there]] = _halves_add(self.sent[y[there], x[there]], d[there])
        self.state = 0
        self.unfused = False
        if self.with_counts:
            self.view_fused = True


def fuse(ranks):
    """One completed fuse among `ranks` (rank = position in the list) -> n_blocks."""
    W = len(ranks)
    bms = np.stack([r.begin(W, k) for k, r in enumerate(ranks)])
    plans = [r.plan(bms) for r in ranks]
    payload = np.concatenate([p[2] for p in plans])
    for r in ranks:
        r.apply(payload)
    return plans[0][0]


def dense(ranks):
    """What the header promises every rank after a fuse from equal grids: (stamps MAX, counters SUM or None)."""
    stamps = np.maximum.reduce([r.stamps for r in ranks])
    counts = np.sum([r.counts for r in ranks], axis=0, dtype=np.uint64) if ranks[0].with_counts else None
    return stamps, counts


# ---- the painter: cells -> qs_update_rays arguments ------------------------------------------------------------------------
def paint(items, seq0, res=0.5, ox=0.0, oy=0.0, size=None):
    """items: (x, y, hit) per cell, in order.  An occupied write is a zero-length valid ray at the cell centre; a free write
    a ray without a hit from the cell centre one cell to the right (its first cell is written, its last is not).  Ray k of
    a call with seq0 carries stamp ((4 * seq0 + k + 1) << 1) | occ (csrc/raycast.hip).
    -> ((rx, ry, hx, hy, valid), (x, y, stamp, hit), sequence numbers the call uses)"""
    a = np.asarray(items, dtype=np.int64).reshape(-1, 3)
    x, y, hit = a[:, 0], a[:, 1], a[:, 2] != 0
    if size is not None:
        assert not (~hit & (x >= size - 1)).any(), "no free write in the last column"
    cx, cy = ox + (x + 0.5) * res, oy + (y + 0.5) * res
    hx = np.where(hit, cx, cx + res)
    stamp = (((4 * int(seq0) + np.arange(len(a), dtype=np.int64) + 1) << 1) | hit).astype(np.uint32)
    return (cx, cy, hx, cy.copy(), hit.astype(np.uint8)), (x, y, stamp, hit), (len(a) + 3) // 4
