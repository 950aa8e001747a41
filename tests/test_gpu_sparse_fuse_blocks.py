"""The sparse (dirty-block) fuse on built block patterns: csrc/sparse_fuse.hip, the dirty marks of the grid's writers and the
three calls qs_sparse_fuse_begin / _plan / _apply against a per-rank simulator of the protocol (tests/sparse_fuse_rules.py).

N contexts of this process play N ranks, as in dist.sparse_fuse_local, but the driver keeps what that function throws away:
every rank's gathered bitmaps, n_blocks / offsets / block_bytes and the payload before and after the exchange.  After every
step -- writes, begin + all-gather, plan, exchange, apply -- every rank is compared with its model rank: raw stamps, own
counters, grid_i8(), counts(), the fused counters, dirty_blocks(), the bitmaps under the valid mask (the live one through a
checkpoint while no fuse is in flight), the own segment byte for byte after plan and the whole payload after the exchange.
The maps are painted with qs_update_rays (cells of 0.5 m from the origin: every cell centre is exact), so blocks, bitmap
words and launch sizes are chosen, not met by chance.  Every comparison is exact."""
import importlib
import struct

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import checkpoint_rules as ck
import sparse_fuse_rules as sf
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RES = 0.5
# launch sizes of csrc/sparse_fuse.hip: pack runs at most 4096 workgroups of 4 waves, apply 8192, one block per wave and trip
PACK_WAVES, APPLY_WAVES = 4096 * 4, 8192 * 4


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def distmod(pkg):
    return importlib.import_module(pkg.__name__ + ".dist")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _live_bitmap(m):
    """The live dirty bitmap as the context saves it: the DIRTY section, the seventh of a checkpoint taken with tracking on
    (refused while a fuse is in flight)."""
    data = m.checkpoint()
    kind, _, off, length = struct.unpack_from("<IIQQ", data, ck.HEADER_FIXED + 24 * (ck.DIRTY - 1))
    assert kind == ck.DIRTY
    return np.frombuffer(data, dtype="<u4", count=length // 4, offset=off)


class Ranks:
    """n contexts of one size with their model ranks.  A fuse is begin -> plan -> exchange -> apply among `parts` (context
    indices; the rank is the position), each step checked; a fuse may be left after any step (abandoned)."""

    def __init__(self, pkg, distmod, size, n, counts=True, **kw):
        self.pkg, self.dist, self.size, self.with_counts = pkg, distmod, size, counts
        self.geo = sf.Geometry(size)
        self.m = []
        try:
            for _ in range(n):
                self.m.append(pkg.QuasarMapper(size, RES, 0.0, 0.0, max_agent=1, enable_counts=counts, **kw))
                self.m[-1].dirty_tracking(True)
        except Exception:
            self.close()
            raise
        self.ad = [distmod.MapperSparseAdapter(m, DEV) for m in self.m]
        self.model = [sf.Rank(size, counts) for _ in range(n)]
        self.seq = 1
        self.bm, self.plans, self.segs = [None] * n, [None] * n, [None] * n
        self.stale = [True] * n
        self.exp = [None] * n

    def close(self):
        for m in self.m:
            m.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- writes -------------------------------------------------------------------------------------------------------------
    def write(self, i, items, seq0=None):
        """(x, y, hit) cells painted on context i; seq0: the call's first sequence number (default: after every earlier
        write of any context, so that later writes win)."""
        if len(items) == 0:
            return
        rays, w, n_seq = sf.paint(items, self.seq if seq0 is None else seq0, RES, size=self.size)
        self.m[i].update_rays(*rays, seq0=self.seq if seq0 is None else seq0)
        self.model[i].write(*w)
        if seq0 is None:
            self.seq += n_seq
        self.stale[i] = True

    def tracking(self, i, on):
        self.m[i].dirty_tracking(on)
        self.model[i].tracking(on)
        self.stale[i] = True

    def reset(self, i):
        self.m[i].reset()
        self.model[i].reset()
        self.stale[i] = True

    # ---- comparison ---------------------------------------------------------------------------------------------------------
    def _expect(self, i):
        if self.stale[i]:
            r, n = self.model[i], self.size
            e = {"stamps": torch.from_numpy(r.stamps.view(np.int32)).to(DEV), "grid": r.grid()}
            if self.with_counts:
                e["counts"] = torch.from_numpy(r.counts.view(np.int32).reshape(n, n, 2)).to(DEV)
                e["fused"] = torch.from_numpy(r.fused.view(np.int32).reshape(n, n, 2)).to(DEV)
            self.exp[i], self.stale[i] = e, False
        e = self.exp[i]
        if self.with_counts:
            e["view"] = self.model[i].view()               # (which counters the view reads changes without a write)
        return e

    def check(self, tag, which=None):
        for i in (range(len(self.m)) if which is None else which):
            m, r, e, t = self.m[i], self.model[i], self._expect(i), f"{tag}: context {i}"
            m.sync()
            st, ct = self.dist.grid_tensors(m, DEV)
            assert torch.equal(st, e["stamps"]), f"{t}: {int((st != e['stamps']).sum())} stamps differ"
            assert (m.grid_i8() == e["grid"]).all(), f"{t}: grid_i8"
            fz = self.dist.fused_counts_view(m, DEV)
            if self.with_counts:
                assert torch.equal(ct, e["counts"]), f"{t}: {int((ct != e['counts']).sum())} own counter halves differ"
                assert torch.equal(fz, e["fused"]), f"{t}: {int((fz != e['fused']).sum())} fused counter halves differ"
                h, mi = m.counts()
                assert (h == e["view"][0]).all() and (mi == e["view"][1]).all(), f"{t}: counts() view"
            else:
                assert ct is None and fz is None, f"{t}: a context without counters has no counter buffers"
            if r.live is None:                             # tracking is off: nothing to count
                with pytest.raises(self.pkg.QuasarError, match="dirty tracking is off"):
                    m.dirty_blocks()
                continue
            assert m.dirty_blocks() == (len(r.dirty_ids()), 64), f"{t}: dirty_blocks() {m.dirty_blocks()[0]}, model {len(r.dirty_ids())}"
            if r.state == 0:                               # the live bitmap, through the checkpoint's DIRTY section
                live = _live_bitmap(m)
                assert (live & self.geo.valid == r.live).all(), f"{t}: live bitmap"
            else:                                          # the bitmap begin took: this rank's row of its array
                own = _u32(self.bm[i][r.rank])
                assert (own & self.geo.valid == r.saved).all(), f"{t}: saved bitmap"

    def check_dense(self, tag, parts=None):
        """The header's promise after a fuse from equal grids: every rank holds MAX of the stamps and SUM of the counters."""
        parts = list(range(len(self.m))) if parts is None else parts
        stamps, counts = sf.dense([self.model[i] for i in parts])
        for i in parts:
            assert (self.model[i].stamps == stamps).all(), f"{tag}: model rank {i}: stamps differ from the dense fuse"
            if self.with_counts:
                assert (self.model[i].fused == counts).all(), f"{tag}: model rank {i}: counters differ from the dense fuse"

    # ---- the steps of a fuse ------------------------------------------------------------------------------------------------
    def begin(self, parts, tag, pad=False):
        """begin on every context of `parts` and the all-gather.  pad: the gathered rows arrive with every padding bit (bits
        beyond blocks_x of a row's last word) set, as a writer that marks whole nibbles may leave them."""
        W = len(parts)
        for i in parts:
            self.m[i].sync()
        for k, i in enumerate(parts):
            self.bm[i] = self.ad[i].begin(W, k)
            self.model[i].begin(W, k)
            assert tuple(self.bm[i].shape) == (W, self.geo.words)
        for i in parts:
            self.m[i].sync()
        for k, i in enumerate(parts):
            for p, j in enumerate(parts):
                if p != k:
                    self.bm[i][p].copy_(self.bm[j][p])
        torch.cuda.synchronize()
        if pad:
            padding = torch.from_numpy((~self.geo.valid).view(np.int32)).to(DEV)
            for i in parts:
                self.bm[i] |= padding[None, :]
            torch.cuda.synchronize()
        for i in parts:                                    # every rank holds every rank's bitmap
            got = _u32(self.bm[i]) & self.geo.valid[None, :]
            for p, j in enumerate(parts):
                assert (got[p] == self.model[j].saved).all(), f"{tag}: context {i}: gathered bitmap of rank {p}"
        self.check(f"{tag}: after begin", parts)

    def plan(self, parts, tag):
        W = len(parts)
        gathered = [_u32(self.bm[i]) for i in parts]
        for k, i in enumerate(parts):
            self.plans[i] = self.ad[i].plan(W)
        for i in parts:
            self.m[i].sync()
        torch.cuda.synchronize()
        for k, i in enumerate(parts):
            n, off, buf, bb = self.plans[i]
            en, eoff, eseg = self.model[i].plan(gathered[k])
            assert bb == self.model[i].block_bytes() == (768 if self.with_counts else 256), f"{tag}: block_bytes {bb}"
            assert (np.asarray(n, dtype=np.int64) == en).all(), f"{tag}: context {i}: n_blocks {n}, model {en}"
            assert (np.asarray(off, dtype=np.int64) == eoff).all(), f"{tag}: context {i}: offsets {off}, model {eoff}"
            assert (buf is None) == (eoff[W] == 0) and (buf is None or buf.numel() == eoff[W])
            if len(eseg):
                got = buf[int(eoff[k]):int(eoff[k + 1])].cpu().numpy()
                assert (got == eseg).all(), f"{tag}: context {i}: {int((got != eseg).sum())} bytes of the own segment differ"
            self.segs[i] = eseg
        self.check(f"{tag}: after plan", parts)
        return self.plans[parts[0]][0]

    def exchange(self, parts, tag):
        for k, i in enumerate(parts):
            n, off, buf, _ = self.plans[i]
            for p, j in enumerate(parts):
                if p != k and off[p + 1] > off[p]:
                    buf[int(off[p]):int(off[p + 1])].copy_(self.plans[j][2][int(off[p]):int(off[p + 1])])
        torch.cuda.synchronize()
        self.payload = np.concatenate([self.segs[i] for i in parts])
        for i in parts:
            buf = self.plans[i][2]
            if buf is not None:
                got = buf.cpu().numpy()
                assert (got == self.payload).all(), f"{tag}: context {i}: {int((got != self.payload).sum())} payload bytes differ"
        self.check(f"{tag}: after the exchange", parts)

    def apply(self, parts, tag):
        for i in parts:
            self.ad[i].apply()
            self.model[i].apply(self.payload)
            self.stale[i] = True
        for i in parts:
            self.m[i].sync()
        self.check(f"{tag}: after apply", parts)

    def fuse(self, parts=None, tag="fuse", pad=False):
        parts = list(range(len(self.m))) if parts is None else parts
        self.begin(parts, tag, pad)
        n = self.plan(parts, tag)
        self.exchange(parts, tag)
        self.apply(parts, tag)
        return np.asarray(n, dtype=np.int64)


# ---- patterns: cells chosen by the block they lie in ----------------------------------------------------------------------------
def _cells_of_blocks(geo, bx, by):
    """one cell (x, y) in each block: column 1, row 1 of the block (a 4-cell-wide last block has it)"""
    return np.asarray(bx, dtype=np.int64) * 16 + 1, np.asarray(by, dtype=np.int64) * 4 + 1


def pattern(name, size):
    """-> (x, y) of the cells rank 0 paints, or None where the size has no such pattern"""
    geo = sf.Geometry(size)
    BX, BY, mid = geo.blocks_x, geo.blocks_y, geo.blocks_y // 2
    if name == "first_last":
        return _cells_of_blocks(geo, [0, BX - 1], [0, BY - 1])
    if name == "row_wrap":                                 # the last block of the first row and the first of the second
        return _cells_of_blocks(geo, [BX - 1, 0], [0, 1]) if BY > 1 else None
    if name == "word_edge":                                # bit 31 of a bitmap word and bit 0 of the next
        if BX > 32:
            return _cells_of_blocks(geo, [31, 32], [mid, mid])
        return _cells_of_blocks(geo, [31, 0], [mid, mid + 1]) if BX == 32 else None
    if name == "block_row":
        return _cells_of_blocks(geo, np.arange(BX), np.full(BX, mid))
    if name == "block_column":                             # the last column: the partial blocks where the size has them
        return _cells_of_blocks(geo, np.full(BY, BX - 1), np.arange(BY))
    if name == "every_block":
        by, bx = np.mgrid[0:BY, 0:BX]
        return _cells_of_blocks(geo, bx.ravel(), by.ravel())
    if name == "checkerboard":
        by, bx = np.mgrid[0:BY, 0:BX]
        keep = ((bx + by) % 2 == 0).ravel()
        return _cells_of_blocks(geo, bx.ravel()[keep], by.ravel()[keep])
    if name == "block_corners":                            # the four corner cells of an interior block (of the only block at 4)
        x0, y0 = (BX // 2) * 16, mid * 4
        x1 = min(x0 + 15, size - 1)
        return np.array([x0, x1, x0, x1]), np.array([y0, y0, y0 + 3, y0 + 3])
    if name == "right_column":                             # the rightmost column of the grid
        return np.full(size, size - 1), np.arange(size)
    raise KeyError(name)


def _items(x, y, size, flip):
    """(x, y, hit): hits and free writes alternate; the last column takes hits only"""
    hit = (((x + y + flip) & 1) == 1) | (x >= size - 1)
    return np.stack([x, y, hit.astype(np.int64)], axis=1)


PATTERNS = ("first_last", "row_wrap", "word_edge", "block_row", "block_column", "every_block", "checkerboard", "block_corners",
            "right_column")
TABLE = [(size, name) for size in (4, 68, 512, 516, 1040) for name in PATTERNS if pattern(name, size) is not None]
TABLE += [(2052, name) for name in ("first_last", "block_row", "checkerboard")]        # (the read-back stays small)


# ---- a. the geometry table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,name", TABLE, ids=[f"{s}-{n}" for s, n in TABLE])
def test_geometry_table(pkg, distmod, size, name):
    """World 2, counters on.  Fuse 1: both ranks paint the pattern, at different cells of the same blocks (rank 1 one row
    off).  Fuse 2: rank 1 alone, a third cell of every block -- and the bitmaps arrive with every padding bit set, which only
    the valid masks of the list kernel keep from becoming blocks (ids of the next bitmap row among them).  Fuse 3: nothing."""
    x, y = pattern(name, size)
    geo = sf.Geometry(size)
    blocks = np.unique(geo.block_of_cell(x, y))
    with Ranks(pkg, distmod, size, 2) as R:
        R.write(0, _items(x, y, size, 0))
        R.write(1, _items(x, y ^ 1, size, 1))
        R.check("painted")
        n = R.fuse(tag="both ranks")
        assert list(n) == [len(blocks)] * 2
        R.check_dense("both ranks")
        R.write(1, _items(x, y ^ 2, size, 0))
        n = R.fuse(tag="rank 1 only, padded bitmaps", pad=True)
        assert list(n) == [0, len(blocks)]
        R.check_dense("rank 1 only")
        assert list(R.fuse(tag="nothing")) == [0, 0]
        R.check_dense("nothing")


def test_padding_bits_carried_by_an_abandoned_fuse_are_never_blocks(pkg, distmod):
    """Size 516: one valid bit in the second word of every bitmap row.  A fuse whose gathered bitmaps had the padding bits set is
    abandoned after begin: the next begin ORs the saved row, padding included, back into the live bitmap and takes it again, so
    the following fuses gather padded rows without the driver's help.  Their lists hold valid blocks only."""
    size = 516
    with Ranks(pkg, distmod, size, 2) as R:
        x, y = pattern("block_column", size)
        R.write(0, _items(x, y, size, 0))
        R.write(1, _items(x[:3] - 16, y[:3], size, 0))
        R.begin([0, 1], "abandoned", pad=True)
        R.begin([1, 0], "begun again: the padding is in the live bitmaps now", pad=False)
        R.begin([0, 1], "and again")
        n = R.plan([0, 1], "completed")
        assert list(n) == [len(x), 3]
        R.exchange([0, 1], "completed"); R.apply([0, 1], "completed")
        R.check_dense("completed")


# ---- b. the grid-stride loops of pack and apply take a second trip -----------------------------------------------------------
def test_pack_and_apply_loops_take_a_second_trip(pkg, distmod):
    size = 1040
    x, y = pattern("every_block", size)
    with Ranks(pkg, distmod, size, 2) as R:
        R.write(0, _items(x, y, size, 0))
        R.write(1, _items(x + 1, y + 2, size, 1))          # another lane of every block
        n = R.fuse(tag="every block from both ranks")
        assert n[0] == n[1] == 16900
        assert n[0] > PACK_WAVES, "pack's loop no longer takes a second trip at this size"
        assert n.sum() > APPLY_WAVES, "apply's loop no longer takes a second trip at this size"
        R.check_dense("every block from both ranks")


# ---- c. ranks with nothing to send ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,dirty", [(5, (1, 3)), (5, (4,)), (5, (0,)), (3, ()), (1, (0,)), (1, ())],
                         ids=["5-ranks_1_3", "5-rank_4", "5-rank_0", "3-none", "1-dirty", "1-clean"])
def test_empty_ranks(pkg, distmod, world, dirty):
    """apply's forward-only search over the ranks' first blocks steps over runs of empty ranks, first and last ones included"""
    size = 68
    with Ranks(pkg, distmod, size, world) as R:
        for fuse_no in range(2):                           # (the second starts from a fused state)
            for k, i in enumerate(dirty):
                x = np.array([3 + fuse_no, 66, 20 * k + 1]); y = np.array([5 * i, 67 - i, 9])
                R.write(i, _items(x, y, size, i))
            before = [r.stamps.copy() for r in R.model]
            n = R.fuse(tag=f"fuse {fuse_no}")
            assert [int(v) for v in n] == [3 if i in dirty else 0 for i in range(world)]
            if not dirty:                                  # nothing moves and nothing changes
                assert all((r.stamps == b).all() and r.state == 0 for r, b in zip(R.model, before))
            R.check_dense(f"fuse {fuse_no}")


# ---- d. one cell written by several ranks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("winner", [0, 1, 2])
def test_one_cell_from_three_ranks(pkg, distmod, winner):
    """All three ranks write cell (37, 22), each with its own mix of hits and misses; the latest stamp is rank `winner`'s and
    its occupied bit differs from rank to rank"""
    size = 68
    with Ranks(pkg, distmod, size, 3) as R:
        for i in range(3):
            hits = [1] * (i + 1) + [0] * (3 - i)
            if i == 1:
                hits = hits[::-1]                          # rank 1 ends on a hit, the others on a miss
            R.write(i, [(37, 22, h) for h in hits], seq0=100 + 10 * ((i - winner - 1) % 3))
        R.fuse(tag=f"winner {winner}")
        R.check_dense(f"winner {winner}")
        top = R.model[winner].stamps[22, 37]
        assert all(r.stamps[22, 37] == top for r in R.model) and (top & 1) == (1 if winner == 1 else 0)
        assert all(r.fused[22, 37] == (6 << 32 | 6) for r in R.model)


# ---- e. world limits and changes of world -----------------------------------------------------------------------------------------
def test_world_64(pkg, distmod):
    """QS_SPARSE_MAX_WORLD ranks (the plan of apply is a by-value kernel argument sized for it): every rank dirty in a block
    of its own and in one shared block, the last -- 4 cells wide -- where ranks 16 apart write the same cell"""
    size, world = 68, 64
    with Ranks(pkg, distmod, size, world) as R:
        for i in range(world):
            R.write(i, [((i % 5) * 16 + 2, (i // 5) * 4 + 1, i & 1), (64 + i % 4, 64 + (i // 4) % 4, 1)])
        n = R.fuse(tag="world 64")
        assert list(n) == [2] * world
        R.check_dense("world 64")


def test_refused_worlds_and_ranks(pkg, distmod):
    size = 68
    with Ranks(pkg, distmod, size, 2) as R:
        R.write(0, [(1, 1, 1)]); R.write(1, [(67, 67, 1)])
        for world, rank in ((0, 0), (65, 0), (2, 2), (2, -1), (1, 1)):
            with pytest.raises(pkg.QuasarError, match=r"qs_sparse_fuse_begin failed \(-1\)"):
                R.m[0].sparse_fuse_begin(world, rank)
        R.check("after the refusals")                      # nothing was taken
        assert list(R.fuse(tag="after the refusals")) == [1, 1]
        R.check_dense("after the refusals")


def test_world_4_then_2_then_4(pkg, distmod):
    """Four contexts fuse as world 4, contexts 1 and 0 as ranks 0 and 1 of world 2 (the per-rank arrays are reallocated), then
    all four again.  What the two exchanged never reaches the others: the expectations are the simulator's."""
    size = 516
    with Ranks(pkg, distmod, size, 4) as R:
        for i in range(4):
            R.write(i, [(515, 4 * i, 1), (100 + i, 100, 0), (7, 7, i & 1)])
        R.fuse(tag="world 4")
        R.check_dense("world 4")
        R.write(1, [(515, 515, 1), (7, 7, 0)]); R.write(0, [(512, 0, 1)]); R.write(2, [(300, 300, 1)])
        assert list(R.fuse([1, 0], tag="world 2")) == [2, 1]
        assert R.model[3].stamps[515, 515] == 0 and R.model[0].stamps[515, 515] != 0
        R.check("world 2: the contexts that stayed out", [2, 3])
        R.write(3, [(515, 515, 0 + 1)])
        assert list(R.fuse(tag="world 4 again")) == [0, 0, 1, 1]
        assert R.model[2].stamps[0, 512] == 0              # rank 0's block travelled in the fuse of two only


@pytest.mark.parametrize("case", ["after_begin", "after_plan", "old_rank_beyond_new_world"])
def test_abandoned_fuse_across_a_change_of_world(pkg, distmod, case):
    """A world-4 fuse is abandoned, two of the contexts begin a world-2 fuse under other ranks -- the saved bitmap has to be
    read before the arrays of the old world are replaced -- and abandon that too; a completed world-4 fuse carries everything.
    In the third case the contexts' old ranks (2, 3) do not exist in the new world."""
    size = 516
    with Ranks(pkg, distmod, size, 4) as R:
        for i in range(4):
            R.write(i, [(515, 8 * i, 1), (16 * 31 + 1, 40 + 4 * i, 0), (200, 200, i & 1)])
        everyone = [0, 1, 2, 3]
        R.begin(everyone, "world 4, abandoned")
        if case == "after_plan":
            R.plan(everyone, "world 4, abandoned")
        R.write(1, [(3, 3, 1)]); R.write(3, [(3, 300, 1)])      # and writes while the fuse lies abandoned
        pair = [3, 2] if case == "old_rank_beyond_new_world" else [1, 0]
        R.begin(pair, "world 2, abandoned")
        if case == "after_plan":
            R.plan(pair, "world 2, abandoned")
        R.check("abandoned twice")
        n = R.fuse(tag="world 4, completed")
        assert list(n) == [3, 4, 3, 4]
        R.check_dense("world 4, completed")


def test_tracking_off_and_on_and_reset(pkg, distmod):
    """Tracking off drops a fuse in flight and returns the counts view to the own counters; on again is refused over unfused
    writes and, after a fuse, starts the fused counters from zero with every block marked once, so the next fuse carries the
    whole map again.  A reset clears everything, a begun fuse included, and leaves tracking on."""
    size = 68
    with Ranks(pkg, distmod, size, 2) as R:
        R.write(0, [(1, 1, 1), (67, 67, 1)]); R.write(1, [(1, 1, 0), (40, 40, 1)])
        R.fuse(tag="first")
        R.write(0, [(20, 20, 1)])
        R.begin([0, 1], "begun, then tracking goes off on rank 0")
        R.tracking(0, False)
        R.check("tracking off", [0])
        with pytest.raises(pkg.QuasarError, match="dirty tracking is off"):
            R.m[0].sparse_fuse_begin(2, 0)
        with pytest.raises(pkg.QuasarError, match="unfused writes"):
            R.m[0].dirty_tracking(True)
        R.m[0].mark_fused(); R.model[0].unfused = False     # the caller's word that the write has travelled by other means
        R.tracking(0, True)
        R.check("tracking on again", [0])
        assert len(R.model[0].dirty_ids()) == 5 * 17
        n = R.fuse(tag="after tracking came back")          # rank 1 carries its abandoned begin into this one
        assert list(n) == [85, 0]
        R.write(1, [(3, 3, 1)])
        R.begin([0, 1], "begun, then reset")
        for i in (0, 1):
            R.reset(i)
        R.check("after the reset")
        R.write(0, [(66, 0, 0)]); R.write(1, [(67, 0, 1)])
        assert list(R.fuse(tag="after the reset")) == [1, 1]
        R.check_dense("after the reset")


# ---- f. contexts without counters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [68, 516])
def test_without_counters(pkg, distmod, size):
    """the COUNTS = false instantiations of pack and apply: 256-byte blocks of stamps, no fused counters"""
    with Ranks(pkg, distmod, size, 3, counts=False) as R:
        for name in ("first_last", "block_column", "block_row"):
            x, y = pattern(name, size)
            for i in range(3):
                R.write(i, _items(x[i::2], y[i::2] ^ i, size, i))
            R.fuse(tag=name)                               # (plan asserts block_bytes == 256, check that no counter buffer exists)
            R.check_dense(name)
        assert R.dist.fused_counts_view(R.m[0], DEV) is None and R.plans[0][3] == 256


# ---- g. writes that land while a fuse is in flight ---------------------------------------------------------------------------------
@pytest.mark.parametrize("when", ["before_plan", "before_apply"])
def test_writes_in_flight(pkg, distmod, when):
    """Rank 0 writes into a block the fuse has listed (a fresh cell, and a cell it carries a second time) and into a fresh
    block, after begin.  Neither lost nor counted twice: `sent` advances by the packed delta only, and one more fuse without
    further writes makes the ranks equal."""
    size = 516
    with Ranks(pkg, distmod, size, 2) as R:
        R.write(0, [(3, 3, 1), (515, 7, 1)]); R.write(1, [(100, 100, 0), (515, 6, 1)])
        late = [(4, 3, 0), (3, 3, 1), (515, 7, 1), (300, 300, 1)]
        R.begin([0, 1], when)
        if when == "before_plan":
            R.write(0, late)
            R.check("written after begin")
        n = R.plan([0, 1], when)
        assert list(n) == [2, 2]                           # the fresh block is not in this fuse
        if when == "before_apply":
            R.write(0, late)
            R.check("written after plan")
        R.exchange([0, 1], when); R.apply([0, 1], when)
        assert (R.model[1].stamps[3, 4] != 0) == (when == "before_plan") and R.model[1].stamps[300, 300] == 0
        assert len(R.model[0].dirty_ids()) == 3
        assert list(R.fuse(tag="the fuse after")) == [3, 0]
        R.check_dense("the fuse after")


# ---- h. every writer marks what it changes ---------------------------------------------------------------------------------------
def _planes(distmod, m):
    m.sync()
    st, ct = distmod.grid_tensors(m, DEV)
    return _u32(st).copy(), ct.cpu().numpy().view(np.uint64).reshape(m.size, m.size).copy()


WRITERS = ("packets_direct", "packets_tiled", "edge_rays", "update_rays", "sweeps_direct", "sweeps_tiled", "fold_range")


@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("size", [68, 516])
def test_every_writer_marks_the_blocks_it_changes(pkg, distmod, size, writer):
    """From a fused state, one call of one writer, steered into the last, partial block column.  Every cell whose stamp or
    counter changed lies in a block whose bit is set; dirty_blocks() is the popcount under the valid mask; the direct writers
    mark exactly the blocks they change."""
    P = pkg.protocol
    geo = sf.Geometry(size)
    res, half = 0.05, size * 0.025
    mode = 2 if writer.endswith("tiled") else 1
    rng = np.random.default_rng(size)
    xe = half - 0.3                                        # 6 cells from the right edge: ranges of 0.2 .. 1.2 m cross it
    with pkg.QuasarMapper(size, res, -half, -half, max_agent=1, raycast_mode=mode) as m:
        m.dirty_tracking(True)
        n0 = 64
        m.ingest_array(P.pack_packets(np.ones(n0, int), rng.uniform(-1.0, 1.0, n0), rng.uniform(-1.0, 1.0, n0), rng.uniform(-3, 3, n0),
                                      np.zeros(n0, int), np.zeros(n0, int), rng.uniform(0.2, 1.1, (n0, 4)), np.zeros(n0, int)))
        distmod.sparse_fuse_local([m], DEV)                # the fused state
        assert m.dirty_blocks()[0] == 0
        st0, ct0 = _planes(distmod, m)
        edge0 = m.counters()["edge_rays"]
        n = 300
        ys = rng.uniform(-half + 0.2, half - 0.2, n)
        if writer in ("packets_direct", "packets_tiled"):
            m.ingest_array(P.pack_packets(np.ones(n, int), rng.uniform(xe - 0.5, xe, n), ys, rng.uniform(-0.7, 0.7, n), np.zeros(n, int),
                                          np.zeros(n, int), rng.uniform(0.2, 1.2, (n, 4)), np.zeros(n, int)))
        elif writer == "edge_rays":                        # poses on cell corners, yaw 0: every ray ends on a cell edge
            # (every 0.25 m is a float32 of the wire format and a cell corner of this grid)
            lat = 0.25 * rng.integers(int((half - 0.5) * 4), int(half * 4), n)
            m.ingest_array(P.pack_packets(np.ones(n, int), lat, 0.25 * rng.integers(-int((half - 0.3) * 4), int((half - 0.3) * 4), n), np.zeros(n),
                                          np.zeros(n, int), np.zeros(n, int), rng.integers(4, 24, (n, 4)) * 0.05, np.zeros(n, int)))
        elif writer == "update_rays":
            rx = rng.uniform(xe - 0.5, xe, n)
            m.update_rays(rx, ys, rx + rng.uniform(0.1, 1.0, n), ys + rng.uniform(-0.5, 0.5, n), rng.integers(0, 2, n).astype(np.uint8))
        elif writer in ("sweeps_direct", "sweeps_tiled"):
            ns = 6
            m.ingest_sweeps(P.pack_sweeps(np.ones(ns, int), np.full(ns, xe), np.linspace(-half + 1.0, half - 1.0, ns),
                                          rng.uniform(-0.3, 0.3, ns), rng.uniform(0.2, 1.2, (ns, 181))))
        else:                                              # the local fold of a peer's copy: a cell range that starts and ends
            y0, y1 = 5, size - 6                           # inside block rows (offset and length in fours, as the call asks)
            lo, hi = y0 * size + size - 4, y1 * size + 4
            peer_st = np.zeros(size * size, dtype=np.int32); peer_ct = np.zeros((size * size, 2), dtype=np.int32)
            k = np.unique(np.concatenate([[lo, hi - 1], rng.integers(lo, hi, 200), np.arange(y0 + 1, y1) * size + size - 1]))
            peer_st[k] = (1 << 29) + np.arange(len(k)); peer_ct[k] = rng.integers(1, 9, (len(k), 2))
            d_st, d_ct = torch.from_numpy(peer_st[lo:hi].copy()).to(DEV), torch.from_numpy(peer_ct[lo:hi].copy()).to(DEV)
            m.fuse_buffers_range([d_st.data_ptr()], [d_ct.data_ptr()], lo, hi - lo)
        m.sync()
        st1, ct1 = _planes(distmod, m)
        if writer == "edge_rays":
            assert m.counters()["edge_rays"] - edge0 == 4 * n, "the stream was to be cast by the exact-trig path alone"
        changed = (st1 != st0) | (ct1 != ct0)
        assert changed[:, size - size % 16:].any(), "no cell of the partial block column changed: the test is empty"
        assert changed[:, size - 1].any()
        raw = _live_bitmap(m)
        marked = set(geo.ids(raw).tolist())
        cy, cx = np.nonzero(changed)
        touched = set(np.unique(geo.block_of_cell(cx, cy)).tolist())
        assert touched <= marked, f"{len(touched - marked)} blocks changed without a mark: {sorted(touched - marked)[:8]}"
        assert m.dirty_blocks() == (len(marked), 64)
        if writer in ("packets_direct", "update_rays", "sweeps_direct", "edge_rays"):
            assert marked == touched, f"{len(marked - touched)} blocks marked without a change"
        if writer == "fold_range":                         # the fold marks whole block rows, and keeps the padding bits clear
            assert not (raw & ~geo.valid).any()
            assert marked == set(geo.block_id(*np.meshgrid(np.arange(geo.blocks_x), np.arange(y0 // 4, y1 // 4 + 1))).ravel().tolist())
