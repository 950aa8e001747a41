"""tests/sparse_fuse_rules.py held to facts it was not written from: the header's equality promise (a completed fuse from
equal grids == MAX of the stamps, SUM of the counters), the repair of an abandoned fuse by the next one, sent <= counts, the
block layout tests/checkpoint_rules.py states for the same sizes, and the oracle's update_rays for the painter."""
import numpy as np
import pytest

import checkpoint_rules as ck
import sparse_fuse_rules as sf
from oracle import oracle as orc

SIZES = (4, 68, 512, 516, 1040, 2052)                     # the geometry table of tests/test_gpu_sparse_fuse_blocks.py
WORLDS = (1, 2, 3, 7)


def _random_items(geo, rng, n=120):
    """(x, y, hit) over a few blocks chosen at random, plus the blocks where the geometry can go wrong; free writes keep
    out of the last column."""
    size = geo.size
    ids = rng.choice(geo.all_ids(), size=min(6, geo.blocks_x * geo.blocks_y), replace=False)
    bx, by = geo.block_xy(ids)
    bx = np.concatenate([bx, [geo.blocks_x - 1, 0, min(31, geo.blocks_x - 1), min(32, geo.blocks_x - 1)]])
    by = np.concatenate([by, [0, min(1, geo.blocks_y - 1), geo.blocks_y - 1, geo.blocks_y - 1]])
    k = rng.integers(0, len(bx), n)
    x = np.minimum(bx[k] * 16 + rng.integers(0, 16, n), size - 1)
    y = by[k] * 4 + rng.integers(0, 4, n)
    hit = (rng.random(n) < 0.4) | (x == size - 1)
    return np.stack([x, y, hit], axis=1)


def _write(rank, items, seq0):
    _, w, n_seq = sf.paint(items, seq0, size=rank.geo.size)
    rank.write(*w)
    return seq0 + n_seq


def _assert_dense(ranks, tag):
    stamps, counts = sf.dense(ranks)
    for k, r in enumerate(ranks):
        assert (r.stamps == stamps).all(), f"{tag}: rank {k}: stamps"
        assert (r.fused == counts).all(), f"{tag}: rank {k}: fused counters"
        assert ((r.sent >> 32) <= (r.counts >> 32)).all() and ((r.sent & 0xffffffff) <= (r.counts & 0xffffffff)).all(), tag
        assert (r.sent == r.counts).all(), f"{tag}: rank {k}: everything written has been sent"
        assert r.state == 0 and len(r.dirty_ids()) == 0


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("size", SIZES)
def test_a_completed_fuse_from_equal_grids_is_the_dense_fuse(size, world):
    rng = np.random.default_rng(size * 100 + world)
    ranks = [sf.Rank(size) for _ in range(world)]
    seq = 1
    for rnd in range(2):                                   # the second round starts from a fused state
        for r in ranks[:world if rnd == 0 else max(1, world - 1)]:     # ... in which the last rank has nothing to send
            seq = _write(r, _random_items(r.geo, rng), seq)
        own = [len(r.dirty_ids()) for r in ranks]
        n = sf.fuse(ranks)
        assert list(n) == own
        _assert_dense(ranks, f"round {rnd}")
    assert list(sf.fuse(ranks)) == [0] * world             # nothing written since: nothing moves
    _assert_dense(ranks, "empty fuse")


@pytest.mark.parametrize("after", ["begin", "plan"])
@pytest.mark.parametrize("size", (68, 516))
def test_an_abandoned_fuse_is_repaired_by_the_next(size, after):
    rng = np.random.default_rng(size)
    ranks = [sf.Rank(size) for _ in range(3)]
    seq = 1
    for r in ranks:
        seq = _write(r, _random_items(r.geo, rng), seq)
    before = [(r.stamps.copy(), r.counts.copy(), r.sent.copy(), r.fused.copy(), r.dirty_ids()) for r in ranks]
    bms = np.stack([r.begin(3, k) for k, r in enumerate(ranks)])
    if after == "plan":
        for r in ranks:
            r.plan(bms)
    for r, b in zip(ranks, before):                        # only apply commits
        assert (r.stamps == b[0]).all() and (r.counts == b[1]).all() and (r.sent == b[2]).all() and (r.fused == b[3]).all()
        assert len(r.dirty_ids()) == 0 and r.state == (1 if after == "begin" else 2)
    seq = _write(ranks[1], _random_items(ranks[1].geo, rng), seq)      # and a write while the fuse lies abandoned
    order = [ranks[2], ranks[0], ranks[1]]                 # the next fuse: other ranks, same world
    n = sf.fuse(order)
    assert list(n[:2]) == [len(before[2][4]), len(before[0][4])] and n[2] >= len(before[1][4])
    _assert_dense(ranks, "after the repair")


def test_writes_in_flight_are_neither_lost_nor_counted_twice():
    size = 516
    for when in ("before_plan", "before_apply"):
        a, b = sf.Rank(size), sf.Rank(size)
        seq = _write(a, [(3, 3, 1), (515, 7, 1)], 1)
        seq = _write(b, [(100, 100, 0)], seq)
        bms = np.stack([a.begin(2, 0), b.begin(2, 1)])
        late = [(4, 3, 0), (3, 3, 1), (300, 300, 1)]      # a listed block (one cell of it a second time) and a fresh one
        if when == "before_plan":
            seq = _write(a, late, seq)
        pa, pb = a.plan(bms), b.plan(bms)
        if when == "before_apply":
            seq = _write(a, late, seq)
        payload = np.concatenate([pa[2], pb[2]])
        a.apply(payload); b.apply(payload)
        assert list(pa[0]) == [2, 1]
        assert b.stamps[300, 300] == 0 and a.stamps[300, 300] != 0      # the fresh block was not listed
        assert (b.stamps[3, 4] != 0) == (when == "before_plan")          # pack reads the grid as it stands at plan
        assert len(a.dirty_ids()) == 2 and (a.sent <= a.counts).all()
        sf.fuse([a, b])
        _assert_dense([a, b], when)


def test_change_of_world_with_an_abandoned_fuse_between():
    size = 68
    ranks = [sf.Rank(size) for _ in range(4)]
    rng = np.random.default_rng(5)
    seq = 1
    for r in ranks:
        seq = _write(r, _random_items(r.geo, rng), seq)
    bms = np.stack([r.begin(4, k) for k, r in enumerate(ranks)])
    ranks[2].plan(bms)
    ranks[3].begin(2, 1); ranks[2].begin(2, 0)             # abandoned at world 4, begun at world 2, abandoned again
    sf.fuse(ranks)
    _assert_dense(ranks, "world 4 after the abandoned fuses")
    # a completed fuse of two of the four: the two agree, the others have not seen it; the next fuse of all four does not
    # carry it (the header promises equality only from equal grids)
    seq = _write(ranks[1], [(1, 1, 1)], seq)
    sf.fuse([ranks[1], ranks[0]])
    assert ranks[0].stamps[1, 1] == ranks[1].stamps[1, 1] != 0 and ranks[2].stamps[1, 1] == 0
    sf.fuse(ranks)
    assert ranks[2].stamps[1, 1] == 0


def test_refusals_tracking_and_reset():
    r = sf.Rank(68, tracking=False)
    with pytest.raises(sf.ProtocolError):
        r.begin(1, 0)
    _write(r, [(67, 0, 1)], 1)
    with pytest.raises(sf.ProtocolError):
        r.tracking(True)                                   # unfused writes
    r.reset(); r.tracking(True)
    for world, rank in ((0, 0), (65, 0), (2, 2), (2, -1)):
        with pytest.raises(sf.ProtocolError):
            r.begin(world, rank)
    with pytest.raises(sf.ProtocolError):
        r.plan(np.zeros((1, r.geo.words), np.uint32))
    _write(r, [(67, 0, 1), (0, 67, 0)], 1)
    assert list(r.dirty_ids()) == [4, 16 * 32]
    sf.fuse([r])
    assert r.view()[0][0, 67] == 1 and r.view()[1][67, 0] == 1
    r.tracking(False)                                      # the view returns to the own counters; on again: everything is marked once
    assert r.view()[0][0, 67] == 1 and not r.view_fused
    r.tracking(True)
    assert len(r.dirty_ids()) == r.geo.blocks_x * r.geo.blocks_y and not r.fused.any()
    sf.fuse([r])
    assert (r.fused == r.counts).all()
    r.reset()
    assert not r.stamps.any() and not r.counts.any() and r.state == 0 and len(r.dirty_ids()) == 0
    no = sf.Rank(68, counts=False)
    no.write([5], [5], [7], [1])
    n, off, seg = no.plan(no.begin(1, 0)[None])
    assert no.block_bytes() == 256 and list(off) == [0, 256] and seg.view("<u4")[(5 & 3) * 16 + 5] == 7 and no.fused is None


@pytest.mark.parametrize("size", SIZES)
def test_geometry_agrees_with_the_checkpoint_rules(size):
    geo = sf.Geometry(size)
    assert (geo.blocks_x, geo.blocks_y, geo.pitch, geo.words) == ck.geometry(size)
    assert (geo.valid == ck.bitmap_of(np.ones((geo.blocks_y, geo.blocks_x), dtype=bool), size)).all()
    ids = geo.all_ids()
    assert len(ids) == geo.blocks_x * geo.blocks_y and (np.diff(ids) > 0).all()
    rng = np.random.default_rng(size)
    some = np.unique(np.concatenate([ids[[0, -1, geo.blocks_x - 1, min(len(ids) - 1, geo.blocks_x)]], rng.choice(ids, min(len(ids), 40))]))
    x, y, there = geo.cells(some)
    for k, bid in enumerate(some):
        cells, inside = ck.block_cells(int(bid), size)
        assert (inside == there[k]).all() and (cells[inside] == (y[k] * size + x[k])[inside]).all()
        assert (geo.block_of_cell(x[k][there[k]], y[k][there[k]]) == bid).all()
    bits = rng.random((geo.blocks_y, geo.blocks_x)) < 0.3
    bm = ck.bitmap_of(bits, size)
    by, bx = np.nonzero(bits)
    assert (geo.bitmap(geo.block_id(bx, by)) == bm).all()
    assert (geo.ids(bm | ~geo.valid) == np.sort(geo.block_id(bx, by))).all()          # padding bits are never blocks
    assert (ck.dirty_bits(geo.bitmap(geo.ids(bm)), size) == bits).all()


@pytest.mark.parametrize("size", (4, 68, 516))
def test_the_painter_writes_what_the_oracle_writes(size):
    rng = np.random.default_rng(size)
    geo = sf.Geometry(size)
    items = np.concatenate([_random_items(geo, rng, 300), [(size - 1, 0, 1), (0, size - 1, 0), (size - 2, size - 1, 0)]])
    for res, ox, oy in ((0.5, 0.0, 0.0), (0.05, -size * 0.025, -size * 0.025)):
        rays, w, n_seq = sf.paint(items, 9, res, ox, oy, size=size)
        assert n_seq == (len(items) + 3) // 4 and w[2][0] == ((4 * 9 + 1) << 1 | int(items[0][2]))
        r = sf.Rank(size)
        r.write(*w)
        o = orc.OracleMapper(size, res, ox, oy, 0.0, max_agent=1)
        o.update_rays(*rays)
        hits, misses = r.view()
        assert (r.grid() == o.grid).all() and (hits == o.hits).all() and (misses == o.misses).all()
        assert hits.sum() + misses.sum() == len(items)
