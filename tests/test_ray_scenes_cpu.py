"""The built raycast scenes (tests/ray_scenes.py) reach the cases they are named for.  Every scene is fed to the CPU oracle and
restated in integers from the oracle's poses and end cells; the assertions below are conditions on the SCENES (if one fails,
the scene is wrong, never the bound).  tests/test_gpu_raycast_edges.py then runs the same bytes through the HIP kernels."""

import numpy as np
import pytest

import ray_scenes as rs
from oracle import oracle as orc


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name):
        if name not in cache:
            sc = rs.get(name)
            o = rs.feed_oracle(sc)
            cache[name] = (sc, o, rs.restate(sc, o))
        return cache[name]
    return get


def _front(sc, st, tag_prefix):
    """Live-ray indices of the front rays of the packets whose tag starts with tag_prefix."""
    pk = np.nonzero(np.char.startswith(sc.tags.astype(str), tag_prefix))[0]
    return np.nonzero(np.isin(st.slot, 4 * pk))[0]


@pytest.mark.parametrize("name", rs.names())
def test_every_end_point_keeps_clear_of_the_cell_edges(restated, name):
    """>= MARGIN (1e-3 cell) from every cell edge: the exact-trig mode (1e-9 + 1e-14 |q|) defers no ray to the host, and no
    last-bit difference between the device's and libm's sin / cos can move an end point into another cell."""
    sc, o, st = restated(name)
    assert len(st.margin) > 0 and st.margin.min() >= rs.MARGIN, (name, st.margin.min(), int(st.margin.argmin()))
    if sc.kind == "packets" and not name.startswith(("corner", "edges", "threshold")):
        assert st.margin.min() > 0.19                       # axis rays: end points within 1e-5 cell of a centre or at .2 / .3
    assert o.n_rays == len(st.x0)


def test_cell_centres_follow_truncation_toward_zero():
    g = rs.Geo("S", 64)
    o = g.oracle()
    cells = np.array([-64, -2, -1, 0, 1, 63, 64, 127])
    assert (o.world_to_grid(g.at_q(g.centre_q(cells)).astype(np.float64)) == cells).all()
    assert g.centre_q(-1) == -1.5 and g.centre_q(0) == 0.5
    assert o.world_to_grid(g.at_q([-0.5, 0.5, -1.5]).astype(np.float64)).tolist() == [0, 0, -1]


def test_restated_bresenham_equals_the_oracles_on_the_oblique_rays(restated):
    n = 0
    for name in ("threshold-L", "threshold-F", "corner", "edges-L-128", "edges-S-68"):
        sc, o, st = restated(name)
        for r in np.nonzero((st.dx > 0) & (st.dy > 0))[0]:
            want = orc.bresenham(int(st.x0[r]), int(st.y0[r]), int(st.x1[r]), int(st.y1[r]))
            assert st.cells(r) == [tuple(v) for v in want.tolist()]
            n += 1
    assert n > 500


def test_stored_oblique_constants_are_what_the_search_finds():
    for (kind, dx, dy), (yaw, d) in rs.OBLIQUE.items():
        g = rs.Geo(kind, 132)
        assert float(np.float32(yaw)) == yaw and float(np.float32(d)) == d
        assert rs.oblique_ok(g, *rs.OBLIQUE_POSE, yaw, d, dx, dy)
        assert rs.search_oblique(g, *rs.OBLIQUE_POSE, dx, dy) == (yaw, d)
    assert {k[1:] for k in rs.OBLIQUE if k[0] == "F"} == {(63, 63), (63, 62), (64, 1), (1, 64), (63, 64)}
    assert {k[1:] for k in rs.OBLIQUE if k[0] == "L"} == {(64, 1), (1, 64)}          # the others are > 76.8 cells long


@pytest.mark.parametrize("kind", ["L", "F"])
def test_threshold(restated, kind):
    sc, o, st = restated("threshold-" + kind)
    seen = set()
    for k in (62, 63, 64, 65):
        for h, (ux, uy) in enumerate(rs.DIR4):
            for c in (0, 1, 63, 64, 65):
                (r,) = _front(sc, st, f"axis k={k} h={h} c={c}")
                assert (st.dx[r], st.dy[r]) == ((k, 0) if ux else (0, k))
                lo = min(st.x0[r], st.x1[r]) if ux else min(st.y0[r], st.y1[r])
                assert lo == c and st.valid[r]
                assert st.binned[r] == (k < 64) and st.direct[r] == (k >= 64)
                n_rec = int((st.rec_ray == r).sum())
                assert n_rec == (0 if k >= 64 else 1 + ((c >> 6) != ((c + k) >> 6)))
                seen.add((k, c, n_rec))
    assert (63, 0, 1) in seen and (63, 1, 2) in seen and (64, 0, 0) in seen       # 0->63: one tile; 1->64: two; 64 cells: direct
    want = {(64, 1), (1, 64)} if kind == "L" else {(63, 63), (63, 62), (64, 1), (1, 64), (63, 64)}
    for dx, dy in want:
        (r,) = _front(sc, st, f"oblique {dx},{dy}")
        assert (st.dx[r], st.dy[r]) == (dx, dy) and st.valid[r]
        assert st.binned[r] == (dx < 64 and dy < 64)
        if st.binned[r]:
            assert int((st.rec_ray == r).sum()) == 4                               # from cell (2, 2): a full 2 x 2 box


def test_corner(restated):
    sc, o, st = restated("corner")
    assert len(sc.data) == 36 * 10 * 3 and st.binned.all()
    front = st.slot % 4 == 0
    # every pose cell of the 6 x 6 block, every heading
    assert {(int(x), int(y)) for x, y in zip(st.x0[front], st.y0[front])} == {(x, y) for x in range(61, 67) for y in range(61, 67)}
    assert set(np.maximum(st.dx, st.dy)[front].tolist()) >= {4, 11, 19, 3, 8, 13}       # axis: k; diagonals: int(k / sqrt 2 + 0.5)
    per_ray = np.bincount(st.rec_ray, minlength=len(st.x0))
    assert set(per_ray.tolist()) == {1, 2, 4}                                            # 1 x 1, 1 x 2 / 2 x 1 and 2 x 2 boxes
    cellless = st.cellless_records()
    assert len(cellless) >= 20, "no ray has a record in a tile where it has no cell"
    for r, t in cellless[:50]:
        assert per_ray[r] == 4 and len({(x >> 6, y >> 6) for x, y in st.cells(r)}) in (2, 3)
    # a pure diagonal through the corner (63,63) -> (64,64) has cells in two tiles and records in four
    diag = [r for r, _ in cellless if st.dx[r] == st.dy[r]]
    assert len(diag) > 0


@pytest.mark.parametrize("kind,size", rs.EDGE_GEOMETRIES)
def test_edges(restated, kind, size):
    sc, o, st = restated(f"edges-{kind}-{size}")
    tags = sc.tags.astype(str)
    last = size - 1
    kmax = 63 if kind == "L" else 19
    inside = lambda x, y: (0 <= x) & (x < size) & (0 <= y) & (y < size)

    def fronts(prefix):
        r = _front(sc, st, prefix)
        assert len(r) > 0, prefix
        return r
    r = fronts("out-in hit on the edge cell")
    assert len(r) == 12 and (~inside(st.x0[r], st.y0[r])).all() and inside(st.x1[r], st.y1[r]).all() and st.valid[r].all()
    assert ((st.x1[r] == 0) | (st.y1[r] == 0) | (st.x1[r] == last) | (st.y1[r] == last)).all()
    assert set(np.maximum(st.dx[r], st.dy[r]).tolist()) == {st.geo.short, st.geo.short + 4, kmax} and st.binned[r].all()
    assert st.x0.min() == -kmax and st.y0.min() == -kmax and st.x0.max() == last + kmax and st.y0.max() == last + kmax
    r = fronts("out-in hit inside")
    assert inside(st.x1[r], st.y1[r]).all() and (st.direct[r].any() == (kind == "L"))
    r = fronts("both out: ends one cell short")
    assert (~st.inbox[r]).all() and (((st.x1[r] == -1) | (st.y1[r] == -1) | (st.x1[r] == size) | (st.y1[r] == size))).all()
    r = fronts("in-out: hit not written")
    assert inside(st.x0[r], st.y0[r]).all() and (~inside(st.x1[r], st.y1[r])).all() and st.valid[r].all() and st.binned[r].all()
    r = fronts("past the corner")
    assert len(r) == 4 and st.binned[r].all() and (st.dx[r] == 4).all() and (st.dy[r] == 4).all()
    for q in r:
        assert st.written_cells(q) == [] and not inside(st.x0[q], st.y0[q]) and not inside(st.x1[q], st.y1[q])
    r = fronts("corner out-in diagonal")
    assert len(r) == 4 and inside(st.x1[r], st.y1[r]).all() and ((st.dx[r] == 5) & (st.dy[r] == 5)).all()
    assert (~inside(st.x0[r], st.y0[r])).all()
    kfar = 63 if kind == "L" else 17
    for axis, tag in ((0, "far corner out-in x"), (1, "far corner out-in y")):
        r = fronts(tag)
        assert len(r) == 4 and st.binned[r].all() and st.valid[r].all() and (~inside(st.x0[r], st.y0[r])).all()
        assert ((st.dx[r], st.dy[r])[axis] == kfar).all() and ((st.dx[r], st.dy[r])[1 - axis] == 2).all()
        assert (np.isin(st.x1[r], (0, last)) & np.isin(st.y1[r], (0, last))).all()       # the hit is on the corner cell
        assert all(len(st.written_cells(q)) >= 1 for q in r)
    # poses at q = -1.5 (cell -1), -0.5 and +0.5 (both cell 0), size - 0.5 (last cell), size + 0.5 (cell `size`)
    for q, cell in ((-1.5, -1), (-0.5, 0), (0.5, 0), (size - 0.5, last), (size + 0.5, size)):
        rx = np.nonzero(np.isin(st.slot // 4, np.nonzero(tags == f"pose qx={q}")[0]))[0]
        ry = np.nonzero(np.isin(st.slot // 4, np.nonzero(tags == f"pose qy={q}")[0]))[0]
        assert len(rx) == 16 and len(ry) == 16 and (st.x0[rx] == cell).all() and (st.y0[ry] == cell).all()
    rd = np.nonzero(np.isin(st.slot // 4, np.nonzero(tags == "pose qx=qy=-0.5")[0]))[0]
    assert (st.x0[rd] == 0).all() and (st.y0[rd] == 0).all()
    # the map has something in it and the partial tiles (sizes 68, 132) are written
    assert (o.grid != -1).sum() > 100
    if size % 64:
        assert (o.grid[:, size - size % 64:] != -1).any() and (o.grid[size - size % 64:, :] != -1).any()
    assert st.rec_off.min() >= -kmax and st.rec_off.max() <= 63 + kmax


def test_edges_record_offsets_reach_plus_126_and_minus_63(restated):
    sc, o, st = restated("edges-L-128")
    for tag, col, want, tile in (("offset +126 x", 0, 126, (1, 1)), ("offset +126 y", 1, 126, (1, 1)),
                                 ("offset -63 x", 0, -63, (0, 0)), ("offset -63 y", 1, -63, (0, 0))):
        (r,) = _front(sc, st, tag)
        (j,) = np.nonzero(st.rec_ray == r)[0]                       # one record: the tile is chosen after clamping to the grid
        assert st.binned[r] and st.rec_off[j, col] == want, (tag, st.rec_off[j])
        assert st.valid[r] and len(st.written_cells(r)) == 1        # only the hit on the edge cell is inside
    assert st.rec_off.max() == 126 and st.rec_off.min() == -63
    assert -128 <= st.rec_off.min() and st.rec_off.max() <= 127


def _writers(st, cell):
    """(ray, occupied) of every write of `cell`, in arrival order."""
    out = []
    for r in range(len(st.x0)):
        w = st.written_cells(r)
        if cell in w:
            out.append((r, bool(st.valid[r]) and (int(st.x1[r]), int(st.y1[r])) == cell))
    return out


@pytest.mark.parametrize("variant", ["adjacent", "chunks"])
@pytest.mark.parametrize("last_is_hit", [True, False])
def test_order(restated, variant, last_is_hit):
    sc, o, st = restated(f"order-{variant}-{'hit' if last_is_hit else 'free'}")
    assert len(sc.data) >= 1100 and st.binned.all() and (st.rec_tile == 0).all()
    assert st.tile_count[0] == 4 * len(sc.data) and st.items[0] >= 3
    w = _writers(st, rs.ORDER_CELL)
    assert w[-1][1] == last_is_hit and w[-2][1] != last_is_hit
    assert int(o.grid[rs.ORDER_CELL[1], rs.ORDER_CELL[0]]) == (100 if last_is_hit else 0)
    pos = {int(r): p for p, r in enumerate(st.tile_records(0))}
    p_last, p_prev = pos[w[-1][0]], pos[w[-2][0]]
    if variant == "adjacent":
        assert len(w) == len(sc.data)
        assert p_last - p_prev == 4 and p_last // 8 == p_prev // 8                  # one 8-record group: adjacent lanes of a wave
        assert sum(1 for _, occ in w if occ) == len(sc.data) // 2
    else:
        assert p_prev // rs.CHUNK == 0 and p_last // rs.CHUNK == 2                   # loser in chunk 0, winner in chunk 2 ...
        assert rs.CHUNK - p_prev % rs.CHUNK > 256 and p_last % rs.CHUNK > 256        # ... both far from a chunk border
        runs = st.raster_runs()
        assert len(runs) == 3 and all(run == [(0, 1, False)] for run in runs)        # ... and in different workgroups
    for split in (1, 255, 256, 257):
        a, b = rs.restate(sc, o, 0, 4 * split), rs.restate(sc, o, 4 * split, None)
        assert len(a.x0) == 4 * split and len(a.x0) + len(b.x0) == len(st.x0)


@pytest.mark.parametrize("n", rs.UNITS_N)
def test_units(restated, n):
    sc, o, st = restated(f"units-{n}")
    assert len(sc.data) == n and st.binned.all()
    assert st.tile_count[st.tile(1, 0)] == n and st.tile_count[st.tile(0, 0)] == 4 * n
    assert st.tile_count.sum() == 5 * n
    crossing = np.bincount(st.rec_ray, minlength=4 * n) == 2
    assert (crossing == (np.arange(4 * n) % 4 == 0)).all()                          # the front ray and only it
    assert st.items[st.tile(1, 0)] == (n + 2047) // 2048


def test_units_maps_differ_with_n():
    grids = [rs.feed_oracle(rs.get(f"units-{n}")).misses for n in (1, 7, 8, 9)]
    assert all((a != b).any() for a, b in zip(grids, grids[1:]))


def test_counters(restated):
    sc, o, st = restated("counters")
    px, py = rs.COUNTERS_POSE
    assert len(sc.data) == 16385 and int(o.misses[py, px]) == 65540 > 65535
    assert st.binned.all() and (st.rec_tile == 0).all() and st.items[0] == 33 > rs.FLUSH_ITEMS
    # one item per workgroup by default: 33 workgroups share the tile, none exclusively
    assert st.raster_runs() == [[(0, 1, False)]] * 33
    assert st.raster_runs(1) == [[(0, 33, True)]]                                   # one run of 33 items: the flush after 31
    assert st.raster_runs(2) == [[(0, 17, False)], [(0, 16, False)]]
    assert st.raster_runs(3) == [[(0, 11, False)]] * 3
    # what 33 items without a flush would do to a 16-bit counter
    assert 33 * rs.CHUNK > 65535 >= rs.FLUSH_ITEMS * rs.CHUNK


def test_runs(restated):
    sc, o, st = restated("runs")
    t = {k: st.tile(*v) for k, v in rs.RUNS_TILES.items()}
    assert st.geo.tiles_x == 9 and sorted(np.nonzero(st.tile_count)[0].tolist()) == sorted(t.values())
    assert st.tile_count[t["middle"]] == 4 * rs.RUNS_MIDDLE_N > rs.CHUNK and st.items[t["middle"]] == 2
    assert st.n_items == 7 and st.binned.all()
    order = [t["first"], t["partial_x"], t["middle"], t["last_full"], t["partial_y"], t["partial_xy"]]
    assert order == sorted(order)
    assert st.raster_runs() == [[(order[0], 1, True)], [(order[1], 1, True)], [(order[2], 1, False)], [(order[2], 1, False)],
                                [(order[3], 1, True)], [(order[4], 1, True)], [(order[5], 1, True)]]
    # one workgroup: tile changes inside the run, empty tiles skipped
    assert st.raster_runs(1) == [[(order[0], 1, True), (order[1], 1, True), (order[2], 2, True), (order[3], 1, True),
                                  (order[4], 1, True), (order[5], 1, True)]]
    # two: the second run starts after empty tiles (the binary search over equal chunk_base entries)
    two = st.raster_runs(2)
    assert [v[0] for v in two[1]] == order[3:] and st.chunk_base[order[3]] == st.chunk_base[order[3] - 1] == 4
    # three: the middle tile is split between workgroups 0 and 1 (atomic merge), the others are exclusive
    three = st.raster_runs(3)
    assert three[0][-1] == (order[2], 1, False) and three[1][0] == (order[2], 1, False) and three[1][1] == (order[3], 1, True)
    # the partial tiles: rays that run over the grid's far edge
    for tag in ("partial_x leaves", "partial_y leaves free"):
        (r,) = _front(sc, st, tag)
        assert st.binned[r] and max(st.x1[r], st.y1[r]) >= 520 and len(st.written_cells(r)) == 5
    assert (o.grid[:, 512:] != -1).any() and (o.grid[512:, :] != -1).any()


@pytest.mark.parametrize("n,per,nwg,R", [(255, 256, 1, 1), (256, 256, 1, 1), (257, 256, 2, 1), (4096, 256, 16, 1), (4097, 256, 17, 2),
                                         (131072, 256, 512, 32), (131073, 320, 410, 26)])
def test_decomp(restated, n, per, nwg, R):
    assert rs.packet_decomposition(n) == (per, nwg, R) and per % 64 == 0 and per >= 256
    sc, o, st = restated(f"decomp-{n}")
    assert len(sc.data) == n
    acc = rs.accepted_mask(sc)
    assert np.nonzero(~acc)[0].tolist() == sc.meta["rejected"] == sorted({s for s in (255, 256, n - 1) if s < n})
    assert o.n_rays == 4 * int(acc.sum())
    assert (st.tile_count > 0).all() and len(st.tile_count) == 4                    # all four tiles
    front = st.slot % 4 == 0
    assert 0.4 < st.valid[front].mean() < 0.6                                       # hit and free fronts alternate
    assert (~st.inbox).sum() == 0 and st.binned.all()
    assert [rs.packet_decomposition(split)[1] for split in (1, 255, 256, 257)] == [1, 1, 1, 2]     # the split ingests' first parts


def test_many_tiles(restated):
    sc, o, st = restated("many_tiles")
    assert st.geo.tiles_x == 33 and st.geo.n_tiles == 1089 > 1024
    assert (st.geo.n_tiles + 1023) // 1024 == 2                                     # pass B2: two tiles per thread
    for t in rs.MANY_TILES:
        assert st.tile_count[t] >= 5, t
    assert st.geo.size - 64 * 32 == 4 and st.tile_count[1088] >= 5 and (o.grid[2048:, 2048:] != -1).sum() >= 8    # the 4 x 4 tile
    assert (o.grid[2048:, :2048] != -1).any() and (o.grid[:2048, 2048:] != -1).any()


@pytest.mark.parametrize("kind", ["S", "L"])
@pytest.mark.parametrize("n", rs.SWEEPS_N)
def test_sweeps(restated, kind, n):
    sc, o, st = restated(f"sweeps-{kind}-{n}")
    n_acc = n - (1 if n > 1 else 0)
    assert len(st.x0) == 181 * n_acc and st.n_slots == 184 * n
    assert rs.sweep_decomposition(n)[1] == (2 if n == 17 else 1)
    assert {(int(x), int(y)) for x, y in zip(st.x0, st.y0)} == set(rs.SWEEP_CELLS[:max(1, min(n, 4))]) - \
        ({rs.SWEEP_CELLS[n // 2]} if 1 < n <= 4 else set())
    axis = np.isin(st.slot % 184, (0, 90, 180))
    assert ((st.dx[axis] == 0) | (st.dy[axis] == 0)).all()
    if kind == "L":
        longest = np.maximum(st.dx, st.dy)
        assert set(longest[axis & st.valid].tolist()) <= {63, 64}
        if n >= 15:
            assert set(longest[axis & st.valid].tolist()) == {63, 64}
        assert st.binned.any() and st.direct.any() and (~st.valid).any()
        assert longest[st.valid].max() == 64
    else:
        assert st.binned.all()
    # the restated stamps replay gives the oracle's map
    ref = rs.sweep_stamps_reference(sc)
    assert ((ref == 0) == (o.grid == -1)).all() and (((ref & 1) == 1) == (o.grid == 100)).all()
