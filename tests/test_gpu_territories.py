"""Territories on the device (qs_territories, qs_frontier_targets_by_territory) against the CPU restatement of
include/quasar_slam.h's rules T1-T5 in territory_rules.py, which is fed the device's own grid_i8() and the same bots.
Maps are painted with update_rays.  Every value is compared with ==."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import plan_rules as R
import territory_rules as T
from conftest import GOLDEN, load_pkg
from test_gpu_plan_rounds import room

pytestmark = pytest.mark.gpu
PART = ("owner", "cost", "status", "area", "box")


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def centres(m, cells):
    return [(m.ox + (gx + 0.5) * m.res, m.oy + (gy + 0.5) * m.res) for gx, gy in cells]


def check(m, bots, clearance=2, snap_radius=10):
    """qs_territories against the restatement: owner, cost, status, area, box and the counts in stats."""
    bots = np.asarray(bots, dtype=np.float64).reshape(-1, 2)
    got = m.territories(bots, clearance=clearance, snap_radius=snap_radius, return_owner=True, return_cost=True)
    want = T.partition(m.grid_i8(), bots, m.res, m.ox, m.oy, clearance, snap_radius)
    T.same(got, want, PART)
    st = got["stats"]
    assert st["bot_cells"] == sum(c is not None for c in want["bot_cells"])
    assert st["owned_cells"] == got["area"].sum() == (got["owner"] >= 0).sum()
    assert st["n_centroids"] == st["centroid_cells"] == st["centroids_owned"] == st["reserved"] == 0
    lean = m.territories(bots, clearance=clearance, snap_radius=snap_radius)      # without the two arrays: the same rest
    assert sorted(lean) == ["area", "box", "stats", "status"] and lean["stats"] == st
    T.same(lean, got, ("status", "area", "box"))
    return got, want


# ---- 1. one tile, symmetric ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size, origin", [(64, -1.6), (200, -5.0)])
def test_one_tile_symmetric(pkg, size, origin):
    with pkg.QuasarMapper(size, 0.05, origin, origin) as m:
        lo, hi = origin + 4 * 0.05, origin + 59 * 0.05
        room(m, lo, hi, lo, hi)
        t = m.traversable(2).astype(bool)
        yy, xx = np.nonzero(t)
        assert len(yy) and xx.max() < 64 and yy.max() < 64
        mx, my = int(xx.min() + xx.max()) // 2, int(yy.min() + yy.max()) // 2
        cells = [(mx - 10, my - 10), (mx + 10, my - 10), (mx - 10, my + 10), (mx + 10, my + 10)]      # column mx, row my: ties
        assert all(t[y, x] for x, y in cells)
        for order in ([0, 1, 2, 3], [3, 1, 0, 2]):
            bots = centres(m, [cells[i] for i in order])
            for _ in range(2):            # a second call must not see anything of the first call's lists
                got, want = check(m, bots)
                assert want["ties"] > 0
                assert got["stats"]["rounds"] == 1 and got["stats"]["tile_visits"] == 1, got["stats"]
                assert got["owner"][my, mx] == 0 and got["area"].sum() == t.sum()


# ---- 2. tile borders ---------------------------------------------------------------------------------------------------------
def cx(g):
    """World coordinate of the centre of cell g of the 200 x 200 scenes (both axes: origin -5, 0.05 m per cell)."""
    return -5.0 + (g + 0.5) * 0.05


def free_rows(m, rows, a, b):
    """FREE cells [a, b) of every row in rows (a ray frees all its cells but the last)."""
    ry = np.array([cx(gy) for gy in rows])
    m.update_rays(np.full(len(ry), cx(a)), ry, np.full(len(ry), cx(b)), ry, np.zeros(len(ry), dtype=np.uint8))


def occupy(m, cells):
    x, y = np.array([cx(gx) for gx, _ in cells]), np.array([cx(gy) for _, gy in cells])
    m.update_rays(x, y, x, y, np.ones(len(x), dtype=np.uint8))


BORDER_CELLS = [(63, 63), (64, 20), (127, 64), (128, 128), (191, 30), (192, 192), (30, 127), (20, 191), (150, 63), (63, 150),
                (60, 180), (68, 180), (100, 170), (99, 30)]      # the last two: in the gap, and beside the wall


HOLE_ROWS, HOLE_COLS = (40, 90, 140, 185), (30, 80, 120, 170)


def border_scene(pkg):
    """One room over FREE cells [4, 196)^2, all four tiles across and down, and a wall at column 100 from the bottom up to
    row 150 (a gap above it): detours.  (60, 180) and (68, 180) are equidistant from the cells of column 64, the first
    column of the next tile.  Sixteen single UNKNOWN cells inside the room give it frontiers besides its rim."""
    m = pkg.QuasarMapper(200, 0.05, -5.0, -5.0)
    free_rows(m, [gy for gy in range(4, 196) if gy not in HOLE_ROWS], 4, 196)
    for a, b in zip((4,) + tuple(h + 1 for h in HOLE_COLS), HOLE_COLS + (196,)):
        free_rows(m, HOLE_ROWS, a, b)
    occupy(m, [(100, gy) for gy in range(2, 150)])
    return m


def test_tile_borders(pkg):
    with border_scene(pkg) as m:
        got, want = check(m, centres(m, BORDER_CELLS))
        assert want["ties"] > 0 and got["stats"]["rounds"] > 1
        assert got["status"].tolist() == [R.OK] * len(BORDER_CELLS) and (got["area"] > 0).all()
        assert got["owner"][63, 63] == 0 and got["owner"][180, 64] == 10 and got["cost"][180, 64] == 20
        assert got["owner"][30, 97] == 13 and got["owner"][30, 101] == -1               # snapped off the wall's clearance band


# ---- 3. degenerate bots ------------------------------------------------------------------------------------------------------
def test_degenerate_bots(pkg):
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        free_rows(m, range(10, 120), 10, 120)                 # the main room
        free_rows(m, range(150, 180), 20, 50)                 # a room of its own, walled all round
        occupy(m, [(gx, gy) for gx in range(19, 51) for gy in (149, 180)] + [(gx, gy) for gy in range(149, 181) for gx in (19, 50)])
        t2 = R.traversable(m.grid_i8(), 2)
        sealed = int(t2[140:190, 10:60].sum())
        assert sealed == 26 * 26
        bots = centres(m, [(30, 30), (100, 100), (100, 100), (35, 165), (160, 60)]) + [(math.nan, 0.0), (0.0, math.inf)]
        got, _ = check(m, bots)
        assert got["status"].tolist() == [R.OK] * 4 + [R.NO_START] * 3
        assert got["area"][2] == 0 and got["box"][2].tolist() == [-1] * 4 and got["area"][1] > 0     # the shared cell
        assert got["area"][3] == sealed and got["box"][3].tolist() == [22, 152, 47, 177]
        assert (got["area"][4:] == 0).all() and (got["box"][4:] == -1).all()
        none, _ = check(m, np.zeros((0, 2)))
        assert none["area"].shape == (0,) and none["box"].shape == (0, 4) and (none["owner"] == -1).all()
        assert (none["cost"] == R.INF).all() and none["stats"]["rounds"] == 0
        one, _ = check(m, bots[:1])
        assert one["area"][0] == t2[:130, :130].sum()
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:        # no FREE cell
        got, _ = check(m, [(0.0, 0.0), (1.0, 1.0)])
        assert got["status"].tolist() == [R.NO_START] * 2 and (got["owner"] == -1).all() and got["stats"]["rounds"] == 0
        res = m.frontier_targets_by_territory([(0.0, 0.0)], return_centroids=True)
        assert res["status"].tolist() == [R.NO_START] and res["idx"].tolist() == [-1] and len(res["centroids"]) == 0


# ---- 4. index width ----------------------------------------------------------------------------------------------------------
def test_index_width(pkg):
    """Owners that need more than a byte, and the largest index."""
    with pkg.QuasarMapper(256, 0.05, -6.4, -6.4) as m:
        c = lambda g: -6.4 + (g + 0.5) * 0.05
        ry = np.array([c(gy) for gy in range(40, 136)])
        m.update_rays(np.full(len(ry), c(40)), ry, np.full(len(ry), c(136)), ry, np.zeros(len(ry), dtype=np.uint8))
        assert m.traversable(0).sum() == 96 * 96              # over the tile borders at 64 and 128, both ways
        rng = np.random.default_rng(1024)
        pick = rng.choice(96 * 96, 1024, replace=False)
        cells = [(40 + int(i) % 96, 40 + int(i) // 96) for i in pick]
        for n in (300, 1024):
            got, _ = check(m, centres(m, cells[:n]), clearance=0, snap_radius=0)
            owners = np.unique(got["owner"][got["owner"] >= 0])
            assert (owners > 255).any() and n - 1 in owners and (got["area"] > 0).all()
        with pytest.raises(ValueError):
            m.territories(np.zeros((1025, 2)))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pos, stat, area, box = np.zeros((1025, 2)), np.zeros(1025, dtype=np.int32), np.zeros(1025, dtype=np.int64), \
            np.zeros((1025, 4), dtype=np.int32)
        assert m._L.qs_territories(m._h, None, p(pos), 1025, None, None, p(stat), p(area), p(box), None) == -1
        assert b"QS_FT_MAX_BOTS" in m._L.qs_last_error(m._h)
        assert m._L.qs_territories(m._h, None, p(pos), 1024, None, None, p(stat), p(area), p(box), None) == 0
        lib = importlib.import_module(pkg.__name__ + "._lib")
        for bad in ((17, 10, 200), (2, 65, 200), (-1, 10, 200)):
            prm = lib.QsPlanParams(*bad, 0)
            assert m._L.qs_territories(m._h, C.byref(prm), p(pos), 4, None, None, p(stat), p(area), p(box), None) == -1, bad


# ---- 5. clearance and snap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clearance", [0, 2, 16])
def test_clearance_and_snap(pkg, clearance):
    with border_scene(pkg) as m:
        for snap in (0, 10):
            got, _ = check(m, centres(m, BORDER_CELLS), clearance=clearance, snap_radius=snap)
            beside = got["status"][13]                        # one cell from the wall: blocked by any clearance, snapped or not
            assert beside == (R.OK if clearance == 0 or (snap and clearance <= 10) else R.NO_START)


# ---- 6. targets ----------------------------------------------------------------------------------------------------------------
def last_poses(m, stream):
    """The pose of each bot's last accepted packet, ascending id."""
    acc, pose = m.last_batch()
    last = {}
    for i in np.nonzero(acc)[0]:
        last[int(stream[i, 4])] = (float(pose[i, 0]), float(pose[i, 1]))
    return [last[b] for b in sorted(last)]


def check_targets(m, bots, min_cluster=3, **params):
    bots = np.asarray(bots, dtype=np.float64).reshape(-1, 2)
    res = m.frontier_targets_by_territory(bots, min_cluster=min_cluster, return_centroids=True, **params)
    ref_c = np.array(m.frontier_centroids(min_cluster), dtype=np.float64).reshape(-1, 2)
    assert res["centroids"].shape == ref_c.shape and (res["centroids"] == ref_c).all()
    want = T.targets(m.grid_i8(), ref_c, bots, m.res, m.ox, m.oy, **params)
    T.same(res, want, ("idx", "xy", ("cost", "cost_b"), "status", "waypoint_cell", "waypoint", "area", "box", "centroid_owner"))
    st = res["stats"]
    assert st["n_centroids"] == len(ref_c) and st["reserved"] == 0
    assert st["centroid_cells"] == sum(c is not None for c in want["centroid_cells"])
    assert st["centroids_owned"] == (want["centroid_owner"] >= 0).sum()
    assert st["bot_cells"] == sum(c is not None for c in want["bot_cells"]) and st["owned_cells"] == res["area"].sum()
    ok = res["idx"] >= 0
    assert (res["status"][ok] == R.OK).all() and (res["centroid_owner"][res["idx"][ok]] == np.nonzero(ok)[0]).all()
    if ok.any():                                              # a separate plan_paths(bot, target) call
        again = m.plan_paths(bots[ok], res["xy"][ok], **params)
        assert (again["status"] == R.OK).all()
        for k in ("cost", "waypoint_cell", "waypoint"):
            assert (again[k] == res[k][ok]).all(), k
    lean = m.frontier_targets_by_territory(bots, min_cluster=min_cluster, waypoints=False, **params)
    T.same(lean, res, ("idx", "xy", "cost", "status", "area", "box"))
    assert (lean["waypoint_cell"] == -1).all() and np.isnan(lean["waypoint"]).all()
    # the partition the targets come from is qs_territories' on the same map
    part = {k: v for k, v in params.items() if k != "lookahead"}
    terr = m.territories(bots, return_owner=True, return_cost=True, **part)
    T.same(terr, res, ("area", "box"))
    for k, cell in enumerate(want["centroid_cells"]):
        assert res["centroid_owner"][k] == (-1 if cell is None else terr["owner"][cell[1], cell[0]]), k
    for b in np.nonzero(ok)[0]:
        cell = want["centroid_cells"][res["idx"][b]]
        assert terr["cost"][cell[1], cell[0]] == res["cost"][b] == want["centroid_cost"][res["idx"][b]]
    return res, want


@pytest.mark.parametrize("name", ["session_512", "laps5_512", "mixed_200"])
def test_targets_on_golden_sessions(pkg, name):
    g = np.load(f"{GOLDEN}/{name}.npz", allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        bots = last_poses(m, g["datagrams"])
        assert len(bots) == 2
        out, _ = check_targets(m, bots)
        assert (out["idx"] >= 0).all() and out["idx"][0] != out["idx"][1]
        check_targets(m, bots[::-1], min_cluster=1, clearance=1, snap_radius=4, lookahead=7)


def test_targets_on_the_border_scene(pkg):
    with border_scene(pkg) as m:
        out, want = check_targets(m, centres(m, BORDER_CELLS), min_cluster=1)
        assert (out["idx"] >= 0).sum() >= 4 and (out["status"] == R.UNREACHABLE).any()
        states = {b + 1: xy for b, xy in enumerate(centres(m, BORDER_CELLS))}
        targets, wps, terr = m.assign_frontier_targets(states, min_cluster=1, by_territory=True, return_waypoints=True,
                                                       return_territory=True)
        assert targets == {b + 1: tuple(out["xy"][b].tolist()) for b in range(len(states)) if out["idx"][b] >= 0}
        assert wps == {b + 1: tuple(out["waypoint"][b].tolist()) for b in range(len(states)) if out["idx"][b] >= 0}
        assert terr == {b + 1: (int(out["area"][b]), tuple(out["box"][b].tolist())) for b in range(len(states))}
        assert m.assign_frontier_targets(states, min_cluster=1, by_territory=True) == targets
        with pytest.raises(ValueError):
            m.assign_frontier_targets(states, by_path=True, by_territory=True)


# ---- 7. no session state -----------------------------------------------------------------------------------------------------
def test_no_session_state(pkg, tmp_path):
    g = np.load(f"{GOLDEN}/session_512.npz", allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        bots = last_poses(m, g["datagrams"]) + [(0.0, 0.0), (math.nan, 1.0)]
        grid = m.grid_i8().tobytes()
        m.save(tmp_path / "before.qs")
        a = m.territories(bots, return_owner=True, return_cost=True)
        b = m.frontier_targets_by_territory(bots, return_centroids=True)
        m.save(tmp_path / "after.qs")
        assert (tmp_path / "before.qs").read_bytes() == (tmp_path / "after.qs").read_bytes()
        assert m.grid_i8().tobytes() == grid
        a2 = m.territories(bots, return_owner=True, return_cost=True)
        b2 = m.frontier_targets_by_territory(bots, return_centroids=True)
        for k in PART:
            assert a[k].tobytes() == a2[k].tobytes(), k
        for k in ("idx", "xy", "cost", "status", "waypoint_cell", "waypoint", "area", "box", "centroids", "centroid_owner"):
            assert b[k].tobytes() == b2[k].tobytes(), k
        assert a["stats"] == a2["stats"] and b["stats"] == b2["stats"]


# ---- 8. 64 bots at 4096^2 ------------------------------------------------------------------------------------------------------
def test_64_bots_4096(pkg):
    """The shape the feature is for, and the only one here with many seeds and many list entries per round.  The whole grid
    is too slow to restate: three bots' connected regions are restated through windows (the tile-aligned bounding box of
    the region and one tile more all round, so that nothing outside the window is within `clearance` of the region)."""
    from scipy import ndimage
    replay = importlib.import_module(pkg.__name__ + ".replay")
    session, _ = replay.telemetry_csv_to_packets()
    stream = replay.multi_bot_stream(session, 64, 64 * 400)
    with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2) as m:
        m.ingest_array(stream)
        bots = np.array(last_poses(m, stream))
        assert len(bots) == 64
        got = m.territories(bots, return_owner=True, return_cost=True)
        assert got["area"].sum() == got["stats"]["owned_cells"] == (got["owner"] >= 0).sum()
        assert got["stats"]["bot_cells"] == (got["status"] == R.OK).sum() > 16
        owners = np.nonzero(got["area"] > 0)[0]
        grid = m.grid_i8()
        trav = m.traversable(2).astype(bool)
        label, _ = ndimage.label(trav, structure=np.ones((3, 3)))      # 8-connected: no smaller than a region of rule 3's moves
        for b in (owners[0], owners[len(owners) // 2], owners[-1]):
            ys, xs = np.nonzero(got["owner"] == b)
            region = label == label[ys[0], xs[0]]
            ry, rx = np.nonzero(region)
            win = (max(rx.min() // 64 * 64 - 64, 0), max(ry.min() // 64 * 64 - 64, 0),
                   min(rx.max() // 64 * 64 + 128, 4096), min(ry.max() // 64 * 64 + 128, 4096))
            sp = T.Window(grid, 2, win)
            assert (sp.t[region] == trav[region]).all()
            want = T.partition(grid, bots, m.res, m.ox, m.oy, space=sp)
            inside = [i for i, c in enumerate(want["bot_cells"]) if c is not None and region[c[1], c[0]]]
            assert b in inside
            assert (got["owner"][region] == want["owner"][region]).all() and (got["cost"][region] == want["cost"][region]).all()
            for k in ("status", "area", "box"):
                assert (got[k][inside] == want[k][inside]).all(), (b, k)
