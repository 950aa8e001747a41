"""The planner's kernels (csrc/plan.hip, territory.hip) on the built scenes of maze_scenes.py: corridors that take the
relaxation through many batches of rounds and back into tiles it has left, blocks that meet at a tile corner, runs that put
the walk's waypoint decision on the edges of its 64-cell chunks, snaps at the radius, clearance discs across tile borders.
test_maze_scenes_cpu.py establishes on the CPU what is taken for granted about the scenes here.  Every scene is painted with
update_rays and read back first; every value is compared with == against plan_rules.py, territory_rules.py and
assign_rules.py."""
import numpy as np
import pytest

import maze_scenes as S
import plan_rules as R
from conftest import load_pkg
from test_gpu_targets_by_path import check as check_by_path
from test_gpu_territories import check as check_territories, check_targets

pytestmark = pytest.mark.gpu
RES, OX, OY = 0.05, -5.0, -5.0                # the 200 geometry of the single scenes
PLAN_CASES = [(name, size) for name in ("serpentine", "spiral") for size in (200, 256, 68, 512)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def mapper(pkg, grid, rays, res=RES, ox=OX, oy=OY):
    """A mapper painted with the scene's rays that holds exactly the intended grid."""
    m = pkg.QuasarMapper(len(grid), res, ox, oy)
    S.paint(m, rays, res, ox, oy)
    got = m.grid_i8()
    assert got.shape == grid.shape and (got == grid).all(), np.argwhere(got != grid)[:8].tolist()
    return m


def xy(cell, res=RES, ox=OX, oy=OY):
    return S.centre(cell, res, ox, oy)


def same_plan(res, i, want):
    """Request i of a plan_paths(return_paths=True) result against plan_rules.plan's dict."""
    assert res["status"][i] == want["status"], (i, res["status"][i], want["status"])
    if want["status"] != R.OK:
        assert res["cost"][i] == R.INF and res["path_len"][i] == 0 and tuple(res["waypoint_cell"][i]) == (-1, -1), i
        assert len(res["paths"][i]) == 0 and np.isnan(res["waypoint"][i]).all(), i
        return
    assert res["cost"][i] == want["cost"] and res["path_len"][i] == len(want["path"]), (i, res["cost"][i], res["path_len"][i])
    got = [tuple(c) for c in res["paths"][i].tolist()]
    assert got == want["path"], (i, next(k for k, (a, b) in enumerate(zip(got, want["path"])) if a != b))
    assert tuple(res["waypoint_cell"][i]) == want["cell"], (i, tuple(res["waypoint_cell"][i]), want["cell"])
    assert tuple(res["waypoint"][i]) == want["xy"], i


def same_result(a, b):
    for k in ("status", "waypoint_cell", "waypoint", "cost", "path_len"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert len(a["paths"]) == len(b["paths"]) and all((p == q).all() and p.shape == q.shape for p, q in zip(a["paths"], b["paths"]))
    assert a["stats"] == b["stats"], (a["stats"], b["stats"])


# ---- 1. fields and paths with 32-bit keys ---------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=PLAN_CASES, ids=lambda p: f"{p[0]}-{p[1]}")
def case(request, pkg):
    c = S.plan_case(*request.param)
    c["name"] = request.param[0]
    c["t"] = R.traversable(c["grid"], 0)
    c["graph"] = R.move_graph(c["t"])
    c["m"] = mapper(pkg, c["grid"], c["rays"], c["res"], c["ox"], c["oy"])
    yield c
    c["m"].close()


def test_fields(case):
    m, path = case["m"], case["path"]
    assert (m.traversable(0).astype(bool) == case["t"]).all()
    for cell in (path[0], path[-1], path[len(path) // 2]):
        f = m.distance_field(xy(cell, case["res"], case["ox"], case["oy"]), clearance=0, snap_radius=0)
        want = R.field_scipy(case["t"], cell, case["graph"])
        assert f.shape == want.shape and f.dtype == want.dtype
        assert (f == want).all(), (cell, int((f != want).sum()), np.argwhere(f != want)[:8].tolist())


def test_paths_of_one_group(case):
    m, c = case["m"], case
    starts = [xy(s, c["res"], c["ox"], c["oy"]) for s, _ in c["requests"]]
    goals = [xy(g, c["res"], c["ox"], c["oy"]) for _, g in c["requests"]]
    want = [R.plan(c["t"], s, g, c["res"], c["ox"], c["oy"], snap_radius=0, lookahead=200, graph=c["graph"])
            for s, g in zip(starts, goals)]
    assert [w["status"] for w in want] == [R.OK] * 5 + [R.UNREACHABLE]
    crossings = max(S.crossings(w["path"]) for w in want[:5])
    assert crossings == S.crossings(want[0]["path"])              # the far end to the first cell is the longest
    first = None
    for _ in range(2):                # the second call must see nothing of the first call's lists, marks or counts
        res = m.plan_paths(starts, goals, clearance=0, snap_radius=0, lookahead=200, return_paths=True)
        for i in range(len(starts)):
            same_plan(res, i, want[i])
        st = res["stats"]
        assert st["groups"] == 1 and st["snapped"] == 0, st
        assert st["rounds"] >= crossings + 1, (st, crossings)
        assert st["tile_visits"] >= st["rounds"], st
        if first is None:
            first = res
        else:
            same_result(res, first)


def test_whole_corridor_with_the_longest_lookahead(case):
    """Every chunk of the corridor's whole path (9357 cells for the serpentine at 200): the waypoint is decided in the
    first, the cells of all the others are still written."""
    m, c = case["m"], case
    s, g = xy(c["path"][-1], c["res"], c["ox"], c["oy"]), xy(c["path"][0], c["res"], c["ox"], c["oy"])
    want = R.plan(c["t"], s, g, c["res"], c["ox"], c["oy"], snap_radius=0, lookahead=65536, graph=c["graph"])
    res = m.plan_paths([s], [g], clearance=0, snap_radius=0, lookahead=65536, return_paths=True)
    same_plan(res, 0, want)
    assert res["path_len"][0] == len(c["path"])


# ---- 2. tile corners ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True], ids=["diag", "anti"])
@pytest.mark.parametrize("corner", [64, 128])
@pytest.mark.parametrize("variant", S.PINCH_VARIANTS)
def test_pinch(pkg, variant, corner, anti):
    grid, rays = S.pinch(variant, corner, anti)
    cell = lambda x, y: S.pinch_cell((corner - 64 + x, corner - 64 + y), corner, anti)
    t = R.traversable(grid, 0)
    graph = R.move_graph(t)
    with mapper(pkg, grid, rays) as m:
        assert (m.traversable(0).astype(bool) == t).all()
        # a goal inside one block, then on each FREE cell that touches the corner: the seed's own tile, and the tiles
        # across x, across y and across the corner
        goals = [cell(66, 66)] + [g for g in (cell(63, 63), cell(64, 64), cell(64, 63), cell(63, 64)) if t[g[1], g[0]]]
        assert len(goals) == 3 + S.PINCH_VARIANTS.index(variant)
        for g in goals:
            f = m.distance_field(xy(g), clearance=0, snap_radius=0)
            want = R.field_scipy(t, g, graph)
            assert (f == want).all(), (g, np.argwhere(f != want)[:8].tolist(), f[f != want][:8].tolist())
            if g == cell(66, 66):
                far = f[corner - 4:corner, corner:corner + 4] if anti else f[corner - 4:corner, corner - 4:corner]
                assert (far == R.INF).all() if variant == "none" else (far != R.INF).all()
        starts = [cell(61, 61), cell(60, 63), cell(63, 63), cell(66, 66), cell(64, 64)]
        for g in goals:
            want = [R.plan(t, xy(s), xy(g), RES, OX, OY, snap_radius=0, graph=graph) for s in starts]
            res = m.plan_paths([xy(s) for s in starts], [xy(g)] * len(starts), clearance=0, snap_radius=0, return_paths=True)
            for i in range(len(starts)):
                same_plan(res, i, want[i])
            if g == cell(66, 66):
                assert res["status"][0] == (R.UNREACHABLE if variant == "none" else R.OK)
                assert variant == "none" or res["cost"][0] == {"one": 38, "both": 35}[variant]


@pytest.mark.parametrize("corner", [64, 128])
@pytest.mark.parametrize("flip_y", [False, True], ids=["", "flipy"])
@pytest.mark.parametrize("flip_x", [False, True], ids=["", "flipx"])
def test_late_corner(pkg, flip_x, flip_y, corner):
    """The cheapest route reaches the cell diagonally across the tile corner rounds after the two cells beside it have
    settled (maze_scenes.late_corner): the diagonal tile must be listed for that improvement alone."""
    (grid, rays), c = S.late_corner(flip_x, flip_y, corner)
    t = R.traversable(grid, 0)
    graph = R.move_graph(t)
    with mapper(pkg, grid, rays) as m:
        for _ in range(2):
            f = m.distance_field(xy(c["G"]), clearance=0, snap_radius=0)
            want = R.field_scipy(t, c["G"], graph)
            assert (f == want).all(), (np.argwhere(f != want)[:8].tolist(), f[f != want][:8].tolist(), want[f != want][:8].tolist())
            assert f[c["P"][1], c["P"][0]] == 192 and f[c["S"][1], c["S"][0]] == 185
        starts = [c["P"], c["Q"], c["R"], c["S"]]
        res = m.plan_paths([xy(s) for s in starts], [xy(c["G"])] * 4, clearance=0, snap_radius=0, return_paths=True)
        for i, s in enumerate(starts):
            same_plan(res, i, R.plan(t, xy(s), xy(c["G"]), RES, OX, OY, snap_radius=0, graph=graph))
        assert tuple(res["paths"][0][1]) == c["S"] and res["stats"]["rounds"] >= 7, res["stats"]


# ---- 3. the walk's chunks of 64 cells -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, top", [(L, 59) for L in S.L_RUNS] + [(L, S.LONG_TOP) for L in S.L_RUNS_LONG])
def test_l_run_waypoint_at_the_corner(pkg, L, top):
    """top = 59: the chunk after the corner is partial.  top = LONG_TOP: it is full and wholly invisible, so the first
    invisible cell is slot 0 (j == 0) while lane 63 already holds a cell of this chunk."""
    grid, rays = S.l_run(L, top)
    t = R.traversable(grid, 0)
    s, g = xy((10, 10)), xy((10 + L, top))
    with mapper(pkg, grid, rays) as m:
        res = m.plan_paths([s], [g], clearance=0, snap_radius=0, lookahead=200, return_paths=True)
        same_plan(res, 0, R.plan(t, s, g, RES, OX, OY, snap_radius=0, lookahead=200))
        assert res["path_len"][0] == L + top - 9
        assert tuple(res["waypoint_cell"][0]) == tuple(res["paths"][0][L]) == (10 + L, 10)
        if (L, top) == (64, 59):                  # path_cap on the path's last cell, one short of it and one past it
            n = L + 50
            for cap in (n - 1, n, n + 1):
                cut = m.plan_paths([s], [g], clearance=0, snap_radius=0, lookahead=200, return_paths=True, path_cap=cap)
                assert cut["path_len"][0] == n and len(cut["paths"][0]) == min(cap, n)
                assert (cut["paths"][0] == res["paths"][0][:cap]).all()
                for k in ("status", "waypoint_cell", "waypoint", "cost"):
                    assert cut[k].tobytes() == res[k].tobytes(), (cap, k)


def test_straight_waypoint_at_the_lookahead(pkg):
    grid, rays = S.straight()
    t = R.traversable(grid, 0)
    s, g = xy((10, 10)), xy((10 + S.STRAIGHT_N - 1, 10))
    with mapper(pkg, grid, rays) as m:
        for la in S.STRAIGHT_LOOKAHEADS:
            res = m.plan_paths([s], [g], clearance=0, snap_radius=0, lookahead=la, return_paths=True)
            same_plan(res, 0, R.plan(t, s, g, RES, OX, OY, snap_radius=0, lookahead=la))
            assert res["path_len"][0] == S.STRAIGHT_N
            assert tuple(res["waypoint_cell"][0]) == tuple(res["paths"][0][la]) == (10 + la, 10), la


# ---- 4. snap edges ----------------------------------------------------------------------------------------------------------------
def test_snap_edges(pkg):
    grid, rays = S.serpentine(*S.SNAP_SCENE)
    t = R.traversable(grid, 0)
    graph = R.move_graph(t)
    goal = xy((4, 4))
    expect = {"ten_cells": (100, 176), "eleven_cells": None, "between_rows": (100, 4), "clipped_window": (179, 176)}
    with mapper(pkg, grid, rays) as m:
        for name, (cell, radius) in S.SNAP_CASES.items():
            want = R.plan(t, xy(cell), goal, RES, OX, OY, snap_radius=radius, lookahead=200, graph=graph)
            res = m.plan_paths([xy(cell)], [goal], clearance=0, snap_radius=radius, lookahead=200, return_paths=True)
            same_plan(res, 0, want)
            if expect[name] is None:
                assert res["status"][0] == R.NO_START and res["stats"]["snapped"] == 0, name
            else:
                assert res["status"][0] == R.OK and tuple(res["paths"][0][0]) == expect[name], name
                assert res["stats"]["snapped"] == 1, (name, res["stats"])
            # the snapped cell as a goal: the field is seeded there
            f = m.distance_field(xy(cell), clearance=0, snap_radius=radius)
            if expect[name] is None:
                assert (f == R.INF).all(), name
            else:
                assert (f == R.field_scipy(t, expect[name], graph)).all(), name


# ---- 5. clearance across tile borders ---------------------------------------------------------------------------------------------
def test_clearance_across_tile_borders(pkg):
    grid, rays = S.room(200, 4, 196, S.CLEARANCE_OCCUPIED)
    with mapper(pkg, grid, rays) as m:
        for c in S.CLEARANCES:
            got, want = m.traversable(c).astype(bool), R.traversable(grid, c)
            assert (got == want).all(), (c, int((got != want).sum()), np.argwhere(got != want)[:8].tolist())


# ---- 6. 64-bit keys ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, size", [("serpentine", 200), ("serpentine", 512), ("spiral", 200)])
def test_territories_along_a_corridor(pkg, name, size):
    c = S.plan_case(name, size)
    path = c["path"]
    bots = S.territory_bots(path, c["res"], c["ox"], c["oy"])
    k = (len(path) // 2) & ~1         # the mid bot's path index (maze_scenes.territory_bots)
    if name == "spiral":
        bots, k = bots[:2], len(path) - 1                         # the outer end and the centre
    assert k % 2 == 0
    with mapper(pkg, c["grid"], c["rays"], c["res"], c["ox"], c["oy"]) as m:
        got, want = check_territories(m, bots, clearance=0, snap_radius=0)
        assert want["ties"] > 0 and got["stats"]["rounds"] > 16, (want["ties"], got["stats"])
        assert got["stats"]["tile_visits"] >= got["stats"]["rounds"]
        # the cell halfway between bot 0 and the other bot on the corridor costs both the same: the lower bot owns it
        tx, ty = path[k // 2]
        assert got["cost"][ty, tx] == R.ORTHO * (k // 2) and got["owner"][ty, tx] == 0
        nx, ny = path[k // 2 + 1]
        assert got["owner"][ny, nx] == (1 if name == "spiral" else 2)
        assert got["status"].tolist() == ([R.OK] * 2 if name == "spiral" else [R.OK] * 4 + [R.NO_START])
        assert got["area"].sum() == len(path)                     # nobody reaches the spare corridor


# ---- 7. the target calls over the shared host path ----------------------------------------------------------------------------------
def test_target_calls_on_the_spiral(pkg):
    c = S.plan_case("spiral", 200)
    bots = [xy(c["path"][0]), xy(c["path"][-1])]
    with mapper(pkg, c["grid"], c["rays"]) as m:
        for sep in (0.0, 1.0):
            res, want = check_by_path(m, bots, sep=sep, min_cluster=1, clearance=0)
            assert res["stats"]["n_centroids"] == 2 and res["status"][0] == R.OK      # the spiral and the spare corridor
        out, want = check_targets(m, bots, min_cluster=1, clearance=0)
        assert (out["idx"] >= 0).sum() == 1 and sorted(out["status"].tolist()) == [R.OK, R.UNREACHABLE]
        assert out["area"].sum() == len(c["path"])
