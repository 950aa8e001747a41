"""The scenes of maze_scenes.py, checked on the CPU: what test_gpu_plan_mazes.py and test_gpu_frontier_mazes.py take for
granted about them is established here by the references alone (the oracle's mapper and frontier code, plan_rules.py,
territory_rules.py), before any device sees them."""
import numpy as np
import pytest

import maze_scenes as S
import plan_rules as R
import territory_rules as T
from oracle import oracle as orc

SIZES = (200, 256, 68)
PLAN_CASES = [(name, size) for name in ("serpentine", "spiral") for size in (200, 256, 68, 512)]


def painted(grid, rays, res, ox, oy):
    o = orc.OracleMapper(len(grid), res, ox, oy)
    S.paint(o, rays, res, ox, oy)
    return o.grid


def assert_paints(grid, rays, res, ox, oy):
    got = painted(grid, rays, res, ox, oy)
    assert got.shape == grid.shape and (got == grid).all(), np.argwhere(got != grid)[:8].tolist()


def one_wide_interior_component(grid):
    """One 4-connected component of FREE cells, no 2 x 2 FREE block, nothing on the grid's rim."""
    size = len(grid)
    free = grid == 0
    ys, xs = np.nonzero(free)
    assert len(ys) and xs.min() >= 1 and ys.min() >= 1 and xs.max() <= size - 2 and ys.max() <= size - 2
    assert not (free[:-1, :-1] & free[1:, :-1] & free[:-1, 1:] & free[1:, 1:]).any()
    _, root = S.components(np.stack([xs, ys], axis=1), size)
    assert len(set(root.values())) == 1


# ---- 1. painting --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(S.FRONTIER_SCENES))
def test_frontier_scene_paints_and_clusters(name, size):
    grid, rays, res, ox, oy = S.build(name, size)
    assert_paints(grid, rays, res, ox, oy)
    assert (R.traversable(grid, 0) == (grid == 0)).all()
    ys, xs = np.nonzero(grid == 0)
    free = np.stack([xs, ys], axis=1).astype(np.int32)           # row-major, as get_frontiers walks
    cells = orc.frontier_cells(grid)
    assert cells.shape == free.shape and (cells == free).all()  # every FREE cell is a frontier cell
    all1 = orc.frontier_clusters(cells, size, 1)
    _, lo, hi, pitch, _, _ = S.GEOMETRY[size][2:]
    if name in S.CORRIDORS:
        one_wide_interior_component(grid)
        assert len(all1) == 1 and all1[0, 0] == len(cells) >= 100
        if name == "comb":
            assert all1[0, 1:3].tolist() == [lo, lo]
        assert (orc.frontier_clusters(cells, size, 3) == all1).all()
    elif name == "lattice":
        assert len(all1) == len(cells) >= 400 and (all1[:, 0] == 1).all() and (all1[:, 1:3] == cells).all()
        assert len(orc.frontier_clusters(cells, size, 3)) == 0
    else:
        assert len(cells) % 4 == 0 and len(all1) == len(cells) // 4 >= 30 and (all1[:, 0] == 4).all()
        assert (orc.frontier_clusters(cells, size, 3) == all1).all()
    # the members' roots by flood fill are the clusters' first cells
    lin, root = S.components(cells, size)
    assert sorted(set(root.values())) == (all1[:, 2] * size + all1[:, 1]).tolist()


# ---- 2. the planner's corridors -------------------------------------------------------------------------------------------
# spiral at 68: only its outermost turn (column 66, row 66) lies beyond the tile border at 64, so its path crosses 4 borders
# however it is walked; every other case crosses more than two batches of 8 rounds' worth
MIN_CROSSINGS = {("spiral", 68): 4}


@pytest.fixture(scope="module", params=PLAN_CASES, ids=lambda p: f"{p[0]}-{p[1]}")
def case(request):
    c = S.plan_case(*request.param)
    c["name"] = request.param[0]
    c["t"] = R.traversable(c["grid"], 0)
    c["graph"] = R.move_graph(c["t"])
    return c


def test_plan_case_paints(case):
    assert_paints(case["grid"], case["rays"], case["res"], case["ox"], case["oy"])
    assert (case["t"] == (case["grid"] == 0)).all()
    plain = case["grid"].copy()
    x0, y0, x1, y1 = S.SPARE[case["name"], case["size"]]
    plain[y0:max(y1, y0 + 1), x0:max(x1, x0 + 1)] = -1
    one_wide_interior_component(plain)
    assert len(case["path"]) == (plain == 0).sum()               # a simple path through every corridor cell
    ys, xs = np.nonzero(case["grid"] == 0)
    assert xs.min() >= 1 and ys.min() >= 1 and max(xs.max(), ys.max()) <= case["size"] - 2


def test_plan_case_path_and_crossings(case):
    t, path = case["t"], case["path"]
    f = R.field_scipy(t, path[0], case["graph"])
    walked = R.walk(t, f, path[-1], path[0])
    assert walked == path[::-1]
    assert int(f[path[-1][1], path[-1][0]]) == R.ORTHO * (len(path) - 1)
    n = S.crossings(walked)
    assert n >= MIN_CROSSINGS.get((case["name"], case["size"]), 17), n
    if case["size"] == 200:
        assert (len(path), n) == {"serpentine": (9357, 147), "spiral": (9313, 130)}[case["name"]]
    if case["size"] == 512:
        assert min(x for x, _ in path) // 64 == 2 and min(y for _, y in path) // 64 == 1


def test_plan_case_requests(case):
    """The statuses of the six requests: all OK but the goal in the spare corridor."""
    t, c = case["t"], case
    want = [R.plan(t, S.centre(s, c["res"], c["ox"], c["oy"]), S.centre(g, c["res"], c["ox"], c["oy"]), c["res"], c["ox"],
                   c["oy"], snap_radius=0, graph=c["graph"]) for s, g in c["requests"]]
    assert [w["status"] for w in want] == [R.OK] * 5 + [R.UNREACHABLE]
    assert want[4]["cost"] == 0 and want[4]["path"] == [c["requests"][4][0]]
    assert want[0]["path"] == c["path"][::-1] and want[1]["path"] == c["path"]


@pytest.mark.parametrize("name, size", [("serpentine", 200), ("serpentine", 512), ("spiral", 200)])
def test_territory_bots_tie(name, size):
    c = S.plan_case(name, size)
    bots = S.territory_bots(c["path"], c["res"], c["ox"], c["oy"])
    if name == "spiral":
        bots = [bots[0], bots[1]]                                # the outer end and the centre
    want = T.partition(c["grid"], bots, c["res"], c["ox"], c["oy"], clearance=0, snap_radius=0)
    assert want["ties"] > 0
    assert want["status"].tolist() == ([R.OK] * 4 + [R.NO_START] if name == "serpentine" else [R.OK] * 2)
    assert (want["area"][:2] > 0).all() and want["area"].sum() == len(c["path"])
    if name == "serpentine":
        assert want["area"][2] > 0 and want["area"][3] == 0      # the duplicate owns nothing


# ---- 3. tile corners ------------------------------------------------------------------------------------------------------
PINCH_COST = {"none": (R.INF, R.INF), "one": (24, 38), "both": (21, 35)}


@pytest.mark.parametrize("anti", [False, True], ids=["diag", "anti"])
@pytest.mark.parametrize("corner", [64, 128])
@pytest.mark.parametrize("variant", S.PINCH_VARIANTS)
def test_pinch(variant, corner, anti):
    grid, rays = S.pinch(variant, corner, anti)
    assert_paints(grid, rays, 0.05, -5.0, -5.0)
    assert (grid == 0).sum() == 32 + S.PINCH_VARIANTS.index(variant)
    t = R.traversable(grid, 0)
    assert (t == (grid == 0)).all()
    cell = lambda x, y: S.pinch_cell((corner - 64 + x, corner - 64 + y), corner, anti)
    f = R.field_scipy(t, cell(66, 66))
    at = lambda x, y: int(f[cell(x, y)[1], cell(x, y)[0]])
    assert (at(63, 63), at(61, 61)) == PINCH_COST[variant]
    assert at(64, 64) == 2 * R.DIAG
    far = np.zeros_like(t)
    lo_block = (slice(corner - 4, corner), slice(corner, corner + 4) if anti else slice(corner - 4, corner))
    far[lo_block] = True
    assert ((f[far] == R.INF).all() and t[far].all()) if variant == "none" else (f[far] != R.INF).all()
    want = R.plan(t, S.centre(cell(61, 61), 0.05, -5.0, -5.0), S.centre(cell(66, 66), 0.05, -5.0, -5.0), 0.05, -5.0, -5.0,
                  snap_radius=0)
    assert want["status"] == (R.UNREACHABLE if variant == "none" else R.OK)
    if variant == "both":                                        # the path takes the diagonal across the tile corner
        k = want["path"].index(cell(63, 63))
        assert want["path"][k + 1] == cell(64, 64)


@pytest.mark.parametrize("corner", [64, 128])
@pytest.mark.parametrize("flip_y", [False, True], ids=["", "flipy"])
@pytest.mark.parametrize("flip_x", [False, True], ids=["", "flipx"])
def test_late_corner(flip_x, flip_y, corner):
    (grid, rays), c = S.late_corner(flip_x, flip_y, corner)
    assert_paints(grid, rays, 0.05, -5.0, -5.0)
    t = R.traversable(grid, 0)
    assert (t == (grid == 0)).all()
    f = R.field_scipy(t, c["G"])
    assert {k: int(f[y, x]) for k, (x, y) in c.items()} == dict(G=0, P=192, Q=190, R=190, S=185)
    tile = lambda cell: (cell[0] // 64, cell[1] // 64)
    assert len({tile(c[k]) for k in "PQRS"}) == 4 and tile(c["G"]) == tile(c["Q"])
    assert abs(tile(c["P"])[0] - tile(c["S"])[0]) == abs(tile(c["P"])[1] - tile(c["S"])[1]) == 1
    want = R.plan(t, S.centre(c["P"], 0.05, -5.0, -5.0), S.centre(c["G"], 0.05, -5.0, -5.0), 0.05, -5.0, -5.0, snap_radius=0)
    assert want["status"] == R.OK and want["cost"] == 192 and want["path"][1] == c["S"] and len(want["path"]) == 39
    # without the diagonal across the corner P would cost 195: Q and R do not improve when S does
    for k in "QR":
        assert int(f[c[k][1], c[k][0]]) == int(f[c["S"][1], c["S"][0]]) + R.ORTHO


# ---- 4. walk chunks -------------------------------------------------------------------------------------------------------
L_RUN_CASES = [(L, 59) for L in S.L_RUNS] + [(L, S.LONG_TOP) for L in S.L_RUNS_LONG]


@pytest.mark.parametrize("L, top", L_RUN_CASES)
def test_l_run(L, top):
    grid, rays = S.l_run(L, top)
    assert_paints(grid, rays, 0.05, -5.0, -5.0)
    one_wide_interior_component(grid)
    t = R.traversable(grid, 0)
    start, goal = (10, 10), (10 + L, top)
    path = R.walk(t, R.field_scipy(t, goal), start, goal)
    assert len(path) == L + top - 9 and path == S.corridor_order(grid, start)
    assert R.waypoint(t, path, 200) == path[L] == (10 + L, 10)
    if top == S.LONG_TOP:             # the 64 path cells after the corner exist, lie within the lookahead and are all invisible
        assert L % 64 == 0 and L + 64 <= min(200, len(path) - 1)
        assert not any(all(t[y, x] for x, y in R.bresenham(10, 10, *cell)) for cell in path[L + 1:L + 65])


def test_straight():
    grid, rays = S.straight()
    assert_paints(grid, rays, 0.05, -5.0, -5.0)
    one_wide_interior_component(grid)
    t = R.traversable(grid, 0)
    start, goal = (10, 10), (10 + S.STRAIGHT_N - 1, 10)
    path = R.walk(t, R.field_scipy(t, goal), start, goal)
    assert len(path) == S.STRAIGHT_N
    for la in S.STRAIGHT_LOOKAHEADS:
        assert R.waypoint(t, path, la) == path[la]


# ---- 5. snap and clearance --------------------------------------------------------------------------------------------------
def test_snap_cases():
    grid, rays = S.serpentine(*S.SNAP_SCENE)
    assert_paints(grid, rays, 0.05, -5.0, -5.0)
    one_wide_interior_component(grid)
    t = R.traversable(grid, 0)
    snaps = {k: R.snap(t, S.centre(cell, 0.05, -5.0, -5.0), 0.05, -5.0, -5.0, r) for k, (cell, r) in S.SNAP_CASES.items()}
    assert snaps == {"ten_cells": (100, 176), "eleven_cells": None, "between_rows": (100, 4), "clipped_window": (179, 176)}
    for k, (cell, r) in S.SNAP_CASES.items():
        assert not t[cell[1], cell[0]]
        near = [(x - cell[0]) ** 2 + (y - cell[1]) ** 2 for y, x in np.argwhere(t)]
        assert min(near) == {"ten_cells": 100, "eleven_cells": 121, "between_rows": 4, "clipped_window": 845}[k]
    assert sum(d == 4 for d in [(x - 100) ** 2 + (y - 6) ** 2 for y, x in np.argwhere(t)]) == 2
    goal = S.centre((4, 4), 0.05, -5.0, -5.0)
    status = {k: R.plan(t, S.centre(cell, 0.05, -5.0, -5.0), goal, 0.05, -5.0, -5.0, snap_radius=r)["status"]
              for k, (cell, r) in S.SNAP_CASES.items()}
    assert status == {"ten_cells": R.OK, "eleven_cells": R.NO_START, "between_rows": R.OK, "clipped_window": R.OK}


def test_clearance_room():
    grid, rays = S.room(200, 4, 196, S.CLEARANCE_OCCUPIED)
    assert_paints(grid, rays, 0.05, -5.0, -5.0)
    assert (grid == 100).sum() == len(S.CLEARANCE_OCCUPIED) and (grid == 0).sum() == 192 * 192 - len(S.CLEARANCE_OCCUPIED)
    sums = [int(R.traversable(grid, c).sum()) for c in S.CLEARANCES]
    assert sums[0] == (grid == 0).sum() and sums == sorted(sums, reverse=True) and len(set(sums)) == len(sums)
    small = grid[:40, :40]                                       # rule 1 word for word round (5, 5), the disc cut by the room's rim
    for c in (1, 15, 16):
        assert (R.traversable(small, c) == R.traversable_brute(small, c)).all()
