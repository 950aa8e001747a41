"""Territories without a GPU: the C ABI declaration, and the CPU restatement (territory_rules.py: one field per bot, folded)
against a second one written differently (ONE heapq Dijkstra over (cost, bot) tuples from all seeds) on grids painted
directly and on the oracle's 200 x 200 golden grids."""
import heapq
import importlib
import math
import os
import re

import numpy as np
import pytest

import plan_rules as R
import territory_rules as T
from conftest import PKG_NAME, ROOT
from test_targets_by_path_cpu import oracle_case


def test_symbols_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    assert re.search(r"int qs_territories\(", txt) and re.search(r"int qs_frontier_targets_by_territory\(", txt)
    block = txt[txt.index("---- territories"):txt.index("---- map view")]
    assert "NO separation rule" in block and all(f" T{i} " in block for i in range(1, 7))
    lib = importlib.import_module(PKG_NAME + "._lib")
    assert len(lib.SIGNATURES["qs_territories"][1]) == 10
    assert len(lib.SIGNATURES["qs_frontier_targets_by_territory"][1]) == 18
    pkg = importlib.import_module(PKG_NAME)
    pkg.build()
    assert hasattr(pkg.load(), "qs_territories") and hasattr(pkg.load(), "qs_frontier_targets_by_territory")


# ---- the second restatement ------------------------------------------------------------------------------------------------
def multi_source(grid, bots, res, ox, oy, clearance, snap_radius):
    """T1-T4 by one Dijkstra whose heap holds (cost, bot, gx, gy): owner, cost, status, area, box."""
    t = R.traversable(np.asarray(grid), clearance)
    h, w = t.shape
    key = {}
    pq = []
    status = []
    for b, xy in enumerate(bots):
        c = R.snap(t, xy, res, ox, oy, snap_radius)
        status.append(R.NO_START if c is None else R.OK)
        if c is not None and (c not in key or (0, b) < key[c]):
            key[c] = (0, b)
            heapq.heappush(pq, (0, b, c[0], c[1]))
    while pq:
        d, b, x, y = heapq.heappop(pq)
        if key[(x, y)] != (d, b):
            continue
        for dx, dy in R.MOVES:
            if R.legal(t, x, y, dx, dy):
                nk = (d + (R.DIAG if dx and dy else R.ORTHO), b)
                c = (x + dx, y + dy)
                if c not in key or nk < key[c]:
                    key[c] = nk
                    heapq.heappush(pq, (nk[0], b, c[0], c[1]))
    owner = np.full((h, w), -1, dtype=np.int16)
    cost = np.full((h, w), R.INF, dtype=np.uint32)
    n = len(bots)
    area = np.zeros(n, dtype=np.int64)
    box = np.full((n, 4), -1, dtype=np.int32)
    for (x, y), (d, b) in key.items():
        owner[y, x], cost[y, x] = b, d
        area[b] += 1
        box[b] = (x, y, x, y) if area[b] == 1 else (min(box[b, 0], x), min(box[b, 1], y), max(box[b, 2], x), max(box[b, 3], y))
    return dict(owner=owner, cost=cost, status=np.array(status, dtype=np.int32).reshape(n), area=area, box=box)


def both(grid, bots, res=1.0, ox=0.0, oy=0.0, clearance=0, snap_radius=2):
    grid = np.asarray(grid, dtype=np.int8)
    a = T.partition(grid, bots, res, ox, oy, clearance, snap_radius)
    b = multi_source(grid, bots, res, ox, oy, clearance, snap_radius)
    T.same(a, b, ("owner", "cost", "status", "area", "box"))
    assert a["area"].sum() == (a["owner"] >= 0).sum()
    return a


def centre(*cells):
    return [(gx + 0.5, gy + 0.5) for gx, gy in cells]


# ---- painted grids (res 1, origin 0: the world position of a cell's centre is gx + 0.5) ----------------------------------
def test_symmetric_scene_ties_go_to_the_lowest_bot():
    g = np.full((45, 45), -1, dtype=np.int8)
    g[2:43, 2:43] = 0                                         # 41 x 41: a middle row and column exist
    cells = [(12, 12), (32, 12), (12, 32), (32, 32)]
    a = both(g, centre(*cells))
    assert a["ties"] > 0 and a["owner"][22, 22] == 0 and a["owner"][5, 22] == 0 and a["owner"][40, 22] == 2
    assert a["owner"][22, 5] == 0 and a["owner"][22, 40] == 1
    assert a["area"].sum() == 41 * 41 and a["area"][0] > a["area"][1] > a["area"][3] and a["area"][1] == a["area"][2]
    order = [3, 1, 0, 2]                                      # the same cells in another order: other winners, same costs
    b = both(g, centre(*[cells[i] for i in order]))
    assert b["ties"] == a["ties"] and (b["cost"] == a["cost"]).all() and not (b["owner"] == a["owner"]).all()
    assert b["owner"][22, 22] == 0 and b["area"][0] == a["area"][0]          # whoever is first takes every tie
    assert a["box"][0].tolist() == [2, 2, 22, 22] and a["box"][3].tolist() == [23, 23, 42, 42]


def test_walled_scene_detours_sealed_room_and_degenerate_bots():
    g = np.full((40, 60), -1, dtype=np.int8)
    g[2:38, 2:58] = 0
    g[2:30, 30] = 100                                         # a wall with a gap at the top: detours
    g[10:20, 40:50] = 100                                     # a sealed room ...
    g[11:19, 41:49] = 0
    bots = centre((28, 4), (32, 4), (45, 15), (45, 15), (10, 35)) + [(math.nan, 3.0), (0.5, 0.5), (200.0, 1.0)]
    a = both(g, bots)
    assert a["status"].tolist() == [R.OK] * 5 + [R.NO_START] * 3
    assert a["area"][2] == 64 and a["box"][2].tolist() == [41, 11, 48, 18]          # exactly its own room
    assert a["area"][3] == 0 and a["box"][3].tolist() == [-1] * 4                   # shares bot 2's cell
    assert (a["area"][5:] == 0).all() and (a["box"][5:] == -1).all()
    assert a["owner"][4, 29] == 0 and a["owner"][4, 31] == 1 and a["cost"][4, 31] == 5
    assert a["owner"][36, 29] != 1                            # bot 1 is two cells away through the wall, far by path
    for cl in (1, 2):
        both(g, bots, clearance=cl, snap_radius=3)
    assert both(g, [])["area"].shape == (0,)
    one = both(g, bots[:1])
    assert one["area"][0] == (R.traversable(g, 0).sum() - 64)
    empty = both(np.full((20, 20), -1, dtype=np.int8), centre((3, 3)))
    assert empty["status"].tolist() == [R.NO_START] and (empty["owner"] == -1).all()


# ---- the oracle's 200 x 200 golden grids -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["session_200", "mixed_200"])
def test_golden_grids(name):
    grid, cents, bots, (res, ox, oy) = oracle_case(name)
    assert grid.shape == (200, 200) and len(bots) == 2
    rng = np.random.default_rng(len(name))
    ys, xs = np.nonzero(grid == 0)
    pick = rng.choice(len(ys), 5, replace=False)
    more = bots + [(ox + (xs[i] + 0.5) * res, oy + (ys[i] + 0.5) * res) for i in pick] + [bots[0]]
    for bl in (bots, more):
        a = both(grid, bl, res, ox, oy, clearance=2, snap_radius=10)
        assert (a["area"][:2] > 0).all()
    assert a["area"][-1] == 0 and a["status"][-1] == R.OK     # the copy of bot 0
    # T5 from the second restatement's arrays
    t = T.targets(grid, cents, more, res, ox, oy)
    ms = multi_source(grid, more, res, ox, oy, 2, 10)
    trav = R.traversable(grid, 2)
    best = {}
    for k, c in enumerate(cents.tolist()):
        cell = R.snap(trav, tuple(c), res, ox, oy, 10)
        o = -1 if cell is None else int(ms["owner"][cell[1], cell[0]])
        assert t["centroid_owner"][k] == o
        if o >= 0:
            assert t["centroid_cost"][k] == ms["cost"][cell[1], cell[0]]
            best[o] = min(best.get(o, (R.INF, -1)), (int(ms["cost"][cell[1], cell[0]]), k))
    for b in range(len(more)):
        if b in best:
            assert (int(t["cost_b"][b]), int(t["idx"][b])) == best[b] and t["status"][b] == R.OK
            assert t["centroid_owner"][t["idx"][b]] == b
            want = R.plan(trav, more[b], tuple(t["xy"][b]), res, ox, oy)
            assert want["status"] == R.OK and want["cost"] == t["cost_b"][b]
            assert tuple(t["waypoint_cell"][b]) == tuple(want["cell"]) and tuple(t["waypoint"][b]) == tuple(want["xy"])
        else:
            assert t["idx"][b] == -1 and t["status"][b] == R.UNREACHABLE and t["cost_b"][b] == R.INF
            assert np.isnan(t["xy"][b]).all() and tuple(t["waypoint_cell"][b]) == (-1, -1)
    assert len(best) >= 2
