"""CPU restatement of the rules of include/quasar_slam.h, "territories" (T1-T5), for the tests, on top of plan_rules.py and
assign_rules.Space.  It is independent of the device's construction: one shortest-path field PER BOT (scipy's Dijkstra),
folded in ascending bot order into the smallest (cost, bot) per cell -- not a multi-source relaxation.

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]); part of a large grid is restated through a Window."""
import numpy as np

import assign_rules as A
import plan_rules as R

INF = R.INF


class Window(A.Space):
    """A.Space over a window (x0, y0, x1, y1) of a large grid: rule 1 is evaluated on the window alone and every cell
    outside it counts as not traversable; coordinates stay the grid's.  It restates the whole grid's rules for the bots inside
    the window when no OCCUPIED cell outside lies within `clearance` of it and no move crosses its edge."""

    def __init__(self, grid, clearance, window):
        x0, y0, x1, y1 = window
        self.t = np.zeros(grid.shape, dtype=bool)
        self.t[y0:y1, x0:x1] = R.traversable(np.asarray(grid[y0:y1, x0:x1]), clearance)
        ys, xs = np.nonzero(self.t[y0:y1, x0:x1])
        self.empty = len(ys) == 0
        if not self.empty:
            self.x0, self.y0 = x0 + int(xs.min()), y0 + int(ys.min())
            self.tc = self.t[self.y0:y0 + int(ys.max()) + 1, self.x0:x0 + int(xs.max()) + 1]
            self.graph = R.move_graph(self.tc)
        self._last = (None, None)


def partition(grid, bots, res, ox, oy, clearance=2, snap_radius=10, space=None):
    """T1-T4: dict of owner int16 [h, w], cost uint32 [h, w], status int32 [n], area int64 [n], box int32 [n, 4],
    bot_cells, and ties = the cells at which two or more bots reach the minimum cost."""
    grid = np.asarray(grid)
    bots = [tuple(b) for b in np.asarray(bots, dtype=np.float64).reshape(-1, 2).tolist()]
    sp = A.Space(grid, clearance) if space is None else space
    n = len(bots)
    h, w = grid.shape
    owner = np.full((h, w), -1, dtype=np.int16)
    cost = np.full((h, w), INF, dtype=np.uint32)
    cells = [R.snap(sp.t, b, res, ox, oy, snap_radius) for b in bots]
    out = dict(owner=owner, cost=cost, status=np.array([R.NO_START if c is None else R.OK for c in cells], dtype=np.int32),
               area=np.zeros(n, dtype=np.int64), box=np.full((n, 4), -1, dtype=np.int32), bot_cells=cells, ties=0, space=sp)
    if sp.empty or not any(c is not None for c in cells):
        return out
    best = np.full(sp.tc.shape, INF, dtype=np.uint32)
    who = np.full(sp.tc.shape, -1, dtype=np.int16)
    reach = np.zeros(sp.tc.shape, dtype=np.int32)          # bots at the minimum
    for b, c in enumerate(cells):                          # ascending: a later bot needs a strictly smaller cost (T3)
        if c is None:
            continue
        f = sp.field(c)
        less = f < best
        reach[(f == best) & (f != INF)] += 1
        reach[less] = 1
        who[less] = b
        best[less] = f[less]
    best[~sp.tc] = INF                                     # (a field never reaches a non-traversable cell anyway)
    who[~sp.tc] = -1
    y1, x1 = sp.y0 + sp.tc.shape[0], sp.x0 + sp.tc.shape[1]
    owner[sp.y0:y1, sp.x0:x1] = who
    cost[sp.y0:y1, sp.x0:x1] = best
    out["ties"] = int((reach >= 2).sum())
    for b in range(n):                                     # T4
        ys, xs = np.nonzero(who == b)
        out["area"][b] = len(ys)
        if len(ys):
            out["box"][b] = (sp.x0 + xs.min(), sp.y0 + ys.min(), sp.x0 + xs.max(), sp.y0 + ys.max())
    return out


def targets(grid, cents, bots, res, ox, oy, clearance=2, snap_radius=10, lookahead=200, waypoints=True):
    """T5 on top of partition(): its keys plus idx, xy, cost_b (per bot; `cost` stays the per-cell array), status (with
    UNREACHABLE), waypoint_cell, waypoint, centroid_cells, centroid_owner int32 [k], centroid_cost uint32 [k]."""
    cents = [tuple(c) for c in np.asarray(cents, dtype=np.float64).reshape(-1, 2).tolist()]
    out = partition(grid, bots, res, ox, oy, clearance, snap_radius)
    sp = out["space"]
    n, k = len(out["bot_cells"]), len(cents)
    ccell = [R.snap(sp.t, c, res, ox, oy, snap_radius) for c in cents]
    cown = np.array([-1 if c is None else out["owner"][c[1], c[0]] for c in ccell], dtype=np.int32).reshape(k)
    ccost = np.array([INF if c is None else out["cost"][c[1], c[0]] for c in ccell], dtype=np.uint32).reshape(k)
    out.update(idx=np.full(n, -1, dtype=np.int64), xy=np.full((n, 2), np.nan), cost_b=np.full(n, INF, dtype=np.uint32),
               waypoint_cell=np.full((n, 2), -1, dtype=np.int32), waypoint=np.full((n, 2), np.nan), centroid_cells=ccell,
               centroid_owner=cown, centroid_cost=ccost)
    for b in range(n):
        if out["bot_cells"][b] is None:
            continue
        mine = [(int(ccost[j]), j) for j in np.nonzero(cown == b)[0].tolist()]
        if not mine:
            out["status"][b] = R.UNREACHABLE
            continue
        c, j = min(mine)
        out["idx"][b], out["xy"][b], out["cost_b"][b] = j, cents[j], c
        if waypoints:
            pc, wp = sp.plan(out["bot_cells"][b], ccell[j], lookahead)
            assert pc == c, (b, j, pc, c)                  # the field of the goal agrees with the partition (symmetric moves)
            out["waypoint_cell"][b] = wp
            out["waypoint"][b] = (ox + (wp[0] + 0.5) * res, oy + (wp[1] + 0.5) * res)       # grid_to_world
    return out


def same(got, want, keys):
    """Every value with ==; NaN equals NaN.  keys: names, or (name in got, name in want) pairs."""
    for key in keys:
        kg, kw = (key, key) if isinstance(key, str) else key
        a, b = np.asarray(got[kg]), np.asarray(want[kw])
        assert a.shape == b.shape and a.dtype == b.dtype, (key, a.shape, b.shape, a.dtype, b.dtype)
        eq = a == b
        if a.dtype.kind == "f":
            eq |= np.isnan(a) & np.isnan(b)
        assert eq.all(), (key, int((~eq).sum()), np.argwhere(~eq)[:8].tolist())
