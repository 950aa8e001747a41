"""CPU restatement of the rules of include/quasar_slam.h, "frontier targets by path cost", for the tests, on top of
plan_rules.py (the planning rules) and of test_frontier_targets_cpu.greedy's separation test.

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]); centroids are world positions in the order of
frontier_centroids(min_cluster)."""
import math

import numpy as np

import plan_rules as R

INF = R.INF


def too_close(cx, cy, tx, ty, sep):
    """qs_frontier_targets' test (dual_bot_mapper.py:977-981): sqrt(dx*dx + dy*dy) < separation, in fp64."""
    return math.sqrt((cx - tx) * (cx - tx) + (cy - ty) * (cy - ty)) < sep


class Space:
    """Rule 1 once: the traversable mask, and its bounding box with the move graph over it.  Fields, walks and waypoints
    only ever touch traversable cells (a Bresenham line between two of them stays in their bounding box), so they are
    computed over the box: the same values, without Dijkstra arrays the size of the whole grid."""

    def __init__(self, grid, clearance):
        self.t = R.traversable(np.asarray(grid), clearance)
        ys, xs = np.nonzero(self.t)
        self.empty = len(ys) == 0
        if not self.empty:
            self.x0, self.y0 = int(xs.min()), int(ys.min())
            self.tc = self.t[self.y0:int(ys.max()) + 1, self.x0:int(xs.max()) + 1]
            self.graph = R.move_graph(self.tc)
        self._last = (None, None)

    def field(self, cell):
        """Rule 3 seeded at a grid cell, over the box (the last one is kept: consecutive bots on one cell share it)."""
        if self._last[0] != cell:
            self._last = (cell, R.field_scipy(self.tc, (cell[0] - self.x0, cell[1] - self.y0), self.graph))
        return self._last[1]

    def at(self, f, cell):
        return int(f[cell[1] - self.y0, cell[0] - self.x0])

    def plan(self, s, g, lookahead):
        """plan_rules.plan's rules 3-5 between two cells that exist: (cost, waypoint cell) or None when not connected."""
        f = self.field(g)
        if self.at(f, s) == INF:
            return None
        sc, gc = (s[0] - self.x0, s[1] - self.y0), (g[0] - self.x0, g[1] - self.y0)
        wp = R.waypoint(self.tc, R.walk(self.tc, f, sc, gc), lookahead)
        return self.at(f, s), (wp[0] + self.x0, wp[1] + self.y0)


def costs(space, cents, bots, res, ox, oy, snap_radius=10):
    """Rules 2 and 3: (centroid cells, bot cells, cost uint32 [n_bots, n_cents]); a cell is (gx, gy) or None."""
    ccell = [R.snap(space.t, c, res, ox, oy, snap_radius) for c in cents]
    bcell = [R.snap(space.t, b, res, ox, oy, snap_radius) for b in bots]
    cost = np.full((len(bots), len(cents)), INF, dtype=np.uint32)
    have = [k for k, c in enumerate(ccell) if c is not None]
    for b, s in enumerate(bcell):
        if s is None or not have:
            continue
        f = space.field(s)                                 # seeded at the bot: the moves are symmetric
        cost[b, have] = [space.at(f, ccell[k]) for k in have]
    return ccell, bcell, cost


def assign(grid, cents, bots, res, ox, oy, separation, clearance=2, snap_radius=10, lookahead=200, waypoints=True):
    """Rules 1-5: dict of idx int64 [n], xy float64 [n, 2], cost uint32 [n], status int32 [n], waypoint_cell int32
    [n, 2], waypoint float64 [n, 2], and n_cost (reachable centroids per bot, before the greedy's exclusions)."""
    cents = [tuple(c) for c in np.asarray(cents, dtype=np.float64).reshape(-1, 2).tolist()]
    bots = [tuple(b) for b in np.asarray(bots, dtype=np.float64).reshape(-1, 2).tolist()]
    space = Space(grid, clearance)
    ccell, bcell, cost = costs(space, cents, bots, res, ox, oy, snap_radius)
    n = len(bots)
    out = dict(idx=np.full(n, -1, dtype=np.int64), xy=np.full((n, 2), np.nan), cost=np.full(n, INF, dtype=np.uint32),
               status=np.zeros(n, dtype=np.int32), waypoint_cell=np.full((n, 2), -1, dtype=np.int32),
               waypoint=np.full((n, 2), np.nan), n_cost=(cost != INF).sum(axis=1), centroid_cells=ccell, bot_cells=bcell)
    targets = []                                           # (k, x, y) of the earlier bots
    for b in range(n):
        if bcell[b] is None:
            out["status"][b] = R.NO_START
            continue
        best = None
        for k in np.nonzero(cost[b] != INF)[0].tolist():
            cx, cy = cents[k]
            if any(k == tk or too_close(cx, cy, tx, ty, separation) for tk, tx, ty in targets):
                continue
            key = (int(cost[b, k]), k)
            if best is None or key < best:
                best = key
        if best is None:
            out["status"][b] = R.UNREACHABLE
            continue
        k = best[1]
        targets.append((k, cents[k][0], cents[k][1]))
        out["idx"][b], out["xy"][b], out["cost"][b], out["status"][b] = k, cents[k], best[0], R.OK
        if waypoints:
            c, wp = space.plan(bcell[b], ccell[k], lookahead)
            assert c == best[0], (b, k, c, best[0])        # the field of the goal agrees with the field of the bot
            out["waypoint_cell"][b] = wp
            out["waypoint"][b] = (ox + (wp[0] + 0.5) * res, oy + (wp[1] + 0.5) * res)       # grid_to_world
    return out


def same(got, want, keys=("idx", "xy", "cost", "status", "waypoint_cell", "waypoint")):
    """Every output of every bot with ==; NaN equals NaN."""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        eq = a == b
        if a.dtype.kind == "f":
            eq |= np.isnan(a) & np.isnan(b)
        assert eq.all(), (k, np.argwhere(~eq)[:8].tolist())
