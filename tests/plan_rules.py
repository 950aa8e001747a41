"""CPU restatement of the path-planning rules of include/quasar_slam.h ("path planning"), for the tests.

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]: -1 UNKNOWN, 0 FREE, 100 OCCUPIED), which is
the stamp reading of the device (0 = UNKNOWN, even = FREE, odd = OCCUPIED)."""
import heapq
import math

import numpy as np

ORTHO, DIAG = 5, 7
INF = 0xFFFFFFFF
OK, NO_START, NO_GOAL, UNREACHABLE = 0, 1, 2, 3
# E, N, W, S, NE, NW, SW, SE (N = +y)
MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))


def traversable(grid, clearance):
    """Rule 1: FREE and no OCCUPIED cell with dx*dx + dy*dy <= clearance^2 (exact nearest occupied cell by scipy's EDT)."""
    from scipy import ndimage
    free = grid == 0
    occ = grid == 100
    if clearance == 0 or not occ.any():
        return free & ~occ
    iy, ix = ndimage.distance_transform_edt(~occ, return_distances=False, return_indices=True)
    yy, xx = np.indices(grid.shape)
    d2 = (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2
    return free & (d2 > clearance * clearance)


def traversable_brute(grid, clearance):
    """Rule 1 word for word (small grids)."""
    h, w = grid.shape
    out = np.zeros((h, w), dtype=bool)
    occ = np.argwhere(grid == 100)
    for y in range(h):
        for x in range(w):
            if grid[y, x] != 0:
                continue
            out[y, x] = not any((oy - y) ** 2 + (ox - x) ** 2 <= clearance * clearance for oy, ox in occ)
    return out


def legal(t, x, y, dx, dy):
    """A move from (x, y) by (dx, dy): both cells traversable, and for a diagonal both orthogonal neighbours."""
    h, w = t.shape
    nx, ny = x + dx, y + dy
    if not (0 <= nx < w and 0 <= ny < h and t[ny, nx]):
        return False
    if dx and dy:
        return bool(t[y, nx] and t[ny, x])
    return True


def field_heapq(t, goal):
    """Rule 3 by Dijkstra with heapq (small grids): uint32 [h, w]."""
    h, w = t.shape
    f = np.full((h, w), INF, dtype=np.uint32)
    gx, gy = goal
    f[gy, gx] = 0
    pq = [(0, gx, gy)]
    while pq:
        d, x, y = heapq.heappop(pq)
        if d != f[y, x]:
            continue
        for dx, dy in MOVES:
            if legal(t, x, y, dx, dy):
                nd = d + (DIAG if dx and dy else ORTHO)
                if nd < f[y + dy, x + dx]:
                    f[y + dy, x + dx] = nd
                    heapq.heappush(pq, (nd, x + dx, y + dy))
    return f


def move_graph(t):
    """The legal moves of rule 3 as a scipy CSR matrix over linear indices gy * w + gx."""
    from scipy import sparse
    h, w = t.shape
    rows, cols, wts = [], [], []
    yy, xx = np.nonzero(t)
    for dx, dy in MOVES:
        nx, ny = xx + dx, yy + dy
        ok = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
        ok[ok] &= t[ny[ok], nx[ok]]
        if dx and dy:
            ok[ok] &= t[yy[ok], nx[ok]] & t[ny[ok], xx[ok]]
        rows.append(yy[ok] * w + xx[ok])
        cols.append(ny[ok] * w + nx[ok])
        wts.append(np.full(int(ok.sum()), float(DIAG if dx and dy else ORTHO)))
    n = h * w
    return sparse.csr_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))


def field_scipy(t, goal, graph=None):
    """Rule 3 by scipy.sparse.csgraph.dijkstra (the moves are symmetric, so distances from the goal are distances to it)."""
    from scipy.sparse import csgraph
    h, w = t.shape
    g = move_graph(t) if graph is None else graph
    d = csgraph.dijkstra(g, directed=True, indices=goal[1] * w + goal[0])
    out = np.full(h * w, INF, dtype=np.uint32)
    fin = np.isfinite(d)
    out[fin] = d[fin].astype(np.uint32)
    return out.reshape(h, w)


def world_to_grid(w, o, res):
    """dual_bot_mapper.py:121-125; None where CPython's int() would raise."""
    q = (w - o) / res
    if math.isnan(q) or math.isinf(q):
        return None
    return int(q)


def snap(t, xy, res, ox, oy, radius):
    """Rule 2: the cell, or None."""
    h, w = t.shape
    gx, gy = world_to_grid(xy[0], ox, res), world_to_grid(xy[1], oy, res)
    if gx is None or gy is None or not (0 <= gx < w and 0 <= gy < h):
        return None
    if t[gy, gx]:
        return (gx, gy)
    best = None
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = gx + dx, gy + dy
            if dx * dx + dy * dy <= radius * radius and 0 <= x < w and 0 <= y < h and t[y, x]:
                key = (dx * dx + dy * dy, y * w + x)
                if best is None or key < best:
                    best = key
    return None if best is None else (best[1] % w, best[1] // w)


def bresenham(x0, y0, x1, y1):
    """OccupancyGrid._bresenham (dual_bot_mapper.py:158-179)."""
    cells = []
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx = 1 if x0 < x1 else -1
    sy = 1 if y0 < y1 else -1
    err = dx - dy
    while True:
        cells.append((x0, y0))
        if x0 == x1 and y0 == y1:
            break
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x0 += sx
        if e2 < dx:
            err += dx
            y0 += sy
    return cells


def walk(t, f, start, goal):
    """Rule 4: the path cells from start to goal (start included)."""
    x, y = start
    path = [(x, y)]
    while (x, y) != tuple(goal):
        for dx, dy in MOVES:
            if legal(t, x, y, dx, dy) and int(f[y + dy, x + dx]) + (DIAG if dx and dy else ORTHO) == int(f[y, x]):
                x, y = x + dx, y + dy
                break
        else:
            raise AssertionError("no descending move")
        path.append((x, y))
    return path


def waypoint(t, path, lookahead):
    """Rule 5: the waypoint cell of a path."""
    sx, sy = path[0]
    wp = path[0]
    for cell in path[1:min(lookahead, len(path) - 1) + 1]:
        if not all(t[cy, cx] for cx, cy in bresenham(sx, sy, cell[0], cell[1])):
            return wp
        wp = cell
    return wp


def plan(t, start_xy, goal_xy, res, ox, oy, snap_radius=10, lookahead=200, graph=None):
    """Rules 2-5 for one request: dict(status, cell, xy, cost, path)."""
    out = dict(status=None, cell=(-1, -1), xy=(math.nan, math.nan), cost=INF, path=[])
    s = snap(t, start_xy, res, ox, oy, snap_radius)
    g = snap(t, goal_xy, res, ox, oy, snap_radius)
    if s is None:
        out["status"] = NO_START
        return out
    if g is None:
        out["status"] = NO_GOAL
        return out
    f = field_scipy(t, g, graph)
    if f[s[1], s[0]] == INF:
        out["status"] = UNREACHABLE
        return out
    path = walk(t, f, s, g)
    wp = waypoint(t, path, lookahead)
    out.update(status=OK, cell=wp, xy=(ox + (wp[0] + 0.5) * res, oy + (wp[1] + 0.5) * res), cost=int(f[s[1], s[0]]),
               path=path)
    return out
