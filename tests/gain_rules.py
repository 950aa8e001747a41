"""CPU restatement of the rules of include/quasar_slam.h, "frontier gain" (G1-G7), for the tests, on top of plan_rules.py
(the Bresenham walk) and assign_rules.py (cells, costs, the separation test, waypoints).

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]: -1 UNKNOWN, 0 FREE, 100 OCCUPIED)."""
import functools

import numpy as np

import assign_rules as A
import plan_rules as R

DEFAULT_RANGE, DEFAULT_BIAS, MAX_RANGE, MAX_BIAS = 24, 120, 64, 1 << 31
OUTSIDE = 50            # padding of a grid: neither UNKNOWN (a target) nor OCCUPIED (a blocker)


def clusters(grid, min_cluster=3):
    """G1: the 4-connected clusters of frontier cells (interior FREE cells with an UNKNOWN 4-neighbour) with at least
    min_cluster cells, ordered by first cell (row-major); each a sorted list of linear indices gy * size + gx."""
    from scipy import ndimage
    g = np.asarray(grid)
    size = g.shape[0]
    unk = g == -1
    near = np.zeros_like(unk)
    near[1:-1, 1:-1] = unk[1:-1, :-2] | unk[1:-1, 2:] | unk[:-2, 1:-1] | unk[2:, 1:-1]
    lab, n = ndimage.label((g == 0) & near, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    idx = np.flatnonzero(lab)
    order = np.argsort(lab.ravel()[idx], kind="stable")                    # members of one label together, ascending
    groups = np.split(idx[order], np.cumsum(np.bincount(lab.ravel()[idx])[1:])[:-1]) if n else []
    out = [m.tolist() for m in groups if len(m) >= min_cluster]
    return sorted(out, key=lambda m: m[0]), size


def centroids(cl, size, res, ox, oy):
    """cluster_centroid_world (:233-237) of each cluster: true division, then the cell centre."""
    out = []
    for m in cl:
        ax, ay = sum(i % size for i in m) / len(m), sum(i // size for i in m) / len(m)
        out.append((ox + (ax + 0.5) * res, oy + (ay + 0.5) * res))
    return out


def viewpoint(members, size):
    """G2 in plain Python: (gx, gy), and how many members share the smallest distance (the tie-break's cases)."""
    n = len(members)
    cx, cy = sum(i % size for i in members) // n, sum(i // size for i in members) // n
    keys = [((i % size - cx) ** 2 + (i // size - cy) ** 2, i) for i in members]
    d2, i = min(keys)
    return (i % size, i // size), sum(1 for k in keys if k[0] == d2)


def gain_direct(grid, v, rng):
    """G3 / G4 word for word for one viewpoint: every cell of the disc, its own _bresenham(v, t)."""
    g = np.asarray(grid)
    size = g.shape[0]
    vx, vy = v
    n = 0
    for ty in range(max(0, vy - rng), min(size, vy + rng + 1)):
        for tx in range(max(0, vx - rng), min(size, vx + rng + 1)):
            if (tx, ty) == (vx, vy) or (tx - vx) ** 2 + (ty - vy) ** 2 > rng * rng or g[ty, tx] != -1:
                continue
            n += all(g[y, x] != 100 for x, y in R.bresenham(vx, vy, tx, ty)[:-1])
    return n


@functools.lru_cache(maxsize=None)
def lines(rng):
    """The walk is translation-invariant: for every offset of the disc, row-major, the cells of
    _bresenham((0, 0), offset) but the last, padded with (0, 0) (the viewpoint: FREE).  (offsets [n, 2], cells [n, L, 2])"""
    offs, cells = [], []
    for dy in range(-rng, rng + 1):
        for dx in range(-rng, rng + 1):
            if (dx or dy) and dx * dx + dy * dy <= rng * rng:
                offs.append((dx, dy))
                cells.append(R.bresenham(0, 0, dx, dy)[:-1])
    L = max(len(c) for c in cells)
    arr = np.zeros((len(cells), L, 2), dtype=np.int64)
    for i, c in enumerate(cells):
        arr[i, :len(c)] = c
    return np.array(offs, dtype=np.int64), arr


def gains(grid, views, rng, chunk=32):
    """G3 / G4 for many viewpoints at once: int64 [n]."""
    offs, cells = lines(rng)
    p = np.pad(np.asarray(grid), rng, constant_values=OUTSIDE)
    v = np.asarray(views, dtype=np.int64).reshape(-1, 2) + rng
    out = np.zeros(len(v), dtype=np.int64)
    for a in range(0, len(v), chunk):
        w = v[a:a + chunk]
        target = p[w[:, None, 1] + offs[None, :, 1], w[:, None, 0] + offs[None, :, 0]] == -1
        hidden = (p[w[:, None, None, 1] + cells[None, :, :, 1], w[:, None, None, 0] + cells[None, :, :, 0]] == 100).any(axis=2)
        out[a:a + chunk] = (target & ~hidden).sum(axis=1)
    return out


def frontier_gain(grid, min_cluster=3, rng=DEFAULT_RANGE):
    """qs_frontier_gain: (viewpoints int32 [k, 2], gain int32 [k], members sharing the smallest distance [k])."""
    cl, size = clusters(grid, min_cluster)
    vt = [viewpoint(m, size) for m in cl]
    views = np.array([v for v, _ in vt], dtype=np.int32).reshape(-1, 2)
    return views, gains(grid, views, rng).astype(np.int32), [t for _, t in vt]


def before(c1, g1, k1, c2, g2, k2, bias):
    """G6: centroid k1 (cost c1, gain g1) comes before k2."""
    l, r = (c1 + bias) * g2, (c2 + bias) * g1
    return l < r or (l == r and (c1, k1) < (c2, k2))


def assign(grid, cents, gain, bots, res, ox, oy, separation, bias=DEFAULT_BIAS, clearance=2, snap_radius=10, lookahead=200,
           waypoints=True, top_k=None):
    """G7: assign_rules.assign with "smallest (cost, k)" replaced by "first in G6's order"; its dict plus gain int32 [n].
    With top_k also "fallbacks": the bots whose first top_k centroids in G6's order were all ineligible (what the device
    decides by a scan of every centroid)."""
    cents = [tuple(c) for c in np.asarray(cents, dtype=np.float64).reshape(-1, 2).tolist()]
    bots = [tuple(b) for b in np.asarray(bots, dtype=np.float64).reshape(-1, 2).tolist()]
    gain = [int(g) for g in gain]
    space = A.Space(grid, clearance)
    ccell, bcell, cost = A.costs(space, cents, bots, res, ox, oy, snap_radius)
    n = len(bots)
    out = dict(idx=np.full(n, -1, dtype=np.int64), xy=np.full((n, 2), np.nan), cost=np.full(n, A.INF, dtype=np.uint32),
               status=np.zeros(n, dtype=np.int32), waypoint_cell=np.full((n, 2), -1, dtype=np.int32),
               waypoint=np.full((n, 2), np.nan), gain=np.zeros(n, dtype=np.int32), centroid_cells=ccell, bot_cells=bcell)
    targets = []
    blocked = lambda k: any(k == tk or A.too_close(cents[k][0], cents[k][1], tx, ty, separation) for tk, tx, ty in targets)
    order = functools.cmp_to_key(lambda p, q: -1 if before(*p, *q, bias) else 1)
    out["fallbacks"] = 0
    for b in range(n):
        if bcell[b] is None:
            out["status"][b] = R.NO_START
            continue
        best = None
        finite = np.nonzero(cost[b] != A.INF)[0].tolist()
        if top_k is not None and len(finite) >= top_k:
            first = sorted(((int(cost[b, k]), gain[k], k) for k in finite), key=order)[:top_k]
            out["fallbacks"] += all(blocked(k) for _, _, k in first)
        for k in finite:
            if blocked(k):
                continue
            cand = (int(cost[b, k]), gain[k], k)
            if best is None or before(*cand, *best, bias):
                best = cand
        if best is None:
            out["status"][b] = R.UNREACHABLE
            continue
        c, g, k = best
        targets.append((k, cents[k][0], cents[k][1]))
        out["idx"][b], out["xy"][b], out["cost"][b], out["status"][b], out["gain"][b] = k, cents[k], c, R.OK, g
        if waypoints:
            pc, wp = space.plan(bcell[b], ccell[k], lookahead)
            assert pc == c, (b, k, pc, c)
            out["waypoint_cell"][b] = wp
            out["waypoint"][b] = (ox + (wp[0] + 0.5) * res, oy + (wp[1] + 0.5) * res)
    return out


KEYS = ("idx", "xy", "cost", "status", "waypoint_cell", "waypoint", "gain")
