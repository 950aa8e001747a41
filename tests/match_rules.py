"""CPU restatement of the sweep-matching rules of include/quasar_slam.h ("sweep matching"), for the tests.

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]: -1 UNKNOWN, 0 FREE, 100 OCCUPIED), which is
the stamp reading of the device (odd = OCCUPIED).  Everything after the (sin, cos) of a rotation is exact integer or
uncontracted fp64 arithmetic, so with the device's own rotation table as input the device must equal this bit for bit.

Also here: the synthetic room the recovery and GPU tests share (this file's own geometry)."""
import math

import numpy as np

DEFAULTS = dict(radius=2, window=6, angle_steps=10, min_hits=20, min_percent=50, angle_step=math.pi / 180)
MAX_RADIUS, MAX_ANGLE_STEPS, MAX_REACH = 7, 45, 127
BEAMS = 181
MATCH_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("it", "<i4"), ("score", "<i4"), ("score0", "<i4"), ("hits", "<i4"),
                        ("accepted_record", "u1"), ("accepted_match", "u1"), ("pad", "u1", (6,)),
                        ("dx", "<f8"), ("dy", "<f8"), ("dyaw", "<f8")])
FIELDS = ("ix", "iy", "it", "score", "score0", "hits", "accepted_record", "accepted_match", "dx", "dy", "dyaw")
# cos / sin of the beam angles (i - 90) * (pi / 180): libm through CPython
CB = np.array([math.cos((i - 90) * (math.pi / 180)) for i in range(BEAMS)])
SB = np.array([math.sin((i - 90) * (math.pi / 180)) for i in range(BEAMS)])


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- rule 1: the likelihood field --------------------------------------------------------------------------------------------
def field(grid, radius):
    """max(0, R + 1 - Chebyshev distance to the nearest OCCUPIED cell), by scipy's chessboard distance transform."""
    from scipy import ndimage
    occ = grid == 100
    if not occ.any():
        return np.zeros(grid.shape, dtype=np.uint8)
    c = ndimage.distance_transform_cdt(~occ, metric="chessboard").astype(np.int64)
    return np.maximum(0, radius + 1 - c).astype(np.uint8)


def field_filter(grid, radius):
    """The same by R rounds of a 3 x 3 maximum filter that loses 1 per round (the form the device's patch uses)."""
    from scipy import ndimage
    v = np.where(grid == 100, radius + 1, 0).astype(np.int64)
    for _ in range(radius):
        v = np.maximum(v, ndimage.maximum_filter(v, size=3, mode="constant", cval=0) - 1)
    return v.astype(np.uint8)


def field_brute(grid, radius):
    """Word for word (small grids)."""
    size_y, size_x = grid.shape
    out = np.zeros(grid.shape, dtype=np.uint8)
    occ = [(int(y), int(x)) for y, x in zip(*np.nonzero(grid == 100))]
    for gy in range(size_y):
        for gx in range(size_x):
            c = min((max(abs(gx - x), abs(gy - y)) for y, x in occ), default=None)
            out[gy, gx] = 0 if c is None else max(0, radius + 1 - c)
    return out


# ---- rule 3: poses and cells -------------------------------------------------------------------------------------------------
def records_of(buf):
    """Structured view of uint8 [n, 743 | 751] sweep records."""
    head = [("magic", "S4"), ("agent", "u1"), ("x", "<f4"), ("y", "<f4"), ("yaw", "<f4")]
    odo = [("enc", "<i4"), ("v2v", "<u4")] if buf.shape[1] == 751 else []
    dt = np.dtype(head + odo + [("scan_count", "<u2"), ("ranges", "<f4", (BEAMS,))])
    assert dt.itemsize == buf.shape[1]
    return np.ascontiguousarray(buf).view(dt).reshape(-1)


def poses_of(recs, lengths=None, offset=None, drift=None, max_agent=2):
    """(accepted bool [n], pose float64 [n, 3]) as qs_ingest_sweeps forms them: offset first, then drift."""
    offset, drift = offset or {}, drift or {}
    n = len(recs)
    acc = np.zeros(n, dtype=bool)
    pose = np.zeros((n, 3))
    for k, r in enumerate(recs):
        a = int(r["agent"])
        if r["magic"] != b"QSRL" or not 1 <= a <= max_agent or (lengths is not None and int(lengths[k]) != recs.dtype.itemsize):
            continue
        dx, dy = drift.get(a, (0.0, 0.0))
        acc[k] = True
        pose[k] = ((float(r["x"]) + offset.get(a, 0.0)) + dx, float(r["y"]) + dy, float(r["yaw"]))
    return acc, pose


def world_to_grid(w, o, res):
    """(cell int64, valid): int((w - o) / res), truncation toward zero; not valid where the quotient is not finite (or
    beyond 9e15, where CPython would walk 1e15 cells)."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = (np.asarray(w, dtype=np.float64) - o) / res
        ok = np.abs(q) < 9.0e15
        return np.trunc(np.where(ok, q, 0.0)).astype(np.int64), ok


def rotations_libm(yaw, T, step):
    """[2 T + 1, 2] (sin, cos) of yaw + it * step from libm."""
    return np.array([[math.sin(yaw + it * step), math.cos(yaw + it * step)] for it in range(-T, T + 1)])


# ---- rules 2-5: one sweep ------------------------------------------------------------------------------------------------------
def match_one(L, geom, pose, ranges, p, smin, smax, rot=None):
    """One accepted sweep.  L: the field of the whole grid; geom = (res, ox, oy); pose = (rx, ry, yaw); ranges float32 [181];
    rot: [2 T + 1, 2] (sin, cos) or None (libm).  Returns a dict of the qs_sweep_match fields."""
    res, ox, oy = geom
    R, W, T, step = p["radius"], p["window"], p["angle_steps"], p["angle_step"]
    rx, ry, yaw = (float(v) for v in pose)
    d = ranges.astype(np.float64)
    with np.errstate(invalid="ignore"):
        hit = (smin < d) & (d <= smax)
    H = int(hit.sum())
    bx, by = d[hit] * CB[hit], d[hit] * SB[hit]
    if rot is None:
        rot = rotations_libm(yaw, T, step)
    size = L.shape[0]
    Lp = np.pad(L.astype(np.int32), 2 * W) if W else L.astype(np.int32)
    sh = np.arange(-W, W + 1)
    scores = np.zeros((2 * T + 1, 2 * W + 1, 2 * W + 1), dtype=np.int64)          # [it, iy, ix]
    for ti in range(2 * T + 1):
        s, c = float(rot[ti, 0]), float(rot[ti, 1])
        with np.errstate(invalid="ignore", over="ignore"):
            ex = rx + (c * bx - s * by)
            ey = ry + (s * bx + c * by)
        cx, okx = world_to_grid(ex, ox, res)
        cy, oky = world_to_grid(ey, oy, res)
        # a cell more than W outside the grid scores 0 under every shift
        use = okx & oky & (cx >= -W) & (cx < size + W) & (cy >= -W) & (cy < size + W)
        if not use.any():
            continue
        cx, cy = cx[use] + 2 * W, cy[use] + 2 * W
        scores[ti] = Lp[cy[:, None, None] + sh[None, :, None], cx[:, None, None] + sh[None, None, :]].sum(axis=0)
    it, iy, ix = np.meshgrid(np.arange(-T, T + 1), sh, sh, indexing="ij")
    sc, it, iy, ix = scores.ravel(), it.ravel(), iy.ravel(), ix.ravel()
    # highest score; then smallest ix^2 + iy^2, smallest |it|, smaller it, smaller iy, smaller ix (lexsort: last key first)
    b = np.lexsort((ix, iy, it, np.abs(it), ix * ix + iy * iy, -sc))[0]
    best = int(sc[b])
    ok = H >= p["min_hits"] and best * 100 >= p["min_percent"] * H * (R + 1)
    return dict(ix=int(ix[b]), iy=int(iy[b]), it=int(it[b]), score=best, score0=int(scores[T, W, W]), hits=H,
                accepted_record=1, accepted_match=int(ok),
                dx=float(ix[b]) * res if ok else 0.0, dy=float(iy[b]) * res if ok else 0.0,
                dyaw=float(it[b]) * step if ok else 0.0)


def match(grid, geom, buf, p=None, lengths=None, smin=0.1, smax=1.2, rot=None, offset=None, drift=None, max_agent=2):
    """Every record of buf (uint8 [n, 743 | 751]) against grid: MATCH_DTYPE [n].  rot: [n, 2 T + 1, 2] or None."""
    p = params(**(p or {}))
    recs = records_of(buf)
    acc, pose = poses_of(recs, lengths, offset, drift, max_agent)
    L = field(grid, p["radius"])
    out = np.zeros(len(recs), dtype=MATCH_DTYPE)
    for k in np.nonzero(acc)[0]:
        r = match_one(L, geom, pose[k], recs["ranges"][k], p, smin, smax, None if rot is None else rot[k])
        for f, v in r.items():
            out[f][k] = v
    return out


def limit_ok(p, smax, res):
    return math.ceil(smax / res) + p["window"] + p["radius"] + 2 <= MAX_REACH


# ---- the sweep rule of qs_ingest_sweeps, for driving update_ray beam by beam ---------------------------------------------------
def beams_of(pose, ranges, smin, smax):
    """(rx, ry, hx, hy, valid) of the 181 beams of one sweep cast from pose (CPython arithmetic, libm trig)."""
    rx, ry, yaw = (float(v) for v in pose)
    hx, hy, valid = [], [], []
    for i, d in enumerate(ranges.tolist()):
        a = yaw + math.radians(i - 90)
        ok = smin < d <= smax
        length = d if ok else (min(d, smax) if d > smin else smax)
        hx.append(rx + length * math.cos(a)); hy.append(ry + length * math.sin(a)); valid.append(1 if ok else 0)
    n = len(valid)
    return np.full(n, rx), np.full(n, ry), np.array(hx), np.array(hy), np.array(valid, dtype=np.uint8)


def beams_of_all(poses, ranges, smin, smax):
    parts = [beams_of(p, r, smin, smax) for p, r in zip(poses, ranges)]
    return [np.concatenate([q[j] for q in parts]) for j in range(5)] if parts else None


# ---- the synthetic room ---------------------------------------------------------------------------------------------------------
ROOM_SMIN, ROOM_SMAX = 0.1, 3.0
ROOM_GRID = (200, 0.05, -5.0, -5.0)          # size, res, ox, oy


def room_segments():
    """Outer walls, a box and two partitions: [m, 4] (x0, y0, x1, y1)."""
    seg = []

    def rect(x0, y0, x1, y1):
        seg.extend([(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)])
    # (every wall runs through the middle of a row or column of cells of ROOM_GRID)
    rect(-3.075, -2.275, 2.925, 2.525)                # outer walls
    rect(0.725, -0.875, 1.525, -0.175)                # a box
    seg.append((-3.075, 0.475, -1.175, 0.475))        # a partition from the west wall
    seg.append((-0.325, 2.525, -0.325, 1.125))        # a partition from the north wall
    return np.array(seg, dtype=np.float64)


def cast(segments, pose, rng=None, sigma=0.0, far=ROOM_SMAX):
    """Ranges float32 [181] of a sweep at pose: nearest intersection of each beam with the segments; beyond `far` or
    nothing: 0 (no echo)."""
    x, y, yaw = pose
    ang = yaw + (np.arange(BEAMS) - 90) * (math.pi / 180)
    dx, dy = np.cos(ang)[:, None], np.sin(ang)[:, None]
    x0, y0, x1, y1 = (segments[:, j][None, :] for j in range(4))
    sx, sy = x1 - x0, y1 - y0
    den = dx * sy - dy * sx
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((x0 - x) * sy - (y0 - y) * sx) / den
        u = ((x0 - x) * dy - (y0 - y) * dx) / den
    t = np.where((np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1), t, np.inf)
    d = t.min(axis=1)
    if rng is not None and sigma > 0:
        d = d + rng.normal(0.0, sigma, BEAMS)
    return np.where(d <= far, d, 0.0).astype(np.float32)


def _pose_ok(seg, x, y):
    a, b = seg[:, :2], seg[:, 2:]
    ab = b - a
    tt = np.clip(((np.array([x, y]) - a) * ab).sum(1) / (ab * ab).sum(1), 0, 1)
    dist = np.hypot(*(a + tt[:, None] * ab - np.array([x, y])).T)
    return dist.min() >= 0.4 and not (0.725 <= x <= 1.525 and -0.875 <= y <= -0.175)


def room_poses(rng, n, spread=False):
    """Poses inside the room, at least 0.4 m from every wall segment.  spread: one pose in each cell of a 6 x 5 lattice over
    the room in turn (so that a mapping run of 30 sweeps sees every corner of it), else anywhere."""
    seg = room_segments()
    x_lo, x_hi, y_lo, y_hi = -2.675, 2.525, -1.875, 2.125
    out = []
    while len(out) < n:
        bx0, bx1, by0, by1 = x_lo, x_hi, y_lo, y_hi
        if spread:
            cx, cy = len(out) % 6, (len(out) // 6) % 5
            bx0, bx1 = x_lo + (x_hi - x_lo) * cx / 6, x_lo + (x_hi - x_lo) * (cx + 1) / 6
            by0, by1 = y_lo + (y_hi - y_lo) * cy / 5, y_lo + (y_hi - y_lo) * (cy + 1) / 5
        for attempt in range(200):
            wide = attempt >= 100                      # (a lattice cell with no room in it: anywhere)
            x = rng.uniform(x_lo if wide else bx0, x_hi if wide else bx1)
            y = rng.uniform(y_lo if wide else by0, y_hi if wide else by1)
            if _pose_ok(seg, x, y):
                break
        out.append((x, y, rng.uniform(-math.pi, math.pi)))
    return np.array(out)


def room_session(seed, n_map, n_query, window, angle_steps, angle_step=math.pi / 180, sigma=0.01):
    """A seeded session in the room: n_map sweeps at their true poses (for mapping), n_query sweeps whose reported pose is
    the true pose displaced by whole cells (|.| <= window) and whole angle steps (|.| <= angle_steps).
    Returns dict(map_pose, map_ranges, q_true, q_pose, q_ranges, q_disp int [n, 3])."""
    rng = np.random.default_rng(seed)
    seg = room_segments()
    res = ROOM_GRID[1]
    mp = room_poses(rng, n_map, spread=True)
    qt = room_poses(rng, n_query)
    disp = np.stack([rng.integers(-window, window + 1, n_query), rng.integers(-window, window + 1, n_query),
                     rng.integers(-angle_steps, angle_steps + 1, n_query)], axis=1)
    qp = qt + disp * np.array([res, res, angle_step])
    # what the packet carries is f32: the pose the matcher sees is that rounding of the displaced pose
    qp = qp.astype(np.float32).astype(np.float64)
    mp = mp.astype(np.float32).astype(np.float64)
    return dict(map_pose=mp, map_ranges=np.stack([cast(seg, p, rng, sigma) for p in mp]),
                q_true=qt, q_pose=qp, q_ranges=np.stack([cast(seg, p, rng, sigma) for p in qt]), q_disp=disp)


def recovered(m, disp):
    """The returned candidate cancels the displacement to within one cell on each axis and one angle step."""
    return (abs(int(m["ix"]) + int(disp[0])) <= 1 and abs(int(m["iy"]) + int(disp[1])) <= 1
            and abs(int(m["it"]) + int(disp[2])) <= 1)
