"""CPU restatement of the relocalisation rules G1-G9 of include/quasar_slam.h ("relocalisation"), for the tests.

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]: -1 UNKNOWN, 0 FREE, 100 OCCUPIED).  Everything is
exact integer or uncontracted fp64 arithmetic and the rotations' (sin, cos) are libm's on both sides, so the device must equal
this bit for bit.  Two forms: `reloc_one`, vectorised (per rotation and distinct beam offset one shifted add of the padded
field), and `reloc_one_brute`, word for word, for small grids.

Also here: the world the recovery and GPU tests share, the small world whose free cells touch the grid's border, query poses, and
the rays that paint a grid into a mapper."""
import math

import numpy as np

import match_rules as MR

DEFAULTS = dict(radius=2, n_rot=180, sep=4, sep_rot=2, min_hits=40, min_percent=70, min_margin=5, box=None)
MAX_ROT, MAX_SEP, TILE = 360, 16, 16
OK, NO_RECORD, NO_CANDIDATE = 0, 1, 2
BEAMS = 181
RELOC_DTYPE = np.dtype([("gx", "<i4"), ("gy", "<i4"), ("j", "<i4"), ("score", "<i4"), ("hits", "<i4"),
                        ("gx2", "<i4"), ("gy2", "<i4"), ("j2", "<i4"), ("score2", "<i4"), ("status", "<i4"),
                        ("accepted_record", "u1"), ("accepted", "u1"), ("pad", "u1", (6,)),
                        ("x", "<f8"), ("y", "<f8"), ("yaw", "<f8")])
FIELDS = ("gx", "gy", "j", "score", "hits", "gx2", "gy2", "j2", "score2", "status", "accepted_record", "accepted", "x", "y", "yaw")


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def limit_ok(p, smax, res):
    return (0 <= p["radius"] <= MR.MAX_RADIUS and 1 <= p["n_rot"] <= MAX_ROT and 0 <= p["sep"] <= MAX_SEP
            and 0 <= p["sep_rot"] < p["n_rot"] and TILE + 2 * (math.ceil(smax / res) + p["radius"] + 1) <= 255)


# ---- G2, G3 -------------------------------------------------------------------------------------------------------------------
def rotations(n_rot):
    """[n_rot, 3]: sin, cos of th_j = j * (2 pi / n_rot) from libm, and the yaw reported for j (G8)."""
    step = 2 * math.pi / n_rot
    out = []
    for j in range(n_rot):
        th = j * step
        out.append((math.sin(th), math.cos(th), th - 2 * math.pi if th > math.pi else th))
    return np.array(out)


def beam_offsets(ranges, rot, res, smin, smax):
    """(H, ax int64 [n_rot, H], ay): the cell offsets of the hit beams' end points under every rotation."""
    d = np.asarray(ranges, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        hit = (smin < d) & (d <= smax)
    bx, by = d[hit] * MR.CB[hit], d[hit] * MR.SB[hit]
    S, C = rot[:, 0][:, None], rot[:, 1][:, None]
    ex = C * bx[None, :] - S * by[None, :]
    ey = S * bx[None, :] + C * by[None, :]
    return int(hit.sum()), np.floor(ex / res + 0.5).astype(np.int64), np.floor(ey / res + 0.5).astype(np.int64)


def clip_box(box, size):
    """(x0, y0, x1, y1) of the search box clipped to the grid; None: the whole grid."""
    if box is None:
        return 0, 0, size, size
    x0, y0, x1, y1 = (int(v) for v in box)
    return max(x0, 0), max(y0, 0), min(x1, size), min(y1, size)


def _result(status, H=0, rec=1):
    r = dict.fromkeys(FIELDS, 0)
    r.update(status=status, accepted_record=rec, hits=H, x=0.0, y=0.0, yaw=0.0)
    if status != NO_RECORD:
        r.update(gx=-1, gy=-1, j=-1, gx2=-1, gy2=-1, j2=-1)
    return r


def _finish(r, best, rival, H, p, geom, rot):
    """G6's outcome, G7, G8 from the best and rival (score, j, gy, gx) tuples (rival None: none)."""
    res, ox, oy = geom
    R = p["radius"]
    r.update(status=OK, score=best[0], j=best[1], gy=best[2], gx=best[3])
    if rival is not None:
        r.update(score2=rival[0], j2=rival[1], gy2=rival[2], gx2=rival[3])
    full = H * (R + 1)
    r["accepted"] = int(H >= p["min_hits"] and r["score"] * 100 >= p["min_percent"] * full
                        and (r["score"] - r["score2"]) * 100 >= p["min_margin"] * full)
    r["x"] = ox + (float(r["gx"]) + 0.5) * res
    r["y"] = oy + (float(r["gy"]) + 0.5) * res
    r["yaw"] = float(rot[r["j"], 2])
    return r


# ---- G4-G9, vectorised -----------------------------------------------------------------------------------------------------------
def reloc_one(L, free, geom, ranges, p, smin, smax, rot=None):
    """One accepted sweep.  L: the field of the whole grid (MR.field(grid, radius)); free: grid == 0; geom = (res, ox, oy)."""
    res = geom[0]
    size = L.shape[0]
    n_rot, sep, sep_rot = p["n_rot"], p["sep"], p["sep_rot"]
    if rot is None:
        rot = rotations(n_rot)
    H, ax, ay = beam_offsets(ranges, rot, res, smin, smax)
    x0, y0, x1, y1 = clip_box(p.get("box"), size)
    if H == 0 or x1 <= x0 or y1 <= y0 or not free[y0:y1, x0:x1].any():
        return _result(NO_CANDIDATE, H)
    pad = int(max(np.abs(ax).max(), np.abs(ay).max()))
    Lp = np.pad(L.astype(np.int16), pad)
    cand = free[y0:y1, x0:x1]
    vol = np.empty((n_rot, y1 - y0, x1 - x0), dtype=np.int16)                   # score, -1 where the cell is no candidate
    for j in range(n_rot):
        off, cnt = np.unique(np.stack([ay[j], ax[j]], axis=1), axis=0, return_counts=True)
        acc = np.zeros((y1 - y0, x1 - x0), dtype=np.int16)
        for (oy_, ox_), c in zip(off.tolist(), cnt.tolist()):
            sl = Lp[y0 + pad + oy_:y1 + pad + oy_, x0 + pad + ox_:x1 + pad + ox_]
            acc += sl if c == 1 else sl * np.int16(c)
        vol[j] = np.where(cand, acc, -1)
    # G5: the first maximum in (j, gy, gx) order
    bj, by_, bx_ = np.unravel_index(int(np.argmax(vol)), vol.shape)
    best = (int(vol[bj, by_, bx_]), int(bj), int(by_) + y0, int(bx_) + x0)
    # G6: without the candidates close to the best on both axes AND in rotation
    dj = np.abs(np.arange(n_rot) - bj)
    near_j = np.nonzero(np.minimum(dj, n_rot - dj) <= sep_rot)[0]
    ya, yb = max(by_ - sep, 0), min(by_ + sep + 1, y1 - y0)
    xa, xb = max(bx_ - sep, 0), min(bx_ + sep + 1, x1 - x0)
    vol[near_j, ya:yb, xa:xb] = -1
    rj, ry, rx = np.unravel_index(int(np.argmax(vol)), vol.shape)
    rival = (int(vol[rj, ry, rx]), int(rj), int(ry) + y0, int(rx) + x0) if vol[rj, ry, rx] >= 0 else None
    return _finish(_result(OK, H), best, rival, H, p, geom, rot)


# ---- G4-G9, word for word ----------------------------------------------------------------------------------------------------------
def reloc_one_brute(grid, geom, ranges, p, smin, smax):
    res = geom[0]
    size = grid.shape[0]
    R, n_rot, sep, sep_rot = p["radius"], p["n_rot"], p["sep"], p["sep_rot"]
    L = MR.field_brute(grid, R)
    rot = rotations(n_rot)
    d = [float(v) for v in np.asarray(ranges, dtype=np.float32)]
    hits = [i for i in range(BEAMS) if smin < d[i] <= smax]
    H = len(hits)
    x0, y0, x1, y1 = clip_box(p.get("box"), size)
    cands = []
    for j in range(n_rot):
        S, C = float(rot[j, 0]), float(rot[j, 1])
        offs = []
        for i in hits:
            bx, by = d[i] * float(MR.CB[i]), d[i] * float(MR.SB[i])
            ex, ey = C * bx - S * by, S * bx + C * by
            offs.append((int(math.floor(ex / res + 0.5)), int(math.floor(ey / res + 0.5))))
        for gy in range(y0, y1):
            for gx in range(x0, x1):
                if grid[gy, gx] != 0:
                    continue
                score = 0
                for ax, ay in offs:
                    cx, cy = gx + ax, gy + ay
                    if 0 <= cx < size and 0 <= cy < size:
                        score += int(L[cy, cx])
                cands.append((score, j, gy, gx))
    if H == 0 or not cands:
        return _result(NO_CANDIDATE, H)
    order = lambda c: (-c[0], c[1], c[2], c[3])
    best = min(cands, key=order)
    far = [c for c in cands if abs(c[3] - best[3]) > sep or abs(c[2] - best[2]) > sep
           or min(abs(c[1] - best[1]), n_rot - abs(c[1] - best[1])) > sep_rot]
    rival = min(far, key=order) if far else None
    return _finish(_result(OK, H), best, rival, H, p, geom, rot)


def reloc(grid, geom, buf, p=None, lengths=None, smin=0.1, smax=1.2, max_agent=2, records=None):
    """Every record of buf (uint8 [n, 743 | 751]) against grid: RELOC_DTYPE [n].  records: restate only these indices."""
    p = params(**(p or {}))
    assert limit_ok(p, smax, geom[0])
    recs = MR.records_of(buf)
    acc, _ = MR.poses_of(recs, lengths, None, None, max_agent)
    L, free, rot = MR.field(grid, p["radius"]), grid == 0, rotations(p["n_rot"])
    out = np.zeros(len(recs), dtype=RELOC_DTYPE)
    for k in (range(len(recs)) if records is None else records):
        r = reloc_one(L, free, geom, recs["ranges"][k], p, smin, smax, rot) if acc[k] else _result(NO_RECORD, rec=0)
        for f in FIELDS:
            out[f][k] = r[f]
    return out


def differing(got, exp):
    """The fields in which two RELOC_DTYPE arrays differ, as text ('' when they are equal; doubles compared as bits)."""
    bad = []
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(exp[f])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if (a != b).any():
            k = int(np.nonzero(a != b)[0][0])
            bad.append(f"{f}[{k}]: {got[f][k]!r} against {exp[f][k]!r} ({int((a != b).sum())} differ)")
    if np.asarray(got["pad"]).any():
        bad.append("pad bytes are not zero")
    return "; ".join(bad)


# ---- the world --------------------------------------------------------------------------------------------------------------------
WORLD_GRID = (192, 0.05, -4.8, -4.8)          # size, res, ox, oy
WORLD_SMIN, WORLD_SMAX = 0.1, 3.0


def world():
    """Three rooms joined by two doorways, with a block, two partitions and a pillar: int8 [192, 192]."""
    size = WORLD_GRID[0]
    g = np.full((size, size), -1, dtype=np.int8)

    def room(x0, y0, x1, y1):
        """The rectangle's border OCCUPIED where it is not already FREE, then its interior FREE."""
        b = np.zeros(g.shape, dtype=bool)
        b[y0, x0:x1 + 1] = b[y1, x0:x1 + 1] = True
        b[y0:y1 + 1, x0] = b[y0:y1 + 1, x1] = True
        g[b & (g != 0)] = 100
        g[y0 + 1:y1, x0 + 1:x1] = 0

    room(20, 24, 121, 99)
    room(121, 40, 171, 83)
    g[55:70, 121] = 0
    room(37, 99, 88, 160)
    g[99, 50:62] = 0
    g[60:75, 45:52] = 100
    g[24:58, 84] = 100
    g[130:133, 60:88] = 100
    g[50:53, 140:143] = 100
    g[72, 150:171] = 100
    return g


def small_world():
    """68 x 68, every cell FREE up to the grid's border but for an L-shaped wall, a bar and two pillars (nothing symmetric)."""
    g = np.zeros((68, 68), dtype=np.int8)
    g[10, 8:40] = 100
    g[10:30, 8] = 100
    g[50, 30:60] = 100
    g[40:44, 20] = 100
    g[25, 50] = g[33, 58] = 100
    return g


def query_poses(grid, geom, n, seed):
    """n poses float32 [n, 3] and their cells int [n, 2] (gx, gy): a uniform FREE cell at least 4 cells (Chebyshev) from every
    OCCUPIED one, a uniform position inside it (0.05 to 0.95 of the cell), a uniform yaw."""
    res, ox, oy = geom
    rng = np.random.default_rng(seed)
    open_cells = np.argwhere((grid == 0) & (MR.field(grid, 3) == 0))
    pick = open_cells[rng.integers(len(open_cells), size=n)]
    fx, fy = rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n)
    pose = np.stack([ox + (pick[:, 1] + fx) * res, oy + (pick[:, 0] + fy) * res, rng.uniform(-math.pi, math.pi, n)], axis=1)
    return pose.astype(np.float32), pick[:, ::-1].copy()


def recovered(r, cell, yaw, n_rot):
    """The found pose lies within one cell on each axis and one rotation step of the truth."""
    step = 2 * math.pi / n_rot
    dy = abs((float(r["yaw"]) - float(yaw) + math.pi) % (2 * math.pi) - math.pi)
    return abs(int(r["gx"]) - int(cell[0])) <= 1 and abs(int(r["gy"]) - int(cell[1])) <= 1 and dy <= step


def paint_rays(grid):
    """Rays (x0, y0, x1, y1, valid) for maze_scenes.paint that draw `grid` into an empty map: per row the runs of FREE cells
    (a free ray frees its cells up to, not including, its end cell), then every OCCUPIED cell as a hit of length 0."""
    size = grid.shape[0]
    rays = []
    for y in range(size):
        free = np.concatenate([[False], grid[y] == 0, [False]])
        edges = np.nonzero(free[1:] != free[:-1])[0]
        for a, b in zip(edges[::2].tolist(), edges[1::2].tolist()):              # FREE cells [a, b)
            if b < size:
                rays.append((a, y, b, y, 0))
            elif a > 0:
                rays.append((size - 1, y, a - 1, y, 0))                             # from the border inwards
            else:
                rays.append((0, y, size - 1, y, 0))
                rays.append((size - 1, y, size - 2, y, 0))
    for y, x in np.argwhere(grid == 100).tolist():
        rays.append((x, y, x, y, 1))
    return np.array(rays, dtype=np.int64).reshape(-1, 5)
