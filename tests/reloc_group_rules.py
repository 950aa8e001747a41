"""CPU restatement of the rules J1-J8 of include/quasar_slam.h ("relocalisation of a group"), for the tests: several sweeps of
one bot, each with its pose in the group's frame, located jointly by the rules G1-G9 (tests/reloc_rules.py).

Everything is exact integer or uncontracted fp64 arithmetic, the relative poses are inputs and the rotations' (sin, cos) are
libm's on both sides, so the device must equal this bit for bit.  Two forms: `group_one`, vectorised (per rotation and distinct
point offset one shifted add of the padded field, over the bounding box of the candidates), and `group_one_brute`, word for
word, for small grids.

Also here: the seeded builder of the groups the recovery and GPU tests share -- a bot that turns and drives on from a query
pose of reloc_rules.query_poses."""
import math

import numpy as np

import match_rules as MR
import reloc_rules as RR

MAX_GROUP = 16
OK, NO_RECORD, NO_CANDIDATE = RR.OK, RR.NO_RECORD, RR.NO_CANDIDATE
REL_DTYPE = np.dtype([("tx", "<f8"), ("ty", "<f8"), ("s", "<f8"), ("c", "<f8")])
GROUP_DTYPE = np.dtype([("gx", "<i4"), ("gy", "<i4"), ("j", "<i4"), ("score", "<i4"), ("hits", "<i4"),
                        ("gx2", "<i4"), ("gy2", "<i4"), ("j2", "<i4"), ("score2", "<i4"), ("status", "<i4"),
                        ("records", "u1"), ("accepted", "u1"), ("pad", "u1", (6,)),
                        ("x", "<f8"), ("y", "<f8"), ("yaw", "<f8")])
FIELDS = ("gx", "gy", "j", "score", "hits", "gx2", "gy2", "j2", "score2", "status", "records", "accepted", "x", "y", "yaw")
IDENTITY = np.array([(0.0, 0.0, 0.0, 1.0)], dtype=REL_DTYPE)


# ---- J1, J8 -------------------------------------------------------------------------------------------------------------------
def groups_ok(n, gsize):
    gsize = [int(g) for g in gsize]
    return all(1 <= g <= MAX_GROUP for g in gsize) and sum(gsize) == n


def reach_cells(smax, travel, res):
    """M of J5."""
    return math.ceil((smax + travel) / res) + 1


def limit_ok(p, smax, travel, res):
    return (math.isfinite(travel) and travel >= 0 and 0 <= p["radius"] <= MR.MAX_RADIUS and 1 <= p["n_rot"] <= RR.MAX_ROT
            and 0 <= p["sep"] <= RR.MAX_SEP and 0 <= p["sep_rot"] < p["n_rot"]
            and RR.TILE + 2 * (math.ceil((smax + travel) / res) + p["radius"] + 1) <= 255)


# ---- J2 -----------------------------------------------------------------------------------------------------------------------
def rel_of(x, y, yaw, anchor=0):
    """REL_DTYPE [n] of one group from f32 poses, as protocol.reloc_rel forms them: fp64, libm; (dx, dy) from the anchor turned
    into the anchor's heading, then sin / cos of yaw - yaw0."""
    x, y, yaw = (np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1) for v in (x, y, yaw))
    out = np.zeros(len(x), dtype=REL_DTYPE)
    if len(x) == 0:
        return out
    c0, s0 = math.cos(float(yaw[anchor])), math.sin(float(yaw[anchor]))
    for k in range(len(x)):
        dx, dy = float(x[k]) - float(x[anchor]), float(y[k]) - float(y[anchor])
        d = float(yaw[k]) - float(yaw[anchor])
        out[k] = (c0 * dx + s0 * dy, c0 * dy - s0 * dx, math.sin(d), math.cos(d))
    return out


# ---- J3, J4 -------------------------------------------------------------------------------------------------------------------
def counts(acc, rel, travel):
    """J3 for one record: G3 accepts it (acc), its rel values are finite, it lies within travel of the frame."""
    tx, ty, s, c = (float(rel[f]) for f in ("tx", "ty", "s", "c"))
    return bool(acc) and all(math.isfinite(v) for v in (tx, ty, s, c)) and tx * tx + ty * ty <= travel * travel


def points(ranges, rel, acc, travel, smin, smax):
    """(records, px float64 [H], py) of one group: ranges float32 [k, 181], rel REL_DTYPE [k], acc bool [k]."""
    records, px, py = 0, [], []
    for k in range(len(ranges)):
        if not counts(acc[k], rel[k], travel):
            continue
        records += 1
        d = np.asarray(ranges[k], dtype=np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            hit = (smin < d) & (d <= smax)
        bx, by = d[hit] * MR.CB[hit], d[hit] * MR.SB[hit]
        tx, ty, s, c = (float(rel[k][f]) for f in ("tx", "ty", "s", "c"))
        with np.errstate(over="ignore", invalid="ignore"):
            px.append(tx + (c * bx - s * by))
            py.append(ty + (s * bx + c * by))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0)
    return records, cat(px), cat(py)


def point_offsets(px, py, rot, res, M):
    """J5: (ax int64 [n_rot, H], ay, reach bool [n_rot, H]); a point out of reach (or not a number) scores 0."""
    S, C = rot[:, 0][:, None], rot[:, 1][:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        ex = C * px[None, :] - S * py[None, :]
        ey = S * px[None, :] + C * py[None, :]
        fx, fy = np.floor(ex / res + 0.5), np.floor(ey / res + 0.5)
        reach = (fx >= -M) & (fx <= M) & (fy >= -M) & (fy <= M)
    return np.where(reach, fx, 0).astype(np.int64), np.where(reach, fy, 0).astype(np.int64), reach


def _result(status, H=0, records=0):
    r = dict.fromkeys(FIELDS, 0)
    r.update(status=status, records=records, hits=H, x=0.0, y=0.0, yaw=0.0)
    if status != NO_RECORD:
        r.update(gx=-1, gy=-1, j=-1, gx2=-1, gy2=-1, j2=-1)
    return r


# ---- J5-J7, vectorised ------------------------------------------------------------------------------------------------------------
def group_one(L, free, geom, records, px, py, p, M, rot=None):
    """One group from its points.  L: the field of the whole grid (MR.field(grid, radius)); free: grid == 0."""
    if records == 0:
        return _result(NO_RECORD)
    res = geom[0]
    size = L.shape[0]
    n_rot, sep, sep_rot = p["n_rot"], p["sep"], p["sep_rot"]
    if rot is None:
        rot = RR.rotations(n_rot)
    H = len(px)
    x0, y0, x1, y1 = RR.clip_box(p.get("box"), size)
    if H == 0 or x1 <= x0 or y1 <= y0 or not free[y0:y1, x0:x1].any():
        return _result(NO_CANDIDATE, H, records)
    ys, xs = np.nonzero(free[y0:y1, x0:x1])                       # the bounding box of the candidates: the order is kept
    y0, y1, x0, x1 = y0 + int(ys.min()), y0 + int(ys.max()) + 1, x0 + int(xs.min()), x0 + int(xs.max()) + 1
    ax, ay, reach = point_offsets(px, py, rot, res, M)
    Lp = np.pad(L.astype(np.int16), M)
    cand = free[y0:y1, x0:x1]
    vol = np.empty((n_rot, y1 - y0, x1 - x0), dtype=np.int16)     # score (at most 16 * 181 * 8 = 23 168), -1 where no candidate
    for j in range(n_rot):
        acc = np.zeros((y1 - y0, x1 - x0), dtype=np.int16)
        if reach[j].any():
            off, cnt = np.unique(np.stack([ay[j][reach[j]], ax[j][reach[j]]], axis=1), axis=0, return_counts=True)
            for (oy_, ox_), c in zip(off.tolist(), cnt.tolist()):
                sl = Lp[y0 + M + oy_:y1 + M + oy_, x0 + M + ox_:x1 + M + ox_]
                acc += sl if c == 1 else sl * np.int16(c)
        vol[j] = np.where(cand, acc, -1)
    bj, by_, bx_ = np.unravel_index(int(np.argmax(vol)), vol.shape)
    best = (int(vol[bj, by_, bx_]), int(bj), int(by_) + y0, int(bx_) + x0)
    dj = np.abs(np.arange(n_rot) - bj)
    near_j = np.nonzero(np.minimum(dj, n_rot - dj) <= sep_rot)[0]
    ya, yb = max(by_ - sep, 0), min(by_ + sep + 1, y1 - y0)
    xa, xb = max(bx_ - sep, 0), min(bx_ + sep + 1, x1 - x0)
    vol[near_j, ya:yb, xa:xb] = -1
    rj, ry, rx = np.unravel_index(int(np.argmax(vol)), vol.shape)
    rival = (int(vol[rj, ry, rx]), int(rj), int(ry) + y0, int(rx) + x0) if vol[rj, ry, rx] >= 0 else None
    return RR._finish(_result(OK, H, records), best, rival, H, p, geom, rot)


# ---- J3-J7, word for word ----------------------------------------------------------------------------------------------------------
def group_one_brute(grid, geom, ranges, rel, acc, travel, p, smin, smax):
    res = geom[0]
    size = grid.shape[0]
    R, n_rot, sep, sep_rot = p["radius"], p["n_rot"], p["sep"], p["sep_rot"]
    M = reach_cells(smax, travel, res)
    L = MR.field_brute(grid, R)
    rot = RR.rotations(n_rot)
    records, pts = 0, []
    for k in range(len(ranges)):
        tx, ty, s, c = (float(rel[k][f]) for f in ("tx", "ty", "s", "c"))
        if not (acc[k] and all(math.isfinite(v) for v in (tx, ty, s, c)) and tx * tx + ty * ty <= travel * travel):
            continue
        records += 1
        d = [float(v) for v in np.asarray(ranges[k], dtype=np.float32)]
        for i in range(RR.BEAMS):
            if smin < d[i] <= smax:
                bx, by = d[i] * float(MR.CB[i]), d[i] * float(MR.SB[i])
                pts.append((tx + (c * bx - s * by), ty + (s * bx + c * by)))
    if records == 0:
        return _result(NO_RECORD)
    H = len(pts)
    x0, y0, x1, y1 = RR.clip_box(p.get("box"), size)
    cands = []
    for j in range(n_rot):
        S, C = float(rot[j, 0]), float(rot[j, 1])
        offs = []
        for qx, qy in pts:
            ex, ey = C * qx - S * qy, S * qx + C * qy
            qa, qb = ex / res + 0.5, ey / res + 0.5
            if not (math.isfinite(qa) and math.isfinite(qb)):
                continue
            a, b = math.floor(qa), math.floor(qb)
            if abs(a) <= M and abs(b) <= M:
                offs.append((a, b))
        for gy in range(y0, y1):
            for gx in range(x0, x1):
                if grid[gy, gx] != 0:
                    continue
                score = 0
                for a, b in offs:
                    cx, cy = gx + a, gy + b
                    if 0 <= cx < size and 0 <= cy < size:
                        score += int(L[cy, cx])
                cands.append((score, j, gy, gx))
    if H == 0 or not cands:
        return _result(NO_CANDIDATE, H, records)
    order = lambda c: (-c[0], c[1], c[2], c[3])
    best = min(cands, key=order)
    far = [c for c in cands if abs(c[3] - best[3]) > sep or abs(c[2] - best[2]) > sep
           or min(abs(c[1] - best[1]), n_rot - abs(c[1] - best[1])) > sep_rot]
    rival = min(far, key=order) if far else None
    return RR._finish(_result(OK, H, records), best, rival, H, p, geom, rot)


def reloc_groups(grid, geom, buf, gsize, rel=None, travel=2.0, p=None, lengths=None, smin=0.1, smax=1.2, max_agent=2, groups=None):
    """The records of buf (uint8 [n, 743 | 751]) in runs of gsize[g] against grid: GROUP_DTYPE [n_groups].  rel None: from the
    packets' poses, a group's first record its frame.  groups: restate only these group indices."""
    p = RR.params(**(p or {}))
    assert limit_ok(p, smax, travel, geom[0]) and groups_ok(len(buf), gsize)
    recs = MR.records_of(buf)
    acc, _ = MR.poses_of(recs, lengths, None, None, max_agent)
    ends = np.cumsum(np.asarray(gsize, dtype=np.int64))
    if rel is None:
        rel = np.concatenate([rel_of(recs["x"][e - g:e], recs["y"][e - g:e], recs["yaw"][e - g:e]) for g, e in zip(gsize, ends)]
                             + [np.zeros(0, dtype=REL_DTYPE)])
    L, free, rot = MR.field(grid, p["radius"]), grid == 0, RR.rotations(p["n_rot"])
    M = reach_cells(smax, travel, geom[0])
    out = np.zeros(len(gsize), dtype=GROUP_DTYPE)
    for g in (range(len(gsize)) if groups is None else groups):
        a, b = int(ends[g]) - int(gsize[g]), int(ends[g])
        records, px, py = points(recs["ranges"][a:b], rel[a:b], acc[a:b], travel, smin, smax)
        r = group_one(L, free, geom, records, px, py, p, M, rot)
        for f in FIELDS:
            out[f][g] = r[f]
    return out


def differing(got, exp):
    """The fields in which two GROUP_DTYPE arrays differ, as text ('' when they are equal; doubles compared as bits)."""
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


# ---- the groups of the recovery and GPU tests -------------------------------------------------------------------------------------
def build_groups(grid, geom, poses, K, step, seed, turn=1.0, tries=40):
    """poses float32 [n, 3] -> float32 [n, K, 3]: from each pose the bot K - 1 times turns by a uniform angle within +-turn
    radians and drives `step` metres straight ahead, through open cells only (FREE and at least 4 cells from every OCCUPIED one,
    sampled every half cell of the way).  A turn whose way is not open is drawn again, after `tries` draws from the full circle;
    a bot that finds no way at all turns on the spot.  The first pose of a group is the query pose: its cell is the truth."""
    res, ox, oy = geom
    rng = np.random.default_rng(seed)
    is_open = (grid == 0) & (MR.field(grid, 3) == 0)
    size = grid.shape[0]

    def way_open(x, y, yaw):
        for t in np.arange(0.0, step + 0.25 * res, 0.5 * res):
            gx, gy = int(math.floor((x + t * math.cos(yaw) - ox) / res)), int(math.floor((y + t * math.sin(yaw) - oy) / res))
            if not (0 <= gx < size and 0 <= gy < size and is_open[gy, gx]):
                return False
        return True

    out = np.zeros((len(poses), K, 3), dtype=np.float32)
    for n, pose in enumerate(np.asarray(poses, dtype=np.float32)):
        x, y, yaw = (float(v) for v in pose)
        out[n, 0] = (x, y, yaw)
        for k in range(1, K):
            for t in range(2 * tries):
                cand = yaw + rng.uniform(-turn, turn) if t < tries else rng.uniform(-math.pi, math.pi)
                if way_open(x, y, cand):
                    yaw = cand
                    x, y = x + step * math.cos(yaw), y + step * math.sin(yaw)
                    break
            else:
                yaw = yaw + rng.uniform(-turn, turn)
            yaw = (yaw + math.pi) % (2 * math.pi) - math.pi
            x, y, yaw = (float(v) for v in np.array([x, y, yaw], dtype=np.float32))
            out[n, k] = (x, y, yaw)
    return out
