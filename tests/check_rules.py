"""CPU restatement of the sweep-check rules V1-V9 of include/quasar_slam.h ("sweep check") and of the guarded ingest's withheld
set, for the tests.

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]: -1 UNKNOWN, 0 FREE, 100 OCCUPIED), which is the stamp
reading of the device (0 = UNKNOWN, odd = OCCUPIED, anything else FREE).  Everything after the one (sin, cos) of a record's yaw is
exact integer or uncontracted fp64 arithmetic, so with the device's own pair as input the device must equal this bit for bit; the
pair defaults to libm's.  Two forms: `check_one`, the 181 walks in lock step as NumPy arrays, and `check_one_brute`, word for word."""
import math

import numpy as np

import match_rules as MR
import plan_rules as R
import sense_rules as SR

BEAMS = 181
AGREE, NEARER, FARTHER, MISSED, UNSEEN, NO_RECORD_BEAM = 0, 1, 2, 3, 4, 255
OK, NO_RECORD, UNDECIDED, CONTRADICTS = 0, 1, 2, 3
MAX_CELLS = SR.MAX_CELLS
CHECK_DTYPE = np.dtype([("agree", "<i4"), ("nearer", "<i4"), ("farther", "<i4"), ("missed", "<i4"), ("unseen", "<i4"),
                        ("checked", "<i4"), ("bad", "<i4"), ("status", "<i4"), ("accepted_record", "u1"), ("pad", "u1", (7,)),
                        ("sin_yaw", "<f8"), ("cos_yaw", "<f8")])
FIELDS = ("agree", "nearer", "farther", "missed", "unseen", "checked", "bad", "status", "accepted_record", "sin_yaw", "cos_yaw")


def params(res, **kw):
    """V8's defaults for a grid of resolution res."""
    p = dict(tol=2.0 * res, min_checked=20, max_bad_percent=30, count_missed=0, reserved=0)
    p.update(kw)
    return p


def limit_ok(p, smax, res):
    """V8: True when the call is valid."""
    return (math.isfinite(p["tol"]) and p["tol"] >= 0 and 0 <= p["min_checked"] <= BEAMS and 0 <= p["max_bad_percent"] <= 100
            and p["count_missed"] in (0, 1) and p.get("reserved", 0) == 0 and math.ceil(smax / res) + 1 <= MAX_CELLS)


def patch_radius(smax, res):
    return math.ceil(smax / res) + 1


def classify(kind, p_, ret, d, smin, smax, tol):
    """V6.  kind: 'hit', 'clear' or 'unknown'; p_: the prediction's distance; ret: d is a return."""
    if kind == "hit":
        if ret:
            return NEARER if d < p_ - tol else (FARTHER if d > p_ + tol else AGREE)
        return MISSED if (smin + tol < p_ and p_ <= smax - tol) else UNSEEN
    if kind == "unknown":
        return NEARER if (ret and d < p_ - tol) else UNSEEN
    return NEARER if ret else AGREE


def start_cells(pose, geom):
    """V2: (x0, y0) or None when the pose is not usable."""
    res, ox, oy = geom
    rx, ry, yaw = (float(v) for v in pose)
    if not (math.isfinite(rx) and math.isfinite(ry) and math.isfinite(yaw)):
        return None
    x0, y0 = SR.cell(rx, ox, res), SR.cell(ry, oy, res)
    return None if x0 is None or y0 is None else (x0, y0)


def summary(cls, p, sn, cs):
    """V7 of the 181 classes of an accepted record."""
    n = [int((cls == c).sum()) for c in range(5)]
    assert sum(n) == BEAMS
    checked = n[AGREE] + n[NEARER] + n[FARTHER] + n[MISSED]
    bad = n[NEARER] + n[FARTHER] + (n[MISSED] if p["count_missed"] else 0)
    status = UNDECIDED if checked < p["min_checked"] else (CONTRADICTS if bad * 100 > p["max_bad_percent"] * checked else OK)
    return dict(agree=n[AGREE], nearer=n[NEARER], farther=n[FARTHER], missed=n[MISSED], unseen=n[UNSEEN], checked=checked, bad=bad,
                status=status, accepted_record=1, sin_yaw=sn, cos_yaw=cs)


# ---- V3-V6, word for word ---------------------------------------------------------------------------------------------------------
def check_one_brute(grid, geom, pose, ranges, p, smin, smax, sincos=None):
    """One accepted sweep: (dict of the qs_sweep_check fields, classes uint8 [181])."""
    res, ox, oy = geom
    size = grid.shape[0]
    rx, ry, yaw = (float(v) for v in pose)
    cls = np.full(BEAMS, UNSEEN, dtype=np.uint8)
    start = start_cells(pose, geom)
    if start is None:
        return summary(cls, p, 0.0, 0.0), cls
    sn, cs = (math.sin(yaw), math.cos(yaw)) if sincos is None else (float(sincos[0]), float(sincos[1]))
    C = patch_radius(smax, res)
    x0, y0 = start
    for i in range(BEAMS):
        ci = cs * float(MR.CB[i]) - sn * float(MR.SB[i])
        si = sn * float(MR.CB[i]) + cs * float(MR.SB[i])
        x1, y1 = SR.cell(rx + smax * ci, ox, res), SR.cell(ry + smax * si, oy, res)
        if x1 is None or y1 is None or abs(x1 - x0) > C or abs(y1 - y0) > C:
            continue
        kind, at = "clear", None
        for x, y in R.bresenham(x0, y0, x1, y1)[1:]:
            v = int(grid[y, x]) if 0 <= x < size and 0 <= y < size else -1
            if v != 0:
                kind, at = ("hit" if v == 100 else "unknown"), (x, y)
                break
        p_ = 0.0
        if at is not None:
            dx, dy = at[0] - x0, at[1] - y0
            p_ = res * math.sqrt(float(dx * dx + dy * dy))
        d = float(np.float32(ranges[i]))
        cls[i] = classify(kind, p_, smin < d <= smax, d, smin, smax, p["tol"])
    return summary(cls, p, sn, cs), cls


# ---- V3-V6, the 181 walks in lock step -----------------------------------------------------------------------------------------------
def _cells(w, o, res):
    """SR.cell over an array: (cell int64, exists)."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = (w - o) / res
        ok = np.abs(q) < 9.0e15
    c = np.trunc(np.where(ok, q, 0.0)).astype(np.int64)
    return np.clip(c, -SR.CLAMP, SR.CLAMP), ok


def check_one(grid, geom, pose, ranges, p, smin, smax, sincos=None):
    """As check_one_brute."""
    res, ox, oy = geom
    size = grid.shape[0]
    rx, ry, yaw = (float(v) for v in pose)
    cls = np.full(BEAMS, UNSEEN, dtype=np.uint8)
    start = start_cells(pose, geom)
    if start is None:
        return summary(cls, p, 0.0, 0.0), cls
    sn, cs = (math.sin(yaw), math.cos(yaw)) if sincos is None else (float(sincos[0]), float(sincos[1]))
    C = patch_radius(smax, res)
    x0, y0 = start
    ci, si = cs * MR.CB - sn * MR.SB, sn * MR.CB + cs * MR.SB
    x1, okx = _cells(rx + smax * ci, ox, res)
    y1, oky = _cells(ry + smax * si, oy, res)
    walks = okx & oky & (np.abs(x1 - x0) <= C) & (np.abs(y1 - y0) <= C)
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    sx, sy = np.where(x0 < x1, 1, -1), np.where(y0 < y1, 1, -1)
    x, y, err = np.full(BEAMS, x0, dtype=np.int64), np.full(BEAMS, y0, dtype=np.int64), dx - dy
    stopped = np.zeros(BEAMS, dtype=bool)
    val = np.zeros(BEAMS, dtype=np.int64)                                   # the cell a stopped walk ended on
    while True:
        act = walks & ~stopped & ((x != x1) | (y != y1))
        if not act.any():
            break
        e2 = 2 * err
        mx, my = act & (e2 > -dy), act & (e2 < dx)
        err = err - np.where(mx, dy, 0) + np.where(my, dx, 0)
        x, y = x + np.where(mx, sx, 0), y + np.where(my, sy, 0)
        inside = (x >= 0) & (x < size) & (y >= 0) & (y < size)
        v = np.where(inside, grid[np.clip(y, 0, size - 1), np.clip(x, 0, size - 1)], -1).astype(np.int64)
        new = act & (v != 0)
        val = np.where(new, v, val)
        stopped |= new
    hx, hy = x - x0, y - y0
    pd = res * np.sqrt((hx * hx + hy * hy).astype(np.float64))
    d = np.asarray(ranges, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ret = (smin < d) & (d <= smax)
    for i in np.nonzero(walks)[0]:
        kind = ("hit" if val[i] == 100 else "unknown") if stopped[i] else "clear"
        cls[i] = classify(kind, float(pd[i]), bool(ret[i]), float(d[i]), smin, smax, p["tol"])
    return summary(cls, p, sn, cs), cls


def check(grid, geom, buf, p=None, lengths=None, smin=0.1, smax=1.2, sincos=None, offset=None, drift=None, max_agent=2, one=check_one,
          records=None):
    """Every record of buf (uint8 [n, 743 | 751]) against grid: (CHECK_DTYPE [n], classes uint8 [n, 181]).  sincos: [n, 2] the
    (sin, cos) of each record's yaw, or None (libm); records: restate only these indices (the others are left NO_RECORD)."""
    p = params(geom[0], **(p or {}))
    assert limit_ok(p, smax, geom[0])
    recs = MR.records_of(buf)
    acc, pose = MR.poses_of(recs, lengths, offset, drift, max_agent)
    out = np.zeros(len(recs), dtype=CHECK_DTYPE)
    out["status"] = NO_RECORD
    cls = np.full((len(recs), BEAMS), NO_RECORD_BEAM, dtype=np.uint8)
    for k in (np.nonzero(acc)[0] if records is None else records):
        if not acc[k]:
            continue
        r, cls[k] = one(grid, geom, pose[k], recs["ranges"][k], p, smin, smax, None if sincos is None else sincos[k])
        for f, v in r.items():
            out[f][k] = v
    return out, cls


def withheld(checks):
    """The guarded ingest's withheld set: bool [n]."""
    return np.asarray(checks["status"]) == CONTRADICTS


def break_magic(buf, mask):
    """A copy of buf in which the records of mask are no longer accepted: what a plain ingest must be given to map what the
    guarded ingest maps."""
    out = np.array(buf, copy=True)
    out[np.asarray(mask, dtype=bool), 0] ^= 0xFF
    return out


# ---- V6's table on a grid where p is exact in f32 ------------------------------------------------------------------------------------
TABLE_GRID = (64, 0.25, -8.0, -8.0)              # size, res, ox, oy
TABLE_POSE = (-8.0 + 10.5 * 0.25, -8.0 + 32.5 * 0.25, 0.0)      # the centre of cell (10, 32), heading +x: beam 90 walks row 32
TABLE_BEAM, TABLE_P = 90, 2.0                    # ... and meets cell (18, 32), 8 cells on: p = 2.0


def table_grid(kind):
    """All FREE but cell (18, 32): OCCUPIED ('hit'), UNKNOWN ('unknown') or FREE as well ('clear')."""
    g = np.zeros((TABLE_GRID[0], TABLE_GRID[0]), dtype=np.int8)
    g[32, 18] = dict(hit=100, unknown=-1, clear=0)[kind]
    return g


def table_cases():
    """(grid kind, f32 range of beam 90, smin, smax, the class V6 gives it): every cell of the table at equality and one f32 step to
    either side, with tol = 0."""
    f = np.float32
    up = lambda v: float(np.nextafter(f(v), f(np.inf)))
    dn = lambda v: float(np.nextafter(f(v), f(0)))
    p = TABLE_P
    return [
        ("hit", dn(p), 0.02, 4.0, NEARER), ("hit", p, 0.02, 4.0, AGREE), ("hit", up(p), 0.02, 4.0, FARTHER),
        ("hit", 0.0, dn(p), 4.0, MISSED), ("hit", 0.0, p, 4.0, UNSEEN), ("hit", 0.0, up(p), 4.0, UNSEEN),
        ("hit", 0.0, 0.02, dn(p), UNSEEN), ("hit", 0.0, 0.02, p, MISSED), ("hit", 0.0, 0.02, up(p), MISSED),
        ("hit", up(4.0), 0.02, 4.0, MISSED), ("hit", float("nan"), 0.02, 4.0, MISSED),
        ("clear", dn(4.0), 0.25, 4.0, NEARER), ("clear", 4.0, 0.25, 4.0, NEARER), ("clear", up(4.0), 0.25, 4.0, AGREE),
        ("clear", dn(0.25), 0.25, 4.0, AGREE), ("clear", 0.25, 0.25, 4.0, AGREE), ("clear", up(0.25), 0.25, 4.0, NEARER),
        ("unknown", dn(p), 0.02, 4.0, NEARER), ("unknown", p, 0.02, 4.0, UNSEEN), ("unknown", up(p), 0.02, 4.0, UNSEEN),
        ("unknown", 0.0, 0.02, 4.0, UNSEEN),
    ]


def differing(got, exp):
    """The fields in which two CHECK_DTYPE arrays differ, as text ('' when they are equal; doubles compared as bits)."""
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
