"""CPU restatement of the rules K1-K8 of include/quasar_slam.h ("trail relocalisation"), for the tests: a trail of 42-byte
packets (trail_rules.parse: K2) whose hit points about the anchor (K3, K4, here) are located over the whole map as a group of
sweeps is (reloc_group_rules.group_one: K5-K7).

Everything after the per-record (sin, cos) is exact integer or uncontracted fp64 arithmetic, so with the device's own rot_out as
input the device must equal this bit for bit.  Two forms: `reloc_one`, vectorised, and `reloc_one_brute`, word for word, for
small grids.

Also here: the seeded trails the recovery and GPU tests drive through a grid world, reported in a frame of the bot's own."""
import math

import numpy as np

import match_rules as MR
import reloc_group_rules as GR
import reloc_rules as RR
import trail_rules as TR

MAX_RECORDS = TR.MAX_RECORDS
OK, NO_RECORD, NO_CANDIDATE = RR.OK, RR.NO_RECORD, RR.NO_CANDIDATE
TRAIL_RELOC_DTYPE = np.dtype([("gx", "<i4"), ("gy", "<i4"), ("j", "<i4"), ("score", "<i4"), ("hits", "<i4"),
                              ("gx2", "<i4"), ("gy2", "<i4"), ("j2", "<i4"), ("score2", "<i4"), ("status", "<i4"),
                              ("records", "u1"), ("accepted", "u1"), ("agent", "u1"), ("pad", "u1"), ("anchor", "<i4"),
                              ("x", "<f8"), ("y", "<f8"), ("yaw", "<f8"), ("ax", "<f8"), ("ay", "<f8")])
FIELDS = ("gx", "gy", "j", "score", "hits", "gx2", "gy2", "j2", "score2", "status", "records", "accepted", "agent", "anchor",
          "x", "y", "yaw", "ax", "ay")
assert TRAIL_RELOC_DTYPE.itemsize == 88


# ---- K1, K8 -------------------------------------------------------------------------------------------------------------------
def groups_ok(n, gsize):
    gsize = [int(g) for g in gsize]
    return all(1 <= g <= MAX_RECORDS for g in gsize) and sum(gsize) == n


def reach_cells(max_dist, travel, res):
    """M of K5."""
    return math.ceil((max_dist + travel) / res) + 1


def limit_ok(p, max_dist, travel, res):
    return GR.limit_ok(p, max_dist, travel, res)


# ---- K2-K4 --------------------------------------------------------------------------------------------------------------------
def points(buf, travel=TR.TRAVEL, lengths=None, rot=None, min_dist=TR.MIN_DIST, max_dist=TR.MAX_DIST, max_agent=2):
    """One trail, buf uint8 [K, stride]: (head, qx float64 [H], qy, rot_out [K, 2]); head = dict(records, anchor, agent, ax, ay).
    rot: [K, 2] (sin, cos) of the records' yaws or None (libm)."""
    acc, agent, x, y, yaw, dist = TR.parse(buf, lengths, max_agent)
    K = len(acc)
    rot_out = np.zeros((K, 2))
    head = dict(records=0, anchor=-1, agent=0, ax=0.0, ay=0.0)
    if not acc.any():
        return head, np.zeros(0), np.zeros(0), rot_out
    anchor = int(np.nonzero(acc)[0][-1])                           # K2: the last accepted record
    bot = int(agent[anchor])
    ax, ay = float(x[anchor]), float(y[anchor])                    # (parse widened the f32 fields)
    t2 = travel * travel
    qx, qy, records = [], [], 0
    for k in range(K):
        ex, ey = float(x[k]) - ax, float(y[k]) - ay
        if not (bool(acc[k]) and int(agent[k]) == bot and ex * ex + ey * ey <= t2):      # K3
            continue
        records += 1
        s, c = (math.sin(yaw[k]), math.cos(yaw[k])) if rot is None else (float(rot[k, 0]), float(rot[k, 1]))
        rot_out[k] = (s, c)
        for j, (ux, uy) in enumerate(((c, s), (-s, c), (-c, -s), (s, -c))):              # K4
            d = float(dist[k, j])
            if min_dist < d <= max_dist:
                qx.append(ex + d * ux); qy.append(ey + d * uy)
    head.update(records=records, anchor=anchor, agent=bot, ax=ax, ay=ay)
    return head, np.array(qx, dtype=np.float64), np.array(qy, dtype=np.float64), rot_out


def _complete(r, head):
    """The trail's own fields on a group result (K7)."""
    r = dict(r)
    r.update(agent=0, anchor=-1, ax=0.0, ay=0.0)
    if r["status"] != NO_RECORD:
        r.update(agent=head["agent"], anchor=head["anchor"], ax=head["ax"], ay=head["ay"])
    return r


# ---- K5-K7, vectorised ----------------------------------------------------------------------------------------------------------
def reloc_one(L, free, geom, buf, p, travel=TR.TRAVEL, lengths=None, rot_in=None, min_dist=TR.MIN_DIST, max_dist=TR.MAX_DIST,
              max_agent=2, rot=None):
    """One trail.  L: the field of the whole grid (MR.field(grid, radius)); free: grid == 0.  Returns (dict of the
    qs_trail_reloc fields, rot_out [K, 2])."""
    head, qx, qy, rot_out = points(buf, travel, lengths, rot_in, min_dist, max_dist, max_agent)
    M = reach_cells(max_dist, travel, geom[0])
    r = GR.group_one(L, free, geom, head["records"], qx, qy, p, M, rot)
    return _complete(r, head), rot_out


# ---- K3-K7, word for word ----------------------------------------------------------------------------------------------------------
def reloc_one_brute(grid, geom, buf, p, travel=TR.TRAVEL, lengths=None, rot_in=None, min_dist=TR.MIN_DIST, max_dist=TR.MAX_DIST,
                    max_agent=2):
    res, ox, oy = geom
    size = grid.shape[0]
    R, n_rot, sep, sep_rot = p["radius"], p["n_rot"], p["sep"], p["sep_rot"]
    acc, agent, x, y, yaw, dist = TR.parse(buf, lengths, max_agent)
    zero = dict.fromkeys(FIELDS, 0)
    zero.update(status=NO_RECORD, anchor=-1, x=0.0, y=0.0, yaw=0.0, ax=0.0, ay=0.0)
    anchor = -1
    for k in range(len(acc)):
        if acc[k]:
            anchor = k
    if anchor < 0:
        return zero
    bot = int(agent[anchor])
    ax, ay = float(x[anchor]), float(y[anchor])
    pts, records = [], 0
    for k in range(len(acc)):
        ex, ey = float(x[k]) - ax, float(y[k]) - ay
        if not acc[k] or int(agent[k]) != bot or not ex * ex + ey * ey <= travel * travel:
            continue
        records += 1
        s, c = (math.sin(yaw[k]), math.cos(yaw[k])) if rot_in is None else (float(rot_in[k, 0]), float(rot_in[k, 1]))
        dirs = ((c, s), (-s, c), (-c, -s), (s, -c))
        for j in range(4):
            d = float(dist[k, j])
            if min_dist < d <= max_dist:
                pts.append((ex + d * dirs[j][0], ey + d * dirs[j][1]))
    H = len(pts)
    M = math.ceil((max_dist + travel) / res) + 1
    Lf = MR.field_brute(grid, R)
    rots = RR.rotations(n_rot)
    x0, y0, x1, y1 = RR.clip_box(p.get("box"), size)
    cands = []
    for j in range(n_rot):
        S, C = float(rots[j, 0]), float(rots[j, 1])
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
                        score += int(Lf[cy, cx])
                cands.append((score, j, gy, gx))
    r = dict(zero)
    r.update(status=NO_CANDIDATE, records=records, hits=H, agent=bot, anchor=anchor, ax=ax, ay=ay,
             gx=-1, gy=-1, j=-1, gx2=-1, gy2=-1, j2=-1)
    if H == 0 or not cands:
        return r
    order = lambda c: (-c[0], c[1], c[2], c[3])
    best = min(cands, key=order)
    far = [c for c in cands if abs(c[3] - best[3]) > sep or abs(c[2] - best[2]) > sep
           or min(abs(c[1] - best[1]), n_rot - abs(c[1] - best[1])) > sep_rot]
    rival = min(far, key=order) if far else None
    r.update(status=OK, score=best[0], j=best[1], gy=best[2], gx=best[3])
    if rival is not None:
        r.update(score2=rival[0], j2=rival[1], gy2=rival[2], gx2=rival[3])
    full = H * (R + 1)
    r["accepted"] = int(H >= p["min_hits"] and r["score"] * 100 >= p["min_percent"] * full
                        and (r["score"] - r["score2"]) * 100 >= p["min_margin"] * full)
    r["x"], r["y"] = ox + (float(r["gx"]) + 0.5) * res, oy + (float(r["gy"]) + 0.5) * res
    r["yaw"] = float(rots[r["j"], 2])
    return r


def reloc_trails(grid, geom, buf, gsize, p=None, travel=TR.TRAVEL, lengths=None, rot=None, min_dist=TR.MIN_DIST,
                 max_dist=TR.MAX_DIST, max_agent=2, groups=None):
    """Every trail of buf (uint8 [n, stride], runs of gsize[g]) against grid: (TRAIL_RELOC_DTYPE [n_groups], rot_out [n, 2]).
    rot: the device's rot_out or None (libm).  groups: restate only these group indices."""
    p = RR.params(**(p or {}))
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    assert limit_ok(p, max_dist, travel, geom[0]) and groups_ok(len(buf), gsize)
    L, free, rots = MR.field(grid, p["radius"]), grid == 0, RR.rotations(p["n_rot"])
    ends = np.cumsum(np.asarray(gsize, dtype=np.int64))
    out = np.zeros(len(gsize), dtype=TRAIL_RELOC_DTYPE)
    rot_out = np.zeros((len(buf), 2))
    for g in (range(len(gsize)) if groups is None else groups):
        a, b = int(ends[g]) - int(gsize[g]), int(ends[g])
        r, ro = reloc_one(L, free, geom, buf[a:b], p, travel, None if lengths is None else lengths[a:b],
                          None if rot is None else rot[a:b], min_dist, max_dist, max_agent, rots)
        for f in FIELDS:
            out[f][g] = r[f]
        rot_out[a:b] = ro
    return out, rot_out


def differing(got, exp):
    """The fields in which two TRAIL_RELOC_DTYPE arrays differ, as text ('' when they are equal; doubles compared as bits)."""
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


def move(r, x, y, yaw):
    """K7's transform of a pose in the packet fields' frame by result r (a dict or record with x, y, yaw, ax, ay)."""
    fx, fy, fyaw, ax, ay = (float(r[k]) for k in ("x", "y", "yaw", "ax", "ay"))
    S, C = math.sin(fyaw), math.cos(fyaw)
    return fx + (C * (x - ax) - S * (y - ay)), fy + (S * (x - ax) + C * (y - ay)), yaw + fyaw


# ---- seeded trails through a grid world ---------------------------------------------------------------------------------------------
def cast4(grid, geom, pose, far, rng=None, sigma=0.0):
    """Ranges float32 [4] (front, left, back, right) at pose: along each beam the distance at which it enters the first OCCUPIED
    cell (sampled every eighth of a cell), noise; beyond `far`, or off the grid: 0 (no echo)."""
    res, ox, oy = geom
    size = grid.shape[0]
    x, y, yaw = (float(v) for v in pose)
    t = np.arange(0.0, far + res, res / 8)
    out = np.zeros(4)
    for j, a in enumerate((yaw, yaw + math.pi / 2, yaw + math.pi, yaw - math.pi / 2)):
        gx = np.floor((x + t * math.cos(a) - ox) / res).astype(np.int64)
        gy = np.floor((y + t * math.sin(a) - oy) / res).astype(np.int64)
        inside = (gx >= 0) & (gx < size) & (gy >= 0) & (gy < size)
        occ = np.zeros(len(t), dtype=bool)
        occ[inside] = grid[gy[inside], gx[inside]] == 100
        stop = occ | ~inside
        if stop.any():
            k = int(np.argmax(stop))
            if occ[k]:
                out[j] = t[k]
    if rng is not None and sigma > 0:
        out = np.where(out > 0, out + rng.normal(0.0, sigma, 4), 0.0)
    return np.where((out > 0) & (out <= far), out, 0.0).astype(np.float32)


def drive(grid, geom, rng, K, step=0.05, max_rate=0.04):
    """True poses float64 [K, 3] of one drive: from a uniform open cell (FREE, at least 4 cells from every OCCUPIED one) steps of
    `step` metres along the heading with a constant yaw rate within +-max_rate rad a step, through open cells only."""
    res, ox, oy = geom
    size = grid.shape[0]
    is_open = (grid == 0) & (MR.field(grid, 3) == 0)
    cells = np.argwhere(is_open)
    while True:
        gy, gx = cells[rng.integers(len(cells))]
        x, y = ox + (gx + rng.uniform(0.05, 0.95)) * res, oy + (gy + rng.uniform(0.05, 0.95)) * res
        yaw, rate = rng.uniform(-math.pi, math.pi), rng.uniform(-max_rate, max_rate)
        out = []
        for _ in range(K):
            cx, cy = int(math.floor((x - ox) / res)), int(math.floor((y - oy) / res))
            if not (0 <= cx < size and 0 <= cy < size and is_open[cy, cx]):
                break
            out.append((x, y, yaw))
            x, y, yaw = x + step * math.cos(yaw), y + step * math.sin(yaw), yaw + rate
        if len(out) == K:
            return np.array(out)


def reported(true, phi, shift):
    """The poses [K, 3] of a trail in the bot's own frame -- the map's turned by phi about its origin and shifted -- rounded to
    f32 as a packet carries them."""
    S, C = math.sin(phi), math.cos(phi)
    pose = np.stack([C * true[:, 0] - S * true[:, 1] + shift[0], S * true[:, 0] + C * true[:, 1] + shift[1], true[:, 2] + phi], axis=1)
    pose[:, 2] = (pose[:, 2] + math.pi) % (2 * math.pi) - math.pi
    return pose.astype(np.float32).astype(np.float64)


def world_trails(grid, geom, seed, n, K, far, sigma=0.01, agent=1, max_rate=0.04):
    """n seeded trails of K packets through grid: dict(true [n, K, 3], pose [n, K, 3] as reported, phi [n], shift [n, 2],
    ranges [n, K, 4], pkts uint8 [n * K, 42], gsize).  Every trail has a frame of its own: any angle, a shift within +-10 m."""
    rng = np.random.default_rng(seed)
    true = np.stack([drive(grid, geom, rng, K, max_rate=max_rate) for _ in range(n)])
    ranges = np.stack([[cast4(grid, geom, q, far, rng, sigma) for q in tr] for tr in true])
    phi = rng.uniform(-math.pi, math.pi, n)
    shift = rng.uniform(-10.0, 10.0, (n, 2))
    pose = np.stack([reported(true[i], phi[i], shift[i]) for i in range(n)])
    flat = pose.reshape(-1, 3)
    pkts = TR.pack(np.full(n * K, agent), flat[:, 0], flat[:, 1], flat[:, 2], ranges.reshape(-1, 4))
    return dict(true=true, pose=pose, phi=phi, shift=shift, ranges=ranges, pkts=pkts, gsize=np.full(n, K, dtype=np.int32))


def recovered(r, anchor_pose, phi, geom, n_rot):
    """The anchor is found within one cell on each axis of its true cell and the frame's turn within two rotation steps."""
    res, ox, oy = geom
    cx, cy = math.floor((anchor_pose[0] - ox) / res), math.floor((anchor_pose[1] - oy) / res)
    dyaw = abs((float(r["yaw"]) + float(phi) + math.pi) % (2 * math.pi) - math.pi)
    return abs(int(r["gx"]) - cx) <= 1 and abs(int(r["gy"]) - cy) <= 1 and dyaw <= 2 * (2 * math.pi / n_rot)
