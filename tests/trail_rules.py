"""CPU restatement of the trail-matching rules of include/quasar_slam.h ("trail matching", T1-T8), for the tests.

A trail is the last K 42-byte packets of one bot, held together rigidly by the bot's own odometry; its hit points (four sonars
a packet) are matched against the map as one constellation.  Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed
[gy, gx]).  Everything after the per-record (sin, cos) is exact integer or uncontracted fp64 arithmetic, so with the device's
own rot_out as input the device must equal this bit for bit.

Also here: the seeded trails the recovery and GPU tests drive through the synthetic room of match_rules."""
import math

import numpy as np

from match_rules import DEFAULTS, MAX_REACH, ROOM_GRID, field, room_poses, room_segments, room_session, world_to_grid

MAX_RECORDS = 64
TRAVEL = 4.0
MIN_DIST, MAX_DIST = 0.05, 1.20              # the reference's trust filter (dual_bot_mapper.py:57-58)
PACKET_DTYPE = np.dtype([("magic", "S4"), ("agent", "u1"), ("x", "<f4"), ("y", "<f4"), ("yaw", "<f4"), ("enc", "<i4"),
                         ("v2v", "<u4"), ("dist", "<f4", (4,)), ("lm", "u1")])
TRAIL_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("it", "<i4"), ("score", "<i4"), ("score0", "<i4"), ("hits", "<i4"),
                        ("records", "<i4"), ("anchor", "<i4"), ("agent", "u1"), ("accepted_match", "u1"), ("pad", "u1", (6,)),
                        ("ax", "<f8"), ("ay", "<f8"), ("dx", "<f8"), ("dy", "<f8"), ("dyaw", "<f8")])
FIELDS = ("ix", "iy", "it", "score", "score0", "hits", "records", "anchor", "agent", "accepted_match", "ax", "ay", "dx", "dy", "dyaw")
assert PACKET_DTYPE.itemsize == 42 and TRAIL_DTYPE.itemsize == 80


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def limit_ok(p, max_dist, travel, res):
    """T8's reach."""
    return math.ceil((max_dist + travel) / res) + p["window"] + p["radius"] + 2 <= MAX_REACH


# ---- T2: acceptance -----------------------------------------------------------------------------------------------------------
def parse(buf, lengths=None, max_agent=2):
    """buf: uint8 [n, stride >= 41].  (accepted bool [n], agent, x, y, yaw float64 [n], dist float64 [n, 4]): qs_ingest's rule --
    length 42 or 41 and <= stride, magic, agent in 1..max_agent, x, y, yaw finite.  A rejected record has zeros."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    n, stride = buf.shape
    acc = np.zeros(n, dtype=bool)
    agent = np.zeros(n, dtype=np.int64)
    x, y, yaw = np.zeros(n), np.zeros(n), np.zeros(n)
    dist = np.zeros((n, 4))
    for k in range(n):
        ln = stride if lengths is None else int(lengths[k])
        if ln not in (41, 42) or ln > stride:
            continue
        raw = bytes(buf[k, :41]) + b"\0"                          # (byte 41, the landmark, is never looked at)
        r = np.frombuffer(raw, dtype=PACKET_DTYPE)[0]
        a = int(r["agent"])
        if r["magic"] != b"QSRL" or not 1 <= a <= max_agent:
            continue
        if not (math.isfinite(r["x"]) and math.isfinite(r["y"]) and math.isfinite(r["yaw"])):
            continue
        acc[k], agent[k] = True, a
        x[k], y[k], yaw[k] = float(r["x"]), float(r["y"]), float(r["yaw"])
        dist[k] = r["dist"].astype(np.float64)
    return acc, agent, x, y, yaw, dist


def rot_libm(buf, lengths=None, max_agent=2):
    """[n, 2] (sin, cos) of every accepted record's yaw from libm (zeros for rejected ones): what rot_out holds to within the
    last bit, for records that count."""
    acc, _, _, _, yaw, _ = parse(buf, lengths, max_agent)
    return np.array([[math.sin(v), math.cos(v)] if a else [0.0, 0.0] for a, v in zip(acc, yaw)]).reshape(-1, 2)


# ---- T3-T7: one trail -------------------------------------------------------------------------------------------------------------
def match_one(L, geom, buf, p, travel=TRAVEL, lengths=None, rot=None, min_dist=MIN_DIST, max_dist=MAX_DIST, offset=None,
              drift=None, max_agent=2):
    """One group.  L: the field of the whole grid; geom = (res, ox, oy); buf uint8 [K, stride]; rot: [K, 2] (sin, cos) of the
    records' yaws or None (libm).  Returns (dict of the qs_trail_match fields, rot_out [K, 2])."""
    res, ox, oy = geom
    offset, drift = offset or {}, drift or {}
    R, W, T, step = p["radius"], p["window"], p["angle_steps"], p["angle_step"]
    acc, agent, x, y, yaw, dist = parse(buf, lengths, max_agent)
    K = len(acc)
    rot_out = np.zeros((K, 2))
    zero = dict(ix=0, iy=0, it=0, score=0, score0=0, hits=0, records=0, anchor=-1, agent=0, accepted_match=0,
                ax=0.0, ay=0.0, dx=0.0, dy=0.0, dyaw=0.0)
    if not acc.any():
        return zero, rot_out
    anchor = int(np.nonzero(acc)[0][-1])                           # T2: the last accepted record
    bot = int(agent[anchor])
    ddx, ddy = drift.get(bot, (0.0, 0.0))
    off = offset.get(bot, 0.0)
    rx = [(float(x[k]) + off) + ddx for k in range(K)]             # T3: ONE offset, ONE drift
    ry = [float(y[k]) + ddy for k in range(K)]
    ax, ay = rx[anchor], ry[anchor]
    t2 = travel * travel
    counts = []
    for k in range(K):                                             # T4
        ex, ey = rx[k] - ax, ry[k] - ay
        counts.append(bool(acc[k]) and int(agent[k]) == bot and ex * ex + ey * ey <= t2)
    if not any(counts):
        return zero, rot_out
    qx, qy = [], []
    for k in range(K):                                             # T5
        if not counts[k]:
            continue
        s, c = (math.sin(yaw[k]), math.cos(yaw[k])) if rot is None else (float(rot[k, 0]), float(rot[k, 1]))
        rot_out[k] = (s, c)
        for j, (ux, uy) in enumerate(((c, s), (-s, c), (-c, -s), (s, -c))):
            d = float(dist[k, j])
            if min_dist < d <= max_dist:
                px, py = rx[k] + d * ux, ry[k] + d * uy
                qx.append(px - ax); qy.append(py - ay)
    qx, qy = np.array(qx, dtype=np.float64), np.array(qy, dtype=np.float64)
    H = len(qx)
    size = L.shape[0]
    Lp = np.pad(L.astype(np.int32), 2 * W) if W else L.astype(np.int32)
    sh = np.arange(-W, W + 1)
    scores = np.zeros((2 * T + 1, 2 * W + 1, 2 * W + 1), dtype=np.int64)          # [it, iy, ix]
    for ti in range(2 * T + 1):                                    # T6
        th = (ti - T) * step
        S, C = math.sin(th), math.cos(th)
        with np.errstate(invalid="ignore", over="ignore"):
            ex = ax + (C * qx - S * qy)
            ey = ay + (S * qx + C * qy)
        cx, okx = world_to_grid(ex, ox, res)
        cy, oky = world_to_grid(ey, oy, res)
        # a cell more than W outside the grid (beyond 2^30 included) scores 0 under every shift
        use = okx & oky & (cx >= -W) & (cx < size + W) & (cy >= -W) & (cy < size + W)
        if not use.any():
            continue
        cx, cy = cx[use] + 2 * W, cy[use] + 2 * W
        scores[ti] = Lp[cy[:, None, None] + sh[None, :, None], cx[:, None, None] + sh[None, None, :]].sum(axis=0)
    it, iy, ix = np.meshgrid(np.arange(-T, T + 1), sh, sh, indexing="ij")
    sc, it, iy, ix = scores.ravel(), it.ravel(), iy.ravel(), ix.ravel()
    # T7 = sweep-matching rule 4: highest score; then smallest ix^2 + iy^2, smallest |it|, smaller it, smaller iy, smaller ix
    b = np.lexsort((ix, iy, it, np.abs(it), ix * ix + iy * iy, -sc))[0]
    best = int(sc[b])
    ok = H >= p["min_hits"] and best * 100 >= p["min_percent"] * H * (R + 1)
    return dict(ix=int(ix[b]), iy=int(iy[b]), it=int(it[b]), score=best, score0=int(scores[T, W, W]), hits=H,
                records=int(sum(counts)), anchor=anchor, agent=bot, accepted_match=int(ok), ax=ax, ay=ay,
                dx=float(ix[b]) * res if ok else 0.0, dy=float(iy[b]) * res if ok else 0.0,
                dyaw=float(it[b]) * step if ok else 0.0), rot_out


def match(grid, geom, buf, gsize, p=None, travel=TRAVEL, lengths=None, rot=None, min_dist=MIN_DIST, max_dist=MAX_DIST,
          offset=None, drift=None, max_agent=2):
    """Every group of buf (uint8 [n, stride], runs of gsize[g]) against grid: (TRAIL_DTYPE [n_groups], rot_out [n, 2])."""
    p = params(**(p or {}))
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    gsize = [int(g) for g in gsize]
    assert all(1 <= g <= MAX_RECORDS for g in gsize) and sum(gsize) == len(buf)
    L = field(grid, p["radius"])
    out = np.zeros(len(gsize), dtype=TRAIL_DTYPE)
    rot_out = np.zeros((len(buf), 2))
    k0 = 0
    for g, K in enumerate(gsize):
        r, ro = match_one(L, geom, buf[k0:k0 + K], p, travel, None if lengths is None else lengths[k0:k0 + K],
                          None if rot is None else rot[k0:k0 + K], min_dist, max_dist, offset, drift, max_agent)
        for f, v in r.items():
            out[f][g] = v
        rot_out[k0:k0 + K] = ro
        k0 += K
    return out, rot_out


def move(m, x, y, yaw):
    """T7's transform of a pose by the correction of match m (a dict or record with ax, ay, dx, dy, dyaw)."""
    ax, ay, dx, dy, dyaw = (float(m[k]) for k in ("ax", "ay", "dx", "dy", "dyaw"))
    S, C = math.sin(dyaw), math.cos(dyaw)
    return ax + (C * (x - ax) - S * (y - ay)) + dx, ay + (S * (x - ax) + C * (y - ay)) + dy, yaw + dyaw


def pack(agent, x, y, yaw, dist4, lm=0):
    """uint8 [n, 42] packets from arrays (this file's own packer: the tests do not depend on the package's)."""
    n = len(x)
    rec = np.zeros(n, dtype=PACKET_DTYPE)
    rec["magic"] = b"QSRL"
    rec["agent"], rec["x"], rec["y"], rec["yaw"] = agent, x, y, yaw
    rec["dist"] = np.asarray(dist4, dtype=np.float32).reshape(n, 4)
    rec["lm"] = lm
    return rec.view(np.uint8).reshape(n, 42)


# ---- seeded trails in the synthetic room -----------------------------------------------------------------------------------------
def room_map_session():
    """The 30 mapping sweeps of match_rules' room that the trail tests share (their poses and ranges: room_session's keys)."""
    return room_session(seed=11, n_map=30, n_query=1, window=0, angle_steps=0)


def _clear(seg, x, y, margin):
    a, b = seg[:, :2], seg[:, 2:]
    ab = b - a
    tt = np.clip(((np.array([x, y]) - a) * ab).sum(1) / (ab * ab).sum(1), 0, 1)
    dist = np.hypot(*(a + tt[:, None] * ab - np.array([x, y])).T)
    inside_box = 0.725 <= x <= 1.525 and -0.875 <= y <= -0.175
    inside_room = -3.075 <= x <= 2.925 and -2.275 <= y <= 2.525
    return dist.min() >= margin and inside_room and not inside_box


def cast4(segments, pose, rng=None, sigma=0.0, far=3.0):
    """Ranges float32 [4] (front, left, back, right) of a packet at pose, cast as match_rules.cast casts its 181 beams: the
    nearest intersection of each beam with the segments, noise, beyond `far` or nothing: 0 (no echo)."""
    x, y, yaw = pose
    ang = yaw + np.array([0.0, math.pi / 2, math.pi, -math.pi / 2])
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
        d = d + rng.normal(0.0, sigma, 4)
    return np.where(d <= far, d, 0.0).astype(np.float32)


def room_trail(rng, K, seg, step=0.05, max_rate=0.08, margin=0.15):
    """True poses [K, 3] of one drive through the room: steps of `step` metres along the heading, a constant yaw rate within
    +-max_rate rad per step, every pose at least `margin` from a wall."""
    while True:
        x, y, yaw = room_poses(rng, 1)[0]
        rate = rng.uniform(-max_rate, max_rate)
        out = []
        for _ in range(K):
            if not _clear(seg, x, y, margin):
                break
            out.append((x, y, yaw))
            x, y, yaw = x + step * math.cos(yaw), y + step * math.sin(yaw), yaw + rate
        if len(out) == K:
            return np.array(out)


def displaced(true, disp, res=ROOM_GRID[1], angle_step=math.pi / 180):
    """The poses [K, 3] of one trail displaced rigidly about its last pose by disp = (ix, iy cells, it angle steps), rounded to
    f32 as a packet carries them."""
    th = int(disp[2]) * angle_step
    S, C = math.sin(th), math.cos(th)
    a = true[-1]
    qx, qy = true[:, 0] - a[0], true[:, 1] - a[1]
    pose = np.stack([a[0] + (C * qx - S * qy) + int(disp[0]) * res, a[1] + (S * qx + C * qy) + int(disp[1]) * res,
                     true[:, 2] + th], axis=1)
    return pose.astype(np.float32).astype(np.float64)


def room_trails(seed, n, K, window, angle_steps, angle_step=math.pi / 180, sigma=0.01, far=3.0, agent=1):
    """n seeded trails of K packets in the room.  Each trail's reported poses are its true poses displaced RIGIDLY about its
    last pose: turned by whole angle steps (|.| <= angle_steps), shifted by whole cells (|.| <= window), then rounded to f32
    as the packet carries them.  Returns dict(true [n, K, 3], pose [n, K, 3], ranges [n, K, 4], disp int [n, 3] (ix, iy, it),
    pkts uint8 [n * K, 42], gsize)."""
    rng = np.random.default_rng(seed)
    seg = room_segments()
    res = ROOM_GRID[1]
    true = np.stack([room_trail(rng, K, seg) for _ in range(n)])
    ranges = np.stack([[cast4(seg, p, rng, sigma, far) for p in tr] for tr in true])
    disp = np.stack([rng.integers(-window, window + 1, n), rng.integers(-window, window + 1, n),
                     rng.integers(-angle_steps, angle_steps + 1, n)], axis=1)
    pose = np.stack([displaced(true[i], disp[i], res, angle_step) for i in range(n)])
    flat = pose.reshape(-1, 3)
    pkts = pack(np.full(n * K, agent), flat[:, 0], flat[:, 1], flat[:, 2], ranges.reshape(-1, 4))
    return dict(true=true, pose=pose, ranges=ranges, disp=disp, pkts=pkts, gsize=np.full(n, K, dtype=np.int32))


def recovered(m, disp):
    """The returned candidate cancels the displacement to within one cell on each axis and one angle step."""
    return (abs(int(m["ix"]) + int(disp[0])) <= 1 and abs(int(m["iy"]) + int(disp[1])) <= 1
            and abs(int(m["it"]) + int(disp[2])) <= 1)
