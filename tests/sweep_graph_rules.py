"""NumPy / Python restatement of graph mode of the sweep path (include/quasar_slam.h, "sweeps in the pose graph"): the landmark
signature of a sweep, PoseGraphSLAM.add_pose after oracle/pymapper.py:74-90 generalised to any agent and to the context's
gap, radius and damping, the bots' drift and zone boxes -- and a seeded two-bot room stream that closes loops.
Test infrastructure only: no GPU, no product code."""
import math

import numpy as np

LM_REJECTED = 255
SMIN, SMAX = 0.1, 1.2


# ---- signature -----------------------------------------------------------------------------------------------------------
def sector_values(ranges, half_width=5):
    """(right, front, left) float32 [n]: the element of rank w of each sector's 2w + 1 ranges, unusable ranges (not finite,
    or <= 0) counted as +inf."""
    r = np.asarray(ranges, dtype=np.float32).reshape(-1, 181)
    w = int(half_width)
    out = []
    for first in (0, 90 - w, 180 - 2 * w):
        v = r[:, first:first + 2 * w + 1]
        with np.errstate(invalid="ignore"):
            v = np.where(np.isfinite(v) & (v > 0), v, np.float32(np.inf)).astype(np.float32)
        out.append(np.sort(v, axis=1, kind="stable")[:, w])
    return tuple(out)


def decide(front, left, right, close=0.40, open=0.80):
    """detectLandmark (AgentFirmware_Bot1.ino:152-169) on float64 values."""
    f, l, r = (np.asarray(v, dtype=np.float64) for v in (front, left, right))
    fc, lc, rc = f < close, l < close, r < close
    fo, lo, ro = f > open, l > open, r > open
    lm = np.zeros(f.shape, dtype=np.uint8)
    lm[fo & lo & ro] = 5
    lm[lc & rc & fo] = 3
    lm[fc & rc] = 2
    lm[fc & lc] = 1
    lm[fc & lc & rc] = 4
    return lm


def signature(ranges, half_width=5, close=0.40, open=0.80):
    right, front, left = sector_values(ranges, half_width)
    return decide(front, left, right, close, open)


def accepted(magic_ok, agent, x, y, yaw, lengths, stride, max_agent=2):
    """qs_ingest_sweeps' rule and the packet path's finiteness test: bool [n]."""
    agent = np.asarray(agent, dtype=np.int64)
    ok = np.asarray(magic_ok, dtype=bool) & (agent >= 1) & (agent <= max_agent)
    if lengths is not None:
        ok &= np.asarray(lengths, dtype=np.int64) == stride
    for v in (x, y, yaw):
        ok &= np.isfinite(np.asarray(v, dtype=np.float32))
    return ok


def signatures_of_records(recs, stride, lengths=None, max_agent=2, half_width=5, close=0.40, open=0.80):
    """uint8 [n] of a structured array of sweep records (protocol.PACKET_DTYPE_V0 / _V0_ODO): LM_REJECTED where rejected."""
    ok = accepted(recs["magic"] == b"QSRL", recs["agent"], recs["x"], recs["y"], recs["yaw"], lengths, stride, max_agent)
    lm = signature(recs["ranges"], half_width, close, open)
    return np.where(ok, lm, LM_REJECTED).astype(np.uint8)


# ---- pose graph ------------------------------------------------------------------------------------------------------------
class Graph:
    """PoseGraphSLAM (:261-326) for any agents."""

    def __init__(self, radius=0.60, gap=30, damp=0.5):
        self.radius, self.gap, self.damp = radius, gap, damp
        self.n_nodes = 0
        self.landmarks = []        # (x, y, type, node)
        self.closures = []         # (landmark's node, node, dx, dy)
        self.closure_agents = []
        self.last_closure = {}

    def add_pose(self, x, y, agent, lm):
        idx = self.n_nodes
        self.n_nodes += 1
        if lm == 0:
            return idx, None
        found = None
        if agent not in self.last_closure or idx - self.last_closure[agent] >= self.gap:
            for lx, ly, lt, li in self.landmarks:
                if lt != lm or idx - li < self.gap:
                    continue
                if math.sqrt((x - lx) ** 2 + (y - ly) ** 2) < self.radius:
                    found = ((lx - x) * self.damp, (ly - y) * self.damp)
                    self.closures.append((li, idx, found[0], found[1]))
                    self.closure_agents.append(agent)
                    self.last_closure[agent] = idx
                    break
        self.landmarks.append((x, y, lm, idx))
        return idx, found


def beams(rx, ry, yaw, ranges, smin=SMIN, smax=SMAX):
    """(hx, hy, valid) of the 181 beams by qs_ingest_sweeps' rule, end points from Python's math.cos / math.sin."""
    hx, hy, va = [], [], []
    for i, d in enumerate(np.asarray(ranges, dtype=np.float32).tolist()):
        a = yaw + math.radians(i - 90)
        ok = smin < d <= smax
        L = d if ok else (min(d, smax) if d > smin else smax)
        hx.append(rx + L * math.cos(a))
        hy.append(ry + L * math.sin(a))
        va.append(1 if ok else 0)
    return hx, hy, va


class SweepGraph:
    """The context's state that graph mode moves: pose graphs, drift, zone boxes."""

    def __init__(self, max_agent=2, bots_per_graph=0, separation=0.0, radius=0.60, gap=30, damp=0.5,
                 half_width=5, close=0.40, open=0.80, smin=SMIN, smax=SMAX):
        self.max_agent = max_agent
        self.bpg = bots_per_graph if bots_per_graph > 0 else max_agent
        self.graphs = [Graph(radius, gap, damp) for _ in range((max_agent + self.bpg - 1) // self.bpg)]
        self.offset = {b: (separation if b == 2 else 0.0) for b in range(1, max_agent + 1)}
        self.drift = {b: [0.0, 0.0] for b in range(1, max_agent + 1)}
        self.zone = {b: None for b in range(1, max_agent + 1)}
        self.sig = dict(half_width=half_width, close=close, open=open)
        self.smin, self.smax = smin, smax

    def _zone_point(self, b, x, y):
        z = self.zone[b]
        self.zone[b] = [x, y, x, y] if z is None else [min(z[0], x), min(z[1], y), max(z[2], x), max(z[3], y)]

    def _node(self, agent, x, y, lm):
        """One accepted record of either kind: (node, rx, ry); the bot's drift moves after it."""
        dr = self.drift[agent]
        rx, ry = (float(x) + self.offset[agent]) + dr[0], float(y) + dr[1]
        node, corr = self.graphs[(agent - 1) // self.bpg].add_pose(rx, ry, agent, int(lm))
        if corr is not None:
            dr[0] += corr[0]
            dr[1] += corr[1]
        return node, rx, ry

    def add_packets(self, agent, x, y, lm, ok=None):
        """42-byte packets (pose graph only): node int64 [n], -1 for a rejected one."""
        out = np.full(len(agent), -1, dtype=np.int64)
        for k in range(len(agent)):
            if ok is None or ok[k]:
                out[k] = self._node(int(agent[k]), np.float32(x[k]), np.float32(y[k]), lm[k])[0]
        return out

    def add_sweeps(self, agent, x, y, yaw, ranges, ok=None, correction=None, zone=True):
        """Sweeps in record order: (node int64 [n], lm uint8 [n], pose float64 [n, 3] the pose each was cast from, NaN for a
        rejected one, chain float64 [n, 2] the (rx, ry) the chain gave).  correction: [n, 3] match corrections (dx, dy, dyaw)
        added to the cast pose only."""
        n = len(agent)
        ranges = np.asarray(ranges, dtype=np.float32).reshape(n, 181)
        lm = signature(ranges, **self.sig)
        node = np.full(n, -1, dtype=np.int64)
        pose = np.full((n, 3), np.nan)
        chain = np.full((n, 2), np.nan)
        for k in range(n):
            if ok is not None and not ok[k]:
                lm[k] = LM_REJECTED
                continue
            a = int(agent[k])
            node[k], rx, ry = self._node(a, np.float32(x[k]), np.float32(y[k]), lm[k])
            chain[k] = rx, ry
            ryaw = float(np.float32(yaw[k]))
            if correction is not None:
                rx, ry, ryaw = rx + correction[k][0], ry + correction[k][1], ryaw + correction[k][2]
            pose[k] = rx, ry, ryaw
            if zone:
                self._zone_point(a, rx, ry)
                hx, hy, va = beams(rx, ry, ryaw, ranges[k], self.smin, self.smax)
                for px, py, v in zip(hx, hy, va):
                    if v:
                        self._zone_point(a, px, py)
        return node, lm, pose, chain


# ---- the room stream ---------------------------------------------------------------------------------------------------------
ROOM_W, ROOM_H, MARGIN, STEP = 3.0, 2.0, 0.3, 0.1


def _walk(points):
    """Poses STEP apart along a polyline: (x, y, yaw) lists; the corner itself belongs to the leg that leaves it."""
    xs, ys, yaws = [], [], []
    for (x0, y0), (x1, y1) in zip(points[:-1], points[1:]):
        L = math.hypot(x1 - x0, y1 - y0)
        m = max(1, int(round(L / STEP)))
        a = math.atan2(y1 - y0, x1 - x0)
        for j in range(m):
            t = j / m
            xs.append(x0 + t * (x1 - x0)); ys.append(y0 + t * (y1 - y0)); yaws.append(a)
    return xs, ys, yaws


def _ranges(x, y, yaw):
    """Distance from (x, y) to the room's walls along the 181 beams."""
    a = yaw + np.radians(np.arange(181) - 90.0)
    c, s = np.cos(a), np.sin(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(c > 0, (ROOM_W - x) / c, np.where(c < 0, -x / c, np.inf))
        ty = np.where(s > 0, (ROOM_H - y) / s, np.where(s < 0, -y / s, np.inf))
    return np.minimum(tx, ty)


def room_stream(seed=5, laps=3, drift_per_step=0.001):
    """Two bots in a ROOM_W x ROOM_H room, MARGIN from the walls, bot 1 counter-clockwise and bot 2 clockwise, each lap
    followed by a diagonal detour to the centre and back; poses STEP apart, records interleaved.  Ranges by ray / wall
    intersection with the reference generator's noise model (sigma 0.01 m, 6 % spurious readings from U(0.02, 2.5)); the
    reported pose drifts slowly, with opposite sign per bot.  Returns agent uint8 [n], x, y, yaw float32 [n], ranges float32
    [n, 181]."""
    rng = np.random.default_rng(seed)
    lo_x, lo_y, hi_x, hi_y = MARGIN, MARGIN, ROOM_W - MARGIN, ROOM_H - MARGIN
    centre = (ROOM_W / 2, ROOM_H / 2)
    ccw = [(lo_x, lo_y), (hi_x, lo_y), (hi_x, hi_y), (lo_x, hi_y), (lo_x, lo_y), centre, (lo_x, lo_y)]
    cw = [(hi_x, hi_y), (hi_x, lo_y), (lo_x, lo_y), (lo_x, hi_y), (hi_x, hi_y), centre, (hi_x, hi_y)]
    paths = []
    for pts in (ccw, cw):
        xs, ys, yaws = [], [], []
        for _ in range(laps):
            a, b, c = _walk(pts)
            xs += a; ys += b; yaws += c
        paths.append((xs, ys, yaws))
    m = min(len(p[0]) for p in paths)
    agent, X, Y, YAW, R = [], [], [], [], []
    for j in range(m):
        for b, (xs, ys, yaws) in enumerate(paths):
            r = _ranges(xs[j], ys[j], yaws[j]) + rng.normal(0.0, 0.01, 181)
            spur = rng.random(181) < 0.06
            r[spur] = rng.uniform(0.02, 2.5, int(spur.sum()))
            sign = 1.0 if b == 0 else -1.0
            agent.append(b + 1)
            X.append(xs[j] + sign * drift_per_step * j); Y.append(ys[j] - sign * 0.5 * drift_per_step * j); YAW.append(yaws[j])
            R.append(r)
    return (np.array(agent, dtype=np.uint8), np.array(X, dtype=np.float32), np.array(Y, dtype=np.float32),
            np.array(YAW, dtype=np.float32), np.array(R, dtype=np.float32))
