"""Seeded walks over one used context: an op table (writers that change the map or the settings, queries of every family at
small and large sizes), a model of the context built from the CPU restatements (oracle/, tests/*_rules.py), and a generator
of op lists.  Plain Python and numpy: no GPU is imported here, `run` takes a QuasarMapper from whoever has one.

An op list is a list of (name, args) with args a dict of ints, floats, strings, tuples and None: it prints as a literal that
can be pasted into a directed test.  Everything an op needs beyond that (poses, bots, clouds) is drawn from
numpy.random.default_rng over the seed in its args.

  op.run(m, args, env)          -> the context's answer (arrays, dicts of them, Refused)
  op.expect(model, args, got)   -> the same structure from the model; a writer also moves the model.  `got` hands over what a
                                   restatement takes from the device by design: the sweeps the device sensed (inputs, not
                                   answers), the rotations of a match and the (sin, cos) of a check (match_rules.py,
                                   check_rules.py); None on a model-only walk, which then senses and rotates with libm.
  differing(got, want)          -> '' or the first difference as text; numbers as ==, doubles as bits"""
import importlib
import math

import numpy as np

import assign_rules as AR
import check_rules as CR
import gain_rules as GR
import match_rules as MR
import maze_scenes as MZ
import merge_rules as MG
import plan_rules as PR
import reloc_group_rules as RG
import reloc_rules as RR
import sense_rules as SR
import sweep_graph_rules as SG
import territory_rules as TR
import view_rules as VR
from conftest import PKG_NAME
from oracle import oracle as orc

RES = 0.05
NEAR = (0.1, 1.2)               # the sweep filter of a new context
NO_RETURN = 9.0                 # what a sensed beam without a hit reports: finite, beyond every filter
GRAPH_PARAMS = dict(half_width=5, close=1e-6, open=1e9)       # no sensed sweep has a landmark signature: graph mode adds nodes only
MATCH_PARAMS = dict(window=3, angle_steps=3)
VOXEL = 0.05


def protocol():
    return importlib.import_module(PKG_NAME + ".protocol")


# ---- lifted from the GPU tests (which import them from here) ---------------------------------------------------------------------
def sweep_beams(recs, offset=None, drift=None, smin=0.1, smax=1.2, max_agent=2):
    """(rx, ry, hx, hy, valid) of every beam of every acceptable record, in order -- the reference's arithmetic in Python."""
    offset = offset or {}
    drift = drift or {}
    out = ([], [], [], [], [])
    for r in recs:
        a_id = int(r["agent"])
        if r["magic"] != b"QSRL" or not 1 <= a_id <= max_agent:
            continue
        dx, dy = drift.get(a_id, (0.0, 0.0))
        px = float(r["x"]) + offset.get(a_id, 0.0) + dx
        py = float(r["y"]) + dy
        yaw = float(r["yaw"])
        for i, d in enumerate(r["ranges"].tolist()):
            a = yaw + math.radians(i - 90)
            ok = smin < d <= smax
            L = d if ok else (min(d, smax) if d > smin else smax)
            out[0].append(px); out[1].append(py)
            out[2].append(px + L * math.cos(a)); out[3].append(py + L * math.sin(a))
            out[4].append(1 if ok else 0)
    return [np.array(v, dtype=np.float64) for v in out[:4]] + [np.array(out[4], dtype=np.uint8)]


def corrected(pose, acc, mt):
    """The poses a matched ingest casts from: each accepted record's pose plus its match's correction."""
    out = pose.copy()
    out[:, 0] = pose[:, 0] + mt["dx"]
    out[:, 1] = pose[:, 1] + mt["dy"]
    out[:, 2] = pose[:, 2] + mt["dyaw"]
    return out[acc]


def greedy(cents, bots, sep):
    """dual_bot_mapper.py:958-992 restated: bots in order; skip taken centroids and those within `sep` of an earlier
    target; the smallest sqrt distance by strict `<` from inf wins (ties: lowest index)."""
    targets, out = [], []
    for bx, by in bots:
        best, bi = math.inf, -1
        for i, (cx, cy) in enumerate(cents):
            if any(i == ti or math.sqrt((cx - tx) * (cx - tx) + (cy - ty) * (cy - ty)) < sep for ti, tx, ty in targets):
                continue
            d = math.sqrt((bx - cx) * (bx - cx) + (by - cy) * (by - cy))
            if d < best:
                best, bi = d, i
        out.append(bi)
        if bi >= 0:
            targets.append((bi, cents[bi][0], cents[bi][1]))
    return out


# ---- the world -----------------------------------------------------------------------------------------------------------------------
def geometry(size):
    """(size, res, ox, oy): the grid centred on the world's origin."""
    return size, RES, -size * RES / 2, -size * RES / 2


def world(size):
    """int8 [size, size]: a walled room with a doorway into UNKNOWN space, an inner bar, a pillar, an UNKNOWN slit and a few
    single UNKNOWN holes, so that frontiers exist.  136: the room spans three 64-cell planner tiles both ways; 68: two."""
    g = np.full((size, size), -1, dtype=np.int8)
    a, b = size // 17, size - 1 - size // 17                 # 8 .. 127, 4 .. 63
    g[a, a:b + 1] = g[b, a:b + 1] = 100
    g[a:b + 1, a] = g[a:b + 1, b] = 100
    g[a + 1:b, a + 1:b] = 0
    g[a, size // 3:size // 3 + size // 12] = 0                 # the doorway: FREE cells beside the UNKNOWN outside
    g[size * 7 // 16:size * 7 // 16 + 3, size // 4:size * 2 // 3] = 100       # the bar
    q = size * 11 // 16
    g[q:q + 4, q:q + 4] = 100                                  # the pillar
    g[size // 4, size // 2:size // 2 + 6] = -1                 # the slit
    for x, y in ((size // 4, size // 4), (size * 3 // 4, size // 3), (size // 3, size * 3 // 4)):
        g[y, x] = -1
    return g


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def open_cells(size):
    """[n, 2] (gy, gx): the world's FREE cells at least 3 cells (Chebyshev) from every OCCUPIED one."""
    w = cached(("world", size), lambda: world(size))
    return cached(("open", size), lambda: np.argwhere((w == 0) & (MR.field(w, 2) == 0)))


def rng_of(args, tag=0):
    return np.random.default_rng([int(args["seed"]), tag])


def draw_poses(size, n, rng):
    """float32 [n, 3]: a uniform open cell of the world, a uniform position inside it, a uniform yaw."""
    _, res, ox, oy = geometry(size)
    pick = open_cells(size)[rng.integers(len(open_cells(size)), size=n)]
    fx, fy = rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n)
    return np.stack([ox + (pick[:, 1] + fx) * res, oy + (pick[:, 0] + fy) * res, rng.uniform(-math.pi, math.pi, n)], axis=1).astype(np.float32)


def draw_points(size, n, rng, odd=True):
    """float64 [n, 2] world positions in the world's open cells; with odd and n >= 3 one is NaN and one lies off the grid."""
    p = draw_poses(size, n, rng)[:, :2].astype(np.float64)
    if odd and n >= 3:
        p[n // 2] = (math.nan, 0.0)
        p[n - 1] = (1e3, -1e3)
    return p


# ---- comparing answers ----------------------------------------------------------------------------------------------------------------
class Refused:
    """A documented refusal (QuasarError, ValueError); equal to any other refusal."""

    def __init__(self, text=""):
        self.text = str(text)

    def __repr__(self):
        return f"Refused({self.text[:80]!r})"


def differing(got, want, path="answer"):
    """'' when the two answers are the same, else where they first differ."""
    if isinstance(want, Refused) or isinstance(got, Refused):
        return "" if isinstance(want, Refused) and isinstance(got, Refused) else f"{path}: {got!r} against {want!r}"
    if isinstance(want, dict):
        if not isinstance(got, dict) or sorted(got) != sorted(want):
            return f"{path}: keys {sorted(got) if isinstance(got, dict) else type(got)} against {sorted(want)}"
        for k in sorted(want):
            why = differing(got[k], want[k], f"{path}[{k!r}]")
            if why:
                return why
        return ""
    if isinstance(want, (list, tuple)):
        if not isinstance(got, (list, tuple)) or len(got) != len(want):
            return f"{path}: {len(got) if isinstance(got, (list, tuple)) else type(got)} items against {len(want)}"
        for i, (a, b) in enumerate(zip(got, want)):
            why = differing(a, b, f"{path}[{i}]")
            if why:
                return why
        return ""
    if want is None or got is None:
        return "" if want is None and got is None else f"{path}: {got!r} against {want!r}"
    a, b = np.asarray(got), np.asarray(want)
    if a.shape != b.shape:
        return f"{path}: shape {a.shape} against {b.shape}"
    if a.dtype.names or b.dtype.names:
        if a.dtype != b.dtype:
            return f"{path}: dtype {a.dtype} against {b.dtype}"
        for f in a.dtype.names:
            why = differing(a[f], b[f], f"{path}.{f}")
            if why:
                return why
        return "" if a.tobytes() == b.tobytes() else f"{path}: padding bytes differ"
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        if a.dtype != b.dtype:
            return f"{path}: dtype {a.dtype} against {b.dtype}"
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        a, b = np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u)
    elif a.dtype.kind in "iub" and b.dtype.kind in "iub":
        a, b = a.astype(np.int64), b.astype(np.int64)
    bad = a != b
    if np.any(bad):
        k = tuple(np.argwhere(bad)[0].tolist()) if a.ndim else ()
        return f"{path}{list(k)}: {np.asarray(got)[k]!r} against {np.asarray(want)[k]!r} ({int(np.sum(bad))} of {a.size} differ)"
    return ""


def refusing(call, errors):
    try:
        return call()
    except errors as e:
        return Refused(e)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
class Model:
    """What a context must show: an orc.OracleMapper for the map and its counters, the settings (sweep filter, graph mode, dirty
    tracking), the number of pose-graph nodes, the merge session (merge_rules.Session over the oracle's grid_to_pcd,
    voxel_downsample and rasterise and the registration given: the oracle's icp_planar by default) and what the last ingest was."""

    def __init__(self, size, register=None):
        self.size = size
        self.geom = geometry(size)[1:]
        self.world = cached(("world", size), lambda: world(size))
        self.filt = NEAR
        self.graph_on = False
        self.tracking = False
        self.session = MG.Session(orc.grid_to_pcd, register or orc.icp_planar, orc.voxel_downsample, orc.rasterise)
        self.merges = 0
        self._new_map()

    def _new_map(self):
        self.o = orc.OracleMapper(*geometry(self.size), 0.0)
        self.graph_sweeps = 0            # accepted sweeps that became pose-graph nodes
        self.unfused = False
        self.last = None                 # None, ("packets", acc, pose), ("sweeps", form, graph, dict of arrays)
        self._grid = None

    @property
    def grid(self):
        if self._grid is None:
            self._grid = np.array(self.o.grid, dtype=np.int8)
        return self._grid

    def wrote(self):
        self._grid = None
        self.unfused = True

    def reset(self):
        self._new_map()

    def restored(self):
        self.last = None

    def nodes(self):
        return int(self.o.n_nodes(0)) + self.graph_sweeps

    def drift(self):
        return {b: tuple(float(v) for v in self.o.drift(b)) for b in (1, 2)}


class Env:
    """What run() needs beyond the mapper: the package (QuasarError), torch where an op takes device buffers, the grid's size."""

    def __init__(self, size, pkg=None, torch=None):
        self.size, self.pkg, self.torch = size, pkg, torch
        self.filt, self.merges = NEAR, 0
        self.errors = (ValueError,) + ((pkg.QuasarError,) if pkg is not None else ())


def sweep_inputs(size, args):
    """(poses float32 [n, 3], agent uint8 [n], odometry) of a sweep-taking op from its args (n, seed, stride)."""
    rng = rng_of(args, 1)
    n = int(args["n"])
    poses = draw_poses(size, n, rng)
    agent = (np.arange(n) % 2 + 1).astype(np.uint8)
    if n >= 16:
        agent[5] = 9                     # a record no context accepts
    return poses, agent, int(args.get("stride", 751)) == 751


def displaced(buf, args):
    """The records with every third one reporting a pose up to 0.3 m and 0.1 rad from where it was sensed: what a match corrects
    and a check may contradict."""
    rng = rng_of(args, 13)
    rec = MR.records_of(buf)
    for k in range(2, len(rec), 3):
        rec["x"][k] += np.float32(rng.uniform(-0.3, 0.3))
        rec["y"][k] += np.float32(rng.uniform(-0.3, 0.3))
        rec["yaw"][k] += np.float32(rng.uniform(-0.1, 0.1))
    return buf


def device_sweeps(m, size, args, smax):
    poses, agent, odo = sweep_inputs(size, args)
    return displaced(m.sense_sweeps(poses, agent, odometry=odo, max_range=smax, noise_amp=0.01, seed=int(args["seed"]), no_return=NO_RETURN), args)


def model_sweeps(model, args, got):
    """The op's sweeps: the device's when it sensed them (they are the op's input), else restated from the model's map."""
    if got is not None and not isinstance(got, Refused):
        return got["buf"]
    poses, agent, odo = sweep_inputs(model.size, args)
    return displaced(SR.sense_sweeps(protocol(), model.grid, *model.geom, poses, agent, odometry=odo, max_range=model.filt[1], noise_amp=0.01,
                                     seed=int(args["seed"]), no_return=NO_RETURN), args)


def aux(got, key):
    return None if got is None or isinstance(got, Refused) else got[key]


# ---- ops ------------------------------------------------------------------------------------------------------------------------------
class Op:
    """name; kind: 'writer' or 'query'; pred: the kind of writer it counts as before a query ('packets', 'sweeps', 'rays', 'reset',
    'restore', or None for a settings writer); sets: {size class: [argument sets]} ('S', 'L'; '-' for an op without sizes);
    twin: whether a restored twin context must answer it the same (merge, last-ingest and refusal ops are outside checkpoints)."""

    def __init__(self, name, kind, sets, run, expect, pred=None, twin=True):
        self.name, self.kind, self.sets, self.run, self.expect, self.pred, self.twin = name, kind, sets, run, expect, pred, twin
        self.sized = sorted(sets) == ["L", "S"]


OPS = {}


def op(name, kind, sets, pred=None, twin=True):
    def deco(cls):
        OPS[name] = Op(name, kind, sets, cls.run, cls.expect, pred, twin)
        return cls
    return deco


# -- writers --
def packets_of(size, args):
    """uint8 [n, 42]: packets from poses in the world's open cells with the four ranges the world gives (restated once per n and
    seed); no landmark, so no closure; from n = 16 on one record carries agent 9."""
    def make():
        rng = rng_of(args, 2)
        n = int(args["n"])
        poses = draw_poses(size, n, rng)
        agent = (np.arange(n) % 2 + 1).astype(np.uint8)
        if n >= 16:
            agent[7] = 9
        w = cached(("world", size), lambda: world(size))
        return SR.sense_packets(protocol(), w, *geometry(size)[1:], poses, agent, max_range=1.2, no_return=NO_RETURN)
    return cached(("packets", size, int(args["n"]), int(args["seed"])), make)


@op("ingest_packets", "writer", {"S": [dict(n=1), dict(n=16)], "L": [dict(n=5000)]}, pred="packets")
class _Packets:
    def run(m, args, env):
        m.ingest_array(packets_of(env.size, args))
        return None

    def expect(model, args, got):
        buf = packets_of(model.size, args)
        model.o.feed_stream(buf)
        model.wrote()
        rec = np.ascontiguousarray(buf).view(protocol().PACKET_DTYPE).reshape(-1)
        acc = ((rec["magic"] == b"QSRL") & (rec["agent"] >= 1) & (rec["agent"] <= 2)).astype(np.uint8)
        pose = np.stack([rec["x"].astype(np.float64), rec["y"].astype(np.float64), rec["yaw"].astype(np.float64)], axis=1)
        model.last = ("packets", acc, pose)
        return None


def _sweeps_run(form):
    def run(m, args, env):
        buf = device_sweeps(m, env.size, args, env.filt[1])
        out = dict(buf=buf)
        if form == "match":
            out["rot"] = m.match_sweeps(buf, params=MATCH_PARAMS, rotations=True)[1]
        if form == "check":
            ck = m.check_sweeps(buf)
            out["sincos"] = np.stack([ck["sin_yaw"], ck["cos_yaw"]], axis=1)
        kw = {"match": dict(match=MATCH_PARAMS), "check": dict(check=True)}.get(form, {})
        r = refusing(lambda: m.ingest_sweeps(buf, **kw), env.errors)
        return r if isinstance(r, Refused) else out
    return run


def _sweeps_expect(form):
    def expect(model, args, got):
        if form == "check" and model.graph_on:
            return Refused("graph mode")
        buf = model_sweeps(model, args, got)
        recs = MR.records_of(buf)
        acc, pose = MR.poses_of(recs, None, None, model.drift())
        smin, smax = model.filt
        arrays = {}
        if form == "match":
            mt = MR.match(model.grid, model.geom, buf, MATCH_PARAMS, None, smin, smax, rot=aux(got, "rot"), drift=model.drift())
            arrays["matches"] = mt
            cast = np.full((len(recs), 3), np.nan)
            cast[acc] = corrected(pose, acc, mt)
        else:
            cast = np.where(acc[:, None], pose, np.nan)
        if form == "check":
            ck, _ = CR.check(model.grid, model.geom, buf, None, None, smin, smax, sincos=aux(got, "sincos"), drift=model.drift())
            arrays["checks"] = ck
            acc = acc & ~CR.withheld(ck)
            cast[~acc] = np.nan
        if acc.any():
            model.o.update_rays(*MR.beams_of_all(cast[acc], recs["ranges"][acc], smin, smax))
        arrays["acc"], arrays["pose"] = acc.astype(np.uint8), cast
        if model.graph_on:
            assert not SG.signature(recs["ranges"][acc], **GRAPH_PARAMS).any(), "a sensed sweep with a landmark signature"
            node = np.full(len(recs), -1, dtype=np.int64)
            node[acc] = model.nodes() + np.arange(int(acc.sum()))
            arrays["node"], arrays["lm"] = node, np.where(acc, 0, SG.LM_REJECTED).astype(np.uint8)
            model.graph_sweeps += int(acc.sum())
        model.wrote()
        model.last = ("sweeps", form, model.graph_on, arrays)
        return got if isinstance(got, dict) else ({} if isinstance(got, Refused) else None)
    return expect


_SWEEP_SETS = {"S": [dict(n=1, stride=751), dict(n=3, stride=743)], "L": [dict(n=65, stride=751), dict(n=65, stride=743)]}
for _form in ("plain", "match", "check"):
    OPS["ingest_sweeps_" + _form] = Op("ingest_sweeps_" + _form, "writer", _SWEEP_SETS, _sweeps_run(_form), _sweeps_expect(_form), pred="sweeps")


def rays_of(size, args):
    """The (rx, ry, hx, hy, valid) batches of an update_rays op: 'world' paints the whole world (free runs, then the OCCUPIED
    cells), 'few' casts 7 rays between points of the world."""
    _, res, ox, oy = geometry(size)
    if args["what"] == "world":
        r = cached(("paint", size), lambda: np.asarray(RR.paint_rays(cached(("world", size), lambda: world(size))), dtype=np.int64).reshape(-1, 5))
        return [MZ.world(part, res, ox, oy) for part in (r[r[:, 4] == 0], r[r[:, 4] != 0]) if len(part)]
    rng = rng_of(args, 3)
    a, b = draw_points(size, 7, rng, odd=False), draw_points(size, 7, rng, odd=False)
    return [(a[:, 0], a[:, 1], b[:, 0], b[:, 1], (np.arange(7) % 2).astype(np.uint8))]


@op("update_rays", "writer", {"-": [dict(what="world"), dict(what="few")]}, pred="rays")
class _Rays:
    def run(m, args, env):
        for batch in rays_of(env.size, args):
            m.update_rays(*batch)
        return None

    def expect(model, args, got):
        for batch in rays_of(model.size, args):
            model.o.update_rays(*batch)
        model.wrote()
        model.last = None
        return None


@op("set_sweep_filter", "writer", {"-": [dict(smin=0.1, smax=1.2), dict(smin=0.1, smax=3.0)]})
class _Filter:
    def run(m, args, env):
        m.set_sweep_filter(args["smin"], args["smax"])
        env.filt = (args["smin"], args["smax"])
        return None

    def expect(model, args, got):
        model.filt = (args["smin"], args["smax"])
        return None


@op("set_sweep_graph", "writer", {"-": [dict(on=True), dict(on=False)]})
class _Graph:
    def run(m, args, env):
        m.set_sweep_graph(args["on"], **GRAPH_PARAMS)
        return m.sweep_graph()[0]

    def expect(model, args, got):
        model.graph_on = bool(args["on"])
        return model.graph_on


@op("dirty_tracking", "writer", {"-": [dict(on=True), dict(on=False)]})
class _Dirty:
    def run(m, args, env):
        return refusing(lambda: m.dirty_tracking(args["on"]), env.errors)

    def expect(model, args, got):
        if args["on"] and not model.tracking and model.unfused:
            return Refused("unfused writes")
        model.tracking = bool(args["on"])
        return None


@op("reset", "writer", {"-": [dict()]}, pred="reset")
class _Reset:
    def run(m, args, env):
        m.reset()
        return None

    def expect(model, args, got):
        model.reset()
        return None


@op("restore", "writer", {"-": [dict()]}, pred="restore")
class _Restore:
    def run(m, args, env):
        m.restore(m.checkpoint())
        return None

    def expect(model, args, got):
        model.restored()
        return None


# -- queries --
@op("views", "query", {"-": [dict()]})
class _Views:
    def run(m, args, env):
        h, mi = m.counts()
        return dict(grid=m.grid_i8(), hits=h, misses=mi, logodds=m.logodds())

    def expect(model, args, got):
        return dict(grid=model.grid, hits=np.array(model.o.hits), misses=np.array(model.o.misses), logodds=model.o.logodds())


def _goal(size, args):
    return draw_points(size, 1, rng_of(args, 4), odd=False)[0]


@op("plan_field", "query", {"-": [dict(clearance=0), dict(clearance=2), dict(clearance=16)]})
class _Field:
    def run(m, args, env):
        return dict(traversable=m.traversable(args["clearance"]), field=m.distance_field(_goal(env.size, args), clearance=args["clearance"]))

    def expect(model, args, got):
        t = PR.traversable(model.grid, args["clearance"])
        g = PR.snap(t, tuple(_goal(model.size, args)), *model.geom, 10)
        f = np.full(t.shape, PR.INF, dtype=np.uint32) if g is None else PR.field_scipy(t, g)
        return dict(traversable=t.astype(np.uint8), field=f)


def _pairs(size, args):
    rng = rng_of(args, 5)
    n = int(args["n"])
    return draw_points(size, n, rng), draw_points(size, n, rng, odd=False)


@op("plan_paths", "query", {"S": [dict(n=1, clearance=2), dict(n=1, clearance=16)], "L": [dict(n=64, clearance=0), dict(n=64, clearance=2)]})
class _Paths:
    def run(m, args, env):
        s, g = _pairs(env.size, args)
        r = m.plan_paths(s, g, clearance=args["clearance"], return_paths=True)
        del r["stats"]
        return r

    def expect(model, args, got):
        s, g = _pairs(model.size, args)
        t = PR.traversable(model.grid, args["clearance"])
        graph = PR.move_graph(t)
        n = len(s)
        out = dict(status=np.zeros(n, np.int32), waypoint_cell=np.full((n, 2), -1, np.int32), waypoint=np.full((n, 2), np.nan),
                   cost=np.full(n, PR.INF, np.uint32), path_len=np.zeros(n, np.int64), paths=[])
        for i in range(n):
            w = PR.plan(t, tuple(s[i]), tuple(g[i]), *model.geom, graph=graph)
            out["status"][i] = w["status"]
            if w["status"] == PR.OK:
                out["waypoint_cell"][i], out["waypoint"][i], out["cost"][i], out["path_len"][i] = w["cell"], w["xy"], w["cost"], len(w["path"])
            out["paths"].append(np.array(w["path"], dtype=np.int32).reshape(-1, 2))
        return out


def centroids_of(model, min_cluster=3):
    cells = orc.frontier_cells(model.grid)
    return orc.cluster_centroids_world(orc.frontier_clusters(cells, model.size, min_cluster), *model.geom)


def _bots(size, args, odd=True):
    return draw_points(size, int(args["bots"]), rng_of(args, 6), odd=odd)


@op("frontier", "query", {"S": [dict(bots=1), dict(bots=0)], "L": [dict(bots=14)]})
class _Frontier:
    def run(m, args, env):
        idx, xy = m.frontier_targets(_bots(env.size, args, odd=False))
        return dict(centroids=np.array(m.frontier_centroids(), dtype=np.float64).reshape(-1, 2), idx=idx, xy=xy)

    def expect(model, args, got):
        cents = centroids_of(model)
        bots = _bots(model.size, args, odd=False)
        idx = np.array(greedy(cents.tolist(), bots.tolist(), protocol().FRONTIER_SEPARATION), dtype=np.int64).reshape(len(bots))
        xy = np.full((len(bots), 2), np.nan)
        xy[idx >= 0] = cents[idx[idx >= 0]]
        return dict(centroids=cents, idx=idx, xy=xy)


_TARGET_KEYS = ("idx", "xy", "cost", "status", "waypoint_cell", "waypoint")
_BOT_SETS = {"S": [dict(bots=1), dict(bots=0)], "L": [dict(bots=14)]}


@op("targets_by_path", "query", _BOT_SETS)
class _ByPath:
    def run(m, args, env):
        r = m.frontier_targets_by_path(_bots(env.size, args))
        return {k: r[k] for k in _TARGET_KEYS}

    def expect(model, args, got):
        w = AR.assign(model.grid, centroids_of(model), _bots(model.size, args), *model.geom, protocol().FRONTIER_SEPARATION)
        return {k: w[k] for k in _TARGET_KEYS}


@op("targets_by_gain", "query", _BOT_SETS)
class _ByGain:
    def run(m, args, env):
        r = m.frontier_targets_by_gain(_bots(env.size, args))
        return {k: r[k] for k in GR.KEYS}

    def expect(model, args, got):
        _, gain, _ = GR.frontier_gain(model.grid)
        w = GR.assign(model.grid, centroids_of(model), gain, _bots(model.size, args), *model.geom, protocol().FRONTIER_SEPARATION)
        return {k: w[k] for k in GR.KEYS}


@op("targets_by_territory", "query", _BOT_SETS)
class _ByTerritory:
    def run(m, args, env):
        r = m.frontier_targets_by_territory(_bots(env.size, args))
        return {k: r[k] for k in _TARGET_KEYS + ("area", "box")}

    def expect(model, args, got):
        w = TR.targets(model.grid, centroids_of(model), _bots(model.size, args), *model.geom)
        out = {k: w[k] for k in ("idx", "xy", "status", "waypoint_cell", "waypoint", "area", "box")}
        out["cost"] = w["cost_b"]
        return out


@op("territories", "query", {"S": [dict(bots=1, owner=True, cost=True), dict(bots=0, owner=False, cost=False)],
                             "L": [dict(bots=14, owner=True, cost=True), dict(bots=14, owner=False, cost=False), dict(bots=14, owner=True, cost=False)]})
class _Territories:
    def run(m, args, env):
        r = m.territories(_bots(env.size, args), return_owner=args["owner"], return_cost=args["cost"])
        del r["stats"]
        return r

    def expect(model, args, got):
        w = TR.partition(model.grid, _bots(model.size, args), *model.geom)
        return {k: w[k] for k in ("status", "area", "box") + (("owner",) if args["owner"] else ()) + (("cost",) if args["cost"] else ())}


@op("frontier_gain", "query", {"S": [dict(range=1), dict(range=24)], "L": [dict(range=64)]})
class _Gain:
    def run(m, args, env):
        view, gain = m.frontier_gain(range=args["range"])
        return dict(view=view, gain=gain)

    def expect(model, args, got):
        view, gain, _ = GR.frontier_gain(model.grid, 3, args["range"])
        return dict(view=view, gain=gain)


_MATCH_SETS = {"S": [dict(n=1, stride=751, radius=0), dict(n=3, stride=743, radius=2)], "L": [dict(n=65, stride=751, radius=7), dict(n=65, stride=743, radius=2)]}


@op("match", "query", _MATCH_SETS)
class _Match:
    def run(m, args, env):
        buf = device_sweeps(m, env.size, args, env.filt[1])
        p = dict(MATCH_PARAMS, radius=args["radius"])
        out, rot = m.match_sweeps(buf, params=p, rotations=True)
        return dict(buf=buf, rot=rot, matches=out, field=m.match_field(args["radius"]))

    def expect(model, args, got):
        buf = model_sweeps(model, args, got)
        p = dict(MATCH_PARAMS, radius=args["radius"])
        mt = MR.match(model.grid, model.geom, buf, p, None, *model.filt, rot=aux(got, "rot"), drift=model.drift())
        out = dict(buf=buf, matches=mt, field=MR.field(model.grid, args["radius"]).astype(np.uint8))
        if got is not None:
            out["rot"] = got["rot"]
        return out


@op("check_sweeps", "query", {"S": [dict(n=1, stride=751), dict(n=3, stride=743)], "L": [dict(n=65, stride=751)]})
class _Check:
    def run(m, args, env):
        buf = device_sweeps(m, env.size, args, env.filt[1])
        ck, cls = m.check_sweeps(buf, classes=True)
        return dict(buf=buf, checks=ck, classes=cls)

    def expect(model, args, got):
        buf = model_sweeps(model, args, got)
        sc = None if got is None else np.stack([got["checks"]["sin_yaw"], got["checks"]["cos_yaw"]], axis=1)
        ck, cls = CR.check(model.grid, model.geom, buf, None, None, *model.filt, sincos=sc, drift=model.drift())
        return dict(buf=buf, checks=ck, classes=cls)


def box_of(size, what):
    """The search boxes of the relocalisation ops: None is the whole grid."""
    c = size // 2 + 3
    return {"cell": (c, c, c + 1, c + 1), "tile": (32, 32, 48, 48), "grid": None, "empty": (5, 5, 5, 9)}[what]


_RELOC_SETS = {"S": [dict(n=1, stride=751, n_rot=8, box="cell", radius=2), dict(n=1, stride=743, n_rot=45, box="tile", radius=0),
                     dict(n=3, stride=751, n_rot=180, box="cell", radius=7), dict(n=1, stride=751, n_rot=8, box="empty", radius=2)],
               "L": [dict(n=1, stride=751, n_rot=8, box="grid", radius=2), dict(n=65, stride=743, n_rot=8, box="tile", radius=2),
                     dict(n=65, stride=751, n_rot=45, box="cell", radius=7), dict(n=1, stride=751, n_rot=180, box="grid", radius=0)]}


@op("relocalise_sweeps", "query", _RELOC_SETS)
class _Reloc:
    def run(m, args, env):
        buf = device_sweeps(m, env.size, args, env.filt[1])
        p = dict(n_rot=args["n_rot"], radius=args["radius"], box=box_of(env.size, args["box"]))
        return dict(buf=buf, out=m.relocalise_sweeps(buf, params=p))

    def expect(model, args, got):
        buf = model_sweeps(model, args, got)
        p = dict(n_rot=args["n_rot"], radius=args["radius"], box=box_of(model.size, args["box"]))
        return dict(buf=buf, out=RR.reloc(model.grid, model.geom, buf, p, None, *model.filt))


_GROUP_SETS = {"S": [dict(groups=(1,), travel=0.0, n_rot=8, box="cell", radius=2, stride=751),
                     dict(groups=(4,), travel=2.0, n_rot=45, box="cell", radius=0, stride=743)],
               "L": [dict(groups=(16, 4, 1), travel=2.0, n_rot=8, box="tile", radius=2, stride=751),
                     dict(groups=(1, 1), travel=0.0, n_rot=8, box="grid", radius=7, stride=751),
                     dict(groups=(16, 16), travel=2.0, n_rot=45, box="cell", radius=2, stride=743)]}


def group_inputs(size, args):
    """A bot per group that turns a little and drives 0.1 m between its sweeps: (poses float32 [n, 3], agent, odometry)."""
    rng = rng_of(args, 7)
    gs = [int(g) for g in args["groups"]]
    first = draw_poses(size, len(gs), rng)
    poses = []
    for g, p in zip(gs, first):
        x, y, yaw = (float(v) for v in p)
        for _ in range(g):
            poses.append((x, y, yaw))
            yaw += rng.uniform(-0.3, 0.3)
            x, y = x + 0.1 * math.cos(yaw), y + 0.1 * math.sin(yaw)
    n = len(poses)
    return np.array(poses, dtype=np.float32).reshape(n, 3), np.ones(n, dtype=np.uint8), int(args["stride"]) == 751


@op("relocalise_groups", "query", _GROUP_SETS)
class _Groups:
    def run(m, args, env):
        poses, agent, odo = group_inputs(env.size, args)
        buf = m.sense_sweeps(poses, agent, odometry=odo, max_range=env.filt[1], noise_amp=0.01, seed=int(args["seed"]), no_return=NO_RETURN)
        p = dict(n_rot=args["n_rot"], radius=args["radius"], box=box_of(env.size, args["box"]))
        return dict(buf=buf, out=m.relocalise_groups(buf, list(args["groups"]), travel=args["travel"], params=p))

    def expect(model, args, got):
        if got is not None:
            buf = got["buf"]
        else:
            poses, agent, odo = group_inputs(model.size, args)
            buf = SR.sense_sweeps(protocol(), model.grid, *model.geom, poses, agent, odometry=odo, max_range=model.filt[1], noise_amp=0.01,
                                  seed=int(args["seed"]), no_return=NO_RETURN)
        p = dict(n_rot=args["n_rot"], radius=args["radius"], box=box_of(model.size, args["box"]))
        return dict(buf=buf, out=RG.reloc_groups(model.grid, model.geom, buf, list(args["groups"]), None, args["travel"], p, None, *model.filt))


@op("sense", "query", {"S": [dict(n=1, beams=181), dict(n=3, beams=4)], "L": [dict(n=65, beams=181)]})
class _Sense:
    """Ranges and hit cells against the restatement, but for the beams whose far point lies within 1e-6 of a cell border
    (sense_rules.edge_beams: the device is not compared on those); the packets are protocol.pack_sweeps of the device's ranges."""

    def run(m, args, env):
        poses = draw_poses(env.size, int(args["n"]), rng_of(args, 8))
        kw = dict(max_range=env.filt[1], noise_amp=0.01, seed=int(args["seed"]), no_return=NO_RETURN)
        ranges, cells = m.sense_ranges(poses, beams=args["beams"], return_cells=True, **kw)
        edge = SR.edge_beams(*geometry(env.size)[1:], poses, args["beams"], env.filt[1])
        out = dict(ranges=np.where(edge, np.float32(0), ranges), cells=np.where(edge, 0, cells))
        if args["beams"] == 181:
            agent = np.ones(len(poses), dtype=np.uint8)
            out["packed"] = bool((m.sense_sweeps(poses, agent, **kw) == protocol().pack_sweeps(agent, poses[:, 0], poses[:, 1], poses[:, 2], ranges)).all())
        return out

    def expect(model, args, got):
        poses = draw_poses(model.size, int(args["n"]), rng_of(args, 8))
        ranges, cells = SR.sense_ranges(model.grid, *model.geom, poses, args["beams"], max_range=model.filt[1], noise_amp=0.01,
                                        seed=int(args["seed"]), no_return=NO_RETURN)
        edge = SR.edge_beams(*model.geom, poses, args["beams"], model.filt[1])
        out = dict(ranges=np.where(edge, np.float32(0), ranges), cells=np.where(edge, 0, cells))
        if args["beams"] == 181:
            out["packed"] = True
        return out


_VIEW_SETS = {"S": [dict(width=1, height=1, scale=100.0, zones=0, prims=0)],
              "L": [dict(width=300, height=200, scale=40.0, zones=4, prims=40), dict(width=300, height=200, scale=40.0, zones=0, prims=0),
                    dict(width=300, height=200, scale=12.0, zones=0, prims=0)]}


def view_lists(size, args):
    """(zones, prims) records of a render_view op: boxes and points, squares and segments over the world and off it."""
    P = protocol()
    rng = rng_of(args, 9)
    half = size * RES / 2
    z = np.zeros(int(args["zones"]), dtype=P.VIEW_ZONE_DTYPE)
    for k in range(len(z)):
        a, b = np.sort(rng.uniform(-1.2 * half, 1.2 * half, 2)), np.sort(rng.uniform(-1.2 * half, 1.2 * half, 2))
        z["box"][k] = (a[0], b[0], a[1], b[1])
        z["color"][k, :3] = rng.integers(0, 256, 3)
    q = np.zeros(int(args["prims"]), dtype=P.VIEW_PRIM_DTYPE)
    for k in range(len(q)):
        q["x0"][k], q["y0"][k], q["x1"][k], q["y1"][k] = rng.uniform(-1.3 * half, 1.3 * half, 4)
        q["kind"][k], q["size"][k] = k % 3, (1, 8, 1)[k % 3]
        q["color"][k, :3] = rng.integers(0, 256, 3)
    return z, q


@op("render_view", "query", _VIEW_SETS)
class _View:
    def run(m, args, env):
        z, q = view_lists(env.size, args)
        return m.render_view(args["width"], args["height"], args["scale"], zones=z, prims=q, draw_occupied=True)

    def expect(model, args, got):
        z, q = view_lists(model.size, args)
        p = VR.params(args["width"], args["height"], args["scale"], draw_occupied=True)
        return VR.render(p, model.grid, *model.geom, *VR.from_records(z, q))


def cloud_of(args):
    rng = rng_of(args, 10)
    return rng.uniform(-3.0, 3.0, (int(args["n"]), 2))


@op("voxel", "query", {"S": [dict(n=1), dict(n=1025)], "L": [dict(n=70001)]})
class _Voxel:
    def run(m, args, env):
        t = env.torch
        xy = cloud_of(args)
        d_in = t.from_numpy(xy).cuda()
        t.cuda.synchronize()
        k = m.voxel_downsample_device(d_in, len(xy), VOXEL)
        d_out = t.zeros((max(k, 1), 2), dtype=t.float64, device="cuda")
        t.cuda.synchronize()
        k2 = m.voxel_downsample_device(d_in, len(xy), VOXEL, d_out, k)
        return dict(k=int(k), k2=int(k2), xy=d_out.cpu().numpy()[:k])

    def expect(model, args, got):
        want = orc.voxel_downsample(cloud_of(args), VOXEL)
        return dict(k=len(want), k2=len(want), xy=want)


def _merge_result(r):
    return {k: r[k] for k in ("status", "T", "fitness", "rmse", "iterations", "n_local", "n_global")}


@op("merge", "query", {"-": [dict()]}, twin=False)
class _Merge:
    """One map_callback with the context's own map as the message, shifted by a few centimetres more each time, then the session's
    cloud and global map."""

    def run(m, args, env):
        k = env.merges = env.merges + 1
        r = m.merge_grid(m.grid_i8(), m.res, m.ox + 0.01 * (k % 5), m.oy - 0.015 * (k % 3))
        g, origin = m.merge_global_map()
        return dict(result=_merge_result(r), cloud=m.merge_cloud(), map=g, origin=None if origin is None else np.asarray(origin))

    def expect(model, args, got):
        k = model.merges = model.merges + 1
        res, ox, oy = model.geom
        r = model.session.callback(model.grid, res, ox + 0.01 * (k % 5), oy - 0.015 * (k % 3))
        r["T"] = np.asarray(r["T"], dtype=np.float64).reshape(3, 3)
        r["fitness"], r["rmse"] = float(r["fitness"]), float(r["rmse"])
        g, origin = model.session.publish()
        return dict(result=_merge_result(r), cloud=model.session.cloud, map=g, origin=None if origin is None else np.asarray(origin))


@op("last", "query", {"-": [dict()]}, twin=False)
class _Last:
    def run(m, args, env):
        names = ("last_batch", "last_sweeps", "last_sweep_matches", "last_sweep_checks", "last_sweep_nodes")
        return {name: refusing(getattr(m, name), env.errors) for name in names}

    def expect(model, args, got):
        out = dict.fromkeys(("last_batch", "last_sweeps", "last_sweep_matches", "last_sweep_checks", "last_sweep_nodes"), Refused("not the last ingest"))
        if model.last is None:
            return out
        if model.last[0] == "packets":
            acc, pose = model.last[1], model.last[2]
            if got is not None and not isinstance(got["last_batch"], Refused):      # a rejected record's pose is not specified
                pose = np.where(acc[:, None] == 1, pose, got["last_batch"][1])
            out["last_batch"] = (acc, pose)
            return out
        _, form, graph, a = model.last
        out["last_sweeps"] = (a["acc"], a["pose"])
        if form == "match":
            out["last_sweep_matches"] = a["matches"]
        if form == "check":
            out["last_sweep_checks"] = a["checks"]
        if graph:
            out["last_sweep_nodes"] = (a["node"], a["lm"])
        return out


_REFUSALS = (("plan", "reloc"), ("groups", "match"), ("check", "sense"), ("view", "gain"), ("filter", "territories"))


@op("refused", "query", {"-": [dict(families=f) for f in _REFUSALS]}, twin=False)
class _Refusal:
    """A call with a parameter the documented argument check refuses, then at once the same call made valid: (refusal, shape)."""

    def run(m, args, env):
        buf = device_sweeps(m, env.size, dict(n=1, seed=args["seed"]), env.filt[1])
        pose = draw_poses(env.size, 1, rng_of(args, 11))
        bots = draw_points(env.size, 2, rng_of(args, 12), odd=False)
        calls = {
            "plan": lambda bad: m.plan_paths(bots[:1], bots[1:], clearance=17 if bad else 2)["status"].shape,
            "reloc": lambda bad: m.relocalise_sweeps(buf, params=dict(n_rot=0 if bad else 8, box=box_of(env.size, "cell"))).shape,
            "groups": lambda bad: m.relocalise_groups(buf, [1], travel=-1.0 if bad else 0.0, params=dict(n_rot=8, box=box_of(env.size, "cell"))).shape,
            "match": lambda bad: m.match_sweeps(buf, params=dict(MATCH_PARAMS, radius=-1 if bad else 2)).shape,
            "check": lambda bad: m.check_sweeps(buf, params=dict(min_checked=182 if bad else 20)).shape,
            "sense": lambda bad: m.sense_ranges(pose, max_range=-1.0 if bad else 1.2).shape,
            "view": lambda bad: m.render_view(0 if bad else 2, 2, 100.0).shape,
            "gain": lambda bad: m.frontier_gain(range=65 if bad else 24)[1].shape[1:],
            "filter": lambda bad: m.set_sweep_filter(1.0, 0.5) if bad else m.set_sweep_filter(*env.filt),
            "territories": lambda bad: m.territories(bots, clearance=-1 if bad else 2)["area"].shape,
        }
        return {f: dict(bad=refusing(lambda: calls[f](True), env.errors), good=calls[f](False)) for f in args["families"]}

    def expect(model, args, got):
        good = {"plan": (1,), "reloc": (1,), "groups": (1,), "match": (1,), "check": (1,), "sense": (1, 181), "view": (2, 2, 4), "gain": (),
                "filter": None, "territories": (2,)}
        return {f: dict(bad=Refused("argument check"), good=good[f]) for f in args["families"]}


WRITERS = [n for n, o in OPS.items() if o.kind == "writer"]
QUERIES = [n for n, o in OPS.items() if o.kind == "query"]
PREDS = ("rays", "packets", "sweeps", "restore", "reset")        # the order inside a block: a reset is followed by the next block's paint


# ---- the generator ----------------------------------------------------------------------------------------------------------------
# (size, seed) of the GPU test's walks.  136 cells: a multiple of 4, ragged against the 16-cell relocalisation tile, the 64-cell
# planner tile and the 16 x 4 dirty block; 68: every patch hangs over every edge
WALKS = ((136, 11), (136, 12), (136, 13), (68, 14))
MAX_OPS = 60


def generate(walks=WALKS):
    """The op lists of the walks, one list of (name, args) per (size, seed).

    The lists are built, not drawn: len(QUERIES) blocks of five (writer, query) pairs -- update_rays, packets, sweeps, restore,
    reset -- are dealt to the walks in runs.  In block b the query after writer kind p is query (b + p) mod len(QUERIES) of a
    seeded permutation, so every query follows every kind once, and its five occurrences lie in consecutive blocks, three or more
    of them in one walk: there a sized op takes its small, large and again small arguments.  The seeds choose the permutation, the
    argument set of every op and every op's own seed.  Settings writers go in front of a block's map writers; one
    relocalise_groups directly follows a relocalise_sweeps with another box, and the reverse."""
    walks = tuple(walks)
    nq = len(QUERIES)
    order = [QUERIES[i] for i in np.random.default_rng([s for _, s in walks]).permutation(nq)]
    share, extra = divmod(nq, len(walks))
    forms = ("plain", "match", "check")
    out, b0, refusals = [], 0, 0
    for w, (size, seed) in enumerate(walks):
        nb = share + (1 if w < extra else 0)
        rng = np.random.default_rng(seed)
        seen = {}

        def item(name, cls=None, which=None):
            """(name, args): a sized op's k-th occurrence in the walk is small, large, small, ...; cls and which override."""
            o = OPS[name]
            k = seen[name] = seen.get(name, -1) + 1
            cls = (cls or "SLSLS"[k % 5]) if o.sized else "-"
            sets = o.sets[cls]
            args = dict(sets[int(rng.integers(len(sets))) if which is None else which % len(sets)])
            args["seed"] = int(rng.integers(1 << 30))
            if o.sized:
                args["size_class"] = cls
            return name, args

        def other_box(args):
            return "tile" if args["box"] != "tile" else "cell"

        ops, paired = [], set()
        for k in range(nb):
            b = b0 + k
            for p, pred in enumerate(PREDS):
                graph = False
                if pred == "rays":
                    if k % 2 == 0:                                 # 1.2 m (the default) -> 3.0 m -> 1.2 m -> 3.0 m
                        ops.append(item("set_sweep_filter", which=1 if k % 4 == 0 else 0))
                    ops.append(item("update_rays", which=1 if k % 3 == 2 else 0))
                elif pred == "packets":
                    ops.append(item("ingest_packets"))
                elif pred == "sweeps":
                    form = forms[(k + w) % 3]
                    graph = k == 3 and form != "check"
                    if graph:
                        ops.append(item("set_sweep_graph", which=0))
                    elif k == 3:                                   # graph mode refuses the guarded ingest: once, then the ingest proper
                        ops += [item("set_sweep_graph", which=0), item("ingest_sweeps_check", cls="SLSLS"[k % 5]), item("set_sweep_graph", which=1)]
                    ops.append(item("ingest_sweeps_" + form, cls="SLSLS"[k % 5]))
                else:
                    ops.append(item(pred))
                q = order[(b + p) % nq]
                if q == "refused":
                    ops.append(item(q, which=refusals))
                    refusals += 1
                else:
                    ops.append(item(q))
                if q == "relocalise_sweeps" and k % 2 == 0 and "groups" not in paired:
                    paired.add("groups")
                    ops.append(("relocalise_groups", dict(groups=(4, 1), travel=2.0, n_rot=ops[-1][1]["n_rot"], box=other_box(ops[-1][1]), radius=2,
                                                          stride=751, seed=int(rng.integers(1 << 30)), size_class="S")))
                elif q == "relocalise_groups" and k % 2 == 1 and "sweeps" not in paired:
                    paired.add("sweeps")
                    ops.append(("relocalise_sweeps", dict(n=3, stride=751, n_rot=ops[-1][1]["n_rot"], box=other_box(ops[-1][1]), radius=2,
                                                          seed=int(rng.integers(1 << 30)), size_class="S")))
                if graph:
                    ops.append(item("set_sweep_graph", which=1))
                if pred == "reset" and k in (0, nb - 2):           # the map is empty: tracking may be switched on
                    ops.append(item("dirty_tracking", which=0 if k == 0 else 1))
        b0 += nb
        out.append(ops)
    return out


def as_literal(ops):
    """The op list as text that evaluates to it."""
    return "[" + ",\n ".join(repr(o) for o in ops) + "]"


# ---- walking a context ----------------------------------------------------------------------------------------------------------------
def same_map(m, model):
    """'' when grid_i8() and counts() of the context are the model's."""
    h, mi = m.counts()
    return differing(dict(grid=m.grid_i8(), hits=h, misses=mi), dict(grid=model.grid, hits=np.array(model.o.hits), misses=np.array(model.o.misses)),
                     "map")


def walk(m, model, env, ops, tag="", twin=None, every=5, failures=None):
    """The ops in turn on the context and on the model.  After every op (a) the answer is the model's, and a query a checkpoint
    covers answers the same when it is asked again at once; after every writer (b) grid_i8() and counts() are the oracle's and the
    five last-ingest calls answer or refuse as the model says; every `every` ops and at the end (c) twin(m, model, env) -- a new context restored
    from m.checkpoint(), with its own Env -- answers the last query a checkpoint covers as the used context answers it now.
    A difference raises AssertionError with the tag, the op's index and the list so far as a literal; with a `failures` list
    it is appended there instead and the walk goes on."""
    def fail(i, what):
        text = f"{tag}: op {i} {ops[i][0]}: {what}\nops = {as_literal(ops[:i + 1])}"
        if failures is None:
            raise AssertionError(text)
        failures.append(text)

    last_query = None
    for i, (name, args) in enumerate(ops):
        o = OPS[name]
        try:
            got = o.run(m, args, env)
        except env.errors as e:                                # a refusal nobody expected
            fail(i, f"refused: {e}")
            got = None
        want = o.expect(model, args, got)
        why = differing(got, want)
        if why:
            fail(i, why)
        if o.kind == "writer":
            why = same_map(m, model)
            if not why:
                last = OPS["last"].run(m, {}, env)
                why = differing(last, OPS["last"].expect(model, {}, last), "last ingest")
            if why:
                fail(i, "after the writer, " + why)
        elif o.twin:
            last_query = i
            why = differing(o.run(m, args, env), got, "asked again")      # (mission control asks the same thing every few seconds)
            if why:
                fail(i, "the same query asked twice in a row: " + why)
        if twin is not None and last_query is not None and ((i + 1) % every == 0 or i == len(ops) - 1):
            qname, qargs = ops[last_query]
            t, tenv = twin(m, model, env)
            try:
                why = differing(OPS[qname].run(t, qargs, tenv), OPS[qname].run(m, qargs, env), "twin")
            finally:
                t.close()
            if why:
                fail(i, f"a context restored from the checkpoint answers op {last_query} {qname} differently: {why}")
