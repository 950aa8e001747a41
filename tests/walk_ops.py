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
import ray_scenes as RS
import reloc_group_rules as RG
import reloc_rules as RR
import sense_rules as SR
import sweep_graph_rules as SG
import sweep_veil_rules as SV
import territory_rules as TR
import trail_reloc_rules as TRR
import trail_rules as TL
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
class _Geo:
    """The walk's grid as veil_rules and sweep_veil_rules take a geometry (ray_scenes.Geo's size, res, ox, oy and oracle)."""

    def __init__(self, size):
        self.size, self.res, self.ox, self.oy = geometry(size)

    def oracle(self, max_agent=2):
        return orc.OracleMapper(self.size, self.res, self.ox, self.oy, 0.0, max_agent=max_agent)


class Model:
    """What a context must show: an orc.OracleMapper for the map and its counters, the settings (sweep filter, graph mode, dirty
    tracking), the number of pose-graph nodes, the merge session (merge_rules.Session over the oracle's grid_to_pcd,
    voxel_downsample and rasterise and the registration given: the oracle's icp_planar by default) and what the last ingest was.

    The bot veil (V1-V7, S0-S8) is sweep_veil_rules.SweepVeilModel's: its table, its running total and the flags it returns.
    `o` is fed the bytes and goes on giving acceptance, poses, nodes and drift.  Until a veil first acts it is the map as well,
    exactly as before; from then on (until a reset) the map is `mo`, a second oracle that has replayed the session so far and is
    driven ray by ray with `valid & ~veiled` by the veil model, whether or not the veil acts in a later call."""

    def __init__(self, size, register=None):
        self.size = size
        self.geom = geometry(size)[1:]
        self.world = cached(("world", size), lambda: world(size))
        self.filt = NEAR
        self.graph_on = False
        self.tracking = False
        self.session = MG.Session(orc.grid_to_pcd, register or orc.icp_planar, orc.voxel_downsample, orc.rasterise)
        self.merges = 0
        self.veil_radius, self.veil_sweeps = 0, False      # kept over reset and restore (V2, S0)
        self.min_margin = math.inf       # of the end points of the packets the veil model has cast, in cells (VeilModel.min_margin)
        self._new_map()

    def _new_map(self):
        self.o = orc.OracleMapper(*geometry(self.size), 0.0)
        self.mo = None                   # the map once a veil has acted
        self.log = []                    # ("stream", buf) | ("rays", batch): what mo replays when it is made
        self.veil = SV.SweepVeilModel(_Geo(self.size), 2, 0)
        self.veil_src = {}               # bot -> "place" | "packets" | "sweeps": who wrote its table entry
        self.flags = None                # the veil flags of the last ingest, uint8 [n, 4] or [n, 181]
        self.hits_judged = 0             # QS_CNT_HITS: beams the filter judged hits (V5, S4)
        self.graph_sweeps = 0            # accepted sweeps that became pose-graph nodes
        self.unfused = False
        self.last = None                 # None, ("packets", acc, pose), ("sweeps", form, graph, dict of arrays)
        self._grid = None

    @property
    def mapo(self):
        return self.o if self.mo is None else self.mo

    @property
    def grid(self):
        if self._grid is None:
            self._grid = np.array(self.mapo.grid, dtype=np.int8)
        return self._grid

    def wrote(self):
        self._grid = None
        self.unfused = True

    def reset(self):
        self._new_map()

    def restored(self):
        """qs_restore: the table is emptied and the running total starts again, as after a reset (V2); the settings stay."""
        self.last = self.flags = None
        self.veil.forget()
        self.veil.total = 0
        self.veil_src = {}

    def fork(self):
        """A veil is about to act: from here on the map is driven ray by ray."""
        if self.mo is None:
            self.mo = self.veil.g.oracle(2)
            for kind, what in self.log:
                if kind == "stream":
                    self.mo.feed_stream(what)
                else:
                    self.mo.update_rays(*what)
            self.log = None

    def cast(self, batch):
        """update_rays of the op table: never veiled (V7)."""
        self.o.update_rays(*batch)
        if self.mo is None:
            self.log.append(("rays", batch))
        else:
            self.mo.update_rays(*batch)

    def veil_model(self):
        """The veil model set to the context's settings and the model's oracles."""
        v = self.veil
        v.o, v.m = self.o, self.mo
        v.radius, v.sweeps, (v.smin, v.smax) = self.veil_radius, self.veil_sweeps, self.filt
        return v

    def heard(self, kind, agents, flags):
        """After an ingest the veil model ran: the flags of the last ingest and who fed the table."""
        self.flags = flags
        for b in agents:
            self.veil_src[int(b)] = kind

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


def with_odometry(buf):
    """The records as uint8 [n, 751]: what sweep_veil_rules reads (a 743-byte record has no encoder and v2v fields: zeros)."""
    if buf.shape[1] == 751:
        return buf
    src = MR.records_of(buf)
    out = np.zeros(len(src), dtype=protocol().PACKET_DTYPE_V0_ODO)
    for f in src.dtype.names:
        out[f] = src[f]
    return out.view(np.uint8).reshape(len(src), 751)


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
    seed); no landmark, so no closure; from n = 16 on one record carries agent 9.  With `clear` in the args (the veil walks) a
    record is drawn again until the end points of its four rays keep more than ray_scenes.MARGIN of a cell from every cell edge:
    the veil is decided by end cells, and never for a ray the exact-trig rule leaves to the host (V4)."""
    def make():
        rng = rng_of(args, 2)
        n = int(args["n"])
        poses = draw_poses(size, n, rng)
        agent = (np.arange(n) % 2 + 1).astype(np.uint8)
        if n >= 16:
            agent[7] = 9
        w = cached(("world", size), lambda: world(size))
        sense = lambda k: SR.sense_packets(protocol(), w, *geometry(size)[1:], poses[k], agent[k], max_range=1.2, no_return=NO_RETURN)
        buf = sense(slice(None))
        while args.get("clear"):
            near = packet_margins(size, buf) <= 2 * RS.MARGIN
            if not near.any():
                break
            poses[near] = draw_poses(size, int(near.sum()), rng)
            buf[near] = sense(near)                            # (a packet's ranges depend on its own pose alone)
        return buf
    return cached(("packets", size, int(args["n"]), int(args["seed"]), bool(args.get("clear"))), make)


def packet_margins(size, buf):
    """float64 [n]: per packet the least distance, in cells, of its four rays' end points from a cell edge (the reference's end
    point formula, as veil_rules.VeilModel.ingest forms it)."""
    rec = np.ascontiguousarray(buf).view(protocol().PACKET_DTYPE).reshape(-1)
    d = np.stack([rec[k] for k in ("front", "left", "back", "right")], axis=1).astype(np.float64)
    ok = (RS.MIN_D < d) & (d <= RS.MAX_D)
    length = np.where(ok, d, np.where(d > RS.MIN_D, np.minimum(d, RS.MAX_D), RS.MAX_D))
    a = rec["yaw"].astype(np.float64)[:, None] + np.array(RS.SENSOR_ANG)[None, :]
    hx, hy = rec["x"].astype(np.float64)[:, None] + length * np.cos(a), rec["y"].astype(np.float64)[:, None] + length * np.sin(a)
    return RS._margin(_Geo(size), hx, hy).min(axis=1)


@op("ingest_packets", "writer", {"S": [dict(n=1), dict(n=16)], "L": [dict(n=5000)]}, pred="packets")
class _Packets:
    def run(m, args, env):
        m.ingest_array(packets_of(env.size, args))
        return None

    def expect(model, args, got):
        buf = packets_of(model.size, args)
        rec = np.ascontiguousarray(buf).view(protocol().PACKET_DTYPE).reshape(-1)
        acc = ((rec["magic"] == b"QSRL") & (rec["agent"] >= 1) & (rec["agent"] <= 2)).astype(np.uint8)
        acting = model.veil_radius > 0
        if acting:
            model.fork()
        if model.mo is None:
            model.o.feed_stream(buf)
            model.log.append(("stream", buf))
            model.flags = np.zeros((len(buf), 4), dtype=np.uint8)
        else:                                                  # (the veil model feeds `o` the bytes itself)
            model.veil.min_margin = math.inf
            veiled, _ = model.veil_model().ingest(buf)
            model.min_margin = min(model.min_margin, model.veil.min_margin)
            model.heard("packets", np.unique(rec["agent"][acc == 1]) if acting else (), veiled)
        d = np.stack([rec[k] for k in ("front", "left", "back", "right")], axis=1).astype(np.float64)[acc == 1]
        model.hits_judged += int(((RS.MIN_D < d) & (d <= RS.MAX_D)).sum())
        model.wrote()
        pose = np.stack([rec["x"].astype(np.float64), rec["y"].astype(np.float64), rec["yaw"].astype(np.float64)], axis=1)
        model.last = ("packets", acc, pose)
        return None


def _sweeps_run(form):
    def run(m, args, env):
        if int(args["stride"]) not in (743, 751) or int(args["n"]) == 0:       # (a directed test's: no such record can be sensed)
            buf = np.zeros((int(args["n"]), int(args["stride"])), dtype=np.uint8)
        else:
            buf = device_sweeps(m, env.size, args, env.filt[1])
        out = dict(buf=buf)
        if form == "match" and len(buf) and buf.shape[1] in (743, 751):
            out["rot"] = m.match_sweeps(buf, params=MATCH_PARAMS, rotations=True)[1]
        if form == "check" and len(buf) and buf.shape[1] in (743, 751):
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
        if int(args["stride"]) not in (743, 751):              # refused before anything changes: the last ingest stays what it was
            return Refused("stride")
        if int(args["n"]) == 0:                                # a sweep ingest of nothing: the map stays, there is no last ingest
            model.last = model.flags = None
            return got if isinstance(got, dict) else None
        buf = model_sweeps(model, args, got)
        recs = MR.records_of(buf)
        acc, pose = MR.poses_of(recs, None, None, model.drift())
        accepted = acc.copy()
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
        acting = model.veil_sweeps and model.veil_radius > 0                    # S0
        if acting:
            model.fork()
        rays = MR.beams_of_all(cast[acc], recs["ranges"][acc], smin, smax) if acc.any() else None
        if rays is not None:
            model.o.update_rays(*rays)
            model.hits_judged += int(rays[4].sum())
        if model.mo is None:
            if rays is not None:
                model.log.append(("rays", rays))
            model.flags = np.zeros((len(recs), MR.BEAMS), dtype=np.uint8)
        else:                                                  # S1: cast from `cast`; a withheld record counts as rejected
            veiled, _ = model.veil_model().ingest_sweeps(with_odometry(buf), withheld=tuple(np.nonzero(accepted & ~acc)[0].tolist()), poses=cast)
            model.heard("sweeps", np.unique(recs["agent"][acc]) if acting else (), veiled)
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
            model.cast(batch)
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


@op("set_bot_veil", "writer", {"-": [dict(radius=0, sweeps=None), dict(radius=3, sweeps=True), dict(radius=8, sweeps=None), dict(radius=32, sweeps=True),
                                     dict(radius=3, sweeps=False)]})
class _SetVeil:
    def run(m, args, env):
        m.set_bot_veil(args["radius"], sweeps=args["sweeps"])
        return None

    def expect(model, args, got):
        model.veil_radius = int(args["radius"])
        if args["sweeps"] is not None:
            model.veil_sweeps = bool(args["sweeps"])
        return None


_SENSORS = ("front", "left", "back", "right")


def beam_of(size, at, beam):
    """(end x, end y, hit?) of beam `beam` of record 0 of the ingest op at = (name, n, seed): a packet's from its own bytes; a
    sweep's from the static world as a sensor reports it there (the device senses the painted map with the same poses: the end it
    maps lies within a cell or so of this one)."""
    name, n, seed = at

    def sensed():
        poses, agent, _ = sweep_inputs(size, dict(n=n, seed=seed))
        w = cached(("world", size), lambda: world(size))
        return MR.records_of(SR.sense_sweeps(protocol(), w, *geometry(size)[1:], poses[:1], agent[:1], odometry=True, max_range=NEAR[1],
                                             noise_amp=0.01, seed=seed, no_return=NO_RETURN))[0]
    if name == "ingest_packets":
        rec = np.ascontiguousarray(packets_of(size, dict(n=n, seed=seed, clear=True))).view(protocol().PACKET_DTYPE).reshape(-1)[0]
        d, a, lo = float(rec[_SENSORS[beam]]), float(rec["yaw"]) + RS.SENSOR_ANG[beam], RS.MIN_D
    else:
        rec = cached(("record 0", size, at), sensed)
        d, a, lo = float(rec["ranges"][beam]), float(rec["yaw"]) + math.radians(beam - 90), NEAR[0]
    return float(rec["x"]) + d * math.cos(a), float(rec["y"]) + d * math.sin(a), lo < d <= NEAR[1]


def _place_xy(size, args):
    return beam_of(size, tuple(args["at"]), args["beam"])[:2] if args.get("at") else (args["x"], args["y"])


@op("bot_veil_place", "writer", {"-": [dict(bot=2, x=0.26, y=-0.31, at=None, beam=None)]})
class _Place:
    """cell[bot] from a world position in the args, or from the end of beam `beam` of record 0 of the later ingest op `at` =
    (name, n, seed), so that a call of one record has something to be veiled by and the list stays a literal."""

    def run(m, args, env):
        m.bot_veil_place(args["bot"], *_place_xy(env.size, args))
        return None

    def expect(model, args, got):
        model.veil.o = model.o
        model.veil.place(args["bot"], *_place_xy(model.size, args))
        model.veil_src[int(args["bot"])] = "place"
        return None


@op("bot_veil_forget", "writer", {"-": [dict(bot=None), dict(bot=2)]})
class _Forget:
    def run(m, args, env):
        m.bot_veil_forget(args["bot"])
        return None

    def expect(model, args, got):
        model.veil.forget(args["bot"])
        for b in ([args["bot"]] if args["bot"] is not None else list(model.veil_src)):
            model.veil_src.pop(b, None)
        return None


# -- queries --
@op("views", "query", {"-": [dict()]})
class _Views:
    def run(m, args, env):
        h, mi = m.counts()
        return dict(grid=m.grid_i8(), hits=h, misses=mi, logodds=m.logodds())

    def expect(model, args, got):
        return dict(grid=model.grid, hits=np.array(model.mapo.hits), misses=np.array(model.mapo.misses), logodds=model.mapo.logodds())


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


TRAIL_STEP = 0.02               # metres between the packets of a trail: 64 of them fit the 68-cell world's room


def trails_of(size, args, own_frame):
    """(uint8 [trails * records, stride], gsize): seeded trails driven through the static world (trail_reloc_rules.drive, cast4
    at the packet filter's 1.2 m).  own_frame: each trail reports in a frame of its own (the relocaliser's input); otherwise it
    reports its true poses displaced rigidly by up to 2 cells and 2 angle steps (the matcher's).  Every third trail is bot 2's;
    from 16 records on one record carries agent 9."""
    def make():
        rng = rng_of(args, 14)
        w = cached(("world", size), lambda: world(size))
        geom = geometry(size)[1:]
        n, K = int(args["trails"]), int(args["records"])
        true = np.stack([TRR.drive(w, geom, rng, K, step=TRAIL_STEP) for _ in range(n)])
        ranges = np.stack([[TRR.cast4(w, geom, q, RS.MAX_D, rng, 0.01) for q in tr] for tr in true])
        if own_frame:
            pose = np.stack([TRR.reported(tr, rng.uniform(-math.pi, math.pi), rng.uniform(-10.0, 10.0, 2)) for tr in true])
        else:
            pose = np.stack([TL.displaced(tr, rng.integers(-2, 3, 3), RES) for tr in true])
        agent = np.repeat(np.where(np.arange(n) % 3 == 2, 2, 1), K)
        if n * K >= 16:
            agent[n * K // 2] = 9
        flat = pose.reshape(-1, 3)
        return TL.pack(agent, flat[:, 0], flat[:, 1], flat[:, 2], ranges.reshape(-1, 4))
    key = ("trails", size, own_frame, int(args["trails"]), int(args["records"]), int(args["seed"]))
    buf = cached(key, make)
    return np.ascontiguousarray(buf[:, :int(args["stride"])]), np.full(int(args["trails"]), int(args["records"]), dtype=np.int32)


_TRAIL_MATCH_SETS = {"S": [dict(trails=1, records=1, stride=42, radius=2, travel=4.0), dict(trails=1, records=4, stride=41, radius=0, travel=0.5)],
                     "L": [dict(trails=1, records=64, stride=42, radius=7, travel=4.0), dict(trails=65, records=4, stride=41, radius=2, travel=4.0)]}


@op("match_trails", "query", _TRAIL_MATCH_SETS)
class _MatchTrails:
    def run(m, args, env):
        buf, gs = trails_of(env.size, args, False)
        p = dict(MATCH_PARAMS, radius=args["radius"], min_hits=8)
        out, rot = m.match_trails(buf, gs, travel=args["travel"], params=p, rotations=True)
        return dict(rot=rot, out=np.frombuffer(out.tobytes(), dtype=TL.TRAIL_DTYPE))

    def expect(model, args, got):
        buf, gs = trails_of(model.size, args, False)
        p = dict(MATCH_PARAMS, radius=args["radius"], min_hits=8)
        out, rot = TL.match(model.grid, model.geom, buf, gs, p, args["travel"], None, aux(got, "rot"), drift=model.drift())
        return dict(rot=rot if got is None else got["rot"], out=out)


_TRAIL_RELOC_SETS = {"S": [dict(trails=1, records=1, stride=42, n_rot=8, box="cell", radius=2, travel=0.0),
                           dict(trails=1, records=4, stride=41, n_rot=45, box="tile", radius=0, travel=0.6)],
                     "L": [dict(trails=1, records=64, stride=42, n_rot=8, box="grid", radius=2, travel=2.0),
                           dict(trails=65, records=4, stride=41, n_rot=8, box="tile", radius=2, travel=0.6),
                           dict(trails=1, records=64, stride=42, n_rot=180, box="cell", radius=7, travel=3.0)]}


@op("relocalise_trails", "query", _TRAIL_RELOC_SETS)
class _RelocTrails:
    def run(m, args, env):
        buf, gs = trails_of(env.size, args, True)
        p = dict(n_rot=args["n_rot"], radius=args["radius"], box=box_of(env.size, args["box"]), min_hits=8)
        out, rot = m.relocalise_trails(buf, gs, travel=args["travel"], params=p, rotations=True)
        return dict(rot=rot, out=np.frombuffer(out.tobytes(), dtype=TRR.TRAIL_RELOC_DTYPE))

    def expect(model, args, got):
        buf, gs = trails_of(model.size, args, True)
        p = dict(n_rot=args["n_rot"], radius=args["radius"], box=box_of(model.size, args["box"]), min_hits=8)
        out, rot = TRR.reloc_trails(model.grid, model.geom, buf, gs, p, args["travel"], None, aux(got, "rot"))
        return dict(rot=rot if got is None else got["rot"], out=out)


@op("veil_state", "query", {"-": [dict()]}, twin=False)
class _VeilState:
    """The settings, the table, the running total, the flags of the last ingest -- answered or refused as the header says: the
    packet flags after a packet ingest, the sweep flags after a sweep ingest of at least one record, zeros where no veil acted --
    and the counters a veiled beam leaves alone (rays, hits) or lowers (cells)."""

    def run(m, args, env):
        c = m.counters()
        return dict(radius=m.bot_veil(), sweeps=m.bot_veil_sweeps(), cells=m.bot_veil_cells(), stats=m.bot_veil_stats(),
                    last_veiled=refusing(m.last_veiled, env.errors), last_sweeps_veiled=refusing(m.last_sweeps_veiled, env.errors),
                    counters={k: c[k] for k in ("cells", "rays", "hits")})

    def expect(model, args, got):
        kind = model.last[0] if model.last is not None else None
        no = Refused("not the last ingest")
        return dict(radius=model.veil_radius, sweeps=model.veil_sweeps, cells=model.veil.cells(), stats=model.veil.total,
                    last_veiled=model.flags if kind == "packets" else no, last_sweeps_veiled=model.flags if kind == "sweeps" else no,
                    counters=dict(cells=int(model.mapo.n_cells_written), rays=int(model.mapo.n_rays), hits=model.hits_judged))


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
VEIL_QUERIES = ("match_trails", "relocalise_trails", "veil_state", "match", "check_sweeps", "relocalise_sweeps", "relocalise_groups", "views", "frontier",
                "last")          # the query list of the veil walks (generate_veil)
QUERIES = [n for n, o in OPS.items() if o.kind == "query" and n not in VEIL_QUERIES[:3]]      # the nineteen of the first four walks
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


# ---- the veil walks -------------------------------------------------------------------------------------------------------------------
VEIL_WALKS = ((136, 21), (136, 22), (68, 23))
# One entry per block, dealt to the walks in runs of 4, 3 and 3.  veil: the set_bot_veil (radius, sweep switch) in front of the
# block (None: as it stands -- the settings survive the reset that ends a block, the table does not); packets: the block's
# packet ingest; form, n: its sweep ingest; graph: in graph mode, after a guarded ingest that graph mode refuses.
#   walk 0: calls of one record with the veil acting, off, acting again (direct kernel against tiled form); then graph mode
#   walk 1: the large calls acting and off; the packet veil without the sweep switch
#   walk 2: 68 cells; off from the start, then radius 32, where nearly every beam of the small room ends near the other bot
_VEIL_PLAN = (dict(veil=(3, True), packets=1, form="plain", n=1), dict(veil=(0, None), packets=1, form="match", n=1),
              dict(veil=(8, None), packets=1, form="check", n=1), dict(veil=(32, True), packets=16, form="match", n=65, graph=True),
              dict(veil=(32, True), packets=5000, form="plain", n=65), dict(veil=(0, None), packets=5000, form="check", n=3),
              dict(veil=(3, False), packets=16, form="match", n=3),
              dict(veil=None, packets=16, form="plain", n=3), dict(veil=(32, True), packets=1, form="match", n=3),
              dict(veil=None, packets=5000, form="check", n=65))
_VEIL_SETS = {(0, None): 0, (3, True): 1, (8, None): 2, (32, True): 3, (3, False): 4}      # set_bot_veil's argument sets


def generate_veil(walks=VEIL_WALKS):
    """The op lists of the veil walks: the block scheme of generate() over VEIL_QUERIES and _VEIL_PLAN.

    Beyond the scheme: while the veil acts, bot 2 is placed on the end of a beam of record 0 in front of every call of one record
    (record 0 is bot 1's); after the first such packet ingest bot 2 is forgotten and the same packet ingested again; in the last
    block a sweep of one record follows the packet ingest and a packet of one record the sweep ingest, with nothing in between
    that empties the table; relocalise_trails directly follows a relocalise_groups with another n_rot, box and travel, and the
    reverse, and match_trails a match with another radius and stride, and the reverse; a walk's first reset under the veil finds
    a bot placed by its world position."""
    walks = tuple(walks)
    nq = len(VEIL_QUERIES)
    order = [VEIL_QUERIES[i] for i in np.random.default_rng([s for _, s in walks]).permutation(nq)]
    runs = (4, 3, 3)
    out, b0 = [], 0
    for w, (size, seed) in enumerate(walks):
        rng = np.random.default_rng(seed)
        seen = {}

        def item(name, cls=None, which=None, **fixed):
            o = OPS[name]
            k = seen[name] = seen.get(name, -1) + 1
            cls = (cls or "SLSLS"[k % 5]) if o.sized else "-"
            sets = [s for s in o.sets[cls] if all(s.get(f) == v for f, v in fixed.items())]
            args = dict(sets[int(rng.integers(len(sets))) if which is None else which % len(sets)])
            args["seed"] = int(rng.integers(1 << 30))
            if o.sized:
                args["size_class"] = cls
            return name, args

        def placed(ingest):
            """(a bot_veil_place of bot 2 on the end of the first beam of the ingest's record 0 that is a hit, the ingest):
            the ingest is drawn again until its record 0 has such a beam."""
            name, n = ingest
            while True:
                one = item(name, cls="S", n=n, **({} if name == "ingest_packets" else dict(stride=751)))
                if name == "ingest_packets":
                    one[1]["clear"] = True
                at = (name, n, one[1]["seed"])
                hit = [k for k in range(4 if name == "ingest_packets" else MR.BEAMS) if beam_of(size, at, k)[2]]
                if hit:
                    return ("bot_veil_place", dict(bot=2, x=None, y=None, at=at, beam=hit[len(hit) // 2], seed=0)), one

        def other_box(args):
            return "tile" if args["box"] != "tile" else "cell"

        ops, paired = [], set()
        for k in range(runs[w]):
            b = b0 + k
            plan = _VEIL_PLAN[b]
            if plan["veil"] is not None:
                ops.append(item("set_bot_veil", which=_VEIL_SETS[plan["veil"]]))
            radius = [a["radius"] for n_, a in ops if n_ == "set_bot_veil"][-1:] or [0]
            sweeps_on = [a["sweeps"] for n_, a in ops if n_ == "set_bot_veil" and a["sweeps"] is not None][-1:] or [False]
            acting, s_acting = radius[0] > 0, radius[0] > 0 and sweeps_on[0]
            for p, pred in enumerate(PREDS):
                again = None
                if pred == "rays":
                    if k % 2 == 0:
                        ops.append(item("set_sweep_filter", which=1 if k % 4 == 0 else 0))
                    ops.append(item("update_rays", which=1 if k % 3 == 2 else 0))
                elif pred == "packets":
                    if plan["packets"] == 1 and acting:
                        place, one = placed(("ingest_packets", 1))
                        ops += [place, one]
                        if "forget" not in paired:
                            paired.add("forget")
                            again = [item("bot_veil_forget", which=1), (one[0], dict(one[1]))]
                    else:                                          # sixteen packets under the veil: drawn again until one of their beams is veiled
                        while True:
                            one = item("ingest_packets", cls="L" if plan["packets"] == 5000 else "S", n=plan["packets"])
                            one[1]["clear"] = True
                            if not acting or plan["packets"] != 16 or SV.SweepVeilModel(_Geo(size), 2, radius[0]).ingest(packets_of(size, one[1]))[0].any():
                                break
                        ops.append(one)
                elif pred == "sweeps":
                    name = "ingest_sweeps_" + plan["form"]
                    cls = "L" if plan["n"] == 65 else "S"
                    if b == len(_VEIL_PLAN) - 1:                       # the table holds what the packet ingest left: no place
                        ops += [item("ingest_sweeps_plain", cls="S", n=1, stride=751), item("veil_state")]
                    if plan.get("graph"):                          # refused once in graph mode, then the ingest proper in graph mode
                        ops += [item("set_sweep_graph", which=0), item("ingest_sweeps_check", cls=cls)]
                    if plan["n"] == 1 and s_acting:
                        ops += list(placed((name, 1)))
                    else:
                        ops.append(item(name, cls=cls, n=plan["n"]))
                    if b == len(_VEIL_PLAN) - 1:
                        again = [item("ingest_packets", cls="S", n=1)]
                        again[0][1]["clear"] = True
                else:
                    if pred == "reset" and acting and "place" not in paired:      # (the restore before it has emptied the table)
                        paired.add("place")
                        ops.append(item("bot_veil_place"))
                    ops.append(item(pred))
                q = order[(b + p) % nq]
                ops.append(item(q))
                if q == "relocalise_groups" and "trails" not in paired:
                    paired.add("trails")
                    n_rot = 45 if ops[-1][1]["n_rot"] != 45 else 8
                    ops.append(("relocalise_trails", dict(trails=1, records=4, stride=42, n_rot=n_rot, box=other_box(ops[-1][1]), radius=2,
                                                          travel=0.6 if ops[-1][1]["travel"] != 0.6 else 0.0, seed=int(rng.integers(1 << 30)), size_class="S")))
                elif q == "relocalise_trails" and "groups" not in paired:
                    paired.add("groups")
                    n_rot = 45 if ops[-1][1]["n_rot"] != 45 else 8
                    ops.append(("relocalise_groups", dict(groups=(4, 1), travel=2.0 if ops[-1][1]["travel"] != 2.0 else 0.0, n_rot=n_rot,
                                                          box=other_box(ops[-1][1]), radius=2, stride=751, seed=int(rng.integers(1 << 30)), size_class="S")))
                elif q == "match" and "match_trails" not in paired:
                    paired.add("match_trails")
                    ops.append(("match_trails", dict(trails=1, records=4, stride=42 if ops[-1][1]["stride"] == 743 else 41,
                                                     radius=2 if ops[-1][1]["radius"] != 2 else 7, travel=4.0, seed=int(rng.integers(1 << 30)), size_class="S")))
                elif q == "match_trails" and "match" not in paired:
                    paired.add("match")
                    ops.append(("match", dict(n=3, stride=743 if ops[-1][1]["stride"] == 42 else 751, radius=2 if ops[-1][1]["radius"] != 2 else 7,
                                              seed=int(rng.integers(1 << 30)), size_class="S")))
                if pred == "sweeps" and plan.get("graph"):
                    ops.append(item("set_sweep_graph", which=1))
                if again:
                    ops += again
        b0 += runs[w]
        out.append(ops)
    return out


def as_literal(ops):
    """The op list as text that evaluates to it."""
    return "[" + ",\n ".join(repr(o) for o in ops) + "]"


# ---- walking a context ----------------------------------------------------------------------------------------------------------------
def same_map(m, model):
    """'' when grid_i8() and counts() of the context are the model's."""
    h, mi = m.counts()
    return differing(dict(grid=m.grid_i8(), hits=h, misses=mi), dict(grid=model.grid, hits=np.array(model.mapo.hits), misses=np.array(model.mapo.misses)),
                     "map")


def walk(m, model, env, ops, tag="", twin=None, every=5, failures=None):
    """The ops in turn on the context and on the model.  After every op (a) the answer is the model's, and a query a checkpoint
    covers answers the same when it is asked again at once; after every writer (b) grid_i8() and counts() are the oracle's and the
    five last-ingest calls answer or refuse as the model says, and so does veil_state (with the veil never switched on: an empty
    table, a total of 0, zero flags); every `every` ops and at the end (c) twin(m, model, env) -- a new context restored
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
            for q in ("last", "veil_state"):
                if not why:
                    said = OPS[q].run(m, {}, env)
                    why = differing(said, OPS[q].expect(model, {}, said), {"last": "last ingest", "veil_state": "veil"}[q])
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
