"""Grid geometries with unequal origins and cell sizes other than 0.05, and the cases the map queries are run on at each of
them.  numpy only; the package is not imported.

Almost every other test builds its grid with res = 0.05 and ox == oy, so a kernel that read ox where it should read oy, or that
is right at 0.05 alone, would pass them all.  Here every family of map queries gets one small case per geometry of GEOMETRIES:
the maps are built in cell space, the poses are cells turned into world coordinates with the geometry under test (off the cell
centre), sweeps and packets come from the CPU sensor (sense_rules) with noise off.  Every input is made on the CPU, so the same
bytes feed the restatement (tests/test_skew_geometry_cpu.py, which also shows that each case tells a swapped or a 0.05 geometry
from the right one) and the device (tests/test_gpu_skew_geometry.py).

A family is a pair (build(name) -> case, restate(case, geom) -> {field: array}): restate runs the family's *_rules restatement on
the case's inputs with any geometry, which is how the CPU test swaps ox and oy.  Where a restatement takes the device's own
rotation tables, restate takes them as `dev`; without, libm's stand in.

Also here: the reach limits of the five calls that have one, in cells, and the metres that lie exactly on them."""
import math

import numpy as np

import assign_rules as AR
import check_rules as CR
import gain_rules as GN
import match_rules as MR
import maze_scenes as MZ
import plan_rules as PR
import reloc_group_rules as GR
import reloc_rules as RR
import sense_rules as SR
import territory_rules as TY
import trail_rules as TR
import view_rules as VR

# name -> (res, ox, oy)
GEOMETRIES = {
    "lop": (0.05, -1.7, 0.95),                 # the usual cell size; origins of opposite sign, 53 cells apart
    "fine": (0.025, 0.4125, -2.7875),          # half-size cells: 3.0 m is 120 cells, beyond several reach limits
    "odd": (0.04, 3.3, -7.14),                 # not a short binary fraction nor 0.05; both origins on half cells
    "far": (0.125, 100.0, -249.9375),          # coarse, exact cells; large unequal origins (f32 pose fields lose bits)
}
NAMES = tuple(GEOMETRIES)
REACH = 60                                     # cells the cases' sweeps are sensed and filtered at (3.0 m at 0.05)
PACKET_REACH, TRAIL_TRAVEL = 40, 30            # cells: the packets' max_dist and the trails' travel
GROUP_STEP, GROUP_TRAVEL = 6, 10               # cells between the sweeps of a group, and the groups' travel


# ---- metres on a reach limit ------------------------------------------------------------------------------------------------------
def reach_metres(cells, res, base=0.0):
    """The largest double t with ceil((base + t) / res) == cells, the arithmetic of every limit check: one step of the last bit
    more is one cell more."""
    t = cells * res - base
    while math.ceil((base + t) / res) > cells:
        t = math.nextafter(t, -math.inf)
    while math.ceil((base + math.nextafter(t, math.inf)) / res) <= cells:
        t = math.nextafter(t, math.inf)
    assert math.ceil((base + t) / res) == cells and math.ceil((base + math.nextafter(t, math.inf)) / res) == cells + 1
    return t


def limit_cells(call, radius=2, window=0):
    """The largest ceil(reach / res) each call accepts (include/quasar_slam.h: rule 5 of sweep matching, T8, V8, G9, J8)."""
    if call in ("match", "trail"):
        return MR.MAX_REACH - 2 - radius - window
    if call == "check":
        return CR.MAX_CELLS - 1
    assert call in ("reloc", "reloc_group")
    return (255 - RR.TILE) // 2 - radius - 1


def reloc_patch_side(reach_m, res, radius):
    """SA of csrc/reloc.hip for a reach in metres (smax, or smax + travel): M = ceil(reach / res) + 1 cells round the tile, and R."""
    return RR.TILE + 2 * (math.ceil(reach_m / res) + 1 + radius)


# ---- poses, sweeps, packets ---------------------------------------------------------------------------------------------------------
def filter_of(res, reach=REACH):
    """The sweep filter of the cases: (two cells, `reach` cells)."""
    return 2 * res, reach_metres(reach, res)


def poses_in(cells, yaw, geom, seed):
    """float32 [n, 3]: a seeded position inside each cell (gx, gy), 0.05 to 0.95 of the cell as reloc_rules.query_poses."""
    res, ox, oy = geom
    rng = np.random.default_rng(seed)
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    fx, fy = rng.uniform(0.05, 0.95, len(c)), rng.uniform(0.05, 0.95, len(c))
    pose = np.stack([ox + (c[:, 0] + fx) * res, oy + (c[:, 1] + fy) * res, np.asarray(yaw, dtype=np.float64)], axis=1).astype(np.float32)
    for k, (gx, gy) in enumerate(c.astype(int).tolist()):                  # (the f32 rounding leaves each pose in its cell)
        assert (SR.cell(float(pose[k, 0]), ox, res), SR.cell(float(pose[k, 1]), oy, res)) == (gx, gy)
    return pose


def pack_sweeps(agent, poses, ranges):
    """uint8 [n, 751]: sweep records with odometry fields 0 and scan_count 181 (protocol.pack_sweeps' bytes)."""
    n = len(poses)
    buf = np.zeros((n, 751), dtype=np.uint8)
    rec = MR.records_of(buf)
    rec["magic"] = b"QSRL"
    rec["agent"], rec["x"], rec["y"], rec["yaw"] = agent, poses[:, 0], poses[:, 1], poses[:, 2]
    rec["scan_count"] = MR.BEAMS
    rec["ranges"] = np.asarray(ranges, dtype=np.float32).reshape(n, MR.BEAMS)
    return buf


def sensed_sweeps(grid, geom, poses, max_range):
    ranges, _ = SR.sense_ranges(grid, *geom, poses, MR.BEAMS, max_range=max_range)
    return pack_sweeps(1, poses, ranges)


def displace(buf, geom, seed, cells=4, steps=3, step=math.pi / 180):
    """The same records with their reported poses moved by whole cells (|.| <= cells) and whole angle steps; (buf, disp)."""
    rng = np.random.default_rng(seed)
    out = buf.copy()
    rec = MR.records_of(out)
    n = len(rec)
    disp = np.stack([rng.integers(-cells, cells + 1, n), rng.integers(-cells, cells + 1, n), rng.integers(-steps, steps + 1, n)], axis=1)
    rec["x"] += (disp[:, 0] * geom[0]).astype(np.float32)
    rec["y"] += (disp[:, 1] * geom[0]).astype(np.float32)
    rec["yaw"] += (disp[:, 2] * step).astype(np.float32)
    return out, disp


SMALL_CELLS = np.array([(3, 3), (64, 2), (1, 66), (66, 66), (30, 30), (45, 20)])


def small_poses(geom, seed=3):
    """Six poses in reloc_rules.small_world(): four near its corners, two inside, headings towards the middle of the grid."""
    yaw = np.arctan2(34 - SMALL_CELLS[:, 1], 34 - SMALL_CELLS[:, 0]) + np.array([0.1, -0.2, 0.3, -0.1, 2.0, 0.4])
    return poses_in(SMALL_CELLS, yaw, geom, seed)


def edge_share(geom, poses, beams, max_range):
    """(edge beams, beams) of the poses: what sense_rules.edge_beams leaves uncompared."""
    e = SR.edge_beams(*geom, poses, beams, max_range)
    return int(e.sum()), int(e.size)


def differs(a, b):
    """The first field in which two restatements' results differ ('' when none does; NaN equals NaN)."""
    if a.keys() != b.keys():
        return "keys"
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            return k
        same = x == y
        if x.dtype.kind == "f":
            same = same | (np.isnan(x) & np.isnan(y))
        if not np.all(same):
            return k
    return ""


def same_records(got, want, fields, tag):
    """Two structured arrays of one dtype: every field with ==, doubles as bits, then every byte (the pads are zero)."""
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, f"{tag}: {f} differs in {len(bad)}, first [{bad[0]}]: {got[f][bad[0]]!r} against {want[f][bad[0]]!r}"
    assert got.tobytes() == want.tobytes(), f"{tag}: bytes differ"


def _fields(arr, names):
    return {f: np.asarray(arr[f]).copy() for f in names}


# ---- sensing -------------------------------------------------------------------------------------------------------------------------
def sensing_case(name):
    geom = GEOMETRIES[name]
    grid = RR.small_world()
    poses = small_poses(geom)
    smin, smax = filter_of(geom[0])
    # a drive of packets through the open middle, every sensor in turn towards a wall
    cells = [(12 + 3 * k, 18 + 2 * k) for k in range(8)]
    ppose = poses_in(cells, np.linspace(-3.0, 3.0, 8), geom, seed=4)
    return dict(name=name, geom=geom, grid=grid, poses=poses, packet_poses=ppose, max_range=smax,
                packet_range=reach_metres(PACKET_REACH, geom[0]))


def sensing_restate(c, geom, dev=None):
    r181, c181 = SR.sense_ranges(c["grid"], *geom, c["poses"], 181, max_range=c["max_range"])
    r4, c4 = SR.sense_ranges(c["grid"], *geom, c["packet_poses"], 4, max_range=c["packet_range"])
    return dict(ranges=r181.view(np.uint32), cells=c181, packet_ranges=r4.view(np.uint32), packet_cells=c4)


# ---- sweep mapping -------------------------------------------------------------------------------------------------------------------
def sweeps_case(name):
    """The sweeps every sweep family shares: sensed in the small world at REACH cells from small_poses."""
    geom = GEOMETRIES[name]
    grid = RR.small_world()
    poses = small_poses(geom)
    smin, smax = filter_of(geom[0])
    return dict(name=name, geom=geom, grid=grid, poses=poses, filt=(smin, smax), buf=sensed_sweeps(grid, geom, poses, smax))


def mapping_restate(c, geom, dev=None):
    """The oracle's update_ray driven beam by beam from the records (as tests/test_gpu_sweeps.py drives it)."""
    from oracle import oracle as orc
    from walk_ops import sweep_beams
    o = orc.OracleMapper(len(c["grid"]), *geom, 0.0)
    o.update_rays(*sweep_beams(MR.records_of(c["buf"]), smin=c["filt"][0], smax=c["filt"][1]))
    return dict(grid=o.grid.copy(), hits=o.hits.copy(), misses=o.misses.copy())


# ---- matching ------------------------------------------------------------------------------------------------------------------------
MATCH_PARAMS = dict(window=4, angle_steps=3)
TRAIL_PARAMS = dict(window=4, angle_steps=3, min_hits=4)
TRAIL_K = 10


def matching_case(name):
    c = sweeps_case(name)
    geom = c["geom"]
    res = geom[0]
    c["queries"], c["disp"] = displace(c["buf"], geom, seed=6)
    # two trails of TRAIL_K packets, a cell a step, displaced rigidly about their last pose
    starts, yaws, disps = [(14, 16), (52, 42)], [0.3, 2.5], [(2, -3, 1), (-4, 1, -2)]
    pk = []
    for (gx, gy), yaw, disp in zip(starts, yaws, disps):
        first = poses_in([(gx, gy)], [yaw], geom, seed=gx).astype(np.float64)[0]
        k = np.arange(TRAIL_K)
        true = np.stack([first[0] + k * res * math.cos(yaw), first[1] + k * res * math.sin(yaw), yaw + 0.05 * k], axis=1)
        true = true.astype(np.float32)
        max_dist = reach_metres(PACKET_REACH, res)
        ranges, _ = SR.sense_ranges(c["grid"], *geom, true, 4, max_range=max_dist)
        rep = TR.displaced(true.astype(np.float64), disp, res)
        pk.append(TR.pack(np.ones(TRAIL_K, int), rep[:, 0], rep[:, 1], rep[:, 2], ranges))
    c.update(packets=np.concatenate(pk), gsize=[TRAIL_K, TRAIL_K], min_dist=0.5 * res, max_dist=reach_metres(PACKET_REACH, res),
             travel=TRAIL_TRAVEL * res)
    return c


def matching_expected(c, geom, rot=None, trail_rot=None):
    """(field uint8 [size, size], MATCH_DTYPE [n], TRAIL_DTYPE [groups], the trails' rot_out); rot, trail_rot: the device's."""
    grid = c["grid"]
    m = MR.match(grid, geom, c["queries"], MR.params(**MATCH_PARAMS), None, *c["filt"], rot=rot)
    t, t_rot = TR.match(grid, geom, c["packets"], c["gsize"], TRAIL_PARAMS, c["travel"], None, rot=trail_rot,
                        min_dist=c["min_dist"], max_dist=c["max_dist"])
    return MR.field(grid, 2), m, t, t_rot


def matching_restate(c, geom, dev=None):
    field, m, t, _ = matching_expected(c, geom)
    out = dict(field=field)
    out.update({"match_" + f: v for f, v in _fields(m, MR.FIELDS).items()})
    out.update({"trail_" + f: v for f, v in _fields(t, TR.FIELDS).items()})
    return out


# ---- contradiction check -------------------------------------------------------------------------------------------------------------
def check_case(name):
    """The sensed sweeps (they agree with the map) and the same displaced by up to 8 cells (they do not)."""
    c = sweeps_case(name)
    moved, _ = displace(c["buf"], c["geom"], seed=8, cells=8, steps=12)
    c["records"] = np.concatenate([c["buf"], moved])
    c["params"] = dict(tol=2.0 * c["geom"][0])
    return c


def check_expected(c, geom, sincos=None):
    """(CHECK_DTYPE [n], classes uint8 [n, 181]); sincos: the device's (sin_yaw, cos_yaw) [n, 2]."""
    return CR.check(c["grid"], geom, c["records"], dict(c["params"]), None, *c["filt"], sincos=sincos)


def check_restate(c, geom, dev=None):
    chk, cls = check_expected(c, geom)
    out = _fields(chk, CR.FIELDS)
    out["classes"] = cls
    return out


# ---- relocalisation ------------------------------------------------------------------------------------------------------------------
RELOC_PARAMS = dict(n_rot=24)
WORLD_PARAMS = dict(n_rot=8, box=(16, 20, 130, 110))


def reloc_case(name):
    """The small world's sweeps, two groups of two sweeps GROUP_STEP cells apart in it, and two sweeps in the three-room world."""
    c = sweeps_case(name)
    geom = c["geom"]
    res = geom[0]
    smax = c["filt"][1]
    G = GR.build_groups(c["grid"], geom, c["poses"][4:6], 2, GROUP_STEP * res, seed=5)
    c.update(group_poses=G, group_buf=sensed_sweeps(c["grid"], geom, G.reshape(-1, 3), smax), gsize=[2, 2], travel=GROUP_TRAVEL * res)
    world = RR.world()
    wposes, wcells = RR.query_poses(world, geom, 2, seed=5)
    c.update(world=world, world_poses=wposes, world_cells=wcells, world_buf=sensed_sweeps(world, geom, wposes, smax))
    return c


def reloc_expected(c, geom):
    """(RELOC_DTYPE of the small world's sweeps, of the three-room world's, GROUP_DTYPE of the groups)."""
    return (RR.reloc(c["grid"], geom, c["buf"], RELOC_PARAMS, None, *c["filt"]),
            RR.reloc(c["world"], geom, c["world_buf"], WORLD_PARAMS, None, *c["filt"]),
            GR.reloc_groups(c["grid"], geom, c["group_buf"], c["gsize"], None, c["travel"], RELOC_PARAMS, None, *c["filt"]))


def reloc_restate(c, geom, dev=None):
    small, world, group = reloc_expected(c, geom)
    out = {"small_" + f: v for f, v in _fields(small, RR.FIELDS).items()}
    out.update({"world_" + f: v for f, v in _fields(world, RR.FIELDS).items()})
    out.update({"group_" + f: v for f, v in _fields(group, GR.FIELDS).items()})
    return out


# ---- paths ---------------------------------------------------------------------------------------------------------------------------
PLAN_SIZE, PLAN_SCENE, PLAN_SPARE = 68, (1, 67, 3), (1, 66, 13, 66)
PLAN_SNAP = 10


def paths_case(name):
    """The serpentine on 68 cells with a spare corridor.  Starts and goals are world points off the cell centre; the last two
    requests start in an UNKNOWN cell beside the corridor and aim into the spare corridor."""
    geom = GEOMETRIES[name]
    res, ox, oy = geom
    plain = MZ.serpentine(PLAN_SIZE, *PLAN_SCENE)
    path = MZ.corridor_order(plain[0], (PLAN_SCENE[0], PLAN_SCENE[0]))
    grid, rays = MZ.add_run(plain, *PLAN_SPARE)
    n = len(path)
    off = (10, 2)                                                          # UNKNOWN; (10, 1) is one cell away
    assert grid[off[1], off[0]] == MZ.UNKNOWN and grid[1, 10] == MZ.FREE
    cells = [(path[-1], path[0]), (path[0], path[-1]), (path[n // 3], path[2 * n // 3]), (path[n // 2], path[n // 2]),
             (off, path[n // 5]), (path[n // 2], PLAN_SPARE[:2])]
    at = lambda cs, seed: poses_in(cs, np.zeros(len(cs)), geom, seed).astype(np.float64)[:, :2]
    return dict(name=name, geom=geom, grid=grid, rays=rays, starts=at([s for s, _ in cells], 11), goals=at([g for _, g in cells], 12),
                snap_goal=at([off], 13)[0])


def paths_expected(c, geom):
    """(plan_rules.plan's dict of every request, the distance field of snap_goal -- all unreached where it does not snap)."""
    res, ox, oy = geom
    t = PR.traversable(c["grid"], 0)
    graph = PR.move_graph(t)
    plans = [PR.plan(t, tuple(s), tuple(g), res, ox, oy, snap_radius=PLAN_SNAP, lookahead=200, graph=graph)
             for s, g in zip(c["starts"], c["goals"])]
    cell = PR.snap(t, tuple(c["snap_goal"]), res, ox, oy, PLAN_SNAP)
    field = np.full(t.shape, PR.INF, dtype=np.uint32) if cell is None else PR.field_scipy(t, cell, graph)
    return plans, field


def paths_restate(c, geom, dev=None):
    plans, field = paths_expected(c, geom)
    return dict(status=np.array([p["status"] for p in plans]), cell=np.array([p["cell"] for p in plans]),
                xy=np.array([p["xy"] for p in plans]), cost=np.array([p["cost"] for p in plans], dtype=np.int64),
                path_len=np.array([len(p["path"]) for p in plans]),
                paths=np.array([xy for p in plans for xy in p["path"]], dtype=np.int64).reshape(-1, 2), field=field)


# ---- targets -------------------------------------------------------------------------------------------------------------------------
TARGET_SIZE = 64
TARGET_SEP = 4                                 # cells: the separation of the greedy calls


def targets_case(name):
    """A FREE room [6, 58)^2 in UNKNOWN space whose ring of frontier cells is cut into five unequal arcs by OCCUPIED cells, and
    three bots off the cell centre; the arcs' centroids lie off their cells, some of them on non-traversable ones."""
    geom = GEOMETRIES[name]
    cuts = [(6, 20), (30, 6), (57, 12), (57, 45), (22, 57)]
    grid, rays = MZ.room(TARGET_SIZE, 6, 58, cuts)
    bots = poses_in([(12, 14), (44, 40), (30, 50)], np.zeros(3), geom, seed=21).astype(np.float64)[:, :2]
    return dict(name=name, geom=geom, grid=grid, rays=rays, bots=bots, sep=TARGET_SEP * geom[0])


PATH_KEYS = ("idx", "xy", "cost", "status", "waypoint_cell", "waypoint")
TERRITORY_KEYS = ("owner", "cost", "area", "box", "idx", "xy", "cost_b", "status", "waypoint_cell", "waypoint", "centroid_owner")


def targets_expected(c, geom):
    """dict: centroids float64 [k, 2] (gain_rules, from the grid), greedy = (idx, xy) of qs_frontier_targets' rule, and the dicts
    of assign_rules.assign (path), gain_rules.assign (gain) and territory_rules.targets (territory)."""
    from test_gpu_frontier_targets import oracle_targets
    res, ox, oy = geom
    grid, bots, sep = c["grid"], c["bots"], c["sep"]
    cl, size = GN.clusters(grid, 3)
    cents = np.array(GN.centroids(cl, size, res, ox, oy), dtype=np.float64).reshape(-1, 2)
    _, gain, _ = GN.frontier_gain(grid, 3, GN.DEFAULT_RANGE)
    return dict(centroids=cents, greedy=oracle_targets(cents, [tuple(b) for b in bots.tolist()], sep),
                path=AR.assign(grid, cents, bots, res, ox, oy, sep), gain_of=gain,
                gain=GN.assign(grid, cents, gain, bots, res, ox, oy, sep, bias=GN.DEFAULT_BIAS, top_k=32),
                territory=TY.targets(grid, cents, bots, res, ox, oy))


def targets_restate(c, geom, dev=None):
    e = targets_expected(c, geom)
    out = dict(centroids=e["centroids"], greedy_idx=e["greedy"][0], greedy_xy=e["greedy"][1])
    out.update({"path_" + k: np.asarray(e["path"][k]) for k in PATH_KEYS})
    out.update({"gain_" + k: np.asarray(e["gain"][k]) for k in GN.KEYS})
    out.update({"territory_" + k: np.asarray(e["territory"][k]) for k in TERRITORY_KEYS})
    return out


# ---- view ----------------------------------------------------------------------------------------------------------------------------
def view_case(name):
    """The small world seen whole in a minified frame (0.6 pixels a cell) and in part in a magnified one (4 pixels a cell), the
    map's middle in the middle of the frame."""
    geom = GEOMETRIES[name]
    res, ox, oy = geom
    grid = RR.small_world()
    size = len(grid)
    frames = []
    for w, h, per_cell in ((80, 60, 0.6), (160, 120, 4.5)):
        scale = per_cell / res
        frames.append(VR.params(w, h, scale, w / 2 - (ox + size * res / 2) * scale, h / 2 + (oy + size * res / 2) * scale,
                                draw_occupied=True))
    assert VR.cell_px(frames[0], res) == 1 and VR.cell_px(frames[1], res) == 4
    return dict(name=name, geom=geom, grid=grid, frames=frames)


def view_restate(c, geom, dev=None):
    return {f"frame{i}": VR.render(p, c["grid"], *geom) for i, p in enumerate(c["frames"])}


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def plumbing_case(name):
    """World values over a 64-cell grid and three cells round it on each axis: seeded ones, and every cell's lower edge."""
    geom = GEOMETRIES[name]
    res, ox, oy = geom
    rng = np.random.default_rng(31)
    w = [np.concatenate([rng.uniform(o - 3 * res, o + 67 * res, 200), o + np.arange(-3, 68) * res]) for o in (ox, oy)]
    return dict(name=name, geom=geom, size=64, w=w)


def plumbing_restate(c, geom, dev=None):
    res, ox, oy = geom
    return {f"axis{a}": np.array([PR.world_to_grid(float(v), o, res) for v in c["w"][a]], dtype=np.int64) for a, o in ((0, ox), (1, oy))}


FAMILIES = {
    "sensing": (sensing_case, sensing_restate),
    "sweep mapping": (sweeps_case, mapping_restate),
    "matching": (matching_case, matching_restate),
    "contradiction check": (check_case, check_restate),
    "relocalisation": (reloc_case, reloc_restate),
    "paths": (paths_case, paths_restate),
    "targets": (targets_case, targets_restate),
    "view": (view_case, view_restate),
    "plumbing": (plumbing_case, plumbing_restate),
}


# ---- the reach limit: a 128-cell room --------------------------------------------------------------------------------------------------
LIMIT_SIZE = 128
LIMIT_GEOMETRIES = ("fine", "lop")


def limit_room():
    """128 x 128: walls on the rows and columns 2 and 125, FREE inside, pillars and two short bars (nothing symmetric); at `fine`
    it is 3.2 m across, so that beams of limit length end inside the map."""
    g = np.full((LIMIT_SIZE, LIMIT_SIZE), -1, dtype=np.int8)
    g[2:126, 2:126] = 100
    g[3:125, 3:125] = 0
    g[30:32, 40:42] = 100
    g[80, 25] = g[95, 100] = g[20, 90] = g[60, 64] = 100
    g[50, 70:85] = 100
    g[90:104, 45] = 100
    return g


LIMIT_CELLS = np.array([(10, 12), (116, 20), (60, 110), (100, 70)])


def limit_poses(geom, n=3):
    yaw = np.arctan2(64 - LIMIT_CELLS[:, 1], 64 - LIMIT_CELLS[:, 0]) + np.array([0.2, -0.3, 0.1, 1.4])
    return poses_in(LIMIT_CELLS[:n], yaw[:n], geom, seed=17)
