"""The map view on the device (include/quasar_slam.h: "map view"; csrc/view.hip) against its numpy restatement
(tests/view_rules.py): every frame must equal the rule applied to grid_i8() byte for byte.  Grids are 64 x 64 and 256 x 256 (and
the 512 x 512 golden session), frames at most 300 x 200."""
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import GOLDEN, load_pkg
import view_rules as V

pytestmark = pytest.mark.gpu

RES = 0.05


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def paint(m, grid):
    """Make m's map equal `grid` (-1 / 0 / 100) with the object API: a FREE cell is the first cell of a two-cell ray without a
    hit, an OCCUPIED cell a zero-length ray with one."""
    gy, gx = np.nonzero(grid == 0)
    cx, cy = m.ox + (gx + 0.5) * m.res, m.oy + (gy + 0.5) * m.res
    if len(gx):
        m.update_rays(cx, cy, cx + m.res, cy, np.zeros(len(gx), dtype=np.uint8))
    gy, gx = np.nonzero(grid == 100)
    cx, cy = m.ox + (gx + 0.5) * m.res, m.oy + (gy + 0.5) * m.res
    if len(gx):
        m.update_rays(cx, cy, cx, cy, np.ones(len(gx), dtype=np.uint8))
    assert (m.grid_i8() == grid).all()


def random_grid(size, seed):
    """Random tri-state with structure at every scale: blocks of 16 cells are mostly unknown or mostly known."""
    rng = np.random.default_rng(seed)
    known = np.kron(rng.random((size // 16, size // 16)) < 0.6, np.ones((16, 16), dtype=bool))
    g = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(size, size), p=[0.3, 0.55, 0.15])
    g[~known & (rng.random((size, size)) < 0.97)] = -1
    g[0, 0], g[size - 1, size - 1], g[0, size - 1], g[size - 1, 0] = 0, 100, 0, 0          # the corners are known
    return g


class Map:
    def __init__(self, pkg, grid, dirty_tracking=False):
        size = grid.shape[0]
        self.m = pkg.QuasarMapper(size, RES, -size * RES / 2, -size * RES / 2)
        if dirty_tracking:
            self.m.dirty_tracking(True)
        paint(self.m, grid)
        self.grid = grid

    def check(self, p, zones=None, prims=None):
        """device frame == rule frame; returns the frame."""
        m = self.m
        z = np.zeros(0, dtype=m_P.VIEW_ZONE_DTYPE) if zones is None else zones
        q = np.zeros(0, dtype=m_P.VIEW_PRIM_DTYPE) if prims is None else prims
        got = m.render_view(p["width"], p["height"], p["scale"], p["offset_x"], p["offset_y"], zones=z, prims=q,
                            line_min=p["line_min"], line_max=p["line_max"], bg=p["bg"], line=p["line"], free=p["free"], occ=p["occ"],
                            draw_occupied=p["draw_occupied"], minify=p["minify"])
        want = V.render(p, self.grid, m.res, m.ox, m.oy, *V.from_records(z, q))
        assert got.shape == want.shape and got.dtype == np.uint8
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
        return got


m_P = None


@pytest.fixture(scope="module")
def maps(pkg):
    global m_P
    m_P = pkg.protocol
    one_occ = np.zeros((64, 64), dtype=np.int8)
    one_occ[30, 37] = 100
    out = {"g64": Map(pkg, random_grid(64, 1)), "g256": Map(pkg, random_grid(256, 2), dirty_tracking=True),
           "unknown": Map(pkg, np.full((64, 64), -1, dtype=np.int8)), "one_occ": Map(pkg, one_occ)}
    yield out
    for v in out.values():
        v.m.close()


def zones_arr(items):
    a = np.zeros(len(items), dtype=m_P.VIEW_ZONE_DTYPE)
    for i, (box, color) in enumerate(items):
        a["box"][i] = box
        a["color"][i, :3] = color
    return a


def prims_arr(items):
    a = np.zeros(len(items), dtype=m_P.VIEW_PRIM_DTYPE)
    for i, (kind, size, color, x0, y0, x1, y1) in enumerate(items):
        a[i] = (x0, y0, x1, y1, kind, size, tuple(color) + (0,), 0)
    return a


def world(p, px, py):
    """World point whose screen point is the middle of pixel (px, py)."""
    return (px + 0.5 - p["offset_x"]) / p["scale"], (p["offset_y"] - py - 0.5) / p["scale"]


# ---- magnified views: cell_px in {2, 3, 5, 25} -------------------------------------------------------------------------------
MAGNIFIED = [
    ("g64", 100, 80, 100.0, 50, 40),                 # cell_px 5, the reference's scale
    ("g64", 100, 80, 47.3, 13.5, 70.25),             # cell_px 2: single pixels; fractional offsets
    ("g64", 37, 53, 163.7, -20.5, 95.0),             # cell_px 8, negative offset, odd frame
    ("g64", 100, 80, 60.0, 50, 40),                  # cell_px 3 (res * scale == 3 up to rounding)
    ("g64", 100, 80, 79.9, 50.5, 39.5),              # cell_px 3 with gaps between the squares (3.995 px per cell)
    ("g64", 64, 64, 500.0, 700.3, -650.1),           # cell_px 25, the map's lower left corner region, row 0 from negative values
    ("g64", 63, 40, 100.0, 31.5, 20.0),
    ("g64", 65, 40, 100.0, 32.5, 20.0),
    ("g64", 257, 3, 100.0, 128.5, 1.5),              # the map is narrower than the frame
    ("g64", 1, 1, 100.0, 0.5, 0.5),
    ("g64", 1, 1, 500.0, -3.0, 7.0),
    ("g64", 100, 80, 100.0, 250.0, 40.0),            # partly off the map (the map ends inside the frame)
    ("g64", 100, 80, 100.0, 5000.0, -3000.0),        # wholly off the map
    ("g64", 100, 80, 100.0, -159.4, 0.3),            # screen values in (-1, 0) reach column / row 0
    ("g256", 300, 200, 100.0, 150.0, 100.0),
    ("g256", 300, 200, 40.0, -200.7, 455.2),         # cell_px 2 on the larger grid, the map's edge region
    ("g256", 129, 200, 500.0, 3200.0, -3100.0),      # a corner of the 256 grid at cell_px 25
]


@pytest.mark.parametrize("case", MAGNIFIED, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("draw_occupied", [False, True])
def test_magnified_views(maps, case, draw_occupied):
    name, w, h, scale, offx, offy = case
    p = V.params(w, h, scale, offx, offy, draw_occupied=draw_occupied)
    assert V.cell_px(p, RES) >= 2
    maps[name].check(p)


def test_magnified_cases_cover_the_cell_sizes():
    assert {V.cell_px(V.params(c[1], c[2], c[3]), RES) for c in MAGNIFIED} >= {2, 3, 5, 25}


# ---- minified views: res * scale in {1.99, 1.0, 0.37, 1/16, 0.0005} -----------------------------------------------------------
CELL_SCALES = (1.99, 1.0, 0.37, 1.0 / 16, 0.0005)


@pytest.mark.parametrize("cell_scale", CELL_SCALES)
@pytest.mark.parametrize("name", ["g64", "g256"])
@pytest.mark.parametrize("draw_occupied", [False, True])
def test_minified_views(maps, name, cell_scale, draw_occupied):
    scale = cell_scale / RES
    size = maps[name].grid.shape[0]
    span = size * cell_scale                                        # the map's extent in pixels
    views = [(300, 200, 150.0, 100.0),                              # the map's middle in the frame's middle
             (300, 200, 40.3 + span / 2, 200.0 - 35.6 - span / 2),  # the lower left corner inside the frame
             (257, 130, span / 2 - 0.6, span / 2 - 0.6),            # the upper left corner of the map at the frame's origin:
             (64, 3, 10.25 - span / 2, 1.5), (65, 70, 33.0, 35.0), (1, 1, 0.5, 0.5)]   # negative values land in column / row 0
    for w, h, offx, offy in views:
        p = V.params(w, h, scale, offx, offy, draw_occupied=draw_occupied)
        assert V.cell_px(p, RES) == 1
        maps[name].check(p)


def test_whole_map_in_one_pixel(maps):
    p = V.params(5, 4, 0.0005 / RES, 2.5, 1.5, draw_occupied=True, line_min=1, line_max=0)
    img = maps["g256"].check(p)
    assert tuple(img[1, 2, :3]) == p["occ"] and (img[0, :, :3] == p["bg"]).all()
    img = maps["g256"].check(dict(p, draw_occupied=False))
    assert tuple(img[1, 2, :3]) == p["free"]


def test_one_occupied_cell_in_a_free_footprint(maps):
    mp = maps["one_occ"]
    p = V.params(40, 30, 0.37 / RES, 20.0, 15.0, line_min=1, line_max=0)
    plain = mp.check(p)
    marked = mp.check(dict(p, draw_occupied=True))
    diff = np.argwhere((plain != marked).any(axis=2))
    assert len(diff) == 1 and tuple(marked[tuple(diff[0])][:3]) == p["occ"] and tuple(plain[tuple(diff[0])][:3]) == p["free"]
    # magnified, the occupied cell is a hole without draw_occupied and a square with it
    p = V.params(100, 80, 100.0, 50.0, 40.0, line_min=1, line_max=0)
    plain, marked = mp.check(p), mp.check(dict(p, draw_occupied=True))
    assert ((plain != marked).any(axis=2)).sum() == 25


def test_unknown_map_and_minify_off(maps):
    for scale in (100.0, 47.3, 20.0, 1.25):
        p = V.params(120, 90, scale, 60.0, 45.0)
        img = maps["unknown"].check(p)
        assert not (img[:, :, :3] == p["free"]).all(axis=2).any()
    for name in ("g64", "g256"):
        p = V.params(120, 90, 20.0, 60.0, 45.0, minify=False, draw_occupied=True)
        img = maps[name].check(p)                                      # below 2 px per cell the reference draws no occupancy
        assert not (img[:, :, :3] == p["free"]).all(axis=2).any() and not (img[:, :, :3] == p["occ"]).all(axis=2).any()
        img = maps[name].check(dict(p, minify=True))
        assert (img[:, :, :3] == p["free"]).all(axis=2).any()
        maps[name].check(dict(p, scale=47.3, minify=False))            # minify does not matter once a cell has 2 pixels


def test_metre_lines_and_colours(maps):
    p = V.params(300, 200, 9.7, 150.3, 99.6, line_min=-20, line_max=20, bg=(1, 2, 3), line=(250, 251, 252), free=(9, 8, 7), occ=(100, 0, 200),
                 draw_occupied=True)
    img = maps["g256"].check(p)
    assert (img[:, :, 3] == 255).all() and (img[:, :, :3] == (250, 251, 252)).all(axis=2).any()
    maps["g256"].check(dict(p, line_min=-3, line_max=-3))
    maps["g256"].check(dict(p, line_min=5, line_max=4))                # no lines
    maps["g64"].check(dict(p, scale=1e-3, line_min=-30000, line_max=30000))       # 60001 lines, all on a few columns


# ---- the golden session, both raycast modes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_view_of_the_ingested_session(pkg, mode):
    g = np.load(os.path.join(GOLDEN, "session_512.npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep, raycast_mode=mode) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        version = m._map_version
        views = [V.params(300, 200, 7.0, 150.0, 100.0, draw_occupied=True),            # the whole 25.6 m map, minified
                 V.params(300, 200, 39.9, 150.0, 100.0), V.params(300, 200, 100.0, 150.0, 100.0, draw_occupied=True),
                 V.params(300, 200, 47.0, 101.5, 77.25)]
        frames = [m.render_view(p["width"], p["height"], p["scale"], p["offset_x"], p["offset_y"], draw_occupied=p["draw_occupied"])
                  for p in views]
        grid = m.grid_i8()
        assert (grid == g["grid"]).all() and m._map_version == version
        for p, got in zip(views, frames):
            assert (got == V.render(p, grid, res, ox, oy)).all()
            assert (got[:, :, :3] == p["free"]).all(axis=2).sum() > 50


# ---- zones -------------------------------------------------------------------------------------------------------------------
def test_zones(maps):
    mp = maps["g64"]
    p = V.params(100, 80, 40.0, 50.0, 40.0)
    a, b, c = (0, 191, 255), (255, 105, 180), (10, 250, 20)
    mp.check(p, zones=zones_arr([]))
    img = mp.check(p, zones=zones_arr([((-0.8, -0.5, 0.4, 0.6), a), ((-0.2, -0.9, 0.9, 0.2), b), ((-0.1, -0.1, 0.3, 0.3), c)]))   # overlapping
    assert (img[:, :, :3] == c).all(axis=2).sum() >= 4 * 15
    x0, y0 = world(p, 10, 20)
    x1, _ = world(p, 11, 20)
    mp.check(p, zones=zones_arr([((x0, y0, x0 + 1e-4, y0 + 1.0), a), ((x0, y0, x0 + 1.0, y0 + 1e-4), b),         # w == 0, h == 0
                                 ((x0, y0, x1, y0 + 1.0), c), ((0.5, 0.5, -0.5, -0.5), a)]))                      # w == 1; inverted
    edges = [((-9.0, -0.2, -1.0, 0.2), a), ((1.0, -0.2, 9.0, 0.2), b), ((-0.2, 0.8, 0.2, 9.0), c), ((-0.2, -9.0, 0.2, -0.8), a),
             ((-9.0, -9.0, 9.0, 9.0), b), ((-1e9, -1.0, 1.0, 1.0), c), ((float("nan"), -1.0, 1.0, 1.0), c),
             ((-1.0, -1.0, float("inf"), 1.0), c), ((-1.25, -1.0, 1.25, 1.0), a), ((30.0, 30.0, 40.0, 40.0), b)]
    mp.check(p, zones=zones_arr(edges))                                 # clipped at each edge, all round, undrawable, off-frame
    for one in edges:
        mp.check(p, zones=zones_arr([one]))
    rng = np.random.default_rng(3)
    many = []
    for i in range(256):
        cx, cy, hw, hh = rng.uniform(-1.5, 1.5), rng.uniform(-1.2, 1.2), rng.uniform(0.0, 0.6), rng.uniform(0.0, 0.6)
        many.append(((cx - hw, cy - hh, cx + hw, cy + hh), tuple(int(v) for v in rng.integers(0, 256, 3))))
    maps["g256"].check(V.params(300, 200, 90.0, 150.0, 100.0), zones=zones_arr(many))
    mp.check(V.params(37, 53, 20.0, 18.5, 26.5), zones=zones_arr(many))


# ---- primitives ----------------------------------------------------------------------------------------------------------------
def random_prims(p, n, seed):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n):
        kind = int(rng.integers(0, 3))
        px, py = rng.uniform(-20, p["width"] + 20), rng.uniform(-20, p["height"] + 20)
        x0, y0 = world(p, px, py)
        x1, y1 = world(p, px + rng.uniform(-60, 60), py + rng.uniform(-60, 60))
        items.append((kind, int(rng.integers(1, 17)), tuple(int(v) for v in rng.integers(0, 256, 3)), x0, y0, x1, y1))
    return prims_arr(items)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000])
def test_primitive_counts(maps, n):
    p = V.params(300, 200, 100.0, 150.0, 100.0)
    maps["g256"].check(p, prims=random_prims(p, n, 10 + n))


def test_primitive_edges(maps):
    mp = maps["g64"]
    p = V.params(100, 80, 100.0, 50.0, 40.0)
    S, Q, L = V.POINT, V.SQUARE, V.SEGMENT
    col = lambda i: ((37 * i) % 256, (91 * i + 5) % 256, (13 * i + 100) % 256)
    x, y = world(p, 40, 30)
    pile = [(i % 3, 1 + i % 5, col(i), x, y, x, y) for i in range(200)]              # many primitives on one pixel: the last wins
    img = mp.check(p, prims=prims_arr(pile))
    assert tuple(img[30, 40, :3]) == col(199)
    squares = []
    for i, (px, py) in enumerate([(0, 0), (99, 0), (0, 79), (99, 79), (50, 0), (50, 79), (0, 40), (99, 40), (-3, -3), (102, 83), (-40, 40),
                                  (50, 40)]):
        for size in (1, 2, 7, 8, 63, 64):
            squares.append((Q, size, col(7 * i + size), *world(p, px, py), 0.0, 0.0))
    mp.check(p, prims=prims_arr(squares))
    for one in squares[::5]:
        mp.check(p, prims=prims_arr([one]))
    cx, cy = 50, 40
    octants = []
    for i, (dx, dy) in enumerate([(30, 0), (30, 11), (30, 30), (11, 30), (0, 30), (-11, 30), (-30, 30), (-30, 11), (-30, 0), (-30, -11),
                                  (-30, -30), (-11, -30), (0, -30), (11, -30), (30, -30), (30, -11), (0, 0), (1, 0), (0, -1), (29, 30)]):
        octants.append((L, 1, col(i), *world(p, cx, cy), *world(p, cx + dx, cy + dy)))
    mp.check(p, prims=prims_arr(octants))
    for one in octants:
        mp.check(p, prims=prims_arr([one]))
    outside = [(L, 1, col(1), *world(p, -50, 10), *world(p, 170, 60)), (L, 1, col(2), *world(p, 20, -300), *world(p, 70, 500)),
               (L, 1, col(3), *world(p, -50, -10), *world(p, 170, -60)), (L, 1, col(4), *world(p, -10, 100), *world(p, 60, -20)),
               (L, 1, col(5), *world(p, 130, 10), *world(p, 170, 60))]                 # both ends off-frame: crossing and missing
    img = mp.check(p, prims=prims_arr(outside))
    assert (img[:, :, :3] == col(1)).all(axis=2).sum() >= 95
    far = [(L, 1, col(6), *world(p, 10, 10), *world(p, 10 + 10 ** 7, 10 + 4 * 10 ** 6)),
           (L, 1, col(7), *world(p, 10 - 10 ** 7, 70 - 10 ** 6), *world(p, 10, 70)),
           (L, 1, col(8), *world(p, -(2 ** 30) + 10, 40), *world(p, 2 ** 30 - 10, 41))]  # the longest drawable segment
    img = mp.check(p, prims=prims_arr(far))
    assert (img[:, :, :3] == col(6)).all(axis=2).sum() >= 88
    nan, inf = float("nan"), float("inf")
    bad = [(S, 1, col(9), nan, 0.0, 0.0, 0.0), (S, 1, col(9), 0.0, inf, 0.0, 0.0), (Q, 8, col(9), -inf, 0.0, 0.0, 0.0),
           (Q, 8, col(9), 0.0, nan, 0.0, 0.0), (L, 1, col(9), 0.0, 0.0, nan, 0.0), (L, 1, col(9), 0.0, 0.0, 0.0, inf),
           (L, 1, col(9), inf, 0.0, 0.1, 0.1), (L, 1, col(9), 0.0, 0.0, 1e300, 0.0), (S, 1, col(9), 1e7 + 5e6, 0.0, 0.0, 0.0),
           (L, 1, col(9), 0.0, 0.0, 2.0 ** 30 / 100.0, 0.0)]
    img = mp.check(p, prims=prims_arr(bad))
    assert not (img[:, :, :3] == col(9)).all(axis=2).any()                              # none of them is drawn
    mp.check(p, prims=prims_arr(bad + octants + squares[:12]))
    mp.check(V.params(1, 1, 100.0, 0.5, 0.5), prims=prims_arr(octants + squares))


# ---- entry points, repeatability, read-only --------------------------------------------------------------------------------
def test_host_entry_equals_device_entry_and_repeats(maps):
    mp = maps["g256"]
    m = mp.m
    for p in (V.params(300, 200, 100.0, 150.0, 100.0, draw_occupied=True), V.params(257, 131, 7.4, 128.5, 65.5), V.params(64, 64, 47.3, 3.5, 60.25)):
        prims = random_prims(p, 300, 77)
        zones = zones_arr([((-1.0, -1.0, 0.5, 0.25), (0, 191, 255)), ((-0.25, -0.5, 1.0, 1.0), (255, 105, 180))])
        kw = dict(zones=zones, prims=prims, draw_occupied=p["draw_occupied"])
        a = m.render_view(p["width"], p["height"], p["scale"], p["offset_x"], p["offset_y"], **kw)
        b = m.render_view(p["width"], p["height"], p["scale"], p["offset_x"], p["offset_y"], **kw)
        d = torch.zeros(p["height"] * p["width"] * 4, dtype=torch.uint8, device="cuda")
        assert m.render_view(p["width"], p["height"], p["scale"], p["offset_x"], p["offset_y"], d_out=d, **kw) is None
        m.sync()
        assert (a == b).all() and (d.cpu().numpy().reshape(a.shape) == a).all()
        assert (a == V.render(p, mp.grid, m.res, m.ox, m.oy, *V.from_records(zones, prims))).all()


def test_a_call_changes_nothing(maps):
    m = maps["g256"].m                                                  # dirty tracking is on for this one
    before = (m.checkpoint(), m.counters(), m.dirty_blocks(), m._map_version, m.zone(1))
    assert before[2][0] > 0
    for p in (V.params(300, 200, 100.0, 150.0, 100.0), V.params(300, 200, 7.4, 150.0, 100.0, draw_occupied=True)):
        m.render_view(p["width"], p["height"], p["scale"], p["offset_x"], p["offset_y"], prims=random_prims(p, 100, 5),
                      zones=zones_arr([((-1.0, -1.0, 1.0, 1.0), (1, 2, 3))]), draw_occupied=p["draw_occupied"])
    after = (m.checkpoint(), m.counters(), m.dirty_blocks(), m._map_version, m.zone(1))
    assert before[0] == after[0] and before[1] == after[1] and before[2:] == after[2:]


def test_view_through_mapview_frame(pkg, maps):
    mp = maps["g64"]
    view = pkg.MapView(100, 80)
    view.zoom(1.15)
    view.pan(-7, 3.5)
    clouds = {1: {"front": [(0.1 * i - 1.0, 0.3) for i in range(20)], "left": [(0.0, 0.0), (-0.5, 0.5)]}, 2: {"right": [(0.4, -0.4)]},
              5: {"back": [(0.2, 0.2)]}}
    paths = {1: ([-1.0, -0.5, 0.2, 0.9], [-0.6, 0.1, 0.0, 0.7]), 5: ([0.0, 0.1], [0.5, 0.6])}
    args = dict(zone_boxes={1: (-0.9, -0.6, 0.2, 0.4), 2: (0.0, -0.5, 0.8, 0.3)}, point_clouds=clouds, paths=paths,
                bot_states={1: {"x": -0.3, "y": -0.2, "online": True}}, targets={1: (0.7, 0.6)}, closures=[(-0.8, 0.6, 0.1, 0.65)])
    got = view.frame(mp.m, **args)
    zones, prims = view.lists(**args)
    p = V.params(100, 80, view.scale, view.offset_x, view.offset_y)
    assert (got == V.render(p, mp.grid, mp.m.res, mp.m.ox, mp.m.oy, *V.from_records(zones, prims))).all()


# ---- bad parameters ----------------------------------------------------------------------------------------------------------
def test_bad_parameters_are_refused(pkg, maps):
    m = maps["g64"].m
    good = dict(width=100, height=80, scale=100.0, offset_x=50.0, offset_y=40.0)
    m.render_view(**good)
    nan, inf = float("nan"), float("inf")
    bad = [dict(width=0), dict(width=8193), dict(width=-5), dict(height=0), dict(height=8193), dict(scale=0.0), dict(scale=-1.0),
           dict(scale=nan), dict(scale=inf), dict(scale=1e300), dict(offset_x=nan), dict(offset_x=inf), dict(offset_y=nan),
           dict(offset_y=-inf), dict(line_min=-40000, line_max=40000),
           dict(prims=prims_arr([(3, 1, (1, 1, 1), 0.0, 0.0, 0.0, 0.0)])), dict(prims=prims_arr([(-1, 1, (1, 1, 1), 0.0, 0.0, 0.0, 0.0)])),
           dict(prims=prims_arr([(V.SQUARE, 0, (1, 1, 1), 0.0, 0.0, 0.0, 0.0)])), dict(prims=prims_arr([(V.SQUARE, 65, (1, 1, 1), 0.0, 0.0, 0.0, 0.0)])),
           dict(zones=zones_arr([((0.0, 0.0, 1.0, 1.0), (1, 2, 3))] * 1025))]
    for kw in bad:
        with pytest.raises(pkg.QuasarError, match=r"\(-1\)"):
            m.render_view(**dict(good, **kw))
    L = pkg.load()
    import ctypes as C
    lib = __import__("importlib").import_module(pkg.__name__ + "._lib")
    vp = lib.QsViewParams()
    vp.width, vp.height, vp.scale, vp.offset_x, vp.offset_y, vp.minify = 10, 10, 100.0, 5.0, 5.0, 1
    out = np.zeros((10, 10, 4), dtype=np.uint8)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert L.qs_render_view(m._h, C.byref(vp), None, 0, None, 0, ptr) == 0
    assert L.qs_render_view(m._h, None, None, 0, None, 0, ptr) == -1 and L.qs_render_view(m._h, C.byref(vp), None, 0, None, 0, None) == -1
    assert L.qs_render_view(m._h, C.byref(vp), None, 1, None, 0, ptr) == -1 and L.qs_render_view(m._h, C.byref(vp), None, 0, None, 1, ptr) == -1
    assert L.qs_render_view(None, C.byref(vp), None, 0, None, 0, ptr) == -1 and L.qs_render_view_device(m._h, C.byref(vp), None, 0, None, 0, None) == -1
    m.render_view(**good)                                               # the context still works
