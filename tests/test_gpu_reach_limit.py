"""The accepted side of the reach limit: match_sweeps, match_trails, check_sweeps, relocalise_sweeps and relocalise_groups with the
largest reach each accepts (include/quasar_slam.h: rule 5 of sweep matching, T8, V8, G9, J8), in metres that lie on the limit to
the last bit (skew_geometry.reach_metres; the arithmetic is shown on the CPU in tests/test_skew_geometry_cpu.py).  The map is a
128-cell room with pillars at `fine` (0.025 m cells: 3.2 m across, so beams of limit length end inside the map) and at `lop`
(0.05 m, unequal origins).  Every output equals the call's restatement, every field with == and doubles as bits; the same call
one cell of reach further is refused with the text the other tests match.

At the relocaliser's limit the scoring kernels hold a patch of SA = 254 cells a side in rows of 272 bytes: two LDS regions of
69 088 bytes, and 16-bit patch offsets up to 64 428.  A module of its own, so that it can be run alone."""
import math

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import check_rules as CR
import match_rules as MR
import maze_scenes as MZ
import reloc_group_rules as GR
import reloc_rules as RR
import sense_rules as SR
import skew_geometry as SK
import trail_rules as TR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
GEOMETRY = pytest.mark.parametrize("name", SK.LIMIT_GEOMETRIES)
RADIUS = pytest.mark.parametrize("radius", [2, 7])
TRAIL_K = 12


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def rooms(pkg):
    """name -> (mapper, grid): the room painted at each geometry; the packets' filter is (half a cell, 40 cells]."""
    out = {}
    grid = SK.limit_room()
    for name in SK.LIMIT_GEOMETRIES:
        geom = SK.GEOMETRIES[name]
        m = pkg.QuasarMapper(len(grid), *geom, min_dist=0.5 * geom[0], max_dist=SK.reach_metres(SK.PACKET_REACH, geom[0]))
        MZ.paint(m, RR.paint_rays(grid), *geom)
        assert (m.grid_i8() == grid).all()
        out[name] = (m, grid)
    yield out
    for m, _ in out.values():
        m.close()


def _sweeps(grid, geom, cells, n=3):
    """n sweeps sensed in the room at `cells` cells of range, their filter, and that range in metres."""
    smax = SK.reach_metres(cells, geom[0])
    assert math.ceil(smax / geom[0]) == cells and SR.check_params(geom[0], smax)
    poses = SK.limit_poses(geom, n)
    buf = SK.sensed_sweeps(grid, geom, poses, smax)
    far = MR.records_of(buf)["ranges"].max(axis=1)
    return buf, (2 * geom[0], smax), far


@GEOMETRY
@pytest.mark.parametrize("radius", [0, 2, 7])
def test_match_sweeps_at_the_limit(pkg, rooms, name, radius):
    """Radius 0 with window 0 is the widest patch there is: 125 cells of reach, 253 cells a side, the one shape whose rows go
    unpadded (window_match.h: wm_pitch) and whose 16-bit patch offsets are fullest."""
    m, grid = rooms[name]
    geom = SK.GEOMETRIES[name]
    res = geom[0]
    cells = SK.limit_cells("match", radius)
    buf, filt, far = _sweeps(grid, geom, cells)
    queries, _ = SK.displace(buf, geom, seed=9, cells=1, steps=1)
    p = dict(radius=radius, window=0, angle_steps=1)
    assert MR.limit_ok(MR.params(**p), filt[1], res) and not MR.limit_ok(MR.params(**dict(p, window=1)), filt[1], res)
    assert far.max() > (cells - 2) * res and cells + radius + 2 == MR.MAX_REACH       # a beam ends in the patch's last cells
    try:
        m.set_sweep_filter(*filt)
        dev, rot = m.match_sweeps(queries, None, params=p, rotations=True)
        want = MR.match(grid, geom, queries, MR.params(**p), None, *filt, rot=rot)
        SK.same_records(dev, want, MR.FIELDS, f"{name} R {radius}")
        assert (dev["hits"] > 60).all() and (dev["score"] > 0).all()
        with pytest.raises(pkg.QuasarError, match="window is too large"):
            m.match_sweeps(queries, None, params=dict(p, window=1))
        for beyond in (math.nextafter(filt[1], math.inf), SK.reach_metres(cells + 1, res)):
            m.set_sweep_filter(filt[0], beyond)
            with pytest.raises(pkg.QuasarError, match="smax is too large"):
                m.match_sweeps(queries, None, params=p)
    finally:
        m.set_sweep_filter()


@GEOMETRY
@RADIUS
def test_match_trails_at_the_limit(pkg, rooms, name, radius):
    """A drive of 12 packets from cell (10, 12) along (0.6, 0.8) that ends two cells short of `travel` from its first pose."""
    m, grid = rooms[name]
    geom = SK.GEOMETRIES[name]
    res, ox, oy = geom
    cells = SK.limit_cells("trail", radius)
    max_dist = SK.reach_metres(SK.PACKET_REACH, res)
    travel = SK.reach_metres(cells, res, max_dist)
    p = dict(radius=radius, window=0, angle_steps=1, min_hits=1)
    assert TR.limit_ok(TR.params(**p), max_dist, travel, res) and not TR.limit_ok(TR.params(**dict(p, window=1)), max_dist, travel, res)
    length = cells - SK.PACKET_REACH - 2
    t = np.linspace(0.0, length, TRAIL_K)
    true = np.stack([ox + (10.5 + 0.6 * t) * res, oy + (12.5 + 0.8 * t) * res, np.linspace(0.2, 1.6, TRAIL_K)], axis=1).astype(np.float32)
    ranges, _ = SR.sense_ranges(grid, *geom, true, 4, max_range=max_dist)
    pk = TR.pack(np.ones(TRAIL_K, int), true[:, 0], true[:, 1], true[:, 2], ranges)
    dev, rot = m.match_trails(pk, [TRAIL_K], None, travel=travel, params=p, rotations=True)
    want, want_rot = TR.match(grid, geom, pk, [TRAIL_K], p, travel, None, rot=rot, min_dist=0.5 * res, max_dist=max_dist)
    SK.same_records(dev, want, TR.FIELDS, f"{name} R {radius}")
    assert (rot == want_rot).all()
    assert dev["records"][0] == TRAIL_K and dev["hits"][0] >= 8 and dev["score"][0] > 0          # the first record counts: it lies within travel
    with pytest.raises(pkg.QuasarError, match="window is too large"):
        m.match_trails(pk, [TRAIL_K], None, travel=travel, params=dict(p, window=1))
    for beyond in (math.nextafter(travel, math.inf), SK.reach_metres(cells + 1, res, max_dist)):
        with pytest.raises(pkg.QuasarError, match=r"max_dist \+ travel is too large"):
            m.match_trails(pk, [TRAIL_K], None, travel=beyond, params=p)


@GEOMETRY
def test_check_sweeps_at_the_limit(pkg, rooms, name):
    """254 cells of reach (C = 255, the sensor's largest patch too): two true sweeps, and the same two displaced."""
    m, grid = rooms[name]
    geom = SK.GEOMETRIES[name]
    res = geom[0]
    cells = SK.limit_cells("check")
    buf, filt, far = _sweeps(grid, geom, cells)
    moved, _ = SK.displace(buf, geom, seed=10, cells=8, steps=12)
    buf, moved = buf[:2], moved[:2]
    records = np.concatenate([buf, moved])
    p = dict(tol=2.0 * res)
    assert CR.limit_ok(CR.params(res, **p), filt[1], res) and CR.patch_radius(filt[1], res) == CR.MAX_CELLS
    try:
        m.set_sweep_filter(*filt)
        dev, cls = m.check_sweeps(records, None, params=p, classes=True)
        want, wcls = CR.check(grid, geom, records, p, None, *filt, sincos=np.stack([dev["sin_yaw"], dev["cos_yaw"]], axis=1))
        why = CR.differing(dev, want)
        assert why == "", why
        assert dev.tobytes() == want.tobytes() and (cls == wcls).all(), np.argwhere(cls != wcls)[:4].tolist()
        assert (dev["status"][:len(buf)] == CR.OK).all() and (dev["status"][len(buf):] == CR.CONTRADICTS).any()
        for beyond in (math.nextafter(filt[1], math.inf), SK.reach_metres(cells + 1, res)):
            m.set_sweep_filter(filt[0], beyond)
            with pytest.raises(pkg.QuasarError, match="smax is too large"):
                m.check_sweeps(records, None, params=p)
    finally:
        m.set_sweep_filter()


@GEOMETRY
@RADIUS
def test_relocalise_sweeps_at_the_limit(pkg, rooms, name, radius):
    m, grid = rooms[name]
    geom = SK.GEOMETRIES[name]
    res = geom[0]
    cells = SK.limit_cells("reloc", radius)
    buf, filt, far = _sweeps(grid, geom, cells)
    p = dict(radius=radius, n_rot=8)
    # reloc_setup and reloc_prepare restated: M = ceil(smax / res) + 1, SA = 16 + 2 (M + R), rows of 16 x (an odd number) bytes
    M = math.ceil(filt[1] / res) + 1
    SA = 16 + 2 * (M + radius)
    pitch = (SA + 15) & ~15
    pitch += 16 * (1 - (pitch >> 4) % 2)
    assert (SA, pitch) == (254, 272) and (M + (M + radius)) * pitch + (M + (M + radius)) < 65536
    assert RR.limit_ok(RR.params(**p), filt[1], res) and far.max() > (cells - 2) * res
    try:
        m.set_sweep_filter(*filt)
        got = m.relocalise_sweeps(buf, params=p)
        want = RR.reloc(grid, geom, buf, p, None, *filt)
        why = RR.differing(got, want)
        assert why == "", why
        assert (got["status"] == RR.OK).all() and (got["hits"] > 60).all() and (got["score"] > 0).all()
        for beyond in (math.nextafter(filt[1], math.inf), SK.reach_metres(cells + 1, res)):
            m.set_sweep_filter(filt[0], beyond)
            with pytest.raises(pkg.QuasarError, match="smax is too large"):
                m.relocalise_sweeps(buf, params=p)
    finally:
        m.set_sweep_filter()


@GEOMETRY
@RADIUS
def test_relocalise_groups_at_the_limit(pkg, rooms, name, radius):
    """Two groups of two sweeps of 60 cells' range; the second sweep lies two cells short of `travel` from the first."""
    m, grid = rooms[name]
    geom = SK.GEOMETRIES[name]
    res = geom[0]
    cells = SK.limit_cells("reloc_group", radius)
    smin, smax = SK.filter_of(res)
    travel = SK.reach_metres(cells, res, smax)
    p = dict(radius=radius, n_rot=8)
    assert 16 + 2 * ((math.ceil((smax + travel) / res) + 1) + radius) == 254
    assert GR.limit_ok(RR.params(**p), smax, travel, res)
    step = (cells - SK.REACH - 2) * res
    G = GR.build_groups(grid, geom, SK.limit_poses(geom, 2), 2, step, seed=7)
    apart = np.hypot(*(G[:, 1, :2].astype(np.float64) - G[:, 0, :2].astype(np.float64)).T)
    assert (apart > step - res).all() and (apart <= travel).all(), apart          # (the bots found a way: nobody turned on the spot)
    buf = SK.sensed_sweeps(grid, geom, G.reshape(-1, 3), smax)
    try:
        m.set_sweep_filter(smin, smax)
        got = m.relocalise_groups(buf, [2, 2], travel=travel, params=p)
        want = GR.reloc_groups(grid, geom, buf, [2, 2], None, travel, p, None, smin, smax)
        why = GR.differing(got, want)
        assert why == "", why
        assert (got["status"] == GR.OK).all() and (got["records"] == 2).all() and (got["score"] > 0).all()
        for beyond in (math.nextafter(travel, math.inf), SK.reach_metres(cells + 1, res, smax)):
            with pytest.raises(pkg.QuasarError, match=r"smax \+ travel is too large"):
                m.relocalise_groups(buf, [2, 2], travel=beyond, params=p)
    finally:
        m.set_sweep_filter()
