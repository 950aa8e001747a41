"""Every family of map queries on the device at the geometries of tests/skew_geometry.py: unequal origins of either sign, cells of
0.025, 0.04 and 0.125 beside the usual 0.05.  The inputs are the CPU-built cases of that module, the bar is each family's own:
every field of every output equal to the family's restatement, doubles as bits, nothing left out but the beams within 1e-6
cells of a cell boundary (sense_rules.edge_beams; at most 0.1 % of a case's beams, shown on the CPU).
tests/test_skew_geometry_cpu.py shows that each case's result changes when ox and oy are swapped or the cells are 0.05."""
import math

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import assign_rules as AR
import check_rules as CR
import gain_rules as GN
import match_rules as MR
import maze_scenes as MZ
import plan_rules as PR
import reloc_group_rules as GR
import reloc_rules as RR
import sense_rules as SR
import skew_geometry as SK
import territory_rules as TY
import trail_rules as TR
from conftest import load_pkg
from test_gpu_plan_mazes import same_plan

pytestmark = pytest.mark.gpu
GEOMETRY = pytest.mark.parametrize("name", SK.NAMES)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _painted(pkg, grid, geom, rays=None, **kw):
    """A mapper at geom that holds exactly `grid`: painted ray by ray, read back (a raycast test at this geometry already)."""
    m = pkg.QuasarMapper(len(grid), *geom, **kw)
    MZ.paint(m, RR.paint_rays(grid) if rays is None else rays, *geom)
    got = m.grid_i8()
    assert (got == grid).all(), np.argwhere(got != grid)[:8].tolist()
    assert (m.res, m.ox, m.oy) == tuple(geom)
    return m


def _within_one_ulp(got, ref):
    return (np.abs(got - ref) <= np.spacing(np.abs(ref))).all()


# ---- sensing -------------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_sensing(pkg, name):
    c = SK.sensing_case(name)
    geom = c["geom"]
    want = SK.sensing_restate(c, geom)
    with _painted(pkg, c["grid"], geom) as m:
        for poses, beams, rng, key in ((c["poses"], 181, c["max_range"], ""), (c["packet_poses"], 4, c["packet_range"], "packet_")):
            edge = SR.edge_beams(*geom, poses, beams, rng)
            assert edge.sum() <= 0.001 * edge.size
            r, cells = m.sense_ranges(poses, beams, return_cells=True, max_range=rng)
            bad = ~edge & ((r.view(np.uint32) != want[key + "ranges"]) | (cells != want[key + "cells"]))
            assert not bad.any(), f"{beams} beams: {bad.sum()} differ, first (record, beam) {np.argwhere(bad)[0]}"
            assert (cells >= 0).mean() > 0.2                              # the world is seen
            exp_r = np.where(edge, r, want[key + "ranges"].view(np.float32))
            if beams == 181:
                got = m.sense_sweeps(poses, 1, max_range=rng)
                assert got.shape == (len(poses), 751) and got.tobytes() == SK.pack_sweeps(1, poses, exp_r).tobytes()
            else:
                got = m.sense_packets(poses, 1, max_range=rng)
                assert got.tobytes() == TR.pack(np.ones(len(poses), int), poses[:, 0], poses[:, 1], poses[:, 2], exp_r).tobytes()


# ---- sweep mapping -------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_sweep_mapping(pkg, name):
    c = SK.sweeps_case(name)
    want = SK.mapping_restate(c, c["geom"])
    assert (want["grid"] == 100).sum() > 50 and (want["grid"] == 0).sum() > 1000
    for mode in (1, 2):
        with pkg.QuasarMapper(len(c["grid"]), *c["geom"], raycast_mode=mode) as m:
            m.set_sweep_filter(*c["filt"])
            assert m.ingest_sweeps(c["buf"]) == len(c["buf"])
            g = m.grid_i8()
            assert (g == want["grid"]).all(), f"mode {mode}: {(g != want['grid']).sum()} cells differ from the oracle"
            h, mi = m.counts()
            assert (h == want["hits"]).all() and (mi == want["misses"]).all(), f"mode {mode}: counters differ"
            acc, pose = m.last_sweeps()
            assert acc.all() and (pose == c["poses"].astype(np.float64)).all()


# ---- matching ------------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_matching(pkg, name):
    c = SK.matching_case(name)
    geom = c["geom"]
    with _painted(pkg, c["grid"], geom, min_dist=c["min_dist"], max_dist=c["max_dist"]) as m:
        m.set_sweep_filter(*c["filt"])
        field = m.match_field(2)
        dev, rot = m.match_sweeps(c["queries"], None, params=SK.MATCH_PARAMS, rotations=True)
        tdev, trot = m.match_trails(c["packets"], c["gsize"], None, travel=c["travel"], params=SK.TRAIL_PARAMS, rotations=True)
        wfield, want, twant, twant_rot = SK.matching_expected(c, geom, rot, trot)
        assert field.dtype == np.uint8 and (field == wfield).all(), f"{(field != wfield).sum()} field cells differ"
        SK.same_records(dev, want, MR.FIELDS, "match_sweeps")
        SK.same_records(tdev, twant, TR.FIELDS, "match_trails")
        # the rotations the restatements were fed: within one ulp of libm's
        pp = MR.params(**SK.MATCH_PARAMS)
        _, pose = MR.poses_of(MR.records_of(c["queries"]))
        for k in range(len(pose)):
            assert _within_one_ulp(rot[k], MR.rotations_libm(float(pose[k, 2]), pp["angle_steps"], pp["angle_step"])), k
        assert (trot == twant_rot).all() and _within_one_ulp(trot, TR.rot_libm(c["packets"]))
        # the displaced sweeps and trails are found where they were sensed
        assert sum(MR.recovered(dev[k], c["disp"][k]) for k in range(len(dev))) >= 5 and tdev["accepted_match"].all()


# ---- contradiction check -------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_contradiction_check(pkg, name):
    c = SK.check_case(name)
    geom = c["geom"]
    with _painted(pkg, c["grid"], geom) as m:
        m.set_sweep_filter(*c["filt"])
        dev, cls = m.check_sweeps(c["records"], None, params=c["params"], classes=True)
        want, wcls = SK.check_expected(c, geom, np.stack([dev["sin_yaw"], dev["cos_yaw"]], axis=1))
        why = CR.differing(dev, want)
        assert why == "", why
        assert dev.tobytes() == want.tobytes()
        bad = np.argwhere(cls != wcls)
        assert len(bad) == 0, f"{len(bad)} classes differ, first (record, beam) {bad[0]}"
        _, pose = MR.poses_of(MR.records_of(c["records"]))
        ref = np.array([[math.sin(y), math.cos(y)] for y in pose[:, 2]])
        assert _within_one_ulp(np.stack([dev["sin_yaw"], dev["cos_yaw"]], axis=1), ref)
        n = len(c["buf"])
        assert (dev["status"][:n] == CR.OK).all() and (dev["status"][n:] == CR.CONTRADICTS).sum() >= 3


# ---- relocalisation ------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_relocalisation(pkg, name):
    c = SK.reloc_case(name)
    geom = c["geom"]
    res, ox, oy = geom
    small, world, group = SK.reloc_expected(c, geom)
    with _painted(pkg, c["grid"], geom) as m:
        m.set_sweep_filter(*c["filt"])
        got = m.relocalise_sweeps(c["buf"], params=SK.RELOC_PARAMS)
        why = RR.differing(got, small)
        assert why == "", why
        # x comes from ox and gx, y from oy and gy, each on its own
        assert (got["x"] == ox + (got["gx"] + 0.5) * res).all() and (got["y"] == oy + (got["gy"] + 0.5) * res).all()
        grp = m.relocalise_groups(c["group_buf"], c["gsize"], travel=c["travel"], params=SK.RELOC_PARAMS)
        why = GR.differing(grp, group)
        assert why == "", why
        assert (grp["x"] == ox + (grp["gx"] + 0.5) * res).all() and (grp["y"] == oy + (grp["gy"] + 0.5) * res).all()
    with _painted(pkg, c["world"], geom) as m:
        m.set_sweep_filter(*c["filt"])
        got = m.relocalise_sweeps(c["world_buf"], params=SK.WORLD_PARAMS)
        why = RR.differing(got, world)
        assert why == "", why


# ---- paths ---------------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_paths(pkg, name):
    c = SK.paths_case(name)
    geom = c["geom"]
    plans, wfield = SK.paths_expected(c, geom)
    assert [p["status"] for p in plans] == [PR.OK] * 5 + [PR.UNREACHABLE]
    with _painted(pkg, c["grid"], geom, c["rays"]) as m:
        res = m.plan_paths(c["starts"], c["goals"], clearance=0, snap_radius=SK.PLAN_SNAP, lookahead=200, return_paths=True)
        for i, want in enumerate(plans):
            same_plan(res, i, want)
        assert res["stats"]["snapped"] == 1                               # the start in the UNKNOWN cell
        f = m.distance_field(c["snap_goal"], clearance=0, snap_radius=SK.PLAN_SNAP)
        assert f.dtype == wfield.dtype and (f == wfield).all(), (int((f != wfield).sum()), np.argwhere(f != wfield)[:8].tolist())


# ---- targets -------------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_targets(pkg, name):
    c = SK.targets_case(name)
    geom = c["geom"]
    e = SK.targets_expected(c, geom)
    cents, bots, sep = e["centroids"], c["bots"], c["sep"]
    assert len(cents) == 5
    with _painted(pkg, c["grid"], geom, c["rays"]) as m:
        host = np.array(m.frontier_centroids(3), dtype=np.float64).reshape(-1, 2)
        assert host.shape == cents.shape and (host == cents).all()
        idx, xy, dcents, st = m.frontier_targets(bots, separation=sep, min_cluster=3, return_centroids=True)
        assert dcents.shape == cents.shape and (dcents == cents).all(), "frontier_targets' centroids"
        assert st["n_centroids"] == len(cents) and (idx == e["greedy"][0]).all() and (xy == e["greedy"][1]).all()
        res = m.frontier_targets_by_path(bots, separation=sep, min_cluster=3, return_centroids=True)
        assert (res["centroids"] == cents).all()
        AR.same(res, e["path"])
        res = m.frontier_targets_by_gain(bots, separation=sep, min_cluster=3, return_centroids=True)
        assert (res["centroids"] == cents).all() and res["stats"]["gain_sum"] == int(e["gain_of"].sum())
        AR.same(res, e["gain"], keys=GN.KEYS)
        res = m.frontier_targets_by_territory(bots, min_cluster=3, return_centroids=True)
        assert (res["centroids"] == cents).all()
        TY.same(res, e["territory"], ("idx", "xy", ("cost", "cost_b"), "status", "waypoint_cell", "waypoint", "area", "box", "centroid_owner"))
        part = m.territories(bots, return_owner=True, return_cost=True)
        TY.same(part, TY.partition(c["grid"], bots, *geom), ("owner", "cost", "status", "area", "box"))
        assert (part["area"] > 0).all()


# ---- view ----------------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_view(pkg, name):
    c = SK.view_case(name)
    geom = c["geom"]
    want = SK.view_restate(c, geom)
    P = pkg.protocol
    with _painted(pkg, c["grid"], geom) as m:
        for i, p in enumerate(c["frames"]):
            got = m.render_view(p["width"], p["height"], p["scale"], p["offset_x"], p["offset_y"], zones=np.zeros(0, dtype=P.VIEW_ZONE_DTYPE),
                                prims=np.zeros(0, dtype=P.VIEW_PRIM_DTYPE), line_min=p["line_min"], line_max=p["line_max"], bg=p["bg"],
                                line=p["line"], free=p["free"], occ=p["occ"], draw_occupied=p["draw_occupied"], minify=p["minify"])
            w = want[f"frame{i}"]
            assert got.shape == w.shape and got.dtype == np.uint8
            bad = np.argwhere((got != w).any(axis=2))
            assert len(bad) == 0, (i, len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), w[tuple(bad[0])].tolist())


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
@GEOMETRY
def test_world_to_grid_on_both_axes(pkg, name):
    c = SK.plumbing_case(name)
    want = SK.plumbing_restate(c, c["geom"])
    assert all(want[k].min() <= -2 and want[k].max() >= 66 for k in want)       # (off the grid on either side; int() truncates)
    with pkg.QuasarMapper(c["size"], *c["geom"]) as m:
        for axis in (0, 1):
            got = m.world_to_grid(c["w"][axis], axis)
            assert (got == want[f"axis{axis}"]).all(), (axis, np.nonzero(got != want[f"axis{axis}"])[0][:8].tolist())
