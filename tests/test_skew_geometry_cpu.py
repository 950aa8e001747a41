"""What tests/test_gpu_skew_geometry.py and tests/test_gpu_reach_limit.py take for granted, shown on the CPU with the restatements
alone: the geometry table's conditions; that every family's case tells the right geometry from one with ox and oy swapped and
from one with the usual 0.05 cells (so a kernel that mixed the two origins up, or was right at 0.05 alone, would fail the
device test); the limits' arithmetic at every cell size; and that the poses leave next to no beam uncompared."""
import math

import numpy as np
import pytest

import check_rules as CR
import match_rules as MR
import reloc_group_rules as GR
import reloc_rules as RR
import sense_rules as SR
import skew_geometry as SK
import trail_rules as TR

RESOLUTIONS = sorted({g[0] for g in SK.GEOMETRIES.values()})


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(family, name):
        if (family, name) not in made:
            made[family, name] = SK.FAMILIES[family][0](name)
        return made[family, name]
    return get


# ---- 1. the table ----------------------------------------------------------------------------------------------------------------
def test_table_conditions():
    assert set(SK.GEOMETRIES) == {"lop", "fine", "odd", "far"}
    for name, (res, ox, oy) in SK.GEOMETRIES.items():
        assert ox != oy and abs(ox - oy) >= 8 * res, name
    ratios = [(ox - oy) / res for res, ox, oy in SK.GEOMETRIES.values()]
    assert any(q != round(q) and abs(q - round(q)) > 0.01 for q in ratios), ratios
    assert {g[0] for g in SK.GEOMETRIES.values()} == {0.05, 0.025, 0.04, 0.125}
    assert round((SK.GEOMETRIES["lop"][2] - SK.GEOMETRIES["lop"][1]) / 0.05) == 53
    for name in ("odd",):                                       # both origins on half cells
        res, ox, oy = SK.GEOMETRIES[name]
        assert all(abs(abs(o / res) % 1 - 0.5) < 1e-9 for o in (ox, oy))


# ---- 2. every case tells a swapped and a 0.05 geometry from its own ---------------------------------------------------------------
@pytest.mark.parametrize("name", SK.NAMES)
@pytest.mark.parametrize("family", list(SK.FAMILIES))
def test_a_swapped_or_a_usual_geometry_changes_the_result(cases, family, name):
    c = cases(family, name)
    restate = SK.FAMILIES[family][1]
    res, ox, oy = c["geom"]
    right = restate(c, (res, ox, oy))
    assert SK.differs(right, restate(c, (res, ox, oy))) == "", "the restatement is not a function of its inputs"
    assert SK.differs(right, restate(c, (res, oy, ox))) != "", "ox and oy swapped: nothing changes"
    if res != 0.05:
        try:
            usual = restate(c, (0.05, ox, oy))
        except AssertionError:                                  # (the rules refuse the case's reach at 0.05: a difference too)
            usual = dict(refused=np.ones(1))
        assert SK.differs(right, usual) != "", "cells of 0.05: nothing changes"


@pytest.mark.parametrize("name", SK.NAMES)
def test_the_cases_see_their_maps(cases, name):
    """Nothing above is decided by empty results: the sweeps hit walls, the matches find their displacement, the check tells the
    displaced sweeps from the true ones, the relocalisation finds the poses, the plans succeed, every bot gets a target."""
    c = cases("matching", name)
    out = SK.matching_restate(c, c["geom"])
    assert (out["match_hits"] >= 30).all() and out["match_accepted_match"].sum() >= 5
    found = sum(MR.recovered({k: out["match_" + k][i] for k in ("ix", "iy", "it")}, c["disp"][i]) for i in range(len(c["disp"])))
    assert found >= 5, found
    assert (out["trail_records"] == SK.TRAIL_K).all() and (out["trail_hits"] >= 8).all() and (out["trail_score"] > 0).all()
    c = cases("contradiction check", name)
    out = SK.check_restate(c, c["geom"])
    n = len(c["buf"])
    assert (out["status"][:n] == CR.OK).all() and (out["bad"][:n] == 0).all() and (out["status"][n:] == CR.CONTRADICTS).sum() >= 3
    c = cases("relocalisation", name)
    out = SK.reloc_restate(c, c["geom"])
    assert out["small_accepted"].sum() >= 4
    for k in np.nonzero(out["small_accepted"])[0]:              # (rotations 15 degrees apart: what the gate accepts is a cell off at most)
        assert max(abs(out["small_gx"][k] - SK.SMALL_CELLS[k][0]), abs(out["small_gy"][k] - SK.SMALL_CELLS[k][1])) <= 1, k
    assert (out["world_status"] == RR.OK).all() and (out["group_status"] == GR.OK).all() and (out["group_records"] == 2).all()
    res, ox, oy = c["geom"]
    assert (out["small_x"] == ox + (out["small_gx"] + 0.5) * res).all() and (out["small_y"] == oy + (out["small_gy"] + 0.5) * res).all()
    c = cases("paths", name)
    out = SK.paths_restate(c, c["geom"])
    assert out["status"].tolist() == [0] * 5 + [3] and (out["field"] != 0xFFFFFFFF).sum() > 1000       # (3: UNREACHABLE)
    c = cases("targets", name)
    out = SK.targets_restate(c, c["geom"])
    assert len(out["centroids"]) == 5
    for call in ("greedy", "path", "gain", "territory"):
        assert (out[call + "_idx"] >= 0).all(), call
    c = cases("view", name)
    out = SK.view_restate(c, c["geom"])
    for frame in out.values():
        free, occ = (frame[:, :, :3] == np.array(SK.VR.FREE)).all(axis=2), (frame[:, :, :3] == np.array(SK.VR.OCC)).all(axis=2)
        assert free.sum() > 500 and occ.sum() > 10


# ---- 3. the limits ------------------------------------------------------------------------------------------------------------------
def _one_cell_more(accepts, cells, res, base=0.0):
    """accepts(metres) holds on the limit and fails one step of the last bit beyond it, and at one whole cell more."""
    at = SK.reach_metres(cells, res, base)
    assert accepts(at), (cells, res)
    assert not accepts(math.nextafter(at, math.inf)) and not accepts(SK.reach_metres(cells + 1, res, base)), (cells, res)
    return at


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_limit_arithmetic(res):
    for R in (0, 2, 7):
        cells = SK.limit_cells("match", R)
        assert cells == 127 - 2 - R
        _one_cell_more(lambda s: MR.limit_ok(MR.params(radius=R, window=0), s, res), cells, res)
        max_dist = SK.reach_metres(SK.PACKET_REACH, res)
        _one_cell_more(lambda t: TR.limit_ok(TR.params(radius=R, window=0), max_dist, t, res), cells, res, max_dist)
        cells = SK.limit_cells("reloc", R)
        assert cells == 119 - R - 1
        at = _one_cell_more(lambda s: RR.limit_ok(RR.params(radius=R), s, res), cells, res)
        assert SK.reloc_patch_side(at, res, R) == 254 and SK.reloc_patch_side(math.nextafter(at, math.inf), res, R) == 256
        smax = SK.reach_metres(SK.REACH, res)
        _one_cell_more(lambda t: GR.limit_ok(RR.params(radius=R), smax, t, res), cells, res, smax)
    cells = SK.limit_cells("check")
    assert cells == 254
    _one_cell_more(lambda s: CR.limit_ok(CR.params(res), s, res), cells, res)
    _one_cell_more(lambda s: SR.check_params(res, s), cells, res)


def test_the_largest_relocalisation_reach_in_metres():
    """R = 2: 116 cells of reach (M = 117 with the cell the rounding adds)."""
    assert SK.limit_cells("reloc", 2) == 116
    for res, metres in ((0.025, 2.9), (0.04, 4.64), (0.05, 5.8), (0.125, 14.5)):
        at = SK.reach_metres(116, res)
        assert metres - res / 5 <= at <= metres + 1e-9, (res, at)           # about 2.895, 4.635, 5.795, 14.495 and up to the cell's end
        assert RR.limit_ok(RR.params(radius=2), at, res) and not RR.limit_ok(RR.params(radius=2), at + res, res)
        assert RR.limit_ok(RR.params(radius=2), metres - res / 5, res) and math.ceil((metres - res / 5) / res) == 116
    # the LDS of the scoring kernels at SA = 254: rows of 272 bytes, two regions, 16-bit offsets
    SA, pitch = 254, 272
    assert 2 * SA * pitch == 138176 <= 160 * 1024 and (117 + 119) * pitch + (117 + 119) == 64428 < 65536


# ---- 4. beams that are not compared -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SK.NAMES)
def test_next_to_no_beam_lies_on_a_cell_boundary(cases, name):
    c = cases("sensing", name)
    for poses, beams, rng in ((c["poses"], 181, c["max_range"]), (c["packet_poses"], 4, c["packet_range"])):
        edge, total = SK.edge_share(c["geom"], poses, beams, rng)
        assert edge <= 0.001 * total, (edge, total)
    r = cases("relocalisation", name)
    for poses in (r["group_poses"].reshape(-1, 3), r["world_poses"]):
        edge, total = SK.edge_share(r["geom"], poses, 181, r["filt"][1])
        assert edge <= 0.001 * total, (edge, total)
    for lname in SK.LIMIT_GEOMETRIES:
        geom = SK.GEOMETRIES[lname]
        poses = SK.limit_poses(geom, 4)
        for cells in (SK.limit_cells("match", 2), SK.limit_cells("match", 7), SK.limit_cells("reloc", 2), SK.limit_cells("reloc", 7),
                      SK.limit_cells("check"), SK.REACH):
            edge, total = SK.edge_share(geom, poses, 181, SK.reach_metres(cells, geom[0]))
            assert edge <= 0.001 * total, (lname, cells, edge, total)
