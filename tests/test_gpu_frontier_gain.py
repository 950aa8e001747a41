"""Frontier gain on the device (qs_frontier_gain, qs_frontier_targets_by_gain) against the CPU restatement of
include/quasar_slam.h's rules in gain_rules.py, which is fed the device's own grid_i8().  Every viewpoint, every gain and
every output of every bot is compared with ==."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import assign_rules as A
import gain_rules as G
import plan_rules as R
from conftest import load_pkg
from test_gpu_targets_by_path import cx, free_rows, golden_case, holes_scene, last_poses

pytestmark = pytest.mark.gpu
K = 32          # AS_K
GOLDENS = ["session_512", "laps5_512", "session_sep_512", "mixed_200"]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def check_gain(m, min_cluster=3, rng=G.DEFAULT_RANGE, grid=None):
    """qs_frontier_gain against the restatement, and its slots against qs_frontier_clusters'."""
    grid = m.grid_i8() if grid is None else grid
    view, gain = m.frontier_gain(min_cluster, rng)
    want_v, want_g, ties = G.frontier_gain(grid, min_cluster, rng)
    assert view.shape == want_v.shape and (view == want_v).all(), np.argwhere(view != want_v)[:8].tolist()
    assert (gain == want_g).all(), np.argwhere(gain != want_g)[:8].tolist()
    cl, size = G.clusters(grid, min_cluster)
    st = m.frontier_clusters(min_cluster)
    assert (st[:, 2] * size + st[:, 1]).tolist() == [c[0] for c in cl] and st[:, 0].tolist() == [len(c) for c in cl]
    assert (gain >= 1).all()
    return view, gain, ties


def check_assign(m, bots, sep=1.0, min_cluster=3, bias=G.DEFAULT_BIAS, rng=G.DEFAULT_RANGE, **params):
    """qs_frontier_targets_by_gain against the restatement: every output of every bot, the centroids and the counts."""
    bots = np.asarray(bots, dtype=np.float64).reshape(-1, 2)
    res = m.frontier_targets_by_gain(bots, separation=sep, min_cluster=min_cluster, gain_range=rng, gain_bias=bias,
                                     return_centroids=True, **params)
    grid = m.grid_i8()
    cents = np.array(m.frontier_centroids(min_cluster), dtype=np.float64).reshape(-1, 2)
    assert res["centroids"].shape == cents.shape and (res["centroids"] == cents).all()
    _, gain, _ = G.frontier_gain(grid, min_cluster, rng)
    want = G.assign(grid, cents, gain, bots, m.res, m.ox, m.oy, sep, bias=bias, top_k=K, **params)
    A.same(res, want, keys=G.KEYS)
    st = res["stats"]
    assert st["n_centroids"] == len(cents) and st["gain_sum"] == int(gain.sum())
    assert st["centroid_cells"] == sum(c is not None for c in want["centroid_cells"])
    assert st["bot_cells"] == sum(c is not None for c in want["bot_cells"])
    assert st["fallbacks"] == want["fallbacks"]
    return res, want, gain


# ---- the golden sessions -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goldens(pkg):
    made = {}

    def get(name):
        if name not in made:
            made[name] = golden_case(pkg, name)
        return made[name]
    yield get
    for m, _ in made.values():
        m.close()


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_gains(goldens, name):
    m, _ = goldens(name)
    _, gain, ties = check_gain(m)
    assert len(gain) > 100 and sum(t > 1 for t in ties) >= 5          # G2's tie-break decides several viewpoints
    if name == "session_512":
        grid = m.grid_i8()
        for rng in (1, 8):
            check_gain(m, rng=rng, grid=grid)
        for mc in (1, 5):                                             # other slot lists of the same labelling
            check_gain(m, min_cluster=mc, grid=grid)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_assignments(goldens, name):
    m, bots = goldens(name)
    assert len(bots) == 2
    path = m.frontier_targets_by_path(bots)
    for bias in (0, G.DEFAULT_BIAS):
        res, _, _ = check_assign(m, bots, bias=bias)
        assert (res["status"] == R.OK).all()
        again = m.plan_paths(bots, res["xy"])                         # G7: a separate plan_paths(bot, target) call
        assert (again["status"] == R.OK).all()
        for k in ("cost", "waypoint_cell", "waypoint"):
            assert (again[k] == res[k]).all(), k
        if name == "mixed_200" and bias == 0:
            assert (res["idx"] == path["idx"]).all()
        else:
            assert (res["idx"] != path["idx"]).any()
        check_assign(m, bots[::-1], bias=bias)


def test_bot_on_a_centroids_cell_with_bias_0(goldens):
    """Cost 0: with the pure ratio that centroid comes first whatever its gain; with the default bias it need not."""
    m, _ = goldens("session_sep_512")
    cents = m.frontier_centroids()
    _, gain = m.frontier_gain()
    k = int(np.argmin(gain))
    res, _, _ = check_assign(m, [cents[k]], bias=0)
    assert res["idx"].tolist() == [k] and res["cost"].tolist() == [0] and res["gain"].tolist() == [int(gain[k])]
    res, _, _ = check_assign(m, [cents[k]])
    assert res["idx"][0] != k


def test_no_side_effects_and_repeatable(goldens):
    m, bots = goldens("session_512")
    bots = bots + [(0.0, 0.0), (math.nan, 1.0)]
    before = (m.grid_i8().tobytes(), bytes(m.checkpoint()))
    a = m.frontier_targets_by_gain(bots, return_centroids=True)
    g1 = m.frontier_gain()
    m.frontier_targets_by_path(bots)
    b = m.frontier_targets_by_gain(bots, return_centroids=True)
    g2 = m.frontier_gain()
    assert before == (m.grid_i8().tobytes(), bytes(m.checkpoint()))
    for k in G.KEYS + ("centroids",):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"] == b["stats"] and all((x == y).all() for x, y in zip(g1, g2))
    assert a["status"].tolist()[-1] == R.NO_START and a["gain"][-1] == 0


# ---- scenes built ray by ray on a 200 x 200 grid -------------------------------------------------------------------------
def occupy(m, cells):
    """OCCUPIED cells: a ray that starts and ends in the cell."""
    x, y = np.array([cx(c[0]) for c in cells]), np.array([cx(c[1]) for c in cells])
    m.update_rays(x, y, x, y, np.ones(len(cells), dtype=np.uint8))


def free_cells(m, cells):
    for gx, gy in cells:
        free_rows(m, [gy], [(gx, gx + 1)])


def strip(pkg):
    """FREE cells [90, 111) of row 100 in an unknown world: one cluster of 21 cells, viewpoint (100, 100)."""
    m = pkg.QuasarMapper(200, 0.05, -5.0, -5.0)
    free_rows(m, [100], [(90, 111)])
    return m


def test_wall_casts_a_shadow(pkg):
    with strip(pkg) as m:
        view, open_gain, _ = check_gain(m)
        assert view.tolist() == [[100, 100]]
        occupy(m, [(gx, 104) for gx in range(95, 106)])
        _, gain, _ = check_gain(m)
        assert gain[0] < open_gain[0] - 11 - 100                      # the wall's own cells and a shadow far larger
        for rng in (3, 4, 64):                                        # short of the wall, at it, far beyond it
            check_gain(m, rng=rng)


def test_scattered_occupied_cells(pkg):
    """Single OCCUPIED cells all round the viewpoint: each hides the targets whose own line from the viewpoint crosses it,
    which a walk from the target, or a closed-form line, gets wrong for some of them."""
    rng = np.random.default_rng(7)
    with strip(pkg) as m:
        cells = set()
        while len(cells) < 40:
            dx, dy = rng.integers(-20, 21, 2).tolist()
            if dy != 0 and 4 <= dx * dx + dy * dy <= 400:
                cells.add((100 + dx, 100 + dy))
        occupy(m, sorted(cells))
        for r in (8, 24, 64):
            check_gain(m, rng=r)


def test_clusters_at_the_grid_edge(pkg):
    """Viewpoints at gx = 1 and gy = size - 2: the disc is clipped by the grid; nothing outside it is a target."""
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        free_cells(m, [(1, gy) for gy in range(98, 103)])
        free_rows(m, [198], [(100, 105)])
        for rng in (24, 64):
            view, gain, _ = check_gain(m, rng=rng)
            assert view.tolist() == [[1, 100], [102, 198]]
            full = sum(dx * dx + dy * dy <= rng * rng for dx in range(-rng, rng + 1) for dy in range(-rng, rng + 1))
            assert (gain < 0.7 * full).all()


def test_u_shaped_cluster_lower_index_wins(pkg):
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        u = [(94, 93), (94, 94), (94, 95), (94, 96), (95, 96), (96, 96), (96, 95), (96, 94), (96, 93)]
        free_cells(m, u)
        view, _, ties = check_gain(m)
        # the centroid cell (95, 94) lies in the notch; (94, 94) and (96, 94) are equally near
        assert ties == [2] and view.tolist() == [[94, 94]] and m.grid_i8()[94, 95] == -1


def test_long_frontier_line(pkg):
    """One cluster of 399 cells over three stretches: its members lie in many workgroups of the viewpoint kernel."""
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        free_rows(m, [20, 60], [(10, 190)])
        free_rows(m, list(range(21, 60)), [(189, 190)])
        st = m.frontier_clusters(1)
        assert st[:, 0].tolist() == [399]
        for rng in (24, 64):
            check_gain(m, rng=rng)


def test_refused_inputs_and_empty_maps(pkg):
    lib = importlib.import_module(pkg.__name__ + "._lib")
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        view, gain = m.frontier_gain()                                # an empty map: no clusters, no FREE cells
        assert view.shape == (0, 2) and gain.shape == (0,)
        res, _, _ = check_assign(m, [(0.0, 0.0), (1.0, 1.0)])
        assert res["status"].tolist() == [R.NO_START] * 2 and (res["gain"] == 0).all() and res["stats"]["gain_sum"] == 0
    with strip(pkg) as m:
        r0 = m.frontier_targets_by_gain(np.zeros((0, 2)), return_centroids=True)      # no bots
        assert r0["idx"].shape == (0,) and r0["gain"].shape == (0,) and r0["stats"]["n_centroids"] == 1
        check_assign(m, [(cx(100), cx(100))], min_cluster=1 << 30)                    # no clusters
        L = m._L
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        n = C.c_size_t()
        v, g = np.zeros((4, 2), dtype=np.int32), np.zeros(4, dtype=np.int32)
        for rng in (0, 65, -1):
            assert L.qs_frontier_gain(m._h, 3, rng, p(v), p(g), 4, C.byref(n)) == -1, rng
            assert b"QS_GAIN_MAX_RANGE" in L.qs_last_error(m._h)
        assert L.qs_frontier_gain(m._h, 3, 24, p(v), None, 4, C.byref(n)) == -1      # one array without the other
        assert L.qs_frontier_gain(m._h, 3, 24, None, None, 0, C.byref(n)) == 0 and n.value == 1
        pos, tidx, txy = np.zeros((2, 2)), np.zeros(2, dtype=np.int64), np.zeros((2, 2))
        cost, stat, tg = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        call = lambda gp: L.qs_frontier_targets_by_gain(m._h, 3, 1.0, None, gp, p(pos), 2, p(tidx), p(txy), p(cost), p(stat),
                                                        None, None, None, 0, C.byref(n), p(tg), None)
        assert call(None) == 0                                        # NULL: the defaults
        assert call(C.byref(lib.QsGainParams(24, 1 << 31, (0, 0)))) == 0
        for bad in ((0, 120, (0, 0)), (65, 120, (0, 0)), (24, (1 << 31) + 1, (0, 0)), (24, 120, (1, 0)), (24, 120, (0, 1))):
            assert call(C.byref(lib.QsGainParams(*bad))) == -1, bad
        with pytest.raises(ValueError):
            m.frontier_targets_by_gain(np.zeros((1025, 2)))


def test_mirror_symmetric_scene_lower_k_wins(pkg):
    """A walled room with one UNKNOWN gap in the left wall and its mirror image in the right: two clusters with equal gain,
    and for a bot on the axis equal cost."""
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        free_rows(m, list(range(90, 111)), [(70, 131)])
        wall = [(gx, gy) for gx in range(69, 132) for gy in (89, 111)]
        wall += [(gx, gy) for gx in (69, 131) for gy in range(90, 111) if not 99 <= gy <= 101]
        occupy(m, wall)
        view, gain, _ = check_gain(m)
        assert view.tolist() == [[70, 100], [130, 100]] and gain[0] == gain[1]
        bot = (cx(100), cx(100))
        for bias in (0, G.DEFAULT_BIAS):
            res, _, _ = check_assign(m, [bot, bot], sep=0.0, bias=bias, clearance=0)
            assert res["idx"].tolist() == [0, 1] and res["cost"][0] == res["cost"][1] == 150


def test_fallback_full_scan(pkg):
    """holes_scene with many bots on one spot: once the targets so far block a bot's whole list of the K first centroids,
    every centroid is scanned with the (cost, gain, k) entry."""
    with holes_scene(pkg) as m:
        spot = (cx(101), cx(101))
        bots = [spot] * 12 + [(cx(62), cx(62)), spot, (cx(137), cx(70)), (math.nan, 0.0)]
        for bias in (0, G.DEFAULT_BIAS):
            res, want, _ = check_assign(m, bots, sep=1.6, min_cluster=1, bias=bias, rng=4, clearance=0)
            assert res["stats"]["fallbacks"] == want["fallbacks"] > 0
            assert res["idx"][0] >= 0 and res["status"][-1] == R.NO_START
        res, _, _ = check_assign(m, bots, sep=0.0, min_cluster=1, rng=4, clearance=0)
        assert res["stats"]["fallbacks"] == 0


def test_16_bots_1024(pkg):
    """Sixteen bots on the smallest map that holds them; all bots and all clusters restated."""
    replay = importlib.import_module(pkg.__name__ + ".replay")
    session, _ = replay.telemetry_csv_to_packets()
    stream = replay.multi_bot_stream(session, 16, 16 * 400, tiles_per_row=4, origin=(-14.0, -14.0))
    with pkg.QuasarMapper(1024, 0.05, -25.6, -25.6, max_agent=16, bots_per_graph=2) as m:
        m.ingest_array(stream)
        acc, pose = m.last_batch()
        xy = pose[np.nonzero(acc)[0], :2]
        assert xy.min() - 1.2 > -25.6 + 0.05 and xy.max() + 1.2 < 25.6 - 0.05      # the tiles fit, beams included
        bots = last_poses(m, stream)
        assert len(bots) == 16
        _, gain, _ = check_gain(m)
        assert len(gain) > 500
        res, _, _ = check_assign(m, bots)
        path = m.frontier_targets_by_path(bots)
        ok = (res["idx"] >= 0) & (path["idx"] >= 0)
        assert ok.sum() >= 8 and (res["idx"][ok] != path["idx"][ok]).any()
        assert res["gain"][ok].mean() > gain[path["idx"][ok]].mean()


def test_assign_frontier_targets_by_gain(goldens):
    m, bots = goldens("laps5_512")
    states = {b + 1: xy for b, xy in enumerate(bots)}
    res = m.frontier_targets_by_gain(bots, gain_bias=0)
    targets, wps = m.assign_frontier_targets(states, by_gain=True, return_waypoints=True, gain_bias=0)
    assert targets == {b + 1: tuple(res["xy"][b].tolist()) for b in range(2)}
    assert wps == {b + 1: tuple(res["waypoint"][b].tolist()) for b in range(2)}
    res = m.frontier_targets_by_gain(bots)
    assert m.assign_frontier_targets(states, by_gain=True) == {b + 1: tuple(res["xy"][b].tolist()) for b in range(2)}
    with pytest.raises(ValueError):
        m.assign_frontier_targets(states, by_gain=True, by_path=True)
