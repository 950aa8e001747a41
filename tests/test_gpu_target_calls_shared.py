"""What the four frontier-target calls (qs_frontier_targets, _by_path, _by_gain, _by_territory) do alike: the centroids they
count and hand back, the `cap` they honour, the waypoint stage of the three path-cost calls, bots without a cell and bots
that share one, no bots, no map, and assign_frontier_targets over each.  Every value is compared with ==; what each call
ranks by is pinned by its own module."""
import ctypes as C

import numpy as np
import pytest

import plan_rules as R
from conftest import load_pkg
from test_gpu_territories import cx, free_rows, occupy

pytestmark = pytest.mark.gpu
MIN_CLUSTER = 3
PATH_CALLS = ("by_path", "by_gain", "by_territory")
CALLS = ("plain",) + PATH_CALLS
SENTINEL = -777.25


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def rooms(pkg):
    """200 x 200 cells.  Two rooms joined by a corridor, a wall in the first (detours: a waypoint is not its target), a
    third room nothing leads to, and a strip of UNKNOWN cells inside the first and the third: the rims and the two sides of
    each strip are clusters of more than MIN_CLUSTER cells."""
    m = pkg.QuasarMapper(200, 0.05, -5.0, -5.0)
    free_rows(m, [gy for gy in range(10, 90) if gy != 50], 10, 90)
    free_rows(m, [50], 10, 40)
    free_rows(m, [50], 48, 90)
    free_rows(m, range(10, 90), 110, 190)
    free_rows(m, range(48, 53), 88, 112)
    free_rows(m, [gy for gy in range(120, 190) if gy != 150], 30, 170)
    free_rows(m, [150], 30, 90)
    free_rows(m, [150], 100, 170)
    occupy(m, [(60, gy) for gy in range(10, 70)])
    return m


def wrapper(m, call, bots, **kw):
    """One wrapper call -> its dict (the plain call's tuple made one)."""
    if call == "plain":
        out = m.frontier_targets(bots, min_cluster=MIN_CLUSTER, return_centroids=kw.get("return_centroids", False))
        return dict(zip(("idx", "xy", "centroids", "stats"), out))
    return getattr(m, "frontier_targets_" + call)(bots, min_cluster=MIN_CLUSTER, **kw)


def raw(m, call, bots, cents, cown, cap):
    """The C entry point with the plan and gain parameters NULL and no waypoints -> (rc, n_centroids)."""
    L, n, k = m._L, len(bots), C.c_size_t()
    idx, xy = np.zeros(n, dtype=np.int64), np.zeros((n, 2))
    cost, stat, gain = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    area, box = np.zeros(n, dtype=np.int64), np.zeros((n, 4), dtype=np.int32)
    if call == "plain":
        rc = L.qs_frontier_targets(m._h, MIN_CLUSTER, 1.0, p(bots), n, p(idx), p(xy), p(cents), cap, C.byref(k), None)
    elif call == "by_path":
        rc = L.qs_frontier_targets_by_path(m._h, MIN_CLUSTER, 1.0, None, p(bots), n, p(idx), p(xy), p(cost), p(stat), None,
                                           None, p(cents), cap, C.byref(k), None)
    elif call == "by_gain":
        rc = L.qs_frontier_targets_by_gain(m._h, MIN_CLUSTER, 1.0, None, None, p(bots), n, p(idx), p(xy), p(cost), p(stat),
                                           None, None, p(cents), cap, C.byref(k), p(gain), None)
    else:
        rc = L.qs_frontier_targets_by_territory(m._h, MIN_CLUSTER, None, p(bots), n, p(idx), p(xy), p(cost), p(stat), None,
                                                None, p(area), p(box), p(cents), p(cown), cap, C.byref(k), None)
    return rc, k.value


@pytest.fixture(scope="module")
def shared(pkg):
    """The scene, its bots and every call's answer, computed once and left unchanged.  Bot 0 stands on free space, bot 1
    off the map, bot 2 elsewhere in bot 0's cell."""
    with rooms(pkg) as m:
        bots = np.array([(cx(20), cx(20)), (1000.0, 1000.0), (cx(20) + 0.01, cx(20) - 0.01)])
        s = dict(bots=bots, ref=np.array(m.frontier_centroids(MIN_CLUSTER), dtype=np.float64).reshape(-1, 2))
        s["full"] = {c: wrapper(m, c, bots, return_centroids=True) for c in CALLS}
        s["lean"] = {c: wrapper(m, c, bots, waypoints=False) for c in PATH_CALLS}
        s["none"] = {c: wrapper(m, c, np.zeros((0, 2)), return_centroids=True) for c in CALLS}
        s["paths"], s["swapped"] = {}, {}
        for c in PATH_CALLS:
            res = s["full"][c]
            ok = res["idx"] >= 0
            s["paths"][c] = m.plan_paths(bots[ok], res["xy"][ok])
            other = np.array([2, 1, 0])[ok]               # bots 0 and 2 stand on one cell: each from the other's position
            s["swapped"][c] = m.plan_paths(bots[other], res["xy"][ok])
        n_cent = len(s["ref"])
        s["capped"] = {}
        for c in CALLS:
            cents, cown = np.full((n_cent, 2), SENTINEL), np.full(n_cent, -777, dtype=np.int32)
            rc, k = raw(m, c, bots, cents, cown, n_cent - 1)
            s["capped"][c] = dict(rc=rc, k=k, cents=cents, cown=cown)
        states = {b + 1: tuple(xy) for b, xy in enumerate(bots.tolist())}
        kw = dict(min_cluster=MIN_CLUSTER)
        s["assigned"] = {
            "plain": (m.assign_frontier_targets(states, **kw), None),
            "by_path": m.assign_frontier_targets(states, by_path=True, return_waypoints=True, **kw),
            "by_gain": m.assign_frontier_targets(states, by_gain=True, return_waypoints=True, **kw),
            "by_territory": m.assign_frontier_targets(states, by_territory=True, return_waypoints=True, **kw)}
        s["assigned_lean"] = {c: m.assign_frontier_targets(states, **{c: True}, **kw) for c in PATH_CALLS}
        s["assigned_empty"] = {c: m.assign_frontier_targets({}, **({} if c == "plain" else {c: True})) for c in CALLS}
        s["assigned_empty_wp"] = {c: m.assign_frontier_targets({}, return_waypoints=True, **{c: True}) for c in PATH_CALLS}
        s["territory"] = m.assign_frontier_targets(states, by_territory=True, return_territory=True, **kw)
    with pkg.QuasarMapper(64, 0.05, -1.6, -1.6) as m:         # nothing mapped
        s["empty"] = {c: wrapper(m, c, bots, return_centroids=True) for c in CALLS}
    return s


def test_centroids_are_the_same(shared):
    ref = shared["ref"]
    assert len(ref) >= 3
    for c in CALLS:
        res = shared["full"][c]
        assert res["centroids"].shape == ref.shape and (res["centroids"] == ref).all(), c
        assert res["stats"]["n_centroids"] == len(ref), c


def test_cap_truncates(shared):
    n_cent = len(shared["ref"])
    for c in CALLS:
        got = shared["capped"][c]
        assert got["rc"] == 0 and got["k"] == n_cent, c
        assert (got["cents"][:n_cent - 1] == shared["ref"][:n_cent - 1]).all(), c
        assert (got["cents"][n_cent - 1] == SENTINEL).all(), c
    cown = shared["capped"]["by_territory"]["cown"]
    assert (cown[:n_cent - 1] == shared["full"]["by_territory"]["centroid_owner"][:n_cent - 1]).all() and cown[n_cent - 1] == -777


def test_waypoints_off_and_on(shared):
    for c in PATH_CALLS:
        full, lean, again = shared["full"][c], shared["lean"][c], shared["paths"][c]
        assert (lean["waypoint_cell"] == -1).all() and np.isnan(lean["waypoint"]).all(), c
        for k in ("idx", "cost", "status"):
            assert (lean[k] == full[k]).all(), (c, k)
        ok = full["idx"] >= 0
        assert ok.any() and (again["status"] == R.OK).all(), c
        for k in ("waypoint_cell", "waypoint", "cost"):
            assert (again[k] == full[k][ok]).all(), (c, k)
        assert (full["waypoint_cell"][~ok] == -1).all() and np.isnan(full["waypoint"][~ok]).all(), c


def test_bot_without_a_cell_and_bots_on_one_cell(shared):
    for c in PATH_CALLS:
        res = shared["full"][c]
        assert res["status"][1] == R.NO_START and res["idx"][1] == -1 and res["cost"][1] == R.INF, c
        assert np.isnan(res["xy"][1]).all(), c
        assert res["status"][0] == R.OK and res["status"][2] in (R.OK, R.UNREACHABLE), c
        ok = res["idx"] >= 0
        swapped = shared["swapped"][c]                    # the cost to a bot's target from the other bot of its cell
        assert (swapped["status"] == R.OK).all() and (swapped["cost"] == res["cost"][ok]).all(), c
    for c in ("by_path", "by_gain"):                      # (by territory the higher bot of a cell owns nothing)
        assert (shared["full"][c]["idx"][[0, 2]] >= 0).all(), c


def test_no_bots(shared):
    for c in CALLS:
        res = shared["none"][c]
        assert res["idx"].shape == (0,) and res["xy"].shape == (0, 2), c
        assert (res["centroids"] == shared["ref"]).all() and res["centroids"].shape == shared["ref"].shape, c
    for c in PATH_CALLS:
        res = shared["none"][c]
        assert res["cost"].shape == res["status"].shape == (0,), c
        assert res["waypoint_cell"].shape == res["waypoint"].shape == (0, 2), c


def test_nothing_mapped(shared):
    for c in CALLS:
        res = shared["empty"][c]
        assert res["centroids"].shape == (0, 2) and res["stats"]["n_centroids"] == 0, c
        assert (res["idx"] == -1).all() and np.isnan(res["xy"]).all(), c
    for c in PATH_CALLS:
        assert shared["empty"][c]["status"].tolist() == [R.NO_START] * 3, c


def test_assign_frontier_targets_is_the_wrappers(shared):
    for c in CALLS:
        res = shared["full"][c]
        got = [b for b in range(3) if res["idx"][b] >= 0]
        targets, wps = shared["assigned"][c]
        assert targets == {b + 1: tuple(res["xy"][b].tolist()) for b in got}, c
        assert shared["assigned_empty"][c] == {}, c
        if c == "plain":
            continue
        assert wps == {b + 1: tuple(res["waypoint"][b].tolist()) for b in got}, c
        assert shared["assigned_lean"][c] == targets, c
        assert shared["assigned_empty_wp"][c] == ({}, {}), c
    res = shared["full"]["by_territory"]
    targets, terr = shared["territory"]
    assert targets == shared["assigned"]["by_territory"][0]
    assert terr == {b + 1: (int(res["area"][b]), tuple(res["box"][b].tolist()) if res["area"][b] else None) for b in range(3)}
