"""Frontier targets by path cost on the device (qs_frontier_targets_by_path) against the CPU restatement of
include/quasar_slam.h's rules in assign_rules.py, which is fed the device's own grid_i8() and the same bots.  Every value
of every bot is compared with ==."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import assign_rules as A
import plan_rules as R
from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu
K = 32          # AS_K


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def check(m, bots, sep=1.0, min_cluster=3, **params):
    """The call against the restatement: centroids, every output of every bot, and the counts in stats."""
    bots = np.asarray(bots, dtype=np.float64).reshape(-1, 2)
    res = m.frontier_targets_by_path(bots, separation=sep, min_cluster=min_cluster, return_centroids=True, **params)
    ref_c = np.array(m.frontier_centroids(min_cluster), dtype=np.float64).reshape(-1, 2)
    assert res["centroids"].shape == ref_c.shape and (res["centroids"] == ref_c).all()
    want = A.assign(m.grid_i8(), ref_c, bots, m.res, m.ox, m.oy, sep, **params)
    A.same(res, want)
    st = res["stats"]
    assert st["n_centroids"] == len(ref_c)
    assert st["centroid_cells"] == sum(c is not None for c in want["centroid_cells"])
    assert st["bot_cells"] == sum(c is not None for c in want["bot_cells"])
    assert st["reserved"] == 0
    return res, want


def golden_case(pkg, name):
    g = np.load(f"{GOLDEN}/{name}.npz", allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    m = pkg.QuasarMapper(int(size), res, ox, oy, separation=sep)
    m.ingest_array(g["datagrams"], g["lengths"])
    return m, last_poses(m, g["datagrams"])


def last_poses(m, stream):
    """The pose of each bot's last accepted packet, ascending id."""
    acc, pose = m.last_batch()
    last = {}
    for i in np.nonzero(acc)[0]:
        last[int(stream[i, 4])] = (float(pose[i, 0]), float(pose[i, 1]))
    return [last[b] for b in sorted(last)]


@pytest.mark.parametrize("name", ["session_512", "laps5_512", "session_sep_512", "mixed_200"])
def test_golden_sessions(pkg, name):
    m, bots = golden_case(pkg, name)
    with m:
        assert len(bots) == 2
        res, _ = check(m, bots)
        assert (res["status"] == R.OK).all() and (res["idx"] >= 0).all()
        # every target of the new call plans OK ...
        again = m.plan_paths(bots, res["xy"])
        assert (again["status"] == R.OK).all()
        for k in ("cost", "waypoint_cell", "waypoint"):
            assert (again[k] == res[k]).all(), k
        # ... where the straight-line targets of the same bots do not
        idx, xy = m.frontier_targets(bots)
        assert (idx >= 0).all()
        line = m.plan_paths(bots, xy)
        if name != "mixed_200":
            assert (line["status"] == R.UNREACHABLE).any()
        check(m, bots[::-1], sep=0.0, min_cluster=1, clearance=1, snap_radius=4, lookahead=7)


@pytest.fixture(scope="module")
def map64(pkg):
    replay = importlib.import_module(pkg.__name__ + ".replay")
    session, _ = replay.telemetry_csv_to_packets()
    stream = replay.multi_bot_stream(session, 64, 64 * 400)
    m = pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2)
    m.ingest_array(stream)
    yield m, last_poses(m, stream)
    m.close()


def test_64_bots_4096(map64):
    m, bots = map64
    assert len(bots) == 64
    res, _ = check(m, bots)                                   # all 64 bots restated in full
    ok = res["idx"] >= 0
    assert (res["status"][ok] == R.OK).all() and ok.sum() > 16
    again = m.plan_paths(np.array(bots)[ok], res["xy"][ok])   # a separate plan_paths(bot, target) call
    assert (again["status"] == R.OK).all()
    for k in ("cost", "waypoint_cell", "waypoint"):
        assert (again[k] == res[k][ok]).all(), k
    idx, xy = m.frontier_targets(bots)
    line = m.plan_paths(np.array(bots)[idx >= 0], xy[idx >= 0])
    assert ok.sum() >= (line["status"] == R.OK).sum()
    # the centroid list is qs_frontier_targets'
    _, _, cents, st = m.frontier_targets(bots, return_centroids=True)
    got = m.frontier_targets_by_path(bots, return_centroids=True, waypoints=False)
    assert got["stats"]["n_centroids"] == st["n_centroids"] and (got["centroids"] == cents).all()
    # without the waypoint stage: the same assignment, no waypoints
    A.same(got, res, keys=("idx", "xy", "cost", "status"))
    assert (got["waypoint_cell"] == -1).all() and np.isnan(got["waypoint"]).all()


# ---- scenes built ray by ray on a 200 x 200 grid ---------------------------------------------------------------------------
def cx(g):
    """World coordinate of the centre of cell g (both axes: origin -5, 0.05 m per cell)."""
    return -5.0 + (g + 0.5) * 0.05


def free_rows(m, rows, segments):
    """FREE cells [a, b) of every row in rows, for every (a, b) of segments (a ray frees all its cells but the last)."""
    rx, ry, hx = [], [], []
    for gy in rows:
        for a, b in segments:
            rx.append(cx(a)); hx.append(cx(b)); ry.append(cx(gy))
    n = len(rx)
    m.update_rays(np.array(rx), np.array(ry), np.array(hx), np.array(ry), np.zeros(n, dtype=np.uint8))


def holes_scene(pkg):
    """An open square of FREE cells [60, 140)^2 with an UNKNOWN cell every 4 cells of every 4th row: hundreds of small
    frontier clusters a few cells apart, all in one connected region."""
    m = pkg.QuasarMapper(200, 0.05, -5.0, -5.0)
    plain = [gy for gy in range(60, 140) if gy % 4]
    free_rows(m, plain, [(60, 140)])
    free_rows(m, [gy for gy in range(60, 140) if gy % 4 == 0], [(a, a + 3) for a in range(60, 140, 4)])
    return m


def test_fallback_full_scan(pkg):
    """Many bots on one spot and more than K centroids within `separation` of the first pick: every later bot's list of
    the K cheapest is entirely ineligible, so its field is computed again and every centroid scanned."""
    with holes_scene(pkg) as m:
        cents = np.array(m.frontier_centroids(1), dtype=np.float64)
        assert len(cents) > 400
        spot = (cx(101), cx(101))
        bots = [spot] * 12 + [(cx(62), cx(62)), spot, (cx(137), cx(70)), (math.nan, 0.0)]
        for sep in (1.0, 1.6):
            first = cents[A.assign(m.grid_i8(), cents, [spot], m.res, m.ox, m.oy, 0.0, clearance=0, waypoints=False)["idx"][0]]
            assert (np.sqrt((cents[:, 0] - first[0]) ** 2 + (cents[:, 1] - first[1]) ** 2) < sep).sum() > K
            res, _ = check(m, bots, sep=sep, min_cluster=1, clearance=0)
            assert res["stats"]["fallbacks"] > 0
            assert (res["idx"][:3] >= 0).all() and res["status"][-1] == R.NO_START
        res, _ = check(m, bots, sep=0.0, min_cluster=1, clearance=0)
        assert res["stats"]["fallbacks"] == 0                 # 13 taken centroids cannot fill a list of K


def wall_scene(pkg):
    """FREE cells [10, 190)^2, a wall at column 100 with one gap (rows 150..169), one UNKNOWN cell on either side of the
    wall in row 40: at column 110 (near the bot in a straight line, far by path) and at column 60."""
    m = pkg.QuasarMapper(200, 0.05, -5.0, -5.0)
    free_rows(m, [gy for gy in range(10, 190) if gy != 40], [(10, 190)])
    free_rows(m, [40], [(10, 60), (61, 110), (111, 190)])
    wy = np.array([cx(gy) for gy in range(8, 192) if not 150 <= gy < 170])
    wx = np.full(len(wy), cx(100))
    m.update_rays(wx, wy, wx, wy, np.ones(len(wy), dtype=np.uint8))
    return m


def test_wall_with_one_gap(pkg):
    with wall_scene(pkg) as m:
        bot = [(cx(90), cx(40))]
        res, _ = check(m, bot, sep=0.0, min_cluster=1)
        idx, xy = m.frontier_targets(bot, separation=0.0, min_cluster=1)
        cents = m.frontier_centroids(1)
        from test_frontier_targets_cpu import greedy
        assert idx.tolist() == greedy(cents, bot, 0.0)       # the straight-line rule, restated
        assert idx[0] >= 0 and res["idx"][0] >= 0 and res["idx"][0] != idx[0]
        assert xy[0, 0] > cx(100) > res["xy"][0, 0]          # across the wall / on the bot's side
        line = m.plan_paths(bot, xy)
        assert line["status"][0] == R.OK and line["cost"][0] > 4 * res["cost"][0]      # round through the gap
        # more bots than one, both sides, and a bot inside the wall's clearance band
        check(m, bot + [(cx(110), cx(45)), (cx(99), cx(100)), (cx(20), cx(180))], sep=0.5, min_cluster=1)


def test_goal_whose_only_move_crosses_a_tile_border(pkg):
    """A goal on the last row of a 64 x 64 tile with no traversable neighbour inside the tile (met on the 64-bot map, where
    an assigned centroid's cell was one): the field must still leave the tile, in both directions."""
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        x = np.array([cx(70)])
        m.update_rays(x, np.array([cx(63)]), x, np.array([cx(71)]), np.zeros(1, dtype=np.uint8))      # column 70, rows 63..70
        t = m.traversable(0).astype(bool)
        assert t.sum() == 8 and t[63, 70] and t[70, 70] and not t[62, 70]
        top, low = (cx(70), cx(70)), (cx(70), cx(63))
        for goal in (low, top):
            f = m.distance_field(goal, clearance=0)
            assert (f == R.field_scipy(t, R.snap(t, goal, m.res, m.ox, m.oy, 10))).all()
        res = m.plan_paths([top, low], [low, top], clearance=0)
        assert res["status"].tolist() == [R.OK, R.OK] and res["cost"].tolist() == [35, 35]


def test_no_side_effects_and_repeatable(pkg):
    m, bots = golden_case(pkg, "session_512")
    with m:
        bots = bots + [(0.0, 0.0), (math.nan, 1.0)]
        before = (m.grid_i8().tobytes(), [c.tobytes() for c in m.counts()], bytes(m.checkpoint()))
        a = m.frontier_targets_by_path(bots, return_centroids=True)
        m.frontier_targets(bots)
        m.plan_paths(bots, bots[::-1])
        b = m.frontier_targets_by_path(bots, return_centroids=True)
        after = (m.grid_i8().tobytes(), [c.tobytes() for c in m.counts()], bytes(m.checkpoint()))
        assert before == after
        for k in ("idx", "xy", "cost", "status", "waypoint_cell", "waypoint", "centroids"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["stats"] == b["stats"]


def test_pending_edge_rays(pkg):
    """Exact-trig rays on cell boundaries wait for the host until the map is observed: the call resolves them first."""
    P = pkg.protocol
    rng = np.random.default_rng(99)
    yaws = np.radians(np.arange(24) * 15.0).astype(np.float32)
    lat = np.arange(-6, 7) * 0.05
    xs, ys, yw = np.meshgrid(lat, lat, yaws, indexing="ij")
    n = xs.size
    stream = P.pack_packets(np.ones(n, dtype=int), xs.ravel(), ys.ravel(), yw.ravel(), np.zeros(n, dtype=int),
                            np.zeros(n, dtype=int), rng.integers(3, 125, (n, 4)) * 0.01, np.zeros(n, dtype=int))
    bots = [(0.0, 0.0), (0.5, 0.5), (-1.0, 0.2), (0.0, 0.0)]
    kw = dict(separation=0.3, min_cluster=1, clearance=0, return_centroids=True)
    edges = 0
    for ox in (0.0, -0.8, -1.6, -3.2):
        cfg = dict(size=64, resolution=0.05, origin_x=ox, origin_y=ox)
        with pkg.QuasarMapper(**cfg) as m, pkg.QuasarMapper(**cfg) as ref:
            m.ingest_array(stream)
            got = m.frontier_targets_by_path(bots, **kw)
            edges += m.counters()["edge_rays"]
            ref.ingest_array(stream)
            ref.grid_i8()                                   # observed before the call: nothing left waiting
            want = ref.frontier_targets_by_path(bots, **kw)
            A.same(got, want, keys=("idx", "xy", "cost", "status", "waypoint_cell", "waypoint", "centroids"))
            check(m, bots, sep=0.3, min_cluster=1, clearance=0)
    assert edges > 0


def test_valid_and_refused_inputs(pkg):
    # an empty map: no centroids, no FREE cells; every bot NO_START
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        res, _ = check(m, [(0.0, 0.0), (1.0, 1.0)])
        assert res["status"].tolist() == [R.NO_START] * 2 and (res["idx"] == -1).all()
        assert res["stats"]["n_centroids"] == 0 and res["stats"]["groups"] == 0
        assert (res["cost"] == R.INF).all() and np.isnan(res["xy"]).all()
    with wall_scene(pkg) as m:
        # clusters all below min_cluster: a map without clusters; bots with a cell are UNREACHABLE
        res, _ = check(m, [(cx(90), cx(40)), (cx(0), cx(0))], min_cluster=1 << 30)
        assert res["status"].tolist() == [R.UNREACHABLE, R.NO_START] and res["stats"]["n_centroids"] == 0
        # no bots
        r0 = m.frontier_targets_by_path(np.zeros((0, 2)), min_cluster=1, return_centroids=True)
        assert r0["idx"].shape == (0,) and r0["waypoint"].shape == (0, 2)
        assert r0["stats"]["n_centroids"] == len(r0["centroids"]) > 0 and r0["stats"]["bot_cells"] == 0
        assert r0["stats"]["centroid_cells"] == len(r0["centroids"])
        # the largest batch, and one more
        rng = np.random.default_rng(5)
        many = np.repeat(rng.uniform(-4.4, 4.4, (16, 2)), 64, axis=0)      # (runs of one spot: the restatement shares a field)
        full, _ = check(m, many, sep=0.25, min_cluster=1)
        assert len(many) == 1024 and 0 < (full["idx"] >= 0).sum() <= full["stats"]["n_centroids"]
        with pytest.raises(ValueError):
            m.frontier_targets_by_path(np.zeros((1025, 2)))
        L = m._L
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        n = C.c_size_t()
        pos, tidx, txy = np.zeros((2048, 2)), np.zeros(2048, dtype=np.int64), np.zeros((2048, 2))
        cost, stat = np.zeros(2048, dtype=np.uint32), np.zeros(2048, dtype=np.int32)
        call = lambda nb, prm, *a: L.qs_frontier_targets_by_path(m._h, 3, 1.0, prm, p(pos), nb, p(tidx), p(txy), p(cost),
                                                                 p(stat), None, None, None, 0, C.byref(n), None)
        assert call(1025, None) == -1 and b"QS_FT_MAX_BOTS" in L.qs_last_error(m._h)
        assert call(4, None) == 0                             # params NULL: the defaults
        lib = importlib.import_module(pkg.__name__ + "._lib")
        for bad in ((17, 10, 200), (2, 65, 200), (2, 10, 0), (-1, 10, 200)):
            prm = lib.QsPlanParams(*bad, 0)
            assert call(4, C.byref(prm)) == -1, bad
        # one of the waypoint pair without the other
        wc = np.zeros((4, 2), dtype=np.int32)
        assert L.qs_frontier_targets_by_path(m._h, 3, 1.0, None, p(pos), 4, p(tidx), p(txy), p(cost), p(stat), p(wc), None,
                                             None, 0, C.byref(n), None) == -1
        assert L.qs_frontier_targets_by_path(m._h, 3, 1.0, None, None, 4, p(tidx), p(txy), p(cost), p(stat), None, None,
                                             None, 0, C.byref(n), None) == -1
        with pytest.raises(Exception, match="clearance"):
            m.frontier_targets_by_path([(0.0, 0.0)], clearance=17)


def test_assign_frontier_targets_by_path(pkg):
    m, bots = golden_case(pkg, "laps5_512")
    with m:
        states = {b + 1: xy for b, xy in enumerate(bots)}
        res = m.frontier_targets_by_path(bots)
        targets, wps = m.assign_frontier_targets(states, by_path=True, return_waypoints=True)
        assert targets == {b + 1: tuple(res["xy"][b].tolist()) for b in range(2)}
        assert wps == {b + 1: tuple(res["waypoint"][b].tolist()) for b in range(2)}
        assert m.assign_frontier_targets(states, by_path=True) == targets
        idx, xy = m.frontier_targets(bots)
        assert m.assign_frontier_targets(states) == {b + 1: tuple(xy[b].tolist()) for b in range(2) if idx[b] >= 0}
        with pytest.raises(ValueError):
            m.assign_frontier_targets(states, return_waypoints=True)


@pytest.mark.parametrize("plan", [False, True])
def test_mission_control_over_udp(pkg, plan):
    import socket
    import time
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    P = importlib.import_module(pkg.__name__ + ".protocol")
    m, poses = golden_case(pkg, "laps5_512")
    with m:
        srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        srv.bind(("127.0.0.1", 0))
        port = srv.getsockname()[1]
        mc = fe.MissionControl(m, sock=srv, max_agent=2, frontier_targets=True, targets_by_path=True, plan_paths=plan,
                               plan_params=dict(lookahead=40))
        bots = {b: socket.socket(socket.AF_INET, socket.SOCK_DGRAM) for b in (1, 2)}
        for s in bots.values():
            s.bind(("127.0.0.1", 0))
            s.settimeout(2.0)
        mc.bot_ports = {b: bots[b].getsockname()[1] for b in bots}
        for b in (1, 2):        # zero ranges: the packets change no cell, only the poses the server remembers
            bots[b].sendto(P.pack_packet(b, poses[b - 1][0], poses[b - 1][1], 0.0, 0, 0, 0.0, 0.0, 0.0, 0.0), ("127.0.0.1", port))
            time.sleep(0.02)
        time.sleep(0.05)
        assert mc.poll(now=1000.0) == 2
        states = [mc.bot_pose[b] for b in (1, 2)]
        sent = mc.target_tick(now=1000.0, force=True)
        want = A.assign(m.grid_i8(), m.frontier_centroids(), states, m.res, m.ox, m.oy, P.FRONTIER_SEPARATION, lookahead=40)
        assert (want["status"] == R.OK).all() and set(sent) == {1, 2}
        for b in (1, 2):
            pkt = P.pack_target(*(want["waypoint"][b - 1] if plan else want["xy"][b - 1]))
            assert sent[b] == pkt and bots[b].recv(64) == pkt
        assert mc.plan_stats == {"waypoint": 2 if plan else 0, "centroid": 0}
        for s in bots.values():
            s.close()
        mc.close()
