"""Path planning on the device (qs_traversable, qs_plan_field, qs_plan_paths) against the CPU restatement of
include/quasar_slam.h's rules in plan_rules.py and scipy's Dijkstra.  Every value is compared with ==."""
import importlib
import math
import socket
import time

import numpy as np
import pytest

import plan_rules as R
from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def golden_mapper(pkg, name):
    g = np.load(f"{GOLDEN}/{name}.npz", allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    m = pkg.QuasarMapper(int(size), res, ox, oy, separation=sep)
    m.ingest_array(g["datagrams"], g["lengths"])
    return m


@pytest.fixture(scope="module")
def map64(pkg):
    replay = importlib.import_module(pkg.__name__ + ".replay")
    session, _ = replay.telemetry_csv_to_packets()
    stream = replay.multi_bot_stream(session, 64, 64 * 400)
    m = pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2)
    m.ingest_array(stream)
    acc, pose = m.last_batch()
    last = {}
    for i in np.nonzero(acc)[0]:
        last[int(stream[i, 4])] = (float(pose[i, 0]), float(pose[i, 1]))
    yield m, [last[b] for b in sorted(last)]
    m.close()


def cell_xy(m, gx, gy):
    return (m.ox + (gx + 0.5) * m.res, m.oy + (gy + 0.5) * m.res)


@pytest.mark.parametrize("name", ["session_512", "laps5_512"])
def test_traversable_golden(pkg, name):
    with golden_mapper(pkg, name) as m:
        grid = m.grid_i8()
        for c in (0, 1, 2, 5, 16):
            t = m.traversable(c)
            assert (t == R.traversable(grid, c)).all(), (name, c)
            assert t.any()


def test_traversable_64_bots_4096(map64):
    m, _ = map64
    grid = m.grid_i8()
    for c in (0, 1, 2, 5, 16):
        assert (map64[0].traversable(c) == R.traversable(grid, c)).all(), c


def goals_of(t, k, seed):
    yy, xx = np.nonzero(t)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(yy), size=k, replace=False)
    return [(int(xx[i]), int(yy[i])) for i in pick]


def check_fields(m, clearance, goals):
    t = m.traversable(clearance).astype(bool)
    graph = R.move_graph(t)
    for gx, gy in goals:
        f = m.distance_field(cell_xy(m, gx, gy), clearance=clearance)
        want = R.field_scipy(t, (gx, gy), graph)
        assert (f == want).all(), (clearance, gx, gy, int((f != want).sum()))
        assert (f == R.INF).any() and (f != R.INF).sum() > 1


@pytest.mark.parametrize("name", ["session_512", "laps5_512"])
def test_distance_field_golden(pkg, name):
    with golden_mapper(pkg, name) as m:
        for c in (0, 2, 5):
            check_fields(m, c, goals_of(m.traversable(c), 3, c))


def test_distance_field_64_bots_4096(map64):
    m, _ = map64
    check_fields(m, 2, goals_of(m.traversable(2), 2, 7))


def test_plans_64_bots_4096_match_restatement(map64):
    m, bots = map64
    cents = m.frontier_centroids()
    idx, xy = m.frontier_targets(bots)
    ok = idx >= 0
    starts, goals = np.array(bots)[ok], xy[ok]
    res = m.plan_paths(starts, goals, return_paths=True)
    t = m.traversable(2).astype(bool)
    graph = R.move_graph(t)
    assert len(cents) and ok.sum() > 16
    assert (res["status"] == R.OK).sum() > 0
    for i in range(0, len(starts), max(1, len(starts) // 8)):
        want = R.plan(t, tuple(starts[i]), tuple(goals[i]), m.res, m.ox, m.oy, graph=graph)
        check_one(res, i, want)


def check_one(res, i, want):
    assert res["status"][i] == want["status"], i
    if want["status"] != R.OK:
        assert tuple(res["waypoint_cell"][i]) == (-1, -1) and np.isnan(res["waypoint"][i]).all()
        assert res["cost"][i] == R.INF and res["path_len"][i] == 0
        return
    assert tuple(res["waypoint_cell"][i]) == tuple(want["cell"]), i
    assert tuple(res["waypoint"][i]) == tuple(want["xy"]), i
    assert res["cost"][i] == want["cost"] and res["path_len"][i] == len(want["path"]), i
    if "paths" in res:
        assert [tuple(c) for c in res["paths"][i].tolist()] == want["path"], i


# ---- a synthetic maze: a wall with one gap between start and goal --------------------------------------------------
def maze(pkg):
    m = pkg.QuasarMapper(200, 0.05, -5.0, -5.0)
    ys = np.arange(-4.5, 4.5, 0.025)
    m.update_rays(np.full(len(ys), -4.5), ys, np.full(len(ys), 4.5), ys, np.zeros(len(ys), dtype=np.uint8))
    wy = np.arange(-4.6, 4.6, 0.05)
    wy = wy[(wy < 2.5) | (wy > 3.5)]                             # the gap: 2.5 < y < 3.5
    wx = np.full(len(wy), 0.025)
    m.update_rays(wx, wy, wx, wy, np.ones(len(wy), dtype=np.uint8))
    return m


def test_maze_gap(pkg):
    with maze(pkg) as m:
        start, goal = (-2.0, -2.0), (2.0, -2.0)
        res = m.plan_paths([start], [goal], return_paths=True)
        t = m.traversable(2).astype(bool)
        want = R.plan(t, start, goal, m.res, m.ox, m.oy)
        assert want["status"] == R.OK and res["status"][0] == R.OK
        check_one(res, 0, want)
        path = res["paths"][0]
        wall_x = int((0.025 + 5.0) / 0.05)
        on_wall = path[path[:, 0] == wall_x]
        assert len(on_wall) and ((on_wall[:, 1] > int((2.5 + 5.0) / 0.05)) & (on_wall[:, 1] < int((3.5 + 5.0) / 0.05))).all()
        gcell = (int((goal[0] + 5.0) / 0.05), int((goal[1] + 5.0) / 0.05))
        wp = tuple(res["waypoint_cell"][0])
        assert wp != gcell
        s = tuple(path[0])
        assert all(t[y, x] for x, y in R.bresenham(s[0], s[1], wp[0], wp[1]))
        from oracle import oracle as orc
        assert [tuple(c) for c in orc.bresenham(s[0], s[1], wp[0], wp[1]).tolist()] == R.bresenham(s[0], s[1], wp[0], wp[1])
        # the lookahead bounds the waypoint; the whole path still comes back
        for la in (1, 5, 50):
            r2 = m.plan_paths([start], [goal], lookahead=la)
            w2 = R.plan(t, start, goal, m.res, m.ox, m.oy, lookahead=la)
            check_one(r2, 0, w2)


def test_edge_cases(pkg):
    with maze(pkg) as m:
        t = m.traversable(2).astype(bool)
        r0 = m.plan_paths(np.zeros((0, 2)), np.zeros((0, 2)))
        assert len(r0["status"]) == 0 and r0["stats"]["groups"] == 0
        inside = (-2.0, -2.0)
        cases = [
            (inside, inside),                       # start == goal
            ((math.nan, 0.0), inside),
            (inside, (math.inf, 0.0)),
            ((-1e300, 0.0), inside),
            ((100.0, 0.0), inside),                 # off the grid
            (inside, (0.0, -5.2)),                  # off the grid (y)
            ((-0.02, -2.0), inside),                # on the wall's clearance band: snaps
            ((-4.9, -4.9), inside),                 # UNKNOWN corner, nothing within 10 cells: cannot snap
            (inside, (-0.02, 1.0)),                 # goal snaps
        ]
        s = [c[0] for c in cases]
        g = [c[1] for c in cases]
        res = m.plan_paths(s, g, return_paths=True)
        for i, (a, b) in enumerate(cases):
            check_one(res, i, R.plan(t, a, b, m.res, m.ox, m.oy))
        assert res["status"].tolist() == [R.OK, R.NO_START, R.NO_GOAL, R.NO_START, R.NO_START, R.NO_GOAL, R.OK,
                                          R.NO_START, R.OK]
        assert res["cost"][0] == 0 and res["path_len"][0] == 1
        assert res["stats"]["snapped"] >= 2
        # path_cap truncation: the first cells, the full length
        full = m.plan_paths([inside], [(2.0, -2.0)], return_paths=True)
        cut = m.plan_paths([inside], [(2.0, -2.0)], return_paths=True, path_cap=7)
        assert cut["path_len"][0] == full["path_len"][0] > 7
        assert (cut["paths"][0] == full["paths"][0][:7]).all()
        with pytest.raises(Exception, match="clearance"):
            m.plan_paths([inside], [inside], clearance=17)
        with pytest.raises(Exception, match="clearance"):
            m.traversable(17)
    # a goal in another component: two rooms with no passage
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        ys = np.arange(-4.0, -2.0, 0.025)
        m.update_rays(np.full(len(ys), -4.0), ys, np.full(len(ys), -1.0), ys, np.zeros(len(ys), dtype=np.uint8))
        m.update_rays(np.full(len(ys), 1.0), ys, np.full(len(ys), 4.0), ys, np.zeros(len(ys), dtype=np.uint8))
        res = m.plan_paths([(-3.0, -3.0)], [(3.0, -3.0)])
        assert res["status"][0] == R.UNREACHABLE and res["cost"][0] == R.INF
        f = m.distance_field((3.0, -3.0))
        assert f[int((-3.0 + 5) / 0.05), int((-3.0 + 5) / 0.05)] == R.INF
    # an empty map
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        res = m.plan_paths([(0.0, 0.0)], [(1.0, 1.0)])
        assert res["status"][0] == R.NO_START
        assert not m.traversable(0).any() and (m.distance_field((0.0, 0.0)) == R.INF).all()


def test_groups_8192(pkg):
    """Requests whose fields exceed QS_PLAN_WS_CAP together run in groups, with the same answers as one at a time."""
    with pkg.QuasarMapper(8192, 0.05, -204.8, -204.8) as m:
        # a room near one corner, and free cells at the far corner: the bounding box spans the whole grid
        ys = np.arange(-200.0, -195.0, 0.025)
        m.update_rays(np.full(len(ys), -200.0), ys, np.full(len(ys), -195.0), ys, np.zeros(len(ys), dtype=np.uint8))
        ys2 = np.arange(200.0, 204.0, 0.025)
        m.update_rays(np.full(len(ys2), 200.0), ys2, np.full(len(ys2), 204.0), ys2, np.zeros(len(ys2), dtype=np.uint8))
        rng = np.random.default_rng(3)
        n = 12
        s = rng.uniform(-199.5, -195.5, size=(n, 2))
        g = rng.uniform(-199.5, -195.5, size=(n, 2))
        g[-1] = (202.0, 202.0)                          # the other component
        res = m.plan_paths(s, g, return_paths=True)
        assert res["stats"]["groups"] >= 2
        assert (res["status"][:-1] == R.OK).all() and res["status"][-1] == R.UNREACHABLE
        for i in range(n):
            one = m.plan_paths(s[i:i + 1], g[i:i + 1], return_paths=True)
            assert one["stats"]["groups"] == 1
            for k in ("status", "waypoint_cell", "waypoint", "cost", "path_len"):
                assert (np.asarray(one[k][0]) == np.asarray(res[k][i])).all() or (
                    k == "waypoint" and np.isnan(res[k][i]).all() and np.isnan(one[k][0]).all()), (i, k)
            assert (one["paths"][0] == res["paths"][i]).all()


def test_no_side_effects(pkg):
    with golden_mapper(pkg, "session_512") as m:
        before = (m.grid_i8().tobytes(), [c.tobytes() for c in m.counts()], bytes(m.checkpoint()))
        s, g = [(0.0, 0.0), (1.0, -1.0), (-2.0, 3.0)], [(3.0, 3.0), (-3.0, 2.0), (0.5, 0.5)]
        a = m.plan_paths(s, g, return_paths=True)
        m.traversable(5)
        m.distance_field((0.0, 0.0))
        b = m.plan_paths(s, g, return_paths=True)
        after = (m.grid_i8().tobytes(), [c.tobytes() for c in m.counts()], bytes(m.checkpoint()))
        assert before == after
        for k in ("status", "waypoint_cell", "cost", "path_len"):
            assert (a[k] == b[k]).all()
        assert a["waypoint"].tobytes() == b["waypoint"].tobytes()
        assert all((x == y).all() for x, y in zip(a["paths"], b["paths"]))
        assert a["stats"] == b["stats"]


def test_mission_control_waypoints_over_udp(pkg):
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    P = importlib.import_module(pkg.__name__ + ".protocol")
    with golden_mapper(pkg, "session_512") as m:
        srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        srv.bind(("127.0.0.1", 0))
        port = srv.getsockname()[1]
        mc = fe.MissionControl(m, sock=srv, max_agent=2, frontier_targets=True, plan_paths=True)
        bots = {b: socket.socket(socket.AF_INET, socket.SOCK_DGRAM) for b in (1, 2)}
        for s in bots.values():
            s.bind(("127.0.0.1", 0))
            s.settimeout(2.0)
        mc.bot_ports = {b: bots[b].getsockname()[1] for b in bots}
        grid = m.grid_i8()
        t = R.traversable(grid, 2)
        yy, xx = np.nonzero(t)
        picks = [len(yy) // 5, (4 * len(yy)) // 5]
        for b, k in zip((1, 2), picks):
            x, y = cell_xy(m, int(xx[k]), int(yy[k]))
            bots[b].sendto(P.pack_packet(b, x, y, 0.0, 0, 0, 0.0, 0.0, 0.0, 0.0), ("127.0.0.1", port))
            time.sleep(0.02)
        time.sleep(0.05)
        assert mc.poll(now=1000.0) == 2
        states = {b: mc.bot_pose[b] for b in (1, 2)}
        assigned = m.assign_frontier_targets(states)
        sent = mc.target_tick(now=1000.0, force=True)
        assert set(sent) == set(assigned) and sent
        t = R.traversable(m.grid_i8(), 2)
        for b, xy in assigned.items():
            want = R.plan(t, states[b], xy, m.res, m.ox, m.oy)
            pkt = P.pack_target(*(want["xy"] if want["status"] == R.OK else xy))
            assert sent[b] == pkt, b
            assert bots[b].recv(64) == pkt
        assert sum(mc.plan_stats.values()) == len(assigned)
        for s in bots.values():
            s.close()
        mc.close()
