"""Path planning without a GPU: the CPU restatement of the rules (plan_rules.py) against scipy's Dijkstra and a word-for-word
rule 1, the C ABI declarations, and MissionControl's waypoint egress with a stub mapper."""
import importlib
import math
import os
import re
import socket
import struct
import time

import numpy as np
import pytest

import plan_rules as R
from conftest import PKG_NAME, ROOT


def random_grid(rng, n, p_occ=0.08, p_unk=0.05):
    g = np.zeros((n, n), dtype=np.int8)
    u = rng.random((n, n))
    g[u < p_occ] = 100
    g[(u >= p_occ) & (u < p_occ + p_unk)] = -1
    return g


def maze_grid(n=41):
    """Walls every 8 columns, each with one gap at alternating ends."""
    g = np.zeros((n, n), dtype=np.int8)
    for k, x in enumerate(range(8, n - 1, 8)):
        g[:, x] = 100
        gap = 2 if k % 2 else n - 4
        g[gap:gap + 2, x] = 0
    return g


def test_traversable_edt_equals_rule():
    rng = np.random.default_rng(1)
    for c in (0, 1, 2, 3, 5):
        g = random_grid(rng, 24, p_occ=0.03)
        assert (R.traversable(g, c) == R.traversable_brute(g, c)).all(), c


def test_heapq_field_equals_scipy():
    rng = np.random.default_rng(2)
    for trial in range(6):
        g = random_grid(rng, 30) if trial < 4 else maze_grid()
        t = R.traversable(g, trial % 2)
        yy, xx = np.nonzero(t)
        for k in rng.choice(len(yy), size=3, replace=False):
            goal = (int(xx[k]), int(yy[k]))
            assert (R.field_heapq(t, goal) == R.field_scipy(t, goal)).all()


def test_no_corner_cutting():
    t = np.ones((3, 3), dtype=bool)
    t[0, 1] = False                     # (1, 0) blocked: (0, 0) -> (1, 1) may not cut past it
    f = R.field_heapq(t, (0, 0))
    assert f[1, 1] == 2 * R.ORTHO and f[0, 2] == 4 * R.ORTHO     # around, not across the corner
    t2 = np.array([[1, 0], [0, 1]], dtype=bool)       # a diagonal pair only: not connected
    assert R.field_heapq(t2, (0, 0))[1, 1] == R.INF


def test_walk_tie_order_and_waypoint():
    # open 5x5: from (0, 0) to (2, 2) both E and N descend at first?  the field decides; E comes first among ties
    t = np.ones((5, 5), dtype=bool)
    f = R.field_heapq(t, (4, 0))
    assert R.walk(t, f, (0, 0), (4, 0)) == [(x, 0) for x in range(5)]
    f = R.field_heapq(t, (2, 1))
    path = R.walk(t, f, (0, 0), (2, 1))
    assert path == [(0, 0), (1, 0), (2, 1)]          # E (5) + NE (7) == 12: E is tried before NE
    # a wall between start and goal: the waypoint stops before the first cell the start cannot see
    g = maze_grid()
    t = R.traversable(g, 0)
    out = R.plan(t, (0.5 * 0.05, 0.5 * 0.05), (20.5 * 0.05, 0.5 * 0.05), 0.05, 0.0, 0.0)
    assert out["status"] == R.OK
    wp = out["cell"]
    assert all(t[y, x] for x, y in R.bresenham(0, 0, wp[0], wp[1]))
    nxt = out["path"][out["path"].index(tuple(wp)) + 1]
    assert not all(t[y, x] for x, y in R.bresenham(0, 0, nxt[0], nxt[1]))
    assert R.plan(t, (0.025, 0.025), (0.025, 0.025), 0.05, 0.0, 0.0)["cost"] == 0


def test_bresenham_matches_oracle():
    from oracle import oracle as orc
    rng = np.random.default_rng(4)
    for _ in range(50):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-30, 30, size=4))
        assert [tuple(c) for c in orc.bresenham(x0, y0, x1, y1).tolist()] == R.bresenham(x0, y0, x1, y1)


def test_snap_rule():
    t = np.zeros((20, 20), dtype=bool)
    t[5, 9] = t[9, 5] = True           # both at d^2 = 16 from (5, 5): the lower gy * w + gx wins
    assert R.snap(t, (5.5, 5.5), 1.0, 0.0, 0.0, 4) == (9, 5)
    assert R.snap(t, (5.5, 5.5), 1.0, 0.0, 0.0, 3) is None
    assert R.snap(t, (math.nan, 1.0), 1.0, 0.0, 0.0, 4) is None
    assert R.snap(t, (-1.5, 1.0), 1.0, 0.0, 0.0, 4) is None


def test_abi_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    for name in ("qs_traversable", "qs_plan_field", "qs_plan_paths"):
        assert re.search(rf"int {name}\(", txt)
    assert "#define QS_PLAN_MAX_CLEARANCE 16" in txt and "QS_PLAN_WS_CAP" in txt
    lib = importlib.import_module(PKG_NAME + "._lib")
    pkg = importlib.import_module(PKG_NAME)
    pkg.build()
    L = pkg.load()
    for name in ("qs_traversable", "qs_plan_field", "qs_plan_paths"):
        assert name in lib.SIGNATURES and hasattr(L, name)


# ---- MissionControl with a stub mapper ----------------------------------------------------------------------------------
class StubMapper:
    CENTS = {1: (1.0, 1.0), 2: (-2.0, 0.0), 3: (4.0, 4.0)}

    def __init__(self):
        self.plan_calls = []
        self._acc = self._pose = None

    def ingest_array(self, buf, lens, times):
        rec = np.frombuffer(np.ascontiguousarray(buf[:, :42]).tobytes(), dtype=[("m", "S4"), ("a", "u1"), ("x", "<f4"),
                                                                               ("y", "<f4"), ("rest", "V29")])
        self._acc = ((lens == 42) & (rec["m"] == b"QSRL")).astype(np.uint8)
        self._pose = np.stack([rec["x"].astype(np.float64), rec["y"].astype(np.float64), np.zeros(len(rec))], axis=1)

    def last_batch(self):
        return self._acc, self._pose

    def zone(self, bot):
        return (0.0, 0.0, 1.0, 1.0)

    def zone_packet(self, bot, online=True):
        return struct.pack("<4sffff", b"ZONE", 0.0, 0.0, 1.0, 1.0)

    def assign_frontier_targets(self, bot_states):
        return {b: self.CENTS[b] for b in bot_states}

    def plan_paths(self, starts, goals, **kw):
        """Bot order in, bot order out: status OK (waypoint = midpoint) for all but a goal at (4, 4) (UNREACHABLE)."""
        self.plan_calls.append((np.array(starts), np.array(goals), kw))
        g = np.array(goals, dtype=np.float64)
        s = np.array(starts, dtype=np.float64)
        st = np.where((g == (4.0, 4.0)).all(axis=1), R.UNREACHABLE, R.OK).astype(np.int32)
        return dict(status=st, waypoint=(s + g) / 2)


def run_mc(plan, **kw):
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    P = importlib.import_module(PKG_NAME + ".protocol")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    port = srv.getsockname()[1]
    stub = StubMapper()
    mc = fe.MissionControl(stub, sock=srv, max_agent=3, frontier_targets=True, plan_paths=plan, **kw)
    bots = {b: socket.socket(socket.AF_INET, socket.SOCK_DGRAM) for b in (1, 2, 3)}
    for s in bots.values():
        s.bind(("127.0.0.1", 0))
        s.settimeout(1.0)
    mc.bot_ports = {b: bots[b].getsockname()[1] for b in bots}
    for b, x, y in ((1, 0.5, 0.5), (2, 0.0, 2.0), (3, 3.0, 3.0)):
        bots[b].sendto(P.pack_packet(b, x, y, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5), ("127.0.0.1", port))
        time.sleep(0.02)
    time.sleep(0.05)
    assert mc.poll(now=500.0) == 3
    sent = mc.target_tick(now=500.0, force=True)
    got = {b: bots[b].recv(64) for b in sent}
    for s in bots.values():
        s.close()
    mc.close()
    return mc, stub, sent, got, P


def test_mission_control_sends_waypoints():
    mc, stub, sent, got, P = run_mc(True, plan_params=dict(clearance=3, lookahead=50))
    assert len(stub.plan_calls) == 1
    starts, goals, kw = stub.plan_calls[0]
    assert kw == dict(clearance=3, lookahead=50)
    poses = {b: mc.bot_pose[b] for b in (1, 2, 3)}
    assert starts.tolist() == [list(poses[b]) for b in (1, 2, 3)]
    assert goals.tolist() == [list(StubMapper.CENTS[b]) for b in (1, 2, 3)]
    for b in (1, 2):
        c = StubMapper.CENTS[b]
        assert sent[b] == P.pack_target((poses[b][0] + c[0]) / 2, (poses[b][1] + c[1]) / 2)
    assert sent[3] == P.pack_target(4.0, 4.0)                      # not OK: the centroid
    assert got == sent
    assert mc.plan_stats == {"waypoint": 2, "centroid": 1}


def test_mission_control_without_planning_is_unchanged():
    mc, stub, sent, got, P = run_mc(False)
    assert stub.plan_calls == []
    assert sent == {b: P.pack_target(*StubMapper.CENTS[b]) for b in (1, 2, 3)} and got == sent


def test_plan_paths_needs_frontier_targets():
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    with pytest.raises(ValueError):
        fe.MissionControl(StubMapper(), sock=srv, plan_paths=True)
    srv.close()
