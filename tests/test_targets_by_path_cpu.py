"""Frontier targets by path cost without a GPU: the C ABI declaration, the CPU restatement (assign_rules.py) on the
oracle's grids with known answers and on small hand-built grids, and MissionControl's egress with a stub mapper."""
import importlib
import math
import os
import re
import socket
import struct
import time

import numpy as np
import pytest

import assign_rules as A
import plan_rules as R
from conftest import GOLDEN, PKG_NAME, ROOT
from test_frontier_targets_cpu import greedy


def test_symbol_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    assert re.search(r"int qs_frontier_targets_by_path\(", txt)
    assert "symmetric" in txt[txt.index("frontier targets by path cost"):]
    lib = importlib.import_module(PKG_NAME + "._lib")
    assert "qs_frontier_targets_by_path" in lib.SIGNATURES
    assert len(lib.SIGNATURES["qs_frontier_targets_by_path"][1]) == 16
    pkg = importlib.import_module(PKG_NAME)
    pkg.build()
    assert hasattr(pkg.load(), "qs_frontier_targets_by_path")


# ---- the oracle's grids: known answers ---------------------------------------------------------------------------------
def oracle_case(name):
    """The oracle's grid, the centroids of its clusters (min_cluster 3) and the last pose of each agent after offset and
    drift."""
    from oracle import oracle as orc
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    m = orc.OracleMapper(int(size), res, ox, oy, sep)
    m.feed_stream(g["datagrams"], g["lengths"])
    grid = m.grid.copy()
    st = orc.frontier_clusters(orc.frontier_cells(grid), int(size), 3)
    cents = orc.cluster_centroids_world(st, res, ox, oy)
    ag, poses = m.pose_agents, m.poses
    bots = [tuple(poses[np.nonzero(ag == a)[0][-1], :2].tolist()) for a in sorted(set(ag.tolist()))]
    return grid, cents, bots, (res, ox, oy)


# name: centroids, bots, straight-line picks, their path costs (None = no path), picks by (cost, idx), their costs,
# reachable centroids per bot
KNOWN = {
    "session_512": (111, [(0.0888250272073492, 0.8032124862074852), (4.705193638801575, 1.415234338492155)],
                    [62, 69], [None, 80], [72, 69], [92, 80], [53, 53]),
    "laps5_512": (132, [(0.09426666708080467, 1.0811650842306748), (4.3049804697726275, 2.3534273450119105)],
                  [56, 80], [None, None], [78, 113], [140, 224], [37, 37]),
    "session_sep_512": (107, [(0.0888250272073492, 0.8032124862074852), (4.4417341984808445, 1.3375749830156565)],
                        [59, 74], [None, None], [68, 60], [92, 70], [40, 40]),
    "mixed_200": (120, [(2.589050054550171, 1.2122000455856323), (3.4203999042510986, 1.7319999933242798)],
                  [51, 61], [25, 17], [51, 61], [25, 17], [75, 75]),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers_on_the_oracle_grids(name):
    n_cent, kbots, line, line_cost, picks, pick_cost, reach = KNOWN[name]
    grid, cents, bots, (res, ox, oy) = oracle_case(name)
    assert len(cents) == n_cent and bots == kbots
    t = R.traversable(grid, 2)
    ccell, bcell, cost = A.costs(A.Space(grid, 2), cents.tolist(), bots, res, ox, oy)
    assert all(c is not None for c in ccell) and all(b is not None for b in bcell)      # every centroid and bot snaps
    got_line = greedy([tuple(c) for c in cents.tolist()], bots, 1.0)
    assert got_line == line
    assert [None if cost[b, k] == A.INF else int(cost[b, k]) for b, k in enumerate(got_line)] == line_cost
    out = A.assign(grid, cents, bots, res, ox, oy, 1.0)
    assert out["idx"].tolist() == picks and out["cost"].tolist() == pick_cost
    assert out["n_cost"].tolist() == reach and (out["status"] == R.OK).all()
    # what the issue is about: straight-line picks without a path, where reachable centroids were to be had
    if name != "mixed_200":
        assert None in line_cost
    # rule 5 again, independently: the waypoint is plan()'s for (bot, target)
    for b in range(len(bots)):
        want = R.plan(t, bots[b], tuple(out["xy"][b]), res, ox, oy)
        assert want["status"] == R.OK and want["cost"] == out["cost"][b]
        assert tuple(out["waypoint_cell"][b]) == tuple(want["cell"]) and tuple(out["waypoint"][b]) == tuple(want["xy"])


# ---- small hand-built grids (res 1, origin 0: the world position of a cell's centre is gx + 0.5) -------------------------
def run(grid, cents, bots, sep=0.0, **kw):
    kw.setdefault("clearance", 0)
    kw.setdefault("snap_radius", 2)
    return A.assign(np.asarray(grid, dtype=np.int8), cents, bots, 1.0, 0.0, 0.0, sep, **kw)


def test_tie_goes_to_the_lower_index_and_taken_is_skipped():
    g = np.zeros((7, 7), dtype=np.int8)
    cents = [(5.5, 3.5), (1.5, 3.5), (3.5, 6.5)]             # costs 10, 10, 15 from (3, 3)
    out = run(g, cents, [(3.5, 3.5)] * 4)
    assert out["idx"].tolist() == [0, 1, 2, -1] and out["cost"].tolist() == [10, 10, 15, A.INF]
    assert out["status"].tolist() == [R.OK, R.OK, R.OK, R.UNREACHABLE]
    assert np.isnan(out["xy"][3]).all() and tuple(out["waypoint_cell"][3]) == (-1, -1)
    out = run(g, cents[::-1], [(3.5, 3.5)])                  # the order of the list decides, not the position
    assert out["idx"].tolist() == [1]


def test_separation_blocks_a_neighbour():
    g = np.zeros((9, 9), dtype=np.int8)
    cents = [(2.5, 4.5), (1.5, 4.5), (7.5, 4.5)]             # costs 10, 15, 15 from (4, 4)
    assert run(g, cents, [(4.5, 4.5)] * 2, sep=0.0)["idx"].tolist() == [0, 1]
    assert run(g, cents, [(4.5, 4.5)] * 2, sep=1.0)["idx"].tolist() == [0, 1]       # 1.0 < 1.0 is false
    assert run(g, cents, [(4.5, 4.5)] * 2, sep=1.5)["idx"].tolist() == [0, 2]
    assert run(g, cents, [(4.5, 4.5)] * 3, sep=1.5)["status"].tolist() == [R.OK, R.OK, R.UNREACHABLE]


def test_bots_without_a_cell_and_walled_in_bots():
    g = np.full((12, 12), -1, dtype=np.int8)
    g[0:5, 0:5] = 0                                           # room A (with the frontier centroids)
    g[7:10, 7:10] = 0                                         # room B: no centroid in its component
    cents = [(0.5, 0.5), (4.5, 4.5)]
    bots = [(math.nan, 1.0), (11.5, 0.5), (8.5, 8.5), (math.inf, 0.0), (2.5, 2.5), (-3.0, 2.0), (2.5, 2.5)]
    out = run(g, cents, bots, snap_radius=1)
    assert out["status"].tolist() == [R.NO_START, R.NO_START, R.UNREACHABLE, R.NO_START, R.OK, R.NO_START, R.OK]
    assert out["idx"].tolist() == [-1, -1, -1, -1, 0, -1, 1]  # the bots after the failures are unaffected
    assert out["cost"].tolist() == [A.INF] * 4 + [14, A.INF, 14]
    assert out["n_cost"].tolist() == [0, 0, 0, 0, 2, 0, 2]


def test_two_centroids_on_one_cell_and_cost_zero():
    g = np.zeros((6, 6), dtype=np.int8)
    g[2, 2] = 100                                             # clearance 0: only the cell itself is blocked
    cents = [(3.25, 2.5), (3.75, 2.25), (2.5, 2.5)]           # 0 and 1 on cell (3, 2); 2 on the OCCUPIED cell: snaps to (2, 1)
    ccell, _, _ = A.costs(A.Space(g, 0), cents, [], 1.0, 0.0, 0.0, 2)
    assert ccell == [(3, 2), (3, 2), (2, 1)]
    out = run(g, cents, [(3.5, 2.5)] * 3)
    assert out["idx"].tolist() == [0, 1, 2] and out["cost"].tolist() == [0, 0, 10]
    # (3, 2) -> (2, 1) is no diagonal move: (2, 2) is blocked, so no corner is cut; S then W instead
    assert out["waypoint_cell"].tolist() == [[3, 2], [3, 2], [2, 1]]
    assert out["waypoint"].tolist() == [[3.5, 2.5], [3.5, 2.5], [2.5, 1.5]]


def test_by_path_differs_from_straight_line_behind_a_wall():
    g = np.zeros((9, 9), dtype=np.int8)
    g[0:8, 4] = 100                                           # a wall with a gap at the top row
    cents = [(5.5, 0.5), (0.5, 6.5)]
    bot = (3.5, 0.5)
    assert greedy(cents, [bot], 0.0) == [0]                   # two cells away through the wall
    out = run(g, cents, [bot])
    assert out["idx"].tolist() == [1] and out["cost"][0] == 3 * 7 + 3 * 5


# ---- MissionControl with a stub mapper -----------------------------------------------------------------------------------
class StubMapper:
    LINE = {1: (1.0, 1.0), 2: (-2.0, 0.0), 3: (4.0, 4.0)}
    PATH = {1: (1.5, 1.0), 2: (-2.0, 0.5)}                    # bot 3 has no reachable centroid

    def __init__(self):
        self.calls, self.plan_calls = [], []
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

    def assign_frontier_targets(self, bot_states, by_path=False, return_waypoints=False, **plan_params):
        self.calls.append((sorted(bot_states), by_path, return_waypoints, plan_params))
        if not by_path:
            return {b: self.LINE[b] for b in bot_states}
        targets = {b: self.PATH[b] for b in bot_states if b in self.PATH}
        if not return_waypoints:
            return targets
        return targets, {b: ((bot_states[b][0] + xy[0]) / 2, (bot_states[b][1] + xy[1]) / 2) for b, xy in targets.items()}

    def plan_paths(self, starts, goals, **kw):
        self.plan_calls.append(kw)
        s, g = np.array(starts, dtype=np.float64), np.array(goals, dtype=np.float64)
        return dict(status=np.zeros(len(s), dtype=np.int32), waypoint=(s + g) / 2)


def run_mc(**kw):
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    P = importlib.import_module(PKG_NAME + ".protocol")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    port = srv.getsockname()[1]
    stub = StubMapper()
    mc = fe.MissionControl(stub, sock=srv, max_agent=3, frontier_targets=True, **kw)
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
    bots[3].settimeout(0.1)
    if 3 not in sent:
        with pytest.raises(socket.timeout):
            bots[3].recv(64)
    for s in bots.values():
        s.close()
    mc.close()
    return mc, stub, sent, got, P


def test_mission_control_targets_by_path_sends_centroids():
    mc, stub, sent, got, P = run_mc(targets_by_path=True, plan_params=dict(clearance=3))
    assert stub.calls == [([1, 2, 3], True, False, dict(clearance=3))] and stub.plan_calls == []     # ONE call
    assert sent == {b: P.pack_target(*StubMapper.PATH[b]) for b in (1, 2)} and got == sent
    assert sent[1] == struct.pack("<4sff", b"TARG", 1.5, 1.0)
    assert mc.plan_stats == {"waypoint": 0, "centroid": 0}


def test_mission_control_targets_by_path_sends_waypoints():
    mc, stub, sent, got, P = run_mc(targets_by_path=True, plan_paths=True, plan_params=dict(clearance=3, lookahead=50))
    assert stub.calls == [([1, 2, 3], True, True, dict(clearance=3, lookahead=50))] and stub.plan_calls == []
    poses = {b: mc.bot_pose[b] for b in (1, 2)}
    want = {b: P.pack_target((poses[b][0] + StubMapper.PATH[b][0]) / 2, (poses[b][1] + StubMapper.PATH[b][1]) / 2)
            for b in (1, 2)}
    assert sent == want and got == sent
    assert mc.plan_stats == {"waypoint": 2, "centroid": 0}          # never a centroid fall-back


def test_targets_by_path_needs_frontier_targets():
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    with pytest.raises(ValueError):
        fe.MissionControl(StubMapper(), sock=srv, targets_by_path=True)
    srv.close()


def test_datagrams_unchanged_with_the_flag_off():
    mc, stub, sent, got, P = run_mc()
    assert mc.targets_by_path is False
    assert stub.calls == [([1, 2, 3], False, False, {})] and stub.plan_calls == []
    assert sent == {b: P.pack_target(*StubMapper.LINE[b]) for b in (1, 2, 3)} and got == sent
    mc, stub, sent, got, P = run_mc(plan_paths=True, plan_params=dict(lookahead=9))
    assert stub.calls == [([1, 2, 3], False, False, {})] and stub.plan_calls == [dict(lookahead=9)]
    poses = {b: mc.bot_pose[b] for b in (1, 2, 3)}
    assert sent == {b: P.pack_target((poses[b][0] + StubMapper.LINE[b][0]) / 2, (poses[b][1] + StubMapper.LINE[b][1]) / 2)
                    for b in (1, 2, 3)} and got == sent
    assert mc.plan_stats == {"waypoint": 3, "centroid": 0}
