"""Frontier gain without a GPU: the C ABI declarations, the CPU restatement (gain_rules.py) on the oracle's grids of the
four golden sessions with known answers and on small hand-built grids, and MissionControl's egress with a stub mapper."""
import functools
import importlib
import os
import re
import socket

import numpy as np
import pytest

import assign_rules as A
import gain_rules as G
import plan_rules as R
from conftest import PKG_NAME, ROOT
from test_targets_by_path_cpu import StubMapper, oracle_case, run_mc


def test_symbols_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    assert re.search(r"int qs_frontier_gain\(", txt) and re.search(r"int qs_frontier_targets_by_gain\(", txt)
    rules = txt[txt.index("frontier gain"):]
    assert all(f" G{i} " in rules for i in range(1, 8))
    assert "#define QS_GAIN_MAX_RANGE 64" in txt and "#define QS_GAIN_DEFAULT_RANGE 24" in txt
    assert "#define QS_GAIN_DEFAULT_BIAS 120u" in txt
    lib = importlib.import_module(PKG_NAME + "._lib")
    assert len(lib.SIGNATURES["qs_frontier_gain"][1]) == 7
    assert len(lib.SIGNATURES["qs_frontier_targets_by_gain"][1]) == len(lib.SIGNATURES["qs_frontier_targets_by_path"][1]) + 2
    assert (lib.QS_GAIN_MAX_RANGE, lib.QS_GAIN_DEFAULT_RANGE, lib.QS_GAIN_DEFAULT_BIAS) == (G.MAX_RANGE, G.DEFAULT_RANGE, G.DEFAULT_BIAS)
    import ctypes as C
    assert C.sizeof(lib.QsGainParams) == 16
    pkg = importlib.import_module(PKG_NAME)
    pkg.build()
    L = pkg.load()
    assert hasattr(L, "qs_frontier_gain") and hasattr(L, "qs_frontier_targets_by_gain")


# ---- the oracle's grids: known answers (range 24, clearance 2, snap 10, separation 1.0) ------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    grid, cents, bots, geo = oracle_case(name)
    views, gain, ties = G.frontier_gain(grid)
    return grid, cents, bots, geo, views, gain, ties


# name: clusters, gain (min, median, max, sum), clusters with two members at the smallest distance, then per rule
# (picks, costs, gains of the picks): by path cost (assign_rules), bias 0, bias 120
KNOWN = {
    "session_512": (111, (73, 596.0, 1370, 70086), 5,
                    ([72, 69], [92, 80], [179, 101]), ([87, 96], [131, 86], [632, 559]), ([87, 96], [131, 86], [632, 559])),
    "laps5_512": (132, (20, 772.5, 1457, 97509), 6,
                  ([78, 113], [140, 224], [460, 159]), ([76, 107], [145, 377], [644, 1322]), ([76, 107], [145, 377], [644, 1322])),
    "session_sep_512": (107, (18, 622.0, 1364, 66322), 5,
                        ([68, 60], [92, 70], [179, 18]), ([83, 17], [131, 319], [632, 1228]), ([83, 17], [131, 319], [632, 1228])),
    "mixed_200": (120, (202, 778.5, 1503, 94807), 8,
                  ([51, 61], [25, 17], [682, 515]), ([51, 61], [25, 17], [682, 515]), ([6, 89], [60, 39], [1177, 799])),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers_on_the_oracle_grids(name):
    n, stats, n_ties, by_path, bias0, bias120 = KNOWN[name]
    grid, cents, bots, (res, ox, oy), views, gain, ties = case(name)
    cl, size = G.clusters(grid, 3)
    assert len(cl) == n == len(cents)
    assert (np.array(G.centroids(cl, size, res, ox, oy)) == cents).all()          # G1: the oracle's list and order
    assert (int(gain.min()), float(np.median(gain)), int(gain.max()), int(gain.sum())) == stats
    assert gain.min() >= 1                                                         # G4
    assert sum(t > 1 for t in ties) == n_ties and 5 <= n_ties <= 8                 # G2's tie-break is exercised
    for (gx, gy), m in zip(views.tolist(), cl):
        assert gy * size + gx in m and grid[gy, gx] == 0                           # a member: a FREE interior cell
        assert 1 <= gx < size - 1 and 1 <= gy < size - 1
    path = A.assign(grid, cents, bots, res, ox, oy, 1.0)
    assert (path["idx"].tolist(), path["cost"].tolist(), [int(gain[k]) for k in path["idx"]]) == by_path
    for bias, want in ((0, bias0), (G.DEFAULT_BIAS, bias120)):
        out = G.assign(grid, cents, gain, bots, res, ox, oy, 1.0, bias=bias)
        assert (out["idx"].tolist(), out["cost"].tolist(), out["gain"].tolist()) == want, bias
        assert (out["status"] == R.OK).all()
        t = R.traversable(grid, 2)
        for b in range(len(bots)):                                                 # G7: the waypoint is plan()'s
            p = R.plan(t, bots[b], tuple(out["xy"][b]), res, ox, oy)
            assert p["status"] == R.OK and p["cost"] == out["cost"][b]
            assert tuple(out["waypoint_cell"][b]) == tuple(p["cell"]) and tuple(out["waypoint"][b]) == tuple(p["xy"])
    if name == "mixed_200":
        assert bias0 == by_path and bias120[0] != by_path[0]
    else:
        assert bias120[0][0] != by_path[0][0]                                      # the first bot's pick moves


def test_session_sep_second_bot_trades_cost_for_gain():
    _, _, _, _, _, gain, _ = case("session_sep_512")
    assert KNOWN["session_sep_512"][3][1][1] == 70 and gain[60] == 18
    assert KNOWN["session_sep_512"][5][1][1] == 319 and gain[17] == 1228


def test_vectorised_gain_equals_the_direct_loop():
    grid, _, _, _, views, gain, _ = case("mixed_200")
    assert [G.gain_direct(grid, tuple(v), 24) for v in views.tolist()] == gain.tolist()
    for rng in (1, 8):
        assert [G.gain_direct(grid, tuple(v), rng) for v in views.tolist()] == G.gains(grid, views, rng).tolist()


def test_walk_is_not_reversal_symmetric():
    """Walking t -> v instead changes the gain of many clusters (the issue counted 85 to 111 per map)."""
    grid, _, _, _, views, gain, _ = case("session_512")
    size = grid.shape[0]

    def reversed_gain(v, rng=24):
        vx, vy = v
        n = 0
        for ty in range(max(0, vy - rng), min(size, vy + rng + 1)):
            for tx in range(max(0, vx - rng), min(size, vx + rng + 1)):
                if (tx - vx) ** 2 + (ty - vy) ** 2 <= rng * rng and grid[ty, tx] == -1:
                    n += all(grid[y, x] != 100 for x, y in R.bresenham(tx, ty, vx, vy)[1:])
        return n
    changed = sum(reversed_gain(tuple(v)) != int(g) for v, g in zip(views.tolist(), gain.tolist()))
    assert 85 <= changed <= 111


# ---- small hand-built grids --------------------------------------------------------------------------------------------
def test_viewpoint_tie_goes_to_the_lower_index():
    size = 16
    u = [y * size + x for x, y in ((4, 4), (4, 5), (4, 6), (5, 6), (6, 6), (6, 5), (6, 4))]       # a U round (5, 5)
    v, ties = G.viewpoint(sorted(u), size)
    assert (sum(i % size for i in u) // 7, sum(i // size for i in u) // 7) == (5, 5) and 5 * size + 5 not in u
    assert ties == 3 and v == (4, 5)                                                             # (4, 5), (6, 5), (5, 6)


def test_shadow_range_and_grid_edge():
    g = np.full((40, 40), -1, dtype=np.int8)
    g[20, 18:21] = 0                                      # three FREE cells in an unknown world: one cluster
    cl, size = G.clusters(g, 3)
    assert cl == [[20 * 40 + 18, 20 * 40 + 19, 20 * 40 + 20]]
    assert G.viewpoint(cl[0], size) == ((19, 20), 1)
    disc = lambda r: sum(dx * dx + dy * dy <= r * r for dx in range(-r, r + 1) for dy in range(-r, r + 1)) - 1
    assert G.gains(g, [(19, 20)], 1).tolist() == [2]                                  # N and S; E and W are FREE
    assert G.gains(g, [(19, 20)], 8).tolist() == [disc(8) - 2]
    assert G.gains(g, [(19, 20)], 24).tolist() == [G.gain_direct(g, (19, 20), 24)]    # clipped by the grid on every side
    g[22, 17:22] = 100                                    # a wall two rows up: itself no target, and it casts a shadow
    lit = G.gains(g, [(19, 20)], 8)[0]
    assert lit == G.gain_direct(g, (19, 20), 8) and lit < disc(8) - 2 - 5
    g[22, 17:22] = 0                                      # FREE cells are no targets but hide nothing
    assert G.gains(g, [(19, 20)], 8).tolist() == [disc(8) - 2 - 5]


def test_order_is_exact_and_ties_go_to_cost_then_index():
    assert G.before(10, 3, 5, 20, 6, 2, 0)                # equal ratios: the smaller cost first
    assert not G.before(20, 6, 2, 10, 3, 5, 0)
    assert G.before(10, 3, 2, 10, 3, 5, 7) and not G.before(10, 3, 5, 10, 3, 2, 7)    # then the lower k
    big = (1 << 32) - 2
    assert G.before(big, 16641, 1, big, 16640, 0, 1 << 31)                          # 64-bit products, no rounding
    assert G.before(0, 1, 9, 1, 1000, 0, 0) and not G.before(0, 1, 9, 1, 1000, 0, 1)  # bias 0: cost 0 always wins


# ---- MissionControl with a stub mapper -----------------------------------------------------------------------------------
class GainStub(StubMapper):
    def assign_frontier_targets(self, bot_states, by_path=False, return_waypoints=False, by_gain=False, **params):
        if by_gain:
            self.calls.append((sorted(bot_states), "gain", return_waypoints, params))
            return super().assign_frontier_targets(bot_states, True, return_waypoints)
        return super().assign_frontier_targets(bot_states, by_path, return_waypoints, **params)


def run_gain_mc(monkeypatch, **kw):
    import test_targets_by_path_cpu as T
    monkeypatch.setattr(T, "StubMapper", GainStub)
    return run_mc(**kw)


def test_mission_control_targets_by_gain(monkeypatch):
    mc, stub, sent, got, P = run_gain_mc(monkeypatch, targets_by_gain=True, plan_params=dict(clearance=3),
                                         gain_params=dict(gain_range=12, gain_bias=0))
    assert stub.calls[0] == ([1, 2, 3], "gain", False, dict(clearance=3, gain_range=12, gain_bias=0)) and stub.plan_calls == []
    assert sent == {b: P.pack_target(*StubMapper.PATH[b]) for b in (1, 2)} and got == sent
    assert mc.plan_stats == {"waypoint": 0, "centroid": 0}
    mc, stub, sent, got, P = run_gain_mc(monkeypatch, targets_by_gain=True, plan_paths=True)
    assert stub.calls[0] == ([1, 2, 3], "gain", True, {}) and stub.plan_calls == []
    poses = {b: mc.bot_pose[b] for b in (1, 2)}
    assert sent == {b: P.pack_target((poses[b][0] + StubMapper.PATH[b][0]) / 2, (poses[b][1] + StubMapper.PATH[b][1]) / 2)
                    for b in (1, 2)} and got == sent
    assert mc.plan_stats == {"waypoint": 2, "centroid": 0}


def test_targets_by_gain_exclusivity():
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    for kw in (dict(), dict(frontier_targets=True, targets_by_path=True), dict(frontier_targets=True, targets_by_territory=True)):
        with pytest.raises(ValueError):
            fe.MissionControl(StubMapper(), sock=srv, targets_by_gain=True, **kw)
    srv.close()
    mapper = importlib.import_module(PKG_NAME + ".mapper")
    for kw in (dict(by_path=True), dict(by_territory=True)):
        with pytest.raises(ValueError):
            mapper.QuasarMapper.assign_frontier_targets(None, {1: (0.0, 0.0)}, by_gain=True, **kw)
