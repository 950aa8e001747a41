"""MissionControl(targets_by_territory=True) over a stand-in mapper, without a GPU: the datagrams sent, plan_stats, the
territory it keeps, and the combinations it refuses."""
import importlib
import socket
import struct
import time

import numpy as np
import pytest

from conftest import PKG_NAME


class StubMapper:
    ox, oy, res = -5.0, -4.0, 0.05
    TARGET = {1: (1.5, 1.0), 2: (-2.0, 0.5)}                  # bot 3 owns no centroid
    SHARE = {1: (1200, (10, 20, 49, 59)), 2: (7, (100, 100, 100, 106)), 3: (0, None)}

    def __init__(self):
        self.calls = []
        self._acc = self._pose = None

    def ingest_array(self, buf, lens, times):
        rec = np.frombuffer(np.ascontiguousarray(buf[:, :42]).tobytes(), dtype=[("m", "S4"), ("a", "u1"), ("x", "<f4"),
                                                                               ("y", "<f4"), ("rest", "V29")])
        self._acc = ((lens == 42) & (rec["m"] == b"QSRL")).astype(np.uint8)
        self._pose = np.stack([rec["x"].astype(np.float64), rec["y"].astype(np.float64), np.zeros(len(rec))], axis=1)

    def last_batch(self):
        return self._acc, self._pose

    def assign_frontier_targets(self, bot_states, by_path=False, return_waypoints=False, by_territory=False,
                                return_territory=False, **plan_params):
        self.calls.append((sorted(bot_states), by_path, by_territory, return_waypoints, return_territory, plan_params))
        assert by_territory and return_territory and not by_path
        out = [{b: self.TARGET[b] for b in bot_states if b in self.TARGET}]
        if return_waypoints:
            out.append({b: ((bot_states[b][0] + xy[0]) / 2, (bot_states[b][1] + xy[1]) / 2) for b, xy in out[0].items()})
        out.append({b: self.SHARE[b] for b in bot_states})
        return tuple(out)


def run_mc(**kw):
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    P = importlib.import_module(PKG_NAME + ".protocol")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    port = srv.getsockname()[1]
    stub = StubMapper()
    mc = fe.MissionControl(stub, sock=srv, max_agent=3, frontier_targets=True, targets_by_territory=True, **kw)
    assert mc.territory == {}
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
    with pytest.raises(socket.timeout):
        bots[3].recv(64)
    for s in bots.values():
        s.close()
    mc.close()
    return mc, stub, sent, got, P


WORLD = {1: (1200, (-5.0 + 10 * 0.05, -4.0 + 20 * 0.05, -5.0 + 50 * 0.05, -4.0 + 60 * 0.05)),
         2: (7, (-5.0 + 100 * 0.05, -4.0 + 100 * 0.05, -5.0 + 101 * 0.05, -4.0 + 107 * 0.05)), 3: (0, None)}


def test_sends_centroids_and_keeps_the_territory():
    mc, stub, sent, got, P = run_mc(plan_params=dict(clearance=3))
    assert stub.calls == [([1, 2, 3], False, True, False, True, dict(clearance=3))]          # ONE call
    assert sent == {b: P.pack_target(*StubMapper.TARGET[b]) for b in (1, 2)} and got == sent
    assert sent[1] == struct.pack("<4sff", b"TARG", 1.5, 1.0)
    assert mc.plan_stats == {"waypoint": 0, "centroid": 0}
    assert mc.territory == WORLD


def test_sends_waypoints_with_plan_paths():
    mc, stub, sent, got, P = run_mc(plan_paths=True, plan_params=dict(clearance=3, lookahead=50))
    assert stub.calls == [([1, 2, 3], False, True, True, True, dict(clearance=3, lookahead=50))]
    poses = {b: mc.bot_pose[b] for b in (1, 2)}
    want = {b: P.pack_target((poses[b][0] + StubMapper.TARGET[b][0]) / 2, (poses[b][1] + StubMapper.TARGET[b][1]) / 2)
            for b in (1, 2)}
    assert sent == want and got == sent
    assert mc.plan_stats == {"waypoint": 2, "centroid": 0}
    assert mc.territory == WORLD


def test_refused_combinations():
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    pkg = importlib.import_module(PKG_NAME)
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    with pytest.raises(ValueError, match="needs frontier_targets"):
        fe.MissionControl(StubMapper(), sock=srv, targets_by_territory=True)
    with pytest.raises(ValueError, match="excludes targets_by_path"):
        fe.MissionControl(StubMapper(), sock=srv, frontier_targets=True, targets_by_territory=True, targets_by_path=True)
    srv.close()
    # assign_frontier_targets refuses both rankings at once before it touches the device
    m = pkg.QuasarMapper.__new__(pkg.QuasarMapper)
    with pytest.raises(ValueError, match="exclude each other"):
        pkg.QuasarMapper.assign_frontier_targets(m, {1: (0.0, 0.0)}, by_path=True, by_territory=True)
    with pytest.raises(ValueError, match="needs by_territory"):
        pkg.QuasarMapper.assign_frontier_targets(m, {1: (0.0, 0.0)}, return_territory=True)
