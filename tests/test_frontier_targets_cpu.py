"""TARG egress without a GPU: the packet, the C ABI declaration, and MissionControl's target timer
(dual_bot_mapper.py:947-996, commented out in the reference) on localhost sockets with a stub mapper whose
assignment is a plain restatement of the reference's greedy loop."""
import importlib
import math
import os
import re
import socket
import struct
import time

import numpy as np

from conftest import PKG_NAME, ROOT
from walk_ops import greedy


class StubMapper:
    CENTS = [(1.0, 1.0), (1.5, 1.0), (-2.0, 0.0)]

    def __init__(self):
        self.assign_calls = []
        self._acc = self._pose = None

    def ingest_array(self, buf, lens, times):
        rec = np.frombuffer(np.ascontiguousarray(buf[:, :42]).tobytes(), dtype=[("m", "S4"), ("a", "u1"), ("x", "<f4"),
                                                                               ("y", "<f4"), ("rest", "V29")])
        self._acc = ((lens == 42) & (rec["m"] == b"QSRL") & (rec["a"] >= 1) & (rec["a"] <= 4)).astype(np.uint8)
        self._pose = np.stack([rec["x"].astype(np.float64), rec["y"].astype(np.float64), np.zeros(len(rec))], axis=1)

    def last_batch(self):
        return self._acc, self._pose

    def zone(self, bot):
        return (0.0, 0.0, 1.0, 1.0)

    def zone_packet(self, bot, online=True):
        return struct.pack("<4sffff", b"ZONE", 0.0, 0.0, 1.0, 1.0)

    def assign_frontier_targets(self, bot_states, separation=1.0):
        self.assign_calls.append(list(bot_states))
        bots = sorted(bot_states)
        got = greedy(self.CENTS, [bot_states[b] for b in bots], separation)
        return {b: self.CENTS[i] for b, i in zip(bots, got) if i >= 0}


def test_pack_target():
    P = importlib.import_module(PKG_NAME + ".protocol")
    for x, y in ((1.25, -3.5), (0.1, 1e6), (-0.0, 7.3)):
        assert P.pack_target(x, y) == struct.pack("<4sff", b"TARG", x, y)
    assert len(P.pack_target(0.0, 0.0)) == P.TARGET_SIZE == 12


def test_symbol_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    assert re.search(r"int qs_frontier_targets\(", txt) and "#define QS_FT_MAX_BOTS 1024" in txt
    lib = importlib.import_module(PKG_NAME + "._lib")
    assert "qs_frontier_targets" in lib.SIGNATURES and lib.QS_FT_MAX_BOTS == 1024
    pkg = importlib.import_module(PKG_NAME)
    pkg.build()
    assert hasattr(pkg.load(), "qs_frontier_targets")


def test_greedy_restatement():
    # ties go to the lower index, the taken centroid is skipped, separation blocks the neighbour
    c = [(1.0, 0.0), (-1.0, 0.0), (0.0, 0.5), (5.0, 5.0)]
    assert greedy(c, [(0.0, 0.0), (0.0, 0.0), (0.0, 0.0)], 0.0) == [2, 0, 1]
    assert greedy(c, [(0.0, 0.0), (0.0, 0.0)], 1.2) == [2, 3]
    assert greedy(c, [(math.nan, 0.0), (math.inf, 0.0), (0.0, 0.0)], 1.0) == [-1, -1, 2]


def test_mission_control_target_timer():
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    P = importlib.import_module(PKG_NAME + ".protocol")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    port = srv.getsockname()[1]
    stub = StubMapper()
    mc = fe.MissionControl(stub, sock=srv, max_agent=4, frontier_targets=True)
    assert mc.bot_ports == {1: 8888, 2: 8889, 3: 8890, 4: 8891}                  # 8887 + bot (:759)
    bots = {b: socket.socket(socket.AF_INET, socket.SOCK_DGRAM) for b in (1, 2, 3)}
    for s in bots.values():
        s.bind(("127.0.0.1", 0)); s.settimeout(1.0)
    mc.bot_ports = {b: bots[b].getsockname()[1] if b in bots else 8887 + b for b in range(1, 5)}
    # bots 3, 1, 2 report in that order; bot 2 twice (its LAST pose counts); bot 4 never
    for b, x, y in ((3, 0.9, 1.1), (1, 1.4, 1.0), (2, 9.0, 9.0), (2, -1.9, 0.2)):
        bots[b].sendto(P.pack_packet(b, x, y, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5), ("127.0.0.1", port))
        time.sleep(0.02)
    time.sleep(0.05)
    t0 = 2000.0
    mc.last_target_send = t0
    assert mc.poll(now=t0) == 4
    assert mc.bot_pose[2] == (float(np.float32(-1.9)), float(np.float32(0.2)))
    # the 3 s cadence, strict >
    assert mc.target_tick(now=t0 + 3.0) == {} and stub.assign_calls == []
    sent = mc.target_tick(now=t0 + 3.01)
    assert stub.assign_calls == [[1, 2, 3]]                                      # ascending bot id
    want = stub.assign_frontier_targets({1: mc.bot_pose[1], 2: mc.bot_pose[2], 3: mc.bot_pose[3]})
    assert sent == {b: P.pack_target(*xy) for b, xy in want.items()}
    assert set(sent) == {1, 2} and 3 not in sent                                 # bot 3: everything near it is taken
    for b in (1, 2):
        assert bots[b].recv(64) == sent[b]
    bots[3].settimeout(0.1)
    try:
        bots[3].recv(64)
        assert False, "bot 3 got no target and must get no packet"
    except socket.timeout:
        pass
    assert mc.target_tick(now=t0 + 4.0) == {}                                    # the timer restarted at t0 + 3.01
    # an offline bot is skipped; a bot without a known address is assigned but not sent to
    mc.online[1] = False
    mc.bot_addrs[2] = None
    sent = mc.target_tick(now=t0 + 6.1)
    assert stub.assign_calls[-1] == [2, 3] and set(sent) == {2, 3}
    assert bots[3].recv(64) == sent[3]
    bots[2].settimeout(0.1)
    try:
        bots[2].recv(64)
        assert False, "bot 2 has no address and must get no packet"
    except socket.timeout:
        pass
    assert mc.target_tick(now=t0 + 6.2, force=True) != {}
    for s in bots.values():
        s.close()
    mc.close()


def test_targets_off_by_default():
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    stub = StubMapper()
    mc = fe.MissionControl(stub, sock=srv)
    assert mc.frontier_targets is False
    mc.step(now=time.time() + 100.0)
    assert stub.assign_calls == []
    mc.close()
