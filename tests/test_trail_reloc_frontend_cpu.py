"""MissionControl(match_packets={"relocalise": ...}) with a stub in place of the mapper and a socket that delivers what is queued:
a bot that comes online without a transform is first located from its trails -- held across rounds, then rewritten by the found
transform and mapped in arrival order, or mapped as it is after the last try."""
import importlib
import math

import numpy as np

import trail_reloc_rules as KR
import trail_rules as TR
from conftest import load_pkg


def _mods():
    pkg = load_pkg()
    return importlib.import_module(pkg.__name__ + ".udp_frontend"), importlib.import_module(pkg.__name__ + ".protocol")


class Sock:
    """A socket whose queued datagrams arrive at the next poll."""

    def __init__(self):
        self.queue = []

    def setblocking(self, flag):
        pass

    def recvfrom_into(self, view, nbytes):
        if not self.queue:
            raise BlockingIOError
        d = self.queue.pop(0)
        view[:len(d)] = d
        return len(d), ("127.0.0.1", 4000)

    def sendto(self, data, addr):
        pass

    def close(self):
        pass


class StubMapper:
    """Records every call.  relocalise_trails answers from `found` (one dict of result fields per call, or nothing: not
    accepted); the anchor is the trail's last record."""

    def __init__(self, found=None, shift=(0.0, 0.0)):
        self.calls, self.found, self.shift = [], list(found or []), shift
        self.relocs, self.ingested = [], []

    def sweep_pose_shift(self, bot):
        return self.shift

    def ingest_array(self, buf, lens, times):
        self.calls.append(("packets", len(buf)))
        self.ingested.append(np.array(buf))
        lens = np.asarray(lens)
        self._acc = ((lens == 42) | (lens == 41)).astype(np.uint8)
        self._pose = np.ascontiguousarray(buf[:, 5:17]).view("<f4").astype(np.float64)

    def last_batch(self):
        return self._acc, self._pose

    def match_trails(self, buf, gsize, lengths=None, travel=None, params=None, rotations=False):
        self.calls.append(("trails", [int(g) for g in gsize]))
        out = np.zeros(len(gsize), dtype=TR.TRAIL_DTYPE)
        out["anchor"] = np.asarray(gsize) - 1
        return out

    def relocalise_trails(self, buf, gsize, lengths=None, travel=None, params=None, rotations=False):
        self.calls.append(("locate", [int(g) for g in gsize]))
        self.relocs.append((np.array(buf), list(gsize), np.array(lengths), travel, params))
        out = np.zeros(len(gsize), dtype=KR.TRAIL_RELOC_DTYPE)
        last = buf[-1]
        out[0]["agent"], out[0]["anchor"], out[0]["records"] = last[4], gsize[0] - 1, gsize[0]
        out[0]["ax"], out[0]["ay"] = (float(v) for v in last[5:13].view("<f4"))
        for k, v in (self.found.pop(0) if self.found else {}).items():
            out[0][k] = v
        return out


def _fields(buf):
    return np.ascontiguousarray(buf[:, 5:17]).view("<f4").reshape(-1, 3)


def _mc(fe, m, **mp):
    sock = Sock()
    return fe.MissionControl(m, sock=sock, match_packets=dict(dict(trail=2, hold=100.0), **mp)), sock


def _send(P, sock, agent, x, y=0.0, yaw=0.0):
    sock.queue.append(P.pack_packet(agent, x, y, yaw, 1, 2, 0.5, 0.6, 0.7, 0.8, 0))


def test_without_relocalise_the_stub_sees_todays_calls():
    fe, P = _mods()
    seen = []
    for mp in (dict(), dict(relocalise=False)):
        m = StubMapper()
        mc, sock = _mc(fe, m, **mp)
        for k in range(2):
            _send(P, sock, 1, 0.1 * k)
            _send(P, sock, 2, 5.0 + k)
        assert mc.poll(now=1.0) == 4
        _send(P, sock, 2, 7.0)
        mc.poll(now=2.0)
        mc.close()
        assert m.calls == [("trails", [2, 2]), ("packets", 4), ("trails", [1]), ("packets", 1)]
        assert mc.trail_stats == dict(held=5, tried=3, accepted=0, moved=0, rewritten=0)
        seen.append([b.tobytes() for b in m.ingested])
    assert seen[0] == seen[1]


def test_the_first_bot_is_never_located_and_the_second_is_held_then_moved():
    """Bot 2 reports in a frame of its own.  Its first trail is refused and stays held; the second is accepted with yaw 90 degrees,
    the anchor's fields (6, 1) set down at (2, 3), and the ingest adds (0.5, -0.25) itself.  So fields (x, y) map to
    (2 - (y - 1) - 0.5, 3 + (x - 6) + 0.25): all four held records in arrival order, then bot 2's trails are matched as bot 1's."""
    fe, P = _mods()
    yaw = 2 * math.pi / 180 * 45
    m = StubMapper(found=[{}, dict(accepted=1, status=0, x=2.0, y=3.0, yaw=yaw)], shift=(0.5, -0.25))
    mc, sock = _mc(fe, m, relocalise=dict(n_rot=90, min_hits=20), tries=3)
    _send(P, sock, 1, 0.0); _send(P, sock, 2, 5.0, 1.0, 0.2); _send(P, sock, 1, 0.1); _send(P, sock, 2, 5.5, 1.0, 0.2)
    mc.poll(now=1.0)
    assert m.calls == [("locate", [2]), ("trails", [2]), ("packets", 2)]      # bot 1: matched and mapped; bot 2: held
    assert m.relocs[0][4] == dict(n_rot=90, min_hits=20) and (m.ingested[0][:, 4] == 1).all()
    assert mc.trail_stats["reloc_tried"] == 1 and 2 in mc._locating and 2 not in mc._trail_T
    _send(P, sock, 2, 5.75, 1.0, 0.2); _send(P, sock, 2, 6.0, 1.0, 0.2)
    mc.poll(now=2.0)
    assert m.calls[3:] == [("locate", [2]), ("packets", 4)]
    assert (mc.trail_stats["reloc_tried"], mc.trail_stats["reloc_accepted"], mc.trail_stats["reloc_gave_up"]) == (2, 1, 0)
    assert mc.trail_relocs[2]["accepted"] == 1 and mc.trail_relocs[2]["ax"] == 6.0
    got = _fields(m.ingested[1])
    c, s = math.cos(yaw), math.sin(yaw)
    for k, x in enumerate((5.0, 5.5, 5.75, 6.0)):
        ex, ey = 2.0 + (c * (x - 6.0) - s * 0.0) - 0.5, 3.0 + (s * (x - 6.0) + c * 0.0) + 0.25
        assert abs(got[k, 0] - ex) < 1e-5 and abs(got[k, 1] - ey) < 1e-5 and abs(got[k, 2] - (0.2 + yaw)) < 1e-5
    assert abs(got[0, 1] - 2.25) < 1e-5 and abs(got[3, 0] - 1.5) < 1e-5        # 90 degrees: (x - 6) turns onto y
    assert mc.trail_stats["rewritten"] == 4
    _send(P, sock, 2, 6.25, 1.0, 0.2); _send(P, sock, 2, 6.5, 1.0, 0.2)
    mc.poll(now=3.0)
    assert m.calls[5:] == [("trails", [2]), ("packets", 2)]                   # located: from now on matched as today
    mc.close()


def test_giving_up_after_tries_and_located_again_after_offline():
    fe, P = _mods()
    m = StubMapper()
    mc, sock = _mc(fe, m, relocalise=True, tries=2)
    _send(P, sock, 1, 0.0); _send(P, sock, 1, 0.1)
    mc.poll(now=1.0)                                               # bot 1 is the first ever seen: the map's frame
    assert m.calls == [("trails", [2]), ("packets", 2)] and not mc._locating
    for k in range(4):
        _send(P, sock, 2, 5.0 + k)
    mc.poll(now=2.0)                                               # two rounds: two tries, then everything held is mapped as it is
    assert m.calls[2:] == [("locate", [2]), ("locate", [2]), ("packets", 4)]
    assert m.relocs[0][4] is None
    assert _fields(m.ingested[1])[:, 0].tolist() == [5.0, 6.0, 7.0, 8.0] and mc.trail_stats["rewritten"] == 0
    assert (mc.trail_stats["reloc_tried"], mc.trail_stats["reloc_accepted"], mc.trail_stats["reloc_gave_up"]) == (2, 0, 1)
    _send(P, sock, 2, 9.0); _send(P, sock, 2, 10.0)
    mc.poll(now=3.0)
    assert m.calls[5:] == [("trails", [2]), ("packets", 2)]                   # left alone
    assert mc.heartbeat(now=3.0 + P.HEARTBEAT_TIMEOUT + 1.0) == [1, 2]
    _send(P, sock, 2, 11.0); _send(P, sock, 2, 12.0)
    mc.poll(now=100.0)                                             # back from offline: located again
    assert m.calls[7:] == [("locate", [2])] and mc._locating[2][0] == 1
    _send(P, sock, 1, 0.2); _send(P, sock, 1, 0.3)
    mc.poll(now=101.0)                                             # bot 1 is back too, and still is not located
    assert m.calls[8:] == [("trails", [2]), ("packets", 2)]
    mc.close()                                                     # what bot 2 still holds is mapped as it is
    assert m.calls[10:] == [("packets", 2)] and mc.trail_stats["reloc_gave_up"] == 2


def test_bots_names_who_is_located():
    fe, P = _mods()
    m = StubMapper()
    mc, sock = _mc(fe, m, relocalise=True, bots=[1])
    _send(P, sock, 1, 0.0); _send(P, sock, 1, 0.1); _send(P, sock, 2, 5.0); _send(P, sock, 2, 5.1)
    mc.poll(now=1.0)
    assert m.calls == [("locate", [2]), ("trails", [2]), ("packets", 2)]
    assert (m.relocs[0][0][:, 4] == 1).all() and (m.ingested[0][:, 4] == 2).all()
    mc.close()


def test_travel_is_what_the_trail_needs_rounded_up_and_capped():
    fe, P = _mods()
    m = StubMapper()
    mc, sock = _mc(fe, m, relocalise=True, trail=3, travel=1.0, tries=9)
    _send(P, sock, 1, 0.0); _send(P, sock, 1, 0.1); _send(P, sock, 1, 0.2)
    for xs in ((5.0, 5.3, 5.6), (0.0, 3.0, 5.9), (4.0, 4.0, 4.0), (1.0, 1.5, 1.25)):
        for x in xs:
            _send(P, sock, 2, x, 2.0)
    mc.poll(now=1.0)
    # 0.6 m -> 0.75; 5.9 m -> the cap; 0 -> 0; exactly 0.25 stays
    assert [r[3] for r in m.relocs] == [0.75, 1.0, 0.0, 0.25]
    mc.close()
