"""MissionControl(match_packets=...) over a loopback socket, a stub in place of the mapper: packets are held back, flushed by
count and by age, matched in one call and mapped in one call per flush, in arrival order, under the bot's composed transform."""
import importlib
import math
import socket
import time

import numpy as np
import pytest

import trail_rules as TR
from conftest import load_pkg


def _mods():
    pkg = load_pkg()
    return importlib.import_module(pkg.__name__ + ".udp_frontend"), importlib.import_module(pkg.__name__ + ".protocol")


class StubMapper:
    """Records every call.  match_trails answers from `answers` (a list of per-call lists of dicts of match fields), or
    unaccepted zeros; the anchor is each group's last record, shifted as sweep_pose_shift says."""

    def __init__(self, answers=None, shift=(0.0, 0.0)):
        self.calls, self.answers, self.shift = [], list(answers or []), shift
        self.trails, self.ingested = [], []

    def sweep_pose_shift(self, bot):
        return self.shift

    def ingest_array(self, buf, lens, times):
        self.calls.append(("packets", len(buf)))
        self.ingested.append((np.array(buf), np.array(lens), np.array(times)))
        lens = np.asarray(lens)
        self._acc = (((lens == 42) | (lens == 41)) & (buf[:, :4] == np.frombuffer(b"QSRL", np.uint8)).all(axis=1)).astype(np.uint8)
        f = np.ascontiguousarray(buf[:, 5:17]).view("<f4").astype(np.float64)
        self._pose = f + np.array([self.shift[0], self.shift[1], 0.0])

    def last_batch(self):
        return self._acc, self._pose

    def ingest_sweeps(self, buf, lens=None, seq0=None, match=None, check=None):
        self.calls.append(("sweeps", len(buf)))
        self._n = len(buf)

    def last_sweeps(self):
        return np.ones(self._n, dtype=np.uint8), np.zeros((self._n, 3))

    def match_trails(self, buf, gsize, lengths=None, travel=None, params=None, rotations=False):
        self.calls.append(("trails", [int(g) for g in gsize]))
        self.trails.append((np.array(buf), list(gsize), np.array(lengths), travel, params))
        out = np.zeros(len(gsize), dtype=TR.TRAIL_DTYPE)
        ans = self.answers.pop(0) if self.answers else [{}] * len(gsize)
        end = np.cumsum(gsize)
        for g, a in enumerate(ans):
            last = buf[end[g] - 1]
            x, y = (float(v) for v in last[5:13].view("<f4"))
            out[g]["agent"], out[g]["anchor"], out[g]["records"] = last[4], gsize[g] - 1, gsize[g]
            out[g]["ax"], out[g]["ay"] = x + self.shift[0], y + self.shift[1]
            for k, v in a.items():
                out[g][k] = v
        return out


def _pair(fe, mapper, **kw):
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    bot = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    bot.bind(("127.0.0.1", 0))
    mc = fe.MissionControl(mapper, sock=srv, **kw)
    return mc, bot, ("127.0.0.1", srv.getsockname()[1])


def _send(P, bot, to, agent, x, y=0.0, yaw=0.0, lm=0):
    bot.sendto(P.pack_packet(agent, x, y, yaw, 1, 2, 0.5, 0.6, 0.7, 0.8, lm), to)


def _fields(buf):
    return np.ascontiguousarray(buf[:, 5:17]).view("<f4").reshape(-1, 3)


def test_without_match_packets_poll_does_what_it_did():
    fe, P = _mods()
    for sweeps in (False, True):
        m = StubMapper()
        mc, bot, to = _pair(fe, m, sweeps=sweeps)
        _send(P, bot, to, 1, 0.1)
        bot.sendto(b"junk", to)
        if sweeps:
            bot.sendto(P.pack_v0(1, 1.0, 0.0, 0.0, np.full(181, 0.6, dtype=np.float32)), to)
        _send(P, bot, to, 2, 0.2)
        time.sleep(0.05)
        assert mc.poll(now=10.0) == (4 if sweeps else 3)
        assert m.calls == ([("packets", 2), ("sweeps", 1), ("packets", 1)] if sweeps else [("packets", 3)])
        assert mc.trail_stats == dict(held=0, tried=0, accepted=0, moved=0, rewritten=0) and not mc.trail_matches
        assert mc.pkt_counts[1] >= 1 and mc.bot_addrs[2] is not None
        mc.close()
        bot.close()
        assert all(c[0] != "trails" for c in m.calls)


@pytest.mark.parametrize("sweeps", [False, True])
def test_packets_are_held_then_flushed_by_count_in_one_match_and_one_ingest(sweeps):
    fe, P = _mods()
    m = StubMapper()
    mc, bot, to = _pair(fe, m, sweeps=sweeps, match_packets=dict(trail=4, hold=5.0, travel=3.0, window=4))
    for k in range(3):
        _send(P, bot, to, 1, 0.1 * k)
    bot.sendto(b"junk", to)                                       # not a packet: to the ingest at once, as today
    _send(P, bot, to, 2, 5.0)
    time.sleep(0.05)
    assert mc.poll(now=10.0) == 5
    assert m.calls == [("packets", 1)] and int(m.ingested[0][1][0]) == 4
    assert mc.trail_stats["held"] == 4 and mc.online[1] and mc.online[2] and mc.last_packet_time[1] == 10.0
    assert mc.bot_addrs[1] == (bot.getsockname()[0], 8888) and mc.pkt_counts[1] == 0 and mc.bot_pose[1] is None
    # the heartbeat sees held packets: nothing is offline 4 s later, both are after 6 s of silence
    assert mc.heartbeat(now=14.0) == [] and mc.online[1]
    # the fourth packet of bot 1 fills its trail: bot 1 flushes alone, bot 2's packet stays
    _send(P, bot, to, 1, 0.3)
    time.sleep(0.05)
    assert mc.poll(now=11.0) == 1
    assert m.calls[1:] == [("trails", [4]), ("packets", 4)]
    buf, gsize, lens, travel, prm = m.trails[0]
    assert buf.shape == (4, 48) and lens.tolist() == [42] * 4 and travel == 3.0 and prm == dict(window=4)
    assert np.allclose(_fields(buf)[:, 0], [0.0, 0.1, 0.2, 0.3])
    assert np.allclose(_fields(m.ingested[1][0])[:, 0], [0.0, 0.1, 0.2, 0.3]) and m.ingested[1][2].tolist() == [10.0, 10.0, 10.0, 11.0]
    assert mc.trail_stats == dict(held=5, tried=1, accepted=0, moved=0, rewritten=0)
    assert mc.pkt_counts[1] == 4 and mc.pkt_counts[2] == 0 and int(mc.trail_matches[1]["records"]) == 4 and 2 not in mc.trail_matches
    assert mc.last_packet_time[1] == 11.0 and mc.last_packet_time[2] == 10.0        # arrival, not mapping, is what counts
    if not sweeps:
        assert mc.bot_pose[1] is None                              # (without frontier_targets no pose is kept, as today)
    mc.close()                                                     # close() flushes what is pending
    assert m.calls[3:] == [("trails", [1]), ("packets", 1)] and mc.pkt_counts[2] == 1
    bot.close()


def test_flush_by_age_and_flush_trails_and_arrival_order():
    fe, P = _mods()
    m = StubMapper()
    mc, bot, to = _pair(fe, m, match_packets=dict(trail=64, hold=2.0))
    for k, a in enumerate((1, 2, 1, 2, 2)):
        _send(P, bot, to, a, float(k))
    time.sleep(0.05)
    assert mc.poll(now=100.0) == 5 and m.calls == []
    assert mc.poll(now=101.9) == 0 and m.calls == []              # not yet 2 s old
    assert mc.poll(now=102.0) == 0                                 # both bots' oldest packets are: ONE match, ONE ingest
    assert m.calls == [("trails", [2, 3]), ("packets", 5)]
    assert _fields(m.trails[0][0])[:, 0].tolist() == [0.0, 2.0, 1.0, 3.0, 4.0]       # one group per bot, ascending id
    assert _fields(m.ingested[0][0])[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]     # mapped in arrival order
    assert m.ingested[0][0][:, 4].tolist() == [1, 2, 1, 2, 2]
    _send(P, bot, to, 1, 9.0)
    time.sleep(0.05)
    assert mc.poll(now=103.0) == 1 and len(m.calls) == 2
    mc.flush_trails(now=103.5)
    assert m.calls[2:] == [("trails", [1]), ("packets", 1)]
    mc.flush_trails()                                              # nothing pending: nothing called
    assert len(m.calls) == 4
    # more than `trail` packets of one bot in one poll flush in rounds of one trail each
    m2 = StubMapper()
    mc2, bot2, to2 = _pair(fe, m2, match_packets=dict(trail=2))
    for k in range(5):
        _send(P, bot2, to2, 1, float(k))
    time.sleep(0.05)
    assert mc2.poll(now=1.0) == 5
    assert m2.calls == [("trails", [2]), ("packets", 2), ("trails", [2]), ("packets", 2)]
    mc2.close()
    assert m2.calls[4:] == [("trails", [1]), ("packets", 1)]
    for s in (bot, bot2):
        s.close()
    mc.close()
    with pytest.raises(ValueError):
        fe.MissionControl(StubMapper(), sock=socket.socket(socket.AF_INET, socket.SOCK_DGRAM), match_packets=dict(trail=65))


def test_two_corrections_compose_and_rewrite_the_f32_fields():
    """Hand-computed.  The mapper adds (0.5, -0.25) to the fields (offset and drift).  Trail one, fields (1, 0) then (2, 0): its
    anchor stands at (2.5, -0.25); the match turns it a quarter turn and shifts it by (0.1, 0): in field coordinates
    p -> R90 (p - (2, 0)) + (2, 0) + (0.1, 0), so (1, 0) -> (2.1, -1), (2, 0) -> (2.1, 0), yaw + pi / 2.  Trail two, field (2, 1),
    is first moved by that: (2, 1) -> (1.1, 0), where the second match (no turn, shift (0, 0.2)) finds it; the composed transform
    maps (2, 1) -> (1.1, 0.2)."""
    fe, P = _mods()
    q = math.pi / 2
    m = StubMapper(answers=[[dict(ix=2, iy=0, it=90, accepted_match=1, dx=0.1, dy=0.0, dyaw=q)],
                            [dict(ix=0, iy=4, it=0, accepted_match=1, dx=0.0, dy=0.2, dyaw=0.0)],
                            [dict(ix=3, iy=3, it=3, accepted_match=0)],          # not accepted: changes nothing
                            [dict(ix=0, iy=0, it=0, accepted_match=1)]],         # accepted at zero: nothing to compose
                   shift=(0.5, -0.25))
    mc, bot, to = _pair(fe, m, match_packets=dict(trail=2), frontier_targets=True)
    f32 = np.float32
    _send(P, bot, to, 1, 1.0, 0.0, 0.25)
    _send(P, bot, to, 1, 2.0, 0.0, 0.25)
    time.sleep(0.05)
    mc.poll(now=1.0)
    assert _fields(m.trails[0][0]).tolist() == [[1.0, 0.0, 0.25], [2.0, 0.0, 0.25]]      # no transform yet
    got = _fields(m.ingested[0][0])
    c, s = math.cos(q), math.sin(q)
    t1 = (2.0 + 0.1 - (c * 2.0 - s * 0.0), 0.0 + 0.0 - (s * 2.0 + c * 0.0))
    want = [[f32(t1[0] + (c * 1.0 - s * 0.0)), f32(t1[1] + (s * 1.0 + c * 0.0)), f32(0.25 + q)],
            [f32(t1[0] + (c * 2.0 - s * 0.0)), f32(t1[1] + (s * 2.0 + c * 0.0)), f32(0.25 + q)]]
    assert got.tolist() == [[float(v) for v in r] for r in want]
    assert np.allclose(got, [[2.1, -1.0, 0.25 + q], [2.1, 0.0, 0.25 + q]], atol=1e-6)
    assert mc.trail_stats == dict(held=2, tried=1, accepted=1, moved=1, rewritten=2)
    assert np.allclose(mc.bot_pose[1], (2.1 + 0.5, 0.0 - 0.25), atol=1e-6)        # the pose the mapper reports for the last record
    _send(P, bot, to, 1, 2.0, 1.0, 0.0)
    _send(P, bot, to, 1, 2.0, 1.0, 0.0)
    time.sleep(0.05)
    mc.poll(now=2.0)
    assert np.allclose(_fields(m.trails[1][0]), [[1.1, 0.0, q]] * 2, atol=1e-6)           # matched as transform one maps it
    assert np.allclose(_fields(m.ingested[1][0]), [[1.1, 0.2, q]] * 2, atol=1e-6)         # mapped as the composed one does
    assert mc.trail_stats == dict(held=4, tried=2, accepted=2, moved=2, rewritten=4)
    T = mc._trail_T[1]
    for k in range(2):                                             # an unaccepted match and an accepted zero change nothing
        _send(P, bot, to, 1, 2.0, 1.0, 0.0)
        _send(P, bot, to, 1, 2.0, 1.0, 0.0)
        time.sleep(0.05)
        mc.poll(now=3.0 + k)
        assert mc._trail_T[1] == T and np.allclose(_fields(m.ingested[2 + k][0]), [[1.1, 0.2, q]] * 2, atol=1e-6)
    assert mc.trail_stats == dict(held=8, tried=4, accepted=3, moved=2, rewritten=8)
    assert int(mc.trail_matches[1]["accepted_match"]) == 1 and int(mc.trail_matches[1]["ix"]) == 0
    mc.close()
    bot.close()
