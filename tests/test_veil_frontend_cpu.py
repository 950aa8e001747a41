"""MissionControl(bot_veil=...) over the stub mapper and stub socket of the other front-end tests: the veil is turned on at the
start, a bot the heartbeat finds offline is forgotten, every sweep bot is placed after each sweep ingest -- in that order -- and
without the option no veil call is made at all."""
import numpy as np

from test_check_frontend_cpu import R181, StubMapper, _fe


def _sock():
    from test_reloc_rules_cpu import StubSock
    return StubSock()


class PacketStub(StubMapper):
    """StubMapper that also accepts 42-byte packets of bots 1 and 2 (pose = the packet's own); it has NO veil method."""

    def __init__(self):
        StubMapper.__init__(self, {})

    def ingest_array(self, buf, lens, times):
        self.calls.append(("packets", buf.copy(), None))
        ok = (np.asarray(lens) == 42) & (buf[:, 4] >= 1) & (buf[:, 4] <= 2)
        self._acc = ok.astype(np.uint8)
        self._pk_pose = np.ascontiguousarray(buf[:, 5:17]).view("<f4").reshape(-1, 3).astype(np.float64)

    def last_batch(self):
        return self._acc, self._pk_pose


class VeilStub(PacketStub):
    def set_bot_veil(self, radius=3):
        self.calls.append(("set_bot_veil", radius))

    def bot_veil_place(self, bot, x, y):
        self.calls.append(("place", bot, x, y))

    def bot_veil_forget(self, bot=None):
        self.calls.append(("forget", bot))


def _names(m):
    return [c[0] for c in m.calls]


def test_the_veil_is_turned_on_at_the_start():
    fe, P = _fe()
    assert P.BOT_VEIL_RADIUS == 3
    mc = fe.MissionControl(VeilStub(), sock=_sock(), bot_veil=True)
    assert mc.mapper.calls == [("set_bot_veil", P.BOT_VEIL_RADIUS)] and mc.bot_veil
    mc = fe.MissionControl(VeilStub(), sock=_sock(), bot_veil={"radius": 5})
    assert mc.mapper.calls == [("set_bot_veil", 5)]
    mc = fe.MissionControl(VeilStub(), sock=_sock(), bot_veil={})
    assert mc.mapper.calls == [("set_bot_veil", P.BOT_VEIL_RADIUS)]


def test_a_bot_found_offline_is_forgotten_once():
    fe, P = _fe()
    sock = _sock()
    mc = fe.MissionControl(VeilStub(), sock=sock, bot_veil=True)
    sock.put(P.pack_packet(1, 1.0, 2.0, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5), P.pack_packet(2, 3.0, 2.0, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5))
    assert mc.poll(now=1.0) == 2
    assert mc.heartbeat(now=2.0) == [] and _names(mc.mapper) == ["set_bot_veil", "packets"]      # packet ingests feed the table themselves
    sock.put(P.pack_packet(2, 3.0, 2.0, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5))
    mc.poll(now=5.0)
    assert mc.heartbeat(now=1.0 + P.HEARTBEAT_TIMEOUT + 0.5) == [1]
    assert mc.mapper.calls[-1] == ("forget", 1)
    n = len(mc.mapper.calls)
    assert mc.heartbeat(now=1.0 + P.HEARTBEAT_TIMEOUT + 1.0) == [] and len(mc.mapper.calls) == n   # (offline already: not again)
    assert mc.heartbeat(now=5.0 + P.HEARTBEAT_TIMEOUT + 0.5) == [2] and mc.mapper.calls[-1] == ("forget", 2)


def test_sweep_bots_are_placed_after_each_sweep_ingest():
    fe, P = _fe()
    sock = _sock()
    mc = fe.MissionControl(VeilStub(), sock=sock, sweeps=True, bot_veil=True)
    sock.put(P.pack_v0(1, 1.0, 0.5, 0.0, R181), P.pack_v0(2, 4.0, 0.25, 0.0, R181), P.pack_v0(1, 1.5, 0.75, 0.0, R181))
    assert mc.poll(now=1.0) == 3
    assert _names(mc.mapper) == ["set_bot_veil", "sweeps", "place", "place"]
    assert sorted(mc.mapper.calls[2:]) == [("place", 1, 1.5, 0.75), ("place", 2, 4.0, 0.25)]        # the latest accepted sweep of each
    # a packet run between two sweep runs: places follow each sweep ingest, none follows the packets
    sock.put(P.pack_v0(2, 2.0, 0.5, 0.0, R181), P.pack_packet(1, 1.0, 2.0, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5), P.pack_v0(1, 0.5, 0.5, 0.0, R181))
    k = len(mc.mapper.calls)
    assert mc.poll(now=2.0) == 3
    assert mc.mapper.calls[k + 1:k + 2] == [("place", 2, 2.0, 0.5)] and mc.mapper.calls[-1] == ("place", 1, 0.5, 0.5)
    assert [c[0] for c in mc.mapper.calls[k:]] == ["sweeps", "place", "packets", "sweeps", "place"]
    # a rejected sweep places nobody
    sock.put(P.pack_v0(7, 2.0, 0.5, 0.0, R181))
    k = len(mc.mapper.calls)
    mc.poll(now=3.0)
    assert [c[0] for c in mc.mapper.calls[k:]] == ["sweeps"]


def test_without_the_option_no_veil_call_is_made():
    """PacketStub has no veil method: any such call would raise."""
    fe, P = _fe()
    for kw in (dict(), dict(bot_veil=False), dict(bot_veil=None)):
        sock = _sock()
        mc = fe.MissionControl(PacketStub(), sock=sock, sweeps=True, **kw)
        sock.put(P.pack_v0(1, 1.0, 0.5, 0.0, R181), P.pack_packet(2, 1.0, 2.0, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5))
        assert mc.poll(now=1.0) == 2 and not mc.bot_veil
        assert mc.heartbeat(now=1.0 + P.HEARTBEAT_TIMEOUT + 1.0) == [1, 2]
        assert _names(mc.mapper) == ["sweeps", "packets"]
