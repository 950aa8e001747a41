"""MissionControl(check_sweeps=...) over a stub mapper and a stub socket: the guarded ingest is what a sweep run goes through, the
run counter, the statistics, the hand-over of a lost bot to the relocaliser, and the options that exclude each other."""
import importlib
import math

import numpy as np
import pytest

import check_rules as CR
from conftest import load_pkg
from test_reloc_rules_cpu import StubSock

R181 = np.full(181, 0.6, dtype=np.float32)


class StubMapper:
    """The guarded ingest of a scripted world: a sweep's status is the next entry of `script[bot]` (OK once it runs out).  A
    withheld sweep is not accepted, as the library has it.  Relocalises any bot at (3, 2, pi / 2), accepting when `accept`."""

    def __init__(self, script, accept=True):
        self.script = {b: list(s) for b, s in script.items()}
        self.accept = accept
        self.calls = []

    def ingest_array(self, buf, lens, times):
        self.calls.append(("packets", buf.copy(), None))
        self._acc = np.zeros(len(buf), dtype=np.uint8)           # (the tests send no 42-byte packet that would be accepted)

    def last_batch(self):
        return self._acc, None

    def ingest_sweeps(self, buf, lens=None, seq0=None, match=None, check=None):
        self.calls.append(("sweeps", buf.copy(), check))
        ok = (np.asarray(lens) == buf.shape[1]) & (buf[:, 4] >= 1) & (buf[:, 4] <= 2)
        self._checks = np.zeros(len(buf), dtype=CR.CHECK_DTYPE)
        for j in range(len(buf)):
            s = self.script.get(int(buf[j, 4]), [])
            self._checks["status"][j] = (s.pop(0) if s else CR.OK) if ok[j] else CR.NO_RECORD
        self._checks["accepted_record"] = ok
        self._acc = (ok & (self._checks["status"] != CR.CONTRADICTS)).astype(np.uint8)
        self._pose = np.ascontiguousarray(buf[:, 5:17]).view("<f4").reshape(-1, 3).astype(np.float64)
        self._pose[self._acc == 0] = np.nan

    def last_sweeps(self):
        return self._acc, self._pose

    def last_sweep_checks(self):
        return self._checks

    def relocalise_sweeps(self, buf, lens=None, params=None):
        self.calls.append(("relocalise", buf.copy(), params))
        out = np.zeros(len(buf), dtype=importlib.import_module(load_pkg().__name__ + ".protocol").RELOC_DTYPE)
        out["accepted_record"] = 1
        out["x"], out["y"], out["yaw"] = 3.0, 2.0, math.pi / 2
        out["accepted"] = self.accept
        return out

    def relocalise_groups(self, recs, sizes, lens, travel=None, params=None):
        self.calls.append(("groups", recs.copy(), params))
        out = np.zeros(1, dtype=importlib.import_module(load_pkg().__name__ + ".protocol").GROUP_RELOC_DTYPE)
        out["x"], out["y"], out["yaw"] = 3.0, 2.0, math.pi / 2
        out["accepted"] = self.accept and len(recs) >= 2
        return out


def _fe():
    pkg = load_pkg()
    return importlib.import_module(pkg.__name__ + ".udp_frontend"), importlib.import_module(pkg.__name__ + ".protocol")


def _kinds(mc, since=0):
    return [c[0] for c in mc.mapper.calls[since:]]


C_, U_, O_ = CR.CONTRADICTS, CR.UNDECIDED, CR.OK


def test_options_that_exclude_each_other():
    fe, P = _fe()
    for kw in (dict(sweeps=False, check_sweeps=True), dict(sweeps=True, check_sweeps=True, sweep_graph=True),
               dict(sweeps=True, check_sweeps={}, sweep_graph={}), dict(sweeps=True, check_sweeps=True, match_sweeps=True),
               dict(sweeps=True, check_sweeps=dict(lost_after=0))):
        with pytest.raises(ValueError, match="check_sweeps"):
            fe.MissionControl(StubMapper({}), sock=StubSock(), **kw)
    mc = fe.MissionControl(StubMapper({}), sock=StubSock(), sweeps=True, check_sweeps=dict(tol=0.2, lost_after=3))
    assert mc.check_params == dict(tol=0.2) and mc.lost_after == 3
    mc = fe.MissionControl(StubMapper({}), sock=StubSock(), sweeps=True, check_sweeps=True)
    assert mc.check_params is True and mc.lost_after == P.CHECK_LOST_AFTER == 5


def test_without_the_option_nothing_changes():
    """Off (the default, False, None): the plain ingest is called without a `check` argument, nothing is counted."""
    fe, P = _fe()

    class Plain(StubMapper):
        def ingest_sweeps(self, buf, lens=None, seq0=None, match=None):      # (the signature before the option existed)
            StubMapper.ingest_sweeps(self, buf, lens, seq0, match)

    for kw in (dict(), dict(check_sweeps=False), dict(check_sweeps=None)):
        sock = StubSock()
        mc = fe.MissionControl(Plain({1: [C_] * 9}), sock=sock, sweeps=True, **kw)
        sock.put(P.pack_v0(1, 1.0, 0.0, 0.0, R181))
        assert mc.poll(now=1.0) == 1 and mc.mapper.calls[0][2] is None
        assert mc.check_stats == {"checked": 0, "withheld": 0, "undecided": 0} and mc.suspect == {1: 0, 2: 0} and mc.last_checks is None


def test_run_counter_and_statistics():
    fe, P = _fe()
    sock = StubSock()
    script = {1: [C_, C_, U_, C_, O_, C_], 2: [O_, U_]}
    mc = fe.MissionControl(StubMapper(script), sock=sock, sweeps=True, check_sweeps=dict(tol=0.15, lost_after=3))
    a, b = P.pack_v0(1, 1.0, 0.5, 0.0, R181), P.pack_v0(2, 7.0, 8.0, 0.5, R181)
    sock.put(a, b, a, b"junk")                       # bot 1: C C; bot 2: OK; one datagram that is no sweep (a run of its own)
    assert mc.poll(now=10.0) == 4
    assert mc.mapper.calls[0][2] == dict(tol=0.15)   # the run went through the guarded ingest with the option's parameters
    assert mc.suspect == {1: 2, 2: 0} and mc.check_stats == {"checked": 3, "withheld": 2, "undecided": 0}
    assert mc.last_checks["status"].tolist()[:3] == [C_, O_, C_]
    # a withheld sweep still shows the bot is there, but does not move it
    assert mc.online == {1: True, 2: True} and mc.bot_pose[1] is None and mc.bot_pose[2] == (7.0, 8.0)
    assert mc.last_packet_time[1] == 10.0 and mc.pkt_counts == {1: 2, 2: 1}
    sock.put(a, b)                                   # bot 1: UNDECIDED leaves the run alone; bot 2: UNDECIDED
    mc.poll(now=11.0)
    assert mc.suspect == {1: 2, 2: 0} and mc.check_stats == {"checked": 5, "withheld": 2, "undecided": 2}
    assert mc.bot_pose[1] == (1.0, 0.5)
    sock.put(a)                                      # C: the run reaches 3 = lost_after, but relocalise is off: nothing is handed over
    mc.poll(now=12.0)
    assert mc.suspect[1] == 3 and mc._lost == set() and "relocalise" not in _kinds(mc)
    sock.put(a, a)                                   # OK resets, C starts anew
    mc.poll(now=13.0)
    assert mc.suspect[1] == 1 and mc.check_stats == {"checked": 8, "withheld": 4, "undecided": 2}
    mc.close()


def test_a_lost_bot_is_handed_to_the_relocaliser():
    fe, P = _fe()
    sock = StubSock()
    mp = StubMapper({1: [O_, C_, C_, C_, C_]})
    mc = fe.MissionControl(mp, sock=sock, sweeps=True, relocalise=dict(n_rot=90), check_sweeps=dict(lost_after=3))
    a = P.pack_v0(1, 1.0, 0.0, 0.0, R181)
    sock.put(a)
    mc.poll(now=1.0)                                 # found offline: relocalised, transform in force
    assert _kinds(mc) == ["relocalise", "sweeps"] and 1 in mc._reloc_T and mc.reloc_stats["accepted"] == 1
    for t in (2.0, 3.0):
        sock.put(a)
        mc.poll(now=t)
    assert mc.suspect[1] == 2 and mc._lost == set() and 1 in mc._reloc_T and _kinds(mc, 2) == ["sweeps", "sweeps"]
    sock.put(a)
    mc.poll(now=4.0)                                 # the third contradiction in a row: lost, the transform is dropped
    assert mc.suspect[1] == 3 and mc._lost == {1} and 1 not in mc._reloc_T and mc.online[1]
    n = len(mp.calls)
    mp.accept = False
    sock.put(a)
    mc.poll(now=5.0)                                 # online, yet relocalised on the record as it arrived; not accepted: still lost
    assert _kinds(mc, n) == ["relocalise", "sweeps"] and mp.calls[n][1].tobytes() == a and mp.calls[n + 1][1].tobytes() == a
    assert mc._lost == {1} and mc.suspect[1] == 4 and 1 not in mc._reloc_T
    n = len(mp.calls)
    mp.accept = True
    sock.put(a)
    mc.poll(now=6.0)                                 # accepted: out of the lost set, the run starts anew, the record is rewritten
    assert _kinds(mc, n) == ["relocalise", "sweeps"] and mc._lost == set() and mc.suspect[1] == 0 and 1 in mc._reloc_T
    got = np.ascontiguousarray(mp.calls[n + 1][1][0, 5:17]).view("<f4").tolist()
    assert got == [3.0, 2.0, float(np.float32(math.pi / 2))]
    n = len(mp.calls)
    sock.put(a)
    mc.poll(now=7.0)                                 # and it is not relocalised again while it stays online and agrees
    assert _kinds(mc, n) == ["sweeps"] and mc.reloc_stats["accepted"] == 2
    mc.close()


def test_a_lost_bot_in_group_mode():
    fe, P = _fe()
    sock = StubSock()
    mp = StubMapper({1: [O_, O_, C_, C_]})
    mc = fe.MissionControl(mp, sock=sock, sweeps=True, relocalise=dict(group=3, travel=1.0), check_sweeps=dict(lost_after=2))
    a = P.pack_v0(1, 1.0, 0.0, 0.0, R181)
    for t in (1.0, 2.0):                             # located from its second sweep
        sock.put(a)
        mc.poll(now=t)
    assert _kinds(mc) == ["groups", "sweeps", "groups", "sweeps"] and 1 in mc._reloc_T and 1 not in mc._reloc_kept
    for t in (3.0, 4.0):
        sock.put(a)
        mc.poll(now=t)
    assert mc._lost == {1} and 1 not in mc._reloc_T
    n = len(mp.calls)
    for t in (5.0, 6.0):                             # kept and located as a group again
        sock.put(a)
        mc.poll(now=t)
    assert _kinds(mc, n) == ["groups", "sweeps", "groups", "sweeps"] and len(mp.calls[n + 2][1]) == 2
    assert mc._lost == set() and 1 in mc._reloc_T and mc.reloc_stats["group_tried"] == 4
    mc.close()
