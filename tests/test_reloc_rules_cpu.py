"""Relocalisation on the CPU: the restatement of include/quasar_slam.h's rules G1-G9 (tests/reloc_rules.py) checked against
itself (vectorised against word for word), against hand-built cases (tie order, the rival's circular rotation distance, the
statuses, every term of the gate) and as a localiser (it finds sensed sweeps in the three-room world); the ABI of the new
entry points; and MissionControl(relocalise=...) over a stub mapper."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import match_rules as MR
import reloc_rules as RR
import sense_rules as S
from conftest import ROOT, load_pkg

GEOM = (0.05, 0.0, 0.0)


def _protocol():
    return importlib.import_module(load_pkg().__name__ + ".protocol")


def _both(grid, ranges, p, smin=0.1, smax=0.6, geom=GEOM):
    """The vectorised and the word-for-word form, which must agree in every field."""
    a = RR.reloc_one(MR.field(grid, p["radius"]), grid == 0, geom, ranges, p, smin, smax)
    b = RR.reloc_one_brute(grid, geom, ranges, p, smin, smax)
    assert a == b, (a, b)
    return a


# ---- the two forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rot", [1, 8, 45])
@pytest.mark.parametrize("radius", [0, 2, 7])
def test_vectorised_form_equals_brute_force_on_random_grids(radius, n_rot):
    rng = np.random.default_rng(1000 + 10 * radius + n_rot)
    grid = rng.choice(np.array([-1, 0, 100], dtype=np.int8), (24, 24), p=[0.2, 0.7, 0.1])
    ranges = np.where(rng.random(181) < 0.2, rng.uniform(0.05, 0.6, 181), 0).astype(np.float32)
    boxes = (None, (3, -2, 19, 17)) if n_rot < 45 else ((15, 1, 30, 17),)          # boxes that cut the 16-cell tiles
    for box in boxes:
        p = RR.params(radius=radius, n_rot=n_rot, sep=3, sep_rot=min(2, n_rot - 1), min_hits=5, box=box)
        r = _both(grid, ranges, p, smax=0.5)
        assert r["status"] == RR.OK and r["hits"] == int(((ranges > 0.1) & (ranges <= 0.5)).sum()) > 10
        x0, y0, x1, y1 = RR.clip_box(box, 24)
        assert x0 <= r["gx"] < x1 and y0 <= r["gy"] < y1 and grid[r["gy"], r["gx"]] == 0


def _free_with(cells, size=24):
    g = np.zeros((size, size), dtype=np.int8)
    for gx, gy in cells:
        g[gy, gx] = 100
    return g


def _beams(**d):
    r = np.zeros(181, dtype=np.float32)
    for i, v in d.items():
        r[int(i[1:])] = v
    return r


def test_tie_order():
    """One beam of 5 cells along the heading, R 0, four rotations: j = 0 looks +x, 1 +y, 2 -x, 3 -y."""
    p = RR.params(radius=0, n_rot=4, sep=0, sep_rot=0, min_hits=1)
    beam = _beams(b90=0.25)
    # (10, 10) is hit from (5, 10) at j 0, (10, 5) at j 1, (15, 10) at j 2, (10, 15) at j 3: the smaller j wins, then the next
    r = _both(_free_with([(10, 10)]), beam, p)
    assert (r["score"], r["j"], r["gx"], r["gy"]) == (1, 0, 5, 10) and (r["score2"], r["j2"], r["gx2"], r["gy2"]) == (1, 1, 10, 5)
    # within j = 0: the smaller gy before the smaller gx
    r = _both(_free_with([(10, 10), (12, 8)]), beam, p)
    assert (r["j"], r["gx"], r["gy"]) == (0, 7, 8) and (r["j2"], r["gx2"], r["gy2"]) == (0, 5, 10)
    r = _both(_free_with([(10, 10), (14, 10)]), beam, p)
    assert (r["j"], r["gx"], r["gy"]) == (0, 5, 10) and (r["j2"], r["gx2"], r["gy2"]) == (0, 9, 10)
    # a higher score beats them all: two beams, both hit only from (10, 10) at j = 3 ((15, 5), where j = 1 would, is no candidate)
    two = _beams(b90=0.25, b180=0.25)
    r = _both(_free_with([(10, 5), (15, 10), (3, 3), (15, 5)]), two, p)
    assert (r["score"], r["j"], r["gx"], r["gy"]) == (2, 3, 10, 10)
    # the pose: the centre of the cell, th_3 = 3 pi / 2 reported as - pi / 2
    assert (r["x"], r["y"], r["yaw"]) == (0.0 + 10.5 * 0.05, 0.0 + 10.5 * 0.05, 3 * (2 * math.pi / 4) - 2 * math.pi)


def test_rival_uses_the_circular_rotation_distance():
    """One candidate cell; the beam ends on an OCCUPIED cell at j = 0 and at j = 7 of 8 (the twin across the wrap)."""
    g = _free_with([(20, 10), (17, 3)], size=32)                  # (10, 10) + (10, 0) and + (7, -7)
    beam = _beams(b90=0.5)
    prm = dict(radius=0, n_rot=8, sep=2, min_hits=1, box=(10, 10, 11, 11))
    a = _both(g, beam, RR.params(sep_rot=0, **prm))
    assert (a["j"], a["score"], a["j2"], a["score2"], a["accepted"]) == (0, 1, 7, 1, 0)
    b = _both(g, beam, RR.params(sep_rot=1, **prm))               # 7 is 1 step from 0, not 7
    assert (b["j"], b["score"], b["j2"], b["score2"], b["accepted"]) == (0, 1, 2, 0, 1)
    c = _both(g, beam, RR.params(sep_rot=7, **prm))
    assert (c["j2"], c["gx2"], c["gy2"], c["score2"], c["accepted"]) == (-1, -1, -1, 0, 1)


def test_statuses_and_the_empty_map():
    P = _protocol()
    r = np.full(181, 0.4, dtype=np.float32)
    g = _free_with([(10, 10)])
    buf = P.pack_sweeps([1, 3, 1, 1], [0.0] * 4, [0.0] * 4, [0.0] * 4, np.stack([r, r, np.zeros(181, np.float32), r]), odometry=False)
    lens = np.array([743, 743, 743, 742], dtype=np.uint16)
    out = RR.reloc(g, GEOM, buf, dict(n_rot=4, sep_rot=1), lens, 0.1, 0.6)
    assert out["status"].tolist() == [RR.OK, RR.NO_RECORD, RR.NO_CANDIDATE, RR.NO_RECORD]
    zero = np.zeros(1, dtype=RR.RELOC_DTYPE)
    zero["status"] = RR.NO_RECORD
    assert out[1].tobytes() == zero.tobytes() == out[3].tobytes()
    assert (out["accepted_record"][2], out["hits"][2], out["gx"][2], out["j2"][2], out["score"][2], out["accepted"][2]) == (1, 0, -1, -1, 0, 0)
    # no FREE cell in the box (OCCUPIED, UNKNOWN, an empty box): no candidate
    for box in ((10, 10, 11, 11), (5, 5, 5, 9), (30, 0, 40, 5)):
        assert RR.reloc(g, GEOM, buf[:1], dict(n_rot=4, sep_rot=1, box=box), None, 0.1, 0.6)["status"][0] == RR.NO_CANDIDATE
    unknown = np.full((24, 24), -1, dtype=np.int8)
    assert RR.reloc(unknown, GEOM, buf[:1], dict(n_rot=4, sep_rot=1), None, 0.1, 0.6)["status"][0] == RR.NO_CANDIDATE
    # a map with FREE cells and nothing OCCUPIED: every score is 0, the first candidate is the best, nothing is accepted
    e = _both(np.zeros((24, 24), dtype=np.int8), r, RR.params(n_rot=4, sep_rot=1, min_hits=1))
    assert (e["status"], e["score"], e["gx"], e["gy"], e["j"], e["accepted"]) == (RR.OK, 0, 0, 0, 0, 0)
    assert (e["score2"], e["gx2"], e["gy2"], e["j2"]) == (0, 5, 0, 0)          # the first cell more than sep = 4 away


def test_every_term_of_the_gate_at_its_threshold_and_past_it():
    """Candidate cell (10, 10) alone; beams 90 and 180 of 5 cells.  j = 0 hits (15, 10) and (10, 15): score 2; j = 1 hits
    (10, 15) only: the rival, score 1; H = 2, R = 0."""
    g = _free_with([(15, 10), (10, 15)])
    two = _beams(b90=0.25, b180=0.25)
    base = dict(radius=0, n_rot=4, sep=0, sep_rot=0, box=(10, 10, 11, 11), min_hits=2, min_percent=100, min_margin=50)
    r = _both(g, two, RR.params(**base))
    assert (r["score"], r["j"], r["score2"], r["j2"], r["hits"], r["accepted"]) == (2, 0, 1, 1, 2, 1)
    for term, past in (("min_hits", 3), ("min_margin", 51)):
        assert _both(g, two, RR.params(**dict(base, **{term: past})))["accepted"] == 0
    # the share: only (15, 10) OCCUPIED: score 1 of H 2, 50 %
    g1 = _free_with([(15, 10)])
    half = dict(base, min_margin=0)
    assert _both(g1, two, RR.params(**dict(half, min_percent=50)))["accepted"] == 1
    assert _both(g1, two, RR.params(**dict(half, min_percent=51)))["accepted"] == 0
    # the pose is reported either way
    r = _both(g1, two, RR.params(**dict(half, min_percent=51)))
    assert (r["gx"], r["gy"], r["x"], r["y"]) == (10, 10, 10.5 * 0.05, 10.5 * 0.05)


# ---- recovery: the rule is a localiser -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,noise,seed", [(24, 0.0, 1), (40, 0.02, 2)])
def test_sensed_sweeps_are_found_in_the_world(n, noise, seed):
    """Poses in the three-room world (a FREE cell at least 4 cells from every wall, anywhere inside it, any yaw), sweeps sensed
    at 3.0 m by sense_rules, the defaults (R 2, 180 rotations, sep 4 / 2, gate 40 / 70 / 5), sweep filter (0.1, 3.0).  A sweep is
    recovered when the found pose lies within one cell and one rotation step of the truth.  The bars: EVERY accepted sweep is
    recovered, and at least half of each set is accepted.
    Measured with this restatement: 24 noise-free poses, seed 1: 21 recovered, 15 accepted, none of them wrong; 40 poses at
    noise_amp 0.02, seed 2: 35 recovered, 27 accepted, none of them wrong."""
    size, res, ox, oy = RR.WORLD_GRID
    geom = (res, ox, oy)
    grid = RR.world()
    assert (grid == 100).sum() > 500 and (grid == 0).sum() > 10000
    poses, cells = RR.query_poses(grid, geom, n, seed)
    ranges, _ = S.sense_ranges(grid, res, ox, oy, poses, max_range=3.0, noise_amp=noise, seed=seed)
    p = RR.params()
    assert RR.limit_ok(p, RR.WORLD_SMAX, res)
    L, free, rot = MR.field(grid, p["radius"]), grid == 0, RR.rotations(p["n_rot"])
    found = accepted = 0
    for k in range(n):
        r = RR.reloc_one(L, free, geom, ranges[k], p, RR.WORLD_SMIN, RR.WORLD_SMAX, rot)
        ok = RR.recovered(r, cells[k], poses[k, 2], p["n_rot"])
        found += int(ok)
        accepted += int(r["accepted"])
        assert ok or not r["accepted"], f"sweep {k} was accepted at the wrong pose: {r}"
    print(f"recovered {found} of {n}, accepted {accepted} (noise_amp {noise}, seed {seed})")
    assert 2 * accepted >= n


def test_paint_rays_draw_the_worlds():
    """The rays the GPU tests paint their worlds with, drawn on the CPU: a free ray frees its cells up to its end cell."""
    for grid in (RR.world(), np.zeros((20, 20), dtype=np.int8), _free_with([(0, 0), (23, 5), (7, 23)])):
        size = len(grid)
        out = np.full(grid.shape, -1, dtype=np.int8)
        for x0, y0, x1, y1, valid in RR.paint_rays(grid).tolist():
            assert y0 == y1 and 0 <= min(x0, x1) and max(x0, x1) < size
            if valid:
                out[y0, x0] = 100
            else:
                out[y0, min(x0, x1 + 1):max(x0 + 1, x1)] = 0
        assert (out == grid).all()


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_structs_and_defaults():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    P = _protocol()
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("qs_relocalise_sweeps", "qs_relocalise_sweeps_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == 7
    assert re.search(r"typedef struct qs_reloc_params \{\s*int32_t radius, n_rot, sep, sep_rot, min_hits, min_percent, min_margin, use_box;"
                     r"\s*int32_t x0, y0, x1, y1;\s*\} qs_reloc_params;", code)
    assert re.search(r"typedef struct qs_sweep_reloc \{\s*int32_t gx, gy, j, score, hits;\s*int32_t gx2, gy2, j2, score2;\s*int32_t status;"
                     r"\s*uint8_t accepted_record, accepted, pad\[6\];\s*double x, y, yaw;\s*\} qs_sweep_reloc;", code)
    assert C.sizeof(L.QsRelocParams) == 12 * 4 == 48
    assert C.sizeof(L.QsSweepReloc) == 10 * 4 + 8 + 3 * 8 == 72 == P.RELOC_DTYPE.itemsize == RR.RELOC_DTYPE.itemsize
    assert P.RELOC_DTYPE == RR.RELOC_DTYPE
    for f in RR.FIELDS:
        assert getattr(L.QsSweepReloc, f).offset == P.RELOC_DTYPE.fields[f][1]
    assert L.QsSweepReloc.status.offset == 36 and L.QsSweepReloc.x.offset == 48
    prm = pkg.QuasarMapper.relocalise_params(True)
    got = (prm.radius, prm.n_rot, prm.sep, prm.sep_rot, prm.min_hits, prm.min_percent, prm.min_margin, prm.use_box)
    assert got == (2, 180, 4, 2, 40, 70, 5, 0) == tuple(RR.DEFAULTS[k] for k in list(RR.DEFAULTS)[:7]) + (0,)
    assert got[:7] == (P.RELOC_RADIUS, P.RELOC_N_ROT, P.RELOC_SEP, P.RELOC_SEP_ROT, P.RELOC_MIN_HITS, P.RELOC_MIN_PERCENT, P.RELOC_MIN_MARGIN)
    boxed = pkg.QuasarMapper.relocalise_params(dict(n_rot=8), box=(-3, 0, 17, 40))
    assert (boxed.n_rot, boxed.use_box, boxed.x0, boxed.y0, boxed.x1, boxed.y1) == (8, 1, -3, 0, 17, 40)
    for name, val in (("QS_RELOC_MAX_ROT", RR.MAX_ROT), ("QS_RELOC_MAX_SEP", RR.MAX_SEP), ("QS_RELOC_OK", RR.OK),
                      ("QS_RELOC_NO_RECORD", RR.NO_RECORD), ("QS_RELOC_NO_CANDIDATE", RR.NO_CANDIDATE)):
        assert re.search(r"#define " + name + r" " + str(val) + r"\b", code)
    assert (P.RELOC_OK, P.RELOC_NO_RECORD, P.RELOC_NO_CANDIDATE, P.RELOC_MAX_ROT, P.RELOC_MAX_SEP) == (0, 1, 2, 360, 16)


# ---- MissionControl(relocalise=...) over a stub mapper and a stub socket --------------------------------------------------------------
class StubSock:
    """The datagrams queued with put() arrive at the next poll, from one address."""

    def __init__(self):
        self.queue = []

    def put(self, *datagrams):
        self.queue.extend(datagrams)

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
    """Records every call with a copy of the records it was handed; relocalises bot 1 at (3, 2, pi / 2) and accepts it, finds
    nothing it would accept for any other bot."""

    def __init__(self, shift=None):
        self.calls = []
        if shift is not None:
            self.sweep_pose_shift = lambda bot: shift

    def ingest_array(self, buf, lens, times):
        self.calls.append(("packets", buf.copy(), None))
        self._acc = np.ones(len(buf), dtype=np.uint8)

    def last_batch(self):
        return self._acc, None

    def relocalise_sweeps(self, buf, lens=None, params=None):
        self.calls.append(("relocalise", buf.copy(), params))
        out = np.zeros(len(buf), dtype=RR.RELOC_DTYPE)
        out["accepted_record"] = 1
        out["x"], out["y"], out["yaw"] = 3.0, 2.0, math.pi / 2
        out["accepted"] = buf[:, 4] == 1
        return out

    def ingest_sweeps(self, buf, lens=None, seq0=None, match=None):
        self.calls.append(("sweeps", buf.copy(), match))
        self._pose = np.ascontiguousarray(buf[:, 5:17]).view("<f4").reshape(-1, 3).astype(np.float64)

    def last_sweeps(self):
        return np.ones(len(self._pose), dtype=np.uint8), self._pose


def _fields(rec):
    return np.ascontiguousarray(rec[5:17]).view("<f4").astype(np.float64).tolist()


def _mc(fe, **kw):
    sock = StubSock()
    return fe.MissionControl(StubMapper(kw.pop("shift", None)), sock=sock, sweeps=True, **kw), sock


def test_mission_control_relocalises_a_bot_that_comes_online():
    fe = importlib.import_module(load_pkg().__name__ + ".udp_frontend")
    P = _protocol()
    r = np.full(181, 0.6, dtype=np.float32)
    for kw in (dict(sweeps=False, relocalise=True), dict(sweeps=True, relocalise=True, sweep_graph=True),
               dict(sweeps=True, relocalise={}, sweep_graph={})):
        with pytest.raises(ValueError, match="relocalise"):
            fe.MissionControl(StubMapper(), sock=StubSock(), **kw)
    mc, sock = _mc(fe, relocalise=dict(n_rot=90))
    a1, a2, b1 = P.pack_v0(1, 1.0, 0.0, 0.0, r), P.pack_v0(1, 1.5, 0.0, 0.125, r), P.pack_v0(2, 7.0, 8.0, 0.5, r)
    sock.put(a1, b1, a2)
    assert mc.poll(now=10.0) == 3
    kinds = [c[0] for c in mc.mapper.calls]
    assert kinds == ["relocalise", "relocalise", "sweeps"]                   # bots 1 and 2, each on its first sweep, then ONE ingest
    assert mc.mapper.calls[0][1].tobytes() == a1 and mc.mapper.calls[1][1].tobytes() == b1 and mc.mapper.calls[0][2] == dict(n_rot=90)
    got = mc.mapper.calls[2][1]
    # bot 1: the triggering record lands on the found pose; the later one is carried by the same rigid transform
    assert _fields(got[0]) == [3.0, 2.0, float(np.float32(math.pi / 2))]
    x, y, yaw = _fields(got[2])
    assert abs(x - 3.0) < 1e-6 and abs(y - 2.5) < 1e-6 and yaw == float(np.float32(0.125 + (math.pi / 2 - 0.0)))
    # nothing else of bot 1's records changed, and bot 2 (not accepted) is byte for byte what arrived
    assert got[0, :5].tobytes() == a1[:5] and got[0, 17:].tobytes() == a1[17:] and got[2, 17:].tobytes() == a2[17:]
    assert got[1].tobytes() == b1
    assert set(mc.relocalised) == {1} and mc.relocalised[1]["x"] == 3.0 and mc.reloc_stats == {"tried": 2, "accepted": 1, "rewritten": 2}
    assert mc.bot_pose[1] == (x, y) and mc.bot_pose[2] == (7.0, 8.0) and mc.online[1] and mc.online[2]
    # online bots are not relocalised again; the transform stays in force
    sock.put(a2, b1)
    mc.poll(now=11.0)
    assert [c[0] for c in mc.mapper.calls[3:]] == ["sweeps"] and mc.mapper.calls[3][1][1].tobytes() == b1
    assert _fields(mc.mapper.calls[3][1][0]) == [x, y, yaw]
    # after the heartbeat takes bot 1 offline its next sweep is relocalised again, on the record as it arrived
    assert mc.heartbeat(now=11.0 + P.HEARTBEAT_TIMEOUT + 1) == [1, 2]
    sock.put(a2)
    mc.poll(now=20.0)
    assert [c[0] for c in mc.mapper.calls[4:]] == ["relocalise", "sweeps"] and mc.mapper.calls[4][1].tobytes() == a2
    assert _fields(mc.mapper.calls[5][1][0]) == [3.0, 2.0, float(np.float32(0.125 + (math.pi / 2 - 0.125)))]
    assert mc.reloc_stats == {"tried": 3, "accepted": 2, "rewritten": 4}
    mc.close()


def test_mission_control_transform_starts_from_the_pose_the_ingest_forms():
    """A mapper that adds (10, -1) to a sweep's x, y (a bot offset and drift): the rewritten fields are the found pose minus the
    shift, so that the ingest lands on the found pose."""
    fe = importlib.import_module(load_pkg().__name__ + ".udp_frontend")
    P = _protocol()
    r = np.full(181, 0.6, dtype=np.float32)
    mc, sock = _mc(fe, relocalise=True, shift=(10.0, -1.0))
    sock.put(P.pack_v0_odo(1, 1.0, 0.0, 0.0, 7, 9, r), P.pack_v0_odo(1, 1.0, 0.5, 0.0, 7, 9, r))
    mc.poll(now=1.0)
    assert mc.mapper.calls[0][2] is True
    got = mc.mapper.calls[1][1]
    assert _fields(got[0]) == [3.0 - 10.0, 2.0 + 1.0, float(np.float32(math.pi / 2))]
    x, y, _ = _fields(got[1])                       # 0.5 m to the left of the trigger, turned by 90 degrees: 0.5 m behind x
    assert abs(x + 10.0 - 2.5) < 1e-6 and abs(y - 1.0 - 2.0) < 1e-6
    mc.close()


def test_mission_control_without_the_option_is_what_it_was():
    fe = importlib.import_module(load_pkg().__name__ + ".udp_frontend")
    P = _protocol()
    r = np.full(181, 0.6, dtype=np.float32)
    sent = [P.pack_packet(1, 0.1, 0.2, 0.3, 1, 2, 0.5, 0.6, 0.7, 0.8, 5), P.pack_v0(1, 1.0, 0.0, 0.0, r), P.pack_v0(2, 2.0, 0.0, 0.0, r)]
    for kw in (dict(), dict(relocalise=False), dict(relocalise=None)):
        mc, sock = _mc(fe, **kw)
        sock.put(*sent)
        assert mc.poll(now=10.0) == 3
        calls = mc.mapper.calls
        assert [(c[0], c[2]) for c in calls] == [("packets", None), ("sweeps", None)]
        assert calls[0][1][0, :42].tobytes() == sent[0] and calls[1][1].tobytes() == sent[1] + sent[2]
        assert mc.relocalised == {} and mc.reloc_stats == {"tried": 0, "accepted": 0, "rewritten": 0}
        assert mc.bot_pose[1] == (1.0, 0.0) and mc.bot_pose[2] == (2.0, 0.0)
        mc.close()
