"""Sweep matching on the CPU: the restatement of include/quasar_slam.h's rules (tests/match_rules.py) checked against
itself (the field three ways), against hand-built cases (the tie order, the gate) and as a matcher (it finds displaced
sweeps in a mapped room); and the ABI of the new entry points."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import match_rules as MR
from conftest import GOLDEN, ROOT, load_pkg
from oracle import oracle as orc


# ---- the field ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 2, 3, 7])
def test_field_forms_agree_on_random_small_grids(radius):
    rng = np.random.default_rng(100 + radius)
    for size, dens in ((1, 1.0), (5, 0.2), (17, 0.05), (24, 0.01), (24, 0.0)):
        g = rng.choice(np.array([-1, 0, 100], dtype=np.int8), (size, size), p=[(1 - dens) / 2, (1 - dens) / 2, dens])
        a, b, c = MR.field(g, radius), MR.field_filter(g, radius), MR.field_brute(g, radius)
        assert (a == c).all() and (b == c).all()
        assert a.max() <= radius + 1 and ((a == radius + 1) == (g == 100)).all()


def test_field_on_the_golden_map_edges_and_corners():
    g = np.load(os.path.join(GOLDEN, "sweeps_512.npz"), allow_pickle=False)["grid"]
    for radius in (0, 2, 7):
        assert (MR.field(g, radius) == MR.field_filter(g, radius)).all()
    assert (MR.field(g, 0) == np.where(g == 100, 1, 0)).all()
    # occupied cells in a corner and on an edge: the field is cut at the grid, not wrapped
    e = np.full((12, 12), -1, dtype=np.int8)
    e[0, 0] = 100
    e[11, 5] = 100
    f = MR.field(e, 2)
    assert (f == MR.field_brute(e, 2)).all()
    assert f[0, 0] == 3 and f[1, 1] == 2 and f[2, 2] == 1 and f[3, 3] == 0 and f[0, 11] == 0 and f[11, 0] == 0
    assert f[11, 5] == 3 and f[9, 7] == 1 and f[8, 5] == 0
    # FREE and UNKNOWN are not told apart
    e2 = np.where(e == -1, 0, e).astype(np.int8)
    assert (MR.field(e2, 2) == f).all()


# ---- hand-built sweeps: tie order and gate --------------------------------------------------------------------------------------
GEOM = (0.05, -5.0, -5.0)


def _one_beam_sweep(d=0.5):
    r = np.zeros(181, dtype=np.float32)
    r[90] = d                                # the beam along the heading
    return r


def _grid_with(cells, size=200):
    g = np.full((size, size), -1, dtype=np.int8)
    for gx, gy in cells:
        g[gy, gx] = 100
    return g


def test_tie_order():
    p = MR.params(radius=0, window=3, angle_steps=0, min_hits=1, min_percent=100)
    pose = (0.025, 0.025, 0.0)               # cell (100, 100); the beam ends in cell (110, 100)
    # two candidates tie on score 1: ix = +2 (r2 4) and iy = -1 (r2 1): the smaller ix^2 + iy^2 wins
    m = MR.match_one(MR.field(_grid_with([(112, 100), (110, 99)]), 0), GEOM, pose, _one_beam_sweep(), p, 0.1, 1.2)
    assert (m["ix"], m["iy"], m["it"], m["score"], m["score0"], m["accepted_match"]) == (0, -1, 0, 1, 0, 1)
    assert (m["dx"], m["dy"], m["dyaw"]) == (0.0, -1 * 0.05, 0.0)
    # three tie on r2 = 1 as well: (0, -1), (0, +1), (-1, 0): the smaller iy wins, before the smaller ix
    m = MR.match_one(MR.field(_grid_with([(110, 99), (110, 101), (109, 100)]), 0), GEOM, pose, _one_beam_sweep(), p, 0.1, 1.2)
    assert (m["ix"], m["iy"], m["it"]) == (0, -1, 0)
    m = MR.match_one(MR.field(_grid_with([(110, 101), (109, 100), (111, 100)]), 0), GEOM, pose, _one_beam_sweep(), p, 0.1, 1.2)
    assert (m["ix"], m["iy"], m["it"]) == (-1, 0, 0)
    # rotations: a wall across the beam scores the same for it = -1, 0, +1: |it| = 0 wins; without 0, the smaller it
    wall = _grid_with([(110, y) for y in range(95, 106)])
    pr = MR.params(radius=0, window=0, angle_steps=1, min_hits=1, min_percent=100)
    m = MR.match_one(MR.field(wall, 0), GEOM, pose, _one_beam_sweep(), pr, 0.1, 1.2)
    assert (m["it"], m["score"], m["score0"]) == (0, 1, 1)
    rot = MR.rotations_libm(0.0, 1, math.pi / 180)
    rot[1] = (1.0, 0.0)                      # make "it = 0" point along +y, where nothing is: -1 and +1 tie
    m = MR.match_one(MR.field(wall, 0), GEOM, pose, _one_beam_sweep(), pr, 0.1, 1.2, rot=rot)
    assert (m["it"], m["score"], m["score0"], m["dyaw"]) == (-1, 1, 0, -1 * (math.pi / 180))


def test_empty_map_and_gate():
    r = np.full(181, 0.8, dtype=np.float32)
    empty = np.full((200, 200), -1, dtype=np.int8)
    m = MR.match_one(MR.field(empty, 2), GEOM, (0.3, 0.4, 1.0), r, MR.params(), 0.1, 1.2)
    assert (m["ix"], m["iy"], m["it"], m["score"], m["hits"], m["accepted_match"]) == (0, 0, 0, 0, 181, 0)
    assert (m["dx"], m["dy"], m["dyaw"]) == (0.0, 0.0, 0.0)
    # too few hit beams: the best candidate is reported, the correction is zero
    g = _grid_with([(112, 100)])
    p = MR.params(radius=0, window=3, angle_steps=0, min_hits=2, min_percent=100)
    m = MR.match_one(MR.field(g, 0), GEOM, (0.025, 0.025, 0.0), _one_beam_sweep(), p, 0.1, 1.2)
    assert (m["ix"], m["score"], m["hits"], m["accepted_match"], m["dx"]) == (2, 1, 1, 0, 0.0)
    # the share: 1 of 2 hit beams scores, 50 % passes "50" and fails "51"
    r2 = _one_beam_sweep()
    r2[0] = 0.5
    for pct, want in ((50, 1), (51, 0)):
        p = MR.params(radius=0, window=3, angle_steps=0, min_hits=1, min_percent=pct)
        assert MR.match_one(MR.field(g, 0), GEOM, (0.025, 0.025, 0.0), r2, p, 0.1, 1.2)["accepted_match"] == want
    # a pose that has no cell scores nothing and raises nothing
    m = MR.match_one(MR.field(g, 0), GEOM, (float("nan"), 0.0, 0.0), _one_beam_sweep(), p, 0.1, 1.2)
    assert (m["ix"], m["iy"], m["it"], m["score"]) == (0, 0, 0, 0)
    # rejected records are all zeros
    P = importlib.import_module(load_pkg().__name__ + ".protocol")
    buf = P.pack_sweeps([1, 3], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], np.stack([r, r]), odometry=False)
    out = MR.match(g, GEOM, buf)
    assert out["accepted_record"].tolist() == [1, 0] and out[1].tobytes() == bytes(MR.MATCH_DTYPE.itemsize)


# ---- recovery: the rule is a matcher ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,window,steps", [(2, 4, 5), (3, 4, 5), (2, 6, 10), (3, 6, 10)])
def test_displaced_sweeps_are_recovered_in_the_room(radius, window, steps):
    """30 mapping sweeps (one in each cell of a lattice over the room) drawn through the reference's update_ray at their
    true poses, 30 queries anywhere in the room displaced by whole cells and angle steps inside the window, range noise sigma
    0.01 m, sweep filter (0.1, 3.0).  A query is recovered when the returned candidate cancels its displacement to within
    one cell on each axis and one angle step.  Bar: at least 90 % (27 of 30).
    Measured with this restatement on the update_ray-drawn map, seed 11: 29 of 30 for each of R2 W4 T5, R3 W4 T5,
    R2 W6 T10 and R3 W6 T10 (27 of them with zero residual); seeds 1..12 at R2 W4 T5 give 28 to 30.  The walls run through
    the middle of cells: with walls ON cell boundaries the 0.01 m noise splits every wall over two rows of cells, later free
    rays erase half of them (update_ray's last writer wins), and the same rule recovers 21 to 26 of 30."""
    size, res, ox, oy = MR.ROOM_GRID
    s = MR.room_session(seed=11, n_map=30, n_query=30, window=window, angle_steps=steps)
    o = orc.OracleMapper(size, res, ox, oy, 0.0)
    o.update_rays(*MR.beams_of_all(s["map_pose"], s["map_ranges"], MR.ROOM_SMIN, MR.ROOM_SMAX))
    grid = o.grid.copy()
    assert (grid == 100).sum() > 300
    p = MR.params(radius=radius, window=window, angle_steps=steps)
    assert MR.limit_ok(p, MR.ROOM_SMAX, res)
    L = MR.field(grid, radius)
    got = gated = 0
    for k in range(30):
        m = MR.match_one(L, (res, ox, oy), s["q_pose"][k], s["q_ranges"][k], p, MR.ROOM_SMIN, MR.ROOM_SMAX)
        got += int(MR.recovered(m, s["q_disp"][k]))
        gated += int(m["accepted_match"])
    print(f"recovered {got} of 30, {gated} matches accepted (R {radius}, W {window}, T {steps})")
    assert got >= 27


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("qs_match_field", "qs_match_sweeps", "qs_match_sweeps_device", "qs_ingest_sweeps_matched",
               "qs_ingest_sweeps_matched_device", "qs_last_sweep_matches")


def test_abi_symbols_structs_and_defaults():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    P = importlib.import_module(pkg.__name__ + ".protocol")
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    # the header's layouts: six int32 and a double; six int32, two uint8 (padded to 8) and three doubles
    assert re.search(r"typedef struct qs_match_params \{ int32_t radius, window, angle_steps, min_hits, min_percent, reserved; "
                     r"double angle_step; \} qs_match_params;", code)
    assert C.sizeof(L.QsMatchParams) == 6 * 4 + 8 == 32
    assert C.sizeof(L.QsSweepMatch) == 6 * 4 + 8 + 3 * 8 == 56 == P.MATCH_DTYPE.itemsize == MR.MATCH_DTYPE.itemsize
    assert P.MATCH_DTYPE == MR.MATCH_DTYPE
    for f in ("dx", "dy", "dyaw", "accepted_record", "accepted_match", "hits"):
        assert getattr(L.QsSweepMatch, f).offset == P.MATCH_DTYPE.fields[f][1]
    assert L.QsSweepMatch.dx.offset == 32
    prm = pkg.QuasarMapper.match_params(True)
    want = (P.MATCH_RADIUS, P.MATCH_WINDOW, P.MATCH_ANGLE_STEPS, P.MATCH_MIN_HITS, P.MATCH_MIN_PERCENT, P.MATCH_ANGLE_STEP)
    assert (prm.radius, prm.window, prm.angle_steps, prm.min_hits, prm.min_percent, prm.angle_step) == want
    assert want == tuple(MR.DEFAULTS[k] for k in ("radius", "window", "angle_steps", "min_hits", "min_percent", "angle_step"))
    assert want == (2, 6, 10, 20, 50, math.pi / 180)
    for name, val in (("QS_MATCH_MAX_RADIUS", MR.MAX_RADIUS), ("QS_MATCH_MAX_ANGLE_STEPS", MR.MAX_ANGLE_STEPS),
                      ("QS_MATCH_MAX_REACH", MR.MAX_REACH)):
        assert re.search(r"#define " + name + r" " + str(val) + r"\b", code)
    assert pkg.QuasarMapper.match_params(dict(window=4), angle_steps=5).window == 4


# ---- MissionControl(match_sweeps=True) over a loopback socket, a stub in place of the mapper -----------------------------------------
class StubMapper:
    def __init__(self):
        self.calls = []

    def ingest_array(self, buf, lens, times):
        self.calls.append(("packets", len(buf), None))
        self._acc = np.ones(len(buf), dtype=np.uint8)

    def last_batch(self):
        return self._acc, None

    def ingest_sweeps(self, buf, lens=None, seq0=None, match=None):
        self.calls.append(("sweeps", len(buf), match))
        self._n = len(buf)
        self._matched = match is not None
        self._x = np.ascontiguousarray(buf[:, 5:9]).view("<f4").reshape(-1).astype(np.float64)

    def last_sweeps(self):
        # a matched ingest reports the corrected pose: the stub's correction is +0.25 m in x
        pose = np.stack([self._x + (0.25 if self._matched else 0.0), np.zeros(self._n), np.zeros(self._n)], axis=1)
        return np.ones(self._n, dtype=np.uint8), pose

    def last_sweep_matches(self):
        assert self._matched
        out = np.zeros(self._n, dtype=MR.MATCH_DTYPE)
        out["dx"] = 0.25
        return out


def test_mission_control_matches_sweeps_when_asked():
    import socket
    import time
    fe = importlib.import_module(load_pkg().__name__ + ".udp_frontend")
    P = importlib.import_module(load_pkg().__name__ + ".protocol")
    with pytest.raises(ValueError):
        fe.MissionControl(StubMapper(), sock=None, sweeps=False, match_sweeps=True)
    r = np.full(181, 0.6, dtype=np.float32)
    for matched, prm in ((False, None), (True, None), (True, dict(window=4, angle_steps=5))):
        srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        srv.bind(("127.0.0.1", 0))
        port = srv.getsockname()[1]
        mc = fe.MissionControl(StubMapper(), sock=srv, sweeps=True, match_sweeps=matched, match_params=prm)
        bot = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        bot.bind(("127.0.0.1", 0))
        bot.sendto(P.pack_packet(1, 0.1, 0.2, 0.3, 1, 2, 0.5, 0.6, 0.7, 0.8, 5), ("127.0.0.1", port))
        bot.sendto(P.pack_v0(1, 1.0, 0.0, 0.0, r), ("127.0.0.1", port))
        bot.sendto(P.pack_v0(2, 2.0, 0.0, 0.0, r), ("127.0.0.1", port))
        time.sleep(0.05)
        assert mc.poll(now=10.0) == 3
        want = (True if prm is None else prm) if matched else None
        assert mc.mapper.calls == [("packets", 1, None), ("sweeps", 2, want)]
        shift = 0.25 if matched else 0.0
        assert mc.bot_pose[1] == (1.0 + shift, 0.0) and mc.bot_pose[2] == (2.0 + shift, 0.0)
        assert (mc.last_matches is not None and len(mc.last_matches) == 2) if matched else mc.last_matches is None
        bot.close()
        mc.close()
