"""Relocalisation of a group on the CPU: the restatement of include/quasar_slam.h's rules J1-J8 (tests/reloc_group_rules.py)
checked against itself (vectorised against word for word), against the single-sweep restatement (the defining property),
against hand-built cases (statuses, J3's three reasons, J5's reach, the refusals) and as a localiser (groups of sensed sweeps
in the three-room world); protocol.reloc_rel on hand-worked poses; the ABI of the new entry points; and
MissionControl(relocalise={"group": K, ...}) over a stub mapper."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import match_rules as MR
import reloc_group_rules as GR
import reloc_rules as RR
import sense_rules as S
from conftest import ROOT, load_pkg

GEOM = (0.05, 0.0, 0.0)


def _protocol():
    return importlib.import_module(load_pkg().__name__ + ".protocol")


def _rel(*rows):
    return np.array([tuple(float(v) for v in r) for r in rows], dtype=GR.REL_DTYPE)


def _both(grid, ranges, rel, acc, travel, p, smin=0.1, smax=0.5, geom=GEOM):
    """The vectorised and the word-for-word form, which must agree in every field."""
    records, px, py = GR.points(ranges, rel, acc, travel, smin, smax)
    M = GR.reach_cells(smax, travel, geom[0])
    a = GR.group_one(MR.field(grid, p["radius"]), grid == 0, geom, records, px, py, p, M)
    b = GR.group_one_brute(grid, geom, ranges, rel, acc, travel, p, smin, smax)
    assert a == b, (a, b)
    return a


def _random_group(rng, k, travel):
    ranges = np.where(rng.random((k, 181)) < 0.12, rng.uniform(0.05, 0.6, (k, 181)), 0).astype(np.float32)
    th = rng.uniform(-math.pi, math.pi, k)
    r, a = rng.uniform(0, travel, k), rng.uniform(-math.pi, math.pi, k)
    rel = _rel(*[(r[i] * math.cos(a[i]), r[i] * math.sin(a[i]), math.sin(th[i]), math.cos(th[i])) for i in range(k)])
    rel[0] = (0.0, 0.0, 0.0, 1.0)
    return ranges, rel


# ---- the two forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rot", [1, 8, 45])
@pytest.mark.parametrize("radius", [0, 2, 7])
def test_vectorised_form_equals_brute_force_on_random_grids(radius, n_rot):
    rng = np.random.default_rng(2000 + 10 * radius + n_rot)
    grid = rng.choice(np.array([-1, 0, 100], dtype=np.int8), (24, 24), p=[0.2, 0.7, 0.1])
    for k in (1, 2, 3, 4):
        ranges, rel = _random_group(rng, k, 0.3)
        acc = np.ones(k, dtype=bool)
        if k >= 3:
            acc[1] = False                                        # a rejected record inside the group
        box = (None, (3, -2, 19, 17), (15, 1, 30, 17), None)[k - 1]
        p = RR.params(radius=radius, n_rot=n_rot, sep=3, sep_rot=min(2, n_rot - 1), min_hits=5, box=box)
        r = _both(grid, ranges, rel, acc, 0.3, p)
        hits = int(((ranges[acc] > 0.1) & (ranges[acc] <= 0.5)).sum())
        assert r["status"] == GR.OK and r["records"] == int(acc.sum()) and r["hits"] == hits > 5
        x0, y0, x1, y1 = RR.clip_box(box, 24)
        assert x0 <= r["gx"] < x1 and y0 <= r["gy"] < y1 and grid[r["gy"], r["gx"]] == 0


def test_a_group_of_one_with_the_identity_is_the_single_sweep():
    """The defining property, against reloc_rules.reloc_one: every field, `records` for `accepted_record`."""
    rng = np.random.default_rng(7)
    grid = rng.choice(np.array([-1, 0, 100], dtype=np.int8), (40, 40), p=[0.2, 0.7, 0.1])
    for radius, n_rot, box in ((0, 8, None), (2, 45, (3, 3, 30, 35)), (7, 180, (10, 10, 26, 26))):
        ranges = np.where(rng.random(181) < 0.4, rng.uniform(0.05, 0.6, 181), 0).astype(np.float32)
        p = RR.params(radius=radius, n_rot=n_rot, sep_rot=min(2, n_rot - 1), min_hits=5, box=box)
        one = RR.reloc_one(MR.field(grid, radius), grid == 0, GEOM, ranges, p, 0.1, 0.5)
        records, px, py = GR.points(ranges[None], GR.IDENTITY, [True], 0.0, 0.1, 0.5)
        grp = GR.group_one(MR.field(grid, radius), grid == 0, GEOM, records, px, py, p, GR.reach_cells(0.5, 0.0, 0.05))
        assert one["status"] == RR.OK and one.pop("accepted_record") == grp.pop("records") == 1
        assert one == grp
    assert GR.GROUP_DTYPE.itemsize == RR.RELOC_DTYPE.itemsize
    assert [GR.GROUP_DTYPE.fields[f][1] for f in GR.FIELDS] == [RR.RELOC_DTYPE.fields[f][1] for f in RR.FIELDS]


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


def test_two_records_score_jointly():
    """Candidate (10, 10) alone.  Record 0 in the frame, one beam of 5 cells ahead; record 1 stands 4 cells to the left and looks
    left, one beam of 3 cells ahead: at j = 0 the points fall on (15, 10) and (10, 17)."""
    g = _free_with([(15, 10), (10, 17)])
    ranges = np.stack([_beams(b90=0.25), _beams(b90=0.15)])
    rel = _rel((0.0, 0.0, 0.0, 1.0), (0.0, 0.2, 1.0, 0.0))
    p = RR.params(radius=0, n_rot=4, sep=0, sep_rot=0, min_hits=2, min_percent=100, min_margin=50, box=(10, 10, 11, 11))
    r = _both(g, ranges, rel, [True, True], 0.2, p)
    assert (r["status"], r["records"], r["hits"], r["score"], r["j"], r["gx"], r["gy"], r["accepted"]) == (GR.OK, 2, 2, 2, 0, 10, 10, 1)
    assert (r["x"], r["y"], r["yaw"]) == (10.5 * 0.05, 10.5 * 0.05, 0.0)          # the pose of the group's frame
    assert r["score2"] <= 1


def test_statuses_and_the_reasons_a_record_does_not_count():
    g = _free_with([(15, 10), (10, 17)])
    beam = _beams(b90=0.25)
    two = np.stack([beam, beam])
    p = RR.params(radius=0, n_rot=4, sep_rot=1, min_hits=1)
    ident = (0.0, 0.0, 0.0, 1.0)
    ok = _both(g, two, _rel(ident, ident), [True, True], 0.0, p)
    assert (ok["status"], ok["records"], ok["hits"]) == (GR.OK, 2, 2)
    # J3: not accepted by G3; a rel value that is not finite (each of the four); beyond travel (and exactly at it: counts)
    assert _both(g, two, _rel(ident, ident), [True, False], 0.0, p)["records"] == 1
    for bad in ((math.nan, 0, 0, 1), (0, math.inf, 0, 1), (0, 0, math.nan, 1), (0, 0, 0, -math.inf)):
        r = _both(g, two, _rel(ident, bad), [True, True], 0.5, p)
        assert (r["status"], r["records"], r["hits"]) == (GR.OK, 1, 1)
    assert _both(g, two, _rel(ident, (0.3, 0.4, 0, 1)), [True, True], 0.5, p)["records"] == 2      # 0.09 + 0.16 <= 0.25
    assert _both(g, two, _rel(ident, (0.3, 0.4000001, 0, 1)), [True, True], 0.5, p)["records"] == 1
    assert _both(g, two, _rel(ident, (0.0, 1e-9, 0, 1)), [True, True], 0.0, p)["records"] == 1
    # NO_RECORD: no record counts; every other field is zero
    none = _both(g, two, _rel(ident, ident), [False, False], 0.0, p)
    assert none == dict(dict.fromkeys(GR.FIELDS, 0), status=GR.NO_RECORD, x=0.0, y=0.0, yaw=0.0)
    # NO_CANDIDATE: H = 0 (records still counted); no FREE cell in the box
    dark = _both(g, np.zeros((2, 181), np.float32), _rel(ident, ident), [True, True], 0.0, p)
    assert (dark["status"], dark["records"], dark["hits"], dark["gx"], dark["j2"], dark["score"]) == (GR.NO_CANDIDATE, 2, 0, -1, -1, 0)
    for box in ((15, 10, 16, 11), (5, 5, 5, 9), (30, 0, 40, 5)):
        r = _both(g, two, _rel(ident, ident), [True, True], 0.0, dict(p, box=box))
        assert (r["status"], r["records"], r["hits"]) == (GR.NO_CANDIDATE, 2, 2)


def test_a_point_out_of_reach_scores_nothing():
    """smax 0.5, travel 0.2, res 0.05: M = 15.  Record 1 carries the dishonest (s, c) = (1, 1): its point lies sqrt(2) times as
    far as its beam is long, 0.2 + 0.5 * 1.41 = 0.91 m along the diagonal -- (13, 13) cells at j = 0, within reach on each axis,
    but (0, 18) after an eighth of a turn: out of reach, it scores 0 there whatever lies in that cell."""
    g = _free_with([(23, 23), (10, 28), (20, 10)], size=40)
    ranges = np.stack([_beams(b90=0.5), _beams(b90=0.5)])
    rel = _rel((0.0, 0.0, 0.0, 1.0), (0.1414, 0.1414, 1.0, 1.0))
    assert GR.reach_cells(0.5, 0.2, 0.05) == 15
    records, px, py = GR.points(ranges, rel, [True, True], 0.2, 0.1, 0.5)
    ax, ay, reach = GR.point_offsets(px, py, RR.rotations(8), 0.05, 15)
    assert (ax[0].tolist(), ay[0].tolist(), reach[0].tolist()) == ([10, 13], [0, 13], [True, True])
    assert reach[1].tolist() == [True, False] and reach[:, 0].all()
    p = RR.params(radius=0, n_rot=8, sep=0, sep_rot=0, min_hits=1, box=(10, 10, 11, 11))
    r = _both(g, ranges, rel, [True, True], 0.2, p, smax=0.5)
    assert (r["hits"], r["score"], r["j"]) == (2, 2, 0)            # j = 0: (20, 10) and (23, 23)
    only = _both(_free_with([(10, 28)], size=40), ranges, rel, [True, True], 0.2, p, smax=0.5)
    assert only["score"] == 0                                      # (10, 10) + (0, 18) is OCCUPIED, and out of reach
    # a point that is not a number scores nothing either
    huge = _both(g, ranges, _rel((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1e308, 1e308)), [True, True], 0.2, p, smax=0.5)
    assert (huge["hits"], huge["score"]) == (2, 1)


def test_every_refusal():
    p = RR.params()
    assert GR.limit_ok(p, 1.2, 2.0, 0.05) and GR.limit_ok(p, 1.2, 4.55, 0.05)          # 16 + 2 * (115 + 3) = 252
    assert not GR.limit_ok(p, 1.2, 4.7, 0.05)                                          # 16 + 2 * (118 + 3) = 258
    assert not GR.limit_ok(p, 1.2, -0.1, 0.05) and not GR.limit_ok(p, 1.2, math.nan, 0.05) and not GR.limit_ok(p, 1.2, math.inf, 0.05)
    for bad in (dict(radius=8), dict(n_rot=0), dict(n_rot=361), dict(sep=17), dict(n_rot=8, sep_rot=8)):
        assert not GR.limit_ok(RR.params(**bad), 1.2, 0.0, 0.05)
    assert GR.groups_ok(5, [1, 4]) and GR.groups_ok(16, [16]) and GR.groups_ok(0, [])
    assert not GR.groups_ok(5, [1, 3]) and not GR.groups_ok(5, [5, 0]) and not GR.groups_ok(17, [17]) and not GR.groups_ok(1, [])
    # the library's texts (the calls themselves need a GPU: tests/test_gpu_relocalise_groups.py)
    src = open(os.path.join(ROOT, load_pkg().__name__.split(".")[-1], "csrc", "reloc.hip")).read()
    for text in ("travel must be finite and not negative", "smax + travel is too large", "must lie in [1, QS_RELOC_MAX_GROUP]",
                 "the group sizes must sum to n"):
        assert text in src


def test_reloc_rel_on_hand_worked_poses():
    P = _protocol()
    # the anchor looks along +y from (1, 2); record 1 stands 2 m ahead of it looking along -x; record 2 stands 1 m to its right
    rel = P.reloc_rel([1.0, 1.0, 2.0], [2.0, 4.0, 2.0], [math.pi / 2, math.pi, 0.0])
    assert rel.dtype == P.RELOC_REL_DTYPE == GR.REL_DTYPE
    assert rel[0].tolist() == (0.0, 0.0, 0.0, 1.0)
    f = float(np.float32(math.pi / 2))
    c0, s0 = math.cos(f), math.sin(f)
    assert rel[1].tolist() == (c0 * 0.0 + s0 * 2.0, c0 * 2.0 - s0 * 0.0, math.sin(float(np.float32(math.pi)) - f), math.cos(float(np.float32(math.pi)) - f))
    assert abs(rel["tx"][1] - 2.0) < 1e-6 and abs(rel["ty"][1]) < 1e-6 and abs(rel["s"][1] - 1.0) < 1e-6 and abs(rel["c"][1]) < 1e-6
    assert abs(rel["tx"][2]) < 1e-6 and abs(rel["ty"][2] + 1.0) < 1e-6 and abs(rel["s"][2] + 1.0) < 1e-6
    # another anchor; the restatement's own form gives the same bits
    back = P.reloc_rel([1.0, 1.0, 2.0], [2.0, 4.0, 2.0], [math.pi / 2, math.pi, 0.0], anchor=2)
    assert back[2].tolist() == (0.0, 0.0, 0.0, 1.0) and back[0].tolist() == (-1.0, 0.0, math.sin(f), math.cos(f))
    rng = np.random.default_rng(3)
    x, y, yaw = rng.uniform(-5, 5, 6), rng.uniform(-5, 5, 6), rng.uniform(-3, 3, 6)
    assert P.reloc_rel(x, y, yaw, anchor=4).tobytes() == GR.rel_of(x, y, yaw, anchor=4).tobytes()
    assert len(P.reloc_rel([], [], [])) == 0


# ---- recovery: a group settles what a sweep leaves open ----------------------------------------------------------------------------
SETS = {"1.2m": (24, 0.0, 1, 1.2, 5, 0.8, 20), "3.0m": (24, 0.0, 1, 3.0, 3, 0.5, 40),
        "1.2m-noise": (40, 0.02, 2, 1.2, 5, 0.8, 20), "3.0m-noise": (40, 0.02, 2, 3.0, 3, 0.5, 40)}


@pytest.mark.parametrize("name", list(SETS))
def test_groups_of_sensed_sweeps_are_found_in_the_world(name):
    """The query poses of the single-sweep recovery test (24 noise-free with seed 1, 40 at noise_amp 0.02 with seed 2); from each
    the bot turns and drives on (reloc_group_rules.build_groups, the same seed): 5 sweeps 0.8 m apart under the 1.2 m filter with
    min_hits 20, 3 sweeps 0.5 m apart under the 3.0 m filter with min_hits 40; otherwise the defaults.  rel from the f32 poses,
    travel = (K - 1) * step.  The single sweep is the group's first, as a group of one.
    The bars: EVERY accepted group lies within one cell on each axis and two rotation steps of the truth (later sweeps sit on
    a lever arm, so the rotation grid is felt more); joint acceptance is at least single-sweep acceptance; at 1.2 m at least
    half of the set is accepted jointly.
    Measured with this restatement, recovered (one cell, ONE rotation step) / accepted:
        1.2 m, 24, noise-free:  single  2 /  1,  joint 22 / 18
        3.0 m, 24, noise-free:  single 21 / 15,  joint 23 / 20
        1.2 m, 40, +-0.02 m:    single  4 /  1,  joint 40 / 27
        3.0 m, 40, +-0.02 m:    single 34 / 27,  joint 40 / 38
    and no accepted group outside the bar."""
    n, noise, seed, smax, K, step, min_hits = SETS[name]
    size, res, ox, oy = RR.WORLD_GRID
    geom = (res, ox, oy)
    grid = RR.world()
    poses, cells = RR.query_poses(grid, geom, n, seed)
    G = GR.build_groups(grid, geom, poses, K, step, seed)
    assert (G[:, 0] == poses).all()
    travel = (K - 1) * step
    p = RR.params(min_hits=min_hits)
    assert GR.limit_ok(p, smax, travel, res)
    L, free, rot = MR.field(grid, p["radius"]), grid == 0, RR.rotations(p["n_rot"])
    ranges, _ = S.sense_ranges(grid, res, ox, oy, G.reshape(-1, 3), max_range=smax, noise_amp=noise, seed=seed)
    ranges = ranges.reshape(n, K, RR.BEAMS)
    turn = 2 * math.pi / p["n_rot"]
    single = [0, 0]
    joint = [0, 0]
    for k in range(n):
        records, px, py = GR.points(ranges[k, :1], GR.IDENTITY, [True], 0.0, RR.WORLD_SMIN, smax)
        one = GR.group_one(L, free, geom, records, px, py, p, GR.reach_cells(smax, 0.0, res), rot)
        single[0] += int(RR.recovered(one, cells[k], poses[k, 2], p["n_rot"]))
        single[1] += int(one["accepted"])
        rel = GR.rel_of(*G[k].T)
        assert (rel["tx"] ** 2 + rel["ty"] ** 2 <= travel * travel).all()
        records, px, py = GR.points(ranges[k], rel, [True] * K, travel, RR.WORLD_SMIN, smax)
        r = GR.group_one(L, free, geom, records, px, py, p, GR.reach_cells(smax, travel, res), rot)
        assert r["records"] == K
        joint[0] += int(RR.recovered(r, cells[k], poses[k, 2], p["n_rot"]))
        joint[1] += int(r["accepted"])
        dyaw = abs((float(r["yaw"]) - float(poses[k, 2]) + math.pi) % (2 * math.pi) - math.pi)
        near = abs(r["gx"] - cells[k][0]) <= 1 and abs(r["gy"] - cells[k][1]) <= 1 and dyaw <= 2 * turn
        assert near or not r["accepted"], f"group {k} was accepted at the wrong pose: {r}"
    print(f"{name}: single {single[0]} / {single[1]}, joint {joint[0]} / {joint[1]} (recovered / accepted of {n})")
    assert joint[1] >= single[1]
    if smax == 1.2:
        assert 2 * joint[1] >= n


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_structs_and_defaults():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    P = _protocol()
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("qs_relocalise_groups", "qs_relocalise_groups_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == 11 and L.SIGNATURES[name][1][9] is C.c_double
    assert re.search(r"typedef struct qs_reloc_rel \{\s*double tx, ty, s, c;\s*\} qs_reloc_rel;", code)
    assert re.search(r"typedef struct qs_group_reloc \{\s*int32_t gx, gy, j, score, hits;\s*int32_t gx2, gy2, j2, score2;\s*int32_t status;"
                     r"\s*uint8_t records, accepted, pad\[6\];\s*double x, y, yaw;\s*\} qs_group_reloc;", code)
    assert C.sizeof(L.QsRelocRel) == 32 == P.RELOC_REL_DTYPE.itemsize == GR.REL_DTYPE.itemsize
    assert C.sizeof(L.QsGroupReloc) == 72 == P.GROUP_RELOC_DTYPE.itemsize == GR.GROUP_DTYPE.itemsize
    assert P.GROUP_RELOC_DTYPE == GR.GROUP_DTYPE and P.RELOC_REL_DTYPE == GR.REL_DTYPE
    for f in GR.FIELDS:
        assert getattr(L.QsGroupReloc, f).offset == P.GROUP_RELOC_DTYPE.fields[f][1]
    assert L.QsGroupReloc.records.offset == 40 and L.QsGroupReloc.accepted.offset == 41 and L.QsGroupReloc.x.offset == 48
    assert re.search(r"#define QS_RELOC_MAX_GROUP 16\b", code) and P.RELOC_MAX_GROUP == GR.MAX_GROUP == 16
    assert 16 * 181 * (MR.MAX_RADIUS + 1) == 23168 < 1 << 16           # the kernel's 16-bit halves; the key's score field has 23 bits


# ---- MissionControl(relocalise={"group": K}) over a stub mapper and a stub socket ----------------------------------------------------
class StubSock:
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
    """Records every call with a copy of the records it was handed; a group of at least `need` records of bot 1 is found at
    (3, 2, pi / 2) and accepted, nothing else is."""

    def __init__(self, need=3):
        self.calls = []
        self.need = need

    def ingest_array(self, buf, lens, times):
        self.calls.append(("packets", buf.copy(), None))
        self._acc = np.ones(len(buf), dtype=np.uint8)

    def last_batch(self):
        return self._acc, None

    def relocalise_sweeps(self, buf, lens=None, params=None):
        raise AssertionError("group mode does not relocalise single sweeps")

    def relocalise_groups(self, buf, gsize, lengths=None, rel=None, travel=None, params=None):
        assert rel is None and list(gsize) == [len(buf)] and (np.asarray(lengths) == buf.shape[1]).all()
        self.calls.append(("groups", buf.copy(), (travel, params)))
        out = np.zeros(1, dtype=GR.GROUP_DTYPE)
        out["records"] = len(buf)
        out["x"], out["y"], out["yaw"] = 3.0, 2.0, math.pi / 2
        out["accepted"] = buf[0, 4] == 1 and len(buf) >= self.need
        return out

    def ingest_sweeps(self, buf, lens=None, seq0=None, match=None):
        self.calls.append(("sweeps", buf.copy(), match))
        self._pose = np.ascontiguousarray(buf[:, 5:17]).view("<f4").reshape(-1, 3).astype(np.float64)

    def last_sweeps(self):
        return np.ones(len(self._pose), dtype=np.uint8), self._pose


def _fields(rec):
    return np.ascontiguousarray(rec[5:17]).view("<f4").astype(np.float64).tolist()


def test_mission_control_locates_a_bot_at_its_third_sweep_and_gives_up_after_k():
    fe = importlib.import_module(load_pkg().__name__ + ".udp_frontend")
    P = _protocol()
    r = np.full(181, 0.6, dtype=np.float32)
    for bad in (dict(group=1), dict(group=17), dict(travel=1.0)):
        with pytest.raises(ValueError, match="relocalise"):
            fe.MissionControl(StubMapper(), sock=StubSock(), sweeps=True, relocalise=bad)
    sock = StubSock()
    mc = fe.MissionControl(StubMapper(), sock=sock, sweeps=True, relocalise=dict(group=4, travel=1.0, n_rot=90))
    assert mc.reloc_stats == {"tried": 0, "accepted": 0, "rewritten": 0, "group_tried": 0, "gave_up": 0}
    a = [P.pack_v0(1, 1.0, 0.0, 0.0, r), P.pack_v0(1, 1.5, 0.0, 0.125, r), P.pack_v0(1, 9.0, 0.0, 0.0, r), P.pack_v0(1, 1.0, 0.5, 0.25, r),
         P.pack_v0(1, 1.0, 1.0, 0.0, r)]
    b = [P.pack_v0(2, 7.0, 8.0, 0.5, r), P.pack_v0(2, 7.1, 8.0, 0.5, r), P.pack_v0(2, 7.2, 8.0, 0.5, r), P.pack_v0(2, 7.3, 8.0, 0.5, r),
         P.pack_v0(2, 7.4, 8.0, 0.5, r)]
    # poll 1: one sweep of each bot: two groups of one, neither accepted, the sweeps ingested as they arrived
    sock.put(a[0], b[0])
    mc.poll(now=1.0)
    assert [c[0] for c in mc.mapper.calls] == ["groups", "groups", "sweeps"]
    assert mc.mapper.calls[0][1].tobytes() == a[0] and mc.mapper.calls[0][2] == (1.0, dict(n_rot=90))
    assert mc.mapper.calls[2][1].tobytes() == a[0] + b[0]
    # poll 2: bot 1's second sweep, and one 8 m away, beyond travel: not kept; the run adds one record -> one call for bot 1
    sock.put(a[1], a[2], b[1])
    mc.poll(now=2.0)
    assert [c[0] for c in mc.mapper.calls[3:]] == ["groups", "groups", "sweeps"]
    assert mc.mapper.calls[3][1].tobytes() == a[0] + a[1] and mc.mapper.calls[4][1].tobytes() == b[0] + b[1]
    assert mc.mapper.calls[5][1].tobytes() == a[1] + a[2] + b[1] and mc.relocalised == {}
    # poll 3: bot 1's third kept sweep: accepted.  The transform runs from the FIRST kept record's pose (1, 0, 0) to (3, 2, pi / 2)
    sock.put(a[3], b[2])
    mc.poll(now=3.0)
    assert [c[0] for c in mc.mapper.calls[6:]] == ["groups", "groups", "sweeps"]
    assert mc.mapper.calls[6][1].tobytes() == a[0] + a[1] + a[3]
    got = mc.mapper.calls[8][1]
    x, y, yaw = _fields(got[0])                      # (1, 0.5, 0.25): 0.5 m to the left of the frame, which looks along +y: x - 0.5
    assert abs(x - 2.5) < 1e-6 and abs(y - 2.0) < 1e-6 and yaw == float(np.float32(0.25 + (math.pi / 2 - 0.0)))
    assert got[0, 17:].tobytes() == a[3][17:] and got[1].tobytes() == b[2]
    assert set(mc.relocalised) == {1} and mc.relocalised[1]["x"] == 3.0 and mc.relocalised[1]["records"] == 3
    assert mc.reloc_stats == {"tried": 0, "accepted": 1, "rewritten": 1, "group_tried": 6, "gave_up": 0}
    # poll 4: bot 1 is located: no more calls for it, its sweeps are rewritten; bot 2's fourth sweep is its K-th: given up
    sock.put(a[4], b[3])
    mc.poll(now=4.0)
    assert [c[0] for c in mc.mapper.calls[9:]] == ["groups", "sweeps"] and mc.mapper.calls[9][1].tobytes() == b"".join(b[:4])
    x, y, _ = _fields(mc.mapper.calls[10][1][0])
    assert abs(x - 2.0) < 1e-6 and abs(y - 2.0) < 1e-6
    assert mc.reloc_stats == {"tried": 0, "accepted": 1, "rewritten": 2, "group_tried": 7, "gave_up": 1}
    # poll 5: nothing is tried for a bot that was given up on
    sock.put(b[4])
    mc.poll(now=5.0)
    assert [c[0] for c in mc.mapper.calls[11:]] == ["sweeps"] and mc.mapper.calls[11][1].tobytes() == b[4]
    assert mc.reloc_stats["group_tried"] == 7 and mc.reloc_stats["gave_up"] == 1
    # ... until the heartbeat has taken it offline: it starts anew; bot 1 keeps its transform
    assert mc.heartbeat(now=5.0 + P.HEARTBEAT_TIMEOUT + 1) == [1, 2]
    sock.put(b[4], a[4])
    mc.poll(now=20.0)
    assert [c[0] for c in mc.mapper.calls[12:]] == ["groups", "sweeps"] and mc.mapper.calls[12][1].tobytes() == b[4]
    mc.close()


def test_mission_control_without_group_is_what_it_was():
    """relocalise=True and a dict without "group": single sweeps, the three statistics only, as before."""
    fe = importlib.import_module(load_pkg().__name__ + ".udp_frontend")
    P = _protocol()
    r = np.full(181, 0.6, dtype=np.float32)

    class Single(StubMapper):
        def relocalise_sweeps(self, buf, lens=None, params=None):
            self.calls.append(("relocalise", buf.copy(), params))
            return np.zeros(len(buf), dtype=RR.RELOC_DTYPE)

        def relocalise_groups(self, *a, **kw):
            raise AssertionError("not in group mode")

    for opt in (True, dict(n_rot=90)):
        sock = StubSock()
        mc = fe.MissionControl(Single(), sock=sock, sweeps=True, relocalise=opt)
        sock.put(P.pack_v0(1, 1.0, 0.0, 0.0, r), P.pack_v0(1, 1.1, 0.0, 0.0, r))
        mc.poll(now=1.0)
        assert [(c[0], c[2]) for c in mc.mapper.calls] == [("relocalise", opt), ("sweeps", None)]
        assert mc.reloc_stats == {"tried": 1, "accepted": 0, "rewritten": 0}
        mc.close()
