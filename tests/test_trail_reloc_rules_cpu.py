"""Trail relocalisation, the rule alone (tests/trail_reloc_rules.py, K1-K8 of include/quasar_slam.h): the vectorised restatement
against the word-for-word one, the record-level cases, and what the rule recovers of trails driven through the world of
tests/reloc_rules.py and reported in frames of their own."""
import importlib
import math

import numpy as np
import pytest

import match_rules as MR
import reloc_rules as RR
import trail_reloc_rules as KR
import trail_rules as TR
from conftest import load_pkg

SMALL_GEOM = (0.05, -1.7, -1.7)
WORLD_GEOM = RR.WORLD_GRID[1:]


def _both(grid, geom, buf, p, travel, max_dist=TR.MAX_DIST, lengths=None):
    """reloc_one and reloc_one_brute of one trail, equal in every field; returns the result."""
    p = RR.params(**p)
    L, free = MR.field(grid, p["radius"]), grid == 0
    vec, _ = KR.reloc_one(L, free, geom, buf, p, travel, lengths, max_dist=max_dist)
    brute = KR.reloc_one_brute(grid, geom, buf, p, travel, lengths, max_dist=max_dist)
    for f in KR.FIELDS:
        a, b = vec[f], brute[f]
        assert (np.float64(a).tobytes() == np.float64(b).tobytes()) if isinstance(b, float) else a == b, (f, a, b)
    return vec


@pytest.fixture(scope="module")
def small():
    grid = RR.small_world()
    return grid, KR.world_trails(grid, SMALL_GEOM, seed=3, n=4, K=12, far=3.0)


@pytest.mark.parametrize("n_rot", [8, 12])
def test_vectorised_equals_word_for_word(small, n_rot):
    grid, T = small
    for i in range(4):
        r = _both(grid, SMALL_GEOM, T["pkts"][12 * i:12 * i + 12], dict(n_rot=n_rot, sep_rot=1, min_hits=4), 0.8, max_dist=3.0)
        assert r["status"] == KR.OK and r["records"] == 12 and r["anchor"] == 11 and r["hits"] >= 1


def _hand_grid():
    g = np.zeros((16, 16), dtype=np.int8)
    g[4, 10] = 100
    return g, (0.5, 0.0, 0.0)


def test_a_trail_worked_by_hand():
    """One packet at fields (100, 200), yaw 0, front sonar 1.0 m; cells of 0.5 m, one OCCUPIED cell (10, 4), R = 0, four
    rotations.  q = (1, 0).  j = 0 puts it 2 cells east: the anchor in (8, 4) scores 1; j = 1: (10, 2); j = 2: (12, 4), cut off
    by the box; j = 3: (10, 6).  The best is the smallest j.  With sep 4 and sep_rot 1 the others lie inside the exclusion, so
    the rival is the first cell of score 0 outside the square: (0, 0) at j = 0.  (100 - 0) * 100 >= 5 * 1: accepted."""
    grid, geom = _hand_grid()
    buf = TR.pack([1], [100.0], [200.0], [0.0], [[1.0, 0.0, 0.0, 0.0]])
    r = _both(grid, geom, buf, dict(radius=0, n_rot=4, sep=4, sep_rot=1, min_hits=1, box=(0, 0, 12, 16)), 0.0)
    exp = dict(gx=8, gy=4, j=0, score=1, hits=1, gx2=0, gy2=0, j2=0, score2=0, status=KR.OK, records=1, accepted=1, agent=1,
               anchor=0, x=4.25, y=2.25, yaw=0.0, ax=100.0, ay=200.0)
    assert r == exp
    assert KR.move(r, 100.0, 200.0, 0.0) == (4.25, 2.25, 0.0)
    assert KR.move(r, 101.0, 200.0, 0.5) == (5.25, 2.25, 0.5)
    # without the box j = 2's (12, 4) is a rival of equal score: the margin fails
    r2 = _both(grid, geom, buf, dict(radius=0, n_rot=4, sep=4, sep_rot=1, min_hits=1), 0.0)
    assert (r2["gx2"], r2["gy2"], r2["j2"], r2["score2"], r2["accepted"]) == (12, 4, 2, 1, 0)


def test_a_rejected_anchor_and_mixed_agents(small):
    grid, T = small
    buf = T["pkts"][:12].copy()
    buf[11, 0] = ord("X")                                          # the last record is broken: the anchor is record 10
    buf[3, 4] = 2                                                  # another bot's
    buf[5, 4] = 9                                                  # beyond max_agent
    r = _both(grid, SMALL_GEOM, buf, dict(n_rot=8, min_hits=4), 0.8, max_dist=3.0)
    assert (r["anchor"], r["records"], r["agent"]) == (10, 9, 1)
    x10 = float(np.frombuffer(bytes(buf[10, 5:9]), "<f4")[0])
    assert r["ax"] == x10
    buf[10, 4] = 2                                                 # the anchor is bot 2's: only its own record and record 3 count
    r = _both(grid, SMALL_GEOM, buf, dict(n_rot=8, min_hits=4), 0.8, max_dist=3.0)
    assert (r["anchor"], r["records"], r["agent"]) == (10, 2, 2)


def test_travel_at_equality_and_one_ulp_under():
    grid, geom = _hand_grid()
    buf = TR.pack([1, 1], [3.0, 0.0], [4.0, 0.0], [0.0, 0.0], [[1.0, 0, 0, 0], [1.0, 0, 0, 0]])
    p = dict(radius=0, n_rot=4, sep_rot=1, min_hits=1)
    at = _both(grid, geom, buf, p, 5.0)
    under = _both(grid, geom, buf, p, math.nextafter(5.0, 0.0))
    assert (at["records"], at["hits"]) == (2, 2) and (under["records"], under["hits"]) == (1, 1)
    zero = _both(grid, geom, buf, p, 0.0)
    assert (zero["records"], zero["anchor"]) == (1, 1)
    buf[0, 5:13] = buf[1, 5:13]                                    # at the anchor's position: counts at travel 0
    assert _both(grid, geom, buf, p, 0.0)["records"] == 2


def test_offset_and_drift_do_not_matter():
    """The same packets shifted by a constant that is exact in f32 give the same q to the bit: whatever is common to every
    record of the trail cancels in K4."""
    rng = np.random.default_rng(5)
    K = 16
    x, y = rng.integers(-2048, 2048, K) / 1024.0, rng.integers(-2048, 2048, K) / 1024.0
    yaw = rng.uniform(-3, 3, K)
    d = rng.uniform(0.1, 1.1, (K, 4))
    base = KR.points(TR.pack([1] * K, x, y, yaw, d), 6.0)
    for sx, sy in ((64.0, -32.0), (0.5, 1024.0)):
        xs, ys = (x + sx).astype(np.float32), (y + sy).astype(np.float32)
        assert (xs.astype(np.float64) == x + sx).all() and (ys.astype(np.float64) == y + sy).all()
        got = KR.points(TR.pack([1] * K, xs, ys, yaw, d), 6.0)
        assert got[1].tobytes() == base[1].tobytes() and got[2].tobytes() == base[2].tobytes()
        assert got[0]["records"] == base[0]["records"] == K and got[0]["ax"] == base[0]["ax"] + sx


def test_no_hits_no_records_and_no_free_cell(small):
    grid, T = small
    buf = T["pkts"][:12].copy()
    p = dict(n_rot=8, min_hits=4)
    blind = buf.copy()
    blind[:, 25:41] = 0
    r = _both(grid, SMALL_GEOM, blind, p, 0.8, max_dist=3.0)
    assert (r["status"], r["records"], r["hits"], r["anchor"], r["agent"], r["gx"], r["score"]) == (KR.NO_CANDIDATE, 12, 0, 11, 1, -1, 0)
    assert r["ax"] == float(np.frombuffer(bytes(buf[11, 5:9]), "<f4")[0]) and r["x"] == 0.0
    broken = buf.copy()
    broken[:, 0] = 0
    r = _both(grid, SMALL_GEOM, broken, p, 0.8, max_dist=3.0)
    assert r["status"] == KR.NO_RECORD and r["anchor"] == -1
    assert all(r[f] == 0 for f in KR.FIELDS if f not in ("status", "anchor"))
    short = _both(grid, SMALL_GEOM, buf, p, 0.8, max_dist=3.0, lengths=np.full(12, 40))
    assert short["status"] == KR.NO_RECORD
    for box in ((20, 40, 21, 44), (30, 30, 30, 40), (68, 0, 70, 68)):          # a wall's cells, an empty box, off the grid
        r = _both(grid, SMALL_GEOM, buf, dict(p, box=box), 0.8, max_dist=3.0)
        assert (r["status"], r["records"], r["anchor"]) == (KR.NO_CANDIDATE, 12, 11) and r["hits"] > 0


def test_ranges_that_are_not_numbers():
    grid, geom = _hand_grid()
    buf = TR.pack([1, 1], [0.0, 0.0], [0.0, 0.0], [0.0, 1.0], [[math.nan, math.inf, -math.inf, 1.0], [1.125, 0.04, 1.21, -1.0]])
    r = _both(grid, geom, buf, dict(radius=0, n_rot=4, sep_rot=1, min_hits=1), 1.0)
    assert (r["records"], r["hits"]) == (2, 2)                      # 1.0 and 1.125 (the filter is 0.05 < d <= 1.2)


def test_protocol_trail_reloc_move_is_rule_k7():
    P = importlib.import_module(load_pkg().__name__ + ".protocol")
    assert P.TRAIL_RELOC_DTYPE == KR.TRAIL_RELOC_DTYPE
    r = np.zeros(1, dtype=P.TRAIL_RELOC_DTYPE)[0]
    r["x"], r["y"], r["yaw"], r["ax"], r["ay"] = 4.25, 2.25, 2 * math.pi / 180 * 37, 100.0, 200.0
    for pose in ((100.0, 200.0, 0.5), (99.2, 203.1, -2.0), (4.0, 4.0, 3.0)):
        assert tuple(float(v) for v in P.trail_reloc_move(r, *pose)) == KR.move(r, *pose)
    x, y, yaw = P.trail_reloc_move(r, np.array([100.0, 99.2]), np.array([200.0, 203.1]), np.array([0.5, -2.0]))
    assert (float(x[0]), float(y[0])) == (4.25, 2.25) and (float(x[1]), float(y[1]), float(yaw[1])) == KR.move(r, 99.2, 203.1, -2.0)


# ---- what the rule recovers ----------------------------------------------------------------------------------------------------------
# (filter, K, min_hits, travel, recovered, accepted) of 16 trails, seed 7, noise 0.01 m, 180 rotations.  travel: the 3.0 m filter
# leaves K8 2.8 m at 5 cm cells; a trail of 64 steps of 0.05 m is 3.15 m long, so its first records may not count
RECOVERY = [(3.0, 64, 40, 2.8, 16, 16), (3.0, 32, 40, 2.8, 16, 14), (1.2, 64, 20, 4.0, 15, 13)]


@pytest.mark.parametrize("far,K,min_hits,travel,n_rec,n_acc", RECOVERY, ids=["3.0m-64", "3.0m-32", "1.2m-64"])
def test_recovery_table(far, K, min_hits, travel, n_rec, n_acc):
    grid = RR.world()
    T = KR.world_trails(grid, WORLD_GEOM, seed=7, n=16, K=K, far=far)
    out, _ = KR.reloc_trails(grid, WORLD_GEOM, T["pkts"], T["gsize"], dict(min_hits=min_hits), travel, max_dist=far)
    rec = np.array([KR.recovered(out[i], T["true"][i, -1], T["phi"][i], WORLD_GEOM, 180) for i in range(16)])
    acc = out["accepted"].astype(bool)
    print(f"filter {far} m, K {K}: recovered {rec.sum()} of 16, accepted {acc.sum()}, hit points {out['hits'].min()}..{out['hits'].max()}")
    assert not (acc & ~rec).any(), "an accepted trail lies outside one cell and two rotation steps"
    if far == 3.0:
        assert rec.sum() >= 12
    assert (int(rec.sum()), int(acc.sum())) == (n_rec, n_acc)
