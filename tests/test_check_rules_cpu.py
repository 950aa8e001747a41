"""The sweep-check rules V1-V9 (include/quasar_slam.h, "sweep check") on the CPU: what the NumPy restatement (tests/check_rules.py)
says about sweeps sensed in the three-room world of tests/reloc_rules.py from true, slightly shifted and lost poses; V6's table at
equality and one f32 step to either side; V8's limits; the two forms of the restatement against each other."""
import functools
import importlib
import math

import numpy as np
import pytest

import check_rules as CR
import reloc_rules as RR
import sense_rules as SR
from conftest import load_pkg

SMIN, TOL = 0.02, 0.10
GEOM = RR.WORLD_GRID[1:]


@functools.lru_cache(maxsize=None)
def _world():
    grid = RR.world()
    poses, _ = RR.query_poses(grid, GEOM, 40, seed=7)
    return grid, poses


@functools.lru_cache(maxsize=None)
def _ranges(R, noise):
    grid, poses = _world()
    return SR.sense_ranges(grid, *GEOM, poses, max_range=R, noise_amp=noise, seed=1234)[0]


def _checks(R, noise, shift=(0.0, 0.0, 0.0)):
    """The 40 sweeps sensed at the true poses, checked from poses displaced by shift: [(fields, classes)]."""
    grid, poses = _world()
    p = CR.params(GEOM[0], tol=TOL)
    reported = (poses.astype(np.float64) + np.array(shift)).astype(np.float32)       # what a packet would carry
    return [CR.check_one(grid, GEOM, reported[k].astype(np.float64), _ranges(R, noise)[k], p, SMIN, R) for k in range(len(poses))]


@pytest.mark.parametrize("R", [1.2, 3.0])
@pytest.mark.parametrize("noise", [0.0, 0.03])
def test_a_sweep_at_its_true_pose_contradicts_nothing(R, noise):
    out = _checks(R, noise)
    for k, (r, cls) in enumerate(out):
        assert r["nearer"] == r["farther"] == r["missed"] == 0, f"sweep {k}: {r}"
        assert r["agree"] + r["unseen"] == 181 and r["status"] in (CR.OK, CR.UNDECIDED) and r["bad"] == 0
    assert any(r["status"] == CR.OK for r, _ in out), "no sweep was decided: the property above shows nothing"


@pytest.mark.parametrize("R", [1.2, 3.0])
def test_a_one_cell_shift_is_the_matchers_job(R):
    """One cell along either axis, in either direction: nothing is flagged (the worst sweep has 28 % of its decided beams bad at
    R = 3.0, 24 % at 1.2).  A shift of one cell on BOTH axes is 1.4 cells: there one sweep of 40 is flagged at R = 3.0 (36 %)."""
    for shift in ((0.05, 0.0, 0.0), (-0.05, 0.0, 0.0), (0.0, 0.05, 0.0), (0.0, -0.05, 0.0)):
        out = _checks(R, 0.0, shift)
        assert not any(r["status"] == CR.CONTRADICTS for r, _ in out), shift


def test_a_lost_pose_is_flagged():
    """Shifted by (0.30, 0.15) m.  Measured with this restatement: 30 of the 39 decided sweeps are flagged at R = 1.2 and 39 of
    39 at R = 3.0 (the figures of the prototype the rule was chosen with)."""
    got = {}
    for R in (1.2, 3.0):
        out = _checks(R, 0.0, (0.30, 0.15, 0.0))
        decided = [r for r, _ in out if r["status"] in (CR.OK, CR.CONTRADICTS)]
        got[R] = (sum(r["status"] == CR.CONTRADICTS for r in decided), len(decided))
    print("flagged of decided:", got)
    assert got[1.2][0] >= 27
    assert got[3.0][0] == got[3.0][1] > 0


def test_a_turned_pose_is_flagged_at_long_range():
    """Turned by 20 degrees: a return from d metres away lands d * sin(20 deg) to the side, more than tol = 0.10 m for every
    d > 0.3 m, so the longer filter sees more of it and flags most sweeps.  Measured: 19 of 40 at R = 1.2, 39 of 40 at R = 3.0."""
    got = {}
    for R in (1.2, 3.0):
        out = _checks(R, 0.0, (0.0, 0.0, math.radians(20)))
        got[R] = sum(r["status"] == CR.CONTRADICTS for r, _ in out)
    print("flagged of 40:", got)
    assert got[3.0] > got[1.2] > 0 and got[3.0] > 20


def test_both_forms_of_the_restatement_agree():
    grid, poses = _world()
    rng = np.random.default_rng(3)
    for k in range(0, 40, 5):
        pose = poses[k].astype(np.float64) + np.array([0.3, -0.2, 0.4]) * (k % 3)
        ranges = _ranges(3.0, 0.03)[k].copy()
        ranges[rng.random(181) < 0.2] = rng.choice(np.array([0.0, np.nan, 5.0, 0.5, -1.0], dtype=np.float32))
        for p, smax in ((CR.params(GEOM[0]), 1.2), (CR.params(GEOM[0], tol=0.0, count_missed=1, min_checked=0, max_bad_percent=0), 3.0)):
            a, ca = CR.check_one(grid, GEOM, pose, ranges, p, 0.1, smax)
            b, cb = CR.check_one_brute(grid, GEOM, pose, ranges, p, 0.1, smax)
            assert a == b and (ca == cb).all()
    # poses with no cell, off the grid and on an OCCUPIED cell
    for pose in ((np.nan, 0.0, 0.0), (0.0, 1e30, 0.0), (0.0, 0.0, np.inf), (-6.0, -6.0, 0.3), (-4.8 + 20.5 * 0.05, -4.8 + 50.5 * 0.05, 0.0)):
        a, ca = CR.check_one(grid, GEOM, np.array(pose), _ranges(1.2, 0.0)[0], CR.params(GEOM[0]), 0.1, 1.2)
        b, cb = CR.check_one_brute(grid, GEOM, np.array(pose), _ranges(1.2, 0.0)[0], CR.params(GEOM[0]), 0.1, 1.2)
        assert a == b and (ca == cb).all()
        if not all(math.isfinite(v) for v in pose) or abs(pose[1]) > 1e20:
            assert a["unseen"] == 181 and a["sin_yaw"] == a["cos_yaw"] == 0.0 and a["status"] == CR.UNDECIDED


def test_the_class_table_at_equality_and_one_step_either_side():
    assert {c[0] for c in CR.table_cases()} == {"hit", "clear", "unknown"}
    assert {(c[0], c[4]) for c in CR.table_cases()} >= {("hit", CR.NEARER), ("hit", CR.FARTHER), ("hit", CR.AGREE), ("hit", CR.MISSED),
                                                        ("hit", CR.UNSEEN), ("clear", CR.NEARER), ("clear", CR.AGREE),
                                                        ("unknown", CR.NEARER), ("unknown", CR.UNSEEN)}
    geom = CR.TABLE_GRID[1:]
    for kind, d, smin, smax, want in CR.table_cases():
        ranges = np.zeros(181, dtype=np.float32)
        ranges[CR.TABLE_BEAM] = d
        assert np.isnan(d) or float(ranges[CR.TABLE_BEAM]) == d, "the case's range must be a float32"
        p = CR.params(geom[0], tol=0.0)
        for one in (CR.check_one, CR.check_one_brute):
            r, cls = one(CR.table_grid(kind), geom, np.array(CR.TABLE_POSE), ranges, p, smin, smax)
            assert cls[CR.TABLE_BEAM] == want, (kind, d, smin, smax, want, int(cls[CR.TABLE_BEAM]))
            assert (r["sin_yaw"], r["cos_yaw"]) == (0.0, 1.0)


def test_summary_and_status():
    p = CR.params(0.05)
    cls = np.full(181, CR.UNSEEN, dtype=np.uint8)
    cls[:19] = CR.AGREE
    assert CR.summary(cls, p, 0.0, 1.0)["status"] == CR.UNDECIDED                # 19 < 20 checked
    cls[19] = CR.MISSED
    r = CR.summary(cls, p, 0.0, 1.0)
    assert (r["checked"], r["bad"], r["status"]) == (20, 0, CR.OK)                # MISSED is not counted by default
    assert CR.summary(cls, dict(p, count_missed=1, max_bad_percent=4), 0.0, 1.0)["status"] == CR.CONTRADICTS     # 100 > 80
    assert CR.summary(cls, dict(p, count_missed=1, max_bad_percent=5), 0.0, 1.0)["status"] == CR.OK              # 100 > 100 is false
    cls[:6] = CR.NEARER
    assert CR.summary(cls, p, 0.0, 1.0)["status"] == CR.OK                        # 600 > 600 is false
    cls[6] = CR.FARTHER
    r = CR.summary(cls, p, 0.0, 1.0)
    assert (r["bad"], r["status"], r["unseen"]) == (7, CR.CONTRADICTS, 161)
    assert CR.summary(np.full(181, CR.UNSEEN, dtype=np.uint8), dict(p, min_checked=0), 0.0, 1.0)["status"] == CR.OK


def test_every_limit_of_v8():
    ok = CR.params(0.05)
    assert CR.limit_ok(ok, 1.2, 0.05) and CR.limit_ok(dict(ok, tol=0.0, min_checked=0, max_bad_percent=0), 1.2, 0.05)
    assert CR.limit_ok(dict(ok, min_checked=181, max_bad_percent=100, count_missed=1), 1.2, 0.05)
    for bad in (dict(tol=-1e-9), dict(tol=math.nan), dict(tol=math.inf), dict(min_checked=-1), dict(min_checked=182),
                dict(max_bad_percent=-1), dict(max_bad_percent=101), dict(count_missed=2), dict(count_missed=-1), dict(reserved=1)):
        assert not CR.limit_ok(dict(ok, **bad), 1.2, 0.05), bad
    assert CR.limit_ok(ok, 12.7, 0.05) and not CR.limit_ok(ok, 12.71, 0.05)       # ceil(smax / res) + 1 <= 255
    assert CR.patch_radius(12.7, 0.05) == 255 and CR.patch_radius(1.2, 0.05) == 25


def test_records_offsets_and_the_withheld_set():
    """check() over packed records: acceptance, offset first then drift, rejected records, and the withheld set."""
    P = importlib.import_module(load_pkg().__name__ + ".protocol")
    grid, poses = _world()
    ranges = _ranges(3.0, 0.0)
    off, drift = {2: 0.5}, {1: (0.25, -0.125), 2: (-0.0625, 0.375)}
    agent = np.array([1, 2] * 4)
    sent = poses[:8].astype(np.float64).copy()
    for k in range(8):                              # what the bot must report for the ingest to form the true pose
        a = int(agent[k])
        sent[k, 0] -= off.get(a, 0.0) + drift[a][0]
        sent[k, 1] -= drift[a][1]
    sent[6, :2] += (0.30, 0.15)                     # a lost bot
    buf = P.pack_sweeps(agent, sent[:, 0], sent[:, 1], sent[:, 2], ranges[:8], odometry=True)
    buf[2, 4] = 9                                   # rejected: agent, magic, length
    buf[3, 0] ^= 1
    lens = np.full(8, 751, dtype=np.uint16)
    lens[4] = 750
    p = dict(tol=TOL)
    out, cls = CR.check(grid, GEOM, buf, p, lens, SMIN, 3.0, offset=off, drift=drift)
    rej = np.array([2, 3, 4])
    assert (out["status"][rej] == CR.NO_RECORD).all() and (cls[rej] == CR.NO_RECORD_BEAM).all()
    assert not out[rej].tobytes().strip(b"\0\1"), "a rejected record is zero apart from its status"
    keep = np.array([0, 1, 5, 7])
    assert (out["status"][keep] == CR.OK).all() and (out["bad"][keep] <= 2).all() and (out["accepted_record"][keep] == 1).all()
    assert out["status"][6] == CR.CONTRADICTS
    assert CR.withheld(out).tolist() == [False] * 6 + [True, False]
    broken = CR.break_magic(buf, CR.withheld(out))
    again, _ = CR.check(grid, GEOM, broken, p, lens, SMIN, 3.0, offset=off, drift=drift)
    assert again["status"][6] == CR.NO_RECORD and CR.differing(np.delete(again, 6), np.delete(out, 6)) == ""
    # without the offset and drift the same records are somewhere else
    plain, _ = CR.check(grid, GEOM, buf, p, lens, SMIN, 3.0)
    assert CR.differing(plain, out) != ""
    # records=: only those are restated
    some, _ = CR.check(grid, GEOM, buf, p, lens, SMIN, 3.0, offset=off, drift=drift, records=[0, 6])
    assert CR.differing(some[[0, 6]], out[[0, 6]]) == "" and (some["status"][[1, 5, 7]] == CR.NO_RECORD).all()
