"""The map merge session's rules (tests/merge_rules.py) run on the CPU with the oracle's icp_planar, voxel_downsample,
grid_to_pcd and rasterise over tests/golden/session_512.npz: the flow the GPU test (tests/test_gpu_merge.py) then holds the
device session to, step by step."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import oracle as orc
import merge_rules as R


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(GOLDEN, "session_512.npz"), allow_pickle=False)["grid"]


def session():
    return R.Session(orc.grid_to_pcd, orc.icp_planar, orc.voxel_downsample, orc.rasterise)


def test_the_golden_map_is_what_the_cases_assume(grid):
    rows, cols = np.nonzero(grid > 50)
    assert len(rows) == 437
    p = R.occupied_points(grid)
    assert (p == orc.grid_to_pcd(grid, R.RES, R.OX, R.OY)).all()
    corners = np.array([[R.OX, R.OY], [R.OX + 25.6, R.OY], [R.OX, R.OY + 25.6], [R.OX + 25.6, R.OY + 25.6]])
    d = np.sqrt(((p[:, None, :] - corners[None, :, :]) ** 2).sum(-1))
    assert d.min() > 5.0                                       # every occupied cell more than 5 m from the grid's corners
    assert 0 < (rows < 270).sum() < 437


def test_moved_is_the_rigid_transform_written_out():
    rng = np.random.default_rng(5)
    p = rng.uniform(-20, 20, (300, 2))
    a = 0.3
    T = np.array([[np.cos(a), -np.sin(a), 1.5], [np.sin(a), np.cos(a), -0.25], [0, 0, 1.0]])
    q = R.moved(p, T)
    np.testing.assert_allclose(q, p @ T[:2, :2].T + T[:2, 2], rtol=0, atol=1e-13)
    for i in (0, 17, 299):                                     # scalar by scalar: the very operations, in their order
        x, y = float(p[i, 0]), float(p[i, 1])
        assert q[i, 0] == (T[0, 0] * x + T[0, 1] * y) + T[0, 2] and q[i, 1] == (T[1, 0] * x + T[1, 1] * y) + T[1, 2]
    assert (R.moved(p, np.eye(3)) == p).all()
    assert (R.moved(p, T.ravel()) == q).all()


def test_six_map_sequence(grid):
    s = session()
    seen = {}
    for name, g, res, ox, oy, want in R.sequence(grid):
        before = s.cloud.copy()
        r = s.callback(g, res, ox, oy)
        seen[name] = r
        assert r["status"] == want, (name, r)
        assert r["n_global"] == len(s.cloud)
        if want == R.ADOPTED:
            assert (s.cloud == orc.grid_to_pcd(g, res, ox, oy)).all() and (s.res, s.origin) == (res, [ox, oy])
            assert (r["T"] == np.eye(3)).all() and r["iterations"] == 0
        elif want == R.MERGED:
            assert r["fitness"] == 1.0 and r["rmse"] < 0.05 and 1 <= r["iterations"] <= 30
            local = orc.grid_to_pcd(g, res, ox, oy)
            assert (s.cloud == orc.voxel_downsample(np.concatenate([before, R.moved(local, r["T"])]), R.RES)).all()
            assert len(before) <= len(s.cloud) <= len(before) + len(local)
        else:
            assert r["fitness"] == 0.0 and r["rmse"] == 0.0 and (r["T"] == np.eye(3)).all() and r["iterations"] == 1
            assert (s.cloud == before).all()                   # a rejected map leaves the cloud untouched
        assert (s.res, s.origin) == (R.RES, [R.OX, R.OY])      # adopted once
        out, origin = s.publish()
        assert (out == 100).sum() <= len(s.cloud) and (origin == s.cloud.min(0)).all()
    # the shifted copy is pulled back by the shift; the rotated maps by their angle
    T = seen["shifted"]["T"]
    assert abs(T[0, 2] + 0.10) < 1e-9 and abs(T[1, 2] - 0.15) < 1e-9 and abs(T[0, 0] - 1.0) < 1e-12
    for name, deg in (("rot3", 3.0), ("rot12", 12.0)):
        T = seen[name]["T"]
        assert abs(np.degrees(np.arctan2(T[1, 0], T[0, 0])) + deg) < 0.5
    assert seen["rot12"]["iterations"] > seen["rot3"]["iterations"]
    assert seen["rows_below_270"]["n_local"] == int((grid[:270] > 50).sum())


def test_empty_map_changes_nothing(grid):
    s = session()
    empty = np.full((8, 8), -1, dtype=np.int8)
    r = s.callback(empty, 0.05, 0.0, 0.0)
    assert r["status"] == R.EMPTY and len(s.cloud) == 0 and s.publish() == (None, None)
    assert s.callback(grid, R.RES, R.OX, R.OY)["status"] == R.ADOPTED            # the first map with points is adopted
    before = s.cloud.copy()
    r = s.callback(np.full((8, 8), 50, dtype=np.int8), 0.1, 3.0, 4.0)            # 50 is not > 50
    assert r["status"] == R.EMPTY and r["n_global"] == 437 and (s.cloud == before).all()
    assert (s.res, s.origin) == (R.RES, [R.OX, R.OY])


def test_fitness_gate_cases(grid):
    """The map plus a block in the grid's corner, against the map itself: the block's cells never correspond at 1 m, the map's
    own all do, so the fitness is a ratio of counts: 437/537 passes the gate of 0.6, 437/837 does not."""
    cases = R.gate_cases(grid)
    assert [c[2] for c in cases] == [437 / 537, 437 / 837]
    for name, g, fitness, want in cases:
        s = session()
        s.callback(grid, R.RES, R.OX, R.OY)
        before = s.cloud.copy()
        r = s.callback(g, R.RES, R.OX, R.OY)
        assert r["fitness"] == fitness and r["status"] == want, (name, r)
        if want == R.REJECTED:
            assert (s.cloud == before).all()
        else:
            assert len(s.cloud) == 437 + (len(orc.grid_to_pcd(g, R.RES, R.OX, R.OY)) - 437)     # the block's cells are new voxels
