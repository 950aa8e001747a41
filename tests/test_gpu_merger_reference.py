"""qs_grid_to_pcd, qs_rasterise and the map merge session against the reference's own MapMerger: tests/golden/
merger_calls.npz holds what server_nodes/map_merger.py's grid_to_pcd, publish_global_map and map_callback did on built grids
and clouds (tests/golden/make_merger_golden.py; tests/test_merger_reference_cpu.py holds the oracle and merge_rules.Session
to the same file).  Only the fixture is read; everything is compared with `==`.

The fixture's callbacks ran on a stand-in registration and a stand-in cloud, so the rows that register (merged, rejected)
are rebuilt here on maps whose registration is exact: the gate at 3/5 == 0.6, the second map of another resolution, the
order of the merged points.  ICP and voxel rounding against Open3D (N3) stay unpinned.
"""
import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import load_pkg
from oracle import oracle as orc
import merge_rules as R
import merger_reference as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def fx():
    return M.load()


@pytest.fixture(scope="module")
def m(pkg):
    with pkg.QuasarMapper() as mapper:
        yield mapper


def test_grid_to_pcd_and_rasterise_equal_the_reference(m, fx):
    for key, data, res, ox, oy, pcd in M.grids(fx):
        got = m.grid_to_pcd(data, res, ox, oy)
        assert got.shape == pcd.shape and got.tobytes() == pcd.tobytes(), key
        M.same_map(m.rasterise(pcd, res), M.published(fx, key))
    for key, xy, res in M.clouds(fx):
        M.same_map(m.rasterise(xy, res), M.published(fx, key))


@pytest.mark.parametrize("on_device", [False, True])
def test_session_empty_and_adopted_rows(m, fx, on_device):
    rows = [(key, data, res, ox, oy, pcd, M.published(fx, key)) for key, data, res, ox, oy, pcd in M.grids(fx)]
    for seq in M.sequences(fx):                               # the callbacks of the fixture that ran on a fresh merger
        key, data, res, ox, oy, _ = seq[0]
        rows.append((key, data, res, ox, oy, fx[key + "_global"], M.published(fx, key)))
    n_empty = 0
    for key, data, res, ox, oy, pcd, want in rows:
        m.merge_reset()
        m.merge_params()
        grid = data
        if on_device:
            grid = torch.from_numpy(np.ascontiguousarray(data)).cuda()
            torch.cuda.synchronize()
        r = m.merge_grid(grid, res, ox, oy)
        assert r["status"] == (R.ADOPTED if len(pcd) else R.EMPTY) and r["n_local"] == r["n_global"] == len(pcd), (key, r)
        assert (r["T"] == np.eye(3)).all() and r["iterations"] == 0
        cloud = m.merge_cloud()
        assert cloud.shape == pcd.shape and cloud.tobytes() == pcd.tobytes(), key
        M.same_map(m.merge_global_map(), want)
        n_empty += len(pcd) == 0
    assert n_empty >= 3


def cells(shape, where):
    g = np.full(shape, -1, dtype=np.int8)
    for r, c in where:
        g[r, c] = 100
    return g


NEAR = [(10, 10), (10, 14), (14, 10)]
FAR = [(60, 60), (60, 62), (62, 60)]                          # 3.5 m from the near cells at 0.05 m: beyond the 1.0 m threshold


@pytest.mark.parametrize("near,status", [(3, R.MERGED), (2, R.REJECTED)])
def test_gate_at_three_fifths(m, near, status):
    """A 5-cell local map of which `near` cells lie on cells of the global map and the others 3.5 m away: fitness near / 5.
    3 / 5 is the double the literal 0.6 is, and `fitness < 0.6` lets it pass (map_merger.py:54)."""
    first = cells((64, 64), NEAR)
    local = cells((64, 64), NEAR[:near] + FAR[:5 - near])
    m.merge_reset()
    m.merge_params()
    assert m.merge_grid(first, 0.05, -1.6, -1.6)["status"] == R.ADOPTED
    before = m.merge_cloud()
    r = m.merge_grid(local, 0.05, -1.6, -1.6)
    assert r["n_local"] == 5 and r["fitness"] == near / 5 and (near / 5 == 0.6) == (near == 3), r
    assert r["status"] == status, r
    if status == R.REJECTED:
        assert np.array_equal(m.merge_cloud(), before)
        M.same_map(m.merge_global_map(), m.rasterise(before, 0.05) + (0.05,))
    else:
        assert (r["T"] == np.eye(3)).all() and r["rmse"] == 0.0, r       # the matched cells coincide
        pts = m.grid_to_pcd(local, 0.05, -1.6, -1.6)
        want = orc.voxel_downsample(np.concatenate([before, R.moved(pts, r["T"])]), 0.05)
        assert np.array_equal(m.merge_cloud(), want)
        assert len(want) == 5                                            # the three shared cells averaged with themselves


def test_second_map_of_another_resolution(m):
    """After adoption at 0.1 m a map at 0.05 m that covers the same walls: the session goes on down-sampling and publishing
    at 0.1 m (map_merger.py:42, :60, :117), and the merged cloud is voxel_downsample(global points, then the moved local
    ones) in that order."""
    first = np.full((32, 32), -1, dtype=np.int8)
    first[4, 4:28] = 100; first[27, 4:28] = 100; first[4:28, 4] = 100; first[4:28, 27] = 100
    second = np.full((64, 64), -1, dtype=np.int8)
    second[8, 8:56] = 100; second[55, 8:56] = 100; second[8:56, 8] = 100; second[8:56, 55] = 100
    m.merge_reset()
    m.merge_params()
    assert m.merge_grid(first, 0.1, -1.6, -1.6)["status"] == R.ADOPTED
    before = m.merge_cloud()
    r = m.merge_grid(second, 0.05, -1.6, -1.6)
    assert r["status"] == R.MERGED and r["fitness"] == 1.0, r
    local = m.grid_to_pcd(second, 0.05, -1.6, -1.6)
    joined = np.concatenate([before, R.moved(local, r["T"])])
    want = orc.voxel_downsample(joined, 0.1)
    got = m.merge_cloud()
    assert np.array_equal(got, want)
    assert len(want) < len(orc.voxel_downsample(joined, 0.05))                               # the other resolution would show
    grid, origin = m.merge_global_map()
    wg, wo = orc.rasterise(want, 0.1)
    assert grid.shape == wg.shape and (grid == wg).all() and (origin == wo).all()
    assert grid.shape != orc.rasterise(want, 0.05)[0].shape
