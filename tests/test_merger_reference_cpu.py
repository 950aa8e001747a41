"""orc.grid_to_pcd, orc.rasterise and merge_rules.Session against the reference's own MapMerger: tests/golden/
merger_calls.npz holds what server_nodes/map_merger.py's grid_to_pcd, publish_global_map and map_callback did, loaded with
stand-in rclpy / nav_msgs / open3d modules (tests/golden/make_merger_golden.py).  Everything is compared with `==`: points,
dims, the origin's bits, data, which callbacks publish, the order and arguments of the cloud calls, which resolution is used.

The stand-in cloud of the generator records calls and stands for no Open3D arithmetic: every transformation is the identity
and voxel_down_sample hands its input back.  ICP and voxel rounding against Open3D (N3) stay unpinned.
"""
import numpy as np
import pytest

from oracle import oracle as orc
import merge_rules as R
import merger_reference as M


@pytest.fixture(scope="module")
def fx():
    return M.load()


def test_fixture_holds_the_cases(fx):
    gs, cs = M.grids(fx), M.clouds(fx)
    shapes = [g[1].shape for g in gs]
    assert any(h < w for h, w in shapes) and any(h > w for h, w in shapes) and (1, 1) in shapes and any(h == 1 < w for h, w in shapes)
    assert set(np.concatenate([g[1].reshape(-1) for g in gs]).tolist()) >= {-128, -1, 0, 50, 51, 100, 127}
    assert {g[2] for g in gs} >= {0.05, 0.1, 0.03} and any(g[3] < 0 for g in gs) and any(abs(g[3]) > 1000 for g in gs)
    assert any(len(g[5]) == 0 for g in gs)
    assert tuple(fx["g0_pub_dims"]) == (7, 14) and fx["g0_data"].shape == (7, 13)            # the ceil(...) + 1 edge
    widths = {}
    for key, xy, res in cs:
        if len(xy) == 5:
            widths.setdefault(res, []).append(int(fx[key + "_pub_dims"][1]))
    assert set(widths) == {0.05, 0.1, 0.03}
    for res, (exact, above, below) in widths.items():                    # an ulp beyond the integer extent: one more column
        assert above == exact + 1 and below == exact
    for key, xy, res in cs:
        assert (fx[key + "_pub_data"] == 100).sum() < len(xy) or len(xy) == 1      # points that truncate into one cell


def test_grid_to_pcd_equals_the_reference(fx):
    for key, data, res, ox, oy, pcd in M.grids(fx):
        got = orc.grid_to_pcd(data, res, ox, oy)
        assert got.shape == pcd.shape and got.tobytes() == pcd.tobytes(), key


def test_rasterise_equals_the_published_message(fx):
    n = 0
    for key, data, res, ox, oy, pcd in M.grids(fx):
        want = M.published(fx, key)
        assert (want is None) == (len(pcd) == 0)
        M.same_map(orc.rasterise(pcd, res), want)
        assert want is None or want[2] == res
        n += want is not None
    for key, xy, res in M.clouds(fx):
        M.same_map(orc.rasterise(xy, res), M.published(fx, key))
        n += 1
    assert n >= 20


class Recorder:
    """register and voxel of a Session that keep what they are called with; voxel hands its input back (as the generator's
    stand-in cloud does), register returns the identity and the fitness the fixture's registration returned."""

    def __init__(self):
        self.calls, self.fitness = [], None

    def register(self, local, cloud, threshold, iterations):
        self.calls.append((M.CALL_ICP, len(local), len(cloud), threshold, iterations))
        return np.eye(3), self.fitness, 0.0, 0

    def voxel(self, xy, res):
        self.calls.append((M.CALL_VOXEL, res, xy.copy()))
        return xy


def test_session_equals_map_callback(fx):
    seen = set()
    for seq in M.sequences(fx):
        rec = Recorder()
        s = R.Session(orc.grid_to_pcd, rec.register, rec.voxel, orc.rasterise)
        for key, data, res, ox, oy, fitness in seq:
            calls = tuple(fx[key + "_calls"].tolist())
            status = M.STATUS_OF_CALLS[calls]
            seen.add(status)
            rec.calls, rec.fitness = [], fitness
            n_before = len(s.cloud)
            r = s.callback(data, res, ox, oy)
            assert r["status"] == status, (key, r["status"], status)
            # the cloud calls, in order, with their arguments
            assert [c[0] for c in rec.calls] == [c for c in calls if c in (M.CALL_ICP, M.CALL_VOXEL)], key
            for c in rec.calls:
                if c[0] == M.CALL_ICP:
                    assert list(c[1:]) == fx[key + "_icp"].tolist(), key                     # local is the source, 1.0, 30
                else:
                    assert c[1] == fx[key + "_voxel_size"][0], key                          # the first map's resolution
                    assert c[2].tobytes() == fx[key + "_voxel_in"].tobytes(), key           # global points first
                    assert fx[key + "_iadd"].tolist() == [n_before, r["n_local"]] and (fx[key + "_T"] == np.eye(4)).all()
            assert [s.res] + list(s.origin) == fx[key + "_state"].tolist(), key             # adopted from the first message only
            assert s.cloud.tobytes() == fx[key + "_global"].tobytes(), key
            want = M.published(fx, key)
            assert (want is not None) == (status in (R.ADOPTED, R.MERGED)), key
            if want is not None:
                M.same_map(s.publish(), want)
                assert s.res == want[2], key                                                # the message's resolution
    assert seen == {R.EMPTY, R.ADOPTED, R.MERGED, R.REJECTED}
    # the gate's two sides are in the fixture: exactly 0.6 merged, the double below it rejected
    fits = {float(f): M.STATUS_OF_CALLS[tuple(fx[k + "_calls"].tolist())] for q in M.sequences(fx) for k, *_, f in q if f == f}
    assert fits[0.6] == R.MERGED and fits[float(np.nextafter(0.6, 0.0))] == R.REJECTED
    # and a later message of another resolution did not change the session's
    key = "q0_m2"
    assert fx[key + "_geom"][0] == 0.05 and fx[key + "_voxel_size"][0] == 0.1 == fx[key + "_pub_res"][0]
