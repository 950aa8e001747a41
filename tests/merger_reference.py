"""Reader of tests/golden/merger_calls.npz: what the reference's own MapMerger (server_nodes/map_merger.py) did on built
grids, clouds and callback sequences (tests/golden/make_merger_golden.py has the layout).  Plain numpy."""
import os

import numpy as np

import merge_rules as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALL_ICP, CALL_TRANSFORM, CALL_IADD, CALL_VOXEL, CALL_PUBLISH = 1, 2, 3, 4, 5
STATUS_OF_CALLS = {(): R.EMPTY, (CALL_PUBLISH,): R.ADOPTED, (CALL_ICP,): R.REJECTED,
                   (CALL_ICP, CALL_TRANSFORM, CALL_IADD, CALL_VOXEL, CALL_PUBLISH): R.MERGED}


def load():
    fx = np.load(os.path.join(GOLDEN, "merger_calls.npz"), allow_pickle=False)
    assert fx["call_codes"].tolist() == [CALL_ICP, CALL_TRANSFORM, CALL_IADD, CALL_VOXEL, CALL_PUBLISH]
    return fx


def published(fx, key):
    """(grid int8 [h, w], origin [2], res) of the message the reference published for `key`, or None."""
    if key + "_pub_data" not in fx.files:
        return None
    grid = fx[key + "_pub_data"]
    assert grid.shape == tuple(fx[key + "_pub_dims"])
    return grid, fx[key + "_pub_origin"], float(fx[key + "_pub_res"][0])


def grids(fx):
    """[(key, data, res, ox, oy, points of the reference's grid_to_pcd)]."""
    return [(f"g{i}", fx[f"g{i}_data"]) + tuple(fx[f"g{i}_geom"].tolist()) + (fx[f"g{i}_pcd"],) for i in range(int(fx["n_grids"][0]))]


def clouds(fx):
    """[(key, xy, res)]."""
    return [(f"c{i}", fx[f"c{i}_xy"], float(fx[f"c{i}_res"][0])) for i in range(int(fx["n_clouds"][0]))]


def sequences(fx):
    """[[(key, data, res, ox, oy, fitness the registration returned or nan)]]."""
    return [[(f"q{i}_m{j}", fx[f"q{i}_m{j}_data"]) + tuple(fx[f"q{i}_m{j}_geom"].tolist()) + (float(fx[f"q{i}_m{j}_fitness"][0]),)
             for j in range(int(fx[f"q{i}_n"][0]))] for i in range(int(fx["n_sequences"][0]))]


def same_map(got, want):
    """got: (grid, origin) of rasterise; want: published()."""
    if want is None:
        assert got is None or got[0] is None
        return
    assert got[0] is not None and got[0].shape == want[0].shape, (None if got[0] is None else got[0].shape, want[0].shape)
    assert (got[0] == want[0]).all()
    assert np.asarray(got[1], dtype=np.float64).tobytes() == want[1].tobytes()          # the origin's bits
