"""The order-preserving compaction (csrc/compact.h) at its own edges: the chunk of 1024 items, the wave of 64 and the
256 items a workgroup ranks per pass.  Every user of it is driven with shapes chosen for those edges and compared, bit for
bit and in order, with the CPU restatements: grid_to_pcd against np.argwhere, and the frontier cells, clusters, members,
centroids and both target assignments on a 36 x 36 map (1296 cells: one full chunk and a partial one of 272)."""
import math

import numpy as np
import pytest

import assign_rules as A
import plan_rules as R
from conftest import load_pkg
from oracle import oracle as orc
from test_gpu_frontier_targets import oracle_targets_py

pytestmark = pytest.mark.gpu
CHUNK = 1024


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


# ---- grid_to_pcd -------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 1024), (1, 1025), (3, 343), (2, 1024), (5, 1000)]


def patterns(n):
    """name -> bool [n]: which cells are marked."""
    i = np.arange(n)
    edge = np.zeros(n, dtype=bool)
    edge[[k for k in (1023, 1024) if k < n]] = True
    return {
        "none": np.zeros(n, dtype=bool),
        "all": np.ones(n, dtype=bool),
        "first": i == 0,
        "last": i == n - 1,
        "1023_1024": edge,
        "wave_and_pass_edges": np.isin(i % CHUNK, (63, 64, 255, 256)),
        "random_half": np.random.default_rng(n).random(n) < 0.5,
    }


@pytest.fixture(scope="module")
def merger(pkg):
    with pkg.QuasarMapper() as m:
        yield m


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_to_pcd_at_chunk_wave_and_pass_edges(merger, shape):
    h, w = shape
    res, ox, oy = 0.05, -12.8, 3.2
    for name, mask in patterns(h * w).items():
        flat = np.full(h * w, -1, dtype=np.int8)
        flat[mask] = 100
        if mask.any():
            flat[np.flatnonzero(mask)[0]] = 51              # the smallest marked value
        if not mask.all():
            flat[np.flatnonzero(~mask)[0]] = 50             # the largest unmarked one
        grid = flat.reshape(h, w)
        rc = np.argwhere(grid > 50)                         # row-major (map_merger.py:72)
        assert len(rc) == mask.sum()
        want = np.stack([rc[:, 1].astype(np.float64) * res + ox, rc[:, 0].astype(np.float64) * res + oy], axis=1)
        got = merger.grid_to_pcd(grid, res, ox, oy)
        assert got.shape == want.shape and (got == want).all(), (shape, name)
        assert (orc.grid_to_pcd(grid, res, ox, oy) == want).all(), (shape, name)


# ---- frontiers on 36 x 36 ------------------------------------------------------------------------------------------------
SIZE, RES = 36, 0.25                # origin (0, 0): every cell centre and every mean of centres is exact in fp64


def cx(g):
    return (g + 0.5) * RES


def free_run(m, gy, a, b):
    """FREE cells [a, b) of row gy (a ray frees all its cells but the last)."""
    m.update_rays(np.array([cx(a)]), np.array([cx(gy)]), np.array([cx(b)]), np.array([cx(gy)]), np.zeros(1, dtype=np.uint8))


@pytest.fixture(scope="module")
def map36(pkg):
    m = pkg.QuasarMapper(SIZE, RES, 0.0, 0.0)
    free_run(m, 1, 1, 34)
    free_run(m, 28, 10, 23)         # linear indices 1018 .. 1030: both sides of the chunk border at 1024 = cell (16, 28)
    free_run(m, 34, 1, 34)          # wholly in the last, partial chunk
    free_run(m, 4, 1, 3)            # a cluster of two and a cluster of one, both further from the middle of the map
    free_run(m, 31, 33, 34)         # than rows 1 and 34 are
    grid = m.grid_i8()
    cells = orc.frontier_cells(grid)
    yield m, grid, cells
    m.close()


def components(cells):
    """linear index -> the lowest linear index of its 4-connected component, over the frontier cells [n, 2] (gx, gy)."""
    lin = [int(y) * SIZE + int(x) for x, y in cells.tolist()]
    root, todo = {}, set(lin)
    for s in sorted(lin):
        if s in root:
            continue
        root[s], stack = s, [s]
        while stack:
            c = stack.pop()
            for nb in ((c - 1) if c % SIZE else -1, (c + 1) if (c + 1) % SIZE else -1, c - SIZE, c + SIZE):
                if nb in todo and nb not in root:
                    root[nb] = s
                    stack.append(nb)
    return lin, root


def test_frontiers_across_the_chunk_border(map36):
    m, grid, cells = map36
    all1, all3 = orc.frontier_clusters(cells, SIZE, 1), orc.frontier_clusters(cells, SIZE, 3)
    lin, root = components(cells)
    # the input is what it claims to be, by the oracle's output
    members = {}
    for c in lin:
        members.setdefault(root[c], []).append(c)
    assert [[len(v), r % SIZE, r // SIZE] for r, v in sorted(members.items())] == all1[:, :3].tolist()
    assert any(min(v) < CHUNK <= max(v) for v in members.values()), "no cluster spans linear index 1024"
    assert any(min(v) >= CHUNK for v in members.values()), "no cluster lies wholly in the last, partial chunk"
    assert {1, 2} <= set(all1[:, 0].tolist()) and len(all3) < len(all1)
    assert SIZE * SIZE > CHUNK and SIZE * SIZE % CHUNK
    # the device against the oracle
    assert (m.frontier_cells() == cells).all() and m.frontier_cells().shape == cells.shape
    assert (m.frontier_clusters(1) == all1).all() and (m.frontier_clusters(3) == all3).all()
    mem = m.frontier_members()
    assert mem.shape == (len(cells), 3) and (mem[:, :2] == cells).all()
    assert mem[:, 2].tolist() == [root[c] for c in lin]
    for mc, st in ((1, all1), (3, all3)):
        want = orc.cluster_centroids_world(st, RES, 0.0, 0.0)
        got = np.array(m.frontier_centroids(mc), dtype=np.float64).reshape(-1, 2)
        assert got.shape == want.shape and (got == want).all()
        _, _, dev, stats = m.frontier_targets(np.zeros((0, 2)), min_cluster=mc, return_centroids=True)   # the device's division
        assert dev.shape == want.shape and (dev == want).all() and stats["n_centroids"] == len(want)


def bots_for(cents, first):
    """One bot nearest the cluster whose first cell is `first`, one at NaN, one equidistant from two centroids."""
    near = cents[first]
    tie = None
    for a in range(len(cents)):
        for b in range(a + 1, len(cents)):
            if cents[a][0] == cents[b][0]:
                tie = (a, b)
    assert tie is not None
    mid = (cents[tie[0]][0], (cents[tie[0]][1] + cents[tie[1]][1]) / 2)
    d = [math.sqrt((mid[0] - x) * (mid[0] - x) + (mid[1] - y) * (mid[1] - y)) for x, y in cents]
    # an exact tie for the nearest once the first bot has taken its cluster: the lower index must win it
    assert d[tie[0]] == d[tie[1]] == min(v for k, v in enumerate(d) if k != first)
    return [(near[0] + RES, near[1] + RES), (math.nan, 1.0), mid], tie


def test_targets_on_the_36_map(map36):
    m, grid, cells = map36
    for mc in (1, 3):
        st = orc.frontier_clusters(cells, SIZE, mc)
        cents = [tuple(c) for c in orc.cluster_centroids_world(st, RES, 0.0, 0.0).tolist()]
        first = [i for i, (_, fx, fy, _, _) in enumerate(st.tolist()) if (fx, fy) == (10, 28)]
        assert len(first) == 1
        bots, tie = bots_for(cents, first[0])
        for sep in (0.0, 0.6, 2.0):       # 2.0: the first bot's target blocks the last bot's second choice
            want = oracle_targets_py(cents, bots, sep)
            idx, xy, dev, stats = m.frontier_targets(bots, separation=sep, min_cluster=mc, return_centroids=True)
            assert (dev == np.array(cents)).all() and stats["fallbacks"] == 0
            assert idx.tolist() == want.tolist() and idx[0] == first[0] and idx[1] == -1 and idx[2] == tie[0]
            assert (xy[[0, 2]] == np.array(cents)[want[[0, 2]]]).all() and np.isnan(xy[1]).all()
            # by path cost: the runs are one cell wide and apart, so clearance 0 and each bot reaches its own run at most
            res = m.frontier_targets_by_path(bots, separation=sep, min_cluster=mc, clearance=0, return_centroids=True)
            assert (res["centroids"] == np.array(cents)).all()
            A.same(res, A.assign(grid, cents, bots, RES, 0.0, 0.0, sep, clearance=0))
            assert res["idx"][0] == first[0] and res["status"][1] == R.NO_START
