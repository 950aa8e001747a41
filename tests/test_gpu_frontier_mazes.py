"""The frontier kernels (csrc/frontier.hip) on the built scenes of maze_scenes.py: one cluster of thousands of cells that
winds through the whole grid (serpentine, spiral, ring), one whose unions all meet late and far from its root (comb),
thousands of one-cell clusters (lattice) and clusters that touch only diagonally (diagonal_pairs), on grids whose last tile
is full, 8 cells wide and 4 cells wide.  With clearance-free corridors in UNKNOWN space every FREE cell is a frontier cell.
Cells, clusters, members and centroids are compared with == and in order against the oracle and a flood fill."""
import numpy as np
import pytest

import maze_scenes as S
from conftest import load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
CASES = [(name, size) for name in sorted(S.FRONTIER_SCENES) for size in (200, 256, 68)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"{p[0]}-{p[1]}")
def scene(request, pkg):
    name, size = request.param
    grid, rays, res, ox, oy = S.build(name, size)
    m = pkg.QuasarMapper(size, res, ox, oy)
    S.paint(m, rays, res, ox, oy)
    got = m.grid_i8()
    assert got.shape == grid.shape and (got == grid).all(), np.argwhere(got != grid)[:8].tolist()
    cells = orc.frontier_cells(grid)
    assert len(cells) == (grid == 0).sum()
    yield dict(name=name, size=size, m=m, grid=grid, cells=cells, res=res, ox=ox, oy=oy)
    m.close()


def test_cells(scene):
    m, cells = scene["m"], scene["cells"]
    for _ in range(2):
        got = m.frontier_cells()
        assert got.shape == cells.shape and got.dtype == cells.dtype and (got == cells).all()


@pytest.mark.parametrize("min_cluster", [1, 3])
def test_clusters_and_centroids(scene, min_cluster):
    m, cells, size = scene["m"], scene["cells"], scene["size"]
    want = orc.frontier_clusters(cells, size, min_cluster)
    first = None
    for _ in range(2):                # the labelling is racy inside and must not be outside
        got = m.frontier_clusters(min_cluster)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert (got == want).all(), (int((got != want).any(axis=1).sum()), got[(got != want).any(axis=1)][:4].tolist())
        first = got if first is None else first
        assert got.tobytes() == first.tobytes()
    cents = np.array(m.frontier_centroids(min_cluster), dtype=np.float64).reshape(-1, 2)
    ref = orc.cluster_centroids_world(want, scene["res"], scene["ox"], scene["oy"])
    assert cents.shape == ref.shape and (cents == ref).all()
    if scene["name"] in S.CORRIDORS:
        assert len(want) == 1 and want[0, 0] == len(cells)
    elif scene["name"] == "lattice":
        assert len(want) == (len(cells) if min_cluster == 1 else 0)
    else:
        assert len(want) == len(cells) // 4


def test_members(scene):
    m, cells, size = scene["m"], scene["cells"], scene["size"]
    lin, root = S.components(cells, size)
    want = np.array([root[c] for c in lin], dtype=np.int32)
    first = None
    for _ in range(2):
        mem = m.frontier_members()
        assert mem.shape == (len(cells), 3) and mem.dtype == np.int32
        assert (mem[:, :2] == cells).all()
        bad = np.nonzero(mem[:, 2] != want)[0]
        assert len(bad) == 0, (len(bad), mem[bad[:8]].tolist(), want[bad[:8]].tolist())
        first = mem if first is None else first
        assert mem.tobytes() == first.tobytes()
    if scene["name"] == "comb":       # all teeth hang under the top of the first
        lo = S.GEOMETRY[size][3]
        assert set(want.tolist()) == {lo * size + lo}
