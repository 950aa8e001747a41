"""The relaxation rounds of qs_plan_paths on maps whose traversable cells lie in one 64x64 tile: the seeded tile settles in
the first round and appends nothing, so exactly one round runs per request group however many empty rounds follow it,
and the fields and plans still equal the CPU restatement (plan_rules.py)."""
import numpy as np
import pytest

import plan_rules as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def room(m, x0, x1, y0, y1, wall_x=None):
    """Free rows from x0 to x1 for y in [y0, y1), and an optional wall of OCCUPIED cells at wall_x with a gap at the top."""
    ys = np.arange(y0, y1, m.res / 2)
    m.update_rays(np.full(len(ys), x0), ys, np.full(len(ys), x1), ys, np.zeros(len(ys), dtype=np.uint8))
    if wall_x is not None:
        wy = np.arange(y0, y1 - 0.6, m.res)
        wx = np.full(len(wy), wall_x)
        m.update_rays(wx, wy, wx, wy, np.ones(len(wy), dtype=np.uint8))


def requests(m, t, k, seed):
    yy, xx = np.nonzero(t)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(yy), size=2 * k, replace=False)
    cells = [(int(xx[i]), int(yy[i])) for i in pick]
    xy = [(m.ox + (gx + 0.5) * m.res, m.oy + (gy + 0.5) * m.res) for gx, gy in cells]
    return xy[:k], xy[k:], cells[k:]


@pytest.mark.parametrize("size, origin", [(64, -1.6), (200, -5.0)])
def test_one_tile_one_round(pkg, size, origin):
    with pkg.QuasarMapper(size, 0.05, origin, origin) as m:
        # everything inside the grid's first tile (cells 4 .. 59)
        lo, hi = origin + 4 * 0.05, origin + 59 * 0.05
        room(m, lo, hi, lo, hi, wall_x=origin + 30.5 * 0.05)
        t = m.traversable(2).astype(bool)
        yy, xx = np.nonzero(t)
        assert len(yy) and xx.max() < 64 and yy.max() < 64
        graph = R.move_graph(t)
        starts, goals, goal_cells = requests(m, t, 6, size)
        for _ in range(2):            # a second call must not see anything of the first call's lists
            res = m.plan_paths(starts, goals, return_paths=True)
            assert res["stats"]["groups"] == 1 and (res["status"] == R.OK).sum() >= len(starts) // 2
            assert res["stats"]["rounds"] == 1 and res["stats"]["tile_visits"] == len(starts), res["stats"]
            for i in range(len(starts)):
                want = R.plan(t, starts[i], goals[i], m.res, m.ox, m.oy, graph=graph)
                assert res["status"][i] == want["status"], i
                if want["status"] != R.OK:
                    continue
                assert tuple(res["waypoint_cell"][i]) == want["cell"] and res["cost"][i] == want["cost"], i
                assert [tuple(c) for c in res["paths"][i].tolist()] == want["path"], i
        for gx, gy in goal_cells[:3]:
            f = m.distance_field((m.ox + (gx + 0.5) * m.res, m.oy + (gy + 0.5) * m.res))
            assert (f == R.field_scipy(t, (gx, gy), graph)).all()
