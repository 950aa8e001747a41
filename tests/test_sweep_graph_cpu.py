"""Graph mode of the sweep path on the CPU: known answers of the signature rule, the restatement's pose graph pinned to the
reference-pinned oracle through shadow packets, and the conditions the room stream must meet for the GPU tests to mean
something.  No GPU."""
import importlib

import numpy as np
import pytest

import sweep_graph_rules as R
from conftest import load_pkg
from oracle import oracle as orc

F32_04 = np.float32(0.4)
F32_08 = np.float32(0.8)


def _sweep(right, front, left, w=5, fill=0.6):
    """One sweep whose three sectors hold one value each, everything between them `fill`."""
    r = np.full(181, fill, dtype=np.float32)
    r[0:2 * w + 1] = right
    r[90 - w:90 + w + 1] = front
    r[180 - 2 * w:181] = left
    return r


@pytest.mark.parametrize("front, left, right, want", [
    (0.3, 0.3, 0.3, 4),      # DEAD_END
    (0.3, 0.3, 0.6, 1),      # CORNER_L
    (0.3, 0.3, 0.9, 1),
    (0.3, 0.6, 0.3, 2),      # CORNER_R
    (0.3, 0.9, 0.3, 2),
    (0.9, 0.3, 0.3, 3),      # CORRIDOR
    (0.6, 0.3, 0.3, 0),      # ... needs an open front
    (0.9, 0.9, 0.9, 5),      # OPEN
    (0.9, 0.9, 0.6, 0),
    (0.3, 0.6, 0.6, 0),      # a wall ahead alone is nothing
    (0.6, 0.6, 0.6, 0),
])
def test_every_row_of_the_decision_table(front, left, right, want):
    for w in (0, 5, 29):
        assert R.signature(_sweep(right, front, left, w), w)[0] == want


def test_thresholds_at_and_beside_the_f32_value():
    # f32(0.4) widens to 0.4000000059604645: not < 0.40; its predecessor is
    assert float(F32_04) == 0.4000000059604645 and not float(F32_04) < 0.40
    below, above = np.nextafter(F32_04, np.float32(0)), np.nextafter(F32_04, np.float32(1))
    assert R.signature(_sweep(below, below, below))[0] == 4
    assert R.signature(_sweep(F32_04, F32_04, F32_04))[0] == 0
    assert R.signature(_sweep(above, above, above))[0] == 0
    # f32(0.8) widens to 0.800000011920929: > 0.80 already; its predecessor 0.7999999523162842 is not
    assert float(F32_08) > 0.80
    below8 = np.nextafter(F32_08, np.float32(0))
    assert not float(below8) > 0.80
    assert R.signature(_sweep(F32_08, F32_08, F32_08))[0] == 5
    assert R.signature(_sweep(below8, below8, below8))[0] == 0
    assert R.signature(_sweep(below, F32_08, below))[0] == 3 and R.signature(_sweep(below, below8, below))[0] == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 0.0, -0.0, -0.3])
def test_unusable_ranges_count_as_far(bad):
    w = 5
    # w unusable of 2w + 1: the median is the LARGEST usable value
    r = _sweep(0.3, 0.3, 0.3, w)
    vals = np.linspace(0.20, 0.39, w + 1).astype(np.float32)
    for first in (0, 90 - w, 180 - 2 * w):
        r[first:first + 2 * w + 1] = bad
        r[first:first + 2 * w + 1:2] = vals                  # w + 1 usable, interleaved with w unusable
    right, front, left = R.sector_values(r, w)
    assert right[0] == front[0] == left[0] == vals.max()
    assert R.signature(r, w)[0] == 4
    # w + 1 unusable: the sector is open
    r2 = r.copy()
    r2[90 - w] = bad                                         # the front sector loses one more
    assert np.isinf(R.sector_values(r2, w)[1][0])
    assert R.signature(r2, w)[0] == 3                        # left and right close, front open: CORRIDOR
    r3 = r2.copy()
    r3[0], r3[180 - 2 * w] = bad, bad
    assert R.signature(r3, w)[0] == 5


def test_half_width_zero_is_the_single_beam_rule():
    rng = np.random.default_rng(2)
    r = rng.uniform(0.0, 1.2, (400, 181)).astype(np.float32)
    r[rng.random(r.shape) < 0.05] = np.nan
    single = np.where(np.isfinite(r) & (r > 0), r, np.inf)
    want = R.decide(single[:, 90], single[:, 180], single[:, 0])
    assert (R.signature(r, 0) == want).all()
    assert len(set(want.tolist())) >= 5


def test_beams_just_outside_a_sector_do_not_count():
    for w in (0, 5, 29):
        r = _sweep(0.3, 0.3, 0.3, w, fill=9.0)
        base = R.signature(r, w)[0]
        assert base == 4
        for i in (2 * w + 1, 90 - w - 1, 90 + w + 1, 180 - 2 * w - 1):
            q = r.copy()
            q[i] = 0.01
            assert R.signature(q, w)[0] == base
        # ... while a sector made of far values with its neighbours close stays far
        q = np.full(181, 0.3, dtype=np.float32)
        q[90 - w:90 + w + 1] = 9.0
        assert R.sector_values(q, w)[1][0] == np.float32(9.0)


def test_ties_keep_the_value():
    r = _sweep(0.3, 0.5, 0.7)
    assert [float(v[0]) for v in R.sector_values(r)] == [float(np.float32(0.3)), float(np.float32(0.5)), float(np.float32(0.7))]


@pytest.fixture(scope="module")
def room():
    agent, x, y, yaw, ranges = R.room_stream()
    sg = R.SweepGraph()
    node, lm, pose, chain = sg.add_sweeps(agent, x, y, yaw, ranges)
    return dict(agent=agent, x=x, y=y, yaw=yaw, ranges=ranges, sg=sg, node=node, lm=lm, pose=pose)


def test_room_stream_conditions(room):
    g = room["sg"].graphs[0]
    n = len(room["agent"])
    assert n == 624 and (room["node"] == np.arange(n)).all()
    assert len(g.closures) >= 4
    owner = {int(k): int(a) for k, a in zip(room["node"], room["agent"])}
    assert sum(1 for (li, ni, _, _) in g.closures if owner[li] != owner[ni]) >= 1, "no closure across the two bots"
    assert len({t for _, _, t, _ in g.landmarks}) >= 2
    assert max(ni for _, ni, _, _ in g.closures) >= 0.9 * n
    assert all(any(abs(v) > 1e-3 for v in room["sg"].drift[b]) for b in (1, 2))
    assert all(room["sg"].zone[b] is not None for b in (1, 2))


def test_graph_part_equals_the_oracle_fed_shadow_packets(room):
    """A shadow packet: the same agent and f32 pose, the landmark byte set to the signature, all distances 0."""
    P = importlib.import_module(load_pkg().__name__ + ".protocol")
    n = len(room["agent"])
    pk = P.pack_packets(room["agent"], room["x"], room["y"], room["yaw"], np.zeros(n), np.zeros(n), np.zeros((n, 4)), room["lm"])
    o = orc.OracleMapper(200, 0.05, -5.0, -5.0)
    assert o.feed_stream(pk) == n
    g = room["sg"].graphs[0]
    idx, corr = o.closures(0)
    assert idx.tolist() == [[li, ni] for li, ni, _, _ in g.closures]
    np.testing.assert_allclose(corr, [[dx, dy] for _, _, dx, dy in g.closures], rtol=0, atol=1e-12)
    xy, ti = o.landmarks(0)
    assert ti.tolist() == [[t, li] for _, _, t, li in g.landmarks]
    np.testing.assert_allclose(xy, [[lx, ly] for lx, ly, _, _ in g.landmarks], rtol=0, atol=1e-12)
    assert o.n_nodes(0) == g.n_nodes
    for b in (1, 2):
        np.testing.assert_allclose(o.drift(b), room["sg"].drift[b], rtol=0, atol=1e-12)
    np.testing.assert_allclose(o.poses[:, :2], room["pose"][:, :2], rtol=0, atol=1e-12)


def test_rejected_records_and_other_graph_parameters():
    agent, x, y, yaw, ranges = R.room_stream()
    ok = np.ones(len(agent), dtype=bool)
    ok[[3, 4, 100]] = False
    sg = R.SweepGraph(gap=10, radius=0.3, damp=0.25)
    node, lm, pose, _ = sg.add_sweeps(agent, x, y, yaw, ranges, ok=ok, zone=False)
    assert (node[~ok] == -1).all() and (lm[~ok] == R.LM_REJECTED).all() and np.isnan(pose[~ok]).all()
    assert (node[ok] == np.arange(ok.sum())).all()
    g = sg.graphs[0]
    assert g.closures and all(ni - li >= 10 for li, ni, _, _ in g.closures)
    # three bots, a graph each: closures never cross
    a3 = (np.arange(len(agent)) % 3 + 1).astype(np.uint8)
    sg3 = R.SweepGraph(max_agent=3, bots_per_graph=1)
    node3, _, _, _ = sg3.add_sweeps(a3, x, y, yaw, ranges, zone=False)
    for b in (1, 2, 3):
        assert (node3[a3 == b] == np.arange((a3 == b).sum())).all()
        assert set(sg3.graphs[b - 1].closure_agents) <= {b}
