"""The look-ahead word of the bucket chains (csrc/qs_internal.h, QsLmNode) on the CPU, from the restatement in
tests/chain_lookahead_rules.py: the lean owner's continuation rule on the look-ahead word finds what the rule on a node's last
entry finds and what a scan of the whole list finds; every scene of tests/test_gpu_chain_lookahead.py reaches the case it was
built for; and on the cycled session the restatement reproduces the oracle's closures with fewer walking decisions."""
import functools
import importlib

import numpy as np
import pytest

import chain_lookahead_rules as R
from conftest import load_pkg
from oracle import oracle as orc

GEOM = R.Geometry(*R.GRID, R.RADIUS)


def test_both_rules_find_the_scan_s_first_match():
    """Random chains in a 4 x 4 block of buckets, among them chains of 0, 1, 6, 7, 8, 13, 14, 15 and 22 entries (the node
    edges), 3000 queries at random poses and limits: both rules return the full scan's first match, and the look-ahead rule
    never needs more rounds."""
    rng = np.random.default_rng(7)
    want = [0, 1, 6, 7, 8, 13, 14, 15, 22, 30, 9, 3, 16, 21, 5, 12]
    cells = [(cx, cy) for cy in range(4) for cx in range(4)]
    pts = []
    for (cx, cy), n in zip(cells, want):                             # (a cell's entries cluster round two places: whole nodes out of reach)
        c = rng.uniform(0.1, 0.9, (2, 2))
        for k in range(n):
            u = np.clip(c[rng.integers(2)] + rng.uniform(-0.08, 0.08, 2), 0.02, 0.98)
            pts.append((R.GRID[2] + (20 + cx + u[0]) * 0.6, R.GRID[3] + (20 + cy + u[1]) * 0.6))
    pts = np.array(pts)[rng.permutation(len(pts))]
    idx = np.sort(rng.choice(5 * len(pts), len(pts), replace=False))
    ch = R.Chains(GEOM, pts, np.full(len(pts), 3), idx)
    ch.check_lookahead()
    assert sorted(len(c) for c in ch.chain.values()) == sorted(n for n in want if n)
    walked = fewer = 0
    for _ in range(3000):
        x, y = R.GRID[2] + rng.uniform(19.5, 24.5) * 0.6, R.GRID[3] + rng.uniform(19.5, 24.5) * 0.6
        eff = int(rng.integers(-1, 5 * len(pts) + 2))
        ref = ch.scan(x, y, 3, eff)
        m_last, r_last, _, _ = ch.query(x, y, 3, eff, "last")
        m_ahead, r_ahead, _, _ = ch.query(x, y, 3, eff, "ahead")
        assert m_last == ref and m_ahead == ref
        assert r_ahead <= r_last
        walked += r_last > 1
        fewer += r_ahead < r_last
    print(f"queries that walk {walked}, that the look-ahead saves a round {fewer}")
    assert walked > 50 and fewer > 5                                 # (the queries do walk, and the look-ahead does save rounds)


@functools.lru_cache(maxsize=None)
def _scene(name, min_between=30):
    stream, _ = R.scene_stream(name)
    o = orc.OracleMapper(*R.GRID, 0.0, max_agent=3)
    o.set_closure_params(R.RADIUS, min_between, 0.5)
    o.feed_stream(stream)
    xy, ti = o.landmarks(0)
    cl = o.closures(0)[0]
    ch = R.Chains(GEOM, xy, ti[:, 0], ti[:, 1])
    ch.check_lookahead()
    last = R.replay(GEOM, xy, ti, cl, min_between, "last")
    ahead = R.replay(GEOM, xy, ti, cl, min_between, "ahead")
    assert (last[0] == cl[:, 0]).all() and (ahead[0] == cl[:, 0]).all()   # the restatement finds the oracle's matches
    return ch, cl, last, ahead


@pytest.mark.parametrize("name", R.SCENES)
def test_scene_reaches_its_case(name):
    ch, cl, last, ahead = _scene(name)
    n_lay = R.scene_stream(name)[1]
    asked = cl[:, 1] >= n_lay                                        # the closures of the asking bots
    assert asked.any()
    (m_l, r_l, lean_l, first_l), (m_a, r_a, lean_a, first_a) = last, ahead
    assert (r_a <= r_l).all()
    what = "fewer" if (r_a[asked] > 1).sum() < (r_l[asked] > 1).sum() else "same"   # (decisions that walk)
    assert what == R.EXPECT[name]
    # a closure that only the walk finds: settled by the lean owner, not by its first rows
    decided = asked & lean_a & (first_a != m_a)
    if name in ("deciding", "third", "batch", "two"):
        assert decided.any() and (m_a[decided] < first_a[decided]).all()
        assert r_a[decided].max() == {"deciding": 2, "third": 3, "batch": 4, "two": 2}[name]
    if name == "two":
        assert decided.sum() >= 2                                    # (one from Q, one from R)
    if name == "avoid":
        assert (r_l[asked] == 2).any() and (r_a[asked] == 1).all() and (first_a[asked] == m_a[asked]).all()
    a_len = ch.length(*R.A, 5)
    if name.startswith("len"):
        assert a_len == int(name[3:])
        assert r_a[asked].max() == {"len7": 1, "len8": 2, "len14": 2, "len15": 2}[name]
        assert r_l[asked].max() == {"len7": 1, "len8": 2, "len14": 2, "len15": 3}[name]
    new = R.new_nodes_per_batch(ch)
    if name == "batch":
        assert a_len == 22 and new[0][GEOM.key(5, *GEOM.cell(*R.A))] == 3   # three pool nodes for one bucket in one batch
    if name == "two":
        assert sum(1 for v in new[0].values() if v >= 1) >= 2        # two buckets with new pool nodes in one batch


@pytest.mark.parametrize("min_between", [0, 1])
def test_scenes_at_short_cool_downs(min_between):
    """MIN_POSES_BETWEEN 0 and 1: every packet is a decision and the bots drift towards what they match; the restatement still
    finds the oracle's closures under both rules (asserted in _scene), and the deciding scenes still hold a closure found by a walk."""
    for name in ("deciding", "third"):
        _, cl, last, ahead = _scene(name, min_between)
        assert (ahead[2] & (ahead[3] != ahead[0])).any()


def test_cycled_session():
    """The first 2^16 packets of the cycled session in the benchmark's world (4096 cells of 0.05 from -102.4): the
    restatement's closures are the oracle's under both rules, and fewer decisions walk a bucket with the look-ahead."""
    grid = (4096, 0.05, -102.4, -102.4)
    geom = R.Geometry(*grid, R.RADIUS)
    replay = importlib.import_module(load_pkg().__name__ + ".replay")
    stream = replay.cycle_stream(replay.telemetry_csv_to_packets()[0], 1 << 16)
    o = orc.OracleMapper(*grid, 0.0, max_agent=2)
    o.set_closure_params(R.RADIUS, 30, 0.5)
    o.feed_stream(stream)
    xy, ti = o.landmarks(0)
    cl = o.closures(0)[0]
    assert len(cl) > 1000
    last = R.replay(geom, xy, ti, cl, 30, "last")
    ahead = R.replay(geom, xy, ti, cl, 30, "ahead")
    assert (last[0] == cl[:, 0]).all() and (ahead[0] == cl[:, 0]).all()
    w_last, w_ahead = int((last[1] > 1).sum()), int((ahead[1] > 1).sum())
    print(f"closures {len(cl)}: walking decisions {w_last} -> {w_ahead}, rounds beyond the first {int((last[1] - 1).sum())} -> {int((ahead[1] - 1).sum())}")
    assert (ahead[1] <= last[1]).all() and 0 < w_ahead < w_last
