"""tests/chain_scout_rules.py on the package's 2-bot session, cycled to 2^16 packets, with the oracle's closures: for every decision
of either bot whose stage is for its candidate, the 3 x 3 buckets around the real pose lie inside the window the scout covers
from the pose it foresaw -- the real pose less the correction of the closure in between, which is under half a bucket edge per
axis (CLOSURE_CORRECTION 0.5 x a distance under CLOSURE_RADIUS 0.6, buckets of 0.6 (1 + 1e-9)) -- for the 4 x 4 window the
kernel uses and for the 5 x 5 one; a correction of 1.5 breaks the bound and the rule says so.  And the number of decisions a
complete index settles from a stage, which tests/test_gpu_chain_scout.py compares the device's count with on its own scenes."""
import functools
import importlib

import numpy as np

import chain_lookahead_rules as L
import chain_plan_rules as P
import chain_scout_rules as S
from conftest import load_pkg
from oracle import oracle as orc

GRID = (512, 0.05, -12.8, -12.8)
N = 1 << 16


@functools.lru_cache(maxsize=None)
def _session(correction, min_between=30):
    replay = importlib.import_module(load_pkg().__name__ + ".replay")
    stream = replay.cycle_stream(replay.telemetry_csv_to_packets()[0], N)
    o = orc.OracleMapper(*GRID, 0.0, max_agent=2)
    o.set_closure_params(0.6, min_between, correction)
    o.feed_stream(stream)
    assert o.n_nodes(0) == len(o.pose_agents)
    return o


def _agents_decisions(o, min_between=30):
    """Per bot of the one graph: (plan, decisions) for the whole stream as one launch."""
    xy, ti = o.landmarks(0)
    idx, corr = o.closures(0)
    node = ti[:, 1]
    agent = np.asarray(o.pose_agents)[node] - 1
    xy_of = {int(n): (float(x), float(y)) for n, (x, y) in zip(node, xy)}
    type_of = {int(n): int(t) for n, t in zip(node, ti[:, 0])}
    corr_of = {int(n): (float(c[0]), float(c[1])) for (_, n), c in zip(idx, corr)}
    plans = P.plan(node, agent, 2, min_between, np.full(2, -min_between, dtype=np.int64))
    return plans, [S.decisions(p, xy_of, corr_of) for p in plans], (xy, ti, xy_of, type_of, corr_of)


def test_the_window_covers_every_staged_decision():
    o = _session(0.5)
    geom = L.Geometry(*GRID, 0.6)
    _, dec, _ = _agents_decisions(o)
    tagged = [d for per in dec for d in per if d[4]]
    assert len(tagged) > 1000
    for w in (4, 5):
        assert all(S.covers(geom, f[0], f[1], q[0], q[1], w) for _, _, q, f, _ in tagged)
    # the shift itself: under half a bucket edge per axis, and not a formality -- some decisions do change cell
    shift = np.array([[q[0] - f[0], q[1] - f[1]] for _, _, q, f, _ in tagged])
    assert np.abs(shift).max() < 0.3
    assert any(geom.cell(*q) != geom.cell(*f) for _, _, q, f, _ in tagged)


def test_a_larger_correction_can_leave_the_window():
    o = _session(1.5)
    geom = L.Geometry(*GRID, 0.6)
    _, dec, _ = _agents_decisions(o)
    tagged = [d for per in dec for d in per if d[4]]
    assert not all(S.covers(geom, f[0], f[1], q[0], q[1], 4) for _, _, q, f, _ in tagged)


def test_decisions_settled_from_a_stage():
    """With the whole index in place a decision is settled from its stage exactly when the lean owner settles it from its first
    rows and the stage is for its candidate: the second condition fails at an agent's first decision and after a decision that
    did not close (unless the next own event is past the cool-down anyway)."""
    o = _session(0.5)
    geom = L.Geometry(*GRID, 0.6)
    plans, dec, (xy, ti, xy_of, type_of, corr_of) = _agents_decisions(o)
    chains = L.Chains(geom, xy, ti[:, 0], ti[:, 1])
    n_dec = n_st = n_lean = 0
    for p, per in zip(plans, dec):
        st, fall, miss = S.staged(geom, chains, p, xy_of, type_of, corr_of, 30)
        assert st + fall == len(per) and miss == 0
        lean = sum(1 for _, node, q, _, _ in per
                   if (lambda r: r[0] >= 0 and r[2] and r[1] == 1)(chains.query(q[0], q[1], type_of[node], node - 30, "ahead")))
        untagged_lean = sum(1 for _, node, q, _, tag in per if not tag
                            and (lambda r: r[0] >= 0 and r[2] and r[1] == 1)(chains.query(q[0], q[1], type_of[node], node - 30, "ahead")))
        assert st == lean - untagged_lean
        n_dec += len(per); n_st += st; n_lean += lean
    assert n_dec > 1000 and n_st > 0.5 * n_dec
