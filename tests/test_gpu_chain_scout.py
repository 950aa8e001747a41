"""The scout waves of the free-running chain (csrc/slam_chain_scout.inc, slam_chain_scout_owner.inc; qs_set_chain_scout): every
scene runs with the scouts on, with them off (the plan owner alone) and with the lean owner off, and the three must agree byte
for byte in closures, landmarks, drifts and sizes, and with oracle.OracleMapper (index pairs and types exact, doubles to 1e-9);
no wait may run out of patience.  chain_scout() gives the owners' decisions settled from a stage and made from their own loads:
zero in the runs without scouts and in graphs of more than two agents; on a last launch whose every match lay in the index at
its start it must equal tests/chain_scout_rules.staged.  Where one launch both lays and asks, the split depends on how far the
committer has got and is printed only."""
import functools

import numpy as np
import pytest
import torch  # before the HIP library (see test_gpu_parity.py)

import chain_lookahead_rules as L
import chain_plan_rules as P
import chain_scout_rules as S
from conftest import load_pkg
from oracle import oracle as orc
from test_gpu_chain_plan import FAR, GRID, _bytes, _equal, _pack, _stream

pytestmark = pytest.mark.gpu

CELL = 0.6 * (1.0 + 1e-9)
CORNER = (GRID[2] + 10 * CELL, GRID[3] + 12 * CELL)
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _scene(kind):
    if kind == "hole":        # lap 1 lays 120 places, lap 2 visits them again -- but place 60, which is somewhere new: no closure there
        k = np.arange(120)
        x, y = -11.0 + 1.2 * (k % 12), -11.0 + 1.2 * (k // 12)
        x2, y2 = x.copy(), y.copy()
        x2[60], y2[60] = 9.0, 9.0
        s = _pack(np.tile(1 + k % 2, 2), np.concatenate([x, x2]), np.concatenate([y, y2]), np.full(240, 5))
    elif kind == "borders":   # eight graphs of two bots: the first bot of graph g leaves a landmark 0.15 beyond a corner of the bucket grid
        #                       (an edge for the straight directions) in direction g, then stands 0.25 before it: every closure
        #                       on that landmark halves the distance, and the second one carries the pose across
        agent, x, y = [], [], []
        for g, (dx, dy) in enumerate(DIRS):
            ex, ey = (0.0 if dx else 0.3), (0.0 if dy else 0.3)         # (straight directions: mid-way along the edge)
            agent.append(2 * g + 1); x.append(CORNER[0] + ex + 0.15 * dx); y.append(CORNER[1] + ey + 0.15 * dy)
            agent.append(2 * g + 2); x.append(FAR[0]); y.append(FAR[1])
        for _ in range(8):
            for g, (dx, dy) in enumerate(DIRS):
                ex, ey = (0.0 if dx else 0.3), (0.0 if dy else 0.3)
                agent.append(2 * g + 1); x.append(CORNER[0] + ex - 0.25 * dx); y.append(CORNER[1] + ey - 0.25 * dy)
                agent.append(2 * g + 2); x.append(FAR[0]); y.append(FAR[1])
        s = _pack(np.array(agent), np.array(x), np.array(y), np.full(len(agent), 5))
    elif kind == "offlap":    # lap 2 stands up to 0.55 beside lap 1's places, a different way at every place: corrections of every size
        k = np.arange(300)
        x, y = -11.0 + 1.2 * (k % 18), -11.0 + 1.2 * (k // 18)
        ox, oy = 0.55 * ((k % 3) - 1) * ((k % 7) / 6.0), 0.3 * ((k % 5) - 2) / 2.0
        s = _pack(np.tile(1 + k % 2, 2), np.concatenate([x, x + ox]), np.concatenate([y, y + oy]), np.full(600, 5))
    else:
        raise KeyError(kind)
    s = np.ascontiguousarray(s)
    s.setflags(write=False)
    return s


def _get(key):
    return _scene(key[0]) if key[0] in ("hole", "borders", "offlap") else _stream(*key)


@functools.lru_cache(maxsize=None)
def _oracle(key, min_between, nb, bpg=0, correction=0.5, upto=None):
    o = orc.OracleMapper(*GRID, 0.0, max_agent=nb, bots_per_graph=bpg)
    o.set_closure_params(0.6, min_between, correction)
    o.feed_stream(_get(key)[:upto])
    return o


@functools.lru_cache(maxsize=None)
def _expected(key, min_between, nb, bpg, correction, lo):
    """chain_scout_rules.staged summed over the bots, for the last launch (packets from lo on): the index as of that launch's
    start, the plans of chain_plan_rules (every packet of these scenes is a node and an event), poses and closures from the oracle."""
    per = bpg if bpg else nb
    geom = L.Geometry(*GRID, 0.6)
    before, after = _oracle(key, min_between, nb, bpg, correction, lo), _oracle(key, min_between, nb, bpg, correction)
    agents = np.asarray(_get(key)[:, 4]).astype(np.int64)                   # (the packet's agent byte)
    tot = np.zeros(3, dtype=np.int64)
    for g in range((nb + per - 1) // per):
        mine = np.nonzero((agents - 1) // per == g)[0]                     # the graph's packets: node k is packet mine[k]
        node = np.nonzero(mine >= lo)[0]
        local = (agents[mine[node]] - 1) % per
        last = np.full(per, -min_between, dtype=np.int64)
        for c in before.closures(g)[0][:, 1]:
            last[(agents[mine[c]] - 1) % per] = c
        plans = P.plan(node, local, per, min_between, last)
        bxy, bti = before.landmarks(g)
        chains = L.Chains(geom, bxy, bti[:, 0], bti[:, 1])
        xy, ti = after.landmarks(g)
        idx, corr = after.closures(g)
        xy_of = {int(n): (float(a), float(b)) for n, (a, b) in zip(ti[:, 1], xy)}
        type_of = {int(n): int(t) for n, t in zip(ti[:, 1], ti[:, 0])}
        corr_of = {int(n): (float(c[0]), float(c[1])) for (_, n), c in zip(idx, corr)}
        assert all(int(lm) < before.n_nodes(g) for (lm, n) in idx if int(n) >= before.n_nodes(g))   # every match lay in the index
        assert len(ti) == len(mine)
        for p in plans:
            tot += S.staged(geom, chains, p, xy_of, type_of, corr_of, min_between)
    return tuple(int(v) for v in tot)


def _run(pkg, key, min_between, nb=2, bpg=0, cuts=(), correction=0.5, scouts=True, settled=False):
    """Returns the scout run's chain_scout() per launch -- and, with settled, the restatement's (staged, fallback, window misses)
    for the last launch."""
    o, stream = _oracle(key, min_between, nb, bpg, correction), _get(key)
    n_graphs = 1 if bpg == 0 else (nb + bpg - 1) // bpg
    ends = tuple(cuts) + (len(stream),)
    out, counts, want = {}, [], None
    for run in ("scout", "plan", "general"):
        with pkg.QuasarMapper(*GRID, max_agent=nb, bots_per_graph=bpg, closure_radius=0.6, min_poses_between=min_between,
                              closure_correction=correction) as m:
            m.set_chain_form("free")
            m.set_chain_lean("off" if run == "general" else "auto")
            m.set_chain_scout(run == "scout")
            lo = 0
            for hi in ends:
                m.ingest_array(stream[lo:hi])
                c = m.chain_scout()
                if run == "scout":
                    counts.append(c)
                assert c == (0, 0) or (run == "scout" and scouts)
                lo = hi
            _equal(m, o, nb, n_graphs)
            if run == "scout" and settled:
                want = _expected(key, min_between, nb, bpg, correction, ends[-2] if cuts else 0)
            out[run] = _bytes(m, nb, n_graphs)
    assert out["scout"] == out["plan"] == out["general"]
    print(key, min_between, "chain_scout per launch:", counts, "restatement:", want)
    return counts, want


def test_a_lap_revisited(pkg):
    """Lap 1 lays 300 places, lap 2 -- a launch of its own -- closes at every one from its first rows: all but each bot's first
    decision are settled from a stage."""
    counts, want = _run(pkg, ("laps",), 5, cuts=(300,), settled=True)
    assert counts[-1][0] > 0 and counts[-1] == want[:2] and want[2] == 0


def test_parked_bots(pkg):
    counts, _ = _run(pkg, ("alternate", 1300), 1)
    assert counts[-1][0] > 0


def test_corrections_across_the_eight_borders(pkg):
    """Eight 2-agent graphs in one launch; in graph g the closures carry the pose over the edge or corner in direction g."""
    key, geom = ("borders",), L.Geometry(*GRID, 0.6)
    o = _oracle(key, 1, 16, 2)
    for g in range(8):
        xy, ti = o.landmarks(g)
        idx, corr = o.closures(g)
        mine = xy[np.abs(xy[:, 0] - FAR[0]) > 1.0]
        cells = [geom.cell(*p) for p in mine[1:]]
        assert len(set(cells)) == 2 and cells[0] != cells[-1]             # the pose starts on one side and ends on the other
        crossing = [p for p, q in zip(mine[1:], mine[2:]) if geom.cell(*p) != geom.cell(*q)][0]
        assert np.abs(crossing - (CORNER[0] + (0.0 if DIRS[g][0] else 0.3), CORNER[1] + (0.0 if DIRS[g][1] else 0.3))).max() < 0.3
        assert (corr != 0).any(axis=1).sum() >= 6
    counts, want = _run(pkg, key, 1, nb=16, bpg=2, cuts=(16,), settled=True)
    assert counts[-1] == want[:2] and want[0] >= 8 * 5 and want[2] == 0


def test_no_closure_in_a_run_of_closures(pkg):
    """Place 60 of lap 2 is new: that decision finds nothing, the next candidate is not the one the stage is for (tag), and
    the owner is back on its stages two decisions later."""
    counts, want = _run(pkg, ("hole",), 5, cuts=(120,), settled=True)
    assert counts[-1] == want[:2] and want[0] > 20 and want[1] >= 3


def test_walks_and_side_lists(pkg):
    """A pile whose closures have to walk past full nodes, then side-list landmarks (types 6 and 7): both are the owner's own query."""
    counts, _ = _run(pkg, ("walk",), 5)
    assert counts[-1][1] > 0


@pytest.mark.parametrize("min_between", [0, 1, 5, 30, 31])
def test_cool_down_lengths(pkg, min_between):
    """Short cool-downs put a query's only match above the frontier the scout read: the stage finds nothing, the fallback must."""
    _run(pkg, ("cycle", 6000), min_between)


def test_cuts_inside_a_cool_down_and_before_a_closure(pkg):
    key = ("pile", 30)
    late = _oracle(key, 5, 2).closures(0)[0][:, 1]
    late = late[late >= 60]
    _run(pkg, key, 5, cuts=(int(late[3]) + 1, int(late[9]) + 2, int(late[15]) - 1))


def test_one_agent_and_three(pkg):
    counts, _ = _run(pkg, ("solo", 3000), 30, nb=1)
    assert counts[-1][0] > 0
    _run(pkg, ("sparse",), 5, nb=3, scouts=False)                          # three agents in the graph: no scouts


def test_a_correction_that_leaves_the_window(pkg):
    """CLOSURE_CORRECTION 1.5: the pose moves by up to 0.9 a closure, further than the window allows for; the owner's check sends
    those decisions to its own loads."""
    key = ("offlap",)
    counts, want = _run(pkg, key, 5, cuts=(300,), correction=1.5, settled=True)
    assert want[2] >= 1 and counts[-1] == want[:2]
