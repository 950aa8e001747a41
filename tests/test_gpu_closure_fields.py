"""The loop-closure search of csrc/slam.hip (and its slam_chain_*.inc owners) on landmark fields built to drive its geometry:
the distance test within an ulp of the radius, poses on cell edges, below the origin and far outside the world, cells that
share a table entry.  The fields and the reference -- a plain list scan that knows nothing of cells or hashes -- are
tests/closure_rules.py's; tests/test_closure_rules_cpu.py proves from them that every scene reaches its case and that a scan
with `<=`, with a threshold of R*R, without the type test, with an index blind to shared entries or to everything past a
chain's first rows closes elsewhere on the scenes named for it.

Every scene runs whole in one call and cut between laying and asking (the askers then read the index an earlier launch wrote);
the smallest ring also a call per event.  Compared with the scan: closure pairs and the landmark log's nodes and types exact;
corrections, landmark poses and drifts to 1e-9; no wait may have run out of patience (bit 40 of slam_rounds).

Raw route (qs_slam_add_poses, doubles as given; every scene): the window kernel, the free-running one -- lean owner on offer
with the look-ahead on and off, lean owner off -- and the posting one, for 2 bots (the 8-wave instantiation) and 6 (the 16-wave
one); 20 bots in one graph (the dealt kernels) free-running and windowed.  The raw route never has a plan or scouts, and its
free-running kernel never runs the lean owner (that one needs drifted poses): the lean owner's own comparisons are reached on
the packet route.
Packet route (ingest_array of packets with zero ranges, pose = value + drift; the scenes an f32 carries): free-running with the
plan on (and the scouts, for 2 bots) and off, with the look-ahead off, and the window kernel; 2 and 6 bots.  chain_lean() must
hold after every free-running launch, chain_plan() where a plan was asked for.

That a scene went the way it claims is asserted from the counters: slam_misc_iters moves in the launch of dense_ring's askers
(the DENSE variant's scan of the log) and in the askers' launch of every scene with a side-list landmark; slam_node_iters moves
in the lean owner's launches of far_collision (first rows filled by the far cell: handed on).  

The distance test is written out thirteen times in csrc/slam.hip and the slam_chain_*.inc owners.  While this file was written
each of them was given `<=` for `<`, one to a build: every one failed tests here -- the lean owner's first rows ring_f32 and
ring_f32_young on packets, its walk ring_f32_walk alone, the rows a scout staged ring_f32_young alone, the two halves of the
window kernel's round over the log dense_ring and dense_ring-64, the side-list scans the "t7" rings, the rest the rings at large.
A scene dropped from here may leave one of them untested.

Where one launch both lays and
asks, a free-running owner may take a landmark the committer has not got to from the pending poses instead of the side list,
as the committer's timing has it: there the side-list count is asserted for the window kernel only, whose ring of three
windows the scenes' 64 fillers outlast."""
import numpy as np
import pytest
import torch  # before the HIP library (see test_gpu_parity.py)

import closure_rules as C
from conftest import load_pkg

pytestmark = pytest.mark.gpu

TOL = 1e-9                      # the tolerance of test_gpu_chain_handover._equal
# (form, lean owner, look-ahead)
RAW_ROUTES = (("window", "auto", True), ("free", "auto", True), ("free", "auto", False), ("free", "off", True),
              ("free_posting", "auto", True))
RAW_RUNS = tuple((nb,) + r for nb in (2, 6) for r in RAW_ROUTES) + ((20, "free", "auto", True), (20, "window", "auto", True))
# (form, plan, look-ahead)
PACKET_ROUTES = (("free", True, True), ("free", False, True), ("free", False, False), ("window", False, True))
PACKET_RUNS = tuple((nb,) + r for nb in (2, 6) for r in PACKET_ROUTES)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


_PACKED = {}


def _packets(sc):
    """The scene as packets with zero ranges, packed once and shared (read only)."""
    key = (sc.name, sc.nb)
    if key not in _PACKED:
        n = len(sc.x)
        z = np.zeros(n, dtype=int)
        s = np.ascontiguousarray(load_pkg().pack_packets(sc.agent.astype(int), sc.x, sc.y, np.zeros(n), z, z, np.zeros((n, 4)),
                                                         sc.type.astype(int)))
        s.setflags(write=False)
        _PACKED[key] = s
    return _PACKED[key]


def _equal(m, ref, bots, graph=0):
    idx, cc = m.closures(graph)
    assert idx.shape == ref["pairs"].shape and (idx == ref["pairs"]).all(), (idx.tolist(), ref["pairs"].tolist())
    assert len(idx) == 0 or np.abs(cc - ref["corr"]).max() < TOL
    xy, ti = m.landmarks(graph)
    assert ti.shape == ref["lm_ti"].shape and (ti == ref["lm_ti"]).all()
    assert len(ti) == 0 or np.abs(xy - ref["lm_xy"]).max() < TOL
    assert m.slam_sizes(graph) == (ref["n_nodes"], len(ref["lm_ti"]), len(ref["pairs"]))
    for b in bots:
        assert np.allclose(m.drift(b), ref["drift"].get(b, (0.0, 0.0)), rtol=0, atol=TOL)
    assert m.counters()["slam_rounds"] < 1 << 40                    # bit 40: a wait ran out of patience


def _mapper(pkg, sc, nb, form, lean="auto", ahead=True, bpg=0, **params):
    p = dict(sc.params, **params)
    m = pkg.QuasarMapper(*sc.world, max_agent=nb, bots_per_graph=bpg, closure_radius=p["radius"],
                         min_poses_between=p["min_between"], closure_correction=p["correction"])
    m.set_chain_form(form)
    m.set_chain_lean(lean)
    m.set_chain_lookahead(ahead)
    return m


def _raw(pkg, sc, nb, form, lean, ahead, cuts):
    """The scene through qs_slam_add_poses.  Returns the counters before the last call and after it."""
    ref = sc.ref
    with _mapper(pkg, sc, nb, form, lean, ahead) as m:
        closed, corr, lo, before = [], [], 0, None
        for hi in tuple(cuts) + (len(sc.x),):
            before = m.counters()
            c, k = m.slam_add_poses(sc.x[lo:hi], sc.y[lo:hi], sc.agent[lo:hi], sc.type[lo:hi])
            closed.append(c); corr.append(k); lo = hi
            assert m.chain_form() == form
        closed, corr = np.concatenate(closed), np.concatenate(corr)
        assert np.nonzero(closed)[0].tolist() == ref["pairs"][:, 1].tolist()      # (one graph: a pose's node is its position)
        assert len(ref["pairs"]) == 0 or np.abs(corr[closed == 1] - ref["corr"]).max() < TOL
        _equal(m, ref, range(1, nb + 1))
        return before, m.counters()


def _packet(pkg, sc, nb, form, plan, ahead, cuts):
    ref, stream = sc.ref, _packets(sc)
    free = form == "free"
    with _mapper(pkg, sc, nb, form, "auto", ahead) as m:
        m.set_chain_plan(plan)
        m.set_chain_scout(plan)
        lo, before = 0, None
        for hi in tuple(cuts) + (len(stream),):
            before = m.counters()
            m.ingest_array(stream[lo:hi]); lo = hi
            assert m.chain_form() == form
            assert m.chain_lean() == free                                # the lean owner ran, in every free-running launch
            assert m.chain_plan() == (free and plan)
        if free and plan and nb == 2:
            assert sum(m.chain_scout()) > 0                              # decisions of owners that had a scout
        _equal(m, ref, range(1, nb + 1))
        return before, m.counters()


def _moved(counters, what):
    return counters[1][what] - counters[0][what]


@pytest.mark.parametrize("name", C.SCENES)
def test_poses_as_given(pkg, name):
    for nb, form, lean, ahead in RAW_RUNS:
        sc = C.scene(name, nb, True)
        for cuts in ((), sc.cuts):
            cnt = _raw(pkg, sc, nb, form, lean, ahead, cuts)
            if "side" in sc.tags and (cuts or form == "window"):
                assert _moved(cnt, "slam_misc_iters") > 0, (nb, form, lean, ahead, cuts)      # the side list was scanned
            if "dense" in sc.tags and cuts:
                # the pile was flagged by the launch that laid it: the askers' launch runs the DENSE variant, and those
                # towards the pile leave the chain for the log
                assert _moved(cnt, "slam_misc_iters") > 0, (nb, form, lean)


@pytest.mark.parametrize("name", C.PACKET)
def test_packets(pkg, name):
    for nb, form, plan, ahead in PACKET_RUNS:
        sc = C.scene(name, nb, False)
        for cuts in ((), sc.cuts):
            cnt = _packet(pkg, sc, nb, form, plan, ahead, cuts)
            if "side" in sc.tags and (cuts or form == "window"):
                assert _moved(cnt, "slam_misc_iters") > 0, (nb, form, plan, ahead, cuts)
            if "far" in sc.tags and form == "free":
                # the asker at C2 finds C1's rows in its first round and nothing within the radius: not the lean owner's to settle
                assert cnt[1]["slam_node_iters"] > 0, (nb, plan, ahead, cuts)
                if cuts:
                    assert _moved(cnt, "slam_node_iters") > 0


@pytest.mark.parametrize("form", ["window", "free"])
def test_smallest_ring_a_call_per_event(pkg, form):
    sc = C.scene(C.SMALLEST_RING, 2, True)
    _raw(pkg, sc, 2, form, "auto", True, tuple(range(1, len(sc.x))))


@pytest.mark.parametrize("form", ["window", "free"])
def test_a_graph_per_bot(pkg, form):
    """max_agent 3, a graph each: the field is laid by bot 1 and asked by bots 2 and 3, twice over.  Every bot closes on its own
    first pass; nobody closes on another graph's landmarks."""
    x, y, agent, lm, params = C.graphs_case()
    per = C.scan_graphs(x, y, agent, lm, 1, raw=True, **params)
    sc = C.scene("types_share_cells", 3, True)
    for cuts in ((), (len(x) // 2,)):
        with _mapper(pkg, sc, 3, form, bpg=1, **params) as m:
            lo = 0
            for hi in cuts + (len(x),):
                m.slam_add_poses(x[lo:hi], y[lo:hi], agent[lo:hi], lm[lo:hi]); lo = hi
            for g in range(3):
                assert len(per[g]["pairs"]) >= 3
                _equal(m, per[g], (g + 1,), graph=g)
