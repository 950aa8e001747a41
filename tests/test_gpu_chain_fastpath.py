"""The lean owner of the free-running chain (csrc/slam.hip, qs_slam_chain_free_kernel): 32-bit node indices and a decision
settled by the first rows of its nine buckets (or by walking on from them), everything else handed to the general query.  Streams that stay on the fast
path, that leave it at every decision of one bot (a neighbour bucket whose full first node is older than the match), that sit
on the node boundaries (a first node exactly full, the first pool node), that find nothing in round one, that cross from the
lean owner to the general one between launches; 1 to 13 bots.  Every case against oracle.OracleMapper fed the same stream --
closure pairs, landmark nodes and types and the grid exact, corrections, landmark poses and drifts to 1e-9 -- and with the lean
owner on offer and switched off: the two runs' closures, landmarks and drifts byte for byte the same."""
import functools
import importlib

import numpy as np
import pytest
import torch  # before the HIP library (see test_gpu_parity.py)

from conftest import load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-9                      # the tolerance of test_gpu_chain_handover._equal
GRID = (512, 0.05, -12.8, -12.8)
P, Q = (0.05, 0.05), (0.75, 0.35)   # tests/k4_adversarial.py: neighbouring buckets of 0.6 m, 0.76 m apart (out of the radius)
FAR = (2.75, 0.35)                  # 2 m from Q, 2.7 m from P
PARK_MB = 5


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _session():
    replay = importlib.import_module(load_pkg().__name__ + ".replay")
    return replay, replay.telemetry_csv_to_packets()[0]


def _parked(legs):
    """Packets of bots standing still: legs = ((agent, (x, y), packets), ...), every packet a landmark of type 5."""
    agent = np.concatenate([np.full(n, a) for a, _, n in legs])
    x = np.concatenate([np.full(n, p[0]) for _, p, n in legs])
    y = np.concatenate([np.full(n, p[1]) for _, p, n in legs])
    n = len(agent)
    z = np.zeros(n, dtype=int)
    return load_pkg().pack_packets(agent, x, y, np.zeros(n), z, z, np.zeros((n, 4)), np.full(n, 5))


@functools.lru_cache(maxsize=None)
def _stream(kind, n=0, nb=0):
    replay, session = _session()
    if kind == "cycle":
        s = replay.cycle_stream(session, n)
    elif kind == "bots":
        s = replay.multi_bot_stream(session, nb, n, pitch=1.0, origin=(-8.0, -8.0), tiles_per_row=5)
    elif kind == "solo":                                             # bot 1's packets of the cycled session
        c = replay.cycle_stream(session, 4 * n)
        s = np.ascontiguousarray(c[c[:, 4] == 1][:n])
        assert len(s) == n
    elif kind == "pile":                                             # bot 1 piles n landmarks at P, then bot 2 parks at Q
        s = _parked(((1, P, n), (2, Q, 200)))
    else:                                                            # ... and goes 2 m away for 50 packets in between
        s = _parked(((1, P, 30), (2, Q, 60), (2, FAR, 50), (2, Q, 60)))
    s = np.ascontiguousarray(s)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _oracle(key, min_between, nb=2):
    """The oracle's results for a stream, computed once and shared (read only)."""
    o = orc.OracleMapper(*GRID, 0.0, max_agent=nb)
    o.set_closure_params(0.6, min_between, 0.5)
    o.feed_stream(_stream(*key))
    return o


def _equal(m, o, nb):
    idx, cc = m.closures(0); oi, oc = o.closures(0)
    assert idx.shape == oi.shape and (idx == oi).all()
    assert len(oi) == 0 or np.abs(cc - oc).max() < TOL
    xy, ti = m.landmarks(0); oxy, oti = o.landmarks(0)
    assert ti.shape == oti.shape and (ti == oti).all()
    assert len(oti) == 0 or np.abs(xy - oxy).max() < TOL
    for b in range(1, nb + 1):
        assert np.allclose(m.drift(b), o.drift(b), rtol=0, atol=TOL)
    assert (m.grid_i8() == o.grid).all()
    assert m.counters()["slam_rounds"] < 1 << 40                    # no wait ran out of patience


def _bytes(m, nb):
    idx, cc = m.closures(0); xy, ti = m.landmarks(0)
    return b"".join(a.tobytes() for a in (idx, cc, xy, ti) + tuple(m.drift(b) for b in range(1, nb + 1)))


def _run(pkg, key, min_between, nb=2, form="free", cuts=(), limit=0):
    """The stream through the lean owner and through the general one: both equal to the oracle and to each other byte for byte.
    Returns what the lean run left: (chain_lean() after every launch, its counters)."""
    o = _oracle(key, min_between, nb)
    stream = _stream(*key)
    out = {}
    for mode in ("auto", "off"):
        with pkg.QuasarMapper(*GRID, max_agent=nb, closure_radius=0.6, min_poses_between=min_between, closure_correction=0.5) as m:
            m.set_chain_form(form)
            m.set_chain_lean(mode, limit)
            lean, lo = [], 0
            for hi in tuple(cuts) + (len(stream),):
                m.ingest_array(stream[lo:hi]); lo = hi
                lean.append(m.chain_lean())
            assert m.chain_form() == form
            _equal(m, o, nb)
            out[mode] = (lean, m.counters(), _bytes(m, nb))
    assert out["auto"][2] == out["off"][2]
    assert not any(out["off"][0]) and out["off"][1]["slam_node_iters"] == 0
    return out["auto"][0], out["auto"][1]


def _decisions(o, stream, min_between):
    """What the owners decide about, from the oracle's closures (every packet of these streams is a node and a landmark):
    an agent's event needs a decision when it is min_between nodes past the agent's last closure (the cool-down starts at
    -min_between).  Returns {agent: (decisions, closures)}."""
    closing = set(o.closures(0)[0][:, 1].tolist())
    out = {}
    for a in np.unique(stream[:, 4]):
        last, dec, cl = -min_between, 0, 0
        for i in np.nonzero(stream[:, 4] == a)[0].tolist():
            if i - last >= min_between:
                dec += 1
                if i in closing:
                    cl += 1; last = i
        out[int(a)] = (dec, cl)
    return out


@pytest.mark.parametrize("form", ["free", "free_posting"])
@pytest.mark.parametrize("min_between", [0, 1, 5, 30])
def test_cycled_session(pkg, min_between, form):
    """The two-bot session, whole and cut at 1, 330 and 5000 (the first nodes of a session: a negative limit, a frontier that
    starts at -1, a cool-down that starts at -min_between)."""
    key = ("cycle", 12000)
    assert len(_oracle(key, min_between).closures(0)[0]) > 100
    for cuts in ((), (1, 330, 5000)):
        lean, cnt = _run(pkg, key, min_between, form=form, cuts=cuts)
        # (the instantiations that post poses have no lean owner: the switch must change nothing there either)
        assert all(lean) if form == "free" else not any(lean) and cnt["slam_node_iters"] == 0


def test_every_decision_of_bot_2_falls_through(pkg):
    """Bot 1 piles 30 landmarks at P; bot 2 then stands at Q, in the next bucket.  Every match of bot 2 is its own first landmark
    at Q, newer than all of P's: P's first node is full, within the limit, has a successor and ends below the match -- the
    general query has to walk P's chain, at every closure of bot 2.  Bot 1's own closures need no second round."""
    key = ("pile", 30)
    o = _oracle(key, PARK_MB)
    dec = _decisions(o, _stream(*key), PARK_MB)
    assert dec[2][1] > 20
    lean, cnt = _run(pkg, key, PARK_MB)
    assert all(lean)
    assert cnt["closures"] == dec[1][1] + dec[2][1]
    # every decision without a match and every closure of bot 2, at the least; not bot 1's closures once the committer has its
    # first landmark in the index
    assert (dec[1][0] - dec[1][1]) + dec[2][0] <= cnt["slam_node_iters"] < dec[1][0] + dec[2][0]


@pytest.mark.parametrize("pile", [7, 8])
def test_pile_at_the_node_boundary(pkg, pile):
    """7 landmarks at P: its first node exactly full and no successor -- nothing to walk, bot 2's closures stay on the fast
    path.  8: the first pool node -- they all leave it."""
    key = ("pile", pile)
    o = _oracle(key, PARK_MB)
    dec = _decisions(o, _stream(*key), PARK_MB)
    assert dec[2][1] > 20
    lean, cnt = _run(pkg, key, PARK_MB)
    assert all(lean)
    nomatch = (dec[1][0] - dec[1][1]) + (dec[2][0] - dec[2][1])
    if pile == 8:
        assert nomatch + dec[2][1] <= cnt["slam_node_iters"] <= dec[1][0] + dec[2][0]
    else:
        # (a closure decided before the committer has the match in the index goes to the general query, which waits for it:
        # bot 2's first may, the later ones come a cool-down apart and find a committer with nothing else to do long done)
        assert nomatch <= cnt["slam_node_iters"] < nomatch + dec[2][1] // 2


def test_no_match_in_round_one(pkg):
    """Bot 2 leaves Q for a place 2 m from anything, reports 50 landmarks there and comes back: decisions whose nine buckets
    are empty, or hold nothing within the limit, then closures against its own landmarks there, then against the old ones at Q."""
    key = ("away",)
    o = _oracle(key, PARK_MB)
    dec = _decisions(o, _stream(*key), PARK_MB)
    assert dec[2][1] > 20 and dec[2][0] > dec[2][1]
    lean, cnt = _run(pkg, key, PARK_MB)
    assert all(lean)
    assert cnt["slam_node_iters"] >= (dec[1][0] - dec[1][1]) + (dec[2][0] - dec[2][1])


def test_predicate_crossing(pkg):
    """The lean owner stops at 5000 nodes; launches of 3000 packets: the first runs it, the others the general owner, each from
    the state the one before left."""
    key = ("cycle", 12000)
    lean, _ = _run(pkg, key, 5, cuts=(3000, 6000, 9000), limit=5000)
    assert lean == [True, False, False, False]


@pytest.mark.parametrize("nb", [1, 5, 6, 13])
def test_agent_counts(pkg, nb):
    """One graph of 1, 5 (the last of the 8-wave instantiation), 6 (the first of the 16-wave one) and 13 bots."""
    key = ("solo", 8000) if nb == 1 else ("bots", 8000, nb)
    assert len(_oracle(key, 5, nb).closures(0)[0]) > 100
    lean, _ = _run(pkg, key, 5, nb, cuts=(3000, 3001))
    assert all(lean)
