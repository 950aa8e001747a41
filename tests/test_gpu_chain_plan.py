"""The lean owner's walk of its agent's plan (csrc/slam.hip: qs_slam_plan_*_kernel, slam_chain_plan_owner.inc): every case runs
three times -- the plan on (default), the plan off (the lean owner streams the shared list in chunks), the lean owner off --
and compares closures (index pairs and corrections), landmarks, drifts and slam_sizes byte for byte between the three, and with
oracle.OracleMapper fed the same stream (index pairs, landmark nodes and types exact; corrections, poses and drifts to 1e-9).
chain_plan() must say what the case expects after every launch, and no wait may have run out of patience (bit 40 of
slam_rounds).  The shapes are the smallest at which the walk can go wrong: own events on both sides of the ring's wrap, an
owner that has to wait for the ring, agents with no event, one event, or nothing past their cool-down, every cool-down length
around the chunk size of the old loop, decisions that find nothing, ingests cut inside a cool-down, the lean limit crossed
between launches, 1 to 14 agents, four graphs at once, a landmark pile, side-list landmarks and buckets that need a walk."""
import functools
import importlib

import numpy as np
import pytest
import torch  # before the HIP library (see test_gpu_parity.py)

from conftest import load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-9
GRID = (512, 0.05, -12.8, -12.8)
P, Q, FAR = (0.05, 0.05), (0.75, 0.35), (2.75, 0.35)   # tests/k4_adversarial.py: P and Q in neighbouring buckets, out of each other's radius


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _pack(agent, x, y, lm):
    n = len(agent)
    z = np.zeros(n, dtype=int)
    s = np.ascontiguousarray(load_pkg().pack_packets(np.asarray(agent), np.asarray(x, dtype=float), np.asarray(y, dtype=float),
                                                     np.zeros(n), z, z, np.zeros((n, 4)), np.asarray(lm)))
    s.setflags(write=False)
    return s


def _legs(legs, lm=5):
    """legs = ((agent, (x, y), packets), ...): bots standing still, every packet a node and a landmark event of type lm."""
    agent = np.concatenate([np.full(n, a) for a, _, n in legs])
    x = np.concatenate([np.full(n, p[0]) for _, p, n in legs])
    y = np.concatenate([np.full(n, p[1]) for _, p, n in legs])
    return _pack(agent, x, y, np.full(len(agent), lm))


@functools.lru_cache(maxsize=None)
def _stream(kind, n=0, nb=0):
    replay = importlib.import_module(load_pkg().__name__ + ".replay")
    session = replay.telemetry_csv_to_packets()[0]
    if kind == "cycle":
        s = replay.cycle_stream(session, n)
    elif kind == "bots":
        s = replay.multi_bot_stream(session, nb, n, pitch=1.0, origin=(-8.0, -8.0), tiles_per_row=5)
    elif kind == "solo":
        c = replay.cycle_stream(session, 4 * n)
        s = c[c[:, 4] == 1][:n]
    elif kind == "alternate":        # bots 1 and 2 take turns, each parked at its own place: own events at every position of the ring
        k = np.arange(n)
        s = _pack(1 + k % 2, np.where(k % 2 == 0, P[0], FAR[0]), np.where(k % 2 == 0, P[1], FAR[1]), np.full(n, 5))
    elif kind == "late":             # bot 2's only events sit far down the list, behind a bot 1 that closes at every event
        s = _legs(((1, P, 1000), (2, FAR, 1), (1, P, 989), (2, FAR, 1), (1, P, 30)))
    elif kind == "sparse":           # three bots on offer: bot 3 has no event, bot 2 one
        s = _legs(((1, P, 100), (2, FAR, 1), (1, P, 100)))
    elif kind == "cooldown":         # bot 2 closes at node 64; what follows of it up to node 95 is inside its cool-down of 64
        k = np.arange(30)
        tail = _pack(1 + k % 2, np.where(k % 2 == 0, P[0], Q[0]), np.where(k % 2 == 0, P[1], Q[1]), np.full(30, 5))
        s = np.concatenate([_legs(((2, Q, 66),)), tail, _legs(((2, Q, 80), (1, P, 80)))])
    elif kind == "laps":             # lap 1: 2 x 150 places more than a radius apart, nothing to match; lap 2: the same places again
        k = np.arange(300)
        x, y = -11.0 + 1.2 * (k % 18), -11.0 + 1.2 * (k // 18)
        s = _pack(np.tile(1 + k % 2, 2), np.tile(x, 2), np.tile(y, 2), np.full(600, 5))
    elif kind == "pile":             # bot 1 piles n landmarks at P, then bot 2 parks at Q
        s = _legs(((1, P, n), (2, Q, 200)))
    else:                            # "walk": the pile of 30 that bot 2's closures have to walk past, and side-list landmarks (types 6, 7)
        a = _legs(((1, P, 30), (2, Q, 60)))
        b = _legs(((1, P, 20), (2, Q, 20)), lm=7)
        c = _legs(((2, Q, 60), (1, P, 40)), lm=6)
        s = np.concatenate([a, b, _legs(((2, Q, 40),)), c])
    s = np.ascontiguousarray(s)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _oracle(key, min_between, nb, bpg=0):
    """The oracle's results for a stream, computed once and shared (read only)."""
    o = orc.OracleMapper(*GRID, 0.0, max_agent=nb, bots_per_graph=bpg)
    o.set_closure_params(0.6, min_between, 0.5)
    o.feed_stream(_stream(*key))
    return o


def _equal(m, o, nb, n_graphs):
    for g in range(n_graphs):
        idx, cc = m.closures(g); oi, oc = o.closures(g)
        assert idx.shape == oi.shape and (idx == oi).all()
        assert len(oi) == 0 or np.abs(cc - oc).max() < TOL
        xy, ti = m.landmarks(g); oxy, oti = o.landmarks(g)
        assert m.slam_sizes(g)[1] == len(oti)
        assert ti.shape == oti.shape and (ti == oti).all()
        assert len(oti) == 0 or np.abs(xy - oxy).max() < TOL
    for b in range(1, nb + 1):
        assert np.allclose(m.drift(b), o.drift(b), rtol=0, atol=TOL)
    assert m.counters()["slam_rounds"] < 1 << 40                    # bit 40: a wait ran out of patience


def _bytes(m, nb, n_graphs):
    out = []
    for g in range(n_graphs):
        idx, cc = m.closures(g); xy, ti = m.landmarks(g)
        out += [idx.tobytes(), cc.tobytes(), xy.tobytes(), ti.tobytes(), repr(m.slam_sizes(g)).encode()]
    return b"".join(out + [m.drift(b).tobytes() for b in range(1, nb + 1)])


def _run(pkg, key, min_between, nb=2, cuts=(), limit=0, bpg=0, expect=True):
    """The stream with the plan on, the plan off and the lean owner off: each equal to the oracle, all three byte for byte the
    same.  expect: what chain_plan() must say after every launch of the first run (one value, or one per launch).
    Returns the first run's (chain_lean() per launch, counters)."""
    o = _oracle(key, min_between, nb, bpg)
    stream = _stream(*key)
    n_graphs = 1 if bpg == 0 else (nb + bpg - 1) // bpg
    ends = tuple(cuts) + (len(stream),)
    out = {}
    for run in ("plan", "chunks", "general"):
        with pkg.QuasarMapper(*GRID, max_agent=nb, bots_per_graph=bpg, closure_radius=0.6, min_poses_between=min_between,
                              closure_correction=0.5) as m:
            m.set_chain_form("free")
            m.set_chain_lean("off" if run == "general" else "auto", limit)
            m.set_chain_plan(run == "plan")
            plan, lean, lo = [], [], 0
            for hi in ends:
                m.ingest_array(stream[lo:hi]); lo = hi
                plan.append(m.chain_plan()); lean.append(m.chain_lean())
            assert m.chain_form() == "free"
            _equal(m, o, nb, n_graphs)
            out[run] = (plan, lean, m.counters(), _bytes(m, nb, n_graphs))
    assert out["plan"][3] == out["chunks"][3] == out["general"][3]
    assert out["plan"][0] == (list(expect) if isinstance(expect, (list, tuple)) else [expect] * len(ends))
    assert not any(out["chunks"][0]) and not any(out["general"][0])
    assert out["chunks"][1] == out["plan"][1] and not any(out["general"][1])
    return out["plan"][1], out["plan"][2]


def _closing(key, min_between, nb=2):
    return _oracle(key, min_between, nb).closures(0)[0][:, 1]


def test_ring_wrap(pkg):
    """Bots 1 and 2 take turns for 1300 events and close at every one: closures of both in the slots on either side of
    positions 63/64 and 511/512/513 (one ring length), and the ring goes round twice."""
    key = ("alternate", 1300)
    cl = set(_closing(key, 1).tolist())
    assert {63, 64, 511, 512, 513, 1023, 1024, 1025} <= cl
    _run(pkg, key, 1)


def test_ring_wait(pkg):
    """Bot 1 closes at every one of its 2000 events; bot 2's two events sit at positions 1000 and 1990: its owner is at its
    first candidate at once, further ahead of the committer than the ring allows, and has to wait -- twice."""
    key = ("late",)
    cl = _closing(key, 1)
    assert len(cl) > 1900 and 1990 in cl
    _run(pkg, key, 1)


def test_agents_without_events_and_with_one(pkg):
    key = ("sparse",)
    assert len(_closing(key, 5, 3)) > 20
    _run(pkg, key, 5, nb=3)
    _run(pkg, key, 5, nb=3, cuts=(100, 101))                        # ... and launches in which bot 1 or bot 2 has none either


def test_every_event_inside_the_cool_down(pkg):
    """MIN_POSES_BETWEEN 64: bot 2 closes at node 64; the second launch holds 15 events of it, all inside that cool-down (no
    candidate: the owner has nothing to do), the third takes it up again."""
    key = ("cooldown",)
    cl = _closing(key, 64)
    assert 64 in cl and not ((cl > 64) & (cl < 96)).any() and (cl >= 96).any()
    _run(pkg, key, 64, cuts=(66, 96))


@pytest.mark.parametrize("min_between", [0, 1, 30, 31, 64])
def test_cool_down_lengths(pkg, min_between):
    key = ("cycle", 6000)
    assert len(_closing(key, min_between)) > 50
    _run(pkg, key, min_between)


def test_nothing_to_match_then_everything(pkg):
    """Lap 1: every decision finds nothing, in the first rows and in the general query behind them, waits for the frontier
    and goes on to the agent's next event; lap 2: every place has its landmark."""
    key = ("laps",)
    cl = _closing(key, 5)
    assert len(cl) > 40 and cl.min() >= 300
    lean, cnt = _run(pkg, key, 5)
    assert all(lean) and cnt["slam_node_iters"] >= 300              # (lap 1's decisions all left the fast path)


@pytest.mark.parametrize("pieces", [2, 3])
def test_split_inside_a_cool_down(pkg, pieces):
    """The same stream in two and in three launches, cut one and two events behind a closure of bot 2: last_closure is carried
    across and the first candidate of the next launch is worked out from it."""
    key = ("pile", 30)
    cl = _closing(key, 5)
    late = cl[cl >= 60]
    assert len(late) > 20
    cuts = (int(late[3]) + 1,) if pieces == 2 else (int(late[3]) + 1, int(late[9]) + 2)
    _run(pkg, key, 5, cuts=cuts)


def test_lean_limit_crossed(pkg):
    """The lean owner stops at 5000 nodes; launches of 3000 packets: the first walks its plan, the others run the general owner."""
    lean, _ = _run(pkg, ("cycle", 12000), 5, cuts=(3000, 6000, 9000), limit=5000, expect=[True, False, False, False])
    assert lean == [True, False, False, False]


@pytest.mark.parametrize("nb", [1, 2, 5, 6, 13, 14])
def test_agent_counts(pkg, nb):
    """One graph of 1, 2, 5 (the 8-wave instantiation), 6 and 13 bots (the 16-wave one); 14: the kernel that deals events,
    which has no plan and whose results are what they were."""
    key = ("solo", 6000) if nb == 1 else ("cycle", 6000) if nb == 2 else ("bots", 6000, nb)
    assert len(_closing(key, 5, nb)) > 50
    lean, _ = _run(pkg, key, 5, nb, cuts=(3000, 3001), expect=nb <= 13)
    assert all(lean) == (nb <= 13)


def test_four_graphs_in_one_launch(pkg):
    key = ("bots", 8000, 8)
    o = _oracle(key, 5, 8, 2)
    assert all(len(o.closures(g)[0]) > 10 for g in range(4))
    _run(pkg, key, 5, nb=8, bpg=2)


def test_landmark_pile(pkg):
    """The pile of tests/k4_adversarial.py, as small as raises the pile flag (a bucket chain of more than 64 pool nodes), in a
    graph of six bots on offer: the launches after the flag run <true, 16, false>, whose lean owner keeps to the chunks."""
    key = ("pile", 7 * 66 + 3)
    n = len(_stream(*key))
    assert len(_closing(key, 5, 6)) > 20
    with pkg.QuasarMapper(*GRID, max_agent=6, closure_radius=0.6, min_poses_between=5, closure_correction=0.5) as m:
        m.ingest_array(_stream(*key))
        m.sync()
        assert m.counters()["slam_rounds"] < 1 << 40
    lean, _ = _run(pkg, key, 5, nb=6, cuts=(n - 150, n - 100, n - 50), expect=[True, False, False, False])
    assert all(lean)


def test_rows_that_need_a_walk(pkg):
    """Landmarks of types 6 and 7 (the side list is not empty: no decision is settled by its first rows from then on), and bot
    2's closures at Q, which have to walk P's chain past its full first node."""
    key = ("walk",)
    assert len(_closing(key, 5)) > 30
    lean, cnt = _run(pkg, key, 5)
    assert all(lean) and cnt["slam_node_iters"] > 20 and cnt["slam_misc_iters"] > 0
