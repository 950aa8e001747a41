"""The plan as the device builds it (csrc/slam.hip): qs_slam_plan_scatter_kernel works every record's skip out itself, from a
window of the event list staged with a halo of the next 256 events, and qs_slam_plan_count_kernel counts pl_first; only a
MIN_POSES_BETWEEN above 256 still runs the search kernel.  Every case checks two things after every launch and at the end:

  * chain_plan_read() of every bot equals tests/chain_plan_rules.plan of that launch's event list field for field (node, r,
    skip, first), with chain_plan() true -- last_closure at the launch's start taken from the oracle's closures;
  * closures, landmarks and drifts are byte-equal with the plan on and off, and equal to oracle.OracleMapper's.

The streams are bots standing still, every packet a node and a landmark event, so a launch's event list is its packets and a
bot closes a loop whenever its cool-down allows: the plan's skips are all walked.  The shapes are the smallest at which the
new code can go wrong: event counts around one and two blocks of 256, windows across a block's end, windows cut by the
graph's end with another graph's events (same local agent numbers) behind it, every cool-down around the halo, bots with no
event and with one, launches that begin inside a cool-down."""
import functools

import numpy as np
import pytest
import torch  # before the HIP library (see test_gpu_parity.py)

import chain_plan_rules as rules
from conftest import load_pkg
from oracle import oracle as orc
from test_gpu_chain_plan import FAR, GRID, P, Q, _bytes, _equal, _pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _agents(kind, n=0):
    """The bot of every packet (1-based), read only."""
    k = np.arange(n)
    if kind == "mixed":              # two bots in runs of 1 to 4: both have events on either side of every block's end
        a = 1 + ((k * 7) % 11 < 5)
    elif kind == "sparse":           # three bots on offer: bot 3 has no event, bot 2 one
        a = np.ones(300, dtype=np.int64); a[140] = 2
    elif kind == "one_block":        # bot 2's 20 events all lie in the second block of three, bot 1's span all of them
        a = np.ones(700, dtype=np.int64); a[300:360:3] = 2
    elif kind == "graphs":           # bots 1..8 in four graphs of 100, 300, 57 and 200 events: no graph ends at a block's end
        a = np.concatenate([np.repeat([1, 2, 1], [40, 30, 30]), 3 + (np.arange(300) * 5 % 7 < 3),
                            np.repeat([5, 6, 5, 6], [10, 20, 7, 20]), 7 + (np.arange(200) % 3 == 0)])
        a = a[np.random.default_rng(5).permutation(len(a))]          # arrival order mixes the graphs; each graph's own order is what counts
    else:                            # "pile": bot 1 leaves 30 landmarks, then bot 2 parks for 400
        a = np.repeat([1, 2], [30, 400])
    a = np.ascontiguousarray(a, dtype=np.int64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _stream(kind, n=0, bpg=0):
    a = _agents(kind, n)
    local = (a - 1) % bpg if bpg else a - 1
    place = np.array([P, FAR, Q])[np.minimum(local, 2)]             # the bots of a graph stand out of each other's radius
    return _pack(a, place[:, 0], place[:, 1], np.full(len(a), 5))


@functools.lru_cache(maxsize=None)
def _oracle(kind, n, min_between, nb, bpg):
    o = orc.OracleMapper(*GRID, 0.0, max_agent=nb, bots_per_graph=bpg)
    o.set_closure_params(0.6, min_between, 0.5)
    o.feed_stream(_stream(kind, n, bpg))
    return o


def _expected_plans(kind, n, min_between, nb, bpg, lo, hi):
    """chain_plan_rules.plan of every bot for the launch of packets [lo, hi): per graph the event list is the graph's packets of
    the launch, their nodes the packets' numbers in the graph, and last_closure what the oracle's closures before it leave."""
    a = _agents(kind, n)
    per = bpg if bpg else nb
    graph = (a - 1) // per
    o = _oracle(kind, n, min_between, nb, bpg)
    out = {}
    for g in range((nb + per - 1) // per):
        mine = np.nonzero(graph == g)[0]                            # the graph's packets: node k is packet mine[k]
        node = np.nonzero((mine >= lo) & (mine < hi))[0]
        local = (a[mine[node]] - 1) % per
        closing = o.closures(g)[0][:, 1]
        first_node = int(node[0]) if len(node) else int((mine < lo).sum())
        closing = closing[closing < first_node]
        last = np.full(per, -min_between, dtype=np.int64)
        for c in closing:
            last[(a[mine[c]] - 1) % per] = c
        for b, p in enumerate(rules.plan(node, local, per, min_between, last)):
            out[g * per + 1 + b] = p
    return out


def _run(pkg, kind, n, min_between, nb=2, bpg=0, cuts=()):
    stream, o = _stream(kind, n, bpg), _oracle(kind, n, min_between, nb, bpg)
    per = bpg if bpg else nb
    n_graphs = (nb + per - 1) // per
    ends = tuple(cuts) + (len(stream),)
    got, plans = {}, []
    for plan_on in (True, False):
        with pkg.QuasarMapper(*GRID, max_agent=nb, bots_per_graph=bpg, closure_radius=0.6, min_poses_between=min_between,
                              closure_correction=0.5) as m:
            m.set_chain_form("free")
            m.set_chain_plan(plan_on)
            lo = 0
            for hi in ends:
                m.ingest_array(stream[lo:hi])
                assert m.chain_plan() == plan_on
                if plan_on:
                    want = _expected_plans(kind, n, min_between, nb, bpg, lo, hi)
                    plans.append(want)
                    for bot in range(1, nb + 1):
                        have, w = m.chain_plan_read(bot), want[bot]
                        assert np.array_equal(have["node"], w["node"]), (bot, lo)
                        assert np.array_equal(have["r"], w["r"]), (bot, lo)
                        assert np.array_equal(have["skip"], w["skip"]), (bot, lo)
                        assert have["first"] == w["first"], (bot, lo)
                else:
                    with pytest.raises(pkg.QuasarError):
                        m.chain_plan_read(1)
                lo = hi
            for g in range(n_graphs):                               # every packet became a node: the event lists are what was assumed
                assert m.slam_sizes(g)[0] == int(((_agents(kind, n) - 1) // per == g).sum())
            _equal(m, o, nb, n_graphs)
            got[plan_on] = _bytes(m, nb, n_graphs)
    assert got[True] == got[False]
    return plans


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513])
def test_event_counts_around_the_block(pkg, n):
    """One graph of n events, cool-down 30: with 257 and 513 the last block holds one event; the windows of events 227..255
    start in the first block and end in the second (n > 256), those of the last 29 end with the list."""
    plans = _run(pkg, "mixed", n, 30)[0]
    assert sum(len(plans[b]["r"]) for b in (1, 2)) == n
    for b in (1, 2):
        p = plans[b]
        assert p["skip"][-1] == len(p["r"]) and (p["skip"] > np.arange(len(p["r"])) + 1).any()
        if n > 500:                                                 # a skip from the first block's last events well into the second
            j = np.nonzero(p["r"] < 256)[0][-1]
            assert p["r"][p["skip"][j]] >= 256 + 20 and p["skip"][j] > j + 1


@pytest.mark.parametrize("min_between", [0, 1, 30, 31, 64, 256, 257, 300])
def test_cool_down_lengths(pkg, min_between):
    """700 events of two bots.  Up to 256 the scatter counts the skip from its staged window (256: the whole halo), 257 and 300
    run the search kernel; 0 and 1 skip nothing."""
    plans = _run(pkg, "mixed", 700, min_between)[0]
    for b in (1, 2):
        p = plans[b]
        if min_between <= 1:
            assert (p["skip"] == np.arange(len(p["r"])) + 1).all()
        else:
            assert (p["skip"][:10] > np.arange(10) + min_between // 4).all() and p["skip"][0] < len(p["r"])
    assert len(_oracle("mixed", 700, min_between, 2, 0).closures(0)[0]) >= 2


def test_bots_without_events_and_with_one(pkg):
    plans = _run(pkg, "sparse", 0, 30, nb=3)[0]
    assert len(plans[3]["r"]) == 0 and len(plans[2]["r"]) == 1 and plans[2]["skip"][0] == 1
    _run(pkg, "sparse", 0, 30, nb=3, cuts=(140, 141))               # ... and launches in which bot 1 or bot 2 has none either


def test_one_bot_in_one_block_the_other_in_three(pkg):
    plans = _run(pkg, "one_block", 0, 30)[0]
    assert plans[2]["r"].min() >= 256 and plans[2]["r"].max() < 512 and plans[1]["r"].max() >= 512
    assert (plans[2]["skip"] > np.arange(20) + 1).any()


def test_four_graphs_in_one_launch(pkg):
    """Graphs of 100, 300, 57 and 200 events in one list of 657: every graph's last 29 events have a window that would run on
    into the next graph's events, whose nodes start again from 0 and whose bots have the same local numbers; the third graph
    lies inside one block with its neighbours' events on both sides."""
    plans = _run(pkg, "graphs", 0, 30, nb=8, bpg=2)[0]
    assert [len(plans[b]["r"]) + len(plans[b + 1]["r"]) for b in (1, 3, 5, 7)] == [100, 300, 57, 200]
    for b in range(1, 9):
        assert plans[b]["skip"][-1] == len(plans[b]["r"])
    o = _oracle("graphs", 0, 30, 8, 2)
    assert all(len(o.closures(g)[0]) >= 2 for g in range(4))


def _cuts_inside_cool_downs(pieces):
    """Cuts of the "pile" stream 5 and 12 events behind a closure of bot 2 (cool-down 30)."""
    cl = _oracle("pile", 0, 30, 2, 0).closures(0)[0][:, 1]
    late = cl[cl >= 60]
    assert len(late) >= 8
    return (int(late[2]) + 5,) if pieces == 2 else (int(late[2]) + 5, int(late[5]) + 12)


@pytest.mark.parametrize("pieces", [2, 3])
def test_launch_begins_inside_a_cool_down(pkg, pieces):
    """The second (and third) launch begins inside the cool-down the one before left: pl_first, counted by the count kernel
    from last_closure on the device, is the number of bot 2's events still inside it -- 30 less the 5 or 12 already gone."""
    cuts = _cuts_inside_cool_downs(pieces)
    plans = _run(pkg, "pile", 0, 30, cuts=cuts)
    assert plans[0][2]["first"] == 0 and plans[0][1]["first"] == 0
    assert plans[1][2]["first"] == 30 - 5
    if pieces == 3:
        assert plans[2][2]["first"] == 30 - 12
    assert all(len(p[1]["r"]) == 0 and p[1]["first"] == 0 for p in plans[1:])
