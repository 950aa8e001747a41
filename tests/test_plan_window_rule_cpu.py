"""The window rule by which csrc/slam.hip's qs_slam_plan_scatter_kernel works out a plan record's skip, and pl_first as the
count qs_slam_plan_count_kernel takes, stated in NumPy on the graph's event list as it comes in and checked against
tests/chain_plan_rules.py, which states both as searches in the agents' own lists.

Take a graph's event list (nodes distinct and ascending) and let event e be own event j of its agent.  With p the first list
position after e whose node is >= node[e] + MIN_POSES_BETWEEN (the list's end without one),

    skip[j] = j + 1 + #{events of the same agent at positions in (e, p)}

and since the nodes are distinct, p <= e + max(MIN_POSES_BETWEEN, 1): the count never looks further than that.
first = #{events of the agent with node < last_closure + MIN_POSES_BETWEEN}."""
import numpy as np
import pytest

import chain_plan_rules as rules

MIN_BETWEEN = [-3, 0, 1, 2, 30, 31, 64, 256, 257]


def window_plan(ev_node, ev_agent, n_agents, min_between, last_closure):
    """Per agent dict(r, node, skip, first), from the event list alone; every event looks at no more than the
    max(min_between, 1) - 1 entries behind it."""
    ev_node = np.asarray(ev_node, dtype=np.int64)
    ev_agent = np.asarray(ev_agent)
    n, window = len(ev_node), max(int(min_between), 1)
    own = np.zeros(n, dtype=np.int64)                  # j: the event's number among its agent's
    seen = np.zeros(n_agents, dtype=np.int64)
    for e in range(n):
        own[e] = seen[ev_agent[e]]
        seen[ev_agent[e]] += 1
    skip = np.zeros(n, dtype=np.int64)
    for e in range(n):
        end = min(n, e + window)
        past = np.nonzero(ev_node[e + 1:end] >= ev_node[e] + np.int64(min_between))[0]
        p = e + 1 + int(past[0]) if len(past) else end
        skip[e] = own[e] + 1 + int((ev_agent[e + 1:p] == ev_agent[e]).sum())
    out = []
    for a in range(n_agents):
        r = np.nonzero(ev_agent == a)[0]
        first = int((ev_node[r] < np.int64(last_closure[a]) + np.int64(min_between)).sum())
        out.append({"r": r, "node": ev_node[r], "skip": skip[r], "first": first})
    return out


def _same(ev_node, ev_agent, n_agents, min_between, last_closure):
    got = window_plan(ev_node, ev_agent, n_agents, min_between, last_closure)
    want = rules.plan(ev_node, ev_agent, n_agents, min_between, last_closure)
    assert len(got) == len(want) == n_agents
    for a, (g, w) in enumerate(zip(got, want)):
        for f in ("r", "node", "skip"):
            assert np.array_equal(g[f], w[f]), (a, f, min_between)
        assert g["first"] == w["first"], (a, min_between)
        assert np.array_equal(w["skip"], rules.skip_table(w["node"], min_between))
        assert w["first"] == rules.first_candidate(w["node"], last_closure[a], min_between)
    return got


def _random_list(rng, n, n_agents, absent=()):
    """n events: nodes ascending with gaps of 1 mostly (every packet an event), now and then a longer one; agents at random
    among those not absent, in runs of random length."""
    gaps = np.where(rng.random(n) < 0.8, 1, rng.integers(2, 70, n))
    node = np.int64(rng.integers(0, 1000)) + np.cumsum(gaps)
    present = [a for a in range(n_agents) if a not in absent]
    agent = np.empty(n, dtype=np.int64)
    k = 0
    while k < n:
        run = int(rng.integers(1, 40))
        agent[k:k + run] = present[int(rng.integers(0, len(present)))]
        k += run
    return node, agent


@pytest.mark.parametrize("min_between", MIN_BETWEEN)
@pytest.mark.parametrize("n_agents", [1, 2, 3, 4, 5, 6])
def test_random_lists(n_agents, min_between):
    rng = np.random.default_rng(1000 * n_agents + min_between + 7)
    for n in (0, 1, 2, 257, 700):
        node, agent = _random_list(rng, n, n_agents)
        lo, hi = (int(node[0]), int(node[-1])) if n else (0, 0)
        for lc in (-(1 << 40), lo - min_between, (lo + hi) // 2, hi, hi + 1000):   # far negative, at the start, inside, at the end, beyond
            _same(node, agent, n_agents, min_between, [lc + a for a in range(n_agents)])


@pytest.mark.parametrize("min_between", MIN_BETWEEN)
def test_agent_without_events_and_with_one(min_between):
    rng = np.random.default_rng(min_between + 11)
    node, agent = _random_list(rng, 400, 4, absent=(1, 3))
    agent[200] = 3                                                  # agent 3's only event; agent 1 has none
    got = _same(node, agent, 4, min_between, [-(1 << 40), 5, int(node[200]) - 1, int(node[200])])
    assert len(got[1]["r"]) == 0 and got[1]["first"] == 0
    assert len(got[3]["r"]) == 1 and got[3]["skip"][0] == 1
    _same(node, agent, 4, min_between, [int(node[-1])] * 4)


@pytest.mark.parametrize("min_between", MIN_BETWEEN)
def test_no_event_after_the_window(min_between):
    """Agent 1's events end well before the list does: behind its last ones the window holds only agent 0's, and the skip is
    agent 1's count, "none".  Agent 0's last events have windows that end with the list."""
    node = np.arange(100, 700, dtype=np.int64)
    agent = np.zeros(600, dtype=np.int64)
    agent[50:300:3] = 1
    got = _same(node, agent, 2, min_between, [-min_between, 350])
    n1 = len(got[1]["r"])
    assert got[1]["skip"][-1] == n1
    assert got[0]["skip"][-1] == len(got[0]["r"])
    if min_between >= 64:                                          # agent 1's last closure at node 350: nothing of it is left past the cool-down
        assert got[1]["first"] == n1
    if min_between > 1:                                             # gaps of 1: the event before the last skips the last as well
        assert got[0]["skip"][-2] == len(got[0]["r"])


@pytest.mark.parametrize("min_between", MIN_BETWEEN)
def test_window_holds_fewer_events_than_the_cool_down(min_between):
    """What makes the rule local: p - e <= max(min_between, 1), whatever the gaps."""
    rng = np.random.default_rng(min_between + 23)
    node, _ = _random_list(rng, 900, 1)
    p = np.maximum(np.searchsorted(node, node + np.int64(min_between), side="left"), np.arange(len(node)) + 1)
    assert (p - np.arange(len(node)) <= max(min_between, 1)).all()
    if min_between >= 1:
        dense = np.arange(5000, 5900, dtype=np.int64)             # gaps of 1: the bound is reached
        p = np.minimum(np.searchsorted(dense, dense + np.int64(min_between), side="left"), len(dense))
        assert (p - np.arange(len(dense)))[: len(dense) - min_between].max() == min_between
