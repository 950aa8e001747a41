"""tests/chain_plan_rules.py, the NumPy restatement of the lean owner's plan, against (1) a brute-force statement of the
reference's rule -- after a closure at node c an agent queries its first later event with node - c >= MIN_POSES_BETWEEN
(dual_bot_mapper.py:304), without one its next event -- on random event lists with random outcomes, and (2) oracle.c on
streams small enough for it: walked with the oracle's outcomes the plan visits every closing node, nothing inside a
cool-down, and ends at the end of the list."""
import numpy as np
import pytest

import chain_plan_rules as rules
from conftest import load_pkg
from oracle import oracle as orc

MINS = [0, 1, 5, 30, 31, 64, 2 ** 30 - 1]


def _brute(nodes, last_closure, min_between, closes):
    """The reference's loop over one agent's events: which are queried (own indices)."""
    last, seen = int(last_closure), []
    for j, nd in enumerate(int(v) for v in nodes):
        if nd - last >= min_between:
            seen.append(j)
            if closes(nd):
                last = nd
    return seen


def _random_list(rng, n_events, n_agents, shape):
    """ev_node strictly ascending from a random first node; ev_agent by `shape`."""
    gaps = rng.integers(1, 40, size=n_events)
    node = np.cumsum(gaps) + int(rng.integers(0, 1000))
    if shape == "one_owns_all":
        agent = np.full(n_events, int(rng.integers(0, n_agents)))
    elif shape == "some_silent":                                      # agents without events, and one that falls silent early
        live = rng.choice(n_agents, size=max(1, n_agents // 2), replace=False)
        agent = rng.choice(live, size=n_events)
        agent[n_events // 8:][agent[n_events // 8:] == live[0]] = live[-1]
    else:
        agent = rng.integers(0, n_agents, size=n_events)
    return node.astype(np.int64), agent.astype(np.int64)


@pytest.mark.parametrize("min_between", MINS)
@pytest.mark.parametrize("n_agents", [1, 2, 5, 13])
def test_restatement_equals_the_reference_rule(n_agents, min_between):
    rng = np.random.default_rng(1000 * n_agents + min_between % 997)
    for shape in ("mixed", "one_owns_all", "some_silent"):
        for n_events in (0, 1, 2, 63, 64, 65, 700):
            node, agent = _random_list(rng, n_events, n_agents, shape)
            lo = int(node[0]) if n_events else 0
            hi = int(node[-1]) if n_events else 0
            # last_closure: the start of a session, far negative, inside the list, beyond it
            for lc in (-min_between, -(2 ** 31), (lo + hi) // 2, hi, hi + 3 * max(min_between, 1)):
                last = np.full(n_agents, lc, dtype=np.int64)
                p = rules.plan(node, agent, n_agents, min_between, last)
                own = rules.own_lists(agent, n_agents)
                assert sorted(np.concatenate(own).tolist()) == list(range(n_events))
                for a in range(n_agents):
                    assert (np.diff(own[a]) > 0).all() and (agent[own[a]] == a).all()          # stable, and the agent's own
                    nodes = node[own[a]]
                    # skip and first against their definitions, by a scan
                    for j in range(len(nodes)):
                        k = next((k for k in range(j + 1, len(nodes)) if nodes[k] - nodes[j] >= min_between), len(nodes))
                        assert p[a]["skip"][j] == k
                    k = next((k for k in range(len(nodes)) if nodes[k] - lc >= min_between), len(nodes))
                    assert p[a]["first"] == k
                    # the walk against the reference's loop, for outcomes that never, always and sometimes close
                    coin = {int(v): bool(rng.integers(0, 2)) for v in nodes}
                    for closes in (lambda nd: False, lambda nd: True, lambda nd: coin[nd]):
                        assert rules.walk(p[a], closes) == _brute(nodes, lc, min_between, closes)


def _parked(legs):
    """Packets of bots standing still: legs = ((agent, (x, y), packets), ...), every packet a node and a landmark of type 5."""
    agent = np.concatenate([np.full(n, a) for a, _, n in legs])
    x = np.concatenate([np.full(n, p[0]) for _, p, n in legs])
    y = np.concatenate([np.full(n, p[1]) for _, p, n in legs])
    n = len(agent)
    z = np.zeros(n, dtype=int)
    return load_pkg().pack_packets(agent, x, y, np.zeros(n), z, z, np.zeros((n, 4)), np.full(n, 5)), agent


P, Q, FAR = (0.05, 0.05), (0.75, 0.35), (2.75, 0.35)
STREAMS = {
    "pile": ((1, P, 30), (2, Q, 200)),
    "away": ((1, P, 30), (2, Q, 60), (2, FAR, 50), (2, Q, 60)),
    "interleaved": tuple((1 + (i % 3), (P, Q, FAR)[i % 3], 7 + i % 5) for i in range(60)),
}


@pytest.mark.parametrize("min_between", [0, 1, 5, 30, 31, 64])
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_walk_with_the_oracles_outcomes(name, min_between):
    stream, agent = _parked(STREAMS[name])
    nb = int(agent.max())
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0, max_agent=nb)
    o.set_closure_params(0.6, min_between, 0.5)
    o.feed_stream(stream)
    closing = set(o.closures(0)[0][:, 1].tolist())
    _, ti = o.landmarks(0)
    node = ti[:, 1]
    assert (node == np.arange(len(agent))).all()                     # every packet a node and an event: the list is the stream
    assert len(closing) > (3 if min_between <= 30 else 0)
    p = rules.plan(node, agent - 1, nb, min_between, np.full(nb, -min_between, dtype=np.int64))
    visited = set()
    for a in range(nb):
        seen = rules.walk(p[a], lambda nd: nd in closing)
        nodes = p[a]["node"]
        last = -min_between
        for j in seen:                                               # nothing inside a cool-down
            assert nodes[j] - last >= min_between
            if int(nodes[j]) in closing:
                last = int(nodes[j])
        # the walk ends at the end of the list: whatever follows its last stop is inside the last cool-down
        tail = nodes[seen[-1] + 1:] if seen else nodes
        assert all(nd - last < min_between for nd in tail)
        visited |= {int(nodes[j]) for j in seen}
    assert closing <= visited
