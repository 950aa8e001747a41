"""The plan of the lean owner of the free-running chain (csrc/slam.hip, qs_slam_plan_*_kernel), restated in NumPy.

A graph's landmark events come as one list in node order (ev_node strictly ascending, ev_agent the owner of each).  Which event
an agent queries next depends on a decision in one way only -- whether it closed a loop:

  * after a closure at its own event j, its first own event k > j with node[k] - node[j] >= MIN_POSES_BETWEEN (skip[j]);
  * without one, its next own event, j + 1;
  * at the start of a launch, its first own event with node - last_closure >= MIN_POSES_BETWEEN (first).

The own lists are a stable partition of the event list by agent; skip and first are binary searches in them (the nodes
ascend).  "None" is the length of the own list."""
import numpy as np


def own_lists(ev_agent, n_agents):
    """Per agent the positions r (in the graph's event list) of its own events, in list order."""
    ev_agent = np.asarray(ev_agent)
    order = np.argsort(ev_agent, kind="stable")
    counts = np.bincount(ev_agent, minlength=n_agents)[:n_agents] if len(ev_agent) else np.zeros(n_agents, dtype=np.int64)
    return np.split(order, np.cumsum(counts)[:-1])


def skip_table(nodes, min_between):
    """skip[j] = the first k > j with nodes[k] - nodes[j] >= min_between, len(nodes) if there is none."""
    nodes = np.asarray(nodes, dtype=np.int64)
    k = np.searchsorted(nodes, nodes + np.int64(min_between), side="left")
    return np.maximum(k, np.arange(len(nodes)) + 1)


def first_candidate(nodes, last_closure, min_between):
    """The first k with nodes[k] - last_closure >= min_between, len(nodes) if there is none."""
    return int(np.searchsorted(np.asarray(nodes, dtype=np.int64), np.int64(last_closure) + np.int64(min_between), side="left"))


def plan(ev_node, ev_agent, n_agents, min_between, last_closure):
    """Per agent a: dict(r, node, skip, first) -- r and node of its own events, skip of each, and its first candidate given
    last_closure[a]."""
    ev_node = np.asarray(ev_node, dtype=np.int64)
    out = []
    for a, r in enumerate(own_lists(ev_agent, n_agents)):
        nodes = ev_node[r]
        out.append({"r": r, "node": nodes, "skip": skip_table(nodes, min_between),
                    "first": first_candidate(nodes, last_closure[a], min_between)})
    return out


def walk(p, closes):
    """The own indices an owner queries, walking the plan p of one agent; closes(node) says whether the query at node closes."""
    j, n, seen = p["first"], len(p["node"]), []
    while j < n:
        seen.append(j)
        j = int(p["skip"][j]) if closes(int(p["node"][j])) else j + 1
    return seen
