"""The scout of the free-running chain (csrc/slam_chain_scout.inc, slam_chain_scout_owner.inc), restated in NumPy on top of
tests/chain_plan_rules.py (which event an owner queries next) and tests/chain_lookahead_rules.py (the index and the lean query).

Decision m of an agent is at its own event j_m, at the pose q_m = p[j_m] + drift after decision m - 1 -- the pose the event's
landmark is stored at.  The stage it can use was made two decisions earlier, for the candidate skip[j_(m-1)] (the tag) at the
pose f_m = p[j_m] + drift after decision m - 2 = q_m - (the correction of decision m - 1).  The scout covers a window of W x W
bucket cells around the cell of f_m: W = 5, two cells either way; W = 4, one cell on the side f_m lies nearer to and two on
the other.  The owner takes the stage if the tag is j_m, the 3 x 3 cells around the cell of q_m lie inside the window, the
landmark's type has a slab in the index, and then settles the decision from it if the first nodes of the 3 x 3 show a match
and no bucket has to be walked further (Chains.query: one round, settled by the lean owner)."""
import numpy as np

import chain_lookahead_rules as L
import chain_plan_rules as P

W = 4


def window(geom, fx, fy, w=W):
    """The base cell of the window the scout covers for the foreseen pose."""
    cx, cy = geom.cell(fx, fy)
    if w == 5:
        return cx - 2, cy - 2
    tx, ty = (fx - geom.ox) * geom.inv, (fy - geom.oy) * geom.inv
    return cx - (2 if tx - np.floor(tx) < 0.5 else 1), cy - (2 if ty - np.floor(ty) < 0.5 else 1)


def covers(geom, fx, fy, qx, qy, w=W):
    """Whether the 3 x 3 cells around the cell of (qx, qy) lie inside the window made for (fx, fy)."""
    bx, by = window(geom, fx, fy, w)
    cx, cy = geom.cell(qx, qy)
    return 0 <= cx - 1 - bx <= w - 3 and 0 <= cy - 1 - by <= w - 3


def decisions(plan, xy_of, corr_of):
    """One agent's decisions in a launch: [(j, node, (qx, qy), (fx, fy), tag is j)], from its plan (chain_plan_rules.plan),
    xy_of[node] the pose its landmark is stored at, corr_of[node] the correction of the closure at node (absent: no closure).
    The first decision has no stage (tag False)."""
    out, prev_j, prev_corr = [], None, (0.0, 0.0)
    for j in P.walk(plan, lambda node: node in corr_of):
        node = int(plan["node"][j])
        q = xy_of[node]
        tag = prev_j is not None and int(plan["skip"][prev_j]) == j
        out.append((j, node, q, (q[0] - prev_corr[0], q[1] - prev_corr[1]), tag))
        prev_j, prev_corr = j, corr_of.get(node, (0.0, 0.0))
    return out


def staged(geom, chains, plan, xy_of, type_of, corr_of, min_between, w=W):
    """(decisions settled from a stage, decisions by the owner's own loads, of those the ones the window missed) for one agent
    in a launch whose every first match lies in `chains`, the index as of the launch's start, with an empty side list."""
    n_staged = n_fall = n_miss = 0
    for j, node, q, f, tag in decisions(plan, xy_of, corr_of):
        t = type_of[node]
        ok = tag and 1 <= t <= L.NTYPES
        if ok and not covers(geom, f[0], f[1], q[0], q[1], w):
            ok = False
            n_miss += 1
        if ok:
            match, rounds, lean, _ = chains.query(q[0], q[1], t, node - max(min_between, 1), "ahead")
            ok = match >= 0 and lean and rounds == 1
        n_staged += ok
        n_fall += not ok
    return n_staged, n_fall, n_miss
