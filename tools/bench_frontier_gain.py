#!/usr/bin/env python3
"""Frontier gain: qs_frontier_gain alone (labelling, compaction, viewpoints, the gain kernel, read-back) and the whole
qs_frontier_targets_by_gain call, each between HIP events on the mapper's stream, median of --reps after --warmup calls.
The yardstick is the same build's qs_frontier_targets_by_path on the same map and bots, timed the same way: the same
stages without the gains and with the (cost, k) order.  The three cases are tools/bench_targets_by_path.py's:
  (a) "64"  : the 64-bot 4096^2 map;  (b) "8192": 255 bots at 8192^2;  (c) "open": 64 bots in one region at 2048^2.
Prints one JSON line with, per case, the three times, the clusters, the gain's distribution, how many bots' targets
changed, the mean gain and the mean cost of the chosen targets under each rule, and the gain kernel's LDS look-ups counted
from the map: for every cluster, the cells of the walks it makes (G3), plus one look-up per cell of the square to find the
targets.  The share of the gain kernel comes from a separate run under rocprofv3 --kernel-trace --stats (--only gain).
  usage: tools/bench_frontier_gain.py [--reps 25] [--warmup 3] [--cases 64,8192,open] [--range 24] [--bias 120] [--only gain]"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the HIP library (see _lib.load)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_targets_by_path import build_case, timed


def lookups(grid, views, rng, chunk=256):
    """LDS look-ups of the gain kernel, counted: per cluster (2 rng + 1)^2 target tests, and for every UNKNOWN cell of
    the disc its walk up to and including the first OCCUPIED cell (else all its cells but the last)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import gain_rules as G
    offs, cells = G.lines(rng)
    length = np.maximum(np.abs(offs[:, 0]), np.abs(offs[:, 1]))                 # cells of a walk but the last
    pad = np.arange(cells.shape[1])[None, :] >= length[:, None]
    p = np.pad(grid, rng, constant_values=G.OUTSIDE)
    v = views.astype(np.int64) + rng
    total = len(v) * (2 * rng + 1) ** 2
    for a in range(0, len(v), chunk):
        w = v[a:a + chunk]
        target = p[w[:, None, 1] + offs[None, :, 1], w[:, None, 0] + offs[None, :, 0]] == -1
        occ = (p[w[:, None, None, 1] + cells[None, :, :, 1], w[:, None, None, 0] + cells[None, :, :, 0]] == 100) & ~pad[None]
        first = np.where(occ.any(axis=2), occ.argmax(axis=2) + 1, length[None, :])
        total += int((first * target).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64,8192,open")
    ap.add_argument("--range", type=int, default=24)
    ap.add_argument("--bias", type=int, default=120)
    ap.add_argument("--only", default="", help="gain: only qs_frontier_gain (for a kernel trace of it alone)")
    a = ap.parse_args()
    side = torch.cuda.Stream()
    out = {"tool": "bench_frontier_gain", "reps": a.reps, "warmup": a.warmup, "range": a.range, "bias": a.bias, "cases": []}
    for name in a.cases.split(","):
        m, bots, min_cluster, desc = build_case(name)
        m.set_stream(side.cuda_stream)
        (view, gain), g_dev, _ = timed(side, a.reps, a.warmup, lambda: m.frontier_gain(min_cluster, a.range))
        case = {"case": name, "desc": desc, "bots": len(bots), "min_cluster": min_cluster, "clusters": len(gain),
                "gain": {"min": int(gain.min()), "median": float(np.median(gain)), "max": int(gain.max()), "sum": int(gain.sum())},
                "gain_ms_median": round(float(np.median(g_dev)), 3), "gain_ms_min": round(float(np.min(g_dev)), 3)}
        if a.only != "gain":
            p, p_dev, _ = timed(side, a.reps, a.warmup, lambda: m.frontier_targets_by_path(bots, min_cluster=min_cluster))
            r, r_dev, _ = timed(side, a.reps, a.warmup, lambda: m.frontier_targets_by_gain(
                bots, min_cluster=min_cluster, gain_range=a.range, gain_bias=a.bias))
            both = (p["idx"] >= 0) & (r["idx"] >= 0)
            case.update({
                "by_gain_ms_median": round(float(np.median(r_dev)), 3), "by_gain_ms_min": round(float(np.min(r_dev)), 3),
                "by_path_ms_median": round(float(np.median(p_dev)), 3), "by_path_ms_min": round(float(np.min(p_dev)), 3),
                "ratio_to_by_path": round(float(np.median(r_dev) / np.median(p_dev)), 3),
                "assigned_by_gain": int((r["idx"] >= 0).sum()), "assigned_by_path": int((p["idx"] >= 0).sum()),
                "targets_changed": int((p["idx"] != r["idx"]).sum()),
                "mean_gain_by_gain": round(float(r["gain"][both].mean()), 1) if both.any() else 0.0,
                "mean_gain_by_path": round(float(gain[p["idx"][both]].mean()), 1) if both.any() else 0.0,
                "mean_cost_by_gain": round(float(r["cost"][both].mean()), 1) if both.any() else 0.0,
                "mean_cost_by_path": round(float(p["cost"][both].mean()), 1) if both.any() else 0.0,
                "stats_by_gain": r["stats"], "stats_by_path": p["stats"]})
            n = lookups(m.grid_i8(), view, a.range)
            case.update({"lds_lookups": n, "lds_lookups_per_cluster": round(n / max(1, len(gain)), 1)})
        out["cases"].append(case)
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
