#!/usr/bin/env python3
"""Territories: qs_territories and qs_frontier_targets_by_territory on the device, each whole call between HIP events on the
mapper's stream, median of --reps after --warmup calls, on the three cases of tools/bench_targets_by_path.py (whose map
builders and timing loop this tool uses).  The baseline is the same build's qs_frontier_targets_by_path on the same map
and bots, with and without its waypoint stage (without: its first field stage, one field per bot, and the assignment).
Prints one JSON line with, per case: the times, rounds and tile visits of each call, and how many bots each method
assigns.  The kernels' shares come from a separate run under rocprofv3 --kernel-trace --stats (--no-baseline).
  usage: tools/bench_territories.py [--reps 25] [--warmup 3] [--cases 64,8192,open] [--no-baseline]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_targets_by_path as B       # (imports torch before the HIP library)
import numpy as np
import torch


def entry(r, dev, wall):
    keep = ("rounds", "tile_visits", "bot_cells", "owned_cells", "n_centroids", "centroid_cells", "centroids_owned", "groups",
            "fallbacks")
    out = {k: v for k, v in r["stats"].items() if k in keep}
    if "idx" in r:
        out["assigned"] = int((r["idx"] >= 0).sum())
    out.update(device_ms_median=round(float(np.median(dev)), 3), device_ms_min=round(float(np.min(dev)), 3),
               wall_ms_median=round(float(np.median(wall)), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64,8192,open")
    ap.add_argument("--no-baseline", action="store_true", help="only the new calls (for a kernel trace of them alone)")
    a = ap.parse_args()
    side = torch.cuda.Stream()
    out = {"tool": "bench_territories", "reps": a.reps, "warmup": a.warmup, "cases": []}
    for name in a.cases.split(","):
        m, bots, min_cluster, desc = B.build_case(name)
        m.set_stream(side.cuda_stream)
        run = lambda fn: entry(*B.timed(side, a.reps, a.warmup, fn))
        case = {"case": name, "desc": desc, "bots": len(bots), "min_cluster": min_cluster,
                "traversable_cells": int(m.traversable().sum()),
                "territories": run(lambda: m.territories(bots)),
                "by_territory": run(lambda: m.frontier_targets_by_territory(bots, min_cluster=min_cluster)),
                "by_territory_no_waypoints": run(lambda: m.frontier_targets_by_territory(bots, min_cluster=min_cluster,
                                                                                         waypoints=False))}
        if not a.no_baseline:
            case["by_path"] = run(lambda: m.frontier_targets_by_path(bots, min_cluster=min_cluster))
            case["by_path_no_waypoints"] = run(lambda: m.frontier_targets_by_path(bots, min_cluster=min_cluster, waypoints=False))
            case["ratio_to_by_path"] = round(case["by_territory"]["device_ms_median"] / case["by_path"]["device_ms_median"], 3)
            case["partition_to_first_field_stage"] = round(case["territories"]["device_ms_median"] /
                                                           case["by_path_no_waypoints"]["device_ms_median"], 3)
        out["cases"].append(case)
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
