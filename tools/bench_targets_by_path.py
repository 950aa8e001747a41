#!/usr/bin/env python3
"""Frontier targets by path cost: qs_frontier_targets_by_path on the device, the whole call (centroids, mask, census,
snaps, every group's rounds, gather / top-K, greedy pass, waypoint fields and walks, read-back) between HIP events on the
mapper's stream, median of --reps after --warmup calls.  The yardstick is the same build's qs_frontier_targets +
qs_plan_paths (to the assigned centroids) on the same map and bots, timed the same way: what a target tick does without
the new call, and strictly less work (one field per assigned bot against one per bot plus one per assigned bot).
Prints one JSON line with, per case, both times and their ratio, rounds, tile visits, groups, fallbacks, and how many
straight-line targets had no path (the new call's have one by construction).
  (a) "64"  : the 64-bot 4096^2 map of test_gpu_plan_paths.py's map64;
  (b) "8192": 255 bots at 8192^2 (case (b) of bench_plan_paths.py);
  (c) "open": 64 bots in ONE connected region of 1600 x 1600 FREE cells at 2048^2 with an UNKNOWN cell every 64 cells of
              every 64th row (625 small frontiers): every field floods the whole region, paths are long.
The share of the gather / top-K kernels comes from a separate run under rocprofv3 --kernel-trace --stats.
  usage: tools/bench_targets_by_path.py [--reps 25] [--warmup 3] [--cases 64,8192,open] [--no-baseline]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "distributed-multi-agent-slam-swarm-robotics-system_amd"
import numpy as np
import torch  # before the HIP library (see _lib.load)

pkg = importlib.import_module(PKG)
replay = importlib.import_module(PKG + ".replay")


def last_poses(m, stream):
    acc, pose = m.last_batch()
    agents = stream[:, 4]
    last = {}
    for i in np.nonzero(acc)[0]:
        last[int(agents[i])] = (float(pose[i, 0]), float(pose[i, 1]))
    return [last[b] for b in sorted(last)]


def open_map():
    """FREE cells [200, 1800)^2 of a 2048^2 grid but for one cell every 64 of every 64th row; 64 bots spread over it."""
    m = pkg.QuasarMapper(2048, 0.05, -51.2, -51.2)
    c = lambda g: -51.2 + (np.asarray(g) + 0.5) * 0.05
    rows = np.arange(200, 1800)
    holed = rows[rows % 64 == 32]
    plain = rows[rows % 64 != 32]
    rx, hx, ry = [np.full(len(plain), c(200))], [np.full(len(plain), c(1800))], [c(plain)]
    for a in range(200, 1800, 64):                        # [a, a + 63) FREE, a + 63 stays UNKNOWN
        rx.append(np.full(len(holed), c(a))); hx.append(np.full(len(holed), c(a + 63))); ry.append(c(holed))
    rx, hx, ry = np.concatenate(rx), np.concatenate(hx), np.concatenate(ry)
    m.update_rays(rx, ry, hx, ry, np.zeros(len(rx), dtype=np.uint8))
    rng = np.random.default_rng(11)
    return m, c(rng.integers(210, 1790, (64, 2)))


def build_case(name):
    if name == "open":
        m, bots = open_map()
        return m, bots, 1, "64 bots in one connected region of 1600^2 FREE cells at 2048^2, 625 one-cell holes"
    session, _ = replay.telemetry_csv_to_packets()
    if name == "64":
        stream = replay.multi_bot_stream(session, 64, 64 * 400)
        m = pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2)
        desc = "64 bots, 4096^2 (the map64 stream)"
    else:
        stream = replay.multi_bot_stream(session, 255, 255 * 200)
        m = pkg.QuasarMapper(8192, 0.05, -204.8, -204.8, max_agent=255)
        desc = "255 bots, 8192^2"
    m.ingest_array(stream)
    return m, np.array(last_poses(m, stream)), 3, desc


def timed(side, reps, warmup, fn):
    for _ in range(warmup):
        fn()
    dev_ms, wall_ms, r = [], [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        t0 = time.perf_counter()
        r = fn()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        e1.record(side)
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    return r, dev_ms, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="64,8192,open")
    ap.add_argument("--no-baseline", action="store_true", help="only the new call (for a kernel trace of it alone)")
    a = ap.parse_args()
    side = torch.cuda.Stream()
    out = {"tool": "bench_targets_by_path", "reps": a.reps, "warmup": a.warmup, "cases": []}
    for name in a.cases.split(","):
        m, bots, min_cluster, desc = build_case(name)
        m.set_stream(side.cuda_stream)

        def baseline():
            idx, xy = m.frontier_targets(bots, min_cluster=min_cluster)
            ok = idx >= 0
            return idx, m.plan_paths(bots[ok], xy[ok])

        (idx, line), b_dev, b_wall = timed(side, 1 if a.no_baseline else a.reps, 0 if a.no_baseline else a.warmup, baseline)
        r, dev, wall = timed(side, a.reps, a.warmup, lambda: m.frontier_targets_by_path(bots, min_cluster=min_cluster))
        st, lst = r["status"], line["status"]
        check = m.plan_paths(bots[r["idx"] >= 0], r["xy"][r["idx"] >= 0])
        med, bmed = float(np.median(dev)), float(np.median(b_dev))
        case = {"case": name, "desc": desc, "bots": len(bots), "min_cluster": min_cluster,
                "status": {k: int((st == i).sum()) for i, k in enumerate(pkg._lib.QS_PLAN_STATUS)},
                "assigned": int((r["idx"] >= 0).sum()), "assigned_unreachable": int((check["status"] != 0).sum()),
                "mean_cost_assigned": round(float(r["cost"][st == 0].mean()), 1) if (st == 0).any() else 0.0,
                "traversable_cells": int(m.traversable().sum()),
                **r["stats"],
                "device_ms_median": round(med, 3), "device_ms_min": round(float(np.min(dev)), 3),
                "wall_ms_median": round(float(np.median(wall)), 3),
                "baseline": {"what": "frontier_targets + plan_paths(assigned)", "assigned": int((idx >= 0).sum()),
                             "unreachable": int((lst == 3).sum()), "ok": int((lst == 0).sum()), **line["stats"],
                             "device_ms_median": round(bmed, 3), "device_ms_min": round(float(np.min(b_dev)), 3),
                             "wall_ms_median": round(float(np.median(b_wall)), 3)},
                "ratio_to_baseline": round(med / bmed, 3)}
        out["cases"].append(case)
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
