#!/usr/bin/env python3
"""Frontier target assignment: qs_frontier_targets on the device against the host path it replaces
(frontier_centroids() plus the reference's greedy loop, dual_bot_mapper.py:958-992, in plain Python).
Prints one JSON line.  Per case: the call's time between HIP events on the mapper's stream (median of --reps, the
whole call: labelling, centroids, lists, greedy pass, read-back), the host wall time of the call, clusters, fallback
scans, and the host path timed once with a cap (--host-cap seconds; `host_capped` says whether the cap was hit).
  usage: tools/bench_frontier_targets.py [--reps 25] [--host-cap 60] [--cases 64,255,8192] [--no-host]"""
import argparse
import importlib
import json
import math
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
P = pkg.protocol


def last_poses(m, stream):
    acc, pose = m.last_batch()
    agents = stream[:, 4]
    last = {}
    for i in np.nonzero(acc)[0]:
        last[int(agents[i])] = (float(pose[i, 0]), float(pose[i, 1]))
    return [last[b] for b in sorted(last)]


def host_path(m, bots, sep, cap_s):
    """frontier_centroids() and the greedy loop as the reference writes it; stops once cap_s has passed."""
    t0 = time.perf_counter()
    cents = m.frontier_centroids(P.FRONTIER_MIN_CLUSTER)
    targets, out = [], []
    for bx, by in bots:
        best, bi = math.inf, -1
        for i, (cx, cy) in enumerate(cents):
            if (i & 1023) == 0 and time.perf_counter() - t0 > cap_s:
                return time.perf_counter() - t0, True, len(out), out
            too_close = False
            for ti, tx, ty in targets:
                if i == ti or math.sqrt((cx - tx) ** 2 + (cy - ty) ** 2) < sep:
                    too_close = True
                    break
            if too_close:
                continue
            d = math.sqrt((bx - cx) ** 2 + (by - cy) ** 2)
            if d < best:
                best, bi = d, i
        out.append(bi)
        if bi >= 0:
            targets.append((bi, cents[bi][0], cents[bi][1]))
    return time.perf_counter() - t0, False, len(out), out


def scatter_rays(n, size, res, ox, seed=5):
    """n short rays (4-10 cells, any direction) spread over the map: about one frontier cluster each."""
    rng = np.random.default_rng(seed)
    lo, hi = ox + 1.0, ox + size * res - 1.0
    rx, ry = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    a, L = rng.uniform(-np.pi, np.pi, n), rng.uniform(4, 10, n) * res
    return rx, ry, rx + L * np.cos(a), ry + L * np.sin(a), np.ones(n, dtype=np.uint8)


def build_case(name):
    session, _ = replay.telemetry_csv_to_packets()
    if name == "64":
        stream = replay.multi_bot_stream(session, 64, 64 * 400)
        m = pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2)
        m.ingest_array(stream)
        return m, last_poses(m, stream), "64 bots, 4096^2 (test_frontiers_full_size_vs_oracle's stream)"
    if name == "255":
        stream = replay.multi_bot_stream(session, 255, 255 * 500)
        m = pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=255)
        m.ingest_array(stream)
        return m, last_poses(m, stream), "255 bots, 4096^2"
    stream = replay.multi_bot_stream(session, 255, 255 * 200)
    m = pkg.QuasarMapper(8192, 0.05, -204.8, -204.8, max_agent=255)
    m.ingest_array(stream)
    bots = last_poses(m, stream)
    m.update_rays(*scatter_rays(180000, 8192, 0.05, -204.8))
    return m, bots, "255 bots, 8192^2, 180k scattered short rays"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-cap", type=float, default=60.0)
    ap.add_argument("--cases", default="64,255,8192")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    side = torch.cuda.Stream()
    out = {"tool": "bench_frontier_targets", "separation": P.FRONTIER_SEPARATION, "min_cluster": P.FRONTIER_MIN_CLUSTER,
           "reps": a.reps, "cases": []}
    for name in a.cases.split(","):
        m, bots, desc = build_case(name)
        m.set_stream(side.cuda_stream)
        for _ in range(a.warmup):
            m.frontier_targets(bots)
        dev_ms, wall_ms = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            t0 = time.perf_counter()
            m.frontier_targets(bots)
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            e1.record(side)
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        idx, xy, cents, st = m.frontier_targets(bots, return_centroids=True)
        case = {"case": name, "desc": desc, "bots": len(bots), "clusters": st["n_centroids"], "k": st["k"],
                "fallbacks": st["fallbacks"], "assigned": int((idx >= 0).sum()),
                "device_ms_median": round(float(np.median(dev_ms)), 4), "device_ms_min": round(float(np.min(dev_ms)), 4),
                "device_ms_max": round(float(np.max(dev_ms)), 4), "wall_ms_median": round(float(np.median(wall_ms)), 4)}
        if not a.no_host:
            hs, capped, done, hidx = host_path(m, bots, P.FRONTIER_SEPARATION, a.host_cap)
            case.update({"host_s": round(hs, 3), "host_capped": capped, "host_bots_done": done,
                         "host_matches_device": (not capped) and hidx == idx.tolist()})
        out["cases"].append(case)
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
