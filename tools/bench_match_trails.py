#!/usr/bin/env python3
"""Trail matching rate: qs_match_trails_device on 2^14 trails of 32 and of 64 packets (42-byte records, device-resident),
sensed by qs_sense_packets_device from drives through a region of a 4096^2 grid of 5 cm mapped from random sweeps, at the
default window (R 2, W 6, T 10) and the default travel; beside it, in the same run, qs_match_sweeps_device on 2^14 sweeps of
the same region (the two share the scoring loop); and the CPU restatement's rate (tests/trail_rules.py, numpy) on a subset.
Median of --reps calls after a warm-up, qs_sync inside the timed span.  Prints one JSON line.

    python tools/bench_match_trails.py [--trails 16384] [--reps 10]

Candidate look-ups of a trail: hit points x (2 W + 1)^2 x (2 T + 1).  The LDS floor the rate is held against is that of the
form csrc/trail.hip builds, which is csrc/match.hip's (a lane per rotation, iy and FOUR adjacent ix): per wave and per four
points one 8-byte read of four patch offsets and eight dword reads of the field, 2 LDS cycles each = 4.5 cycles per point,
over (2 T + 1) (2 W + 1) ceil((2 W + 1) / 4) / 64 waves' worth of lanes, on 256 CUs at 2.4 GHz."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quasar_amd as qa  # noqa: E402
import trail_rules as TR  # noqa: E402

P = qa.protocol
CUS, CLOCK_HZ = 256, 2.4e9
SIZE, RES, REGION = 4096, 0.05, 20.0


def sweeps(n, seed, half):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.05, 1.6, (n, P.SWEEP_BEAMS)).astype(np.float32)
    return P.pack_sweeps(rng.integers(1, 3, n), rng.uniform(-half, half, n), rng.uniform(-half, half, n),
                         rng.uniform(-math.pi, math.pi, n), r, odometry=True)


def drives(n, K, seed, half, step=0.05, max_rate=0.08):
    """Poses float32 [n * K, 3] of n drives of K steps: `step` metres along the heading, a constant yaw rate per drive."""
    rng = np.random.default_rng(seed)
    yaw = rng.uniform(-math.pi, math.pi, n)[:, None] + rng.uniform(-max_rate, max_rate, n)[:, None] * np.arange(K)[None, :]
    x = rng.uniform(-half, half, n)[:, None] + np.concatenate([np.zeros((n, 1)), np.cumsum(step * np.cos(yaw[:, :-1]), axis=1)], axis=1)
    y = rng.uniform(-half, half, n)[:, None] + np.concatenate([np.zeros((n, 1)), np.cumsum(step * np.sin(yaw[:, :-1]), axis=1)], axis=1)
    return np.stack([x, y, yaw], axis=2).reshape(n * K, 3).astype(np.float32)


def lds_floor_cycles(points, W, T):
    ny = 2 * W + 1
    return (2 * T + 1) * ny * ((ny + 3) // 4) / 64.0 * points * 4.5


def timed(fn, m, reps):
    fn()
    m.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        m.sync()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t)


def run(n_trails, reps, cpu_trails=8):
    dev = torch.device("cuda", 0)
    half = SIZE * RES / 2
    out = dict(trails=[])
    with qa.QuasarMapper(SIZE, RES, -half, -half, raycast_mode=0) as m:
        world = sweeps(1 << 16, 1, REGION)
        d_world = torch.from_numpy(world).to(dev)
        torch.cuda.synchronize()
        m.ingest_sweeps_device(d_world.data_ptr(), len(world), world.shape[1])          # the mapped region
        m.sync()
        p = m.match_params(None)
        for K in (32, 64):
            n = n_trails * K
            d_pose = torch.from_numpy(drives(n_trails, K, 10 + K, REGION)).to(dev)
            d_agent = torch.ones(n, dtype=torch.uint8, device=dev)
            d_pk = torch.zeros(n * P.PACKET_SIZE, dtype=torch.uint8, device=dev)
            d_out = torch.zeros(n_trails * P.TRAIL_MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            gsize = np.full(n_trails, K, dtype=np.int32)
            torch.cuda.synchronize()
            m.sense_packets_device(d_pose, d_agent, n, d_pk)
            m.sync()
            call = lambda: m.match_trails_device(d_pk.data_ptr(), n, P.PACKET_SIZE, gsize, d_out.data_ptr(), params=p)
            med, best = timed(call, m, reps)
            res = d_out.cpu().numpy().view(P.TRAIL_MATCH_DTYPE)
            hits = float(res["hits"].mean())
            lookups = float(res["hits"].sum()) * (2 * p.window + 1) ** 2 * (2 * p.angle_steps + 1)
            floor_s = n_trails * lds_floor_cycles(hits, p.window, p.angle_steps) / (CUS * CLOCK_HZ)
            row = dict(K=K, trails=n_trails, radius=p.radius, window=p.window, angle_steps=p.angle_steps, travel=P.TRAIL_TRAVEL,
                       ms_median=med * 1e3, ms_min=best * 1e3, trails_per_s=n_trails / med, lookups_per_s=lookups / med,
                       hit_points_mean=hits, records_mean=float(res["records"].mean()),
                       accepted_matches=int(res["accepted_match"].sum()), lds_floor_ms=floor_s * 1e3, lds_floor_fraction=floor_s / med)
            if K == 64:                                            # the CPU restatement on a few of the same trails
                grid = m.grid_i8()
                pk = d_pk.cpu().numpy().reshape(n, P.PACKET_SIZE)[:cpu_trails * K]
                pp = TR.params()
                L = TR.field(grid, pp["radius"])
                t0 = time.perf_counter()
                h = sum(TR.match_one(L, (RES, -half, -half), pk[k * K:(k + 1) * K], pp)[0]["hits"] for k in range(cpu_trails))
                dt = time.perf_counter() - t0
                out["cpu_restatement"] = dict(trails=cpu_trails, K=K, trails_per_s=cpu_trails / dt, lookups_per_s=h * 13 * 13 * 21 / dt)
            out["trails"].append(row)
        # the yardstick: sweep matching in the same run, same map, as many records as there are trails
        ns = min(n_trails, len(world))
        d_sw = d_world                                             # (its first ns records)
        d_mo = torch.zeros(ns * P.MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        med, best = timed(lambda: m.match_sweeps_device(d_sw.data_ptr(), ns, world.shape[1], d_mo.data_ptr(), params=p), m, reps)
        res = d_mo.cpu().numpy().view(P.MATCH_DTYPE)
        hits = float(res["hits"].mean())
        lookups = float(res["hits"].sum()) * (2 * p.window + 1) ** 2 * (2 * p.angle_steps + 1)
        floor_s = ns * lds_floor_cycles(hits, p.window, p.angle_steps) / (CUS * CLOCK_HZ)
        out["sweeps"] = dict(sweeps=ns, ms_median=med * 1e3, ms_min=best * 1e3, sweeps_per_s=ns / med, lookups_per_s=lookups / med,
                             hit_beams_mean=hits, lds_floor_ms=floor_s * 1e3, lds_floor_fraction=floor_s / med)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trails", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    out = dict(metric="trail_match", size=SIZE, res=RES, region_m=2 * REGION, stride=P.PACKET_SIZE)
    out.update(run(a.trails, a.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
