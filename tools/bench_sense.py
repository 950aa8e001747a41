#!/usr/bin/env python3
"""Sensing rate: qs_sense_sweeps_device and qs_sense_packets_device from 2^16 device-resident poses in a mapped world of 4096^2
and 8192^2 cells of 5 cm, at R = 1.2 m and 3.0 m.  Median of --reps calls with qs_sync inside the span.  Prints one JSON line.

    python tools/bench_sense.py [--poses 65536] [--reps 10]

The world is a 40 m x 40 m floor in the middle of the grid, FREE, with walls every 4 m that have a half-metre door in each
stretch: at 1.2 m most beams return nothing and walk their whole line, at 3.0 m most end on a wall.  Beside each sweep rate stands
the same run's qs_ingest_sweeps_device rate on the records just sensed (another context, trust filter 0.02 < d <= R): sensing
feeds that call, and the loop is as fast as the slower of the two.  The restatement's rate on the CPU (tests/sense_rules.py) is
measured on 64 of the poses.

The floor of the form built: a sweep record requests its (2 C + 1)^2 patch of stamps, 4 bytes a cell, once, and
writes its 751 bytes; a packet requests up to C stamps per beam and writes 42 bytes.  `floor_share` is the time those bytes take
at 8 TB/s over the measured time.  (At this pose density the patches overlap and come from L2, not HBM.)"""
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
import sense_rules as S  # noqa: E402

P = qa.protocol
PEAK_BPS = 8.0e12
RES, REGION_M, ROOM_CELLS, DOOR = 0.05, 40.0, 80, (35, 45)


def paint_world(m):
    """The floor's rows as free rays, then every wall cell as a zero-length hit (a later ray wins a cell)."""
    n = int(REGION_M / RES)
    lo = (m.size - n) // 2
    c = lambda g, o: o + (np.asarray(g, dtype=np.float64) + 0.5) * m.res
    rows = np.arange(lo, lo + n)
    m.update_rays(c(np.full(n, lo), m.ox), c(rows, m.oy), c(np.full(n, lo + n), m.ox), c(rows, m.oy), np.zeros(n, np.uint8))
    t = np.arange(n + 1)
    wall = t[(t % ROOM_CELLS < DOOR[0]) | (t % ROOM_CELLS >= DOOR[1])]
    lines = np.arange(0, n + 1, ROOM_CELLS)
    wx = np.concatenate([np.repeat(lines, len(wall)), np.tile(wall, len(lines))]) + lo
    wy = np.concatenate([np.tile(wall, len(lines)), np.repeat(lines, len(wall))]) + lo
    m.update_rays(c(wx, m.ox), c(wy, m.oy), c(wx, m.ox), c(wy, m.oy), np.ones(len(wx), np.uint8))
    return int(len(np.unique(wy * m.size + wx)))


def timed(call, sync, reps):
    call(); sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(); sync()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t)


def run(size, poses, reps):
    dev = torch.device("cuda", 0)
    n = len(poses)
    half = size * RES / 2
    d_pose = torch.from_numpy(poses).to(dev)
    d_agent = torch.ones(n, dtype=torch.uint8, device=dev)
    d_pkts = torch.zeros(n * P.PACKET_SIZE_V0_ODO, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    out = dict(size=size, runs=[])
    with qa.QuasarMapper(size, RES, -half, -half) as world:
        out["wall_cells"] = paint_world(world)
        for R in (1.2, 3.0):
            C = math.ceil(R / RES) + 1
            patch_bytes = (2 * C + 1) ** 2 * 4
            med, best = timed(lambda: world.sense_sweeps_device(d_pose, d_agent, n, d_pkts, P.PACKET_SIZE_V0_ODO, max_range=R), world.sync, reps)
            ranges = S.ranges_of(P, d_pkts.cpu().numpy().reshape(n, P.PACKET_SIZE_V0_ODO))
            r = dict(kind="sweeps", max_range=R, C=C, ms_median=med * 1e3, ms_min=best * 1e3, sweeps_per_s=n / med,
                     beams_per_s=n * P.SWEEP_BEAMS / med, return_share=float((ranges > 0).mean()),
                     floor_bytes_per_record=patch_bytes + P.PACKET_SIZE_V0_ODO, lds_reads_per_beam_max=C,
                     floor_share=n * (patch_bytes + P.PACKET_SIZE_V0_ODO) / PEAK_BPS / med)
            with qa.QuasarMapper(size, RES, -half, -half, min_dist=0.02, max_dist=R) as m:
                m.set_sweep_filter(0.02, R)
                imed, ibest = timed(lambda: m.ingest_sweeps_device(d_pkts.data_ptr(), n, P.PACKET_SIZE_V0_ODO), m.sync, reps)
            r.update(ingest_ms_median=imed * 1e3, ingest_sweeps_per_s=n / imed, sense_over_ingest=med / imed)
            out["runs"].append(r)
            med, best = timed(lambda: world.sense_packets_device(d_pose, d_agent, n, d_pkts, max_range=R), world.sync, reps)
            out["runs"].append(dict(kind="packets", max_range=R, C=C, ms_median=med * 1e3, ms_min=best * 1e3, packets_per_s=n / med,
                                    beams_per_s=4 * n / med, floor_bytes_per_record=4 * C * 4 + P.PACKET_SIZE,
                                    floor_share=n * (4 * C * 4 + P.PACKET_SIZE) / PEAK_BPS / med))
        if size == 4096:
            grid = world.grid_i8()
            cpu = {}
            for R in (1.2, 3.0):
                t0 = time.perf_counter()
                S.sense_ranges(grid, RES, -half, -half, poses[:64], max_range=R)
                dt = time.perf_counter() - t0
                cpu[str(R)] = dict(sweeps_per_s=64 / dt, beams_per_s=64 * P.SWEEP_BEAMS / dt)
            out["cpu_restatement"] = cpu
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    h = REGION_M / 2
    poses = np.stack([rng.uniform(-h, h, a.poses), rng.uniform(-h, h, a.poses), rng.uniform(-math.pi, math.pi, a.poses)],
                     axis=1).astype(np.float32)
    print(json.dumps(dict(metric="sense", poses=a.poses, reps=a.reps, region_m=REGION_M, peak_bps=PEAK_BPS,
                          gpu=[run(s, poses, a.reps) for s in (4096, 8192)])))


if __name__ == "__main__":
    main()
