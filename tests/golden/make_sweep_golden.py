#!/usr/bin/env python3
"""Golden vectors of the servo-sweep path.  RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).

Loads the reference as make_golden.py does, takes ~200 poses of session_telemetry.csv, computes 181 ranges per pose with
the generator's own cast_ray (simulation_tools/generate_fake_dual_session.py:83-90) at angle yaw + math.radians(i - 90), and
plants seeded NaN / 0 / 0.07 / 1.2 / 1.25 / 2.5 values.  Every pose is packed as a 743-byte v0 and a 751-byte v0 + odometry
record (same content; a few with a bad magic or agent), and the reference's OccupancyGrid.update_ray is driven beam by beam
with the sweep rule of include/quasar_slam.h (generate_topdown_map.py:39-57: hit when 0.1 < d <= 1.2, else a free ray of
min(d, 1.2) if d > 0.1 else 1.2), bot 2 offset by the separation.

    python tests/golden/make_sweep_golden.py      -> tests/golden/sweeps_512.npz
"""
import csv
import math
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402

SIZE, RES, OX, OY, SEP = 512, 0.05, -12.8, -12.8, 0.5
SMIN, SMAX = 0.1, 1.2
FMT_V0, FMT_ODO = "<4sBfffH181f", "<4sBfffiIH181f"


def f32(v):
    return struct.unpack("<f", struct.pack("<f", v))[0]


def main():
    mapper, gen = load_reference()
    with open(os.path.join(HERE, "session_telemetry.csv"), newline="") as f:
        rows = list(csv.DictReader(f))[::3][:200]
    rng = np.random.default_rng(2026)
    n = len(rows)
    agent = np.array([int(r["agent"]) for r in rows], dtype=np.int64)
    x = np.array([f32(float(r["x"])) for r in rows])
    y = np.array([f32(float(r["y"])) for r in rows])
    yaw = np.array([f32(math.radians(float(r["yaw_deg"]))) for r in rows])
    ranges = np.zeros((n, 181), dtype=np.float32)
    for k in range(n):
        for i in range(181):
            ranges[k, i] = gen.cast_ray(float(x[k]), float(y[k]), float(yaw[k]) + math.radians(i - 90))
    special = np.array([np.nan, 0.0, 0.07, 1.2, 1.25, 2.5], dtype=np.float32)
    mask = rng.random((n, 181)) < 0.06
    ranges[mask] = special[rng.integers(0, len(special), int(mask.sum()))]
    magic = [b"QSRL"] * n
    for k in rng.choice(n, 4, replace=False):
        magic[k] = b"QSRX"
    agent_w = agent.copy()
    bad_agents = rng.choice(n, 6, replace=False)
    agent_w[bad_agents[:3]] = 0
    agent_w[bad_agents[3:]] = 3
    v0 = np.zeros((n, 743), dtype=np.uint8)
    odo = np.zeros((n, 751), dtype=np.uint8)
    for k in range(n):
        rk = [float(v) for v in ranges[k]]
        v0[k] = np.frombuffer(struct.pack(FMT_V0, magic[k], int(agent_w[k]), x[k], y[k], yaw[k], 181, *rk), np.uint8)
        odo[k] = np.frombuffer(struct.pack(FMT_ODO, magic[k], int(agent_w[k]), x[k], y[k], yaw[k], 1000 + k, 500, 181, *rk),
                               np.uint8)
    grid = mapper.OccupancyGrid(SIZE, RES, OX, OY)
    hits = np.zeros((SIZE, SIZE), dtype=np.int32)
    misses = np.zeros((SIZE, SIZE), dtype=np.int32)
    accepted = np.zeros(n, dtype=np.uint8)
    for k in range(n):
        if magic[k] != b"QSRL" or not 1 <= agent_w[k] <= 2:
            continue
        accepted[k] = 1
        rx = float(x[k]) + (SEP if agent_w[k] == 2 else 0.0) + 0.0      # offset, then drift (none here)
        ry = float(y[k]) + 0.0
        for i in range(181):
            d = float(ranges[k, i])
            a = float(yaw[k]) + math.radians(i - 90)
            valid = SMIN < d <= SMAX
            rng_m = d if valid else (min(d, SMAX) if d > SMIN else SMAX)
            ex, ey = rx + rng_m * math.cos(a), ry + rng_m * math.sin(a)
            grid.update_ray(rx, ry, ex, ey, valid)
            x0, y0 = grid.world_to_grid(rx, ry)
            x1, y1 = grid.world_to_grid(ex, ey)
            cells = grid._bresenham(x0, y0, x1, y1)
            for gx, gy in cells[:-1]:
                if grid.in_bounds(gx, gy):
                    misses[gy, gx] += 1
            if valid and grid.in_bounds(*cells[-1]):
                hits[cells[-1][1], cells[-1][0]] += 1
    out = os.path.join(HERE, "sweeps_512.npz")
    np.savez_compressed(out, cfg=np.array([SIZE, RES, OX, OY, SEP]), sweeps_v0=v0, sweeps_odo=odo, accepted=accepted,
                        grid=grid.grid, hits=hits.astype(np.uint16), misses=misses.astype(np.uint16))
    print(f"{out}: {n} sweeps, {int(accepted.sum())} accepted, {int((grid.grid == 100).sum())} occupied, "
          f"{int((grid.grid == 0).sum())} free, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
