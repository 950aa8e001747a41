#!/usr/bin/env python3
"""Servo-sweep ingest rate: qs_ingest_sweeps_device on a 2^16-sweep batch (751-byte records, device-resident), at 4096^2 and
8192^2 cells of 5 cm, and the CPU oracle's update_ray rate on the same beams beside it.  Prints one JSON line.

    python tools/bench_sweeps.py [--sweeps 65536] [--reps 10]

Algorithmic bytes per sweep (HBM, the kernels' own traffic, grid merge excluded): the record (751 B) read once, 184 ray
slots (8 B) written by pass A and read by pass C, 184 hit flags written and read, and ~1.4 tile records (8 B) per beam
written by pass C and read by pass D."""
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
import quasar_amd as qa  # noqa: E402
from oracle import oracle as orc  # noqa: E402

P = qa.protocol
PEAK_BPS = 8.0e12
REC_PER_BEAM = 1.4


def sweeps(n, seed, half):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.05, 1.6, (n, P.SWEEP_BEAMS)).astype(np.float32)
    return P.pack_sweeps(rng.integers(1, 3, n), rng.uniform(-half, half, n), rng.uniform(-half, half, n),
                         rng.uniform(-math.pi, math.pi, n), r, odometry=True)


def bytes_per_sweep():
    return P.PACKET_SIZE_V0_ODO + 184 * 8 * 2 + 184 * 2 + P.SWEEP_BEAMS * REC_PER_BEAM * 8 * 2


def gpu_rate(size, buf, reps):
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(buf).to(dev)
    torch.cuda.synchronize()
    n, stride = buf.shape
    half = size * 0.05 / 2
    with qa.QuasarMapper(size, 0.05, -half, -half, raycast_mode=0) as m:
        m.ingest_sweeps_device(d.data_ptr(), n, stride)
        m.sync()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            m.ingest_sweeps_device(d.data_ptr(), n, stride)
            m.sync()
            t.append(time.perf_counter() - t0)
        c = m.counters()
    med = float(np.median(t))
    return dict(size=size, sweeps_per_s=n / med, rays_per_s=n * P.SWEEP_BEAMS / med, ms_median=med * 1e3,
                ms_min=min(t) * 1e3, edge_rays=c["edge_rays"], peak_fraction=n * bytes_per_sweep() / med / PEAK_BPS)


def cpu_rate(buf, n=256):
    rec = buf[:n].view(P.PACKET_DTYPE_V0_ODO).reshape(-1)
    rx, ry, hx, hy, v = [], [], [], [], []
    for r in rec:
        x, y, yaw = float(r["x"]), float(r["y"]), float(r["yaw"])
        for i, d in enumerate(r["ranges"].tolist()):
            a = yaw + math.radians(i - 90)
            ok = 0.1 < d <= 1.2
            L = d if ok else (min(d, 1.2) if d > 0.1 else 1.2)
            rx.append(x); ry.append(y); hx.append(x + L * math.cos(a)); hy.append(y + L * math.sin(a)); v.append(ok)
    o = orc.OracleMapper(4096, 0.05, -102.4, -102.4)
    t0 = time.perf_counter()
    o.update_rays(np.array(rx), np.array(ry), np.array(hx), np.array(hy), np.array(v, np.uint8))
    dt = time.perf_counter() - t0
    return dict(sweeps_per_s=n / dt, rays_per_s=n * P.SWEEP_BEAMS / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    buf = sweeps(a.sweeps, 1, 20.0)
    out = dict(metric="sweep_ingest", sweeps=a.sweeps, stride=P.PACKET_SIZE_V0_ODO, region_m=40.0,
               bytes_per_sweep=bytes_per_sweep(), gpu=[gpu_rate(s, buf, a.reps) for s in (4096, 8192)],
               cpu_oracle=cpu_rate(buf))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
