#!/usr/bin/env python3
"""Sweep matching rate: qs_match_sweeps_device on a 2^16-sweep batch (751-byte records, device-resident, uniform poses in
a region mapped from sweeps of the same kind), at the default window (R 2, W 6, T 10) and at W 4 / T 5, on 4096^2 and
8192^2 cells of 5 cm; the matched ingest beside the plain ingest in the same run; and the CPU restatement's rate
(tests/match_rules.py, numpy) on a subset.  Median of --reps calls after a warm-up, qs_sync inside the timed span.
Prints one JSON line.

    python tools/bench_match_sweeps.py [--sweeps 65536] [--reps 10]

Candidate look-ups of a sweep: hit beams x (2 W + 1)^2 x (2 T + 1).  The LDS floor the rate is held against is that of the
form csrc/match.hip builds (a lane per rotation, iy and FOUR adjacent ix): per wave and per four beams one 8-byte read of
four patch offsets and eight dword reads of the field, 2 LDS cycles each = 4.5 cycles per beam, over
(2 T + 1) (2 W + 1) ceil((2 W + 1) / 4) / 64 waves' worth of lanes, on 256 CUs at 2.4 GHz."""
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
import match_rules as MR  # noqa: E402

P = qa.protocol
CUS, CLOCK_HZ = 256, 2.4e9
CONFIGS = (("default", dict()), ("w4_t5", dict(window=4, angle_steps=5)))


def sweeps(n, seed, half):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.05, 1.6, (n, P.SWEEP_BEAMS)).astype(np.float32)
    return P.pack_sweeps(rng.integers(1, 3, n), rng.uniform(-half, half, n), rng.uniform(-half, half, n),
                         rng.uniform(-math.pi, math.pi, n), r, odometry=True)


def lds_floor_cycles(hit_beams, W, T):
    ny = 2 * W + 1
    return (2 * T + 1) * ny * ((ny + 3) // 4) / 64.0 * hit_beams * 4.5


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


def gpu_rates(size, buf, reps):
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(buf).to(dev)
    n, stride = buf.shape
    d_out = torch.zeros(n * P.MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    half = size * 0.05 / 2
    out = dict(size=size, match=[])
    with qa.QuasarMapper(size, 0.05, -half, -half, raycast_mode=0) as m:
        m.ingest_sweeps_device(d.data_ptr(), n, stride)          # the mapped region
        m.sync()
        for name, prm in CONFIGS:
            p = m.match_params(prm)
            med, best = timed(lambda: m.match_sweeps_device(d.data_ptr(), n, stride, d_out.data_ptr(), params=p), m, reps)
            res = d_out.cpu().numpy().view(P.MATCH_DTYPE)
            hits = float(res["hits"].mean())
            lookups = float(res["hits"].sum()) * (2 * p.window + 1) ** 2 * (2 * p.angle_steps + 1)
            floor_s = n * lds_floor_cycles(hits, p.window, p.angle_steps) / (CUS * CLOCK_HZ)
            out["match"].append(dict(config=name, radius=p.radius, window=p.window, angle_steps=p.angle_steps,
                                     sweeps_per_s=n / med, lookups_per_s=lookups / med, ms_median=med * 1e3, ms_min=best * 1e3,
                                     hit_beams_mean=hits, accepted_matches=int(res["accepted_match"].sum()),
                                     lds_floor_ms=floor_s * 1e3, lds_floor_fraction=floor_s / med))
        plain, _ = timed(lambda: m.ingest_sweeps_device(d.data_ptr(), n, stride), m, reps)
        matched, _ = timed(lambda: m.ingest_sweeps_matched_device(d.data_ptr(), n, stride), m, reps)
        out["ingest"] = dict(plain_ms=plain * 1e3, matched_ms=matched * 1e3, plain_sweeps_per_s=n / plain,
                             matched_sweeps_per_s=n / matched,
                             match_plus_plain_ms=out["match"][0]["ms_median"] + plain * 1e3)
    return out


def cpu_rate(buf, n=8):
    """The restatement on n sweeps against a 4096^2 map drawn by the GPU from the same batch (the field is not timed)."""
    half = 4096 * 0.05 / 2
    with qa.QuasarMapper(4096, 0.05, -half, -half) as m:
        m.ingest_sweeps(buf[:4096])
        grid = m.grid_i8()
    p = MR.params()
    L = MR.field(grid, p["radius"])
    recs = MR.records_of(buf[:n])
    acc, pose = MR.poses_of(recs)
    t0 = time.perf_counter()
    hits = 0
    for k in range(n):
        hits += MR.match_one(L, (0.05, -half, -half), pose[k], recs["ranges"][k], p, 0.1, 1.2)["hits"]
    dt = time.perf_counter() - t0
    return dict(sweeps=n, sweeps_per_s=n / dt, lookups_per_s=hits * 13 * 13 * 21 / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    buf = sweeps(a.sweeps, 1, 20.0)
    out = dict(metric="sweep_match", sweeps=a.sweeps, stride=P.PACKET_SIZE_V0_ODO, region_m=40.0,
               gpu=[gpu_rates(s, buf, a.reps) for s in (4096, 8192)], cpu_restatement=cpu_rate(buf))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
