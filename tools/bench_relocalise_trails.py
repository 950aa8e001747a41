#!/usr/bin/env python3
"""Trail relocalisation time: qs_relocalise_trails_device on ONE trail of 32 and of 64 packets, sensed on the device at 1.2 m and
at 3.0 m along a drive through the mapped 4096^2 grid of tools/bench_relocalise.py, at the defaults (R 2, 180 rotations).  The
travel is what the front-end would pass: the trail's own extent rounded up to 0.25 m, capped by rule K8.  Beside each case, in
the same run, qs_relocalise_groups_device on a group of two sweeps sensed at the trail's last poses with the same filter and
travel, its beams blanked down to the trail's number of hit points: the two calls share the scoring kernel and the patch, so
they should cost the same.  Whole calls between HIP events on the mapper's stream, median of --reps after a warm-up.  Prints one
JSON line.

    python tools/bench_relocalise_trails.py [--reps 10] [--size 4096]

The floor is that of tools/bench_relocalise.py with the trail's H: (FREE cells / 256) tiles' worth of waves, per rotation and per
hit point 4.5 LDS cycles, on 256 CUs at 2.4 GHz.  `fit_ms` is DESIGN 4.20's fit of the group call at travel 2.0 m, 0.119 ms a
point plus 10.6 ms, for comparison."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quasar_amd as qa  # noqa: E402
import maze_scenes as MZ  # noqa: E402
import reloc_rules as RR  # noqa: E402
import trail_reloc_rules as KR  # noqa: E402
from bench_relocalise import CLOCK_HZ, CUS, tiled_world  # noqa: E402

P = qa.protocol
MIN_DIST = 0.05


def timed(call, side, warmup, reps):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        call()
        e1.record(side)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms_median=round(float(np.median(ms)), 3), ms_min=round(float(np.min(ms)), 3), ms_max=round(float(np.max(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    res = 0.05
    half = a.size * res / 2
    geom = (res, -half, -half)
    grid = tiled_world(a.size)
    free = int((grid == 0).sum())
    rays = RR.paint_rays(grid)
    true = KR.drive(grid, geom, np.random.default_rng(1), 64).astype(np.float32)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream()
    out = dict(tool="bench_relocalise_trails", size=a.size, free_cells=free, reps=a.reps, cases=[])
    for far in (1.2, 3.0):
        with qa.QuasarMapper(a.size, res, -half, -half, min_dist=MIN_DIST, max_dist=far) as m:
            MZ.paint(m, rays, res, -half, -half)
            m.set_sweep_filter(0.1, far)
            pk = m.sense_packets(true, 1, max_range=far)
            sw = m.sense_sweeps(true[-2:], 1, max_range=far)
            prm = m.relocalise_params()
            d_pk = torch.from_numpy(pk).to(dev)
            d_out = torch.zeros(P.TRAIL_RELOC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_gout = torch.zeros(P.GROUP_RELOC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            rel = P.reloc_rel(*true[-2:].T, anchor=1)               # the last pose is the frame, as it is the trail's anchor
            d_rel = torch.from_numpy(rel.view(np.float64).copy()).to(dev)
            torch.cuda.synchronize()
            m.set_stream(side.cuda_stream)
            for K in (32, 64):
                q = true[64 - K:]
                extent = float(np.hypot(q[:, 0] - q[-1, 0], q[:, 1] - q[-1, 1]).max())
                cap = math.floor((115.5 * res - far) / 0.25) * 0.25      # K8 at R 2: ceil((max_dist + travel) / res) <= 116
                travel = min(math.ceil(extent / 0.25) * 0.25, cap)
                first = d_pk.data_ptr() + (64 - K) * 42
                t = timed(lambda: m.relocalise_trails_device(first, K, 42, [K], d_out.data_ptr(), travel=travel, params=prm),
                          side, a.warmup, a.reps)
                r = d_out.cpu().numpy().view(P.TRAIL_RELOC_DTYPE)[0]
                H = int(r["hits"])
                # the group beside it: two sweeps, the hit beams beyond the trail's H blanked
                g = sw.copy()
                left = H
                for k in range(len(g)):
                    rg = g[k, -724:].view("<f4")
                    hit = np.nonzero((rg.astype(np.float64) > 0.1) & (rg.astype(np.float64) <= far))[0]
                    rg[hit[left:]] = 0.0
                    left = max(left - len(hit), 0)
                d_sw = torch.from_numpy(g).to(dev)
                torch.cuda.synchronize()
                tg = timed(lambda: m.relocalise_groups_device(d_sw.data_ptr(), 2, g.shape[1], d_rel.data_ptr(), [2], d_gout.data_ptr(),
                                                              travel=travel, params=prm), side, a.warmup, a.reps)
                gr = d_gout.cpu().numpy().view(P.GROUP_RELOC_DTYPE)[0]
                floor_ms = (free / 256.0) * prm.n_rot * H * 4.5 / (CUS * CLOCK_HZ) * 1e3
                out["cases"].append(dict(filter_m=far, packets=K, travel=travel, hit_points=H, records=int(r["records"]),
                                         accepted=int(r["accepted"]), status=int(r["status"]), **t,
                                         lds_floor_ms=round(floor_ms, 3), floor_fraction=round(floor_ms / t["ms_median"], 3),
                                         fit_ms=round(0.119 * H + 10.6, 1), group_hit_points=int(gr["hits"]),
                                         group_ms_median=tg["ms_median"], group_ms_min=tg["ms_min"], group_ms_max=tg["ms_max"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
