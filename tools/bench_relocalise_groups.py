#!/usr/bin/env python3
"""Group relocalisation time: qs_relocalise_groups_device on ONE group of 1, 3, 5 and 8 sweeps sensed at 3.0 m, 0.25 m apart, in
the mapped 4096^2 grid of tools/bench_relocalise.py (the three-room world of tests/reloc_rules.py tiled 21 x 21), at the defaults
(R 2, 180 rotations), sweep filter (0.1, 3.0), travel 2.0 m.  Whole calls between HIP events on the mapper's stream, median of
--reps after a warm-up.  Prints one JSON line.

    python tools/bench_relocalise_groups.py [--reps 10] [--size 4096]

The floor is that of tools/bench_relocalise.py with the group's H: (FREE cells / 256) tiles' worth of waves, per rotation and per
hit point 4.5 LDS cycles, on 256 CUs at 2.4 GHz."""
import argparse
import json
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
import reloc_group_rules as GR  # noqa: E402
import reloc_rules as RR  # noqa: E402
from bench_relocalise import CLOCK_HZ, CUS, tiled_world  # noqa: E402

P = qa.protocol
SIZES = (1, 3, 5, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    res, travel = 0.05, 2.0
    half = a.size * res / 2
    geom = (res, -half, -half)
    grid = tiled_world(a.size)
    free = int((grid == 0).sum())
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream()
    out = dict(tool="bench_relocalise_groups", size=a.size, free_cells=free, reps=a.reps, travel=travel, cases=[])
    with qa.QuasarMapper(a.size, res, -half, -half) as m:
        MZ.paint(m, RR.paint_rays(grid), res, -half, -half)
        m.set_sweep_filter(RR.WORLD_SMIN, RR.WORLD_SMAX)
        poses, _ = RR.query_poses(grid, geom, 1, seed=1)
        G = GR.build_groups(grid, geom, poses, max(SIZES), 0.25, seed=1)[0]
        buf = m.sense_sweeps(G, 1, max_range=3.0)
        rel = P.reloc_rel(*G.T)
        d = torch.from_numpy(buf).to(dev)
        d_rel = torch.from_numpy(rel.view(np.float64).copy()).to(dev)
        d_out = torch.zeros(P.GROUP_RELOC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        m.set_stream(side.cuda_stream)
        prm = m.relocalise_params()
        for k in SIZES:
            call = lambda: m.relocalise_groups_device(d.data_ptr(), k, buf.shape[1], d_rel.data_ptr(), [k], d_out.data_ptr(),
                                                      travel=travel, params=prm)
            for _ in range(a.warmup):
                call()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                call()
                e1.record(side)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            r = d_out.cpu().numpy().view(P.GROUP_RELOC_DTYPE)[0]
            hits = int(r["hits"])
            floor_ms = (free / 256.0) * prm.n_rot * hits * 4.5 / (CUS * CLOCK_HZ) * 1e3
            med = float(np.median(ms))
            out["cases"].append(dict(group=k, ms_median=round(med, 3), ms_min=round(float(np.min(ms)), 3), ms_max=round(float(np.max(ms)), 3),
                                     hit_points=hits, records=int(r["records"]), lds_floor_ms=round(floor_ms, 3),
                                     floor_fraction=round(floor_ms / med, 3), accepted=int(r["accepted"]), status=int(r["status"])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
