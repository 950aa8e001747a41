#!/usr/bin/env python3
"""Relocalisation time: qs_relocalise_sweeps_device on 1, 8 and 64 sweeps sensed at 3.0 m in a mapped 4096^2 grid of 5 cm (the
three-room world of tests/reloc_rules.py tiled 21 x 21), at the defaults (R 2, 180 rotations), sweep filter (0.1, 3.0).  Whole
calls between HIP events on the mapper's stream, median of --reps after a warm-up.  Prints one JSON line.

    python tools/bench_relocalise.py [--reps 10] [--size 4096]

The floor the time is held against is that of the form csrc/reloc.hip builds (a wave per rotation scores a 16 x 16 tile, a lane
four adjacent cells): per FREE cell / 256 tiles' worth of waves, per rotation and per hit beam 4.5 LDS cycles, on 256 CUs at
2.4 GHz.  Tiles are scored whole, so the cells of the launched tiles are reported beside the FREE cells searched."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quasar_amd as qa  # noqa: E402
import maze_scenes as MZ  # noqa: E402
import reloc_rules as RR  # noqa: E402

P = qa.protocol
CUS, CLOCK_HZ = 256, 2.4e9


def tiled_world(size):
    w = RR.world()
    g = np.full((size, size), -1, dtype=np.int8)
    k = size // len(w)
    g[:k * len(w), :k * len(w)] = np.tile(w, (k, k))
    return g


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
    tiles = int((grid == 0).reshape(a.size // 16, 16, a.size // 16, 16).any(axis=(1, 3)).sum())
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream()
    out = dict(tool="bench_relocalise", size=a.size, free_cells=free, tiles_launched=tiles, reps=a.reps, cases=[])
    with qa.QuasarMapper(a.size, res, -half, -half) as m:
        MZ.paint(m, RR.paint_rays(grid), res, -half, -half)
        m.set_sweep_filter(RR.WORLD_SMIN, RR.WORLD_SMAX)
        poses, _ = RR.query_poses(grid, geom, 64, seed=1)
        buf = m.sense_sweeps(poses, 1, max_range=3.0)
        d = torch.from_numpy(buf).to(dev)
        d_out = torch.zeros(64 * P.RELOC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        m.set_stream(side.cuda_stream)
        prm = m.relocalise_params()
        for n in (1, 8, 64):
            call = lambda: m.relocalise_sweeps_device(d.data_ptr(), n, buf.shape[1], d_out.data_ptr(), params=prm)
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
            r = d_out.cpu().numpy().view(P.RELOC_DTYPE)[:n]
            hits = float(r["hits"].mean())
            floor_ms = n * (free / 256.0) * prm.n_rot * hits * 4.5 / (CUS * CLOCK_HZ) * 1e3
            med = float(np.median(ms))
            out["cases"].append(dict(sweeps=n, ms_median=round(med, 3), ms_min=round(float(np.min(ms)), 3),
                                     ms_per_sweep=round(med / n, 3), hit_beams_mean=round(hits, 1),
                                     lds_floor_ms=round(floor_ms, 3), floor_fraction=round(floor_ms / med, 3),
                                     accepted=int(r["accepted"].sum()), status_ok=int((r["status"] == 0).sum())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
