#!/usr/bin/env python3
"""Sweep-check rate: qs_check_sweeps_device on 2^16 device-resident sweeps sensed from as many poses in a mapped world of 4096^2
cells of 5 cm, at R = 1.2 m and 3.0 m, beside qs_sense_ranges_device from the same poses and qs_ingest_sweeps_device of the same
records in the same run; and the guarded ingest (qs_ingest_sweeps_checked_device) beside check + plain ingest.  Every figure is
the median of --reps calls between two device events on the contexts' stream, after --warmup calls.  Prints one JSON line.

    python tools/bench_check_sweeps.py [--poses 65536] [--reps 10] [--warmup 2]

The world is tools/bench_sense.py's: a 40 m x 40 m floor with walls every 4 m.  The records are sensed at the true poses with
0.02 m of noise, and every fourth one then reports a pose 0.3 m off, so that the guarded ingest has something to withhold
(`withheld_share`).  The check walks the lines the sensing walks, over a patch packed to two bit planes instead of one: sensing's
time is the yardstick (`check_over_sense`).  The two ingests map into a second context that holds the same world, restored from a
checkpoint before every timed call, so that both see the map the records were sensed from."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quasar_amd as qa  # noqa: E402
from bench_sense import REGION_M, RES, paint_world  # noqa: E402

P = qa.protocol
SIZE = 4096


def timed(call, before, stream, reps, warmup):
    """Median and minimum, in ms, of `call` between two events on `stream`; `before` (untimed) runs ahead of every call."""
    ms = []
    for rep in range(warmup + reps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    n, stride = a.poses, P.PACKET_SIZE_V0_ODO
    rng = np.random.default_rng(1)
    h = REGION_M / 2
    poses = np.stack([rng.uniform(-h, h, n), rng.uniform(-h, h, n), rng.uniform(-math.pi, math.pi, n)], axis=1).astype(np.float32)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream()
    d_pose = torch.from_numpy(poses).to(dev)
    d_agent = torch.ones(n, dtype=torch.uint8, device=dev)
    d_pkts = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    d_ranges = torch.zeros(n * P.SWEEP_BEAMS, dtype=torch.float32, device=dev)
    d_out = torch.zeros(n * P.CHECK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    half = SIZE * RES / 2
    out = dict(metric="check_sweeps", size=SIZE, poses=n, reps=a.reps, warmup=a.warmup, runs=[])
    nothing = lambda: None
    with qa.QuasarMapper(SIZE, RES, -half, -half) as world, qa.QuasarMapper(SIZE, RES, -half, -half) as m:
        out["wall_cells"] = paint_world(world)
        for c in (world, m):
            c.set_stream(side.cuda_stream)
        for R in (1.2, 3.0):
            world.set_sweep_filter(0.02, R)
            ckpt = world.checkpoint()                                       # (a checkpoint carries the sweep filter)
            restore = lambda: m.restore(ckpt)
            world.sense_sweeps_device(d_pose, d_agent, n, d_pkts, stride, max_range=R, noise_amp=0.02, seed=7)
            world.sync()
            buf = d_pkts.cpu().numpy().reshape(n, stride)
            x = np.ascontiguousarray(buf[:, 5:9]).view("<f4")
            x[::4] += np.float32(0.3)                                       # every fourth bot is lost by 0.3 m
            buf[:, 5:9] = x.view(np.uint8)
            d_pkts.copy_(torch.from_numpy(buf.reshape(-1)))
            torch.cuda.synchronize()
            sense = timed(lambda: world.sense_ranges_device(d_pose, n, d_ranges, max_range=R), nothing, side, a.reps, a.warmup)
            check = timed(lambda: world.check_sweeps_device(d_pkts.data_ptr(), n, stride, d_out.data_ptr()), nothing, side, a.reps, a.warmup)
            ck = d_out.cpu().numpy().view(P.CHECK_DTYPE)
            plain = timed(lambda: m.ingest_sweeps_device(d_pkts.data_ptr(), n, stride), restore, side, a.reps, a.warmup)
            guarded = timed(lambda: m.ingest_sweeps_checked_device(d_pkts.data_ptr(), n, stride), restore, side, a.reps, a.warmup)
            assert m.last_sweep_checks().tobytes() == ck.tobytes()
            out["runs"].append(dict(
                max_range=R, C=math.ceil(R / RES) + 1,
                sense_ms_median=sense[0], sense_ms_min=sense[1], check_ms_median=check[0], check_ms_min=check[1],
                check_sweeps_per_s=n / check[0] * 1e3, check_over_sense=check[0] / sense[0],
                ingest_ms_median=plain[0], ingest_ms_min=plain[1], guarded_ms_median=guarded[0], guarded_ms_min=guarded[1],
                guarded_over_check_plus_ingest=guarded[0] / (check[0] + plain[0]),
                withheld_share=float((ck["status"] == P.CHECK_CONTRADICTS).mean()),
                undecided_share=float((ck["status"] == P.CHECK_UNDECIDED).mean()),
                checked_beams_share=float(ck["checked"].sum() / (n * P.SWEEP_BEAMS))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
