#!/usr/bin/env python3
"""What the bot veil costs: HIP events round whole qs_ingest_device calls of 2^20 packets (device-resident), the median of
--reps after warm-up, on the 64-bot stream of bench.py's configs[3] shape (every bot its own generator run in its own room
tile, one pose graph per two bots).  Prints one JSON line per case.

    python tools/bench_bot_veil.py [--batch 1048576] [--reps 10] [--ab other/libquasar_slam.so] [--rounds 3]

  off     veil off, 4096^2.  With --ab: this library and the other one (a build of the parent commit) alternate --rounds times,
          a fresh process each; the claim to support is overlapping ranges (the veil-off path differs by one host branch)
  on      veil radius 3, 4096^2 / 64 bots and 8192^2 / 255 bots: the whole call, and from a second pass with stage timing on the
          veil stage's own time (qs_bot_veil_time) beside the same run's decode and raycast stages; rays veiled per call
  small   20 packets, veil on (the tiled form) against veil off (the direct kernel): what the live UDP path pays

A library without the veil's entry points (the parent's) runs the `off` case only."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys

import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quasar_amd as qa  # noqa: E402

_lib = importlib.import_module(qa.__name__ + "._lib")
replay = importlib.import_module(qa.__name__ + ".replay")
HAS_VEIL = hasattr(ctypes.CDLL(_lib.LIB_PATH), "qs_set_bot_veil")
if not HAS_VEIL:                                        # an older build of the same ABI: declare only what it has
    for k in [k for k in _lib.SIGNATURES if "veil" in k]:
        del _lib.SIGNATURES[k]


def timed(m, side, d, n, reps, warm=3):
    """ms of `reps` whole ingest calls, by events on the context's stream."""
    out = []
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        m.ingest_device(d.data_ptr(), n, qa.protocol.PACKET_SIZE)
        e1.record(side)
        side.synchronize()
        if k >= warm:
            out.append(e0.elapsed_time(e1))
    return out


def case(size, bots, batch, reps, radius, stages=False):
    dev = torch.device("cuda", 0)
    half = size * 0.05 / 2
    stream = replay.multi_bot_stream(None, bots, batch, origin=(-half + 4.4, -half + 4.4))
    d = torch.from_numpy(stream).to(dev)
    side = torch.cuda.Stream(dev)
    out = {}
    with qa.QuasarMapper(size, 0.05, -half, -half, max_agent=bots, bots_per_graph=2, device=0) as m:
        m.set_stream(side.cuda_stream)
        if radius:
            m.set_bot_veil(radius)
        t = timed(m, side, d, batch, reps)
        out.update(ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t))
        if radius:
            v0 = m.bot_veil_stats()
            m.ingest_device(d.data_ptr(), batch, qa.protocol.PACKET_SIZE)
            out["veiled_per_call"] = m.bot_veil_stats() - v0
        if stages:
            m.timing_enable(True)
            m.stage_times(reset=True)
            if radius:
                m.bot_veil_time(reset=True)
            for _ in range(reps):
                m.ingest_device(d.data_ptr(), batch, qa.protocol.PACKET_SIZE)
            st = m.stage_times(reset=True)
            out["stage_ms_per_call"] = {k: st[k][0] / reps for k in ("decode", "slam", "raycast", "rc_rays", "rc_sort", "rc_raster")}
            if radius:
                out["stage_ms_per_call"]["veil"] = m.bot_veil_time()[0] / reps
    return out


def child(lib, batch, reps):
    env = dict(os.environ)
    if lib:
        env["QUASAR_SLAM_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "off", "--batch", str(batch), "--reps", str(reps)],
                       env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ab", default=None, help="another build of the library (the parent commit's) for the veil-off comparison")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("off", "on", "small"))
    a = ap.parse_args()
    if a.only == "off":
        print(json.dumps(dict(metric="bot_veil_off", size=4096, bots=64,
                              batch=a.batch, **case(4096, 64, a.batch, a.reps, 0))), flush=True)
        return
    if a.ab and a.only is None:
        for rnd in range(a.rounds):                     # fresh processes, alternating, before this one touches the GPU
            for name, lib in (("this", None), ("other", a.ab)):
                r = child(lib, a.batch, a.reps)
                print(json.dumps(dict(r, metric="bot_veil_off_ab", round=rnd, lib=name)), flush=True)
    if not HAS_VEIL:
        return
    if a.only in (None, "on"):
        for size, bots in ((4096, 64), (8192, 255)):
            print(json.dumps(dict(metric="bot_veil_on", size=size, bots=bots, batch=a.batch, radius=3,
                                  on=case(size, bots, a.batch, a.reps, 3, stages=True),
                                  off=case(size, bots, a.batch, a.reps, 0, stages=True))), flush=True)
    if a.only in (None, "small"):
        print(json.dumps(dict(metric="bot_veil_small", size=4096, bots=64, batch=20, on=case(4096, 64, 20, 50, 3),
                              off=case(4096, 64, 20, 50, 0))), flush=True)


if __name__ == "__main__":
    main()
