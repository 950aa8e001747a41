#!/usr/bin/env python3
"""What the bot veil for sweeps costs (include/quasar_slam.h, rules S0-S8): HIP events round whole qs_ingest_sweeps_device calls
of 2^16 device-resident sweeps (751-byte records) at 4096^2 cells of 5 cm, the median of --reps after 3 warm-up calls.  Prints
one JSON line per case.

    python tools/bench_sweep_veil.py [--sweeps 65536] [--reps 10] [--ab other/libquasar_slam.so] [--rounds 3] [--only CASE]

  off      the switch off.  With --ab: this library and the other one (a build of the parent commit) alternate --rounds times, a
           fresh process each; the claim to support is overlapping ranges.  packets_on is run the same way (2^20 packets, packet
           veil radius 3): the packet stage shares its scan over blocks with the sweep stage
  look     the veil acting (radius 3) against the switch off in the same process, sweep filter 1.2 m and 3.0 m, 64 and 255 bots on
           a lattice (5 m / 2.5 m apart, each jittering about its own place): whole calls, the stage's own time
           (qs_bot_veil_time) beside the raycast's stages, beams veiled per call, and the stage against its floor -- 184 slots x
           (8 B ray + 1 B flag read + 1 B flag written) per sweep over the device-to-device copy rate this run measures
  room     a case that veils something: tests/sweep_veil_rules.py's room of four sweep bots that face each other, sensed through
           sim.body_sweep_ranges, 64 rounds in one call: beams veiled per call, and the phantom cells (OCCUPIED in the mapper,
           FREE in the world) with the veil on and off

A library without the sweep veil's entry points (the parent's) runs `off` and `packets_on` only."""
import argparse
import ctypes
import importlib
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np
import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quasar_amd as qa  # noqa: E402

_lib = importlib.import_module(qa.__name__ + "._lib")
replay = importlib.import_module(qa.__name__ + ".replay")
sim = importlib.import_module(qa.__name__ + ".sim")
P = qa.protocol
HAS = hasattr(ctypes.CDLL(_lib.LIB_PATH), "qs_set_bot_veil_sweeps")
if not HAS:                                             # an older build of the same ABI: declare only what it has
    for k in ("qs_set_bot_veil_sweeps", "qs_bot_veil_sweeps", "qs_last_sweeps_veiled"):
        _lib.SIGNATURES.pop(k, None)
STAGE_BYTES = 184 * (8 + 1 + 1)                         # per sweep: what the form built must move when it reads the rays


def lattice_sweeps(n, bots, smax, seed=1):
    """n sweeps of `bots` bots in turn, each jittering 0.5 m about its own lattice place; ranges uniform up to 1.3 smax."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(bots)))
    pitch = 40.0 / side
    agent = 1 + np.arange(n) % bots
    gx, gy = (agent - 1) % side, (agent - 1) // side
    x = (gx + 0.5) * pitch - 20.0 + rng.uniform(-0.5, 0.5, n)
    y = (gy + 0.5) * pitch - 20.0 + rng.uniform(-0.5, 0.5, n)
    r = rng.uniform(0.05, 1.3 * smax, (n, P.SWEEP_BEAMS)).astype(np.float32)
    return P.pack_sweeps(agent, x, y, rng.uniform(-math.pi, math.pi, n), r, odometry=True)


def timed(call, side, reps, warm=3):
    out = []
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        call()
        e1.record(side)
        side.synchronize()
        if k >= warm:
            out.append(e0.elapsed_time(e1))
    return dict(ms_median=statistics.median(out), ms_min=min(out), ms_max=max(out))


def sweep_case(buf, bots, smax, reps, radius, stages=False, size=4096):
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(buf).to(dev)
    side = torch.cuda.Stream(dev)
    n, stride = buf.shape
    half = size * 0.05 / 2
    with qa.QuasarMapper(size, 0.05, -half, -half, max_agent=bots, device=0) as m:
        m.set_stream(side.cuda_stream)
        m.set_sweep_filter(0.1, smax)
        if radius:
            m.set_bot_veil(radius, sweeps=True)
        call = lambda: m.ingest_sweeps_device(d.data_ptr(), n, stride)
        out = timed(call, side, reps)
        if radius:
            v0 = m.bot_veil_stats()
            call()
            out["veiled_per_call"] = m.bot_veil_stats() - v0
        if stages:
            m.timing_enable(True)
            m.stage_times(reset=True)
            if radius:
                m.bot_veil_time(reset=True)
            for _ in range(reps):
                call()
            st = m.stage_times(reset=True)
            out["stage_ms_per_call"] = {k: st[k][0] / reps for k in ("raycast", "rc_rays", "rc_sort", "rc_raster")}
            if radius:
                out["stage_ms_per_call"]["veil"] = m.bot_veil_time()[0] / reps
        out["edge_rays"] = m.counters()["edge_rays"]
    return out


def packets_case(batch, reps):
    dev = torch.device("cuda", 0)
    half = 4096 * 0.05 / 2
    stream = replay.multi_bot_stream(None, 64, batch, origin=(-half + 4.4, -half + 4.4))
    d = torch.from_numpy(stream).to(dev)
    side = torch.cuda.Stream(dev)
    with qa.QuasarMapper(4096, 0.05, -half, -half, max_agent=64, bots_per_graph=2, device=0) as m:
        m.set_stream(side.cuda_stream)
        m.set_bot_veil(3)
        return timed(lambda: m.ingest_device(d.data_ptr(), batch, P.PACKET_SIZE), side, reps)


def copy_rate():
    """GB/s of a device-to-device copy of 256 MiB (read + write counted), the median of 10."""
    a = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    t = []
    for k in range(13):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if k >= 3:
            t.append(e0.elapsed_time(e1))
    return 2 * a.numel() / (statistics.median(t) * 1e-3) / 1e9


def room_case(rounds=64):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import sweep_veil_rules as sv
    g = sv.geo()
    world = sv.room_world()
    body = sv.ROOM_BODY * g.res
    buf = sv.room_stream(lambda pose, agent, ranges: sim.body_sweep_ranges(pose, agent, ranges, body, P.SWEEP_MAX_DIST_M), rounds=rounds)
    out = dict(sweeps=len(buf), bots=4, body_cells=sv.ROOM_BODY, radius=sv.ROOM_RADIUS)
    for key, radius in (("off", 0), ("on", sv.ROOM_RADIUS)):
        with qa.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=4) as m:
            if radius:
                m.set_bot_veil(radius, sweeps=True)
            m.ingest_sweeps(buf)
            grid = m.grid_i8()
            out[key] = dict(veiled_per_call=int(m.bot_veil_stats()), phantoms=int(((grid == 100) & (world == 0)).sum()),
                            walls=int(((grid == 100) & (world == 100)).sum()))
    return out


def child(lib, case, a):
    env = dict(os.environ)
    if lib:
        env["QUASAR_SLAM_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", case, "--sweeps", str(a.sweeps), "--reps", str(a.reps),
                        "--packets", str(a.packets)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=1 << 16)
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ab", default=None, help="another build of the library (the parent commit's) for the switch-off comparison")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("off", "packets_on", "look", "look1", "room"))
    a = ap.parse_args()
    if a.only == "off":
        print(json.dumps(dict(metric="sweep_veil_off", size=4096, bots=64, sweeps=a.sweeps,
                              **sweep_case(lattice_sweeps(a.sweeps, 64, 1.2), 64, 1.2, a.reps, 0))), flush=True)
        return
    if a.only == "packets_on":
        print(json.dumps(dict(metric="packet_veil_on", size=4096, bots=64, batch=a.packets, **packets_case(a.packets, a.reps))), flush=True)
        return
    if a.only == "look1":                               # one case alone, for a kernel trace
        print(json.dumps(dict(metric="sweep_veil_look1", **sweep_case(lattice_sweeps(a.sweeps, 255, 3.0), 255, 3.0, a.reps, 3))), flush=True)
        return
    if a.ab and a.only is None:
        for case in ("off", "packets_on"):              # fresh processes, alternating, before this one touches the GPU
            for rnd in range(a.rounds):
                for name, lib in (("this", None), ("other", a.ab)):
                    print(json.dumps(dict(child(lib, case, a), round=rnd, lib=name)), flush=True)
    if not HAS:
        return
    if a.only in (None, "look"):
        rate = copy_rate()
        floor_ms = a.sweeps * STAGE_BYTES / (rate * 1e9) * 1e3
        for smax in (1.2, 3.0):
            for bots in (64, 255):
                buf = lattice_sweeps(a.sweeps, bots, smax)
                on = sweep_case(buf, bots, smax, a.reps, 3, stages=True)
                off = sweep_case(buf, bots, smax, a.reps, 0, stages=True)
                veil = on["stage_ms_per_call"]["veil"]
                print(json.dumps(dict(metric="sweep_veil_look", size=4096, sweeps=a.sweeps, smax=smax, bots=bots, radius=3, on=on, off=off,
                                      copy_gb_s=rate, floor_ms=floor_ms, stage_over_floor=veil / floor_ms)), flush=True)
    if a.only in (None, "room"):
        print(json.dumps(dict(metric="sweep_veil_room", **room_case())), flush=True)


if __name__ == "__main__":
    main()
