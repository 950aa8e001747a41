#!/usr/bin/env python3
"""Servo-sweep ingest rate: qs_ingest_sweeps_device on a 2^16-sweep batch (751-byte records, device-resident), at 4096^2 and
8192^2 cells of 5 cm, and the CPU oracle's update_ray rate on the same beams beside it.  Prints one JSON line.

    python tools/bench_sweeps.py [--sweeps 65536] [--reps 10] [--graph]

--graph adds a second JSON line, metric "sweep_graph": the same call on the same buffer and on the room stream of
tests/sweep_graph_rules.py scaled to 64 bots x 1024 sweeps (32 rooms of two bots, a pose graph each), with graph mode
(qs_set_sweep_graph) off and on, alternating, the map reset before every timed call; beside the times the share of sweeps with
a signature other than NONE (the loop-closure chain's cost follows it) and the QS_STAGE_DECODE / QS_STAGE_SLAM shares of a
graph-mode call.  On a build without graph mode only the "off" figures are printed.

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


def room_sweeps(bots=64, per_bot=1024):
    """The two-bot room stream, 10 laps cut to per_bot sweeps per bot, repeated in bots / 2 rooms 10 m apart (bots 2 r + 1 and
    2 r + 2 in room r), interleaved bot by bot: uint8 [bots * per_bot, 751]."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sweep_graph_rules as R
    agent, x, y, yaw, ranges = R.room_stream(laps=(per_bot + 103) // 104)
    agent, x, y, yaw, ranges = (v[:2 * per_bot] for v in (agent, x, y, yaw, ranges))
    rooms = bots // 2
    A, X, Y, W, RR = [], [], [], [], []
    for j in range(per_bot):
        for r in range(rooms):
            for b in range(2):
                k = 2 * j + b
                A.append(2 * r + int(agent[k])); X.append(float(x[k]) + 10.0 * (r % 8) - 40.0); Y.append(float(y[k]) + 10.0 * (r // 8) - 20.0)
                W.append(yaw[k]); RR.append(k)
    return P.pack_sweeps(np.array(A), np.array(X), np.array(Y), np.array(W), ranges[np.array(RR)], odometry=True)


def graph_rate(size, buf, reps, max_agent, bots_per_graph):
    """qs_ingest_sweeps_device with graph mode off and on, alternating, from an empty map each time."""
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(buf).to(dev)
    torch.cuda.synchronize()
    n, stride = buf.shape
    half = size * 0.05 / 2
    out = dict(size=size, sweeps=n, max_agent=max_agent, bots_per_graph=bots_per_graph)
    with qa.QuasarMapper(size, 0.05, -half, -half, raycast_mode=0, max_agent=max_agent, bots_per_graph=bots_per_graph) as m:
        has = hasattr(m, "set_sweep_graph")
        modes = (False, True) if has else (False,)
        t = {on: [] for on in modes}
        for rep in range(reps + 1):                         # (the first round warms up)
            for on in modes:
                if has:
                    m.set_sweep_graph(on)
                m.reset()
                m.sync()
                t0 = time.perf_counter()
                m.ingest_sweeps_device(d.data_ptr(), n, stride)
                m.sync()
                if rep:
                    t[on].append(time.perf_counter() - t0)
        for on in modes:
            key = "on" if on else "off"
            out[key + "_ms_median"] = float(np.median(t[on])) * 1e3
            out[key + "_ms_min"] = min(t[on]) * 1e3
            out[key + "_ms_max"] = max(t[on]) * 1e3
        if has:
            out["on_over_off"] = out["on_ms_median"] / out["off_ms_median"]
            _, lm = m.last_sweep_nodes()
            out["non_none_share"] = float(((lm != 0) & (lm != P.SWEEP_LM_REJECTED)).mean())
            out["closures"] = int(sum(m.slam_sizes(g)[2] for g in range(m.n_graphs)))
            m.timing_enable(True)
            m.stage_times(reset=True)
            for _ in range(3):
                m.reset()
                m.ingest_sweeps_device(d.data_ptr(), n, stride)
            st = m.stage_times(reset=True)
            m.timing_enable(False)
            total = st["decode"][0] + st["slam"][0] + st["raycast"][0]
            out["stage_ms"] = {k: st[k][0] / 3 for k in ("decode", "slam", "slam_chain", "raycast")}
            out["decode_share"] = st["decode"][0] / total
            out["slam_share"] = st["slam"][0] / total
    return out


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
    ap.add_argument("--graph", action="store_true", help="also: graph mode off / on, on this buffer and on the 64-bot room stream")
    a = ap.parse_args()
    buf = sweeps(a.sweeps, 1, 20.0)
    out = dict(metric="sweep_ingest", sweeps=a.sweeps, stride=P.PACKET_SIZE_V0_ODO, region_m=40.0,
               bytes_per_sweep=bytes_per_sweep(), gpu=[gpu_rate(s, buf, a.reps) for s in (4096, 8192)],
               cpu_oracle=cpu_rate(buf))
    print(json.dumps(out))
    if a.graph:
        room = room_sweeps()
        print(json.dumps(dict(metric="sweep_graph", reps=a.reps,
                              random=graph_rate(4096, buf, a.reps, 2, 0), room=graph_rate(4096, room, a.reps, 64, 2))))


if __name__ == "__main__":
    main()
