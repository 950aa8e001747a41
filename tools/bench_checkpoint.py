#!/usr/bin/env python3
"""Checkpoint and restore of a mapping session (qs_checkpoint / qs_restore): bytes, checkpoint time (census + pack + copy to
the host) and restore time (copy to the device + unpack + index rebuild) after one bench.py step (2^20 packets, device
resident) of four shapes.  Prints one JSON line.

    python tools/bench_checkpoint.py [--batch 1048576] [--reps 5]

  c1          configs[1]: the 2-bot session cycled, 4096^2, one pose graph
  c3          configs[3]-shaped: 64 bots in their own room tiles, one pose graph per 2 bots (32 graphs), 4096^2
  one_graph   the same 64 bots in ONE pose graph, 4096^2: the longest landmark log, so the longest index rebuild
  one_graph_8192  the same at 8192^2 (the census reads four times the cells)

Every restore goes into a fresh context of the same configuration and is checked: a second checkpoint of it equals the
first, byte for byte."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quasar_amd as qa  # noqa: E402

replay = importlib.import_module(qa.__name__ + ".replay")


def shape(name, batch):
    size = 8192 if name.endswith("8192") else 4096
    half = size * 0.05 / 2
    if name == "c1":
        session, _ = replay.telemetry_csv_to_packets()
        return dict(size=size, resolution=0.05, origin_x=-half, origin_y=-half, max_agent=2), replay.cycle_stream(session, batch)
    bpg = 2 if name == "c3" else 0
    return (dict(size=size, resolution=0.05, origin_x=-half, origin_y=-half, max_agent=64, bots_per_graph=bpg),
            replay.multi_bot_stream(None, 64, batch))


def run(name, batch, reps):
    kw, stream = shape(name, batch)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(stream).to(dev)
    torch.cuda.synchronize()
    with qa.QuasarMapper(**kw) as m:
        m.ingest_device(d.data_ptr(), len(stream), stream.shape[1])
        m.sync()
        ck = m.checkpoint()                                  # (warm: workspaces allocated)
        t_ck = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ck = m.checkpoint()
            t_ck.append(time.perf_counter() - t0)
        k = qa.checkpoint_config(ck)
        sizes = [m.slam_sizes(g) for g in range(m.n_graphs)]
    t_rs = []
    for _ in range(reps):
        with qa.QuasarMapper(**kw) as t:
            t.sync()
            t0 = time.perf_counter()
            t.restore(ck)
            t_rs.append(time.perf_counter() - t0)
            assert t.checkpoint() == ck, f"{name}: the restored session checkpoints differently"
    landmarks = sum(s[1] for s in sizes)
    return dict(shape=name, size=kw["size"], graphs=len(sizes), packets=len(stream), landmarks=landmarks,
                max_landmarks_per_graph=max(s[1] for s in sizes), closures=sum(s[2] for s in sizes), bytes=len(ck),
                blocks=k["n_blocks"], dense_plane_bytes=kw["size"] ** 2 * 12, fraction_of_dense=len(ck) / (kw["size"] ** 2 * 12),
                checkpoint_ms_median=float(np.median(t_ck)) * 1e3, checkpoint_ms_min=min(t_ck) * 1e3,
                restore_ms_median=float(np.median(t_rs)) * 1e3, restore_ms_min=min(t_rs) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c3,one_graph,one_graph_8192")
    a = ap.parse_args()
    out = dict(metric="checkpoint_restore", batch=a.batch, reps=a.reps, shapes=[run(s, a.batch, a.reps) for s in a.shapes.split(",")])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
