#!/usr/bin/env python3
"""The exploration strategies compared by what they uncover: the same bots from the same starts in the same world, once per
strategy (nearest, by_path, by_territory, by_gain), sensing on the device (sim.SwarmSim).  Prints one JSON line per strategy:
the mapper's known cells after every --every ticks.

    python tools/explore_sim.py [--size 400] [--bots 4] [--ticks 120] [--kind sweeps] [--seed 1] [--bodies R] [--veil r]

--bodies R (metres; --kind packets): the bots are discs of that radius and see each other (sim.SwarmSim(bodies=R)); --veil r
turns the mapper's bot veil on with a radius of r cells.  Every line also carries "phantom": the cells OCCUPIED in the mapper
and FREE in the world when the run ends -- walls that are not there.

The world ("rooms"): a walled floor that leaves a 10-cell margin, cut into rooms of 60 cells by walls with a 12-cell door in
every stretch, plus --seed's 30 random pillars of 2 to 5 cells.  The bots start together in the middle room, 0.3 m apart,
facing outward.  The mapper comes from SwarmSim.make_mapper: its trust filters start at 0.02 m, below one cell, since a wall
in the neighbouring cell returns d = res (include/quasar_slam.h, S6)."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch  # before the HIP library (torch bundles its own HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quasar_amd as qa  # noqa: E402

sim = importlib.import_module(qa.__name__ + ".sim")
ROOM, DOOR, MARGIN = 60, (24, 36), 10


def rooms(size, seed):
    """bool [size, size]: the OCCUPIED cells; and the floor's bounds (lo, hi)."""
    lo, hi = MARGIN, size - MARGIN
    occ = np.zeros((size, size), dtype=bool)
    t = np.arange(lo, hi)
    wall = t[((t - lo) % ROOM < DOOR[0]) | ((t - lo) % ROOM >= DOOR[1])]
    for line in list(range(lo, hi, ROOM)) + [hi - 1]:
        solid = t if line in (lo, hi - 1) else wall
        occ[line, solid] = True
        occ[solid, line] = True
    rng = np.random.default_rng(seed)
    for _ in range(30):
        x, y = rng.integers(lo + 2, hi - 7, 2)
        w, h = rng.integers(2, 6, 2)
        occ[y:y + h, x:x + w] = True
    return occ, lo, hi


def paint(m, occ, lo, hi):
    c = lambda g, o: o + (np.asarray(g, dtype=np.float64) + 0.5) * m.res
    rows = np.arange(lo, hi)
    n = len(rows)
    m.update_rays(c(np.full(n, lo), m.ox), c(rows, m.oy), c(np.full(n, hi), m.ox), c(rows, m.oy), np.zeros(n, np.uint8))
    wy, wx = np.nonzero(occ)
    m.update_rays(c(wx, m.ox), c(wy, m.oy), c(wx, m.ox), c(wy, m.oy), np.ones(len(wx), np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--bots", type=int, default=4)
    ap.add_argument("--ticks", type=int, default=120)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--kind", default="sweeps", choices=("sweeps", "packets"))
    ap.add_argument("--max-range", type=float, default=1.2)
    ap.add_argument("--speed", type=float, default=0.4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bodies", type=float, default=None, metavar="R", help="body radius in metres: the bots see each other (packets)")
    ap.add_argument("--veil", type=int, default=0, metavar="r", help="radius of the mapper's bot veil in cells (0 = off)")
    a = ap.parse_args()
    res = 0.05
    half = a.size * res / 2
    occ, lo, hi = rooms(a.size, a.seed)
    mid = lo + ((a.size // 2 - lo) // ROOM) * ROOM + ROOM // 2            # the centre of the room that holds the grid's middle
    occ[mid - 8:mid + 9, mid - 8:mid + 9] = False                        # (no pillar on the starts)
    cx = -half + (mid + 0.5) * res
    ring = [2 * math.pi * k / a.bots for k in range(a.bots)]
    starts = [(cx + 0.3 * math.cos(t), cx + 0.3 * math.sin(t), math.atan2(math.sin(t), math.cos(t))) for t in ring]
    with qa.QuasarMapper(a.size, res, -half, -half) as world:
        paint(world, occ, lo, hi)
        truth = world.grid_i8()
        floor = int((truth != -1).sum())
        for strategy in sim.STRATEGIES:
            with sim.SwarmSim.make_mapper(world, max_agent=a.bots, max_range=a.max_range) as m:
                if a.veil:
                    m.set_bot_veil(a.veil)
                s = sim.SwarmSim(world, m, starts, kind=a.kind, max_range=a.max_range, speed=a.speed, bodies=a.bodies)
                for _ in range(a.ticks):
                    s.step(strategy)
                print(json.dumps(dict(strategy=strategy, world="rooms", size=a.size, seed=a.seed, bots=a.bots, kind=a.kind,
                                      max_range=a.max_range, speed=a.speed, world_cells=floor, every=a.every,
                                      bodies=a.bodies, veil=a.veil, phantom=int(((m.grid_i8() == 100) & (truth == 0)).sum()),
                                      known=s.history[a.every - 1::a.every], final=s.history[-1])), flush=True)


if __name__ == "__main__":
    main()
