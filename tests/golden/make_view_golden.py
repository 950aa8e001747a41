#!/usr/bin/env python3
"""Golden calls of the reference's map renderer.  RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference), like make_golden.py.

MapRenderer (server_nodes/dual_bot_mapper.py:380-668) cannot be constructed without pygame, but its pixel rules for the layers
the map view rebuilds are plain Python around four pygame calls: Surface.set_at, a filled draw.rect, a 1-pixel draw.line and a
blit of a filled Surface.  This script loads the reference with a stub `pygame` whose calls record their arguments, calls
_draw_occupancy, _draw_grid, _draw_zones and _draw_point_cloud unbound on an object that holds the view state, and writes what
was recorded -- integers only -- to view_calls.npz, next to the inputs (grids, views, boxes, clouds) and the colour constants.

    python tests/golden/make_view_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

VIEWS = [(100, 80, 100.0, 50, 40),
         (100, 80, 47.3, 13.5, 70.25),        # cell_px == 2: the set_at branch
         (37, 53, 163.7, -20.5, 95.0),
         (100, 80, 39.9, 50, 40),             # cell_px == 1: the reference draws nothing
         (64, 64, 500.0, 700.3, -650.1),
         (100, 80, 60.0, 50, 40)]
SIZE, RES, OX, OY = 64, 0.05, -1.6, -1.6


class Recorder:
    def __init__(self):
        self.set_at, self.rects, self.outlines, self.lines, self.wide_lines, self.blits = [], [], [], [], [], []
        self.ordered = []          # set_at (kind 0, as a 1 x 1 rect) and filled rects (kind 1) in call order


def stub_pygame(rec):
    pg = types.ModuleType("pygame")
    pg.SRCALPHA = 65536
    draw = types.ModuleType("pygame.draw")

    def rect(surface, color, r, width=0):
        (rec.outlines if width else rec.rects).append([int(v) for v in r] + [int(c) for c in color[:3]] + ([int(width)] if width else []))
        if not width:
            rec.ordered.append([1] + [int(v) for v in r] + [int(c) for c in color[:3]])

    def line(surface, color, a, b, width=1):
        (rec.lines if width == 1 else rec.wide_lines).append([int(a[0]), int(a[1]), int(b[0]), int(b[1])] + [int(c) for c in color[:3]])

    draw.rect, draw.line = rect, line
    pg.draw = draw

    class Surface:
        def __init__(self, size, flags=0):
            self.size, self.flags, self.color = (int(size[0]), int(size[1])), flags, None

        def fill(self, color):
            self.color = tuple(int(c) for c in color)

    pg.Surface = Surface
    return pg


class Screen:
    def __init__(self, rec):
        self.rec = rec

    def set_at(self, pos, color):
        self.rec.set_at.append([int(pos[0]), int(pos[1])] + [int(c) for c in color[:3]])
        self.rec.ordered.append([0, int(pos[0]), int(pos[1]), 1, 1] + [int(c) for c in color[:3]])

    def blit(self, surf, pos):
        self.rec.blits.append([int(pos[0]), int(pos[1]), surf.size[0], surf.size[1]] + list(surf.color))


def load_reference(pg):
    pg.gfxdraw = types.ModuleType("pygame.gfxdraw")             # `from pygame import gfxdraw` (:31); never called by these layers
    sys.modules["pygame"], sys.modules["pygame.gfxdraw"] = pg, pg.gfxdraw
    spec = importlib.util.spec_from_file_location("ref_dual_bot_mapper_view", os.path.join(REF, "server_nodes", "dual_bot_mapper.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def arr(rows, n):
    return np.array(rows, dtype=np.int32).reshape(-1, n)


def main():
    rec = Recorder()
    ref = load_reference(stub_pygame(rec))
    rng = np.random.default_rng(20260611)
    out = {"views": np.array(VIEWS, dtype=np.float64), "geom": np.array([SIZE, RES, OX, OY], dtype=np.float64)}
    grids = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(2, SIZE, SIZE), p=[0.4, 0.45, 0.15])
    out["grids"] = grids
    # inputs of the zone and cloud layers, on a 1/64 m lattice (exact in binary, and they compress)
    boxes = {1: (-1.25, -0.75, 0.5, 0.875), 2: (-0.25, -1.5, 1.40625, 0.25)}
    out["zone_boxes"] = np.array([boxes[1], boxes[2]], dtype=np.float64)
    clouds = {b: {s: [tuple(p) for p in np.round(rng.uniform(-2.0, 2.0, size=(n, 2)) * 64) / 64]
                  for s, n in zip(ref.SENSOR_ANGLES_RAD, counts)}
              for b, counts in ((1, (300, 2100, 0, 150)), (2, (120, 40, 2500, 260)))}
    for b in clouds:
        for s in clouds[b]:
            out[f"cloud_bot{b}_{s}"] = np.array(clouds[b][s], dtype=np.float64).reshape(-1, 2)
    for name in ("BG_COLOR", "GRID_COLOR", "CELL_COLOR_FREE", "CELL_COLOR_OCCUPIED"):
        out["color_" + name] = np.array(getattr(ref, name), dtype=np.int32)
    for b in (1, 2):
        for key in ("main", "path", "front", "left", "back", "right"):
            out[f"color_bot{b}_{key}"] = np.array(ref.BOT_COLORS[b][key], dtype=np.int32)
    R = ref.MapRenderer
    for i, (w, h, scale, offx, offy) in enumerate(VIEWS):
        view = types.SimpleNamespace(width=w, height=h, scale=scale, offset_x=offx, offset_y=offy, screen=Screen(rec))
        view.world_to_screen = lambda wx, wy, v=view: R.world_to_screen(v, wx, wy)
        occ = ref.OccupancyGrid(SIZE, RES, OX, OY)
        occ.grid = grids[i % 2].copy()
        rec.__init__()
        R._draw_occupancy(view, occ)
        assert not (rec.outlines or rec.lines or rec.wide_lines or rec.blits)
        out[f"occ_set_at_{i}"], out[f"occ_rects_{i}"] = arr(rec.set_at, 5), arr(rec.rects, 7)
        rec.__init__()
        R._draw_grid(view)
        assert not (rec.set_at or rec.rects or rec.outlines or rec.blits) and len(rec.wide_lines) == 2       # the crosshair
        out[f"grid_lines_{i}"] = arr(rec.lines, 7)
        rec.__init__()
        R._draw_zones(view, boxes)
        assert not (rec.set_at or rec.rects or rec.lines or rec.wide_lines) and len(rec.blits) == len(rec.outlines)
        out[f"zone_blits_{i}"], out[f"zone_borders_{i}"] = arr(rec.blits, 8), arr(rec.outlines, 8)
        rec.__init__()
        for b in (1, 2):
            R._draw_point_cloud(view, b, clouds[b])
        assert not (rec.outlines or rec.lines or rec.wide_lines or rec.blits)
        # set_at and rect calls interleave by sensor: kept in call order as (kind, x, y, w, h, r, g, b), a set_at as a 1 x 1 rect
        out[f"cloud_calls_{i}"] = arr(rec.ordered, 8)
        print(f"view {i}: occ set_at {len(out[f'occ_set_at_{i}'])} rects {len(out[f'occ_rects_{i}'])}; lines "
              f"{len(out[f'grid_lines_{i}'])}; zones {len(rec.blits)}; cloud calls {len(out[f'cloud_calls_{i}'])}")
    path = os.path.join(HERE, "view_calls.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
