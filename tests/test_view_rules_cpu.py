"""The map view's rules (include/quasar_slam.h: "map view") on the CPU: the numpy restatement (tests/view_rules.py) against the
calls the reference's renderer made through a recording stub pygame (tests/golden/view_calls.npz, written by
tests/golden/make_view_golden.py), the segment closed form against the reference's _bresenham walk, and the host-side Python:
MapView's lists and MissionControl(track_view=True)."""
import ctypes as C
import importlib
import os
import random
import socket
import time

import numpy as np
import pytest

from conftest import GOLDEN, PKG_NAME, load_pkg
import view_rules as V


@pytest.fixture(scope="module")
def calls():
    return np.load(os.path.join(GOLDEN, "view_calls.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def P():
    return importlib.import_module(PKG_NAME + ".protocol")


def view_params(calls, i, **kw):
    w, h, scale, offx, offy = calls["views"][i]
    return V.params(int(w), int(h), scale, offx, offy, **kw)


def geometry(calls):
    size, res, ox, oy = calls["geom"]
    return int(size), float(res), float(ox), float(oy)


N_VIEWS = 6
NO_LINES = dict(line_min=1, line_max=0)


# ---- the restatement against the reference's recorded calls ---------------------------------------------------------------
def test_fixture_is_small_and_holds_the_six_views(calls):
    assert os.path.getsize(os.path.join(GOLDEN, "view_calls.npz")) < 100 * 1024
    assert calls["views"].tolist() == [[100, 80, 100.0, 50, 40], [100, 80, 47.3, 13.5, 70.25], [37, 53, 163.7, -20.5, 95.0],
                                       [100, 80, 39.9, 50, 40], [64, 64, 500.0, 700.3, -650.1], [100, 80, 60.0, 50, 40]]
    assert calls["grids"].shape == (2, 64, 64) and set(np.unique(calls["grids"]).tolist()) == {-1, 0, 100}
    assert len(calls["occ_set_at_1"]) > 0 and len(calls["occ_rects_1"]) == 0          # view 1 is the cell_px == 2 branch
    assert len(calls["occ_set_at_3"]) == 0 and len(calls["occ_rects_3"]) == 0          # view 3 draws nothing


@pytest.mark.parametrize("i", range(N_VIEWS))
def test_occupancy_equals_the_recorded_calls(calls, i):
    """minify off (the reference's behaviour).  With the reference's cull applied the restatement IS the recorded frame.  The
    rule itself is unculled: a cell just beyond the culled range on the side of the larger gy, whose screen y lies in
    (-cell_px, 0), reaches frame row 0 through the truncation toward zero, so the two may differ there and nowhere else (view
    4 shows it with this fixture's grid)."""
    size, res, ox, oy = geometry(calls)
    p = view_params(calls, i, minify=False, **NO_LINES)
    grid = calls["grids"][i % 2]
    want = V.replay(p["width"], p["height"], p["bg"], set_at=calls[f"occ_set_at_{i}"], rects=calls[f"occ_rects_{i}"])
    culled = V.render(p, grid, res, ox, oy, cull=True)[:, :, :3]
    assert (culled == want).all()
    rule = V.render(p, grid, res, ox, oy)[:, :, :3]
    assert (rule[1:] == want[1:]).all()
    differ = (rule[0] != want[0]).any(axis=1)
    assert (rule[0][differ] == p["free"]).all()           # the rule only ever draws more there


@pytest.mark.parametrize("i", range(N_VIEWS))
def test_metre_lines_equal_the_recorded_calls(calls, i):
    size, res, ox, oy = geometry(calls)
    p = view_params(calls, i)
    want = V.replay(p["width"], p["height"], p["bg"], lines=calls[f"grid_lines_{i}"])
    assert (V.render(p, np.full((size, size), -1, np.int8), res, ox, oy)[:, :, :3] == want).all()
    assert (calls[f"grid_lines_{i}"][:, 4:] == p["line"]).all()


@pytest.mark.parametrize("i", range(N_VIEWS))
def test_zone_rectangles_and_borders_equal_the_recorded_calls(calls, i, P):
    p = view_params(calls, i)
    blits, borders = calls[f"zone_blits_{i}"], calls[f"zone_borders_{i}"]
    rects = [V.zone_rect(p, box) for box in calls["zone_boxes"]]
    drawn = [r for r in rects if r is not None]
    assert len(drawn) == len(blits) == 2
    for r, bl, bo, bot in zip(drawn, blits, borders, (1, 2)):
        assert list(r) == bl[:4].tolist() == bo[:4].tolist()
        assert bl[4:].tolist() == list(P.BOT_COLORS[bot]["main"]) + [25] and bo[4:].tolist() == list(P.BOT_COLORS[bot]["main"]) + [1]
    # the border pixels of the rendered frame are where a 1-pixel outline of that rectangle lies
    size, res, ox, oy = geometry(calls)
    zones = [(*calls["zone_boxes"][b - 1].tolist(), P.BOT_COLORS[b]["main"]) for b in (1, 2)]
    img = V.render(dict(p, **NO_LINES), np.full((size, size), -1, np.int8), res, ox, oy, zones=zones)[:, :, :3]
    x, y, w, h = drawn[1]                                     # the later zone's border is on top
    for px, py in ((x, y), (x + w - 1, y), (x, y + h - 1), (x + w - 1, y + h - 1), (x + w // 2, y), (x, y + h // 2)):
        if 0 <= px < p["width"] and 0 <= py < p["height"]:
            assert tuple(img[py, px]) == P.BOT_COLORS[2]["main"]
    bg = np.array(p["bg"])
    inside = [(px, py) for px in range(max(x + 1, 0), min(x + w - 1, p["width"])) for py in range(max(y + 1, 0), min(y + h - 1, p["height"]))]
    once = (np.array(P.BOT_COLORS[2]["main"]) * 25 + bg * 230 + 127) // 255
    x1, y1, w1, h1 = drawn[0]
    for px, py in inside[::37]:
        if not (x1 <= px < x1 + w1 and y1 <= py < y1 + h1):
            assert (img[py, px] == once).all()


@pytest.mark.parametrize("i", range(N_VIEWS))
def test_cloud_points_and_squares_equal_the_recorded_calls(calls, i, P):
    """MapView.lists (last 2000 points, the on-screen test, 8 x 8 squares for bot 1 left / bot 2 right) under R5."""
    pkg = load_pkg()
    size, res, ox, oy = geometry(calls)
    p = view_params(calls, i, **NO_LINES)
    w, h, scale, offx, offy = calls["views"][i]
    view = pkg.MapView(int(w), int(h), scale, offx, offy)
    clouds = {b: {s: [tuple(q) for q in calls[f"cloud_bot{b}_{s}"].tolist()] for s in P.SENSOR_NAMES} for b in (1, 2)}
    zones, prims = view.lists(point_clouds=clouds)
    assert len(zones) == 0 and len(prims) == len(calls[f"cloud_calls_{i}"])
    rec = calls[f"cloud_calls_{i}"]
    assert (prims["kind"] == np.where(rec[:, 0] == 1, P.VIEW_SQUARE, P.VIEW_POINT)).all()
    want = V.replay(p["width"], p["height"], p["bg"], rects=rec[:, 1:])
    got = V.render(p, np.full((size, size), -1, np.int8), res, ox, oy, *V.from_records(zones, prims))[:, :, :3]
    assert (got == want).all()


def test_protocol_defaults_are_the_recorded_colours(calls, P):
    assert tuple(calls["color_BG_COLOR"]) == P.BG_COLOR == V.BG and tuple(calls["color_GRID_COLOR"]) == P.GRID_COLOR == V.LINE
    assert tuple(calls["color_CELL_COLOR_FREE"]) == P.CELL_COLOR_FREE == V.FREE
    assert tuple(calls["color_CELL_COLOR_OCCUPIED"]) == P.CELL_COLOR_OCCUPIED == V.OCC
    for b in (1, 2):
        for key in ("main", "path", "front", "left", "back", "right"):
            assert tuple(calls[f"color_bot{b}_{key}"]) == P.BOT_COLORS[b][key] == P.bot_colors(b)[key]
    assert (P.VIEW_WIDTH, P.VIEW_HEIGHT, P.VIEW_SCALE, P.VIEW_SCALE_LIMITS) == (1000, 800, 100.0, (20.0, 500.0))
    assert (P.VIEW_LINE_MIN, P.VIEW_LINE_MAX, P.VIEW_CLOUD_RECENT, P.VIEW_CLOUD_RECT, P.VIEW_PATH_POINTS) == (-20, 20, 2000, 8, 500)
    # beyond bot 2: a stated function of the id, byte colours, the sensors of bot 1 (odd) / bot 2 (even)
    seen = set()
    for b in range(3, 65):
        c = P.bot_colors(b)
        assert all(0 <= v <= 255 for v in c["main"] + c["path"]) and max(c["main"]) == 255 and min(c["main"]) == 0
        assert c["left"] == P.BOT_COLORS[1 if b % 2 else 2]["left"]
        seen.add(c["main"])
    assert len(seen) > 40 and P.bot_colors(7) == P.bot_colors(7)


def test_struct_layouts_match_the_header(P):
    lib = importlib.import_module(PKG_NAME + "._lib")
    assert C.sizeof(lib.QsViewParams) == 72 and lib.QsViewParams.scale.offset == 8 and lib.QsViewParams.bg.offset == 40
    assert lib.QsViewParams.draw_occupied.offset == 56
    assert P.VIEW_ZONE_DTYPE.itemsize == 40 and P.VIEW_ZONE_DTYPE.fields["color"][1] == 32
    assert P.VIEW_PRIM_DTYPE.itemsize == 48 and P.VIEW_PRIM_DTYPE.fields["kind"][1] == 32 and P.VIEW_PRIM_DTYPE.fields["color"][1] == 40
    txt = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "quasar_slam.h")).read()
    assert "QS_VIEW_POINT = 0, QS_VIEW_SQUARE = 1, QS_VIEW_SEGMENT = 2" in txt
    assert (P.VIEW_POINT, P.VIEW_SQUARE, P.VIEW_SEGMENT) == (V.POINT, V.SQUARE, V.SEGMENT) == (0, 1, 2)


# ---- the segment closed form against the reference's walk -----------------------------------------------------------------
def bresenham_walk(x0, y0, x1, y1):
    """dual_bot_mapper.py:158-179, statement for statement."""
    cells = []
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx = 1 if x0 < x1 else -1
    sy = 1 if y0 < y1 else -1
    err = dx - dy
    while True:
        cells.append((x0, y0))
        if x0 == x1 and y0 == y1:
            break
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x0 += sx
        if e2 < dx:
            err += dx
            y0 += sy
    return cells


def test_segment_closed_form_exhaustive_d40():
    g = np.load(os.path.join(GOLDEN, "bresenham_d40.npz"), allow_pickle=False)
    D, starts, cells = int(g["D"][0]), g["starts"], g["cells"].astype(np.int64)
    i = 0
    for dy in range(-D, D + 1):
        for dx in range(-D, D + 1):
            want = cells[starts[i]:starts[i + 1]]
            got = V.segment_cells(0, 0, dx, dy)
            assert got.shape == want.shape and (got == want).all(), (dx, dy)
            i += 1


def test_segment_closed_form_random_long():
    rng = random.Random(5)
    for case in range(60):
        big = rng.choice([1, 2, 3, 17, 255, 1000, 4097, 99991, 100000])
        small = rng.randint(0, big) if case % 5 else rng.choice([0, 1, big - 1, big, big // 2])
        small = max(0, small)
        dx, dy = (big, small) if case % 2 else (small, big)
        x0, y0 = rng.randint(-10 ** 6, 10 ** 6), rng.randint(-10 ** 6, 10 ** 6)
        x1, y1 = x0 + rng.choice([-1, 1]) * dx, y0 + rng.choice([-1, 1]) * dy
        want = np.array(bresenham_walk(x0, y0, x1, y1), dtype=np.int64)
        got = V.segment_cells(x0, y0, x1, y1)
        assert got.shape == want.shape and (got == want).all(), (x0, y0, x1, y1)


def test_segment_clip_keeps_exactly_the_frame_pixels():
    rng = random.Random(9)
    W, H = 37, 53
    for _ in range(300):
        x0, y0, x1, y1 = (rng.randint(-80, 120) for _ in range(4))
        inside = [c for c in bresenham_walk(x0, y0, x1, y1) if 0 <= c[0] < W and 0 <= c[1] < H]
        got = V.segment_pixels(x0, y0, x1, y1, W, H)
        assert sorted(map(tuple, got.tolist())) == sorted(inside)
    far = V.segment_pixels(5, 7, 5 + 10 ** 7, 7 + 3 * 10 ** 6, W, H)          # bounded by the frame, not by the length
    assert 0 < len(far) <= W and tuple(far[0]) == (5, 7)


# ---- MapView --------------------------------------------------------------------------------------------------------------
def test_mapview_defaults_zoom_pan_and_screen_mapping():
    pkg = load_pkg()
    v = pkg.MapView()
    assert (v.width, v.height, v.scale, v.offset_x, v.offset_y) == (1000, 800, 100.0, 500.0, 400.0)
    assert v.world_to_screen(1.25, -0.5) == (625, 450) and v.world_to_screen(-5.004, 4.004) == (0, 0)
    for _ in range(40):
        v.zoom(1.15)
    assert v.scale == 500.0
    for _ in range(80):
        v.zoom(1 / 1.15)
    assert v.scale == 20.0
    wide = pkg.MapView(scale=4.0, scale_limits=(1.0, 500.0))
    assert wide.zoom(0.5) == 2.0 and wide.zoom(0.1) == 1.0
    v.pan(-30, 12.5)
    assert (v.offset_x, v.offset_y) == (470.0, 412.5)
    assert pkg.MapView(64, 64, 500.0, 700.3, -650.1).world_to_screen(-1.4, -1.3) == (0, 0)     # (-1, 1) -> 0: truncation


class RecordingMapper:
    def render_view(self, *a, **kw):
        self.args, self.kw = a, kw
        return np.zeros((a[1], a[0], 4), dtype=np.uint8)


def test_mapview_lists_order_and_subsampling(P, tmp_path):
    pkg = load_pkg()
    v = pkg.MapView(200, 100, 10.0)
    n_path = 1234
    clouds = {2: {"front": [(0.5, 0.5)], "right": [(1.0, 1.0), (900.0, 0.0)]},                   # (900, 0) is off-screen: dropped
              1: {"front": [(float(i) * 1e-3, 0.0) for i in range(2500)], "left": [(-1.0, 2.0)], "back": [], "right": []}}
    paths = {1: ([0.01 * i for i in range(n_path)], [0.0] * n_path), 2: ([1.0], [1.0]), 3: ([0.0, 1.0, 2.0], [0.0, 1.0, 0.0])}
    states = {1: {"x": 0.0, "y": 0.0, "online": True}, 2: {"x": 1.0, "y": 1.0, "online": False}}
    m = RecordingMapper()
    frame = v.frame(m, zone_boxes={2: (0, 0, 1, 1), 1: (-1, -1, 0, 0), 3: None}, point_clouds=clouds, paths=paths, bot_states=states,
                    targets={1: (2.0, 2.0), 2: (3.0, 3.0)}, closures=[(0.0, 0.0, 1.0, 0.5)], draw_occupied=True)
    assert frame.shape == (100, 200, 4) and m.args == (200, 100, 10.0, 100.0, 50.0) and m.kw["draw_occupied"] is True
    zones, prims = m.kw["zones"], m.kw["prims"]
    assert zones["box"].tolist() == [[-1, -1, 0, 0], [0, 0, 1, 1]]                                # bot-id order, None skipped
    assert [tuple(c[:3]) for c in zones["color"].tolist()] == [P.BOT_COLORS[1]["main"], P.BOT_COLORS[2]["main"]]
    step = max(1, n_path // 500)
    n_seg1 = len(range(0, n_path, step)) - 1
    kinds = prims["kind"].tolist()
    want_kinds = ([P.VIEW_POINT] * 2000 + [P.VIEW_SQUARE] + [P.VIEW_POINT] + [P.VIEW_SQUARE]        # bot 1 front, left; bot 2 front, right
                  + [P.VIEW_SEGMENT] * (n_seg1 + 2) + [P.VIEW_SEGMENT] * 2)                          # paths 1 and 3; target; closure
    assert kinds == want_kinds
    assert prims["x0"][0] == 0.5 and prims["x0"][1999] == 2.499                                    # the LAST 2000 of 2500
    assert prims["size"][2000] == 8 and (prims["x0"][2000], prims["y0"][2000]) == (-1.0, 2.0)
    assert tuple(prims["color"][2000][:3]) == P.BOT_COLORS[1]["left"] and tuple(prims["color"][2002][:3]) == P.BOT_COLORS[2]["right"]
    seg = prims[2003:2003 + n_seg1]
    assert (seg["x0"] == np.array(paths[1][0])[::step][:-1]).all() and (seg["x1"] == np.array(paths[1][0])[::step][1:]).all()
    assert tuple(seg["color"][0][:3]) == P.BOT_COLORS[1]["path"]
    assert tuple(prims["color"][2003 + n_seg1][:3]) == P.bot_colors(3)["path"]
    target, closure = prims[-2], prims[-1]                                                         # bot 2 is offline: no target line
    assert (target["x0"], target["y0"], target["x1"], target["y1"]) == (0.0, 0.0, 2.0, 2.0)
    assert tuple(target["color"][:3]) == P.BOT_COLORS[1]["main"] and tuple(closure["color"][:3]) == (0, 255, 100)
    assert (closure["x0"], closure["y0"], closure["x1"], closure["y1"]) == (0.0, 0.0, 1.0, 0.5)
    z0, p0 = v.lists()
    assert len(z0) == 0 and len(p0) == 0 and p0.dtype == P.VIEW_PRIM_DTYPE
    rgba = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    pkg.MapView.save_ppm(str(tmp_path / "f.ppm"), rgba)
    assert open(tmp_path / "f.ppm", "rb").read() == b"P6\n3 2\n255\n" + rgba[:, :, :3].tobytes()


# ---- MissionControl(track_view=True) ----------------------------------------------------------------------------------------
class StubMapper:
    """ingest_array / last_batch / last_hits of a mapper whose pose is the packet's and whose only valid ray is the front one."""

    def ingest_array(self, buf, lens, times):
        P = importlib.import_module(PKG_NAME + ".protocol")
        self.rec = np.ascontiguousarray(buf[:, :42]).view(P.PACKET_DTYPE).reshape(-1)
        self.acc = ((lens == 42) & (self.rec["magic"] == b"QSRL") & (self.rec["agent"] >= 1) & (self.rec["agent"] <= 2)).astype(np.uint8)

    def last_batch(self):
        return self.acc, np.stack([self.rec["x"], self.rec["y"], self.rec["yaw"]], axis=1).astype(np.float64)

    def last_hits(self):
        n = len(self.acc)
        xy = np.zeros((n, 4, 2))
        xy[:, 0, 0] = self.rec["x"] + self.rec["front"]
        xy[:, 0, 1] = self.rec["y"]
        xy[:, 3, :] = 7.0
        valid = np.zeros((n, 4), dtype=np.uint8)
        valid[:, 0] = 1
        valid[:, 3] = self.rec["right"] > 1.0
        return xy, valid


def test_mission_control_track_view_keeps_clouds_and_paths(P):
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    off = fe.MissionControl(StubMapper(), sock=srv.dup())
    assert off.track_view is False and off.paths == {1: ([], []), 2: ([], [])}
    off.close()
    mc = fe.MissionControl(StubMapper(), sock=srv, track_view=True)
    bot = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    p1 = P.pack_packet(1, 0.5, 0.25, 0.0, 1, 2, 0.5, 0.6, 0.7, 0.8, 0)
    p2 = P.pack_packet(2, 1.0, -1.0, 0.0, 1, 2, 0.25, 0.6, 0.7, 2.0, 0)
    for d in (p1, b"junk", p2, p1):
        bot.sendto(d, srv.getsockname())
    deadline = time.time() + 2.0
    n = 0
    while n < 4 and time.time() < deadline:
        n += mc.poll(now=1.0)
    assert n == 4
    assert mc.paths == {1: ([0.5, 0.5], [0.25, 0.25]), 2: ([1.0], [-1.0])}
    assert mc.point_clouds[1] == {"front": [(1.0, 0.25), (1.0, 0.25)], "left": [], "back": [], "right": []}
    assert mc.point_clouds[2] == {"front": [(1.25, -1.0)], "left": [], "back": [], "right": [(7.0, 7.0)]}
    bot.close()
    mc.close()
