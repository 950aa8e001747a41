"""The rules of the map view (include/quasar_slam.h: "map view"; MapRenderer, server_nodes/dual_bot_mapper.py:380-668)
restated in numpy, for the CPU and the GPU tests.  Every expression is fp64 with each operation rounded on its own (numpy
evaluates `off + w * scale` as a multiply and an add), int() truncates toward zero.  The occupancy layer is the UNCULLED rule:
every cell of the grid is looked at, whatever the view."""
import numpy as np

POINT, SQUARE, SEGMENT = 0, 1, 2
LIMIT = float(1 << 30)
# the reference's colour constants (:346-347, :373-374); tests compare them with the recorded ones
BG, LINE, FREE, OCC = (22, 33, 62), (40, 50, 80), (30, 45, 70), (200, 200, 200)


def params(width=1000, height=800, scale=100.0, offset_x=None, offset_y=None, line_min=-20, line_max=20, bg=BG, line=LINE,
           free=FREE, occ=OCC, draw_occupied=False, minify=True):
    return dict(width=int(width), height=int(height), scale=float(scale),
                offset_x=float(width / 2 if offset_x is None else offset_x),
                offset_y=float(height / 2 if offset_y is None else offset_y), line_min=int(line_min), line_max=int(line_max),
                bg=tuple(bg), line=tuple(line), free=tuple(free), occ=tuple(occ), draw_occupied=bool(draw_occupied),
                minify=bool(minify))


# ---- R0 -------------------------------------------------------------------------------------------------------------------
def screen_x(p, wx):
    """-> (int64 sx, drawable) of world x values (array or scalar)."""
    with np.errstate(all="ignore"):
        v = p["offset_x"] + np.asarray(wx, dtype=np.float64) * p["scale"]
        ok = np.abs(v) <= LIMIT                    # False for NaN and infinities
        return np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0).astype(np.int64), ok


def screen_y(p, wy):
    with np.errstate(all="ignore"):
        v = p["offset_y"] - np.asarray(wy, dtype=np.float64) * p["scale"]
        ok = np.abs(v) <= LIMIT
        return np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0).astype(np.int64), ok


def cell_px(p, res):
    return max(1, int(res * p["scale"]))


# ---- R2 -------------------------------------------------------------------------------------------------------------------
def line_columns_rows(p):
    v = np.arange(p["line_min"], p["line_max"] + 1, dtype=np.float64)
    sx, okx = screen_x(p, v)
    sy, oky = screen_y(p, v)
    return (sorted(set(sx[okx & (sx >= 0) & (sx < p["width"])].tolist())),
            sorted(set(sy[oky & (sy >= 0) & (sy < p["height"])].tolist())))


# ---- R3 -------------------------------------------------------------------------------------------------------------------
def visible_cells(p, size, res, ox, oy):
    """The reference's cull (:500-508): (gx_min, gx_max, gy_min, gy_max), the ranges its loops run over.  NOT part of the
    rule: the golden test uses it to show where the recorded calls and the unculled rule can differ (frame row 0)."""
    world_left = -p["offset_x"] / p["scale"]
    world_right = (p["width"] - p["offset_x"]) / p["scale"]
    world_top = p["offset_y"] / p["scale"]
    world_bottom = -(p["height"] - p["offset_y"]) / p["scale"]
    return (max(0, int((world_left - ox) / res) - 1), min(size, int((world_right - ox) / res) + 1),
            max(0, int((world_bottom - oy) / res) - 1), min(size, int((world_top - oy) / res) + 1))


def occupancy_cover(p, grid, res, ox, oy, cull=False):
    """-> (free_cover, occ_cover) bool [h, w]: the pixel is touched by a FREE / an OCCUPIED cell's square or point (or lies
    in its footprint, minified); None, None where the rule draws nothing.  cull: only the cells of visible_cells count."""
    w, h = p["width"], p["height"]
    cpx = cell_px(p, res)
    if cpx < 2 and not p["minify"]:
        return None, None
    size = grid.shape[0]
    if cull:
        x0, x1, y0, y1 = visible_cells(p, size, res, ox, oy)
        kept = np.full_like(grid, -1)
        kept[y0:max(y1, y0), x0:max(x1, x0)] = grid[y0:max(y1, y0), x0:max(x1, x0)]
        grid = kept
    g = np.arange(size, dtype=np.float64)
    sx, okx = screen_x(p, ox + (g + 0.5) * res)
    sy, oky = screen_y(p, oy + (g + 0.5) * res)
    px = np.arange(w, dtype=np.int64)[:, None]
    py = np.arange(h, dtype=np.int64)[:, None]
    if cpx >= 3:
        half = cpx // 2
        ax = okx[None, :] & (sx[None, :] - half <= px) & (px < sx[None, :] - half + cpx)       # [w, size]
        ay = oky[None, :] & (sy[None, :] - half <= py) & (py < sy[None, :] - half + cpx)       # [h, size]
    else:
        ax = okx[None, :] & (sx[None, :] == px)
        ay = oky[None, :] & (sy[None, :] == py)
    ax32, ay32 = ax.astype(np.float32), ay.astype(np.float32)
    cover = []
    for val in (0, 100):
        f = (grid == val).astype(np.float32)                   # [gy, gx]; counts stay below 2^24: exact in fp32
        cover.append((ay32 @ f @ ax32.T) > 0)
    return cover[0], cover[1]


# ---- R5: the closed form of the reference's _bresenham (:158-179) --------------------------------------------
def segment_cells(x0, y0, x1, y1, k=None):
    """Cells k (default: all, 0..M) of _bresenham((x0, y0), (x1, y1)) -> int64 [n, 2]."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    big, small = max(dx, dy), min(dx, dy)
    k = np.arange(big + 1, dtype=np.int64) if k is None else np.asarray(k, dtype=np.int64)
    minor = (2 * k * small + big - 1) // (2 * big) if big else np.zeros_like(k)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    if dx >= dy:
        return np.stack([x0 + sx * k, y0 + sy * minor], axis=1)
    return np.stack([x0 + sx * minor, y0 + sy * k], axis=1)


def segment_pixels(x0, y0, x1, y1, width, height):
    """The segment's pixels inside the frame: k clipped along the major axis first, so the cost is bounded by the frame."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    big = max(dx, dy)
    a0, a1, lim = (x0, x1, width) if dx >= dy else (y0, y1, height)
    if a0 <= a1:
        klo, khi = max(0, -a0), min(big, lim - 1 - a0)
    else:
        klo, khi = max(0, a0 - (lim - 1)), min(big, a0)
    if khi < klo:
        return np.zeros((0, 2), dtype=np.int64)
    c = segment_cells(x0, y0, x1, y1, np.arange(klo, khi + 1, dtype=np.int64))
    return c[(c[:, 0] >= 0) & (c[:, 0] < width) & (c[:, 1] >= 0) & (c[:, 1] < height)]


# ---- the frame --------------------------------------------------------------------------------------------------------------
def zone_rect(p, box):
    """R4's rectangle (sx1, sy1, w, h) of a box (minx, miny, maxx, maxy), or None when it is not drawn."""
    (sx1, sx2), okx = screen_x(p, [box[0], box[2]])
    (sy1, sy2), oky = screen_y(p, [box[3], box[1]])
    if not (okx.all() and oky.all()):
        return None
    w, h = int(sx2 - sx1), int(sy2 - sy1)
    return (int(sx1), int(sy1), w, h) if w > 0 and h > 0 else None


def render(p, grid, res, ox, oy, zones=(), prims=(), cull=False):
    """-> uint8 [height, width, 4].  grid: int8 [size, size] of -1 / 0 / 100 (row = gy); zones: (minx, miny, maxx, maxy, (r, g,
    b)); prims: (kind, size, (r, g, b), x0, y0, x1, y1)."""
    W, H = p["width"], p["height"]
    img = np.empty((H, W, 3), dtype=np.int64)
    img[:] = p["bg"]                                                                     # R1
    cols, rows = line_columns_rows(p)                                                    # R2
    img[:, cols] = p["line"]
    img[rows, :] = p["line"]
    free_c, occ_c = occupancy_cover(p, np.asarray(grid), res, ox, oy, cull)                    # R3
    if free_c is not None:
        img[free_c] = p["free"]
        if p["draw_occupied"]:
            img[occ_c] = p["occ"]
    for z in zones:                                                                      # R4
        r = zone_rect(p, z[:4])
        if r is None:
            continue
        c = np.array(z[4], dtype=np.int64)
        x0, y0, x1, y1 = r[0], r[1], r[0] + r[2], r[1] + r[3]
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        if cx0 >= cx1 or cy0 >= cy1:
            continue
        img[cy0:cy1, cx0:cx1] = (c * 25 + img[cy0:cy1, cx0:cx1] * 230 + 127) // 255
        for yb in (y0, y1 - 1):
            if 0 <= yb < H:
                img[yb, cx0:cx1] = c
        for xb in (x0, x1 - 1):
            if 0 <= xb < W:
                img[cy0:cy1, xb] = c
    for kind, size, color, x0, y0, x1, y1 in prims:                                      # R5
        (sx,), okx = screen_x(p, [x0])
        (sy,), oky = screen_y(p, [y0])
        if not (okx[0] and oky[0]):
            continue
        sx, sy = int(sx), int(sy)
        if kind == POINT:
            if 0 <= sx < W and 0 <= sy < H:
                img[sy, sx] = color
        elif kind == SQUARE:
            xa, ya = sx - size // 2, sy - size // 2
            img[max(ya, 0):max(min(ya + size, H), 0), max(xa, 0):max(min(xa + size, W), 0)] = color
        else:
            (ex,), okx = screen_x(p, [x1])
            (ey,), oky = screen_y(p, [y1])
            if okx[0] and oky[0]:
                c = segment_pixels(sx, sy, int(ex), int(ey), W, H)
                img[c[:, 1], c[:, 0]] = color
    out = np.full((H, W, 4), 255, dtype=np.uint8)
    out[:, :, :3] = img
    return out


# ---- the reference's recorded calls, replayed (tests/golden/view_calls.npz) -----------------------------------------------
def from_records(zones, prims):
    """QuasarMapper.render_view's record arrays (protocol.VIEW_ZONE_DTYPE / VIEW_PRIM_DTYPE) as render's tuples."""
    return ([(*z["box"].tolist(), tuple(z["color"][:3].tolist())) for z in zones],
            [(int(q["kind"]), int(q["size"]), tuple(q["color"][:3].tolist()), float(q["x0"]), float(q["y0"]), float(q["x1"]),
              float(q["y1"])) for q in prims])


def replay(width, height, fill, set_at=(), rects=(), lines=()):
    """A frame from recorded pygame calls: screen.fill, then set_at (x, y, r, g, b), filled draw.rect (x, y, w, h, r, g, b)
    and width-1 axis-parallel draw.line (x0, y0, x1, y1, r, g, b; end points inclusive, clipped) in the given arrays'
    order -- callers pass one kind of call per layer."""
    img = np.empty((height, width, 3), dtype=np.int64)
    img[:] = fill
    for x, y, r, g, b in np.asarray(set_at, dtype=np.int64).reshape(-1, 5):
        if 0 <= x < width and 0 <= y < height:                      # Surface.set_at ignores points outside
            img[y, x] = (r, g, b)
    for x, y, w, h, r, g, b in np.asarray(rects, dtype=np.int64).reshape(-1, 7):
        img[max(y, 0):max(min(y + h, height), 0), max(x, 0):max(min(x + w, width), 0)] = (r, g, b)
    for x0, y0, x1, y1, r, g, b in np.asarray(lines, dtype=np.int64).reshape(-1, 7):
        assert x0 == x1 or y0 == y1
        xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        img[max(ya, 0):max(min(yb + 1, height), 0), max(xa, 0):max(min(xb + 1, width), 0)] = (r, g, b)
    return img
