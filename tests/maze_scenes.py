"""Built scenes for the planner and frontier tests: corridors one cell wide in UNKNOWN space, isolated cells, blocks that
meet at a tile corner.  numpy only; the package is not imported.

Every builder returns (grid, rays):
  grid  int8 [size, size] indexed [gy, gx]: -1 UNKNOWN, 0 FREE, 100 OCCUPIED -- the map the scene is meant to be;
  rays  int64 [n, 5]: cell end points x0, y0, x1, y1 and valid.  A free ray (valid 0) frees every cell from (x0, y0) to
        (x1, y1) but the last; an OCCUPIED cell is a zero-length ray with valid 1.  world() turns the end points into cell
        centres ox + (g + 0.5) * res, paint() feeds them to anything with the mappers' update_rays.
With clearance 0 a corridor needs no walls, and every corridor cell (FREE beside UNKNOWN, interior) is a frontier cell."""
import numpy as np

TILE = 64
UNKNOWN, FREE, OCCUPIED = -1, 0, 100

# size -> (res, ox, oy, lo, hi, pitch, dx, dy): the corridor scenes are built from (size, lo, hi, pitch) and moved by (dx, dy)
#   200: the last tile is 8 cells wide and the scenes reach into it;   256: exact tiles;   68: the second tile is 4 cells wide;
#   512: the scene lies over cells [130, 322) x [70, 262), so the planner's bounding box starts at tile (2, 1)
GEOMETRY = {
    200: (0.05, -5.0, -5.0, 4, 196, 4, 0, 0),
    256: (0.05, -6.4, -6.4, 4, 252, 4, 0, 0),
    68: (0.05, -1.7, -1.7, 1, 67, 3, 0, 0),
    512: (0.05, -12.8, -12.8, 4, 196, 4, 126, 66),
}


class _Canvas:
    """The grid and the ray list of a scene, drawn by the same calls."""

    def __init__(self, size):
        self.size = size
        self.grid = np.full((size, size), UNKNOWN, dtype=np.int8)
        self.rays = []

    def row(self, y, a, b):
        """FREE cells [a, b) of row y."""
        assert a < b
        self.grid[y, a:b] = FREE
        self.rays.append((a, y, b, y, 0))

    def col(self, x, a, b):
        """FREE cells [a, b) of column x."""
        assert a < b
        self.grid[a:b, x] = FREE
        self.rays.append((x, a, x, b, 0))

    def occupy(self, x, y):
        self.grid[y, x] = OCCUPIED
        self.rays.append((x, y, x, y, 1))

    def done(self):
        return self.grid, np.array(self.rays, dtype=np.int64).reshape(-1, 5)


def world(rays, res, ox, oy):
    """(rx, ry, hx, hy, valid) of update_rays: the centres of the rays' end cells."""
    r = np.asarray(rays, dtype=np.int64).reshape(-1, 5)
    c = lambda g, o: o + (g.astype(np.float64) + 0.5) * res
    return c(r[:, 0], ox), c(r[:, 1], oy), c(r[:, 2], ox), c(r[:, 3], oy), r[:, 4].astype(np.uint8)


def paint(m, rays, res, ox, oy):
    """The free rays, then the OCCUPIED cells (a later ray wins a cell), through m.update_rays."""
    r = np.asarray(rays, dtype=np.int64).reshape(-1, 5)
    for part in (r[r[:, 4] == 0], r[r[:, 4] != 0]):
        if len(part):
            m.update_rays(*world(part, res, ox, oy))


def centre(cell, res, ox, oy):
    return (ox + (cell[0] + 0.5) * res, oy + (cell[1] + 0.5) * res)


def add_run(scene, x0, y0, x1, y1):
    """The scene with one more free ray (x0, y0) -> (x1, y1), horizontal or vertical: a corridor of its own."""
    grid, rays = scene
    c = _Canvas(len(grid))
    c.grid[:] = grid
    c.rays = [tuple(r) for r in rays.tolist()]
    if y0 == y1:
        c.row(y0, x0, x1)
    else:
        assert x0 == x1
        c.col(x0, y0, y1)
    return c.done()


# ---- corridors ---------------------------------------------------------------------------------------------------------
def serpentine(size, lo, hi, pitch, dx=0, dy=0):
    """Rows y = lo, lo + pitch, ... free over [lo, hi); consecutive rows joined alternately at x = hi - 1 and x = lo."""
    c = _Canvas(size)
    ys = list(range(lo, hi, pitch))
    for y in ys:
        c.row(y + dy, lo + dx, hi + dx)
    for i, y in enumerate(ys[:-1]):
        c.col((hi - 1 if i % 2 == 0 else lo) + dx, y + 1 + dy, y + pitch + dy)
    return c.done()


def spiral(size, lo, hi, pitch, dx=0, dy=0):
    """A rectangular spiral inwards from (lo, lo): legs of n, n, n - pitch, n - pitch, ... steps (n = hi - 1 - lo) turning
    east, north, west, south, so that parallel arms lie pitch cells apart."""
    c = _Canvas(size)
    x, y, n, k = lo + dx, lo + dy, hi - 1 - lo, 0
    c.row(y, x, x + 1)
    while n > 0:
        d = k % 4
        if d == 0:
            c.row(y, x + 1, x + n + 1); x += n
        elif d == 1:
            c.col(x, y + 1, y + n + 1); y += n
        elif d == 2:
            c.row(y, x - n, x); x -= n
        else:
            c.col(x, y - n, y); y -= n
        k += 1
        if k % 2 == 0:
            n -= pitch
    return c.done()


def comb(size, lo, hi, pitch, dx=0, dy=0):
    """Teeth: columns x = lo, lo + pitch, ... over [lo, hi - 1); a spine joins them along row hi - 1, the highest row.
    The lowest linear index of the cluster is the top of the first tooth, (lo, lo), and all the unions meet late."""
    c = _Canvas(size)
    xs = list(range(lo, hi, pitch))
    for x in xs:
        c.col(x + dx, lo + dy, hi - 1 + dy)
    c.row(hi - 1 + dy, xs[0] + dx, xs[-1] + 1 + dx)
    return c.done()


def lattice(size, lo, hi, pitch, dx=0, dy=0):
    """Single FREE cells every pitch cells in both axes, one ray of length 1 each."""
    c = _Canvas(size)
    for y in range(lo, hi, pitch):
        for x in range(lo, hi, pitch):
            c.row(y + dy, x + dx, x + 1 + dx)
    return c.done()


def diagonal_pairs(size, lo, hi, pitch=None, dx=0, dy=0):
    """2 x 2 FREE blocks in a staircase: each touches the next corner to corner only."""
    c = _Canvas(size)
    for a in range(lo, hi - 1, 2):
        c.row(a + dy, a + dx, a + 2 + dx)
        c.row(a + 1 + dy, a + dx, a + 2 + dx)
    return c.done()


def ring(size, lo, hi, pitch=None, dx=0, dy=0):
    """A closed rectangular loop over the rows and columns lo and hi - 1."""
    c = _Canvas(size)
    c.row(lo + dy, lo + dx, hi + dx)
    c.row(hi - 1 + dy, lo + dx, hi + dx)
    c.col(lo + dx, lo + 1 + dy, hi - 1 + dy)
    c.col(hi - 1 + dx, lo + 1 + dy, hi - 1 + dy)
    return c.done()


CORRIDORS = {"serpentine": serpentine, "spiral": spiral, "comb": comb, "ring": ring}
FRONTIER_SCENES = dict(CORRIDORS, lattice=lattice, diagonal_pairs=diagonal_pairs)


def build(name, size):
    """(grid, rays, res, ox, oy) of a frontier scene on one of the geometries."""
    res, ox, oy, lo, hi, pitch, dx, dy = GEOMETRY[size]
    grid, rays = FRONTIER_SCENES[name](size, lo, hi, pitch, dx, dy)
    return grid, rays, res, ox, oy


# ---- tile corners ------------------------------------------------------------------------------------------------------
PINCH_SIZE = 200
PINCH_VARIANTS = ("none", "one", "both")


def pinch_cell(cell, corner, anti):
    """A cell of the diagonal form as it lies in the mirrored (anti-diagonal) form: x -> 2 * corner - 1 - x."""
    return (2 * corner - 1 - cell[0], cell[1]) if anti else tuple(cell)


def pinch(variant, corner=64, anti=False, size=PINCH_SIZE):
    """Two 4 x 4 FREE blocks [corner - 4, corner)^2 and [corner, corner + 4)^2 that meet at the tile corner.  `one` frees
    (corner, corner - 1) as well, `both` also (corner - 1, corner): only then is the diagonal move across the corner legal.
    anti: the mirror image, blocks [corner, corner + 4) x [corner - 4, corner) and [corner - 4, corner) x [corner, corner + 4)."""
    assert variant in PINCH_VARIANTS and corner % TILE == 0
    c = _Canvas(size)
    for k in range(4):
        for y, a in ((corner - 4 + k, corner - 4), (corner + k, corner)):
            xa, xb = sorted((pinch_cell((a, y), corner, anti)[0], pinch_cell((a + 3, y), corner, anti)[0]))
            c.row(y, xa, xb + 1)
    extra = {"none": [], "one": [(corner, corner - 1)], "both": [(corner, corner - 1), (corner - 1, corner)]}[variant]
    for cell in extra:
        x, y = pinch_cell(cell, corner, anti)
        c.row(y, x, x + 1)
    return c.done()


def late_corner(flip_x=False, flip_y=False, corner=64, size=PINCH_SIZE):
    """Four FREE cells round a tile corner, P (c-1, c-1), Q (c, c-1), R (c-1, c), S (c, c), and three corridors to them
    from the goal G (c+32, c-1), here for c = 64:
      A  G down to row 60, west to column 64, up to Q: 38 steps, all in G's tile, settled in round 1;
      B  G up to row 66, west to column 63, down to R: 38 steps through two tile borders, settled in round 3;
      C  G west along rows 63 and 64, changing row (and tile) five times, to S: 37 steps, settled in round 6.
    Q and R hold 190 before S falls to 185, so neither improves then: the only way P learns of its diagonal move to S
    (192 instead of 195 over Q or R) is the diagonal tile being listed for S's improvement -- side bits 4..7 of the round
    kernel.  flip_x / flip_y mirror the scene about the corner, one orientation for each of the four bits."""
    c = _Canvas(size)
    k = corner - 64
    tf = lambda x, y: (2 * corner - 1 - (x + k) if flip_x else x + k, 2 * corner - 1 - (y + k) if flip_y else y + k)

    def seg(x0, y0, x1, y1):
        (ax, ay), (bx, by) = tf(x0, y0), tf(x1, y1)
        if ay == by:
            c.row(ay, min(ax, bx), max(ax, bx) + 1)
        else:
            assert ax == bx
            c.col(ax, min(ay, by), max(ay, by) + 1)

    seg(96, 60, 96, 66)                                          # the trunk through G (96, 63)
    seg(64, 60, 95, 60); seg(64, 61, 64, 63)                     # A, up to Q (64, 63)
    seg(63, 66, 95, 66); seg(63, 64, 63, 65)                     # B, down to R (63, 64)
    for x0, x1, y in ((90, 95, 63), (84, 90, 64), (78, 84, 63), (72, 78, 64), (68, 72, 63), (64, 68, 64)):
        seg(x0, y, x1, y)                                        # C, to S (64, 64); consecutive runs share a column
    seg(63, 63, 63, 63)                                          # P
    cells = {name: tf(*xy) for name, xy in dict(G=(96, 63), P=(63, 63), Q=(64, 63), R=(63, 64), S=(64, 64)).items()}
    return c.done(), cells


# ---- walk chunks ---------------------------------------------------------------------------------------------------------
RUN_SIZE = 200
L_RUNS = (63, 64, 65, 127, 128, 129)
STRAIGHT_N = 150
STRAIGHT_LOOKAHEADS = (1, 63, 64, 65, 127, 128, 129)


L_RUNS_LONG = (64, 128)
LONG_TOP = 140


def l_run(L, top=59, size=RUN_SIZE):
    """The row (10 .. 10 + L, 10), then the column (10 + L, 10 .. top): from (10, 10) the cells of the row are visible, the
    first cell up the column is not, so the waypoint is path index L; the path has L + top - 9 cells.  With top = 59 the
    chunk of 64 path cells after the corner is partial; with top = LONG_TOP and L a multiple of 64 it is full and wholly
    invisible, so every lane of the wave holds a cell of it when the first invisible cell is found in slot 0."""
    c = _Canvas(size)
    c.row(10, 10, 10 + L)
    c.col(10 + L, 10, top + 1)
    return c.done()


def straight(n=STRAIGHT_N, size=RUN_SIZE):
    """One row of n cells from (10, 10)."""
    c = _Canvas(size)
    c.row(10, 10, 10 + n)
    return c.done()


def room(size, lo, hi, occupied):
    """FREE cells [lo, hi)^2 with single OCCUPIED cells."""
    c = _Canvas(size)
    for y in range(lo, hi):
        c.row(y, lo, hi)
    for x, y in occupied:
        c.occupy(x, y)
    return c.done()


CLEARANCE_OCCUPIED = ((63, 63), (64, 64), (128, 10), (5, 5), (194, 194))
CLEARANCES = (0, 1, 15, 16)


# ---- what the tests read off a scene -----------------------------------------------------------------------------------
def corridor_order(grid, first):
    """The cells of a corridor that is a simple 4-connected path, from `first` (an end) to the far end."""
    size = len(grid)
    free = grid == FREE
    path, prev, cur = [tuple(first)], None, tuple(first)
    assert free[cur[1], cur[0]]
    while True:
        nxt = [(cur[0] + ddx, cur[1] + ddy) for ddx, ddy in ((1, 0), (0, 1), (-1, 0), (0, -1))
               if 0 <= cur[0] + ddx < size and 0 <= cur[1] + ddy < size and free[cur[1] + ddy, cur[0] + ddx]
               and (cur[0] + ddx, cur[1] + ddy) != prev]
        if not nxt:
            return path
        assert len(nxt) == 1, (cur, nxt)
        prev, cur = cur, nxt[0]
        path.append(cur)


def crossings(path):
    """Tile borders a path crosses: steps whose two cells lie in different 64 x 64 tiles."""
    t = [(x // TILE, y // TILE) for x, y in path]
    return sum(a != b for a, b in zip(t, t[1:]))


def components(cells, size):
    """(lin, root): the linear indices gy * size + gx of the cells [n, 2] (gx, gy) in their order, and linear index -> the
    lowest linear index of its 4-connected component."""
    lin = [int(y) * size + int(x) for x, y in np.asarray(cells).reshape(-1, 2).tolist()]
    root, todo = {}, set(lin)
    for s in sorted(lin):
        if s in root:
            continue
        root[s], stack = s, [s]
        while stack:
            c = stack.pop()
            for nb in ((c - 1) if c % size else -1, (c + 1) if (c + 1) % size else -1, c - size, c + size):
                if nb in todo and nb not in root:
                    root[nb] = s
                    stack.append(nb)
    return lin, root


# ---- the planner's cases on the serpentine and the spiral -----------------------------------------------------------------
# a second corridor of 12 cells that touches nothing of the scene, per geometry: the free ray (x0, y0, x1, y1)
SPARE = {
    ("serpentine", 200): (4, 198, 16, 198), ("spiral", 200): (4, 198, 16, 198),
    ("serpentine", 256): (4, 254, 16, 254), ("spiral", 256): (4, 254, 16, 254),
    ("serpentine", 68): (1, 66, 13, 66), ("spiral", 68): (1, 3, 1, 15),
    ("serpentine", 512): (130, 264, 142, 264), ("spiral", 512): (130, 264, 142, 264),
}


def plan_case(name, size):
    """The serpentine or the spiral of a geometry with its spare corridor: dict of grid, rays, res, ox, oy, path (the
    corridor's cells from the first to the far end), spare (a cell of the spare corridor), and requests: six (start cell,
    goal cell) pairs of one plan_paths call -- far end -> first cell and back, two mid pairs, start == goal, and a goal in
    the spare corridor."""
    res, ox, oy, lo, hi, pitch, dx, dy = GEOMETRY[size]
    plain = CORRIDORS[name](size, lo, hi, pitch, dx, dy)
    path = corridor_order(plain[0], (lo + dx, lo + dy))
    grid, rays = add_run(plain, *SPARE[name, size])
    n = len(path)
    spare = (SPARE[name, size][0], SPARE[name, size][1])
    mid = path[n // 2]
    requests = [(path[-1], path[0]), (path[0], path[-1]), (path[n // 3], path[2 * n // 3]), (path[n - 7], path[n // 5]),
                (mid, mid), (mid, spare)]
    return dict(grid=grid, rays=rays, res=res, ox=ox, oy=oy, path=path, spare=spare, requests=requests, size=size)


def territory_bots(path, res, ox, oy):
    """Bots of the 64-bit-key cases on a corridor: one at each end, one mid-corridor (an even number of steps from the
    first end, so that one cell lies equally far from both), a duplicate of it, and one at NaN."""
    k = (len(path) // 2) & ~1
    cells = [path[0], path[-1], path[k], path[k]]
    return [centre(c, res, ox, oy) for c in cells] + [(float("nan"), 0.0)]


# snap edges: a serpentine on the 200 geometry that leaves UNKNOWN space above it (rows 4 .. 176, columns 4 .. 179); the
# full one comes within 2 cells of every cell of the grid
SNAP_SCENE = (200, 4, 180, 4)
# name -> (start cell, snap_radius); the goal is the corridor's first cell
SNAP_CASES = {
    "ten_cells": ((100, 186), 10),         # (100, 176) lies 10 cells below: d^2 == r^2 snaps
    "eleven_cells": ((100, 187), 10),      # 11 cells: NO_START
    "between_rows": ((100, 6), 10),        # 2 cells from (100, 4) and from (100, 8): the lower gy * size + gx wins
    "clipped_window": ((198, 198), 64),    # the window [134, 262]^2 is cut at 199 on two sides
}
