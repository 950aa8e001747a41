"""The loop-closure search as a plain list scan, and landmark fields built to drive its geometry on purpose: the distance test
at the radius, the cell a pose falls in, the hash table over the cells.  For tests/test_closure_rules_cpu.py and
tests/test_gpu_closure_fields.py.

scan() restates PoseGraphSLAM.add_pose / _check_closure (server_nodes/dual_bot_mapper.py:273-326) with the closure radius, the
cool-down, the correction factor and "poses as given" as parameters.  It knows nothing of cells, buckets or hashes: a list of
(x, y, type, node), scanned in list order for every landmark event, the test sqrt(dx^2 + dy^2) < radius in Python floats.

Every scene asserts its own premise while it is built (Build.ask(want=...) asserts what the scan answers to every asking event;
the builders assert the cells, keys and rounds they were made for), so a change of a hash constant or of a cell edge makes the
scene fail loudly instead of quietly testing nothing.

Two things the scenes had to take into account:
  * Python's x ** 2 is libm's pow(x, 2), which is not correctly rounded: about one square in a thousand differs from x * x by
    an ulp.  The ring scenes pick their points where both agree, so they test the comparison and not libm.
  * r2_threshold(0.625) is one ulp BELOW 0.625 ** 2 (sqrt rounds that value up to 0.625), so of the two dyadic radii only 0.75
    has d2 == threshold at its "equal" point; at 0.625 the point has d2 == radius ** 2 exactly, the first value the scan refuses."""
import functools
import itertools
import math

import numpy as np

from chain_lookahead_rules import CAP, NTYPES, Chains, Geometry, r2_threshold

REF = dict(radius=0.6, min_between=30, correction=0.5)          # the reference's constants (:99-101)
WORLDS = {200: (200, 0.05, -5.0, -5.0), 64: (64, 0.05, -1.6, -1.6), 512: (512, 0.05, -12.8, -12.8)}
# wrong variants of the scan (tests/test_closure_rules_cpu.py shows which scenes tell each from the scan):
#   le      sqrt(d2) <= radius
#   rr      dx*dx + dy*dy < radius*radius instead of the square root (the threshold the device must not use)
#   notype  the landmark's type is not looked at
#   cell    an index that takes a table entry to belong to one cell -- the cell that wrote to it first: a landmark whose cell
#           shares the entry with an earlier cell is never seen.  (Read literally, "a landmark is seen only if its true cell is one
#           of the query's nine" holds for every landmark within the radius, and is no mutant at all.)
#   rows    per table entry only the first seven entries -- the first node's rows -- are looked at
MUTANTS = ("le", "rr", "notype", "cell", "rows")


class Scanner:
    """The list scan, an event at a time."""

    def __init__(self, radius, min_between, correction, raw, mutant=None, geom=None):
        assert mutant is None or mutant in MUTANTS
        assert mutant not in ("cell", "rows") or geom is not None
        self.radius, self.min_between, self.correction, self.raw = radius, min_between, correction, raw
        self.mutant, self.geom = mutant, geom
        self.n_nodes = 0
        self.landmarks = []               # (x, y, type, node)                             :269
        self.pairs, self.corrs = [], []   # (matched landmark's node, closing node); (dx, dy)   :270
        self.last = {}                    # agent -> node of its last closure; -min_between at the start   :271
        self.drift = {}                   # agent -> [dx, dy]                              :782
        self.asked = []                   # (node, x, y, type, match or -1) of every event past its agent's cool-down
        self._seen = []                   # mutants "cell" and "rows": whether the wrong index shows the landmark
        self._entry = {}                  # table entry -> [the cell that wrote first, entries]

    def _within(self, x, y, lx, ly):
        if self.mutant == "rr":
            return (x - lx) * (x - lx) + (y - ly) * (y - ly) < self.radius * self.radius
        d = math.sqrt((x - lx) ** 2 + (y - ly) ** 2)
        return d <= self.radius if self.mutant == "le" else d < self.radius

    def add(self, x, y, agent, lm):
        """One pose.  Returns (node, pose x, pose y, the matched landmark's node or None)."""
        d = self.drift.setdefault(agent, [0.0, 0.0])
        if not self.raw:
            x, y = x + d[0], y + d[1]                                            # :855-857
        idx = self.n_nodes
        self.n_nodes += 1
        if lm == 0:
            return idx, x, y, None
        match = None
        if idx - self.last.get(agent, -self.min_between) >= self.min_between:   # :303-304
            for k, (lx, ly, lt, li) in enumerate(self.landmarks):
                if (lt != lm and self.mutant != "notype") or idx - li < self.min_between or not self._seen[k]:
                    continue
                if self._within(x, y, lx, ly):
                    cx, cy = (lx - x) * self.correction, (ly - y) * self.correction
                    self.pairs.append((li, idx))
                    self.corrs.append((cx, cy))
                    self.last[agent] = idx
                    d[0] += cx                                                   # :908-914 (the caller's, on poses as given)
                    d[1] += cy
                    match = li
                    break
            self.asked.append((idx, x, y, lm, -1 if match is None else match))
        seen = True
        if self.geom is not None and 1 <= lm <= NTYPES:
            c = self.geom.cell(x, y)
            e = self._entry.setdefault(self.geom.key(lm, *c), [c, 0])
            seen = (self.mutant != "cell" or e[0] == c) and (self.mutant != "rows" or e[1] < CAP)
            e[1] += 1
        self._seen.append(seen)
        self.landmarks.append((x, y, lm, idx))
        return idx, x, y, match

    def result(self):
        return dict(pairs=np.array(self.pairs, dtype=np.int64).reshape(-1, 2),
                    corr=np.array(self.corrs, dtype=np.float64).reshape(-1, 2),
                    lm_xy=np.array([l[:2] for l in self.landmarks], dtype=np.float64).reshape(-1, 2),
                    lm_ti=np.array([l[2:] for l in self.landmarks], dtype=np.int64).reshape(-1, 2),
                    drift={a: tuple(v) for a, v in self.drift.items()}, asked=list(self.asked), n_nodes=self.n_nodes)


def scan(x, y, agent, lm, radius=REF["radius"], min_between=REF["min_between"], correction=REF["correction"], raw=True,
         mutant=None, geom=None):
    """The whole stream.  raw: the poses are used as given (the qs_slam_add_poses contract); otherwise pose = value + the agent's
    drift, and the drift takes every correction (the packet route, separation 0).  Returns dict(pairs [n, 2] (matched landmark's
    node, closing node), corr [n, 2], lm_xy [m, 2], lm_ti [m, 2] (type, node), drift {agent: (dx, dy)}, asked, n_nodes)."""
    s = Scanner(radius, min_between, correction, raw, mutant, geom)
    for i in range(len(x)):
        s.add(float(x[i]), float(y[i]), int(agent[i]), int(lm[i]))
    return s.result()


def scan_graphs(x, y, agent, lm, bots_per_graph, **kw):
    """One scan per pose graph (agents 1..bots_per_graph, the next bots_per_graph, ...): {graph: scan result}."""
    x, y, agent, lm = (np.asarray(v) for v in (x, y, agent, lm))
    g = (agent.astype(np.int64) - 1) // bots_per_graph
    return {int(k): scan(x[g == k], y[g == k], agent[g == k], lm[g == k], **kw) for k in np.unique(g)}


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, b):
        self.name, self.nb, self.raw, self.f32 = b.name, b.nb, b.raw, b.f32
        self.world, self.radius, self.min_between, self.correction = b.world, b.radius, b.min_between, b.correction
        rows = np.array(b.rows, dtype=np.float64).reshape(-1, 4)
        self.x, self.y = np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1])
        self.agent, self.type = rows[:, 2].astype(np.uint8), rows[:, 3].astype(np.uint8)
        self.cuts = tuple(b.cuts)                      # where the stream may be cut: between laying and asking
        self.tags = frozenset(b.tags)
        self.want = tuple(b.want)                      # (matched node or None, asking node) of every event put with ask()
        self.ref = b.sc.result()
        for a in (self.x, self.y, self.agent, self.type):
            a.setflags(write=False)
        assert 0 < len(self.x) < 1500 and all(0 < c < len(self.x) for c in self.cuts)

    @property
    def params(self):
        return dict(radius=self.radius, min_between=self.min_between, correction=self.correction)

    def geom(self):
        return Geometry(*self.world, self.radius)

    def chains(self):
        return Chains(self.geom(), self.ref["lm_xy"], self.ref["lm_ti"][:, 0], self.ref["lm_ti"][:, 1])


class Build:
    """Bot 1 lays and pads, bots 2..nb ask in turn.  raw: the values are the poses.  Otherwise (the packet route) a value is the
    pose wanted less the bot's drift so far, rounded to f32, and the pose is what that gives: put() returns it."""
    PAD = (-4.0, 4.5)                                  # where bot 1 stands for the poses that carry no landmark

    def __init__(self, name, nb, raw, world=200, radius=REF["radius"], min_between=REF["min_between"],
                 correction=REF["correction"], f32=None):
        assert nb >= 2
        self.name, self.nb, self.raw, self.f32 = name, nb, raw, (not raw) if f32 is None else f32
        assert raw or self.f32
        self.world, self.radius, self.min_between, self.correction = WORLDS[world], radius, min_between, correction
        self.g = Geometry(*self.world, radius)
        self.sc = Scanner(radius, min_between, correction, raw)
        self.rows, self.cuts, self.tags, self.want = [], [], set(), []
        self._askers = itertools.cycle(range(2, nb + 1))

    def put(self, agent, x, y, lm):
        d = self.sc.drift.get(agent, (0.0, 0.0))
        vx, vy = (x, y) if self.raw else (x - d[0], y - d[1])
        if self.f32:
            vx, vy = float(np.float32(vx)), float(np.float32(vy))
        self.rows.append((vx, vy, agent, lm))
        return self.sc.add(vx, vy, agent, lm)

    def lay(self, x, y, t, quiet=True):
        node, px, py, match = self.put(1, x, y, t)
        assert not quiet or match is None, (self.name, "the laying bot closed", node)
        return node, px, py

    def pad(self, n=None):
        for _ in range(self.min_between if n is None else n):
            self.put(1, *self.PAD, 0)

    def cut(self):
        self.cuts.append(len(self.rows))

    def fillers(self, clear_of, n=64, t=4):
        """n landmarks of bot 1, each at a place of its own more than two metres from `clear_of` and 1.25 m from the next: what
        was laid before them has left every window, ring and pending list of a kernel that takes the stream in one launch."""
        pts = [(-5.5 + 1.25 * i, -5.5 + 1.25 * j) for j in range(10) for i in range(10)]
        pts = [p for p in pts if math.dist(p, clear_of) > 2.1][:n]
        assert len(pts) == n and self.radius < 1.25
        for p in pts:
            self.lay(*p, t)

    def ask(self, x, y, t, want, agent=None, wait=True):
        """An asking event; want: the landmark's node the scan must answer, None for nothing.  wait: the bot stands out its
        cool-down first (poses without a landmark), so that the event is a query."""
        a = next(self._askers) if agent is None else agent
        while wait and self.sc.n_nodes - self.sc.last.get(a, -self.min_between) < self.min_between:
            self.put(1, *self.PAD, 0)
        was_query = self.sc.n_nodes - self.sc.last.get(a, -self.min_between) >= self.min_between
        node, px, py, match = self.put(a, x, y, t)
        assert match == want, (self.name, "asked at node", node, "wanted", want, "the scan says", match)
        self.want.append((want, node))
        return node, px, py, a, was_query

    def done(self):
        return Scene(self)


def _step(v, k):
    for _ in range(abs(k)):
        v = math.nextafter(v, math.inf if k > 0 else -math.inf)
    return v


def d2_device(qx, qy, lx, ly):
    """dx*dx + dy*dy as the device rounds it (no contraction: csrc/Makefile)."""
    dx, dy = qx - lx, qy - ly
    return dx * dx + dy * dy


def d2_reference(qx, qy, lx, ly):
    return (qx - lx) ** 2 + (qy - ly) ** 2


def edge_point(lx, ly, ux, uy, target):
    """A double point in direction (ux, uy) from (lx, ly) -- to some 1e-5 rad: along an axis the squares of the doubles skip
    more than every other value, so the other coordinate makes up the remainder -- whose dx*dx + dy*dy rounds to `target`
    exactly, by the device's arithmetic and by the reference's."""
    t = math.sqrt(target)
    swap = abs(uy) > abs(ux)
    if swap:
        lx, ly, ux, uy = ly, lx, uy, ux
    start = lx + t * ux / math.hypot(ux, uy)
    # (steps of a nanometre, not of single doubles: on a diagonal dx ~ dy, and one double more in x against one less in y
    # changes the sum by next to nothing -- the sums reachable that way lie some ten values apart)
    for i in sorted(range(-4096, 4097), key=abs):
        qa = start + i * 1.0000001e-9
        rem = target - (qa - lx) * (qa - lx)
        if rem < 0:
            continue
        for j in (0, -1, 1):
            qb = _step(ly + math.copysign(math.sqrt(rem), uy if uy else 1.0), j)
            q = (qb, qa) if swap else (qa, qb)
            l = (ly, lx) if swap else (lx, ly)
            if d2_device(*q, *l) == target and d2_reference(*q, *l) == target:
                return q
    raise AssertionError(("no point with d2 ==", target, "towards", (ux, uy)))


DIRECTIONS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
CLASSES = ("equal", "above", "below")                   # asked in this order: the one that closes comes last


def ring_points(lx, ly, radius, only=None):
    """{direction: {class: point}}: per direction the points whose rounded d2 is the last double below r2_threshold(radius),
    equal to it, and the first above it.  Premise: all three exist, and sqrt(d2) < radius holds for "below" alone."""
    r2 = r2_threshold(radius)
    targets = {"below": math.nextafter(r2, 0.0), "equal": r2, "above": math.nextafter(r2, math.inf)}
    out = {}
    for u in DIRECTIONS:
        out[u] = {c: edge_point(lx, ly, *u, targets[c]) for c in CLASSES if only is None or only == (u, c)}
        for c, q in out[u].items():
            assert d2_device(*q, lx, ly) == targets[c]
            assert (math.sqrt(d2_reference(*q, lx, ly)) < radius) == (c == "below")
            assert (d2_device(*q, lx, ly) < r2) == (c == "below")
    return out


RING_RADII = (0.6, 0.3, 0.45, 1.0)          # tests/test_gpu_parity.py, test_closure_constants_other_than_the_reference
RING_VARIANTS = ("t5", "t7", "old", "lds")


def _ask_ring(b, pts, t, node):
    """Every asker is a landmark itself, within the radius of its neighbours on the ring.  So the sixteen that must find
    nothing come first, on consecutive nodes -- too young for each other --, and then the eight that close: on L, the first in
    list order whatever lies around.  Returns {(direction, class): what ask() returned}."""
    assert 2 * len(DIRECTIONS) < b.min_between
    out, n0 = {}, b.sc.n_nodes
    for c in ("equal", "above"):
        for u in DIRECTIONS:
            out[(u, c)] = b.ask(*pts[u][c], t, None)
    assert b.sc.n_nodes == n0 + 2 * len(DIRECTIONS)
    for u in DIRECTIONS:
        out[(u, "below")] = b.ask(*pts[u]["below"], t, node)
    return out


def ring(radius, variant, nb=2, raw=True):
    """One landmark L and 24 asking points a hair inside, on and outside the radius.  Variants: "t5" a type the directory
    indexes; "t7" one it does not (the side list), and "old": 64 landmarks of another type between L and the askers, so that L
    has long left every window and ring when they come (with "t7": the window kernel has to go to the side list for it); "lds": cool-down 1 and a landmark of its own for every asker, laid at
    the node before it -- the window kernel answers from the window it keeps in LDS."""
    assert raw and variant in RING_VARIANTS
    lds = variant == "lds"
    b = Build(f"ring-{radius}-{variant}", nb, raw, min_between=1 if lds else REF["min_between"], radius=radius)
    t = 7 if variant == "t7" else 5
    b.tags |= {"ring"} | ({"side"} if t == 7 else set())
    if lds:
        k = 0
        for u in DIRECTIONS:
            for c in CLASSES:
                lx, ly = -4.03 + 3.5 * (k % 5), -4.02 + 3.5 * (k // 5)          # a place of its own, clear of the others
                q = ring_points(lx, ly, radius, only=(u, c))[u][c]
                node = b.lay(lx, ly, t)[0]
                if k == 11:
                    b.cut()
                b.ask(*q, t, node if c == "below" else None)
                k += 1
        return b.done()
    lx, ly = 0.03, -0.02
    node = b.lay(lx, ly, t)[0]
    if variant in ("old", "t7"):
        b.fillers((lx, ly))
    b.pad()
    b.cut()
    _ask_ring(b, ring_points(lx, ly, radius), t, node)
    assert len(b.sc.pairs) == len(DIRECTIONS)
    return b.done()


def ring_f32(radius, nb=2, raw=True):
    """The edge in values an f32 carries: 0.75 with Q = (0.75, 0), 0.625 with Q = (0.375, 0.5), L = (0, 0).  d2 == radius^2
    exactly: no closure; one f32 nearer: a closure; one f32 farther: none."""
    q = {0.75: (0.75, 0.0), 0.625: (0.375, 0.5)}[radius]
    f = np.float32(q[0])
    nearer, farther = float(np.nextafter(f, np.float32(0))), float(np.nextafter(f, np.float32(2)))
    r2 = r2_threshold(radius)
    assert d2_device(*q, 0.0, 0.0) == radius * radius >= r2 and math.sqrt(d2_reference(*q, 0.0, 0.0)) == radius
    assert (r2 == radius * radius) == (radius == 0.75)                  # (see the module's docstring)
    assert d2_device(nearer, q[1], 0.0, 0.0) < r2 < d2_device(farther, q[1], 0.0, 0.0)
    b = Build(f"ring_f32-{radius}", nb, raw, radius=radius, f32=True)
    b.tags |= {"ring_f32", "f32"}
    node = b.lay(0.0, 0.0, 5)[0]
    b.pad()
    b.cut()
    for qx, want in ((q[0], None), (farther, None), (nearer, node)):
        n_, px, py, a, _ = b.ask(qx, q[1], 5, want)
        assert (px, py) == (qx, q[1])                                    # (no drift yet: the pose is the value)
    return b.done()


def ring_f32_young(radius, walk, nb=2, raw=True):
    """ring_f32's three askers with a sure match M next to them, laid after L: on the radius and beyond it the answer is M, a
    hair inside it is L, the older.  Every asker comes a cool-down after its bot's event before -- a far-away one that finds
    nothing, for the first --, which is what lets a scout stage its rows (tests/chain_scout_rules.py): the decision is
    settled from the first rows, the owner's own or the staged ones.  walk: seven landmarks out of reach fill the first node
    of L's bucket, so L is the first entry of the second and only a walk from a first-round match finds it -- the lean
    owner's own loop."""
    q = {0.75: (0.75, 0.0), 0.625: (0.375, 0.5)}[radius]
    far = {0.75: (-0.375, -0.375), 0.625: (-0.5, -0.5)}[radius]
    f = np.float32(q[0])
    nearer, farther = float(np.nextafter(f, np.float32(0))), float(np.nextafter(f, np.float32(2)))
    r2 = r2_threshold(radius)
    assert d2_device(*q, 0.0, 0.0) == radius * radius >= r2 and math.sqrt(d2_reference(*q, 0.0, 0.0)) == radius
    assert d2_device(nearer, q[1], 0.0, 0.0) < r2 < d2_device(farther, q[1], 0.0, 0.0)
    b = Build(f"ring_f32_{'walk' if walk else 'young'}-{radius}", nb, raw, radius=radius, f32=True)
    b.tags |= {"ring_f32", "f32"}
    if walk:
        for _ in range(CAP):
            b.lay(*far, 5)
        assert math.dist(far, q) > 1.2 * radius
    l = b.lay(0.0, 0.0, 5)
    m = b.lay(q[0] + 0.0625, q[1] + 0.0625, 5)
    assert b.g.cell(*m[1:]) == b.g.cell(*q) != b.g.cell(0.0, 0.0) and (not walk or b.g.cell(*far) == b.g.cell(0.0, 0.0))
    b.pad()
    b.cut()
    asked = []
    for qx, want in ((q[0], m[0]), (farther, m[0]), (nearer, l[0])):
        agent = next(b._askers)
        b.ask(-3.0, -3.0 - 1.5 * len(asked), 5, None, agent=agent)           # (a decision before it in every launch)
        b.pad()
        n_, px, py, _, _ = b.ask(qx, q[1], 5, want, agent=agent)
        assert (px, py) == (qx, q[1]) or not raw and nb == 2                # (the first asker of a bot has no drift yet)
        asked.append((n_, px, py, want))
    sc = b.done()
    ch = sc.chains()
    for n_, px, py, want in asked:
        for rule in ("last", "ahead"):
            assert ch.query(px, py, 5, n_ - sc.min_between, rule)[:3] == (want, 2 if walk else 1, True)
    return sc


def age_edges(min_between, nb=2, raw=True):
    """A landmark at node j asked for at j + min_between - 1 (too young) and j + min_between; the bot that closed there asks
    again min_between - 1 nodes later (still cooling down) and min_between nodes later."""
    assert min_between >= 2
    b = Build(f"age_edges-{min_between}", nb, raw, min_between=min_between, f32=True)
    b.tags |= {"age", "f32"}
    j = b.lay(1.0, 1.0, 5)[0]
    b.pad(min_between - 2)
    b.cut()
    n0 = b.ask(1.125, 1.0, 5, None, agent=2)[0]
    n1, _, _, a, _ = b.ask(1.0, 1.125, 5, j, agent=nb)
    assert (n0, n1) == (j + min_between - 1, j + min_between)
    b.pad(min_between - 2)
    n2, _, _, _, q2 = b.ask(0.875, 1.0, 5, None, agent=a, wait=False)
    n3, _, _, _, q3 = b.ask(1.0, 0.875, 5, j, agent=a, wait=False)
    assert (n2, n3) == (n1 + min_between - 1, n1 + min_between) and not q2 and q3
    return b.done()


def _f32_below(v):
    f = np.float32(v)
    return float(f if f < v else np.nextafter(f, np.float32(-np.inf)))


def _f32_above(v):
    f = np.float32(v)
    return float(f if f > v else np.nextafter(f, np.float32(np.inf)))


def cell_edges(nb=2, raw=True):
    """Pairs closer than the radius on either side of a cell boundary in x, in y and across a corner; at the boundary's own
    coordinate b0 + k*cell and the doubles (f32s on the packet route) next to it; across cells -1 | 0 below the origin; the
    same at x ~ 1e6; and pairs farther than the radius in adjacent cells.  Premise: Geometry.cell puts the poses there."""
    b = Build("cell_edges", nb, raw)
    b.tags |= {"cells"} | ({"f32"} if not raw else set())
    g, (ox, oy) = b.g, b.world[2:]
    cell = b.radius * (1.0 + 1e-9)
    lo, hi = (_f32_below, _f32_above) if b.f32 else (lambda v: v, lambda v: v)
    pairs = []                                                          # (landmark, asker, cell step wanted, closes)

    def first_in(k, axis):
        """The smallest double of cell k along an axis (0: x, 1: y)."""
        v = (ox, oy)[axis] + k * cell
        one = (lambda w: g.cell(w, oy)[0]) if axis == 0 else (lambda w: g.cell(ox, w)[1])
        while one(v) >= k:
            v = math.nextafter(v, -math.inf)
        while one(v) < k:
            v = math.nextafter(v, math.inf)
        return v

    kf = int(round((1.0e6 - ox) / cell))
    bf = first_in(kf, 0)                                               # far outside the world: first (no drift yet on any route)
    pairs.append(((lo(bf - 0.125), 0.7), (hi(bf + 0.125), 0.7), (1, 0), True))
    pairs.append(((lo(bf - 0.4375), 2.7), (hi(bf + 0.4375), 2.7), (1, 0), False))
    bx, by = first_in(8, 0), first_in(9, 1)
    pairs.append(((bx - 0.125, -3.0), (bx + 0.125, -3.0), (1, 0), True))                # a boundary in x
    pairs.append(((-3.0, by - 0.125), (-3.0, by + 0.125), (0, 1), True))                # in y
    pairs.append(((bx - 0.125, 3.0 + by - 0.125), (bx + 0.125, 3.0 + by + 0.125), None, True))   # a corner (checked below)
    pairs.append(((bx + 0.125, -1.8 + by - 0.125), (bx - 0.125, -1.8 + by + 0.125), None, True))  # the other diagonal
    pairs.append(((bx - 0.375, 2.0), (bx + 0.375, 2.0), (1, 0), False))                 # adjacent cells, too far
    pairs.append(((-1.5, by - 0.375), (-1.5, by + 0.375), (0, 1), False))
    pairs.append(((ox - 0.125, -1.5), (ox + 0.125, -1.5), (1, 0), True))                # cells -1 | 0
    pairs.append(((1.5, oy - 0.125), (1.5, oy + 0.125), (0, 1), True))
    pairs.append(((ox - 0.125, oy - 0.125), (ox + 0.125, oy + 0.125), (1, 1), True))
    pairs.append(((ox - 0.75, 0.5), (ox - 0.5, 0.5), (1, 0), True))                     # cells -2 | -1
    # the boundary's own coordinate and its neighbours, asked from both sides
    e = first_in(12, 0)
    on = (_f32_below(e), _f32_above(e), _f32_above(_f32_above(e))) if b.f32 else (math.nextafter(e, -math.inf), e, ox + 12 * cell)
    assert g.cell(on[0], 0.0)[0] == 11 and g.cell(on[1], 0.0)[0] == 12
    for i, v in enumerate(on):
        pairs.append(((v, 3.5 - 1.5 * i), (v - 0.25, 3.5 - 1.5 * i), None, True))
        pairs.append(((v, 4.25 - 1.5 * i), (v + 0.25, 4.25 - 1.5 * i), None, True))
    laid = [b.lay(*p[0], 5) for p in pairs]
    b.pad()
    b.cut()
    for (l, q, step, closes), (node, lx, ly) in zip(pairs, laid):
        _, px, py, _, _ = b.ask(*q, 5, node if closes else None)
        cl, cq = g.cell(lx, ly), g.cell(px, py)
        if step is not None:
            assert (cq[0] - cl[0], cq[1] - cl[1]) == step, (b.name, l, q, cl, cq)
        assert max(abs(cq[0] - cl[0]), abs(cq[1] - cl[1])) <= 1
    c0 = [g.cell(*p[:2]) for p in b.sc.landmarks]
    assert min(c[0] for c in c0) == -2 and min(c[1] for c in c0) == -1 and max(c[0] for c in c0) >= kf
    # the corners really are diagonal neighbours
    for i in (4, 5):
        cl = g.cell(*laid[i][1:])
        cq = [g.cell(x, y) for (x, y, _, n) in b.sc.landmarks if (laid[i][0], n) in b.sc.pairs][0]
        assert abs(cq[0] - cl[0]) == 1 and abs(cq[1] - cl[1]) == 1
    return b.done()


def _cells_of(world, radius):
    size, res = WORLDS[world][:2]
    return int(math.ceil(size * res / (radius * (1.0 + 1e-9))))


def _centre(world, radius, c):
    cell = radius * (1.0 + 1e-9)
    return WORLDS[world][2] + (c[0] + 0.5) * cell, WORLDS[world][3] + (c[1] + 0.5) * cell


@functools.lru_cache(maxsize=None)
def far_cells(world, radius=REF["radius"], t=5):
    """Two cells of the world more than two cells apart on one table entry (searched for)."""
    g, n = Geometry(*WORLDS[world], radius), _cells_of(world, radius)
    cells = [(cx, cy) for cy in range(n) for cx in range(n)]
    for c1 in cells:
        for c2 in cells:
            if c2 > c1 and max(abs(c1[0] - c2[0]), abs(c1[1] - c2[1])) > 2 and g.key(t, *c1) == g.key(t, *c2):
                return c1, c2
    raise AssertionError("no two far cells share a table entry")


FAR_COUNTS = (7, 8, 15)          # C1's landmarks: the first node exactly full / the first pool node begun / C2's entry in the third node


def far_collision(world, n1, nb=2, raw=True):
    """n1 landmarks in C1, one in C2 on the same table entry, far away: the asker at C2 finds C1's rows first."""
    b = Build(f"far_collision-{world}-{n1}", nb, raw, world=world, f32=True)
    b.tags |= {"far", "f32"}
    c1, c2 = far_cells(world)
    assert b.g.key(5, *c1) == b.g.key(5, *c2) and max(abs(c1[0] - c2[0]), abs(c1[1] - c2[1])) > 2
    p1, p2 = _centre(world, b.radius, c1), _centre(world, b.radius, c2)
    first = [b.lay(*p1, 5) for _ in range(n1)]
    l2 = b.lay(*p2, 5)
    assert all(b.g.cell(x, y) == c1 for _, x, y in first) and b.g.cell(*l2[1:]) == c2
    b.pad()
    b.cut()
    n2, qx, qy, _, _ = b.ask(p2[0] + 0.125, p2[1] + 0.0625, 5, l2[0])
    b.ask(p1[0] + 0.125, p1[1] + 0.0625, 5, first[0][0])
    sc = b.done()
    m, rounds, lean, _ = sc.chains().query(qx, qy, 5, n2 - sc.min_between, "ahead")
    assert m == l2[0] and rounds == n1 // CAP + 1 > 1 and not lean
    return sc


@functools.lru_cache(maxsize=None)
def neighbour_cells(world, radius=REF["radius"], t=5):
    """(c, a, b, pa, pb, pn): a cell c two of whose nine neighbours a, b share a table entry, and points of c within the radius of
    a's centre alone, of b's alone, and of neither (searched for)."""
    g, n = Geometry(*WORLDS[world], radius), _cells_of(world, radius)
    cell = radius * (1.0 + 1e-9)
    for cy in range(n):
        for cx in range(n):
            nine = [(cx + i, cy + j) for j in (-1, 0, 1) for i in (-1, 0, 1)]
            for a, b in itertools.combinations(nine, 2):
                if g.key(t, *a) != g.key(t, *b):
                    continue
                la, lb = _centre(world, radius, a), _centre(world, radius, b)
                x0, y0 = WORLDS[world][2] + cx * cell, WORLDS[world][3] + cy * cell
                pts = [(x0 + cell * (i + 0.5) / 16, y0 + cell * (j + 0.5) / 16) for i in range(16) for j in range(16)]
                da = lambda p: math.dist(p, la) / radius
                db = lambda p: math.dist(p, lb) / radius
                pa = [p for p in pts if da(p) < 0.9 and db(p) > 1.1]
                pb = [p for p in pts if db(p) < 0.9 and da(p) > 1.1]
                pn = [p for p in pts if da(p) > 1.1 and db(p) > 1.1]
                if pa and pb and pn:
                    return (cx, cy), a, b, pa[0], pb[0], pn[0]
    raise AssertionError("no cell with two neighbours on one table entry")


def neighbour_collision(world, nb=2, raw=True):
    """Two of a cell's nine neighbours on one table entry: their landmarks interleaved in one chain, asked from that cell."""
    b = Build(f"neighbour_collision-{world}", nb, raw, world=world, f32=True)
    b.tags |= {"neighbour", "f32"}
    c, ca, cb, pa, pb, pn = neighbour_cells(world)
    nine = [b.g.key(5, c[0] + i, c[1] + j) for j in (-1, 0, 1) for i in (-1, 0, 1)]
    assert len(set(nine)) < 9 and b.g.key(5, *ca) == b.g.key(5, *cb) and ca != cb
    la, lb = _centre(world, b.radius, ca), _centre(world, b.radius, cb)
    laid = [b.lay(*(la if k % 2 == 0 else lb), 5) for k in range(10)]
    assert all(b.g.cell(x, y) == (ca if k % 2 == 0 else cb) for k, (_, x, y) in enumerate(laid))
    b.pad()
    b.cut()
    asked = [b.ask(*pn, 5, None), b.ask(*pb, 5, laid[1][0]), b.ask(*pa, 5, laid[0][0])]
    assert all(b.g.cell(x, y) == c for _, x, y, _, _ in asked)
    return b.done()


def types_share_cells(nb=2, raw=True):
    """Types 1..5 and 7 laid at one point: an asker of each type matches its own, one of type 6 nothing."""
    b = Build("types_share_cells", nb, raw, f32=True)
    b.tags |= {"types", "side", "f32"}
    node = {t: b.lay(1.0, -2.0, t)[0] for t in (3, 1, 7, 5, 2, 4)}
    b.fillers((1.0, -2.0))
    b.pad()
    b.cut()
    for k, t in enumerate((5, 6, 1, 7, 4, 2, 3)):
        b.ask(1.0 + 0.0625 * (k - 3), -2.125, t, node.get(t))
    return b.done()


PILE = 7 * 66 + 3                # tests/test_gpu_chain_plan.py, test_landmark_pile: as small as raises the pile flag
P_ = (0.05, 0.05)                # tests/k4_adversarial.py's pile
DENSE_AFTER = 8                  # node rounds before a query of the DENSE variant scans the log (csrc/slam.hip)


def dense_ring(shift=0, nb=2, raw=True):
    """The pile at P, then ring(0.6)'s landmark in the bucket diagonally next to it, laid after the pile, then the askers.
    Those towards the pile have its bucket among their nine: "below" holds a match younger than the pile and walks it, the
    others find nothing and walk it -- past DENSE_AFTER rounds, into the scan of the log and its own distance test.
    shift: landmarks of another type laid between the pile and L.  The window kernel scans the log 128 entries a round with a
    comparison of its own for either half: without a shift L is in the second half of its round, with 64 in the first."""
    assert raw and shift in (0, 64)
    b = Build("dense_ring" + (f"-{shift}" if shift else ""), nb, raw, world=512)
    b.tags |= {"dense", "ring"}
    for _ in range(PILE):
        b.lay(*P_, 5, quiet=False)
    n_own = len(b.sc.pairs)
    lx, ly = 0.95, 0.95
    if shift:
        b.fillers((lx, ly), shift)
    node = b.lay(lx, ly, 5)[0]
    assert (len(b.sc.landmarks) - 1) % 128 // 64 == (0 if shift else 1)
    cp, cl = b.g.cell(*P_), b.g.cell(lx, ly)
    assert (cl[0] - cp[0], cl[1] - cp[1]) == (1, 1) and b.g.key(5, *cp) != b.g.key(5, *cl)
    b.pad()
    b.cut()
    pts = ring_points(lx, ly, b.radius)
    assert all(math.dist(pts[u][c], P_) > 1.1 * b.radius for u in DIRECTIONS for c in CLASSES)
    asked = _ask_ring(b, pts, 5, node)
    sc = b.done()
    ch, walked = sc.chains(), 0
    assert ch.length(*P_, 5) > 64 * CAP                                       # a pile
    for u in DIRECTIONS:
        r = [ch.query(asked[(u, c)][1], asked[(u, c)][2], 5, asked[(u, c)][0] - sc.min_between, "last")[1] for c in CLASSES]
        walked += all(v > DENSE_AFTER for v in r)
    assert walked >= 3 and len(sc.ref["pairs"]) == n_own + len(DIRECTIONS)
    return sc


def graphs_case():
    """(x, y, agent, type, closure parameters): types_share_cells for three bots, twice over, cool-down 1 -- for graphs of one
    bot each, where a bot's second pass closes on its own first and on nobody else's."""
    sc = scene("types_share_cells", 3, True)
    x, y, agent, lm = (np.concatenate([v, v]) for v in (sc.x, sc.y, sc.agent, sc.type))
    return x, y, agent, lm, dict(radius=sc.radius, min_between=1, correction=sc.correction)


# ---- the registry ---------------------------------------------------------------------------------------------------------------
_MAKERS = {}
for _r in RING_RADII:
    for _v in RING_VARIANTS:
        _MAKERS[f"ring-{_r}-{_v}"] = functools.partial(ring, _r, _v)
for _r in (0.75, 0.625):
    _MAKERS[f"ring_f32-{_r}"] = functools.partial(ring_f32, _r)
    _MAKERS[f"ring_f32_young-{_r}"] = functools.partial(ring_f32_young, _r, False)
    _MAKERS[f"ring_f32_walk-{_r}"] = functools.partial(ring_f32_young, _r, True)
for _m in (30, 3):
    _MAKERS[f"age_edges-{_m}"] = functools.partial(age_edges, _m)
_MAKERS["cell_edges"] = cell_edges
for _w in (200, 64):
    for _n in FAR_COUNTS:
        _MAKERS[f"far_collision-{_w}-{_n}"] = functools.partial(far_collision, _w, _n)
    _MAKERS[f"neighbour_collision-{_w}"] = functools.partial(neighbour_collision, _w)
_MAKERS["types_share_cells"] = types_share_cells
_MAKERS["dense_ring"] = functools.partial(dense_ring, 0)
_MAKERS["dense_ring-64"] = functools.partial(dense_ring, 64)
SCENES = tuple(_MAKERS)
RAW_ONLY = tuple(n for n in SCENES if n.startswith(("ring-", "dense_ring")))    # values an f32 does not carry
PACKET = tuple(n for n in SCENES if n not in RAW_ONLY)
SMALLEST_RING = "ring-0.6-t5"


@functools.lru_cache(maxsize=None)
def scene(name, nb=2, raw=True):
    """The scene, built once and shared (read only): .x .y .agent .type, .cuts, .ref (the scan's answer), .want."""
    assert raw or name in PACKET
    sc = _MAKERS[name](nb=nb, raw=raw)
    assert sc.name == name
    return sc
