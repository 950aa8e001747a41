"""A NumPy restatement of the loop-closure index (csrc/slam.hip, chain_insert_lanes) and of the lean owner's nine-bucket
first-match query (csrc/slam_chain_decide.inc), for tests/test_chain_lookahead_cpu.py and tests/test_gpu_chain_lookahead.py.

The index: a hash table over bucket cells of edge CLOSURE_RADIUS * (1 + 1e-9), one slab per landmark type 1..5; each bucket a
chain of nodes of seven entries in insertion order (ascending node index).  Every node also carries its look-ahead word: the
node index of its successor node's first entry, EMPTY while there is none.

The query looks at the 3 x 3 buckets round the pose, a node of each per round.  A bucket is done at its first hit (an entry
at or below `eff` and within the radius).  Without one it goes on to its next node while the node is full within the limit
(its seventh entry is at or below eff), has a successor, and
    rule "last":  the node's LAST entry lies below the best match so far       (the general query's rule),
    rule "ahead": the node's LOOK-AHEAD word lies below the best match so far  (the lean owner's, with the look-ahead on).
The lean owner only settles a decision itself if the first round has a hit; otherwise the general query takes over, rule
"last" whatever the switch says.  The answer is the lowest index among the hits: what a scan of the whole list finds first."""
import numpy as np

CAP = 7
EMPTY = 0x7F7F7F7F
NTYPES = 5


def r2_threshold(radius):
    """The largest-but-one double t with sqrt(t) < radius, as qs_api.hip works it out: d2 < t  <=>  sqrt(d2) < radius."""
    t = radius * radius
    while np.sqrt(t) >= radius:
        t = np.nextafter(t, 0.0)
    while np.sqrt(t) < radius:
        t = np.nextafter(t, np.inf)
    return float(t)


class Geometry:
    def __init__(self, size, res, ox, oy, radius):
        self.ox, self.oy = ox, oy
        cell = radius * (1.0 + 1e-9)
        self.inv = 1.0 / cell
        nbd = min(max(np.ceil(size * res / cell) + 1.0, 1.0), 1024.0)
        slab = 256
        while slab < nbd * nbd:
            slab <<= 1
        self.hmask = slab - 1
        self.r2 = r2_threshold(radius)

    def cell(self, x, y):
        return int(np.floor((x - self.ox) * self.inv)), int(np.floor((y - self.oy) * self.inv))

    def key(self, t, cx, cy):
        h = (((cx * 0x9E3779B1) & 0xFFFFFFFF) ^ ((cy * 0x85EBCA77) & 0xFFFFFFFF)) & 0xFFFFFFFF
        h ^= h >> 15
        return (t - 1) * (self.hmask + 1) + (h & self.hmask)


class Chains:
    """The bucket chains after the landmarks (xy [n, 2], types [n], node indices [n], in insertion order) were appended."""

    def __init__(self, geom, xy, types, idx):
        self.g = geom
        self.xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        self.types = np.asarray(types, dtype=np.int64)
        self.idx = np.asarray(idx, dtype=np.int64)
        assert (np.diff(self.idx) > 0).all()
        self.chain = {}
        for i in range(len(self.idx)):
            t = int(self.types[i])
            if 1 <= t <= NTYPES:
                self.chain.setdefault(geom.key(t, *geom.cell(*self.xy[i])), []).append(i)

    def length(self, x, y, t):
        return len(self.chain.get(self.g.key(t, *self.g.cell(x, y)), ()))

    def node(self, key, k):
        """Node k of a chain: (entries, look-ahead word, has a successor)."""
        c = self.chain.get(key, ())
        e = c[CAP * k:CAP * (k + 1)]
        nxt = len(c) > CAP * (k + 1)
        return e, (int(self.idx[c[CAP * (k + 1)]]) if nxt else EMPTY), nxt

    def check_lookahead(self):
        """The rule at the struct: every node's word is its successor's entry 0, EMPTY at the tail."""
        for key, c in self.chain.items():
            for k in range((len(c) + CAP - 1) // CAP):
                e, la, nxt = self.node(key, k)
                assert la == (int(self.idx[c[CAP * (k + 1)]]) if len(c) > CAP * (k + 1) else EMPTY)
                assert not nxt or la > int(self.idx[e[-1]])

    def scan(self, x, y, t, eff):
        """The reference: the first landmark of the type in list order, at or below eff and within the radius (-1: none)."""
        m = (self.types == t) & (self.idx <= eff)
        d = self.xy[m] - (x, y)
        hit = np.nonzero(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < self.g.r2)[0]
        return int(self.idx[m][hit[0]]) if len(hit) else -1

    def query(self, x, y, t, eff, rule):
        """(match or -1, rounds, settled by the lean owner, the first round's match or -1).  rule: "last" or "ahead"."""
        cx, cy = self.g.cell(x, y)
        keys = [self.g.key(t, cx + (b % 3) - 1, cy + (b // 3) - 1) for b in range(9)]
        at = [0] * 9                       # the node every bucket is at; -1: done
        best = EMPTY
        rounds, lean, first = 0, True, -1
        while any(k >= 0 for k in at):
            rounds += 1
            full, ends, ahead, succ = [False] * 9, [0] * 9, [0] * 9, [False] * 9
            hitb = [False] * 9
            for b in range(9):
                if at[b] < 0:
                    continue
                e, la, nxt = self.node(keys[b], at[b])
                for i in e:
                    if self.idx[i] <= eff:
                        dx, dy = x - self.xy[i, 0], y - self.xy[i, 1]
                        if dx * dx + dy * dy < self.g.r2:
                            hitb[b] = True
                            best = min(best, int(self.idx[i]))
                            break
                full[b] = len(e) == CAP and self.idx[e[-1]] <= eff
                ends[b] = int(self.idx[e[-1]]) if len(e) == CAP else EMPTY
                ahead[b], succ[b] = la, nxt
            if rounds == 1:
                first = best if best != EMPTY else -1
                lean = best != EMPTY       # nothing in the first rows: the general query, its own rule
            use = ahead if (rule == "ahead" and lean) else ends
            for b in range(9):
                if at[b] >= 0:
                    at[b] = at[b] + 1 if (not hitb[b] and full[b] and succ[b] and use[b] < best) else -1
        return (best if best != EMPTY else -1), rounds, lean, first


def replay(geom, xy, ti, closures, min_between, rule):
    """Every closure (matched landmark, closing node) of a graph replayed as a query at the closing node's own landmark pose
    against the chains as of its limit.  Returns (matches [n], rounds [n], settled-by-the-lean-owner [n], first-round matches [n])."""
    ch = Chains(geom, xy, ti[:, 0], ti[:, 1])
    where = {int(n): i for i, n in enumerate(ch.idx)}
    out = []
    for _, node in closures:
        i = where[int(node)]
        out.append(ch.query(ch.xy[i, 0], ch.xy[i, 1], int(ch.types[i]), int(node) - max(min_between, 1), rule))
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.int64),
            np.array([o[2] for o in out], dtype=bool), np.array([o[3] for o in out], dtype=np.int64))


def new_nodes_per_batch(ch, batch=64):
    """The chains filled again the way a restore fills them -- the log in batches of `batch` entries -- : per batch, the
    number of new pool nodes every bucket needs ({key: nodes})."""
    have, out = {}, []
    for lo in range(0, len(ch.idx), batch):
        add = {}
        for i in range(lo, min(lo + batch, len(ch.idx))):
            t = int(ch.types[i])
            if 1 <= t <= NTYPES:
                k = ch.g.key(t, *ch.g.cell(*ch.xy[i]))
                add[k] = add.get(k, 0) + 1
        new = {}
        for k, n in add.items():
            tot = have.get(k, 0) + n
            nn = max(0, -(-tot // CAP) - 1) - max(0, -(-have.get(k, 0) // CAP) - 1)
            if nn:
                new[k] = nn
            have[k] = tot
        out.append(new)
    return out


# ---- the scenes of tests/test_gpu_chain_lookahead.py: bots that stand at a few places, every packet a node and a landmark ----
# Grid origin -12.8, buckets of 0.6: A and B share a cell, Q lies in the next one; B is within the radius of Q (0.55), A is not
# (1.05).  D / E: the same one row up.  FAR: out of everybody's reach; a bot parked there closes on itself, correction 0.
GRID = (512, 0.05, -12.8, -12.8)
RADIUS = 0.6
A, B, Q = (0.45, 0.05), (0.95, 0.05), (1.5, 0.05)
D, E, R = (0.45, 3.05), (0.95, 3.05), (1.5, 3.05)
FAR = (6.05, 6.05)


def scene_legs(name):
    """((agent, place, packets), ...) of a scene.  Bot 1 lays the landmarks and then parks at FAR for 40 packets (past every
    cool-down the tests use); bot 2 queries from Q (and bot 3 from R)."""
    pad = (1, FAR, 40)
    ask = (2, Q, 3)
    return {
        # seven out of reach, the eighth in reach and older than the match in the query's own bucket: a closure only a walk finds
        "deciding": ((1, A, 7), (1, B, 1), (1, Q, 1), pad, ask),
        # ... the same with the deciding entry in the third node
        "third": ((1, A, 14), (1, B, 1), (1, Q, 1), pad, ask),
        # the successor starts above the match: the walk finds nothing older, and is not started with the look-ahead
        "avoid": ((1, A, 7), (1, Q, 1), (1, B, 1), pad, ask),
        "len7": ((1, A, 7), (1, Q, 1), pad, ask),
        "len8": ((1, A, 8), (1, Q, 1), pad, ask),
        "len14": ((1, A, 14), (1, Q, 1), pad, ask),
        "len15": ((1, A, 14), (1, Q, 1), (1, B, 1), pad, ask),
        # 22 in a row for one bucket (three pool nodes in one batch of a restore), the deciding entry in the fourth node
        "batch": ((1, A, 21), (1, B, 1), (1, Q, 1), pad, ask),
        # two buckets that need pool nodes in the same batch, a deciding entry in each
        "two": ((1, A, 7), (1, D, 7), (1, B, 1), (1, E, 1), (1, Q, 1), (1, R, 1), pad, ask, (3, R, 3)),
    }[name]


def scene_stream(name, lm=5):
    """(packets uint8 [n, 42], the position of the first asking packet: what lies before it lays and pads)."""
    return legs_stream(scene_legs(name), lm)


def legs_stream(legs, lm=5):
    from conftest import load_pkg
    agent = np.concatenate([np.full(n, a) for a, _, n in legs])
    x = np.concatenate([np.full(n, p[0]) for _, p, n in legs])
    y = np.concatenate([np.full(n, p[1]) for _, p, n in legs])
    n = len(agent)
    z = np.zeros(n, dtype=int)
    s = np.ascontiguousarray(load_pkg().pack_packets(agent, x, y, np.zeros(n), z, z, np.zeros((n, 4)), np.full(n, lm)))
    s.setflags(write=False)
    return s, int(np.argmax(agent != 1))


SCENES = ("deciding", "third", "avoid", "len7", "len8", "len14", "len15", "batch", "two")
# what the look-ahead does to the number of the askers' decisions that walk a bucket (what slam_node_iters counts): "fewer" (a
# walk is avoided), "same" (nothing can be avoided -- in len15 the walk goes on, but ends a round earlier)
EXPECT = {"deciding": "same", "third": "same", "avoid": "fewer", "len7": "same", "len8": "same", "len14": "same",
          "len15": "same", "batch": "same", "two": "same"}
