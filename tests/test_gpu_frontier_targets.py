"""Frontier target assignment on the device (qs_frontier_targets) against a restatement of the reference's greedy
loop, dual_bot_mapper.py:947-996 (commented out there), fed by QuasarMapper.frontier_centroids().

Rules restated here:
  1. centroids: the clusters of cluster_frontiers with size >= min_cluster, in that order (frontier_centroids());
  2. bots in the order given (the reference: online bots, ascending id, at their last accepted pose);
  3. each bot skips centroids already taken and centroids within `separation` (sqrt(dx*dx + dy*dy) < separation) of any
     target assigned so far, and takes the smallest sqrt((bx-cx)*(bx-cx) + (by-cy)*(by-cy)) by strict `<` from inf,
     so ties go to the lowest index;
  4. no target when nothing qualifies (a NaN or inf position included: NaN < inf and inf < inf are false).
Results must be bit-equal: indices, and float64 coordinates compared with ==."""
import math

import numpy as np
import pytest

from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu
INF = float("inf")
K = 32          # QS_FT_K


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def oracle_targets(cents, bots, sep):
    """Rules 2-4 with numpy's elementwise fp64 (the same IEEE operations as CPython floats; nothing is fused)."""
    C = np.asarray(cents, dtype=np.float64).reshape(-1, 2)
    cx, cy = C[:, 0], C[:, 1]
    ok = np.ones(len(C), dtype=bool)
    idx = np.full(len(bots), -1, dtype=np.int64)
    xy = np.full((len(bots), 2), np.nan)
    for b, (bx, by) in enumerate(bots):
        if not len(C):
            break
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = bx - cx, by - cy
            d = np.sqrt(dx * dx + dy * dy)
            d = np.where(ok & (d < INF), d, INF)
        i = int(np.argmin(d))                     # the first of equal minima: the lowest index
        if not d[i] < INF:
            continue
        idx[b], xy[b] = i, C[i]
        ok[i] = False                             # taken
        ex, ey = cx - C[i, 0], cy - C[i, 1]
        ok &= ~(np.sqrt(ex * ex + ey * ey) < sep)  # too close to this target
    return idx, xy


def oracle_targets_py(cents, bots, sep):
    """The same rules as the reference's loop shape, plain Python floats (small inputs only)."""
    targets, taken, out = [], set(), []
    for bx, by in bots:
        best, bi = INF, -1
        for i, (cx, cy) in enumerate(cents):
            if i in taken:
                continue
            if any(math.sqrt((cx - tx) * (cx - tx) + (cy - ty) * (cy - ty)) < sep for tx, ty in targets):
                continue
            dx, dy = bx - cx, by - cy
            try:
                d = math.sqrt(dx * dx + dy * dy)
            except ValueError:
                d = math.nan
            if d < best:
                best, bi = d, i
        out.append(bi)
        if bi >= 0:
            taken.add(bi)
            targets.append(tuple(cents[bi]))
    return np.array(out, dtype=np.int64)


def check(m, bots, sep, min_cluster=3):
    bots = np.asarray(bots, dtype=np.float64).reshape(-1, 2)
    idx, xy, cents, st = m.frontier_targets(bots, separation=sep, min_cluster=min_cluster, return_centroids=True)
    ref_c = np.array(m.frontier_centroids(min_cluster), dtype=np.float64).reshape(-1, 2)
    assert cents.shape == ref_c.shape and (cents == ref_c).all()
    assert st["n_centroids"] == len(ref_c) and st["k"] == K
    oi, oxy = oracle_targets(ref_c, [tuple(b) for b in bots.tolist()], sep)
    assert (idx == oi).all(), (sep, min_cluster, np.nonzero(idx != oi)[0][:8])
    a = oi >= 0
    assert (xy[a] == oxy[a]).all() and np.isnan(xy[~a]).all()
    return idx, st


def last_poses(m, stream):
    """bot_states: the pose of each bot's last accepted packet (:850-866), ascending id."""
    acc, pose = m.last_batch()
    agents = stream[:, 4]
    last = {}
    for i in np.nonzero(acc)[0]:
        last[int(agents[i])] = (float(pose[i, 0]), float(pose[i, 1]))
    return [last[b] for b in sorted(last)]


def _replay(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".replay")


def test_centroids_on_golden_sessions(pkg):
    for name in ("session_512", "session_4096"):
        g = np.load(f"{GOLDEN}/{name}.npz", allow_pickle=False)
        size, res, ox, oy, sep = g["cfg"]
        with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as m:
            m.ingest_array(g["datagrams"], g["lengths"])
            for mc in (1, 3, 5):
                _, st = check(m, [(0.0, 0.0), (1.0, -1.0)], 1.0, mc)
                assert st["n_centroids"] > 0


@pytest.fixture(scope="module")
def map64(pkg):
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    stream = replay.multi_bot_stream(session, 64, 64 * 400)
    m = pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2)
    m.ingest_array(stream)
    yield m, last_poses(m, stream)
    m.close()


@pytest.mark.parametrize("sep", [1.0, 0.0, 0.3])
def test_assignment_64_bots_4096(map64, sep):
    m, bots = map64
    assert len(bots) == 64
    for mc in (1, 3, 1 << 30):
        idx, st = check(m, bots, sep, mc)
        if mc == 1 << 30:
            assert st["n_centroids"] == 0 and (idx == -1).all()
        else:
            assert st["n_centroids"] > 100 and (idx >= 0).sum() > 32
    want = {b: tuple(xy) for b, xy in zip(range(1, 65), oracle_targets(m.frontier_centroids(), bots, sep)[1].tolist())
            if not math.isnan(xy[0])}
    assert m.assign_frontier_targets(dict(zip(range(1, 65), bots)), separation=sep) == want


def test_assignment_255_bots(pkg):
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    stream = replay.multi_bot_stream(session, 255, 255 * 500)
    with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=255) as m:
        m.ingest_array(stream)
        bots = last_poses(m, stream)
        assert len(bots) == 255
        for sep in (1.0, 0.0, 0.3):
            for mc in (1, 3, 1 << 30):
                idx, st = check(m, bots, sep, mc)
                if mc != 1 << 30:
                    assert (idx >= 0).sum() > 128


# ---- adversarial maps built ray by ray ------------------------------------------------------------------------
def lattice_rays(nx, ny, sx, sy, x0=-20.0, y0=-20.0):
    """One 4-cell horizontal ray per lattice site: a cluster of 4 free cells each, binary-exact centroids."""
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny))
    rx = x0 + gx.ravel() * sx + 0.125
    ry = y0 + gy.ravel() * sy + 0.125
    return rx, ry, rx + 1.0, ry.copy(), np.ones(len(rx), dtype=np.uint8)


def lattice_mapper(pkg, nx, ny, sx, sy):
    m = pkg.QuasarMapper(256, 0.25, -32.0, -32.0)
    m.update_rays(*lattice_rays(nx, ny, sx, sy))
    return m


def squares_agree(bots, cents):
    """d**2 == d*d on every bot-centroid difference (libm's pow is not correctly rounded everywhere: where it is not,
    the reference's `**2` and the device's x*x could differ, and such data would test libm, not the kernel).
    Differences too large to square finitely are skipped: their keys are inf whichever way they are squared."""
    for bx, by in bots:
        for cx, cy in cents:
            for d in (bx - cx, by - cy):
                if math.isfinite(d) and abs(d) < 1e150 and d ** 2 != d * d:
                    return False
    return True


def order_inversion(cents):
    """A bot position where two centroids i < j have d2_i > d2_j yet sqrt(d2_i) == sqrt(d2_j): ordering by d2 alone
    would pick j, the reference picks i."""
    top = float(cents[:, 1].max())
    row = np.nonzero(cents[:, 1] == top)[0]
    i, j = int(row[0]), int(row[1])
    (xi, yi), (xj, yj) = cents[i].tolist(), cents[j].tolist()
    mid = (xi + xj) / 2
    for k in range(1, 2000):
        by = top + 1000.0 + k * 0.37
        for t in range(1, 400):
            bx = mid + t * 2.0 ** -40
            di = (bx - xi) * (bx - xi) + (by - yi) * (by - yi)
            dj = (bx - xj) * (bx - xj) + (by - yj) * (by - yj)
            if di > dj and math.sqrt(di) == math.sqrt(dj) and squares_agree([(bx, by)], cents.tolist()):
                return (bx, by), i, j
    raise AssertionError("no order inversion found")


def test_adversarial_lattice(pkg):
    with lattice_mapper(pkg, 6, 5, 2.0, 1.5) as m:
        cents = np.array(m.frontier_centroids(), dtype=np.float64)
        assert len(cents) == 30 and len(set(map(tuple, cents.tolist()))) == 30
        inv, i, j = order_inversion(cents)
        c0, c1, c6 = cents[0].tolist(), cents[1].tolist(), cents[6].tolist()
        tie2 = ((c0[0] + c1[0]) / 2, c0[1])                          # exactly equidistant from clusters 0 and 1
        tie4 = ((c0[0] + c1[0]) / 2, (c0[1] + c6[1]) / 2)            # ... from 0, 1, 6 and 7
        rng = np.random.default_rng(7)
        rand = [p for p in map(tuple, rng.uniform(-22.0, -8.0, (60, 2)).tolist()) if squares_agree([p], cents.tolist())][:30]
        assert len(rand) == 30
        bots = ([inv, tie2, tie4, tie2, tie4, (math.nan, 0.0), (INF, -INF), (0.0, math.nan), (-INF, 3.0),
                 (1e6, -1e6), (1e200, 0.0), tie4] + rand + rand[:5] + [tie2] * 3)
        assert len(bots) > len(cents)                                # more bots than centroids
        # the test data: d**2 == d*d on every difference the oracle squares (a libm misrounding would show up
        # here, not as a kernel bug); the 1e200 outlier's d*d is inf, its key is inf and it gets no target
        far = 1e200 - float(cents[0, 0])
        assert squares_agree(bots, cents.tolist()) and far * far == INF
        (bx, by), (xi, yi), (xj, yj) = inv, cents[i].tolist(), cents[j].tolist()
        di = (bx - xi) * (bx - xi) + (by - yi) * (by - yi)
        dj = (bx - xj) * (bx - xj) + (by - yj) * (by - yj)
        assert i < j and di > dj and math.sqrt(di) == math.sqrt(dj)
        for sep in (0.0, 1.0, 1.6, 2.5, 0.3, INF):
            idx, _ = check(m, bots, sep)
            assert (idx == oracle_targets_py(cents.tolist(), bots, sep)).all()
            assert idx[0] == i                                       # the lower index, not the smaller d2
            assert (idx[5:9] == -1).all() and idx[10] == -1          # NaN / inf / overflowing positions
        idx, _ = check(m, bots, 0.0)
        assert (idx >= 0).sum() == len(cents) and (idx == -1).sum() > 0
        assert idx[1] == 0 and idx[2] == 1 and idx[3] == 6          # ties: each takes the lowest free index


def test_fallback_full_scan(pkg):
    """Many bots on one spot and more than K centroids within `separation` of the first pick: every later bot's
    top-K list is entirely blocked, so the device scans every centroid for it."""
    with lattice_mapper(pkg, 20, 30, 1.5, 0.5) as m:
        cents = np.array(m.frontier_centroids(), dtype=np.float64)
        assert len(cents) == 600
        spot = (-6.0, -12.6)
        bots = [spot] * 12 + [(-19.0, -19.0), spot, (0.0, 0.0)]
        assert squares_agree(bots, cents.tolist())
        for sep in (4.0, 6.0):
            c = cents[oracle_targets(cents, [spot], 0.0)[0][0]]
            assert (np.sqrt((cents[:, 0] - c[0]) ** 2 + (cents[:, 1] - c[1]) ** 2) < sep).sum() > K
            idx, st = check(m, bots, sep)
            assert st["fallbacks"] > 0
            assert (idx == oracle_targets_py(cents.tolist(), bots, sep)).all()


# ---- life cycle -------------------------------------------------------------------------------------------------
def _session(pkg):
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    return replay, replay.multi_bot_stream(session, 8, 8 * 400)


BOTS = [(-98.0 + 8.0 * i + 1.0, -97.0) for i in range(8)] + [(-60.0, -90.0), (math.nan, 1.0)]


def _same(a, b):
    (ia, xa, ca, sa), (ib, xb, cb, sb) = a, b
    assert (ia == ib).all() and ((xa == xb) | (np.isnan(xa) & np.isnan(xb))).all()
    assert ca.shape == cb.shape and (ca == cb).all() and sa == sb


def test_after_reset(pkg):
    replay, stream = _session(pkg)
    other = replay.adversarial_stream(3000, lo=-100.0, hi=-60.0, max_agent=8)
    cfg = dict(size=2048, resolution=0.05, origin_x=-102.4, origin_y=-102.4, max_agent=8)
    with pkg.QuasarMapper(**cfg) as m, pkg.QuasarMapper(**cfg) as fresh:
        m.ingest_array(other)
        m.frontier_targets(BOTS)
        m.reset()
        m.ingest_array(stream)
        fresh.ingest_array(stream)
        for sep in (1.0, 0.0):
            got = m.frontier_targets(BOTS, separation=sep, return_centroids=True)
            _same(got, fresh.frontier_targets(BOTS, separation=sep, return_centroids=True))
            check(m, BOTS, sep)


def test_pending_edge_rays(pkg):
    """Exact-trig rays on cell boundaries wait for the host until the map is observed: the call resolves them first."""
    P = pkg.protocol
    rng = np.random.default_rng(99)
    yaws = np.radians(np.arange(24) * 15.0).astype(np.float32)
    lat = np.arange(-6, 7) * 0.05
    xs, ys, yw = np.meshgrid(lat, lat, yaws, indexing="ij")
    n = xs.size
    stream = P.pack_packets(np.ones(n, dtype=int), xs.ravel(), ys.ravel(), yw.ravel(), np.zeros(n, dtype=int),
                            np.zeros(n, dtype=int), rng.integers(3, 125, (n, 4)) * 0.01, np.zeros(n, dtype=int))
    bots = [(0.0, 0.0), (0.5, 0.5), (-1.0, 0.2), (0.0, 0.0)]
    edges = 0
    for ox in (0.0, -0.8, -1.6, -3.2):
        cfg = dict(size=64, resolution=0.05, origin_x=ox, origin_y=ox)
        with pkg.QuasarMapper(**cfg) as m, pkg.QuasarMapper(**cfg) as ref:
            m.ingest_array(stream)
            got = m.frontier_targets(bots, separation=0.3, min_cluster=1, return_centroids=True)
            edges += m.counters()["edge_rays"]
            ref.ingest_array(stream)
            ref.grid_i8()                                   # observed before the call: nothing left waiting
            _same(got, ref.frontier_targets(bots, separation=0.3, min_cluster=1, return_centroids=True))
            check(m, bots, 0.3, 1)
    assert edges > 0


def test_after_fuse(pkg):
    replay, stream = _session(pkg)
    cfg = dict(size=2048, resolution=0.05, origin_x=-102.4, origin_y=-102.4, max_agent=8)
    agents = stream[:, 4]
    with pkg.QuasarMapper(**cfg) as a, pkg.QuasarMapper(**cfg) as b:
        a.ingest_array(stream[agents <= 4])
        b.ingest_array(stream[agents > 4])
        before = a.frontier_targets(BOTS, return_centroids=True)
        a.fuse([b])
        idx, st = check(a, BOTS, 1.0)
        assert st["n_centroids"] > before[3]["n_centroids"]      # the call sees the fused map
        assert (idx[:9] >= 0).all() and idx[9] == -1


def test_arguments(pkg):
    import ctypes as C
    with lattice_mapper(pkg, 3, 3, 2.0, 1.5) as m:
        idx, xy = m.frontier_targets(np.zeros((0, 2)))
        assert idx.shape == (0,) and xy.shape == (0, 2)
        with pytest.raises(ValueError):
            m.frontier_targets(np.zeros((1025, 2)))
        L = m._L
        n = C.c_size_t()
        tidx = np.zeros(2048, dtype=np.int64)
        txy = np.zeros((2048, 2))
        pos = np.zeros((2048, 2))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.qs_frontier_targets(m._h, 3, 1.0, p(pos), 1025, p(tidx), p(txy), None, 0, C.byref(n), None) == -1
        assert b"QS_FT_MAX_BOTS" in L.qs_last_error(m._h)
        assert L.qs_frontier_targets(m._h, 3, 1.0, None, 2, p(tidx), p(txy), None, 0, C.byref(n), None) == -1
        assert L.qs_frontier_targets(m._h, 3, 1.0, p(pos), 1024, p(tidx), p(txy), None, 0, C.byref(n), None) == 0
        assert n.value == 9 and (tidx[:9] >= 0).all() and (tidx[9:1024] == -1).all()
        # the largest batch the call takes, exact as well
        rng = np.random.default_rng(3)
        bots = rng.uniform(-22.0, -12.0, (1024, 2))
        check(m, bots, 0.0, 3)
