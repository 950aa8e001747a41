"""The host-side state machine around the kernels: qs_reset, the dense and the sparse fuse, qs_dirty_tracking and
qs_counts_source, driven in the orders production drives them (bench.py resets every step, dist.ShardedMapper fuses after
every batch, an exchange can fail between qs_sparse_fuse_begin and qs_sparse_fuse_apply) and in orders nobody planned.

N contexts of one process play N ranks (dist.sparse_fuse_local, device-to-device copies in the collectives' place); rank r
has its own oracle fed the same slices with set_sequence(r, N).  After a fuse every rank must hold stamps = element-wise MAX
and counts() = SUM over the ranks' oracles as they stood at that fuse; before the session's first fuse a rank shows its own
oracle.  A fuse that no rank applied (the exchange "failed": plan / apply are simply not called) must be carried in full by
the next one.  A reset context must be indistinguishable from a newly created one."""
import hashlib
import importlib
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import GOLDEN, load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
FLOAT_TOL = 1e-5
GEO = dict(pitch=5.0, tiles_per_row=8, origin=(-22.0, -20.0))        # rooms 5 m apart: neighbours share blocks
GRIDS = {"260": (260, 0.2, 26.0), "1024": (1024, 0.05, 25.6)}        # 260: the last 16-cell block of a row is 4 cells wide


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def mods(pkg):
    return importlib.import_module(pkg.__name__ + ".dist"), importlib.import_module(pkg.__name__ + ".replay")


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)


def _logodds(hits, misses, l_occ=0.85, l_free=0.4, lmin=-2.0, lmax=3.5):
    """qso_logodds (oracle/oracle.c) in float32."""
    v = hits.astype(np.float32) * np.float32(l_occ) - misses.astype(np.float32) * np.float32(l_free)
    return np.clip(v, np.float32(lmin), np.float32(lmax))


def _tri(stamps):
    s = np.asarray(stamps).astype(np.int64)
    return np.where(s == 0, -1, np.where(s & 1, 100, 0)).astype(np.int8)


def _stamps(distmod, m):
    m.sync()
    st, _ = distmod.grid_tensors(m, torch.device("cuda", 0))
    return st.cpu().numpy().astype(np.uint32)


def _check_map(distmod, m, stamps, hits, misses, tag):
    """Every view of the map of one context against the expected stamps and counters."""
    st = _stamps(distmod, m)
    assert (st == stamps).all(), f"{tag}: {int((st != stamps).sum())} stamps differ"
    grid = m.grid_i8()
    tri = _tri(stamps)
    assert (grid == tri).all(), f"{tag}: grid_i8: {int((grid != tri).sum())} cells differ"
    h, mi = m.counts()
    assert (h == hits).all() and (mi == misses).all(), \
        f"{tag}: counts(): {int((h != hits).sum())} hit / {int((mi != misses).sum())} miss counters differ " \
        f"(device sums {int(h.sum())} / {int(mi.sum())}, expected {int(hits.sum())} / {int(misses.sum())})"
    lo = m.logodds()
    want = _logodds(hits, misses)
    assert np.abs(lo - want).max() <= 1e-6, f"{tag}: logodds(): {int((np.abs(lo - want) > 1e-6).sum())} cells differ"


def _rank_streams(replay, world, n, bots=4):
    session, _ = replay.telemetry_csv_to_packets()
    return [replay.multi_bot_stream(session, bots, n, tile0=r * bots, **GEO) for r in range(world)]


class Ranks:
    """W contexts playing W ranks of a per-shard deployment, and the model of what each must show: its own oracle of the
    session, the MAX / SUM over the oracles as they stood at the session's last fuse, and whether dirty tracking is on."""

    def __init__(self, pkg, distmod, world, grid, streams, mode=0, bots=4):
        self.distmod, self.world, self.streams, self.bots = distmod, world, streams, bots
        self.G, self.res, self.half = GRIDS[grid]
        self.dev = torch.device("cuda", 0)
        self.mappers = [pkg.QuasarMapper(self.G, self.res, -self.half, -self.half, max_agent=bots, bots_per_graph=2,
                                         seq_stride=world, raycast_mode=mode) for _ in range(world)]
        for m in self.mappers:
            m.dirty_tracking(True)
        self.tracking = True
        self.src = 0                       # next slice of the streams (runs on over resets: a new session, new data)
        self._new_session()

    def _new_session(self):
        self.oracles = [orc.OracleMapper(self.G, self.res, -self.half, -self.half, 0.0, max_agent=self.bots, bots_per_graph=2)
                        for _ in range(self.world)]
        for r, o in enumerate(self.oracles):
            o.set_sequence(r, self.world)
        self.pos = 0                       # records per rank since the reset
        self.snap = None                   # (stamps MAX, hits SUM, misses SUM) at the session's last fuse

    def close(self):
        for m in self.mappers:
            m.close()

    def ingest(self, n):
        lo, hi = self.src, self.src + n
        assert hi <= len(self.streams[0]), "test streams too short"
        for r, (m, o) in enumerate(zip(self.mappers, self.oracles)):
            m.ingest_array(self.streams[r][lo:hi], seq0=self.pos * self.world + r)
            o.feed_stream(self.streams[r][lo:hi])
        self.src, self.pos = hi, self.pos + n

    def reset(self):
        for m in self.mappers:
            m.reset()
        self._new_session()

    def fuse(self):
        self.distmod.sparse_fuse_local(self.mappers, self.dev)
        self.snap = (np.maximum.reduce([o.stamps for o in self.oracles]),
                     np.sum([o.hits for o in self.oracles], axis=0), np.sum([o.misses for o in self.oracles], axis=0))

    def abandon(self, after_plan):
        """Every rank begins a fuse and the bitmaps are all-gathered (and with after_plan every rank packs its segment);
        then the exchange "fails": no segment travels and no rank applies."""
        W = self.world
        ads = [self.distmod.MapperSparseAdapter(m, self.dev) for m in self.mappers]
        for m in self.mappers:
            m.sync()
        bms = [a.begin(W, r) for r, a in enumerate(ads)]
        for m in self.mappers:
            m.sync()
        for r in range(W):
            for p in range(W):
                if p != r:
                    bms[r][p].copy_(bms[p][p])
        torch.cuda.synchronize()
        if after_plan:
            for a in ads:
                a.plan(W)
            for m in self.mappers:
                m.sync()

    def tracking_off(self):
        for m in self.mappers:
            m.dirty_tracking(False)
        self.tracking = False

    def expected(self, r):
        o = self.oracles[r]
        if self.snap is None:
            return o.stamps.copy(), o.hits.copy(), o.misses.copy()
        stamps = np.maximum(self.snap[0], o.stamps)              # stamps fused at the last fuse, own writes since
        if not self.tracking:
            return stamps, o.hits.copy(), o.misses.copy()        # the views read the own counters again
        return stamps, self.snap[1], self.snap[2]

    def check(self, tag):
        for r, m in enumerate(self.mappers):
            _check_map(self.distmod, m, *self.expected(r), f"{tag}: rank {r}")


# ---- a. the dense path's counts view across a reset --------------------------------------------------------------------
def test_dense_counts_view_across_a_reset(pkg, mods):
    """dist.allreduce_grids turns the fused view on (qs_fused_counts + qs_counts_source(1)); a reset must turn it off, or the
    next session's counts() / logodds() read the zeroed snapshot."""
    distmod, replay = mods
    G, res, half = GRIDS["260"]
    a, b = _rank_streams(replay, 2, 3000)
    oa = orc.OracleMapper(G, res, -half, -half, 0.0, max_agent=4, bots_per_graph=2)
    ob = orc.OracleMapper(G, res, -half, -half, 0.0, max_agent=4, bots_per_graph=2)
    oa.feed_stream(a)
    ob.feed_stream(b)
    with pkg.QuasarMapper(G, res, -half, -half, max_agent=4, bots_per_graph=2) as m:
        m.ingest_array(a)
        m.fused_counts()
        m.counts_source(True)
        _check_map(distmod, m, oa.stamps, oa.hits, oa.misses, "session A, fused view of a one-rank snapshot")
        m.reset()
        m.ingest_array(b)
        _check_map(distmod, m, ob.stamps, ob.hits, ob.misses, "session B after the reset")
        for g in range(2):
            assert (m.closures(g)[0] == ob.closures(g)[0]).all()


# ---- b. the sparse path's counts view across a reset -------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["260", "1024"])
def test_sparse_counts_view_across_a_reset(pkg, mods, grid):
    distmod, replay = mods
    R = Ranks(pkg, distmod, 3, grid, _rank_streams(replay, 3, 9000))
    try:
        for k in range(2):
            R.ingest(3000)
            R.fuse()
            R.check(f"session A, fuse {k}")
        R.reset()
        R.ingest(3000)
        R.check("session B before its first fuse")
        R.fuse()
        R.check("session B after its first fuse")
    finally:
        R.close()


# ---- c. tracking switched off after a sparse fuse ----------------------------------------------------------------------
def test_tracking_off_after_a_sparse_fuse(pkg, mods):
    distmod, replay = mods
    R = Ranks(pkg, distmod, 3, "260", _rank_streams(replay, 3, 9000))
    try:
        R.ingest(3000)
        R.fuse()
        R.check("fused")
        R.tracking_off()
        R.check("tracking off")
        R.ingest(2000)
        R.check("tracking off, more ingest")
        with pytest.raises(pkg.QuasarError):
            R.mappers[0].dirty_tracking(True)              # unfused writes: the sparse fuse could not account for them
        R.reset()
        for m in R.mappers:
            m.dirty_tracking(True)
        R.tracking = True
        R.ingest(3000)
        R.check("tracking on again after the reset")
        R.fuse()
        R.check("first fuse of the new session")
    finally:
        R.close()


# ---- d / e. a fuse abandoned after begin / after plan ------------------------------------------------------------------
@pytest.mark.parametrize("after_plan", [False, True], ids=["after_begin", "after_plan"])
def test_abandoned_sparse_fuse_is_carried_by_the_next(pkg, mods, after_plan):
    """The blocks (and counter deltas) of a fuse that no rank applied travel with the next fuse; a last small batch touches
    few blocks, so the next fuse would not move the abandoned ones on its own account."""
    distmod, replay = mods
    R = Ranks(pkg, distmod, 3, "260", _rank_streams(replay, 3, 9000))
    try:
        R.ingest(3000)
        R.fuse()
        R.ingest(3000)
        R.abandon(after_plan)
        R.ingest(100)
        R.fuse()
        R.check("the fuse after the abandoned one")
        R.ingest(1000)
        R.fuse()
        R.check("one more fuse")
    finally:
        R.close()


# ---- f. a reset context is a fresh context -----------------------------------------------------------------------------
def _views(distmod, m, n_graphs, bots, ekf):
    v = {"grid_i8": m.grid_i8(), "stamps": _stamps(distmod, m), "logodds": m.logodds(), "frontier_cells": m.frontier_cells()}
    v["hits"], v["misses"] = m.counts()
    for g in range(n_graphs):
        v[f"slam_sizes[{g}]"] = np.array(m.slam_sizes(g))
        v[f"closures_idx[{g}]"], v[f"closures_corr[{g}]"] = m.closures(g)
        v[f"landmarks_xy[{g}]"], v[f"landmarks_ti[{g}]"] = m.landmarks(g)
    for b in range(1, bots + 1):
        v[f"drift[{b}]"] = m.drift(b)
        z = m.zone(b)
        v[f"zone[{b}]"] = np.array(z if z is not None else [np.nan] * 4)
        if ekf:
            v[f"ekf_x[{b}]"], v[f"ekf_P[{b}]"] = m.ekf_state(b)
    return v


def _oracle_agrees(v, o, bots, ekf, tag):
    assert (v["grid_i8"] == o.grid).all(), f"{tag}: grid_i8"
    assert (v["stamps"] == o.stamps).all(), f"{tag}: stamps"
    assert (v["hits"] == o.hits).all() and (v["misses"] == o.misses).all(), f"{tag}: counts"
    assert np.abs(v["logodds"] - _logodds(o.hits, o.misses)).max() <= 1e-6, f"{tag}: logodds"
    assert (v["frontier_cells"] == orc.frontier_cells(o.grid)).all(), f"{tag}: frontier_cells"
    for g in range(o.n_graphs):
        oi, oc = o.closures(g)
        oxy, oti = o.landmarks(g)
        assert tuple(v[f"slam_sizes[{g}]"]) == (o.n_nodes(g), len(oti), len(oi)), f"{tag}: slam_sizes({g})"
        assert (v[f"closures_idx[{g}]"] == oi).all() and (len(oi) == 0 or np.abs(v[f"closures_corr[{g}]"] - oc).max() < FLOAT_TOL), \
            f"{tag}: closures({g})"
        assert (v[f"landmarks_ti[{g}]"] == oti).all() and (len(oti) == 0 or np.abs(v[f"landmarks_xy[{g}]"] - oxy).max() < FLOAT_TOL), \
            f"{tag}: landmarks({g})"
    for b in range(1, bots + 1):
        assert np.abs(v[f"drift[{b}]"] - o.drift(b)).max() < FLOAT_TOL, f"{tag}: drift({b})"
        oz = o.zone(b)
        z = v[f"zone[{b}]"]
        assert np.isnan(z).all() == (oz is None) and (oz is None or np.abs(z - oz).max() < FLOAT_TOL), f"{tag}: zone({b})"
        if ekf:
            ox_, oP = o.ekf_state(b)
            assert np.abs(v[f"ekf_x[{b}]"] - ox_).max() <= 1e-9 * max(1.0, np.abs(ox_).max()), f"{tag}: ekf_state({b}) x"
            assert np.abs(v[f"ekf_P[{b}]"] - oP).max() <= 1e-9 * max(1.0, np.abs(oP).max()), f"{tag}: ekf_state({b}) P"


def _reset_equals_fresh(pkg, distmod, cfg, before, stream, times=None, ekf=False, tag=""):
    """`before(m)` drives a context into some state; it is reset, and it and a new context are fed `stream`.  Every view
    of the two is the same, and the oracle's."""
    kw = dict(cfg)
    bots = kw.get("max_agent", 2)
    o = orc.OracleMapper(kw["size"], kw["resolution"], kw["origin_x"], kw["origin_y"], 0.0, max_agent=bots)
    if ekf:
        o.enable_ekf(0.0107)
    o.feed_stream(stream, None, times)
    with pkg.QuasarMapper(enable_ekf=ekf, **kw) as m, pkg.QuasarMapper(enable_ekf=ekf, **kw) as fresh:
        before(m)
        m.reset()
        for c in (m, fresh):
            c.ingest_array(stream, recv_time=times)
        vr = _views(distmod, m, m.n_graphs, bots, ekf)
        vf = _views(distmod, fresh, fresh.n_graphs, bots, ekf)
        for k in vf:
            assert vr[k].shape == vf[k].shape and np.array_equal(vr[k], vf[k], equal_nan=vr[k].dtype.kind == "f"), \
                f"{tag}: reset context != fresh context: {k}"
        _oracle_agrees(vf, o, bots, ekf, tag)
        cr, cf = m.counters(), fresh.counters()
        for k in ("datagrams", "accepted", "rays", "cells", "hits", "closures", "landmarks", "rebases", "edge_rays"):
            assert cr[k] == cf[k], f"{tag}: counter {k}: {cr[k]} after the reset, {cf[k]} fresh"
        return cf


S512 = dict(size=512, resolution=0.05, origin_x=-12.8, origin_y=-12.8)


def _pile_stream(P):
    """test_gpu_parity.py::test_landmark_pile_dense_fallback's stream: a landmark pile that sends the chain to its DENSE variant"""
    L, NQ = 6000, 900
    px, py, qx, qy = 0.05, 0.05, 0.75, 0.35

    def pk(agent, x, y, n, lm=5):
        return P.pack_packets(np.full(n, agent), np.full(n, x), np.full(n, y), np.zeros(n), np.zeros(n, dtype=int),
                              np.zeros(n, dtype=int), np.full((n, 4), 0.3), np.full(n, lm))
    rng = np.random.default_rng(2)
    tail = np.concatenate([pk(1, px, py, 40), pk(2, qx, qy, 40), pk(2, qx + 0.3, qy - 0.2, 60), pk(1, px + 0.2, py + 0.1, 60)])
    rng.shuffle(tail, axis=0)
    return np.concatenate([pk(1, px, py, L), pk(2, qx, qy, NQ), tail])


def test_reset_after_pending_edge_rays(pkg, mods):
    """Exact-trig edge rays are resolved when the map is next observed; a reset straight after the ingest drops them."""
    distmod, _ = mods
    P = pkg.protocol
    rng = np.random.default_rng(99)
    yaws = np.radians(np.arange(24) * 15.0).astype(np.float32)
    lat = np.arange(-6, 7) * 0.05
    xs, ys, yw = np.meshgrid(lat, lat, yaws, indexing="ij")
    n = xs.size
    stream = P.pack_packets(np.ones(n, dtype=int), xs.ravel(), ys.ravel(), yw.ravel(), np.zeros(n, dtype=int),
                            np.zeros(n, dtype=int), rng.integers(3, 125, (n, 4)) * 0.01, np.zeros(n, dtype=int))
    edges = 0
    for ox in (0.0, -0.8, -1.6, -3.2):
        for mode in (1, 2):
            cfg = dict(size=64, resolution=0.05, origin_x=ox, origin_y=ox, raycast_mode=mode)
            c = _reset_equals_fresh(pkg, distmod, cfg, lambda m: m.ingest_array(stream[::-1]), stream, tag=f"origin {ox}, mode {mode}")
            edges += c["edge_rays"]
    assert edges > 0                                         # the stream does put rays on cell boundaries


def test_reset_after_a_stamp_epoch_rebase(pkg, mods):
    distmod, _ = mods
    g = _golden("session_200")
    size, res, ox, oy, _ = g["cfg"]
    pk = g["datagrams"][:, :42]
    cfg = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy)

    def before(m):
        m.ingest_array(pk[:400], seq0=5)
        m.ingest_array(pk[400:], seq0=(1 << 28) + 77)
        assert m.counters()["rebases"] == 1
    _reset_equals_fresh(pkg, distmod, cfg, before, pk, tag="after a rebase")
    with pkg.QuasarMapper(**cfg) as m:                      # and the session after the reset is the golden one
        before(m)
        m.reset()
        m.ingest_array(g["datagrams"], g["lengths"])
        assert hashlib.sha256(m.grid_i8().tobytes()).digest() == g["grid_sha256"].tobytes()


def test_reset_with_the_ekf_on(pkg, mods):
    distmod, _ = mods
    g = _golden("session_512")
    pk, t = g["datagrams"][:, :42], g["recv_time"]
    _reset_equals_fresh(pkg, distmod, S512, lambda m: m.ingest_array(pk, recv_time=t), pk[:500], times=t[:500], ekf=True,
                        tag="EKF on")


def test_reset_after_the_landmark_pile_fallback(pkg, mods):
    distmod, _ = mods
    stream = _pile_stream(pkg.protocol)
    pk = _golden("session_512")["datagrams"][:, :42]

    def before(m):
        for lo, hi in ((0, 2500), (2500, 6000), (6000, 6300), (6300, len(stream))):
            m.ingest_array(stream[lo:hi])
        assert m.counters()["slam_misc_iters"] > 0            # the DENSE variant ran
    _reset_equals_fresh(pkg, distmod, S512, before, pk, tag="after the pile")


def test_reset_after_capacity_growth(pkg, mods):
    distmod, _ = mods
    pk = _golden("session_512")["datagrams"][:, :42]
    laps = np.tile(pk, (30, 1))

    def before(m):
        pos, k, sizes = 0, 0, [5, 700, 1500, 64, 3000, 1, 9000, 20000]
        while pos < len(laps):
            m.ingest_array(laps[pos:pos + sizes[k % len(sizes)]])
            pos += sizes[k % len(sizes)]
            k += 1
    _reset_equals_fresh(pkg, distmod, S512, before, pk[:600], tag="after growth")


def test_reset_after_a_sparse_fuse(pkg, mods):
    """Tracking on, a (one-rank) sparse fuse, more unfused writes, then the reset: the views read the local counters again."""
    distmod, _ = mods
    pk = _golden("session_512")["datagrams"][:, :42]

    def before(m):
        m.dirty_tracking(True)
        m.ingest_array(pk[:300])
        distmod.sparse_fuse_local([m], torch.device("cuda", 0))
        m.ingest_array(pk[300:])
    _reset_equals_fresh(pkg, distmod, S512, before, pk[::-1].copy(), tag="after a sparse fuse")


# ---- g. seeded state-machine walk --------------------------------------------------------------------------------------
def walk(pkg, distmod, replay, world, seed, steps=30, log=None):
    """A seeded walk over ingest / sparse fuse / fuse abandoned after begin or plan / reset / read, checked after every step
    against the model in Ranks.  Raises AssertionError naming the seed and the step."""
    rng = np.random.default_rng(seed)
    streams = _rank_streams(replay, world, steps * 1500 + 1500)
    R = Ranks(pkg, distmod, world, "260", streams, mode=int(rng.integers(0, 3)))
    history = []
    try:
        for step in range(steps):
            op = str(rng.choice(["ingest", "ingest", "fuse", "abandon_begin", "abandon_plan", "reset", "read"],
                                p=[0.3, 0.1, 0.2, 0.1, 0.1, 0.1, 0.1]))
            if op == "ingest":
                n = int(rng.integers(100, 1500))
                R.ingest(n)
                op = f"ingest {n}"
            elif op == "fuse":
                R.fuse()
            elif op.startswith("abandon"):
                R.abandon(op == "abandon_plan")
            elif op == "reset":
                R.reset()
            history.append(op)
            try:
                R.check(f"seed {seed}, world {world}, step {step} ({op})")
            except AssertionError as e:
                raise AssertionError(f"{e}\n  steps so far: {history}") from None
        if log is not None:
            log.append(history)
    finally:
        R.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_state_machine_walk(pkg, mods, world, seed):
    distmod, replay = mods
    walk(pkg, distmod, replay, world, 1000 * world + seed)
