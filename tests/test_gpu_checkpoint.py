"""qs_checkpoint / qs_restore: a session that is checkpointed, destroyed and restored into a fresh context must answer every
later call bit for bit as the uninterrupted session does.

Run A ingests a stream in two parts.  Run B ingests the first part, checkpoints, is destroyed; a new context restores the
checkpoint and ingests the rest.  Every view of A and B is compared exactly (raw stamps, counters, grid, log-odds, closures,
closure agents, landmarks, sizes, drift, ZONE packets, EKF state, session counters, frontier clusters and targets), and the
views the oracle has against the oracle fed the whole stream.  The split is chosen so that a closure after it matches a
landmark logged before it: the rebuilt bucket index has to answer that query."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import GOLDEN, load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SESSION_COUNTERS = ("datagrams", "accepted", "rays", "cells", "hits", "closures", "landmarks", "rebases", "edge_rays")
W4096 = dict(size=4096, resolution=0.05, origin_x=-102.4, origin_y=-102.4)
QS_E_INVAL, QS_E_RANGE, QS_E_STATE = -1, -4, -6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def mods(pkg):
    return importlib.import_module(pkg.__name__ + ".dist"), importlib.import_module(pkg.__name__ + ".replay")


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)


def _scenario(name, replay):
    """(mapper kwargs, oracle args, datagrams [n, stride], lengths or None, recv_time or None)"""
    if name in ("session_4096", "adversarial_dense_200"):
        g = _golden(name)
        size, res, ox, oy, sep = g["cfg"]
        kw = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy, separation=sep, max_agent=2)
        orc_kw = dict(args=(int(size), res, ox, oy, sep), max_agent=2, bots_per_graph=0)
        return kw, orc_kw, g["datagrams"], g["lengths"], (g["recv_time"] if "recv_time" in g.files else None)
    stream = replay.multi_bot_stream(None, 64, 22_000)
    bpg = 2 if name == "multibot_32_graphs" else 0
    kw = dict(W4096, max_agent=64, bots_per_graph=bpg)
    orc_kw = dict(args=(4096, 0.05, -102.4, -102.4, 0.0), max_agent=64, bots_per_graph=bpg)
    return kw, orc_kw, stream, None, None


def _ingest(m, data, lens, times, lo, hi):
    m.ingest_array(data[lo:hi], None if lens is None else lens[lo:hi], None if times is None else times[lo:hi])


def _graph_of(data, lens, acc, bpg, max_agent):
    agent = data[:, 4].astype(np.int64)
    g = (agent - 1) // (bpg if bpg > 0 else max_agent)
    return np.where(acc.astype(bool), g, -1)


def _pick_split(pkg, kw, data, lens, times):
    """A packet index k such that graph 0 has a closure at a node after k whose landmark node lies before k."""
    with pkg.QuasarMapper(**kw) as p:
        _ingest(p, data, lens, times, 0, len(data))
        acc, _ = p.last_batch()
        cl, _ = p.closures(0)
    assert len(cl), "the stream has no closure in graph 0"
    graph = _graph_of(data, lens, acc, kw.get("bots_per_graph", 0), kw["max_agent"])
    nodes0 = np.cumsum(graph == 0)                          # graph-0 nodes among packets [0..i]
    best = None
    for lm, node in cl.tolist():
        if node - lm >= 4 and (best is None or abs((lm + node) / 2 - nodes0[-1] / 2) < abs(sum(best) / 2 - nodes0[-1] / 2)):
            best = (lm, node)
    lm, node = best
    mid = (lm + node + 1) // 2
    k = int(np.searchsorted(nodes0, mid))                   # packets [0, k) hold mid graph-0 nodes at most
    return k


def _bots_xy(kw):
    rng = np.random.default_rng(7)
    half = kw["size"] * kw["resolution"] / 2
    return np.column_stack([rng.uniform(kw["origin_x"], kw["origin_x"] + 2 * half, 8),
                            rng.uniform(kw["origin_y"], kw["origin_y"] + 2 * half, 8)])


def _views(distmod, m, kw):
    """Every view the contract covers, as plain arrays."""
    m.sync()
    st, _ = distmod.grid_tensors(m, DEV)
    v = {"stamps": st.cpu().numpy().copy(), "grid": m.grid_i8()}
    h, mi = m.counts()
    v.update(hits=h, misses=mi, logodds=m.logodds())
    for g in range(m.n_graphs):
        v[f"sizes{g}"] = np.array(m.slam_sizes(g))
        idx, corr = m.closures(g)
        xy, ti = m.landmarks(g)
        v.update({f"cl{g}": idx, f"corr{g}": corr, f"clag{g}": m.closure_agents(g), f"lmxy{g}": xy, f"lmti{g}": ti})
    for b in range(1, m.max_agent + 1):
        v[f"drift{b}"] = m.drift(b)
        v[f"zone{b}"] = np.frombuffer(m.zone_packet(b), dtype=np.uint8).copy()
        if m.cfg.enable_ekf:
            x, P = m.ekf_state(b)
            v[f"ekfx{b}"], v[f"ekfP{b}"] = x, P
    c = m.counters()
    v["counters"] = np.array([c[k] for k in SESSION_COUNTERS], dtype=np.uint64)
    v["clusters"] = m.frontier_clusters(3)
    idx, xy = m.frontier_targets(_bots_xy(kw))[:2]
    v["targets"], v["targets_xy"] = idx, xy
    return v


def _assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, f"{tag}: {k}: shapes {x.shape} / {y.shape}"
        assert x.dtype == y.dtype, f"{tag}: {k}"
        same = (x.view(np.uint8) == y.view(np.uint8)).all() if x.size else True     # bit for bit (NaN included)
        assert same, f"{tag}: {k} differs ({int((x != y).sum())} elements)"


def _assert_oracle(m, orc_kw, data, lens, tag):
    o = orc.OracleMapper(*orc_kw["args"], max_agent=orc_kw["max_agent"], bots_per_graph=orc_kw["bots_per_graph"])
    o.feed_stream(data, lens)
    grid = m.grid_i8()
    assert (grid == o.grid).all(), f"{tag}: {int((grid != o.grid).sum())} cells differ from the oracle"
    for g in range(m.n_graphs):
        idx, corr = m.closures(g)
        oi, oc = o.closures(g)
        assert idx.shape == oi.shape and (idx == oi).all(), f"{tag}: graph {g} closures differ from the oracle"
        if len(corr):
            assert np.abs(corr - oc).max() < 1e-5
    for b in range(1, m.max_agent + 1):
        assert np.abs(m.drift(b) - o.drift(b)).max() < 1e-5, f"{tag}: drift of bot {b}"
        assert m.zone_packet(b) == o.zone_packet(b), f"{tag}: ZONE of bot {b}"


def _run_a(pkg, kw, data, lens, times, k):
    m = pkg.QuasarMapper(**kw)
    _ingest(m, data, lens, times, 0, k)
    _ingest(m, data, lens, times, k, len(data))
    return m


def _run_b(pkg, kw, data, lens, times, k, form=None, restore_kw=None):
    with pkg.QuasarMapper(**kw) as first:
        _ingest(first, data, lens, times, 0, k)
        split_nodes = [first.slam_sizes(g)[0] for g in range(first.n_graphs)]
        ck = first.checkpoint()
    m = pkg.QuasarMapper(**dict(kw, **(restore_kw or {})))
    m.restore(ck)
    if form is not None:
        m.set_chain_form(form)
    _ingest(m, data, lens, times, k, len(data))
    return m, split_nodes


SCENARIOS = ["session_4096", "multibot_32_graphs", "multibot_one_graph", "adversarial_dense_200"]


@pytest.mark.parametrize("name", SCENARIOS)
def test_resume_equals_uninterrupted_run(pkg, mods, name):
    distmod, replay = mods
    kw, orc_kw, data, lens, times = _scenario(name, replay)
    kw = dict(kw, enable_ekf=True)
    k = _pick_split(pkg, kw, data, lens, times)
    with _run_a(pkg, kw, data, lens, times, k) as a:
        va = _views(distmod, a, kw)
    b, split_nodes = _run_b(pkg, kw, data, lens, times, k)
    with b:
        vb = _views(distmod, b, kw)
        _assert_oracle(b, orc_kw, data, lens, name)
        # the rebuilt index was used: a closure after the split matched a landmark logged before it
        used = False
        for g in range(b.n_graphs):
            cl, _ = b.closures(g)
            if len(cl):
                used |= bool(((cl[:, 1] >= split_nodes[g]) & (cl[:, 0] < split_nodes[g])).any())
        assert used, f"{name}: no closure after the split reaches back before it"
    _assert_same(va, vb, name)


@pytest.mark.parametrize("form", ["free", "free_posting", "window"])
@pytest.mark.parametrize("name", ["multibot_32_graphs", "adversarial_dense_200"])
def test_every_chain_form_after_restore(pkg, mods, name, form):
    distmod, replay = mods
    kw, _, data, lens, times = _scenario(name, replay)
    k = _pick_split(pkg, kw, data, lens, times)
    with _run_a(pkg, kw, data, lens, times, k) as a:
        va = _views(distmod, a, kw)
    b, _ = _run_b(pkg, kw, data, lens, times, k, form=form)
    with b:
        vb = _views(distmod, b, kw)
    _assert_same(va, vb, f"{name}/{form}")


def test_epoch_boundary(pkg, mods):
    distmod, _ = mods
    g = _golden("session_512")
    size, res, ox, oy, sep = g["cfg"]
    kw = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy, separation=sep)
    data, lens = g["datagrams"], g["lengths"]
    k = len(data) // 2
    seq0 = (1 << 28) - 2 - k - 50                          # the first part fits the epoch, the second crosses it

    def first_part(m):
        m.ingest_array(data[:k], lens[:k], seq0=seq0)
        assert m.counters()["rebases"] == 0
    a = pkg.QuasarMapper(**kw)
    first_part(a)
    a.ingest_array(data[k:], lens[k:])
    with pkg.QuasarMapper(**kw) as first:
        first_part(first)
        ck = first.checkpoint()
    b = pkg.QuasarMapper(**kw)
    b.restore(ck)
    b.ingest_array(data[k:], lens[k:])
    with a, b:
        assert a.counters()["rebases"] == 1 and b.counters()["rebases"] == 1
        _assert_same(_views(distmod, a, kw), _views(distmod, b, kw), "epoch")


def test_sweeps_and_offsets(pkg, mods):
    distmod, _ = mods
    g, s = _golden("session_512"), _golden("sweeps_512")
    size, res, ox, oy, sep = g["cfg"]
    kw = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy, separation=sep)
    data, lens, sw = g["datagrams"], g["lengths"], s["sweeps_odo"]
    kp, ks = len(data) // 2, len(sw) // 2

    def setup(m):
        m.set_bot_offset(1, -0.35)
        m.set_bot_offset(2, 0.8)
        m.set_sweep_filter(0.15, 1.0)

    def part1(m):
        m.ingest_array(data[:kp // 2], lens[:kp // 2])
        m.ingest_sweeps(sw[:ks])
        m.ingest_array(data[kp // 2:kp], lens[kp // 2:kp])

    def part2(m):
        m.ingest_sweeps(sw[ks:])
        m.ingest_array(data[kp:], lens[kp:])
        return m.last_batch()[1]

    a = pkg.QuasarMapper(**kw)
    setup(a)
    part1(a)
    pose_a = part2(a)
    with pkg.QuasarMapper(**kw) as first:
        setup(first)
        part1(first)
        ck = first.checkpoint()
    b = pkg.QuasarMapper(**kw)                                # default offsets and filter: the checkpoint brings them
    b.restore(ck)
    with pytest.raises(pkg.QuasarError):
        b.last_batch()                                       # the resident batch is not part of a session
    pose_b = part2(b)
    with a, b:
        assert (pose_a.view(np.uint8) == pose_b.view(np.uint8)).all()
        _assert_same(_views(distmod, a, kw), _views(distmod, b, kw), "sweeps")


def test_sparse_fuse_rank_restored(pkg, mods):
    """Two contexts as ranks with tracking on; rank 1 is checkpointed with unfused writes after an earlier fuse, restored into
    a new context, and the fusing goes on: both ranks equal the run without a restore."""
    distmod, replay = mods
    session, _ = replay.telemetry_csv_to_packets()
    streams = [replay.multi_bot_stream(session, 4, 2400, pitch=5.0, tiles_per_row=8, origin=(-22.0, -20.0), tile0=4 * r)
               for r in range(2)]
    kw = dict(size=1024, resolution=0.05, origin_x=-25.6, origin_y=-25.6, max_agent=4, bots_per_graph=2, seq_stride=2)

    def ranks():
        ms = [pkg.QuasarMapper(**kw) for _ in range(2)]
        for m in ms:
            m.dirty_tracking(True)
        return ms

    def ingest(ms, lo, hi):
        for r, m in enumerate(ms):
            m.ingest_array(streams[r][lo:hi], seq0=lo * 2 + r)

    def state(ms):
        out = []
        for m in ms:
            m.sync()
            st, _ = distmod.grid_tensors(m, DEV)
            fc = distmod.fused_counts_view(m, DEV)
            h, mi = m.counts()
            out.append((st.cpu().numpy().copy(), fc.cpu().numpy().copy(), h, mi))
        return out

    def run(restore):
        ms = ranks()
        ingest(ms, 0, 800)
        distmod.sparse_fuse_local(ms, DEV)
        ingest(ms, 800, 1600)                                # unfused writes on both ranks
        if restore:
            ck = ms[1].checkpoint()
            ms[1].close()
            ms[1] = pkg.QuasarMapper(**kw)                   # tracking off: the restore switches it on
            ms[1].restore(ck)
        distmod.sparse_fuse_local(ms, DEV)
        ingest(ms, 1600, 2400)
        distmod.sparse_fuse_local(ms, DEV)
        s = state(ms)
        for m in ms:
            m.close()
        return s

    ref, got = run(False), run(True)
    for r in range(2):
        for what, x, y in zip(("stamps", "fused counts", "hits", "misses"), ref[r], got[r]):
            assert (x == y).all(), f"rank {r}: {what}: {int((x != y).sum())} cells differ"


def _rc_restore(m, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    rc = m._L.qs_restore(m._h, a.ctypes.data_as(C.c_void_p), len(a))
    return rc, m._L.qs_last_error(m._h).decode()


def _fingerprint(distmod, m):
    m.sync()
    st, _ = distmod.grid_tensors(m, DEV)
    return st.cpu().numpy().copy(), m.closures(0)[0], m.slam_sizes(0)


def test_refusals_leave_the_context_unchanged(pkg, mods):
    distmod, _ = mods
    g = _golden("session_512")
    size, res, ox, oy, sep = g["cfg"]
    kw = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy, separation=sep)
    data, lens = g["datagrams"], g["lengths"]
    with pkg.QuasarMapper(**kw) as src:
        src.ingest_array(data, lens)
        ck = bytearray(src.checkpoint())
        # cap below the size
        n = C.c_size_t()
        buf = np.zeros(len(ck), dtype=np.uint8)
        assert src._L.qs_checkpoint(src._h, buf.ctypes.data_as(C.c_void_p), len(ck) - 1, C.byref(n)) == QS_E_RANGE
        assert n.value == len(ck)
    h = len(ck) // 2
    cases = {"size": (dict(kw, size=int(size) + 64), ck, "size"),
             "closure_radius": (dict(kw, closure_radius=0.61), ck, "closure_radius"),
             "flipped": (kw, ck[:h] + bytes([ck[h] ^ 0x10]) + ck[h + 1:], "CRC"),
             "truncated": (kw, ck[:-9], "")}
    for tag, (tkw, blob, field) in cases.items():
        with pkg.QuasarMapper(**tkw) as t:
            t.ingest_array(data[:300], lens[:300])
            before = _fingerprint(distmod, t)
            rc, err = _rc_restore(t, blob)
            assert rc == QS_E_INVAL, f"{tag}: rc {rc} ({err})"
            assert field in err, f"{tag}: '{field}' not named in '{err}'"
            after = _fingerprint(distmod, t)
            assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and before[2] == after[2], tag
    # a sparse fuse in flight: both calls refuse
    with pkg.QuasarMapper(**kw) as t:
        t.dirty_tracking(True)
        t.ingest_array(data[:300], lens[:300])
        before = _fingerprint(distmod, t)
        t.sparse_fuse_begin(1, 0)
        rc, err = _rc_restore(t, ck)
        assert rc == QS_E_STATE, err
        assert t._L.qs_checkpoint(t._h, None, 0, C.byref(n)) == QS_E_STATE
        t.sparse_fuse_plan(1)
        t.sparse_fuse_apply()
        after = _fingerprint(distmod, t)
        assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and before[2] == after[2]


def test_size_and_idempotence(pkg, mods):
    distmod, _ = mods
    g = _golden("session_4096")
    size, res, ox, oy, sep = g["cfg"]
    kw = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy, separation=sep)
    data, lens = g["datagrams"], g["lengths"]
    with pkg.QuasarMapper(**kw) as empty:
        k0 = pkg.checkpoint_config(empty.checkpoint())
        assert k0["n_blocks"] == 0
    with pkg.QuasarMapper(**kw) as m:
        m.ingest_array(data[:400], lens[:400])
        ck = m.checkpoint()
        dense = int(size) * int(size) * (4 + 8)
        assert len(ck) < 0.01 * dense, f"{len(ck)} bytes against {dense} of dense planes"
        assert pkg.checkpoint_config(ck)["n_blocks"] > 0
        m.restore(ck)
        assert m.checkpoint() == ck                          # restore into the same context, checkpoint again: same bytes
        m.ingest_array(data[400:], lens[400:])
        va = _views(distmod, m, kw)
    with pkg.QuasarMapper(**dict(kw, raycast_mode=2)) as t:  # another raycast mode: accepted, same results
        t.restore(ck)
        t.ingest_array(data[400:], lens[400:])
        _assert_same(va, _views(distmod, t, kw), "raycast_mode")


def test_save_and_load(pkg, mods, tmp_path):
    distmod, replay = mods
    kw, _, data, lens, times = _scenario("multibot_32_graphs", replay)
    kw = dict(kw, enable_ekf=True, closure_radius=0.55, min_poses_between=25)
    path = tmp_path / "session.qsck"
    with pkg.QuasarMapper(**kw) as m:
        m.ingest_array(data[:12_000])
        n = m.save(path)
        assert os.path.getsize(path) == n and not [p for p in os.listdir(tmp_path) if ".tmp-" in p]
        va = _views(distmod, m, kw)
        cfg = {f: getattr(m.cfg, f) for f, _ in m.cfg._fields_ if f not in ("reserved", "device", "separation")}
    with pkg.QuasarMapper.load(path) as t:
        assert {f: getattr(t.cfg, f) for f in cfg} == cfg
        _assert_same(va, _views(distmod, t, kw), "load")
