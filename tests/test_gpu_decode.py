"""K0, the packet decoder (csrc/decode.hip), at every stride, alignment and tile edge -- both kernels (LDS-staged for strides
<= 64, per-lane for wider ones), the host entry (qs_ingest) and the device entry (qs_ingest_device, qs_ingest_sweeps_device).

The yardsticks: tests/decode_rules.py, a byte-level restatement pinned to the reference's fixtures and the oracle by
tests/test_decode_rules_cpu.py (accept, agent, landmark type, pose, distances, encoder: exact), and the CPU oracle fed the same
records as datagrams (map, hit points, pose graphs, zones, EKF).  Decode is exact, so the pose of a batch is compared bit
for bit; the stages behind it keep the bars the project already holds them to (1e-9 absolute for hit points, landmark
positions, closure corrections, drift and zones; 1e-9 relative for the EKF).

Every buffer carries random NON-ZERO padding after its records, every pool is 15-40 % rejected records (bad magic, agents 0 /
max_agent + 1 / 255, odd lengths, non-finite poses) and its kept records carry v1 truncation, specials in every float, encoder
extremes and the landmark bytes 0..5, 7, 255.

What the cases reach (test_device_alignment_reaches_every_shift asserts it from the kernel's own arithmetic): the record shift
sh in {0, 1, 2, 3} (odd strides, host path already), the range misalignment mis in {1, 2, 3} (device path at byte offsets 1, 2,
3, 5 only: the host path stages into an aligned buffer and a tile is a multiple of 4 bytes), all 16 (mis, sh) pairs, the bytewise
staging branch at the start (offset buffers) and at the end (n * stride not a multiple of 4) of a buffer, and the wide kernel
(strides 65, 72, 100, 255).

Mutants of decode.hip these tests were run against, one at a time (tests of this file that fail / of 82; the parity,
life-cycle and checkpoint tests stayed green on all but the last):
  sh forced to sh & 2                                    38: every odd stride, host and device
  mis dropped from the record offset                     11: the device-offset cases
  landmark byte read whatever the length (LDS kernel)    59
  the same in the wide kernel                            19: strides 65, 72, 100, 255
  the wide kernel's d3 read at byte 36                    9: the oracle comparisons at strides 65, 72, 255 (hit points, map)
  (size_t)len <= stride dropped                           2: test_length_above_the_stride_is_refused
  s_acc flushed inside the tile loop                     58 (test_session_exact_float_agreement_with_oracle sees it too)
The whole file takes about 9 s on an MI355X."""
import importlib
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import decode_rules as dr
from conftest import GOLDEN, load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SIZE, RES, OX, OY, SEP = 1024, 0.05, -25.6, -25.6, 1.25      # +-25.6 m: the pools' poses stay within +-20 m
NO_CLOSURES = 1 << 30          # min_poses_between no stream reaches: every drift stays 0.0 and the reported pose is the decoded one
MPT = 0.0107
SLACK = 64                     # bytes of the tensor before and after every range handed to a device entry point
NS = (1, 255, 256, 257, 2047, 2048, 2049, 4097, 5003)
HOST_CASES = [(41, False), (42, False)] + [(s, True) for s in range(42, 65)] + [(s, True) for s in (65, 72, 100, 255)]
FULL_CASES = [(41, False), (42, False), (42, True), (43, True), (48, True), (63, True), (64, True), (65, True), (255, True)]
DEVICE_CASES = [(41, False), (42, False), (43, True), (48, True), (64, True), (65, True)]
DEVICE_OFFSETS = (0, 1, 2, 3, 5)
SLACK_RECORD = dr.struct.pack(dr.FMT_V2, b"QSRL", 1, 3.0, -4.0, 0.25, 11, 0, 0.5, 0.6, 0.7, 0.8, 5)
MAP_COUNTERS = ("datagrams", "accepted", "rays", "cells", "hits", "closures", "landmarks")


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _base(pkg, max_agent, seed):
    """42-byte records to mutate: the recorded session (two bots, a few metres) and an adversarial stream over +-20 m."""
    replay = importlib.import_module(pkg.__name__ + ".replay")
    g = np.load(os.path.join(GOLDEN, "session_512.npz"), allow_pickle=False)
    return np.concatenate([g["datagrams"][:, :42], replay.adversarial_stream(6000, seed=seed, lo=-20.0, hi=20.0, max_agent=max_agent)])


def _offsets(max_agent):
    off = np.zeros(max_agent + 1)
    if max_agent >= 2:
        off[2] = SEP
    return off


def _times(n, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.choice([0.05, 0.02, 0.0, -0.01, 0.3], size=n, p=[.7, .1, .08, .04, .08])) + 100.0


def _mapper(pkg, **kw):
    cfg = dict(size=SIZE, resolution=RES, origin_x=OX, origin_y=OY, separation=SEP, max_agent=7, bots_per_graph=2)
    cfg.update(kw)
    return pkg.QuasarMapper(**cfg)


def _bpg(max_agent, bots_per_graph):
    return bots_per_graph if bots_per_graph > 0 else max_agent


def _share(ref, tag):
    share = 1.0 - float(ref["accept"].mean())
    assert 0.15 <= share <= 0.40, f"{tag}: {share:.3f} of the records rejected -- the pool must stay between 15 % and 40 %"


class _Walk:
    """The oracle fed the datagrams one at a time: per record the accepted flag and its valid hit points."""

    def __init__(self, P, grams, max_agent=7, bots_per_graph=2, times=None, ekf=False, owned=None, per_record=True):
        o = orc.OracleMapper(SIZE, RES, OX, OY, SEP, max_agent=max_agent, bots_per_graph=bots_per_graph)
        if owned:
            o.set_owned(*owned)
        if ekf:
            o.enable_ekf(MPT)
        self.o, n = o, len(grams)
        assert max(len(d) for d in grams) <= 48
        buf, lens = P.pack_datagrams(grams)
        if not per_record:
            self.n_acc = o.feed_stream(buf, lens, times)
            return
        L = orc.lib()
        self.acc = np.zeros(n, dtype=np.uint8)
        h0 = np.zeros(n + 1, dtype=np.int64)
        for k in range(n):
            self.acc[k] = o.feed_stream(buf[k:k + 1], lens[k:k + 1], None if times is None else times[k:k + 1])
            h0[k + 1] = L.qso_n_hits(o._h)
        self.n_acc = int(self.acc.sum())
        pts, code = o.hit_points, o.hit_agent_sensor
        rec = np.repeat(np.arange(n), np.diff(h0))
        self.valid = np.zeros((n, 4), dtype=np.uint8)
        self.hits = np.zeros((n, 4, 2), dtype=np.float64)
        self.valid[rec, code % 4] = 1
        self.hits[rec, code % 4] = pts


def _graph_counts(ref, max_agent, bots_per_graph):
    """Per graph, from the byte-level reference alone: accepted records, landmark events, and the (type, node index) list."""
    bpg = _bpg(max_agent, bots_per_graph)
    n_graphs = (max_agent + bpg - 1) // bpg
    ok = ref["accept"] == 1
    g_of = (ref["agent"][ok].astype(np.int64) - 1) // bpg
    lm = ref["lm"][ok]
    nodes = np.bincount(g_of, minlength=n_graphs)
    lms = np.bincount(g_of[lm != 0], minlength=n_graphs)
    idx_in_graph = np.zeros(len(g_of), dtype=np.int64)
    for g in range(n_graphs):
        sel = g_of == g
        idx_in_graph[sel] = np.arange(int(sel.sum()))
    return n_graphs, g_of, nodes, lms, lm, idx_in_graph, ref["agent"][ok]


def _check_decode(m, ref, max_agent, bots_per_graph, tag, pose_exact=True):
    """The observables that come from the reference alone (cheap: no map read): accept, the pose bit for bit (contexts that
    close no loop), the two decode counters, per-graph node and landmark counts, landmark types and order, and the per-bot
    landmark-event counts they imply."""
    n = len(ref["accept"])
    acc, pose = m.last_batch()
    assert (acc == ref["accept"]).all(), f"{tag}: accept differs at records {np.nonzero(acc != ref['accept'])[0][:8].tolist()}"
    ok = acc == 1
    if pose_exact:
        want = dr.pose_as_reported(ref)
        same = (pose[ok].view(np.uint64) == want[ok].view(np.uint64)).all(axis=1)
        assert same.all(), f"{tag}: pose differs at accepted records {np.nonzero(ok)[0][~same][:8].tolist()}"
    assert np.isnan(pose[~ok]).all(), tag
    c = m.counters()
    assert c["datagrams"] == n and c["accepted"] == int(ref["accept"].sum()), (tag, c["datagrams"], c["accepted"])
    n_graphs, g_of, nodes, lms, lm, idx_in_graph, agents = _graph_counts(ref, max_agent, bots_per_graph)
    events_per_bot = np.zeros(max_agent + 1, dtype=np.int64)
    for g in range(n_graphs):
        sizes = m.slam_sizes(g)
        assert sizes[:2] == (int(nodes[g]), int(lms[g])), f"{tag}: graph {g} holds {sizes[:2]}, the reference {(nodes[g], lms[g])}"
        ti = m.landmarks(g)[1]
        sel = (g_of == g) & (lm != 0)
        assert (ti[:, 0] == lm[sel]).all() and (ti[:, 1] == idx_in_graph[sel]).all(), f"{tag}: graph {g}: landmark types / order"
        of_graph = agents[g_of == g]
        events_per_bot += np.bincount(of_graph[ti[:, 1]], minlength=max_agent + 1)
    assert (events_per_bot == np.bincount(agents[lm != 0], minlength=max_agent + 1)).all(), tag
    assert c["landmarks"] == int((lm != 0).sum()), tag


def _ekf_close(m, o, bots, rtol=1e-9):
    """The bar of tests/test_gpu_parity.py::_ekf_close."""
    for b in bots:
        x, P = m.ekf_state(b)
        xo, Po = o.ekf_state(b)
        assert np.abs(x - xo).max() <= rtol * max(1.0, np.abs(xo).max()), (b, x, xo)
        assert np.abs(P - Po).max() <= rtol * max(1.0, np.abs(Po).max()), b


def _check_oracle(m, ref, w, max_agent, bots_per_graph, tag, ekf=False, owned=None):
    """Everything behind the decoder against the oracle fed the same records as datagrams (one ingest on a fresh context)."""
    o = w.o
    acc, pose = m.last_batch()
    assert (acc == w.acc).all() and (acc == ref["accept"]).all(), tag
    assert np.abs(pose[acc == 1] - o.poses).max() <= 1e-9, tag
    mine = np.ones(len(acc), dtype=bool) if owned is None else (ref["agent"] >= owned[0]) & (ref["agent"] <= owned[1])
    xy, valid = m.last_hits()
    assert (valid[mine] == w.valid[mine]).all(), f"{tag}: hit validity differs at {np.nonzero((valid != w.valid).any(axis=1) & mine)[0][:8].tolist()}"
    sel = (w.valid == 1) & mine[:, None]
    assert sel.sum() > 0 and np.abs(xy[sel] - w.hits[sel]).max() <= 1e-9, f"{tag}: hit points {np.abs(xy[sel] - w.hits[sel]).max()}"
    grid = m.grid_i8()
    assert (grid == o.grid).all(), f"{tag}: {(grid != o.grid).sum()} cells differ from the oracle"
    h, mi = m.counts()
    assert (h == o.hits).all() and (mi == o.misses).all(), f"{tag}: hit / miss counters"
    bpg = _bpg(max_agent, bots_per_graph)
    n_graphs = (max_agent + bpg - 1) // bpg
    n_cls = n_lms = 0
    for g in range(n_graphs):
        assert m.slam_sizes(g)[0] == o.n_nodes(g), f"{tag}: graph {g} nodes"
        lxy, ti = m.landmarks(g)
        oxy, oti = o.landmarks(g)
        assert ti.shape == oti.shape and (ti == oti).all(), f"{tag}: graph {g} landmark types / order"
        assert len(oti) == 0 or np.abs(lxy - oxy).max() <= 1e-9, f"{tag}: graph {g} landmark positions"
        idx, corr = m.closures(g)
        oi, oc = o.closures(g)
        assert idx.shape == oi.shape and (idx == oi).all(), f"{tag}: graph {g} closures"
        assert len(oi) == 0 or np.abs(corr - oc).max() <= 1e-9, f"{tag}: graph {g} closure corrections"
        n_cls += len(oi)
        n_lms += len(oti)
    for b in range(1, max_agent + 1):
        assert np.abs(m.drift(b) - o.drift(b)).max() <= 1e-9, f"{tag}: drift of bot {b}"
        z, zo = m.zone(b), o.zone(b)
        assert (z is None) == (zo is None), f"{tag}: zone of bot {b}"
        assert z is None or np.abs(np.array(z) - zo).max() <= 1e-9, f"{tag}: zone of bot {b}"
    if ekf:
        _ekf_close(m, o, range(1, max_agent + 1) if owned is None else range(owned[0], owned[1] + 1))
    c = m.counters()
    want = dict(datagrams=len(acc), accepted=w.n_acc, rays=o.n_rays, cells=o.n_cells_written, hits=len(o.hit_points),
                closures=n_cls, landmarks=n_lms)
    assert {k: c[k] for k in MAP_COUNTERS} == want, tag
    return n_cls


def _observe(m, max_agent, bots_per_graph, ekf):
    """Everything a caller can read, for comparing two contexts exactly."""
    bpg = _bpg(max_agent, bots_per_graph)
    out = dict(grid=m.grid_i8())
    out["hits"], out["misses"] = m.counts()
    for g in range((max_agent + bpg - 1) // bpg):
        out[f"sizes{g}"] = np.array(m.slam_sizes(g))
        out[f"lm_xy{g}"], out[f"lm_ti{g}"] = m.landmarks(g)
        out[f"cl_idx{g}"], out[f"cl_corr{g}"] = m.closures(g)
    for b in range(1, max_agent + 1):
        out[f"drift{b}"] = m.drift(b)
        z = m.zone(b)
        out[f"zone{b}"] = np.full(4, np.nan) if z is None else np.array(z)
        if ekf:
            out[f"ekf_x{b}"], out[f"ekf_P{b}"] = m.ekf_state(b)
    return out


def _observe_batch(m):
    out = {}
    out["acc"], out["pose"] = m.last_batch()
    out["hit_xy"], out["hit_valid"] = m.last_hits()
    c = m.counters()
    out["counters"] = np.array([c[k] for k in MAP_COUNTERS], dtype=np.uint64)
    return out


def _same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, k)
        assert x.tobytes() == y.tobytes(), f"{tag}: {k} differs"


class _OnDevice:
    """A buffer of dr.build (head and tail slack of at least SLACK bytes, holding well-formed records on the stride lattice)
    in one torch uint8 tensor; .ptr is the address of record 0, `off` bytes past a 4-byte boundary.  The library is only ever
    given the n * stride bytes in the middle: the range never touches either end of the allocation."""

    def __init__(self, records, stride, rng, off, lens=True, times=None, body=None):
        n = len(records)
        head, tail = SLACK + off, SLACK + (-(SLACK + off + n * stride)) % 8
        self.host, lens_np = dr.build(records, stride, rng, head=head, tail=tail, slack_record=SLACK_RECORD)
        if body is not None:                       # the very bytes of another buffer of these records, padding included
            self.host[head:head + n * stride] = body
        self.t = torch.from_numpy(self.host).cuda()
        assert self.t.data_ptr() % 256 == 0 and head >= SLACK and self.t.numel() - (head + n * stride) >= SLACK
        self.ptr, self.n, self.stride, self.head = self.t.data_ptr() + head, n, stride, head
        self.lens_np = lens_np if lens else None
        self.t_lens = torch.from_numpy(lens_np.copy()).cuda() if lens and n else None
        self.t_time = torch.from_numpy(np.ascontiguousarray(times, dtype=np.float64)).cuda() if times is not None else None
        assert self.t_lens is None or self.t_lens.data_ptr() % 2 == 0
        assert self.t_time is None or self.t_time.data_ptr() % 8 == 0
        torch.cuda.synchronize()

    def body(self):
        return self.host[self.head:self.head + self.n * self.stride]

    def ingest(self, m):
        m.ingest_device(self.ptr, self.n, self.stride, self.t_lens.data_ptr() if self.t_lens is not None else 0,
                        self.t_time.data_ptr() if self.t_time is not None else 0)
        m.sync()                                   # the tensors may go once the context has read them


def _pool(pkg, stride, with_lens, n, seed, max_agent=7):
    rng = np.random.default_rng(seed)
    pool = dr.make_pool(_base(pkg, max_agent, seed), rng, max_agent, n, odd_lengths=with_lens)
    return dr.fit(pool, stride, with_lens), rng


# ---- stride sweep, host path -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quiet(pkg):
    """A context that closes no loop (drift 0.0: the reported pose is the decoded one, bit for bit); landmarks are still logged."""
    with _mapper(pkg, min_poses_between=NO_CLOSURES) as m:
        yield m


@pytest.mark.parametrize("stride,with_lens", HOST_CASES, ids=[f"{s}{'' if wl else '_nolens'}" for s, wl in HOST_CASES])
def test_stride_sweep_host_path(pkg, quiet, stride, with_lens):
    """Every stride 41..64 (LDS-staged kernel) and 65, 72, 100, 255 (wide kernel), each at 1, 255, 256, 257, 2047, 2048, 2049,
    4097 and 5003 records (tile = 256, workgroup = 2048): accept and pose bit for bit, counters, per-graph counts, landmark
    types, against the byte-level reference."""
    pool, rng = _pool(pkg, stride, with_lens, NS[-1], seed=1000 + stride + 500 * with_lens)
    off = _offsets(7)
    full_buf, full_lens = dr.build(pool, stride, rng)
    ref_all = dr.decode(full_buf, len(pool), stride, full_lens if with_lens else None, 7, off)
    _share(ref_all, f"stride {stride} pool")
    first_ok, first_bad = int(np.argmax(ref_all["accept"] == 1)), int(np.argmax(ref_all["accept"] == 0))
    runs = [("n=1 accepted", [pool[first_ok]]), ("n=1 rejected", [pool[first_bad]])] + [(f"n={n}", pool[:n]) for n in NS[1:]]
    for name, recs in runs:
        tag = f"stride {stride}{'' if with_lens else ' (no lengths)'}, {name}"
        n = len(recs)
        buf, lens = dr.build(recs, stride, rng)
        lens = lens if with_lens else None
        ref = dr.decode(buf, n, stride, lens, 7, off)
        if n >= 255:
            _share(ref, tag)
        quiet.reset()
        quiet.ingest_array(buf.reshape(n, stride), lens)
        _check_decode(quiet, ref, 7, 2, tag)


@pytest.mark.parametrize("n", [255, 2049, 4097])
@pytest.mark.parametrize("stride,with_lens", FULL_CASES, ids=[f"{s}{'' if wl else '_nolens'}" for s, wl in FULL_CASES])
def test_full_state_vs_oracle_host_path(pkg, stride, with_lens, n):
    """Map, hit points, pose graphs (closures on), zones, EKF and counters against the oracle, below and above the direct /
    tiled raycast switch (256) and the serial / scan EKF switch (4096)."""
    pool, rng = _pool(pkg, stride, with_lens, n, seed=2000 + stride + 500 * with_lens + n)
    buf, lens = dr.build(pool, stride, rng)
    lens = lens if with_lens else None
    ref = dr.decode(buf, n, stride, lens, 7, _offsets(7))
    tag = f"stride {stride}, n={n}"
    _share(ref, tag)
    times = _times(n, n)
    w = _Walk(_P(pkg), dr.datagrams(buf, n, stride, lens), times=times, ekf=True)
    with _mapper(pkg, enable_ekf=True) as m:
        m.ingest_array(buf.reshape(n, stride), lens, recv_time=times)
        _check_decode(m, ref, 7, 2, tag, pose_exact=False)
        _check_oracle(m, ref, w, 7, 2, tag, ekf=True)


# ---- device path and alignment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,with_lens", DEVICE_CASES, ids=[f"{s}{'' if wl else '_nolens'}" for s, wl in DEVICE_CASES])
def test_device_path_at_every_alignment(pkg, stride, with_lens):
    """qs_ingest_device with record 0 at byte offsets 0, 1, 2, 3 and 5 past a 4-byte boundary, inside a tensor with 64 bytes of
    slack either side that hold acceptable records: every observable equals the host path's on the same records, the byte-level
    reference and the oracle.  d_lens is a uint16 tensor or 0, d_time a float64 tensor or 0 (even strides run the EKF)."""
    n, ekf = 2305, stride % 2 == 0                       # ten tiles: workgroup 0 full, workgroup 1 = one tile + one record
    pool, rng = _pool(pkg, stride, with_lens, n, seed=3000 + stride)
    times = _times(n, stride) if ekf else None
    buf, lens = dr.build(pool, stride, rng)
    lens = lens if with_lens else None
    ref = dr.decode(buf, n, stride, lens, 7, _offsets(7))
    _share(ref, f"stride {stride}")
    w = _Walk(_P(pkg), dr.datagrams(buf, n, stride, lens), times=times, ekf=ekf)
    with _mapper(pkg, enable_ekf=ekf) as m:
        m.ingest_array(buf.reshape(n, stride), lens, recv_time=times)
        _check_oracle(m, ref, w, 7, 2, f"stride {stride}, host", ekf=ekf)
        host_state, host_batch = _observe(m, 7, 2, ekf), _observe_batch(m)
    for off in DEVICE_OFFSETS:
        tag = f"stride {stride}, device offset {off}"
        d = _OnDevice(pool, stride, np.random.default_rng(off), off, lens=with_lens, times=times, body=buf)
        assert d.ptr % 4 == off % 4
        ref_d = dr.decode(d.body(), n, stride, d.lens_np, 7, _offsets(7))
        _same({k: ref_d[k] for k in ("accept", "agent", "lm", "enc", "dist")}, {k: ref[k] for k in ("accept", "agent", "lm", "enc", "dist")}, tag)
        with _mapper(pkg, enable_ekf=ekf) as m:
            d.ingest(m)
            _check_decode(m, ref, 7, 2, tag, pose_exact=False)
            _check_oracle(m, ref, w, 7, 2, tag, ekf=ekf)
            _same(_observe(m, 7, 2, ekf), host_state, tag)
            _same(_observe_batch(m), host_batch, tag)


def test_device_alignment_reaches_every_shift(pkg, quiet):
    """All (offset, stride) pairs of the device case again on the context that closes no loop -- pose bit for bit -- and, from
    the kernel's own arithmetic on the addresses actually used, what they reach: all 16 (mis, sh) pairs, the bytewise branch
    at the start and at the end of a buffer, and the wide kernel."""
    reached, bytewise_first, bytewise_last, wide = set(), 0, 0, 0
    n = 2305
    for stride, with_lens in DEVICE_CASES:
        pool, rng = _pool(pkg, stride, with_lens, n, seed=3500 + stride)
        for off in DEVICE_OFFSETS:
            tag = f"stride {stride}, device offset {off}"
            d = _OnDevice(pool, stride, rng, off, lens=with_lens)
            ref = dr.decode(d.body(), n, stride, d.lens_np, 7, _offsets(7))
            _share(ref, tag)
            quiet.reset()
            d.ingest(quiet)
            _check_decode(quiet, ref, 7, 2, tag)
            if stride <= dr.MAX_LDS_STRIDE:
                reached |= dr.shifts(d.ptr, n, stride)
                tiles = dr.bytewise_tiles(d.ptr, n, stride)
                bytewise_first += 0 in tiles
                bytewise_last += (n - 1) // dr.TILE in tiles
            else:
                wide += 1
    assert reached == {(mis, sh) for mis in range(4) for sh in range(4)}
    assert bytewise_first >= 10 and bytewise_last >= 10 and wide == len(DEVICE_OFFSETS)


# ---- tile and workgroup edges with rejections -------------------------------------------------------------------------------
def _patterned(pool, ref, mask):
    good = [r for r, a in zip(pool, ref["accept"]) if a]
    bad = [r for r, a in zip(pool, ref["accept"]) if not a]
    gi = bi = 0
    out = []
    for keep in mask:
        if keep:
            out.append(good[gi % len(good)]); gi += 1
        else:
            out.append(bad[bi % len(bad)]); bi += 1
    return out


@pytest.mark.parametrize("stride,with_lens,dev_off", [(41, False, None), (43, True, None), (64, True, None), (72, True, None),
                                                      (41, False, 3), (43, True, 1), (64, True, 3), (72, True, 1)])
def test_rejections_across_tile_and_workgroup_edges(pkg, quiet, stride, with_lens, dev_off):
    """Runs of rejected records straddling records 255/256, 2047/2048 and the last, partial tile; then the first and last
    record of the batch the only accepted ones; then the only rejected ones.  n * stride is odd for the odd strides here, so
    the last tile is staged bytewise on the host path too; the offset device buffers add the first tile."""
    n = 2405
    pool, rng = _pool(pkg, stride, with_lens, 6000, seed=4000 + stride)
    buf, lens = dr.build(pool, stride, rng)
    ref_pool = dr.decode(buf, len(pool), stride, lens if with_lens else None, 7, _offsets(7))
    _share(ref_pool, f"stride {stride} pool")
    runs = np.ones(n, dtype=bool)
    for lo, hi in ((200, 300), (1900, 2200), (2290, 2330), (2381, n)):
        runs[lo:hi] = False
    ends_kept = np.zeros(n, dtype=bool)
    ends_kept[[0, n - 1]] = True
    for name, mask in (("runs", runs), ("ends kept", ends_kept), ("ends dropped", ~ends_kept)):
        tag = f"stride {stride}, {name}, {'host' if dev_off is None else f'device offset {dev_off}'}"
        recs = _patterned(pool, ref_pool, mask)
        quiet.reset()
        if dev_off is None:
            b, ln = dr.build(recs, stride, rng)
            ln = ln if with_lens else None
            ref = dr.decode(b, n, stride, ln, 7, _offsets(7))
            quiet.ingest_array(b.reshape(n, stride), ln)
        else:
            d = _OnDevice(recs, stride, rng, dev_off, lens=with_lens)
            ref = dr.decode(d.body(), n, stride, d.lens_np, 7, _offsets(7))
            d.ingest(quiet)
        assert (ref["accept"] == mask).all(), tag
        if name == "runs":
            _share(ref, tag)
        _check_decode(quiet, ref, 7, 2, tag)


@pytest.mark.parametrize("dev_off", [None, 1])
def test_length_above_the_stride_is_refused(pkg, quiet, dev_off):
    """Stride 41 WITH lengths: a record whose length says 42 does not fit its slot and is dropped (a decoder without the
    len <= stride rule would take the next record's 'Q' for its landmark byte and accept it); the 41-byte ones around it
    decode.  The byte-level reference is the yardstick here: a datagram longer than its slot has no meaning to the oracle."""
    stride = 41
    for n in (255, 2049):
        rng = np.random.default_rng(4500 + n)
        pool = dr.make_pool(_base(pkg, 7, 45), rng, 7, n, reject_share=0.2)
        pool = [r[:41] if len(r) == 42 and rng.random() < 0.9 else r for r in pool]
        tag = f"stride 41 with lengths, n={n}, {'host' if dev_off is None else f'device offset {dev_off}'}"
        quiet.reset()
        if dev_off is None:
            buf, lens = dr.build(pool, stride, rng)
            quiet.ingest_array(buf.reshape(n, stride), lens)
        else:
            d = _OnDevice(pool, stride, rng, dev_off)
            buf, lens = d.body(), d.lens_np
            d.ingest(quiet)
        ref = dr.decode(buf, n, stride, lens, 7, _offsets(7))
        _share(ref, tag)
        too_long = lens == 42
        assert too_long.sum() >= 10 and not ref["accept"][too_long].any() and ref["accept"][lens == 41].sum() > n // 2
        _check_decode(quiet, ref, 7, 2, tag)


# ---- graph counts, both forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_agent,bots_per_graph", [(64, 2), (255, 1), (255, 0)], ids=["32_graphs_lds", "255_graphs_global", "one_graph"])
def test_per_graph_counts_over_several_workgroups(pkg, max_agent, bots_per_graph):
    """About 20 000 records over ten workgroups: 32 graphs (the LDS histogram), 255 graphs (global atomics) and one graph.
    slam_sizes of every graph equal the reference's accepted and landmark-event counts, the landmark lists imply the reference's
    per-bot event counts; the whole state against the oracle at stride 45 (LDS-staged), the counts again at 72 (wide)."""
    n = 20011
    for stride in (45, 72):
        pool, rng = _pool(pkg, stride, True, n, seed=5000 + max_agent + bots_per_graph + stride, max_agent=max_agent)
        buf, lens = dr.build(pool, stride, rng)
        ref = dr.decode(buf, n, stride, lens, max_agent, _offsets(max_agent))
        tag = f"{max_agent} bots, {bots_per_graph} per graph, stride {stride}"
        _share(ref, tag)
        with _mapper(pkg, max_agent=max_agent, bots_per_graph=bots_per_graph) as m:
            m.ingest_array(buf.reshape(n, stride), lens)
            _check_decode(m, ref, max_agent, bots_per_graph, tag, pose_exact=False)
            if stride == 45:
                w = _Walk(_P(pkg), dr.datagrams(buf, n, stride, lens), max_agent=max_agent, bots_per_graph=bots_per_graph)
                _check_oracle(m, ref, w, max_agent, bots_per_graph, tag)


# ---- sharded contexts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,with_lens", [(42, False), (72, True)])
def test_sharded_contexts_through_both_kernels(pkg, stride, with_lens):
    """shard_bots = 2 of 4 bots (map_ok != accept): every shard accepts every decodable record into the pose graph, casts rays,
    keeps zones and runs the EKF for its own two bots only -- the oracle with the same ownership -- through the LDS-staged
    kernel (stride 42) and the wide one (72).  The two shards' ray counts add up to the unsharded oracle's."""
    n = 3001
    pool, rng = _pool(pkg, stride, with_lens, n, seed=6000 + stride, max_agent=4)
    buf, lens = dr.build(pool, stride, rng)
    lens = lens if with_lens else None
    ref = dr.decode(buf, n, stride, lens, 4, _offsets(4))
    _share(ref, f"stride {stride}")
    times = _times(n, 6)
    grams = dr.datagrams(buf, n, stride, lens)
    whole = _Walk(_P(pkg), grams, max_agent=4, bots_per_graph=0, times=times, per_record=False).o
    rays = 0
    for rank, owned in ((0, (1, 2)), (1, (3, 4))):
        tag = f"stride {stride}, shard {rank}"
        w = _Walk(_P(pkg), grams, max_agent=4, bots_per_graph=0, times=times, ekf=True, owned=owned)
        assert (w.acc == ref["accept"]).all()
        unowned = (ref["accept"] == 1) & ((ref["agent"] < owned[0]) | (ref["agent"] > owned[1]))
        assert unowned.sum() > 100 and not w.valid[unowned].any()
        with _mapper(pkg, max_agent=4, bots_per_graph=0, shard_bots=2, shard_rank=rank, enable_ekf=True) as m:
            m.ingest_array(buf.reshape(n, stride), lens, recv_time=times)
            _check_decode(m, ref, 4, 0, tag, pose_exact=False)
            _check_oracle(m, ref, w, 4, 0, tag, ekf=True, owned=owned)
            assert not (m.grid_i8() == whole.grid).all()
            rays += m.counters()["rays"]
    assert rays == whole.n_rays


# ---- batch splitting across strides and entry points ---------------------------------------------------------------------------
def test_batch_splitting_across_strides_and_entry_points(pkg):
    """The same records as one host call at stride 48, and as ragged calls that alternate the host and the device entry point
    (offsets 1, 2, 3, 5) and repack at strides 43, 64, 72, 57, 100, 42, 255 between calls: the same map, pose graphs, zones and
    EKF state, bit for bit (every call is below the EKF's scan switch), and the oracle's."""
    n = 4000
    pool, rng = _pool(pkg, 48, True, n, seed=7000)
    pool = dr.fit(pool, 42, True)                       # (every record fits every stride used below)
    times = _times(n, 7)
    buf, lens = dr.build(pool, 48, rng)
    ref = dr.decode(buf, n, 48, lens, 7, _offsets(7))
    _share(ref, "pool")
    w = _Walk(_P(pkg), dr.datagrams(buf, n, 48, lens), times=times, ekf=True)
    with _mapper(pkg, enable_ekf=True) as m:
        m.ingest_array(buf.reshape(n, 48), lens, recv_time=times)
        n_cls = _check_oracle(m, ref, w, 7, 2, "one call", ekf=True)
        assert n_cls > 0
        one = _observe(m, 7, 2, True)
    sizes = [1, 255, 256, 257, 1000, 3, 700, 2, 1526]
    strides = [43, 64, 72, 57, 100, 42, 255, 45, 65]
    assert sum(sizes) == n
    with _mapper(pkg, enable_ekf=True) as m:
        lo = 0
        for k, (size, stride) in enumerate(zip(sizes, strides)):
            recs, t = pool[lo:lo + size], times[lo:lo + size]
            if k % 2 == 0:
                b, ln = dr.build(recs, stride, rng)
                m.ingest_array(b.reshape(size, stride), ln, recv_time=t)
            else:
                _OnDevice(recs, stride, rng, (1, 2, 3, 5)[(k // 2) % 4], times=t).ingest(m)
            acc, _ = m.last_batch()
            assert (acc == ref["accept"][lo:lo + size]).all(), f"call {k} (stride {stride})"
            lo += size
        _same(_observe(m, 7, 2, True), one, "ragged calls")


# ---- sweeps, device entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odometry", [False, True], ids=["743", "751"])
def test_sweeps_device_entry_at_offsets(pkg, odometry):
    """qs_ingest_sweeps_device with record 0 at byte offsets 1, 2 and 3 (slack as above) equals qs_ingest_sweeps on the same
    records: map, counters, accepted flags and poses.  (The strides are odd, so every per-record shift runs on the host path
    already; this adds the entry point and the start-of-buffer bytewise branch of sw_stage.)"""
    P = _P(pkg)
    n, rng = 300, np.random.default_rng(8 + odometry)
    r = rng.uniform(0.0, 1.6, (n, 181)).astype(np.float32)
    r[rng.random((n, 181)) < 0.03] = np.nan
    agent = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), n, p=[.1, .4, .4, .1])
    buf = P.pack_sweeps(agent, rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-np.pi, np.pi, n), r, odometry=odometry).copy()
    bad_magic = rng.random(n) < 0.1
    buf[bad_magic, 2] ^= 0x20
    stride = buf.shape[1]
    assert stride == (751 if odometry else 743)
    lens = np.full(n, stride, dtype=np.uint16)
    lens[rng.random(n) < 0.05] = stride - 1
    want_acc = (~bad_magic & (agent >= 1) & (agent <= 2) & (lens == stride)).astype(np.uint8)
    assert 0.15 <= 1.0 - want_acc.mean() <= 0.40
    with _mapper(pkg, max_agent=2, bots_per_graph=0) as m:
        m.ingest_sweeps(buf, lens)
        host = dict(grid=m.grid_i8(), counters=np.array([m.counters()[k] for k in MAP_COUNTERS], dtype=np.uint64))
        host["hits"], host["misses"] = m.counts()
        host["acc"], host["pose"] = m.last_sweeps()
    assert (host["acc"] == want_acc).all() and (host["grid"] != -1).sum() > 1000
    rows = [row.tobytes() for row in buf]
    for off in (1, 2, 3):
        d = _OnDevice(rows, stride, rng, off)
        d.t_lens = torch.from_numpy(lens.copy()).cuda()
        torch.cuda.synchronize()
        assert (d.body().reshape(n, stride) == buf).all() and d.ptr % 4 == off
        with _mapper(pkg, max_agent=2, bots_per_graph=0) as m:
            m.ingest_sweeps_device(d.ptr, n, stride, d.t_lens.data_ptr())
            m.sync()
            dev = dict(grid=m.grid_i8(), counters=np.array([m.counters()[k] for k in MAP_COUNTERS], dtype=np.uint64))
            dev["hits"], dev["misses"] = m.counts()
            dev["acc"], dev["pose"] = m.last_sweeps()
        _same(dev, host, f"sweeps stride {stride}, device offset {off}")


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_unchanged(pkg):
    """A stride below 41 is QS_E_INVAL on both entry points and changes nothing; n == 0 with a NULL pointer is accepted."""
    import ctypes as C
    n, stride = 500, 48
    pool, rng = _pool(pkg, stride, True, n, seed=9000)
    buf, lens = dr.build(pool, stride, rng)
    with _mapper(pkg, enable_ekf=True) as m:
        m.ingest_array(buf.reshape(n, stride), lens, recv_time=_times(n, 9))
        before, batch = _observe(m, 7, 2, True), _observe_batch(m)
        d = _OnDevice(pool[:100], 40, rng, 1, lens=False)
        for bad_stride in (40, 1, 0):
            with pytest.raises(pkg.QuasarError, match=r"\(-1\)"):
                m.ingest_array(np.zeros((100, bad_stride), dtype=np.uint8) if bad_stride else np.zeros((100, 0), dtype=np.uint8))
            rc = m._L.qs_ingest_device(m._h, C.c_void_p(d.ptr), 100, bad_stride, None, None, 2 ** 64 - 1)
            assert rc == -1, bad_stride
        m._last_n = n
        _same(_observe(m, 7, 2, True), before, "after refused calls")
        _same(_observe_batch(m), batch, "after refused calls")
        assert m._L.qs_ingest(m._h, None, 0, 42, None, None, 2 ** 64 - 1) == 0
        assert m._L.qs_ingest_device(m._h, None, 0, 42, None, None, 2 ** 64 - 1) == 0
        _same(_observe(m, 7, 2, True), before, "after empty calls")
        assert m.counters()["datagrams"] == n
