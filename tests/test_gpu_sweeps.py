"""Servo-sweep packets (qs_ingest_sweeps) on the GPU.  The bar: the reference's OccupancyGrid.update_ray driven beam by beam
with the sweep rule of include/quasar_slam.h -- the golden fixture (tests/golden/make_sweep_golden.py) and the CPU oracle
fed the same beams in the same order, end points from Python's math.cos / math.sin (glibc, as CPython) -- cell for cell,
counters included."""
import importlib
import math
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import GOLDEN, load_pkg
from oracle import oracle as orc
from walk_ops import sweep_beams as _beams

pytestmark = pytest.mark.gpu
SMIN, SMAX = 0.1, 1.2


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _records(P, buf):
    dt = P.PACKET_DTYPE_V0 if buf.shape[1] == P.PACKET_SIZE_V0 else P.PACKET_DTYPE_V0_ODO
    return np.ascontiguousarray(buf).view(dt).reshape(-1)


def _same_map(m, o, tag):
    g = m.grid_i8()
    assert (g == o.grid).all(), f"{tag}: {(g != o.grid).sum()} cells differ from the oracle"
    h, mi = m.counts()
    assert (h == o.hits).all() and (mi == o.misses).all(), f"{tag}: counters differ"


def _stamps(pkg, m):
    distmod = importlib.import_module(pkg.__name__ + ".dist")
    st, _ = distmod.grid_tensors(m, torch.device("cuda", 0))
    torch.cuda.synchronize()
    return st.cpu().numpy().copy()


def _random_sweeps(P, n, seed, lo=-20.0, hi=20.0, odometry=True, agents=(1, 2)):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0, 1.6, (n, 181)).astype(np.float32)
    r[rng.random((n, 181)) < 0.03] = np.nan
    return P.pack_sweeps(rng.choice(np.array(agents), n), rng.uniform(lo, hi, n), rng.uniform(lo, hi, n),
                         rng.uniform(-math.pi, math.pi, n), r, odometry=odometry)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fmt", ["sweeps_v0", "sweeps_odo"])
def test_golden_sweeps(pkg, fmt, mode):
    g = np.load(os.path.join(GOLDEN, "sweeps_512.npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep, raycast_mode=mode) as m:
        assert m.ingest_sweeps(g[fmt]) == len(g[fmt])
        assert (m.grid_i8() == g["grid"]).all(), f"{(m.grid_i8() != g['grid']).sum()} cells differ from the reference"
        h, mi = m.counts()
        assert (h == g["hits"]).all() and (mi == g["misses"]).all()
        acc, pose = m.last_sweeps()
        assert (acc == g["accepted"]).all()
        c = m.counters()
        n_acc = int(g["accepted"].sum())
        assert c["datagrams"] == len(g[fmt]) and c["accepted"] == n_acc and c["rays"] == 181 * n_acc


def test_random_sweeps_equal_the_oracle_and_direct_equals_tiled(pkg):
    P = _P(pkg)
    n, G, half = 1 << 14, 4096, 102.4
    buf = _random_sweeps(P, n, seed=77)
    o = orc.OracleMapper(G, 0.05, -half, -half, 0.0)
    o.update_rays(*_beams(_records(P, buf)))
    stamps = []
    for mode in (1, 2):
        with pkg.QuasarMapper(G, 0.05, -half, -half, raycast_mode=mode) as m:
            m.ingest_sweeps(buf)
            _same_map(m, o, f"mode {mode}")
            stamps.append(_stamps(pkg, m))
    assert (stamps[0] == stamps[1]).all(), f"{(stamps[0] != stamps[1]).sum()} stamps differ between direct and tiled"
    assert stamps[0].max() <= 2 * 4 * 46 * n + 1


def test_long_beams_take_the_direct_branch_of_the_tiled_pass(pkg):
    """At 13 mm a 1.2 m beam spans 92 cells, more than a 64-cell tile: most beams of pass A leave the binning for the
    direct walk.  Direct and tiled, counts on and off, equal the oracle; so does the matched ingest on the empty map
    (nothing to match against: zero corrections), which runs the corrected instantiation of the same pass."""
    P = _P(pkg)
    n, G, res = 64, 260, 0.013
    half = G * res / 2
    buf = _random_sweeps(P, n, seed=13, lo=-0.9 * half, hi=0.9 * half)
    o = orc.OracleMapper(G, res, -half, -half, 0.0)
    o.update_rays(*_beams(_records(P, buf)))
    stamps, cells = {}, {}
    for mode in (1, 2):
        for counts in (True, False):
            with pkg.QuasarMapper(G, res, -half, -half, raycast_mode=mode, enable_counts=counts) as m:
                m.ingest_sweeps(buf)
                assert (m.grid_i8() == o.grid).all(), f"mode {mode}, counts {counts}: {(m.grid_i8() != o.grid).sum()} cells differ"
                if counts:
                    _same_map(m, o, f"mode {mode}")
                    stamps[mode] = _stamps(pkg, m)
                cells[mode, counts] = m.counters()["cells"]
    assert (stamps[1] == stamps[2]).all(), f"{(stamps[1] != stamps[2]).sum()} stamps differ between direct and tiled"
    assert len(set(cells.values())) == 1 and cells[1, True] == o.n_cells_written, cells
    d_buf = torch.from_numpy(buf).cuda()
    with pkg.QuasarMapper(G, res, -half, -half, raycast_mode=2) as m:
        m.ingest_sweeps_matched_device(d_buf.data_ptr(), n, buf.shape[1])
        m.sync()
        mt = m.last_sweep_matches()
        assert not (mt["dx"].any() or mt["dy"].any() or mt["dyaw"].any())
        _same_map(m, o, "matched, device")


def test_interleaved_with_packets_closures_and_separation(pkg):
    P = _P(pkg)
    g = np.load(os.path.join(GOLDEN, "session_sep_512.npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    dg, ln = g["datagrams"], g["lengths"]
    cut = 2 * len(dg) // 3
    sw = _random_sweeps(P, 300, seed=3, lo=-3.0, hi=3.0, odometry=False)
    for mode in (0, 2):
        o = orc.OracleMapper(int(size), res, ox, oy, sep)
        o.feed_stream(dg[:cut], ln[:cut])
        drift = {b: tuple(o.drift(b)) for b in (1, 2)}
        assert any(v != (0.0, 0.0) for v in drift.values()), "the first part must close a loop"
        o.update_rays(*_beams(_records(P, sw), {2: float(sep)}, drift))
        o.feed_stream(dg[cut:], ln[cut:])
        with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep, raycast_mode=mode) as m:
            m.ingest_array(dg[:cut], ln[:cut])
            m.ingest_sweeps(sw)
            acc, pose = m.last_sweeps()
            rec = _records(P, sw)
            for k in range(len(rec)):
                a_id = int(rec["agent"][k])
                assert pose[k, 0] == float(rec["x"][k]) + (float(sep) if a_id == 2 else 0.0) + drift[a_id][0]
                assert pose[k, 1] == float(rec["y"][k]) + drift[a_id][1]
            m.ingest_array(dg[cut:], ln[cut:])
            _same_map(m, o, f"mode {mode}")


def test_later_beam_then_next_packet_win(pkg):
    P = _P(pkg)
    r = np.full(181, np.nan, dtype=np.float32)
    r[90] = 0.5                       # heading 0: an occupied end cell 0.5 m ahead
    # beam 91 (1 degree left) is a 1.2 m free ray through that same cell: the later beam wins it
    sw = P.pack_sweeps([1], [0.0125], [0.0125], [0.0], r[None, :])
    pkt = np.frombuffer(P.pack_packet(1, 0.0125, 0.0125, 0.0, 0, 0, 0.5, 9.0, 9.0, 9.0, 0), np.uint8)[None, :]
    o = orc.OracleMapper(200, 0.05, -5.0, -5.0)
    gx, gy = (int((0.0125 + 0.5 + 5.0) / 0.05), int((0.0125 + 5.0) / 0.05))
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        m.ingest_sweeps(sw)
        o.update_rays(*_beams(_records(P, sw)))
        assert m.grid_i8()[gy, gx] == 0 and o.grid[gy, gx] == 0
        h, mi = m.counts()
        assert h[gy, gx] == 1 and mi[gy, gx] >= 1
        _same_map(m, o, "sweep")
        m.ingest_array(pkt)                                     # the next packet's front ray ends there: occupied again
        o.feed_stream(pkt)
        assert m.grid_i8()[gy, gx] == 100
        _same_map(m, o, "sweep then packet")


def test_rejects_and_last_sweeps(pkg):
    P = _P(pkg)
    r = np.full(181, 0.6, dtype=np.float32)
    good = P.pack_v0_odo(1, 0.5, 0.5, 0.0, 0, 0, r, scan_count=7)      # scan_count is ignored
    recs = [good, b"QSRX" + good[4:], good[:4] + b"\x00" + good[5:], good[:4] + b"\x03" + good[5:], good]
    lens = np.array([751, 751, 751, 751, 700], dtype=np.uint16)
    buf = np.stack([np.frombuffer(x, np.uint8) for x in recs])
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        m.ingest_sweeps(buf, lens)
        acc, pose = m.last_sweeps()
        assert acc.tolist() == [1, 0, 0, 0, 0]
        assert pose[0].tolist() == [0.5, 0.5, 0.0] and np.isnan(pose[1:]).all()
        c = m.counters()
        assert c["datagrams"] == 5 and c["accepted"] == 1 and c["rays"] == 181
        with pytest.raises(pkg.QuasarError):
            m.last_batch()                                      # the last ingest was a sweep call
        with pytest.raises(pkg.QuasarError):
            m.last_hits()
        # mixed lengths in a list: one format per call
        with pytest.raises(ValueError):
            m.ingest_sweeps([good, good[:743]])
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        m.ingest_sweeps(buf[1:4])
        assert (m.grid_i8() == -1).all() and m.last_sweeps()[0].tolist() == [0, 0, 0]
        m.ingest_sweeps(buf[:1], seq0=None)
        m.ingest_array(np.frombuffer(P.pack_packet(1, 0.5, 0.5, 0.0, 0, 0, 9.0, 9.0, 9.0, 9.0, 0), np.uint8)[None, :])
        acc, pose = m.last_batch()
        assert acc.tolist() == [1]
        with pytest.raises(pkg.QuasarError):
            m.last_sweeps()


def test_sequence_numbers_follow_sweeps(pkg):
    P = _P(pkg)
    r = np.full(181, np.nan, dtype=np.float32)
    r[180] = 0.5         # the last beam (+90 degrees): nothing later in the sweep crosses its end cell
    sw = P.pack_sweeps([1, 1, 1], [0.0125] * 3, [0.0125] * 3, [0.0] * 3, np.repeat(r[None, :], 3, 0))
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        m.ingest_sweeps(sw, seq0=10)
        st = _stamps(pkg, m)
        gx, gy = int((0.0125 + 5.0) / 0.05), int((0.0125 + 0.5 + 5.0) / 0.05)
        # the last sweep's beam 180 wrote the end cell: ordinal 4 (10 + 46 * 2) + 180 + 1, occupied
        assert st[gy, gx] == ((4 * (10 + 46 * 2) + 180 + 1) << 1) | 1
        m.ingest_array(np.frombuffer(P.pack_packet(1, 3.0125, 3.0125, 0.0, 0, 0, 0.5, 9.0, 9.0, 9.0, 0), np.uint8)[None, :])
        st = _stamps(pkg, m)
        gx2, gy2 = int((3.0125 + 0.5 + 5.0) / 0.05), int((3.0125 + 5.0) / 0.05)
        assert st[gy2, gx2] == ((4 * (10 + 46 * 3) + 0 + 1) << 1) | 1   # next_seq = seq0 + 46 n


def test_edge_band_beams_are_resolved_on_the_host(pkg):
    P = _P(pkg)
    # pose (0, 0), yaw 0 on a 5 cm grid from -12.8: beams 0, 90 and 180 point at -90, 0 and +90 degrees, and each of their
    # end points lies on a cell boundary (y = -0.5, x = 0.25 / 1.3, y = 1.2 / 1.25), so the host recomputes all three --
    # from the beam index (a wrong sign or offset of (i - 90) * pi / 180 would mirror beams 0 and 180) and with the sweep
    # filter (beams 90 and 180 change sides between the two filters below)
    r = np.full(181, np.nan, dtype=np.float32)
    r[0], r[90], r[180] = 0.5, 0.25, 1.25
    sw = P.pack_sweeps([1], [0.0], [0.0], [0.0], r[None, :])
    for smin, smax in ((SMIN, SMAX), (0.3, 1.3)):
        o = orc.OracleMapper(512, 0.05, -12.8, -12.8)
        o.update_rays(*_beams(_records(P, sw), smin=smin, smax=smax))
        for mode in (1, 2):
            with pkg.QuasarMapper(512, 0.05, -12.8, -12.8, raycast_mode=mode) as m:
                m.set_sweep_filter(smin, smax)
                m.ingest_sweeps(sw)
                _same_map(m, o, f"filter {smin} .. {smax}, mode {mode}")
                assert m.counters()["edge_rays"] >= 3
    # with exact_trig off every beam is cast with the device's trig: nothing waits for the host
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8, exact_trig=False) as m:
        m.ingest_sweeps(sw)
        assert m.counters()["edge_rays"] == 0


class _FakeSock:
    """A socket that hands out a fixed list of datagrams (MissionControl's recvfrom_into / sendto)."""

    def __init__(self, datagrams):
        self.q = list(datagrams)

    def setblocking(self, flag):
        pass

    def recvfrom_into(self, view, nbytes):
        if not self.q:
            raise BlockingIOError
        d = self.q.pop(0)
        m = min(len(d), nbytes)
        view[:m] = d[:m]
        return m, ("127.0.0.1", 40000)

    def sendto(self, data, addr):
        return len(data)

    def close(self):
        pass


def test_front_end_continues_the_mappers_sequence(pkg):
    """A replayed sweep log, then live traffic over the same room through MissionControl(sweeps=True): the live runs take
    their sequence numbers after the replay's, so live observations win cells the replay wrote."""
    P = _P(pkg)
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    logged = _random_sweeps(P, 40, seed=31, lo=-1.0, hi=1.0)
    live_sw = _random_sweeps(P, 6, seed=32, lo=-1.0, hi=1.0)
    pk = P.pack_packets([1, 2] * 5, np.linspace(-1, 1, 10), np.linspace(1, -1, 10), np.linspace(0, 6, 10), np.arange(10),
                        np.zeros(10), np.full((10, 4), 0.7), np.zeros(10))
    live = [x.tobytes() for x in pk[:5]] + [x.tobytes() for x in live_sw[:3]] + [x.tobytes() for x in pk[5:]] + \
           [x.tobytes() for x in live_sw[3:]]
    o = orc.OracleMapper(200, 0.05, -5.0, -5.0)
    o.update_rays(*_beams(_records(P, logged)))
    o.feed_stream(pk[:5])
    o.update_rays(*_beams(_records(P, live_sw[:3])))
    o.feed_stream(pk[5:])
    o.update_rays(*_beams(_records(P, live_sw[3:])))
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        m.ingest_sweeps(logged)
        mc = fe.MissionControl(m, sock=_FakeSock(live), sweeps=True)
        assert mc.poll(now=1.0) == len(live)
        _same_map(m, o, "replay, then live")
        assert mc.online == {1: True, 2: True}
        # the mapper's next sequence number is 46 * 40 + 5 + 46 * 3 + 5 + 46 * 3: the next packet's front ray says so
        m.ingest_array(np.frombuffer(P.pack_packet(1, 3.0125, 3.0125, 0.0, 0, 0, 0.5, 9.0, 9.0, 9.0, 0), np.uint8)[None, :])
        gx, gy = int((3.0125 + 0.5 + 5.0) / 0.05), int((3.0125 + 5.0) / 0.05)
        nxt = 46 * 40 + 5 + 46 * 3 + 5 + 46 * 3
        assert _stamps(pkg, m)[gy, gx] == ((4 * nxt + 1) << 1) | 1


def test_sparse_fuse_of_sweep_only_shards_equals_dense(pkg):
    P = _P(pkg)
    distmod = importlib.import_module(pkg.__name__ + ".dist")
    dev = torch.device("cuda", 0)
    G, half = 1024, 25.6
    parts = [_random_sweeps(P, 700, seed=11, lo=-20.0, hi=0.0), _random_sweeps(P, 900, seed=12, lo=-5.0, hi=15.0)]
    mappers = [pkg.QuasarMapper(G, 0.05, -half, -half, raycast_mode=2 - r) for r in range(2)]
    try:
        for m in mappers:
            m.dirty_tracking(True)
        mappers[0].ingest_sweeps(parts[0], seq0=0)
        mappers[1].ingest_sweeps(parts[1], seq0=46 * 700)
        st = [_stamps(pkg, m) for m in mappers]
        cnt = [m.counts() for m in mappers]
        for m in mappers:
            assert m.dirty_blocks()[0] > 0
        distmod.sparse_fuse_local(mappers, dev)
        expect = np.maximum(st[0], st[1])
        hits, misses = cnt[0][0] + cnt[1][0], cnt[0][1] + cnt[1][1]
        for r, m in enumerate(mappers):
            assert (_stamps(pkg, m) == expect).all(), f"rank {r}: stamps differ from the dense fuse"
            h, mi = m.counts()
            assert (h == hits).all() and (mi == misses).all(), f"rank {r}: counters differ from the dense fuse"
    finally:
        for m in mappers:
            m.close()


def test_epoch_rebase_inside_a_run_of_sweeps(pkg):
    P = _P(pkg)
    limit = (1 << 28) - 2
    a = _random_sweeps(P, 10, seed=21, lo=-2.0, hi=2.0)
    b = _random_sweeps(P, 5, seed=22, lo=-2.0, hi=2.0)
    pk = P.pack_packets([1, 2] * 20, np.linspace(-2, 2, 40), np.linspace(2, -2, 40), np.linspace(0, 6, 40), np.arange(40),
                        np.zeros(40), np.full((40, 4), 0.8), np.zeros(40))
    o = orc.OracleMapper(200, 0.05, -5.0, -5.0)
    o.update_rays(*_beams(_records(P, a)))
    o.update_rays(*_beams(_records(P, b)))
    o.feed_stream(pk)
    for mode in (1, 2):
        with pkg.QuasarMapper(200, 0.05, -5.0, -5.0, raycast_mode=mode) as m:
            m.ingest_sweeps(a, seq0=limit - 46 * 10)
            assert m.counters()["rebases"] == 0
            m.ingest_sweeps(b)                                  # crosses the epoch: rebase first
            assert m.counters()["rebases"] == 1
            m.ingest_array(pk)
            _same_map(m, o, f"mode {mode}")


def test_reset_clears_sweeps(pkg):
    P = _P(pkg)
    sw = _random_sweeps(P, 64, seed=5, lo=-4.0, hi=4.0)
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as fresh:
        fresh.ingest_sweeps(sw)
        want = (fresh.grid_i8(), *fresh.counts())
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        m.ingest_sweeps(_random_sweeps(P, 64, seed=6, lo=-4.0, hi=4.0), seq0=1000)
        m.reset()
        assert (m.grid_i8() == -1).all() and all((c == 0).all() for c in m.counts())
        assert m.counters()["rays"] == 0
        with pytest.raises(pkg.QuasarError):
            m.last_sweeps()
        m.ingest_sweeps(sw)
        got = (m.grid_i8(), *m.counts())
        assert all((x == y).all() for x, y in zip(got, want))


def test_sweep_filter(pkg):
    P = _P(pkg)
    sw = _random_sweeps(P, 200, seed=8, lo=-3.0, hi=3.0)
    o = orc.OracleMapper(200, 0.05, -5.0, -5.0)
    o.update_rays(*_beams(_records(P, sw), smin=0.3, smax=1.0))
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        m.set_sweep_filter(0.3, 1.0)
        m.ingest_sweeps(sw)
        _same_map(m, o, "filter 0.3 .. 1.0")
        with pytest.raises(pkg.QuasarError):
            m.set_sweep_filter(1.0, 0.5)


def test_sharded_contexts_refuse_sweeps(pkg):
    P = _P(pkg)
    sw = _random_sweeps(P, 2, seed=1)
    for kw in (dict(seq_stride=2), dict(shard_bots=1, shard_rank=0)):
        with pkg.QuasarMapper(200, 0.05, -5.0, -5.0, **kw) as m:
            with pytest.raises(pkg.QuasarError):
                m.ingest_sweeps(sw)
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        with pytest.raises(pkg.QuasarError):
            m.ingest_sweeps(np.zeros((2, 742), np.uint8))
