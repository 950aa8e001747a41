"""GPU parity proper: the HIP path (through the C ABI) against
  (a) the fixtures the reference itself produced (tests/golden), and
  (b) the CPU oracle on the same inputs.
Bar: integer/byte/index results bit-exact; float pose / drift / correction / zone values within
1e-5 (north_star); here they are in fact expected to agree to ~1e-12."""
import hashlib
import importlib
import os
import struct

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import GOLDEN, ROOT, load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("radius,min_between,corr", [(0.6, 1, 0.5), (0.3, 5, 0.25), (1.0, 64, 0.5), (0.6, 0, 1.0), (0.45, 31, 0.1)])
def test_closure_constants_other_than_the_reference(pkg, radius, min_between, corr):
    """CLOSURE_RADIUS / MIN_POSES_BETWEEN / CLOSURE_CORRECTION (:99-101) are module constants in the reference and
    fields of qs_config here: windows of 1 node, windows capped at 32 nodes below MIN_POSES_BETWEEN = 64, no
    cool-down at all -- same closures, landmarks, drift and grid as the reference's loop with those constants."""
    g = load("session_512")
    stream = np.tile(g["datagrams"][:, :42], (12, 1))
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0)
    o.set_closure_params(radius, min_between, corr)
    o.feed_stream(stream)
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8, closure_radius=radius, min_poses_between=min_between,
                          closure_correction=corr) as m:
        m.ingest_array(stream[:5000]); m.ingest_array(stream[5000:])
        idx, cc = m.closures(0); oi, oc = o.closures(0)
        assert len(oi) > 50 and (idx == oi).all() and np.abs(cc - oc).max() < FLOAT_TOL
        xy, ti = m.landmarks(0); oxy, oti = o.landmarks(0)
        assert (ti == oti).all() and np.abs(xy - oxy).max() < FLOAT_TOL
        for b in (1, 2):
            assert np.abs(m.drift(b) - o.drift(b)).max() < FLOAT_TOL
        assert (m.grid_i8() == o.grid).all()


SCENARIOS = ["session_200", "session_512", "session_4096", "session_sep_512", "laps5_512",
             "session_fine_1024", "mixed_200", "adversarial_512", "adversarial_dense_200"]
FLOAT_TOL = 1e-5


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def make_mapper(pkg, g, **kw):
    size, res, ox, oy, sep = g["cfg"]
    return pkg.QuasarMapper(int(size), res, ox, oy, separation=sep, **kw)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario_vs_reference_golden(pkg, name, mode):
    g = load(name)
    with make_mapper(pkg, g, raycast_mode=mode) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        acc, pose = m.last_batch()
        assert (acc == g["accepted"]).all()
        grid = m.grid_i8()
        assert hashlib.sha256(grid.tobytes()).digest() == g["grid_sha256"].tobytes(), \
            f"cells differing: {(grid[g['grid_known_yx'][:, 0], g['grid_known_yx'][:, 1]] != g['grid_known_val']).sum()}"
        assert [(grid == 0).sum(), (grid == 100).sum(), (grid == -1).sum()] == g["grid_counts"].tolist()
        np.testing.assert_allclose(pose[acc == 1], g["pose_xyyaw"], rtol=0, atol=FLOAT_TOL)
        n_nodes, n_lms, n_cls = m.slam_sizes(0)
        assert n_nodes == int(g["n_nodes"][0])
        idx, corr = m.closures(0)
        assert (idx == g["closures_idx"]).all()
        np.testing.assert_allclose(corr, g["closures_corr"], rtol=0, atol=FLOAT_TOL)
        xy, ti = m.landmarks(0)
        assert (ti == g["landmarks_type_idx"]).all()
        np.testing.assert_allclose(xy, g["landmarks_xy"], rtol=0, atol=FLOAT_TOL)
        for b in (1, 2):
            np.testing.assert_allclose(m.drift(b), g["drift"][b - 1], rtol=0, atol=FLOAT_TOL)
            z = m.zone(b)
            if np.isnan(g[f"zone_bot{b}"]).any():
                assert z is None
            else:
                np.testing.assert_allclose(z, g[f"zone_bot{b}"], rtol=0, atol=FLOAT_TOL)
            # the ZONE datagram is f32 on the wire: allow 1 ulp of f32 on each field
            got = np.frombuffer(m.zone_packet(b), dtype=np.uint8)
            want = g[f"zone_bytes_bot{b}"]
            assert got[:4].tobytes() == b"ZONE"
            gf, wf = got[4:].view("<f4"), want[4:].view("<f4")
            assert np.all(np.abs(gf - wf) <= np.spacing(np.abs(wf)).astype(np.float32))
        hxy, hvalid = m.last_hits()
        agents = g["datagrams"][:, 4]
        for b in (1, 2):
            for s, k in enumerate(("front", "left", "back", "right")):
                sel = (acc == 1) & (agents == b) & (hvalid[:, s] == 1)
                np.testing.assert_allclose(hxy[sel, s, :], g[f"hits_bot{b}_{k}"], rtol=0, atol=FLOAT_TOL)


@pytest.mark.parametrize("mode", [1, 2])
def test_session_exact_float_agreement_with_oracle(pkg, mode):
    """Same inputs through the oracle: counters, hit/miss counts, log-odds, poses."""
    g = load("session_512")
    size, res, ox, oy, sep = g["cfg"]
    o = orc.OracleMapper(int(size), res, ox, oy, sep)
    o.feed_stream(g["datagrams"], g["lengths"])
    with make_mapper(pkg, g, raycast_mode=mode) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        hits, misses = m.counts()
        assert (hits == o.hits).all() and (misses == o.misses).all()
        np.testing.assert_allclose(m.logodds(), o.logodds(), rtol=0, atol=1e-6)
        c = m.counters()
        assert c["datagrams"] == 687 and c["accepted"] == 687 and c["rays"] == 2748
        assert c["cells"] == o.n_cells_written and c["hits"] == 1041 and c["closures"] == 10
        assert c["landmarks"] == 132
        assert m.zone_packet(1).hex() == "5a4f4e4561328dbfb615cfbf957370401ceb2240"
        assert m.zone_packet(1, online=False) == struct.pack("<4sffff", b"ZONE", 999.0, 999.0, -999.0, -999.0)


@pytest.mark.parametrize("mode", [1, 2])
def test_batch_splitting_is_invisible(pkg, mode):
    """Feeding the stream in ragged batches (1, 2, 29, 30, 31, 64, ...) gives the same state as one call."""
    g = load("laps5_512")
    with make_mapper(pkg, g, raycast_mode=mode) as m:
        sizes = [1, 2, 29, 30, 31, 64, 255, 256, 257, 1000, 3, 1]
        pos, k = 0, 0
        n = len(g["datagrams"])
        poses = []
        while pos < n:
            step = sizes[k % len(sizes)]; k += 1
            m.ingest_array(g["datagrams"][pos:pos + step], g["lengths"][pos:pos + step])
            poses.append(m.last_batch()[1])
            pos += step
        grid = m.grid_i8()
        assert hashlib.sha256(grid.tobytes()).digest() == g["grid_sha256"].tobytes()
        idx, corr = m.closures(0)
        assert (idx == g["closures_idx"]).all()
        np.testing.assert_allclose(np.concatenate(poses), g["pose_xyyaw"], rtol=0, atol=FLOAT_TOL)
        m.ingest_array(np.zeros((0, 42), dtype=np.uint8))       # empty batch is a no-op
        assert hashlib.sha256(m.grid_i8().tobytes()).digest() == g["grid_sha256"].tobytes()


def test_update_ray_object_api(pkg):
    t = load("update_ray_cases")
    size, res, ox, oy = t["cfg"]
    rays = t["rays"]
    with pkg.QuasarMapper(int(size), res, ox, oy) as m:
        # every single-ray case on a fresh grid
        for i in range(0, len(rays), 7):
            m.reset()
            rx, ry, hx, hy, v = rays[i]
            m.occ_grid.update_ray(rx, ry, hx, hy, bool(v))
            assert (m.occ_grid.grid == t["grids"][i]).all(), i
        m.reset()
        m.update_rays(rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 3], rays[:, 4].astype(np.uint8))
        assert (m.grid_i8() == t["grid_sequential"]).all()


def test_world_to_grid_device(pkg):
    import json
    kat = json.load(open(os.path.join(GOLDEN, "kat.json")))
    for key, cfg in (("world_to_grid_200", (200, 0.05, -5.0, -5.0)),
                     ("world_to_grid_4096", (4096, 0.05, -102.4, -102.4))):
        with pkg.QuasarMapper(*cfg) as m:
            w = np.array([p[0] for p in kat[key]])
            want = np.array([p[1] for p in kat[key]])
            assert (m.world_to_grid(w, 0) == want).all()
            assert [m.occ_grid.world_to_grid(x, x)[0] for x in w] == want.tolist()


def test_reset_starts_a_new_session(pkg):
    g = load("session_200")
    with make_mapper(pkg, g) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        m.reset()
        assert (m.grid_i8() == -1).all() and m.slam_sizes(0) == (0, 0, 0) and m.zone(1) is None
        m.ingest_array(g["datagrams"], g["lengths"])
        assert hashlib.sha256(m.grid_i8().tobytes()).digest() == g["grid_sha256"].tobytes()
        assert (m.closures(0)[0] == g["closures_idx"]).all()


def _oracle_ekf_over_stream(g, metres_per_tick=0.0107):
    """The build-defined EKF wiring (oracle.c:qso_ekf_packet) over a golden datagram stream."""
    import struct as _st
    ek = orc.OracleEKF(3)
    sep = g["cfg"][4]
    for i, (d, n) in enumerate(zip(g["datagrams"], g["lengths"])):
        if not g["accepted"][i]:
            continue
        f = _st.unpack("<4sBfffiIffff", d[:41].tobytes())
        agent, x, y, yaw, enc = f[1], f[2], f[3], f[4], f[5]
        px = float(np.float32(x)) + (sep if agent == 2 else 0.0)
        ek.packet(agent, float(g["recv_time"][i]), px, float(np.float32(y)), float(np.float32(yaw)), float(enc),
                  metres_per_tick)
    return ek


def test_ekf_ingest_matches_oracle(pkg):
    """EKF (A7): the HIP filter against the build's CPU restatement of ekf.cpp (itself bit-equal to the firmware's
    own ekf.cpp on tests/golden/ekf_ref.npz: tests/test_ekf_reference_cpu.py; the kernels against that file:
    tests/test_gpu_ekf_reference.py), tolerance 1e-5 (north_star), expected ~1e-12."""
    g = load("session_512")
    ek = _oracle_ekf_over_stream(g)
    with make_mapper(pkg, g, enable_ekf=True) as m:
        m.ingest_array(g["datagrams"], g["lengths"], recv_time=g["recv_time"])
        for b in (1, 2):
            x, P = m.ekf_state(b)
            np.testing.assert_allclose(x, ek.state(b), rtol=0, atol=1e-5)
            np.testing.assert_allclose(P, ek.cov(b), rtol=0, atol=1e-5)
            assert np.abs(x - ek.state(b)).max() < 1e-9 and np.abs(P - ek.cov(b)).max() < 1e-9
    # ragged batches give the same filter state
    with make_mapper(pkg, g, enable_ekf=True) as m:
        for lo in range(0, 687, 100):
            m.ingest_array(g["datagrams"][lo:lo + 100], g["lengths"][lo:lo + 100], recv_time=g["recv_time"][lo:lo + 100])
        for b in (1, 2):
            x, P = m.ekf_state(b)
            assert np.abs(x - ek.state(b)).max() < 1e-9 and np.abs(P - ek.cov(b)).max() < 1e-9


def _ekf_close(m, o, bots, rtol=1e-9):
    for b in bots:
        x, P = m.ekf_state(b)
        xo, Po = o.ekf_state(b)
        assert np.abs(x - xo).max() <= rtol * max(1.0, np.abs(xo).max()), (b, x, xo)
        assert np.abs(P - Po).max() <= rtol * max(1.0, np.abs(Po).max()), b


@pytest.mark.gpu
def test_ekf_parallel_in_time_long_streams(pkg):
    """csrc/ekf_scan.hip (batches >= 4096 packets): chunked, parallel-in-time form of the filter against the
    sequential CPU restatement over many chunks, several batches (state carried in between, including a
    switch between the serial small-batch kernel and the scan), nominal and irregular time stamps (zero and
    negative steps skip the predict, ekf.cpp:28-29).  Agreement is to rounding, not bit for bit: 1e-9
    relative here, north_star's bar is 1e-5."""
    replay = importlib.import_module(pkg.__name__ + ".replay")
    session, _ = replay.telemetry_csv_to_packets()
    n = 150_000
    stream = replay.cycle_stream(session, n)
    cfg = dict(size=512, resolution=0.05, origin_x=-12.8, origin_y=-12.8, separation=5.0)
    rng = np.random.default_rng(11)
    irregular = np.cumsum(rng.choice([0.05, 0.02, 0.0, -0.01, 0.3], size=n, p=[.7, .1, .08, .04, .08])) + 100.0
    for times in (None, irregular):
        o = orc.OracleMapper(512, 0.05, -12.8, -12.8, separation=5.0)
        o.enable_ekf(0.0107)
        o.feed_stream(stream, None, times)
        # one batch
        with pkg.QuasarMapper(**cfg, enable_ekf=True) as m:
            m.ingest_array(stream, recv_time=times)
            _ekf_close(m, o, (1, 2))
            assert m.counters()["ekf_wrap_clamp"] == 0
        # ragged batches: scan, serial (< 4096), scan, ...
        with pkg.QuasarMapper(**cfg, enable_ekf=True) as m:
            lo = 0
            for size in (5000, 100, 70_000, 3, 4096, 1, 60_000, n):
                hi = min(lo + size, n)
                m.ingest_array(stream[lo:hi], recv_time=None if times is None else times[lo:hi])
                lo = hi
                if lo == n:
                    break
            _ekf_close(m, o, (1, 2))


@pytest.mark.gpu
def test_ekf_parallel_in_time_many_bots(pkg):
    """64 bots (1 to 3 chunks each, ragged) through the scan form against the sequential restatement."""
    replay = importlib.import_module(pkg.__name__ + ".replay")
    session, _ = replay.telemetry_csv_to_packets()
    n = 100_000
    stream = replay.multi_bot_stream(session, 64, n)
    o = orc.OracleMapper(4096, 0.05, -102.4, -102.4, separation=0.0, max_agent=64, bots_per_graph=2)
    o.enable_ekf(0.0107)
    o.feed_stream(stream)
    with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2, enable_ekf=True) as m:
        m.ingest_array(stream)
        _ekf_close(m, o, range(1, 65))


def test_ekf_object_api_hand_derived(pkg):
    """Hand-derived KATs: one predict from x=0, P=I, dt=0.1, omega_m=0.5 gives
    theta=0.05 and P grown by Q on the diagonal (+ dt^2 coupling); one update with z=[1,0]."""
    with pkg.QuasarMapper(max_agent=4) as m:
        for b in (1, 2, 3, 4):
            m.ekf_init(b, 10.0, np.zeros(6))
        m.ekf_step([1, 3], [0.5, 0.5], [10.1, 10.1])                       # predict only
        ek = orc.OracleEKF(5)
        for b in (1, 3):
            ek.init(b, 10.0, np.zeros(6)); ek.predict(b, 0.5, 10.1)
            x, P = m.ekf_state(b)
            assert abs(x[2] - 0.05) < 1e-15 and x[4] == 0.5 and x[0] == 0 and x[1] == 0
            np.testing.assert_allclose(x, ek.state(b), rtol=0, atol=1e-12)
            np.testing.assert_allclose(P, ek.cov(b), rtol=0, atol=1e-12)
            assert abs(P[0, 0] - (1.0 + 0.1 * 0.1 + 0.01)) < 1e-12      # P00 + (cos*dt)^2*P33 + Q00
        x2, P2 = m.ekf_state(2)
        assert (x2 == 0).all() and (P2 == np.eye(6)).all()                  # untouched bot
        m.ekf_step([1], [0.5], [10.2], z_v=[1.0], z_omega=[0.0])           # predict + update
        ek.predict(1, 0.5, 10.2); ek.update(1, 1.0, 0.0)
        x, P = m.ekf_state(1)
        np.testing.assert_allclose(x, ek.state(1), rtol=0, atol=1e-12)
        np.testing.assert_allclose(P, ek.cov(1), rtol=0, atol=1e-12)
        assert 0 < x[3] < 1.0                                               # pulled toward z_v = 1


def _alternating_stream(g):
    """Strictly alternating bot-1 / bot-2 packets from the golden session (330 each)."""
    pk = g["datagrams"][:, :42]
    b1, b2 = pk[pk[:, 4] == 1][:330], pk[pk[:, 4] == 2][:330]
    inter = np.empty((660, 42), dtype=np.uint8)
    inter[0::2], inter[1::2] = b1, b2
    return inter, b1, b2


def test_fuse_of_sharded_contexts_equals_one_mapper(pkg):
    """K3 grid fuse (shared-grid semantics, dual_bot_mapper.py:785): two contexts each ingest one bot's
    packets with GLOBAL arrival indices (seq0 = rank, stride 2); fusing them (latest stamp wins,
    counts add) must equal one mapper (two independent pose graphs) fed the interleaved stream."""
    g = load("session_512")
    inter, b1, b2 = _alternating_stream(g)
    b2_as_1 = b2.copy(); b2_as_1[:, 4] = 1
    kw = dict(size=512, resolution=0.05, origin_x=-12.8, origin_y=-12.8)
    with pkg.QuasarMapper(max_agent=2, bots_per_graph=1, **kw) as ref, \
         pkg.QuasarMapper(max_agent=1, seq_stride=2, **kw) as a, \
         pkg.QuasarMapper(max_agent=1, seq_stride=2, **kw) as b:
        ref.ingest_array(inter)
        a.ingest_array(b1, seq0=0)
        b.ingest_array(b2_as_1, seq0=1)
        assert not (a.grid_i8() == ref.grid_i8()).all()          # a shard alone is not the map
        a.fuse([b])
        assert (a.grid_i8() == ref.grid_i8()).all()
        ha, ma = a.counts(); hr, mr = ref.counts()
        assert (ha == hr).all() and (ma == mr).all()
        # and against the CPU oracle on the interleaved stream
        o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0, max_agent=2, bots_per_graph=1)
        o.feed_stream(inter)
        assert (a.grid_i8() == o.grid).all() and (ha == o.hits).all()
        for gr in (0, 1):
            assert (ref.closures(gr)[0] == o.closures(gr)[0]).all()


def test_stamp_epoch_rebase_keeps_order(pkg):
    """Stamps are 30-bit ordinals; crossing 2^28 arrival indices rebases the grid in place.  A later
    batch must still win over everything written before the rebase."""
    g = load("session_200")
    size, res, ox, oy, sep = g["cfg"]
    n = len(g["datagrams"])
    with make_mapper(pkg, g) as m:
        m.ingest_array(g["datagrams"][:400], g["lengths"][:400], seq0=5)
        m.ingest_array(g["datagrams"][400:], g["lengths"][400:], seq0=(1 << 28) + 77)
        assert m.counters()["rebases"] == 1
        assert hashlib.sha256(m.grid_i8().tobytes()).digest() == g["grid_sha256"].tobytes()
        with pytest.raises(pkg.QuasarError):
            m.ingest_array(g["datagrams"][:10], g["lengths"][:10], seq0=3)     # sequence numbers must not go back


def test_map_merger_ops_match_oracle(pkg):
    """A11: MapMerger.grid_to_pcd / publish_global_map restated (map_merger.py:64-127), against the CPU
    restatement and a hand-built 4x4 case.  Pinned against the reference's own methods by
    tests/golden/merger_calls.npz (tests/test_merger_reference_cpu.py, tests/test_gpu_merger_reference.py)."""
    small = np.full((4, 4), -1, dtype=np.int8); small[1, 2] = 100; small[3, 0] = 51; small[0, 0] = 50
    with pkg.QuasarMapper() as m:
        xy = m.grid_to_pcd(small, 0.5, -1.0, 2.0)
        assert xy.tolist() == [[0.0, 2.5], [-1.0, 3.5]]            # (col*res+ox, row*res+oy), row-major
        grid, origin = m.rasterise(xy, 0.5)
        assert origin.tolist() == [-1.0, 2.5] and grid.shape == (3, 3)
        want = np.full((3, 3), -1, dtype=np.int8); want[0, 2] = 100; want[2, 0] = 100
        assert (grid == want).all()
        g = load("session_512")
        big = g["grid"]
        xy = m.grid_to_pcd(big, 0.05, -12.8, -12.8)
        oxy = orc.grid_to_pcd(big, 0.05, -12.8, -12.8)
        assert xy.shape == oxy.shape == (437, 2) and (xy == oxy).all()
        # shift one cloud like a registered local map and merge
        merged = np.concatenate([xy, xy + [0.31, -0.17]])
        grid, origin = m.rasterise(merged, 0.05)
        ogrid, oorigin = orc.rasterise(merged, 0.05)
        assert grid.shape == ogrid.shape and (grid == ogrid).all() and (origin == oorigin).all()
        assert m.rasterise(np.zeros((0, 2)), 0.05) == (None, None)


def _replay(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".replay")


def test_full_size_properties_4096(pkg):
    """BASELINE configs[1] at full grid size (4096^2) and a 2^18-packet stream: properties that do
    not need the (quadratic) oracle over the whole stream -- the two raycast schedules agree bit for
    bit, ragged batching is invisible, counters are consistent -- and the oracle over the whole stream."""
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    B = 1 << 18
    stream = replay.cycle_stream(session, B)
    kw = dict(size=4096, resolution=0.05, origin_x=-102.4, origin_y=-102.4)
    with pkg.QuasarMapper(raycast_mode=2, **kw) as t, pkg.QuasarMapper(raycast_mode=1, **kw) as d:
        t.ingest_array(stream); d.ingest_array(stream)
        gt, gd = t.grid_i8(), d.grid_i8()
        assert (gt == gd).all()
        (ht, mt), (hd, md) = t.counts(), d.counts()
        assert (ht == hd).all() and (mt == md).all()
        c = t.counters()
        assert int(ht.sum()) + int(mt.sum()) == c["cells"] and c["rays"] == 4 * B and c["accepted"] == B
        assert ((ht + mt > 0) == (gt != -1)).all()
        assert t.slam_sizes(0) == d.slam_sizes(0)
        assert (t.closures(0)[0] == d.closures(0)[0]).all()
        # ragged batches
        t.reset()
        pos = 0
        for step in (1, 70000, 33, 100000, 4096, B):
            t.ingest_array(stream[pos:pos + step]); pos += step
            if pos >= B:
                break
        assert (t.grid_i8() == gt).all() and (t.counts()[0] == ht).all()
        assert (t.closures(0)[0] == d.closures(0)[0]).all()
    # the oracle over the whole 2^18-packet stream (~1 s in C)
    n = B
    o = orc.OracleMapper(4096, 0.05, -102.4, -102.4, 0.0)
    o.feed_stream(stream[:n])
    with pkg.QuasarMapper(**kw) as m:
        m.ingest_array(stream[:n])
        assert (m.grid_i8() == o.grid).all()
        h, mi = m.counts()
        assert (h == o.hits).all() and (mi == o.misses).all()
        idx, corr = m.closures(0); oi, oc = o.closures(0)
        assert (idx == oi).all() and np.abs(corr - oc).max() < FLOAT_TOL
        for b in (1, 2):
            assert np.abs(m.drift(b) - o.drift(b)).max() < FLOAT_TOL
            assert np.abs(np.array(m.zone(b)) - o.zone(b)).max() < FLOAT_TOL


def test_64_bots_32_graphs_vs_oracle(pkg):
    """BASELINE configs[2] shape: 64 bots on one GPU, one pose graph per 2 bots (the reference's
    deployment unit), 4096^2 grid."""
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    n = 64 * 700
    stream = replay.multi_bot_stream(session, 64, n)
    o = orc.OracleMapper(4096, 0.05, -102.4, -102.4, 0.0, max_agent=64, bots_per_graph=2)
    assert o.feed_stream(stream) == n
    with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2) as m:
        m.ingest_array(stream[:20000]); m.ingest_array(stream[20000:])
        assert (m.grid_i8() == o.grid).all()
        h, mi = m.counts()
        assert (h == o.hits).all() and (mi == o.misses).all()
        total = 0
        for gr in range(32):
            idx, corr = m.closures(gr); oi, oc = o.closures(gr)
            assert (idx == oi).all(), gr
            if len(oi):
                assert np.abs(corr - oc).max() < FLOAT_TOL
            total += len(oi)
            assert m.slam_sizes(gr)[0] == o.n_nodes(gr)
        assert total > 100
        for b in range(1, 65):
            assert np.abs(m.drift(b) - o.drift(b)).max() < FLOAT_TOL
            assert np.abs(np.array(m.zone(b)) - o.zone(b)).max() < FLOAT_TOL
    # all 64 bots in ONE pose graph (the reference's own semantics, cross-bot matches allowed)
    o1 = orc.OracleMapper(4096, 0.05, -102.4, -102.4, 0.0, max_agent=64)
    o1.feed_stream(stream[:16000])
    with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64) as m:
        m.ingest_array(stream[:16000])
        assert (m.grid_i8() == o1.grid).all()
        assert (m.closures(0)[0] == o1.closures(0)[0]).all()


@pytest.mark.parametrize("bpg", [1, 0, 20])
def test_255_bots_graph_partitions(pkg, bpg):
    """The protocol's maximum of 255 agents: one pose graph each (255 workgroups, 255 bucket indexes allocated
    at their first packet), all in one graph (13 owner waves with up to 20 agents each), 13 graphs of 20."""
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    n = 255 * 500
    stream = replay.multi_bot_stream(session, 255, n)
    o = orc.OracleMapper(4096, 0.05, -102.4, -102.4, 0.0, max_agent=255, bots_per_graph=bpg)
    assert o.feed_stream(stream) == n
    with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=255, bots_per_graph=bpg) as m:
        m.ingest_array(stream[:30000]); m.ingest_array(stream[30000:])
        assert (m.grid_i8() == o.grid).all()
        total = 0
        for gr in range(o.n_graphs):
            idx, corr = m.closures(gr); oi, oc = o.closures(gr)
            assert idx.shape == oi.shape and (idx == oi).all(), gr
            if len(oi):
                assert np.abs(corr - oc).max() < FLOAT_TOL
            total += len(oi)
        assert total > (500 if bpg == 1 else 10000)
        for b in range(1, 256):
            assert np.abs(m.drift(b) - o.drift(b)).max() < FLOAT_TOL
        m.reset(); m.ingest_array(stream)                       # the index of every graph emptied and refilled
        assert (m.grid_i8() == o.grid).all()
        for gr in range(o.n_graphs):
            assert (m.closures(gr)[0] == o.closures(gr)[0]).all()


def test_device_buffer_aliasing_and_nccl_allreduce_single_rank(pkg):
    """The N>1 plumbing on one GPU: torch aliases the library's stamp / counter buffers through
    __cuda_array_interface__, and the RCCL all-reduce (world_size 1) runs on them in place."""
    import importlib
    import torch
    import torch.distributed as dist
    distmod = importlib.import_module(pkg.__name__ + ".dist")
    g = load("session_512")
    dev = torch.device("cuda", 0)
    with make_mapper(pkg, g) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        stamps, counts = distmod.grid_tensors(m, dev)
        assert stamps.dtype == torch.int32 and tuple(stamps.shape) == (512, 512) and tuple(counts.shape) == (512, 512, 2)
        tri = distmod.tri_state_from_stamps(stamps.cpu().numpy())
        assert (tri == m.grid_i8()).all()
        hits, misses = m.counts()
        assert (counts[..., 1].cpu().numpy() == hits).all() and (counts[..., 0].cpu().numpy() == misses).all()
        assert int(stamps.max()) < 2 ** 31 and int(stamps.min()) >= 0
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29577")
        dist.init_process_group("nccl", rank=0, world_size=1)
        try:
            distmod.allreduce_grids(m, dev)
            torch.cuda.synchronize()
        finally:
            dist.destroy_process_group()
        assert hashlib.sha256(m.grid_i8().tobytes()).digest() == g["grid_sha256"].tobytes()
        assert (m.counts()[0] == hits).all()


@pytest.mark.parametrize("name", ["session_200", "session_512", "laps5_512", "adversarial_dense_200", "mixed_200"])
def test_frontiers_vs_reference_golden(pkg, name):
    """N1: get_frontiers / cluster_frontiers / cluster_centroid_world on the device grid
    (dual_bot_mapper.py:181-237) against what the reference itself computed on its own grid."""
    fr = load("frontiers")
    g = load(name)
    with make_mapper(pkg, g) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        cells = m.frontier_cells()
        assert (cells == fr[name + "_cells"]).all()
        st = m.frontier_clusters()
        assert (st[:, 0] == fr[name + "_sizes"]).all()
        assert (st[:, 1:3] == fr[name + "_first"]).all()
        assert (st[:, 3:5] == fr[name + "_sums"]).all()
        cents = np.array(m.frontier_centroids()).reshape(-1, 2)
        assert (cents == fr[name + "_centroids"]).all()
        assert m.occ_grid.get_frontiers()[:3] == [tuple(c) for c in fr[name + "_cells"][:3].tolist()]
        # all clusters (min size 1) partition the frontier cells
        assert int(m.frontier_clusters(min_cluster=1)[:, 0].sum()) == len(cells)


def test_frontiers_full_size_vs_oracle(pkg):
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    stream = replay.multi_bot_stream(session, 64, 64 * 400)
    with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=64, bots_per_graph=2) as m:
        m.ingest_array(stream)
        grid = m.grid_i8()
        cells = m.frontier_cells()
        ocells = orc.frontier_cells(grid)
        assert len(cells) > 5000 and (cells == ocells).all()
        assert (m.frontier_clusters() == orc.frontier_clusters(ocells, 4096)).all()


def test_udp_frontend_end_to_end(pkg):
    """N2: the session's datagrams sent over real UDP to the front-end, ingested in whatever
    batches the polls happen to form; the map must equal the reference's."""
    import importlib, socket, time
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    g = load("mixed_200")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
    srv.bind(("127.0.0.1", 0))
    port = srv.getsockname()[1]
    with make_mapper(pkg, g) as m:
        mc = fe.MissionControl(m, sock=srv)
        tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        sent = 0
        for d, n in zip(g["datagrams"], g["lengths"]):
            if n == 0:
                continue                      # an empty datagram is legal UDP but carries nothing to test
            tx.sendto(d[:n].tobytes(), ("127.0.0.1", port)); sent += 1
            if sent % 64 == 0:
                time.sleep(0.002); mc.poll()
        time.sleep(0.05)
        while mc.poll():
            pass
        assert mc.datagrams == sent
        assert hashlib.sha256(m.grid_i8().tobytes()).digest() == g["grid_sha256"].tobytes()
        assert (m.closures(0)[0] == g["closures_idx"]).all()
        assert mc.pkt_counts[1] + mc.pkt_counts[2] == int(g["accepted"].sum())
        pk = mc.zone_tick(force=True)
        assert pk[1] == g["zone_bytes_bot2"].tobytes() or np.allclose(
            np.frombuffer(pk[1][4:], "<f4"), g["zone_bytes_bot2"][4:].view("<f4"), atol=1e-5)
        tx.close(); mc.close()


def test_long_session_capacity_growth(pkg):
    """30 laps of the session (20.6 k packets) fed in uneven batches WITHOUT resets: the landmark log,
    node pool, closure list and batch buffers all have to grow while the state is preserved."""
    g = load("session_512")
    pk = g["datagrams"][:, :42]
    stream = np.tile(pk, (30, 1))
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0)
    o.feed_stream(stream)
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8) as m:
        pos, k = 0, 0
        sizes = [5, 700, 1500, 64, 3000, 1, 9000, 20000]
        while pos < len(stream):
            m.ingest_array(stream[pos:pos + sizes[k % len(sizes)]]); pos += sizes[k % len(sizes)]; k += 1
        assert (m.grid_i8() == o.grid).all()
        idx, corr = m.closures(0); oi, oc = o.closures(0)
        assert len(oi) > 400 and (idx == oi).all() and np.abs(corr - oc).max() < FLOAT_TOL
        xy, ti = m.landmarks(0); oxy, oti = o.landmarks(0)
        assert len(oti) > 3500 and (ti == oti).all() and np.abs(xy - oxy).max() < FLOAT_TOL
        for b in (1, 2):
            assert np.abs(m.drift(b) - o.drift(b)).max() < FLOAT_TOL
        h, mi = m.counts()
        assert (h == o.hits).all() and (mi == o.misses).all()
        assert m.slam_sizes(0)[0] == len(stream)


def test_api_edge_cases_and_errors(pkg):
    with pytest.raises(pkg.QuasarError):
        pkg.QuasarMapper(size=201)                              # size must be a multiple of 4
    with pytest.raises(pkg.QuasarError):
        pkg.QuasarMapper(max_agent=0)
    with pkg.QuasarMapper(max_agent=3) as m:
        assert m.ingest([]) == 0
        m.ingest([b"", b"x", b"QSRL"])                           # nothing decodable: all dropped, nothing written
        acc, pose = m.last_batch()
        assert acc.tolist() == [0, 0, 0] and np.isnan(pose).all()
        assert (m.grid_i8() == -1).all() and m.counters()["accepted"] == 0 and m.zone(1) is None
        with pytest.raises(pkg.QuasarError):
            m.drift(4)
        with pytest.raises(pkg.QuasarError):
            m.zone(0)
        with pytest.raises(pkg.QuasarError):
            m.closures(1)                                       # only graph 0 exists
        P = pkg.protocol
        one = P.pack_packet(3, 0.0, 0.0, 0.0, 0, 0, 0.5, 0.0, float("nan"), 3.0, 7)   # agent 3, odd landmark type 7
        m.ingest([one])
        acc, pose = m.last_batch()
        assert acc.tolist() == [1] and pose[0].tolist() == [0.0, 0.0, 0.0]
        o = orc.OracleMapper(max_agent=3); o.feed(one)
        assert (m.grid_i8() == o.grid).all() and m.counters()["rays"] == 4 and m.counters()["hits"] == 1
        xy, ti = m.landmarks(0)
        assert ti.tolist() == [[7, 0]]                          # type > 5 lives in the side list, still logged
        bad = P.pack_packet(1, float("inf"), 0.0, 0.0, 0, 0, 0.5, 0.5, 0.5, 0.5, 0)
        m.ingest([bad])
        assert m.last_batch()[0].tolist() == [0]                # non-finite pose: dropped (CPython would raise)
    # landmark types above 5 and poses outside the bucket grid still close loops (side list)
    P = pkg.protocol
    # (long enough that the side list in HBM is consulted, not only the LDS ring of recent landmarks)
    pk = [P.pack_packet(1, 50.0 + 0.01 * (i % 3), 0.0, 0.0, i, 0, 0.0, 0.0, 0.0, 0.0, 9 if i % 10 == 0 else 0) for i in range(6000)]
    with pkg.QuasarMapper() as m:                               # 200x200 grid at (-5,-5): x = 50 is far outside
        m.ingest(pk)
        o = orc.OracleMapper()
        for d in pk:
            o.feed(d)
        assert len(o.closures(0)[0]) > 0 and (m.closures(0)[0] == o.closures(0)[0]).all()
        assert m.counters()["slam_misc_iters"] > 0 and (m.grid_i8() == -1).all()
    # an indexed type far outside the bucket grid: the border buckets take it, no side list
    pk = [P.pack_packet(1 + (i & 1), -80.0 + 0.01 * (i % 3), 60.0, 0.0, i, 0, 0.0, 0.0, 0.0, 0.0, 5 if i % 10 < 2 else 0) for i in range(6000)]
    with pkg.QuasarMapper() as m:
        m.ingest(pk)
        o = orc.OracleMapper()
        for d in pk:
            o.feed(d)
        assert len(o.closures(0)[0]) > 0 and (m.closures(0)[0] == o.closures(0)[0]).all() and (m.closures(0)[1] == o.closures(0)[1]).all()
        assert m.counters()["slam_misc_iters"] == 0


def _rigid(theta, tx, ty):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty], [0, 0, 1.0]])


def test_icp_and_voxel_downsample(pkg):
    """N3 (parity unpinned: Open3D absent): the HIP ICP against the numpy restatement of the same
    published algorithm, and recovery of known rigid transforms on rasterised session maps."""
    g = load("session_512")
    with pkg.QuasarMapper() as m:
        dst = m.grid_to_pcd(g["grid"], 0.05, -12.8, -12.8)                       # 437 occupied cells
        for theta, tx, ty in ((np.radians(3.0), 0.12, -0.08), (np.radians(-5.0), -0.2, 0.15), (0.0, 0.0, 0.0)):
            Tt = _rigid(theta, tx, ty)
            src = dst @ np.linalg.inv(Tt)[:2, :2].T + np.linalg.inv(Tt)[:2, 2]   # so that Tt maps src onto dst
            T, fit, rm, it = m.icp(src, dst, 1.0, 30)
            To, fo, ro, io = orc.icp_planar(src, dst, 1.0, 30)
            assert it == io and abs(fit - fo) < 1e-12 and abs(rm - ro) < 1e-9
            np.testing.assert_allclose(T, To, rtol=0, atol=1e-9)
            assert fit == 1.0 and rm < 2e-2
            np.testing.assert_allclose(T, Tt, rtol=0, atol=3e-2)                  # recovered up to grid ambiguity
            assert abs(np.linalg.det(T[:2, :2]) - 1.0) < 1e-12
        # partial overlap and a far-away cloud (no correspondences -> fitness 0, identity)
        T, fit, rm, it = m.icp(dst[:200] + [0.03, 0.02], dst, 1.0, 30)
        assert fit == 1.0 and rm < 0.05
        T, fit, rm, it = m.icp(dst + [500.0, 0.0], dst, 1.0, 30)
        assert fit == 0.0 and rm == 0.0 and (T == np.eye(3)).all() and it == 1
        # voxel down-sample
        cloud = np.concatenate([dst, dst + [0.011, 0.007], dst[:50] + [0.4, 0.0]])
        v = m.voxel_downsample(cloud, 0.05)
        vo = orc.voxel_downsample(cloud, 0.05)
        assert v.shape == vo.shape and len(v) < len(cloud) and np.abs(v - vo).max() < 1e-12
        assert m.voxel_downsample(np.zeros((0, 2)), 0.05).shape == (0, 2)


def test_map_merger_flow(pkg):
    """MapMerger.map_callback (map_merger.py:35-62) end to end: first map adopted, a shifted copy
    registered and merged, an unrelated map rejected by the fitness gate."""
    import importlib
    merger = importlib.import_module(pkg.__name__ + ".merger")
    g = load("session_512")
    grid = g["grid"]
    with pkg.QuasarMapper() as m:
        mm = merger.MapMerger(m)
        assert mm.map_callback(np.full((8, 8), -1, dtype=np.int8), 0.05, 0.0, 0.0) is None      # empty local map :37
        out, origin = mm.map_callback(grid, 0.05, -12.8, -12.8, agent_id=1)                    # adopted :40-43
        # publish_global_map truncates ((p - min) / res).astype(int) (:109-110): neighbouring cells can
        # collapse, exactly as in the reference; the CPU restatement is the yardstick, not 437
        want, worigin = orc.rasterise(orc.grid_to_pcd(grid, 0.05, -12.8, -12.8), 0.05)
        assert (out == want).all() and (origin == worigin).all() and mm.last_registration is None
        # agent 2 reports the same room in a frame shifted by (+0.10, -0.15): ICP must pull it back
        out2, origin2 = mm.map_callback(grid, 0.05, -12.8 + 0.10, -12.8 - 0.15, agent_id=2)
        T, fit, rm, it = mm.last_registration
        assert fit >= 0.6 and abs(T[0, 2] + 0.10) < 0.03 and abs(T[1, 2] - 0.15) < 0.03
        assert 350 <= (out2 == 100).sum() <= 2 * 437 and 437 <= len(mm.global_xy) <= 2 * 437   # merged + voxel-averaged
        # an unrelated map far away: no correspondences, fitness 0 < 0.6 -> rejected, global unchanged (:54-56)
        before = mm.global_xy.copy()
        far = np.full((64, 64), -1, dtype=np.int8); far[10:20, 10:20] = 100
        assert mm.map_callback(far, 0.05, 300.0, 300.0, agent_id=3) is None
        assert (mm.global_xy == before).all()


def test_grid_8192_configs4(pkg):
    """BASELINE configs[4] grid size: 8192^2 (16384 tiles: 64 KiB LDS histogram in the binning passes).
    64 bots on a 16 m pitch, checked against the oracle."""
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    n = 64 * 300
    stream = replay.multi_bot_stream(session, 64, n, pitch=40.0, tiles_per_row=8, origin=(-190.0, -190.0))
    o = orc.OracleMapper(8192, 0.05, -204.8, -204.8, 0.0, max_agent=64, bots_per_graph=2)
    assert o.feed_stream(stream) == n
    with pkg.QuasarMapper(8192, 0.05, -204.8, -204.8, max_agent=64, bots_per_graph=2) as m:
        m.ingest_array(stream)
        grid = m.grid_i8()
        assert (grid == o.grid).all()
        h, mi = m.counts()
        assert (h == o.hits).all() and (mi == o.misses).all()
        assert int((grid != -1).sum()) > 100000
        for gr in (0, 7, 31):
            assert (m.closures(gr)[0] == o.closures(gr)[0]).all()
        cells = m.frontier_cells()
        assert (cells == orc.frontier_cells(grid)).all()


def test_pose_graph_object_api_add_pose(pkg):
    """PoseGraphSLAM.add_pose driven exactly as main() drives it (:850-857, :908-914): the caller keeps
    drift_correction, applies it, calls add_pose per packet and adds the returned correction.  Must
    reproduce the reference's closures on the golden session, one pose at a time and in batches."""
    g = load("session_512")
    want_idx, want_corr = g["closures_idx"], g["closures_corr"]
    poses, agents = g["pose_xyyaw"], g["pose_agent"]               # reference poses AFTER drift (what add_pose saw)
    lm = g["datagrams"][:, 41]
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8) as m:
        got = []
        for i in range(len(poses)):
            closed, dx, dy = m.slam.add_pose(poses[i, 0], poses[i, 1], poses[i, 2], int(agents[i]), int(lm[i]), 0.0)
            if closed:
                got.append((i, dx, dy))
        assert [k for k, _, _ in got] == want_idx[:, 1].tolist()
        np.testing.assert_allclose(np.array([[a, b] for _, a, b in got]), want_corr, rtol=0, atol=FLOAT_TOL)
        assert (m.closures(0)[0] == want_idx).all() and m.slam.n_nodes == 687
        np.testing.assert_allclose(m.slam.get_correction_for_agent(1), g["drift"][0], rtol=0, atol=FLOAT_TOL)
        assert (m.grid_i8() == -1).all()                              # no rays were cast
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8) as m:              # the same in two batches
        c1, k1 = m.slam_add_poses(poses[:300, 0], poses[:300, 1], agents[:300], lm[:300])
        c2, k2 = m.slam_add_poses(poses[300:, 0], poses[300:, 1], agents[300:], lm[300:])
        closed = np.concatenate([c1, c2]); corr = np.concatenate([k1, k2])
        assert np.nonzero(closed)[0].tolist() == want_idx[:, 1].tolist()
        np.testing.assert_allclose(corr[closed == 1], want_corr, rtol=0, atol=FLOAT_TOL)


@pytest.mark.parametrize("size,res,span", [(4, 0.5, 1.5), (8, 0.05, 0.5), (68, 0.05, 2.5), (132, 0.013, 1.2),
                                           (200, 0.2, 25.0), (1028, 0.05, 30.0)])
@pytest.mark.parametrize("mode", [1, 2])
def test_odd_geometries_adversarial(pkg, size, res, span, mode):
    """Grids that are tiny, not multiples of the 64-cell raster tile, coarse or fine (long rays take the
    direct path inside the tiled pipeline), fed a random stream that pokes every edge: out-of-bounds
    poses, NaN / inf / boundary distances."""
    replay = _replay(pkg)
    origin = -size * res / 2
    stream = replay.adversarial_stream(3000, seed=size * 7 + mode, lo=-span, hi=span)
    rec = stream.view(pkg.protocol.PACKET_DTYPE).reshape(-1)
    rng = np.random.default_rng(size)
    k = rng.integers(0, 3000, 200)
    rec["front"][k[:50]] = np.nan; rec["left"][k[50:100]] = np.inf; rec["back"][k[100:150]] = 0.05; rec["right"][k[150:]] = 1.2
    o = orc.OracleMapper(size, res, origin, origin, 0.0)
    o.feed_stream(stream)
    with pkg.QuasarMapper(size, res, origin, origin, raycast_mode=mode) as m:
        m.ingest_array(stream[:1111]); m.ingest_array(stream[1111:])
        assert (m.grid_i8() == o.grid).all()
        h, mi = m.counts()
        assert (h == o.hits).all() and (mi == o.misses).all()
        assert m.counters()["cells"] == o.n_cells_written
        assert (m.closures(0)[0] == o.closures(0)[0]).all()
        assert (m.frontier_cells() == orc.frontier_cells(o.grid)).all()


@pytest.mark.parametrize("size,res,span", [(68, 0.05, 2.5), (132, 0.013, 1.2)], ids=["short_rays", "long_rays"])
def test_counts_off_equals_counts_on(pkg, size, res, span):
    """enable_counts=False selects the COUNTS = false instantiation of every raycast kernel (and the raster's other way of
    counting written cells).  On two of test_odd_geometries_adversarial's geometries -- short rays on a grid that is no
    multiple of the tile, long rays inside the tiled pipeline -- and its stream, direct and tiled, counts on and off, all
    give the oracle's grid, one stamps array and the same ray / cell / hit / edge-ray counters."""
    from test_gpu_sweeps import _stamps
    replay = _replay(pkg)
    origin = -size * res / 2
    stream = replay.adversarial_stream(3000, seed=size * 7 + 1, lo=-span, hi=span)
    rec = stream.view(pkg.protocol.PACKET_DTYPE).reshape(-1)
    k = np.random.default_rng(size).integers(0, 3000, 200)
    rec["front"][k[:50]] = np.nan; rec["left"][k[50:100]] = np.inf; rec["back"][k[100:150]] = 0.05; rec["right"][k[150:]] = 1.2
    o = orc.OracleMapper(size, res, origin, origin, 0.0)
    o.feed_stream(stream)
    runs = {}
    for mode in (1, 2):
        for counts in (True, False):
            with pkg.QuasarMapper(size, res, origin, origin, raycast_mode=mode, enable_counts=counts) as m:
                m.ingest_array(stream[:1111]); m.ingest_array(stream[1111:])
                assert (m.grid_i8() == o.grid).all(), (mode, counts)
                c = m.counters()
                runs[mode, counts] = (_stamps(pkg, m), {key: c[key] for key in ("rays", "cells", "hits", "edge_rays")})
    first = runs[1, True]
    assert first[1]["cells"] == o.n_cells_written
    for key, (stamps, cnt) in runs.items():
        assert (stamps == first[0]).all(), f"{key}: {(stamps != first[0]).sum()} stamps differ from (1, True)"
        assert cnt == first[1], (key, cnt, first[1])


def test_raster_long_runs_flush_and_tile_changes(pkg):
    """The persistent raster workgroups accumulate consecutive work items of a tile in LDS (16-bit counters:
    forced merge every 31 items) and merge when the tile changes.  With the default 1024 workgroups a run is
    3 items at 1 M packets, so the long-run paths are reached here by asking for 4 workgroups
    (QS_RASTER_WGS is read when the first batch is rastered: own process)."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import importlib, os, sys, hashlib, numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module(%r)
        replay = importlib.import_module(%r + ".replay")
        session, _ = replay.telemetry_csv_to_packets()
        n = 300_000
        for stream, bots, bpg in ((replay.cycle_stream(session, n), 2, 0), (replay.multi_bot_stream(session, 16, n), 16, 2)):
            out = []
            for mode in (1, 2):              # direct (one global atomic per cell) vs tiled
                with pkg.QuasarMapper(4096, 0.05, -102.4, -102.4, max_agent=bots, bots_per_graph=bpg, raycast_mode=mode) as m:
                    m.ingest_array(stream)
                    h, mi = m.counts()
                    out.append((hashlib.sha256(m.grid_i8().tobytes()).hexdigest(), int(h.sum()), int(mi.sum()),
                                hashlib.sha256(h.tobytes()).hexdigest(), hashlib.sha256(mi.tobytes()).hexdigest(), m.counters()["cells"]))
            assert out[0] == out[1], (bots, out)
            assert out[0][1] + out[0][2] == out[0][5]
        print("OK")
    """) % (ROOT, pkg.__name__, pkg.__name__)
    env = dict(os.environ, QS_RASTER_WGS="4")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


# ---- round 2: the N > 1 path emulated on one GPU (two HIP contexts = two ranks) ------------------------------------------
def _exchange_stamps(a, b):
    """What the MAX all-reduce leaves on both ranks, through the K3 kernel on raw device buffers."""
    sa, _, _, _ = a.device_buffers(); sb_, _, _, _ = b.device_buffers()
    a.sync(); b.sync()
    a.fuse_buffers([sb_], None); a.sync()
    b.fuse_buffers([sa], None); b.sync()
    a.mark_fused(); b.mark_fused()


def _sum_counter_snapshots(a, b, cells):
    """What the SUM all-reduce of the counter SNAPSHOTS leaves on both ranks."""
    a.sync(); b.sync()
    fa, _ = a.fused_counts(); fb, _ = b.fused_counts()
    a.sync(); b.sync()
    _, _, ca, _ = a.device_buffers(); _, _, cb, _ = b.device_buffers()
    a.fuse_buffers_range(None, [cb], 0, cells, counts_into_fused=True); a.sync()
    b.fuse_buffers_range(None, [ca], 0, cells, counts_into_fused=True); b.sync()
    a.counts_source(True); b.counts_source(True)


def test_two_contexts_as_two_ranks_across_an_epoch_boundary(pkg):
    """two HIP contexts drive the sharded path as two ranks (seq_stride = 2, seq0 = base + rank),
    three batches with NO reset, the stream crossing the 2^28 stamp-epoch boundary between the second and the third.
    Before the batch that rebases, the ranks exchange their stamps (dist.ShardedMapper does it when qs_epoch_query says
    so; here by hand through qs_fuse_buffers) -- an ingest that would rebase with unfused writes is refused.  After every
    batch the fused grid and the sum of the counter snapshots equal one mapper fed the interleaved stream, and the oracle."""
    g = load("laps5_512")
    pk = g["datagrams"][:, :42]
    b1, b2 = pk[pk[:, 4] == 1], pk[pk[:, 4] == 2]
    n = min(len(b1), len(b2)) // 3 * 3
    b1, b2 = b1[:n], b2[:n].copy()
    inter = np.empty((2 * n, 42), dtype=np.uint8); inter[0::2], inter[1::2] = b1, b2
    b2[:, 4] = 1                                     # on its own rank's wire the bot is agent 1
    kw = dict(size=512, resolution=0.05, origin_x=-12.8, origin_y=-12.8)
    cells = 512 * 512
    third = n // 3
    base = (1 << 28) - 2 - 2 * 2 * third - 40        # batches 1 and 2 fit the first epoch, batch 3 does not
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0, max_agent=2, bots_per_graph=1)
    with pkg.QuasarMapper(max_agent=2, bots_per_graph=1, **kw) as ref, \
         pkg.QuasarMapper(max_agent=1, seq_stride=2, **kw) as a, \
         pkg.QuasarMapper(max_agent=1, seq_stride=2, **kw) as b:
        for k in range(3):
            lo, hi = k * third, (k + 1) * third
            seq = base + 2 * lo
            assert a.epoch_would_rebase(third, seq) == b.epoch_would_rebase(third, seq + 1) == (k == 2)
            if k == 2:
                _exchange_stamps(a, b)                               # (a no-op here: nothing was written since the last one)
            a.ingest_array(b1[lo:hi], seq0=seq)
            b.ingest_array(b2[lo:hi], seq0=seq + 1)
            ref.ingest_array(inter[2 * lo:2 * hi], seq0=seq)
            o.feed_stream(inter[2 * lo:2 * hi])
            _exchange_stamps(a, b)
            _sum_counter_snapshots(a, b, cells)
            ga, gb = a.grid_i8(), b.grid_i8()
            assert (ga == o.grid).all() and (gb == o.grid).all() and (ref.grid_i8() == o.grid).all(), f"batch {k}"
            for m in (a, b):
                h, mi = m.counts()                                    # fused view: global sums, no double counting
                assert (h == o.hits).all() and (mi == o.misses).all(), f"batch {k}"
        assert a.counters()["rebases"] == 1 and b.counters()["rebases"] == 1 and ref.counters()["rebases"] == 1
        for gr, m in ((0, a), (1, b)):
            assert (m.closures(0)[0] == o.closures(gr)[0]).all() and (ref.closures(gr)[0] == o.closures(gr)[0]).all()
        # a shard with writes its peers have not seen must not rebase: the ingest is refused (QS_E_STATE), nothing is lost
        a.ingest_array(b1[:10], seq0=base + 6 * third + 100)
        with pytest.raises(pkg.QuasarError, match="crosses a stamp epoch"):
            a.ingest_array(b1[:10], seq0=(1 << 29) + 1000)
        a.mark_fused()
        a.ingest_array(b1[:10], seq0=(1 << 29) + 1000)
        assert a.counters()["rebases"] == 2
        a.counts_source(False)
        h_local, _ = a.counts()
        assert int(h_local.sum()) < int(o.hits.sum())                 # the local counters still hold rank 0's writes only


def test_replicated_pose_graph_two_contexts(pkg):
    """VERDICT r1 item 8 (replicated mode): ONE pose graph over all bots -- node indices global across
    bots (:275), cross-bot matches allowed (:294-309) -- with the map sharded by agent.  Every rank ingests the whole
    interleaved stream (decode + chain replicated) and casts rays only for its own agent (shard_bots = 1); fused grid,
    closures, drift = one mapper with one pose graph = the oracle = the reference's semantics."""
    g = load("laps5_512")
    inter = g["datagrams"][:, :42]
    kw = dict(size=512, resolution=0.05, origin_x=-12.8, origin_y=-12.8, max_agent=2, bots_per_graph=0)
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0)
    o.feed_stream(inter)
    with pkg.QuasarMapper(shard_bots=1, shard_rank=0, enable_ekf=True, **kw) as a, \
         pkg.QuasarMapper(shard_bots=1, shard_rank=1, enable_ekf=True, **kw) as b:
        half = len(inter) // 2
        for lo, hi in ((0, half), (half, len(inter))):
            a.ingest_array(inter[lo:hi]); b.ingest_array(inter[lo:hi])
        oi, oc = o.closures(0)
        assert len(oi) > 20
        for m in (a, b):                                              # the replicated chain: identical everywhere
            idx, corr = m.closures(0)
            assert (idx == oi).all() and np.abs(corr - oc).max() < FLOAT_TOL
            for bot in (1, 2):
                assert np.abs(m.drift(bot) - o.drift(bot)).max() < FLOAT_TOL
        ga = a.grid_i8()
        assert not (ga == o.grid).all()                               # a shard alone holds only its agent's rays
        _exchange_stamps(a, b)
        _sum_counter_snapshots(a, b, 512 * 512)
        assert (a.grid_i8() == o.grid).all() and (b.grid_i8() == o.grid).all()
        h, mi = a.counts()
        assert (h == o.hits).all() and (mi == o.misses).all()
        # zones and rays belong to the owner only
        assert a.zone(2) is None and b.zone(1) is None
        assert np.abs(np.array(a.zone(1)) - o.zone(1)).max() < FLOAT_TOL and np.abs(np.array(b.zone(2)) - o.zone(2)).max() < FLOAT_TOL
        ca, cb = a.counters(), b.counters()
        assert ca["rays"] + cb["rays"] == o.n_rays and ca["cells"] + cb["cells"] == o.n_cells_written
        acc, _ = a.last_batch()
        assert acc.all()                                              # accepted = part of the pose graph, owned or not


def test_sharded_mapper_wrapper_single_rank_nccl(pkg):
    """dist.ShardedMapper end to end on one GPU (RCCL, world_size 1): ingest -> fuse (both algorithms) -> repeated fuse
    without reset leaves the counters alone (an in-place SUM all-reduce doubled them)."""
    import importlib
    import torch
    import torch.distributed as dist
    distmod = importlib.import_module(pkg.__name__ + ".dist")
    g = load("session_512")
    dev = torch.device("cuda", 0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ["MASTER_PORT"] = "29578"
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        side = torch.cuda.Stream(device=dev)          # (torch's default stream has handle 0 = "own stream" to qs_set_stream)
        torch.cuda.set_stream(side)
        for algo in ("allreduce", "direct"):
            with make_mapper(pkg, g) as m:
                m.set_stream(side.cuda_stream)
                sm = distmod.ShardedMapper(m, dev, 0, 1, fuse=algo)
                d = torch.from_numpy(np.ascontiguousarray(g["datagrams"][:, :42])).to(dev)
                ok = g["lengths"] == 42
                assert ok.all()
                sm.ingest(d[:300], None, seq_base=0)
                distmod.allreduce_grids(m, dev, algo=algo, sync=False)
                sm.ingest(d[300:], None, seq_base=300)
                distmod.allreduce_grids(m, dev, algo=algo, sync=False)
                distmod.allreduce_grids(m, dev, algo=algo, sync=False)
                torch.cuda.synchronize()
                assert hashlib.sha256(m.grid_i8().tobytes()).digest() == g["grid_sha256"].tobytes()
                o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0); o.feed_stream(g["datagrams"], g["lengths"])
                h, mi = m.counts()
                assert (h == o.hits).all() and (mi == o.misses).all()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        dist.destroy_process_group()


def test_fuse_kernel_many_sources_and_ranges(pkg):
    """K3 with 1..70 sources (unrolled groups of 8 + a partial group + a second launch past 64) and on cell ranges,
    against numpy."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    with pkg.QuasarMapper(256, 0.05, -6.4, -6.4) as m:
        cells = 256 * 256
        for G in (1, 7, 8, 9, 33, 64, 70):
            m.reset(); m.sync()
            st = rng.integers(0, 1 << 30, (G, cells)).astype(np.int32)
            ct = rng.integers(0, 1 << 16, (G, cells, 2)).astype(np.int32)
            d_st = torch.from_numpy(st).to(dev); d_ct = torch.from_numpy(ct).to(dev)
            m.fuse_buffers([d_st[k].data_ptr() for k in range(G)], [d_ct[k].data_ptr() for k in range(G)])
            m.sync()
            stamps = st.max(axis=0)
            exp = np.where(stamps == 0, -1, np.where(stamps & 1, 100, 0)).astype(np.int8).reshape(256, 256)
            assert (m.grid_i8() == exp).all(), G
            h, mi = m.counts()
            assert (h.reshape(-1) == ct[:, :, 1].sum(axis=0)).all() and (mi.reshape(-1) == ct[:, :, 0].sum(axis=0)).all(), G
        # a range: only cells [off, off + n) change
        m.reset(); m.sync()
        off, n = 1024, 4096
        src = torch.from_numpy(rng.integers(2, 1 << 20, (3, n)).astype(np.int32)).to(dev)
        m.fuse_buffers_range([src[k].data_ptr() for k in range(3)], None, off, n)
        m.sync()
        gi = m.grid_i8().reshape(-1)
        assert (gi[:off] == -1).all() and (gi[off + n:] == -1).all() and (gi[off:off + n] != -1).all()
        with pytest.raises(pkg.QuasarError):
            m.fuse_buffers_range([src[0].data_ptr()], None, 2, 4)        # ranges are multiples of 4 cells


def test_nn_search_mfma_equals_scalar_equals_numpy(pkg):
    """Row J1 / N3: the correspondence search on the matrix cores (v_mfma_f64_16x16x4_f64 as a screen, fp64 re-evaluation of
    what passes) returns exactly what the scalar fp64 brute force returns -- indices and squared distances bit for bit, ties to
    the lowest target index -- and both equal numpy's argmin over the same expression."""
    rng = np.random.default_rng(3)

    def ref(src, dst, md):
        d2 = (src[:, None, 0] - dst[None, :, 0]) ** 2 + (src[:, None, 1] - dst[None, :, 1]) ** 2
        j = d2.argmin(1)                                  # first minimum = lowest index
        dm = d2[np.arange(len(src)), j]
        ok = dm < md * md
        return np.where(ok, j, -1).astype(np.int32), np.where(ok, dm, 0.0)

    cases = []
    for ns, nd in ((1, 1), (3, 15), (16, 16), (17, 17), (33, 63), (64, 64), (129, 1025), (1000, 777), (2048, 4099)):
        cases.append((f"random {ns}x{nd}", rng.uniform(-50, 50, (ns, 2)), rng.uniform(-50, 50, (nd, 2)), 5.0))
    lat = lambda n, o: rng.integers(0, 200, (n, 2)) * 0.05 + o
    cases.append(("lattice: exact ties", lat(1500, 0.0), lat(1200, 0.0), 1.0))
    cases.append(("lattice far from the origin", lat(900, 1.0e4), lat(1100, 1.0e4), 1.0))
    cases.append(("half-cell offset: four equidistant targets", lat(500, 0.025), np.unique(lat(3000, 0.0), axis=0), 1.0))
    dup = rng.uniform(-1, 1, (300, 2)); cases.append(("duplicated targets", rng.uniform(-1, 1, (400, 2)), np.concatenate([dup, dup, dup]), 0.5))
    cases.append(("nothing in range", rng.uniform(0, 1, (100, 2)), rng.uniform(50, 51, (130, 2)), 1.0))
    bad = rng.uniform(-5, 5, (200, 2)); bad[7] = np.nan; bad[9, 0] = np.inf
    cases.append(("non-finite targets", rng.uniform(-5, 5, (150, 2)), bad, 2.0))
    # sources that are non-finite or far outliers (the screen's margin is per row: one of them among a wave's 64 rows
    # must neither change its neighbours' results nor their speed), and enough of both for several target parts
    sb = rng.uniform(-5, 5, (300, 2)); sb[3] = np.nan; sb[70, 1] = np.inf; sb[130] = (1.0e9, -3.0e8); sb[131] = (-1.0e150, 2.0)
    cases.append(("non-finite and outlier sources", sb, rng.uniform(-5, 5, (900, 2)), 2.0))
    cases.append(("many parts", rng.uniform(-30, 30, (700, 2)), rng.uniform(-30, 30, (40000, 2)), 3.0))
    with pkg.QuasarMapper(64, 0.05, -1.6, -1.6) as m:
        for name, src, dst, md in cases:
            c1, d1, _ = m.nn_search(src, dst, md, 1)
            c2, d2, _ = m.nn_search(src, dst, md, 2)
            assert (c1 == c2).all() and (d1 == d2).all(), name
            if not (np.isfinite(dst).all() and np.isfinite(src).all()):
                continue
            cr, dr = ref(src, dst, md)
            assert (c1 == cr).all() and (d1 == dr).all(), name
        assert m.mfma_f64_rate() > 1.0


@pytest.mark.parametrize("name", ["session_200", "laps5_512", "adversarial_dense_200"])
def test_object_api_the_reference_callers_use(pkg, name):
    """the look-alikes of what main() and MapRenderer touch.
      * occ_grid.cluster_frontiers(cells) / cluster_centroid_world(cluster) (:951-955) against the reference's own clusters;
      * slam.nodes: len() and nodes[node_idx].agent_id, so that get_correction_for_agent's loop (:328-338) works as written;
      * occ_grid.grid read cell by cell as the renderer does (:505-516) costs ONE download per change of the map."""
    fr = load("frontiers")
    g = load(name)
    with make_mapper(pkg, g) as m:
        og, slam = m.occ_grid, m.slam
        m.ingest_array(g["datagrams"], g["lengths"])
        # -- main() :951-955, verbatim call pattern
        frontier_cells = og.get_frontiers()
        clusters = og.cluster_frontiers(frontier_cells)
        centroids = [og.cluster_centroid_world(c) for c in clusters]
        assert [len(c) for c in clusters] == fr[name + "_sizes"].tolist()
        assert [min(c, key=lambda p: (p[1], p[0])) for c in clusters] == [tuple(v) for v in fr[name + "_first"].tolist()]
        assert [[sum(p[0] for p in c), sum(p[1] for p in c)] for c in clusters] == fr[name + "_sums"].tolist()
        assert (np.array(centroids).reshape(-1, 2) == fr[name + "_centroids"]).all()
        cellset = set(frontier_cells)
        for c in clusters:                                  # every cluster is 4-connected inside the frontier set
            assert set(c) <= cellset
            seen, todo = {c[0]}, [c[0]]
            while todo:
                x, y = todo.pop()
                for nb in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                    if nb in cellset and nb not in seen:
                        seen.add(nb); todo.append(nb)
            assert seen == set(c)
        with pytest.raises(ValueError):
            og.cluster_frontiers(frontier_cells[:-1])
        # -- PoseGraphSLAM.get_correction_for_agent, the reference's loop (:328-338) on the look-alike's attributes
        assert len(slam.nodes) == int(g["n_nodes"][0])
        nodes = slam.nodes
        for agent_id in (1, 2):
            tx = ty = 0.0
            for lm_idx, node_idx, cdx, cdy in slam.closures:
                if nodes[node_idx].agent_id == agent_id:
                    tx += cdx; ty += cdy
            assert abs(tx - m.drift(agent_id)[0]) < 1e-9 and abs(ty - m.drift(agent_id)[1]) < 1e-9
            assert np.abs(np.array(slam.get_correction_for_agent(agent_id)) - g["drift"][agent_id - 1]).max() < FLOAT_TOL
        # -- MapRenderer's read pattern (:505-516)
        og.downloads = 0
        size = og.size
        free = 0
        for gy in range(0, size, 7):
            for gx in range(0, size, 7):
                val = og.grid[gy, gx]
                if val == 0:
                    free += 1
        assert og.downloads == 1 and free > 0
        assert hashlib.sha256(og.grid.tobytes()).digest() == g["grid_sha256"].tobytes()
        og.update_ray(0.0, 0.0, 1.0, 0.5, True)             # any write drops the cached copy ...
        assert og.grid[og.world_to_grid(1.0, 0.5)[1], og.world_to_grid(1.0, 0.5)[0]] == 100 and og.downloads == 2
        for _ in range(50):                                  # ... and the object API's per-ray calls reuse their staging
            og.update_ray(0.0, 0.0, -1.0, 0.25, False)
        assert og.downloads == 2 and og.grid is og.grid


def _one_packet(P, x, y, yaw, d4, agent=1, lm=0):
    return P.pack_packets([agent], [x], [y], [yaw], [0], [0], np.asarray(d4, dtype=np.float64).reshape(1, 4), [lm])


def test_trig_edge_hunt_exact_mode(pkg):
    """VERDICT r1 item 10.  A cell index is int((rx + d cos a - ox) / res); the device library's sin / cos may differ from
    glibc's (CPython's math.cos) in the last bit, which can change the index only if the quotient sits within ~1e-12 of an
    integer.  Hunt for such inputs and show that exact mode (qs_config.exact_trig, default) gives the oracle's cells:
      1. structured streams -- yaw multiples of 15 degrees, poses on the cell lattice, centimetre distances -- on grids whose
         origin is 0 or small (the subtraction of a large origin would absorb a last-bit difference);
      2. crafted geometries: for random rays the grid origin is placed so that the HOST quotient is an integer, or the
         double just below one -- any last-bit difference on the device flips the cell;
      3. 2^17 random packets at 5 mm resolution (480 cells per ray, ~1e8 cell decisions).
    With exact_trig = 0 the same inputs are run for the record (flips are counted and printed, not asserted)."""
    P = pkg.protocol
    rng = np.random.default_rng(99)
    flips_off, edges = 0, 0
    # -- 1. structured
    yaws = np.radians(np.arange(24) * 15.0).astype(np.float32)
    lat = np.arange(-6, 7) * 0.05
    xs, ys, yw = np.meshgrid(lat, lat, yaws, indexing="ij")
    n = xs.size
    dist = (rng.integers(3, 125, (n, 4)) * 0.01)                      # whole centimetres, like the firmware's median filter
    stream = P.pack_packets(np.ones(n, dtype=int), xs.ravel(), ys.ravel(), yw.ravel(), np.zeros(n, dtype=int), np.zeros(n, dtype=int),
                            dist, np.zeros(n, dtype=int))
    for ox in (0.0, -0.8, -1.6, -3.2):
        o = orc.OracleMapper(64, 0.05, ox, ox, 0.0); o.feed_stream(stream)
        for mode in (1, 2):
            with pkg.QuasarMapper(64, 0.05, ox, ox, raycast_mode=mode) as m:
                m.ingest_array(stream)
                assert (m.grid_i8() == o.grid).all(), (ox, mode)
                h, mi = m.counts()
                assert (h == o.hits).all() and (mi == o.misses).all()
                edges += m.counters()["edge_rays"]
        with pkg.QuasarMapper(64, 0.05, ox, ox, exact_trig=False) as m:
            m.ingest_array(stream)
            flips_off += int((m.grid_i8() != o.grid).sum())
    assert edges > 0                                                   # the structured inputs DO land on cell boundaries
    # -- 2. crafted: one ray per geometry, the host quotient on / just under an integer
    import math
    crafted = 0
    for case in range(160):
        yaw = np.float32(rng.uniform(-math.pi, math.pi)); s = int(rng.integers(0, 4))
        rx, ry = np.float32(rng.uniform(0.3, 1.2)), np.float32(rng.uniform(0.3, 1.2))
        d = np.float32(rng.uniform(0.2, 1.1))
        a = float(yaw) + (0.0, math.pi / 2, math.pi, -math.pi / 2)[s]
        ex = float(rx) + float(d) * math.cos(a)
        k = int(rng.integers(20, 40))
        ox = ex - k * 0.05
        for _ in range(64):                                            # walk ox until int((ex - ox) / 0.05) changes at the next double
            if int((ex - ox) / 0.05) >= k:
                ox = np.nextafter(ox, np.inf)
            else:
                break
        ox = float(np.nextafter(ox, -np.inf)) if case % 2 else float(ox)   # quotient == k exactly / the double just below k
        d4 = [0.0, 0.0, 0.0, 0.0]; d4[s] = float(d)
        pkt = _one_packet(P, float(rx), float(ry), float(yaw), d4)
        o = orc.OracleMapper(64, 0.05, ox, -0.4, 0.0); o.feed_stream(pkt)
        with pkg.QuasarMapper(64, 0.05, ox, -0.4) as m:
            m.ingest_array(pkt)
            assert (m.grid_i8() == o.grid).all(), case
            crafted += m.counters()["edge_rays"]
        with pkg.QuasarMapper(64, 0.05, ox, -0.4, exact_trig=False) as m:
            m.ingest_array(pkt)
            flips_off += int((m.grid_i8() != o.grid).sum())
    assert crafted >= 100                                              # the crafted rays were recognised as edge rays
    # -- 3. volume: random packets, fine resolution
    stream = pkg_replay_adversarial(pkg, 1 << 17, 7)
    o = orc.OracleMapper(2048, 0.005, -5.12, -5.12, 0.0); o.feed_stream(stream)
    with pkg.QuasarMapper(2048, 0.005, -5.12, -5.12) as m:
        m.ingest_array(stream)
        assert (m.grid_i8() == o.grid).all()
        h, mi = m.counts()
        assert (h == o.hits).all() and (mi == o.misses).all()
        assert m.counters()["cells"] == o.n_cells_written
    print(f"\n[trig-edge hunt] edge rays resolved on the host: structured {edges}, crafted {crafted}; "
          f"cells differing from the oracle with exact_trig=0: {flips_off}")


def _chain_equal(m, o, n_graphs, nb):
    for g in range(n_graphs):
        idx, cc = m.closures(g); oi, oc = o.closures(g)
        assert idx.shape == oi.shape and (idx == oi).all() and (len(oi) == 0 or np.abs(cc - oc).max() < 1e-9)
        xy, ti = m.landmarks(g); oxy, oti = o.landmarks(g)
        assert ti.shape == oti.shape and (ti == oti).all() and (len(oti) == 0 or np.abs(xy - oxy).max() < 1e-9)
    for b in range(1, nb + 1):
        assert np.allclose(m.drift(b), o.drift(b), rtol=0, atol=1e-9)


@pytest.mark.parametrize("form", ["free", "free_posting", "window"])
@pytest.mark.parametrize("workload", ["session_2_bots", "adversarial_2_bots", "20_bots_one_graph", "14_bots_two_graphs"])
def test_both_chain_forms_equal_the_oracle(pkg, form, workload):
    """dual_bot_mapper.py:292-326 has several device forms (csrc/slam.hip): free-running (owner waves decide, a committer inserts
    behind them) without and with the owners posting their landmarks' poses for each other's queries; graphs of more than 13
    bots: events dealt to 14 owners (always posting); and one barrier per window.  QS_CHAIN_AUTO picks per stream, so each form
    is pinned here on its own: same closures, landmarks, drifts and grid as the oracle, over batch cuts."""
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    nb, bpg = {"session_2_bots": (2, 0), "adversarial_2_bots": (2, 0), "20_bots_one_graph": (20, 0), "14_bots_two_graphs": (14, 7)}[workload]
    if workload == "session_2_bots":
        stream = replay.cycle_stream(session, 30000)
    elif workload == "adversarial_2_bots":
        stream = replay.adversarial_stream(30000, seed=5, lo=-6.0, hi=6.0)
    else:
        stream = replay.multi_bot_stream(session, nb, 30000, pitch=1.0, origin=(-8.0, -8.0), tiles_per_row=5)
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0, max_agent=nb, bots_per_graph=bpg)
    o.feed_stream(stream)
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8, max_agent=nb, bots_per_graph=bpg) as m:
        m.set_chain_form(form)
        for lo, hi in ((0, 7000), (7000, 7001), (7001, 19000), (19000, 30000)):
            m.ingest_array(stream[lo:hi])
            assert m.chain_form() == (form if bpg or nb <= 13 or form == "window" else "free")   # (the dealt kernel reports "free")
        assert (m.grid_i8() == o.grid).all()
        _chain_equal(m, o, m.n_graphs, nb)
        assert m.counters()["slam_rounds"] < (1 << 40)              # no wait of the free-running form ran out of patience


def test_chain_form_follows_the_stream(pkg):
    """QS_CHAIN_AUTO: the free-running form without posted poses while its decisions rarely wait for the committer (the 2-bot
    session: 99.8 % of the queries find a match in what the index already holds), with them once a batch's decisions waited in
    more than 1 of 8 cases (uniform-random poses: many queries find nothing in the index), and back.  The choice survives
    qs_reset; results equal the oracle's throughout."""
    replay = _replay(pkg)
    session, _ = replay.telemetry_csv_to_packets()
    calm = replay.cycle_stream(session, 20000)
    wild = replay.adversarial_stream(20000, seed=9, lo=-12.0, hi=12.0)
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0)
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8) as m:
        forms = []
        for part in (calm, wild, wild, calm, calm):
            m.ingest_array(part); o.feed_stream(part)
            forms.append(m.chain_form())
        assert forms[0] == "free" and forms[1] == "free"            # the wild batch itself still ran free; its counts arrive after it
        assert forms[2] == "free_posting"
        assert forms[4] == "free"
        assert (m.grid_i8() == o.grid).all()
        _chain_equal(m, o, 1, 2)
        m.reset()
        m.ingest_array(wild)
        assert m.chain_form() == "free"                             # (the calm batches chose it)
        m.reset()
        m.ingest_array(wild[:5000])
        assert m.chain_form() == "free_posting"                     # kept over the reset: it describes the stream


def pkg_replay_adversarial(pkg, n, seed):
    import importlib
    replay = importlib.import_module(pkg.__name__ + ".replay")
    return replay.adversarial_stream(n, seed=seed, lo=-4.0, hi=4.0)


def test_chain_form_for_a_stream_that_hardly_ever_matches(pkg):
    """QS_CHAIN_AUTO's third state: uniform-random poses over a world so large that most queries find nothing even among the
    posted poses (more scans than closures) -- the per-window kernel, whose LDS windows are the cheaper way to find nothing.
    free -> free_posting -> window, the oracle's results throughout."""
    replay = _replay(pkg)
    parts = [replay.adversarial_stream(12000, seed=20 + i, lo=-50.0, hi=50.0) for i in range(4)]
    o = orc.OracleMapper(2048, 0.05, -51.2, -51.2, 0.0)
    with pkg.QuasarMapper(2048, 0.05, -51.2, -51.2) as m:
        forms = []
        for part in parts:
            m.ingest_array(part); o.feed_stream(part)
            forms.append(m.chain_form())
        assert forms == ["free", "free_posting", "window", "window"], forms
        assert (m.grid_i8() == o.grid).all()
        _chain_equal(m, o, 1, 2)


@pytest.mark.parametrize("max_agent,form", [(2, "auto"), (2, "free_posting"), (2, "window"), (16, "auto"), (16, "window")],
                         ids=["2_bots_free", "2_bots_free_posting", "2_bots_window", "16_bot_graph_dealt", "16_bot_graph_window"])
def test_landmark_pile_dense_fallback(pkg, max_agent, form):
    """Row J1 (K4): the stream that defeats the bucket index -- a pile of landmarks in a neighbour bucket, out of reach of the
    query point and older than the query's own first match, so every query walks the whole chain.  Once the insert wave has
    seen a chain pass 64 pool nodes the library launches the chain kernel's DENSE variant, in which a runaway query scans the
    insertion-ordered landmark log instead (the reference's own loop, a wave wide).  Same closures, landmarks and drift as the
    oracle -- whose scan IS the reference's -- before, while and after the variant changes.  Every chain kernel has the variant:
    the free-running one (2 bots), the one that deals events to 14 owners (a graph sized for 16 bots), the per-window one."""
    P = pkg.protocol
    L, NQ = 6000, 900
    px, py, qx, qy = 0.05, 0.05, 0.75, 0.35                        # |PQ| = 0.76 m: neighbouring 0.6 m buckets, out of the 0.6 m radius
    def pk(agent, x, y, n, lm=5):
        return P.pack_packets(np.full(n, agent), np.full(n, x), np.full(n, y), np.zeros(n), np.zeros(n, dtype=int), np.zeros(n, dtype=int),
                              np.full((n, 4), 0.3), np.full(n, lm))
    rng = np.random.default_rng(2)
    tail = np.concatenate([pk(1, px, py, 40), pk(2, qx, qy, 40), pk(2, qx + 0.3, qy - 0.2, 60), pk(1, px + 0.2, py + 0.1, 60)])
    rng.shuffle(tail, axis=0)
    stream = np.concatenate([pk(1, px, py, L), pk(2, qx, qy, NQ), tail])
    o = orc.OracleMapper(512, 0.05, -12.8, -12.8, 0.0, max_agent=max_agent)
    o.feed_stream(stream)
    with pkg.QuasarMapper(512, 0.05, -12.8, -12.8, max_agent=max_agent) as m:
        m.set_chain_form(form)
        for lo, hi in ((0, 2500), (2500, L), (L, L + 300), (L + 300, len(stream))):      # the pile forms in the first batches
            m.ingest_array(stream[lo:hi])
        assert m.counters()["slam_misc_iters"] > 0                  # linear (log) scans happened: the DENSE variant ran
        idx, corr = m.closures(0); oi, oc = o.closures(0)
        assert len(oi) > 200 and (idx == oi).all() and np.abs(corr - oc).max() < FLOAT_TOL
        xy, ti = m.landmarks(0); oxy, oti = o.landmarks(0)
        assert (ti == oti).all() and np.abs(xy - oxy).max() < FLOAT_TOL
        for b in (1, 2):
            assert np.abs(m.drift(b) - o.drift(b)).max() < FLOAT_TOL
        assert (m.grid_i8() == o.grid).all()
        m.reset()                                                   # a new session starts with the plain variant again
        m.ingest_array(stream[:200])
        assert m.counters()["slam_misc_iters"] == 0


@pytest.mark.parametrize("extra", [[], ["--fuse", "direct"], ["--slam-mode", "replicated", "--bots", "31"]], ids=["per_shard", "direct_fuse", "replicated"])
def test_bench_two_ranks_rehearsed_on_one_gpu(extra):
    """The N > 1 path of bench.py end to end with the REAL HIP path on every rank: `python bench.py --gpus 2` starts its two
    ranks itself; here both use cuda:0 and gloo carries the collectives (a one-GPU box has no second device for RCCL).  Each
    rank ingests its own 64 bots (own tiles, global arrival indices), the grids are fused, and the bench's own parity check
    -- fused stamps and fused counters of all ranks against the same fuse of the ranks' oracle grids, closures / landmarks /
    drift per rank -- must hold.  The timings mean nothing here."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--rehearse-on-one-gpu",
           "--batch", "65536", "--steps", "1", "--warmup", "1", "--full", "--no-micro"] + extra
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["parity_checked"] is True
    assert rec["counters_per_step"]["closures"] > 100


def test_bench_dump_outputs_same_in_every_run(tmp_path):
    """bench.py --dump-outputs: the last timed step's results, read back after the steps --steps asked for; every step starts
    from a fresh session, so a --full run of 3 steps (parity checked) and a plain run of 1 step dump the same arrays, and the dumped
    closure and landmark lists agree with the step's counters."""
    import json
    import subprocess
    import sys
    recs = []
    for name, extra in (("a", ["--steps", "3", "--warmup", "1", "--full"]), ("b", ["--steps", "1", "--warmup", "0"])):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "65536", "--no-micro",
               "--dump-outputs", str(tmp_path / name)] + extra
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        recs.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
    assert recs[0]["steps"] == 3 and recs[1]["steps"] == 1 and recs[0]["parity_checked"] is True
    assert recs[1]["parity_checked"] is None and "cpu_baseline" not in recs[1]     # the plain run left the oracle out
    assert all(r["ms_per_step"] > 0 and r["outputs_dumped"]["bytes"] < 64e6 for r in recs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "grid_cells.npy" in names and "ekf_x.npy" in names
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    cnt = recs[0]["counters_per_step"]
    sizes = np.load(tmp_path / "a" / "slam_sizes.npy")
    assert sizes[:, 2].sum() == cnt["closures"] > 0 and sizes[:, 1].sum() == cnt["landmarks"]
    assert len(np.load(tmp_path / "a" / "closures.npy")) == cnt["closures"]
