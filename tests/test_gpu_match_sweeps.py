"""Sweep matching on the GPU (qs_match_field, qs_match_sweeps*, qs_ingest_sweeps_matched*).  The bar: the CPU restatement of
include/quasar_slam.h's rules (tests/match_rules.py) fed with the rotations the device reports -- every field of every
qs_sweep_match bit for bit -- those rotations within one ulp of libm, and for the matched ingest the reference's
update_ray driven beam by beam from the corrected poses."""
import importlib
import math
import os
import socket
import time

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import match_rules as MR
from conftest import GOLDEN, load_pkg
from oracle import oracle as orc
from walk_ops import corrected as _corrected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _assert_equal(dev, ref, tag):
    for f in MR.FIELDS:
        bad = np.nonzero(dev[f] != ref[f])[0]
        assert len(bad) == 0, f"{tag}: field {f} differs in {len(bad)} records, first {bad[0]}: {dev[bad[0]]} vs {ref[bad[0]]}"
    assert dev.tobytes() == ref.tobytes(), f"{tag}: bytes differ"


def _assert_rot(rot, pose, acc, T, step, tag):
    """The device's (sin, cos) within one ulp of libm's; zeros for rejected records."""
    for k in range(len(acc)):
        if not acc[k]:
            assert (rot[k] == 0).all(), f"{tag}: rotations of rejected record {k} not zero"
            continue
        ref = MR.rotations_libm(float(pose[k, 2]), T, step)
        assert (np.abs(rot[k] - ref) <= np.spacing(np.abs(ref))).all(), f"{tag}: record {k} rotations beyond one ulp of libm"


def _check(m, grid, geom, buf, p, smin, smax, tag, lengths=None, offset=None):
    """qs_match_sweeps == the restatement fed with the device's rotations; returns the device's matches."""
    dev, rot = m.match_sweeps(buf, lengths, params=p, rotations=True)
    pp = MR.params(**p)
    ref = MR.match(grid, geom, buf, pp, lengths, smin, smax, rot=rot, offset=offset)
    _assert_equal(dev, ref, tag)
    acc, pose = MR.poses_of(MR.records_of(buf), lengths, offset)
    _assert_rot(rot, pose, acc, pp["angle_steps"], pp["angle_step"], tag)
    assert (m.match_sweeps(buf, lengths, params=p).tobytes() == dev.tobytes()), f"{tag}: with and without rot_out differ"
    return dev


def _golden_mapper(pkg, **kw):
    g = np.load(os.path.join(GOLDEN, "sweeps_512.npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    m = pkg.QuasarMapper(int(size), res, ox, oy, separation=sep, **kw)
    m.ingest_sweeps(g["sweeps_odo"])
    return g, m, (float(res), float(ox), float(oy)), float(sep)


def _displace(P, buf, seed, cells=4, steps=6, res=0.05):
    """The same records with poses displaced by up to `cells` cells and `steps` degrees."""
    rng = np.random.default_rng(seed)
    out = buf.copy()
    rec = MR.records_of(out)
    n = len(rec)
    rec["x"] += (rng.integers(-cells, cells + 1, n) * res).astype(np.float32)
    rec["y"] += (rng.integers(-cells, cells + 1, n) * res).astype(np.float32)
    rec["yaw"] += (rng.integers(-steps, steps + 1, n) * (math.pi / 180)).astype(np.float32)
    return out


@pytest.mark.parametrize("radius", [0, 2, 7])
def test_field_equals_the_restatement(pkg, radius):
    g, m, _, _ = _golden_mapper(pkg)
    with m:
        grid = m.grid_i8()
        assert (grid == g["grid"]).all()
        f = m.match_field(radius)
        ref = MR.field(grid, radius)
        assert f.dtype == np.uint8 and (f == ref).all(), f"{(f != ref).sum()} field cells differ"
        with pytest.raises(pkg.QuasarError):
            m.match_field(8)


@pytest.mark.parametrize("fmt", ["sweeps_v0", "sweeps_odo"])
def test_golden_sweeps_displaced_equal_the_restatement(pkg, fmt):
    P = _P(pkg)
    g, m, geom, sep = _golden_mapper(pkg)
    with m:
        grid = m.grid_i8()
        buf = _displace(P, g[fmt], seed=5)
        lens = np.full(len(buf), buf.shape[1], dtype=np.uint16)
        buf[3, :4] = np.frombuffer(b"QSRX", np.uint8)        # rejected: magic, agent, length
        buf[7, 4] = 3
        lens[11] = buf.shape[1] - 1
        for tag, p in (("defaults", {}), ("W4 T5 R3", dict(radius=3, window=4, angle_steps=5)),
                       ("loose gate", dict(min_hits=1, min_percent=0, angle_step=0.03))):
            dev = _check(m, grid, geom, buf, p, 0.1, 1.2, f"{fmt} {tag}", lens, {2: sep})
            assert dev["accepted_record"][[3, 7, 11]].tolist() == [0, 0, 0] and dev["accepted_record"].sum() >= 150
        assert dev["accepted_match"].sum() > 20 and (dev["score"] >= dev["score0"]).all()
        # lens = NULL means every length equals the stride
        a, b = m.match_sweeps(buf[:20], None), m.match_sweeps(buf[:20], lens[:20])
        keep = lens[:20] == buf.shape[1]
        assert a[keep].tobytes() == b[keep].tobytes() and a["accepted_record"][11] == 1


def _room_mapper(pkg, s, dirty=False, **kw):
    P = _P(pkg)
    size, res, ox, oy = MR.ROOM_GRID
    m = pkg.QuasarMapper(size, res, ox, oy, **kw)
    if dirty:
        m.dirty_tracking(True)
    m.set_sweep_filter(MR.ROOM_SMIN, MR.ROOM_SMAX)
    mp = s["map_pose"]
    m.ingest_sweeps(P.pack_sweeps(np.ones(len(mp), int), mp[:, 0], mp[:, 1], mp[:, 2], s["map_ranges"], odometry=True))
    return m


def _queries(P, s, agent=1, odometry=True):
    q = s["q_pose"]
    return P.pack_sweeps(np.full(len(q), agent), q[:, 0], q[:, 1], q[:, 2], s["q_ranges"], odometry=odometry)


ROOM_CASES = [("defaults", dict(), 30), ("W4 T5", dict(window=4, angle_steps=5), 30),
              ("window at the limit", dict(radius=2, window=127 - 2 - 60 - 2, angle_steps=0), 3),
              ("T 0", dict(angle_steps=0), 30), ("W 0", dict(window=0), 30), ("W 0 T 0", dict(window=0, angle_steps=0), 30),
              ("R 7 T max", dict(radius=7, window=1, angle_steps=45, angle_step=0.01), 6),
              ("R 0", dict(radius=0, window=5, angle_steps=3), 30), ("W 1 odd rows", dict(radius=1, window=1, angle_steps=2), 30)]


@pytest.mark.parametrize("tag,p,n", ROOM_CASES, ids=[c[0] for c in ROOM_CASES])
def test_room_equals_the_restatement(pkg, tag, p, n):
    """The synthetic room with the sweep filter (0.1, 3.0): ceil(3.0 / 0.05) = 60 cells of reach."""
    P = _P(pkg)
    pp = MR.params(**p)
    s = MR.room_session(seed=11, n_map=30, n_query=30, window=min(pp["window"], 6), angle_steps=min(pp["angle_steps"], 10))
    _, res, ox, oy = MR.ROOM_GRID
    assert math.ceil(MR.ROOM_SMAX / res) == 60 and MR.limit_ok(pp, MR.ROOM_SMAX, res)
    with _room_mapper(pkg, s) as m:
        grid = m.grid_i8()
        dev = _check(m, grid, (res, ox, oy), _queries(P, s)[:n], p, MR.ROOM_SMIN, MR.ROOM_SMAX, tag)
        if tag == "defaults":
            got = sum(MR.recovered(dev[k], s["q_disp"][k]) for k in range(30))
            print(f"device: recovered {got} of 30")
            assert got >= 27 and dev["accepted_match"].sum() >= 27


def _random_sweeps(P, n, seed, lo, hi, odometry=True):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0, 1.6, (n, 181)).astype(np.float32)
    r[rng.random((n, 181)) < 0.03] = np.nan
    return P.pack_sweeps(rng.choice(np.array([1, 2]), n), rng.uniform(lo, hi, n), rng.uniform(lo, hi, n),
                         rng.uniform(-math.pi, math.pi, n), r, odometry=odometry)


def test_edges_empty_sweeps_and_a_seeded_fuzz(pkg):
    """A 200^2 grid mapped from random sweeps up to and beyond its edges, so that patches hang outside it; queries that
    have no hit beam, no cell (NaN, 1e30) or lie off the grid; random parameters and sweep filters."""
    P = _P(pkg)
    size, res, ox, oy = 200, 0.05, -5.0, -5.0
    rng = np.random.default_rng(2024)
    with pkg.QuasarMapper(size, res, ox, oy) as m:
        empty = _random_sweeps(P, 8, 1, -4.0, 4.0)
        dev = _check(m, m.grid_i8(), (res, ox, oy), empty, {}, 0.1, 1.2, "empty map")
        assert (dev["score"] == 0).all() and (dev["accepted_match"] == 0).all() and (dev["ix"] == 0).all() and (dev["it"] == 0).all()
        m.ingest_sweeps(_random_sweeps(P, 600, 2, -5.6, 5.6))
        grid = m.grid_i8()
        assert (grid[0] == 100).any() and (grid[:, -1] == 100).any(), "the map must reach the grid's edges"
        q = _random_sweeps(P, 48, 3, -5.6, 5.6, odometry=False)
        rec = MR.records_of(q)
        rec["x"][:4] = [-4.99, 4.99, -4.99, 4.99]              # the four corners: three quarters of the patch off the grid
        rec["y"][:4] = [-4.99, -4.99, 4.99, 4.99]
        rec["ranges"][4] = np.nan                              # no hit beam
        rec["ranges"][5] = 0.0
        rec["ranges"][6] = 5.0
        rec["x"][7] = np.nan                                   # no cell
        rec["y"][8] = 1e30
        rec["x"][9] = -3e9
        rec["yaw"][10] = 50.0
        rec["x"][11], rec["y"][11] = 7.0, 7.0                  # off the grid, beyond reach of it
        dev = _check(m, grid, (res, ox, oy), q, {}, 0.1, 1.2, "edges")
        assert dev["hits"][4:7].tolist() == [0, 0, 0] and (dev["score"][7:10] == 0).all() and dev["score"][11] == 0
        assert dev["score"][:4].max() > 0, "a corner sweep must see the map"
        for it in range(6):                                     # the seeded loop
            smin = float(rng.uniform(0.0, 0.3))
            smax = float(rng.uniform(0.5, 2.0))
            R = int(rng.integers(0, 8))
            reach = math.ceil(smax / res)
            p = dict(radius=R, window=int(rng.integers(0, min(12, 127 - 2 - R - reach) + 1)), angle_steps=int(rng.integers(0, 8)),
                     angle_step=float(rng.uniform(0.0, 0.05)), min_hits=int(rng.integers(0, 60)), min_percent=int(rng.integers(0, 101)))
            m.set_sweep_filter(smin, smax)
            _check(m, grid, (res, ox, oy), _random_sweeps(P, 24, 100 + it, -5.3, 5.3, odometry=bool(it & 1)), p, smin, smax, f"fuzz {it} {p}")


def test_match_writes_nothing(pkg):
    P = _P(pkg)
    s = MR.room_session(seed=3, n_map=30, n_query=30, window=6, angle_steps=10)
    with _room_mapper(pkg, s, dirty=True) as m:
        m.ingest_sweeps(_queries(P, s)[:5])
        before = (m.grid_i8(), m.counts(), m.counters(), m.dirty_blocks(), m.checkpoint())
        for _ in range(2):
            m.match_sweeps(_queries(P, s), rotations=True)
            m.match_field(2)
        after = (m.grid_i8(), m.counts(), m.counters(), m.dirty_blocks(), m.checkpoint())
        assert (before[0] == after[0]).all() and (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        assert before[2] == after[2] and before[3] == after[3]
        assert before[4] == after[4], "checkpoint bytes (grid, counters, next sequence number, dirty blocks) changed"
        acc, pose = m.last_sweeps()                             # the last ingest is still the last ingest
        assert len(acc) == 5
        with pytest.raises(pkg.QuasarError):
            m.last_sweep_matches()


def _same_map(m, o, tag):
    g = m.grid_i8()
    assert (g == o.grid).all(), f"{tag}: {(g != o.grid).sum()} cells differ from update_ray driven with the corrected poses"
    h, mi = m.counts()
    assert (h == o.hits).all() and (mi == o.misses).all(), f"{tag}: counters differ"


@pytest.mark.parametrize("mode", [1, 2])
def test_matched_ingest_equals_update_ray_from_the_corrected_poses(pkg, mode):
    P = _P(pkg)
    size, res, ox, oy = MR.ROOM_GRID
    s = MR.room_session(seed=11, n_map=30, n_query=30, window=6, angle_steps=10)
    q = _queries(P, s)
    q[4, 4] = 9                                                 # a rejected record in the middle
    with _room_mapper(pkg, s, raycast_mode=mode, exact_trig=True) as m:
        o = orc.OracleMapper(size, res, ox, oy, 0.0)
        o.update_rays(*MR.beams_of_all(s["map_pose"], s["map_ranges"], MR.ROOM_SMIN, MR.ROOM_SMAX))
        _same_map(m, o, "before")
        pre = m.match_sweeps(q)
        c0 = m.counters()
        assert m.ingest_sweeps(q, match=True) == len(q)
        mt = m.last_sweep_matches()
        assert mt.tobytes() == pre.tobytes(), "the matches of the ingest are not those of the pre-call map"
        assert mt["accepted_match"].sum() >= 25 and (mt["ix"] != 0).any() and (mt["it"] != 0).any()
        acc, pose = MR.poses_of(MR.records_of(q))
        cp = _corrected(pose, acc, mt)
        a2, p2 = m.last_sweeps()
        assert (a2.astype(bool) == acc).all() and (p2[acc] == cp).all() and np.isnan(p2[~acc]).all()
        o.update_rays(*MR.beams_of_all(cp, MR.records_of(q)["ranges"][acc], MR.ROOM_SMIN, MR.ROOM_SMAX))
        _same_map(m, o, f"mode {mode}")
        c1 = m.counters()
        assert c1["datagrams"] - c0["datagrams"] == 30 and c1["accepted"] - c0["accepted"] == 29
        assert c1["rays"] - c0["rays"] == 29 * 181
        # the plain ingest afterwards continues the sequence numbers: one more sweep wins its cells
        m.ingest_sweeps(q[:1])
        o.update_rays(*MR.beams_of_all(pose[:1], MR.records_of(q)["ranges"][:1], MR.ROOM_SMIN, MR.ROOM_SMAX))
        _same_map(m, o, "plain after matched")
        with pytest.raises(pkg.QuasarError):
            m.last_sweep_matches()


def test_matched_ingest_in_chunks_matches_against_the_pre_call_map(pkg):
    """A call of more than one internal chunk (65536 records): the first chunk draws the room (and 65 thousand rejected
    records), the second holds the queries.  Matched after chunk 1 was mapped they would find the room; matched as the rule
    says, against the map before the call, they find nothing."""
    P = _P(pkg)
    size, res, ox, oy = MR.ROOM_GRID
    s = MR.room_session(seed=11, n_map=30, n_query=30, window=4, angle_steps=5)
    mp = s["map_pose"]
    draw = P.pack_sweeps(np.ones(30, int), mp[:, 0], mp[:, 1], mp[:, 2], s["map_ranges"], odometry=True)
    n1 = (1 << 16)
    big = np.zeros((n1 + 30, draw.shape[1]), dtype=np.uint8)
    big[:] = draw[0]
    big[:, 4] = 9                                               # rejected: agent 9
    big[1000:1030] = draw
    big[n1:] = _queries(P, s)
    prm = dict(window=4, angle_steps=5)
    with pkg.QuasarMapper(size, res, ox, oy) as m:
        m.set_sweep_filter(MR.ROOM_SMIN, MR.ROOM_SMAX)
        seed_sweep = draw[:1]
        m.ingest_sweeps(seed_sweep)                             # a map that is not empty, but not the room
        pre = m.match_sweeps(big, params=prm)
        m.ingest_sweeps(big, match=prm)
        mt = m.last_sweep_matches()
        assert mt.tobytes() == pre.tobytes()
        acc, pose = MR.poses_of(MR.records_of(big))
        assert acc.sum() == 60
        o = orc.OracleMapper(size, res, ox, oy, 0.0)
        o.update_rays(*MR.beams_of_all(mp[:1], s["map_ranges"][:1], MR.ROOM_SMIN, MR.ROOM_SMAX))
        o.update_rays(*MR.beams_of_all(_corrected(pose, acc, mt), MR.records_of(big)["ranges"][acc], MR.ROOM_SMIN, MR.ROOM_SMAX))
        _same_map(m, o, "chunked")
        late = m.match_sweeps(big[n1:], params=prm)             # the same queries against the map after the call
        assert late["accepted_match"].sum() >= 25 > mt["accepted_match"][n1:].sum()
        assert late.tobytes() != mt[n1:].tobytes()


def test_host_and_device_variants_agree(pkg):
    P = _P(pkg)
    s = MR.room_session(seed=5, n_map=30, n_query=30, window=6, angle_steps=10)
    q = _queries(P, s, odometry=False)
    lens = np.full(len(q), q.shape[1], dtype=np.uint16)
    lens[2] = 100
    dev = torch.device("cuda", 0)
    dq, dl = torch.from_numpy(q).to(dev), torch.from_numpy(lens.view(np.int16)).to(dev)
    T = 10
    d_out = torch.zeros(len(q) * MR.MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_rot = torch.zeros(len(q) * (2 * T + 1) * 2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with _room_mapper(pkg, s) as m, _room_mapper(pkg, s) as m2:
        host, rot = m.match_sweeps(q, lens, rotations=True)
        m.match_sweeps_device(dq.data_ptr(), len(q), q.shape[1], d_out.data_ptr(), d_lens=dl.data_ptr(), d_rot=d_rot.data_ptr())
        m.sync()
        assert d_out.cpu().numpy().tobytes() == host.tobytes()
        assert (d_rot.cpu().numpy().reshape(rot.shape) == rot).all()
        m.ingest_sweeps(q, lens, match=True)
        m2.ingest_sweeps_matched_device(dq.data_ptr(), len(q), q.shape[1], d_lens=dl.data_ptr())
        m2.sync()
        assert m.last_sweep_matches().tobytes() == m2.last_sweep_matches().tobytes() == host.tobytes()
        assert (m.grid_i8() == m2.grid_i8()).all()
        for a, b in zip(m.counts(), m2.counts()):
            assert (a == b).all()
        for a, b in zip(m.last_sweeps(), m2.last_sweeps()):
            assert np.array_equal(a, b, equal_nan=True)
        assert m.checkpoint() == m2.checkpoint()


def test_refusals(pkg):
    P = _P(pkg)
    r = np.full((2, 181), 0.6, dtype=np.float32)
    q = P.pack_sweeps([1, 2], [0.0, 0.1], [0.0, 0.1], [0.0, 0.1], r, odometry=True)
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0) as m:
        # ceil(1.2 / 0.05) cells of reach, radius 2: the last window that fits the limit
        wmax = MR.MAX_REACH - 2 - 2 - math.ceil(1.2 / 0.05)
        assert MR.limit_ok(MR.params(window=wmax), 1.2, 0.05) and not MR.limit_ok(MR.params(window=wmax + 1), 1.2, 0.05)
        m.match_sweeps(q, params=dict(window=wmax, angle_steps=0))
        for call in (lambda p: m.match_sweeps(q, params=p), lambda p: m.ingest_sweeps(q, match=p)):
            with pytest.raises(pkg.QuasarError, match="window is too large"):
                call(dict(window=wmax + 1, angle_steps=0))
            with pytest.raises(pkg.QuasarError, match="radius"):
                call(dict(radius=8))
            with pytest.raises(pkg.QuasarError, match="angle_steps"):
                call(dict(angle_steps=46))
            with pytest.raises(pkg.QuasarError, match="min_percent"):
                call(dict(min_percent=101))
        with pytest.raises(pkg.QuasarError, match="stride"):
            m.match_sweeps(np.ascontiguousarray(q[:, :700]))
        with pytest.raises(pkg.QuasarError, match="stride"):
            m.ingest_sweeps(np.ascontiguousarray(q[:, :700]), match=True)
        m.set_sweep_filter(0.1, 6.5)                            # 130 cells of reach: no window fits
        with pytest.raises(pkg.QuasarError, match="smax is too large"):
            m.match_sweeps(q, params=dict(window=0))
        assert m.counters()["datagrams"] == 0 and (m.grid_i8() == -1).all()
        m.set_sweep_filter()
        assert len(m.match_sweeps(q[:0])) == 0
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0, seq_stride=2) as m:
        with pytest.raises(pkg.QuasarError, match="sharded"):
            m.match_sweeps(q)
        with pytest.raises(pkg.QuasarError, match="sharded"):
            m.ingest_sweeps(q, match=True)


def test_mission_control_shows_the_corrected_pose(pkg):
    P = _P(pkg)
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    s = MR.room_session(seed=11, n_map=30, n_query=30, window=6, angle_steps=10)
    q = _queries(P, s)
    with _room_mapper(pkg, s) as m:
        q[1, 4] = 2
        want = m.match_sweeps(q[:2])
        srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        srv.bind(("127.0.0.1", 0))
        mc = fe.MissionControl(m, sock=srv, sweeps=True, match_sweeps=True)
        bot = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        bot.bind(("127.0.0.1", 0))
        for k in (0, 1):
            bot.sendto(q[k].tobytes(), ("127.0.0.1", srv.getsockname()[1]))
        time.sleep(0.05)
        assert mc.poll(now=1.0) == 2
        assert mc.last_matches.tobytes() == want.tobytes() and want["accepted_match"].all()
        for k, b in ((0, 1), (1, 2)):
            assert mc.bot_pose[b] == (s["q_pose"][k, 0] + want["dx"][k], s["q_pose"][k, 1] + want["dy"][k])
            assert mc.online[b]
        bot.close()
        mc.close()
