"""Trail matching on the GPU (qs_match_trails*).  The bar: the CPU restatement of include/quasar_slam.h's rules T1-T8
(tests/trail_rules.py) fed with the (sin, cos) the device reports -- every field of every qs_trail_match bit for bit, no case
excluded -- and those (sin, cos) within one ulp of libm.  Grids are 200 (the room) and 68 (edges), plus the 512 of the golden
session whose closures leave a drift."""
import importlib
import math
import os
import socket
import time

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import match_rules as MR
import trail_rules as TR
from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu

ROOM_MAX, ROOM_TRAVEL = 3.0, 2.8             # the room's trust filter (0.05, 3.0] and the travel its patch allows (T8)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def room():
    """The mapping sweeps and the trails every room test shares."""
    return dict(map=TR.room_map_session(), t64=TR.room_trails(21, 6, 64, 6, 10, far=ROOM_MAX))


def _P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _room_mapper(pkg, room, min_dist=TR.MIN_DIST, max_dist=ROOM_MAX, dirty=False, **kw):
    P = _P(pkg)
    size, res, ox, oy = MR.ROOM_GRID
    m = pkg.QuasarMapper(size, res, ox, oy, min_dist=min_dist, max_dist=max_dist, **kw)
    if dirty:
        m.dirty_tracking(True)
    m.set_sweep_filter(MR.ROOM_SMIN, MR.ROOM_SMAX)
    mp = room["map"]["map_pose"]
    m.ingest_sweeps(P.pack_sweeps(np.ones(len(mp), int), mp[:, 0], mp[:, 1], mp[:, 2], room["map"]["map_ranges"], odometry=True))
    return m


def _geom(m):
    return (m.res, m.ox, m.oy)


def _assert_equal(dev, ref, tag):
    for f in TR.FIELDS:
        bad = np.nonzero(dev[f] != ref[f])[0]
        assert len(bad) == 0, f"{tag}: field {f} differs in {len(bad)} trails, first {bad[0]}: {dev[bad[0]]} vs {ref[bad[0]]}"
    assert dev.tobytes() == ref.tobytes(), f"{tag}: bytes differ"


def _check(m, buf, gsize, p, travel, tag, lengths=None, min_dist=TR.MIN_DIST, max_dist=TR.MAX_DIST, sep=0.0, grid=None):
    """qs_match_trails == the restatement fed with the device's rot_out; returns the device's matches."""
    dev, rot = m.match_trails(buf, gsize, lengths, travel=travel, params=p, rotations=True)
    grid = m.grid_i8() if grid is None else grid
    bots = range(1, m.max_agent + 1)
    ref, ref_rot = TR.match(grid, _geom(m), buf, gsize, p, travel, lengths, rot=rot, min_dist=min_dist, max_dist=max_dist,
                            offset={2: sep} if m.max_agent >= 2 else {}, drift={b: tuple(float(v) for v in m.drift(b)) for b in bots},
                            max_agent=m.max_agent)
    _assert_equal(dev, ref, tag)
    # rot_out: zeros for records that do not count, else within one ulp of libm
    assert rot.tobytes() == ref_rot.tobytes() or (rot == ref_rot).all(), f"{tag}: rot_out is not zero where no record counts"
    lib = TR.rot_libm(buf, lengths, m.max_agent)
    used = (ref_rot != 0).any(axis=1)
    assert (np.abs(rot[used] - lib[used]) <= np.spacing(np.abs(lib[used]))).all(), f"{tag}: rot_out beyond one ulp of libm"
    assert m.match_trails(buf, gsize, lengths, travel=travel, params=p).tobytes() == dev.tobytes(), f"{tag}: with and without rot_out differ"
    return dev


def _pad(buf, stride):
    out = np.zeros((len(buf), stride), dtype=np.uint8)
    out[:, :min(stride, buf.shape[1])] = buf[:, :stride]
    return out


# ---- group sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 63, 64])
def test_room_trails_of_every_size_equal_the_restatement(pkg, room, K):
    t = room["t64"]
    pk = t["pkts"].reshape(6, 64, 42)[:, 64 - K:].reshape(-1, 42)           # the last K packets of each trail
    with _room_mapper(pkg, room) as m:
        dev = _check(m, pk, [K] * 6, {}, ROOM_TRAVEL, f"K {K}", max_dist=ROOM_MAX)
        assert (dev["records"] >= min(K, 50)).all() and (dev["anchor"] == K - 1).all() and (dev["agent"] == 1).all()
        if K == 64:
            got = sum(TR.recovered(dev[k], t["disp"][k]) for k in range(6))
            print(f"device: recovered {got} of 6 at K 64")
            assert got == 6 and dev["accepted_match"].all()


def test_one_group_more_than_a_host_chunk_and_no_group_at_all(pkg, room):
    """513 groups of 1 to 3 records: the host-side call stages 512 groups a round trip, the device-side one launches 512."""
    sizes = ([1, 2, 3] * 171)[:513]
    n = sum(sizes)
    pk = room["t64"]["pkts"]
    pk = np.concatenate([pk] * (n // len(pk) + 1))[:n]
    with _room_mapper(pkg, room) as m:
        p = dict(window=3, angle_steps=2, min_hits=2)
        dev = _check(m, pk, sizes, p, ROOM_TRAVEL, "513 groups", max_dist=ROOM_MAX)
        assert len(dev) == 513 and (dev["records"] >= 1).all() and (dev["anchor"] == np.array(sizes) - 1).all()
        d_pk = torch.from_numpy(pk.reshape(-1)).cuda()
        d_out = torch.full((513 * 80,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m.match_trails_device(d_pk.data_ptr(), n, 42, sizes, d_out.data_ptr(), travel=ROOM_TRAVEL, params=p)
        m.sync()
        assert d_out.cpu().numpy().tobytes() == dev.tobytes()
        out, rot = m.match_trails(pk[:0], [], travel=ROOM_TRAVEL, rotations=True)
        assert len(out) == 0 and rot.shape == (0, 2)
        m.match_trails_device(0, 0, 42, [], 0, travel=ROOM_TRAVEL)


# ---- parameter extremes -------------------------------------------------------------------------------------------------------------------
REACH = math.ceil((ROOM_MAX + ROOM_TRAVEL) / 0.05)
# (R 7 needs a window of 1 to stay inside T8 at this reach; every other case changes its one parameter alone.  The last case is
# the widest patch there is, 253 cells, with R = W = 0: the one shape whose rows are not padded, so that offsets stay 16-bit)
PARAM_CASES = [("W 0", dict(window=0), ROOM_TRAVEL), ("T 0", dict(angle_steps=0), ROOM_TRAVEL), ("R 0", dict(radius=0), ROOM_TRAVEL),
               ("R 7", dict(radius=7, window=1), ROOM_TRAVEL), ("T 45", dict(angle_steps=45, angle_step=0.004), ROOM_TRAVEL),
               ("the largest legal reach", dict(radius=2, window=127 - 2 - 2 - REACH, angle_steps=1), ROOM_TRAVEL),
               ("the widest patch, R 0 W 0", dict(radius=0, window=0, angle_steps=2), 3.25)]


@pytest.mark.parametrize("tag,p,travel", PARAM_CASES, ids=[c[0] for c in PARAM_CASES])
def test_parameter_extremes_equal_the_restatement(pkg, room, tag, p, travel):
    assert TR.limit_ok(TR.params(**p), ROOM_MAX, travel, 0.05)
    if tag.startswith("the widest"):
        assert math.ceil((ROOM_MAX + travel) / 0.05) + 2 == 127
    if tag == "the largest legal reach":
        assert not TR.limit_ok(TR.params(**dict(p, window=p["window"] + 1)), ROOM_MAX, ROOM_TRAVEL, 0.05)
    pk, gs = room["t64"]["pkts"][:3 * 64], [64, 33, 31, 64]
    if tag.startswith("the widest"):
        # a trail that fills the launch's patch: a record 3.25 m west of the anchor whose front sonar looks 3 m farther west
        far = TR.pack([1, 1], [-2.25, 1.0], [0.0, 0.0], [math.pi, 0.0], [[3.0, 0.5, 0.5, 0.5], [1.0, 1.0, 1.0, 1.0]])
        pk, gs = np.concatenate([pk, far]), gs + [2]
    with _room_mapper(pkg, room) as m:
        dev = _check(m, pk, gs, p, travel, tag, max_dist=ROOM_MAX)
        if tag.startswith("the widest"):
            assert (dev["records"][-1], dev["hits"][-1]) == (2, 8)


# ---- anchors and geometry: the 68-grid ------------------------------------------------------------------------------------------------------
def _edge_mapper(pkg):
    P = _P(pkg)
    m = pkg.QuasarMapper(68, 0.05, -1.7, -1.7)
    rng = np.random.default_rng(7)
    n = 300
    r = rng.uniform(0.0, 1.6, (n, 181)).astype(np.float32)
    m.ingest_sweeps(P.pack_sweeps(np.ones(n, int), rng.uniform(-1.9, 1.9, n), rng.uniform(-1.9, 1.9, n), rng.uniform(-math.pi, math.pi, n), r))
    return m


def test_anchors_in_every_corner_and_on_every_edge_off_the_grid_and_beyond_2_30(pkg):
    rng = np.random.default_rng(8)
    ends = [(-1.69, -1.69), (1.69, -1.69), (-1.69, 1.69), (1.69, 1.69), (0.0, -1.69), (0.0, 1.69), (-1.69, 0.0), (1.69, 0.0),
            (0.01, 0.01), (7.0, 7.0), (-40.0, 0.0), (6.0e7, 0.0), (0.0, -6.0e7), (1.0e30, 0.0), (3.0e38, 3.0e38)]
    K = 8
    groups = []
    for ex, ey in ends:
        th = rng.uniform(-math.pi, math.pi)
        back = np.arange(K - 1, -1, -1) * 0.05
        x, y = ex - back * math.cos(th), ey - back * math.sin(th)             # a straight drive that ends at (ex, ey)
        groups.append(TR.pack(np.ones(K, int), x, y, np.full(K, th), rng.uniform(0.0, 1.4, (K, 4))))
    pk = np.concatenate(groups)
    with _edge_mapper(pkg) as m:
        grid = m.grid_i8()
        assert (grid[0] == 100).any() and (grid[-1] == 100).any() and (grid[:, 0] == 100).any() and (grid[:, -1] == 100).any()
        for tag, p in (("defaults", {}), ("loose gate", dict(min_hits=1, min_percent=0, radius=3))):
            dev = _check(m, pk, [K] * len(ends), p, 1.0, f"68-grid {tag}", grid=grid)
        assert dev["score"][:9].min() > 0, "a trail that ends in a corner or on an edge must see the map"
        assert (dev["score"][9:] == 0).all() and (dev["hits"][9:] > 0).all() and (dev["ix"][9:] == 0).all() and (dev["it"][9:] == 0).all()
        # (at 6e7 a float32 steps by 4 m: the drive collapses onto a few poses; at 1e30 and 3e38 the records still count)
        assert (dev["records"][:11] == K).all() and (dev["records"][11:] >= 1).all()


# ---- record-level cases ---------------------------------------------------------------------------------------------------------------------
def test_record_level_cases_go_through_the_device(pkg, room):
    t = room["t64"]
    base = t["pkts"][:64].copy()
    rec = lambda b: b.view(TR.PACKET_DTYPE).reshape(-1)
    cases, lens = [], []

    def add(b, ln=None):
        cases.append(b)
        lens.append(np.full(len(b), 42, dtype=np.uint16) if ln is None else ln)

    for how in ("magic", "agent", "length", "nan x", "inf yaw"):                 # a rejected last record: an earlier anchor
        b, ln = base[:9].copy(), np.full(9, 42, dtype=np.uint16)
        if how == "magic":
            b[8, 3] = ord("X")
        elif how == "agent":
            b[8, 4] = 3
        elif how == "length":
            ln[8] = 43
        elif how == "nan x":
            rec(b)["x"][8] = np.nan
        else:
            rec(b)["yaw"][8] = np.inf
        add(b, ln)
    b = base[:12].copy()                                                       # mixed agents: the anchor's bot rules
    b[::2, 4] = 2
    add(b)
    add(b[:11])
    b = base[:3].copy()                                                        # travel: 1 m and 2 m from the anchor, exactly
    rec(b)["x"][:] = (-1.0, 0.0, 0.0)
    rec(b)["y"][:] = (0.0, 2.0, 0.0)
    travel_case = len(cases)
    add(b)
    b = base[:8].copy()                                                        # ranges that are not numbers, zero, negative, huge
    rec(b)["dist"][:] = [[np.nan, np.inf, -np.inf, 0.0], [-1.0, 1e30, 0.04, 0.049]] * 4
    add(b)
    b = base[:5].copy()                                                        # all rejected
    b[:, 0] = 0
    add(b)
    ln41 = np.full(6, 41, dtype=np.uint16)                                     # v1 packets: 41 bytes, no landmark byte
    add(base[:6].copy(), ln41)
    pk, ln, gs = np.concatenate(cases), np.concatenate(lens), [len(c) for c in cases]
    loose = dict(min_hits=1, min_percent=10)
    with _room_mapper(pkg, room) as m:
        grid = m.grid_i8()
        dev = _check(m, _pad(pk, 48), gs, loose, ROOM_TRAVEL, "record cases", ln, max_dist=ROOM_MAX, grid=grid)
        assert dev["anchor"][:5].tolist() == [7] * 5 and dev["records"][:5].tolist() == [8] * 5
        assert (dev["agent"][5], dev["records"][5], dev["agent"][6], dev["records"][6]) == (1, 6, 2, 6)
        assert dev["hits"][travel_case + 1] == 0 and dev["records"][travel_case + 1] == 8
        want = np.zeros(1, dtype=TR.TRAIL_DTYPE)
        want["anchor"] = -1
        assert dev[travel_case + 2].tobytes() == want.tobytes()
        assert dev["records"][travel_case + 3] == 6
        for travel, n in ((2.0, 3), (math.nextafter(2.0, 0.0), 2), (1.0, 2), (math.nextafter(1.0, 0.0), 1), (0.0, 1)):
            d = _check(m, pk, gs, loose, travel, f"travel {travel!r}", ln, max_dist=ROOM_MAX, grid=grid)
            assert d["records"][travel_case] == n
    # ranges exactly at the bounds of a filter a float32 holds exactly
    b = base[:8].copy()
    up = lambda v, to: float(np.nextafter(np.float32(v), np.float32(to)))
    rec(b)["dist"][:] = [[0.25, up(0.25, 1), 1.5, up(1.5, 2)], [up(0.25, 0), 0.26, up(1.5, 0), 1.51]] * 4
    with _room_mapper(pkg, room, min_dist=0.25, max_dist=1.5) as m:
        d = _check(m, b, [8], loose, 4.0, "filter bounds", min_dist=0.25, max_dist=1.5)
        assert d["hits"][0] == 4 * 2 + 4 * 2


# ---- drift and offset -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["session_512", "session_sep_512"])
def test_drift_and_bot_twos_offset_enter_the_pose(pkg, name):
    """A context that has ingested a golden session: its closures leave both bots a drift (and session_sep_512 sets bot 2 half a
    metre apart).  The session's own packets are the trails: interleaved bots as they arrived, and each bot's own."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    d, ln = g["datagrams"], g["lengths"]
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as m:
        m.ingest_array(d, ln, recv_time=None)
        assert np.abs(m.drift(1)).max() > 0.1 and np.abs(m.drift(2)).max() > 0.1
        own = [d[d[:, 4] == b][-128:] for b in (1, 2)]
        pk = np.concatenate([d[-256:], own[0], own[1]])
        lens = np.concatenate([ln[-256:], np.full(256, 42, dtype=np.uint16)])
        dev = _check(m, pk, [64] * 8, dict(min_hits=5), 4.0, name, lens, sep=float(sep))
        assert set(dev["agent"][:4].tolist()) <= {1, 2} and dev["agent"][4:].tolist() == [1, 1, 2, 2]
        assert (dev["records"][4:] == 64).all() and (dev["records"][:4] < 64).all() and (dev["hits"] > 0).all()
        # ONE drift: what qs_drift reports now
        k = int(dev["anchor"][6])
        x, y = (float(v) for v in own[1][k, 5:13].view("<f4"))
        assert (dev["ax"][6], dev["ay"][6]) == ((x + float(sep)) + float(m.drift(2)[0]), y + float(m.drift(2)[1]))


# ---- strides and alignment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [42, 41, 48, 64, 100])
def test_strides_and_device_buffers_at_odd_addresses(pkg, room, stride):
    """Every stride through the host entry and, at byte offsets 0 to 3, through the device entry: equal bytes."""
    pk = room["t64"]["pkts"][:2 * 64 + 20]
    gs = [64, 33, 31, 20]
    n = len(pk)
    buf = _pad(pk, stride)
    lens = np.full(n, 41 if stride == 41 else 42, dtype=np.uint16)
    dev = torch.device("cuda", 0)
    with _room_mapper(pkg, room) as m:
        want, rot = m.match_trails(buf, gs, lens, travel=ROOM_TRAVEL, rotations=True)
        ref = _check(m, buf, gs, {}, ROOM_TRAVEL, f"stride {stride}", lens, max_dist=ROOM_MAX)
        assert ref.tobytes() == want.tobytes()
        if stride != 41:                                           # lens = NULL: every length is the stride
            keep = m.match_trails(buf, gs, None, travel=ROOM_TRAVEL)
            if stride == 42:
                assert keep.tobytes() == want.tobytes()
            else:
                assert (keep["anchor"] == -1).all()                # a 48-byte "packet" is no packet
        d_lens = torch.from_numpy(lens.view(np.int16)).to(dev)
        for mis in (0, 1, 2, 3):
            d_q = torch.full((buf.size + 8,), 0xEE, dtype=torch.uint8, device=dev)
            d_q[mis:mis + buf.size] = torch.from_numpy(buf.reshape(-1)).to(dev)
            d_out = torch.full((len(gs) * 80,), 0xAB, dtype=torch.uint8, device=dev)
            d_rot = torch.full((2 * n,), 7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            m.match_trails_device(d_q.data_ptr() + mis, n, stride, gs, d_out.data_ptr(), d_lens=d_lens.data_ptr(),
                                  d_rot=d_rot.data_ptr(), travel=ROOM_TRAVEL)
            m.sync()
            assert d_out.cpu().numpy().tobytes() == want.tobytes(), f"stride {stride}, offset {mis}: device entry differs"
            assert d_rot.cpu().numpy().tobytes() == rot.tobytes(), f"stride {stride}, offset {mis}: rot_out differs"
            assert (d_q[:mis].cpu().numpy() == 0xEE).all() and (d_q[mis + buf.size:].cpu().numpy() == 0xEE).all()


# ---- state ---------------------------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_before_equals_one_after(pkg, room):
    pk = room["t64"]["pkts"]
    with _room_mapper(pkg, room, dirty=True, enable_ekf=True) as m:
        m.ingest_array(pk[:100])
        before, cnt = m.checkpoint(), m.counters()
        for p in ({}, dict(radius=7, window=1, angle_steps=45, angle_step=0.004)):
            m.match_trails(pk, room["t64"]["gsize"], travel=ROOM_TRAVEL, params=p, rotations=True)
        assert m.checkpoint() == before and m.counters() == cnt
        acc, _ = m.last_batch()                                    # the last ingest is still the packets'
        assert len(acc) == 100


def test_every_refusal_with_its_text(pkg, room):
    pk = room["t64"]["pkts"][:64]
    with _room_mapper(pkg, room) as m:
        before = m.checkpoint()
        for p, word in ((dict(radius=8), "radius"), (dict(radius=-1), "radius"), (dict(window=-1), "window"),
                        (dict(angle_steps=46), "angle_steps"), (dict(angle_steps=-1), "angle_steps"), (dict(min_hits=-1), "min_hits"),
                        (dict(min_percent=101), "min_percent"), (dict(angle_step=float("nan")), "angle_step"),
                        (dict(angle_step=-0.1), "angle_step"), (dict(window=127 - 2 - 2 - REACH + 1), "window is too large"),
                        (dict(radius=7, window=127 - 7 - 2 - REACH + 1), "window is too large")):
            with pytest.raises(pkg.QuasarError, match=word):
                m.match_trails(pk, [64], travel=ROOM_TRAVEL, params=p)
        for travel in (-1.0, float("nan"), float("inf")):
            with pytest.raises(pkg.QuasarError, match="travel must be finite"):
                m.match_trails(pk, [64], travel=travel)
        with pytest.raises(pkg.QuasarError, match=r"max_dist \+ travel is too large"):
            m.match_trails(pk, [64], travel=4.0)
        for gs, word in (([0, 64], r"gsize\[0\] must lie in \[1, QS_TRAIL_MAX_RECORDS\]"), ([32, 65], r"gsize\[1\] must lie in"),
                         ([32, -1], r"gsize\[1\]"), ([63], "sum to n"), ([64, 1], "sum to n"), ([], "sum to n")):
            with pytest.raises(pkg.QuasarError, match=word):
                m.match_trails(pk, gs, travel=ROOM_TRAVEL)
        with pytest.raises(pkg.QuasarError, match="stride must be at least 41"):
            m.match_trails(pk[:, :40], [64], travel=ROOM_TRAVEL)
        d_pk = torch.from_numpy(pk.reshape(-1)).cuda()
        d_out = torch.zeros(80, dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.QuasarError, match=r"gsize\[0\]"):
            m.match_trails_device(d_pk.data_ptr(), 64, 42, [65], d_out.data_ptr(), travel=ROOM_TRAVEL)
        with pytest.raises(pkg.QuasarError, match="travel"):
            m.match_trails_device(d_pk.data_ptr(), 64, 42, [64], d_out.data_ptr(), travel=-1.0)
        assert m.checkpoint() == before
        assert len(m.match_trails(pk, [64], travel=ROOM_TRAVEL)) == 1          # and the context still answers
    with pkg.QuasarMapper(200, 0.05, -5.0, -5.0, seq_stride=2) as m:
        with pytest.raises(pkg.QuasarError, match="sharded"):
            m.match_trails(pk, [64])


def test_the_query_in_a_used_context(pkg, room):
    """After update_rays, packets, sweeps, a restore and a reset the answer is the restatement's on the map as it then stands:
    nothing is kept between calls, and a query of another shape in between (the 131 KiB patch, then the small one) changes none."""
    P = _P(pkg)
    size, res, ox, oy = MR.ROOM_GRID
    t = room["t64"]
    pk, gs = t["pkts"], t["gsize"]
    s = room["map"]
    big = dict(radius=2, window=127 - 2 - 2 - REACH, angle_steps=0)
    with pkg.QuasarMapper(size, res, ox, oy, min_dist=TR.MIN_DIST, max_dist=ROOM_MAX) as m:
        m.set_sweep_filter(MR.ROOM_SMIN, MR.ROOM_SMAX)
        dev = _check(m, pk, gs, {}, ROOM_TRAVEL, "empty map", max_dist=ROOM_MAX)
        assert (dev["score"] == 0).all() and not dev["accepted_match"].any() and (dev["ix"] == 0).all() and (dev["it"] == 0).all()
        m.update_rays(*MR.beams_of_all(s["map_pose"][:15], s["map_ranges"][:15], MR.ROOM_SMIN, MR.ROOM_SMAX))
        a = _check(m, pk, gs, {}, ROOM_TRAVEL, "after update_rays", max_dist=ROOM_MAX)
        assert a["score"].max() > 0
        _check(m, pk[:64], [64], big, ROOM_TRAVEL, "the largest patch", max_dist=ROOM_MAX)
        m.ingest_array(pk[:64])                                    # the first trail's own packets: it now agrees with itself
        b = _check(m, pk, gs, {}, ROOM_TRAVEL, "after packets", max_dist=ROOM_MAX)
        assert b["score0"][0] > a["score0"][0]
        mp = s["map_pose"][15:]
        m.ingest_sweeps(P.pack_sweeps(np.ones(len(mp), int), mp[:, 0], mp[:, 1], mp[:, 2], s["map_ranges"][15:], odometry=True))
        c = _check(m, pk, gs, {}, ROOM_TRAVEL, "after sweeps", max_dist=ROOM_MAX)
        ck = m.checkpoint()
        with pkg.QuasarMapper(size, res, ox, oy, min_dist=TR.MIN_DIST, max_dist=ROOM_MAX) as twin:
            twin.set_sweep_filter(MR.ROOM_SMIN, MR.ROOM_SMAX)
            twin.restore(ck)
            d = _check(twin, pk, gs, {}, ROOM_TRAVEL, "after a restore", max_dist=ROOM_MAX)
            assert d.tobytes() == c.tobytes()
        m.reset()
        e = _check(m, pk, gs, {}, ROOM_TRAVEL, "after a reset", max_dist=ROOM_MAX)
        assert e.tobytes() == dev.tobytes()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def _drive(pkg, room, pkts, **mc_kw):
    """A real MissionControl on a mapped room, fed pkts over a socket pair; (occupied cells, trail_stats, matches)."""
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    bot = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    bot.bind(("127.0.0.1", 0))
    with _room_mapper(pkg, room) as m:
        mc = fe.MissionControl(m, sock=srv, **mc_kw)
        for r in pkts:
            bot.sendto(r.tobytes(), srv.getsockname())
        for _ in range(200):                                       # (loopback delivers at once; the loop only bounds the wait)
            if mc.datagrams >= len(pkts):
                break
            mc.poll(now=50.0)
            time.sleep(0.001)
        assert mc.datagrams == len(pkts)
        mc.flush_trails(now=51.0)
        occ = m.grid_i8() == 100
        out = (occ, dict(mc.trail_stats), dict(mc.trail_matches), int(m.counters()["accepted"]))
        mc.close()
    bot.close()
    return out


def test_mission_control_maps_a_displaced_trail_where_the_undisplaced_one_is(pkg, room):
    """A trail displaced rigidly by (3, -2) cells and 4 degrees, fed to a MissionControl that matches packets, ends up mapped where
    the undisplaced one is: the same OCCUPIED cells to within ROUND_TRIP_CELLS = 1 (test_sense_rules_cpu.py's bound).  Fed to a
    MissionControl that does not match, it does not."""
    from scipy import ndimage
    K = 64
    t = TR.room_trails(31, 1, K, 0, 0, far=ROOM_MAX)
    true, ranges = t["true"][0], t["ranges"][0]
    packets = lambda pose: TR.pack(np.ones(K, int), pose[:, 0], pose[:, 1], pose[:, 2], ranges)
    straight, moved = packets(TR.displaced(true, (0, 0, 0))), packets(TR.displaced(true, (3, -2, 4)))
    on = dict(match_packets=dict(trail=K, travel=ROOM_TRAVEL))
    occ_a, st_a, ma_a, n_a = _drive(pkg, room, straight, **on)
    occ_b, st_b, ma_b, n_b = _drive(pkg, room, moved, **on)
    occ_c, st_c, _, n_c = _drive(pkg, room, moved)
    assert st_a == dict(held=K, tried=1, accepted=1, moved=0, rewritten=0), st_a
    assert st_b == dict(held=K, tried=1, accepted=1, moved=1, rewritten=K), st_b
    assert st_c == dict(held=0, tried=0, accepted=0, moved=0, rewritten=0)
    assert n_a == n_b == n_c == K + len(room["map"]["map_pose"])   # (the counter counts the mapping sweeps too)
    assert (int(ma_a[1]["ix"]), int(ma_a[1]["iy"]), int(ma_a[1]["it"])) == (0, 0, 0)
    assert (int(ma_b[1]["ix"]), int(ma_b[1]["iy"]), int(ma_b[1]["it"])) == (-3, 2, -4) and int(ma_b[1]["records"]) >= 50
    grow = lambda o: ndimage.maximum_filter(o.astype(np.uint8), size=3, mode="constant", cval=0) > 0
    miss_b = int((occ_b & ~grow(occ_a)).sum()) + int((occ_a & ~grow(occ_b)).sum())
    miss_c = int((occ_c & ~grow(occ_a)).sum()) + int((occ_a & ~grow(occ_c)).sum())
    print(f"occupied cells farther than one cell from the other map: matched {miss_b}, unmatched {miss_c}")
    assert miss_b == 0
    assert miss_c > 0
