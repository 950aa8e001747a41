"""Relocalisation of a group on the GPU (qs_relocalise_groups and its _device twin).  The bar: the CPU restatement of the rules
J1-J8 (tests/reloc_group_rules.py) fed grid_i8() -- every field of every output with ==, the doubles as bits.  The worlds are
painted as tests/test_gpu_relocalise.py paints them and the sweeps are sensed on the device, so both sides read the same bytes."""
import importlib
import math

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import maze_scenes as MZ
import reloc_group_rules as GR
import reloc_rules as RR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
SIZE, RES, OX, OY = RR.WORLD_GRID
GEOM = (RES, OX, OY)
FAR, NEAR = (0.1, 3.0), (0.1, 1.2)
SMALL_GEOM = (0.05, -1.7, -1.7)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _painted(pkg, grid, res, ox, oy):
    m = pkg.QuasarMapper(len(grid), res, ox, oy)
    MZ.paint(m, RR.paint_rays(grid), res, ox, oy)
    assert (m.grid_i8() == grid).all()
    return m


@pytest.fixture(scope="module")
def W(pkg):
    """The world of tests/reloc_rules.py painted into a mapper, and 6 groups of 3 sweeps 0.5 m apart sensed in it at 3.0 m:
    (mapper, grid, sweeps uint8 [18, 751], poses float32 [6, 3, 3], cells)."""
    grid = RR.world()
    m = _painted(pkg, grid, RES, OX, OY)
    poses, cells = RR.query_poses(grid, GEOM, 6, seed=5)
    G = GR.build_groups(grid, GEOM, poses, 3, 0.5, seed=5)
    buf = m.sense_sweeps(G.reshape(-1, 3), 1, max_range=3.0)
    yield m, grid, buf, G, cells
    m.close()


@pytest.fixture(scope="module")
def S(pkg):
    """The small world and 3 groups of 2 sweeps sensed in it at 3.0 m, the second 0.3 m ahead of the first."""
    grid = RR.small_world()
    m = _painted(pkg, grid, *SMALL_GEOM)
    cells = np.array([(3, 3), (64, 2), (30, 30)])
    yaw = np.arctan2(34 - cells[:, 1], 34 - cells[:, 0]) + np.array([0.1, -0.2, 2.0])
    first = np.stack([SMALL_GEOM[1] + (cells[:, 0] + 0.5) * 0.05, SMALL_GEOM[2] + (cells[:, 1] + 0.5) * 0.05, yaw], axis=1)
    second = first + np.stack([0.3 * np.cos(yaw), 0.3 * np.sin(yaw), np.full(3, 0.4)], axis=1)
    poses = np.stack([first, second], axis=1).reshape(-1, 3).astype(np.float32)
    buf = m.sense_sweeps(poses, 1, max_range=3.0)
    yield m, grid, buf
    m.close()


def _check(m, grid, geom, buf, gsize, p=None, filt=FAR, travel=2.0, rel=None, lengths=None, expected=None):
    """One host call against the restatement; returns the device's output."""
    m.set_sweep_filter(*filt)
    got = m.relocalise_groups(buf, gsize, lengths, rel, travel, params=p)
    exp = GR.reloc_groups(grid, geom, buf, gsize, rel, travel, p, lengths, *filt) if expected is None else expected
    assert got.dtype == GR.GROUP_DTYPE and len(got) == len(gsize)
    bad = GR.differing(got, exp)
    assert not bad, bad
    return got


@pytest.mark.parametrize("filt", [FAR, NEAR], ids=["3.0m", "1.2m"])
def test_sensed_groups_equal_the_restatement(W, filt):
    m, grid, buf, G, cells = W
    got = _check(m, grid, GEOM, buf, [3] * 6, dict(n_rot=36), filt, travel=1.1)
    assert (got["status"] == GR.OK).all() and (got["records"] == 3).all()
    if filt == FAR:                              # three sweeps at 3.0 m see enough: found within a cell, whatever the gate says
        near = sum(abs(int(got["gx"][k]) - cells[k][0]) <= 1 and abs(int(got["gy"][k]) - cells[k][1]) <= 1 for k in range(6))
        assert near >= 4, near


def test_group_sizes_one_two_and_sixteen(W, pkg):
    """16 sweeps 0.2 m apart (travel 3.1 m, the 1.2 m filter: a patch of 16 + 2 * 89 cells), with a group of 1 and one of 2."""
    m, grid = W[:2]
    poses, cells = RR.query_poses(grid, GEOM, 3, seed=9)
    long_ = GR.build_groups(grid, GEOM, poses[:1], 16, 0.2, seed=9)[0]
    pair = GR.build_groups(grid, GEOM, poses[1:2], 2, 0.5, seed=9)[0]
    buf = m.sense_sweeps(np.concatenate([poses[2:3], pair, long_]), 1, max_range=1.2)
    gx, gy = cells[0]
    got = _check(m, grid, GEOM, buf, [1, 2, 16], dict(n_rot=36, box=(gx - 24, gy - 24, gx + 24, gy + 24), min_hits=20), NEAR, travel=3.1)
    assert got["records"].tolist() == [1, 2, 16]


def test_a_group_of_one_gives_the_bytes_of_the_single_sweep_call(W):
    m, grid, buf = W[:3]
    q = buf[:5].copy()
    q[3, 0] = ord("X")
    for filt, p in ((FAR, None), (NEAR, dict(radius=7, n_rot=45))):
        m.set_sweep_filter(*filt)
        single = m.relocalise_sweeps(q, params=p)
        group = m.relocalise_groups(q, [1] * 5, rel=np.repeat(GR.IDENTITY, 5), travel=0.0, params=p)
        assert group.tobytes() == single.tobytes()
        assert single["status"].tolist() == [RR.OK] * 3 + [RR.NO_RECORD, RR.OK]


def _dense_group(P, k, seed):
    """k records whose 181 beams all hit (0.3 to 1.1 m) at small relative poses: (buf, rel)."""
    rng = np.random.default_rng(seed)
    ranges = rng.uniform(0.3, 1.1, (k, 181)).astype(np.float32)
    buf = P.pack_sweeps([1] * k, [0.0] * k, [0.0] * k, [0.0] * k, ranges)
    th = rng.uniform(-math.pi, math.pi, k)
    rel = np.array([(rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), math.sin(t), math.cos(t)) for t in th], dtype=GR.REL_DTYPE)
    return buf, rel


def _keep_hits(buf, H):
    """The first H beams of the records, in record order, kept; the others blanked."""
    q = buf.copy()
    blank = np.repeat(np.arange(len(q) * 181).reshape(len(q), 181) >= H, 4, axis=1)
    q[:, 27:][blank] = 0
    return q


@pytest.mark.parametrize("radius,span", [(2, 80), (7, 24), (0, 248)])
def test_hit_counts_at_the_edges_of_the_loops(S, P, radius, span):
    """The pass over the offsets takes them eight, then four, then one at a time, in spans whose byte sums cannot overflow:
    H on both sides of 8 and of one and two spans."""
    m, grid, _ = S
    assert span == (255 // (radius + 1)) & ~7
    counts = [7, 8, 9, span - 1, span, span + 1, 2 * span + 3]
    base, rel1 = _dense_group(P, 3, seed=radius)
    buf = np.concatenate([_keep_hits(base, H) for H in counts])
    rel = np.tile(rel1, len(counts))
    got = _check(m, grid, SMALL_GEOM, buf, [3] * len(counts), dict(radius=radius, n_rot=8, min_hits=1), NEAR, travel=0.5, rel=rel)
    assert got["hits"].tolist() == counts and (got["status"] == GR.OK).all()


def test_the_most_points_a_group_can_have(S, P):
    """16 records of 181 hit beams, R = 7: H = 2 896, full score 23 168."""
    m, grid, _ = S
    buf, rel = _dense_group(P, 16, seed=11)
    got = _check(m, grid, SMALL_GEOM, buf, [16], dict(radius=7, n_rot=8, min_hits=1), NEAR, travel=0.5, rel=rel)
    assert got["hits"][0] == 2896 and got["records"][0] == 16 and got["score"][0] > 0


def test_points_at_the_edge_of_reach_and_a_dishonest_rotation(S, P):
    """travel 4.59 m with the 1.2 m filter is J8's limit at 5 cm: ceil(5.79 / 0.05) = 116, a patch of 254 cells (2 x 69 KB of
    LDS).  Records stand at the four ends of travel and look outwards: their points (beams of 1.19 m) reach 5.78 m, M - 1 cells, on each axis.  A
    fifth carries (s, c) = (1, 1) and is out of reach under some rotations."""
    m, grid, _ = S
    t = 4.59
    assert 16 + 2 * (math.ceil((1.2 + t) / 0.05) + 2 + 1) == 254
    r = np.full((5, 181), 1.19, dtype=np.float32)
    buf = P.pack_sweeps([1] * 5, [0.0] * 5, [0.0] * 5, [0.0] * 5, r)
    rel = np.array([(t, 0, 0, 1), (-t, 0, 0, -1), (0, t, 1, 0), (0, -t, -1, 0), (t, 0, 1, 1)], dtype=GR.REL_DTYPE)
    records, px, py = GR.points(r, rel, [True] * 5, t, 0.1, 1.2)
    ax, ay, reach = GR.point_offsets(px, py, RR.rotations(36), 0.05, 117)
    assert records == 5 and max(np.abs(ax).max(), np.abs(ay).max()) >= 116 and reach[:, :724].all() and not reach[:, 724:].all()
    got = _check(m, grid, SMALL_GEOM, buf, [5], dict(n_rot=36, min_hits=1), NEAR, travel=t, rel=rel)
    assert (got["status"][0], got["records"][0], got["hits"][0]) == (GR.OK, 5, 905)


def test_rejected_records_in_a_group(W):
    """A broken record first, in the middle, last; every record broken; a record out of travel; a group that sees nothing."""
    m, grid, buf = W[:3]
    q = buf.copy()
    lens = np.full(len(q), q.shape[1], dtype=np.uint16)
    q[0, 0] = ord("X")                           # group 0: first
    q[4, 4] = 3                                  # group 1: middle (agent beyond max_agent)
    lens[8] = 750                                # group 2: last
    q[9, 4] = 0; q[10, 0] = 0; lens[11] = 7      # group 3: all
    q[12:15, 27:] = 0                            # group 4: H = 0
    rel = np.concatenate([GR.rel_of(*q[3 * g:3 * g + 3, 5:17].copy().view("<f4").T) for g in range(6)])
    rel["tx"][16] = 5.0                          # group 5: its middle record lies beyond travel
    got = _check(m, grid, GEOM, q, [3] * 6, dict(n_rot=36), FAR, travel=1.1, rel=rel, lengths=lens)
    assert got["records"].tolist() == [2, 2, 2, 0, 3, 2]
    assert got["status"].tolist() == [GR.OK, GR.OK, GR.OK, GR.NO_RECORD, GR.NO_CANDIDATE, GR.OK]
    assert got[3].tobytes() == bytes([0] * 36 + [GR.NO_RECORD] + [0] * 35) and got["hits"][4] == 0 and got["gx"][4] == -1


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_group_counts_and_one_more_than_a_chunk(W, n):
    """65 is one group more than the 64 a launch takes.  The 6 sensed groups in turn; the restatement runs on those 6."""
    m, grid, buf = W[:3]
    p = dict(n_rot=8, box=(16, 20, 130, 110))
    base = GR.reloc_groups(grid, GEOM, buf, [3] * 6, None, 1.1, p, None, *FAR)
    idx = np.arange(n) % 6
    recs = (3 * idx[:, None] + np.arange(3)[None, :]).reshape(-1)
    _check(m, grid, GEOM, np.ascontiguousarray(buf[recs]), [3] * n, p, FAR, travel=1.1, expected=base[idx])


def test_box_edges(S):
    m, grid, buf = S
    size = len(grid)
    boxes = [(-3, -3, 15, 15), (0, 0, 16, 16), (15, 16, 17, size + 5), (16, 15, size + 5, 17), (17, 17, size + 5, size + 5),
             (-3, 0, size + 5, 16), (0, -3, 17, size), (15, 15, 16, 16), (16, 16, 17, 17)]
    for box in boxes:
        got = _check(m, grid, SMALL_GEOM, buf, [2, 2, 2], dict(n_rot=8, box=box), travel=0.5)
        x0, y0, x1, y1 = RR.clip_box(box, size)
        assert (got["status"] == GR.OK).all() and (got["gx"] >= x0).all() and (got["gx"] < x1).all()
        assert (got["gy"] >= y0).all() and (got["gy"] < y1).all()
    for box in ((20, 40, 21, 44), (30, 30, 30, 40), (size, 0, size + 5, size)):
        none = _check(m, grid, SMALL_GEOM, buf, [2, 2, 2], dict(n_rot=8, box=box), travel=0.5)
        assert (none["status"] == GR.NO_CANDIDATE).all() and (none["records"] == 2).all()


def test_best_on_a_tile_corner_and_the_exclusion_square(W):
    """A group whose frame stands in cell (63, 47), the last column and row of its tile: the square round the best covers four
    tiles at sep 4, one at sep 0 and nine at sep 16."""
    m, grid = W[:2]
    x, y = OX + 63.5 * RES, OY + 47.5 * RES
    pose = np.array([[x, y, 0.3], [x + 0.4 * math.cos(0.5), y + 0.4 * math.sin(0.5), 0.9]], dtype=np.float32)
    buf = m.sense_sweeps(pose, 1, max_range=3.0)
    for sep in (0, 4, 16):
        got = _check(m, grid, GEOM, buf, [2], dict(sep=sep), travel=0.5)
        assert (got["gx"][0], got["gy"][0]) == (63, 47), "the group was meant to be found in its own cell"
        near = _check(m, grid, GEOM, buf, [2], dict(sep=sep, box=(48, 32, 80, 64)), travel=0.5)
        assert (near["gx"][0], near["gy"][0], near["j"][0]) == (63, 47, got["j"][0]) and 48 <= near["gx2"][0] < 80


@pytest.mark.parametrize("n_rot", [1, 360])
def test_rotation_counts(W, n_rot):
    m, grid, buf = W[:3]
    _check(m, grid, GEOM, buf[:6], [3, 3], dict(n_rot=n_rot, sep_rot=min(2, n_rot - 1), box=(16, 20, 100, 84)), travel=1.1)


def test_host_call_and_device_twin_at_both_strides_and_every_misalignment(W):
    m, grid, buf = W[:3]
    m.set_sweep_filter(*FAR)
    dev = torch.device("cuda", 0)
    p = dict(n_rot=24)
    gsize = [1, 3, 2, 3]
    for odometry in (True, False):
        q = np.ascontiguousarray(buf[:9] if odometry else np.delete(buf[:9], np.s_[17:25], axis=1))
        assert q.shape[1] == (751 if odometry else 743)
        lens = np.full(len(q), q.shape[1], dtype=np.uint16)
        lens[5] = 7
        host = m.relocalise_groups(q, gsize, lens, travel=1.0, params=p)
        exp = GR.reloc_groups(grid, GEOM, q, gsize, None, 1.0, p, lens, *FAR)
        assert not GR.differing(host, exp) and host["records"][0] == host["records"][2] == 1      # (record 5 is broken)
        pose = q[:, 5:17].copy().view("<f4")
        rel = np.concatenate([GR.rel_of(*pose[a:b].T) for a, b in ((0, 1), (1, 4), (4, 6), (6, 9))])
        d_rel = torch.from_numpy(rel.view(np.float64).copy()).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int16)).to(dev)
        for mis in range(4):
            d_q = torch.zeros(q.size + 8, dtype=torch.uint8, device=dev)
            d_q[mis:mis + q.size] = torch.from_numpy(q.reshape(-1)).to(dev)
            d_out = torch.full((len(gsize) * GR.GROUP_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            m.relocalise_groups_device(d_q.data_ptr() + mis, len(q), q.shape[1], d_rel.data_ptr(), gsize, d_out.data_ptr(),
                                       d_lens=d_lens.data_ptr(), travel=1.0, params=p)
            m.sync()
            assert d_out.cpu().numpy().tobytes() == host.tobytes(), (odometry, mis)


def test_a_call_leaves_the_context_unchanged(W):
    m, grid, buf = W[:3]
    m.set_sweep_filter(*FAR)
    before = (m.grid_i8(), m.counters(), m.checkpoint())
    m.relocalise_groups(buf[:6], [3, 3], travel=1.1, params=dict(n_rot=8))
    after = (m.grid_i8(), m.counters(), m.checkpoint())
    assert (before[0] == after[0]).all() and before[1] == after[1]
    assert before[2] == after[2], "checkpoint bytes changed"


def test_invalid_arguments_are_refused_with_the_text(pkg, W):
    m, grid, buf = W[:3]
    m.set_sweep_filter(*NEAR)
    call = lambda q=buf[:3], gsize=(3,), **kw: m.relocalise_groups(q, list(gsize), **kw)
    for bad, text in ((dict(radius=8), "radius"), (dict(radius=-1), "radius"), (dict(n_rot=0), "n_rot"), (dict(n_rot=361), "n_rot"),
                      (dict(sep=17), "sep must"), (dict(sep=-1), "sep must"), (dict(n_rot=8, sep_rot=8), "sep_rot"),
                      (dict(sep_rot=-1), "sep_rot"), (dict(min_hits=-1), "min_hits"), (dict(min_percent=101), "min_percent"),
                      (dict(min_margin=101), "min_margin"), (dict(min_margin=-1), "min_margin")):
        with pytest.raises(pkg.QuasarError, match=text):
            call(params=bad)
    for travel in (-0.5, math.nan, math.inf):
        with pytest.raises(pkg.QuasarError, match="travel must be finite and not negative"):
            call(travel=travel)
    for travel, ok in ((4.59, True), (4.7, False)):                # 16 + 2 * (116 + 3) = 254; 16 + 2 * (118 + 3) = 258
        if ok:
            call(travel=travel, params=dict(n_rot=1, sep_rot=0, box=(60, 40, 61, 41)))
        else:
            with pytest.raises(pkg.QuasarError, match=r"smax \+ travel is too large"):
                call(travel=travel)
            with pytest.raises(pkg.QuasarError, match=r"smax \+ travel is too large"):
                call(buf[:0], (), travel=travel)                   # refused whatever n is
    ident = np.repeat(GR.IDENTITY, 3)
    with pytest.raises(pkg.QuasarError, match="sum to n"):
        call(gsize=(2,), rel=ident)
    with pytest.raises(pkg.QuasarError, match="sum to n"):
        call(gsize=(3, 1), rel=ident)
    with pytest.raises(pkg.QuasarError, match=r"gsize\[1\] must lie in \[1, QS_RELOC_MAX_GROUP\]"):
        call(gsize=(3, 0), rel=ident)
    with pytest.raises(pkg.QuasarError, match=r"gsize\[0\] must lie"):
        call(np.ascontiguousarray(np.tile(buf[:1], (17, 1))), (17,), rel=np.repeat(GR.IDENTITY, 17))
    with pytest.raises(pkg.QuasarError, match="stride"):
        call(np.ascontiguousarray(buf[:3, :700]), rel=ident)
    with pytest.raises(ValueError, match="rel must have one entry per record"):
        call(rel=ident[:2])
    with pytest.raises(ValueError, match="group sizes"):
        call(gsize=(2,))
    assert len(call(buf[:0], ())) == 0
    with pkg.QuasarMapper(64, 0.05, 0.0, 0.0, seq_stride=2) as sh:
        with pytest.raises(pkg.QuasarError, match="sharded"):
            sh.relocalise_groups(buf[:3], [3])


class _Sock:
    """A socket whose queued datagrams arrive at the next poll."""

    def __init__(self):
        self.queue = []

    def setblocking(self, flag):
        pass

    def recvfrom_into(self, view, nbytes):
        if not self.queue:
            raise BlockingIOError
        d = self.queue.pop(0)
        view[:len(d)] = d
        return len(d), ("127.0.0.1", 4000)

    def sendto(self, data, addr):
        pass

    def close(self):
        pass


def test_closed_loop_a_lost_bot_under_the_short_filter(pkg, W):
    """Query pose 7 of the noise-free 1.2 m recovery set: the restatement refuses its first sweep alone and accepts the group
    from the third sweep on.  The bot reports poses in a frame of its own (its first pose at (50, 50), off the map: what is ingested before it is
    located changes nothing).  The single-sweep call
    refuses the first sweep; MissionControl(relocalise={"group": 5, ...}), one sweep a poll, locates the bot at the poll the
    restatement says, within a cell and two rotation steps of the truth, and maps the later sweeps from the found frame."""
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    grid = W[1]
    poses, cells = RR.query_poses(grid, GEOM, 24, seed=1)
    true = GR.build_groups(grid, GEOM, poses, 5, 0.8, seed=1)[7]
    rel = GR.rel_of(*true.T)
    own = np.stack([50.0 + rel["tx"], 50.0 + rel["ty"], np.arctan2(rel["s"], rel["c"])], axis=1).astype(np.float32)
    prm = dict(min_hits=20)
    with _painted(pkg, grid, RES, OX, OY) as live:
        live.set_sweep_filter(*NEAR)
        lost = live.sense_sweeps(true, 1, max_range=1.2)
        lost[:, 5:17] = own.view(np.uint8).reshape(5, 12)
        alone = live.relocalise_sweeps(lost[:1], params=prm)[0]
        assert alone["status"] == RR.OK and not alone["accepted"]
        exp = [GR.reloc_groups(grid, GEOM, lost[:k], [k], None, 3.3, prm, None, *NEAR)[0] for k in range(1, 6)]
        at = [bool(e["accepted"]) for e in exp].index(True)
        assert 1 <= at <= 4, "the restatement was meant to accept this group, and not at its first sweep"
        sock = _Sock()
        mc = fe.MissionControl(live, sock=sock, sweeps=True, relocalise=dict(prm, group=5, travel=3.3))
        for k in range(5):
            sock.queue.append(bytes(lost[k]))
            assert mc.poll(now=1.0 + k) == 1
            assert (1 in mc.relocalised) == (k >= at)
        assert mc.reloc_stats == {"tried": 0, "accepted": 1, "rewritten": 5 - at, "group_tried": at + 1, "gave_up": 0}
        found = mc.relocalised[1]
        assert not GR.differing(np.array([found]), np.array([exp[at]]))
        turn = 2 * math.pi / 180
        dyaw = abs((float(found["yaw"]) - float(true[0, 2]) + math.pi) % (2 * math.pi) - math.pi)
        assert abs(found["gx"] - cells[7][0]) <= 1 and abs(found["gy"] - cells[7][1]) <= 1 and dyaw <= 2 * turn
        acc, used = live.last_sweeps()           # the last sweep was cast from the found frame: a cell and two rotation steps on a 3.2 m lever from the truth
        assert acc.tolist() == [1] and math.hypot(used[0, 0] - true[4, 0], used[0, 1] - true[4, 1]) < 0.4
        mc.close()
