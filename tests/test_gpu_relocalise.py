"""Relocalisation on the GPU (qs_relocalise_sweeps and its _device twin).  The bar: the CPU restatement of the rules G1-G9
(tests/reloc_rules.py) fed grid_i8() -- every field of every output with ==, the doubles as bits.  The sweeps are sensed on the
device in the painted world (the sense calls have their own tests), so both sides read the same bytes."""
import importlib
import math

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import maze_scenes as MZ
import reloc_rules as RR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
SIZE, RES, OX, OY = RR.WORLD_GRID
GEOM = (RES, OX, OY)
FAR, NEAR = (0.1, 3.0), (0.1, 1.2)


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
    """The world of tests/reloc_rules.py painted into a mapper, and 12 sweeps sensed in it at 3.0 m: (mapper, grid, sweeps
    uint8 [12, 751], poses, cells)."""
    grid = RR.world()
    m = _painted(pkg, grid, RES, OX, OY)
    poses, cells = RR.query_poses(grid, GEOM, 12, seed=5)
    buf = m.sense_sweeps(poses, 1, max_range=3.0)
    yield m, grid, buf, poses, cells
    m.close()


SMALL_GEOM = (0.05, -1.7, -1.7)


@pytest.fixture(scope="module")
def S(pkg):
    grid = RR.small_world()
    m = _painted(pkg, grid, *SMALL_GEOM)
    cells = np.array([(3, 3), (64, 2), (1, 66), (66, 66), (30, 30), (45, 20)])
    # headings towards the middle of the grid, so that every sweep sees something (33 to 136 hit beams at 3.0 m)
    yaw = np.arctan2(34 - cells[:, 1], 34 - cells[:, 0]) + np.array([0.1, -0.2, 0.3, -0.1, 2.0, 0.4])
    poses = np.stack([SMALL_GEOM[1] + (cells[:, 0] + 0.5) * 0.05, SMALL_GEOM[2] + (cells[:, 1] + 0.5) * 0.05, yaw], axis=1)
    buf = m.sense_sweeps(poses.astype(np.float32), 1, max_range=3.0)
    assert (buf[:, 27:].view("<f4") > 0.1).sum(axis=1).min() >= 30
    yield m, grid, buf
    m.close()


def _check(m, grid, geom, buf, p=None, filt=FAR, lengths=None, expected=None):
    """One host call against the restatement; returns the device's output."""
    m.set_sweep_filter(*filt)
    got = m.relocalise_sweeps(buf, lengths, params=p)
    exp = RR.reloc(grid, geom, buf, p, lengths, *filt) if expected is None else expected
    assert got.dtype == RR.RELOC_DTYPE and len(got) == len(buf)
    bad = RR.differing(got, exp)
    assert not bad, bad
    return got


@pytest.mark.parametrize("filt", [FAR, NEAR], ids=["3.0m", "1.2m"])
def test_sensed_sweeps_equal_the_restatement(W, filt):
    """12 poses, the default parameters; at 3.0 m most are found (the restatement's own recovery is a CPU test), at the default
    1.2 m most sweeps see one wall or nothing and the rival ties: the outputs must agree all the same."""
    m, grid, buf, poses, cells = W
    got = _check(m, grid, GEOM, buf, None, filt)
    assert (got["status"] == RR.OK).all()
    if filt == FAR:                              # (the restatement finds 11 of these 12 and accepts 8)
        found = sum(RR.recovered(got[k], cells[k], poses[k, 2], 180) for k in range(len(buf)))
        assert found >= 9 and got["accepted"].sum() >= 6, (found, got["accepted"].sum())


@pytest.mark.parametrize("n_rot", [1, 8, 180, 360])
def test_rotation_counts(W, n_rot):
    m, grid, buf = W[:3]
    _check(m, grid, GEOM, buf[:3], dict(n_rot=n_rot, sep_rot=min(2, n_rot - 1)))


@pytest.mark.parametrize("radius", [0, 2, 7])
def test_radii(W, radius):
    m, grid, buf = W[:3]
    _check(m, grid, GEOM, buf[3:7], dict(radius=radius, n_rot=45))
    _check(m, grid, GEOM, buf[3:5], dict(radius=radius, n_rot=45), NEAR)


def test_small_world_whose_free_cells_touch_the_border(S):
    """At 3.0 m the patch (142 cells a side) hangs over every edge of the 68-cell grid from every tile."""
    m, grid, buf = S
    _check(m, grid, SMALL_GEOM, buf, dict(n_rot=90))
    _check(m, grid, SMALL_GEOM, buf, dict(n_rot=90), NEAR)


def test_box_edges(S):
    m, grid, buf = S
    size = len(grid)
    boxes = [(-3, -3, 15, 15), (0, 0, 16, 16), (15, 16, 17, size + 5), (16, 15, size + 5, 17), (17, 17, size + 5, size + 5),
             (-3, 0, size + 5, 16), (0, -3, 17, size), (15, 15, 16, 16), (16, 16, 17, 17)]
    for box in boxes:
        got = _check(m, grid, SMALL_GEOM, buf[:3], dict(n_rot=8, box=box))
        x0, y0, x1, y1 = RR.clip_box(box, size)
        ok = got[got["status"] == RR.OK]
        assert len(ok) == 3 and (ok["gx"] >= x0).all() and (ok["gx"] < x1).all() and (ok["gy"] >= y0).all() and (ok["gy"] < y1).all()
    one = _check(m, grid, SMALL_GEOM, buf[:3], dict(n_rot=8, box=(30, 31, 31, 32)))           # a box of one cell
    assert (one["status"] == RR.OK).all() and (one["gx"] == 30).all() and (one["gy"] == 31).all()
    for box in ((20, 40, 21, 44), (8, 10, 40, 11), (30, 30, 30, 40), (40, 40, 30, 30), (size, 0, size + 5, size), (-9, -9, 0, 0)):
        none = _check(m, grid, SMALL_GEOM, buf[:3], dict(n_rot=8, box=box))                  # no FREE cell: walls, empty boxes
        assert (none["status"] == RR.NO_CANDIDATE).all() and (none["gx"] == -1).all()


def test_best_on_a_tile_corner_and_the_exclusion_square(W):
    """A pose in cell (63, 47), the last column and row of its tile: the square round the best covers four tiles at sep 4, one at
    sep 0 and nine at sep 16."""
    m, grid, _, _, _ = W
    pose = np.array([[OX + 63.5 * RES, OY + 47.5 * RES, 0.3]], dtype=np.float32)
    buf = m.sense_sweeps(pose, 1, max_range=3.0)
    for sep in (0, 4, 16):
        got = _check(m, grid, GEOM, buf, dict(sep=sep))
        assert (got["gx"][0], got["gy"][0]) == (63, 47), "the sweep was meant to be found in its own cell"
        assert got["status"][0] == RR.OK and got["gx2"][0] >= 0
        assert max(abs(got["gx2"][0] - 63), abs(got["gy2"][0] - 47)) > sep or \
            min(abs(got["j2"][0] - got["j"][0]), 180 - abs(got["j2"][0] - got["j"][0])) > 2
        # the four tiles round the corner alone: every candidate lies in a re-scored tile, the rival is the EXCL launch's
        near = _check(m, grid, GEOM, buf, dict(sep=sep, box=(48, 32, 80, 64)))
        assert (near["gx"][0], near["gy"][0], near["j"][0]) == (63, 47, got["j"][0]) and 48 <= near["gx2"][0] < 80


def test_twins_across_the_rotation_wrap(pkg, P):
    """One beam, one candidate cell, OCCUPIED cells where the beam ends at j = 0 and at j = 7 of 8: the best is j = 0 and its
    twin is j = 7, at circular distance 1 -- the rival with sep_rot 0, excluded with sep_rot 1."""
    g = np.zeros((68, 68), dtype=np.int8)
    g[30, 40] = 100                              # (30, 30) + (10, 0)
    g[23, 37] = 100                              # (30, 30) + (7, -7): the beam turned by -45 degrees
    r = np.zeros((1, 181), dtype=np.float32)
    r[0, 90] = 0.5
    buf = P.pack_sweeps([1], [0.0], [0.0], [0.0], r)
    m = _painted(pkg, g, *SMALL_GEOM)
    try:
        prm = dict(radius=0, n_rot=8, sep=2, min_hits=1, box=(30, 30, 31, 31))
        a = _check(m, g, SMALL_GEOM, buf, dict(prm, sep_rot=0))
        assert (a["j"][0], a["score"][0], a["j2"][0], a["score2"][0], a["accepted"][0]) == (0, 1, 7, 1, 0)
        b = _check(m, g, SMALL_GEOM, buf, dict(prm, sep_rot=1))
        assert (b["j"][0], b["score"][0], b["j2"][0], b["score2"][0], b["accepted"][0]) == (0, 1, 2, 0, 1)
        c = _check(m, g, SMALL_GEOM, buf, dict(prm, sep_rot=7))                               # every rotation is near: no rival
        assert (c["j2"][0], c["gx2"][0], c["gy2"][0], c["score2"][0]) == (-1, -1, -1, 0)
    finally:
        m.close()


def test_broken_and_empty_records(W, P):
    m, grid, buf = W[:3]
    for odometry in (True, False):
        q = buf[:8].copy() if odometry else np.ascontiguousarray(np.delete(buf[:8], np.s_[17:25], axis=1))
        off = 27 if odometry else 19
        lens = np.full(len(q), q.shape[1], dtype=np.uint16)
        q[1, 0] = ord("X")                       # magic
        q[2, 4] = 3                              # agent beyond max_agent
        q[3, 4] = 0
        lens[4] = q.shape[1] - 1                 # a wrong length
        q[5, off:] = 0                           # an all-zero sweep: accepted, H = 0
        q[6, off:off + 4 * 60] = np.frombuffer(np.full(60, np.nan, dtype="<f4").tobytes(), dtype=np.uint8)
        q[7, 5:17] = np.frombuffer(np.array([np.nan, np.inf, 1e30], dtype="<f4").tobytes(), dtype=np.uint8)   # the pose is not read
        got = _check(m, grid, GEOM, q, dict(n_rot=45), FAR, lens)
        assert got["status"].tolist() == [RR.OK, RR.NO_RECORD, RR.NO_RECORD, RR.NO_RECORD, RR.NO_RECORD, RR.NO_CANDIDATE, RR.OK, RR.OK]
        assert got[1].tobytes() == bytes([0] * 36 + [RR.NO_RECORD] + [0] * 35)
        assert got["hits"][5] == 0 and got["accepted_record"][5] == 1 and got["hits"][6] <= 121


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_record_counts_and_one_more_than_a_chunk(W, n):
    """65 is one sweep more than the 64 a launch takes.  The 12 sensed sweeps in turn; the restatement runs on those 12."""
    m, grid, buf = W[:3]
    p = dict(n_rot=8, box=(16, 20, 130, 110))
    idx = np.arange(n) % len(buf)
    base = RR.reloc(grid, GEOM, buf, p, None, *FAR)
    _check(m, grid, GEOM, np.ascontiguousarray(buf[idx]), p, FAR, expected=base[idx])


def test_host_call_and_device_twin_give_the_same_bytes(W):
    m, grid, buf = W[:3]
    m.set_sweep_filter(*FAR)
    q = np.ascontiguousarray(np.concatenate([buf, buf[:5]]))
    lens = np.full(len(q), q.shape[1], dtype=np.uint16)
    lens[3] = 7
    p = dict(n_rot=24)
    host = m.relocalise_sweeps(q, lens, params=p)
    dev = torch.device("cuda", 0)
    dq, dl = torch.from_numpy(q).to(dev), torch.from_numpy(lens.view(np.int16)).to(dev)
    d_out = torch.full((len(q) * RR.RELOC_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    m.relocalise_sweeps_device(dq.data_ptr(), len(q), q.shape[1], d_out.data_ptr(), d_lens=dl.data_ptr(), params=p)
    m.sync()
    assert d_out.cpu().numpy().tobytes() == host.tobytes()
    assert host["status"][3] == RR.NO_RECORD


def test_a_call_leaves_the_context_unchanged(W):
    m, grid, buf = W[:3]
    m.set_sweep_filter(*FAR)
    before = (m.grid_i8(), m.counters(), m.checkpoint())
    m.relocalise_sweeps(buf[:2], params=dict(n_rot=8))
    after = (m.grid_i8(), m.counters(), m.checkpoint())
    assert (before[0] == after[0]).all() and before[1] == after[1]
    assert before[2] == after[2], "checkpoint bytes changed"


def test_invalid_arguments_are_refused_with_the_text(pkg, W):
    m, grid, buf = W[:3]
    m.set_sweep_filter(*FAR)
    for bad, text in ((dict(radius=8), "radius"), (dict(radius=-1), "radius"), (dict(n_rot=0), "n_rot"), (dict(n_rot=361), "n_rot"),
                      (dict(sep=17), "sep must"), (dict(sep=-1), "sep must"), (dict(n_rot=8, sep_rot=8), "sep_rot"),
                      (dict(sep_rot=-1), "sep_rot"), (dict(min_hits=-1), "min_hits"), (dict(min_percent=101), "min_percent"),
                      (dict(min_margin=101), "min_margin"), (dict(min_margin=-1), "min_margin")):
        with pytest.raises(pkg.QuasarError, match=text):
            m.relocalise_sweeps(buf[:1], params=bad)
    with pytest.raises(pkg.QuasarError, match="stride"):
        m.relocalise_sweeps(np.ascontiguousarray(buf[:1, :700]))
    m.set_sweep_filter(0.1, 6.0)                 # 16 + 2 * (120 + 2 + 1) = 262
    try:
        with pytest.raises(pkg.QuasarError, match="smax is too large"):
            m.relocalise_sweeps(buf[:1])
        with pytest.raises(pkg.QuasarError, match="smax is too large"):
            m.relocalise_sweeps(buf[:0])         # refused whatever n is
    finally:
        m.set_sweep_filter(*FAR)
    assert len(m.relocalise_sweeps(buf[:0])) == 0
    with pkg.QuasarMapper(64, 0.05, 0.0, 0.0, seq_stride=2) as sh:
        with pytest.raises(pkg.QuasarError, match="sharded"):
            sh.relocalise_sweeps(buf[:1])


def test_an_empty_map_scores_nothing_and_accepts_nothing(pkg, W):
    buf = W[2]
    with pkg.QuasarMapper(68, *SMALL_GEOM) as m:
        m.set_sweep_filter(*FAR)
        got = m.relocalise_sweeps(buf[:2], params=dict(n_rot=8))
        assert (got["status"] == RR.NO_CANDIDATE).all()                       # no FREE cell at all
        MZ.paint(m, RR.paint_rays(np.zeros((68, 68), dtype=np.int8)), *SMALL_GEOM)
        got = _check(m, np.zeros((68, 68), dtype=np.int8), SMALL_GEOM, buf[:2], dict(n_rot=8))
        assert (got["status"] == RR.OK).all() and (got["score"] == 0).all() and (got["accepted"] == 0).all()
        assert (got["gx"] == 0).all() and (got["gy"] == 0).all() and (got["j"] == 0).all()


class _Sock:
    """A socket whose queued datagrams arrive at the next poll."""

    def __init__(self, datagrams):
        self.queue = list(datagrams)

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


def test_closed_loop_lost_bots_are_mapped_where_they_are(pkg, W):
    """Two bots stand at query poses 1 and 3 of the world and send two noisy sweeps each with their pose fields zeroed.  A
    MissionControl(relocalise=True) finds both (the restatement accepts both first sweeps, within a cell and a rotation step
    of the truth) and maps all four sweeps from the found poses: its grid equals, cell for cell, the grid of a plain ingest
    of the same sweeps carrying the poses the restatement finds."""
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    _, grid, _, poses, cells = W
    who = [1, 3, 1, 3]
    with _painted(pkg, grid, RES, OX, OY) as live, _painted(pkg, grid, RES, OX, OY) as ref:
        for m in (live, ref):
            m.set_sweep_filter(*FAR)
        sensed = live.sense_sweeps(poses[who], [1, 2, 1, 2], max_range=3.0, noise_amp=0.01, seed=7)
        lost = sensed.copy()
        lost[:, 5:17] = 0
        exp = RR.reloc(grid, GEOM, lost[:2], None, None, *FAR)
        for k in (0, 1):
            assert exp["accepted"][k] and RR.recovered(exp[k], cells[who[k]], poses[who[k], 2], 180)
        mc = fe.MissionControl(live, sock=_Sock(bytes(r) for r in lost), sweeps=True, relocalise=True)
        assert mc.poll(now=1.0) == 4
        assert mc.reloc_stats == {"tried": 2, "accepted": 2, "rewritten": 4} and set(mc.relocalised) == {1, 2}
        for bot in (1, 2):
            assert not RR.differing(np.array([mc.relocalised[bot]]), exp[bot - 1:bot])
        assert mc.bot_pose[1] == (float(np.float32(exp["x"][0])), float(np.float32(exp["y"][0])))
        told = sensed.copy()
        told[:, 5:17] = np.stack([exp[f][[0, 1, 0, 1]] for f in ("x", "y", "yaw")], axis=1).astype("<f4").view(np.uint8)
        ref.ingest_sweeps(told)
        a, b = live.grid_i8(), ref.grid_i8()
        assert (a == b).all(), f"{(a != b).sum()} cells differ"
        acc, used = live.last_sweeps()           # all four were cast, from the found poses
        assert acc.tolist() == [1, 1, 1, 1] and (used == told[:, 5:17].copy().view("<f4").astype(np.float64)).all()
        mc.close()
