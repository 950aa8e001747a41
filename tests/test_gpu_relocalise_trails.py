"""Trail relocalisation on the GPU (qs_relocalise_trails and its _device twin).  The bar: the CPU restatement of the rules K1-K8
(tests/trail_reloc_rules.py) fed grid_i8() and the (sin, cos) the device reports -- every field of every qs_trail_reloc with ==
on the bytes -- and those (sin, cos) within one ulp of libm.  The worlds are those of tests/reloc_rules.py, painted as
tests/test_gpu_relocalise.py paints them; the trust filter is (0.05, 3.0] m."""
import importlib
import math

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import maze_scenes as MZ
import reloc_rules as RR
import trail_reloc_rules as KR
import trail_rules as TR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
SIZE, RES, OX, OY = RR.WORLD_GRID
GEOM = (RES, OX, OY)
SMALL_GEOM = (0.05, -1.7, -1.7)
MIN_DIST, MAX_DIST = 0.05, 3.0
FAR_TRAVEL = 2.8                                 # K8 at 5 cm cells and 3.0 m: ceil(5.8 / 0.05) = 116, a patch of 254 cells


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _painted(pkg, grid, res, ox, oy, **kw):
    m = pkg.QuasarMapper(len(grid), res, ox, oy, min_dist=MIN_DIST, max_dist=MAX_DIST, **kw)
    MZ.paint(m, RR.paint_rays(grid), res, ox, oy)
    assert (m.grid_i8() == grid).all()
    return m


@pytest.fixture(scope="module")
def W(pkg):
    """The 192-cell world painted into a mapper and 4 trails of 64 packets driven through it, each in a frame of its own."""
    grid = RR.world()
    m = _painted(pkg, grid, RES, OX, OY)
    yield m, grid, KR.world_trails(grid, GEOM, seed=7, n=4, K=64, far=MAX_DIST)
    m.close()


@pytest.fixture(scope="module")
def S(pkg):
    """The 68-cell world, whose free cells touch the grid's border."""
    grid = RR.small_world()
    m = _painted(pkg, grid, *SMALL_GEOM)
    yield m, grid
    m.close()


def _dense(K, seed, agent=1):
    """K packets at small poses (within 0.57 m of one another: inside a travel of 0.6 m) whose four ranges all hit (0.3 to
    1.1 m): H = 4 K."""
    rng = np.random.default_rng(seed)
    return TR.pack(np.full(K, agent), rng.uniform(-0.2, 0.2, K), rng.uniform(-0.2, 0.2, K), rng.uniform(-math.pi, math.pi, K),
                   rng.uniform(0.3, 1.1, (K, 4)))


def _pad(buf, stride):
    out = np.zeros((len(buf), stride), dtype=np.uint8)
    out[:, :min(stride, buf.shape[1])] = buf[:, :stride]
    return out


def _check(m, grid, geom, buf, gsize, p=None, travel=0.6, lengths=None, tag=""):
    """One host call against the restatement fed the device's rot_out; returns the device's output."""
    dev, rot = m.relocalise_trails(buf, gsize, lengths, travel=travel, params=p, rotations=True)
    exp, exp_rot = KR.reloc_trails(grid, geom, buf, gsize, p, travel, lengths, rot=rot, min_dist=MIN_DIST, max_dist=MAX_DIST,
                                   max_agent=m.max_agent)
    assert dev.dtype == KR.TRAIL_RELOC_DTYPE and len(dev) == len(gsize)
    bad = KR.differing(dev, exp)
    assert not bad, f"{tag}: {bad}"
    assert dev.tobytes() == exp.tobytes(), f"{tag}: bytes differ"
    assert (rot == exp_rot).all(), f"{tag}: rot_out is not zero where no record counts"
    lib = TR.rot_libm(buf, lengths, m.max_agent)
    used = (exp_rot != 0).any(axis=1)
    assert (np.abs(rot[used] - lib[used]) <= np.spacing(np.abs(lib[used]))).all(), f"{tag}: rot_out beyond one ulp of libm"
    assert m.relocalise_trails(buf, gsize, lengths, travel=travel, params=p).tobytes() == dev.tobytes(), f"{tag}: rot_out NULL differs"
    return dev


# ---- trail sizes and counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 63, 64])
def test_trails_of_every_size_equal_the_restatement(S, K):
    """A lane per record: one lane, half a wave and its neighbours, the whole wave; 64 records of four hits fill the list."""
    m, grid = S
    buf = np.concatenate([_dense(K, seed=K), _dense(K, seed=100 + K)])
    dev = _check(m, grid, SMALL_GEOM, buf, [K, K], dict(n_rot=8, min_hits=1), tag=f"K {K}")
    assert (dev["hits"] == 4 * K).all() and (dev["records"] == K).all() and (dev["anchor"] == K - 1).all() and (dev["status"] == KR.OK).all()


def test_driven_trails_at_the_reach_limit(W):
    """64 packets driven through the world at the largest reach K8 admits, and their last 33 and 17."""
    m, grid, T = W
    pk = T["pkts"].reshape(4, 64, 42)
    buf = np.concatenate([pk[0], pk[1, 31:], pk[2, 47:], pk[3]])
    c = T["true"][0, -1]
    gx, gy = int((c[0] - OX) / RES), int((c[1] - OY) / RES)
    dev = _check(m, grid, GEOM, buf, [64, 33, 17, 64], dict(n_rot=24, box=(gx - 20, gy - 20, gx + 20, gy + 20)), FAR_TRAVEL, tag="driven")
    assert (dev["status"] == KR.OK).all() and dev["records"][0] >= 50


@pytest.mark.parametrize("n", [0, 65])
def test_no_trail_and_one_more_than_a_launch(S, n):
    """65 trails of 1, 2 and 3 records: the second launch takes the last, whose first record is the 129th."""
    m, grid = S
    sizes = ([1, 2, 3] * 22)[:n]
    buf = _dense(sum(sizes), seed=4) if n else np.zeros((0, 42), np.uint8)
    p = dict(n_rot=4, sep_rot=1, min_hits=1, box=(20, 20, 44, 44))
    dev = _check(m, grid, SMALL_GEOM, buf, sizes, p, tag=f"{n} trails")
    assert len(dev) == n
    if n:
        assert (dev["anchor"] == np.array(sizes) - 1).all() and len(set(dev["ax"].tolist())) > 60
        d_pk = torch.from_numpy(buf.reshape(-1)).cuda()
        d_out = torch.full((n * 88,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m.relocalise_trails_device(d_pk.data_ptr(), len(buf), 42, sizes, d_out.data_ptr(), travel=0.6, params=p)
        m.sync()
        assert d_out.cpu().numpy().tobytes() == dev.tobytes()
    else:
        out, rot = m.relocalise_trails(buf, [], travel=0.6, rotations=True)
        assert len(out) == 0 and rot.shape == (0, 2)
        m.relocalise_trails_device(0, 0, 42, [], 0, travel=0.6)


# ---- parameters ------------------------------------------------------------------------------------------------------------------------
PARAMS = [("n_rot 1", dict(n_rot=1, sep_rot=0)), ("n_rot 7", dict(n_rot=7)), ("n_rot 180", dict(n_rot=180)), ("n_rot 360", dict(n_rot=360)),
          ("radius 0", dict(radius=0, n_rot=12)), ("radius 7", dict(radius=7, n_rot=12)), ("sep 0", dict(sep=0, n_rot=12)),
          ("sep 16", dict(sep=16, n_rot=12)), ("defaults", None)]


@pytest.mark.parametrize("tag,p", PARAMS, ids=[c[0] for c in PARAMS])
def test_parameters_equal_the_restatement(S, tag, p):
    """7 rotations: the second round has three live waves of four."""
    m, grid = S
    buf = np.concatenate([_dense(20, seed=1), _dense(7, seed=2)])
    dev = _check(m, grid, SMALL_GEOM, buf, [20, 7], p and dict(p, min_hits=10), tag=tag)
    assert (dev["status"] == KR.OK).all()


def test_boxes_tile_corners_and_the_grid_edge(S):
    """Boxes clipped to one tile, of one cell at a tile's corner and in the grid's corners (the patch hangs off the grid), and
    boxes with no FREE cell.  A box of two cells in adjacent tiles with sep 0 and every rotation excluded: the rival is the other
    cell, found by the nine-tile re-score."""
    m, grid = S
    size = len(grid)
    buf = _dense(20, seed=3)
    for box in ((-3, -3, 15, 15), (0, 0, 16, 16), (15, 15, 16, 16), (16, 16, 17, 17), (0, 0, 1, 1), (67, 67, 68, 68), (67, 0, size + 5, 1),
                (63, 47, 64, 48)):
        dev = _check(m, grid, SMALL_GEOM, buf, [20], dict(n_rot=8, min_hits=1, box=box), tag=f"box {box}")
        x0, y0, x1, y1 = RR.clip_box(box, size)
        assert dev["status"][0] == KR.OK and x0 <= dev["gx"][0] < x1 and y0 <= dev["gy"][0] < y1
    for box in ((20, 40, 21, 44), (30, 30, 30, 40), (size, 0, size + 5, size)):
        dev = _check(m, grid, SMALL_GEOM, buf, [20], dict(n_rot=8, box=box), tag=f"box {box}")
        assert (dev["status"][0], dev["records"][0], dev["hits"][0], dev["anchor"][0], dev["agent"][0]) == (KR.NO_CANDIDATE, 20, 80, 19, 1)
    for box in ((15, 5, 17, 6), (5, 15, 6, 17)):
        dev = _check(m, grid, SMALL_GEOM, buf, [20], dict(n_rot=8, sep=0, sep_rot=7, min_hits=1, box=box), tag=f"box {box}")
        cells = {(int(dev["gx"][0]), int(dev["gy"][0])), (int(dev["gx2"][0]), int(dev["gy2"][0]))}
        assert cells == {(box[0], box[1]), (box[2] - 1, box[3] - 1)}


# ---- records ------------------------------------------------------------------------------------------------------------------------------
def test_record_level_cases(S):
    """A rejected anchor, mixed agents, every record broken, a trail that sees nothing, ranges that are not numbers, and travel:
    at equality, one ulp under, and zero."""
    m, grid = S
    a = _dense(12, seed=5)
    a[11, 0] = ord("X"); a[3, 4] = 2; a[5, 4] = 9                  # anchor 10; another bot's; beyond max_agent
    b = _dense(6, seed=6)
    b[:, 0] = 0                                                    # no record at all
    c = _dense(6, seed=7)
    c[:, 25:41] = 0                                                # H = 0
    d = TR.pack([1, 1], [0.0, 0.0], [0.0, 0.0], [0.0, 1.0], [[math.nan, math.inf, -math.inf, 1.0], [3.0, 0.04, 3.01, -1.0]])
    e = _dense(5, seed=8)
    lens = np.full(12 + 6 + 6 + 2 + 5, 42, dtype=np.uint16)
    lens[26] = 41; lens[27] = 40; lens[28] = 43                    # 41 is a packet; 40 and 43 are not
    buf = np.concatenate([a, b, c, d, e])
    dev = _check(m, grid, SMALL_GEOM, buf, [12, 6, 6, 2, 5], dict(n_rot=8, min_hits=1), lengths=lens, tag="records")
    assert dev["anchor"].tolist() == [10, -1, 5, 1, 4] and dev["records"].tolist() == [9, 0, 6, 2, 3]
    assert dev["status"].tolist() == [KR.OK, KR.NO_RECORD, KR.NO_CANDIDATE, KR.OK, KR.OK] and dev["hits"].tolist() == [36, 0, 0, 2, 12]
    assert dev[1].tobytes() == bytes([0] * 36 + [KR.NO_RECORD] + [0] * 7 + [255] * 4 + [0] * 40)
    f = TR.pack([1, 1, 1], [0.75, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.3, 0.0], [[1.0, 0, 0, 0]] * 3)        # 0.75^2 + 1 = 1.25^2
    for travel, records in ((1.25, 3), (math.nextafter(1.25, 0.0), 2), (0.0, 2)):
        dev = _check(m, grid, SMALL_GEOM, f, [3], dict(n_rot=8, min_hits=1), travel, tag=f"travel {travel}")
        assert dev["records"][0] == records
    mixed = np.concatenate([_dense(4, seed=9, agent=2), _dense(4, seed=10, agent=1), _dense(1, seed=11, agent=2)])
    dev = _check(m, grid, SMALL_GEOM, mixed, [9], dict(n_rot=8, min_hits=1), tag="bot 2")
    assert (dev["agent"][0], dev["records"][0], dev["anchor"][0]) == (2, 5, 8)


def test_offset_drift_and_a_common_shift_do_not_matter(pkg):
    """The bot's offset is not read, and a shift of every record that is exact in f32 changes ax and ay alone."""
    grid = RR.small_world()
    rng = np.random.default_rng(13)
    K = 16
    x, y = rng.integers(-200, 200, K) / 1024.0, rng.integers(-200, 200, K) / 1024.0
    yaw, d = rng.uniform(-3, 3, K), rng.uniform(0.3, 1.1, (K, 4))
    p = dict(n_rot=8, min_hits=1)
    with _painted(pkg, grid, *SMALL_GEOM, separation=0.75) as m:
        base = _check(m, grid, SMALL_GEOM, TR.pack([2] * K, x, y, yaw, d), [K], p, tag="bot 2, separation 0.75")
        m.set_bot_offset(2, -3.5)
        again = _check(m, grid, SMALL_GEOM, TR.pack([2] * K, x, y, yaw, d), [K], p, tag="bot 2, offset -3.5")
        assert again.tobytes() == base.tobytes() and base["status"][0] == KR.OK and base["hits"][0] == 4 * K
        moved = _check(m, grid, SMALL_GEOM, TR.pack([2] * K, x + 64.0, y - 32.0, yaw, d), [K], p, tag="shifted")
        assert (moved["ax"][0], moved["ay"][0]) == (base["ax"][0] + 64.0, base["ay"][0] - 32.0)
        moved["ax"], moved["ay"] = base["ax"], base["ay"]
        assert moved.tobytes() == base.tobytes()


# ---- limits and refusals ---------------------------------------------------------------------------------------------------------------------
def test_the_largest_reach_and_every_refusal(pkg, S):
    m, grid = S
    buf = _dense(3, seed=12)
    call = lambda q=buf, gsize=(3,), travel=0.6, **kw: m.relocalise_trails(q, list(gsize), travel=travel, **kw)
    assert 16 + 2 * (math.ceil((MAX_DIST + FAR_TRAVEL) / 0.05) + 2 + 1) == 254
    far = TR.pack([1, 1], [-FAR_TRAVEL, 0.0], [0.0, 0.0], [math.pi, 0.0], [[2.99, 0, 0, 0], [2.99, 2.99, 2.99, 2.99]])
    dev = _check(m, grid, SMALL_GEOM, far, [2], dict(n_rot=4, sep_rot=1, min_hits=1), FAR_TRAVEL, tag="the largest reach")
    assert (dev["records"][0], dev["hits"][0]) == (2, 5)           # a point 5.79 m west of the anchor: 116 cells
    for travel in (2.85, 4.0):
        with pytest.raises(pkg.QuasarError, match=r"max_dist \+ travel is too large"):
            call(travel=travel)
        with pytest.raises(pkg.QuasarError, match=r"max_dist \+ travel is too large"):
            call(buf[:0], (), travel=travel)                       # refused whatever n is
    with pytest.raises(pkg.QuasarError, match=r"max_dist \+ travel is too large"):
        call(travel=FAR_TRAVEL, params=dict(radius=3))
    for bad, text in ((dict(n_rot=0), "n_rot"), (dict(n_rot=361), "n_rot"), (dict(radius=8), "radius"), (dict(sep=17), "sep must"),
                      (dict(n_rot=8, sep_rot=8), "sep_rot"), (dict(min_hits=-1), "min_hits"), (dict(min_percent=101), "min_percent"),
                      (dict(min_margin=-1), "min_margin")):
        with pytest.raises(pkg.QuasarError, match=text):
            call(params=bad)
    for travel in (-0.5, math.nan, math.inf):
        with pytest.raises(pkg.QuasarError, match="travel must be finite and not negative"):
            call(travel=travel)
    with pytest.raises(pkg.QuasarError, match="sum to n"):
        call(gsize=(2,))
    with pytest.raises(pkg.QuasarError, match=r"gsize\[1\] must lie in \[1, QS_TRAIL_MAX_RECORDS\]"):
        call(gsize=(3, 0))
    with pytest.raises(pkg.QuasarError, match=r"gsize\[0\] must lie"):
        call(_dense(65, seed=1), (65,))
    with pytest.raises(pkg.QuasarError, match="stride must be at least 41"):
        call(np.ascontiguousarray(buf[:, :40]))
    with pkg.QuasarMapper(64, 0.05, 0.0, 0.0, seq_stride=2) as sh:
        with pytest.raises(pkg.QuasarError, match="sharded"):
            sh.relocalise_trails(buf, [3])


# ---- strides, alignment, the two entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [41, 42, 48, 64, 100])
def test_strides_and_device_buffers_at_every_misalignment(S, stride):
    """Strides up to 64 are staged through LDS, 100 is read per lane; the device buffers start at byte offsets 0 to 3 and end
    with their last record."""
    m, grid = S
    gsize = [64, 1, 33]
    buf = _pad(np.concatenate([_dense(64, seed=20), _dense(1, seed=21), _dense(33, seed=22)]), stride)
    lens = np.full(len(buf), min(stride, 42), dtype=np.uint16)
    lens[70] = 7
    p = dict(n_rot=8, min_hits=1, box=(16, 16, 52, 52))
    host = _check(m, grid, SMALL_GEOM, buf, gsize, p, lengths=lens, tag=f"stride {stride}")
    _, host_rot = m.relocalise_trails(buf, gsize, lens, travel=0.6, params=p, rotations=True)
    d_lens = torch.from_numpy(lens.view(np.int16)).cuda()
    for mis in range(4):
        d_q = torch.zeros(mis + buf.size, dtype=torch.uint8, device="cuda")
        d_q[mis:] = torch.from_numpy(buf.reshape(-1)).cuda()
        d_out = torch.full((len(gsize) * 88,), 0xAB, dtype=torch.uint8, device="cuda")
        d_rot = torch.full((len(buf), 2), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        m.relocalise_trails_device(d_q.data_ptr() + mis, len(buf), stride, gsize, d_out.data_ptr(), d_lens=d_lens.data_ptr(),
                                   d_rot=d_rot.data_ptr(), travel=0.6, params=p)
        m.sync()
        assert d_out.cpu().numpy().tobytes() == host.tobytes(), (stride, mis)
        assert d_rot.cpu().numpy().tobytes() == host_rot.tobytes(), (stride, mis)


# ---- the context ------------------------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_the_context_unchanged(W):
    m, grid, T = W
    before = (m.grid_i8(), m.counters(), m.checkpoint())
    m.relocalise_trails(T["pkts"][:64], [64], travel=1.0, params=dict(n_rot=8))
    after = (m.grid_i8(), m.counters(), m.checkpoint())
    assert (before[0] == after[0]).all() and before[1] == after[1]
    assert before[2] == after[2], "checkpoint bytes changed"


def test_the_query_sees_the_map_as_it_stands(pkg):
    """After update_rays, after packets were mapped, after a restore and after a reset (no FREE cell left)."""
    grid = RR.small_world()
    buf = _dense(20, seed=30)
    p = dict(n_rot=8, min_hits=1)
    with _painted(pkg, grid, *SMALL_GEOM) as m:
        first = _check(m, grid, SMALL_GEOM, buf, [20], p, tag="painted")
        saved = m.checkpoint()
        wall = np.array([(30, y, 30, y, 1) for y in range(20, 36)], dtype=np.int64)
        MZ.paint(m, wall, *SMALL_GEOM)
        g2 = m.grid_i8()
        assert (g2 != grid).any()
        second = _check(m, g2, SMALL_GEOM, buf, [20], p, tag="after update_rays")
        m.ingest_array(TR.pack([1] * 8, np.linspace(-1.0, 1.0, 8), np.full(8, 0.9), np.zeros(8), np.full((8, 4), 0.4)))
        g3 = m.grid_i8()
        assert (g3 != g2).any()
        _check(m, g3, SMALL_GEOM, buf, [20], p, tag="after packets")
        m.restore(saved)
        assert (m.grid_i8() == grid).all()
        again = _check(m, grid, SMALL_GEOM, buf, [20], p, tag="after a restore")
        assert again.tobytes() == first.tobytes() and second.tobytes() != first.tobytes()
        m.reset()
        gone = _check(m, m.grid_i8(), SMALL_GEOM, buf, [20], p, tag="after a reset")
        assert (gone["status"][0], gone["records"][0], gone["hits"][0]) == (KR.NO_CANDIDATE, 20, 80)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_a_lost_bot_is_found_and_its_poses_moved(W, P):
    """64 packets sensed on the device along a drive through the world, reported in a frame turned by 137 degrees and shifted by
    (7.3, -4.1) m.  The anchor is found within one cell and the frame's turn within two rotation steps; moved by
    protocol.trail_reloc_move, every heading lies within two steps of the truth and every pose within one cell plus what
    two steps make on its lever to the anchor (plus a cell for the anchor's own place inside its cell)."""
    m, grid, _ = W
    true = KR.drive(grid, GEOM, np.random.default_rng(41), 64).astype(np.float32).astype(np.float64)
    pk = m.sense_packets(true.astype(np.float32), 1, max_range=MAX_DIST)
    phi, shift = math.radians(137.0), (7.3, -4.1)
    rep = KR.reported(true, phi, shift)
    pk[:, 5:17] = rep.astype(np.float32).view(np.uint8).reshape(64, 12)
    dev = _check(m, grid, GEOM, pk, [64], None, FAR_TRAVEL, tag="end to end")[0]
    step = 2 * math.pi / 180
    assert dev["status"] == KR.OK and KR.recovered(dev, true[-1], phi, GEOM, 180)
    x, y, yaw = P.trail_reloc_move(dev, rep[:, 0], rep[:, 1], rep[:, 2])
    lever = np.hypot(true[:, 0] - true[-1, 0], true[:, 1] - true[-1, 1])
    assert (np.abs((yaw - true[:, 2] + math.pi) % (2 * math.pi) - math.pi) <= 2 * step + 1e-6).all()
    assert (np.hypot(x - true[:, 0], y - true[:, 1]) <= math.hypot(2 * RES, 2 * RES) + lever * 2 * step).all()
    assert abs(math.floor((x[-1] - OX) / RES) - math.floor((true[-1, 0] - OX) / RES)) <= 1
    assert abs(math.floor((y[-1] - OY) / RES) - math.floor((true[-1, 1] - OY) / RES)) <= 1
