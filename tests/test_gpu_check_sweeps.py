"""The sweep check on the GPU (qs_check_sweeps*, qs_ingest_sweeps_checked*, qs_last_sweep_checks).  The bar: the CPU restatement of
the rules V1-V9 (tests/check_rules.py) fed grid_i8() and the (sin_yaw, cos_yaw) the device reports -- every field of every
qs_sweep_check and every class byte with ==, the reported pair within one ulp of libm's -- and for the guarded ingest a plain ingest,
into a second context, of the same records with the withheld ones made unacceptable: the two checkpoints byte for byte."""
import importlib
import math
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import check_rules as CR
import match_rules as MR
import maze_scenes as MZ
import reloc_rules as RR
from conftest import GOLDEN, load_pkg
from test_gpu_sense import _scene

pytestmark = pytest.mark.gpu
NEAR, FAR = (0.02, 1.2), (0.02, 3.0)
HOST_CHUNK = 4096                                    # CK_HOST_CHUNK of csrc/check.hip


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _painted(pkg, grid, res, ox, oy, **kw):
    m = pkg.QuasarMapper(len(grid), res, ox, oy, **kw)
    MZ.paint(m, RR.paint_rays(grid), res, ox, oy)
    assert (m.grid_i8() == grid).all()
    return m


@pytest.fixture(scope="module")
def worlds(pkg):
    """{size: (mapper, grid)}: the scenes painted at 68 (the second tile is 4 cells wide) and at 200, and the 192 three-room world."""
    out = {}
    for size, seed in ((68, 5), (200, 11)):
        grid, rays, res, ox, oy = _scene(size, seed)
        m = pkg.QuasarMapper(size, res, ox, oy)
        MZ.paint(m, rays, res, ox, oy)
        assert (m.grid_i8() == grid).all()
        out[size] = (m, grid)
    grid = RR.world()
    out[192] = (_painted(pkg, grid, *RR.WORLD_GRID[1:]), grid)
    yield out
    for m, _ in out.values():
        m.close()


def _geom(m):
    return (m.res, m.ox, m.oy)


def _poses(m, grid, n, seed, margin=0.3):
    """n float32 poses: the four corners, the four edge middles, a cell just outside each corner, one on an OCCUPIED cell, then
    random ones over the grid and a margin round it."""
    rng = np.random.default_rng(seed)
    lo, hi = m.ox - margin, m.ox + m.size * m.res + margin
    p = np.stack([rng.uniform(lo, hi, n), rng.uniform(lo, hi, n), rng.uniform(-math.pi, math.pi, n)], axis=1)
    a, b, c = m.ox + 0.5 * m.res, m.ox + (m.size / 2 + 0.37) * m.res, m.ox + (m.size - 0.5) * m.res
    fixed = [(a, a), (c, a), (a, c), (c, c), (b, a), (b, c), (a, b), (c, b), (a - m.res, a - m.res), (c + m.res, c + m.res)]
    oy_, ox_ = np.argwhere(grid == 100)[len(np.argwhere(grid == 100)) // 2]
    fixed.append((m.ox + (ox_ + 0.5) * m.res, m.oy + (oy_ + 0.5) * m.res))
    for j, (x, y) in enumerate(fixed[:n]):
        p[j, :2] = (x, y)
    return p.astype(np.float32)


def _sweeps(P, m, poses, smax, seed, odometry=True, agent=1):
    """Records for the poses: sensed from the map (so that the true ones agree), every third one displaced by up to 0.4 m and 0.3
    rad, every fourth one with a fifth of its ranges replaced by values round the filter's ends, zeros, NaN and negatives."""
    rng = np.random.default_rng(seed)
    n = len(poses)
    buf = m.sense_sweeps(poses, np.broadcast_to(np.asarray(agent, dtype=np.uint8), (n,)), odometry=odometry, max_range=smax,
                         noise_amp=0.02, seed=seed)
    rec = MR.records_of(buf)
    for k in range(0, n, 3):
        rec["x"][k] += np.float32(rng.uniform(-0.4, 0.4))
        rec["y"][k] += np.float32(rng.uniform(-0.4, 0.4))
        rec["yaw"][k] += np.float32(rng.uniform(-0.3, 0.3))
    odd = np.array([0.0, np.nan, -1.0, smax, np.nextafter(np.float32(smax), np.float32(np.inf)), 0.02, 0.021, 0.3, np.inf], dtype=np.float32)
    for k in range(1, n, 4):
        sel = rng.random(181) < 0.2
        rec["ranges"][k][sel] = rng.choice(odd, int(sel.sum()))
    return buf


def _ulp_ok(dev, pose_yaw):
    ref = np.array([[math.sin(y), math.cos(y)] for y in pose_yaw]).reshape(-1, 2)
    got = np.stack([dev["sin_yaw"], dev["cos_yaw"]], axis=1)
    return (np.abs(got - ref) <= np.spacing(np.abs(ref))).all()


def _check(m, grid, buf, p, filt, tag, lens=None, offset=None, drift=None, records=None, expand=None):
    """qs_check_sweeps == the restatement fed with the device's (sin, cos); returns the device's (checks, classes).
    records / expand: restate only `records` and compare record k with the restatement's record expand[k]."""
    m.set_sweep_filter(*filt)
    dev, cls = m.check_sweeps(buf, lens, params=p, classes=True)
    assert dev.dtype == CR.CHECK_DTYPE and cls.shape == (len(buf), 181)
    sc = np.stack([dev["sin_yaw"], dev["cos_yaw"]], axis=1)
    ref, rcls = CR.check(grid, _geom(m), buf, p, lens, *filt, sincos=sc, offset=offset, drift=drift, records=records)
    if expand is not None:
        ref, rcls = ref[expand], rcls[expand]
    why = CR.differing(dev, ref)
    assert why == "", f"{tag}: {why}"
    assert dev.tobytes() == ref.tobytes(), f"{tag}: bytes differ"
    bad = np.argwhere(cls != rcls)
    assert len(bad) == 0, f"{tag}: {len(bad)} classes differ, first (record, beam) {bad[0]}: {cls[tuple(bad[0])]} against {rcls[tuple(bad[0])]}"
    acc, pose = MR.poses_of(MR.records_of(buf), lens, offset, drift)
    usable = acc & np.array([CR.start_cells(q, _geom(m)) is not None for q in pose])
    assert _ulp_ok(dev[usable], pose[usable, 2]), f"{tag}: sin_yaw / cos_yaw beyond one ulp of libm"
    assert (dev["sin_yaw"][~usable] == 0).all() and (dev["cos_yaw"][~usable] == 0).all()
    assert m.check_sweeps(buf, lens, params=p).tobytes() == dev.tobytes(), f"{tag}: with and without cls_out differ"
    return dev, cls


# ---- the rules, beam by beam -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [68, 200, 192])
def test_checks_and_classes_equal_the_restatement(P, worlds, size):
    """33 sweeps in and round each world, over every edge and corner, true, displaced and with odd ranges; both record formats; the
    default parameters, a strict and a loose set."""
    m, grid = worlds[size]
    poses = _poses(m, grid, 33, seed=size)
    seen = np.zeros(5, dtype=np.int64)
    status = set()
    for filt, odo, p in ((NEAR, True, None), (FAR, False, dict(tol=0.0, min_checked=0, max_bad_percent=0, count_missed=1)),
                         (NEAR, False, dict(tol=0.3, min_checked=181, max_bad_percent=100))):
        buf = _sweeps(P, m, poses, filt[1], seed=size + int(odo), odometry=odo, agent=np.arange(33) % 2 + 1)
        dev, cls = _check(m, grid, buf, p, filt, f"{size} {filt} {p}")
        seen += np.bincount(cls.ravel(), minlength=5)[:5]
        status |= set(dev["status"].tolist())
        counts = np.stack([dev[f] for f in ("agree", "nearer", "farther", "missed", "unseen")], axis=1)
        assert (counts == np.stack([(cls == c).sum(axis=1) for c in range(5)], axis=1)).all()
    assert (seen > 0).all(), f"a class never occurred: {seen}"
    assert status == {CR.OK, CR.UNDECIDED, CR.CONTRADICTS}


def test_the_class_table_on_the_device(pkg):
    """V6 at equality and one f32 step to either side (tests/check_rules.py: table_cases), p exact in f32."""
    size, res, ox, oy = CR.TABLE_GRID
    P = importlib.import_module(pkg.__name__ + ".protocol")
    ms = {kind: _painted(pkg, CR.table_grid(kind), res, ox, oy) for kind in ("hit", "clear", "unknown")}
    try:
        for kind, d, smin, smax, want in CR.table_cases():
            r = np.zeros((1, 181), dtype=np.float32)
            r[0, CR.TABLE_BEAM] = d
            buf = P.pack_sweeps([1], [CR.TABLE_POSE[0]], [CR.TABLE_POSE[1]], [CR.TABLE_POSE[2]], r, odometry=True)
            dev, cls = _check(ms[kind], CR.table_grid(kind), buf, dict(tol=0.0), (smin, smax), f"{kind} {d} {smin} {smax}")
            assert cls[0, CR.TABLE_BEAM] == want and (dev["sin_yaw"][0], dev["cos_yaw"][0]) == (0.0, 1.0)
    finally:
        for m in ms.values():
            m.close()


@pytest.mark.parametrize("smax,C", [(0.04, 2), (1.2, 25), (2.93, 60), (12.68, 255)])
def test_every_patch_radius(P, worlds, smax, C):
    """C = 2, 25, 60 and 255 (the last needs more than 64 KiB of LDS): a patch far wider than the world included."""
    m, grid = worlds[192]
    assert CR.patch_radius(smax, m.res) == C
    poses = _poses(m, grid, 12, seed=C)
    buf = _sweeps(P, m, poses, smax, seed=C)
    dev, _ = _check(m, grid, buf, dict(min_checked=1), (0.01, smax), f"C {C}")
    assert (dev["checked"] > 0).any()


def test_poses_with_no_cell_off_the_grid_and_on_a_wall(P, worlds):
    m, grid = worlds[192]
    poses = _poses(m, grid, 16, seed=1)
    buf = _sweeps(P, m, poses, 3.0, seed=2)
    rec = MR.records_of(buf)
    rec["x"][0] = np.nan                                # no cell
    rec["y"][1] = np.inf
    rec["yaw"][2] = np.nan
    rec["yaw"][3] = -np.inf
    rec["x"][4] = 1e30                                  # beyond 9e15 cells
    rec["y"][5] = -3e9                                  # clamped at 2^30 cells
    rec["x"][6], rec["y"][6] = 40.0, 40.0               # far off the grid
    rec["yaw"][7] = 50.0
    dev, cls = _check(m, grid, buf, dict(min_checked=0), FAR, "odd poses")
    assert (cls[:5] == CR.UNSEEN).all() and (dev["unseen"][:5] == 181).all() and (dev["status"][:5] == CR.OK).all()
    assert (dev["accepted_record"][:8] == 1).all() and (dev["sin_yaw"][5:8] != 0).all()
    assert (dev["farther"][5:7] == 0).all() and (dev["missed"][5:7] == 0).all()  # (off the grid everything is UNKNOWN: no hit)
    assert dev["checked"][10] > 0                                              # the pose on an OCCUPIED cell is checked like any other
    dev, _ = _check(m, grid, buf[:5], None, FAR, "odd poses, default gate")
    assert (dev["status"] == CR.UNDECIDED).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, HOST_CHUNK + 1])
def test_any_number_of_records(P, worlds, n):
    """16 distinct records repeated: every copy must equal the restatement of its original, across the host call's chunks."""
    m, grid = worlds[68]
    base = _sweeps(P, m, _poses(m, grid, 16, seed=3), 1.2, seed=4, agent=np.arange(16) % 2 + 1)
    idx = np.arange(n) % 16
    buf = np.ascontiguousarray(base[idx])
    lens = np.full(n, buf.shape[1], dtype=np.uint16)
    rejected = [n - 1] + ([20] if n > 20 else [])       # (copies: the 16 originals stay intact, but for n = 1)
    buf[n - 1, 0] ^= 0x40                                # by its magic
    if n > 20:
        lens[20] = 743                                   # by its length
    m.set_sweep_filter(*NEAR)
    dev, cls = m.check_sweeps(buf, lens, classes=True)
    sc = np.stack([dev["sin_yaw"], dev["cos_yaw"]], axis=1)
    ref, rcls = CR.check(grid, _geom(m), np.ascontiguousarray(base[:min(n, 16)]), None, None, *NEAR, sincos=sc[:min(n, 16)])
    ref, rcls = ref[idx], rcls[idx]
    for k in rejected:
        ref[k] = np.zeros(1, dtype=CR.CHECK_DTYPE)[0]
        ref["status"][k] = CR.NO_RECORD
        rcls[k] = CR.NO_RECORD_BEAM
    assert CR.differing(dev, ref) == "" and dev.tobytes() == ref.tobytes() and (cls == rcls).all()
    assert len(m.check_sweeps(buf[:0])) == 0


def test_wrong_lengths_magic_and_agent(P, worlds):
    m, grid = worlds[200]
    for odo in (True, False):
        buf = _sweeps(P, m, _poses(m, grid, 12, seed=8), 1.2, seed=9, odometry=odo, agent=np.arange(12) % 2 + 1)
        stride = buf.shape[1]
        lens = np.full(12, stride, dtype=np.uint16)
        lens[1], lens[2], lens[3] = stride - 1, 42, 65535
        buf[4, :4] = np.frombuffer(b"QSRX", np.uint8)
        buf[5, 4], buf[6, 4] = 0, 3
        dev, cls = _check(m, grid, buf, None, NEAR, f"stride {stride}", lens)
        rej = [1, 2, 3, 4, 5, 6]
        assert (dev["status"][rej] == CR.NO_RECORD).all() and (dev["accepted_record"][rej] == 0).all() and (cls[rej] == 255).all()
        assert (dev["accepted_record"][[0, 7, 8, 9, 10, 11]] == 1).all()
        a, b = m.check_sweeps(buf, None), m.check_sweeps(buf, lens)                # lens = NULL: every length equals the stride
        keep = lens == stride
        assert a[keep].tobytes() == b[keep].tobytes() and a["accepted_record"][1] == 1


def test_bot_offset_and_drift(pkg, P):
    """A context with a separation whose first packets close a loop: the check forms its poses as the ingest does, offset first,
    then the drift read on the device."""
    g = np.load(os.path.join(GOLDEN, "session_sep_512.npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    dg, ln = g["datagrams"], g["lengths"]
    cut = 2 * len(dg) // 3
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as m:
        m.ingest_array(dg[:cut], ln[:cut])
        drift = {b: tuple(float(v) for v in m.drift(b)) for b in (1, 2)}
        assert any(v != (0.0, 0.0) for v in drift.values()), "the first part must close a loop"
        grid = m.grid_i8()
        free = np.argwhere(grid == 0)
        rng = np.random.default_rng(12)
        pick = free[rng.integers(len(free), size=14)]
        true = np.stack([ox + (pick[:, 1] + 0.5) * res, oy + (pick[:, 0] + 0.5) * res, rng.uniform(-3, 3, 14)], axis=1).astype(np.float32)
        agent = np.arange(14) % 2 + 1
        buf = _sweeps(P, m, true, 1.2, seed=13, agent=agent)
        rec = MR.records_of(buf)
        for k in range(14):                          # report what makes the ingest form (about) the true pose
            a = int(agent[k])
            rec["x"][k] -= np.float32((float(sep) if a == 2 else 0.0) + drift[a][0])
            rec["y"][k] -= np.float32(drift[a][1])
        dev, _ = _check(m, grid, buf, dict(min_checked=5), NEAR, "offset and drift", offset={2: float(sep)}, drift=drift)
        plain = CR.check(grid, (res, ox, oy), buf, dict(min_checked=5), None, *NEAR)[0]
        assert (dev["checked"] > 0).any() and (plain["agree"] != dev["agree"]).any(), "offset and drift must matter here"
        m.ingest_sweeps(buf, check=dict(min_checked=5))
        acc, pose = m.last_sweeps()
        exp_acc, exp_pose = MR.poses_of(rec, None, {2: float(sep)}, drift)
        held = CR.withheld(dev)
        assert (acc.astype(bool) == (exp_acc & ~held)).all() and (pose[acc.astype(bool)] == exp_pose[acc.astype(bool)]).all()
        assert m.last_sweep_checks().tobytes() == dev.tobytes()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("odometry", [True, False])
def test_host_call_and_device_twin_at_every_byte_offset(P, worlds, odometry):
    """Strides 751 and 743 at byte offsets 0..3 of the device buffer: the same bytes as the host call."""
    m, grid = worlds[200]
    buf = _sweeps(P, m, _poses(m, grid, 21, seed=21), 1.2, seed=22, odometry=odometry, agent=np.arange(21) % 2 + 1)
    n, stride = buf.shape
    lens = np.full(n, stride, dtype=np.uint16)
    lens[2] = 100
    m.set_sweep_filter(*NEAR)
    host, hcls = m.check_sweeps(buf, lens, classes=True)
    d_lens = _dev(lens.view(np.int16))
    for off in range(4):
        raw = torch.zeros(n * stride + 8, dtype=torch.uint8, device="cuda")
        raw[off:off + n * stride] = _dev(buf.reshape(-1))
        d_out = torch.full((n * CR.CHECK_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        d_cls = torch.full((n * 181 + 3,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m.check_sweeps_device(raw.data_ptr() + off, n, stride, d_out.data_ptr(), d_lens=d_lens.data_ptr(), d_cls=d_cls.data_ptr())
        m.sync()
        assert d_out.cpu().numpy().tobytes() == host.tobytes(), f"offset {off}"
        got = d_cls.cpu().numpy()
        assert (got[:n * 181].reshape(n, 181) == hcls).all() and (got[n * 181:] == 0xEE).all(), f"offset {off}"
        d_out.fill_(0xEE)
        m.check_sweeps_device(raw.data_ptr() + off, n, stride, d_out.data_ptr(), d_lens=d_lens.data_ptr())     # cls_out is optional
        m.sync()
        assert d_out.cpu().numpy().tobytes() == host.tobytes()


def test_a_check_writes_nothing(pkg, P):
    grid = RR.world()
    res, ox, oy = RR.WORLD_GRID[1:]
    with pkg.QuasarMapper(len(grid), res, ox, oy) as m:
        m.dirty_tracking(True)
        MZ.paint(m, RR.paint_rays(grid), res, ox, oy)
        m.set_sweep_filter(*FAR)
        buf = _sweeps(P, m, _poses(m, grid, 20, seed=30), 3.0, seed=31)
        m.ingest_sweeps(buf[:5])
        before = (m.grid_i8(), m.counts(), m.counters(), m.dirty_blocks(), m.checkpoint())
        for _ in range(2):
            m.check_sweeps(buf, classes=True)
        d_out = torch.zeros(20 * 56, dtype=torch.uint8, device="cuda")
        m.check_sweeps_device(_dev(buf).data_ptr(), 20, buf.shape[1], d_out.data_ptr())
        m.sync()
        after = (m.grid_i8(), m.counts(), m.counters(), m.dirty_blocks(), m.checkpoint())
        assert (before[0] == after[0]).all() and (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        assert before[2] == after[2] and before[3] == after[3]
        assert before[4] == after[4], "checkpoint bytes (grid, counters, next sequence number, dirty blocks) changed"
        acc, _ = m.last_sweeps()                            # the last ingest is still the last ingest
        assert len(acc) == 5
        with pytest.raises(pkg.QuasarError):
            m.last_sweep_checks()


def test_refusals(pkg, P, worlds):
    m, grid = worlds[68]
    buf = _sweeps(P, m, _poses(m, grid, 2, seed=40), 1.2, seed=41)
    m.set_sweep_filter(*NEAR)
    for call in (lambda p: m.check_sweeps(buf, params=p), lambda p: m.ingest_sweeps(buf, check=p)):
        for bad, text in ((dict(tol=-0.01), "tol"), (dict(tol=math.nan), "tol"), (dict(tol=math.inf), "tol"),
                          (dict(min_checked=-1), "min_checked"), (dict(min_checked=182), "min_checked"),
                          (dict(max_bad_percent=-1), "max_bad_percent"), (dict(max_bad_percent=101), "max_bad_percent"),
                          (dict(count_missed=2), "count_missed"), (dict(count_missed=-1), "count_missed"), (dict(reserved=1), "reserved")):
            with pytest.raises(pkg.QuasarError, match=text):
                call(bad)
    with pytest.raises(pkg.QuasarError, match="stride"):
        m.check_sweeps(np.ascontiguousarray(buf[:, :700]))
    with pytest.raises(pkg.QuasarError, match="stride"):
        m.ingest_sweeps(np.ascontiguousarray(buf[:, :700]), check=True)
    with pytest.raises(ValueError, match="match and check"):
        m.ingest_sweeps(buf, match=True, check=True)
    m.check_sweeps(buf, params=dict(tol=0.0, min_checked=181, max_bad_percent=100, count_missed=1))       # the limits themselves
    m.set_sweep_filter(0.02, 12.75)                      # ceil(12.75 / 0.05) + 1 = 256
    try:
        for call in (lambda: m.check_sweeps(buf), lambda: m.check_sweeps(buf[:0]), lambda: m.ingest_sweeps(buf, check=True)):
            with pytest.raises(pkg.QuasarError, match="smax is too large"):
                call()
    finally:
        m.set_sweep_filter(*NEAR)
    assert m.counters()["datagrams"] == 0, "a refused guarded ingest must not have ingested"
    with pkg.QuasarMapper(64, 0.05, 0.0, 0.0, seq_stride=2) as sh:
        with pytest.raises(pkg.QuasarError, match="sharded"):
            sh.check_sweeps(buf)
        with pytest.raises(pkg.QuasarError, match="sharded"):
            sh.ingest_sweeps(buf, check=True)


# ---- the guarded ingest ------------------------------------------------------------------------------------------------------------
def _same_context(a, b, tag):
    assert (a.grid_i8() == b.grid_i8()).all(), f"{tag}: grids differ"
    for x, y in zip(a.counts(), b.counts()):
        assert (x == y).all(), f"{tag}: hit / miss counters differ"
    assert a.counters() == b.counters(), f"{tag}: {a.counters()} against {b.counters()}"
    assert a.checkpoint() == b.checkpoint(), f"{tag}: checkpoints differ"


@pytest.mark.parametrize("mode", [1, 2])
def test_guarded_ingest_equals_a_plain_ingest_without_the_withheld_records(pkg, P, mode):
    """Direct (1) and tiled (2) raycast.  40 sweeps in the three-room world, a third of them displaced, three rejected: the guarded
    ingest into one context against the plain ingest, into a second one, of the buffer with the withheld records' magic broken."""
    grid = RR.world()
    geom = RR.WORLD_GRID[1:]
    with _painted(pkg, grid, *geom, raycast_mode=mode) as m, _painted(pkg, grid, *geom, raycast_mode=mode) as ref:
        for c in (m, ref):
            c.set_sweep_filter(*FAR)
        poses, _ = RR.query_poses(grid, geom, 40, seed=7)
        buf = _sweeps(P, m, poses, 3.0, seed=50, agent=np.arange(40) % 2 + 1)
        lens = np.full(40, buf.shape[1], dtype=np.uint16)
        buf[5, 4], lens[17] = 9, 10
        buf[29, 1] ^= 1
        p = dict(tol=0.10)
        pre, _ = _check(m, grid, buf, p, FAR, f"mode {mode}, before", lens)
        held = CR.withheld(pre)
        assert held.sum() >= 3 and (pre["status"] == CR.OK).sum() >= 3, "the scene must withhold some sweeps and map some"
        c0 = m.counters()
        assert m.ingest_sweeps(buf, lens, check=p) == 40
        got = m.last_sweep_checks()
        assert got.tobytes() == pre.tobytes(), "the checks of the ingest are not those of the pre-call map"
        acc, pose = m.last_sweeps()
        exp_acc, exp_pose = MR.poses_of(MR.records_of(buf), lens)
        mapped = exp_acc & ~held
        assert (acc.astype(bool) == mapped).all() and (pose[mapped] == exp_pose[mapped]).all() and np.isnan(pose[~mapped]).all()
        c1 = m.counters()
        assert c1["datagrams"] - c0["datagrams"] == 40 and c1["accepted"] - c0["accepted"] == mapped.sum()
        assert c1["rays"] - c0["rays"] == 181 * mapped.sum()
        assert ref.ingest_sweeps(CR.break_magic(buf, held), lens) == 40
        _same_context(m, ref, f"mode {mode}")
        a2, p2 = ref.last_sweeps()
        assert (a2 == acc).all() and np.array_equal(p2, pose, equal_nan=True)
        # the sequence numbers went on as if nothing had been withheld: one more plain sweep into both
        for c in (m, ref):
            c.ingest_sweeps(buf[:1])
        _same_context(m, ref, "plain after guarded")
        with pytest.raises(pkg.QuasarError):
            m.last_sweep_checks()
        m.ingest_sweeps(buf[:3], check=p)
        m.ingest_array(np.zeros((1, 48), dtype=np.uint8), np.array([42], dtype=np.uint16), np.zeros(1))
        with pytest.raises(pkg.QuasarError):
            m.last_sweep_checks()


def test_guarded_ingest_with_nothing_withheld_is_the_plain_ingest(pkg, P):
    """True poses: nothing is withheld, and the context is byte for byte what the plain ingest leaves; host against device twin."""
    grid = RR.world()
    geom = RR.WORLD_GRID[1:]
    with _painted(pkg, grid, *geom) as m, _painted(pkg, grid, *geom) as ref, _painted(pkg, grid, *geom) as dv:
        for c in (m, ref, dv):
            c.set_sweep_filter(*FAR)
        poses, _ = RR.query_poses(grid, geom, 24, seed=7)
        buf = m.sense_sweeps(poses, np.ones(24, dtype=np.uint8), odometry=False, max_range=3.0)
        lens = np.full(24, buf.shape[1], dtype=np.uint16)
        lens[3] = 5
        m.ingest_sweeps(buf, lens, check=True)
        ck = m.last_sweep_checks()
        assert not CR.withheld(ck).any() and (ck["status"] == CR.OK).sum() >= 3 and ck["status"][3] == CR.NO_RECORD
        ref.ingest_sweeps(buf, lens)
        _same_context(m, ref, "nothing withheld")
        d_buf, d_lens = _dev(buf), _dev(lens.view(np.int16))
        torch.cuda.synchronize()
        dv.ingest_sweeps_checked_device(d_buf.data_ptr(), 24, buf.shape[1], d_lens=d_lens.data_ptr())
        dv.sync()
        assert dv.last_sweep_checks().tobytes() == ck.tobytes()
        _same_context(m, dv, "device twin")
        for a, b in zip(m.last_sweeps(), dv.last_sweeps()):
            assert np.array_equal(a, b, equal_nan=True)
        # an empty map decides nothing, so it withholds nothing
        with pkg.QuasarMapper(192, *geom) as e, pkg.QuasarMapper(192, *geom) as e2:
            for c in (e, e2):
                c.set_sweep_filter(*FAR)
            e.ingest_sweeps(buf, lens, check=True)
            e2.ingest_sweeps(buf, lens)
            assert (e.last_sweep_checks()["status"][[0, 1, 2]] == CR.UNDECIDED).all()
            _same_context(e, e2, "empty map")


def test_guarded_ingest_in_chunks_checks_against_the_pre_call_map(pkg, P):
    """A call of more than one internal chunk (65536 records): the first chunk draws the room (and 65 thousand rejected records),
    the second holds sweeps that contradict that room.  Checked after chunk 1 was mapped they would be withheld; checked as the
    rule says, against the map before the call, most of them are undecided and mapped."""
    size, res, ox, oy = MR.ROOM_GRID
    s = MR.room_session(seed=11, n_map=30, n_query=30, window=4, angle_steps=5)
    mp = s["map_pose"]
    draw = P.pack_sweeps(np.ones(30, int), mp[:, 0], mp[:, 1], mp[:, 2], s["map_ranges"], odometry=True)
    q = s["q_pose"].copy()
    q[:, 0] += 0.6                                        # lost by 0.6 m and 0.5 rad
    q[:, 2] += 0.5
    late = P.pack_sweeps(np.ones(30, int), q[:, 0], q[:, 1], q[:, 2], s["q_ranges"], odometry=True)
    n1 = 1 << 16
    big = np.zeros((n1 + 30, draw.shape[1]), dtype=np.uint8)
    big[:] = draw[0]
    big[:, 4] = 9                                         # rejected: agent 9
    big[1000:1030] = draw
    big[n1:] = late
    filt = (MR.ROOM_SMIN, MR.ROOM_SMAX)
    with pkg.QuasarMapper(size, res, ox, oy) as m, pkg.QuasarMapper(size, res, ox, oy) as ref, pkg.QuasarMapper(size, res, ox, oy) as dv:
        for c in (m, ref, dv):
            c.set_sweep_filter(*filt)
            c.ingest_sweeps(draw[:1])                     # a map that is not empty, but not the room
        pre = m.check_sweeps(big)
        held = CR.withheld(pre)                           # (the one seed sweep decides a few of them)
        m.ingest_sweeps(big, check=True)
        assert m.last_sweep_checks().tobytes() == pre.tobytes()
        acc, _ = m.last_sweeps()
        assert acc.sum() == 60 - held.sum()
        ref.ingest_sweeps(CR.break_magic(big, held))
        _same_context(m, ref, "chunked")
        with pkg.QuasarMapper(size, res, ox, oy) as room:  # the same sweeps against the map as chunk 1 leaves it
            room.set_sweep_filter(*filt)
            room.ingest_sweeps(draw)
            would = CR.withheld(room.check_sweeps(late))
            assert (would & ~held[n1:]).sum() >= 5, "the scene must hold sweeps that only the room of chunk 1 contradicts"
        d_big = _dev(big)
        torch.cuda.synchronize()
        dv.ingest_sweeps_checked_device(d_big.data_ptr(), len(big), big.shape[1])
        dv.sync()
        assert dv.last_sweep_checks().tobytes() == pre.tobytes()
        _same_context(m, dv, "chunked, device twin")


def test_graph_mode_refuses_the_guarded_ingest_but_not_the_check(pkg, P, worlds):
    grid = RR.world()
    geom = RR.WORLD_GRID[1:]
    w, _ = worlds[192]
    with _painted(pkg, grid, *geom) as m:
        m.set_sweep_filter(*FAR)
        buf = _sweeps(P, m, _poses(m, grid, 9, seed=60), 3.0, seed=61)
        w.set_sweep_filter(*FAR)
        plain = w.check_sweeps(buf)
        m.set_sweep_graph(True)
        before = m.checkpoint()
        with pytest.raises(pkg.QuasarError, match="graph mode"):
            m.ingest_sweeps(buf, check=True)
        d_buf = _dev(buf)
        with pytest.raises(pkg.QuasarError, match="graph mode"):
            m.ingest_sweeps_checked_device(d_buf.data_ptr(), 9, buf.shape[1])
        assert m.checkpoint() == before and m.counters()["datagrams"] == w.counters()["datagrams"]
        assert m.check_sweeps(buf).tobytes() == plain.tobytes()
        m.set_sweep_graph(False)
        m.ingest_sweeps(buf, check=True)
        assert m.last_sweep_checks().tobytes() == plain.tobytes()
