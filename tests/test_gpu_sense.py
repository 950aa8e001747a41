"""Sensing a world on the GPU (qs_sense_ranges / _sweeps / _packets and their _device twins).  The bar: the CPU restatement of
the rules S1-S8 (tests/sense_rules.py) fed grid_i8() -- every range, hit cell and packet byte with ==.  Beams whose far point lies
within 1e-6 cells of a cell boundary (sense_rules.edge_beams) are not compared, and every test asserts that they are at most
0.1 % of its beams, so a skipped beam cannot hide a failure."""
import importlib
import math
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import maze_scenes as MZ
import sense_rules as S
from conftest import GOLDEN, load_pkg
from test_sense_rules_cpu import ROUND_TRIP_CELLS

pytestmark = pytest.mark.gpu
MAX_R = 12.68           # ceil(12.68 / 0.05) + 1 = 255 = QS_SENSE_MAX_CELLS


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


def _scene(size, seed):
    """A walled room with boxes and a diagonal wall whose cells touch corner to corner (a Bresenham line can slip through)."""
    res, ox, oy, lo, hi = MZ.GEOMETRY[size][:5]
    rng = np.random.default_rng(seed)
    occ = set()
    for t in range(lo, hi):
        occ |= {(t, lo), (t, hi - 1), (lo, t), (hi - 1, t)}
    for _ in range(size // 6):
        x, y = rng.integers(lo + 2, hi - 8, 2)
        w, h = rng.integers(1, 7, 2)
        occ |= {(int(x) + i, int(y) + j) for i in range(w) for j in range(h)}
    for t in range(size // 3):
        occ.add((lo + 4 + t, lo + 9 + t))
    grid, rays = MZ.room(size, lo, hi, sorted(occ))
    return grid, rays, res, ox, oy


@pytest.fixture(scope="module")
def worlds(pkg):
    """{size: (mapper, grid)}: the scenes painted at 68 (the second tile is 4 cells wide) and at 200."""
    out = {}
    for size, seed in ((68, 5), (200, 11)):
        grid, rays, res, ox, oy = _scene(size, seed)
        m = pkg.QuasarMapper(size, res, ox, oy)
        MZ.paint(m, rays, res, ox, oy)
        assert (m.grid_i8() == grid).all()
        out[size] = (m, grid)
    yield out
    for m, _ in out.values():
        m.close()


def _poses(m, grid, n, seed, margin=0.3):
    """n float32 poses: random ones over the grid and a margin round it, then, as far as n reaches, yaws at the multiples of 45
    degrees from free cells."""
    rng = np.random.default_rng(seed)
    lo, hi = m.ox - margin, m.ox + m.size * m.res + margin
    p = np.stack([rng.uniform(lo, hi, n), rng.uniform(lo, hi, n), rng.uniform(-math.pi, math.pi, n)], axis=1).astype(np.float32)
    free = np.argwhere(grid == 0)
    for j in range(min(n // 2, 9)):
        gy, gx = free[rng.integers(len(free))]
        p[n - 1 - j] = (m.ox + (gx + 0.37) * m.res, m.oy + (gy + 0.61) * m.res, (j - 4) * math.pi / 4)
    return p


def _rules_kw(kw):
    """The restatement's keywords from the Python API's (dropout as a share -> q16)."""
    out = dict(kw)
    if "dropout" in out:
        out["dropout_q16"] = int(round(out.pop("dropout") * 65536))
    return out


def _edges(m, poses, beams, max_range=1.2, records=None):
    sel = np.arange(len(poses)) if records is None else np.asarray(records)
    edge = np.zeros((len(poses), beams), dtype=bool)
    edge[sel] = S.edge_beams(m.res, m.ox, m.oy, np.asarray(poses, dtype=np.float32)[sel], beams, max_range)
    assert edge.sum() <= 0.001 * len(sel) * beams, f"{edge.sum()} edge beams of {len(sel) * beams}"
    return edge


def _check_ranges(m, poses, beams, records=None, **kw):
    """sense_ranges against the restatement fed grid_i8(); returns the device's (ranges, cells)."""
    poses = np.asarray(poses, dtype=np.float32)
    got_r, got_c = m.sense_ranges(poses, beams, return_cells=True, **kw)
    exp_r, exp_c = S.sense_ranges(m.grid_i8(), m.res, m.ox, m.oy, poses, beams, records=records, **_rules_kw(kw))
    edge = _edges(m, poses, beams, kw.get("max_range", 1.2), records)
    ok = ~edge
    if records is not None:
        ok &= np.isin(np.arange(len(poses)), records)[:, None]
    assert got_r.shape == exp_r.shape == (len(poses), beams)
    bad = ok & ((got_r.view(np.uint32) != exp_r.view(np.uint32)) | (got_c != exp_c))
    assert not bad.any(), f"{bad.sum()} beams differ, first (record, beam) {np.argwhere(bad)[0]}: " \
                          f"{got_r[bad][0]} / {got_c[bad][0]} against {exp_r[bad][0]} / {exp_c[bad][0]}"
    return got_r, got_c


def _expected_records(P, m, kind, poses, agent, got, records=None, max_range=1.2, **fields_and_kw):
    """The restatement's records for `kind` (743, 751 or 42) with the device's own value put into the edge beams' range fields."""
    fields = {k: fields_and_kw.pop(k) for k in ("enc", "v2v", "landmark") if k in fields_and_kw}
    kw = _rules_kw(dict(fields_and_kw, max_range=max_range))
    grid = m.grid_i8()
    beams = 4 if kind == P.PACKET_SIZE else S.BEAMS
    edge = _edges(m, poses, beams, max_range, records)
    if kind == P.PACKET_SIZE:
        exp = S.sense_packets(P, grid, m.res, m.ox, m.oy, poses, agent, records=records, **fields, **kw)
        names = ("front", "left", "back", "right")
        er, gr = exp.view(P.PACKET_DTYPE).reshape(-1), np.ascontiguousarray(got).view(P.PACKET_DTYPE).reshape(-1)
        for s, name in enumerate(names):
            er[name][edge[:, s]] = gr[name][edge[:, s]]
        return exp
    odometry = kind == P.PACKET_SIZE_V0_ODO
    exp = S.sense_sweeps(P, grid, m.res, m.ox, m.oy, poses, agent, odometry=odometry, records=records, **fields, **kw)
    dt = P.PACKET_DTYPE_V0_ODO if odometry else P.PACKET_DTYPE_V0
    er, gr = exp.view(dt).reshape(-1), np.ascontiguousarray(got).view(dt).reshape(-1)
    er["ranges"][edge] = gr["ranges"][edge]
    return exp


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the rules, beam by beam -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [68, 200])
def test_ranges_and_records_equal_the_restatement(pkg, P, worlds, size):
    """65 poses in and round the grid, random yaws and every multiple of 45 degrees: ranges and hit cells of both forms, and the
    bytes of the three record formats with their pass-through fields."""
    m, grid = worlds[size]
    poses = _poses(m, grid, 65, seed=size)
    r181, c181 = _check_ranges(m, poses, 181)
    r4, c4 = _check_ranges(m, poses, 4)
    assert (c181 >= 0).mean() > 0.2 and (c4 >= 0).mean() > 0.2          # the scene is seen
    # all eight octants, steep and flat lines: the hit cells lie on every side of their poses
    x0 = np.array([S.cell(float(p[0]), m.ox, m.res) for p in poses])[:, None]
    y0 = np.array([S.cell(float(p[1]), m.oy, m.res) for p in poses])[:, None]
    hit = c181 >= 0
    dx, dy = (c181 % size - x0)[hit], (c181 // size - y0)[hit]
    octant = (dx > 0).astype(int) + 2 * (dy > 0) + 4 * (np.abs(dx) > np.abs(dy))
    assert set(octant[(dx != 0) & (dy != 0) & (np.abs(dx) != np.abs(dy))].tolist()) == set(range(8))
    rng = np.random.default_rng(1)
    agent = rng.integers(1, 255, 65).astype(np.uint8)
    enc = rng.integers(-2 ** 31, 2 ** 31, 65).astype(np.int32)
    v2v = rng.integers(0, 2 ** 32, 65, dtype=np.uint64).astype(np.uint32)
    lm = rng.integers(0, 6, 65).astype(np.uint8)
    got = m.sense_sweeps(poses, agent, enc=enc, v2v=v2v)
    assert got.shape == (65, 751) and got.tobytes() == _expected_records(P, m, 751, poses, agent, got, enc=enc, v2v=v2v).tobytes()
    assert S.ranges_of(P, got).tobytes() == r181.tobytes()
    got = m.sense_sweeps(poses, agent, odometry=False)
    assert got.shape == (65, 743) and got.tobytes() == _expected_records(P, m, 743, poses, agent, got).tobytes()
    got = m.sense_packets(poses, agent, enc=enc, v2v=v2v, landmark=lm)
    assert got.shape == (65, 42)
    assert got.tobytes() == _expected_records(P, m, 42, poses, agent, got, enc=enc, v2v=v2v, landmark=lm).tobytes()
    assert S.ranges_of(P, got).tobytes() == r4.tobytes()
    # NULL enc / v2v / landmark mean 0
    got = m.sense_packets(poses, agent)
    assert got.tobytes() == _expected_records(P, m, 42, poses, agent, got).tobytes()
    got = m.sense_sweeps(poses, agent)
    assert got.tobytes() == _expected_records(P, m, 751, poses, agent, got).tobytes()


@pytest.mark.parametrize("size", [68, 200])
def test_edges_corners_outside_nonfinite_and_occupied_poses(pkg, P, worlds, size):
    """The patch hangs over each edge and each corner of the grid; one pose stands outside and looks in; poses that are not finite
    return nothing; a pose on an OCCUPIED cell is not blocked by it."""
    m, grid = worlds[size]
    w = m.size * m.res
    lo, mid, hi = m.ox + 0.031, m.ox + w / 2 + 0.013, m.ox + w - 0.031
    spots = [(lo, mid), (hi, mid), (mid, lo), (mid, hi), (lo, lo), (lo, hi), (hi, lo), (hi, hi)]
    poses = [(x, y, yaw) for x, y in spots for yaw in (0.3, 2.0, -1.1, -2.6)]
    poses.append((m.ox - 0.42, mid, 0.05))                 # outside, looking in
    poses.append((mid, m.oy + w + 0.33, -math.pi / 2 + 0.02))
    occ = np.argwhere(grid == 100)
    for gy, gx in occ[:: max(1, len(occ) // 7)]:
        poses.append((m.ox + (gx + 0.5) * m.res, m.oy + (gy + 0.45) * m.res, 0.7))
    n_fin = len(poses)
    poses += [(math.nan, mid, 0.0), (mid, math.inf, 0.0), (mid, mid, -math.inf), (3e38, mid, 0.0), (mid, -3e38, 1.0)]
    poses = np.array(poses, dtype=np.float32)
    for beams in (181, 4):
        r, c = _check_ranges(m, poses, beams, no_return=-1.0)
        assert (r[n_fin:] == -1.0).all() and (c[n_fin:] == -1).all()
        assert (c[32] >= 0).any() or beams == 4             # the pose outside sees the wall inside
        assert (c[34:n_fin] >= 0).any()                     # poses on OCCUPIED cells see past their own
    got = m.sense_packets(poses, 1)
    assert got.tobytes() == _expected_records(P, m, 42, poses, 1, got).tobytes()       # NaN poses travel bit for bit


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_record_counts_round_a_workgroup(pkg, P, worlds, n):
    m, grid = worlds[68]
    poses = _poses(m, grid, n, seed=100 + n) if n else np.zeros((0, 3), np.float32)
    _check_ranges(m, poses, 4)
    _check_ranges(m, poses, 181)
    got = m.sense_packets(poses, 2, enc=7)
    assert got.shape == (n, 42) and got.tobytes() == _expected_records(P, m, 42, poses, 2, got, enc=7).tobytes()
    got = m.sense_sweeps(poses, 2, odometry=False)
    assert got.shape == (n, 743) and got.tobytes() == _expected_records(P, m, 743, poses, 2, got).tobytes()


def test_one_record_more_than_a_host_chunk(pkg, P, worlds):
    """A host call stages 4096 records at a time; the device call does not: 4097 records agree between the two byte for byte,
    the packets with the restatement throughout, the sweeps (R of one cell: C = 2) on the records round the seam."""
    m, grid = worlds[68]
    n = 4097
    poses = _poses(m, grid, n, seed=4097, margin=0.05)
    agent = (np.arange(n) % 200 + 1).astype(np.uint8)
    enc = np.arange(n, dtype=np.int32)
    kw = dict(noise_amp=0.01, dropout=0.1, seed=3, first_record=5)
    got = m.sense_packets(poses, agent, enc=enc, **kw)
    assert got.tobytes() == _expected_records(P, m, 42, poses, agent, got, enc=enc, **kw).tobytes()
    d_pose, d_agent, d_enc = _dev(poses), _dev(agent), _dev(enc)
    d_out = torch.zeros(n * 751 + 8, dtype=torch.uint8, device="cuda")
    m.sense_packets_device(d_pose, d_agent, n, d_out.data_ptr() + 3, d_enc=d_enc, **kw)
    m.sync()
    assert d_out[3:3 + n * 42].cpu().numpy().tobytes() == got.tobytes()
    near = [0, 1, 4094, 4095, 4096]
    kw["max_range"] = 0.05
    got = m.sense_sweeps(poses, agent, enc=enc, **kw)
    exp = _expected_records(P, m, 751, poses, agent, got, records=near, enc=enc, **kw)
    assert got[near].tobytes() == exp[near].tobytes()
    d_out.zero_()
    m.sense_sweeps_device(d_pose, d_agent, n, d_out.data_ptr() + 1, 751, d_enc=d_enc, **kw)
    m.sync()
    assert d_out[1:1 + n * 751].cpu().numpy().tobytes() == got.tobytes()
    assert d_out[0] == 0 and (d_out[1 + n * 751:] == 0).all()          # nothing written round the records
    _check_ranges(m, poses, 181, records=near, **kw)


@pytest.mark.parametrize("max_range,C", [(0.05, 2), (1.2, 25), (2.93, 60), (MAX_R, 255)])
def test_patch_sizes(pkg, P, worlds, max_range, C):
    """C = ceil(R / res) + 1 at its smallest, at the default sensor range (24 cells), at 60 and at QS_SENSE_MAX_CELLS."""
    assert math.ceil(max_range / 0.05) + 1 == C
    for size, n in ((68, 5), (200, 4)):
        m, grid = worlds[size]
        poses = _poses(m, grid, n, seed=C)
        _, c = _check_ranges(m, poses, 181, max_range=max_range)
        _check_ranges(m, poses, 4, max_range=max_range)
        if C >= 25:
            assert (c >= 0).any()


def test_golden_session_sensed_from_its_own_last_poses(pkg, P):
    """A mapped session is a world too.  The sense call is the first to observe the map after the ingest, so waiting exact-trig edge
    rays are resolved by it (S1)."""
    g = np.load(os.path.join(GOLDEN, "session_512.npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    poses = g["pose_xyyaw"][-48:].astype(np.float32)
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as m:
        m.ingest_array(g["datagrams"], g["lengths"])
        got_r, got_c = m.sense_ranges(poses, 181, return_cells=True, max_range=3.0)
        assert (m.grid_i8() == g["grid"]).all()
        r, c = _check_ranges(m, poses, 181, max_range=3.0)
        assert r.tobytes() == got_r.tobytes() and (c == got_c).all() and (c >= 0).sum() > 100
        _check_ranges(m, poses, 4, max_range=1.2)


# ---- the two entry-point families ------------------------------------------------------------------------------------------
def test_device_twins_give_the_host_calls_bytes(pkg, P, worlds):
    m, grid = worlds[200]
    n = 65
    poses = _poses(m, grid, n, seed=9)
    rng = np.random.default_rng(2)
    agent = rng.integers(1, 255, n).astype(np.uint8)
    enc = rng.integers(-1000, 1000, n).astype(np.int32)
    v2v = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    lm = rng.integers(0, 6, n).astype(np.uint8)
    d_pose, d_agent, d_enc, d_v2v, d_lm = _dev(poses), _dev(agent), _dev(enc), _dev(v2v), _dev(lm)
    kw = dict(max_range=2.0, noise_amp=0.02, dropout=0.05, seed=11, first_record=77, no_return=-3.0)
    for beams in (181, 4):
        hr, hc = m.sense_ranges(poses, beams, return_cells=True, **kw)
        d_r = torch.zeros((n, beams), dtype=torch.float32, device="cuda")
        d_c = torch.zeros((n, beams), dtype=torch.int32, device="cuda")
        m.sense_ranges_device(d_pose, n, d_r, beams, d_cells=d_c, **kw)
        m.sync()
        assert d_r.cpu().numpy().tobytes() == hr.tobytes() and (d_c.cpu().numpy() == hc).all()
        d_r.zero_()
        m.sense_ranges_device(d_pose, n, d_r, beams, **kw)                   # hit_cell may be NULL
        m.sync()
        assert d_r.cpu().numpy().tobytes() == hr.tobytes()
    for stride in (743, 751):
        host = m.sense_sweeps(poses, agent, enc=enc, v2v=v2v, odometry=stride == 751, **kw)
        for shift in range(4):                                               # every alignment of the first record
            d_out = torch.zeros(n * stride + 8, dtype=torch.uint8, device="cuda")
            m.sense_sweeps_device(d_pose, d_agent, n, d_out.data_ptr() + shift, stride, d_enc=d_enc, d_v2v=d_v2v, **kw)
            m.sync()
            out = d_out.cpu().numpy()
            assert out[shift:shift + n * stride].tobytes() == host.tobytes()
            assert not out[:shift].any() and not out[shift + n * stride:].any()
    host = m.sense_packets(poses, agent, enc=enc, v2v=v2v, landmark=lm, **kw)
    for shift in range(4):
        d_out = torch.zeros(n * 42 + 8, dtype=torch.uint8, device="cuda")
        m.sense_packets_device(d_pose, d_agent, n, d_out.data_ptr() + shift, d_enc=d_enc, d_v2v=d_v2v, d_landmark=d_lm, **kw)
        m.sync()
        out = d_out.cpu().numpy()
        assert out[shift:shift + n * 42].tobytes() == host.tobytes()
        assert not out[:shift].any() and not out[shift + n * 42:].any()
    rec = host.view(P.PACKET_DTYPE).reshape(-1)
    assert (rec["agent"] == agent).all() and (rec["enc"] == enc).all() and (rec["v2v"] == v2v).all() and (rec["lm"] == lm).all()
    assert (rec["magic"] == b"QSRL").all() and rec["x"].tobytes() == poses[:, 0].tobytes()


def test_noise_dropout_and_the_split_call(pkg, P, worlds):
    m, grid = worlds[200]
    poses = _poses(m, grid, 64, seed=21, margin=0.0)
    kw = dict(max_range=3.0, noise_amp=0.03, dropout=0.1, seed=0xC0FFEE)
    whole_r, whole_c = _check_ranges(m, poses, 181, first_record=1000, **kw)
    a_r, a_c = m.sense_ranges(poses[:32], 181, return_cells=True, first_record=1000, **kw)
    b_r, b_c = m.sense_ranges(poses[32:], 181, return_cells=True, first_record=1032, **kw)
    assert np.concatenate([a_r, b_r]).tobytes() == whole_r.tobytes() and (np.concatenate([a_c, b_c]) == whole_c).all()
    clean_r, clean_c = m.sense_ranges(poses, 181, return_cells=True, max_range=3.0)
    hit = clean_c >= 0
    dropped = hit & (whole_c < 0)
    far = np.float32(3.0 - 0.031)                          # noise cannot push these past R
    sure = hit & (clean_r < far)
    assert 0.07 < dropped[sure].mean() < 0.13
    extra = ~hit & (whole_c >= 0)                          # a wall just beyond R that the noise pulled inside it: nothing else
    assert (whole_r[extra] > np.float32(3.0 - 0.031)).all()
    kept = hit & (whole_c >= 0)
    assert (whole_c[kept] == clean_c[kept]).all() and (whole_r[kept] != clean_r[kept]).mean() > 0.9
    assert (np.abs(whole_r[kept].astype(np.float64) - clean_r[kept]) < 0.03 + 2.0 ** -21).all()
    _check_ranges(m, poses, 4, first_record=2 ** 40, **kw)
    got = m.sense_sweeps(poses, 1, first_record=1000, **kw)
    assert S.ranges_of(P, got).tobytes() == whole_r.tobytes()


def test_the_world_is_untouched(pkg, P, worlds):
    m, grid = worlds[200]
    before = (m.grid_i8().tobytes(), m.counters(), m.checkpoint())
    poses = _poses(m, grid, 70, seed=5)
    m.sense_ranges(poses, 181, return_cells=True, max_range=MAX_R)
    m.sense_ranges(poses, 4)
    m.sense_sweeps(poses, 1, noise_amp=0.1, dropout=0.5, seed=1)
    m.sense_packets(poses, 2)
    d_pose, d_agent = _dev(poses), _dev(np.ones(70, np.uint8))
    d_out = torch.zeros(70 * 751, dtype=torch.uint8, device="cuda")
    m.sense_sweeps_device(d_pose, d_agent, 70, d_out, 751)
    m.sense_packets_device(d_pose, d_agent, 70, d_out)
    m.sync()
    after = (m.grid_i8().tobytes(), m.counters(), m.checkpoint())
    assert before[0] == after[0] and before[1] == after[1] and before[2] == after[2]


def test_invalid_arguments(pkg, P, worlds):
    m, grid = worlds[68]
    poses = _poses(m, grid, 3, seed=1)
    L = importlib.import_module(pkg.__name__ + "._lib")
    assert L.QS_SENSE_MAX_CELLS == 255 == S.MAX_CELLS
    bad = [dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=math.inf), dict(max_range=math.nan), dict(max_range=MAX_R + 0.05),
           dict(noise_amp=-0.01), dict(noise_amp=math.inf), dict(noise_amp=math.nan), dict(dropout=1.0 + 1 / 65536)]
    for kw in bad:
        assert not S.check_params(m.res, **_rules_kw(dict(dict(max_range=1.2), **kw)))
        for call in (lambda: m.sense_ranges(poses, 181, **kw), lambda: m.sense_ranges(poses, 4, **kw),
                     lambda: m.sense_sweeps(poses, 1, **kw), lambda: m.sense_packets(poses, 1, **kw),
                     lambda: m.sense_packets(poses[:0], 1, **kw)):
            with pytest.raises(pkg.QuasarError, match=r"\(-1\)"):
                call()
    m.sense_ranges(poses, 181, max_range=MAX_R, dropout=1.0)                   # the limits themselves are valid
    for beams in (0, 3, 5, 180, 182):
        with pytest.raises(pkg.QuasarError, match=r"\(-1\)"):
            m.sense_ranges(poses, beams)
    import ctypes as C
    lib, prm = pkg.load(), m.sense_params()
    out = np.zeros((3, 800), np.uint8)
    agent = np.ones(3, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for stride in (0, 42, 742, 744, 750, 752):
        assert lib.qs_sense_sweeps(m._h, ptr(poses), ptr(agent), None, None, 3, C.byref(prm), ptr(out), stride) == -1
    assert lib.qs_sense_sweeps(m._h, ptr(poses), ptr(agent), None, None, 3, C.byref(prm), ptr(out), 743) == 0
    for field in (0, 1):
        p2 = m.sense_params()
        p2.reserved[field] = 1
        assert lib.qs_sense_ranges(m._h, ptr(poses), 3, 181, C.byref(p2), ptr(out), None) == -1
        assert lib.qs_sense_packets(m._h, ptr(poses), ptr(agent), None, None, None, 3, C.byref(p2), ptr(out)) == -1
    assert lib.qs_sense_ranges(m._h, ptr(poses), 3, 181, None, ptr(out), None) == -1              # params is required
    assert lib.qs_sense_sweeps(m._h, ptr(poses), None, None, None, 3, C.byref(prm), ptr(out), 751) == -1      # ... and agent
    assert lib.qs_sense_packets(m._h, ptr(poses), None, None, None, None, 3, C.byref(prm), ptr(out)) == -1
    assert lib.qs_sense_ranges(m._h, None, 0, 181, C.byref(prm), None, None) == 0                  # n == 0 is valid


# ---- the closed loop ------------------------------------------------------------------------------------------------------------
def test_closed_loop_three_bots_by_path(pkg, P, worlds):
    """Three bots explore the size-200 scene for 40 ticks by qs_frontier_targets_by_path: the known area never shrinks and grows,
    and every cell the swarm maps OCCUPIED lies within ROUND_TRIP_CELLS (measured in tests/test_sense_rules_cpu.py) of an OCCUPIED
    cell of the world.  The same bots sensed with 42-byte packets ingest and add pose-graph nodes."""
    sim_mod = importlib.import_module(pkg.__name__ + ".sim")
    world, grid = worlds[200]
    c = lambda gx, gy, yaw: (world.ox + (gx + 0.5) * world.res, world.oy + (gy + 0.5) * world.res, yaw)
    free = lambda gx, gy: grid[gy - 2:gy + 3, gx - 2:gx + 3].max() == 0
    cells = [(gx, gy) for gy in range(90, 120) for gx in range(90, 120) if free(gx, gy)]
    starts = [c(*cells[0], 0.0), c(*cells[len(cells) // 2], 2.0), c(*cells[-1], -2.0)]
    with sim_mod.SwarmSim.make_mapper(world, max_agent=3) as m:
        sim = sim_mod.SwarmSim(world, m, starts, kind="sweeps", max_range=1.2, speed=0.4)
        known = [sim.step("by_path") for _ in range(40)]
        assert sim.history == known and all(b >= a for a, b in zip(known, known[1:])), known
        assert known[-1] > known[0] > 0, known
        assert np.abs(sim.poses[:, :2] - np.array(starts, dtype=np.float32)[:, :2]).max() > 0.5      # the bots went somewhere
        mapped = m.grid_i8()
        assert (mapped == 100).sum() > 50
        assert S.chebyshev_to_occupied(mapped == 100, grid == 100) <= ROUND_TRIP_CELLS
        recs = sim.last_records()
        assert recs.shape == (3, 751) and (recs[:, 4] == [1, 2, 3]).all()
    with sim_mod.SwarmSim.make_mapper(world, max_agent=3) as m:
        sim = sim_mod.SwarmSim(world, m, starts, kind="packets", max_range=1.2, speed=0.4)
        for _ in range(5):
            sim.step("nearest")
        assert m.slam_sizes(0)[0] == 15 and sim.known_cells() > 0
        acc, _ = m.last_batch()
        assert acc.tolist() == [1, 1, 1]
