"""The map merge session and the device voxel down-sampling (include/quasar_slam.h: "map merge session") against the
host-to-host entry points they restate: every step of a callback must equal, bit for bit, what qs_grid_to_pcd, qs_icp,
qs_voxel_downsample and qs_rasterise give for the same data (tests/merge_rules.py strings them together)."""
import hashlib
import importlib
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import GOLDEN, load_pkg
from oracle import oracle as orc
import merge_rules as R

pytestmark = pytest.mark.gpu

VOXEL = 0.05
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5003, 70001)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "session_512.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def m(pkg):
    with pkg.QuasarMapper() as mapper:
        yield mapper


def rules_session(m):
    """tests/merge_rules.py over the mapper's host-to-host entry points: the second opinion of every step."""
    return R.Session(m.grid_to_pcd, m.icp, m.voxel_downsample, m.rasterise)


def same_result(r, want):
    assert r["status"] == want["status"], (r, want)
    assert (r["T"] == want["T"]).all() and r["fitness"] == want["fitness"] and r["rmse"] == want["rmse"], (r, want)
    assert r["iterations"] == want["iterations"] and r["n_local"] == want["n_local"] and r["n_global"] == want["n_global"], (r, want)


def same_map(got, want):
    if want[0] is None:
        assert got is None or got[0] is None
        return
    assert got[0].shape == want[0].shape and (got[0] == want[0]).all() and (np.asarray(got[1]) == np.asarray(want[1])).all()


@pytest.fixture(scope="module")
def expected(m, golden):
    """The six-map sequence through the rules, once: per step (result, cloud after, published map)."""
    s = rules_session(m)
    out = []
    for name, g, res, ox, oy, status in R.sequence(golden["grid"]):
        r = s.callback(g, res, ox, oy)
        assert r["status"] == status, (name, r)
        out.append((r, s.cloud.copy(), s.publish()))
    return out


# ---- 1. voxel down-sampling on the device ------------------------------------------------------------------------------
def voxel_keys(xy):
    mn = xy.min(0) - VOXEL * 0.5
    v = np.floor((xy - mn) / VOXEL).astype(np.int64)
    return v[:, 1] * (1 << 32) + v[:, 0]


def cloud(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "uniform":
        return rng.uniform(0.0, 20.0, (n, 2))
    if kind == "one_voxel":                                    # one run across every workgroup tile
        return 3.0 + rng.uniform(0.0, 0.02, (n, 2))
    if kind == "lattice_duplicates":                           # 900 lattice nodes: exact duplicates from n = 63 up
        return rng.integers(0, 30, (n, 2)) * 0.05 + 1.0
    if kind == "strip":                                        # 4 km x 3 m: vx needs three digit passes, vy one
        return rng.uniform(0.0, 1.0, (n, 2)) * [4000.0, 3.0]
    if kind == "strip_transposed":
        return rng.uniform(0.0, 1.0, (n, 2)) * [3.0, 4000.0]
    if kind == "negative":
        return rng.uniform(-30.0, -10.0, (n, 2))
    xy = rng.uniform(0.0, 20.0, (n, 2))
    order = np.argsort(voxel_keys(xy), kind="stable")
    return np.ascontiguousarray(xy[order] if kind == "key_order" else xy[order[::-1]])


def voxel_on_device(m, xy, cap=None):
    n = len(xy)
    d_in = torch.from_numpy(np.ascontiguousarray(xy)).cuda()
    torch.cuda.synchronize()
    k = m.voxel_downsample_device(d_in, n, VOXEL)
    cap = k if cap is None else cap
    d_out = torch.full((max(cap, 1) + 3, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    k2 = m.voxel_downsample_device(d_in, n, VOXEL, d_out, cap)
    assert k2 == k
    out = d_out.cpu().numpy()
    assert (out[cap:] == -7.0).all()                           # nothing behind the capacity is written
    return k, out[:cap]


@pytest.mark.parametrize("kind", ["uniform", "one_voxel", "lattice_duplicates", "strip", "strip_transposed", "negative",
                                  "key_order", "reverse_key_order"])
def test_voxel_downsample_device_equals_the_host_path(m, kind):
    for n in SIZES:
        xy = cloud(kind, n)
        want = m.voxel_downsample(xy, VOXEL)
        k, got = voxel_on_device(m, xy)
        assert k == len(want) and np.array_equal(got, want), (kind, n, k, len(want))
        if n <= 5003:
            assert np.array_equal(got, orc.voxel_downsample(xy, VOXEL)), (kind, n)
        if kind == "one_voxel":
            assert k == 1
        if kind == "lattice_duplicates" and n >= 2049:
            assert k < n
        if kind in ("strip", "strip_transposed") and n >= 1023:
            v = np.floor((xy - (xy.min(0) - VOXEL * 0.5)) / VOXEL).max(0)
            assert (v[0] >= 65536 and v[1] < 256) if kind == "strip" else (v[1] >= 65536 and v[0] < 256)   # three digits, one


def test_voxel_downsample_device_capacity_and_empty(m):
    xy = cloud("uniform", 5003)
    want = m.voxel_downsample(xy, VOXEL)
    for cap in (0, 1, len(want) // 2, len(want) - 1):
        k, got = voxel_on_device(m, xy, cap=cap)
        assert k == len(want) and np.array_equal(got, want[:cap])
    assert m.voxel_downsample_device(0, 0, VOXEL) == 0
    d = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert m.voxel_downsample_device(d, 0, VOXEL, d, 4) == 0
    with pytest.raises(Exception, match=r"\(-1\)"):
        m.voxel_downsample_device(d, 4, 0.0)


# ---- 2. the callback, step by step -----------------------------------------------------------------------------------------
def test_six_map_sequence_step_by_step(m, golden, expected):
    m.merge_reset()
    m.merge_params()
    assert m.merge_cloud().shape == (0, 2) and m.merge_global_map() == (None, None)
    for (name, g, res, ox, oy, status), (want, cloud_after, published) in zip(R.sequence(golden["grid"]), expected):
        before = m.merge_cloud()
        local = m.grid_to_pcd(g, res, ox, oy)
        r = m.merge_grid(g, res, ox, oy)
        same_result(r, want)
        after = m.merge_cloud()
        if status == R.ADOPTED:
            assert (after == local).all()
        else:
            T, fit, rm, it = m.icp(local, before, 1.0, 30)
            assert (r["T"] == T).all() and r["fitness"] == fit and r["rmse"] == rm and r["iterations"] == it, name
        if status == R.MERGED:
            assert r["fitness"] == 1.0
            assert np.array_equal(after, m.voxel_downsample(np.concatenate([before, R.moved(local, r["T"])]), R.RES)), name
        if status == R.REJECTED:
            assert r["fitness"] == 0.0 and (r["T"] == np.eye(3)).all() and r["iterations"] == 1
            assert np.array_equal(after, before)
        assert np.array_equal(after, cloud_after), name
        same_map(m.merge_global_map(), m.rasterise(after, R.RES))
        same_map(m.merge_global_map(), published)
    # an empty map changes nothing
    before = m.merge_cloud()
    r = m.merge_grid(np.full((8, 8), -1, dtype=np.int8), 0.1, 3.0, 4.0)
    assert r["status"] == R.EMPTY and r["n_local"] == 0 and r["n_global"] == len(before) and (r["T"] == np.eye(3)).all()
    assert np.array_equal(m.merge_cloud(), before)


def test_fitness_gate_cases(m, golden):
    grid = golden["grid"]
    for name, g, fitness, status in R.gate_cases(grid):
        m.merge_reset()
        s = rules_session(m)
        assert m.merge_grid(grid, R.RES, R.OX, R.OY)["status"] == R.ADOPTED
        s.callback(grid, R.RES, R.OX, R.OY)
        before = m.merge_cloud()
        r = m.merge_grid(g, R.RES, R.OX, R.OY)
        same_result(r, s.callback(g, R.RES, R.OX, R.OY))
        assert r["fitness"] == fitness and r["status"] == status, (name, r)
        assert np.array_equal(m.merge_cloud(), s.cloud)
        if status == R.REJECTED:
            assert np.array_equal(m.merge_cloud(), before)


# ---- 3. a map that is already on the device --------------------------------------------------------------------------------
def test_device_grid_and_context_maps_equal_the_host_grid(pkg, golden):
    size, res, ox, oy, sep = golden["cfg"]
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as a, \
         pkg.QuasarMapper(int(size), res, ox + 0.10, oy - 0.15, separation=sep) as b:
        for mp in (a, b):
            mp.ingest_array(golden["datagrams"], golden["lengths"])
        views = [(a.grid_i8(), res, ox, oy), (b.grid_i8(), res, ox + 0.10, oy - 0.15)]
        assert hashlib.sha256(views[0][0].tobytes()).digest() == golden["grid_sha256"].tobytes()
        assert (views[1][0] == 100).sum() > 300
        # the yardstick: the host grids through qs_merge_grid, in b's session
        want = [b.merge_grid(*v) for v in views]
        want_cloud = b.merge_cloud()
        assert [w["status"] for w in want] == [R.ADOPTED, R.MERGED]
        # a's session: its own map (src == ctx), then b's, both read from the stamps
        got = [a.merge_map(a), a.merge_map(b)]
        for r, w in zip(got, want):
            same_result(r, w)
        assert np.array_equal(a.merge_cloud(), want_cloud)
        same_map(a.merge_global_map(), b.merge_global_map())
        # the same views as device tensors
        a.merge_reset()
        tensors = [torch.from_numpy(v[0]).cuda() for v in views]
        torch.cuda.synchronize()
        for t, v, w in zip(tensors, views, want):
            same_result(a.merge_grid(t, *v[1:]), w)
        assert np.array_equal(a.merge_cloud(), want_cloud)
        assert hashlib.sha256(a.grid_i8().tobytes()).digest() == golden["grid_sha256"].tobytes()      # the maps are only read


# ---- 4. life cycle -----------------------------------------------------------------------------------------------------------
def block_map(edge, size=96):
    g = np.full((size, size), -1, dtype=np.int8)
    lo = (size - edge) // 2
    g[lo:lo + edge, lo:lo + edge] = 100
    return g


def test_growth_keeps_the_contents(m):
    m.merge_reset()
    s = rules_session(m)
    small, large = block_map(8), block_map(44)                 # 64 points, then 1936: 30 times as many
    for g in (small, large):
        same_result(m.merge_grid(g, 0.05, -2.0, -2.0), s.callback(g, 0.05, -2.0, -2.0))
        assert np.array_equal(m.merge_cloud(), s.cloud)
    assert len(s.cloud) > 1024                                  # beyond the first block of the cloud: it has grown
    same_map(m.merge_global_map(), s.publish())


def test_ingest_reset_and_parameters(pkg, golden):
    size, res, ox, oy, sep = golden["cfg"]
    grid = golden["grid"]
    sha = golden["grid_sha256"].tobytes()
    with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep) as mp:
        assert mp.merge_grid(grid, res, ox, oy)["status"] == R.ADOPTED
        cloud0 = mp.merge_cloud()
        mp.ingest_array(golden["datagrams"], golden["lengths"])                      # the mapper goes on mapping
        assert hashlib.sha256(mp.grid_i8().tobytes()).digest() == sha
        assert np.array_equal(mp.merge_cloud(), cloud0)
        assert mp.merge_grid(grid, res, ox + 0.10, oy - 0.15)["status"] == R.MERGED
        assert hashlib.sha256(mp.grid_i8().tobytes()).digest() == sha                # a callback does not touch the map
        cloud1 = mp.merge_cloud()
        mp.reset()                                                                   # qs_reset: the merger is a node of its own
        assert (mp.grid_i8() == -1).all() and np.array_equal(mp.merge_cloud(), cloud1)
        mp.merge_reset()
        assert mp.merge_cloud().shape == (0, 2) and mp.merge_global_map() == (None, None)
        r = mp.merge_grid(grid, res, ox + 1.0, oy)
        assert r["status"] == R.ADOPTED and (mp.merge_cloud() == mp.grid_to_pcd(grid, res, ox + 1.0, oy)).all()
        for bad in ((0.0, 30, 0.6), (-1.0, 30, 0.6), (1.0, -1, 0.6)):
            with pytest.raises(pkg.QuasarError, match=r"\(-1\)"):
                mp.merge_params(*bad)
        # parameters that were refused changed nothing; accepted ones hold: a gate of 0.9 rejects 437/537
        mp.merge_params(1.0, 30, 0.9)
        mp.merge_reset()
        mp.merge_grid(grid, res, ox, oy)
        r = mp.merge_grid(R.with_corner_block(grid, 10), res, ox, oy)
        assert r["status"] == R.REJECTED and r["fitness"] == 437 / 537
        mp.merge_params(1.0, 0, 0.6)                                                 # no iteration: the first evaluation only
        r = mp.merge_grid(grid, res, ox + 0.10, oy - 0.15)
        T, fit, rm, it = mp.icp(mp.grid_to_pcd(grid, res, ox + 0.10, oy - 0.15), cloud0, 1.0, 0)
        assert r["iterations"] == 0 == it and (r["T"] == np.eye(3)).all() and r["fitness"] == fit and r["rmse"] == rm


# ---- 5. the merger node over the session -------------------------------------------------------------------------------------
def test_map_merger_device_equals_the_steps(pkg, m, golden, expected):
    merger = importlib.import_module(pkg.__name__ + ".merger")
    mm = merger.MapMerger(m, device=True)
    assert mm.publish_global_map() is None and mm.global_xy.shape == (0, 2)
    assert mm.map_callback(np.full((8, 8), -1, dtype=np.int8), 0.05, 0.0, 0.0) is None
    for (name, g, res, ox, oy, status), (want, cloud_after, published) in zip(R.sequence(golden["grid"]), expected):
        out = mm.map_callback(g, res, ox, oy, agent_id=1)
        if status == R.REJECTED:
            assert out is None
        else:
            same_map(out, published)
        if status == R.ADOPTED:
            assert mm.last_registration is None and (mm.map_resolution, mm.map_origin) == (res, [ox, oy])
        else:
            T, fit, rm, it = mm.last_registration
            assert (T == want["T"]).all() and (fit, rm, it) == (want["fitness"], want["rmse"], want["iterations"])
        assert np.array_equal(mm.global_xy, cloud_after), name
        same_map(mm.publish_global_map(), published)
    assert (mm.map_resolution, mm.map_origin) == (R.RES, [R.OX, R.OY])
