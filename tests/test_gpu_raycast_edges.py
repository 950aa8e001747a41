"""The tile-binned raycast on built rays (tests/ray_scenes.py): every scene puts its rays on one edge of csrc/raycast_tiled.hip,
raycast_tiled.h or raycast_common.h -- tests/test_ray_scenes_cpu.py proves on the CPU that it gets there -- and the map must
equal the CPU oracle's, fed the same bytes, with `==`: cells, hit / miss counters, stamps, ray / hit / cell counters.
edge_rays == 0 is what makes this a test of the DEVICE kernels: no ray was left to the host's exact-trig loop.
Zones are compared at the parity suite's float tolerance.  Direct (raycast_mode 1) and tiled (2)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import ray_scenes as rs
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
FLOAT_TOL = 1e-5                  # tests/test_gpu_parity.py's
VARIANTS = {"threshold": ({}, {"exact_trig": False}, {"enable_counts": False}),
            "corner": ({}, {"exact_trig": False}),
            "edges": ({}, {"exact_trig": False}, {"enable_counts": False}),
            "units": ({}, {"enable_counts": False})}
SPLITS = (1, 255, 256, 257)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


_REF = {}


def reference(pkg, name):
    """The oracle's answer for a scene, computed once and shared."""
    if name not in _REF:
        from test_gpu_sweeps import _P, _beams, _records
        sc = rs.get(name)
        o = sc.geo.oracle(sc.max_agent)
        if sc.kind == "packets":
            o.feed_stream(sc.data)
            stamps, hits = o.stamps, len(o.hit_points)
        else:
            # update_rays stamps every beam alike, so the expected stamps are a per-beam replay of the oracle's own
            # world_to_grid and bresenham with the sweep ordinals (ray_scenes.sweep_stamps_reference)
            beams = _beams(_records(_P(pkg), sc.data))
            o.update_rays(*beams)
            stamps, hits = rs.sweep_stamps_reference(sc), int(beams[4].sum())
        ref = dict(grid=o.grid, hits=o.hits, misses=o.misses, stamps=stamps, n_rays=o.n_rays, n_hits=hits,
                   n_cells=o.n_cells_written, zones=[o.zone(b) for b in (1, 2)])
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = ref
    return _REF[name]


def run_scene(pkg, name, mode, split=None, **kw):
    """The scene through a fresh mapper (in two ingests if split); what the comparisons need of its state."""
    from test_gpu_sweeps import _stamps
    sc, g = rs.get(name), rs.get(name).geo
    parts = [sc.data] if split is None else [sc.data[:split], sc.data[split:]]
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=sc.max_agent, raycast_mode=mode, **kw) as m:
        for part in parts:
            if sc.kind == "packets":
                m.ingest_array(part)
            else:
                m.ingest_sweeps(part)
        out = dict(grid=m.grid_i8(), stamps=_stamps(pkg, m), counters=m.counters(), zones=[m.zone(b) for b in (1, 2)])
        if kw.get("enable_counts", True):
            out["hits"], out["misses"] = m.counts()
    return out


def check(name, ref, out, tag):
    sc = rs.get(name)
    assert (out["grid"] == ref["grid"]).all(), f"{tag}: {(out['grid'] != ref['grid']).sum()} cells differ from the oracle"
    if "hits" in out:
        assert (out["hits"] == ref["hits"]).all(), f"{tag}: {(out['hits'] != ref['hits']).sum()} hit counters differ"
        assert (out["misses"] == ref["misses"]).all(), f"{tag}: {(out['misses'] != ref['misses']).sum()} miss counters differ"
    assert (out["stamps"] == ref["stamps"]).all(), f"{tag}: {(out['stamps'] != ref['stamps']).sum()} stamps differ"
    c = out["counters"]
    assert c["rays"] == ref["n_rays"] and c["hits"] == ref["n_hits"], (tag, c, ref["n_rays"], ref["n_hits"])
    assert c["cells"] == ref["n_cells"], (tag, c["cells"], ref["n_cells"])
    assert c["edge_rays"] == 0, f"{tag}: {c['edge_rays']} rays were left to the host"
    if sc.kind == "packets":
        for z, oz in zip(out["zones"], ref["zones"]):
            assert (z is None) == (oz is None), tag
            if oz is not None:
                np.testing.assert_allclose(z, oz, rtol=0, atol=FLOAT_TOL)


def run_and_check(pkg, name, mode, **kw):
    out = run_scene(pkg, name, mode, **kw)
    check(name, reference(pkg, name), out, f"{name}, mode {mode}, {kw}")
    return out


SINGLE = [n for n in rs.names() if not n.startswith(("order", "decomp"))]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", SINGLE)
def test_scene_equals_the_oracle(pkg, name, mode):
    """counters and runs here run with the default raster workgroup count: one item per workgroup, so the tiles they share
    go through the atomic merge."""
    for kw in VARIANTS.get(name.split("-")[0], ({},)):
        run_and_check(pkg, name, mode, **kw)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", rs.names("order") + rs.names("decomp"))
def test_scene_equals_the_oracle_whole_and_split(pkg, name, mode):
    """Also ingested in two parts, split at 1, 255, 256 and 257 records: the same stamps as unsplit (winner and loser of a
    cell in different ingests; the parts' own workgroup decompositions)."""
    whole = run_and_check(pkg, name, mode)
    n = len(rs.get(name).data)
    for split in SPLITS:
        if split < n:
            out = run_and_check(pkg, name, mode, split=split)
            assert (out["stamps"] == whole["stamps"]).all(), f"split at {split}"


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import test_gpu_raycast_edges as T
pkg = T.load_pkg()
for name in ("counters", "runs"):
    for kw in ({}, {"enable_counts": False}):
        T.run_and_check(pkg, name, 2, **kw)
print("OK")
"""


@pytest.mark.parametrize("wgs", [1, 2, 3])
def test_counters_and_runs_with_few_raster_workgroups(wgs):
    """QS_RASTER_WGS is read once per process (see test_raster_long_runs_flush_and_tile_changes): one fresh child per value.
    1: one run of 33 items of one tile (the flush after 31 items: a cell with 65540 misses) and a run across six tiles with
    empty tiles between them; 2: a run that starts after empty tiles; 3: a tile split between two workgroups."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, QS_RASTER_WGS=str(wgs))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
