"""The bot veil on the device (csrc/veil.hip) against its restatement (tests/veil_rules.py), by ==: the flags of every ingest, the
map (cells, stamps, hit and miss counters), the table of bot cells, the statistics word and the ray / hit / cell counters, on
the built scenes that tests/test_veil_rules_cpu.py proves reach their cases.  edge_rays == 0: no ray was left to the host.
256 x 256 grids."""
import importlib

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import veil_rules as vr
from conftest import load_pkg

pytestmark = pytest.mark.gpu
QS_E_INVAL = -1


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _stamps(pkg, m):
    from test_gpu_sweeps import _stamps as st
    return st(pkg, m)


def state(pkg, m):
    xy, known = m.bot_veil_cells()
    out = dict(grid=m.grid_i8(), stamps=_stamps(pkg, m), xy=xy, known=known, total=m.bot_veil_stats(), counters=m.counters())
    if m.cfg.enable_counts:
        out["hits"], out["misses"] = m.counts()
    return out


def same_state(got, want, tag):
    for k in ("grid", "stamps", "hits", "misses", "xy", "known"):
        if k in got:
            assert (got[k] == want[k]).all(), f"{tag}: {k}: {int((got[k] != want[k]).sum())} entries differ from the rule"
    assert got["total"] == want["total"], (tag, got["total"], want["total"])
    c = got["counters"]
    assert (c["rays"], c["hits"], c["cells"]) == (want["n_rays"], want["n_hits"], want["n_cells"]), (tag, c, want["n_rays"], want["n_hits"], want["n_cells"])
    assert c["edge_rays"] == 0, f"{tag}: {c['edge_rays']} rays were left to the host"


def run_scene(pkg, name, **kw):
    """The scene's steps through a fresh mapper with the veil on; every ingest's flags and hit flags, and the session's state
    before every reset and at the end, against the model's."""
    sc = vr.get(name)
    model, veiled, valid = vr.model(name)
    g = sc.g
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=sc.max_agent, **kw) as m:
        m.set_bot_veil(sc.radius)
        assert m.bot_veil() == sc.radius
        k = snap = 0
        for st in sc.steps:
            if st[0] == "ingest":
                m.ingest_array(st[1])
                got = m.last_veiled()
                assert (got == veiled[k]).all(), f"{name}, ingest {k}: flags differ at {np.argwhere(got != veiled[k])[:8].tolist()}"
                assert (m.last_hits()[1] == valid[k]).all(), f"{name}, ingest {k}: V5: last_hits changed"
                k += 1
            elif st[0] == "place":
                m.bot_veil_place(*st[1:])
            elif st[0] == "forget":
                m.bot_veil_forget(st[1])
            elif st[0] == "reset":
                same_state(state(pkg, m), model.snaps[snap], f"{name}, before reset {snap}")
                snap += 1
                m.reset()
                assert m.bot_veil() == sc.radius and not m.bot_veil_cells()[1].any() and m.bot_veil_stats() == 0
        same_state(state(pkg, m), model.snaps[snap], f"{name}, end")


@pytest.mark.parametrize("name", vr.names("radius"))
def test_radius_edge(pkg, name):
    """d^2 == radius^2 is veiled, radius^2 + 1 is not: radius 1, 3, 32, and 5 at the offset (3, 4)."""
    run_scene(pkg, name)


def test_which_pose_speaks(pkg):
    """Just before / just after; the later of two; a rejected packet between; the table from the previous ingest; bot_veil_place;
    after bot_veil_forget and after reset nothing is veiled."""
    run_scene(pkg, "which-pose")


@pytest.mark.parametrize("name", vr.names("blocks") + ["one-bot-block", "many-bots"])
def test_block_edges(pkg, name):
    run_scene(pkg, name)


@pytest.mark.parametrize("name", ["never", "tile-border"])
def test_never_veiled_and_tile_borders(pkg, name):
    run_scene(pkg, name)


def test_variants_without_counts_and_with_device_trig(pkg):
    for kw in ({"enable_counts": False}, {"exact_trig": False}, {"raycast_mode": 2}):
        run_scene(pkg, "mixed-300", **kw)
        run_scene(pkg, "tile-border", **kw)


@pytest.mark.parametrize("n", vr.SMALL_N)
def test_small_batches_take_the_tiled_form(pkg, n):
    """1, 4 and 20 packets: a veil-off context sends them through the direct kernel."""
    run_scene(pkg, f"mixed-{n}")
    sc = vr.get("which-pose")                                    # (its ingests are 1 to 12 packets: veiled beams in small batches)
    assert max(len(st[1]) for st in sc.steps if st[0] == "ingest") <= 20


def _plain(pkg, sc, prepare=None):
    g = sc.g
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=sc.max_agent) as m:
        if prepare:
            prepare(m)
        m.ingest_array(sc.steps[0][1])
        out = state(pkg, m)
        out.update(veiled=m.last_veiled(), last_hits=m.last_hits(), zones={b: m.zone(b) for b in range(1, sc.max_agent + 1)}, radius=m.bot_veil())
    return out


def test_v5_the_rest_sees_the_beam_as_the_filter_judged_it(pkg):
    """last_hits, the zone boxes and the counters of a veiled context equal a veil-off context's on the same stream -- but for
    QS_CNT_CELLS, which counts cells written: one less per veiled ray."""
    sc = vr.get("mixed-300")
    off = _plain(pkg, sc)
    on = _plain(pkg, sc, lambda m: m.set_bot_veil(sc.radius))
    assert on["veiled"].any() and not off["veiled"].any()
    assert (on["last_hits"][1] == off["last_hits"][1]).all()
    assert np.array_equal(on["last_hits"][0][on["last_hits"][1] == 1], off["last_hits"][0][off["last_hits"][1] == 1])
    for b in off["zones"]:
        assert (on["zones"][b] is None) == (off["zones"][b] is None)
        if off["zones"][b] is not None:
            assert (np.asarray(on["zones"][b]) == np.asarray(off["zones"][b])).all()
    c_on, c_off = dict(on["counters"]), dict(off["counters"])
    assert c_on.pop("cells") == c_off.pop("cells") - int(on["veiled"].sum()) and on["total"] == int(on["veiled"].sum())
    timing = {k for k in c_on if k.startswith("slam_")}          # (cycle counts of the chain kernel: never equal between two runs)
    assert {k: v for k, v in c_on.items() if k not in timing} == {k: v for k, v in c_off.items() if k not in timing}


def test_off_means_off(pkg):
    sc = vr.get("mixed-300")
    never = _plain(pkg, sc)
    onoff = _plain(pkg, sc, lambda m: (m.set_bot_veil(3), m.set_bot_veil(0)))
    assert never["radius"] == 0 and onoff["radius"] == 0
    for k in ("grid", "stamps", "hits", "misses"):
        assert (never[k] == onoff[k]).all(), k
    assert not never["veiled"].any() and not onoff["veiled"].any() and never["veiled"].shape == (300, 4)
    for k in ("rays", "hits", "cells", "accepted", "datagrams"):
        assert never["counters"][k] == onoff["counters"][k]
    assert not onoff["known"].any() and onoff["total"] == 0      # an ingest with the veil off does not feed the table either


def test_refusals_leave_the_setting_unchanged(pkg):
    g = vr.geo()
    L = importlib.import_module(pkg.__name__ + "._lib").load()
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=3) as m:
        m.set_bot_veil(3)
        for r in (33, -1):
            assert L.qs_set_bot_veil(m._h, r) == QS_E_INVAL and m.bot_veil() == 3
    for kw in (dict(raycast_mode=1), dict(shard_bots=1, shard_rank=0), dict(seq_stride=2)):
        with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=3, **kw) as m:
            assert L.qs_set_bot_veil(m._h, 3) == QS_E_INVAL and m.bot_veil() == 0
            with pytest.raises(pkg.QuasarError):
                m.set_bot_veil(3)


def test_last_veiled_follows_last_hits_convention(pkg):
    g = vr.geo()
    L = importlib.import_module(pkg.__name__ + "._lib").load()
    sc = vr.get("mixed-20")
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=3) as m:
        m.set_bot_veil(3)
        m.ingest_array(sc.steps[0][1])
        buf = np.zeros((19, 4), dtype=np.uint8)
        assert L.qs_last_veiled(m._h, buf.ctypes.data, 19) == QS_E_INVAL
        assert m.last_veiled().shape == (20, 4)


def test_restore_empties_the_table_and_keeps_the_setting(pkg):
    """V2: checkpoints do not carry the table."""
    sc = vr.get("mixed-20")
    g = sc.g
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=sc.max_agent) as m:
        m.set_bot_veil(3)
        m.ingest_array(sc.steps[0][1])
        assert m.bot_veil_cells()[1][1:].all()
        data = m.checkpoint()
        grid = m.grid_i8()
        m.restore(data)
        assert m.bot_veil() == 3 and not m.bot_veil_cells()[1].any() and m.bot_veil_stats() == 0
        assert (m.grid_i8() == grid).all()
        m.ingest_array(sc.steps[0][1])
        assert m.bot_veil_cells()[1][1:].all() and m.last_veiled().shape == (20, 4)


# ---- the sim: bots that see each other -----------------------------------------------------------------------------------------
def test_sim_bodies_leave_phantoms_without_the_veil_and_none_with_it(pkg):
    sim_mod = importlib.import_module(pkg.__name__ + ".sim")
    g = vr.geo()
    world_cells = vr.room_world()
    body = vr.ROOM_BODY * g.res
    c = lambda q, o: o + (np.asarray(q, dtype=np.float64) + 0.5) * g.res
    poses = [(float(c(cx, g.ox)), float(c(cy, g.oy)), float(vr.rs.YAW4[h])) for _, cx, cy, h, _ in vr.room_ranges()]
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy) as world:
        fy, fx = np.nonzero(world_cells == 0)
        world.update_rays(c(fx, g.ox), c(fy, g.oy), c(fx + 1, g.ox), c(fy, g.oy), np.zeros(len(fx), np.uint8))
        wy, wx = np.nonzero(world_cells == 100)
        world.update_rays(c(wx, g.ox), c(wy, g.oy), c(wx, g.ox), c(wy, g.oy), np.ones(len(wx), np.uint8))
        assert (world.grid_i8() == world_cells).all()
        with pytest.raises(ValueError):
            with sim_mod.SwarmSim.make_mapper(world, max_agent=4) as m:
                sim_mod.SwarmSim(world, m, poses, kind="sweeps", bodies=body)
        phantoms = {}
        for radius in (0, vr.ROOM_RADIUS):
            with sim_mod.SwarmSim.make_mapper(world, max_agent=4) as m:
                m.set_bot_veil(radius)
                s = sim_mod.SwarmSim(world, m, poses, kind="packets", max_range=1.2, bodies=body)
                for _ in range(3):
                    s.sense()
                    s.tick += 1
                rec = s.last_records().view(importlib.import_module(pkg.__name__ + ".protocol").PACKET_DTYPE).reshape(-1)
                assert np.allclose(rec["front"], (2 * vr.ROOM_A - vr.ROOM_BODY) * g.res, atol=1e-6)      # every front beam stops on a body
                phantoms[radius] = int(((m.grid_i8() == 100) & (world_cells == 0)).sum())
                assert (m.bot_veil_stats() > 0) == (radius > 0)
        assert phantoms[0] > 0 and phantoms[vr.ROOM_RADIUS] == 0, phantoms
