"""The bot veil for sweeps on the device (csrc/veil.hip, the sweep stage) against its restatement (tests/sweep_veil_rules.py), by
==: the flags of every ingest, the map (cells, stamps, hit and miss counters), the table of bot cells, the statistics word and the
ray / hit / cell counters, on the built scenes that tests/test_sweep_veil_rules_cpu.py proves reach their cases.
edge_rays == 0: no beam was left to the host.  256 x 256 grids (the matched ingest: match_rules' room, 200 x 200)."""
import importlib

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import match_rules as MR
import ray_scenes as rs
import sweep_veil_rules as sv
import veil_rules as vr
from conftest import load_pkg
from oracle import oracle as orc
from test_gpu_bot_veil import same_state, state

pytestmark = pytest.mark.gpu
QS_E_INVAL = -1
CONTRADICTS = 3


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def to_743(buf):
    """The same sweeps without the odometry fields (743-byte records)."""
    return np.ascontiguousarray(np.concatenate([buf[:, :17], buf[:, 25:]], axis=1))


def ingest(m, buf, entry="host", stride=751, offset=0, **kw):
    """One sweep ingest of the 751-byte records `buf` through the given entry point, stride and byte offset of record 0."""
    data = buf if stride == 751 else to_743(buf)
    if entry == "host":
        if offset:
            raw = np.zeros(data.size + 4, dtype=np.uint8)
            base = (-raw.ctypes.data) % 4 + offset                 # record 0 at `offset` bytes past a dword boundary
            raw[base:base + data.size] = data.reshape(-1)
            data = raw[base:base + data.size].reshape(data.shape)
        m.ingest_sweeps(data, **kw)
    else:
        d = torch.zeros(data.size + 4, dtype=torch.uint8, device="cuda")
        d[offset:offset + data.size] = torch.from_numpy(data.reshape(-1)).cuda()
        m.ingest_sweeps_device(d.data_ptr() + offset, len(data), stride)
        torch.cuda.synchronize()
        m.counters()                                             # (the call is asynchronous: d must outlive it)


def make(pkg, sc, veil=True, **kw):
    g = sc.g
    m = pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, max_agent=sc.max_agent, **kw)
    if veil:
        m.set_bot_veil(sc.radius, sweeps=True)
        assert m.bot_veil() == sc.radius and m.bot_veil_sweeps() is True
    if sc.smax != rs.SMAX_D:
        m.set_sweep_filter(rs.SMIN_D, sc.smax)
    return m


def run_scene(pkg, name, entry="host", stride=751, offset=0, **kw):
    """The scene's steps through a fresh mapper with the sweep veil acting; every ingest's flags, and the session's state before
    every reset and at the end, against the model's."""
    sc = sv.get(name)
    model, veiled, valid = sv.model(name)
    with make(pkg, sc, **kw) as m:
        k = snap = 0
        for st in sc.steps:
            if st[0] == "sweeps":
                ingest(m, st[1], entry, stride, offset)
                got = m.last_sweeps_veiled()
                assert got.shape == veiled[k].shape and got.dtype == np.uint8
                assert (got == veiled[k]).all(), f"{name}, ingest {k}: flags differ at {np.argwhere(got != veiled[k])[:8].tolist()}"
                assert (m.last_sweeps()[0] == valid[k].any(axis=1)).all()          # (every beam of a built sweep is a hit or a free beam of an accepted one)
                k += 1
            elif st[0] == "packets":
                m.ingest_array(st[1])
                got = m.last_veiled()
                assert (got == veiled[k]).all(), f"{name}, packet ingest {k}: flags differ at {np.argwhere(got != veiled[k])[:8].tolist()}"
                k += 1
            elif st[0] == "place":
                m.bot_veil_place(*st[1:])
            elif st[0] == "forget":
                m.bot_veil_forget(st[1])
            elif st[0] == "reset":
                same_state(state(pkg, m), model.snaps[snap], f"{name}, before reset {snap}")
                snap += 1
                m.reset()
                assert m.bot_veil() == sc.radius and m.bot_veil_sweeps() and not m.bot_veil_cells()[1].any() and m.bot_veil_stats() == 0
        same_state(state(pkg, m), model.snaps[snap], f"{name}, end")


@pytest.mark.parametrize("name", sv.names("radius"))
def test_radius_edge(pkg, name):
    """d^2 == radius^2 is veiled, radius^2 + 1 is not: radius 1, 3, 32, and 5 at the offset (3, 4)."""
    run_scene(pkg, name)


def test_each_lane_and_round_of_the_beam_loop(pkg):
    """Beams 0, 63, 64, 127, 128 and 180 veiled one at a time; slots 181..183 do not exist in the flags."""
    run_scene(pkg, "each-beam")
    _, veiled, _ = sv.model("each-beam")
    assert all(v.shape == (1, 181) for v in veiled)


def test_who_speaks(pkg):
    """An earlier sweep of the call against the table; the later of two; a rejected sweep between; the bot's own later sweep;
    bot_veil_place; after bot_veil_forget and after reset nothing is veiled."""
    run_scene(pkg, "who-speaks")


@pytest.mark.parametrize("name", sv.names("blocks") + ["one-bot-block", "many-bots"])
def test_block_edges(pkg, name):
    run_scene(pkg, name)


@pytest.mark.parametrize("name", ["chunk-edge", "chunk-edge-far"])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_chunk_edge(pkg, name, entry):
    """2^16 + 1 records: the table written back after the first chunk is what the second chunk is seeded from."""
    run_scene(pkg, name, entry=entry)


@pytest.mark.parametrize("name", ["never", "long-beam", "tile-border"])
def test_never_veiled_and_tile_borders(pkg, name):
    run_scene(pkg, name)


def test_the_shared_table(pkg):
    """A sweep bot veils a packet beam of a later qs_ingest; a packet bot veils a sweep beam."""
    run_scene(pkg, "with-packets")


@pytest.mark.parametrize("entry,stride,offset", [("host", 751, 0), ("host", 743, 1), ("device", 751, 1), ("device", 751, 2),
                                                 ("device", 743, 3), ("device", 743, 0)])
def test_entry_points_strides_and_offsets(pkg, entry, stride, offset):
    run_scene(pkg, "mixed-60", entry=entry, stride=stride, offset=offset)


def test_variants_without_counts_with_device_trig_and_forced_tiled(pkg):
    for kw in ({"enable_counts": False}, {"exact_trig": False}, {"raycast_mode": 2}):
        run_scene(pkg, "mixed-60", **kw)
        run_scene(pkg, "tile-border", **kw)


def _plain(pkg, sc, prepare=None, **kw):
    with make(pkg, sc, veil=False, **kw) as m:
        if prepare:
            prepare(m)
        for st in sc.steps:
            assert st[0] == "sweeps"
            ingest(m, st[1])
        out = state(pkg, m)
        out.update(veiled=m.last_sweeps_veiled(), last=m.last_sweeps(), zones={b: m.zone(b) for b in range(1, sc.max_agent + 1)},
                   radius=m.bot_veil(), switch=m.bot_veil_sweeps())
    return out


@pytest.mark.parametrize("n", sv.SMALL_N)
def test_small_calls_take_the_tiled_form(pkg, n):
    """1 and 4 sweeps: a context without the sweep veil sends them through the direct kernel.  With a bot near the flags and the
    map are the rule's; without a bot near the tiled form writes exactly what the direct form writes."""
    run_scene(pkg, f"mixed-{n}")
    run_scene(pkg, f"mixed-{n}-apart")
    sc = sv.get(f"mixed-{n}-apart")
    direct = _plain(pkg, sc)
    tiled = _plain(pkg, sc, lambda m: m.set_bot_veil(sc.radius, sweeps=True))
    assert not tiled["veiled"].any() and tiled["total"] == 0
    for k in ("grid", "stamps", "hits", "misses"):
        assert (direct[k] == tiled[k]).all(), k
    for k in ("rays", "hits", "cells", "accepted", "datagrams"):
        assert direct["counters"][k] == tiled["counters"][k], k


def test_s4_the_rest_sees_the_beam_as_the_filter_judged_it(pkg):
    """last_sweeps, the zone boxes and the counters of a context with the sweep veil equal those of one without it on the same
    stream -- but for QS_CNT_CELLS, which counts cells written: one less per veiled beam."""
    sc = sv.get("mixed-60")
    off = _plain(pkg, sc)
    on = _plain(pkg, sc, lambda m: m.set_bot_veil(sc.radius, sweeps=True))
    assert on["veiled"].any() and not off["veiled"].any()
    assert (on["last"][0] == off["last"][0]).all() and np.array_equal(on["last"][1], off["last"][1], equal_nan=True)
    for b in off["zones"]:
        assert (on["zones"][b] is None) == (off["zones"][b] is None)
        if off["zones"][b] is not None:
            assert (np.asarray(on["zones"][b]) == np.asarray(off["zones"][b])).all()
    c_on, c_off = dict(on["counters"]), dict(off["counters"])
    # (mixed-60 is one ingest: the flags of the last ingest are all of the session's)
    assert c_on.pop("cells") == c_off.pop("cells") - int(on["veiled"].sum()) and on["total"] == int(on["veiled"].sum())
    timing = {k for k in c_on if k.startswith("slam_")}
    assert {k: v for k, v in c_on.items() if k not in timing} == {k: v for k, v in c_off.items() if k not in timing}


def test_off_means_off(pkg):
    """The switch off with the radius on, and the switch on with the radius 0: every output and the table are byte for byte what
    a context that never heard of the switch gives; last_sweeps_veiled is zeros."""
    sc = sv.get("mixed-60")
    never = _plain(pkg, sc)
    cases = {"switch off, radius on": lambda m: m.set_bot_veil(3), "switch on, radius 0": lambda m: m.set_bot_veil(0, sweeps=True),
             "on and off again": lambda m: (m.set_bot_veil(3, sweeps=True), m.set_bot_veil(3, sweeps=False))}
    assert never["radius"] == 0 and never["switch"] is False
    for tag, prepare in cases.items():
        got = _plain(pkg, sc, prepare)
        for k in ("grid", "stamps", "hits", "misses", "xy", "known"):
            assert got[k].tobytes() == never[k].tobytes(), (tag, k)
        assert not got["veiled"].any() and got["veiled"].shape == (60, 181) and got["total"] == 0, tag
        assert not got["known"].any(), tag                         # sweeps do not feed the table either
        for k in ("rays", "hits", "cells", "accepted", "datagrams", "edge_rays"):
            assert never["counters"][k] == got["counters"][k], (tag, k)


def test_the_switch_is_kept(pkg):
    sc = sv.get("mixed-4")
    with make(pkg, sc) as m:
        m.set_bot_veil(5)
        assert m.bot_veil_sweeps() is True and m.bot_veil() == 5   # sweeps=None leaves the switch
        m.set_bot_veil(0)
        assert m.bot_veil_sweeps() is True
        m.reset()
        assert m.bot_veil_sweeps() is True
        m.set_bot_veil(3, sweeps=False)
        assert m.bot_veil_sweeps() is False and m.bot_veil() == 3


def test_refusals(pkg):
    sc = sv.get("mixed-4")
    L = importlib.import_module(pkg.__name__ + "._lib").load()
    with make(pkg, sc) as m:
        buf = np.zeros((4, 181), dtype=np.uint8)
        assert L.qs_last_sweeps_veiled(m._h, buf.ctypes.data, 4) == QS_E_INVAL            # no sweep ingest yet
        ingest(m, sc.steps[0][1])
        assert L.qs_last_sweeps_veiled(m._h, buf.ctypes.data, 3) == QS_E_INVAL
        assert L.qs_last_sweeps_veiled(m._h, buf.ctypes.data, 5) == QS_E_INVAL
        assert L.qs_last_sweeps_veiled(m._h, None, 4) == QS_E_INVAL
        assert L.qs_bot_veil_sweeps(m._h, None) == QS_E_INVAL
        assert L.qs_last_sweeps_veiled(None, buf.ctypes.data, 4) == QS_E_INVAL and L.qs_set_bot_veil_sweeps(None, 1) == QS_E_INVAL
        assert L.qs_last_sweeps_veiled(m._h, buf.ctypes.data, 4) == 0 and m.last_sweeps_veiled().shape == (4, 181)
        m.ingest_array(vr.get("mixed-20").steps[0][1])
        assert L.qs_last_sweeps_veiled(m._h, buf.ctypes.data, 4) == QS_E_INVAL            # the last ingest was no sweep ingest


def test_restore_empties_the_table_and_keeps_the_switch(pkg):
    sc = sv.get("mixed-4")
    with make(pkg, sc) as m:
        ingest(m, sc.steps[0][1])
        assert m.bot_veil_cells()[1][1:].all()
        data = m.checkpoint()
        grid = m.grid_i8()
        m.restore(data)
        assert m.bot_veil() == sc.radius and m.bot_veil_sweeps() and not m.bot_veil_cells()[1].any() and m.bot_veil_stats() == 0
        assert (m.grid_i8() == grid).all()


# ---- the other sweep ingests ----------------------------------------------------------------------------------------------------
def test_a_withheld_record_is_silent_and_unveiled(pkg):
    """The guarded ingest: the record its check contradicts (the one test_sweep_veil_rules_cpu.py finds with the check's own
    restatement) does not speak and has no flags; the scene's later sweeps are veiled by the rule."""
    sc = sv.get("guard")
    model, veiled, _ = sv.model("guard")
    with make(pkg, sc) as m:
        ingest(m, sc.steps[0][1])
        assert not m.last_sweeps_veiled().any()
        ingest(m, sc.steps[1][1], check=True)
        status = m.last_sweep_checks()["status"]
        assert np.nonzero(status == CONTRADICTS)[0].tolist() == [sv.GUARD_WITHHELD], status
        got = m.last_sweeps_veiled()
        assert (got == veiled[1]).all() and not got[sv.GUARD_WITHHELD].any() and got.any()
        assert not m.last_sweeps()[0][sv.GUARD_WITHHELD]
        same_state(state(pkg, m), model.snaps[-1], "guarded")


def test_graph_mode_speaks_from_the_chains_pose(pkg):
    """Graph mode: acceptance, agent and pose come from the batch the chain left; the model is given the poses qs_last_sweeps
    reports (S1) and must give the same flags and map.  (exact_trig off: the chain may move a pose off its cell centre.)"""
    sc = sv.get("mixed-60")
    with make(pkg, sc, exact_trig=False) as m:
        m.set_sweep_graph(True)
        model = sv.SweepVeilModel(sc.g, sc.max_agent, sc.radius)
        ingest(m, sc.steps[0][1])
        acc, pose = m.last_sweeps()
        assert acc.all()
        want, _ = model.ingest_sweeps(sc.steps[0][1], poses=pose)
        got = m.last_sweeps_veiled()
        assert want.any() and (got == want).all()
        got_state, snap = state(pkg, m), vr.snapshot(model)
        for k in ("grid", "stamps", "hits", "misses", "xy", "known"):
            assert (got_state[k] == snap[k]).all(), k
        assert got_state["total"] == snap["total"] and got_state["counters"]["edge_rays"] == 0


class _RoomGeo:
    """match_rules' room as the model's geometry."""
    size, res, ox, oy = MR.ROOM_GRID

    def oracle(self, max_agent=2):
        return orc.OracleMapper(self.size, self.res, self.ox, self.oy, 0.0, max_agent=max_agent)


def test_the_matched_ingest_speaks_from_the_corrected_pose(pkg):
    """match_rules' room: 30 sweeps of two bots in turn whose reported poses are displaced by whole cells; the matched ingest casts
    them from the corrected poses.  The model given those poses gives the device's flags; given the reported poses it gives
    others.  (exact_trig off: a corrected pose is on no cell centre, so nothing here keeps the end points off the cell edges.)"""
    P = importlib.import_module(pkg.__name__ + ".protocol")
    g = _RoomGeo()
    s = MR.room_session(seed=11, n_map=30, n_query=30, window=6, angle_steps=10)
    q = s["q_pose"]
    buf = P.pack_sweeps(1 + np.arange(len(q)) % 2, q[:, 0], q[:, 1], q[:, 2], s["q_ranges"], odometry=True)
    radius = 12
    with pkg.QuasarMapper(g.size, g.res, g.ox, g.oy, exact_trig=False) as m:
        m.set_sweep_filter(MR.ROOM_SMIN, MR.ROOM_SMAX)
        mp = s["map_pose"]
        first = P.pack_sweeps(np.ones(len(mp), int), mp[:, 0], mp[:, 1], mp[:, 2], s["map_ranges"], odometry=True)
        m.set_bot_veil(radius, sweeps=True)
        models = [sv.SweepVeilModel(g, 2, radius, smin=MR.ROOM_SMIN, smax=MR.ROOM_SMAX) for _ in range(2)]
        m.ingest_sweeps(first)
        for mod in models:
            mod.ingest_sweeps(first)
        assert not m.last_sweeps_veiled().any()                  # (bot 1 alone so far)
        m.ingest_sweeps(buf, match=True)
        mt = m.last_sweep_matches()
        assert mt["accepted_match"].sum() >= 25
        acc, pose = m.last_sweeps()
        assert acc.all()
        want, _ = models[0].ingest_sweeps(buf, poses=pose)
        other, _ = models[1].ingest_sweeps(buf)
        got = m.last_sweeps_veiled()
        assert (got == want).all(), f"{int((got != want).sum())} flags differ from the rule at the corrected poses"
        assert want.any() and (want != other).any()
        assert (m.grid_i8() == models[0].grid).all()
        xy, known = m.bot_veil_cells()
        mxy, mknown = models[0].cells()
        assert (xy == mxy).all() and (known == mknown).all() and m.bot_veil_stats() == models[0].total
