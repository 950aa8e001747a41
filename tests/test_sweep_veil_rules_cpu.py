"""The sweep veil's restatement (tests/sweep_veil_rules.py) on the CPU: every built scene reaches the case it is named for and no
beam would be left to the host; a built room of sweep bots that face each other, sensed through sim.body_sweep_ranges, has phantom
cells without the veil and none with it; MissionControl hands the switch on and stops placing sweep bots when it is on.  No GPU."""
import importlib

import numpy as np
import pytest

import check_rules as CR
import ray_scenes as rs
import sweep_veil_rules as sv
from conftest import PKG_NAME

OCC = 100
NAMED = [n for n in sv.names() if not n.startswith("mixed")]


def _sweep_ingests(sc):
    """Position among all the scene's ingests of its sweep ingests, in order."""
    kinds = [st[0] for st in sc.steps if st[0] in ("sweeps", "packets")]
    return [j for j, k in enumerate(kinds) if k == "sweeps"]


@pytest.mark.parametrize("name", NAMED)
def test_scene_reaches_its_case(name):
    sc = sv.get(name)
    m, veiled, valid = sv.model(name)
    at = _sweep_ingests(sc)
    assert sc.expect, "a scene without a named case"
    for (ing, rec, beam), want in sc.expect.items():
        assert bool(veiled[at[ing]][rec, beam]) == want, (name, ing, rec, beam, want)
        assert valid[at[ing]][rec, beam] == 1 or not want
    assert any(v.any() for v in veiled), "all flags zero"
    assert set(sc.expect.values()) == {True, False}               # every scene names a veiled beam and one that is not
    assert m.min_margin >= rs.MARGIN                              # exact-trig mode defers nothing: the device decides every beam
    for v, h in zip(veiled, valid):
        assert not (v.astype(bool) & ~h.astype(bool)).any()       # only hits are veiled


def test_beams_from_is_sweep_beams_on_the_records_own_poses():
    sc = sv.get("mixed-60")
    buf = sc.steps[0][1].copy()
    buf[7, 0] = ord("X")
    live = sv.accepted_records(buf, 3)
    own = [(float(r["x"]), float(r["y"]), float(r["yaw"])) for _, r in live]
    a = sv.beams_from(live, own, rs.SMIN_D, rs.SMAX_D)
    b = rs.sweep_beams(sv.as_scene(sc.g, buf, 3))
    assert len(live) == 59 and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_mixed_scenes_veil_some_and_not_all():
    m, veiled, valid = sv.model("mixed-60")
    v, h = veiled[0].astype(bool), valid[0].astype(bool)
    assert v.any() and (h & ~v).any() and not (v & ~h).any() and h.all()
    assert m.min_margin >= rs.MARGIN
    for n in sv.SMALL_N:
        assert len(sv.get(f"mixed-{n}").steps[0][1]) == n
        near, apart = sv.model(f"mixed-{n}"), sv.model(f"mixed-{n}-apart")
        assert not apart[1][0].any() and apart[0].total == 0 and (n == 1 or near[1][0].any())
        assert near[0].min_margin >= rs.MARGIN and apart[0].min_margin >= rs.MARGIN


def test_radius_scenes_sit_on_the_radius():
    """d^2 == radius^2 is veiled, radius^2 + 1 is not; radius 5 at (3, 4): no axis-aligned offset."""
    for name in sv.names("radius"):
        _, veiled, _ = sv.model(name)
        assert [bool(veiled[0][rec, 90]) for rec in (1, 3, 5)] == [True, False, True], name


def test_each_beam_scene_veils_every_lane_and_round():
    sc = sv.get("each-beam")
    _, veiled, _ = sv.model("each-beam")
    assert len(veiled) == len(sv.BEAM_IDS) == 6
    for i, v in zip(sv.BEAM_IDS, veiled):
        hit = np.nonzero(v[0])[0]
        assert v[0, i] and 1 <= len(hit) <= 3 and (abs(hit - i) <= 1).all(), (i, hit)      # the beam, at most with its neighbours
    assert {i >> 6 for i in sv.BEAM_IDS} == {0, 1, 2} and {i & 63 for i in sv.BEAM_IDS} >= {0, 63, 52}


def _records(buf):
    return np.ascontiguousarray(buf).view(rs._P().PACKET_DTYPE_V0_ODO).reshape(-1)


def test_block_scenes_put_speaker_and_beam_on_the_block_edges():
    seen = set()
    for n in sv.BLOCK_N:
        sc = sv.get(f"blocks-{n}")
        for st in sc.steps:
            if st[0] != "sweeps":
                continue
            assert len(st[1]) == n
            rec = _records(st[1])
            for k in np.nonzero(rec["magic"] == b"QSRL")[0]:
                seen.add((n, "bot" if rec["agent"][k] == 2 else "beam", int(k)))
    for n, k in ((257, 255), (257, 256), (256, 255), (255, 254), (4097, 4096), (4097, 255), (4097, 256), (255, 0)):
        assert (n, "bot", k) in seen or (n, "beam", k) in seen, (n, k)
    assert (257, "bot", 255) in seen and (257, "beam", 256) in seen      # the last of a block speaks to the first of the next
    assert (4097, "bot", 256) in seen and (4097, "beam", 4096) in seen
    many = _records(sv.get("many-bots").steps[0][1])
    assert len(set(many["agent"][:256].tolist())) == 255 and sv.get("many-bots").max_agent == 255 and len(many) == 510
    one = _records(sv.get("one-bot-block").steps[0][1])
    assert (one["agent"][256:512] == 1).all() and (one["magic"][256:512] == b"QSRL").all()


def test_chunk_scenes_straddle_the_chunk():
    for name in ("chunk-edge", "chunk-edge-far"):
        rec = _records(sv.get(name).steps[0][1])
        live = np.nonzero(rec["magic"] == b"QSRL")[0].tolist()
        assert len(rec) == sv.CHUNK + 1 and live[0] == 0 and live[-2:] == [sv.CHUNK - 1, sv.CHUNK]
        assert rec["agent"][sv.CHUNK - 1] == 2 and rec["agent"][sv.CHUNK] == 1 and rec["agent"][0] == 3
        _, veiled, _ = sv.model(name)
        assert veiled[0][sv.CHUNK, 90]
    # far: only record 0's bot is within reach of the second chunk's beam
    m, _, _ = sv.model("chunk-edge-far")
    ex, ey = sv.E
    d2 = {b: (x - ex) ** 2 + (y - ey) ** 2 for b, (x, y) in m.table.items()}
    assert d2[3] <= 9 < d2[2]


def test_never_and_long_beam_scenes():
    g = sv.geo()
    o = g.oracle(3)
    sc = sv.get("long-beam")
    rx, ry, hx, hy, valid, slot = rs.sweep_beams(sv.as_scene(g, sc.steps[0][1], 3), rs.SMIN_D, sv.LONG_SMAX)
    dx = np.abs(o.world_to_grid(hx, 0) - o.world_to_grid(rx, 0))
    long = {int(s // rs.SWEEP_SLOTS): int(d) for s, d in zip(slot, dx) if s % rs.SWEEP_SLOTS == 90}
    assert long[1] == 64 and long[3] == 63 and valid.all()
    sc = sv.get("never")
    rx, ry, hx, hy, valid, slot = rs.sweep_beams(sv.as_scene(g, sc.steps[0][1], 3))
    x1 = o.world_to_grid(hx, 0)
    by = {int(s): (int(v), int(x)) for s, v, x in zip(slot, valid, x1) if s % rs.SWEEP_SLOTS == 90}
    assert by[rs.SWEEP_SLOTS * 3 + 90][0] == 0                    # the range-rejected beam
    assert by[rs.SWEEP_SLOTS * 5 + 90] == (1, sv.SIZE + 4)        # a hit that ends outside the grid


def test_the_guard_scene_withholds_its_first_record():
    """The check's own restatement on the map the first ingest leaves: record GUARD_WITHHELD contradicts it, the others do not."""
    sc = sv.get("guard")
    g = sc.g
    mod = sv.SweepVeilModel(g, 3, sc.radius)
    mod.ingest_sweeps(sc.steps[0][1])
    out, _ = CR.check(mod.grid, (g.res, g.ox, g.oy), sc.steps[1][1], max_agent=3)
    assert np.nonzero(CR.withheld(out))[0].tolist() == [sv.GUARD_WITHHELD] == list(sc.steps[1][2]["withheld"])
    _, veiled, valid = sv.model("guard")
    assert not valid[1][sv.GUARD_WITHHELD].any() and not veiled[1][sv.GUARD_WITHHELD].any()


def test_switch_off_or_radius_zero_is_the_plain_oracle():
    sc = sv.get("mixed-60")
    o = rs.feed_oracle(sv.as_scene(sc.g, sc.steps[0][1], sc.max_agent))
    st = rs.sweep_stamps_reference(sv.as_scene(sc.g, sc.steps[0][1], sc.max_agent))
    for kw in (dict(radius=0), dict(sweeps=False)):
        m, veiled, _ = sv.run_model(sc, **kw)
        assert not veiled[0].any() and m.table == {} and m.total == 0
        assert (m.grid == o.grid).all() and (m.hits == o.hits).all() and (m.misses == o.misses).all() and (m.stamps == st).all()
        assert m.n_cells == o.n_cells_written


def test_with_packets_shares_one_table():
    m, veiled, _ = sv.model("with-packets")
    assert veiled[1].shape[1] == 4 and veiled[1][0, 0] and veiled[2][0, 90] and not veiled[2][1, 90]
    assert sorted(m.table) == [1, 2, 3]


# ---- sim.body_sweep_ranges ------------------------------------------------------------------------------------------------------
def _sim():
    return importlib.import_module(PKG_NAME + ".sim")


def test_body_sweep_ranges_agrees_with_body_ranges_on_the_shared_beams():
    """Beams 90, 180 and 0 of a sweep point where a packet's front, left and right sensors point."""
    sim = _sim()
    rng = np.random.default_rng(5)
    pose = np.concatenate([rng.uniform(-1.0, 1.0, (6, 2)), rng.uniform(-3.0, 3.0, (6, 1))], axis=1)
    pose[:, 2] = np.array([np.arctan2(pose[(k + 1) % 6, 1] - pose[k, 1], pose[(k + 1) % 6, 0] - pose[k, 0]) for k in range(6)])
    agent = np.array([1, 2, 3, 1, 2, 3])
    world = rng.uniform(0.0, 3.0, (6, 181)).astype(np.float32)
    world[:, ::7] = 0.0
    got = sim.body_sweep_ranges(pose, agent, world, 0.15, 3.0)
    four = sim.body_ranges(pose, agent, np.stack([world[:, 90], world[:, 180], world[:, 0], world[:, 0]], axis=1), 0.15, 3.0)
    assert got.shape == (6, 181) and got.dtype == np.float32
    assert np.allclose(got[:, 90], four[:, 0], rtol=0, atol=1e-6) and np.allclose(got[:, 180], four[:, 1], rtol=0, atol=1e-6)
    assert np.allclose(got[:, 0], four[:, 3], rtol=0, atol=1e-6)
    assert (got[:, 90] < world[:, 90]).any() or (world[:, 90] == 0).any()
    changed = got != world
    assert changed.any() and (got[changed] <= 3.0).all() and not np.shares_memory(got, world)
    same = agent[:, None] == agent[None, :]
    alone = sim.body_sweep_ranges(pose[:1], agent[:1], world[:1], 0.15, 3.0)
    assert same[0, 3] and (alone == world[:1]).all()              # nobody else: nothing changes


# ---- the built room -------------------------------------------------------------------------------------------------------------
def _room(radius):
    sim = _sim()
    g = sv.geo()
    body = sv.ROOM_BODY * g.res
    buf = sv.room_stream(lambda pose, agent, ranges: sim.body_sweep_ranges(pose, agent, ranges, body, rs.SMAX_D))
    m = sv.SweepVeilModel(g, 4, radius)
    for b, (x, y, _) in zip((b for b, *_ in sv.ROOM_BOTS), sv.room_poses()):
        m.place(b, x, y)                                         # the bots are known before the first sweep (as after one round)
    veiled, _ = m.ingest_sweeps(buf)
    return m, veiled, buf


def test_room_phantoms_without_the_veil_and_none_with_it():
    world = sv.room_world()
    off, v_off, buf = _room(0)
    on, v_on, _ = _room(sv.ROOM_RADIUS)
    assert sv.ROOM_RADIUS >= sv.ROOM_BODY + 1.5                    # the bound body / res + 1.5 for a stationary bot
    walls = sv.room_wall_ranges()
    rec = _records(buf)
    assert (rec["ranges"][:4] < walls).any() and (rec["ranges"][:4] <= walls).all()        # bodies shorten some beams, lengthen none
    phantom_off = (off.grid == OCC) & (world == 0)
    phantom_on = (on.grid == OCC) & (world == 0)
    assert not v_off.any() and phantom_off.sum() > 0
    assert v_on.any() and phantom_on.sum() == 0, np.argwhere(phantom_on).tolist()
    wall_off, wall_on = (off.grid == OCC) & (world == OCC), (on.grid == OCC) & (world == OCC)
    assert wall_off.sum() > 40 and (wall_off == wall_on).all()    # the walls are drawn, and the same with the veil
    yy, xx = np.mgrid[0:sv.SIZE, 0:sv.SIZE]
    for _, dx, dy, _ in sv.ROOM_BOTS:
        near = (xx - (sv.ROOM_C + dx)) ** 2 + (yy - (sv.ROOM_C + dy)) ** 2 <= sv.ROOM_RADIUS ** 2
        assert not (near & (world == OCC)).any()                  # no wall cell lies within the radius of a bot
    assert on.cells()[1].tolist() == [0, 1, 1, 1, 1] and on.total == int(v_on.sum())


# ---- the front end --------------------------------------------------------------------------------------------------------------
def _front():
    from test_veil_frontend_cpu import VeilStub, _sock
    from test_check_frontend_cpu import R181, _fe

    class SweepVeilStub(VeilStub):
        def set_bot_veil(self, radius=3, sweeps=None):
            self.calls.append(("set_bot_veil", radius, sweeps))

    return SweepVeilStub, _sock, R181, _fe


def test_the_switch_reaches_set_bot_veil():
    Stub, _sock, R181, _fe = _front()
    fe, P = _fe()
    mc = fe.MissionControl(Stub(), sock=_sock(), bot_veil={"radius": 5, "sweeps": True})
    assert mc.mapper.calls == [("set_bot_veil", 5, True)] and mc.bot_veil and mc.bot_veil_sweeps
    mc = fe.MissionControl(Stub(), sock=_sock(), bot_veil={"sweeps": True})
    assert mc.mapper.calls == [("set_bot_veil", P.BOT_VEIL_RADIUS, True)] and mc.bot_veil_sweeps
    mc = fe.MissionControl(Stub(), sock=_sock(), bot_veil={"radius": 4, "sweeps": False})
    assert mc.mapper.calls == [("set_bot_veil", 4, False)] and not mc.bot_veil_sweeps
    for opt in (True, {"radius": 4}, {}):
        mc = fe.MissionControl(Stub(), sock=_sock(), bot_veil=opt)
        assert mc.mapper.calls[0][2] is None and mc.bot_veil and not mc.bot_veil_sweeps      # the switch is left alone


def test_placement_is_skipped_with_the_switch_on_and_done_with_it_off():
    Stub, _sock, R181, _fe = _front()
    fe, P = _fe()
    for opt, places in (({"radius": 3, "sweeps": True}, 0), ({"radius": 3, "sweeps": False}, 2), ({"radius": 3}, 2), (True, 2)):
        sock = _sock()
        mc = fe.MissionControl(Stub(), sock=sock, sweeps=True, bot_veil=opt)
        sock.put(P.pack_v0(1, 1.0, 0.5, 0.0, R181), P.pack_v0(2, 4.0, 0.25, 0.0, R181), P.pack_v0(1, 1.5, 0.75, 0.0, R181))
        assert mc.poll(now=1.0) == 3
        names = [c[0] for c in mc.mapper.calls]
        assert names == ["set_bot_veil", "sweeps"] + ["place"] * places, (opt, names)
        if places:
            assert sorted(mc.mapper.calls[2:]) == [("place", 1, 1.5, 0.75), ("place", 2, 4.0, 0.25)]
        # a bot found offline is forgotten either way
        assert mc.heartbeat(now=1.0 + P.HEARTBEAT_TIMEOUT + 0.5) == [1, 2]
        assert [c for c in mc.mapper.calls if c[0] == "forget"] == [("forget", 1), ("forget", 2)]
