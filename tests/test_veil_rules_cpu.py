"""The bot veil's restatement (tests/veil_rules.py) on the CPU: every built scene reaches the case it is named for, its flags
differ from all-zero, no ray would be left to the host; and on a built room the veil does what it is for -- four stationary
bots that face each other leave phantom cells without it and none with it.  No GPU."""
import importlib

import numpy as np
import pytest

import ray_scenes as rs
import veil_rules as vr
from conftest import PKG_NAME

OCC = 100


@pytest.mark.parametrize("name", [n for n in vr.names() if not n.startswith("mixed")])
def test_scene_reaches_its_case(name):
    sc = vr.get(name)
    m, veiled, valid = vr.model(name)
    assert sc.expect, "a scene without a named case"
    for (ing, slot, s), want in sc.expect.items():
        assert bool(veiled[ing][slot, s]) == want, (name, ing, slot, s, want)
        assert valid[ing][slot, s] == 1 or not want
    assert any(v.any() for v in veiled), "all flags zero"
    assert set(sc.expect.values()) == {True, False}               # every scene names a veiled beam and one that is not
    assert m.min_margin >= rs.MARGIN                              # exact-trig mode defers nothing: the device decides every ray


def test_mixed_scenes_veil_some_and_not_all():
    m, veiled, valid = vr.model("mixed-300")
    v, h = veiled[0].astype(bool), valid[0].astype(bool)
    assert v.any() and (h & ~v).any() and not (v & ~h).any()
    assert m.min_margin >= rs.MARGIN
    for n in vr.SMALL_N:
        assert len(vr.get(f"mixed-{n}").steps[0][1]) == n


def test_radius_scenes_sit_on_the_radius():
    """d^2 == radius^2 is veiled, radius^2 + 1 is not; radius 5 at (3, 4): no axis-aligned offset."""
    for name in vr.names("radius"):
        sc = vr.get(name)
        _, veiled, _ = vr.model(name)
        assert [bool(veiled[0][slot, 0]) for slot in (1, 3, 5)] == [True, False, True], name
    m5, veiled, _ = vr.model("radius-5")
    assert m5.radius == 5


def test_block_scenes_put_speaker_and_beam_on_the_block_edges():
    seen = set()
    for n in vr.BLOCK_N:
        sc = vr.get(f"blocks-{n}")
        for st in sc.steps:
            if st[0] != "ingest":
                continue
            assert len(st[1]) == n
            tags = list(st[2])
            seen |= {(n, t, k) for k, t in enumerate(tags) if t in ("bot", "beam")}
    for n, slot in ((257, 255), (257, 256), (256, 255), (255, 254), (4097, 4096), (4097, 255), (4097, 256), (255, 0)):
        assert (n, "bot", slot) in seen or (n, "beam", slot) in seen, (n, slot)
    assert (257, "bot", 255) in seen and (257, "beam", 256) in seen      # the last of a block speaks to the first of the next
    many = vr.get("many-bots")
    agents = np.ascontiguousarray(many.steps[0][1]).view(rs._P().PACKET_DTYPE).reshape(-1)["agent"]
    assert len(set(agents[:256].tolist())) == 255 and many.max_agent == 255
    one = vr.get("one-bot-block")
    agents = np.ascontiguousarray(one.steps[0][1]).view(rs._P().PACKET_DTYPE).reshape(-1)["agent"]
    assert (agents[256:512] == 1).all()


def test_radius_zero_is_the_plain_oracle():
    sc = vr.get("mixed-300")
    m, veiled, _ = vr.run_model(sc, radius=0)
    o = sc.g.oracle(sc.max_agent)
    o.feed_stream(sc.steps[0][1])
    assert not veiled[0].any() and m.table == {}
    assert (m.grid == o.grid).all() and (m.stamps == o.stamps).all() and (m.hits == o.hits).all() and (m.misses == o.misses).all()
    assert m.n_cells == o.n_cells_written


# ---- the built room ---------------------------------------------------------------------------------------------------------
def _room(radius):
    sim = importlib.import_module(PKG_NAME + ".sim")
    g = vr.geo()
    body = vr.ROOM_BODY * g.res
    buf = vr.room_stream(lambda pose, agent, ranges: sim.body_ranges(pose, agent, ranges, body, rs.MAX_D))
    m = vr.VeilModel(g, 4, radius)
    veiled, _ = m.ingest(buf)
    return m, veiled, buf


def test_room_bodies_shorten_the_facing_beams():
    _, _, buf = _room(0)
    rec = buf.view(rs._P().PACKET_DTYPE).reshape(-1)
    g = vr.geo()
    # every bot faces the one opposite, 2 A cells away: its front beam stops on that body, the others reach the walls
    assert (rec["front"] == g.dist(2 * vr.ROOM_A - vr.ROOM_BODY)).all()
    for (_, _, _, _, d), r in zip(vr.room_ranges(), rec[:4]):
        assert [r["left"], r["back"], r["right"]] == [g.dist(d[1]), g.dist(d[2]), g.dist(d[3])]


def test_room_phantoms_without_the_veil_and_none_with_it():
    world = vr.room_world()
    off, v_off, _ = _room(0)
    on, v_on, _ = _room(vr.ROOM_RADIUS)
    assert vr.ROOM_RADIUS >= vr.ROOM_BODY + 1.5                    # the bound body / res + 1.5 for a stationary bot
    assert off.min_margin >= rs.MARGIN
    phantom_off = (off.grid == OCC) & (world == 0)
    phantom_on = (on.grid == OCC) & (world == 0)
    assert not v_off.any() and phantom_off.sum() > 0
    assert v_on.any() and phantom_on.sum() == 0
    # the walls: the same OCCUPIED cells as without the veil, except those within the radius of a bot's cell
    near = np.zeros_like(world, dtype=bool)
    yy, xx = np.mgrid[0:vr.SIZE, 0:vr.SIZE]
    for _, cx, cy, _, _ in vr.room_ranges():
        near |= (xx - cx) ** 2 + (yy - cy) ** 2 <= vr.ROOM_RADIUS ** 2
    wall_off, wall_on = (off.grid == OCC) & (world == OCC), (on.grid == OCC) & (world == OCC)
    assert wall_off.sum() == 12 and (wall_off & ~near == wall_on & ~near).all()
    lost = np.argwhere(wall_off & ~wall_on)
    assert len(lost) == 0, lost.tolist()                           # (the bots stand 7 cells from the walls: none lies that near)
    assert on.cells()[1].tolist() == [0, 1, 1, 1, 1]
