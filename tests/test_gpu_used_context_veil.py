"""The bot veil and the trail queries in a used context.  The veil reroutes every ingest to the tiled form, keeps flags in
workspaces laid out from sizes an earlier call left (`veil_ws` from `cap_batch`; `sveil_ws` from the chunk size and call size of
`qs_sweep_veil_reserve`), answers for them later behind `last_veil` and `last_sveil`, and shares one table between packets,
sweeps and `qs_bot_veil_place`; the trail relocaliser shares the rotation table, the workspace and one kernel's sticky
dynamic-LDS attribute with the group form, the trail matcher the window core and `io_ws` with the sweep matcher.  The veil walks
of tests/walk_ops.py drive one context through all of it in a built order; the directed lists below pin the orders that reuse a
workspace, a flag or a table with other sizes or settings.  Every comparison is `==` (doubles as bits) with the model of
walk_ops.py: veil_rules / sweep_veil_rules for the veil, trail_rules / trail_reloc_rules for the trails."""
import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import match_rules as MR
import ray_scenes as RS
import walk_ops as W
from conftest import load_pkg
from test_gpu_used_context import FAR, NEAR, PAINT, context, sequence, twin_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def lists():
    return W.generate_veil()


def veil(radius, sweeps=None):
    return ("set_bot_veil", dict(radius=radius, sweeps=sweeps, seed=0))


def packets(n, seed):
    return ("ingest_packets", dict(n=n, seed=seed, clear=True))


def sweeps(form, n, seed, stride=751):
    return ("ingest_sweeps_" + form, dict(n=n, stride=stride, seed=seed))


def place_at(ingest, beam, bot=2):
    """Bot `bot` on the end of beam `beam` of record 0 of the ingest op (record 0 is bot 1's)."""
    name, args = ingest
    return ("bot_veil_place", dict(bot=bot, x=None, y=None, at=(name, args["n"], args["seed"]), beam=beam, seed=0))


STATE = ("veil_state", dict(seed=0))
VIEWS = ("views", dict(seed=0))
LAST = ("last", dict(seed=0))
GRAPH_ON, GRAPH_OFF = ("set_sweep_graph", dict(on=True, seed=0)), ("set_sweep_graph", dict(on=False, seed=0))
FORGET_ALL = ("bot_veil_forget", dict(bot=None, seed=0))


def hit_beam(size, ingest):
    """A beam of the ingest's record 0 that is a hit, from the middle of those that are; None without one."""
    name, args = ingest
    hits = [k for k in range(4 if name == "ingest_packets" else MR.BEAMS) if W.beam_of(size, (name, args["n"], args["seed"]), k)[2]]
    return hits[len(hits) // 2] if hits else None


def seen(size, ingest):
    """The ingest with the first seed, counting on in thousands, at which its record 0 has a beam that is a hit."""
    name, args = ingest
    while hit_beam(size, (name, args)) is None:
        args = dict(args, seed=args["seed"] + 1000)
    return name, args


def placed(size, ingest):
    ingest = seen(size, ingest)
    return [place_at(ingest, hit_beam(size, ingest)), ingest]


# ---- the walks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(W.VEIL_WALKS)))
def test_veil_walk(pkg, lists, k):
    size, seed = W.VEIL_WALKS[k]
    m, model, env = context(pkg, size)
    with m:
        W.walk(m, model, env, lists[k], f"veil walk {k} (size {size}, seed {seed})", twin_of(pkg))


# ---- workspaces laid out from an earlier call's sizes --------------------------------------------------------------------------------------
def test_ingest_sizes_under_a_standing_veil(pkg):
    """Packets of 16, 5000, 16: veil_ws grows with cap_batch and is then read at the old size.  Sweeps of 1, 65, 1 with the switch
    on: the chunk size and the call size of the sweep veil's workspace change from call to call."""
    ops = [veil(32, True), PAINT]
    for s, n in enumerate((16, 5000, 16)):
        ops += [packets(n, 50 + s), STATE]
    for s, n in enumerate((1, 65, 1)):
        ops += (placed(136, sweeps("plain", n, 60 + s)) if n == 1 else [sweeps("plain", n, 60 + s)]) + [STATE, LAST]
    model = sequence(pkg, ops, tag="sizes under a veil")
    assert model.veil.total > 0 and model.min_margin > RS.MARGIN


def test_the_veil_switched_round_calls_of_one_record(pkg):
    """Radius 3 -> 0 -> 3 round packet ingests of one record (tiled, direct, tiled), the sweep switch on -> off -> on round sweep
    ingests of one record; the same record each time, with bot 2 standing on the end of one of its beams."""
    one, sw = seen(136, packets(1, 70)), seen(136, sweeps("plain", 1, 71))
    ops = [PAINT, veil(3, True)] + placed(136, one) + [VIEWS, STATE, veil(0), one, VIEWS, STATE, veil(3), one, VIEWS, STATE]
    ops += [place_at(sw, hit_beam(136, sw)), sw, VIEWS, STATE, veil(3, False), sw, VIEWS, STATE, veil(3, True), sw, VIEWS, STATE, LAST]
    sequence(pkg, ops, tag="veil switched")


# ---- what the last ingest was -----------------------------------------------------------------------------------------------------------
def test_every_kind_of_ingest_after_a_veiled_one(pkg):
    """S7 and qs_last_veiled after: an ingest with the veil off (zeros), a sweep ingest of nothing (no last ingest), a sweep ingest
    refused for its stride and a guarded ingest refused in graph mode (both leave the last ingest and its flags), an ingest of
    the other kind (refused)."""
    size = 68
    first = sweeps("match", 3, 80)
    again = lambda s: placed(size, sweeps("match", 3, s))
    ops = [PAINT, veil(32, True)] + placed(size, first) + [STATE, LAST]
    ops += [veil(32, False), sweeps("plain", 3, 81), STATE, veil(32, True)]                       # an unveiled sweep ingest
    ops += again(82) + [sweeps("plain", 0, 83), STATE, LAST]                                      # a sweep ingest of nothing
    ops += again(84) + [sweeps("match", 3, 85, stride=700), STATE, LAST]                          # refused: stride
    ops += [GRAPH_ON, sweeps("check", 3, 86), STATE, LAST, GRAPH_OFF]                             # refused: graph mode
    ops += [packets(16, 87), STATE, LAST]                                                         # a packet ingest
    ops += [sweeps("plain", 3, 88, stride=700), STATE, GRAPH_ON, sweeps("check", 1, 89), STATE, GRAPH_OFF]      # the same after packets
    ops += [veil(0), packets(16, 90), STATE, veil(32), sweeps("check", 3, 91), STATE, LAST]
    model = sequence(pkg, ops, size=size, tag="after a veiled ingest")
    assert model.veil.total > 0


# ---- one table ---------------------------------------------------------------------------------------------------------------------------
def test_one_table_for_packets_sweeps_and_placed_bots(pkg):
    size = 68
    ops = [PAINT, veil(32, True)]
    for s in (100, 110):
        one = seen(size, packets(1, s))
        ops += placed(size, one) + [STATE, sweeps("plain", 3, s + 1), STATE, sweeps("match", 3, s + 2, stride=743), STATE,
                                    ("bot_veil_forget", dict(bot=2, seed=0)), one, STATE, ("reset", dict(seed=0)), PAINT]
    ops += [packets(16, 120), sweeps("plain", 3, 121), ("restore", dict(seed=0)), STATE, packets(1, 122), sweeps("check", 1, 123), STATE]
    model = sequence(pkg, ops, size=size, tag="one table")
    assert (model.veil_radius, model.veil_sweeps) == (32, True)


# ---- trails and groups: one kernel, one rotation table, one workspace ---------------------------------------------------------------------
def _groups(travel, n_rot=8, seed=8):
    return ("relocalise_groups", dict(groups=(4, 1), travel=travel, n_rot=n_rot, box="tile", radius=2, stride=751, seed=seed))


def _trails(travel, n_rot=8, trails=1, records=4, box="tile", seed=9):
    return ("relocalise_trails", dict(trails=trails, records=records, stride=42, n_rot=n_rot, box=box, radius=2, travel=travel, seed=seed))


def test_trails_against_groups_over_the_sticky_lds_attribute(pkg):
    """The group kernel's dynamic LDS: over 64 KiB for the groups at 3.0 m and travel 2.0, under 32 KiB for trails at the smallest
    reach (the attribute is set only above 32 KiB and stays), over 64 KiB again; then the rotation table 8 -> 180 -> 8 across
    relocalise_sweeps and relocalise_trails."""
    single = lambda n_rot, seed: ("relocalise_sweeps", dict(n=3, stride=751, n_rot=n_rot, box="tile", radius=2, seed=seed))
    sequence(pkg, [PAINT, FAR, _groups(2.0), _trails(0.0), _groups(2.0, seed=10), _trails(0.0, trails=65, seed=11), single(8, 12),
                   _trails(0.6, n_rot=180, seed=13), single(8, 14), _trails(3.0, n_rot=8, records=64, box="cell", seed=15), NEAR, _groups(0.0, seed=16),
                   _trails(0.0, seed=17)], tag="trails and groups")


@pytest.mark.parametrize("first", ["match_trails", "relocalise_trails"])
def test_a_trail_call_as_the_first_of_the_sweep_family(pkg, first):
    """Whichever comes first builds the lazy tables (match_tab, reloc_rot) and sizes io_ws for the others."""
    fam = {"match_trails": ("match_trails", dict(trails=65, records=4, stride=41, radius=2, travel=4.0, seed=30)),
           "match": ("match", dict(n=3, stride=751, radius=2, seed=31)),
           "check_sweeps": ("check_sweeps", dict(n=3, stride=743, seed=32)),
           "relocalise_trails": ("relocalise_trails", dict(trails=1, records=64, stride=42, n_rot=45, box="tile", radius=2, travel=0.6, seed=33))}
    sequence(pkg, [PAINT, FAR, fam[first]] + [fam[n] for n in fam if n != first] + [fam[first]], tag=f"first caller {first}")


# ---- dirty tracking -----------------------------------------------------------------------------------------------------------------------
def test_a_veiled_context_marks_the_blocks_a_veil_off_context_marks(pkg):
    """Dirty tracking on; a veiled packet ingest and a veiled sweep ingest.  A twin context with the veil off is fed the same rays
    through update_rays with `valid & ~veiled` (a veiled beam is a free ray without its end cell, V5 / S4): the same map, the same
    blocks marked."""
    size = 68
    pk, sw = packets(16, 130), sweeps("plain", 3, 131)
    m, model, env = context(pkg, size)
    t, _, _ = context(pkg, size)
    with m, t:
        W.walk(m, model, env, [("dirty_tracking", dict(on=True, seed=0)), PAINT, veil(32, True), pk], "dirty, veiled")
        v4 = m.last_veiled().reshape(-1)
        swept = W.device_sweeps(m, size, sw[1], env.filt[1])       # what the op is about to sense: the map does not change in between
        W.walk(m, model, env, [sw], "dirty, veiled")
        v181 = m.last_sweeps_veiled()
        assert v4.any() and v181.any(), "nothing was veiled"
        t.dirty_tracking(True)
        for batch in W.rays_of(size, PAINT[1]):
            t.update_rays(*batch)
        buf = W.packets_of(size, pk[1])
        rec = np.ascontiguousarray(buf).view(W.protocol().PACKET_DTYPE).reshape(-1)
        acc = (rec["magic"] == b"QSRL") & (rec["agent"] >= 1) & (rec["agent"] <= 2)
        d = np.stack([rec[k] for k in ("front", "left", "back", "right")], axis=1).astype(np.float64)[acc]
        ok = (RS.MIN_D < d) & (d <= RS.MAX_D)
        length = np.where(ok, d, np.where(d > RS.MIN_D, np.minimum(d, RS.MAX_D), RS.MAX_D))
        a = rec["yaw"].astype(np.float64)[acc][:, None] + np.array(RS.SENSOR_ANG)[None, :]
        rx, ry = np.repeat(rec["x"].astype(np.float64)[acc], 4), np.repeat(rec["y"].astype(np.float64)[acc], 4)
        keep = ok.reshape(-1) & (v4.reshape(-1, 4)[acc].reshape(-1) == 0)
        t.update_rays(rx, ry, rx + (length * np.cos(a)).reshape(-1), ry + (length * np.sin(a)).reshape(-1), keep.astype(np.uint8))
        recs = MR.records_of(swept)
        srx, sry, shx, shy, valid = W.sweep_beams(recs, smin=env.filt[0], smax=env.filt[1])
        accs = np.array([r["magic"] == b"QSRL" and 1 <= int(r["agent"]) <= 2 for r in recs])
        t.update_rays(srx, sry, shx, shy, (valid.astype(bool) & (v181[accs].reshape(-1) == 0)).astype(np.uint8))
        why = W.differing(dict(grid=t.grid_i8(), counts=t.counts()), dict(grid=m.grid_i8(), counts=m.counts()), "twin map")
        assert why == "", why
        assert t.dirty_blocks() == m.dirty_blocks() and m.dirty_blocks()[0] > 0
