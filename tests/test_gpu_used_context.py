"""Every query in a used context.  One qs_ctx lives for a whole mission: writers change the map between queries, and queries of
every kind and size follow one another over shared grow-on-demand workspaces, lazily built tables, the dynamic-LDS attribute of
the kernels and the "last ingest" flags.  The walks of tests/walk_ops.py drive one context through writers and queries in
seeded orders; after every op the answer must equal (==, doubles as bits) the CPU restatement fed the model's map, after every
writer the map must be the oracle's, and every fifth op a new context restored from the used one's checkpoint must answer the
last query the same.  The directed sequences below pin the orders that reuse one workspace or table with other parameters."""
import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import reloc_rules as RR
import walk_ops as W
from conftest import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def lists():
    return W.generate()


_ICP = []


def context(pkg, size):
    """(a new context, its model, its env).  The model's merge session registers with qs_icp of a context of its own that sees
    nothing else: the oracle's icp_planar follows the same steps but ends an ulp away (test_gpu_parity compares it to 1e-9), so the
    exact second opinion of a merge in a used context is the same registration in an unused one."""
    if not _ICP:
        _ICP.append(pkg.QuasarMapper(64, 0.05, -1.6, -1.6))
    return pkg.QuasarMapper(*W.geometry(size)), W.Model(size, register=_ICP[0].icp), W.Env(size, pkg, torch)


def twin_of(pkg):
    def twin(m, model, env):
        t = pkg.QuasarMapper(*W.geometry(model.size))
        t.set_sweep_graph(model.graph_on, **W.GRAPH_PARAMS)      # not in a checkpoint; the sweep filter and dirty tracking are
        t.restore(m.checkpoint())
        tenv = W.Env(model.size, pkg, torch)
        tenv.filt = env.filt
        return t, tenv
    return twin


def sequence(pkg, ops, size=136, tag="sequence", twin=True):
    """A directed op list on a new context, compared op by op with the model; the world is painted first unless the list does."""
    m, model, env = context(pkg, size)
    with m:
        W.walk(m, model, env, ops, tag, twin_of(pkg) if twin else None)
    return model


PAINT = ("update_rays", dict(what="world", seed=1))
FAR = ("set_sweep_filter", dict(smin=0.1, smax=3.0, seed=0))
NEAR = ("set_sweep_filter", dict(smin=0.1, smax=1.2, seed=0))


# ---- the walks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(W.WALKS)))
def test_walk(pkg, lists, k):
    size, seed = W.WALKS[k]
    m, model, env = context(pkg, size)
    with m:
        W.walk(m, model, env, lists[k], f"walk {k} (size {size}, seed {seed})", twin_of(pkg))


# ---- first-caller tables ----------------------------------------------------------------------------------------------------------------
def _sweep_family(seed):
    return {"match": ("match", dict(n=3, stride=751, radius=2, seed=seed)),
            "check_sweeps": ("check_sweeps", dict(n=3, stride=743, seed=seed + 1)),
            "relocalise_sweeps": ("relocalise_sweeps", dict(n=3, stride=751, n_rot=45, box="tile", radius=2, seed=seed + 2)),
            "relocalise_groups": ("relocalise_groups", dict(groups=(4, 1), travel=2.0, n_rot=45, box="tile", radius=2, stride=751, seed=seed + 3))}


@pytest.mark.parametrize("first", ["match", "check_sweeps", "relocalise_sweeps", "relocalise_groups"])
def test_each_sweep_family_call_as_the_first_of_a_context(pkg, first):
    """Whichever of match, check, relocalise and relocalise-groups comes first builds the lazy tables the others then use."""
    fam = _sweep_family(40)
    sequence(pkg, [PAINT, FAR, fam[first]] + [fam[n] for n in fam if n != first] + [fam[first]], tag=f"first caller {first}")


# ---- relocalisation: workspace and table reuse ------------------------------------------------------------------------------------------
def _reloc(box, n_rot=8, n=3, radius=2, seed=7):
    return ("relocalise_sweeps", dict(n=n, stride=751, n_rot=n_rot, box=box, radius=radius, seed=seed))


def _groups(box, n_rot=8, groups=(4, 1), travel=2.0, seed=8):
    return ("relocalise_groups", dict(groups=groups, travel=travel, n_rot=n_rot, box=box, radius=2, stride=751, seed=seed))


def test_relocalise_box_whole_grid_one_cell_whole_grid(pkg):
    sequence(pkg, [PAINT, FAR, _reloc("grid"), _reloc("cell"), _reloc("grid", seed=9), _reloc("empty"), _reloc("tile")], tag="reloc boxes")


def test_relocalise_rotation_table_180_8_180(pkg):
    """reloc_rot is keyed by n_rot alone and shared by the single and the group form."""
    sequence(pkg, [PAINT, FAR, _reloc("tile", 180), _reloc("tile", 8), _reloc("tile", 180), _groups("tile", 8), _reloc("tile", 45),
                   _groups("tile", 45), _groups("tile", 180, groups=(1,)), _reloc("cell", 8)], tag="reloc n_rot")


def test_relocalise_single_and_group_forms_alternate(pkg):
    sequence(pkg, [PAINT, FAR, _reloc("tile", n=65), _groups("cell", groups=(16, 4, 1)), _reloc("cell", n=1), _groups("tile", groups=(1,), travel=0.0),
                   _reloc("grid", n=1), _groups("grid", groups=(1, 1), travel=0.0)], tag="reloc forms")


def test_relocalise_filter_1_2_then_3_0_then_1_2(pkg):
    """At 0.05 m the single form's LDS goes from about 11 KiB to about 41 KiB and back; with travel 2.0 the group form goes from under
    32 KiB to over 64 KiB and back: the dynamic-LDS attribute is set only above 32 KiB and stays at the last value set."""
    sequence(pkg, [PAINT, _reloc("tile"), _groups("tile", travel=0.0), FAR, _reloc("tile"), _groups("tile"), NEAR, _reloc("tile"),
                   _groups("tile", travel=0.0), _groups("tile")], tag="reloc filter")


def test_three_relocalisations_enqueued_without_a_sync(pkg):
    """One tile, the whole grid (the workspace grows while the first launch may still run), one tile: three output buffers, then
    one sync()."""
    m, model, env = context(pkg, 136)
    with m:
        W.walk(m, model, env, [PAINT, FAR], "async reloc")
        args = dict(n=3, stride=751, seed=21)
        buf = W.device_sweeps(m, 136, args, env.filt[1])
        d_buf = torch.from_numpy(buf).cuda()
        boxes = ("tile", "grid", "tile")
        outs = [torch.full((3 * RR.RELOC_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda") for _ in boxes]
        torch.cuda.synchronize()
        for box, d_out in zip(boxes, outs):
            m.relocalise_sweeps_device(d_buf.data_ptr(), 3, buf.shape[1], d_out.data_ptr(), params=dict(n_rot=8, box=W.box_of(136, box)))
        m.sync()
        for box, d_out in zip(boxes, outs):
            want = RR.reloc(model.grid, model.geom, buf, dict(n_rot=8, box=W.box_of(136, box)), None, *model.filt)
            got = d_out.cpu().numpy().view(RR.RELOC_DTYPE)
            assert W.differing(got, want) == "", (box, W.differing(got, want))


# ---- plan_ws: paths, territories and targets carve the same workspace ----------------------------------------------------------------------
def test_territories_layouts_share_the_plan_workspace(pkg):
    both = ("territories", dict(bots=14, owner=True, cost=True, seed=3))
    none = ("territories", dict(bots=14, owner=False, cost=False, seed=3))
    sequence(pkg, [PAINT, both, none, ("targets_by_territory", dict(bots=14, seed=4)), both,
                   ("plan_paths", dict(n=64, clearance=2, seed=5)), ("territories", dict(bots=1, owner=True, cost=False, seed=6)),
                   ("plan_paths", dict(n=1, clearance=2, seed=7)), ("targets_by_path", dict(bots=14, seed=8)), none], tag="plan_ws")


def test_view_layouts(pkg):
    sequence(pkg, [PAINT, ("render_view", dict(width=300, height=200, scale=40.0, zones=4, prims=40, seed=1)),
                   ("render_view", dict(width=1, height=1, scale=100.0, zones=0, prims=0, seed=2)),
                   ("render_view", dict(width=300, height=200, scale=12.0, zones=0, prims=0, seed=3)),
                   ("render_view", dict(width=300, height=200, scale=40.0, zones=1, prims=3, seed=4))], tag="view")


def test_voxel_downsampling_between_two_merges(pkg):
    sequence(pkg, [PAINT, ("merge", dict(seed=0)), ("voxel", dict(n=70001, seed=5)), ("merge", dict(seed=0)), ("voxel", dict(n=1, seed=6)),
                   ("merge", dict(seed=0))], tag="voxel between merges", twin=False)


def test_ingest_sizes_16_5000_16_and_1_65_1(pkg):
    fam = lambda s: [("views", dict(seed=s)), ("plan_paths", dict(n=1, clearance=2, seed=s)), ("frontier", dict(bots=1, seed=s)),
                     ("check_sweeps", dict(n=1, stride=751, seed=s)), ("last", dict(seed=s))]
    ops = [PAINT]
    for s, n in enumerate((16, 5000, 16)):
        ops += [("ingest_packets", dict(n=n, seed=30 + s))] + fam(s)
    for s, (form, n) in enumerate((("plain", 1), ("match", 65), ("check", 1), ("plain", 65), ("match", 1))):
        ops += [("ingest_sweeps_" + form, dict(n=n, stride=751 if s % 2 else 743, seed=40 + s))] + fam(10 + s)
    sequence(pkg, ops, tag="ingest sizes")


# ---- reset and restore ------------------------------------------------------------------------------------------------------------------
def _every_query(seed):
    """One small call of every query a checkpoint covers."""
    rng = np.random.default_rng(seed)
    out = []
    for name in W.QUERIES:
        o = W.OPS[name]
        if name in ("merge", "refused"):
            continue
        sets = o.sets["S" if o.sized else "-"]
        out.append((name, dict(sets[0], seed=int(rng.integers(1 << 30)))))
    return out


def test_after_reset_every_query_is_a_new_contexts(pkg):
    """The merge session and the settings (sweep filter, graph mode) survive a reset, as the header says; everything else is a newly
    created context's."""
    used = [PAINT, FAR, ("ingest_packets", dict(n=5000, seed=1)), ("set_sweep_graph", dict(on=True, seed=0)),
            ("ingest_sweeps_match", dict(n=65, stride=751, seed=2)), ("relocalise_sweeps", dict(n=1, stride=751, n_rot=180, box="grid", radius=2, seed=3)),
            ("territories", dict(bots=14, owner=True, cost=True, seed=4)), ("merge", dict(seed=0)), ("reset", dict(seed=0))]
    m, model, env = context(pkg, 136)
    fresh, fmodel, fenv = context(pkg, 136)
    with m, fresh:
        W.walk(m, model, env, used, "before the reset")
        assert (m.grid_i8() == -1).all() and m.counters()["rays"] == 0
        assert m.sweep_graph()[0] is True and len(m.merge_cloud()) == len(model.session.cloud) > 0
        W.walk(fresh, fmodel, fenv, [FAR, ("set_sweep_graph", dict(on=True, seed=0))], "the new context")
        for name, args in _every_query(5):
            a, b = W.OPS[name].run(m, args, env), W.OPS[name].run(fresh, args, fenv)
            assert W.differing(a, b) == "", (name, W.differing(a, b))
        again = [PAINT, ("ingest_sweeps_plain", dict(n=3, stride=751, seed=6)), ("last", dict(seed=0)), ("merge", dict(seed=0))]
        W.walk(m, model, env, again + _every_query(7), "after the reset", twin_of(pkg))


def test_after_restore_every_query_is_the_checkpointed_models(pkg):
    used = [PAINT, FAR, ("ingest_packets", dict(n=16, seed=1)), ("ingest_sweeps_check", dict(n=65, stride=743, seed=2)),
            ("relocalise_groups", dict(groups=(16, 4, 1), travel=2.0, n_rot=8, box="tile", radius=2, stride=751, seed=3)), ("last", dict(seed=0)),
            ("restore", dict(seed=0)), ("last", dict(seed=0))]
    sequence(pkg, used + _every_query(8) + [("ingest_sweeps_plain", dict(n=1, stride=751, seed=9)), ("last", dict(seed=0))], tag="restore")


def test_a_guarded_ingest_refused_in_graph_mode_leaves_the_last_ingest(pkg):
    """Graph mode refuses the guarded ingest before anything changes: the map, and what the last ingest was, stay."""
    sequence(pkg, [PAINT, ("ingest_sweeps_check", dict(n=3, stride=751, seed=1)), ("last", dict(seed=0)), ("set_sweep_graph", dict(on=True, seed=0)),
                   ("ingest_sweeps_check", dict(n=3, stride=751, seed=2)), ("last", dict(seed=0)), ("views", dict(seed=0)),
                   ("ingest_sweeps_match", dict(n=3, stride=751, seed=3)), ("last", dict(seed=0))], tag="refused guarded ingest")
