"""tests/closure_rules.py checked on the CPU: the list scan against the two statements of the reference's path the project
already has (oracle/pymapper.py on poses as given, oracle/oracle.c on packets), the index restatement
(tests/chain_lookahead_rules.py, Chains.query) against the list scan on every query of every scene -- hash collisions included
--, and the sensitivity of the scenes: every wrong variant of the scan is told from the scan by the scenes built to catch it.
That last part is the evidence that tests/test_gpu_closure_fields.py would fail on a kernel with the same mistake."""
import numpy as np
import pytest

import closure_rules as C
from conftest import load_pkg
from oracle import oracle as orc
from oracle.pymapper import PyMapper

NBS = (2, 6, 20)
REFERENCE = [n for n in C.SCENES if n.startswith("ring-0.6") and not n.endswith("lds")
             or n in ("age_edges-30", "cell_edges", "types_share_cells", "dense_ring", "dense_ring-64") or n.split("-")[0] in
             ("far_collision", "neighbour_collision")]


def _pack(sc):
    n = len(sc.x)
    z = np.zeros(n, dtype=int)
    return np.ascontiguousarray(load_pkg().pack_packets(sc.agent.astype(int), sc.x, sc.y, np.zeros(n), z, z, np.zeros((n, 4)),
                                                        sc.type.astype(int)))


def _same(a, b):
    assert a["pairs"].shape == b["pairs"].shape and (a["pairs"] == b["pairs"]).all()
    assert a["corr"].tobytes() == b["corr"].tobytes()
    assert a["lm_ti"].shape == b["lm_ti"].shape and (a["lm_ti"] == b["lm_ti"]).all()
    assert a["lm_xy"].tobytes() == b["lm_xy"].tobytes()
    assert a["drift"] == b["drift"] and a["asked"] == b["asked"] and a["n_nodes"] == b["n_nodes"]


@pytest.mark.parametrize("name", C.SCENES)
def test_every_scene_builds_and_scan_answers_what_it_was_built_for(name):
    """Building a scene asserts its premise (closure_rules.Build.ask, and each builder's own assertions).  scan() on the
    scene's arrays gives what the builder's event-by-event scan gave, and closes exactly where the scene says."""
    for nb in NBS:
        for raw in (True, False) if name in C.PACKET else (True,):
            if not raw and nb == 20:
                continue
            sc = C.scene(name, nb, raw)
            got = C.scan(sc.x, sc.y, sc.agent, sc.type, raw=raw, **sc.params)
            _same(got, sc.ref)
            closing = {node: want for want, node in sc.want}
            assert all(closing[int(n)] == int(l) for l, n in got["pairs"] if int(n) in closing)
            assert {n for n, w in closing.items() if w is not None} <= {int(n) for _, n in got["pairs"]}
            if sc.f32:
                assert np.float32(sc.x).astype(np.float64).tobytes() == sc.x.tobytes()
                assert np.float32(sc.y).astype(np.float64).tobytes() == sc.y.tobytes()


def test_ring_classes():
    """Every direction has its three points, and the scan closes on the "below" one alone: 8 closures for 24 askers."""
    for r in C.RING_RADII:
        pts = C.ring_points(0.03, -0.02, r)
        assert len(pts) == 8 and all(set(p) == set(C.CLASSES) for p in pts.values())
        for v in C.RING_VARIANTS:
            sc = C.scene(f"ring-{r}-{v}")
            assert sum(w is not None for w, _ in sc.want) == 8 and len(sc.want) == 24
    for name in ("dense_ring", "dense_ring-64"):
        assert sum(w is not None for w, _ in C.scene(name).want) == 8 and len(C.scene(name).want) == 24


@pytest.mark.parametrize("name", REFERENCE)
def test_scan_equals_pymapper_on_poses_as_given(name):
    """oracle.pymapper.PyMapper.add_pose at the reference's constants: closures with their corrections, and the landmark list."""
    for nb in (2, 6):
        sc = C.scene(name, nb, True)
        assert sc.params == C.REF
        p = PyMapper(*sc.world)
        for i in range(len(sc.x)):
            p.add_pose(float(sc.x[i]), float(sc.y[i]), int(sc.agent[i]), int(sc.type[i]))
        ref = sc.ref
        assert [(c[0], c[1]) for c in p.closures] == [tuple(v) for v in ref["pairs"].tolist()]
        assert np.array([c[2:] for c in p.closures], dtype=np.float64).reshape(-1, 2).tobytes() == ref["corr"].tobytes()
        assert [(l[2], l[3]) for l in p.landmarks] == [tuple(v) for v in ref["lm_ti"].tolist()]
        assert np.array([l[:2] for l in p.landmarks], dtype=np.float64).reshape(-1, 2).tobytes() == ref["lm_xy"].tobytes()
        assert p.n_nodes == ref["n_nodes"]


@pytest.mark.parametrize("name", C.PACKET)
def test_scan_equals_the_oracle_on_packets(name):
    """oracle.OracleMapper fed the scene as packets (pose = value + drift): pairs, corrections, log and drifts bit for bit."""
    for nb in (2, 6):
        sc = C.scene(name, nb, False)
        o = orc.OracleMapper(*sc.world, 0.0, max_agent=nb)
        o.set_closure_params(sc.radius, sc.min_between, sc.correction)
        assert o.feed_stream(_pack(sc)) == len(sc.x)
        ref = sc.ref
        oi, oc = o.closures(0)
        assert oi.shape == ref["pairs"].shape and (oi == ref["pairs"]).all() and oc.tobytes() == ref["corr"].tobytes()
        oxy, oti = o.landmarks(0)
        assert oti.shape == ref["lm_ti"].shape and (oti == ref["lm_ti"]).all() and oxy.tobytes() == ref["lm_xy"].tobytes()
        for b in range(1, nb + 1):
            assert tuple(o.drift(b)) == ref["drift"].get(b, (0.0, 0.0))
        assert o.n_nodes(0) == ref["n_nodes"]


@pytest.mark.parametrize("name", C.SCENES)
def test_the_index_restatement_finds_what_the_list_finds(name):
    """Chains.query -- nine buckets, node by node, by either rule -- on every query of the scene for a type the directory
    indexes, against the scan's answer."""
    for raw in (True, False) if name in C.PACKET else (True,):
        sc = C.scene(name, 2, raw)
        ch = sc.chains()
        ch.check_lookahead()
        asked = [a for a in sc.ref["asked"] if 1 <= a[3] <= C.NTYPES]
        assert asked or name.endswith("-t7")                  # (the side list is no part of the index)
        for node, x, y, t, match in asked:
            eff = node - max(sc.min_between, 1)
            assert ch.scan(x, y, t, eff) == match
            for rule in ("last", "ahead"):
                assert ch.query(x, y, t, eff, rule)[0] == match, (name, node, rule)


def test_collisions_are_exercised():
    """What the collision scenes rest on, stated once more from the outside: C1 and C2 lie apart and share an entry, the
    asker at C2 needs more than one round, and the cell with two neighbours on one entry has them in its own nine."""
    for world in (200, 64):
        c1, c2 = C.far_cells(world)
        g = C.Geometry(*C.WORLDS[world], 0.6)
        assert g.key(5, *c1) == g.key(5, *c2) and max(abs(c1[0] - c2[0]), abs(c1[1] - c2[1])) > 2
        c, a, b = C.neighbour_cells(world)[:3]
        assert a != b and g.key(5, *a) == g.key(5, *b) and all(max(abs(v[0] - c[0]), abs(v[1] - c[1])) <= 1 for v in (a, b))
        for n1 in C.FAR_COUNTS:
            sc = C.scene(f"far_collision-{world}-{n1}")
            node, x, y, t, match = [q for q in sc.ref["asked"] if q[4] == n1][0]            # the asker at C2
            assert sc.chains().query(x, y, t, node - sc.min_between, "last")[1:3] == (n1 // C.CAP + 1, False)


CAUGHT_BY = {
    "le": [n for n in C.SCENES if n.startswith(("ring", "dense_ring"))],
    "rr": [n for n in C.SCENES if n.startswith(("ring-0.6", "ring-0.3", "ring-0.45"))],
    "notype": ["types_share_cells"],
    "cell": [n for n in C.SCENES if n.startswith(("far_collision", "neighbour_collision"))],
    "rows": [n for n in C.SCENES if n.startswith("far_collision")],
}


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_sensitivity(mutant):
    """The wrong variant closes elsewhere than the scan on every scene named for it -- on both routes where the scene has two."""
    assert CAUGHT_BY[mutant]
    for name in CAUGHT_BY[mutant]:
        for raw in (True, False) if name in C.PACKET else (True,):
            sc = C.scene(name, 2, raw)
            got = C.scan(sc.x, sc.y, sc.agent, sc.type, raw=raw, mutant=mutant, geom=sc.geom(), **sc.params)
            assert got["pairs"].tolist() != sc.ref["pairs"].tolist(), (mutant, name, raw)


def test_the_right_scan_is_not_told_from_itself():
    """The mutant switch left alone, with the geometry passed in as the mutants need it: the scan's own answer."""
    for name in ("far_collision-200-15", "neighbour_collision-64", "ring-0.45-t5"):
        sc = C.scene(name)
        _same(C.scan(sc.x, sc.y, sc.agent, sc.type, raw=True, geom=sc.geom(), **sc.params), sc.ref)


def test_graphs_of_one_bot():
    """scan_graphs on the field laid and asked twice over, a graph per bot: every bot closes on its own first pass, and bots 2
    and 3 find nothing of bot 1's field, which one graph for all would have them close on."""
    x, y, agent, lm, params = C.graphs_case()
    per = C.scan_graphs(x, y, agent, lm, 1, raw=True, **params)
    one = C.scan(x, y, agent, lm, raw=True, **params)
    assert set(per) == {0, 1, 2} and all(len(r["pairs"]) >= 3 for r in per.values())
    assert sum(r["n_nodes"] for r in per.values()) == len(x) == one["n_nodes"]
    assert sum(len(r["pairs"]) for r in per.values()) < len(one["pairs"])
