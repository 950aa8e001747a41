"""The op lists of the used-context walks (tests/walk_ops.py), checked without a GPU: what the lists cover, and every op's
expectation run once against the model alone, so that a broken expectation fails here and not on the GPU machine."""
import hashlib

import numpy as np
import pytest

import ray_scenes as RS
import walk_ops as W


@pytest.fixture(scope="module")
def walks():
    return W.generate()


@pytest.fixture(scope="module")
def veil_walks():
    return W.generate_veil()


# SHA-256 of as_literal of the four walks as they stood before the veil and the trail queries joined the op table: new ops must
# not move them
DIGESTS = ("f4d78380c5528be0103a9bbf081cd7db0d3a739e4a8a067c0acb4ca34f615f6f", "19afb19974bcf501e1663a6ac0856b1f7f973bf0369c487f969ee8be8808a50f",
           "73f02eed5cefb2f99a7328e72a8a25b3ead75e3f7184ad443748cdc31ef0cd02", "f720cd573a07aff63121a95cbfe518bef583f405cad068add699a4e92d8ea165")


def test_the_first_four_walks_are_the_lists_they_were(walks):
    assert tuple(hashlib.sha256(W.as_literal(ops).encode()).hexdigest() for ops in walks) == DIGESTS


def test_same_seeds_same_lists(walks):
    assert W.as_literal(W.generate()[0]) == W.as_literal(walks[0])
    assert [W.as_literal(w) for w in W.generate(W.WALKS)] == [W.as_literal(w) for w in walks]
    other = W.generate(tuple((size, seed + 100) for size, seed in W.WALKS))
    assert [W.as_literal(w) for w in other] != [W.as_literal(w) for w in walks]
    assert [W.as_literal(w) for w in W.generate_veil()] == [W.as_literal(w) for w in W.generate_veil(W.VEIL_WALKS)]
    for ops in walks + W.generate_veil():                      # a list is a literal: it evaluates to itself
        assert eval(W.as_literal(ops)) == ops


def test_no_walk_is_longer_than_60_ops(walks, veil_walks):
    assert len(walks) == len(W.WALKS) == 4 and [size for size, _ in W.WALKS] == [136, 136, 136, 68]
    assert len(veil_walks) == len(W.VEIL_WALKS) == 3 and [size for size, _ in W.VEIL_WALKS] == [136, 136, 68]
    assert all(0 < len(ops) <= W.MAX_OPS == 60 for ops in walks + veil_walks), [len(ops) for ops in walks + veil_walks]


def test_every_op_occurs_at_least_twice(walks, veil_walks):
    count = dict.fromkeys(W.OPS, 0)
    for ops in walks + veil_walks:
        for name, _ in ops:
            count[name] += 1
    assert min(count.values()) >= 2, {k: v for k, v in count.items() if v < 2}
    families = {f for ops in walks for name, args in ops if name == "refused" for f in args["families"]}
    assert families == {f for pair in W._REFUSALS for f in pair}, "a family without its refused call"


def test_every_query_directly_follows_every_kind_of_writer(walks):
    """The kinds: a packet ingest, a sweep ingest (any form), update_rays, reset, restore."""
    seen = set()
    for ops in walks:
        for (a, _), (b, _) in zip(ops, ops[1:]):
            if W.OPS[a].pred and W.OPS[b].kind == "query":
                seen.add((W.OPS[a].pred, b))
    missing = [(p, q) for p in W.PREDS for q in W.QUERIES if (p, q) not in seen]
    assert not missing, missing
    assert set(W.PREDS) == {"rays", "packets", "sweeps", "restore", "reset"}


def test_every_sized_op_goes_from_large_to_small_and_back(walks, veil_walks):
    for name, o in W.OPS.items():
        if not o.sized:
            continue
        steps = set()
        for ops in (veil_walks if name in ("match_trails", "relocalise_trails") else walks):
            cls = [args["size_class"] for n, args in ops if n == name]
            steps |= set(zip(cls, cls[1:]))
        assert ("L", "S") in steps and ("S", "L") in steps, (name, steps)


def test_the_relocalisation_forms_follow_each_other_with_another_box(walks):
    pairs = set()
    for ops in walks:
        for (a, x), (b, y) in zip(ops, ops[1:]):
            if {a, b} == {"relocalise_sweeps", "relocalise_groups"} and x["box"] != y["box"]:
                pairs.add((a, b))
    assert pairs == {("relocalise_sweeps", "relocalise_groups"), ("relocalise_groups", "relocalise_sweeps")}, pairs


@pytest.fixture(scope="module")
def answers(walks):
    """Every walk against the model alone (no GPU: the model senses its own sweeps and rotates with libm): per walk a list of
    (name, args, the expectation, whether the map was empty before the op, and after a writer the model's map and what the
    last-ingest calls must say)."""
    out = []
    for k, ops in enumerate(walks):
        model = W.Model(W.WALKS[k][0])
        rows = []
        for name, args in ops:
            empty = bool((model.grid == -1).all())
            want = W.OPS[name].expect(model, args, None)
            writer = W.OPS[name].kind == "writer"
            rows.append((name, args, want, empty, model.grid.copy() if writer else None, W.OPS["last"].expect(model, {}, None) if writer else None))
        out.append(rows)
    return out


@pytest.mark.parametrize("k", range(len(W.WALKS)))
def test_every_expectation_runs_against_the_model_alone(answers, k):
    painted = False
    world = W.world(W.WALKS[k][0])
    for i, (name, args, want, empty, grid, _) in enumerate(answers[k]):
        assert W.differing(want, want) == "", (i, name)
        if name == "update_rays" and args["what"] == "world" and empty:
            assert (grid == world).all(), "painting the world into an empty map must give the world"
            painted = True
        if name == "reset":
            assert (grid == -1).all()
    assert painted


def test_the_answers_are_not_trivial(answers):
    """The walks must ask something: paths that exist and paths that do not, targets, territories, gains, matches that move a
    sweep, checks of every status, a withheld sweep, relocalisations with a score, refusals and answers of the last-ingest calls."""
    rows = [r for walk in answers for r in walk]
    of = lambda name: [r[2] for r in rows if r[0] == name and not isinstance(r[2], W.Refused)]
    status = np.concatenate([w["status"] for w in of("plan_paths")])
    assert (status == 0).sum() > 50 and (status == 1).any()
    for name in ("frontier", "targets_by_path", "targets_by_gain", "targets_by_territory"):
        assert any((w["idx"] >= 0).any() for w in of(name)) and any((w["idx"] < 0).any() for w in of(name)), name
    assert max(int((w["area"] > 0).sum()) for w in of("territories")) >= 10
    assert any(len(w["gain"]) >= 3 and (w["gain"] > 0).all() for w in of("frontier_gain"))
    matches = np.concatenate([w["matches"] for w in of("match")])
    assert matches["accepted_match"].sum() > 50 and (matches["ix"] != 0).any() and (matches["it"] != 0).any()
    checks = np.concatenate([w["checks"] for w in of("check_sweeps")])
    assert set(checks["status"].tolist()) >= {0, 1, 2, 3}, "OK, CONTRADICTS, UNDECIDED and NO_RECORD"
    for name in ("relocalise_sweeps", "relocalise_groups"):
        out = np.concatenate([w["out"] for w in of(name)])
        assert (out["score"] > 0).sum() >= 5 and (out["status"] != 0).any(), name
    last = [r[5] for r in rows if r[5] is not None]               # (the GPU walk asks them after every writer)
    for key in ("last_batch", "last_sweeps", "last_sweep_matches", "last_sweep_checks", "last_sweep_nodes"):
        kinds = {isinstance(w[key], W.Refused) for w in last}
        assert kinds == {True, False}, f"{key}: answered and refused must both occur"
    assert any(isinstance(r[2], W.Refused) for r in rows if r[0] == "ingest_sweeps_check"), "the guarded ingest refused in graph mode"
    held = [int(W.CR.withheld(r[5]["last_sweep_checks"]).sum()) for r in rows if r[0] == "ingest_sweeps_check" and not isinstance(r[2], W.Refused)]
    assert max(held) > 0, "no guarded ingest withheld a sweep"


def test_differing_tells_answers_apart():
    a = dict(x=np.arange(4, dtype=np.int32), y=(np.array([1.0, np.nan]), None), z=W.Refused("a"))
    b = dict(x=np.arange(4, dtype=np.int32), y=(np.array([1.0, np.nan]), None), z=W.Refused("b"))
    assert W.differing(a, b) == ""
    b["x"] = b["x"].copy()
    b["x"][2] = 9
    assert "x" in W.differing(a, b)
    assert W.differing(np.array([0.0]), np.array([-0.0])) != "", "doubles compare as bits"
    assert W.differing(W.Refused("a"), np.zeros(1)) != "" and W.differing(np.zeros(1), W.Refused("a")) != ""
    assert W.differing(dict(a=1), dict(b=1)) != "" and W.differing((1, 2), (1,)) != ""


# ---- the veil walks: what the lists cover ------------------------------------------------------------------------------------------------
def settings_along(ops):
    """Per op (name, args, veil radius, sweep switch, graph mode) as they stand when the op begins."""
    radius, sweeps, graph, out = 0, False, False, []
    for name, args in ops:
        out.append((name, args, radius, sweeps, graph))
        if name == "set_bot_veil":
            radius = args["radius"]
            sweeps = sweeps if args["sweeps"] is None else args["sweeps"]
        if name == "set_sweep_graph":
            graph = args["on"]
    return out


def test_set_bot_veil_covers_every_radius_and_every_switch():
    sets = W.OPS["set_bot_veil"].sets["-"]
    assert {s["radius"] for s in sets} == {0, 3, 8, 32} and {s["sweeps"] for s in sets} == {True, False, None}


def test_veil_walks_every_query_directly_follows_every_kind_of_writer(veil_walks):
    seen = set()
    for ops in veil_walks:
        for (a, _), (b, _) in zip(ops, ops[1:]):
            if W.OPS[a].pred and W.OPS[b].kind == "query":
                seen.add((W.OPS[a].pred, b))
    assert len(W.VEIL_QUERIES) == 10 and set(W.VEIL_QUERIES[:3]) == {"match_trails", "relocalise_trails", "veil_state"}
    missing = [(p, q) for p in W.PREDS for q in W.VEIL_QUERIES if (p, q) not in seen]
    assert not missing, missing


def test_veil_walks_ingest_every_size_and_form_with_the_veil_acting_and_off(veil_walks):
    rows = [r for ops in veil_walks for r in settings_along(ops)]
    packets = {(args["n"], radius > 0) for name, args, radius, _, _ in rows if name == "ingest_packets"}
    assert packets >= {(n, on) for n in (1, 16, 5000) for on in (True, False)}, packets
    sweeps = {(name[len("ingest_sweeps_"):], radius > 0 and sw) for name, args, radius, sw, graph in rows
              if name.startswith("ingest_sweeps_") and not (graph and name.endswith("check"))}
    assert sweeps >= {(f, True) for f in ("plain", "match", "check")} and any(not on for _, on in sweeps), sweeps
    assert any(name.startswith("ingest_sweeps_") and not name.endswith("check") and graph and radius > 0 and sw
               for name, _, radius, sw, graph in rows), "no ingest in graph mode with the sweep veil acting"
    assert any(name == "ingest_sweeps_check" and graph and radius > 0 and sw for name, _, radius, sw, graph in rows), \
        "no guarded ingest refused in graph mode with the sweep veil acting"


def test_veil_walks_switch_the_veil_round_calls_of_one_record(veil_walks):
    """Acting -> off -> acting in one walk: the tiled form, the direct kernel and the tiled form again."""
    def turns(states):
        runs = [s for k, s in enumerate(states) if k == 0 or s != states[k - 1]]
        return any(runs[k:k + 3] == [True, False, True] for k in range(len(runs)))
    packets = [[radius > 0 for name, args, radius, _, _ in settings_along(ops) if name == "ingest_packets" and args["n"] == 1] for ops in veil_walks]
    sweeps = [[radius > 0 and sw for name, args, radius, sw, _ in settings_along(ops) if name.startswith("ingest_sweeps_") and args["n"] == 1]
              for ops in veil_walks]
    assert any(turns(s) for s in packets), packets
    assert any(turns(s) for s in sweeps), sweeps


def test_veil_walks_pair_the_trail_queries_with_their_sweep_forms(veil_walks):
    pairs = set()
    for ops in veil_walks:
        for (a, x), (b, y) in zip(ops, ops[1:]):
            if {a, b} == {"relocalise_trails", "relocalise_groups"} and x["n_rot"] != y["n_rot"] and x["box"] != y["box"] and x["travel"] != y["travel"]:
                pairs.add((a, b))
            if {a, b} == {"match_trails", "match"} and x["radius"] != y["radius"]:
                pairs.add((a, b))
    assert pairs == {("relocalise_trails", "relocalise_groups"), ("relocalise_groups", "relocalise_trails"), ("match_trails", "match"),
                     ("match", "match_trails")}, pairs


# ---- the veil walks against the model alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def veil_answers(veil_walks):
    """Every veil walk against the model alone: per walk a list of dicts -- the op, its expectation, and round an ingest the veil
    flags, whether a veil acted, who had written the table entries of the other bots before it, the table after it."""
    out = []
    for k, ops in enumerate(veil_walks):
        model = W.Model(W.VEIL_WALKS[k][0])
        rows = []
        for (name, args, radius, sweeps, graph) in settings_along(ops):
            ingest = name.startswith("ingest_")
            src = dict(model.veil_src)
            last = model.last
            want = W.OPS[name].expect(model, args, None)
            row = dict(name=name, args=args, want=want, acting=radius > 0 and (sweeps or name == "ingest_packets"), graph=graph, src=src)
            if ingest and not isinstance(want, W.Refused):
                row.update(flags=model.flags.copy(), known=model.veil.cells()[1].copy())
            if isinstance(want, W.Refused):
                row.update(kept=model.last is last)
            if W.OPS[name].kind == "writer":
                row.update(state=W.OPS["veil_state"].expect(model, {}, None), grid_unknown=bool((model.grid == -1).all()),
                           radius=model.veil_radius, sweeps=model.veil_sweeps)
            rows.append(row)
        assert model.min_margin > RS.MARGIN, f"veil walk {k}: an end point {model.min_margin} of a cell from a cell edge: draw another seed"
        out.append(rows)
    return out


@pytest.mark.parametrize("k", range(len(W.VEIL_WALKS)))
def test_every_veil_expectation_runs_against_the_model_alone(veil_answers, k):
    for i, row in enumerate(veil_answers[k]):
        assert W.differing(row["want"], row["want"]) == "", (i, row["name"])
        if row["name"] == "reset":
            assert row["grid_unknown"]


def test_the_veil_answers_are_not_trivial(veil_answers):
    rows = [r for walk in veil_answers for r in walk]
    ingests = [r for r in rows if "flags" in r]
    for n in (1, 16, 5000):
        assert any(r["flags"].any() for r in ingests if r["name"] == "ingest_packets" and r["args"]["n"] == n), f"no veiled beam in a packet ingest of {n}"
    for form in ("plain", "match", "check"):
        assert any(r["flags"].any() for r in ingests if r["name"] == "ingest_sweeps_" + form), f"no veiled beam in a {form} sweep ingest"
    assert any(r["flags"].any() for r in ingests if r["name"].startswith("ingest_sweeps_") and r["args"]["n"] == 1), "no veiled beam in a sweep call of one record"
    assert any(r["flags"].any() for r in ingests if r["name"].startswith("ingest_sweeps_") and r["graph"]), "no veiled beam in graph mode"
    assert not any(r["flags"].any() for r in ingests if not r["acting"]), "a beam veiled while no veil acted"
    # a call of one record hears nobody before its record 0 (bot 1's): whatever veils its beams was in the table when it began
    one = [r for r in ingests if r["args"]["n"] == 1 and r["flags"].any()]
    others = lambda r: {s for b, s in r["src"].items() if b != 1}
    assert any(r["name"] == "ingest_packets" and others(r) == {"sweeps"} for r in one), "no packet beam veiled by a cell only a sweep ingest wrote"
    assert any(r["name"] != "ingest_packets" and others(r) == {"packets"} for r in one), "no sweep beam veiled by a cell only a packet ingest wrote"
    assert any(others(r) == {"place"} for r in one), "no beam veiled through a placed cell"
    forgot = [(a, c) for a, _, b, c in zip(rows, rows[1:], rows[2:], rows[3:])          # the ingest, its query, forget, the same ingest
              if b["name"] == "bot_veil_forget" and a["name"] == c["name"] == "ingest_packets" and a["args"] == c["args"]]
    assert forgot and all(a["flags"].any() and not c["flags"].any() for a, c in forgot), "forget must un-veil the record it veiled before"
    for name in ("reset", "restore"):
        writers = [r for r in rows if "state" in r]
        after = [(a, b) for a, b in zip(writers, writers[1:]) if b["name"] == name]          # the writer before it, the reset or restore
        assert any(a["state"]["cells"][1].any() and not b["state"]["cells"][1].any() and b["state"]["stats"] == 0
                   and b["radius"] > 0 and b["sweeps"] for a, b in after), f"no {name} that empties a table while the settings stand"
    refused = [(a, b) for a, b in zip(rows, rows[1:]) if b["name"] == "ingest_sweeps_check" and isinstance(b["want"], W.Refused) and b["acting"]]
    assert refused and all(b["kept"] and not isinstance(b["state"]["last_veiled"], W.Refused) for a, b in refused), \
        "after the guarded ingest refused in graph mode veil_state must show the ingest before it"
    of = lambda name: [r["want"] for r in rows if r["name"] == name]
    mt = np.concatenate([w["out"] for w in of("match_trails")])
    assert (((mt["ix"] != 0) | (mt["iy"] != 0) | (mt["it"] != 0)) & (mt["accepted_match"] == 1)).sum() >= 2, "no two trail matches that move a trail"
    rt = np.concatenate([w["out"] for w in of("relocalise_trails")])
    assert len(set(rt["status"].tolist())) > 1 and (rt["score"] > 0).sum() >= 5, "trail relocalisations of one status only"
    states = [r["state"] for r in rows if "state" in r]
    for key in ("last_veiled", "last_sweeps_veiled"):
        assert {isinstance(s[key], W.Refused) for s in states} == {True, False}, f"{key}: answered and refused must both occur"
    assert max(s["stats"] for s in states) > 0


def test_with_the_veil_never_on_the_state_is_empty(answers):
    """What walk() now asks after every writer of the first four walks."""
    for k, walk in enumerate(answers):
        model = W.Model(W.WALKS[k][0])
        for name, args, *_ in walk:
            W.OPS[name].expect(model, args, None)
            s = W.OPS["veil_state"].expect(model, {}, None)
            assert model.mo is None and s["radius"] == 0 and s["sweeps"] is False and s["stats"] == 0 and not s["cells"][1].any()
            for key in ("last_veiled", "last_sweeps_veiled"):
                assert isinstance(s[key], W.Refused) or not s[key].any()
