"""The op lists of the used-context walks (tests/walk_ops.py), checked without a GPU: what the lists cover, and every op's
expectation run once against the model alone, so that a broken expectation fails here and not on the GPU machine."""
import numpy as np
import pytest

import walk_ops as W


@pytest.fixture(scope="module")
def walks():
    return W.generate()


def test_same_seeds_same_lists(walks):
    assert W.as_literal(W.generate()[0]) == W.as_literal(walks[0])
    assert [W.as_literal(w) for w in W.generate(W.WALKS)] == [W.as_literal(w) for w in walks]
    other = W.generate(tuple((size, seed + 100) for size, seed in W.WALKS))
    assert [W.as_literal(w) for w in other] != [W.as_literal(w) for w in walks]
    for ops in walks:                                          # a list is a literal: it evaluates to itself
        assert eval(W.as_literal(ops)) == ops


def test_no_walk_is_longer_than_60_ops(walks):
    assert len(walks) == len(W.WALKS) == 4 and [size for size, _ in W.WALKS] == [136, 136, 136, 68]
    assert all(0 < len(ops) <= W.MAX_OPS == 60 for ops in walks), [len(ops) for ops in walks]


def test_every_op_occurs_at_least_twice(walks):
    count = dict.fromkeys(W.OPS, 0)
    for ops in walks:
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


def test_every_sized_op_goes_from_large_to_small_and_back(walks):
    for name, o in W.OPS.items():
        if not o.sized:
            continue
        steps = set()
        for ops in walks:
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
