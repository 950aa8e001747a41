"""The look-ahead word of the bucket chains on the device (csrc/qs_internal.h QsLmNode; written by chain_insert_lanes in
csrc/slam.hip, read by the lean owner in csrc/slam_chain_decide.inc).  Every case runs six times -- the look-ahead on
(default), off (the same load on the node's last entry), the lean owner off; each with the plan on and off -- and compares
closures (index pairs and corrections), landmarks, drifts and slam_sizes byte for byte between the six, and with
oracle.OracleMapper fed the same stream (index pairs, landmark nodes and types exact; corrections, poses and drifts to 1e-9).
No wait may have run out of patience (bit 40 of slam_rounds).

The scenes are tests/chain_lookahead_rules.py's; tests/test_chain_lookahead_cpu.py proves from the restatement that each
reaches its case: a closure that only a walk past seven entries out of reach finds (a writer that skips the look-ahead store,
or a reader that ignores an older entry behind it, loses that closure), the same in the third and fourth node, a walk that
the look-ahead avoids, chains of exactly 7, 8, 14 and 15, several pool nodes for one bucket and for two buckets in one batch.

slam_node_iters counts the lean owner's decisions that its first rows did not settle.  It is compared between look-ahead on
and off over the LAST launch of a case whose earlier launches laid every landmark the askers can see: the index is complete
when that launch starts, so what a decision sees does not depend on how far the committer has got, and the counts are the
restatement's.  With the look-ahead on it is never above the run with it off, strictly below on the scenes built to avoid a
walk, equal where nothing can be avoided.  Over a launch that lays and asks at once the count depends on the committer's
timing by a few decisions in either direction; there it is printed, and the results are compared."""
import functools
import importlib

import numpy as np
import pytest
import torch  # before the HIP library (see test_gpu_parity.py)

import chain_lookahead_rules as R
from conftest import load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-9
P_, Q_ = (0.05, 0.05), (0.75, 0.35)        # tests/k4_adversarial.py's pile and the place next to it
RUNS = tuple((plan, mode) for plan in (True, False) for mode in ("ahead", "last", "general"))


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _stream(key):
    if key[0] == "scene":
        return R.scene_stream(key[1])[0]
    if key[0] == "legs":
        return R.legs_stream(key[1])[0]
    replay = importlib.import_module(load_pkg().__name__ + ".replay")
    session = replay.telemetry_csv_to_packets()[0]
    if key[0] == "cycle":
        s = replay.cycle_stream(session, key[1])
    else:                                                            # "bots"
        s = replay.multi_bot_stream(session, key[2], key[1], pitch=1.0, origin=(-8.0, -8.0), tiles_per_row=5)
    s = np.ascontiguousarray(s)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _oracle(key, min_between, nb, bpg=0):
    """The oracle's results for a stream, computed once and shared (read only)."""
    o = orc.OracleMapper(*R.GRID, 0.0, max_agent=nb, bots_per_graph=bpg)
    o.set_closure_params(R.RADIUS, min_between, 0.5)
    o.feed_stream(_stream(key))
    return o


def _equal(m, o, nb, n_graphs):
    for g in range(n_graphs):
        idx, cc = m.closures(g); oi, oc = o.closures(g)
        assert idx.shape == oi.shape and (idx == oi).all()
        assert len(oi) == 0 or np.abs(cc - oc).max() < TOL
        xy, ti = m.landmarks(g); oxy, oti = o.landmarks(g)
        assert m.slam_sizes(g)[1] == len(oti)
        assert ti.shape == oti.shape and (ti == oti).all()
        assert len(oti) == 0 or np.abs(xy - oxy).max() < TOL
    for b in range(1, nb + 1):
        assert np.allclose(m.drift(b), o.drift(b), rtol=0, atol=TOL)
    assert m.counters()["slam_rounds"] < 1 << 40                    # bit 40: a wait ran out of patience


def _bytes(m, nb, n_graphs):
    out = []
    for g in range(n_graphs):
        idx, cc = m.closures(g); xy, ti = m.landmarks(g)
        out += [idx.tobytes(), cc.tobytes(), xy.tobytes(), ti.tobytes(), repr(m.slam_sizes(g)).encode()]
    return b"".join(out + [m.drift(b).tobytes() for b in range(1, nb + 1)])


def _mapper(pkg, nb, min_between, bpg, plan, mode, limit):
    m = pkg.QuasarMapper(*R.GRID, max_agent=nb, bots_per_graph=bpg, closure_radius=R.RADIUS, min_poses_between=min_between,
                         closure_correction=0.5)
    m.set_chain_form("free")
    m.set_chain_lean("off" if mode == "general" else "auto", limit)
    m.set_chain_plan(plan)
    m.set_chain_lookahead(mode == "ahead")
    assert m.chain_lookahead() == (mode == "ahead")
    return m


def _run(pkg, key, min_between, nb=3, cuts=(), bpg=0, limit=0, lean=True, before=None, restore_at=None):
    """The stream in the six ways, each equal to the oracle, all byte for byte the same.  cuts: where the ingests end.
    before: a stream ingested and reset away first.  restore_at: the session is checkpointed after that many ingests and goes
    on in a fresh context restored from it.  lean: what chain_lean() must say after every launch of the lean runs (one value,
    or one per launch).  Returns {(plan, mode): (slam_node_iters of the last launch, of the whole run)}."""
    o = _oracle(key, min_between, nb, bpg)
    stream = _stream(key)
    n_graphs = 1 if bpg == 0 else (nb + bpg - 1) // bpg
    ends = tuple(cuts) + (len(stream),)
    want = list(lean) if isinstance(lean, (list, tuple)) else [lean] * len(ends)
    out, images = {}, []
    for plan, mode in RUNS:
        m = _mapper(pkg, nb, min_between, bpg, plan, mode, limit)
        try:
            if before is not None:
                m.ingest_array(_stream(before)); m.sync(); m.reset()
            said, lo, n0 = [], 0, 0
            for i, hi in enumerate(ends):
                if restore_at == i:
                    data = m.checkpoint()
                    m.close()
                    m = _mapper(pkg, nb, min_between, bpg, plan, mode, limit)
                    m.restore(data)
                n0 = m.counters()["slam_node_iters"]
                m.ingest_array(stream[lo:hi]); lo = hi
                said.append(m.chain_lean())
            assert m.chain_form() == "free"
            assert said == (want if mode != "general" else [False] * len(ends))
            _equal(m, o, nb, n_graphs)
            n1 = m.counters()["slam_node_iters"]
            out[(plan, mode)] = (n1 - n0, n1)
            images.append(_bytes(m, nb, n_graphs))
        finally:
            m.close()
    assert all(b == images[0] for b in images)
    print(key[0], key[1] if key[0] != "legs" else len(stream), min_between, {f"{'plan' if p else 'chunks'}/{md}": v for (p, md), v in out.items()})
    return out


def _counts(out, expect):
    """slam_node_iters of the last launch, look-ahead on against off."""
    for plan in (True, False):
        on, off = out[(plan, "ahead")][0], out[(plan, "last")][0]
        assert on <= off
        assert (on < off) if expect == "fewer" else (on == off)


@pytest.mark.parametrize("name", R.SCENES)
def test_scene_laid_by_the_launch_before(pkg, name):
    """MIN_POSES_BETWEEN 30, the ingest split in front of the askers: the deciding entries, and the look-ahead words behind
    them, were written by the launch before."""
    _counts(_run(pkg, ("scene", name), 30, cuts=(R.scene_stream(name)[1],)), R.EXPECT[name])


@pytest.mark.parametrize("name", R.SCENES)
def test_scene_in_one_launch(pkg, name):
    """Laying and asking in one launch: the askers' owners stand at their first candidate when the kernel starts, ahead of the
    committer, and that decision goes to the general query and waits for the frontier."""
    _run(pkg, ("scene", name), 30)


@pytest.mark.parametrize("min_between", [0, 1])
@pytest.mark.parametrize("name", ["deciding", "third", "avoid", "len15", "two"])
def test_short_cool_downs(pkg, name, min_between):
    """Every packet a decision, the bots drifting towards what they match; split in front of the askers."""
    out = _run(pkg, ("scene", name), min_between, cuts=(R.scene_stream(name)[1],))
    for plan in (True, False):
        assert out[(plan, "ahead")][0] <= out[(plan, "last")][0]


def test_deciding_entry_just_behind_the_frontier(pkg):
    """One launch; the deciding entry at node 17, the first round's match at node 18.  Bot 2's first event, node 47 at a place
    of its own, finds nothing and so waits until the frontier stands at its limit, node 17; its next, node 48 at Q, has node
    18 for its limit: the frontier is there by then and the lean owner walks to node 17's entry, or it is not and the
    general query waits for it."""
    legs = ((1, R.A, 7), (1, R.FAR, 10), (1, R.B, 1), (1, R.Q, 1), (1, R.FAR, 28), (2, (-6.05, -6.05), 1), (2, R.Q, 3))
    key = ("legs", legs)
    cl = _oracle(key, 30, 3).closures(0)[0]
    assert [17, 48] in cl.tolist()
    _run(pkg, key, 30)


@pytest.mark.parametrize("name", ["deciding", "avoid"])
def test_after_a_reset(pkg, name):
    """A session with longer chains at the same places first (its look-ahead words point at other entries), then qs_reset."""
    _counts(_run(pkg, ("scene", name), 30, cuts=(R.scene_stream(name)[1],), before=("scene", "batch")), R.EXPECT[name])


@pytest.mark.parametrize("name", ["deciding", "avoid", "batch", "two"])
def test_after_checkpoint_and_restore(pkg, name):
    """The askers come to a context restored from a checkpoint: the chains, and every look-ahead word, are the rebuild's --
    64 log entries a batch, so 22 entries of one bucket, and two buckets' eighth entries, arrive in one."""
    _counts(_run(pkg, ("scene", name), 30, cuts=(R.scene_stream(name)[1],), restore_at=1), R.EXPECT[name])


@pytest.mark.parametrize("name", ["deciding", "avoid"])
def test_after_the_node_table_has_grown(pkg, name):
    """1064 packets of padding in a launch of their own, each at a place of its own more than a radius from every other (no
    pile, no closure): the graph's arrays, the node table among them, are grown (from 1024 landmarks to 2048) and copied,
    look-ahead words included, between the laying and the asking."""
    lay = R.scene_legs(name)[:-2]
    rows = [-12.0 + 0.65 * r for r in range(16)] + [4.5 + 0.65 * r for r in range(12)]     # (clear of the scene's places)
    pad = tuple((1, (-12.4 + 0.65 * c, y), 1) for y in rows for c in range(38))
    legs = lay + pad + ((2, R.Q, 3),)
    n_lay = sum(n for _, _, n in lay)
    assert n_lay + len(pad) > 1024
    _counts(_run(pkg, ("legs", legs), 30, cuts=(n_lay, n_lay + len(pad))), R.EXPECT[name])


def test_lean_limit_crossed(pkg):
    """The lean owner stops at 5000 nodes; launches of 3000 packets: the first runs it, the others the general owner -- on
    chains whose look-ahead words the lean launch's committer and theirs wrote alike."""
    _run(pkg, ("cycle", 12000), 5, nb=2, cuts=(3000, 6000, 9000), limit=5000, lean=[True, False, False, False])


def test_lean_switched_off_and_on_between_launches(pkg):
    """qs_set_chain_lean between launches: the general owner's launch appends (its committer writes the look-ahead words), the
    lean owner's next launch reads them."""
    name = "deciding"
    stream, n_lay = R.scene_stream(name)
    o = _oracle(("scene", name), 30, 3)
    with _mapper(pkg, 3, 30, 0, True, "general", 0) as m:
        m.ingest_array(stream[:n_lay])
        assert not m.chain_lean()
        m.set_chain_lean("auto", 0)
        m.set_chain_lookahead(True)
        m.ingest_array(stream[n_lay:])
        assert m.chain_lean()
        _equal(m, o, 3, 1)


def test_four_graphs_in_one_launch(pkg):
    key = ("bots", 8000, 8)
    o = _oracle(key, 5, 8, 2)
    assert all(len(o.closures(g)[0]) > 10 for g in range(4))
    _run(pkg, key, 5, nb=8, bpg=2)


def test_landmark_pile(pkg):
    """The pile of tests/k4_adversarial.py, as small as raises the pile flag (a bucket chain of more than 64 pool nodes), in a
    graph of six bots on offer: the launches after the flag run <true, 16, false>, whose lean owner keeps to the chunks and
    hands every decision with a bucket to walk to the general query -- fewer of them with the look-ahead."""
    legs = ((1, P_, 7 * 66 + 3), (2, Q_, 200))
    key = ("legs", legs)
    n = 7 * 66 + 3 + 200
    assert len(_oracle(key, 5, 6).closures(0)[0]) > 20
    with pkg.QuasarMapper(*R.GRID, max_agent=6, closure_radius=R.RADIUS, min_poses_between=5, closure_correction=0.5) as m:
        m.ingest_array(_stream(key))
        m.sync()
        assert m.counters()["slam_rounds"] < 1 << 40
    _run(pkg, key, 5, nb=6, cuts=(n - 150, n - 100, n - 50))
