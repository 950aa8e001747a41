"""The free-running chain's closure hand-over (csrc/slam.hip, qs_slam_chain_free_kernel): the owners leave every closure in
the slot of its event's position in the event list, the committer reads a batch's slots a lane each and takes the drift in
force at an event from its agent's last closure before it.  Streams that put several closures of one agent into a batch,
wrap the ring, leave one owner alone for more than two ring lengths, cross launches and resets, and pass poses as given --
every one against oracle.OracleMapper fed the same stream: closure pairs, landmark types and nodes and the grid exact,
corrections, landmark poses and drifts to 1e-9."""
import functools
import importlib

import numpy as np
import pytest
import torch  # before the HIP library (see test_gpu_parity.py)

from conftest import GOLDEN, load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-9                      # the tolerance of test_gpu_parity._chain_equal
TWO_RINGS = 2 * 1024 + 64       # landmark events that wrap the hand-over ring twice at either depth it may have
GRID = (512, 0.05, -12.8, -12.8)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _session():
    replay = importlib.import_module(load_pkg().__name__ + ".replay")
    return replay, replay.telemetry_csv_to_packets()[0]


@functools.lru_cache(maxsize=None)
def _stream(kind, n=0, nb=0, bot=0):
    replay, session = _session()
    if kind == "cycle":
        s = replay.cycle_stream(session, n)
    elif kind == "bots":
        s = replay.multi_bot_stream(session, nb, n, pitch=1.0, origin=(-8.0, -8.0), tiles_per_row=5)
    elif kind == "solo":                                             # one bot's packets of the cycled session
        c = replay.cycle_stream(session, 4 * n)
        s = np.ascontiguousarray(c[c[:, 4] == bot][:n])
        assert len(s) == n
    else:                                                            # one owner far ahead, then both
        s = np.concatenate([_stream("solo", 12500, bot=bot), replay.cycle_stream(session, 4000)])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _oracle(key, min_between, nb=2):
    """The oracle's results for a stream, computed once and shared (read only)."""
    o = orc.OracleMapper(*GRID, 0.0, max_agent=nb)
    o.set_closure_params(0.6, min_between, 0.5)
    o.feed_stream(_stream(*key))
    return o


def _equal(m, o, nb):
    idx, cc = m.closures(0); oi, oc = o.closures(0)
    assert idx.shape == oi.shape and (idx == oi).all()
    assert len(oi) == 0 or np.abs(cc - oc).max() < TOL
    xy, ti = m.landmarks(0); oxy, oti = o.landmarks(0)
    assert ti.shape == oti.shape and (ti == oti).all()
    assert len(oti) == 0 or np.abs(xy - oxy).max() < TOL
    for b in range(1, nb + 1):
        assert np.allclose(m.drift(b), o.drift(b), rtol=0, atol=TOL)
    assert (m.grid_i8() == o.grid).all()
    assert m.counters()["slam_rounds"] < 1 << 40                    # no wait ran out of patience


def _mapper(pkg, min_between, nb=2, form="free"):
    m = pkg.QuasarMapper(*GRID, max_agent=nb, closure_radius=0.6, min_poses_between=min_between, closure_correction=0.5)
    m.set_chain_form(form)
    return m


def _ingest(m, stream, cuts=()):
    lo = 0
    for hi in tuple(cuts) + (len(stream),):
        m.ingest_array(stream[lo:hi]); lo = hi


@pytest.mark.parametrize("form", ["free", "free_posting"])
@pytest.mark.parametrize("min_between", [0, 1, 5, 30])
def test_dense_closures_two_bots(pkg, min_between, form):
    """Without a cool-down nearly every landmark event closes: several closures of one agent in every batch, on adjacent
    lanes, on the first and the last lane of a batch; the ring wraps more than twice.  Whole and cut at 1, 330 and 5000."""
    key = ("cycle", 12000)
    o = _oracle(key, min_between)
    n_cl, n_lm = len(o.closures(0)[0]), len(o.landmarks(0)[1])
    assert n_lm >= TWO_RINGS
    if min_between <= 1:
        assert n_cl >= 0.8 * n_lm
    for cuts in ((), (1, 330, 5000)):
        with _mapper(pkg, min_between, form=form) as m:
            _ingest(m, _stream(*key), cuts)
            assert m.chain_form() == form
            _equal(m, o, 2)


@pytest.mark.parametrize("min_between", [1, 30])
@pytest.mark.parametrize("nb", [1, 5, 6, 13])
def test_agent_counts_at_the_instantiation_edges(pkg, nb, min_between):
    """One graph of 1, 5 (the last of the 8-wave instantiation), 6 (the first of the 16-wave one) and 13 bots (the last
    graph this kernel takes)."""
    key = ("solo", 8000, 0, 1) if nb == 1 else ("bots", 8000, nb)
    o = _oracle(key, min_between, nb)
    assert len(o.closures(0)[0]) > 100
    with _mapper(pkg, min_between, nb) as m:
        _ingest(m, _stream(*key), (3000, 3001))
        assert m.chain_form() == "free"
        _equal(m, o, nb)


@pytest.mark.parametrize("form", ["free", "free_posting"])
@pytest.mark.parametrize("min_between", [1, 30])
@pytest.mark.parametrize("bot", [1, 2])
def test_one_owner_far_ahead(pkg, bot, min_between, form):
    """More than two ring lengths of one bot's events alone -- its owner's wait at the top of a chunk, the other owner idle --
    then both bots: in one launch."""
    key = ("ahead", 0, 0, bot)
    solo = _stream("solo", 12500, bot=bot)
    assert int((solo[:, 41] != 0).sum()) >= TWO_RINGS
    o = _oracle(key, min_between)
    assert len(o.landmarks(0)[1]) >= TWO_RINGS and len(o.closures(0)[0]) > 100
    with _mapper(pkg, min_between, form=form) as m:
        _ingest(m, _stream(*key))
        assert m.chain_form() == form
        _equal(m, o, 2)


def test_reset_and_again(pkg):
    """The same stream before and after a reset: the same results both times."""
    key = ("cycle", 12000)
    o = _oracle(key, 1)
    with _mapper(pkg, 1) as m:
        for _ in range(2):
            _ingest(m, _stream(*key))
            _equal(m, o, 2)
            m.reset()


def test_drift_carried_across_many_launches(pkg):
    """64 launches of 64 packets, then the rest: owners and committer both start every launch from the stored drifts."""
    key = ("cycle", 12000)
    o = _oracle(key, 1)
    with _mapper(pkg, 1) as m:
        _ingest(m, _stream(*key), tuple(64 * (i + 1) for i in range(64)))
        _equal(m, o, 2)


def test_poses_as_given(pkg):
    """qs_slam_add_poses (poses as given: no drift is applied) still records closures and the agents' closure lists.  The poses
    are the ones add_pose saw in an oracle without a cool-down fed the golden session; batches of 1, 63, 64, 65 and the rest."""
    g = np.load(GOLDEN + "/session_512.npz", allow_pickle=False)
    dg = np.ascontiguousarray(g["datagrams"][:, :42])
    o = orc.OracleMapper(*GRID, 0.0)
    o.set_closure_params(0.6, 0, 0.5)
    o.feed_stream(dg)
    poses, agents, lm = np.array(o.poses), np.array(o.pose_agents), dg[:, 41]
    assert len(poses) == len(dg)
    oi, oc = o.closures(0)
    assert len(oi) > 50
    with pkg.QuasarMapper(*GRID, min_poses_between=0) as m:
        m.set_chain_form("free")
        closed, corr, lo = [], [], 0
        for n in (1, 63, 64, 65, len(dg) - 193):
            c, k = m.slam_add_poses(poses[lo:lo + n, 0], poses[lo:lo + n, 1], agents[lo:lo + n], lm[lo:lo + n])
            closed.append(c); corr.append(k); lo += n
        assert lo == len(dg)
        closed, corr = np.concatenate(closed), np.concatenate(corr)
        assert np.nonzero(closed)[0].tolist() == oi[:, 1].tolist()
        assert np.abs(corr[closed == 1] - oc).max() < TOL
        idx, cc = m.closures(0)
        assert idx.shape == oi.shape and (idx == oi).all() and np.abs(cc - oc).max() < TOL
        xy, ti = m.landmarks(0); oxy, oti = o.landmarks(0)
        assert ti.shape == oti.shape and (ti == oti).all() and np.abs(xy - oxy).max() < TOL
        assert m.counters()["slam_rounds"] < 1 << 40
