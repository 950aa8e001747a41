"""Graph mode of the sweep path on the GPU (qs_set_sweep_graph): signatures, nodes, closures, drift and zone boxes against the
restatement (tests/sweep_graph_rules.py), the grid against the reference's update_ray driven beam by beam from the poses the
device reports."""
import importlib
import os
import socket

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import match_rules as MR
import sweep_graph_rules as R
from conftest import GOLDEN, load_pkg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
FLOAT_TOL = 1e-5          # tests/test_gpu_parity.py's


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _P(pkg):
    return importlib.import_module(pkg.__name__ + ".protocol")


CUTS = [1, 8]             # calls of 1, 7 and the rest
RESTORE_AT = 300
# records of the room stream made unacceptable, one of every kind, mid-call and either side of every call cut
REJECTS = {7: "magic", 8: "agent0", 100: "agent3", 101: "length", 150: "nan_x", 200: "nan_yaw", 299: "inf_y", 300: "magic", 610: "agent0"}


def _spoil(buf, lens, k, how):
    f32 = lambda v: np.frombuffer(np.float32(v).tobytes(), np.uint8)
    if how == "magic":
        buf[k, :4] = np.frombuffer(b"QSRX", np.uint8)
    elif how == "agent0":
        buf[k, 4] = 0
    elif how == "agent3":
        buf[k, 4] = 3                                          # max_agent + 1
    elif how == "length":
        lens[k] = buf.shape[1] - 8
    elif how == "nan_x":
        buf[k, 5:9] = f32(np.nan)
    elif how == "inf_y":
        buf[k, 9:13] = f32(np.inf)
    elif how == "nan_yaw":
        buf[k, 13:17] = f32(np.nan)


@pytest.fixture(scope="module")
def room(pkg):
    """The room stream with REJECTS spoilt, packed, with the restatement's answer -- computed once, never changed.  A record with
    a NaN pose is what graph mode's one acceptance decision rejects and the plain path does not.  `clean`: the stream unspoilt."""
    agent, x, y, yaw, ranges = R.room_stream()
    n = len(agent)
    clean = _P(pkg).pack_sweeps(agent, x, y, yaw, ranges, odometry=True)
    buf, lens = clean.copy(), np.full(n, clean.shape[1], dtype=np.uint16)
    ok = np.ones(n, dtype=bool)
    for k, how in REJECTS.items():
        _spoil(buf, lens, k, how)
        ok[k] = False
    recs = MR.records_of(buf)
    assert np.array_equal(R.signatures_of_records(recs, buf.shape[1], lens) != R.LM_REJECTED, ok)
    sg = R.SweepGraph()
    node, lm, pose, chain = sg.add_sweeps(agent, x, y, yaw, ranges, ok=ok)
    g = sg.graphs[0]
    owner = {int(k): int(a) for k, a in zip(node, agent) if k >= 0}
    # the conditions of the clean stream (tests/test_sweep_graph_cpu.py) still hold with the gaps in it
    assert len(g.closures) >= 4 and any(owner[li] != owner[ni] for li, ni, _, _ in g.closures)
    assert np.flatnonzero(node == max(ni for _, ni, _, _ in g.closures))[0] >= 0.9 * n
    assert node[RESTORE_AT + 1] == RESTORE_AT + 1 - (~ok[:RESTORE_AT + 1]).sum()      # numbering goes on past the gaps
    return dict(agent=agent, x=x, y=y, yaw=yaw, ranges=ranges, sg=sg, node=node, lm=lm, pose=pose, chain=chain, buf=buf, lens=lens,
                ok=ok, clean=clean)


def _stamps(pkg, m):
    distmod = importlib.import_module(pkg.__name__ + ".dist")
    st, _ = distmod.grid_tensors(m, torch.device("cuda", 0))
    torch.cuda.synchronize()
    return st.cpu().numpy().copy()


def _graph_state(m, graph=0):
    idx, corr = m.closures(graph)
    xy, ti = m.landmarks(graph)
    return dict(sizes=tuple(m.slam_sizes(graph)), idx=idx, corr=corr, agents=np.asarray(m.closure_agents(graph)), xy=xy, ti=ti)


def _assert_graph(st, g, tag):
    """Device graph == restatement Graph: indices, types and sizes exactly, and -- the arithmetic is the same uncontracted
    fp64 -- the corrections and landmark positions exactly too."""
    assert st["sizes"] == (g.n_nodes, len(g.landmarks), len(g.closures)), f"{tag}: sizes {st['sizes']}"
    assert st["idx"].tolist() == [[li, ni] for li, ni, _, _ in g.closures], f"{tag}: closures"
    assert st["agents"].tolist() == list(g.closure_agents), f"{tag}: closure agents"
    assert st["ti"].tolist() == [[t, li] for _, _, t, li in g.landmarks], f"{tag}: landmarks"
    want_c = np.array([[dx, dy] for _, _, dx, dy in g.closures]).reshape(-1, 2)
    want_l = np.array([[lx, ly] for lx, ly, _, _ in g.landmarks]).reshape(-1, 2)
    print(f"{tag}: max |closure corr diff| {np.abs(st['corr'] - want_c).max(initial=0.0):.3e}, "
          f"max |landmark diff| {np.abs(st['xy'] - want_l).max(initial=0.0):.3e}")
    assert np.array_equal(st["corr"], want_c), f"{tag}: closure corrections"
    assert np.array_equal(st["xy"], want_l), f"{tag}: landmark positions"


def _ingest_in_calls(m, buf, lens, cuts, **kw):
    """The stream in calls cut at `cuts`: (node, lm, accepted, pose) of all records, concatenated."""
    out = [[], [], [], []]
    edges = [0] + list(cuts) + [len(buf)]
    for a, b in zip(edges[:-1], edges[1:]):
        m.ingest_sweeps(buf[a:b], lens[a:b], **kw)
        node, lm = m.last_sweep_nodes()
        acc, pose = m.last_sweeps()
        for o, v in zip(out, (node, lm, acc, pose)):
            o.append(v)
    return [np.concatenate(o) for o in out]


def _oracle_of_poses(pose, acc, ranges, size=200, res=0.05, ox=-5.0, oy=-5.0):
    o = orc.OracleMapper(size, res, ox, oy)
    ks = np.nonzero(acc)[0]
    o.update_rays(*MR.beams_of_all(pose[ks], ranges[ks], R.SMIN, R.SMAX))
    return o


def _same_map(m, o, tag):
    g = m.grid_i8()
    assert (g == o.grid).all(), f"{tag}: {(g != o.grid).sum()} cells differ from the oracle"
    h, mi = m.counts()
    assert (h == o.hits).all() and (mi == o.misses).all(), f"{tag}: counters differ"


def _room_outputs(pkg, room, mode, cuts, restore_at=None):
    """Everything test 2 looks at, of one run."""
    m = pkg.QuasarMapper(raycast_mode=mode)
    try:
        m.set_sweep_graph(True)
        if restore_at is None:
            node, lm, acc, pose = _ingest_in_calls(m, room["buf"], room["lens"], cuts)
        else:
            first = _ingest_in_calls(m, room["buf"][:restore_at], room["lens"][:restore_at], [])
            data = m.checkpoint()
            m.close()
            m = pkg.QuasarMapper(raycast_mode=mode)
            assert m.sweep_graph()[0] is False
            m.restore(data)
            assert m.sweep_graph()[0] is False, "qs_restore must leave the context's setting alone"
            m.set_sweep_graph(True)
            rest = _ingest_in_calls(m, room["buf"][restore_at:], room["lens"][restore_at:], [])
            node, lm, acc, pose = (np.concatenate([a, b]) for a, b in zip(first, rest))
        return dict(node=node, lm=lm, acc=acc, pose=pose, graph=_graph_state(m), drift=[m.drift(b) for b in (1, 2)],
                    zone=[m.zone(b) for b in (1, 2)], grid=m.grid_i8(), counts=m.counts(), counters=m.counters(),
                    stamps=_stamps(pkg, m))
    finally:
        m.close()


def _assert_room(out, room, tag):
    n = len(room["agent"])
    sg = room["sg"]
    ok = room["ok"]
    assert np.array_equal(out["node"], room["node"]) and np.array_equal(out["lm"], room["lm"]), f"{tag}: nodes / signatures"
    assert (out["node"][~ok] == -1).all() and (out["lm"][~ok] == R.LM_REJECTED).all() and (~ok).sum() == len(REJECTS)
    assert np.array_equal(out["acc"], ok.astype(np.uint8)), f"{tag}: accepted flags"
    assert np.isnan(out["pose"][~ok]).all() and np.isfinite(out["pose"][ok]).all()
    _assert_graph(out["graph"], sg.graphs[0], tag)
    print(f"{tag}: max |pose diff| {np.abs(out['pose'] - room['pose']).max():.3e}")
    np.testing.assert_allclose(out["pose"], room["pose"], rtol=0, atol=FLOAT_TOL)
    for b in (1, 2):
        np.testing.assert_allclose(out["drift"][b - 1], sg.drift[b], rtol=0, atol=FLOAT_TOL)
        assert out["zone"][b - 1] is not None, f"{tag}: bot {b} has no zone box"
        np.testing.assert_allclose(out["zone"][b - 1], sg.zone[b], rtol=0, atol=FLOAT_TOL)
    o = _oracle_of_poses(out["pose"], out["acc"], room["ranges"])
    assert (out["grid"] == o.grid).all(), f"{tag}: {(out['grid'] != o.grid).sum()} cells differ from the oracle"
    assert (out["counts"][0] == o.hits).all() and (out["counts"][1] == o.misses).all(), f"{tag}: counters differ"
    c = out["counters"]
    assert c["datagrams"] == n and c["accepted"] == ok.sum() and c["rays"] == 181 * ok.sum()
    assert c["closures"] == len(sg.graphs[0].closures) and c["landmarks"] == len(sg.graphs[0].landmarks)


# ---- 1. the signature kernel ---------------------------------------------------------------------------------------------------
def _signature_pool(P, odometry):
    """35 records: ranges around both thresholds with NaN, +-inf, 0 and negatives, and one record of every kind of rejection."""
    rng = np.random.default_rng(41)
    n = 35
    r = rng.uniform(0.05, 1.3, (n, 181)).astype(np.float32)
    # records whose sectors sit on one side of a threshold, so that every signature occurs
    for k, (right, front, left) in enumerate([(0.3, 0.3, 0.3), (0.6, 0.3, 0.3), (0.3, 0.3, 0.6), (0.3, 0.9, 0.3), (0.9, 0.9, 0.9),
                                              (0.4, 0.4, 0.4), (0.8, 0.8, 0.8)]):
        q = r[12 + k]
        q[:59], q[61:120], q[122:] = right, front, left
        q += rng.normal(0, 1e-3, 181).astype(np.float32) if k < 5 else 0
    bad = rng.random((n, 181))
    for lo, v in ((0.00, np.nan), (0.04, np.inf), (0.08, -np.inf), (0.12, 0.0), (0.16, -0.5)):
        r[(bad >= lo) & (bad < lo + 0.04)] = v
    r[20, :11] = np.nan                                    # a whole default sector unusable: open
    agent = rng.choice(np.array([1, 2]), n)
    buf = P.pack_sweeps(agent, rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), r, odometry=odometry)
    stride = buf.shape[1]
    lens = np.full(n, stride, dtype=np.uint16)
    buf[1, :4] = np.frombuffer(b"QSRX", np.uint8)          # bad magic
    buf[2, 9:13] = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)       # NaN y
    buf[5, 4] = 0                                          # agent 0
    buf[7, 4] = 3                                          # agent max_agent + 1
    lens[9] = stride - 8                                   # wrong length
    buf[11, 5:9] = np.frombuffer(np.float32(np.inf).tobytes(), np.uint8)       # infinite x
    buf[16, 13:17] = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)     # NaN yaw
    return buf, lens


@pytest.mark.parametrize("odometry", [False, True], ids=["743", "751"])
def test_signatures_equal_the_restatement(pkg, odometry):
    P = _P(pkg)
    buf, lens = _signature_pool(P, odometry)
    stride = buf.shape[1]
    recs = MR.records_of(buf)
    dev = torch.device("cuda", 0)
    with pkg.QuasarMapper() as m:
        seen = set()
        for w in (0, 5, 29):
            want = R.signatures_of_records(recs, stride, lens, 2, w)
            assert (want[[1, 2, 5, 7, 9, 11, 16]] == R.LM_REJECTED).all() and (want != R.LM_REJECTED).sum() == 28
            seen |= set(want.tolist())
            got = m.sweep_signatures(buf, lens, params=dict(half_width=w))
            assert np.array_equal(got, want), f"host buffers, w {w}: {np.nonzero(got != want)[0]}"
            for n in (1, 3, 4, 5, 17, 35):
                for off in range(4):
                    d_buf = torch.zeros(n * stride + 8, dtype=torch.uint8, device=dev)
                    d_buf[off:off + n * stride] = torch.from_numpy(buf[:n].reshape(-1).copy()).to(dev)
                    d_lens = torch.from_numpy(lens[:n].astype(np.int16)).to(dev)
                    d_out = torch.full((n + 8,), 77, dtype=torch.uint8, device=dev)
                    torch.cuda.synchronize()
                    m.sweep_signatures_device(d_buf.data_ptr() + off, n, stride, d_out.data_ptr(), d_lens.data_ptr(),
                                              params=dict(half_width=w))
                    m.sync()
                    got = d_out.cpu().numpy()
                    assert np.array_equal(got[:n], want[:n]), f"w {w}, n {n}, offset {off}: {got[:n]} vs {want[:n]}"
                    assert (got[n:] == 77).all(), "wrote past its n records"
        assert seen == {0, 1, 2, 3, 4, 5, R.LM_REJECTED}
        # the thresholds are parameters: everything closer than 2 m is close
        want = R.signatures_of_records(recs, stride, lens, 2, 5, 2.0, 2.0)
        assert np.array_equal(m.sweep_signatures(buf, lens, params=dict(close=2.0, open=2.0)), want)
        assert (m.grid_i8() == -1).all() and m.slam_sizes() == (0, 0, 0) and m.counters()["datagrams"] == 0


# ---- 2. the room stream ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room_runs(pkg, room):
    return {(mode, tag): _room_outputs(pkg, room, mode, cuts)
            for mode in (1, 2) for tag, cuts in (("one", []), ("split", CUTS))}


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("calls", ["one", "split"])
def test_room_stream_equals_the_restatement(room, room_runs, mode, calls):
    _assert_room(room_runs[(mode, calls)], room, f"mode {mode}, {calls}")


def test_room_stream_direct_stamps_equal_tiled(room_runs):
    for calls in ("one", "split"):
        a, b = room_runs[(1, calls)]["stamps"], room_runs[(2, calls)]["stamps"]
        assert (a == b).all(), f"{calls}: {(a != b).sum()} stamps differ between direct and tiled"
    assert (room_runs[(1, "one")]["stamps"] == room_runs[(1, "split")]["stamps"]).all()


# ---- 3. interleaved with 42-byte packets -------------------------------------------------------------------------------------------
def _decode_packets(P, dg, ln):
    """(ok, agent, x, y, lm) of 42 / 41-byte datagrams by the packet path's acceptance rule."""
    n = len(dg)
    ok = np.zeros(n, dtype=bool)
    rec = np.ascontiguousarray(dg[:, :42]).view(P.PACKET_DTYPE).reshape(-1)
    for k in range(n):
        if ln[k] in (41, 42) and rec["magic"][k] == b"QSRL" and 1 <= rec["agent"][k] <= 2:
            ok[k] = np.isfinite([rec["x"][k], rec["y"][k], rec["yaw"][k]]).all()
    lm = np.where(ln == 42, rec["lm"], 0)
    return ok, rec["agent"], rec["x"], rec["y"], lm


def _shaped(right, front, left):
    r = np.full(181, 0.6, dtype=np.float32)
    r[:11], r[85:96], r[170:] = right, front, left
    return r


def test_interleaved_with_packets(pkg):
    P = _P(pkg)
    g = np.load(os.path.join(GOLDEN, "session_sep_512.npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    sep = float(sep)
    dg, ln = g["datagrams"], g["lengths"]
    cut = 2 * len(dg) // 3
    A, B = (3.5, -3.5), (-3.5, 3.5)                          # far from the session's own landmarks
    pkt_a = np.frombuffer(P.pack_packet(1, A[0], A[1], 0.0, 0, 0, 9.0, 9.0, 9.0, 9.0, P.LM_CORNER_R), np.uint8)[None, :]
    pkt_b = np.frombuffer(P.pack_packet(2, B[0] - sep + 0.1, B[1], 0.0, 0, 0, 9.0, 9.0, 9.0, 9.0, P.LM_CORRIDOR), np.uint8)[None, :]
    n_fill = 40
    s_agent = np.array([1] + [1, 2] * (n_fill // 2) + [2], dtype=np.uint8)
    s_x = np.array([B[0]] + [0.0] * n_fill + [A[0] - sep + 0.2], dtype=np.float32)
    s_y = np.array([B[1]] + [-4.0] * n_fill + [A[1] - 0.1], dtype=np.float32)
    s_r = np.stack([_shaped(0.3, 0.9, 0.3)] + [_shaped(0.6, 0.6, 0.6)] * n_fill + [_shaped(0.3, 0.3, 0.6)])
    sw = P.pack_sweeps(s_agent, s_x, s_y, np.zeros(len(s_agent)), s_r, odometry=False)
    sg = R.SweepGraph(separation=sep)
    ok, agent, x, y, lm = _decode_packets(P, dg, ln)
    sg.add_packets(agent[:cut], x[:cut], y[:cut], lm[:cut], ok[:cut])
    node_a = sg.add_packets([1], [np.float32(A[0])], [np.float32(A[1])], [P.LM_CORNER_R])[0]
    s_node, s_lm, s_pose, _ = sg.add_sweeps(s_agent, s_x, s_y, np.zeros(len(s_agent), np.float32), s_r, zone=False)
    assert s_lm[0] == P.LM_CORRIDOR and s_lm[-1] == P.LM_CORNER_R and (s_lm[1:-1] == 0).all()
    sg.add_packets(agent[cut:], x[cut:], y[cut:], lm[cut:], ok[cut:])
    node_b = sg.add_packets([2], [np.float32(B[0] - sep + 0.1)], [np.float32(B[1])], [P.LM_CORRIDOR])[0]
    gr = sg.graphs[0]
    pairs = [(li, ni) for li, ni, _, _ in gr.closures]
    assert (node_a, s_node[-1]) in pairs, "a sweep must close on the landmark a packet stored"
    assert (s_node[0], node_b) in pairs, "a packet must close on the landmark a sweep stored"
    assert s_node[0] == node_a + 1 and ok[:cut].sum() == node_a       # node indices count both kinds
    for mode in (1, 2):
        with pkg.QuasarMapper(int(size), res, ox, oy, separation=sep, raycast_mode=mode) as m:
            m.set_sweep_graph(True)
            m.ingest_array(dg[:cut], ln[:cut])
            m.ingest_array(pkt_a)
            m.ingest_sweeps(sw)
            node, lms = m.last_sweep_nodes()
            acc, pose = m.last_sweeps()
            assert np.array_equal(node, s_node) and np.array_equal(lms, s_lm) and (acc == 1).all()
            np.testing.assert_allclose(pose, s_pose, rtol=0, atol=FLOAT_TOL)
            with pytest.raises(pkg.QuasarError):
                m.last_batch()
            m.ingest_array(dg[cut:], ln[cut:])
            m.ingest_array(pkt_b)
            with pytest.raises(pkg.QuasarError):
                m.last_sweep_nodes()                            # the last ingest was a packet call
            _assert_graph(_graph_state(m), gr, f"mode {mode}")
            for b in (1, 2):
                np.testing.assert_allclose(m.drift(b), sg.drift[b], rtol=0, atol=FLOAT_TOL)
            assert len(m.slam.nodes) == gr.n_nodes and m.slam.nodes[int(s_node[-1])].agent_id == 2


# ---- 4. a graph per bot ----------------------------------------------------------------------------------------------------------
def test_three_bots_a_graph_each(pkg, room):
    P = _P(pkg)
    a3 = (np.arange(len(room["agent"])) % 3 + 1).astype(np.uint8)
    sg = R.SweepGraph(max_agent=3, bots_per_graph=1)
    node, lm, pose, _ = sg.add_sweeps(a3, room["x"], room["y"], room["yaw"], room["ranges"], zone=False)
    assert sum(len(g.closures) for g in sg.graphs) >= 3
    buf = P.pack_sweeps(a3, room["x"], room["y"], room["yaw"], room["ranges"], odometry=False)
    with pkg.QuasarMapper(max_agent=3, bots_per_graph=1) as m:
        m.set_sweep_graph(True)
        m.ingest_sweeps(buf)
        dn, dl = m.last_sweep_nodes()
        assert np.array_equal(dn, node) and np.array_equal(dl, lm)
        np.testing.assert_allclose(m.last_sweeps()[1], pose, rtol=0, atol=FLOAT_TOL)
        for g in range(3):
            st = _graph_state(m, g)
            _assert_graph(st, sg.graphs[g], f"graph {g}")
            assert set(st["agents"].tolist()) <= {g + 1}, "closures never cross graphs"
            np.testing.assert_allclose(m.drift(g + 1), sg.drift[g + 1], rtol=0, atol=FLOAT_TOL)


# ---- 5. the chunk boundary ---------------------------------------------------------------------------------------------------------
def test_chunk_boundary(pkg):
    P = _P(pkg)
    n = (1 << 16) + 24
    rng = np.random.default_rng(9)
    x = rng.uniform(-4.0, 4.0, n).astype(np.float32)
    y = rng.uniform(-4.0, 4.0, n).astype(np.float32)
    yaw = rng.uniform(-3.0, 3.0, n).astype(np.float32)
    ranges = np.full((n, 181), 0.6, dtype=np.float32)
    corner = _shaped(0.6, 0.3, 0.3)                          # CORNER_L
    spots = {0: (1.0, 1.0), (1 << 16) - 36: (1.2, 1.0), (1 << 16) + 4: (1.0, 1.3)}
    for k, (cx, cy) in spots.items():
        x[k], y[k], ranges[k] = cx, cy, corner
    agent = np.ones(n, dtype=np.uint8)
    ok = np.ones(n, dtype=bool)
    ok[[(1 << 16) - 1, 1 << 16]] = False                     # the last record of the first chunk and the first of the second
    sg = R.SweepGraph()
    node, lm, pose, _ = sg.add_sweeps(agent, x, y, yaw, ranges, ok=ok, zone=False)
    g = sg.graphs[0]
    assert [ni for _, ni, _, _ in g.closures] == [(1 << 16) - 36, (1 << 16) + 4 - 2]
    assert np.bincount(lm).tolist()[:2] == [n - 5, 3] and node[-1] == n - 3
    assert sg.drift[1] != [0.0, 0.0]
    buf = P.pack_sweeps(agent, x, y, yaw, ranges, odometry=False)
    buf[(1 << 16) - 1, 4] = 0                                # agent 0
    buf[1 << 16, 5:9] = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)     # NaN x: rejected in graph mode only
    stamps = []
    for mode in (1, 2):
        with pkg.QuasarMapper(raycast_mode=mode) as m:
            m.set_sweep_graph(True)
            m.ingest_sweeps(buf)
            dn, dl = m.last_sweep_nodes()
            acc, dp = m.last_sweeps()
            assert np.array_equal(dn, node) and np.array_equal(dl, lm) and np.array_equal(acc, ok.astype(np.uint8))
            assert np.isnan(dp[~ok]).all()
            print(f"mode {mode}: max |pose diff| {np.nanmax(np.abs(dp - pose)):.3e}")
            np.testing.assert_allclose(dp, pose, rtol=0, atol=FLOAT_TOL)
            # the first closure moves every later sweep of the call, across the boundary
            assert abs(dp[(1 << 16) + 10, 0] - float(x[(1 << 16) + 10])) > 0.05
            _assert_graph(_graph_state(m), g, f"mode {mode}")
            np.testing.assert_allclose(m.drift(1), sg.drift[1], rtol=0, atol=FLOAT_TOL)
            c = m.counters()
            assert c["datagrams"] == n and c["accepted"] == n - 2 and c["rays"] == 181 * (n - 2)
            stamps.append(_stamps(pkg, m))
    assert (stamps[0] == stamps[1]).all(), f"{(stamps[0] != stamps[1]).sum()} stamps differ between direct and tiled"


# ---- 6. matched and graph together --------------------------------------------------------------------------------------------------
def test_matched_ingest_reads_the_chains_poses(pkg, room):
    lap = len(room["agent"]) // 3
    buf, rest = room["buf"][:lap], room["buf"][lap:]
    lens, ok = room["lens"], room["ok"]
    assert (~ok[:lap]).any() and (~ok[lap:]).any()
    p = dict(radius=2, window=6, angle_steps=2)
    pp = MR.params(**p)
    with pkg.QuasarMapper(raycast_mode=2) as m:
        m.set_sweep_graph(True)
        m.ingest_sweeps(buf, lens[:lap])
        grid = m.grid_i8()
        _, rot = m.match_sweeps(room["clean"][lap:], params=p, rotations=True)    # the rotations depend on the yaw alone
        m.ingest_sweeps(rest, lens[lap:], match=p)
        dev = m.last_sweep_matches()
        node, lm = m.last_sweep_nodes()
        acc, pose = m.last_sweeps()
        # nodes and closures as without matching: the correction does not enter the graph
        assert np.array_equal(node, room["node"][lap:]) and np.array_equal(lm, room["lm"][lap:])
        _assert_graph(_graph_state(m), room["sg"].graphs[0], "matched")
        L = MR.field(grid, pp["radius"])
        moved = 0
        assert np.array_equal(acc, ok[lap:].astype(np.uint8))
        for k in range(len(rest)):
            if not ok[lap + k]:                                  # rejected by the one decision: the matcher skips it too
                assert dev[k].tobytes() == bytes(dev.dtype.itemsize) and np.isnan(pose[k]).all(), f"record {k}"
                continue
            chain = (room["chain"][lap + k, 0], room["chain"][lap + k, 1], float(room["yaw"][lap + k]))
            ref = MR.match_one(L, (0.05, -5.0, -5.0), chain, room["ranges"][lap + k], pp, R.SMIN, R.SMAX, rot[k])
            for f in MR.FIELDS:
                assert dev[f][k] == ref[f], f"record {k}: field {f}: {dev[f][k]} vs {ref[f]}"
            want = (chain[0] + ref["dx"], chain[1] + ref["dy"], chain[2] + ref["dyaw"])
            np.testing.assert_allclose(pose[k], want, rtol=0, atol=FLOAT_TOL)
            moved += ref["accepted_match"] and (ref["ix"], ref["iy"], ref["it"]) != (0, 0, 0)
        assert moved >= 10, "the drifting stream must give the matcher something to correct"
        assert all(m.zone(b) is not None for b in (1, 2))


# ---- 7. off again, bad parameters, reset, shards -----------------------------------------------------------------------------------
def test_switch_off_bad_parameters_reset_and_shards(pkg, room):
    with pkg.QuasarMapper() as never:
        never.ingest_sweeps(room["clean"])
        want = (never.grid_i8(), *never.counts(), never.last_sweeps()[1])
        assert never.slam_sizes() == (0, 0, 0) and never.zone(1) is None
        with pytest.raises(pkg.QuasarError):
            never.last_sweep_nodes()
    with pkg.QuasarMapper() as m:
        assert m.sweep_graph() == (False, {"half_width": 5, "close": 0.40, "open": 0.80})
        m.set_sweep_graph(True, half_width=7, close=0.3, open=0.9)
        assert m.sweep_graph() == (True, {"half_width": 7, "close": 0.3, "open": 0.9})
        m.ingest_sweeps(room["clean"][:50])
        assert m.slam_sizes()[0] == 50
        for bad, field in ((dict(half_width=-1), "half_width"), (dict(half_width=30), "half_width"), (dict(close=0.0), "close"),
                           (dict(close=float("nan")), "close"), (dict(close=0.5, open=0.4), "open"), (dict(open=float("inf")), "open")):
            with pytest.raises(pkg.QuasarError, match=field):
                m.set_sweep_graph(True, **bad)
        assert m.sweep_graph() == (True, {"half_width": 7, "close": 0.3, "open": 0.9})      # a refused call changes nothing
        m.reset()
        assert m.sweep_graph() == (True, {"half_width": 7, "close": 0.3, "open": 0.9})      # kept over reset
        m.set_sweep_graph(False)
        assert m.sweep_graph()[0] is False
        m.ingest_sweeps(room["clean"])
        got = (m.grid_i8(), *m.counts(), m.last_sweeps()[1])
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "switched off, the ingest is the plain one"
        assert m.slam_sizes() == (0, 0, 0) and m.zone(1) is None and m.zone(2) is None
        with pytest.raises(pkg.QuasarError):
            m.last_sweep_nodes()
    for kw in (dict(seq_stride=2), dict(shard_bots=1, shard_rank=0)):
        with pkg.QuasarMapper(**kw) as m:
            m.set_sweep_graph(True)
            with pytest.raises(pkg.QuasarError):
                m.ingest_sweeps(room["buf"][:2])


# ---- 8. checkpoint in the middle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_checkpoint_in_the_middle(pkg, room, room_runs, mode):
    out = _room_outputs(pkg, room, mode, [], restore_at=RESTORE_AT)
    _assert_room(out, room, f"restored, mode {mode}")
    ref = room_runs[(mode, "one")]
    for f in ("node", "lm", "acc", "pose", "grid", "stamps"):
        assert np.array_equal(out[f], ref[f], equal_nan=(f == "pose")), f"{f} differs from the uninterrupted run"
    assert all(np.array_equal(a, b) for a, b in zip(out["counts"], ref["counts"]))
    assert all(np.array_equal(out["graph"][f], ref["graph"][f]) for f in ("idx", "corr", "agents", "xy", "ti"))
    assert out["graph"]["sizes"] == ref["graph"]["sizes"]
    for f in ("datagrams", "accepted", "rays", "cells", "hits", "closures", "landmarks", "rebases", "edge_rays"):
        assert out["counters"][f] == ref["counters"][f], f"counter {f}"
    assert all(np.array_equal(a, b) for a, b in zip(out["drift"] + out["zone"], ref["drift"] + ref["zone"]))


# ---- 9. the front-end ----------------------------------------------------------------------------------------------------------------
def test_mission_control_sends_sweep_bots_real_zones(pkg, room):
    P = _P(pkg)
    fe = importlib.import_module(pkg.__name__ + ".udp_frontend")
    with pkg.QuasarMapper() as m:
        for on in (True, {}):                                   # an empty dict is "on with the defaults", not "off"
            with socket.socket(socket.AF_INET, socket.SOCK_DGRAM) as udp, pytest.raises(ValueError):
                fe.MissionControl(m, sock=udp, sweep_graph=on)
        assert m.sweep_graph()[0] is False
        a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
        try:
            mc = fe.MissionControl(m, sock=a, sweeps=True, sweep_graph=dict(half_width=5))
            assert m.sweep_graph()[0] is True
            k = 40
            for rec, ln in zip(room["buf"][:k], room["lens"][:k]):
                b.send(rec.tobytes()[:int(ln)])
            # (a socket pair has no source address: give the front-end one)
            orig = a.recvfrom_into
            mc.sock = type("S", (), {"recvfrom_into": lambda s, v, nb: (orig(v, nb)[0], ("127.0.0.1", 40000)),
                                     "sendto": lambda s, d, addr: len(d), "close": lambda s: None})()
            assert mc.poll(now=1.0) == k
            assert mc.online == {1: True, 2: True}
            sent = mc.zone_tick(now=1.0, force=True)
            lifted = P.zone_packet(None)
            sg = R.SweepGraph()
            sg.add_sweeps(room["agent"][:k], room["x"][:k], room["y"][:k], room["yaw"][:k], room["ranges"][:k], ok=room["ok"][:k])
            for bot, other in ((1, 2), (2, 1)):
                assert sent[bot] != lifted, f"bot {bot} got the lifted box"
                box = np.frombuffer(sent[bot][4:], dtype="<f4")
                assert sent[bot][:4] == b"ZONE"
                np.testing.assert_allclose(box, np.array(sg.zone[other], dtype=np.float32), rtol=0, atol=FLOAT_TOL)
            assert m.slam_sizes()[0] == room["ok"][:k].sum() == k - 2
        finally:
            a.close()
            b.close()
