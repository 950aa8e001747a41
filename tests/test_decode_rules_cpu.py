"""tests/decode_rules.py (the byte-level restatement the decoder's GPU tests compare with) against the fixtures the reference
produced and the CPU oracle: the yardstick is checked without a GPU, and never against the kernel."""
import hashlib
import importlib
import os

import numpy as np
import pytest

import decode_rules as dr
from conftest import GOLDEN, PKG_NAME
from oracle import oracle as orc

NAMES = ["mixed_200", "session_200", "adversarial_512"]
NO_CLOSURES = 1 << 40          # min_poses_between no stream reaches: no closure, every drift stays 0.0


def _golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    size, res, ox, oy, sep = g["cfg"]
    recs = []
    for row, L in zip(g["datagrams"], g["lengths"].tolist()):
        recs.append(row[:min(L, 48)].tobytes() + b"\xff" * max(0, L - 48))
    return g, (int(size), float(res), float(ox), float(oy), float(sep)), recs


def _offsets(sep, max_agent=2):
    off = np.zeros(max_agent + 1)
    off[2] = sep
    return off


@pytest.mark.parametrize("stride", [48, 64, 57])
@pytest.mark.parametrize("name", NAMES)
def test_accept_equals_the_oracle_and_the_golden(name, stride):
    g, cfg, recs = _golden(name)
    buf, lens = dr.build(recs, stride, np.random.default_rng(stride))
    ref = dr.decode(buf, len(recs), stride, lens, 2, _offsets(cfg[4]))
    assert (ref["accept"] == g["accepted"]).all()
    o = orc.OracleMapper(*cfg)
    fed = np.array([o.feed(d) for d in dr.datagrams(buf, len(recs), stride, lens)], dtype=np.uint8)
    assert (fed == ref["accept"]).all()
    assert 0 < int(fed.sum())
    # the rebuilt records (another stride, garbage padding) are the golden's stream: the reference's own grid
    assert hashlib.sha256(o.grid.tobytes()).digest() == g["grid_sha256"].tobytes()
    assert (o.pose_agents == ref["agent"][ref["accept"] == 1]).all()


@pytest.mark.parametrize("name", NAMES)
def test_fields_equal_the_oracle_bit_for_bit_without_closures(name):
    g, cfg, recs = _golden(name)
    stride = 43
    recs = [r if len(r) <= stride else r[:stride] + b"\x01" for r in recs]          # (true length stays above the stride)
    buf, lens = dr.build(recs, stride, np.random.default_rng(5))
    ref = dr.decode(buf, len(recs), stride, lens, 2, _offsets(cfg[4]))
    assert (ref["accept"] == g["accepted"]).all()
    o = orc.OracleMapper(*cfg)
    o.set_closure_params(0.6, NO_CLOSURES, 0.5)
    for d in dr.datagrams(buf, len(recs), stride, lens):
        o.feed(d)
    assert len(o.closures(0)[0]) == 0
    want = dr.pose_as_reported(ref)[ref["accept"] == 1]
    assert want.shape == o.poses.shape and (want.view(np.uint64) == o.poses.view(np.uint64)).all()
    # landmark types through the pose graph: every non-zero type is a landmark, in order, with its node index
    ti = o.landmarks(0)[1]
    lm = ref["lm"][ref["accept"] == 1]
    assert (ti[:, 0] == lm[lm != 0]).all() and (ti[:, 1] == np.nonzero(lm)[0]).all()


def test_vector_form_equals_the_struct_form_on_a_mutated_pool():
    """decode (numpy, what the GPU tests use) against decode_one (struct, one datagram at a time) and the oracle, on the pool of
    the GPU tests: every mutation, strides with and without lengths, garbage padding."""
    replay = importlib.import_module(PKG_NAME + ".replay")
    base = replay.adversarial_stream(4000, seed=3, lo=-20.0, hi=20.0, max_agent=7)
    off = np.zeros(8)
    off[2] = 1.25
    seen = set()
    for stride, with_lens in ((41, False), (42, False), (42, True), (45, True), (48, True), (64, True), (100, True)):
        rng = np.random.default_rng(stride)
        pool = dr.fit(dr.make_pool(base, rng, 7, 3000, odd_lengths=with_lens), stride, with_lens)
        buf, lens = dr.build(pool, stride, rng)
        lens = lens if with_lens else None
        ref = dr.decode(buf, len(pool), stride, lens, 7, off)
        share = 1.0 - ref["accept"].mean()
        assert 0.15 <= share <= 0.40, (stride, share)
        o = orc.OracleMapper(512, 0.05, -25.6, -25.6, 1.25, max_agent=7)
        o.set_closure_params(0.6, NO_CLOSURES, 0.5)
        for k, d in enumerate(dr.datagrams(buf, len(pool), stride, lens)):
            one = dr.decode_one(d, 7, off)
            assert o.feed(d) == ref["accept"][k] == (one is not None), (stride, k)
            if one is None:
                continue
            agent, lm, px, py, yaw, dist, enc = one
            assert (agent, lm, enc) == (ref["agent"][k], ref["lm"][k], ref["enc"][k])
            got = np.array([ref["px"][k], ref["py"][k], ref["yaw"][k]])
            assert (got.view(np.uint64) == np.array([px, py, yaw]).view(np.uint64)).all()
            assert (dist.view(np.uint32) == ref["dist"][k].view(np.uint32)).all()
            seen.add(len(d))
            if len(d) == 41:
                assert lm == 0
        want = dr.pose_as_reported(ref)[ref["accept"] == 1]
        assert (want.view(np.uint64) == o.poses.view(np.uint64)).all()
    assert seen == {41, 42}


def test_padding_is_never_read_and_lengths_rule():
    off = np.zeros(3)
    v2 = dr.struct.pack(dr.FMT_V2, b"QSRL", 1, 1.0, 2.0, 0.5, 7, 0, 0.3, 0.4, 0.5, 0.6, 5)
    rng = np.random.default_rng(0)
    for stride in (42, 43, 64, 65, 255):
        buf, lens = dr.build([v2[:41], v2, v2[:40], v2 + b"\x09"], stride, rng)
        assert (buf != 0).sum() >= len(buf) - 4 * 42                       # (the padding is non-zero everywhere)
        ref = dr.decode(buf, 4, stride, lens, 2, off)
        want = [1, 1, 0, 0]
        assert ref["accept"].tolist() == want and ref["lm"].tolist() == [0, 5, 0, 0]
        assert buf[41] != 0                                                 # the byte after the v1 record is garbage
    # no lengths: the length is the stride
    assert dr.decode(v2[:41], 1, 41, None, 2, off)["accept"][0] == 1
    assert dr.decode(v2, 1, 42, None, 2, off)["lm"][0] == 5
    assert dr.decode(v2 + b"\x00", 1, 43, None, 2, off)["accept"][0] == 0
    # a length above the stride is refused even when it is 42
    assert dr.decode(v2[:41], 1, 41, np.array([42], dtype=np.uint16), 2, off)["accept"][0] == 0


def test_shift_arithmetic_of_the_cases():
    """What the GPU tests claim to reach, from the kernel's own arithmetic: an aligned buffer (the host path's staging) reaches
    sh of 1 and 3 at odd strides but never mis != 0; byte offsets 0, 1, 2, 3, 5 with strides 41, 42, 43, 48, 64 reach all 16
    (mis, sh) pairs, and the first and last tiles of an offset buffer take the bytewise branch."""
    host = set()
    for stride in [41] + list(range(42, 65)):
        host |= dr.shifts(0, 5000, stride)
    assert host == {(0, s) for s in range(4)}
    dev = set()
    for off in (0, 1, 2, 3, 5):
        for stride in (41, 42, 43, 48, 64):
            dev |= dr.shifts(4096 + off, 2049, stride)
    assert dev == {(m, s) for m in range(4) for s in range(4)}
    assert dr.bytewise_tiles(4096, 5000, 42) == [] and dr.bytewise_tiles(4096, 2049, 41) == [8]
    assert dr.bytewise_tiles(4097, 2049, 64) == [0, 8] and dr.bytewise_tiles(4099, 100, 43) == [0]
