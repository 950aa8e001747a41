"""CPU side of tests/test_gpu_ekf_edges.py: every stream of its table (tests/ekf_rules.py) is what its row promises, the oracle
the device is compared with agrees with a long-double restatement of the sequential filter on it, and the stream meets the
conditions under which the chunked form may be compared at all.

Per stream: oracle vs sequential_ld <= 1e-11 (measured: <= 5.1e-13; the device bar is 1e-9), admit(trace), and the row's own
promise (record counts, wrap counts per direction, a wrap at the aimed record, time stamps).  A bot with more than 20 000
records is traced in fp64 by the same function.  Single-bot streams: the numpy restatement of the scan algebra
(test_ekf_scan_math.scan_filter) at the chunk length the device will choose agrees with sequential_ld to 1e-10.  The clamp
stream of group H must clamp at chunk 128, and scan_filter must raise on it."""
import numpy as np
import pytest

from oracle import oracle as orc
import ekf_rules as R
from test_ekf_scan_math import scan_filter

LD_MAX = 20000
ROWS = {f"{g}-{name}": (g, name, spec) for g, name, spec in R.table()}
_cache = {}


def traced(key):
    """(spec, records, oracle, {bot: (x, P, trace)}) of a row, computed once."""
    if key not in _cache:
        _, _, spec = ROWS[key]
        pk, times, records = R.build(spec)
        o = orc.OracleMapper(max_agent=spec["max_agent"])
        o.enable_ekf(R.MPT)
        assert o.feed_stream(pk, None, times) == spec["n"] - len(spec.get("rejects", {}))
        runs = {b: R.sequential_ld(r, R.MPT, np.longdouble if len(r) <= LD_MAX else np.float64)
                for b, r in records.items() if len(r)}
        _cache[key] = (spec, records, o, runs)
    return _cache[key]


@pytest.mark.parametrize("key", list(ROWS))
def test_oracle_agrees_with_long_double_and_stream_is_admitted(key):
    spec, records, o, runs = traced(key)
    worst = 0.0
    for b, (x, Pm, tr) in runs.items():
        xo, Po = o.ekf_state(b)
        worst = max(worst, R.rel_err(xo, x), R.rel_err(Po, Pm))
        if ROWS[key][0] != "H":
            assert R.admit(tr), (key, b, np.abs(tr.heading).max())
    for b, r in records.items():
        if len(r) == 0:
            assert not o.ekf_state(b)[0].any()
    print(f"EKF-RULES {key}: oracle vs long double {worst:.2e}")
    assert worst <= 1e-11


def counts(records):
    return [len(records[b]) for b in sorted(records)]


@pytest.mark.parametrize("c", R.A_COUNTS + (None,))
def test_a_counts(c):
    _, records, _, _ = traced("A-bot2_none" if c is None else f"A-c{c}")
    assert counts(records) == ([8192, 0] if c is None else [c, 8192 - c])


@pytest.mark.parametrize("n,chunk", R.B_SIZES)
def test_b_smallest_n_of_every_chunk_length(n, chunk):
    _, records, _, _ = traced(f"B-n{n}")
    assert counts(records) == [n] and R.chunk_for(n, 1) == chunk
    assert n == R.SCAN_MIN_BATCH or R.chunk_for(n - 1, 1) == chunk // 2


@pytest.mark.parametrize("n", R.C_SIZES + R.C_EXTRA)
def test_c_bots_by_tile_and_rejects_of_every_kind(n):
    spec, records, _, _ = traced(f"C-n{n}")
    last0 = (n - 1) // R.TILE * R.TILE
    s1, s2, s3 = (R.slots(spec, b) for b in (1, 2, 3))
    assert len(s1) and s1.max() < R.TILE
    assert (s3 >= last0).all() and (len(s3) or n - last0 == 1)          # a one-datagram last tile is the rejected last record
    assert set(s2 // R.TILE) == set(range(last0 // R.TILE + (1 if n - last0 > 1 else 0)))
    assert counts(records) == [len(s1), len(s2), len(s3)]
    rej = spec["rejects"]
    assert set(rej.values()) == set(R.REJECT_KINDS)
    assert all(i in rej for i in (0, n - 1, R.TILE - 1, R.TILE) if i < n)


def test_c_every_kind_at_every_edge():
    at = {"first": set(), "last": set(), "before_edge": set(), "after_edge": set()}
    for n in R.C_SIZES + R.C_EXTRA:
        rej = R.spec_c(n)["rejects"]
        at["first"].add(rej[0]); at["last"].add(rej[n - 1])
        if R.TILE - 1 < n - 1: at["before_edge"].add(rej[R.TILE - 1])
        if R.TILE < n - 1: at["after_edge"].add(rej[R.TILE])
    assert all(len(v) >= 2 for v in at.values()), at


@pytest.mark.parametrize("nominal", [False, True])
def test_d_stream(nominal):
    spec, records, _, _ = traced("D-nominal" if nominal else "D-recv_time")
    assert counts(records) == [9000, 11000]
    if nominal:
        for b in (1, 2):
            assert (records[b][:, 0] == R.slots(spec, b)).all()


def test_e_wraps_in_both_directions():
    _, _, _, runs = traced("E-spin_both_ways")
    tr = runs[1][2]
    assert len(tr.wraps_up) >= 500 and len(tr.wraps_down) >= 500


def test_e_unwrapped_heading_of_thousands_of_radians():
    for key in ("E-spin_one_way", "E-constant_rate"):
        tr = traced(key)[3][1][2]
        assert (len(tr.wraps_up) - len(tr.wraps_down)) * 2 * R.PI > 5000


def test_e_wraps_at_the_aimed_records():
    tr = traced("E-aimed_wraps")[3][1][2]
    assert sorted(tr.wraps_up + tr.wraps_down) == sorted(R.AIMED)
    assert len(tr.wraps_up) == 3 and len(tr.wraps_down) == 3


def test_e_update_driven_excursions():
    tr = traced("E-jittered_spin")[3][1][2]
    assert np.abs(tr.heading).max() > R.PI + 0.5


def test_e_excursions_land_on_chunk_starts():
    """The heading after the last record of a chunk is the next chunk's start: beyond -pi the start's wrap count is the third
    candidate, beyond +pi the first."""
    tr = traced("E-excursions_at_chunk_starts")[3][1][2]
    h = np.asarray(tr.heading)[list(R.CHUNK_ENDS)]
    assert (h < -R.PI - 0.05).sum() >= 3 and (h > R.PI + 0.05).sum() >= 3


@pytest.mark.parametrize("name,sign", [("last_chunk_starts_above_pi", 1), ("last_chunk_starts_below_pi", -1)])
def test_e_last_chunk_starts_on_an_excursion_and_never_predicts(name, sign):
    spec, records, _, runs = traced("E-" + name)
    tr, rec = runs[1][2], records[1]
    assert R.chunk_for(spec["n"], 1) == 128 and len(rec) == 4100
    assert sign * tr.heading[4095] > R.PI + 0.05 and tr.heading[-1] == tr.heading[4095]
    assert (rec[4096:, 0] == rec[4095, 0]).all() and max(tr.pred_index) < 4095


def test_e_heading_near_pi_without_crossing():
    tr = traced("E-near_pi")[3][1][2]
    start, length = R.NEAR_PI
    h = np.asarray(tr.heading[start:start + length])
    assert (np.abs(h - R.PI) < 0.01).all() and (h < R.PI).all()
    assert not tr.wraps_up and not tr.wraps_down


def test_f_time_edges():
    rec, tr = traced("F-equal_stamps")[1][1], traced("F-equal_stamps")[3][1][2]
    assert (rec[256:512, 0] == rec[255, 0]).all()                       # two whole chunks of 128 without a step record
    assert not [k for k in tr.pred_index if 256 <= k < 512]
    rec, tr = traced("F-updates_without_predicts")[1][1], traced("F-updates_without_predicts")[3][1][2]
    assert (np.diff(rec[255:512, 0]) > 0).all()                         # every one a step record ...
    assert not [k for k in tr.pred_index if 256 <= k < 512]             # ... and none a predict
    assert [k for k in tr.pred_index if k > 552]                        # predicts resume
    rec = traced("F-negative_stamps")[1][1]
    assert rec[0, 0] < 0 < rec[-1, 0] and (np.diff(rec[:, 0]) <= 0).any()
    rec = traced("F-epoch_stamps")[1][1]
    assert rec[:, 0].min() >= 1.7e9 and np.abs(np.diff(rec[:, 0]) - 0.05).max() < 1e-6


def test_g_counts():
    c = counts(traced("G-round_robin")[1])
    assert len(c) == 255 and set(c) == {16, 17}
    c = counts(traced("G-one_long_40_absent")[1])
    assert c[R.G_LONG_BOT - 1] == R.G_LONG_COUNT and c.count(0) == 40 and sum(c) == 8192
    assert max(v for i, v in enumerate(c) if i != R.G_LONG_BOT - 1) < 128


SINGLE = [k for k, (g, _, spec) in ROWS.items() if spec["max_agent"] == 1 and spec["n"] <= LD_MAX and g != "H"]


@pytest.mark.parametrize("key", SINGLE)
def test_scan_restatement_at_the_device_chunk(key):
    spec, records, _, runs = traced(key)
    r = records[1]
    chunk = R.chunk_for(spec["n"], 1)
    x, Pm, _ = scan_filter(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], R.MPT, chunk)
    xs, Ps, _ = runs[1]
    worst = max(R.rel_err(x, xs), R.rel_err(Pm, Ps))
    print(f"EKF-RULES {key}: restatement (chunk {chunk}) vs long double {worst:.2e}")
    assert worst <= 1e-10


def test_h_clamp_stream():
    spec, records, _, runs = traced("H-sawtooth")
    tr = runs[1][2]
    assert not R.admit(tr) and R.must_clamp(tr, 128) and R.chunk_for(spec["n"], 1) == 128
    r = records[1]
    with pytest.raises(AssertionError):
        scan_filter(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], R.MPT, 128)
