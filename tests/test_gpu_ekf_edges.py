"""The EKF kernels (csrc/ekf.hip, csrc/ekf_scan.hip) on built streams: chunk, tile, wrap and time edges.

Reference: the sequential filter of oracle/oracle.c (OracleMapper.enable_ekf / feed_stream / ekf_state), itself within 1e-11
of a long-double restatement on every one of these streams (tests/test_ekf_rules_cpu.py).  Bar: _ekf_close of
tests/test_gpu_parity.py, unchanged: 1e-9 x max(1, |ref|max) on x and on P.  The streams come from tests/ekf_rules.py; every
compared one meets ekf_rules.admit (checked on the CPU).  Small map: the default 200 x 200 grid, poses within +-3 m.  Unless a
row says otherwise: enable_ekf=True, explicit recv_time, every bot compared, and counters()["ekf_wrap_clamp"] == 0.

| Group | Shapes | What it hits |
| --- | --- | --- |
| A. Record counts at chunk edges | max_agent=2, one batch of 8 192. Bot 1 has c records, bot 2 the rest, c in {1, 2, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097}. Plus one batch where bot 2 has none. | Last chunk of 1 record or a full one; init-only bot; count == 0 bot; chunk_base prefix |
| B. Every chunk length | max_agent=1, n = 4 096 (128), 33 024 (256), 65 792 (512), 131 328 (1024): the smallest n for which es_chunk_for gives each value (asserted by restating that function). Spin heading, jittered time. | 256 and 1024 for the first time |
| C. Tile of 16 384 | max_agent=3, n in {16 383, 16 384, 16 385, 32 769} (and 40 000, whose last tile is not a single datagram). One bot only in the first tile, one only in the last, one throughout. Rejected datagrams of every kind, including at indices 16 383 and 16 384 and as the first and last record. | tile_off, compaction order, map_ok |
| D. Batch switch, state carried | One 20 000-record stream fed as batches [4095, 4096, 1, 4097, 3, 4096, rest]. The oracle is fed the same slices. Compared after every batch. Once with recv_time, once with recv_time=None (nominal time continues with the sequence counter). | Prior taken from stored state; prev hand-over; last_t across forms |
| E. Wraps | Single bot, 4 096 records, at least 500 wraps in each direction. Wraps aimed at bot-record indices 127, 128, 129 and 255, 256, 257. Update-driven excursions beyond +-pi (the time-jittered spin stream), and one stream that puts such an excursion on every chunk start, in both directions; two more end on a chunk that starts on such an excursion (one above +pi, one below -pi) and holds no step record. One stream whose heading sits within 0.01 rad of +pi for 300 records without crossing. | The three-candidate rule and the fold's pick; es_sincos on an unwrapped heading of thousands of radians |
| F. Time edges | A whole chunk of equal time stamps (no step records: the identity element). A chunk of updates without predicts (t <= last while t > t_prev). Negative time stamps. Stamps near 1.7e9 s with 50 ms steps. | cmax "0 = none", prefix max of es_last_kernel, es_next_step |
| G. Many bots, few records | max_agent=255, n = 4 096 round robin (16-17 records each). Then n = 8 192 with one bot holding 3 000 and 40 bots holding none. | Bots shorter than a chunk; es_bot_of; launch sizes from max_agent |
| H. The clamp is never silent | The sawtooth stream of the CPU test in one batch of at least 4 096 (scan): ekf_wrap_clamp >= 1 and every state value finite. Then the same stream to a fresh mapper in batches of 4 095 (serial): agreement with the oracle by the bar and a counter of 0. | The documented contract of the counter |
| I. Serial kernel, bit for bit | Three bots, batches of n in {63, 64, 65, 255, 256, 257, 1000}. The watched bot's records sit at lane 0 and at lane 63 of a 64-record group, with an empty group in between, and alone in a group. Compared with the oracle by the bar, and np.array_equal with a replay through ekf_init + one ekf_step per step record. | The 64-lane group hand-over, chained / carry, the prefetch past n, the "bit for bit" claim |
"""
import numpy as np
import pytest
import torch  # noqa: F401  before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import load_pkg
from oracle import oracle as orc
import ekf_rules as R
from test_gpu_parity import _ekf_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def oracle_for(spec):
    o = orc.OracleMapper(max_agent=spec["max_agent"])
    o.enable_ekf(R.MPT)
    return o


def mapper_for(pkg, spec):
    return pkg.QuasarMapper(max_agent=spec["max_agent"], enable_ekf=True)


def close(m, o, spec, label):
    """Print the figure (share of the bar used, worst bot), then _ekf_close unchanged."""
    bots = range(1, spec["max_agent"] + 1)
    worst = 0.0
    for b in bots:
        x, Pm = m.ekf_state(b)
        xo, Po = o.ekf_state(b)
        worst = max(worst, R.rel_err(x, xo), R.rel_err(Pm, Po))
    print(f"EKF-EDGE {label}: worst error {worst:.3e} = {worst / R.BAR:.2e} of the bar")
    _ekf_close(m, o, bots)


def one_batch(pkg, spec, label):
    pk, times, _ = R.build(spec)
    o = oracle_for(spec)
    o.feed_stream(pk, None, times)
    with mapper_for(pkg, spec) as m:
        m.ingest_array(pk, recv_time=times)
        close(m, o, spec, label)
        assert m.counters()["ekf_wrap_clamp"] == 0


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.A_COUNTS + (None,))
def test_a_record_counts_at_chunk_edges(pkg, c):
    spec = R.spec_a(c)
    assert R.chunk_for(spec["n"], 2) == 128 and spec["n"] >= R.SCAN_MIN_BATCH
    one_batch(pkg, spec, f"A c={c}")


# ---- B ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk", R.B_SIZES)
def test_b_every_chunk_length(pkg, n, chunk):
    assert R.chunk_for(n, 1) == chunk and (n == R.SCAN_MIN_BATCH or R.chunk_for(n - 1, 1) == chunk // 2)
    one_batch(pkg, R.spec_b(n), f"B n={n} chunk={chunk}")


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.C_SIZES + R.C_EXTRA)
def test_c_tile_edges_and_rejected_datagrams(pkg, n):
    spec = R.spec_c(n)
    for i in (0, n - 1, R.TILE - 1, R.TILE):
        assert i >= n or i in spec["rejects"]
    pk, times, records = R.build(spec)
    o = oracle_for(spec)
    o.feed_stream(pk, None, times)
    with mapper_for(pkg, spec) as m:
        m.ingest_array(pk, recv_time=times)
        acc = m.last_batch()[0]
        assert acc.sum() == n - len(spec["rejects"]) == sum(len(r) for r in records.values())
        assert not acc[list(spec["rejects"])].any()
        close(m, o, spec, f"C n={n}")
        assert m.counters()["ekf_wrap_clamp"] == 0


# ---- D ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nominal", [False, True])
def test_d_batch_switch_state_carried(pkg, nominal):
    spec = R.spec_d(nominal)
    pk, times, _ = R.build(spec)
    assert (times is None) == nominal
    o = oracle_for(spec)
    sizes = list(R.D_BATCHES) + [spec["n"] - sum(R.D_BATCHES)]
    assert 0 < sizes[-1] < R.SCAN_MIN_BATCH
    with mapper_for(pkg, spec) as m:
        lo = 0
        for k, size in enumerate(sizes):
            sl = slice(lo, lo + size)
            o.feed_stream(pk[sl], None, None if nominal else times[sl])
            m.ingest_array(pk[sl], recv_time=None if nominal else times[sl])
            close(m, o, spec, f"D nominal={nominal} after batch {k} ({size})")
            lo += size
        assert lo == spec["n"]
        assert m.counters()["ekf_wrap_clamp"] == 0


# ---- E, F ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.E_ROWS))
def test_e_wraps(pkg, name):
    one_batch(pkg, R.E_ROWS[name], f"E {name}")


@pytest.mark.parametrize("name", list(R.F_ROWS))
def test_f_time_edges(pkg, name):
    one_batch(pkg, R.F_ROWS[name], f"F {name}")


# ---- G ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["round_robin", "ragged"])
def test_g_many_bots_few_records(pkg, which):
    spec = R.spec_g(which)
    assert spec["max_agent"] == 255 and spec["n"] >= R.SCAN_MIN_BATCH
    one_batch(pkg, spec, f"G {which}")


# ---- H ---------------------------------------------------------------------------------------------------------------------
def test_h_the_clamp_is_never_silent(pkg):
    spec = R.spec_h()
    pk, times, _ = R.build(spec)
    assert spec["n"] >= R.SCAN_MIN_BATCH
    o = oracle_for(spec)
    o.feed_stream(pk, None, times)
    with mapper_for(pkg, spec) as m:                                  # scan form: outside what it can replay, and it says so
        m.ingest_array(pk, recv_time=times)
        x, Pm = m.ekf_state(1)
        print(f"EKF-EDGE H scan: ekf_wrap_clamp = {m.counters()['ekf_wrap_clamp']}")
        assert m.counters()["ekf_wrap_clamp"] >= 1
        assert np.isfinite(x).all() and np.isfinite(Pm).all()
    with mapper_for(pkg, spec) as m:                                  # serial form: the sequential filter itself
        for lo in range(0, spec["n"], R.SCAN_MIN_BATCH - 1):
            sl = slice(lo, lo + R.SCAN_MIN_BATCH - 1)
            m.ingest_array(pk[sl], recv_time=times[sl])
        close(m, o, spec, "H serial")
        assert m.counters()["ekf_wrap_clamp"] == 0


# ---- I ---------------------------------------------------------------------------------------------------------------------
WATCHED = 2


def step_records(rec, mpt):
    """(t, omega_m, v_enc) of every step record of a bot, in float64 with the kernel's expression order."""
    out = []
    for k in range(1, len(rec)):
        t, _, _, yaw, enc = rec[k]
        tp, _, _, yawp, encp = rec[k - 1]
        dtp = t - tp
        if dtp > 0:
            dyaw = yaw - yawp
            if dyaw > R.PI: dyaw -= 2 * R.PI
            elif dyaw < -R.PI: dyaw += 2 * R.PI
            inv_dt = 1.0 / dtp
            out.append((t, dyaw * inv_dt, (enc - encp) * mpt * inv_dt))
    return out


@pytest.mark.parametrize("n", R.I_SIZES)
def test_i_serial_kernel_bit_for_bit(pkg, n):
    spec = R.spec_i(n)
    assert n < R.SCAN_MIN_BATCH
    pk, times, records = R.build(spec)
    ag = np.asarray(spec["agents"])
    mine = np.nonzero(ag == WATCHED)[0]
    assert mine[0] == 0 and (n <= 63 or 63 in mine)                                  # lane 0 and lane 63 of a group
    assert n <= 192 or (not ((mine >= 128) & (mine < 192)).any() and (mine >= 192).any())     # an empty group in between
    assert n <= 448 or (ag[384:448] == WATCHED).all()                                # alone in a group
    o = oracle_for(spec)
    o.feed_stream(pk, None, times)
    with mapper_for(pkg, spec) as m:
        m.ingest_array(pk, recv_time=times)
        close(m, o, spec, f"I n={n}")
        assert m.counters()["ekf_wrap_clamp"] == 0
        x, Pm = m.ekf_state(WATCHED)
    rec = records[WATCHED]
    with pkg.QuasarMapper(max_agent=3) as m2:
        m2.ekf_init(WATCHED, rec[0, 0], [rec[0, 1], rec[0, 2], rec[0, 3], 0.0, 0.0, 0.0])
        for t, om, ve in step_records(rec, R.MPT):
            m2.ekf_step([WATCHED], [om], [t], z_v=[ve], z_omega=[om])
        x2, P2 = m2.ekf_state(WATCHED)
    assert np.array_equal(x, x2), (x, x2)
    assert np.array_equal(Pm, P2), np.abs(Pm - P2).max()
