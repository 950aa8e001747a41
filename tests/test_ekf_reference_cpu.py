"""oracle.c's EKF against the firmware's own arithmetic: tests/golden/ekf_ref.npz holds what AgentFirmware_Bot1/ekf.cpp,
compiled unmodified against the stand-in headers of oracle/ref/stub, computed on the streams S1-S6
(tests/golden/make_ekf_golden.py; esp32_firmware/lib/ekf/ekf.cpp gave the same bytes).

Bar: equal bits, x and P, at every stored row of every stream.  Measured in the build container (glibc's cos / sin on both
sides, the stand-in's products in ascending k like oracle.c's):

| Stream | Rows | Worst |x - ref| | Worst |P - ref| | Bar |
| --- | --- | --- | --- | --- |
| S1 before init, general x0 | 37 | 0 | 0 | 0 |
| S2 time edges | 181 | 0 | 0 | 0 |
| S3 wrap edges | 97 | 0 | 0 | 0 |
| S4 predicts only, updates only | 33 of 2 101 | 0 | 0 | 0 |
| S5 ESP32 loop | 79 of 5 026 | 0 | 0 | 0 |
| S6E wired, wraps | 64 of 8 191 | 0 | 0 | 0 |
| S6F wired, time edges | 64 of 8 189 | 0 | 0 | 0 |

The rows are compared as bytes, so the sign of a zero counts too.  An `I` operation is a new filter followed by init
(EKF::init alone keeps the covariance; the firmware calls it once, and qso_ekf_init is "constructor + init").

NaN times are in no stream: the reference goes on with dt = NaN because `dt <= 0` is false, while csrc/ekf.hip:77 and the
ingest kernels skip such a step on purpose.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
import ekf_reference as E
import ekf_rules as R


@pytest.fixture(scope="module")
def fx():
    return E.load()


def replay_oracle(fx, s):
    """Every operation of stream s through qso_ekf_init / predict / update -> x [n, 6], P [n, 6, 6] after each."""
    ek = orc.OracleEKF(1)
    xs, Ps = [], []
    for op, a, b, x0 in E.ops(fx, s):
        if op == E.OP_I:
            ek.init(0, a, x0)
        elif op == E.OP_P:
            ek.predict(0, a, b)
        else:
            ek.update(0, a, b)
        xs.append(ek.state(0)); Ps.append(ek.cov(0))
    return np.array(xs), np.array(Ps)


@pytest.mark.parametrize("s", E.STEP_STREAMS + E.WIRED_STREAMS)
def test_oracle_equals_the_firmware_filter(fx, s):
    x, Pm = replay_oracle(fx, s)
    rows = fx[s + "_rows"]
    assert np.array_equal(rows, E.stored_rows(len(x))) or s in E.WIRED_STREAMS
    dx, dP = np.abs(x[rows] - fx[s + "_x"]).max(), np.abs(Pm[rows] - fx[s + "_P"]).max()
    print(f"EKF-REF {s}: {len(rows)} rows of {len(x)}; worst |x - ref| {dx:.3e}, worst |P - ref| {dP:.3e}")
    assert np.isfinite(fx[s + "_x"]).all() and np.isfinite(fx[s + "_P"]).all()
    bad = [int(r) for j, r in enumerate(rows)
           if x[r].tobytes() != fx[s + "_x"][j].tobytes() or Pm[r].tobytes() != fx[s + "_P"][j].tobytes()]
    assert not bad, f"first row whose bits differ: operation {bad[0]}"


def test_streams_hold_what_they_promise(fx):
    """Read off the fixture alone, so the edges stay in it when it is regenerated."""
    x, Pm = fx["S1_x"], fx["S1_P"]
    assert (fx["S1_op"][:4] != E.OP_I).all() and fx["S1_op"][4] == E.OP_I
    assert (x[:4] == 0).all() and (Pm[:4] == np.eye(6)).all()                        # no-ops on the constructed object
    assert fx["S1_x0"][0, 5] != 0 and fx["S1_x0"][0, 3] < 0
    op, t = fx["S2_op"], np.where(fx["S2_op"] == E.OP_P, fx["S2_b"], np.nan)
    pred = np.nonzero(op == E.OP_P)[0]
    same = [i for i in pred if (fx["S2_x"][i] == fx["S2_x"][i - 1]).all()]           # skipped predicts
    assert len(same) >= 5 and np.nanmin(t) < 0 and np.nanmax(t) > 1.7e9
    th = fx["S3_x"][:, 2]
    up, down = np.nextafter(np.pi, np.inf), np.nextafter(-np.pi, -np.inf)
    assert th[1] == np.pi and th[5] == up - 2 * np.pi and th[9] == -np.pi and th[13] == down + 2 * np.pi
    assert np.abs(th).max() > 3 * np.pi
    crossed = [i for i in range(1, len(th)) if fx["S3_op"][i] == E.OP_U and abs(th[i]) > np.pi >= abs(th[i - 1])]
    assert {float(np.sign(th[i])) for i in crossed} == {1.0, -1.0}
    assert (fx["S4_op"][1:2001] == E.OP_P).all() and (fx["S4_op"][2001:] == E.OP_U).all() and len(fx["S4_op"]) == 2101
    assert (fx["S5_op"] == E.OP_P).sum() == 5000 and (fx["S5_op"] == E.OP_U).sum() == 25
    for s in E.WIRED_STREAMS:
        assert len(fx[s + "_packets"]) >= R.SCAN_MIN_BATCH
    for name in fx.files:                                                            # no NaN time, nor any other
        if fx[name].dtype == np.float64:
            assert not np.isnan(fx[name]).any(), name


@pytest.mark.parametrize("s", E.WIRED_STREAMS)
def test_wiring_of_the_oracle_mapper(fx, s):
    """qso_ekf_packet (oracle.c:618-644) over the stored packets and receive times, fed in slices that end on the stored
    packets: the state after each equals the reference's on the reduced (omega_m, t, v_enc)."""
    pk, times, recs = fx[s + "_packets"], fx[s + "_times"], fx[s + "_recs"]
    rec = pk.view(R.P.PACKET_DTYPE).reshape(len(pk))
    records = np.stack([times] + [rec[k].astype(np.float64) for k in ("x", "y", "yaw", "enc")], axis=1)
    op, a, b, x0, last = E.wiring(records, E.mpt(fx))
    assert np.array_equal(op, fx[s + "_op"]) and np.array_equal(a, fx[s + "_a"]) and np.array_equal(b, fx[s + "_b"])
    assert np.array_equal(x0, fx[s + "_x0"]) and np.array_equal(last[recs], fx[s + "_rows"])
    o = orc.OracleMapper(max_agent=1)
    o.enable_ekf(E.mpt(fx))
    lo = 0
    for j, k in enumerate(recs.tolist()):
        o.feed_stream(pk[lo:k + 1], None, times[lo:k + 1])
        lo = k + 1
        x, Pm = o.ekf_state(1)
        assert x.tobytes() == fx[s + "_x"][j].tobytes() and Pm.tobytes() == fx[s + "_P"][j].tobytes(), f"after packet {k}"


@pytest.mark.parametrize("s", E.WIRED_STREAMS)
def test_long_double_restatement_within_its_bar(fx, s):
    """ekf_rules.sequential_ld (np.longdouble) against the reference's doubles, by the 1e-11 of tests/test_ekf_rules_cpu.py:
    after the first 1 024 packets and after all of them."""
    pk, times = fx[s + "_packets"], fx[s + "_times"]
    rec = pk.view(R.P.PACKET_DTYPE).reshape(len(pk))
    records = np.stack([times] + [rec[k].astype(np.float64) for k in ("x", "y", "yaw", "enc")], axis=1)
    recs = fx[s + "_recs"].tolist()
    for k in (1023, len(pk) - 1):
        j = recs.index(k)
        x, Pm, _ = R.sequential_ld(records[:k + 1], E.mpt(fx))
        ex, eP = E.rel_err(x, fx[s + "_x"][j]), E.rel_err(Pm, fx[s + "_P"][j])
        print(f"EKF-REF {s} long double after packet {k}: x {ex:.3e}, P {eP:.3e} (bar 1e-11)")
        assert ex < 1e-11 and eP < 1e-11


@pytest.mark.skipif(not os.path.exists(orc.EKF_REF), reason="the reference binary is built in the build container only")
def test_reference_binary_reproduces_the_fixture(fx):
    lines = []
    for s in E.STEP_STREAMS + E.WIRED_STREAMS:
        lines.append("N")
        for op, a, b, x0 in E.ops(fx, s):
            if op == E.OP_I:
                lines.append("I " + " ".join(float(v).hex() for v in [a] + x0.tolist()))
            else:
                lines.append(("P " if op == E.OP_P else "U ") + float(a).hex() + " " + float(b).hex())
    raw = subprocess.run([orc.EKF_REF], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout
    out = np.frombuffer(raw, dtype=np.float64).reshape(-1, 42)
    at = 0
    for s in E.STEP_STREAMS + E.WIRED_STREAMS:
        rows = fx[s + "_rows"] + at
        assert out[rows, :6].tobytes() == fx[s + "_x"].tobytes() and out[rows, 6:].tobytes() == fx[s + "_P"].tobytes(), s
        at += len(fx[s + "_op"])
    assert at == len(out)
