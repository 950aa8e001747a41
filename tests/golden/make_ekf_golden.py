#!/usr/bin/env python3
"""Golden states of the firmware's own EKF.  RUNS ONLY IN THE BUILD CONTAINER (needs oracle/_ref/ekf_ref, which
__graft_entry__.build() compiles from /root/reference where that tree exists), like make_golden.py.

Builds the operation streams S1-S6 (tests/ekf_reference.py has the layout), runs them through oracle/_ref/ekf_ref (the
unmodified AgentFirmware_Bot1/ekf.cpp behind oracle/ref/ekf_driver.cpp) and through oracle/_ref/ekf_ref_esp32
(esp32_firmware/lib/ekf/ekf.cpp), requires identical output of the two, and writes tests/golden/ekf_ref.npz.

An `I` operation is a new EKF object followed by init: EKF::init alone keeps the covariance, the firmware calls it once per
object, and qs_ekf_init / qso_ekf_init are "constructor + init".  No stream holds a NaN time: the reference goes on with
dt = NaN (`dt <= 0` is false), csrc/ekf.hip skips on purpose.

    python tests/golden/make_ekf_golden.py
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
import ekf_reference as E  # noqa: E402
import ekf_rules as R  # noqa: E402
from npz_fixed import write_npz  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ekf_ref")
REF_BIN_ESP32 = os.path.join(ROOT, "oracle", "_ref", "ekf_ref_esp32")
PI = float(np.pi)
X0 = [1.25, -2.5, 0.7, -0.35, 0.1, 0.02]            # general: non-zero bias, negative v


class Stream:
    def __init__(self):
        self.op, self.a, self.b, self.x0 = [], [], [], []

    def I(self, t, x0):
        self.op.append(E.OP_I); self.a.append(float(t)); self.b.append(0.0); self.x0.append([float(v) for v in x0])

    def P(self, omega, t):
        self.op.append(E.OP_P); self.a.append(float(omega)); self.b.append(float(t))

    def U(self, z_v, z_omega):
        self.op.append(E.OP_U); self.a.append(float(z_v)); self.b.append(float(z_omega))

    def arrays(self):
        return (np.array(self.op, dtype=np.uint8), np.array(self.a, dtype=np.float64), np.array(self.b, dtype=np.float64),
                np.array(self.x0, dtype=np.float64).reshape(-1, 6))


def s1():
    """predict and update before init (no-ops on the constructed object), then init with a general x0 and a short run."""
    s = Stream()
    s.P(0.3, 1.0); s.U(0.2, 0.1); s.P(-1.0, 2.0); s.U(-0.4, 0.0)
    s.I(5.0, X0)
    rng = np.random.default_rng(1)
    t = 5.0
    for k in range(24):
        t += 0.05
        s.P(rng.normal(0.4, 0.3), t)
        if k % 3 == 2:
            s.U(rng.normal(-0.3, 0.05), rng.normal(0.4, 0.1))
    return s


def s2():
    """Time edges."""
    s = Stream()
    rng = np.random.default_rng(2)
    s.I(100.0, X0)
    s.P(0.5, 100.0)                  # dt == 0: skipped
    s.P(0.5, 99.5)                   # dt < 0: skipped, and the last accepted time stays 100.0
    s.P(0.5, 100.05)                 # dt counts from 100.0, not from 99.5
    s.U(-0.3, 0.45)
    s.P(0.5, 100.05)                 # dt == 0 again, after an update
    s.P(-0.2, 100.05 + 1e-9)         # dt = 1e-9
    s.P(0.03, 110.05 + 1e-9)         # dt = 10
    s.U(-0.2, 0.0)
    s.I(-50.0, X0)                   # negative stamps
    t = -50.0
    for step in (0.05, 0.0, -0.25, 0.3, 0.05, -0.01, 0.02, 49.7, 0.05, 0.05):      # crosses zero
        t += step
        s.P(rng.normal(0.0, 0.5), t)
        s.U(rng.normal(-0.3, 0.05), rng.normal(0.0, 0.5))
    s.I(1.7e9, [0.5, 0.25, -1.0, 0.2, 0.0, 0.0])            # epoch stamps, 50 ms steps
    t = 1.7e9
    for k in range(120):
        t += 0.05
        s.P(rng.normal(0.3, 0.2), t)
        if k % 4 == 3:
            s.U(rng.normal(0.2, 0.02), rng.normal(0.3, 0.05))
    return s


def s3():
    """Wrap edges.  The first four cases start at theta = target - 0.5 (exact: same binade as pi) and predict with
    omega * dt = 0.5 and no bias, so theta_new is the target itself."""
    s = Stream()
    rng = np.random.default_rng(3)
    up, down = float(np.nextafter(PI, np.inf)), float(np.nextafter(-PI, -np.inf))
    for target, sign in ((PI, 1.0), (up, 1.0), (-PI, -1.0), (down, -1.0)):
        start = target - sign * 0.5
        assert start + sign * 0.5 == target
        s.I(0.0, [0.0, 0.0, start, 0.3, 0.0, 0.0])
        s.P(sign * 0.5, 1.0)
        s.P(0.1, 1.5); s.U(0.3, 0.1)
    # |omega * dt| up to 20: one wrap only, the heading stays outside +-pi and cos / sin are taken of it
    s.I(0.0, [0.0, 0.0, 0.3, 0.4, 0.0, 0.01])
    t = 0.0
    for k, turn in enumerate([20.0, 9.0, -17.5, 19.9, -20.0, 12.0, -3.0, 20.0, 20.0, -8.0] + list(rng.uniform(-20, 20, 30))):
        dt = (0.5, 1.0, 2.0)[k % 3]
        t += dt
        s.P(turn / dt, t)
        if k % 4 == 1:
            s.U(rng.normal(0.4, 0.05), turn / dt)
    # updates that push theta across +-pi: update never wraps
    for sign in (1.0, -1.0):
        s.I(0.0, [0.0, 0.0, sign * (PI - 0.02), 0.2, 0.0, 0.0])
        t = 0.0
        for _ in range(5):
            t += 0.1
            s.P(0.0, t)
        s.U(0.2, sign * 40.0)        # cov(theta, omega) > 0 after the predicts: the innovation moves theta beyond +-pi
        for _ in range(4):
            t += 0.1
            s.P(sign * 0.1, t)       # the next predict wraps it back
            s.U(0.2, sign * 0.1)
    return s


def s4():
    """2 000 predicts without an update (the loop of AgentFirmware_Bot1.ino:697-702: predict at millis() / 1000.0 every
    pass, passes of 2-7 ms and now and then two in the same millisecond), then a run of updates without a predict."""
    s = Stream()
    rng = np.random.default_rng(4)
    ms = 3000
    s.I(ms / 1000.0, [0.0, 0.0, 0.0, 0.25, 0.0, 0.0])
    steps = rng.choice([0, 2, 3, 5, 7], size=2000, p=[0.05, 0.3, 0.3, 0.25, 0.1])
    gyro = np.round(rng.normal(0.0, 0.02, 2000) + 0.6 * np.sin(np.arange(2000) / 150.0), 4)
    for k in range(2000):
        ms += int(steps[k])
        s.P(gyro[k], ms / 1000.0)
    for k in range(100):
        s.U(round(float(rng.normal(0.25, 0.02)), 4), round(float(rng.normal(0.3, 0.05)), 4))
    return s


def s5():
    """The loop of esp32_firmware/src/main.cpp:176-188: predict every 10 ms, update every 2 000 ms, times millis() / 1000.0,
    over a drive-and-turn profile of 5 000 ticks (4 s straight at 0.2 m/s, 1.6 s turning at +-1 rad/s)."""
    s = Stream()
    rng = np.random.default_rng(5)
    ms = 1500
    s.I(ms / 1000.0, [0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    last_pub = ms
    noise = np.round(rng.normal(0.0, 0.01, 5000), 4)
    for k in range(5000):
        ms += 10
        phase = (k % 560)
        turning = phase >= 400
        sign = 1.0 if (k // 560) % 3 != 2 else -1.0
        omega = sign * 1.0 if turning else 0.0
        v = 0.0 if turning else 0.2
        s.P(omega + 0.02 + noise[k], ms / 1000.0)            # a gyro with a constant bias of 0.02 rad/s
        if ms - last_pub >= 2000:
            last_pub = ms
            s.U(round(v + float(rng.normal(0.0, 0.01)), 4), round(omega + float(rng.normal(0.0, 0.02)), 4))
    return s


def run_reference(binary, streams):
    """All streams through one process (an `N` line between them) -> {name: float64 [n_ops, 42]}."""
    lines = []
    for name, (op, a, b, x0) in streams.items():
        lines.append("N")
        k = 0
        for o, va, vb in zip(op.tolist(), a.tolist(), b.tolist()):
            if o == E.OP_I:
                lines.append("I " + " ".join(float(v).hex() for v in [va] + x0[k].tolist())); k += 1
            else:
                lines.append(("P " if o == E.OP_P else "U ") + float(va).hex() + " " + float(vb).hex())
    raw = subprocess.run([binary], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout
    out = np.frombuffer(raw, dtype=np.float64).reshape(-1, 42)
    assert len(out) == sum(len(v[0]) for v in streams.values())
    res, at = {}, 0
    for name, v in streams.items():
        res[name] = out[at:at + len(v[0])]; at += len(v[0])
    return raw, res


def main():
    streams = {name: fn().arrays() for name, fn in (("S1", s1), ("S2", s2), ("S3", s3), ("S4", s4), ("S5", s5))}
    wired = {}
    for name, spec in (("S6E", R.E_ROWS["spin_both_ways"]), ("S6F", R.F_ROWS["updates_without_predicts"])):
        pk, times, records = R.build(spec)
        assert spec["max_agent"] == 1 and len(pk) >= R.SCAN_MIN_BATCH
        op, a, b, x0, last = E.wiring(records[1], R.MPT)
        streams[name] = (op, a, b, x0)
        wired[name] = (pk, times, last)
    raw, res = run_reference(REF_BIN, streams)
    raw2, _ = run_reference(REF_BIN_ESP32, streams)
    assert raw == raw2, "AgentFirmware_Bot1/ekf.cpp and esp32_firmware/lib/ekf/ekf.cpp disagree"
    assert np.isfinite(np.frombuffer(raw, dtype=np.float64)).all()

    # what the streams promise, read off the reference's own output
    x = res["S1"][:, :6]; Pm = res["S1"][:, 6:]
    assert (x[:4] == 0).all() and (Pm[:4] == np.eye(6).reshape(36)).all() and (x[4] == X0).all()
    th = res["S2"][:, 2]
    assert th[1] == th[0] == th[2] and th[3] == X0[2] + (0.5 - X0[5]) * (100.05 - 100.0) and th[5] == th[4]
    th = res["S3"][:, 2]
    up, down = float(np.nextafter(PI, np.inf)), float(np.nextafter(-PI, -np.inf))
    assert th[1] == PI and th[5] == up - 2 * PI and th[9] == -PI and th[13] == down + 2 * PI
    op3 = streams["S3"][0]
    assert np.abs(th).max() > 3 * PI                                    # the heading stays outside +-pi after a big turn
    crossed = [i for i in range(1, len(th)) if op3[i] == E.OP_U and abs(th[i]) > PI and abs(th[i - 1]) <= PI]
    assert len(crossed) >= 2, crossed                                   # updates pushed theta across +pi and across -pi
    assert {np.sign(th[i]) for i in crossed} == {1.0, -1.0}
    for name in wired:
        th = res[name][:, 2]
        op = streams[name][0]
        pred = np.nonzero(op == E.OP_P)[0]
        jumps = np.abs(th[pred] - th[pred - 1]) > PI
        print(f"{name}: {len(op)} operations, {int(jumps.sum())} predicts that wrapped")

    out = {}
    for name, (op, a, b, x0) in streams.items():
        if name in wired:
            pk, times, last = wired[name]
            n = len(pk)
            recs = np.array(sorted(set(range(63, n, 64)) | {n - 1}), dtype=np.int32)
            rows = last[recs]
            out[name + "_packets"], out[name + "_times"], out[name + "_recs"] = pk, times, recs
        else:
            rows = E.stored_rows(len(op))
        out[name + "_op"], out[name + "_a"], out[name + "_b"], out[name + "_x0"] = op, a, b, x0
        out[name + "_rows"] = rows.astype(np.int32)
        out[name + "_x"] = res[name][rows, :6]
        out[name + "_P"] = res[name][rows, 6:].reshape(-1, 6, 6)
        print(f"{name}: {len(op)} operations, {len(rows)} stored rows")
    out["metres_per_tick"] = np.array(R.MPT)
    path = os.path.join(HERE, "ekf_ref.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
