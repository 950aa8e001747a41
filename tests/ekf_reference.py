"""Reader of tests/golden/ekf_ref.npz: operation streams and what the firmware's own ekf.cpp computed on them
(tests/golden/make_ekf_golden.py wrote it through oracle/ref/ekf_driver.cpp).  Plain numpy: no device, no ctypes.

Per stream S (STEP_STREAMS and WIRED_STREAMS):
  S_op    uint8 [n]     0 = I (a new EKF object, then init), 1 = P (predict), 2 = U (update)
  S_a, S_b  float64 [n] I: t, -;  P: omega, t;  U: z_v, z_omega
  S_x0    float64 [k, 6]  the x0 of the k-th I
  S_rows  int32 [m]     the operations after which the state is stored: all of them for a short stream, every 64th and the
                        last for a long one
  S_x     float64 [m, 6], S_P float64 [m, 6, 6]   the reference's state and covariance after those operations
Wired streams (S6) add S_packets uint8 [N, 42], S_times float64 [N] and S_recs int32 [m]: row j is the state after packet
S_recs[j], whose last operation is S_rows[j].  metres_per_tick is the factor the reduction used.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP_STREAMS = ("S1", "S2", "S3", "S4", "S5")
WIRED_STREAMS = ("S6E", "S6F")
OP_I, OP_P, OP_U = 0, 1, 2
PI = np.pi
LONG = 256                          # streams with more operations store every 64th row and the last


def load():
    return np.load(os.path.join(GOLDEN, "ekf_ref.npz"), allow_pickle=False)


def mpt(fx):
    return float(fx["metres_per_tick"].reshape(-1)[0])


def ops(fx, s):
    """[(op, a, b, x0 or None)] of stream s."""
    out, k = [], 0
    x0 = fx[s + "_x0"]
    for op, a, b in zip(fx[s + "_op"].tolist(), fx[s + "_a"].tolist(), fx[s + "_b"].tolist()):
        if op == OP_I:
            out.append((op, a, b, x0[k])); k += 1
        else:
            out.append((op, a, b, None))
    return out


def stored_rows(n):
    if n <= LONG:
        return np.arange(n, dtype=np.int32)
    rows = list(range(63, n, 64))
    if rows[-1] != n - 1:
        rows.append(n - 1)
    return np.array(rows, dtype=np.int32)


def wiring(records, metres_per_tick):
    """oracle.c:618-623 on a bot's records (t, x, y, yaw, enc) in Python doubles, one rounding per operation ->
    op, a, b, x0 arrays as stored, and per record the index of the last operation up to and including it."""
    op, a, b, last = [OP_I], [float(records[0][0])], [0.0], [0]
    x0 = np.array([[records[0][1], records[0][2], records[0][3], 0.0, 0.0, 0.0]], dtype=np.float64)
    pi = float(PI)
    for k in range(1, len(records)):
        t, _, _, yaw, enc = (float(v) for v in records[k])
        tp, _, _, yawp, encp = (float(v) for v in records[k - 1])
        dt = t - tp
        if dt > 0:
            dyaw = yaw - yawp
            if dyaw > pi:
                dyaw = dyaw - 2 * pi
            elif dyaw < -pi:
                dyaw = dyaw + 2 * pi
            inv_dt = 1.0 / dt
            omega_m = dyaw * inv_dt
            v_enc = ((enc - encp) * metres_per_tick) * inv_dt
            op += [OP_P, OP_U]; a += [omega_m, v_enc]; b += [t, omega_m]
        last.append(len(op) - 1)
    return (np.array(op, dtype=np.uint8), np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), x0,
            np.array(last, dtype=np.int32))


def rel_err(got, ref):
    """The measure of tests/test_gpu_parity.py::_ekf_close: max-abs difference over max(1, |ref|max)."""
    got = np.asarray(got, dtype=np.longdouble); ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))
