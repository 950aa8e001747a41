"""The EKF kernels (csrc/ekf.hip, csrc/ekf_scan.hip) against the firmware's own arithmetic: tests/golden/ekf_ref.npz holds
what AgentFirmware_Bot1/ekf.cpp, compiled unmodified, computed on the streams S1-S6 (tests/golden/make_ekf_golden.py;
tests/test_ekf_reference_cpu.py holds oracle.c to the same file, bit for bit).  Only the fixture is read.

Bar: _ekf_close of tests/test_gpu_parity.py, unchanged: 1e-9 x max(1, |ref|max) on x and on P.

| Group | What runs | Compared |
| --- | --- | --- |
| step S1-S5 | qs_ekf_init, then one qs_ekf_step per operation: a P is a step without update; a U is a step with update whose time is the last accepted one, so its predict is skipped | every stored row |
| many bots | n in {63, 64, 65} bots (the kernel's block is 64), bot b on stream S((b - 1) mod 5 + 1), the first 192 operations of each. Per operation index one qs_ekf_step call for the bots whose operation is a P and one for those whose is a U; a call carries all n bots where every stream holds the same kind (asserted: at least 8 such calls), 13 to 52 elsewhere | every 16th operation and each stream's last |
| ingest S6, serial | the stored packets and receive times in batches of 64 and of 1 024 (below SCAN_MIN_BATCH) | after every batch |
| ingest S6, scan | the same in one batch of 4 096 (ekf_scan.hip) | after the batch; ekf_wrap_clamp == 0 everywhere |

A bot that was never initialised reports the constructed filter (x = 0, P = I), as S1's first rows have it.  NaN times are
in no stream: the reference goes on with dt = NaN because `dt <= 0` is false; csrc/ekf.hip:77 skips such a step on purpose.
"""
import numpy as np
import pytest
import torch  # noqa: F401  before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import load_pkg
import ekf_reference as E
import ekf_rules as R
from test_gpu_parity import _ekf_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def fx():
    return E.load()


class Ref:
    """The fixture's rows in the shape _ekf_close asks its second argument for."""

    def __init__(self):
        self.rows = {}

    def ekf_state(self, b):
        return self.rows[b]


class Worst:
    def __init__(self, label):
        self.label, self.worst, self.n = label, 0.0, 0

    def close(self, m, ref, bots):
        for b in bots:
            x, Pm = m.ekf_state(b)
            xo, Po = ref.ekf_state(b)
            self.worst = max(self.worst, E.rel_err(x, xo), E.rel_err(Pm, Po))
            self.n += 1
        _ekf_close(m, ref, bots)

    def report(self):
        print(f"EKF-REF {self.label}: {self.n} comparisons, worst error {self.worst:.3e} = {self.worst / R.BAR:.2e} of the bar")


class Replayer:
    """One bot's stream through the step API; keeps the last accepted time for update-only steps."""

    def __init__(self, m, bot):
        self.m, self.bot, self.last_t, self.init = m, bot, 0.0, False

    def step_args(self, op, a, b):
        """-> (omega, t, z_v, z_omega) of the qs_ekf_step entry that stands for a P or a U."""
        if op == E.OP_P:
            if self.init and b - self.last_t > 0:
                self.last_t = b
            return a, b, None, None
        return 0.0, self.last_t, a, b

    def do_init(self, t, x0):
        self.m.ekf_init(self.bot, t, x0)
        self.last_t, self.init = t, True


@pytest.mark.parametrize("s", E.STEP_STREAMS)
def test_step_api_equals_the_firmware_filter(pkg, fx, s):
    rows = {int(r): j for j, r in enumerate(fx[s + "_rows"])}
    ref, w = Ref(), Worst(f"step {s}")
    with pkg.QuasarMapper(max_agent=2) as m:
        rp = Replayer(m, 2)
        for i, (op, a, b, x0) in enumerate(E.ops(fx, s)):
            if op == E.OP_I:
                rp.do_init(a, x0)
            else:
                om, t, zv, zo = rp.step_args(op, a, b)
                if zv is None:
                    m.ekf_step([2], [om], [t])
                else:
                    m.ekf_step([2], [om], [t], z_v=[zv], z_omega=[zo])
            if i in rows:
                ref.rows[2] = (fx[s + "_x"][rows[i]], fx[s + "_P"][rows[i]])
                w.close(m, ref, (2,))
        assert i == max(rows)
        x1, P1 = m.ekf_state(1)
        assert (x1 == 0).all() and (P1 == np.eye(6)).all()                  # the neighbour was never touched
    w.report()


@pytest.mark.parametrize("n", [63, 64, 65])
def test_one_step_call_over_many_bots(pkg, fx, n):
    limit = 192
    streams = {s: E.ops(fx, s)[:limit] for s in E.STEP_STREAMS}
    rows = {s: {int(r): j for j, r in enumerate(fx[s + "_rows"])} for s in E.STEP_STREAMS}
    of = {b: E.STEP_STREAMS[(b - 1) % len(E.STEP_STREAMS)] for b in range(1, n + 1)}
    ref, w = Ref(), Worst(f"many bots n={n}")
    full_calls = 0
    with pkg.QuasarMapper(max_agent=n) as m:
        rp = {b: Replayer(m, b) for b in of}
        for i in range(limit):
            pred, upd = [], []
            for b, s in of.items():
                if i >= len(streams[s]):
                    continue
                op, a, bb, x0 = streams[s][i]
                if op == E.OP_I:
                    rp[b].do_init(a, x0)
                else:
                    (pred if op == E.OP_P else upd).append((b,) + rp[b].step_args(op, a, bb))
            full_calls += len(pred) == n or len(upd) == n
            if pred:
                m.ekf_step([p[0] for p in pred], [p[1] for p in pred], [p[2] for p in pred])
            if upd:
                m.ekf_step([u[0] for u in upd], [u[1] for u in upd], [u[2] for u in upd],
                           z_v=[u[3] for u in upd], z_omega=[u[4] for u in upd])
            check = [b for b, s in of.items() if i in rows[s] and i < len(streams[s]) and (i % 16 == 15 or i == len(streams[s]) - 1)]
            for b in check:
                j = rows[of[b]][i]
                ref.rows[b] = (fx[of[b] + "_x"][j], fx[of[b] + "_P"][j])
            w.close(m, ref, check)
    assert w.n >= n * 2 and full_calls >= 8, full_calls                 # calls of exactly n entries: across the block edge
    w.report()


@pytest.mark.parametrize("s", E.WIRED_STREAMS)
@pytest.mark.parametrize("batch", [64, 1024, 4096])
def test_ingest_equals_the_firmware_filter(pkg, fx, s, batch):
    pk, times, recs = fx[s + "_packets"], fx[s + "_times"], fx[s + "_recs"].tolist()
    assert len(pk) == 4096 == R.SCAN_MIN_BATCH and (batch < R.SCAN_MIN_BATCH or batch == len(pk))
    ref, w = Ref(), Worst(f"ingest {s} batches of {batch} ({'scan' if batch >= R.SCAN_MIN_BATCH else 'serial'})")
    with pkg.QuasarMapper(max_agent=1, enable_ekf=True, ekf_metres_per_tick=E.mpt(fx)) as m:
        for lo in range(0, len(pk), batch):
            hi = min(lo + batch, len(pk))
            m.ingest_array(pk[lo:hi], recv_time=times[lo:hi])
            assert m.last_batch()[0].all()
            j = recs.index(hi - 1)
            ref.rows[1] = (fx[s + "_x"][j], fx[s + "_P"][j])
            w.close(m, ref, (1,))
            assert m.counters()["ekf_wrap_clamp"] == 0
    w.report()
