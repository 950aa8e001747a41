"""Servo-sweep packets on the CPU: wire formats, the standalone receiver's CSV, and the UDP front-end's run splitting
(a stub in place of the HIP mapper)."""
import csv
import importlib
import socket
import struct
import time

import numpy as np

from conftest import PKG_NAME


def _P():
    return importlib.import_module(PKG_NAME + ".protocol")


def test_sweep_formats_round_trip():
    P = _P()
    assert (P.PACKET_SIZE_V0, P.PACKET_SIZE_V0_ODO) == (743, 751)
    assert P.PACKET_FMT_V0_ODO == "<4sBfffiIH181f" and P.PACKET_DTYPE_V0_ODO.itemsize == 751
    rng = np.random.default_rng(5)
    r = rng.uniform(0.0, 3.0, 181).astype(np.float32)
    a = P.pack_v0(2, 1.5, -2.25, 0.5, r)
    assert len(a) == 743 and struct.unpack(P.PACKET_FMT_V0, a)[:6] == (b"QSRL", 2, 1.5, -2.25, 0.5, 181)
    agent, x, y, yaw, rr = P.unpack_v0(a)
    assert (agent, x, y, yaw) == (2, 1.5, -2.25, 0.5) and (rr == r).all()
    b = P.pack_v0_odo(1, 0.25, 0.75, -1.0, -12, 7, r, scan_count=90)
    assert len(b) == 751
    u = struct.unpack(P.PACKET_FMT_V0_ODO, b)
    assert u[:8] == (b"QSRL", 1, 0.25, 0.75, -1.0, -12, 7, 90) and np.array_equal(np.float32(u[8:]), r)
    agent, x, y, yaw, enc, v2v, rr = P.unpack_v0_odo(b)
    assert (agent, x, y, yaw, enc, v2v) == (1, 0.25, 0.75, -1.0, -12, 7) and (rr == r).all()
    assert P.unpack_v0_odo(b[:743]) is None and P.unpack_v0_odo(b"QSRX" + b[4:]) is None
    # the vectorised packer writes the same bytes
    vec = P.pack_sweeps([1], [0.25], [0.75], [-1.0], r[None, :], enc=[-12], v2v=[7], scan_count=90)
    assert vec.shape == (1, 751) and vec.tobytes() == b
    vec0 = P.pack_sweeps([2], [1.5], [-2.25], [0.5], r[None, :], odometry=False)
    assert vec0.shape == (1, 743) and vec0.tobytes() == a


def test_sweep_csv_to_packets(tmp_path):
    P = _P()
    replay = importlib.import_module(PKG_NAME + ".replay")
    path = tmp_path / "agent_2_log.csv"
    rng = np.random.default_rng(9)
    rows = []
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["timestamp", "idx", "x", "y", "yaw", "encoder", "v2v_link"] + [f"r_{i}" for i in range(181)])
        for k in range(5):
            rr = [float(v) for v in rng.uniform(0.0, 4.0, 181)]
            row = [1000.0 + k, 17, 0.1 * k, -0.2 * k, 0.3 * k - 1.0, 40 * k, 3] + rr
            rows.append(row)
            w.writerow(row)
    pk, t = replay.sweep_csv_to_packets(str(path))
    assert pk.shape == (5, 751) and pk.dtype == np.uint8
    assert t.tolist() == [1000.0 + k for k in range(5)]
    for k, row in enumerate(rows):
        agent, x, y, yaw, enc, v2v, rr = P.unpack_v0_odo(pk[k].tobytes())
        assert agent == 2 and enc == 40 * k and v2v == 3
        assert (x, y, yaw) == tuple(float(np.float32(v)) for v in row[2:5])
        assert (rr == np.float32(row[7:])).all()
    pk1, _ = replay.sweep_csv_to_packets(str(path), agent=1)
    assert (pk1[:, 4] == 1).all()


class StubMapper:
    """ingest_array / ingest_sweeps with the decoder's accept rules and the library's sequence rule (seq0 None: continue the
    mapper's own counter, 1 per packet, 46 per sweep); remembers every call with the seq0 it was given and the start it got."""

    def __init__(self, next_seq=0):
        self.calls = []
        self.next_seq = next_seq

    def _seq(self, seq0, n):
        start = self.next_seq if seq0 is None else seq0
        self.next_seq = start + n
        return start

    def _accept(self, buf, lens, sizes):
        ok = np.isin(lens, sizes)
        magic = (buf[:, 0] == ord("Q")) & (buf[:, 1] == ord("S")) & (buf[:, 2] == ord("R")) & (buf[:, 3] == ord("L"))
        agent = (buf[:, 4] >= 1) & (buf[:, 4] <= 2)
        return (ok & magic & agent).astype(np.uint8)

    def ingest_array(self, buf, lens, times, seq0=None):
        self.calls.append(("pkt", buf.shape, lens.tolist(), seq0, self._seq(seq0, len(buf))))
        self._acc = self._accept(buf, lens, (41, 42))
        self._pose = np.zeros((len(buf), 3))

    def last_batch(self):
        return self._acc, self._pose

    def ingest_sweeps(self, buf, lens, seq0=None):
        self.calls.append(("sweep", buf.shape, lens.tolist(), seq0, self._seq(seq0, 46 * len(buf))))
        self._sacc = self._accept(buf, lens, (buf.shape[1],))
        x = buf[:, 5:9].copy().view("<f4")[:, 0].astype(np.float64)
        y = buf[:, 9:13].copy().view("<f4")[:, 0].astype(np.float64)
        self._spose = np.stack([x, y, np.zeros(len(buf))], axis=1)

    def last_sweeps(self):
        return self._sacc, self._spose

    def zone(self, bot):
        return None

    def zone_packet(self, bot, online=True):
        return struct.pack("<4sffff", b"ZONE", 999.0, 999.0, -999.0, -999.0)


def _pair():
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    bot = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    bot.bind(("127.0.0.1", 0))
    return srv, bot


def test_mission_control_sweep_runs():
    P = _P()
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    srv, bot = _pair()
    port = srv.getsockname()[1]
    mc = fe.MissionControl(StubMapper(next_seq=1000), sock=srv, sweeps=True)    # the mapper already holds 1000 sequence numbers
    r = np.full(181, 0.5, dtype=np.float32)
    p1 = P.pack_packet(1, 0.1, 0.2, 0.3, 1, 2, 0.5, 0.6, 0.7, 0.8, 0)
    s_odo = P.pack_v0_odo(2, 3.0, 4.0, 0.0, 0, 0, r)
    s_v0 = P.pack_v0(1, -1.0, -2.0, 0.0, r)
    seq = [p1, p1[:41], s_odo, s_odo, s_v0, b"junk", p1, s_odo + b"x", s_odo, b"QSRX" + s_odo[4:]]
    for d in seq:
        bot.sendto(d, ("127.0.0.1", port))
    time.sleep(0.05)
    t0 = 500.0
    assert mc.poll(now=t0) == len(seq)
    calls = mc.mapper.calls
    # maximal runs of one kind, in arrival order: a 752-byte datagram is oversize and joins the packet run
    assert [(c[0], c[1][0]) for c in calls] == [("pkt", 2), ("sweep", 2), ("sweep", 1), ("pkt", 3), ("sweep", 2)]
    assert [c[1][1] for c in calls] == [48, 751, 743, 48, 751]
    assert calls[3][2] == [4, 42, 65535]
    # no run names its sequence numbers: the mapper continues its own counter from what it held, 1 per packet, 46 per sweep
    assert all(c[3] is None for c in calls)
    assert [c[4] for c in calls] == [1000, 1002, 1002 + 92, 1002 + 92 + 46, 1002 + 92 + 46 + 3]
    assert mc.mapper.next_seq == 1002 + 92 + 46 + 3 + 92
    # accepted sweeps mark their bot online and set its pose
    assert mc.online == {1: True, 2: True} and mc.pkt_counts == {1: 4, 2: 3}
    assert mc.bot_pose[2] == (3.0, 4.0) and mc.bot_pose[1] == (-1.0, -2.0)
    assert mc.bot_addrs[2] == ("127.0.0.1", mc.bot_ports[2])
    # heartbeat: silence takes a sweep-only bot offline, its next sweep brings it back
    assert set(mc.heartbeat(now=t0 + 5.5)) == {1, 2}
    bot.sendto(s_odo, ("127.0.0.1", port))
    time.sleep(0.05)
    assert mc.poll(now=t0 + 6.0) == 1
    assert mc.online == {1: False, 2: True} and calls[-1][3] is None and calls[-1][4] == mc.mapper.next_seq - 46
    srv.close(); bot.close()


def test_mission_control_without_sweeps_drops_them():
    P = _P()
    fe = importlib.import_module(PKG_NAME + ".udp_frontend")
    srv, bot = _pair()
    port = srv.getsockname()[1]
    mc = fe.MissionControl(StubMapper(), sock=srv)
    r = np.full(181, 0.5, dtype=np.float32)
    for d in (P.pack_v0(1, 0.0, 0.0, 0.0, r), P.pack_v0_odo(2, 0.0, 0.0, 0.0, 0, 0, r)):
        bot.sendto(d, ("127.0.0.1", port))
    time.sleep(0.05)
    assert mc.poll(now=1.0) == 2
    (kind, shape, lens, seq0, _), = mc.mapper.calls
    assert kind == "pkt" and shape == (2, 48) and lens == [65535, 65535] and seq0 is None
    assert mc.online == {1: False, 2: False}
    srv.close(); bot.close()

