"""Host-side mirror of the reference mapper's object API over the HIP library.

`QuasarMapper` is the batched equivalent of dual_bot_mapper.py's main() recv loop
(:815-945): it owns one GPU context and exposes look-alikes of the objects the reference's
renderer and timers read -- `OccupancyGrid` (:110-237), `PoseGraphSLAM` (:261-338),
`drift_correction`, `zone_boxes`.  All arithmetic happens in the HIP kernels; this file only
marshals buffers (numpy <-> C ABI).
"""
import ctypes as C
import os
import struct
import types
import zlib

import numpy as np

from . import _lib
from ._lib import QsConfig, QsMergeResult, QsViewParams, QS_MERGE_STATUS, QuasarError, UINT64_MAX, check
from . import protocol as P


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dev_addr(a):
    """A device address: an int, or anything with data_ptr() (a torch tensor)."""
    return int(a.data_ptr()) if hasattr(a, "data_ptr") else int(a or 0)


# ---- checkpoint file header (include/quasar_slam.h: "checkpoint / restore") ------------------------------------------------
CKPT_MAGIC = b"QSCK"
CKPT_VERSION = 1
CKPT_HEADER_FIXED = 144
CKPT_SECTIONS = {1: "scalars", 2: "bots", 3: "counters", 4: "graphs", 5: "block_ids", 6: "blocks", 7: "dirty"}
_CKPT_HEAD = struct.Struct("<4sIIIQII")                  # magic, version, header_bytes, n_sections, total_bytes, crc32, reserved
_CKPT_INTS = ("size", "min_poses_between", "max_agent", "bots_per_graph", "enable_counts", "enable_ekf", "seq_stride",
              "shard_bots", "shard_rank", "exact_trig", "dirty_tracking")
_CKPT_F64 = ("res", "ox", "oy", "min_dist", "max_dist", "closure_radius", "closure_correction", "ekf_metres_per_tick")
_CKPT_CFG = struct.Struct("<12i8d")
_CKPT_SEC = struct.Struct("<IIQQ")


def checkpoint_config(data):
    """The header of a checkpoint (QuasarMapper.checkpoint / save) as a dict: the configuration it was taken with, the format
    version, the total length, the sections {name: (offset, length)} and the number of grid blocks.  Checks magic, version,
    lengths and the CRC-32 of the body (ValueError); needs no GPU."""
    mv = memoryview(data).cast("B")
    if len(mv) < CKPT_HEADER_FIXED:
        raise ValueError(f"checkpoint: truncated header ({len(mv)} bytes)")
    magic, version, hb, n_sec, total, crc, _ = _CKPT_HEAD.unpack_from(mv, 0)
    if magic != CKPT_MAGIC:
        raise ValueError("checkpoint: bad magic (not a checkpoint)")
    if version != CKPT_VERSION:
        raise ValueError(f"checkpoint: unknown format version {version} (this reader knows {CKPT_VERSION})")
    if n_sec not in (6, 7) or hb != CKPT_HEADER_FIXED + _CKPT_SEC.size * n_sec or len(mv) < hb:
        raise ValueError("checkpoint: bad header or section table")
    if total != len(mv):
        raise ValueError(f"checkpoint: length {len(mv)} does not match the header's {total} (truncated?)")
    if zlib.crc32(mv[hb:]) != crc:
        raise ValueError("checkpoint: CRC mismatch (corrupted checkpoint)")
    vals = _CKPT_CFG.unpack_from(mv, 32)
    out = dict(zip(_CKPT_INTS, vals[:11]))
    out.update(zip(_CKPT_F64, vals[12:]))
    for k in ("enable_counts", "enable_ekf", "exact_trig", "dirty_tracking"):
        out[k] = bool(out[k])
    sections = {}
    for i in range(n_sec):
        kind, _, off, length = _CKPT_SEC.unpack_from(mv, CKPT_HEADER_FIXED + _CKPT_SEC.size * i)
        if kind not in CKPT_SECTIONS or CKPT_SECTIONS[kind] in sections or off < hb or off % 8 or off + length > total:
            raise ValueError(f"checkpoint: bad section table entry {i}")
        sections[CKPT_SECTIONS[kind]] = (off, length)
    if "block_ids" not in sections:
        raise ValueError("checkpoint: no block list")
    out.update(version=version, total_bytes=total, sections=sections, n_blocks=sections["block_ids"][1] // 4)
    return out


class QuasarMapper:
    """One mapper instance on one GPU.  Defaults are the reference's constants."""

    def __init__(self, size=P.GRID_SIZE, resolution=P.GRID_RESOLUTION, origin_x=P.GRID_ORIGIN_X,
                 origin_y=P.GRID_ORIGIN_Y, separation=0.0, max_agent=2, bots_per_graph=0,
                 enable_counts=True, enable_ekf=False, device=0, raycast_mode=0,
                 ekf_metres_per_tick=0.0107, min_poses_between=P.MIN_POSES_BETWEEN,
                 closure_radius=P.CLOSURE_RADIUS, closure_correction=P.CLOSURE_CORRECTION,
                 seq_stride=1, shard_bots=0, shard_rank=0, exact_trig=True, min_dist=None, max_dist=None):
        self._L = _lib.load()
        cfg = QsConfig()
        check(None, self._L.qs_config_default(C.byref(cfg)), "qs_config_default")
        cfg.size, cfg.res, cfg.ox, cfg.oy = size, resolution, origin_x, origin_y
        cfg.separation = separation
        cfg.max_agent, cfg.bots_per_graph = max_agent, bots_per_graph
        cfg.enable_counts, cfg.enable_ekf = int(enable_counts), int(enable_ekf)
        cfg.device, cfg.raycast_mode = device, raycast_mode
        cfg.ekf_metres_per_tick = ekf_metres_per_tick
        cfg.min_poses_between = min_poses_between
        cfg.closure_radius, cfg.closure_correction = closure_radius, closure_correction
        cfg.seq_stride = seq_stride
        cfg.shard_bots, cfg.shard_rank = shard_bots, shard_rank
        cfg.exact_trig = int(bool(exact_trig))
        if min_dist is not None:
            cfg.min_dist = min_dist
        if max_dist is not None:
            cfg.max_dist = max_dist
        self.cfg = cfg
        self.size, self.res, self.ox, self.oy = size, resolution, origin_x, origin_y
        self.max_agent = max_agent
        h = C.c_void_p()
        rc = self._L.qs_create(C.byref(cfg), C.byref(h))      # validates every field
        if rc != 0:
            raise QuasarError(f"qs_create failed ({rc}): {self._L.qs_last_error(None).decode()}")
        self._h = h
        self.bots_per_graph = bots_per_graph if bots_per_graph > 0 else max_agent
        self.n_graphs = (max_agent + self.bots_per_graph - 1) // self.bots_per_graph
        self._last_n = 0
        self._bot_offset = {2: float(separation)} if max_agent >= 2 else {}
        self._map_version = 0          # bumped by everything that can change a cell: the look-alike's .grid cache key
        self.occ_grid = OccupancyGrid._attached(self)
        self.slam = PoseGraphSLAM._attached(self)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.qs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc, what):
        check(self._h, rc, what)

    def reset(self):
        self._chk(self._L.qs_reset(self._h), "qs_reset")
        self._map_version += 1

    def sync(self):
        self._chk(self._L.qs_sync(self._h), "qs_sync")

    # -- checkpoint / restore (include/quasar_slam.h) ------------------------------------------------------------------------
    def checkpoint(self) -> bytes:
        """The session state as bytes (qs_checkpoint): a fresh context restored from them answers every later call as this
        one would."""
        n = C.c_size_t()
        self._chk(self._L.qs_checkpoint(self._h, None, 0, C.byref(n)), "qs_checkpoint")
        buf = np.empty(n.value, dtype=np.uint8)
        self._chk(self._L.qs_checkpoint(self._h, _ptr(buf), n.value, C.byref(n)), "qs_checkpoint")
        return buf[:n.value].tobytes()

    def restore(self, data):
        """Load a checkpoint into this context (qs_restore; its configuration must match).  A refused restore leaves the
        context as it was."""
        a = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
        self._chk(self._L.qs_restore(self._h, _ptr(a), len(a)), "qs_restore")
        self._map_version += 1
        self._last_n = 0
        self._last_sweeps_n = 0

    def save(self, path):
        """checkpoint() written atomically: a temporary file beside `path`, fsync, then os.replace."""
        data = self.checkpoint()
        path = os.fspath(path)
        tmp = f"{path}.tmp-{os.getpid()}"
        try:
            with open(tmp, "wb") as f:
                f.write(data)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return len(data)

    @classmethod
    def load(cls, path, device=0, raycast_mode=0):
        """A mapper built from the configuration in the checkpoint's header, with the checkpoint restored into it."""
        with open(path, "rb") as f:
            data = f.read()
        k = checkpoint_config(data)
        m = cls(k["size"], k["res"], k["ox"], k["oy"], max_agent=k["max_agent"], bots_per_graph=k["bots_per_graph"],
                enable_counts=k["enable_counts"], enable_ekf=k["enable_ekf"], device=device, raycast_mode=raycast_mode,
                ekf_metres_per_tick=k["ekf_metres_per_tick"], min_poses_between=k["min_poses_between"],
                closure_radius=k["closure_radius"], closure_correction=k["closure_correction"], seq_stride=k["seq_stride"],
                shard_bots=k["shard_bots"], shard_rank=k["shard_rank"], exact_trig=k["exact_trig"],
                min_dist=k["min_dist"], max_dist=k["max_dist"])
        try:
            m.restore(data)
        except BaseException:
            m.close()
            raise
        return m

    def set_stream(self, hip_stream_ptr):
        self._chk(self._L.qs_set_stream(self._h, C.c_void_p(hip_stream_ptr)), "qs_set_stream")

    def set_bot_offset(self, bot, off_x):
        self._chk(self._L.qs_set_bot_offset(self._h, bot, off_x), "qs_set_bot_offset")
        self._bot_offset[int(bot)] = float(off_x)

    def sweep_pose_shift(self, bot):
        """(sx, sy): what a sweep ingest adds to the packet's x, y to form the pose it casts from -- the bot's offset (the
        separation for bot 2, or set_bot_offset through this object) plus its closure drift as it stands."""
        d = self.drift(bot)
        return self._bot_offset.get(int(bot), 0.0) + float(d[0]), float(d[1])

    # -- ingest: dual_bot_mapper.py:826-919 ---------------------------------------------------
    def ingest(self, datagrams, recv_time=None, seq0=None):
        """datagrams: list of bytes objects (any lengths), in arrival order."""
        if len(datagrams) == 0:
            return 0
        if all(len(d) == P.PACKET_SIZE for d in datagrams):
            buf = np.frombuffer(b"".join(datagrams), dtype=np.uint8).reshape(-1, P.PACKET_SIZE)
            return self.ingest_array(buf, None, recv_time, seq0)
        buf, lens = P.pack_datagrams(datagrams)
        return self.ingest_array(buf, lens, recv_time, seq0)

    def ingest_array(self, buf, lengths=None, recv_time=None, seq0=None):
        """buf: uint8 [n, stride] host array; lengths: uint16 [n] or None."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        if buf.ndim != 2:
            raise ValueError("buf must be [n, stride]")
        n, stride = buf.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        t = None if recv_time is None else np.ascontiguousarray(recv_time, dtype=np.float64)
        if lens is not None and len(lens) != n:
            raise ValueError("lengths must have one entry per record")
        if t is not None and len(t) != n:
            raise ValueError("recv_time must have one entry per record")
        self._chk(self._L.qs_ingest(self._h, _ptr(buf), n, stride, _ptr(lens), _ptr(t),
                                    UINT64_MAX if seq0 is None else int(seq0)), "qs_ingest")
        self._map_version += 1
        self._last_n = n
        return n

    def ingest_device(self, d_pkts, n, stride, d_lens=0, d_time=0, seq0=None):
        """Device-resident input (raw device addresses as ints): n records, record k at d_pkts + k * stride, stride >= 41.
        d_pkts may be any byte address (the decoder reads only the n * stride bytes given); d_lens (uint16 [n], 0 = every
        length is the stride) and d_time (float64 [n], 0 = none) must be aligned to their element size.  Asynchronous on the
        context's stream: the buffers must be written before the call (for that stream) and stay alive and unchanged until
        the work has run (sync(), or any call that waits for the stream)."""
        self._chk(self._L.qs_ingest_device(self._h, C.c_void_p(d_pkts), n, stride,
                                           C.c_void_p(d_lens) if d_lens else None,
                                           C.c_void_p(d_time) if d_time else None,
                                           UINT64_MAX if seq0 is None else int(seq0)), "qs_ingest_device")
        self._map_version += 1
        self._last_n = n

    def last_batch(self):
        """(accepted uint8 [n], pose float64 [n,3]) of the last ingest (rx, ry, ryaw; :850-857)."""
        n = self._last_n
        acc = np.zeros(n, dtype=np.uint8)
        pose = np.zeros((n, 3), dtype=np.float64)
        self._chk(self._L.qs_last_batch(self._h, _ptr(acc), _ptr(pose), n), "qs_last_batch")
        return acc, pose

    def last_hits(self):
        """(xy float64 [n,4,2], valid uint8 [n,4]) of the last ingest: point_clouds appends (:892)."""
        n = self._last_n
        xy = np.zeros((n, 4, 2), dtype=np.float64)
        valid = np.zeros((n, 4), dtype=np.uint8)
        self._chk(self._L.qs_last_hits(self._h, _ptr(xy), _ptr(valid), n), "qs_last_hits")
        return xy, valid

    # -- bot veil (include/quasar_slam.h, rules V1-V7 and S0-S8) -------------------------------------------------------------
    def set_bot_veil(self, radius=P.BOT_VEIL_RADIUS, sweeps=None):
        """Veil packet beams that end within `radius` cells (1..32) of the cell where another bot was last heard: they are cast
        free, without their end cell.  0 turns the veil off; the table of bot cells is kept either way.  sweeps: True / False
        sets the switch that extends the veil to sweep beams (sweeps then feed the table too); None leaves it as it is."""
        self._chk(self._L.qs_set_bot_veil(self._h, int(radius)), "qs_set_bot_veil")
        if sweeps is not None:
            self._chk(self._L.qs_set_bot_veil_sweeps(self._h, 1 if sweeps else 0), "qs_set_bot_veil_sweeps")

    def bot_veil_sweeps(self):
        """Is the sweep switch on?  (The sweep veil acts only while it is on and bot_veil() > 0.)"""
        on = C.c_int32()
        self._chk(self._L.qs_bot_veil_sweeps(self._h, C.byref(on)), "qs_bot_veil_sweeps")
        return bool(on.value)

    def last_sweeps_veiled(self):
        """uint8 [n, 181]: the beams of the last sweep ingest that the veil cast without their end cell (zeros unless the sweep
        veil was acting)."""
        n = getattr(self, "_last_sweeps_n", 0)
        v = np.zeros((n, P.SWEEP_BEAMS), dtype=np.uint8)
        self._chk(self._L.qs_last_sweeps_veiled(self._h, _ptr(v), n), "qs_last_sweeps_veiled")
        return v

    def bot_veil(self):
        """The veil's radius in cells; 0 = off."""
        r = C.c_int32()
        self._chk(self._L.qs_bot_veil(self._h, C.byref(r)), "qs_bot_veil")
        return r.value

    def bot_veil_place(self, bot, x, y):
        """cell[bot] from a world position: a sweep bot (sweep ingests feed the table only under the sweep switch), a charging dock
        given a spare id."""
        self._chk(self._L.qs_bot_veil_place(self._h, int(bot), float(x), float(y)), "qs_bot_veil_place")

    def bot_veil_forget(self, bot=None):
        """Forget where `bot` was last heard (None: every bot)."""
        self._chk(self._L.qs_bot_veil_forget(self._h, 0 if bot is None else int(bot)), "qs_bot_veil_forget")

    def bot_veil_cells(self):
        """(xy int32 [max_agent + 1, 2], known uint8 [max_agent + 1]): the cell where each bot was last heard; row 0 is unused."""
        xy = np.zeros((self.max_agent + 1, 2), dtype=np.int32)
        known = np.zeros(self.max_agent + 1, dtype=np.uint8)
        self._chk(self._L.qs_bot_veil_cells(self._h, _ptr(xy), _ptr(known)), "qs_bot_veil_cells")
        return xy, known

    def last_veiled(self):
        """uint8 [n, 4]: the rays of the last packet ingest that the veil cast without their end cell (zeros with the veil off)."""
        n = self._last_n
        v = np.zeros((n, 4), dtype=np.uint8)
        self._chk(self._L.qs_last_veiled(self._h, _ptr(v), n), "qs_last_veiled")
        return v

    def bot_veil_stats(self):
        """Rays veiled since the context was created or reset."""
        t = C.c_uint64()
        self._chk(self._L.qs_bot_veil_stats(self._h, C.byref(t)), "qs_bot_veil_stats")
        return t.value

    def bot_veil_time(self, reset=True):
        """(ms, launches) of the veil stage alone since the last reset of the figure; needs timing_enable()."""
        ms, k = C.c_double(), C.c_uint64()
        self._chk(self._L.qs_bot_veil_time(self._h, C.byref(ms), C.byref(k), int(reset)), "qs_bot_veil_time")
        return ms.value, k.value

    # -- servo sweeps (v0 '<4sBfffH181f' / v0 + odometry '<4sBfffiIH181f'; include/quasar_slam.h) --------------------------
    def ingest_sweeps(self, datagrams, lengths=None, seq0=None, match=None, check=None):
        """Map servo-sweep packets: a list of bytes objects (one format: 743 or 751 bytes; other lengths are dropped) or a
        uint8 [n, 743 | 751] array with optional uint16 lengths.  Sweep k uses sequence numbers seq0 + 46 k ... + 45.
        match: True (default parameters) or what match_params takes -- every sweep of the call is first matched against
        the map as it stands and mapped from its corrected pose (qs_ingest_sweeps_matched); last_sweep_matches() has the
        matches.  None or False: the plain ingest.
        check: True (default parameters) or what check_params takes -- every sweep of the call is first checked against the
        map as it stands and withheld from it when it contradicts it (qs_ingest_sweeps_checked); last_sweep_checks() has the
        checks.  Not together with match."""
        if match not in (None, False) and check not in (None, False):
            raise ValueError("ingest_sweeps: match and check cannot be combined")
        buf, lengths = self._sweep_buffer(datagrams, lengths)
        return self._sweeps_call(buf, lengths, seq0, match, check)

    @staticmethod
    def _sweep_buffer(datagrams, lengths):
        if isinstance(datagrams, np.ndarray):
            buf = np.ascontiguousarray(datagrams, dtype=np.uint8)
            if buf.ndim != 2:
                raise ValueError("sweeps must be [n, stride]")
            return buf, lengths
        if len(datagrams) == 0:
            return np.zeros((0, P.PACKET_SIZE_V0_ODO), np.uint8), None
        sizes = {len(d) for d in datagrams} & {P.PACKET_SIZE_V0, P.PACKET_SIZE_V0_ODO}
        if len(sizes) > 1:
            raise ValueError("one sweep format per call: 743- and 751-byte records mixed")
        stride = sizes.pop() if sizes else P.PACKET_SIZE_V0_ODO
        buf = np.zeros((len(datagrams), stride), dtype=np.uint8)
        lengths = np.zeros(len(datagrams), dtype=np.uint16)
        for i, d in enumerate(datagrams):
            m = min(len(d), stride)
            buf[i, :m] = np.frombuffer(d[:m], dtype=np.uint8)
            lengths[i] = min(len(d), 65535)
        return buf, lengths

    def _sweeps_call(self, buf, lengths, seq0, match=None, check=None):
        n, stride = buf.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        if lens is not None and len(lens) != n:
            raise ValueError("lengths must have one entry per record")
        seq = UINT64_MAX if seq0 is None else int(seq0)
        # (what the last ingest was changes only once the library has taken the call: a refused one leaves it)
        if check is not None and check is not False:
            prm = self.check_params(check)
            self._chk(self._L.qs_ingest_sweeps_checked(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens), seq),
                      "qs_ingest_sweeps_checked")
            self._last_matches_n, self._last_checks_n = None, n
        elif match is None or match is False:
            self._chk(self._L.qs_ingest_sweeps(self._h, _ptr(buf) if n else None, n, stride, _ptr(lens), seq), "qs_ingest_sweeps")
            self._last_matches_n, self._last_checks_n = None, None
        else:
            prm = self.match_params(match)
            self._chk(self._L.qs_ingest_sweeps_matched(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens), seq),
                      "qs_ingest_sweeps_matched")
            self._last_matches_n, self._last_checks_n = n, None
        self._map_version += 1
        self._last_n = 0
        self._last_sweeps_n = n
        return n

    def ingest_sweeps_device(self, d_pkts, n, stride, d_lens=0, seq0=None):
        """Device-resident sweeps (raw device addresses as ints); asynchronous."""
        self._chk(self._L.qs_ingest_sweeps_device(self._h, C.c_void_p(d_pkts), n, stride,
                                                  C.c_void_p(d_lens) if d_lens else None,
                                                  UINT64_MAX if seq0 is None else int(seq0)), "qs_ingest_sweeps_device")
        self._map_version += 1
        self._last_n = 0
        self._last_sweeps_n = n
        self._last_matches_n = None
        self._last_checks_n = None

    # -- sweeps in the pose graph (include/quasar_slam.h, "sweeps in the pose graph") ---------------------------------------------
    @staticmethod
    def sweep_graph_params(params=None, **kw):
        """A qs_sweep_graph_params from None / True (the defaults of protocol.SWEEP_GRAPH_*), a dict of its fields, or one
        already built."""
        if isinstance(params, _lib.QsSweepGraphParams):
            return params
        d = dict(half_width=P.SWEEP_GRAPH_HALF_WIDTH, close=P.SWEEP_GRAPH_CLOSE_M, open=P.SWEEP_GRAPH_OPEN_M)
        if isinstance(params, dict):
            d.update(params)
        elif params not in (None, True):
            raise TypeError("sweep graph parameters: None, True, a dict or a QsSweepGraphParams")
        d.update({k: v for k, v in kw.items() if v is not None})
        return _lib.QsSweepGraphParams(half_width=int(d["half_width"]), reserved=0, close=float(d["close"]), open=float(d["open"]))

    def set_sweep_graph(self, on=True, half_width=None, close=None, open=None):
        """Graph mode of the sweep ingests: every accepted sweep becomes a pose-graph node with a landmark signature derived
        from its ranges (the median of 2 * half_width + 1 beams to the right, front and left against the firmware's close /
        open thresholds), the loop-closure chain runs, the sweep is cast from the pose the chain gives it and feeds the bot's
        zone box.  Off by default; kept over reset(), not saved in a checkpoint."""
        prm = self.sweep_graph_params(None, half_width=half_width, close=close, open=open)
        self._chk(self._L.qs_set_sweep_graph(self._h, int(bool(on)), C.byref(prm)), "qs_set_sweep_graph")

    def sweep_graph(self):
        """(enabled, {"half_width", "close", "open"}) as the context holds them."""
        on, prm = C.c_int32(), _lib.QsSweepGraphParams()
        self._chk(self._L.qs_sweep_graph(self._h, C.byref(on), C.byref(prm)), "qs_sweep_graph")
        return bool(on.value), {"half_width": prm.half_width, "close": prm.close, "open": prm.open}

    def sweep_signatures(self, datagrams, lengths=None, params=None):
        """The landmark signature of every sweep (as ingest_sweeps takes them) by the graph-mode rule, uint8 [n]:
        protocol.LM_* or SWEEP_LM_REJECTED for a record that is not accepted.  Writes nothing to the mapper.  params: None
        (the mapper's current parameters) or what sweep_graph_params takes."""
        buf, lengths = self._sweep_buffer(datagrams, lengths)
        n, stride = buf.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        if lens is not None and len(lens) != n:
            raise ValueError("lengths must have one entry per record")
        prm = None if params is None else C.byref(self.sweep_graph_params(params))
        out = np.zeros(n, dtype=np.uint8)
        self._chk(self._L.qs_sweep_signatures(self._h, prm, _ptr(buf) if n else None, n, stride, _ptr(lens),
                                              _ptr(out) if n else None), "qs_sweep_signatures")
        return out

    def sweep_signatures_device(self, d_pkts, n, stride, d_out, d_lens=0, params=None):
        """Device-resident form (raw device addresses as ints; d_out: n bytes); asynchronous."""
        prm = None if params is None else C.byref(self.sweep_graph_params(params))
        self._chk(self._L.qs_sweep_signatures_device(self._h, prm, C.c_void_p(d_pkts), n, stride,
                                                     C.c_void_p(d_lens) if d_lens else None, C.c_void_p(d_out)),
                  "qs_sweep_signatures_device")

    def last_sweep_nodes(self):
        """(node int64 [n], lm uint8 [n]) of the last sweep ingest in graph mode: the node index of each sweep in its bot's
        pose graph (-1: rejected) and its signature (SWEEP_LM_REJECTED: rejected); an error after any other ingest."""
        n = getattr(self, "_last_sweeps_n", 0)
        node = np.zeros(n, dtype=np.int64)
        lm = np.zeros(n, dtype=np.uint8)
        self._chk(self._L.qs_last_sweep_nodes(self._h, _ptr(node) if n else None, _ptr(lm) if n else None, n), "qs_last_sweep_nodes")
        return node, lm

    # -- sweep matching (include/quasar_slam.h, "sweep matching") -----------------------------------------------------------
    @staticmethod
    def match_params(params=None, **kw):
        """A qs_match_params from None / True (the defaults of protocol.MATCH_*), a dict of its fields, or one already built."""
        if isinstance(params, _lib.QsMatchParams):
            return params
        d = dict(radius=P.MATCH_RADIUS, window=P.MATCH_WINDOW, angle_steps=P.MATCH_ANGLE_STEPS, min_hits=P.MATCH_MIN_HITS,
                 min_percent=P.MATCH_MIN_PERCENT, angle_step=P.MATCH_ANGLE_STEP)
        if isinstance(params, dict):
            d.update(params)
        elif params not in (None, True):
            raise TypeError("match parameters: None, True, a dict or a QsMatchParams")
        d.update(kw)
        return _lib.QsMatchParams(radius=int(d["radius"]), window=int(d["window"]), angle_steps=int(d["angle_steps"]),
                                  min_hits=int(d["min_hits"]), min_percent=int(d["min_percent"]), reserved=0,
                                  angle_step=float(d["angle_step"]))

    def match_field(self, radius=P.MATCH_RADIUS):
        """The likelihood field of the whole grid, uint8 [size, size]: max(0, radius + 1 - Chebyshev distance to the nearest
        occupied cell)."""
        out = np.empty((self.size, self.size), dtype=np.uint8)
        self._chk(self._L.qs_match_field(self._h, int(radius), _ptr(out)), "qs_match_field")
        return out

    def match_sweeps(self, datagrams, lengths=None, params=None, rotations=False):
        """Match sweeps (as ingest_sweeps takes them) against the map without mapping them or changing anything: a structured
        array of protocol.MATCH_DTYPE, one entry per record; with rotations also the (sin, cos) the device used, float64
        [n, 2 * angle_steps + 1, 2]."""
        buf, lengths = self._sweep_buffer(datagrams, lengths)
        n, stride = buf.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        if lens is not None and len(lens) != n:
            raise ValueError("lengths must have one entry per record")
        prm = self.match_params(params)
        out = np.zeros(n, dtype=P.MATCH_DTYPE)
        rot = np.zeros((n, 2 * prm.angle_steps + 1, 2), dtype=np.float64) if rotations else None
        self._chk(self._L.qs_match_sweeps(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens),
                                          _ptr(out) if n else None, _ptr(rot) if rotations and n else None), "qs_match_sweeps")
        return (out, rot) if rotations else out

    def match_sweeps_device(self, d_pkts, n, stride, d_out, d_lens=0, d_rot=0, params=None):
        """Device-resident match (raw device addresses as ints; d_out: n records of protocol.MATCH_DTYPE); asynchronous."""
        prm = self.match_params(params)
        self._chk(self._L.qs_match_sweeps_device(self._h, C.byref(prm), C.c_void_p(d_pkts), n, stride,
                                                 C.c_void_p(d_lens) if d_lens else None, C.c_void_p(d_out),
                                                 C.c_void_p(d_rot) if d_rot else None), "qs_match_sweeps_device")

    def ingest_sweeps_matched_device(self, d_pkts, n, stride, d_lens=0, seq0=None, params=None):
        """Device-resident matched ingest (raw device addresses as ints); asynchronous."""
        prm = self.match_params(params)
        self._chk(self._L.qs_ingest_sweeps_matched_device(self._h, C.byref(prm), C.c_void_p(d_pkts), n, stride,
                                                          C.c_void_p(d_lens) if d_lens else None,
                                                          UINT64_MAX if seq0 is None else int(seq0)),
                  "qs_ingest_sweeps_matched_device")
        self._map_version += 1
        self._last_n = 0
        self._last_sweeps_n = n
        self._last_matches_n = n
        self._last_checks_n = None

    def last_sweep_matches(self):
        """The matches of the last matched sweep ingest (protocol.MATCH_DTYPE [n]); an error after any other ingest."""
        n = getattr(self, "_last_matches_n", None)
        out = np.zeros(n or 0, dtype=P.MATCH_DTYPE)
        self._chk(self._L.qs_last_sweep_matches(self._h, _ptr(out) if n else None, n or 0), "qs_last_sweep_matches")
        return out

    # -- sweep check (include/quasar_slam.h, "sweep check") -------------------------------------------------------------------
    def check_params(self, params=None, **kw):
        """A qs_check_params from None / True (the defaults of protocol.CHECK_*; tol = CHECK_TOL_CELLS cells of this grid), a dict
        of its fields, or one already built."""
        if isinstance(params, _lib.QsCheckParams):
            return params
        d = dict(tol=P.CHECK_TOL_CELLS * self.res, min_checked=P.CHECK_MIN_CHECKED, max_bad_percent=P.CHECK_MAX_BAD_PERCENT,
                 count_missed=P.CHECK_COUNT_MISSED)
        if isinstance(params, dict):
            d.update(params)
        elif params not in (None, True):
            raise TypeError("check parameters: None, True, a dict or a QsCheckParams")
        d.update(kw)
        return _lib.QsCheckParams(tol=float(d["tol"]), min_checked=int(d["min_checked"]), max_bad_percent=int(d["max_bad_percent"]),
                                  count_missed=int(d["count_missed"]), reserved=int(d.get("reserved", 0)))

    def check_sweeps(self, datagrams, lengths=None, params=None, classes=False):
        """Check sweeps (as ingest_sweeps takes them) against the map without mapping them or changing anything: a structured
        array of protocol.CHECK_DTYPE, one entry per record; with classes also every beam's class, uint8 [n, 181]
        (protocol.BEAM_*; BEAM_NO_RECORD throughout for a record that is not accepted)."""
        buf, lengths = self._sweep_buffer(datagrams, lengths)
        n, stride = buf.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        if lens is not None and len(lens) != n:
            raise ValueError("lengths must have one entry per record")
        prm = self.check_params(params)
        out = np.zeros(n, dtype=P.CHECK_DTYPE)
        cls = np.zeros((n, P.SWEEP_BEAMS), dtype=np.uint8) if classes else None
        self._chk(self._L.qs_check_sweeps(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens),
                                          _ptr(out) if n else None, _ptr(cls) if classes and n else None), "qs_check_sweeps")
        return (out, cls) if classes else out

    def check_sweeps_device(self, d_pkts, n, stride, d_out, d_lens=0, d_cls=0, params=None):
        """Device-resident check (raw device addresses as ints; d_out: n records of protocol.CHECK_DTYPE, d_cls: n x 181
        bytes); asynchronous."""
        prm = self.check_params(params)
        self._chk(self._L.qs_check_sweeps_device(self._h, C.byref(prm), C.c_void_p(d_pkts), n, stride,
                                                 C.c_void_p(d_lens) if d_lens else None, C.c_void_p(d_out),
                                                 C.c_void_p(d_cls) if d_cls else None), "qs_check_sweeps_device")

    def ingest_sweeps_checked_device(self, d_pkts, n, stride, d_lens=0, seq0=None, params=None):
        """Device-resident guarded ingest (raw device addresses as ints); asynchronous."""
        prm = self.check_params(params)
        self._chk(self._L.qs_ingest_sweeps_checked_device(self._h, C.byref(prm), C.c_void_p(d_pkts), n, stride,
                                                          C.c_void_p(d_lens) if d_lens else None,
                                                          UINT64_MAX if seq0 is None else int(seq0)),
                  "qs_ingest_sweeps_checked_device")
        self._map_version += 1
        self._last_n = 0
        self._last_sweeps_n = n
        self._last_matches_n = None
        self._last_checks_n = n

    def last_sweep_checks(self):
        """The checks of the last guarded sweep ingest (protocol.CHECK_DTYPE [n]); an error after any other ingest."""
        n = getattr(self, "_last_checks_n", None)
        out = np.zeros(n or 0, dtype=P.CHECK_DTYPE)
        self._chk(self._L.qs_last_sweep_checks(self._h, _ptr(out) if n else None, n or 0), "qs_last_sweep_checks")
        return out

    # -- relocalisation (include/quasar_slam.h, "relocalisation") -------------------------------------------------------------
    @staticmethod
    def relocalise_params(params=None, **kw):
        """A qs_reloc_params from None / True (the defaults of protocol.RELOC_*), a dict of its fields, or one already built.
        box = (x0, y0, x1, y1) searches the cells [x0, x1) x [y0, y1) only (clipped to the grid); None: the whole grid."""
        if isinstance(params, _lib.QsRelocParams):
            return params
        d = dict(radius=P.RELOC_RADIUS, n_rot=P.RELOC_N_ROT, sep=P.RELOC_SEP, sep_rot=P.RELOC_SEP_ROT, min_hits=P.RELOC_MIN_HITS,
                 min_percent=P.RELOC_MIN_PERCENT, min_margin=P.RELOC_MIN_MARGIN, box=None)
        if isinstance(params, dict):
            d.update(params)
        elif params not in (None, True):
            raise TypeError("relocalisation parameters: None, True, a dict or a QsRelocParams")
        d.update(kw)
        box = d.pop("box")
        x0, y0, x1, y1 = (int(v) for v in box) if box is not None else (0, 0, 0, 0)
        return _lib.QsRelocParams(use_box=int(box is not None), x0=x0, y0=y0, x1=x1, y1=y1, **{k: int(v) for k, v in d.items()})

    def relocalise_sweeps(self, datagrams, lengths=None, params=None):
        """Locate sweeps (as ingest_sweeps takes them) against the whole map, whatever pose they carry: a structured array of
        protocol.RELOC_DTYPE, one entry per record -- the best pose, the best rival away from it, and whether the gate on
        hits, score and margin accepts.  Reads the map, changes nothing."""
        buf, lengths = self._sweep_buffer(datagrams, lengths)
        n, stride = buf.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        if lens is not None and len(lens) != n:
            raise ValueError("lengths must have one entry per record")
        prm = self.relocalise_params(params)
        out = np.zeros(n, dtype=P.RELOC_DTYPE)
        self._chk(self._L.qs_relocalise_sweeps(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens),
                                               _ptr(out) if n else None), "qs_relocalise_sweeps")
        return out

    def relocalise_sweeps_device(self, d_pkts, n, stride, d_out, d_lens=0, params=None):
        """Device-resident form (raw device addresses as ints; d_out: n records of protocol.RELOC_DTYPE); asynchronous."""
        prm = self.relocalise_params(params)
        self._chk(self._L.qs_relocalise_sweeps_device(self._h, C.byref(prm), C.c_void_p(d_pkts), n, stride,
                                                      C.c_void_p(d_lens) if d_lens else None, C.c_void_p(d_out)),
                  "qs_relocalise_sweeps_device")

    def relocalise_groups(self, datagrams, gsize, lengths=None, rel=None, travel=P.RELOC_TRAVEL, params=None):
        """Locate groups of sweeps against the whole map, the sweeps of a group scored jointly (include/quasar_slam.h,
        "relocalisation of a group"): records [sum(gsize)] in runs of gsize[g], a structured array of protocol.GROUP_RELOC_DTYPE,
        one entry per group -- the pose of the group's frame.  rel (protocol.RELOC_REL_DTYPE, one per record): each record's pose
        in its group's frame; None: from the packets' poses, the first record of each group the frame (protocol.reloc_rel).
        Reads the map, changes nothing."""
        buf, lengths = self._sweep_buffer(datagrams, lengths)
        n, stride = buf.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        if lens is not None and len(lens) != n:
            raise ValueError("lengths must have one entry per record")
        gs = np.ascontiguousarray(gsize, dtype=np.int32).reshape(-1)
        if rel is None:
            if (gs < 0).any() or int(gs.sum()) != n:
                raise ValueError("the group sizes must sum to the number of records")
            pose = buf[:, 5:17].copy().view("<f4") if n else np.zeros((0, 3), np.float32)
            ends = np.cumsum(gs)
            rel = np.concatenate([P.reloc_rel(*pose[e - g:e].T) for g, e in zip(gs.tolist(), ends.tolist())]
                                 + [np.zeros(0, dtype=P.RELOC_REL_DTYPE)])
        rel = np.ascontiguousarray(rel, dtype=P.RELOC_REL_DTYPE).reshape(-1)
        if len(rel) != n:
            raise ValueError("rel must have one entry per record")
        prm = self.relocalise_params(params)
        out = np.zeros(len(gs), dtype=P.GROUP_RELOC_DTYPE)
        self._chk(self._L.qs_relocalise_groups(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens),
                                               _ptr(rel) if n else None, _ptr(gs) if len(gs) else None, len(gs), float(travel),
                                               _ptr(out) if len(gs) else None), "qs_relocalise_groups")
        return out

    def relocalise_groups_device(self, d_pkts, n, stride, d_rel, gsize, d_out, d_lens=0, travel=P.RELOC_TRAVEL, params=None):
        """Device-resident form (raw device addresses as ints; d_rel: n records of protocol.RELOC_REL_DTYPE, d_out: len(gsize)
        records of protocol.GROUP_RELOC_DTYPE; gsize a host array); asynchronous."""
        prm = self.relocalise_params(params)
        gs = np.ascontiguousarray(gsize, dtype=np.int32).reshape(-1)
        self._chk(self._L.qs_relocalise_groups_device(self._h, C.byref(prm), C.c_void_p(d_pkts), n, stride,
                                                      C.c_void_p(d_lens) if d_lens else None, C.c_void_p(d_rel),
                                                      _ptr(gs) if len(gs) else None, len(gs), float(travel), C.c_void_p(d_out)),
                  "qs_relocalise_groups_device")

    # -- trail matching (include/quasar_slam.h, "trail matching") ---------------------------------------------------------------
    @staticmethod
    def _trail_buffer(datagrams, lengths):
        """(uint8 [n, stride], uint16 lengths or None) of the packets of a trail call: an array as it is, datagrams packed."""
        if isinstance(datagrams, np.ndarray):
            buf = np.ascontiguousarray(datagrams, dtype=np.uint8)
            if buf.ndim != 2:
                raise ValueError("packets must be [n, stride]")
        elif len(datagrams) == 0:
            buf = np.zeros((0, P.PACKET_SIZE), np.uint8)
        elif all(len(d) == P.PACKET_SIZE for d in datagrams):
            buf = np.frombuffer(b"".join(datagrams), dtype=np.uint8).reshape(-1, P.PACKET_SIZE)
        else:
            buf, lengths = P.pack_datagrams(datagrams)
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint16)
        if lens is not None and len(lens) != len(buf):
            raise ValueError("lengths must have one entry per record")
        return buf, lens

    def match_trails(self, datagrams, gsize, lengths=None, travel=P.TRAIL_TRAVEL, params=None, rotations=False):
        """Match trails of 42-byte packets against the map without mapping them or changing anything: packets (as ingest /
        ingest_array take them) in runs of gsize[g], each run the last packets of one bot in arrival order; a structured array
        of protocol.TRAIL_MATCH_DTYPE, one entry per trail (protocol.trail_move applies one).  params: what match_params
        takes.  With rotations also the (sin, cos) of each record's yaw as the device formed them, float64 [n, 2]."""
        buf, lens = self._trail_buffer(datagrams, lengths)
        n, stride = buf.shape
        gs = np.ascontiguousarray(gsize, dtype=np.int32).reshape(-1)
        prm = self.match_params(params)
        out = np.zeros(len(gs), dtype=P.TRAIL_MATCH_DTYPE)
        rot = np.zeros((n, 2), dtype=np.float64) if rotations else None
        self._chk(self._L.qs_match_trails(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens),
                                          _ptr(gs) if len(gs) else None, len(gs), float(travel), _ptr(out) if len(gs) else None,
                                          _ptr(rot) if rotations and n else None), "qs_match_trails")
        return (out, rot) if rotations else out

    def match_trails_device(self, d_pkts, n, stride, gsize, d_out, d_lens=0, d_rot=0, travel=P.TRAIL_TRAVEL, params=None):
        """Device-resident form (raw device addresses as ints; d_out: len(gsize) records of protocol.TRAIL_MATCH_DTYPE, d_rot:
        float64 [n, 2] or 0; gsize a host array); asynchronous."""
        prm = self.match_params(params)
        gs = np.ascontiguousarray(gsize, dtype=np.int32).reshape(-1)
        self._chk(self._L.qs_match_trails_device(self._h, C.byref(prm), C.c_void_p(d_pkts) if d_pkts else None, n, stride,
                                                 C.c_void_p(d_lens) if d_lens else None, _ptr(gs) if len(gs) else None, len(gs),
                                                 float(travel), C.c_void_p(d_out) if d_out else None,
                                                 C.c_void_p(d_rot) if d_rot else None), "qs_match_trails_device")

    # -- trail relocalisation (include/quasar_slam.h, "trail relocalisation") -----------------------------------------------------
    def relocalise_trails(self, datagrams, gsize, lengths=None, travel=P.TRAIL_TRAVEL, params=None, rotations=False):
        """Locate trails of 42-byte packets against the whole map, whatever frame their poses are in: packets (as match_trails
        takes them) in runs of gsize[g]; a structured array of protocol.TRAIL_RELOC_DTYPE, one entry per trail
        (protocol.trail_reloc_move applies one).  params: what relocalise_params takes.  With rotations also the (sin, cos)
        of each counting record's yaw as the device formed them, float64 [n, 2].  Reads the map, changes nothing."""
        buf, lens = self._trail_buffer(datagrams, lengths)
        n, stride = buf.shape
        gs = np.ascontiguousarray(gsize, dtype=np.int32).reshape(-1)
        prm = self.relocalise_params(params)
        out = np.zeros(len(gs), dtype=P.TRAIL_RELOC_DTYPE)
        rot = np.zeros((n, 2), dtype=np.float64) if rotations else None
        self._chk(self._L.qs_relocalise_trails(self._h, C.byref(prm), _ptr(buf) if n else None, n, stride, _ptr(lens),
                                               _ptr(gs) if len(gs) else None, len(gs), float(travel),
                                               _ptr(out) if len(gs) else None, _ptr(rot) if rotations and n else None),
                  "qs_relocalise_trails")
        return (out, rot) if rotations else out

    def relocalise_trails_device(self, d_pkts, n, stride, gsize, d_out, d_lens=0, d_rot=0, travel=P.TRAIL_TRAVEL, params=None):
        """Device-resident form (raw device addresses as ints; d_out: len(gsize) records of protocol.TRAIL_RELOC_DTYPE, d_rot:
        float64 [n, 2] or 0; gsize a host array); asynchronous."""
        prm = self.relocalise_params(params)
        gs = np.ascontiguousarray(gsize, dtype=np.int32).reshape(-1)
        self._chk(self._L.qs_relocalise_trails_device(self._h, C.byref(prm), C.c_void_p(d_pkts) if d_pkts else None, n, stride,
                                                      C.c_void_p(d_lens) if d_lens else None, _ptr(gs) if len(gs) else None,
                                                      len(gs), float(travel), C.c_void_p(d_out) if d_out else None,
                                                      C.c_void_p(d_rot) if d_rot else None), "qs_relocalise_trails_device")

    def last_sweeps(self):
        """(accepted uint8 [n], pose float64 [n, 3]) of the last sweep ingest: the pose each sweep was cast from (rx, ry after
        offset and drift, yaw); NaN for rejected records."""
        n = getattr(self, "_last_sweeps_n", 0)
        acc = np.zeros(n, dtype=np.uint8)
        pose = np.zeros((n, 3), dtype=np.float64)
        self._chk(self._L.qs_last_sweeps(self._h, _ptr(acc), _ptr(pose), n), "qs_last_sweeps")
        return acc, pose

    def set_sweep_filter(self, smin=P.SWEEP_MIN_DIST_M, smax=P.SWEEP_MAX_DIST_M):
        """Trust filter of sweep beams: a hit when smin < d <= smax (default: the reference's 0.1 < d <= 1.2)."""
        self._chk(self._L.qs_set_sweep_filter(self._h, float(smin), float(smax)), "qs_set_sweep_filter")

    # -- sensing a world (include/quasar_slam.h, "sensing a world") -----------------------------------------------------------
    @staticmethod
    def sense_params(max_range=P.MAX_DIST_M, noise_amp=0.0, dropout=0.0, seed=0, first_record=0, no_return=0.0):
        """A qs_sense_params: max_range and noise_amp in metres, dropout the share of hit beams that report no return (kept as
        round(dropout * 65536) / 65536), seed and first_record the noise's stream, no_return what a beam without a hit reports."""
        p = _lib.QsSenseParams()
        p.max_range, p.noise_amp, p.no_return = float(max_range), float(noise_amp), float(no_return)
        q = dropout * 65536.0
        p.dropout_q16 = int(round(q)) if 0.0 <= q <= 65536.0 else 0xFFFFFFFF          # (the library refuses the rest)
        p.seed, p.first_record = int(seed) & UINT64_MAX, int(first_record) & UINT64_MAX
        return p

    @staticmethod
    def _sense_poses(pose_xyyaw):
        pose = np.ascontiguousarray(pose_xyyaw, dtype=np.float32)
        if pose.ndim != 2 or pose.shape[1] != 3:
            raise ValueError("poses must be [n, 3]: x, y, yaw")
        return pose

    @staticmethod
    def _sense_field(v, n, dtype, name):
        if v is None:
            return None
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (n,)))
        if a.shape != (n,):
            raise ValueError(f"{name} must have one entry per pose")
        return a

    def sense_ranges(self, pose_xyyaw, beams=P.SWEEP_BEAMS, return_cells=False, **params):
        """What each beam returns from each pose in this context's map -> float32 [n, beams] (beams: 181, a sweep, or 4, a
        packet's sensors); with return_cells also int32 [n, beams], the hit cell gy * size + gx or -1.  Poses are world poses
        float32 [n, 3]; keywords as sense_params.  Reads the map, writes nothing."""
        pose = self._sense_poses(pose_xyyaw)
        n = len(pose)
        prm = self.sense_params(**params)
        ranges = np.empty((n, int(beams)), dtype=np.float32)
        cells = np.empty((n, int(beams)), dtype=np.int32) if return_cells else None
        self._chk(self._L.qs_sense_ranges(self._h, _ptr(pose), n, int(beams), C.byref(prm), _ptr(ranges), _ptr(cells)), "qs_sense_ranges")
        return (ranges, cells) if return_cells else ranges

    def sense_ranges_device(self, d_pose, n, d_ranges, beams=P.SWEEP_BEAMS, d_cells=0, **params):
        """sense_ranges with device-resident float32 poses and outputs (addresses or torch tensors); asynchronous."""
        prm = self.sense_params(**params)
        cells = _dev_addr(d_cells)
        self._chk(self._L.qs_sense_ranges_device(self._h, C.c_void_p(_dev_addr(d_pose)), n, int(beams), C.byref(prm),
                                                 C.c_void_p(_dev_addr(d_ranges)), C.c_void_p(cells) if cells else None),
                  "qs_sense_ranges_device")

    def sense_sweeps(self, pose_xyyaw, agent, enc=None, v2v=None, odometry=True, **params):
        """The sweep packets bots at these poses would send -> uint8 [n, 751] (odometry) or [n, 743]: exactly
        protocol.pack_sweeps of the same fields with the ranges of sense_ranges."""
        pose = self._sense_poses(pose_xyyaw)
        n = len(pose)
        stride = P.PACKET_SIZE_V0_ODO if odometry else P.PACKET_SIZE_V0
        prm = self.sense_params(**params)
        out = np.empty((n, stride), dtype=np.uint8)
        self._chk(self._L.qs_sense_sweeps(self._h, _ptr(pose), _ptr(self._sense_field(agent, n, np.uint8, "agent")),
                                          _ptr(self._sense_field(enc, n, np.int32, "enc")), _ptr(self._sense_field(v2v, n, np.uint32, "v2v")),
                                          n, C.byref(prm), _ptr(out), stride), "qs_sense_sweeps")
        return out

    def sense_sweeps_device(self, d_pose, d_agent, n, d_out, stride=P.PACKET_SIZE_V0_ODO, d_enc=0, d_v2v=0, **params):
        """sense_sweeps with device-resident inputs and output (d_out: n * stride bytes at any address); asynchronous on the
        context's stream.  What it writes is what ingest_sweeps_device of another context reads."""
        prm = self.sense_params(**params)
        opt = lambda a: C.c_void_p(_dev_addr(a)) if _dev_addr(a) else None
        self._chk(self._L.qs_sense_sweeps_device(self._h, C.c_void_p(_dev_addr(d_pose)), C.c_void_p(_dev_addr(d_agent)), opt(d_enc),
                                                 opt(d_v2v), n, C.byref(prm), C.c_void_p(_dev_addr(d_out)), int(stride)),
                  "qs_sense_sweeps_device")

    def sense_packets(self, pose_xyyaw, agent, enc=None, v2v=None, landmark=None, **params):
        """The 42-byte packets bots at these poses would send -> uint8 [n, 42]: exactly protocol.pack_packets of the same fields
        with the four ranges of sense_ranges(beams=4)."""
        pose = self._sense_poses(pose_xyyaw)
        n = len(pose)
        prm = self.sense_params(**params)
        out = np.empty((n, P.PACKET_SIZE), dtype=np.uint8)
        self._chk(self._L.qs_sense_packets(self._h, _ptr(pose), _ptr(self._sense_field(agent, n, np.uint8, "agent")),
                                           _ptr(self._sense_field(enc, n, np.int32, "enc")), _ptr(self._sense_field(v2v, n, np.uint32, "v2v")),
                                           _ptr(self._sense_field(landmark, n, np.uint8, "landmark")), n, C.byref(prm), _ptr(out)),
                  "qs_sense_packets")
        return out

    def sense_packets_device(self, d_pose, d_agent, n, d_out, d_enc=0, d_v2v=0, d_landmark=0, **params):
        """sense_packets with device-resident inputs and output (n * 42 bytes); asynchronous on the context's stream."""
        prm = self.sense_params(**params)
        opt = lambda a: C.c_void_p(_dev_addr(a)) if _dev_addr(a) else None
        self._chk(self._L.qs_sense_packets_device(self._h, C.c_void_p(_dev_addr(d_pose)), C.c_void_p(_dev_addr(d_agent)), opt(d_enc),
                                                  opt(d_v2v), opt(d_landmark), n, C.byref(prm), C.c_void_p(_dev_addr(d_out))),
                  "qs_sense_packets_device")

    # -- grid ---------------------------------------------------------------------------------
    def grid_i8(self):
        out = np.empty((self.size, self.size), dtype=np.int8)
        self._chk(self._L.qs_grid_i8(self._h, _ptr(out)), "qs_grid_i8")
        return out

    def grid_i8_device(self, d_out):
        self._chk(self._L.qs_grid_i8_device(self._h, C.c_void_p(d_out)), "qs_grid_i8_device")

    # -- map view: MapRenderer, dual_bot_mapper.py:380-668, rendered on the device (include/quasar_slam.h) ----------------
    def render_view(self, width=P.VIEW_WIDTH, height=P.VIEW_HEIGHT, scale=P.VIEW_SCALE, offset_x=None, offset_y=None,
                    zones=None, prims=None, line_min=P.VIEW_LINE_MIN, line_max=P.VIEW_LINE_MAX, bg=P.BG_COLOR,
                    line=P.GRID_COLOR, free=P.CELL_COLOR_FREE, occ=P.CELL_COLOR_OCCUPIED, draw_occupied=False, minify=True,
                    d_out=None):
        """One frame of the map -> uint8 [height, width, 4] (R, G, B, 255; row 0 at the top).  The defaults are the
        reference's view (:383-397): offsets default to width / 2 and height / 2.  zones: P.VIEW_ZONE_DTYPE records (or None),
        prims: P.VIEW_PRIM_DTYPE records (or None), drawn in array order; MapView.lists builds both in the reference's draw
        order.  minify=False gives the reference's behaviour below 2 pixels per cell: no occupancy at all.  With d_out (a
        device address or a torch uint8 tensor of height * width * 4 bytes on this GPU) the frame stays on the device and
        None is returned.  Reads the map, writes nothing."""
        vp = QsViewParams()
        vp.width, vp.height, vp.scale = int(width), int(height), float(scale)
        vp.offset_x = float(width / 2 if offset_x is None else offset_x)
        vp.offset_y = float(height / 2 if offset_y is None else offset_y)
        vp.line_min, vp.line_max = int(line_min), int(line_max)
        for name, c in (("bg", bg), ("line", line), ("free", free), ("occ", occ)):
            getattr(vp, name)[:3] = [int(v) for v in c[:3]]
        vp.draw_occupied, vp.minify = int(bool(draw_occupied)), int(bool(minify))
        z = np.ascontiguousarray(zones if zones is not None else [], dtype=P.VIEW_ZONE_DTYPE).reshape(-1)
        q = np.ascontiguousarray(prims if prims is not None else [], dtype=P.VIEW_PRIM_DTYPE).reshape(-1)
        zp, qp = (_ptr(z) if len(z) else None), (_ptr(q) if len(q) else None)
        if d_out is not None:
            self._chk(self._L.qs_render_view_device(self._h, C.byref(vp), zp, len(z), qp, len(q), C.c_void_p(_dev_addr(d_out))),
                      "qs_render_view_device")
            return None
        ok = 1 <= vp.width <= 8192 and 1 <= vp.height <= 8192          # (the library refuses the rest; no buffer for it)
        out = np.empty((vp.height, vp.width, 4) if ok else (1, 1, 4), dtype=np.uint8)
        self._chk(self._L.qs_render_view(self._h, C.byref(vp), zp, len(z), qp, len(q), _ptr(out)), "qs_render_view")
        return out

    def counts(self):
        hits = np.empty((self.size, self.size), dtype=np.int32)
        misses = np.empty((self.size, self.size), dtype=np.int32)
        self._chk(self._L.qs_grid_counts(self._h, _ptr(hits), _ptr(misses)), "qs_grid_counts")
        return hits, misses

    def logodds(self, l_occ=0.85, l_free=0.4, lmin=-2.0, lmax=3.5):
        out = np.empty((self.size, self.size), dtype=np.float32)
        self._chk(self._L.qs_grid_logodds(self._h, l_occ, l_free, lmin, lmax, _ptr(out)), "qs_grid_logodds")
        return out

    def update_rays(self, rx, ry, hx, hy, valid, seq0=None):
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (rx, ry, hx, hy)]
        v = np.ascontiguousarray(valid, dtype=np.uint8)
        self._chk(self._L.qs_update_rays(self._h, *[_ptr(x) for x in a], _ptr(v), len(v),
                                         UINT64_MAX if seq0 is None else int(seq0)), "qs_update_rays")
        self._map_version += 1

    def world_to_grid(self, w, axis=0):
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.empty(len(w), dtype=np.int64)
        self._chk(self._L.qs_world_to_grid(self._h, _ptr(w), len(w), axis, _ptr(out)), "qs_world_to_grid")
        return out

    def device_buffers(self):
        """(stamps_ptr, stamps_bytes, counts_ptr, counts_bytes) raw device addresses.  Whoever gets them may write the
        grid (a collective): the look-alike's cached .grid is dropped."""
        self._map_version += 1
        sp, cp = C.c_void_p(), C.c_void_p()
        sb, cb = C.c_size_t(), C.c_size_t()
        self._chk(self._L.qs_device_buffers(self._h, C.byref(sp), C.byref(sb), C.byref(cp), C.byref(cb)),
                  "qs_device_buffers")
        return sp.value, sb.value, cp.value or 0, cb.value

    # -- SLAM -----------------------------------------------------------------------------------
    def slam_sizes(self, graph=0):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.qs_slam_sizes(self._h, graph, C.byref(a), C.byref(b), C.byref(c)), "qs_slam_sizes")
        return a.value, b.value, c.value

    def closure_agents(self, graph=0):
        """agent_id of each closure's closing node (self.nodes[node_idx].agent_id in the reference, :335)."""
        n = self.slam_sizes(graph)[2]
        out = np.zeros(n, dtype=np.uint8)
        if n:
            self._chk(self._L.qs_slam_closure_agents(self._h, graph, _ptr(out), n), "qs_slam_closure_agents")
        return out

    def closures(self, graph=0):
        n = self.slam_sizes(graph)[2]
        idx = np.zeros((n, 2), dtype=np.int64)
        corr = np.zeros((n, 2), dtype=np.float64)
        if n:
            self._chk(self._L.qs_slam_closures(self._h, graph, _ptr(idx), _ptr(corr), n), "qs_slam_closures")
        return idx, corr

    def landmarks(self, graph=0):
        n = self.slam_sizes(graph)[1]
        xy = np.zeros((n, 2), dtype=np.float64)
        ti = np.zeros((n, 2), dtype=np.int64)
        if n:
            self._chk(self._L.qs_slam_landmarks(self._h, graph, _ptr(xy), _ptr(ti), n), "qs_slam_landmarks")
        return xy, ti

    def slam_add_poses(self, x, y, agent, landmark):
        """Batched PoseGraphSLAM.add_pose on poses as given -> (closed uint8 [n], corr float64 [n, 2])."""
        xs = np.ascontiguousarray(x, dtype=np.float64); ys = np.ascontiguousarray(y, dtype=np.float64)
        ag = np.ascontiguousarray(agent, dtype=np.uint8); lm = np.ascontiguousarray(landmark, dtype=np.uint8)
        n = len(xs)
        closed = np.zeros(n, dtype=np.uint8); corr = np.zeros((n, 2), dtype=np.float64)
        self._chk(self._L.qs_slam_add_poses(self._h, _ptr(xs), _ptr(ys), _ptr(ag), _ptr(lm), n, _ptr(closed), _ptr(corr)),
                  "qs_slam_add_poses")
        return closed, corr

    def drift(self, bot):
        out = np.zeros(2, dtype=np.float64)
        self._chk(self._L.qs_drift(self._h, bot, _ptr(out)), "qs_drift")
        return out

    @property
    def drift_correction(self):
        """dict bot -> (dx, dy), as main()'s drift_correction (:782)."""
        return {b: tuple(self.drift(b)) for b in range(1, self.max_agent + 1)}

    # -- ZONE -------------------------------------------------------------------------------------
    def zone(self, bot):
        out = np.zeros(4, dtype=np.float64)
        valid = C.c_int32()
        self._chk(self._L.qs_zone(self._h, bot, _ptr(out), C.byref(valid)), "qs_zone")
        return tuple(out) if valid.value else None

    def zone_packet(self, bot, online=True) -> bytes:
        out = np.zeros(P.ZONE_SIZE, dtype=np.uint8)
        self._chk(self._L.qs_zone_packet(self._h, bot, int(online), _ptr(out)), "qs_zone_packet")
        return out.tobytes()

    @property
    def zone_boxes(self):
        return {b: self.zone(b) for b in range(1, self.max_agent + 1)}

    # -- merge ------------------------------------------------------------------------------------
    def fuse(self, others):
        arr = (C.c_void_p * len(others))(*[o._h for o in others])
        self._chk(self._L.qs_fuse(self._h, arr, len(others)), "qs_fuse")
        self._map_version += 1

    def fuse_buffers(self, stamp_ptrs, count_ptrs=None):
        n = len(stamp_ptrs)
        sp = (C.c_void_p * n)(*stamp_ptrs)
        cp = (C.c_void_p * n)(*count_ptrs) if count_ptrs else None
        self._chk(self._L.qs_fuse_buffers(self._h, sp, cp, n), "qs_fuse_buffers")
        self._map_version += 1

    def fuse_buffers_range(self, stamp_ptrs, count_ptrs, cell_offset, n_cells, counts_into_fused=False):
        """Fold peers' copies of cells [cell_offset, cell_offset + n_cells) into this grid (raw device addresses of the
        first cell of the range; either list may be None)."""
        n = len(stamp_ptrs if stamp_ptrs else count_ptrs)
        sp = (C.c_void_p * n)(*stamp_ptrs) if stamp_ptrs else None
        cp = (C.c_void_p * n)(*count_ptrs) if count_ptrs else None
        self._chk(self._L.qs_fuse_buffers_range(self._h, sp, cp, n, cell_offset, n_cells, int(counts_into_fused)),
                  "qs_fuse_buffers_range")
        self._map_version += 1

    def fused_counts(self):
        """Snapshot the local counters into the context's second buffer -> (device address, bytes); a collective sums
        that buffer over the ranks (never the local counters themselves)."""
        p, b = C.c_void_p(), C.c_size_t()
        self._chk(self._L.qs_fused_counts(self._h, C.byref(p), C.byref(b)), "qs_fused_counts")
        return p.value, b.value

    # -- the same fuse with RCCL behind the C ABI (hosts without torch; csrc/rccl_fuse.hip) -------------------------------
    @staticmethod
    def rccl_unique_id():
        out = np.zeros(128, dtype=np.uint8)
        check(None, _lib.load().qs_rccl_unique_id(_ptr(out)), "qs_rccl_unique_id")
        return out

    def rccl_comm_init(self, unique_id, world, rank):
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        comm = C.c_void_p()
        self._chk(self._L.qs_rccl_comm_init(self._h, _ptr(uid), world, rank, C.byref(comm)), "qs_rccl_comm_init")
        return comm

    def rccl_comm_destroy(self, comm):
        self._chk(self._L.qs_rccl_comm_destroy(comm), "qs_rccl_comm_destroy")

    def sparse_fuse_rccl(self, comm, world, rank):
        """One sparse fuse over RCCL -> dict(blocks_own, payload_bytes, sent_bytes, received_bytes)."""
        st = np.zeros(4, dtype=np.uint64)
        self._chk(self._L.qs_sparse_fuse_rccl(self._h, comm, world, rank, _ptr(st)), "qs_sparse_fuse_rccl")
        self._map_version += 1
        return dict(zip(("blocks_own", "payload_bytes", "sent_bytes", "received_bytes"), (int(v) for v in st)))

    def fused_counts_buffer(self):
        """(device address, bytes) of the fused counters as they stand (no snapshot); address 0 before the first fuse."""
        p, b = C.c_void_p(), C.c_size_t()
        self._chk(self._L.qs_fused_counts_buffer(self._h, C.byref(p), C.byref(b)), "qs_fused_counts_buffer")
        return p.value or 0, b.value

    def counts_source(self, fused):
        self._chk(self._L.qs_counts_source(self._h, int(bool(fused))), "qs_counts_source")

    def epoch_would_rebase(self, n, seq0=None):
        w = C.c_int32()
        self._chk(self._L.qs_epoch_query(self._h, UINT64_MAX if seq0 is None else int(seq0), n, C.byref(w)), "qs_epoch_query")
        return bool(w.value)

    def mark_fused(self):
        """Record that the shards have exchanged their stamps.  Whoever fuses into the device buffers from outside (a
        collective on dist.grid_tensors) calls this afterwards: it also drops the look-alike's cached .grid."""
        self._chk(self._L.qs_mark_fused(self._h), "qs_mark_fused")
        self._map_version += 1

    # -- sparse fuse: only the blocks written since the last fuse travel (include/quasar_slam.h) -----------------------
    def dirty_tracking(self, on=True):
        self._chk(self._L.qs_dirty_tracking(self._h, int(bool(on))), "qs_dirty_tracking")

    def dirty_blocks(self):
        """(blocks marked since the last sparse fuse, cells per block)."""
        n, cells = C.c_size_t(), C.c_size_t()
        self._chk(self._L.qs_dirty_blocks(self._h, C.byref(n), C.byref(cells)), "qs_dirty_blocks")
        return n.value, cells.value

    def sparse_fuse_begin(self, world, rank):
        """-> (device address of the [world][bitmap_bytes] bitmap array, bitmap_bytes); slot `rank` holds this rank's."""
        p, b = C.c_void_p(), C.c_size_t()
        self._chk(self._L.qs_sparse_fuse_begin(self._h, world, rank, C.byref(p), C.byref(b)), "qs_sparse_fuse_begin")
        return p.value, b.value

    def sparse_fuse_plan(self, world):
        """-> (n_blocks uint32 [world], offsets [world + 1] bytes, payload device address, block_bytes)."""
        n = np.zeros(world, dtype=np.uint32)
        off = np.zeros(world + 1, dtype=np.uintp)
        p, bb = C.c_void_p(), C.c_size_t()
        self._chk(self._L.qs_sparse_fuse_plan(self._h, _ptr(n), _ptr(off), C.byref(p), C.byref(bb)), "qs_sparse_fuse_plan")
        return n, off.astype(np.int64), p.value or 0, bb.value

    def sparse_fuse_apply(self):
        self._chk(self._L.qs_sparse_fuse_apply(self._h), "qs_sparse_fuse_apply")
        self._map_version += 1

    def grid_to_pcd(self, grid, res, ox, oy):
        """MapMerger.grid_to_pcd (map_merger.py:64-85) -> float64 [n,2] (x, y)."""
        grid = np.ascontiguousarray(grid, dtype=np.int8)
        h, w = grid.shape
        n = C.c_size_t()
        self._chk(self._L.qs_grid_to_pcd(self._h, _ptr(grid), h, w, res, ox, oy, None, 0, C.byref(n)),
                  "qs_grid_to_pcd")
        xy = np.zeros((n.value, 2), dtype=np.float64)
        if n.value:
            self._chk(self._L.qs_grid_to_pcd(self._h, _ptr(grid), h, w, res, ox, oy, _ptr(xy), n.value,
                                             C.byref(n)), "qs_grid_to_pcd")
        return xy

    def rasterise(self, xy, res):
        """MapMerger.publish_global_map (map_merger.py:87-127) -> (int8 grid, (min_x, min_y))."""
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        dims = np.zeros(2, dtype=np.int32)
        origin = np.zeros(2, dtype=np.float64)
        self._chk(self._L.qs_rasterise(self._h, _ptr(xy), len(xy), res, _ptr(dims), _ptr(origin), None),
                  "qs_rasterise")
        if len(xy) == 0:
            return None, None
        grid = np.empty((int(dims[0]), int(dims[1])), dtype=np.int8)
        self._chk(self._L.qs_rasterise(self._h, _ptr(xy), len(xy), res, _ptr(dims), _ptr(origin), _ptr(grid)),
                  "qs_rasterise")
        return grid, origin

    # -- ICP / voxel down-sample: map_merger.py:45-60 (Open3D semantics: N3, parity unpinned; grid_to_pcd and rasterise
    #    above are pinned against the reference's own methods, tests/golden/merger_calls.npz) ---------
    def icp(self, src_xy, dst_xy, max_dist=1.0, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        """registration_icp(source, target, max_dist, I, PointToPoint, max_iteration) on planar clouds.
        Returns (T 3x3, fitness, inlier_rmse, iterations)."""
        a = np.ascontiguousarray(src_xy, dtype=np.float64); b = np.ascontiguousarray(dst_xy, dtype=np.float64)
        T = np.zeros(9, dtype=np.float64)
        fit, rm, it = C.c_double(), C.c_double(), C.c_int32()
        self._chk(self._L.qs_icp(self._h, _ptr(a), len(a), _ptr(b), len(b), max_dist, max_iter, rel_fitness, rel_rmse,
                                 _ptr(T), C.byref(fit), C.byref(rm), C.byref(it)), "qs_icp")
        return T.reshape(3, 3), fit.value, rm.value, it.value

    def nn_search(self, src_xy, dst_xy, max_dist=1.0, mode=0):
        """Nearest target of every source point (the correspondence step of registration_icp): (corr int32 [n], d2 float64 [n],
        (search_ms, prep_ms)).  mode 0 auto, 1 scalar fp64, 2 MFMA-screened; results are identical."""
        a = np.ascontiguousarray(src_xy, dtype=np.float64); b = np.ascontiguousarray(dst_xy, dtype=np.float64)
        corr = np.empty(len(a), dtype=np.int32); d2 = np.empty(len(a), dtype=np.float64)
        ms = np.zeros(2, dtype=np.float32)
        self._chk(self._L.qs_nn_search(self._h, _ptr(a), len(a), _ptr(b), len(b), max_dist, mode, _ptr(corr), _ptr(d2), _ptr(ms)),
                  "qs_nn_search")
        return corr, d2, (float(ms[0]), float(ms[1]))

    CHAIN_FORMS = {"auto": 0, "free": 1, "window": 2, "free_posting": 3}

    def set_chain_form(self, form):
        """Which device form of the loop-closure chain runs: "auto" (default), "free" (free-running), "free_posting" (free-running,
        the owner waves post their landmarks' poses for each other), "window" (one barrier per window).  Same closures,
        landmarks and drifts whichever (dual_bot_mapper.py:292-326)."""
        self._chk(self._L.qs_set_chain_form(self._h, self.CHAIN_FORMS[form]), "qs_set_chain_form")

    def chain_form(self):
        """The form the last ingest used: "free", "free_posting" or "window"."""
        return {1: "free", 2: "window", 3: "free_posting"}[self._L.qs_chain_form(self._h)]

    def set_chain_lean(self, mode="auto", limit=0):
        """The lean owner of the free-running chain (32-bit node indices, decisions settled by their first rows): "auto"
        (default: wherever a launch's graph allows it) or "off".  limit: the node count at which it stops (0: the largest
        possible, 0x7f7f7f7f).  Same results either way."""
        self._chk(self._L.qs_set_chain_lean(self._h, {"auto": 0, "off": 1}[mode], int(limit)), "qs_set_chain_lean")

    def chain_lean(self):
        """Whether every graph of the last ingest ran the lean owner (waits for the stream)."""
        r = self._L.qs_chain_lean(self._h)
        if r < 0:
            self._chk(r, "qs_chain_lean")
        return bool(r)

    def set_chain_plan(self, on=True):
        """The lean owner walks a per-agent plan of its events, built on the device ahead of the chain (default), or streams
        the graph's whole event list as the general owner does (on=False).  Same results either way."""
        self._chk(self._L.qs_set_chain_plan(self._h, 1 if on else 0), "qs_set_chain_plan")

    def chain_plan(self):
        """Whether the last ingest had a plan and every graph's lean owner walked it (waits for the stream)."""
        r = self._L.qs_chain_plan(self._h)
        if r < 0:
            self._chk(r, "qs_chain_plan")
        return bool(r)

    def chain_plan_read(self, bot):
        """Diagnostic: bot's part of the plan of the last ingest, valid until the next one: dict(node int32 [n_own], r uint32,
        skip uint32, first int) -- its events in list order (node index, position in the graph's event list, own index it goes
        on at after a closure there) and the own index of its first event past the cool-down it came with.  Raises if the
        last ingest had no plan."""
        n, first = C.c_size_t(0), C.c_uint32(0)
        self._chk(self._L.qs_chain_plan_read(self._h, bot, None, None, None, 0, C.byref(n), C.byref(first)), "qs_chain_plan_read")
        node = np.empty(n.value, dtype=np.int32); r = np.empty(n.value, dtype=np.uint32); skip = np.empty(n.value, dtype=np.uint32)
        if n.value:
            self._chk(self._L.qs_chain_plan_read(self._h, bot, _ptr(node), _ptr(r), _ptr(skip), n.value, C.byref(n), C.byref(first)),
                      "qs_chain_plan_read")
        return {"node": node, "r": r, "skip": skip, "first": int(first.value)}

    def set_chain_lookahead(self, on=True):
        """The lean owner walks a bucket on only if its node's look-ahead word -- the index of the successor node's first
        entry -- lies below the match it has (default), or by the node's own last entry as the general query does
        (on=False).  Same results either way; fewer walks with it on."""
        self._chk(self._L.qs_set_chain_lookahead(self._h, 1 if on else 0), "qs_set_chain_lookahead")

    def chain_lookahead(self):
        """Whether the lean owner tests the look-ahead word."""
        r = self._L.qs_chain_lookahead(self._h)
        if r < 0:
            self._chk(r, "qs_chain_lookahead")
        return bool(r)

    def set_chain_scout(self, on=True):
        """In graphs of up to two agents a scout wave per owner stages the rows of the decision after next in LDS, and the
        owner settles from them the decisions it can (on=True), or every decision is made from the owner's own loads
        (the default: the scouts measured slower).  Same results either way."""
        self._chk(self._L.qs_set_chain_scout(self._h, 1 if on else 0), "qs_set_chain_scout")

    def chain_scout(self):
        """(staged, fallback) of the last ingest: the owners' decisions settled from a scout's stage and those made from their
        own loads; (0, 0) if the launch had no scouts (waits for the stream)."""
        s, f = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.qs_chain_scout(self._h, C.byref(s), C.byref(f)), "qs_chain_scout")
        return int(s.value), int(f.value)

    def mfma_f64_rate(self):
        """Measured dense fp64 MFMA rate of this GPU in TFLOP/s (diagnostic)."""
        v = C.c_double()
        self._chk(self._L.qs_diag_mfma_f64_rate(self._h, C.byref(v)), "qs_diag_mfma_f64_rate")
        return v.value

    def diag_latencies(self):
        """Measured latencies (shader-clock cycles) of the primitives a loop-closure decision chains together, by one
        workgroup on this GPU: dict with l2_load, l1_load, lds_read, fma_f64, dpp_step, readlane_step, barrier_16_waves,
        barrier_5_waves, clock_mhz."""
        out = np.zeros(9, dtype=np.float64)
        self._chk(self._L.qs_diag_latencies(self._h, _ptr(out)), "qs_diag_latencies")
        names = ("l2_load", "l1_load", "lds_read", "fma_f64", "dpp_step", "readlane_step", "barrier_16_waves", "barrier_5_waves", "clock_mhz")
        return dict(zip(names, (float(v) for v in out)))

    def voxel_downsample(self, xy, voxel):
        a = np.ascontiguousarray(xy, dtype=np.float64)
        n = C.c_size_t()
        self._chk(self._L.qs_voxel_downsample(self._h, _ptr(a), len(a), voxel, None, 0, C.byref(n)), "qs_voxel_downsample")
        out = np.zeros((n.value, 2), dtype=np.float64)
        if n.value:
            self._chk(self._L.qs_voxel_downsample(self._h, _ptr(a), len(a), voxel, _ptr(out), n.value, C.byref(n)),
                      "qs_voxel_downsample")
        return out

    def voxel_downsample_device(self, d_xy, n, voxel, d_out=0, cap=0):
        """voxel_downsample over a cloud on the device (qs_voxel_downsample_device): d_xy, d_out are device addresses of float64
        x y pairs (n points in, room for cap out; d_out = 0 queries the count) or torch tensors on this GPU.  -> number of
        voxels.  Same points, same order, same bits as voxel_downsample."""
        k = C.c_size_t()
        self._chk(self._L.qs_voxel_downsample_device(self._h, C.c_void_p(_dev_addr(d_xy)), int(n), voxel,
                                                     C.c_void_p(_dev_addr(d_out)), int(cap), C.byref(k)), "qs_voxel_downsample_device")
        return k.value

    # -- map merge session: map_merger.py:28-127 with the node's state on the device ----------------
    def merge_reset(self):
        """Empty the session's global cloud (the ICP parameters stay); the next map is adopted."""
        self._chk(self._L.qs_merge_reset(self._h), "qs_merge_reset")

    def merge_params(self, icp_threshold=1.0, icp_iterations=30, min_fitness=0.6):
        self._chk(self._L.qs_merge_params(self._h, icp_threshold, icp_iterations, min_fitness), "qs_merge_params")

    @staticmethod
    def _merge_result(r):
        return {"status": QS_MERGE_STATUS[r.status], "iterations": int(r.iterations), "n_local": int(r.n_local),
                "n_global": int(r.n_global), "fitness": float(r.fitness), "rmse": float(r.rmse),
                "T": np.array(r.T, dtype=np.float64).reshape(3, 3)}

    def merge_grid(self, grid, res, ox, oy):
        """One map_callback (map_merger.py:35-62) of the session: grid is an int8 [h, w] numpy array, or a contiguous torch
        int8 tensor on this GPU whose contents are complete (nothing is uploaded then).  -> dict: status ("empty", "adopted",
        "merged", "rejected"), T, fitness, rmse, iterations (those of icp(local, global cloud)), n_local, n_global."""
        r = QsMergeResult()
        if hasattr(grid, "data_ptr"):
            if not (grid.is_cuda and grid.is_contiguous() and grid.dim() == 2 and grid.element_size() == 1):
                raise ValueError("merge_grid: a device grid is a contiguous 2-D int8 tensor on the GPU")
            h, w = grid.shape
            self._chk(self._L.qs_merge_grid_device(self._h, C.c_void_p(grid.data_ptr()), h, w, res, ox, oy, C.byref(r)),
                      "qs_merge_grid_device")
        else:
            grid = np.ascontiguousarray(grid, dtype=np.int8)
            h, w = grid.shape
            self._chk(self._L.qs_merge_grid(self._h, _ptr(grid), h, w, res, ox, oy, C.byref(r)), "qs_merge_grid")
        return self._merge_result(r)

    def merge_map(self, src):
        """One map_callback with another mapper's own map (or this one's) as the message, read from its stamps on the device:
        what merge_grid(src.grid_i8(), src.res, src.ox, src.oy) gives, with no int8 view and no transfer."""
        r = QsMergeResult()
        self._chk(self._L.qs_merge_map(self._h, src._h, C.byref(r)), "qs_merge_map")
        return self._merge_result(r)

    def merge_cloud(self):
        """The session's global cloud -> float64 [n, 2]."""
        n = C.c_size_t()
        self._chk(self._L.qs_merge_cloud(self._h, None, 0, C.byref(n)), "qs_merge_cloud")
        xy = np.zeros((n.value, 2), dtype=np.float64)
        if n.value:
            self._chk(self._L.qs_merge_cloud(self._h, _ptr(xy), n.value, C.byref(n)), "qs_merge_cloud")
        return xy

    def merge_global_map(self):
        """publish_global_map (map_merger.py:87-127) of the session's cloud -> (int8 grid, (min_x, min_y)), or (None, None)
        while it is empty."""
        dims = np.zeros(2, dtype=np.int32)
        origin = np.zeros(2, dtype=np.float64)
        self._chk(self._L.qs_merge_global_map(self._h, _ptr(dims), _ptr(origin), None), "qs_merge_global_map")
        if dims[0] == 0:
            return None, None
        grid = np.empty((int(dims[0]), int(dims[1])), dtype=np.int8)
        self._chk(self._L.qs_merge_global_map(self._h, _ptr(dims), _ptr(origin), _ptr(grid)), "qs_merge_global_map")
        return grid, origin

    # -- frontiers: dual_bot_mapper.py:181-237, :948-956 ----------------------------------------
    def frontier_cells(self):
        """OccupancyGrid.get_frontiers() -> int32 [n, 2] (gx, gy), row-major order."""
        n = C.c_size_t()
        self._chk(self._L.qs_frontier_cells(self._h, None, 0, C.byref(n)), "qs_frontier_cells")
        xy = np.zeros((n.value, 2), dtype=np.int32)
        if n.value:
            self._chk(self._L.qs_frontier_cells(self._h, _ptr(xy), n.value, C.byref(n)), "qs_frontier_cells")
        return xy

    def frontier_clusters(self, min_cluster=3):
        """cluster_frontiers() as int64 [k, 5]: size, first_gx, first_gy, sum_gx, sum_gy, in the
        reference's cluster order."""
        n = C.c_size_t()
        self._chk(self._L.qs_frontier_clusters(self._h, min_cluster, None, 0, C.byref(n)), "qs_frontier_clusters")
        st = np.zeros((n.value, 5), dtype=np.int64)
        if n.value:
            self._chk(self._L.qs_frontier_clusters(self._h, min_cluster, _ptr(st), n.value, C.byref(n)),
                      "qs_frontier_clusters")
        return st

    def frontier_members(self):
        """int32 [n, 3]: every frontier cell (gx, gy) in row-major order with the linear index of the first cell of its
        4-connected cluster (clusters labelled on the device)."""
        n = C.c_size_t()
        self._chk(self._L.qs_frontier_members(self._h, None, 0, C.byref(n)), "qs_frontier_members")
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._chk(self._L.qs_frontier_members(self._h, _ptr(out), n.value, C.byref(n)), "qs_frontier_members")
        return out

    def frontier_centroids(self, min_cluster=3):
        """[cluster_centroid_world(c) for c in clusters] (:955): mean cell index by true division,
        then grid_to_world (:127-131, cell centre)."""
        out = []
        for size, _, _, sx, sy in self.frontier_clusters(min_cluster).tolist():
            ax, ay = sx / size, sy / size
            out.append((self.ox + (ax + 0.5) * self.res, self.oy + (ay + 0.5) * self.res))
        return out

    def _bot_array(self, who, bot_xy):
        """bot_xy as float64 [n, 2]; more than QS_FT_MAX_BOTS bots are refused in the name of `who`."""
        b = np.ascontiguousarray(bot_xy, dtype=np.float64).reshape(-1, 2)
        if len(b) > _lib.QS_FT_MAX_BOTS:
            raise ValueError(f"{who}: at most {_lib.QS_FT_MAX_BOTS} bots per call")
        return b

    def _centroid_buffer(self, min_cluster, wanted):
        """(float64 [k, 2], k) for a target call asked to hand back the centroids, else (None, 0).  The count comes first: a
        second call would observe the same map."""
        if not wanted:
            return None, 0
        k = C.c_size_t()
        self._chk(self._L.qs_frontier_clusters(self._h, min_cluster, None, 0, C.byref(k)), "qs_frontier_clusters")
        return np.zeros((k.value, 2), dtype=np.float64), k.value

    def frontier_targets(self, bot_xy, separation=P.FRONTIER_SEPARATION, min_cluster=P.FRONTIER_MIN_CLUSTER,
                         return_centroids=False):
        """The greedy frontier assignment of dual_bot_mapper.py:958-992 on the device.  bot_xy: [n, 2] positions in
        greedy order.  Returns (idx int64 [n]: index into frontier_centroids(min_cluster), -1 = no target;
        xy float64 [n, 2]: that centroid, NaN where idx is -1), plus (centroids float64 [k, 2], stats dict) on request."""
        b = self._bot_array("frontier_targets", bot_xy)
        n = len(b)
        idx = np.full(n, -1, dtype=np.int64)
        xy = np.full((n, 2), np.nan, dtype=np.float64)
        st = np.zeros(4, dtype=np.uint64)
        k = C.c_size_t()
        cents, cap = self._centroid_buffer(min_cluster, return_centroids)
        self._chk(self._L.qs_frontier_targets(self._h, min_cluster, float(separation), _ptr(b), n, _ptr(idx), _ptr(xy),
                                              _ptr(cents) if cap else None, cap, C.byref(k), _ptr(st)),
                  "qs_frontier_targets")
        if not return_centroids:
            return idx, xy
        stats = dict(zip(("n_centroids", "k", "fallbacks", "reserved"), (int(v) for v in st)))
        return idx, xy, cents[:k.value], stats

    def assign_frontier_targets(self, bot_states, separation=P.FRONTIER_SEPARATION, min_cluster=P.FRONTIER_MIN_CLUSTER,
                                by_path=False, return_waypoints=False, by_territory=False, return_territory=False,
                                by_gain=False, **plan_params):
        """The reference's target_assignments (:958-992): {bot: (x, y)} of the online bots -> {bot: (tx, ty)} for
        the bots that got a target, bots taken in ascending id.  by_path=True (opt-in): the targets of
        frontier_targets_by_path instead (plan_params: clearance, snap_radius, lookahead), and with return_waypoints
        also {bot: (wx, wy)}, the waypoint of each assigned bot's path, as a second dict.  by_territory=True (opt-in,
        excludes by_path): the targets of frontier_targets_by_territory likewise (`separation` plays no part), and with
        return_territory also {bot: (area, box)} of every bot given, box a tuple of cells or None, as the last value.
        by_gain=True (opt-in, excludes the other two): the targets of frontier_targets_by_gain, with by_path's returns;
        plan_params may then also hold gain_range and gain_bias."""
        if by_path + by_territory + by_gain > 1:
            raise ValueError("assign_frontier_targets: by_path, by_territory and by_gain exclude each other")
        if return_territory and not by_territory:
            raise ValueError("assign_frontier_targets: return_territory needs by_territory=True")
        plain = not (by_path or by_territory or by_gain)
        if plain and (return_waypoints or plan_params):
            raise ValueError("assign_frontier_targets: waypoints and plan parameters need by_path=True or by_gain=True")
        bots = sorted(bot_states)
        pos = [bot_states[b] for b in bots]
        if not bots:
            res = None                 # (no call: nothing below looks at it)
        elif plain:
            res = dict(zip(("idx", "xy"), self.frontier_targets(pos, separation, min_cluster)))
        elif by_territory:
            res = self.frontier_targets_by_territory(pos, min_cluster, waypoints=return_waypoints, **plan_params)
        else:
            call = self.frontier_targets_by_gain if by_gain else self.frontier_targets_by_path
            res = call(pos, separation, min_cluster, waypoints=return_waypoints, **plan_params)
        got = [(i, b) for i, b in enumerate(bots) if res["idx"][i] >= 0]
        out = [{b: (float(res["xy"][i, 0]), float(res["xy"][i, 1])) for i, b in got}]
        if return_waypoints:
            out.append({b: (float(res["waypoint"][i, 0]), float(res["waypoint"][i, 1])) for i, b in got})
        if return_territory:
            out.append({b: (int(res["area"][i]), tuple(int(v) for v in res["box"][i]) if res["area"][i] else None)
                        for i, b in enumerate(bots)})
        return out[0] if len(out) == 1 else tuple(out)

    _PATH_STATS = ("n_centroids", "centroid_cells", "bot_cells", "groups", "rounds", "tile_visits", "fallbacks")
    _TERRITORY_STATS = ("rounds", "tile_visits", "bot_cells", "owned_cells", "n_centroids", "centroid_cells", "centroids_owned",
                        "reserved")

    def _path_cost_targets(self, who, call, bot_xy, min_cluster, plan, return_centroids, waypoints, stat_names,
                           per_bot=(), per_centroid=()):
        """What frontier_targets_by_path, _by_gain and _by_territory do alike round their one C call: the bots, the plan
        parameters (clearance, snap_radius, lookahead), the per-bot output arrays, the centroid buffers on request, then
        call(a) and the result dict.  a holds the C call's arguments: prm, bots (bot_xy, n, then the six per-bot arrays,
        the two waypoint ones None without waypoints), cents, cap, k, st, and one pointer for each name in per_bot
        {name: (dtype, fill, shape after n)} and per_centroid {name: (dtype, fill)}, which also become keys of the result."""
        b = self._bot_array(who, bot_xy)
        n = len(b)
        prm = self._plan_params(*plan)
        out = dict(idx=np.full(n, -1, dtype=np.int64), xy=np.full((n, 2), np.nan, dtype=np.float64),
                   cost=np.full(n, 0xFFFFFFFF, dtype=np.uint32), status=np.zeros(n, dtype=np.int32),
                   waypoint_cell=np.full((n, 2), -1, dtype=np.int32), waypoint=np.full((n, 2), np.nan, dtype=np.float64))
        a = types.SimpleNamespace(prm=C.byref(prm), bots=[_ptr(b), n] + [_ptr(out[key]) for key in ("idx", "xy", "cost", "status")])
        a.bots += [_ptr(out[key]) if waypoints else None for key in ("waypoint_cell", "waypoint")]
        for name, (dtype, fill, shape) in dict(per_bot).items():
            out[name] = np.full((n,) + shape, fill, dtype=dtype)
            setattr(a, name, _ptr(out[name]))
        st = np.zeros(8, dtype=np.uint64)
        k = C.c_size_t()
        cents, cap = self._centroid_buffer(min_cluster, return_centroids)
        per_c = {name: np.full(cap, fill, dtype=dtype) for name, (dtype, fill) in dict(per_centroid).items()}
        a.cents, a.cap, a.k, a.st = _ptr(cents) if cap else None, cap, C.byref(k), _ptr(st)
        for name, arr in per_c.items():
            setattr(a, name, _ptr(arr) if cap else None)
        self._chk(call(a), "qs_" + who)
        out["stats"] = dict(zip(stat_names, (int(v) for v in st)))
        if return_centroids:
            out["centroids"] = cents[:k.value]
            out.update((name, arr[:k.value]) for name, arr in per_c.items())
        return out

    def frontier_targets_by_path(self, bot_xy, separation=P.FRONTIER_SEPARATION, min_cluster=P.FRONTIER_MIN_CLUSTER,
                                 clearance=P.PLAN_CLEARANCE, snap_radius=P.PLAN_SNAP_RADIUS, lookahead=P.PLAN_LOOKAHEAD,
                                 return_centroids=False, waypoints=True):
        """Frontier targets ranked by path cost over the mapped free space (include/quasar_slam.h, "frontier targets by
        path cost"): bots in greedy order, each takes the eligible centroid with the smallest (cost, index).  Returns a
        dict of numpy arrays: idx int64 [n] (index into frontier_centroids(min_cluster), -1 = none), xy float64 [n, 2]
        (NaN where none), cost uint32 [n], status int32 [n] (QS_PLAN_OK / _NO_START / _UNREACHABLE), waypoint_cell int32
        [n, 2] and waypoint float64 [n, 2] (what plan_paths(bot, target) returns; -1 / NaN where none or with
        waypoints=False, which skips that stage), stats; with return_centroids also centroids float64 [k, 2]."""
        return self._path_cost_targets(
            "frontier_targets_by_path", lambda a: self._L.qs_frontier_targets_by_path(
                self._h, min_cluster, float(separation), a.prm, *a.bots, a.cents, a.cap, a.k, a.st),
            bot_xy, min_cluster, (clearance, snap_radius, lookahead), return_centroids, waypoints, self._PATH_STATS + ("reserved",))

    # -- frontier gain (include/quasar_slam.h, "frontier gain"; no reference counterpart) --------------------------
    def frontier_gain(self, min_cluster=P.FRONTIER_MIN_CLUSTER, range=_lib.QS_GAIN_DEFAULT_RANGE):
        """(viewpoints int32 [k, 2] (gx, gy), gain int32 [k]) of the clusters of frontier_clusters(min_cluster), in their
        order: the member cell nearest the integer centroid, and the UNKNOWN cells within `range` cells of it that no
        OCCUPIED cell hides."""
        n = C.c_size_t()
        self._chk(self._L.qs_frontier_gain(self._h, min_cluster, int(range), None, None, 0, C.byref(n)), "qs_frontier_gain")
        view, gain = np.zeros((n.value, 2), dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._chk(self._L.qs_frontier_gain(self._h, min_cluster, int(range), _ptr(view), _ptr(gain), n.value, C.byref(n)),
                      "qs_frontier_gain")
        return view, gain

    def frontier_targets_by_gain(self, bot_xy, separation=P.FRONTIER_SEPARATION, min_cluster=P.FRONTIER_MIN_CLUSTER,
                                 clearance=P.PLAN_CLEARANCE, snap_radius=P.PLAN_SNAP_RADIUS, lookahead=P.PLAN_LOOKAHEAD,
                                 gain_range=_lib.QS_GAIN_DEFAULT_RANGE, gain_bias=_lib.QS_GAIN_DEFAULT_BIAS,
                                 return_centroids=False, waypoints=True):
        """frontier_targets_by_path with the centroids ordered by gain over cost (include/quasar_slam.h, "frontier gain",
        G6): a bot takes the eligible centroid k with the smallest (cost + gain_bias) / gain[k].  Returns that call's dict
        plus gain int32 [n] (the gain of each bot's target, 0 where none); stats["gain_sum"] is the sum of all gains."""
        gprm = _lib.QsGainParams(int(gain_range), int(gain_bias), (0, 0))
        return self._path_cost_targets(
            "frontier_targets_by_gain", lambda a: self._L.qs_frontier_targets_by_gain(
                self._h, min_cluster, float(separation), a.prm, C.byref(gprm), *a.bots, a.cents, a.cap, a.k, a.gain, a.st),
            bot_xy, min_cluster, (clearance, snap_radius, lookahead), return_centroids, waypoints, self._PATH_STATS + ("gain_sum",),
            per_bot=dict(gain=(np.int32, 0, ())))

    # -- territories (include/quasar_slam.h, "territories"; no reference counterpart) ----------------------------
    def territories(self, bot_xy, clearance=P.PLAN_CLEARANCE, snap_radius=P.PLAN_SNAP_RADIUS, return_owner=False,
                    return_cost=False):
        """The traversable cells partitioned among the bots by path cost: each cell belongs to the bot with the smallest
        (cost, bot).  Returns a dict of numpy arrays: status int32 [n] (QS_PLAN_OK / _NO_START), area int64 [n] (cells
        owned), box int32 [n, 4] (min gx, min gy, max gx, max gy; -1 where area is 0), stats; with return_owner also owner
        int16 [size, size] indexed [gy, gx] (-1 = nobody's), with return_cost also cost uint32 [size, size] (0xFFFFFFFF
        there)."""
        b = self._bot_array("territories", bot_xy)
        n = len(b)
        prm = self._plan_params(clearance, snap_radius, P.PLAN_LOOKAHEAD)
        status = np.zeros(n, dtype=np.int32)
        area = np.zeros(n, dtype=np.int64)
        box = np.full((n, 4), -1, dtype=np.int32)
        st = np.zeros(8, dtype=np.uint64)
        owner = np.empty((self.size, self.size), dtype=np.int16) if return_owner else None
        cost = np.empty((self.size, self.size), dtype=np.uint32) if return_cost else None
        self._chk(self._L.qs_territories(self._h, C.byref(prm), _ptr(b), n, _ptr(owner) if return_owner else None,
                                         _ptr(cost) if return_cost else None, _ptr(status), _ptr(area), _ptr(box), _ptr(st)),
                  "qs_territories")
        out = dict(status=status, area=area, box=box, stats=dict(zip(self._TERRITORY_STATS, (int(v) for v in st))))
        if return_owner:
            out["owner"] = owner
        if return_cost:
            out["cost"] = cost
        return out

    def frontier_targets_by_territory(self, bot_xy, min_cluster=P.FRONTIER_MIN_CLUSTER, clearance=P.PLAN_CLEARANCE,
                                      snap_radius=P.PLAN_SNAP_RADIUS, lookahead=P.PLAN_LOOKAHEAD, return_centroids=False,
                                      waypoints=True):
        """Frontier targets by territory (include/quasar_slam.h, "territories", T5): each bot takes the centroid with the
        smallest (cost, index) among those whose cell it owns; there is no separation rule.  Returns the keys of
        frontier_targets_by_path (idx, xy, cost, status, waypoint_cell, waypoint, stats) plus area int64 [n] and box int32
        [n, 4]; with return_centroids also centroids float64 [k, 2] and centroid_owner int32 [k] (-1 = nobody's)."""
        return self._path_cost_targets(
            "frontier_targets_by_territory", lambda a: self._L.qs_frontier_targets_by_territory(
                self._h, min_cluster, a.prm, *a.bots, a.area, a.box, a.cents, a.centroid_owner, a.cap, a.k, a.st),
            bot_xy, min_cluster, (clearance, snap_radius, lookahead), return_centroids, waypoints, self._TERRITORY_STATS,
            per_bot=dict(area=(np.int64, 0, ()), box=(np.int32, -1, (4,))), per_centroid=dict(centroid_owner=(np.int32, -1)))

    # -- path planning (include/quasar_slam.h, "path planning"; no reference counterpart) ----------------------
    def traversable(self, clearance=P.PLAN_CLEARANCE):
        """Rule 1 over the whole grid: uint8 [size, size] indexed [gy, gx], 1 = traversable."""
        out = np.zeros((self.size, self.size), dtype=np.uint8)
        self._chk(self._L.qs_traversable(self._h, int(clearance), _ptr(out)), "qs_traversable")
        return out

    @staticmethod
    def _plan_params(clearance, snap_radius, lookahead):
        return _lib.QsPlanParams(int(clearance), int(snap_radius), int(lookahead), 0)

    def distance_field(self, goal_xy, clearance=P.PLAN_CLEARANCE, snap_radius=P.PLAN_SNAP_RADIUS,
                       lookahead=P.PLAN_LOOKAHEAD):
        """Rule 3 for one goal (world x, y): uint32 [size, size] indexed [gy, gx], 0xFFFFFFFF = unreached."""
        g = np.ascontiguousarray(goal_xy, dtype=np.float64).reshape(2)
        out = np.empty((self.size, self.size), dtype=np.uint32)
        prm = self._plan_params(clearance, snap_radius, lookahead)
        self._chk(self._L.qs_plan_field(self._h, C.byref(prm), _ptr(g), _ptr(out)), "qs_plan_field")
        return out

    def plan_paths(self, starts, goals, clearance=P.PLAN_CLEARANCE, snap_radius=P.PLAN_SNAP_RADIUS,
                   lookahead=P.PLAN_LOOKAHEAD, return_paths=False, path_cap=None):
        """Paths from starts[i] to goals[i] (world [n, 2] each) and the waypoint a bot can drive to straight.  Returns a
        dict of numpy arrays: status int32 [n] (QS_PLAN_*), waypoint_cell int32 [n, 2], waypoint float64 [n, 2], cost
        uint32 [n], path_len int64 [n]; with return_paths also paths: a list of int32 [k, 2] cell arrays (the first
        path_cap cells; None = every cell), and stats: rounds, tile_visits, groups, snapped."""
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        if len(s) != len(g):
            raise ValueError("plan_paths: starts and goals differ in length")
        n = len(s)
        prm = self._plan_params(clearance, snap_radius, lookahead)
        st = np.zeros(n, dtype=np.int32)
        wc = np.zeros((n, 2), dtype=np.int32)
        wxy = np.zeros((n, 2), dtype=np.float64)
        cost = np.zeros(n, dtype=np.uint32)
        plen = np.zeros(n, dtype=np.int64)
        stats = np.zeros(4, dtype=np.uint64)
        cap, path = 0, None
        if return_paths:
            if path_cap is None:       # every cell: the lengths first (a second call observes the same map)
                self._chk(self._L.qs_plan_paths(self._h, C.byref(prm), _ptr(s), _ptr(g), n, _ptr(st), _ptr(wc), _ptr(wxy),
                                                _ptr(cost), None, 0, _ptr(plen), None), "qs_plan_paths")
                path_cap = int(plen.max()) if n else 0
            cap = int(path_cap)
            path = np.zeros((n, max(cap, 1), 2), dtype=np.int32)
        self._chk(self._L.qs_plan_paths(self._h, C.byref(prm), _ptr(s), _ptr(g), n, _ptr(st), _ptr(wc), _ptr(wxy),
                                        _ptr(cost), _ptr(path) if cap else None, cap, _ptr(plen), _ptr(stats)),
                  "qs_plan_paths")
        out = dict(status=st, waypoint_cell=wc, waypoint=wxy, cost=cost, path_len=plen,
                   stats=dict(zip(("rounds", "tile_visits", "groups", "snapped"), (int(v) for v in stats))))
        if return_paths:
            out["paths"] = [path[i, :min(int(plen[i]), cap)].copy() for i in range(n)]
        return out

    # -- EKF --------------------------------------------------------------------------------------
    def ekf_init(self, bot, t, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self._chk(self._L.qs_ekf_init(self._h, bot, t, _ptr(x0)), "qs_ekf_init")

    def ekf_step(self, bots, omega_m, t, z_v=None, z_omega=None):
        b = np.ascontiguousarray(bots, dtype=np.int32)
        om = np.ascontiguousarray(omega_m, dtype=np.float64)
        tt = np.ascontiguousarray(t, dtype=np.float64)
        upd = z_v is not None
        zv = np.ascontiguousarray(z_v, dtype=np.float64) if upd else None
        zo = np.ascontiguousarray(z_omega, dtype=np.float64) if upd else None
        self._chk(self._L.qs_ekf_step(self._h, _ptr(b), _ptr(om), _ptr(tt), _ptr(zv), _ptr(zo), len(b), int(upd)),
                  "qs_ekf_step")

    def ekf_state(self, bot):
        x = np.zeros(6, dtype=np.float64)
        Pm = np.zeros((6, 6), dtype=np.float64)
        self._chk(self._L.qs_ekf_state(self._h, bot, _ptr(x), _ptr(Pm)), "qs_ekf_state")
        return x, Pm

    # -- counters / timing ------------------------------------------------------------------------
    def counters(self):
        out = np.zeros(len(_lib.QS_CNT_NAMES), dtype=np.uint64)
        self._chk(self._L.qs_counters(self._h, _ptr(out)), "qs_counters")
        return dict(zip(_lib.QS_CNT_NAMES, (int(v) for v in out)))

    def timing_enable(self, on=True):
        self._chk(self._L.qs_timing_enable(self._h, int(on)), "qs_timing_enable")

    def stage_times(self, reset=True):
        ms = np.zeros(len(_lib.QS_STAGE_NAMES), dtype=np.float64)
        ln = np.zeros(len(_lib.QS_STAGE_NAMES), dtype=np.uint64)
        self._chk(self._L.qs_stage_times(self._h, _ptr(ms), _ptr(ln), int(reset)), "qs_stage_times")
        return {k: (float(m), int(c)) for k, m, c in zip(_lib.QS_STAGE_NAMES, ms, ln)}


class MapView:
    """The view state of the reference's renderer (MapRenderer.__init__, :383-402): width, height, scale (pixels per
    metre), offset_x / offset_y (screen position of the world origin), with its zoom and pan (:415-430) and the lists of one
    frame in its draw order (:447-468).  scale_limits are the reference's 20..500 by default; a 200 m map needs about
    4 px/m, so they are a parameter."""

    def __init__(self, width=P.VIEW_WIDTH, height=P.VIEW_HEIGHT, scale=P.VIEW_SCALE, offset_x=None, offset_y=None,
                 scale_limits=P.VIEW_SCALE_LIMITS):
        self.width, self.height = int(width), int(height)
        self.scale_limits = (float(scale_limits[0]), float(scale_limits[1]))
        self.scale = float(scale)
        self.offset_x = width / 2 if offset_x is None else offset_x          # :396-397
        self.offset_y = height / 2 if offset_y is None else offset_y

    def zoom(self, factor):
        """The mouse wheel (:417-419): scale *= factor, clamped to scale_limits."""
        self.scale = max(self.scale_limits[0], min(self.scale_limits[1], self.scale * factor))
        return self.scale

    def pan(self, dx, dy):
        """A drag by (dx, dy) pixels (:427-430)."""
        self.offset_x += dx
        self.offset_y += dy

    def world_to_screen(self, wx, wy):                                       # :404-408
        return int(self.offset_x + wx * self.scale), int(self.offset_y - wy * self.scale)

    def _on_screen(self, xy):
        """The reference's test before a cloud point is drawn (:567-568), vectorised: R0 of the points inside the frame."""
        with np.errstate(all="ignore"):
            vx = self.offset_x + xy[:, 0] * self.scale
            vy = self.offset_y - xy[:, 1] * self.scale
            ok = (np.abs(vx) <= 2.0 ** 30) & (np.abs(vy) <= 2.0 ** 30)
            sx, sy = np.trunc(np.where(ok, vx, -9.0)), np.trunc(np.where(ok, vy, -9.0))
        return ok & (sx >= 0) & (sx < self.width) & (sy >= 0) & (sy < self.height)

    def lists(self, zone_boxes=None, point_clouds=None, paths=None, bot_states=None, targets=None, closures=None):
        """(zones, prims) of one frame, in the reference's draw order (:447-468):
          1. zones in bot-id order, colour 'main' (:537-551); a None box is skipped;
          2. per bot (ascending id) and sensor (the clouds' own order) the last 2000 cloud points whose screen point is inside
             the frame (:561, :568), 8 x 8 squares for bot 1 left and bot 2 right (:563-565), single pixels otherwise;
          3. per bot its path ([xs], [ys]) subsampled by max(1, len // 500), as segments in 'path' (:576-589);
          4. target lines from an online bot's state to its target in 'main' (:619-628), then closure lines
             (x1, y1, x2, y2) (:632-637).
        Colours are protocol.bot_colors(bot_id)."""
        zones = []
        for b in sorted(zone_boxes or {}):
            box = zone_boxes[b]
            if box is not None:
                zones.append((tuple(float(v) for v in box), tuple(P.bot_colors(b)["main"]) + (0,), 0))
        chunks = []

        def add(kind, size, color, x0, y0, x1=None, y1=None):
            a = np.zeros(len(x0), dtype=P.VIEW_PRIM_DTYPE)
            a["x0"], a["y0"] = x0, y0
            a["x1"], a["y1"] = (x0 if x1 is None else x1), (y0 if y1 is None else y1)
            a["kind"], a["size"] = kind, size
            a["color"][:, :3] = color
            chunks.append(a)

        for b in sorted(point_clouds or {}):
            colors = P.bot_colors(b)
            for sensor, points in point_clouds[b].items():
                if len(points) == 0:
                    continue
                xy = np.asarray(points[-P.VIEW_CLOUD_RECENT:], dtype=np.float64).reshape(-1, 2)
                xy = xy[self._on_screen(xy)]
                rect = (b == 1 and sensor == "left") or (b == 2 and sensor == "right")
                add(P.VIEW_SQUARE if rect else P.VIEW_POINT, P.VIEW_CLOUD_RECT if rect else 1,
                    colors.get(sensor, (150, 150, 150)), xy[:, 0], xy[:, 1])
        for b in sorted(paths or {}):
            xs, ys = paths[b]
            if len(xs) < 2:
                continue
            step = max(1, len(xs) // P.VIEW_PATH_POINTS)
            x = np.asarray(xs, dtype=np.float64)[::step]
            y = np.asarray(ys, dtype=np.float64)[::step]
            if len(x) >= 2:
                add(P.VIEW_SEGMENT, 1, P.bot_colors(b)["path"], x[:-1], y[:-1], x[1:], y[1:])
        for b, (tx, ty) in (targets or {}).items():
            st = (bot_states or {}).get(b)
            if st and st["online"]:
                add(P.VIEW_SEGMENT, 1, P.bot_colors(b)["main"], [st["x"]], [st["y"]], [tx], [ty])
        for x1, y1, x2, y2 in (closures or ()):
            add(P.VIEW_SEGMENT, 1, P.CLOSURE_LINE_COLOR, [x1], [y1], [x2], [y2])
        return (np.array(zones, dtype=P.VIEW_ZONE_DTYPE).reshape(-1),
                np.concatenate(chunks) if chunks else np.zeros(0, dtype=P.VIEW_PRIM_DTYPE))

    def frame(self, mapper, zone_boxes=None, point_clouds=None, paths=None, bot_states=None, targets=None, closures=None,
              **render_args):
        """One frame of `mapper`'s map under this view with the lists above -> uint8 [height, width, 4]; render_args go to
        QuasarMapper.render_view (colours, draw_occupied, minify, d_out)."""
        zones, prims = self.lists(zone_boxes, point_clouds, paths, bot_states, targets, closures)
        return mapper.render_view(self.width, self.height, self.scale, self.offset_x, self.offset_y, zones=zones, prims=prims,
                                  **render_args)

    @staticmethod
    def save_ppm(path, frame):
        """A frame as a binary PPM (P6): viewable without any imaging library."""
        frame = np.asarray(frame)
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (frame.shape[1], frame.shape[0]))
            f.write(np.ascontiguousarray(frame[:, :, :3]).tobytes())


class OccupancyGrid:
    """Look-alike of dual_bot_mapper.py::OccupancyGrid (:110-237) backed by the device grid.
    `.grid` is synchronised from the GPU on access; attribute names match what MapRenderer
    reads (:494-512)."""

    def __init__(self, size=P.GRID_SIZE, resolution=P.GRID_RESOLUTION,
                 origin_x=P.GRID_ORIGIN_X, origin_y=P.GRID_ORIGIN_Y, device=0):
        m = QuasarMapper(size, resolution, origin_x, origin_y, device=device)
        self._m = m
        self.size, self.res, self.ox, self.oy = size, resolution, origin_x, origin_y

    @classmethod
    def _attached(cls, mapper):
        g = cls.__new__(cls)
        g._m = mapper
        g.size, g.res, g.ox, g.oy = mapper.size, mapper.res, mapper.ox, mapper.oy
        return g

    @property
    def grid(self):
        """np.int8 [size, size], indexed [gy, gx] (:119).  Downloaded from the GPU once per change of the map, not per
        access: the renderer reads occ_grid.grid[gy, gx] cell by cell (:505-516)."""
        v = self._m._map_version
        if getattr(self, "_grid_cache", None) is None or self._grid_cache[0] != v:
            self._grid_cache = (v, self._m.grid_i8())
            self.downloads = getattr(self, "downloads", 0) + 1
        return self._grid_cache[1]

    def world_to_grid(self, wx, wy):                      # :121-125
        gx = int((wx - self.ox) / self.res)
        gy = int((wy - self.oy) / self.res)
        return gx, gy

    def grid_to_world(self, gx, gy):                      # :127-131
        return self.ox + (gx + 0.5) * self.res, self.oy + (gy + 0.5) * self.res

    def in_bounds(self, gx, gy):                          # :133-134
        return 0 <= gx < self.size and 0 <= gy < self.size

    def update_ray(self, robot_x, robot_y, hit_x, hit_y, hit_valid):   # :136-156
        self._m.update_rays([robot_x], [robot_y], [hit_x], [hit_y], [1 if hit_valid else 0])

    def update_rays(self, robot_x, robot_y, hit_x, hit_y, hit_valid):
        self._m.update_rays(robot_x, robot_y, hit_x, hit_y, hit_valid)

    def get_frontiers(self):                              # :181-196
        return [tuple(c) for c in self._m.frontier_cells().tolist()]

    def cluster_frontiers(self, frontier_cells=None, min_cluster=P.FRONTIER_MIN_CLUSTER):     # :198-231
        """Clusters of 4-connected frontier cells with at least FRONTIER_MIN_CLUSTER members, in the reference's cluster
        order (by first cell, row-major), each a list of (gx, gy).  The labelling runs on the device over the current
        grid; `frontier_cells`, if given, must be get_frontiers() of that grid (as main() passes it, :951-952).  Inside a
        cluster the cells come in row-major order, not in the reference's BFS visiting order (nothing reads that order:
        the reference only takes len() and the coordinate sums, :233-237)."""
        mem = self._m.frontier_members()
        if frontier_cells is not None and len(frontier_cells) != len(mem):
            raise ValueError("cluster_frontiers: frontier_cells is not get_frontiers() of the current grid")
        if len(mem) == 0:
            return []
        order = np.argsort(mem[:, 2], kind="stable")                 # by cluster (= by first cell), row-major inside
        roots, start = np.unique(mem[order, 2], return_index=True)
        bounds = list(start) + [len(mem)]
        out = []
        for k in range(len(roots)):
            cells = mem[order[bounds[k]:bounds[k + 1]], :2]
            if len(cells) >= min_cluster:
                out.append([(int(x), int(y)) for x, y in cells])
        return out

    def cluster_centroid_world(self, cluster):                       # :233-237
        avg_x = sum(c[0] for c in cluster) / len(cluster)
        avg_y = sum(c[1] for c in cluster) / len(cluster)
        return self.grid_to_world(avg_x, avg_y)

    def frontier_centroids(self, min_cluster=P.FRONTIER_MIN_CLUSTER):    # :951-956
        return self._m.frontier_centroids(min_cluster)


class _Node:
    __slots__ = ("index", "agent_id")

    def __init__(self, index, agent_id):
        self.index, self.agent_id = index, agent_id


class _NodeList:
    def __init__(self, mapper, graph):
        self._n = mapper.slam_sizes(graph)[0]
        idx, _ = mapper.closures(graph)
        self._agent = dict(zip((int(v) for v in idx[:, 1]), (int(a) for a in mapper.closure_agents(graph))))

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        if i not in self._agent:
            raise KeyError(f"node {i}: only the closing nodes of closures keep their agent_id on the host side")
        return _Node(i, self._agent[i])


class PoseGraphSLAM:
    """Read view of the device pose graph with the reference's attribute names (:267-271)."""

    @classmethod
    def _attached(cls, mapper, graph=0):
        s = cls.__new__(cls)
        s._m, s._g = mapper, graph
        return s

    @property
    def closures(self):
        idx, corr = self._m.closures(self._g)
        return [(int(i[0]), int(i[1]), float(c[0]), float(c[1])) for i, c in zip(idx, corr)]

    @property
    def landmarks(self):
        xy, ti = self._m.landmarks(self._g)
        return [(float(p[0]), float(p[1]), int(t[0]), int(t[1])) for p, t in zip(xy, ti)]

    @property
    def n_nodes(self):
        return self._m.slam_sizes(self._g)[0]

    @property
    def nodes(self):
        """self.nodes (:268) as far as the reference reads it: len(nodes) (:275) and nodes[node_idx].agent_id for the
        closing node of a closure (:335).  The poses themselves stay on the device (qs_last_batch returns a batch's)."""
        return _NodeList(self._m, self._g)

    def add_pose(self, x, y, yaw, agent_id, landmark_type, timestamp=0.0):
        """dual_bot_mapper.py:273-290: returns (closure_detected, correction_dx, correction_dy).  The
        pose is used as given (the caller applies its own drift correction first, :855-857)."""
        closed, corr = self._m.slam_add_poses([x], [y], [agent_id], [landmark_type])
        return bool(closed[0]), float(corr[0, 0]), float(corr[0, 1])

    def get_correction_for_agent(self, agent_id):
        """:328-338: the sum of this agent's closure corrections, i.e. its drift correction."""
        return tuple(float(v) for v in self._m.drift(agent_id))
