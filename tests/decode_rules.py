"""CPU restatement of the packet decoder's rules (csrc/decode.hip, K0; dual_bot_mapper.py:826-857), byte by byte, for the tests.

Plain numpy / struct over the caller's bytes: no ctypes, no oracle, nothing of the device.  A record is accepted when
  * its length is exactly 42 (v2) or 41 (v1) and not above the stride (the length is the stride when there are no lengths),
  * its first four bytes are 'QSRL',
  * 1 <= agent (byte 4) <= max_agent,
  * x, y and yaw (little-endian f32 at bytes 5, 9, 13) are finite.
Its fields: px = f64(x) + offset[agent] (one fp64 add), py = f64(y), yaw = f64(yaw), enc = i32 at byte 17, the four distances
f32 at bytes 25, 29, 33, 37, and the landmark type = byte 41 of a 42-byte record, 0 for a 41-byte one whatever byte follows
it.  The layout is protocol.PACKET_FMT / PACKET_FMT_V1 ('<4sBfffiIffffB', packed).

Also here: the builder of test buffers (any stride, padding of random non-zero bytes), the (mis, sh) arithmetic of the
staging kernel, and the record pool the decoder tests draw from."""
import struct

import numpy as np

FMT_V2, FMT_V1 = "<4sBfffiIffffB", "<4sBfffiIffff"
SIZE_V2, SIZE_V1 = struct.calcsize(FMT_V2), struct.calcsize(FMT_V1)
assert (SIZE_V2, SIZE_V1) == (42, 41)
MAGIC = b"QSRL"
# the device's launch shape (decode.hip): records per tile, tiles per workgroup, widest stride of the LDS-staged kernel
TILE, TILES_PER_WG, MAX_LDS_STRIDE = 256, 8, 64
WG = TILE * TILES_PER_WG


def decode_one(datagram, max_agent, offsets):
    """One datagram (bytes of its true length) by struct: None if dropped, else (agent, lm, px, py, yaw, dist[4], enc)."""
    if len(datagram) == SIZE_V2:
        magic, agent, x, y, yaw, enc, _, d0, d1, d2, d3, lm = struct.unpack(FMT_V2, datagram)
    elif len(datagram) == SIZE_V1:
        magic, agent, x, y, yaw, enc, _, d0, d1, d2, d3 = struct.unpack(FMT_V1, datagram)
        lm = 0
    else:
        return None
    if magic != MAGIC or not 1 <= agent <= max_agent:
        return None
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(yaw)):
        return None
    # struct hands back the f32 widened to a Python float (= f64): the add is the one fp64 add of :851-852
    return agent, lm, x + float(offsets[agent]), y, yaw, np.array([d0, d1, d2, d3], dtype=np.float32), enc


def _f32(rec, off):
    return np.ascontiguousarray(rec[:, off:off + 4]).view("<f4").reshape(-1)


def decode(buf_bytes, n, stride, lens, max_agent, offsets):
    """n records, record k at byte k * stride of buf_bytes; lens: uint16 [n] or None (every length == stride);
    offsets: float64 [max_agent + 1] (the bots' x offsets, index = agent).  Returns a dict of arrays, one entry per record:
    accept uint8, agent uint8, lm uint8, px / py / yaw float64, dist float32 [n, 4], enc int32.  The fields of a dropped record
    are 0 (NaN for the pose)."""
    raw = np.frombuffer(memoryview(buf_bytes).cast("B"), dtype=np.uint8, count=n * stride).reshape(n, stride)
    length = np.full(n, stride, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.uint16).astype(np.int64)
    assert len(length) == n
    len_ok = ((length == SIZE_V2) | (length == SIZE_V1)) & (length <= stride)
    # the bytes a rule may look at: a record's first `length` ones.  A row of 42 with everything else zeroed.
    rec = np.zeros((n, SIZE_V2), dtype=np.uint8)
    w = min(stride, SIZE_V2)
    rec[:, :w] = raw[:, :w]
    rec[np.arange(SIZE_V2)[None, :] >= length[:, None]] = 0
    agent = rec[:, 4].astype(np.int64)
    x, y, yaw = _f32(rec, 5), _f32(rec, 9), _f32(rec, 13)
    with np.errstate(invalid="ignore"):
        accept = (len_ok & (rec[:, :4] == np.frombuffer(MAGIC, dtype=np.uint8)).all(axis=1)
                  & (agent >= 1) & (agent <= max_agent) & np.isfinite(x) & np.isfinite(y) & np.isfinite(yaw))
    off = np.asarray(offsets, dtype=np.float64)
    a_idx = np.where(accept, agent, 0)
    nan = np.float64("nan")
    with np.errstate(invalid="ignore"):
        px = np.where(accept, x.astype(np.float64) + off[a_idx], nan)
    out = dict(accept=accept.astype(np.uint8), agent=np.where(accept, agent, 0).astype(np.uint8),
               lm=np.where(accept & (length == SIZE_V2), rec[:, 41], 0).astype(np.uint8),
               px=px, py=np.where(accept, y.astype(np.float64), nan), yaw=np.where(accept, yaw.astype(np.float64), nan),
               dist=np.stack([_f32(rec, o) for o in (25, 29, 33, 37)], axis=1),
               enc=np.where(accept, np.ascontiguousarray(rec[:, 17:21]).view("<i4").reshape(-1), 0).astype(np.int32))
    out["dist"][~accept] = 0
    return out


def pose_as_reported(ref, drift_x=0.0, drift_y=0.0):
    """float64 [n, 3]: the pose qs_last_batch reports, px + drift_x, py + drift_y, yaw (:855-857: one fp64 add each on x and y
    even when the drift is 0.0, which turns a y of -0.0 into +0.0, in CPython as on the device); NaN for dropped records."""
    return np.stack([ref["px"] + drift_x, ref["py"] + drift_y, ref["yaw"]], axis=1)


def build(records, stride, pad_byte_rng, head=0, tail=0, slack_record=None):
    """Lay record k (bytes; cut to the stride if longer) at byte head + k * stride of a fresh uint8 array of
    head + n * stride + tail bytes and fill ALL padding after the records with random NON-ZERO bytes.  head / tail: slack
    before and after the n * stride range; with slack_record (a well-formed 42-byte record) the slack holds copies of it on
    the records' own stride lattice (records -1, -2, ... and n, n + 1, ...), so that a decoder that is off by a record, or
    reads into a neighbour, finds something it would accept.  Returns (array, lens uint16 [n]): the records' true lengths."""
    n = len(records)
    out = pad_byte_rng.integers(1, 256, head + n * stride + tail, dtype=np.uint8)
    if slack_record is not None:
        cell = out[:stride].copy()
        m = min(len(slack_record), stride)
        cell[:m] = np.frombuffer(slack_record[:m], dtype=np.uint8)
        reps = max(head, tail) // stride + 2
        if head:
            out[:head] = np.tile(cell, reps)[-head:]
        if tail:
            out[head + n * stride:] = np.tile(cell, reps)[:tail]
    lens = np.zeros(n, dtype=np.uint16)
    body = out[head:head + n * stride].reshape(n, stride) if n else None
    for k, r in enumerate(records):
        m = min(len(r), stride)
        body[k, :m] = np.frombuffer(r[:m], dtype=np.uint8)
        lens[k] = len(r)
    return out, lens


def shifts(addr, n, stride):
    """The set of (mis, sh) the LDS-staged kernel computes for n records at byte address addr: per tile of 256 records
    mis = (addr + tile_base * stride) & 3, and per record of the tile sh = (mis + tid * stride) & 3 (decode.hip)."""
    out = set()
    for base in range(0, n, TILE):
        mis = (addr + base * stride) & 3
        for tid in range(min(TILE, n - base)):
            out.add((mis, (mis + tid * stride) & 3))
    return out


def bytewise_tiles(addr, n, stride):
    """The tiles whose staged dword range reaches outside [addr, addr + n * stride): the kernel's bytewise branch."""
    out = []
    end = addr + n * stride
    for base in range(0, n, TILE):
        a0 = addr + base * stride
        mis = a0 & 3
        nrec = min(TILE, n - base)
        ndw = (mis + nrec * stride + 3) // 4
        if a0 - mis < addr or a0 - mis + 4 * ndw > end:
            out.append(base // TILE)
    return out


# ---- the record pool -----------------------------------------------------------------------------------------------------------
F32_SPECIALS = [np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(1e-42), np.float32(-0.0)]
ENC_SPECIALS = [-2 ** 31, -1, 2 ** 31 - 1]
LM_BYTES = [0, 1, 2, 3, 4, 5, 7, 255]
ODD_LENGTHS = [0, 20, 40, 43, 48]


def make_pool(base42, rng, max_agent, n, reject_share=0.27, landmarks=True, odd_lengths=True):
    """n records (a list of bytes, v2 unless mutated) drawn from the 42-byte records base42 (uint8 [m, 42], agents within
    1..max_agent, poses within +-20 m) and mutated by a seeded rng:
      dropped ones (about reject_share of them): bad magic; agent 0, max_agent + 1 (if <= 255) and 255 (if > max_agent); NaN,
        +inf or -inf in x, y or yaw; with odd_lengths also a length of 0, 20, 40, 43 or 48;
      kept ones: v1 truncation; agent max_agent; all-zero distances; NaN, +-inf, a denormal or -0.0 in any distance; a
        denormal or -0.0 in x, y or yaw; enc INT32_MIN, -1, INT32_MAX; landmark bytes 0..5, 7, 255 (landmarks=False: every
        landmark byte 0, for runs that must not close a loop)."""
    dt = np.dtype([("magic", "S4"), ("agent", "u1"), ("x", "<f4"), ("y", "<f4"), ("yaw", "<f4"), ("enc", "<i4"), ("v2v", "<u4"),
                   ("d", "<f4", (4,)), ("lm", "u1")])
    assert dt.itemsize == SIZE_V2
    rec = np.ascontiguousarray(base42[rng.integers(0, len(base42), n)]).view(dt).reshape(-1).copy()
    if not landmarks:
        rec["lm"] = 0
    drop_kinds = ["magic", "agent0", "agent_hi", "agent255", "nan_pose"] + (["length"] if odd_lengths else [])
    if max_agent == 255:
        drop_kinds = [k for k in drop_kinds if k not in ("agent_hi", "agent255")]
    length = np.full(n, SIZE_V2, dtype=np.int64)
    dropped = rng.random(n) < reject_share
    for k in range(n):
        if dropped[k]:
            kind = drop_kinds[int(rng.integers(len(drop_kinds)))]
            if kind == "magic":
                m = bytearray(MAGIC)
                m[int(rng.integers(4))] ^= 1 << int(rng.integers(8))
                rec["magic"][k] = bytes(m)
            elif kind == "agent0":
                rec["agent"][k] = 0
            elif kind == "agent_hi":
                rec["agent"][k] = max_agent + 1
            elif kind == "agent255":
                rec["agent"][k] = 255
            elif kind == "nan_pose":
                rec[("x", "y", "yaw")[int(rng.integers(3))]][k] = F32_SPECIALS[int(rng.integers(3))]
            else:
                length[k] = ODD_LENGTHS[int(rng.integers(len(ODD_LENGTHS)))]
            continue
        u = rng.random()
        if u < 0.12:
            length[k] = SIZE_V1
        elif u < 0.16:
            rec["agent"][k] = max_agent
        elif u < 0.20:
            rec["d"][k] = 0.0
        elif u < 0.32:
            rec["d"][k, int(rng.integers(4))] = F32_SPECIALS[int(rng.integers(5))]
        elif u < 0.38:
            rec[("x", "y", "yaw")[int(rng.integers(3))]][k] = F32_SPECIALS[3 + int(rng.integers(2))]
        elif u < 0.46:
            rec["enc"][k] = ENC_SPECIALS[int(rng.integers(3))]
        elif u < 0.58 and landmarks:
            rec["lm"][k] = LM_BYTES[int(rng.integers(len(LM_BYTES)))]
    raw = rec.view(np.uint8).reshape(n, SIZE_V2)
    out = []
    for k in range(n):
        L = int(length[k])
        b = raw[k].tobytes()
        out.append(b[:L] if L <= SIZE_V2 else b + bytes(rng.integers(1, 256, L - SIZE_V2, dtype=np.uint8)))
    return out


def fit(records, stride, with_lens):
    """The pool as a buffer of this stride can carry it.  With lengths: a record longer than the stride keeps its first 42
    bytes (a length the stride does not allow is not used).  Without: every record must have 41 bytes or more (a pool made
    with odd_lengths=False) and is cut to the stride; build() pads a shorter one, and its length is then the stride."""
    if with_lens:
        assert stride >= SIZE_V2
        return [r if len(r) <= stride else r[:SIZE_V2] for r in records]
    assert stride in (SIZE_V1, SIZE_V2) and all(len(r) >= SIZE_V1 for r in records)
    return [r[:stride] for r in records]


def datagrams(buf, n, stride, lens, head=0):
    """What build() laid down, as the datagrams a receiver would have seen: record k's first lens[k] (or stride) bytes."""
    b = np.asarray(buf, dtype=np.uint8)[head:head + n * stride].reshape(n, stride)
    return [b[k, :(stride if lens is None else min(int(lens[k]), stride))].tobytes() for k in range(n)]
