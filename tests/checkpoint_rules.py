"""The checkpoint file (include/quasar_slam.h, "checkpoint / restore", format version 1) restated in numpy, for the tests:
an independent reader and writer.  Written from the header's text alone: no ctypes, nothing of the package, nothing of the
device code.

The file, little-endian, every section at an 8-byte aligned offset, in kind order, padded with zero bytes:
  header     0 "QSCK"  4 u32 version  8 u32 header_bytes = 144 + 24 n_sections  12 u32 n_sections  16 u64 total_bytes
            24 u32 crc32 (zlib's) of bytes [header_bytes, total_bytes)  28 u32 reserved
            32 i32 x 12: CONFIG_INTS, reserved   80 f64 x 8: CONFIG_F64   144 table: n_sections x {u32 kind, u32 0, u64 off, u64 len}
  SCALARS    72 bytes: SCALAR_FIELDS
  BOTS       six arrays over the n_bots = max_agent + 1 slots: f64 offset, f64 drift[2], i64 last_closure, u64 zone[4],
             f64 ekf[44], f64 ekf_prev[4]
  COUNTERS   u64[len(CNT_NAMES)]
  GRAPHS     n_graphs x {i64 n_nodes, L, C}, then per graph f64 x[L], y[L], i64 node[L], u8 type[L] (padded to 8),
             i64 landmark[C], node[C], f64 dx[C], dy[C], u8 agent[C] (padded to 8)
  BLOCK_IDS  u32[n_blocks] ascending; block (bx, by) has id by * 32 * pitch + bx
  BLOCKS     per block u32 stamps[64], then u64 counters[64] (enable_counts), then u64 sent[64], fused[64] (and tracking);
             lane = 16 * row + column of the 4 x 16 cells; lanes beyond the grid's edge are 0
  DIRTY      tracking only: u32[blocks_y * pitch]; bit (id % 32) of word (id / 32) is block id

A state is a plain dict:
  config     {name: value} for CONFIG_INTS (the four flags as bool) and CONFIG_F64
  scalars    {name: value} for SCALAR_FIELDS
  bots       {offset [nb], drift [nb, 2], last_closure [nb], zone [nb, 4], ekf [nb, 44], ekf_prev [nb, 4]}
  counters   uint64 [len(CNT_NAMES)]
  graphs     list of {n_nodes, lm_x, lm_y, lm_node, lm_type, cl_landmark, cl_node, cl_dx, cl_dy, cl_agent}
  block_ids  uint32 [n_blocks]
  stamps     uint32 [size, size];  counts, sent, fused: uint64 [size, size], whichever the configuration saves
  dirty      uint32 [words] with tracking, else absent
read(data) returns one (and refuses, with ValueError, whatever breaks the layout above); write(state) is its inverse."""
import struct
import zlib

import numpy as np

MAGIC, VERSION, HEADER_FIXED = b"QSCK", 1, 144
BLOCK_W, BLOCK_H, CELLS = 16, 4, 64                       # QS_DIRTY_BLOCK_W, QS_DIRTY_BLOCK_H
SCALARS, BOTS, COUNTERS, GRAPHS, BLOCK_IDS, BLOCKS, DIRTY = range(1, 8)      # QS_CKPT_*
CONFIG_INTS = ("size", "min_poses_between", "max_agent", "bots_per_graph", "enable_counts", "enable_ekf", "seq_stride",
               "shard_bots", "shard_rank", "exact_trig", "dirty_tracking")
CONFIG_FLAGS = ("enable_counts", "enable_ekf", "exact_trig", "dirty_tracking")
CONFIG_F64 = ("res", "ox", "oy", "min_dist", "max_dist", "closure_radius", "closure_correction", "ekf_metres_per_tick")
SCALAR_FIELDS = ("next_seq", "epoch_base", "n_rebases", "edge_rays", "edge_overflow", "sweep_min", "sweep_max",
                 "dirty_since_fuse", "counts_view_fused", "n_graphs", "n_bots")
_SCALARS = struct.Struct("<5Q2d4I")
assert _SCALARS.size == 72
# the QS_CNT_* enum, in order
CNT_NAMES = ("DATAGRAMS", "ACCEPTED", "RAYS", "CELLS", "HITS", "CLOSURES", "LANDMARKS", "REBASES", "SLAM_WINDOWS", "SLAM_ROUNDS",
             "SLAM_NODE_ITERS", "SLAM_MISC_ITERS", "SLAM_CYCLES", "SLAM_REALTIME", "SLAM_CYC_A", "SLAM_CYC_B", "SLAM_CYC_C",
             "EKF_WRAP_CLAMP", "EDGE_RAYS", "EDGE_OVERFLOW")
BOT_ARRAYS = (("offset", "<f8", 1), ("drift", "<f8", 2), ("last_closure", "<i8", 1), ("zone", "<u8", 4), ("ekf", "<f8", 44),
              ("ekf_prev", "<f8", 4))
LANDMARK_ARRAYS = (("lm_x", "<f8"), ("lm_y", "<f8"), ("lm_node", "<i8"), ("lm_type", "u1"))
CLOSURE_ARRAYS = (("cl_landmark", "<i8"), ("cl_node", "<i8"), ("cl_dx", "<f8"), ("cl_dy", "<f8"), ("cl_agent", "u1"))
PLANES = ("stamps", "counts", "sent", "fused")
# a zone box of a bot without points: the identities of the minimum and the maximum
ZONE_EMPTY = (0xffffffffffffffff, 0xffffffffffffffff, 0, 0)
# the malformed files write() can make, each with a correct CRC (the host checks of qs_restore behind the CRC)
MALFORMED = ("ids_equal", "ids_descending", "id_bx_past_edge", "id_by_past_edge", "ids_length_not_4", "graph_L_gt_N",
             "graph_C_gt_N", "graph_negative", "duplicate_kind", "offset_unaligned", "seven_sections_tracking_off",
             "blocks_one_short")


def _pad8(n):
    return (n + 7) & ~7


def _need(ok, what):
    if not ok:
        raise ValueError("checkpoint: " + what)


# ---- geometry ------------------------------------------------------------------------------------------------------------
def geometry(size):
    """(blocks_x, blocks_y, pitch, words): blocks of 4 rows x 16 columns, bitmap rows of `pitch` 32-bit words."""
    blocks_x, blocks_y = -(-size // BLOCK_W), -(-size // BLOCK_H)
    pitch = -(-blocks_x // 32)
    return blocks_x, blocks_y, pitch, blocks_y * pitch


def block_xy(ids, size):
    """(bx, by) of block ids (any integer array)."""
    pitch = geometry(size)[2]
    ids = np.asarray(ids, dtype=np.int64)
    return ids % (32 * pitch), ids // (32 * pitch)


def _block_cells(ids, size):
    """cells int64 [n, 64] (row-major cell index y * size + x of every lane), inside bool [n, 64]"""
    bx, by = block_xy(ids, size)
    lane = np.arange(CELLS, dtype=np.int64)
    x = bx[:, None] * BLOCK_W + lane[None, :] % BLOCK_W
    y = by[:, None] * BLOCK_H + lane[None, :] // BLOCK_W
    return y * size + x, (x < size) & (y < size)


def block_cells(bid, size):
    """The 64 cell indices (y * size + x) of block `bid` in lane order, and which of them lie inside the grid."""
    cells, inside = _block_cells(np.array([bid]), size)
    return cells[0], inside[0]


def planes_of(config):
    """Names of the planes a checkpoint of this configuration saves."""
    if not config["enable_counts"]:
        return PLANES[:1]
    return PLANES if config["dirty_tracking"] else PLANES[:2]


def block_bytes(n_planes):
    return CELLS * (4 + 8 * (n_planes - 1))


def _block_dtype(names):
    return np.dtype([(n, "<u4" if n == "stamps" else "<u8", (CELLS,)) for n in names])


def n_graphs_of(config):
    per = config["bots_per_graph"] if config["bots_per_graph"] > 0 else config["max_agent"]
    return -(-config["max_agent"] // per)


def dirty_bits(dirty, size):
    """bool [blocks_y, blocks_x]: the valid bits of a dirty bitmap."""
    blocks_x, blocks_y, pitch, words = geometry(size)
    d = np.asarray(dirty, dtype=np.uint32).reshape(blocks_y, pitch)
    bits = (d[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(blocks_y, pitch * 32)[:, :blocks_x].astype(bool)


def bitmap_of(bits, size):
    """The inverse of dirty_bits: uint32 [words] with the padding bits clear."""
    blocks_x, blocks_y, pitch, words = geometry(size)
    full = np.zeros((blocks_y, pitch * 32), dtype=np.uint64)
    full[:, :blocks_x] = np.asarray(bits, dtype=bool)
    w = (full.reshape(blocks_y, pitch, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2)
    return w.astype(np.uint32).reshape(-1)


def expected_ids(planes, dirty, size):
    """Ascending ids of every block in which any of `planes` (full-grid arrays) is nonzero, or whose valid dirty bit is set
    (dirty: the bitmap words, or None)."""
    blocks_x, blocks_y, pitch, words = geometry(size)
    any_nz = np.zeros((blocks_y * BLOCK_H, blocks_x * BLOCK_W), dtype=bool)
    for p in planes:
        any_nz[:size, :size] |= np.asarray(p).reshape(size, size) != 0
    held = any_nz.reshape(blocks_y, BLOCK_H, blocks_x, BLOCK_W).any(axis=(1, 3))
    if dirty is not None:
        held |= dirty_bits(dirty, size)
    by, bx = np.nonzero(held)                               # row-major: ascending ids
    return (by * 32 * pitch + bx).astype(np.uint32)


# ---- the orderable words of a zone box --------------------------------------------------------------------------------
def zone_words(values):
    """f64 -> the u64 that orders as the number does: the bits, inverted if the sign bit is set, else with the sign bit set."""
    b = np.asarray(values, dtype="<f8").view("<u8")
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def zone_values(words):
    k = np.asarray(words, dtype="<u8")
    b = np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k)
    return b.astype("<u8").view("<f8")


# ---- reader ---------------------------------------------------------------------------------------------------------------
def read(data):
    """bytes -> state (see the module text); ValueError for whatever is not a version-1 checkpoint."""
    buf = bytes(memoryview(data).cast("B"))
    _need(len(buf) >= HEADER_FIXED, "truncated header")
    magic, version, hb, n_sec, total, crc, reserved = struct.unpack_from("<4sIIIQII", buf, 0)
    _need(magic == MAGIC, "bad magic")
    _need(version == VERSION, f"unknown version {version}")
    _need(n_sec in (6, 7) and hb == HEADER_FIXED + 24 * n_sec and len(buf) >= hb, "bad header or section table")
    _need(total == len(buf), f"length {len(buf)} against the header's {total}")
    _need(zlib.crc32(buf[hb:]) == crc, "CRC mismatch")
    _need(reserved == 0, "reserved header word is not 0")
    vals = struct.unpack_from("<12i8d", buf, 32)
    _need(vals[11] == 0, "reserved configuration word is not 0")
    config = dict(zip(CONFIG_INTS, vals[:11]))
    config.update(zip(CONFIG_F64, vals[12:]))
    for k in CONFIG_FLAGS:
        _need(config[k] in (0, 1), f"flag {k} is {config[k]}")
        config[k] = bool(config[k])
    tracking, size = config["dirty_tracking"], config["size"]
    _need(n_sec == (7 if tracking else 6), "the DIRTY section goes with dirty_tracking")
    _need(size >= 4 and size % 4 == 0, f"size {size}")
    # sections: kind order, 8-byte aligned, back to back from the header to the end, zero padding
    off, length = {}, {}
    at = hb
    for i in range(n_sec):
        kind, zero, o, n = struct.unpack_from("<IIQQ", buf, HEADER_FIXED + 24 * i)
        _need(kind == i + 1, f"section table entry {i} has kind {kind}")
        _need(zero == 0, f"section table entry {i}: reserved word")
        _need(o % 8 == 0, f"section {kind} at the unaligned offset {o}")
        _need(o == at and n <= total - o, f"section {kind}: offset {o} length {n} (expected offset {at})")
        _need(not any(buf[o + n:o + _pad8(n)]), f"section {kind}: padding is not zero")
        off[kind], length[kind] = o, n
        at = o + _pad8(n)
    _need(at == total, "the sections do not fill the file")

    def arr(o, dtype, count):
        return np.frombuffer(buf, dtype=dtype, count=count, offset=o).copy()

    _need(length[SCALARS] == _SCALARS.size, "bad scalars section")
    scalars = dict(zip(SCALAR_FIELDS, _SCALARS.unpack_from(buf, off[SCALARS])))
    nb, G = scalars["n_bots"], scalars["n_graphs"]
    _need(nb == config["max_agent"] + 1, "n_bots is not max_agent + 1")
    _need(G == n_graphs_of(config), "n_graphs does not follow from max_agent and bots_per_graph")
    _need(length[BOTS] == nb * 8 * sum(w for _, _, w in BOT_ARRAYS), "bad bots section")
    bots, o = {}, off[BOTS]
    for name, dt, w in BOT_ARRAYS:
        a = arr(o, dt, nb * w)
        bots[name] = a if w == 1 else a.reshape(nb, w)
        o += 8 * nb * w
    _need(length[COUNTERS] == 8 * len(CNT_NAMES), "bad counters section")
    counters = arr(off[COUNTERS], "<u8", len(CNT_NAMES))
    # graphs
    _need(length[GRAPHS] >= 24 * G, "truncated graphs section")
    sizes = arr(off[GRAPHS], "<i8", 3 * G).reshape(G, 3)
    graphs, o = [], off[GRAPHS] + 24 * G
    end = off[GRAPHS] + length[GRAPHS]
    for g in range(G):
        N, L, C = (int(v) for v in sizes[g])
        _need(N >= 0 and 0 <= L <= N and 0 <= C <= N, f"bad sizes of graph {g}: {N} nodes, {L} landmarks, {C} closures")
        _need(o + 24 * L + _pad8(L) + 32 * C + _pad8(C) <= end, f"graph {g} runs past its section")
        gr = {"n_nodes": N}
        for arrays, n in ((LANDMARK_ARRAYS, L), (CLOSURE_ARRAYS, C)):
            for name, dt in arrays:
                gr[name] = arr(o, dt, n)
                o += n * np.dtype(dt).itemsize
            _need(not any(buf[o:o - n + _pad8(n)]), f"graph {g}: byte array padding is not zero")
            o += _pad8(n) - n
        graphs.append(gr)
    _need(o == end, "the graphs do not fill their section")
    # blocks
    blocks_x, blocks_y, pitch, words = geometry(size)
    _need(length[BLOCK_IDS] % 4 == 0, "BLOCK_IDS length is no multiple of 4")
    n_blk = length[BLOCK_IDS] // 4
    ids = arr(off[BLOCK_IDS], "<u4", n_blk)
    _need((np.diff(ids.astype(np.int64)) > 0).all(), "block ids are not ascending")
    bx, by = block_xy(ids, size)
    _need((bx < blocks_x).all() and (by < blocks_y).all(), "a block id lies outside the grid")
    names = planes_of(config)
    _need(length[BLOCKS] == n_blk * block_bytes(len(names)), "BLOCKS length does not match the block list")
    rec = np.frombuffer(buf, dtype=_block_dtype(names), count=n_blk, offset=off[BLOCKS])
    cells, inside = _block_cells(ids, size)
    state = {"config": config, "scalars": scalars, "bots": bots, "counters": counters, "graphs": graphs, "block_ids": ids}
    for name in names:
        v = rec[name]
        _need(not v[~inside].any(), f"{name}: a cell beyond the grid's edge is not 0")
        plane = np.zeros(size * size, dtype=v.dtype)
        plane[cells[inside]] = v[inside]
        state[name] = plane.reshape(size, size)
    if tracking:
        _need(length[DIRTY] == 4 * words, "bad dirty section")
        state["dirty"] = arr(off[DIRTY], "<u4", words)
    return state


# ---- writer ---------------------------------------------------------------------------------------------------------------
def write(state, malformed=None):
    """state -> bytes.  Without "block_ids" the blocks are expected_ids of the planes and the bitmap; with it, exactly the
    listed blocks are written (a listed block may be all zero; what the planes hold elsewhere is not written).
    malformed: one of MALFORMED -- that one thing is wrong, everything else and the CRC are right."""
    assert malformed is None or malformed in MALFORMED, malformed
    config, size = state["config"], state["config"]["size"]
    tracking = bool(config["dirty_tracking"])
    blocks_x, blocks_y, pitch, words = geometry(size)
    names = planes_of(config)
    dirty = np.asarray(state["dirty"], dtype="<u4") if tracking else None
    ids = state.get("block_ids")
    if ids is None:
        ids = expected_ids([state[n] for n in names], dirty, size)
    ids = np.asarray(ids, dtype="<u4").copy()
    cells, inside = _block_cells(ids, size)                 # (what is written: the blocks as listed before any damage)
    rec = np.zeros(len(ids), dtype=_block_dtype(names))
    for name in names:
        flat = np.asarray(state[name]).reshape(-1)
        rec[name][inside] = flat[cells[inside]]
    if malformed in ("ids_equal", "ids_descending"):
        assert len(ids) >= 2
        ids[:2] = (ids[0], ids[0]) if malformed == "ids_equal" else (ids[1], ids[0])
    elif malformed == "id_bx_past_edge":                    # the first padding bit of the last listed block's bitmap row
        assert len(ids) >= 1 and blocks_x % 32 != 0
        ids[-1] = ids[-1] // (32 * pitch) * (32 * pitch) + blocks_x
    elif malformed == "id_by_past_edge":
        assert len(ids) >= 1
        ids[-1] = blocks_y * 32 * pitch
    ids_bytes = ids.tobytes() + (b"\0\0" if malformed == "ids_length_not_4" else b"")
    blocks_bytes = rec.tobytes()
    if malformed == "blocks_one_short":
        assert len(ids) >= 1
        blocks_bytes = blocks_bytes[:-block_bytes(len(names))]
    sc = dict(state["scalars"])
    scalars = _SCALARS.pack(*(sc[k] for k in SCALAR_FIELDS))
    nb = sc["n_bots"]
    bots = b"".join(np.asarray(state["bots"][name], dtype=dt).reshape(nb * w).tobytes() for name, dt, w in BOT_ARRAYS)
    counters = np.asarray(state["counters"], dtype="<u8").tobytes()
    assert len(counters) == 8 * len(CNT_NAMES)
    head, logs = b"", b""
    for g, gr in enumerate(state["graphs"]):
        gr = dict(gr)
        N, L, C = gr["n_nodes"], len(gr["lm_x"]), len(gr["cl_node"])
        if g == 0 and malformed == "graph_L_gt_N":
            assert L >= 1
            N = L - 1
        elif g == 0 and malformed == "graph_C_gt_N":
            assert C >= 1 and L < C
            N = C - 1
        elif g == 0 and malformed == "graph_negative":     # the closure log is left out and its length stated as -1
            C = 0
        for arrays, n in ((LANDMARK_ARRAYS, L), (CLOSURE_ARRAYS, C)):
            for name, dt in arrays:
                a = np.asarray(gr[name], dtype=dt)[:n]
                assert len(a) == n, name
                logs += a.tobytes()
            logs += bytes(_pad8(n) - n)
        head += struct.pack("<3q", N, L, -1 if g == 0 and malformed == "graph_negative" else C)
    sections = [(SCALARS, scalars), (BOTS, bots), (COUNTERS, counters), (GRAPHS, head + logs), (BLOCK_IDS, ids_bytes),
                (BLOCKS, blocks_bytes)]
    if tracking or malformed == "seven_sections_tracking_off":
        sections.append((DIRTY, dirty.tobytes() if tracking else bytes(4 * words)))
    hb = HEADER_FIXED + 24 * len(sections)
    body, table = b"", []
    for kind, payload in sections:
        table.append([kind, 0, hb + len(body), len(payload)])
        body += payload + bytes(_pad8(len(payload)) - len(payload))
    if malformed == "duplicate_kind":
        table[COUNTERS - 1][0] = BOTS
    elif malformed == "offset_unaligned":
        table[COUNTERS - 1][2] += 4
    ints = [int(config[k]) for k in CONFIG_INTS] + [0]
    out = struct.pack("<4sIIIQII", MAGIC, VERSION, hb, len(sections), hb + len(body), zlib.crc32(body), 0)
    out += struct.pack("<12i8d", *ints, *(float(config[k]) for k in CONFIG_F64))
    out += b"".join(struct.pack("<IIQQ", *t) for t in table)
    assert len(out) == hb
    return out + body


# ---- states for the tests -----------------------------------------------------------------------------------------------
def empty_state(config, n_nodes=0):
    """What a context of this configuration holds after its creation: no writes, no poses; bots without zone boxes."""
    config = dict(config)
    size, nb, G = config["size"], config["max_agent"] + 1, n_graphs_of(config)
    st = {"config": config,
          "scalars": dict(next_seq=0, epoch_base=0, n_rebases=0, edge_rays=0, edge_overflow=0, sweep_min=0.0, sweep_max=0.0,
                          dirty_since_fuse=0, counts_view_fused=0, n_graphs=G, n_bots=nb),
          "bots": {name: np.zeros(nb if w == 1 else (nb, w), dtype=dt) for name, dt, w in BOT_ARRAYS},
          "counters": np.zeros(len(CNT_NAMES), dtype="<u8"),
          "graphs": [dict({name: np.zeros(0, dtype=dt) for name, dt in LANDMARK_ARRAYS + CLOSURE_ARRAYS}, n_nodes=n_nodes)
                     for _ in range(G)]}
    st["bots"]["zone"][:] = np.array(ZONE_EMPTY, dtype="<u8")
    for name in planes_of(config):
        st[name] = np.zeros((size, size), dtype="<u4" if name == "stamps" else "<u8")
    if config["dirty_tracking"]:
        st["dirty"] = np.zeros(geometry(size)[3], dtype="<u4")
    return st


def same_state(a, b):
    """None if two states are equal bit for bit, else the path of the first difference."""
    def walk(x, y, path):
        if isinstance(x, dict):
            if not isinstance(y, dict) or x.keys() != y.keys():
                return path + ": keys"
            for k in x:
                d = walk(x[k], y[k], f"{path}.{k}")
                if d:
                    return d
            return None
        if isinstance(x, (list, tuple)):
            if len(x) != len(y):
                return path + ": length"
            for i, (p, q) in enumerate(zip(x, y)):
                d = walk(p, q, f"{path}[{i}]")
                if d:
                    return d
            return None
        p, q = np.asarray(x), np.asarray(y)
        if p.shape != q.shape or p.dtype.kind != q.dtype.kind or p.dtype.itemsize != q.dtype.itemsize:
            return f"{path}: {p.dtype}{p.shape} against {q.dtype}{q.shape}"
        return None if p.tobytes() == q.tobytes() else path + ": values"
    return walk(a, b, "state")
