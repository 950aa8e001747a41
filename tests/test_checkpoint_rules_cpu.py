"""tests/checkpoint_rules.py checked without a GPU: its geometry against a double loop over cells, its writer against its
reader on random states, its reader against the package's own header reader, and every malformed file its writer can make
against its reader."""
import re

import numpy as np
import pytest

import checkpoint_rules as ck
from conftest import load_pkg

SIZES = (4, 20, 200, 512, 516, 1040, 2052)
BASE = dict(size=20, min_poses_between=30, max_agent=10, bots_per_graph=2, enable_counts=True, enable_ekf=True, seq_stride=1,
            shard_bots=0, shard_rank=0, exact_trig=True, dirty_tracking=False, res=0.05, ox=-0.5, oy=-0.5, min_dist=0.05,
            max_dist=1.2, closure_radius=0.6, closure_correction=0.5, ekf_metres_per_tick=0.0107)
LOG_LENGTHS = (0, 1, 7, 8, 9)                               # the byte arrays are padded to 8


def _config(size, n_planes, dirty):
    """n_planes 1: no counters; 2: counters; 4: counters and tracking.  dirty without counters: tracking, one plane."""
    return dict(BASE, size=size, enable_counts=n_planes >= 2, dirty_tracking=bool(dirty))


def random_state(rng, config, lengths=LOG_LENGTHS):
    st = ck.empty_state(config)
    size, nb = config["size"], config["max_agent"] + 1
    u64 = lambda shape=None: rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    st["scalars"].update(next_seq=int(u64()), epoch_base=int(u64()), n_rebases=int(u64()), edge_rays=int(u64()),
                         edge_overflow=int(u64()), sweep_min=float(rng.uniform(0, 1)), sweep_max=float(rng.uniform(1, 2)),
                         dirty_since_fuse=int(rng.integers(0, 2)), counts_view_fused=int(rng.integers(0, 2)))
    for name, dt, w in ck.BOT_ARRAYS:
        shape = nb if w == 1 else (nb, w)
        st["bots"][name] = u64(shape).astype("<u8") if dt == "<u8" else u64(shape).view(dt)      # any bits, NaN included
    st["counters"] = u64(len(ck.CNT_NAMES))
    for g, gr in enumerate(st["graphs"]):
        L, C = lengths[g % len(lengths)], lengths[(g + 2) % len(lengths)]
        gr["n_nodes"] = max(L, C) + int(rng.integers(0, 5))
        for arrays, n in ((ck.LANDMARK_ARRAYS, L), (ck.CLOSURE_ARRAYS, C)):
            for name, dt in arrays:
                gr[name] = rng.integers(1, 256, n).astype(dt) if dt == "u1" else u64(n).view(dt)
    for name in ck.planes_of(config):
        plane = u64((size, size)).astype(st[name].dtype)
        plane[rng.random((size, size)) < 0.9] = 0           # most cells empty: some blocks are left out
        st[name] = plane
    if config["dirty_tracking"]:
        st["dirty"] = ck.bitmap_of(rng.random(ck.geometry(size)[:2][::-1]) < 0.3, size)
    return st


# ---- geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_geometry_and_block_cells_against_a_loop_over_cells(size):
    blocks_x, blocks_y, pitch, words = ck.geometry(size)
    # the block of every cell, cell by cell: (x // 16, y // 4), and rows of whole 32-bit words that hold blocks_x bits
    owner = {}
    for y in range(size):
        for x in range(size):
            owner.setdefault((x // 16, y // 4), []).append(y * size + x)
    assert blocks_x == 1 + max(bx for bx, _ in owner) and blocks_y == 1 + max(by for _, by in owner)
    assert 32 * (pitch - 1) < blocks_x <= 32 * pitch and words == blocks_y * pitch
    rng = np.random.default_rng(size)
    some = set(map(tuple, rng.integers(0, (blocks_x, blocks_y), (40, 2)).tolist()))
    some |= {(0, 0), (blocks_x - 1, 0), (0, blocks_y - 1), (blocks_x - 1, blocks_y - 1), (min(31, blocks_x - 1), 0),
             (min(32, blocks_x - 1), blocks_y // 2)}
    for bx, by in some:
        bid = by * 32 * pitch + bx
        cells, inside = ck.block_cells(bid, size)
        assert cells.shape == (64,) and inside.shape == (64,)
        assert sorted(cells[inside].tolist()) == owner[(bx, by)], (bx, by)
        for lane in range(64):                              # lane = 16 * row + column
            x, y = 16 * bx + lane % 16, 4 * by + lane // 16
            assert bool(inside[lane]) == (x < size and y < size)
            if inside[lane]:
                assert cells[lane] == y * size + x
        assert tuple(int(v[0]) for v in ck.block_xy([bid], size)) == (bx, by)
    # every cell lies in exactly one block of the id space
    all_ids = np.array([by * 32 * pitch + bx for by in range(blocks_y) for bx in range(blocks_x)])
    cells, inside = ck._block_cells(all_ids, size)
    assert sorted(cells[inside].tolist()) == list(range(size * size))


@pytest.mark.parametrize("size", (4, 20, 516))
def test_expected_ids_and_bitmap(size):
    blocks_x, blocks_y, pitch, words = ck.geometry(size)
    rng = np.random.default_rng(size + 1)
    plane = np.zeros((size, size), dtype=np.uint32)
    want = set()
    for _ in range(12):
        x, y = (int(v) for v in rng.integers(0, size, 2))
        plane[y, x] = 7
        want.add((y // 4) * 32 * pitch + x // 16)
    assert ck.expected_ids([plane], None, size).tolist() == sorted(want)
    bits = rng.random((blocks_y, blocks_x)) < 0.2
    bm = ck.bitmap_of(bits, size)
    assert bm.shape == (words,) and (ck.dirty_bits(bm, size) == bits).all()
    for by, bx in zip(*np.nonzero(bits)):
        bid = int(by) * 32 * pitch + int(bx)
        assert bm[bid // 32] >> (bid % 32) & 1
        want.add(bid)
    assert int(sum(bin(int(w)).count("1") for w in bm)) == int(bits.sum())
    noisy = bm.copy()                                       # padding bits set: they are no blocks
    if blocks_x % 32:
        noisy = noisy.reshape(blocks_y, pitch)
        noisy[:, -1] |= np.uint32(1 << (blocks_x % 32))
        noisy = noisy.reshape(-1)
    assert ck.expected_ids([plane], noisy, size).tolist() == sorted(want)


def test_zone_words_order_as_the_numbers_do():
    v = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-300, 2.0, np.inf])
    w = ck.zone_words(v)
    assert (np.diff(w.astype(object)) > 0).all()
    assert ck.zone_values(w).tobytes() == v.tobytes()
    assert all(int(a) > int(w[-1]) for a in ck.ZONE_EMPTY[:2]) and all(int(a) < int(w[0]) for a in ck.ZONE_EMPTY[2:])


def test_counter_names_are_the_header_enum():
    from importlib import import_module
    with open(import_module(load_pkg().__name__ + "._lib").HEADER) as f:
        txt = f.read()
    body = re.search(r"enum \{ (QS_CNT_DATAGRAMS.*?QS_CNT_N) \};", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.S).group(1)
    names = [n.split("=")[0].strip() for n in body.split(",")]
    assert names == ["QS_CNT_" + n for n in ck.CNT_NAMES] + ["QS_CNT_N"]
    kinds = re.search(r"enum \{ (QS_CKPT_SCALARS.*?) \};", txt).group(1)
    assert [k.split("=")[0].strip() for k in kinds.split(",")] == ["QS_CKPT_" + n for n in ("SCALARS", "BOTS", "COUNTERS", "GRAPHS",
                                                                                          "BLOCK_IDS", "BLOCKS", "DIRTY")]
    assert (ck.SCALARS, ck.DIRTY) == (1, 7)


# ---- a file packed by hand -----------------------------------------------------------------------------------------------
def _hand_packed():
    """A 20 x 20 checkpoint with counters and tracking, packed here with struct, field by field as the header lists them
    (nothing of the rules' writer), and the state it holds.  Blocks 1 = (bx 1, by 0), whose columns 20..31 lie beyond the
    edge, 96 = (0, 3) and 129 = (1, 4), which is dirty and holds nothing."""
    import struct
    import zlib
    size, nb = 20, 3
    cfg = dict(BASE, size=size, max_agent=2, bots_per_graph=0, dirty_tracking=True)
    value = {"stamps": lambda x, y: 1 + y * size + x, "counts": lambda x, y: (x + 1 << 32) | (y + 1),
             "sent": lambda x, y: (x + 1 << 32) | y, "fused": lambda x, y: (7 * x + 1 << 32) | (5 * y + 1)}
    held = ((1, 0), (0, 3))
    planes = {n: np.zeros((size, size), dtype="<u4" if n == "stamps" else "<u8") for n in value}
    blocks = b""
    for bx, by in held + ((1, 4),):
        for name, fmt in (("stamps", "<64I"), ("counts", "<64Q"), ("sent", "<64Q"), ("fused", "<64Q")):
            lanes = []
            for row in range(4):
                for column in range(16):                    # lane = 16 * row + column
                    x, y = 16 * bx + column, 4 * by + row
                    inside = x < size and y < size and (bx, by) in held
                    lanes.append(value[name](x, y) if inside else 0)
                    if inside:
                        planes[name][y, x] = lanes[-1]
            blocks += struct.pack(fmt, *lanes)
    dirty = [0, 0, 0, 1 << 0, 1 << 1]                       # pitch 1: block (0, 3) is bit 0 of word 3, (1, 4) bit 1 of word 4
    scalars = dict(next_seq=11, epoch_base=2, n_rebases=3, edge_rays=4, edge_overflow=5, sweep_min=0.25, sweep_max=1.5,
                   dirty_since_fuse=1, counts_view_fused=1, n_graphs=1, n_bots=nb)
    bots = {"offset": [0.0, -0.5, 0.75], "drift": [[0, 0], [0.125, -0.25], [1.5, 2.5]], "last_closure": [0, -1, 40],
            "zone": [list(ck.ZONE_EMPTY), [1, 2, 3, 4], [5, 6, 7, 8]], "ekf": [[b * 100.0 + i for i in range(44)] for b in range(nb)],
            "ekf_prev": [[b * 10.0 + i for i in range(4)] for b in range(nb)]}
    counters = list(range(100, 120))
    graph = dict(n_nodes=5, lm_x=[0.5], lm_y=[-0.5], lm_node=[2], lm_type=[3], cl_landmark=[0, 0], cl_node=[3, 4],
                 cl_dx=[0.01, 0.02], cl_dy=[-0.01, -0.02], cl_agent=[1, 2])
    flat = lambda rows: [v for r in rows for v in r]
    sections = [
        struct.pack("<5Q2d4I", *(scalars[k] for k in ck.SCALAR_FIELDS)),
        struct.pack("<3d6d3q12Q132d12d", *bots["offset"], *flat(bots["drift"]), *bots["last_closure"], *flat(bots["zone"]),
                    *flat(bots["ekf"]), *flat(bots["ekf_prev"])),
        struct.pack("<20Q", *counters),
        struct.pack("<3q", 5, 1, 2) + struct.pack("<ddqB7x", 0.5, -0.5, 2, 3) +
        struct.pack("<2q2q2d2d2B6x", 0, 0, 3, 4, 0.01, 0.02, -0.01, -0.02, 1, 2),
        struct.pack("<3I", 1, 96, 129),
        blocks,
        struct.pack("<5I", *dirty)]
    hb = 144 + 24 * 7
    body, table = b"", b""
    for kind, payload in enumerate(sections, start=1):
        table += struct.pack("<IIQQ", kind, 0, hb + len(body), len(payload))
        body += payload + bytes(-len(payload) % 8)
    head = struct.pack("<4sIIIQII", b"QSCK", 1, hb, 7, hb + len(body), zlib.crc32(body), 0)
    head += struct.pack("<12i8d", *(int(cfg[k]) for k in ck.CONFIG_INTS), 0, *(cfg[k] for k in ck.CONFIG_F64))
    state = dict(config=cfg, scalars=scalars, counters=np.array(counters, dtype=np.uint64), block_ids=np.array([1, 96, 129], dtype=np.uint32),
                 bots={name: np.array(bots[name], dtype=dt) for name, dt, _ in ck.BOT_ARRAYS},
                 graphs=[dict(graph, **{name: np.array(graph[name], dtype=dt) for name, dt in ck.LANDMARK_ARRAYS + ck.CLOSURE_ARRAYS})],
                 dirty=np.array(dirty, dtype=np.uint32), **planes)
    return head + table + body, state


def test_a_file_packed_by_hand():
    data, state = _hand_packed()
    assert len(data) == 144 + 24 * 7 + 72 + 3 * 56 * 8 + 160 + (24 + 32 + 72) + 16 + 3 * 1792 + 24
    back = ck.read(data)
    assert ck.same_state(state, back) is None, ck.same_state(state, back)
    assert ck.write(state) == data
    assert ck.expected_ids([state[n] for n in ck.PLANES], state["dirty"], 20).tolist() == [1, 96, 129]
    assert ck.expected_ids([state[n] for n in ck.PLANES], None, 20).tolist() == [1, 96]
    assert back["stamps"][3, 19] == 1 + 3 * 20 + 19 and back["counts"][12, 0] == (1 << 32) | 13 and back["sent"][15, 15] == (16 << 32) | 15
    k = load_pkg().checkpoint_config(data)
    assert k["n_blocks"] == 3 and k["dirty_tracking"] is True and k["sections"]["dirty"][1] == 20


# ---- writer against reader ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_planes,dirty", ((1, False), (1, True), (2, False), (4, True)))
@pytest.mark.parametrize("size", (4, 20, 516))
def test_write_then_read_is_the_identity(size, n_planes, dirty):
    cfg = _config(size, n_planes, dirty)
    assert len(ck.planes_of(cfg)) == n_planes
    rng = np.random.default_rng(1000 * size + 10 * n_planes + dirty)
    st = random_state(rng, cfg)
    data = ck.write(st)
    back = ck.read(data)
    want = dict(st, block_ids=ck.expected_ids([st[n] for n in ck.planes_of(cfg)], st.get("dirty"), size))
    assert ck.same_state(want, back) is None, ck.same_state(want, back)
    assert ck.write(back) == data
    # the graphs' lengths were the ones asked for
    assert [len(g["lm_type"]) for g in back["graphs"]] == [0, 1, 7, 8, 9] and [len(g["cl_agent"]) for g in back["graphs"]] == [7, 8, 9, 0, 1]
    # a listed block that holds nothing is kept as listed
    if len(want["block_ids"]) < ck.geometry(size)[0] * ck.geometry(size)[1]:
        bx, by, pitch = *ck.geometry(size)[:2], ck.geometry(size)[2]
        every = np.array([y * 32 * pitch + x for y in range(by) for x in range(bx)], dtype=np.uint32)
        full = ck.read(ck.write(dict(st, block_ids=every)))
        assert ck.same_state(dict(st, block_ids=every), full) is None


@pytest.mark.parametrize("n_planes,dirty", ((1, False), (2, False), (4, True)))
def test_reader_agrees_with_the_package_header_reader(n_planes, dirty):
    cfg = _config(516, n_planes, dirty)
    st = random_state(np.random.default_rng(n_planes), cfg)
    data = ck.write(st)
    back, k = ck.read(data), load_pkg().checkpoint_config(data)
    for name in ck.CONFIG_INTS + ck.CONFIG_F64:
        assert k[name] == back["config"][name] == cfg[name], name
        assert type(k[name]) is type(back["config"][name]), name
    assert k["version"] == 1 and k["total_bytes"] == len(data) and k["n_blocks"] == len(back["block_ids"]) > 0
    want = ["scalars", "bots", "counters", "graphs", "block_ids", "blocks"] + (["dirty"] if dirty else [])
    assert list(k["sections"]) == want
    off, length = k["sections"]["blocks"]
    rec = np.frombuffer(data, dtype="<u4", count=64, offset=off)   # the first block's stamps, where the package says they lie
    cells, inside = ck.block_cells(int(back["block_ids"][0]), 516)
    assert (rec[inside] == back["stamps"].reshape(-1)[cells[inside]]).all() and not rec[~inside].any()
    assert length == len(back["block_ids"]) * ck.block_bytes(n_planes)
    if dirty:
        off, length = k["sections"]["dirty"]
        assert np.frombuffer(data, dtype="<u4", count=length // 4, offset=off).tobytes() == st["dirty"].tobytes()


def _malformable(size=516):
    """A state every malformed variant can be made from: two blocks or more, graph 0 with fewer landmarks than closures."""
    st = random_state(np.random.default_rng(5), _config(size, 2, False), lengths=(2, 9, 5))
    assert len(st["graphs"][0]["lm_x"]) == 2 and len(st["graphs"][0]["cl_node"]) == 5
    return st


@pytest.mark.parametrize("what", ck.MALFORMED)
def test_every_malformed_file_is_refused(what):
    st = _malformable()
    good = ck.write(st)
    ck.read(good)
    bad = ck.write(st, malformed=what)
    assert bad != good
    if what not in ("duplicate_kind", "offset_unaligned"):
        load_pkg().checkpoint_config(bad)                   # the CRC is right: the header reader has nothing to object to
    with pytest.raises(ValueError):
        ck.read(bad)


@pytest.mark.parametrize("damage", ("magic", "version", "length", "crc", "padding", "edge_cell", "flag"))
def test_reader_refuses_damage(damage):
    import struct
    import zlib
    st = _malformable(20)                                   # 20 = 16 + 4: the second block column is partial
    st["stamps"][3, 19] = 9
    data = bytearray(ck.write(st))
    hb = struct.unpack_from("<I", data, 8)[0]
    fix_crc = True
    if damage == "magic":
        data[:4], fix_crc = b"QSCX", False
    elif damage == "version":
        struct.pack_into("<I", data, 4, 2)
    elif damage == "length":
        data, fix_crc = data[:-8], False
    elif damage == "crc":
        data[-1] ^= 1
        fix_crc = False
    elif damage == "padding":                               # graph 0's landmark types: 2 bytes, then 6 of padding
        off = struct.unpack_from("<Q", data, 144 + 24 * 3 + 8)[0]
        at = off + 24 * len(st["graphs"]) + 24 * 2 + 2
        assert not any(data[at:at + 6])
        data[at + 5] = 1
    elif damage == "edge_cell":                             # block 1 (bx 1): columns 20.. lie beyond the edge
        ids = ck.read(bytes(data))["block_ids"].tolist()
        off = struct.unpack_from("<Q", data, 144 + 24 * 5 + 8)[0]
        at = off + ids.index(1) * ck.block_bytes(2) + 4 * (16 * 3 + 4)
        assert struct.unpack_from("<I", data, at - 4)[0] == 9
        struct.pack_into("<I", data, at, 5)
    elif damage == "flag":
        struct.pack_into("<i", data, 32 + 4 * 4, 2)
    if fix_crc:
        struct.pack_into("<I", data, 24, zlib.crc32(bytes(data[hb:])))
    with pytest.raises(ValueError):
        ck.read(bytes(data))
