"""The checkpoint file against an independent reader and writer (tests/checkpoint_rules.py, written from the format text of
include/quasar_slam.h): what qs_checkpoint writes is decoded by the documented layout and compared with the views of the
context, and files the library did not write are restored and compared the same way.  A mistake made alike in the pack and
the unpack kernel round-trips; it does not survive either comparison.

The maps are painted: numpy planes folded into a context with qs_fuse_buffers*, so that any bits lie in any cell of a small
grid -- block, bitmap-word and launch edges chosen, not met by chance.  Recorded sessions are used for the pose-graph sections
only.  Every comparison is exact."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch  # before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

import checkpoint_rules as ck
from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
QS_E_INVAL = -1
SIZES = (4, 20, 512, 516, 1040)
MODES = ("stamps", "counts", "tracking")                   # counters off; counters on; counters on with dirty tracking


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def mods(pkg):
    return importlib.import_module(pkg.__name__ + ".dist"), importlib.import_module(pkg.__name__ + ".replay")


def _kw(size, mode="counts"):
    return dict(size=size, resolution=0.05, origin_x=-size * 0.025, origin_y=-size * 0.025, enable_counts=mode != "stamps")


def _mapper(pkg, size, mode):
    m = pkg.QuasarMapper(**_kw(size, mode))
    if mode == "tracking":
        m.dirty_tracking(True)                              # before the first paint: refused once the grid has unfused writes
    return m


# ---- painting ------------------------------------------------------------------------------------------------------------
def paint(m, stamps, counts, rows=None):
    """Fold numpy planes into the context: stamps uint32 [size, size] in [0, 2^31) or None, counts int32 [size, size, 2]
    (misses, hits) or None.  rows = (y0, y1): only those grid rows, through qs_fuse_buffers_range."""
    size = m.size
    y0, y1 = rows if rows is not None else (0, size)
    d_st = None if stamps is None else torch.from_numpy(np.ascontiguousarray(stamps[y0:y1]).view(np.int32)).to(DEV)
    d_ct = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts[y0:y1], dtype=np.int32)).to(DEV)
    sp = None if d_st is None else [d_st.data_ptr()]
    cp = None if d_ct is None else [d_ct.data_ptr()]
    if rows is None and sp is not None:
        m.fuse_buffers(sp, cp)
    else:
        m.fuse_buffers_range(sp, cp, y0 * size, (y1 - y0) * size)       # stamp_ptrs None: counters without stamps
    m.sync()                                                # (the uploads stay alive until the fold has run)


def _u64(pairs):
    """int32 [..., 2] (misses, hits) -> the u64 counter words"""
    return np.ascontiguousarray(pairs, dtype=np.int32).view(np.uint64).reshape(pairs.shape[:-1])


def _pairs(words):
    return np.ascontiguousarray(words, dtype=np.uint64).view(np.int32).reshape(words.shape + (2,))


def _device_planes(distmod, m):
    """What the context holds, by the views that alias its buffers: stamps u32, counts u64 or None, fused u64 or None."""
    m.sync()
    st, ct = distmod.grid_tensors(m, DEV)
    fu = distmod.fused_counts_view(m, DEV) if ct is not None else None
    return (st.cpu().numpy().view(np.uint32).copy(), None if ct is None else _u64(ct.cpu().numpy()),
            None if fu is None else _u64(fu.cpu().numpy()))


def pattern(size, rng):
    """The cells where the block code can go wrong -> (stamps u32, counts i32 pairs on the same cells, counts i32 pairs of
    one block that gets counters and no stamps -- all zero when the grid is a single block)."""
    pts = {(0, 0), (size - 1, 0), (0, size - 1), (size - 1, size - 1)}               # the four corners
    pts |= {(size - 1, y) for y in range(min(size, 10))}                             # the last valid column, over two block rows
    if size % 16:
        pts.add((size - size % 16, min(size - 1, 6)))                                # the partial last block
    pts |= {(x, y) for x in (15, 16) for y in (3, 4) if x < size and y < size}       # block border x block-row border
    pts |= {(x, min(size - 1, 13)) for x in (511, 512) if x < size}                  # bitmap-word border: bx = 31 | 32
    stamps = np.zeros((size, size), dtype=np.uint32)
    counts = np.zeros((size, size, 2), dtype=np.int32)
    for x, y in sorted(pts):
        stamps[y, x] = rng.integers(1, 1 << 31)
        counts[y, x] = rng.integers(0, 1 << 16, 2)
    only = np.zeros((size, size, 2), dtype=np.int32)
    if size >= 12:                                          # block (0, 2): rows 8..11, columns 0..15 hold no stamp
        assert not stamps[8:12, :16].any()
        only[9, 5] = rng.integers(1, 1 << 16, 2)
        only[11, 0] = (0, 3)
    return stamps, counts, only


def _block_rows(size, row_ranges):
    """bool [blocks_y, blocks_x]: every block of the block rows that hold a grid row of the ranges."""
    blocks_x, blocks_y = ck.geometry(size)[:2]
    bits = np.zeros((blocks_y, blocks_x), dtype=bool)
    for y0, y1 in row_ranges:
        bits[y0 // 4:(y1 - 1) // 4 + 1] = True
    return bits


def _popcount(bits):
    return int(np.asarray(bits).sum())


def _check_file(pkg, distmod, m, data, mode, want=None, touched=None):
    """Decode a checkpoint of m by the rules and compare it with the context's own views (and with `want`, the numpy planes
    that were painted: {name: plane}); returns the decoded state."""
    size = m.size
    st = ck.read(data)
    names = ck.planes_of(st["config"])
    assert names == {"stamps": ck.PLANES[:1], "counts": ck.PLANES[:2], "tracking": ck.PLANES}[mode]
    assert st["config"]["size"] == size and st["config"]["dirty_tracking"] == (mode == "tracking")
    d_st, d_ct, d_fu = _device_planes(distmod, m)
    assert (st["stamps"] == d_st).all(), f"stamps: {int((st['stamps'] != d_st).sum())} cells differ from the device's"
    if mode != "stamps":
        assert (st["counts"] == d_ct).all(), f"counts: {int((st['counts'] != d_ct).sum())} cells differ from the device's"
    if mode == "tracking":
        assert (st["fused"] == d_fu).all(), f"fused: {int((st['fused'] != d_fu).sum())} cells differ from the device's"
    for name, plane in (want or {}).items():
        assert (st[name] == plane).all(), f"{name}: {int((st[name] != plane).sum())} cells differ from what was painted"
    dirty = st.get("dirty")
    ids = ck.expected_ids([st[n] for n in names], dirty, size)
    assert st["block_ids"].tolist() == ids.tolist()
    assert pkg.checkpoint_config(data)["n_blocks"] == len(ids)
    if mode == "tracking":
        bits = ck.dirty_bits(dirty, size)
        assert _popcount(bits) == m.dirty_blocks()[0]
        if touched is not None:
            assert (bits == touched).all(), "the DIRTY section is not the block rows the folds touched"
    assert ck.write(st) == data
    return st


# ---- a. decode what the library wrote: painted planes ------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_painted_planes_decode_by_the_documented_layout(pkg, mods, size, mode):
    distmod, _ = mods
    rng = np.random.default_rng(size * 10 + MODES.index(mode))
    stamps, counts, only = pattern(size, rng)
    with _mapper(pkg, size, mode) as m:
        if mode == "stamps":
            paint(m, stamps, None)
            want = {"stamps": stamps}
            st = _check_file(pkg, distmod, m, m.checkpoint(), mode, want)
            return
        if mode == "counts":
            paint(m, stamps, counts)
            paint(m, None, only)
            want = {"stamps": stamps, "counts": _u64(counts + only)}
            st = _check_file(pkg, distmod, m, m.checkpoint(), mode, want)
            if size >= 12:                                  # the block with counters and no stamps is in the file
                assert 2 * 32 * ck.geometry(size)[2] in st["block_ids"].tolist()
            return
        # tracking: row ranges, whose marking leaves all-zero blocks dirty (a fold marks whole block rows)
        top, low = (0, min(size, 14)), (size - 4, size)
        ranges = [top] + ([low] if size > 14 else [])
        assert not stamps[top[1]:low[0]].any() and not only[top[1]:].any()      # (the pattern lies in those rows)
        for r in ranges:
            paint(m, stamps, counts, rows=r)
        if size >= 12:
            paint(m, None, only, rows=(8, 12))
        c1 = _u64(counts + only)
        zero = np.zeros((size, size), dtype=np.uint64)
        touched = _block_rows(size, ranges)
        st = _check_file(pkg, distmod, m, m.checkpoint(), mode, {"stamps": stamps, "counts": c1, "sent": zero, "fused": zero},
                         touched)
        held = ck.expected_ids([stamps, c1], None, size)
        assert len(st["block_ids"]) == _popcount(touched) and (size < 512 or len(held) < len(st["block_ids"]))
        # a one-rank sparse fuse carries the first layer; a second layer on other rows
        m.sparse_fuse_begin(1, 0)
        m.sparse_fuse_plan(1)
        m.sparse_fuse_apply()
        rows2 = (20, 26) if size >= 28 else (0, 4)
        st2 = np.zeros_like(stamps)
        ct2 = np.zeros_like(counts)
        for y in range(*rows2):
            for x in {0, size - 1, min(size - 1, 17)}:
                st2[y, x] = rng.integers(1, 1 << 31)
                ct2[y, x] = rng.integers(0, 1 << 16, 2)
        paint(m, st2, ct2, rows=rows2)
        want = {"stamps": np.maximum(stamps, st2), "counts": _u64(counts + only + ct2), "sent": c1, "fused": c1}
        _check_file(pkg, distmod, m, m.checkpoint(), mode, want, _block_rows(size, [rows2]))


# ---- c. restore what the library did not write ---------------------------------------------------------------------------
def _written_state(pkg, size, mode, rng, density=None):
    """A state by the rules' writer for a context of _kw(size, mode): configuration, scalars and bots as a new context has
    them (decoded from its checkpoint), the planes and the bitmap random (most cells zero; a third of them on the grids
    of a few blocks, where every plane must still hold something)."""
    density = (0.3 if size <= 20 else 0.02) if density is None else density
    with _mapper(pkg, size, mode) as fresh:
        st = ck.read(fresh.checkpoint())
    assert len(st["block_ids"]) == 0 and not st["stamps"].any()
    for name in ck.planes_of(st["config"]):
        if name == "stamps":
            plane = rng.integers(1, 1 << 31, (size, size), dtype=np.uint32)
        else:
            plane = _u64(rng.integers(0, 1 << 16, (size, size, 2)).astype(np.int32))
        if density < 1:
            plane[rng.random((size, size)) >= density] = 0
            plane[8:12] = 0                                 # (a block row that holds nothing, whatever the density)
        st[name] = plane
    st["stamps"][0, 0], st["stamps"][size - 1, size - 1] = 5, 6          # never empty, and the last block is there
    if mode == "tracking":
        blocks_x, blocks_y = ck.geometry(size)[:2]
        st["dirty"] = ck.bitmap_of(rng.random((blocks_y, blocks_x)) < 0.1, size)    # some of them blocks that hold nothing
        st["scalars"]["dirty_since_fuse"] = 1
    del st["block_ids"]
    return st


def _check_restored(pkg, distmod, m, st, mode):
    size = m.size
    d_st, d_ct, d_fu = _device_planes(distmod, m)
    assert (d_st == st["stamps"]).all(), f"stamps: {int((d_st != st['stamps']).sum())} cells differ"
    tri = np.where(st["stamps"] == 0, -1, np.where(st["stamps"] & 1, 100, 0)).astype(np.int8)
    assert (m.grid_i8() == tri).all()
    if mode != "stamps":
        assert (d_ct == st["counts"]).all(), f"counts: {int((d_ct != st['counts']).sum())} cells differ"
        hits, misses = m.counts()                           # (counts_view_fused is 0 in the file: the local counters)
        pairs = _pairs(st["counts"])
        assert (hits == pairs[..., 1]).all() and (misses == pairs[..., 0]).all()
    if mode == "tracking":
        assert (d_fu == st["fused"]).all(), f"fused: {int((d_fu != st['fused']).sum())} cells differ"
        assert m.dirty_blocks()[0] == _popcount(ck.dirty_bits(st["dirty"], size))


def _restore_written(pkg, distmod, size, mode, rng, density=None):
    st = _written_state(pkg, size, mode, rng, density)
    data = ck.write(st)
    with pkg.QuasarMapper(**_kw(size, mode)) as m:          # tracking off here: the restore switches it on
        m.restore(data)
        _check_restored(pkg, distmod, m, st, mode)
        again = m.checkpoint()
        assert len(again) == len(data) and again == data, "checkpoint() of the restored context is not the written file"
    return st, data


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_restore_a_file_the_library_did_not_write(pkg, mods, size, mode):
    distmod, _ = mods
    rng = np.random.default_rng(size * 10 + 5 + MODES.index(mode))
    st, data = _restore_written(pkg, distmod, size, mode, rng)
    # a listed block that holds nothing is legal (a dirty block may be empty); the next checkpoint does not list it
    names = ck.planes_of(ck.read(data)["config"])
    ids = ck.expected_ids([st[n] for n in names], st.get("dirty"), size)
    blocks_x, blocks_y, pitch, _ = ck.geometry(size)
    every = np.array([by * 32 * pitch + bx for by in range(blocks_y) for bx in range(blocks_x)], dtype=np.uint32)
    spare = np.setdiff1d(every, ids)
    if len(spare) == 0:                                     # (size 4: one block, and it is held) -- list it empty instead
        st = dict(st, **{n: np.zeros_like(st[n]) for n in names})
        if mode == "tracking":
            st["dirty"] = np.zeros_like(st["dirty"])
        ids, spare, data = np.zeros(0, dtype=np.uint32), every, None
    listed = np.sort(np.concatenate([ids, spare[[0, -1]] if len(spare) > 1 else spare])).astype(np.uint32)
    with pkg.QuasarMapper(**_kw(size, mode)) as m:
        m.restore(ck.write(dict(st, block_ids=listed)))
        _check_restored(pkg, distmod, m, st, mode)
        assert m.checkpoint() == ck.write(st)


# ---- b. launch edges -------------------------------------------------------------------------------------------------------
def test_launch_edges_at_2052(pkg, mods):
    """Every cell of 2052^2 nonzero: 66 177 blocks (the pack launch has 16 384 waves: its stride loop runs), 2 565 bitmap words
    (three per thread of the list kernel), 1 052 676 quads of cells (the census launch covers 524 288 per pass)."""
    distmod, _ = mods
    size = 2052
    blocks_x, blocks_y, pitch, words = ck.geometry(size)
    assert (blocks_x * blocks_y, words) == (66_177, 2_565) and blocks_x * blocks_y > 16_384 and words > 2 * 1024
    assert size * size // 4 > 2048 * 256
    rng = np.random.default_rng(2052)
    stamps = rng.integers(1, 1 << 31, (size, size), dtype=np.uint32)
    counts = rng.integers(0, 1 << 16, (size, size, 2)).astype(np.int32)
    with _mapper(pkg, size, "counts") as m:
        paint(m, stamps, counts)
        data = m.checkpoint()
        st = _check_file(pkg, distmod, m, data, "counts", {"stamps": stamps, "counts": _u64(counts)})
        assert len(st["block_ids"]) == blocks_x * blocks_y
    del data, st
    _restore_written(pkg, distmod, size, "counts", rng, density=1.0)


# ---- d. the host checks of qs_restore behind the CRC ---------------------------------------------------------------------
def _rc_restore(m, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    rc = m._L.qs_restore(m._h, a.ctypes.data_as(C.c_void_p), len(a))
    return rc, m._L.qs_last_error(m._h).decode()


def _fingerprint(distmod, m):
    m.sync()
    st, _ = distmod.grid_tensors(m, DEV)
    return st.cpu().numpy().copy(), m.closures(0)[0], m.slam_sizes(0)


# what qs_last_error has to name for each malformed file of the rules' writer
REFUSALS = {"ids_equal": "bad block id at 1", "ids_descending": "bad block id at 1", "id_bx_past_edge": "bad block id at",
            "id_by_past_edge": "bad block id at", "ids_length_not_4": "section", "graph_L_gt_N": "bad sizes of graph 0",
            "graph_C_gt_N": "bad sizes of graph 0", "graph_negative": "bad sizes of graph 0",
            "duplicate_kind": "bad section table entry 2", "offset_unaligned": "bad section table entry 2",
            "seven_sections_tracking_off": "section lengths do not add up", "blocks_one_short": "section lengths do not add up"}


def test_every_malformed_variant_has_a_case():
    assert set(REFUSALS) == set(ck.MALFORMED)


@pytest.fixture(scope="module")
def malformable(pkg):
    """A good file for _kw(516, "counts") -- 33 block columns: bit 33 of a two-word bitmap row is the first padding bit --
    whose graph holds 10 nodes, 2 landmarks and 5 closures."""
    rng = np.random.default_rng(516)
    st = _written_state(pkg, 516, "counts", rng)
    assert len(st["graphs"]) == 1
    g = st["graphs"][0]
    g.update(n_nodes=10, lm_x=np.array([0.5, 1.5]), lm_y=np.array([0.25, 0.75]), lm_node=np.array([1, 4]),
             lm_type=np.array([1, 2], dtype=np.uint8), cl_landmark=np.array([0, 0, 1, 1, 0]), cl_node=np.array([5, 6, 7, 8, 9]),
             cl_dx=np.zeros(5), cl_dy=np.zeros(5), cl_agent=np.ones(5, dtype=np.uint8))
    ck.read(ck.write(st))
    return st


@pytest.mark.parametrize("what", ck.MALFORMED)
def test_host_checks_behind_the_crc(pkg, mods, malformable, what):
    """Every case returns from qs_restore on the host, before anything is launched or changed (csrc/checkpoint.hip: all of
    them fail a check above the call of ck_apply)."""
    distmod, _ = mods
    bad = ck.write(malformable, malformed=what)
    if what not in ("duplicate_kind", "offset_unaligned"):
        pkg.checkpoint_config(bad)                          # (the CRC is right: the header reader has nothing to object to)
    with pytest.raises(ValueError):
        ck.read(bad)
    rng = np.random.default_rng(3)
    stamps, counts, only = pattern(516, rng)
    with _mapper(pkg, 516, "counts") as m:
        paint(m, stamps, counts)
        before = _fingerprint(distmod, m)
        assert (before[0].view(np.uint32) == stamps).all()
        rc, err = _rc_restore(m, bad)
        assert rc == QS_E_INVAL, f"{what}: rc {rc} ({err})"
        assert REFUSALS[what] in err, f"{what}: '{REFUSALS[what]}' not named in '{err}'"
        after = _fingerprint(distmod, m)
        assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and before[2] == after[2], what
        _, d_ct, _ = _device_planes(distmod, m)
        assert (d_ct == _u64(counts)).all()


# ---- e. decode what the library wrote: real sessions -----------------------------------------------------------------------
def _golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)


def _session(name, pkg, replay):
    """(mapper kwargs, run(m), offsets {bot: x offset}, sweep filter)"""
    P = importlib.import_module(pkg.__name__ + ".protocol")
    default_filter = (P.SWEEP_MIN_DIST_M, P.SWEEP_MAX_DIST_M)
    if name == "adversarial_dense_200":
        g = _golden(name)
        size, res, ox, oy, sep = g["cfg"]
        kw = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy, separation=sep, max_agent=2)
        times = g["recv_time"] if "recv_time" in g.files else None
        return kw, (lambda m: m.ingest_array(g["datagrams"], g["lengths"], times)), {1: 0.0, 2: float(sep)}, default_filter
    if name == "session_512":
        g, s = _golden("session_512"), _golden("sweeps_512")
        size, res, ox, oy, sep = g["cfg"]
        kw = dict(size=int(size), resolution=res, origin_x=ox, origin_y=oy, separation=sep)
        data, lens, sw = g["datagrams"], g["lengths"], s["sweeps_odo"]
        kp, ks = len(data) // 2, len(sw) // 2

        def run(m):                                         # the first part of test_sweeps_and_offsets (test_gpu_checkpoint.py)
            m.set_bot_offset(1, -0.35)
            m.set_bot_offset(2, 0.8)
            m.set_sweep_filter(0.15, 1.0)
            m.ingest_array(data[:kp // 2], lens[:kp // 2])
            m.ingest_sweeps(sw[:ks])
            m.ingest_array(data[kp // 2:kp], lens[kp // 2:kp])
        return kw, run, {1: -0.35, 2: 0.8}, (0.15, 1.0)
    stream = replay.multi_bot_stream(None, 64, 22_000)[:4000]
    kw = dict(size=4096, resolution=0.05, origin_x=-102.4, origin_y=-102.4, max_agent=64, bots_per_graph=2, enable_ekf=True)
    return kw, (lambda m: m.ingest_array(stream)), {b: 0.0 for b in range(1, 65)}, default_filter


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["adversarial_dense_200", "session_512", "multibot_4000"])
def test_real_sessions_decode_by_the_documented_layout(pkg, mods, name):
    distmod, replay = mods
    kw, run, offsets, sweep_filter = _session(name, pkg, replay)
    with pkg.QuasarMapper(**kw) as m:
        run(m)
        data = m.checkpoint()
        st = ck.read(data)
        cfg, sc, bots = st["config"], st["scalars"], st["bots"]
        assert cfg["size"] == kw["size"] and cfg["max_agent"] == m.max_agent and cfg["enable_ekf"] == bool(kw.get("enable_ekf"))
        assert cfg["res"] == kw["resolution"] and cfg["ox"] == kw["origin_x"] and cfg["oy"] == kw["origin_y"]
        assert sc["n_graphs"] == m.n_graphs == len(st["graphs"]) and sc["n_bots"] == m.max_agent + 1
        n_lm = n_cl = 0
        for g, gr in enumerate(st["graphs"]):
            assert (gr["n_nodes"], len(gr["lm_x"]), len(gr["cl_node"])) == m.slam_sizes(g), f"sizes of graph {g}"
            xy, ti = m.landmarks(g)
            assert _same_bits(np.column_stack([gr["lm_x"], gr["lm_y"]]), xy), f"landmark positions of graph {g}"
            assert _same_bits(np.column_stack([gr["lm_type"].astype(np.int64), gr["lm_node"]]), ti), f"landmark type / node of graph {g}"
            idx, corr = m.closures(g)
            assert _same_bits(np.column_stack([gr["cl_landmark"], gr["cl_node"]]), idx), f"closures of graph {g}"
            assert _same_bits(np.column_stack([gr["cl_dx"], gr["cl_dy"]]), corr), f"closure corrections of graph {g}"
            assert _same_bits(gr["cl_agent"], m.closure_agents(g)), f"closure agents of graph {g}"
            n_lm, n_cl = n_lm + len(gr["lm_x"]), n_cl + len(gr["cl_node"])
        assert name != "adversarial_dense_200" or (n_lm > 0 and n_cl > 0), "the session has no closure"
        boxes = 0
        for b in range(1, m.max_agent + 1):
            assert _same_bits(bots["drift"][b], m.drift(b)), f"drift of bot {b}"
            assert bots["offset"][b] == offsets[b], f"offset of bot {b}"
            words = tuple(int(w) for w in bots["zone"][b])
            box = None if words[0] == ck.ZONE_EMPTY[0] else tuple(ck.zone_values(bots["zone"][b]).tolist())
            assert box == m.zone(b), f"zone of bot {b}"
            want = (999.0, 999.0, -999.0, -999.0) if box is None else box
            assert m.zone_packet(b) == b"ZONE" + np.array(want, dtype="<f4").tobytes(), f"ZONE packet of bot {b}"
            boxes += box is not None
            x, P = m.ekf_state(b)
            assert _same_bits(bots["ekf"][b, :6], x) and _same_bits(bots["ekf"][b, 6:42].reshape(6, 6), P), f"EKF of bot {b}"
            assert bots["ekf"][b, 43] in (0.0, 1.0)
        assert boxes > 0 and (not cfg["enable_ekf"] or bots["ekf"][1:, 43].any())
        cnt = m.counters()
        names = importlib.import_module(pkg.__name__ + "._lib").QS_CNT_NAMES
        assert len(names) == len(ck.CNT_NAMES)
        from_scalars = {"REBASES": "n_rebases", "EDGE_RAYS": "edge_rays", "EDGE_OVERFLOW": "edge_overflow"}
        for i, (mine, theirs) in enumerate(zip(ck.CNT_NAMES, names)):
            got = sc[from_scalars[mine]] if mine in from_scalars else int(st["counters"][i])
            assert got == cnt[theirs], f"counter {mine}"
        assert cnt["accepted"] > 0 and cnt["cells"] > 0
        assert (sc["sweep_min"], sc["sweep_max"]) == sweep_filter
        assert sc["next_seq"] > 0
        d_st, d_ct, _ = _device_planes(distmod, m)
        assert (st["stamps"] == d_st).all() and (st["counts"] == d_ct).all() and d_st.any() and d_ct.any()
        assert st["block_ids"].tolist() == ck.expected_ids([st["stamps"], st["counts"]], None, kw["size"]).tolist()
        assert ck.write(st) == data


# ---- f. sparse fuse on painted planes ---------------------------------------------------------------------------------------
def _layer(size, rng, row_ranges):
    """Random cells in the given grid rows, the last (partial) block column among them -> (stamps, counts pairs)"""
    stamps = np.zeros((size, size), dtype=np.uint32)
    counts = np.zeros((size, size, 2), dtype=np.int32)
    for y0, y1 in row_ranges:
        n = y1 - y0
        mask = rng.random((n, size)) < 0.03
        mask[:, size - 1] = rng.random(n) < 0.5
        mask[0, size - 1] = True
        stamps[y0:y1][mask] = rng.integers(1, 1 << 31, int(mask.sum()), dtype=np.uint32)
        cmask = mask | (rng.random((n, size)) < 0.01)       # some counters without stamps
        counts[y0:y1][cmask] = rng.integers(0, 1 << 16, (int(cmask.sum()), 2)).astype(np.int32)
    return stamps, counts


@pytest.mark.parametrize("size", (20, 516, 2052))
def test_sparse_fuse_of_painted_layers(pkg, mods, size):
    """Two contexts as ranks, each with a layer of its own: rows 0..11 of both overlap, the rest is disjoint, and the block
    rows in between stay untouched.  After the fuse both hold the cell-wise maximum of the stamps and the sum of the counters;
    a second round with new layers shows that deltas, not totals, travel."""
    distmod, _ = mods
    rng = np.random.default_rng(size + 77)
    q = size // 4
    rounds = [([(0, 12)] + ([(q - 2, q + 6)] if size > 20 else []), [(4, 12)] + ([(3 * q - 3, 3 * q + 5)] if size > 20 else [(16, 20)])),
              ([(8, 16)], [(size - 8, size)])]
    ms = [_mapper(pkg, size, "tracking") for _ in range(2)]
    try:
        st_all = np.zeros((size, size), dtype=np.uint32)
        ct_all = np.zeros((size, size), dtype=np.uint64)
        own = [np.zeros((size, size), dtype=np.uint64) for _ in ms]
        for k, ranges in enumerate(rounds):
            for r, m in enumerate(ms):
                stamps, counts = _layer(size, rng, ranges[r])
                for rows in ranges[r]:
                    paint(m, stamps, counts, rows=rows)
                st_all = np.maximum(st_all, stamps)
                ct_all += _u64(counts)
                own[r] += _u64(counts)
                assert m.dirty_blocks()[0] == _popcount(_block_rows(size, ranges[r]))
            distmod.sparse_fuse_local(ms, DEV)
            for r, m in enumerate(ms):
                d_st, d_ct, d_fu = _device_planes(distmod, m)
                assert (d_st == st_all).all(), f"round {k}, rank {r}: {int((d_st != st_all).sum())} stamps differ from the maximum"
                assert (d_fu == ct_all).all(), f"round {k}, rank {r}: {int((d_fu != ct_all).sum())} fused counters differ from the sum"
                assert (d_ct == own[r]).all(), f"round {k}, rank {r}: the local counters changed"
                assert m.dirty_blocks()[0] == 0
                hits, misses = m.counts()                   # the counts view reads the fused counters from now on
                pairs = _pairs(ct_all)
                assert (hits == pairs[..., 1]).all() and (misses == pairs[..., 0]).all()
                # a file whose sent and fused planes differ (after a one-rank fuse they are equal): sent is the own total
                _check_file(pkg, distmod, m, m.checkpoint(), "tracking",
                            {"stamps": st_all, "counts": own[r], "sent": own[r], "fused": ct_all})
    finally:
        for m in ms:
            m.close()
