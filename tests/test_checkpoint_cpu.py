"""The checkpoint file's header, read without a GPU: a header packed by hand from the layout documented in
include/quasar_slam.h must come back as the configuration it holds, and every kind of damage must be refused."""
import re
import struct
import zlib

import pytest

from conftest import load_pkg

CFG = dict(size=4096, min_poses_between=30, max_agent=64, bots_per_graph=2, enable_counts=True, enable_ekf=True, seq_stride=1,
           shard_bots=0, shard_rank=0, exact_trig=True, dirty_tracking=False, res=0.05, ox=-102.4, oy=-102.4, min_dist=0.05,
           max_dist=1.2, closure_radius=0.6, closure_correction=0.5, ekf_metres_per_tick=0.0107)
INTS = ("size", "min_poses_between", "max_agent", "bots_per_graph", "enable_counts", "enable_ekf", "seq_stride", "shard_bots",
        "shard_rank", "exact_trig", "dirty_tracking")
F64 = ("res", "ox", "oy", "min_dist", "max_dist", "closure_radius", "closure_correction", "ekf_metres_per_tick")


def _pack(cfg=CFG, version=1, n_blocks=3):
    """A checkpoint by the documented layout: fixed header, section table, 8-byte aligned sections, CRC of the body."""
    sections = [(1, 72), (2, 65 * 448), (3, 20 * 8), (4, 32 * 24), (5, 4 * n_blocks), (6, 768 * n_blocks)]
    hb = 144 + 24 * len(sections)
    body = bytearray()
    table = b""
    for kind, length in sections:
        table += struct.pack("<IIQQ", kind, 0, hb + len(body), length)
        body += bytes((kind * 7 + i) & 0xff for i in range(length)) + bytes(-length % 8)
    ints = [int(cfg[k]) for k in INTS] + [0]
    head = struct.pack("<4sIIIQII", b"QSCK", version, hb, len(sections), hb + len(body), zlib.crc32(body), 0)
    head += struct.pack("<12i8d", *ints, *(cfg[k] for k in F64))
    assert len(head) == 144
    return bytearray(head + table + body)


def test_header_round_trip():
    ck = load_pkg().checkpoint_config
    data = _pack()
    k = ck(bytes(data))
    for name, v in CFG.items():
        assert k[name] == v, name
    assert k["version"] == 1 and k["total_bytes"] == len(data) and k["n_blocks"] == 3
    assert set(k["sections"]) == {"scalars", "bots", "counters", "graphs", "block_ids", "blocks"}
    off, length = k["sections"]["blocks"]
    assert length == 3 * 768 and off % 8 == 0 and off + length <= len(data)
    assert ck(memoryview(data))["size"] == 4096                       # any buffer object


@pytest.mark.parametrize("damage", ["magic", "version", "truncated_header", "truncated_section", "crc", "table"])
def test_header_refusals(damage):
    ck = load_pkg().checkpoint_config
    data = _pack()
    if damage == "magic":
        data[:4] = b"QSCX"
    elif damage == "version":
        data = _pack(version=2)
    elif damage == "truncated_header":
        data = data[:100]
    elif damage == "truncated_section":
        data = data[:-8]
    elif damage == "crc":
        data[-1] ^= 0x01
    elif damage == "table":                                           # a section reaching past the end, CRC still right
        struct.pack_into("<Q", data, 144 + 24 * 5 + 16, 10 ** 9)
    with pytest.raises(ValueError):
        ck(bytes(data))


def test_checkpoint_symbols_are_declared_and_bound():
    from importlib import import_module
    lib = import_module(load_pkg().__name__ + "._lib")
    assert "qs_checkpoint" in lib.SIGNATURES and "qs_restore" in lib.SIGNATURES
    with open(lib.HEADER) as f:
        txt = f.read()
    assert re.search(r"int qs_checkpoint\(qs_ctx \*ctx, uint8_t \*buf, size_t cap, size_t \*n_out\);", txt)
    assert re.search(r"int qs_restore\(qs_ctx \*ctx, const uint8_t \*buf, size_t n\);", txt)
    assert '#define QS_CKPT_MAGIC "QSCK"' in txt and "#define QS_CKPT_VERSION 1" in txt
    assert "#define QS_CKPT_HEADER_FIXED 144" in txt
