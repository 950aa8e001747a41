"""Trail matching: the ABI of the two entry points -- symbols, the 80-byte result against protocol.TRAIL_MATCH_DTYPE and the
restatement's, the constants, and the header's text of the limits."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np

import trail_rules as TR
from conftest import ROOT, load_pkg

NEW_SYMBOLS = ("qs_match_trails", "qs_match_trails_device")


def test_symbols_struct_and_constants():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    P = importlib.import_module(pkg.__name__ + ".protocol")
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == 11
    # six int32, two int32, two uint8 padded to 8, five doubles
    assert re.search(r"typedef struct qs_trail_match \{\s*int32_t ix, iy, it, score, score0, hits;\s*int32_t records, anchor;\s*"
                     r"uint8_t agent, accepted_match, pad\[6\];\s*double ax, ay, dx, dy, dyaw;\s*\} qs_trail_match;", code)
    assert C.sizeof(L.QsTrailMatch) == 8 * 4 + 8 + 5 * 8 == 80 == P.TRAIL_MATCH_DTYPE.itemsize == TR.TRAIL_DTYPE.itemsize
    assert P.TRAIL_MATCH_DTYPE == TR.TRAIL_DTYPE
    for f in TR.FIELDS:
        assert getattr(L.QsTrailMatch, f).offset == P.TRAIL_MATCH_DTYPE.fields[f][1], f
    assert L.QsTrailMatch.ax.offset == 40 and L.QsTrailMatch.anchor.offset == 28 and L.QsTrailMatch.agent.offset == 32
    assert re.search(r"#define QS_TRAIL_MAX_RECORDS 64\b", code)
    assert P.TRAIL_MAX_RECORDS == L.QS_TRAIL_MAX_RECORDS == TR.MAX_RECORDS == 64
    assert P.TRAIL_TRAVEL == TR.TRAVEL == 4.0
    assert (P.MIN_DIST_M, P.MAX_DIST_M) == (TR.MIN_DIST, TR.MAX_DIST)
    assert np.dtype(P.PACKET_DTYPE).itemsize == TR.PACKET_DTYPE.itemsize == 42
    # the default travel fits the reference's filter and grid with the default window; the room's filter needs less
    assert TR.limit_ok(TR.params(), P.MAX_DIST_M, P.TRAIL_TRAVEL, P.GRID_RESOLUTION)
    assert not TR.limit_ok(TR.params(), 3.0, P.TRAIL_TRAVEL, P.GRID_RESOLUTION) and TR.limit_ok(TR.params(), 3.0, 2.8, P.GRID_RESOLUTION)


def test_the_header_states_the_rule_and_its_limits():
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    sec = txt[txt.index("---- trail matching"):txt.index("---- OccupancyGrid object API")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for rule in ("T1.", "T2.", "T3.", "T4.", "T5.", "T6.", "T7.", "T8."):
        assert rule in sec
    for words in ("ceil((max_dist + travel) / res) + window + radius + 2 <= QS_MATCH_MAX_REACH", "travel finite and >= 0",
                  "1 <= gsize[g] <= QS_TRAIL_MAX_RECORDS", "QS_E_INVAL", "A sharded context refuses",
                  "write nothing to the context", "gsize is a HOST array", "anchor = -1",
                  "front (c, s), left (-s, c), back (-c, -s), right (s, -c)", "min_dist < d <= max_dist",
                  "ex = ax + (C * qx - S * qy), ey = ay + (S * qx + C * qy)", "tests/trail_rules.py"):
        assert words in flat, words


def test_trail_move_is_rule_t7():
    P = importlib.import_module(load_pkg().__name__ + ".protocol")
    m = np.zeros(1, dtype=P.TRAIL_MATCH_DTYPE)[0]
    m["ax"], m["ay"], m["dx"], m["dy"], m["dyaw"] = 1.0, 2.0, 0.15, -0.1, 3 * math.pi / 180
    for pose in ((1.0, 2.0, 0.5), (0.2, -3.1, -2.0), (4.0, 4.0, 3.0)):
        got = P.trail_move(m, *pose)
        assert tuple(float(v) for v in got) == TR.move(m, *pose)
    x, y, yaw = P.trail_move(m, np.array([1.0, 0.2]), np.array([2.0, -3.1]), np.array([0.5, -2.0]))
    assert (float(x[0]), float(y[0]), float(yaw[0])) == (1.15, 1.9, 0.5 + 3 * math.pi / 180)
    zero = np.zeros(1, dtype=P.TRAIL_MATCH_DTYPE)[0]
    zero["ax"], zero["ay"] = 1.0, 2.0
    assert tuple(float(v) for v in P.trail_move(zero, 0.25, 0.5, 1.0)) == (0.25, 0.5, 1.0)
