"""Trail relocalisation: the ABI of the two entry points -- symbols, the 88-byte result against protocol.TRAIL_RELOC_DTYPE, the
restatement's and qs_group_reloc's prefix, the ctypes signatures, and the header's text of the rule."""
import ctypes as C
import importlib
import os
import re

import reloc_group_rules as GR
import trail_reloc_rules as KR
from conftest import ROOT, load_pkg

NEW_SYMBOLS = ("qs_relocalise_trails", "qs_relocalise_trails_device")


def test_symbols_struct_and_signatures():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    P = importlib.import_module(pkg.__name__ + ".protocol")
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    vp, sz = C.c_void_p, C.c_size_t
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        # ctx, params, pkts, n, stride, lens, gsize, n_groups, travel, out, rot_out: qs_match_trails' shape
        assert L.SIGNATURES[name] == (C.c_int32, [vp, vp, vp, sz, sz, vp, vp, sz, C.c_double, vp, vp])
        assert L.SIGNATURES[name] == L.SIGNATURES["qs_match_trails"]
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert re.search(r"typedef struct qs_trail_reloc \{\s*int32_t gx, gy, j, score, hits;\s*int32_t gx2, gy2, j2, score2;\s*"
                     r"int32_t status;\s*uint8_t records, accepted, agent, pad;\s*int32_t anchor;\s*double x, y, yaw, ax, ay;\s*"
                     r"\} qs_trail_reloc;", code)
    assert C.sizeof(L.QsTrailReloc) == 10 * 4 + 4 + 4 + 5 * 8 == 88 == P.TRAIL_RELOC_DTYPE.itemsize == KR.TRAIL_RELOC_DTYPE.itemsize
    assert P.TRAIL_RELOC_DTYPE == KR.TRAIL_RELOC_DTYPE
    for f in KR.FIELDS + ("pad",):
        assert getattr(L.QsTrailReloc, f).offset == P.TRAIL_RELOC_DTYPE.fields[f][1], f
    # offsets 0..41 and 48..71 are qs_group_reloc's
    for f in ("gx", "gy", "j", "score", "hits", "gx2", "gy2", "j2", "score2", "status", "records", "accepted", "x", "y", "yaw"):
        assert getattr(L.QsTrailReloc, f).offset == getattr(L.QsGroupReloc, f).offset == GR.GROUP_DTYPE.fields[f][1], f
    assert (L.QsTrailReloc.accepted.offset, L.QsTrailReloc.agent.offset, L.QsTrailReloc.pad.offset) == (41, 42, 43)
    assert (L.QsTrailReloc.anchor.offset, L.QsTrailReloc.x.offset, L.QsTrailReloc.ax.offset, L.QsTrailReloc.ay.offset) == (44, 48, 72, 80)
    assert KR.MAX_RECORDS == P.TRAIL_MAX_RECORDS == L.QS_TRAIL_MAX_RECORDS == 64
    # the reference's filter at the default travel and 5 cm cells lies inside K8; the 3.0 m filter needs a travel of 2.8 m
    prm = dict(radius=P.RELOC_RADIUS, n_rot=P.RELOC_N_ROT, sep=P.RELOC_SEP, sep_rot=P.RELOC_SEP_ROT)
    assert KR.limit_ok(prm, P.MAX_DIST_M, P.TRAIL_TRAVEL, P.GRID_RESOLUTION)
    assert KR.limit_ok(prm, 3.0, 2.8, 0.05) and not KR.limit_ok(prm, 3.0, 2.85, 0.05)


def test_the_header_states_the_rule_and_its_limits():
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    sec = txt[txt.index("---- trail relocalisation"):txt.index("---- OccupancyGrid object API")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for rule in ("K1.", "K2.", "K3.", "K4.", "K5.", "K6.", "K7.", "K8."):
        assert rule in sec
    for words in ("16 + 2 * (ceil((max_dist + travel) / res) + radius + 1) <= 255", "travel finite and >= 0", "stride >= 41",
                  "gsize[g] in 1..QS_TRAIL_MAX_RECORDS", "QS_E_INVAL", "A sharded context refuses", "write nothing to the context",
                  "a HOST array", "anchor = -1", "min_dist < d <= max_dist", "qx = (X_k - X_a) + d * ux",
                  "M = ceil((max_dist + travel) / res) + 1", "offset and drift are NOT read", "tests/trail_reloc_rules.py",
                  "(x + (C (px - ax) - S (py - ay)),  y + (S (px - ax) + C (py - ay)),  pyaw + yaw)"):
        assert words in flat, words


def test_the_python_layer_has_the_calls():
    pkg = load_pkg()
    for name in ("relocalise_trails", "relocalise_trails_device"):
        assert callable(getattr(pkg.QuasarMapper, name))
