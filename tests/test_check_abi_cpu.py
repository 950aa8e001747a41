"""CPU-side check of the sweep-check entry points (include/quasar_slam.h, "sweep check"): the library exports the five symbols, the
binding declares them, and the structs and constants have the header's layout and values."""
import ctypes as C
import importlib
import os
import re

import numpy as np

import check_rules as CR
from conftest import ROOT, load_pkg

SYMBOLS = ("qs_check_sweeps", "qs_check_sweeps_device", "qs_ingest_sweeps_checked", "qs_ingest_sweeps_checked_device",
           "qs_last_sweep_checks")


def _header():
    return open(os.path.join(ROOT, "include", "quasar_slam.h")).read()


def _struct_fields(txt, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def test_library_exports_the_check_symbols():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    txt = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is not declared in the binding"
        assert re.search(r"\bint %s\(" % name, txt), f"{name} is not declared in the header"
    for name in ("qs_check_sweeps", "qs_ingest_sweeps_checked"):
        assert L.SIGNATURES[name] == L.SIGNATURES[name + "_device"]         # a twin takes the same arguments
    assert L.SIGNATURES["qs_check_sweeps"] == L.SIGNATURES["qs_match_sweeps"]
    assert L.SIGNATURES["qs_ingest_sweeps_checked"] == L.SIGNATURES["qs_ingest_sweeps_matched"]
    assert L.SIGNATURES["qs_last_sweep_checks"] == L.SIGNATURES["qs_last_sweep_matches"]


def test_structs_and_constants_match_the_header():
    pkg = load_pkg()
    L = importlib.import_module(pkg.__name__ + "._lib")
    P = importlib.import_module(pkg.__name__ + ".protocol")
    txt = _header()
    assert _struct_fields(txt, "qs_check_params") == [f[0] for f in L.QsCheckParams._fields_]
    assert _struct_fields(txt, "qs_sweep_check") == [f[0] for f in L.QsSweepCheck._fields_]
    assert C.sizeof(L.QsCheckParams) == 24 and L.QsCheckParams.min_checked.offset == 8 and L.QsCheckParams.reserved.offset == 20
    assert C.sizeof(L.QsSweepCheck) == 56 and L.QsSweepCheck.accepted_record.offset == 32 and L.QsSweepCheck.sin_yaw.offset == 40
    for dt in (P.CHECK_DTYPE, CR.CHECK_DTYPE):
        assert dt.itemsize == 56 and list(dt.names) == [f[0] for f in L.QsSweepCheck._fields_]
        assert [dt.fields[n][1] for n in dt.names] == [getattr(L.QsSweepCheck, n).offset for n in dt.names]
    want = dict(QS_BEAM_AGREE=0, QS_BEAM_NEARER=1, QS_BEAM_FARTHER=2, QS_BEAM_MISSED=3, QS_BEAM_UNSEEN=4, QS_BEAM_NO_RECORD=255,
                QS_CHECK_OK=0, QS_CHECK_NO_RECORD=1, QS_CHECK_UNDECIDED=2, QS_CHECK_CONTRADICTS=3)
    for name, v in want.items():
        assert int(re.search(r"#define %s (\d+)" % name, txt).group(1)) == v == getattr(L, name)
        assert getattr(P, name[3:]) == v
    assert (CR.AGREE, CR.NEARER, CR.FARTHER, CR.MISSED, CR.UNSEEN, CR.NO_RECORD_BEAM) == (0, 1, 2, 3, 4, 255)
    assert (CR.OK, CR.NO_RECORD, CR.UNDECIDED, CR.CONTRADICTS) == (0, 1, 2, 3)


def test_check_params_builder():
    pkg = load_pkg()
    L = importlib.import_module(pkg.__name__ + "._lib")
    P = importlib.import_module(pkg.__name__ + ".protocol")

    class Res:                                       # check_params reads nothing of the mapper but its resolution
        res = 0.05
    build = pkg.QuasarMapper.check_params
    p = build(Res(), None)
    assert (p.tol, p.min_checked, p.max_bad_percent, p.count_missed, p.reserved) == (2 * 0.05, 20, 30, 0, 0)
    assert (P.CHECK_TOL_CELLS, P.CHECK_MIN_CHECKED, P.CHECK_MAX_BAD_PERCENT, P.CHECK_COUNT_MISSED) == (2, 20, 30, 0)
    assert CR.params(0.05) == dict(tol=p.tol, min_checked=20, max_bad_percent=30, count_missed=0, reserved=0)
    p = build(Res(), dict(tol=0.25, count_missed=1), min_checked=7)
    assert (p.tol, p.min_checked, p.max_bad_percent, p.count_missed) == (0.25, 7, 30, 1)
    assert build(Res(), p) is p and isinstance(build(Res(), True), L.QsCheckParams)
    assert np.dtype(P.CHECK_DTYPE) == CR.CHECK_DTYPE
