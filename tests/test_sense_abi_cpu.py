"""CPU-side check of the sensing entry points (include/quasar_slam.h, "sensing a world"): the library exports the six symbols, the
binding declares them, and the parameter struct has the header's layout."""
import ctypes as C
import importlib
import os
import re

from conftest import ROOT, load_pkg

SYMBOLS = ("qs_sense_ranges", "qs_sense_ranges_device", "qs_sense_sweeps", "qs_sense_sweeps_device", "qs_sense_packets",
           "qs_sense_packets_device")


def test_library_exports_the_sensing_symbols():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    for name in SYMBOLS[::2]:
        assert L.SIGNATURES[name] == L.SIGNATURES[name + "_device"]         # a twin takes the same arguments


def test_params_struct_and_constants_match_the_header():
    pkg = load_pkg()
    L = importlib.import_module(pkg.__name__ + "._lib")
    txt = open(os.path.join(ROOT, "include", "quasar_slam.h")).read()
    assert int(re.search(r"#define QS_SENSE_MAX_CELLS (\d+)", txt).group(1)) == L.QS_SENSE_MAX_CELLS
    body = re.search(r"typedef struct qs_sense_params \{(.*?)\} qs_sense_params;", txt, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [f[0] for f in L.QsSenseParams._fields_]
    assert C.sizeof(L.QsSenseParams) == 48 and L.QsSenseParams.seed.offset == 24 and L.QsSenseParams.reserved.offset == 40
    p = pkg.QuasarMapper.sense_params(max_range=3.0, noise_amp=0.02, dropout=0.25, seed=(1 << 64) - 1, first_record=7, no_return=-1.0)
    assert (p.max_range, p.noise_amp, p.no_return, p.dropout_q16, p.seed, p.first_record) == (3.0, 0.02, -1.0, 16384, (1 << 64) - 1, 7)
    assert tuple(p.reserved) == (0, 0)
