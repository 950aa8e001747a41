"""CPU-side check of the sweep veil's entry points (include/quasar_slam.h, rules S0-S8): the library exports the three symbols, the
binding declares them with the argument lists of their packet counterparts, and the header states the rule."""
import importlib
import os
import re

from conftest import ROOT, load_pkg

SYMBOLS = ("qs_set_bot_veil_sweeps", "qs_bot_veil_sweeps", "qs_last_sweeps_veiled")


def _header():
    return open(os.path.join(ROOT, "include", "quasar_slam.h")).read()


def test_library_exports_the_sweep_veil_symbols():
    pkg = load_pkg()
    pkg.build()
    lib = pkg.load()
    L = importlib.import_module(pkg.__name__ + "._lib")
    txt = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is not declared in the binding"
        assert re.search(r"\bint %s\(" % name, txt), f"{name} is not declared in the header"
    assert L.SIGNATURES["qs_set_bot_veil_sweeps"] == L.SIGNATURES["qs_set_bot_veil"]
    assert L.SIGNATURES["qs_bot_veil_sweeps"] == L.SIGNATURES["qs_bot_veil"]
    assert L.SIGNATURES["qs_last_sweeps_veiled"] == L.SIGNATURES["qs_last_veiled"]


def test_header_states_the_rule():
    txt = _header()
    for k in range(9):
        assert re.search(r"\*\s+S%d  " % k, txt), f"S{k} is missing from the header"
    assert "n x 181" in txt and "every sweep entry\n *       point (sweep bots reach the table through qs_bot_veil_place only)" not in txt


def test_python_layer_has_the_methods():
    pkg = load_pkg()
    import inspect
    sig = inspect.signature(pkg.QuasarMapper.set_bot_veil)
    P = importlib.import_module(pkg.__name__ + ".protocol")
    assert sig.parameters["sweeps"].default is None and sig.parameters["radius"].default == P.BOT_VEIL_RADIUS
    assert callable(pkg.QuasarMapper.bot_veil_sweeps) and callable(pkg.QuasarMapper.last_sweeps_veiled)
    sim = importlib.import_module(pkg.__name__ + ".sim")
    assert list(inspect.signature(sim.body_sweep_ranges).parameters) == list(inspect.signature(sim.body_ranges).parameters)
