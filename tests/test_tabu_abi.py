"""CPU: the TabuSearch entry points are declared in include/solverforge_amd.h, listed in _lib.SYMBOLS and exported by the library, the
acceptor kind has its number, and the ctypes / numpy layouts are the header's (no compute calls: no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_solver_configure_tabu", "sf_get_tabu_state", "sf_debug_tabu_script")


def test_tabu_symbols_are_declared_listed_and_exported():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    header = open(os.path.join(ROOT, "include", "solverforge_amd.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"SF_ACCEPT_TABU_SEARCH\s*=\s*7\b", header) and re.search(r"#define\s+SF_TABU_MAX_TENURE_MOVE\s+64\b", header)


def test_tabu_layouts_are_the_header_s():
    import solverforge_amd as sfa
    from solverforge_amd import _lib

    assert sfa.Acceptor.TABU_SEARCH == 7
    assert ctypes.sizeof(_lib.TabuConfigStruct) == 4 * 8 + 2 * 4
    assert _lib.TABU_SIGNATURE_DTYPE.itemsize == 2 * 4 + 2 * 4 + 2 * 8 + 2 * 8
    assert _lib.TABU_RECORD_DTYPE.itemsize == 4 * 8 + 64 * 4 * 8 + 64 * _lib.TABU_SIGNATURE_DTYPE.itemsize + 8 + 4 + 4
    assert (_lib.TABU_STATE_FIXED, _lib.TABU_MAX_TENURE_MOVE, _lib.TABU_NO_TOKEN) == (16, 64, 0xFFFFFFFF)
