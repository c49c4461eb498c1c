"""CPU: the Variable Neighborhood Descent entry points are declared in include/solverforge_amd.h, listed in _lib.SYMBOLS, exported by the
library and wrapped by the director; the phase's internal kind is no acceptor of the C ABI (no compute calls: no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_solver_configure_vnd", "sf_get_vnd_state", "sf_vnd_done_count")


def test_vnd_symbols_are_declared_listed_and_exported():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    header = open(os.path.join(ROOT, "include", "solverforge_amd.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert not re.search(r"SF_ACCEPT_\w+\s*=\s*8\b", header)  # the phase travels as an internal kind, not as an acceptor


def test_director_has_the_phase():
    import solverforge_amd as sfa

    for name in ("configure_vnd", "vnd_state", "vnd_done_count", "solve_vnd"):
        assert callable(getattr(sfa.GpuScoreDirector, name)), name
    assert 8 not in {v for k, v in vars(sfa.Acceptor).items() if not k.startswith("_")}
