"""CPU: the scalar ruin-and-recreate entry points are declared in include/solverforge_amd.h, listed in _lib.SYMBOLS, exported by the library
and wrapped by the director; the new enum values collide with no existing one (no compute calls: no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_selector_add_scalar_ruin", "sf_get_scalar_ruin_table")


def _header():
    return open(os.path.join(ROOT, "include", "solverforge_amd.h")).read()


def _enum(header, name):
    body = re.search(r"typedef enum %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"(SF_\w+)\s*=\s*(-?\d+)", body)}


def test_symbols_are_declared_listed_and_exported():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("SF_SEL_SCALAR_RUIN", "SF_MOVE_SCALAR_RUIN", "sf_recreate_heuristic"):
        assert name in integration, name


def test_enum_values_are_distinct():
    header = _header()
    selectors, moves, recreate = _enum(header, "sf_selector_kind"), _enum(header, "sf_move_kind"), _enum(header, "sf_recreate_heuristic")
    assert selectors["SF_SEL_SCALAR_RUIN"] == 32768 and moves["SF_MOVE_SCALAR_RUIN"] == 11
    assert len(set(selectors.values())) == len(selectors) and len(set(moves.values())) == len(moves)
    assert all(v & (v - 1) == 0 for v in selectors.values())  # one bit each: leaves are named as a mask
    assert recreate == {"SF_RECREATE_FIRST_FIT": 0, "SF_RECREATE_CHEAPEST_INSERTION": 1}


def test_director_has_the_leaf():
    import solverforge_amd as sfa
    from solverforge_amd.director import MoveKind, Recreate, SelectorKind

    for name in ("add_scalar_ruin_selector", "scalar_ruin_table"):
        assert callable(getattr(sfa.GpuScoreDirector, name)), name
    assert SelectorKind.SCALAR_RUIN == 32768 and MoveKind.SCALAR_RUIN == 11 and (Recreate.FIRST_FIT, Recreate.CHEAPEST_INSERTION) == (0, 1)
    kinds = [v for k, v in vars(MoveKind).items() if not k.startswith("_")]
    assert len(set(kinds)) == len(kinds)
