"""sf_generic_launch_bits (include/solverforge_amd.h) and its decoder in the Python binding agree, field by field (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_bits():
    text = open(os.path.join(ROOT, "include", "solverforge_amd.h")).read()
    body = re.search(r"typedef enum sf_generic_launch_bits \{(.*?)\} sf_generic_launch_bits;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = {}
    for name, expr in re.findall(r"(SF_GEN_\w+)\s*=\s*([^,\n]+)", body):
        m = re.fullmatch(r"(\d+)(?:\s*<<\s*(\d+))?", expr.strip())  # an integer literal, or one shifted by another
        assert m, (name, expr)
        out[name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


def test_header_fields_do_not_overlap_and_keep_the_old_bits():
    b = _header_bits()
    assert (b["SF_GEN_FAST"], b["SF_GEN_NODE_GLOBAL"], b["SF_GEN_RING32"], b["SF_GEN_RUIN_SHIFT"], b["SF_GEN_VT_SHIFT"]) == (1, 2, 4, 4, 8)
    fields = [(0, 1), (1, 1), (2, 1), (b["SF_GEN_RUIN_SHIFT"], 2), (b["SF_GEN_VT_SHIFT"], 4), (b["SF_GEN_PREC_STATIC_SHIFT"], 2),
              (b["SF_GEN_PREC_GROUPS_SHIFT"], 5), (b["SF_GEN_LEVELS_SHIFT"], 3)]
    for flag in ("SF_GEN_PREC", "SF_GEN_PREC_LDS", "SF_GEN_PREC_OCC", "SF_GEN_PREC_SWEEP", "SF_GEN_PREC_INC", "SF_GEN_RUIN_INST"):
        assert b[flag] & (b[flag] - 1) == 0
        fields.append((b[flag].bit_length() - 1, 1))
    used = 0
    for shift, width in fields:
        mask = ((1 << width) - 1) << shift
        assert used & mask == 0, (shift, width)
        used |= mask
    assert used < 1 << 31  # the word is an int32 whose -1 means "no launch yet"


def test_decoder_reads_every_field():
    from solverforge_amd.director import decode_generic_launch_bits as dec

    b = _header_bits()
    zero = dec(0)
    assert not any(zero.values())
    single = {"SF_GEN_FAST": "fast", "SF_GEN_NODE_GLOBAL": "node_global", "SF_GEN_RING32": "ring32", "SF_GEN_PREC": "prec", "SF_GEN_PREC_LDS": "prec_lds",
              "SF_GEN_PREC_OCC": "prec_occ", "SF_GEN_PREC_SWEEP": "prec_sweep", "SF_GEN_PREC_INC": "prec_inc", "SF_GEN_RUIN_INST": "ruin_inst"}
    for flag, key in single.items():
        got = dec(b[flag])
        assert got[key] is True and sum(bool(v) for v in got.values()) == 1, flag
    multi = {"SF_GEN_RUIN_SHIFT": ("ruin", (1, 2, 3)), "SF_GEN_VT_SHIFT": ("value_bytes", (1, 2)), "SF_GEN_PREC_STATIC_SHIFT": ("prec_static", (1, 2)),
             "SF_GEN_PREC_GROUPS_SHIFT": ("prec_groups", (2, 4, 8, 16)), "SF_GEN_LEVELS_SHIFT": ("levels", (2, 4))}
    for shift, (key, values) in multi.items():
        for v in values:
            got = dec(v << b[shift])
            assert got[key] == v and sum(bool(x) for x in got.values()) == 1, (shift, v)
    # a MODE 2 PREC + RUIN launch of the two-level template: scratch in LDS, slim copy, no groups, 2-byte values
    word = (b["SF_GEN_PREC"] | b["SF_GEN_PREC_LDS"] | 2 << b["SF_GEN_PREC_STATIC_SHIFT"] | b["SF_GEN_PREC_OCC"] | b["SF_GEN_RUIN_INST"] |
            2 << b["SF_GEN_LEVELS_SHIFT"] | 2 << b["SF_GEN_VT_SHIFT"] | 1 << b["SF_GEN_RUIN_SHIFT"])
    assert dec(word) == {"fast": False, "node_global": False, "ring32": False, "ruin": 1, "value_bytes": 2, "prec": True, "prec_lds": True,
                         "prec_static": 2, "prec_groups": 0, "prec_occ": True, "prec_sweep": False, "prec_inc": False, "ruin_inst": True, "levels": 2}
