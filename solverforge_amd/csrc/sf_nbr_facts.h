// Facts of a presorted neighbour index (NbrIndex::keys: u16 entries, bit 15 = same distance as the entry before, 0xFFFF = past the row's
// finite entries) that hold for the life of a context: the index is built once, at sf_initialize, from an immutable matrix.  Host only.  The
// wave engine's run-time unit is compiled for them (sf_wave_spec.h); sf_debug_nbr_facts hands the reduction to the tests.
#pragma once
#include <stdint.h>

struct NbrFacts {
    int32_t tie_max = 64;   // the widest run of entries of one row that share a distance, saturated at 64 (0: no finite entry anywhere)
    int32_t rows_full = 0;  // every row has at least min(dim, 64) finite entries: no end mark in any row's first chunk
};                          // (the defaults: what a kernel may assume of an index nobody has looked at -- nothing)
// Pure host pass over `rows` rows of `dim` entries, folded into `f` (start from {0, 1}): the index may come down in pieces.
static inline void nbr_facts_rows(const uint16_t* keys, int64_t rows, int32_t dim, NbrFacts& f) {
    const int32_t full = dim < 64 ? dim : 64;
    for (int64_t r = 0; r < rows; ++r) {
        const uint16_t* row = keys + r * dim;
        int32_t finite = 0, run = 0;
        for (int32_t t = 0; t < dim && row[t] != 0xFFFFu; ++t) {  // (finite entries sort first)
            ++finite;
            run = (t > 0 && (row[t] & 0x8000u)) ? run + 1 : 1;
            if (run > f.tie_max) f.tie_max = run < 64 ? run : 64;
        }
        if (finite < full) f.rows_full = 0;
    }
}
