// A fact of the compact u16 distance matrix (ListModel::mat16) that holds for the life of a context: the copy is built once, at sf_initialize,
// from an immutable matrix.  Host only.  The wave engine's run-time unit is compiled for it (sf_wave_spec.h); sf_debug_mat_sym hands
// the reduction to the tests.  The fact is taken on the words the kernel reads, not on the 64-bit entries they were made from: two entries
// that differ but compress to the same word (both not finite, say) are the same leg to the kernel.
#pragma once
#include <stdint.h>

// The word k_mat_compress16 stores for a 64-bit entry: the value itself below 0xFFFF, else 0xFFFF = not finite.
static inline uint16_t mat16_word(int64_t v) { return (v >= 0 && v < 0xFFFF) ? (uint16_t)v : (uint16_t)0xFFFFu; }

// Pure host pass: 1 when mat[a][b] == mat[b][a] for every pair of the dim x dim matrix, the not-finite word included (tiles of 64 x 64: the
// transposed reads stay in cache).  The renumbered copy (ListModel::perm) is the same matrix under one permutation of rows and columns: it is
// symmetric exactly when this one is.
static inline int32_t mat16_symmetric(const uint16_t* mat, int32_t dim) {
    constexpr int32_t T = 64;
    for (int32_t a0 = 0; a0 < dim; a0 += T)
        for (int32_t b0 = a0; b0 < dim; b0 += T) {
            const int32_t a1 = a0 + T < dim ? a0 + T : dim, b1 = b0 + T < dim ? b0 + T : dim;
            for (int32_t a = a0; a < a1; ++a)
                for (int32_t b = (b0 > a + 1 ? b0 : a + 1); b < b1; ++b)
                    if (mat[(size_t)a * dim + b] != mat[(size_t)b * dim + a]) return 0;
        }
    return 1;
}
