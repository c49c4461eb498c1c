// Seam of the scalar construction phase (sf_construct_scalar): what k_scalar_construct needs beside the ScalarModel travels in a
// kernel-argument struct of its own (as the time-window tables of the 2-opt phase do, sf_kopt_tw.hip), so ScalarModel and SearchParams
// stay as they are and no other kernel sees the phase.  The kernel is compiled in a unit of its own (sf_tu_scalar_construct.hip); the
// C-ABI unit sees this header only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sf {

struct ScalarModel;

enum ScalarConstructForager : int32_t { SCF_FIRST_FIT = 0, SCF_BEST_FIT = 1, SCF_WEAKEST_FIT = 2, SCF_STRONGEST_FIT = 3 };

struct ScalarConstructArgs {
    const uint32_t* order;  // [n_order] entities in placement order (stable sort by the entity key); null = canonical (0, 1, ..)
    int32_t n_order;
    int32_t forager;        // ScalarConstructForager
    int32_t baseline;       // keep-current is a choice: the variable allows unassigned AND the obligation is PreserveUnassigned
    int32_t live_refresh;   // the placement cursor restarts at the head of the order after every step
    uint32_t limit;         // value_candidate_limit: the canonical value list is cut to its first `limit` values (0xFFFFFFFF = none)
    int32_t range_n;        // candidates of an entity without value lists: min(n_values, limit)
    const uint32_t* c_off;  // [n + 1] candidate values per entity: the class's value lists, or their copy in value-key order (rows cut to
    const int32_t* c_val;   //         the limit first); null = the countable range
    const int32_t* perm;    // [range_n] the countable range in value-key order; null = canonical
    const int64_t* vkey;    // [n_values] strength of a value (weakest / strongest fit)
    uint32_t* kept;         // [R][n] entities that kept current, in placement order (live refresh with a baseline), else null
    uint64_t* stats;        // [R][SF_STATS_WORDS]
};

hipError_t launch_tu_scalar_construct(const ScalarModel& m, const ScalarConstructArgs& a, int n_replicas, size_t lds, hipStream_t stream);

}  // namespace sf
