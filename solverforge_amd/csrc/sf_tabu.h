// TabuSearch (acceptor 7; phase/localsearch/acceptor/tabu_search.rs:64-237, policy builder/acceptor.rs:383-405): the one acceptor that
// reads the move as well as its score.  Everything it needs is defined here once: the move signature in the device's packing
// (heuristic/move/change.rs:189-220, swap.rs:228-260, list_kernel/change.rs:155-204, list_kernel/swap.rs:110-155), the four memories,
// the decision of a chunk and the record of a step.  Callers: the fused scalar engine (k_scalar_search_wave), the wave engine's general
// replay (k_list_search_wave<L, true, 0>) and the generic engine (k_mixed_search_wave) -- TRACE instantiations only, like acceptors 5 and 6:
// DESIGN 24, 25 -- and sf_debug_tabu_script.
//
// Packing.  The reference hashes values and names (hash_str, hash_debug) and compares tokens and identities for EQUALITY only
// (TabuMemory::contains, :78-80), so any injective map of (scope, entity), (scope, value) and of the identity tuples decides the same:
//   token      an index into the replica's stamp table of its kind: scope base + entity index, scope base + value index + 1 (None = base + 0).
//              Scopes (MoveTabuScope, metadata.rs:32-58: one per declared planning variable) own disjoint index ranges.
//   identity   two words: (op << 56 | scope << 48 | f0 << 24 | f1, f2 << 48 | f3 << 24 | f4), every field below 2^24 (checked on the host at
//              phase start), op = 1 change (e, from, to) / 2 swap (min, max) / 3 list change (a, i, b, j', v) / 4 list swap ((a, i) <= (b, j)).
//              Values in a field are index + 1, None = 0.  Different ops never compare equal, as the reference's tuples of different
//              arity or operation tag never do.
//
// Entity and value memories are stamp tables, not rings.  A TabuMemory is a FIFO of the last min(tenure, pushes) pushes (record, :82-90;
// record_many pushes every token, duplicates included, :92-99); a token is in it exactly when its LATEST push is among those.  So each
// memory keeps a push counter npush and stamp[token] = the 1-based ordinal of the token's latest push (0 = never pushed):
//     tabu(token)  <=>  stamp[token] != 0  &&  npush - stamp[token] < tenure
// A candidate costs one gather per token whatever the tenure.  Stamps and counters are 64 bits: they do not wrap in any run.
// Move and undo memories are rings of identities (tenure <= TABU_MAX_TENURE_MOVE), slot = push ordinal % tenure.
//
// State.  TB_WORDS words at the head of the replica's acceptor-state row (SaParams::state, as AX_* in sf_step.h: SearchParams keeps its
// layout), and an arena of the replica in global memory, reached through the row: [entity stamps][value stamps][move ring][undo ring],
// a memory without a tenure takes no room.  Nothing changes inside a step: a chunk is decided against the state of step begin, and
// tabu_step_ended, by the one writer lane, records the applied move and the step score.
#pragma once
#include "sf_anneal.h"
#include "sf_common.h"

namespace sf {
//   TB_BEST    4  the acceptor's own best step score (not the solver's best solution)
//   TB_NPUSH   4  pushes into the entity / value / move / undo memory since phase start
//   TB_TENURE  4  their tenures, 0 = the policy has no such memory (from the host)
//   TB_ASPIRE  1  aspiration_enabled (from the host)
//   TB_ARENA   1  device address of the replica's arena (from the host)
//   TB_NENT    1  entity tokens of all scopes; TB_NVAL: value tokens (from the host)
enum : int { TB_BEST = 0, TB_NPUSH = 4, TB_TENURE = 8, TB_ASPIRE = 12, TB_ARENA = 13, TB_NENT = 14, TB_NVAL = 15, TB_WORDS = 16 };
enum : int { TB_MEM_ENTITY = 0, TB_MEM_VALUE = 1, TB_MEM_MOVE = 2, TB_MEM_UNDO = 3 };
static_assert(TB_WORDS <= SA_WORDS, "TabuSearch lives in the replica's acceptor-state row");
constexpr uint32_t TABU_NO_TOKEN = 0xFFFFFFFFu;
constexpr uint64_t TABU_MAX_TENURE_MOVE = 64;
constexpr uint64_t TABU_FIELD_LIMIT = 1ull << 24;  // entity indices, positions and value indices + 1 under TabuSearch
enum : uint64_t { TABU_OP_CHANGE = 1, TABU_OP_SWAP = 2, TABU_OP_LIST_CHANGE = 3, TABU_OP_LIST_SWAP = 4 };

// MoveTabuSignature (metadata.rs:72-79).  A token slot that the move does not fill is TABU_NO_TOKEN.
struct TabuSig {
    uint32_t ent[2], val[2];
    uint64_t mid[2], uid[2];
};
// one declared planning variable: its number in identities and where its tokens start in the two tables
struct TabuScope {
    uint32_t id, ent_base, val_base;
};

// word offset of memory `mem` in a replica's arena; mem = 4: the arena's size
__host__ __device__ inline uint64_t tabu_arena_offset(const uint64_t* row, int mem) {
    uint64_t o = 0;
    if (mem > TB_MEM_ENTITY && row[TB_TENURE + TB_MEM_ENTITY]) o += row[TB_NENT];
    if (mem > TB_MEM_VALUE && row[TB_TENURE + TB_MEM_VALUE]) o += row[TB_NVAL];
    if (mem > TB_MEM_MOVE) o += 2 * row[TB_TENURE + TB_MEM_MOVE];
    if (mem > TB_MEM_UNDO) o += 2 * row[TB_TENURE + TB_MEM_UNDO];
    return o;
}

__host__ __device__ inline void tabu_pack(uint64_t op, uint32_t scope, uint64_t f0, uint64_t f1, uint64_t f2, uint64_t f3, uint64_t f4, uint64_t* id) {
    id[0] = (op << 56) | ((uint64_t)scope << 48) | (f0 << 24) | f1;
    id[1] = (f2 << 48) | (f3 << 24) | f4;
}

// ---- signature builders: from the working solution BEFORE the move (phase/candidates.rs:190-196, phase/step.rs:135-142) ------------
// scalar change of entity e, from -> to (value indices, -1 = None): change.rs:189-220
__host__ __device__ inline void tabu_sig_change(const TabuScope& sc, uint32_t e, int32_t from, int32_t to, TabuSig& s) {
    s.ent[0] = sc.ent_base + e, s.ent[1] = TABU_NO_TOKEN;
    s.val[0] = sc.val_base + (uint32_t)(to + 1), s.val[1] = TABU_NO_TOKEN;
    tabu_pack(TABU_OP_CHANGE, sc.id, e, (uint64_t)(from + 1), (uint64_t)(to + 1), 0, 0, s.mid);
    tabu_pack(TABU_OP_CHANGE, sc.id, e, (uint64_t)(to + 1), (uint64_t)(from + 1), 0, 0, s.uid);
}
// scalar swap of entities l, r holding lv, rv: swap.rs:228-260 (destination values: rv then lv; the identity orders the pair)
__host__ __device__ inline void tabu_sig_swap(const TabuScope& sc, uint32_t l, uint32_t r, int32_t lv, int32_t rv, TabuSig& s) {
    s.ent[0] = sc.ent_base + l, s.ent[1] = sc.ent_base + r;
    s.val[0] = sc.val_base + (uint32_t)(rv + 1), s.val[1] = sc.val_base + (uint32_t)(lv + 1);
    tabu_pack(TABU_OP_SWAP, sc.id, l < r ? l : r, l < r ? r : l, 0, 0, 0, s.mid);
    s.uid[0] = s.mid[0], s.uid[1] = s.mid[1];
}
// list change of element v from (a, i) to (b, jadj), jadj = adjusted_destination (list_kernel/change.rs:28-34,155-204)
__host__ __device__ inline void tabu_sig_list_change(const TabuScope& sc, uint32_t a, uint32_t i, uint32_t b, uint32_t jadj, uint32_t v, TabuSig& s) {
    s.ent[0] = sc.ent_base + a, s.ent[1] = b != a ? sc.ent_base + b : TABU_NO_TOKEN;
    s.val[0] = sc.val_base + v + 1, s.val[1] = TABU_NO_TOKEN;
    tabu_pack(TABU_OP_LIST_CHANGE, sc.id, a, i, b, jadj, (uint64_t)v + 1, s.mid);
    tabu_pack(TABU_OP_LIST_CHANGE, sc.id, b, jadj, a, i, (uint64_t)v + 1, s.uid);
}
// list swap of (a, i) holding u with (b, j) holding w: list_kernel/swap.rs:110-155 (destination values: w then u)
__host__ __device__ inline void tabu_sig_list_swap(const TabuScope& sc, uint32_t a, uint32_t i, uint32_t u, uint32_t b, uint32_t j, uint32_t w, TabuSig& s) {
    s.ent[0] = sc.ent_base + a, s.ent[1] = b != a ? sc.ent_base + b : TABU_NO_TOKEN;
    s.val[0] = sc.val_base + w + 1, s.val[1] = sc.val_base + u + 1;
    const bool first = a < b || (a == b && i <= j);  // ordered_coordinate_pair (metadata.rs:175-181)
    tabu_pack(TABU_OP_LIST_SWAP, sc.id, first ? a : b, first ? i : j, first ? b : a, first ? j : i, 0, s.mid);
    s.uid[0] = s.mid[0], s.uid[1] = s.mid[1];
}
}  // namespace sf

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace sf {

// ---- phase start -----------------------------------------------------------------------------------------------------------------
// acceptor.phase_started(initial) (:198-204): memories cleared, best = initial.  The arena's words by every thread of the caller
// (`tid` of `nthreads`), the row's words by thread 0; tenures, flag, arena address and token counts are the host's and stay.
__device__ __forceinline__ void tabu_phase_started(uint64_t* row, const int64_t* initial, uint32_t tid, uint32_t nthreads) {
    uint64_t* arena = (uint64_t*)row[TB_ARENA];
    const uint64_t words = tabu_arena_offset(row, 4);
    for (uint64_t w = tid; w < words; w += nthreads) arena[w] = 0;
    if (tid == 0)
        for (int k = 0; k < 4; ++k) {
            row[TB_BEST + k] = (uint64_t)initial[k];
            row[TB_NPUSH + k] = 0;
        }
}

// ---- step begin: the state every candidate of the step is decided against, wave-uniform -------------------------------------------
template <int L>
struct TabuStep {
    ScoreV<L> best;
    uint64_t npush[4], tenure[4];
    const uint64_t* mem[4];
    bool aspire;
};
__device__ __forceinline__ uint64_t tabu_uni64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
template <int L>
__device__ __forceinline__ void tabu_step_begin(const uint64_t* row, TabuStep<L>& t) {
#pragma unroll
    for (int k = 0; k < L; ++k) t.best.v[k] = (int64_t)tabu_uni64(row[TB_BEST + k]);
    const uint64_t* arena = (const uint64_t*)tabu_uni64(row[TB_ARENA]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        t.npush[q] = tabu_uni64(row[TB_NPUSH + q]);
        t.tenure[q] = tabu_uni64(row[TB_TENURE + q]);
        t.mem[q] = arena + tabu_uni64(tabu_arena_offset(row, q));
    }
    t.aspire = tabu_uni64(row[TB_ASPIRE]) != 0;
}

// is_tabu (:162-173) of one candidate; called by every lane of the wave (the ring loops are wave-uniform), `on` = the lane holds a signature
template <int L>
__device__ __forceinline__ bool tabu_is_tabu(const TabuStep<L>& t, bool on, const TabuSig& s) {
    bool tabu = false;
#pragma unroll
    for (int q = 0; q < 2; ++q) {  // entity memory, then value memory
        if (!t.tenure[q]) continue;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t tok = q ? s.val[k] : s.ent[k];
            if (on && tok != TABU_NO_TOKEN) {
                const uint64_t st = t.mem[q][tok];
                tabu = tabu || (st != 0 && t.npush[q] - st < t.tenure[q]);  // never pushed: not tabu, however few pushes there were
            }
        }
    }
#pragma unroll
    for (int q = 2; q < 4; ++q) {  // move memory, then undo memory: the candidate's move_id against both (:171-172)
        const uint64_t live = t.npush[q] < t.tenure[q] ? t.npush[q] : t.tenure[q];
        for (uint64_t k = 0; k < live; ++k) tabu = tabu || (on && t.mem[q][2 * k] == s.mid[0] && t.mem[q][2 * k + 1] == s.mid[1]);
    }
    return tabu;
}

// is_accepted (:181-196): aspirational (aspiration_enabled && sc > best, strict) or not tabu; the last step score is not read
template <int L>
__device__ __forceinline__ bool tabu_accepts(const TabuStep<L>& t, bool consult, const ScoreV<L>& sc, const TabuSig& s) {
    const bool aspirational = t.aspire && score_cmp<L>(sc, t.best) > 0;
    const bool tabu = tabu_is_tabu<L>(t, consult && !aspirational, s);
    return consult && !tabu;
}

// ---- step end ----------------------------------------------------------------------------------------------------------------------
// step_ended(step_score, accepted signature) (:214-236) by the one lane `writer`: the applied move's tokens and identities are pushed
// (`sig` = nullptr: the step applied nothing), then best = step score where it beats best strictly -- on every step
template <int L>
__device__ __forceinline__ void tabu_step_ended(uint64_t* row, bool writer, const int64_t* cur, const TabuSig* sig) {
    if (!writer) return;
    uint64_t* arena = (uint64_t*)row[TB_ARENA];
    if (sig) {
        for (int q = 0; q < 2; ++q) {  // record_many: every token in order, each a push of its own
            if (!row[TB_TENURE + q]) continue;
            uint64_t* stamp = arena + tabu_arena_offset(row, q);
            for (int k = 0; k < 2; ++k) {
                const uint32_t tok = q ? sig->val[k] : sig->ent[k];
                if (tok != TABU_NO_TOKEN) stamp[tok] = ++row[TB_NPUSH + q];
            }
        }
        for (int q = 2; q < 4; ++q) {
            const uint64_t tenure = row[TB_TENURE + q];
            if (!tenure) continue;
            uint64_t* ring = arena + tabu_arena_offset(row, q);
            const uint64_t slot = row[TB_NPUSH + q] % tenure;  // full: the oldest entry's slot
            const uint64_t* id = q == TB_MEM_MOVE ? sig->mid : sig->uid;
            ring[2 * slot] = id[0], ring[2 * slot + 1] = id[1];
            row[TB_NPUSH + q] += 1;
        }
    }
    ScoreV<L> b, c;
#pragma unroll
    for (int k = 0; k < L; ++k) b.v[k] = (int64_t)row[TB_BEST + k], c.v[k] = cur[k];
    if (score_cmp<L>(c, b) > 0) {
#pragma unroll
        for (int k = 0; k < L; ++k) row[TB_BEST + k] = (uint64_t)cur[k];
    }
}

}  // namespace sf
#endif  // __HIPCC__
