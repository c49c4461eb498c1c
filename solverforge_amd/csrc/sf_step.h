// The local-search step around one 64-candidate replay chunk (lanes = pulls in union cursor order).  Two groups of rules, with different callers:
//
// 1. The acceptors without state of their own (is_accepted of hill_climbing.rs, late_acceptance.rs:89-125,
//    diversified_late_acceptance.rs:139-159), the forager's pick (forager.rs:143-420, forager/improving.rs:92-95,205-208), and what a step
//    does before and after its candidates (step.rs:53-74,216-221, diversified_late_acceptance.rs:161-170, scope_progress.rs:89-107):
//    step_begin, acceptor_accepts, forager_pick_update, step_improved, acceptor_step_ended.  Called by the block engine only.  The wave
//    engine's general replay (sf_list_wave.hip), the generic engine (sf_mixed_wave.hip), the fused scalar engine (k_scalar_search_wave)
//    and the provider step (k_scalar_step_decide) hold their own copies of these rules (DESIGN 23 says why): a fix to the tie-break has to
//    be made there too.  A chunk goes through
//        acceptor_accepts (or sa_decide, sf_anneal.h) -> forager_chunk_cut (sf_forager.h) -> [sa_commit] -> acc &= lane < nconsumed
//        -> forager_pick_update -> forager_quits
// 2. GreatDeluge (5, great_deluge.rs:89-129) and StepCountingHillClimbing (6, step_counting.rs:85-129): acceptor_phase_started,
//    ax_step_begin, ax_accepts, ax_step_ended.  Defined here alone and called from all five places.  In the four fused engines the calls
//    are compiled into the TRACE instantiations only, and a launch under these two acceptors takes those: the untraced
//    kernels, which every other policy runs, hold none of this code.
// 3. The Variable Neighborhood Descent phase (phase/localsearch/vnd/phase.rs:31-167 solve_vnd_with_resources, :181-404
//    find_best_improving_move; neighbourhoods compiled with SelectionOrder::Original, runtime/compiler/local_search.rs:55-89):
//    vnd_phase_started, vnd_step_begin, vnd_accepts, vnd_step_ended.  Called by the generic engine's TRACE instantiations.
//
// Nothing here owns memory: the callers keep their registers and LDS words and pass references or row pointers.  SimulatedAnnealing
// (sa_decide / sa_commit / sa_step_ended) and the statistics counters stay with the kernels.
#pragma once
#include "sf_anneal.h"
#include "sf_common.h"
#include "sf_forager.h"

namespace sf {
// State of acceptors 5 and 6: AX_WORDS words per replica at the head of the replica's acceptor-state row (SaParams::state, [R][SA_WORDS]; one
// acceptor runs at a time, and SimulatedAnnealing's words are rewritten at every phase start).  The search kernels' argument block keeps
// its layout this way, so the kernels that never run these acceptors load every field from the offset they had.
//   AX_LEVEL  4  GreatDeluge: the water level.  StepCounting: the best step score since the count was reset (the acceptor's own "best")
//   AX_INCR   4  GreatDeluge: |initial score| x rain_speed per level, fixed at phase start.  StepCounting: zeros
//   AX_SINCE  1  StepCounting: steps since that best score improved.  GreatDeluge: 0
//   AX_PARAM  1  from the host at phase start: rain_speed (f64 bits) / step_count_limit
enum : int { AX_LEVEL = 0, AX_INCR = 4, AX_SINCE = 8, AX_PARAM = 9, AX_WORDS = 10 };
static_assert(AX_WORDS <= SA_WORDS, "acceptors 5 and 6 live in the replica's acceptor-state row");
// State of the Variable Neighborhood Descent phase (group 3 below), in the same words: no acceptor runs under it.
//   VND_K     the neighbourhood of the next step, 0 .. n
//   VND_N     the number of neighbourhoods, from the host at phase start
//   VND_DONE  k == n: the replica runs no further step (it survives launch boundaries; a new phase start clears it)
//   VND_IDLE  steps that found nothing
enum : int { VND_K = 0, VND_N = 1, VND_DONE = 2, VND_IDLE = 3, VND_WORDS = 4 };
// The phase travels through SearchParams::acceptor as this kind.  It is no acceptor of the C ABI (sf_solver_configure refuses it): only
// sf_solver_configure_vnd sets it.
enum : int { VND_KIND = 8 };
}  // namespace sf

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace sf {

// ---- wave64 primitives -------------------------------------------------------------------------------------------------------
// A value every lane holds alike, said to the compiler: it moves to scalar registers.  Changes no value.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | (uint64_t)uni((uint32_t)v);
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl(lo, src);
    hi = __shfl(hi, src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_xor(lo, m);
    hi = __shfl_xor(hi, m);
    return ((uint64_t)hi << 32) | lo;
}
template <int L>
__device__ __forceinline__ ScoreV<L> wave_max_score(ScoreV<L> s, bool valid) {
    // lexicographic max across the wave; invalid lanes contribute -inf
    if (!valid) {
#pragma unroll
        for (int k = 0; k < L; ++k) s.v[k] = INT64_MIN;
    }
#pragma unroll
    for (int mlane = 32; mlane >= 1; mlane >>= 1) {
        ScoreV<L> o;
#pragma unroll
        for (int k = 0; k < L; ++k) o.v[k] = (int64_t)shfl_xor_u64((uint64_t)s.v[k], mlane);
        if (score_cmp<L>(o, s) > 0) s = o;
    }
    return s;
}

template <int L>
__device__ __forceinline__ ScoreV<L> score_of(const int64_t* w) {
    ScoreV<L> s;
#pragma unroll
    for (int k = 0; k < L; ++k) s.v[k] = w[k];
    return s;
}

// ---- step begin ----------------------------------------------------------------------------------------------------------------
// The thresholds of the step: `late` = the LateAcceptance history slot of this step (la_row, read by acceptors 1 and 4), `dla_thr` =
// DiversifiedLateAcceptance's best step score of the phase (dla_row) minus its tolerance band; both `late` where the acceptor has none.
template <int L>
__device__ __forceinline__ void step_begin(int acceptor, const int64_t* la_row, const int64_t* dla_row, double dla_tolerance, ScoreV<L>& late,
                                           ScoreV<L>& dla_thr) {
#pragma unroll
    for (int k = 0; k < L; ++k) late.v[k] = 0;
    if (acceptor == 1 || acceptor == 4) {
#pragma unroll
        for (int k = 0; k < L; ++k) late.v[k] = (int64_t)uni64((uint64_t)la_row[k]);
    }
    dla_thr = late;
    if (acceptor == 4) {
        ScoreV<L> db;
#pragma unroll
        for (int k = 0; k < L; ++k) db.v[k] = (int64_t)uni64((uint64_t)dla_row[k]);
        dla_thr = dla_threshold<L>(db, dla_tolerance);
    }
}

// Acceptors 5 and 6 (ax_row, read wave-uniform) say their rule as one threshold and one flag, so a candidate costs two compares:
//     accepted  <=>  sc > cur  ||  (thr_on && sc >= late)
//   GreatDeluge     late = the water level, thr_on
//   StepCounting    since < limit: every candidate passes, late = the least score, thr_on;  else thr_on is off: sc > cur alone
template <int L>
__device__ __forceinline__ void ax_step_begin(int acceptor, const uint64_t* ax_row, ScoreV<L>& late, bool& thr_on) {
    thr_on = true;
    if (acceptor == 5) {
#pragma unroll
        for (int k = 0; k < L; ++k) late.v[k] = (int64_t)uni64(ax_row[AX_LEVEL + k]);
    }
    if (acceptor == 6) {
        thr_on = uni64(ax_row[AX_SINCE]) < uni64(ax_row[AX_PARAM]);
#pragma unroll
        for (int k = 0; k < L; ++k) late.v[k] = INT64_MIN;
    }
}

// ---- acceptor --------------------------------------------------------------------------------------------------------------------
// is_accepted of HillClimbing (0), LateAcceptance (1) and DiversifiedLateAcceptance (4) for a candidate that reaches the acceptor
// (`consult`: doable, and not held back by a gate of evaluation.rs:75-113); `cur` = the last step score.
template <int L>
__device__ __forceinline__ bool acceptor_accepts(int acceptor, bool consult, const ScoreV<L>& sc, const ScoreV<L>& cur, const ScoreV<L>& late,
                                                 const ScoreV<L>& dla_thr) {
    bool acc = false;
    if (consult) {
        if (acceptor == 0)
            acc = score_cmp<L>(sc, cur) > 0;
        else if (acceptor == 1)
            acc = score_cmp<L>(sc, cur) >= 0 || score_cmp<L>(sc, late) >= 0;
        else if (acceptor == 4)
            acc = score_cmp<L>(sc, cur) >= 0 || score_cmp<L>(sc, late) >= 0 || score_cmp<L>(sc, dla_thr) >= 0;
    }
    return acc;
}
// is_accepted of GreatDeluge (5) and StepCountingHillClimbing (6): the first compare is strict (great_deluge.rs:90-106,
// step_counting.rs:86-99); `late` / `thr_on` from ax_step_begin
template <int L>
__device__ __forceinline__ bool ax_accepts(bool consult, const ScoreV<L>& sc, const ScoreV<L>& cur, const ScoreV<L>& late, bool thr_on) {
    return consult && (score_cmp<L>(sc, cur) > 0 || (thr_on && score_cmp<L>(sc, late) >= 0));
}

// ---- forager: who is the pick after this chunk --------------------------------------------------------------------------------
// `acc` = accepted and consumed (after forager_chunk_cut and the re-masking), `accmask` its ballot.  Returns the lane whose candidate
// becomes the step's pick, or -1 where the pick stays; the caller shuffles its own move words from that lane (two words and a leaf,
// three in the generic engine, an index in the provider step), so each keeps them in the registers it chose.  `best`, `equal_count`
// (EQ: the caller's width; the reservoir hashes it as 64 bits) and `has_best` are the forager's running state of the step, wave-uniform.
//   improving_pick   BestCandidate::replace by the candidate that ends the step: lane nconsumed - 1
//   FirstAccepted    the first accepted lane, once
//   otherwise        the lexicographic maximum of the accepted lanes; among equals (of this chunk and the ones before) the first stays
//                    unless random_ties lets the reservoir move the pick to a later one (forager.rs:143-148,245-263)
// The test in front of the maximum only skips work: without an accepted lane at or above `best` the maximum is below it.
template <int L, typename EQ>
__device__ __forceinline__ int forager_pick_update(int forager, bool random_ties, uint64_t sseed, bool acc, uint64_t accmask, uint32_t nconsumed,
                                                   bool improving_pick, const ScoreV<L>& sc, ScoreV<L>& best, EQ& equal_count, int& has_best) {
    int sel = -1;
    if (!accmask) return sel;
    if (improving_pick) {
        sel = (int)nconsumed - 1;
#pragma unroll
        for (int k = 0; k < L; ++k) best.v[k] = (int64_t)uni64(shfl_u64((uint64_t)sc.v[k], sel));
        equal_count = 1;
        has_best = 1;
    } else if (forager == FORAGER_FIRST_ACCEPTED) {
        if (!has_best) {
            sel = __ffsll((unsigned long long)accmask) - 1;
#pragma unroll
            for (int k = 0; k < L; ++k) best.v[k] = (int64_t)uni64(shfl_u64((uint64_t)sc.v[k], sel));
            has_best = 1;
        }
    } else if (!has_best || __ballot(acc && score_cmp<L>(sc, best) >= 0)) {
        const ScoreV<L> M = wave_max_score<L>(sc, acc);
        const int cm = has_best ? score_cmp<L>(M, best) : 1;
        if (cm >= 0) {
            const bool newmax = cm > 0;
            const EQ eq_base = newmax ? 0 : equal_count;
            const bool in_eq = acc && score_cmp<L>(sc, M) == 0;
            const uint64_t eq = __ballot(in_eq);
            const uint32_t rank = forager_mbcnt64(eq) + 1u;  // this lane's place among the chunk's equals, from 1
            const uint64_t cntq = (uint64_t)eq_base + rank;
            const bool pick = in_eq && ((newmax && rank == 1) || (random_ties && cntq > 1 && reservoir_pick(sseed, cntq)));
            const uint64_t pm = __ballot(pick);
            if (pm) sel = 63 - __clzll((unsigned long long)pm);
#pragma unroll
            for (int k = 0; k < L; ++k) best.v[k] = (int64_t)uni64((uint64_t)M.v[k]);
            equal_count = eq_base + (EQ)__popcll(eq);
            has_best = 1;
        }
    }
    return sel;
}

// ---- step end ------------------------------------------------------------------------------------------------------------------
// update_best_solution's test (scope_progress.rs:89-107): the step applied a move and its score beats the best one strictly
template <int L>
__device__ __forceinline__ bool step_improved(bool applied, const int64_t* cur, const int64_t* best_sol) {
    return applied && score_cmp<L>(score_of<L>(cur), score_of<L>(best_sol)) > 0;
}

// ---- phase start ---------------------------------------------------------------------------------------------------------------
// acceptor.phase_started(initial_score) of acceptors 5 and 6, by one thread of the phase-start kernels; `initial` and the state rows are
// four words wide whatever the score's width (levels it does not have are zero and stay zero).
//   GreatDeluge (great_deluge.rs:108-111)    water = initial; the increment of every step_ended, initial.abs().multiply(rain_speed), is
//       constant over the phase and kept: per level (|x| as f64 * rain_speed).round() as i64 (score/macros.rs:61-63, bendable.rs:142-152) --
//       one f64 multiply, round half away from zero, the cast saturates and maps NaN to 0, as in dla_threshold.  |INT64_MIN| wraps.
//   StepCounting (step_counting.rs:101-104)   best = initial, since = 0
__device__ __forceinline__ void acceptor_phase_started(int acceptor, const int64_t* initial, uint64_t* ax_row) {
    if (acceptor != 5 && acceptor != 6) return;
    double rain_speed;
    __builtin_memcpy(&rain_speed, &ax_row[AX_PARAM], 8);
    for (int k = 0; k < 4; ++k) {
        const int64_t a = initial[k] < 0 ? wsub(0, initial[k]) : initial[k];
        ax_row[AX_LEVEL + k] = (uint64_t)initial[k];
        ax_row[AX_INCR + k] = acceptor == 5 ? (uint64_t)f64_as_i64(__builtin_round((double)a * rain_speed)) : 0u;
    }
    ax_row[AX_SINCE] = 0;
}

// acceptor.step_ended(last_step_score), always (step.rs:216-221), by the one lane `writer`: the LateAcceptance history slot of the step
// takes the score; DiversifiedLateAcceptance keeps the phase's best step score (diversified_late_acceptance.rs:161-170)
template <int L>
__device__ __forceinline__ void acceptor_step_ended(int acceptor, bool writer, const int64_t* cur, int64_t* la_row, int64_t* dla_row) {
    if ((acceptor == 1 || acceptor == 4) && writer) {
#pragma unroll
        for (int k = 0; k < L; ++k) la_row[k] = cur[k];
    }
    if (acceptor == 4 && writer) {
        if (score_cmp<L>(score_of<L>(cur), score_of<L>(dla_row)) > 0) {
#pragma unroll
            for (int k = 0; k < L; ++k) dla_row[k] = cur[k];
        }
    }
}
// ... of acceptors 5 and 6: GreatDeluge's water rises by its increment (great_deluge.rs:113-123; the sum wraps); StepCounting resets its
// count when the step score beats its best strictly and counts the step otherwise (step_counting.rs:106-123)
template <int L>
__device__ __forceinline__ void ax_step_ended(int acceptor, bool writer, const int64_t* cur, uint64_t* ax_row) {
    if (acceptor == 5 && writer) {
#pragma unroll
        for (int k = 0; k < L; ++k) ax_row[AX_LEVEL + k] = (uint64_t)wadd((int64_t)ax_row[AX_LEVEL + k], (int64_t)ax_row[AX_INCR + k]);
    }
    if (acceptor == 6 && writer) {
        ScoreV<L> b;
#pragma unroll
        for (int k = 0; k < L; ++k) b.v[k] = (int64_t)ax_row[AX_LEVEL + k];
        if (score_cmp<L>(score_of<L>(cur), b) > 0) {
#pragma unroll
            for (int k = 0; k < L; ++k) ax_row[AX_LEVEL + k] = (uint64_t)cur[k];
            ax_row[AX_SINCE] = 0;
        } else {
            ax_row[AX_SINCE] += 1;
        }
    }
}

// ---- Variable Neighborhood Descent -------------------------------------------------------------------------------------------------
// k = 0 at phase start (phase.rs:48); the host wrote n.  A phase without a neighbourhood is done before its first step (`while k < n`).
__device__ __forceinline__ void vnd_phase_started(int acceptor, uint64_t* vnd_row) {
    if (acceptor != VND_KIND) return;
    vnd_row[VND_K] = 0;
    vnd_row[VND_DONE] = vnd_row[VND_N] == 0 ? 1 : 0;
    vnd_row[VND_IDLE] = 0;
}
// The neighbourhood of this step and whether the phase has ended for the replica, wave-uniform (phase.rs:58: `while k < n`)
__device__ __forceinline__ void vnd_step_begin(const uint64_t* vnd_row, uint32_t& k, bool& done) {
    k = uni((uint32_t)vnd_row[VND_K]);
    done = uni((uint32_t)vnd_row[VND_DONE]) != 0;
}
// A candidate that reaches the comparison (`consult`: doable and not held back by a requires_*_improvement gate, phase.rs:279-333) is a
// possible pick when it beats the current score strictly (:339).  Among those the step keeps the first strictly best one (:340-357): the
// BestScore pick without random ties.
template <int L>
__device__ __forceinline__ bool vnd_accepts(bool consult, const ScoreV<L>& sc, const ScoreV<L>& cur) {
    return consult && score_cmp<L>(sc, cur) > 0;
}
// Found: k = 0 (phase.rs:132).  Not found: k += 1 (:136), and the step counts among the idle ones.  By the one lane `writer`.
__device__ __forceinline__ void vnd_step_ended(uint64_t* vnd_row, bool writer, bool applied) {
    if (!writer) return;
    const uint64_t k = applied ? 0 : vnd_row[VND_K] + 1;
    vnd_row[VND_K] = k;
    vnd_row[VND_DONE] = k >= vnd_row[VND_N] ? 1 : 0;
    if (!applied) vnd_row[VND_IDLE] += 1;
}

}  // namespace sf
#endif  // __HIPCC__
