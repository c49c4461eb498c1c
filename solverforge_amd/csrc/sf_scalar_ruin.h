// Scalar ruin-and-recreate leaf of the generic N-leaf engine (one wavefront = one replica): MoveSelectorConfig::RuinRecreateMoveSelector
// (solverforge-config/src/move_selector.rs:53-54,299-328), the large-neighbourhood leaf of the scalar class.
//
// Reference semantics restated (paths under crates/solverforge-solver/src/):
//   heuristic/selector/scalar_neighborhood/spec.rs:122-139      1 <= min_ruin_count <= max_ruin_count, moves_per_step.unwrap_or(10).max(1),
//                                                               value_candidate_limit, FirstFit (default) or CheapestInsertion
//   heuristic/selector/scalar_neighborhood/cursor.rs:234-256    ONE SmallRng per solve, seeded from scoped_seed(random_seed, descriptor,
//                                                               variable, "scalar_ruin_recreate_move_selector"); every cursor open draws from
//                                                               it directly (no per-cursor stream, no offset seed)
//   scalar_neighborhood/cursor.rs:144-175, cursor/ruin.rs:13-48 cursor open: moves_per_step batches -- identity permutation, ruin count
//                                                               (no draw when min == max), partial Fisher-Yates, the first ruin_count entries
//                                                               in swap order -- then apply_selection_order(0x5CA1_A2C0_7A11_0001 ^ slot)
//   move_selector/iter.rs:149-157                               apply_selection_order: ordered[i] = drawn[selection_index(i, n, salt)]
//   scalar_neighborhood/cursor/ruin.rs:87-141                   emission against the snapshot taken at open: some entity assigned, and (the
//                                                               variable allows unassigned or every assigned entity has a candidate value)
//   scalar_neighborhood/move/apply.rs:66-90,156-172,337-450     the move: unassign the batch in order, then place every entity in order --
//                                                               FirstFit: the first legal value strictly above the baseline (no baseline: the
//                                                               first legal one); CheapestInsertion: the strictly best, first ordinal of
//                                                               equals, taken when >= the baseline.  The baseline is the score before the
//                                                               placement and exists only when the variable allows unassigned
//   phase/localsearch/evaluation.rs:52-60                       the candidate's score is the score after the recreate; one score
//                                                               calculation per candidate
// rand's xoshiro256++ / random_range are not in the reference tree: restated from the published algorithm, unpinned against the crate, pinned
// between the oracle (oracle/sfo_core.hpp) and the device through sf_ruin.h's SaRng / ruin_random_range, which this leaf shares.
//
// GPU formulation.  The reference scores a candidate by a chain of do / score / undo round trips, one per candidate value of every ruined
// entity.  Here every placement of the chain lays the entity's candidate values onto the lanes, 64 at a time, and each lane prices its
// value with the engine's own eval_scalar_move + apply_scalar_delta against the working state of the chain (values, per-value tables,
// running score, running load statistic); a ballot (first fit) or a lexicographic wave maximum (cheapest insertion) picks, lane 0 commits
// through scalar_tables_apply, and the next placement sees it.  The unassignments run through the same code with the one candidate "none".
// After the last placement the old values go back through the same table update: integer adds and subtracts, so the replica's state is
// bit-identical before and after a trial.  A committed candidate re-applies the result values the trial recorded.
//
// Every loop is bounded by data: <= 16 batches, <= 8 entities, ceil(candidates / 64) chunks; none waits on another wave.
#pragma once
#include <stdint.h>

namespace sf {

constexpr uint64_t SALT_SRUIN_ORDER = 0x5CA1A2C07A110001ULL;  // scalar_neighborhood/cursor.rs:160
constexpr uint32_t SRUIN_MAX_COUNT = 8;                       // entities per batch (reference default 2..=5)
constexpr uint32_t SRUIN_MAX_MOVES = 16;                      // moves_per_step (reference default 10)
// the table as sf_get_scalar_ruin_table reads it: counts[16], entities[16][8], values[16][8], emitted[16], replica, written flag
constexpr int SRUIN_TAB_CNT = 0, SRUIN_TAB_ENT = 16, SRUIN_TAB_VAL = 16 + 128, SRUIN_TAB_EMIT = 16 + 256, SRUIN_TAB_REPLICA = 32 + 256;
constexpr int SRUIN_TAB_WORDS = SRUIN_TAB_REPLICA + 2;

// Per-replica LDS block of the leaf (GCarve reserves it only when the union holds the leaf).  Entity indices are 32-bit words throughout.
struct SRuinLds {
    static constexpr size_t bytes = 4 * 8 + SRUIN_MAX_MOVES * 4 * 8 + 2 * SRUIN_MAX_MOVES * SRUIN_MAX_COUNT * 4 + 2 * SRUIN_MAX_MOVES * 4 + SRUIN_MAX_COUNT * 4;
    static_assert(bytes == SRUIN_LDS_BYTES, "GCarve reserves SRUIN_LDS_BYTES");
    uint64_t* prng;  // [4] per-solve stream (loaded at launch start, stored at launch end)
    int64_t* score;  // [16][4] trial score of every emitted batch
    uint32_t* ent;   // [16][8] batches in cursor order
    int32_t* val;    // [16][8] the value the recreate gave every entity (-1 = left unassigned); during the cursor open: the batches as drawn
    uint32_t* cnt;   // [16]
    uint32_t* emit;  // [16] the cursor emits the batch; during the cursor open: the counts as drawn
    int32_t* old;    // [8] old values of the batch on trial
    __device__ explicit SRuinLds(unsigned char* base) {
        prng = (uint64_t*)base;
        score = (int64_t*)(prng + 4);
        ent = (uint32_t*)(score + SRUIN_MAX_MOVES * 4);
        val = (int32_t*)(ent + SRUIN_MAX_MOVES * SRUIN_MAX_COUNT);
        cnt = (uint32_t*)(val + SRUIN_MAX_MOVES * SRUIN_MAX_COUNT);
        emit = cnt + SRUIN_MAX_MOVES;
        old = (int32_t*)(emit + SRUIN_MAX_MOVES);
    }
};

// visit_candidate_values: the first `limit` values of the entity's canonical list (the range 0..n_values, or its value list)
__device__ __forceinline__ uint32_t sruin_candidate_count(const SRuinParams& rp, const ScalarModel& sm, uint32_t e) {
    const uint32_t len = value_count(sm, e);
    return (rp.limit >= 0 && (uint32_t)rp.limit < len) ? (uint32_t)rp.limit : len;
}
__device__ __forceinline__ int32_t sruin_candidate(const ScalarModel& sm, uint32_t e, uint32_t k) {
    return sm.vl_off ? sm.vl[sm.vl_off[e] + k] : (int32_t)k;
}

// Cursor open, once per step: draws the step's batches from the per-solve stream (a dry run peeks without consuming), orders them, and
// computes the emission flags against the step snapshot.  Returns the number of emitted batches.
template <class VT>
__device__ __forceinline__ uint32_t sruin_open_cursor(const SRuinParams& rp, const SRuinLds& sl, const ScalarModel& sm, const VT* vals, const StreamCtx& ctx,
                                                      uint64_t identity, bool advance, uint32_t lane) {
    SaRng g{uni64(sl.prng[0]), uni64(sl.prng[1]), uni64(sl.prng[2]), uni64(sl.prng[3])};
    const uint32_t n = (uint32_t)sm.n, mps = (uint32_t)rp.moves_per_step;
    const uint32_t mn = (uint32_t)rp.min_count < n ? (uint32_t)rp.min_count : n, mx = (uint32_t)rp.max_count < n ? (uint32_t)rp.max_count : n;
    uint32_t* draw = (uint32_t*)sl.val;
    for (uint32_t b = 0; b < mps; ++b) {  // generate_ruin_batches (cursor/ruin.rs:13-48)
        uint32_t cnt = 0, mine = 0;
        if (n != 0) {
            cnt = mn == mx ? mn : uni(ruin_random_range(g, mn, mx));
            // partial Fisher-Yates of the identity kept sparse (as ruin_next_candidate): lane t < n_ov holds one displaced entry (position, value)
            uint32_t ov_pos = 0, ov_val = 0, n_ov = 0;
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint32_t j = uni(ruin_random_range(g, i, n - 1u));
                const uint64_t mi = __ballot(lane < n_ov && ov_pos == i);
                const uint32_t vi = mi ? uni((uint32_t)__shfl((int)ov_val, __ffsll((unsigned long long)mi) - 1)) : i;
                const uint64_t mj = __ballot(lane < n_ov && ov_pos == j);
                const uint32_t vj = mj ? uni((uint32_t)__shfl((int)ov_val, __ffsll((unsigned long long)mj) - 1)) : j;
                const uint32_t slot = mj ? (uint32_t)(__ffsll((unsigned long long)mj) - 1) : n_ov;
                if (lane == slot) ov_pos = j, ov_val = vi;
                if (!mj) n_ov += 1;
                if (lane == i) mine = vj;  // permutation[i] after the swap
            }
        }
        if (lane < SRUIN_MAX_COUNT) draw[b * SRUIN_MAX_COUNT + lane] = lane < cnt ? mine : 0u;
        if (lane == 0) sl.emit[b] = cnt;
    }
    if (lane == 0 && advance) sl.prng[0] = g.s0, sl.prng[1] = g.s1, sl.prng[2] = g.s2, sl.prng[3] = g.s3;
    wave_sync();
    // apply_selection_order: entry `lane` and entry `lane + 64` of the ordered table, the ordered counts in lanes 0..15
    const uint64_t salt = SALT_SRUIN_ORDER ^ identity;
    const uint32_t i0 = lane >> 3, k = lane & 7u;
    uint32_t e0 = 0, e1 = 0, c = 0;
    if (i0 < mps) e0 = draw[ctx.selection_index(i0, mps, salt) * SRUIN_MAX_COUNT + k];
    if (i0 + 8u < mps) e1 = draw[ctx.selection_index(i0 + 8u, mps, salt) * SRUIN_MAX_COUNT + k];
    if (lane < mps) c = sl.emit[ctx.selection_index(lane, mps, salt)];
    wave_sync();
    sl.ent[lane] = e0, sl.ent[lane + 64u] = e1;
    sl.val[lane] = -1, sl.val[lane + 64u] = -1;
    if (lane < SRUIN_MAX_MOVES) sl.cnt[lane] = c;
    wave_sync();
    // emission (cursor/ruin.rs:87-141): one ballot for "assigned", one for "assigned without a candidate value under the limit"
    uint32_t n_emit = 0;
    for (uint32_t b = 0; b < SRUIN_MAX_MOVES; ++b) {
        const uint32_t cnt = b < mps ? uni(sl.cnt[b]) : 0u;
        bool assigned = false, stuck = false;
        if (lane < cnt) {
            const uint32_t e = sl.ent[b * SRUIN_MAX_COUNT + lane];
            assigned = (int32_t)vals[e] >= 0;
            stuck = assigned && sruin_candidate_count(rp, sm, e) == 0u;
        }
        const uint64_t am = __ballot(assigned), sm_ = __ballot(stuck);
        const bool emitted = am != 0ull && (sm.allows_unassigned != 0 || sm_ == 0ull);
        if (lane == 0) sl.emit[b] = emitted ? 1u : 0u;
        n_emit += emitted ? 1u : 0u;
    }
    wave_sync();
    return uni(n_emit);
}

// One step of the chain committed into the working state by every lane alike (wave-uniform arguments): the running load statistic is
// shifted as eval_scalar_move_v shifts it (read BEFORE the tables change), then lane 0 updates the tables and the value.
template <class VT>
__device__ __forceinline__ void sruin_commit_change(const ScalarModel& sm, VT* vals, uint32_t* t_cnt, int64_t* t_sum, bool tables, int64_t* lb, uint32_t e,
                                                    int32_t v, uint32_t lane) {
    const int32_t old = (int32_t)vals[e];
    if (tables && sm.grp_level >= 0 && sm.grp_mode >= 1) {
        const bool by_count = sm.grp_mode == 2;
        const int64_t sz = by_count ? 1 : (int64_t)sm.size[e];
        int64_t s1 = lb[0], s2 = lb[1];
        uint32_t nk = (uint32_t)lb[2];
        if (old >= 0) {
            lb_shift(s1, s2, by_count ? (int64_t)t_cnt[old] : t_sum[old], -sz);
            nk -= t_cnt[old] == 1u ? 1u : 0u;
        }
        if (v >= 0) {
            lb_shift(s1, s2, by_count ? (int64_t)t_cnt[v] : t_sum[v], sz);
            nk += t_cnt[v] == 0u ? 1u : 0u;
        }
        lb[0] = s1, lb[1] = s2, lb[2] = (int64_t)nk, lb[3] = global_stat(sm, s1, s2, nk);
    }
    wave_sync();  // every lane has read the old value and the tables
    if (lane == 0) {
        if (tables) scalar_tables_apply(sm, vals, 0, e, 0u, v, t_cnt, t_sum);
        vals[e] = (VT)v;
    }
    wave_sync();
}

// Trial of batch b: ruin, chained recreate, score and result values into the table, then the old values back.  `lb_step` = the step's
// (S1, S2, keys, statistic); `cur` = the step's score.  `priced` counts the lanes priced (candidates_scored).
template <int L, class VT>
__device__ __forceinline__ void sruin_trial(const SRuinParams& rp, const SRuinLds& sl, const ScalarModel& sm_step, VT* vals, uint32_t* t_cnt, int64_t* t_sum, bool tables,
                                            const int64_t* lb_step, const int64_t* cur, uint32_t b, uint32_t lane, uint32_t& priced) {
    ScalarModel sm = sm_step;
    sm.allows_unassigned = 1;  // the ruin unassigns whatever the variable allows (apply_one(.., None), apply.rs:349-352)
    const bool baseline_on = sm_step.allows_unassigned != 0;
    const uint32_t cnt = uni(sl.cnt[b]);
    const uint32_t* ents = sl.ent + (size_t)b * SRUIN_MAX_COUNT;
    int64_t lb[4] = {lb_step[0], lb_step[1], lb_step[2], lb_step[3]};
    ScoreV<L> run;
#pragma unroll
    for (int q = 0; q < L; ++q) run.v[q] = cur[q];
    if (lane < cnt) sl.old[lane] = (int32_t)vals[ents[lane]];
    wave_sync();
    // ops 0 .. cnt-1 unassign the batch in order (one candidate, "none", always taken); ops cnt .. 2 cnt-1 place the entities in order
    for (uint32_t op = 0; op < 2u * cnt; ++op) {
        const bool ruin = op < cnt;
        const uint32_t i = ruin ? op : op - cnt;
        const uint32_t e = uni(ents[i]);
        if (ruin && (int32_t)uni((uint32_t)(int32_t)vals[e]) < 0) continue;  // already unassigned: nothing changes
        const uint32_t len = ruin ? 1u : uni(sruin_candidate_count(rp, sm, e));
        const bool first_fit = ruin || rp.heuristic == 0;
        const bool need_above = !ruin && baseline_on;  // first fit: strictly above the score before the placement
        bool select = false;
        uint32_t best_k = 0;
        ScoreV<L> best_sc = run;
        for (uint32_t base = 0; base < len; base += 64u) {
            const uint32_t k = base + lane;
            const bool valid = k < len;
            const int32_t v = ruin ? -1 : sruin_candidate(sm, e, valid ? k : len - 1u);
            const ScalarDelta d = eval_scalar_move(sm, vals, 0, e, 0u, v, tables ? t_cnt : nullptr, tables ? t_sum : nullptr, tables ? lb : nullptr);
            const ScoreV<L> sc = apply_scalar_delta<L>(sm, run.v, d);
            const bool ok = valid && d.doable;  // change_is_legal: a value of the entity's own list
            if (!ruin) priced += 64u;
            if (first_fit) {
                const uint64_t hit = __ballot(ok && (!need_above || score_cmp<L>(sc, run) > 0));
                if (hit) {
                    const int sel = __ffsll((unsigned long long)hit) - 1;
                    select = true, best_k = base + (uint32_t)sel;
#pragma unroll
                    for (int q = 0; q < L; ++q) best_sc.v[q] = (int64_t)uni64(shfl_u64((uint64_t)sc.v[q], sel));
                    break;
                }
            } else if (__ballot(ok)) {  // the strictly best, the lowest ordinal of equals within and across chunks
                const ScoreV<L> M = wave_max_score<L>(sc, ok);
                if (!select || score_cmp<L>(M, best_sc) > 0) {
                    const uint64_t eq = __ballot(ok && score_cmp<L>(sc, M) == 0);
                    select = true, best_k = base + (uint32_t)__ffsll((unsigned long long)eq) - 1u;
#pragma unroll
                    for (int q = 0; q < L; ++q) best_sc.v[q] = (int64_t)uni64((uint64_t)M.v[q]);
                }
            }
        }
        if (!first_fit && select && baseline_on && score_cmp<L>(best_sc, run) < 0) select = false;  // cheapest insertion: taken when >= the baseline
        int32_t chosen = -1;
        if (select) {
            chosen = ruin ? -1 : (int32_t)uni((uint32_t)sruin_candidate(sm, e, best_k));
            sruin_commit_change(sm, vals, t_cnt, t_sum, tables, lb, e, chosen, lane);
            run = best_sc;
        }
        if (!ruin && lane == 0) sl.val[(size_t)b * SRUIN_MAX_COUNT + i] = chosen;
    }
    wave_sync();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sl.score[(size_t)b * 4 + q] = q < L ? run.v[q] : 0;
        for (uint32_t i = 0; i < cnt; ++i) {  // undo: the old values back (integer table updates: the state is what it was before the trial)
            const uint32_t e = ents[i];
            const int32_t o = sl.old[i];
            if ((int32_t)vals[e] != o) {
                if (tables) scalar_tables_apply(sm, vals, 0, e, 0u, o, t_cnt, t_sum);
                vals[e] = (VT)o;
            }
        }
    }
    wave_sync();
}

// The picked candidate: the result values of its trial in batch order, through the same unassign-then-assign path.
template <class VT>
__device__ __forceinline__ void sruin_commit(const SRuinLds& sl, const ScalarModel& sm, VT* vals, uint32_t* t_cnt, int64_t* t_sum, bool tables, uint32_t b, uint32_t lane) {
    if (lane == 0) {
        const uint32_t cnt = sl.cnt[b];
        const uint32_t* ents = sl.ent + (size_t)b * SRUIN_MAX_COUNT;
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t e = ents[i];
            if ((int32_t)vals[e] < 0) continue;
            if (tables) scalar_tables_apply(sm, vals, 0, e, 0u, -1, t_cnt, t_sum);
            vals[e] = (VT)-1;
        }
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t e = ents[i];
            const int32_t v = sl.val[(size_t)b * SRUIN_MAX_COUNT + i];
            if (v < 0) continue;
            if (tables) scalar_tables_apply(sm, vals, 0, e, 0u, v, t_cnt, t_sum);
            vals[e] = (VT)v;
        }
    }
    wave_sync();
}

}  // namespace sf
