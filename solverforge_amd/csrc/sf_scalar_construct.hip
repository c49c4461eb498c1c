// Construction heuristics of the scalar class on the device (sf_construct_scalar), gfx950 wave64.
//
// Reference semantics restated (paths under crates/solverforge-solver/src/phase/construction/ unless noted):
//   runtime_slots/placement.rs:73-147,174-227,307-368   heuristic -> entity order, value order, forager, live refresh; the placement cursor
//   placer/queued.rs:242-295                            an assigned entity / an entity without values is skipped
//   forager_step.rs:149-332,463-625, decision.rs:50-154 first fit, best fit, weakest / strongest fit; the keep-current baseline
//   phase/selection.rs:14-86, frontier.rs:32-50, scope/solver/scope_progress.rs:590-606   commit, completion at the solution revision
//   phase/phase_type.rs:74-149                          one step per placement, kept or assigned
//
// One wavefront = one replica.  The replica's values stay in HBM (a class of 100,000 rows does not fit a wave's LDS slice; a trial reads
// deg(e) of them through the vector L1); the per-value tables and the runs / presence table are in LDS, built once and updated at each
// commit.  One placement lays the entity's ordered candidate values on the lanes, 64 at a time, and every lane prices its candidate with the
// search engines' own eval_scalar_move + apply_scalar_delta.  The counters are those of the sequential phase (they come from the chosen
// ordinal, never from the chunk width).
//
// Live refresh: after every step the reference reopens the cursor at the head of the order and skips the assigned entities and the
// entities that kept current at the CURRENT solution revision.  A commit advances the revision, so it reopens exactly the kept entities
// before the frontier, in order.  Here those sit in a per-replica list that is retried from its start after every assignment: the same
// sequence of placements without the walk over the assigned prefix.
//
// Every loop is bounded: the frontier only advances (<= n_order / 64 + 1 scans), a chunk loop runs ceil(candidates / 64) times, and the
// placement loop carries its own budget -- n_order steps in one pass, n_order (n_order + 1) with live refresh (an assignment is followed
// by at most one retry of every kept entity).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_scalar_construct.h"
#include "sf_scalar_kernels.hip"

namespace sf {

__device__ __forceinline__ int64_t construct_wave_extreme(int64_t x, bool want_max) {
#pragma unroll
    for (int mlane = 32; mlane >= 1; mlane >>= 1) {
        const int64_t o = (int64_t)shfl_xor_u64((uint64_t)x, mlane);
        x = want_max ? (o > x ? o : x) : (o < x ? o : x);
    }
    return x;
}

// candidate values of entity e after the cut (visit_candidate_values: the canonical list's first `limit` values)
__device__ __forceinline__ uint32_t construct_candidate_count(const ScalarConstructArgs& a, uint32_t e) {
    if (!a.c_off) return (uint32_t)a.range_n;
    const uint32_t len = a.c_off[e + 1] - a.c_off[e];
    return len < a.limit ? len : a.limit;
}
__device__ __forceinline__ int32_t construct_candidate(const ScalarConstructArgs& a, uint32_t e, uint32_t k) {
    if (a.c_off) return a.c_val[a.c_off[e] + k];
    return a.perm ? a.perm[k] : (int32_t)k;
}

__global__ __launch_bounds__(64) void k_scalar_construct(ScalarModel m, ScalarConstructArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tab_mem[];
    __shared__ int64_t s_lb[4];
    constexpr int L = 4;  // scores padded with zero levels: the lexicographic order is unchanged
    const uint32_t lane = threadIdx.x & 63u;
    const int r = (int)blockIdx.x;
    int32_t* vals = m.vals + (size_t)r * m.n;
    int64_t* t_sum = (int64_t*)tab_mem;
    uint32_t* t_cnt = (uint32_t*)(tab_mem + sizeof(int64_t) * (size_t)m.n_values);
    const bool tables = m.tables();
    const bool global_stat_on = m.grp_level >= 0 && m.grp_mode >= 1;
    if (tables) {
        for (int v = (int)lane; v < m.n_values; v += 64) {
            t_sum[v] = 0;
            t_cnt[v] = 0;
        }
        wave_sync();
        scalar_tables_accumulate(m, vals, lane, 64u, t_cnt, t_sum);
        wave_sync();
    }
    if (lane == 0) {
        s_lb[0] = s_lb[1] = s_lb[2] = s_lb[3] = 0;
        if (global_stat_on) lb_from_tables(m, t_cnt, t_sum, s_lb);
    }
    wave_sync();
    ScoreV<L> cur;
#pragma unroll
    for (int k = 0; k < L; ++k) cur.v[k] = m.score[(size_t)r * 4 + k];

    const uint32_t n_order = (uint32_t)a.n_order;
    uint32_t* kept = a.kept ? a.kept + (size_t)r * (size_t)m.n : nullptr;
    uint32_t n_kept = 0, kr = 0, pos = 0;
    bool retry = false;
    uint64_t st_steps = 0, st_pulled = 0, st_calc = 0, st_assigned = 0, st_not_doable = 0, st_priced = 0;
    const bool want_max = a.forager == SCF_STRONGEST_FIT;
    const uint64_t budget = a.live_refresh ? (uint64_t)n_order * ((uint64_t)n_order + 1ull) : (uint64_t)n_order;

    for (uint64_t step = 0; step < budget; ++step) {
        // ---- next placement: a kept entity reopened by the last assignment, else the next unassigned entity with values at the frontier
        uint32_t e;
        const bool from_kept = retry && kr < n_kept;
        if (from_kept) {
            e = uni(kept[kr]);
        } else {
            retry = false;
            bool found = false;
            while (pos < n_order) {
                const uint32_t t = pos + lane;
                bool open = false;
                if (t < n_order) {
                    const uint32_t et = a.order ? a.order[t] : t;
                    open = vals[et] < 0 && construct_candidate_count(a, et) > 0;
                }
                const uint64_t mask = __ballot(open);
                if (mask) {
                    pos += (uint32_t)__ffsll((unsigned long long)mask) - 1u;
                    found = true;
                    break;
                }
                pos += 64u;
            }
            if (!found) break;
            e = uni(a.order ? a.order[pos] : pos);
        }
        const uint32_t len = uni(construct_candidate_count(a, e));

        // ---- the forager: chosen ordinal (or keep current), the counters of the sequential scan
        bool select = false, scored = false;
        uint32_t best_k = 0;
        ScoreV<L> best_sc = cur;
        if (a.forager == SCF_FIRST_FIT && !a.baseline) {  // the first doable candidate, unscored (forager_step.rs:197-206)
            uint32_t pulled = len;
            for (uint32_t base = 0; base < len; base += 64u) {
                const uint32_t k = base + lane;
                const bool valid = k < len;
                const int32_t v = construct_candidate(a, e, valid ? k : len - 1u);
                const bool doable = valid && v >= 0 && v < m.n_values;
                const uint64_t hit = __ballot(doable);
                if (hit) {
                    const uint32_t sel = (uint32_t)__ffsll((unsigned long long)hit) - 1u;
                    select = true, best_k = base + sel, pulled = best_k + 1u;
                    st_not_doable += sel;
                    break;
                }
                st_not_doable += (uint64_t)__popcll(__ballot(valid));
            }
            st_pulled += pulled;
        } else if (a.forager == SCF_FIRST_FIT || a.forager == SCF_BEST_FIT) {
            uint32_t pulled = len;
            for (uint32_t base = 0; base < len; base += 64u) {
                const uint32_t k = base + lane;
                const bool valid = k < len;
                const int32_t v = construct_candidate(a, e, valid ? k : len - 1u);
                const ScalarDelta d = eval_scalar_move(m, vals, 0, e, 0u, v, t_cnt, t_sum, s_lb);
                const ScoreV<L> sc = apply_scalar_delta<L>(m, cur.v, d);
                const bool ok = valid && d.doable;
                const uint64_t okmask = __ballot(ok);
                st_priced += 64u;
                if (a.forager == SCF_FIRST_FIT) {  // strictly above the baseline, lowest ordinal (decision.rs:56-64)
                    const uint64_t hit = __ballot(ok && score_cmp<L>(sc, cur) > 0);
                    if (hit) {
                        const int sel = __ffsll((unsigned long long)hit) - 1;
                        const uint64_t upto = sel >= 63 ? ~0ull : ((1ull << (sel + 1)) - 1ull);
                        select = true, scored = true, best_k = base + (uint32_t)sel, pulled = best_k + 1u;
#pragma unroll
                        for (int q = 0; q < L; ++q) best_sc.v[q] = (int64_t)shfl_u64((uint64_t)sc.v[q], sel);
                        st_calc += (uint64_t)__popcll(okmask & upto);
                        st_not_doable += (uint64_t)(sel + 1) - (uint64_t)__popcll(okmask & upto);
                        break;
                    }
                } else if (okmask) {  // the strictly best trial score, the first of equals stays (forager_step.rs:300-309)
                    const ScoreV<L> M = wave_max_score<L>(sc, ok);
                    if (!select || score_cmp<L>(M, best_sc) > 0) {
                        const uint64_t eq = __ballot(ok && score_cmp<L>(sc, M) == 0);
                        select = true, scored = true, best_k = base + (uint32_t)__ffsll((unsigned long long)eq) - 1u;
#pragma unroll
                        for (int q = 0; q < L; ++q) best_sc.v[q] = (int64_t)uni64((uint64_t)M.v[q]);
                    }
                }
                st_calc += (uint64_t)__popcll(okmask);
                st_not_doable += (uint64_t)__popcll(__ballot(valid)) - (uint64_t)__popcll(okmask);
            }
            st_pulled += pulled;
            // best fit keeps current only when the baseline is strictly greater than every trial (decision.rs:114-143)
            if (a.forager == SCF_BEST_FIT && select && a.baseline && score_cmp<L>(cur, best_sc) > 0) select = false;
        } else {  // weakest / strongest fit: least / greatest strength among the doable candidates, first of equals; ONE trial
            int64_t best_key = 0;
            for (uint32_t base = 0; base < len; base += 64u) {
                const uint32_t k = base + lane;
                const bool valid = k < len;
                const int32_t v = construct_candidate(a, e, valid ? k : len - 1u);
                const bool ok = valid && v >= 0 && v < m.n_values;
                const uint64_t okmask = __ballot(ok);
                st_not_doable += (uint64_t)__popcll(__ballot(valid)) - (uint64_t)__popcll(okmask);
                if (!okmask) continue;
                const int64_t key = ok ? a.vkey[v] : (want_max ? INT64_MIN : INT64_MAX);
                const int64_t x = (int64_t)uni64((uint64_t)construct_wave_extreme(key, want_max));
                if (!select || (want_max ? x > best_key : x < best_key)) {
                    const uint64_t eq = __ballot(ok && key == x);
                    select = true, best_key = x, best_k = base + (uint32_t)__ffsll((unsigned long long)eq) - 1u;
                }
            }
            st_pulled += len;
            if (select && a.baseline) {  // scored once, taken only if strictly above the baseline (forager_step.rs:557-580)
                const ScalarDelta d = eval_scalar_move(m, vals, 0, e, 0u, construct_candidate(a, e, best_k), t_cnt, t_sum, s_lb);
                best_sc = apply_scalar_delta<L>(m, cur.v, d);
                scored = true;
                st_calc += 1;
                st_priced += 64u;
                select = score_cmp<L>(best_sc, cur) > 0;
            }
        }
        st_steps += 1;

        // ---- commit (selection.rs:23-47): the search kernels' own -- tables, value, score -- then the wave sees the new value
        if (select) {
            const int32_t v = (int32_t)uni((uint32_t)construct_candidate(a, e, best_k));
            wave_sync();
            if (lane == 0) {
                if (global_stat_on) {  // (S1, S2, keys, statistic) after the move, as eval_scalar_move_v shifts them
                    const bool by_count = m.grp_mode == 2;
                    int64_t s1 = s_lb[0], s2 = s_lb[1];
                    uint32_t nk = (uint32_t)s_lb[2];
                    lb_shift(s1, s2, by_count ? (int64_t)t_cnt[v] : t_sum[v], by_count ? 1 : (int64_t)m.size[e]);
                    nk += t_cnt[v] == 0 ? 1u : 0u;
                    s_lb[0] = s1, s_lb[1] = s2, s_lb[2] = (int64_t)nk, s_lb[3] = global_stat(m, s1, s2, nk);
                }
                if (tables) scalar_tables_apply(m, vals, 0, e, 0u, v, t_cnt, t_sum);
                vals[e] = v;
            }
            if (scored) cur = best_sc;  // the base of the next placement's trials; an unscored pick (no baseline) leaves it: trials of one placement share it
            st_assigned += 1;
            wave_sync();
            if (from_kept) {  // the entity leaves the kept list: the tail moves down one (ascending chunks, reads ahead of writes)
                for (uint32_t b = kr; b + 1u < n_kept; b += 64u) {
                    const uint32_t t = b + lane;
                    const bool in = t + 1u < n_kept;
                    const uint32_t x = in ? kept[t + 1u] : 0u;
                    wave_sync();
                    if (in) kept[t] = x;
                    wave_sync();
                }
                n_kept -= 1u;
            } else {
                pos += 1u;
            }
            if (a.live_refresh && n_kept > 0u) retry = true, kr = 0u;  // the new revision reopens every kept entity, from the head
        } else if (from_kept) {
            kr += 1u;  // kept again, at the current revision
        } else {
            if (kept) {
                if (lane == 0) kept[n_kept] = e;
                n_kept += 1u;
                wave_sync();
            }
            pos += 1u;
        }
    }

    // (the running score served the baselines only: the host commits the full recalculation, as after the list constructions)
    if (lane == 0) {
        if (a.stats) {
            uint64_t* gs = a.stats + (size_t)r * SF_STATS_WORDS;
            gs[0] += st_steps;     // one step per placement, kept or assigned (phase_type.rs:108-148)
            gs[1] += st_pulled;    // one generated + one evaluated per pulled candidate, not-doable ones included
            gs[2] += st_pulled;
            gs[3] += st_assigned;  // one accepted + one applied per selected candidate (selection.rs:32-41)
            gs[4] += st_assigned;
            gs[5] += st_calc;      // one score calculation per trial
            gs[6] += st_not_doable;
            gs[7] += st_priced;    // device work: lanes priced, the tail of a chunk included
        }
    }
}

hipError_t launch_tu_scalar_construct(const ScalarModel& m, const ScalarConstructArgs& a, int n_replicas, size_t lds, hipStream_t stream) {
    return launch_with_lds(k_scalar_construct, dim3((unsigned)n_replicas), dim3(64), lds, stream, m, a);
}

}  // namespace sf
