// The replay batch of k_list_search_wave's SMALL kernels (sf_list_wave.hip), as statements: included inside the kernel, once in the general loop
// and once in the lockstep round (DESIGN 28) -- a text fragment for the reason given in sf_wave_pair_pass.inc.  The including scope holds
//   in   lf, idx      this lane's leaf and ring entry          valid, nvalid   the lane holds a candidate; how many lanes do (the round: a literal
//                                                                              true and 64 -- every select on `valid` and the stand-in entry fold away)
//   out  m0, m1, doable, acc, consumed, accmask, nconsumed     (declared by the includer; nconsumed starts at nvalid)
// and the step's forager state, `accepted`, `done` and st_scored, which the batch updates in place.
// ---- delta-space replay (MODE 2): int32 level deltas against the step's current score ----
// Every ring entry of a FAST kernel is a nearby candidate generated from the committed lists of THIS step: structurally doable
// (eval_generated_small), so there is no doability test, and no exec-mask region either -- a lane past the valid ones re-prices
// the batch's first candidate and is masked out of the decisions.
int32_t dv[L];
{
    const uint32_t lf0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lf), idx0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
    const uint32_t lfq = valid ? lf : lf0;
    const uint32_t qi = (valid ? idx : idx0) & RCM;
    const uint32_t* rq = ring + ((size_t)lfq * cv.rc + qi) * 2;
    m0 = rq[0];
    m1 = rq[1];
    const uint32_t a = m0 >> 16, i = m0 & 0xFFFFu, b = m1 >> 16, j = m1 & 0xFFFFu;
    eval_generated_small<L, LT, COMPACT, OT, RBATCH>(m, lvl, s_visits, s_off, s_load, 1u - lfq, a, i, b, j, dv);  // FAST: leaf 0 = change, leaf 1 = swap; COMPACT reads the u16 matrix
}
doable = valid;
// LateAcceptance: score >= last step score || score >= late score (late_acceptance.rs:89-125).  Two levels: the pair of int32 deltas
// is ONE signed 64-bit key (hard x 2^32 + soft, |soft| < 2^31 keeps the order lexicographic), and the two tests are one compare
// against the wave-uniform min(0, late - current)
int64_t key = 0;
if constexpr (L == 2) {
    key = (int64_t)(((uint64_t)(uint32_t)dv[0] << 32) + (uint64_t)(int64_t)dv[1]);
    acc = valid && key >= acc_thr;
} else {
    acc = valid && (small_ge0<L>(dv) || small_ge<L>(dv, late_d));
}
accmask = __ballot(acc);
// AcceptedCount quota (forager.rs:232-239): the step ends at the lane whose accepted candidate is the limit-th.  That lane exists
// only in a batch with at least `remaining` accepted lanes -- the step's last one, one batch in ten at the default limit -- so one
// wave-uniform compare on the batch's count (formed for `accepted` anyway) stands in front of the prefix count, the second
// ballot and the re-masking; every other batch consumes its nvalid lanes, and `acc` (valid lanes only) is final as it stands.
// `>=`: 64 accepted lanes with exactly 64 remaining do cut, at lane 63.  The same compare IS the forager's quit test.  Precondition:
// FAST implies forager == FORAGER_ACCEPTED_COUNT (host-checked), whose forager_quits is `accepted >= limit`, and the host keeps
// p.limit >= 1 for it; `accepted` never passes the limit.  A batch with at least `remaining` accepted lanes always holds the
// limit-th accepted lane, so the cut fires in it, `accepted` becomes `limit` and the step ends; a batch with fewer leaves
// `accepted` below the limit.  Cut and quit coincide: the step's end is decided here, not a second time at the batch's end.
consumed = valid;
if (!RBATCH || (uint32_t)__popcll(accmask) >= (uint32_t)SF_SPEC_LIMIT(p.limit) - accepted) {
    const uint32_t remaining = (uint32_t)SF_SPEC_LIMIT(p.limit) - accepted;
    const uint32_t pre = mbcnt64(accmask) + (acc ? 1u : 0u);
    const uint64_t cutmask = __ballot(acc && pre == remaining);
    nconsumed = cutmask ? (uint32_t)__ffsll((unsigned long long)cutmask) : nvalid;
    consumed = lane < nconsumed;
    acc = acc && consumed;
    accmask = __ballot(acc);
    if constexpr (RBATCH) {
        st_scored += nvalid - nconsumed;  // scored but not consumed (candidates_scored is added once per step, from `pulls`)
        done = 1;
    }
}
bool challenger;
if constexpr (L == 2)
    challenger = acc && key >= best_key;
else
    challenger = acc && small_ge<L>(dv, best_d);
if (accmask && (!has_best || __ballot(challenger))) {
    // lexicographic maximum of the accepted lanes, level by level
    int32_t M[L];
    bool in_max = acc;
#pragma unroll
    for (int kk = 0; kk < L; ++kk) {
        M[kk] = wave_max_i32(in_max ? dv[kk] : (int32_t)0x80000000);
        in_max = in_max && dv[kk] == M[kk];
    }
    // (two levels: the forager's best is best_key alone -- best_d[] would be the same value a second time in two more registers)
    int64_t Mkey = 0;
    if constexpr (L == 2) Mkey = (int64_t)(((uint64_t)(uint32_t)M[0] << 32) + (uint64_t)(int64_t)M[1]);
    bool ge, gt;
    if constexpr (L == 2) {
        ge = !has_best || Mkey >= best_key;
        gt = !has_best || Mkey > best_key;
    } else {
        ge = !has_best || small_ge<L>(M, best_d);
        gt = !has_best || !small_ge<L>(best_d, M);
    }
    if (ge) {
        const bool newmax = gt;
        const uint32_t eq_base = newmax ? 0u : equal_count;
        const uint64_t eq = __ballot(in_max);
        const uint32_t rank = mbcnt64(eq) + 1u;
        const uint64_t cntq = (uint64_t)(eq_base + rank);
        const bool pick = in_max && ((newmax && rank == 1) ||
                                     (p.random_ties && cntq > 1 && reservoir_pick(sseed, cntq)));
        const uint64_t pm = __ballot(pick);
        if (pm) {
            const int sel = 63 - __clzll((unsigned long long)pm);
            best_m0 = __shfl(m0, sel);
            best_m1 = __shfl(m1, sel);
            best_leaf = (int)__shfl(lf, sel);
        }
        if constexpr (L == 2) {
            best_key = Mkey;
        } else {
#pragma unroll
            for (int kk = 0; kk < L; ++kk) best_d[kk] = M[kk];
        }
        equal_count = eq_base + (uint32_t)__popcll(eq);
        has_best = 1;
    }
}
